"""Batch shapes of the loss wrappers: the inputs, the blockwise long-double yardstick, the case tables and the launch-plan restatement
of tests/test_loss_batch_shapes_host.py and tests/test_gpu_loss_batch_shapes.py (test infrastructure; numpy and torch only -- the yardstick
imports nothing from the product package or the oracle; call_wrapper, the one function that makes the product's call, imports it when called).

compute_mmd / compute_scoring_rule / compute_expected_scoring_rule take the one-launch loss route by default (csrc/sk_loss.hip,
HipBackend.loss_forward, _SigKernelLoss): a pair layout of its own -- the rectangle K(X, [X; Y]), then the strict triangle of K(Y, Y),
from a table k_prep_cat decodes -- a reduction kernel of its own, an edge-keeping rule that stops at pair A (A + B) and an adjoint fed
from staged arrays with the upstream scalar as `gscale`.  The kernels' behaviour over values and path lengths is other files' business
(tests/value_regimes.py); the shapes here are the smallest that reach the BATCH-shape edges of that route: chunk counts of the finish
kernels below, at and beyond their lane split and batch, pair counts beyond the reduction's threads and its batched round, launches
whose lane-group chunks hold pairs of the rectangle AND of the triangle, launches that draw from the work counter.

Yardstick: loss_ld evaluates a loss in row blocks of X (16 rows at a time) with value_regimes.gram_ld -- the long-double solver and
analytic gradient the value-regime tests use -- and returns the scalar, dL/dX and the per-pair values in the one-launch route's order.
Tolerance: the suite's one rule, value_regimes.BASE_TOL + 4 x the recorded distance of the CPU oracle from the yardstick on the same
case (tests/golden/loss_batch_shapes.json, written by tests/golden/measure_loss_batch_shapes.py)."""
import functools

import numpy as np
import torch

import value_regimes as V
from launch_plans import earlier_plan

LD = V.LD
KINDS = V.KINDS
SIGMA = 1.5              # RBFKernel's sigma everywhere here
STEP_X, STEP_Y = 0.25, 0.28   # per-coordinate step of the walks: |K| stays within a few tens on paths of 6 to 9 points (the json's max_k:
                              # below 60 everywhere but for one pair of the 40 768 of 127 + 129 paths, 130)
BLOCK = 16               # rows of X per call of the yardstick
N_CU = 256               # MI355X; the host tests plan for it whatever box they run on


# ------------------------------------------------------------------------------------------------------------------- inputs
def walks(n, M, D, seed, step):
    """seeded fp64 random walks (n, M, D): cumulative sums of N(0, step^2) increments"""
    g = torch.Generator().manual_seed(int(seed))
    return (torch.cumsum(torch.randn(n, M, D, generator=g, dtype=torch.float64), 1) * step).numpy()


def case(wrapper, A, B, M, D, d, knobs=None, upstream=1.0):
    return {"wrapper": wrapper, "A": A, "B": B, "M": M, "D": D, "d": d, "knobs": dict(knobs or {}), "upstream": upstream}


def case_key(c, kind):
    return "%s|%s|%dx%d_M%d_D%d_d%d" % (c["wrapper"], kind, c["A"], c["B"], c["M"], c["D"], c["d"])


@functools.lru_cache(maxsize=None)
def _inputs(A, B, M, D):
    seed = 7000 + 131 * A + 17 * B + 5 * M + D
    return walks(A, M, D, seed, STEP_X), walks(B, M, D, seed + 1, STEP_Y)


def inputs(c):
    """X (A, M, D), Y (B, M, D): different seeds, slightly different step scales (the loss is not near 0)"""
    return _inputs(c["A"], c["B"], c["M"], c["D"])


def sigma_of(kind):
    return SIGMA if kind == "rbf" else None


# ------------------------------------------------------------------------------------------------------------------- yardstick
def triangle_pairs(n):
    """(i, j) of the strict upper triangle of n paths, i < j, row-major: the order of the one-launch route's triangle -> (rows, cols)"""
    return np.triu_indices(n, 1)


def loss_ld(kind, sigma, X, Y, d, with_yy, grad=True, block=BLOCK):
    """K_XX_m - 2 mean(K_XY) [+ K_YY_m] in long double, by row blocks of X against Z = [X; Y] under the weights
    w = [2 (1 - I) / (A (A - 1)) | -2 / (A B)] (the identity at the block's own columns; 2: the reference's rule for K_XX in the
    gradient), and gram_ld(Y, Y) for the triangle -> (scalar, dL/dX (A, M, D) or None, per-pair values: the rectangle row-major,
    then -- with_yy -- the pairs i < j of K(Y, Y) row-major).  Y may hold ONE path (compute_scoring_rule)."""
    A, B = X.shape[0], Y.shape[0]
    Z = np.concatenate([X, Y])
    rect = np.empty((A, A + B), dtype=LD)
    g = np.zeros(X.shape, dtype=LD) if grad else None
    wxx = LD(2) / LD(A * (A - 1)) if A > 1 else LD(0)
    wxy = LD(-2) / LD(A * B)
    for a0 in range(0, A, block):
        a1 = min(A, a0 + block)
        if grad:
            w = np.empty((a1 - a0, A + B), dtype=LD)
            w[:, :A] = wxx
            w[np.arange(a1 - a0), np.arange(a0, a1)] = 0
            w[:, A:] = wxy
            rect[a0:a1], g[a0:a1] = V.gram_ld(kind, sigma, X[a0:a1], Z, d, w)
        else:
            rect[a0:a1] = V.gram_ld(kind, sigma, X[a0:a1], Z, d)[0]
    off = ~np.eye(A, dtype=bool)
    value = (rect[:, :A][off].sum() / LD(A * (A - 1)) if A > 1 else LD(0)) - 2 * rect[:, A:].mean()
    pairs = rect.reshape(-1)
    if with_yy:
        Kyy = V.gram_ld(kind, sigma, Y, Y, d)[0]
        tri = Kyy[triangle_pairs(B)]
        if B > 1:
            value = value + 2 * tri.sum() / LD(B * (B - 1))
        pairs = np.concatenate([pairs, tri])
    return value, g, pairs


def distance_ld(kind, sigma, X, Y, d):
    """compute_distance: mean k(x_i, x_i) + mean k(y_i, y_i) - 2 mean k(x_i, y_i) -> (scalar, dL/dX (n, M, D)).  The diagonal of gram_ld
    under a diagonal weight; no 2x rule: x_i enters k(x_i, x_i) through the first argument only, as in the reference."""
    n = X.shape[0]
    eye = np.eye(n).astype(LD) / LD(n)
    Kxx, gxx = V.gram_ld(kind, sigma, X, X, d, eye)
    Kxy, gxy = V.gram_ld(kind, sigma, X, Y, d, -2 * eye)
    Kyy = V.gram_ld(kind, sigma, Y, Y, d)[0]
    return (np.trace(Kxx) + np.trace(Kyy) - 2 * np.trace(Kxy)) / LD(n), gxx + gxy


WITH_YY = {"mmd": True, "esr": False, "sr": False}


@functools.lru_cache(maxsize=None)
def _want(wrapper, kind, A, B, M, D, d, grad):
    X, Y = _inputs(A, B, M, D)
    if wrapper == "distance":
        return distance_ld(kind, sigma_of(kind), X, Y, d) + (None,)
    if wrapper == "sym":
        return None, None, V.gram_ld(kind, sigma_of(kind), X, X, d)[0]
    if wrapper in ("pairs_yy", "pairs"):
        return loss_ld(kind, sigma_of(kind), X, Y, d, wrapper == "pairs_yy", grad=False)
    return loss_ld(kind, sigma_of(kind), X, Y, d, WITH_YY[wrapper], grad=grad)


def want(c, kind, grad=True):
    """the yardstick's (scalar, gradient, per-pair values) of a case, computed once per process and left unchanged"""
    return _want(c["wrapper"], kind, c["A"], c["B"], c["M"], c["D"], c["d"], bool(grad))


def call_wrapper(c, kind, dev, upstream=None):
    """the case's loss wrapper on `dev` with a gradient for X -> (value, X.grad, Y.grad) as numpy / None; the upstream scalar of the
    case (or `upstream`) multiplies the loss before backward"""
    import sigkernel_amd
    X, Y = inputs(c)
    Xg, Yd = torch.from_numpy(X).clone().to(dev).requires_grad_(True), torch.from_numpy(Y).clone().to(dev)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(SIGMA), c["d"])
    fn = {"mmd": sk.compute_mmd, "esr": sk.compute_expected_scoring_rule, "sr": sk.compute_scoring_rule, "distance": sk.compute_distance}[c["wrapper"]]
    v = fn(Xg, Yd)
    up = c["upstream"] if upstream is None else upstream
    (v if up == 1.0 else up * v).backward()
    return v.detach().cpu().numpy(), Xg.grad.detach().cpu().numpy(), Yd.grad


def wb_closed_form(A, B):
    """d value / dK of the rectangle, the K_XX block doubled: what k_loss_value writes for the adjoint (fp64: one correctly rounded
    division per entry, a doubling is exact)"""
    w = np.empty((A, A + B))
    w[:, :A] = 2.0 * (1.0 / (float(A) * float(A - 1))) if A > 1 else 0.0
    w[np.arange(A), np.arange(A)] = 0.0
    w[:, A:] = -2.0 / (float(A) * float(B))
    return w.reshape(-1)


# ------------------------------------------------------------------------------------------------------------------- tables
def _settings(i):
    """path settings by table position: 6 to 9 points, D in {2, 3}, dyadic order 0 and 1 across a table (not the full product)"""
    return 6 + i % 4, 2 + i % 2, (i // 2) % 2


SMALL_SHAPES = {
    "mmd": [(2, 2), (3, 2), (2, 7), (7, 2), (5, 4), (9, 8), (17, 16), (33, 32)],
    "esr": [(2, 1), (2, 3), (5, 4), (16, 1), (33, 32)],
    "sr": [(2, 1), (3, 1), (8, 1), (64, 1)],
}
SMALL = [case(wr, A, B, *_settings(i + 3 * k)) for k, wr in enumerate(("mmd", "esr", "sr")) for i, (A, B) in enumerate(SMALL_SHAPES[wr])]
# the other two routes: a subset that still has A + B in {3, 33} (and 5, 9, 65)
OTHER_ROUTE_SHAPES = {("mmd", 2, 2), ("mmd", 5, 4), ("mmd", 17, 16), ("esr", 2, 1), ("esr", 33, 32), ("sr", 2, 1), ("sr", 8, 1), ("sr", 64, 1)}
ROUTES = ("one_launch", "no_loss_launch", "no_merged_loss")


def small_cases():
    """[(case, kind, route)]: every (wrapper, shape) on the one-launch route for both kinds; the other two routes on the subset, the
    static kernels alternating"""
    out = [(c, kind, "one_launch") for c in SMALL for kind in KINDS]
    n = 0
    for c in SMALL:
        if (c["wrapper"], c["A"], c["B"]) in OTHER_ROUTE_SHAPES:
            for r, route in enumerate(ROUTES[1:]):
                out.append((c, KINDS[(n + r) % 2], route))
            n += 1
    return out


# loss_forward per pair: (23, 46) puts the rectangle (3 105 pairs) and the triangle (1 035) past k_loss_value's 1024 threads,
# (64, 129) puts both (12 352 and 8 256) past its 8192-entry batched round
PER_PAIR = [case(wr, A, B, M, D, d) for (A, B, M, D, d) in ((5, 4, 7, 3, 1), (23, 46, 6, 2, 0), (64, 129, 9, 3, 1)) for wr in ("pairs_yy", "pairs")]

# compute_Gram(X, X, sym=True) without a gradient: the inclusive triangle of k_prep_cat (tri_n = -1); 4-point paths, dyadic 0.  The
# one-launch triangle serves every size here (it declines beyond 2^26 pairs only): 363 paths are 66 066 pairs
SYM = [case("sym", A, A, 4, 2 + i % 2, 0) for i, A in enumerate((2, 3, 45, 46, 182, 363))]

DISTANCE = [case("distance", n, n, 6 + i, 3 - i % 2, (i + 1) % 2) for i, n in enumerate((1, 2, 5, 33))]
DISTANCE_UNMERGED = case("distance", 5, 5, 7, 2, 0)      # (the same inputs as DISTANCE[2]; routes.no_merged_loss)

# Large launches, where the plan matters: compute_mmd with gradient, 8 points, 3 dims, dyadic 1.  knobs: development knobs of the
# library (read from the environment by sk_reload_knobs) the case runs under; none: natural residency (LDS holds the edge-keeping
# variants of these shapes to 4 waves per CU: 8192 lane groups on 256 CUs).  Properties on a 256-CU device, asserted by the host test
# from the restated plan and by the GPU test for the device it runs on:
#   91 + 90, no knob       16 471 + 4 005 pairs, 2 or 3 per lane group: the chunk [16470, 16472) holds the last pair of the rectangle
#                          and the first of the triangle; adjoint chunks of 2 pairs, 181 columns in 91 chunks (the uneven split);
#                          upstream scalar 3.5 (gscale on the multi-chunk finish kernels).  No counter: too few pairs per lane group.
#   127 + 129, no knob     32 512 + 8 256 pairs, 4 or 5 per lane group: the chunk [32510, 32515); adjoint chunks of 2, 256 columns in 128
#                          chunks (even).  (127 + 128 itself does not straddle under this plan: pair 32 385 is the first of its chunk.)
#   127 + 128, SK_FUSED_WPC=1   one wave per CU, 20 pairs per lane group.  LinearKernel: 7 dealt out up front, the rest DRAWN FROM THE
#                          COUNTER in chunks of 2, the drawn chunk [32384, 32386) straddles.  RBFKernel (drawn chunks would be 4 pairs and
#                          need 32 per lane group): no counter, the fixed chunk [32369, 32388) keeps edges for 16 pairs and none for 3.
#                          Adjoint chunks of 2, 255 columns in 128 chunks (uneven).
#   161 + 160, SK_FUSED_WPC=1, RBFKernel   51 681 + 12 720 pairs, 32 per lane group: 6 up front, drawn chunks of 4, [51680, 51684)
#                          straddles; adjoint chunks of 4, 321 columns in 81 chunks (uneven); upstream scalar 3.5.
# So: the boundary and the multi-chunk adjoint (uneven split, gscale) are reached without a knob, the work counter only under
# SK_FUSED_WPC=1 (a natural launch of this layout draws from it from 8 pairs per lane group of 8192 on: beyond 65 536 pairs).
def _props(straddle, queue, uneven):
    return {"straddle": straddle, "queue": queue, "uneven": uneven}


WPC1 = {"SK_FUSED_WPC": "1"}
LARGE = [
    (case("mmd", 91, 90, 8, 3, 1, upstream=3.5), {k: _props((16470, 16472), False, True) for k in KINDS}),
    (case("mmd", 127, 129, 8, 3, 1), {k: _props((32510, 32515), False, False) for k in KINDS}),
    (case("mmd", 127, 128, 8, 3, 1, knobs=WPC1), {"linear": _props((32384, 32386), True, True), "rbf": _props((32369, 32388), False, True)}),
    (case("mmd", 161, 160, 8, 3, 1, knobs=WPC1, upstream=3.5), {"rbf": _props((51680, 51684), True, True)}),
]


def large_cases():
    """[(case, kind, {"straddle": the chunk on both sides of pair A (A + B) on a 256-CU device, "queue": the launch draws from its
    counter, "uneven": (A + B) % chunks != 0 in the adjoint})]"""
    return [(c, kind, props[kind]) for c, props in LARGE for kind in KINDS if kind in props]


def golden_entries():
    """{key: (case, kind)} of every case a GPU test holds to the yardstick: exactly what tests/golden/loss_batch_shapes.json records"""
    out = {}
    for c, kind, _ in small_cases():
        out.setdefault(case_key(c, kind), (c, kind))
    for table in (PER_PAIR, SYM, DISTANCE, [DISTANCE_UNMERGED]):
        for c in table:
            for kind in KINDS:
                out.setdefault(case_key(c, kind), (c, kind))
    for c, kind, _ in large_cases():
        out.setdefault(case_key(c, kind), (c, kind))
    return out


def tolerance(recorded, c, kind, name):
    """the suite's one rule: base + 4 x the recorded distance of the CPU oracle from the yardstick on this case"""
    return V.BASE_TOL["grad" if name == "grad" else "value"] + 4.0 * recorded[case_key(c, kind)][name]


# ------------------------------------------------------------------------------------------------------------------- the launch plan
# The loss launch's lane-group chunks are a function of its plan alone: one_band_geometry (sk_pair_stream.h), the waves per CU
# launch_fwd_fused / launch_fused_nd settle on (sk_wave_fused.hip) and plan_pair_stream (launch_plans.earlier_plan), restated.
def loss_geometry(kind, M, D, d, edges=True):
    """one_band_geometry for the loss layout (tri = 2, fp64, default stencil, paths of M points on both sides) -> dict"""
    rbf = kind == "rbf"
    Mc = Nc = M - 1
    nd = 4 if D <= 4 else 8                                               # fused_nd
    if d == 1:                                                            # fused_rcx
        rcx = 4 if (not rbf or nd == 4) else 0
    elif d == 2:
        rcx = 2 if (edges and (not rbf or nd == 4)) else 0
    else:
        rcx = 2 if (rbf and nd == 8) else 0
    RC = rcx or (4, 2, 1)[d]
    assert not (rbf and d == 0 and nd == 8 and edges), "the fixed lane count of that variant is not restated"
    NU = (Nc + 2) // 2 if rbf else (Nc + 1) // 2
    NUp = (NU + 7) // 8 * 8
    rows = Mc + 1 if rbf else Mc
    logL = 3
    while logL < 6 and (RC << logL) < rows:
        logL += 1
    L = 1 << logL
    assert L * RC >= rows, "more than one band per pair"
    G = 64 // L
    JMAX = (L + NUp - 1) // NUp
    xw = 4 if (not rbf and nd == 8 and RC == 4 and not edges) else 8      # x_window
    lds = G * (((L >> 3) + 2) * nd * 128) + G * (2 * JMAX * RC * xw * (32 if nd == 4 else 64))
    cap = 8 if d == 0 else (16 if (d == 2 and nd == 4) else 12)
    return dict(NUp=NUp, L=L, G=G, lag=2 if rbf else 0, lds=lds, cap=cap)


def waves_per_cu(geo, knob=0):
    """the resident waves per CU the launcher can settle on -> a list: with SK_FUSED_WPC the one value (a knob up to 4 is below every
    register cap); without, what LDS allows in whole four-wave workgroups, or fewer -- the variant's registers and the small-launch
    rule both take whole multiples of four away"""
    w = (160 * 1024) // geo["lds"]
    if knob > 0:
        assert knob <= 4, "beyond 4 the variant's VGPR count decides"
        return [max(1, min(w, 16, knob))]
    w = min(w, geo["cap"])
    if w > 4:
        w &= ~3
    w = max(w, 1)
    return sorted(set([w] + [q for q in (4, 8, 12) if q < w]))


def forward_plan(kind, A, B, M, D, d, with_yy, wpc, n_cu, pct, edges=True):
    """the plan of sk_solve_fwd_loss_f64's launch -> dict (earlier_plan's fields, P, P_rect, G, NUp, L)"""
    geo = loss_geometry(kind, M, D, d, edges)
    P_rect = A * (A + B)
    P = P_rect + (B * (B - 1) // 2 if with_yy else 0)
    p = earlier_plan(P, geo["NUp"], geo["L"], geo["lag"], wpc, n_cu, pct, P >= 16384, geo["G"])      # (_lib._queue: a counter from 16384 pairs on)
    # shares by wave age rank (launch_fused_nd, no counter): never at these sizes -- the intervals below do not restate them
    nr, wpr = wpc // 4, n_cu * 4
    T = (P + wpr * geo["G"] - 1) // (wpr * geo["G"])
    ranked = (not p["queue"] and p["waves"] == n_cu * wpc and wpc % 4 == 0 and 2 <= nr <= 4 and wpr * nr == p["waves"] and T >= 4 * nr)
    p.update(P=P, P_rect=P_rect, G=geo["G"], NUp=geo["NUp"], L=geo["L"], ranked=ranked, wpc=wpc)
    return p


def chunk_intervals(p):
    """[(lo, hi)] of every lane-group chunk of the launch (k_fwd_fused's prologue and draw): the fixed first chunks
    [cb0 + g c0, cb0 + (g + 1) c0) of every wave, then the drawn ones, bases q_first + k G 2^logC whichever wave draws them"""
    assert not p["ranked"], "shares by age rank are not restated"
    G, P, out = p["G"], p["P"], []
    for w in range(p["waves"]):
        c0 = p["C0"] + (1 if w < p["n_big"] else 0)
        cb0 = G * (w * p["C0"] + min(w, p["n_big"]))
        for g in range(G):
            lo, hi = cb0 + g * c0, min(cb0 + (g + 1) * c0, P)
            if lo < hi:
                out.append((lo, hi))
    if p["queue"]:
        CQ = 1 << p["logC"]
        b = p["q_first"]
        while b < P:
            for g in range(G):
                lo, hi = b + g * CQ, min(b + (g + 1) * CQ, P)
                if lo < hi:
                    out.append((lo, hi))
            b += G * CQ
    return out


def straddlers(p):
    """the lane-group chunks that hold pairs on both sides of pair A (A + B) -- the last pair that keeps edges is A (A + B) - 1"""
    return [(lo, hi) for lo, hi in chunk_intervals(p) if lo < p["P_rect"] < hi]


def pick_chunk(A, Bz, max_groups):
    """pick_chunk (sk_wave_common.h): pairs per lane-group chunk of a fused adjoint over A rows of Bz columns"""
    ppg = next(dd for dd in range(1, Bz + 1) if Bz % dd == 0 and A * (Bz // dd) <= max_groups) if A <= max_groups else Bz
    nch = min(max(max_groups // A, 1), Bz)
    return min(ppg, (Bz + nch - 1) // nch)
