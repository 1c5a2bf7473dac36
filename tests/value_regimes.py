"""Value regimes: the inputs, the long-double yardstick and the case tables of tests/test_value_regimes_host.py and
tests/test_gpu_value_regimes.py (test infrastructure; numpy only -- the paths come from conftest.walk, nothing here imports the
product package or the oracle).

Every other numerical test draws unit random walks with sigma in [0.5, 1.5]: coordinates O(1), RBF exponents in about [-8, 0],
increments <= 0.1.  The families below leave that point of value space:

    drift    Y + s sqrt(3 / D) u on every coordinate, u = drift_schedule(N) from 0 to 1, sigma = 1, s in {5, 15, 30}: the most negative
             exponent is about -83, -690, -2700 at any path dim (the sqrt(3 / D) keeps |x - y|^2 what it is at dim 3) -- the whole
             range of the hand-written exponential, its subnormal results and its clamp at -800
    sigma    unit walks, sigma in {1e-2, 1e2, 1e6, 1e12}
    scale    s X, s Y, s in {1e-3, 3, 10}, sigma = 0.8; LinearKernel at s = 10 has |K| up to 1e18 -- the "wild" regime of the rescue
             kernels -- and runs only on the rows that name a shape for it
    offset   X + c, Y + c, c in {1e2, 1e4}, sigma = 0.8; LinearKernel also X + c, Y - 3 c (it is invariant under separate shifts)

The yardstick: static kernel, increments, the reference's solver (ld_reference._solve_fine_ld's recurrence, swept by anti-diagonals:
the same operations per cell, the same bits -- the host test holds the two together) and the ANALYTIC gradient in numpy long double:
W = 4^-d sum_cell K K~ (the reference's weights), times the upstream weights, scattered by the four-corner adjoint into dL/dG,
contracted with d G / d x.  Everything is formed from coordinate DIFFERENCES: ld_reference._static_ld restates the reference's
|x|^2 + |y|^2 - 2 <x, y>, which at an offset of 1e4 carries 3e8 x 2^-64 = 2e-11 into every exponent and 1e-9 relative into a
LinearKernel increment of size 0.01 -- ten times the bar this yardstick has to judge.  Differences of doubles are exact in long
double, so here a common offset costs no digit at all.
"""
import functools

import numpy as np

from ld_reference import LD, _corner

KINDS = ("linear", "rbf")
BASE_TOL = {"value": 1e-10, "grad": 1e-8, "k": 1e-10}      # instance_ledger.TOL64
OFFSET_SEEDS = 8                                           # value_regimes.json records the maximum over these for `offset`

# family -> kind -> [(parameter label, {settings})]
FAMILIES = {
    "drift": {"rbf": [("s=%g" % s, {"drift": s, "sigma": 1.0}) for s in (5.0, 15.0, 30.0)]},
    "sigma": {"rbf": [("sigma=%g" % s, {"sigma": s}) for s in (1e-2, 1e2, 1e6, 1e12)]},
    "scale": {"rbf": [("s=%g" % s, {"scale": s, "sigma": 0.8}) for s in (1e-3, 3.0, 10.0)],
              "linear": [("s=%g" % s, {"scale": s}) for s in (1e-3, 3.0)] + [("s=10", {"scale": 10.0, "wild": True})]},
    "offset": {"rbf": [("c=%g" % c, {"offset": (c, c), "sigma": 0.8}) for c in (1e2, 1e4)],
               "linear": [("c=%g" % c, {"offset": (c, c)}) for c in (1e2, 1e4)]
               + [("c=%g,-3c" % c, {"offset": (c, -3 * c)}) for c in (1e2, 1e4)]},
}


def family_cases(kind, families=None):
    """[(family, parameter label, settings)] of a static kernel, in table order"""
    return [(f, lab, st) for f in FAMILIES if families is None or f in families for lab, st in FAMILIES[f].get(kind, [])]


# ------------------------------------------------------------------------------------------------------------------- inputs
def shape(A, B, M, N, D, d, sym=False, f32=False):
    return {"A": A, "B": B, "M": M, "N": N, "D": D, "d": d, "sym": bool(sym), "f32": bool(f32)}


def shape_key(sh):
    return "%dx%d_%dx%d_D%d_d%d%s%s" % (sh["A"], sh["B"], sh["M"], sh["N"], sh["D"], sh["d"], "_sym" if sh["sym"] else "", "_f32" if sh["f32"] else "")


def drift_schedule(N):
    """The drift of y along its N points, in units of s: 0 to 1 in even steps, with four points around 0.52.  At s = 30 those sit where
    |x - y|^2 crosses 708 .. 800 -- the subnormal results and the zeros above the clamp, a band 0.03 wide that the even steps of a short
    path (1/16 at 17 points) jump over."""
    assert N >= 8
    return np.sort(np.concatenate([np.linspace(0.0, 1.0, N - 4), [0.505, 0.518, 0.531, 0.544]]))


def inputs(settings, sh, seed=0):
    """-> X (A,M,D), Y (B,N,D), w (A,B) numpy fp64 (fp32-rounded for an fp32 shape; Y = X for a symmetric one), sigma or None"""
    import torch
    from conftest import walk
    gen = torch.Generator().manual_seed(int(seed))
    A, B, M, N, D = (sh[k] for k in "ABMND")
    X = walk(gen, A, M, D).numpy()
    Y = X.copy() if sh["sym"] else walk(gen, B, N, D).numpy()
    w = torch.randn(A, B, generator=gen, dtype=torch.float64).numpy()
    s = settings.get("scale", 1.0)
    X, Y = s * X, s * Y
    if "drift" in settings:
        assert not sh["sym"]
        Y = Y + settings["drift"] * np.sqrt(3.0 / D) * drift_schedule(N)[None, :, None]
    cx, cy = settings.get("offset", (0.0, 0.0))
    X, Y = X + cx, Y + (cx if sh["sym"] else cy)
    if sh["f32"]:
        X, Y = X.astype(np.float32).astype(np.float64), Y.astype(np.float32).astype(np.float64)
    return X, Y, w, settings.get("sigma")


# ------------------------------------------------------------------------------------------------------------------- yardstick
def exponents_ld(X, Y, sigma):
    """-|x_p - y_q|^2 / sigma at every node, (A,B,M,N) long double, from coordinate differences"""
    diff = X.astype(LD)[:, None, :, None, :] - Y.astype(LD)[None, :, None, :, :]
    return -(diff * diff).sum(-1) / LD(sigma)


def increments_ld(kind, sigma, X, Y):
    """-> (coarse increments (A,B,M-1,N-1), node matrix G (A,B,M,N) or None for LinearKernel) in long double"""
    if kind == "linear":      # <dx_p, dy_q>: the four-corner difference of <x, y>, without the cancellation
        dX, dY = np.diff(X.astype(LD), axis=1), np.diff(Y.astype(LD), axis=1)
        return np.einsum("ipk,jqk->ijpq", dX, dY), None
    G = np.exp(exponents_ld(X, Y, sigma))
    return _corner(G), G


def tile(inc_c, d):
    r = 1 << d
    return np.repeat(np.repeat(inc_c.astype(LD), r, axis=-2), r, axis=-1) / LD(r * r)


def _cell_coeffs(g):
    one, half, twelfth = LD(1), LD(0.5), LD(1) / LD(12)
    return one + half * g + twelfth * g * g, one - twelfth * g * g


def solve_diag_ld(inc):
    """ld_reference._solve_fine_ld(inc, naive=False) swept by anti-diagonals: the cells of one diagonal at once, each by the very
    expression of that function -> the full grids [..., MM+1, NN+1]"""
    MM, NN = inc.shape[-2:]
    K = np.ones(inc.shape[:-2] + (MM + 1, NN + 1), dtype=LD)
    one, half, twelfth = LD(1), LD(0.5), LD(1) / LD(12)
    for s in range(MM + NN - 1):
        i = np.arange(max(0, s - NN + 1), min(MM - 1, s) + 1)
        j = s - i
        g = inc[..., i, j]
        K[..., i + 1, j + 1] = (K[..., i + 1, j] + K[..., i, j + 1]) * (one + half * g + twelfth * g * g) - \
            K[..., i, j] * (one - twelfth * g * g)
    return K


def weights_ld(inc_c, d):
    """ld_reference.adjoint_weights_ld (W = 4^-d sum_cell K K~, the reference's gradient formula) on the diagonal sweep
    -> (K[MM][NN], W) per pair"""
    r = 1 << d
    inc = tile(inc_c, d)
    K = solve_diag_ld(inc)
    Kr = solve_diag_ld(inc[..., ::-1, ::-1])[..., ::-1, ::-1]
    KK = K[..., :-1, :-1] * Kr[..., 1:, 1:]
    Mc, Nc = inc_c.shape[-2:]
    return K[..., -1, -1], KK.reshape(KK.shape[:-2] + (Mc, r, Nc, r)).sum(axis=(-3, -1)) / LD(r * r)


def exact_weights_ld(inc_c, d):
    """W = d K[MM][NN] / d inc_c of the discrete solver itself (SigKernel(exact_gradient=True); the recurrence of
    tests/exact_gradient_reference.py, default stencil) in long double, by anti-diagonals -> (K[MM][NN], W)"""
    r = 1 << d
    g = tile(inc_c, d)
    MM, NN = g.shape[-2:]
    K = solve_diag_ld(g)
    lead = g.shape[:-2]
    P, Q = np.zeros(lead + (MM + 1, NN + 1), dtype=LD), np.zeros(lead + (MM + 1, NN + 1), dtype=LD)
    P[..., :MM, :NN], Q[..., :MM, :NN] = _cell_coeffs(g)
    u = np.zeros(lead + (MM + 1, NN + 1), dtype=LD)      # (cells outside the grid: zero)
    u[..., MM - 1, NN - 1] = 1
    for s in range(MM + NN - 3, -1, -1):
        i = np.arange(max(0, s - NN + 1), min(MM - 1, s) + 1)
        j = s - i
        u[..., i, j] = P[..., i, j + 1] * u[..., i, j + 1] + P[..., i + 1, j] * u[..., i + 1, j] - Q[..., i + 1, j + 1] * u[..., i + 1, j + 1]
    dP, dQ = LD(0.5) + g / LD(6), -g / LD(6)
    Wf = u[..., :MM, :NN] * ((K[..., 1:, :-1] + K[..., :-1, 1:]) * dP - K[..., :-1, :-1] * dQ)
    Mc, Nc = inc_c.shape[-2:]
    return K[..., -1, -1], Wf.reshape(lead + (Mc, r, Nc, r)).sum(axis=(-3, -1)) / LD(r * r)


def _chain_ld(kind, sigma, X, Y, G, Ww):
    """dL/dX (A,M,D) from Ww = dL/d inc_c (A,B,M-1,N-1), upstream weights included"""
    A, B, Mc, Nc = Ww.shape
    if kind == "linear":      # inc[p][q] = <x_{p+1} - x_p, dy_q>
        T = np.einsum("abpq,bqk->apk", Ww, np.diff(Y.astype(LD), axis=1))
        g = np.zeros((A, Mc + 1, X.shape[2]), dtype=LD)
        g[:, 1:] += T
        g[:, :-1] -= T
        return g
    dG = np.zeros((A, B, Mc + 1, Nc + 1), dtype=LD)      # the four-corner adjoint
    dG[..., 1:, 1:] += Ww
    dG[..., :-1, :-1] += Ww
    dG[..., 1:, :-1] -= Ww
    dG[..., :-1, 1:] -= Ww
    diff = X.astype(LD)[:, None, :, None, :] - Y.astype(LD)[None, :, None, :, :]
    return np.einsum("abpq,abpqk->apk", dG * G * (LD(-2) / LD(sigma)), diff)


def gram_ld(kind, sigma, X, Y, d, w=None, exact=False):
    """-> (K (A,B), d sum(w K) / dX (A,M,D) or None without w) in long double; exact: the discrete solver's own gradient"""
    inc_c, G = increments_ld(kind, sigma, X, Y)
    if w is None:
        return solve_diag_ld(tile(inc_c, d))[..., -1, -1], None
    K, W = (exact_weights_ld if exact else weights_ld)(inc_c, d)
    return K, _chain_ld(kind, sigma, X, Y, G, W * np.asarray(w).astype(LD)[:, :, None, None])


def prefix_ld(kind, sigma, X, Y, d):
    """k(x[:m], y[:n]) at every coarse node: (A,B,M,N)"""
    inc_c, _ = increments_ld(kind, sigma, X, Y)
    r = 1 << d
    return solve_diag_ld(tile(inc_c, d))[..., ::r, ::r]


def _wxx(A):
    return ((np.ones((A, A)) - np.eye(A)) / (A * (A - 1.0))).astype(LD)


def mmd_ld(kind, sigma, X, Y, d):
    """compute_mmd (the unbiased estimate; the reference's 2x rule for K_XX in the gradient) -> (loss, d loss / dX (A,M,D))"""
    A, B = X.shape[0], Y.shape[0]
    Kxx, gxx = gram_ld(kind, sigma, X, X, d, _wxx(A))
    Kxy, gxy = gram_ld(kind, sigma, X, Y, d, np.full((A, B), -2.0 / (A * B)))
    Kyy, _ = gram_ld(kind, sigma, Y, Y, d)
    return (Kxx * _wxx(A)).sum() + (Kyy * _wxx(B)).sum() - 2 * Kxy.mean(), 2 * gxx + gxy


# ------------------------------------------------------------------------------------------------------------------- comparison
def value_error(got, want):
    """instance_ledger.compare_values' measure against a long-double `want`: max per element |got - want| / max(|want|, 1)"""
    got, want = np.asarray(got).astype(LD), np.asarray(want).astype(LD)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.all(np.isfinite(got.astype(np.float64))):
        return float("inf")
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), LD(1))))


def grad_error(got, want):
    """instance_ledger.compare_grads' measure: per path, max |got - want| over the path / max |want| over the path"""
    got, want = np.asarray(got).astype(LD), np.asarray(want).astype(LD)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.all(np.isfinite(got.astype(np.float64))):
        return float("inf")
    n = want.shape[0]
    norm = np.maximum(np.abs(want).reshape(n, -1).max(1), LD(1e-300))
    return float(np.max(np.abs(got - want).reshape(n, -1).max(1) / norm))


# ------------------------------------------------------------------------------------------------------------------- census
BANDS = ("[-30, 0]", "(-708, -30)", "(-745.13, -708]", "(-800, -745.13]", "<= -800")      # normal / deep / subnormal results / zero / the clamp


def census(X, Y, sigma):
    """nodes of the (A,B,M,N) grid by the band of their RBF exponent -> {band: count}"""
    e = exponents_ld(X, Y, sigma).astype(np.float64)
    masks = (e >= -30, (e > -708) & (e < -30), (e > -745.13) & (e <= -708), (e > -800) & (e <= -745.13), e <= -800)
    assert sum(int(m.sum()) for m in masks) == e.size
    return {b: int(m.sum()) for b, m in zip(BANDS, masks)}


# ------------------------------------------------------------------------------------------------------------------- routes
# One row per route family of DESIGN.md section 5 at the smallest shape that reaches it.  op: what the GPU test calls;
# claims: substrings of mangled kernel names, at least one launched instance must carry each ({kind} is replaced; a dict: per kind);
# invariant: the static kernels for which the route forms the increments AND the gradient so that a common offset of the paths costs
# no digit the base tolerance could see (`why` says where, per kind) -- their offset cases get no allowance for the oracle's own loss;
# wild: shapes whose LinearKernel cases include s = 10 (|K| up to 1e18: the suite's "wild" regime, held to the ledger's
# RESCUE_GRAD_TOL and only where the rescue kernels are on the trace).
def _row(name, op, shapes, kinds=KINDS, knobs=None, families=None, claims=(), invariant=(), why="", outputs=("value", "grad"), wild=()):
    return {"name": name, "op": op, "shapes": shapes, "kinds": kinds, "knobs": knobs or {}, "families": families, "claims": claims,
            "invariant": invariant, "why": why, "outputs": outputs, "wild": tuple(shape_key(sh) for sh in wild)}


BASE = shape(3, 3, 20, 17, 3, 1)
LONG = shape(2, 2, 150, 140, 3, 0)
F1 = ("k_fwd_fusedI",)
A1 = ("k_fwd_fusedI", "k_adj_fused_{kind}I")
WHY_F1 = ("sk_wave_fused.hip:658 (rbf nodes from d2 = sum (x - y)^2; linear: staged path differences), sk_wave_adj_fused_rbf.hip:510, "
          "sk_wave_adj_fused.hip (W against staged differences)")
# LinearKernel through the static stage: k_static_linear / k_static_linear_mfma form <dx, dy> from differences (sk_static.hip:48, :62);
# the chain rule is sk_linear_adjoint on pre-differenced y (dim <= 8, _lib.py:1362), a GEMM with dY (_lib.py:1378), or
# k_static_linear_adj_tiled (9..32 dims, <= 128 points), which contracts W[n-1] - W[n] with the POINTS y[n]: not invariant, its error is
# about 2^-53 c / |dy| sqrt(N) relative -- 3e-10 at c = 3e4 with steps of 0.05 -- thirty times below the gradient's base tolerance
WHY_LIN_STATIC = "sk_static.hip:48, :62 (differences); gradient: _lib.py:1362 / :1378 on dY, or sk_static.hip:727 at 2^-53 c / |dy| sqrt(N) = 3e-10"
ROUTES = [
    _row("F1/A1", "gram_grad", [BASE], claims=A1, invariant=KINDS, why=WHY_F1, wild=[BASE]),
    _row("F1/A1 rbf d=0 (four rows per lane)", "gram_grad", [shape(3, 3, 20, 17, 3, 0)], kinds=("rbf",), claims=A1, invariant=KINDS, why=WHY_F1),
    _row("F1/A1 rbf D=6 (one row per lane)", "gram_grad", [shape(3, 3, 20, 17, 6, 1)], kinds=("rbf",), claims=A1, invariant=KINDS, why=WHY_F1),
    _row("A1 swapped (second-argument sums)", "gram_grad", [shape(2, 3, 150, 20, 3, 1)], claims=A1, invariant=KINDS, why=WHY_F1),
    _row("F1 symmetric triangle", "sym", [shape(4, 4, 20, 20, 3, 1, sym=True)], claims=F1, invariant=KINDS, why=WHY_F1, outputs=("value",)),
    _row("F1 symmetric triangle with gradient", "sym_grad", [shape(4, 4, 20, 20, 3, 1, sym=True)], claims=A1, invariant=KINDS, why=WHY_F1),
    _row("prefix sweep", "prefix", [shape(2, 2, 20, 17, 3, 1)], claims=("k_fwd_prefix",), invariant=KINDS,
         why="sk_wave_prefix.hip:511 (d2; linear: staged differences)", outputs=("value",)),
    _row("F2/A2 multi-band", "gram_grad", [LONG, shape(2, 2, 20, 17, 12, 1)], knobs={"no_stream": True},
         claims=("k_fwd_fused_mbId", "k_adj_fused_{kind}_mbI"), invariant=KINDS, wild=[LONG],
         why="sk_wave_fused_mb.hip:634, :656 (fp64 rings: d2; linear: staged differences), sk_wave_adj_fused_mb.hip (the same for !Y32)"),
    # fp32 inputs: up to 8 dims they are staged as fp64 (the fp64 ring's d2 form, fp32 output); the fp32 ring -- |x|^2 + |y|^2 - 2 <x, y>
    # on exact products, the degree-9 polynomial -- is RBFKernel's at 9..16 dims and dyadic >= 1 (_lib.py:1034; k_fwd_fused_mb<float, .., Y32 = true, ..>)
    _row("F2/A2 fp32 inputs", "gram_grad", [shape(2, 2, 150, 140, 3, 0, f32=True)], knobs={"no_stream": True}, families=("drift", "scale"),
         claims=("k_fwd_fused_mbIfLi0ELb0E", "k_adj_fused_{kind}_mbI")),
    _row("F2/A2 fp32 inputs D=12 d=1 (fp32 ring, degree-9 polynomial)", "gram_grad", [shape(2, 2, 150, 140, 12, 1, f32=True)], kinds=("rbf",),
         knobs={"no_stream": True}, families=("drift", "scale"), claims=("k_fwd_fused_mbIfLi1ELb1E", "k_adj_fused_rbf_mbI")),
    _row("S1/S2 static stage D=12", "gram_grad", [shape(3, 3, 20, 17, 12, 1)], invariant=("linear",), why=WHY_LIN_STATIC,
         claims=("k_fwd_wave", "k_adj_wave", "k_static_{static}", "k_static_{kind}_adj")),
    _row("S1/S2 static stage D=3 (no_fused_rbf)", "gram_grad", [BASE], kinds=("rbf",), knobs={"no_fused_rbf": True},
         claims=("k_fwd_wave", "k_adj_wave", "k_static_nodes", "k_static_rbf_adj")),
    _row("S2 static adjoint D=3 (no_fused_adjoint)", "gram_grad", [BASE], knobs={"no_fused_adjoint": True}, invariant=("linear",),
         why=WHY_LIN_STATIC, claims=("k_adj_wave", "{kind}_adj")),
    _row("wide static tiles D=20", "gram_grad", [shape(2, 2, 20, 17, 20, 1), shape(2, 2, 140, 20, 20, 1)], invariant=("linear",),
         why=WHY_LIN_STATIC, claims=("k_static_{static}", "k_static_{kind}_adj_tiled")),
    # second paths beyond 128 points: RBFKernel's chain rule is k_static_rbf_adj (128 lanes), LinearKernel's the library GEMM with dY
    _row("wide static D=20, second paths > 128 points", "gram_grad", [shape(2, 2, 20, 140, 20, 1)], invariant=("linear",), why=WHY_LIN_STATIC,
         claims={"rbf": ("k_static_nodes", "k_static_rbf_adjI"), "linear": ("k_static_linear",)}),
    _row("merged loss launch", "mmd_grad", [shape(4, 4, 20, 20, 3, 1)], claims=("k_fwd_fusedI", "k_loss_value", "k_adj_fused_{kind}I"),
         invariant=KINDS, why="sk_loss.hip stages [X; Y] for the one-band kernels; " + WHY_F1),
    _row("exact_gradient=True", "exact_grad", [BASE], claims=("k_fwd_fusedI", "k_static_{static}", "{kind}_adj"), invariant=("linear",),
         why=WHY_LIN_STATIC),
    # compute_kernel_and_derivatives_Gram at this size: node values of X, X + eps gamma, X + 2 eps gamma by k_static_nodes<.., NV = 3>,
    # which keeps the LIBRARY exp (sk_static.hip:208), then the derivative solver
    _row("derivative Gram (static nodes with the library exp)", "kgrad", [shape(2, 2, 12, 10, 3, 1)], kinds=("rbf",), families=("drift",),
         claims=("k_static_nodesIdLi4ELi1ELi3E", "k_deriv_wave"), outputs=("k",)),
]
# Paths of more than 32 dims (HipBackend.MAX_FUSED_DIM): static kernel, increments and the first pass of the RBF chain rule are
# k_static_wide_mfma (tests/wide_value_regimes.py holds it to the yardstick launch by launch; these rows do it through the API).
# LinearKernel: WIDE_LINEAR stages the row-differenced paths (sk_static.hip:1165, s^2 (p1[k] - p0[k])) and the chain rule is a library
# GEMM of W with dY (_lib.py:1397): a common offset never reaches a product.  RBFKernel forms |x|^2 + |y|^2 - 2 <x, y> from the points
# (sk_static.hip:1260) and the second pass subtracts rowsum(H) x from H @ y (_lib.py:1414): the reference's own arithmetic, with its
# allowance.  The D = 32 row next to D = 33 runs the same settings through k_static_nodes (the same form of the exponent).
# (These rows, and OPERATION_ROUTES below, are kept apart from ROUTES because tests/upstream_gradients.py takes every gradient row of
# ROUTES through its own families; route_cases() walks all three lists.)
WHY_LIN_WIDE = "sk_static.hip:1165 (WIDE_LINEAR stages differences), _lib.py:1397 (GEMM of W with dY)"
WIDE = ("k_static_wide_mfma",)
WIDE_ROUTES = [
    _row("wide static D=40, tile edges", "gram_grad", [shape(2, 5, 66, 65, 40, 1)], invariant=("linear",), why=WHY_LIN_WIDE,
         claims=WIDE + ("k_fwd_wave", "k_adj_wave")),
    _row("wide static D=33 d=0", "gram_grad", [shape(2, 2, 20, 17, 33, 0)], invariant=("linear",), why=WHY_LIN_WIDE,
         claims=WIDE + ("k_fwd_wave", "k_adj_wave")),
    _row("static tiles D=32 d=0 (beside D=33)", "gram_grad", [shape(2, 2, 20, 17, 32, 0)], invariant=("linear",), why=WHY_LIN_STATIC,
         claims=("k_fwd_wave", "k_adj_wave", "k_static_{static}", "k_static_{kind}_adj_tiled")),
    _row("wide static D=40 symmetric with gradient", "sym_grad", [shape(4, 4, 20, 20, 40, 1, sym=True)], invariant=("linear",),
         why=WHY_LIN_WIDE, claims=WIDE + ("k_fwd_wave", "k_adj_wave")),
    _row("wide static D=40 exact_gradient=True", "exact_grad", [shape(3, 3, 20, 17, 40, 1)], invariant=("linear",), why=WHY_LIN_WIDE,
         claims=WIDE + ("k_fwd_wave", "k_adj_simple")),
    _row("wide static D=40 loss", "mmd_grad", [shape(4, 4, 20, 20, 40, 1)], invariant=("linear",), why=WHY_LIN_WIDE,
         claims=WIDE + ("k_fwd_wave", "k_adj_wave")),
]
# compute_kernel (paired batches) with its gradient, and the gradient with respect to the SECOND argument of compute_Gram
PAIRED40 = shape(3, 3, 20, 17, 40, 1)
OPERATION_ROUTES = [
    _row("paired F1/A1", "paired_grad", [BASE], claims=A1, invariant=KINDS, why=WHY_F1),
    _row("paired S1/S2 static stage D=12", "paired_grad", [shape(3, 3, 20, 17, 12, 1)], invariant=("linear",), why=WHY_LIN_STATIC,
         claims=("k_fwd_wave", "k_adj_wave", "k_static_{static}", "k_static_{kind}_adj")),
    _row("paired wide static D=40", "paired_grad", [PAIRED40], invariant=("linear",), why=WHY_LIN_WIDE, claims=WIDE + ("k_fwd_wave", "k_adj_wave")),
    # (exact_gradient=True: the only mode with a gradient for Y.  Up to 8 dims LinearKernel's is sk_static_adjoint2 on pre-differenced x
    # (_lib.py:1438); beyond, and for RBFKernel beyond 32, sk_static_adjoint on the swapped pairs with W transposed)
    _row("second argument exact_gradient=True", "gram_grad_y", [BASE], invariant=("linear",), why="_lib.py:1438 (pre-differenced x); " + WHY_LIN_STATIC,
         claims=("k_fwd_fusedI", "k_adj_simple", "k_static_{static}", "k_{kind}_adj2")),
    _row("second argument static stage D=12", "gram_grad_y", [shape(3, 3, 20, 17, 12, 1)], invariant=("linear",), why=WHY_LIN_STATIC,
         claims={"linear": ("k_fwd_wave", "k_adj_simple", "k_static_linear", "k_static_linear_adj_tiled"),
                 "rbf": ("k_fwd_wave", "k_adj_simple", "k_static_nodes", "k_rbf_adj2")}),
    _row("second argument wide static D=40", "gram_grad_y", [PAIRED40], invariant=("linear",), why=WHY_LIN_WIDE,
         claims=WIDE + ("k_fwd_wave", "k_adj_simple")),
]
ALL_ROUTES = ROUTES + WIDE_ROUTES + OPERATION_ROUTES
RESCUE_CLAIMS = ("k_screen", "k_fused_rescue")


def claims_of(row, kind, settings=None):
    cl = row["claims"][kind] if isinstance(row["claims"], dict) else row["claims"]
    cl = [c.format(kind=kind, static="linear" if kind == "linear" else "nodes") for c in cl]
    return cl + list(RESCUE_CLAIMS) if settings and settings.get("wild") else cl


def route_cases():
    """[(row, shape, kind, family, parameter label, settings)] -- every cell of the GPU test"""
    out = []
    for row in ALL_ROUTES:
        for sh in row["shapes"]:
            for kind in row["kinds"]:
                for fam, lab, st in family_cases(kind, row["families"]):
                    if sh["sym"] and (fam == "drift" or st.get("offset", (0, 0))[0] != st.get("offset", (0, 0))[1]):
                        continue      # (one batch: nothing to drift away from, no separate shifts)
                    if st.get("wild") and shape_key(sh) not in row["wild"]:
                        continue
                    out.append((row, sh, kind, fam, lab, st))
    return out


def golden_key(fam, lab, kind, sh):
    return "%s|%s|%s|%s" % (fam, lab, kind, shape_key(sh))


def golden_entries():
    """the distinct (family, parameter, kernel, shape) of route_cases(), keyed as value_regimes.json is"""
    out = {}
    for row, sh, kind, fam, lab, st in route_cases():
        out.setdefault(golden_key(fam, lab, kind, sh), (fam, lab, kind, sh, st))
    return out


@functools.lru_cache(maxsize=None)
def _cached_inputs(fam, lab, kind, key, seed):
    st = dict(FAMILIES[fam][kind])[lab]
    return inputs(st, _SHAPES[key], seed)


_SHAPES = {shape_key(sh): sh for row in ALL_ROUTES for sh in row["shapes"]}


def case_inputs(fam, lab, kind, sh, seed=0):
    return _cached_inputs(fam, lab, kind, shape_key(sh), seed)


@functools.lru_cache(maxsize=None)
def _cached_want(fam, lab, kind, key, what):
    X, Y, w, sigma = _cached_inputs(fam, lab, kind, key, 0)
    d = _SHAPES[key]["d"]
    if what == "gram":
        return gram_ld(kind, sigma, X, Y, d, w)
    if what == "exact":
        return gram_ld(kind, sigma, X, Y, d, w, exact=True)
    if what == "sym":      # d sum(w K(X, X)) / dX: the first- and the second-argument sums
        K, g1 = gram_ld(kind, sigma, X, X, d, w)
        _, g2 = gram_ld(kind, sigma, X, X, d, w.T.copy())
        return K, (2 * g1, g1 + g2)      # the reference's 2x rule (all pairs) or both arguments (the triangle)
    if what == "prefix":
        return prefix_ld(kind, sigma, X, Y, d), None
    if what == "paired":      # compute_kernel: the diagonal pairs, weighted by the diagonal of w
        K, g = gram_ld(kind, sigma, X, Y, d, np.diag(np.diag(w)))
        return np.diagonal(K).copy(), g
    if what == "gram_y":      # d sum(w K(X, Y)) / dY: the first-argument gradient of K(Y, X) under the transposed weights; the API returns a
        K, g = gram_ld(kind, sigma, Y, X, d, w.T.copy(), exact=True)      # gradient for Y under exact_gradient=True alone
        return K.T.copy(), g
    assert what == "mmd", what
    return mmd_ld(kind, sigma, X, Y, d)


def case_want(fam, lab, kind, sh, what):
    """the yardstick's (value, gradient) of a case, computed once per process"""
    return _cached_want(fam, lab, kind, shape_key(sh), what)
