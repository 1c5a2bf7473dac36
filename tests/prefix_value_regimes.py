"""The prefix sweep (k_fwd_prefix, csrc/sk_wave_prefix.hip) and everything built on it -- compute_Gram_prefixes / compute_kernel_prefixes
with their slices, compute_mmd_prefixes, the ragged methods and the ragged exact gradient -- away from the unit-walk inputs: the case
table, the long-double yardstick and the padding variants of tests/test_prefix_value_regimes_host.py and
tests/test_gpu_prefix_value_regimes.py (test infrastructure; numpy and torch on the CPU only -- nothing here imports the product package
or the oracle).

Families: value_regimes.FAMILIES, unchanged.  Yardstick: value_regimes.prefix_ld -- every coarse node of the long-double grid, formed
from coordinate differences; a ragged value is node (len_x - 1, len_y - 1) of it; a ragged exact gradient is, pair by pair on the
TRUNCATED paths, value_regimes.exact_weights_ld on the pair's own sub-block and value_regimes._chain_ld for X and, roles swapped, for Y,
times the upstream weight, and exactly zero on every padded point.  Its certificate (the host test): a central difference of the
long-double value along a random direction.

Rows: one per item that k_fwd_prefix, its launcher and the host layer decide by, at the smallest shape that reaches it --
    the four instances (linear dyadic 0: four rows per lane; rbf dyadic 0: two; dyadic 1 and 2: either static kernel), each at a pair
    that takes a few lanes (two or more lane groups per wave: a Gram launch runs the shared-y pair order) and at one that needs all 64
    (`lanes_of`: the launcher's rule, sk_pair_stream.h one_band_geometry);
    store scheme 3 (even N, even grid distance, aligned `out`) and scheme 2 (odd N; an even N written into a view of `out` that starts
    at an odd element: `store_scheme`, the launcher's can_wide);  D = 1, 3, 8 of the 8 staged dims;  3 x 3 Gram pairs (no lane-group
    count -- 8, 4, 2 -- divides 9) and the paired launch;  fp32 stores;  the streamed fallback at D = 12 and one row past the one-band
    limit;  compute_mmd_prefixes, compute_mmd_ragged;  the ragged exact gradients of compute_Gram_ragged / compute_kernel_ragged at
    D = 3, 12 (static stage) and 40 (k_static_wide_mfma) on every family, of compute_mmd_ragged at the same dims on the families of its value
    row (drift and offset: three Gram matrices per case, and the yardstick's cost with them).
The slices (`nodes` = diagonal / last_row / last_col) and the ragged node get no second comparison with the yardstick: every case of a
grid row asserts their bit-equality with the grid it has just compared (one launch each); the ragged launch runs on NINE paths per side
-- the row's paths repeated -- so that every length `ragged_lens` aims at (1, 2, the padded length, the rows of the first and of the
last lane) is met in every case.

The bound is the project's one rule, base + 4 r: base = value_regimes.BASE_TOL; r = the recorded distance of the reference's
arithmetic from the yardstick on that case (tests/golden/prefix_value_regimes.json -- the maximum over ALL nodes of the grid, gradients
per path); fp32: two fp32 ulps on top.  No allowance on `offset` (base alone) for the VALUES of the fused rows, either static kernel
(sk_wave_prefix.hip:511 forms d2 from differences; LinearKernel stages differences), and for the GRADIENTS of LinearKernel (the chain
rule is the static stage's: value_regimes.WHY_LIN_STATIC / WHY_LIN_WIDE).
"""
import functools

import numpy as np

import value_regimes as V
from value_regimes import LD

# ------------------------------------------------------------------------------------------------------------------- the launcher's rules
LARGEST = {("linear", 0): 257, ("rbf", 0): 128, ("linear", 1): 129, ("rbf", 1): 128, ("linear", 2): 65, ("rbf", 2): 64}   # test_gpu_ragged.LARGEST
MAX_FUSED_D = 8


def rows_per_lane(kind, d):
    """prefix_rc (sk_wave_prefix.hip)"""
    return 2 if (kind == "rbf" and d == 0) else (4, 2, 1)[d]


def lanes_of(kind, d, M):
    """lanes per pair: the smallest of 8, 16, 32, 64 whose rows hold the pair (M - 1 increment rows, M node rows for RBFKernel)"""
    rows, L = (M if kind == "rbf" else M - 1), 8
    while L < 64 and rows_per_lane(kind, d) * L < rows:
        L *= 2
    return L


def is_fused(kind, d, M, D):
    return D <= MAX_FUSED_D and M <= LARGEST[(kind, d)]


def store_scheme(M, N, odd_view=False):
    """3: two-column pieces (even N, an even distance M N between the grids, `out` aligned to two elements); else 2"""
    return 3 if N % 2 == 0 and (M * N) % 2 == 0 and not odd_view else 2


def instance_claim(kind, d):
    """the mangled template arguments of k_fwd_prefix<DY, KIND, RCX>"""
    return "k_fwd_prefixILi%dELi%dELi%dEE" % (d, (0 if kind == "linear" else 1) if d == 0 else 2, 2 if (kind == "rbf" and d == 0) else 0)


def ragged_lens(seed, count, top):
    """test_gpu_ragged._lens, restated (that module imports the product; the GPU test holds the two together): 1, 2 and top first, then
    the rows k < 4 of the first lane, the rows of the last lane, both parities, then random ones; permuted"""
    aimed = [1, 2, top, 3, top - 1, 4, top - 2, 5, top - 3]
    if count < 3:
        aimed = [top, 2, 1]
    aimed = [v for i, v in enumerate(aimed) if 1 <= v <= top and v not in aimed[:i]]
    g = np.random.default_rng(seed)
    lens = (aimed + g.integers(1, top + 1, size=max(0, count - len(aimed))).tolist())[:count]
    return [int(v) for v in g.permutation(lens)]


RAGGED_COUNT = 9      # paths per side of the ragged launch of a grid row: path i is the row's path i % batch


def ragged_case(sh, gram):
    """-> (ix, iy, lx, ly): which of the row's paths the nine (paired: nine pairs of) ragged paths are, and their lengths"""
    n = RAGGED_COUNT
    ix, iy = [i % sh["A"] for i in range(n)], [i % sh["B"] for i in range(n)]
    return ix, iy, ragged_lens(sh["M"], n, sh["M"]), ragged_lens(sh["N"] + 1, n, sh["N"])


# ------------------------------------------------------------------------------------------------------------------- rows
VALUE_OPS = ("grid", "grid_out", "mmd_prefixes", "mmd_ragged")
GRAD_OPS = ("gram_ragged_grad", "kernel_ragged_grad", "mmd_ragged_grad")


def _row(name, op, sh, kinds=V.KINDS, gram=True, families=None, lanes=None, scheme=None, fused=True, wild=False, claims=()):
    return {"name": name, "op": op, "shape": sh, "kinds": kinds, "gram": gram, "families": families, "lanes": lanes, "scheme": scheme,
            "fused": fused, "wild": wild, "claims": claims}


S = V.shape
F32_FAMILIES = ("drift", "scale")
MMD_FAMILIES = ("drift", "offset")
GRAD_SHAPES = {3: S(3, 3, 20, 17, 3, 1), 12: S(3, 3, 20, 17, 12, 1), 40: S(3, 3, 20, 17, 40, 1)}      # value_regimes BASE / D = 12 / PAIRED40


def grad_lens(M, N):
    """three lengths per side: the padded length, a length inside the grid, two points; one point (k = 1, no gradient) -- (20, 6, 2) and
    (1, 5, 17) on the gradient rows"""
    return [M, max(2, M // 3), 2], [1, max(2, N // 3), N]


ROWS = [
    # the four instances: few lanes (>= 2 lane groups, shared-y in a Gram launch), then all 64 lanes
    _row("linear d=0, 8 lanes, scheme 3", "grid", S(3, 3, 20, 16, 3, 0), kinds=("linear",), lanes=8, scheme=3, wild=True),
    _row("linear d=0, 64 lanes (M - 1 > 128)", "grid", V.LONG, kinds=("linear",), lanes=64, scheme=3),
    _row("rbf d=0 (two rows per lane), 16 lanes, scheme 2", "grid", S(3, 3, 20, 17, 3, 0), kinds=("rbf",), lanes=16, scheme=2),
    _row("rbf d=0, 64 lanes (64 < M <= 128), D=1", "grid", S(2, 2, 70, 16, 1, 0), kinds=("rbf",), lanes=64, scheme=3),
    _row("d=1, 16 lanes, D=8, scheme 3", "grid", S(3, 3, 20, 16, 8, 1), lanes=16, scheme=3),
    _row("d=1, 64 lanes, scheme 2", "grid", S(2, 2, 70, 17, 3, 1), lanes=64, scheme=2),
    _row("d=2, 32 lanes, D=1, scheme 2", "grid", S(3, 3, 20, 17, 1, 2), lanes=32, scheme=2),
    _row("d=2, 64 lanes (32 < rows <= 64), D=8", "grid", S(2, 2, 40, 16, 8, 2), lanes=64, scheme=3),
    _row("paired launch d=1", "grid", S(3, 3, 20, 16, 3, 1), gram=False, lanes=16, scheme=3),
    _row("paired launch d=0, scheme 2", "grid", S(3, 3, 20, 17, 3, 0), gram=False, scheme=2),
    _row("even N into an odd view of out (scheme 2)", "grid_out", S(2, 2, 20, 16, 3, 1), lanes=16, scheme=2),
    _row("fp32 stores, scheme 3", "grid", S(3, 3, 20, 16, 3, 1, f32=True), families=F32_FAMILIES, lanes=16, scheme=3),
    _row("fp32 stores d=0, scheme 2", "grid", S(2, 2, 20, 17, 3, 0, f32=True), families=F32_FAMILIES, scheme=2),
    # the streamed fallback: static stage + the stored-grid solver (k_fwd_simple: solve_fwd(want_grid=True)) + gather
    _row("streamed D=12", "grid", S(2, 2, 20, 17, 12, 1), fused=False, claims=("k_fwd_simple", "k_static_{static}")),
    _row("streamed: rbf d=2, one point past the band", "grid", S(2, 2, 65, 9, 3, 2), kinds=("rbf",), fused=False, claims=("k_fwd_simple",)),
    _row("compute_mmd_prefixes", "mmd_prefixes", S(3, 3, 20, 17, 3, 1), families=MMD_FAMILIES),
    _row("compute_mmd_ragged", "mmd_ragged", S(3, 3, 20, 17, 3, 1), families=MMD_FAMILIES),
    # the ragged exact gradients: forward as above; backward k_adj_simple on every pair's sub-grid, then the static adjoint of the
    # non-ragged row of value_regimes.OPERATION_ROUTES / ROUTES (exact_grad, gram_grad_y)
    _row("compute_Gram_ragged gradients D=3", "gram_ragged_grad", GRAD_SHAPES[3],
         claims=("k_adj_simple", "k_static_{static}", "{kind}_adj", "k_{kind}_adj2")),
    _row("compute_Gram_ragged gradients D=12", "gram_ragged_grad", GRAD_SHAPES[12], fused=False,
         claims={"linear": ("k_fwd_simple", "k_adj_simple", "k_static_linear", "k_static_linear_adj_tiled"),
                 "rbf": ("k_fwd_simple", "k_adj_simple", "k_static_nodes", "k_static_rbf_adj", "k_rbf_adj2")}),
    _row("compute_Gram_ragged gradients D=40", "gram_ragged_grad", GRAD_SHAPES[40], fused=False,
         claims=("k_static_wide_mfma", "k_fwd_simple", "k_adj_simple")),
    _row("compute_kernel_ragged gradients D=3", "kernel_ragged_grad", GRAD_SHAPES[3], gram=False,
         claims=("k_adj_simple", "k_static_{static}", "{kind}_adj")),
    _row("compute_kernel_ragged gradients D=12", "kernel_ragged_grad", GRAD_SHAPES[12], gram=False, fused=False,
         claims=("k_fwd_simple", "k_adj_simple", "k_static_{static}", "k_static_{kind}_adj")),
    _row("compute_kernel_ragged gradients D=40", "kernel_ragged_grad", GRAD_SHAPES[40], gram=False, fused=False,
         claims=("k_static_wide_mfma", "k_fwd_simple", "k_adj_simple")),
    _row("compute_mmd_ragged gradients D=3", "mmd_ragged_grad", GRAD_SHAPES[3], families=MMD_FAMILIES,
         claims=("k_adj_simple", "k_static_{static}", "{kind}_adj", "k_{kind}_adj2")),
    _row("compute_mmd_ragged gradients D=12", "mmd_ragged_grad", GRAD_SHAPES[12], families=MMD_FAMILIES, fused=False,
         claims={"linear": ("k_fwd_simple", "k_adj_simple", "k_static_linear", "k_static_linear_adj_tiled"),
                 "rbf": ("k_fwd_simple", "k_adj_simple", "k_static_nodes", "k_static_rbf_adj", "k_rbf_adj2")}),
    _row("compute_mmd_ragged gradients D=40", "mmd_ragged_grad", GRAD_SHAPES[40], families=MMD_FAMILIES, fused=False,
         claims=("k_static_wide_mfma", "k_fwd_simple", "k_adj_simple")),
]


def outputs_of(row):
    return ("value", "grad_x", "grad_y") if row["op"] in GRAD_OPS else ("value",)


def claims_of(row, kind):
    cl = row["claims"][kind] if isinstance(row["claims"], dict) else row["claims"]
    cl = [c.format(kind=kind, static="linear" if kind == "linear" else "nodes") for c in cl]
    return cl + ([instance_claim(kind, row["shape"]["d"])] if row["fused"] else [])


def cases():
    """[(row, kind, family, label, settings)]"""
    out = []
    for row in ROWS:
        for kind in row["kinds"]:
            for fam, lab, st in V.family_cases(kind, row["families"]):
                if st.get("wild") and not row["wild"]:
                    continue
                out.append((row, kind, fam, lab, st))
    return out


def op_class(row):
    return {"grid": "grid", "grid_out": "grid", "mmd_prefixes": "mmdp", "mmd_ragged": "mmdr", "gram_ragged_grad": "ggrad",
            "kernel_ragged_grad": "kgrad", "mmd_ragged_grad": "mgrad"}[row["op"]]


def geometry_key(row):
    return V.shape_key(row["shape"]) + ("" if row["gram"] else "_paired")


def golden_key(c):
    row, kind, fam, lab, st = c
    return "%s|%s|%s|%s|%s" % (op_class(row), fam, lab, kind, geometry_key(row))


def case_id(c):
    return "%s-%s-%s-%s" % (c[0]["name"].replace(" ", "_"), c[1], c[2], c[3])


def golden_entries():
    out = {}
    for c in CASES:
        out.setdefault(golden_key(c), c)
    return out


def invariant(c, name):
    """no allowance on `offset`: values of the fused rows; gradients of LinearKernel (module docstring)"""
    row, kind, fam, lab, st = c
    if fam != "offset":
        return False
    return row["fused"] if name == "value" else kind == "linear"


def tolerance(c, name, recorded, assume_invariant=True):
    """assume_invariant=False: the host test's back-end IS the reference's arithmetic, whose loss on offsets the invariance is about"""
    from instance_ledger import F32_ULPS2
    base = V.BASE_TOL["value" if name == "value" else "grad"] + (F32_ULPS2 if c[0]["shape"]["f32"] else 0.0)
    if assume_invariant and invariant(c, name):
        return base
    return base + 4.0 * recorded[golden_key(c)][name]


# ------------------------------------------------------------------------------------------------------------------- inputs
def inputs(c, seed=0):
    """-> X (A,M,D), Y (B,N,D), w numpy fp64, sigma; w: (A,B) Gram, (A,) paired, () the loss"""
    row, kind, fam, lab, st = c
    X, Y, w, sigma = V.inputs(st, row["shape"], seed)
    if row["op"] in ("mmd_prefixes", "mmd_ragged", "mmd_ragged_grad"):
        w = w[0, 0]
    elif not row["gram"]:
        w = np.diagonal(w).copy()
    return X, Y, w, sigma


def lens_of(row):
    """the lengths a row's ragged call gets (the grid rows: see ragged_case) -> (lx, ly)"""
    sh = row["shape"]
    if row["op"] in GRAD_OPS:
        return grad_lens(sh["M"], sh["N"])
    return ragged_lens(sh["M"], sh["A"], sh["M"]), ragged_lens(sh["N"] + 1, sh["B"], sh["N"])


@functools.lru_cache(maxsize=None)
def _cached_inputs(key, seed):
    out = inputs(CASE_BY_ID[key], seed)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def case_inputs(c, seed=0):
    return _cached_inputs(case_id(c), seed)


# ------------------------------------------------------------------------------------------------------------------- yardstick
def grid_ld(kind, sigma, X, Y, d, gram):
    """every coarse node: (A,B,M,N) Gram, (A,M,N) paired"""
    if gram:
        return V.prefix_ld(kind, sigma, X, Y, d)
    return np.stack([V.prefix_ld(kind, sigma, X[a:a + 1], Y[a:a + 1], d)[0, 0] for a in range(X.shape[0])])


def nodes_at(grid, lx, ly, gram):
    """node (lx - 1, ly - 1) of every pair's grid (numpy, any dtype): (A,B) Gram, (A,) paired"""
    ia, ib = np.asarray(lx) - 1, np.asarray(ly) - 1
    if gram:
        A, B = grid.shape[:2]
        return grid[np.arange(A)[:, None], np.arange(B)[None, :], ia[:, None], ib[None, :]]
    return grid[np.arange(grid.shape[0]), ia, ib]


def slice_of(grid, nodes):
    """sigkernel._prefix_nodes on numpy"""
    if nodes == "diagonal":
        return np.diagonal(grid, axis1=-2, axis2=-1)
    return grid[..., -1, :] if nodes == "last_row" else grid[..., :, -1]


def _offdiag_mean(K):
    """compute_mmd's mean of K without its diagonal, over the two leading axes"""
    A = K.shape[0]
    return (K.sum(axis=(0, 1)) - np.trace(K, axis1=0, axis2=1)) / LD(A * (A - 1.0))


def mmd_prefixes_from(gxx, gyy, gxy):
    """compute_mmd_prefixes from three prefix grids (any float dtype): value t from node (t, t)"""
    T = min(gxy.shape[-2:])
    dxx, dyy, dxy = (slice_of(g, "diagonal")[..., :T] for g in (gxx, gyy, gxy))
    return _offdiag_mean(dxx) + _offdiag_mean(dyy) - 2 * dxy.mean(axis=(0, 1))


def mmd_ragged_from(gxx, gyy, gxy, lx, ly):
    kxx, kyy, kxy = nodes_at(gxx, lx, lx, True), nodes_at(gyy, ly, ly, True), nodes_at(gxy, lx, ly, True)
    kxx, kyy = (kxx + kxx.T) / 2, (kyy + kyy.T) / 2
    return _offdiag_mean(kxx) + _offdiag_mean(kyy) - 2 * kxy.mean()


def pair_grads_ld(kind, sigma, x, y, d):
    """one pair of TRUNCATED paths x (m,D), y (n,D), m, n >= 2 -> (k, dk/dx (m,D), dk/dy (n,D)) in long double: exact_weights_ld on
    the pair's own block, _chain_ld for x and -- the roles swapped, W and the nodes transposed -- for y"""
    inc, G = V.increments_ld(kind, sigma, x[None], y[None])
    K, W = V.exact_weights_ld(inc, d)
    gx = V._chain_ld(kind, sigma, x[None], y[None], G, W)[0]
    Gt = None if G is None else np.ascontiguousarray(G.transpose(1, 0, 3, 2))
    gy = V._chain_ld(kind, sigma, y[None], x[None], Gt, np.ascontiguousarray(W.transpose(1, 0, 3, 2)))[0]
    return K[0, 0], gx, gy


def ragged_grads_ld(kind, sigma, X, Y, lx, ly, d, w, pairs=None):
    """sum over the pairs (a, b) of w[a, b] k(x_a[:lx[a]], y_b[:ly[b]]) -> (K (A,B), dL/dX (A,M,D), dL/dY (B,N,D)); exactly zero on the
    padded points; a one-point path: k = 1, no gradient.  pairs: only these (the rest of K stays 1, their weights unused)"""
    A, B = X.shape[0], Y.shape[0]
    K, gX, gY = np.ones((A, B), dtype=LD), np.zeros(X.shape, dtype=LD), np.zeros(Y.shape, dtype=LD)
    for a, b in (pairs if pairs is not None else [(a, b) for a in range(A) for b in range(B)]):
        m, n = lx[a], ly[b]
        if m < 2 or n < 2:
            continue
        k, gx, gy = pair_grads_ld(kind, sigma, X[a, :m], Y[b, :n], d)
        K[a, b] = k
        gX[a, :m] += LD(w[a, b]) * gx
        gY[b, :n] += LD(w[a, b]) * gy
    return K, gX, gY


def mmd_weights(A, B):
    """the loss as weighted sums of the three Gram matrices: K_XX and K_YY symmetrised, without their diagonals"""
    wxx, wyy = ((np.ones((n, n)) - np.eye(n)) / (n * (n - 1.0)) for n in (A, B))
    return wxx, wyy, np.full((A, B), -2.0 / (A * B))


def assemble(op, gram, X, Y, lx, ly, w, gram_fn):
    """The three gradient operations from a function gram_fn(P, Q, lp, lq, weights, pairs) -> (K, dL/dP, dL/dQ) of weighted ragged
    Gram matrices -- shared by the yardstick and the reference's arithmetic -> (value, dL/dX, dL/dY)"""
    A, B = X.shape[0], Y.shape[0]
    if op == "gram_ragged_grad":
        return gram_fn(X, Y, lx, ly, w, None)
    if op == "kernel_ragged_grad":
        K, gx, gy = gram_fn(X, Y, lx, ly, np.diag(w), [(a, a) for a in range(A)])
        return np.diagonal(K).copy(), gx, gy
    assert op == "mmd_ragged_grad", op
    wxx, wyy, wxy = mmd_weights(A, B)
    # (K + K^T) / 2 under symmetric weights is K under the same weights, and k(x_a, x_b) = k(x_b, x_a): the pairs a < b under twice the
    # weight (the diagonal has none).  X is both arguments of K_XX: the two gradients add.
    upper = lambda n: [(a, b) for a in range(n) for b in range(a + 1, n)]      # noqa: E731
    Kxx, g1, g2 = gram_fn(X, X, lx, lx, 2 * w * wxx, upper(A))
    Kyy, h1, h2 = gram_fn(Y, Y, ly, ly, 2 * w * wyy, upper(B))
    Kxy, gx, gy = gram_fn(X, Y, lx, ly, w * wxy, None)
    value = (np.triu(Kxx, 1) * 2 * wxx).sum() + (np.triu(Kyy, 1) * 2 * wyy).sum() + (Kxy * wxy).sum()
    return value, g1 + g2 + gx, h1 + h2 + gy


def want_of(c, seed=0):
    """the yardstick of a case -> {"value", "grad_x", "grad_y"} (gradient rows) or {"value", "grid": (gxx, gyy, gxy) or the grid}"""
    row, kind, fam, lab, st = c
    X, Y, w, sigma = case_inputs(c, seed)
    d, op = row["shape"]["d"], row["op"]
    if op in ("grid", "grid_out"):
        g = grid_ld(kind, sigma, X, Y, d, row["gram"])
        return {"value": g}
    if op in ("mmd_prefixes", "mmd_ragged"):
        grids = (V.prefix_ld(kind, sigma, X, X, d), V.prefix_ld(kind, sigma, Y, Y, d), V.prefix_ld(kind, sigma, X, Y, d))
        if op == "mmd_prefixes":
            return {"value": mmd_prefixes_from(*grids)}
        return {"value": np.asarray(mmd_ragged_from(*grids, *lens_of(row)))}
    lx, ly = lens_of(row)
    value, gx, gy = assemble(op, row["gram"], X, Y, lx, ly, w,
                             lambda P, Q, lp, lq, ww, pairs: ragged_grads_ld(kind, sigma, P, Q, lp, lq, d, ww, pairs))
    return {"value": np.asarray(value), "grad_x": gx, "grad_y": gy}


@functools.lru_cache(maxsize=None)
def _cached_want(key):
    return want_of(CASE_BY_ID[key])


def case_want(c):
    return _cached_want(case_id(c))


def error(name, got, want):
    """value_regimes.value_error per node (per element over max(|want|, 1)); gradients value_regimes.grad_error per path -- over the TRUE
    points and the padding alike (the yardstick is zero there)"""
    if name == "value":
        return V.value_error(np.asarray(got).reshape(np.shape(want)), want)
    return V.grad_error(got, want)


# ------------------------------------------------------------------------------------------------------------------- certificate
def fd_certificate(c, seed=7, h=1e-6):
    """the gradient yardstick of a case against a central difference of the long-double VALUE of its loss sum(w k) along one random
    direction (U, V) of all true points of both batches, step h times the largest step of the paths ->
    |<dL/dX, U> + <dL/dY, V> - difference| / (sum |dL/dX U| + sum |dL/dY V|)"""
    row, kind, fam, lab, st = c
    X, Y, w, sigma = case_inputs(c)
    d, op = row["shape"]["d"], row["op"]
    lx, ly = lens_of(row)
    want = case_want(c)
    g = np.random.default_rng(seed)
    U, Vd = g.standard_normal(X.shape).astype(LD), g.standard_normal(Y.shape).astype(LD)
    span = max(float(np.max(np.abs(np.diff(X, axis=1)))), float(np.max(np.abs(np.diff(Y, axis=1)))))
    hh = LD(h) * LD(span)

    def values(P, Q, lp, lq, ww, pairs):
        K = np.ones((P.shape[0], Q.shape[0]), dtype=LD)
        for a, b in (pairs if pairs is not None else [(a, b) for a in range(P.shape[0]) for b in range(Q.shape[0])]):
            if lp[a] >= 2 and lq[b] >= 2:
                inc, _ = V.increments_ld(kind, sigma, P[a, :lp[a]][None], Q[b, :lq[b]][None])      # (its cast of a long double: the identity)
                K[a, b] = V.solve_diag_ld(V.tile(inc, d))[0, 0, -1, -1]
        return K, None, None

    def loss(P, Q):
        value, _, _ = assemble_values(op, P, Q, lx, ly, w, values)
        return value
    fd = (loss(X.astype(LD) + hh * U, Y.astype(LD) + hh * Vd) - loss(X.astype(LD) - hh * U, Y.astype(LD) - hh * Vd)) / (2 * hh)
    tx, ty = want["grad_x"] * U, want["grad_y"] * Vd
    return float(abs(tx.sum() + ty.sum() - fd) / (np.abs(tx).sum() + np.abs(ty).sum()))


def assemble_values(op, X, Y, lx, ly, w, values_fn):
    """the loss sum(w k) of a gradient operation from ragged Gram VALUES alone (the weights of `assemble`)"""
    A, B = X.shape[0], Y.shape[0]
    if op == "gram_ragged_grad":
        return (values_fn(X, Y, lx, ly, w, None)[0] * w.astype(LD)).sum(), None, None
    if op == "kernel_ragged_grad":
        return (np.diagonal(values_fn(X, Y, lx, ly, None, [(a, a) for a in range(A)])[0]) * w.astype(LD)).sum(), None, None
    wxx, wyy, wxy = mmd_weights(A, B)
    return LD(w) * ((values_fn(X, X, lx, lx, None, None)[0] * wxx).sum() + (values_fn(Y, Y, ly, ly, None, None)[0] * wyy).sum()
                    + (values_fn(X, Y, lx, ly, None, None)[0] * wxy).sum()), None, None


# ------------------------------------------------------------------------------------------------------------------- padding variants
PADDINGS = ("repeat", "walk", "garbage37", "1e100", "1e200", "+-1.5e308", "nan+inf")      # (a) .. (g) of the module's claims
PAD_VALUES = {False: (1e100, 1e200, 1.5e308), True: (1e18, 1e30, 3e38)}                  # fp64 / their fp32 counterparts


def padded(P, lens, variant, f32=False, seed=3):
    """a copy of the paths P (batch, length, D; the walk goes on behind every path's end) with the points from lens[i] on replaced:
    repeat: the last true point; walk: left as they are; garbage37: 37 randn; 1e100 (finite), 1e200 (its square overflows; fp32: 1e18,
    1e30); +-1.5e308 alternating from point to point (differences overflow; fp32: 3e38); nan+inf: the repeated point with one NaN
    (the first padded coordinate) and one +inf (the last) -- in every path that has padding"""
    out = np.array(P, dtype=np.float64)
    g = np.random.default_rng(seed)
    big = PAD_VALUES[bool(f32)]
    for i, n in enumerate(lens):
        tail = out[i, n:]
        if tail.shape[0] == 0 or variant == "walk":
            continue
        if variant in ("repeat", "nan+inf"):
            tail[:] = out[i, n - 1]
            if variant == "nan+inf":
                tail.reshape(-1)[0] = np.nan
                if tail.size > 1:
                    tail.reshape(-1)[-1] = np.inf
        elif variant == "garbage37":
            tail[:] = 37.0 * g.standard_normal(tail.shape)
        elif variant == "+-1.5e308":
            tail[:] = big[2] * np.where(np.arange(tail.shape[0]) % 2 == 0, 1.0, -1.0)[:, None]
        else:
            tail[:] = big[PADDINGS.index(variant) - 3]
    if f32:
        with np.errstate(over="ignore"):
            out = out.astype(np.float32).astype(np.float64)
        assert variant == "nan+inf" or np.all(np.isfinite(out))
    return out


CASES = cases()
CASE_BY_ID = {case_id(c): c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)
