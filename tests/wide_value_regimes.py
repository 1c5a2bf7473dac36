"""Paths of more than 32 dims, launch by launch: the case table of tests/test_wide_value_regimes_host.py and
tests/test_gpu_wide_value_regimes.py (test infrastructure; numpy and torch on the CPU only -- nothing here imports the product package).

Beyond HipBackend.MAX_FUSED_DIM the static kernel, its increments and the first pass of the RBF chain rule are one kernel,
k_static_wide_mfma (sk_static.hip), with three run-time epilogues; the GPU half calls

    be.static_increments(kind, param, X, Y, gram)            WIDE_LINEAR (kind 0) / WIDE_RBF (kind 1)
    be.static_adjoint(kind, param, X, Y, W, go, gram)         WIDE_RBF_ADJ + the second pass in torch (kind 1); a GEMM of W with dY (kind 0)

directly, on the families of tests/value_regimes.py (unchanged; LinearKernel's s = 10 is left out: no rescue at this level), against
value_regimes.increments_ld and value_regimes._chain_ld on W * go -- both in long double, both from coordinate differences.

GEOMETRIES puts every tiling boundary of the kernel in play without a cross product: M - 1 = 63 (one RBF tile exactly), 64 (one linear
/ adjoint tile, the first row of a second RBF tile), 126 (two RBF tiles exactly), N = 129 (three RBF column tiles; a third adjoint
column tile of one node), y-groups of WD_NB = 4 paths filled exactly, twice, with a tail of one, and the paired mode; D gives chunk
tails (WD_KC = 8 dims, two per thread) of 1, 2, 7, 0, 1 and 0 dims.  Every family case meets two geometries per mode, `offset` meets
all of them.

The bound is the project's one rule, base + 4 r:
    increments    base = 1e-13 max(1, max |G|)   (tests/test_gpu_wide.py's)     G: the RBF node matrix; LinearKernel: see `scale_of`
    chain rule    base = 1e-8 in value_regimes.grad_error's measure             (the ledger's fp64 gradient tolerance)
    r             the recorded distance of the REFERENCE's arithmetic from the yardstick on that case (tests/golden/
                  wide_value_regimes.json, written by tests/golden/measure_wide_value_regimes.py: the _Linear / _RBF restatements of
                  measure_value_regimes.py, differenced in fp64 on the CPU, with their autograd chain rule); `offset`: the maximum over
                  value_regimes.OFFSET_SEEDS seeds
    fp32          yardstick on the fp32-rounded inputs, instance_ledger.F32_ULPS2 on top
LinearKernel gets base ALONE on every offset case, values and gradient: WIDE_LINEAR stages s^2 (x[p+1][k] - x[p][k]) and the same of y
(sk_static.hip:1165, `fetch`), and the chain rule is the library GEMM of W with Y[:, 1:] - Y[:, :-1] (_lib.py:1397) -- a common offset
never reaches a product.  RBFKernel is not invariant by construction (sk_static.hip:1260: |x|^2 + |y|^2 - 2 <x, y>; _lib.py:1414:
H @ Y - rowsum(H) X) and gets the allowance.
"""
import functools

import numpy as np

import value_regimes as V
from value_regimes import LD

INC_BASE = 1e-13
GRAD_BASE = V.BASE_TOL["grad"]
MODES = ("inc", "adj")
SUBNORMAL_LIMIT = -745.2        # exponents below it give exactly 0 (tests/test_gpu_value_regimes.py::test_gpu_exp_probe)


def geometry(A, B, M, N, D, gram=True):
    assert gram or A == B
    return {"A": A, "B": B, "M": M, "N": N, "D": D, "gram": bool(gram)}


# (A, B) x (M, N) x D -- each listed value of the three once, the large shapes on the small batches
GEOMETRIES = [
    geometry(2, 1, 2, 2, 72),
    geometry(1, 4, 64, 65, 33),
    geometry(2, 5, 65, 64, 34),
    geometry(1, 8, 127, 3, 39),
    geometry(3, 3, 66, 129, 40, gram=False),
    geometry(2, 1, 64, 65, 41),
    geometry(3, 3, 65, 64, 72, gram=False),
]


def geometry_key(g, f32=False):
    return "%s%dx%d_%dx%d_D%d%s" % ("" if g["gram"] else "paired", g["A"], g["B"], g["M"], g["N"], g["D"], "_f32" if f32 else "")


def _shape(g, f32):
    return V.shape(g["A"], g["B"], g["M"], g["N"], g["D"], 0, f32=f32)


def cases():
    """[(mode, kind, family, label, settings, geometry, f32)]: fp64 on every family (two geometries each, `offset` all of them), fp32 on
    drift and scale (one geometry each).  A drift case needs N >= 8 points (value_regimes.drift_schedule)."""
    out = []
    for mi, mode in enumerate(MODES):
        for kind in V.KINDS:
            fams = [c for c in V.family_cases(kind) if not c[2].get("wild")]
            for i, (fam, lab, st) in enumerate(fams):
                ok = [g for g in GEOMETRIES if fam != "drift" or g["N"] >= 8]
                picked = ok if fam == "offset" else [ok[(i + mi) % len(ok)], ok[(i + mi + len(ok) // 2) % len(ok)]]
                out += [(mode, kind, fam, lab, st, g, False) for g in picked]
                if fam in ("drift", "scale"):
                    out.append((mode, kind, fam, lab, st, ok[(i + mi + 1) % len(ok)], True))
    return out


def case_key(c):
    mode, kind, fam, lab, st, g, f32 = c
    return "%s|%s|%s|%s|%s" % (mode, kind, fam, lab, geometry_key(g, f32))


def case_id(c):
    return case_key(c).replace("|", "-")


# ------------------------------------------------------------------------------------------------------------------- inputs
def inputs(c, seed=0):
    """-> X (A,M,D), Y (B,N,D), W (P.., M-1, N-1), go (P..) numpy fp64 (fp32-rounded for an fp32 case), sigma or None.  W and go are
    standard normal, as in tests/test_gpu_wide.py."""
    import torch
    mode, kind, fam, lab, st, g, f32 = c
    X, Y, _, sigma = V.inputs(st, _shape(g, f32), seed)
    gen = torch.Generator().manual_seed(1000 + int(seed))
    P = (g["A"], g["B"]) if g["gram"] else (g["A"],)
    W = torch.randn(P + (g["M"] - 1, g["N"] - 1), generator=gen, dtype=torch.float64).numpy()
    go = torch.randn(P, generator=gen, dtype=torch.float64).numpy()
    if f32:
        W, go = W.astype(np.float32).astype(np.float64), go.astype(np.float32).astype(np.float64)
    return X, Y, W, go, sigma


@functools.lru_cache(maxsize=None)
def _cached_inputs(key):
    out = inputs(CASE_BY_KEY[key])
    for a in out[:4]:
        a.setflags(write=False)
    return out


def case_inputs(c):
    return _cached_inputs(case_key(c))


# ------------------------------------------------------------------------------------------------------------------- yardstick
def _pairs(g):
    return [(a, b) for a in range(g["A"]) for b in range(g["B"])] if g["gram"] else [(a, a) for a in range(g["A"])]


def increments_ld(kind, sigma, X, Y, gram):
    """value_regimes.increments_ld for a Gram batch (A,B,M-1,N-1) or a paired one (A,M-1,N-1) -> (increments, nodes or None)"""
    if gram:
        return V.increments_ld(kind, sigma, X, Y)
    per = [V.increments_ld(kind, sigma, X[a:a + 1], Y[a:a + 1]) for a in range(X.shape[0])]
    return np.stack([p[0][0, 0] for p in per]), (None if kind == "linear" else np.stack([p[1][0, 0] for p in per]))


def chain_ld(kind, sigma, X, Y, G, W, go, gram):
    """value_regimes._chain_ld on W * go -> dL/dX (A,M,D)"""
    Ww = W.astype(LD) * go.astype(LD)[..., None, None]
    if gram:
        return V._chain_ld(kind, sigma, X, Y, G, Ww)
    return np.concatenate([V._chain_ld(kind, sigma, X[a:a + 1], Y[a:a + 1], None if G is None else G[a][None, None], Ww[a][None, None])
                           for a in range(X.shape[0])])


def scale_of(kind, inc, G):
    """max(1, max |G|) of the increments' bound.  RBF: G is the node matrix (<= 1).  LinearKernel: the node Gram <x, y> grows with the
    square of a common offset (3e9 at c = 1e4) and would make the bound on offset paths empty, so the largest INCREMENT |<dx, dy>| stands
    in for it -- never larger than the node Gram's entries it is the corner difference of, up to the factor 4."""
    return max(1.0, float(np.max(np.abs(inc if G is None else G))))


def increments_error(got, want, scale):
    got = np.asarray(got).astype(LD)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.all(np.isfinite(got.astype(np.float64))):
        return float("inf")
    return float(np.max(np.abs(got - want))) / scale


@functools.lru_cache(maxsize=None)
def _cached_want(key):
    c = CASE_BY_KEY[key]
    mode, kind, fam, lab, st, g, f32 = c
    X, Y, W, go, sigma = case_inputs(c)
    inc, G = increments_ld(kind, sigma, X, Y, g["gram"])
    if mode == "inc":
        return inc, G
    return chain_ld(kind, sigma, X, Y, G, W, go, g["gram"]), G


def case_want(c):
    """inc mode: (increments, nodes); adj mode: (dL/dX, nodes) -- the yardstick's, once per process"""
    return _cached_want(case_key(c))


# ------------------------------------------------------------------------------------------------------------------- the reference's arithmetic
@functools.lru_cache(maxsize=None)
def _measure_module():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("measure_value_regimes", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                                                                        "measure_value_regimes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_arithmetic(kind, sigma, X, Y, W, go, gram):
    """The reference's static kernels as measure_value_regimes.py restates them (nodes from the POINTS: <x, y>, |x|^2 + |y|^2 - 2 <x, y>),
    differenced in fp64, and autograd's chain rule through them -> (increments, dL/dX) numpy fp64"""
    import torch
    k = _measure_module().static_kernel(kind, sigma)
    Xt, Yt = torch.from_numpy(np.array(X)).requires_grad_(True), torch.from_numpy(np.array(Y))
    G = k.Gram_matrix(Xt, Yt)
    if not gram:
        G = G[torch.arange(X.shape[0]), torch.arange(X.shape[0])]
    inc = G[..., 1:, 1:] + G[..., :-1, :-1] - G[..., 1:, :-1] - G[..., :-1, 1:]
    (g,) = torch.autograd.grad(inc, Xt, torch.from_numpy(W * go[..., None, None]))
    return inc.detach().numpy(), g.numpy()


def reference_distance(c, seed=0):
    """r of one case and seed, in the measure of its mode"""
    mode, kind, fam, lab, st, g, f32 = c
    X, Y, W, go, sigma = inputs(c, seed)
    ref_inc, ref_g = reference_arithmetic(kind, sigma, X, Y, W, go, g["gram"])
    inc, G = increments_ld(kind, sigma, X, Y, g["gram"])
    if mode == "inc":
        return increments_error(ref_inc, inc, scale_of(kind, inc, G))
    return V.grad_error(ref_g, chain_ld(kind, sigma, X, Y, G, W, go, g["gram"]))


def measure(c):
    mode, kind, fam = c[:3]
    return max(reference_distance(c, seed) for seed in (range(V.OFFSET_SEEDS) if fam == "offset" else (0,)))


def invariant(c):
    """LinearKernel on offset paths: base alone (module docstring)"""
    return c[1] == "linear" and c[2] == "offset"


def tolerance(c, recorded, scale=1.0):
    """the bound of a case; increments: in units of `scale` = scale_of(...) already divided out by increments_error"""
    from instance_ledger import F32_ULPS2
    base = (INC_BASE if c[0] == "inc" else GRAD_BASE) + (F32_ULPS2 if c[6] else 0.0)
    return base if invariant(c) else base + 4.0 * recorded[case_key(c)]


CASES = cases()
CASE_BY_KEY = {case_key(c): c for c in CASES}
assert len(CASE_BY_KEY) == len(CASES)


# ------------------------------------------------------------------------------------------------------------------- exact claims
def restate(kind, sigma, X, Y):
    """The wide kernel's arithmetic restated in numpy fp64 for the exact claims on the CPU (Gram batches): WIDE_LINEAR's <dx, dy> from
    differenced paths; WIDE_RBF's exp(-(|x|^2 + |y|^2 - 2 <x, y>) / sigma) at the nodes, four-corner differenced."""
    with np.errstate(all="ignore"):
        if kind == "linear":
            return np.einsum("ipk,jqk->ijpq", np.diff(X, axis=1), np.diff(Y, axis=1))
        xy = np.einsum("ipk,jqk->ijpq", X, Y)
        d2 = -2.0 * xy + ((X * X).sum(-1)[:, None, :, None] + (Y * Y).sum(-1)[None, :, None, :])
        G = np.exp(-d2 / sigma)
        return ((G[..., 1:, 1:] + G[..., :-1, :-1]) - G[..., 1:, :-1]) - G[..., :-1, 1:]


EXACT_GEOMETRY = geometry(2, 5, 65, 66, 40)      # two y-groups, a second row tile, M - 1 on the linear tile's edge
REPEAT_X, REPEAT_Y = (1, 63), (4, 64)            # (path, point p): x[p + 1] = x[p] -- the last row of the first tile; y: the first column of the second
BAD_X, BAD_Y, BAD_DIM = (1, 64), (4, 63), 37     # (path, node) given a NaN or an inf coordinate (a dim of the last, partial chunk)


def exact_inputs(seed=5):
    """unit walks moved to positive coordinates (so that an inf coordinate meets |x|^2 - 2 <x, y> = inf - inf, as in the reference)"""
    g = EXACT_GEOMETRY
    X, Y, _, _ = V.inputs({}, _shape(g, False), seed)
    _, _, W, go, _ = inputs(("adj", "rbf", "sigma", "", {}, g, False), seed)
    return X + 3.0, Y + 3.0, W, go


def touched(M, N, g, side, path, node):
    """masks of what a non-finite coordinate in node `node` of x_path (side "X") or y_path ("Y") must reach:
    -> (increments (A,B,M-1,N-1) bool, RBF gradient rows (A,M) bool, LinearKernel gradient rows (A,M) bool).
    Increments: the two rows (columns) around the node, in every pair of that path.  RBF dL/dX: row `node` of x_path (H's row), or every
    row of every x (H's column n of every pair with y_path).  LinearKernel dL/dX = W @ dY does not read X at all; a bad y reaches every
    row of every x (in coordinate BAD_DIM)."""
    A, B = g["A"], g["B"]
    inc, rbf, lin = np.zeros((A, B, M - 1, N - 1), bool), np.zeros((A, M), bool), np.zeros((A, M), bool)
    if side == "X":
        inc[path, :, max(node - 1, 0):node + 1] = True
        rbf[path, node] = True
    else:
        inc[:, path, :, max(node - 1, 0):node + 1] = True
        rbf[:], lin[:] = True, True
    return inc, rbf, lin


def dead_increments(X, Y, sigma, gram):
    """the increments whose four nodes all have an exponent below SUBNORMAL_LIMIT (by the long-double exponents): exactly 0"""
    if gram:
        low = V.exponents_ld(X, Y, sigma) < SUBNORMAL_LIMIT
    else:
        low = np.stack([V.exponents_ld(X[a:a + 1], Y[a:a + 1], sigma)[0, 0] for a in range(X.shape[0])]) < SUBNORMAL_LIMIT
    return low[..., 1:, 1:] & low[..., :-1, :-1] & low[..., 1:, :-1] & low[..., :-1, 1:]


# ------------------------------------------------------------------------------------------------------------------- function-valued kernels
# Through the API on 4-D paths (batch, T, Lx = 12, d = 3): 36 flattened dims (RBF_ID_Kernel), 72 features (RBF_SQR_Kernel) -- the wide
# route.  `scale` and `offset` families of RBFKernel, sigma = sigma1 = 0.8; RBF_SQR_Kernel's second bandwidth is 0.8 on `scale` and
# 0.8 (2 c)^2 on `offset` (x^2 - y^2 = (x - y)(x + y) is 2 c times the difference there: the second factor stays a kernel, not a zero).
FV_SHAPE = V.shape(3, 3, 20, 17, 36, 1)
FV_LX, FV_D = 12, 3
FV_CASES = [(cls, fam, lab, st) for cls in ("rbf_id", "rbf_sqr") for fam, lab, st in V.family_cases("rbf", ("scale", "offset"))]


def fv_key(c, name):
    return "fv-%s|%s|%s|%s" % (name, c[0], c[1], c[2])


def fv_outputs(c):
    return ("value", "grad") if c[0] == "rbf_id" else ("value",)


def fv_sigma2(st):
    return 0.8 * max(1.0, (2.0 * st.get("offset", (0.0, 0.0))[0]) ** 2)


def fv_inputs(c, seed=0):
    """-> X (A,T,36), Y (B,T',36), w (A,B): the flattened paths (the API gets them reshaped to (.., 12, 3))"""
    return V.inputs(c[3], FV_SHAPE, seed)[:3]


def fv_yardstick(c, X, Y, w):
    """the class's own formula in long double from differences, fed to solve_diag_ld -> (K, dL/dX or None)"""
    cls, fam, lab, st = c
    if cls == "rbf_id":      # RBFKernel on the flattened paths
        return V.gram_ld("rbf", st["sigma"], X, Y, FV_SHAPE["d"], w)
    diff = X.astype(LD)[:, None, :, None, :] - Y.astype(LD)[None, :, None, :, :]
    summ = X.astype(LD)[:, None, :, None, :] + Y.astype(LD)[None, :, None, :, :]
    sq = diff * summ      # x^2 - y^2
    G = np.exp(-(diff * diff).sum(-1) / LD(st["sigma"]) - (sq * sq).sum(-1) / LD(fv_sigma2(st)))
    return V.solve_diag_ld(V.tile(V._corner(G), FV_SHAPE["d"]))[..., -1, -1], None


class _SQR:
    """RBF_SQR_Kernel's torch formula, rbf1(X) * rbf2(X ** 2) (static_kernels.py), on measure_value_regimes' _RBF"""

    def __init__(self, sigma1, sigma2):
        self.rbf1, self.rbf2 = _measure_module().static_kernel("rbf", sigma1), _measure_module().static_kernel("rbf", sigma2)

    def Gram_matrix(self, X, Y):
        return self.rbf1.Gram_matrix(X, Y) * self.rbf2.Gram_matrix(X ** 2, Y ** 2)


def fv_reference_distance(c, seed=0):
    """the oracle on the class's torch formula in fp64 against the yardstick -> {"value", "grad"}"""
    import torch
    cls, fam, lab, st = c
    X, Y, w = fv_inputs(c, seed)
    if cls == "rbf_id":
        return _measure_module().oracle_distance("rbf", X, Y, w, st["sigma"], FV_SHAPE["d"])
    K, _ = fv_yardstick(c, X, Y, w)
    got = _measure_module().O.gram_forward(torch.from_numpy(X), torch.from_numpy(Y), _SQR(st["sigma"], fv_sigma2(st)), FV_SHAPE["d"])
    return {"value": V.value_error(got, K)}


def fv_measure(c):
    ds = [fv_reference_distance(c, seed) for seed in (range(V.OFFSET_SEEDS) if c[1] == "offset" else (0,))]
    return {fv_key(c, name): max(d[name] for d in ds) for name in fv_outputs(c)}


FV_KEYS = [fv_key(c, name) for c in FV_CASES for name in fv_outputs(c)]
