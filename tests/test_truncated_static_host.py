"""TruncatedSigKernel(static_kernel=...) without a GPU: the torch restatement on second differences of a static kernel's Gram against an
independent evaluation in long double, the closed form of level 1, the unchanged default, gradients, duck-typed and function-valued
kernels, tiling, and the rows of the route rule.

THE YARDSTICK (``ld_levels``): the reference has no kernelised truncated kernel, so the recursion stated at the top of
csrc/sk_truncated.hip is evaluated here in plain numpy loops in ``np.longdouble`` -- explicit prefix sums over nodes and planes, G from
differences of coordinates -- sharing no code with sigkernel_amd/truncated.py.  Level terms are signed and shrink factorially (9 x 7
points, level 6: 2e-9), so an error is judged PER LEVEL against ``scale[m] = max over pairs of sum_{nodes, planes} |R^m|``, never against
``max(|want|, 1)``.  ``err_ref`` -- the distance of the fp64 restatement from the loops in those units -- is what the GPU tests build their
bar from (test_gpu_truncated_static.py).

Shapes are (A, B, Mp, Np, D) with Mp, Np in POINTS."""
import numpy as np
import pytest
import torch

LD = np.longdouble
SHAPE = (2, 3, 9, 7, 3)


def walks(rng, n, points, D, dtype=np.float64):
    """n random walks of `points` points, step std 0.5"""
    return np.cumsum(0.5 * rng.standard_normal((n, points, D)), axis=1).astype(dtype)


def rbf_ld(s):
    """kappa(x, y) = exp(-|x - y|^2 / s) of point sets x (M, D), y (N, D) -> (M, N), from differences of coordinates"""
    def kappa(x, y):
        e = x[:, None, :] - y[None, :, :]
        return np.exp(-(e * e).sum(2) / LD(s))
    return kappa


def poly_ld(x, y):
    """the duck-typed test kernel below: (1 + <x, y> / 4)^2"""
    return (1 + (x[:, None, :] * y[None, :, :]).sum(2) / LD(4)) ** 2


def _excl_rows(T):
    out = np.zeros_like(T)
    for i in range(1, T.shape[0]):
        out[i] = out[i - 1] + T[i - 1]
    return out


def _excl_cols(T):
    out = np.zeros_like(T)
    for j in range(1, T.shape[1]):
        out[:, j] = out[:, j - 1] + T[:, j - 1]
    return out


def _pair_levels(x, y, kappa, L, order):
    """one pair: ([k_1 .. k_L], [sum |R^m|]) in long double"""
    K = kappa(x.astype(LD), y.astype(LD))
    M, N = K.shape[0] - 1, K.shape[1] - 1
    G = np.zeros((M, N), dtype=LD)
    for i in range(M):
        for j in range(N):
            G[i, j] = K[i + 1, j + 1] - K[i + 1, j] - K[i, j + 1] + K[i, j]
    R = [[G]]
    ks, mags = [], []
    for m in range(1, L + 1):
        ks.append(sum(R[p][q].sum() for p in range(len(R)) for q in range(len(R))))
        mags.append(sum(np.abs(R[p][q]).sum() for p in range(len(R)) for q in range(len(R))))
        if m == L:
            break
        d, dn = len(R), min(m + 1, order)
        nxt = [[None] * dn for _ in range(dn)]
        for p in range(dn):
            for q in range(dn):
                if p == 0 and q == 0:
                    total = np.zeros((M, N), dtype=LD)
                    for pp in range(d):
                        for qq in range(d):
                            total = total + R[pp][qq]
                    nxt[0][0] = G * _excl_rows(_excl_cols(total))
                elif p == 0:
                    col = np.zeros((M, N), dtype=LD)
                    for pp in range(d):
                        col = col + R[pp][q - 1]
                    nxt[0][q] = G * _excl_rows(col) / LD(q + 1)
                elif q == 0:
                    row = np.zeros((M, N), dtype=LD)
                    for qq in range(d):
                        row = row + R[p - 1][qq]
                    nxt[p][0] = G * _excl_cols(row) / LD(p + 1)
                else:
                    nxt[p][q] = G * R[p - 1][q - 1] / LD((p + 1) * (q + 1))
        R = nxt
    return ks, mags


def ld_levels(X, Y, kappa, L, order, paired=False):
    """-> (levels (L + 1, A, B) -- paired (L + 1, P) -- in long double with levels[0] = 1, scale (L + 1,) with scale[0] = 1).
    X (A, Mp, D), Y (B, Np, D): numpy POINTS; order < 1: L."""
    order = L if order < 1 else order
    A, B = X.shape[0], Y.shape[0]
    pairs = [(a, a) for a in range(A)] if paired else [(a, b) for a in range(A) for b in range(B)]
    lev = np.ones((L + 1, len(pairs)), dtype=LD)
    scale = np.zeros(L + 1, dtype=LD)
    scale[0] = 1
    for n, (a, b) in enumerate(pairs):
        ks, mags = _pair_levels(X[a], Y[b], kappa, L, order)
        for m in range(1, L + 1):
            lev[m, n] = ks[m - 1]
            scale[m] = max(scale[m], mags[m - 1])
    return (lev if paired else lev.reshape(L + 1, A, B)), scale


def level_errors(got, want, scale):
    """max over pairs of |got - want| / scale[m], per level -> (L + 1,) floats; a level that is exactly zero (more levels than steps) must
    be met exactly: 0, else inf"""
    got = np.asarray(got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else got, dtype=LD)
    diff = [np.max(np.abs(got[m] - want[m])) for m in range(len(scale))]
    return np.array([float(d / s) if s > 0 else (0.0 if d == 0 else np.inf) for d, s in zip(diff, scale)])


def restatement_levels(X, Y, static_kernel, L, order, paired=False, workspace_bytes=None):
    """the level terms of the torch restatement on CPU fp64 tensors, through the public object"""
    import sigkernel_amd
    tk = sigkernel_amd.TruncatedSigKernel(L, 1., order, workspace_bytes=workspace_bytes, static_kernel=static_kernel)
    return tk._levels(torch.as_tensor(X), torch.as_tensor(Y), paired, False)


def test_the_loops_reproduce_the_closed_form_of_level_one():
    """the yardstick's own check: level 1 telescopes, independently of the recursion"""
    rng = np.random.default_rng(11)
    A, B, Mp, Np, D = SHAPE
    X, Y = walks(rng, A, Mp, D), walks(rng, B, Np, D)
    lev, scale = ld_levels(X, Y, rbf_ld(1.0), 1, 1)
    for a in range(A):
        for b in range(B):
            K = rbf_ld(1.0)(X[a].astype(LD), Y[b].astype(LD))
            assert abs(lev[1, a, b] - (K[-1, -1] - K[-1, 0] - K[0, -1] + K[0, 0])) <= 1e-17 * float(scale[1]) * Mp * Np


@pytest.mark.parametrize("s", [1.0, 0.3])
@pytest.mark.parametrize("order,L", [(o, L) for L in (1, 4, 6) for o in (1, 2, 4, -1) if o <= L])
@pytest.mark.parametrize("paired", [False, True])
def test_restatement_against_the_long_double_loops(s, order, L, paired):
    """err_ref: the fp64 restatement's distance from the loops, per level in units of scale[m].  The bar: a level is a sum of Mp Np
    products of at most L factors G, each G a second difference of exp values of relative error <= 2^-52 (torch.exp, and
    RBFKernel.Gram_matrix's expansion of the distance: ~1e-15 absolute on kappa <= 1 at these coordinates), so 1e-13 of scale[m] holds
    with two digits to spare and fails for any term dropped or misplaced (the smallest is 1 / (Mp Np) of the scale)."""
    import sigkernel_amd
    rng = np.random.default_rng(100 + L)
    A, B, Mp, Np, D = SHAPE
    X, Y = walks(rng, A, Mp, D), walks(rng, A if paired else B, Np, D)
    want, scale = ld_levels(X, Y, rbf_ld(s), L, order, paired)
    got = restatement_levels(X, Y, sigkernel_amd.RBFKernel(s), L, order, paired)
    assert got.shape == want.shape
    err = level_errors(got, want, scale)
    print("err_ref s=%g order=%d L=%d paired=%d: %s" % (s, order, L, paired, " ".join("%.2e" % e for e in err)))
    assert err[0] == 0.0 and np.all(err <= 1e-13), err


def test_level_one_is_the_closed_form():
    import sigkernel_amd
    rng = np.random.default_rng(12)
    A, B, Mp, Np, D = SHAPE
    X, Y = walks(rng, A, Mp, D), walks(rng, B, Np, D)
    got = restatement_levels(X, Y, sigkernel_amd.RBFKernel(1.0), 1, 1)
    tk = sigkernel_amd.TruncatedSigKernel(1, 1., 1, static_kernel=sigkernel_amd.RBFKernel(1.0))
    K = tk.compute_Gram(torch.as_tensor(X), torch.as_tensor(Y))
    for a in range(A):
        for b in range(B):
            kap = rbf_ld(1.0)(X[a].astype(LD), Y[b].astype(LD))
            k1 = float(kap[-1, -1] - kap[-1, 0] - kap[0, -1] + kap[0, 0])
            assert abs(float(got[1, a, b]) - k1) <= 1e-14       # a sum of 48 differences of values <= 1
            assert abs(float(K[a, b]) - (1 + k1)) <= 1e-14


@pytest.mark.parametrize("static_kernel", ["none", "linear", "linear3"])
@pytest.mark.parametrize("method", ["compute_Gram", "compute_kernel", "compute_mmd"])
def test_linear_and_default_are_unchanged(static_kernel, method):
    """static_kernel=None, LinearKernel() and LinearKernel(scale=3.) ARE the object built without the keyword: torch.equal values and
    gradients"""
    import sigkernel_amd
    sk = {"none": None, "linear": sigkernel_amd.LinearKernel(), "linear3": sigkernel_amd.LinearKernel(scale=3.)}[static_kernel]
    rng = np.random.default_rng(13)
    X0, Y0 = torch.as_tensor(walks(rng, 3, 6, 2)), torch.as_tensor(walks(rng, 3, 5, 2))
    sigma = torch.tensor([0.5, 1.0, -0.7, 0.3], dtype=torch.float64)
    out = []
    for tk in (sigkernel_amd.TruncatedSigKernel(3, sigma, 2), sigkernel_amd.TruncatedSigKernel(3, sigma, 2, static_kernel=sk)):
        X, Y = X0.clone().requires_grad_(True), Y0.clone().requires_grad_(True)
        K = getattr(tk, method)(X, Y)
        (K * torch.arange(1, K.numel() + 1, dtype=K.dtype).reshape(K.shape)).sum().backward()
        out.append((K.detach(), X.grad, Y.grad))
    for u, v in zip(*out):
        assert torch.equal(u, v)


def test_positional_arguments_mean_what_they_meant():
    import sigkernel_amd
    tk = sigkernel_amd.TruncatedSigKernel(3, 0.5, 2, 1 << 20)
    assert (tk.num_levels, tk.sigma, tk.order, tk.workspace_bytes, tk.static_kernel) == (3, 0.5, 2, 1 << 20, None)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("method", ["compute_Gram", "compute_kernel"])
def test_gradcheck_of_the_restatement(order, method):
    import sigkernel_amd
    rng = np.random.default_rng(14)
    X = torch.as_tensor(walks(rng, 2, 4, 2)).requires_grad_(True)
    Y = torch.as_tensor(walks(rng, 2, 3, 2)).requires_grad_(True)
    sigma = torch.tensor([1.0, 0.8, -0.6, 0.9], dtype=torch.float64, requires_grad=True)

    def f(x, y, s):
        tk = sigkernel_amd.TruncatedSigKernel(3, s, order, static_kernel=sigkernel_amd.RBFKernel(1.0))
        return getattr(tk, method)(x, y)
    assert torch.autograd.gradcheck(f, (X, Y, sigma), eps=1e-6, atol=1e-8, rtol=1e-6)


class PolyKernel:
    """a duck-typed static kernel: (1 + <x, y> / 4)^2, with the two methods of static_kernels.py and nothing else"""

    def batch_kernel(self, X, Y):
        return (1 + torch.bmm(X, Y.transpose(1, 2)) / 4) ** 2

    def Gram_matrix(self, X, Y):
        return (1 + torch.matmul(X[:, None], Y[None].transpose(-1, -2)) / 4) ** 2


@pytest.mark.parametrize("paired", [False, True])
def test_duck_typed_kernel_matches_the_loops(paired):
    """bar: as test_restatement_against_the_long_double_loops -- the polynomial's values stay below 1e2 at these coordinates, its second
    differences carry <= 1e-14 absolute, and scale[m] >= 1 here, so 1e-12 of the scale holds and a misplaced term does not"""
    rng = np.random.default_rng(15)
    A, B, Mp, Np, D = SHAPE
    X, Y = walks(rng, A, Mp, D), walks(rng, A if paired else B, Np, D)
    want, scale = ld_levels(X, Y, poly_ld, 4, 2, paired)
    err = level_errors(restatement_levels(X, Y, PolyKernel(), 4, 2, paired), want, scale)
    print("duck-typed, paired=%d: %s" % (paired, err))
    assert np.all(err <= 1e-12), err


def test_function_valued_kernel_matches_the_loops():
    """RBF_ID_Kernel on paths (batch, T, Lx, d): the RBF lift of the flattened paths"""
    import sigkernel_amd
    rng = np.random.default_rng(16)
    X, Y = walks(rng, 2, 6, 4), walks(rng, 3, 5, 4)
    want, scale = ld_levels(X, Y, rbf_ld(2.0), 3, 1)
    tk = sigkernel_amd.TruncatedSigKernel(3, 1., 1, static_kernel=sigkernel_amd.RBF_ID_Kernel(2.0))
    got = tk._levels(torch.as_tensor(X).reshape(2, 6, 2, 2), torch.as_tensor(Y).reshape(3, 5, 2, 2), False, False)
    err = level_errors(got, want, scale)
    assert np.all(err <= 1e-13), err
    K = tk.compute_Gram(torch.as_tensor(X).reshape(2, 6, 2, 2), torch.as_tensor(Y).reshape(3, 5, 2, 2))
    assert torch.equal(K, got.sum(0))


@pytest.mark.parametrize("paired", [False, True])
def test_tiling_gives_the_same_values(paired):
    import sigkernel_amd
    rng = np.random.default_rng(17)
    A, B, Mp, Np, D = SHAPE
    X, Y = walks(rng, A, Mp, D), walks(rng, A if paired else B, Np, D)
    one = restatement_levels(X, Y, sigkernel_amd.RBFKernel(1.0), 4, 2, paired, workspace_bytes=1)
    whole = restatement_levels(X, Y, sigkernel_amd.RBFKernel(1.0), 4, 2, paired)
    assert torch.equal(one, whole)


def test_paths_of_one_point_keep_the_empty_case_rule():
    import sigkernel_amd
    tk = sigkernel_amd.TruncatedSigKernel(3, [2.0, 1.0, 1.0, 1.0], 1, static_kernel=sigkernel_amd.RBFKernel(1.0))
    K = tk.compute_Gram(torch.zeros(2, 1, 3, dtype=torch.float64), torch.ones(3, 4, 3, dtype=torch.float64))
    assert torch.equal(K, torch.full((2, 3), 2.0, dtype=torch.float64))


ROUTE_ROWS = [
    # (order, D, Mp, Np, L) -> route; 1 FUSED, 4 FUSED_SWAP, 0 STREAM
    ((1, 8, 128, 128, 8), 1), ((1, 8, 129, 128, 8), 4), ((1, 8, 129, 129, 8), 0),     # 128 / 129 points on the first side
    ((1, 16, 128, 128, 8), 1), ((1, 17, 128, 128, 8), 0),                            # dim 16 / 17
    ((1, 8, 128, 256, 8), 1), ((1, 8, 128, 257, 8), 0),                              # 256 / 257 second-side points at dim <= 8
    ((1, 9, 128, 128, 8), 1), ((1, 9, 128, 129, 8), 0),                              # 128 / 129 at dim 9 .. 16
    ((1, 8, 128, 128, 9), 0),                                                        # 8 / 9 levels
    ((1, 3, 2, 2, 1), 1), ((1, 3, 1, 2, 1), 0), ((1, 3, 2, 1, 1), 0),                # one step a side; a path of one point
    ((-1, 3, 9, 7, 1), 1),                                                           # order -1 at one level IS order 1
    # orders 2 .. 4 stay with the restatement: the mode does not fit k_trunc_sig<4, 1> under 256 registers
    ((2, 3, 64, 64, 4), 0), ((2, 3, 65, 64, 4), 0), ((4, 3, 9, 7, 4), 0), ((-1, 3, 9, 7, 4), 0),
]


@pytest.mark.parametrize("row,want", ROUTE_ROWS)
def test_route_rows_of_the_points_mode(row, want):
    from sigkernel_amd import _lib
    order, D, Mp, Np, L = row
    q = _lib.load().sk_route_query
    assert q(_lib.OP_TRUNCATED_RBF, order, D, Mp, Np, L, 0, 8, 0) == want
    assert q(_lib.OP_TRUNCATED_RBF, order, D, Mp, Np, L, 0, 4, 0) == want
    assert q(_lib.OP_TRUNCATED_RBF, order, D, Mp, Np, L, 0, 2, 0) == 0


def test_the_existing_truncated_rows_answer_what_they_answered():
    from sigkernel_amd import _lib
    q = _lib.load().sk_route_query
    for row, want in [((1, 8, 128, 128, 8), 1), ((1, 8, 129, 128, 8), 4), ((2, 8, 64, 64, 8), 1), ((2, 8, 65, 64, 8), 4), ((2, 8, 65, 65, 8), 0),
                      ((4, 16, 64, 128, 8), 1), ((5, 3, 9, 7, 8), 0), ((1, 3, 1, 1, 1), 1), ((1, 17, 9, 7, 2), 0), ((1, 8, 9, 257, 2), 0)]:
        order, D, M, N, L = row
        assert q(_lib.OP_TRUNCATED, order, D, M, N, L, 0, 8, 0) == want, row
    for row, want in [((1, 8, 128, 128, 8), 1), ((1, 9, 128, 128, 8), 0), ((2, 8, 64, 64, 8), 0), ((1, 8, 129, 128, 8), 0)]:
        order, D, M, N, L = row
        assert q(_lib.OP_TRUNCATED_ADJOINT, order, D, M, N, L, 0, 8, 0) == want, row


def test_the_c_entry_point_checks_its_arguments_without_a_device():
    import ctypes
    from sigkernel_amd import _lib
    lib, p = _lib.load(), ctypes.c_void_p(16)
    sig = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
    args = (p, p, 1, 1, 4, 4, 4, 16, 3, 8, 2, 1)
    assert lib.sk_truncated_points_f64(*args, 2, 1.0, 0, 0, sig, p, None) == 1         # kind 2
    assert lib.sk_truncated_points_f64(*args, 1, 0.0, 0, 0, sig, p, None) == 1         # 1 / sigma must be positive
    assert lib.sk_truncated_points_f64(*args, 1, 1.0, 0, 0, None, p, None) == 1        # weights missing outside the levels mode
    assert lib.sk_truncated_points_f64(p, p, 1, 1, 4, 4, 4, 16, 3, 8, 2, 2, 1, 1.0, 0, 0, sig, p, None) == 2     # order 2: not covered
    assert lib.sk_truncated_points_f32(p, p, 1, 1, 129, 129, 4, 16, 3, 8, 2, 1, 1, 1.0, 0, 1, None, p, None) == 2   # 129 points
    assert lib.sk_version() == 340
