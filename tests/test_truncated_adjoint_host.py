"""The gradient of the truncated signature kernel without a GPU: the closed form the HIP adjoint sweep evaluates (csrc/sk_truncated.hip:
trunc_adjoint), restated here in torch and held against autograd of the torch restatement; TruncatedSigKernel on CPU tensors, where it
takes the torch route as a whole; and the SK_OP_TRUNCATED_ADJOINT rows of the route table.

Order 1, G[i, j] = <x_i, y_j>:  R^1 = G,  R^{m+1} = G * P^m with P^m the exclusive 2-D prefix of R^m (P^0 = 1),  k_m = sum R^m.  For
weights w_1 .. w_L of a pair's level terms
    Rb^L = w_L,   Rb^m = w_m + (exclusive 2-D SUFFIX of G * Rb^{m+1}),   dG = sum_m Rb^m * P^{m-1},
    dX[a, i] = sum_b sum_j dG_ab[i, j] Y[b, j],   dY[b, j] = sum_a sum_i dG_ab[i, j] X[a, i]."""
import numpy as np
import pytest
import torch

from test_truncated_host import steps


def _excl(t, dim):
    c = torch.cumsum(t, dim)
    return torch.cat([torch.zeros_like(c.narrow(dim, 0, 1)), c.narrow(dim, 0, c.shape[dim] - 1)], dim)


def _excl_suffix(t, dim):
    return _excl(t.flip(dim), dim).flip(dim)


def closed_form(X, Y, w):
    """(dX, dY) of sum_{m, a, b} w[m - 1, a, b] k_m(X[a], Y[b]) for X (A, M, D), Y (B, N, D), w (L, A, B)"""
    L = w.shape[0]
    G = torch.einsum("aid,bjd->abij", X, Y)
    P, R = [torch.ones_like(G)], G
    for _ in range(1, L):
        P.append(_excl(_excl(R, -2), -1))
        R = G * P[-1]
    Rb = w[L - 1][:, :, None, None] * torch.ones_like(G)
    dG = Rb * P[L - 1]
    for m in range(L - 1, 0, -1):
        Rb = w[m - 1][:, :, None, None] + _excl_suffix(_excl_suffix(G * Rb, -2), -1)
        dG = dG + Rb * P[m - 1]
    return torch.einsum("abij,bjd->aid", dG, Y), torch.einsum("abij,aid->bjd", dG, X)


def autograd_gradients(X, Y, w):
    """the same by autograd of the torch restatement; w (L + 1, A, B): level 0 is the constant 1 and takes no gradient"""
    from sigkernel_amd.truncated import _truncated_levels_torch
    X, Y = X.clone().requires_grad_(), Y.clone().requires_grad_()
    (w * _truncated_levels_torch(X, Y, w.shape[0] - 1, 1)).sum().backward()
    return X.grad, Y.grad


SHAPES = [(3, 2, 5, 7, 3, 4), (2, 3, 9, 4, 2, 8), (1, 1, 1, 1, 1, 1), (2, 2, 3, 3, 2, 2), (2, 3, 128, 65, 8, 8)]


@pytest.mark.parametrize("A,B,M,N,D,L", SHAPES)
def test_closed_form_is_the_gradient_of_the_restatement(A, B, M, N, D, L):
    """The closed form against autograd of _truncated_levels_torch: <= 1e-13 of each gradient's max-norm.  Measured at
    (2, 3, 128, 65, 8, 8): 2.1e-15 in dX and 1.5e-15 in dY -- below the 1e-12 the GPU test's 1e-10 bar needs of its reference."""
    rng = np.random.default_rng(100 * M + N + L)
    X, Y = torch.as_tensor(steps(rng, A, M, D)), torch.as_tensor(steps(rng, B, N, D))
    w = torch.as_tensor(rng.standard_normal((L + 1, A, B)))
    dX, dY = closed_form(X, Y, w[1:])
    wX, wY = autograd_gradients(X, Y, w)
    for name, got, want in (("dX", dX, wX), ("dY", dY, wY)):
        err = float((got - want).abs().max() / want.abs().max())
        print("closed form vs autograd %s %s: %.2e" % ((A, B, M, N, D, L), name, err))
        assert err <= 1e-13, (name, err)


def paths(rng, n, m, D, dtype=np.float64):
    return np.cumsum(steps(rng, n, m, D, dtype), axis=1, dtype=dtype)


@pytest.mark.parametrize("order", [1, 2, -1])
def test_truncated_sig_kernel_object_on_cpu_tensors(order):
    from sigkernel_amd import TruncatedSigKernel
    from sigkernel_amd.truncated import _truncated_torch, _truncated_paired_torch
    rng = np.random.default_rng(3)
    X, Y = torch.as_tensor(paths(rng, 4, 7, 3)), torch.as_tensor(paths(rng, 3, 6, 3))
    sigma = torch.as_tensor(rng.uniform(0.5, 1.5, 5))
    tk = TruncatedSigKernel(4, sigma, order)
    dX, dY = X[:, 1:] - X[:, :-1], Y[:, 1:] - Y[:, :-1]
    K = tk.compute_Gram(X, Y)
    assert K.shape == (4, 3) and torch.allclose(K, _truncated_torch(dX, dY, 4, sigma, order), rtol=1e-13, atol=0)
    assert torch.allclose(tk.compute_Gram(X, X, sym=True), _truncated_torch(dX, dX, 4, sigma, order), rtol=1e-13, atol=0)
    k = tk.compute_kernel(X[:3], Y)
    assert k.shape == (3,) and torch.allclose(k, _truncated_paired_torch(dX[:3], dY, 4, sigma, order), rtol=1e-13, atol=0)
    # the estimator written out: means of K_XX and K_YY without their diagonals, minus twice the mean of K_XY
    KXX, KYY = _truncated_torch(dX, dX, 4, sigma, order), _truncated_torch(dY, dY, 4, sigma, order)
    want = (KXX.sum() - KXX.diag().sum()) / (4 * 3.) + (KYY.sum() - KYY.diag().sum()) / (3 * 2.) - 2. * K.mean()
    assert torch.allclose(tk.compute_mmd(X, Y), want, rtol=1e-12, atol=1e-15)
    # fp32 paths give fp32 values; a scalar sigma weighs every level alike
    K32 = TruncatedSigKernel(4, 0.9, order).compute_Gram(X.float(), Y.float())
    assert K32.dtype == torch.float32
    assert torch.allclose(K32.double(), _truncated_torch(dX, dY, 4, 0.9, order), rtol=1e-4, atol=1e-5)


def test_truncated_sig_kernel_object_gradcheck():
    from sigkernel_amd import TruncatedSigKernel
    rng = np.random.default_rng(11)
    X = torch.as_tensor(paths(rng, 2, 4, 2)).requires_grad_()
    Y = torch.as_tensor(paths(rng, 2, 4, 2)).requires_grad_()
    sigma = torch.as_tensor(rng.uniform(0.5, 1.5, 4)).requires_grad_()
    for order in (1, -1):
        assert torch.autograd.gradcheck(lambda x, y, s: TruncatedSigKernel(3, s, order).compute_Gram(x, y), (X, Y, sigma), atol=1e-9, rtol=1e-7)
        assert torch.autograd.gradcheck(lambda x, y, s: TruncatedSigKernel(3, s, order).compute_kernel(x, y), (X, Y, sigma), atol=1e-9, rtol=1e-7)
        assert torch.autograd.gradcheck(lambda x, s: TruncatedSigKernel(3, s, order).compute_Gram(x, x, sym=True), (X, sigma), atol=1e-9, rtol=1e-7)
        assert torch.autograd.gradcheck(lambda x, y, s: TruncatedSigKernel(3, s, order).compute_mmd(x, y), (X, Y, sigma), atol=1e-9, rtol=1e-7)


def test_truncated_sig_kernel_object_argument_errors():
    """the checks and messages of truncated_sig_kernel (both go through truncated._check_args and _sigma_vector)"""
    from sigkernel_amd import TruncatedSigKernel
    X, Y = torch.rand(2, 5, 3, dtype=torch.float64), torch.rand(3, 4, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match=r"shape \(batch, length, dim\)"):
        TruncatedSigKernel(3).compute_Gram(X[0], Y)
    with pytest.raises(ValueError, match="same path dimension"):
        TruncatedSigKernel(3).compute_Gram(X, Y[:, :, :2])
    with pytest.raises(ValueError, match="share dtype and device"):
        TruncatedSigKernel(3).compute_Gram(X, Y.float())
    with pytest.raises(TypeError, match="float64 and float32"):
        TruncatedSigKernel(3).compute_Gram(X.half(), Y.half())
    with pytest.raises(ValueError, match="positive integer"):
        TruncatedSigKernel(0).compute_Gram(X, Y)
    with pytest.raises(ValueError, match="must be an integer"):
        TruncatedSigKernel(3, order=1.5).compute_Gram(X, Y)
    with pytest.raises(ValueError, match="must not exceed num_levels"):
        TruncatedSigKernel(3, order=4).compute_Gram(X, Y)
    with pytest.raises(ValueError, match="same number of paths"):
        TruncatedSigKernel(3).compute_kernel(X, Y)
    with pytest.raises(ValueError, match=r"num_levels \+ 1 = 4 values"):
        TruncatedSigKernel(3, sigma=[1., 2.]).compute_Gram(X, Y)
    with pytest.raises(ValueError, match="Y is X"):
        TruncatedSigKernel(3).compute_Gram(X, Y, sym=True)


def test_route_table_states_the_adjoint_scope():
    from sigkernel_amd import _lib
    from sigkernel_amd.truncated import truncated_route
    F, S, W = _lib.ROUTE_FUSED, _lib.ROUTE_STREAM, _lib.ROUTE_FUSED_SWAP
    q = lambda D, M, N, L, order, es=8: int(_lib.load().sk_route_query(_lib.OP_TRUNCATED_ADJOINT, order, D, M, N, L, 0, es, 0))
    assert _lib.OP_TRUNCATED_ADJOINT == 5
    assert q(8, 128, 256, 8, 1) == F and q(8, 128, 256, 8, 1, 4) == F and q(1, 1, 1, 1, 1) == F and q(3, 9, 6, 1, -1) == F
    assert q(9, 128, 256, 8, 1) == S          # two staging columns per step: the forward's scope, not the adjoint's
    assert q(8, 129, 256, 8, 1) == S          # never swapped: the other batch's gradient is the query on (N, M)
    assert q(8, 128, 256, 8, 2) == S and q(8, 64, 64, 4, -1) == S
    assert q(8, 128, 256, 9, 1) == S
    assert q(8, 128, 257, 8, 1) == S and q(8, 128, 256, 8, 1, 2) == S
    # SK_OP_TRUNCATED answers what it answered (the rows of test_truncated_host.py)
    for (D, M, N, L, order, es), want in {(8, 64, 64, 4, -1, 8): F, (8, 65, 64, 4, -1, 8): W, (8, 65, 65, 4, -1, 8): S, (8, 128, 128, 8, 1, 8): F,
                                          (8, 129, 128, 8, 1, 4): W, (8, 129, 130, 8, 1, 8): S, (16, 64, 128, 8, 4, 4): F, (16, 64, 129, 8, 4, 8): S,
                                          (17, 8, 8, 3, 1, 8): S, (4, 8, 8, 9, 1, 8): S, (4, 8, 8, 6, 5, 8): S, (4, 8, 8, 5, 5, 8): S,
                                          (4, 8, 8, 4, 4, 8): F, (1, 2, 3, 1, -1, 8): F, (8, 64, 256, 3, 2, 8): F, (8, 64, 257, 3, 2, 8): S,
                                          (4, 200, 40, 6, 3, 8): W, (4, 300, 40, 6, 3, 8): S}.items():
        assert truncated_route(D, M, N, L, order, es) == want, (D, M, N, L, order, es)


def test_adjoint_plan_splits_and_bounds_the_slab():
    """sk_truncated_adjoint_plan (host only): chunks of second paths fill the resident blocks, and the block count comes down until the
    slabs -- (L - 1) (N + lanes - 1) KB a block -- fit the workspace; one block that does not fit is UNSUPPORTED, one level needs none."""
    import ctypes
    from sigkernel_amd import _lib
    lib = _lib.load()

    def plan(A, B, M, N, D, L, paired, ws):
        out = (ctypes.c_int64 * 3)()
        rc = lib.sk_truncated_adjoint_plan(A, B, M, N, D, L, paired, ws, ctypes.cast(out, ctypes.c_void_p))
        return rc, tuple(out)

    rc, (chunks, blocks, slab) = plan(5, 37, 20, 33, 3, 6, 0, 1 << 30)      # 16 lanes a group, 4 groups: 2 row tiles
    assert rc == 0 and chunks == 37 and blocks == 74 and slab == 74 * 5 * (33 + 15) * 1024
    rc, (chunks, blocks, slab) = plan(5, 37, 20, 33, 3, 6, 0, 3 * 5 * 48 * 1024 + 5)
    assert rc == 0 and chunks == 37 and blocks == 3 and slab == 3 * 5 * 48 * 1024
    assert plan(5, 37, 20, 33, 3, 6, 0, 5 * 48 * 1024 - 1)[0] == 2
    rc, (chunks, blocks, slab) = plan(5, 37, 20, 33, 3, 1, 0, 0)
    assert rc == 0 and slab == 0 and blocks == 74
    rc, (chunks, blocks, slab) = plan(13, 13, 9, 9, 2, 3, 1, 1 << 30)       # paired: 8 lanes a group, 8 pairs a position
    assert rc == 0 and chunks == 1 and blocks == 2 and slab == 2 * 2 * (9 + 7) * 1024
    assert plan(2, 2, 8, 8, 9, 3, 0, 1 << 30)[0] == 2 and plan(2, 2, 129, 8, 3, 3, 0, 1 << 30)[0] == 2
    assert plan(0, 2, 8, 8, 3, 3, 0, 1 << 30)[0] == 1
