"""Ragged batches with gradients under SigKernel(exact_gradient=True), the parts that need no GPU: the autograd function, the per-tile
table of sub-grids and the chain rule on the padded paths, on an oracle-backed back-end whose discrete adjoint answers from the
restatement (tests/exact_gradient_reference.py) on every pair's own sub-block, zeros elsewhere.

Reference: torch autograd through exact_gradient_reference.gram_torch on the TRUNCATED paths X[a, :lx[a]], Y[b, :ly[b]], pair by pair.
Bar: 1e-12 of each path's max-norm gradient, the bar of tests/test_exact_gradient_host.py (fp64 on both sides, at most 10 x 8 fine cells
per pair)."""
import functools

import numpy as np
import pytest
import torch

import sigkernel_amd
from sigkernel_amd import _lib
from fake_backend import OracleBackend
import exact_gradient_reference as R

TOL = 1e-12
LX = [2, 6, 1]              # two points, the padded length, one point
LY = [5, 1, 2, 3]


class RaggedExactBackend(OracleBackend):
    """OracleBackend with the discrete adjoint and its ragged mode.  The static-kernel stages run row by row of X, and the
    second-argument sums fold those rows in index order, so that a row-tiled backward performs the very operations of the untiled one."""

    def solve_adj(self, inc_c, dyadic, naive=False, flags=0, edges=None, discrete=False, cells=None):
        if not discrete:
            assert cells is None
            return super().solve_adj(inc_c, dyadic, naive, flags, edges)
        a = inc_c.detach().double().numpy()
        Mc, Nc = a.shape[-2:]
        flat = a.reshape(-1, Mc, Nc)
        if cells is None:
            tab = np.tile(np.array([[Mc, Nc]]), (flat.shape[0], 1))
        else:
            assert cells.dtype == torch.int32 and tuple(cells.shape) == tuple(a.shape[:-2]) + (2,)
            tab = np.clip(cells.numpy().reshape(-1, 2), 0, [Mc, Nc])
        k, W = np.ones(flat.shape[0]), np.zeros_like(flat)
        for p, (mc, nc) in enumerate(tab):
            if mc > 0 and nc > 0:
                k[p], W[p, :mc, :nc] = R.exact_adjoint(flat[p, :mc, :nc], dyadic, naive)
        return torch.from_numpy(k.reshape(a.shape[:-2])).to(inc_c.dtype), torch.from_numpy(W.reshape(a.shape)).to(inc_c.dtype)

    def static_increments(self, kind, param, X, Y, gram):
        up = super().static_increments
        return torch.cat([up(kind, param, X[a:a + 1], Y if gram else Y[a:a + 1], gram) for a in range(X.shape[0])])

    def static_adjoint(self, kind, param, X, Y, W, scale, gram):
        up = super().static_adjoint
        return torch.cat([up(kind, param, X[a:a + 1], Y if gram else Y[a:a + 1], W[a:a + 1], scale[a:a + 1], gram)
                          for a in range(X.shape[0])])

    def static_adjoint2(self, kind, param, X, Y, W, scale, b0=0):
        up = super().static_adjoint2
        return functools.reduce(torch.add, [up(kind, param, X[a:a + 1], Y, W[a:a + 1], scale[a:a + 1], b0) for a in range(X.shape[0])])


@pytest.fixture
def ragged_backend():
    prev = _lib.set_backend(RaggedExactBackend())
    yield
    _lib.set_backend(prev)


def _kernel(kind):
    return sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(1.0)


def _paths(garbage=False):
    """X (3, 6, 2), Y (4, 5, 2): fp64 random walks, padded by repeating the last point of the true path, or with finite garbage"""
    gen = torch.Generator().manual_seed(5)
    X = torch.cumsum(0.5 * torch.randn(3, 6, 2, generator=gen, dtype=torch.float64), dim=1)
    Y = torch.cumsum(0.5 * torch.randn(4, 5, 2, generator=gen, dtype=torch.float64), dim=1)
    for T, lens in ((X, LX), (Y, LY)):
        for i, n in enumerate(lens):
            T[i, n:] = 37. * torch.randn(T.shape[1] - n, 2, generator=gen, dtype=torch.float64) if garbage else T[i, n - 1]
    return X, Y


def _ref_pair(x, y, kernel, d, naive):
    if x.shape[0] < 2 or y.shape[0] < 2:
        return torch.ones((), dtype=torch.float64)
    return R.gram_torch(x[None], y[None], kernel, d, naive)[0, 0]


def _ref_gram(X, lx, Y, ly, kernel, d, naive):
    return torch.stack([torch.stack([_ref_pair(X[a, :lx[a]], Y[b, :ly[b]], kernel, d, naive) for b in range(Y.shape[0])])
                        for a in range(X.shape[0])])


def _ref_mmd(X, lx, Y, ly, kernel, d, naive):
    def off_diagonal_mean(K):
        K = 0.5 * (K + K.t())
        return (K.sum() - torch.diag(K).sum()) / (K.shape[0] * (K.shape[0] - 1.))
    return (off_diagonal_mean(_ref_gram(X, lx, X, lx, kernel, d, naive)) + off_diagonal_mean(_ref_gram(Y, ly, Y, ly, kernel, d, naive))
            - 2. * _ref_gram(X, lx, Y, ly, kernel, d, naive).mean())


def _assert_per_path(got, want, what):
    got, want = got.numpy(), want.numpy()
    for a in range(want.shape[0]):
        scale = np.abs(want[a]).max()
        err = np.abs(got[a] - want[a]).max()
        assert err <= TOL * scale, "%s, path %d: |error| %.3e against a max-norm gradient of %.3e" % (what, a, err, scale)


def _assert_padding_is_zero(grad, lens):
    for i, n in enumerate(lens):
        assert bool((grad[i, n:] == 0.0).all()), (i, grad[i, n:])


def _both(method, kernel, d, naive, garbage=False, workspace_bytes=None):
    """(gradients of the library, gradients of the reference) of sum(w * method), for X and Y"""
    Xc, Yc = _paths(garbage)
    sk = sigkernel_amd.SigKernel(kernel, d, _naive_solver=naive, exact_gradient=True, workspace_bytes=workspace_bytes)
    gen = torch.Generator().manual_seed(9)
    X, Y = Xc.clone().requires_grad_(True), Yc.clone().requires_grad_(True)
    Xr, Yr = Xc.clone().requires_grad_(True), Yc.clone().requires_grad_(True)
    if method == "gram":
        w = torch.randn(3, 4, generator=gen, dtype=torch.float64)
        out, want = sk.compute_Gram_ragged(X, Y, LX, LY), _ref_gram(Xr, LX, Yr, LY, kernel, d, naive)
        lens = (LX, LY)
    elif method == "kernel":
        w = torch.randn(3, generator=gen, dtype=torch.float64)
        Y, Yr = Yc[:3].clone().requires_grad_(True), Yc[:3].clone().requires_grad_(True)
        out = sk.compute_kernel_ragged(X, Y, LX, LY[:3])
        want = torch.stack([_ref_pair(Xr[a, :LX[a]], Yr[a, :LY[a]], kernel, d, naive) for a in range(3)])
        lens = (LX, LY[:3])
    else:
        w = torch.randn((), generator=gen, dtype=torch.float64)
        out, want = sk.compute_mmd_ragged(X, LX, Y, LY), _ref_mmd(Xr, LX, Yr, LY, kernel, d, naive)
        lens = (LX, LY)
    assert out.grad_fn is not None and out.shape == want.shape
    assert float((out.detach() - want.detach()).abs().max()) <= TOL * float(want.detach().abs().max())
    (out * w).sum().backward()
    (want * w).sum().backward()
    return (X.grad, Y.grad), (Xr.grad, Yr.grad), lens


@pytest.mark.parametrize("naive", [False, True], ids=["default", "naive"])
@pytest.mark.parametrize("d", [0, 1])
@pytest.mark.parametrize("kind", ["linear", "rbf"])
@pytest.mark.parametrize("method", ["gram", "kernel", "mmd"])
def test_gradients_equal_autograd_on_the_truncated_paths(ragged_backend, method, kind, d, naive):
    got, want, lens = _both(method, _kernel(kind), d, naive)
    for g, w, n, name in zip(got, want, lens, ("X", "Y")):
        _assert_per_path(g, w, "%s.grad of %s" % (name, method))
        _assert_padding_is_zero(g, n)


@pytest.mark.parametrize("kind", ["linear", "rbf"])
@pytest.mark.parametrize("method", ["gram", "kernel", "mmd"])
def test_garbage_padding_gets_an_exactly_zero_gradient(ragged_backend, method, kind):
    """the padding holds random finite values (scale 37) instead of the repeated last point: the same gradients on the true points --
    the reference never sees the padding -- and exactly 0.0 on every padded point"""
    got, want, lens = _both(method, _kernel(kind), 1, False, garbage=True)
    for g, w, n, name in zip(got, want, lens, ("X", "Y")):
        _assert_padding_is_zero(g, n)
        _assert_per_path(g, w, "%s.grad of %s" % (name, method))


@pytest.mark.parametrize("kind", ["linear", "rbf"])
def test_values_are_those_of_the_no_grad_call(ragged_backend, kind):
    Xc, Yc = _paths()
    sk = sigkernel_amd.SigKernel(_kernel(kind), 1, exact_gradient=True)
    X, Y = Xc.clone().requires_grad_(True), Yc.clone().requires_grad_(True)
    K = sk.compute_Gram_ragged(X, Y, LX, LY)
    k = sk.compute_kernel_ragged(X, Y[:3], LX, LY[:3])
    assert K.requires_grad and k.requires_grad
    assert torch.equal(K.detach(), sk.compute_Gram_ragged(Xc, Yc, LX, LY))
    assert torch.equal(k.detach(), sk.compute_kernel_ragged(Xc, Yc[:3], LX, LY[:3]))
    with torch.no_grad():
        assert sk.compute_Gram_ragged(X, Y, LX, LY).grad_fn is None
    # only Y requires grad: X gets nothing, Y the same gradient
    K.sum().backward()
    Y2 = Yc.clone().requires_grad_(True)
    sk.compute_Gram_ragged(Xc, Y2, LX, LY).sum().backward()
    assert torch.equal(Y.grad, Y2.grad)


def test_where_x_is_y_autograd_adds_the_two_contributions(ragged_backend):
    Xc, _ = _paths()
    sk = sigkernel_amd.SigKernel(_kernel("rbf"), 1, exact_gradient=True)
    w = torch.randn(3, 3, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    X = Xc.clone().requires_grad_(True)
    (sk.compute_Gram_ragged(X, X, LX, LX) * w).sum().backward()
    X1, X2 = Xc.clone().requires_grad_(True), Xc.clone().requires_grad_(True)
    (sk.compute_Gram_ragged(X1, X2, LX, LX) * w).sum().backward()
    assert torch.equal(X.grad, X1.grad + X2.grad)


def test_the_default_object_still_raises(ragged_backend):
    Xc, Yc = _paths()
    sk = sigkernel_amd.SigKernel(_kernel("linear"), 1)
    X = Xc.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="forward only"):
        sk.compute_Gram_ragged(X, Yc, LX, LY)
    with pytest.raises(NotImplementedError, match="forward only"):
        sk.compute_kernel_ragged(Xc, X, LX, LX)
    with pytest.raises(NotImplementedError, match="forward only"):
        sk.compute_mmd_ragged(X, LX, Yc, LY)
    with pytest.raises(NotImplementedError, match="exact_gradient=True"):
        sk.compute_Gram_ragged(X, Yc, LX, LY)


@pytest.mark.parametrize("method", ["gram", "kernel"])
def test_row_tiled_backward_equals_the_untiled_one_bit_for_bit(ragged_backend, method, monkeypatch):
    """workspace_bytes=1: one row of X per tile, each with its own slice of the table"""
    calls = []
    real = RaggedExactBackend.solve_adj

    def counted(self, *a, **kw):
        calls.append(tuple(kw["cells"].shape))
        return real(self, *a, **kw)
    monkeypatch.setattr(RaggedExactBackend, "solve_adj", counted)
    whole, _, _ = _both(method, _kernel("rbf"), 1, False, garbage=True)
    assert calls == [(3, 4, 2) if method == "gram" else (3, 2)]
    del calls[:]
    tiled, _, _ = _both(method, _kernel("rbf"), 1, False, garbage=True, workspace_bytes=1)
    assert calls == [(1, 4, 2) if method == "gram" else (1, 2)] * 3
    assert torch.equal(whole[0], tiled[0]) and torch.equal(whole[1], tiled[1])


def test_binding_rejects_cells_without_the_discrete_mode():
    with pytest.raises(ValueError, match="discrete"):
        _lib.HipBackend.solve_adj(_lib.HipBackend.__new__(_lib.HipBackend), torch.zeros(1, 2, 2), 0, cells=torch.zeros(1, 2, dtype=torch.int32))
    assert _lib.FLAG_RAGGED == 32
