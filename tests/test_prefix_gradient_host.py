"""Prefix kernels with gradients under SigKernel(exact_gradient=True), the parts that need no GPU: the recurrence with a source per
coarse node (tests/prefix_gradient_reference.py) against torch autograd, its two bit identities, and the autograd function -- sources
per `nodes` mode, the row tiling, the unit-weight chain rule -- on an oracle-backed back-end whose discrete adjoint answers from that
recurrence.

Reference: torch autograd through prefix_gradient_reference.prefix_grid_torch (the plain double loop on torch scalars, all coarse
nodes).  Bars: the recurrence against autograd 1e-12 of max |W| (fp64 on both sides, at most 12 x 16 fine cells); the library's
gradients GRAD_BAR = 1e-8 of each path's max-norm gradient, the project's gradient bar."""
import functools

import numpy as np
import pytest
import torch

import sigkernel_amd
from sigkernel_amd import _lib
from fake_backend import OracleBackend
import exact_gradient_reference as R
import prefix_gradient_reference as PR

GRAD_BAR = 1e-8
NODES = ["all", "diagonal", "last_row", "last_col"]
SHAPES = [(1, 1, 0), (5, 3, 1), (3, 4, 2), (6, 5, 0)]


def _inc(Mc, Nc, d):
    return np.random.default_rng(11 * Mc + 3 * Nc + d).normal(scale=0.4, size=(Mc, Nc))


@pytest.mark.parametrize("naive", [False, True], ids=["default", "naive"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_d%d" % s)
def test_recurrence_with_sources_equals_autograd_of_the_weighted_sum(shape, naive):
    Mc, Nc, d = shape
    inc = _inc(Mc, Nc, d)
    S = np.random.default_rng(5).normal(size=(Mc, Nc))
    k, W = PR.source_adjoint(inc, S, d, naive)
    t = torch.from_numpy(inc).requires_grad_(True)
    nodes = PR.prefix_nodes_torch(t, d, naive)
    assert float(nodes[-1, -1].detach()) == k and bool((nodes[0] == 1).all()) and bool((nodes[:, 0] == 1).all())
    (nodes[1:, 1:] * torch.from_numpy(S)).sum().backward()
    want = t.grad.numpy()
    assert np.abs(W - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("naive", [False, True], ids=["default", "naive"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_d%d" % s)
def test_one_hot_sources_give_the_corner_and_the_sub_block_adjoints_bit_for_bit(shape, naive):
    Mc, Nc, d = shape
    inc = _inc(Mc, Nc, d)
    S = np.zeros((Mc, Nc))
    S[-1, -1] = 1.
    k, W = PR.source_adjoint(inc, S, d, naive)
    k0, W0 = R.exact_adjoint(inc, d, naive)
    assert k == k0 and np.array_equal(W, W0)
    for m, n in {(1, 1), (Mc // 2 + 1, Nc // 2 + 1), (Mc, 1), (1, Nc)}:
        S = np.zeros((Mc, Nc))
        S[m - 1, n - 1] = 1.
        _, W = PR.source_adjoint(inc, S, d, naive)
        _, Wsub = R.exact_adjoint(inc[:m, :n], d, naive)
        assert np.array_equal(W[:m, :n], Wsub)
        out = np.ones((Mc, Nc), dtype=bool)
        out[:m, :n] = False
        assert np.all(W[out] == 0.0)


class PrefixExactBackend(OracleBackend):
    """OracleBackend with the discrete adjoint and its sources mode.  The static-kernel stages run row by row of X, and the
    second-argument sums fold those rows in index order, so that a row-tiled backward performs the very operations of the untiled one."""

    def solve_adj(self, inc_c, dyadic, naive=False, flags=0, edges=None, discrete=False, cells=None, sources=None):
        if not discrete:
            assert cells is None and sources is None
            return super().solve_adj(inc_c, dyadic, naive, flags, edges)
        assert cells is None
        a = inc_c.detach().double().numpy()
        if sources is None:
            k, W = R.exact_adjoint_batch(a, dyadic, naive)
        else:
            assert sources.dtype == inc_c.dtype and tuple(sources.shape) == tuple(inc_c.shape)
            k, W = PR.source_adjoint_batch(a, sources.detach().double().numpy(), dyadic, naive)
        return torch.from_numpy(np.asarray(k)).to(inc_c.dtype), torch.from_numpy(W).to(inc_c.dtype)

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
def prefix_backend():
    prev = _lib.set_backend(PrefixExactBackend())
    yield
    _lib.set_backend(prev)


def _kernel(kind):
    return sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(1.0)


def _paths(M=5, N=4):
    """X (3, M, 2), Y (3, N, 2): fp64 random walks"""
    gen = torch.Generator().manual_seed(5)
    X = torch.cumsum(0.5 * torch.randn(3, M, 2, generator=gen, dtype=torch.float64), dim=1)
    Y = torch.cumsum(0.5 * torch.randn(3, N, 2, generator=gen, dtype=torch.float64), dim=1)
    return X, Y


def _assert_per_path(got, want, what):
    got, want = got.numpy(), want.numpy()
    for a in range(want.shape[0]):
        scale = np.abs(want[a]).max()
        err = np.abs(got[a] - want[a]).max()
        assert err <= GRAD_BAR * scale, "%s, path %d: |error| %.3e against a max-norm gradient of %.3e" % (what, a, err, scale)


def _both(method, nodes, kernel, d, workspace_bytes=None, M=5, N=4):
    """(values, gradients of the library, gradients of the reference) of sum(w * method), for X and Y"""
    Xc, Yc = _paths(M, N)
    sk = sigkernel_amd.SigKernel(kernel, d, exact_gradient=True, workspace_bytes=workspace_bytes)
    X, Y = Xc.clone().requires_grad_(True), Yc.clone().requires_grad_(True)
    Xr, Yr = Xc.clone().requires_grad_(True), Yc.clone().requires_grad_(True)
    if method == "gram":
        out, want = sk.compute_Gram_prefixes(X, Y, nodes=nodes), PR.slice_nodes(PR.prefix_grid_torch(Xr, Yr, kernel, d), nodes)
    elif method == "kernel":
        out = sk.compute_kernel_prefixes(X, Y, nodes=nodes)
        want = PR.slice_nodes(PR.prefix_grid_torch(Xr, Yr, kernel, d, paired=True), nodes)
    else:
        out, want = sk.compute_mmd_prefixes(X, Y), PR.mmd_prefixes_torch(Xr, Yr, kernel, d)
    assert out.grad_fn is not None and out.shape == want.shape
    assert float((out.detach() - want.detach()).abs().max()) <= 1e-12 * float(want.detach().abs().max())
    w = torch.randn(want.shape, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    (out * w).sum().backward()
    (want * w).sum().backward()
    return out.detach(), (X.grad, Y.grad), (Xr.grad, Yr.grad)


@pytest.mark.parametrize("d", [0, 1])
@pytest.mark.parametrize("kind", ["linear", "rbf"])
@pytest.mark.parametrize("nodes", NODES)
@pytest.mark.parametrize("method", ["gram", "kernel"])
def test_prefix_gradients_equal_autograd_through_the_restatement(prefix_backend, method, nodes, kind, d):
    _, got, want = _both(method, nodes, _kernel(kind), d)
    for g, w, name in zip(got, want, ("X", "Y")):
        _assert_per_path(g, w, "%s.grad of %s, nodes=%s" % (name, method, nodes))


@pytest.mark.parametrize("d", [0, 1])
@pytest.mark.parametrize("kind", ["linear", "rbf"])
def test_mmd_prefixes_gradients_equal_autograd_through_the_restatement(prefix_backend, kind, d):
    _, got, want = _both("mmd", None, _kernel(kind), d)
    for g, w, name in zip(got, want, ("X", "Y")):
        _assert_per_path(g, w, "%s.grad of compute_mmd_prefixes" % name)


@pytest.mark.parametrize("nodes", NODES)
def test_values_are_those_of_the_no_grad_call(prefix_backend, nodes):
    Xc, Yc = _paths()
    sk = sigkernel_amd.SigKernel(_kernel("rbf"), 1, exact_gradient=True)
    X, Y = Xc.clone().requires_grad_(True), Yc.clone().requires_grad_(True)
    K, k = sk.compute_Gram_prefixes(X, Y, nodes=nodes), sk.compute_kernel_prefixes(X, Y, nodes=nodes)
    assert K.requires_grad and k.requires_grad
    assert torch.equal(K.detach(), sk.compute_Gram_prefixes(Xc, Yc, nodes=nodes))
    assert torch.equal(k.detach(), sk.compute_kernel_prefixes(Xc, Yc, nodes=nodes))
    assert torch.equal(sk.compute_mmd_prefixes(X, Y).detach(), sk.compute_mmd_prefixes(Xc, Yc))
    with torch.no_grad():
        assert sk.compute_Gram_prefixes(X, Y, nodes=nodes).grad_fn is None
    # only Y requires grad: the same gradient for Y
    K.sum().backward()
    Y2 = Yc.clone().requires_grad_(True)
    sk.compute_Gram_prefixes(Xc, Y2, nodes=nodes).sum().backward()
    assert torch.equal(Y.grad, Y2.grad)


@pytest.mark.parametrize("method", ["gram", "kernel"])
@pytest.mark.parametrize("nodes", ["all", "diagonal"])
def test_row_tiled_backward_equals_the_untiled_one_bit_for_bit(prefix_backend, method, nodes, monkeypatch):
    """workspace_bytes=1: one row of X per tile, each with its own slice of the sources (paths of 5 and 4 points: the diagonal's backward
    runs on 4 and 4)"""
    cells = (4, 3) if nodes == "all" else (3, 3)
    calls = []
    real = PrefixExactBackend.solve_adj

    def counted(self, *a, **kw):
        calls.append(tuple(kw["sources"].shape))
        return real(self, *a, **kw)
    monkeypatch.setattr(PrefixExactBackend, "solve_adj", counted)
    _, whole, _ = _both(method, nodes, _kernel("rbf"), 1)
    assert calls == [((3, 3) if method == "gram" else (3,)) + cells]
    del calls[:]
    _, tiled, _ = _both(method, nodes, _kernel("rbf"), 1, workspace_bytes=1)
    assert calls == [((1, 3) if method == "gram" else (1,)) + cells] * 3
    assert torch.equal(whole[0], tiled[0]) and torch.equal(whole[1], tiled[1])


def test_where_x_is_y_autograd_adds_the_two_contributions(prefix_backend):
    Xc, _ = _paths()
    sk = sigkernel_amd.SigKernel(_kernel("rbf"), 1, exact_gradient=True)
    w = torch.randn(3, 3, 5, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    X = Xc.clone().requires_grad_(True)
    (sk.compute_Gram_prefixes(X, X, nodes="diagonal") * w).sum().backward()
    X1, X2 = Xc.clone().requires_grad_(True), Xc.clone().requires_grad_(True)
    (sk.compute_Gram_prefixes(X1, X2, nodes="diagonal") * w).sum().backward()
    assert torch.equal(X.grad, X1.grad + X2.grad)


@pytest.mark.parametrize("M,N", [(6, 4), (3, 5)])
def test_diagonal_of_unequal_lengths_gives_exact_zeros_beyond_the_shorter_path(prefix_backend, M, N):
    T = min(M, N)
    out, got, want = _both("gram", "diagonal", _kernel("rbf"), 1, M=M, N=N)
    assert out.shape == (3, 3, T)
    for g, w, name in zip(got, want, ("X", "Y")):
        assert bool((g[:, T:] == 0.0).all()) and bool((w[:, T:] == 0.0).all())
        _assert_per_path(g, w, "%s.grad" % name)
    _, got, want = _both("mmd", None, _kernel("linear"), 0, M=M, N=N)
    for g, w, name in zip(got, want, ("X", "Y")):
        assert bool((g[:, T:] == 0.0).all())
        _assert_per_path(g, w, "%s.grad of compute_mmd_prefixes" % name)


def test_one_point_paths_get_zeros(prefix_backend):
    sk = sigkernel_amd.SigKernel(_kernel("linear"), 1, exact_gradient=True)
    X, Y = _paths(1, 4)
    X, Y = X.requires_grad_(True), Y.requires_grad_(True)
    out = sk.compute_Gram_prefixes(X, Y)
    assert out.shape == (3, 3, 1, 4) and bool((out == 1).all())
    out.sum().backward()
    assert bool((X.grad == 0).all()) and bool((Y.grad == 0).all())


def test_the_default_object_still_raises(prefix_backend):
    Xc, Yc = _paths()
    sk = sigkernel_amd.SigKernel(_kernel("linear"), 1)
    X = Xc.clone().requires_grad_(True)
    for call in (lambda: sk.compute_Gram_prefixes(X, Yc), lambda: sk.compute_kernel_prefixes(Xc, X, nodes="diagonal"),
                 lambda: sk.compute_mmd_prefixes(X, Yc), lambda: sk.compute_mmd_prefixes(Xc, X)):
        with pytest.raises(NotImplementedError, match="forward only"):
            call()
        with pytest.raises(NotImplementedError, match="exact_gradient=True"):
            call()


def test_binding_rejects_sources_without_the_discrete_mode_and_with_cells():
    be = _lib.HipBackend.__new__(_lib.HipBackend)
    with pytest.raises(ValueError, match="discrete"):
        _lib.HipBackend.solve_adj(be, torch.zeros(1, 2, 2), 0, sources=torch.zeros(1, 2, 2))
    with pytest.raises(ValueError, match="cells"):
        _lib.HipBackend.solve_adj(be, torch.zeros(1, 2, 2), 0, discrete=True, sources=torch.zeros(1, 2, 2),
                                  cells=torch.zeros(1, 2, dtype=torch.int32))
    assert _lib.FLAG_SOURCES == 64
