"""The gradient of the RBF-lifted truncated kernel without a GPU: the closed form the HIP points-adjoint sweep evaluates (csrc/sk_truncated.hip:
trunc_points_adjoint), restated in torch and held against autograd of the torch restatement; the SK_OP_TRUNCATED_RBF_ADJOINT rows of the
route table; the plan's slab; and the routing of TruncatedSigKernel(..., points_adjoint=True) on a stand-in backend.

Points x_0 .. x_{M-1}, y_0 .. y_{N-1};  kap(i, c) = exp(-|x_i - y_c|^2 / s) from differences of coordinates;
    G(i, c)  = kap(i, c) - kap(i, c - 1) - kap(i - 1, c) + kap(i - 1, c - 1)  for i, c >= 1, zero in row 0 and column 0;
    dG       = sum_m Rb^m P^{m-1}  on the nodes i, c >= 1 (the reverse recursion of test_truncated_adjoint_host.py on this G), zero off them;
    H(i, c)  = dG(i, c) - dG(i, c + 1) - dG(i + 1, c) + dG(i + 1, c + 1)  = d / d kap(i, c);
    dx_i     = sum_c H(i, c) kap(i, c) (-2 / s) (x_i - y_c),     dy_c = -sum_i (the same term).
Shapes are (A, B, Mp, Np, D, L) with Mp, Np in POINTS."""
import ctypes

import numpy as np
import pytest
import torch

from test_truncated_adjoint_host import _excl, _excl_suffix
from test_truncated_static_host import walks


def lifted_closed_form(X, Y, w, s):
    """(dX, dY) of sum_{m, a, b} w[m - 1, a, b] k_m(X[a], Y[b]), k_m the level terms lifted through RBFKernel(s); X (A, Mp, D), Y (B, Np, D)
    POINTS, w (L, A, B)"""
    L = w.shape[0]
    e = X[:, None, :, None, :] - Y[None, :, None, :, :]          # (A, B, Mp, Np, D)
    kap = torch.exp(-(e * e).sum(-1) / s)
    G = torch.zeros_like(kap)
    G[..., 1:, 1:] = (kap[..., 1:, 1:] - kap[..., 1:, :-1]) - (kap[..., :-1, 1:] - kap[..., :-1, :-1])
    P, R = [torch.ones_like(G)], G
    for _ in range(1, L):
        P.append(_excl(_excl(R, -2), -1))
        R = G * P[-1]
    Rb = w[L - 1][:, :, None, None] * torch.ones_like(G)
    dG = Rb * P[L - 1]
    for m in range(L - 1, 0, -1):
        Rb = w[m - 1][:, :, None, None] + _excl_suffix(_excl_suffix(G * Rb, -2), -1)
        dG = dG + Rb * P[m - 1]
    dG[..., 0, :] = 0           # row 0 and column 0 carry no node
    dG[..., :, 0] = 0
    pad = torch.nn.functional.pad(dG, (0, 1, 0, 1))             # dG is zero beyond the last row and column
    H = (pad[..., :-1, :-1] - pad[..., :-1, 1:]) - (pad[..., 1:, :-1] - pad[..., 1:, 1:])
    coef = H * kap * (-2.0 / s)
    return torch.einsum("abij,abijd->aid", coef, e), -torch.einsum("abij,abijd->bjd", coef, e)


def lifted_autograd(X, Y, w, s):
    """the same by autograd of the torch restatement; w (L + 1, A, B): level 0 is the constant 1 and takes no gradient"""
    from sigkernel_amd import RBFKernel
    from sigkernel_amd.truncated import _lifted_gram, _truncated_levels_torch
    X, Y = X.clone().requires_grad_(), Y.clone().requires_grad_()
    (w * _truncated_levels_torch(X, Y, w.shape[0] - 1, 1, False, None, _lifted_gram(RBFKernel(s)))).sum().backward()
    return X.grad, Y.grad


@pytest.mark.parametrize("A,B,Mp,Np,D,L", [(3, 2, 6, 5, 3, 4), (2, 2, 2, 2, 1, 1)])
def test_closed_form_is_the_gradient_of_the_lifted_restatement(A, B, Mp, Np, D, L):
    """<= 1e-12 of each gradient's max-norm; every point gets a gradient, the first one included"""
    rng = np.random.default_rng(100 * Mp + Np + L)
    X, Y = torch.as_tensor(walks(rng, A, Mp, D)), torch.as_tensor(walks(rng, B, Np, D))
    w = torch.as_tensor(rng.standard_normal((L + 1, A, B)))
    s = 1.3
    dX, dY = lifted_closed_form(X, Y, w[1:], s)
    wX, wY = lifted_autograd(X, Y, w, s)
    for name, got, want in (("dX", dX, wX), ("dY", dY, wY)):
        err = float((got - want).abs().max() / want.abs().max())
        print("lifted closed form vs autograd %s %s: %.2e" % ((A, B, Mp, Np, D, L), name, err))
        assert err <= 1e-12, (name, err)
    assert bool((dX[:, 0].abs() > 0).any()) and bool((dY[:, 0].abs() > 0).any())
    if L == 1:      # k_1 = kap(1, 1) - kap(1, 0) - kap(0, 1) + kap(0, 0), differentiated by hand
        kap = lambda x, y: torch.exp(-((x - y) ** 2).sum() / s)
        dk = lambda x, y: kap(x, y) * (-2.0 / s) * (x - y)         # d kap(x, y) / dx = -d kap(x, y) / dy
        hX, hY = torch.zeros_like(X), torch.zeros_like(Y)
        for a in range(A):
            for b in range(B):
                x, y, c = X[a], Y[b], w[1, a, b]
                hX[a, 1] += c * (dk(x[1], y[1]) - dk(x[1], y[0]))
                hX[a, 0] += c * (dk(x[0], y[0]) - dk(x[0], y[1]))
                hY[b, 1] -= c * (dk(x[1], y[1]) - dk(x[0], y[1]))
                hY[b, 0] -= c * (dk(x[0], y[0]) - dk(x[1], y[0]))
        assert float((dX - hX).abs().max() / hX.abs().max()) <= 1e-12
        assert float((dY - hY).abs().max() / hY.abs().max()) <= 1e-12


def test_route_table_states_the_points_adjoint_scope():
    from sigkernel_amd import _lib
    F, S = _lib.ROUTE_FUSED, _lib.ROUTE_STREAM
    q = lambda D, M, N, L, order, es=8: int(_lib.load().sk_route_query(_lib.OP_TRUNCATED_RBF_ADJOINT, order, D, M, N, L, 0, es, 0))
    assert _lib.OP_TRUNCATED_RBF_ADJOINT == 7
    assert q(8, 128, 256, 8, 1) == F and q(8, 128, 256, 8, 1, 4) == F and q(1, 2, 2, 1, -1) == F
    assert q(9, 128, 256, 8, 1) == S          # sixteen doubles per point: the forward's scope, not the adjoint's
    assert q(8, 129, 256, 8, 1) == S          # never swapped: the other batch's gradient is the query on (N, M)
    assert q(8, 256, 128, 8, 1) == S and q(8, 128, 257, 8, 1) == S
    assert q(8, 128, 256, 8, 2) == S          # order 2
    assert q(8, 1, 256, 8, 1) == S and q(8, 128, 1, 8, 1) == S      # one point is no path
    assert q(8, 128, 256, 9, 1) == S
    assert q(8, 128, 256, 8, 1, 2) == S       # elem_size 2
    # the forward's rule and the plain adjoint's answer what they answered
    lib = _lib.load()
    assert lib.sk_route_query(_lib.OP_TRUNCATED_RBF, 1, 9, 128, 128, 8, 0, 8, 0) == F
    assert lib.sk_route_query(_lib.OP_TRUNCATED_ADJOINT, 1, 8, 1, 1, 1, 0, 8, 0) == F
    assert lib.sk_version() == 340


def _plan(name, A, B, M, N, D, L, paired, ws):
    from sigkernel_amd import _lib
    out = (ctypes.c_int64 * 3)()
    rc = getattr(_lib.load(), name)(A, B, M, N, D, L, paired, ws, ctypes.cast(out, ctypes.c_void_p))
    return rc, tuple(out)


def test_points_adjoint_plan_counts_the_plane_of_g():
    """sk_truncated_points_adjoint_plan (host only): the plain adjoint's split with L planes a block -- L - 1 prefix factors and g -- of
    (N + lanes - 1) steps x 1 KB.  (5, 37, 20, 33, 3, 6): 20 points = 10 lanes -> groups of 16, 4 groups a wave, 2 row tiles; 37 chunks; 74
    blocks of 6 x (33 + 15) KB."""
    from sigkernel_amd import _lib
    name = "sk_truncated_points_adjoint_plan"
    block = 6 * (33 + 15) * 1024
    rc, (chunks, blocks, slab) = _plan(name, 5, 37, 20, 33, 3, 6, 0, 1 << 30)
    assert rc == 0 and chunks == 37 and blocks == 74 and slab == 74 * block
    rc, (chunks, blocks, slab) = _plan(name, 5, 37, 20, 33, 3, 6, 0, 3 * block + 5)
    assert rc == 0 and chunks == 37 and blocks == 3 and slab == 3 * block
    assert _plan(name, 5, 37, 20, 33, 3, 6, 0, block - 1)[0] == 2
    rc, (chunks, blocks, slab) = _plan(name, 5, 37, 20, 33, 3, 1, 0, 1 << 30)       # one level: the plane of g alone
    assert rc == 0 and slab == 74 * 48 * 1024
    assert _plan(name, 5, 37, 20, 33, 3, 1, 0, 0)[0] == 2
    rc, (chunks, blocks, slab) = _plan(name, 13, 13, 10, 10, 2, 3, 1, 1 << 30)      # paired: 8 lanes a group, 8 pairs a position
    assert rc == 0 and chunks == 1 and blocks == 2 and slab == 2 * 3 * (10 + 7) * 1024
    assert _plan(name, 2, 2, 8, 8, 9, 3, 0, 1 << 30)[0] == 2 and _plan(name, 2, 2, 129, 8, 3, 3, 0, 1 << 30)[0] == 2
    assert _plan(name, 2, 2, 1, 8, 3, 3, 0, 1 << 30)[0] == 2 and _plan(name, 0, 2, 8, 8, 3, 3, 0, 1 << 30)[0] == 1
    # the plain adjoint's plan returns what it returned
    rc, (chunks, blocks, slab) = _plan("sk_truncated_adjoint_plan", 5, 37, 20, 33, 3, 6, 0, 1 << 30)
    assert rc == 0 and chunks == 37 and blocks == 74 and slab == 74 * 5 * 48 * 1024
    be = _lib.HipBackend()
    assert be.truncated_points_adjoint_fits(5, 37, 20, 33, 3, 6, False, block) and not be.truncated_points_adjoint_fits(5, 37, 20, 33, 3, 6, False, block - 1)
    assert not be.truncated_points_adjoint_fits(5, 37, 20, 33, 9, 6) and be.truncated_adjoint_fits(5, 37, 20, 33, 3, 6, False, 5 * 48 * 1024)


class PointsBackend:
    """Stand-in for HipBackend on CPU tensors -- TESTS ONLY: the route table and the plan are the library's (host only), the levels are the
    torch restatement's and the adjoint the closed form above; every call is recorded."""
    name = "points-fake"

    def __init__(self):
        self.levels, self.adjoints = [], []

    def route(self, *args, **kw):
        from sigkernel_amd import _lib
        return _lib.HipBackend.route(*args, **kw)

    def truncated_points_adjoint_fits(self, *args, **kw):
        from sigkernel_amd import _lib
        return _lib.HipBackend().truncated_points_adjoint_fits(*args, **kw)

    def truncated_levels(self, X, Y, num_levels, order, paired=False, kind=0, param=0.0):
        from sigkernel_amd import RBFKernel, _lib
        from sigkernel_amd.truncated import _lifted_gram, _truncated_levels_torch
        assert kind == 1 and not X.requires_grad and not Y.requires_grad
        if self.route(_lib.OP_TRUNCATED_RBF, order, X.shape[2], X.shape[1], Y.shape[1], num_levels, False, X.element_size()) != _lib.ROUTE_FUSED:
            return None
        self.levels.append((tuple(X.shape), tuple(Y.shape)))
        return _truncated_levels_torch(X, Y, num_levels, order, paired, None, _lifted_gram(RBFKernel(param)))

    def truncated_points_adjoint(self, X, Y, w, num_levels, param, paired=False, workspace_bytes=None):
        assert not paired and w.shape == (num_levels, X.shape[0], Y.shape[0]) and w.is_contiguous()
        self.adjoints.append((X, Y, w.clone()))
        return lifted_closed_form(X.detach(), Y.detach(), w, param)[0]


@pytest.fixture
def fake(monkeypatch):
    from sigkernel_amd import _lib, truncated
    be = PointsBackend()
    prev = _lib.set_backend(be)
    monkeypatch.setattr(truncated, "_on_hip", lambda t: True)
    yield be
    _lib.set_backend(prev)


def _routing_inputs(Mp=6, Np=5, D=3, L=3):
    rng = np.random.default_rng(17)
    X, Y = torch.as_tensor(walks(rng, 3, Mp, D)), torch.as_tensor(walks(rng, 2, Np, D))
    sigma = torch.as_tensor(rng.uniform(0.5, 1.5, L + 1))
    up = torch.as_tensor(rng.standard_normal((3, 2)))
    return X, Y, sigma, up, L


def _object(L, sigma, **kw):
    from sigkernel_amd import RBFKernel, TruncatedSigKernel
    return TruncatedSigKernel(L, sigma, 1, static_kernel=RBFKernel(0.8), **kw)


@pytest.mark.parametrize("grads", ["x", "y", "xy"])
def test_points_adjoint_routes_each_side_that_needs_a_gradient(fake, grads):
    X, Y, sigma, up, L = _routing_inputs()
    Xg, Yg = X.clone().requires_grad_("x" in grads), Y.clone().requires_grad_("y" in grads)
    (up * _object(L, sigma, points_adjoint=True).compute_Gram(Xg, Yg)).sum().backward()
    assert fake.levels == [((3, 6, 3), (2, 5, 3))]
    w = sigma[1:, None, None] * up[None]          # the upstream gradient of the level terms
    want = ([(Xg, Yg, w)] if "x" in grads else []) + ([(Yg, Xg, w.transpose(1, 2))] if "y" in grads else [])
    assert len(fake.adjoints) == len(want)
    for (x, y, v), (wx, wy, wv) in zip(fake.adjoints, want):
        assert x.shape == wx.shape and y.shape == wy.shape and torch.equal(x, wx.detach()) and torch.allclose(v, wv, rtol=1e-15, atol=0)
    # ... and end to end: the gradients of the restatement, which a default object takes
    Xr, Yr = X.clone().requires_grad_("x" in grads), Y.clone().requires_grad_("y" in grads)
    n = len(fake.adjoints)
    (up * _object(L, sigma).compute_Gram(Xr, Yr)).sum().backward()
    assert len(fake.adjoints) == n and len(fake.levels) == 1         # points_adjoint=False never calls it
    for got, ref in ((Xg.grad, Xr.grad), (Yg.grad, Yr.grad)):
        assert (got is None) == (ref is None)
        if ref is not None:
            assert float((got - ref).abs().max() / ref.abs().max()) <= 1e-12


def test_points_adjoint_sym_is_one_call_with_w_plus_its_transpose(fake):
    X, _, sigma, _, L = _routing_inputs()
    up = torch.as_tensor(np.random.default_rng(5).standard_normal((3, 3)))
    Xg, Xr = X.clone().requires_grad_(), X.clone().requires_grad_()
    (up * _object(L, sigma, points_adjoint=True).compute_Gram(Xg, Xg, sym=True)).sum().backward()
    assert len(fake.levels) == 1 and len(fake.adjoints) == 1
    w = sigma[1:, None, None] * up[None]
    assert torch.allclose(fake.adjoints[0][2], w + w.transpose(1, 2), rtol=1e-15, atol=0)
    (up * _object(L, sigma).compute_Gram(Xr, Xr, sym=True)).sum().backward()
    assert float((Xg.grad - Xr.grad).abs().max() / Xr.grad.abs().max()) <= 1e-12


def test_points_adjoint_keeps_the_gradient_of_a_learnable_sigma(fake):
    X, Y, sigma, up, L = _routing_inputs()
    s1, s2 = sigma.clone().requires_grad_(), sigma.clone().requires_grad_()
    (up * _object(L, s1, points_adjoint=True).compute_Gram(X.clone().requires_grad_(), Y)).sum().backward()
    (up * _object(L, s2).compute_Gram(X.clone().requires_grad_(), Y)).sum().backward()
    assert len(fake.adjoints) == 1
    assert float((s1.grad - s2.grad).abs().max() / s2.grad.abs().max()) <= 1e-12


def test_one_side_out_of_scope_sends_the_whole_call_to_the_restatement(fake):
    """130 points on a side that needs a gradient: nothing of the backend is called, not even the forward, which alone would be in scope"""
    X, Y, sigma, up, L = _routing_inputs(Mp=6, Np=130)
    tk = _object(L, sigma, points_adjoint=True)
    Xg, Yg = X.clone().requires_grad_(), Y.clone().requires_grad_()
    K = tk.compute_Gram(Xg, Yg)
    assert fake.levels == [] and fake.adjoints == [] and K.requires_grad
    # with X alone requiring grad the same shapes are served: 130 points on the side that only streams past
    K = tk.compute_Gram(Xg, Y)
    (up * K).sum().backward()
    assert len(fake.levels) == 1 and len(fake.adjoints) == 1
    # a workspace below one block's slab, order 2, dim 9: the restatement as a whole
    X9, Y9 = _routing_inputs(D=9)[:2]
    for tk2, x, y in ((_object(L, sigma, points_adjoint=True, workspace_bytes=L * (5 + 3) * 1024 - 1), Xg, _routing_inputs()[1]),
                      (type(tk)(L, sigma, 2, static_kernel=tk.static_kernel, points_adjoint=True), Xg, _routing_inputs()[1]),
                      (tk, X9.clone().requires_grad_(), Y9)):
        n = (len(fake.levels), len(fake.adjoints))
        assert tk2.compute_Gram(x, y).requires_grad
        assert (len(fake.levels), len(fake.adjoints)) == n
    # no gradient enabled: the forward-only route, one levels call and no adjoint
    n = (len(fake.levels), len(fake.adjoints))
    with torch.no_grad():
        tk.compute_Gram(Xg, _routing_inputs()[1])
    assert (len(fake.levels), len(fake.adjoints)) == (n[0] + 1, n[1])


def test_points_adjoint_is_the_last_keyword_and_defaults_to_false():
    import inspect
    from sigkernel_amd import TruncatedSigKernel
    params = list(inspect.signature(TruncatedSigKernel.__init__).parameters.values())
    assert params[-1].name == "points_adjoint" and params[-1].default is False
    assert TruncatedSigKernel(3).points_adjoint is False
