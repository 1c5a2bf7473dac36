"""The truncated kernel's WIDE-ADJOINT mode without a GPU (csrc/sk_truncated.hip: trunc_wide_adjoint): the SK_OP_TRUNCATED_WIDE_ADJOINT
rows of the route table, the plan's slab arithmetic and its paired widening at 16 staged coordinates, the C entry point's argument checks,
and the routing of TruncatedSigKernel(wide_adjoint=True) on a stand-in backend whose adjoint is the closed form the kernel evaluates
(test_truncated_adjoint_host.py: closed_form).

Every test here fails on the parent: no operation 10, no export, and the keyword is a TypeError.  Shapes are in STEPS."""
import ctypes

import numpy as np
import pytest
import torch

from test_truncated_adjoint_host import closed_form
from test_truncated_host import steps

# rows of the side that needs the gradient: two rows per lane hold at fd = 16 ("Wide adjoint"), so the scope's M is the
# adjoint mode's
M_MAX = 128


def q(op, D, M, N, L, order, es=8, flags=0):
    from sigkernel_amd import _lib
    return int(_lib.load().sk_route_query(op, order, D, M, N, L, 0, es, flags))


def test_version_and_the_op_number():
    from sigkernel_amd import _lib
    assert _lib.load().sk_version() == 340
    assert _lib.OP_TRUNCATED_WIDE_ADJOINT == 10


def test_route_table_states_the_wide_adjoint_scope():
    from sigkernel_amd import _lib
    F, S = _lib.ROUTE_FUSED, _lib.ROUTE_STREAM
    op = _lib.OP_TRUNCATED_WIDE_ADJOINT
    for es in (8, 4):
        for D, M, N, L in ((9, M_MAX, 128, 8), (16, M_MAX, 128, 8), (9, 1, 1, 1), (12, 9, 6, 4)):
            assert q(op, D, M, N, L, 1, es) == F, (D, M, N, L, es)
    assert q(op, 8, 20, 20, 4, 1) == S            # not mine: the adjoint mode serves dims up to 8
    assert q(op, 17, 20, 20, 4, 1) == S
    assert q(op, 9, M_MAX + 1, 20, 4, 1) == S     # never swapped: the other batch's gradient is the query on (N, M)
    assert q(op, 9, 20, 129, 4, 1) == S           # 16 x ceil16(129) doubles are beyond a wave's y block
    assert q(op, 9, 20, 20, 9, 1) == S
    assert q(op, 9, 20, 20, 4, 2) == S and q(op, 9, 20, 20, 4, -1) == S
    assert q(op, 9, 20, 20, 1, -1) == F           # one level is order 1
    assert q(op, 9, 20, 20, 4, 1, 2) == S
    assert q(op, 9, M_MAX, 128, 8, 1, 8, 4) == F  # (SK_ROUTE_NO_SWAP changes nothing: there is no swap to forbid)


def test_pinned_rows_of_the_other_truncated_routes_are_unchanged():
    from sigkernel_amd import _lib
    from sigkernel_amd.truncated import truncated_route
    F, W, S = _lib.ROUTE_FUSED, _lib.ROUTE_FUSED_SWAP, _lib.ROUTE_STREAM
    # operation 5, the rows of test_truncated_adjoint_host.py
    a = lambda D, M, N, L, order, es=8: q(_lib.OP_TRUNCATED_ADJOINT, D, M, N, L, order, es)
    assert a(8, 128, 256, 8, 1) == F and a(8, 128, 256, 8, 1, 4) == F and a(1, 1, 1, 1, 1) == F and a(3, 9, 6, 1, -1) == F
    assert a(9, 128, 256, 8, 1) == S and a(8, 129, 256, 8, 1) == S and a(8, 128, 256, 8, 2) == S and a(8, 64, 64, 4, -1) == S
    assert a(8, 128, 256, 9, 1) == S and a(8, 128, 257, 8, 1) == S and a(8, 128, 256, 8, 1, 2) == S
    # operation 4
    for (D, M, N, L, order, es), want in {(8, 64, 64, 4, -1, 8): F, (8, 65, 64, 4, -1, 8): W, (8, 65, 65, 4, -1, 8): S, (8, 128, 128, 8, 1, 8): F,
                                          (8, 129, 128, 8, 1, 4): W, (8, 129, 130, 8, 1, 8): S, (16, 64, 128, 8, 4, 4): F, (16, 64, 129, 8, 4, 8): S,
                                          (17, 8, 8, 3, 1, 8): S, (4, 8, 8, 9, 1, 8): S, (4, 8, 8, 6, 5, 8): S, (4, 8, 8, 5, 5, 8): S,
                                          (4, 8, 8, 4, 4, 8): F, (1, 2, 3, 1, -1, 8): F, (8, 64, 256, 3, 2, 8): F, (8, 64, 257, 3, 2, 8): S,
                                          (4, 200, 40, 6, 3, 8): W, (4, 300, 40, 6, 3, 8): S}.items():
        assert truncated_route(D, M, N, L, order, es) == want, (D, M, N, L, order, es)
    # operations 6 .. 9 on the same shapes (M, N: points for 6 and 7)
    rbf = lambda *r: q(_lib.OP_TRUNCATED_RBF, *r)
    assert rbf(8, 128, 128, 8, 1) == F and rbf(8, 129, 128, 8, 1) == W and rbf(8, 129, 130, 8, 1) == S and rbf(8, 64, 64, 4, -1) == S
    assert rbf(16, 128, 128, 8, 1) == F and rbf(8, 1, 8, 3, 1) == S
    rba = lambda *r: q(_lib.OP_TRUNCATED_RBF_ADJOINT, *r)
    assert rba(8, 128, 256, 8, 1) == F and rba(9, 128, 128, 8, 1) == S and rba(8, 129, 128, 8, 1) == S and rba(8, 128, 256, 8, 2) == S
    lg = lambda *r: q(_lib.OP_TRUNCATED_LONG, *r)
    assert lg(8, 128, 130, 8, 1) == F and lg(8, 130, 128, 8, 1) == W and lg(8, 1000, 129, 8, 1) == F and lg(16, 513, 512, 8, 1) != S
    assert lg(8, 300, 300, 2, 2) == S and lg(17, 300, 300, 8, 1) == S
    la = lambda *r: q(_lib.OP_TRUNCATED_LONG_ADJOINT, *r)
    assert la(8, 129, 129, 8, 1) == F and la(9, 129, 129, 8, 1) == S and la(8, 129, 129, 9, 1) == S and la(8, 129, 129, 2, 2) == S
    assert _lib.load().sk_version() == 340


def _plan(A, B, M, N, D, L, paired, ws):
    from sigkernel_amd import _lib
    out = (ctypes.c_int64 * 3)()
    rc = _lib.load().sk_truncated_wide_adjoint_plan(A, B, M, N, D, L, paired, ws, ctypes.cast(out, ctypes.c_void_p))
    return rc, tuple(out)


def test_plan_splits_and_bounds_the_slab_and_widens_paired_groups_by_sixteen_coordinates():
    """sk_truncated_wide_adjoint_plan (host only): the adjoint mode's split -- chunks of second paths fill the resident blocks, the block
    count comes down until the slabs, (L - 1) (N + lanes - 1) KB a block, fit -- with the paired widening counting 16 x Ncp doubles a block"""
    big = 1 << 30
    block = 5 * (33 + 15) * 1024                  # 16 lanes a group, 4 groups: 2 row tiles
    rc, (chunks, blocks, slab) = _plan(5, 37, 20, 33, 13, 6, 0, big)
    assert rc == 0 and chunks == 37 and blocks == 74 and slab == 74 * block
    rc, (chunks, blocks, slab) = _plan(5, 37, 20, 33, 13, 6, 0, 3 * block + 5)
    assert rc == 0 and chunks == 37 and blocks == 3 and slab == 3 * block
    assert _plan(5, 37, 20, 33, 13, 6, 0, block - 1)[0] == 2
    rc, (chunks, blocks, slab) = _plan(5, 37, 20, 33, 13, 1, 0, 0)
    assert rc == 0 and slab == 0 and blocks == 74
    # paired, nine rows: five lanes would make groups of 8, but 8 x 16 x 48 doubles (and 4 x) are beyond the 2048 of a wave, 2 x are not:
    # groups of 32 lanes, two pairs a position, three positions
    rc, (chunks, blocks, slab) = _plan(5, 5, 9, 33, 16, 3, 1, big)
    assert rc == 0 and chunks == 1 and blocks == 3 and slab == 3 * 2 * (33 + 31) * 1024
    # ... where the adjoint mode at eight coordinates has 8 x 8 x 48 > 2048 >= 4 x 8 x 48: groups of 16, as before
    out = (ctypes.c_int64 * 3)()
    from sigkernel_amd import _lib
    assert _lib.load().sk_truncated_adjoint_plan(5, 5, 9, 33, 8, 3, 1, big, ctypes.cast(out, ctypes.c_void_p)) == 0
    assert tuple(out) == (1, 2, 2 * 2 * (33 + 15) * 1024)
    # paired with narrow y blocks: 8 x 16 x 16 doubles fit, eight pairs a position
    rc, (chunks, blocks, slab) = _plan(13, 13, 9, 9, 10, 5, 1, big)
    assert rc == 0 and chunks == 1 and blocks == 2 and slab == 2 * 4 * (9 + 7) * 1024
    # outside the scope, and bad arguments
    assert _plan(2, 2, 8, 8, 8, 3, 0, big)[0] == 2 and _plan(2, 2, M_MAX + 1, 8, 9, 3, 0, big)[0] == 2 and _plan(2, 2, 8, 129, 9, 3, 0, big)[0] == 2
    assert _plan(0, 2, 8, 8, 9, 3, 0, big)[0] == 1 and _plan(2, 2, 8, 8, 9, 0, 0, big)[0] == 1
    assert _lib.load().sk_truncated_wide_adjoint_plan(2, 2, 8, 8, 9, 3, 0, big, None) == 1


def test_the_c_entry_point_checks_its_arguments_without_a_device():
    from sigkernel_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    call = lambda **k: lib.sk_truncated_wide_adjoint(*[k.get(n, d) for n, d in (
        ("Xr", p), ("Yt", p), ("A", 1), ("B", 1), ("Mrows", 2), ("M", 2), ("N", 2), ("Ncp", 16), ("D", 9), ("fd", 16), ("L", 2), ("w", p),
        ("Tpart", p), ("n_chunks", 1), ("slab", p), ("slab_bytes", 1 << 20), ("stream", None), ("paired", 0))])
    assert call(Xr=None) == 1 and call(Yt=None) == 1 and call(w=None) == 1 and call(Tpart=None) == 1 and call(slab=None) == 1
    assert call(fd=8) == 1 and call(D=12, fd=8) == 1 and call(fd=24) == 1     # 16 staged coordinates, nothing else
    assert call(M=0) == 1 and call(Ncp=1) == 1 and call(N=17) == 1
    assert call(A=2, B=3, paired=1) == 1
    assert call(n_chunks=0) == 1 and call(n_chunks=2) == 1 and call(A=2, B=2, paired=1, n_chunks=2) == 1
    assert call(A=0) == 0                                                   # an empty batch launches nothing
    assert call(D=8, fd=8) == 2 and call(D=8) == 2 and call(D=17, fd=24) == 2     # SK_ERR_UNSUPPORTED outside the scope: dims
    assert call(L=9) == 2 and call(M=M_MAX + 1, Mrows=M_MAX + 1) == 2 and call(N=129, Ncp=144) == 2
    assert call(slab_bytes=2 * 1024 - 1) == 2                               # one lane a group: a block's slab is 2 steps x 1 KB; one byte less


# ---- host routing ----------------------------------------------------------------------------------------------------------------------------
class WideAdjointBackend:
    """Stand-in for HipBackend on CPU tensors -- TESTS ONLY: the route table and the plans are the library's (host only), the level terms
    are the torch restatement's and the wide adjoint is the closed form; every call is recorded in order"""
    name = "wide-adjoint-fake"

    def __init__(self):
        self.calls = []
        self.w = []

    def route(self, *args, **kw):
        from sigkernel_amd import _lib
        return _lib.HipBackend.route(*args, **kw)

    def truncated_adjoint_fits(self, *args, **kw):
        from sigkernel_amd import _lib
        return _lib.HipBackend().truncated_adjoint_fits(*args, **kw)

    def truncated_wide_adjoint_fits(self, *args, **kw):
        from sigkernel_amd import _lib
        return _lib.HipBackend().truncated_wide_adjoint_fits(*args, **kw)

    def truncated_levels(self, X, Y, num_levels, order, paired=False, kind=0, param=0.0):
        from sigkernel_amd import _lib
        from sigkernel_amd.truncated import _restatement
        fused = self.route(_lib.OP_TRUNCATED, order, X.shape[2], X.shape[1], Y.shape[1], num_levels, False, X.element_size()) == _lib.ROUTE_FUSED
        self.calls.append(("levels", X.shape[1], Y.shape[1], fused))
        return _restatement(X, Y, num_levels, None, order, paired, None) if fused else None

    def _closed(self, what, X, Y, w, paired):
        self.calls.append((what, X.shape[1], Y.shape[1], True))
        self.w.append(w.detach().clone())
        X, Y, w = X.detach().double(), Y.detach().double(), w.detach().double()
        if not paired:
            return closed_form(X, Y, w)[0]
        return torch.cat([closed_form(X[p:p + 1], Y[p:p + 1], w[:, p].reshape(-1, 1, 1))[0] for p in range(X.shape[0])], 0)

    def truncated_adjoint(self, X, Y, w, num_levels, paired=False, workspace_bytes=None):
        return self._closed("adjoint", X, Y, w, paired)

    def truncated_wide_adjoint(self, X, Y, w, num_levels, paired=False, workspace_bytes=None):
        assert w.shape[0] == num_levels and 9 <= X.shape[2] <= 16
        return self._closed("wide_adjoint", X, Y, w, paired)


@pytest.fixture
def fake(monkeypatch):
    from sigkernel_amd import _lib, truncated
    be = WideAdjointBackend()
    prev = _lib.set_backend(be)
    monkeypatch.setattr(_lib, "_dev", lambda t, name: t)
    monkeypatch.setattr(truncated, "_on_hip", lambda t: True)
    yield be
    _lib.set_backend(prev)


def _paths(M=20, N=17, D=9, A=2, B=3):
    """paths of M and N STEPS (M + 1 and N + 1 points), level weights, a weight per pair"""
    rng = np.random.default_rng(M + N + D)
    cum = lambda v: torch.as_tensor(np.concatenate([np.zeros((v.shape[0], 1, D)), np.cumsum(v, 1)], 1))
    return cum(steps(rng, A, M, D)), cum(steps(rng, B, N, D)), torch.as_tensor(rng.uniform(0.5, 1.5, 5)), torch.as_tensor(rng.standard_normal((A, B)))


def _restated(X, Y, sigma, c, grads, method="compute_Gram", order=1, **kw):
    """value and gradients of sum(c * method(X, Y)) through the torch restatement (no HIP stand-in asked: CPU tensors as they are)"""
    from sigkernel_amd import TruncatedSigKernel, truncated
    x, y = X.clone().requires_grad_("x" in grads), Y.clone().requires_grad_("y" in grads)
    prev = truncated._on_hip
    truncated._on_hip = lambda t: False
    try:
        K = getattr(TruncatedSigKernel(4, sigma, order), method)(x, x if Y is X else y, **kw)
        (K * c).sum().backward()
    finally:
        truncated._on_hip = prev
    return K.detach(), x.grad, y.grad


def _close(a, b):
    return float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())


def test_without_the_keyword_nothing_is_asked_at_dim_nine(fake):
    import sigkernel_amd
    X, Y, sigma, c = _paths()
    x = X.clone().requires_grad_()
    K = sigkernel_amd.TruncatedSigKernel(4, sigma).compute_Gram(x, Y)
    (K * c).sum().backward()
    assert fake.calls == []                 # a gradient pending at dim 9: the restatement as a whole, as before the keyword existed
    Kr, gx, _ = _restated(X, Y, sigma, c, "x")
    assert _close(K.detach(), Kr) and _close(x.grad, gx)
    with pytest.raises(TypeError):
        sigkernel_amd.TruncatedSigKernel(4, sigma, wide_adjoints=True)
    assert sigkernel_amd.TruncatedSigKernel(4).wide_adjoint is False


def test_keyword_is_levels_forward_and_one_wide_adjoint_call_per_side(fake):
    import sigkernel_amd
    X, Y, sigma, c = _paths()
    tk = sigkernel_amd.TruncatedSigKernel(4, sigma, wide_adjoint=True)
    x = X.clone().requires_grad_()
    K = tk.compute_Gram(x, Y)
    assert fake.calls == [("levels", 20, 17, True)]
    (K * c).sum().backward()
    assert fake.calls[1:] == [("wide_adjoint", 20, 17, True)]
    Kr, gx, _ = _restated(X, Y, sigma, c, "x")
    assert _close(K.detach(), Kr) and _close(x.grad, gx)
    wx = fake.w[0]
    assert torch.allclose(wx, (sigma[1:, None, None] * c[None]).double(), rtol=1e-15, atol=0)
    # Y requires grad too: a second call on (Y, X) with w transposed
    del fake.calls[:], fake.w[:]
    x, y = X.clone().requires_grad_(), Y.clone().requires_grad_()
    (tk.compute_Gram(x, y) * c).sum().backward()
    assert fake.calls == [("levels", 20, 17, True), ("wide_adjoint", 20, 17, True), ("wide_adjoint", 17, 20, True)]
    assert torch.equal(fake.w[0], wx) and torch.equal(fake.w[1], wx.transpose(1, 2))
    Kr, gx, gy = _restated(X, Y, sigma, c, "xy")
    assert _close(x.grad, gx) and _close(y.grad, gy)
    # only Y: one call, on (Y, X)
    del fake.calls[:], fake.w[:]
    y = Y.clone().requires_grad_()
    (tk.compute_Gram(X, y) * c).sum().backward()
    assert fake.calls == [("levels", 20, 17, True), ("wide_adjoint", 17, 20, True)] and _close(y.grad, gy)


def test_sym_is_one_call_with_w_plus_its_transpose(fake):
    import sigkernel_amd
    X, _, sigma, _ = _paths(A=3)
    c = torch.as_tensor(np.random.default_rng(3).standard_normal((3, 3)))       # not symmetric
    x = X.clone().requires_grad_()
    (sigkernel_amd.TruncatedSigKernel(4, sigma, wide_adjoint=True).compute_Gram(x, x, sym=True) * c).sum().backward()
    assert [k[0] for k in fake.calls] == ["levels", "wide_adjoint"]
    g = (sigma[1:, None, None] * c[None]).double()
    assert torch.allclose(fake.w[0], g + g.transpose(1, 2), rtol=1e-15, atol=0)
    _, gx, _ = _restated(X, X, sigma, c, "x", sym=True)
    assert _close(x.grad, gx)


def test_compute_kernel_and_sigma_keep_their_gradients(fake):
    import sigkernel_amd
    X, Y, sigma, c = _paths(A=3, B=3, D=12)
    s = sigma.clone().requires_grad_()
    x, y = X.clone().requires_grad_(), Y.clone().requires_grad_()
    k = sigkernel_amd.TruncatedSigKernel(4, s, wide_adjoint=True).compute_kernel(x, y)
    (k * c[0]).sum().backward()
    assert [k[0] for k in fake.calls] == ["levels", "wide_adjoint", "wide_adjoint"] and fake.w[0].shape == (4, 3)
    s2 = sigma.clone().requires_grad_()
    kr, gx, gy = _restated(X, Y, s2, c[0], "xy", method="compute_kernel")
    assert _close(k.detach(), kr) and _close(x.grad, gx) and _close(y.grad, gy) and _close(s.grad, s2.grad)


def test_compute_mmd_costs_no_adjoint_call_for_the_sample_without_a_gradient(fake):
    """K_XX is one levels call and ONE wide-adjoint call (sym), K_YY one levels call and nothing else, K_XY one of each"""
    import sigkernel_amd
    X, Y, sigma, _ = _paths(A=4, B=3, M=20, N=20)
    s = sigma.clone().requires_grad_()
    x = X.clone().requires_grad_()
    v = sigkernel_amd.TruncatedSigKernel(4, s, wide_adjoint=True).compute_mmd(x, Y)
    assert fake.calls == [("levels", 20, 20, True)] * 3
    v.backward()
    assert sorted(k[0] for k in fake.calls[3:]) == ["wide_adjoint", "wide_adjoint"]
    s2 = sigma.clone().requires_grad_()
    vr, gx, _ = _restated(X, Y, s2, torch.ones(()), "x", method="compute_mmd")
    assert abs(float(v.detach()) - float(vr)) <= 1e-12 * max(1.0, abs(float(vr))) and _close(x.grad, gx) and _close(s.grad, s2.grad)


def test_at_dim_five_the_plain_adjoint_is_asked_never_the_wide_one(fake):
    import sigkernel_amd
    X, Y, sigma, c = _paths(D=5)
    x, y = X.clone().requires_grad_(), Y.clone().requires_grad_()
    (sigkernel_amd.TruncatedSigKernel(4, sigma, wide_adjoint=True).compute_Gram(x, y) * c).sum().backward()
    assert fake.calls == [("levels", 20, 17, True), ("adjoint", 20, 17, True), ("adjoint", 17, 20, True)]


def test_everything_else_takes_the_restatement(fake):
    from sigkernel_amd import TruncatedSigKernel
    X, Y, sigma, c = _paths()
    # order 2
    x = X.clone().requires_grad_()
    (TruncatedSigKernel(4, sigma, order=2, wide_adjoint=True).compute_Gram(x, Y) * c).sum().backward()
    assert fake.calls == []
    _, gx, _ = _restated(X, Y, sigma, c, "x", order=2)
    assert _close(x.grad, gx)
    # 129 steps on the side that needs the gradient
    Xl, Yl, _, _ = _paths(M=M_MAX + 1)
    x = Xl.clone().requires_grad_()
    (TruncatedSigKernel(4, sigma, wide_adjoint=True).compute_Gram(x, Yl) * c).sum().backward()
    assert fake.calls == []
    _, gx, _ = _restated(Xl, Yl, sigma, c, "x")
    assert _close(x.grad, gx)
    # ... and on the other side: 16 x ceil16(129) doubles are no y block
    y = Yl.clone().requires_grad_()
    (TruncatedSigKernel(4, sigma, wide_adjoint=True).compute_Gram(y, Xl) * c.T).sum().backward()
    assert not any(k[0] == "wide_adjoint" for k in fake.calls) and y.grad is not None
    # an empty batch
    del fake.calls[:]
    x = X.clone().requires_grad_()
    K = TruncatedSigKernel(4, sigma, wide_adjoint=True).compute_Gram(x, Y[:0])
    assert fake.calls == [] and K.shape == (2, 0)
    # a workspace below one block's slab (3 levels x 32 steps x 1 KB)
    x = X.clone().requires_grad_()
    (TruncatedSigKernel(4, sigma, wide_adjoint=True, workspace_bytes=1 << 16).compute_Gram(x, Y) * c).sum().backward()
    assert fake.calls == [] and x.grad is not None
    # no gradient pending (torch.no_grad(), or no leaf): the levels launch alone, as without the keyword -- the wide mode is never asked
    with torch.no_grad():
        TruncatedSigKernel(4, sigma, wide_adjoint=True).compute_Gram(X.clone().requires_grad_(), Y)
    assert fake.calls == [("levels", 20, 17, True)]
    del fake.calls[:]
    TruncatedSigKernel(4, sigma, wide_adjoint=True).compute_Gram(X, Y)
    assert fake.calls == [("levels", 20, 17, True)]


def test_a_backend_without_the_method_sees_no_difference(monkeypatch):
    import sigkernel_amd
    from sigkernel_amd import _lib, truncated
    monkeypatch.setattr(_lib, "_dev", lambda t, name: t)
    monkeypatch.setattr(truncated, "_on_hip", lambda t: True)

    class Plain:
        route = WideAdjointBackend.route
        truncated_adjoint_fits = WideAdjointBackend.truncated_adjoint_fits
        truncated_levels = WideAdjointBackend.truncated_levels

        def __init__(self):
            self.calls = []
    be = Plain()
    prev = _lib.set_backend(be)
    try:
        X, Y, sigma, c = _paths()
        x = X.clone().requires_grad_()
        (sigkernel_amd.TruncatedSigKernel(4, sigma, wide_adjoint=True).compute_Gram(x, Y) * c).sum().backward()
    finally:
        _lib.set_backend(prev)
    assert be.calls == [] and x.grad is not None
    _, gx, _ = _restated(X, Y, sigma, c, "x")
    assert _close(x.grad, gx)
