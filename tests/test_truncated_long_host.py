"""The truncated kernel's LONG mode without a GPU (csrc/sk_truncated.hip: trunc_long): the SK_OP_TRUNCATED_LONG rows of the route table,
the plan's slab, the band / tile / carry scheme of the sweep restated in numpy and held to a plain long-double double loop, and the
routing of the public functions and TruncatedSigKernel behind the opt-in switch `sigkernel_amd.routes.truncated_long` on a stand-in backend.

The scheme, for one pair with G (M x N) and level s + 1 = R_s (R_0 = G, R_{s+1} = G x exclusive 2-D prefix of R_s):
    rows in BANDS of 128, columns in TILES of 2048 / fd; inside a band and a tile
        rowpre(i, j) = rowS[s][i] + sum_{tile's j' < j} R_s(i, j')                      (rowS: the row's sum over the tiles before)
        P(i, j)      = carry[s][j] + sum_{band's i' < i} rowpre(i', j)                   (carry: zeros in band 0)
        carry[s][j] += sum_{band's i} rowpre(i, j)      in place, for the next band;     rowS[s][i] += the row's sum over the tile
Shapes are (M, N, D, L) in STEPS."""
import ctypes

import numpy as np
import pytest
import torch

from test_truncated_host import steps


def q(D, M, N, L, order, es=8, op=None, flags=0):
    from sigkernel_amd import _lib
    return int(_lib.load().sk_route_query(_lib.OP_TRUNCATED_LONG if op is None else op, order, D, M, N, L, 0, es, flags))


def test_version_and_the_op_number():
    from sigkernel_amd import _lib
    assert _lib.load().sk_version() == 340
    assert _lib.OP_TRUNCATED_LONG == 8


def test_route_table_states_the_long_scope():
    """fails on the parent, whose sk_route_query knows no operation 8"""
    from sigkernel_amd import _lib
    F, W, S = _lib.ROUTE_FUSED, _lib.ROUTE_FUSED_SWAP, _lib.ROUTE_STREAM
    assert q(8, 128, 130, 8, 1) == F            # one band of 193 steps against two of 191
    assert q(8, 130, 128, 8, 1) == W
    assert q(8, 1000, 129, 8, 1) == F           # 8 bands x 192 steps against 2 bands x (1000 + 4 x 63)
    assert q(8, 129, 1000, 8, 1) == W
    assert q(16, 513, 512, 8, 1) != S
    assert q(4, 300, 300, 1, -1) != S           # one level is order 1
    assert q(8, 129, 1000, 8, 1, flags=_lib.ROUTE_NO_SWAP) == F
    assert q(8, 128, 130, 8, 1, 4) == F
    # every order-1 shape of the plain scope is inside: one shape, both launches
    assert q(8, 128, 256, 8, 1) == F and q(8, 128, 256, 8, 1, op=_lib.OP_TRUNCATED) == F
    assert q(8, 1 << 20, 1 << 20, 8, 1) == F and q(8, (1 << 20) + 1, 5, 8, 1) == S and q(8, 5, (1 << 20) + 1, 8, 1) == S
    for args in ((8, 300, 300, 2, 2), (8, 300, 300, 8, -1), (8, 300, 300, 4, 3)):      # order 2 and beyond with L >= 2
        assert q(*args) == S
    assert q(17, 300, 300, 8, 1) == S and q(8, 300, 300, 9, 1) == S and q(8, 300, 300, 8, 1, 2) == S and q(0, 300, 300, 8, 1) == S


def test_pinned_rows_of_the_plain_route_are_unchanged():
    from sigkernel_amd import _lib
    F, W, S = _lib.ROUTE_FUSED, _lib.ROUTE_FUSED_SWAP, _lib.ROUTE_STREAM
    p = lambda *a, **k: q(*a, op=_lib.OP_TRUNCATED, **k)
    assert p(8, 128, 256, 8, 1) == F and p(16, 128, 128, 8, 1) == F and p(8, 64, 256, 8, 4) == F
    assert p(4, 129, 127, 8, 1) == W and p(8, 130, 65, 5, 1) == W and p(3, 200, 21, 4, 3) == W
    assert p(4, 129, 129, 8, 1) == S and p(4, 130, 131, 3, 1) == S and p(8, 64, 257, 3, 2) == S and p(9, 64, 129, 3, 2) == S
    assert p(8, 128, 257, 8, 1) == S and p(17, 20, 15, 3, 1) == S and p(4, 20, 15, 9, 1) == S and p(4, 20, 15, 6, 5) == S


def _plan(A, B, M, N, D, L, paired, ws):
    from sigkernel_amd import _lib
    out = (ctypes.c_int64 * 3)()
    rc = _lib.load().sk_truncated_long_plan(A, B, M, N, D, L, paired, ws, ctypes.cast(out, ctypes.c_void_p))
    return rc, tuple(out)


def test_plan_counts_one_slab_a_block():
    """sk_truncated_long_plan (host only): blocks, one block's slab -- (L - 1) planes of ceil64(N) doubles beyond one band and one level --
    and their product; the blocks fall until the slabs fit"""
    # one band (M <= 128) or one level: no slab, whatever the workspace
    for args in ((3, 5, 128, 1000, 8, 8, 0), (3, 5, 40, 600, 3, 6, 0), (3, 5, 300, 300, 4, 1, 0), (7, 7, 128, 300, 4, 6, 1)):
        rc, (blocks, block, total) = _plan(*args, 0)
        assert rc == 0 and block == 0 and total == 0 and blocks >= 1, args
    rc, (blocks, block, total) = _plan(3, 5, 40, 600, 3, 6, 0, 1 << 30)
    assert blocks == 10                                     # 20 lanes -> groups of 32, two a wave: 2 row tiles x 5 columns
    # bands: one pair a wave, a slab of 7 x 320 doubles
    rc, (blocks, block, total) = _plan(50, 45, 129, 300, 2, 8, 0, 1 << 30)
    assert rc == 0 and block == 7 * 320 * 8 and blocks == min(50 * 45, blocks) and total == blocks * block
    full = blocks
    rc, (blocks, block, total) = _plan(50, 45, 129, 300, 2, 8, 0, 2 * block + 5)
    assert rc == 0 and blocks == 2 < full and total == 2 * block
    rc, (blocks, block, total) = _plan(50, 45, 129, 300, 2, 8, 0, block)
    assert rc == 0 and blocks == 1
    assert _plan(50, 45, 129, 300, 2, 8, 0, block - 1)[0] == 2          # SK_ERR_UNSUPPORTED below one slab
    rc, (blocks, block, total) = _plan(5, 5, 200, 270, 4, 6, 1, 1 << 30)        # paired: 5 pairs, one a wave
    assert rc == 0 and blocks == 5 and block == 5 * 320 * 8 and total == 5 * block
    rc, (blocks, block, total) = _plan(2, 2, 257, 129, 9, 3, 0, 1 << 30)
    assert rc == 0 and blocks == 4 and block == 2 * 192 * 8
    # outside the scope, and bad arguments
    assert _plan(2, 2, 300, 300, 17, 3, 0, 1 << 30)[0] == 2 and _plan(2, 2, 300, 300, 4, 9, 0, 1 << 30)[0] == 2
    assert _plan(0, 2, 300, 300, 4, 3, 0, 1 << 30)[0] == 1 and _plan(2, 2, 0, 300, 4, 3, 0, 1 << 30)[0] == 1


def test_the_c_entry_point_checks_its_arguments_without_a_device():
    from sigkernel_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    call = lambda **k: lib.sk_truncated_long_f64(*[k.get(n, d) for n, d in (
        ("Xr", p), ("Yt", p), ("A", 1), ("B", 1), ("Mrows", 2), ("M", 2), ("N", 2), ("Ncp", 16), ("D", 2), ("fd", 8), ("L", 2), ("order", 1),
        ("paired", 0), ("levels", 0), ("sigma", p), ("slab", None), ("slab_bytes", 0), ("out", p), ("stream", None))])
    assert call(Xr=None) == 1 and call(out=None) == 1 and call(sigma=None) == 1 and call(M=0) == 1 and call(Ncp=1) == 1 and call(slab_bytes=8) == 1
    assert call(A=0) == 0                       # an empty batch launches nothing
    assert call(order=2) == 2 and call(L=9) == 2 and call(D=17, fd=24) == 2       # SK_ERR_UNSUPPORTED outside the scope
    assert call(Ncp=24) == 1 and call(fd=16) == 1                                 # Ncp a multiple of 16, fd the staging rule's


# ---- the scheme, restated ------------------------------------------------------------------------------------------------------------------
def banded_levels(G, L, band=128, tile=256):
    """k_1 .. k_L of ONE pair by the sweep's band / tile / carry scheme in fp64 numpy (the module docstring)"""
    M, N = G.shape
    tot = np.zeros(L)
    carry = np.zeros((max(L - 1, 1), N))                    # the slab: written in place, never cleared between bands
    for r0 in range(0, M, band):
        Gb = G[r0:r0 + band]
        rowS = np.zeros((max(L - 1, 1), Gb.shape[0]))
        first = r0 == 0
        for c0 in range(0, N, tile):
            Gt = Gb[:, c0:c0 + tile]
            R = Gt
            tot[0] += R.sum()
            for s in range(L - 1):
                inc = np.cumsum(R, 1)
                rowpre = rowS[s][:, None] + np.concatenate([np.zeros((R.shape[0], 1)), inc[:, :-1]], 1)
                cin = np.zeros(Gt.shape[1]) if first else carry[s, c0:c0 + tile]        # band 0 takes zeros, not what the slab holds
                down = np.cumsum(rowpre, 0)
                P = cin[None, :] + np.concatenate([np.zeros((1, R.shape[1])), down[:-1]], 0)
                carry[s, c0:c0 + tile] = cin + down[-1]
                rowS[s] += inc[:, -1]
                R = Gt * P
                tot[s + 1] += R.sum()
    return tot


def long_double_levels(G, L):
    """k_1 .. k_L of one pair: a plain double loop per level in long double"""
    G = G.astype(np.longdouble)
    M, N = G.shape
    R, out = G, [G.sum()]
    for _ in range(1, L):
        P = np.zeros((M + 1, N + 1), dtype=np.longdouble)       # P[i + 1][j + 1]: the inclusive prefix at (i, j)
        for i in range(M):
            row = np.longdouble(0)
            for j in range(N):
                row += R[i, j]
                P[i + 1, j + 1] = P[i, j + 1] + row
        R = G * P[:M, :N]
        out.append(R.sum())
    return np.array(out, dtype=np.longdouble)


@pytest.mark.parametrize("M,N,D,L,tile", [(129, 130, 4, 8, 256), (257, 259, 4, 4, 256), (40, 600, 3, 6, 256), (130, 131, 9, 3, 128)])
def test_band_tile_carry_scheme_against_a_long_double_double_loop(M, N, D, L, tile):
    """every level within 1e-13 of the level's largest entry over the pairs; the slab dirty from the pair before"""
    if np.finfo(np.longdouble).eps > 2e-19:
        pytest.skip("no extended precision on this host")
    rng = np.random.default_rng(1000 * M + N)
    X, Y = steps(rng, 1, M, D), steps(rng, 2, N, D)
    got = np.stack([banded_levels(X[0] @ Y[b].T, L, 128, tile) for b in range(2)])
    want = np.stack([long_double_levels(X[0] @ Y[b].T, L) for b in range(2)])
    err = np.abs(got - want).max(0) / np.abs(want).max(0)
    print("band/tile/carry vs long double", (M, N, D, L), ["%.1e" % float(e) for e in err])
    assert float(err.max()) <= 1e-13, err
    # ... and the torch restatement the GPU tests use as their reference
    from sigkernel_amd.truncated import _truncated_levels_torch
    ref = _truncated_levels_torch(torch.as_tensor(X), torch.as_tensor(Y), L, 1)[1:, 0].T.numpy()
    assert float((np.abs(ref - want).max(0) / np.abs(want).max(0)).max()) <= 1e-13


# ---- host routing ----------------------------------------------------------------------------------------------------------------------------
class LongBackend:
    """Stand-in for HipBackend on CPU tensors -- TESTS ONLY: the route table is the library's (host only), values are the torch
    restatement's; every call is recorded in order"""
    name = "long-fake"

    def __init__(self):
        self.calls = []

    def route(self, *args, **kw):
        from sigkernel_amd import _lib
        return _lib.HipBackend.route(*args, **kw)

    def truncated_adjoint_fits(self, *args, **kw):
        from sigkernel_amd import _lib
        return _lib.HipBackend().truncated_adjoint_fits(*args, **kw)

    def _plain(self, what, X, Y, L, sigma, order, paired):
        from sigkernel_amd import _lib
        from sigkernel_amd.truncated import _restatement
        fused = self.route(_lib.OP_TRUNCATED, order, X.shape[2], X.shape[1], Y.shape[1], L, False, X.element_size()) == _lib.ROUTE_FUSED
        self.calls.append((what, X.shape[1], Y.shape[1], fused))
        return _restatement(X, Y, L, sigma, order, paired, None) if fused else None

    def truncated_gram(self, X, Y, num_levels, sigma, order, kind=0, param=0.0):
        return self._plain("gram", X, Y, num_levels, sigma, order, False)

    def truncated_paired(self, X, Y, num_levels, sigma, order, kind=0, param=0.0):
        return self._plain("paired", X, Y, num_levels, sigma, order, True)

    def truncated_levels(self, X, Y, num_levels, order, paired=False, kind=0, param=0.0):
        return self._plain("levels", X, Y, num_levels, None, order, paired)

    def truncated_long(self, X, Y, num_levels, sigma, paired=False, workspace_bytes=None):
        from sigkernel_amd import _lib
        from sigkernel_amd.truncated import _restatement
        assert not X.requires_grad and not Y.requires_grad
        fused = self.route(_lib.OP_TRUNCATED_LONG, 1, X.shape[2], X.shape[1], Y.shape[1], num_levels, False, X.element_size()) == _lib.ROUTE_FUSED
        self.calls.append(("long", X.shape[1], Y.shape[1], fused))
        return _restatement(X, Y, num_levels, sigma, 1, paired, None) if fused else None


@pytest.fixture
def fake(monkeypatch):
    from sigkernel_amd import _lib, truncated
    be = LongBackend()
    prev = _lib.set_backend(be)
    monkeypatch.setattr(_lib, "_dev", lambda t, name: t)
    monkeypatch.setattr(truncated, "_on_hip", lambda t: True)
    yield be
    _lib.set_backend(prev)


def _inputs(M=130, N=131, D=3, A=2, B=3):
    rng = np.random.default_rng(M + N)
    return torch.as_tensor(steps(rng, A, M, D)), torch.as_tensor(steps(rng, B, N, D)), torch.as_tensor(rng.uniform(0.5, 1.5, 5))


def test_switch_off_never_asks_the_long_method(fake):
    import sigkernel_amd
    assert sigkernel_amd.routes.truncated_long is False
    X, Y, sigma = _inputs()
    sigkernel_amd.truncated_sig_kernel(X, Y, 4, sigma, 1)
    sigkernel_amd.truncated_sig_kernel_levels(X, Y, 4, 1)
    sigkernel_amd.truncated_sig_kernel_paired(X[:2], Y[:2], 4, sigma, 1)
    sigkernel_amd.TruncatedSigKernel(4, sigma).compute_Gram(torch.cumsum(X, 1), torch.cumsum(Y, 1))
    assert fake.calls and not any(c[0] == "long" for c in fake.calls)


def test_switch_on_asks_after_the_plain_method_declined_both_orientations(fake, monkeypatch):
    import sigkernel_amd
    from sigkernel_amd.truncated import _truncated_torch, _truncated_levels_torch, _truncated_paired_torch
    monkeypatch.setattr(sigkernel_amd.routes, "truncated_long", True)
    X, Y, sigma = _inputs()         # 130 x 131 steps, two bands either way: the sweep on (Y, X) is two steps shorter
    K = sigkernel_amd.truncated_sig_kernel(X, Y, 4, sigma, 1)
    assert fake.calls == [("gram", 130, 131, False), ("gram", 131, 130, False), ("long", 130, 131, False), ("long", 131, 130, True)]
    assert K.shape == (2, 3) and K.is_contiguous()
    assert torch.allclose(K, _truncated_torch(X, Y, 4, sigma, 1), rtol=1e-13, atol=0)
    del fake.calls[:]
    Kt = sigkernel_amd.truncated_sig_kernel(Y, X, 4, sigma, 1)      # ... which is the first orientation of this call
    assert fake.calls[2:] == [("long", 131, 130, True)]
    assert Kt.shape == (3, 2) and torch.allclose(Kt, K.T, rtol=1e-13, atol=0)
    del fake.calls[:]
    lev = sigkernel_amd.truncated_sig_kernel_levels(X, Y, 4, 1)
    assert [c[0] for c in fake.calls] == ["levels", "levels", "long", "long"]
    assert lev.shape == (5, 2, 3) and torch.allclose(lev, _truncated_levels_torch(X, Y, 4, 1), rtol=1e-13, atol=0)
    del fake.calls[:]
    k = sigkernel_amd.truncated_sig_kernel_paired(X, Y[:2], 4, sigma, 1)
    assert [c[0] for c in fake.calls] == ["paired", "paired", "long", "long"]
    assert torch.allclose(k, _truncated_paired_torch(X, Y[:2], 4, sigma, 1), rtol=1e-13, atol=0)
    del fake.calls[:]
    lev = sigkernel_amd.truncated_sig_kernel_levels(X, Y[:2], 4, 1, paired=True)
    assert [c[0] for c in fake.calls] == ["levels", "levels", "long", "long"] and lev.shape == (5, 2)
    del fake.calls[:]
    Kn = sigkernel_amd.truncated_sig_kernel(X, Y, 4, sigma, 1, normalize=True)     # normalize: its two diagonals through the paired route
    assert [c for c in fake.calls if c[0] == "long" and c[3]] == [("long", 131, 130, True), ("long", 130, 130, True), ("long", 131, 131, True)]
    kx, ky = _truncated_paired_torch(X, X, 4, sigma, 1), _truncated_paired_torch(Y, Y, 4, sigma, 1)
    assert torch.allclose(Kn, K / torch.sqrt(kx[:, None] * ky[None, :]), rtol=1e-12, atol=0)


def test_inside_the_plain_scope_the_long_method_is_not_asked(fake, monkeypatch):
    import sigkernel_amd
    monkeypatch.setattr(sigkernel_amd.routes, "truncated_long", True)
    X, Y, sigma = _inputs(128, 131)
    sigkernel_amd.truncated_sig_kernel(X, Y, 4, sigma, 1)
    sigkernel_amd.truncated_sig_kernel(Y, X, 4, sigma, 1)
    assert fake.calls == [("gram", 128, 131, True), ("gram", 131, 128, False), ("gram", 128, 131, True)]


def test_other_orders_and_pending_gradients_take_the_restatement(fake, monkeypatch):
    import sigkernel_amd
    monkeypatch.setattr(sigkernel_amd.routes, "truncated_long", True)
    X, Y, sigma = _inputs()
    sigkernel_amd.truncated_sig_kernel(X, Y, 4, sigma, 2)
    sigkernel_amd.truncated_sig_kernel(X, Y, 4, sigma, -1)
    sigkernel_amd.truncated_sig_kernel_levels(X, Y, 4, 3)
    assert not any(c[0] == "long" for c in fake.calls)
    del fake.calls[:]
    Xg = X.clone().requires_grad_()
    assert sigkernel_amd.truncated_sig_kernel(Xg, Y, 4, sigma, 1).requires_grad
    assert sigkernel_amd.truncated_sig_kernel(X, Y, 4, sigma.clone().requires_grad_(), 1).requires_grad
    assert sigkernel_amd.truncated_sig_kernel_levels(X, Y.clone().requires_grad_(), 4, 1).requires_grad
    assert fake.calls == []
    with torch.no_grad():
        sigkernel_amd.truncated_sig_kernel(Xg, Y, 4, sigma, 1)
    assert [c[0] for c in fake.calls] == ["gram", "gram", "long", "long"]
    del fake.calls[:]
    sigkernel_amd.truncated_sig_kernel(X, Y, 1, 1.0, -1)             # one level IS order 1
    assert [c[0] for c in fake.calls] == ["gram", "gram", "long", "long"]


def test_object_on_its_plain_kernel_takes_the_long_route(fake, monkeypatch):
    import sigkernel_amd
    from sigkernel_amd import LinearKernel, RBFKernel, TruncatedSigKernel
    monkeypatch.setattr(sigkernel_amd.routes, "truncated_long", True)
    X, Y, sigma = _inputs()
    PX, PY = torch.cumsum(X, 1), torch.cumsum(Y, 1)           # 130 points: 129 steps; 131 points: 130 steps
    want = TruncatedSigKernel(4, sigma).compute_Gram(PX.clone().requires_grad_(), PY)       # a gradient pending: the restatement
    assert want.requires_grad and fake.calls == []
    for sk in (None, LinearKernel()):
        del fake.calls[:]
        K = TruncatedSigKernel(4, sigma, static_kernel=sk).compute_Gram(PX, PY)
        assert fake.calls == [("long", 129, 130, False), ("long", 130, 129, True)]
        assert torch.allclose(K, want.detach(), rtol=1e-12, atol=0)
    del fake.calls[:]
    k = TruncatedSigKernel(4, sigma).compute_kernel(PX, PY[:2])
    assert fake.calls == [("long", 129, 130, False), ("long", 130, 129, True)] and k.shape == (2,)
    del fake.calls[:]
    TruncatedSigKernel(4, sigma, order=2).compute_Gram(PX, PY)
    TruncatedSigKernel(4, sigma, static_kernel=RBFKernel(0.8)).compute_Gram(PX, PY)      # the lift on long paths: not in this mode
    assert not any(c[0] == "long" for c in fake.calls)


def test_a_backend_without_the_method_sees_no_difference(monkeypatch):
    import sigkernel_amd
    from sigkernel_amd import _lib, truncated
    monkeypatch.setattr(sigkernel_amd.routes, "truncated_long", True)
    monkeypatch.setattr(_lib, "_dev", lambda t, name: t)
    monkeypatch.setattr(truncated, "_on_hip", lambda t: True)

    class Plain:
        route = LongBackend.route
        truncated_adjoint_fits = LongBackend.truncated_adjoint_fits
        _plain = LongBackend._plain
        truncated_gram = LongBackend.truncated_gram
        truncated_levels = LongBackend.truncated_levels

        def __init__(self):
            self.calls = []
    be = Plain()
    prev = _lib.set_backend(be)
    try:
        X, Y, sigma = _inputs()
        K = sigkernel_amd.truncated_sig_kernel(X, Y, 4, sigma, 1)
        sigkernel_amd.TruncatedSigKernel(4, sigma).compute_Gram(torch.cumsum(X, 1), torch.cumsum(Y, 1))
    finally:
        _lib.set_backend(prev)
    assert [c[0] for c in be.calls] == ["gram", "gram"] and K.shape == (2, 3)


def test_the_switch_reads_its_environment_variable(monkeypatch):
    from sigkernel_amd import _routes
    assert _routes._ENV["truncated_long"] == "SK_TRUNCATED_LONG" and "SK_TRUNCATED_LONG" in _routes.__doc__
    monkeypatch.setenv("SK_TRUNCATED_LONG", "1")
    assert _routes.Routes().truncated_long is True
    monkeypatch.delenv("SK_TRUNCATED_LONG")
    assert _routes.Routes().truncated_long is False
