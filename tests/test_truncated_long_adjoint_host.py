"""The truncated kernel's LONG-ADJOINT mode without a GPU (csrc/sk_truncated.hip: trunc_long_adjoint): the SK_OP_TRUNCATED_LONG_ADJOINT
rows of the route table, the plan's slab arithmetic, the C entry point's argument checks, the banded reverse sweep restated in numpy and
held to autograd of the torch restatement, and the routing of TruncatedSigKernel(long_adjoint=True) on a stand-in backend.

The scheme, for one pair with G (M x N), P^m the exclusive 2-D prefix of level m (R^1 = G, R^{m+1} = G P^m) and weights w_1 .. w_L:
    Rb^L = w_L,  Rb^m = w_m + exclusive 2-D SUFFIX of (G Rb^{m+1}),  dG = sum_m Rb^m P^{m-1}  (P^0 = 1),  dx_i = sum_j dG[i][j] y_j
    rows in BANDS, columns in TILES.  A forward pass keeps every band's incoming carry (the prefix at the band's first row, per level and
    column); then the bands from the last to the first: the band's prefix factors again from its carry, tiles left to right, then the
    mirrored sweep, tiles right to left, with rowT (a row's sum over the tiles to the right) kept across the tiles and a REVERSE carry (the
    suffix over all later rows, per level and column) handed to the band above through one of two halves.
Every test here fails on the parent: no operation 9, no export, and the keyword is a TypeError.  Shapes are in STEPS."""
import ctypes

import numpy as np
import pytest
import torch

from test_truncated_host import steps


def q(op, D, M, N, L, order, es=8, flags=0):
    from sigkernel_amd import _lib
    return int(_lib.load().sk_route_query(op, order, D, M, N, L, 0, es, flags))


def test_version_and_the_op_number():
    from sigkernel_amd import _lib
    assert _lib.load().sk_version() == 340
    assert _lib.OP_TRUNCATED_LONG_ADJOINT == 9


def test_route_table_states_the_long_adjoint_scope():
    from sigkernel_amd import _lib
    F, W, S = _lib.ROUTE_FUSED, _lib.ROUTE_FUSED_SWAP, _lib.ROUTE_STREAM
    op = _lib.OP_TRUNCATED_LONG_ADJOINT
    for D, M, N, L in ((8, 129, 129, 8), (8, 40, 300, 3), (1, 1 << 20, 1 << 20, 8), (8, 128, 256, 8)):
        assert q(op, D, M, N, L, 1) == F, (D, M, N, L)
    assert q(op, 8, 128, 256, 8, 1) == q(_lib.OP_TRUNCATED_ADJOINT, 8, 128, 256, 8, 1) == F       # a plain-adjoint shape: inside both
    assert q(op, 9, 129, 129, 8, 1) == S and q(op, 8, 129, 129, 9, 1) == S
    assert q(op, 8, 129, 129, 2, 2) == S and q(op, 8, 129, 129, 8, -1) == S and q(op, 8, 129, 129, 4, 3) == S
    assert q(op, 8, 129, 129, 1, -1) == F and q(op, 8, 129, 129, 1, 2) == F                       # one level is order 1
    assert q(op, 8, (1 << 20) + 1, 5, 4, 1) == S and q(op, 8, 5, (1 << 20) + 1, 4, 1) == S and q(op, 0, 5, 5, 4, 1) == S
    assert q(op, 8, 129, 129, 8, 1, 4) == F and q(op, 8, 129, 129, 8, 1, 2) == S
    # never swapped: the gradient goes to the rows -- also where the long FORWARD prefers (y, x)
    for M, N in ((130, 128), (129, 1000), (1000, 129), (5, 700), (700, 5)):
        assert q(op, 8, M, N, 8, 1) == F
    assert q(_lib.OP_TRUNCATED_LONG, 8, 130, 128, 8, 1) == W


def test_pinned_rows_of_the_other_truncated_routes_are_unchanged():
    from sigkernel_amd import _lib
    F, W, S = _lib.ROUTE_FUSED, _lib.ROUTE_FUSED_SWAP, _lib.ROUTE_STREAM
    p = lambda *a, **k: q(_lib.OP_TRUNCATED, *a, **k)
    assert p(8, 128, 256, 8, 1) == F and p(16, 128, 128, 8, 1) == F and p(8, 64, 256, 8, 4) == F
    assert p(4, 129, 127, 8, 1) == W and p(8, 130, 65, 5, 1) == W and p(3, 200, 21, 4, 3) == W
    assert p(4, 129, 129, 8, 1) == S and p(8, 128, 257, 8, 1) == S and p(17, 20, 15, 3, 1) == S and p(4, 20, 15, 6, 5) == S
    a = lambda *a, **k: q(_lib.OP_TRUNCATED_ADJOINT, *a, **k)
    assert a(8, 128, 256, 8, 1) == F and a(8, 129, 20, 8, 1) == S and a(9, 20, 20, 4, 1) == S and a(8, 20, 257, 4, 1) == S and a(8, 20, 20, 4, 2) == S
    lg = lambda *a, **k: q(_lib.OP_TRUNCATED_LONG, *a, **k)
    assert lg(8, 128, 130, 8, 1) == F and lg(8, 130, 128, 8, 1) == W and lg(8, 1000, 129, 8, 1) == F and lg(16, 513, 512, 8, 1) != S
    assert lg(8, 300, 300, 2, 2) == S and lg(17, 300, 300, 8, 1) == S


def _plan(A, B, M, N, D, L, paired, ws):
    from sigkernel_amd import _lib
    out = (ctypes.c_int64 * 4)()
    rc = _lib.load().sk_truncated_long_adjoint_plan(A, B, M, N, D, L, paired, ws, ctypes.cast(out, ctypes.c_void_p))
    return rc, tuple(out)


def block_bytes(M, N, L, W):
    """the header's formula: the factors of ONE band, (L - 1) x (N + tiles x (W - 1)) KB, and with more than one band the carry planes
    and the two reverse-carry halves, (bands + 2) x (L - 1) x ceil64(N) doubles"""
    tiles, bands, Ns = -(-N // 256), -(-M // (2 * W)), -(-N // 64) * 64
    return (L - 1) * (N + tiles * (W - 1)) * 1024 + ((bands + 2) * (L - 1) * Ns * 8 if bands > 1 else 0)


def test_plan_counts_one_slab_a_block():
    """sk_truncated_long_adjoint_plan (host only): plan[0..3] = n_chunks, blocks, the launch's slab bytes, ONE block's slab bytes"""
    big = 1 << 40
    # one band with one tile: 20 lanes -> groups of 32, two a wave; 3 paths are 2 row tiles, the 2 second paths one chunk each
    rc, (n_chunks, blocks, total, block) = _plan(3, 2, 40, 40, 3, 4, 0, big)
    assert rc == 0 and block == block_bytes(40, 40, 4, 32) == 3 * 71 * 1024 and (n_chunks, blocks, total) == (2, 4, 4 * block)
    # one band with two tiles: the skew drains twice
    rc, (n_chunks, blocks, total, block) = _plan(3, 2, 40, 300, 2, 3, 0, big)
    assert rc == 0 and block == block_bytes(40, 300, 3, 32) == 2 * (300 + 2 * 31) * 1024 and total == blocks * block
    # three bands: one pair a wave, 64 lanes, five carry planes of 7 x 128 doubles
    rc, (n_chunks, blocks, total, block) = _plan(3, 2, 257, 70, 8, 8, 0, big)
    assert rc == 0 and block == block_bytes(257, 70, 8, 64) == 7 * (133 * 1024 + 5 * 128 * 8) and (n_chunks, blocks, total) == (2, 6, 6 * block)
    # two bands x two tiles
    rc, (n_chunks, blocks, total, block) = _plan(3, 2, 130, 257, 5, 2, 0, big)
    assert rc == 0 and block == block_bytes(130, 257, 2, 64) == (257 + 2 * 63) * 1024 + 4 * 320 * 8
    # one level: no slab at all, whatever the workspace
    rc, (n_chunks, blocks, total, block) = _plan(3, 2, 200, 300, 4, 1, 0, 0)
    assert rc == 0 and block == 0 and total == 0 and blocks == 6
    # paired: one chunk, 5 pairs of two bands, one a wave
    rc, (n_chunks, blocks, total, block) = _plan(5, 5, 200, 270, 4, 4, 1, big)
    assert rc == 0 and (n_chunks, blocks) == (1, 5) and block == block_bytes(200, 270, 4, 64) and total == 5 * block
    # every shape of the plain adjoint's scope has a plan, with the plain adjoint's factor slab
    rc, (n_chunks, blocks, total, block) = _plan(5, 37, 20, 33, 3, 6, 0, big)
    assert rc == 0 and block == 5 * (33 + 15) * 1024 and n_chunks == 37
    # the blocks fall from 8 per CU until the slabs fit
    rc, (n_chunks, full, total, block) = _plan(50, 45, 129, 300, 2, 8, 0, big)
    assert rc == 0 and full > 2 and total == full * block
    rc, (n2, blocks, total, b2) = _plan(50, 45, 129, 300, 2, 8, 0, 2 * block + 5)
    assert rc == 0 and blocks == 2 < full and total == 2 * block and b2 == block and n2 == n_chunks
    rc, (_, blocks, total, _) = _plan(50, 45, 129, 300, 2, 8, 0, block)
    assert rc == 0 and blocks == 1 and total == block                   # exactly one slab leaves one block
    assert _plan(50, 45, 129, 300, 2, 8, 0, block - 1)[0] == 2          # one byte less: SK_ERR_UNSUPPORTED
    # outside the scope, and bad arguments
    assert _plan(2, 2, 300, 300, 9, 3, 0, big)[0] == 2 and _plan(2, 2, 300, 300, 4, 9, 0, big)[0] == 2
    assert _plan(0, 2, 300, 300, 4, 3, 0, big)[0] == 1 and _plan(2, 2, 0, 300, 4, 3, 0, big)[0] == 1 and _plan(2, 2, 300, 300, 4, 0, 0, big)[0] == 1
    from sigkernel_amd import _lib
    assert _lib.load().sk_truncated_long_adjoint_plan(2, 2, 300, 300, 4, 3, 0, big, None) == 1


def test_the_c_entry_point_checks_its_arguments_without_a_device():
    from sigkernel_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    call = lambda **k: lib.sk_truncated_long_adjoint(*[k.get(n, d) for n, d in (
        ("Xr", p), ("Yt", p), ("A", 1), ("B", 1), ("Mrows", 2), ("M", 2), ("N", 2), ("Ncp", 16), ("D", 2), ("fd", 8), ("L", 2), ("w", p),
        ("Tpart", p), ("n_chunks", 1), ("slab", p), ("slab_bytes", 1 << 20), ("stream", None), ("paired", 0))])
    assert call(Xr=None) == 1 and call(Yt=None) == 1 and call(w=None) == 1 and call(Tpart=None) == 1 and call(slab=None) == 1
    assert call(M=0) == 1 and call(Ncp=1) == 1 and call(Ncp=24) == 1 and call(fd=16) == 1 and call(n_chunks=0) == 1 and call(n_chunks=2) == 1
    assert call(A=0) == 0                                   # an empty batch launches nothing
    assert call(L=9) == 2 and call(D=9, fd=16) == 2         # SK_ERR_UNSUPPORTED outside the scope
    assert call(slab_bytes=2 * 1024 - 1) == 2               # one lane a group: a block's slab is 2 steps x 1 KB; one byte less
    assert call(M=300, Mrows=300, N=300, Ncp=304, slab_bytes=block_bytes(300, 300, 2, 64) - 1) == 2


# ---- the scheme, restated ------------------------------------------------------------------------------------------------------------------
def _excl(a, axis, reverse=False):
    """exclusive running sum along `axis`, from the front or (reverse) from the back"""
    a = np.flip(a, axis) if reverse else a
    c = np.cumsum(a, axis)
    c = np.concatenate([np.zeros_like(np.take(c, [0], axis)), np.delete(c, -1, axis)], axis)
    return np.flip(c, axis) if reverse else c


def _band_forward(Gb, cin, L, tile, carry_out=None, fac=None):
    """one band's forward sweep through the tiles, left to right, from its incoming carry cin[s][j]: the prefix factors P^{s+1} into fac[s]
    and / or what the last row hands down into carry_out[s][j]"""
    rows, N = Gb.shape
    rowS = np.zeros((max(L - 1, 1), rows))
    for c0 in range(0, N, tile):
        Gt = Gb[:, c0:c0 + tile]
        R = Gt
        for s in range(L - 1):
            rowpre = rowS[s][:, None] + _excl(R, 1)
            P = cin[s, c0:c0 + tile][None, :] + _excl(rowpre, 0)
            if carry_out is not None:
                carry_out[s, c0:c0 + tile] = cin[s, c0:c0 + tile] + rowpre.sum(0)
            if fac is not None:
                fac[s][:, c0:c0 + tile] = P
            rowS[s] += R.sum(1)
            R = Gt * P


def banded_adjoint(G, w, band=128, tile=256):
    """dG of sum_m w[m - 1] k_m for ONE pair by the kernel's scheme (the module docstring) in fp64 numpy"""
    M, N = G.shape
    L = len(w)
    starts = list(range(0, M, band))
    fcar = np.zeros((len(starts), max(L - 1, 1), N))                # every band's incoming carry is kept: plane 0 stays zeros
    for k, r0 in enumerate(starts[:-1]):
        _band_forward(G[r0:r0 + band], fcar[k], L, tile, carry_out=fcar[k + 1])
    dG = np.zeros_like(G)
    rcar = np.full((2, max(L - 1, 1), N), np.nan)                   # two halves: band k writes half k & 1 and reads the other
    for k in reversed(range(len(starts))):
        Gb = G[starts[k]:starts[k] + band]
        rows = Gb.shape[0]
        fac = np.zeros((max(L - 1, 1), rows, N))
        _band_forward(Gb, fcar[k], L, tile, fac=fac)                # (a)
        rin = rcar[(k + 1) & 1] if k + 1 < len(starts) else np.zeros((max(L - 1, 1), N))
        rowT = np.zeros((max(L - 1, 1), rows))
        for c0 in reversed(range(0, N, tile)):                      # (b): tiles right to left
            Gt, sl = Gb[:, c0:c0 + tile], slice(c0, c0 + tile)
            rb = np.full(Gt.shape, w[L - 1])
            d = rb * (fac[L - 2][:, sl] if L > 1 else 1.0)
            for m in range(L, 1, -1):
                s = m - 2
                U = Gt * rb
                rowsuf = rowT[s][:, None] + _excl(U, 1, reverse=True)       # the row's U to the right, the tiles done before included
                rb = w[s] + rin[s, sl][None, :] + _excl(rowsuf, 0, reverse=True)
                rcar[k & 1][s, sl] = rin[s, sl] + rowsuf.sum(0)
                rowT[s] += U.sum(1)
                d = d + rb * (fac[s - 1][:, sl] if s > 0 else 1.0)
            dG[starts[k]:starts[k] + band, sl] = d
    return dG


@pytest.mark.parametrize("M,N,L", [(9, 11, 4), (4, 5, 1), (13, 3, 8), (3, 12, 2)])
def test_banded_reverse_sweep_against_autograd_of_the_restatement(M, N, L):
    """bands of 4 rows, tiles of 5 columns: forward carries per band, the reverse carry through its two halves, rowT across the tiles.
    Bar: 1e-12 of the gradient's max-norm (the restatement sits <= 2.1e-15 from the closed form, test_truncated_adjoint_host.py)."""
    from sigkernel_amd.truncated import _restatement
    A, B, D = 2, 3, 3
    rng = np.random.default_rng(100 * M + N + L)
    X, Y = steps(rng, A, M, D), steps(rng, B, N, D)
    w = rng.standard_normal((L, A, B))
    Xt = torch.as_tensor(X).requires_grad_()
    lev = _restatement(Xt, torch.as_tensor(Y), L, None, 1, False, None)
    (lev[1:] * torch.as_tensor(w)).sum().backward()
    want = Xt.grad.numpy()
    got = np.zeros_like(X)
    for a in range(A):
        for b in range(B):
            got[a] += banded_adjoint(X[a] @ Y[b].T, w[:, a, b], band=4, tile=5) @ Y[b]
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print("banded reverse sweep vs autograd", (M, N, L), "%.1e" % err)
    assert err <= 1e-12, err
    # ... and whatever the bands and tiles: one band with one tile is trunc_adjoint's sweep
    one = sum(banded_adjoint(X[0] @ Y[b].T, w[:, 0, b], band=M, tile=N) @ Y[b] for b in range(B))
    assert float(np.abs(one - want[0]).max() / np.abs(want).max()) <= 1e-12


# ---- host routing ----------------------------------------------------------------------------------------------------------------------------
class LongAdjointBackend:
    """Stand-in for HipBackend on CPU tensors -- TESTS ONLY: the route table and the plans are the library's (host only), values and
    gradients are the torch restatement's; every call is recorded in order"""
    name = "long-adjoint-fake"

    def __init__(self):
        self.calls = []
        self.w = []

    def route(self, *args, **kw):
        from sigkernel_amd import _lib
        return _lib.HipBackend.route(*args, **kw)

    def truncated_adjoint_fits(self, *args, **kw):
        from sigkernel_amd import _lib
        return _lib.HipBackend().truncated_adjoint_fits(*args, **kw)

    def truncated_long_adjoint_fits(self, *args, **kw):
        from sigkernel_amd import _lib
        return _lib.HipBackend().truncated_long_adjoint_fits(*args, **kw)

    def truncated_levels(self, X, Y, num_levels, order, paired=False, kind=0, param=0.0):
        from sigkernel_amd import _lib
        from sigkernel_amd.truncated import _restatement
        fused = self.route(_lib.OP_TRUNCATED, order, X.shape[2], X.shape[1], Y.shape[1], num_levels, False, X.element_size()) == _lib.ROUTE_FUSED
        self.calls.append(("levels", X.shape[1], Y.shape[1], fused))
        return _restatement(X, Y, num_levels, None, order, paired, None) if fused else None

    def truncated_long(self, X, Y, num_levels, sigma, paired=False, workspace_bytes=None):
        from sigkernel_amd import _lib
        from sigkernel_amd.truncated import _restatement
        assert not X.requires_grad and not Y.requires_grad
        fused = self.route(_lib.OP_TRUNCATED_LONG, 1, X.shape[2], X.shape[1], Y.shape[1], num_levels, False, X.element_size()) == _lib.ROUTE_FUSED
        self.calls.append(("long", X.shape[1], Y.shape[1], fused))
        return _restatement(X, Y, num_levels, sigma, 1, paired, None) if fused else None

    def _grad(self, what, X, Y, w, L, paired):
        from sigkernel_amd.truncated import _restatement
        self.calls.append((what, X.shape[1], Y.shape[1], True))
        self.w.append(w.detach().clone())
        with torch.enable_grad():
            x = X.detach().clone().requires_grad_()
            (_restatement(x, Y.detach(), L, None, 1, paired, None)[1:] * w).sum().backward()
        return x.grad.double()

    def truncated_adjoint(self, X, Y, w, num_levels, paired=False, workspace_bytes=None):
        return self._grad("adjoint", X, Y, w, num_levels, paired)

    def truncated_long_adjoint(self, X, Y, w, num_levels, paired=False, workspace_bytes=None):
        return self._grad("long_adjoint", X, Y, w, num_levels, paired)


@pytest.fixture
def fake(monkeypatch):
    from sigkernel_amd import _lib, truncated
    be = LongAdjointBackend()
    prev = _lib.set_backend(be)
    monkeypatch.setattr(_lib, "_dev", lambda t, name: t)
    monkeypatch.setattr(truncated, "_on_hip", lambda t: True)
    yield be
    _lib.set_backend(prev)


def _paths(M=130, N=131, D=3, A=2, B=3):
    """paths of M and N STEPS (M + 1 and N + 1 points), level weights, a weight per pair"""
    rng = np.random.default_rng(M + N + D)
    cum = lambda v: torch.as_tensor(np.concatenate([np.zeros((v.shape[0], 1, D)), np.cumsum(v, 1)], 1))
    return cum(steps(rng, A, M, D)), cum(steps(rng, B, N, D)), torch.as_tensor(rng.uniform(0.5, 1.5, 5)), torch.as_tensor(rng.standard_normal((A, B)))


def _restated(X, Y, sigma, c, grads, method="compute_Gram", order=1, static_kernel=None, **kw):
    """value and gradients of sum(c * method(X, Y)) through the torch restatement (no HIP stand-in asked: CPU tensors as they are)"""
    from sigkernel_amd import TruncatedSigKernel, _lib, truncated
    x, y = X.clone().requires_grad_("x" in grads), Y.clone().requires_grad_("y" in grads)
    prev = truncated._on_hip
    truncated._on_hip = lambda t: False
    try:
        K = getattr(TruncatedSigKernel(4, sigma, order, static_kernel=static_kernel), method)(x, x if Y is X else y, **kw)
        (K * c).sum().backward()
    finally:
        truncated._on_hip = prev
    return K.detach(), x.grad, y.grad


def _close(a, b):
    return float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())


def test_without_the_keyword_the_method_is_never_asked(fake, monkeypatch):
    import sigkernel_amd
    X, Y, sigma, c = _paths()
    for switch in (False, True):
        monkeypatch.setattr(sigkernel_amd.routes, "truncated_long", switch)
        x = X.clone().requires_grad_()
        (sigkernel_amd.TruncatedSigKernel(4, sigma).compute_Gram(x, Y) * c).sum().backward()
        assert fake.calls == [] and x.grad is not None      # a gradient pending: the restatement as a whole, as before the keyword existed
        with pytest.raises(TypeError):
            sigkernel_amd.TruncatedSigKernel(4, sigma, long_adjoints=True)
    assert sigkernel_amd.TruncatedSigKernel(4).long_adjoint is False


@pytest.mark.parametrize("switch", [False, True])
def test_keyword_routes_forward_and_backward_to_the_long_calls(fake, monkeypatch, switch):
    """130 x 131 steps: the long forward on (Y, X) (two steps shorter), one adjoint call per batch that requires grad; the keyword does
    not depend on routes.truncated_long"""
    import sigkernel_amd
    monkeypatch.setattr(sigkernel_amd.routes, "truncated_long", switch)
    X, Y, sigma, c = _paths()
    tk = sigkernel_amd.TruncatedSigKernel(4, sigma, long_adjoint=True)
    x = X.clone().requires_grad_()
    K = tk.compute_Gram(x, Y)
    assert fake.calls == [("long", 130, 131, False), ("long", 131, 130, True)]
    (K * c).sum().backward()
    assert fake.calls[2:] == [("long_adjoint", 130, 131, True)]
    Kr, gx, _ = _restated(X, Y, sigma, c, "x")
    assert _close(K.detach(), Kr) and _close(x.grad, gx)
    wx = fake.w[0]
    # Y requires grad too: a second adjoint call on (Y, X) with w transposed
    del fake.calls[:], fake.w[:]
    x, y = X.clone().requires_grad_(), Y.clone().requires_grad_()
    (tk.compute_Gram(x, y) * c).sum().backward()
    assert fake.calls[2:] == [("long_adjoint", 130, 131, True), ("long_adjoint", 131, 130, True)]
    assert torch.equal(fake.w[0], wx) and torch.equal(fake.w[1], wx.transpose(1, 2))
    Kr, gx, gy = _restated(X, Y, sigma, c, "xy")
    assert _close(x.grad, gx) and _close(y.grad, gy)
    # only Y: one adjoint call, on (Y, X)
    del fake.calls[:], fake.w[:]
    y = Y.clone().requires_grad_()
    (tk.compute_Gram(X, y) * c).sum().backward()
    assert fake.calls[2:] == [("long_adjoint", 131, 130, True)] and _close(y.grad, gy)


def test_sym_is_one_adjoint_call_with_w_plus_its_transpose(fake):
    import sigkernel_amd
    X, _, sigma, _ = _paths(A=3)
    c = torch.as_tensor(np.random.default_rng(3).standard_normal((3, 3)))       # not symmetric
    x = X.clone().requires_grad_()
    (sigkernel_amd.TruncatedSigKernel(4, sigma, long_adjoint=True).compute_Gram(x, x, sym=True) * c).sum().backward()
    assert [k[0] for k in fake.calls] == ["long", "long_adjoint"]
    g = (sigma[1:, None, None] * c[None]).double()
    assert torch.allclose(fake.w[0], g + g.transpose(1, 2), rtol=1e-15, atol=0)
    _, gx, _ = _restated(X, X, sigma, c, "x", sym=True)
    assert _close(x.grad, gx)


def test_paired_and_sigma_keep_their_gradients(fake):
    import sigkernel_amd
    X, Y, sigma, c = _paths(A=3, B=3)
    s = sigma.clone().requires_grad_()
    x, y = X.clone().requires_grad_(), Y.clone().requires_grad_()
    k = sigkernel_amd.TruncatedSigKernel(4, s, long_adjoint=True).compute_kernel(x, y)
    (k * c[0]).sum().backward()
    assert [k[0] for k in fake.calls] == ["long", "long", "long_adjoint", "long_adjoint"] and fake.w[0].shape == (4, 3)
    from sigkernel_amd import truncated
    s2 = sigma.clone().requires_grad_()
    kr, gx, gy = _restated(X, Y, s2, c[0], "xy", method="compute_kernel")
    assert _close(k.detach(), kr) and _close(x.grad, gx) and _close(y.grad, gy) and _close(s.grad, s2.grad)


def test_inside_the_plain_adjoints_scope_the_existing_route_is_taken(fake):
    import sigkernel_amd
    X, Y, sigma, c = _paths(100, 120)
    x, y = X.clone().requires_grad_(), Y.clone().requires_grad_()
    (sigkernel_amd.TruncatedSigKernel(4, sigma, long_adjoint=True).compute_Gram(x, y) * c).sum().backward()
    assert fake.calls == [("levels", 100, 120, True), ("adjoint", 100, 120, True), ("adjoint", 120, 100, True)]


def test_everything_else_takes_the_restatement(fake):
    import sigkernel_amd
    from sigkernel_amd import RBFKernel, TruncatedSigKernel
    X, Y, sigma, c = _paths()
    for kw in (dict(order=2), dict(static_kernel=RBFKernel(0.8))):
        x = X.clone().requires_grad_()
        (TruncatedSigKernel(4, sigma, long_adjoint=True, **kw).compute_Gram(x, Y) * c).sum().backward()
        assert not any(k[0] in ("long", "long_adjoint") for k in fake.calls), (kw, fake.calls)
        _, gx, _ = _restated(X, Y, sigma, c, "x", **kw)
        assert _close(x.grad, gx)
    X9, Y9, _, _ = _paths(D=9)
    del fake.calls[:]
    x = X9.clone().requires_grad_()
    (TruncatedSigKernel(4, sigma, long_adjoint=True).compute_Gram(x, Y9) * c).sum().backward()
    assert not any(k[0] in ("long", "long_adjoint") for k in fake.calls)
    # dim 9 in the batch that needs NO gradient is out of the adjoint's scope all the same (one dim for both): nothing is asked
    # a workspace below one block's slab: the restatement
    del fake.calls[:]
    x = X.clone().requires_grad_()
    (TruncatedSigKernel(4, sigma, long_adjoint=True, workspace_bytes=1 << 16).compute_Gram(x, Y) * c).sum().backward()
    assert fake.calls == [] and x.grad is not None
    # no gradient pending: the keyword changes nothing (the switch is off: the restatement)
    del fake.calls[:]
    TruncatedSigKernel(4, sigma, long_adjoint=True).compute_Gram(X, Y)
    assert fake.calls == []


def test_a_backend_without_the_method_sees_no_difference(monkeypatch):
    import sigkernel_amd
    from sigkernel_amd import _lib, truncated
    monkeypatch.setattr(_lib, "_dev", lambda t, name: t)
    monkeypatch.setattr(truncated, "_on_hip", lambda t: True)

    class Plain:
        route = LongAdjointBackend.route
        truncated_adjoint_fits = LongAdjointBackend.truncated_adjoint_fits
        truncated_levels = LongAdjointBackend.truncated_levels
        truncated_long = LongAdjointBackend.truncated_long

        def __init__(self):
            self.calls = []
    be = Plain()
    prev = _lib.set_backend(be)
    try:
        X, Y, sigma, c = _paths()
        x = X.clone().requires_grad_()
        (sigkernel_amd.TruncatedSigKernel(4, sigma, long_adjoint=True).compute_Gram(x, Y) * c).sum().backward()
    finally:
        _lib.set_backend(prev)
    assert be.calls == [] and x.grad is not None
    _, gx, _ = _restated(X, Y, sigma, c, "x")
    assert _close(x.grad, gx)
