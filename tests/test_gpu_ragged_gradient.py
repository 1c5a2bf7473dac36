"""Ragged batches with gradients under SigKernel(exact_gradient=True) on the GPU: sk_solve_adj_* with SK_FLAG_DISCRETE | SK_FLAG_RAGGED
against the restatement (tests/exact_gradient_reference.py) on every pair's own sub-block, the two bit-equalities that follow from
"the arithmetic of a cell does not depend on how far the sweep continues", the C entry point with reused slots and NaN-filled memory,
and torch.autograd.gradcheck through the ragged methods."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import sigkernel_amd
from sigkernel_amd import _lib
import exact_gradient_reference as R
from poison import poisoned, same_bits
from test_ragged_gradient_host import LX, LY, _paths, _ref_gram, _ref_pair

DEV = "cuda:0"
VALUE_BAR = 1e-10        # the project's value bar, relative to max |W|
GRAD_BAR = 1e-8          # the project's gradient bar, relative to each path's max-norm gradient
GRADCHECK = dict(eps=1e-6, atol=1e-7, rtol=1e-6)      # the settings of tests/test_gpu_exact_gradient.py

# padded (Mc, Nc, d): both orientations, fine diagonals longer than 64 lanes (80 and 70 nodes), dyadic orders 0..2
SHAPES = [(9, 5, 1), (5, 9, 1), (40, 3, 1), (3, 70, 0), (7, 6, 2)]
P = 7


def _table(Mc, Nc):
    """7 pairs: empty on either side, the full block IMMEDIATELY before the smallest sub-grid, an interior one, one-cell rows / columns.
    With two slots (the C-entry test) block 0 takes pairs 0, 2, 4, 6: the full grid, then the interior one in the slot it left full."""
    m, n = Mc // 2 + 1, Nc // 2 + 1
    return np.array([(0, n), (m, 0), (Mc, Nc), (1, 1), (m, n), (Mc, 1), (1, Nc)], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _case(shape, naive, f32):
    """(increments (P, Mc, Nc), table, final (P,), W (P, Mc, Nc)) of the restatement on the sub-blocks, zeros elsewhere: computed once"""
    Mc, Nc, d = shape
    inc = np.random.default_rng(7 * Mc + Nc + d).normal(scale=0.3, size=(P, Mc, Nc))
    if f32:
        inc = inc.astype(np.float32).astype(np.float64)
    return (inc, _table(Mc, Nc)) + _reference(inc, _table(Mc, Nc), d, naive)


def _reference(inc, tab, d, naive):
    k, W = np.ones(inc.shape[0]), np.zeros_like(inc)
    for p, (mc, nc) in enumerate(tab):
        if mc > 0 and nc > 0:
            k[p], W[p, :mc, :nc] = R.exact_adjoint(inc[p, :mc, :nc], d, naive)
    return k, W


def _padded(inc, dtype):
    """the increments on the device in rows padded to whole cache lines, as a view of their first Nc columns"""
    n, Mc, Nc = inc.shape
    ld = _lib._padded_ld(Nc, 8 if dtype == torch.float64 else 4)
    buf = torch.zeros(n, Mc, ld, dtype=dtype, device=DEV)
    buf[..., :Nc] = torch.from_numpy(inc).to(DEV, dtype)
    return buf[..., :Nc]


def _outside(tab, Mc, Nc):
    """mask (P, Mc, Nc) of the cells outside each pair's sub-block"""
    a, b = np.arange(Mc)[None, :, None], np.arange(Nc)[None, None, :]
    return (a >= tab[:, 0, None, None]) | (b >= tab[:, 1, None, None])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("naive", [False, True], ids=["default", "naive"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_d%d" % s)
def test_ragged_adjoint_against_the_restatement(shape, naive, dtype):
    """W and the value of solve_adj(discrete=True, cells=...) against the recurrence on the sub-blocks, 1e-10 x max |W| (fp32 storage:
    plus half an fp32 ulp element by element, as in test_discrete_adjoint_against_the_restatement); exact zeros outside the sub-blocks;
    in fp64 the two bit-equalities: the contiguous slice solved alone, and node (mc << d, nc << d) of the padded pair's forward grid."""
    Mc, Nc, d = shape
    inc, tab, want_k, want_w = _case(shape, naive, dtype == torch.float32)
    be = _lib.HipBackend()
    dinc = _padded(inc, dtype)
    k, W, res = be.solve_adj(dinc, d, naive, discrete=True, cells=torch.from_numpy(tab).to(DEV), return_residual=True)
    assert k.dtype == dtype and W.dtype == dtype and W.shape == (P, Mc, Nc)
    Wh, kh = W.double().cpu().numpy(), k.double().cpu().numpy()
    store = 2.0 ** -24 if dtype == torch.float32 else 0.0
    err = np.abs(Wh - want_w)
    print("worst |W - restatement| / max |W| = %.3e" % (err.max() / np.abs(want_w).max()))
    assert np.all(err <= VALUE_BAR * np.abs(want_w).max() + store * np.abs(want_w))
    assert np.all(np.abs(kh - want_k) <= VALUE_BAR * np.abs(want_k) + store * np.abs(want_k))
    assert np.all(Wh[_outside(tab, Mc, Nc)] == 0.0)
    assert np.all(kh[:2] == 1.0)                       # an empty sub-grid: exactly 1
    assert not res.cpu().numpy().any()
    if dtype == torch.float64:
        _, grid, _ = be.solve_fwd(dinc, d, naive, flags=_lib.FLAG_SIMPLE, want_grid=True)
        for p, (mc, nc) in enumerate(tab.tolist()):
            assert same_bits(k[p], grid[p, mc << d, nc << d])[0], p
            if mc > 0 and nc > 0:
                k1, W1 = be.solve_adj(dinc[p:p + 1, :mc, :nc].contiguous(), d, naive, discrete=True)
                ok, msg = same_bits(W[p, :mc, :nc].contiguous(), W1[0].contiguous())
                assert ok, (p, msg)
                assert same_bits(k[p], k1[0])[0], p


def _c_entry(lib, buf, ld, tab, Mc, Nc, d, naive, slots, ldw, flags=None, short=0):
    """sk_solve_adj_f64 with the ragged flags on NaN-filled W, value vector, residuals and slots; returns (rc, k, W, err) on the host"""
    n = tab.shape[0]
    slot = int(lib.sk_adj_rescue_slot_bytes(Mc, Nc, d))
    head = (8 * n + 255) // 256 * 256
    ws = torch.full(((head + slots * slot) // 8,), float("nan"), dtype=torch.float64, device=DEV)
    ws.view(torch.int32)[:2 * n] = torch.from_numpy(tab.reshape(-1)).to(DEV)
    W = torch.full((n, Mc, ldw), float("nan"), dtype=torch.float64, device=DEV)
    k = torch.full((n,), float("nan"), dtype=torch.float64, device=DEV)
    err = torch.full((n,), float("nan"), dtype=torch.float64, device=DEV)
    rc = lib.sk_solve_adj_f64(buf.data_ptr(), ld, n, Mc, Nc, d, _lib.SCHEME_NAIVE if naive else _lib.SCHEME_DEFAULT,
                              _lib.FLAG_DISCRETE | _lib.FLAG_RAGGED if flags is None else flags, k.data_ptr(), W.data_ptr(), ldw,
                              err.data_ptr(), ws.data_ptr(), ctypes.c_size_t(head + slots * slot - short), _lib._stream(buf))
    torch.cuda.synchronize()
    return rc, k.cpu().numpy(), W.cpu().numpy(), err.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("naive", [False, True], ids=["default", "naive"])
def test_ragged_adjoint_reuses_its_slots_and_reads_nothing_unwritten(naive):
    """The C entry point itself: 7 pairs with workspace for only 2 blocks (every slot serves several pairs, a small sub-grid after the
    full one), odd ld / ldw, and slots, W, value vector and the increments' padding columns full of NaN before the launch: no result may
    depend on unwritten memory and the padding of W stays untouched.  The flag's argument checks; and a table with values outside
    [0, Mc] x [0, Nc] gives what the clamped table gives (all of it on valid memory)."""
    shape = (9, 5, 1)
    Mc, Nc, d = shape
    ld, ldw = Nc + 3, Nc + 5
    inc, tab, want_k, want_w = _case(shape, naive, False)
    buf = torch.full((P, Mc, ld), float("nan"), dtype=torch.float64, device=DEV)
    buf[..., :Nc] = torch.from_numpy(inc).to(DEV)
    lib = _lib.load()
    slot = int(lib.sk_adj_rescue_slot_bytes(Mc, Nc, d))
    both = _lib.FLAG_DISCRETE | _lib.FLAG_RAGGED
    assert int(lib.sk_adj_workspace_bytes(P, Mc, Nc, d, both, 8)) == 256 + P * slot
    assert int(lib.sk_adj_workspace_bytes(33, Mc, Nc, d, both, 8)) == 512 + 33 * slot
    assert int(lib.sk_adj_workspace_bytes(P, Mc, Nc, d, _lib.FLAG_RAGGED, 8)) == 0
    rc, k, W, err = _c_entry(lib, buf, ld, tab, Mc, Nc, d, naive, 2, ldw)
    assert rc == 0, rc
    assert np.isnan(W[..., Nc:]).all()
    assert np.abs(W[..., :Nc] - want_w).max() <= VALUE_BAR * np.abs(want_w).max()
    assert np.all(W[..., :Nc][_outside(tab, Mc, Nc)] == 0.0)
    assert np.abs(k - want_k).max() <= VALUE_BAR * np.abs(want_k).max()
    assert not err.any()
    # the slots' count does not reach the bits: one slot per pair gives the same
    rc, k7, W7, _ = _c_entry(lib, buf, ld, tab, Mc, Nc, d, naive, P, ldw)
    assert rc == 0 and np.array_equal(k7, k) and np.array_equal(W7[..., :Nc], W[..., :Nc])
    # a table outside the block is clamped
    wild = np.array([(-3, Nc + 5), (Mc + 100, -1), (2 ** 31 - 1, 2 ** 31 - 1), (1, 1), (Mc // 2 + 1, Nc + 1), (-2 ** 31, 4), (1, 2 ** 30)], dtype=np.int32)
    clamped = np.clip(wild, 0, [Mc, Nc]).astype(np.int32)
    rc1, k1, W1, _ = _c_entry(lib, buf, ld, wild, Mc, Nc, d, naive, 2, ldw)
    rc2, k2, W2, _ = _c_entry(lib, buf, ld, clamped, Mc, Nc, d, naive, 2, ldw)
    assert rc1 == 0 and rc2 == 0
    assert np.array_equal(k1, k2) and np.array_equal(W1[..., :Nc], W2[..., :Nc]) and np.isnan(W1[..., Nc:]).all()
    ck, cw = _reference(inc, clamped, d, naive)
    assert np.abs(W1[..., :Nc] - cw).max() <= VALUE_BAR * np.abs(cw).max() and np.abs(k1 - ck).max() <= VALUE_BAR * np.abs(ck).max()
    # the flag alone, or with "fast only", is a bad argument; a workspace that holds the head but not one slot is refused
    assert _c_entry(lib, buf, ld, tab, Mc, Nc, d, naive, 2, ldw, flags=_lib.FLAG_RAGGED)[0] != 0
    assert _c_entry(lib, buf, ld, tab, Mc, Nc, d, naive, 2, ldw, flags=both | _lib.FLAG_FAST_ONLY)[0] != 0
    assert _c_entry(lib, buf, ld, tab, Mc, Nc, d, naive, 1, ldw, short=8)[0] != 0


@pytest.mark.gpu
def test_ragged_adjoint_under_poisoned_allocations():
    """Through the binding with every torch.empty of the library filled with 0xFF (NaN) and 0x55 (huge, finite): the bits of a plain call."""
    be = _lib.HipBackend()
    inc, tab, _, _ = _case((7, 6, 2), False, False)
    dinc, cells = _padded(inc, torch.float64), torch.from_numpy(tab).to(DEV)
    k0, W0 = be.solve_adj(dinc, 2, discrete=True, cells=cells)
    for byte in (0xFF, 0x55):
        with poisoned(byte) as p:
            k, W = be.solve_adj(dinc, 2, discrete=True, cells=cells)
        assert p.count > 0
        assert same_bits(k0, k)[0] and same_bits(W0.contiguous(), W.contiguous())[0]


class CubicKernel:
    """a duck-typed static kernel (neither LinearKernel nor RBFKernel): k(x, y) = (1 + <x, y> / 2)^3"""

    def batch_kernel(self, X, Y):
        return (1. + 0.5 * torch.bmm(X, Y.transpose(1, 2))) ** 3

    def Gram_matrix(self, X, Y):
        return (1. + 0.5 * torch.matmul(X[:, None], Y[None].transpose(-1, -2))) ** 3


def _walks(seed, *shape):
    gen = torch.Generator().manual_seed(seed)
    return torch.cumsum(0.5 * torch.randn(*shape, generator=gen, dtype=torch.float64), dim=1).to(DEV)


GX, GY = [4, 2], [5, 1, 3]        # A = 2, B = 3, M = 4, N = 5: the padded length, two points, one point, an interior length


def _gradcheck_all(sk, X, Y):
    """compute_kernel_ragged and compute_Gram_ragged in both arguments, compute_Gram_ragged(x, x, sym=True), compute_mmd_ragged.  The
    padded points are inputs like any other: their numerical and their analytic gradient are both zero."""
    X, Y = X.clone().requires_grad_(True), Y.clone().requires_grad_(True)
    Yp = Y[:X.shape[0]].detach().clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x, y: sk.compute_kernel_ragged(x, y, GX, GY[:2]), (X, Yp), **GRADCHECK)
    assert torch.autograd.gradcheck(lambda x, y: sk.compute_Gram_ragged(x, y, GX, GY), (X, Y), **GRADCHECK)
    assert torch.autograd.gradcheck(lambda x: sk.compute_Gram_ragged(x, x, GX, GX, sym=True), (X,), **GRADCHECK)
    assert torch.autograd.gradcheck(lambda x, y: sk.compute_mmd_ragged(x, GX, y, GY), (X, Y), **GRADCHECK)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,d,naive", [("linear", 0, False), ("linear", 1, False), ("rbf", 0, False), ("rbf", 1, False), ("rbf", 1, True)],
                         ids=["linear_d0", "linear_d1", "rbf_d0", "rbf_d1", "rbf_d1_naive"])
def test_gradcheck(kernel, d, naive):
    """A = 2, B = 3, M = 4, N = 5, D = 2, fp64, lengths [4, 2] and [5, 1, 3]"""
    k = sigkernel_amd.LinearKernel() if kernel == "linear" else sigkernel_amd.RBFKernel(0.7)
    sk = sigkernel_amd.SigKernel(k, d, _naive_solver=naive, exact_gradient=True)
    _gradcheck_all(sk, _walks(1, 2, 4, 2), _walks(2, 3, 5, 2))


@pytest.mark.gpu
def test_gradcheck_duck_typed_static_kernel():
    sk = sigkernel_amd.SigKernel(CubicKernel(), 1, exact_gradient=True)
    _gradcheck_all(sk, 0.5 * _walks(3, 2, 4, 2), 0.5 * _walks(4, 3, 5, 2))


@pytest.mark.gpu
def test_gradcheck_function_valued_kernel():
    """paths (batch, T, Lx, d) through RBF_ID_Kernel's feature map: the gradient reaches them through torch autograd of the map"""
    sk = sigkernel_amd.SigKernel(sigkernel_amd.RBF_ID_Kernel(0.7), 1, exact_gradient=True)
    _gradcheck_all(sk, _walks(5, 2, 4, 2).reshape(2, 4, 2, 1), _walks(6, 3, 5, 2).reshape(3, 5, 2, 1))


@pytest.mark.gpu
def test_gradcheck_linear_paths_wider_than_the_second_argument_kernel():
    """LinearKernel at dim 9: dL/dY of a Gram block comes from the swapped contraction, with the table's W transposed like any other"""
    sk = sigkernel_amd.SigKernel(sigkernel_amd.LinearKernel(), 1, exact_gradient=True)
    X, Y = (0.5 * _walks(14, 2, 4, 9)).requires_grad_(True), (0.5 * _walks(15, 3, 5, 9)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x, y: sk.compute_Gram_ragged(x, y, GX, GY), (X, Y), **GRADCHECK)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["linear", "rbf"])
def test_full_lengths_give_the_gradients_of_compute_Gram_bit_for_bit(kernel):
    k = sigkernel_amd.LinearKernel() if kernel == "linear" else sigkernel_amd.RBFKernel(0.7)
    sk = sigkernel_amd.SigKernel(k, 1, exact_gradient=True)
    Xc, Yc = _walks(21, 3, 6, 3), _walks(22, 4, 5, 3)
    w = torch.randn(3, 4, generator=torch.Generator().manual_seed(3), dtype=torch.float64).to(DEV)
    grads = []
    for ragged in (False, True):
        X, Y = Xc.clone().requires_grad_(True), Yc.clone().requires_grad_(True)
        K = sk.compute_Gram_ragged(X, Y, [6] * 3, [5] * 4) if ragged else sk.compute_Gram(X, Y)
        (K * w).sum().backward()
        grads.append((X.grad, Y.grad))
    assert same_bits(grads[0][0], grads[1][0])[0] and same_bits(grads[0][1], grads[1][1])[0]


def _worst(got, want):
    """max over the paths of |error| / the path's max-norm gradient (a path whose gradient is zero must get exactly zero)"""
    worst = 0.0
    for a in range(want.shape[0]):
        scale, err = np.abs(want[a]).max(), np.abs(got[a] - want[a]).max()
        if scale == 0.0:
            assert err == 0.0, a
        else:
            worst = max(worst, err / scale)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("garbage", [False, True], ids=["repeated", "garbage"])
@pytest.mark.parametrize("d", [0, 1])
@pytest.mark.parametrize("kernel", ["linear", "rbf"])
def test_gradients_on_the_host_tests_inputs(kernel, d, garbage):
    """The inputs of tests/test_ragged_gradient_host.py (lengths 1, 2 and the padded length; padding = the repeated last point, or
    finite garbage): Gram and paired gradients within 1e-8 of each path's max-norm of CPU autograd through the restatement on the
    truncated paths, and exactly zero on every padded point."""
    k = sigkernel_amd.LinearKernel() if kernel == "linear" else sigkernel_amd.RBFKernel(1.0)
    sk = sigkernel_amd.SigKernel(k, d, exact_gradient=True)
    Xc, Yc = _paths(garbage)
    gen = torch.Generator().manual_seed(9)
    w, wp = torch.randn(3, 4, generator=gen, dtype=torch.float64), torch.randn(3, generator=gen, dtype=torch.float64)
    Xr, Yr = Xc.clone().requires_grad_(True), Yc.clone().requires_grad_(True)
    want = torch.autograd.grad((_ref_gram(Xr, LX, Yr, LY, k, d, False) * w).sum(), (Xr, Yr))
    wantp = torch.autograd.grad((torch.stack([_ref_pair(Xr[a, :LX[a]], Yr[a, :LY[a]], k, d, False) for a in range(3)]) * wp).sum(), (Xr, Yr))
    X, Y = Xc.to(DEV).requires_grad_(True), Yc.to(DEV).requires_grad_(True)
    (sk.compute_Gram_ragged(X, Y, LX, LY) * w.to(DEV)).sum().backward()
    got = (X.grad.cpu(), Y.grad.cpu())
    X, Y = Xc.to(DEV).requires_grad_(True), Yc[:3].to(DEV).requires_grad_(True)
    (sk.compute_kernel_ragged(X, Y, LX, LY[:3]) * wp.to(DEV)).sum().backward()
    gotp = (X.grad.cpu(), Y.grad.cpu())
    worst = max(_worst(got[0].numpy(), want[0].numpy()), _worst(got[1].numpy(), want[1].numpy()),
                _worst(gotp[0].numpy(), wantp[0].numpy()), _worst(gotp[1].numpy(), wantp[1][:3].numpy()))
    print("worst |gradient - CPU autograd| / path max-norm = %.3e" % worst)
    for g, lens in ((got[0], LX), (got[1], LY), (gotp[0], LX), (gotp[1], LY[:3])):
        for i, n in enumerate(lens):
            assert bool((g[i, n:] == 0.0).all()), (i, g[i, n:])
    assert worst <= GRAD_BAR, worst


@pytest.mark.gpu
def test_garbage_padding_gets_exact_zeros_from_the_generic_route():
    """the duck-typed kernel: increments_adjoint + one VJP through the static kernel, on padding full of finite garbage"""
    sk = sigkernel_amd.SigKernel(CubicKernel(), 1, exact_gradient=True)
    Xc, Yc = _paths(True)
    X, Y = (0.1 * Xc).to(DEV).requires_grad_(True), (0.1 * Yc).to(DEV).requires_grad_(True)
    sk.compute_mmd_ragged(X, LX, Y, LY).backward()
    for g, lens in ((X.grad, LX), (Y.grad, LY)):
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
        for i, n in enumerate(lens):
            assert bool((g[i, n:] == 0.0).all()), (i, g[i, n:])


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["gram", "paired"])
def test_fp32_paths_get_fp32_gradients_of_the_up_cast_backward(paired):
    """fp32 paths: the backward runs in fp64 on the up-cast paths and is rounded at the end -- against the fp64 object on the same
    (fp32-representable) paths at the project's fp32 bar, rtol 1e-4 / atol 1e-5"""
    Xc, Yc = _walks(12, 3, 6, 3).float(), _walks(13, 3, 5, 3).float()
    lx, ly = [6, 3, 1], [2, 5, 4]
    grads = []
    for dt in (torch.float32, torch.float64):
        sk = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(0.7), 1, exact_gradient=True)
        X, Y = Xc.detach().clone().to(dt).requires_grad_(True), Yc.detach().clone().to(dt).requires_grad_(True)
        K = sk.compute_kernel_ragged(X, Y, lx, ly) if paired else sk.compute_Gram_ragged(X, Y, lx, ly)
        assert K.dtype == dt
        K.sum().backward()
        assert X.grad.dtype == dt and Y.grad.dtype == dt
        grads.append((X.grad.double().cpu().numpy(), Y.grad.double().cpu().numpy()))
    for a, b in zip(*grads):
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-5)
