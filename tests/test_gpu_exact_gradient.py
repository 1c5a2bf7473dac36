"""SigKernel(exact_gradient=True) on the GPU: sk_solve_adj_* with SK_FLAG_DISCRETE against the double-loop restatement of the discrete
solver's exact adjoint (tests/exact_gradient_reference.py), torch.autograd.gradcheck through the public methods, and the default
object, which must keep the reference's formula bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import sigkernel_amd
from sigkernel_amd import _lib
from oracle import oracle as O
import exact_gradient_reference as R
from poison import poisoned, same_bits

DEV = "cuda:0"
VALUE_BAR = 1e-10        # the project's value bar, relative to max |W|

# (Mc, Nc, d): both orientations; one-cell rows and columns (dropped terms); 81 nodes on a diagonal (lanes stride past 64); a long second side
SHAPES = [(5, 9, 1), (9, 5, 1), (1, 7, 0), (7, 1, 2), (40, 3, 1), (3, 70, 0)]


def _increments(shape, seed, P=2):
    return np.random.default_rng(seed).normal(scale=0.3, size=(P,) + shape)


def _padded(inc, dtype):
    """the increments on the device in rows padded to whole cache lines, as a view of their first Nc columns"""
    P, Mc, Nc = inc.shape
    ld = _lib._padded_ld(Nc, 8 if dtype == torch.float64 else 4)
    buf = torch.zeros(P, Mc, ld, dtype=dtype, device=DEV)
    buf[..., :Nc] = torch.from_numpy(inc).to(DEV, dtype)
    return buf[..., :Nc]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("naive", [False, True], ids=["default", "naive"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_d%d" % s)
def test_discrete_adjoint_against_the_restatement(shape, naive, dtype):
    """W and the final value of solve_adj(discrete=True) against the recurrence, 1e-10 x max |W|.  fp32 increments: the sweep's state is
    fp64 either way, so the reference runs on the fp32 values up-cast and the bound gains exactly what storing W in fp32 costs -- half
    an fp32 ulp, 2^-24 |W|, element by element."""
    Mc, Nc, d = shape
    inc = _increments((Mc, Nc), 7 * Mc + Nc + d)
    if dtype == torch.float32:
        inc = inc.astype(np.float32).astype(np.float64)
    k, W, res = _lib.HipBackend().solve_adj(_padded(inc, dtype), d, naive, discrete=True, return_residual=True)
    want_k, want_w = R.exact_adjoint_batch(inc, d, naive)
    W, k = W.double().cpu().numpy(), k.double().cpu().numpy()
    store = 2.0 ** -24 if dtype == torch.float32 else 0.0
    err = np.abs(W - want_w)
    print("worst |W - restatement| / max |W| = %.3e" % (err.max() / np.abs(want_w).max()))
    assert np.all(err <= VALUE_BAR * np.abs(want_w).max() + store * np.abs(want_w))
    assert np.all(np.abs(k - want_k) <= VALUE_BAR * np.abs(want_k) + store * np.abs(want_k))
    assert not res.cpu().numpy().any()          # out_err is zero-filled


@pytest.mark.gpu
@pytest.mark.parametrize("naive", [False, True], ids=["default", "naive"])
def test_discrete_adjoint_reuses_its_slots_and_reads_nothing_unwritten(naive):
    """The C entry point itself: 5 pairs with workspace for only 2 blocks (every slot serves several pairs), ld and ldw padded by odd
    amounts, and workspace, W and the value vector full of NaN before the launch -- no result may depend on unwritten memory, the
    padding of W stays untouched, and SK_FLAG_EDGES_GIVEN beside the flag is ignored."""
    Mc, Nc, d, P = 5, 9, 1, 5
    ld, ldw = Nc + 3, Nc + 5
    inc = _increments((Mc, Nc), 11, P)
    buf = torch.full((P, Mc, ld), float("nan"), dtype=torch.float64, device=DEV)
    buf[..., :Nc] = torch.from_numpy(inc).to(DEV)
    lib = _lib.load()
    slot = int(lib.sk_adj_rescue_slot_bytes(Mc, Nc, d))
    assert slot == 16 * ((Mc << d) + 1) * ((Nc << d) + 1)
    assert int(lib.sk_adj_workspace_bytes(P, Mc, Nc, d, _lib.FLAG_DISCRETE, 8)) == P * slot
    want_k, want_w = R.exact_adjoint_batch(inc, d, naive)
    for flags in (_lib.FLAG_DISCRETE, _lib.FLAG_DISCRETE | _lib.FLAG_EDGES_GIVEN):
        ws = torch.full((2 * slot // 8,), float("nan"), dtype=torch.float64, device=DEV)
        W = torch.full((P, Mc, ldw), float("nan"), dtype=torch.float64, device=DEV)
        k = torch.full((P,), float("nan"), dtype=torch.float64, device=DEV)
        err = torch.full((P,), float("nan"), dtype=torch.float64, device=DEV)
        rc = lib.sk_solve_adj_f64(buf.data_ptr(), ld, P, Mc, Nc, d, _lib.SCHEME_NAIVE if naive else _lib.SCHEME_DEFAULT, flags,
                                  k.data_ptr(), W.data_ptr(), ldw, err.data_ptr(), ws.data_ptr(), ctypes.c_size_t(2 * slot),
                                  _lib._stream(buf))
        assert rc == 0, rc
        Wh = W.cpu().numpy()
        assert np.isnan(Wh[..., Nc:]).all()
        assert np.abs(Wh[..., :Nc] - want_w).max() <= VALUE_BAR * np.abs(want_w).max()
        assert np.abs(k.cpu().numpy() - want_k).max() <= VALUE_BAR * np.abs(want_k).max()
        assert not err.cpu().numpy().any()
    # one slot short of one block is refused, and the mode cannot be "fast only"
    args = (buf.data_ptr(), ld, P, Mc, Nc, d, 0)
    tail = (k.data_ptr(), W.data_ptr(), ldw, err.data_ptr(), ws.data_ptr())
    assert lib.sk_solve_adj_f64(*args, _lib.FLAG_DISCRETE, *tail, ctypes.c_size_t(slot - 8), _lib._stream(buf)) != 0
    assert lib.sk_solve_adj_f64(*args, _lib.FLAG_DISCRETE | _lib.FLAG_FAST_ONLY, *tail, ctypes.c_size_t(2 * slot), _lib._stream(buf)) != 0
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_discrete_adjoint_under_poisoned_allocations():
    """Through the binding with every torch.empty of the library filled with 0xFF (NaN) and 0x55 (huge, finite): the bits of a plain call."""
    be = _lib.HipBackend()
    inc = _padded(_increments((6, 5), 3, 7), torch.float64)
    k0, W0 = be.solve_adj(inc, 1, discrete=True)
    for byte in (0xFF, 0x55):
        with poisoned(byte) as p:
            k, W = be.solve_adj(inc, 1, discrete=True)
        assert p.count > 0
        assert same_bits(k0, k)[0] and same_bits(W0.contiguous(), W.contiguous())[0]


@pytest.mark.gpu
def test_without_the_flag_the_stored_grid_adjoint_keeps_its_bits():
    """The default path of the same kernel instance: SK_FLAG_SIMPLE / SK_FLAG_EXACT against oracle.adjoint_coarse at tolerance 0."""
    be = _lib.HipBackend()
    inc = _increments((7, 6), 5, 3)
    for naive in (False, True):
        want_k, want_w = O.adjoint_coarse(inc, 1, naive=naive)
        for flags in (_lib.FLAG_SIMPLE, _lib.FLAG_EXACT):
            k, W = be.solve_adj(_padded(inc, torch.float64), 1, naive, flags=flags)
            assert np.array_equal(W.cpu().numpy(), want_w) and np.array_equal(k.cpu().numpy(), want_k)


class CubicKernel:
    """a duck-typed static kernel (neither LinearKernel nor RBFKernel): k(x, y) = (1 + <x, y> / 2)^3"""

    def batch_kernel(self, X, Y):
        return (1. + 0.5 * torch.bmm(X, Y.transpose(1, 2))) ** 3

    def Gram_matrix(self, X, Y):
        return (1. + 0.5 * torch.matmul(X[:, None], Y[None].transpose(-1, -2))) ** 3


def _walks(seed, *shape):
    gen = torch.Generator().manual_seed(seed)
    return torch.cumsum(0.5 * torch.randn(*shape, generator=gen, dtype=torch.float64), dim=1).to(DEV)


GRADCHECK = dict(eps=1e-6, atol=1e-7, rtol=1e-6)      # the bar of the project's gradcheck tests


def _gradcheck_all(sk, X, Y):
    """compute_kernel and compute_Gram in both arguments, compute_Gram(X, X, sym=True), compute_mmd"""
    X, Y = X.clone().requires_grad_(True), Y.clone().requires_grad_(True)
    Yp = Y[:X.shape[0]].detach().clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x, y: sk.compute_kernel(x, y), (X, Yp), **GRADCHECK)
    assert torch.autograd.gradcheck(lambda x, y: sk.compute_Gram(x, y), (X, Y), **GRADCHECK)
    assert torch.autograd.gradcheck(lambda x: sk.compute_Gram(x, x, sym=True), (X,), **GRADCHECK)
    assert torch.autograd.gradcheck(lambda x, y: sk.compute_mmd(x, y), (X, Y), **GRADCHECK)


@pytest.mark.gpu
@pytest.mark.parametrize("naive", [False, True], ids=["default", "naive"])
@pytest.mark.parametrize("d", [0, 1])
@pytest.mark.parametrize("kernel", ["linear", "rbf"])
def test_gradcheck(kernel, d, naive):
    """A = 2, B = 3, M = 4, N = 5, D = 2, fp64"""
    k = sigkernel_amd.LinearKernel() if kernel == "linear" else sigkernel_amd.RBFKernel(0.7)
    sk = sigkernel_amd.SigKernel(k, d, _naive_solver=naive, exact_gradient=True)
    _gradcheck_all(sk, _walks(1, 2, 4, 2), _walks(2, 3, 5, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,d", [("linear", 1), ("rbf", 0)])
def test_gradcheck_of_the_other_losses(kernel, d):
    """compute_distance and the scoring rules are compositions in this mode and take a second input that requires grad"""
    k = sigkernel_amd.LinearKernel() if kernel == "linear" else sigkernel_amd.RBFKernel(0.7)
    sk = sigkernel_amd.SigKernel(k, d, exact_gradient=True)
    X, Y = _walks(1, 2, 4, 2).requires_grad_(True), _walks(2, 3, 5, 2).requires_grad_(True)
    Xp = _walks(7, 3, 5, 2).requires_grad_(True)          # compute_distance's merged route would take equal shapes: it must decline
    assert torch.autograd.gradcheck(lambda x, y: sk.compute_distance(x, y), (Xp, Y), **GRADCHECK)
    assert torch.autograd.gradcheck(lambda x, y: sk.compute_expected_scoring_rule(x, y), (X, Y), **GRADCHECK)
    assert torch.autograd.gradcheck(lambda x, y: sk.compute_scoring_rule(x, y[:1]), (X, Y), **GRADCHECK)


@pytest.mark.gpu
def test_gradcheck_linear_paths_wider_than_the_second_argument_kernel():
    """LinearKernel at dim 9: sk_static_adjoint2 has no kernel there, dL/dY of a Gram block comes from the swapped contraction"""
    sk = sigkernel_amd.SigKernel(sigkernel_amd.LinearKernel(), 1, exact_gradient=True)
    X, Y = (0.5 * _walks(14, 2, 4, 9)).requires_grad_(True), (0.5 * _walks(15, 3, 5, 9)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x, y: sk.compute_Gram(x, y), (X, Y), **GRADCHECK)


@pytest.mark.gpu
def test_gradcheck_duck_typed_static_kernel():
    sk = sigkernel_amd.SigKernel(CubicKernel(), 1, exact_gradient=True)
    _gradcheck_all(sk, 0.5 * _walks(3, 2, 4, 2), 0.5 * _walks(4, 3, 5, 2))


@pytest.mark.gpu
def test_gradcheck_function_valued_kernel():
    """paths (batch, T, Lx, d) through RBF_ID_Kernel's feature map: the gradient reaches them through torch autograd of the map"""
    sk = sigkernel_amd.SigKernel(sigkernel_amd.RBF_ID_Kernel(0.7), 1, exact_gradient=True)
    X = _walks(5, 2, 4, 2).reshape(2, 4, 2, 1)
    Y = _walks(6, 3, 5, 2).reshape(3, 5, 2, 1)
    _gradcheck_all(sk, X, Y)


@pytest.mark.gpu
@pytest.mark.parametrize("naive", [False, True], ids=["default", "naive"])
@pytest.mark.parametrize("d", [0, 1, 2])
def test_default_and_exact_objects_on_the_host_tests_inputs(d, naive):
    """setup_paths (tests/test_exact_gradient_host.py proves the reference formula is > 10 % off there): the default object still
    returns the reference formula's X.grad and no Y.grad; the exact object returns the gradient of the computed matrix for both."""
    Xc, Yc, w = R.setup_paths()
    k = sigkernel_amd.LinearKernel()
    grads = {}
    for exact in (False, True):
        sk = sigkernel_amd.SigKernel(k, d, _naive_solver=naive, exact_gradient=exact)
        X, Y = Xc.to(DEV).requires_grad_(True), Yc.to(DEV).requires_grad_(exact)
        (sk.compute_Gram(X, Y) * w.to(DEV)).sum().backward()
        grads[exact] = (X.grad.cpu().numpy(), None if Y.grad is None else Y.grad.cpu().numpy())
    ref = O.gram_grad_weighted(Xc, Yc, w.numpy(), k, d, naive=naive)
    assert np.abs(grads[False][0] - ref).max() <= 1e-9 * np.abs(ref).max()
    assert grads[False][1] is None
    Xg, Yg = Xc.clone().requires_grad_(True), Yc.clone().requires_grad_(True)
    wx, wy = torch.autograd.grad((R.gram_torch(Xg, Yg, k, d, naive) * w).sum(), (Xg, Yg))
    wx, wy = wx.numpy(), wy.numpy()
    assert np.linalg.norm(grads[False][0] - grads[True][0]) > 0.10 * np.linalg.norm(grads[True][0])
    assert np.abs(grads[True][0] - wx).max() <= 1e-9 * np.abs(wx).max()
    assert np.abs(grads[True][1] - wy).max() <= 1e-9 * np.abs(wy).max()


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["gram", "paired"])
def test_fp32_paths_get_fp32_gradients_of_the_up_cast_backward(paired):
    """fp32 paths: the backward runs in fp64 on the up-cast paths and is rounded at the end -- against the fp64 object on the same
    (fp32-representable) paths at the project's fp32 bar, rtol 1e-4 / atol 1e-5"""
    Xc, Yc = _walks(12, 3, 6, 3).float(), _walks(13, 3, 5, 3).float()
    grads = []
    for dt in (torch.float32, torch.float64):
        sk = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(0.7), 1, exact_gradient=True)
        X, Y = Xc.detach().clone().to(dt).requires_grad_(True), Yc.detach().clone().to(dt).requires_grad_(True)
        K = sk.compute_kernel(X, Y) if paired else sk.compute_Gram(X, Y)
        assert K.dtype == dt
        K.sum().backward()
        assert X.grad.dtype == dt and Y.grad.dtype == dt
        grads.append((X.grad.double().cpu().numpy(), Y.grad.double().cpu().numpy()))
    for a, b in zip(*grads):
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["rbf", "cubic"])
def test_tiled_backward_equals_the_untiled_one(kernel, monkeypatch):
    """12 x 10 pairs with a workspace that holds 4 rows of a tile: at least 3 row tiles, the same gradients to 1e-12"""
    k = sigkernel_amd.RBFKernel(0.7) if kernel == "rbf" else CubicKernel()
    Xc, Yc = 0.5 * _walks(8, 12, 6, 2), 0.5 * _walks(9, 10, 6, 2)
    w = torch.randn(12, 10, generator=torch.Generator().manual_seed(10), dtype=torch.float64).to(DEV)
    calls = []
    real = _lib.HipBackend.solve_adj

    def counted(self, *a, **kw):
        calls.append(kw.get("discrete", False))
        return real(self, *a, **kw)
    monkeypatch.setattr(_lib.HipBackend, "solve_adj", counted)
    out = []
    for ws in (None, 2 * 4 * (3 if kernel == "rbf" else 8) * 10 * 6 * 6 * 8):
        del calls[:]
        sk = sigkernel_amd.SigKernel(k, 1, workspace_bytes=ws, exact_gradient=True)
        X, Y = Xc.clone().requires_grad_(True), Yc.clone().requires_grad_(True)
        (sk.compute_Gram(X, Y) * w).sum().backward()
        out.append((X.grad, Y.grad, len(calls)))
        assert all(calls)
    assert out[0][2] == 1 and out[1][2] >= 3, (out[0][2], out[1][2])
    for a, b in zip(out[0][:2], out[1][:2]):
        assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max())
