"""Prefix kernels with gradients under SigKernel(exact_gradient=True) on the GPU: sk_solve_adj_* with SK_FLAG_DISCRETE | SK_FLAG_SOURCES
(W in/out: a weight per coarse node in, the weighted sum's derivative out) against the restatement (tests/prefix_gradient_reference.py),
the bit identities that tie it to the plain and the ragged discrete adjoint, the C entry point on NaN-filled memory, non-finite and
scaled sources, torch.autograd.gradcheck through every prefix method, and the launch count of a backward."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import sigkernel_amd
from sigkernel_amd import _lib
import prefix_gradient_reference as PR
from poison import same_bits
from test_gpu_ragged_gradient import DEV, GRAD_BAR, GRADCHECK, VALUE_BAR, CubicKernel, _padded, _table, _walks, _worst

# (Mc, Nc, d): one cell, both orientations, fine diagonals longer than 64 lanes (80 and 70 nodes), dyadic orders 0..2
SHAPES = [(1, 1, 0), (9, 5, 1), (5, 9, 1), (40, 3, 1), (3, 70, 0), (7, 6, 2)]
P = 7
NODES = ["all", "diagonal", "last_row", "last_col"]


@functools.lru_cache(maxsize=None)
def _case(shape, naive, f32):
    """(increments (P, Mc, Nc), sources (P, Mc, Nc), final (P,), W (P, Mc, Nc)) of the restatement: computed once"""
    Mc, Nc, d = shape
    rng = np.random.default_rng(7 * Mc + Nc + d)
    inc, S = rng.normal(scale=0.3, size=(P, Mc, Nc)), rng.normal(size=(P, Mc, Nc))
    if f32:
        inc, S = inc.astype(np.float32).astype(np.float64), S.astype(np.float32).astype(np.float64)
    return (inc, S) + PR.source_adjoint_batch(inc, S, d, naive)


def _src(S, dtype=torch.float64):
    return torch.from_numpy(S).to(DEV, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("naive", [False, True], ids=["default", "naive"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_d%d" % s)
def test_source_adjoint_against_the_restatement(shape, naive, dtype):
    """W and the value of solve_adj(discrete=True, sources=S) against the recurrence, 1e-10 x max |W| (fp32 storage: plus half an fp32
    ulp element by element, as tests/test_gpu_ragged_gradient.py does it); the sources handed in are left as they were."""
    Mc, Nc, d = shape
    inc, S, want_k, want_w = _case(shape, naive, dtype == torch.float32)
    be = _lib.HipBackend()
    src = _src(S, dtype)
    keep = src.clone()
    k, W, res = be.solve_adj(_padded(inc, dtype), d, naive, discrete=True, sources=src, return_residual=True)
    assert k.dtype == dtype and W.dtype == dtype and W.shape == (P, Mc, Nc)
    assert same_bits(src, keep)[0]
    Wh, kh = W.double().cpu().numpy(), k.double().cpu().numpy()
    store = 2.0 ** -24 if dtype == torch.float32 else 0.0
    err = np.abs(Wh - want_w)
    print("worst |W - restatement| / max |W| = %.3e" % (err.max() / np.abs(want_w).max()))
    assert np.all(err <= VALUE_BAR * np.abs(want_w).max() + store * np.abs(want_w))
    assert np.all(np.abs(kh - want_k) <= VALUE_BAR * np.abs(want_k) + store * np.abs(want_k))
    assert not res.cpu().numpy().any()


@pytest.mark.gpu
@pytest.mark.parametrize("naive", [False, True], ids=["default", "naive"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_d%d" % s)
def test_one_hot_and_zero_sources_bit_for_bit(shape, naive):
    """fp64.  A one-hot 1.0 at the far corner: W and the value of solve_adj(discrete=True).  A one-hot 1.0 at (mc - 1, nc - 1), the
    entries of the ragged test's table that have no empty side: on [:mc, :nc] the W of solve_adj(discrete=True, cells=...), exactly
    zero elsewhere.  All-zero sources: W == 0 everywhere and the plain value."""
    Mc, Nc, d = shape
    inc = _case(shape, naive, False)[0]
    be = _lib.HipBackend()
    dinc = _padded(inc, torch.float64)
    k0, W0 = be.solve_adj(dinc, d, naive, discrete=True)
    S = torch.zeros(P, Mc, Nc, dtype=torch.float64, device=DEV)
    kz, Wz = be.solve_adj(dinc, d, naive, discrete=True, sources=S)
    assert bool((Wz == 0).all()) and same_bits(kz, k0)[0]
    S[:, -1, -1] = 1.
    k1, W1 = be.solve_adj(dinc, d, naive, discrete=True, sources=S)
    ok, msg = same_bits(W1.contiguous(), W0.contiguous())
    assert ok, msg
    assert same_bits(k1, k0)[0]
    tab = np.array([(mc, nc) for mc, nc in _table(Mc, Nc).tolist() if mc > 0 and nc > 0], dtype=np.int32)
    n = tab.shape[0]
    S = torch.zeros(n, Mc, Nc, dtype=torch.float64, device=DEV)
    for p, (mc, nc) in enumerate(tab.tolist()):
        S[p, mc - 1, nc - 1] = 1.
    sub = dinc[:n]
    _, Wr = be.solve_adj(sub, d, naive, discrete=True, cells=torch.from_numpy(tab).to(DEV))
    k2, W2 = be.solve_adj(sub, d, naive, discrete=True, sources=S)
    assert same_bits(k2, k0[:n])[0]          # the value stays K[MM][NN] of the whole pair
    for p, (mc, nc) in enumerate(tab.tolist()):
        ok, msg = same_bits(W2[p, :mc, :nc].contiguous(), Wr[p, :mc, :nc].contiguous())
        assert ok, (p, msg)
        outside = torch.ones(Mc, Nc, dtype=torch.bool, device=DEV)
        outside[:mc, :nc] = False
        assert bool((W2[p][outside] == 0).all()), p


def _c_entry(lib, buf, ld, S, Mc, Nc, d, naive, slots, ldw, flags):
    """sk_solve_adj_f64 on NaN-filled value vector, residuals, slots and W padding columns, W[..., :Nc] holding the sources"""
    n = S.shape[0]
    slot = int(lib.sk_adj_rescue_slot_bytes(Mc, Nc, d))
    ws = torch.full((slots * slot // 8,), float("nan"), dtype=torch.float64, device=DEV)
    W = torch.full((n, Mc, ldw), float("nan"), dtype=torch.float64, device=DEV)
    W[..., :Nc] = S
    k = torch.full((n,), float("nan"), dtype=torch.float64, device=DEV)
    err = torch.full((n,), float("nan"), dtype=torch.float64, device=DEV)
    rc = lib.sk_solve_adj_f64(buf.data_ptr(), ld, n, Mc, Nc, d, _lib.SCHEME_NAIVE if naive else _lib.SCHEME_DEFAULT, flags, k.data_ptr(),
                              W.data_ptr(), ldw, err.data_ptr(), ws.data_ptr(), ctypes.c_size_t(slots * slot), _lib._stream(buf))
    torch.cuda.synchronize()
    return rc, k, W, err


@pytest.mark.gpu
@pytest.mark.parametrize("naive", [False, True], ids=["default", "naive"])
def test_c_entry_on_poisoned_memory(naive):
    """The C entry point itself: 7 pairs with workspace for only 2 blocks (every slot serves several pairs), odd ld / ldw; slots, value
    vector, residuals, the increments' padding columns and the padding columns Nc..ldw of W full of NaN before the launch, the first
    Nc columns of W holding the sources: the bits of the binding's call, the padding of W untouched.  The flag's argument checks."""
    shape = (9, 5, 1)
    Mc, Nc, d = shape
    ld, ldw = Nc + 3, Nc + 5
    inc, S, _, _ = _case(shape, naive, False)
    lib = _lib.load()
    assert int(lib.sk_version()) == 340
    both = _lib.FLAG_DISCRETE | _lib.FLAG_SOURCES
    assert int(lib.sk_adj_workspace_bytes(P, Mc, Nc, d, both, 8)) == int(lib.sk_adj_workspace_bytes(P, Mc, Nc, d, _lib.FLAG_DISCRETE, 8))
    # the three bad combinations: refused before any launch
    tiny = torch.zeros(1, 1, 1, dtype=torch.float64, device=DEV)
    for flags in (_lib.FLAG_SOURCES, both | _lib.FLAG_RAGGED, both | _lib.FLAG_FAST_ONLY):
        rc = _c_entry(lib, tiny, 1, tiny.clone(), 1, 1, 0, naive, 2, 1, flags)[0]
        assert rc == 1, (flags, rc)          # SK_ERR_BAD_ARG
    buf = torch.full((P, Mc, ld), float("nan"), dtype=torch.float64, device=DEV)
    buf[..., :Nc] = torch.from_numpy(inc).to(DEV)
    src = _src(S)
    kb, Wb = _lib.HipBackend().solve_adj(_padded(inc, torch.float64), d, naive, discrete=True, sources=src)
    rc, k, W, err = _c_entry(lib, buf, ld, src, Mc, Nc, d, naive, 2, ldw, both)
    assert rc == 0, rc
    assert bool(torch.isnan(W[..., Nc:]).all())
    ok, msg = same_bits(W[..., :Nc].contiguous(), Wb.contiguous())
    assert ok, msg
    assert same_bits(k, kb)[0]
    assert not bool(err.any())


@pytest.mark.gpu
def test_a_non_finite_source_stays_in_its_pair_and_powers_of_two_scale_exactly():
    shape = (7, 6, 2)
    Mc, Nc, d = shape
    inc, S, _, _ = _case(shape, False, False)
    be = _lib.HipBackend()
    dinc = _padded(inc, torch.float64)
    _, W0 = be.solve_adj(dinc, d, discrete=True, sources=_src(S))
    assert bool(torch.isfinite(W0).all())
    for bad in (float("nan"), float("inf")):
        Sb = _src(S)
        Sb[3, 2, 4] = bad
        _, W = be.solve_adj(dinc, d, discrete=True, sources=Sb)
        assert not bool(torch.isfinite(W[3]).all())
        others = [p for p in range(P) if p != 3]
        ok, msg = same_bits(W[others].contiguous(), W0[others].contiguous())
        assert ok, (bad, msg)
    for e in (-3, 5):
        _, W = be.solve_adj(dinc, d, discrete=True, sources=_src(S) * 2.0 ** e)
        ok, msg = same_bits(W.contiguous(), (W0 * 2.0 ** e).contiguous())
        assert ok, (e, msg)


def _gradcheck_all(sk, X, Y, Xp, Yp):
    """compute_Gram_prefixes with nodes="all" on (X, Y), every slice mode and the paired and MMD forms on (Xp, Yp) / (Xp, Yp[:len(Xp)])"""
    X, Y, Xp, Yp = (t.clone().requires_grad_(True) for t in (X, Y, Xp, Yp))
    assert torch.autograd.gradcheck(lambda x, y: sk.compute_Gram_prefixes(x, y), (X, Y), **GRADCHECK)
    for nodes in NODES[1:]:
        assert torch.autograd.gradcheck(lambda x, y: sk.compute_Gram_prefixes(x, y, nodes=nodes), (Xp, Yp), **GRADCHECK), nodes
    Xq = torch.cat((Xp, Xp[:1] * 0.5)).detach().requires_grad_(True)        # a batch as long as Yp's
    assert Xq.shape[0] == Yp.shape[0]
    for nodes in NODES:
        assert torch.autograd.gradcheck(lambda x, y: sk.compute_kernel_prefixes(x, y, nodes=nodes), (Xq, Yp), **GRADCHECK), nodes
    assert torch.autograd.gradcheck(lambda x, y: sk.compute_mmd_prefixes(x, y), (Xq, Yp), **GRADCHECK)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,d,naive", [("linear", 0, False), ("linear", 1, False), ("rbf", 0, False), ("rbf", 1, False), ("rbf", 1, True)],
                         ids=["linear_d0", "linear_d1", "rbf_d0", "rbf_d1", "rbf_d1_naive"])
def test_gradcheck(kernel, d, naive):
    """fp64, X and Y together: nodes="all" on X (2, 4, 2), Y (2, 3, 2); the slice modes on X (2, 5, 2), Y (3, 4, 2); the paired form and
    compute_mmd_prefixes on (3, 5, 2) / (3, 4, 2)"""
    k = sigkernel_amd.LinearKernel() if kernel == "linear" else sigkernel_amd.RBFKernel(0.7)
    sk = sigkernel_amd.SigKernel(k, d, _naive_solver=naive, exact_gradient=True)
    _gradcheck_all(sk, _walks(1, 2, 4, 2), _walks(2, 2, 3, 2), _walks(3, 2, 5, 2), _walks(4, 3, 4, 2))


@pytest.mark.gpu
def test_gradcheck_duck_typed_static_kernel():
    sk = sigkernel_amd.SigKernel(CubicKernel(), 1, exact_gradient=True)
    _gradcheck_all(sk, 0.5 * _walks(5, 2, 4, 2), 0.5 * _walks(6, 2, 3, 2), 0.5 * _walks(7, 2, 5, 2), 0.5 * _walks(8, 3, 4, 2))


@pytest.mark.gpu
def test_gradcheck_function_valued_kernel():
    """paths (batch, T, Lx, d) through RBF_ID_Kernel's feature map: the gradient reaches them through torch autograd of the map"""
    sk = sigkernel_amd.SigKernel(sigkernel_amd.RBF_ID_Kernel(0.7), 1, exact_gradient=True)
    _gradcheck_all(sk, _walks(9, 2, 4, 2).reshape(2, 4, 2, 1), _walks(10, 2, 3, 2).reshape(2, 3, 2, 1),
                   _walks(11, 2, 5, 2).reshape(2, 5, 2, 1), _walks(12, 3, 4, 2).reshape(3, 4, 2, 1))


@pytest.mark.gpu
def test_gradcheck_linear_paths_wider_than_the_second_argument_kernel():
    """LinearKernel at dim 9: dL/dY of a Gram block comes from the swapped contraction, with W transposed"""
    sk = sigkernel_amd.SigKernel(sigkernel_amd.LinearKernel(), 1, exact_gradient=True)
    X, Y = (0.5 * _walks(14, 2, 5, 9)).requires_grad_(True), (0.5 * _walks(15, 3, 4, 9)).requires_grad_(True)
    for nodes in ("all", "diagonal"):
        assert torch.autograd.gradcheck(lambda x, y: sk.compute_Gram_prefixes(x, y, nodes=nodes), (X, Y), **GRADCHECK), nodes


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["linear", "rbf"])
def test_the_last_node_gives_the_gradients_of_compute_Gram_bit_for_bit(kernel):
    k = sigkernel_amd.LinearKernel() if kernel == "linear" else sigkernel_amd.RBFKernel(0.7)
    sk = sigkernel_amd.SigKernel(k, 1, exact_gradient=True)
    Xc, Yc = _walks(21, 3, 6, 3), _walks(22, 4, 5, 3)
    grads = []
    for prefixes in (False, True):
        X, Y = Xc.clone().requires_grad_(True), Yc.clone().requires_grad_(True)
        K = sk.compute_Gram_prefixes(X, Y)[..., -1, -1] if prefixes else sk.compute_Gram(X, Y)
        K.sum().backward()
        grads.append((X.grad, Y.grad))
    for a, b in zip(*grads):
        ok, msg = same_bits(a, b)
        assert ok, msg


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["linear", "rbf"])
def test_mmd_prefixes_gradient_is_that_of_compute_mmd_on_the_truncated_paths(kernel):
    k = sigkernel_amd.LinearKernel() if kernel == "linear" else sigkernel_amd.RBFKernel(0.7)
    sk = sigkernel_amd.SigKernel(k, 1, exact_gradient=True)
    Xc, Yc = _walks(23, 4, 6, 3), _walks(24, 3, 5, 3)
    T = 5
    for t in (1, T - 1):
        X, Y = Xc.clone().requires_grad_(True), Yc.clone().requires_grad_(True)
        curve = sk.compute_mmd_prefixes(X, Y)
        assert curve.shape == (T,)
        curve[t].backward()
        X2, Y2 = Xc.clone().requires_grad_(True), Yc.clone().requires_grad_(True)
        one = sk.compute_mmd(X2[:, :t + 1], Y2[:, :t + 1])
        assert abs(float(curve[t].detach()) - float(one.detach())) <= VALUE_BAR * max(abs(float(one.detach())), 1.0)
        one.backward()
        worst = max(_worst(X.grad.cpu().numpy(), X2.grad.cpu().numpy()), _worst(Y.grad.cpu().numpy(), Y2.grad.cpu().numpy()))
        print("t = %d: worst |gradient difference| / path max-norm = %.3e" % (t, worst))
        assert worst <= GRAD_BAR, (t, worst)
        assert bool((X.grad[:, t + 1:] == 0).all()) and bool((Y.grad[:, t + 1:] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("nodes", NODES)
def test_fp32_paths_get_fp32_gradients_of_the_up_cast_backward(nodes):
    """fp32 paths: the backward runs in fp64 on the up-cast paths and is rounded at the end -- against the fp64 object on the same
    (fp32-representable) paths at the project's fp32 bar, rtol 1e-4 / atol 1e-5"""
    Xc, Yc = _walks(12, 3, 6, 3).float(), _walks(13, 2, 5, 3).float()
    grads = []
    for dt in (torch.float32, torch.float64):
        sk = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(0.7), 1, exact_gradient=True)
        X, Y = Xc.detach().clone().to(dt).requires_grad_(True), Yc.detach().clone().to(dt).requires_grad_(True)
        K = sk.compute_Gram_prefixes(X, Y, nodes=nodes)
        assert K.dtype == dt
        w = torch.randn(K.shape, generator=torch.Generator().manual_seed(4), dtype=torch.float64).to(DEV, dt)
        (K * w).sum().backward()
        assert X.grad.dtype == dt and Y.grad.dtype == dt
        grads.append((X.grad.double().cpu().numpy(), Y.grad.double().cpu().numpy()))
    for a, b in zip(*grads):
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-5)


SOLVERS = ("k_adj_", "k_fwd_", "k_deriv_wave", "k_deriv_simple", "k_deriv_fused", "k_fused_rescue", "k_trunc_sig")


def _backward_launches(loss):
    """{solver kernel: launches} of loss.backward()"""
    was = _lib.launch_trace(True)
    try:
        torch.cuda.synchronize()
        _lib.launch_counts(reset=True)
        loss.backward()
        torch.cuda.synchronize()
        counts = _lib.launch_counts(reset=True)
    finally:
        _lib.launch_trace(was)
    return {k: v for k, v in counts.items() if v > 0 and any(s in k for s in SOLVERS)}


@pytest.mark.gpu
@pytest.mark.parametrize("workspace_bytes", [None, 1], ids=["one_tile", "a_tile_per_row"])
@pytest.mark.parametrize("nodes", ["all", "diagonal"])
def test_a_prefix_backward_launches_what_a_compute_Gram_backward_launches(nodes, workspace_bytes):
    """one stored-grid sweep per row tile, as for compute_Gram on the same shapes and budget, and no other solver kernel"""
    sk = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(0.7), 1, exact_gradient=True, workspace_bytes=workspace_bytes)
    Xc, Yc = _walks(31, 3, 6, 3), _walks(32, 4, 6, 3)
    X, Y = Xc.clone().requires_grad_(True), Yc.clone().requires_grad_(True)
    plain = _backward_launches(sk.compute_Gram(X, Y).sum())
    X, Y = Xc.clone().requires_grad_(True), Yc.clone().requires_grad_(True)
    K = sk.compute_Gram_prefixes(X, Y, nodes=nodes)
    w = torch.randn(K.shape, generator=torch.Generator().manual_seed(6), dtype=torch.float64).to(DEV)
    prefix = _backward_launches((K * w).sum())
    assert prefix and all("k_adj_simple" in k for k in prefix), prefix
    assert sum(prefix.values()) == (1 if workspace_bytes is None else 3)
    assert prefix == plain, (prefix, plain)
