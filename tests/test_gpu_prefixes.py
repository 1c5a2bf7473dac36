"""compute_Gram_prefixes / compute_kernel_prefixes on the GPU: the fused prefix kernel (csrc/sk_wave_prefix.hip) and the streamed
fallback against the CPU oracle's full grid, the routes they take (sk_launch_trace), bit-identity of the last node with the fused
forward, and the stores the kernel must not make.

Tolerances are those of tests/test_gpu_parity.py (FAST_TOL for fp64, the reference's own fp32 acceptance for fp32 paths) and of the
streaming route's tests (1e-11)."""
import numpy as np
import pytest
import torch

import sigkernel_amd
from sigkernel_amd import _lib
from oracle import oracle as O
from conftest import rel_err, walk

pytestmark = pytest.mark.gpu

FAST_TOL = 1e-12                    # tests/test_gpu_parity.py
F32_RTOL, F32_ATOL = 1e-4, 1e-5     # tests/test_gpu_parity.py (the reference's own fp32 acceptance)
STREAM_TOL = 1e-11
DEV = "cuda"

SHAPES = [(5, 7, 2, 2, 1), (4, 3, 9, 14, 3), (3, 5, 33, 20, 8), (6, 6, 64, 63, 4), (3, 2, 40, 257, 2), (2, 3, 129, 40, 5)]
KINDS = ["linear", "rbf"]


def _kernel(kind):
    return sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(1.0)


def _oracle_grid(X, Y, kind, dyadic, naive, gram):
    """The oracle's full grid at the coarse nodes: static kernel in torch (fp64, CPU), increments and PDE sweep in the C oracle."""
    k = _kernel(kind)
    Xc, Yc = X.double().cpu(), Y.double().cpu()
    G = (k.Gram_matrix(Xc, Yc) if gram else k.batch_kernel(Xc, Yc)).numpy()
    r = 1 << dyadic
    return O.solve_coarse(O.increments(G), dyadic, naive, want_grid=True)[1][..., ::r, ::r]


def _prefix_launches():
    counts = _lib.launch_counts(reset=True)
    return (sum(v for k, v in counts.items() if "k_fwd_prefix" in k), sum(v for k, v in counts.items() if "k_fwd_simple" in k))


def _is_fused(kind, D, M, N, dyadic, naive, elem_size=8):
    return _lib.HipBackend.route(_lib.OP_PREFIX, 0 if kind == "linear" else 1, D, M, N, dyadic, naive, elem_size) == _lib.ROUTE_FUSED


CASES = [(kind, dyadic, naive, shape) for kind in KINDS for dyadic in (0, 1, 2) for naive in (False, True) for shape in SHAPES]


def test_the_first_five_shapes_are_inside_one_band():
    """A route rule that quietly declines cannot pass through the fallback: at least 60 of the 72 Gram cases must be the fused kernel's."""
    fused = [c for c in CASES if _is_fused(c[0], c[3][4], c[3][2], c[3][3], c[1], c[2])]
    assert len(fused) >= 60, len(fused)
    for kind, dyadic, naive, shape in CASES:
        if shape != SHAPES[-1]:
            assert _is_fused(kind, shape[4], shape[2], shape[3], dyadic, naive), (kind, dyadic, naive, shape)


@pytest.mark.parametrize("kind,dyadic,naive,shape", CASES)
def test_prefix_grids_match_the_oracle_and_take_the_route_the_library_names(kind, dyadic, naive, shape):
    A, B, M, N, D = shape
    gen = torch.Generator().manual_seed(1000 * dyadic + 10 * M + N)
    X, Y = walk(gen, A, M, D).to(DEV), walk(gen, B, N, D).to(DEV)
    sk = sigkernel_amd.SigKernel(_kernel(kind), dyadic, _naive_solver=naive)
    fused = _is_fused(kind, D, M, N, dyadic, naive)
    was = _lib.launch_trace(True)
    try:
        for gram in (True, False):
            Yg = Y if gram else walk(gen, A, N, D).to(DEV)
            _lib.launch_counts(reset=True)
            out = sk.compute_Gram_prefixes(X, Yg) if gram else sk.compute_kernel_prefixes(X, Yg)
            torch.cuda.synchronize()
            n_prefix, n_simple = _prefix_launches()
            assert out.shape == ((A, B, M, N) if gram else (A, M, N)) and out.dtype == X.dtype and out.grad_fn is None
            if fused:
                assert n_prefix >= 1 and n_simple == 0, (n_prefix, n_simple)
            else:
                assert n_prefix == 0 and n_simple >= 1, (n_prefix, n_simple)
            want = _oracle_grid(X, Yg, kind, dyadic, naive, gram)
            err = rel_err(out.cpu().numpy(), want)
            print("%s d=%d naive=%d %s gram=%d fused=%d: rel err %.3e" % (kind, dyadic, naive, shape, gram, fused, err))
            assert err <= FAST_TOL, err      # the whole list, whichever route serves the case
            assert bool((out[..., 0, :] == 1).all()) and bool((out[..., :, 0] == 1).all())
    finally:
        _lib.launch_trace(was)


@pytest.mark.parametrize("naive", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dyadic", [0, 1, 2])
def test_fp32_paths(kind, dyadic, naive):
    for A, B, M, N, D in [(4, 3, 33, 20, 3), (5, 7, 2, 2, 1), (4, 3, 9, 15, 8), (3, 2, 40, 257, 2)]:
        gen = torch.Generator().manual_seed(7)
        X, Y = walk(gen, A, M, D, torch.float32).to(DEV), walk(gen, B, N, D, torch.float32).to(DEV)
        sk = sigkernel_amd.SigKernel(_kernel(kind), dyadic, _naive_solver=naive)
        out = sk.compute_Gram_prefixes(X, Y)
        assert out.dtype == torch.float32
        np.testing.assert_allclose(out.cpu().numpy(), _oracle_grid(X, Y, kind, dyadic, naive, True), rtol=F32_RTOL, atol=F32_ATOL)
        pair = sk.compute_kernel_prefixes(X[:min(A, B)], Y[:min(A, B)])
        np.testing.assert_allclose(pair.cpu().numpy(), _oracle_grid(X[:min(A, B)], Y[:min(A, B)], kind, dyadic, naive, False), rtol=F32_RTOL, atol=F32_ATOL)


@pytest.mark.parametrize("naive", [False, True])
@pytest.mark.parametrize("dyadic", [0, 1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_the_last_node_is_the_fused_forward_bit_for_bit(kind, dyadic, naive):
    be = _lib.get_backend()
    for A, B, M, N, D in [(5, 7, 9, 14, 3), (3, 5, 33, 20, 8), (6, 6, 64, 63, 4), (37, 29, 40, 70, 6)]:
        gen = torch.Generator().manual_seed(M)
        X, Y = walk(gen, A, M, D).to(DEV), walk(gen, B, N, D).to(DEV)
        sk = sigkernel_amd.SigKernel(_kernel(kind), dyadic, _naive_solver=naive)
        assert _is_fused(kind, D, M, N, dyadic, naive)
        grid = sk.compute_Gram_prefixes(X, Y)
        assert torch.equal(grid[..., -1, -1], sk.compute_Gram(X, Y)), (A, B, M, N, D)
        one_band = be.solve_fwd_fused_linear if kind == "linear" else be.solve_fwd_fused_rbf
        assert torch.equal(grid[..., -1, -1], one_band(X, Y, 1.0, dyadic, naive, True))
        Yp = walk(gen, A, N, D).to(DEV)
        assert torch.equal(sk.compute_kernel_prefixes(X, Yp)[..., -1, -1], sk.compute_kernel(X, Yp))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("dyadic", [0, 1, 2])
@pytest.mark.parametrize("kind", KINDS)
# Mc = 1; M - 1 not a multiple of RC; odd and even N.  lead / pad: where a pair's grid starts inside the sentinel array and how far the
# grids are apart -- an odd start or distance allows only one-element stores, an even start and distance (with even N) the two-column
# pieces: both store schemes of the kernel, both output dtypes, both stencils
@pytest.mark.parametrize("M,N,lead,pad,naive", [(2, 7, 11, 37, False), (8, 15, 12, 38, True), (31, 2, 12, 38, False), (12, 33, 11, 37, True),
                                               (9, 20, 12, 38, False), (9, 20, 11, 38, True), (33, 64, 16, 40, True), (6, 10, 12, 37, False)])
def test_no_stray_stores(kind, dyadic, M, N, lead, pad, naive, dtype):
    A, B, D = 3, 5, 3
    gen = torch.Generator().manual_seed(11)
    X, Y = walk(gen, A, M, D, dtype).to(DEV), walk(gen, B, N, D, dtype).to(DEV)
    be = _lib.get_backend()
    k, param = (0, 1.0) if kind == "linear" else (1, 1.0)
    # every pair's grid sits inside a slot with a margin of NaNs before and behind it, the whole array inside a guard band
    slot, guard = M * N + pad, 4096
    for gram in (True, False):
        Yg = Y if gram else Y[:A].contiguous()
        P = A * B if gram else A
        shape, strides = ((A, B, M, N), (B * slot, slot, N, 1)) if gram else ((A, M, N), (slot, N, 1))
        big = torch.full((guard + P * slot + guard,), float("nan"), dtype=dtype, device=DEV)
        view = big[guard + lead:guard + lead + P * slot].as_strided(shape, strides)
        out = be.solve_prefix_fused(k, param, X, Yg, dyadic, naive, gram, out=view)
        torch.cuda.synchronize()
        assert out is not None and out.data_ptr() == view.data_ptr()
        assert not bool(torch.isnan(view).any())
        mask = torch.zeros_like(big, dtype=torch.bool)
        mask[guard + lead:guard + lead + P * slot].as_strided(shape, strides).fill_(True)
        assert bool(torch.isnan(big[~mask]).all())
        assert bool((view[..., 0, :] == 1).all()) and bool((view[..., :, 0] == 1).all())
        want = _oracle_grid(X, Yg, kind, dyadic, naive, gram)
        if dtype == torch.float64:
            assert rel_err(view.cpu().numpy(), want) <= FAST_TOL
        else:
            np.testing.assert_allclose(view.cpu().numpy(), want, rtol=F32_RTOL, atol=F32_ATOL)


@pytest.mark.parametrize("kind", KINDS)
def test_big_batches_draw_from_the_work_queue(kind):
    """Enough pairs to fill the chip (the launch then deals out a first share and draws the rest from its counter), odd batch sizes in
    the shared-y order: every pair's grid lands in its own place."""
    A, B, M, N, D = 301, 203, 17, 12, 2
    gen = torch.Generator().manual_seed(3)
    X, Y = walk(gen, A, M, D).to(DEV), walk(gen, B, N, D).to(DEV)
    sk = sigkernel_amd.SigKernel(_kernel(kind), 1)
    out = sk.compute_Gram_prefixes(X, Y)
    assert rel_err(out.cpu().numpy(), _oracle_grid(X, Y, kind, 1, False, True)) <= FAST_TOL
    assert torch.equal(out[..., -1, -1], sk.compute_Gram(X, Y))
    Yp = walk(gen, 40000, N, D).to(DEV)
    Xp = walk(gen, 40000, M, D).to(DEV)
    outp = sk.compute_kernel_prefixes(Xp, Yp)
    assert rel_err(outp.cpu().numpy(), _oracle_grid(Xp, Yp, kind, 1, False, False)) <= FAST_TOL


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("A,B,M,N,D,dyadic", [(3, 4, 20, 17, 12, 1), (2, 3, 300, 300, 3, 1), (3, 2, 30, 25, 3, 3)])
def test_fallback_on_the_gpu(kind, A, B, M, N, D, dyadic):
    gen = torch.Generator().manual_seed(5)
    X, Y = walk(gen, A, M, D).to(DEV), walk(gen, B, N, D).to(DEV)
    assert not _is_fused(kind, D, M, N, dyadic, False)
    sk = sigkernel_amd.SigKernel(_kernel(kind), dyadic)
    was = _lib.launch_trace(True)
    try:
        _lib.launch_counts(reset=True)
        out = sk.compute_Gram_prefixes(X, Y)
        torch.cuda.synchronize()
        n_prefix, _ = _prefix_launches()
    finally:
        _lib.launch_trace(was)
    assert n_prefix == 0
    assert rel_err(out.cpu().numpy(), _oracle_grid(X, Y, kind, dyadic, False, True)) <= STREAM_TOL
    tiled = sigkernel_amd.SigKernel(_kernel(kind), dyadic, workspace_bytes=1).compute_Gram_prefixes(X, Y)
    assert torch.equal(tiled, out)
    assert rel_err(out[..., -1, -1].cpu().numpy(), sk.compute_Gram(X, Y).cpu().numpy()) <= STREAM_TOL


def test_the_switch_sends_everything_to_the_fallback(monkeypatch):
    gen = torch.Generator().manual_seed(9)
    X, Y = walk(gen, 4, 20, 3).to(DEV), walk(gen, 3, 17, 3).to(DEV)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(1.0), 1)
    fused = sk.compute_Gram_prefixes(X, Y)
    monkeypatch.setattr(sigkernel_amd.routes, "no_fused_prefix", True)
    was = _lib.launch_trace(True)
    try:
        _lib.launch_counts(reset=True)
        streamed = sk.compute_Gram_prefixes(X, Y)
        torch.cuda.synchronize()
        assert _prefix_launches()[0] == 0
    finally:
        _lib.launch_trace(was)
    assert rel_err(fused.cpu().numpy(), streamed.cpu().numpy()) <= STREAM_TOL


def test_requires_grad_raises_on_the_gpu_too():
    gen = torch.Generator().manual_seed(2)
    X, Y = walk(gen, 2, 9, 2).to(DEV).requires_grad_(True), walk(gen, 2, 8, 2).to(DEV)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.LinearKernel(), 0)
    with pytest.raises(NotImplementedError):
        sk.compute_Gram_prefixes(X, Y)
    with torch.no_grad():
        assert sk.compute_kernel_prefixes(X, Y).shape == (2, 9, 8)
