"""Slices of the prefix grid on the GPU: nodes="diagonal" | "last_row" | "last_col" of compute_Gram_prefixes / compute_kernel_prefixes
and compute_mmd_prefixes.

Inside the fused scope the slice is a store mode of k_fwd_prefix (csrc/sk_wave_prefix.hip): the same sweep, so every element is
bit for bit the node nodes="all" holds there (torch.equal), from exactly the kernel instance the full grid launches (sk_launch_trace).
Outside it the slice is taken from each row tile's streamed grid: the tolerance of tests/test_gpu_prefixes.py's streamed route.  The
memory bound is a condition: a slice call must not allocate anything of the full grid's size."""
import pytest
import torch

import sigkernel_amd
from sigkernel_amd import _lib
from conftest import rel_err, walk

pytestmark = pytest.mark.gpu

STREAM_TOL = 1e-11                  # tests/test_gpu_prefixes.py
DEV = "cuda"
NODES = ["diagonal", "last_row", "last_col"]
KINDS = ["linear", "rbf"]


def _kernel(kind):
    return sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(1.0)


def _slice_of(grid, nodes):
    if nodes == "diagonal":
        return torch.diagonal(grid, dim1=-2, dim2=-1)
    return grid[..., -1, :] if nodes == "last_row" else grid[..., :, -1]


def _length(nodes, M, N):
    return {"diagonal": min(M, N), "last_row": N, "last_col": M}[nodes]


def _is_fused(kind, D, M, N, dyadic, naive=False, elem_size=8):
    return _lib.HipBackend.route(_lib.OP_PREFIX, 0 if kind == "linear" else 1, D, M, N, dyadic, naive, elem_size) == _lib.ROUTE_FUSED


def _traced(f):
    """f() with the launch trace on -> (result, {k_fwd_prefix instance: launches}, launches of the streaming solver)"""
    was = _lib.launch_trace(True)
    try:
        _lib.launch_counts(reset=True)
        out = f()
        torch.cuda.synchronize()
        counts = _lib.launch_counts(reset=True)
    finally:
        _lib.launch_trace(was)
    return out, {k: v for k, v in counts.items() if "k_fwd_prefix" in k and v > 0}, sum(v for k, v in counts.items() if "k_fwd_simple" in k)


# (A, B, M, N, D): M < N, M == N, M > N; odd and even N; M - 1 not a multiple of the rows per lane (4 / 2 / 1); batches that leave
# stream positions of the shared-y order without a pair (A not a multiple of the lane groups per wave)
SHAPES = [(3, 5, 9, 14, 3), (5, 3, 33, 20, 8), (6, 6, 64, 63, 4), (2, 3, 40, 257, 2), (7, 2, 2, 2, 1), (3, 4, 31, 31, 5), (1, 1, 12, 7, 2)]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("naive", [False, True])
@pytest.mark.parametrize("dyadic", [0, 1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_slices_are_the_full_grids_nodes_bit_for_bit_from_the_same_instance(kind, dyadic, naive, dtype):
    sk = sigkernel_amd.SigKernel(_kernel(kind), dyadic, _naive_solver=naive)
    for A, B, M, N, D in SHAPES:
        assert _is_fused(kind, D, M, N, dyadic, naive, 8 if dtype == torch.float64 else 4)
        gen = torch.Generator().manual_seed(100 * M + N)
        X, Y = walk(gen, A, M, D, dtype).to(DEV), walk(gen, B, N, D, dtype).to(DEV)
        Yp = walk(gen, A, N, D, dtype).to(DEV)
        for gram in (True, False):
            Yg = Y if gram else Yp
            call = sk.compute_Gram_prefixes if gram else sk.compute_kernel_prefixes
            grid, inst_all, simple_all = _traced(lambda: call(X, Yg))
            assert len(inst_all) == 1 and simple_all == 0, (inst_all, simple_all)
            for nodes in NODES:
                out, inst, simple = _traced(lambda: call(X, Yg, nodes=nodes))
                where = (kind, dyadic, naive, dtype, (A, B, M, N, D), gram, nodes)
                assert out.shape == ((A, B) if gram else (A,)) + (_length(nodes, M, N),) and out.dtype == dtype and out.grad_fn is None, where
                assert set(inst) == set(inst_all) and simple == 0, (where, inst, inst_all, simple)
                want = _slice_of(grid, nodes)
                assert torch.equal(out, want), (where, float((out.double() - want.double()).abs().max()))
                assert bool((out[..., 0] == 1).all()), where
            last = sk.compute_Gram(X, Yg) if gram else sk.compute_kernel(X, Yg)
            assert torch.equal(call(X, Yg, nodes="last_row")[..., -1], last) and torch.equal(call(X, Yg, nodes="last_col")[..., -1], last)


@pytest.mark.parametrize("nodes", NODES)
@pytest.mark.parametrize("kind", KINDS)
def test_big_batches_draw_from_the_work_queue(kind, nodes):
    """Enough pairs to fill the chip (a first share dealt out, the rest drawn from the counter), odd batch sizes in the shared-y order:
    every pair's slice lands in its own place."""
    A, B, M, N, D = 301, 203, 17, 12, 2
    gen = torch.Generator().manual_seed(3)
    X, Y = walk(gen, A, M, D).to(DEV), walk(gen, B, N, D).to(DEV)
    sk = sigkernel_amd.SigKernel(_kernel(kind), 1)
    assert torch.equal(sk.compute_Gram_prefixes(X, Y, nodes=nodes), _slice_of(sk.compute_Gram_prefixes(X, Y), nodes))
    Xp, Yp = walk(gen, 40000, M, D).to(DEV), walk(gen, 40000, N, D).to(DEV)
    assert torch.equal(sk.compute_kernel_prefixes(Xp, Yp, nodes=nodes), _slice_of(sk.compute_kernel_prefixes(Xp, Yp), nodes))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("nodes", NODES)
@pytest.mark.parametrize("kind", KINDS)
def test_no_stray_stores(kind, nodes, dtype):
    """Every pair's slice inside a slot with NaNs around it, the array inside a guard band: the kernel writes the slice's elements
    1 .. L - 1 of every pair and nothing else (element 0 is the host's fill)."""
    be = _lib.get_backend()
    k, param = (0, 1.0) if kind == "linear" else (1, 1.0)
    for dyadic, (A, B, M, N, D) in [(0, (3, 5, 9, 14, 3)), (1, (3, 5, 12, 33, 3)), (2, (5, 3, 31, 2, 3)), (1, (3, 5, 2, 7, 3))]:
        gen = torch.Generator().manual_seed(11)
        X, Y = walk(gen, A, M, D, dtype).to(DEV), walk(gen, B, N, D, dtype).to(DEV)
        L = _length(nodes, M, N)
        slot, guard, lead = L + 5, 4096, 3
        for gram in (True, False):
            Yg = Y if gram else walk(gen, A, N, D, dtype).to(DEV)
            P = A * B if gram else A
            shape, strides = ((A, B, L), (B * slot, slot, 1)) if gram else ((A, L), (slot, 1))
            big = torch.full((guard + P * slot + guard,), float("nan"), dtype=dtype, device=DEV)
            view = big[guard + lead:guard + lead + P * slot].as_strided(shape, strides)
            out = be.solve_prefix_fused(k, param, X, Yg, dyadic, False, gram, out=view, nodes=nodes)
            torch.cuda.synchronize()
            assert out is not None and out.data_ptr() == view.data_ptr()
            assert not bool(torch.isnan(view).any())
            mask = torch.zeros_like(big, dtype=torch.bool)
            mask[guard + lead:guard + lead + P * slot].as_strided(shape, strides).fill_(True)
            assert bool(torch.isnan(big[~mask]).all())
            assert torch.equal(view, _slice_of(be.solve_prefix_fused(k, param, X, Yg, dyadic, False, gram), nodes))


@pytest.mark.parametrize("nodes", NODES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("A,B,M,N,D,dyadic", [(3, 4, 20, 17, 12, 1),      # dim 12
                                              (3, 2, 30, 25, 3, 3),       # dyadic 3
                                              (2, 3, 300, 290, 3, 1)])    # rows over one band
def test_outside_the_fused_scope_the_slice_comes_from_the_tiled_route(kind, nodes, A, B, M, N, D, dyadic):
    gen = torch.Generator().manual_seed(5)
    X, Y = walk(gen, A, M, D).to(DEV), walk(gen, B, N, D).to(DEV)
    assert not _is_fused(kind, D, M, N, dyadic)
    sk = sigkernel_amd.SigKernel(_kernel(kind), dyadic)
    out, inst, simple = _traced(lambda: sk.compute_Gram_prefixes(X, Y, nodes=nodes))
    assert not inst and simple >= 1, (inst, simple)
    assert out.shape == (A, B, _length(nodes, M, N))
    want = _slice_of(sk.compute_Gram_prefixes(X, Y), nodes)
    err = rel_err(out.cpu().numpy(), want.cpu().numpy())
    print("%s %s %s d=%d: rel err %.3e" % (kind, nodes, (A, B, M, N, D), dyadic, err))
    assert err <= STREAM_TOL, err
    assert bool((out[..., 0] == 1).all())
    tiled = sigkernel_amd.SigKernel(_kernel(kind), dyadic, workspace_bytes=1).compute_Gram_prefixes(X, Y, nodes=nodes)
    assert torch.equal(tiled, out)
    pair = sk.compute_kernel_prefixes(X[:2], Y[:2], nodes=nodes)
    assert rel_err(pair.cpu().numpy(), _slice_of(sk.compute_kernel_prefixes(X[:2], Y[:2]), nodes).cpu().numpy()) <= STREAM_TOL


def _peak_over(f):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = f()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - before


def test_a_diagonal_call_allocates_nothing_of_the_grids_size():
    """256 x 256 pairs of 128 points, dim 8, fp64: the full grid would be 8.6 GB; the diagonal is 67 MB and the staged inputs are
    under 10 MB.  The peak of allocated memory rises by less than 1 GB over the call."""
    gen = torch.Generator().manual_seed(1)
    X, Y = walk(gen, 256, 128, 8).to(DEV), walk(gen, 256, 128, 8).to(DEV)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(1.0), 1)
    assert _is_fused("rbf", 8, 128, 128, 1)
    out, rise = _peak_over(lambda: sk.compute_Gram_prefixes(X, Y, nodes="diagonal"))
    print("diagonal of 256 x 256 pairs of 128 points: peak allocated memory rose by %.1f MB" % (rise / 1e6))
    assert out.shape == (256, 256, 128)
    assert rise < 1e9, rise
    assert torch.equal(out[..., -1], sk.compute_Gram(X, Y)) and bool((out[..., 0] == 1).all())
    # a few pairs against the full grid of those pairs
    assert torch.equal(out[:3, :5], _slice_of(sk.compute_Gram_prefixes(X[:3], Y[:5]), "diagonal"))


def test_mmd_prefixes_on_the_gpu_within_the_same_memory_bound():
    """256 + 256 paths of 128 points: three diagonal sweeps and their reductions, under 1 GB; the values are compute_mmd's on the
    truncated samples (three means of Gram matrices that agree to 1e-12 of their largest entry, one of them twice: 4e-12 of it)."""
    gen = torch.Generator().manual_seed(2)
    X, Y = walk(gen, 256, 128, 8).to(DEV), 1.2 * walk(gen, 256, 128, 8).to(DEV)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(1.0), 1)
    out, rise = _peak_over(lambda: sk.compute_mmd_prefixes(X, Y))
    print("compute_mmd_prefixes at 256 + 256 paths of 128 points: peak allocated memory rose by %.1f MB" % (rise / 1e6))
    assert out.shape == (128,) and out.grad_fn is None and float(out[0]) == 0.0
    assert rise < 1e9, rise
    for t in (1, 2, 17, 64, 127):
        Xt, Yt = X[:, :t + 1].contiguous(), Y[:, :t + 1].contiguous()
        want = float(sk.compute_mmd(Xt, Yt))
        kmax = max(float(sk.compute_Gram(Z, W).abs().max()) for Z, W in ((Xt, Xt), (Yt, Yt), (Xt, Yt)))
        print("t = %d: mmd %.12e, compute_mmd %.12e, bound %.3e" % (t, float(out[t]), want, 4e-12 * kmax))
        assert abs(float(out[t]) - want) <= 4e-12 * kmax, (t, float(out[t]), want)
    with pytest.raises(NotImplementedError):
        sk.compute_mmd_prefixes(X.clone().requires_grad_(True), Y)
