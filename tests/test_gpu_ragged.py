"""compute_Gram_ragged / compute_kernel_ragged / compute_mmd_ragged on the GPU: store mode SK_NODES_AT of k_fwd_prefix -- ONE launch per
call, one node per pair.  The claim is bit-equality with node (len_x - 1, len_y - 1) of compute_Gram_prefixes' grid at the same padded
shape (the same sweep, another store); closeness to the CPU oracle on the TRUNCATED paths at the bar of tests/test_gpu_prefixes.py.
Lengths are aimed at every row k < RC of the first lane and of the last lane of a pair, at the first and the second node column of a
macro-step, and include 1, 2 and the padded length in every batch."""
import numpy as np
import pytest
import torch

import sigkernel_amd
from sigkernel_amd import _lib
from oracle import oracle as O
from conftest import rel_err, walk

pytestmark = pytest.mark.gpu
FAST_TOL = 1e-12                    # tests/test_gpu_prefixes.py
F32_RTOL, F32_ATOL = 1e-4, 1e-5     # tests/test_gpu_prefixes.py (the reference's own fp32 acceptance)
STREAM_TOL = 1e-11                  # tests/test_gpu_prefixes.py: the streamed fallback
DEV = "cuda"
KD = [("linear", 0), ("rbf", 0), ("linear", 1), ("rbf", 1), ("linear", 2), ("rbf", 2)]      # RC 4, 2, 2, 2, 1, 1: all four instances
LARGEST = {("linear", 0): 257, ("rbf", 0): 128, ("linear", 1): 129, ("rbf", 1): 128, ("linear", 2): 65, ("rbf", 2): 64}


def _kernel(kind):
    return sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(1.0)


def _is_fused(kind, D, M, N, dyadic, naive, elem_size=8):
    return _lib.HipBackend.route(_lib.OP_PREFIX, 0 if kind == "linear" else 1, D, M, N, dyadic, naive, elem_size) == _lib.ROUTE_FUSED


def _lens(seed, count, top):
    """`count` lengths in [1, top]: 1, 2 and top first, then the rows k < 4 of the first lane (3, 4, 5), the rows of the last lane (top - 1
    .. top - 3), both parities everywhere -- first and second node column of a macro-step -- and random ones"""
    aimed = [1, 2, top, 3, top - 1, 4, top - 2, 5, top - 3]
    if count < 3:          # a batch of one or two: a node must be stored and compared, so the padded length comes first
        aimed = [top, 2, 1]
    aimed = [v for i, v in enumerate(aimed) if 1 <= v <= top and v not in aimed[:i]]
    g = np.random.default_rng(seed)
    lens = (aimed + g.integers(1, top + 1, size=max(0, count - len(aimed))).tolist())[:count]
    return [int(v) for v in g.permutation(lens)]


def _oracle_at(X, Y, lx, ly, kind, dyadic, naive, gram):
    """the oracle on the truncated paths x[:lx], y[:ly], one call per distinct pair of lengths; a one-point path: exactly 1"""
    k = _kernel(kind)
    Xc, Yc = X.double().cpu(), Y.double().cpu()
    lx, ly = np.asarray(lx), np.asarray(ly)
    out = np.ones((len(lx), len(ly)) if gram else (len(lx),))
    if gram:
        for m in sorted(set(lx.tolist()) - {1}):
            for n in sorted(set(ly.tolist()) - {1}):
                ia, ib = np.nonzero(lx == m)[0], np.nonzero(ly == n)[0]
                out[np.ix_(ia, ib)] = O.gram_forward(Xc[ia, :m], Yc[ib, :n], k, dyadic, naive)
    else:
        for m, n in sorted(set(zip(lx.tolist(), ly.tolist()))):
            if m > 1 and n > 1:
                i = np.nonzero((lx == m) & (ly == n))[0]
                G = k.batch_kernel(Xc[i, :m], Yc[i, :n]).numpy()
                out[i] = O.solve_coarse(O.increments(G), dyadic, naive)
    return out


def _traced(f):
    """f() under the launch trace: (result, launches of k_fwd_prefix, launches of the streamed pieces)"""
    was = _lib.launch_trace(True)
    try:
        _lib.launch_counts(reset=True)
        out = f()
        torch.cuda.synchronize()
        counts = _lib.launch_counts(reset=True)
    finally:
        _lib.launch_trace(was)
    streamed = ("k_fwd_wave", "k_fwd_simple", "k_solve", "k_static", "k_increments")
    return (out, sum(v for k, v in counts.items() if "k_fwd_prefix" in k),
            sum(v for k, v in counts.items() if any(s in k for s in streamed)))


def _gather(grid, lx, ly, gram):
    ia, ib = torch.tensor(lx, device=grid.device) - 1, torch.tensor(ly, device=grid.device) - 1
    if gram:
        A, B = grid.shape[:2]
        return grid[torch.arange(A, device=grid.device)[:, None], torch.arange(B, device=grid.device)[None, :], ia[:, None], ib[None, :]]
    return grid[torch.arange(grid.shape[0], device=grid.device), ia, ib]


def _check(kind, dyadic, naive, dtype, A, B, M, N, D, gram, seed=0):
    gen = torch.Generator().manual_seed(1000 * dyadic + 10 * M + N + seed)
    X, Y = walk(gen, A, M, D, dtype).to(DEV), walk(gen, B if gram else A, N, D, dtype).to(DEV)
    lx, ly = _lens(seed + M, A, M), _lens(seed + N + 1, B if gram else A, N)
    sk = sigkernel_amd.SigKernel(_kernel(kind), dyadic, _naive_solver=naive)
    call = (lambda: sk.compute_Gram_ragged(X, Y, lx, ly)) if gram else (lambda: sk.compute_kernel_ragged(X, Y, lx, ly))
    K, n_prefix, n_streamed = _traced(call)
    assert K.shape == ((A, B) if gram else (A,)) and K.dtype == dtype and K.grad_fn is None
    fused = _is_fused(kind, D, M, N, dyadic, naive, X.element_size())
    if fused:
        assert n_prefix == 1 and n_streamed == 0, (n_prefix, n_streamed)
    else:
        assert n_prefix == 0 and n_streamed >= 1, (n_prefix, n_streamed)
    grid = sk.compute_Gram_prefixes(X, Y) if gram else sk.compute_kernel_prefixes(X, Y)
    assert torch.equal(K, _gather(grid, lx, ly, gram)), "not the grid's node bit for bit"
    del grid
    want = _oracle_at(X, Y, lx, ly, kind, dyadic, naive, gram)
    if dtype == torch.float64:
        err = rel_err(K.cpu().numpy(), want)
        print("%s d=%d naive=%d %s (%d, %d) x (%d, %d) dim %d gram=%d fused=%d: rel err %.3e" % (kind, dyadic, naive, dtype, A, B, M, N, D, gram, fused, err))
        assert err <= (FAST_TOL if fused else STREAM_TOL), err
    else:
        np.testing.assert_allclose(K.cpu().numpy(), want, rtol=F32_RTOL, atol=F32_ATOL)
    ones = torch.tensor([v == 1 for v in lx], device=DEV)
    assert bool((K[ones] == 1).all())
    assert torch.equal(K, call())          # repeated calls: bit-identical
    # the padding is irrelevant: other finite values behind every path's end
    X2, Y2 = X.clone(), Y.clone()
    for i, n in enumerate(lx):
        X2[i, n:] = 1e3
    for i, n in enumerate(ly):
        Y2[i, n:] = -7.0
    assert torch.equal(K, sk.compute_Gram_ragged(X2, Y2, lx, ly) if gram else sk.compute_kernel_ragged(X2, Y2, lx, ly))
    return fused


SHAPES = [(3, 2), (6, 5), (9, 8), (34, 17), (65, 33)]


@pytest.mark.parametrize("i,MN", list(enumerate(SHAPES + ["largest"])))
@pytest.mark.parametrize("kind,dyadic", KD)
def test_every_instance_stores_the_grids_node(kind, dyadic, i, MN):
    """padded shapes with odd and even N and the largest one-band length of the instance; the stencil, the output dtype and the path
    dimension (1, 3, 8) rotate over the cases so that every instance meets both stencils, both dtypes and all three dimensions"""
    M, N = (LARGEST[(kind, dyadic)], 20 + (dyadic & 1)) if MN == "largest" else MN
    j = i + dyadic + (kind == "rbf")
    naive, dtype, D = bool(j & 1), (torch.float64, torch.float32)[(j >> 1) & 1], (1, 3, 8)[j % 3]
    fused = _check(kind, dyadic, naive, dtype, 5, 7, M, N, D, True)
    assert fused or (M, N) == (65, 33)      # (65 points: beyond one band for rbf at dyadic 2 alone)
    _check(kind, dyadic, not naive, torch.float64 if dtype == torch.float32 else torch.float32, 9, 9, M, N, D, False, seed=1)


@pytest.mark.parametrize("A,B", [(1, 1), (3, 4), (5, 7), (40, 3), (130, 33)])
@pytest.mark.parametrize("kind,dyadic", KD)
def test_batches_with_idle_lane_groups(kind, dyadic, A, B):
    """short pairs put several lane groups into a wave; batch sizes that leave some of them idle under the shared-y order"""
    assert _check(kind, dyadic, False, torch.float64, A, B, 9, 8, 3, True, seed=A)
    assert _check(kind, dyadic, True, torch.float64, A, B, 34, 17, 8, True, seed=B)


@pytest.mark.parametrize("n", [1, 9, 300])
@pytest.mark.parametrize("kind,dyadic", KD)
def test_paired_batches(kind, dyadic, n):
    assert _check(kind, dyadic, False, torch.float64, n, n, 9, 8, 3, False, seed=n)
    assert _check(kind, dyadic, True, torch.float32, n, n, 34, 17, 1, False, seed=n + 1)


@pytest.mark.parametrize("kind", ["linear", "rbf"])
def test_big_batches_draw_from_the_work_queue(kind):
    """enough pairs that the launch draws from its counter (the sizes of tests/test_gpu_prefixes.py), odd batch sizes in the shared-y order"""
    assert _check(kind, 1, False, torch.float64, 301, 203, 17, 12, 2, True)
    assert _check(kind, 1, False, torch.float64, 40000, 40000, 17, 12, 2, False)


@pytest.mark.parametrize("kind,dyadic,M,N,D", [("linear", 1, 20, 17, 9), ("rbf", 1, 30, 25, 12), ("linear", 1, 140, 7, 3), ("rbf", 2, 70, 9, 3)])
def test_outside_the_fused_scope_the_fallback_holds(kind, dyadic, M, N, D):
    """dim 9 and more; two bands: the tiled route, the same values"""
    assert not _is_fused(kind, D, M, N, dyadic, False)
    assert not _check(kind, dyadic, False, torch.float64, 3, 4, M, N, D, True)
    assert not _check(kind, dyadic, False, torch.float64, 5, 5, M, N, D, False)
    # tiled by a tiny workspace: the same bits
    gen = torch.Generator().manual_seed(M)
    X, Y = walk(gen, 3, M, D).to(DEV), walk(gen, 4, N, D).to(DEV)
    lx, ly = _lens(1, 3, M), _lens(2, 4, N)
    big = sigkernel_amd.SigKernel(_kernel(kind), dyadic).compute_Gram_ragged(X, Y, lx, ly)
    assert torch.equal(big, sigkernel_amd.SigKernel(_kernel(kind), dyadic, workspace_bytes=1).compute_Gram_ragged(X, Y, lx, ly))


def test_the_switch_sends_everything_to_the_fallback(monkeypatch):
    gen = torch.Generator().manual_seed(9)
    X, Y = walk(gen, 4, 20, 3).to(DEV), walk(gen, 3, 17, 3).to(DEV)
    lx, ly = _lens(3, 4, 20), _lens(4, 3, 17)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(1.0), 1)
    fused, n_prefix, _ = _traced(lambda: sk.compute_Gram_ragged(X, Y, lx, ly))
    assert n_prefix == 1
    monkeypatch.setattr(sigkernel_amd.routes, "no_fused_prefix", True)
    streamed, n_prefix, n_streamed = _traced(lambda: sk.compute_Gram_ragged(X, Y, lx, ly))
    assert n_prefix == 0 and n_streamed >= 1
    assert rel_err(fused.cpu().numpy(), streamed.cpu().numpy()) <= STREAM_TOL


def test_sym_and_mmd():
    lx, ly = _lens(5, 6, 12), _lens(6, 5, 10)
    gen = torch.Generator().manual_seed(5)
    X, Y = walk(gen, 6, 12, 3).to(DEV), walk(gen, 5, 10, 3).to(DEV)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(1.0), 1)
    K = sk.compute_Gram_ragged(X, X, lx, torch.tensor(lx, device=DEV), sym=True)
    full = sk.compute_Gram_ragged(X, X, lx, lx)
    assert torch.equal(K, K.T) and torch.equal(K, 0.5 * (full + full.T))
    kxx, kyy, kxy = (_oracle_at(a, b, la, lb, "rbf", 1, False, True) for a, b, la, lb in ((X, X, lx, lx), (Y, Y, ly, ly), (X, Y, lx, ly)))
    assert rel_err(K.cpu().numpy(), kxx) <= FAST_TOL
    want = (kxx.sum() - np.trace(kxx)) / 30. + (kyy.sum() - np.trace(kyy)) / 20. - 2. * kxy.mean()
    got = float(sk.compute_mmd_ragged(X, lx, Y, ly))
    assert abs(got - want) <= 4 * FAST_TOL * max(kxx.max(), kyy.max(), kxy.max())


def test_nothing_of_the_grids_size_is_allocated():
    """128 x 128 pairs of 64 points: the (A, B, M, N) grid would be 537 MB; the call's peak rises by less than a tenth of that"""
    A, M, d = 128, 64, 3
    gen = torch.Generator().manual_seed(7)
    X, Y = walk(gen, A, M, d).to(DEV), walk(gen, A, M, d).to(DEV)
    lx, ly = _lens(8, A, M), _lens(9, A, M)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.LinearKernel(), 1)
    sk.compute_Gram_ragged(X[:2], Y[:2], lx[:2], ly[:2])          # warm-up: library handles, caches
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    K, n_prefix, n_streamed = _traced(lambda: sk.compute_Gram_ragged(X, Y, lx, ly))
    rise = torch.cuda.max_memory_allocated() - base
    assert n_prefix == 1 and n_streamed == 0
    assert rise < A * A * M * M * 8 / 10, rise
    assert rel_err(K.cpu().numpy(), _oracle_at(X, Y, lx, ly, "linear", 1, False, True)) <= FAST_TOL
