"""Ragged batches OFF the fused prefix kernel's scope: one node per pair and no fine grid (sk_solve_fwd_at_*).

1. the streaming solver's per-pair end node (k_fwd_wave with WaveParams.cells), every non-EDGES variant, at back-end level: bit for bit
   what the same instance family gives on the increments CUT to the pair's own sub-grid (the same cell arithmetic in another geometry),
   and close to the CPU oracle on the cut;
2. the anti-diagonal kernel's sub-grid sweep (k_fwd_simple with FWD_RAGGED): bit for bit the node of its own stored grid;
3. the default route of compute_Gram_ragged / compute_kernel_ragged: the bits of the stored-grid gather (routes.no_ragged_nodes) without
   the grid's memory;
4. the opt-in route (routes.ragged_stream): the streaming kernel, within the streamed route's tolerance of the default route and of the
   oracle on the truncated paths, blind to whatever the padding holds;
5. the launches that existed before keep their bits (tests/golden/ragged_nodes_parent.npz, recorded on the parent commit).

Tolerances: STREAM_TOL, F32_RTOL / F32_ATOL as in tests/test_gpu_ragged.py."""
import ctypes

import numpy as np
import pytest
import torch

import sigkernel_amd
from sigkernel_amd import _lib, routes
from oracle import oracle as O
from conftest import golden, rel_err, walk
import ragged_nodes_cases as R

pytestmark = pytest.mark.gpu
STREAM_TOL = 1e-11                  # tests/test_gpu_ragged.py, tests/test_gpu_prefixes.py: the streamed route against the oracle
F32_RTOL, F32_ATOL = 1e-4, 1e-5     # tests/test_gpu_ragged.py (the reference's own fp32 acceptance)
DEV = "cuda"


def _traced(f):
    """(f(), {device symbol: launches})"""
    was = _lib.launch_trace(True)
    try:
        _lib.launch_counts(reset=True)
        out = f()
        torch.cuda.synchronize()
        counts = _lib.launch_counts(reset=True)
    finally:
        _lib.launch_trace(was)
    return out, {k.split(".kd")[0]: v for k, v in counts.items() if v > 0}


def _launched(counts, name):
    return sum(v for k, v in counts.items() if name in k)


def _cut(inc, mc, nc):
    """pair's own increments [:mc, :nc], copied to rows of whole 128-byte lines (16-byte aligned stride), zero-padded"""
    elem = inc.element_size()
    ld = -(-nc * elem // 128) * 128 // elem
    buf = torch.zeros(inc.shape[0], mc, ld, dtype=inc.dtype, device=inc.device)
    buf[..., :nc] = inc[:, :mc, :nc]
    return buf[..., :nc]


# ---- 1. every non-EDGES variant of k_fwd_wave ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", R.GEOMETRIES)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("naive", [False, True], ids=["default", "naive"])
@pytest.mark.parametrize("dyadic", [0, 1, 2, 3])
def test_streaming_kernel_stores_each_pairs_own_node(dyadic, naive, dtype, geometry):
    be = _lib.get_backend()
    elem = 8 if dtype == torch.float64 else 4
    for Mc, Nc in R.shapes(geometry, dyadic, elem):
        L, multiband = R.expected(geometry, Mc, Nc, dyadic, elem)
        cells = R.aimed_cells(Mc, Nc, dyadic, elem, seed=Mc + Nc)
        P = cells.shape[0]
        inc = R.increments(R.case_seed(dyadic, naive, Mc, Nc) + 1, P, Mc, Nc, dtype, DEV)
        got, counts = _traced(lambda: be.solve_fwd_at(inc, cells.to(DEV), dyadic, naive, flags=_lib.FLAG_FAST_ONLY))
        assert counts == {R.instance(dtype, dyadic, naive, multiband, L): 1}, counts
        assert got.shape == (P,) and got.dtype == dtype
        assert torch.equal(got, be.solve_fwd_at(inc, cells.to(DEV), dyadic, naive, flags=_lib.FLAG_FAST_ONLY))      # repeated: the same bits
        got = got.cpu().numpy()
        host = inc.cpu()
        oracle = np.ones(P)
        for mc, nc in sorted(set(map(tuple, cells.tolist()))):
            idx = np.nonzero((cells[:, 0] == mc).numpy() & (cells[:, 1] == nc).numpy())[0]
            if mc == 0 or nc == 0:
                assert (got[idx] == 1).all(), (mc, nc, got[idx])
                continue
            cut = _cut(inc[idx], mc, nc)
            ref = be.solve_fwd(cut, dyadic, naive, flags=_lib.FLAG_FAST_ONLY).cpu().numpy()
            assert np.array_equal(got[idx], ref), "(%d, %d) of %d x %d: not the cut sweep's bits: %r vs %r" % (mc, nc, Mc, Nc, got[idx], ref)
            oracle[idx] = O.solve_coarse(host[idx, :mc, :nc].double().numpy(), dyadic, naive)
        err = rel_err(got, oracle)
        print("d=%d naive=%d %s %s %d x %d, %d pairs: rel err vs oracle %.3e" % (dyadic, naive, dtype, geometry, Mc, Nc, P, err))
        if dtype == torch.float64:
            assert err <= STREAM_TOL, err
        else:
            np.testing.assert_allclose(got, oracle, rtol=F32_RTOL, atol=F32_ATOL)


# ---- 2. the anti-diagonal kernel's sub-grid sweep ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("dyadic,naive,Mc,Nc,ld", [(0, False, 9, 17, None), (1, True, 33, 7, None), (2, False, 7, 34, None), (3, True, 5, 9, None),
                                                   (4, False, 6, 5, None), (1, False, 13, 11, 11)])
def test_simple_kernel_sweeps_each_pairs_own_subgrid(dyadic, naive, Mc, Nc, ld, dtype):
    """dyadic 0-4; dyadic 4 and a row stride of 11 elements (no 16-byte multiple) are shapes the streaming kernel declines"""
    be = _lib.get_backend()
    elem = 8 if dtype == torch.float64 else 4
    cells = R.aimed_cells(Mc, Nc, min(dyadic, 3), elem, seed=dyadic)
    P = cells.shape[0]
    inc = R.increments(77 + dyadic, P, Mc, Nc, dtype, DEV, ld=ld)
    if dyadic == 4 or ld is not None:
        with pytest.raises(ValueError, match="sk_status 2"):
            be.solve_fwd_at(inc, cells.to(DEV), dyadic, naive, flags=_lib.FLAG_FAST_ONLY)
    got, counts = _traced(lambda: be.solve_fwd_at(inc, cells.to(DEV), dyadic, naive, flags=_lib.FLAG_SIMPLE))
    assert _launched(counts, "k_fwd_simple") == 1 and _launched(counts, "k_fwd_wave") == 0, counts
    _, grid, _ = be.solve_fwd(inc, dyadic, naive, want_grid=True)
    p = torch.arange(P, device=DEV)
    node = grid[p, cells[:, 0].to(DEV).long() << dyadic, cells[:, 1].to(DEV).long() << dyadic]
    assert torch.equal(got, node), "not the stored grid's node bit for bit"
    empty = ((cells[:, 0] == 0) | (cells[:, 1] == 0)).to(DEV)
    assert bool(empty.any()) and bool((got[empty] == 1).all())
    if dyadic == 4 or ld is not None:      # flags = 0 falls back to the same kernel where the streaming one declines
        assert torch.equal(got, be.solve_fwd_at(inc, cells.to(DEV), dyadic, naive, flags=0))


def test_a_wrong_table_touches_nothing_but_its_own_output():
    """values outside [0, Mc] x [0, Nc] are clamped; the only address formed from an entry is out + p (guard words around `out` survive)"""
    be = _lib.get_backend()
    Mc, Nc, dyadic = 9, 17, 1
    bad = torch.tensor([[-5, 3], [4, -1], [Mc + 100, 5], [3, Nc + 7], [2 ** 31 - 1, 2 ** 31 - 1], [-2 ** 31, -2 ** 31], [2 ** 31 - 1, -2 ** 31],
                        [Mc, Nc], [Mc + 1, Nc + 1]], dtype=torch.int32)
    clamped = torch.stack((bad[:, 0].clamp(0, Mc), bad[:, 1].clamp(0, Nc)), dim=-1)
    P = bad.shape[0]
    inc = R.increments(5, P, Mc, Nc, torch.float64, DEV)
    _, grid, _ = be.solve_fwd(inc, dyadic, False, want_grid=True)
    node = grid[torch.arange(P, device=DEV), clamped[:, 0].to(DEV).long() << dyadic, clamped[:, 1].to(DEV).long() << dyadic]
    for flags in (_lib.FLAG_SIMPLE, _lib.FLAG_FAST_ONLY):
        buf = torch.full((P + 64,), -77.0, dtype=torch.float64, device=DEV)
        buf[32:32 + P] = 1.0
        tab = bad.to(DEV)
        rc = _lib.load().sk_solve_fwd_at_f64(ctypes.c_void_p(inc.data_ptr()), inc.stride(-2), P, Mc, Nc, dyadic, 0, flags,
                                             ctypes.c_void_p(tab.data_ptr()), ctypes.c_void_p(buf[32:].data_ptr()), None)
        torch.cuda.synchronize()
        assert rc == 0, rc
        assert bool((buf[:32] == -77.0).all()) and bool((buf[32 + P:] == -77.0).all())
        if flags == _lib.FLAG_SIMPLE:
            assert torch.equal(buf[32:32 + P], node)
        else:
            assert rel_err(buf[32:32 + P].cpu().numpy(), node.cpu().numpy()) <= STREAM_TOL


def test_argument_errors():
    lib = _lib.load()
    inc = torch.zeros(2, 3, 4, dtype=torch.float64, device=DEV)
    tab = torch.ones(2, 2, dtype=torch.int32, device=DEV)
    out = torch.ones(2, dtype=torch.float64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.sk_solve_fwd_at_f64(p(inc), 4, 2, 3, 4, 1, 0, 0, None, p(out), None) == 1          # no table
    assert lib.sk_solve_fwd_at_f64(p(inc), 4, 2, 3, 4, 1, 0, 0, p(tab), None, None) == 1          # no output
    assert lib.sk_solve_fwd_at_f64(p(inc), 4, 2, 3, 4, 1, 0, _lib.FLAG_SIMPLE | _lib.FLAG_FAST_ONLY, p(tab), p(out), None) == 1
    assert lib.sk_solve_fwd_at_f64(p(inc), 4, 2, 3, 4, 1, 0, _lib.FLAG_EDGES_GIVEN, p(tab), p(out), None) == 1
    assert lib.sk_solve_fwd_at_f64(p(inc), 4, 0, 3, 4, 1, 0, 0, p(tab), p(out), None) == 0          # no pairs: nothing to do
    with pytest.raises(ValueError):
        _lib.get_backend().solve_fwd_at(inc, tab.long(), 1)


# ---- 3. the default route through the API ------------------------------------------------------------------------------------------------
def _kernel(kind):
    if kind == "linear":
        return sigkernel_amd.LinearKernel()
    return sigkernel_amd.RBFKernel(1.0) if kind == "rbf" else sigkernel_amd.RBF_SQR_Kernel(1.0, 2.0)


def _lens(seed, count, top):
    """as tests/test_gpu_ragged.py aims them: 1, 2 and the padded length, the first and the last rows, both parities, random ones"""
    aimed = [1, 2, top, 3, top - 1, 4, top - 2, 5, top - 3]
    if count < 3:
        aimed = [top, 2, 1]
    aimed = [v for i, v in enumerate(aimed) if 1 <= v <= top and v not in aimed[:i]]
    g = np.random.default_rng(seed)
    lens = (aimed + g.integers(1, top + 1, size=max(0, count - len(aimed))).tolist())[:count]
    return [int(v) for v in g.permutation(lens)]


def _paths(kind, seed, A, B, M, N, D, dtype=torch.float64):
    gen = torch.Generator().manual_seed(seed)
    if kind == "sqr":       # a function-valued kernel: paths (batch, T, Lx, d), D = Lx * d features twice over
        return walk(gen, A, M, D, dtype).reshape(A, M, D // 2, 2).to(DEV), walk(gen, B, N, D, dtype).reshape(B, N, D // 2, 2).to(DEV)
    return walk(gen, A, M, D, dtype).to(DEV), walk(gen, B, N, D, dtype).to(DEV)


OFF_SCOPE = [("linear", 1, 20, 17, 9), ("rbf", 1, 30, 25, 12), ("linear", 1, 140, 7, 3), ("rbf", 2, 70, 9, 3),      # tests/test_gpu_ragged.py
             ("rbf", 1, 12, 10, 40), ("sqr", 1, 14, 9, 6), ("linear", 4, 9, 8, 3)]


@pytest.mark.parametrize("kind,dyadic,M,N,D", OFF_SCOPE)
def test_default_route_keeps_the_bits_of_the_stored_grid(kind, dyadic, M, N, D, monkeypatch):
    for gram, A, B in ((True, 5, 6), (False, 7, 7)):
        X, Y = _paths(kind, M + N + D, A, B, M, N, D)
        lx, ly = _lens(M, A, M), _lens(N + 1, B, N)
        sk = sigkernel_amd.SigKernel(_kernel(kind), dyadic)
        call = (lambda s=sk: s.compute_Gram_ragged(X, Y, lx, ly)) if gram else (lambda s=sk: s.compute_kernel_ragged(X, Y, lx, ly))
        K, counts = _traced(call)
        assert _launched(counts, "k_fwd_simple") == 1 and _launched(counts, "k_fwd_wave") == 0 and _launched(counts, "k_fwd_prefix") == 0, counts
        tiled = sigkernel_amd.SigKernel(_kernel(kind), dyadic, workspace_bytes=1)
        assert torch.equal(K, call(tiled)), "tiled by a tiny workspace: other bits"
        monkeypatch.setattr(routes, "no_ragged_nodes", True)
        base, counts = _traced(call)
        monkeypatch.setattr(routes, "no_ragged_nodes", False)
        assert _launched(counts, "k_fwd_simple") == 1, counts
        assert torch.equal(K, base), "not the stored grid's node bit for bit"
        ones = torch.tensor([v == 1 for v in lx], device=DEV)
        assert bool((K[ones] == 1).all())


def _peak_rise(call):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = call()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    del out
    return rise


def test_default_route_allocates_no_fine_grid(monkeypatch):
    """32 x 32 pairs of 140 x 60 points, dim 3, dyadic 2 (two bands: off the fused scope): the fine grid of the padded pairs, which the
    stored-grid route must allocate, is 1024 x 557 x 237 doubles = 1.08 GB.  The call's peak stays below that; under the switch it exceeds
    it -- the second claim guards the measure itself."""
    A, M, N, D, dyadic = 32, 140, 60, 3, 2
    grid_bytes = A * A * (((M - 1) << dyadic) + 1) * (((N - 1) << dyadic) + 1) * 8
    X, Y = _paths("linear", 3, A, A, M, N, D)
    lx, ly = _lens(1, A, M), _lens(2, A, N)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.LinearKernel(), dyadic)
    assert not _lib.HipBackend.route(_lib.OP_PREFIX, 0, D, M, N, dyadic, False, 8) == _lib.ROUTE_FUSED
    sk.compute_Gram_ragged(X[:2], Y[:2], lx[:2], ly[:2])          # warm-up: library handles, caches
    rise = _peak_rise(lambda: sk.compute_Gram_ragged(X, Y, lx, ly))
    monkeypatch.setattr(routes, "no_ragged_nodes", True)
    rise_base = _peak_rise(lambda: sk.compute_Gram_ragged(X, Y, lx, ly))
    print("peak rise: %.1f MB (default), %.1f MB (stored grid); the grid: %.1f MB" % (rise / 1e6, rise_base / 1e6, grid_bytes / 1e6))
    assert rise < grid_bytes < rise_base, (rise, grid_bytes, rise_base)


# ---- 4. the opt-in route through the API -------------------------------------------------------------------------------------------------
def _oracle_at(X, Y, lx, ly, kind, dyadic, gram):
    """the oracle on the truncated paths x[:lx], y[:ly], one call per distinct pair of lengths; a one-point path: exactly 1"""
    k = _kernel(kind)
    Xc, Yc = X.double().cpu(), Y.double().cpu()
    lx, ly = np.asarray(lx), np.asarray(ly)
    out = np.ones((len(lx), len(ly)) if gram else (len(lx),))
    if gram:
        for m in sorted(set(lx.tolist()) - {1}):
            for n in sorted(set(ly.tolist()) - {1}):
                ia, ib = np.nonzero(lx == m)[0], np.nonzero(ly == n)[0]
                out[np.ix_(ia, ib)] = O.gram_forward(Xc[ia, :m], Yc[ib, :n], k, dyadic, False)
    else:
        for m, n in sorted(set(zip(lx.tolist(), ly.tolist()))):
            if m > 1 and n > 1:
                i = np.nonzero((lx == m) & (ly == n))[0]
                out[i] = O.solve_coarse(O.increments(k.batch_kernel(Xc[i, :m], Yc[i, :n]).numpy()), dyadic, False)
    return out


def _stream_check(monkeypatch, kind, dyadic, A, B, M, N, D, gram, seed=0, oracle=True):
    X, Y = _paths(kind, 1000 * dyadic + 10 * M + N + seed, A, B if gram else A, M, N, D)
    lx, ly = _lens(seed + M, A, M), _lens(seed + N + 1, B if gram else A, N)
    sk = sigkernel_amd.SigKernel(_kernel(kind), dyadic)
    call = (lambda s=sk: s.compute_Gram_ragged(X, Y, lx, ly)) if gram else (lambda s=sk: s.compute_kernel_ragged(X, Y, lx, ly))
    default = call()
    monkeypatch.setattr(routes, "ragged_stream", True)
    K, counts = _traced(call)
    assert _launched(counts, "k_fwd_wave") >= 1 and _launched(counts, "k_fwd_simple") == 0 and _launched(counts, "k_fwd_prefix") == 0, counts
    assert K.shape == default.shape and K.dtype == default.dtype
    err = rel_err(K.cpu().numpy(), default.cpu().numpy())
    assert err <= STREAM_TOL, err
    if oracle:
        err = rel_err(K.cpu().numpy(), _oracle_at(X, Y, lx, ly, kind, dyadic, gram))
        assert err <= STREAM_TOL, err
    assert torch.equal(K, call())                                                                     # repeated calls: the same bits
    assert torch.equal(K, call(sigkernel_amd.SigKernel(_kernel(kind), dyadic, workspace_bytes=1)))    # tiled: the same bits
    ones = torch.tensor([v == 1 for v in lx], device=DEV)
    assert bool((K[ones] == 1).all())
    monkeypatch.setattr(routes, "ragged_stream", False)
    return K


@pytest.mark.parametrize("A,B", [(1, 1), (5, 7), (130, 33)])
@pytest.mark.parametrize("kind,dyadic,M,N,D", [("linear", 1, 20, 17, 9), ("rbf", 1, 30, 25, 12), ("linear", 1, 140, 7, 3), ("rbf", 2, 70, 9, 3),
                                               ("linear", 0, 20, 17, 9), ("rbf", 3, 12, 10, 3)])
def test_opt_in_route_streams(kind, dyadic, M, N, D, A, B, monkeypatch):
    """Gram and paired; batch sizes that leave lane groups idle"""
    _stream_check(monkeypatch, kind, dyadic, A, B, M, N, D, True, seed=A)
    _stream_check(monkeypatch, kind, dyadic, A, B, M, N, D, False, seed=B)


def test_opt_in_route_many_short_pairs(monkeypatch):
    """40 000 paired pairs of 9 x 8 points, dim 9: several pairs per lane group, and the shares by age rank"""
    _stream_check(monkeypatch, "linear", 1, 40000, 40000, 9, 8, 9, False, oracle=False)
    _stream_check(monkeypatch, "rbf", 0, 5000, 5000, 9, 8, 9, False)


def test_opt_in_route_sym_and_mmd(monkeypatch):
    lx, ly = _lens(5, 6, 12), _lens(6, 5, 10)
    X, Y = _paths("rbf", 5, 6, 5, 12, 10, 9)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(1.0), 1)
    monkeypatch.setattr(routes, "ragged_stream", True)
    (K, full, mmd), counts = _traced(lambda: (sk.compute_Gram_ragged(X, X, lx, torch.tensor(lx, device=DEV), sym=True),
                                              sk.compute_Gram_ragged(X, X, lx, lx), sk.compute_mmd_ragged(X, lx, Y, ly)))
    assert _launched(counts, "k_fwd_wave") >= 5 and _launched(counts, "k_fwd_simple") == 0, counts
    assert torch.equal(K, K.T) and torch.equal(K, 0.5 * (full + full.T))
    kxx, kyy, kxy = (_oracle_at(a, b, la, lb, "rbf", 1, True) for a, b, la, lb in ((X, X, lx, lx), (Y, Y, ly, ly), (X, Y, lx, ly)))
    assert rel_err(K.cpu().numpy(), kxx) <= STREAM_TOL
    want = (kxx.sum() - np.trace(kxx)) / 30. + (kyy.sum() - np.trace(kyy)) / 20. - 2. * kxy.mean()
    assert abs(float(mmd) - want) <= 4 * STREAM_TOL * max(kxx.max(), kyy.max(), kxy.max())


@pytest.mark.parametrize("poison", [1e300, float("inf"), float("nan")])
@pytest.mark.parametrize("kind,dyadic,M,N,D", [("linear", 1, 20, 17, 9), ("rbf", 1, 30, 25, 12), ("linear", 2, 140, 7, 3), ("rbf", 2, 70, 9, 3)])
def test_opt_in_route_is_blind_to_the_padding(kind, dyadic, M, N, D, poison, monkeypatch):
    """the sweep runs the padded shape: whatever stands behind a path's end reaches no result, not even through a select"""
    monkeypatch.setattr(routes, "ragged_stream", True)
    A, B = 6, 7
    X, Y = _paths(kind, M + D, A, B, M, N, D)
    lx, ly = _lens(3, A, M), _lens(4, B, N)
    sk = sigkernel_amd.SigKernel(_kernel(kind), dyadic)
    clean, counts = _traced(lambda: sk.compute_Gram_ragged(X, Y, lx, ly))
    assert _launched(counts, "k_fwd_wave") == 1 and _launched(counts, "k_fwd_simple") == 0, counts
    X2, Y2 = X.clone(), Y.clone()
    for i, n in enumerate(lx):
        X2[i, n:] = poison
    for i, n in enumerate(ly):
        Y2[i, n:] = -poison
    assert bool(torch.isfinite(clean).all())
    assert torch.equal(clean, sk.compute_Gram_ragged(X2, Y2, lx, ly))
    lp = _lens(5, A, N)
    Y3 = Y[:A].clone()
    for i, n in enumerate(lp):
        Y3[i, n:] = -poison
    assert torch.equal(sk.compute_kernel_ragged(X, Y[:A], lx, lp), sk.compute_kernel_ragged(X2, Y3, lx, lp))


@pytest.mark.parametrize("kind,dyadic,M,N,D", [("linear", 1, 20, 17, 9), ("rbf", 2, 70, 9, 3)])
def test_opt_in_route_under_exact_gradient(kind, dyadic, M, N, D, monkeypatch):
    """the forward is the no-grad call's, bit for bit, on either route; the backward does not read the forward's values, so the
    gradients are the default route's, bit for bit"""
    A, B = 4, 5
    X, Y = _paths(kind, M, A, B, M, N, D)
    lx, ly = _lens(7, A, M), _lens(8, B, N)
    w = torch.linspace(-1, 1, A * B, dtype=torch.float64, device=DEV).reshape(A, B)

    def run():
        sk = sigkernel_amd.SigKernel(_kernel(kind), dyadic, exact_gradient=True)
        Xg, Yg = X.clone().requires_grad_(True), Y.clone().requires_grad_(True)
        K = sk.compute_Gram_ragged(Xg, Yg, lx, ly)
        (K * w).sum().backward()
        with torch.no_grad():
            plain = sk.compute_Gram_ragged(X, Y, lx, ly)
        return K.detach(), plain, Xg.grad, Yg.grad

    K0, plain0, gx0, gy0 = run()
    monkeypatch.setattr(routes, "ragged_stream", True)
    (K1, plain1, gx1, gy1), counts = _traced(run)
    assert _launched(counts, "k_fwd_wave") >= 2 and _launched(counts, "k_fwd_simple") == 0, counts
    assert torch.equal(K0, plain0) and torch.equal(K1, plain1)
    assert rel_err(K1.cpu().numpy(), K0.cpu().numpy()) <= STREAM_TOL
    assert torch.equal(gx0, gx1) and torch.equal(gy0, gy1)


# ---- 5. existing launches keep their bits ------------------------------------------------------------------------------------------------
def test_plain_solves_keep_the_parents_bits():
    want = golden("ragged_nodes_parent")
    got = R.record(_lib, DEV)
    assert sorted(got) == sorted(want)
    bad = [k for k in sorted(want) if not np.array_equal(got[k], want[k])]
    assert not bad, "%d of %d cases differ from the parent's bits: %s" % (len(bad), len(want), bad[:8])
