"""compute_Gram_ragged / compute_kernel_ragged off the fused prefix kernel's scope, host logic (no GPU): with a back-end that has
solve_fwd_at, _prefix_at hands every row tile's increments and the table {len_x - 1, len_y - 1} of its pairs to it and never asks for a
fine grid; the two switches of sigkernel_amd.routes; a back-end without the method keeps the stored-grid gather.

The stand-in's solve_fwd_at is the CPU oracle on each pair's increments CUT to its own sub-grid: node (mc << d, nc << d) of the PDE grid
depends on the cells a < mc, b < nc alone, and the oracle sweeps them in the same order whatever the extent, so the result is the node of
the stored grid bit for bit."""
import numpy as np
import pytest
import torch

import sigkernel_amd
from sigkernel_amd import _lib, _routes, routes
from oracle import oracle as O
from conftest import rel_err, walk
from fake_backend import OracleBackend

TOL = 1e-12          # tests/test_ragged_host.py
D = 3
LEN_X = [1, 2, 6, 4, 6]
LEN_Y = [5, 1, 2, 3]


class NodesBackend(OracleBackend):
    """the oracle-backed stand-in plus solve_fwd_at; records every call's table, flags and tile, and every request for a grid"""

    def __init__(self):
        self.at_calls, self.grid_calls = [], 0

    def solve_fwd(self, inc_c, dyadic, naive=False, flags=0, want_grid=False, want_edges=False):
        self.grid_calls += bool(want_grid)
        return super().solve_fwd(inc_c, dyadic, naive, flags, want_grid, want_edges)

    def solve_fwd_at(self, inc_c, cells, dyadic, naive=False, flags=0):
        assert cells.dtype == torch.int32 and tuple(cells.shape) == tuple(inc_c.shape[:-2]) + (2,)
        self.at_calls.append((cells.clone(), int(flags), tuple(inc_c.shape)))
        a = inc_c.detach().double().numpy()
        flat, tab = a.reshape((-1,) + a.shape[-2:]), cells.reshape(-1, 2).tolist()
        out = np.ones(len(tab))
        for p, (mc, nc) in enumerate(tab):
            assert 0 <= mc <= a.shape[-2] and 0 <= nc <= a.shape[-1]
            if mc > 0 and nc > 0:
                out[p] = O.solve_coarse(np.ascontiguousarray(flat[p, :mc, :nc]), dyadic, naive)
        return torch.from_numpy(out.reshape(a.shape[:-2])).to(inc_c.dtype)


@pytest.fixture
def nodes_backend():
    be = NodesBackend()
    prev = _lib.set_backend(be)
    yield be
    _lib.set_backend(prev)


def _kernel(kind):
    return sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(1.0)


def _batch(seed, lens):
    gen = torch.Generator().manual_seed(seed)
    paths = [walk(gen, 1, n, D)[0] for n in lens]
    X, _ = sigkernel_amd.pad_paths(paths)
    return X, paths


def _stored_grid(call):
    """the same call on the stored-grid route: a back-end WITHOUT the method"""
    prev = _lib.set_backend(OracleBackend())
    try:
        return call()
    finally:
        _lib.set_backend(prev)


@pytest.mark.parametrize("dyadic", [0, 1, 2, 4])
@pytest.mark.parametrize("kind", ["linear", "rbf"])
def test_gram_hands_over_the_broadcast_table_and_asks_for_no_grid(nodes_backend, kind, dyadic):
    X, ps = _batch(0, LEN_X)
    Y, qs = _batch(1, LEN_Y)
    sk = sigkernel_amd.SigKernel(_kernel(kind), dyadic)
    K = sk.compute_Gram_ragged(X, Y, LEN_X, LEN_Y)
    assert nodes_backend.grid_calls == 0 and len(nodes_backend.at_calls) == 1
    cells, flags, shape = nodes_backend.at_calls[0]
    assert flags == _lib.FLAG_SIMPLE and shape == (5, 4, 5, 4)
    want = torch.stack((torch.tensor(LEN_X)[:, None].expand(5, 4) - 1, torch.tensor(LEN_Y)[None, :].expand(5, 4) - 1), dim=-1)
    assert torch.equal(cells.long(), want)
    assert K.shape == (5, 4) and K.dtype == X.dtype
    assert bool((K[0] == 1).all()) and bool((K[:, 1] == 1).all())          # lengths of 1: exactly 1
    assert torch.equal(K, _stored_grid(lambda: sk.compute_Gram_ragged(X, Y, LEN_X, LEN_Y))), "not the stored grid's node bit for bit"
    want = np.array([[1.0 if min(len(p), len(q)) < 2 else float(O.gram_forward(p[None], q[None], _kernel(kind), dyadic, False)[0, 0])
                      for q in qs] for p in ps])
    assert rel_err(K.numpy(), want) <= TOL


@pytest.mark.parametrize("kind", ["linear", "rbf"])
def test_paired_hands_over_its_own_table(nodes_backend, kind):
    lens_y = [3, 5, 1, 5, 2]
    X, _ = _batch(2, LEN_X)
    Y, _ = _batch(3, lens_y)
    sk = sigkernel_amd.SigKernel(_kernel(kind), 1)
    k = sk.compute_kernel_ragged(X, Y, torch.tensor(LEN_X), torch.tensor(lens_y, dtype=torch.int32))
    assert nodes_backend.grid_calls == 0 and len(nodes_backend.at_calls) == 1
    cells, flags, shape = nodes_backend.at_calls[0]
    assert flags == _lib.FLAG_SIMPLE and shape == (5, 5, 4)
    assert cells.tolist() == [[a - 1, b - 1] for a, b in zip(LEN_X, lens_y)]
    assert float(k[0]) == 1.0 and float(k[2]) == 1.0
    assert torch.equal(k, _stored_grid(lambda: sk.compute_kernel_ragged(X, Y, LEN_X, lens_y)))


@pytest.mark.parametrize("gram", [True, False])
def test_tiles_carry_their_slice_of_the_table(nodes_backend, gram):
    lens_y = LEN_Y if gram else [3, 5, 1, 5, 2]
    X, _ = _batch(5, LEN_X)
    Y, _ = _batch(6, lens_y)
    f = (lambda s: s.compute_Gram_ragged(X, Y, LEN_X, lens_y)) if gram else (lambda s: s.compute_kernel_ragged(X, Y, LEN_X, lens_y))
    want = f(sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(1.0), 1))
    del nodes_backend.at_calls[:]
    got = f(sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(1.0), 1, workspace_bytes=1))
    assert torch.equal(got, want) and nodes_backend.grid_calls == 0
    assert len(nodes_backend.at_calls) == len(LEN_X)           # one row per tile
    for a, (cells, _, shape) in enumerate(nodes_backend.at_calls):
        if gram:
            assert shape[:2] == (1, len(lens_y)) and cells.tolist() == [[[LEN_X[a] - 1, n - 1] for n in lens_y]]
        else:
            assert shape[0] == 1 and cells.tolist() == [[LEN_X[a] - 1, lens_y[a] - 1]]


def test_the_row_budget_holds_increments_and_table_but_no_grid(nodes_backend):
    """per row of a Gram tile: B pairs of (M - 1) rows of N + 16 padded increments, and 8 bytes of table each.  A budget of three such
    rows makes tiles of three rows; the stored-grid route at the same budget, whose rows also hold the fine grid, gets one row per tile"""
    A, B, M, N, dyadic = 7, 4, 6, 5, 3
    gen = torch.Generator().manual_seed(11)
    X, Y = walk(gen, A, M, D), walk(gen, B, N, D)
    lx, ly = [6, 2, 3, 1, 5, 6, 4], [5, 1, 2, 3]
    per_row = B * ((M - 1) * (N + 16) * 8 + 8)
    grid_row = B * (((M - 1) << dyadic) + 1) * (((N - 1) << dyadic) + 1) * 8
    assert 3 * per_row < per_row + grid_row          # (so that the two routes tile differently at this budget)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.LinearKernel(), dyadic, workspace_bytes=3 * per_row + per_row // 2)
    K = sk.compute_Gram_ragged(X, Y, lx, ly)
    assert [c[2][0] for c in nodes_backend.at_calls] == [3, 3, 1] and nodes_backend.grid_calls == 0
    routes_calls = []
    real = OracleBackend.solve_fwd

    class Counting(OracleBackend):
        def solve_fwd(self, inc_c, *a, **k):
            routes_calls.append(inc_c.shape[0])
            return real(self, inc_c, *a, **k)
    prev = _lib.set_backend(Counting())
    try:
        base = sk.compute_Gram_ragged(X, Y, lx, ly)
    finally:
        _lib.set_backend(prev)
    assert routes_calls == [1] * A
    assert torch.equal(K, base)


def test_no_ragged_nodes_restores_the_stored_grid(nodes_backend, monkeypatch):
    X, _ = _batch(7, LEN_X)
    Y, _ = _batch(8, LEN_Y)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(1.0), 1)
    K = sk.compute_Gram_ragged(X, Y, LEN_X, LEN_Y)
    assert (len(nodes_backend.at_calls), nodes_backend.grid_calls) == (1, 0)
    monkeypatch.setattr(routes, "no_ragged_nodes", True)
    monkeypatch.setattr(routes, "ragged_stream", True)          # without effect under the first switch
    base = sk.compute_Gram_ragged(X, Y, LEN_X, LEN_Y)
    assert (len(nodes_backend.at_calls), nodes_backend.grid_calls) == (1, 1)
    assert torch.equal(K, base)


@pytest.mark.parametrize("dyadic", [1, 4])
def test_ragged_stream_asks_for_the_streaming_kernel(nodes_backend, dyadic, monkeypatch):
    """flags = 0 at every dyadic order: above 3 the library's call takes the anti-diagonal kernel itself (no refinement on the host)"""
    X, _ = _batch(9, LEN_X)
    Y, _ = _batch(10, LEN_Y)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.LinearKernel(), dyadic)
    monkeypatch.setattr(routes, "ragged_stream", True)
    sk.compute_Gram_ragged(X, Y, LEN_X, LEN_Y)
    sk.compute_kernel_ragged(X[:4], Y, LEN_X[:4], LEN_Y)
    assert [c[1] for c in nodes_backend.at_calls] == [0, 0] and nodes_backend.grid_calls == 0


def test_the_switches_and_their_environment_names(monkeypatch):
    assert _routes._ENV["no_ragged_nodes"] == "SK_NO_RAGGED_NODES" and _routes._ENV["ragged_stream"] == "SK_RAGGED_STREAM"
    assert "SK_NO_RAGGED_NODES" in _routes.__doc__ and "SK_RAGGED_STREAM" in _routes.__doc__
    assert routes.no_ragged_nodes is False and routes.ragged_stream is False          # both off by default
    for attr, name in (("no_ragged_nodes", "SK_NO_RAGGED_NODES"), ("ragged_stream", "SK_RAGGED_STREAM")):
        monkeypatch.setenv(name, "1")
        r = _routes.Routes()
        assert getattr(r, attr) is True and sum(bool(getattr(r, a)) for a in _routes._ENV) == 1
        monkeypatch.delenv(name)
    assert not any(getattr(_routes.Routes(), a) for a in _routes._ENV)


def test_a_backend_without_the_method_takes_the_stored_grid(oracle_backend, monkeypatch):
    assert not hasattr(_lib.get_backend(), "solve_fwd_at")
    X, ps = _batch(12, LEN_X)
    Y, qs = _batch(13, LEN_Y)
    grids = []
    real = OracleBackend.solve_fwd

    def counted(self, inc_c, dyadic, naive=False, flags=0, want_grid=False, want_edges=False):
        grids.append(bool(want_grid))
        return real(self, inc_c, dyadic, naive, flags, want_grid, want_edges)
    monkeypatch.setattr(OracleBackend, "solve_fwd", counted)
    K = sigkernel_amd.SigKernel(sigkernel_amd.LinearKernel(), 1).compute_Gram_ragged(X, Y, LEN_X, LEN_Y)
    assert grids == [True]
    assert float(K[2, 0]) == float(O.gram_forward(ps[2][None], qs[0][None], sigkernel_amd.LinearKernel(), 1, False)[0, 0])


def test_one_point_batches_never_reach_the_backend(nodes_backend):
    gen = torch.Generator().manual_seed(14)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.LinearKernel(), 1)
    K = sk.compute_Gram_ragged(walk(gen, 3, 1, D), walk(gen, 2, 5, D), [1, 1, 1], [5, 2])
    assert K.shape == (3, 2) and bool((K == 1).all()) and not nodes_backend.at_calls
    k = sk.compute_kernel_ragged(walk(gen, 3, 4, D), walk(gen, 3, 5, D), [1, 1, 1], [1, 1, 1])          # every LENGTH 1 in padded batches
    assert bool((k == 1).all()) and len(nodes_backend.at_calls) == 1 and nodes_backend.at_calls[0][0].tolist() == [[0, 0]] * 3


def test_a_default_object_still_refuses_paths_that_require_grad(nodes_backend):
    X, _ = _batch(15, LEN_X)
    Y, _ = _batch(16, LEN_Y)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.LinearKernel(), 1)
    with pytest.raises(NotImplementedError, match="exact_gradient=True"):
        sk.compute_Gram_ragged(X.clone().requires_grad_(True), Y, LEN_X, LEN_Y)
    with pytest.raises(NotImplementedError, match="exact_gradient=True"):
        sk.compute_kernel_ragged(X[:4], Y.clone().requires_grad_(True), LEN_X[:4], LEN_Y)
    assert not nodes_backend.at_calls
    with torch.no_grad():
        sk.compute_Gram_ragged(X.clone().requires_grad_(True), Y, LEN_X, LEN_Y)
    assert len(nodes_backend.at_calls) == 1
