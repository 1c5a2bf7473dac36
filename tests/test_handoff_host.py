"""What a forward leaves for its backward (sigkernel._Kept / _Tile), on the CPU with the oracle-backed back-end: the record's own
decisions against literal tables, and -- through public calls and back-end hooks only -- that kept increments are freed before the
chain rule allocates, that nothing rides on a tensor as a Python attribute, and that a second backward through a retained graph
finds nothing kept and sweeps forward by itself."""
import weakref

import pytest
import torch

import sigkernel_amd
from conftest import golden
from fake_backend import OracleBackend

NAME = "gram_c2mini_rbf_d1"


def fixture():
    c = golden(NAME)
    X, Y, w = (torch.from_numpy(c[k]) for k in ("X", "Y", "w"))
    return c, X, Y, w, sigkernel_amd.RBFKernel(float(c["param"])), int(c["dyadic"])


def sixteen(X):
    """16 distinct paths from the fixture's 6: the symmetric route takes row blocks from 8 paths per block on"""
    gen = torch.Generator().manual_seed(5)
    return torch.cat([X, X + 0.01 * torch.randn(X.shape, generator=gen, dtype=X.dtype), X.flip(1), 0.5 * X])[:16].contiguous()


def sym_blocks(monkeypatch):
    from sigkernel_amd import sigkernel as S
    monkeypatch.setattr(S, "_SYM_TILES", 2)
    monkeypatch.setattr(S, "_SYM_MIN_CELLS", 0.0)
    monkeypatch.setattr(S, "_SYM_MIN_ROWS", 1)


class backend:
    """install a back-end for a with-block"""

    def __init__(self, be):
        self.be = be

    def __enter__(self):
        from sigkernel_amd import _lib
        self.prev = _lib.set_backend(self.be)
        return self.be

    def __exit__(self, *exc):
        from sigkernel_amd import _lib
        _lib.set_backend(self.prev)


# ---- the record's own decisions (these two tests know the record: they are the only ones that do not run on the commit before it)

def kept_of(*tiles, K=None):
    from sigkernel_amd import sigkernel as S
    kept = S._Kept(K=K)
    for t in tiles:
        kept.add(*t)
    return kept


E8 = torch.arange(8.0)          # edges of 4 rows, 2 numbers per row
INC = torch.ones(4, 3, 2, 2)

# kept tiles, n_rows, per_row, budget, strict -> [(a0, a1, edges, increments)], released?
TILINGS = [
    # one kept block, one backward tile: as kept, increments and all
    ([(0, 4, E8, INC)], 4, 10, 40, True, [(0, 4, E8, INC)], False),
    ([(0, 4, E8, INC)], 4, 10, 40, False, [(0, 4, E8, INC)], False),
    # one kept block, several backward tiles: its edges sliced per tile (the increments of all rows are of no use to a slice)
    ([(0, 4, E8, INC)], 4, 10, 20, True, [(0, 2, E8[0:4], None), (2, 4, E8[4:8], None)], False),
    ([(0, 4, E8, None)], 4, 10, 30, False, [(0, 3, E8[0:6], None), (3, 4, E8[6:8], None)], False),
    # the forward's own tiling, a tile without edges among them: as kept where it fits the budget ...
    ([(0, 2, E8[:4], None), (2, 4, None, None)], 4, 10, 20, True, [(0, 2, E8[:4], None), (2, 4, None, None)], False),
    ([(0, 2, E8[:4], None), (2, 4, E8[4:], None)], 4, 10, 40, True, [(0, 2, E8[:4], None), (2, 4, E8[4:], None)], False),
    # ... or, larger than the budget allows, where the caller is not strict about it
    ([(0, 3, E8[:6], None), (3, 4, E8[6:], None)], 4, 10, 20, False, [(0, 3, E8[:6], None), (3, 4, E8[6:], None)], False),
    # one block for all rows WITHOUT edges is a tiling like any other
    ([(0, 4, None, None)], 4, 10, 40, True, [(0, 4, None, None)], False),
    # strict, and the forward's tiles are larger than the budget allows: fresh tiles without edges, the record released
    ([(0, 3, E8[:6], None), (3, 4, E8[6:], None)], 4, 10, 20, True, [(0, 2, None, None), (2, 4, None, None)], True),
    ([(0, 4, None, INC)], 4, 10, 10, True, [(0, 1, None, None), (1, 2, None, None), (2, 3, None, None), (3, 4, None, None)], True),
    # nothing kept: fresh tiles
    ([], 4, 10, 20, True, [(0, 2, None, None), (2, 4, None, None)], True),
    ([], 5, 10, 1000, False, [(0, 5, None, None)], True),
]


def same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.data_ptr() == b.data_ptr() and torch.equal(a, b))


@pytest.mark.parametrize("row", range(len(TILINGS)))
def test_row_tiles_table(row):
    tiles, n_rows, per_row, budget, strict, want, released = TILINGS[row]
    kept = kept_of(*tiles, K=torch.zeros(n_rows))
    got = kept.row_tiles(n_rows, per_row, budget, strict=strict)
    assert [(t.a0, t.a1) for t in got] == [w[:2] for w in want]
    assert all(same(t.edges, w[2]) and same(t.increments, w[3]) for t, w in zip(got, want))
    assert (kept.tiles == []) == released and kept.K is not None


def test_whole_edges_take_increments_release():
    from sigkernel_amd import sigkernel as S
    # the one-whole-block predicate: ONE tile, all rows, with edges
    assert kept_of((0, 4, E8)).whole_edges(4) is E8
    assert kept_of((0, 4, E8)).whole_edges(5) is None and kept_of((0, 4, None)).whole_edges(4) is None
    assert kept_of((0, 2, E8), (2, 4, E8)).whole_edges(4) is None and kept_of().whole_edges(4) is None
    assert kept_of((1, 5, E8)).whole_edges(4) is None
    # taking a tile's increments clears the field, whatever comes back; another dtype than asked for gives None
    t = S._Tile(0, 4, E8, INC)
    assert t.take_increments(torch.float32) is INC and t.increments is None and t.take_increments(torch.float32) is None
    t = S._Tile(0, 4, E8, INC)
    assert t.take_increments(torch.float64) is None and t.increments is None
    kept = kept_of((0, 4, E8, INC), K=E8)
    kept.release()
    assert kept.tiles == [] and kept.K is E8
    # the consume-once helper: the record comes off ctx, None stays
    ctx = type("Ctx", (), {})()
    ctx.kept = kept
    assert S._take(ctx) is kept and ctx.kept is None and S._take(ctx) is None and S._take(ctx, "never_set") is None


# ---- through public calls and back-end hooks only

class Watching(OracleBackend):
    """static_increments remembers (weakly) what it returned; solve_adj which increments it is solving with; static_adjoint -- the
    chain rule, the next allocation -- insists that those are gone"""

    def __init__(self):
        self.formed, self.solving, self.chain_rules = [], None, 0

    def static_increments(self, *a, **kw):
        inc = OracleBackend.static_increments(self, *a, **kw)
        self.formed.append(weakref.ref(inc))
        return inc

    def solve_adj(self, inc_c, *a, **kw):
        self.solving = weakref.ref(inc_c)
        return OracleBackend.solve_adj(self, inc_c, *a, **kw)

    def static_adjoint(self, *a, **kw):
        assert self.solving is not None and self.solving() is None, "the increments outlive the adjoint sweep"
        self.chain_rules += 1
        return OracleBackend.static_adjoint(self, *a, **kw)


def test_kept_increments_are_gone_before_the_chain_rule_allocates(monkeypatch):
    c, X, Y, w, k, d = fixture()
    sk = sigkernel_amd.SigKernel(k, d)
    with backend(Watching()) as be:
        Xg = X.clone().requires_grad_(True)
        K = sk.compute_Gram(Xg, Y)
        assert len(be.formed) == 1 and be.formed[0]() is not None       # one tile: the forward kept what it formed ...
        (K * w).sum().backward()
        assert len(be.formed) == 1 and be.formed[0]() is None and be.chain_rules == 1       # ... backward used it, and let go
    sym_blocks(monkeypatch)
    with backend(Watching()) as be:
        Xg = sixteen(X).requires_grad_(True)
        K = sk.compute_Gram(Xg, Xg, sym=True)
        assert len(be.formed) == 2 and all(r() is not None for r in be.formed)        # two row blocks, each keeps its own
        K.sum().backward()
        assert len(be.formed) == 2 and all(r() is None for r in be.formed) and be.chain_rules == 2


def reachable_tensors(out):
    """every tensor reachable from the autograd nodes behind `out` through attributes, slots and containers"""
    seen, tensors, nodes, stack = set(), [], [], [out.grad_fn]
    while stack:      # the graph
        fn = stack.pop()
        if fn is None or id(fn) in seen:
            continue
        seen.add(id(fn))
        nodes.append(fn)
        stack.extend(f for f, _ in fn.next_functions)

    def walk(obj, depth=0):
        if obj is None or id(obj) in seen or depth > 6 or isinstance(obj, (str, bytes, int, float, bool, type)):
            return
        seen.add(id(obj))
        if isinstance(obj, torch.Tensor):
            tensors.append(obj)
        elif isinstance(obj, dict):
            for v in obj.values():
                walk(v, depth + 1)
        elif isinstance(obj, (list, tuple)):
            for v in obj:
                walk(v, depth + 1)
        elif type(obj).__module__.startswith("sigkernel_amd"):
            for name in list(getattr(obj, "__dict__", {})) + list(getattr(type(obj), "__slots__", ())):
                walk(getattr(obj, name, None), depth + 1)
    for fn in nodes:
        walk(dict(getattr(fn, "__dict__", {})))
        walk(tuple(getattr(fn, "saved_tensors", ())))
    return tensors


HANDOFFS = ["paired", "gram_one_tile", "gram_tiles", "sym_blocks", "loss_composed"]


def forward_of(which, monkeypatch):
    """(output with its graph, leaf) of one host-reachable way to leave something for backward"""
    c, X, Y, w, k, d = fixture()
    A, B, M, N = X.shape[0], Y.shape[0], X.shape[1], Y.shape[1]
    Xg = X.clone().requires_grad_(True)
    if which == "paired":
        return sigkernel_amd.SigKernel(k, d).compute_kernel(Xg, Y), Xg
    if which == "gram_one_tile":
        return sigkernel_amd.SigKernel(k, d).compute_Gram(Xg, Y), Xg
    if which == "gram_tiles":      # room for two rows of the streaming route per tile
        return sigkernel_amd.SigKernel(k, d, workspace_bytes=3 * B * M * N * 8 * 2).compute_Gram(Xg, Y), Xg
    if which == "sym_blocks":
        sym_blocks(monkeypatch)
        Xg = sixteen(X).requires_grad_(True)
        return sigkernel_amd.SigKernel(k, d).compute_Gram(Xg, Xg, sym=True), Xg
    return sigkernel_amd.SigKernel(k, d).compute_mmd(Xg, Y), Xg


@pytest.mark.parametrize("which", HANDOFFS)
def test_nothing_rides_on_a_tensor(oracle_backend, monkeypatch, which):
    out, _ = forward_of(which, monkeypatch)
    tensors = reachable_tensors(out)
    assert len(tensors) >= 2, "the walk did not reach the hand-off"
    assert all(t.__dict__ == {} for t in tensors), [sorted(t.__dict__) for t in tensors if t.__dict__]


class Counting(OracleBackend):
    def __init__(self):
        self.calls = 0

    def static_increments(self, *a, **kw):
        self.calls += 1
        return OracleBackend.static_increments(self, *a, **kw)


# static_increments calls of (the forward, the first backward, the second backward through the retained graph), as the commit before
# the record made them: what the forward kept spares the first backward a call per kept tile; the second finds nothing and forms
# everything again -- the symmetric call on ALL pairs in one tile (it falls from the triangle to the rows' route)
SECOND_BACKWARD = {"paired": (1, 1, 1), "gram_one_tile": (1, 0, 1), "gram_tiles": (3, 3, 3), "sym_blocks": (2, 0, 1), "loss_composed": (2, 0, 1)}


@pytest.mark.parametrize("which", HANDOFFS)
def test_second_backward_through_a_retained_graph(monkeypatch, which):
    with backend(Counting()) as be:
        out, Xg = forward_of(which, monkeypatch)
        w = torch.randn(out.shape, generator=torch.Generator().manual_seed(3), dtype=out.dtype)      # fixed, not symmetric
        loss = (out * w).sum()
        n_fwd, be.calls = be.calls, 0
        (g1,) = torch.autograd.grad(loss, Xg, retain_graph=True)
        n_first, be.calls = be.calls, 0
        (g2,) = torch.autograd.grad(loss, Xg, retain_graph=True)
        n_second = be.calls
    assert (n_fwd, n_first, n_second) == SECOND_BACKWARD[which]
    if which == "sym_blocks":
        # the first backward folds the triangle, the second takes the rows' route over all pairs (the blocks are gone with what
        # they kept; tests/golden/handoff_parent.npz holds the same fall on the GPU) -- the same sums in another order, so equal to
        # round-off, not bit for bit: the 1e-12 of test_host_logic.py::test_symmetric_gram_triangular_blocks_with_gradient, which
        # compares the same two routes (measured here: 5.2e-15)
        err = float((g1 - g2).abs().max() / g1.abs().max())
        print("sym_blocks: second backward against the first, max-norm relative:", err)
        assert err <= 1e-12
    else:
        assert torch.equal(g1, g2)
