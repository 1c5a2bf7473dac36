"""compute_Gram_prefixes / compute_kernel_prefixes: out[..., m, n] = k_sig(x[:m+1], y[:n+1]) for every pair of prefixes.

Host logic on the oracle-backed back-end (no GPU): the route every input can take -- increments, the solver's full grid, its coarse
nodes -- against truncated compute_Gram / compute_kernel calls, node by node.  Node (i, j) of the PDE grid depends only on the cells
before it, so the solver part of a prefix kernel is identical by construction; only the static kernel's matrix product on truncated
tensors may round differently, hence 1e-12.  The SK_OP_PREFIX rule of sk_route_query is pinned against a table.
"""
import numpy as np
import pytest
import torch

import sigkernel_amd
from sigkernel_amd import _lib
from conftest import rel_err, walk

TOL = 1e-12
A, B, M, N, D = 3, 2, 6, 5, 3


def _kernel(kind):
    return sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(1.0)


def _paths(seed=0, a=A, b=B, m=M, n=N, d=D):
    gen = torch.Generator().manual_seed(seed)
    return walk(gen, a, m, d), walk(gen, b, n, d)


@pytest.mark.parametrize("naive", [False, True])
@pytest.mark.parametrize("dyadic", [0, 1, 2])
@pytest.mark.parametrize("kind", ["linear", "rbf"])
def test_gram_prefixes_equal_truncated_gram_calls_at_every_node(oracle_backend, kind, dyadic, naive):
    X, Y = _paths()
    sk = sigkernel_amd.SigKernel(_kernel(kind), dyadic, _naive_solver=naive)
    out = sk.compute_Gram_prefixes(X, Y)
    assert out.shape == (A, B, M, N) and out.dtype == X.dtype and out.device == X.device and out.grad_fn is None
    for m in range(M):
        for n in range(N):
            want = sk.compute_Gram(X[:, :m + 1], Y[:, :n + 1])
            assert rel_err(out[:, :, m, n].numpy(), want.numpy()) <= TOL, (m, n)
    assert bool((out[:, :, 0, :] == 1).all()) and bool((out[:, :, :, 0] == 1).all())
    assert torch.equal(out[..., -1, -1], sk.compute_Gram(X, Y))


@pytest.mark.parametrize("naive", [False, True])
@pytest.mark.parametrize("dyadic", [0, 1, 2])
@pytest.mark.parametrize("kind", ["linear", "rbf"])
def test_kernel_prefixes_equal_truncated_kernel_calls_at_every_node(oracle_backend, kind, dyadic, naive):
    X, Y = _paths(1, b=A)
    sk = sigkernel_amd.SigKernel(_kernel(kind), dyadic, _naive_solver=naive)
    out = sk.compute_kernel_prefixes(X, Y)
    assert out.shape == (A, M, N) and out.dtype == X.dtype and out.grad_fn is None
    for m in range(M):
        for n in range(N):
            want = sk.compute_kernel(X[:, :m + 1], Y[:, :n + 1])
            assert rel_err(out[:, m, n].numpy(), want.numpy()) <= TOL, (m, n)
    assert bool((out[:, 0, :] == 1).all()) and bool((out[:, :, 0] == 1).all())
    assert torch.equal(out[..., -1, -1], sk.compute_kernel(X, Y))


def test_dtype_and_degenerate_shapes(oracle_backend):
    sk = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(0.7), 1)
    X, Y = _paths(2)
    out32 = sk.compute_Gram_prefixes(X.float(), Y.float())
    assert out32.dtype == torch.float32 and out32.shape == (A, B, M, N)
    np.testing.assert_allclose(out32.numpy(), sk.compute_Gram_prefixes(X, Y).numpy(), rtol=1e-4, atol=1e-5)
    one = sk.compute_Gram_prefixes(X[:, :1], Y)                     # M = 1
    assert one.shape == (A, B, 1, N) and bool((one == 1).all())
    one = sk.compute_Gram_prefixes(X, Y[:, :1])                     # N = 1
    assert one.shape == (A, B, M, 1) and bool((one == 1).all())
    one = sk.compute_kernel_prefixes(X[:2, :1], Y[:, :1])
    assert one.shape == (2, 1, 1) and bool((one == 1).all())
    assert sk.compute_Gram_prefixes(X[:0], Y).shape == (0, B, M, N)  # A = 0
    assert sk.compute_Gram_prefixes(X, Y[:0]).shape == (A, 0, M, N)  # B = 0
    assert sk.compute_kernel_prefixes(X[:0], Y[:0]).shape == (0, M, N)
    assert torch.equal(sk.compute_Gram_prefixes(X, Y, max_batch=1), sk.compute_Gram_prefixes(X, Y))
    with pytest.raises(ValueError):
        sk.compute_Gram_prefixes(X, Y[:, :, :2])
    with pytest.raises(ValueError):
        sk.compute_kernel_prefixes(X, Y)                             # paired: batch sizes differ


@pytest.mark.parametrize("gram", [True, False])
def test_a_tiny_workspace_tiles_the_rows_and_changes_nothing(oracle_backend, gram, monkeypatch):
    X, Y = _paths(3, a=5, b=5 if not gram else B)
    be = _lib.get_backend()
    calls = []
    real = type(be).solve_fwd

    def counted(self, *a, **k):
        calls.append(1)
        return real(self, *a, **k)
    monkeypatch.setattr(type(be), "solve_fwd", counted)
    big = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(1.0), 1)
    small = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(1.0), 1, workspace_bytes=1)
    f = (lambda s: s.compute_Gram_prefixes(X, Y)) if gram else (lambda s: s.compute_kernel_prefixes(X, Y))
    want = f(big)
    assert len(calls) == 1
    del calls[:]
    got = f(small)
    assert len(calls) == 5           # one row per tile
    assert torch.equal(got, want)


def test_forward_only(oracle_backend):
    X, Y = _paths(4)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.LinearKernel(), 1)
    Xg = X.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="forward only"):
        sk.compute_Gram_prefixes(Xg, Y)
    with pytest.raises(NotImplementedError, match="forward only"):
        sk.compute_kernel_prefixes(X[:B], Y.clone().requires_grad_(True))
    with torch.no_grad():
        out = sk.compute_Gram_prefixes(Xg, Y)
    assert out.grad_fn is None and not out.requires_grad
    assert torch.equal(out, sk.compute_Gram_prefixes(X, Y))
    grouped = sigkernel_amd.SigKernel(sigkernel_amd.LinearKernel(), 1, process_group=object())
    with pytest.raises(NotImplementedError, match="process group"):
        grouped.compute_Gram_prefixes(X, Y)
    with pytest.raises(NotImplementedError, match="process group"):
        grouped.compute_kernel_prefixes(X[:B], Y)


def test_function_valued_kernel_goes_through_its_features(oracle_backend):
    gen = torch.Generator().manual_seed(5)
    X = walk(gen, 2, 5, 6).reshape(2, 5, 3, 2)
    Y = walk(gen, 3, 4, 6).reshape(3, 4, 3, 2)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.RBF_ID_Kernel(1.0), 1)
    out = sk.compute_Gram_prefixes(X, Y)
    assert out.shape == (2, 3, 5, 4)
    for m in range(5):
        for n in range(4):
            assert rel_err(out[:, :, m, n].numpy(), sk.compute_Gram(X[:, :m + 1], Y[:, :n + 1]).numpy()) <= TOL, (m, n)
    pair = sk.compute_kernel_prefixes(X, Y[:2])
    assert rel_err(pair[:, -1, -1].numpy(), sk.compute_kernel(X, Y[:2]).numpy()) <= TOL


@pytest.mark.parametrize("kind", ["linear", "rbf"])
def test_ragged_batches_are_one_gather(oracle_backend, kind):
    gen = torch.Generator().manual_seed(6)
    lens = [4, 7, 5]
    paths = [walk(gen, 1, n, D)[0] for n in lens]
    others = [walk(gen, 1, n, D)[0] for n in reversed(lens)]
    Lx, Ly = max(lens), max(lens)
    X = torch.stack([torch.cat([p, torch.full((Lx - p.shape[0], D), 1e3, dtype=p.dtype)]) for p in paths])      # padded with anything
    Y = torch.stack([torch.cat([p, torch.full((Ly - p.shape[0], D), -7.0, dtype=p.dtype)]) for p in others])
    sk = sigkernel_amd.SigKernel(_kernel(kind), 1)
    grid = sk.compute_kernel_prefixes(X, Y)
    ia = torch.tensor(lens) - 1
    ib = torch.tensor(list(reversed(lens))) - 1
    got = grid[torch.arange(3), ia, ib]
    want = torch.stack([sk.compute_kernel(p[None], q[None])[0] for p, q in zip(paths, others)])
    assert rel_err(got.numpy(), want.numpy()) <= TOL


FUSED, STREAM = _lib.ROUTE_FUSED, _lib.ROUTE_STREAM
# (kind, D, M, N, dyadic, naive, elem_size) -> SK_OP_PREFIX's answer: one band per pair -- rows <= 64 RC, RC = 4 / 2 / 1 at dyadic
# 0 / 1 / 2, rows = M - 1 linear, M rbf; rbf at dyadic 0: two rows per lane -- path dim <= 8, dyadic <= 2, any N; never swapped
PREFIX_TABLE = [
    ((0, 8, 128, 128, 1, False, 8), FUSED), ((1, 3, 64, 64, 1, False, 8), FUSED), ((1, 4, 64, 64, 2, False, 8), FUSED),
    ((0, 8, 128, 128, 1, False, 4), FUSED), ((0, 1, 2, 2, 0, True, 8), FUSED), ((1, 8, 64, 5000, 2, True, 4), FUSED),
    ((0, 8, 257, 40, 0, False, 8), FUSED), ((0, 8, 258, 40, 0, False, 8), STREAM),
    ((0, 5, 129, 40, 1, False, 8), FUSED), ((0, 5, 130, 40, 1, False, 8), STREAM),
    ((0, 5, 65, 40, 2, False, 8), FUSED), ((0, 5, 66, 40, 2, False, 8), STREAM), ((0, 5, 129, 40, 2, False, 8), STREAM),
    ((1, 4, 128, 40, 0, False, 8), FUSED), ((1, 4, 129, 40, 0, False, 8), STREAM), ((1, 8, 128, 40, 0, True, 4), FUSED),
    ((1, 5, 128, 40, 1, False, 8), FUSED), ((1, 5, 129, 40, 1, False, 8), STREAM),
    ((1, 5, 64, 40, 2, False, 8), FUSED), ((1, 5, 65, 40, 2, False, 8), STREAM),
    ((0, 3, 300, 20, 1, False, 8), STREAM),      # the second paths would fit: no swapped form (it would need a transposed store)
    ((0, 9, 30, 30, 1, False, 8), STREAM), ((1, 12, 30, 30, 1, False, 8), STREAM), ((0, 3, 30, 30, 3, False, 8), STREAM),
    ((2, 3, 30, 30, 1, False, 8), STREAM), ((0, 3, 1, 30, 1, False, 8), STREAM), ((0, 3, 30, 1, 1, False, 8), STREAM),
    ((0, 17, 30, 30, 1, False, 8), STREAM), ((0, 3, 30, 30, 1, False, 2), STREAM),
]


def test_route_query_knows_the_prefix_op():
    be = _lib.HipBackend()
    assert _lib.OP_PREFIX == 3
    for args, want in PREFIX_TABLE:
        assert be.route(_lib.OP_PREFIX, *args) == want, (args, be.route(_lib.OP_PREFIX, *args), want)
        assert be.route(_lib.OP_PREFIX, *args, no_stream=True) == want, args      # no other fused family serves a prefix grid
    # the other ops answer on these shapes what they answered before (values of tests/test_routes.py's table)
    MB, FSWAP = _lib.ROUTE_FUSED_MB, _lib.ROUTE_FUSED_SWAP
    for args, want in [((_lib.OP_FORWARD, 0, 8, 128, 128, 1, False, 8), FUSED), ((_lib.OP_ADJOINT, 0, 8, 128, 128, 1, False, 8), FUSED),
                       ((_lib.OP_FORWARD, 0, 8, 258, 260, 0, False, 8), MB), ((_lib.OP_FORWARD, 0, 3, 700, 20, 0, False, 8), FSWAP),
                       ((_lib.OP_ADJOINT, 0, 9, 20, 20, 1, False, 8), STREAM), ((_lib.OP_ADJOINT_SYM, 1, 3, 64, 64, 1, False, 8), FUSED),
                       ((_lib.OP_ADJOINT_SYM, 1, 3, 65, 65, 1, False, 8), STREAM), ((_lib.OP_FORWARD, 1, 5, 129, 100, 0, False, 8), FSWAP)]:
        assert be.route(*args) == want, args
    assert _lib.load().sk_version() == 340       # purely additive


def test_prefix_entry_points_report_bad_arguments_without_a_device():
    lib = _lib.load()
    buf = (8 * 4096) * b"\0"
    import ctypes
    p = ctypes.cast(ctypes.create_string_buffer(buf), ctypes.c_void_p).value
    ok = dict(A=1, B=1, Mrows=256, Mc=3, Nc=3, Ncp=16, D=2, dyadic=1, scheme=0)

    def lin(out=p, ldo=16, **kw):
        a = dict(ok, **kw)
        return lib.sk_solve_prefix_linear_f64(p, p, a["A"], a["B"], a["Mrows"], a["Mc"], a["Nc"], a["Ncp"], a["D"], a["dyadic"], a["scheme"],
                                              out, ldo, None, None)

    def rbf(inv_sigma=1.0, out=p, ldo=16, **kw):
        a = dict(ok, **kw)
        return lib.sk_solve_prefix_rbf_f32(p, p, a["A"], a["B"], a["Mrows"], a["Mc"], a["Nc"], a["Ncp"], a["D"], a["dyadic"], a["scheme"],
                                           inv_sigma, out, ldo, None, None)
    BAD = 1
    assert lin(out=None) == BAD and lin(ldo=15) == BAD and lin(Mc=0) == BAD and lin(D=0) == BAD and lin(scheme=7) == BAD and lin(A=-1) == BAD
    assert rbf(inv_sigma=0.0) == BAD and rbf(inv_sigma=float("nan")) == BAD and rbf(ldo=0) == BAD and rbf(dyadic=-1) == BAD
    assert lin(A=0) == 0 and rbf(A=0) == 0                       # nothing to do: no launch
    UNSUPPORTED = 2
    assert lin(D=9) == UNSUPPORTED and lin(dyadic=3) == UNSUPPORTED and lin(Mc=300, ldo=301 * 4) == UNSUPPORTED
    assert rbf(Mc=128, dyadic=0, ldo=129 * 4) == UNSUPPORTED     # 129 node rows on two rows per lane
