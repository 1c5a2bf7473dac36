"""Slices of the prefix grid: compute_Gram_prefixes / compute_kernel_prefixes with nodes="diagonal" | "last_row" | "last_col", and
compute_mmd_prefixes.

Host logic on the oracle-backed back-end (no GPU), as tests/test_prefixes_host.py: every element of a slice against a
compute_Gram / compute_kernel call on the truncated paths at that file's bar (1e-12: the solver part of a prefix kernel is identical by
construction, only the static kernel's matrix product on truncated tensors may round differently), and against the matching slice of
nodes="all" exactly (the same numbers, taken from the same grid).
"""
import numpy as np
import pytest
import torch

import sigkernel_amd
from sigkernel_amd import _lib
from conftest import rel_err, walk

TOL = 1e-12          # tests/test_prefixes_host.py
A, B, D = 3, 2, 3
LENGTHS = [(4, 6), (5, 5), (6, 4)]      # M < N, M == N, M > N
NODES = ["diagonal", "last_row", "last_col"]


def _kernel(kind):
    return sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(1.0)


def _paths(seed, m, n, a=A, b=B, d=D):
    gen = torch.Generator().manual_seed(seed)
    return walk(gen, a, m, d), walk(gen, b, n, d)


def _length(nodes, M, N):
    return {"diagonal": min(M, N), "last_row": N, "last_col": M}[nodes]


def _truncations(nodes, M, N):
    """(points of x, points of y) behind element i of the slice"""
    if nodes == "diagonal":
        return [(t + 1, t + 1) for t in range(min(M, N))]
    if nodes == "last_row":
        return [(M, n + 1) for n in range(N)]
    return [(m + 1, N) for m in range(M)]


def _slice_of(grid, nodes):
    if nodes == "diagonal":
        return torch.diagonal(grid, dim1=-2, dim2=-1)
    return grid[..., -1, :] if nodes == "last_row" else grid[..., :, -1]


@pytest.mark.parametrize("M,N", LENGTHS)
@pytest.mark.parametrize("nodes", NODES)
@pytest.mark.parametrize("naive", [False, True])
@pytest.mark.parametrize("dyadic", [0, 1, 2])
@pytest.mark.parametrize("kind", ["linear", "rbf"])
def test_gram_slices_equal_truncated_gram_calls_at_every_index(oracle_backend, kind, dyadic, naive, nodes, M, N):
    X, Y = _paths(10 * M + N, M, N)
    sk = sigkernel_amd.SigKernel(_kernel(kind), dyadic, _naive_solver=naive)
    out = sk.compute_Gram_prefixes(X, Y, nodes=nodes)
    assert out.shape == (A, B, _length(nodes, M, N)) and out.dtype == X.dtype and out.device == X.device and out.grad_fn is None
    for i, (m, n) in enumerate(_truncations(nodes, M, N)):
        want = sk.compute_Gram(X[:, :m], Y[:, :n])
        assert rel_err(out[:, :, i].numpy(), want.numpy()) <= TOL, (i, m, n)
    assert bool((out[..., 0] == 1).all())
    if nodes != "diagonal" or M == N:
        assert torch.equal(out[..., -1], sk.compute_Gram(X, Y))
    assert torch.equal(out, _slice_of(sk.compute_Gram_prefixes(X, Y), nodes))
    assert torch.equal(out, _slice_of(sk.compute_Gram_prefixes(X, Y, nodes="all"), nodes))


@pytest.mark.parametrize("M,N", LENGTHS)
@pytest.mark.parametrize("nodes", NODES)
@pytest.mark.parametrize("naive", [False, True])
@pytest.mark.parametrize("dyadic", [0, 1, 2])
@pytest.mark.parametrize("kind", ["linear", "rbf"])
def test_kernel_slices_equal_truncated_kernel_calls_at_every_index(oracle_backend, kind, dyadic, naive, nodes, M, N):
    X, Y = _paths(100 + 10 * M + N, M, N, b=A)
    sk = sigkernel_amd.SigKernel(_kernel(kind), dyadic, _naive_solver=naive)
    out = sk.compute_kernel_prefixes(X, Y, nodes=nodes)
    assert out.shape == (A, _length(nodes, M, N)) and out.dtype == X.dtype and out.grad_fn is None
    for i, (m, n) in enumerate(_truncations(nodes, M, N)):
        want = sk.compute_kernel(X[:, :m], Y[:, :n])
        assert rel_err(out[:, i].numpy(), want.numpy()) <= TOL, (i, m, n)
    assert bool((out[..., 0] == 1).all())
    if nodes != "diagonal" or M == N:
        assert torch.equal(out[..., -1], sk.compute_kernel(X, Y))
    assert torch.equal(out, _slice_of(sk.compute_kernel_prefixes(X, Y), nodes))


@pytest.mark.parametrize("nodes", NODES)
def test_shapes_dtype_and_degenerate_inputs(oracle_backend, nodes):
    M, N = 6, 5
    sk = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(0.7), 1)
    X, Y = _paths(2, M, N)
    L = _length(nodes, M, N)
    out32 = sk.compute_Gram_prefixes(X.float(), Y.float(), nodes=nodes)
    assert out32.dtype == torch.float32 and out32.shape == (A, B, L)
    np.testing.assert_allclose(out32.numpy(), sk.compute_Gram_prefixes(X, Y, nodes=nodes).numpy(), rtol=1e-4, atol=1e-5)
    # one-point paths: every prefix kernel is 1
    one = sk.compute_Gram_prefixes(X[:, :1], Y, nodes=nodes)                     # M = 1
    assert one.shape == (A, B, _length(nodes, 1, N)) and bool((one == 1).all())
    one = sk.compute_Gram_prefixes(X, Y[:, :1], nodes=nodes)                     # N = 1
    assert one.shape == (A, B, _length(nodes, M, 1)) and bool((one == 1).all())
    one = sk.compute_kernel_prefixes(X[:2, :1], Y[:, :1], nodes=nodes)
    assert one.shape == (2, 1) and bool((one == 1).all())
    # empty batches
    assert sk.compute_Gram_prefixes(X[:0], Y, nodes=nodes).shape == (0, B, L)
    assert sk.compute_Gram_prefixes(X, Y[:0], nodes=nodes).shape == (A, 0, L)
    assert sk.compute_kernel_prefixes(X[:0], Y[:0], nodes=nodes).shape == (0, L)
    assert torch.equal(sk.compute_Gram_prefixes(X, Y, max_batch=1, nodes=nodes), sk.compute_Gram_prefixes(X, Y, nodes=nodes))
    with pytest.raises(ValueError):
        sk.compute_Gram_prefixes(X, Y[:, :, :2], nodes=nodes)
    with pytest.raises(ValueError):
        sk.compute_kernel_prefixes(X, Y, nodes=nodes)                             # paired: batch sizes differ


def test_an_unknown_value_of_nodes_is_a_value_error(oracle_backend):
    X, Y = _paths(3, 5, 4)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.LinearKernel(), 0)
    for bad in ("diag", "row", "ALL", "", None, 1):
        with pytest.raises(ValueError, match="nodes"):
            sk.compute_Gram_prefixes(X, Y, nodes=bad)
        with pytest.raises(ValueError, match="nodes"):
            sk.compute_kernel_prefixes(X[:B], Y, nodes=bad)
    fn = sigkernel_amd.SigKernel(sigkernel_amd.RBF_ID_Kernel(1.0), 0)
    with pytest.raises(ValueError, match="nodes"):
        fn.compute_Gram_prefixes(X.reshape(A, 5, 3, 1), Y.reshape(B, 4, 3, 1), nodes="diag")


@pytest.mark.parametrize("nodes", NODES)
@pytest.mark.parametrize("gram", [True, False])
def test_a_tiny_workspace_tiles_the_rows_and_changes_nothing(oracle_backend, gram, nodes, monkeypatch):
    """Outside the fused scope the slice is taken tile by tile: one solver call per row under a one-byte budget, no grid of the whole
    batch, the same numbers."""
    X, Y = _paths(3, 6, 5, a=5, b=5 if not gram else B)
    be = _lib.get_backend()
    calls, biggest = [], [0]
    real = type(be).solve_fwd

    def counted(self, inc, *a, **k):
        calls.append(1)
        res = real(self, inc, *a, **k)
        biggest[0] = max(biggest[0], res[1].shape[0])
        return res
    monkeypatch.setattr(type(be), "solve_fwd", counted)
    big = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(1.0), 1)
    small = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(1.0), 1, workspace_bytes=1)
    f = (lambda s: s.compute_Gram_prefixes(X, Y, nodes=nodes)) if gram else (lambda s: s.compute_kernel_prefixes(X, Y, nodes=nodes))
    want = f(big)
    assert len(calls) == 1
    del calls[:]
    biggest[0] = 0
    got = f(small)
    assert len(calls) == 5 and biggest[0] == 1          # one row per tile
    assert torch.equal(got, want)


@pytest.mark.parametrize("nodes", NODES)
def test_forward_only(oracle_backend, nodes):
    X, Y = _paths(4, 6, 5)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.LinearKernel(), 1)
    Xg = X.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="forward only"):
        sk.compute_Gram_prefixes(Xg, Y, nodes=nodes)
    with pytest.raises(NotImplementedError, match="forward only"):
        sk.compute_kernel_prefixes(X[:B], Y.clone().requires_grad_(True), nodes=nodes)
    with torch.no_grad():
        out = sk.compute_Gram_prefixes(Xg, Y, nodes=nodes)
    assert out.grad_fn is None and not out.requires_grad
    assert torch.equal(out, sk.compute_Gram_prefixes(X, Y, nodes=nodes))
    grouped = sigkernel_amd.SigKernel(sigkernel_amd.LinearKernel(), 1, process_group=object())
    with pytest.raises(NotImplementedError, match="process group"):
        grouped.compute_Gram_prefixes(X, Y, nodes=nodes)
    with pytest.raises(NotImplementedError, match="process group"):
        grouped.compute_kernel_prefixes(X[:B], Y, nodes=nodes)


@pytest.mark.parametrize("nodes", NODES)
def test_function_valued_kernel_goes_through_its_features(oracle_backend, nodes):
    gen = torch.Generator().manual_seed(5)
    X = walk(gen, 2, 5, 6).reshape(2, 5, 3, 2)
    Y = walk(gen, 3, 4, 6).reshape(3, 4, 3, 2)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.RBF_ID_Kernel(1.0), 1)
    out = sk.compute_Gram_prefixes(X, Y, nodes=nodes)
    assert out.shape == (2, 3, _length(nodes, 5, 4))
    for i, (m, n) in enumerate(_truncations(nodes, 5, 4)):
        assert rel_err(out[:, :, i].numpy(), sk.compute_Gram(X[:, :m], Y[:, :n]).numpy()) <= TOL, (i, m, n)
    assert torch.equal(out, _slice_of(sk.compute_Gram_prefixes(X, Y), nodes))
    pair = sk.compute_kernel_prefixes(X, Y[:2], nodes=nodes)
    assert torch.equal(pair, _slice_of(sk.compute_kernel_prefixes(X, Y[:2]), nodes))


# compute_mmd_prefixes against compute_mmd on truncated paths.  Both are  mean'(K_XX) + mean'(K_YY) - 2 mean(K_XY)  of Gram matrices that
# agree entry by entry to TOL relative to their largest entry (the tests above), and compute_mmd may sum in another order (its merged
# route): each of the three means is then within TOL * max|K| of the other's, the factor 2 makes it four such terms.  The MMD itself is a
# difference of numbers of size max|K|, so the bound is absolute in that scale, not relative to the MMD.
def _mmd_bound(sk, X, Y, t):
    kmax = max(float(sk.compute_Gram(Z[:, :t + 1], W[:, :t + 1]).abs().max()) for Z, W in ((X, X), (Y, Y), (X, Y)))
    return 4 * TOL * kmax


@pytest.mark.parametrize("M,N", [(5, 7), (6, 6), (7, 4)])
@pytest.mark.parametrize("dyadic", [0, 1])
@pytest.mark.parametrize("kind", ["linear", "rbf"])
def test_mmd_prefixes_equal_mmd_of_truncated_paths(oracle_backend, kind, dyadic, M, N):
    X, Y = _paths(7 * M + N, M, N, a=4, b=5)
    sk = sigkernel_amd.SigKernel(_kernel(kind), dyadic)
    out = sk.compute_mmd_prefixes(X, Y)
    T = min(M, N)
    assert out.shape == (T,) and out.dtype == X.dtype and out.grad_fn is None
    assert float(out[0]) == 0.0
    for t in range(1, T):
        want = float(sk.compute_mmd(X[:, :t + 1], Y[:, :t + 1]))
        assert abs(float(out[t]) - want) <= _mmd_bound(sk, X, Y, t), (t, float(out[t]), want)


def test_mmd_prefixes_refuse_a_gradient_and_a_process_group(oracle_backend):
    X, Y = _paths(8, 5, 5, a=3, b=3)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(1.0), 0)
    with pytest.raises(NotImplementedError, match="forward only"):
        sk.compute_mmd_prefixes(X.clone().requires_grad_(True), Y)
    with pytest.raises(NotImplementedError, match="forward only"):
        sk.compute_mmd_prefixes(X, Y.clone().requires_grad_(True))
    with torch.no_grad():
        out = sk.compute_mmd_prefixes(X.clone().requires_grad_(True), Y)
    assert out.grad_fn is None and torch.equal(out, sk.compute_mmd_prefixes(X, Y))
    grouped = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(1.0), 0, process_group=object())
    with pytest.raises(NotImplementedError, match="process group"):
        grouped.compute_mmd_prefixes(X, Y)


def test_mmd_prefixes_of_function_valued_paths(oracle_backend):
    gen = torch.Generator().manual_seed(9)
    X = walk(gen, 3, 5, 6).reshape(3, 5, 3, 2)
    Y = walk(gen, 4, 6, 6).reshape(4, 6, 3, 2)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.RBF_ID_Kernel(1.0), 1)
    out = sk.compute_mmd_prefixes(X, Y)
    assert out.shape == (5,) and float(out[0]) == 0.0
    for t in range(1, 5):
        assert abs(float(out[t]) - float(sk.compute_mmd(X[:, :t + 1], Y[:, :t + 1]))) <= _mmd_bound(sk, X, Y, t), t


def test_slice_entry_points_report_bad_arguments_without_a_device():
    """The sibling entry points check their arguments before any HIP call, the slice's length in place of the grid's size."""
    import ctypes
    lib = _lib.load()
    p = ctypes.cast(ctypes.create_string_buffer((8 * 4096) * b"\0"), ctypes.c_void_p).value
    ok = dict(A=1, B=1, Mrows=256, Mc=3, Nc=5, Ncp=16, D=2, dyadic=1, scheme=0)

    def lin(nodes, out=p, ldo=6, **kw):
        a = dict(ok, **kw)
        return lib.sk_solve_prefix_nodes_linear_f64(p, p, a["A"], a["B"], a["Mrows"], a["Mc"], a["Nc"], a["Ncp"], a["D"], a["dyadic"],
                                                    a["scheme"], nodes, out, ldo, None, None)

    def rbf(nodes, inv_sigma=1.0, out=p, ldo=6, **kw):
        a = dict(ok, **kw)
        return lib.sk_solve_prefix_nodes_rbf_f32(p, p, a["A"], a["B"], a["Mrows"], a["Mc"], a["Nc"], a["Ncp"], a["D"], a["dyadic"],
                                                 a["scheme"], inv_sigma, nodes, out, ldo, None, None)
    BAD, UNSUPPORTED = 1, 2
    assert _lib.PREFIX_NODES == {"all": 0, "diagonal": 1, "last_row": 2, "last_col": 3}
    assert lin(4) == BAD and lin(-1) == BAD and rbf(7) == BAD
    # ldo: at least min(Mc, Nc) + 1 = 4 / Nc + 1 = 6 / Mc + 1 = 4 / (Mc + 1) (Nc + 1) = 24 elements
    assert lin(1, ldo=3) == BAD and lin(2, ldo=5) == BAD and lin(3, ldo=3) == BAD and lin(0, ldo=23) == BAD
    assert rbf(1, ldo=3) == BAD and rbf(2, ldo=5) == BAD and rbf(3, ldo=3) == BAD
    for nodes in (1, 2, 3):
        assert lin(nodes, out=None) == BAD and lin(nodes, Mc=0) == BAD and lin(nodes, scheme=7) == BAD
        assert rbf(nodes, inv_sigma=0.0) == BAD and rbf(nodes, dyadic=-1) == BAD
        assert lin(nodes, A=0) == 0 and rbf(nodes, A=0) == 0                       # nothing to do: no launch
        assert lin(nodes, D=9) == UNSUPPORTED and lin(nodes, dyadic=3) == UNSUPPORTED and lin(nodes, Mc=300, ldo=400) == UNSUPPORTED
