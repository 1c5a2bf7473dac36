"""compute_Gram_ragged / compute_kernel_ragged / compute_mmd_ragged / pad_paths: batches of paths of unequal length, padded at their ends.

Host logic on the oracle-backed back-end (no GPU): the tiled route -- increments, the solver's full grid, the gather of one node per
pair from every tile -- against the CPU oracle run PER PAIR on the truncated paths x[:len_x], y[:len_y].  Node (i, j) of the PDE grid
depends only on the cells before it, so the solver part is identical by construction; only the static kernel's matrix product on
truncated tensors may round differently, hence the forward bar of tests/test_prefixes_host.py.
"""
import numpy as np
import pytest
import torch

import sigkernel_amd
from sigkernel_amd import _lib
from oracle import oracle as O
from conftest import rel_err, walk

TOL = 1e-12          # tests/test_prefixes_host.py
D = 3
LEN_X = [1, 2, 6, 4, 6]          # one point (exactly 1), two points, the padded length
LEN_Y = [5, 1, 2, 3]


def _kernel(kind):
    return sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(1.0)


def _batch(seed, lens, pad=None):
    """paths of the given lengths, padded to max(lens) by pad_paths (pad=None) or with the constant `pad`"""
    gen = torch.Generator().manual_seed(seed)
    paths = [walk(gen, 1, n, D)[0] for n in lens]
    X, got = sigkernel_amd.pad_paths(paths)
    assert got.tolist() == list(lens)
    if pad is not None:
        for i, n in enumerate(lens):
            X[i, n:] = pad
    return X, paths


def _oracle_pair(p, q, kernel, dyadic, naive):
    if p.shape[0] < 2 or q.shape[0] < 2:
        return 1.0
    return float(O.gram_forward(p[None], q[None], kernel, dyadic, naive)[0, 0])


def _oracle_gram(ps, qs, kernel, dyadic, naive=False):
    return np.array([[_oracle_pair(p, q, kernel, dyadic, naive) for q in qs] for p in ps])


@pytest.mark.parametrize("naive", [False, True])
@pytest.mark.parametrize("dyadic", [0, 1, 2])
@pytest.mark.parametrize("kind", ["linear", "rbf"])
def test_gram_ragged_equals_the_oracle_on_truncated_paths(oracle_backend, kind, dyadic, naive):
    X, ps = _batch(0, LEN_X)
    Y, qs = _batch(1, LEN_Y)
    sk = sigkernel_amd.SigKernel(_kernel(kind), dyadic, _naive_solver=naive)
    K = sk.compute_Gram_ragged(X, Y, LEN_X, LEN_Y)
    assert K.shape == (len(LEN_X), len(LEN_Y)) and K.dtype == X.dtype and K.grad_fn is None
    assert rel_err(K.numpy(), _oracle_gram(ps, qs, _kernel(kind), dyadic, naive)) <= TOL
    assert bool((K[0] == 1).all()) and bool((K[:, 1] == 1).all())          # a one-point path: exactly 1
    # ... and node (len_x - 1, len_y - 1) of the prefix grid at the same padded shape, bit for bit
    grid = sk.compute_Gram_prefixes(X, Y)
    ia, ib = torch.tensor(LEN_X) - 1, torch.tensor(LEN_Y) - 1
    assert torch.equal(K, grid[torch.arange(len(LEN_X))[:, None], torch.arange(len(LEN_Y))[None, :], ia[:, None], ib[None, :]])


@pytest.mark.parametrize("dyadic", [0, 1, 2])
@pytest.mark.parametrize("kind", ["linear", "rbf"])
def test_kernel_ragged_equals_the_oracle_on_truncated_paths(oracle_backend, kind, dyadic):
    lens_y = [3, 5, 1, 5, 2]
    X, ps = _batch(2, LEN_X)
    Y, qs = _batch(3, lens_y)
    sk = sigkernel_amd.SigKernel(_kernel(kind), dyadic)
    k = sk.compute_kernel_ragged(X, Y, torch.tensor(LEN_X), torch.tensor(lens_y, dtype=torch.int32))
    assert k.shape == (len(LEN_X),) and k.dtype == X.dtype
    want = np.array([_oracle_pair(p, q, _kernel(kind), dyadic, False) for p, q in zip(ps, qs)])
    assert rel_err(k.numpy(), want) <= TOL
    assert float(k[0]) == 1.0 and float(k[2]) == 1.0
    grid = sk.compute_kernel_prefixes(X, Y)
    assert torch.equal(k, grid[torch.arange(len(LEN_X)), torch.tensor(LEN_X) - 1, torch.tensor(lens_y) - 1])


@pytest.mark.parametrize("kind", ["linear", "rbf"])
def test_sym_computes_every_pair_and_symmetrises(oracle_backend, kind):
    X, ps = _batch(4, LEN_X)
    sk = sigkernel_amd.SigKernel(_kernel(kind), 1)
    K = sk.compute_Gram_ragged(X, X, LEN_X, LEN_X, sym=True)
    assert torch.equal(K, K.T)
    assert rel_err(K.numpy(), _oracle_gram(ps, ps, _kernel(kind), 1)) <= TOL
    full = sk.compute_Gram_ragged(X, X, LEN_X, LEN_X)
    assert torch.equal(K, 0.5 * (full + full.T))
    with pytest.raises(ValueError, match="Y is X"):
        sk.compute_Gram_ragged(X, X.clone(), LEN_X, LEN_X, sym=True)
    with pytest.raises(ValueError, match="len_y"):
        sk.compute_Gram_ragged(X, X, LEN_X, [1, 2, 6, 4, 5], sym=True)


@pytest.mark.parametrize("gram", [True, False])
def test_a_tiny_workspace_tiles_the_rows_and_changes_nothing(oracle_backend, gram, monkeypatch):
    lens_y = LEN_Y if gram else [3, 5, 1, 5, 2]
    X, _ = _batch(5, LEN_X)
    Y, _ = _batch(6, lens_y)
    be = _lib.get_backend()
    calls = []
    real = type(be).solve_fwd

    def counted(self, *a, **k):
        calls.append(1)
        return real(self, *a, **k)
    monkeypatch.setattr(type(be), "solve_fwd", counted)
    big = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(1.0), 1)
    small = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(1.0), 1, workspace_bytes=1)
    f = (lambda s: s.compute_Gram_ragged(X, Y, LEN_X, lens_y)) if gram else (lambda s: s.compute_kernel_ragged(X, Y, LEN_X, lens_y))
    want = f(big)
    assert len(calls) == 1
    del calls[:]
    got = f(small)
    assert len(calls) == len(LEN_X)           # one row per tile
    assert torch.equal(got, want)


@pytest.mark.parametrize("kind", ["linear", "rbf"])
def test_the_padding_never_reaches_a_result(oracle_backend, kind):
    X, _ = _batch(7, LEN_X)
    Y, _ = _batch(8, LEN_Y)
    X2, _ = _batch(7, LEN_X, pad=1e3)
    Y2, _ = _batch(8, LEN_Y, pad=-7.0)
    sk = sigkernel_amd.SigKernel(_kernel(kind), 1)
    assert torch.equal(sk.compute_Gram_ragged(X, Y, LEN_X, LEN_Y), sk.compute_Gram_ragged(X2, Y2, LEN_X, LEN_Y))
    assert torch.equal(sk.compute_kernel_ragged(X, X, LEN_X, LEN_X), sk.compute_kernel_ragged(X2, X2, LEN_X, LEN_X))


def test_pad_paths_round_trips():
    gen = torch.Generator().manual_seed(9)
    paths = [walk(gen, 1, n, 2, torch.float32)[0] for n in (3, 1, 7, 7, 2)]
    X, lens = sigkernel_amd.pad_paths(paths)
    assert X.shape == (5, 7, 2) and X.dtype == torch.float32 and lens.dtype == torch.int64 and lens.tolist() == [3, 1, 7, 7, 2]
    for i, p in enumerate(paths):
        assert torch.equal(X[i, :lens[i]], p)
        assert bool((X[i, lens[i]:] == p[-1]).all())          # padded by repeating the last point
    assert "pad_paths" in sigkernel_amd.__all__
    with pytest.raises(ValueError):
        sigkernel_amd.pad_paths([])
    with pytest.raises(ValueError):
        sigkernel_amd.pad_paths([paths[0], paths[1][:, :1]])
    with pytest.raises(ValueError):
        sigkernel_amd.pad_paths([paths[0], paths[1][:0]])


def test_lengths_are_checked_on_the_host(oracle_backend):
    X, _ = _batch(10, LEN_X)
    Y, _ = _batch(11, LEN_Y)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.LinearKernel(), 1)
    with pytest.raises(ValueError, match="len_x"):
        sk.compute_Gram_ragged(X, Y, LEN_X[:-1], LEN_Y)                       # a wrong count
    with pytest.raises(ValueError, match="len_y"):
        sk.compute_Gram_ragged(X, Y, LEN_X, LEN_Y + [2])
    with pytest.raises(ValueError, match="len_x"):
        sk.compute_Gram_ragged(X, Y, torch.tensor(LEN_X, dtype=torch.float64), LEN_Y)      # not integers
    with pytest.raises(ValueError, match="len_y"):
        sk.compute_Gram_ragged(X, Y, LEN_X, [5.0, 1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="len_x"):
        sk.compute_Gram_ragged(X, Y, [0, 2, 6, 4, 6], LEN_Y)                  # below 1
    with pytest.raises(ValueError, match="len_y"):
        sk.compute_Gram_ragged(X, Y, LEN_X, [5, 1, 2, 6])                     # beyond the padded length
    with pytest.raises(ValueError, match="len_y"):
        sk.compute_kernel_ragged(X, X, LEN_X, torch.tensor([LEN_X]))          # not one-dimensional
    with pytest.raises(ValueError):
        sk.compute_kernel_ragged(X, Y, LEN_X, LEN_Y)                          # paired: batch sizes differ
    with pytest.raises(ValueError, match="len_x"):
        sk.compute_mmd_ragged(X, [9] * 5, Y, LEN_Y)


def test_forward_only_and_no_process_group(oracle_backend):
    X, _ = _batch(12, LEN_X)
    Y, _ = _batch(13, LEN_Y)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.LinearKernel(), 1)
    Xg = X.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="forward only"):
        sk.compute_Gram_ragged(Xg, Y, LEN_X, LEN_Y)
    with pytest.raises(NotImplementedError, match="forward only"):
        sk.compute_kernel_ragged(X, Xg, LEN_X, LEN_X)
    with pytest.raises(NotImplementedError, match="forward only"):
        sk.compute_mmd_ragged(Xg, LEN_X, Y, LEN_Y)
    with torch.no_grad():
        K = sk.compute_Gram_ragged(Xg, Y, LEN_X, LEN_Y)
    assert K.grad_fn is None and not K.requires_grad and torch.equal(K, sk.compute_Gram_ragged(X, Y, LEN_X, LEN_Y))
    grouped = sigkernel_amd.SigKernel(sigkernel_amd.LinearKernel(), 1, process_group=object())
    with pytest.raises(NotImplementedError, match="process group"):
        grouped.compute_Gram_ragged(X, Y, LEN_X, LEN_Y)
    with pytest.raises(NotImplementedError, match="process group"):
        grouped.compute_kernel_ragged(X, X, LEN_X, LEN_X)
    with pytest.raises(NotImplementedError, match="process group"):
        grouped.compute_mmd_ragged(X, LEN_X, Y, LEN_Y)


def test_trivial_shapes(oracle_backend):
    X, _ = _batch(14, LEN_X)
    Y, _ = _batch(15, LEN_Y)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(0.7), 1)
    assert sk.compute_Gram_ragged(X[:0], Y, [], LEN_Y).shape == (0, len(LEN_Y))
    assert sk.compute_Gram_ragged(X, Y[:0], LEN_X, torch.zeros(0, dtype=torch.int64)).shape == (len(LEN_X), 0)
    assert sk.compute_kernel_ragged(X[:0], X[:0], [], []).shape == (0,)
    one = sk.compute_Gram_ragged(X[:, :1], Y, [1] * len(LEN_X), LEN_Y)           # padded length 1
    assert one.shape == (len(LEN_X), len(LEN_Y)) and bool((one == 1).all())
    k32 = sk.compute_Gram_ragged(X.float(), Y.float(), LEN_X, LEN_Y)
    assert k32.dtype == torch.float32
    np.testing.assert_allclose(k32.numpy(), sk.compute_Gram_ragged(X, Y, LEN_X, LEN_Y).numpy(), rtol=1e-4, atol=1e-5)


def test_function_valued_kernel_goes_through_its_features(oracle_backend):
    gen = torch.Generator().manual_seed(16)
    X = walk(gen, 3, 5, 6).reshape(3, 5, 3, 2)
    Y = walk(gen, 2, 4, 6).reshape(2, 4, 3, 2)
    lx, ly = [5, 2, 3], [4, 3]
    sk = sigkernel_amd.SigKernel(sigkernel_amd.RBF_ID_Kernel(1.0), 1)
    K = sk.compute_Gram_ragged(X, Y, lx, ly)
    for a in range(3):
        for b in range(2):
            want = sk.compute_Gram(X[a:a + 1, :lx[a]], Y[b:b + 1, :ly[b]])
            assert rel_err(K[a:a + 1, b:b + 1].numpy(), want.numpy()) <= TOL, (a, b)


# compute_mmd_ragged with every length full against compute_mmd: the bound of tests/test_prefix_slices_host.py for compute_mmd_prefixes
# (three means of Gram matrices that agree entry by entry to TOL of their largest entry, the factor 2 on K_XY: four such terms)
@pytest.mark.parametrize("dyadic", [0, 1])
@pytest.mark.parametrize("kind", ["linear", "rbf"])
def test_mmd_ragged_with_full_lengths_equals_mmd(oracle_backend, kind, dyadic):
    gen = torch.Generator().manual_seed(17 + dyadic)
    X, Y = walk(gen, 4, 6, D), walk(gen, 5, 7, D)
    sk = sigkernel_amd.SigKernel(_kernel(kind), dyadic)
    got = sk.compute_mmd_ragged(X, [6] * 4, Y, [7] * 5)
    assert got.dim() == 0 and got.grad_fn is None
    kmax = max(float(sk.compute_Gram(Z, W).abs().max()) for Z, W in ((X, X), (Y, Y), (X, Y)))
    assert abs(float(got) - float(sk.compute_mmd(X, Y))) <= 4 * TOL * kmax


@pytest.mark.parametrize("kind", ["linear", "rbf"])
def test_mmd_ragged_is_the_estimator_on_the_truncated_samples(oracle_backend, kind):
    X, ps = _batch(18, LEN_X)
    Y, qs = _batch(19, LEN_Y)
    sk = sigkernel_amd.SigKernel(_kernel(kind), 1)
    got = float(sk.compute_mmd_ragged(X, LEN_X, Y, LEN_Y))
    kxx, kyy, kxy = (_oracle_gram(a, b, _kernel(kind), 1) for a, b in ((ps, ps), (qs, qs), (ps, qs)))
    A, B = len(ps), len(qs)
    want = (kxx.sum() - np.trace(kxx)) / (A * (A - 1.)) + (kyy.sum() - np.trace(kyy)) / (B * (B - 1.)) - 2. * kxy.mean()
    assert abs(got - want) <= 4 * TOL * max(np.abs(kxx).max(), np.abs(kyy).max(), np.abs(kxy).max())


AT_FUNCTIONS = ["sk_solve_prefix_at_%s_%s" % (k, t) for k in ("linear", "rbf") for t in ("f64", "f32")]


def test_header_table_and_library_agree_on_the_new_entry_points():
    """the way tests/test_abi.py does it for the others: declared in the header, in _lib's signature table, exported by the library"""
    import ctypes
    import os
    import re
    from conftest import ROOT
    from sigkernel_amd import build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sigkernel_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sk_[a-z0-9_]+)\s*\(", text))
    lib = ctypes.CDLL(build.build())
    for name in AT_FUNCTIONS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        m = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, text)
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == len(_lib.SIGNATURES[name][1]), name
        assert "const int *len_x" in args and "const int *len_y" in args and not any(a.endswith(" nodes") or a.endswith(" ldo") for a in args)
    assert re.search(r"#define\s+SK_NODES_AT\s+4\b", text)
    assert "at" not in _lib.PREFIX_NODES and sorted(_lib.PREFIX_NODES.values()) == [0, 1, 2, 3]      # the public nodes= keeps its four values
    assert _lib.load().sk_version() == 340       # purely additive


def test_new_entry_points_report_bad_arguments_without_a_device():
    import ctypes
    lib = _lib.load()
    p = ctypes.cast(ctypes.create_string_buffer((8 * 4096) * b"\0"), ctypes.c_void_p).value
    ok = dict(A=1, B=1, Mrows=256, Mc=3, Nc=3, Ncp=16, D=2, dyadic=1, scheme=0)

    def lin(out=p, len_x=p, len_y=p, **kw):
        a = dict(ok, **kw)
        return lib.sk_solve_prefix_at_linear_f64(p, p, a["A"], a["B"], a["Mrows"], a["Mc"], a["Nc"], a["Ncp"], a["D"], a["dyadic"], a["scheme"],
                                                 len_x, len_y, out, None, None)

    def rbf(inv_sigma=1.0, out=p, len_x=p, len_y=p, **kw):
        a = dict(ok, **kw)
        return lib.sk_solve_prefix_at_rbf_f32(p, p, a["A"], a["B"], a["Mrows"], a["Mc"], a["Nc"], a["Ncp"], a["D"], a["dyadic"], a["scheme"],
                                              inv_sigma, len_x, len_y, out, None, None)
    BAD, UNSUPPORTED = 1, 2
    assert lin(len_x=None) == BAD and lin(len_y=None) == BAD and rbf(len_x=None) == BAD and rbf(len_y=None) == BAD
    assert lin(out=None) == BAD and lin(Mc=0) == BAD and lin(D=0) == BAD and lin(scheme=7) == BAD and lin(A=-1) == BAD
    assert rbf(inv_sigma=0.0) == BAD and rbf(inv_sigma=float("nan")) == BAD and rbf(dyadic=-1) == BAD
    assert lin(A=0) == 0 and rbf(A=0) == 0                       # nothing to do: no launch
    assert lin(D=9) == UNSUPPORTED and lin(dyadic=3) == UNSUPPORTED and lin(Mc=300) == UNSUPPORTED and rbf(Mc=128, dyadic=0) == UNSUPPORTED
    # the public slice entry point does not take the mode: it has no lengths
    assert lib.sk_solve_prefix_nodes_linear_f64(p, p, 1, 1, 256, 3, 3, 16, 2, 1, 0, 4, p, 16, None, None) == BAD
