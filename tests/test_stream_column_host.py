"""SigKernel.open_stream(..., resume="always") on the host: the column route's bookkeeping against a test-owned back-end -- the
oracle-backed stand-in plus a plain-numpy solve_fwd_resume with the solver's cell formula, and a static stage whose entries round the
same whatever the second path's length (fake_backend._rowwise_gram), so that a piece's increments have the bits of the whole's
columns, as the HIP static kernels' do.  What is checked: the pieces an append hands over ([last point] + new points, nothing of the
history), the alternation of the two column arrays, row tiling under workspace_bytes, paired and Gram, a first chunk of one point,
state_bytes constant in the stream, `route`; the fallback of a back-end without the call; the refusals before any back-end call; and the
C ABI of the new entry points: header, library and ctypes table agree, sk_version() stays, and every bad-argument / unsupported answer
comes before any HIP call."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import sigkernel_amd
from sigkernel_amd import _lib
from conftest import ROOT, walk
from fake_backend import OracleBackend, _rowwise_gram

A, B, D, M = 3, 2, 3, 5
N0 = [1, 2, 4]
CHUNKS = [[1, 1, 1, 1], [2, 3], [3, 1, 2], [5]]
NEW = ["sk_solve_fwd_resume_f64", "sk_solve_fwd_resume_f32", "sk_solve_fwd_resume_fits"]


def _kernel(kind):
    return sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(1.0)


class ColumnBackend(OracleBackend):
    """the oracle-backed stand-in + solve_fwd_resume; records every resumed launch"""

    def __init__(self):
        self.calls = []      # (pairs of the launch, Mc, Nc, data_ptr of col_in, data_ptr of col_out, first pair's offset in the array)

    def static_increments(self, kind, param, X, Y, gram):
        if gram:
            return self.increments(_rowwise_gram(kind, param, X, Y))
        return torch.stack([self.increments(_rowwise_gram(kind, param, X[a:a + 1], Y[a:a + 1]))[0, 0] for a in range(X.shape[0])])

    def solve_fwd_resume(self, inc_c, dyadic, naive, col_in, col_out):
        Mc, Nc = inc_c.shape[-2:]
        batch = inc_c.shape[:-2]
        inc = inc_c.detach().double().reshape(-1, Mc, Nc).numpy()
        P, MM, NN = inc.shape[0], Mc << dyadic, Nc << dyadic
        assert col_in.dtype == col_out.dtype == torch.float64 and tuple(col_in.shape) == tuple(col_out.shape) == (P, MM + 1)
        assert col_in.is_contiguous() and col_out.is_contiguous()
        lo, hi = sorted((col_in.data_ptr(), col_out.data_ptr()))
        assert hi - lo >= 8 * P * (MM + 1), "col_in and col_out overlap"
        self.calls.append((P, Mc, Nc, col_in.data_ptr(), col_out.data_ptr()))
        cin = col_in.numpy()
        K = np.ones((P, MM + 1, NN + 1))
        K[:, 1:, 0] = cin[:, 1:]                      # element 0 of a slot is never read
        rs = 1.0 / (1 << dyadic)
        for i in range(1, MM + 1):
            for j in range(1, NN + 1):
                g = (inc[:, (i - 1) >> dyadic, (j - 1) >> dyadic] * rs) * rs
                k10, k01, k00 = K[:, i, j - 1], K[:, i - 1, j], K[:, i - 1, j - 1]
                if naive:
                    K[:, i, j] = (k10 + k01) * (1. + 0.5 * g) - k00
                else:
                    K[:, i, j] = (k10 + k01) * ((1. + 0.5 * g) + (1. / 12.) * (g * g)) - k00 * (1. - (1. / 12.) * (g * g))
        col_out[:, 1:] = torch.from_numpy(K[:, 1:, NN].copy())      # element 0 stays the caller's
        row = torch.full((P, NN + 1), float("nan"), dtype=torch.float64)
        row[:, 1:] = torch.from_numpy(K[:, MM, 1:].copy())
        return row.reshape(batch + (NN + 1,))


@pytest.fixture
def column_backend():
    be = ColumnBackend()
    prev = _lib.set_backend(be)
    yield be
    _lib.set_backend(prev)


class _NoBackend:
    """a back-end that fails the test when anything is asked of it"""
    name = "none"

    def __getattr__(self, what):
        raise AssertionError("back-end call: " + what)


@pytest.fixture
def no_backend():
    prev = _lib.set_backend(_NoBackend())
    yield
    _lib.set_backend(prev)


@pytest.mark.parametrize("paired", [False, True], ids=["gram", "paired"])
@pytest.mark.parametrize("naive", [False, True])
@pytest.mark.parametrize("dyadic", [0, 1, 3])
@pytest.mark.parametrize("kind", ["linear", "rbf"])
def test_appends_are_the_one_shot_last_row_exactly(column_backend, kind, dyadic, naive, paired):
    sk = sigkernel_amd.SigKernel(_kernel(kind), dyadic, _naive_solver=naive)
    nb = A if paired else B
    pairs = A if paired else A * B
    fixed = 2 * pairs * (((M - 1) << dyadic) + 1) * 8 + A * M * D * 8 + nb * D * 8      # two columns, the bank, the kept point
    for n0 in N0:
        for chunks in CHUNKS:
            gen = torch.Generator().manual_seed(100 * n0 + len(chunks))
            X, Yall = walk(gen, A, M, D), walk(gen, nb, n0 + sum(chunks), D)
            whole = (sk.compute_kernel_prefixes if paired else sk.compute_Gram_prefixes)(X, Yall, nodes="last_row")
            del column_backend.calls[:]
            st = sk.open_stream(X, Yall[:, :n0], paired=paired, resume="always")
            assert st.route == "column" and st.resumes is True and st.length == n0 and st.state_bytes == fixed
            # a first chunk of one point sweeps nothing
            assert [c[2] for c in column_backend.calls] == ([] if n0 == 1 else [n0 - 1])
            got, n = [], n0
            for c in chunks:
                before = len(column_backend.calls)
                new = st.append(Yall[:, n:n + c])
                n += c
                assert new.shape == ((A, c) if paired else (A, B, c)) and new.dtype == X.dtype and new.grad_fn is None
                assert st.length == n and st.state_bytes == fixed
                # one launch over all the pairs, of exactly the c new columns: nothing of the history is swept again
                assert [(k[0], k[1], k[2]) for k in column_backend.calls[before:]] == [(pairs, M - 1, c)]
                now = sk.compute_kernel(X, Yall[:, :n]) if paired else sk.compute_Gram(X, Yall[:, :n])
                assert torch.equal(st.kernel, now), (n0, chunks, n)
                got.append(new)
            assert torch.equal(torch.cat(got, dim=-1), whole[..., n0:]), (n0, chunks)
            # the two arrays alternate: every launch reads what the one before wrote
            calls = column_backend.calls
            assert len({k[3] for k in calls} | {k[4] for k in calls}) == 2
            for prev, nxt in zip(calls, calls[1:]):
                assert nxt[3] == prev[4] and nxt[4] == prev[3]


def test_the_first_chunk_returns_the_ones_and_the_swept_nodes(column_backend):
    gen = torch.Generator().manual_seed(11)
    X, Y = walk(gen, A, M, D), walk(gen, B, 6, D)
    sk = sigkernel_amd.SigKernel(_kernel("rbf"), 1)
    one = sk.open_stream(X, Y[:, :1], resume="always")
    assert torch.equal(one.kernel, torch.ones(A, B, dtype=X.dtype)) and not column_backend.calls
    st = sk.open_stream(X, Y[:, :4], resume="always")
    assert torch.equal(st.kernel, sk.compute_Gram(X, Y[:, :4]))
    assert torch.equal(one.append(Y[:, 1:4]), sk.compute_Gram_prefixes(X, Y[:, :4], nodes="last_row")[..., 1:])
    assert torch.equal(one.kernel, st.kernel)


def test_row_tiles_under_a_small_workspace_slice_the_columns(column_backend):
    gen = torch.Generator().manual_seed(12)
    X, Y = walk(gen, A, M, D), walk(gen, B, 7, D)
    big = sigkernel_amd.SigKernel(_kernel("linear"), 1)
    small = sigkernel_amd.SigKernel(_kernel("linear"), 1, workspace_bytes=1)      # one bank path per tile
    whole = big.compute_Gram_prefixes(X, Y, nodes="last_row")
    st = small.open_stream(X, Y[:, :2], resume="always")
    del column_backend.calls[:]
    got = st.append(Y[:, 2:])
    assert torch.equal(got, whole[..., 2:]) and torch.equal(st.kernel, whole[..., -1])
    calls = column_backend.calls
    assert [(k[0], k[2]) for k in calls] == [(B, 5)] * A
    stride = B * (((M - 1) << 1) + 1) * 8      # a tile's slice of either array starts where the tile before ended
    assert [k[3] - calls[0][3] for k in calls] == [a * stride for a in range(A)]
    assert [k[4] - calls[0][4] for k in calls] == [a * stride for a in range(A)]
    # paired: the tile's own streams
    Yp = walk(gen, A, 7, D)
    sp = small.open_stream(X, Yp[:, :3], paired=True, resume="always")
    assert torch.equal(sp.append(Yp[:, 3:]), big.compute_kernel_prefixes(X, Yp, nodes="last_row")[..., 3:])


def test_duck_typed_and_function_valued_kernels_take_the_column_route(column_backend):
    gen = torch.Generator().manual_seed(3)
    X, Y = walk(gen, A, M, D), walk(gen, B, 6, D)

    class Duck:
        def batch_kernel(self, X, Y):
            return sigkernel_amd.RBFKernel(0.7).batch_kernel(X, Y)

        def Gram_matrix(self, X, Y):
            return sigkernel_amd.RBFKernel(0.7).Gram_matrix(X, Y)

    sk = sigkernel_amd.SigKernel(Duck(), 1)
    st = sk.open_stream(X, Y[:, :3], resume="always")
    assert st.route == "column" and st.resumes is True
    new, want = st.append(Y[:, 3:]), sk.compute_Gram_prefixes(X, Y, nodes="last_row")[..., 3:]
    # the Gram of a piece is another torch matmul than the Gram of the whole: the project's bar for values that do not share bits
    assert bool(((new - want).abs() <= 1e-12 * want.abs().clamp_min(1.0)).all())
    # function-valued paths (batch, T, Lx, d): the bank mapped once, every piece as it arrives
    Xf, Yf = X.reshape(A, M, 3, 1).expand(A, M, 3, 2).contiguous(), Y.reshape(B, 6, 3, 1).expand(B, 6, 3, 2).contiguous()
    skf = sigkernel_amd.SigKernel(sigkernel_amd.RBF_ID_Kernel(0.9), 1)
    sf = skf.open_stream(Xf, Yf[:, :2], resume="always")
    assert sf.route == "column"
    fixed = sf.state_bytes
    assert torch.equal(sf.append(Yf[:, 2:5]), skf.compute_Gram_prefixes(Xf, Yf[:, :5], nodes="last_row")[..., 2:])
    assert torch.equal(sf.append(Yf[:, 5:]), skf.compute_Gram_prefixes(Xf, Yf, nodes="last_row")[..., 5:])
    assert torch.equal(sf.kernel, skf.compute_Gram(Xf, Yf)) and sf.state_bytes == fixed
    with pytest.raises(ValueError):
        sf.append(Y[:, :1])      # points of the feature shape are not points of the paths


def test_the_default_and_a_back_end_without_the_call_keep_the_history(column_backend, oracle_backend):
    # (oracle_backend, installed last, is the back-end here: it has no solve_fwd_resume)
    gen = torch.Generator().manual_seed(4)
    X, Y = walk(gen, A, M, D), walk(gen, B, 6, D)
    sk = sigkernel_amd.SigKernel(_kernel("rbf"), 1)
    want = sk.compute_Gram_prefixes(X, Y, nodes="last_row")[..., 2:]
    st = sk.open_stream(X, Y[:, :2], resume="always")
    assert st.route == "history" and st.resumes is False
    assert torch.equal(st.append(Y[:, 2:]), want) and st.state_bytes == B * 6 * D * 8
    _lib.set_backend(column_backend)
    dflt = sk.open_stream(X, Y[:, :2])
    assert dflt.route == "history" and dflt.resumes is False and not column_backend.calls
    assert torch.equal(dflt.append(Y[:, 2:]), want) and dflt.state_bytes == B * 6 * D * 8
    assert torch.equal(sk.open_stream(X, Y[:, :2], resume="fused").append(Y[:, 2:]), want) and not column_backend.calls
    col = sk.open_stream(X, Y[:, :2], resume="always")
    assert col.route == "column" and torch.equal(col.append(Y[:, 2:]), want)


def test_a_bank_beyond_the_limit_keeps_its_history(column_backend):
    column_backend.resume_fits = lambda M, dyadic: False
    gen = torch.Generator().manual_seed(6)
    X, Y = walk(gen, A, M, D), walk(gen, B, 4, D)
    st = sigkernel_amd.SigKernel(_kernel("linear"), 0).open_stream(X, Y[:, :2], resume="always")
    assert st.route == "history" and st.resumes is False and not column_backend.calls


def test_bad_arguments_are_refused_before_any_back_end_call(no_backend):
    gen = torch.Generator().manual_seed(1)
    X, Y = walk(gen, A, M, D), walk(gen, B, 6, D)
    sk = sigkernel_amd.SigKernel(_kernel("linear"), 1)
    for bad in ("column", "never", "", None, True):
        with pytest.raises(ValueError):
            sk.open_stream(X, Y[:, :2], resume=bad)
    with pytest.raises(NotImplementedError):
        sk.open_stream(X.clone().requires_grad_(True), Y[:, :2], resume="always")
    with pytest.raises(NotImplementedError):
        sk.open_stream(X, Y[:, :2].clone().requires_grad_(True), resume="always")
    with pytest.raises(NotImplementedError):
        sigkernel_amd.SigKernel(_kernel("linear"), 1, process_group=object()).open_stream(X, Y[:, :2], resume="always")
    with pytest.raises(ValueError):
        sk.open_stream(X, Y[:, :0], resume="always")                              # no point yet
    with pytest.raises(ValueError):
        sk.open_stream(X, Y[:, :2, :2], resume="always")                          # another path dimension
    with pytest.raises(ValueError):
        sk.open_stream(X, Y[:, :2].float(), resume="always")                      # another dtype
    with pytest.raises(ValueError):
        sk.open_stream(X, Y[:, :2], paired=True, resume="always")                 # paired needs one stream per bank path


def test_append_checks_its_points_and_an_empty_chunk_is_empty(column_backend):
    gen = torch.Generator().manual_seed(2)
    X, Y = walk(gen, A, M, D), walk(gen, B, 6, D)
    sk = sigkernel_amd.SigKernel(_kernel("rbf"), 0)
    for paired in (False, True):
        st = sk.open_stream(X, walk(gen, A, 2, D) if paired else Y[:, :2], paired=paired, resume="always")
        assert st.route == "column"
        nb = A if paired else B
        good = walk(gen, nb, 3, D)
        prev = _lib.set_backend(_NoBackend())
        try:
            empty = st.append(good[:, :0])
            assert empty.shape == ((A, 0) if paired else (A, B, 0)) and empty.dtype == X.dtype and st.length == 2
            for bad in (good.float(), good[:, :, :2], good[:1], good[0], good.to("meta")):
                with pytest.raises(ValueError):
                    st.append(bad)
            with pytest.raises(NotImplementedError):
                st.append(good.clone().requires_grad_(True))
            assert st.length == 2
        finally:
            _lib.set_backend(prev)
        assert st.append(good).shape[-1] == 3 and st.length == 5


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_ctypes_table_agree_on_the_new_entry_points():
    from sigkernel_amd import build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sigkernel_amd.h")).read(), flags=re.S)
    lib = ctypes.CDLL(build.build())
    for name in NEW:
        m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, "not declared: " + name
        assert hasattr(lib, name), "missing export: " + name
        restype, argtypes = _lib.SIGNATURES[name]
        args = [a.strip() for a in m.group(2).split(",")]
        assert len(args) == len(argtypes), (name, args)
        for a, t in zip(args, argtypes):
            want = ctypes.c_void_p if "*" in a else ctypes.c_int64 if a.startswith("int64_t") else ctypes.c_double if a.startswith("double") \
                else ctypes.c_int
            assert t is want, (name, a, t)
        assert restype is ctypes.c_int and m.group(1) == "int"
    assert _lib.SIGNATURES["sk_solve_fwd_resume_f64"] == _lib.SIGNATURES["sk_solve_fwd_resume_f32"]
    assert _lib.load().sk_version() == _lib.ABI_VERSION == 340


def test_argument_errors_and_the_limit_are_reported_without_a_device():
    lib = _lib.load()
    p, q, r = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 24)
    ok = dict(ld=6, P=5, Mc=8, Nc=6, dyadic=1, scheme=0)
    BAD, UNSUPPORTED = 1, 2

    def call(fn=lib.sk_solve_fwd_resume_f64, inc=p, col_in=q, col_out=r, row=p, **kw):
        a = dict(ok, **kw)
        return fn(inc, a["ld"], a["P"], a["Mc"], a["Nc"], a["dyadic"], a["scheme"], col_in, col_out, row, None)

    for fn in (lib.sk_solve_fwd_resume_f64, lib.sk_solve_fwd_resume_f32):
        assert call(fn, col_in=None) == BAD and call(fn, col_out=None) == BAD and call(fn, row=None) == BAD and call(fn, inc=None) == BAD
        assert call(fn, Nc=0) == BAD and call(fn, Nc=-1) == BAD and call(fn, Mc=0) == BAD and call(fn, P=-1) == BAD
        assert call(fn, ld=5) == BAD and call(fn, dyadic=-1) == BAD and call(fn, scheme=7) == BAD
        slot = 5 * ((8 << 1) + 1) * 8      # bytes of either array
        assert call(fn, col_out=q) == BAD                                                  # the same array
        assert call(fn, col_out=ctypes.c_void_p((1 << 20) + slot - 8)) == BAD              # its last element
        assert call(fn, col_out=ctypes.c_void_p((1 << 20) - slot + 8)) == BAD
        assert call(fn, col_in=ctypes.c_void_p((1 << 20) + 4)) == BAD                      # not a double's address
        # beyond the LDS limit: 3 * 8 * (MM + 1) bytes within 160 KiB, MM + 1 <= 6826
        assert call(fn, Mc=6826, dyadic=0) == UNSUPPORTED and call(fn, Mc=3413, dyadic=1) == UNSUPPORTED
        assert call(fn, P=0) == 0 and call(fn, P=0, Mc=6825, dyadic=0) == 0      # nothing to do
    assert lib.sk_solve_fwd_resume_fits(6825, 0) == 1 and lib.sk_solve_fwd_resume_fits(6826, 0) == 0
    assert lib.sk_solve_fwd_resume_fits(3412, 1) == 1 and lib.sk_solve_fwd_resume_fits(3413, 1) == 0
    assert lib.sk_solve_fwd_resume_fits(426, 4) == 1 and lib.sk_solve_fwd_resume_fits(427, 4) == 0
    assert lib.sk_solve_fwd_resume_fits(0, 0) == 0 and lib.sk_solve_fwd_resume_fits(8, -1) == 0
    assert _lib.HipBackend.resume_fits(6826, 0) is True and _lib.HipBackend.resume_fits(6827, 0) is False and _lib.HipBackend.resume_fits(1, 0) is False
