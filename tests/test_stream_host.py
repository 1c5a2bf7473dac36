"""SigKernel.open_stream / SigKernelStream on the host: the oracle-backed back-end has no solve_prefix_resume, so a stream keeps its
history and every append is compute_Gram_prefixes(X, history, nodes="last_row") -- the route every shape outside the fused prefix
kernel's scope takes on the GPU as well.  Exact equality with the one-shot call on the whole stream, the argument checks (raised
before any back-end call), and the C ABI of the resume entry points: header, library and ctypes table agree, the bad-argument
answers come before any HIP call, and sk_prefix_state_pitch covers a bank path's fine rows."""
import ctypes
import os
import re

import pytest
import torch

import sigkernel_amd
from sigkernel_amd import _lib
from conftest import ROOT, walk

A, B, D, M = 3, 2, 3, 5
N0 = [1, 2, 4]
CHUNKS = [[1, 1, 1, 1], [2, 3], [3, 1, 2], [5]]
RESUME = ["sk_solve_prefix_resume_linear_f64", "sk_solve_prefix_resume_linear_f32", "sk_solve_prefix_resume_rbf_f64",
          "sk_solve_prefix_resume_rbf_f32"]


def _kernel(kind):
    return sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(1.0)


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
@pytest.mark.parametrize("dyadic", [0, 1, 2])
@pytest.mark.parametrize("kind", ["linear", "rbf"])
def test_appends_are_the_one_shot_last_row_exactly(oracle_backend, kind, dyadic, naive, paired):
    sk = sigkernel_amd.SigKernel(_kernel(kind), dyadic, _naive_solver=naive)
    nb = A if paired else B
    for n0 in N0:
        for chunks in CHUNKS:
            gen = torch.Generator().manual_seed(100 * n0 + len(chunks))
            X, Yall = walk(gen, A, M, D), walk(gen, nb, n0 + sum(chunks), D)
            whole = (sk.compute_kernel_prefixes if paired else sk.compute_Gram_prefixes)(X, Yall, nodes="last_row")
            st = sk.open_stream(X, Yall[:, :n0], paired=paired)
            assert st.resumes is False and st.length == n0
            got, n = [], n0
            for c in chunks:
                new = st.append(Yall[:, n:n + c])
                n += c
                assert new.shape == ((A, c) if paired else (A, B, c)) and new.dtype == X.dtype and new.grad_fn is None
                assert st.length == n
                now = sk.compute_kernel(X, Yall[:, :n]) if paired else sk.compute_Gram(X, Yall[:, :n])
                assert torch.equal(st.kernel, now), (n0, chunks, n)
                assert st.state_bytes == nb * n * D * 8
                got.append(new)
            assert torch.equal(torch.cat(got, dim=-1), whole[..., n0:]), (n0, chunks)


def test_an_exact_gradient_object_streams_the_same_values(oracle_backend):
    gen = torch.Generator().manual_seed(5)
    X, Y = walk(gen, A, M, D), walk(gen, B, 7, D)
    a = sigkernel_amd.SigKernel(_kernel("rbf"), 1).open_stream(X, Y[:, :2])
    b = sigkernel_amd.SigKernel(_kernel("rbf"), 1, exact_gradient=True).open_stream(X, Y[:, :2])
    assert torch.equal(a.append(Y[:, 2:]), b.append(Y[:, 2:])) and torch.equal(a.kernel, b.kernel)


def test_bad_arguments_are_refused_before_any_back_end_call(no_backend):
    gen = torch.Generator().manual_seed(1)
    X, Y = walk(gen, A, M, D), walk(gen, B, 6, D)
    sk = sigkernel_amd.SigKernel(_kernel("linear"), 1)
    with pytest.raises(NotImplementedError):
        sk.open_stream(X.clone().requires_grad_(True), Y[:, :2])
    with pytest.raises(NotImplementedError):
        sk.open_stream(X, Y[:, :2].clone().requires_grad_(True))
    with pytest.raises(NotImplementedError):
        sigkernel_amd.SigKernel(_kernel("linear"), 1, process_group=object()).open_stream(X, Y[:, :2])
    with pytest.raises(ValueError):
        sk.open_stream(X, Y[:, :0])                              # no point yet
    with pytest.raises(ValueError):
        sk.open_stream(X, Y[:, :2, :2])                          # another path dimension
    with pytest.raises(ValueError):
        sk.open_stream(X, Y[:, :2].float())                      # another dtype
    with pytest.raises(ValueError):
        sk.open_stream(X, Y[:, :2], paired=True)                 # paired needs one stream per bank path


def test_append_checks_its_points_and_an_empty_chunk_is_empty(oracle_backend):
    gen = torch.Generator().manual_seed(2)
    X, Y = walk(gen, A, M, D), walk(gen, B, 6, D)
    sk = sigkernel_amd.SigKernel(_kernel("rbf"), 0)
    for paired in (False, True):
        st = sk.open_stream(X, walk(gen, A, 2, D) if paired else Y[:, :2], paired=paired)
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


def test_function_valued_and_duck_typed_kernels_keep_their_history(oracle_backend):
    gen = torch.Generator().manual_seed(3)
    X, Y = walk(gen, A, M, D), walk(gen, B, 6, D)

    class Duck:
        def batch_kernel(self, X, Y):
            return sigkernel_amd.RBFKernel(0.7).batch_kernel(X, Y)

        def Gram_matrix(self, X, Y):
            return sigkernel_amd.RBFKernel(0.7).Gram_matrix(X, Y)

    sk = sigkernel_amd.SigKernel(Duck(), 1)
    st = sk.open_stream(X, Y[:, :3])
    assert st.resumes is False
    assert torch.equal(st.append(Y[:, 3:]), sk.compute_Gram_prefixes(X, Y, nodes="last_row")[..., 3:])
    assert torch.equal(st.kernel, sk.compute_Gram(X, Y))


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------
def _declared():
    text = open(os.path.join(ROOT, "include", "sigkernel_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return text


def test_header_library_and_ctypes_table_agree_on_the_resume_entry_points():
    from sigkernel_amd import build
    text = _declared()
    lib = ctypes.CDLL(build.build())
    for name in RESUME + ["sk_prefix_state_pitch"]:
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
        assert restype is (ctypes.c_int64 if m.group(1) == "int64_t" else ctypes.c_int)
    # the nodes entry points' arguments with the mode fixed, plus col_in, col_out, their pitch and the state unit
    for kind in ("linear", "rbf"):
        for sfx in ("f64", "f32"):
            nodes = list(_lib.SIGNATURES["sk_solve_prefix_nodes_%s_%s" % (kind, sfx)][1])
            resume = list(_lib.SIGNATURES["sk_solve_prefix_resume_%s_%s" % (kind, sfx)][1])
            at = 11 if kind == "linear" else 12
            assert nodes[at] is ctypes.c_int
            del nodes[at]
            assert resume == nodes[:-2] + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int] + nodes[-2:]
    assert _lib.load().sk_version() == _lib.ABI_VERSION


def test_resume_argument_errors_are_reported_without_a_device():
    lib = _lib.load()
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 20)
    lin = lib.sk_solve_prefix_resume_linear_f64
    # (dXr, dYt, A, B, Mrows, Mc, Nc, Ncp, D, dyadic, scheme, out, ldo, col_in, col_out, ld_col, state_unit, queue, stream)
    ok = dict(A=2, B=3, Mrows=256, Mc=8, Nc=6, Ncp=16, D=3, dyadic=1, scheme=0, ldo=7, ld_col=16, unit=3)

    def call(col_in=q, col_out=p, out=p, **kw):
        a = dict(ok, **kw)
        return lin(p, p, a["A"], a["B"], a["Mrows"], a["Mc"], a["Nc"], a["Ncp"], a["D"], a["dyadic"], a["scheme"], out, a["ldo"], col_in, col_out,
                   a["ld_col"], a["unit"], None, None)

    assert lib.sk_prefix_state_pitch(8, 1, 0) == 16
    assert call(out=None) == 1
    assert call(ldo=6) == 1                                  # the slice does not fit
    assert call(unit=0) == 1 and call(unit=4) == 1           # a state column outside the piece's whole units
    assert call(col_out=None, unit=3) == 1                   # a state unit without a place for the state
    assert call(ld_col=14) == 1 and call(ld_col=17) == 1     # shorter than the fine rows' lanes; odd
    assert call(col_in=ctypes.c_void_p(4096 + 8)) == 1       # not 16-byte aligned
    assert call(col_in=ctypes.c_void_p(4096 + 64)) == 1      # the two arrays overlap
    assert call(dyadic=3) == 2 and call(D=9) == 2            # outside the kernel's scope
    assert call(Mc=200, ld_col=400) == 2                            # more than one band at dyadic 1
    assert lib.sk_solve_prefix_resume_rbf_f32(p, p, 2, 3, 256, 8, 6, 16, 3, 1, 0, 0.0, p, 7, q, p, 16, 3, None, None) == 1   # 1/sigma must be positive
    assert call(A=0) == 0                                    # nothing to do


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("dyadic", [0, 1, 2])
def test_the_state_pitch_covers_the_fine_rows(kind, dyadic):
    lib = _lib.load()
    for m in range(2, 258):
        pitch = lib.sk_prefix_state_pitch(m - 1, dyadic, kind)
        assert pitch >= (m - 1) << dyadic and pitch % 2 == 0, (m, pitch)
        assert pitch - ((m - 1) << dyadic) < 4 << dyadic      # less than one lane of rows more
        assert _lib.HipBackend.state_pitch(kind, m, dyadic) == pitch
    assert lib.sk_prefix_state_pitch(0, dyadic, kind) == 0 and lib.sk_prefix_state_pitch(8, 3, kind) == 0 and lib.sk_prefix_state_pitch(8, dyadic, 2) == 0
