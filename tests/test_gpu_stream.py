"""SigKernel.open_stream on the GPU: a bank of complete paths against streams that grow.

Inside the fused prefix kernel's scope an append is ONE launch of k_fwd_prefix in its resume mode (csrc/sk_wave_prefix.hip, RESUME): the
sweep starts from the fine column the stream kept and repeats, cell for cell, what a sweep of the whole history does there -- so every
value is torch.equal to the one-shot compute_Gram_prefixes(X, all of y, nodes="last_row"), fp32 streams included (the state is fp64),
and comes from the kernel instance the one-shot call launches (sk_launch_trace).  Outside the scope the stream keeps its history.
The launches that existed before the resume mode went in are held to the parent commit's bits (tests/golden/stream_resume_parent.npz,
recorded on an MI355X by tests/golden/make_golden_stream_resume_parent.py).  No test provokes a fault: bad arguments are refused on the
host and tested there (tests/test_stream_host.py)."""
import os

import numpy as np
import pytest
import torch

import sigkernel_amd
from sigkernel_amd import _lib
from conftest import walk
import stream_resume_parent as parent

pytestmark = pytest.mark.gpu

DEV = "cuda"
KINDS = ["linear", "rbf"]
# (A, B, M, D): rows that do not fill the lanes, an A that is no multiple of the lane groups, the two-point bank path
BANKS = [(3, 5, 9, 3), (5, 3, 33, 8), (6, 6, 64, 4), (7, 2, 2, 1)]
N0 = [1, 2]
# states that do not advance, two odd launches in a row, even and odd tails
CHUNKS = [[1, 1, 1, 1, 1], [2, 2], [3, 3], [1, 16, 1], [7, 9, 2]]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stream_resume_parent.npz")


def _kernel(kind):
    return sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(1.0)


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


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("naive", [False, True])
@pytest.mark.parametrize("dyadic", [0, 1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_appends_are_the_one_shot_sweep_bit_for_bit_from_the_same_instance(kind, dyadic, naive, dtype):
    sk = sigkernel_amd.SigKernel(_kernel(kind), dyadic, _naive_solver=naive)
    longest = max(N0) + max(sum(c) for c in CHUNKS)
    for A, B, M, D in BANKS:
        gen = torch.Generator().manual_seed(1000 * M + D)
        X = walk(gen, A, M, D, dtype).to(DEV)
        for gram in (True, False):
            Ylong = walk(gen, B if gram else A, longest, D, dtype).to(DEV)
            last_row = sk.compute_Gram_prefixes if gram else sk.compute_kernel_prefixes
            final = sk.compute_Gram if gram else sk.compute_kernel
            whole = {}       # total length -> (one-shot last row, its instance, one-shot kernel): computed once, shared
            for n0 in N0:
                for chunks in CHUNKS:
                    total = n0 + sum(chunks)
                    where = (kind, dyadic, naive, dtype, (A, B, M, D), gram, n0, chunks)
                    assert _is_fused(kind, D, M, total, dyadic, naive, 8 if dtype == torch.float64 else 4), where
                    Yall = Ylong[:, :total].contiguous()
                    if total not in whole:
                        row, inst, simple = _traced(lambda: last_row(X, Yall, nodes="last_row"))
                        assert len(inst) == 1 and sum(inst.values()) == 1 and simple == 0, (where, inst, simple)
                        whole[total] = (row, inst, final(X, Yall))
                    want, inst_all, k_all = whole[total]
                    st = sk.open_stream(X, Yall[:, :n0], paired=not gram)
                    assert st.resumes is True and st.length == n0, where
                    held = st.state_bytes
                    got, n = [], n0
                    for c in chunks:
                        new, inst, simple = _traced(lambda: st.append(Yall[:, n:n + c]))
                        n += c
                        assert new.shape == ((A, B) if gram else (A,)) + (c,) and new.dtype == dtype and new.grad_fn is None, where
                        assert inst == inst_all and simple == 0, (where, c, inst, inst_all, simple)
                        assert st.length == n
                        got.append(new)
                    got = torch.cat(got, dim=-1)
                    assert torch.equal(got, want[..., n0:]), (where, float((got.double() - want[..., n0:].double()).abs().max()))
                    assert torch.equal(st.kernel, k_all), where
                    # constant in the stream's length: the two columns, the staged bank, one or two kept points
                    assert abs(st.state_bytes - held) <= (B if gram else A) * D * X.element_size(), where


def test_big_batches_draw_from_the_work_queue():
    """Enough pairs to fill the chip (a first share dealt out, the rest drawn from the counter), odd batch sizes in the shared-y order:
    every pair's state and every pair's values land in their own places."""
    A, B, M, D = 301, 203, 17, 2
    gen = torch.Generator().manual_seed(3)
    sk = sigkernel_amd.SigKernel(_kernel("linear"), 1)
    X, Y = walk(gen, A, M, D).to(DEV), walk(gen, B, 12, D).to(DEV)
    st = sk.open_stream(X, Y[:, :1])
    assert st.resumes
    got = torch.cat([st.append(Y[:, 1:7]), st.append(Y[:, 7:12])], dim=-1)
    assert torch.equal(got, sk.compute_Gram_prefixes(X, Y, nodes="last_row")[..., 1:])
    assert torch.equal(st.kernel, sk.compute_Gram(X, Y))
    sk = sigkernel_amd.SigKernel(_kernel("rbf"), 1)
    Xp, Yp = walk(gen, 40000, M, D).to(DEV), walk(gen, 40000, 12, D).to(DEV)
    st = sk.open_stream(Xp, Yp[:, :1], paired=True)
    got = torch.cat([st.append(Yp[:, 1:7]), st.append(Yp[:, 7:12])], dim=-1)
    assert torch.equal(got, sk.compute_kernel_prefixes(Xp, Yp, nodes="last_row")[..., 1:])
    assert torch.equal(st.kernel, sk.compute_kernel(Xp, Yp))


def _bits(t):
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kind", KINDS)
def test_no_stray_stores_and_nothing_read_that_was_not_written(kind, dtype):
    """`out` in slots with NaNs around them and col_out inside a guard band: a launch writes elements 1 .. n - 1 of every pair's slice and
    the Mc << dyadic fine rows of every pair's column, nothing else; then every element of col_in the header calls the caller's (a slot's
    tail past the fine rows) is set to NaN and the next launch -- output and column -- does not change a bit."""
    be = _lib.get_backend()
    k, param = (0, 1.0) if kind == "linear" else (1, 1.0)
    for dyadic, (A, B, M, D) in [(0, (3, 5, 9, 3)), (1, (3, 5, 12, 3)), (2, (5, 3, 31, 3)), (1, (3, 5, 2, 3)), (0, (2, 3, 6, 2))]:
        gen = torch.Generator().manual_seed(11)
        X = walk(gen, A, M, D, dtype).to(DEV)
        pitch, fine = be.state_pitch(k, M, dyadic), (M - 1) << dyadic
        for gram in (True, False):
            P = A * B if gram else A
            Y = walk(gen, B if gram else A, 11, D, dtype).to(DEV)
            guard = 4096

            def column():
                big = torch.full((guard + P * pitch + guard,), float("nan"), dtype=torch.float64, device=DEV)
                return big, big[guard:guard + P * pitch].view(P, pitch)

            def launch(piece, col_in, col_out):
                n = piece.shape[1]
                slot, lead = n + 5, 3
                shape, strides = ((A, B, n), (B * slot, slot, 1)) if gram else ((A, n), (slot, 1))
                big = torch.full((guard + P * slot + guard,), float("nan"), dtype=dtype, device=DEV)
                view = big[guard + lead:guard + lead + P * slot].as_strided(shape, strides)
                res = be.solve_prefix_resume(k, param, X, piece, dyadic, False, gram, col_in, col_out, out=view)
                torch.cuda.synchronize()
                assert res is not None and res[0].data_ptr() == view.data_ptr()
                written = torch.zeros_like(big, dtype=torch.bool)
                written[guard + lead:guard + lead + P * slot].as_strided(shape, strides)[..., 1:] = True
                assert bool(torch.isnan(big[~written]).all()) and bool(torch.isfinite(big[written]).all())
                return view, res[1]

            # a first launch over 6 points: state behind column 4
            big1, col1 = column()
            out1, adv1 = launch(Y[:, :6].contiguous(), None, col1)
            assert adv1 == 4
            kept = torch.zeros_like(big1, dtype=torch.bool)
            kept[guard:guard + P * pitch].view(P, pitch)[:, :fine] = True
            assert bool(torch.isnan(big1[~kept]).all()) and bool(torch.isfinite(big1[kept]).all())
            # resumed over points 4 .. 10, twice: the caller's elements of col_in as they are (NaN already), then the same with the
            # fine rows copied into a column whose every other element is NaN of another bit pattern
            big2, col2 = column()
            out2, adv2 = launch(Y[:, 4:].contiguous(), col1, col2)
            assert adv2 == 6
            assert bool(torch.isnan(big2[~kept]).all()) and bool(torch.isfinite(big2[kept]).all())
            other = torch.full_like(col1, float("nan")).neg_()
            other[:, :fine] = col1[:, :fine]
            big3, col3 = column()
            out3, _ = launch(Y[:, 4:].contiguous(), other, col3)
            assert torch.equal(_bits(out3[..., 1:]), _bits(out2[..., 1:])) and torch.equal(_bits(big3), _bits(big2))
            # and they are the one-shot values
            want = be.solve_prefix_fused(k, param, X, Y, dyadic, False, gram, nodes="last_row")
            assert torch.equal(out1[..., 1:], want[..., 1:6]) and torch.equal(out2[..., 1:], want[..., 5:])


@pytest.mark.parametrize("kind", KINDS)
def test_outside_the_fused_scope_the_stream_keeps_its_history(kind):
    gen = torch.Generator().manual_seed(5)
    wall = 2
    while _is_fused(kind, 3, wall + 1, 8, 1):
        wall += 1                                   # the longest bank path of one band at dyadic 1
    assert 32 <= wall <= 256
    for A, B, M, D in [(3, 4, 20, 9), (2, 3, wall + 1, 3)]:      # dim 9; a bank path one past the band
        assert not _is_fused(kind, D, M, 8, 1)
        X, Y = walk(gen, A, M, D).to(DEV), walk(gen, B, 8, D).to(DEV)
        sk = sigkernel_amd.SigKernel(_kernel(kind), 1)
        st = sk.open_stream(X, Y[:, :2])
        assert st.resumes is False and st.state_bytes == B * 2 * D * 8
        got = [st.append(Y[:, 2:5])]
        assert st.state_bytes == B * 5 * D * 8
        got.append(st.append(Y[:, 5:]))
        assert st.state_bytes == B * 8 * D * 8 and st.length == 8
        assert torch.equal(torch.cat(got, dim=-1), sk.compute_Gram_prefixes(X, Y, nodes="last_row")[..., 2:])
        assert torch.equal(st.kernel, sk.compute_Gram_prefixes(X, Y, nodes="last_row")[..., -1])
    # the route switch takes a shape inside the scope there too
    X, Y = walk(gen, 3, 9, 3).to(DEV), walk(gen, 2, 8, 3).to(DEV)
    sk = sigkernel_amd.SigKernel(_kernel(kind), 1)
    sigkernel_amd.routes.no_fused_prefix = True
    try:
        off = sk.open_stream(X, Y[:, :2])
        assert off.resumes is False
        slow = off.append(Y[:, 2:])
    finally:
        sigkernel_amd.routes.no_fused_prefix = False
    on = sk.open_stream(X, Y[:, :2])
    assert on.resumes is True and slow.shape == (3, 2, 6)
    assert torch.equal(on.append(Y[:, 2:]), sk.compute_Gram_prefixes(X, Y, nodes="last_row")[..., 2:])


def test_the_launches_that_existed_are_what_they_were():
    """The full grid, the three slices and compute_Gram_ragged of k_fwd_prefix against the parent commit's bits."""
    gold = dict(np.load(GOLDEN, allow_pickle=False))
    got = parent.record(sigkernel_amd)
    assert sorted(got) == sorted(gold)
    differ = [k for k in sorted(got) if not (got[k].shape == gold[k].shape and torch.equal(torch.from_numpy(got[k]), torch.from_numpy(gold[k])))]
    assert not differ, differ
