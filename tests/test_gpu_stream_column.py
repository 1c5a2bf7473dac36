"""SigKernel.open_stream(..., resume="always") OFF the fused prefix kernel's scope, on the GPU: the column route.

Off the scope a stream's values come from the anti-diagonal solver (k_fwd_simple, csrc/sk_simple.hip).  Its RESUME mode
(sk_solve_fwd_resume_*) sweeps a piece of a pair's grid from a kept fine column, every cell from the same operands in the same order as
the one-shot sweep of the whole grid -- so the back-end tests ask for torch.equal with the grid solve_fwd(want_grid=True) stores, for
every row piece and for the last column, and the API tests for torch.equal with compute_Gram_prefixes(X, all of y, nodes="last_row")
wherever the static stage is a HIP kernel: sk_static_increments_* computes an increment (p, q) from x[p], x[p + 1], y[q], y[q + 1] alone,
in an order that does not depend on the second path's length (k_static_linear / _mfma: one fma chain or one MFMA chain over the dims
per entry; k_static_nodes / k_static_wide_mfma: one node value per (row, column), then ((G11 + G00) - G10) - G01), so a piece's increments
have the bits of the whole's columns.  No route was found whose increments depend on the second path's length.  A duck-typed kernel's
Gram_matrix is a torch matmul, which may round a piece differently from the whole: fp64 within 1e-12 max(1, |value|), the project's bar
for forward values that do not share bits (tests/test_gpu_parity.py).

A function-valued kernel (RBF_ID_Kernel, ...) is its base kernel on the features, in the one-shot call as in the stream: (4, 2)-valued
points have 8 features, INSIDE the fused scope, where the one-shot values are the fused prefix kernel's and the anti-diagonal solver's
differ from them by 4.9e-15 (measured on the column route before the stream of features was built); such a stream takes the fused
resume and keeps the bits (ROUTE below).  (5, 2)-valued points, 10 features, take the column route.

`st.kernel` is the last node of the last row, so it is compared bit for bit with that node of the one-shot last row.  compute_Gram off
the fused scope is served by other solvers (the streaming and multi-band kernels), whose values agree with the anti-diagonal solver's
at the bar above and not to the bit (as tests/test_gpu_stream.py's history-route test already has it): st.kernel is held to
compute_Gram at that bar in fp64.

No test provokes a fault: bad arguments are refused on the host before any launch (tests/test_stream_column_host.py, and the overlap
test here, which launches nothing)."""
import ctypes

import pytest
import torch

import sigkernel_amd
from sigkernel_amd import _lib
from conftest import walk

pytestmark = pytest.mark.gpu

DEV = "cuda"
N0 = [1, 2, 5]
CHUNKS = [(1, 1, 3), (2, 4), (6,)]


def _bits(t):
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def _increments(P, Mc, Nc, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    return (0.05 * torch.randn(P, Mc, Nc, generator=gen, dtype=torch.float64)).to(dtype).to(DEV)


def _resumed(be, inc, dyadic, naive, cuts):
    """the resumed launches over the column cuts, from a column of ones -> (the row pieces' coarse nodes, the last col_out)"""
    P, Mc = inc.shape[0], inc.shape[1]
    MM, r = Mc << dyadic, 1 << dyadic
    cols = [torch.ones(P, MM + 1, dtype=torch.float64, device=DEV), torch.full((P, MM + 1), float("nan"), dtype=torch.float64, device=DEV)]
    cur, j0, pieces = 0, 0, []
    for c in cuts:
        row = be.solve_fwd_resume(inc[:, :, j0:j0 + c], dyadic, naive, cols[cur], cols[1 - cur])
        assert row.shape == (P, (c << dyadic) + 1) and row.dtype == torch.float64
        pieces.append(row[:, r::r])
        cur, j0 = 1 - cur, j0 + c
    return pieces, cols[cur]


# ---- the back-end: sk_solve_fwd_resume_* against the stored grid -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("naive", [False, True])
@pytest.mark.parametrize("Mc,dyadic", [(1, 0), (3, 1), (33, 1), (5, 4)])
def test_resumed_pieces_are_the_stored_grid_bit_for_bit(Mc, dyadic, naive, dtype):
    be = _lib.get_backend()
    P, Nc, r = 5, 9, 1 << dyadic
    inc = _increments(P, Mc, Nc, dtype, 7 * Mc + dyadic)
    _, grid, _ = be.solve_fwd(inc, dyadic, naive, want_grid=True)
    for cuts in ([1, 1, 2, 5], [9]):
        pieces, col = _resumed(be, inc, dyadic, naive, cuts)
        j0 = 0
        for c, piece in zip(cuts, pieces):
            cols = torch.arange(j0 + 1, j0 + c + 1, device=DEV) * r
            want = grid[:, -1, cols]
            assert torch.equal(_bits(piece.to(dtype)), _bits(want)), (cuts, j0, float((piece - want.double()).abs().max()))
            j0 += c
        assert torch.equal(_bits(col[:, 1:].to(dtype)), _bits(grid[:, 1:, -1])), cuts


def test_more_pairs_than_blocks_stride_over_the_grid():
    be = _lib.get_backend()
    P, Mc, dyadic = 4100, 2, 1
    inc = _increments(P, Mc, 2, torch.float64, 3)
    _, grid, _ = be.solve_fwd(inc, dyadic, False, want_grid=True)
    pieces, col = _resumed(be, inc, dyadic, False, [1, 1])
    assert torch.equal(pieces[0][:, 0], grid[:, -1, 2]) and torch.equal(pieces[1][:, 0], grid[:, -1, 4])
    assert torch.equal(col[:, 1:], grid[:, 1:, -1])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_no_stray_stores_and_nothing_read_that_was_not_written(dtype):
    """col_out and the row output prefilled with NaN inside a NaN guard band, col_in's element 0 NaN: a launch writes elements 1 .. MM of
    every pair's column and 1 .. NN of every pair's row, all finite, and nothing else; they are the stored grid's."""
    lib = _lib.load()
    fn = getattr(lib, "sk_solve_fwd_resume_" + ("f64" if dtype == torch.float64 else "f32"))
    guard = 4096
    for P, Mc, Nc, dyadic in [(5, 3, 4, 1), (7, 33, 1, 1), (3, 1, 2, 0), (300, 2, 3, 2)]:
        MM, NN = Mc << dyadic, Nc << dyadic
        inc = _increments(P, Mc, 2 * Nc, dtype, 5)
        _, grid, _ = _lib.get_backend().solve_fwd(inc, dyadic, False, want_grid=True)

        def guarded(width):
            big = torch.full((guard + P * width + guard,), float("nan"), dtype=torch.float64, device=DEV)
            return big, big[guard:guard + P * width].view(P, width)

        col_in = torch.ones(P, MM + 1, dtype=torch.float64, device=DEV)
        for j0 in (0, Nc):
            col_in[:, 0] = float("nan")      # never read
            piece = inc[:, :, j0:j0 + Nc]
            big_col, col_out = guarded(MM + 1)
            big_row, row = guarded(NN + 1)
            with torch.cuda.device(inc.device):
                rc = fn(_lib._ptr(piece), piece.stride(-2), P, Mc, Nc, dyadic, _lib.SCHEME_DEFAULT, _lib._ptr(col_in), _lib._ptr(col_out),
                        _lib._ptr(row), _lib._stream(inc))
            torch.cuda.synchronize()
            assert rc == 0
            for big, width in ((big_col, MM + 1), (big_row, NN + 1)):
                written = torch.zeros_like(big, dtype=torch.bool)
                written[guard:guard + P * width].view(P, width)[:, 1:] = True
                assert bool(torch.isnan(big[~written]).all()) and bool(torch.isfinite(big[written]).all()), (P, Mc, Nc, dyadic, j0)
            fine = torch.arange(j0 * (1 << dyadic) + 1, (j0 + Nc) * (1 << dyadic) + 1, device=DEV)
            assert torch.equal(_bits(row[:, 1:].to(dtype)), _bits(grid[:, -1, fine]))
            assert torch.equal(_bits(col_out[:, 1:].to(dtype)), _bits(grid[:, 1:, (j0 + Nc) << dyadic]))
            col_in = col_out.clone()


def test_overlapping_columns_are_refused():
    lib = _lib.load()
    P, Mc, Nc, dyadic = 4, 3, 2, 1
    inc = _increments(P, Mc, Nc, torch.float64, 1)
    width = (Mc << dyadic) + 1
    both = torch.ones(2 * P * width, dtype=torch.float64, device=DEV)
    row = torch.zeros(P, (Nc << dyadic) + 1, dtype=torch.float64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    for a, b in ((both[:P * width], both[:P * width]), (both[:P * width], both[width:width + P * width]),
                 (both[P * width - 1:2 * P * width - 1], both[:P * width])):
        assert lib.sk_solve_fwd_resume_f64(p(inc), Nc, P, Mc, Nc, dyadic, 0, p(a), p(b), p(row), None) == 1      # SK_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool((both == 1).all()) and bool((row == 0).all())      # nothing was launched
    with pytest.raises(ValueError):
        col = both[:P * width].view(P, width)
        _lib.get_backend().solve_fwd_resume(inc, dyadic, False, col, col)


# ---- the API: resume="always" against the one-shot last row -------------------------------------------------------------------------------
def _is_fused(kind, D, M, N, dyadic, naive=False, elem_size=8):
    return _lib.HipBackend.route(_lib.OP_PREFIX, 0 if kind == "linear" else 1, D, M, N, dyadic, naive, elem_size) == _lib.ROUTE_FUSED


def _wall():
    wall = 2
    while _is_fused("linear", 3, wall + 1, 8, 1):
        wall += 1                                   # the longest bank path of one band at dyadic 1
    assert 32 <= wall <= 256
    return wall


class Duck:
    """a duck-typed static kernel: torch's Gram_matrix, not the HIP static stage"""

    def batch_kernel(self, X, Y):
        return sigkernel_amd.RBFKernel(0.7).batch_kernel(X, Y)

    def Gram_matrix(self, X, Y):
        return sigkernel_amd.RBFKernel(0.7).Gram_matrix(X, Y)


def _close(a, b):
    """the project's bar for fp64 forward values that do not share bits: 1e-12 max(1, |value|)"""
    return bool(((a.double() - b.double()).abs() <= 1e-12 * b.double().abs().clamp_min(1.0)).all())


# id -> (static kernel, dyadic, (A, B, M, D) with M None = one past the band, paired, dtype, workspace_bytes, exact bits)
CASES = {
    "dim9-linear": (lambda: sigkernel_amd.LinearKernel(), 1, (3, 4, 20, 9), False, torch.float64, None, True),
    "dim9-rbf": (lambda: sigkernel_amd.RBFKernel(1.0), 1, (3, 4, 20, 9), False, torch.float64, None, True),
    "past-the-band-linear": (lambda: sigkernel_amd.LinearKernel(), 1, (2, 3, None, 3), False, torch.float64, None, True),
    "past-the-band-rbf": (lambda: sigkernel_amd.RBFKernel(1.0), 1, (2, 3, None, 3), False, torch.float64, None, True),
    "dyadic3": (lambda: sigkernel_amd.RBFKernel(1.0), 3, (3, 2, 9, 3), False, torch.float64, None, True),
    "dim40-linear": (lambda: sigkernel_amd.LinearKernel(), 1, (2, 3, 12, 40), False, torch.float64, None, True),
    "dim40-rbf": (lambda: sigkernel_amd.RBFKernel(2.0), 1, (2, 3, 12, 40), False, torch.float64, None, True),
    "paired": (lambda: sigkernel_amd.RBFKernel(1.0), 1, (3, 3, 20, 9), True, torch.float64, None, True),
    "fp32": (lambda: sigkernel_amd.RBFKernel(1.0), 1, (3, 4, 20, 9), False, torch.float32, None, True),
    # (4, 2)-valued points have 8 features: the one-shot call maps them and lands INSIDE the fused scope of its base kernel, on the fused
    # prefix kernel -- whose bits the anti-diagonal solver does not share (measured here: 4.9e-15 apart).  The stream of a
    # function-valued kernel is the stream of its features, so it takes the fused resume there (ROUTE below) and keeps the bits;
    # (5, 2)-valued points, 10 features, are off the scope and take the column route.
    "rbf-id": (lambda: sigkernel_amd.RBF_ID_Kernel(1.0), 1, (2, 3, 7, (4, 2)), False, torch.float64, None, True),
    "rbf-id-dim10": (lambda: sigkernel_amd.RBF_ID_Kernel(1.0), 1, (2, 3, 7, (5, 2)), False, torch.float64, None, True),
    "linear-id-dim10": (lambda: sigkernel_amd.Linear_ID_Kernel(), 1, (2, 3, 7, (5, 2)), False, torch.float64, None, True),
    "row-tiles": (lambda: sigkernel_amd.LinearKernel(), 1, (3, 4, 20, 9), False, torch.float64, 1, True),
    "duck": (Duck, 1, (3, 4, 20, 9), False, torch.float64, None, False),
}


ROUTE = {"rbf-id": "fused"}      # every other case: "column"


@pytest.mark.parametrize("case", sorted(CASES))
def test_appends_are_the_one_shot_last_row(case):
    make, dyadic, (A, B, M, D), paired, dtype, workspace, exact = CASES[case]
    M = _wall() + 1 if M is None else M
    tail = D if isinstance(D, tuple) else (D,)
    flat = 1
    for t in tail:
        flat *= t
    sk = sigkernel_amd.SigKernel(make(), dyadic, workspace_bytes=workspace)
    ref = sigkernel_amd.SigKernel(make(), dyadic)      # the one-shot reference never row-tiles
    gen = torch.Generator().manual_seed(17)
    X = walk(gen, A, M, flat, dtype).reshape((A, M) + tail).to(DEV)
    Ylong = walk(gen, B, max(N0) + 6, flat, dtype).reshape((B, max(N0) + 6) + tail).to(DEV)
    last_row = ref.compute_kernel_prefixes if paired else ref.compute_Gram_prefixes
    final = ref.compute_kernel if paired else ref.compute_Gram
    same = (lambda a, b: torch.equal(_bits(a), _bits(b))) if exact else _close
    whole = {}       # total length -> (one-shot last row, one-shot kernel): computed once, shared
    for n0 in N0:
        for chunks in CHUNKS:
            total = n0 + sum(chunks)
            Yall = Ylong[:, :total].contiguous()
            if total not in whole:
                whole[total] = (last_row(X, Yall, nodes="last_row"), final(X, Yall))
            want, k_all = whole[total]
            st = sk.open_stream(X, Yall[:, :n0], paired=paired, resume="always")
            assert st.route == ROUTE.get(case, "column") and st.resumes is True and st.length == n0, (case, n0)
            held = st.state_bytes
            got, n = [], n0
            for c in chunks:
                new = st.append(Yall[:, n:n + c])
                n += c
                assert new.shape == ((A,) if paired else (A, B)) + (c,) and new.dtype == dtype and new.grad_fn is None
                # constant in the stream: exactly on the column route; the fused resume keeps one or two points
                slack = 0 if st.route == "column" else B * flat * X.element_size()
                assert st.length == n and abs(st.state_bytes - held) <= slack, (case, n0, chunks)
                got.append(new)
            got = torch.cat(got, dim=-1)
            err = float((got.double() - want[..., n0:].double()).abs().max())
            print("%s n0=%d chunks=%s: max |stream - one shot| = %.3g, kernel vs compute_Gram: %.3g"
                  % (case, n0, chunks, err, float((st.kernel.double() - k_all.double()).abs().max())))
            assert same(got, want[..., n0:]), (case, n0, chunks, err)
            assert same(st.kernel, want[..., -1]), (case, n0, chunks)
            if dtype == torch.float64:
                assert _close(st.kernel, k_all), (case, n0, chunks)
    if ROUTE.get(case, "column") != "column":
        return
    pairs = A if paired else A * B
    fine = ((M - 1) << dyadic) + 1
    assert held ==2 * pairs * fine * 8 + (A * M + B) * flat * X.element_size()      # two fp64 columns, the bank, the kept point


def test_a_nan_point_poisons_its_own_stream_alone():
    A, B, M, D = 3, 4, 12, 9
    gen = torch.Generator().manual_seed(23)
    X, Y = walk(gen, A, M, D).to(DEV), walk(gen, B, 9, D).to(DEV)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(1.0), 1)
    clean = sk.open_stream(X, Y[:, :2], resume="always")
    want = torch.cat([clean.append(Y[:, 2:5]), clean.append(Y[:, 5:])], dim=-1)
    bad = Y.clone()
    bad[2, 3, 4] = float("nan")      # one coordinate of one new point of stream 2
    st = sk.open_stream(X, bad[:, :2], resume="always")
    got = torch.cat([st.append(bad[:, 2:5]), st.append(bad[:, 5:])], dim=-1)      # columns 2 .. 8
    others = [b for b in range(B) if b != 2]
    assert torch.equal(_bits(got[:, others]), _bits(want[:, others])) and torch.equal(_bits(st.kernel[:, others]), _bits(clean.kernel[:, others]))
    assert torch.equal(_bits(got[:, 2, :1]), _bits(want[:, 2, :1]))             # the point before it
    assert not bool(torch.isfinite(got[:, 2, 1:]).any()) and not bool(torch.isfinite(st.kernel[:, 2]).any())


def test_the_default_and_the_fused_scope_are_what_they_were():
    gen = torch.Generator().manual_seed(29)
    # off the scope the default keeps the history
    X, Y = walk(gen, 3, 20, 9).to(DEV), walk(gen, 4, 8, 9).to(DEV)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(1.0), 1)
    for st in (sk.open_stream(X, Y[:, :2]), sk.open_stream(X, Y[:, :2], resume="fused")):
        assert st.resumes is False and st.route == "history" and st.state_bytes == 4 * 2 * 9 * 8
        assert torch.equal(st.append(Y[:, 2:]), sk.compute_Gram_prefixes(X, Y, nodes="last_row")[..., 2:])
        assert st.state_bytes == 4 * 8 * 9 * 8
    # inside the scope "always" is the fused resume: its route, its bits, its state
    X, Y = walk(gen, 3, 9, 3).to(DEV), walk(gen, 2, 8, 3).to(DEV)
    assert _is_fused("rbf", 3, 9, 8, 1)
    a, b = sk.open_stream(X, Y[:, :2]), sk.open_stream(X, Y[:, :2], resume="always")
    assert a.route == b.route == "fused" and b.resumes is True and a.state_bytes == b.state_bytes
    assert torch.equal(_bits(a.append(Y[:, 2:])), _bits(b.append(Y[:, 2:]))) and torch.equal(_bits(a.kernel), _bits(b.kernel))
    # the route switch sends a shape inside the scope to the column route under "always"
    sigkernel_amd.routes.no_fused_prefix = True
    try:
        off = sk.open_stream(X, Y[:, :2], resume="always")
        assert off.route == "column"
        slow = off.append(Y[:, 2:])
        assert torch.equal(slow, sk.compute_Gram_prefixes(X, Y, nodes="last_row")[..., 2:])
    finally:
        sigkernel_amd.routes.no_fused_prefix = False
