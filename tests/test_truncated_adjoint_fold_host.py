"""The truncated kernel's four adjoint modes after their host code was folded into one plan and one launcher (csrc/sk_truncated.hip:
truncated_adjoint_plan / launch_truncated_adjoint over a table of modes), held to the build BEFORE the fold without a GPU:
tests/golden/truncated_adjoint_fold_plans.npz, recorded from the parent commit by tests/golden/make_golden_truncated_adjoint_fold.py.

* the four exported plan entry points over a thinned grid of shapes x four workspaces: the return code and every plan entry;
* the four exported launch entry points on calls the parent REJECTS before any HIP call: the return code.  Nothing here reaches a launch.

The plans are host-only arithmetic on the CU count.  Without a device the library takes 256 CUs, the MI355X's own count, so the record
ASSUMES 256 CUs: on a device with another count the plan test would compare against the wrong record (the file says so: `cu_count`)."""
import ctypes
import itertools
import os

import numpy as np
import pytest

from conftest import ROOT

PLANS = os.path.join(ROOT, "tests", "golden", "truncated_adjoint_fold_plans.npz")

# the entry points, in the order of the record's entry axis; (plan, launch, staging width, takes param)
ENTRIES = [
    ("sk_truncated_adjoint_plan", "sk_truncated_adjoint", 8, False),
    ("sk_truncated_points_adjoint_plan", "sk_truncated_points_adjoint", 8, True),
    ("sk_truncated_long_adjoint_plan", "sk_truncated_long_adjoint", 8, False),
    ("sk_truncated_wide_adjoint_plan", "sk_truncated_wide_adjoint", 16, False),
]
PLAIN, POINTS, LONG, WIDE = range(4)

WORKSPACES = (0, 64 << 10, 1 << 20, 1 << 30)
THIN = 5        # every THIN-th shape of the full grid of 13440: the file stays small, and the fixture test checks that every value of every axis stays
UNTOUCHED = -1  # what a plan entry holds before the call


def shapes():
    """the thinned grid: (A, B, M, N, D, L, paired), each with all four WORKSPACES"""
    full = itertools.product((1, 5, 300, 5000), (1, 5, 300, 5000), (1, 2, 9, 64, 128, 129, 300), (1, 8, 33, 257, 600), (1, 8, 9, 16),
                             (1, 2, 8), (0, 1))
    return [s for i, s in enumerate(full) if i % THIN == 0]


def plan(lib, entry, A, B, M, N, D, L, paired, ws):
    """(rc, plan[0..3]) of one plan entry point; entries the call leaves alone stay UNTOUCHED"""
    out = (ctypes.c_int64 * 4)(*[UNTOUCHED] * 4)
    rc = getattr(lib, ENTRIES[entry][0])(A, B, M, N, D, L, paired, ws, ctypes.cast(out, ctypes.c_void_p))
    return (int(rc),) + tuple(int(v) for v in out)


def record_plans(lib):
    """-> int64 (shapes, workspaces, entries, 5): rc and the four plan entries"""
    return np.array([[[plan(lib, e, *s, ws) for e in range(4)] for ws in WORKSPACES] for s in shapes()], dtype=np.int64)


# ---- the launch entry points' rejected calls -------------------------------------------------------------------------------------------------
def _valid(entry):
    """a call of launch entry `entry` that passes every check (never made): each case below changes it in one respect"""
    wide = entry == WIDE
    return dict(A=1, B=1, Mrows=2, M=2, N=2, Ncp=16, D=9 if wide else 2, fd=16 if wide else 8, L=2, param=0.5, n_chunks=1, slab_bytes=1 << 20,
                paired=0, null=())


def rejected_cases(entry):
    """[(name, the keywords that differ from _valid)]: null pointers, the staging, the chunk count, the pairs, the slab, param, the scopes"""
    wide = entry == WIDE
    cases = [("null_" + n, dict(null=(n,))) for n in ("Xr", "Yt", "w", "Tpart")]
    cases += [
        ("slab_bytes_without_slab", dict(null=("slab",))),
        ("no_slab_at_all", dict(null=("slab",), slab_bytes=0)),                 # points: BAD_ARG; the others go on and find one block's slab too large
        ("Mrows_below_M", dict(Mrows=1)),
        ("Ncp_below_N", dict(Ncp=1)),
        ("Ncp_24", dict(Ncp=24, slab_bytes=1)),                                 # fits the wave's y block: only the long mode minds; the others find the slab too small
        ("fd_other", dict(fd=8 if wide else 16)),
        ("fd_below_D", dict(D=9 if not wide else 16, fd=8)),
        ("n_chunks_0", dict(n_chunks=0)),
        ("n_chunks_B_plus_1", dict(B=3, n_chunks=4)),
        ("paired_n_chunks_2", dict(paired=1, n_chunks=2)),
        ("paired_A_not_B", dict(A=1, B=2, paired=1, slab_bytes=1)),             # wide: BAD_ARG; the others take B = A and find the slab too small
        ("slab_one_byte", dict(slab_bytes=1)),                                  # one block's slab does not fit
        ("param_zero", dict(param=0.0, slab_bytes=1)),                          # points: BAD_ARG; the others take no param and find the slab too small
        ("param_negative", dict(param=-1.0, slab_bytes=1)),
        ("param_nan", dict(param=float("nan"), slab_bytes=1)),
        ("D_0", dict(D=0)),
        ("D_other_scope", dict(D=8, fd=16) if wide else dict(D=9, fd=16)),
        ("D_17", dict(D=17, fd=32)),
        ("M_0", dict(M=0)),
        ("M_1_point", dict(M=1, slab_bytes=1)),                                 # the points mode: a path has at least one step; the others: the slab
        ("M_129", dict(M=129, Mrows=129, slab_bytes=1)),                        # long: in scope, the slab too small
        ("M_beyond_2_20", dict(M=(1 << 20) + 1, Mrows=(1 << 20) + 1)),
        ("N_beyond_the_y_block", dict(N=257, Ncp=272, slab_bytes=1)),           # long: in scope, the slab too small
        ("L_0", dict(L=0)),
        ("L_9", dict(L=9)),
    ]
    return cases


def launch_rc(lib, entry, kw):
    """the return code of launch entry `entry` on _valid changed by `kw`; the pointers are one dummy host buffer -- no accepted call may be made"""
    a = dict(_valid(entry), **kw)
    buf = (ctypes.c_double * 64)()
    p = lambda name: None if name in a["null"] else ctypes.cast(buf, ctypes.c_void_p)
    args = [p("Xr"), p("Yt"), a["A"], a["B"], a["Mrows"], a["M"], a["N"], a["Ncp"], a["D"], a["fd"], a["L"]]
    if ENTRIES[entry][3]:
        args.append(ctypes.c_double(a["param"]))
    args += [p("w"), p("Tpart"), a["n_chunks"], p("slab"), a["slab_bytes"], None, a["paired"]]
    return int(getattr(lib, ENTRIES[entry][1])(*args))


def record_launch_rcs(lib):
    """-> (case names, int64 (cases, entries))"""
    names = [n for n, _ in rejected_cases(PLAIN)]
    assert all([n for n, _ in rejected_cases(e)] == names for e in range(4))
    return names, np.array([[launch_rc(lib, e, dict(rejected_cases(e))[n]) for e in range(4)] for n in names], dtype=np.int64)


# ---- the tests ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def record():
    return np.load(PLANS)


def test_fixture_file_covers_what_it_should(record):
    """under 100 KB, and every regime the grid is there for occurs: both declines, the lowered block count, the paired widening at 8 and
    at 16 coordinates, more than one band with more than one column tile"""
    assert os.path.getsize(PLANS) < 100 << 10
    assert int(record["cu_count"]) == 256
    S, P = shapes(), record["plans"]
    assert P.shape == (len(S), len(WORKSPACES), 4, 5) and len(S) >= 1500
    for axis, values in enumerate(((1, 5, 300, 5000), (1, 5, 300, 5000), (1, 2, 9, 64, 128, 129, 300), (1, 8, 33, 257, 600), (1, 8, 9, 16),
                                   (1, 2, 8), (0, 1))):
        assert {s[axis] for s in S} == set(values), axis
    rc, big = P[..., 0], len(WORKSPACES) - 1
    assert set(np.unique(rc)) == {0, 2}
    for e in range(4):
        out_of_scope = rc[:, big, e] == 2                       # 1 GiB holds one block's slab of every shape of the grid
        too_large = (rc[:, 0, e] == 2) & ~out_of_scope
        lowered = (rc[:, 1, e] == 0) & (P[:, 1, e, 2] < P[:, big, e, 2]) | (rc[:, 2, e] == 0) & (P[:, 2, e, 2] < P[:, big, e, 2])
        assert out_of_scope.any() and (~out_of_scope).any() and too_large.any() and lowered.any(), ENTRIES[e][0]
        # a declined call leaves the plan alone; only the long adjoint's plan has a fourth entry
        assert (P[..., e, 1:][rc[..., e] == 2] == UNTOUCHED).all()
        assert ((P[..., e, 4] != UNTOUCHED) == ((rc[..., e] == 0) & (e == LONG))).all()
    # the lanes of a pair's group, from the slab of a block: planes x (N + W - 1) KB
    def lanes(e, i, s):
        A, B, M, N, D, L, paired = s
        planes = L if e == POINTS else L - 1
        return P[i, big, e, 3] // P[i, big, e, 2] // (planes << 10) - N + 1
    natural = lambda M: 1 << max(0, (M + 1) // 2 - 1).bit_length()
    for e in (PLAIN, POINTS, WIDE):
        widened = [s for i, s in enumerate(S) if s[6] and s[5] > 1 and rc[i, big, e] == 0 and lanes(e, i, s) > natural(s[2])]
        unwidened = [s for i, s in enumerate(S) if s[5] > 1 and rc[i, big, e] == 0 and lanes(e, i, s) == natural(s[2])]
        assert widened and unwidened, ENTRIES[e][0]
    assert any(rc[i, big, LONG] == 0 and s[2] > 128 and s[3] > 256 and s[5] > 1 for i, s in enumerate(S))     # bands x tiles
    assert any(rc[i, big, LONG] == 0 and s[2] > 128 and s[6] for i, s in enumerate(S))
    names, R = [str(n) for n in record["launch_cases"]], record["launch_rc"]
    assert names == [n for n, _ in rejected_cases(PLAIN)] and R.shape == (len(names), 4)
    assert set(np.unique(R)) == {1, 2}                                                                          # rejected, every one
    row = lambda n: tuple(int(v) for v in R[names.index(n)])
    assert row("paired_A_not_B") == (2, 2, 2, 1)            # (plain, points, long, wide): only the wide entry minds the pairs
    assert row("no_slab_at_all") == (2, 1, 2, 2) and row("param_zero")[POINTS] == 1 and row("M_129")[LONG] == 2 and row("M_129")[PLAIN] == 2
    assert row("fd_other") == (1, 1, 1, 1) and row("D_other_scope") == (2, 2, 2, 2)


def test_plans_are_the_parents(record):
    from sigkernel_amd import _lib
    got, want = record_plans(_lib.load()), record["plans"]
    bad = np.argwhere((got != want).any(-1))
    assert bad.size == 0, [(shapes()[i], WORKSPACES[j], ENTRIES[e][0], got[i, j, e].tolist(), want[i, j, e].tolist()) for i, j, e in bad[:5]]


def test_rejected_launch_calls_return_what_the_parent_returned(record):
    from sigkernel_amd import _lib
    names, got = record_launch_rcs(_lib.load())
    want = record["launch_rc"]
    assert names == [str(n) for n in record["launch_cases"]]
    bad = np.argwhere(got != want)
    assert bad.size == 0, [(names[i], ENTRIES[e][1], int(got[i, e]), int(want[i, e])) for i, e in bad[:10]]
