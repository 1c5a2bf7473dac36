"""Row-local dealing of the fused Gram forward (csrc/sk_pair_stream.h: plan_row_dealing; csrc/sk_wave_fused.hip).

In the shared-y order stream position q of a wave is Gram row-block q // B (the rows x_a, a = G (q // B) + g, of its G lane groups) and
column q % B.  Where the row-blocks divide the resident waves evenly, every row-block has waves of its own -- a static share each, then
draws from the row-block's own counter, then from following row-blocks' counters, found in a bounded number of looks -- so a wave stays with
the x rows of one row-block and fetches them once: a position that opens the row-block of the wave's previous one issues no x DMA and
no reload of the rows into registers.  Which wave computes a pair changes; how a pair is computed does not, so every output is, bit
for bit, what the commit before returned.

CPU: the exported plan (sk_plan_row_dealing) partitions the positions exactly, is off wherever a condition fails and is then the
earlier plan field for field (restated here); a replay of the kernel's draw loop hands out every position once for any bound.

GPU (the headline instance: linear, dyadic 1, 8 dims, 128 points; the smallest launches that still draw from the counter):
  256 x 192   every wave sees one row-block            1024 x 49   rows shorter than a CU's share: steals all the time
  257 x 192   odd A: 129 row-blocks do not divide 3072 waves, the mode is off          250 x 200   the mode is off
and one RBF Gram with four lane groups per wave (dim 3, 64 points, 512 x 512).  Each: 256 seeded entries (16 rows x 16 columns) against
the CPU oracle at 1e-12 and bit for bit against tests/golden/fused_row_dealing_parent.npz -- the PARENT commit's values, recorded once
on an MI355X by record_golden() (run with the parent's package first on sys.path) -- and no entry of the output left unwritten: the
call runs on an output and workspaces that held 0xFF bytes (tests/poison.py), so an unwritten entry is a NaN."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import sigkernel_amd
from launch_plans import earlier_plan as _earlier_plan      # (plan_pair_stream restated: the plan before row-local dealing)
from oracle import oracle as O
from poison import poisoned

FAST_TOL = 1e-12
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_row_dealing_parent.npz")
N_CU = 256          # MI355X; the CPU tests plan for it whatever box they run on


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
FIELDS = ("mode", "waves", "per", "q_first", "C0", "n_big", "logC", "queue", "wprb", "n_rb", "row_q0", "row_rem", "queues")


def _plan(A, B, G, NUp, L, lag=0, wpc=12, n_cu=N_CU, pct=35, words=None):
    """sk_plan_row_dealing -> ({field: value}, static [waves][2], queues [n][2])"""
    from sigkernel_amd import _lib
    lib = _lib.load()
    words = (A // 2 + 1 if words is None else words)
    plan = np.zeros(13, np.int64)
    cap = n_cu * wpc
    sf, se = np.zeros(cap, np.int64), np.zeros(cap, np.int64)
    qcap = max(1, (A + G - 1) // G)
    qf, qe = np.zeros(qcap, np.int64), np.zeros(qcap, np.int64)
    rc = lib.sk_plan_row_dealing(A, B, G, NUp, L, lag, wpc, n_cu, pct, words, plan.ctypes.data, cap, sf.ctypes.data, se.ctypes.data,
                                 qcap, qf.ctypes.data, qe.ctypes.data)
    assert rc == 0, rc
    f = dict(zip(FIELDS, (int(v) for v in plan)))
    return f, np.stack([sf, se], 1)[: f["waves"]], np.stack([qf, qe], 1)[: f["queues"]]


def _mode_expected(A, B, G, NUp, L, lag, wpc, n_cu, pct, words):
    """the conditions of the mode, one by one"""
    if G < 2:
        return False
    n_rb = (A + G - 1) // G
    e = _earlier_plan(n_rb * B, NUp, L, lag, wpc, n_cu, pct, words > 0)
    return bool(e["queue"]) and e["waves"] % n_rb == 0 and e["waves"] // n_rb >= 1 and L <= NUp and words >= n_rb


# A, B, G, NUp, L, lag, waves per CU, pct: the headline (c3), the GPU cases below, the other shared-y shape of the timing protocol
# (2048 x 2048 pairs of 64 points at dyadic 0: L = 16, G = 4, chunks of 8), the RBF case, and shapes around every condition
SHAPES = [
    (512, 512, 2, 64, 32, 0, 12, 35),      # c3: 256 row-blocks x 12 waves
    (256, 192, 2, 64, 32, 0, 12, 35),
    (1024, 49, 2, 64, 32, 0, 12, 35),
    (257, 192, 2, 64, 32, 0, 12, 35),      # 129 row-blocks: off
    (250, 200, 2, 64, 32, 0, 12, 35),      # 125 row-blocks: off
    (2048, 2048, 4, 32, 16, 0, 8, 35),
    (512, 512, 4, 32, 16, 2, 8, 20),       # the RBF case
    (511, 512, 2, 64, 32, 0, 12, 35),      # odd A, 256 row-blocks all the same: on, the last row-block's second group is empty
    (512, 511, 2, 64, 32, 0, 12, 35),      # odd B
    (512, 512, 2, 8, 32, 0, 12, 35),       # L > NUp (four laps of lanes per position): off
    (512, 512, 1, 64, 64, 0, 12, 35),      # one lane group per wave: no row-blocks
    (64, 64, 2, 64, 32, 0, 12, 35),        # too few positions for the counter
    (6144, 40, 2, 64, 32, 0, 12, 35),      # one wave per row-block
    (12288, 20, 2, 64, 32, 0, 12, 35),     # more row-blocks than waves: off
    (512, 512, 2, 64, 32, 0, 12, 99),      # nearly everything up front
    (512, 1000, 8, 16, 8, 0, 8, 35),       # eight lane groups
    (768, 333, 2, 64, 32, 0, 12, 50),
    (1536, 97, 4, 32, 16, 0, 8, 35),
]


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d_G%d_NUp%d_pct%d" % (s[0], s[1], s[2], s[3], s[7]) for s in SHAPES])
def test_the_plan_partitions_the_positions_and_falls_back_to_the_earlier_plan(shape):
    A, B, G, NUp, L, lag, wpc, pct = shape
    f, static, queues = _plan(A, B, G, NUp, L, lag, wpc, N_CU, pct)
    n_pos = (A + G - 1) // G * B if G >= 2 else A * B
    assert bool(f["mode"]) == _mode_expected(A, B, G, NUp, L, lag, wpc, N_CU, pct, A // 2 + 1), f
    seen = np.zeros(n_pos, np.int32)
    for lo, hi in list(static) + list(queues):
        assert 0 <= lo <= hi <= n_pos
        seen[lo:hi] += 1
    assert seen.min() == 1 and seen.max() == 1, f
    earlier = _earlier_plan(n_pos, NUp, L, lag, wpc, N_CU, pct, True)
    if not f["mode"]:
        assert {k: f[k] for k in earlier} == earlier, (f, earlier)
        assert f["wprb"] == f["n_rb"] == f["row_q0"] == f["row_rem"] == 0
        assert f["queues"] == f["queue"]
    else:
        CQ = 1 << f["logC"]
        n_rb = (A + G - 1) // G
        assert f["queue"] == 1 and f["n_rb"] == f["queues"] == n_rb and f["wprb"] * n_rb == f["waves"] == earlier["waves"]
        assert f["logC"] == earlier["logC"] and f["per"] == earlier["per"]
        assert f["C0"] == min(earlier["C0"], B // f["wprb"])      # the same per cent of the equal share
        assert 0 <= f["row_rem"] < CQ and f["row_q0"] == f["wprb"] * f["C0"] + f["row_rem"]
        for h in range(n_rb):
            lo, hi = queues[h]
            assert h * B <= lo <= hi == (h + 1) * B and (hi - lo) % CQ == 0      # whole chunks, inside the row-block
            home = static[h::n_rb]                                             # wave w is at home in row-block w % n_rb
            assert len(home) == f["wprb"]
            assert home[0][0] == h * B and home[-1][1] == lo and all(home[i][1] == home[i + 1][0] for i in range(len(home) - 1))


def test_the_headline_and_the_gpu_cases_are_planned_as_the_tests_below_assume():
    on = {s[:2]: _plan(*s[:6], wpc=s[6], pct=s[7])[0] for s in SHAPES[:6]}
    assert [on[k]["mode"] for k in ((512, 512), (256, 192), (1024, 49), (257, 192), (250, 200), (2048, 2048))] == [1, 1, 1, 0, 0, 1]
    assert all(p["queue"] == 1 for p in on.values())                  # every one of them draws from a counter
    rbf = _plan(*SHAPES[6][:6], wpc=SHAPES[6][6], pct=SHAPES[6][7])[0]
    assert (rbf["mode"], rbf["wprb"], rbf["n_rb"]) == (1, 16, 128)
    c3 = on[(512, 512)]
    assert (c3["waves"], c3["per"], c3["C0"], c3["logC"], c3["wprb"], c3["n_rb"], c3["row_q0"]) == (3072, 43, 15, 0, 12, 256, 180)
    assert on[(1024, 49)]["wprb"] * on[(1024, 49)]["per"] > 49         # a row-block is shorter than its waves' equal shares
    # a caller with too few counters, or none, gets the earlier plan
    assert _plan(512, 512, 2, 64, 32, words=255)[0]["mode"] == 0 and _plan(512, 512, 2, 64, 32, words=256)[0]["mode"] == 1
    assert _plan(512, 512, 2, 64, 32, words=1)[0] == dict(_plan(512, 512, 2, 64, 32, words=8)[0])
    assert _plan(512, 512, 2, 64, 32, words=0)[0]["queue"] == 0


def _replay(f, B, bound, rng):
    """The kernel's draw loop (sk_wave_fused.hip: ensure), waves interleaved at random: every wave takes its static share, then draws a
    chunk at a time from its row-block's counter; that used up, it looks at most `bound` times at the next 64 counters for a row-block that
    has positions left.  -> times each position is dealt"""
    n_rb, wprb, CQ = f["n_rb"], f["wprb"], 1 << f["logC"]
    seen = np.zeros(n_rb * B, np.int32)
    counter = [0] * n_rb
    live = []
    for w in range(f["waves"]):
        j, h = divmod(w, n_rb)
        first = h * B + j * f["C0"]
        seen[first:first + f["C0"] + (f["row_rem"] if j == wprb - 1 else 0)] += 1
        live.append([h, bound])
    while live:
        i = rng.randrange(len(live))
        rb, more = live[i]
        while True:
            v = counter[rb]
            counter[rb] += CQ
            o = f["row_q0"] + v
            if o < B:
                seen[rb * B + o: rb * B + o + CQ] += 1
                break
            # used up: looks at the next 64 counters at a time for a row-block that has positions left
            cand, reach = -1, min(n_rb - 1, 64)
            while more > 0 and cand < 0:
                more -= 1
                open_ = [k for k in range(reach) if f["row_q0"] + counter[(rb + 1 + k) % n_rb] < B]
                if open_:
                    cand = (rb + 1 + open_[0]) % n_rb
                elif reach < 64:
                    more = 0
                else:
                    rb = (rb + 64) % n_rb
            if cand < 0:
                rb = -1
                break
            rb = cand
        if rb < 0:
            live.pop(i)
        else:
            live[i] = [rb, more]
    return seen


@pytest.mark.parametrize("bound", [0, 1, 3, 31])
@pytest.mark.parametrize("shape", [(48, 96, 2, 64, 32, 12, 4),(192, 17, 2, 64, 32, 12, 8), (128, 600, 4, 32, 16, 8, 4), (1536, 9, 2, 64, 32, 12, 64)], ids=["even", "short_rows", "chunks", "many_rows"])
def test_every_position_is_dealt_once_whatever_the_bound_and_the_order(shape, bound):
    A, B, G, NUp, L, wpc, n_cu = shape      # (small chips: the replay is Python)
    f, _, _ = _plan(A, B, G, NUp, L, 0, wpc, n_cu, 35)
    assert f["mode"] == 1, f
    for seed in range(3):
        seen = _replay(f, B, bound, random.Random(100 * bound + seed))
        assert seen.min() == 1 and seen.max() == 1, (bound, seed)


# ---- the launches -----------------------------------------------------------------------------------------------------------------------
# name, A, B, points, dims, static kernel, dyadic
CASES = [("one_block", 256, 192, 128, 8, "linear", 1),
         ("steals", 1024, 49, 128, 8, "linear", 1),
         ("odd_rows", 257, 192, 128, 8, "linear", 1),
         ("mode_off", 250, 200, 128, 8, "linear", 1),
         ("rbf_g4", 512, 512, 64, 3, "rbf", 1)]
IDS = [c[0] for c in CASES]


def _kernel(kind):
    return sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(0.75)


def _walk(gen, A, M, D):
    return torch.cumsum(torch.randn(A, M, D, generator=gen, dtype=torch.float64), dim=1) / np.sqrt(M * D)


def _inputs(case):
    name, A, B, M, D, kind, dyadic = case
    gen = torch.Generator().manual_seed(9100 + 61 * IDS.index(name))
    X, Y = _walk(gen, A, M, D), _walk(gen, B, M, D)
    # 16 rows x 16 columns: the corners of the Gram (row A - 1 is the odd case's lone group), the rest seeded
    rows = sorted(set([0, 1, A - 2, A - 1] + torch.randperm(A - 4, generator=gen)[:12].add(2).tolist()))
    cols = sorted(set([0, B - 1] + torch.randperm(B - 2, generator=gen)[:14].add(1).tolist()))
    assert len(rows) == 16 and len(cols) == 16
    return X, Y, rows, cols


def _gram(case, X, Y, poison):
    """the whole Gram on the GPU; poison: on an output and workspaces of 0xFF bytes (an unwritten entry stays a NaN)"""
    name, A, B, M, D, kind, dyadic = case
    sk = sigkernel_amd.SigKernel(_kernel(kind), dyadic_order=dyadic)
    if not poison:
        K = sk.compute_Gram(X.to(DEV), Y.to(DEV))
    else:
        with poisoned(0xFF, {("_lib", "_queue")}) as p:
            K = sk.compute_Gram(X.to(DEV), Y.to(DEV))
        assert p.sites.get(("_lib", "_queue"), 0) == 1 and p.count >= 2, p.sites      # the counters and the output among them
    torch.cuda.synchronize()
    return K.cpu().numpy()


def _sample(case, poison=False):
    X, Y, rows, cols = _inputs(case)
    K = _gram(case, X, Y, poison)
    name = case[0]
    return K, {name + "_in": np.array([float(X.sum()), float(Y.sum())]), name + "_rows": np.array(rows), name + "_cols": np.array(cols),
               name + "_K": K[np.ix_(rows, cols)].copy()}


def record_golden(path=GOLDEN):
    """Write the golden file from whatever build of the package is imported: run ONCE with the parent commit's build on an MI355X."""
    out = {}
    for case in CASES:
        out.update(_sample(case)[1])
    np.savez_compressed(path, **out)
    return path


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN, allow_pickle=False))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_row_dealing_writes_every_entry_keeps_every_bit_and_matches_the_oracle(case, gold):
    name, A, B, M, D, kind, dyadic = case
    X, Y, rows, cols = _inputs(case)
    K, got = _sample(case, poison=True)
    assert K.shape == (A, B)
    unwritten = int(np.count_nonzero(~np.isfinite(K)))
    want = O.gram_forward(X[rows], Y[cols], _kernel(kind), dyadic, nthreads=min(16, O.max_threads()))
    err = float(np.max(np.abs(got[name + "_K"] - want)) / max(np.max(np.abs(want)), 1e-300))
    same = {k: bool(np.array_equal(got[k], gold[k])) for k in got}
    print("row dealing %s: %d entries unwritten, oracle rel err %.3g, bit-identical to the parent %s" % (name, unwritten, err, same))
    assert unwritten == 0, "%d entries of the Gram were never written" % unwritten
    assert same[name + "_in"] and same[name + "_rows"] and same[name + "_cols"], "the seeded inputs are not the recorded ones"
    assert err <= FAST_TOL, err
    assert same[name + "_K"], "the sampled entries are not bit-identical to the parent commit's"
