"""The host arithmetic the fused adjoints, the multi-band forward and the fused derivative solver share (csrc/sk_wave_common.h:
plan_adjoint_chunks; csrc/sk_pair_stream.h: one_draw_waves_per_cu, plan_one_draw), exported as sk_plan_adjoint_chunks and
sk_plan_one_draw, against what every launcher computed on its own before (tests/launch_plans.py: restated from the commit before).

Each launcher used to carry a copy: the rows-per-launch search twice, the one-draw plan three times.  One table per plan holds the
shapes around every branch -- the tables assert that they reach them -- and a few thousand seeded random shapes hold the rest: restatement
== export field for field, and wherever a Gram is swept in several launches, the launches tile its rows once with the same chunks per row."""
import random

import numpy as np
import pytest

import launch_plans as LP

N_CU = 256          # MI355X; the plans are computed for it whatever box the test runs on
UNSUPPORTED = 2     # SK_ERR_UNSUPPORTED


def _lib():
    from sigkernel_amd import _lib
    return _lib.load()


def plan_adjoint(A, B, G, NUp, wpc=8, wpb_knob=0, lds=20000, paired=True, force_nch=0, n_cu=N_CU):
    """sk_plan_adjoint_chunks -> {field: value}, or None where a 32-bit guard refuses the launch"""
    out = np.full(5, -1, np.int64)
    rc = _lib().sk_plan_adjoint_chunks(A, B, G, NUp, n_cu, wpc, wpb_knob, lds, int(paired), force_nch, out.ctypes.data)
    assert rc in (0, UNSUPPORTED), rc
    return dict(zip(("PPG", "ppp", "rows_per_launch", "groups", "nch"), (int(v) for v in out))) if rc == 0 else None


def plan_one_draw(P, lds, wpb0, vgprs, wpc_knob, units, pct, ws_stride, n_cu=N_CU):
    """sk_plan_one_draw -> {field: value}, or None where a 32-bit guard refuses the launch"""
    out = np.full(7, -1, np.int64)
    rc = _lib().sk_plan_one_draw(P, lds, wpb0, vgprs, wpc_knob, n_cu, units, pct, ws_stride, out.ctypes.data)
    assert rc in (0, UNSUPPORTED), rc
    return dict(zip(("wpc", "waves", "per", "C0", "q_first", "queue", "ws_doubles"), (int(v) for v in out))) if rc == 0 else None


def _restated_adjoint(A, B, G, NUp, wpc=8, wpb_knob=0, lds=20000, paired=True, force_nch=0, n_cu=N_CU):
    r = LP.adjoint_chunks(A, B, G, NUp, n_cu, wpc, wpb_knob, lds, paired, force_nch)
    if r is not None:
        r["nch"] = LP.chunks_of(B, r["PPG"])
    return r


def _restated_one_draw(P, lds, wpb0, vgprs, wpc_knob, units, pct, ws_stride, n_cu=N_CU):
    wpc = LP.one_draw_waves_per_cu(lds, wpb0, vgprs, wpc_knob)
    r = LP.one_draw(P, n_cu * wpc, units, pct, ws_stride)
    if r is not None:
        r["wpc"] = wpc
    return r


# ---- the adjoint chunk planner ----------------------------------------------------------------------------------------------------------
# With 8 waves per CU and four waves per workgroup (20000 bytes of LDS a wave) there are 2048 G resident lane groups in two age ranks.
# tag: what the row is there for, asserted from the plan --
#   fill      one launch that fills the chip exactly, chunks a multiple of the ranks      whole    several launches, a whole number
#   partial   several launches, the last one partial                                      one      one launch that does not fill exactly
#   paired    a paired batch                                                              forced   the chunks per row are the caller's
#   refused   a 32-bit guard
# (A, B, G, NUp, keywords, tag)
def _mg(G, wpc=8):
    return N_CU * wpc * G


ADJ_ROWS = []
for _G in (1, 2, 4, 8):
    ADJ_ROWS += [
        (_mg(_G) // 64, 512, _G, 16, {}, "fill"),             # 64 chunks of 8 per row
        (_mg(_G) // 8 * 3, 64, _G, 16, {}, "whole"),          # three launches of 8 chunks of 8 per row
        (_mg(_G) // 8 * 3 - 5, 64, _G, 24, {}, "partial"),
        {1: (108, 256), 2: (111, 512), 4: (118, 1536), 8: (519, 2048)}[_G] + (_G, 16, {}, "partial"),
    ]
ADJ_ROWS += [
    (1536, 64, 2, 24, {}, "whole"),                           # the launches of tests/test_gpu_adjoint_launches.py
    (1536, 64, 1, 24, {"lds": 45000, "wpc": 8}, "one"),       # 45000 bytes a wave: three waves per workgroup do not divide the 8 per CU
    (997, 96, 2, 16, {}, "partial"),                          # A prime
    (4096, 127, 2, 16, {}, "one"),                            # B prime: no m divides it
    (2048, 7, 2, 16, {}, "one"),                              # B < 4 nr: no chunk of four pairs per rank
    (100, 64, 2, 16, {}, "one"),                              # A < rows per launch for every m
    (511, 64, 2, 16, {}, "one"),                              # A nch one below max_groups at m = 8 (512 rows a launch): one launch
    (513, 64, 2, 16, {}, "one"),                              # ... and one above: a second launch for one row does not pay
    (4095, 1, 2, 16, {}, "one"),                              # A nch = max_groups - 1 with one chunk per row
    (4097, 1, 2, 16, {}, "one"),
    (64, 512, 2, 16, {"lds": 60000}, "fill"),                 # two waves per workgroup: four ranks
    (1536, 64, 2, 16, {"lds": 60000}, "partial"),             # (launches of 1024 rows, four chunks of 16)
    (64, 512, 2, 16, {"lds": 100000}, "fill"),                # one wave per workgroup: eight ranks
    (64, 512, 2, 16, {"wpb_knob": 2}, "fill"),
    (64, 512, 2, 16, {"wpc": 4}, "one"),                      # one rank: no shares by rank, no search
    (64 * 4096 - 1, 0, 2, 16, {}, "paired"),                  # a paired batch below, at and above 64 x max_groups
    (64 * 4096, 0, 2, 16, {}, "paired"),
    (64 * 4096 + 1, 0, 2, 16, {}, "paired"),
    (3 * 4096 + 5, 0, 2, 16, {}, "paired"),
    (3 * 4096 + 5, 0, 2, 16, {"paired": False}, "paired"),    # a variant without the PAIRED form: one pair per lane group
    (17, 0, 8, 8, {}, "paired"),
    (1536, 64, 2, 24, {"force_nch": 8}, "forced"),
    (300, 200, 4, 16, {"force_nch": 7}, "forced"),            # uneven chunks
    (512, 64, 2, 16, {"force_nch": 64}, "forced"),
    (2, 0x3fffffff // 16, 1, 16, {"force_nch": 1}, "forced"),         # the chunk-length guard: at the limit ...
    (2, 0x3fffffff // 16 + 1, 1, 16, {"force_nch": 1}, "refused"),    # ... and beyond
    (0x7ff00000 - 1, 0, 2, 16, {}, "paired"),                         # the pair-index guard: below ...
    (0x7ff00000, 0, 2, 16, {}, "refused"),                            # ... and at the limit
    (0x7ff00000 // 64, 64, 2, 16, {"force_nch": 8}, "refused"),
]


def _tag(A, B, G, kw, p):
    if p is None:
        return "refused"
    if B == 0:
        return "paired"
    if kw.get("force_nch", 0) > 0:
        return "forced"
    if p["rows_per_launch"] > 0:
        return "whole" if A % p["rows_per_launch"] == 0 else "partial"
    mg, nr = _mg(G, kw.get("wpc", 8)), _ranks(G, kw)
    return "fill" if nr >= 2 and A * p["nch"] == mg and p["nch"] % nr == 0 and B % p["nch"] == 0 else "one"


def _ranks(G, kw):
    wpc = kw.get("wpc", 8)
    wpb = LP.wave_group_wpb(kw.get("lds", 20000), N_CU * wpc, kw.get("wpb_knob", 0))
    return wpc // wpb if wpc % wpb == 0 else 0


@pytest.mark.parametrize("row", ADJ_ROWS, ids=["%dx%d_G%d_%s_%d" % (r[0], r[1], r[2], r[5], i) for i, r in enumerate(ADJ_ROWS)])
def test_the_adjoint_planner_is_what_both_launchers_computed(row):
    A, B, G, NUp, kw, tag = row
    got, want = plan_adjoint(A, B, G, NUp, **kw), _restated_adjoint(A, B, G, NUp, **kw)
    assert got == want, (got, want)
    assert _tag(A, B, G, kw, got) == tag, got
    if got is None:
        return
    mg = _mg(G, kw.get("wpc", 8))
    if B == 0:
        want_ppp = max(1, min(64, A // mg)) if kw.get("paired", True) else 1
        assert (got["ppp"], got["PPG"], got["rows_per_launch"], got["groups"]) == (want_ppp, want_ppp, 0, -(-A // want_ppp))
    else:
        assert got["ppp"] == 1 and got["groups"] == A * got["nch"] and got["nch"] == -(-B // got["PPG"])
    if tag == "forced":
        assert got["nch"] == kw["force_nch"] and got["rows_per_launch"] == 0
    if got["rows_per_launch"] > 0:      # every launch but a partial last one fills the chip exactly, with whole ranks of chunks per row
        nr = _ranks(G, kw)
        assert got["rows_per_launch"] * got["nch"] == mg and got["nch"] % nr == 0 and B % got["nch"] == 0 and got["PPG"] >= 4 * nr
        assert A >= got["rows_per_launch"]


def test_the_adjoint_table_reaches_every_branch():
    tags = [r[5] for r in ADJ_ROWS]
    plans = [plan_adjoint(r[0], r[1], r[2], r[3], **r[4]) for r in ADJ_ROWS]
    multi = sum(1 for p in plans if p is not None and p["rows_per_launch"] > 0)
    assert 5 * multi >= len(ADJ_ROWS), (multi, len(ADJ_ROWS))      # at least a fifth take several launches
    for G in (1, 2, 4, 8):
        for tag in ("fill", "whole", "partial"):
            assert any(r[2] == G and r[5] == tag for r in ADJ_ROWS), (G, tag)
    assert {"one", "paired", "forced", "refused"} <= set(tags)
    ppp = [p["ppp"] for r, p in zip(ADJ_ROWS, plans) if r[5] == "paired"]
    assert {1, 3, 63, 64} <= set(ppp)
    # the shape of the GPU test: three launches of 512 rows, eight chunks of eight pairs per row
    assert plan_adjoint(1536, 64, 2, 24) == dict(PPG=8, ppp=1, rows_per_launch=512, groups=12288, nch=8)


# ---- the one-draw plan ------------------------------------------------------------------------------------------------------------------
# 21000 bytes of LDS a wave: seven waves by LDS, four a workgroup -> 4 by LDS in whole workgroups; 9000 bytes: 16 by LDS, so that the
# registers decide (128: 16, 168: 12, 169: 8, 256: 8 -- and the cap of 8 on top).
# (P or a function of max_waves, lds, wpb0, vgprs, wpc knob, units = nb x NUp, pct, ws_stride)
def _one_draw_rows():
    rows = []
    for vgprs in (128, 168, 169, 256):
        for knob in (0, 12, 6):
            wpc = LP.one_draw_waves_per_cu(9000, 4, vgprs, knob)
            mw = N_CU * wpc
            rows += [(8 * mw - 1, 9000, 4, vgprs, knob, 80, 50, 1000), (8 * mw, 9000, 4, vgprs, knob, 80, 50, 1000)]
    mw = N_CU * 8
    rows += [(8 * mw - mw, 9000, 4, 256, 0, 80, 50, 1000),      # per = 7: the equal split
             (7 * mw + 1, 9000, 4, 256, 0, 80, 50, 1000),       # per = 8 with hardly any pair in the last share
             (mw - 1, 9000, 4, 256, 0, 80, 50, 1000),           # P < max_waves: a wave per pair
             (1, 9000, 4, 256, 0, 80, 50, 1000),
             (mw, 9000, 4, 256, 0, 80, 50, 1000),
             (10 * mw + 77, 9000, 4, 256, 0, 80, 50, 1000),     # P no multiple of per
             (3 * mw + 5, 9000, 4, 256, 0, 80, 50, 1000)]       # P no multiple of per, no counter: fewer waves than resident
    for pct in (1, 50, 99, 100):
        rows += [(20 * mw + 3, 9000, 4, 256, 0, 160, pct, 2000), (8 * mw, 21000, 4, 200, 0, 160, pct, 2000)]
    rows += [(16384, 41000, 3, 256, 0, 96, 50, 500),            # three waves a workgroup by LDS: 3 a CU
             (16384, 100000, 1, 256, 0, 96, 50, 500),           # one wave a CU
             (16384, 21000, 4, 256, 2, 96, 50, 500),            # the knob below a workgroup
             (mw * (0x1fffffff // 640), 9000, 4, 256, 0, 640, 50, 10),          # the share guard: at the limit ...
             (mw * (0x1fffffff // 640) + 1, 9000, 4, 256, 0, 640, 50, 10),      # ... and beyond (nb x NUp = 640 trips it)
             (0x7ff00000 - 1, 9000, 4, 256, 0, 8, 50, 0),                       # the pair-index guard
             (0x7ff00000, 9000, 4, 256, 0, 8, 50, 0)]
    return rows


OD_ROWS = _one_draw_rows()


@pytest.mark.parametrize("row", OD_ROWS, ids=["P%d_lds%d_v%d_k%d_pct%d" % (r[0], r[1], r[3], r[4], r[6]) for r in OD_ROWS])
def test_the_one_draw_plan_is_what_the_three_launchers_computed(row):
    P, lds, wpb0, vgprs, knob, units, pct, stride = row
    got, want = plan_one_draw(*row), _restated_one_draw(*row)
    assert got == want, (got, want)
    if got is None:
        assert P >= 0x7ff00000 or -(-P // min(P, N_CU * LP.one_draw_waves_per_cu(lds, wpb0, vgprs, knob))) > 0x1fffffff // units
        return
    mw = N_CU * got["wpc"]
    assert 1 <= got["wpc"] <= 8 and got["ws_doubles"] == min(P, mw) * stride
    if got["queue"]:      # a filled chip: every wave takes C0 pairs up front, the counter hands out the rest one by one
        assert got["waves"] == mw and got["per"] >= 8 and pct < 100
        assert got["C0"] == got["per"] * pct // 100 and got["q_first"] == mw * got["C0"] <= P
    else:                 # equal shares of `per`, the last one shorter: no more waves than that takes
        assert got["C0"] == got["per"] and got["q_first"] == P
        assert (got["waves"] - 1) * got["per"] < P <= got["waves"] * got["per"] and got["waves"] <= mw


def test_the_one_draw_table_reaches_every_branch():
    plans = [plan_one_draw(*r) for r in OD_ROWS]
    used = sum(1 for p in plans if p is not None and p["queue"])
    assert 3 * used >= len(OD_ROWS), (used, len(OD_ROWS))      # at least a third draw from the counter
    assert sum(1 for p in plans if p is None) == 2
    assert {p["wpc"] for p in plans if p is not None} >= {1, 2, 3, 4, 8}      # (a knob of 6 is 4 in whole workgroups of four)
    by_regs = {v: plan_one_draw(16384, 9000, 4, v, 12, 80, 50, 0)["wpc"] for v in (128, 168, 169, 256)}
    assert by_regs == {128: 8, 168: 8, 169: 8, 256: 8}         # the cap of two waves per SIMD holds whatever the registers allow
    assert [LP.waves_by_vgprs(16, v) for v in (128, 168, 169, 256)] == [16, 12, 8, 8]
    # one below 8 x max_waves the equal share is still 8 pairs: the counter is used from 7 x max_waves + 1 pairs on
    mw = N_CU * 8
    assert [plan_one_draw(P, 9000, 4, 256, 0, 80, 50, 0)["queue"] for P in (7 * mw, 7 * mw + 1, 8 * mw - 1, 8 * mw)] == [0, 1, 1, 1]
    # the derivative solver's fixed half is pct = 50: the same integer
    assert all(plan_one_draw(mw * per, 9000, 4, 256, 0, 80, 50, 0)["C0"] == per // 2 for per in range(8, 40))


# ---- seeded random shapes ---------------------------------------------------------------------------------------------------------------
def test_random_adjoint_shapes_restatement_equals_export_and_the_launches_tile_the_rows():
    rng = random.Random(20240)
    multi = 0
    for _ in range(3000):
        G, NUp = rng.choice([1, 2, 4, 8]), rng.choice([8, 16, 24, 32, 64])
        kw = dict(wpc=rng.choice([4, 8, 8, 8, 12]), wpb_knob=rng.choice([0, 0, 1, 2, 4]), lds=rng.choice([9000, 20000, 30000, 45000, 60000, 90000]),
                  n_cu=rng.choice([256, 256, 64, 8]), paired=rng.random() < 0.5)
        mg = kw["n_cu"] * kw["wpc"] * G
        if rng.random() < 0.2:
            A, B = rng.randrange(1, (200 if rng.random() < 0.3 else 3) * mg), 0
        else:
            B = rng.choice([rng.randrange(1, 300), rng.randrange(1, 3000), 64, 128, 256, 512, 640, 768, 1536])
            A = rng.randrange(1, max(2, 4 * mg // B + 50))
        kw["force_nch"] = rng.randrange(1, B + 1) if B > 0 and rng.random() < 0.25 else 0
        got, want = plan_adjoint(A, B, G, NUp, **kw), _restated_adjoint(A, B, G, NUp, **kw)
        assert got == want, (A, B, G, NUp, kw, got, want)
        rpl = got["rows_per_launch"]
        if rpl > 0:
            multi += 1
            # the launcher's loop: rows [a0, a0 + An), each launch planned again with the chunks per row forced
            seen = np.zeros(A, np.int32)
            for a0 in range(0, A, rpl):
                An = min(rpl, A - a0)
                seen[a0:a0 + An] += 1
                one = plan_adjoint(An, B, G, NUp, **dict(kw, force_nch=got["nch"]))
                assert one["nch"] == got["nch"] and one["PPG"] == got["PPG"] and one["groups"] == An * got["nch"] <= mg, (A, B, G, kw, one, got)
            assert seen.min() == 1 and seen.max() == 1
    assert multi >= 100, multi


def test_random_one_draw_shapes_restatement_equals_export():
    rng = random.Random(20241)
    used = 0
    for _ in range(3000):
        lds = rng.choice([9000, 14000, 21000, 30000, 41000, 60000, 100000])
        wpb0 = LP.wave_group_wpb(lds, 1 << 20, rng.choice([0, 1, 2, 4]))
        vgprs, knob, n_cu = rng.choice([64, 96, 128, 129, 168, 169, 200, 256, 300, 512]), rng.choice([0, 0, 2, 4, 6, 8, 12]), rng.choice([256, 64, 8])
        mw = n_cu * LP.one_draw_waves_per_cu(lds, wpb0, vgprs, knob)
        P = rng.choice([rng.randrange(1, mw + 5), rng.randrange(1, 20 * mw), 8 * mw, 8 * mw - 1, 7 * mw + 1, 7 * mw])
        row = (P, lds, wpb0, vgprs, knob, rng.choice([80, 96, 160, 640]), rng.choice([1, 35, 50, 99, 100]), rng.choice([0, 1000, 5000]))
        got, want = plan_one_draw(*row, n_cu=n_cu), _restated_one_draw(*row, n_cu=n_cu)
        assert got == want, (row, n_cu, got, want)
        used += got["queue"]
    assert used >= 500, used
