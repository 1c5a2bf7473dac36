"""tests/loss_batch_shapes.py on the CPU: the blockwise yardstick against value_regimes.mmd_ld and against plain loops, the recorded
file against the tables, every table through the oracle-backed back-end (a typo in a table fails here, not on the GPU box), and the
restated launch plan: its lane-group chunks partition the pairs, and the large shapes have -- on a 256-CU device -- the properties
tests/test_gpu_loss_batch_shapes.py runs them for."""
import json
import os

import numpy as np
import pytest
import torch

import loss_batch_shapes as S
import value_regimes as V
from conftest import GOLDEN

with open(os.path.join(GOLDEN, "loss_batch_shapes.json")) as _f:
    RECORDED = json.load(_f)
LD_AGREEMENT = 1e-15      # two long-double evaluations of one formula in another summation order -- 2^-64 = 5e-20 per operation, a few hundred
                          # terms per path, the K_XX and K_XY parts of a gradient cancelling to a tenth or less: five decades below the GPU bars
PCT = {"linear": 35, "rbf": 20}      # fused_static_share_{linear,rbf} of the library's cost table (asserted below)


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A, B", [(5, 4), (18, 3)], ids=["5x4", "18x3_two_blocks"])
@pytest.mark.parametrize("kind", S.KINDS)
def test_the_blockwise_yardstick_is_mmd_ld(kind, A, B):
    X, Y = S.walks(A, 7, 3, 11, S.STEP_X), S.walks(B, 7, 3, 12, S.STEP_Y)
    sigma = S.sigma_of(kind)
    v0, g0 = V.mmd_ld(kind, sigma, X, Y, 1)
    v1, g1, pairs = S.loss_ld(kind, sigma, X, Y, 1, True)
    assert V.value_error(v1, v0) <= LD_AGREEMENT and V.grad_error(g1, g0) <= LD_AGREEMENT
    # the pairs, one by one, in the one-launch route's order: the rectangle row-major, then i < j row-major
    Z = np.concatenate([X, Y])
    order = [(Z[a], Z[b]) for a in range(A) for b in range(A + B)] + [(Y[i], Y[j]) for i in range(B) for j in range(i + 1, B)]
    assert len(order) == len(pairs)
    one = np.array([V.gram_ld(kind, sigma, x[None], y[None], 1)[0][0, 0] for x, y in order], dtype=V.LD)
    assert V.value_error(pairs, one) <= LD_AGREEMENT
    # without the triangle: the scoring rules; a one-path y
    v2, g2, p2 = S.loss_ld(kind, sigma, X, Y[:1], 1, False)
    Kxx, gxx = V.gram_ld(kind, sigma, X, X, 1, V._wxx(A))
    Kxy, gxy = V.gram_ld(kind, sigma, X, Y[:1], 1, np.full((A, 1), -2.0 / A))
    assert V.value_error(v2, (Kxx * V._wxx(A)).sum() - 2 * Kxy.mean()) <= LD_AGREEMENT and V.grad_error(g2, 2 * gxx + gxy) <= LD_AGREEMENT
    assert len(p2) == A * (A + 1)


def test_the_triangle_order_is_the_double_loop():
    for n in (1, 2, 3, 7, 46):
        i, j = S.triangle_pairs(n)
        assert list(zip(i.tolist(), j.tolist())) == [(a, b) for a in range(n) for b in range(a + 1, n)]


@pytest.mark.parametrize("kind", S.KINDS)
def test_the_paired_yardstick_is_the_sum_over_single_pairs(kind):
    X, Y = S.walks(3, 6, 2, 21, S.STEP_X), S.walks(3, 6, 2, 22, S.STEP_Y)
    sigma = S.sigma_of(kind)
    v, g = S.distance_ld(kind, sigma, X, Y, 0)
    one = np.ones((1, 1))
    want_v, want_g = V.LD(0), np.zeros(X.shape, dtype=V.LD)
    for i in range(3):
        kxx, gxx = V.gram_ld(kind, sigma, X[i:i + 1], X[i:i + 1], 0, one)      # (the first argument only)
        kxy, gxy = V.gram_ld(kind, sigma, X[i:i + 1], Y[i:i + 1], 0, one)
        kyy = V.gram_ld(kind, sigma, Y[i:i + 1], Y[i:i + 1], 0)[0]
        want_v += (kxx[0, 0] + kyy[0, 0] - 2 * kxy[0, 0]) / 3
        want_g[i] = (gxx[0] - 2 * gxy[0]) / 3
    assert V.value_error(v, want_v) <= LD_AGREEMENT and V.grad_error(g, want_g) <= LD_AGREEMENT


def test_wb_closed_form():
    w = S.wb_closed_form(3, 2).reshape(3, 5)
    assert np.array_equal(w[:, :3], (1 - np.eye(3)) * (2.0 * (1.0 / 6.0))) and np.array_equal(w[:, 3:], np.full((3, 2), -2.0 / 6.0))


# ---- the tables ---------------------------------------------------------------------------------------------------------------------------
def test_the_recorded_file_holds_exactly_the_cases_of_the_tables():
    assert set(RECORDED) - {"_provenance"} == set(S.golden_entries())
    for key, (c, kind) in S.golden_entries().items():
        need = {"sym": {"value"}, "pairs": {"value", "loss"}, "pairs_yy": {"value", "loss"}}.get(c["wrapper"], {"value", "grad"})
        assert need <= set(RECORDED[key]), key
        assert all(0 <= RECORDED[key][n] < 1e-12 for n in need), (key, RECORDED[key])      # the oracle is a double-precision solver, not a bound to hide behind


def test_the_tables_are_what_the_issue_lists():
    shapes = lambda wr: [(c["A"], c["B"]) for c in S.SMALL if c["wrapper"] == wr]
    assert shapes("mmd") == [(2, 2), (3, 2), (2, 7), (7, 2), (5, 4), (9, 8), (17, 16), (33, 32)]
    assert shapes("esr") == [(2, 1), (2, 3), (5, 4), (16, 1), (33, 32)] and shapes("sr") == [(2, 1), (3, 1), (8, 1), (64, 1)]
    assert {c["A"] + c["B"] for c in S.SMALL} == {3, 4, 5, 9, 17, 33, 65}
    for table in (S.SMALL, S.PER_PAIR, S.DISTANCE):
        assert all(6 <= c["M"] <= 9 and c["D"] in (2, 3) for c in table) and {c["d"] for c in table} == {0, 1}
    cases = S.small_cases()
    assert {(c["wrapper"], c["A"], c["B"], k) for c, k, r in cases if r == "one_launch"} == {(c["wrapper"], c["A"], c["B"], k) for c in S.SMALL for k in S.KINDS}
    for route in S.ROUTES[1:]:
        sub = [(c, k) for c, k, r in cases if r == route]
        assert {3, 33} <= {c["A"] + c["B"] for c, _ in sub} and {k for _, k in sub} == set(S.KINDS)
    assert [(c["A"], c["B"]) for c in S.PER_PAIR[::2]] == [(5, 4), (23, 46), (64, 129)]
    assert [c["A"] for c in S.SYM] == [2, 3, 45, 46, 182, 363] and all(c["M"] == 4 and c["d"] == 0 for c in S.SYM)
    assert [c["A"] for c in S.DISTANCE] == [1, 2, 5, 33]
    assert any(not c["knobs"] for c, _, _ in S.large_cases()) and any(c["upstream"] != 1.0 for c, _, _ in S.large_cases())
    assert all(c["M"] == 8 and c["D"] == 3 and c["d"] == 1 for c, _, _ in S.large_cases())


def _held(c, kind, got_value, got_grad):
    value, grad, _ = S.want(c, kind)
    ev, eg = V.value_error(got_value, value), V.grad_error(got_grad / c["upstream"], grad)
    tv, tg = S.tolerance(RECORDED, c, kind, "value"), S.tolerance(RECORDED, c, kind, "grad")
    assert ev <= tv and eg <= tg, "%s: value %.3e (bound %.3e), gradient %.3e (bound %.3e)" % (S.case_key(c, kind), ev, tv, eg, tg)


WRAPPER_CASES = [(c, k) for c in S.SMALL + S.DISTANCE + [S.DISTANCE_UNMERGED] for k in S.KINDS] + [(c, k) for c, k, _ in S.large_cases()[:2]]


@pytest.mark.parametrize("c, kind", WRAPPER_CASES, ids=[S.case_key(c, k) for c, k in WRAPPER_CASES])
def test_every_wrapper_case_through_the_oracle_backend(c, kind, oracle_backend):
    v, g, gy = S.call_wrapper(c, kind, "cpu")
    assert gy is None and g.shape == (c["A"], c["M"], c["D"])
    _held(c, kind, v, g)


@pytest.mark.parametrize("c", S.SYM[:4], ids=["A%d" % c["A"] for c in S.SYM[:4]])
@pytest.mark.parametrize("kind", S.KINDS)
def test_every_symmetric_case_through_the_oracle_backend(c, kind, oracle_backend):
    import sigkernel_amd
    X = torch.from_numpy(S.inputs(c)[0])
    K = sigkernel_amd.SigKernel(sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(S.SIGMA), 0).compute_Gram(X, X, sym=True)
    assert torch.equal(K, K.t())
    assert V.value_error(K.numpy(), S.want(c, kind)[2]) <= S.tolerance(RECORDED, c, kind, "value")


def test_the_per_pair_cases_have_the_pair_counts_they_are_there_for():
    for c in S.PER_PAIR:
        for kind in S.KINDS:
            _, _, pairs = S.want(c, kind)
            assert len(pairs) == c["A"] * (c["A"] + c["B"]) + (c["B"] * (c["B"] - 1) // 2 if c["wrapper"] == "pairs_yy" else 0)
    counts = lambda A, B: (A * (A + B), B * (B - 1) // 2)      # rectangle, triangle
    assert 1024 < counts(23, 46)[1] < counts(23, 46)[0] < 8192 < counts(64, 129)[1] < counts(64, 129)[0]      # k_loss_value: LV_THREADS, LV_THREADS * LV_BATCH


# ---- the launch plan ------------------------------------------------------------------------------------------------------------------------
def test_the_static_shares_are_the_cost_tables():
    from sigkernel_amd import _lib
    assert {k: int(_lib.cost("fused_static_share_" + k)) for k in S.KINDS} == PCT
    assert int(_lib.cost("fused_mid_min_pairs_per_rank")) == 4      # (forward_plan's `ranked`)


def _plans(c, kind, n_cu=S.N_CU):
    geo = S.loss_geometry(kind, c["M"], c["D"], c["d"])
    return [S.forward_plan(kind, c["A"], c["B"], c["M"], c["D"], c["d"], True, w, n_cu, PCT[kind])
            for w in S.waves_per_cu(geo, int(c["knobs"].get("SK_FUSED_WPC", 0)))]


@pytest.mark.parametrize("n_cu", [256, 64, 7])
def test_the_lane_group_chunks_partition_the_pairs(n_cu):
    cases = [(c, k) for c, k, _ in S.large_cases()] + [(c, k) for c in S.SMALL for k in S.KINDS if c["wrapper"] == "mmd"]
    queues = 0
    for c, kind in cases:
        geo = S.loss_geometry(kind, c["M"], c["D"], c["d"])
        for wpc in (1, 2, 4):
            p = S.forward_plan(kind, c["A"], c["B"], c["M"], c["D"], c["d"], True, min(wpc, (160 * 1024) // geo["lds"]), n_cu, PCT[kind])
            seen = np.zeros(p["P"], np.int32)
            for lo, hi in S.chunk_intervals(p):
                seen[lo:hi] += 1
            assert seen.min() == 1 and seen.max() == 1, (c, kind, wpc, p)
            queues += p["queue"]
    assert queues > 0


def test_the_large_shapes_have_their_properties_on_256_cus():
    for c, kind, props in S.large_cases():
        plans = _plans(c, kind)
        assert len(plans) == 1, "LDS holds these variants to 4 waves per CU: one plan, whatever the registers"
        p = plans[0]
        assert S.straddlers(p) == [props["straddle"]], (S.case_key(c, kind), S.straddlers(p))
        assert bool(p["queue"]) == props["queue"]
        if props["queue"]:      # the straddling chunk is a drawn one
            assert props["straddle"][0] >= p["q_first"] and (props["straddle"][0] - p["q_first"]) % (1 << p["logC"]) == 0
        Bz = c["A"] + c["B"]
        ppg = S.pick_chunk(c["A"], Bz, S.N_CU * 8 * 8)      # the one-band adjoints: 8 waves per CU of 8 lane groups at these lengths
        chunks = -(-Bz // ppg)
        assert ppg > 1 and (Bz % chunks != 0) == props["uneven"], (S.case_key(c, kind), ppg, chunks)
    every = [props for _, _, props in S.large_cases()]
    natural = [props for c, _, props in S.large_cases() if not c["knobs"]]
    assert any(p["queue"] for p in every) and any(p["uneven"] for p in natural) and all(p["straddle"] for p in every)


def test_the_candidate_127_plus_128_does_not_straddle_without_a_knob():
    """why the natural row is 127 + 129: at 127 + 128 pair 32 385 opens a lane-group chunk"""
    c = S.case("mmd", 127, 128, 8, 3, 1)
    for kind in S.KINDS:
        (p,) = _plans(c, kind)
        assert S.straddlers(p) == [] and any(lo == p["P_rect"] for lo, _ in S.chunk_intervals(p))


def test_the_small_shapes_run_one_pair_per_adjoint_chunk():
    for c in S.SMALL + S.PER_PAIR:
        assert S.pick_chunk(c["A"], c["A"] + c["B"], S.N_CU * 8 * 8) == 1      # (8 waves per CU of 8 lane groups)
