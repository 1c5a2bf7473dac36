"""The wide-path case table without a GPU (tests/wide_value_regimes.py): every tiling boundary is in the table, the drift inputs still
reach the subnormal results and the clamp at these dims, tests/golden/wide_value_regimes.json -- the distance of the reference's
arithmetic from the long-double yardstick that the GPU test's bounds rest on -- recomputed, and the exact claims of the GPU test on the
CPU restatement of the kernel's arithmetic."""
import json
import os

import numpy as np
import pytest

import value_regimes as V
import wide_value_regimes as WV
from conftest import GOLDEN

with open(os.path.join(GOLDEN, "wide_value_regimes.json")) as _f:
    RECORDED = json.load(_f)


def test_every_listed_value_is_in_every_mode_and_static_kernel():
    """(M, N), batches, D: each listed value in at least one case per mode and static kernel; fp32 on drift and scale only; LinearKernel's
    s = 10 nowhere; about 150 cases."""
    sizes = {(2, 2), (64, 65), (65, 64), (127, 3), (66, 129)}
    batches = {(True, 2, 1), (True, 1, 4), (True, 2, 5), (True, 1, 8), (False, 3, 3)}
    dims = {33, 34, 39, 40, 41, 72}
    for mode in WV.MODES:
        for kind in V.KINDS:
            mine = [c for c in WV.CASES if c[0] == mode and c[1] == kind]
            gs = [c[5] for c in mine]
            assert {(g["M"], g["N"]) for g in gs} == sizes
            assert {(g["gram"], g["A"], g["B"]) for g in gs} == batches
            assert {g["D"] for g in gs} == dims
            assert {(c[2], c[3]) for c in mine} == {(f, lab) for f, lab, st in V.family_cases(kind) if not st.get("wild")}
            assert {c[2] for c in mine if c[6]} == ({"drift", "scale"} if kind == "rbf" else {"scale"})
            for fam in ("drift", "scale"):      # fp64 AND fp32 of every drift and scale parameter
                labs = {c[3] for c in mine if c[2] == fam}
                assert labs == {c[3] for c in mine if c[2] == fam and c[6]}
    assert not any(c[4].get("wild") for c in WV.CASES)
    assert 140 <= len(WV.CASES) <= 160, len(WV.CASES)


def test_linear_offset_cases_get_base_alone():
    for c in WV.CASES:
        tol = WV.tolerance(c, RECORDED)
        if c[1] == "linear" and c[2] == "offset":
            assert tol == (WV.INC_BASE if c[0] == "inc" else WV.GRAD_BASE)
        else:
            assert tol >= (WV.INC_BASE if c[0] == "inc" else WV.GRAD_BASE)


def _drift_geometries():
    seen = {}
    for c in WV.CASES:
        if c[2] == "drift":
            seen.setdefault(WV.geometry_key(c[5]), c[5])
    return sorted(seen.items())


@pytest.mark.parametrize("key, g", _drift_geometries(), ids=[k for k, _ in _drift_geometries()])
def test_drift_census_covers_every_band_at_these_dims(key, g):
    """as tests/test_value_regimes_host.py: the drift cases of a geometry together put at least 8 nodes into each band of the exponent, and
    s = 30 alone reaches the subnormal results, the zeros and the clamp (paired geometries: the diagonal pairs)"""
    per = {}
    for lab, st in V.FAMILIES["drift"]["rbf"]:
        X, Y, _, sigma = V.inputs(st, WV._shape(g, False), seed=0)
        if g["gram"]:
            per[lab] = V.census(X, Y, sigma)
        else:
            cs = [V.census(X[a:a + 1], Y[a:a + 1], sigma) for a in range(g["A"])]
            per[lab] = {b: sum(c[b] for c in cs) for b in V.BANDS}
    total = {b: sum(c[b] for c in per.values()) for b in V.BANDS}
    print(key, per)
    assert all(total[b] >= 8 for b in V.BANDS), total
    assert all(per["s=30"][b] > 0 for b in V.BANDS[2:]), per["s=30"]


def test_recorded_entries_are_the_case_table():
    assert set(RECORDED) - {"_provenance"} == set(WV.CASE_BY_KEY) | set(WV.FV_KEYS)


@pytest.mark.parametrize("key", sorted(WV.CASE_BY_KEY))
def test_recorded_reference_distance_reproduces(key):
    """wide_value_regimes.json holds what the committed script measures here, within a factor 2 (the rounding of the restatements moves with
    the libm and the BLAS underneath them, not by more)."""
    got, rec = WV.measure(WV.CASE_BY_KEY[key]), RECORDED[key]
    print(key, got, rec)
    floor = 1e-15
    assert got <= 2 * rec + floor and rec <= 2 * got + floor, (got, rec)


@pytest.mark.parametrize("case", WV.FV_CASES, ids=["%s-%s-%s" % c[:3] for c in WV.FV_CASES])
def test_recorded_function_valued_distance_reproduces(case):
    for key, got in WV.fv_measure(case).items():
        rec = RECORDED[key]
        print(key, got, rec)
        assert got <= 2 * rec + 1e-15 and rec <= 2 * got + 1e-15, (key, got, rec)


def test_rbf_sqr_yardstick_is_the_class_formula():
    """(x - y)(x + y) is x^2 - y^2: on unit walks the long-double kernel from differences equals the product of the two RBF kernels on x
    and x^2 in double to a few ulps of the node scale"""
    c = next(c for c in WV.FV_CASES if c[0] == "rbf_sqr" and c[2] == "s=3")
    assert WV.fv_reference_distance(c)["value"] <= 4 * 7e-14      # (tests/test_value_regimes_host.py's figure for the yardstick on unit walks)


@pytest.mark.parametrize("kind, sigma", [("linear", None), ("rbf", 0.8)])
def test_restatement_agrees_with_the_yardstick_on_unit_walks(kind, sigma):
    """the CPU restatement of the kernel's arithmetic (the exact claims below run on it) is the operation the yardstick computes: on unit
    walks within 4 x 2^-53 D of the node scale"""
    g = WV.geometry(2, 5, 20, 17, 40)
    X, Y, _, _ = V.inputs({}, WV._shape(g, False), seed=1)
    inc, G = V.increments_ld(kind, sigma, X, Y)
    assert WV.increments_error(WV.restate(kind, sigma, X, Y), inc, WV.scale_of(kind, inc, G)) <= 4 * 2.0 ** -53 * g["D"]


def test_a_repeated_point_gives_exactly_zero_linear_increments_on_the_restatement():
    X, Y, _, _ = WV.exact_inputs()
    X, Y = X.copy(), Y.copy()
    (a, p), (b, q) = WV.REPEAT_X, WV.REPEAT_Y
    X[a, p + 1], Y[b, q + 1] = X[a, p], Y[b, q]
    inc = WV.restate("linear", None, X, Y)
    assert np.all(inc[a, :, p] == 0) and np.all(inc[:, b, :, q] == 0)
    assert np.count_nonzero(inc) == inc.size - inc[a, :, p].size - inc[:, b, :, q].size + inc[a, b, p, q].size


def test_nodes_below_the_subnormal_limit_contribute_exactly_zero_on_the_restatement():
    c = next(c for c in WV.CASES if c[0] == "inc" and c[2] == "drift" and c[3] == "s=30" and not c[6])
    X, Y, _, _, sigma = WV.case_inputs(c)
    dead = WV.dead_increments(X, Y, sigma, c[5]["gram"])
    inc = WV.restate("rbf", sigma, X, Y)
    if not c[5]["gram"]:
        inc = inc[np.arange(X.shape[0]), np.arange(X.shape[0])]
    assert dead.sum() >= 8
    assert np.all(inc[dead] == 0)


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("side", ["X", "Y"])
@pytest.mark.parametrize("kind, sigma", [("linear", None), ("rbf", 0.8)])
def test_a_non_finite_coordinate_reaches_what_touches_its_node_on_the_restatement(kind, sigma, side, bad):
    """the rows (columns) around the node are NaN (LinearKernel with an inf coordinate: +-inf or NaN -- inf times a finite step), every
    other increment keeps its bits"""
    X, Y, _, _ = WV.exact_inputs()
    clean = WV.restate(kind, sigma, X, Y)
    Xb, Yb = X.copy(), Y.copy()
    path, node = WV.BAD_X if side == "X" else WV.BAD_Y
    (Xb if side == "X" else Yb)[path, node, WV.BAD_DIM] = bad
    got = WV.restate(kind, sigma, Xb, Yb)
    mask, _, _ = WV.touched(X.shape[1], Y.shape[1], WV.EXACT_GEOMETRY, side, path, node)
    assert 0 < mask.sum() < mask.size
    if kind == "linear" and np.isinf(bad):
        assert not np.any(np.isfinite(got[mask]))
    else:
        assert np.all(np.isnan(got[mask]))
    assert np.array_equal(got[~mask], clean[~mask])
