"""The truncated value-regime yardstick and tables without a GPU (tests/truncated_value_regimes.py): the CERTIFICATES of the long-double
yardstick -- its levels against the same recursion in mpmath at 50 digits, its gradient against central differences of its own levels --
the CPU restatement within the recorded distance on every measured case, tests/golden/truncated_value_regimes.json against the case
table, and the route table's rows against sk_route_query."""
import importlib.util
import json
import os

import numpy as np
import pytest

import truncated_value_regimes as T
from conftest import GOLDEN


def _measure_module():
    spec = importlib.util.spec_from_file_location("measure_truncated_value_regimes", os.path.join(GOLDEN, "measure_truncated_value_regimes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MEASURE = _measure_module()
with open(MEASURE.PATH) as _f:
    RECORDED = json.load(_f)
ENTRIES = T.golden_entries()
# one row per way the yardstick forms G and per order: the certificates run on their first pair of every family x parameter
CERTIFIED = ["plain-gram-3x2x20x17x3", "function_levels_order_2-gram-3x2x20x17x3", "function_levels_order_3-gram-3x2x20x17x3",
             "function_levels_order_4-gram-3x2x20x17x3", "plain_dim_12-gram-3x2x20x17x12", "points-gram-3x2x20x17x3", "points_dim_12-gram-3x2x20x17x12"]
CERT_CASES = [(rid, fam, lab) for rid in CERTIFIED for fam in T.MEASURED for lab, _ in T.FAMILIES[fam].get(T.ROW_BY_ID[rid]["variant"], [])]


def _first_pair(row, fam, lab):
    """(settings, the pair's PATHS x, y, what the yardstick works on): pair (0, 0) -- in the degenerate batch, whose path 0 is constant,
    pair (1, 1), the paths with repeated points"""
    st = dict(T.FAMILIES[fam][row["variant"]])[lab]
    X, Y = T.inputs(st, row)
    kx, ky = T.kernel_inputs(row, X, Y)
    i = 1 if fam == "degenerate" else 0
    return st, X[i], Y[i], kx[i], ky[i]


@pytest.mark.parametrize("rid, fam, lab", CERT_CASES, ids=["%s-%s-%s" % c for c in CERT_CASES])
def test_level_yardstick_against_mpmath_at_50_digits(rid, fam, lab):
    """<= 1e-15 of scale[m][pair] at every level (the scales themselves included): a thousand times below the GPU test's base.  Every
    family x parameter of the table holds it -- sigma = 1e12 too, where subtracting expl values would be off by 1e-9."""
    row = T.ROW_BY_ID[rid]
    st, _, _, kx, ky = _first_pair(row, fam, lab)
    c = T.level_certificate(row["variant"], st.get("sigma"), kx, ky, row["L"], row["order"])
    print(rid, fam, lab, "%.2e" % c)
    assert c <= 1e-15


@pytest.mark.parametrize("rid, fam, lab", [c for c in CERT_CASES if T.ROW_BY_ID[c[0]]["order"] == 1],
                         ids=["%s-%s-%s" % c for c in CERT_CASES if T.ROW_BY_ID[c[0]]["order"] == 1])
def test_gradient_yardstick_against_central_differences(rid, fam, lab):
    """<= 1e-11 of the path's largest entry, with h = 1e-6 of the path's largest step: the truncation of the central difference is
    h^2 = 1e-12 relative, its rounding 2^-64 / h = 5e-14"""
    row = T.ROW_BY_ID[rid]
    st, x, y, kx, ky = _first_pair(row, fam, lab)
    _, scale = T.want_levels(row["variant"], st.get("sigma"), kx[None], ky[None], row["L"])
    c = T.fd_certificate(row["variant"], st.get("sigma"), x, y, T.upstream_weights(scale)[:, 0, 0])
    print(rid, fam, lab, "%.2e" % c)
    assert c <= 1e-11


def test_upstream_weights_make_every_level_count():
    """w[m] scale[m] is O(1) at every level of every scaled case, from level 8 at 1e-291 to 1e45"""
    row = T.ROW_BY_ID["adjoint-gram-3x2x20x17x3"]
    for lab, _ in T.FAMILIES["scale"]["plain"]:
        want = T.case_want(row, "scale", lab)
        top = np.abs(want["w"]).reshape(row["L"], -1).max(1) * want["scale"][1:].reshape(row["L"], -1).max(1).astype(np.float64)
        assert np.all((top > 0.1) & (top < 10)), (lab, top)


def test_recorded_entries_are_the_case_table():
    assert set(RECORDED) - {"_provenance"} == set(ENTRIES)
    for key, (row, fam, lab, st) in ENTRIES.items():
        assert set(RECORDED[key]) == {"value"} | ({n for n in ("dX", "dY") if n in row["outputs"]}), key
        assert len(RECORDED[key]["value"]) == row["L"] + 1


@pytest.mark.parametrize("key", sorted(ENTRIES))
def test_restatement_within_the_recorded_distance(key):
    """On the CPU the fp64 restatement is within 1e-12 + r of the yardstick per level and pair (1e-10 + r per path for its autograd
    gradients), r the recorded distance -- the json holds what the committed script measures here (seed 0; `offset` records the maximum
    over 8 seeds, never less)"""
    row, fam, lab, st = ENTRIES[key]
    got, rec = MEASURE.distance(row, fam, lab, 0), RECORDED[key]
    print(key, got, rec)
    assert np.all(np.asarray(got["value"]) <= T.VALUE_BASE + np.asarray(rec["value"])), (got["value"], rec["value"])
    for name in ("dX", "dY"):
        if name in got:
            assert got[name] <= T.GRAD_BASE + rec[name], (name, got[name], rec[name])


@pytest.mark.parametrize("row", T.ROWS, ids=[r["id"] for r in T.ROWS])
def test_rows_are_in_the_scope_the_route_query_states(row):
    """every row's shape is served by the HIP kernel as given (FUSED, on (X, Y) and for a gradient row on (Y, X) too: dY), so that the
    GPU test cannot silently compare the torch restatement with the yardstick"""
    from sigkernel_amd import _lib
    q = _lib.load().sk_route_query
    routes = [row["route"]] + ([row["forward_route"]] if "forward_route" in row else [])
    for op, order, D, M, N, L in routes:
        flags = _lib.ROUTE_NO_SWAP if op == "OP_TRUNCATED_LONG" else 0
        sides = [(M, N)] + ([(N, M)] if T.is_gradient(row) and row["op"] != "sym" else [])
        for m, n in sides:
            got = q(getattr(_lib, op), order, D, m, n, L, 0, 4 if row["f32"] else 8, flags)
            if op == "OP_TRUNCATED_LONG" and T.is_gradient(row):
                assert got in (_lib.ROUTE_FUSED, _lib.ROUTE_FUSED_SWAP), (op, m, n, got)
            else:
                assert got == _lib.ROUTE_FUSED, (op, order, D, m, n, L, got)
