"""The value-regime yardstick and inputs, without a GPU (tests/value_regimes.py): the long-double yardstick against the CPU oracle on
unit walks, its diagonal sweep against ld_reference's plain loop, the exponent census of the drift inputs, and
tests/golden/value_regimes.json -- the oracle's distance from the yardstick that the GPU test's bounds rest on -- recomputed."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import ld_reference as L
import value_regimes as V
from conftest import GOLDEN


def _measure_module():
    spec = importlib.util.spec_from_file_location("measure_value_regimes", os.path.join(GOLDEN, "measure_value_regimes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MEASURE = _measure_module()
with open(MEASURE.PATH) as _f:
    RECORDED = json.load(_f)
ENTRIES = V.golden_entries()


@pytest.mark.parametrize("kind, sigma", [("linear", None), ("rbf", 0.8)])
def test_yardstick_agrees_with_the_oracle_on_unit_walks(kind, sigma):
    """7e-14 (values) and 3e-14 (gradients) is what the analytic long-double gradient measured against the double oracle on unit walks of
    the base shape; a factor 4 on top."""
    X, Y, w, _ = V.inputs({}, V.BASE, seed=0)
    dist = MEASURE.oracle_distance(kind, X, Y, w, sigma, V.BASE["d"])
    print(kind, dist)
    assert dist["value"] <= 4 * 7e-14 and dist["grad"] <= 4 * 3e-14, dist


@pytest.mark.parametrize("kind, sigma", [("linear", None), ("rbf", 0.8)])
def test_yardstick_is_the_reference_formula_in_long_double(kind, sigma):
    """On unit walks (where forming the static kernel the reference's way costs nothing in long double) the yardstick's pieces are
    ld_reference's, and the diagonal sweep returns the plain loop's bits."""
    X, Y, w, _ = V.inputs({}, V.shape(2, 3, 7, 6, 3, 1), seed=1)
    inc, _ = V.increments_ld(kind, sigma, X, Y)
    fine = V.tile(inc, 1)
    assert np.array_equal(V.solve_diag_ld(fine), L._solve_fine_ld(fine, False))
    assert np.array_equal(V.weights_ld(inc, 1)[1], L.adjoint_weights_ld(inc, 1, False))
    ref_inc = L._corner(L._static_ld(kind, sigma, X, Y, True))
    assert float(np.max(np.abs(inc - ref_inc))) <= 1e-17
    # the analytic gradient against the reference's finite-difference formula in long double: its O(h) truncation, h = 1e-9
    K, g = V.gram_ld(kind, sigma, X, Y, 1, w)
    fd = np.einsum("ab,abmd->amd", w.astype(L.LD), L.grad_points_ld(kind, sigma, X, Y, 1, False))
    assert V.grad_error(fd, g) <= 1e-7


def test_exact_weights_are_the_discrete_solvers_gradient():
    """exact_weights_ld against torch autograd through the plain double loop (tests/exact_gradient_reference.py)"""
    import exact_gradient_reference as E
    X, Y, w, _ = V.inputs({}, V.shape(1, 1, 5, 4, 2, 1), seed=2)
    inc, _ = V.increments_ld("linear", None, X, Y)
    K, W = V.exact_weights_ld(inc, 1)
    t = torch.from_numpy(inc[0, 0].astype(np.float64)).requires_grad_(True)
    k = E.forward_torch(t, 1)
    k.backward()
    assert abs(float(K[0, 0]) - float(k.detach())) <= 1e-14 * abs(float(k.detach()))
    assert float(np.max(np.abs(W[0, 0].astype(np.float64) - t.grad.numpy()))) <= 1e-14 * float(t.grad.abs().max())


def _drift_shapes():
    seen = {}
    for row, sh, kind, fam, lab, st in V.route_cases():
        if fam == "drift":
            seen.setdefault(V.shape_key(sh), sh)
    return sorted(seen.items())


@pytest.mark.parametrize("key, sh", _drift_shapes(), ids=[k for k, _ in _drift_shapes()])
def test_drift_census_covers_every_band_of_the_exponential(key, sh):
    """The drift cases of every shape together put at least 8 nodes into each band of the exponent (normal, deep, subnormal results,
    zero, clamped), and s = 30 alone reaches the last three."""
    per = {}
    for lab, st in V.FAMILIES["drift"]["rbf"]:
        X, Y, _, sigma = V.inputs(st, sh, seed=0)
        per[lab] = V.census(X, Y, sigma)
    total = {b: sum(c[b] for c in per.values()) for b in V.BANDS}
    print(key, per)
    assert all(total[b] >= 8 for b in V.BANDS), total
    assert all(per["s=30"][b] > 0 for b in V.BANDS[2:]), per["s=30"]


def test_recorded_entries_are_the_case_table():
    assert set(RECORDED) - {"_provenance"} == set(ENTRIES)


@pytest.mark.parametrize("key", sorted(ENTRIES))
def test_recorded_oracle_distance_reproduces(key):
    """value_regimes.json holds what the committed script measures here, within a factor 2 (the oracle's rounding moves with the libm
    and the BLAS underneath it, not by more)."""
    got, rec = MEASURE.measure(*ENTRIES[key]), RECORDED[key]
    print(key, got, rec)
    for name in ("value", "grad"):
        floor = 1e-15      # (a distance of a few ulps is a coin toss: both sides within 2x of each other above that)
        assert got[name] <= 2 * rec[name] + floor and rec[name] <= 2 * got[name] + floor, (name, got, rec)
