"""The derivative Gram's yardstick, case table and recorded bounds, without a GPU (tests/deriv_value_regimes.py): the long-double
three-state sweep against its own central differences, against value_regimes.gram_ld and against the oracle's solver; the oracle's
exact zero for gamma = 0; tests/golden/deriv_value_regimes.json -- the oracle's distance from the yardstick that the GPU test's bounds
rest on -- regenerated bit for bit, and the share of its entries that judge anything; the oracle-backed fake backend held to those bounds
through the API."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import deriv_value_regimes as DV
import value_regimes as V
from conftest import GOLDEN


def _measure_module():
    spec = importlib.util.spec_from_file_location("measure_deriv_value_regimes", os.path.join(GOLDEN, "measure_deriv_value_regimes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MEASURE = _measure_module()
with open(MEASURE.PATH) as _f:
    RECORDED = json.load(_f)
ENTRIES = DV.golden_entries()
YARD_SHAPE = DV.shape(3, 2, 8, 7, 2, 3)      # test_derivatives.py::test_oracle_derivatives_are_derivatives' sizes, dyadic 3


def _unit(kind):
    (lab, st), = DV.FAMILIES["unit"][kind]
    return st


# ------------------------------------------------------------------------------------------------------------------- the yardstick
@pytest.mark.parametrize("kind", DV.KINDS)
def test_yardstick_derivatives_are_derivatives_of_its_own_k(kind):
    """k_gamma and k_gamma_gamma against central differences (h = 1e-3) of the yardstick's k along gamma, to 2e-3 -- the statement
    test_oracle_derivatives_are_derivatives makes of the oracle -- and k with value_regimes.gram_ld's bits."""
    X, Y, g, X1, X2, sigma = DV.inputs(_unit(kind), YARD_SHAPE, seed=2)
    d = YARD_SHAPE["d"]
    k, kd, kdd = DV.kgrad_ld(kind, sigma, X, X1, X2, Y, d)
    k0, _ = V.gram_ld(kind, sigma, X, Y, d)
    assert np.array_equal(k, k0)
    h = 1e-3
    kp, _ = V.gram_ld(kind, sigma, X + h * g, Y, d)
    km, _ = V.gram_ld(kind, sigma, X - h * g, Y, d)
    e1, e2 = DV.error((kp - km) / (2 * h), kd), DV.error((kp - 2 * k0 + km) / h ** 2, kdd)
    print(kind, e1, e2)
    assert e1 <= 2e-3 and e2 <= 2e-3, (e1, e2)


@pytest.mark.parametrize("kind", DV.KINDS)
def test_yardstick_solver_is_the_oracles_solver(kind):
    """The solver half alone, without the 1 / eps^2 amplification: on the yardstick's three increment arrays rounded to double the
    long-double sweep and oracle.solve_deriv_coarse agree to 1e-13 on k and 1e-12 on k_gamma, k_gamma_gamma."""
    from oracle import oracle as O
    X, Y, g, X1, X2, sigma = DV.inputs(_unit(kind), YARD_SHAPE, seed=2)
    d = YARD_SHAPE["d"]
    inc3 = [a.astype(np.float64) for a in DV.deriv_increments_ld(kind, sigma, X, X1, X2, Y)]
    want = DV.solve_deriv_diag_ld(*(V.tile(a, d) for a in inc3))
    err = DV.errors(O.solve_deriv_coarse(inc3[0], inc3[1], inc3[2], d), want)
    print(kind, err)
    assert err["k"] <= 1e-13 and err["k_gamma"] <= 1e-12 and err["k_gamma_gamma"] <= 1e-12, err


def test_stacked_sweep_has_the_bits_of_single_sweeps():
    sh = DV.SHORT
    draws = []
    for seed in (0, 1):
        X, Y, g, X1, X2, sigma = DV.inputs(_unit("rbf"), sh, seed)
        draws.append((X, X1, X2, Y, sigma))
    both = DV.stacked_want("rbf", draws, sh["d"])
    for n, (X, X1, X2, Y, sigma) in enumerate(draws):
        for a, b in zip(both, DV.kgrad_ld("rbf", sigma, X, X1, X2, Y, sh["d"])):
            assert np.array_equal(a[n], b)


@pytest.mark.parametrize("kind", DV.KINDS)
def test_oracle_k_gamma_is_exactly_zero_for_gamma_zero(kind):
    """increments(-c G) + increments(c G) cancels bitwise: the oracle's k_gamma for gamma = 0 is exactly 0 (the GPU test asks the
    kernels for the same bits), and k is the k of any other gamma."""
    X, Y, g, X1, X2, sigma = DV.inputs(_unit(kind), DV.SHORT, seed=0)
    k, kd, kdd = MEASURE.oracle_kgrad(kind, sigma, X, Y, np.zeros_like(g), DV.SHORT["d"])
    assert np.all(kd == 0.0)
    assert np.array_equal(k, MEASURE.oracle_kgrad(kind, sigma, X, Y, g, DV.SHORT["d"])[0])


# ------------------------------------------------------------------------------------------------------------------- the recorded bounds
def test_recorded_entries_are_the_case_table():
    assert set(RECORDED) - {"_provenance"} == set(ENTRIES)
    for key, (fam, lab, kind, sh, st) in ENTRIES.items():
        assert set(RECORDED[key]) == set(DV.outputs_of(sh)) | ({DV.F32_STAGE} if sh["f32"] else set()), key


def test_gpu_seed_is_a_recorded_seed():
    assert 0 <= DV.GPU_SEED < DV.SEEDS == 8


def test_judged_share():
    """An output of a case is judged when the oracle itself is within JUDGED_CAP = 1e-5 of the yardstick there: every k, at least 85 % of
    all entries, at least 80 % of the k_gamma_gamma entries."""
    assert DV.JUDGED_CAP == 1e-5 and DV.BASE == 1e-10 and DV.FACTOR == 4.0
    per = {name: [v[name] for k, v in RECORDED.items() if k != "_provenance" and name in v] for name in DV.OUTPUTS}
    judged = {name: sum(x <= DV.JUDGED_CAP for x in xs) for name, xs in per.items()}
    total, n = sum(judged.values()), sum(len(xs) for xs in per.values())
    print({name: "%d / %d" % (judged[name], len(per[name])) for name in DV.OUTPUTS}, "all: %d / %d" % (total, n))
    assert judged["k"] == len(per["k"])
    assert total >= 0.85 * n
    assert judged["k_gamma_gamma"] >= 0.80 * len(per["k_gamma_gamma"])


@pytest.mark.parametrize("key", sorted(ENTRIES))
def test_recorded_oracle_distance_regenerates_bit_for_bit(key):
    """deriv_value_regimes.json holds exactly what the committed script measures here: the same doubles (all SEEDS seeds, one stacked
    sweep per entry)."""
    got, rec = MEASURE.measure(*ENTRIES[key]), RECORDED[key]
    assert got == rec, (key, got, rec)


# ------------------------------------------------------------------------------------------------------------------- the fake backend
# through the API on the oracle-backed backend, every row's host logic at the shapes that cost the yardstick little (fp64: the fake
# backend computes fp32 inputs in fp32 throughout, which no HIP route does)
HOST_CASES = [c for c in DV.route_cases() if c[1]["M"] * c[1]["N"] << (2 * c[1]["d"]) <= 4000 and not c[0]["knobs"] and not c[1]["f32"]]


def _id(c):
    row, sh, kind, fam, lab, st = c
    return "%s-%s-%s-%s-%s" % (row["name"].replace(" ", "_"), DV.shape_key(sh), kind, fam, lab)


@pytest.mark.parametrize("case", HOST_CASES, ids=[_id(c) for c in HOST_CASES])
def test_fake_backend_through_the_api_within_the_bounds(oracle_backend, case):
    row, sh, kind, fam, lab, st = case
    X, Y, g, X1, X2, sigma = DV.inputs(st, sh)
    got = [t.double().numpy() for t in DV.call(row, sh, kind, sigma, X, Y, g)]
    err = DV.errors(got, DV.case_want(fam, lab, kind, sh), row["outputs"])
    rec = RECORDED[DV.golden_key(fam, lab, kind, sh)]
    bad = ["%s: %.3e > %.3e" % (n, e, DV.bound(rec, n, sh["f32"])) for n, e in err.items() if not e <= DV.bound(rec, n, sh["f32"])]
    assert not bad, bad
