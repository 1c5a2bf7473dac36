"""The instance ledger without a GPU: the claims of tests/instance_cases.py cover every row of the variants table (minus a short,
reasoned exemption list), name only instances the build has, every case's oracle work is under the cap, and the comparator fails
on ONE perturbed entry of every operation's output -- one pair among 9001, one small entry of a gradient row."""
import os

import numpy as np
import pytest
import torch

import instance_cases
import instance_ledger as L
from conftest import ROOT

VARIANTS_TABLE = os.path.join(ROOT, "profiles", "r06_variants.txt")
SWEEP_UNITS = ("sk_wave", "sk_static", "sk_truncated", "sk_loss")


def _table():
    rows = {}
    for ln in open(VARIANTS_TABLE):
        p = ln.rstrip("\n").split("\t")
        if len(p) >= 9 and p[0] != "unit":
            rows[p[8]] = (p[0], p[7])
    return rows


def test_claims_cover_the_variants_table():
    rows = _table()
    assert len(rows) == 540
    exempt = instance_cases.EXEMPT
    assert len(exempt) <= 5
    for m, reason in exempt.items():
        assert m in rows, m
        assert isinstance(reason, str) and len(reason) > 20 and "\n" not in reason, m
        assert not rows[m][0].startswith(SWEEP_UNITS), "a sweep or static unit's instance is exempt: %s" % rows[m][1]
    claimed = set(m for c in instance_cases.CASES for m in c["claims"])
    unknown = sorted(claimed - set(rows))
    assert not unknown, "claims of instances the build does not have: %s" % unknown
    assert not (claimed & set(exempt)), sorted(rows[m][1] for m in claimed & set(exempt))
    missing = sorted(rows[m][1] for m in set(rows) - claimed - set(exempt))
    assert not missing, "instances no case compares with the oracle: %s" % missing


RESCUE_ONLY = ("k_screen", "k_fused_rescue", "k_adj_rescue<double>", "k_adj_rescue<float>")


def test_cases_are_complete_and_under_the_cost_cap():
    labels, rows = set(), _table()
    for c in instance_cases.CASES:
        for key in ("label", "op", "kind", "param", "dtype", "dyadic", "naive", "A", "B", "M", "N", "D", "seed", "claims", "cells"):
            assert key in c, (c.get("label"), key)
        assert c["label"] not in labels, c["label"]
        labels.add(c["label"])
        assert c["claims"], c["label"]
        assert c["cells"] == int(L.cells(c)) and L.cells(c) < L.CELL_CAP, (c["label"], L.cells(c))
        if any(rows[m][1] in RESCUE_ONLY for m in c["claims"]):
            assert c.get("wild"), "the screen and the rescues are claimed by a case with one large-kernel pair: %s" % c["label"]
        if c["op"] == "kgrad" and c["dtype"] == "f32":
            assert not any(rows[m][1].startswith("k_deriv_wave") for m in c["claims"]), c["label"]
            assert set(c.get("f32_bound") or {}) <= {"k"}, "k' and k'' of fp32 paths carry no allowance: %s" % c["label"]
        if c["dtype"] == "f32" and c.get("f32_bound"):
            for b in c["f32_bound"].values():      # a measured bound: the fp32 stage's source lines, the restatement's distance, 4 x that
                assert b["source"] in L.F32_STAGE_SOURCE and b["tol"] == 4 * b["distance"], c["label"]
    ops = set((c["op"], c.get("order", 0) if c["op"].startswith("truncated") else 0) for c in instance_cases.CASES)
    assert ("truncated_golden", 1) in ops and ("truncated_golden", 2) in ops and ("truncated_golden", 4) in ops


def _spec(op, **kw):
    import reach_sweep
    s = reach_sweep._spec(op, kw.pop("kind", "rbf"), kw.pop("param", 0.9), kw.pop("dtype", "f64"), kw.pop("dyadic", 1), False,
                          kw.pop("A", 3), kw.pop("B", 4), kw.pop("M", 6), kw.pop("N", 5), kw.pop("D", 2), 5, **kw)
    if op in reach_sweep.GRAD_OPS:
        s["w"] = "randn"
    return s


SHAPES = [_spec(op) for op in ("gram", "gram_sym", "kernel", "gram_grad", "gram_sym_grad", "kernel_grad", "mmd", "scoring_rule", "distance", "kgrad")]
SHAPES += [_spec("mmd_grad", N=6), _spec("esr_grad", N=6), _spec("gram_grad", dtype="f32"), _spec("kernel_grad", kind="linear", param=None, A=9001, B=9001, M=3, N=3),
           _spec("gram_grad", A=40, B=3), _spec("gram_grad", kind="poly", param=None),
           _spec("adj_wild", kind="none", param=None, A=6, B=1, M=9, N=11, D=0, wild=[2]), _spec("deriv", kind="none", param=None, A=5, B=1, M=9, N=11, D=0),
           _spec("truncated_golden", kind="none", param=None, A=3, B=2, M=9, N=6, D=3, L=4, order=1, fixture=6),
           _spec("kernel_fn", kind="rbf_id", param=2.0, A=3, B=3, D=6, F=3), _spec("truncated", kind="none", param=None, L=3, order=-1),
           _spec("exact_fwd", kind="none", param=None, A=6, B=1, M=9, N=11, D=0), _spec("exact_adj", kind="none", param=None, A=6, B=1, M=9, N=11, D=0),
           _spec("exact_deriv", kind="none", param=None, A=6, B=1, M=9, N=11, D=0), _spec("loss_weights", kind="none", param=None, A=5, B=7, M=0, N=0, D=0)]
SHAPES += [_spec(op, nodes=nodes) for op in ("prefix_gram", "prefix_kernel") for nodes in ("all", "diagonal", "last_row", "last_col")]


@pytest.mark.parametrize("spec", SHAPES, ids=["%s_%s_%s_%d%s" % (s["op"], s["kind"], s["dtype"], s["A"], s.get("nodes", "")) for s in SHAPES])
def test_one_perturbed_entry_fails_the_comparator(spec):
    """The oracle's own output passes; with ONE entry off by 10 x the tolerance (of that element's scale / that path's max-norm; one ulp
    where the bound is bit equality) it fails, at that entry -- the smallest entry of the array, of the smallest row of a gradient."""
    import reach_sweep
    t = reach_sweep.inputs(spec)
    want = L.expected(spec, t)
    rows = list(range(spec["A"]))

    def returned(n, v):      # (the call returns every row of a gradient; the sample is compared)
        v = torch.from_numpy(np.array(v[0] if isinstance(v, tuple) else v, dtype=np.float64))
        if n != "grad":
            return v
        full = torch.zeros((spec["A"],) + tuple(v.shape[1:]), dtype=torch.float64)
        full[rows] = v
        return full
    for name, w in want.items():
        w = w[0] if isinstance(w, tuple) else w
        tol = L.tolerance(spec, name)
        got = returned(name, w)
        assert L.check_case(spec, {n: returned(n, v) for n, v in want.items()}, want) == []
        w = np.asarray(w)
        if name == "grad" or (name == "W" and tol > 0):      # compared per path / per pair
            norms = np.abs(w).reshape(w.shape[0], -1).max(1)
            r = int(np.argmin(norms))
            i = (r,) + np.unravel_index(int(np.argmin(np.abs(w[r]))), w[r].shape)
            step, at = 10 * tol * norms[r], (rows[r],) + tuple(int(j) for j in i[1:])
            assert norms[r] <= np.abs(w).max()
        else:
            i = np.unravel_index(int(np.argmin(np.abs(w))), w.shape) if w.ndim else ()
            step, at = 10 * tol * max(abs(float(w[i])), 1.0), tuple(int(j) for j in i)
        off = got.clone()
        if tol == 0.0:
            off[at] = float(np.nextafter(float(w[i]), np.inf))
        else:
            off[at] += step
        bad = L.check_case(spec, {n: (off if n == name else returned(n, v)) for n, v in want.items()}, want)
        assert len(bad) == 1 and bad[0][0] == name and bad[0][1] == at, (name, at, bad)


def test_non_finite_entries_must_match_exactly():
    w = np.array([1.0, np.inf, np.nan, 2.0])
    assert L.compare_values(w.copy(), w, 1e-10)[0]
    for i, v in ((0, np.nan), (1, 1e300), (2, 0.0), (1, -np.inf)):
        g = w.copy()
        g[i] = v
        ok, at, _ = L.compare_values(g, w, 1e-10)
        assert not ok and at == (i,)
    gw = np.ones((3, 2, 2))
    g = gw.copy()
    g[1, 0, 1] = np.nan
    assert L.compare_grads(gw, gw, 1e-8)[0] and L.compare_grads(g, gw, 1e-8)[:2] == (False, (1, 0, 1))
