"""compute_kernel_and_derivatives_Gram on every route (tests/deriv_value_regimes.py: the fused solver with one band, the LDS ring and the
L2 boundary, the static-increment kernels with the wave solver, the generic route, dyadic 3, k_deriv_simple, a function-valued static
kernel, fp32 inputs) away from the unit walks: k, k_gamma and k_gamma_gamma against the LONG-DOUBLE yardstick of the same operation.
Each case runs under the launch trace and asserts that the route's kernels were launched and the other route's were not.

The bound has one rule: 1e-10 + 4 x the recorded distance of the CPU oracle from the yardstick for that (family, setting, kind, shape,
output), the maximum over eight seeds of which this test draws one (tests/golden/deriv_value_regimes.json).  It is never derived from a
GPU result.  fp32 inputs are judged on k alone, with the instance ledger's fp32 allowance on top (deriv_value_regimes.bound: two fp32
ulps, and 4 x the recorded distance of the ledger's fp32-stage restatement from the yardstick -- the unfused route hands node values and
increments on in fp32): with eps = 1e-4 an fp32 finite difference keeps 3 digits of k_gamma and none of k_gamma_gamma.

Beside the yardstick, per route: batch composition (a pair's three outputs have the same bits in the full batch, alone, and with the
rows of X permuted), workspace tiling and strided inputs, gamma = 0 (k_gamma exactly 0 as the oracle's is), gamma on one path only.

With SK_DERIV_VALUE_REGIMES_REPORT=<file> every case appends its measured errors and bounds to that file
(profiles/deriv_value_regimes.txt)."""
import json
import os

import numpy as np
import pytest
import torch

import deriv_value_regimes as DV
import instance_ledger as L
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "deriv_value_regimes.json")) as _f:
    RECORDED = json.load(_f)
CASES = DV.route_cases()


def _report(line):
    print(line)
    path = os.environ.get("SK_DERIV_VALUE_REGIMES_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _short(names):
    return sorted(n.split("_GLOBAL__N_1")[-1][:48] for n in names)


def _id(c):
    row, sh, kind, fam, lab, st = c
    return "%s-%s-%s-%s-%s" % (row["name"].replace(" ", "_"), DV.shape_key(sh), kind, fam, lab)


def _knobs(row, monkeypatch):
    import sigkernel_amd
    for knob, v in row["knobs"].items():
        monkeypatch.setattr(sigkernel_amd.routes, knob, v)


def _numpy(out3):
    return [t.detach().double().cpu().numpy() for t in out3]


def _assert_trace(row, kind, sh, names):
    missing, present = DV.check_trace(row, kind, sh, names)
    assert not missing and not present, "%s %s: claims without a launch %s, launched against the row %s (launched: %s)" % (
        row["name"], DV.shape_key(sh), missing, present, _short(names))


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_route_matches_the_long_double_yardstick(case, monkeypatch):
    row, sh, kind, fam, lab, st = case
    _knobs(row, monkeypatch)
    X, Y, g, X1, X2, sigma = DV.inputs(st, sh)
    out, names = L.traced(lambda: DV.call(row, sh, kind, sigma, X, Y, g, "cuda"))
    assert all(t.dtype == (torch.float32 if sh["f32"] else torch.float64) and t.shape == (sh["A"], sh["B"]) for t in out)
    err = DV.errors(_numpy(out), DV.case_want(fam, lab, kind, sh), row["outputs"])
    rec = RECORDED[DV.golden_key(fam, lab, kind, sh)]
    bad = []
    for name, e in err.items():
        tol = DV.bound(rec, name, sh["f32"])
        _report("%-52s %-24s %-6s %-6s %-11s %-13s %.2e  bound %.2e  ratio %.3f%s" % (
            row["name"], DV.shape_key(sh), kind, fam, lab, name, e, tol, e / tol, "" if rec[name] <= DV.JUDGED_CAP else "  (not judged)"))
        if not e <= tol:
            bad.append("%s: %.3e > %.3e" % (name, e, tol))
    _assert_trace(row, kind, sh, names)
    assert not bad, "%s %s %s %s %s: %s" % (row["name"], DV.shape_key(sh), kind, fam, lab, "; ".join(bad))


# ------------------------------------------------------------------------------------------------------------------- properties
# every row's route at its first shape, one family per static kernel
PROP_FAMILY = {"rbf": ("scale", "s=3"), "linear": ("scale", "s=3")}
PROPS = [(row, row["shapes"][0], kind) for row in DV.ROWS for kind in row["kinds"] if not row["shapes"][0]["f32"]]
PROP_IDS = ["%s-%s-%s" % (row["name"].replace(" ", "_"), DV.shape_key(sh), kind) for row, sh, kind in PROPS]
API_PROPS = [(p, i) for p, i in zip(PROPS, PROP_IDS) if p[0]["op"] != "simple"]      # (workspace_bytes is SigKernel's)

def _prop_inputs(row, sh, kind, **kw):
    fam, lab = PROP_FAMILY[kind]
    st = dict(DV.FAMILIES[fam][kind])[lab]
    X, Y, g, X1, X2, sigma = DV.inputs(st, sh, **kw)
    return (fam, lab), X, Y, g, sigma


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _same(got3, ref3, what):
    """bit equality of three outputs (the generic route's static Gram matrices are torch's batched GEMM: at these shapes it gives a pair
    the same bits in every batch; k_kgrad makes its inputs contiguous first, so a view meets the same GEMM as its copy)"""
    for name, a, b in zip(DV.OUTPUTS, got3, ref3):
        assert torch.equal(a, b), (what, name, float((a - b).abs().max()))


@pytest.mark.parametrize("prop", PROPS, ids=PROP_IDS)
def test_batch_composition(prop, monkeypatch):
    """Row a, column b of the three outputs: computed in the full batch, as X[a:a+1], Y[b:b+1], and with the rows of X permuted -- the
    persistent-wave dealing and the pair stream must not reach the arithmetic."""
    row, sh, kind = prop
    _knobs(row, monkeypatch)
    key, X, Y, g, sigma = _prop_inputs(row, sh, kind)
    Xd, Yd, gd = _dev(X, Y, g)
    full = DV.call_tensors(row, sh, kind, sigma, Xd, Yd, gd)
    a, b = sh["A"] - 1, 0
    one = DV.call_tensors(row, sh, kind, sigma, Xd[a:a + 1].contiguous(), Yd[b:b + 1].contiguous(), gd[a:a + 1].contiguous())
    _same([t[0, 0] for t in one], [t[a, b] for t in full], "alone")
    perm = torch.arange(sh["A"] - 1, -1, -1, device="cuda")
    flipped = DV.call_tensors(row, sh, kind, sigma, Xd[perm].contiguous(), Yd, gd[perm].contiguous())
    _same([t[perm] for t in flipped], list(full), "rows of X permuted")


@pytest.mark.parametrize("prop", [p for p, _ in API_PROPS], ids=[i for _, i in API_PROPS])
def test_workspace_tiling_and_strided_inputs(prop, monkeypatch):
    """workspace_bytes = 1 (one row of X per tile) gives the default's bits on the device; inputs that are strided views (transposed
    and back; a slice with a storage offset) give the bits of their contiguous copies."""
    row, sh, kind = prop
    _knobs(row, monkeypatch)
    key, X, Y, g, sigma = _prop_inputs(row, sh, kind)
    Xd, Yd, gd = _dev(X, Y, g)
    full, names = L.traced(lambda: DV.call_tensors(row, sh, kind, sigma, Xd, Yd, gd))
    tiled, names_t = L.traced(lambda: DV.call_tensors(row, sh, kind, sigma, Xd, Yd, gd, workspace_bytes=1))
    _assert_trace(row, kind, sh, names_t)
    _same(tiled, full, "workspace_bytes=1")
    Xs = Xd.transpose(1, 2).contiguous().transpose(1, 2)
    gs = torch.cat((gd[:1] * 0 + 7.0, gd))[1:]
    Ys = torch.cat((Yd[:1] * 0 - 3.0, Yd, Yd[:1]))[1:-1]
    assert not Xs.is_contiguous() and gs.storage_offset() > 0 and Ys.storage_offset() > 0
    strided = DV.call_tensors(row, sh, kind, sigma, Xs, Ys, gs)
    _same(strided, full, "strided views")


@pytest.mark.parametrize("prop", PROPS, ids=PROP_IDS)
def test_gamma_zero_and_gamma_on_one_path(prop, monkeypatch):
    """gamma = 0: k_gamma is exactly 0 -- the oracle's bits (increments(-c G) + increments(c G) cancels bitwise; the host test asserts
    the oracle's zero) --, k has the bits of the gamma != 0 call, and k_gamma_gamma, whose yardstick is 0, stays within the case's bound
    in units of the gamma != 0 case's matrix norm.  gamma nonzero on one path only: every other row's k_gamma keeps its gamma = 0 bits."""
    row, sh, kind = prop
    _knobs(row, monkeypatch)
    key, X, Y, g, sigma = _prop_inputs(row, sh, kind)
    Xd, Yd, gd = _dev(X, Y, g)
    full = DV.call_tensors(row, sh, kind, sigma, Xd, Yd, gd)
    zero = DV.call_tensors(row, sh, kind, sigma, Xd, Yd, torch.zeros_like(gd))
    assert torch.equal(zero[0], full[0])
    assert bool((zero[1] == 0).all()), float(zero[1].abs().max())
    want = DV.case_want(key[0], key[1], kind, sh)
    rec = RECORDED[DV.golden_key(key[0], key[1], kind, sh)]
    e2 = float(zero[2].abs().max()) / float(np.max(np.abs(want[2])))
    assert e2 <= DV.bound(rec, "k_gamma_gamma"), e2
    g1 = gd.clone()
    g1[1:] = 0
    one = DV.call_tensors(row, sh, kind, sigma, Xd, Yd, g1)
    assert torch.equal(one[0], full[0])
    assert torch.equal(one[1][1:], zero[1][1:])
    assert torch.equal(one[1][:1], full[1][:1]) and torch.equal(one[2][:1], full[2][:1])
