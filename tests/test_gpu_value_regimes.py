"""Every route family away from the unit-walk inputs (tests/value_regimes.py: drifting, rescaled and offset paths, sigma over 14
decades), values and gradients against the LONG-DOUBLE yardstick -- not the oracle: the kernels that form everything from coordinate
differences are more accurate than the reference's |x|^2 + |y|^2 - 2 <x, y> on offset paths.  Each case runs under the launch trace
and asserts that an instance of the route's kernel family was launched.

The bound has one rule: base + 4 x the recorded distance of the oracle from the yardstick on that case
(tests/golden/value_regimes.json; base = the ledger's 1e-10 values / 1e-8 gradients, 4 = the ledger's factor for a differing
summation order).  Outside `offset` the second term is below 1e-11.  Rows marked invariant for a static kernel
(value_regimes.ROUTES, with the source that says so) get NO allowance on offset paths: a common shift must not cost them a digit.
fp32 inputs: two fp32 ulps on top.  LinearKernel at s = 10 (|K| up to 1e18) is held to the ledger's RESCUE_GRAD_TOL and must show the
rescue kernels on its trace.

Beside the routes of value_regimes.ROUTES the table holds the rows above 32 dims (WIDE_ROUTES: k_static_wide_mfma through the API, D = 33
beside D = 32) and two operations on three shapes each (OPERATION_ROUTES): `paired_grad`, compute_kernel weighted by a random vector, and
`gram_grad_y`, the gradient with respect to the second argument of compute_Gram (exact_gradient=True, the mode that returns one).

test_gpu_exp_probe measures the hand-written exponential itself (csrc/sk_internal.h: exp_nonpos) through single isolated nodes.

With SK_VALUE_REGIMES_REPORT=<file> every case appends its measured error and bound to that file (profiles/value_regimes.txt)."""
import json
import os

import numpy as np
import pytest
import torch

import instance_ledger as L
import value_regimes as V
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "value_regimes.json")) as _f:
    RECORDED = json.load(_f)
CASES = V.route_cases()
WANT = {"gram_grad": "gram", "exact_grad": "exact", "sym": "sym", "sym_grad": "sym", "prefix": "prefix", "mmd_grad": "mmd", "kgrad": "gram",
        "paired_grad": "paired", "gram_grad_y": "gram_y"}


def _report(line):
    print(line)
    path = os.environ.get("SK_VALUE_REGIMES_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _short(names):
    return sorted(n.split("_GLOBAL__N_1")[-1][:48] for n in names)


def _id(c):
    row, sh, kind, fam, lab, st = c
    return "%s-%s-%s-%s-%s" % (row["name"].replace(" ", "_"), V.shape_key(sh), kind, fam, lab)


def _call(row, sh, kind, X, Y, w, sigma):
    """the route's call on the GPU -> {output: tensor}"""
    import sigkernel_amd
    dt = torch.float32 if sh["f32"] else torch.float64
    Xd, Yd, wd = (torch.from_numpy(a).to(dt).cuda() for a in (X, Y, w))
    kern = sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(sigma)
    op = row["op"]
    sk = sigkernel_amd.SigKernel(kern, sh["d"], exact_gradient=op in ("exact_grad", "gram_grad_y"))
    if op == "sym":
        return {"value": sk.compute_Gram(Xd, Xd, sym=True)}
    if op == "prefix":
        return {"value": sk.compute_Gram_prefixes(Xd, Yd)}
    if op == "kgrad":
        gamma = torch.randn(X.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(dt).cuda()
        return {"k": sk.compute_kernel_and_derivatives_Gram(Xd, Yd, gamma)[0]}
    if op == "gram_grad_y":
        Yg = Yd.clone().requires_grad_(True)
        v = sk.compute_Gram(Xd, Yg)
        (v * wd).sum().backward()
        return {"value": v.detach(), "grad": Yg.grad}
    Xg = Xd.clone().requires_grad_(True)
    if op == "paired_grad":
        v = sk.compute_kernel(Xg, Yd)
        (v * wd.diagonal()).sum().backward()
        return {"value": v.detach(), "grad": Xg.grad}
    if op == "mmd_grad":
        v = sk.compute_mmd(Xg, Yd)
        v.backward()
    else:
        v = sk.compute_Gram(Xg, Xg, sym=True) if op == "sym_grad" else sk.compute_Gram(Xg, Yd)
        (v * wd).sum().backward()
    return {"value": v.detach(), "grad": Xg.grad}


def _tolerance(row, sh, kind, fam, lab, st, name):
    base = (L.RESCUE_GRAD_TOL if st.get("wild") and name == "grad" else V.BASE_TOL[name]) + (L.F32_ULPS2 if sh["f32"] else 0.0)
    if kind in row["invariant"] and fam == "offset":
        return base
    return base + 4.0 * RECORDED[V.golden_key(fam, lab, kind, sh)]["value" if name == "k" else name]


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_route_matches_the_long_double_yardstick(case, monkeypatch):
    import sigkernel_amd
    row, sh, kind, fam, lab, st = case
    for knob, v in row["knobs"].items():
        monkeypatch.setattr(sigkernel_amd.routes, knob, v)
    X, Y, w, sigma = V.case_inputs(fam, lab, kind, sh)
    out, names = L.traced(lambda: _call(row, sh, kind, X, Y, w, sigma))
    missing = [c for c in V.claims_of(row, kind, st) if not any(c in n for n in names)]
    want_value, want_grad = V.case_want(fam, lab, kind, sh, WANT[row["op"]])
    bad = []
    for name in row["outputs"]:
        got = out[name].detach().double().cpu().numpy()
        if name == "grad":
            err = min(V.grad_error(got, g) for g in (want_grad if isinstance(want_grad, tuple) else (want_grad,)))
        else:
            err = V.value_error(got, want_value)
        tol = _tolerance(row, sh, kind, fam, lab, st, name)
        _report("%-52s %-22s %-6s %-7s %-12s %-5s %.2e  bound %.2e%s" % (row["name"], V.shape_key(sh), kind, fam, lab, name, err, tol,
                                                                    "  invariant" if kind in row["invariant"] and fam == "offset" else ""))
        if not err <= tol:
            bad.append("%s: %.3e > %.3e" % (name, err, tol))
    assert not missing, "%s no longer launches %s (launched: %s)" % (row["name"], missing, _short(names))
    assert not bad, "%s %s %s %s: %s" % (row["name"], kind, fam, lab, "; ".join(bad))


# ------------------------------------------------------------------------------------------------------------------- the exponential
def _probe_k(scale):
    """4096 integers k spread over [0, 29 scale]: t = k / scale has t^2 exact in double and -t^2 down to -841"""
    return np.unique(np.round(np.linspace(0.0, 29.0, 4096) * scale)).astype(np.int64)


PROBES = [(D, 1.0, 12) for D in (1, 8, 12, 20, 32, 40)] + [(8, 0.5, 13)]


@pytest.mark.parametrize("D, sigma, shift", PROBES, ids=["D%d-sigma%g" % (D, s) for D, s, _ in PROBES])
def test_gpu_exp_probe(D, sigma, shift):
    """exp_nonpos as the static-increment kernels evaluate it, one node at a time: pairs of 2-point paths x = (1e5, t), y = (-1e5, 0)
    in coordinate 0.  Three of the four nodes underflow to exactly 0, so the increment IS exp(-t^2 / sigma) as the kernel computed
    it; with t = k 2^-shift the squares and the exponent are exact in double (|x|^2 + |y|^2 - 2 <x, y> = t^2 + 0 - 0), so the only
    error is the function's own, and the yardstick is expl of that exact exponent.  On these inputs the CPU libm is at 0.67 ulp
    (normal results) and 0.50 units of 2^-1074 (subnormal ones).

    Bounds: normal results 2 ulp (the header's budget is about 1: 0.5 from the last FMA, 0.3 from the Horner steps below it, 0.2 from
    the polynomial); exponents below -745.2 exactly 0; subnormal results finite, non-negative, within 2^-1022 (a flush to zero passes,
    garbage does not)."""
    from sigkernel_amd import _lib
    k = _probe_k(np.sqrt(sigma) * 2.0 ** shift) if sigma != 1.0 else _probe_k(2.0 ** shift)
    t = k / 2.0 ** shift
    e = -(t * t) / sigma
    assert np.all((k.astype(object) ** 2) * int(round(1 / sigma)) == [int(v) for v in -e * 4.0 ** shift]), "the exponents are not exact"
    n = len(t)
    X, Y = np.zeros((n, 2, D)), np.zeros((n, 2, D))
    X[:, 0, 0], X[:, 1, 0], Y[:, 0, 0] = 1e5, t, -1e5
    be = _lib.get_backend()
    inc, names = L.traced(lambda: be.static_increments(1, sigma, torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), False))
    got = inc[:, 0, 0].cpu().numpy()
    dmax = next(m for m in (4, 8, 16, 24, 32, 0) if D <= m or m == 0)
    claim = "k_static_nodesIdLi%dELi1ELi1E" % dmax if dmax else "k_static_wide_mfma"
    assert any(claim in nm for nm in names), (claim, _short(names))
    want = np.exp(e.astype(V.LD))
    tiny = 2.0 ** -1022
    normal, zero = want >= tiny, e < -745.2
    sub = ~normal & ~zero
    err = np.abs(got.astype(V.LD) - want)
    ulps = float(np.max(err[normal] / np.spacing(want[normal].astype(np.float64))))
    sub_err = float(np.max(err[sub] / V.LD(2.0 ** -1074)))
    gradual = bool(np.any(got[sub] > 0))
    _report("exp probe %-28s sigma %-4g %4d normal results: worst %.3f ulp (bound 2); %3d subnormal: worst %.2f x 2^-1074, gradual underflow %s; "
            "%3d below -745.2: %s; %d clamped" % (claim, sigma, int(normal.sum()), ulps, int(sub.sum()), sub_err, "holds" if gradual else "FLUSHED",
                                                   int(zero.sum()), "all 0" if np.all(got[zero] == 0) else "NOT all 0", int((e < -800).sum())))
    assert normal.sum() > 3000 and sub.sum() >= 50 and (e < -800).sum() >= 50
    assert np.all(np.isfinite(got)) and np.all(got >= 0)
    assert np.all(got[zero] == 0)
    assert np.all(err[sub] <= tiny)
    assert ulps <= 2.0, "exp_nonpos is %.3f ulp off on a normal result (instance %s)" % (ulps, claim)
