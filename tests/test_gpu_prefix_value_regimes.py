"""k_fwd_prefix and everything built on it away from the unit-walk inputs (tests/prefix_value_regimes.py: the four instances at a few
lanes and at all 64, both store schemes, D = 1 / 3 / 8, 3 x 3 Gram pairs and the paired launch, fp32 stores, the streamed fallback, the
two prefix / ragged losses, the ragged exact gradients at D = 3 / 12 / 40) against the LONG-DOUBLE yardstick over every node of the
grid, under the launch trace: every case asserts that its instance of k_fwd_prefix -- or, on the streamed rows, none of them -- was
launched.  Bound: base + 4 r (tests/golden/prefix_value_regimes.json), base ALONE on offset paths for the values of the fused rows and
for LinearKernel's gradients; fp32: two ulps on top.

The slices (`nodes`) and the ragged node are compared with the grid of the same case bit for bit (one more launch each; the ragged one on
nine paths per side with every length test_gpu_ragged._lens aims at).

EXACT CLAIMS on the padding (the same true paths and lengths, the points behind every path's end (a) the repeated last point, (b) the
walk's continuation, (c) 37 randn, (d) 1e100, (e) 1e200, (f) +-1.5e308 alternating, (g) the repeated point with one NaN and one +inf
coordinate; fp32 paths: 1e18, 1e30, +-3e38): the values -- fused SK_NODES_AT and the streamed fallback -- bit-identical to (a)'s, the
ragged exact gradients (D = 3, 12, 40, Gram and paired, both static kernels, both arguments) bit-identical to (a)'s on the true points
and exactly 0.0 on every padded point.

With SK_PREFIX_VALUE_REGIMES_REPORT=<file> every case appends its measured error and bound to that file
(profiles/prefix_value_regimes.txt)."""
import os

import pytest
import torch

import prefix_value_regimes as PV
import test_prefix_value_regimes_host as H
import value_regimes as V

pytestmark = pytest.mark.gpu
DEV = "cuda"
RECORDED = H.RECORDED
STREAMED = ("k_fwd_wave", "k_fwd_simple", "k_solve", "k_static", "k_increments")      # test_gpu_ragged._traced's split


def _report(line):
    print(line)
    path = os.environ.get("SK_PREFIX_VALUE_REGIMES_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _traced(f):
    """f() under the launch trace -> (result, names of the instances launched, launches of k_fwd_prefix, launches of the streamed pieces)"""
    from sigkernel_amd import _lib
    was = _lib.launch_trace(True)
    try:
        _lib.launch_counts(reset=True)
        out = f()
        torch.cuda.synchronize()
        counts = _lib.launch_counts(reset=True)
    finally:
        _lib.launch_trace(was)
    return (out, set(k.split(".kd")[0] for k, v in counts.items() if v > 0), sum(v for k, v in counts.items() if "k_fwd_prefix" in k),
            sum(v for k, v in counts.items() if any(s in k for s in STREAMED)))


def _short(names):
    return sorted(n.split("_GLOBAL__N_1")[-1][:48] for n in names)


def test_the_restated_launch_rules_are_the_librarys():
    """prefix_value_regimes restates test_gpu_ragged's lengths and limits and the router's scope (it may not import the product)"""
    import test_gpu_ragged as R
    assert PV.LARGEST == R.LARGEST
    for seed, count, top in ((3, 9, 20), (18, 9, 17), (1, 2, 5), (0, 3, 150)):
        assert PV.ragged_lens(seed, count, top) == R._lens(seed, count, top)
    for row in PV.ROWS:
        sh = row["shape"]
        for kind in row["kinds"]:
            assert R._is_fused(kind, sh["D"], sh["M"], sh["N"], sh["d"], False, 4 if sh["f32"] else 8) == row["fused"], (row["name"], kind)


@pytest.mark.parametrize("case", PV.CASES, ids=[PV.case_id(c) for c in PV.CASES])
def test_case_matches_the_long_double_yardstick(case):
    row, kind, fam, lab, st = case
    (out, sk, Xd, Yd), names, n_prefix, n_streamed = _traced(lambda: H.run_case(case, DEV))
    want = PV.case_want(case)
    bad = []
    for name in PV.outputs_of(row):
        got = out[name].detach()
        assert got.dtype == (torch.float32 if row["shape"]["f32"] else torch.float64)
        err = PV.error(name, got.double().cpu().numpy(), want[name])
        tol = PV.tolerance(case, name, RECORDED)
        _report("%-52s %-26s %-6s %-7s %-12s %-6s %.2e  bound %.2e%s" % (row["name"], PV.geometry_key(row), kind, fam, lab, name, err, tol,
                                                                    "  invariant" if PV.invariant(case, name) else ""))
        if not err <= tol:
            bad.append("%s: %.3e > %.3e" % (name, err, tol))
    missing = [c for c in PV.claims_of(row, kind) if not any(c in n for n in names)]
    assert not missing, "%s no longer launches %s (launched: %s)" % (row["name"], missing, _short(names))
    if row["fused"]:
        # one sweep per Gram matrix, nothing streamed in the forward (the backward of a gradient row has its static stage)
        sweeps = {"grid": 1, "grid_out": 1, "mmd_prefixes": 3, "mmd_ragged": 3, "gram_ragged_grad": 1, "kernel_ragged_grad": 1, "mmd_ragged_grad": 3}
        assert n_prefix == sweeps[row["op"]], (n_prefix, _short(names))
        assert row["op"] in PV.GRAD_OPS or n_streamed == 0, _short(names)
    else:
        assert n_prefix == 0 and n_streamed >= 1, (n_prefix, n_streamed, _short(names))
    assert not bad, "%s %s %s %s: %s" % (row["name"], kind, fam, lab, "; ".join(bad))
    if row["op"] == "grid":
        _, names2, n_prefix2, n_streamed2 = _traced(lambda: H.check_slices_and_ragged(case, sk, Xd, Yd, out["value"]))
        if row["fused"]:
            assert n_prefix2 == 4 and n_streamed2 == 0 and all(PV.instance_claim(kind, row["shape"]["d"]) in n for n in names2 if "k_fwd_prefix" in n)
        else:
            assert n_prefix2 == 0 and n_streamed2 >= 4
    if row["op"] in PV.GRAD_OPS:
        lx, ly = PV.lens_of(row)
        H.assert_padding_is_zero(out["grad_x"], lx)
        H.assert_padding_is_zero(out["grad_y"], ly)


@pytest.mark.parametrize("kind, d, D, gram, f32", H.PAD_FORWARD, ids=[H.pad_id(t) for t in H.PAD_FORWARD])
def test_padding_never_reaches_a_value(kind, d, D, gram, f32):
    """a true node reads only true cells: bit-identical values under every padding, the NaN / inf one included"""
    _, names, n_prefix, n_streamed = _traced(lambda: H.padding_forward(kind, d, D, gram, f32, DEV))
    if D <= PV.MAX_FUSED_D:
        assert n_prefix == len(PV.PADDINGS) and n_streamed == 0 and any(PV.instance_claim(kind, d) in n for n in names), _short(names)
    else:
        assert n_prefix == 0 and n_streamed >= len(PV.PADDINGS)


@pytest.mark.parametrize("kind, D, gram, f32", H.PAD_GRADIENT, ids=[H.pad_id(t) for t in H.PAD_GRADIENT])
def test_padding_never_reaches_a_gradient(kind, D, gram, f32):
    _, names, _, _ = _traced(lambda: H.padding_gradient(kind, D, gram, f32, DEV))
    row = next(r for r in PV.ROWS if r["op"] == ("gram_ragged_grad" if gram else "kernel_ragged_grad") and r["shape"]["D"] == D)
    missing = [c for c in PV.claims_of(row, kind) if not any(c in n for n in names)]
    assert not missing, (missing, _short(names))
