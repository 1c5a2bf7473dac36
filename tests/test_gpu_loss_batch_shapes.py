"""The loss wrappers over BATCH SHAPES, every route, against the blockwise long-double yardstick (tests/loss_batch_shapes.py): values and
the gradient of every path of X.  The one-launch loss route (csrc/sk_loss.hip, sk_solve_fwd_loss_f64, HipBackend.loss_forward,
_SigKernelLoss) is held to a reference elsewhere at 4 + 4 and 9 + 2 paths only; here

  1  small shapes, three wrappers, three routes: A + B in {3, 4, 5, 9, 17, 33, 65} is the finish kernels' chunk count (one pair per
     chunk: last_fused_ppg == 1) -- quarters shorter than the lane split, equal, ragged, empty, longer than one and two rounds of 8;
  2  HipBackend.loss_forward entry by entry: every pair of the rectangle and of the triangle, the weights it leaves for the adjoint and
     the scalar, with pair counts beyond k_loss_value's 1024 threads and beyond its batched round of 8192, on poisoned buffers;
  3  compute_Gram(X, X, sym=True) entry by entry up to 66 066 pairs: k_prep_cat's inclusive triangle, on poisoned buffers;
  4  large launches whose PLAN has the properties they run for (loss_batch_shapes.LARGE says which, and which under a knob): a
     lane-group chunk of the forward on both sides of pair A (A + B), where edge-keeping stops; pairs drawn from the work counter;
     adjoint chunks of several pairs in the uneven split, with an upstream scalar other than 1;
  5  compute_distance's merged paired batch, value and gradient.

The bound has one rule: value_regimes.BASE_TOL (1e-10 values, 1e-8 gradients) + 4 x the recorded distance of the CPU oracle from the
yardstick on that case (tests/golden/loss_batch_shapes.json: below 1e-13 everywhere).  Values per element, gradients per path.  Every
case runs under the launch trace and claims its route's kernels.

With SK_LOSS_BATCH_SHAPES_REPORT=<file> every case appends its measured errors and bounds to that file."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

import instance_ledger as L
import loss_batch_shapes as S
import value_regimes as V
from conftest import GOLDEN
from poison import poisoned

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
QUEUE = ("_lib", "_queue")
# the audited integer sites of tests/test_gpu_poison.py these calls reach: the work counter and the rescue's byte workspace
AUDITED = frozenset([QUEUE, ("_lib", "_fused_rescue_args")])
with open(os.path.join(GOLDEN, "loss_batch_shapes.json")) as _f:
    RECORDED = json.load(_f)


def _report(line):
    print(line)
    path = os.environ.get("SK_LOSS_BATCH_SHAPES_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _short(names):
    return sorted(n.split("_GLOBAL__N_1")[-1][:40] for n in names)


def _claims(names, present=(), absent=()):
    missing = [c for c in present if not any(c in n for n in names)]
    extra = [c for c in absent if any(c in n for n in names)]
    assert not missing and not extra, "not launched: %s; launched: %s (trace: %s)" % (missing, extra, _short(names))


def _check(test, c, kind, what, got, want, name, tol=None):
    """one output against the yardstick -> None or the failure's text; the figure is printed before anything is asserted"""
    err = V.grad_error(got, want) if name == "grad" else V.value_error(got, want)
    tol = S.tolerance(RECORDED, c, kind, name) if tol is None else tol
    _report("%-10s %-34s %-16s %-6s %.2e  bound %.2e" % (test, S.case_key(c, kind), what, name, err, tol))
    return None if err <= tol else "%s %s: %.3e > %.3e" % (what, name, err, tol)


def _kernel_args(kind):
    return (0, 1.0) if kind == "linear" else (1, S.SIGMA)


# ---- 1: small batch shapes, three wrappers, three routes ----------------------------------------------------------------------------------
SMALL = S.small_cases()


@pytest.mark.parametrize("case", SMALL, ids=["%s-%s" % (S.case_key(c, k), r) for c, k, r in SMALL])
def test_small_batch_shapes_on_three_routes(case, monkeypatch):
    import sigkernel_amd
    from sigkernel_amd import _lib
    c, kind, route = case
    if route != "one_launch":
        monkeypatch.setattr(sigkernel_amd.routes, route, True)
    be = _lib.get_backend()
    be.last_fused_ppg = None
    (v, g, gy), names = L.traced(lambda: S.call_wrapper(c, kind, DEV))
    value, grad, _ = S.want(c, kind)
    bad = [_check("small", c, kind, route, v, value, "value"), _check("small", c, kind, route, g, grad, "grad")]
    if route == "one_launch":
        # A + B chunks of one pair each: the multi-chunk finish kernel (k_*_adjoint_finish, not ..._finish1)
        _claims(names, ("k_prep_cat", "k_fwd_fusedI", "k_loss_value", "k_adj_fused_%sI" % kind, "k_%s_adjoint_finishE" % kind))
        assert be.last_fused_ppg == 1, be.last_fused_ppg
    else:
        _claims(names, absent=("k_loss_value",))
    assert gy is None
    assert not any(bad), "; ".join(b for b in bad if b)


# ---- 2: loss_forward per pair ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep_edges", [False, True], ids=["no_edges", "edges"])
@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("c", S.PER_PAIR, ids=["%dx%d_%s" % (c["A"], c["B"], c["wrapper"]) for c in S.PER_PAIR])
def test_loss_forward_writes_every_pair_the_weights_and_the_scalar(c, kind, keep_edges):
    from sigkernel_amd import _lib
    be = _lib.get_backend()
    A, B, with_yy = c["A"], c["B"], c["wrapper"] == "pairs_yy"
    X, Y = (torch.from_numpy(a).to(DEV) for a in S.inputs(c))
    k, param = _kernel_args(kind)
    with poisoned(0xFF, AUDITED) as p:      # an unwritten entry of `out` or `wb` stays a NaN
        res, names = L.traced(lambda: be.loss_forward(k, param, X, Y, c["d"], False, with_yy, keep_edges))
    assert res is not None and p.count >= 3, p.sites
    value, out, edges, staged, wb = res
    _claims(names, ("k_prep_cat", "k_fwd_fusedI", "k_loss_value"))
    want_value, _, pairs = S.want(c, kind)
    assert out.shape == (A * (A + B) + (B * (B - 1) // 2 if with_yy else 0),) == pairs.shape
    what = "edges" if keep_edges else "no edges"
    bad = [_check("per_pair", c, kind, what, out.cpu().numpy(), pairs, "value"),
           _check("per_pair", c, kind, what + ", scalar", value.cpu().numpy(), want_value, "value",
                  V.BASE_TOL["value"] + 4.0 * RECORDED[S.case_key(c, kind)]["loss"])]
    if keep_edges:
        assert edges is not None and wb is not None and wb.shape == (A * (A + B),)
        # d value / dK in closed form: one correctly rounded division per entry on either side -> the same doubles
        assert np.array_equal(wb.cpu().numpy(), S.wb_closed_form(A, B)), "wb is not [2 (1 - I) / (A (A - 1)) | -2 / (A B)]"
    else:
        assert edges is None and wb is None
    assert not any(bad), "; ".join(b for b in bad if b)


# ---- 3: the symmetric triangle per entry ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("c", S.SYM, ids=["A%d" % c["A"] for c in S.SYM])
def test_the_one_launch_triangle_writes_every_entry_of_a_symmetric_gram(c, kind):
    import sigkernel_amd
    X = torch.from_numpy(S.inputs(c)[0]).to(DEV)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(S.SIGMA), c["d"])
    with poisoned(0xFF, AUDITED) as p:
        K, names = L.traced(lambda: sk.compute_Gram(X, X, sym=True))
    assert p.sites.get(QUEUE, 0) == 1 and p.count >= 3, p.sites      # counter, staging + pair table, output
    # solve_fwd_fused_sym: k_prep_cat decodes the inclusive triangle (tri_n = -1), one forward launch solves it
    _claims(names, ("k_prep_cat", "k_fwd_fusedI"), absent=("k_prep_pair", "k_prep_paths"))
    assert K.shape == (c["A"], c["A"]) and torch.equal(K, K.t())
    bad = _check("sym", c, kind, "every entry", K.cpu().numpy(), S.want(c, kind)[2], "value")
    assert not bad, bad


# ---- 4: large launches, where the plan matters ---------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _knobs(knobs):
    """development knobs of the library, read from the environment by sk_reload_knobs; restored on the way out"""
    from sigkernel_amd import _lib
    was = {k: os.environ.get(k) for k in knobs}
    try:
        os.environ.update(knobs)
        _lib.load().sk_reload_knobs()
        yield
    finally:
        for k, v in was.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        _lib.load().sk_reload_knobs()


LARGE = S.large_cases()


@pytest.mark.parametrize("case", LARGE, ids=["%s%s" % (S.case_key(c, k), "-" + ",".join("%s=%s" % kv for kv in sorted(c["knobs"].items())) if c["knobs"] else "")
                                             for c, k, _ in LARGE])
def test_large_launches_straddle_the_boundary_draw_from_the_counter_and_chunk_the_adjoint(case):
    from sigkernel_amd import _lib
    c, kind, props = case
    A, B = c["A"], c["B"]
    be = _lib.get_backend()
    # the launch's plan, restated for THIS device (tests/test_loss_batch_shapes_host.py holds the table's figures for 256 CUs)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    pct = int(_lib.cost("fused_static_share_" + kind))
    geo = S.loss_geometry(kind, c["M"], c["D"], c["d"])
    wpcs = S.waves_per_cu(geo, int(c["knobs"].get("SK_FUSED_WPC", 0)))
    plans = [S.forward_plan(kind, A, B, c["M"], c["D"], c["d"], True, w, n_cu, pct) for w in wpcs]
    for p in plans:
        cut = S.straddlers(p)
        _report("%-10s %-34s plan on %d CUs at %d waves per CU: waves %d, per %d, C0 %d, n_big %d, logC %d, queue %d, q_first %d; straddling %s"
                % ("large", S.case_key(c, kind), n_cu, p["wpc"], p["waves"], p["per"], p["C0"], p["n_big"], p["logC"], p["queue"], p["q_first"], cut))
        assert cut, "no lane-group chunk holds pairs on both sides of pair %d" % p["P_rect"]
        assert bool(p["queue"]) == props["queue"], p
        if n_cu == S.N_CU:
            assert cut == [props["straddle"]], (cut, props)
    with _knobs(c["knobs"]):
        with poisoned(0xFF, AUDITED) as rec:
            (v, g, gy), names = L.traced(lambda: S.call_wrapper(c, kind, DEV))
            ppg = be.last_fused_ppg      # (poisoned() drops the back-end's last-launch records on its way in and out)
    _claims(names, ("k_prep_cat", "k_fwd_fusedI", "k_loss_value", "k_adj_fused_%sI" % kind, "k_%s_adjoint_finishE" % kind))
    assert rec.sites.get(QUEUE, 0) >= 1, rec.sites      # the launch was handed a counter (16384 pairs and more); the plan says whether it drew
    chunks = -(-(A + B) // ppg)
    _report("%-10s %-34s adjoint: last_fused_ppg %d, %d chunks of %d columns, uneven %s; upstream %g"
            % ("large", S.case_key(c, kind), ppg, chunks, A + B, (A + B) % chunks != 0, c["upstream"]))
    assert ppg > 1, ppg
    assert ((A + B) % chunks != 0) == props["uneven"], (ppg, chunks)
    value, grad, _ = S.want(c, kind)
    what = ",".join("%s=%s" % kv for kv in sorted(c["knobs"].items())) or "no knob"
    bad = [_check("large", c, kind, what, v, value, "value"), _check("large", c, kind, what, g / c["upstream"], grad, "grad")]
    assert gy is None
    assert not any(bad), "; ".join(b for b in bad if b)


# ---- 5: compute_distance -----------------------------------------------------------------------------------------------------------------
def _launches(fn):
    """fn() -> (result, {instance name: launches})"""
    from sigkernel_amd import _lib
    was = _lib.launch_trace(True)
    try:
        _lib.launch_counts(reset=True)
        out = fn()
        torch.cuda.synchronize()
        counts = _lib.launch_counts(reset=True)
    finally:
        _lib.launch_trace(was)
    return out, counts


DISTANCE = [(c, k, True) for c in S.DISTANCE for k in S.KINDS] + [(S.DISTANCE_UNMERGED, "rbf", False)]


@pytest.mark.parametrize("c, kind, merged", DISTANCE, ids=["%s-%s" % (S.case_key(c, k), "merged" if m else "no_merged_loss") for c, k, m in DISTANCE])
def test_compute_distance_value_and_gradient(c, kind, merged, monkeypatch):
    import sigkernel_amd
    if not merged:
        monkeypatch.setattr(sigkernel_amd.routes, "no_merged_loss", True)
    (v, g, gy), counts = _launches(lambda: S.call_wrapper(c, kind, DEV))
    fwd = sum(n for name, n in counts.items() if "k_fwd_fusedI" in name)
    adj = sum(n for name, n in counts.items() if "k_adj_fused_%sI" % kind in name)
    # merged: cat(X, X) against cat(X.detach(), Y) in one paired batch + k(Y, Y); else k(X, X), k(Y, Y), k(X, Y) and an adjoint for two
    assert (fwd, adj) == ((2, 1) if merged else (3, 2)), (fwd, adj, _short(counts))
    value, grad, _ = S.want(c, kind)
    what = "merged" if merged else "no_merged_loss"
    bad = [_check("distance", c, kind, what, v, value, "value"), _check("distance", c, kind, what, g, grad, "grad")]
    assert gy is None, "Y.grad must stay None"
    assert not any(bad), "; ".join(b for b in bad if b)
