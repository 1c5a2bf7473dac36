"""The launches behind the shared host arithmetic of the fused adjoints and the one-draw kernels (csrc/sk_wave_common.h:
plan_adjoint_chunks, sweep_gram_rows; csrc/sk_adj_fused_rescue.hip: arm_fused_rescue; csrc/sk_pair_stream.h: plan_one_draw).

The arithmetic was one copy per launcher; it is shared now, and nothing a launch computes may have moved.  Every shape is chosen with
the exported plan, asked with the device's CU count, and the test asserts what the plan says -- a shape that stops reaching its branch
fails.  Every call runs on workspaces and outputs of 0xFF bytes (tests/poison.py): a slot no launch wrote is a NaN.  Sampled rows and
pairs -- the first and last row of every launch, the first and last pair of the stream -- are held against the CPU oracle and, bit for
bit, against tests/golden/adjoint_launches_parent.npz: the PARENT commit's values, recorded once on an MI355X by record_golden() (run
with the parent's package first on sys.path).

  one-band adjoints (linear and RBF, fp64, dyadic 1, dim 3, 40 points, 64 second paths)
    several    the smallest Gram the plan sweeps in three launches or more: plain, second-argument sums (the ypart stride), and with
               forward values and one exploding pair in the LAST launch (scale, residual and rescue offsets at a0 > 0)
    one        the same three calls on a Gram that fills the chip exactly in one launch
    paired     a paired batch of several pairs per lane group
  one-draw kernels (paired batches, dim 9, 8 points; the derivative solver: dim 8, 8 x 113 points)
    counter    8 x 8 x CUs pairs: at most 8 waves per CU are resident whatever a variant's registers, so the equal share is 8 pairs or
               more and the counter is used; the last 16 pairs of the stream are among the sampled ones
    below      one pair fewer.  (At 8 waves per CU the equal share is still 8 and the counter still used: the plan says so.)
    static     7 x CUs pairs: an equal share below 8 whatever the waves per CU -- no counter"""
import functools
import os

import numpy as np
import pytest
import torch

import launch_plans as LP
import sigkernel_amd
from conftest import rel_err, walk
from oracle import oracle as O
from poison import poisoned
from sigkernel_amd import _lib

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adjoint_launches_parent.npz")
GRAD_TOL = 1e-9            # gradients against the oracle (tests/test_configs.py)
RESCUE_GRAD_TOL = 2e-8     # rows with a rescued pair (tests/instance_ledger.py: 2 x ADJ_RESIDUAL_TOL)
TOL_K, TOL_KD, TOL_KDD = 1e-12, {"linear": 1e-9, "rbf": 1e-8}, 1e-5      # the fused derivative solver against the oracle (tests/test_derivatives.py)
AUDITED = frozenset(("_lib", f) for f in ("_queue", "solve_fwd_fused_static", "linear_adjoint_fused_mb", "rbf_adjoint_fused_mb", "solve_deriv_fused",
                                          "_fused_rescue_args", "solve_adj", "_grid_scratch"))      # tests/test_gpu_poison.py
M1, D1, B1, DY1 = 40, 3, 64, 1
SIGMA = 0.75
NT = min(16, O.max_threads())


def _kernel(kind):
    return sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(SIGMA)


def _n_cu():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


# ---- the plans --------------------------------------------------------------------------------------------------------------------------
# How the one-band adjoints lay 40 points at dyadic 1 on a wave (launch_adj_fused_{linear,rbf}_rows): two coarse rows per lane, 39 rows
# -> 32 lanes per pair, two lane groups per wave; 20 units per row -> NUp = 24.  The RBF sweep that forms BOTH sets of sums takes one
# row per lane: 64 lanes, one lane group.  LDS bytes of a wave from the same functions (four waves per workgroup fit in each case).
GEOM = {("linear", False): (2, 24, 21568), ("linear", True): (2, 24, 21568), ("rbf", False): (2, 24, 24640), ("rbf", True): (1, 24, 15392)}


RESTATED_PLANS = False      # record_golden(): the parent's library has no plan exports; tests/launch_plans.py restates them


@functools.lru_cache(maxsize=None)
def _plan_fields(G, NUp, lds, A, B, n_cu, restated):
    if restated:
        r = LP.adjoint_chunks(A, B, G, NUp, n_cu, 8, 0, lds, True)
        return (r["PPG"], r["ppp"], r["rows_per_launch"], r["groups"], LP.chunks_of(B, r["PPG"]))
    out = np.full(5, -1, np.int64)
    rc = _lib.load().sk_plan_adjoint_chunks(A, B, G, NUp, n_cu, 8, 0, lds, 1, 0, out.ctypes.data)
    assert rc == 0, rc
    return tuple(int(v) for v in out)


def _plan(kind, yside, A, B):
    return dict(zip(("PPG", "ppp", "rows_per_launch", "groups", "nch"), _plan_fields(*GEOM[(kind, yside)], A, B, _n_cu(), RESTATED_PLANS)))


def _several(kind, yside):
    """the smallest A for which A x 64 is swept in three launches or more"""
    for A in range(1, 1 << 14):
        p = _plan(kind, yside, A, B1)
        if p["rows_per_launch"] > 0 and -(-A // p["rows_per_launch"]) >= 3:
            return A, p
    raise AssertionError("no Gram of %d columns is swept in three launches" % B1)


def _one(kind, yside):
    """the smallest A for which A x 64 fills the chip exactly in one launch, with chunks of eight pairs or more (shares by rank)"""
    G = GEOM[(kind, yside)][0]
    for A in range(1, 1 << 14):
        p = _plan(kind, yside, A, B1)
        if p["rows_per_launch"] == 0 and A * p["nch"] == _n_cu() * 8 * G and p["PPG"] >= 8:
            return A, p
    raise AssertionError("no Gram of %d columns fills the chip in one launch" % B1)


def _launch_rows(A, p):
    """first and last row of every launch"""
    rpl = p["rows_per_launch"] or A
    return sorted({a for a0 in range(0, A, rpl) for a in (a0, min(a0 + rpl, A) - 1)})


# ---- the one-band adjoints --------------------------------------------------------------------------------------------------------------
def _one_band_inputs(kind, A, seed, wild_row=None):
    gen = torch.Generator().manual_seed(seed)
    X, Y = walk(gen, A, M1, D1), walk(gen, B1, M1, D1)
    if wild_row is not None:      # x_a and y_5 the same straight line: k(x_a, y_5) explodes, the rest is tame (test_configs._one_wild_pair)
        # (the same extent as there: 31 steps of 0.6)
        line = torch.arange(M1, dtype=torch.float64)[:, None] * (0.6 * 31 / (M1 - 1)) * torch.ones(1, D1, dtype=torch.float64) / np.sqrt(D1)
        X[wild_row], Y[5] = line, line.clone()
    w = torch.randn(A, B1, generator=gen, dtype=torch.float64)
    return X, Y, w


def _one_band(kind, mode, A, p, rows, seed):
    """One call of be.{linear,rbf}_adjoint_fused on an A x 64 Gram, poisoned.  mode: plain | yside | rescue.
    -> {name: sampled array}, (max error, bound) per sampled row against the oracle"""
    be = _lib.get_backend()
    k = _kernel(kind)
    rpl = p["rows_per_launch"] or A
    wild = None
    if mode == "rescue":      # the first row of the last launch (one launch: a row in the middle); it is among the sampled rows
        wild = (A - 1) // rpl * rpl if p["rows_per_launch"] else A // 2
        assert wild in rows and (wild > 0 or not p["rows_per_launch"])
    X, Y, w = _one_band_inputs(kind, A, seed, wild)
    if mode == "yside":      # the upstream gradient is folded in afterwards: nonzero on the sampled rows only, so that the oracle is cheap
        keep = torch.zeros(A, 1, dtype=torch.float64)
        keep[rows] = 1.0
        w = w * keep
    Xd, Yd = X.to(DEV), Y.to(DEV)
    fwd = be.solve_fwd_fused_linear if kind == "linear" else be.solve_fwd_fused_rbf
    adj = be.linear_adjoint_fused if kind == "linear" else be.rbf_adjoint_fused
    param = 1.0 if kind == "linear" else SIGMA
    with poisoned(0xFF, AUDITED):
        K, edges = fwd(Xd, Yd, param, DY1, False, True, keep_edges=True)
        assert edges is not None
        res = adj(Xd, Yd, param, DY1, edges, w.reshape(-1).to(DEV), gram=True, yside=(mode == "yside"),
                  kfinal=K.reshape(-1) if mode == "rescue" else None)
        assert res is not None, "the fused adjoint declined the case"
        ppg, err = be.last_fused_ppg, be.last_fused_err.cpu().numpy().reshape(A, B1)
    torch.cuda.synchronize()
    assert ppg == p["PPG"], "the launcher planned chunks of %d pairs, the export %d" % (ppg, p["PPG"])
    out, checks = {}, []
    if mode == "yside":
        sums = res[2]
        used = sums if kind == "linear" else torch.cat([sums[..., :1], sums[..., 2:]], -1)      # (RBF: [S0, unused, S1])
        assert bool(torch.isfinite(used).all()), "second-argument sums left unwritten"
        out["ysums"] = sums[rows][:, [0, B1 - 1]].cpu().numpy().copy()
        got = be.second_argument_gradient(sums, Yd, None if kind == "linear" else SIGMA, w.to(DEV)).cpu().numpy()
        want = O.gram_grad_weighted(Y, X[rows], w[rows].t().contiguous().numpy(), k, DY1, nthreads=NT)
        checks.append(("dY", rel_err(got, want), GRAD_TOL))
        if res[0] is not None:      # (RBF, dims <= 4: the first-argument gradient of the same sweep)
            out["dX"] = res[0][rows].cpu().numpy().copy()
    else:
        g = res[0]
        assert bool(torch.isfinite(g).all()), "rows of the gradient left unwritten"
        out["dX"] = g[rows].cpu().numpy().copy()
        want = O.gram_grad_weighted(X[rows], Y, w[rows].numpy(), k, DY1, nthreads=NT)
        for i, a in enumerate(rows):
            rescued = bool((err[a] < 0).any())
            # (a sweep armed with forward values keeps pairs up to the screen, whose backward recompute of K loses ~1e-16 K^2: every
            # row of such a call is held to twice the self-check bound, as in tests/test_configs.py)
            checks.append(("dX[%d]%s" % (a, " rescued" if rescued else ""), rel_err(out["dX"][i], want[i]), RESCUE_GRAD_TOL if mode == "rescue" else GRAD_TOL))
        if mode == "rescue":
            assert err[wild, 5] == -1.0, "the exploding pair was not taken out of the sweep"
            assert wild // rpl == (A - 1) // rpl, "the exploding pair is not in the last launch"
            out["err"] = err[rows][:, [0, 5, B1 - 1]].copy()
        else:
            assert float(err.max()) <= be.ADJ_RESIDUAL_TOL
    out["in"] = np.array([float(X.sum()), float(Y.sum()), float(w.sum())])
    return out, checks


ONE_BAND = [(kind, shape, mode) for kind in ("linear", "rbf") for shape in ("several", "one") for mode in ("plain", "yside", "rescue")]


def _one_band_case(kind, shape, mode):
    yside = mode == "yside"
    A, p = (_several if shape == "several" else _one)(kind, yside)
    rows = _launch_rows(A, p)
    if shape == "one":
        rows = sorted(set(rows + [A // 2]))
    seed = 7000 + 13 * ONE_BAND.index((kind, shape, mode))
    out, checks = _one_band(kind, mode, A, p, rows, seed)
    name = "%s_%s_%s" % (kind, shape, mode)
    out["rows"] = np.array(rows)
    return A, p, {"%s_%s" % (name, k): v for k, v in out.items()}, checks


def _paired_case(kind):
    """a paired batch of several pairs per lane group (the PAIRED form), one pair past a whole number of them"""
    be = _lib.get_backend()
    G = GEOM[(kind, False)][0]
    P = 2 * _n_cu() * 8 * G + 1
    p = _plan(kind, False, P, 0)
    gen = torch.Generator().manual_seed(7100 + (kind == "rbf"))
    X, Y = walk(gen, P, M1, D1), walk(gen, P, M1, D1)
    w = torch.randn(P, generator=gen, dtype=torch.float64)
    pairs = sorted(set([0, 1, 2, 3, P // 2, P - 3, P - 2, P - 1] + torch.randperm(P, generator=gen)[:8].tolist()))
    fwd = be.solve_fwd_fused_linear if kind == "linear" else be.solve_fwd_fused_rbf
    adj = be.linear_adjoint_fused if kind == "linear" else be.rbf_adjoint_fused
    param = 1.0 if kind == "linear" else SIGMA
    with poisoned(0xFF, AUDITED):
        K, edges = fwd(X.to(DEV), Y.to(DEV), param, DY1, False, False, keep_edges=True)
        res = adj(X.to(DEV), Y.to(DEV), param, DY1, edges, w.to(DEV), gram=False)
        assert res is not None
        ppg = be.last_fused_ppg
    torch.cuda.synchronize()
    assert ppg == p["PPG"] == p["ppp"]
    g = res[0]
    assert bool(torch.isfinite(g).all()), "rows of the gradient left unwritten"
    got = g[pairs].cpu().numpy().copy()
    checks = []
    for i, q in enumerate(pairs):
        want = O.gram_grad_weighted(X[q:q + 1], Y[q:q + 1], w[q:q + 1, None].numpy(), _kernel(kind), DY1)[0]
        checks.append(("dX[%d]" % q, rel_err(got[i], want), GRAD_TOL))
    name = "%s_paired" % kind
    return P, p, {name + "_dX": got, name + "_pairs": np.array(pairs), name + "_in": np.array([float(X.sum()), float(Y.sum()), float(w.sum())])}, checks


# ---- the one-draw kernels ---------------------------------------------------------------------------------------------------------------
ONE_DRAW = ["counter", "below", "static"]


def _one_draw_pairs(which):
    n = _n_cu()
    return {"counter": 64 * n, "below": 64 * n - 1, "static": 7 * n}[which]


def _one_draw_plan(P, wpc_knob):
    """sk_plan_one_draw for a variant that LDS and registers allow 8 waves per CU, capped by the knob"""
    out = np.full(7, -1, np.int64)
    rc = _lib.load().sk_plan_one_draw(P, 9000, 4, 256, wpc_knob, _n_cu(), 80, 50, 0, out.ctypes.data)
    assert rc == 0, rc
    return dict(zip(("wpc", "waves", "per", "C0", "q_first", "queue", "ws_doubles"), (int(v) for v in out)))


def _assert_one_draw_plan(which, P):
    if RESTATED_PLANS:
        return
    by_wpc = {k: _one_draw_plan(P, k) for k in (8, 4, 2, 1)}      # whatever the variant's registers and LDS leave resident
    used = {k: v["queue"] for k, v in by_wpc.items()}
    if which == "static":
        assert not any(used.values()), used
    else:
        assert all(used.values()), used      # (below: one pair fewer still makes an equal share of 8 at 8 waves per CU)
        assert by_wpc[8]["per"] == 8 and by_wpc[8]["C0"] == 4 and by_wpc[8]["q_first"] == 4 * 8 * _n_cu()


def _sampled(P, gen):
    """64 pairs: the first four, the last 16 of the stream (drawn from the counter where it is used), the rest seeded"""
    fixed = [0, 1, 2, 3] + list(range(P - 16, P))
    rest = [q for q in torch.randperm(P - 20, generator=gen).add(4).tolist()][:44]
    return sorted(fixed + rest)


def _multiband_case(which, kind):
    """paired batch, dim 9, 8 points: the multi-band forward that keeps edges, then the multi-band adjoint"""
    be = _lib.get_backend()
    P = _one_draw_pairs(which)
    _assert_one_draw_plan(which, P)
    gen = torch.Generator().manual_seed(7200 + 7 * ONE_DRAW.index(which) + (kind == "rbf"))
    X, Y = walk(gen, P, 8, 9), walk(gen, P, 8, 9)
    w = torch.randn(P, generator=gen, dtype=torch.float64)
    pairs = _sampled(P, gen)
    k = sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(0.7)
    kd, param = (0, 1.0) if kind == "linear" else (1, 0.7)
    with poisoned(0xFF, AUDITED):
        res = be.solve_fwd_fused_static(kd, param, X.to(DEV), Y.to(DEV), DY1, False, False, keep_edges=True)
        assert res is not None and res[1] is not None, "the multi-band forward declined the case"
        K, edges = res
        adj = be.linear_adjoint_fused_mb if kind == "linear" else be.rbf_adjoint_fused_mb
        out = adj(X.to(DEV), Y.to(DEV), param, DY1, edges, w.to(DEV), gram=False)
        assert out is not None, "the multi-band adjoint declined the case"
    torch.cuda.synchronize()
    assert bool(torch.isfinite(K).all()) and bool(torch.isfinite(out[0]).all()), "pairs left unwritten"
    assert float(out[1]) <= be.ADJ_RESIDUAL_TOL
    gotK, gotG = K[pairs].cpu().numpy().copy(), out[0][pairs].cpu().numpy().copy()
    checks = []
    for i, q in enumerate(pairs):
        wantK = O.gram_forward(X[q:q + 1], Y[q:q + 1], k, DY1)[0, 0]
        wantG = O.gram_grad_weighted(X[q:q + 1], Y[q:q + 1], w[q:q + 1, None].numpy(), k, DY1)[0]
        checks.append(("K[%d]" % q, abs(gotK[i] - wantK) / abs(wantK), 1e-11))
        checks.append(("dX[%d]" % q, float(np.abs(gotG[i] - wantG).max() / max(np.abs(wantG).max(), 1e-300)), 1e-10))
    name = "mb_%s_%s" % (which, kind)
    ends = [i for i, q in enumerate(pairs) if q < 4 or q >= P - 16]      # (the golden file keeps the gradients of the stream's two ends)
    return {name + "_K": gotK, name + "_dX": gotG[ends], name + "_pairs": np.array(pairs), name + "_in": np.array([float(X.sum()), float(Y.sum())])}, checks


def _deriv_case(which, kind):
    """the fused derivative solver on an A x B Gram of the same number of pairs: dim 8, 8 points against 113 (rows of 64 units)"""
    be = _lib.get_backend()
    P = _one_draw_pairs(which)
    _assert_one_draw_plan(which, P)
    A = max(a for a in range(1, 129) if P % a == 0)      # (16384 = 128 x 128, 16383 = 127 x 129, 1792 = 128 x 14 on MI355X)
    B = P // A
    gen = torch.Generator().manual_seed(7300 + 7 * ONE_DRAW.index(which) + (kind == "rbf"))
    X, Y = walk(gen, A, 8, 8), walk(gen, B, 113, 8)
    gam = torch.randn(A, 8, 8, generator=gen, dtype=torch.float64) / 8
    eps = 1e-4
    k = sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(0.9)
    kd, param = (0, 1.0) if kind == "linear" else (1, 0.9)
    pairs = _sampled(P, gen)
    with poisoned(0xFF, AUDITED):
        res = be.solve_deriv_fused(kd, param, X.to(DEV), (X + eps * gam).to(DEV), (X + 2 * eps * gam).to(DEV), Y.to(DEV), 0, eps)
        assert res is not None, "the fused derivative solver declined the case"
    torch.cuda.synchronize()
    got = torch.stack(res).reshape(3, P)
    assert bool(torch.isfinite(got).all()), "pairs left unwritten"
    got = got[:, pairs].cpu().numpy().copy()
    rows_a = sorted({q // B for q in pairs})
    want = np.stack(O.kgrad(X[rows_a], Y, gam[rows_a], k, 0, eps=eps, nthreads=NT))      # (3, rows, B)
    want = np.stack([want[:, rows_a.index(q // B), q % B] for q in pairs], 1)
    checks = [(n, rel_err(got[i], want[i]), t) for i, (n, t) in enumerate((("k", TOL_K), ("k_gamma", TOL_KD[kind]), ("k_gamma_gamma", TOL_KDD)))]
    name = "deriv_%s_%s" % (which, kind)
    return {name + "_out": got, name + "_pairs": np.array(pairs), name + "_in": np.array([float(X.sum()), float(Y.sum()), float(gam.sum())])}, checks


# ---- golden -----------------------------------------------------------------------------------------------------------------------------
def record_golden(path=GOLDEN):
    """Write the golden file from whatever build of the package is imported: run ONCE with the parent commit's build on an MI355X.
    (The parent's library has no plan exports: the shapes come from the restatement, which tests/test_adjoint_launch_plans.py holds
    equal to the exports, and the one-draw plans are not asked.)"""
    global RESTATED_PLANS
    RESTATED_PLANS = True
    out = {}
    for kind, shape, mode in ONE_BAND:
        out.update(_one_band_case(kind, shape, mode)[2])
    for kind in ("linear", "rbf"):
        out.update(_paired_case(kind)[2])
        for which in ONE_DRAW:
            out.update(_multiband_case(which, kind)[0])
            out.update(_deriv_case(which, kind)[0])
    np.savez_compressed(path, **out)
    return path


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN, allow_pickle=False))


def _hold(what, got, checks, gold):
    same = {k: bool(np.array_equal(v, gold[k], equal_nan=True)) for k, v in got.items()}
    for name, err, tol in checks:
        print("%s: %-44s %.3e  bound %.1e" % (what, name, err, tol))
    print("%s: bit-identical to the parent %s" % (what, same))
    for name, err, tol in checks:
        assert err <= tol, (what, name, err, tol)
    assert all(same.values()), "%s: not bit-identical to the parent commit's: %s" % (what, [k for k, v in same.items() if not v])


# ---- the tests --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind,shape,mode", ONE_BAND, ids=["%s_%s_%s" % c for c in ONE_BAND])
def test_one_band_adjoint_launches_keep_every_bit_and_match_the_oracle(kind, shape, mode, gold):
    A, p, got, checks = _one_band_case(kind, shape, mode)
    launches = -(-A // p["rows_per_launch"]) if p["rows_per_launch"] else 1
    print("%s %s %s: %d x %d, plan %s, %d launches" % (kind, shape, mode, A, B1, p, launches))
    assert launches >= 3 if shape == "several" else (launches == 1 and A * p["nch"] == _n_cu() * 8 * GEOM[(kind, mode == "yside")][0])
    _hold("%s %s %s" % (kind, shape, mode), got, checks, gold)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["linear", "rbf"])
def test_paired_batch_of_several_pairs_per_lane_group(kind, gold):
    P, p, got, checks = _paired_case(kind)
    print("%s paired: %d pairs, plan %s" % (kind, P, p))
    assert p["ppp"] == 2 and p["groups"] == (P + 1) // 2
    _hold("%s paired" % kind, got, checks, gold)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["linear", "rbf"])
@pytest.mark.parametrize("which", ONE_DRAW)
def test_multiband_forward_and_adjoint_on_a_one_draw_launch(which, kind, gold):
    got, checks = _multiband_case(which, kind)
    _hold("multi-band %s %s" % (which, kind), got, checks, gold)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["linear", "rbf"])
@pytest.mark.parametrize("which", ONE_DRAW)
def test_fused_derivative_solver_on_a_one_draw_launch(which, kind, gold):
    got, checks = _deriv_case(which, kind)
    _hold("derivative solver %s %s" % (which, kind), got, checks, gold)
