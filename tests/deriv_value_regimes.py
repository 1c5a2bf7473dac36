"""Derivative Gram (compute_kernel_and_derivatives_Gram, k_kgrad): families, inputs, the long-double yardstick and the row table of
tests/test_deriv_value_regimes_host.py and tests/test_gpu_deriv_value_regimes.py (test infrastructure; numpy and torch's CPU arithmetic for
the perturbed paths only -- nothing but call() at the end imports the product package, nothing the oracle).

The operation: X1 = X + eps gamma and X2 = X + 2 eps gamma are formed in fp64 by torch exactly as k_kgrad forms them (sigkernel.py:1136,
eps = 1e-4) -- their rounding is part of the operation, not of the error -- and the three static Gram matrices of (X, Y), (X1, Y), (X2, Y)
give increments I0, I1, I2; inc = I0, inc_gamma = (I1 - I0) / eps, inc_gamma_gamma = (I0 - 2 I1 + I2) / eps^2 drive the reference's coupled
three-state stencil (oracle/sigkernel_oracle.c:328-339; boundary K = 1, K_gamma = K_gamma_gamma = 0).  The yardstick is that, in numpy long
double: value_regimes.increments_ld (coordinate differences) for I0, I1, I2, value_regimes.tile, and the stencil swept by anti-diagonals.
Its K state is value_regimes.solve_diag_ld's expression, so its k has gram_ld's bits.

The families are the derivative's own: the finite differences amplify the rounding of a node value by 1 / eps^2 = 1e8, so the value
regimes at offsets of 1e2 and above or sigma >= 1e6 leave the reference's |x|^2 + |y|^2 - 2 <x, y> no digit of k_gamma_gamma and judge
nothing.  What is left:

    rbf      drift s in {5, 30} (sigma = 1); sigma in {1e-2, 1e2} on unit walks; scale s in {0.3, 3, 10} (sigma = 0.8);
             offset c in {1, 5} (sigma = 0.8)
    linear   scale s in {0.1, 3}; offset (c, c), c in {1, 10}; offset (0.5, -1.5)
    gamma    randn of X's shape from a seeded generator

Three settings are nearer than first planned, because at the final shapes the oracle alone left only 63 % of the k_gamma_gamma entries
judged (recorded <= 1e-5), below the 80 % the table has to keep: rbf scale 0.1 -> 0.3 (1.2e-5 .. 1.6e-5 at five shapes), rbf offset 10 -> 5
(1.1e-5 .. 3.0e-5 at nine), linear offset (10, -30) -> (0.5, -1.5) (1e-4 .. 4e-3 everywhere; (1, -3) still left six above 1e-5).  Linear
offset (10, 10) and sigma = 1e2 stay as the cases whose k_gamma_gamma the oracle cannot judge.

The error measure, per output: max |got - want| / max(max |want| over the (A, B) matrix, 1e-300) -- the matrix norm on purpose: a pair's
noise scales with |G| / eps^2, not with its own value; batches stay at 6 pairs or fewer, so little can hide behind a neighbour.

The bound, one rule: base + 4 x recorded, base = 1e-10 (the ledger's value tolerance) for all three outputs, recorded = the distance of the
CPU oracle's kgrad from the yardstick on that (family, setting, kind, shape, output), the maximum over SEEDS seeds of paths and gamma
(tests/golden/deriv_value_regimes.json, written by tests/golden/measure_deriv_value_regimes.py), 4 = the ledger's factor for a differing
summation order and a different exp.  An output of a case is JUDGED when recorded <= JUDGED_CAP: above that the oracle itself has lost the
digits and the bound says little; the host test holds the share of judged entries (every k; >= 85 % of all; >= 80 % of k_gamma_gamma)."""
import functools
import re

import numpy as np

import value_regimes as V
from ld_reference import LD

EPS = 1e-4                                   # k_kgrad's default step
SEEDS = 8                                    # recorded = the maximum over seeds 0 .. SEEDS - 1
GPU_SEED = 0                                 # the GPU test's draw: one of the recorded seeds
BASE = 1e-10                                 # instance_ledger.TOL64["value"]
FACTOR = 4.0
JUDGED_CAP = 1e-5
OUTPUTS = ("k", "k_gamma", "k_gamma_gamma")
KINDS = V.KINDS

FAMILIES = {
    "drift": {"rbf": [("s=%g" % s, {"drift": s, "sigma": 1.0}) for s in (5.0, 30.0)]},
    "sigma": {"rbf": [("sigma=%g" % s, {"sigma": s}) for s in (1e-2, 1e2)]},
    "scale": {"rbf": [("s=%g" % s, {"scale": s, "sigma": 0.8}) for s in (0.3, 3.0, 10.0)],
              "linear": [("s=%g" % s, {"scale": s}) for s in (0.1, 3.0)]},
    "offset": {"rbf": [("c=%g" % c, {"offset": (c, c), "sigma": 0.8}) for c in (1.0, 5.0)],
               "linear": [("c=%g" % c, {"offset": (c, c)}) for c in (1.0, 10.0)] + [("c=0.5,-1.5", {"offset": (0.5, -1.5)})]},
}
# sigma = 1, no scale, no offset: the host test of the yardstick and the degenerate batch shapes
FAMILIES["unit"] = {"rbf": [("sigma=1", {"sigma": 1.0})], "linear": [("plain", {})]}
MAIN = ("drift", "sigma", "scale", "offset")


def family_cases(kind, families=MAIN):
    return [(f, lab, st) for f in FAMILIES if f in families for lab, st in FAMILIES[f].get(kind, [])]


# ------------------------------------------------------------------------------------------------------------------- inputs
def shape(A, B, M, N, D, d, f32=False, Lx=0):
    """Lx > 0: function-valued paths (batch, length, Lx, D / Lx) -- the static kernel's `features` flattens them to D channels"""
    sh = V.shape(A, B, M, N, D, d, f32=f32)
    sh["Lx"] = int(Lx)
    return sh


def shape_key(sh):
    return V.shape_key(sh) + ("_Lx%d" % sh["Lx"] if sh.get("Lx") else "")


def inputs(settings, sh, seed=GPU_SEED, gamma_rows=None, gamma_scale=1.0):
    """-> X (A,M,D), Y (B,N,D), gamma (A,M,D), X1, X2 (numpy fp64; fp32-representable for an fp32 shape), sigma or None.  X, Y are
    value_regimes.inputs' draw; gamma = randn of X's shape from a generator of its own; X1 = X + eps gamma and X2 = X + 2 eps gamma by
    torch, in the inputs' dtype, as k_kgrad forms them.  gamma_rows: rows of gamma kept, the others zeroed (the property tests)."""
    import torch
    if "drift" in settings and sh["N"] < 8:      # (value_regimes.drift_schedule needs 8 points: the same even steps without the four extra ones)
        X, Y, _, sigma = V.inputs({k: v for k, v in settings.items() if k != "drift"}, sh, seed)
        Y = Y + settings["drift"] * np.sqrt(3.0 / sh["D"]) * np.linspace(0.0, 1.0, sh["N"])[None, :, None]
        if sh["f32"]:
            Y = Y.astype(np.float32).astype(np.float64)
    else:
        X, Y, _, sigma = V.inputs(settings, sh, seed)
    gen = torch.Generator().manual_seed(7919 + int(seed))
    gamma = torch.randn(X.shape, generator=gen, dtype=torch.float64) * gamma_scale
    if gamma_rows is not None:
        keep = torch.zeros(X.shape[0], dtype=torch.bool)
        keep[list(gamma_rows)] = True
        gamma = torch.where(keep[:, None, None], gamma, torch.zeros_like(gamma))
    dt = torch.float32 if sh["f32"] else torch.float64
    Xt, gt = torch.from_numpy(X).to(dt), gamma.to(dt)
    X1, X2 = Xt + EPS * gt, Xt + 2. * EPS * gt      # sigkernel.py:1136
    return X, Y, gt.double().numpy(), X1.double().numpy(), X2.double().numpy(), sigma


# ------------------------------------------------------------------------------------------------------------------- yardstick
def deriv_increments_ld(kind, sigma, X, X1, X2, Y, eps=EPS):
    """-> the coarse increments (inc, inc_gamma, inc_gamma_gamma), (A,B,M-1,N-1) long double each"""
    I0, I1, I2 = (V.increments_ld(kind, sigma, P, Y)[0] for P in (X, X1, X2))
    e = LD(eps)
    return I0, (I1 - I0) / e, (I0 - LD(2) * I1 + I2) / (e * e)


def solve_deriv_diag_ld(inc, incd, incdd):
    """The reference's coupled three-state stencil (oracle/sigkernel_oracle.c:328-339) on FINE increments [..., MM, NN] in long double,
    swept by anti-diagonals -> (k, k_gamma, k_gamma_gamma) [...] at the last node.  The K state is value_regimes.solve_diag_ld's
    expression, operand for operand."""
    MM, NN = inc.shape[-2:]
    lead = inc.shape[:-2]
    K = np.ones(lead + (MM + 1, NN + 1), dtype=LD)
    Kd, Kdd = np.zeros_like(K), np.zeros_like(K)
    one, half, twelfth, quarter, two = LD(1), LD(0.5), LD(1) / LD(12), LD(0.25), LD(2)
    for s in range(MM + NN - 1):
        i = np.arange(max(0, s - NN + 1), min(MM - 1, s) + 1)
        j = s - i
        g, gd, gdd = inc[..., i, j], incd[..., i, j], incdd[..., i, j]
        k01, k10, k00 = K[..., i, j + 1], K[..., i + 1, j], K[..., i, j]
        k01d, k10d, k00d = Kd[..., i, j + 1], Kd[..., i + 1, j], Kd[..., i, j]
        k01dd, k10dd, k00dd = Kdd[..., i, j + 1], Kdd[..., i + 1, j], Kdd[..., i, j]
        k11 = (k10 + k01) * (one + half * g + twelfth * g * g) - k00 * (one - twelfth * g * g)
        f1 = k00 * gd + k00d * g
        f2 = k01 * gd + k01d * g
        f3 = k10 * gd + k10d * g
        f4 = k11 * gd + (k01d + k10d - k00d + f1) * g
        k11d = k01d + k10d - k00d + quarter * (f1 + f2 + f3 + f4)
        h1 = k00 * gdd + two * k00d * gd + k00dd * g
        h2 = k01 * gdd + two * k01d * gd + k01dd * g
        h3 = k10 * gdd + two * k10d * gd + k10dd * g
        h4 = k11 * gdd + two * k11d * gd + (k01dd + k10dd - k00dd + h1) * g
        k11dd = k01dd + k10dd - k00dd + quarter * (h1 + h2 + h3 + h4)
        K[..., i + 1, j + 1], Kd[..., i + 1, j + 1], Kdd[..., i + 1, j + 1] = k11, k11d, k11dd
    return K[..., -1, -1], Kd[..., -1, -1], Kdd[..., -1, -1]


def kgrad_ld(kind, sigma, X, X1, X2, Y, d, eps=EPS):
    """-> (k, k_gamma, k_gamma_gamma), (A,B) long double each"""
    return solve_deriv_diag_ld(*(V.tile(a, d) for a in deriv_increments_ld(kind, sigma, X, X1, X2, Y, eps)))


def error(got, want):
    """max |got - want| / max(max |want| over the matrix, 1e-300); inf for a non-finite result"""
    got64 = np.asarray(got, dtype=np.float64)
    want = np.asarray(want).astype(LD)
    assert got64.shape == want.shape, (got64.shape, want.shape)
    if not np.all(np.isfinite(got64)):
        return float("inf")
    return float(np.max(np.abs(got64.astype(LD) - want)) / max(np.max(np.abs(want)), LD(1e-300)))


def outputs_of(sh):
    """the outputs a shape is judged on: fp32 inputs on k alone (with eps = 1e-4 an fp32 finite difference keeps 3 digits of k_gamma and
    none of k_gamma_gamma)"""
    return OUTPUTS[:1] if sh["f32"] else OUTPUTS


def errors(got3, want3, names=OUTPUTS):
    return {name: error(g, w) for name, g, w in zip(OUTPUTS, got3, want3) if name in names}


F32_STAGE = "k_f32_stage"      # recorded for fp32 shapes beside k: see bound()


def bound(recorded, name, f32=False):
    """base + 4 x recorded.  fp32 inputs (k alone) carry the instance ledger's fp32 allowance on top: two fp32 ulps for the rounding of the
    output (instance_ledger.F32_ULPS2), and -- the unfused route hands node values and the three increment arrays from launch to launch
    in fp32 (instance_ledger.F32_STAGE_SOURCE["deriv_fused"]) -- 4 x the recorded distance of the ledger's fp32-stage restatement
    (instance_ledger.expected_f32_stage) from the yardstick"""
    if not f32:
        return BASE + FACTOR * recorded[name]
    assert name == "k"
    return BASE + 2.0 ** -22 + FACTOR * (recorded[name] + recorded[F32_STAGE])


# ------------------------------------------------------------------------------------------------------------------- rows
# One row per route family at the smallest shape that reaches it (A, B, M, N, D, dyadic).  op: "api" (SigKernel.compute_kernel_and_
# derivatives_Gram), "api_subclass" (a subclass of RBFKernel: never fused), "api_functional" (RBF_ID_Kernel on 4-D batches) or "simple"
# (be.solve_deriv(flags=FLAG_SIMPLE) on the increments of be.static_deriv_increments: no public shape reaches k_deriv_simple -- the fast
# solver covers every aligned layout the library produces below 160 KB of LDS).  claims: regular expressions, each must match the mangled
# name of a launched instance ({dy}: the dyadic order, {kno}: 0 linear / 1 rbf); forbid: must match none.
# The fused solver's plan (sk_wave_deriv_fused.hip: df_plan): units of two columns, NU = (Nc + 2) / 2 rounded up to 8 is NUp; in scope from
# NUp >= 64; bands of 64 coarse rows; several bands hand the boundary row down through the LDS ring when NUp < 80 (template flag LDSB, the
# fourth of k_deriv_fused<DY, KIND, FD, LDSB, SHIFT>) and through L2 from 80 on.
def _row(name, shapes, op="api", kinds=KINDS, knobs=None, claims=(), forbid=(), outputs=OUTPUTS, families=MAIN):
    return {"name": name, "op": op, "shapes": shapes, "kinds": kinds, "knobs": knobs or {}, "claims": claims, "forbid": forbid, "outputs": outputs,
            "families": families}


FUSED = r"k_deriv_fusedILi{dy}ELi{kno}ELi8ELb%dE"
NODES3 = r"k_static_nodesI[df]Li\d+ELi{kno}ELi3E"      # k_static_nodes<T, DMAX, KIND, NV = 3, CPT>: X, X + eps gamma, X + 2 eps gamma in one launch
WAVE = r"k_deriv_waveI[df]Li{dy}E"
UNFUSED = (NODES3, WAVE)
GENERIC = ("k_deriv_increments", WAVE)
SHORT = shape(2, 2, 12, 10, 3, 1)
LONG2 = shape(2, 2, 20, 130, 3, 1)
ROWS = [
    _row("fused, one band (no boundary to hand down)", [shape(2, 2, 20, 130, 3, 0), LONG2], claims=(FUSED % 0,), forbid=(NODES3, "k_deriv_wave")),
    _row("fused, three bands, boundary through the LDS ring", [shape(2, 2, 130, 128, 5, 1)], claims=(FUSED % 1,), forbid=(NODES3, "k_deriv_wave")),
    _row("fused, two bands, boundary through L2", [shape(2, 3, 70, 200, 8, 0)], claims=(FUSED % 0,), forbid=(NODES3, "k_deriv_wave")),
    _row("fused, dyadic 2", [shape(2, 2, 20, 161, 2, 2)], claims=(FUSED % 0,), forbid=(NODES3, "k_deriv_wave")),
    _row("static increments + wave solver, short second path", [SHORT, shape(2, 2, 9, 9, 8, 2)], claims=UNFUSED, forbid=("k_deriv_fused",)),
    _row("static increments + wave solver, dim 12", [shape(2, 2, 12, 10, 12, 1)], claims=UNFUSED, forbid=("k_deriv_fused",)),
    _row("static increments + wave solver, dim 20", [shape(2, 2, 12, 10, 20, 1)], claims=UNFUSED, forbid=("k_deriv_fused",)),
    _row("generic route, paths over 32 dims", [shape(2, 2, 12, 10, 40, 1)], claims=GENERIC, forbid=("k_deriv_fused", "k_static_nodes")),
    _row("generic route, RBFKernel subclass", [SHORT], op="api_subclass", kinds=("rbf",), claims=GENERIC, forbid=("k_deriv_fused", "k_static_nodes")),
    _row("dyadic 3 (host-refined increments, dyadic-2 solver)", [shape(2, 2, 8, 7, 3, 3)], claims=(NODES3, r"k_deriv_waveI[df]Li2E"),
         forbid=("k_deriv_fused",)),
    _row("no_fused_deriv on a long second path", [LONG2], knobs={"no_fused_deriv": True}, claims=UNFUSED, forbid=("k_deriv_fused",)),
    _row("k_deriv_simple on the backend's increments", [SHORT], op="simple", claims=(NODES3, "k_deriv_simple"), forbid=("k_deriv_fused", "k_deriv_wave")),
    _row("function-valued static kernel (RBF_ID_Kernel)", [shape(2, 2, 8, 7, 6, 1, Lx=6)], op="api_functional", kinds=("rbf",), claims=UNFUSED,
         forbid=("k_deriv_fused",)),
    # fp32 inputs: with eps = 1e-4 an fp32 finite difference keeps 3 digits of k_gamma and none of k_gamma_gamma -- judged on k alone
    _row("fp32 inputs (k alone)", [shape(2, 2, 12, 10, 3, 1, f32=True)], claims=UNFUSED, forbid=("k_deriv_fused",), outputs=("k",)),
]
NOT_FUSED = ("k_deriv_fused",)
ONLY_FUSED = (NODES3, "k_deriv_wave")
# Degenerate batches on unit-scale inputs: one path on either side, one coarse row, one coarse column, and the two sides of the fused
# solver's scope.  Its docstring names 126 points; df_plan's condition NUp >= 64 is met from Nc = 112, a second path of 113 points: both
# pairs of lengths are rows, each with the kernel its trace has to show.
DEGENERATE = [
    _row("unfused, A = 1", [shape(1, 2, 12, 10, 3, 1)], claims=UNFUSED, forbid=NOT_FUSED, families=("unit",)),
    _row("unfused, B = 1", [shape(2, 1, 12, 10, 3, 1)], claims=UNFUSED, forbid=NOT_FUSED, families=("unit",)),
    _row("unfused, M = 2 (one coarse row)", [shape(2, 2, 2, 10, 3, 1)], claims=UNFUSED, forbid=NOT_FUSED, families=("unit",)),
    _row("unfused, N = 2 (one coarse column)", [shape(2, 2, 12, 2, 3, 1)], claims=UNFUSED, forbid=NOT_FUSED, families=("unit",)),
    _row("fused, A = 1", [shape(1, 2, 20, 130, 3, 1)], claims=(FUSED % 0,), forbid=ONLY_FUSED, families=("unit",)),
    _row("fused, B = 1", [shape(2, 1, 20, 130, 3, 1)], claims=(FUSED % 0,), forbid=ONLY_FUSED, families=("unit",)),
    _row("fused, M = 2 (one coarse row)", [shape(2, 2, 2, 130, 3, 1)], claims=(FUSED % 0,), forbid=ONLY_FUSED, families=("unit",)),
    _row("fused, N = 126 and N = 125", [shape(2, 2, 20, 126, 3, 1), shape(2, 2, 20, 125, 3, 1)], claims=(FUSED % 0,), forbid=ONLY_FUSED,
         families=("unit",)),
    _row("fused, N = 113: the first length in scope", [shape(2, 2, 20, 113, 3, 1)], claims=(FUSED % 0,), forbid=ONLY_FUSED, families=("unit",)),
    _row("unfused, N = 112: the last length out of scope", [shape(2, 2, 20, 112, 3, 1)], claims=UNFUSED, forbid=NOT_FUSED, families=("unit",)),
]
ALL_ROWS = ROWS + DEGENERATE
_SHAPES = {shape_key(sh): sh for row in ALL_ROWS for sh in row["shapes"]}


def claims_of(row, kind, sh, which="claims"):
    return [c.format(dy=sh["d"], kno=0 if kind == "linear" else 1) for c in row[which]]


def check_trace(row, kind, sh, names):
    """-> (claims no launched instance matches, forbidden patterns that one does)"""
    missing = [c for c in claims_of(row, kind, sh) if not any(re.search(c, n) for n in names)]
    present = [c for c in claims_of(row, kind, sh, "forbid") if any(re.search(c, n) for n in names)]
    return missing, present


def route_cases():
    """[(row, shape, kind, family, parameter label, settings)] -- every cell of the GPU test"""
    return [(row, sh, kind, fam, lab, st) for row in ALL_ROWS for sh in row["shapes"] for kind in row["kinds"]
            for fam, lab, st in family_cases(kind, row["families"])]


def golden_key(fam, lab, kind, sh):
    return "%s|%s|%s|%s" % (fam, lab, kind, shape_key(sh))


def golden_entries():
    """the distinct (family, parameter, kind, shape) of route_cases(), keyed as deriv_value_regimes.json is"""
    out = {}
    for row, sh, kind, fam, lab, st in route_cases():
        out.setdefault(golden_key(fam, lab, kind, sh), (fam, lab, kind, sh, st))
    return out


def stacked_want(kind, draws, d):
    """the yardstick of several draws of one shape in ONE sweep: draws = [(X, X1, X2, Y, sigma)] -> three arrays (len(draws), A, B)"""
    incs = [deriv_increments_ld(kind, sg, X, X1, X2, Y) for X, X1, X2, Y, sg in draws]
    return solve_deriv_diag_ld(*(V.tile(np.stack([t[i] for t in incs]), d) for i in range(3)))


@functools.lru_cache(maxsize=None)
def _shape_wants(key, kind):
    """{(family, label): (k, k_gamma, k_gamma_gamma)} of every case of a shape and static kernel at the GPU test's seed, in one sweep"""
    sh = _SHAPES[key]
    cases = sorted(set((fam, lab) for row, sh_, kind_, fam, lab, st in route_cases() if kind_ == kind and shape_key(sh_) == key))
    draws = []
    for fam, lab in cases:
        X, Y, _, X1, X2, sigma = inputs(dict(FAMILIES[fam][kind])[lab], sh)
        draws.append((X, X1, X2, Y, sigma))
    want = stacked_want(kind, draws, sh["d"])
    return {case: tuple(w[n] for w in want) for n, case in enumerate(cases)}


def case_want(fam, lab, kind, sh):
    """the yardstick's three matrices of a case of the table, computed once per process (and per shape and static kernel, not per case)"""
    return _shape_wants(shape_key(sh), kind)[fam, lab]


# ------------------------------------------------------------------------------------------------------------------- the call
def call(row, sh, kind, sigma, X, Y, gamma, device="cpu", workspace_bytes=None):
    """the row's call on numpy inputs -> (k, k_gamma, k_gamma_gamma) tensors on `device` (the only function here that imports the
    product package: on the backend that is installed -- the HIP one on a GPU, the oracle-backed fake in the host test)"""
    import torch
    dt = torch.float32 if sh["f32"] else torch.float64
    return call_tensors(row, sh, kind, sigma, *(torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(device) for a in (X, Y, gamma)),
                        workspace_bytes=workspace_bytes)


def call_tensors(row, sh, kind, sigma, Xd, Yd, gd, workspace_bytes=None):
    import sigkernel_amd
    from sigkernel_amd import _lib
    op = row["op"]
    if op == "simple":
        be = _lib.get_backend()
        inc3 = be.static_deriv_increments(0 if kind == "linear" else 1, 1.0 if kind == "linear" else float(sigma), Xd.contiguous(),
                                          Xd + EPS * gd, Xd + 2. * EPS * gd, Yd.contiguous(), EPS)
        return be.solve_deriv(inc3, sh["d"], flags=_lib.FLAG_SIMPLE)
    if op == "api_subclass":
        class MyRBF(sigkernel_amd.RBFKernel):      # a subclass is never fused
            pass
        kern = MyRBF(sigma)
    elif op == "api_functional":
        kern = sigkernel_amd.RBF_ID_Kernel(sigma)
        Lx = sh["Lx"]
        Xd, Yd, gd = (t.reshape(t.shape[0], t.shape[1], Lx, t.shape[2] // Lx) for t in (Xd, Yd, gd))
    else:
        kern = sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(sigma)
    sk = sigkernel_amd.SigKernel(kern, sh["d"], **({} if workspace_bytes is None else {"workspace_bytes": workspace_bytes}))
    return sk.compute_kernel_and_derivatives_Gram(Xd, Yd, gd)
