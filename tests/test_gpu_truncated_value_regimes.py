"""Every launch-time mode of k_trunc_sig (csrc/sk_truncated.hip: plain, paired, levels, points, long, adjoint, points-adjoint,
long-adjoint, wide-adjoint) away from the unit-walk inputs -- tests/truncated_value_regimes.py: rescaled, offset and drifting paths, RBF
bandwidths over 14 decades, degenerate and non-finite paths -- against the LONG-DOUBLE yardstick, PER PAIR and PER LEVEL.  Each case runs
under the launch trace and asserts the row's instance of the kernel on it.

THE BOUND has one rule.
  Values, per level m and per pair:   |got - want| <= (1e-12 + 4 r) scale[m][pair] + floor
    * scale[m][pair] = sum over nodes and planes of |R^m| of THAT pair; 1e-12 is the README's bar for the truncated kernel;
    * r: the recorded distance of the CPU fp64 torch restatement from the yardstick on that case and level, in the same units
      (tests/golden/truncated_value_regimes.json, written by tests/golden/measure_truncated_value_regimes.py); 4 is the ledger's allowance
      for a measured stage (instance_ledger.py).  Cases marked invariant (every plain row on `offset`: the kernel works on steps; the
      points rows on `offset` and `sigma >= 1e2`: sk_truncated.hip:268-272) get r = 0: there the restatement loses up to 1e-3 and the
      kernel must not;
    * floor = n_nodes 2^-1022 max(1, scale[m-1][pair]): results below the double range only -- a level is a sum of n_nodes products
      G x (a prefix of the level below, at most scale[m-1]), each of which may lose 2^-1022 absolute when it is subnormal or flushed.
      A flush to zero passes, garbage does not;
    * a weighted value: the levels' bars summed with |sigma[m]|, plus (L + 1) 2^-53 sum_m |sigma[m] k_m| for forming the sum in fp64 (sigma[0]
      alone is 0.5 where the levels are 1e-50);  normalize=True, K / sqrt(kx ky) with kx, ky the weighted self kernels:
      first order, bar(K) / sqrt(kx ky) + |K / sqrt(kx ky)| (bar(kx) / 2 kx + bar(ky) / 2 ky + 2^-51) -- the self kernels' bars by the same rule with
      the case's r, 2^-51 for the sqrt, the product and the division;
    * fp32 output: two fp32 ulps of the level more, and 2^-126 absolute where the level is below the fp32 range (a flush passes); where
      |want| exceeds the fp32 range by more than an ulp the result must be the infinity of the right sign.
  Gradients, per path:  max |got - want| over the path <= (1e-10 + 4 r) max |want| over the path, r recorded the same way from CPU
  autograd of the restatement; invariant cases r = 0.  The upstream weights are w[m] = randn / max_pair scale[m]: every level counts.
  `degenerate`, on top: levels >= 1 of a constant path and levels above a path's number of non-zero steps are exactly 0.0; a pair of
  constant paths has gradient rows of exactly 0.0 (a constant path paired with a moving one HAS a gradient: d k_1 / d x_end = y_end - y_0);
  a sym=True call equals the general call on (X, X.clone()) bit for bit.
  `nonfinite` (no yardstick): every entry of the poisoned path's row (column) at levels >= 1 is non-finite and level 0 is 1; every other
  entry has the bits of the same call on the clean batch; a gradient of a path whose pairs do not involve the poisoned path keeps its bits,
  the poisoned path's own gradient is non-finite throughout.  This checks containment: the wave shares one y block in LDS among its lane
  groups, and hand-downs travel by DPP.

With SK_TRUNCATED_VALUE_REGIMES_REPORT=<file> every case appends its measured errors and bounds (profiles/truncated_value_regimes.txt)."""
import json
import os

import numpy as np
import pytest
import torch

import instance_ledger as LEDGER
import truncated_value_regimes as T
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "truncated_value_regimes.json")) as _f:
    RECORDED = json.load(_f)
CASES = T.cases()
LD = T.LD
F32_MAX, F32_TINY = float(np.finfo(np.float32).max), 2.0 ** -126


def _report(line):
    print(line)
    path = os.environ.get("SK_TRUNCATED_VALUE_REGIMES_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _short(names):
    return sorted(n.split("_GLOBAL__N_1")[-1][:48] for n in names)


def _np(t):
    return None if t is None else t.detach().double().cpu().numpy()


def _call(row, sigma, X, Y, w=None):
    """the row's call on the GPU -> {output: numpy fp64 (exact values of an fp32 result)}, the dtype of the levels"""
    import sigkernel_amd
    from sigkernel_amd import _lib
    dt = torch.float32 if row["f32"] else torch.float64
    L, order, paired, sym = row["L"], row["order"], row["op"] == "paired", row["op"] == "sym"
    sig = T.signed_sigma(L)
    out = {}
    if row["api"] == "object":
        static = sigkernel_amd.RBFKernel(sigma) if row["variant"] == "rbf" else None
        make = lambda s: sigkernel_amd.TruncatedSigKernel(L, s, order, static_kernel=static, **row["kw"])
        Xd = torch.from_numpy(np.array(X)).to(dt).cuda()
        Yd = Xd if Y is X else torch.from_numpy(np.array(Y)).to(dt).cuda()
        if w is None:
            lev = make(1.)._levels(Xd, Yd, paired, sym)
            if row["f32"]:      # the kernel's own weighted sum, rounded once (the object would add fp32 levels in fp32: inf - inf beyond the range)
                out["weighted"] = _np(sigkernel_amd.truncated_sig_kernel(Xd[:, 1:] - Xd[:, :-1], Yd[:, 1:] - Yd[:, :-1], L, sig, order))
            else:
                tk = make(torch.from_numpy(sig))
                out["weighted"] = _np(tk.compute_kernel(Xd, Yd) if paired else tk.compute_Gram(Xd, Yd, sym=sym))
        else:
            Xg = Xd.clone().requires_grad_(True)
            Yg = Xg if sym else Yd.clone().requires_grad_(True)
            lev = make(1.)._levels(Xg, Yg, paired, sym)
            (lev[1:] * torch.from_numpy(np.array(w)).cuda()).sum().backward()
            out["dX"], out["dY"] = _np(Xg.grad), (None if sym else _np(Yg.grad))
        out["levels"] = _np(lev)
        return out, lev.dtype
    kx, ky = T.kernel_inputs(row, X, Y)
    Xd, Yd = torch.from_numpy(kx).to(dt).cuda(), torch.from_numpy(ky).to(dt).cuda()
    if row["api"] == "long":
        be = _lib.get_backend()
        lev = be.truncated_long(Xd, Yd, L, None, paired, None, no_swap=True)
        out["levels"], out["weighted"] = _np(lev), _np(be.truncated_long(Xd, Yd, L, [float(v) for v in sig], paired, None, no_swap=True))
        return out, lev.dtype
    assert row["api"] == "function"
    lev = sigkernel_amd.truncated_sig_kernel_levels(Xd, Yd, L, order)
    out["levels"] = _np(lev)
    if "weighted" in row["outputs"]:
        out["weighted"] = _np(sigkernel_amd.truncated_sig_kernel(Xd, Yd, L, sig, order))
    if "normalized" in row["outputs"] and np.all(np.isfinite(kx)) and np.all(np.isfinite(ky)):
        out["normalized"] = _np(sigkernel_amd.truncated_sig_kernel(Xd, Yd, L, np.abs(sig), order, normalize=True))
    return out, lev.dtype


def _bars(row, want, r, f32):
    """bar[m][pair] of the module docstring; r: (L + 1,) per level"""
    scale, lev = want["scale"], want["levels"]
    allow = (LD(T.VALUE_BASE) + 4 * np.asarray(r, dtype=LD)).reshape((-1,) + (1,) * (scale.ndim - 1))
    bar = allow * scale + T.level_floor(row, scale)
    if f32 == "levels":
        with np.errstate(over="ignore"):      # (the spacing of the largest float is inf: such entries are judged as overflows)
            bar = bar + 2 * np.spacing(np.minimum(np.abs(lev), F32_MAX).astype(np.float32)).astype(LD) + LD(F32_TINY)
    bar[0] = 0
    return bar


def _check_values(what, got, want, bar, f32, bad, line):
    """|got - want| <= bar elementwise; an fp32 result whose yardstick is beyond the fp32 range: the infinity of the right sign"""
    got = np.asarray(got, dtype=LD)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    over = np.abs(want) > F32_MAX * (1 + 2.0 ** -23) if f32 else np.zeros(want.shape, dtype=bool)
    edge = (np.abs(want) > F32_MAX * (1 - 2.0 ** -23)) & ~over if f32 else over      # either the largest float or the infinity
    with np.errstate(invalid="ignore"):
        ok = np.where(over, got == np.sign(want) * LD(np.inf), np.where(edge, np.sign(got) == np.sign(want), np.abs(got - want) <= bar))
        rel = np.where(over | edge | (bar <= 0), 0, np.abs(got - want) / np.where(bar > 0, bar, 1))
    worst = float(np.max(np.where(np.isnan(rel), np.inf, rel)))
    line.append("%s %.2g of its bar%s" % (what, worst, " (%d beyond fp32: inf)" % int(over.sum()) if over.any() else ""))
    if not bool(np.all(ok)):
        idx = np.argwhere(~ok)[0]
        bad.append("%s: %d entries beyond their bar, first at %s: got %r want %r bar %.3e (worst %.3g of the bar)"
                   % (what, int((~ok).sum()), tuple(idx), float(got[tuple(idx)]), float(want[tuple(idx)]), float(bar[tuple(idx)]), worst))


def _weighted_ld(lev, sig):
    return sum(LD(sig[m]) * lev[m] for m in range(len(sig)))


def _sum_rounding(lev, sig):
    """forming sigma[0] + sum_m sigma[m] k_m in fp64, in any order: L + 1 roundings of partial sums of at most sum_m |sigma[m] k_m|"""
    return len(sig) * LD(2.0 ** -53) * sum(abs(LD(sig[m])) * np.abs(lev[m]) for m in range(len(sig)))


def _measured(row, fam, lab, st, names, line, bad):
    want = T.case_want(row, fam, lab)
    X, Y, sigma = want["X"], want["Y"], want["sigma"]
    rec = RECORDED[T.golden_key(row, fam, lab)]
    inv = T.is_invariant(row, fam, lab, st)
    r = np.zeros(row["L"] + 1) if inv else np.asarray(rec["value"])
    (out, dtype), launched = LEDGER.traced(lambda: _call(row, sigma, X, Y, want.get("w")))
    names |= launched
    f32 = row["f32"]
    assert dtype == (torch.float32 if f32 else torch.float64)
    bar, bar64 = _bars(row, want, r, "levels" if f32 else False), _bars(row, want, r, False)
    line.append("r %.1e%s" % (float(np.max(r)), " invariant" if inv else ""))
    lev = want["levels"]
    assert np.all(out["levels"][0] == 1.0)
    _check_values("levels", out["levels"], lev, bar, f32, bad, line)
    sig = T.signed_sigma(row["L"])
    if "weighted" in out:
        wv = _weighted_ld(lev, sig)      # fp32: the kernel rounds its fp64 sum once -- two fp32 ulps of the VALUE, 2^-126 below the range
        wbar = sum(abs(sig[m]) * bar64[m] for m in range(1, len(sig))) + _sum_rounding(lev, sig)
        if f32:
            with np.errstate(over="ignore"):
                wbar = wbar + 2 * np.spacing(np.minimum(np.abs(wv), F32_MAX).astype(np.float32)).astype(LD) + LD(F32_TINY)
        _check_values("weighted", out["weighted"], wv, wbar, f32, bad, line)
    if "normalized" in out:
        pos = np.abs(sig)
        kx, ky = T.kernel_inputs(row, X, Y)
        K, Kbar = _weighted_ld(lev, pos), sum(pos[m] * bar64[m] for m in range(1, len(pos))) + _sum_rounding(lev, pos)
        selfs = []
        for P in (kx, ky):
            sl, ss = T.want_levels(row["variant"], sigma, P, P, row["L"], row["order"], paired=True)
            sb = _bars(row, {"scale": ss, "levels": sl}, r, False)
            selfs.append((_weighted_ld(sl, pos), sum(pos[m] * sb[m] for m in range(1, len(pos))) + _sum_rounding(sl, pos)))
        (vx, bx), (vy, by) = selfs
        norm = np.sqrt(vx[:, None] * vy[None, :])
        Kn = K / norm
        nbar = Kbar / norm + np.abs(Kn) * (bx[:, None] / (2 * vx[:, None]) + by[None, :] / (2 * vy[None, :]) + LD(2.0 ** -51))
        _check_values("normalized", out["normalized"], Kn, nbar, f32, bad, line)
    for name in ("dX", "dY"):
        if name in row["outputs"]:
            tol = T.GRAD_BASE + (0.0 if inv else 4.0 * rec[name])
            err = T.grad_errors(out[name], want[name])
            line.append("%s %.2e bound %.2e" % (name, float(np.max(err)), tol))
            if not np.all(err <= tol):
                bad.append("%s: per path %s > %.3e" % (name, err, tol))
    if fam == "degenerate":
        _degenerate(row, sigma, X, Y, want, out, bad)


def _degenerate(row, sigma, X, Y, want, out, bad):
    lev, A, few = out["levels"], row["shape"][0], T.FEW_STEPS * row["order"]      # (order o visits a node up to o times: level <= o x steps)
    paired, sym = row["op"] == "paired", row["op"] == "sym"
    zero = [("a constant path of X", lev[1:, 0]), ("levels above the steps of a path of X", lev[few + 1:, A - 1])]
    if not paired:
        zero.append(("a constant path of Y", lev[1:, :, 0]))
    if sym:
        zero.append(("levels above the steps, second argument", lev[few + 1:, :, A - 1]))
    if paired and "dX" in out:
        zero += [("dX of a pair of constant paths", out["dX"][0]), ("dY of a pair of constant paths", out["dY"][0])]
    for what, v in zero:
        if not np.all(v == 0.0):
            bad.append("%s: not exactly 0.0 (largest %.3e)" % (what, float(np.max(np.abs(v)))))
    if sym:      # the general call on a second buffer, with the same gradient pending (so that it takes the same route)
        general, _ = _call(dict(row, op="gram"), sigma, X, X.copy(), want.get("w"))
        for name in ("levels", "weighted"):
            if name in out and not np.array_equal(out[name], general[name]):
                bad.append("sym=True %s differ from the general call's bits" % name)


def _bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


def _nonfinite(row, fam, lab, st, names, line, bad):
    want = T.case_want(row, fam, lab)                  # the clean batch: inputs, and the scales behind the upstream weights
    X, Y, sigma = want["X"], want["Y"], want["sigma"]
    Xp, Yp, side, p = T.poisoned(X, Y, st)
    w = want.get("w")
    clean, _ = _call(row, sigma, X, Y, w)
    (got, _), launched = LEDGER.traced(lambda: _call(row, sigma, Xp, Yp, w))
    names |= launched
    paired, sym = row["op"] == "paired", row["op"] == "sym"
    for name in ("levels", "weighted"):
        if name not in got:
            continue
        g, c = got[name], clean[name]
        lead = g.ndim - (1 if paired else 2)                      # 1 for the levels' leading axis
        hit = np.zeros(g.shape[lead:], dtype=bool)
        if paired:
            hit[p] = True
        else:
            if side == "X" or sym:
                hit[p, :] = True
            if side == "Y" or sym:
                hit[:, p] = True
        body = g[1:] if lead else g
        if lead and not np.all(g[0] == 1.0):
            bad.append("level 0 is not 1")
        n_fin = int(np.isfinite(body[..., hit]).sum())
        if n_fin:
            bad.append("%s: %d of %d entries of the poisoned path are finite" % (name, n_fin, body[..., hit].size))
        if not _bits(g[..., ~hit], c[..., ~hit]):
            bad.append("%s: an entry of a clean pair lost the clean call's bits" % name)
        line.append("%s: %d poisoned entries, %d finite; %d clean entries" % (name, body[..., hit].size, n_fin, g[..., ~hit].size))
    for name in ("dX", "dY"):
        if name not in row["outputs"]:
            continue
        g, c = got[name], clean[name]
        own = name[1] == side or sym
        if own and np.isfinite(g[p]).any():
            bad.append("%s of the poisoned path: %d of %d entries are finite" % (name, int(np.isfinite(g[p]).sum()), g[p].size))
        keep = [q for q in range(g.shape[0]) if q != p] if (own or paired) and not sym else []      # paths none of whose pairs involve it
        if keep and not _bits(g[keep], c[keep]):
            bad.append("%s: a path whose pairs are all clean lost the clean call's bits" % name)
        line.append("%s: %d paths keep their bits" % (name, len(keep)))


@pytest.mark.parametrize("case", CASES, ids=[T.case_id(c) for c in CASES])
def test_mode_matches_the_long_double_yardstick(case, monkeypatch):
    import sigkernel_amd
    row, fam, lab, st = case
    for knob, v in row["knobs"].items():
        monkeypatch.setattr(sigkernel_amd.routes, knob, v)
    names, line, bad = set(), [], []
    (_nonfinite if fam == "nonfinite" else _measured)(row, fam, lab, st, names, line, bad)
    _report("%-58s %-10s %-12s %s" % (row["id"], fam, lab, "; ".join(line)))
    assert any(row["claim"] in n for n in names), "%s no longer launches %s (launched: %s)" % (row["id"], row["claim"], _short(names))
    assert not bad, "%s %s %s: %s" % (row["id"], fam, lab, "; ".join(bad))
