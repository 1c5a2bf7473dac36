#!/usr/bin/env python3
"""The distance of the CPU fp64 torch restatement of the truncated kernel (sigkernel_amd/truncated.py: _level_sums on _step_gram or on the
second differences of RBFKernel.Gram_matrix, and autograd through it) from the long-double yardstick (tests/truncated_value_regimes.py)
on every measured case of the truncated value-regime table.  The GPU test's bound is base + 4 x this (none for the cases marked
invariant); the script runs on the CPU and imports the restatement and the yardstick, never a kernel.

Recorded per case: "value" -- per level m, the maximum over pairs of (|restatement - yardstick| - floor) / scale[m][pair], floor the
below-double-range allowance of truncated_value_regimes.level_floor; "dX" / "dY" (gradient rows) -- the maximum over paths of
|restatement - yardstick| over the path / the path's largest yardstick entry.  `offset` entries hold the maximum over
truncated_value_regimes.OFFSET_SEEDS seeds, all others seed 0.  Numbers are kept to three significant digits, rounded up.

    python tests/golden/measure_truncated_value_regimes.py        # rewrites tests/golden/truncated_value_regimes.json
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import truncated_value_regimes as T  # noqa: E402

PATH = os.path.join(HERE, "truncated_value_regimes.json")


def restatement(row, sigma, X, Y, w=None):
    """the restatement's results on CPU fp64 tensors, as the row's call reaches it: an object row through TruncatedSigKernel on the
    PATHS; a function or long row through _truncated_levels_torch on the STEPS it is given, and so an fp32 row -- on the exact fp64
    values of its fp32 steps, since the kernel's arithmetic is fp64 whatever the dtype at its ends (an fp32 restatement would be off by
    1e-7 and allow as much) -> {"levels", and with w "dX", "dY"} numpy"""
    import sigkernel_amd
    from sigkernel_amd import truncated
    dt = torch.float64
    Xt = torch.from_numpy(np.array(X)).to(dt)
    Yt = Xt if Y is X else torch.from_numpy(np.array(Y)).to(dt)
    paired, sym = row["op"] == "paired", row["op"] == "sym"
    if row["api"] != "object" or row["f32"]:
        kx, ky = T.kernel_inputs(row, X, Y)
        lev = truncated._truncated_levels_torch(torch.from_numpy(kx).to(dt), torch.from_numpy(ky).to(dt), row["L"], row["order"], paired)
        return {"levels": lev.double().numpy()}
    static = sigkernel_amd.RBFKernel(sigma) if row["variant"] == "rbf" else None
    tk = sigkernel_amd.TruncatedSigKernel(row["L"], 1., row["order"], static_kernel=static)
    if w is None:
        return {"levels": tk._levels(Xt, Yt, paired, sym).double().numpy()}
    Xg = Xt.clone().requires_grad_(True)
    Yg = Xg if sym else Yt.clone().requires_grad_(True)
    lev = tk._levels(Xg, Yg, paired, sym)
    (lev[1:] * torch.from_numpy(np.array(w))).sum().backward()
    return {"levels": lev.detach().double().numpy(), "dX": Xg.grad.numpy(), "dY": None if sym else Yg.grad.numpy()}


def value_distance(row, got, want):
    """per level: max over pairs of (|got - want| - floor) / scale, 0 where the scale is 0"""
    lev, scale = want["levels"], want["scale"]
    excess = np.maximum(np.abs(np.asarray(got, dtype=T.LD) - lev) - T.level_floor(row, scale), 0)
    return [float(np.max(np.where(scale[m] > 0, excess[m] / np.where(scale[m] > 0, scale[m], 1), 0))) for m in range(lev.shape[0])]


def distance(row, fam, lab, seed):
    """one case and seed; the restatement runs on ONE thread, so that the rounding of its reductions does not move with the pool size"""
    want = T.case_want(row, fam, lab, seed)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        got = restatement(row, want["sigma"], want["X"], want["Y"], want.get("w"))
    finally:
        torch.set_num_threads(threads)
    out = {"value": value_distance(row, got["levels"], want)}
    for name in ("dX", "dY"):
        if name in row["outputs"]:
            out[name] = float(np.max(T.grad_errors(got[name], want[name], skip_zero=True)))
    return out


def _round(v):
    """three significant digits, never below the measurement"""
    if isinstance(v, list):
        return [_round(x) for x in v]
    if not (v > 0 and np.isfinite(v)):
        return float(v)
    q = 10.0 ** (int(np.floor(np.log10(v))) - 2)
    r = float("%.3g" % (np.ceil(v / q) * q))
    return r if r >= v else float("%.3g" % ((np.ceil(v / q) + 1) * q))


def measure(row, fam, lab, settings):
    ds = [distance(row, fam, lab, seed) for seed in (range(T.OFFSET_SEEDS) if fam == "offset" else (0,))]
    return {name: _round(np.max([d[name] for d in ds], axis=0).tolist()) for name in ds[0]}


def main():
    out = {}
    for key, entry in sorted(T.golden_entries().items()):
        out[key] = measure(*entry)
        print("%-72s value %.2e%s" % (key, max(out[key]["value"]), "".join("  %s %.2e" % (n, out[key][n]) for n in ("dX", "dY") if n in out[key])),
              flush=True)
    out["_provenance"] = ("distance of the CPU fp64 torch restatement from the long-double yardstick, values per level in units of the pair's "
                          "scale, gradients per path; offset: maximum over %d seeds; tests/golden/measure_truncated_value_regimes.py" % T.OFFSET_SEEDS)
    with open(PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
