#!/usr/bin/env python3
"""The distance of the CPU oracle's kgrad from the long-double yardstick of the derivative Gram (tests/deriv_value_regimes.py) on every
(family, parameter, static kernel, shape) of its case table, per output (k, k_gamma, k_gamma_gamma): what the REFERENCE's own arithmetic
(the static Gram matrices in double from |x|^2 + |y|^2 - 2 <x, y> / <x, y>, scaled by 1 / eps and 1 / eps^2, differenced, summed) has
lost there.  The GPU test's bound is base + 4 x this.  Each entry is the MAXIMUM over deriv_value_regimes.SEEDS seeds of paths and gamma
(the digits a finite difference loses vary by a factor 3 from draw to draw); the GPU test draws one of those seeds.  The script imports
the oracle and the yardstick, never the product's kernels: the static kernels are measure_value_regimes' restatements of the reference's
two formulas in torch.

    python tests/golden/measure_deriv_value_regimes.py        # rewrites tests/golden/deriv_value_regimes.json
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE]

import deriv_value_regimes as DV  # noqa: E402
from measure_value_regimes import static_kernel  # noqa: E402
from oracle import oracle as O  # noqa: E402

PATH = os.path.join(HERE, "deriv_value_regimes.json")


def oracle_kgrad(kind, sigma, X, Y, gamma, d):
    """the oracle on the doubles the library sees (fp32 inputs: the perturbed paths are formed in fp32, so gamma goes in as it is and
    only k is judged -- the oracle's k does not depend on gamma)"""
    return O.kgrad(torch.from_numpy(X), torch.from_numpy(Y), torch.from_numpy(gamma), static_kernel(kind, sigma), d, eps=DV.EPS)


def f32_stage_k(kind, sigma, X, Y, gamma, sh):
    """k of the instance ledger's restatement of the fp32 stages of the call (instance_ledger.expected_f32_stage: node values rounded to
    fp32, their scaling and 4-corner differences in fp32, the three increment arrays fp32, the sweep fp64)"""
    import instance_ledger as L
    spec = {"op": "kgrad", "dtype": "f32", "dyadic": sh["d"], "kind": kind, "param": sigma, "A": sh["A"], "B": sh["B"]}
    t = {"X": torch.from_numpy(X), "Y": torch.from_numpy(Y), "gamma": torch.from_numpy(gamma)}
    return L.expected_f32_stage(spec, t)["k"]


def measure(fam, lab, kind, sh, settings, seeds=None):
    """-> {output: max over the seeds of the oracle's distance from the yardstick}; fp32 inputs: k alone, and under F32_STAGE the distance
    of the fp32-stage restatement's k from the yardstick -- the ledger's allowance for a route that hands fp32 arrays between launches"""
    seeds = range(DV.SEEDS) if seeds is None else seeds
    draws, got, stage = [], [], []
    for seed in seeds:
        X, Y, gamma, X1, X2, sigma = DV.inputs(settings, sh, seed)
        draws.append((X, X1, X2, Y, sigma))
        got.append(oracle_kgrad(kind, sigma, X, Y, gamma, sh["d"]))
        if sh["f32"]:
            stage.append(f32_stage_k(kind, sigma, X, Y, gamma, sh))
    want = DV.stacked_want(kind, draws, sh["d"])
    names = DV.outputs_of(sh)
    per = [DV.errors(g, tuple(w[n] for w in want), names) for n, g in enumerate(got)]
    out = {name: max(e[name] for e in per) for name in names}
    if sh["f32"]:
        out[DV.F32_STAGE] = max(DV.error(s, want[0][n]) for n, s in enumerate(stage))
    return out


def main():
    out = {}
    for key, entry in sorted(DV.golden_entries().items()):
        out[key] = measure(*entry)
        print("%-48s %s" % (key, "  ".join("%s %.2e" % (n, v) for n, v in out[key].items())), flush=True)
    out["_provenance"] = ("distance of the CPU oracle's kgrad from the long-double yardstick, max |got - want| / max |want| over the (A, B) "
                          "matrix, maximum over %d seeds; tests/golden/measure_deriv_value_regimes.py" % DV.SEEDS)
    with open(PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
