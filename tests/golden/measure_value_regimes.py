#!/usr/bin/env python3
"""The distance of the CPU oracle from the long-double yardstick (tests/value_regimes.py) on every (family, parameter, static kernel,
shape) of the value-regime case table -- the distance the REFERENCE's own arithmetic (|x|^2 + |y|^2 - 2 <x, y> and <x, y> at the
nodes, in double) has from the truth there.  The GPU test's bound is base + 4 x this; the script imports the oracle and the
yardstick, never the product's kernels (the static kernels below restate the reference's two formulas in torch, as the oracle's
callers always hand them in).  Measured like the instance ledger compares: values per element relative to max(|want|, 1), gradients
per path relative to the path's largest entry.  `offset` entries hold the maximum over value_regimes.OFFSET_SEEDS seeds (the digits
lost to an offset vary by a factor 3 from draw to draw), all others seed 0.

    python tests/golden/measure_value_regimes.py        # rewrites tests/golden/value_regimes.json
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import value_regimes as V  # noqa: E402
from oracle import oracle as O  # noqa: E402

PATH = os.path.join(HERE, "value_regimes.json")


class _Linear:
    def Gram_matrix(self, X, Y):      # static_kernels.py:33
        return torch.einsum("ipk,jqk->ijpq", X, Y)


class _RBF:
    def __init__(self, sigma):
        self.sigma = sigma

    def Gram_matrix(self, X, Y):      # static_kernels.py:58-73
        A, B, M, N = X.shape[0], Y.shape[0], X.shape[1], Y.shape[1]
        Xs, Ys = torch.sum(X ** 2, dim=2), torch.sum(Y ** 2, dim=2)
        dist = -2. * torch.einsum("ipk,jqk->ijpq", X, Y)
        dist += torch.reshape(Xs, (A, 1, M, 1)) + torch.reshape(Ys, (1, B, 1, N))
        return torch.exp(-dist / self.sigma)


def static_kernel(kind, sigma):
    return _Linear() if kind == "linear" else _RBF(sigma)


def oracle_distance(kind, X, Y, w, sigma, d):
    """-> {"value", "grad"}: the oracle's Gram matrix and weighted gradient against the yardstick's"""
    k = static_kernel(kind, sigma)
    Xt, Yt = torch.from_numpy(X), torch.from_numpy(Y)
    K, g = V.gram_ld(kind, sigma, X, Y, d, w)
    return {"value": V.value_error(O.gram_forward(Xt, Yt, k, d), K), "grad": V.grad_error(O.gram_grad_weighted(Xt, Yt, w, k, d), g)}


def measure(fam, lab, kind, sh, settings):
    seeds = range(V.OFFSET_SEEDS) if fam == "offset" else (0,)
    ds = [oracle_distance(kind, *V.inputs(settings, sh, seed)[:3], settings.get("sigma"), sh["d"]) for seed in seeds]
    return {name: max(x[name] for x in ds) for name in ("value", "grad")}


def main():
    out = {}
    for key, entry in sorted(V.golden_entries().items()):
        out[key] = measure(*entry)
        print("%-60s value %.2e grad %.2e" % (key, out[key]["value"], out[key]["grad"]), flush=True)
    out["_provenance"] = ("distance of the CPU oracle from the long-double yardstick, in the instance ledger's measures; offset: maximum "
                          "over %d seeds; tests/golden/measure_value_regimes.py" % V.OFFSET_SEEDS)
    with open(PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
