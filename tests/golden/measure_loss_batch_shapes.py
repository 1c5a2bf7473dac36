#!/usr/bin/env python3
"""The distance of the CPU oracle from the blockwise long-double yardstick (tests/loss_batch_shapes.py) on every case of the
batch-shape tables -- the distance the REFERENCE's own arithmetic has from the truth there.  The GPU tests' bound is base + 4 x this;
the script imports the oracle and the yardstick, never the product's kernels (the static kernels restate the reference's two formulas
in torch: tests/golden/measure_value_regimes.py).  The oracle's side is the reference's composition: K(X, [X; Y]) and K(Y, Y) by
gram_forward, the loss by the reference's formula, dL/dX by gram_grad_weighted under the loss's weights with the 2x rule for K_XX;
compute_distance: the diagonals, the first argument only.  Measured like the instance ledger compares: values per element relative to
max(|want|, 1), gradients per path relative to the path's largest entry.

    python tests/golden/measure_loss_batch_shapes.py        # rewrites tests/golden/loss_batch_shapes.json
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE]

import loss_batch_shapes as S  # noqa: E402
import value_regimes as V  # noqa: E402
from measure_value_regimes import static_kernel  # noqa: E402
from oracle import oracle as O  # noqa: E402

PATH = os.path.join(HERE, "loss_batch_shapes.json")


def oracle_loss(kind, sigma, X, Y, d, with_yy, grad=True):
    """-> (loss, dL/dX or None, per-pair values in the one-launch route's order) from the oracle"""
    k = static_kernel(kind, sigma)
    nt = min(16, O.max_threads())
    A, B = X.shape[0], Y.shape[0]
    Xt, Yt = torch.from_numpy(X), torch.from_numpy(Y)
    Zt = torch.cat([Xt, Yt])
    K = O.gram_forward(Xt, Zt, k, d, nthreads=nt)
    Kxx, Kxy = K[:, :A], K[:, A:]
    value = (Kxx.sum() - np.trace(Kxx)) / (A * (A - 1.0)) - 2.0 * Kxy.mean()
    pairs = K.reshape(-1)
    if with_yy:
        Kyy = O.gram_forward(Yt, Yt, k, d, nthreads=nt)
        if B > 1:
            value = value + (Kyy.sum() - np.trace(Kyy)) / (B * (B - 1.0))
        pairs = np.concatenate([pairs, Kyy[S.triangle_pairs(B)]])
    g = None
    if grad:
        w = np.empty((A, A + B))
        w[:, :A] = 2.0 / (A * (A - 1.0))
        w[np.arange(A), np.arange(A)] = 0.0
        w[:, A:] = -2.0 / (A * B)
        g = O.gram_grad_weighted(Xt, Zt, w, k, d, nthreads=nt)
    return value, g, pairs


def oracle_distance(kind, sigma, X, Y, d):
    k = static_kernel(kind, sigma)
    n = X.shape[0]
    Xt, Yt = torch.from_numpy(X), torch.from_numpy(Y)
    Kxx, Kxy, Kyy = (np.diagonal(O.gram_forward(a, b, k, d)) for a, b in ((Xt, Xt), (Xt, Yt), (Yt, Yt)))
    g = O.gram_grad_weighted(Xt, Xt, np.eye(n) / n, k, d) + O.gram_grad_weighted(Xt, Yt, -2.0 * np.eye(n) / n, k, d)
    return Kxx.mean() + Kyy.mean() - 2.0 * Kxy.mean(), g


def measure(c, kind):
    """{"value": the scalar (or, for the per-pair tables, the worst entry), "grad", "loss": the scalar of a per-pair case, "max_k"}"""
    X, Y = S.inputs(c)
    sigma, wr, d = S.sigma_of(kind), c["wrapper"], c["d"]
    value, grad, pairs = S.want(c, kind)
    if wr == "distance":
        v, g = oracle_distance(kind, sigma, X, Y, d)
        return {"value": V.value_error(v, value), "grad": V.grad_error(g, grad)}
    if wr == "sym":
        K = O.gram_forward(torch.from_numpy(X), torch.from_numpy(X), static_kernel(kind, sigma), d, nthreads=min(16, O.max_threads()))
        return {"value": V.value_error(K, pairs), "max_k": float(np.max(np.abs(pairs)))}
    if wr in ("pairs", "pairs_yy"):
        v, _, p = oracle_loss(kind, sigma, X, Y, d, wr == "pairs_yy", grad=False)
        return {"value": V.value_error(p, pairs), "loss": V.value_error(v, value), "max_k": float(np.max(np.abs(pairs)))}
    v, g, p = oracle_loss(kind, sigma, X, Y, d, S.WITH_YY[wr])
    return {"value": V.value_error(v, value), "grad": V.grad_error(g, grad), "max_k": float(np.max(np.abs(pairs)))}


def main():
    out = {}
    for key, (c, kind) in sorted(S.golden_entries().items()):
        out[key] = measure(c, kind)
        print("%-40s %s" % (key, "  ".join("%s %.2e" % kv for kv in sorted(out[key].items()))), flush=True)
    out["_provenance"] = ("distance of the CPU oracle (the reference's composition) from the blockwise long-double yardstick, in the instance "
                          "ledger's measures; max_k: the largest |K| of the case; tests/golden/measure_loss_batch_shapes.py")
    with open(PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
