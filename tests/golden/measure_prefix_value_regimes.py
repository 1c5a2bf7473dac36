#!/usr/bin/env python3
"""The distance of the REFERENCE's arithmetic from the long-double yardstick on every case of tests/prefix_value_regimes.py -- the r of
the GPU test's bound base + 4 r.

Values: the static kernels as measure_value_regimes.py restates them (_Linear / _RBF: nodes from the POINTS, in double), the oracle's
increments and solve_coarse(..., want_grid=True); measured over ALL coarse nodes of every grid (value_regimes.value_error: per element
over max(|want|, 1)), not over the last node alone.  The two loss rows: the same reductions on the reference's grids.
Gradients: tests/exact_gradient_reference.py's exact_adjoint on the increments of every pair's TRUNCATED paths, autograd's chain rule
through the restated static kernel; measured per path (value_regimes.grad_error), for X and for Y.
`offset` entries hold the maximum over value_regimes.OFFSET_SEEDS seeds, all others seed 0.  The script imports the oracle, the
restatements and the yardstick, never the product's kernels.

    python tests/golden/measure_prefix_value_regimes.py        # rewrites tests/golden/prefix_value_regimes.json
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import exact_gradient_reference as R  # noqa: E402
import prefix_value_regimes as PV  # noqa: E402
import value_regimes as V  # noqa: E402
from oracle import oracle as O  # noqa: E402

PATH = os.path.join(HERE, "prefix_value_regimes.json")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


static_kernel = _load("measure_value_regimes").static_kernel


def reference_grid(kind, sigma, X, Y, d, gram):
    """every coarse node by the reference's arithmetic in fp64: (A,B,M,N) Gram, (A,M,N) paired"""
    G = static_kernel(kind, sigma).Gram_matrix(torch.from_numpy(np.array(X)), torch.from_numpy(np.array(Y))).numpy()
    if not gram:
        G = G[np.arange(X.shape[0]), np.arange(X.shape[0])]
    _, grid = O.solve_coarse(O.increments(np.ascontiguousarray(G)), d, False, want_grid=True)
    r = 1 << d
    return grid[..., ::r, ::r]


def reference_ragged_grads(kind, sigma, X, Y, lx, ly, d, w, pairs=None):
    """prefix_value_regimes.ragged_grads_ld's sums by the reference's arithmetic in fp64"""
    k = static_kernel(kind, sigma)
    A, B = X.shape[0], Y.shape[0]
    K, gX, gY = np.ones((A, B)), np.zeros(X.shape), np.zeros(Y.shape)
    for a, b in (pairs if pairs is not None else [(a, b) for a in range(A) for b in range(B)]):
        m, n = lx[a], ly[b]
        if m < 2 or n < 2:
            continue
        x, y = torch.from_numpy(np.array(X[a, :m])).requires_grad_(True), torch.from_numpy(np.array(Y[b, :n])).requires_grad_(True)
        G = k.Gram_matrix(x[None], y[None])[0, 0]
        inc = G[1:, 1:] + G[:-1, :-1] - G[1:, :-1] - G[:-1, 1:]
        K[a, b], W = R.exact_adjoint(inc.detach().numpy(), d)
        gx, gy = torch.autograd.grad(inc, (x, y), torch.from_numpy(W * float(w[a, b])))
        gX[a, :m] += gx.numpy()
        gY[b, :n] += gy.numpy()
    return K, gX, gY


def reference_of(c, seed=0):
    """what prefix_value_regimes.want_of returns, by the reference's arithmetic"""
    row, kind, fam, lab, st = c
    X, Y, w, sigma = PV.inputs(c, seed)
    d, op = row["shape"]["d"], row["op"]
    if op in ("grid", "grid_out"):
        return {"value": reference_grid(kind, sigma, X, Y, d, row["gram"])}
    if op in ("mmd_prefixes", "mmd_ragged"):
        grids = tuple(reference_grid(kind, sigma, P, Q, d, True) for P, Q in ((X, X), (Y, Y), (X, Y)))
        if op == "mmd_prefixes":
            return {"value": PV.mmd_prefixes_from(*grids)}
        return {"value": np.asarray(PV.mmd_ragged_from(*grids, *PV.lens_of(row)))}
    lx, ly = PV.lens_of(row)
    value, gx, gy = PV.assemble(op, row["gram"], X, Y, lx, ly, w,
                                lambda P, Q, lp, lq, ww, pairs: reference_ragged_grads(kind, sigma, P, Q, lp, lq, d, ww, pairs))
    return {"value": np.asarray(value), "grad_x": gx, "grad_y": gy}


def distance(c, seed=0):
    ref, want = reference_of(c, seed), (PV.case_want(c) if seed == 0 else PV.want_of(c, seed))
    return {name: PV.error(name, ref[name], want[name]) for name in PV.outputs_of(c[0])}


def measure(c):
    ds = [distance(c, seed) for seed in (range(V.OFFSET_SEEDS) if c[2] == "offset" else (0,))]
    return {name: max(x[name] for x in ds) for name in ds[0]}


def main():
    out = {}
    for key, c in sorted(PV.golden_entries().items()):
        out[key] = measure(c)
        print("%-72s %s" % (key, "  ".join("%s %.2e" % kv for kv in sorted(out[key].items()))), flush=True)
    out["_provenance"] = ("distance of the reference's arithmetic (restated static kernels, oracle solver with its grid, exact_gradient_reference) "
                          "from the long-double yardstick, maximum over all nodes / per path; offset: maximum over %d seeds; "
                          "tests/golden/measure_prefix_value_regimes.py" % V.OFFSET_SEEDS)
    with open(PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
