#!/usr/bin/env python3
"""Timing of TruncatedSigKernel with an RBF static kernel (GPU box): the points mode of k_trunc_sig beside the linear mode of the
same build and the torch restatement of the same lift.

  python tools/time_truncated_static.py [--repeats 7] [--warmup 2] [--torch-rows 2] [--rbf-sigma 1.0]
      compute_Gram(X, Y) under no_grad at the shapes of profiles/truncated_levels.txt, paths of `points` points, event-timed around the
      public call (staging and allocation included), interleaved, medians:
        (a) static_kernel=RBFKernel(s): one k_trunc_sig launch in its points mode;
        (b) static_kernel=None: the levels mode on the steps, k_trunc_sig<1, 2> of the same build -- the SAME PATHS, so its grid has
            points - 1 rows and columns where (a) sweeps points x points (127 against 128: under 2 % of the nodes);
        (c) the torch restatement of (a) on the same device (RBFKernel.Gram_matrix, its second difference, the recursion): it holds
            nine arrays of rows x B x M x N, so it is timed on the first --torch-rows rows of X -- the default 1 GiB workspace makes a tile
            of one row at these shapes anyway -- and scaled to the batch.
      The last column is the run's own accuracy check: (a) against (c) on those rows, per level in units of the level's largest value.
The A/B of the existing launches against another checkout is tools/time_truncated_adjoint.py (--forward --tree DIR, and its default
mode for the adjoint)."""
import os, sys
import numpy as np, torch

arg = lambda name, d: type(d)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else d
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sigkernel_amd
from sigkernel_amd import _lib
from sigkernel_amd.truncated import _lifted_gram, _truncated_levels_torch

# name, A = B, points, dim, levels
SHAPES = [("512^2 x 128, dim 8, L4", 512, 128, 8, 4), ("512^2 x 128, dim 8, L8", 512, 128, 8, 8), ("2048^2 x 64, dim 4, L6", 2048, 64, 4, 6)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main(repeats, warmup, trows, s):
    print("# TruncatedSigKernel.compute_Gram(X, Y), no gradient (ms, median of %d interleaved repeats after %d warm-ups; torch route on %d rows "
          "of X, scaled); RBFKernel(%g)" % (repeats, warmup, trows, s))
    print("# %s; %s" % (torch.cuda.get_device_name(0), _lib.load().sk_build_info().decode()))
    print("shape\t(a) rbf points mode\tmin..max\t(b) linear\tmin..max\ta/b\t(c) torch rbf (scaled)\tc/a\tworst level |a - c| / max")
    g = torch.Generator().manual_seed(0)
    for name, A, P, D, L in SHAPES:
        mk = lambda n: torch.cumsum(0.3 * torch.randn(n, P, D, generator=g, dtype=torch.float64) / np.sqrt(D), 1).cuda()
        X, Y = mk(A), mk(A)
        rbf = sigkernel_amd.TruncatedSigKernel(L, static_kernel=sigkernel_amd.RBFKernel(s))
        lin = sigkernel_amd.TruncatedSigKernel(L)
        with torch.no_grad():
            fns = (("rbf", lambda: rbf._levels(X, Y, False, False)), ("lin", lambda: lin._levels(X, Y, False, False)),
                   ("torch", lambda: _truncated_levels_torch(X[:trows], Y, L, 1, False, None, _lifted_gram(rbf.static_kernel))))
            t, out = {k: [] for k, _ in fns}, {}
            for i in range(warmup + repeats):
                for k, fn in fns:
                    ms, out[k] = timed(fn)
                    if i >= warmup:
                        t[k].append(ms)
        med = {k: float(np.median(v)) for k, v in t.items()}
        err = max(float((out["rbf"][m, :trows] - out["torch"][m]).abs().max() / out["torch"][m].abs().max()) for m in range(1, L + 1))
        tt = med["torch"] * A / trows
        print("%s\t%.3f\t%.3f..%.3f\t%.3f\t%.3f..%.3f\t%.2f\t%.1f\t%.1f\t%.2g" % (
            name, med["rbf"], min(t["rbf"]), max(t["rbf"]), med["lin"], min(t["lin"]), max(t["lin"]), med["rbf"] / med["lin"], tt,
            tt / med["rbf"], err), flush=True)
        del X, Y, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main(arg("--repeats", 7), arg("--warmup", 2), arg("--torch-rows", 2), arg("--rbf-sigma", 1.0))
