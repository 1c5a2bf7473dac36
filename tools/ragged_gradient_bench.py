#!/usr/bin/env python3
"""Call times of a Gram matrix's exact backward on a batch of paths of unequal length (forward + backward, host clock around a device
synchronise) on one GPU, under SigKernel(..., exact_gradient=True):

  padded   compute_Gram(X, Y).sum().backward()                       -- every pair swept over the padded grid: what a masked loss on
                                                                        the padded batch costs, the only such gradient before the
                                                                        ragged mode (it runs on older builds too)
  ragged   compute_Gram_ragged(X, Y, len_x, len_y).sum().backward()  -- every pair swept over its own sub-grid
                                                                        (sk_solve_adj_* with SK_FLAG_DISCRETE | SK_FLAG_RAGGED)

at the two shapes of profiles/exact_gradient.txt, lengths uniform in [2, M] (seeded).  The routes alternate inside every round; medians
over the rounds, with the ratio of swept to padded coarse cells beside them.  Then the adjoint launch alone (solve_adj on the same
increments, with and without the table): what of the saving is the sweep's and what the static-kernel stages and the host keep.

--base NAME imports the package from ab_base/NAME (tools/ab.py's layout: an older build, for the padded figure on the same box);
a build without the ragged mode prints that and times the padded route alone."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def timed(fn, rounds, warmup=2):
    """{name: [seconds]} of the callables in `fn`, alternating inside every round"""
    times = {k: [] for k in fn}
    for rnd in range(rounds + warmup):
        for key, f in fn.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            if rnd >= warmup:
                times[key].append(time.perf_counter() - t0)
    return times


def report(times, key):
    v = times[key]
    return "median %9.3f ms  (min %9.3f, max %9.3f, %d rounds)" % (1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v), len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="scale the batch sizes (a rehearsal at a toy size)")
    ap.add_argument("--base", default=None, help="import the package from ab_base/NAME instead of the working tree")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "ab_base", args.base) if args.base else ROOT)
    import sigkernel_amd
    from sigkernel_amd import _lib
    has_ragged = hasattr(_lib, "FLAG_RAGGED")
    print("# package: %s%s" % (args.base or "working tree", "" if has_ragged else "  (no ragged gradients in this build: padded route only)"))
    shapes = [("128 x 128 pairs, 64 points, dim 3, RBF, dyadic 1", 128, 64, 3, sigkernel_amd.RBFKernel(1.0), 1),
              ("256 x 256 pairs, 64 points, dim 8, Linear, dyadic 0", 256, 64, 8, sigkernel_amd.LinearKernel(), 0)]
    for name, A, M, D, kernel, d in shapes:
        A = max(2, int(A * args.scale))
        gen = torch.Generator().manual_seed(A + D)
        X = (torch.cumsum(torch.randn(A, M, D, generator=gen, dtype=torch.float64), 1) / (M * D) ** 0.5).to(DEV)
        Y = (torch.cumsum(torch.randn(A, M, D, generator=gen, dtype=torch.float64), 1) / (M * D) ** 0.5).to(DEV)
        lx = torch.randint(2, M + 1, (A,), generator=gen)
        ly = torch.randint(2, M + 1, (A,), generator=gen)
        share = float((lx - 1).sum() * (ly - 1).sum()) / (A * A * (M - 1) ** 2)
        # two more pieces of arithmetic to read the times by: a wave takes an anti-diagonal of up to 64 fine cells in one pass, so a pair
        # costs by its diagonals (mc + nc) rather than its cells where the grid is that narrow; and pair p runs on block p mod 1024, so
        # the launch ends with the block whose pairs hold the most diagonals
        diag = (lx - 1)[:, None] + (ly - 1)[None, :]
        blocks = min(A * A, 1024)
        per_block = torch.zeros(blocks, dtype=torch.int64).index_add_(0, torch.arange(A * A) % blocks, diag.reshape(-1))
        diag_share = float(diag.sum()) / (A * A * 2 * (M - 1))
        tail_share = float(per_block.max()) * blocks / (A * A * 2 * (M - 1))
        exact = sigkernel_amd.SigKernel(kernel, d, exact_gradient=True)
        grads = {}

        def padded():
            x = X.clone().requires_grad_(True)
            exact.compute_Gram(x, Y).sum().backward()
            grads["padded"] = x.grad

        def ragged():
            x = X.clone().requires_grad_(True)
            exact.compute_Gram_ragged(x, Y, lx, ly).sum().backward()
            grads["ragged"] = x.grad

        routes = {"padded": padded, "ragged": ragged} if has_ragged else {"padded": padded}
        times = timed(routes, args.rounds)
        print(name)
        print("  lengths uniform in [2, %d]: swept / padded coarse cells = %.3f   anti-diagonals = %.3f   anti-diagonals of the fullest of "
              "%d blocks = %.3f" % (M, share, diag_share, blocks, tail_share))
        for k in routes:
            print("  %-7s %s   |X.grad| = %.6e" % (k, report(times, k), float(grads[k].norm())))
        if not has_ragged:
            sys.stdout.flush()
            continue
        med = {k: statistics.median(v) for k, v in times.items()}
        print("  ragged / padded = %.3f" % (med["ragged"] / med["padded"]))
        # the adjoint launch alone, on the increments of the padded batch
        be = _lib.get_backend()
        kind, param = (1, float(kernel.sigma)) if isinstance(kernel, sigkernel_amd.RBFKernel) else (0, 1.0)
        inc = be.static_increments(kind, param, X, Y, True)
        if inc is None:
            inc = be.increments(kernel.Gram_matrix(X, Y).contiguous())
        cells = torch.stack(((lx - 1)[:, None].expand(A, A), (ly - 1)[None, :].expand(A, A)), dim=-1).to(torch.int32).contiguous().to(DEV)
        full = torch.full_like(cells, M - 1)
        launch = timed({"padded": lambda: be.solve_adj(inc, d, discrete=True), "ragged": lambda: be.solve_adj(inc, d, discrete=True, cells=cells),
                        "table, full lengths": lambda: be.solve_adj(inc, d, discrete=True, cells=full)}, args.rounds)
        print("  the adjoint launch alone (solve_adj on the padded batch's increments):")
        for k in launch:
            print("    %-20s %s" % (k, report(launch, k)))
        lm = {k: statistics.median(v) for k, v in launch.items()}
        print("    ragged / padded = %.3f  (cells: %.3f)" % (lm["ragged"] / lm["padded"], share), flush=True)


if __name__ == "__main__":
    main()
