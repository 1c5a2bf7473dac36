#!/usr/bin/env python3
"""Call times of a loss over time and its gradient (forward + backward, host clock around a device synchronise, X and Y require grad) on
one GPU, under SigKernel(..., exact_gradient=True), at the two shapes of profiles/exact_gradient.txt:

  (a) prefixes     compute_mmd_prefixes(X, Y).sum().backward()          -- sum_t MMD^2(X[:, :t+1], Y[:, :t+1]): three nodes="diagonal"
                                                                           forward sweeps, three reverse sweeps with a source per node
                                                                           (sk_solve_adj_* with SK_FLAG_DISCRETE | SK_FLAG_SOURCES)
  (b) floor        compute_mmd(X, Y).backward()                         -- the last term alone: the same number of sweeps
  (c) composition  sum(compute_mmd(X[:, :t+1], Y[:, :t+1]) for t ...).backward()
                                                                        -- the only way to (a)'s gradient before the prefix gradients
                                                                           (it runs on older builds too): one backward per t, all
                                                                           t = 1..T-1.  With --subset LIST only the listed t are
                                                                           timed and the figure is extrapolated by the fine cells
                                                                           swept, sum t^2 over all t against the subset's

The routes alternate inside every round; medians over the rounds.  Then the adjoint launch alone (solve_adj on the same increments,
without sources and with them), and the unchanged calls: compute_Gram(...).sum().backward() and compute_Gram_ragged(...).sum().backward().

--base NAME imports the package from ab_base/NAME (tools/ab.py's layout: an older build, for (b), (c) and the unchanged calls on the
same box); a build without the prefix gradients prints that and skips (a)."""
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
    ap.add_argument("--subset", default=None, help="time the composition on these t alone (comma-separated; points: t + 1) and extrapolate")
    args = ap.parse_args()
    args.full = args.subset is None
    sys.path.insert(0, os.path.join(ROOT, "ab_base", args.base) if args.base else ROOT)
    import sigkernel_amd
    from sigkernel_amd import _lib
    has_prefix = hasattr(_lib, "FLAG_SOURCES")
    print("# package: %s%s" % (args.base or "working tree", "" if has_prefix else "  (no prefix gradients in this build: (a) skipped)"))
    shapes = [("128 x 128 pairs, 64 points, dim 3, RBF, dyadic 1", 128, 64, 3, sigkernel_amd.RBFKernel(1.0), 1),
              ("256 x 256 pairs, 64 points, dim 8, Linear, dyadic 0", 256, 64, 8, sigkernel_amd.LinearKernel(), 0)]
    for name, A, M, D, kernel, d in shapes:
        A = max(2, int(A * args.scale))
        gen = torch.Generator().manual_seed(A + D)
        X = (torch.cumsum(torch.randn(A, M, D, generator=gen, dtype=torch.float64), 1) / (M * D) ** 0.5).to(DEV)
        Y = (torch.cumsum(torch.randn(A, M, D, generator=gen, dtype=torch.float64), 1) / (M * D) ** 0.5).to(DEV)
        ts = list(range(1, M)) if args.full else [int(t) for t in args.subset.split(",") if 1 <= int(t) < M]      # (t = 0: the constant 0)
        factor = sum(t * t for t in range(1, M)) / float(sum(t * t for t in ts))
        exact = sigkernel_amd.SigKernel(kernel, d, exact_gradient=True)
        grads = {}

        def leaves():
            return X.clone().requires_grad_(True), Y.clone().requires_grad_(True)

        def prefixes():
            x, y = leaves()
            exact.compute_mmd_prefixes(x, y).sum().backward()
            grads["(a) prefixes"] = (x.grad, y.grad)

        def floor():
            x, y = leaves()
            exact.compute_mmd(x, y).backward()
            grads["(b) floor"] = (x.grad, y.grad)

        def composition():
            x, y = leaves()
            sum(exact.compute_mmd(x[:, :t + 1], y[:, :t + 1]) for t in ts).backward()
            grads["(c) composition"] = (x.grad, y.grad)

        routes = {"(a) prefixes": prefixes, "(b) floor": floor, "(c) composition": composition}
        if not has_prefix:
            del routes["(a) prefixes"]
        times = timed(routes, args.rounds)
        print(name)
        for k in routes:
            print("  %-16s %s   |X.grad| = %.6e  |Y.grad| = %.6e" % (k, report(times, k), float(grads[k][0].norm()), float(grads[k][1].norm())))
        med = {k: statistics.median(v) for k, v in times.items()}
        full_c = med["(c) composition"] * factor
        print("  (c) over t = %s%s" % ("1..%d" % (M - 1) if args.full else ",".join(str(t) for t in ts),
                                        "" if args.full else ": x %.3f (fine cells of all t over the subset's) = %.1f ms EXTRAPOLATED" % (factor, 1e3 * full_c)))
        if has_prefix:
            print("  (a) / (b) = %.3f   (c) / (a) = %.1f%s" % (med["(a) prefixes"] / med["(b) floor"], full_c / med["(a) prefixes"],
                                                            "" if args.full else "  (extrapolated)"))
            if args.full:      # the very sum: the two gradients agree
                ga, gc = grads["(a) prefixes"], grads["(c) composition"]
                print("  max |(a) - (c)| / max |(c)|: X.grad %.2e  Y.grad %.2e" % tuple(float((p - q).abs().max() / q.abs().max()) for p, q in zip(ga, gc)))
            # what (a) pays over (b), piece by piece: the forward sweeps, and the adjoint launch with and without the sources
            with torch.no_grad():
                fwd = timed({"three nodes=\"diagonal\" forwards": lambda: exact.compute_mmd_prefixes(X, Y),
                             "three plain forwards": lambda: exact.compute_mmd(X, Y)}, args.rounds)
            print("  the forward alone (no gradient pending):")
            for k in fwd:
                print("    %-34s %s" % (k, report(fwd, k)))
            be = _lib.get_backend()
            kind, param = (1, float(kernel.sigma)) if isinstance(kernel, sigkernel_amd.RBFKernel) else (0, 1.0)
            inc = be.static_increments(kind, param, X, Y, True)
            if inc is None:
                inc = be.increments(kernel.Gram_matrix(X, Y).contiguous())
            go = torch.randn(A, A, M, generator=gen, dtype=torch.float64).to(DEV)
            from sigkernel_amd.sigkernel import _prefix_sources
            S = _prefix_sources(go, "diagonal", M - 1, M - 1)
            launch = timed({"plain": lambda: be.solve_adj(inc, d, discrete=True), "sources": lambda: be.solve_adj(inc, d, discrete=True, sources=S),
                            "scatter + sources": lambda: be.solve_adj(inc, d, discrete=True, sources=_prefix_sources(go, "diagonal", M - 1, M - 1))},
                           args.rounds)
            print("  the adjoint launch alone (solve_adj on X x Y's increments; sources: the copy into W included; scatter: building them from grad_output too):")
            for k in launch:
                print("    %-20s %s" % (k, report(launch, k)))
        # the calls this change must not move
        lx = torch.randint(2, M + 1, (A,), generator=gen)
        ly = torch.randint(2, M + 1, (A,), generator=gen)

        def gram():
            x = X.clone().requires_grad_(True)
            exact.compute_Gram(x, Y).sum().backward()

        def ragged():
            x = X.clone().requires_grad_(True)
            exact.compute_Gram_ragged(x, Y, lx, ly).sum().backward()

        same = timed({"compute_Gram": gram, "compute_Gram_ragged": ragged}, args.rounds)
        print("  unchanged calls (.sum().backward(), X requires grad):")
        for k in same:
            print("    %-20s %s" % (k, report(same, k)))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
