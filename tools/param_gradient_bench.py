#!/usr/bin/env python3
"""What a learnable RBFKernel.sigma costs under SigKernel(..., exact_gradient=True): call times of compute_Gram(X, Y).sum().backward()
(forward + backward, host clock around a device synchronise, X requires grad) on one GPU, at the two shapes of
profiles/exact_gradient.txt and at 256 x 256 pairs of 64 points in 16 and 20 dims (RBF, dyadic 1):

  (a) float      sigma a float                      -- the unchanged call; with --base NAME also on the older build under ab_base/NAME
                                                       (tools/ab.py's layout), the two builds alternating process by process, and the
                                                       base against itself: the spread a difference has to exceed to mean anything
  (b) sigma      sigma a tensor that requires grad  -- dX and dsigma from ONE k_static_rbf_adj launch in its parameter mode (at 17..32
                                                       dims that launch replaces the float call's k_static_rbf_adj_tiled)
  (c) generic    (b) with the one-launch method taken away: torch Gram_matrix + sk_increments_adjoint + one vector-Jacobian product
                 through the static kernel for (X, sigma) -- what a backend without the method runs, and what RBF beyond 32 dims runs

Within a process the routes alternate inside every round (two warm-up rounds, medians over the rounds); with --base every build gets
`--rounds` processes, alternating, and the figure of a build is the median of its processes' medians."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SHAPES = [("128 x 128 pairs, 64 points, dim 3, RBF, dyadic 1", 128, 64, 3, "rbf", 1),
          ("256 x 256 pairs, 64 points, dim 8, Linear, dyadic 0", 256, 64, 8, "linear", 0),
          ("256 x 256 pairs, 64 points, dim 16, RBF, dyadic 1", 256, 64, 16, "rbf", 1),
          ("256 x 256 pairs, 64 points, dim 20, RBF, dyadic 1", 256, 64, 20, "rbf", 1)]


def one(args):
    """one process, one build: 'T <shape index> <route> <median seconds>' lines"""
    sys.path.insert(0, os.path.join(ROOT, "ab_base", args.one) if args.one != "new" else ROOT)
    import torch
    import sigkernel_amd
    from sigkernel_amd import _lib
    has_mode = hasattr(_lib.HipBackend, "static_adjoint_param")
    for i, (name, A, M, D, kind, d) in enumerate(SHAPES):
        A = max(2, int(A * args.scale))
        gen = torch.Generator().manual_seed(A + D)
        X = (torch.cumsum(torch.randn(A, M, D, generator=gen, dtype=torch.float64), 1) / (M * D) ** 0.5).to(DEV)
        Y = (torch.cumsum(torch.randn(A, M, D, generator=gen, dtype=torch.float64), 1) / (M * D) ** 0.5).to(DEV)
        sigma = torch.tensor(1.0, dtype=torch.float64, device=DEV, requires_grad=True)
        kernels = {"float": sigkernel_amd.RBFKernel(1.0) if kind == "rbf" else sigkernel_amd.LinearKernel()}
        if kind == "rbf" and has_mode and not args.float_only:
            kernels["sigma"] = kernels["generic"] = sigkernel_amd.RBFKernel(sigma)
        sks = {k: sigkernel_amd.SigKernel(v, d, exact_gradient=True) for k, v in kernels.items()}
        method = _lib.HipBackend.static_adjoint_param if has_mode else None
        times, grads = {k: [] for k in sks}, {}
        for rnd in range(args.calls + 2):          # two warm-up rounds
            for key, sk in sks.items():
                if key == "generic":
                    del _lib.HipBackend.static_adjoint_param
                try:
                    x = X.clone().requires_grad_(True)
                    sigma.grad = None
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    sk.compute_Gram(x, Y).sum().backward()
                    torch.cuda.synchronize()
                    if rnd >= 2:
                        times[key].append(time.perf_counter() - t0)
                    grads[key] = (x.grad, None if sigma.grad is None else float(sigma.grad))
                finally:
                    if key == "generic":
                        _lib.HipBackend.static_adjoint_param = method
        for key in sks:
            print("T %d %s %.9f" % (i, key, statistics.median(times[key])), flush=True)
        if "sigma" in grads:
            gx, gs = grads["sigma"]
            print("C %d sigma.grad %.15g (generic branch %.15g); X.grad against the float call's: max |diff| / max = %.2e (generic %.2e)"
                  % (i, gs, grads["generic"][1], float((gx - grads["float"][0]).abs().max() / grads["float"][0].abs().max()),
                     float((grads["generic"][0] - grads["float"][0]).abs().max() / grads["float"][0].abs().max())), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="processes per build")
    ap.add_argument("--calls", type=int, default=5, help="timed calls per route and process")
    ap.add_argument("--scale", type=float, default=1.0, help="scale the batch sizes (a rehearsal at a toy size)")
    ap.add_argument("--base", default=None, help="an older build under ab_base/NAME to alternate with (the unchanged calls)")
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--float-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        return one(args)
    # base, base again (its own spread), new -- process by process
    builds = ([("base", args.base, True), ("base'", args.base, True)] if args.base else []) + [("new", "new", False)]
    res, checks = {}, {}
    for rnd in range(args.rounds):
        for label, which, float_only in builds:
            cmd = [sys.executable, os.path.abspath(__file__), "--one", which, "--calls", str(args.calls), "--scale", str(args.scale)]
            out = subprocess.run(cmd + (["--float-only"] if float_only else []), capture_output=True, text=True, timeout=900)
            if out.returncode:
                print(out.stdout, out.stderr)
                sys.exit("%s failed with status %d: nothing more is started" % (label, out.returncode))
            print("# round %d, %s: done" % (rnd, label), file=sys.stderr, flush=True)
            for ln in out.stdout.splitlines():
                p = ln.split(" ", 3)
                if p[0] == "T":
                    res.setdefault((int(p[1]), label, p[2]), []).append(float(p[3]))
                elif p[0] == "C":
                    checks[int(p[1])] = ln[2:].split(" ", 1)[1]

    def fig(i, label, route):
        v = res.get((i, label, route))
        return None if not v else (statistics.median(v), min(v), max(v))

    def line(what, f):
        return "  %-22s median %9.3f ms  (min %9.3f, max %9.3f over %d processes)" % (what, 1e3 * f[0], 1e3 * f[1], 1e3 * f[2], args.rounds)
    for i, (name, *_rest) in enumerate(SHAPES):
        print(name)
        new = fig(i, "new", "float")
        if args.base:
            b0, b1 = fig(i, "base", "float"), fig(i, "base'", "float")
            print(line("(a) float, base", b0))
            print(line("(a) float, base again", b1))
            print(line("(a) float, this build", new))
            print("      this build / base = %.4f    base again / base = %.4f" % (new[0] / b0[0], b1[0] / b0[0]))
        else:
            print(line("(a) float", new))
        s, g = fig(i, "new", "sigma"), fig(i, "new", "generic")
        if s:
            print(line("(b) sigma", s))
            print(line("(c) generic branch", g))
            print("      (b) / (a) = %.4f    (c) / (a) = %.4f    (b) / (c) = %.4f" % (s[0] / new[0], g[0] / new[0], s[0] / g[0]))
            print("      " + checks.get(i, ""))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
