#!/usr/bin/env python3
"""Call times of compute_Gram(X, Y).sum().backward() (forward + backward, host clock around a device synchronise) on one GPU:

  default   SigKernel(...)                         -- the reference's adjoint formula on its fastest route
  exact     SigKernel(..., exact_gradient=True)    -- the discrete solver's true gradient (sk_solve_adj_* with SK_FLAG_DISCRETE)
  torch     torch autograd through a vectorised anti-diagonal restatement of the solver, on the same GPU -- what a user would
            write to get the true gradient without the HIP mode

at the two shapes of profiles/exact_gradient.txt.  The three routes alternate inside every round; medians over the rounds.
Also prints how far each route's X.grad is from the torch restatement's (the exact route must agree, the default must not)."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sigkernel_amd  # noqa: E402

DEV = "cuda:0"


def torch_restatement(X, Y, kernel, d, naive=False):
    """(A, B) Gram matrix of the discrete solver, every anti-diagonal of all pairs as one torch expression (autograd keeps them)"""
    G = kernel.Gram_matrix(X, Y)
    inc = G[..., 1:, 1:] + G[..., :-1, :-1] - G[..., 1:, :-1] - G[..., :-1, 1:]
    r = 1 << d
    g = (inc.repeat_interleave(r, -2).repeat_interleave(r, -1) * 0.25 ** d).flatten(0, 1)      # (P, MM, NN)
    P, MM, NN = g.shape
    g = g.reshape(P, MM * NN)
    p = 1. + 0.5 * g + (0. if naive else g * g / 12.)
    q = torch.ones_like(g) if naive else 1. - g * g / 12.
    prev2 = prev = torch.ones(P, MM + 1, dtype=X.dtype, device=X.device)      # node diagonals s - 2 and s - 1, indexed by the row i
    for s in range(2, MM + NN + 1):
        ilo, ihi = max(1, s - NN), min(MM, s - 1)
        i = torch.arange(ilo, ihi + 1, device=X.device)
        idx = (i - 1) * NN + (s - i - 1)
        new = torch.ones(P, MM + 1, dtype=X.dtype, device=X.device)
        new[:, ilo:ihi + 1] = (prev[:, ilo:ihi + 1] + prev[:, ilo - 1:ihi]) * p[:, idx] - prev2[:, ilo - 1:ihi] * q[:, idx]
        prev2, prev = prev, new
    return prev[:, MM].reshape(X.shape[0], Y.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="scale the batch sizes (a rehearsal at a toy size)")
    args = ap.parse_args()
    shapes = [("128 x 128 pairs, 64 points, dim 3, RBF, dyadic 1", 128, 64, 3, sigkernel_amd.RBFKernel(1.0), 1),
              ("256 x 256 pairs, 64 points, dim 8, Linear, dyadic 0", 256, 64, 8, sigkernel_amd.LinearKernel(), 0)]
    for name, A, M, D, kernel, d in shapes:
        A = max(2, int(A * args.scale))
        gen = torch.Generator().manual_seed(A + D)
        X = (torch.cumsum(torch.randn(A, M, D, generator=gen, dtype=torch.float64), 1) / (M * D) ** 0.5).to(DEV)
        Y = (torch.cumsum(torch.randn(A, M, D, generator=gen, dtype=torch.float64), 1) / (M * D) ** 0.5).to(DEV)
        default, exact = sigkernel_amd.SigKernel(kernel, d), sigkernel_amd.SigKernel(kernel, d, exact_gradient=True)
        routes = {"default": lambda x: default.compute_Gram(x, Y), "exact": lambda x: exact.compute_Gram(x, Y),
                  "torch": lambda x: torch_restatement(x, Y, kernel, d)}
        times, grads = {k: [] for k in routes}, {}
        for rnd in range(args.rounds + 2):          # two warm-up rounds
            for key, fn in routes.items():
                x = X.clone().requires_grad_(True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(x).sum().backward()
                torch.cuda.synchronize()
                if rnd >= 2:
                    times[key].append(time.perf_counter() - t0)
                grads[key] = x.grad
        med = {k: statistics.median(v) for k, v in times.items()}
        print(name)
        for k in routes:
            gap = float((grads[k] - grads["torch"]).norm() / grads["torch"].norm())
            print("  %-8s median %9.3f ms  (min %9.3f, max %9.3f, %d rounds)   |X.grad - torch's| / |torch's| = %.2e"
                  % (k, 1e3 * med[k], 1e3 * min(times[k]), 1e3 * max(times[k]), len(times[k]), gap))
        print("  exact / default = %.2f    torch / exact = %.2f" % (med["exact"] / med["default"], med["torch"] / med["exact"]), flush=True)


if __name__ == "__main__":
    main()
