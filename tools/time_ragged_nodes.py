#!/usr/bin/env python3
"""Call times for profiles/ragged_nodes.txt, tools/ab.py's protocol: every (build, case) runs in a process of its own, the builds
alternate within ONE job, three rounds; a time is the host clock around a call that ends in torch.cuda.synchronize(), after warm-up.

  existing launches (the parent's package under ab_base/<SK_AB_BASE>/ against the working tree): compute_Gram on the streaming route,
  sk_solve_fwd on 131 072 pairs of 127 x 127 increments, one want_grid call -- the kernels that gained a launch-time mode;
  the feature (working tree only): compute_Gram_ragged, lengths uniform in [2, M], on the stored-grid route (routes.no_ragged_nodes), the
  default route, the opt-in route (routes.ragged_stream), and compute_Gram on the padded batch (the floor of a padded sweep), with the
  peak memory of each.

usage: SK_AB_BASE=parent tools/time_ragged_nodes.py [existing] [feature]"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXISTING = ["gram:linear:256:64:20:1:f64", "gram:rbf:256:64:20:1:f64", "gram:linear:256:64:20:1:f32", "gram:rbf:256:64:20:1:f32",
            "gram:linear:64:600:20:1:f64", "solve:131072:127:0", "grid:1024:64:1"]
FEATURE = ["rbf:256:64:20:1", "linear:256:300:3:1", "rbf:128:64:40:1"]
MODES = ["stored_grid", "default", "stream", "padded"]


def one(which, case, mode):
    sys.path.insert(0, os.path.join(ROOT, "ab_base", which) if which != "new" else ROOT)
    import numpy as np
    import torch
    import sigkernel_amd
    from sigkernel_amd import _lib
    gen = torch.Generator().manual_seed(0)

    def walk(A, M, D, dt=torch.float64):
        return (torch.cumsum(torch.randn(A, M, D, generator=gen, dtype=torch.float64), dim=1) / np.sqrt(M * D)).to(dt).cuda()

    def kernel(kind):
        return sigkernel_amd.RBFKernel(1.0) if kind == "rbf" else sigkernel_amd.LinearKernel()
    f = case.split(":")
    n = 10
    if f[0] == "gram":
        A, M, D, d = (int(v) for v in f[2:6])
        dt = torch.float64 if f[6] == "f64" else torch.float32
        X, Y = walk(A, M, D, dt), walk(A, M, D, dt)
        sk = sigkernel_amd.SigKernel(kernel(f[1]), d)
        fn = lambda: sk.compute_Gram(X, Y)
    elif f[0] == "solve":
        P, Mc, d = int(f[1]), int(f[2]), int(f[3])
        inc = torch.zeros(P, Mc, 128, dtype=torch.float64, device="cuda")
        inc[..., :Mc] = torch.randn(1, Mc, Mc, generator=gen, dtype=torch.float64).cuda() / Mc
        inc = inc[..., :Mc]
        be = _lib.get_backend()
        fn = lambda: be.solve_fwd(inc, d, flags=_lib.FLAG_FAST_ONLY)
    elif f[0] == "grid":
        P, Mc, d = int(f[1]), int(f[2]), int(f[3])
        inc = torch.randn(P, Mc, Mc, generator=gen, dtype=torch.float64).cuda() / Mc
        be = _lib.get_backend()
        fn = lambda: be.solve_fwd(inc, d, want_grid=True)[1]
    else:
        A, M, D, d = (int(v) for v in f[1:5])
        X, Y = walk(A, M, D), walk(A, M, D)
        g = np.random.default_rng(1)
        lx, ly = torch.tensor(g.integers(2, M + 1, A)), torch.tensor(g.integers(2, M + 1, A))
        sk = sigkernel_amd.SigKernel(kernel(f[0]), d)
        sigkernel_amd.routes.no_ragged_nodes = mode == "stored_grid"
        sigkernel_amd.routes.ragged_stream = mode == "stream"
        fn = (lambda: sk.compute_Gram(X, Y)) if mode == "padded" else (lambda: sk.compute_Gram_ragged(X, Y, lx, ly))
        n = 6
    for _ in range(3):
        out = fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    peak = (torch.cuda.max_memory_allocated() - base) / 1e6
    print("%-7s %-30s %-12s median %9.3f ms  (min %9.3f .. max %9.3f)  peak +%8.1f MB  checksum %r"
          % (which, case, mode, float(np.median(ts)), min(ts), max(ts), peak, float(out.double().sum())), flush=True)


def main():
    what = sys.argv[1:] or ["existing", "feature"]
    base = os.environ.get("SK_AB_BASE", "parent")
    if "existing" in what:
        for case in EXISTING:
            for _ in range(3):
                for which in (base, "new"):
                    subprocess.run([sys.executable, __file__, "--one", which, case, "-"])
    if "feature" in what:
        for case in FEATURE:
            for _ in range(3):
                for mode in MODES:
                    subprocess.run([sys.executable, __file__, "--one", "new", case, mode])


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(*sys.argv[2:5])
    else:
        main()
