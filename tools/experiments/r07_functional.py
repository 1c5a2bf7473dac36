#!/usr/bin/env python3
"""Paths of more than 32 dims and function-valued paths: the HIP route (k_static_wide_mfma) against the generic route (Gram_matrix
in torch + sk_increments, autograd through the static kernel) on the same box in the same run, the two alternated.  A subclass such
as `_GenericRBF(RBFKernel)` always takes the generic route (_fused_static tests `type(...) is`), so no route switch is needed.
    python tools/experiments/r07_functional.py [--reps R] [--only SUBSTRING]      (GPU box)   -> profiles/r07_functional.txt
Times: median and [min, max] of R alternated repetitions (ms, CUDA events around the call, synchronised).  --only picks the cases
whose label contains SUBSTRING (a profiler run of one shape: rocprofv3 --kernel-trace --stats -- python ... --only ...)."""
import argparse, os, statistics, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import sigkernel_amd as S


class _GenericRBF(S.RBFKernel):
    pass


class _GenericLinear(S.LinearKernel):
    pass


def walk(g, A, M, D):
    return (torch.cumsum(torch.randn(A, M, D, generator=g, dtype=torch.float64), 1) / np.sqrt(M)).cuda()


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def case(label, fns, reps, out):
    for f in fns.values():        # warm-up
        f()
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            t[k].append(timed(f))
    med = {k: statistics.median(v) for k, v in t.items()}
    line = "%-58s " % label + "  ".join("%s %8.3f [%.3f, %.3f]" % (k, med[k], min(t[k]), max(t[k])) for k in fns)
    if "hip" in med and "generic" in med:
        line += "  speed-up %.2fx" % (med["generic"] / med["hip"])
    print(line, flush=True)
    out.append(line)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    out = []
    print("# %s; median [min, max] of %d alternated repetitions, ms" % (torch.cuda.get_device_name(0), a.reps))
    # function-valued paths: 128 x 128 paths, T = 32, Lx = 64 / 128 / 256, d = 1, dyadic 1
    for kname in ("RBF_ID", "RBF_CEXP"):
        for Lx in (64, 128, 256):
            k = S.RBF_ID_Kernel(float(Lx)) if kname == "RBF_ID" else S.RBF_CEXP_Kernel(2.0, float(Lx) / 8, 8)
            X = walk(g, 128, 32, Lx).reshape(128, 32, Lx, 1)
            Y = walk(g, 128, 32, Lx).reshape(128, 32, Lx, 1)
            hip = S.SigKernel(k, 1)

            def gen_of(X, Y, k=k, Lx=Lx):      # the same feature map, then the generic route of the base kernel
                return S.SigKernel(_GenericRBF(k.base_kernel.sigma), 1), k.features(X), k.features(Y)

            def gram(sk):
                return lambda: sk.compute_Gram(X, Y)

            def gram_gen():
                sk, fx, fy = gen_of(X, Y)
                sk.compute_Gram(fx, fy)

            def grad(hip_route):
                def f():
                    Xg = X.clone().requires_grad_(True)
                    if hip_route:
                        hip.compute_Gram(Xg, Y).sum().backward()
                    else:
                        sk, fx, fy = gen_of(Xg, Y)
                        sk.compute_Gram(fx, fy).sum().backward()
                return f

            def esr(hip_route):
                def f():
                    Xg = X.clone().requires_grad_(True)
                    if hip_route:
                        hip.compute_expected_scoring_rule(Xg, Y).backward()
                    else:
                        sk, fx, fy = gen_of(Xg, Y)
                        sk.compute_expected_scoring_rule(fx, fy).backward()
                return f

            base = "%s 128x128 T=32 Lx=%d" % (kname, Lx)
            for what, fns in (("Gram", {"hip": gram(hip), "generic": gram_gen}), ("Gram+backward", {"hip": grad(True), "generic": grad(False)}),
                              ("expected_scoring_rule+backward", {"hip": esr(True), "generic": esr(False)})):
                if a.only in base + " " + what:
                    case(base + " " + what, fns, a.reps, out)
    # plain Linear / RBF: 256 x 256 pairs of 64 points, D = 48 / 64 / 128, dyadic 1
    for kname in ("Linear", "RBF"):
        for D in (48, 64, 128):
            X, Y = walk(g, 256, 64, D), walk(g, 256, 64, D)
            mk = (lambda gen: (_GenericLinear() if gen else S.LinearKernel())) if kname == "Linear" else \
                 (lambda gen, D=D: (_GenericRBF(float(D)) if gen else S.RBFKernel(float(D))))
            sks = {"hip": S.SigKernel(mk(False), 1), "generic": S.SigKernel(mk(True), 1)}
            base = "%sKernel 256x256 M=N=64 D=%d" % (kname, D)

            def fw(sk):
                return lambda: sk.compute_Gram(X, Y)

            def bw(sk):
                def f():
                    Xg = X.clone().requires_grad_(True)
                    sk.compute_Gram(Xg, Y).sum().backward()
                return f
            for what, mkf in (("Gram", fw), ("Gram+backward", bw)):
                if a.only in base + " " + what:
                    med = case(base + " " + what, {k: mkf(v) for k, v in sks.items()}, a.reps, out)
            if a.only in base:
                # the increment kernel alone, and its share of fp64 peak (2 D flops per node, 256 x 256 x 64 x 64 nodes)
                be = S._lib.get_backend()
                code, par = (0, 1.0) if kname == "Linear" else (1, float(D))
                t = [timed(lambda: be.static_increments(code, par, X, Y, True)) for _ in range(a.reps)]
                tm = statistics.median(t)
                flops = 2.0 * D * 256 * 256 * 64 * 64
                line = "%-58s increments kernel %.3f ms  %.1f TFLOP/s fp64 (%.1f %% of the 78.6 TFLOP/s fp64 peak, spec), %.2f GB written" % (
                    base + " static_increments", tm, flops / tm / 1e9, 100 * flops / tm / 1e9 / 78.6, 256 * 256 * 63 * 64 * 8 / 1e9)
                print(line, flush=True)
                out.append(line)


if __name__ == "__main__":
    main()
