#!/usr/bin/env python3
"""Timing of the truncated kernel's LONG mode (GPU box): k_trunc_sig<4, 1> with row bands and column tiles (csrc/sk_truncated.hip:
trunc_long) beside the torch restatement of the same call, its cost per cell beside the plain launch, and the A/B of the launches that
share its instance.

  python tools/time_truncated_long.py [--repeats 5] [--warmup 2] [--torch-rows 1]
      truncated_sig_kernel / truncated_sig_kernel_paired at order 1, fp64, event-timed around the public calls (staging and allocation
      included), interleaved, medians:
        (a) routes.truncated_long on: ONE launch of k_trunc_sig<4, 1> in its long mode;
        (b) the switch off -- what the call takes by default: the torch restatement on the same device.  It holds eight arrays of
            rows x B x M x N, so it is timed on the first --torch-rows rows of X (pairs, when paired) and SCALED to the batch (it is tiled
            over rows anyway);
      the last column is the run's own accuracy check, (a) against (b) on the timed rows, of the matrix's max-norm.
      Then the cost per cell: 128 x 128 steps, inside the plain scope, through the plain launch (k_trunc_sig<1, 2>) and forced through the
      long mode (one band, one tile: what the mode's step costs beside the plain one), and the long shapes' cells per second beside them.
  python tools/time_truncated_long.py --few-pairs [--repeats 3] [--warmup 1]
      where the restatement wins: 1 .. 64 pairs of 200 .. 4096 steps, (a) against (b) on the WHOLE batch -- one wave sweeps one pair, so
      below the GPU's resident waves (a) does not fall with the pair count and (b) does.
  python tools/time_truncated_long.py --existing --tree DIR [--repeats 7] [--warmup 2]
      the launches k_trunc_sig<4, 1> already served -- orders 2 - 4, the points forward, the points adjoint -- of the package under DIR
      (another checkout with its library built: parent and branch run alternately, each in a fresh process): one line per shape with the
      median call time and a checksum of the result's bits."""
import hashlib, os, sys
import numpy as np, torch

import time_truncated_static_adjoint as base     # --tree, the package under it, timed(), paths(), the forward shapes
from time_truncated_static_adjoint import arg, timed, sigkernel_amd, _lib

# name, A, B, steps M, steps N, dim, levels, paired
LONG_SHAPES = [("256^2 x 512 steps, dim 16, L4", 256, 256, 512, 512, 16, 4, False), ("256^2 x 512 steps, dim 16, L8", 256, 256, 512, 512, 16, 8, False),
               ("512^2 x 256 steps, dim 8, L8", 512, 512, 256, 256, 8, 8, False), ("512^2 x 129 steps, dim 8, L8", 512, 512, 129, 129, 8, 8, False),
               ("64 pairs x 4096 steps, dim 8, L8", 64, 64, 4096, 4096, 8, 8, True)]
# inside the plain scope: name, A = B, steps, dim, levels
CELL_SHAPES = [("512^2 x 128 steps, dim 8, L8", 512, 128, 8, 8), ("256^2 x 128 steps, dim 16, L4", 256, 128, 16, 4),
               ("256^2 x 128 steps, dim 16, L8", 256, 128, 16, 8)]


def step_batch(n, M, D, g):
    v = torch.randn(n, M, D, generator=g, dtype=torch.float64)
    return (v * (0.35 / v.norm(dim=2, keepdim=True))).cuda()


def interleaved(fns, repeats, warmup):
    t, out = {k: [] for k, _ in fns}, {}
    for i in range(warmup + repeats):
        for k, fn in fns:
            ms, out[k] = timed(fn)
            if i >= warmup:
                t[k].append(ms)
    return t, out


def long_shapes(repeats, warmup, trows):
    print("# truncated_sig_kernel(X, Y, L, 1.0, order=1), fp64 (ms, median of %d interleaved repeats after %d warm-ups; torch route on %d row(s) "
          "of X, scaled)" % (repeats, warmup, trows))
    print("# %s; %s" % (torch.cuda.get_device_name(0), _lib.load().sk_build_info().decode()))
    print("shape\t(a) long mode\tmin..max\tGcells/s\t(b) torch restatement (scaled)\tb/a\tworst |a - b| / max")
    g = torch.Generator().manual_seed(0)
    rates = {}
    for name, A, B, M, N, D, L, paired in LONG_SHAPES:
        X, Y = step_batch(A, M, D, g), step_batch(B, N, D, g)
        call = sigkernel_amd.truncated_sig_kernel_paired if paired else sigkernel_amd.truncated_sig_kernel

        def hip():
            sigkernel_amd.routes.truncated_long = True
            try:
                return call(X, Y, L, 1.0, 1)
            finally:
                sigkernel_amd.routes.truncated_long = False

        def restatement():
            return call(X[:trows], Y[:trows] if paired else Y, L, 1.0, 1)
        t, out = interleaved((("hip", hip), ("torch", restatement)), repeats, warmup)
        ms, tt = float(np.median(t["hip"])), float(np.median(t["torch"])) * A / trows
        err = float((out["hip"][:trows] - out["torch"]).abs().max() / out["torch"].abs().max())
        rates[name] = (A if paired else A * B) * M * N / ms / 1e6
        print("%s\t%.3f\t%.3f..%.3f\t%.2f\t%.1f\t%.1f\t%.2g" % (name, ms, min(t["hip"]), max(t["hip"]), rates[name], tt, tt / ms, err), flush=True)
        del X, Y, out
        torch.cuda.empty_cache()
    print("\n# cost per cell inside the plain scope: truncated_levels (k_trunc_sig<1, 2>) and truncated_long forced on the same tensors (one band, one tile)")
    print("shape\tplain launch\tGcells/s\tlong mode\tGcells/s\tlong / plain\tbit-equal")
    be = _lib.get_backend()
    for name, A, M, D, L in CELL_SHAPES:
        X, Y = step_batch(A, M, D, g), step_batch(A, M, D, g)
        t, out = interleaved((("plain", lambda: be.truncated_levels(X, Y, L, 1)), ("long", lambda: be.truncated_long(X, Y, L, None, False, None, no_swap=True))),
                             repeats, warmup)
        p, l = float(np.median(t["plain"])), float(np.median(t["long"]))
        cells = A * A * M * M / 1e6
        print("%s\t%.3f\t%.2f\t%.3f\t%.2f\t%.3f\t%s" % (name, p, cells / p, l, cells / l, l / p, torch.equal(out["plain"], out["long"])), flush=True)
        del X, Y, out
        torch.cuda.empty_cache()


def few_pairs(repeats, warmup):
    print("# truncated_sig_kernel(X, Y, L, 1.0, order=1), fp64, A x B pairs of steps x steps (ms, median of %d interleaved repeats after %d warm-up(s))"
          % (repeats, warmup))
    print("pairs\tsteps\tD\tL\tlong ms\ttorch ms\ttorch/long", flush=True)
    g = torch.Generator().manual_seed(0)
    for D, L in ((8, 8), (8, 4), (16, 8)):
        for steps in (200, 512, 1024, 4096):
            for A in (1, 2, 4, 8):
                if steps == 4096 and A > 4:
                    continue
                X, Y = step_batch(A, steps, D, g), step_batch(A, steps, D, g)

                def hip():
                    sigkernel_amd.routes.truncated_long = True
                    try:
                        return sigkernel_amd.truncated_sig_kernel(X, Y, L, 1.0, 1)
                    finally:
                        sigkernel_amd.routes.truncated_long = False
                t, out = interleaved((("hip", hip), ("torch", lambda: sigkernel_amd.truncated_sig_kernel(X, Y, L, 1.0, 1))), repeats, warmup)
                h, tt = float(np.median(t["hip"])), float(np.median(t["torch"]))
                print("%d\t%d\t%d\t%d\t%.3f\t%.3f\t%.2f" % (A * A, steps, D, L, h, tt, tt / h), flush=True)
                del X, Y, out
                torch.cuda.empty_cache()


def existing(repeats, warmup):
    base.forward_ab(repeats, warmup)
    g = torch.Generator().manual_seed(1)
    name, A, P, D, L = base.GRAD_SHAPES[0]
    X, Y = base.paths(A, P, D, g), base.paths(A, P, D, g)
    tk = sigkernel_amd.TruncatedSigKernel(L, static_kernel=sigkernel_amd.RBFKernel(1.0), points_adjoint=True)

    def fn():
        x = X.clone().requires_grad_()
        tk.compute_Gram(x, Y).sum().backward()
        return x.grad
    ms = [timed(fn)[0] for _ in range(warmup + repeats)][warmup:]
    digest = hashlib.sha256(fn().cpu().numpy().tobytes()).hexdigest()[:16]
    print("points fwd+adjoint %s\t%.4f\t%.4f..%.4f\t%s" % (name, float(np.median(ms)), min(ms), max(ms), digest), flush=True)


if __name__ == "__main__":
    if "--existing" in sys.argv:
        existing(arg("--repeats", 7), arg("--warmup", 2))
    elif "--few-pairs" in sys.argv:
        few_pairs(arg("--repeats", 3), arg("--warmup", 1))
    else:
        long_shapes(arg("--repeats", 5), arg("--warmup", 2), arg("--torch-rows", 1))
