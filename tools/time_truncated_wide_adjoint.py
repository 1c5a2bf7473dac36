#!/usr/bin/env python3
"""Timing of TruncatedSigKernel(wide_adjoint=True) (GPU box): the levels launch forward and the WIDE-ADJOINT mode of k_trunc_sig<4, 1>
backward (csrc/sk_truncated.hip: trunc_wide_adjoint) beside the route these calls take without the keyword and beside the dim-8 adjoint
mode of the same build.

  python tools/time_truncated_wide_adjoint.py [--repeats 5] [--warmup 2] [--torch-rows 4]
      compute_Gram(X, Y).sum().backward() with X requiring grad, forward + backward, interleaved, event-timed, medians:
        wide   TruncatedSigKernel(L, wide_adjoint=True) at path dim 9 .. 16
        torch  (A) the same object without the keyword -- the torch restatement as a whole -- on the first --torch-rows rows of X, scaled
               (it keeps (2 + 6) L arrays of rows x B x M x N under autograd and is tiled over rows anyway)
        dim 8  (B) TruncatedSigKernel(L) on the first 8 coordinates of the same paths: levels + the adjoint mode of k_trunc_sig<1, 2>
      and the worst |dX - torch| / max over the rows the torch route ran.
  python tools/time_truncated_wide_adjoint.py --existing --tree DIR [--repeats 7] [--warmup 2]
      the launches k_trunc_sig<4, 1> already served -- orders 2 - 4, the points forward, the points adjoint, the long forward, and the long
      adjoint -- of the package under DIR (another checkout with its library built: parent and branch run alternately, each in a fresh
      process): one line per shape with the median call time and a checksum of the result's bits."""
import hashlib, sys
import numpy as np, torch

import time_truncated_long_adjoint as long_adjoint_tool     # --tree, the package under it, timed(), path_batch(), existing()
from time_truncated_long_adjoint import arg, timed, sigkernel_amd, _lib, path_batch

# name, A = B, steps, dim, levels
SHAPES = [("512^2 x 128, dim 16, L4", 512, 128, 16, 4), ("512^2 x 128, dim 16, L8", 512, 128, 16, 8),
          ("512^2 x 128, dim 9, L4", 512, 128, 9, 4), ("512^2 x 128, dim 9, L8", 512, 128, 9, 8),
          ("2048^2 x 64, dim 9, L6", 2048, 64, 9, 6)]


def main(repeats, warmup, trows):
    print("# TruncatedSigKernel.compute_Gram(X, Y).sum().backward(), X requires grad (ms, median of %d interleaved repeats after %d warm-ups; "
          "torch route on %d rows of X, scaled)" % (repeats, warmup, trows))
    print("# %s; %s" % (torch.cuda.get_device_name(0), _lib.load().sk_build_info().decode()))
    print("shape\twide fwd+bwd\tmin..max\tfwd alone\twide bwd (difference)\ttorch fwd+bwd (scaled)\ttorch/wide\tdim-8 fwd+bwd\twide/dim-8"
          "\tworst |dX - torch| / max")
    g = torch.Generator().manual_seed(0)
    for name, A, M, D, L in SHAPES:
        mk = lambda n: (0.3 * torch.randn(n, M + 1, D, generator=g, dtype=torch.float64) / np.sqrt(D)).cuda()     # M + 1 points: M steps
        X, Y = mk(A), mk(A)
        X8, Y8 = X[..., :8].contiguous(), Y[..., :8].contiguous()
        wide_k, plain_k = sigkernel_amd.TruncatedSigKernel(L, wide_adjoint=True), sigkernel_amd.TruncatedSigKernel(L)

        def backward(tk, Xs, Ys):
            def fn():
                x = Xs.clone().requires_grad_()
                tk.compute_Gram(x, Ys).sum().backward()
                return x.grad
            return fn

        def fwd():
            with torch.no_grad():
                return wide_k.compute_Gram(X, Y)
        fns = (("wide", backward(wide_k, X, Y)), ("fwd", fwd), ("torch", backward(plain_k, X[:trows], Y)), ("dim8", backward(plain_k, X8, Y8)))
        was = _lib.launch_trace(True)
        _lib.launch_counts(reset=True)
        fns[0][1]()
        torch.cuda.synchronize()
        counts = {k: v for k, v in _lib.launch_counts().items() if "k_trunc_sig" in k and v}
        _lib.launch_trace(was)
        assert any("ILi4ELi1E" in k for k in counts), counts         # the wide mode ran, not the restatement
        t, out = {k: [] for k, _ in fns}, {}
        for i in range(warmup + repeats):
            for k, fn in fns:
                ms, out[k] = timed(fn)
                if i >= warmup:
                    t[k].append(ms)
        med = {k: float(np.median(v)) for k, v in t.items()}
        err = float((out["wide"][:trows] - out["torch"]).abs().max() / out["torch"].abs().max())
        tt = med["torch"] * A / trows
        print("%s\t%.3f\t%.3f..%.3f\t%.3f\t%.3f\t%.1f\t%.1f\t%.3f\t%.2f\t%.2g" % (
            name, med["wide"], min(t["wide"]), max(t["wide"]), med["fwd"], med["wide"] - med["fwd"], tt, tt / med["wide"], med["dim8"],
            med["wide"] / med["dim8"], err), flush=True)
        del X, Y, X8, Y8, out
        torch.cuda.empty_cache()


def existing(repeats, warmup):
    long_adjoint_tool.existing(repeats, warmup)
    g = torch.Generator().manual_seed(3)
    for name, A, M, D, L in (("long fwd+adjoint 256^2 x 300 steps, dim 8, L8", 256, 300, 8, 8), ("long fwd+adjoint 512^2 x 129 steps, dim 8, L4", 512, 129, 8, 4)):
        X, Y = path_batch(A, M, D, g), path_batch(A, M, D, g)
        tk = sigkernel_amd.TruncatedSigKernel(L, long_adjoint=True)

        def fn():
            x = X.clone().requires_grad_()
            tk.compute_Gram(x, Y).sum().backward()
            return x.grad
        ms = [timed(fn)[0] for _ in range(warmup + repeats)][warmup:]
        digest = hashlib.sha256(fn().cpu().numpy().tobytes()).hexdigest()[:16]
        print("%s\t%.4f\t%.4f..%.4f\t%s" % (name, float(np.median(ms)), min(ms), max(ms), digest), flush=True)
        del X, Y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    if "--existing" in sys.argv:
        existing(arg("--repeats", 7), arg("--warmup", 2))
        sys.exit(0)
    main(arg("--repeats", 5), arg("--warmup", 2), arg("--torch-rows", 4))
