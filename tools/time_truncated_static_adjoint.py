#!/usr/bin/env python3
"""Timing of the gradient of TruncatedSigKernel with an RBF static kernel (GPU box): the points-adjoint mode of k_trunc_sig beside the
torch restatement of the same call and the plain kernel's HIP adjoint, and the A/B of the forward launches that share its instance.

  python tools/time_truncated_static_adjoint.py [--repeats 5] [--warmup 2] [--torch-rows 2] [--rbf-sigma 1.0]
      compute_Gram(X, Y).sum().backward() with X requiring grad, forward + backward, paths of `points` points, event-timed around the
      public calls (staging and allocation included), interleaved, medians:
        (a) static_kernel=RBFKernel(s), points_adjoint=True: the points mode's levels launch + one points-adjoint launch (k_trunc_sig<4, 1>);
        (b) the same object without the keyword -- what every call took before it existed: the torch restatement on the same device.  It
            keeps (2 + 7) L arrays of rows x B x M x N under autograd, so it is timed on the first --torch-rows rows of X and scaled (it
            is tiled over rows anyway);
        (c) static_kernel=None on the same paths, for scale: the levels mode + the adjoint mode of k_trunc_sig<1, 2>, points - 1 steps;
      and (a)'s forward alone, so its backward alone is the difference.  The last column is the run's own accuracy check: (a) against (b)
      on the timed rows, in units of the gradient's max-norm.
  python tools/time_truncated_static_adjoint.py --forward --tree DIR [--repeats 7] [--warmup 2]
      the forward launches k_trunc_sig<4, 1> serves -- the points mode and orders 2 - 4 on 64 steps -- of the package under DIR (another
      checkout with its library built: parent and branch run alternately, each in a fresh process): one line per shape with the median
      call time and a checksum of the result's bits."""
import hashlib, os, sys
import numpy as np, torch

arg = lambda name, d: type(d)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else d
ROOT = os.path.abspath(arg("--tree", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)
import sigkernel_amd
from sigkernel_amd import _lib

# name, A = B, points, dim, levels
GRAD_SHAPES = [("512^2 x 128, dim 8, L4", 512, 128, 8, 4), ("512^2 x 128, dim 8, L8", 512, 128, 8, 8), ("2048^2 x 64, dim 4, L6", 2048, 64, 4, 6)]
# name, A = B, points, dim, levels, order; order 0: the points mode (RBFKernel(1)), else the plain kernel on the paths' steps
FWD_SHAPES = [("points 512^2 x 128, dim 8, L4", 512, 128, 8, 4, 0), ("points 512^2 x 128, dim 8, L8", 512, 128, 8, 8, 0),
              ("points 2048^2 x 64, dim 4, L6", 2048, 64, 4, 6, 0), ("gram 512^2 x 64 steps, L8 o2", 512, 65, 8, 8, 2),
              ("gram 512^2 x 64 steps, L8 o3", 512, 65, 8, 8, 3), ("gram 512^2 x 64 steps, L8 o4", 512, 65, 8, 8, 4)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def paths(n, P, D, g):
    return torch.cumsum(0.3 * torch.randn(n, P, D, generator=g, dtype=torch.float64) / np.sqrt(D), 1).cuda()


def forward_ab(repeats, warmup):
    g = torch.Generator().manual_seed(0)
    print("# %s; %s" % (ROOT, _lib.load().sk_build_info().decode()))
    for name, A, P, D, L, order in FWD_SHAPES:
        X, Y = paths(A, P, D, g), paths(A, P, D, g)
        tk = sigkernel_amd.TruncatedSigKernel(L, 1., max(order, 1), static_kernel=None if order else sigkernel_amd.RBFKernel(1.0))

        def fn():
            with torch.no_grad():
                return tk.compute_Gram(X, Y)
        ms = [timed(fn)[0] for _ in range(warmup + repeats)][warmup:]
        digest = hashlib.sha256(fn().cpu().numpy().tobytes()).hexdigest()[:16]
        print("%s\t%.4f\t%.4f..%.4f\t%s" % (name, float(np.median(ms)), min(ms), max(ms), digest), flush=True)
        del X, Y
        torch.cuda.empty_cache()


def gradient(repeats, warmup, trows, s):
    print("# TruncatedSigKernel.compute_Gram(X, Y).sum().backward(), X requires grad, RBFKernel(%g) (ms, median of %d interleaved repeats after "
          "%d warm-ups; torch route on %d rows of X, scaled)" % (s, repeats, warmup, trows))
    print("# %s; %s" % (torch.cuda.get_device_name(0), _lib.load().sk_build_info().decode()))
    print("shape\t(a) hip fwd+bwd\tmin..max\thip fwd alone\thip bwd (difference)\tbwd/fwd\t(b) torch fwd+bwd (scaled)\tb/a\t(c) plain hip fwd+bwd\ta/c\t"
          "worst |dX(a) - dX(b)| / max")
    g = torch.Generator().manual_seed(0)
    for name, A, P, D, L in GRAD_SHAPES:
        X, Y = paths(A, P, D, g), paths(A, P, D, g)
        rbf = sigkernel_amd.RBFKernel(s)
        hipk = sigkernel_amd.TruncatedSigKernel(L, static_kernel=rbf, points_adjoint=True)
        torchk = sigkernel_amd.TruncatedSigKernel(L, static_kernel=rbf)
        plaink = sigkernel_amd.TruncatedSigKernel(L)

        def backward(tk, rows):
            def run():
                x = X[:rows].clone().requires_grad_()
                tk.compute_Gram(x, Y).sum().backward()
                return x.grad
            return run

        def fwd():
            with torch.no_grad():
                return hipk.compute_Gram(X, Y)
        fns = (("hip", backward(hipk, A)), ("fwd", fwd), ("torch", backward(torchk, trows)), ("plain", backward(plaink, A)))
        t, out = {k: [] for k, _ in fns}, {}
        for i in range(warmup + repeats):
            for k, fn in fns:
                ms, out[k] = timed(fn)
                if i >= warmup:
                    t[k].append(ms)
        med = {k: float(np.median(v)) for k, v in t.items()}
        err = float((out["hip"][:trows] - out["torch"]).abs().max() / out["torch"].abs().max())
        tt = med["torch"] * A / trows
        print("%s\t%.3f\t%.3f..%.3f\t%.3f\t%.3f\t%.2f\t%.1f\t%.1f\t%.3f\t%.2f\t%.2g" % (
            name, med["hip"], min(t["hip"]), max(t["hip"]), med["fwd"], med["hip"] - med["fwd"], (med["hip"] - med["fwd"]) / med["fwd"], tt,
            tt / med["hip"], med["plain"], med["hip"] / med["plain"], err), flush=True)
        del X, Y, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    if "--forward" in sys.argv:
        forward_ab(arg("--repeats", 7), arg("--warmup", 2))
    else:
        gradient(arg("--repeats", 5), arg("--warmup", 2), arg("--torch-rows", 2), arg("--rbf-sigma", 1.0))
