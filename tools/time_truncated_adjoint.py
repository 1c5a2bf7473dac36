#!/usr/bin/env python3
"""Timing of TruncatedSigKernel's gradient (GPU box), and the A/B of the forward launches that share its kernel instance.

  python tools/time_truncated_adjoint.py [--repeats 5] [--warmup 2] [--torch-rows 4]
      compute_Gram(X, Y).sum().backward() with X requiring grad, forward + backward: the HIP route (levels mode + adjoint mode of
      k_trunc_sig<1, 2>) against the same object forced onto the torch route with the same workspace, interleaved, event-timed, medians;
      the HIP forward alone beside it, so backward alone = the difference.  The torch route keeps (2 + 6) L arrays of rows x B x M x N
      under autograd, so it is timed on the first --torch-rows rows of X and scaled (it is tiled over rows anyway).
  python tools/time_truncated_adjoint.py --forward --tree DIR [--repeats 7] [--warmup 2]
      the plain, paired and levels launches of the package under DIR (another checkout with its library built: parent and branch run
      alternately, each in a fresh process): one line per shape with the median call time and a checksum of the result's bits."""
import hashlib, os, sys
import numpy as np, torch

arg = lambda name, d: type(d)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else d
ROOT = os.path.abspath(arg("--tree", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)
import sigkernel_amd
from sigkernel_amd import _lib

# name, A = B, steps, dim, levels
GRAD_SHAPES = [("512^2 x 128, dim 8, L4", 512, 128, 8, 4), ("512^2 x 128, dim 8, L8", 512, 128, 8, 8), ("2048^2 x 64, dim 4, L6", 2048, 64, 4, 6)]
# name, call, A = B, steps, dim, levels, order
FWD_SHAPES = [("gram 512^2 x 128, L4 o1", "gram", 512, 128, 8, 4, 1), ("gram 512^2 x 128, L8 o1", "gram", 512, 128, 8, 8, 1),
              ("gram 512^2 x 64, L8 o4", "gram", 512, 64, 8, 8, 4), ("gram 2048^2 x 64, dim 4, L6 o1", "gram", 2048, 64, 4, 6, 1),
              ("levels 512^2 x 128, L8 o1", "levels", 512, 128, 8, 8, 1), ("paired 262144 x 64, dim 4, L6 o1", "paired", 262144, 64, 4, 6, 1)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def inputs(A, M, D, g, B=None):
    mk = lambda n: (0.3 * torch.randn(n, M, D, generator=g, dtype=torch.float64) / np.sqrt(D)).cuda()
    return mk(A), mk(A if B is None else B)


def forward_ab(repeats, warmup):
    g = torch.Generator().manual_seed(0)
    print("# %s; %s" % (ROOT, _lib.load().sk_build_info().decode()))
    for name, call, A, M, D, L, order in FWD_SHAPES:
        X, Y = inputs(A, M, D, g)
        fn = {"gram": lambda: sigkernel_amd.truncated_sig_kernel(X, Y, L, sigma=1., order=order),
              "paired": lambda: sigkernel_amd.truncated_sig_kernel_paired(X, Y, L, sigma=1., order=order),
              "levels": lambda: sigkernel_amd.truncated_sig_kernel_levels(X, Y, L, order=order)}[call]
        ms = [timed(fn)[0] for _ in range(warmup + repeats)][warmup:]
        digest = hashlib.sha256(fn().cpu().numpy().tobytes()).hexdigest()[:16]
        print("%s\t%.4f\t%.4f..%.4f\t%s" % (name, float(np.median(ms)), min(ms), max(ms), digest), flush=True)
        del X, Y
        torch.cuda.empty_cache()


def gradient(repeats, warmup, trows):
    from sigkernel_amd.truncated import _truncated_levels_torch, truncated_from_levels
    print("# TruncatedSigKernel.compute_Gram(X, Y).sum().backward(), X requires grad (ms, median of %d interleaved repeats after %d warm-ups; "
          "torch route on %d rows of X, scaled)" % (repeats, warmup, trows))
    print("# %s; %s" % (torch.cuda.get_device_name(0), _lib.load().sk_build_info().decode()))
    print("shape\thip fwd+bwd\tmin..max\thip fwd alone\thip bwd (difference)\tbwd/fwd\ttorch fwd+bwd (scaled)\ttorch/hip\tworst |dX - torch| / max")
    g = torch.Generator().manual_seed(0)
    for name, A, M, D, L in GRAD_SHAPES:
        X, Y = inputs(A, M + 1, D, g)            # paths of M + 1 points: M steps
        tk = sigkernel_amd.TruncatedSigKernel(L)

        def hip():
            x = X.clone().requires_grad_()
            tk.compute_Gram(x, Y).sum().backward()
            return x.grad

        def fwd():
            with torch.no_grad():
                return tk.compute_Gram(X, Y)

        def ref():
            x = X[:trows].clone().requires_grad_()
            dx, dy = x[:, 1:] - x[:, :-1], Y[:, 1:] - Y[:, :-1]
            truncated_from_levels(_truncated_levels_torch(dx, dy, L, 1, False, tk.workspace_bytes), 1.).sum().backward()
            return x.grad
        t = {"hip": [], "fwd": [], "torch": []}
        out = {}
        for i in range(warmup + repeats):
            for k, fn in (("hip", hip), ("fwd", fwd), ("torch", ref)):
                ms, out[k] = timed(fn)
                if i >= warmup:
                    t[k].append(ms)
        med = {k: float(np.median(v)) for k, v in t.items()}
        err = float((out["hip"][:trows] - out["torch"]).abs().max() / out["torch"].abs().max())
        tt = med["torch"] * A / trows
        print("%s\t%.3f\t%.3f..%.3f\t%.3f\t%.3f\t%.2f\t%.1f\t%.1f\t%.2g" % (
            name, med["hip"], min(t["hip"]), max(t["hip"]), med["fwd"], med["hip"] - med["fwd"], (med["hip"] - med["fwd"]) / med["fwd"], tt,
            tt / med["hip"], err), flush=True)
        del X, Y, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    if "--forward" in sys.argv:
        forward_ab(arg("--repeats", 7), arg("--warmup", 2))
    else:
        gradient(arg("--repeats", 5), arg("--warmup", 2), arg("--torch-rows", 4))
