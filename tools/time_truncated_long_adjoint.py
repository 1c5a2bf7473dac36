#!/usr/bin/env python3
"""Timing of TruncatedSigKernel(long_adjoint=True) (GPU box): the long mode's levels launch forward and the LONG-ADJOINT mode of
k_trunc_sig<4, 1> backward (csrc/sk_truncated.hip: trunc_long_adjoint) beside the torch restatement of the same call, the long forward
launch alone, the plain adjoint mode where both serve, and the A/B of the launches that share the instance.

  python tools/time_truncated_long_adjoint.py [--repeats 3] [--warmup 1] [--torch-rows 1]
      compute_Gram(X, Y).sum().backward() (paired: compute_kernel) with X requiring grad, forward + backward, paths of steps + 1 points,
      fp64, event-timed around the public calls (differencing, staging, allocation and the chunk sum included), interleaved, medians:
        (a) long_adjoint=True at the default workspace_bytes (1 GiB): the slabs lower the block count (printed);
        (b) long_adjoint=True with a workspace that lets 8 blocks per CU keep their slabs (printed);
        (c) the same object without the keyword -- what the call takes today: the torch restatement on the same device, timed on the first
            --torch-rows rows of X (pairs, when paired) and SCALED to the batch (it is tiled over rows anyway);
        (d) the long mode's levels launch alone (HipBackend.truncated_long on the steps): what one forward sweep costs.
      The last column is the run's own accuracy check: dX of (b) against (c) on the timed rows, of the gradient's max-norm.
      Then 128 x 256 steps, inside the plain adjoint's scope: HipBackend.truncated_adjoint (k_trunc_sig<1, 2>) and truncated_long_adjoint
      forced on the same tensors (one band, one tile) -- the price of generality.
  python tools/time_truncated_long_adjoint.py --existing --tree DIR [--repeats 7] [--warmup 2]
      the launches k_trunc_sig<4, 1> already served -- orders 2 - 4, the points forward, the points adjoint, the long forward -- of the
      package under DIR (another checkout with its library built: parent and branch run alternately, each in a fresh process): one line
      per shape with the median call time and a checksum of the result's bits."""
import ctypes, hashlib, sys
import numpy as np, torch

import time_truncated_long as long_tool     # --tree, the package under it, timed(), step_batch(), existing()
from time_truncated_long import arg, timed, sigkernel_amd, _lib, step_batch, interleaved

# name, A, B, steps M, steps N, dim, levels, paired
SHAPES = [("512^2 x 256 steps, dim 8, L4", 512, 512, 256, 256, 8, 4, False), ("512^2 x 256 steps, dim 8, L8", 512, 512, 256, 256, 8, 8, False),
          ("256^2 x 512 steps, dim 8, L8", 256, 256, 512, 512, 8, 8, False), ("512^2 x 129 steps, dim 8, L8", 512, 512, 129, 129, 8, 8, False),
          ("64 pairs x 4096 steps, dim 8, L8", 64, 64, 4096, 4096, 8, 8, True)]


def path_batch(n, M, D, g):
    return torch.cat([torch.zeros(n, 1, D, dtype=torch.float64).cuda(), torch.cumsum(step_batch(n, M, D, g), 1)], 1)


def plan(A, B, M, N, D, L, paired, ws):
    out = (ctypes.c_int64 * 4)()
    rc = _lib.load().sk_truncated_long_adjoint_plan(A, B, M, N, D, L, int(paired), ws, ctypes.cast(out, ctypes.c_void_p))
    assert rc == 0, rc
    return tuple(out)       # n_chunks, blocks, the launch's slab bytes, one block's


def gradient(repeats, warmup, trows):
    print("# TruncatedSigKernel(L).compute_Gram(X, Y).sum().backward(), X requires grad, fp64 (ms, median of %d interleaved repeats after %d "
          "warm-up(s); torch route on %d row(s) of X, scaled)" % (repeats, warmup, trows))
    print("# %s; %s" % (torch.cuda.get_device_name(0), _lib.load().sk_build_info().decode()))
    print("shape\t(a) 1 GiB: blocks\tfwd+bwd ms\t(b) full: blocks\tworkspace MiB\tfwd+bwd ms\tmin..max\t(d) long fwd alone\t(b - d) / d\t"
          "(c) torch fwd+bwd (scaled)\tc/a\tc/b\tworst |dX(b) - dX(c)| / max")
    g = torch.Generator().manual_seed(0)
    be = _lib.get_backend()
    for name, A, B, M, N, D, L, paired in SHAPES:
        X, Y = path_batch(A, M, D, g), path_batch(B, N, D, g)
        dX, dY = (X[:, 1:] - X[:, :-1]).contiguous(), (Y[:, 1:] - Y[:, :-1]).contiguous()
        method = "compute_kernel" if paired else "compute_Gram"
        _, blocks_d, _, block = plan(A, B, M, N, D, L, paired, 1 << 30)
        _, blocks_f, total, _ = plan(A, B, M, N, D, L, paired, 1 << 50)
        ws = max(total, 1 << 30)

        def backward(tk, rows):
            def run():
                x = X[:rows].clone().requires_grad_()
                getattr(tk, method)(x, Y[:rows] if paired else Y).sum().backward()
                return x.grad
            return run
        fns = (("a", backward(sigkernel_amd.TruncatedSigKernel(L, long_adjoint=True), A)),
               ("b", backward(sigkernel_amd.TruncatedSigKernel(L, long_adjoint=True, workspace_bytes=ws), A)),
               ("d", lambda: be.truncated_long(dX, dY, L, None, paired, None)),
               ("c", backward(sigkernel_amd.TruncatedSigKernel(L), trows)))
        t, out = interleaved(fns, repeats, warmup)
        med = {k: float(np.median(v)) for k, v in t.items()}
        tt = med["c"] * A / trows
        err = float((out["b"][:trows] - out["c"]).abs().max() / out["c"].abs().max())
        print("%s\t%d\t%.2f\t%d\t%.0f\t%.2f\t%.2f..%.2f\t%.2f\t%.2f\t%.0f\t%.1f\t%.1f\t%.2g" % (
            name, blocks_d, med["a"], blocks_f, ws / 2 ** 20, med["b"], min(t["b"]), max(t["b"]), med["d"], (med["b"] - med["d"]) / med["d"], tt,
            tt / med["a"], tt / med["b"], err), flush=True)
        del X, Y, dX, dY, out
        torch.cuda.empty_cache()
    print("\n# inside the plain adjoint's scope: truncated_adjoint (k_trunc_sig<1, 2>) and truncated_long_adjoint on the same tensors (one band, one tile)")
    print("shape\tplain adjoint ms\tlong adjoint ms\tlong / plain\tworst |difference| / max")
    for name, A, M, N, D, L in (("512^2 x 128 x 256 steps, dim 8, L8", 512, 128, 256, 8, 8), ("512^2 x 128 x 256 steps, dim 8, L4", 512, 128, 256, 8, 4)):
        X, Y = step_batch(A, M, D, g), step_batch(A, N, D, g)
        w = torch.randn(L, A, A, generator=g, dtype=torch.float64).cuda()
        ws = max(plan(A, A, M, N, D, L, False, 1 << 50)[2], 1 << 30)
        t, out = interleaved((("plain", lambda: be.truncated_adjoint(X, Y, w, L, False, ws)), ("long", lambda: be.truncated_long_adjoint(X, Y, w, L, False, ws))),
                             repeats, warmup)
        p, l = float(np.median(t["plain"])), float(np.median(t["long"]))
        print("%s\t%.2f\t%.2f\t%.3f\t%.2g" % (name, p, l, l / p, float((out["plain"] - out["long"]).abs().max() / out["plain"].abs().max())), flush=True)
        del X, Y, w, out
        torch.cuda.empty_cache()


def existing(repeats, warmup):
    long_tool.existing(repeats, warmup)
    g = torch.Generator().manual_seed(2)
    be = _lib.get_backend()
    for name, A, M, D, L in (("long fwd 256^2 x 300 steps, dim 8, L8", 256, 300, 8, 8), ("long fwd 128^2 x 300 steps, dim 16, L4", 128, 300, 16, 4)):
        X, Y = step_batch(A, M, D, g), step_batch(A, M, D, g)
        fn = lambda: be.truncated_long(X, Y, L, None, False, None)
        ms = [timed(fn)[0] for _ in range(warmup + repeats)][warmup:]
        digest = hashlib.sha256(fn().cpu().numpy().tobytes()).hexdigest()[:16]
        print("%s\t%.4f\t%.4f..%.4f\t%s" % (name, float(np.median(ms)), min(ms), max(ms), digest), flush=True)
        del X, Y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    if "--existing" in sys.argv:
        existing(arg("--repeats", 7), arg("--warmup", 2))
    else:
        gradient(arg("--repeats", 3), arg("--warmup", 1), arg("--torch-rows", 1))
