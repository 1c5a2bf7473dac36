#!/usr/bin/env python3
"""Timing of truncated_sig_kernel (GPU box): the HIP route (k_trunc_sig) against the torch restatement of the recursion on the same
inputs, in one process, interleaved, event-timed, medians.  These are CALL times (staging and allocation included).  The torch route
holds (2 d^2 + 6) arrays of rows x B x M x N, so it is timed on the first --torch-rows rows of X and scaled to the batch (it is tiled
over rows anyway: the per-row cost does not depend on the batch).  KERNEL times come from a kernel trace of the HIP side alone:
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o t -- python tools/time_truncated.py --hip-only --repeats 5
    python tools/time_truncated.py --from-trace DIR [--repeats 5]     -> median k_trunc_sig time per shape, fp64 lane operations per second
usage: python tools/time_truncated.py [--repeats 7] [--warmup 2] [--torch-rows 8] [--out profiles/r09_truncated.txt]"""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sigkernel_amd
from sigkernel_amd import _lib
from sigkernel_amd.truncated import _truncated_torch

FP64_PEAK = 78.6e12     # vector fp64 FLOP/s, the figure DESIGN.md uses (an FMA counts two)

# name, A = B, steps, dim, levels, order, dtype
SHAPES = [("512^2 x 128, L4 o1", 512, 128, 8, 4, 1, torch.float64), ("512^2 x 128, L8 o1", 512, 128, 8, 8, 1, torch.float64),
          ("512^2 x 64, L4 full", 512, 64, 8, 4, -1, torch.float64), ("512^2 x 64, L8 o4", 512, 64, 8, 8, 4, torch.float64),
          ("2048^2 x 64, dim 4, L6 o1", 2048, 64, 4, 6, 1, torch.float64), ("2048^2 x 64, dim 4, L4 full", 2048, 64, 4, 4, -1, torch.float64),
          ("512^2 x 128, L4 o1 fp32", 512, 128, 8, 4, 1, torch.float32)]


def lane_ops_per_node(D, L, order):
    """fp64 lane operations per node of the sweep as written (csrc/sk_truncated.hip), an FMA as one: fd for G, per level the sums of its
    planes and the weighted total, per next level its planes (one or two products each) and the four prefix updates"""
    fd = 8 if D <= 8 else 16
    o = L if order < 1 else order
    n = fd
    for lv in range(1, L + 1):
        d = min(lv, o)
        n += 3 * d * d + 1
        if lv < L:
            dn = min(lv + 1, o)
            n += 2 * dn * dn + 2 + 2 * (dn - 1)
    return n


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    del out
    return a.elapsed_time(b)


def from_trace(d, per_shape):
    import csv, glob
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted((r for r in csv.DictReader(open(f)) if "k_trunc_sig" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == per_shape * len(SHAPES), (len(rows), per_shape)
    print("shape\tkernel_ms (median of %d)\tmin..max\tlane_ops_per_node\tfp64_lane_TFLOP/s (FMA = 2)\tshare_of_78.6" % per_shape)
    for i, (name, A, M, D, L, order, dt) in enumerate(SHAPES):
        ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows[i * per_shape:(i + 1) * per_shape]]
        ops = lane_ops_per_node(D, L, order)
        rate = 2.0 * ops * A * A * M * M / (float(np.median(ms)) * 1e-3)
        print("%s\t%.3f\t%.3f..%.3f\t%d\t%.2f\t%.2f" % (name, float(np.median(ms)), min(ms), max(ms), ops, rate / 1e12, rate / FP64_PEAK))


def main():
    arg = lambda name, d: type(d)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else d
    repeats, warmup, out_path, trows = arg("--repeats", 7), arg("--warmup", 2), arg("--out", ""), arg("--torch-rows", 8)
    if "--from-trace" in sys.argv:
        return from_trace(arg("--from-trace", ""), repeats + warmup)
    lines = ["# truncated_sig_kernel: HIP route vs torch route (ms, median of %d interleaved repeats after %d warm-ups; torch timed on %d rows of X and scaled)"
             % (repeats, warmup, trows), "# %s; %s" % (torch.cuda.get_device_name(0), _lib.load().sk_build_info().decode()),
             "shape\tpairs\thip_ms\tmin..max\ttorch_ms (scaled)\ttorch/hip\tlane_ops_per_node\tshare_of_78.6_TFLOP/s (call time)"]
    g = torch.Generator().manual_seed(0)
    for name, A, M, D, L, order, dt in SHAPES:
        X = (0.3 * torch.randn(A, M, D, generator=g, dtype=torch.float64) / np.sqrt(D)).to(dt).cuda()
        Y = (0.3 * torch.randn(A, M, D, generator=g, dtype=torch.float64) / np.sqrt(D)).to(dt).cuda()
        hip = lambda: sigkernel_amd.truncated_sig_kernel(X, Y, L, sigma=1., order=order)
        ref = lambda: _truncated_torch(X[:trows], Y, L, 1., order)
        sides = {"hip": hip} if "--hip-only" in sys.argv else {"hip": hip, "torch": ref}
        t = {k: [] for k in sides}
        for i in range(warmup + repeats):
            for k, fn in sides.items():
                ms = timed(fn)
                if i >= warmup:
                    t[k].append(ms)
        if "--hip-only" in sys.argv:
            continue
        med = {k: float(np.median(v)) for k, v in t.items()}
        tt = med["torch"] * A / trows
        ops = lane_ops_per_node(D, L, order)
        lines.append("%s (dim %d, %s)\t%d\t%.3f\t%.3f..%.3f\t%.1f\t%.1f\t%d\t%.3f" % (
            name, D, str(dt).split(".")[1], A * A, med["hip"], min(t["hip"]), max(t["hip"]), tt, tt / med["hip"], ops,
            2.0 * ops * A * A * M * M / (med["hip"] * 1e-3) / FP64_PEAK))
        print(lines[-1], flush=True)
        del X, Y
        torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
