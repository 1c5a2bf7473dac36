#!/usr/bin/env python3
"""Timing of compute_Gram_prefixes (GPU box): the fused prefix kernel against the same result from the streamed pieces (increments ->
the streaming solver's full grid -> its coarse nodes, tiled to the same budget: routes.no_fused_prefix) and against compute_Gram on the
same inputs (the same sweep without the stores -- the floor).  All sides in one process, interleaved, event-timed, medians.  These are
CALL times: staging, the output's allocation (from the caching allocator after the warm-ups -- its cache is not emptied between
repeats) and the fill of row 0 included.  KERNEL times come from a kernel trace of the fused side alone:
    rocprofv3 --kernel-trace -f csv -d DIR -o t -- python tools/time_prefixes.py --fused-only --repeats 5
    python tools/time_prefixes.py --from-trace DIR [--repeats 5]      -> median k_fwd_prefix time per shape, store rate
with SK_PREFIX_STORE=1|2|3 in the environment of the traced run for the store schemes of csrc/sk_wave_prefix.hip.
usage: python tools/time_prefixes.py [--repeats 11] [--warmup 2] [--out profiles/r08_prefixes.txt]"""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sigkernel_amd
from sigkernel_amd import _lib

HBM_PEAK = 8e12      # bytes / s, the figure the README's rooflines use

# name, kernel, A = B, points, dim, dyadic, dtype
SHAPES = [("headline", "linear", 512, 128, 8, 1, torch.float64), ("C2", "rbf", 128, 64, 3, 1, torch.float64),
          ("C4 / 512", "rbf", 512, 64, 4, 2, torch.float64), ("headline fp32", "linear", 512, 128, 8, 1, torch.float32)]


def walk(g, A, M, D, dt):
    return (torch.cumsum(torch.randn(A, M, D, generator=g, dtype=torch.float64), 1) / np.sqrt(M * D)).to(dt).cuda()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    del out
    return a.elapsed_time(b)


def from_trace(d, per_shape):
    """median duration of the k_fwd_prefix dispatches of a traced --fused-only run, per shape (per_shape dispatches each, in order)"""
    import csv, glob
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted((r for r in csv.DictReader(open(f)) if "k_fwd_prefix" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == per_shape * len(SHAPES), (len(rows), per_shape)
    print("shape\tkernel_ms (median of %d)\tmin..max\toutput_GB\tstore_TB/s\tshare_of_8TB/s" % per_shape)
    for i, (name, kname, A, M, D, d_, dt) in enumerate(SHAPES):
        ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows[i * per_shape:(i + 1) * per_shape]]
        gb = A * A * M * M * (8 if dt == torch.float64 else 4) / 1e9
        bw = gb * 1e9 / (float(np.median(ms)) * 1e-3)
        print("%s\t%.3f\t%.3f..%.3f\t%.2f\t%.2f\t%.2f" % (name, float(np.median(ms)), min(ms), max(ms), gb, bw / 1e12, bw / HBM_PEAK))


def main():
    arg = lambda name, d: type(d)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else d
    repeats, warmup, out_path = arg("--repeats", 11), arg("--warmup", 2), arg("--out", "")
    if "--from-trace" in sys.argv:
        return from_trace(arg("--from-trace", ""), repeats + warmup)
    lines = ["# compute_Gram_prefixes: fused prefix kernel vs streamed pieces vs compute_Gram (ms, median of %d interleaved repeats after %d warm-ups)"
             % (repeats, warmup), "# %s; %s" % (torch.cuda.get_device_name(0), _lib.load().sk_build_info().decode()),
             "shape\tpairs\tfused_ms\tmin..max\tstreamed_ms\tmin..max\tgram_ms\tstreamed/fused\tfused/gram\toutput_GB\tstore_TB/s\tshare_of_8TB/s"]
    g = torch.Generator().manual_seed(0)
    routes = sigkernel_amd.routes
    for name, kname, A, M, D, d, dt in SHAPES:
        sk = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(1.0) if kname == "rbf" else sigkernel_amd.LinearKernel(), d)
        X, Y = walk(g, A, M, D, dt), walk(g, A, M, D, dt)

        def fused():
            routes.no_fused_prefix = False
            return sk.compute_Gram_prefixes(X, Y)

        def streamed():
            routes.no_fused_prefix = True
            try:
                return sk.compute_Gram_prefixes(X, Y)
            finally:
                routes.no_fused_prefix = False
        sides = {"fused": fused, "streamed": streamed, "gram": lambda: sk.compute_Gram(X, Y)}
        if "--fused-only" in sys.argv:      # (a traced run: kernel times are read from the trace)
            for i in range(warmup + repeats):
                timed(fused)
            del X, Y
            torch.cuda.empty_cache()
            continue
        t = {k: [] for k in sides}
        for i in range(warmup + repeats):
            for k, fn in sides.items():
                ms = timed(fn)
                if i >= warmup:
                    t[k].append(ms)
        med = {k: float(np.median(v)) for k, v in t.items()}
        gb = A * A * M * M * X.element_size() / 1e9
        bw = gb * 1e9 / (med["fused"] * 1e-3)
        lines.append("%s (%s %dx%d, %d points, dim %d, d=%d, %s)\t%d\t%.3f\t%.3f..%.3f\t%.3f\t%.3f..%.3f\t%.3f\t%.2f\t%.2f\t%.2f\t%.2f\t%.2f"
                     % (name, kname, A, A, M, D, d, str(dt).split(".")[1], A * A, med["fused"], min(t["fused"]), max(t["fused"]), med["streamed"],
                        min(t["streamed"]), max(t["streamed"]), med["gram"], med["streamed"] / med["fused"], med["fused"] / med["gram"], gb,
                        bw / 1e12, bw / HBM_PEAK))
        print(lines[-1], flush=True)
        del X, Y
        torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
