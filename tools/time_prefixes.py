#!/usr/bin/env python3
"""Timing of compute_Gram_prefixes (GPU box): the fused prefix kernel against the same result from the streamed pieces (increments ->
the streaming solver's full grid -> its coarse nodes, tiled to the same budget: routes.no_fused_prefix) and against compute_Gram on the
same inputs (the same sweep without the stores -- the floor).  All sides in one process, interleaved, event-timed, medians.  These are
CALL times: staging, the output's allocation (from the caching allocator after the warm-ups -- its cache is not emptied between
repeats) and the fill of row 0 included.  KERNEL times come from a kernel trace of the fused side alone:
    rocprofv3 --kernel-trace -f csv -d DIR -o t -- python tools/time_prefixes.py --fused-only --repeats 5
    python tools/time_prefixes.py --from-trace DIR [--repeats 5]      -> median k_fwd_prefix time per shape, store rate
with SK_PREFIX_STORE=1|2|3 in the environment of the traced run for the store schemes of csrc/sk_wave_prefix.hip.
usage: python tools/time_prefixes.py [--repeats 11] [--warmup 2] [--out profiles/r08_prefixes.txt]

SLICES (nodes="diagonal" | "last_row" | "last_col", profiles/r10_prefix_slices.txt): per shape and mode, interleaved in one process,
(1) the slice call, (2) the way to the same values without the store modes -- compute_Gram_prefixes(X, Y) followed by the torch slice,
made contiguous --, (3) compute_Gram alone (the sweep without stores); then "diagonal" on 4096 x 4096 pairs of 64 points, dim 4, whose
full grid (550 GB) does not exist on any card.  Kernel times of the slice calls from a kernel trace of them alone:
    python tools/time_prefixes.py --slices [--repeats 11] [--out profiles/r10_prefix_slices.txt]
    rocprofv3 --kernel-trace -f csv -d DIR -o t -- python tools/time_prefixes.py --slices --slices-only --repeats 5
    python tools/time_prefixes.py --slices --from-trace DIR [--repeats 5]"""
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


NODES = ("diagonal", "last_row", "last_col")
BIG = ("4096 x 4096", "rbf", 4096, 64, 4, 1, torch.float64)      # "diagonal" only: the full grid would be 550 GB


def take(grid, nodes):
    if nodes == "diagonal":
        return torch.diagonal(grid, dim1=-2, dim2=-1).contiguous()
    return (grid[..., -1, :] if nodes == "last_row" else grid[..., :, -1]).contiguous()


def slices_from_trace(d, per_call):
    """median duration of the k_fwd_prefix dispatches of a traced --slices --slices-only run: per_call dispatches per (shape, mode), in order"""
    import csv, glob
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted((r for r in csv.DictReader(open(f)) if "k_fwd_prefix" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
    calls = [(sh[0], n) for sh in SHAPES for n in NODES] + [(BIG[0], "diagonal")]
    assert len(rows) == per_call * len(calls), (len(rows), per_call, len(calls))
    print("shape\tnodes\tkernel_ms (median of %d)\tmin..max" % per_call)
    for i, (name, n) in enumerate(calls):
        ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows[i * per_call:(i + 1) * per_call]]
        print("%s\t%s\t%.3f\t%.3f..%.3f" % (name, n, float(np.median(ms)), min(ms), max(ms)))


def slices(repeats, warmup, out_path):
    only = "--slices-only" in sys.argv      # (a traced run: kernel times are read from the trace)
    lines = ["# slices of the prefix grid: (1) compute_Gram_prefixes(nodes=...), (2) compute_Gram_prefixes + the torch slice, (3) compute_Gram"
             " (ms, median of %d interleaved repeats after %d warm-ups)" % (repeats, warmup),
             "# %s; %s" % (torch.cuda.get_device_name(0), _lib.load().sk_build_info().decode()),
             "shape\tnodes\tslice_ms\tmin..max\tgrid_then_slice_ms\tmin..max\tgram_ms\tmin..max\tfull_grid_ms\tgrid_then_slice/slice\tslice/gram\tslice_MB"]
    g = torch.Generator().manual_seed(0)
    for name, kname, A, M, D, d, dt in SHAPES + [BIG]:
        sk = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(1.0) if kname == "rbf" else sigkernel_amd.LinearKernel(), d)
        X, Y = walk(g, A, M, D, dt), walk(g, A, M, D, dt)
        big = name == BIG[0]
        for nodes in (("diagonal",) if big else NODES):
            sides = {"slice": lambda: sk.compute_Gram_prefixes(X, Y, nodes=nodes)}
            if not only:
                sides["gram"] = lambda: sk.compute_Gram(X, Y)
                if not big:
                    sides["grid_then_slice"] = lambda: take(sk.compute_Gram_prefixes(X, Y), nodes)
                    sides["full_grid"] = lambda: sk.compute_Gram_prefixes(X, Y)
            t = {k: [] for k in sides}
            for i in range(warmup + repeats):
                for k, fn in sides.items():
                    ms = timed(fn)
                    if i >= warmup:
                        t[k].append(ms)
            if only:
                continue
            med = {k: float(np.median(v)) for k, v in t.items()}
            rng = lambda k: "%.3f..%.3f" % (min(t[k]), max(t[k]))
            mb = A * A * M * X.element_size() / 1e6
            if big:
                lines.append("%s (%s, %d points, dim %d, d=%d, %s)\t%s\t%.3f\t%s\t(550 GB grid: cannot run)\t-\t%.3f\t%s\t-\t-\t%.2f\t%.1f"
                             % (name, kname, M, D, d, str(dt).split(".")[1], nodes, med["slice"], rng("slice"), med["gram"], rng("gram"),
                                med["slice"] / med["gram"], mb))
            else:
                lines.append("%s (%s %dx%d, %d points, dim %d, d=%d, %s)\t%s\t%.3f\t%s\t%.3f\t%s\t%.3f\t%s\t%.3f\t%.2f\t%.2f\t%.1f"
                             % (name, kname, A, A, M, D, d, str(dt).split(".")[1], nodes, med["slice"], rng("slice"), med["grid_then_slice"],
                                rng("grid_then_slice"), med["gram"], rng("gram"), med["full_grid"], med["grid_then_slice"] / med["slice"],
                                med["slice"] / med["gram"], mb))
            print(lines[-1], flush=True)
        del X, Y
        torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    arg = lambda name, d: type(d)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else d
    repeats, warmup, out_path = arg("--repeats", 11), arg("--warmup", 2), arg("--out", "")
    if "--slices" in sys.argv:
        if "--from-trace" in sys.argv:
            return slices_from_trace(arg("--from-trace", ""), repeats + warmup)
        return slices(repeats, warmup, out_path)
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
