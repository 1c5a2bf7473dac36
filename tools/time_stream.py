#!/usr/bin/env python3
"""Timing of SigKernelStream (GPU box; profiles/stream_resume.txt), same-job alternating A/B against an older build.

The base is a copy of the package built from the parent commit under ab_base/<name>/ (tools/ab.py says how to make one).  Every
measurement runs in a process of its own, base and new alternating, so that only timings of ONE job are compared.

  existing   the launches of k_fwd_prefix that existed before the resume mode: compute_Gram_prefixes for the full grid and each slice,
             and compute_Gram_ragged, at the headline shape and C2's shape of the README -- base against new
  feature    a bank against 64 streams with 1024 points of history: st.append(chunk) on the new build against
             compute_Gram_prefixes(X, history + chunk, nodes="last_row") on the BASE, chunks of 1, 16, 64, 256 points; and the share of an
             append that staging the bank again would be (stage_prefix_bank, paid once when the stream is opened)

CALL times, event-timed, medians of --repeats calls after warm-ups.
usage: SK_AB_BASE=<name> python tools/time_stream.py [--rounds 7] [--repeats 9] [--out profiles/stream_resume.txt]

  --column   OFF the fused scope (profiles/stream_column.txt; no base build needed): st.append(chunk) after 64 / 256 / 1024 points of
             history on a stream opened with resume="always" (the column route) against the same append on a stream opened with the
             default (the history route: the parent commit's behaviour), chunks of 1, 16, 64, 256 points, with peak memory; host clock
             around a call that ends in a synchronise.
usage: python tools/time_stream.py --column [--rounds 3] [--repeats 3] [--out profiles/stream_column.txt]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXISTING = [("headline", "linear", 512, 128, 8, 1), ("C2", "rbf", 128, 64, 3, 1)]
FEATURE = [("bank 512 x 128 points, dim 8, Linear, dyadic 1", "linear", 512, 128, 8, 1), ("bank 2048 x 64 points, dim 4, RBF, dyadic 2", "rbf", 2048, 64, 4, 2)]
STREAMS, HISTORY, CHUNKS = 64, 1024, [1, 16, 64, 256]


def one(which, what, repeats):
    sys.path.insert(0, os.path.join(ROOT, "ab_base", which) if which != "new" else ROOT)
    import numpy as np
    import torch
    import sigkernel_amd
    assert os.path.abspath(sigkernel_amd.__file__).startswith((os.path.join(ROOT, "ab_base", which) if which != "new" else ROOT) + os.sep)
    gen = torch.Generator().manual_seed(0)

    def walk(A, M, D):
        return (torch.cumsum(torch.randn(A, M, D, generator=gen, dtype=torch.float64), dim=1) / np.sqrt(M * D)).cuda()

    def kernel(kind):
        return sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(1.0)

    def median(fn, setup=None):
        ts = []
        for i in range(repeats + 3):
            arg = setup() if setup else None
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn(arg) if setup else fn()
            b.record()
            torch.cuda.synchronize()
            del out
            if i >= 3:
                ts.append(a.elapsed_time(b))
        return float(np.median(ts))

    res = {}
    if what == "existing":
        for name, kind, A, M, D, d in EXISTING:
            X, Y = walk(A, M, D), walk(A, M, D)
            sk = sigkernel_amd.SigKernel(kernel(kind), d)
            lx = torch.randint(2, M + 1, (A,), generator=gen)
            ly = torch.randint(2, M + 1, (A,), generator=gen)
            for nodes in ("all", "diagonal", "last_row", "last_col"):
                res["%s %s" % (name, nodes)] = median(lambda: sk.compute_Gram_prefixes(X, Y, nodes=nodes))
            res["%s ragged" % name] = median(lambda: sk.compute_Gram_ragged(X, Y, lx, ly))
    else:
        for name, kind, A, M, D, d in FEATURE:
            X, Y = walk(A, M, D), walk(STREAMS, HISTORY + max(CHUNKS), D)
            sk = sigkernel_amd.SigKernel(kernel(kind), d)
            for c in CHUNKS:
                hist = Y[:, :HISTORY + c].contiguous()
                if which != "new":
                    res["%s | c=%d" % (name, c)] = median(lambda: sk.compute_Gram_prefixes(X, hist, nodes="last_row"))
                else:
                    st = sk.open_stream(X, Y[:, :HISTORY])
                    assert st.resumes
                    chunk = hist[:, HISTORY:]
                    # (appending the same chunk again and again: the values differ from call to call, the work does not)
                    res["%s | c=%d" % (name, c)] = median(lambda: st.append(chunk))
            if which == "new":
                be = sigkernel_amd._lib.get_backend()
                k, p = (0, 1.0) if kind == "linear" else (1, 1.0)
                res["%s | staging the bank" % name] = median(lambda: be.stage_prefix_bank(k, p, X, d, True))
    print("RESULT " + json.dumps(res))


COLUMN = [("256 x 256 pairs, bank of 64 points, dim 20, RBF, dyadic 1", "rbf", 256, 256, 64, 20, 1),
          ("256 x 256 pairs, bank of 300 points, dim 3, Linear, dyadic 1", "linear", 256, 256, 300, 3, 1),
          ("128 x 128 pairs, bank of 64 points, dim 40, RBF, dyadic 1", "rbf", 128, 128, 64, 40, 1)]
HISTORIES = [64, 256, 1024]


def one_column(shape, repeats):
    """one shape of COLUMN on this build: st.append(chunk) after `history` points on a stream opened with resume="always" (the column
    route) and on one opened with the default (the history route: what the parent commit does off the fused scope)"""
    sys.path.insert(0, ROOT)
    import time
    import numpy as np
    import torch
    import sigkernel_amd
    name, kind, A, B, M, D, d = COLUMN[shape]
    gen = torch.Generator().manual_seed(0)

    def walk(n, L):
        return (torch.cumsum(torch.randn(n, L, D, generator=gen, dtype=torch.float64), dim=1) / np.sqrt(L * D)).cuda()

    X, Y = walk(A, M), walk(B, max(HISTORIES) + max(CHUNKS))
    sk = sigkernel_amd.SigKernel(sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(1.0), d)
    res = {}
    for H in HISTORIES:
        for c in CHUNKS:
            chunk = Y[:, H:H + c].contiguous()
            for route in ("column", "history"):
                st = sk.open_stream(X, Y[:, :H].contiguous(), resume="always" if route == "column" else "fused")
                assert st.route == route, st.route
                hist0 = st._hist
                ts = []
                for i in range(repeats + 1):
                    if route == "history":      # (put back to H points: the job must not grow from repeat to repeat)
                        st._hist, st.length = hist0, H
                    torch.cuda.synchronize()
                    if i == 1:
                        torch.cuda.reset_peak_memory_stats()
                        base = torch.cuda.memory_allocated()
                    t0 = time.perf_counter()
                    out = st.append(chunk)
                    torch.cuda.synchronize()
                    if i >= 1:
                        ts.append(1e3 * (time.perf_counter() - t0))
                    del out
                res["%s|%d|%d" % (route, H, c)] = [float(np.median(ts)), min(ts), max(ts), (torch.cuda.max_memory_allocated() - base) / 1e6,
                                                   st.state_bytes / 1e6]
                del st
    print("RESULT " + json.dumps(res))


def main_column(args):
    """profiles/stream_column.txt: the column route against the history route, every shape in a process of its own, `rounds` times"""
    rounds = int(args[args.index("--rounds") + 1]) if "--rounds" in args else 3
    repeats = int(args[args.index("--repeats") + 1]) if "--repeats" in args else 3
    out = args[args.index("--out") + 1] if "--out" in args else None
    lines = ["SigKernelStream off the fused scope: st.append(chunk) after `history` points, resume=\"always\" (column route) against the default",
             "(history route: the parent commit's behaviour), this build.  Call times in ms: host clock around a call that ends in",
             "torch.cuda.synchronize(), after one warm-up call; every shape in a process of its own, %d rounds in one job; a cell is the median over"
             % rounds, "the rounds of each round's median of %d calls, [min .. max] over ALL calls of all rounds = the run-to-run spread.  peak = growth of" % repeats,
             "torch.cuda.max_memory_allocated() over the timed calls.", "command: python tools/time_stream.py " + " ".join(args), ""]
    for s, shape in enumerate(COLUMN):
        runs = []
        for r in range(rounds):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one-column", str(s), str(repeats)], capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                print(p.stdout + p.stderr)
                return p.returncode
            runs.append(json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
            print("shape %d round %d of %d done" % (s, r + 1, rounds), flush=True)
        pairs = shape[2] * shape[3]
        lines.append(shape[0] + "   (state of the column route: %.1f MB, constant)" % runs[0]["column|%d|%d" % (HISTORIES[0], CHUNKS[0])][4])
        lines.append("  chunk  history |   column: median [min .. max]   peak MB |   history route: median [min .. max]   peak MB | history / column")

        def cell(route, H, c):
            meds = sorted(r["%s|%d|%d" % (route, H, c)][0] for r in runs)
            return (meds[len(meds) // 2], min(r["%s|%d|%d" % (route, H, c)][1] for r in runs), max(r["%s|%d|%d" % (route, H, c)][2] for r in runs),
                    max(r["%s|%d|%d" % (route, H, c)][3] for r in runs))
        for c in CHUNKS:
            cols = []
            for H in HISTORIES:
                a, b = cell("column", H, c), cell("history", H, c)
                cols.append(a)
                lines.append("  %5d  %7d | %9.3f [%9.3f .. %9.3f] %9.1f | %10.3f [%10.3f .. %10.3f] %9.1f | %8.1fx"
                             % (c, H, a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3], b[0] / a[0]))
            meds = [a[0] for a in cols]
            spread = max(a[2] - a[1] for a in cols)
            lines.append("         column route over the histories: medians span %.3f ms, the widest run-to-run spread of a cell %.3f ms: %s; "
                         "%.3f us per pair and append" % (max(meds) - min(meds), spread, "inside" if max(meds) - min(meds) <= spread else "OUTSIDE",
                                                         1e3 * meds[0] / pairs))
        lines.append("")
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text)
    return 0


def main():
    args = sys.argv[1:]
    if args and args[0] == "--one":
        return one(args[1], args[2], int(args[3]))
    if args and args[0] == "--one-column":
        return one_column(int(args[1]), int(args[2]))
    if "--column" in args:
        return main_column(args)
    rounds = int(args[args.index("--rounds") + 1]) if "--rounds" in args else 7
    repeats = int(args[args.index("--repeats") + 1]) if "--repeats" in args else 9
    out = args[args.index("--out") + 1] if "--out" in args else None
    base = os.environ.get("SK_AB_BASE", "parent")
    runs = {(w, what): [] for w in (base, "new") for what in ("existing", "feature")}
    for r in range(rounds):
        for what in ("existing", "feature"):
            for w in (base, "new"):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", w, what, str(repeats)], capture_output=True, text=True, timeout=600)
                if p.returncode != 0:
                    print(p.stdout + p.stderr)
                    return p.returncode
                runs[(w, what)].append(json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
        print("round %d of %d done" % (r + 1, rounds), flush=True)
    lines = ["SigKernelStream: call times in ms, %d alternating runs per build in one job (each run: the median of %d calls)" % (rounds, repeats), ""]
    lines.append("EXISTING LAUNCHES of k_fwd_prefix, base (the parent commit) against new: median [min .. max] over the runs")
    for key in runs[(base, "existing")][0]:
        b = sorted(r[key] for r in runs[(base, "existing")])
        n = sorted(r[key] for r in runs[("new", "existing")])
        mb, mn = b[len(b) // 2], n[len(n) // 2]
        inside = abs(mn - mb) <= 2 * (b[-1] - b[0])
        lines.append("  %-20s base %8.4f [%8.4f .. %8.4f]   new %8.4f [%8.4f .. %8.4f]   new - base %+8.4f   twice the base's range %7.4f   %s"
                     % (key, mb, b[0], b[-1], mn, n[0], n[-1], mn - mb, 2 * (b[-1] - b[0]), "inside" if inside else "OUTSIDE"))
    lines += ["", "THE FEATURE: %d streams with %d points of history; st.append(chunk) on the new build against" % (STREAMS, HISTORY),
              "compute_Gram_prefixes(X, history + chunk, nodes=\"last_row\") on the base"]
    for key in runs[("new", "feature")][0]:
        n = sorted(r[key] for r in runs[("new", "feature")])
        mn = n[len(n) // 2]
        if key in runs[(base, "feature")][0]:
            b = sorted(r[key] for r in runs[(base, "feature")])
            mb = b[len(b) // 2]
            lines.append("  %-58s recompute %8.4f [%8.4f .. %8.4f]   append %8.4f [%8.4f .. %8.4f]   %6.2fx" % (key, mb, b[0], b[-1], mn, n[0], n[-1], mb / mn))
        else:
            lines.append("  %-58s %8.4f [%8.4f .. %8.4f]" % (key, mn, n[0], n[-1]))
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
