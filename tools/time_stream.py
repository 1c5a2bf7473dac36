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
usage: SK_AB_BASE=<name> python tools/time_stream.py [--rounds 7] [--repeats 9] [--out profiles/stream_resume.txt]"""
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


def main():
    args = sys.argv[1:]
    if args and args[0] == "--one":
        return one(args[1], args[2], int(args[3]))
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
