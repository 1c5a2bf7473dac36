#!/usr/bin/env python3
"""Choose the cases of the instance ledger (tests/instance_cases.py) on a GPU box: for every kernel instance of the build at least one
small call whose outputs tests/test_gpu_instances.py compares with the CPU oracle while that instance is on the launch trace.

    python tools/instance_cover.py --replay replay.json      (GPU)  every item of tools/reach_sweep.py on its own, the trace reset per item,
                                                                    plus the candidates the sweep has no use for (full-order truncated calls,
                                                                    a Gram block with one large-kernel pair); then smaller candidates: the
                                                                    same call with the smallest batch that still launches the same instances
    python tools/instance_cover.py --cover replay.json --table tests/instance_cases.py      (CPU)  greedy set cover, cheapest oracle work
                                                                    (fine-grid cells) per newly covered instance first; writes the table

--replay also writes replay.json.counts ("count<TAB>symbol", what reach_sweep.py --out gives).  Without arguments: both steps."""
import json, os, pprint, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import reach_sweep
import instance_ledger as L

VARIANTS = os.path.join(ROOT, "profiles", "r06_variants.txt")
# an fp32 call through one of these units hands fp32 arrays (increments, adjoint weights) from one launch to the next: its bound is measured
F32_STAGE_UNITS = ("sk_static", "sk_increments", "sk_simple", "sk_wave", "sk_wave_adj", "sk_wave_deriv")
# claimed by a case with one legitimately large-kernel pair only: with tame pairs these kernels run and write nothing
RESCUE_ONLY = ("k_screen", "k_fused_rescue", "k_adj_rescue<double>", "k_adj_rescue<float>")
# the golden truncated calls every table holds whatever the cover would choose: order 1 over several levels, an order below the levels,
# four levels at the full order (tests/golden/truncated.npz, fixtures 6, 8, 12)
FORCED_FIXTURES = (6, 8, 12)
SHRINK_ABOVE = 2e8                                # cells: a case above this is worth a search for a smaller batch
KEEP_PER_INSTANCE = 4


def table_rows():
    rows = []
    for ln in open(VARIANTS):
        p = ln.rstrip("\n").split("\t")
        if len(p) >= 9 and p[0] != "unit":
            rows.append((p[0], p[7], p[8]))
    return rows


def extras():
    """Candidates the sweep does not make: truncated_sig_kernel at the FULL order (the only one the tensor-level Chen oracle defines;
    one level: the order-1 instance, three: the general one; direct and on (y, x)), and the rescue's case (one large-kernel pair)."""
    out = []
    for dt in ("f64", "f32"):
        for A, B, M, N, D, lv in ((5, 7, 100, 40, 6, 1), (5, 7, 200, 60, 6, 1), (3, 4, 65, 33, 5, 1), (5, 7, 40, 30, 6, 3), (2, 3, 200, 21, 3, 3), (3, 4, 33, 65, 4, 4)):
            out.append(reach_sweep._spec("truncated", "none", None, dt, 0, False, A, B, M, N, D, 7000 + M, L=lv, order=-1))
    z = __import__("numpy").load(os.path.join(ROOT, "tests", "golden", "truncated.npz"))
    for c in FORCED_FIXTURES:
        X, Y = z["c%02d_X" % c], z["c%02d_Y" % c]
        out.append(reach_sweep._spec("truncated_golden", "none", None, "f64", 0, False, X.shape[0], Y.shape[0], X.shape[1], Y.shape[1], X.shape[2], c,
                                     L=int(z["c%02d_num_levels" % c]), order=int(z["c%02d_order" % c]), fixture=c))
    # the stored-grid rescue of the streaming adjoint: increments with one pair whose residual exceeds the self-check's tolerance
    for dt in ("f64", "f32"):
        out.append(reach_sweep._spec("adj_wild", "none", None, dt, 1, False, 6, 1, 63, 63, 0, 5, wild=[2]))
    # the derivative solver on GIVEN increments, fp64 and fp32, at the lengths of the sweep's derivative calls
    for dt in ("f64", "f32"):
        for d in (0, 1, 2):
            for M, N in [(m, n) for m, n in reach_sweep.SHAPES if max(m, n) <= 130] + [(65, 130), (129, 140), (129, 200), (100, 140), (300, 520)]:
                out.append(reach_sweep._spec("deriv", "none", None, dt, d, False, 12, 1, M - 1, N - 1, 0, 900 + M))
    for kind, D, d in (("linear", 4, 1), ("rbf", 4, 2), ("rbf", 3, 1)):
        out.append(reach_sweep._spec("gram_grad", kind, 1.0 if kind == "rbf" else None, "f64", d, False, 6, 40, 32, 32, D, 41, wild=[2, 5], w="randn"))
    return out


def launched(spec):
    from sigkernel_amd import _lib
    be = _lib.get_backend()
    be.last_fused_ppg = None
    was = _lib.launch_trace(True)
    try:
        _lib.launch_counts(reset=True)
        out = reach_sweep.execute(spec)
        torch.cuda.synchronize()
        COUNTS.clear(); COUNTS.update(_lib.launch_counts(reset=True))
    finally:
        _lib.launch_trace(was)
    del out
    if spec.get("free"):
        torch.cuda.empty_cache()
    return set(k.split(".kd")[0] for k, v in COUNTS.items() if v > 0), getattr(be, "last_fused_ppg", None)


COUNTS = {}      # launches per device symbol of the last launched() call


def budgeted(spec, ppg):
    """the spec as a case would carry it (random upstream weights for a gradient); None if its oracle work is over the cap"""
    spec = dict(spec)
    if spec["op"] in reach_sweep.GRAD_OPS:
        spec["w"] = "randn"
    return spec if L.cells(spec) <= L.CELL_CAP else None


def smaller(spec, want):
    """the same call with the smallest batch (odd sizes: a chunk or share split never comes out even) that still launches `want`"""
    A, B = spec["A"], spec["B"]
    if A <= 5: return None
    if spec["op"] == "gram_sym_grad" and not spec.get("knobs"):
        # the blocked triangle is gated by the call's grid cells (sym_min_cells): lower that threshold through the host layer's own
        # override, if the trace shows the same instances
        k = dict(spec, knobs={"_SYM_MIN_CELLS": 0.0})
        if want <= launched(k)[0]: spec = k
    lo, hi = 3, A       # invariant: hi launches want
    while lo < hi:
        mid = ((lo + hi) // 2) | 1
        if mid >= hi: break
        s = dict(spec, A=mid, B=mid if B == A else max(2, (B * mid) // A))
        names, _ = launched(s)
        if want <= names: hi = mid
        else: lo = mid + 2
    if hi >= A and not spec.get("knobs"): return None
    s = dict(spec, A=hi, B=hi if B == A else max(2, (B * hi) // A))
    return s


def replay(path):
    cand, counts, per, forced = [], {}, {}, set()
    from sigkernel_amd import _lib
    todo = [s for _, s in reach_sweep.items() if s is not None]
    n_sweep = len(todo)
    for i, spec in enumerate(todo + extras()):
        spec = dict(spec); spec.pop("sweep_check", None)
        names, ppg = launched(spec)
        if i < n_sweep:
            for k, v in COUNTS.items(): counts[k] = counts.get(k, 0) + v
        b = budgeted(spec, ppg)
        if b is None:      # over the oracle's cap as the sweep makes it: the smallest batch with the same trace, or not a candidate
            s = smaller(spec, names)
            if s is None: continue
            names2, ppg = launched(s)
            b = budgeted(s, ppg)
            if b is None or not names <= names2: continue
            names = names2
            forced.add(len(cand))
        if spec["op"] == "truncated" and spec["order"] != -1: continue      # no oracle below the full order
        c = L.cells(b)
        keep = False
        if spec.get("wild") or spec["op"] in ("truncated_golden", "deriv"): forced.add(len(cand))
        for k in names:
            best = per.setdefault(k, [])
            if len(best) < KEEP_PER_INSTANCE or c < best[-1][0]:
                best.append((c, len(cand))); best.sort(); del best[KEEP_PER_INSTANCE:]; keep = True
        cand.append({"spec": b, "names": sorted(names), "cells": c, "ppg": ppg, "keep": keep})
        if i % 5000 == 0: print(i, "items replayed", flush=True)
    used = set(j for best in per.values() for _, j in best) | forced
    cand = [c for j, c in enumerate(cand) if j in used]
    print("%d items, %d candidates kept, %d instances seen" % (len(todo), len(cand), len(per)), flush=True)
    with open(path + ".counts", "w") as f:
        for k in sorted(counts): f.write("%d\t%s\n" % (counts[k], k))
    json.dump(cand, open(path, "w"))
    # smaller candidates of the expensive ones that some instance depends on
    need = set(j for best in per.values() for _, j in best[:2])
    keep_idx = sorted(used)
    extra = []
    for pos, j in enumerate(keep_idx):
        c = cand[pos]
        if j not in need or c["cells"] < SHRINK_ABOVE: continue
        s = smaller(c["spec"], set(c["names"]))
        if s is None: continue
        names, ppg = launched(s)
        b = budgeted(s, ppg)
        if b is not None and set(c["names"]) <= names:
            extra.append({"spec": b, "names": sorted(names), "cells": L.cells(b), "ppg": ppg, "smaller_of": reach_sweep.label(c["spec"])})
            print("smaller: %s -> %dx%d (%.2g -> %.2g cells)" % (reach_sweep.label(c["spec"]), b["A"], b["B"], c["cells"], L.cells(b)), flush=True)
            json.dump(cand + extra, open(path, "w"))
    json.dump(cand + extra, open(path, "w"))


def cover(path, table):
    cand = json.load(open(path))
    rows = table_rows()
    universe = set(m for _, _, m in rows)
    short = {m: inst for _, inst, m in rows}
    unit = {m: u for u, _, m in rows}
    for c in cand:
        wild = bool(c["spec"].get("wild"))
        f32_deriv = c["spec"]["op"] == "kgrad" and c["spec"]["dtype"] == "f32"      # (its k', k'' do not bound the solver: a "deriv" case does)
        c["can"] = set(k for k in c["names"] if k in universe and (wild or short[k] not in RESCUE_ONLY)
                       and not (f32_deriv and short[k].startswith("k_deriv_wave")))
    left, cases = set(universe), []
    for c in cand:      # the forced truncated cases first: each claims the k_trunc_sig instance it launches
        if c["spec"]["op"] == "truncated_golden":
            s = dict(c["spec"]); s["label"] = reach_sweep.label(s); s["cells"] = int(L.cells(s))
            s["claims"] = sorted(k for k in c["can"] if short[k].startswith("k_trunc_sig"))
            assert s["claims"], s["label"]
            cases.append(s)
            left -= set(s["claims"])
    cand = [c for c in cand if c["spec"]["op"] != "truncated_golden"]
    while left:
        best = max(cand, key=lambda c: (len(c["can"] & left) / max(c["cells"], 1.0), -c["cells"]))
        new = best["can"] & left
        if not new: break
        left -= new
        s = dict(best["spec"])
        s["label"] = reach_sweep.label(s) + (" wild" if s.get("wild") else "")
        s["cells"] = int(L.cells(s))
        s["claims"] = sorted(new)
        if s["dtype"] == "f32" and s["op"] in L.F32_STAGE_OPS and any(
                unit[m] in F32_STAGE_UNITS and "float" in short[m] for m in best["names"] if m in unit):
            s["f32_bound"] = L.measure_f32_bound(s, reach_sweep.inputs(s), 8)
        cases.append(s)
    cases.sort(key=lambda s: (s["op"], s["kind"], s["dtype"], s["dyadic"], s["label"]))
    print("%d cases cover %d of %d instances; uncovered: %s" % (len(cases), len(universe) - len(left), len(universe), sorted(short[k] for k in left)))
    head = open(table).read().split("# ---- generated")[0] if os.path.exists(table) else ""
    with open(table, "w") as f:
        f.write(head + "# ---- generated by tools/instance_cover.py: do not edit below this line\nCASES = ")
        f.write(pprint.pformat(cases, width=160, compact=True, sort_dicts=False) + "\n")
    return left


if __name__ == "__main__":
    a = sys.argv[1:]
    path = a[a.index("--replay") + 1] if "--replay" in a else (a[a.index("--cover") + 1] if "--cover" in a else "instance_replay.json")
    if "--cover" not in a: replay(path)
    if "--replay" not in a: cover(path, a[a.index("--table") + 1] if "--table" in a else os.path.join(ROOT, "tests", "instance_cases.py"))
