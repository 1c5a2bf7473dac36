#!/usr/bin/env python3
"""Every route of the public API once: static kernel x path dim x dyadic order x stencil x precision x lengths x operation (Gram,
symmetric Gram, paired batch -- each with and without a gradient --, the loss wrappers, the derivative Gram, few pairs of long paths),
then the calls whose kernel variants are gated by BATCH SIZE or by special lengths (work queue, age-rank shares, triangular blocks with
second-argument sums, bands on several waves, full multi-band efficiency, the derivative solver's unshifted bands).  The library counts
its own launches per kernel instance (sk_launch_trace, round 6: no profiler, no runtime log -- a minute natively): an instance no call
here launches is unreachable through sk_route_query / the exported entry points, and tests/test_abi.py fails on it.  usage:
    python tools/reach_sweep.py [first stride] [--out counts.txt]      (GPU box)   -> "count<TAB>device symbol" per instance launched
    python tools/variants.py --reached counts.txt > profiles/rNN_variants.txt     (CPU: the build's instances with their launches)
As a module: run(first=0, stride=1, check=0.0) -> {device symbol: launches}; check > 0: that share of the small Gram calls is compared
with the CPU oracle (values to 1e-9 / 1e-4 fp32, gradients to 1e-7 / 1e-3).

Every API call of the sweep is an ITEM: items() yields (label, spec), spec a plain dict (operation, static kernel, dtype, dyadic order,
stencil, batch and path shapes, a seed: inputs(spec) draws the call's tensors from it, execute(spec) makes the call and returns its
outputs).  run() executes the items in order; tools/instance_cover.py replays them one at a time and tests/instance_ledger.py compares
what execute() returns with the oracle."""
import itertools, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sigkernel_amd
from sigkernel_amd import _lib

DTYPES = {"f64": torch.float64, "f32": torch.float32}


def walk(g, A, M, D, dt):
    return (torch.cumsum(torch.randn(A, M, D, generator=g, dtype=torch.float64), 1) / np.sqrt(M * D)).to(dt).cuda()


class _Poly:
    """a user-defined static kernel (the generic route: Gram_matrix in torch -> sk_increments -> solver -> sk_increments_adjoint)"""
    def Gram_matrix(self, X, Y): return (1.0 + torch.einsum("amd,bnd->abmn", X, Y)) ** 2
    def batch_kernel(self, X, Y): return (1.0 + torch.einsum("amd,and->amn", X, Y)) ** 2


SHAPES = ((8, 8), (20, 33), (33, 20), (64, 64), (65, 65), (100, 90), (128, 128), (129, 40), (40, 129), (130, 129), (200, 40), (257, 161), (300, 520),
          (64, 512), (512, 64))

# operations of a spec: what the call returns, and which paths it takes from the two drawn batches X (A paths) and Y (B paths)
GRAD_OPS = ("gram_grad", "gram_sym_grad", "kernel_grad", "mmd_grad", "esr_grad")
PAIRED_OPS = ("kernel", "kernel_grad", "distance", "kernel_fn", "prefix_kernel")      # Y[:A]
BACKEND_OPS = ("exact_fwd", "exact_adj", "exact_deriv", "loss_weights", "adj_wild", "deriv")


def make_kernel(spec):
    kind, p = spec["kind"], spec.get("param")
    if kind == "linear":
        return sigkernel_amd.LinearKernel() if p is None else sigkernel_amd.LinearKernel(p)
    if kind == "rbf":
        return sigkernel_amd.RBFKernel(p)
    if kind == "rbf_id":
        return sigkernel_amd.RBF_ID_Kernel(p)
    assert kind == "poly", kind
    return _Poly()


def inputs(spec):
    """The call's tensors, on the CPU in the spec's dtype, from its seed alone: {"X", "Y"} and "gamma" (kgrad), "w" (a gradient's
    upstream weights, when the spec asks for random ones), "inc" (back-end calls)."""
    g = torch.Generator().manual_seed(int(spec["seed"]))
    dt, op = DTYPES[spec["dtype"]], spec["op"]
    A, B, M, N, D = (spec[k] for k in "ABMND")
    f64 = torch.float64
    if op in BACKEND_OPS:
        if op == "loss_weights":
            return {}
        if op == "adj_wild":      # increments of tame pairs and ONE with a legitimately large kernel (tests/test_gpu_parity.py): its residual
            inc = torch.randn(A, M, (N + 15) // 16 * 16, generator=g, dtype=f64) * 0.02      # exceeds the self-check's tolerance
            inc[spec["wild"][0]] = torch.randn(M, inc.shape[-1], generator=g, dtype=f64) * 0.9
            inc[..., N:] = 0      # (rows padded to whole 128-byte lines with zeros, as the library's own increment kernels leave them)
            return {"inc": inc.to(dt)}
        if op == "deriv":         # three increment arrays of A pairs, [3, A, M, N] (tests/test_derivatives.py)
            return {"inc": (torch.randn(3, A, M, (N + 15) // 16 * 16, generator=g, dtype=f64) * (1.5 / np.sqrt(M * N))).to(dt)}
        return {"inc": (torch.randn(A, M, 16, generator=g, dtype=f64) * 0.1).to(dt)}
    if op == "truncated_golden":      # a recorded call of the reference (tests/golden/truncated.npz): steps, levels, order and weights
        z = np.load(os.path.join(ROOT, "tests", "golden", "truncated.npz"))
        k = "c%02d_" % spec["fixture"]
        return {"X": torch.as_tensor(z[k + "X"]), "Y": torch.as_tensor(z[k + "Y"]), "sigma": torch.as_tensor(z[k + "sigma"])}
    if op in ("truncated", "truncated_paired"):      # steps, not points
        return {"X": (0.3 * torch.randn(A, M, D, generator=g)).to(dt), "Y": (0.3 * torch.randn(B, N, D, generator=g)).to(dt)}
    X = (torch.cumsum(torch.randn(A, M, D, generator=g, dtype=f64), 1) / np.sqrt(M * D)).to(dt)
    Y = (torch.cumsum(torch.randn(B, N, D, generator=g, dtype=f64), 1) / np.sqrt(N * D)).to(dt)
    if spec.get("wild"):      # walks twice as wide, x_a0 and y_b0 the same straight line: k(x_a0, y_b0) is legitimately large (1e6 and
        a0, b0 = spec["wild"]  # more), every other pair tame -- ordinary finite input (tests/test_configs.py, _one_wild_pair)
        line = (torch.arange(M, dtype=f64)[:, None] * 0.6 * torch.ones(1, D, dtype=f64) / np.sqrt(D)).to(dt)
        X, Y = X * 2, Y * 2
        X[a0], Y[b0] = line, line.clone()
    t = {"X": X, "Y": Y}
    if op == "kgrad":
        t["gamma"] = torch.randn(A, M, D, generator=g, dtype=f64).to(dt)
    if spec.get("w") == "randn":
        t["w"] = torch.randn(A, A if "sym" in op else (1 if op == "kernel_grad" else B), generator=g, dtype=f64)
    return t


class _Knobs:
    """the spec's route knobs for the length of one call: routes.<name>, module attributes of sigkernel (the cost table's overrides)"""
    def __init__(self, spec): self.knobs, self.was = spec.get("knobs") or {}, []
    def __enter__(self):
        from sigkernel_amd import sigkernel as S
        for name, v in self.knobs.items():
            if name == "workspace_bytes": continue
            obj, attr = (sigkernel_amd.routes, name[7:]) if name.startswith("routes.") else (S, name)
            self.was.append((obj, attr, getattr(obj, attr))); setattr(obj, attr, v)
    def __exit__(self, *a):
        for obj, attr, v in reversed(self.was): setattr(obj, attr, v)


def execute(spec, t=None):
    """Make the spec's call on the GPU -> {output name: tensor}: "value" (Gram matrix, paired values, loss, prefix grid or slice),
    "grad" (of the first batch, under the spec's weights), "k" / "k1" / "k2" (kgrad), "W" (exact_adj)."""
    t = inputs(spec) if t is None else t
    op, d = spec["op"], spec["dyadic"]
    dt = DTYPES[spec["dtype"]]
    dev = {k: v if v.is_cuda else v.cuda() for k, v in t.items()}
    if op in BACKEND_OPS:
        be = _lib.get_backend()
        if op == "loss_weights":
            return {"value": be.loss_weights(spec["A"], spec["B"], torch.ones((), dtype=torch.float64).cuda(), torch.device("cuda"))}
        inc = dev["inc"][..., :spec["N"]]
        if op == "adj_wild":
            k, W = be.solve_adj(inc, d)[:2]
            return {"value": k, "W": W}
        if op == "deriv":
            k, k1, k2 = be.solve_deriv(inc, d)
            return {"k": k, "k1": k1, "k2": k2}
        if op == "exact_fwd":
            return {"value": be.solve_fwd(inc, d, flags=_lib.FLAG_EXACT)}
        if op == "exact_adj":
            k, W = be.solve_adj(inc, d, flags=_lib.FLAG_EXACT)[:2]
            return {"value": k, "W": W}
        k, k1, k2 = be.solve_deriv(torch.stack([inc, inc, inc]), d, flags=_lib.FLAG_EXACT)
        return {"k": k, "k1": k1, "k2": k2}
    X, Y, A = dev["X"], dev["Y"], spec["A"]
    if op == "truncated":
        return {"value": sigkernel_amd.truncated_sig_kernel(X, Y, spec["L"], order=spec["order"])}
    if op == "truncated_paired":      # the same instances in their paired mode: the pairs (X[p], Y[p])
        return {"value": sigkernel_amd.truncated_sig_kernel_paired(X, Y[:A], spec["L"], order=spec["order"])}
    if op == "truncated_golden":
        sg = dev["sigma"]
        return {"value": sigkernel_amd.truncated_sig_kernel(X, Y, spec["L"], sigma=float(sg) if sg.dim() == 0 else sg.cpu(), order=spec["order"])}
    with _Knobs(spec):
        sk = sigkernel_amd.SigKernel(make_kernel(spec), d, _naive_solver=bool(spec.get("naive")), **(
            {"workspace_bytes": spec["knobs"]["workspace_bytes"]} if "workspace_bytes" in (spec.get("knobs") or {}) else {}))
        if op in PAIRED_OPS: Y = Y[:A]
        if op == "scoring_rule": Y = Y[:1]
        if op == "gram": return {"value": sk.compute_Gram(X, Y)}
        if op == "gram_sym": return {"value": sk.compute_Gram(X, X, sym=True)}
        if op == "kernel": return {"value": sk.compute_kernel(X, Y)}
        if op == "kernel_fn":
            F = spec["F"]
            return {"value": sk.compute_kernel(X.reshape(A, spec["M"], spec["D"] // F, F), Y.reshape(A, spec["N"], spec["D"] // F, F))}
        if op in ("mmd", "scoring_rule", "distance"): return {"value": getattr(sk, "compute_" + op)(X, Y)}
        if op == "kgrad":
            k, k1, k2 = sk.compute_kernel_and_derivatives_Gram(X, Y, dev["gamma"])
            return {"k": k, "k1": k1, "k2": k2}
        if op in ("prefix_gram", "prefix_kernel"):
            call = sk.compute_Gram_prefixes if op == "prefix_gram" else sk.compute_kernel_prefixes
            return {"value": call(X, Y) if spec["nodes"] == "all" else call(X, Y, nodes=spec["nodes"])}
        assert op in GRAD_OPS, op
        Xg = X.clone().requires_grad_(True)
        if op == "gram_grad": v = sk.compute_Gram(Xg, Y)
        elif op == "gram_sym_grad": v = sk.compute_Gram(Xg, Xg, sym=True)
        elif op == "kernel_grad": v = sk.compute_kernel(Xg, Y)
        elif op == "mmd_grad": v = sk.compute_mmd(Xg, Y)
        else: v = sk.compute_expected_scoring_rule(Xg, Y)
        if "w" in dev and v.dim() > 0:
            (v * dev["w"].to(dt).reshape(v.shape)).sum().backward()
        else:
            v.sum().backward()
        return {"value": v.detach(), "grad": Xg.grad}


def _spec(op, kind, param, dt, d, naive, A, B, M, N, D, seed, **more):
    s = dict(op=op, kind=kind, param=param, dtype="f64" if dt in (torch.float64, "f64") else "f32", dyadic=d, naive=bool(naive), A=A, B=B, M=M, N=N, D=D,
             seed=seed)
    s.update(more)
    return s


def label(s):
    extra = "".join(" %s=%s" % (k, s[k]) for k in ("nodes", "L", "order", "F", "fixture") if k in s)
    return "%s %s %s d%d%s %dx%d %dx%d D%d%s" % (s["op"], s["kind"], s["dtype"], s["dyadic"], " naive" if s["naive"] else "", s["A"], s["B"], s["M"], s["N"], s["D"], extra)


def items(first=0, stride=1):
    """(label, spec) for every API call of the sweep, in the order run() makes them.  The calls of one shape combination share a seed:
    the same paths, as one training step would pass them to several calls."""
    seed = [0]

    def combo():
        seed[0] += 1
        return seed[0]

    def it(op, kind, param, dt, d, naive, A, B, M, N, D, sd, **more):
        s = _spec(op, kind, param, dt, d, naive, A, B, M, N, D, sd, **more)
        return label(s), s
    f64, f32 = torch.float64, torch.float32
    shapes = SHAPES[first::stride]
    for kname, D, d, naive, dt in itertools.product(("linear", "rbf"), (1, 3, 4, 5, 8, 9, 16, 20), (0, 1, 2, 3), (False, True), (f64, f32)):
        p = 0.9 if kname == "rbf" else None
        for M, N in shapes:
            if d == 3 and max(M, N) > 130: continue
            a = (kname, p, dt, d, naive, 3, 4, M, N, D, combo())
            yield it("gram", *a); yield it("gram_sym", *a); yield it("kernel", *a)
            yield it("gram_grad", *a, sweep_check=True)
            yield it("gram_sym_grad", *a); yield it("kernel_grad", *a)
            if M == N:
                yield it("mmd_grad", *a); yield it("mmd", *a); yield it("scoring_rule", *a); yield it("distance", *a); yield it("esr_grad", *a)
            if not naive and max(M, N) <= 130 and d <= 2:
                yield it("kgrad", *a)
            yield None, None      # (one shape combination done)
    # a user-defined static kernel and the bit-exact kernels (the stored-grid rescue of the streaming adjoint runs them on exploding pairs)
    for dt in (f64, f32):
        for d in (0, 1):
            a = ("poly", None, dt, d, False, 3, 4, 20, 17, 3, combo())
            yield it("gram", *a); yield it("gram_grad", *a); yield it("kernel_grad", *a); yield it("kgrad", *a)
    for dt in (f64, f32):
        a = ("none", None, dt, 1, False, 6, 1, 9, 11, 0, combo())      # inc [6, 9, 16][..., :11]
        yield it("exact_fwd", *a); yield it("exact_adj", *a); yield it("exact_deriv", *a)
    if first == 0:
        for x in gated_items(combo, it): yield x


def gated_items(combo, it):
    """The variants a 3 x 4 batch cannot show."""
    f64, f32 = torch.float64, torch.float32
    # big batches (work queue, age-rank shares, triangular blocks), long paths (bands on several waves)
    for kname, D, d, A, M in (("linear", 8, 1, 512, 128), ("rbf", 4, 2, 512, 64), ("rbf", 3, 1, 128, 64), ("rbf", 16, 2, 64, 512), ("linear", 4, 0, 8, 2048),
                              ("rbf", 3, 1, 4, 1500)):
        a = (kname, 1.0 if kname == "rbf" else None, f32 if D == 16 else f64, d, False, A, A, M, M, D, combo())
        yield it("gram", *a); yield it("gram_sym", *a)
        if M <= 512:
            yield it("mmd_grad", *a)
    # the symmetric Gram WITH a gradient and enough grid cells for the blocked triangle (sym_min_cells, 5e9): second-argument sums of the
    # one-band RBF adjoint -- one coarse row per lane on fewer than 64 lanes at dyadic 1 / 2 (paths of <= 32 points), two on the full
    # wave at dyadic 0 (65..128 points), and the full-wave forms of BASELINE configs[3]'s shape ...
    for d, M, A in ((1, 32, 1280), (2, 32, 640), (0, 128, 640), (0, 40, 2048), (1, 64, 640), (2, 64, 320)):
        yield it("gram_sym_grad", "rbf", 0.8, f64, d, False, A, A, M, M, 3, combo(), free=True)
    # ... and of the streaming route (sk_static_adjoint2: dyadic 3 is beyond every fused kernel), path dims 4 / 8 / 16 / 32 wide
    for kname, D, dt in itertools.product(("rbf", "linear"), (3, 8, 12, 20), (f64, f32)):
        if kname == "linear" and D > 8: continue      # (no second-argument kernel: such calls solve all pairs)
        yield it("gram_sym_grad", kname, 0.8 if kname == "rbf" else None, dt, 3, False, 1024, 1024, 10, 10, D, combo(), free=True)
    # long first paths against short second ones with a gradient, LinearKernel: the one-band adjoint on (y, x) with second-argument sums,
    # on the full wave and on fewer lanes at each dyadic order (the 3 x 4 sweep above has no second paths of <= 33 points at dyadic 2)
    for d, (M, N) in itertools.product((0, 1, 2), ((200, 20), (300, 100), (400, 60))):
        yield it("gram_grad", "linear", None, f64, d, False, 5, 7, M, N, 6, combo())
    # ... and RBFKernel: the one-band adjoint's second-argument sums INSTEAD of the first-argument ones (dim 3: every dyadic order, two
    # rows per lane at dyadic 1; dim 6: dyadic 0 and 1)
    for D, d, (M, N) in itertools.product((3, 6), (0, 1, 2), ((200, 20), (300, 100), (400, 60))):
        if (D == 6 and (d == 2 or (d == 1 and N > 64))) or (d == 2 and N > 64): continue
        yield it("gram_grad", "rbf", 0.9, f64, d, False, 5, 7, M, N, D, combo())
    # paired batches of more pairs than resident lane groups, with a gradient: several pairs per lane group in the linear one-band
    # adjoint (PAIRED), on the full wave and on fewer lanes
    for kname, (d, M, Pn) in itertools.product(("linear", "rbf"), ((0, 128, 5000), (0, 40, 9000), (1, 128, 5000), (1, 40, 9000), (2, 64, 5000), (2, 30, 9000))):
        yield it("kernel_grad", kname, 0.9 if kname == "rbf" else None, f64, d, False, Pn, Pn, M, M, 4, combo(), free=True)
    # paths of 25..32 dims with a gradient (the static adjoint's 32-dim instances; the sweep above has 20 dims: the 24-dim ones)
    for kname, dt, (M, N) in itertools.product(("rbf", "linear"), (f64, f32), ((40, 50), (30, 140))):
        yield it("gram_grad", kname, 0.9 if kname == "rbf" else None, dt, 1, False, 3, 4, M, N, 30, combo())
    # paths of more than 32 dims, with a gradient: the K-looped matrix-core node Gram (k_static_wide_mfma: linear / rbf increments and
    # the rbf chain rule's first pass), through a kernel of function-valued paths too
    for kname, dt in itertools.product(("linear", "rbf"), (f64, f32)):
        yield it("gram_grad", kname, 0.9 if kname == "rbf" else None, dt, 1, False, 3, 5, 40, 30, 40, combo())
    yield it("kernel_fn", "rbf_id", 2.0, f64, 1, False, 3, 3, 20, 25, 48, combo(), F=3)
    # paths of 9..32 dims with a gradient: the tiled static adjoints (LinearKernel 16 / 24 / 32 dims, RBFKernel 24 / 32; second paths of
    # <= 64 and of 65..128 points)
    for kname, D, dt, N in itertools.product(("linear", "rbf"), (12, 20, 30), (f64, f32), (50, 100)):
        yield it("gram_grad", kname, 0.9 if kname == "rbf" else None, dt, 1, False, 3, 4, 40, N, D, combo())
    # the fused derivative solver on first paths of 64 k + 1 points (bands that need no shifted lanes) against second paths of 126 points
    # and more; its in-LDS band boundary (two bands, 126..157-point second paths)
    for kname, d, (M, N) in itertools.product(("linear", "rbf"), (0, 1, 2), ((65, 130), (129, 140), (129, 200), (100, 140))):
        yield it("kgrad", kname, 0.8 if kname == "rbf" else None, f64, d, False, 3, 4, M, N, 3, combo())
    # the unfused derivative solver on fp32 increments of several full-wave bands (a user-defined static kernel takes it at any size)
    for d in (0, 1):
        yield it("kgrad", "poly", None, f32, d, False, 2, 2, 300, 520, 3, combo())
    # full bands: where the multi-band forward is the default for 9..16 staged fp64 dims of the RBF kernel (sweep efficiency >= 0.85)
    for d, D in itertools.product((0, 1, 2), (9, 16)):
        a = ("rbf", 0.8, f64, d, False, 3, 4, 256, 200, D, combo())
        yield it("gram", *a); yield it("kernel", *a)
    # prefix grids: every instance of the fused prefix kernel (kind x dyadic order x stencil x output dtype), Gram and paired, in each of
    # its four store modes (the full grid, its diagonal, last row, last column), and the route everything else takes (increments + the
    # streaming solver's grid, the slice taken from it)
    for kname, d, naive, dt in itertools.product(("linear", "rbf"), (0, 1, 2), (False, True), (f64, f32)):
        a = (kname, 0.9 if kname == "rbf" else None, dt, d, naive, 3, 4, 33, 20, 5, combo())
        for nodes in ("all", "diagonal", "last_row", "last_col"):      # the slice store modes of the same instances
            yield it("prefix_gram", *a, nodes=nodes); yield it("prefix_kernel", *a, nodes=nodes)
    a = ("linear", None, f64, 1, False, 3, 4, 20, 17, 12, combo())
    yield it("prefix_gram", *a, nodes="all"); yield it("prefix_gram", *a, nodes="diagonal")
    # truncated_sig_kernel: both instances of k_trunc_sig (order 1, two rows per lane; the general order), direct and on (y, x), each output dtype
    for dt, (M, N, L, order) in itertools.product((f64, f32), ((100, 40, 6, 1), (50, 30, 5, -1), (40, 30, 4, 2), (200, 60, 4, 3))):
        yield it("truncated", "none", None, dt, 0, False, 5, 7, M, N, 6, combo(), L=L, order=order)
    # an exported entry point the host layer has no call of any more (the one-launch loss route carries its weights from the forward)
    yield it("loss_weights", "none", None, f64, 0, False, 5, 7, 0, 0, 0, combo())
    # truncated_sig_kernel_paired: the paired mode of k_trunc_sig's general instance (a launch-time mode: no instance of its own)
    yield it("truncated_paired", "none", None, f64, 0, False, 5, 7, 40, 30, 6, combo(), L=4, order=2)


def run(first=0, stride=1, check=0.0, verbose=True):
    _lib.launch_trace(True)
    _lib.launch_counts(reset=True)
    rng = np.random.default_rng(0)
    O = None
    if check > 0:
        from oracle import oracle as O      # noqa: N811 -- the checker (test infrastructure), never the thing measured
    n = checked = 0
    worst = 0.0
    last_seed, t, K = None, None, None
    for lab, spec in items(first, stride):
        if spec is None:
            n += 1
            if verbose and n % 500 == 0: print(n, "combinations", flush=True)
            continue
        if spec["seed"] != last_seed or spec["op"] == "kgrad":
            last_seed, t = spec["seed"], {k: v.cuda() for k, v in inputs(spec).items()}      # (on the device once per shape combination)
        out = execute(spec, t)
        if spec["op"] == "gram": K = out["value"]
        if spec.get("sweep_check") and O is not None and max(spec["M"], spec["N"]) <= 130 and spec["dyadic"] <= 2 and rng.random() < check:
            k, d, naive = make_kernel(spec), spec["dyadic"], spec["naive"]
            X, Y = t["X"].cpu(), t["Y"].cpu()
            tol = (1e-9, 1e-7) if spec["dtype"] == "f64" else (1e-4, 1e-3)
            want = O.gram_forward(X, Y, k, d, naive=naive)
            e = float(np.max(np.abs(K.double().cpu().numpy() - want)) / np.max(np.abs(want)))
            assert e <= tol[0], ("value", lab, e)
            gw = O.gram_grad_weighted(X, Y, np.ones((spec["A"], spec["B"])), k, d, naive=naive)
            eg = float(np.max(np.abs(out["grad"].double().cpu().numpy() - gw)) / np.max(np.abs(gw)))
            assert eg <= tol[1], ("gradient", lab, eg)
            worst = max(worst, e / tol[0], eg / tol[1])
            checked += 1
        if spec.get("free"):      # (the big batches: return their blocks before the next one)
            del out
            torch.cuda.empty_cache()
    torch.cuda.synchronize()
    counts = _lib.launch_counts()
    if verbose:
        print("%d shape combinations swept, %d Gram matrices checked against the oracle (worst error / tolerance %.2g), %d kernel instances launched"
              % (n, checked, worst, len(counts)))
    return counts


if __name__ == "__main__":
    out = None
    if "--out" in sys.argv:
        i = sys.argv.index("--out"); out = sys.argv[i + 1]; del sys.argv[i:i + 2]
    first, stride = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (0, 1)
    counts = run(first, stride)
    if out:
        with open(out, "w") as f:
            for name in sorted(counts):
                f.write("%d\t%s\n" % (counts[name], name))
