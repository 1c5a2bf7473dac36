"""The instance ledger's helpers: traced(fn), one oracle adapter per operation of tests/instance_cases.py (expected values from
oracle/oracle.py alone -- never from the library's torch restatements or its streaming route), and a comparator that cannot average a
fault away (per element for values, per path for gradients, the worst index reported).

A case's spec is the dict tools/reach_sweep.py defines (operation, static kernel, dtype, dyadic order, stencil, shapes, seed, knobs):
reach_sweep.inputs(spec) draws the tensors, reach_sweep.execute(spec) makes the call on the GPU, expected(spec, tensors) is what the
oracle says the call returns, for the same fp32-rounded inputs in fp64."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import oracle as O  # noqa: E402

CELL_CAP = 2e10                    # oracle work of one case, fine-grid cells
F32_ULPS2 = 2.0 ** -22             # two fp32 ulps of the per-element scale: both sides round once, the fp64 error may cross one boundary
# fp64 tolerances by output: tools/fuzz_api.py (values, gradients, k, k', k''), README (truncated)
TOL64 = {"value": 1e-10, "grad": 1e-8, "k": 1e-10, "k1": 1e-6, "k2": 1e-3, "W": 0.0}
RESCUE_GRAD_TOL = 2e-8             # 2 * ADJ_RESIDUAL_TOL (tests/test_configs.py: the pairs a rescuing sweep keeps)
TRUNCATED_TOL = 1e-12


def traced(fn):
    """fn() with the library counting its launches from zero -> (result, set of the mangled names of the instances launched); the
    trace's previous state is restored."""
    from sigkernel_amd import _lib
    was = _lib.launch_trace(True)
    try:
        _lib.launch_counts(reset=True)
        out = fn()
        torch.cuda.synchronize()
        counts = _lib.launch_counts(reset=True)
    finally:
        _lib.launch_trace(was)
    return out, set(k.split(".kd")[0] for k, v in counts.items() if v > 0)


# ------------------------------------------------------------------------------------------------------------------- tolerances
def tolerance(spec, name):
    """The bound for output `name` of the case: the fp64 tolerance, plus two fp32 ulps where the call's I/O is fp32 (its arithmetic
    fp64).  A case whose route hands fp32 arrays from one launch to the next carries a measured allowance for that on top
    (spec["f32_bound"][name]: the source lines, the distance of expected_f32_stage from the all-fp64 oracle, and 4 x that distance)."""
    if spec["op"] in ("exact_fwd", "exact_adj", "exact_deriv"):
        return 0.0
    t = TRUNCATED_TOL if spec["op"] in ("truncated", "truncated_golden") else TOL64[name]
    if spec["op"] == "deriv":      # the solver on given increments: no finite difference in between, the bar of the values
        t = TOL64["value"]
    if name in ("grad", "W") and spec.get("wild"):
        t = RESCUE_GRAD_TOL
    if spec["dtype"] == "f32":
        t += F32_ULPS2
        if spec.get("f32_bound") and name in spec["f32_bound"]:      # the fp32 stage's allowance on top of the output's rounding
            t += float(spec["f32_bound"][name]["tol"])
    return t


# ------------------------------------------------------------------------------------------------------------------- comparator
def compare_values(got, want, tol):
    """per element |got - want| <= tol * max(|want|, 1); non-finite entries must match exactly (tol 0: bit equality of the values).
    -> (ok, worst index, worst error in units of the bound's scale)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False, None, float("inf")
    if got.size == 0:
        return True, None, 0.0
    fin = np.isfinite(want)
    same = np.where(fin, np.isfinite(got), (got == want) | (np.isnan(got) & np.isnan(want)))
    with np.errstate(invalid="ignore"):
        err = np.where(fin & np.isfinite(got), np.abs(got - want) / np.maximum(np.abs(want), 1.0), 0.0)
    err = np.where(same, err, np.inf)
    i = np.unravel_index(int(np.argmax(err)), err.shape)
    return bool(err[i] <= tol), tuple(int(j) for j in i), float(err[i])


def compare_grads(got, want, tol):
    """per path (axis 0): max |got - want| over the path <= tol * max |want| over that path; non-finite entries must match exactly.
    -> (ok, worst (path, point, channel), worst relative error)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False, None, float("inf")
    if got.size == 0:
        return True, None, 0.0
    fin = np.isfinite(want)
    same = np.where(fin, np.isfinite(got), (got == want) | (np.isnan(got) & np.isnan(want)))
    with np.errstate(invalid="ignore"):
        diff = np.where(fin & np.isfinite(got), np.abs(got - want), 0.0)
    flat = (slice(None),) + (None,) * (want.ndim - 1)
    norm = np.maximum(np.max(np.where(fin, np.abs(want), 0.0).reshape(want.shape[0], -1), axis=1), 1e-300)[flat]
    err = np.where(same, diff / norm, np.inf)
    i = np.unravel_index(int(np.argmax(err)), err.shape)
    return bool(err[i] <= tol), tuple(int(j) for j in i), float(err[i])


def compare(name, got, want, tol):
    """gradients per path; so are an adjoint's weights W (per pair) unless the bound is bit equality"""
    return compare_grads(got, want, tol) if name == "grad" or (name == "W" and tol > 0) else compare_values(got, want, tol)


# ------------------------------------------------------------------------------------------------------------------- oracle adapters
class _Paired:
    """The oracle's Gram route on pairs with batch_kernel's scaling (tools/fuzz_api.py): a (P, 1) Gram matrix of P pairs."""

    def __init__(self, k):
        self.k = k

    def Gram_matrix(self, X, Y):
        return self.k.batch_kernel(X, Y)[:, None]


def _rows(spec, A):
    return list(range(A))


def _weights(spec, t, shape):
    return t["w"].double().numpy().reshape(shape) if "w" in t else np.ones(shape)


def _wxx(A):
    return (1.0 - np.eye(A)) / (A * (A - 1.0))


def expected(spec, t, nthreads=1):
    """{output name: numpy array} the oracle gives for the case;
    "grad" may be a tuple of arrays: the call may return any of them (the symmetric Gram's two equivalent rules)."""
    import reach_sweep
    op, d, nv, nt = spec["op"], spec["dyadic"], bool(spec.get("naive")), nthreads
    A, B, M, N = spec["A"], spec["B"], spec["M"], spec["N"]
    if op == "loss_weights":
        w = np.empty((A, A + B))
        w[:, :A] = 2.0 * _wxx(A) if A > 1 else 0.0
        w[:, A:] = -2.0 / (A * B)
        return {"value": w.reshape(-1)}
    if op in ("exact_fwd", "exact_adj", "exact_deriv", "adj_wild", "deriv"):
        inc = t["inc"][..., :N].double().numpy()
        if op == "adj_wild":
            k, W = O.adjoint_coarse(inc, d, nthreads=nt)
            return {"value": k, "W": W}
        if op == "deriv":
            return dict(zip(("k", "k1", "k2"), O.solve_deriv_coarse(inc[0], inc[1], inc[2], d, nthreads=nt)))
        if op == "exact_fwd":
            return {"value": O.solve_coarse(inc, d)}
        if op == "exact_adj":
            k, W = O.adjoint_coarse(inc, d)
            return {"value": k, "W": W}
        return dict(zip(("k", "k1", "k2"), O.solve_deriv_coarse(inc, inc, inc, d)))
    if op == "truncated_golden":      # what the reference returned for this recorded call
        z = np.load(os.path.join(ROOT, "tests", "golden", "truncated.npz"))
        return {"value": np.asarray(z["c%02d_K" % spec["fixture"]], dtype=np.float64)}
    X, Y = t["X"].double(), t["Y"].double()
    if op == "truncated":      # the tensor-level Chen evaluation: defined for the full order only
        from test_truncated_host import chen_kernel
        assert min(spec["L"], spec["L"] if spec["order"] < 1 else spec["order"]) == spec["L"], "no oracle below the full order"
        return {"value": chen_kernel(X.numpy(), Y.numpy(), spec["L"], 1.0)}
    k = reach_sweep.make_kernel(spec)
    R = _rows(spec, A)
    if op in reach_sweep.PAIRED_OPS:
        Y = Y[:A]
    if op in ("gram", "gram_grad"):
        out = {"value": O.gram_forward(X, Y, k, d, naive=nv, nthreads=nt)}
        if op == "gram_grad":
            out["grad"] = O.gram_grad_weighted(X[R], Y, _weights(spec, t, (A, B))[R], k, d, naive=nv, nthreads=nt)
        return out
    if op in ("gram_sym", "gram_sym_grad"):
        out = {"value": O.gram_forward(X, X, k, d, naive=nv, nthreads=nt)}
        if op == "gram_sym_grad":      # the reference's 2x rule (all pairs) or first plus second argument (the triangle)
            w = _weights(spec, t, (A, A))
            g1 = O.gram_grad_weighted(X[R], X, w[R], k, d, naive=nv, nthreads=nt)
            g2 = g1 if np.array_equal(w, w.T) else O.gram_grad_weighted(X[R], X, w.T[R].copy(), k, d, naive=nv, nthreads=nt)
            out["grad"] = (2.0 * g1, g1 + g2)
        return out
    if op in ("kernel", "kernel_grad", "kernel_fn"):
        if op == "kernel_fn":
            F = spec["F"]
            X, Y = X.reshape(A, M, spec["D"] // F, F), Y.reshape(A, N, spec["D"] // F, F)
        out = {"value": O.gram_forward(X, Y, _Paired(k), d, naive=nv, nthreads=nt)[:, 0]}
        if op == "kernel_grad":
            out["grad"] = O.gram_grad_weighted(X[R], Y[R], _weights(spec, t, (A, 1))[R], _Paired(k), d, naive=nv, nthreads=nt)
        return out
    if op == "distance":      # tools/fuzz_api.py:155
        kk = [O.gram_forward(P, Q, _Paired(k), d, naive=nv, nthreads=nt).mean() for P, Q in ((X, X), (Y, Y), (X, Y))]
        return {"value": np.array(kk[0] + kk[1] - 2.0 * kk[2])}
    if op in ("mmd", "mmd_grad", "scoring_rule", "esr_grad"):      # tools/fuzz_api.py:158-178
        if op == "scoring_rule":
            Y = Y[:1]
        Bv = Y.shape[0]
        Kxx = O.gram_forward(X, X, k, d, naive=nv, nthreads=nt)
        Kxy = O.gram_forward(X, Y, k, d, naive=nv, nthreads=nt)
        want = float((Kxx * _wxx(A)).sum() - 2.0 * Kxy.mean())
        if op in ("mmd", "mmd_grad"):
            Kyy = O.gram_forward(Y, Y, k, d, naive=nv, nthreads=nt)
            want += float((Kyy.sum() - np.trace(Kyy)) / (Bv * (Bv - 1.0)))
        out = {"value": np.array(want)}
        if op in ("mmd_grad", "esr_grad"):
            out["grad"] = (2.0 * O.gram_grad_weighted(X[R], X, _wxx(A)[R], k, d, naive=nv, nthreads=nt)
                           + O.gram_grad_weighted(X[R], Y, np.full((len(R), Bv), -2.0 / (A * Bv)), k, d, naive=nv, nthreads=nt))
        return out
    if op == "kgrad":
        out = dict(zip(("k", "k1", "k2"), O.kgrad(X, Y, t["gamma"].double(), k, d, nthreads=nt)))
        if spec["dtype"] == "f32" and spec.get("f32_bound"):
            # the finite differences of fp32 node values amplify their rounding by 1 / eps^2: k' and k'' are compared on the increments
            # the solver really receives (the fp32 restatement's), at the derived bound; k keeps the all-fp64 oracle and its allowance
            st = expected_f32_stage(spec, t, nt)
            out["k1"], out["k2"] = st["k1"], st["k2"]
        return out
    if op in ("prefix_gram", "prefix_kernel"):      # the oracle's full grid at the coarse nodes (tests/test_gpu_prefixes.py)
        G = (k.Gram_matrix(X, Y) if op == "prefix_gram" else k.batch_kernel(X, Y)).numpy()
        r = 1 << d
        grid = O.solve_coarse(O.increments(G), d, nv, want_grid=True, nthreads=nt)[1][..., ::r, ::r]
        nodes = spec["nodes"]
        if nodes == "diagonal":
            grid = np.diagonal(grid, axis1=-2, axis2=-1)
        elif nodes == "last_row":
            grid = grid[..., -1, :]
        elif nodes == "last_col":
            grid = grid[..., :, -1]
        return {"value": np.ascontiguousarray(grid)}
    raise ValueError("no oracle adapter for operation %r" % op)


F32_STAGE_OPS = ("gram", "gram_sym", "kernel", "gram_grad", "gram_sym_grad", "kernel_grad", "kgrad")
F32_STAGE_SOURCE = {      # the fp32 stages of a route, by the key a case's "f32_bound" carries
    "deriv_fused": "sigkernel_amd/sigkernel.py:798 (X + eps gamma formed in fp32); csrc/sk_static.hip:224 (node values, their 1/eps scaling and "
                   "the 4-corner differences in fp32); sigkernel_amd/_lib.py:1374 (the three increment arrays fp32)",
    "deriv_user": "sigkernel_amd/sigkernel.py:798, :811-813 (X + eps gamma and the three Gram matrices by torch in fp32); csrc/sk_increments.hip:120 "
                  "(scaling and differences in fp32); sigkernel_amd/_lib.py:1357 (the increment arrays fp32)",
    "stream_rbf": "sigkernel_amd/_lib.py:450 (increments stored fp32); solve_adj returns W in the increments' dtype",
    "stream_linear": "sigkernel_amd/_lib.py:450 (increments stored fp32), :1107-1125 (T = sum_b w W @ dy and its scatter into the gradient in fp32)",
    "stream_user": "sigkernel_amd/_lib.py:428 (the Gram matrix by torch in fp32, increments stored fp32), :1185 (dL/dG fp32, torch's fp32 backward)"}


def f32_stage_key(spec):
    user = spec["kind"] == "poly"
    if spec["op"] == "kgrad":
        return "deriv_user" if user else "deriv_fused"
    return "stream_user" if user else "stream_" + spec["kind"]


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def expected_f32_stage(spec, t, nthreads=1):
    """The reference-side restatement of the fp32 stages of a streamed fp32 call: every array the route hands from one launch to the
    next in the inputs' dtype (the lines of F32_STAGE_SOURCE) is rounded to fp32 here, a user-defined static kernel is evaluated and
    differentiated by torch in fp32, the perturbed paths of the derivative Gram are formed in fp32; everything else is the oracle in
    fp64, and the outputs are NOT rounded.  Same outputs as expected()."""
    import reach_sweep
    op, d, nv, nt = spec["op"], spec["dyadic"], bool(spec.get("naive")), nthreads
    A, B = spec["A"], spec["B"]
    assert spec["dtype"] == "f32" and op in F32_STAGE_OPS
    k, user = reach_sweep.make_kernel(spec), spec["kind"] == "poly"
    Xf, Yf = t["X"].float(), t["Y"].float()
    if op in reach_sweep.PAIRED_OPS:
        Yf = Yf[:A]
    kk = _Paired(k) if op in ("kernel", "kernel_grad") else k

    def gram(Xa, Ya):      # the static Gram matrix: torch in fp32 for a user-defined kernel, the library's fp64 arithmetic otherwise
        return kk.Gram_matrix(Xa, Ya) if user else kk.Gram_matrix(Xa.double(), Ya.double())

    if op == "kgrad":
        eps = 1e-4
        gf = t["gamma"].float()
        X1, X2 = Xf + eps * gf, Xf + 2. * eps * gf
        # node values rounded to fp32, then the reference's scaling, the 4-corner differences and their sums in fp32, in the kernels'
        # operand order: ((G11 + G00) - G10) - G01, the differenced arrays added left to right
        G0, G1, G2 = (gram(Xa, Yf).float() for Xa in (Xf, X1, X2))
        c1, c2, c3 = (torch.tensor(v, dtype=torch.float32) for v in (1. / eps, 2. / eps, 1. / eps ** 2))

        def inc4(G):
            return ((G[..., 1:, 1:] + G[..., :-1, :-1]) - G[..., 1:, :-1]) - G[..., :-1, 1:]
        d1, d2 = -c1 * G0, c1 * G1
        dd1, dd2, dd3 = -c1 * d1, -c2 * d2, c3 * G2
        inc, inc_d, inc_dd = inc4(G0), inc4(d1) + inc4(d2), (inc4(dd1) + inc4(dd2)) + inc4(dd3)
        assert inc.dtype == inc_dd.dtype == torch.float32
        return dict(zip(("k", "k1", "k2"), O.solve_deriv_coarse(inc.double().numpy(), inc_d.double().numpy(), inc_dd.double().numpy(), d, nthreads=nt)))

    def forward(Xa, Ya):
        with torch.no_grad():
            return O.solve_coarse(_f32(O.increments(gram(Xa, Ya).double().numpy())), d, nv, nthreads=nt)

    def gradient(Xa, Ya, w):
        Xa = (Xa if user else Xa.double()).clone().requires_grad_(True)
        with torch.enable_grad():
            G = gram(Xa, Ya)
        _, W = O.adjoint_coarse(_f32(O.increments(G.detach().double().numpy())), d, nv, nthreads=nt)
        if spec["kind"] == "linear":      # T = sum_b w W @ dy and its scatter into the gradient, in the inputs' dtype (_lib.py:1107-1125)
            Ws = torch.from_numpy(_f32(W)).float() * torch.from_numpy(np.asarray(w, dtype=np.float64)).float()[:, :, None, None]
            dY = Ya[:, 1:] - Ya[:, :-1]
            T = torch.einsum("abmn,and->amd" if isinstance(kk, _Paired) else "abmn,bnd->amd", Ws, dY)
            g = torch.zeros(Xa.shape, dtype=torch.float32)
            g[:, 1:] += T
            g[:, :-1] -= T
            assert g.dtype == torch.float32 and spec.get("param") is None
            return g.double().numpy()
        dG = O.increments_adjoint(_f32(W)) * np.asarray(w, dtype=np.float64)[:, :, None, None]
        (g,) = torch.autograd.grad(G, Xa, grad_outputs=torch.from_numpy(_f32(dG) if user else dG).to(G.dtype))
        return g.double().numpy()

    R = _rows(spec, A)
    sym = op in ("gram_sym", "gram_sym_grad")
    Y2 = Xf if sym else Yf
    val = forward(Xf, Y2)
    out = {"value": val[:, 0] if op in ("kernel", "kernel_grad") else val}
    if op == "gram_grad":
        out["grad"] = gradient(Xf[R], Yf, _weights(spec, t, (A, B))[R])
    elif op == "kernel_grad":
        out["grad"] = gradient(Xf[R], Yf[R], _weights(spec, t, (A, 1))[R])
    elif op == "gram_sym_grad":
        w = _weights(spec, t, (A, A))
        g1, g2 = gradient(Xf[R], Xf, w[R]), gradient(Xf[R], Xf, w.T[R].copy())
        out["grad"] = (2.0 * g1, g1 + g2)
    return out


def measure_f32_bound(spec, t, nthreads=1):
    """{output: {"source", "distance", "tol"}}: the distance of the fp32-stage restatement from the all-fp64 oracle in the comparator's
    own measure, and 4 x that distance (the summation order differs)."""
    want, stage = expected(dict(spec, f32_bound=None), t, nthreads), expected_f32_stage(spec, t, nthreads)
    out = {}
    for name, w in want.items():
        if spec["op"] == "kgrad" and name != "k":      # (compared on the restatement's own increments: no allowance)
            continue
        pairs = zip(stage[name], w) if isinstance(w, tuple) else ((stage[name], w),)
        dist = max(compare(name, s_, w_, 0.0)[2] for s_, w_ in pairs)
        out[name] = {"source": f32_stage_key(spec), "distance": dist, "tol": 4 * dist}
    return out


def cells(spec):
    """The oracle's work for the case in fine-grid cells (a forward sweep 1 per cell, an adjoint 2, the derivative solver 3)."""
    op, A, B, M, N = spec["op"], spec["A"], spec["B"], spec["M"], spec["N"]
    r = 4 ** spec["dyadic"]
    R = len(_rows(spec, A))
    xy, xx, yy = (M - 1) * (N - 1) * r, (M - 1) * (M - 1) * r, (N - 1) * (N - 1) * r
    if op in ("loss_weights",): return A * (A + B)
    if op in ("exact_fwd",): return A * xy
    if op in ("exact_adj", "adj_wild"): return 2 * A * xy
    if op == "deriv": return 3 * A * xy
    if op == "truncated_golden": return A * B * M * N
    if op == "exact_deriv": return 3 * A * xy
    if op == "truncated": return A * M * spec["D"] ** spec["L"] + B * N * spec["D"] ** spec["L"] + A * B * spec["D"] ** spec["L"]
    if op == "gram": return A * B * xy
    if op == "gram_grad": return (A + 2 * R) * B * xy
    if op == "gram_sym": return A * A * xx
    if op == "gram_sym_grad": return (A + 4 * R) * A * xx
    if op in ("kernel", "kernel_fn"): return A * xy
    if op == "kernel_grad": return (A + 2 * R) * xy
    if op == "distance": return A * (xx + yy + xy)
    if op == "scoring_rule": return A * A * xx + A * xy
    if op == "esr_grad": return (A + 2 * R) * A * xx + (A + 2 * R) * B * xy
    if op == "mmd": return A * A * xx + B * B * yy + A * B * xy
    if op == "mmd_grad": return (A + 2 * R) * A * xx + B * B * yy + (A + 2 * R) * B * xy
    if op == "kgrad": return 3 * A * B * xy
    if op in ("prefix_gram",): return A * B * xy
    if op == "prefix_kernel": return A * xy
    raise ValueError(op)


def check_case(spec, outputs, want):
    """Every output of the call against the oracle -> list of failures (output, worst index, error, tolerance)."""
    bad = []
    R = _rows(spec, spec["A"])
    for name, w in want.items():
        got = outputs[name].detach().double().cpu().numpy()
        tol = tolerance(spec, name)
        if name == "grad":
            got = got[R]
        if tol == 0.0:      # FLAG_EXACT: the oracle's value, rounded once to the output's dtype, bit for bit
            w = w.astype(np.float32).astype(np.float64) if outputs[name].dtype == torch.float32 else w
        res = [compare(name, got, wi, tol) for wi in (w if isinstance(w, tuple) else (w,))]
        best = min(res, key=lambda r: r[2])
        if not best[0]:
            idx = best[1]
            if name == "grad" and idx is not None:
                idx = (R[idx[0]],) + idx[1:]
            bad.append((name, idx, best[2], tol))
    assert set(want) == set(outputs), (sorted(want), sorted(outputs))
    return bad
