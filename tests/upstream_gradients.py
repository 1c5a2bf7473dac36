"""Upstream gradients: the rows, the weights and the expectations of tests/test_upstream_gradients_host.py and
tests/test_gpu_upstream_gradients.py (test infrastructure; numpy and torch only -- nothing here imports the product package: the test
modules hand in the call that runs a row and the static kernels the references differentiate).

Every backward kernel has two inputs, the paths and the upstream gradient.  The other numerical tests vary the paths; their upstream
gradient is `ones` or a fresh `torch.randn`: never zero, never non-finite, of one magnitude on every pair, contiguous, and at the
start of an aligned allocation.  The families below vary the upstream gradient alone, on unit-walk paths:

    onehot     one pair at the first, the last and a middle position (and on either side of a lane group's chunk boundary where the
               back-end reports its chunks): the paths the pair does not reach are EXACTLY zero, the reached ones are the pair's own gradient
    zero       all zero (exactly zero everywhere), one zero row, a checkerboard
    scaled     w 2^40 and w 2^-40 against 2^+-40 times the gradient of w, bit for bit
    levels     (truncated rows) sigma = e_1, e_L, and sigma with one zero in the middle
    nonfinite  NaN, +inf, -inf at one pair, an all-NaN w: every element of a reached path whose reference contribution is non-zero is
               non-finite (NaN for NaN), every other path is finite and is the gradient of w with that entry zero
    address    w -- and X, Y and w together -- as views at an element offset inside a NaN-filled buffer: the bits of the aligned call
    layout     the expanded gradient of .sum(), a transposed / strided w: the bits of the contiguous copy

The reference of every row is a PER-PAIR gradient tensor, computed once and contracted with each weight in numpy: px[a, b] = d k(x_a, y_b) /
d x_a (A, B, M, D), py[a, b] = d k(x_a, y_b) / d y_b (A, B, N, D) where the row returns dY.  SigKernel rows: oracle.gram_grad_points;
exact_gradient rows: the recurrence of tests/exact_gradient_reference.py chained through the static kernel by torch autograd on the
CPU; truncated rows: CPU fp64 autograd of the torch restatement, one pair at a time.  Bounds: the instance ledger's (1e-8 per path,
RESCUE_GRAD_TOL on the rows with an exploding pair, two fp32 ulps on top for fp32 paths), 1e-8 for exact_gradient, 1e-10 truncated."""
import numpy as np
import torch

import value_regimes as V

SIGMA = 0.8
NAN, INF = float("nan"), float("inf")
F32_ULPS2 = 2.0 ** -22             # instance_ledger.F32_ULPS2
GRAD_TOL = 1e-8                    # instance_ledger.TOL64["grad"]; the bar of tests/test_gpu_exact_gradient.py
RESCUE_GRAD_TOL = 2e-8             # instance_ledger.RESCUE_GRAD_TOL
TRUNCATED_GRAD_TOL = 1e-10         # README: gradients of the truncated kernel
FAMILIES = ("onehot", "zero", "scaled", "levels", "nonfinite", "address", "layout")
ADJOINT_ENTRIES = ("linear_adjoint_fused", "rbf_adjoint_fused", "linear_adjoint_fused_mb", "rbf_adjoint_fused_mb", "static_adjoint",
                   "static_adjoint2", "second_argument_gradient", "truncated_adjoint", "truncated_points_adjoint", "truncated_long_adjoint",
                   "truncated_wide_adjoint")
WILD_PAIR = (2, 5)                 # tests/test_configs.py::_one_wild_pair


# ------------------------------------------------------------------------------------------------------------------- rows
def _sig(name, op, sh, kind, knobs=None, claims=(), tol=GRAD_TOL, outputs=("dX",), wild=False, ppg=False, fused=False, lens=None, route=None):
    """one SigKernel row: op gram / sym / paired / loss / exact / ragged; claims: substrings of mangled kernel names the trace must show"""
    wshape = () if op == "loss" else ((sh["A"],) if op == "paired" else (sh["A"], sh["B"]))
    return {"name": name, "api": "sig", "op": op, "shape": sh, "kind": kind, "knobs": dict(knobs or {}), "claims": tuple(claims),
            "tol": tol + (F32_ULPS2 if sh["f32"] else 0.0), "outputs": outputs, "wild": wild, "ppg": ppg, "fused": fused, "lens": lens,
            "wshape": wshape, "sym": op == "sym", "f32": sh["f32"], "route": route,
            "id": "%s-%s-%s" % (name.replace(" ", "_"), V.shape_key(sh), kind)}


_OPS = {"gram_grad": "gram", "sym_grad": "sym", "mmd_grad": "loss", "exact_grad": "exact"}
_FUSED_CLAIMS = ("k_adj_fused_",)


def _reused_rows():
    """the rows of value_regimes.ROUTES whose outputs include the gradient, with their shapes, knobs and claims"""
    out = []
    for row in V.ROUTES:
        if "grad" not in row["outputs"]:
            continue
        for sh in row["shapes"]:
            for kind in row["kinds"]:
                claims = V.claims_of(row, kind)
                out.append(_sig(row["name"], _OPS[row["op"]], sh, kind, row["knobs"], claims,
                                fused=any(f in c for c in claims for f in _FUSED_CLAIMS), route=row["name"]))
    return out


# Shapes of the rows added here.  PPG_GRAM_B / PPG_PAIRED_P: the smallest batches of 8-point paths at which the fused adjoints report more
# than one pair per lane-group chunk (HipBackend.last_fused_ppg > 1), found on one MI355X by bisection: the 7 x 1009 pairs of
# test_batches_without_a_suitable_divisor_fill_the_lane_groups (24-point paths there) still have a lane group each at 8 points -- ppg is
# 1 up to 7 x 2340 and 2 from 7 x 2341 pairs (16384 lane groups), and 1 up to 32767 paired pairs.  The rows assert the mode, so a
# change of the launch plan fails by name.
PPG_GRAM_B = 2341
PPG_PAIRED_P = 32768


def _new_rows():
    rows = []
    for kind in V.KINDS:
        rows.append(_sig("Gram chunks of several pairs", "gram", V.shape(7, PPG_GRAM_B, 8, 8, 3, 1), kind, claims=("k_adj_fused_%sI" % kind,),
                         ppg=True, fused=True))
        rows.append(_sig("paired chunks of several pairs", "paired", V.shape(PPG_PAIRED_P, PPG_PAIRED_P, 8, 8, 3, 1), kind,
                         claims=("k_adj_fused_%sI" % kind,), ppg=True, fused=True))
    # test_fused_adjoints_rescue_an_exploding_pair_on_the_device: 6 x 40 pairs of 32 points, pair (2, 5) explodes, the default screen 1e3
    for kind, D, d in (("linear", 4, 1), ("rbf", 3, 1)):
        rows.append(_sig("one wild pair (device rescue)", "gram", V.shape(6, 40, 32, 32, D, d), kind,
                         claims=("k_adj_fused_%sI" % kind,) + V.RESCUE_CLAIMS, tol=RESCUE_GRAD_TOL, wild=True, fused=True))
    # the loss wrappers: value_regimes' "merged loss launch" row is the one-launch glue (k_loss_value, the upstream scalar as `gscale` of
    # the finish kernels); beside it the merged route through torch ops (routes.no_loss_launch), whose weights are wb * grad_output
    for kind in V.KINDS:
        rows.append(_sig("merged loss, torch glue", "loss", V.shape(4, 4, 20, 20, 3, 1), kind, knobs={"no_loss_launch": True},
                         claims=("k_fwd_fusedI", "k_adj_fused_%sI" % kind), fused=True))
    rows.append(_sig("one-launch loss", "loss", V.shape(9, 2, 20, 20, 2, 0), "rbf", claims=("k_loss_value", "k_adj_fused_rbfI"), fused=True))
    for kind in V.KINDS:
        static = "linear" if kind == "linear" else "nodes"
        rows.append(_sig("exact_gradient=True, dX and dY", "exact", V.shape(2, 3, 6, 5, 3, 1), kind, claims=("k_static_" + static, kind + "_adj"),
                         outputs=("dX", "dY")))
        rows.append(_sig("exact_gradient=True, ragged", "ragged", V.shape(3, 4, 6, 5, 2, 1), kind, claims=("k_static_" + static, kind + "_adj"),
                         outputs=("dX", "dY"), lens=((2, 6, 4), (5, 2, 4, 3))))
    return rows


TRUNC_ORDER1, TRUNC_GENERAL = "k_trunc_sigILi1ELi2E", "k_trunc_sigILi4ELi1E"      # tests/test_gpu_truncated.py
# mode -> (keywords of TruncatedSigKernel, the back-end entry that must be called, (A, B, points M, points N, D), the claimed instance):
# the smallest shape of each mode's own GPU test file, L = 4
TRUNC_MODES = {
    "plain": ({}, "truncated_adjoint", (3, 2, 10, 7, 3), TRUNC_ORDER1),
    "points_adjoint": ({"points_adjoint": True, "rbf": 1.0}, "truncated_points_adjoint", (3, 2, 10, 7, 3), "k_trunc_sig"),
    "long_adjoint": ({"long_adjoint": True}, "truncated_long_adjoint", (3, 2, 130, 41, 3), TRUNC_GENERAL),
    "wide_adjoint": ({"wide_adjoint": True}, "truncated_wide_adjoint", (3, 2, 10, 7, 9), TRUNC_GENERAL),
}
TRUNC_L = 4


def _trunc_rows():
    rows = []
    for mode, (kw, entry, (A, B, M, N, D), claim) in TRUNC_MODES.items():
        for op in ("gram", "paired", "sym"):
            Bv = A if op in ("paired", "sym") else B
            Nv = M if op == "sym" else N
            sh = V.shape(A, Bv, M, Nv, D, 0, sym=op == "sym")
            rows.append({"name": "truncated " + mode, "api": "trunc", "op": op, "shape": sh, "kind": mode, "knobs": dict(kw), "claims": (claim,),
                         "tol": TRUNCATED_GRAD_TOL, "outputs": ("dX",) if op == "sym" else ("dX", "dY"), "wild": False, "ppg": False,
                         "fused": False, "lens": None, "wshape": (A,) if op == "paired" else (A, Bv), "sym": op == "sym", "f32": False,
                         "entry": entry, "route": None, "id": "truncated_%s-%s-%s" % (mode, op, V.shape_key(sh))})
    return rows


ROWS = _reused_rows() + _new_rows() + _trunc_rows()
ROW_BY_ID = {r["id"]: r for r in ROWS}
assert len(ROW_BY_ID) == len(ROWS)


def families_of(row):
    if row["op"] == "loss":      # a scalar factor on the value
        return ("zero", "scaled", "nonfinite", "address")
    return tuple(f for f in FAMILIES if f != "levels" or row["api"] == "trunc")


def cases():
    return [(row, fam) for row in ROWS for fam in families_of(row)]


# ------------------------------------------------------------------------------------------------------------------- inputs
def _one_wild_pair(gen, A, B, M, D):
    """tests/test_configs.py::_one_wild_pair: random walks, except that x_2 and y_5 are the same straight line"""
    from conftest import walk
    X, Y = walk(gen, A, M, D) * 2, walk(gen, B, M, D) * 2
    line = torch.arange(M, dtype=torch.float64)[:, None] * 0.6 * torch.ones(1, D, dtype=torch.float64) / np.sqrt(D)
    X[2], Y[5] = line, line.clone()
    return X.numpy(), Y.numpy()


_INPUTS = {}


def inputs(row):
    """-> X (A, M, D), Y (B, N, D), w0 (the row's weight shape; symmetric for a symmetric row; a scalar for a loss): numpy fp64,
    fp32-rounded for an fp32 row, computed once per row and never written to"""
    if row["id"] in _INPUTS:
        return _INPUTS[row["id"]]
    sh = row["shape"]
    gen = torch.Generator().manual_seed(7)
    if row["wild"]:
        X, Y = _one_wild_pair(torch.Generator().manual_seed(41), sh["A"], sh["B"], sh["M"], sh["D"])
    elif row["api"] == "trunc":      # paths that start at the origin, steps as in tests/test_truncated_host.py: N(0, 1) / sqrt(steps D)
        X, Y, _, _ = V.inputs({}, sh, seed=11)
        X, Y = X - X[:, :1], Y - Y[:, :1]
    elif row["op"] == "paired":      # (value_regimes.inputs also draws an (A, B) weight)
        from conftest import walk
        g3 = torch.Generator().manual_seed(3)
        X, Y = walk(g3, sh["A"], sh["M"], sh["D"]).numpy(), walk(g3, sh["A"], sh["N"], sh["D"]).numpy()
    else:
        X, Y, _, _ = V.inputs({}, sh, seed=3)
    if row["lens"] is not None:      # padded at the end by repeating the last point (sigkernel_amd.pad_paths)
        for T, lens in ((X, row["lens"][0]), (Y, row["lens"][1])):
            for i, n in enumerate(lens):
                T[i, n:] = T[i, n - 1]
    if row["op"] == "loss":
        w = np.float64(0.75)
    else:
        w = torch.randn(row["wshape"], generator=gen, dtype=torch.float64).numpy()
        if row["sym"]:
            w = w + w.T
        if row["f32"]:
            w = w.astype(np.float32).astype(np.float64)
    for a in (X, Y, w):
        a.setflags(write=False)
    _INPUTS[row["id"]] = (X, Y, w)
    return X, Y, w


def trunc_sigma(row, label="base"):
    """the level weights sigma_0 .. sigma_L of a truncated row: `base` in [0.5, 1.5]; e1 / eL: one level alone; hole: one zero in the middle"""
    L = TRUNC_L
    s = np.random.default_rng(5).uniform(0.5, 1.5, L + 1)
    if label in ("e1", "eL"):
        s = np.zeros(L + 1)
        s[1 if label == "e1" else L] = 1.0
    elif label == "hole":
        s[L // 2] = 0.0
    else:
        assert label == "base", label
    return s


# ------------------------------------------------------------------------------------------------------------------- weights
def positions(row, ppg=None):
    """[(label, index)] of the one-hot family: first, last, middle; with ppg (pairs per lane-group chunk, > 1) the two pairs on either
    side of the first chunk boundary of the middle row (Gram: chunk c of an a is [c B / chunks, (c + 1) B / chunks)) or of the batch
    (paired: runs of ppg consecutive pairs)"""
    ws = row["wshape"]
    if len(ws) == 1:
        P = ws[0]
        out = [("first", (0,)), ("last", (P - 1,)), ("middle", (P // 2,))]
        if ppg and ppg > 1 and ppg < P:
            out += [("chunk end", (ppg - 1,)), ("chunk start", (ppg,))]
        return out
    A, B = ws
    out = [("first", (0, 0)), ("last", (A - 1, B - 1)), ("middle", (A // 2, B // 2 + (1 if row["sym"] and A // 2 == B // 2 and B > 2 else 0)))]
    if row["wild"]:
        out.append(("wild", WILD_PAIR))
    if ppg and ppg > 1 and ppg < B:
        chunks = -(-B // ppg)
        b1 = B // chunks
        out += [("chunk end", (A // 2, b1 - 1)), ("chunk start", (A // 2, b1))]
    return out


def onehot(row, idx, value=1.0):
    w = np.zeros(row["wshape"])
    w[idx] = value
    if row["sym"]:
        w = w + w.T      # e(a0, b0) + e(b0, a0): the 2x rule and the triangle fold agree only for symmetric weights
    return w


def with_entry(row, w0, idx, value):
    w = np.array(w0, dtype=np.float64)
    w[idx] = value
    if row["sym"]:
        w[idx[::-1]] = value
    return w


def zero_weights(row, w0):
    """[(label, w)]: all zero, one zero row (and column, symmetric rows), a checkerboard"""
    w0 = np.asarray(w0)
    if w0.ndim == 1:
        one = w0.copy()
        one[1] = 0.0
        return [("all zero", np.zeros_like(w0)), ("one zero", one), ("checkerboard", w0 * (np.arange(w0.shape[0]) % 2))]
    one = w0.copy()
    one[1, :] = 0.0
    if row["sym"]:
        one[:, 1] = 0.0
    a, b = np.indices(w0.shape)
    return [("all zero", np.zeros_like(w0)), ("one zero row", one), ("checkerboard", w0 * ((a + b) % 2))]


def offset_view(values, offset, dtype, device, tail=5):
    """`values` as a contiguous view at element `offset` inside a NaN-filled buffer, NaNs behind it too -> (view, buffer, guard mask)"""
    values = torch.as_tensor(np.array(values)).to(dtype)
    n = values.numel()
    buf = torch.full((offset + n + tail,), NAN, dtype=dtype, device=device)
    view = buf[offset:offset + n].view(values.shape)
    view.copy_(values.to(device))
    guard = torch.ones(buf.shape, dtype=torch.bool, device=device)
    guard[offset:offset + n] = False
    assert view.storage_offset() == offset and view.is_contiguous()
    assert view.data_ptr() % 16 == (buf.data_ptr() + offset * buf.element_size()) % 16
    return view, buf, guard


def guards_intact(buf, guard):
    return bool(torch.isnan(buf[guard]).all())


# ------------------------------------------------------------------------------------------------------------------- references
class PairGrads:
    """px (A, B, M, D) [and py (A, B, N, D)] of a row; paired rows hold (P, 1, ...); fold(w) contracts them with a weight"""

    def __init__(self, row, px, py=None, base=None):
        self.row, self.px, self.py, self.base = row, np.asarray(px, dtype=np.float64), None if py is None else np.asarray(py, dtype=np.float64), base

    def _w2(self, w):
        w = np.asarray(w, dtype=np.float64)
        return w[:, None] if w.ndim == 1 else w

    def fold(self, w):
        """{output: gradient} for the upstream weight w (a scalar for a loss row: base = d value / dX)"""
        row = self.row
        if row["op"] == "loss":
            with np.errstate(invalid="ignore"):
                return {"dX": float(w) * self.base}
        w = self._w2(w)
        with np.errstate(invalid="ignore", over="ignore"):
            gx = np.einsum("ab,abmd->amd", w, self.px)
            if row["sym"] and row["api"] == "sig":
                return {"dX": 2.0 * gx}      # the reference's 2x rule (w symmetric: equal to the fold of both arguments)
            if row["sym"]:                   # X is Y: autograd adds both arguments
                return {"dX": gx + np.einsum("ab,abnd->bnd", w, self.py)}
            out = {"dX": gx}
            if "dY" in row["outputs"]:
                out["dY"] = np.einsum("ab,abnd->bnd", w, self.py) if len(row["wshape"]) == 2 else np.einsum("ab,abnd->and", w, self.py)
            return out

    def reached(self, w):
        """{output: bool per path}: whether a non-zero entry of w reaches the path"""
        row = self.row
        if row["op"] == "loss":
            return {"dX": np.full(self.base.shape[0], bool(w != 0))}
        nz = self._w2(w) != 0
        paired = len(row["wshape"]) == 1
        if row["sym"]:
            return {"dX": nz.any(1) | nz.any(0)}
        out = {"dX": nz.any(1)}
        if "dY" in row["outputs"]:
            out["dY"] = nz.any(1) if paired else nz.any(0)
        return out

    def touched(self, mask):
        """{output: bool per element}: whether any pair of the boolean mask `mask` (the weight's shape) has a non-zero reference
        contribution to the element"""
        row = self.row
        if row["op"] == "loss":
            return {"dX": self.base != 0}
        m = self._w2(mask).astype(bool)
        paired = len(row["wshape"]) == 1
        tx = ((self.px != 0) & m[:, :, None, None]).any(1)
        if row["sym"]:
            ty = ((self.py if self.py is not None else self.px) != 0) & m[:, :, None, None]
            return {"dX": tx | (ty.any(0) if self.py is not None else (((self.px != 0) & m.T[:, :, None, None]).any(1)))}
        out = {"dX": tx}
        if "dY" in row["outputs"]:
            ty = (self.py != 0) & m[:, :, None, None]
            out["dY"] = ty.any(1) if paired else ty.any(0)
        return out


def _pair_grads_autograd(G, leaves, dG):
    """per-pair gradients of sum(dG[a, b] * G[a, b]) with respect to the leaves, pair by pair -> one (A, B) + leaf.shape[1:] array per
    leaf, the slice of the leaf's own path"""
    A, B = dG.shape[:2]
    outs = [np.zeros((A, B) + tuple(t.shape[1:])) for t in leaves]
    for a in range(A):
        for b in range(B):
            mask = torch.zeros_like(dG)
            mask[a, b] = dG[a, b]
            gs = torch.autograd.grad(G, leaves, grad_outputs=mask, retain_graph=True, allow_unused=True)
            for o, g, i in zip(outs, gs, (a, b)):
                o[a, b] = 0.0 if g is None else g[i].numpy()
    return outs


def sig_reference(row, kernel, paired_kernel=None):
    """PairGrads of a SigKernel row.  kernel: the static kernel object (Gram_matrix / batch_kernel in torch); the standard rows contract
    oracle.gram_grad_points, the exact_gradient rows chain tests/exact_gradient_reference.py's W through the static kernel"""
    from oracle import oracle as O
    X, Y, _ = inputs(row)
    sh, d = row["shape"], row["shape"]["d"]
    Xt, Yt = torch.from_numpy(np.array(X)), torch.from_numpy(np.array(Y))
    op = row["op"]
    if op == "gram" and row["ppg"]:      # thousands of second paths: every pair as one row of a paired batch, one vector-Jacobian product
        A, B = sh["A"], sh["B"]
        Xr, Yr = Xt[:, None].expand(-1, B, -1, -1).reshape((A * B,) + X.shape[1:]), Yt[None].expand(A, -1, -1, -1).reshape((A * B,) + Y.shape[1:])
        return PairGrads(row, O.gram_grad_weighted(Xr, Yr, np.ones((A * B, 1)), paired_kernel, d).reshape((A, B) + X.shape[1:]))
    if op in ("gram", "sym"):
        return PairGrads(row, O.gram_grad_points(Xt, Xt if op == "sym" else Yt, kernel, d))
    if op == "paired":      # (instance_ledger's adapter of paired batches: a (P, 1) Gram matrix of P pairs)
        return PairGrads(row, O.gram_grad_weighted(Xt, Yt, np.ones((sh["A"], 1)), paired_kernel, d)[:, None])
    if op == "loss":      # tools/fuzz_api.py:158-178 with the reference's 2x rule on K_XX
        A, B = sh["A"], sh["B"]
        wxx = (1.0 - np.eye(A)) / (A * (A - 1.0))
        base = 2.0 * O.gram_grad_weighted(Xt, Xt, wxx, kernel, d) + O.gram_grad_weighted(Xt, Yt, np.full((A, B), -2.0 / (A * B)), kernel, d)
        return PairGrads(row, np.zeros((A, 1) + X.shape[1:]), base=base)
    assert op in ("exact", "ragged"), op
    import exact_gradient_reference as R
    A, B = sh["A"], sh["B"]
    lx, ly = row["lens"] if row["lens"] is not None else ((sh["M"],) * A, (sh["N"],) * B)
    px, py = np.zeros((A, B) + X.shape[1:]), np.zeros((A, B) + Y.shape[1:])
    for a in range(A):
        for b in range(B):
            if lx[a] < 2 or ly[b] < 2:
                continue
            xa, yb = Xt[a:a + 1, :lx[a]].clone().requires_grad_(True), Yt[b:b + 1, :ly[b]].clone().requires_grad_(True)
            G = kernel.Gram_matrix(xa, yb)
            inc = O.increments(G.detach().numpy())
            _, W = R.exact_adjoint(inc[0, 0], d)
            dG = torch.from_numpy(O.increments_adjoint(W[None, None]))
            gx, gy = torch.autograd.grad(G, (xa, yb), grad_outputs=dG)
            px[a, b, :lx[a]], py[a, b, :ly[b]] = gx[0].numpy(), gy[0].numpy()
    return PairGrads(row, px, py)


def trunc_reference(row, make, sigma_label="base"):
    """PairGrads of a truncated row by CPU fp64 autograd of the restatement, one pair at a time.  make(sigma) -> the object under test's
    twin for CPU tensors"""
    X, Y, _ = inputs(row)
    tk = make(torch.from_numpy(trunc_sigma(row, sigma_label)))
    A, B = row["shape"]["A"], row["shape"]["B"]
    paired = row["op"] == "paired"
    px = np.zeros(((A, 1) if paired else (A, B)) + X.shape[1:])
    py = np.zeros(((A, 1) if paired else (A, B)) + Y.shape[1:])
    Ys = X if row["sym"] else Y
    for a in range(A):
        for b in ((a,) if paired else range(B)):
            xa = torch.from_numpy(np.array(X[a:a + 1])).requires_grad_(True)
            yb = torch.from_numpy(np.array(Ys[b:b + 1])).requires_grad_(True)
            k = tk.compute_kernel(xa, yb) if paired else tk.compute_Gram(xa, yb)
            gx, gy = torch.autograd.grad(k.sum(), (xa, yb), allow_unused=True)
            px[a, 0 if paired else b] = 0.0 if gx is None else gx[0].numpy()
            py[a, 0 if paired else b] = 0.0 if gy is None else gy[0].numpy()
    return PairGrads(row, px, py)


# ------------------------------------------------------------------------------------------------------------------- comparison
def compare_grads(got, want, tol):
    """instance_ledger.compare_grads: per path, max |got - want| over the path <= tol max |want| over the path -> (ok, worst index, error)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.all(np.isfinite(got)):
        return False, None, float("inf")
    diff = np.abs(got - want)
    flat = (slice(None),) + (None,) * (want.ndim - 1)
    norm = np.maximum(np.abs(want).reshape(want.shape[0], -1).max(1), 1e-300)[flat]
    err = diff / norm
    i = np.unravel_index(int(np.argmax(err)), err.shape)
    return bool(err[i] <= tol), tuple(int(j) for j in i), float(err[i])


def check_against(ref, w, got, tol, what, report=None):
    """a finite weight: unreached paths exactly zero, every path within the bound of the reference -> list of failures"""
    want, reached = ref.fold(w), ref.reached(w)
    bad = []
    for name, g in got.items():
        g = g.detach().double().cpu().numpy()
        un = ~reached[name]
        if un.any() and not np.all(g[un] == 0.0):
            i = np.argwhere(g[un] != 0.0)[0]
            bad.append("%s %s: an unreached path is not exactly zero (path %d of the unreached, element %s: %r)"
                       % (what, name, i[0], tuple(i[1:]), float(g[un][tuple(i)])))
        ok, idx, err = compare_grads(g, want[name], tol)
        if report:
            report("%s %s" % (what, name), err, tol)
        if not ok:
            bad.append("%s %s: %.3e > %.3e at %s" % (what, name, err, tol, idx))
    return bad


def check_nonfinite(ref, w, got, tol, what, value, pad=None, report=None):
    """w holds `value` (NaN, +inf or -inf) where it is not finite: on the paths those entries reach every element with a non-zero
    reference contribution is non-finite (NaN for NaN); every other path is finite and within the bound of the reference with those
    entries set to zero.  pad: {output: bool per element} left out of the non-finite assertion (ragged padding)"""
    w = np.asarray(w, dtype=np.float64)
    hot = ~np.isfinite(w)
    wfin = np.where(hot, 0.0, w)
    want = ref.fold(wfin)
    hit = ref.reached(hot.astype(np.float64))
    must = ref.touched(hot)
    bad = []
    for name, g in got.items():
        g = g.detach().double().cpu().numpy()
        m = must[name] & hit[name][(slice(None),) + (None,) * (g.ndim - 1)]
        if pad is not None:
            m = m & ~pad[name]
        if not m.any():
            bad.append("%s %s: the entry reaches no element with a non-zero reference contribution" % (what, name))
        wrong = m & (~np.isnan(g) if np.isnan(value) else np.isfinite(g))
        if wrong.any():
            i = tuple(int(v) for v in np.argwhere(wrong)[0])
            bad.append("%s %s: %d of %d reached elements are %s, the first at %s: %r" % (what, name, int(wrong.sum()), int(m.sum()),
                                                                                        "not NaN" if np.isnan(value) else "finite", i, float(g[i])))
        rest = ~hit[name]
        if rest.any():
            ok, idx, err = compare_grads(g[rest], want[name][rest], tol)
            if report:
                report("%s %s (other paths)" % (what, name), err, tol)
            if not ok:
                bad.append("%s %s: the paths the entry does not reach: %.3e > %.3e at %s" % (what, name, err, tol, idx))
    return bad


def mask_size(ref, idx):
    """elements of the reached paths that the non-finite family skips for a non-finite entry at idx: where the pair's reference
    contribution is exactly zero -> {output: count}"""
    row = ref.row
    hot = np.zeros(row["wshape"], dtype=bool)
    hot[idx] = True
    if row["sym"]:
        hot[idx[::-1]] = True
    must, hit = ref.touched(hot), ref.reached(hot.astype(np.float64))
    return {n: int((~must[n] & hit[n][(slice(None),) + (None,) * (must[n].ndim - 1)]).sum()) for n in must}


# ------------------------------------------------------------------------------------------------------------------- the families
def _bits(first, other, what, report=None):
    """every output of `other` has the bits of `first` -> list of failures"""
    from poison import same_bits
    bad = []
    for name in first:
        ok, msg = same_bits(first[name], other[name])
        if report:
            report("%s %s" % (what, name), 0.0 if ok else float("inf"), 0.0)
        if not ok:
            bad.append("%s %s: %s" % (what, name, msg))
    return bad


def _padding(row, got):
    if row["lens"] is None:
        return None
    pad = {}
    for name, lens in zip(("dX", "dY"), row["lens"]):
        if name in got:
            m = np.zeros(tuple(got[name].shape), dtype=bool)
            for i, n in enumerate(lens):
                m[i, n:] = True
            pad[name] = m
    return pad


def run_family(row, fam, ref_for, call, device, report=None, ppg=None, dtype=None):
    """One family on one row -> list of failures (empty: the row passes).

    call(w, X=None, Y=None, sigma="base", expanded=False) -> {"dX": tensor[, "dY": tensor]}: the row's operation with the upstream
    gradient w (a numpy array: made a contiguous tensor of the row's dtype on `device`; a tensor: passed as it is; expanded: .sum().backward()
    instead), on the row's paths unless leaves X, Y are given.  ref_for(sigma label) -> PairGrads.  dtype: of the views this function
    builds (default: the row's)."""
    X, Y, w0 = inputs(row)
    ref, tol = ref_for("base"), row["tol"]
    dtype = dtype or (torch.float32 if row["f32"] else torch.float64)
    loss = row["op"] == "loss"
    bad = []
    if fam == "onehot":
        for label, idx in positions(row, ppg):
            w = onehot(row, idx)
            bad += check_against(ref, w, call(w), tol, "one-hot %s %s" % (label, idx), report)
    elif fam == "zero":
        todo = [("zero factor", np.float64(0.0))] if loss else zero_weights(row, w0)
        for label, w in todo:
            got = call(w)
            if not np.any(w):
                for name, g in got.items():
                    exact = bool((g == 0).all())
                    if report:
                        report("%s %s" % (label, name), 0.0 if exact else float("inf"), 0.0)
                    if not exact:
                        bad.append("%s %s: %d elements are not exactly zero" % (label, name, int((g != 0).sum())))
            else:
                bad += check_against(ref, w, got, tol, label, report)
    elif fam == "scaled":
        g0 = call(w0)
        bad += check_against(ref, w0, g0, tol, "w", report)
        for e in (40, -40):
            got = call(w0 * 2.0 ** e)
            bad += _bits({n: g * 2.0 ** e for n, g in g0.items()}, got, "w 2^%d against 2^%d times the gradient of w" % (e, e), report)
    elif fam == "levels":
        for label in ("e1", "eL", "hole"):
            bad += check_against(ref_for(label), w0, call(w0, sigma=label), tol, "sigma " + label, report)
    elif fam == "nonfinite":
        if loss:
            for v in (NAN, INF, -INF):
                bad += check_nonfinite(ref, np.float64(v), call(np.float64(v)), tol, "factor %r" % v, v, report=report)
        else:
            spots = [p for p in positions(row) if p[0] in ("middle", "wild")]
            for label, idx in spots:
                for v in (NAN, INF, -INF):
                    w = with_entry(row, w0, idx, v)
                    got = call(w)
                    bad += check_nonfinite(ref, w, got, tol, "%r at the %s pair %s" % (v, label, idx), v, _padding(row, got), report)
            w = np.full(row["wshape"], NAN)
            got = call(w)
            bad += check_nonfinite(ref, w, got, tol, "all NaN", NAN, _padding(row, got), report)
    elif fam == "address":
        g0 = call(w0)
        for off in ((1, 2, 3) if row["f32"] else (1,)):
            wv, wbuf, wguard = offset_view(w0, off, dtype, device)
            bad += _bits(g0, call(wv), "w at element offset %d" % off, report)
            Xv, xbuf, xguard = offset_view(X, off, dtype, device)
            Xl = Xv.detach().requires_grad_()
            assert Xl.is_leaf and Xl.storage_offset() == off and Xl.data_ptr() == Xv.data_ptr()
            if row["sym"]:
                Yl, ybuf, yguard = None, xbuf, xguard
            else:
                Yv, ybuf, yguard = offset_view(Y, off, dtype, device)
                Yl = Yv.detach().requires_grad_() if "dY" in row["outputs"] else Yv
            bad += _bits(g0, call(wv, X=Xl, Y=Yl), "X, Y and w at element offset %d" % off, report)
            for what, b, g in (("w", wbuf, wguard), ("X", xbuf, xguard), ("Y", ybuf, yguard)):
                if not guards_intact(b, g):
                    bad.append("the NaNs around %s (element offset %d) were written to" % (what, off))
    elif fam == "layout":
        ones = np.ones(row["wshape"])
        bad += _bits(call(ones), call(None, expanded=True), "the expanded gradient of .sum() against contiguous ones", report)
        g0 = call(w0)
        if len(row["wshape"]) == 2:
            wt = torch.as_tensor(np.ascontiguousarray(w0.T)).to(dtype).to(device).t()
        else:
            buf = torch.full((2 * row["wshape"][0],), NAN, dtype=dtype, device=device)
            wt = buf[::2]
            wt.copy_(torch.as_tensor(np.array(w0)).to(dtype))
        assert not wt.is_contiguous() and tuple(wt.shape) == tuple(row["wshape"])
        bad += _bits(g0, call(wt), "a non-contiguous w against its contiguous copy", report)
    else:
        raise ValueError(fam)
    return bad
