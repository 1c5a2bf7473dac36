"""The forward-to-backward hand-off on the GPU, bit for bit against the build before it became an explicit record
(tests/golden/handoff_parent.npz, recorded on the GPU from the parent commit by tests/golden/make_golden_handoff_parent.py).  One case
per way a forward leaves something for its backward -- edges of one block, edges sliced over several tiles, edges of the up-cast
paths, increments beside the edges, row blocks of the triangle, the staged arrays of the one-launch loss -- and per way a backward
does without.  Per case the value, the gradient, the gradient of a SECOND backward through the retained graph (nothing is kept for
it: it sweeps forward itself) must be equal (torch.equal), and the forward and each backward must launch what they launched.
Every case also states the routes (sk_route_query) it is named for: a shape that drifts off its route fails here, not silently."""
import contextlib
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

PARENT = os.path.join(ROOT, "tests", "golden", "handoff_parent.npz")

F64, F32 = "float64", "float32"
SYM = {"S._SYM_TILES": 2, "S._SYM_MIN_CELLS": 0, "S._SYM_MIN_ROWS": 1}
ONE_BAND, LONG_X, LONG, WIDE = (5, 7, 9, 8, 3), (3, 4, 140, 12, 3), (2, 3, 140, 140, 3), (3, 4, 10, 9, 20)
# the one-band adjoint's transient bytes per Gram row at ONE_BAND (64 B + 2048 M, sigkernel._fused_gradient): three rows fit, the
# block's edges (8 A B (MM + NN + 32) = 17360 bytes) stay within keep_edges_fraction = 1/2 of it
THREE_ROWS_FUSED = 3 * (64 * 7 + 2048 * 9) + 8000
TWO_ROWS_STREAM = 2 * 3 * 4 * 10 * 9 * 8       # two rows of the streaming route at WIDE: 3 B M N doubles each

# name, call, static kernel, (A, B, M, N, D), dyadic, dtype, workspace_bytes, overrides, (forward route, adjoint route, one-launch loss? / triangle with a gradient?)
CASES = [
    ("gram_linear_one_band", "gram", "linear", ONE_BAND, 1, F64, None, {}, ("FUSED", "FUSED", None)),
    ("gram_rbf_one_band", "gram", "rbf", ONE_BAND, 1, F64, None, {}, ("FUSED", "FUSED", None)),
    ("gram_linear_fp32_upcast_edges", "gram", "linear", ONE_BAND, 1, F32, None, {}, ("FUSED", "FUSED", None)),
    ("gram_rbf_d0_adjoint_forms_edges", "gram", "rbf", (5, 7, 9, 8, 6), 0, F64, None, {}, ("FUSED", "FUSED", None)),
    ("gram_rbf_one_block_sliced", "gram", "rbf", ONE_BAND, 1, F64, THREE_ROWS_FUSED, {}, ("FUSED", "FUSED", None)),
    ("gram_rbf_swapped", "gram", "rbf", LONG_X, 1, F64, None, {}, ("FUSED_SWAP", "FUSED_SWAP", None)),
    ("gram_linear_multi_band", "gram", "linear", LONG, 1, F64, None, {}, ("FUSED_MB", "FUSED_MB", None)),
    # (wide RBF paths: the plain forward streams, the forward WITH a gradient pending follows the adjoint's route and keeps its edges)
    ("gram_rbf_multi_band_d12", "gram", "rbf", (2, 3, 140, 140, 12), 1, F64, None, {}, ("STREAM", "FUSED_MB", None)),
    ("gram_linear_stream_kept_inc", "gram", "linear", WIDE, 1, F64, None, {}, ("STREAM", "STREAM", None)),
    ("gram_rbf_stream_kept_inc", "gram", "rbf", WIDE, 1, F64, None, {}, ("STREAM", "STREAM", None)),
    ("gram_linear_stream_no_inc", "gram", "linear", WIDE, 1, F64, None, {"S._KEEP_INCREMENTS_FRACTION": 0.0}, ("STREAM", "STREAM", None)),
    ("gram_rbf_stream_no_inc", "gram", "rbf", WIDE, 1, F64, None, {"S._KEEP_INCREMENTS_FRACTION": 0.0}, ("STREAM", "STREAM", None)),
    ("gram_linear_stream_tiles", "gram", "linear", WIDE, 1, F64, TWO_ROWS_STREAM, {}, ("STREAM", "STREAM", None)),
    ("gram_rbf_one_band_stream_adjoint", "gram", "rbf", ONE_BAND, 1, F64, None, {"routes.no_fused_adjoint": True}, ("FUSED", "STREAM", None)),
    ("gram_user_kernel", "gram", "user", (3, 4, 9, 8, 3), 1, F64, None, {}, ("STREAM", "STREAM", None)),
    ("gram_rbf_max_launch_pairs", "gram", "rbf", ONE_BAND, 1, F64, 1 << 30, {"S._MAX_LAUNCH_PAIRS": 2 * 7}, ("FUSED", "FUSED", None)),
    ("gram_linear_stream_max_launch_pairs", "gram", "linear", WIDE, 1, F64, 1 << 30, {"S._MAX_LAUNCH_PAIRS": 2 * 4}, ("STREAM", "STREAM", None)),
    ("paired_linear_one_band", "paired", "linear", (6, 6, 9, 8, 3), 1, F64, None, {}, ("FUSED", "FUSED", None)),
    ("paired_linear_multi_band", "paired", "linear", (6, 6, 140, 140, 3), 1, F64, None, {}, ("FUSED_MB", "FUSED_MB", None)),
    ("paired_rbf_stream", "paired", "rbf", (6, 6, 10, 9, 20), 1, F64, None, {}, ("STREAM", "STREAM", None)),
    ("sym_rbf_fused_triangle", "sym", "rbf", (16, 16, 9, 9, 3), 1, F64, None, SYM, ("FUSED", "FUSED", True)),
    # (the linear second-argument kernel serves up to 8 dims, and such paths stream from dyadic 3 on: at dim 20 the call solves all pairs)
    ("sym_linear_unfused_triangle", "sym", "linear", (16, 16, 10, 10, 8), 3, F64, None, SYM, ("STREAM", "STREAM", True)),
    ("sym_rbf_unfused_triangle", "sym", "rbf", (16, 16, 10, 10, 20), 1, F64, None, SYM, ("STREAM", "STREAM", True)),
    ("sym_rbf_fused_one_block", "sym", "rbf", (16, 16, 9, 9, 3), 1, F64, None, {}, ("FUSED", "FUSED", True)),
    ("mmd_rbf_one_launch", "mmd", "rbf", (6, 5, 9, 9, 3), 1, F64, None, {}, ("FUSED", "FUSED", True)),
    ("mmd_rbf_composed_d20", "mmd", "rbf", (6, 5, 9, 9, 20), 1, F64, None, {}, ("STREAM", "STREAM", False)),
    ("mmd_rbf_composed_fused_block", "mmd", "rbf", (6, 5, 9, 9, 3), 1, F64, None, {"routes.no_loss_launch": True}, ("FUSED", "FUSED", False)),
    ("score_rbf_one_launch", "score", "rbf", (6, 1, 9, 9, 3), 1, F64, None, {}, ("FUSED", "FUSED", True)),
]
IDS = [c[0] for c in CASES]


class UserKernel:
    """A static kernel the library has no kernel for: the generic route (Gram_matrix / batch_kernel in torch, autograd through them)."""

    def batch_kernel(self, X, Y):
        return (1.0 + 0.5 * torch.bmm(X, Y.permute(0, 2, 1))) ** 2

    def Gram_matrix(self, X, Y):
        return (1.0 + 0.5 * torch.einsum("ipk,jqk->ijpq", X, Y)) ** 2


def walks(steps, dtype):
    """paths from their recorded steps (small integers): exact in fp64, so the record holds the inputs in one byte per coordinate"""
    A, M, D = steps.shape
    return (np.cumsum(steps.astype(np.float64), axis=1) * (1.0 / (3.0 * np.sqrt(M * D)))).astype(dtype)


def inputs(case):
    """(steps of X, steps of Y or None where Y is X, integer weights or None) of a case -- what the maker records; the test reads the record"""
    name, call, kernel, (A, B, M, N, D) = case[:4]
    rng = np.random.default_rng(1000 + IDS.index(name))
    sx = rng.integers(-7, 8, (A, M, D)).astype(np.int8)
    sy = None if call == "sym" else rng.integers(-7, 8, (B, N, D)).astype(np.int8)
    w = None if call in ("mmd", "score") else rng.integers(-64, 65, (A,) if call == "paired" else (A, B)).astype(np.int8)
    return sx, sy, w


def tensors(case, sx, sy, w):
    """device tensors (X, Y, upstream weights) of a case from its record: the weights are fixed and not symmetric"""
    dtype = case[5]
    X = torch.as_tensor(walks(sx, dtype)).cuda()
    Y = X if sy is None else torch.as_tensor(walks(sy, dtype)).cuda()
    return X, Y, (None if w is None else torch.as_tensor((w.astype(np.float64) / 32.0).astype(dtype)).cuda())


def static_kernel(pkg, case):
    return {"linear": pkg.LinearKernel, "rbf": lambda: pkg.RBFKernel(1.0), "user": UserKernel}[case[2]]()


@contextlib.contextmanager
def overrides(pkg, case):
    """the case's module attributes (sigkernel._X) and route switches (routes.x), restored afterwards"""
    targets = {"S": pkg.sigkernel, "routes": pkg.routes}
    saved = []
    try:
        for key, value in case[7].items():
            obj, attr = targets[key.split(".")[0]], key.split(".")[1]
            saved.append((obj, attr, getattr(obj, attr)))
            setattr(obj, attr, value)
        yield
    finally:
        for obj, attr, value in reversed(saved):
            setattr(obj, attr, value)


def on_route(pkg, case, X, Y):
    """(forward route, adjoint route, one-launch loss? / sym: the triangle with a gradient?) of the case's shape, as the library and the host layer answer now"""
    S = pkg.sigkernel
    be, k, d, gram = pkg._lib.get_backend(), static_kernel(pkg, case), case[4], case[1] != "paired"
    names = {getattr(S, n): n for n in ("STREAM", "FUSED", "FUSED_MB", "FUSED_SWAP", "FUSED_MB_SWAP")}
    launch = None
    if case[1] in ("mmd", "score"):
        launch = S._loss_launch_ok(be, k, X, Y, d, False, True, case[1] == "mmd", case[6]) is not None
    elif case[1] == "sym":
        launch = bool(S._sym_triangle_ok(be, k, X, d, False))
    return (names[S._route(be, S.OP_FORWARD, k, X, Y, d, False, gram)], names[S._route(be, S.OP_ADJOINT, k, X, Y, d, False, gram)], launch)


def replay(pkg, case, X, Y, w):
    """the case's public call with two backward passes through its retained graph ->
    (value, gradient, second gradient, [launch counts of the forward, the first backward, the second])"""
    _lib = pkg._lib
    sk = pkg.SigKernel(static_kernel(pkg, case), case[4], workspace_bytes=case[6])
    call = {"gram": lambda Xg: sk.compute_Gram(Xg, Y), "paired": lambda Xg: sk.compute_kernel(Xg, Y),
            "sym": lambda Xg: sk.compute_Gram(Xg, Xg, sym=True), "mmd": lambda Xg: sk.compute_mmd(Xg, Y),
            "score": lambda Xg: sk.compute_scoring_rule(Xg, Y)}[case[1]]

    def counts():
        torch.cuda.synchronize()
        return {k: v for k, v in _lib.launch_counts(reset=True).items() if v > 0}
    with overrides(pkg, case):
        was = _lib.launch_trace(True)
        try:
            _lib.launch_counts(reset=True)
            Xg = X.clone().requires_grad_(True)
            val = call(Xg)
            launches = [counts()]
            loss = val if w is None else (val * w).sum()
            (g1,) = torch.autograd.grad(loss, Xg, retain_graph=True)
            launches.append(counts())
            (g2,) = torch.autograd.grad(loss, Xg, retain_graph=True)
            launches.append(counts())
        finally:
            _lib.launch_trace(was)
    return val.detach(), g1, g2, launches


def result_shapes(case):
    name, call, _, (A, B, M, N, D) = case[:4]
    return {"gram": (A, B), "sym": (A, A), "paired": (A,)}.get(call, ()), (A, M, D)


def save(path, record):
    """{case name: {X, Y, w (integer steps / weights or None), value, grad, grad2, routes, launches}} -> one small .npz.  Everything is
    laid end to end in the order of CASES: the integers as they are, the results as the byte planes of their fp64 values (fp32 results
    are exact in fp64; planes of like bytes compress, whole doubles do not), a second gradient that differs from the first as the
    difference of their bit patterns, routes and launch counts as JSON text."""
    import json
    ints = [np.ravel(record[c[0]][k]) for c in CASES for k in ("X", "Y", "w") if record[c[0]][k] is not None]
    results = np.concatenate([np.ravel(record[c[0]][k]).astype(np.float64) for c in CASES for k in ("value", "grad")])
    differs = [c[0] for c in CASES if not np.array_equal(record[c[0]]["grad"], record[c[0]]["grad2"])]
    bits = lambda a: np.ravel(a).astype(np.float64).view(np.int64)
    second = np.concatenate([bits(record[n]["grad2"]) - bits(record[n]["grad"]) for n in differs] or [np.zeros(0, np.int64)])
    meta = {c[0]: {"routes": [str(r) for r in record[c[0]]["routes"]], "launches": record[c[0]]["launches"], "grad2_differs": c[0] in differs}
            for c in CASES}
    np.savez_compressed(path, steps=np.concatenate(ints).astype(np.int8), results=results.view(np.uint8).reshape(-1, 8).T.copy(),
                        second=second, meta=np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8))


def load(path=PARENT):
    """the record save() wrote"""
    import json
    z = np.load(path)
    steps, results, second = z["steps"], z["results"].T.copy().view(np.float64).ravel(), z["second"]
    meta = json.loads(z["meta"].tobytes().decode())
    at = {"steps": 0, "results": 0, "second": 0}

    def take(which, flat, shape):
        n = int(np.prod(shape, dtype=np.int64))
        at[which] += n
        return flat[at[which] - n:at[which]].reshape(shape)
    record = {}
    for c in CASES:
        name, call, _, (A, B, M, N, D) = c[:4]
        vshape, gshape = result_shapes(c)
        r = record[name] = dict(meta[name])
        r["X"] = take("steps", steps, (A, M, D))
        r["Y"] = None if call == "sym" else take("steps", steps, (B, N, D))
        r["w"] = None if call in ("mmd", "score") else take("steps", steps, (A,) if call == "paired" else (A, B))
        r["value"], r["grad"] = take("results", results, vshape).astype(c[5]), take("results", results, gshape).astype(c[5])
        r["grad2"] = r["grad"]
        if r["grad2_differs"]:
            r["grad2"] = (r["grad"].astype(np.float64).view(np.int64) + take("second", second, gshape)).view(np.float64).astype(c[5])
    assert at == {"steps": steps.size, "results": results.size, "second": second.size}, at
    return record


def total(launches, word):
    return sum(n for k, n in launches.items() if word in k)


def test_fixture_file_covers_what_it_should():
    assert os.path.getsize(PARENT) < 200 << 10
    record = load()          # (asserts that the file holds exactly what the cases need, end to end)
    for case in CASES:
        r = record[case[0]]
        assert tuple(r["routes"]) == tuple(str(v) for v in case[8]), case[0]
        assert len(r["launches"]) == 3 and all(sum(l.values()) > 0 for l in r["launches"]), case[0]
        assert np.isfinite(r["value"]).all() and np.isfinite(r["grad"]).all() and np.abs(r["grad"]).max() > 0, case[0]
        assert r["grad2_differs"] == (not np.array_equal(r["grad"], r["grad2"])), case[0]
    fwd, bwd, again = record["gram_rbf_one_block_sliced"]["launches"]
    whole = record["gram_rbf_one_band"]["launches"]
    # the small budget: the forward still kept its one block (backward sweeps forward no more than with the whole budget: not at all)
    # and backward took it in two tiles; with nothing kept, a forward sweep per tile
    assert fwd == whole[0] and total(bwd, "k_fwd_fused") == total(whole[1], "k_fwd_fused") == 0
    assert (total(whole[1], "k_adj_fused"), total(bwd, "k_adj_fused")) == (1, 2)
    assert (total(whole[2], "k_fwd_fused"), total(again, "k_fwd_fused")) == (1, 2)
    # increments kept beside the edges: the first backward neither forms them nor sweeps forward; a fraction of 0: it forms them
    kept, no_inc = record["gram_linear_stream_kept_inc"]["launches"], record["gram_linear_stream_no_inc"]["launches"]
    assert [total(l, "k_static_linear_mfma") for l in kept] == [1, 0, 1] and [total(l, "k_static_linear_mfma") for l in no_inc] == [1, 1, 1]
    assert [total(l, "k_fwd_wave") for l in kept] == [total(l, "k_fwd_wave") for l in no_inc] == [1, 0, 1]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_hand_off_is_bit_for_bit_the_parents(case):
    import sigkernel_amd
    name = case[0]
    r = load()[name]
    X, Y, w = tensors(case, r["X"], r["Y"], r["w"])
    with overrides(sigkernel_amd, case):
        assert on_route(sigkernel_amd, case, X, Y) == case[8], name
    val, g1, g2, launches = replay(sigkernel_amd, case, X, Y, w)
    assert launches == r["launches"], (name, launches)
    for got, key in ((val, "value"), (g1, "grad"), (g2, "grad2")):
        want = torch.as_tensor(r[key]).cuda()
        assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want), (name, key)
