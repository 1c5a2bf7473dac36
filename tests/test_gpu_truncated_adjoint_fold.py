"""TruncatedSigKernel's four gradient routes on the GPU, bit for bit against the build before their host code was folded into one route
record, one autograd function, one predicate, one plan and one launcher (tests/golden/truncated_adjoint_fold_parent.npz, recorded on the
GPU from the parent commit by tests/golden/make_golden_truncated_adjoint_fold.py; the routes promise reproducible bits, and the maker
ran every case twice).  Every value and every gradient must be equal (np.array_equal) and every call must launch each instance of
k_trunc_sig as often as it did.  The shapes are the smallest that reach each branch: both sides requiring grad, sym, the paired runs of
three pairs, fp32, the paired widening at 16 coordinates, two row bands with two column tiles, the long gradient on (Y, X) alone, a lowered block
count, and without a keyword the restatement.  The three points cases were re-recorded after trunc_points / trunc_points_adjoint began to
round the first difference D once before using it (equal rows then give g = 0 exactly: CHANGELOG, "Truncated-kernel value regimes"),
which moved their values by <= 3.1e-16 relative; every other entry of the file came out bit-identical in that recording."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_gpu_truncated import GENERAL, ORDER1, traced

PARENT = os.path.join(ROOT, "tests", "golden", "truncated_adjoint_fold_parent.npz")

# one pair's fp64 staging at (M, N, D) = (9, 8, 3): 8 bytes x fd = 8 doubles x (9 rows + 8 columns padded to 16)
THREE_PAIRS = 3 * 8 * 8 * (9 + 16)
ONE_BLOCK = "one block"     # workspace_bytes: eight bytes above one block's slab, from the long adjoint's plan entry

WIDE, LONG, POINTS = dict(wide_adjoint=True), dict(long_adjoint=True), dict(points_adjoint=True, rbf=0.7)

# name, route keywords, call, (A, B, M, N, D) in STEPS (the points route: POINTS), num_levels, dtype, who requires grad, sym, workspace_bytes
CASES = [
    ("plain_gram", {}, "gram", (5, 7, 9, 8, 3), 4, np.float64, "xy", False, None),
    ("plain_sym", {}, "gram", (5, 5, 9, 9, 3), 4, np.float64, "x", True, None),
    # three pairs a run -- and a workspace that holds no block's slab of 3 x 15 KB: the route declines as a whole, as in the parent
    ("plain_paired", {}, "kernel", (9, 9, 9, 8, 3), 4, np.float64, "xy", False, THREE_PAIRS),
    ("plain_paired_runs", {}, "kernel", (9, 9, 9, 8, 3), 1, np.float64, "x", False, THREE_PAIRS),    # one level has no slab: three runs a launch site
    ("plain_fp32_mmd", {}, "mmd", (5, 7, 9, 8, 3), 4, np.float32, "xy", False, None),
    ("wide_gram", WIDE, "gram", (5, 7, 9, 8, 9), 4, np.float64, "xy", False, None),
    ("wide_paired", WIDE, "kernel", (5, 5, 9, 33, 16), 3, np.float64, "x", False, None),             # the lane groups widen: 16 x 48 doubles a y block
    ("wide_sym", WIDE, "gram", (3, 3, 9, 9, 10), 4, np.float64, "x", True, None),
    ("long_gram", LONG, "gram", (2, 2, 130, 260, 3), 3, np.float64, "xy", False, None),              # two row bands, two column tiles
    ("long_swapped", LONG, "gram", (2, 2, 40, 130, 3), 3, np.float64, "y", False, None),             # the gradient's sweep is the one on (Y, X)
    ("long_paired", LONG, "kernel", (3, 3, 130, 20, 3), 3, np.float64, "xy", False, None),
    ("long_one_block", LONG, "gram", (1, 2, 130, 20, 1), 3, np.float64, "x", False, ONE_BLOCK),      # the block count lowered from 2 to 1
    ("points_gram", POINTS, "gram", (5, 7, 10, 9, 3), 4, np.float64, "xy", False, None),
    ("points_sym", POINTS, "gram", (5, 5, 10, 10, 3), 4, np.float64, "x", True, None),
    ("points_paired", POINTS, "kernel", (6, 6, 10, 9, 8), 4, np.float64, "xy", False, None),
    ("no_keyword_dim9", {}, "gram", (2, 3, 4, 3, 9), 4, np.float64, "x", False, None),               # the restatement, as in the parent
    ("no_keyword_130_steps", {}, "gram", (1, 2, 130, 5, 1), 3, np.float64, "x", False, None),
]


def one_block_workspace(lib, case):
    """eight bytes above ONE block's slab of the case's long-adjoint launch on (X, Y): plan[3] of the plan entry point"""
    A, B, M, N, D = case[3]
    out = (ctypes.c_int64 * 4)()
    rc = lib.sk_truncated_long_adjoint_plan(A, B, M, N, D, case[4], 0, 1 << 40, ctypes.cast(out, ctypes.c_void_p))
    assert rc == 0 and out[1] > 1 and out[3] > 0, (rc, tuple(out))
    return int(out[3]) + 8


def lattice(seed, shape):
    """integers in [-128, 127], the same on every machine and numpy: the top byte of a mixed 64-bit counter (no generator's stream is relied on)"""
    v = np.arange(1, int(np.prod(shape, dtype=np.int64)) + 1, dtype=np.uint64) + np.uint64(seed * 0x9E3779B97F4A7C15 % 2 ** 64)
    for shift, mult in ((30, 0xBF58476D1CE4E5B9), (27, 0x94D049BB133111EB)):
        v = (v ^ (v >> np.uint64(shift))) * np.uint64(mult)         # (wraps modulo 2^64)
    return ((v ^ (v >> np.uint64(31))) >> np.uint64(56)).astype(np.int64).reshape(shape) - 128


def inputs(case):
    """(X, Y or None where Y is X, sigma, c) of a case as numpy arrays: PATHS of M and N steps -- the points route: of M and N points --
    the level weights and the weights of the sum that is differentiated.  Every number is a small integer times a power of two
    (`lattice`), exact in fp32 too, so the record holds no inputs: the maker and the test both build them here."""
    name, kw, call, (A, B, M, N, D), L, dtype, grads, sym, ws = case
    seed = 10 * CASES.index(case)
    pts = 0 if "rbf" in kw else 1       # a path of M steps has M + 1 points
    scale = 2.0 ** -(9 + (D > 4) + (D > 9))     # steps of norm <= 1/2 or so
    path = lambda k, n, m: np.concatenate([np.zeros((n, 1, D)), np.cumsum(lattice(seed + k, (n, m + pts - 1, D)) * scale, 1)], 1).astype(dtype)
    X = path(1, A, M)
    Y = None if sym else path(2, B, N)
    c = lattice(seed + 3, () if call == "mmd" else (A,) if call == "kernel" else (A, B)) / 64.0
    return X, Y, 1.0 + lattice(seed + 4, (L + 1,)) / 256.0, c


def replay(sigkernel_amd, case, X, Y, sigma, c, ws):
    """the case's call and its weighted-sum backward on device tensors -> ((value, dX or None, dY or None), {instance tag: launches})"""
    name, kw, call, shape, L, dtype, grads, sym, _ = case
    kw = dict(kw)
    static = sigkernel_amd.RBFKernel(kw.pop("rbf")) if "rbf" in kw else None
    tk = sigkernel_amd.TruncatedSigKernel(L, sigma, 1, workspace_bytes=ws, static_kernel=static, **kw)

    def fn():
        x = X.detach().clone().requires_grad_("x" in grads)
        y = x if sym else Y.detach().clone().requires_grad_("y" in grads)
        K = tk.compute_Gram(x, y, sym=sym) if call == "gram" else tk.compute_kernel(x, y) if call == "kernel" else tk.compute_mmd(x, y)
        (K * c.to(K.dtype)).sum().backward()
        return K.detach(), x.grad, None if sym else y.grad
    return traced(fn)


def test_fixture_file_covers_what_it_should():
    z = np.load(PARENT)
    assert os.path.getsize(PARENT) < 100 << 10
    launches = {}
    for case in CASES:
        name, kw, call, (A, B, M, N, D), L, dtype, grads, sym, ws = case
        X, Y, sigma, c = inputs(case)
        assert X.shape == (A, M + (0 if "rbf" in kw else 1), D) and X.dtype == dtype and np.array_equal(X, X.astype(np.float32)), name
        assert z[name + "_K"].shape == c.shape and z[name + "_K"].dtype == dtype, name
        assert ((name + "_dX") in z) == ("x" in grads) and ((name + "_dY") in z) == ("y" in grads and not sym), name
        for g, src in (("_dX", X), ("_dY", Y)):
            if name + g in z:
                assert z[name + g].shape == src.shape and z[name + g].dtype == dtype and np.abs(z[name + g]).max() > 0, name
        launches[name] = (int(z[name + "_launches"][0]), int(z[name + "_launches"][1]))      # (ORDER1, GENERAL)
    # forward + one adjoint launch per batch that requires grad; the plain route is <1, 2>'s, every other adjoint <4, 1>'s
    assert launches["plain_gram"] == (3, 0) and launches["plain_sym"] == (2, 0) and launches["plain_fp32_mmd"] == (7, 0)
    assert launches["plain_paired"] == (0, 0) and launches["plain_paired_runs"] == (6, 0)        # three runs forward, three backward
    assert launches["wide_gram"] == (1, 2) and launches["wide_paired"] == (1, 1) and launches["wide_sym"] == (1, 1)
    assert launches["long_gram"] == (0, 3) and launches["long_swapped"] == (0, 2) and launches["long_paired"] == (0, 3)
    assert launches["long_one_block"] == (0, 2)
    assert launches["points_gram"] == (0, 3) and launches["points_sym"] == (0, 2) and launches["points_paired"] == (0, 3)
    assert launches["no_keyword_dim9"] == (0, 0) and launches["no_keyword_130_steps"] == (0, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_values_gradients_and_launches_are_the_parents(case):
    import sigkernel_amd
    from sigkernel_amd import _lib
    z = np.load(PARENT)
    name, sym, ws = case[0], case[7], case[8]
    if ws == ONE_BLOCK:
        ws = one_block_workspace(_lib.load(), case)
        assert ws == int(z[name + "_ws"])
    X, Y, sigma, c = inputs(case)
    X = torch.as_tensor(X).cuda()
    Y = X if sym else torch.as_tensor(Y).cuda()
    (K, dX, dY), hit = replay(sigkernel_amd, case, X, Y, torch.as_tensor(sigma), torch.as_tensor(c).cuda(), ws)
    assert (hit.get(ORDER1, 0), hit.get(GENERAL, 0)) == tuple(int(v) for v in z[name + "_launches"]), (name, hit)
    for key, got in (("_K", K), ("_dX", dX), ("_dY", dY)):
        assert (got is None) == (name + key not in z), (name, key)
        if got is not None:
            want = z[name + key]
            assert got.is_cuda and got.cpu().numpy().dtype == want.dtype and got.shape == want.shape, (name, key)
            assert np.array_equal(got.cpu().numpy(), want), (name, key)
