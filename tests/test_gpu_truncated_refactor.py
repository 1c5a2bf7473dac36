"""The truncated kernel's host side on the GPU, bit for bit against the build before its three modes were folded into one recursion, one
tiler, one HIP call and one route (tests/golden/truncated_refactor_parent.npz, recorded on the GPU from the parent commit by
tests/golden/make_golden_truncated_refactor_parent.py).  The plain Gram and paired launches are pinned by
test_gpu_truncated_levels.py::test_plain_launches_are_bit_for_bit_the_parents; these calls reach what that one does not: the levels mode
on both instances, the (Y, X) route with its transpose, the paired chunker and its join axis, normalisation with and without the saved
launch, the fp32 output and fd = 16 staging.  Every output must be equal (np.array_equal) and every call must launch what it launched."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_gpu_truncated import GENERAL, ORDER1, traced
from test_truncated_host import steps

PARENT = os.path.join(ROOT, "tests", "golden", "truncated_refactor_parent.npz")

# one pair's fp64 staging at (M, N, D) = (9, 8, 3): 8 bytes x fd = 8 doubles x (9 rows + 8 columns padded to 16)
THREE_PAIRS = 3 * 8 * 8 * (9 + 16)

# name, call, (A, B, M, N, D), num_levels, order, dtype, workspace_bytes, weighted?, Y is X?
CASES = [
    ("levels_general", "levels", (5, 7, 9, 8, 3), 4, 2, np.float64, None, False, False),
    ("levels_order1", "levels", (5, 7, 9, 8, 3), 4, 1, np.float64, None, False, False),             # two rows per lane
    ("levels_swapped", "levels", (3, 2, 70, 30, 4), 3, 2, np.float64, None, False, False),          # only (Y, X) fits: transposed back
    ("levels_paired", "levels_paired", (9, 9, 9, 8, 3), 4, 2, np.float64, None, False, False),
    ("levels_paired_chunked", "levels_paired", (9, 9, 9, 8, 3), 4, 2, np.float64, THREE_PAIRS, False, False),   # three launches, axis 1
    ("levels_paired_swapped", "levels_paired", (3, 3, 70, 30, 4), 3, 2, np.float64, None, False, False),
    ("paired_chunked", "paired", (9, 9, 9, 8, 3), 4, 2, np.float64, THREE_PAIRS, True, False),                  # three launches, axis 0
    ("normalized", "normalized", (5, 7, 9, 8, 3), 4, 2, np.float64, None, True, False),             # one Gram launch and two paired
    ("normalized_same", "normalized", (5, 5, 9, 9, 3), 4, 2, np.float64, None, True, True),         # ... one paired: Y is X
    ("gram_fp32", "gram", (5, 7, 9, 8, 3), 4, 2, np.float32, None, True, False),
    ("gram_dim9", "gram", (5, 7, 9, 8, 9), 4, 2, np.float64, None, True, False),                    # fd = 16
]


def inputs(case):
    """(X, Y or None where Y is X, sigma or None) of a case as numpy arrays -- what the maker records; the test reads the record"""
    name, call, (A, B, M, N, D), L, order, dtype, ws, weighted, same = case
    rng = np.random.default_rng(len(name) + 100 * CASES.index(case))
    X = steps(rng, A, M, D, dtype)
    Y = None if same else steps(rng, B, N, D, dtype)
    return X, Y, (rng.uniform(0.5, 1.5, L + 1) if weighted else None)


def replay(sigkernel_amd, case, X, Y, sigma):
    """the case's public call on device tensors -> (result, {instance tag: launches})"""
    name, call, shape, L, order, dtype, ws, weighted, same = case
    if call == "levels":
        fn = lambda: sigkernel_amd.truncated_sig_kernel_levels(X, Y, L, order=order, workspace_bytes=ws)
    elif call == "levels_paired":
        fn = lambda: sigkernel_amd.truncated_sig_kernel_levels(X, Y, L, order=order, paired=True, workspace_bytes=ws)
    elif call == "paired":
        fn = lambda: sigkernel_amd.truncated_sig_kernel_paired(X, Y, L, sigma=sigma, order=order, workspace_bytes=ws)
    else:
        fn = lambda: sigkernel_amd.truncated_sig_kernel(X, Y, L, sigma=sigma, order=order, workspace_bytes=ws, normalize=call == "normalized")
    return traced(fn)


def test_fixture_file_covers_what_it_should():
    z = np.load(PARENT)
    assert os.path.getsize(PARENT) < 100 << 10
    for case in CASES:
        name, call, (A, B, M, N, D), L = case[:4]
        lead = (L + 1,) if call.startswith("levels") else ()
        assert z[name + "_out"].shape == lead + ((A,) if "paired" in call else (A, B)), name
        assert z[name + "_out"].dtype == case[5] and z[name + "_X"].shape == (A, M, D)
    launches = {c[0]: (int(z[c[0] + "_launches"][0]), int(z[c[0] + "_launches"][1])) for c in CASES}      # (ORDER1, GENERAL)
    assert launches["levels_order1"] == (1, 0) and launches["levels_general"] == (0, 1) and launches["levels_swapped"] == (0, 1)
    assert launches["levels_paired_chunked"] == (0, 3) and launches["paired_chunked"] == (0, 3) and launches["levels_paired"] == (0, 1)
    assert launches["normalized"] == (0, 3) and launches["normalized_same"] == (0, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_calls_are_bit_for_bit_the_parents(case):
    import sigkernel_amd
    z = np.load(PARENT)
    name = case[0]
    X = torch.as_tensor(z[name + "_X"]).cuda()
    Y = X if case[-1] else torch.as_tensor(z[name + "_Y"]).cuda()
    sigma = torch.as_tensor(z[name + "_sigma"]) if case[-2] else None
    got, hit = replay(sigkernel_amd, case, X, Y, sigma)
    want = z[name + "_out"]
    assert (hit.get(ORDER1, 0), hit.get(GENERAL, 0)) == tuple(int(v) for v in z[name + "_launches"]), (name, hit)
    assert got.is_cuda and got.is_contiguous() and got.cpu().numpy().dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got.cpu().numpy(), want), name
