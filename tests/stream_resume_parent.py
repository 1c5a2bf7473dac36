"""What the prefix kernel's existing launches returned BEFORE the resume mode (SigKernelStream) went into k_fwd_prefix: the record
tests/golden/stream_resume_parent.npz holds and tests/test_gpu_stream.py replays.

Per static kernel (linear, rbf), dyadic order (0, 1, 2) and the first three SHAPES of tests/test_gpu_prefix_slices.py, fp64 Gram calls:
the three slices of compute_Gram_prefixes and compute_Gram_ragged (seeded lengths) whole; the full grid whole at the first shape and
as the SHA-256 of its bytes at all three (36 x 64 x 63 doubles six times over would not fit a committed file; a digest of the bytes
is the same bit-for-bit statement).  record() runs on whatever build of the package it is given: tests/golden/
make_golden_stream_resume_parent.py hands it the parent commit's, the test this checkout's."""
import hashlib

import numpy as np
import torch

from conftest import walk

DEV = "cuda"
SHAPES = [(3, 5, 9, 14, 3), (5, 3, 33, 20, 8), (6, 6, 64, 63, 4)]      # tests/test_gpu_prefix_slices.py: SHAPES[:3]
KINDS = ["linear", "rbf"]
DYADICS = [0, 1, 2]
SLICES = ["diagonal", "last_row", "last_col"]


def inputs(i):
    A, B, M, N, D = SHAPES[i]
    gen = torch.Generator().manual_seed(7300 + i)
    X, Y = walk(gen, A, M, D), walk(gen, B, N, D)
    lx = torch.randint(1, M + 1, (A,), generator=gen)
    ly = torch.randint(1, N + 1, (B,), generator=gen)
    return X, Y, lx, ly


def digest(t):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).digest(), dtype=np.uint8).copy()


def record(pkg):
    """{name: array} of the calls above on the package `pkg` (a sigkernel_amd module)"""
    out = {}
    for i in range(len(SHAPES)):
        X, Y, lx, ly = inputs(i)
        out["s%d_in" % i] = np.array([float(X.sum()), float(Y.sum()), float(lx.sum()), float(ly.sum())])
        Xd, Yd = X.to(DEV), Y.to(DEV)
        for kind in KINDS:
            for d in DYADICS:
                sk = pkg.SigKernel(pkg.LinearKernel() if kind == "linear" else pkg.RBFKernel(1.0), d)
                key = "s%d_%s_d%d_" % (i, kind, d)
                grid = sk.compute_Gram_prefixes(Xd, Yd)
                out[key + "grid_sha"] = digest(grid)
                if i == 0:
                    out[key + "grid"] = grid.cpu().numpy()
                for nodes in SLICES:
                    out[key + nodes] = sk.compute_Gram_prefixes(Xd, Yd, nodes=nodes).cpu().numpy()
                out[key + "ragged"] = sk.compute_Gram_ragged(Xd, Yd, lx, ly).cpu().numpy()
    torch.cuda.synchronize()
    return out
