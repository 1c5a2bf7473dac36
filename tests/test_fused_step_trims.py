"""The fused forward's step-loop trims (sk_wave_fused.hip): the top row of a block is the neighbour lane's values with the first lane
of every lane group set to 1.0 under an EXEC mask (no selects), the linear sweep without edges resets a lane's K state in the block
that fetches its x rows (one pair-start block per step, one per-lane constant less), and the y ring address advances in place.
None of it touches the arithmetic: every result is, bit for bit, what the commit before the trims returned.

Each case
* compares compute_Gram / compute_kernel with the CPU oracle at the fast kernels' bar (1e-12 relative, FAST_TOL of
  test_fused_shared_y.py; gradients at test_gpu_parity.py's ADJ_TOL = 1e-10), and
* requires bit equality with tests/golden/fused_step_trims.npz: the outputs of the PARENT commit's build for the same seeded inputs,
  recorded once on an MI355X by record_golden() below (run with the parent's package first on sys.path).

Shapes: the smallest at which the touched code can go wrong -- the top lane of a second, fourth and eighth lane group with several
pairs per group (pair starts fall mid-stream), one lane group per wave (the full-wave branch, which must be unchanged), dyadic 2 and
the four-dimension variant, RBF (the sweep cursor trails the reload), the edge-keeping forward with its gradient, and the paired /
symmetric launches.
"""
import os

import numpy as np
import pytest
import torch

import sigkernel_amd
from oracle import oracle as O

FAST_TOL = 1e-12
ADJ_TOL = 1e-10
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_step_trims.npz")

# name, what, A, B, points of x, points of y, dims, static kernel, dyadic
CASES = [
    ("g2", "gram", 5, 7, 128, 128, 8, "linear", 1),          # two lane groups: the headline instance
    ("g4", "gram", 6, 11, 60, 60, 8, "linear", 0),           # four lane groups
    ("g8", "gram", 11, 6, 30, 30, 3, "linear", 1),           # eight lane groups
    ("g8_few", "gram", 5, 4, 12, 20, 8, "linear", 1),        # eight lane groups, A < G
    ("full", "gram", 3, 3, 200, 200, 8, "linear", 1),        # one lane group per wave
    ("d2", "gram", 13, 4, 12, 12, 8, "linear", 2),           # dyadic 2
    ("nd4", "gram", 7, 5, 128, 128, 3, "linear", 0),         # the four-dimension variant
    ("rbf", "gram", 7, 5, 60, 60, 8, "rbf", 1),              # RBF: the trailing sweep cursor
    ("rbf_nd4", "gram", 9, 5, 30, 30, 3, "rbf", 0),
    ("edges", "grad", 5, 7, 128, 128, 8, "linear", 1),       # the edge-keeping forward and its gradient
    ("edges_rbf", "grad", 3, 4, 30, 30, 8, "rbf", 1),
    ("pairsym", "pairsym", 9, 9, 60, 60, 8, "linear", 1),    # paired compute_kernel and the symmetric Gram
]
IDS = [c[0] for c in CASES]


def _walk(gen, A, M, D):
    return torch.cumsum(torch.randn(A, M, D, generator=gen, dtype=torch.float64), dim=1) / np.sqrt(M * D)


def _kernel(kind):
    return sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(0.75)


def _rel_err(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _inputs(case):
    name, what, A, B, M, N, D, kind, dyadic = case
    gen = torch.Generator().manual_seed(4100 + 97 * IDS.index(name))
    X, Y = _walk(gen, A, M, D), _walk(gen, B, N, D)
    w = torch.randn(A, B, generator=gen, dtype=torch.float64)
    return X, Y, w


def _outputs(case):
    """{key: numpy array} of what the case computes on the GPU."""
    name, what, A, B, M, N, D, kind, dyadic = case
    X, Y, w = _inputs(case)
    sk = sigkernel_amd.SigKernel(_kernel(kind), dyadic_order=dyadic)
    out = {name + "_in": np.array([float(X.sum()), float(Y.sum()), float(w.sum())])}      # the inputs are the recorded ones
    if what == "gram":
        out[name + "_K"] = sk.compute_Gram(X.to(DEV), Y.to(DEV)).cpu().numpy()
    elif what == "grad":
        Xg = X.to(DEV).requires_grad_()
        K = sk.compute_Gram(Xg, Y.to(DEV))
        out[name + "_K"] = K.detach().cpu().numpy()
        (K * w.to(DEV)).sum().backward()
        out[name + "_grad"] = Xg.grad.cpu().numpy()
    else:
        out[name + "_paired"] = sk.compute_kernel(X.to(DEV), Y.to(DEV)).cpu().numpy()
        out[name + "_sym"] = sk.compute_Gram(X.to(DEV), X.to(DEV), sym=True).cpu().numpy()
    torch.cuda.synchronize()
    return out


def record_golden(path=GOLDEN):
    """Write the golden file from whatever build of the package is imported: run ONCE with the parent commit's build on an MI355X."""
    out = {}
    for case in CASES:
        out.update(_outputs(case))
    np.savez_compressed(path, **out)
    return path


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN, allow_pickle=False))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_step_trims_keep_every_bit_and_match_the_oracle(case, gold):
    name, what, A, B, M, N, D, kind, dyadic = case
    X, Y, w = _inputs(case)
    got = _outputs(case)
    nt = min(16, O.max_threads())
    want = {}
    if what in ("gram", "grad"):
        want[name + "_K"] = O.gram_forward(X, Y, _kernel(kind), dyadic, nthreads=nt)
    if what == "grad":
        want[name + "_grad"] = O.gram_grad_weighted(X, Y, w.numpy(), _kernel(kind), dyadic, nthreads=nt)
    if what == "pairsym":
        want[name + "_paired"] = np.diagonal(O.gram_forward(X, Y, _kernel(kind), dyadic, nthreads=nt))
        want[name + "_sym"] = O.gram_forward(X, X, _kernel(kind), dyadic, nthreads=nt)
    errs = {k: _rel_err(got[k], v) for k, v in want.items()}
    same = {k: bool(np.array_equal(got[k], gold[k])) for k in got}
    print("step trims %s: oracle rel err %s, bit-identical to the parent %s" % (name, errs, same))
    assert same[name + "_in"], "the seeded inputs are not the recorded ones"
    for k, v in want.items():
        assert got[k].shape == v.shape
        assert errs[k] <= (ADJ_TOL if k.endswith("_grad") else FAST_TOL), (k, errs[k])
    for k in got:
        assert same[k], "%s is not bit-identical to the parent commit's output" % k
