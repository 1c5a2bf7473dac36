"""The fused forward's carried y-ring address (sk_wave_fused.hip).  In the linear sweep without edges and with two or more lane
groups per wave a lane no longer advances and wraps its own read address: at the end of a macro-step it takes the address of the
lane above (lane l reads at step t the stream unit lane l - 1 read at step t - 1), and the first lane of every lane group receives
the group's fresh address -- a scalar ring offset that runs on the scalar unit, added to the lane's ring base -- inside the EXEC
window that already sets its top row to 1.0.  The ring's layout (slabs, parity swizzle, wrap) and every byte a lane reads are what
they were, so every result is, bit for bit, what the commit before the change returned.

GPU cases
* compare compute_Gram / compute_kernel with the CPU oracle at the fast kernels' bar (1e-12 relative, FAST_TOL of
  test_fused_producers.py), and
* require bit equality with tests/golden/fused_carried_y_parent.npz: the outputs of the PARENT commit's build for the same seeded
  inputs, recorded once on an MI355X by record_golden() below (run with the parent's package first on sys.path).

Shapes: the headline instance (linear, dyadic 1, 8 dims, 128 points on x: 32 lanes per pair, two lane groups, four rows per lane)
with an x batch of 5 (odd: the shared-y order reaches a >= A) against y batches of 3 and 7 of 128, 65, 17 and 9 points: the ring
wraps several times per pair, once, and a pair is one slab, each with a half-filled last unit.  The pair-per-group orders, whose lane
groups each own a ring (symmetric Gram, paired compute_kernel, compute_mmd with its gradient), the four-dimension variant, and the
instances that keep the per-lane address (RBF, dyadic 0 on short paths = eight lane groups; the full-wave and edge-keeping ones run
inside compute_mmd's gradient and in `full`).

The CPU test restates the scalar recurrence of the first lane and the hand-down in plain Python and checks it against the closed
form of the address (slab, parity swizzle, wrap) for every ring size the launcher can choose.
"""
import os

import numpy as np
import pytest
import torch

import sigkernel_amd
from oracle import oracle as O

FAST_TOL = 1e-12
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_carried_y_parent.npz")

# name, what, A, B, points of x, points of y, dims, static kernel, dyadic
CASES = [("y%d_b%d" % (N, B), "gram", 5, B, 128, N, 8, "linear", 1) for B in (3, 7) for N in (128, 65, 17, 9)] + [
    ("sym", "sym", 5, 5, 128, 128, 8, "linear", 1),          # symmetric Gram: a ring per lane group
    ("paired", "paired", 7, 7, 128, 65, 8, "linear", 1),     # paired compute_kernel
    ("mmd", "mmd", 4, 4, 128, 65, 8, "linear", 1),           # compute_mmd (the loss layout) and its gradient
    ("nd4", "gram", 5, 3, 128, 65, 4, "linear", 1),          # ND = 4
    ("rbf", "gram", 5, 3, 60, 33, 3, "rbf", 1),              # RBF keeps the per-lane address
    ("d0", "gram", 5, 7, 30, 17, 8, "linear", 0),            # dyadic 0
    ("full", "gram", 3, 2, 200, 65, 8, "linear", 1),         # one lane group per wave keeps the per-lane address
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
    gen = torch.Generator().manual_seed(7300 + 89 * IDS.index(name))
    return _walk(gen, A, M, D), _walk(gen, B, N, D)


def _outputs(case):
    """{key: numpy array} of what the case computes on the GPU."""
    name, what, A, B, M, N, D, kind, dyadic = case
    X, Y = _inputs(case)
    sk = sigkernel_amd.SigKernel(_kernel(kind), dyadic_order=dyadic)
    out = {name + "_in": np.array([float(X.sum()), float(Y.sum())])}      # the inputs are the recorded ones
    if what == "gram":
        out[name + "_K"] = sk.compute_Gram(X.to(DEV), Y.to(DEV)).cpu().numpy()
    elif what == "sym":
        out[name + "_K"] = sk.compute_Gram(X.to(DEV), X.to(DEV), sym=True).cpu().numpy()
    elif what == "paired":
        out[name + "_K"] = sk.compute_kernel(X.to(DEV), Y.to(DEV)).cpu().numpy()
    else:
        Xg = X.to(DEV).requires_grad_()
        mmd = sk.compute_mmd(Xg, Y.to(DEV))
        mmd.backward()
        out[name + "_mmd"] = mmd.detach().cpu().numpy()
        out[name + "_grad"] = Xg.grad.cpu().numpy()
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
def test_carried_address_keeps_every_bit_and_matches_the_oracle(case, gold):
    name, what, A, B, M, N, D, kind, dyadic = case
    X, Y = _inputs(case)
    got = _outputs(case)
    nt = min(16, O.max_threads())
    want = {}
    if what == "gram":
        want[name + "_K"] = O.gram_forward(X, Y, _kernel(kind), dyadic, nthreads=nt)
    elif what == "sym":
        want[name + "_K"] = O.gram_forward(X, X, _kernel(kind), dyadic, nthreads=nt)
    elif what == "paired":
        want[name + "_K"] = np.diagonal(O.gram_forward(X, Y, _kernel(kind), dyadic, nthreads=nt))
    errs = {k: _rel_err(got[k], v) for k, v in want.items()}
    same = {k: bool(np.array_equal(got[k], gold[k])) for k in got}
    print("carried y %s: oracle rel err %s, bit-identical to the parent %s" % (name, errs, same))
    assert same[name + "_in"], "the seeded inputs are not the recorded ones"
    for k, v in want.items():
        assert got[k].shape == v.shape
        assert errs[k] <= FAST_TOL, (k, errs[k])
    for k in got:
        assert same[k], "%s is not bit-identical to the parent commit's output" % k


# ---- the address, restated -------------------------------------------------------------------------------------------------------------
def _closed_form(v, L, pitch, grp_par):
    """Byte offset in its ring of virtual stream unit v (may be negative: a lane that has not started): slab v // 8 in ring slot
    (v // 8) mod NSLAB, unit v mod 8 at 16 bytes each, odd slabs (by slab number plus the lane group's parity) 128 bytes on."""
    nslab = (L >> 3) + 2
    s = v // 8
    return (s % nslab) * pitch + ((v & 7) << 4) + (((s + grp_par) & 1) << 7)


def _scalar_step(off, t, pitch, ring_bytes):
    """The first lane's offset after macro-step t, from the one before: the per-lane advance of the parent, on the scalar unit."""
    off += 16
    if ((t + 1) & 7) == 0:      # the first lane's unit number is t itself: lam7 = 0
        e = (off + pitch - 128) ^ 128
        off = e - (ring_bytes if e >= ring_bytes else 0)
    return off


@pytest.mark.parametrize("nd", [4, 8])
@pytest.mark.parametrize("L", [8, 16, 32, 64])
def test_carried_address_is_the_closed_form(L, nd):
    pitch = nd * 128
    nslab = (L >> 3) + 2
    ring_bytes = nslab * pitch
    period = 16 * nslab                      # steps after which slot and parity both repeat
    for grp_par in (0, 1):
        base = 256 * 5 * (1 + grp_par)       # a 256-byte aligned ring base, as the wave slices and the rings are
        # what every lane holds before step 0: the closed form, once (lanes below L only exist when lam < L; 64 covers every lam)
        held = [base + _closed_form(-lam, L, pitch, grp_par) for lam in range(64)]
        off = 0
        for t in range(4 * period):
            for lam in range(64):
                want = base + _closed_form(t - lam, L, pitch, grp_par)
                assert held[lam] == want, (L, nd, grp_par, t, lam)
                # the 16-byte reads at (a, a ^ 128) + 0, 256, .. stay inside the ring
                for a in (held[lam], held[lam] ^ 128):
                    assert base <= a and a + (nd // 2 - 1) * 256 + 16 <= base + ring_bytes
            off = _scalar_step(off, t, pitch, ring_bytes)
            assert 0 <= off < ring_bytes
            # every lane takes the address of the lane above; the first lane the scalar offset, parity folded in by XOR, plus its base
            held = [((off ^ (grp_par << 7)) + base)] + held[:-1]
