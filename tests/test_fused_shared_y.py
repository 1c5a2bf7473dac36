"""The fused forward's SHARED-Y pair order (sk_wave_fused.hip, FusedParams::shy_A): in a plain Gram launch without edges the lane groups
of a wave sweep the same y_b against G different x_a and share one y ring.

* GPU: compute_Gram through the fused route against the CPU oracle at the fast kernels' tolerance (1e-12 relative, as in
  test_gpu_parity.py), over the shapes where the order matters: A odd, A < G, A = 1, B = 1, A not a multiple of G for G = 2, 4, 8,
  dims 3 and 8, both static kernels, dyadic 0..2, a launch that draws from the queue and one that uses the age-rank shares.
* GPU: the launches that keep the pair-per-group order (symmetric Gram, a forward that keeps edges for a pending gradient, paired
  compute_kernel) return, bit for bit, what the commit before this order returned for the same inputs on an MI355X
  (tests/golden/fused_shared_y_fallback.npz, written by fallback_outputs() below), and agree with the oracle.
* CPU: the position -> pair mapping, restated in Python, is a bijection onto [0, A) x [0, B).
"""
import os

import numpy as np
import pytest
import torch

import sigkernel_amd
from sigkernel_amd import _lib
from oracle import oracle as O

FAST_TOL = 1e-12
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_shared_y_fallback.npz")

# A, B, points of x, points of y, dims, static kernel, dyadic -- with the lane groups per wave (G) the launcher gives the shape
CASES = [
    (5, 7, 128, 128, 8, "linear", 1),      # G = 2, A odd
    (1, 9, 128, 100, 8, "linear", 1),      # G = 2, A = 1 < G
    (7, 5, 128, 128, 3, "linear", 0),      # G = 2, dims 3 (the four-dimension variant), dyadic 0
    (3, 5, 60, 60, 3, "linear", 1),        # G = 4, A < G
    (9, 1, 60, 40, 8, "linear", 1),        # G = 4, B = 1
    (6, 11, 60, 60, 8, "linear", 0),       # G = 4, A not a multiple of G
    (11, 6, 30, 30, 3, "linear", 1),       # G = 8
    (5, 4, 12, 20, 8, "linear", 1),        # G = 8, A < G
    (13, 4, 12, 12, 8, "linear", 2),       # G = 4 (one row per lane at dyadic 2)
    (21, 3, 30, 30, 8, "linear", 2),       # G = 2
    (7, 5, 60, 60, 8, "rbf", 1),           # G = 2 (two rows per lane)
    (3, 4, 30, 30, 8, "rbf", 1),           # G = 4, A < G
    (9, 5, 30, 30, 3, "rbf", 0),           # G = 8, four-dimension variant
    (5, 6, 12, 12, 3, "rbf", 1),           # G = 8
    (6, 5, 30, 26, 8, "rbf", 2),           # G = 2
    (7, 3, 12, 12, 3, "rbf", 2),           # G = 4
    (301, 257, 30, 30, 3, "linear", 1),    # G = 8: 38 row groups x 257 columns, several chunks per wave
    (64, 512, 128, 128, 8, "linear", 1),   # fills the chip without the queue: shares by age rank
    (512, 512, 128, 128, 8, "linear", 1),  # the headline launch: the queue
]


def lane_groups(M, kind, D, dyadic):
    """Lane groups per wave of the one-band fused forward WITHOUT edges (launch_fwd_fused: rows per lane by fused_rcx, 8 lanes at least)."""
    nd = 4 if D <= 4 else 8
    if dyadic == 1:
        rc = 4 if (kind == "linear" or nd == 4) else 2
    elif dyadic == 2:
        rc = 1
    else:
        rc = 2 if (kind == "rbf" and nd == 8) else 4
    rows = M if kind == "rbf" else M - 1
    L = 8
    while L < 64 and rc * L < rows:
        L *= 2
    assert rc * L >= rows
    return 64 // L


def position_to_pair(q, g, A, B, G):
    """Stream position q of lane group g -> (a, b), or None when the group has no pair there."""
    a, b = G * (q // B) + g, q % B
    return (a, b) if a < A else None


@pytest.mark.parametrize("A,B,M,N,D,kind,dyadic", CASES)
def test_positions_map_onto_every_pair_once(A, B, M, N, D, kind, dyadic):
    G = lane_groups(M, kind, D, dyadic)
    assert G >= 2
    n_pos = (A + G - 1) // G * B
    seen = np.zeros((A, B), np.int32)
    for q in range(n_pos):
        some = False
        for g in range(G):
            ab = position_to_pair(q, g, A, B, G)
            if ab is not None:
                seen[ab] += 1
                some = True
        assert some                      # no position is empty: lane group 0 always has a pair
        assert position_to_pair(q, 0, A, B, G) is not None
    assert seen.min() == 1 and seen.max() == 1
    # the positions of one pair's neighbours in a row group share b: that is what lets the groups share the y ring
    for q in (0, n_pos // 2, n_pos - 1):
        bs = {position_to_pair(q, g, A, B, G)[1] for g in range(G) if position_to_pair(q, g, A, B, G)}
        assert len(bs) == 1


def _walk(gen, A, M, D):
    return torch.cumsum(torch.randn(A, M, D, generator=gen, dtype=torch.float64), dim=1) / np.sqrt(M * D)


def _kernel(kind):
    return sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(0.75)


def _rel_err(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _fused_launches():
    return sum(v for k, v in _lib.launch_counts(reset=True).items() if "k_fwd_fusedI" in k)


@pytest.mark.gpu
@pytest.mark.parametrize("A,B,M,N,D,kind,dyadic", CASES)
def test_gram_in_shared_y_order_matches_the_oracle(A, B, M, N, D, kind, dyadic):
    gen = torch.Generator().manual_seed(1000 * A + B + dyadic)
    X, Y = _walk(gen, A, M, D), _walk(gen, B, N, D)
    sk = sigkernel_amd.SigKernel(_kernel(kind), dyadic_order=dyadic)
    was = _lib.launch_trace(True)
    try:
        _lib.launch_counts(reset=True)
        K = sk.compute_Gram(X.to(DEV), Y.to(DEV)).cpu().numpy()
        torch.cuda.synchronize()
        assert _fused_launches() == 1, "the call did not take the one-band fused forward"
    finally:
        _lib.launch_trace(was)
    want = O.gram_forward(X, Y, _kernel(kind), dyadic, nthreads=min(16, O.max_threads()))
    assert K.shape == want.shape == (A, B)
    err = _rel_err(K, want)
    print("shared-y %s A=%d B=%d M=%d N=%d D=%d d=%d: rel err %.3e" % (kind, A, B, M, N, D, dyadic, err))
    assert err <= FAST_TOL


# ---- the launches that keep the pair-per-group order ----------------------------------------------------------------------------

FALLBACK_SHAPES = [   # name, A, B, M, D, static kernel, dyadic
    ("lin_d1", 7, 5, 60, 8, "linear", 1),
    ("rbf_d1", 6, 6, 30, 3, "rbf", 1),
]


def fallback_inputs():
    out = {}
    for name, A, B, M, D, kind, dyadic in FALLBACK_SHAPES:
        gen = torch.Generator().manual_seed(77 + A + M)
        out[name + "_X"] = _walk(gen, A, M, D).numpy()
        out[name + "_Y"] = _walk(gen, B, M, D).numpy()
    return out


def fallback_outputs(inp):
    """{name: array}: symmetric Gram of X, Gram with a gradient pending on X (the forward keeps edges) and its gradient, paired kernel."""
    out = {}
    for name, A, B, M, D, kind, dyadic in FALLBACK_SHAPES:
        X, Y = torch.from_numpy(inp[name + "_X"]).to(DEV), torch.from_numpy(inp[name + "_Y"]).to(DEV)
        sk = sigkernel_amd.SigKernel(_kernel(kind), dyadic_order=dyadic)
        out[name + "_sym"] = sk.compute_Gram(X, X, sym=True).cpu().numpy()
        Xg = X.clone().requires_grad_(True)
        K = sk.compute_Gram(Xg, Y)
        out[name + "_edges"] = K.detach().cpu().numpy()
        K.sum().backward()
        out[name + "_grad"] = Xg.grad.cpu().numpy()
        n = min(A, B)
        out[name + "_paired"] = sk.compute_kernel(X[:n], Y[:n]).cpu().numpy()
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
def test_pair_per_group_launches_are_what_they_were():
    gold = np.load(GOLDEN)
    inp = {k: gold[k] for k in fallback_inputs()}      # the recorded inputs themselves, not a second draw
    got = fallback_outputs(inp)
    for name, A, B, M, D, kind, dyadic in FALLBACK_SHAPES:
        X, Y = torch.from_numpy(inp[name + "_X"]), torch.from_numpy(inp[name + "_Y"])
        for what in ("sym", "edges", "grad", "paired"):
            assert np.array_equal(got[name + "_" + what], gold[name + "_" + what]), "%s_%s is not bit-identical" % (name, what)
        assert _rel_err(got[name + "_sym"], O.gram_forward(X, X, _kernel(kind), dyadic)) <= FAST_TOL
        assert _rel_err(got[name + "_edges"], O.gram_forward(X, Y, _kernel(kind), dyadic)) <= FAST_TOL
        n = min(A, B)
        assert _rel_err(got[name + "_paired"], np.diagonal(O.gram_forward(X[:n], Y[:n], _kernel(kind), dyadic))) <= FAST_TOL
