"""The fused forward's producers (sk_wave_fused.hip): what a producer fetches changes only where its stream position does, so the
look-up of a position -- chunk, ring, bounds, the pair's (a, b) -- runs once, in the visit that opens the position, and is parked in
the lanes of one VGPR for the visits that follow; the division by B behind it is a multiply and a shift (div_magic,
sk_pair_stream.h), also in the store branch.  None of it touches the arithmetic.

* Shared-y Grams at the shapes where a parked position or a multiply-shift can go wrong, against the CPU oracle at the bar of
  test_fused_shared_y.py (1e-12 relative); every call must have taken the one-band fused forward.
* The pair-per-group orders (symmetric Gram, a Gram with a gradient pending, paired compute_kernel, the loss layout of compute_mmd):
  bit for bit what the PARENT commit's build returned, tests/golden/fused_producers_parent.npz, recorded once on an MI355X by
  record_golden() below (run with the parent's package first on sys.path).
* CPU: the launcher's multiplier and shift (sk_pair_div_magic) against integer division.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import sigkernel_amd
from sigkernel_amd import _lib
from oracle import oracle as O

FAST_TOL = 1e-12
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_producers_parent.npz")

# A, B, points, dims, dyadic, static kernel
CASES = [
    (9, 1, 60, 8, 1, "linear"),        # B = 1: every position is a new row group
    (5, 2, 30, 3, 1, "linear"),        # B = 2, eight lane groups
    (4, 3, 12, 8, 1, "linear"),        # A < G, B = 3
    (37, 251, 30, 3, 1, "linear"),     # prime B, no multiple of any chunk size: chunk entries land mid-row
    (301, 257, 30, 3, 1, "linear"),    # several drawn chunks per wave
    (64, 512, 128, 8, 1, "linear"),    # the age-rank shares
    (70, 641, 30, 8, 0, "linear"),     # B with a wide multiplier
    (6, 6, 30, 3, 1, "rbf"),
    (7, 5, 60, 8, 1, "rbf"),
]
IDS = ["%dx%d_%dpt_%dd_dy%d_%s" % c for c in CASES]


def _walk(gen, A, M, D):
    return torch.cumsum(torch.randn(A, M, D, generator=gen, dtype=torch.float64), dim=1) / np.sqrt(M * D)


def _kernel(kind):
    return sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(0.75)


def _rel_err(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _fused_launches():
    return sum(v for k, v in _lib.launch_counts(reset=True).items() if "k_fwd_fusedI" in k)


@pytest.mark.gpu
@pytest.mark.parametrize("A,B,M,D,dyadic,kind", CASES, ids=IDS)
def test_gram_with_parked_positions_matches_the_oracle(A, B, M, D, dyadic, kind):
    gen = torch.Generator().manual_seed(5200 + 31 * A + B)
    X, Y = _walk(gen, A, M, D), _walk(gen, B, M, D)
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
    print("producers %s A=%d B=%d M=%d D=%d d=%d: rel err %.3e" % (kind, A, B, M, D, dyadic, err))
    assert err <= FAST_TOL


# ---- the pair-per-group orders: bit for bit the parent build's ---------------------------------------------------------------------
def _group_inputs():
    gen = torch.Generator().manual_seed(5311)
    return {"X9": _walk(gen, 9, 30, 3), "X5": _walk(gen, 5, 30, 3), "Y7": _walk(gen, 7, 30, 3), "Y6": _walk(gen, 6, 30, 3),
            "w": torch.randn(5, 7, generator=gen, dtype=torch.float64)}


def group_outputs():
    """{name: array} of the launches that give every lane group its own run of pairs, and how many fused forwards each took."""
    inp = _group_inputs()
    sk = sigkernel_amd.SigKernel(sigkernel_amd.LinearKernel(), dyadic_order=1)
    out = {"in": np.array([float(v.sum()) for v in inp.values()])}
    n = {}
    was = _lib.launch_trace(True)
    try:
        _lib.launch_counts(reset=True)
        out["sym"] = sk.compute_Gram(inp["X9"].to(DEV), inp["X9"].to(DEV), sym=True).cpu().numpy()
        n["sym"] = _fused_launches()
        Xg = inp["X5"].to(DEV).requires_grad_()
        K = sk.compute_Gram(Xg, inp["Y7"].to(DEV))
        n["edges"] = _fused_launches()
        out["edges_K"] = K.detach().cpu().numpy()
        (K * inp["w"].to(DEV)).sum().backward()
        out["edges_grad"] = Xg.grad.cpu().numpy()
        _lib.launch_counts(reset=True)
        out["paired"] = sk.compute_kernel(inp["X9"].to(DEV), inp["X9"].flip(0).to(DEV)).cpu().numpy()
        n["paired"] = _fused_launches()
        Xm = inp["X5"].to(DEV).requires_grad_()
        mmd = sk.compute_mmd(Xm, inp["Y6"].to(DEV))
        n["mmd"] = _fused_launches()
        out["mmd"] = mmd.detach().cpu().numpy().reshape(1)
        mmd.backward()
        out["mmd_grad"] = Xm.grad.cpu().numpy()
        torch.cuda.synchronize()
    finally:
        _lib.launch_trace(was)
    return out, n


def record_golden(path=GOLDEN):
    """Write the golden file from whatever build of the package is imported: run ONCE with the parent commit's build on an MI355X."""
    out, _ = group_outputs()
    np.savez_compressed(path, **out)
    return path


@pytest.mark.gpu
def test_pair_per_group_orders_keep_every_bit():
    gold = dict(np.load(GOLDEN, allow_pickle=False))
    got, n = group_outputs()
    same = {k: bool(np.array_equal(got[k], gold[k])) for k in got}
    print("producers, pair-per-group orders: fused forwards %s, bit-identical to the parent %s" % (n, same))
    assert same["in"], "the seeded inputs are not the recorded ones"
    for k, v in n.items():
        assert v >= 1, "%s did not take the one-band fused forward" % k
    assert sorted(got) == sorted(gold)
    for k in got:
        assert same[k], "%s is not bit-identical to the parent commit's output" % k
    # and they are right: the symmetric Gram and the paired kernel against the oracle
    inp = _group_inputs()
    nt = min(16, O.max_threads())
    assert _rel_err(got["sym"], O.gram_forward(inp["X9"], inp["X9"], sigkernel_amd.LinearKernel(), 1, nthreads=nt)) <= FAST_TOL
    want = np.diagonal(O.gram_forward(inp["X9"], inp["X9"].flip(0), sigkernel_amd.LinearKernel(), 1, nthreads=nt))
    assert _rel_err(got["paired"], want) <= FAST_TOL


# ---- CPU: the multiply-shift against integer division --------------------------------------------------------------------------------
P_MAX = 0x7ff00000          # the launchers refuse more pairs (plan_pair_stream)
DIVISORS = [1, 2, 3, 5, 7, 255, 256, 257, 512, 641, 65535, 65537, 6700417, 0x7fefffff]


def _magic(B):
    m, s = ctypes.c_uint32(0), ctypes.c_int(0)
    assert _lib.load().sk_pair_div_magic(B, ctypes.byref(m), ctypes.byref(s)) == 0
    return m.value, s.value


def _div(p, m, s):
    """the kernel's form, mulhi(2 p, m) >> s, in 64-bit integers (2 p < 2^32 and m < 2^32: the product fits)"""
    return ((p.astype(np.uint64) * np.uint64(2) * np.uint64(m)) >> np.uint64(32)) >> np.uint64(s)


@pytest.mark.parametrize("B", DIVISORS)
def test_multiply_shift_is_integer_division(B):
    m, s = _magic(B)
    assert 0 < m < 2 ** 32 and 0 <= s <= 31
    kmax = P_MAX // B                                   # k B < P_MAX for k < kmax (and k = kmax where B does not divide P_MAX)
    ks = np.unique(np.concatenate([np.arange(0, min(1000, kmax + 1)), np.arange(max(0, kmax - 1000), kmax + 1)])).astype(np.int64)
    p = np.concatenate([ks * B - 1, ks * B, ks * B + 1, np.random.default_rng(B).integers(0, P_MAX, size=10 ** 6)])
    p = p[(p >= 0) & (p < P_MAX)]
    got = _div(p, m, s)
    want = (p // B).astype(np.uint64)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "B = %d: p = %d gives %d, not %d" % (B, p[bad[0]], got[bad[0]], want[bad[0]])
    # remainder by multiply-subtract
    assert np.array_equal(p.astype(np.uint64) - got * np.uint64(B), (p % B).astype(np.uint64))


def test_div_magic_refuses_what_it_cannot_divide_by():
    m, s = ctypes.c_uint32(0), ctypes.c_int(0)
    lib = _lib.load()
    assert lib.sk_pair_div_magic(0, ctypes.byref(m), ctypes.byref(s)) == 1
    assert lib.sk_pair_div_magic(-3, ctypes.byref(m), ctypes.byref(s)) == 1
    assert lib.sk_pair_div_magic(2 ** 31, ctypes.byref(m), ctypes.byref(s)) == 1
    assert lib.sk_pair_div_magic(5, None, ctypes.byref(s)) == 1
