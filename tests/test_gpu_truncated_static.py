"""TruncatedSigKernel(static_kernel=RBFKernel(s)) on the GPU: the points mode of k_trunc_sig (csrc/sk_truncated.hip: trunc_points, compiled
into the <4, 1> instance) against the long-double loops of test_truncated_static_host.py, run on the CPU.  The launch trace
(sk_launch_trace) proves which route ran: one launch of k_trunc_sig<4, 1>, none of <1, 2>, one of the prep kernel.

THE BAR, per level m:  |got - want| <= max(4 err_ref[m], n_nodes 2^-53) scale[m]
  * scale[m] = max over pairs of sum_{nodes, planes} |R^m| (level terms are signed and shrink factorially: never max(|want|, 1));
  * err_ref[m]: the CPU fp64 torch restatement's own distance from the loops ON THE SAME INPUTS, in units of scale[m]; the factor 4 is
    the project's allowance for a measured stage (instance_ledger.py);
  * the floor is the worst-case bound for re-ordering a sum of n_nodes terms; n_nodes = Mp Np, the grid the sweep runs on;
  * a weighted value: the levels' bars summed with |sigma[m]|; fp32 in and out: two fp32 ulps of the level more.
Every test prints the errors it measured in units of its bar.

Shapes are (A, B, Mp, Np, D) with Mp, Np in POINTS; inputs are random walks with step std 0.5 and RBFKernel(1.0) unless stated."""
import functools

import numpy as np
import pytest
import torch

from test_truncated_static_host import LD, ld_levels, level_errors, rbf_ld, walks

pytestmark = pytest.mark.gpu

SWEEP, GENERAL, PREP = "k_trunc_sigILi1ELi2E", "k_trunc_sigILi4ELi1E", "k_prep_pair"
BASE = (5, 3, 5, 7, 3)


def traced(fn):
    """fn() with the library counting its launches -> (result, launches of k_trunc_sig<1, 2>, of k_trunc_sig<4, 1>, of k_prep_pair)"""
    from sigkernel_amd import _lib
    was = _lib.launch_trace(True)
    try:
        _lib.launch_counts(reset=True)
        out = fn()
        torch.cuda.synchronize()
        counts = _lib.launch_counts()
    finally:
        _lib.launch_trace(was)
    return (out,) + tuple(sum(n for name, n in counts.items() if tag in name) for tag in (SWEEP, GENERAL, PREP))


def lifted(L, sigma=1., order=1, s=1.0, **kw):
    import sigkernel_amd
    return sigkernel_amd.TruncatedSigKernel(L, sigma, order, static_kernel=sigkernel_amd.RBFKernel(s), **kw)


def signed_sigma(L):
    return torch.tensor([0.5] + [(-1.0) ** m * (1.0 + 0.25 * m) for m in range(1, L + 1)], dtype=torch.float64)


def case(shape, L, seed, s=1.0, paired=False, order=1, dtype="float64"):
    """inputs, the loops' levels and scale, err_ref of the CPU fp64 restatement on the same inputs, and the bar per level -- computed
    once per case and shared; nobody writes to what it returns"""
    return _case(shape, L, seed, s, paired, order, dtype)


@functools.lru_cache(maxsize=None)
def _case(shape, L, seed, s, paired, order, dtype):
    A, B, Mp, Np, D = shape
    rng = np.random.default_rng(seed)
    X, Y = walks(rng, A, Mp, D, dtype), walks(rng, B, Np, D, dtype)
    X64, Y64 = X.astype(np.float64), Y.astype(np.float64)      # the fp32-rounded inputs, exactly
    want, scale = ld_levels(X64, Y64, rbf_ld(s), L, order, paired)
    ref = lifted(L, 1., order, s)._levels(torch.as_tensor(X64), torch.as_tensor(Y64), paired, False)
    err_ref = level_errors(ref, want, scale)
    bar = np.maximum(4 * err_ref, Mp * Np * 2.0 ** -53) * scale.astype(np.float64)
    if dtype == "float32":
        bar = bar + 2 * np.spacing(np.abs(want).reshape(L + 1, -1).max(1).astype(np.float32)).astype(np.float64)
    bar[0] = 0.0
    return X, Y, want, scale, err_ref, bar


def check_levels(got, want, bar, what):
    got = np.asarray(got.detach().cpu().double().numpy(), dtype=LD)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.array([float(np.max(np.abs(got[m] - want[m]))) for m in range(len(bar))])
    print("%s: error / bar per level: %s" % (what, " ".join("%.2g" % (e / b) if b > 0 else "%.2g" % e for e, b in zip(err, bar))))
    assert np.all(err <= bar), (what, err, bar)


def check_weighted(got, want, sigma, bar, what):
    sig = sigma.double().numpy()
    wanted = sum(LD(sig[m]) * want[m] for m in range(len(sig)))
    total = float(np.sum(np.abs(sig) * bar))
    err = float(np.max(np.abs(np.asarray(got.detach().cpu().double().numpy(), dtype=LD) - wanted)))
    print("%s: weighted error / bar: %.2g" % (what, err / total))
    assert got.shape == wanted.shape and err <= total, (what, err, total)


def run_case(shape, L, seed, s=1.0, paired=False, dtype="float64"):
    """levels and a signed weighted value of one case on the GPU: one sweep and one prep launch each, within the bar"""
    X, Y, want, scale, err_ref, bar = case(shape, L, seed, s, paired, 1, dtype)
    Xd, Yd = torch.as_tensor(X).cuda(), torch.as_tensor(Y).cuda()
    sigma = signed_sigma(L)
    lev, n, g, p = traced(lambda: lifted(L, 1., 1, s)._levels(Xd, Yd, paired, False))
    assert (n, g, p) == (0, 1, 1), (n, g, p)
    assert lev.dtype == Xd.dtype
    check_levels(lev, want, bar, "levels %s L=%d s=%g paired=%d %s" % (shape, L, s, paired, dtype))
    tk = lifted(L, sigma, 1, s)
    K, n, g, p = traced(lambda: tk.compute_kernel(Xd, Yd) if paired else tk.compute_Gram(Xd, Yd))
    assert (n, g, p) == (0, 1, 1), (n, g, p)
    check_weighted(K, want, sigma, bar, "weighted %s L=%d" % (shape, L))
    return lev, K


# (5, 3, 5, 7, 3)     an odd row count under two rows per lane, columns no multiple of 16, 16 groups of 4 lanes with A = 5
# (2, 2, 2, 2, 1)     one step a side: every node but one is masked
# (2, 2, 128, 33, 8)  all 64 lanes, 8 levels;  (1, 1, 127, 16, 8): the last lane's second row is padding
# (3, 2, 6, 20, D)    D = 9 and 16: sixteen doubles per point
GRAM = [(BASE, 4), ((2, 2, 2, 2, 1), 1), ((2, 2, 2, 2, 1), 3), ((2, 2, 128, 33, 8), 8), ((1, 1, 127, 16, 8), 8), ((3, 2, 6, 20, 9), 4),
        ((3, 2, 6, 20, 16), 4)]


@pytest.mark.parametrize("shape,L", GRAM)
def test_gram_against_the_loops(shape, L):
    run_case(shape, L, 7000 + shape[2] + 3 * shape[4] + L)


# P = 7, 4 x 40 points: G fd Ncp > 2048 forces fewer, wider groups, and P is no multiple of G;  P = 70, 5 x 7 points: several positions
@pytest.mark.parametrize("shape,L", [((7, 7, 4, 40, 3), 4), ((70, 70, 5, 7, 3), 3)])
def test_paired_against_the_loops(shape, L):
    run_case(shape, L, 7100 + shape[0], paired=True)


def test_levels_mode_at_one_level_is_the_closed_form():
    lev, _ = run_case(BASE, 1, 7201)
    X, Y = case(BASE, 1, 7201)[:2]
    scale, bar = case(BASE, 1, 7201)[3], case(BASE, 1, 7201)[5]
    for a in range(BASE[0]):
        for b in range(BASE[1]):
            kap = rbf_ld(1.0)(X[a].astype(LD), Y[b].astype(LD))
            k1 = kap[-1, -1] - kap[-1, 0] - kap[0, -1] + kap[0, 0]
            assert abs(LD(float(lev[1, a, b])) - k1) <= bar[1], (a, b)
    assert torch.equal(lev[0], torch.ones_like(lev[0]))


def test_levels_mode_every_plane_of_six():
    lev, _ = run_case(BASE, 6, 7202)
    assert lev.shape == (7, BASE[0], BASE[1]) and all(lev[m].is_contiguous() for m in range(7))


def test_swap_when_only_the_second_batch_fits():
    """(3, 2, 200, 100, 2): 200 points are out of scope on the first side, (Y, X) is in: one launch, the result transposed back"""
    from sigkernel_amd import _lib
    shape, L = (3, 2, 200, 100, 2), 3
    assert _lib.load().sk_route_query(_lib.OP_TRUNCATED_RBF, 1, 2, 200, 100, L, 0, 8, 0) == _lib.ROUTE_FUSED_SWAP
    run_case(shape, L, 7300)


@pytest.mark.parametrize("order", [2, 4])
def test_orders_above_one_take_the_restatement(order):
    """the points mode is order 1 only: the route says STREAM, nothing of k_trunc_sig is launched, and the values are the restatement's, on the GPU"""
    from sigkernel_amd import _lib
    shape, L = (3, 2, 9, 7, 3), 4
    assert _lib.load().sk_route_query(_lib.OP_TRUNCATED_RBF, order, 3, 9, 7, L, 0, 8, 0) == _lib.ROUTE_STREAM
    X, Y, want, scale, err_ref, bar = case(shape, L, 7400, 1.0, False, order)
    Xd, Yd = torch.as_tensor(X).cuda(), torch.as_tensor(Y).cuda()
    lev, n, g, p = traced(lambda: lifted(L, 1., order)._levels(Xd, Yd, False, False))
    assert (n, g, p) == (0, 0, 0)
    check_levels(lev, want, bar, "order %d: the restatement on the GPU" % order)


def test_fp32_paths_in_and_out():
    lev, K = run_case(BASE, 4, 7500, dtype="float32")
    assert lev.dtype == torch.float32 and K.dtype == torch.float32


@pytest.mark.parametrize("s", [0.3, 30.0])
def test_bandwidths(s):
    run_case(BASE, 4, 7600, s=s)


def test_a_common_offset_costs_no_digits():
    """100 added to every coordinate of X and Y: the loops on the shifted fp64 inputs, at the bar measured on the UNSHIFTED inputs -- the
    shifted restatement loses digits through RBFKernel.Gram_matrix's expansion and must not loosen it.  Holds only for distances formed
    from differences of coordinates."""
    L = 4
    X, Y, _, _, _, bar = case(BASE, L, 7700)
    Xs, Ys = X + 100.0, Y + 100.0
    want, _ = ld_levels(Xs, Ys, rbf_ld(1.0), L, 1)
    lev, n, g, p = traced(lambda: lifted(L)._levels(torch.as_tensor(Xs).cuda(), torch.as_tensor(Ys).cuda(), False, False))
    assert (n, g, p) == (0, 1, 1)
    check_levels(lev, want, bar, "offset 100")


def test_a_pending_gradient_launches_nothing_and_agrees():
    L = 4
    X, Y, want, scale, err_ref, bar = case(BASE, L, 7800)
    Xd, Yd = torch.as_tensor(X).cuda().requires_grad_(True), torch.as_tensor(Y).cuda()
    sigma = signed_sigma(L)
    K, n, g, p = traced(lambda: lifted(L, sigma)._levels(Xd, Yd, False, False))
    assert (n, g, p) == (0, 0, 0)
    assert K.requires_grad
    check_levels(K, want, bar, "restatement on the GPU, gradient pending")
    K.sum().backward()
    assert Xd.grad is not None and bool(torch.isfinite(Xd.grad).all())


def test_two_calls_give_the_same_bits():
    X, Y = case((2, 2, 128, 33, 8), 8, 7000 + 128 + 24 + 8)[:2]
    Xd, Yd = torch.as_tensor(X).cuda(), torch.as_tensor(Y).cuda()
    tk = lifted(8, signed_sigma(8))
    assert torch.equal(tk.compute_Gram(Xd, Yd), tk.compute_Gram(Xd, Yd))
    P = case((70, 70, 5, 7, 3), 3, 7170, 1.0, True)
    Xp, Yp = torch.as_tensor(P[0]).cuda(), torch.as_tensor(P[1]).cuda()
    tk = lifted(3, signed_sigma(3))
    assert torch.equal(tk.compute_kernel(Xp, Yp), tk.compute_kernel(Xp, Yp))


def test_compute_mmd_is_the_composition_of_three_grams():
    shape, L = (6, 5, 8, 8, 2), 4
    rng = np.random.default_rng(7900)
    X, Y = torch.as_tensor(walks(rng, 6, 8, 2)).cuda(), torch.as_tensor(walks(rng, 5, 8, 2)).cuda()
    tk = lifted(L, signed_sigma(L))
    mmd, n, g, p = traced(lambda: tk.compute_mmd(X, Y))
    assert (n, g, p) == (0, 3, 3)
    K_XX, K_YY, K_XY = tk.compute_Gram(X, X, sym=True), tk.compute_Gram(Y, Y, sym=True), tk.compute_Gram(X, Y)
    want = (K_XX.sum() - K_XX.diag().sum()) / (6 * 5.) + (K_YY.sum() - K_YY.diag().sum()) / (5 * 4.) - 2. * K_XY.mean()
    assert torch.equal(mmd, want)
