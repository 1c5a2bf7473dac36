"""truncated_sig_kernel_levels on the GPU: the public function on the HIP route (k_trunc_sig in its levels mode, csrc/sk_truncated.hip)
against the reference's per-level outputs (tests/golden/truncated_levels.npz) and against the torch restatement on the CPU on shapes
chosen where the mode's epilogue can go wrong; the launch trace (sk_launch_trace) proves which route ran.  And the plain Gram and paired
launches, which share the instances: bit for bit what the build before the mode gave (tests/golden/truncated_levels_parent.npz).

Bars: fp64 <= 1e-12 of EACH LEVEL's own max-norm (on the CPU two summation orders and a long-double evaluation differ by <= 1.5e-15 at
(5, 7, 128, 65, 8) with 8 levels, so the bar hides nothing and the reference meets it; a level that is exactly zero -- order 1 beyond
min(M, N) steps -- must come out exactly zero); fp32 I/O rtol 1e-4 / atol 1e-5, per level."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_gpu_truncated import GENERAL, ORDER1, expected_instance, expected_launches, traced
from test_truncated_host import assert_close, steps

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "truncated_levels.npz")
PARENT = os.path.join(ROOT, "tests", "golden", "truncated_levels_parent.npz")


def assert_levels(got, want, dtype, what=""):
    """got, want (L + 1, ...) arrays: every level against its own max-norm; prints the worst figure before it asserts"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    errs = []
    for m in range(want.shape[0]):
        scale = np.abs(want[m]).max()
        err = np.abs(got[m] - want[m]).max()
        errs.append(err / scale if scale > 0 else (0.0 if err == 0 else np.inf))
    print("levels %s: worst level error %.3g (per level: %s)" % (what, max(errs), " ".join("%.2g" % e for e in errs)))
    for m in range(want.shape[0]):
        if dtype == np.float64:
            assert errs[m] <= 1e-12, (what, "level", m, errs[m])
        else:
            assert_close(got[m], want[m], dtype, (what, "level", m))


def test_hip_route_reproduces_the_reference_levels():
    import sigkernel_amd
    z = np.load(GOLDEN)
    seen = {}
    for c in range(int(z["n_cases"])):
        k = "c%02d_" % c
        X, Y, L, order, want = z[k + "X"], z[k + "Y"], int(z[k + "num_levels"]), int(z[k + "order"]), z[k + "levels"]
        Xd, Yd = torch.as_tensor(X).cuda(), torch.as_tensor(Y).cuda()
        got, hit = traced(lambda: sigkernel_amd.truncated_sig_kernel_levels(Xd, Yd, L, order=order))
        assert hit == expected_launches(L, order), (c, hit)          # (full order five and six: the torch route on the device)
        for tag, n in hit.items():
            seen[tag] = seen.get(tag, 0) + n
        assert got.shape == want.shape and got.dtype == Xd.dtype and got.is_cuda and got.is_contiguous()
        assert_levels(got.cpu().numpy(), want, X.dtype.type, ("fixture", c))
        if X.shape[0] == Y.shape[0]:
            pd, hit = traced(lambda: sigkernel_amd.truncated_sig_kernel_levels(Xd, Yd, L, order=order, paired=True))
            assert hit == expected_launches(L, order), (c, hit)
            assert_levels(pd.cpu().numpy(), np.stack([np.diagonal(v) for v in want]), X.dtype.type, ("fixture paired", c))
    assert seen.get(ORDER1, 0) >= 2 and seen.get(GENERAL, 0) >= 2, seen
    # numpy in, numpy out
    Kn = sigkernel_amd.transforms.truncated_sig_kernel_levels(z["c07_X"], z["c07_Y"], 4, order=2)
    assert isinstance(Kn, np.ndarray) and Kn.dtype == np.float64
    assert_levels(Kn, z["c07_levels"], np.float64, "numpy")


# (A, B, M, N, D, L, order).  M: 1, 2, 64, 65 at order 1 (the second row of the last lane is padding), 128, 33 at order 2, 64 at order 4;
# N: 1, 17, 65; D: 1, 8, 9, 16; L: 1 (no row sums at all), 2, 7, 8 (the last level comes from acc at TR_LMAX); A never a multiple of the
# lane groups per wave where there are several (M = 1, 2: 64 or 32 groups; 64 rows at order 1: 2; 7 rows: 8 -- dead groups store nothing).
# D = 1 goes with the SHORT paths only: in one dimension every G[i][j] = x_i y_j carries a random sign and a high level of a long pair is
# what massive cancellation leaves -- at (3, 4, 33, 65, D = 1, L = 8, order 3) two summation orders of the torch restatement ON THE CPU,
# (x, y) and (y, x) transposed, differ by 1.3e-13 at level 7 and 1.8e-12 at level 8 of those levels' max-norms (7.4e-16 at D = 3), so the
# reference itself misses the 1e-12 bar there and the shape can show nothing about the kernel (which sat at 1.7e-12 on it).
SWEEP = [(5, 7, 1, 1, 1, 1, -1), (5, 3, 1, 17, 8, 2, 1), (5, 3, 2, 65, 9, 7, 1), (5, 3, 2, 17, 16, 8, 2), (5, 7, 64, 65, 8, 8, 1),
         (3, 4, 65, 17, 9, 7, 1), (5, 7, 128, 65, 8, 8, 1), (3, 4, 128, 1, 16, 2, 1), (3, 4, 33, 17, 8, 7, 2), (3, 4, 33, 65, 3, 8, 3),
         (3, 4, 64, 65, 16, 8, 4), (3, 2, 64, 17, 9, 2, 2), (67, 3, 7, 17, 3, 8, 4), (3, 4, 64, 1, 8, 1, 1)]
# only the second batch fits the lanes: the same launch on (y, x), every level transposed
SWAPPED = [(3, 4, 65, 33, 8, 8, 4), (3, 4, 129, 65, 8, 7, 1)]
# (P, M, N, D, L, order): P = 1, 5, 300; (5, 2, 65, 8) and (300, 7, 65, 16) are wide enough that the launch widens the groups (64 and 8
# groups of y blocks of 640 and 1280 doubles do not fit a wave's 2048)
PAIRED = [(1, 64, 65, 8, 8, 4), (5, 2, 17, 1, 7, 1), (5, 2, 65, 8, 8, 1), (300, 7, 17, 9, 8, 3), (300, 7, 65, 16, 7, 3), (5, 128, 65, 8, 8, 1),
          (5, 65, 17, 9, 2, 1), (300, 33, 1, 1, 1, 1),
          (5, 129, 17, 8, 2, 1), (5, 65, 33, 8, 7, 3)]          # ... and two that only fit as (y, x): nothing to transpose


def cpu_levels(X, Y, L, order, paired=False):
    from sigkernel_amd.truncated import _truncated_levels_torch
    return _truncated_levels_torch(X.double().cpu(), Y.double().cpu(), L, order, paired).numpy()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", SWEEP + SWAPPED)
def test_levels_against_the_torch_route_on_the_cpu(shape, dtype):
    import sigkernel_amd
    A, B, M, N, D, L, order = shape
    rng = np.random.default_rng(2000 + M + 7 * N + L)
    X, Y = torch.as_tensor(steps(rng, A, M, D, dtype)).cuda(), torch.as_tensor(steps(rng, B, N, D, dtype)).cuda()
    got, hit = traced(lambda: sigkernel_amd.truncated_sig_kernel_levels(X, Y, L, order=order))
    assert hit == {expected_instance(L, order): 1}, hit
    assert got.shape == (L + 1, A, B) and got.dtype == X.dtype and got.is_contiguous()
    assert torch.equal(got[0], torch.ones_like(got[0]))
    assert_levels(got.cpu().numpy(), cpu_levels(X, Y, L, order), dtype, shape)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", PAIRED)
def test_paired_levels_against_the_torch_route_on_the_cpu(shape, dtype):
    import sigkernel_amd
    P, M, N, D, L, order = shape
    rng = np.random.default_rng(3000 + M + 7 * N + L)
    X, Y = torch.as_tensor(steps(rng, P, M, D, dtype)).cuda(), torch.as_tensor(steps(rng, P, N, D, dtype)).cuda()
    got, hit = traced(lambda: sigkernel_amd.truncated_sig_kernel_levels(X, Y, L, order=order, paired=True))
    assert hit == {expected_instance(L, order): 1}, hit
    assert got.shape == (L + 1, P) and got.dtype == X.dtype
    assert torch.equal(got[0], torch.ones_like(got[0]))
    assert_levels(got.cpu().numpy(), cpu_levels(X, Y, L, order, True), dtype, shape)


def test_paired_staging_is_bounded_by_the_workspace():
    import sigkernel_amd
    rng = np.random.default_rng(31)
    X, Y = torch.as_tensor(steps(rng, 11, 7, 3)).cuda(), torch.as_tensor(steps(rng, 11, 5, 3)).cuda()
    whole = sigkernel_amd.truncated_sig_kernel_levels(X, Y, 4, order=2, paired=True)
    parts, hit = traced(lambda: sigkernel_amd.truncated_sig_kernel_levels(X, Y, 4, order=2, paired=True, workspace_bytes=4 * 8 * 8 * (7 + 16)))
    assert hit == {GENERAL: 3}, hit                 # four pairs per launch
    assert torch.equal(parts, whole)


@pytest.mark.parametrize("shape", [(5, 7, 64, 65, 8, 8, 4), (5, 7, 128, 65, 8, 8, 1), (9, 4, 20, 33, 3, 6, 2), (3, 4, 65, 33, 8, 8, 4)])
def test_weighted_levels_are_the_truncated_kernel_of_the_same_device(shape):
    """sum_m sigma[m] levels[m] against truncated_sig_kernel on the same device, 1e-12 of the matrix's max-norm; and paired"""
    import sigkernel_amd
    A, B, M, N, D, L, order = shape
    rng = np.random.default_rng(41 + M)
    X, Y = torch.as_tensor(steps(rng, A, M, D)).cuda(), torch.as_tensor(steps(rng, B, N, D)).cuda()
    sigma = torch.as_tensor(rng.uniform(0.5, 1.5, L + 1))
    lv = sigkernel_amd.truncated_sig_kernel_levels(X, Y, L, order=order)
    want = sigkernel_amd.truncated_sig_kernel(X, Y, L, sigma=sigma, order=order)
    got = sigkernel_amd.truncated_from_levels(lv, sigma)
    assert got.is_cuda and got.shape == want.shape
    err = float((got - want).abs().max() / want.abs().max())
    print("weighted levels %s: %.3g" % (shape, err))
    assert err <= 1e-12
    assert float(((lv * sigma.cuda()[:, None, None]).sum(0) - want).abs().max() / want.abs().max()) <= 1e-12
    P = min(A, B)
    pd = sigkernel_amd.truncated_sig_kernel_levels(X[:P], Y[:P], L, order=order, paired=True)
    wantp = sigkernel_amd.truncated_sig_kernel_paired(X[:P], Y[:P], L, sigma=sigma, order=order)
    assert float((sigkernel_amd.truncated_from_levels(pd, sigma) - wantp).abs().max() / wantp.abs().max()) <= 1e-12
    # a learnable weight vector: the levels come from the kernel, the gradient from torch
    s = sigma.cuda().requires_grad_()
    c = torch.as_tensor(rng.standard_normal((A, B))).cuda()
    (sigkernel_amd.truncated_from_levels(lv, s) * c).sum().backward()
    wantg = (lv * c).sum((1, 2))
    assert float((s.grad - wantg).abs().max() / wantg.abs().max()) <= 1e-13     # the same A B products, summed in another order


@pytest.mark.parametrize("shape", [(37, 29, 64, 65, 8, 8, 4), (37, 29, 128, 65, 8, 8, 1), (300, 9, 20, 33, 3, 6, 2)])
def test_repeated_calls_are_bitwise_identical(shape):
    import sigkernel_amd
    A, B, M, N, D, L, order = shape
    rng = np.random.default_rng(2)
    X, Y = torch.as_tensor(steps(rng, A, M, D)).cuda(), torch.as_tensor(steps(rng, B, N, D)).cuda()
    first = sigkernel_amd.truncated_sig_kernel_levels(X, Y, L, order=order)
    firstp = sigkernel_amd.truncated_sig_kernel_levels(X[:9], Y[:9], L, order=order, paired=True)
    for _ in range(4):
        assert torch.equal(sigkernel_amd.truncated_sig_kernel_levels(X, Y, L, order=order), first)
        assert torch.equal(sigkernel_amd.truncated_sig_kernel_levels(X[:9], Y[:9], L, order=order, paired=True), firstp)


def test_inputs_that_require_grad_take_the_differentiable_route():
    import sigkernel_amd
    from sigkernel_amd.truncated import _truncated_torch
    rng = np.random.default_rng(11)
    Xc, Yc = torch.as_tensor(steps(rng, 2, 4, 2)), torch.as_tensor(steps(rng, 2, 3, 2))
    w = torch.as_tensor(rng.uniform(0.5, 1.5, 5))
    c = torch.as_tensor(rng.standard_normal((2, 2)))
    for order in (-1, 1, 2):
        Xh, Yh = Xc.clone().requires_grad_(), Yc.clone().requires_grad_()
        (_truncated_torch(Xh, Yh, 4, w, order) * c).sum().backward()
        Xg, Yg = Xc.cuda().requires_grad_(), Yc.cuda().requires_grad_()
        lv, hit = traced(lambda: sigkernel_amd.truncated_sig_kernel_levels(Xg, Yg, 4, order=order))
        assert hit == {} and lv.requires_grad
        (sigkernel_amd.truncated_from_levels(lv, w) * c.cuda()).sum().backward()
        assert_close(Xg.grad.cpu().numpy(), Xh.grad.numpy(), np.float64, ("dX", order))
        assert_close(Yg.grad.cpu().numpy(), Yh.grad.numpy(), np.float64, ("dY", order))
        _, hit = traced(lambda: sigkernel_amd.truncated_sig_kernel_levels(Xg, Yg, 4, order=order, paired=True))
        assert hit == {}
        # without a gradient pending the same tensors go through the kernel
        with torch.no_grad():
            _, hit = traced(lambda: sigkernel_amd.truncated_sig_kernel_levels(Xg, Yg, 4, order=order))
        assert sum(hit.values()) == 1


def test_backend_entry_point_states_its_scope():
    from sigkernel_amd import _lib
    be = _lib.get_backend()
    rng = np.random.default_rng(4)
    X, Y = torch.as_tensor(steps(rng, 3, 70, 4)).cuda(), torch.as_tensor(steps(rng, 2, 30, 4)).cuda()
    assert be.truncated_levels(X, Y, 3, 2) is None                          # 70 rows at order 2: only (y, x) fits
    assert be.truncated_levels(X, X[:, :30].contiguous(), 3, 2, paired=True) is None
    Kt = be.truncated_levels(Y, X, 3, 2)
    assert_levels(Kt.transpose(1, 2).cpu().numpy(), cpu_levels(X, Y, 3, 2), np.float64, "backend swapped")
    assert be.truncated_levels(X, Y, 5, 5) is None and be.truncated_levels(Y, X, 5, 5) is None       # order 5: the torch route


def test_plain_launches_are_bit_for_bit_the_parents():
    """The levels mode lives after the step loop of the two instances every plain call launches: three outputs recorded on the GPU from
    the build before the mode existed (order 1, order 4, paired) must come out bit for bit."""
    import sigkernel_amd
    z = np.load(PARENT)
    for name, want_tag in (("order1", ORDER1), ("order4", GENERAL), ("paired", GENERAL)):
        X, Y = torch.as_tensor(z[name + "_X"]).cuda(), torch.as_tensor(z[name + "_Y"]).cuda()
        L, order, sigma = int(z[name + "_num_levels"]), int(z[name + "_order"]), torch.as_tensor(z[name + "_sigma"])
        fn = sigkernel_amd.truncated_sig_kernel_paired if name == "paired" else sigkernel_amd.truncated_sig_kernel
        got, hit = traced(lambda: fn(X, Y, L, sigma=sigma, order=order))
        assert hit == {want_tag: 1}, (name, hit)
        assert np.array_equal(got.cpu().numpy(), z[name + "_K"]), name


def test_robust_normalised_kernel_end_to_end():
    """levels -> scales -> truncated_from_levels on 6 x 5 paths whose steps are scaled so that some self-kernels exceed C, against the
    same composition of the torch restatement on the CPU.  The levels carry <= 1e-12 each (the bar above); a scale solves
    sum_m lam^(2m) n_m = psi(s), both sides of which take that error, and enters the matrix with powers up to L = 6: two orders of
    magnitude are left for the equation's conditioning and the powers, 1e-10 of the matrix's max-norm."""
    import sigkernel_amd
    from sigkernel_amd.truncated import _truncated_levels_torch, truncated_from_levels, truncated_robust_scales
    rng = np.random.default_rng(51)
    L, order, C = 6, 4, 4.0
    X = torch.as_tensor(steps(rng, 6, 20, 3)) * torch.as_tensor(np.linspace(0.5, 3.0, 6))[:, None, None]
    Y = torch.as_tensor(steps(rng, 5, 13, 3)) * torch.as_tensor(np.linspace(3.0, 0.4, 5))[:, None, None]
    sigma = torch.as_tensor(rng.uniform(0.5, 1.5, L + 1))

    def compose(levels_fn, X, Y):
        nx, ny = levels_fn(X, X, L, order, True), levels_fn(Y, Y, L, order, True)
        lx, ly = truncated_robust_scales(nx, C), truncated_robust_scales(ny, C)
        return truncated_from_levels(levels_fn(X, Y, L, order, False), sigma, lx, ly), lx, ly, nx.sum(0), ny.sum(0)

    want, lx_c, ly_c, sx, sy = compose(lambda x, y, l, o, p: _truncated_levels_torch(x, y, l, o, p), X, Y)
    assert bool((sx > C).any()) and bool((sx <= C).any()) and bool((sy > C).any()) and bool((sy <= C).any())
    (got, lx, ly, _, _), hit = traced(lambda: compose(lambda x, y, l, o, p: sigkernel_amd.truncated_sig_kernel_levels(x, y, l, order=o, paired=p), X.cuda(), Y.cuda()))
    assert hit == {GENERAL: 3}, hit
    assert got.is_cuda and got.shape == (6, 5)
    assert torch.equal(lx.cpu() == 1, lx_c == 1) and torch.equal(ly.cpu() == 1, ly_c == 1)
    serr = max(float((lx.cpu() - lx_c).abs().max()), float((ly.cpu() - ly_c).abs().max()))
    err = float((got.cpu() - want).abs().max() / want.abs().max())
    print("robust end to end: scales differ by %.3g, matrix by %.3g of its max-norm" % (serr, err))
    assert err <= 1e-10
