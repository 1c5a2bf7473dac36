"""truncated_sig_kernel_paired and truncated_sig_kernel(..., normalize=True) on the GPU: the paired mode of k_trunc_sig
(csrc/sk_truncated.hip: one pair per lane group, each group's y block its own piece of the wave's LDS) against the torch restatement of
the recursion on the CPU and against the diagonal of the Gram launch; the launch trace (sk_launch_trace) proves which route ran.

Bars, those of tests/test_gpu_truncated.py: fp64 <= 1e-12 of the max-norm, fp32 I/O rtol 1e-4 / atol 1e-5.  Bit
equality with the Gram launch is NOT claimed: the paired launch may give a pair a wider lane group, and the butterfly that adds the
lanes' sums up then has more stages."""
import numpy as np
import pytest
import torch

from test_gpu_truncated import GENERAL, ORDER1, expected_instance, traced
from test_truncated_host import assert_close, steps

pytestmark = pytest.mark.gpu

# (P, M, N, D, L, order).  A wave holds G = 64 / W lane groups, W = the power of two >= M rows (order 1: M / 2 rows), G halved until
# G fd ceil16(N) <= 2048 doubles (fd = 8 up to dim 8, else 16).
CASES = [
    # the order <= 4 instance, one row per lane: M 1, 2, 5, 16, 17, 64
    (1, 1, 1, 1, 4, 2),         # W 1 -> 4 (sixteen y blocks of 128 doubles fill the LDS), one live group of 16
    (3, 2, 8, 8, 4, 4),         # W 2 -> 4, 3 of 16 groups live
    (9, 5, 17, 9, 8, 2),        # W 8 -> 16 (fd 16, Ncp 32), 9 pairs on 4 groups: three positions, the last with one live group
    (130, 16, 33, 16, 4, 4),    # W 16 -> 32 (fd 16, Ncp 48), 65 positions, all groups live
    (9, 17, 8, 1, 8, 4),        # W 32, 2 groups, odd P
    (3, 64, 33, 8, 8, 4),       # full width, G 1
    (130, 5, 1, 8, 4, 2),       # W 8, 8 groups: 17 positions, 2 live groups in the last; one column
    (130, 2, 17, 3, 1, -1),     # one level (the order-1 instance by L = 1), W 1 -> 4
    # the order-1 instance, two rows per lane: M 2, 33, 128
    (1, 2, 1, 1, 4, 1),         # one lane per pair by M, W 1 -> 4
    (9, 33, 8, 16, 8, 1),       # odd M: the last lane holds one row; W 32 (17 lanes), G 2
    (130, 128, 33, 8, 4, 1),    # full width
    (3, 33, 17, 1, 8, 1),
    # LDS-forced grouping: M = 8 asks for 8 groups, each y block is 16 x 112 doubles -- only one fits, W 8 -> 64
    (9, 8, 100, 12, 4, 2),
    # more positions than resident single-wave workgroups (2048 on 256 CUs): waves take a second position and stage over the first
    (8200, 16, 9, 3, 3, 2),
]
# only the second batch fits the lanes: the same launch on (Y, X), nothing transposed
SWAPPED = [(9, 70, 30, 4, 3, 2), (3, 130, 64, 8, 4, 1)]


def hip_paired(X, Y, L, sigma, order, **kw):
    import sigkernel_amd
    return traced(lambda: sigkernel_amd.truncated_sig_kernel_paired(X, Y, L, sigma=sigma, order=order, **kw))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", CASES + SWAPPED)
def test_paired_mode_against_the_torch_restatement(shape, dtype):
    import sigkernel_amd
    from sigkernel_amd.truncated import _truncated_paired_torch
    P, M, N, D, L, order = shape
    rng = np.random.default_rng(3000 + M + 7 * N + P)
    # the paths are views of larger buffers: what lies beyond M and N steps (NaN here) must never reach a value
    Xb, Yb = np.full((P, M + 3, D), np.nan, dtype), np.full((P, N + 2, D), np.nan, dtype)
    Xb[:, :M], Yb[:, :N] = steps(rng, P, M, D, dtype), steps(rng, P, N, D, dtype)
    Xb, Yb = torch.as_tensor(Xb).cuda(), torch.as_tensor(Yb).cuda()
    X, Y = Xb[:, :M], Yb[:, :N]
    sigma = torch.as_tensor(rng.uniform(0.5, 1.5, L + 1).astype(dtype))
    got, hit = hip_paired(X, Y, L, sigma, order)
    assert hit == {expected_instance(L, order): 1}, hit
    assert got.shape == (P,) and got.dtype == X.dtype and got.is_cuda
    want = _truncated_paired_torch(X.cpu().double(), Y.cpu().double(), L, sigma.double(), order)
    err = float((got.double().cpu() - want).abs().max() / want.abs().max())
    print("paired %s P %d M %d N %d D %d L %d order %d: max-norm error %.3g, launches %s" % (np.dtype(dtype).name, P, M, N, D, L, order, err, hit))
    assert_close(got.cpu().numpy(), want.numpy(), dtype, shape)
    # the diagonal of the Gram launch (the Gram of 8200 paths is 67 M pairs for 8200 values: the first 130 pairs stand for it)
    Q = min(P, 130)
    diag = sigkernel_amd.truncated_sig_kernel(X[:Q], Y[:Q], L, sigma=sigma, order=order).diagonal()
    assert_close(got[:Q].cpu().numpy(), diag.cpu().numpy(), dtype, (shape, "diagonal"))
    # repeated calls, and other values behind the views' ends: the same bits
    Xb[:, M:], Yb[:, N:] = 7.0, -3.0
    for _ in range(2):
        assert torch.equal(sigkernel_amd.truncated_sig_kernel_paired(X, Y, L, sigma=sigma, order=order), got)
    # numpy in, numpy out
    if P <= 9:
        kn = sigkernel_amd.transforms.truncated_sig_kernel_paired(X.cpu().numpy(), Y.cpu().numpy(), L, sigma=sigma.numpy(), order=order)
        assert isinstance(kn, np.ndarray) and kn.dtype == dtype and np.array_equal(kn, got.cpu().numpy())


def test_backend_entry_point_states_its_scope():
    """HipBackend.truncated_paired: (P,) inside sk_route_query(SK_OP_TRUNCATED) == FUSED, None outside, exactly as truncated_gram"""
    from sigkernel_amd import _lib
    from sigkernel_amd.truncated import _truncated_paired_torch
    be = _lib.get_backend()
    rng = np.random.default_rng(4)
    X, Y = torch.as_tensor(steps(rng, 3, 70, 4)).cuda(), torch.as_tensor(steps(rng, 3, 30, 4)).cuda()
    w = [1.0, 0.5, 2.0, 0.25]
    assert be.truncated_paired(X, Y, 3, w, 2) is None                           # 70 rows at order 2: only (y, x) fits
    assert_close(be.truncated_paired(Y, X, 3, w, 2).cpu().numpy(), _truncated_paired_torch(X.cpu(), Y.cpu(), 3, w, 2).numpy(), np.float64)
    assert be.truncated_paired(X, X, 3, w, 2) is None                           # neither way: the caller's torch restatement
    assert_close(be.truncated_paired(X, Y, 3, w, 1).cpu().numpy(), _truncated_paired_torch(X.cpu(), Y.cpu(), 3, w, 1).numpy(), np.float64)


def test_shapes_outside_the_kernel_take_the_torch_route():
    from sigkernel_amd.truncated import _truncated_paired_torch
    rng = np.random.default_rng(6)
    for P, M, N, D, L, order in [(3, 65, 66, 4, 3, 2), (3, 20, 15, 17, 3, 1), (2, 10, 9, 4, 6, 5)]:
        X, Y = torch.as_tensor(steps(rng, P, M, D)).cuda(), torch.as_tensor(steps(rng, P, N, D)).cuda()
        got, hit = hip_paired(X, Y, L, 0.9, order)
        assert hit == {}
        assert_close(got.cpu().numpy(), _truncated_paired_torch(X.cpu(), Y.cpu(), L, 0.9, order).numpy(), np.float64, (P, M, N, D, L, order))


def test_normalised_gram_matrix():
    """5 x 7 paths of 9 x 8 steps: one Gram launch and two paired ones; on (X, X) one paired launch and a unit diagonal"""
    import sigkernel_amd
    from sigkernel_amd.truncated import _truncated_paired_torch, _truncated_torch
    rng = np.random.default_rng(12)
    X, Y = torch.as_tensor(steps(rng, 5, 9, 3)).cuda(), torch.as_tensor(steps(rng, 7, 8, 3)).cuda()
    sig = torch.as_tensor(rng.uniform(0.5, 1.5, 5))
    for order, tag in ((2, GENERAL), (1, ORDER1)):
        K, hit = traced(lambda: sigkernel_amd.truncated_sig_kernel(X, Y, 4, sigma=sig, order=order, normalize=True))
        assert hit == {tag: 3}, hit
        Xc, Yc = X.cpu(), Y.cpu()
        kx, ky = _truncated_paired_torch(Xc, Xc, 4, sig, order), _truncated_paired_torch(Yc, Yc, 4, sig, order)
        want = _truncated_torch(Xc, Yc, 4, sig, order) / torch.sqrt(kx[:, None] * ky[None, :])
        assert K.shape == (5, 7)
        assert_close(K.cpu().numpy(), want.numpy(), np.float64, order)
        S, hit = traced(lambda: sigkernel_amd.truncated_sig_kernel(X, X, 4, sigma=sig, order=order, normalize=True))
        assert hit == {tag: 2}, hit
        print("normalised (X, X) order %d: diagonal off 1 by %.3g" % (order, float((S.diagonal() - 1).abs().max())))
        assert float((S.diagonal() - 1).abs().max()) <= 1e-14
        # the default: the plain matrix, one launch, the same bits with and without the keyword
        P0, hit = traced(lambda: sigkernel_amd.truncated_sig_kernel(X, Y, 4, sigma=sig, order=order, normalize=False))
        assert hit == {tag: 1} and torch.equal(P0, sigkernel_amd.truncated_sig_kernel(X, Y, 4, sigma=sig, order=order))
    with pytest.raises(ValueError, match="`X`"):
        sigkernel_amd.truncated_sig_kernel(10 * X, Y, 1, sigma=torch.as_tensor([1.0, -1.0]), normalize=True)


def test_inputs_that_require_grad_take_the_differentiable_route():
    import sigkernel_amd
    from sigkernel_amd.truncated import _truncated_paired_torch
    rng = np.random.default_rng(11)
    Xc, Yc = torch.as_tensor(steps(rng, 3, 4, 2)), torch.as_tensor(steps(rng, 3, 3, 2))
    sig = torch.as_tensor(rng.uniform(0.5, 1.5, 5))
    w = torch.as_tensor(rng.standard_normal(3))
    for order in (-1, 1, 2):
        Xh, Yh = Xc.clone().requires_grad_(), Yc.clone().requires_grad_()
        (_truncated_paired_torch(Xh, Yh, 4, sig, order) * w).sum().backward()
        Xg, Yg = Xc.cuda().requires_grad_(), Yc.cuda().requires_grad_()
        k, hit = hip_paired(Xg, Yg, 4, sig, order)
        assert hit == {} and k.requires_grad
        (k * w.cuda()).sum().backward()
        with torch.no_grad():       # forward only: the same tensors go through the kernel
            k0, hit = hip_paired(Xg, Yg, 4, sig, order)
        assert sum(hit.values()) == 1
        assert_close(k.detach().cpu().numpy(), k0.cpu().numpy(), np.float64, ("values", order))
        for got, want, what in ((Xg.grad, Xh.grad, "dX"), (Yg.grad, Yh.grad, "dY")):
            err = float((got.cpu() - want).abs().max() / want.abs().max())
            assert err <= 1e-10, (what, order, err)
    # the normalised matrix with a gradient: the matrix and both diagonals on the torch route, autograd through the quotient
    from sigkernel_amd.truncated import _truncated_torch
    Xg, Yg = Xc.cuda().requires_grad_(), Yc.cuda().requires_grad_()
    Kn, hit = traced(lambda: sigkernel_amd.truncated_sig_kernel(Xg, Yg, 4, sigma=sig, order=2, normalize=True))
    assert hit == {} and Kn.requires_grad
    W = torch.as_tensor(rng.standard_normal((3, 3)))
    (Kn * W.cuda()).sum().backward()
    Xh, Yh = Xc.clone().requires_grad_(), Yc.clone().requires_grad_()
    kx, ky = _truncated_paired_torch(Xh, Xh, 4, sig, 2), _truncated_paired_torch(Yh, Yh, 4, sig, 2)
    (_truncated_torch(Xh, Yh, 4, sig, 2) / torch.sqrt(kx[:, None] * ky[None, :]) * W).sum().backward()
    for got, want, what in ((Xg.grad, Xh.grad, "dX"), (Yg.grad, Yh.grad, "dY")):
        err = float((got.cpu() - want).abs().max() / want.abs().max())
        assert err <= 1e-10, (what, "normalised", err)
    with torch.no_grad():
        K0, hit = traced(lambda: sigkernel_amd.truncated_sig_kernel(Xg, Yg, 4, sigma=sig, order=2, normalize=True))
    assert hit == {GENERAL: 3}
    assert_close(Kn.detach().cpu().numpy(), K0.cpu().numpy(), np.float64, "normalised values")
    # a batch that needs no gradient keeps its diagonal on the kernel: one paired launch, for ky
    Kn, hit = traced(lambda: sigkernel_amd.truncated_sig_kernel(Xc.cuda().requires_grad_(), Yc.cuda(), 4, sigma=sig, order=2, normalize=True))
    assert hit == {GENERAL: 1} and Kn.requires_grad
    assert_close(Kn.detach().cpu().numpy(), K0.cpu().numpy(), np.float64, "normalised values, dX only")


def test_nothing_of_the_gram_matrix_size_is_allocated():
    """2048 pairs of 64 x 64 steps, dim 4, four levels.  The (2048, 2048) Gram call needs 16.8 MB of fp64 staging (8 doubles per step of
    either batch) and 33.6 MB of output.  A paired call with its DEFAULT workspace stages the same 16.8 MB in one launch -- a third of that
    sum, and all of it the paths' own staging: checked against staging + 2048 values.  Held to a tenth of the sum (5.0 MB), the call has
    to be told so: workspace_bytes bounds the staging, the batch then goes in several launches and the values are the same bits."""
    import sigkernel_amd
    P, M, D, L = 2048, 64, 4, 4
    rng = np.random.default_rng(13)
    X, Y = torch.as_tensor(steps(rng, P, M, D)).cuda(), torch.as_tensor(steps(rng, P, M, D)).cuda()
    sigkernel_amd.truncated_sig_kernel_paired(X[:2], Y[:2], L)          # warm-up: library handles, caches
    staging = 8 * 8 * (M + M) * P
    gram_needs = staging + P * P * 8

    def rise_of(**kw):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        k, hit = hip_paired(X, Y, L, 1.0, -1, **kw)
        return k, hit, torch.cuda.max_memory_allocated() - base

    k, hit, rise = rise_of()
    print("paired call, default workspace: peak rises by %d bytes (staging %d, Gram staging + output %d)" % (rise, staging, gram_needs))
    assert hit == {GENERAL: 1}
    assert rise <= staging + 8 * P + (1 << 16), rise
    k4, hit, rise = rise_of(workspace_bytes=4 << 20)
    print("paired call, workspace_bytes = 4 MiB: peak rises by %d bytes in %d launches" % (rise, hit[GENERAL]))
    assert rise < gram_needs / 10, rise
    assert hit == {GENERAL: 4} and torch.equal(k4, k)          # 512 pairs (4 MiB of staging) at a time
