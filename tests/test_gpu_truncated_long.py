"""The truncated kernel's LONG mode on the GPU (csrc/sk_truncated.hip: trunc_long, k_trunc_sig<4, 1> with TruncParams::adjoint = 4): row
bands with the carry in a slab, column tiles of the y block.  Every case is held to the torch restatement on CPU fp64 copies of the inputs,
and the launch trace (sk_launch_trace) proves which instance ran.

Bars: fp64 <= 1e-12 of each level's largest entry (the project's; the restatement itself lies within 1e-14 of long double on these shapes,
tests/test_truncated_long_host.py); fp32 I/O rtol 1e-4 / atol 1e-5.  The switch is routes.truncated_long, set by monkeypatch."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_truncated import GENERAL, ORDER1, traced
from test_truncated_host import assert_close, steps

pytestmark = pytest.mark.gpu

ONE = {GENERAL: 1}      # exactly one launch of k_trunc_sig<4, 1>, none of <1, 2>


@pytest.fixture
def long_on(monkeypatch):
    import sigkernel_amd
    monkeypatch.setattr(sigkernel_amd.routes, "truncated_long", True)


def paths(A, B, M, N, D, dtype=np.float64, seed=None):
    rng = np.random.default_rng(1000 * M + N + D if seed is None else seed)
    return torch.as_tensor(steps(rng, A, M, D, dtype)).cuda(), torch.as_tensor(steps(rng, B, N, D, dtype)).cuda()


def reference(X, Y, L, paired=False):
    from sigkernel_amd.truncated import _truncated_levels_torch
    return _truncated_levels_torch(X.detach().double().cpu(), Y.detach().double().cpu(), L, 1, paired)


def level_errors(got, want):
    """per level: the largest deviation over the pairs, of the level's largest entry"""
    got, want = got.double().cpu().reshape(got.shape[0], -1), want.reshape(want.shape[0], -1)
    return ((got - want).abs().max(1).values / want.abs().max(1).values)


def check_levels(got, want, what):
    err = level_errors(got, want)
    print("truncated long %s: level errors %s" % (what, ["%.1e" % float(e) for e in err]))
    assert got.shape == want.shape
    assert float(err.max()) <= 1e-12, (what, err)


# (A, B, M, N, D, L), swept in THIS orientation (no_swap): the second band is one row | two bands x two tiles at fd 8, the second tile one column |
# three bands at fd 16, tiles of 128 + 1 | 300 x 300 | one band, two lane groups with a dead one, rowS across three tiles | one level, no slab |
# more positions than resident blocks: a block's second position meets a used slab
SHAPES = [(2, 3, 129, 130, 4, 8), (2, 2, 130, 257, 8, 8), (2, 2, 257, 129, 9, 3), (1, 2, 300, 300, 8, 8), (3, 2, 40, 600, 3, 6),
          (2, 2, 200, 270, 4, 1), (50, 45, 129, 20, 2, 3)]


@pytest.mark.parametrize("shape", SHAPES)
def test_bands_and_tiles_against_the_restatement(shape):
    from sigkernel_amd import _lib
    A, B, M, N, D, L = shape
    X, Y = paths(A, B, M, N, D)
    be = _lib.get_backend()
    got, hit = traced(lambda: be.truncated_long(X, Y, L, None, False, None, no_swap=True))
    assert hit == ONE, hit
    assert got.dtype == X.dtype and got.is_cuda
    check_levels(got, reference(X, Y, L), shape)


def test_a_workspace_of_two_slabs_leaves_two_blocks():
    """2250 positions on two blocks: every position but a block's first meets a used slab"""
    from sigkernel_amd import _lib
    A, B, M, N, D, L = 50, 45, 129, 20, 2, 3
    plan = (ctypes.c_int64 * 3)()
    block = (L - 1) * 64 * 8
    assert _lib.load().sk_truncated_long_plan(A, B, M, N, D, L, 0, 2 * block + 5, ctypes.cast(plan, ctypes.c_void_p)) == 0
    assert tuple(plan) == (2, block, 2 * block)
    X, Y = paths(A, B, M, N, D)
    got, hit = traced(lambda: _lib.get_backend().truncated_long(X, Y, L, None, False, 2 * block + 5, no_swap=True))
    assert hit == ONE, hit
    check_levels(got, reference(X, Y, L), "two blocks")


def test_a_workspace_below_one_slab_takes_the_restatement(long_on):
    import sigkernel_amd
    A, B, M, N, D, L = 2, 3, 129, 130, 4, 8
    X, Y = paths(A, B, M, N, D)
    got, hit = traced(lambda: sigkernel_amd.truncated_sig_kernel_levels(X, Y, L, 1, workspace_bytes=7 * 192 * 8 - 1))
    assert hit == {}, hit
    check_levels(got, reference(X, Y, L), "restatement")
    got, hit = traced(lambda: sigkernel_amd.truncated_sig_kernel_levels(X, Y, L, 1, workspace_bytes=7 * 192 * 8))
    assert hit == ONE, hit
    check_levels(got, reference(X, Y, L), "one slab")


def test_public_functions_take_the_shorter_orientation(long_on):
    """130 x 257 steps at fd 8: three bands of one tile on (Y, X) against two bands of two tiles -- one launch, transposed back"""
    import sigkernel_amd
    X, Y = paths(2, 3, 130, 257, 8)
    got, hit = traced(lambda: sigkernel_amd.truncated_sig_kernel_levels(X, Y, 8, 1))
    assert hit == ONE and got.shape == (9, 2, 3) and got.is_contiguous()
    check_levels(got, reference(X, Y, 8), "swapped")


def test_paired_levels_and_weighted_sum(long_on):
    import sigkernel_amd
    P, M, N, D, L = 5, 200, 270, 4, 6
    X, Y = paths(P, P, M, N, D)
    lev, hit = traced(lambda: sigkernel_amd.truncated_sig_kernel_levels(X, Y, L, 1, paired=True))
    assert hit == ONE and lev.shape == (L + 1, P)
    want = reference(X, Y, L, paired=True)
    check_levels(lev, want, "paired")
    sigma = torch.as_tensor(np.random.default_rng(3).uniform(0.5, 1.5, L + 1))
    k, hit = traced(lambda: sigkernel_amd.truncated_sig_kernel_paired(X, Y, L, sigma, 1))
    assert hit == ONE and k.shape == (P,)
    ref = (sigma[:, None] * want).sum(0)
    assert float((k.cpu() - ref).abs().max() / ref.abs().max()) <= 1e-12


def test_weighted_gram_is_the_weighted_sum_of_the_levels(long_on):
    import sigkernel_amd
    X, Y = paths(2, 3, 150, 140, 3)
    sigma = torch.as_tensor(np.random.default_rng(4).uniform(0.5, 1.5, 5))
    K, hit = traced(lambda: sigkernel_amd.truncated_sig_kernel(X, Y, 4, sigma, 1))
    assert hit == ONE and K.shape == (2, 3)
    lev = sigkernel_amd.truncated_sig_kernel_levels(X, Y, 4, 1)
    want = sigkernel_amd.truncated_from_levels(lev, sigma.cuda())
    assert float((K - want).abs().max() / want.abs().max()) <= 1e-13
    check_levels(lev, reference(X, Y, 4), "gram levels")


def test_normalize_reaches_the_long_route_through_its_paired_calls(long_on):
    import sigkernel_amd
    from sigkernel_amd.truncated import _truncated_paired_torch, _truncated_torch
    X, Y = paths(2, 3, 150, 140, 3)
    K, hit = traced(lambda: sigkernel_amd.truncated_sig_kernel(X, Y, 4, 1.0, 1, normalize=True))
    assert hit == {GENERAL: 3}, hit
    Xc, Yc = X.cpu(), Y.cpu()
    kx, ky = _truncated_paired_torch(Xc, Xc, 4, 1.0, 1), _truncated_paired_torch(Yc, Yc, 4, 1.0, 1)
    want = _truncated_torch(Xc, Yc, 4, 1.0, 1) / torch.sqrt(kx[:, None] * ky[None, :])
    assert float((K.cpu() - want).abs().max() / want.abs().max()) <= 1e-12


def test_fp32_inputs(long_on):
    import sigkernel_amd
    X, Y = paths(2, 3, 130, 257, 8, np.float32)
    got, hit = traced(lambda: sigkernel_amd.truncated_sig_kernel_levels(X, Y, 6, 1))
    assert hit == ONE and got.dtype == torch.float32
    assert_close(got.cpu().numpy(), reference(X, Y, 6).numpy(), np.float32, "fp32 levels")
    K = sigkernel_amd.truncated_sig_kernel(X, Y, 6, 0.7, 1)
    assert K.dtype == torch.float32
    assert_close(K.cpu().numpy(), (0.7 * reference(X, Y, 6)).sum(0).numpy(), np.float32, "fp32 gram")


def test_both_launches_agree_inside_the_plain_scope():
    from sigkernel_amd import _lib
    X, Y = paths(2, 2, 128, 256, 8)
    be = _lib.get_backend()
    plain, hit = traced(lambda: be.truncated_levels(X, Y, 8, 1))
    assert hit == {ORDER1: 1}, hit
    got, hit = traced(lambda: be.truncated_long(X, Y, 8, None, False, None, no_swap=True))
    assert hit == ONE, hit
    err = level_errors(got, plain.double().cpu())
    print("long against plain launch: level errors %s, bit-equal %s" % (["%.1e" % float(e) for e in err], torch.equal(got, plain)))
    assert float(err.max()) <= 1e-13


def test_zero_steps_appended_change_nothing():
    """100 steps (one band) against the same paths with 200 zero steps behind them (three bands: the carry runs through two bands of
    nothing), Y of 270 steps (two tiles)"""
    from sigkernel_amd import _lib
    X, Y = paths(2, 2, 100, 270, 5)
    Xp = torch.cat([X, torch.zeros(2, 200, 5, dtype=X.dtype, device=X.device)], 1).contiguous()
    be = _lib.get_backend()
    short, hit = traced(lambda: be.truncated_long(X, Y, 7, None, False, None, no_swap=True))
    assert hit == ONE
    padded, hit = traced(lambda: be.truncated_long(Xp, Y, 7, None, False, None, no_swap=True))
    assert hit == ONE
    err = level_errors(padded, short.cpu())
    print("padded against short: %s" % ["%.1e" % float(e) for e in err])
    assert float(err.max()) <= 1e-13


def test_repeated_calls_are_bit_equal(long_on):
    import sigkernel_amd
    X, Y = paths(3, 3, 257, 300, 6)
    first = sigkernel_amd.truncated_sig_kernel_levels(X, Y, 8, 1)
    for _ in range(4):
        assert torch.equal(sigkernel_amd.truncated_sig_kernel_levels(X, Y, 8, 1), first)


def test_object_front_with_and_without_the_switch(monkeypatch):
    import sigkernel_amd
    rng = np.random.default_rng(11)
    X = torch.cumsum(torch.as_tensor(steps(rng, 3, 200, 4)), 1).cuda()
    Y = torch.cumsum(torch.as_tensor(steps(rng, 2, 200, 4)), 1).cuda()
    tk = sigkernel_amd.TruncatedSigKernel(6)
    off, hit = traced(lambda: tk.compute_Gram(X, Y))
    assert hit == {}, hit                               # the switch is off: the restatement, as before
    monkeypatch.setattr(sigkernel_amd.routes, "truncated_long", True)
    on, hit = traced(lambda: tk.compute_Gram(X, Y))
    assert hit == ONE, hit
    Xg = X.clone().requires_grad_()
    pending, hit = traced(lambda: tk.compute_Gram(Xg, Y))
    assert hit == {} and pending.requires_grad          # a gradient pending: the restatement takes the call
    for other in (off, pending.detach()):
        assert float((on - other).abs().max() / other.abs().max()) <= 1e-12
