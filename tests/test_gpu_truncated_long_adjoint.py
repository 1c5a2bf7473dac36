"""TruncatedSigKernel(long_adjoint=True) on the GPU: gradients of the plain truncated kernel beyond the adjoint mode's 128 steps, from the
LONG-ADJOINT mode of k_trunc_sig<4, 1> (csrc/sk_truncated.hip: trunc_long_adjoint, TruncParams::adjoint = 5) behind the long mode's levels
launch.  Every case is held to autograd of the torch restatement on CPU fp64 copies of the inputs, and the launch trace (sk_launch_trace)
proves which instance ran how often.

Bars: gradients fp64 <= 1e-10 of the gradient's max-norm (the project's bar for truncated gradients, test_gpu_truncated_adjoint.py; the
banded scheme itself sits <= 1e-12 from that reference, test_truncated_long_adjoint_host.py), forward values <= 1e-12 relative; fp32 I/O
rtol 1e-4 / atol 1e-5.

Measured maxima: MEASURED below.

Shapes are (M, N, D, L) in STEPS: the paths have M + 1 and N + 1 points; batches of A = 3 and B = 2."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_gpu_truncated import GENERAL, ORDER1, traced
from test_gpu_truncated_adjoint import assert_grad, paths

pytestmark = pytest.mark.gpu

# MEASURED on one MI355X (profiles/truncated_long_adjoint.txt, section 1): fp64 gradients <= 4.6e-15 of the gradient's max-norm over every case
# below (the largest: dY at 257 x 70 steps, 8 levels), forward values <= 1.5e-15 relative; fp32 paths 1.9e-7 of the max-norm.
A, B = 3, 2


def run_gpu(X, Y, L, sigma, c, grads, method="compute_Gram", workspace_bytes=None, long_adjoint=True, **kw):
    """loss = sum(c * method(X, Y)) and its gradients on the GPU, traced -> K, {name: grad}, launches"""
    import sigkernel_amd
    Xd, Yd = X.cuda().clone().requires_grad_("x" in grads), Y.cuda().clone().requires_grad_("y" in grads)
    sd = sigma.cuda().clone().requires_grad_("s" in grads) if isinstance(sigma, torch.Tensor) else sigma
    tk = sigkernel_amd.TruncatedSigKernel(L, sd, 1, workspace_bytes=workspace_bytes, long_adjoint=long_adjoint)

    def run():
        K = getattr(tk, method)(Xd, Xd if Y is X else Yd, **kw)
        (K * c.cuda().to(K.dtype)).sum().backward()
        return K
    K, hit = traced(run)
    return K.detach(), {"x": Xd.grad, "y": Yd.grad, "s": sd.grad if isinstance(sd, torch.Tensor) else None}, hit


def run_cpu(X, Y, L, sigma, c, grads, method="compute_Gram", **kw):
    """the same through the torch restatement on CPU fp64 copies"""
    import sigkernel_amd
    Xd, Yd = X.double().clone().requires_grad_("x" in grads), Y.double().clone().requires_grad_("y" in grads)
    sd = sigma.double().clone().requires_grad_("s" in grads) if isinstance(sigma, torch.Tensor) else sigma
    K = getattr(sigkernel_amd.TruncatedSigKernel(L, sd, 1), method)(Xd, Xd if Y is X else Yd, **kw)
    (K * c.double()).sum().backward()
    return K.detach(), {"x": Xd.grad, "y": Yd.grad, "s": sd.grad if isinstance(sd, torch.Tensor) else None}


def check_value(K, Kc, what):
    err = float((K.double().cpu() - Kc).abs().max() / Kc.abs().max())
    print("forward %s: %.3g relative" % (what, err))
    assert err <= 1e-12, (what, err)


# (M, N, D, L) and the launches (instance, count) with a gradient in x, in y, in both -- forward + one adjoint launch per batch:
#   (129, 40)   two bands, the second of one row; N < 64.  dY alone is inside the plain adjoint's scope (40 rows): the existing route, <1, 2>
#   (257, 70)   three bands: the middle one takes and leaves both carries; all levels, full fd
#   (40, 300)   one band, lane groups of 32 with a dead group (A = 3), two tiles
#   (130, 257)  two bands x two tiles, the second tile one column wide; one slab plane
#   (200, 300)  one level: no slab at all
GRAM = [((129, 40, 3, 4), {"x": (GENERAL, 2), "y": (ORDER1, 2), "xy": (GENERAL, 3)}),
        ((257, 70, 8, 8), {"x": (GENERAL, 2), "y": (GENERAL, 2), "xy": (GENERAL, 3)}),
        ((40, 300, 2, 3), {"x": (GENERAL, 2), "y": (GENERAL, 2), "xy": (GENERAL, 3)}),
        ((130, 257, 5, 2), {"x": (GENERAL, 2), "y": (GENERAL, 2), "xy": (GENERAL, 3)}),
        ((200, 300, 4, 1), {"x": (GENERAL, 2), "y": (GENERAL, 2), "xy": (GENERAL, 3)})]


@functools.lru_cache(maxsize=None)
def gram_case(shape):
    """inputs and the CPU reference of one shape, computed once for its three cases and left unchanged"""
    M, N, D, L = shape
    rng = np.random.default_rng(7000 + M + 7 * N + L)
    X, Y = paths(rng, A, M, D), paths(rng, B, N, D)
    sigma = torch.as_tensor(rng.uniform(0.5, 1.5, L + 1))
    c = torch.as_tensor(rng.standard_normal((A, B)))
    return X, Y, sigma, c, run_cpu(X, Y, L, sigma, c, "xy")


@pytest.mark.parametrize("grads", ["x", "y", "xy"])
@pytest.mark.parametrize("shape,launches", GRAM)
def test_gram_gradients_against_autograd_on_the_cpu(shape, launches, grads):
    X, Y, sigma, c, (Kc, gc) = gram_case(shape)
    K, g, hit = run_gpu(X, Y, shape[3], sigma, c, grads)
    assert hit == dict([launches[grads]]), hit
    assert K.is_cuda and K.dtype == torch.float64
    check_value(K, Kc, shape)
    for n in "xy":
        if n in grads:
            assert g[n].is_cuda and g[n].dtype == torch.float64
            assert_grad(g[n], gc[n], (shape, "d" + n))
        else:
            assert g[n] is None


def test_symmetric_gram_is_one_adjoint_launch():
    M, D, L = 150, 4, 5
    rng = np.random.default_rng(23)
    X = paths(rng, A, M, D)
    sigma = torch.as_tensor(rng.uniform(0.5, 1.5, L + 1))
    c = torch.as_tensor(rng.standard_normal((A, A)))          # not symmetric: the launch takes w + w^T
    K, g, hit = run_gpu(X, X, L, sigma, c, "x", sym=True)
    Kc, gc = run_cpu(X, X, L, sigma, c, "x", sym=True)
    assert hit == {GENERAL: 2}, hit
    check_value(K, Kc, "sym")
    assert_grad(g["x"], gc["x"], "sym dX")


def test_paired_gradients_of_both_sides():
    P, M, N, D, L = 5, 200, 270, 3, 4
    rng = np.random.default_rng(29)
    X, Y = paths(rng, P, M, D), paths(rng, P, N, D)
    sigma = torch.as_tensor(rng.uniform(0.5, 1.5, L + 1))
    c = torch.as_tensor(rng.standard_normal(P))
    K, g, hit = run_gpu(X, Y, L, sigma, c, "xy", method="compute_kernel")
    Kc, gc = run_cpu(X, Y, L, sigma, c, "xy", method="compute_kernel")
    assert hit == {GENERAL: 3}, hit
    assert K.shape == (P,)
    check_value(K, Kc, "paired")
    assert_grad(g["x"], gc["x"], "paired dX")
    assert_grad(g["y"], gc["y"], "paired dY")


def test_mmd_with_sigma_a_leaf():
    """compute_mmd: two long forward launches and two adjoint ones (K_XX once, as sym; K_XY); K_YY needs no path gradient and takes what
    it took without the keyword (the restatement, routes.truncated_long being off); dsigma from plain autograd on the level terms"""
    M, D, L = 140, 3, 4
    rng = np.random.default_rng(31)
    X, Y = paths(rng, A, M, D), paths(rng, B, M, D)
    sigma = torch.as_tensor(rng.uniform(0.5, 1.5, L + 1))
    v, g, hit = run_gpu(X, Y, L, sigma, torch.ones(()), "xs", method="compute_mmd")
    vc, gc = run_cpu(X, Y, L, sigma, torch.ones(()), "xs", method="compute_mmd")
    assert hit == {GENERAL: 4}, hit
    assert abs(float(v) - float(vc)) <= 1e-12 * max(1.0, abs(float(vc)))
    assert_grad(g["x"], gc["x"], "mmd dX")
    assert_grad(g["s"], gc["s"], "mmd dsigma")


def test_fp32_paths_return_fp32_gradients():
    M, N, D, L = 129, 40, 3, 4
    rng = np.random.default_rng(41)
    X, Y = paths(rng, A, M, D, np.float32), paths(rng, B, N, D, np.float32)
    c = torch.as_tensor(rng.standard_normal((A, B)))
    K, g, hit = run_gpu(X, Y, L, 0.9, c, "xy")
    Kc, gc = run_cpu(X, Y, L, 0.9, c, "xy")
    assert hit == {GENERAL: 3}, hit
    assert K.dtype == torch.float32 and g["x"].dtype == torch.float32 and g["y"].dtype == torch.float32
    assert_grad(g["x"], gc["x"], "fp32 dX", np.float32)
    assert_grad(g["y"], gc["y"], "fp32 dY", np.float32)


def long_adjoint_plan(a, b, M, N, D, L, paired, ws):
    from sigkernel_amd import _lib
    out = (ctypes.c_int64 * 4)()
    assert _lib.load().sk_truncated_long_adjoint_plan(a, b, M, N, D, L, paired, ws, ctypes.cast(out, ctypes.c_void_p)) == 0
    return tuple(out)


def test_small_workspaces():
    """exactly two block slabs: a plan of two blocks, every position but a block's first through used slabs, the same gradient to 1e-13;
    below one slab: nothing is launched and the gradient arrives through the restatement"""
    from sigkernel_amd import _lib
    a, b, M, N, D, L = 5, 4, 130, 70, 3, 4
    rng = np.random.default_rng(43)
    X, Y = paths(rng, a, M, D), paths(rng, b, N, D)
    sigma = torch.as_tensor(rng.uniform(0.5, 1.5, L + 1))
    c = torch.as_tensor(rng.standard_normal((a, b)))
    n_chunks, blocks, total, block = long_adjoint_plan(a, b, M, N, D, L, 0, 1 << 30)
    assert (n_chunks, blocks) == (4, 20) and block == (L - 1) * ((N + 63) * 1024 + 4 * 128 * 8) and total == 20 * block
    assert long_adjoint_plan(a, b, M, N, D, L, 0, 2 * block)[:3] == (4, 2, 2 * block)
    K, g, hit = run_gpu(X, Y, L, sigma, c, "x")
    K2, g2, hit2 = run_gpu(X, Y, L, sigma, c, "x", workspace_bytes=2 * block)
    assert hit == hit2 == {GENERAL: 2}, (hit, hit2)
    Kc, gc = run_cpu(X, Y, L, sigma, c, "x")
    assert_grad(g["x"], gc["x"], "default workspace dX")
    assert float((g2["x"] - g["x"]).abs().max()) <= 1e-13 * float(g["x"].abs().max())
    K3, g3, hit3 = run_gpu(X, Y, L, sigma, c, "x", workspace_bytes=block - 1)
    assert hit3 == {}, hit3
    assert_grad(g3["x"], gc["x"], "restatement dX")
    be = _lib.get_backend()
    dx = (X[:, 1:] - X[:, :-1]).cuda()
    dy = (Y[:, 1:] - Y[:, :-1]).cuda()
    w = torch.ones(L, a, b, dtype=torch.float64).cuda()
    out, hit = traced(lambda: be.truncated_long_adjoint(dx, dy, w, L, workspace_bytes=block - 1))
    assert out is None and hit == {}
    assert not be.truncated_long_adjoint_fits(a, b, M, N, D, L, False, block - 1) and be.truncated_long_adjoint_fits(a, b, M, N, D, L, False, block)


def test_two_backward_calls_give_equal_bits():
    import sigkernel_amd
    a, b, M, N, D, L = 9, 7, 257, 300, 8, 8
    rng = np.random.default_rng(2)
    X, Y = paths(rng, a, M, D).cuda(), paths(rng, b, N, D).cuda()
    c = torch.as_tensor(rng.standard_normal((a, b))).cuda()
    tk = sigkernel_amd.TruncatedSigKernel(L, long_adjoint=True)
    got = []
    for _ in range(3):
        x, y = X.clone().requires_grad_(), Y.clone().requires_grad_()
        (tk.compute_Gram(x, y) * c).sum().backward()
        got.append((x.grad, y.grad))
    for gx, gy in got[1:]:
        assert torch.equal(gx, got[0][0]) and torch.equal(gy, got[0][1])


def test_with_the_keyword_off_nothing_is_launched_with_a_gradient_pending(monkeypatch):
    import sigkernel_amd
    X, Y, sigma, c, (Kc, gc) = gram_case((129, 40, 3, 4))
    for switch in (False, True):
        monkeypatch.setattr(sigkernel_amd.routes, "truncated_long", switch)
        K, g, hit = run_gpu(X, Y, 4, sigma, c, "x", long_adjoint=False)
        assert hit == {}, hit
        assert_grad(g["x"], gc["x"], ("torch route dX", switch))


def test_backward_allocates_nothing_of_the_size_of_the_step_grids():
    """Peak memory over forward + backward, above what is held before: the two batches' staging, Tpart, the slabs of both launches (bounded
    by workspace_bytes), the summed gradient, and a few arrays of the size of the level terms -- far below ONE array of pairs x M x N
    doubles, of which the torch route keeps dozens."""
    import sigkernel_amd
    a, b, M, N, D, L = 48, 48, 160, 160, 4, 4
    ws = 64 << 20
    rng = np.random.default_rng(9)
    X, Y = paths(rng, a, M, D).cuda().requires_grad_(), paths(rng, b, N, D).cuda()
    tk = sigkernel_amd.TruncatedSigKernel(L, workspace_bytes=ws, long_adjoint=True)
    tk.compute_Gram(X, Y).sum().backward()          # (warm: library load, the allocator's pools)
    X.grad = None
    n_chunks, blocks, slab, block = long_adjoint_plan(a, b, M, N, D, L, 0, ws)
    assert slab <= ws and blocks >= 1
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    (_, hit) = traced(lambda: tk.compute_Gram(X, Y).sum().backward())
    peak = torch.cuda.max_memory_allocated() - base
    assert hit == {GENERAL: 2}, hit
    steps_bytes = 2 * 8 * (a * M * D + b * N * D)                           # the differenced paths and their contiguous copies
    staging = 8 * 8 * (a * M + b * (N + 15))
    tpart = 8 * 8 * n_chunks * a * M
    outputs = 8 * 8 * a * M + 2 * 8 * a * (M + 1) * D                       # the chunks' sum, dsteps, dX
    levels = 8 * (L + 1) * a * b
    allowed = steps_bytes + 2 * staging + tpart + slab + outputs + 8 * levels + (1 << 20)
    grid = 8 * a * b * M * N
    print("backward peak %.1f MB, allowed %.1f MB, one pairs x M x N array %.1f MB" % (peak / 2 ** 20, allowed / 2 ** 20, grid / 2 ** 20))
    assert peak <= allowed and allowed < grid / 4
