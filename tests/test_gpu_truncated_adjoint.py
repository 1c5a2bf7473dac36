"""TruncatedSigKernel on the GPU: gradients from the adjoint mode of k_trunc_sig<1, 2> (csrc/sk_truncated.hip: trunc_adjoint) against
autograd of the torch restatement run on the CPU in fp64 -- the same object on CPU tensors, where it takes that route as a whole.  The
launch trace (sk_launch_trace) proves which route ran.

Bars: fp64 <= 1e-10 of the gradient's max-norm (the project's bar for truncated gradients, test_gpu_truncated_paired.py; the reference
itself sits <= 2.1e-15 from the closed form the kernel evaluates, test_truncated_adjoint_host.py); fp32 I/O rtol 1e-4 / atol 1e-5.

Shapes are (A, B, M, N, D, L) in STEPS: the paths have M + 1 and N + 1 points."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_truncated import GENERAL, ORDER1, traced
from test_truncated_adjoint_host import closed_form
from test_truncated_host import steps

pytestmark = pytest.mark.gpu


def paths(rng, n, m, D, dtype=np.float64):
    """n paths of m steps that start at the origin"""
    return torch.as_tensor(np.concatenate([np.zeros((n, 1, D)), np.cumsum(steps(rng, n, m, D), axis=1)], axis=1).astype(dtype))


def assert_grad(got, want, what, dtype=np.float64):
    got, want = got.detach().double().cpu(), want.detach().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = float(want.abs().max())
    err = float((got - want).abs().max()) / scale if scale > 0 else float((got - want).abs().max())
    print("gradient %s: %.3g of its max-norm" % (what, err))
    if dtype == np.float64:
        assert err <= 1e-10, (what, err)
    else:
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-4, atol=1e-5, err_msg=str(what))


def both_routes(X, Y, L, sigma, c, grads, method="compute_Gram", order=1, workspace_bytes=None, **kw):
    """loss = sum(c * method(X, Y)) and its gradients on the GPU (traced) and on the CPU in fp64 -> (value, grads, launches), (value, grads)"""
    import sigkernel_amd
    out = []
    for dev in ("cuda", "cpu"):
        Xd = X.to(dev) if dev == "cuda" else X.double()
        Yd = Y.to(dev) if dev == "cuda" else Y.double()
        Xd = Xd.clone().requires_grad_("x" in grads)
        Yd = Yd.clone().requires_grad_("y" in grads)
        sd = sigma.to(dev).clone().requires_grad_("s" in grads) if isinstance(sigma, torch.Tensor) else sigma
        tk = sigkernel_amd.TruncatedSigKernel(L, sd, order, workspace_bytes=workspace_bytes if dev == "cuda" else None)
        cd = c.to(dev) if dev == "cuda" else c.double()

        def run():
            K = getattr(tk, method)(Xd, Xd if Y is X else Yd, **kw)
            (K * cd.to(K.dtype)).sum().backward()
            return K
        if dev == "cuda":
            K, hit = traced(run)
        else:
            K, hit = run(), None
        g = {"x": Xd.grad, "y": Yd.grad, "s": sd.grad if isinstance(sd, torch.Tensor) else None}
        out.append((K.detach(), g, hit))
    return out


# (A, B, M, N, D, L), which inputs require grad, the launches of k_trunc_sig<1, 2> in forward + backward
#   (3, 2, 9, 6)     eight-lane groups, dead groups, an odd row count
#   (2, 3, 128, 65)  a full wave, every level, N no multiple of 16
#   (2, 2, 2, 3) L 5 levels beyond min(M, N) are exactly zero and must add nothing
#   (5, 37, 20, 33)  several chunks per row tile, B not divisible
#   (2, 3, 100, 120) gradients in both batches: two adjoint launches
#   (2, 3, 70, 130)  dY out of scope (130 rows): the whole call launches nothing
GRAM = [((3, 2, 9, 6, 3, 4), "x", 2), ((2, 3, 128, 65, 8, 8), "xy", 3), ((1, 1, 1, 1, 1, 1), "xy", 3), ((2, 2, 2, 3, 2, 5), "xy", 3),
        ((5, 37, 20, 33, 3, 6), "x", 2), ((2, 3, 100, 120, 4, 3), "xy", 3), ((2, 3, 70, 130, 4, 3), "xy", 0), ((2, 3, 70, 130, 4, 3), "x", 2),
        ((3, 2, 9, 6, 3, 4), "y", 2)]


@pytest.mark.parametrize("shape,grads,launches", GRAM)
def test_gram_gradients_against_autograd_on_the_cpu(shape, grads, launches):
    A, B, M, N, D, L = shape
    rng = np.random.default_rng(5000 + M + 7 * N + L)
    X, Y = paths(rng, A, M, D), paths(rng, B, N, D)
    sigma = torch.as_tensor(rng.uniform(0.5, 1.5, L + 1))
    c = torch.as_tensor(rng.standard_normal((A, B)))
    (K, g, hit), (Kc, gc, _) = both_routes(X, Y, L, sigma, c, grads)
    assert hit == ({ORDER1: launches} if launches else {}), hit
    assert K.is_cuda and K.dtype == torch.float64 and float((K.cpu() - Kc).abs().max() / Kc.abs().max()) <= 1e-12
    for n in grads:
        assert g[n].is_cuda and g[n].dtype == torch.float64
        assert_grad(g[n], gc[n], (shape, "d" + n))
    for n in "xy":
        if n not in grads:
            assert g[n] is None


def adjoint_plan(A, B, M, N, D, L, paired, ws):
    from sigkernel_amd import _lib
    out = (ctypes.c_int64 * 3)()
    assert _lib.load().sk_truncated_adjoint_plan(A, B, M, N, D, L, paired, ws, ctypes.cast(out, ctypes.c_void_p)) == 0
    return tuple(out)


def test_backend_adjoint_with_arbitrary_level_weights_and_a_small_slab():
    """HipBackend.truncated_adjoint on weights of either sign per level and pair, against the closed form in torch on the CPU; then the
    same launch with a workspace of three blocks' slabs, so that every block walks 24 or 25 of the 74 positions through ONE slab: equal
    bits -- the chunking is the same, and a reused slab leaks nothing."""
    from sigkernel_amd import _lib
    be = _lib.get_backend()
    A, B, M, N, D, L = 5, 37, 20, 33, 3, 6
    rng = np.random.default_rng(77)
    X, Y = torch.as_tensor(steps(rng, A, M, D)), torch.as_tensor(steps(rng, B, N, D))
    w = torch.as_tensor(rng.standard_normal((L, A, B)))
    want, wantY = closed_form(X, Y, w)
    Xd, Yd, wd = X.cuda(), Y.cuda(), w.cuda()
    got, hit = traced(lambda: be.truncated_adjoint(Xd, Yd, wd, L))
    assert hit == {ORDER1: 1} and got.shape == (A, M, D) and got.dtype == torch.float64
    assert_grad(got, want, "backend dX")
    assert_grad(be.truncated_adjoint(Yd, Xd, wd.transpose(1, 2).contiguous(), L), wantY, "backend dY")
    block = (L - 1) * (N + 16 - 1) * 1024
    assert adjoint_plan(A, B, M, N, D, L, 0, 1 << 30) == (37, 74, 74 * block)
    assert adjoint_plan(A, B, M, N, D, L, 0, 3 * block + 100) == (37, 3, 3 * block)
    small = be.truncated_adjoint(Xd, Yd, wd, L, workspace_bytes=3 * block + 100)
    assert torch.equal(small, got)
    assert be.truncated_adjoint(Xd, Yd, wd, L, workspace_bytes=block - 1) is None          # not one block's slab
    # outside the scope: None, and nothing launched
    X9 = torch.as_tensor(steps(rng, 2, 8, 9)).cuda()
    out, hit = traced(lambda: be.truncated_adjoint(X9, X9, torch.ones(3, 2, 2, dtype=torch.float64).cuda(), 3))
    assert out is None and hit == {}
    # through the public object: the small workspace gives the same gradient bits as the default
    import sigkernel_amd
    Xp, Yp = paths(rng, A, M, D).cuda(), paths(rng, B, N, D).cuda()
    grads = []
    for ws in (None, 3 * block + 100):
        x = Xp.clone().requires_grad_()
        sigkernel_amd.TruncatedSigKernel(L, workspace_bytes=ws).compute_Gram(x, Yp).sum().backward()
        grads.append(x.grad)
    assert torch.equal(grads[0], grads[1])


def test_paired_gradients():
    """P = 13 pairs of nine steps: eight-lane groups, eight pairs a position -- the second position has five live groups"""
    P, M, N, D, L = 13, 9, 9, 2, 5
    rng = np.random.default_rng(13)
    X, Y = paths(rng, P, M, D), paths(rng, P, N, D)
    sigma = torch.as_tensor(rng.uniform(0.5, 1.5, L + 1))
    c = torch.as_tensor(rng.standard_normal(P))
    (K, g, hit), (Kc, gc, _) = both_routes(X, Y, L, sigma, c, "xy", method="compute_kernel")
    assert hit == {ORDER1: 3}, hit
    assert K.shape == (P,) and float((K.cpu() - Kc).abs().max() / Kc.abs().max()) <= 1e-12
    assert_grad(g["x"], gc["x"], "paired dX")
    assert_grad(g["y"], gc["y"], "paired dY")
    # unequal step counts, one side only, 100 pairs under a workspace of ONE block's slab (4 levels x 24 steps x 1 KB), which holds the
    # staging of 37 pairs: three forward and three adjoint launches, each of five positions through one block
    P2, block = 100, 4 * (17 + 8 - 1) * 1024
    X2, Y2 = paths(rng, P2, M, D), paths(rng, P2, 17, D)
    c2 = torch.as_tensor(rng.standard_normal(P2))
    (K, g, hit), (Kc, gc, _) = both_routes(X2, Y2, L, sigma, c2, "x", method="compute_kernel", workspace_bytes=block + 512)
    assert hit == {ORDER1: 6}, hit
    assert_grad(g["x"], gc["x"], "paired dX in three launches")


def test_symmetric_gram_is_one_adjoint_launch():
    A, M, D, L = 5, 20, 3, 6
    rng = np.random.default_rng(21)
    X = paths(rng, A, M, D)
    sigma = torch.as_tensor(rng.uniform(0.5, 1.5, L + 1))
    c = torch.as_tensor(rng.standard_normal((A, A)))          # not symmetric: the launch takes w + w^T
    (K, g, hit), (Kc, gc, _) = both_routes(X, X, L, sigma, c, "x", sym=True)
    assert hit == {ORDER1: 2}, hit
    assert_grad(g["x"], gc["x"], "sym dX")
    # the same matrix without sym: X feeds both arguments, forward + two adjoint launches, the same gradient
    (K2, g2, hit), _ = both_routes(X, X, L, sigma, c, "x")
    assert hit == {ORDER1: 3}, hit
    assert_grad(g2["x"], gc["x"], "X twice dX")


def test_sigma_leaf_and_mmd():
    """sigma as a leaf beside X: its gradient comes from plain autograd on the level terms of the same sweep; compute_mmd with a sample
    that needs no gradient: three forward launches, two adjoint ones (K_XX once, as sym; K_XY), none for K_YY"""
    A, B, M, N, D, L = 6, 5, 20, 33, 3, 4
    rng = np.random.default_rng(31)
    X, Y = paths(rng, A, M, D), paths(rng, B, N, D)
    sigma = torch.as_tensor(rng.uniform(0.5, 1.5, L + 1))
    c = torch.as_tensor(rng.standard_normal((A, B)))
    (K, g, hit), (Kc, gc, _) = both_routes(X, Y, L, sigma, c, "xs")
    assert hit == {ORDER1: 2}, hit
    assert_grad(g["x"], gc["x"], "dX beside sigma")
    assert_grad(g["s"], gc["s"], "dsigma")
    (v, g, hit), (vc, gc, _) = both_routes(X, Y, L, sigma, torch.ones(()), "xs", method="compute_mmd")
    assert hit == {ORDER1: 5}, hit
    assert abs(float(v) - float(vc)) <= 1e-12 * max(1.0, abs(float(vc)))
    assert_grad(g["x"], gc["x"], "mmd dX")
    assert_grad(g["s"], gc["s"], "mmd dsigma")


def test_fp32_paths_return_fp32_gradients():
    A, B, M, N, D, L = 3, 2, 9, 6, 3, 4
    rng = np.random.default_rng(41)
    X, Y = paths(rng, A, M, D, np.float32), paths(rng, B, N, D, np.float32)
    c = torch.as_tensor(rng.standard_normal((A, B)))
    (K, g, hit), (Kc, gc, _) = both_routes(X, Y, L, 0.9, c, "xy")
    assert hit == {ORDER1: 3}, hit
    assert K.dtype == torch.float32 and g["x"].dtype == torch.float32 and g["y"].dtype == torch.float32
    assert_grad(g["x"], gc["x"], "fp32 dX", np.float32)
    assert_grad(g["y"], gc["y"], "fp32 dY", np.float32)


@pytest.mark.parametrize("order,D", [(2, 3), (1, 9), (-1, 3)])
def test_outside_the_adjoint_scope_nothing_is_launched_with_a_gradient(order, D):
    A, B, M, N, L = 3, 2, 9, 6, 4
    rng = np.random.default_rng(51)
    X, Y = paths(rng, A, M, D), paths(rng, B, N, D)
    sigma = torch.as_tensor(rng.uniform(0.5, 1.5, L + 1))
    c = torch.as_tensor(rng.standard_normal((A, B)))
    (K, g, hit), (Kc, gc, _) = both_routes(X, Y, L, sigma, c, "xy", order=order)
    assert hit == {}, hit
    assert_grad(g["x"], gc["x"], ("torch route dX", order, D))
    assert_grad(g["y"], gc["y"], ("torch route dY", order, D))
    # without a gradient pending the forward is the kernel's, whichever instance serves the order
    import sigkernel_amd
    with torch.no_grad():
        Kn, hit = traced(lambda: sigkernel_amd.TruncatedSigKernel(L, sigma.cuda(), order).compute_Gram(X.cuda(), Y.cuda()))
    assert hit == {(ORDER1 if order == 1 else GENERAL): 1}, hit
    assert float((Kn.cpu() - Kc).abs().max() / Kc.abs().max()) <= 1e-12


def test_two_backward_calls_give_equal_bits():
    import sigkernel_amd
    A, B, M, N, D, L = 37, 29, 64, 65, 8, 8
    rng = np.random.default_rng(2)
    X, Y = paths(rng, A, M, D).cuda(), paths(rng, B, N, D).cuda()
    c = torch.as_tensor(rng.standard_normal((A, B))).cuda()
    tk = sigkernel_amd.TruncatedSigKernel(L)
    got = []
    for _ in range(3):
        x, y = X.clone().requires_grad_(), Y.clone().requires_grad_()
        (tk.compute_Gram(x, y) * c).sum().backward()
        got.append((x.grad, y.grad))
    for gx, gy in got[1:]:
        assert torch.equal(gx, got[0][0]) and torch.equal(gy, got[0][1])


def test_backward_allocates_nothing_of_the_size_of_the_step_grids():
    """Peak memory over forward + backward, above what is held before: the two batches' staging, Tpart, the slab (bounded by
    workspace_bytes), the summed gradient, and a few arrays of the size of the level terms (grad_levels, w, autograd's products in
    truncated_from_levels -- allowed: eight) -- far below ONE array of pairs x M x N doubles, of which the torch route keeps dozens."""
    import sigkernel_amd
    A, B, M, N, D, L = 96, 96, 64, 64, 4, 4
    ws = 32 << 20
    rng = np.random.default_rng(9)
    X, Y = paths(rng, A, M, D).cuda().requires_grad_(), paths(rng, B, N, D).cuda()
    tk = sigkernel_amd.TruncatedSigKernel(L, workspace_bytes=ws)
    tk.compute_Gram(X, Y).sum().backward()          # (warm: library load, the allocator's pools)
    X.grad = None
    n_chunks, blocks, slab = adjoint_plan(A, B, M, N, D, L, 0, ws)
    assert slab <= ws and blocks >= 1
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    (_, hit) = traced(lambda: tk.compute_Gram(X, Y).sum().backward())
    peak = torch.cuda.max_memory_allocated() - base
    assert hit == {ORDER1: 2}, hit
    steps_bytes = 2 * 8 * (A * M * D + B * N * D)                           # the differenced paths and their contiguous copies
    staging = 8 * 8 * (A * M + B * N)
    tpart = 8 * 8 * n_chunks * A * M
    outputs = 8 * 8 * A * M + 2 * 8 * A * (M + 1) * D                       # the chunks' sum, dsteps, dX
    levels = 8 * (L + 1) * A * B
    allowed = steps_bytes + 2 * staging + tpart + slab + outputs + 8 * levels + (1 << 20)
    grid = 8 * A * B * M * N
    print("backward peak %.1f MB, allowed %.1f MB, one pairs x M x N array %.1f MB" % (peak / 2 ** 20, allowed / 2 ** 20, grid / 2 ** 20))
    assert peak <= allowed and allowed < grid / 4
