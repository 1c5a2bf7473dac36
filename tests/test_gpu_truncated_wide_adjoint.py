"""TruncatedSigKernel(wide_adjoint=True) on the GPU: gradients at path dims 9 .. 16 from the wide-adjoint mode of k_trunc_sig<4, 1>
(csrc/sk_truncated.hip: trunc_wide_adjoint) against autograd of the torch restatement run on the CPU in fp64 -- the same object on CPU
tensors, where it takes that route as a whole.  The launch trace (sk_launch_trace) proves which route ran: the forward is the levels
launch of <1, 2>, every adjoint launch is one of <4, 1>.

Bars, the project's: values <= 1e-12 of their max, fp64 gradients <= 1e-10 of the gradient's max-norm (the reference itself sits
<= 2.1e-15 from the closed form the kernel evaluates, test_truncated_adjoint_host.py); fp32 I/O rtol 1e-4 / atol 1e-5.

MEASURED on one MI355X (profiles/truncated_wide_adjoint.txt, section 1): fp64 gradients <= 4.9e-15 of the gradient's max-norm over every
case of this file, values <= 3.9e-15 of their max, fp32 gradients <= 8.8e-8; the zero-padded batch gives the adjoint mode's bits.

Shapes are (A, B, M, N, D, L) in STEPS: the paths have M + 1 and N + 1 points."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_truncated import GENERAL, ORDER1, traced
from test_gpu_truncated_adjoint import assert_grad, paths
from test_truncated_adjoint_host import closed_form
from test_truncated_host import steps

pytestmark = pytest.mark.gpu


def both_routes(X, Y, L, sigma, c, grads, method="compute_Gram", order=1, workspace_bytes=None, wide_adjoint=True, **kw):
    """test_gpu_truncated_adjoint.both_routes with the keyword: loss = sum(c * method(X, Y)) and its gradients on the GPU (traced) and on
    the CPU in fp64 -> (value, grads, launches), (value, grads)"""
    import sigkernel_amd
    out = []
    for dev in ("cuda", "cpu"):
        Xd = X.to(dev) if dev == "cuda" else X.double()
        Yd = Y.to(dev) if dev == "cuda" else Y.double()
        Xd = Xd.clone().requires_grad_("x" in grads)
        Yd = Yd.clone().requires_grad_("y" in grads)
        sd = sigma.to(dev).clone().requires_grad_("s" in grads) if isinstance(sigma, torch.Tensor) else sigma
        tk = sigkernel_amd.TruncatedSigKernel(L, sd, order, workspace_bytes=workspace_bytes if dev == "cuda" else None,
                                              wide_adjoint=wide_adjoint)
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


# (A, B, M, N, D, L), which inputs require grad, the adjoint launches of k_trunc_sig<4, 1> (None: the whole call is out of scope)
#   (3, 2, 9, 6, 9)       eight-lane groups, dead groups, an odd row count, ONE coordinate in the second half of y, seven zero-padded dims
#   (2, 3, 128, 65, 16)   a full wave, every level, all 16 dims, N no multiple of 16
#   (2, 3, 128, 128, 16)  the scope's corner on both sides
#   (1, 1, 1, 1, 9) L 1   one level, no slab
#   (2, 2, 2, 3, 12) L 5  levels beyond min(M, N) are exactly zero and must add nothing
#   (5, 37, 20, 33, 13)   several chunks per row tile, B not divisible
#   (2, 3, 70, 129, 9)    129 columns at 16 staged coordinates: outside the scope, nothing is launched
GRAM = [((3, 2, 9, 6, 9, 4), "x", 1), ((3, 2, 9, 6, 9, 4), "y", 1), ((2, 3, 128, 65, 16, 8), "xy", 2), ((2, 3, 128, 128, 16, 8), "xy", 2),
        ((1, 1, 1, 1, 9, 1), "xy", 2), ((2, 2, 2, 3, 12, 5), "xy", 2), ((5, 37, 20, 33, 13, 6), "x", 1), ((2, 3, 70, 129, 9, 3), "xy", None)]


@pytest.mark.parametrize("shape,grads,launches", GRAM)
def test_gram_gradients_against_autograd_on_the_cpu(shape, grads, launches):
    A, B, M, N, D, L = shape
    rng = np.random.default_rng(6000 + M + 7 * N + L)
    X, Y = paths(rng, A, M, D), paths(rng, B, N, D)
    sigma = torch.as_tensor(rng.uniform(0.5, 1.5, L + 1))
    c = torch.as_tensor(rng.standard_normal((A, B)))
    (K, g, hit), (Kc, gc, _) = both_routes(X, Y, L, sigma, c, grads)
    assert hit == ({ORDER1: 1, GENERAL: launches} if launches else {}), hit
    err = float((K.cpu() - Kc).abs().max() / Kc.abs().max())
    print("values %s: %.3g of their max" % (shape, err))
    assert K.is_cuda and K.dtype == torch.float64 and err <= 1e-12
    for n in grads:
        assert g[n].is_cuda and g[n].dtype == torch.float64
        assert_grad(g[n], gc[n], (shape, "d" + n))
    for n in "xy":
        if n not in grads:
            assert g[n] is None


def wide_plan(A, B, M, N, D, L, paired, ws):
    from sigkernel_amd import _lib
    out = (ctypes.c_int64 * 3)()
    assert _lib.load().sk_truncated_wide_adjoint_plan(A, B, M, N, D, L, paired, ws, ctypes.cast(out, ctypes.c_void_p)) == 0
    return tuple(out)


def test_backend_with_arbitrary_level_weights_a_small_slab_and_equal_bits():
    """HipBackend.truncated_wide_adjoint on weights of either sign per level and pair, against the closed form in torch on the CPU; then the
    same launch with a workspace of three blocks' slabs, so that every block walks 24 or 25 of the 74 positions through ONE slab: equal
    bits -- the chunking is the same, and a reused slab leaks nothing; a repeated call: equal bits"""
    from sigkernel_amd import _lib
    be = _lib.get_backend()
    A, B, M, N, D, L = 5, 37, 20, 33, 13, 6
    rng = np.random.default_rng(78)
    X, Y = torch.as_tensor(steps(rng, A, M, D)), torch.as_tensor(steps(rng, B, N, D))
    w = torch.as_tensor(rng.standard_normal((L, A, B)))
    want, wantY = closed_form(X, Y, w)
    Xd, Yd, wd = X.cuda(), Y.cuda(), w.cuda()
    got, hit = traced(lambda: be.truncated_wide_adjoint(Xd, Yd, wd, L))
    assert hit == {GENERAL: 1} and got.shape == (A, M, D) and got.dtype == torch.float64
    assert_grad(got, want, "backend dX")
    assert_grad(be.truncated_wide_adjoint(Yd, Xd, wd.transpose(1, 2).contiguous(), L), wantY, "backend dY")
    assert torch.equal(be.truncated_wide_adjoint(Xd, Yd, wd, L), got)
    block = (L - 1) * (N + 16 - 1) * 1024
    assert wide_plan(A, B, M, N, D, L, 0, 1 << 30) == (37, 74, 74 * block)
    assert wide_plan(A, B, M, N, D, L, 0, 3 * block + 100) == (37, 3, 3 * block)
    small = be.truncated_wide_adjoint(Xd, Yd, wd, L, workspace_bytes=3 * block + 100)
    assert torch.equal(small, got)
    assert be.truncated_wide_adjoint(Xd, Yd, wd, L, workspace_bytes=block - 1) is None          # not one block's slab
    # dim 8 is the adjoint mode's: None, and nothing launched
    X8 = torch.as_tensor(steps(rng, 2, 8, 8)).cuda()
    out, hit = traced(lambda: be.truncated_wide_adjoint(X8, X8, torch.ones(3, 2, 2, dtype=torch.float64).cuda(), 3))
    assert out is None and hit == {}


@pytest.mark.parametrize("P,M,N,D,L", [(13, 9, 9, 10, 5), (5, 9, 33, 16, 3)])
def test_paired_gradients(P, M, N, D, L):
    """13 pairs of nine steps: eight-lane groups, eight pairs a position, the second position has five live groups.  5 pairs of 9 x 33 steps
    at dim 16: the y blocks of 16 x 48 doubles widen the groups to 32 lanes, two pairs a position, the last position half dead"""
    rng = np.random.default_rng(13 + P)
    X, Y = paths(rng, P, M, D), paths(rng, P, N, D)
    sigma = torch.as_tensor(rng.uniform(0.5, 1.5, L + 1))
    c = torch.as_tensor(rng.standard_normal(P))
    (K, g, hit), (Kc, gc, _) = both_routes(X, Y, L, sigma, c, "xy", method="compute_kernel")
    assert hit == {ORDER1: 1, GENERAL: 2}, hit
    assert K.shape == (P,) and float((K.cpu() - Kc).abs().max() / Kc.abs().max()) <= 1e-12
    assert_grad(g["x"], gc["x"], ("paired dX", P, M, N, D, L))
    assert_grad(g["y"], gc["y"], ("paired dY", P, M, N, D, L))


def test_symmetric_gram_sigma_leaf_and_mmd():
    """sym=True costs ONE adjoint launch (w + w^T); sigma as a leaf gets its gradient from plain autograd on the level terms of the same
    sweep; compute_mmd with a sample that needs no gradient: three forward launches, two adjoint ones (K_XX once, as sym; K_XY), none for K_YY"""
    A, B, M, N, D, L = 4, 3, 20, 20, 9, 4
    rng = np.random.default_rng(32)
    X, Y = paths(rng, A, M, D), paths(rng, B, N, D)
    sigma = torch.as_tensor(rng.uniform(0.5, 1.5, L + 1))
    c = torch.as_tensor(rng.standard_normal((A, A)))          # not symmetric: the launch takes w + w^T
    (K, g, hit), (Kc, gc, _) = both_routes(X, X, L, sigma, c, "xs", sym=True)
    assert hit == {ORDER1: 1, GENERAL: 1}, hit
    assert_grad(g["x"], gc["x"], "sym dX")
    assert_grad(g["s"], gc["s"], "sym dsigma")
    (v, g, hit), (vc, gc, _) = both_routes(X, Y, L, sigma, torch.ones(()), "xs", method="compute_mmd")
    assert hit == {ORDER1: 3, GENERAL: 2}, hit
    assert abs(float(v) - float(vc)) <= 1e-12 * max(1.0, abs(float(vc)))
    assert_grad(g["x"], gc["x"], "mmd dX")
    assert_grad(g["s"], gc["s"], "mmd dsigma")


def test_zero_padded_dims_give_the_plain_adjoints_gradient_and_exact_zeros():
    """a dim-5 batch padded with four zero coordinates to dim 9: the wide mode's dX[..., :5] within 1e-13 of the max-norm of the adjoint
    mode's dX on the unpadded batch (g adds zeros to the same FMA chain), and dX[..., 5:] is 0.0 exactly (dG times a zero coordinate)"""
    from sigkernel_amd import _lib
    be = _lib.get_backend()
    A, B, M, N, L = 3, 4, 21, 18, 5
    rng = np.random.default_rng(55)
    X, Y = torch.as_tensor(steps(rng, A, M, 5)).cuda(), torch.as_tensor(steps(rng, B, N, 5)).cuda()
    w = torch.as_tensor(rng.standard_normal((L, A, B))).cuda()
    pad = lambda t: torch.cat([t, torch.zeros(t.shape[0], t.shape[1], 4, dtype=t.dtype, device=t.device)], 2)
    plain, hit = traced(lambda: be.truncated_adjoint(X, Y, w, L))
    assert hit == {ORDER1: 1}
    wide, hit = traced(lambda: be.truncated_wide_adjoint(pad(X), pad(Y), w, L))
    assert hit == {GENERAL: 1} and wide.shape == (A, M, 9)
    err = float((wide[..., :5] - plain).abs().max() / plain.abs().max())
    print("wide on zero-padded dims vs the plain adjoint: %.3g of its max-norm" % err)
    assert err <= 1e-13
    assert torch.equal(wide[..., 5:], torch.zeros_like(wide[..., 5:]))


def test_fp32_paths_return_fp32_gradients():
    A, B, M, N, D, L = 3, 2, 9, 6, 11, 4
    rng = np.random.default_rng(42)
    X, Y = paths(rng, A, M, D, np.float32), paths(rng, B, N, D, np.float32)
    c = torch.as_tensor(rng.standard_normal((A, B)))
    (K, g, hit), (Kc, gc, _) = both_routes(X, Y, L, 0.9, c, "xy")
    assert hit == {ORDER1: 1, GENERAL: 2}, hit
    assert K.dtype == torch.float32 and g["x"].dtype == torch.float32 and g["y"].dtype == torch.float32
    assert_grad(g["x"], gc["x"], "fp32 dX", np.float32)
    assert_grad(g["y"], gc["y"], "fp32 dY", np.float32)


def test_without_the_keyword_nothing_is_launched_at_dim_nine_with_a_gradient():
    A, B, M, N, D, L = 3, 2, 9, 6, 9, 4
    rng = np.random.default_rng(52)
    X, Y = paths(rng, A, M, D), paths(rng, B, N, D)
    sigma = torch.as_tensor(rng.uniform(0.5, 1.5, L + 1))
    c = torch.as_tensor(rng.standard_normal((A, B)))
    (K, g, hit), (Kc, gc, _) = both_routes(X, Y, L, sigma, c, "xy", wide_adjoint=False)
    assert hit == {}, hit
    assert_grad(g["x"], gc["x"], "torch route dX")
    assert_grad(g["y"], gc["y"], "torch route dY")
