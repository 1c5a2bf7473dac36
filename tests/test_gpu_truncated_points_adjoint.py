"""TruncatedSigKernel(static_kernel=RBFKernel(s), points_adjoint=True) on the GPU: gradients from the points-adjoint mode of k_trunc_sig
(csrc/sk_truncated.hip: trunc_points_adjoint, hosted by the <4, 1> instance) against autograd of the same object on CPU tensors in fp64,
where it takes the torch restatement as a whole.  The launch trace (sk_launch_trace) proves which route ran: launches of k_trunc_sig<4, 1>
(the points mode's forward and its adjoint) and of <1, 2> (none, ever).

Bars: fp64 <= 1e-10 of the gradient's max-norm, the project's bar for truncated gradients (test_gpu_truncated_adjoint.py); fp32 in and out
rtol 1e-4 / atol 1e-5.  Every comparison prints the error it measured.

Shapes are (A, B, Mp, Np, D, L) with Mp, Np in POINTS; inputs are walks(...) of test_truncated_static_host.py, RBFKernel(1.0) unless stated."""
import numpy as np
import pytest
import torch

from test_gpu_truncated import GENERAL, ORDER1, traced
from test_gpu_truncated_adjoint import assert_grad
from test_truncated_points_adjoint_host import _plan, lifted_closed_form
from test_truncated_static_host import walks

pytestmark = pytest.mark.gpu


def lifted(L, sigma=1., s=1.0, order=1, **kw):
    import sigkernel_amd
    return sigkernel_amd.TruncatedSigKernel(L, sigma, order, static_kernel=sigkernel_amd.RBFKernel(s), **kw)


def both_routes(X, Y, L, sigma, c, grads, method="compute_Gram", s=1.0, workspace_bytes=None, points_adjoint=True, Xcpu=None, Ycpu=None, **kw):
    """loss = sum(c * method(X, Y)) and its gradients on the GPU (traced, points_adjoint as given) and on the CPU in fp64 (on Xcpu, Ycpu when
    given) -> (value, grads, launches), (value, grads, None)"""
    out = []
    for dev in ("cuda", "cpu"):
        if dev == "cuda":
            Xd, Yd = X.cuda(), Y.cuda()
        else:
            Xd, Yd = (X if Xcpu is None else Xcpu).double(), (Y if Ycpu is None else Ycpu).double()
        Xd = Xd.clone().requires_grad_("x" in grads)
        Yd = Yd.clone().requires_grad_("y" in grads)
        sd = sigma.to(dev).clone().requires_grad_("s" in grads) if isinstance(sigma, torch.Tensor) else sigma
        tk = lifted(L, sd, s, workspace_bytes=workspace_bytes if dev == "cuda" else None, points_adjoint=points_adjoint and dev == "cuda")
        cd = c.to(dev) if dev == "cuda" else c.double()

        def run():
            K = getattr(tk, method)(Xd, Xd if Y is X else Yd, **kw)
            (K * cd.to(K.dtype)).sum().backward()
            return K
        K, hit = traced(run) if dev == "cuda" else (run(), None)
        g = {"x": Xd.grad, "y": Yd.grad, "s": sd.grad if isinstance(sd, torch.Tensor) else None}
        out.append((K.detach(), g, hit))
    return out


def inputs(shape, seed, dtype=np.float64, paired=False):
    A, B, Mp, Np, D, L = shape
    rng = np.random.default_rng(seed)
    X, Y = torch.as_tensor(walks(rng, A, Mp, D, dtype)), torch.as_tensor(walks(rng, B, Np, D, dtype))
    sigma = torch.as_tensor(rng.uniform(0.5, 1.5, L + 1))
    c = torch.as_tensor(rng.standard_normal((A,) if paired else (A, B)))
    return X, Y, sigma, c


def check(shape, grads, launches, seed, value_tol=1e-12, **kw):
    X, Y, sigma, c = inputs(shape, seed)
    (K, g, hit), (Kc, gc, _) = both_routes(X, Y, shape[5], sigma, c, grads, **kw)
    assert hit == ({GENERAL: launches} if launches else {}), hit
    assert K.is_cuda and K.dtype == torch.float64 and float((K.cpu() - Kc).abs().max() / Kc.abs().max()) <= value_tol
    for n in grads:
        assert g[n].is_cuda and g[n].dtype == torch.float64
        assert_grad(g[n], gc[n], (shape, "d" + n))
    for n in "xy":
        if n not in grads:
            assert g[n] is None
    return g, gc


# (A, B, Mp, Np, D, L), which inputs require grad, the launches of k_trunc_sig<4, 1> in forward + backward
#   (3, 2, 10, 7)    eight-lane groups and dead groups
#   (3, 2, 9, 7)     an odd point count: the last lane's second row is padding
#   (2, 3, 128, 65)  a full wave, every level, N no multiple of 16
#   (5, 37, 20, 33)  several chunks per row tile, B not divisible
#   (2, 3, 70, 130)  dY out of scope (130 points): the whole call launches nothing; with dX alone it is served
GRAM = [((3, 2, 10, 7, 3, 4), "x", 2), ((3, 2, 10, 7, 3, 4), "y", 2), ((3, 2, 10, 7, 3, 4), "xy", 3), ((3, 2, 9, 7, 3, 4), "xy", 3),
        ((2, 3, 128, 65, 8, 8), "xy", 3), ((5, 37, 20, 33, 3, 6), "x", 2), ((2, 3, 70, 130, 4, 3), "xy", 0), ((2, 3, 70, 130, 4, 3), "x", 2),
        ((3, 2, 10, 7, 9, 4), "xy", 0)]


@pytest.mark.parametrize("shape,grads,launches", GRAM)
def test_gram_gradients_against_autograd_on_the_cpu(shape, grads, launches):
    g, gc = check(shape, grads, launches, 9000 + shape[2] + 7 * shape[3] + shape[5])
    if "x" in grads:        # the first point carries no node and does receive a gradient
        first, scale = g["x"][:, 0].cpu(), float(gc["x"].abs().max())
        assert bool((first.abs() > 0).all())
        assert float((first - gc["x"][:, 0]).abs().max()) <= 1e-10 * scale


@pytest.mark.parametrize("L", [1, 3])
def test_one_node_per_pair(L):
    """two points a path: one node, and all four points get a gradient; levels beyond min(Mp, Np) - 1 add exactly nothing"""
    shape = (2, 2, 2, 2, 1, L)
    g, gc = check(shape, "xy", 3, 9100)
    assert bool((g["x"].abs() > 0).all()) and bool((g["y"].abs() > 0).all())
    if L > 1:
        X, Y, sigma, c = inputs(shape, 9100)
        (_, g1, _), _ = both_routes(X, Y, 1, sigma[:2], c, "xy")
        assert torch.equal(g["x"], g1["x"]) and torch.equal(g["y"], g1["y"])


# P = 13 pairs of 10 points: eight-lane groups, eight pairs a position -- the second position has dead groups
# P = 7 pairs of 4 x 40 points: G fd Ncp > 2048 for dX, the groups are widened until their y blocks fit LDS
@pytest.mark.parametrize("P,Mp,Np,D,L", [(13, 10, 10, 2, 5), (7, 4, 40, 3, 4)])
def test_paired_gradients(P, Mp, Np, D, L):
    X, Y, sigma, c = inputs((P, P, Mp, Np, D, L), 9200 + P, paired=True)
    (K, g, hit), (Kc, gc, _) = both_routes(X, Y, L, sigma, c, "xy", method="compute_kernel")
    assert hit == {GENERAL: 3}, hit
    assert K.shape == (P,) and float((K.cpu() - Kc).abs().max() / Kc.abs().max()) <= 1e-12
    assert_grad(g["x"], gc["x"], ("paired dX", P))
    assert_grad(g["y"], gc["y"], ("paired dY", P))


def test_symmetric_gram_is_one_forward_and_one_adjoint_launch():
    shape = (5, 5, 20, 20, 3, 6)
    X, _, sigma, c = inputs(shape, 9300)          # c is not symmetric: the launch takes w + w^T
    (K, g, hit), (Kc, gc, _) = both_routes(X, X, 6, sigma, c, "x", sym=True)
    assert hit == {GENERAL: 2}, hit
    assert_grad(g["x"], gc["x"], "sym dX")


def test_mmd_with_one_sample_requiring_grad_and_a_learnable_sigma():
    """K_XX forward + one adjoint (sym), K_YY forward alone, K_XY forward + one adjoint: five launches of <4, 1>, none of <1, 2>; sigma as a
    leaf keeps its gradient through truncated_from_levels and the route stays the kernel's"""
    shape = (6, 5, 20, 33, 3, 4)
    X, Y, sigma, c = inputs(shape, 9400)
    (v, g, hit), (vc, gc, _) = both_routes(X, Y, 4, sigma, torch.ones(()), "x", method="compute_mmd")
    assert hit == {GENERAL: 5}, hit
    assert ORDER1 not in hit
    assert abs(float(v) - float(vc)) <= 1e-12 * max(1.0, abs(float(vc)))
    assert_grad(g["x"], gc["x"], "mmd dX")
    (K, g, hit), (Kc, gc, _) = both_routes(X, Y, 4, sigma, c, "xs")
    assert hit == {GENERAL: 2}, hit
    assert_grad(g["x"], gc["x"], "dX beside sigma")
    assert_grad(g["s"], gc["s"], "dsigma")


@pytest.mark.parametrize("s", [0.3, 30.0])
def test_bandwidths(s):
    check((3, 2, 10, 7, 3, 4), "xy", 3, 9500, s=s)


def test_a_common_offset_costs_no_digits():
    """100 added to every coordinate of both batches, against CPU autograd on the UNSHIFTED inputs at the same bar: the gradient is
    translation invariant, the kernel forms kap and the chain rule from differences of coordinates, and the restatement on shifted inputs
    loses digits through RBFKernel.Gram_matrix's expansion"""
    shape = (3, 2, 10, 7, 3, 4)
    X, Y, sigma, c = inputs(shape, 9600)
    (K, g, hit), (Kc, gc, _) = both_routes(X + 100.0, Y + 100.0, 4, sigma, c, "xy", Xcpu=X, Ycpu=Y)
    assert hit == {GENERAL: 3}, hit
    assert_grad(g["x"], gc["x"], "offset 100 dX")
    assert_grad(g["y"], gc["y"], "offset 100 dY")


def test_fp32_paths_return_fp32_gradients():
    shape = (3, 2, 10, 7, 3, 4)
    rng = np.random.default_rng(9700)
    X, Y = torch.as_tensor(walks(rng, 3, 10, 3, np.float32)), torch.as_tensor(walks(rng, 2, 7, 3, np.float32))
    c = torch.as_tensor(rng.standard_normal((3, 2)))
    (K, g, hit), (Kc, gc, _) = both_routes(X, Y, 4, 0.9, c, "xy")
    assert hit == {GENERAL: 3}, hit
    assert K.dtype == torch.float32 and g["x"].dtype == torch.float32 and g["y"].dtype == torch.float32
    assert_grad(g["x"], gc["x"], "fp32 dX", np.float32)
    assert_grad(g["y"], gc["y"], "fp32 dY", np.float32)


def test_backend_adjoint_with_arbitrary_level_weights_two_calls_and_a_small_slab():
    """HipBackend.truncated_points_adjoint on weights of either sign per level and pair, against the closed form in torch on the CPU; two
    calls give equal bits; a workspace of three blocks' slabs gives equal bits (every block walks its positions through ONE slab); one byte
    below one block's slab is None, and through the object the whole call then takes the restatement, nothing launched"""
    from sigkernel_amd import _lib
    be = _lib.get_backend()
    A, B, Mp, Np, D, L = 5, 37, 20, 33, 3, 6
    rng = np.random.default_rng(9800)
    X, Y = torch.as_tensor(walks(rng, A, Mp, D)), torch.as_tensor(walks(rng, B, Np, D))
    w = torch.as_tensor(rng.standard_normal((L, A, B)))
    want, wantY = lifted_closed_form(X, Y, w, 0.7)
    Xd, Yd, wd = X.cuda(), Y.cuda(), w.cuda()
    got, hit = traced(lambda: be.truncated_points_adjoint(Xd, Yd, wd, L, 0.7))
    assert hit == {GENERAL: 1} and got.shape == (A, Mp, D) and got.dtype == torch.float64
    assert_grad(got, want, "backend dX")
    assert_grad(be.truncated_points_adjoint(Yd, Xd, wd.transpose(1, 2).contiguous(), L, 0.7), wantY, "backend dY")
    assert torch.equal(be.truncated_points_adjoint(Xd, Yd, wd, L, 0.7), got)
    block = L * (Np + 16 - 1) * 1024
    assert _plan("sk_truncated_points_adjoint_plan", A, B, Mp, Np, D, L, 0, 1 << 30)[1][2] % block == 0
    assert _plan("sk_truncated_points_adjoint_plan", A, B, Mp, Np, D, L, 0, 3 * block + 100) == (0, (37, 3, 3 * block))
    assert torch.equal(be.truncated_points_adjoint(Xd, Yd, wd, L, 0.7, workspace_bytes=3 * block + 100), got)
    assert be.truncated_points_adjoint(Xd, Yd, wd, L, 0.7, workspace_bytes=block - 1) is None
    X9 = torch.as_tensor(walks(rng, 2, 8, 9)).cuda()
    out, hit = traced(lambda: be.truncated_points_adjoint(X9, X9, torch.ones(3, 2, 2, dtype=torch.float64).cuda(), 3, 0.7))
    assert out is None and hit == {}
    # through the public object
    grads = []
    for ws, launches in ((None, 2), (None, 2), (3 * block + 100, 2), (block - 1, 0)):
        x = Xd.clone().requires_grad_()
        _, hit = traced(lambda: lifted(L, workspace_bytes=ws, points_adjoint=True).compute_Gram(x, Yd).sum().backward())
        assert hit == ({GENERAL: launches} if launches else {}), (ws, hit)
        grads.append(x.grad)
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2])
    assert_grad(grads[3], grads[0].cpu(), "the restatement under a workspace below one block's slab")


def test_without_the_keyword_a_pending_gradient_launches_nothing():
    """the default object does what it did: a gradient pending means the restatement, on the GPU, and the same gradient"""
    shape = (3, 2, 10, 7, 3, 4)
    X, Y, sigma, c = inputs(shape, 9900)
    (K, g, hit), (Kc, gc, _) = both_routes(X, Y, 4, sigma, c, "xy", points_adjoint=False)
    assert hit == {}, hit
    assert_grad(g["x"], gc["x"], "default object dX")
    (K, g, hit), _ = both_routes(X, Y, 4, sigma, c, "xy")
    assert hit == {GENERAL: 3}, hit
    # ... and with the keyword but no gradient pending, the forward is the points mode's one launch
    with torch.no_grad():
        _, hit = traced(lambda: lifted(4, points_adjoint=True).compute_Gram(X.cuda(), Y.cuda()))
    assert hit == {GENERAL: 1}, hit
