"""truncated_sig_kernel_levels, truncated_from_levels and truncated_robust_scales without a GPU: the torch restatement that keeps each
level's sum (sigkernel_amd/truncated.py: _truncated_levels_torch) on CPU tensors against the reference's per-level outputs
(tests/golden/truncated_levels.npz, written by tests/golden/make_golden_truncated_levels.py: the reference called once per level with
the unit vectors as sigma), against _truncated_torch, and the public functions on stand-in back-ends (tests/fake_backend.py).

Bars: fp64 <= 1e-12 of EACH LEVEL's own max-norm against the reference; the restatement against itself on other axes or other weights
to a few ulp (stated at each check); fp32 I/O at the bar of tests/test_truncated_host.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from fake_backend import OracleBackend
from test_truncated_host import assert_close, steps

GOLDEN = os.path.join(ROOT, "tests", "golden", "truncated_levels.npz")


def level_fixtures():
    z = np.load(GOLDEN)
    for c in range(int(z["n_cases"])):
        k = "c%02d_" % c
        yield c, z[k + "X"], z[k + "Y"], int(z[k + "num_levels"]), int(z[k + "order"]), z[k + "levels"]


def assert_levels_close(got, want, dtype, what=""):
    """every level at the bar of assert_close, against ITS OWN max-norm"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for m in range(want.shape[0]):
        assert_close(got[m], want[m], dtype, (what, "level", m))


def level_err(got, want):
    """the worst level's max-norm error relative to that level's max-norm (a level that is exactly zero must come out exactly zero)"""
    worst = 0.0
    for g, w in zip(got, want):
        scale = float(w.abs().max())
        err = float((g - w).abs().max())
        worst = max(worst, err / scale if scale > 0 else (0.0 if err == 0 else float("inf")))
    return worst


def psi(s, C, a):
    return np.where(s <= C, s, C + C ** (1 + a) * (C ** -a - np.maximum(s, C) ** -a) / a)


class LevelsBackend(OracleBackend):
    """The level entry point of HipBackend on CPU tensors, with the kernel's swap rule in small: None when the first batch is longer than
    the second (the caller then asks for (Y, X)) and when neither has at most 6 steps (the caller takes the torch restatement)."""

    def __init__(self):
        self.calls = []

    def truncated_levels(self, X, Y, num_levels, order, paired=False):
        from sigkernel_amd.truncated import _truncated_levels_torch
        self.calls.append((tuple(X.shape), tuple(Y.shape), paired))
        if X.shape[1] > 6:
            return None
        return _truncated_levels_torch(X, Y, num_levels, order, paired)


@pytest.fixture
def torch_only(monkeypatch):
    """a back-end without truncated_levels / truncated_gram and no device check: the public functions take the torch restatement"""
    from sigkernel_amd import _lib
    monkeypatch.setattr(_lib, "_dev", lambda t, name: t)
    prev = _lib.set_backend(object())
    yield
    _lib.set_backend(prev)


@pytest.fixture
def levels_backend(monkeypatch):
    from sigkernel_amd import _lib
    monkeypatch.setattr(_lib, "_dev", lambda t, name: t)
    be = LevelsBackend()
    prev = _lib.set_backend(be)
    yield be
    _lib.set_backend(prev)


def test_fixture_file_covers_what_it_should():
    cases = list(level_fixtures())
    assert {c[1].dtype for c in cases} == {np.dtype(np.float64), np.dtype(np.float32)}
    assert {c[3] for c in cases} == {1, 2, 3, 4, 5, 6}
    assert {c[4] for c in cases} == {-1, 1, 2, 3}
    assert {c[1].shape[2] for c in cases} == {1, 3, 8}
    assert all(max(c[1].shape[1], c[2].shape[1]) <= 12 for c in cases)
    assert all(c[5].shape == (c[3] + 1, c[1].shape[0], c[2].shape[0]) and np.array_equal(c[5][0], np.ones_like(c[5][0])) for c in cases)
    assert any(c[1].shape[0] == c[2].shape[0] for c in cases) and any(c[1].shape[0] != c[2].shape[0] for c in cases)
    assert os.path.getsize(GOLDEN) < 100 << 10


@pytest.mark.parametrize("case", range(15))
def test_levels_reproduce_the_reference(case, torch_only):
    import sigkernel_amd
    from sigkernel_amd.truncated import _truncated_levels_torch
    c, X, Y, L, order, want = list(level_fixtures())[case]
    Xt, Yt = torch.as_tensor(X), torch.as_tensor(Y)
    got = _truncated_levels_torch(Xt, Yt, L, order)
    assert got.dtype == Xt.dtype and got.is_contiguous()
    assert_levels_close(got.numpy(), want, X.dtype.type, c)
    assert torch.equal(got[0], torch.ones_like(got[0]))
    # tiled one row at a time by the workspace budget; the public function (here: the torch route); the transforms alias
    assert_levels_close(_truncated_levels_torch(Xt, Yt, L, order, workspace_bytes=1).numpy(), want, X.dtype.type, (c, "tiled"))
    assert torch.equal(sigkernel_amd.truncated_sig_kernel_levels(Xt, Yt, L, order), got)
    assert torch.equal(sigkernel_amd.transforms.truncated_sig_kernel_levels(Xt, Yt, L, order=order), got)
    if X.shape[0] == Y.shape[0]:
        pd = sigkernel_amd.truncated_sig_kernel_levels(Xt, Yt, L, order, paired=True)
        assert_levels_close(pd.numpy(), np.stack([np.diagonal(v) for v in want]), X.dtype.type, (c, "paired"))


@pytest.mark.parametrize("L,order", [(1, 1), (3, -1), (4, 1), (4, 2), (6, 3), (8, 1), (8, 4), (8, 8)])
def test_levels_recombine_to_the_truncated_kernel(L, order):
    """truncated_from_levels(levels, sigma) against _truncated_torch: the same terms, summed over nodes before the weights instead of
    after -- a few ulp of the largest term, held to 1e-14 of the matrix's max-norm"""
    from sigkernel_amd.truncated import _truncated_levels_torch, _truncated_paired_torch, _truncated_torch, truncated_from_levels
    rng = np.random.default_rng(10 * L + order + 1)
    X, Y = torch.as_tensor(steps(rng, 3, 7, 3)), torch.as_tensor(steps(rng, 4, 5, 3))
    lv = _truncated_levels_torch(X, Y, L, order)
    assert lv.shape == (L + 1, 3, 4)
    for sigma in (1., 0.8, torch.as_tensor(rng.uniform(0.5, 1.5, L + 1)), torch.as_tensor(rng.standard_normal(L + 1))):
        want = _truncated_torch(X, Y, L, sigma, order)
        got = truncated_from_levels(lv, sigma)
        assert got.shape == want.shape and float((got - want).abs().max() / want.abs().max()) <= 1e-14
    # every truncation below L is in the same output: level m <= l has min(m, order) planes whatever l is
    for l in range(1, L + 1):
        want = _truncated_torch(X, Y, l, 1., min(order, l) if order > 0 else -1)
        got = truncated_from_levels(lv[:l + 1], 1.)
        assert float((got - want).abs().max() / want.abs().max()) <= 1e-14
    # paired: the per-level diagonal (the batched product may sum the path dimension in another order: 1e-13 of each level's max-norm;
    # at order 1 the levels beyond min(M, N) = 5 are exactly zero on both)
    Y3 = torch.as_tensor(steps(rng, 3, 5, 3))
    pd = _truncated_levels_torch(X, Y3, L, order, paired=True)
    full = _truncated_levels_torch(X, Y3, L, order)
    assert pd.shape == (L + 1, 3)
    assert level_err(pd, full.diagonal(dim1=1, dim2=2)) <= 1e-13
    assert level_err(_truncated_levels_torch(X, Y3, L, order, paired=True, workspace_bytes=1), pd) <= 1e-13
    sig = torch.as_tensor(rng.uniform(0.5, 1.5, L + 1))
    want = _truncated_paired_torch(X, Y3, L, sig, order)
    assert float(((truncated_from_levels(pd, sig) - want).abs() / want.abs()).max()) <= 1e-13


@pytest.mark.parametrize("order", [-1, 1, 2])
def test_scaling_a_path_by_two_scales_level_m_by_two_to_the_m_exactly(order):
    """multiplying by a power of two is exact in every product and sum of the recursion"""
    from sigkernel_amd.truncated import _truncated_levels_torch, truncated_from_levels
    rng = np.random.default_rng(3)
    L = 5
    X, Y = torch.as_tensor(steps(rng, 3, 6, 2)), torch.as_tensor(steps(rng, 2, 7, 2))
    base = _truncated_levels_torch(X, Y, L, order)
    pw = torch.as_tensor([2.0 ** m for m in range(L + 1)]).reshape(-1, 1, 1)
    assert torch.equal(_truncated_levels_torch(2 * X, Y, L, order), pw * base)
    assert torch.equal(_truncated_levels_torch(X, 2 * Y, L, order), pw * base)
    assert torch.equal(_truncated_levels_torch(2 * X, 0.5 * Y, L, order), base)
    # ... which is what the scales of truncated_from_levels rest on: the kernel of (lx X, ly Y) without another sweep
    lx, ly = torch.as_tensor([2.0, 0.5, 4.0]), torch.as_tensor([0.25, 2.0])
    sig = torch.as_tensor(rng.uniform(0.5, 1.5, L + 1))
    want = truncated_from_levels(_truncated_levels_torch(lx[:, None, None] * X, ly[:, None, None] * Y, L, order), sig)
    got = truncated_from_levels(base, sig, lx, ly)
    assert float((got - want).abs().max() / want.abs().max()) <= 1e-15
    got1 = truncated_from_levels(base, sig, scale_x=lx)
    want1 = truncated_from_levels(_truncated_levels_torch(lx[:, None, None] * X, Y, L, order), sig)
    assert float((got1 - want1).abs().max() / want1.abs().max()) <= 1e-15
    # paired, with a scalar scale
    Y3 = torch.as_tensor(steps(rng, 3, 7, 2))
    pd = _truncated_levels_torch(X, Y3, L, order, paired=True)
    want = truncated_from_levels(_truncated_levels_torch(lx[:, None, None] * X, 2 * Y3, L, order, paired=True), sig)
    got = truncated_from_levels(pd, sig, lx, 2.0)
    assert got.shape == (3,) and float(((got - want) / want).abs().max()) <= 1e-15


def test_the_swap_route_transposes_every_level(levels_backend):
    import sigkernel_amd
    from sigkernel_amd.truncated import _truncated_levels_torch
    rng = np.random.default_rng(4)
    X, Y = torch.as_tensor(steps(rng, 3, 9, 2)), torch.as_tensor(steps(rng, 2, 5, 2))
    want = _truncated_levels_torch(X, Y, 4, 2)
    got = sigkernel_amd.truncated_sig_kernel_levels(X, Y, 4, 2)
    assert levels_backend.calls == [((3, 9, 2), (2, 5, 2), False), ((2, 5, 2), (3, 9, 2), False)]
    assert got.shape == (5, 3, 2) and got.is_contiguous()
    assert float((got - want).abs().max()) <= 1e-15
    # the direct route, and neither: the torch restatement after both were asked
    del levels_backend.calls[:]
    assert torch.equal(sigkernel_amd.truncated_sig_kernel_levels(Y, X, 4, 2), _truncated_levels_torch(Y, X, 4, 2))
    assert levels_backend.calls == [((2, 5, 2), (3, 9, 2), False)]
    del levels_backend.calls[:]
    Y9 = torch.as_tensor(steps(rng, 2, 8, 2))
    assert torch.equal(sigkernel_amd.truncated_sig_kernel_levels(X, Y9, 4, 2), _truncated_levels_torch(X, Y9, 4, 2))
    assert len(levels_backend.calls) == 2
    # paired: the swapped call needs no transposing; the staging budget splits the batch (8 * 8 * (5 + 16) bytes per pair)
    del levels_backend.calls[:]
    X3, Y3 = torch.as_tensor(steps(rng, 3, 9, 2)), torch.as_tensor(steps(rng, 3, 5, 2))
    wantp = _truncated_levels_torch(X3, Y3, 4, 2, paired=True)
    gotp = sigkernel_amd.truncated_sig_kernel_levels(X3, Y3, 4, 2, paired=True)
    assert gotp.shape == (5, 3) and float(((gotp - wantp) / wantp).abs().max()) <= 1e-13
    assert levels_backend.calls == [((3, 9, 2), (3, 5, 2), True), ((3, 5, 2), (3, 9, 2), True)]
    del levels_backend.calls[:]
    gotp = sigkernel_amd.truncated_sig_kernel_levels(Y3, X3, 4, 2, paired=True, workspace_bytes=2 * 8 * 8 * (5 + 16))
    assert [c[0][0] for c in levels_backend.calls] == [2, 1]
    assert gotp.shape == (5, 3) and float(((gotp - wantp) / wantp).abs().max()) <= 1e-13


def test_inputs_that_require_grad_skip_the_backend(levels_backend):
    import sigkernel_amd
    rng = np.random.default_rng(6)
    X, Y = torch.as_tensor(steps(rng, 2, 4, 2)).requires_grad_(), torch.as_tensor(steps(rng, 2, 3, 2))
    lv = sigkernel_amd.truncated_sig_kernel_levels(X, Y, 3)
    assert lv.requires_grad and levels_backend.calls == []
    with torch.no_grad():
        sigkernel_amd.truncated_sig_kernel_levels(X, Y, 3)
    assert len(levels_backend.calls) == 1


@pytest.mark.parametrize("order", [-1, 1, 2])
def test_gradients_match_autograd_through_the_truncated_kernel(order, torch_only):
    """d/dX, d/dY of sum_m w_m sum_ab c_ab k_m through the levels against the same through _truncated_torch with sigma = w; d/dsigma
    through truncated_from_levels against _truncated_torch's.  The same graph up to the order of two sums: 1e-12 of each gradient's max."""
    import sigkernel_amd
    from sigkernel_amd.truncated import _truncated_torch
    rng = np.random.default_rng(11 + order)
    L = 4
    Xc, Yc = torch.as_tensor(steps(rng, 3, 5, 2)), torch.as_tensor(steps(rng, 2, 4, 2))
    w = torch.as_tensor(rng.uniform(0.5, 1.5, L + 1))
    c = torch.as_tensor(rng.standard_normal((3, 2)))
    X, Y, sig = Xc.clone().requires_grad_(), Yc.clone().requires_grad_(), w.clone().requires_grad_()
    lv = sigkernel_amd.truncated_sig_kernel_levels(X, Y, L, order)
    assert lv.requires_grad
    (sigkernel_amd.truncated_from_levels(lv, sig) * c).sum().backward()
    Xr, Yr, sr = Xc.clone().requires_grad_(), Yc.clone().requires_grad_(), w.clone().requires_grad_()
    (_truncated_torch(Xr, Yr, L, sr, order) * c).sum().backward()
    for got, want, name in ((X.grad, Xr.grad, "dX"), (Y.grad, Yr.grad, "dY"), (sig.grad, sr.grad, "dsigma")):
        err = float((got - want).abs().max() / want.abs().max())
        assert err <= 1e-12, (name, err)
    # sigma alone: the levels need no graph (this is the route a learnable weight vector takes on the GPU)
    s2 = w.clone().requires_grad_()
    (sigkernel_amd.truncated_from_levels(lv.detach(), s2) * c).sum().backward()
    assert float((s2.grad - sr.grad).abs().max() / sr.grad.abs().max()) <= 1e-12
    # ... and the scales are differentiable too
    lx = torch.ones(3, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda a, b: sigkernel_amd.truncated_from_levels(lv.detach(), w, a, b),
                                    (lx, torch.full((2,), 0.7, dtype=torch.float64, requires_grad=True)), eps=1e-6, atol=1e-8, rtol=1e-6)


def test_levels_gradcheck():
    from sigkernel_amd.truncated import _truncated_levels_torch
    rng = np.random.default_rng(12)
    X = torch.as_tensor(steps(rng, 2, 4, 2)).requires_grad_()
    Y = torch.as_tensor(steps(rng, 2, 3, 2)).requires_grad_()
    for paired in (False, True):
        assert torch.autograd.gradcheck(lambda x, y: _truncated_levels_torch(x, y, 3, 2, paired), (X, Y), eps=1e-6, atol=1e-7, rtol=1e-6)


@pytest.mark.parametrize("C,a", [(4.0, 1.0), (2.0, 0.5), (1.5, 2.0)])
def test_robust_scales(C, a, torch_only):
    import sigkernel_amd
    from sigkernel_amd.truncated import _truncated_levels_torch
    rng = np.random.default_rng(13)
    L = 5
    # steps scaled so that the self-kernels s = sum_m n_m straddle C
    X = torch.as_tensor(steps(rng, 12, 6, 3)) * torch.as_tensor(np.linspace(0.3, 4.0, 12))[:, None, None]
    n = sigkernel_amd.truncated_sig_kernel_levels(X, X, L, paired=True)
    assert n.shape == (L + 1, 12) and bool((n >= 0).all())
    s = n.sum(0)
    assert bool((s <= C).any()) and bool((s > C).any())
    lam = sigkernel_amd.truncated_robust_scales(n, C, a)
    assert lam.shape == (12,) and lam.dtype == torch.float64 and not lam.requires_grad
    assert bool(((lam >= 0) & (lam <= 1)).all())
    assert torch.equal(lam[s <= C], torch.ones_like(lam[s <= C])) and bool((lam[s > C] < 1).all())
    # the defining equation, to 1e-12 of its right side
    lhs = sum(lam ** (2 * m) * n[m] for m in range(L + 1))
    want = torch.as_tensor(psi(s.numpy(), C, a))
    assert float(((lhs - want).abs() / want).max()) <= 1e-12
    assert float(want.max()) <= C * (1 + 1 / a)
    # the rescaled self-kernel is psi(s): through truncated_from_levels, and by actually rescaling the paths
    assert float(((sigkernel_amd.truncated_from_levels(n, 1., lam, lam) - want).abs() / want).max()) <= 1e-12
    again = _truncated_levels_torch(lam[:, None, None] * X, lam[:, None, None] * X, L, paired=True).sum(0)
    assert float(((again - want).abs() / want).max()) <= 1e-12
    # numpy in, numpy out; the transforms alias; fp32 levels give fp32 scales
    ln = sigkernel_amd.transforms.truncated_robust_scales(n.numpy(), C, a)
    assert isinstance(ln, np.ndarray) and np.array_equal(ln, lam.numpy())
    assert sigkernel_amd.truncated_robust_scales(n.float(), C, a).dtype == torch.float32


def test_robust_scales_reject_negative_levels_and_bad_arguments():
    import sigkernel_amd
    n = torch.as_tensor([[1.0, 1.0], [3.0, 2.0], [-0.5, 4.0]])
    with pytest.raises(ValueError, match="negative"):
        sigkernel_amd.truncated_robust_scales(n)
    with pytest.raises(ValueError, match="shape"):
        sigkernel_amd.truncated_robust_scales(torch.ones(3, 2, 2))
    with pytest.raises(ValueError, match="positive"):
        sigkernel_amd.truncated_robust_scales(n.abs(), C=0.0)
    with pytest.raises(ValueError, match="positive"):
        sigkernel_amd.truncated_robust_scales(n.abs(), a=-1.0)


def test_argument_errors(torch_only):
    import sigkernel_amd
    from sigkernel_amd.truncated import _truncated_levels_torch
    X, Y = torch.rand(3, 4, 3, dtype=torch.float64), torch.rand(3, 5, 3, dtype=torch.float64)
    for fn in (_truncated_levels_torch, sigkernel_amd.truncated_sig_kernel_levels):
        with pytest.raises(ValueError, match="shape"):
            fn(X[0], Y, 3)
        with pytest.raises(ValueError, match="same path dimension"):
            fn(X, Y[..., :2], 3)
        with pytest.raises(ValueError, match="dtype and device"):
            fn(X, Y.float(), 3)
        with pytest.raises(TypeError, match="float64 and float32"):
            fn(X.half(), Y.half(), 3)
        with pytest.raises(ValueError, match="num_levels"):
            fn(X, Y, 0)
        with pytest.raises(ValueError, match="order"):
            fn(X, Y, 3, 4)
        with pytest.raises(ValueError, match="same number of paths"):
            fn(X, Y[:2], 3, paired=True)
        assert fn(X, Y[:2], 3).shape == (4, 3, 2)
        assert fn(X.float(), Y.float(), 3).dtype == torch.float32
        assert fn(X[:0], Y, 3).shape == (4, 0, 3) and fn(X[:0], Y[:0], 3, paired=True).shape == (4, 0)
    lv = _truncated_levels_torch(X, Y, 3)
    with pytest.raises(ValueError, match="sigma"):
        sigkernel_amd.truncated_from_levels(lv, [1., 2., 3.])
    with pytest.raises(ValueError, match="scale_x"):
        sigkernel_amd.truncated_from_levels(lv, 1., torch.ones(2))
    with pytest.raises(ValueError, match="scale_y"):
        sigkernel_amd.truncated_from_levels(lv, 1., None, torch.ones(2))
    with pytest.raises(ValueError, match="levels must have shape"):
        sigkernel_amd.truncated_from_levels(lv[0, 0], 1.)
    out = sigkernel_amd.truncated_from_levels(lv.numpy(), 0.5)
    assert isinstance(out, np.ndarray) and out.shape == (3, 3)


def test_levels_function_is_a_product_path():
    """no stand-in: HIP devices only, like the rest of the library"""
    import sigkernel_amd
    X = torch.rand(2, 4, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sigkernel_amd.truncated_sig_kernel_levels(X, X, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sigkernel_amd.truncated_sig_kernel_levels(X, X, 3, paired=True)


def test_the_level_entry_points_of_the_c_abi():
    from sigkernel_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sigkernel_amd.h")).read(), flags=re.S)
    lib = ctypes.CDLL(build.build())
    for name in ("sk_truncated_levels_f64", "sk_truncated_levels_f32", "sk_truncated_levels_paired_f64", "sk_truncated_levels_paired_f32"):
        assert re.search(r"\bint %s\s*\(" % name, text), name
        # the plain entry point's arguments without the weights
        plain = name.replace("levels_paired", "paired") if "paired" in name else name.replace("levels", "gram")
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[plain][1]) - 1
        assert hasattr(lib, name), name
    assert hasattr(_lib.HipBackend, "truncated_levels")
    # argument errors before any HIP call, and the Gram entry points' scope
    p = ctypes.c_void_p(16)
    f = _lib.load().sk_truncated_levels_f64
    assert f(None, p, 4, 3, 8, 8, 8, 16, 3, 8, 2, 2, p, None) == 1
    assert f(p, p, 4, -1, 8, 8, 8, 16, 3, 8, 2, 2, p, None) == 1
    assert f(p, p, 4, 3, 7, 8, 8, 16, 3, 8, 2, 2, p, None) == 1            # Mrows < M
    assert f(p, p, 4, 3, 8, 8, 8, 16, 3, 8, 2, 2, None, None) == 1         # no output
    assert f(p, p, 4, 0, 8, 8, 8, 16, 3, 8, 2, 2, p, None) == 0            # no pairs: nothing to do
    assert f(p, p, 4, 3, 65, 65, 8, 16, 3, 8, 2, 2, p, None) == 2          # 65 rows at order 2: outside the route's scope
    assert _lib.load().sk_truncated_levels_f32(p, p, 4, 3, 8, 8, 8, 16, 3, 8, 9, 1, p, None) == 2      # nine levels
    g = _lib.load().sk_truncated_levels_paired_f64
    assert g(p, None, 4, 8, 8, 8, 16, 3, 8, 2, 2, p, None) == 1
    assert g(p, p, 0, 8, 8, 8, 16, 3, 8, 2, 2, p, None) == 0
    assert g(p, p, 4, 8, 8, 8, 16, 17, 32, 2, 2, p, None) == 2             # dim 17
    assert _lib.load().sk_truncated_levels_paired_f32(p, p, 4, 8, 8, 8, 4, 3, 8, 2, 2, p, None) == 1     # Ncp < N
