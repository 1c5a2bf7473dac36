"""truncated_sig_kernel_paired and truncated_sig_kernel(..., normalize=True) without a GPU: the paired torch restatement
(sigkernel_amd/truncated.py: _truncated_paired_torch) on CPU tensors against the diagonal of the Gram restatement and of the reference's
recorded matrices (tests/golden/truncated.npz), its gradient, the normalised matrix through the public function on a stand-in back-end
that has no kernel (so both parts take the torch route), argument errors, and the two new entry points of the C ABI.

Bars: the paired restatement is the Gram restatement's arithmetic on other axes, so fp64 values agree to 1e-13 of each value (a batched
matrix product may sum the path dimension in another order: a few ulp of G, carried through at most eight levels); the fixtures at the
bar of tests/test_truncated_host.py."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_truncated_host import assert_close, fixtures, sigma_arg, steps

PAIRED_TOL = 1e-13


def rel(got, want):
    return float(((got - want).abs() / want.abs()).max())


@pytest.fixture
def torch_only(monkeypatch):
    """The public functions on CPU tensors: a back-end without truncated_gram / truncated_paired (every call takes the torch restatement)
    and no device check -- the stand-in these tests need, nothing more."""
    from sigkernel_amd import _lib
    monkeypatch.setattr(_lib, "_dev", lambda t, name: t)
    prev = _lib.set_backend(object())
    yield
    _lib.set_backend(prev)


@pytest.mark.parametrize("L,order", [(1, 1), (4, 1), (4, 2), (4, 4), (8, 1), (8, 2), (8, 8)])
def test_paired_restatement_is_the_diagonal_of_the_gram_restatement(L, order):
    from sigkernel_amd.truncated import _truncated_paired_torch, _truncated_torch
    rng = np.random.default_rng(100 * L + order)
    worst = 0.0
    for P, M, N, D in itertools.product((1, 3), (1, 2, 5, 7), (1, 2, 5, 7), (1, 3)):
        X, Y = torch.as_tensor(steps(rng, P, M, D)), torch.as_tensor(steps(rng, P, N, D))
        for sigma in (0.8, torch.as_tensor(rng.uniform(0.5, 1.5, L + 1))):
            want = _truncated_torch(X, Y, L, sigma, order).diagonal()
            got = _truncated_paired_torch(X, Y, L, sigma, order)
            assert got.shape == (P,) and got.dtype == torch.float64
            worst = max(worst, rel(got, want))
            # tiled one pair at a time by the workspace budget: the same values
            assert rel(_truncated_paired_torch(X, Y, L, sigma, order, workspace_bytes=1), want) <= PAIRED_TOL
    print("paired restatement L %d order %d: worst relative difference %.3g" % (L, order, worst))
    assert worst <= PAIRED_TOL


def test_paired_restatement_reproduces_the_reference_diagonal():
    from sigkernel_amd.truncated import _truncated_paired_torch
    seen = 0
    for c, X, Y, L, sigma, order, K in fixtures():
        if X.shape[0] != Y.shape[0]:
            continue
        seen += 1
        got = _truncated_paired_torch(torch.as_tensor(X), torch.as_tensor(Y), L, sigma_arg(sigma), order)
        assert got.shape == (X.shape[0],) and got.dtype == torch.as_tensor(X).dtype
        assert_close(got.numpy(), np.diagonal(K), X.dtype.type, c)
    assert seen > 0


def test_paired_restatement_gradcheck():
    from sigkernel_amd.truncated import _truncated_paired_torch
    rng = np.random.default_rng(21)
    X = torch.as_tensor(steps(rng, 2, 4, 2)).requires_grad_()
    Y = torch.as_tensor(steps(rng, 2, 3, 2)).requires_grad_()
    sig = torch.as_tensor(rng.uniform(0.5, 1.5, 4))
    assert torch.autograd.gradcheck(lambda x, y: _truncated_paired_torch(x, y, 3, sig, 2), (X, Y), eps=1e-6, atol=1e-7, rtol=1e-6)


def test_public_paired_function_and_its_gradient(torch_only):
    import sigkernel_amd
    from sigkernel_amd.truncated import _truncated_torch
    rng = np.random.default_rng(5)
    Xc, Yc = torch.as_tensor(steps(rng, 3, 5, 2)), torch.as_tensor(steps(rng, 3, 4, 2))
    sig = torch.as_tensor(rng.uniform(0.5, 1.5, 4))
    w = torch.as_tensor(rng.standard_normal(3))
    X, Y = Xc.clone().requires_grad_(), Yc.clone().requires_grad_()
    k = sigkernel_amd.truncated_sig_kernel_paired(X, Y, 3, sigma=sig, order=2)
    assert k.shape == (3,) and k.requires_grad
    (k * w).sum().backward()
    Xr, Yr = Xc.clone().requires_grad_(), Yc.clone().requires_grad_()
    (_truncated_torch(Xr, Yr, 3, sig, 2).diagonal() * w).sum().backward()
    assert rel(k.detach(), _truncated_torch(Xc, Yc, 3, sig, 2).diagonal()) <= PAIRED_TOL
    assert torch.allclose(X.grad, Xr.grad, rtol=1e-12, atol=1e-14) and torch.allclose(Y.grad, Yr.grad, rtol=1e-12, atol=1e-14)
    assert torch.equal(sigkernel_amd.transforms.truncated_sig_kernel_paired(Xc, Yc, 3, sigma=sig, order=2), k.detach())
    # empty batches: (0,)
    assert sigkernel_amd.truncated_sig_kernel_paired(Xc[:0], Yc[:0], 3).shape == (0,)


def test_normalised_matrix(torch_only):
    import sigkernel_amd
    from sigkernel_amd.truncated import _truncated_paired_torch, _truncated_torch
    rng = np.random.default_rng(8)
    X, Y = torch.as_tensor(steps(rng, 4, 6, 3)), torch.as_tensor(steps(rng, 3, 5, 3))
    sig = torch.as_tensor(rng.uniform(0.5, 1.5, 5))
    for order in (1, 2, 4):
        K = sigkernel_amd.truncated_sig_kernel(X, Y, 4, sigma=sig, order=order, normalize=True)
        kx, ky = _truncated_paired_torch(X, X, 4, sig, order), _truncated_paired_torch(Y, Y, 4, sig, order)
        want = _truncated_torch(X, Y, 4, sig, order) / torch.sqrt(kx[:, None] * ky[None, :])
        assert K.shape == (4, 3) and rel(K, want) <= 1e-14
        # unit diagonal and symmetry on (X, X), passed as the same object and as an equal one
        for X2 in (X, X.clone()):
            S = sigkernel_amd.truncated_sig_kernel(X, X2, 4, sigma=sig, order=order, normalize=True)
            assert (S.diagonal() - 1).abs().max() <= 1e-14
            assert (S - S.t()).abs().max() <= 1e-14
            assert S.abs().max() <= 1 + 1e-14 or order < 4      # Cauchy-Schwarz holds for the full order's inner product
    # the default changes nothing
    for a in ((X, Y), (X, X)):
        assert torch.equal(sigkernel_amd.truncated_sig_kernel(*a, 4, sigma=sig, order=2, normalize=False), sigkernel_amd.truncated_sig_kernel(*a, 4, sigma=sig, order=2))
        assert torch.equal(sigkernel_amd.truncated_sig_kernel(*a, 4, sigma=sig, order=2), _truncated_torch(*a, 4, sig, 2))
    assert torch.equal(sigkernel_amd.transforms.truncated_sig_kernel(X, Y, 4, sigma=sig, order=2, normalize=True),
                       sigkernel_amd.truncated_sig_kernel(X, Y, 4, sigma=sig, order=2, normalize=True))


def test_normalised_matrix_under_scaling(torch_only):
    """What X -> c X does at order = num_levels: level m of the kernel is homogeneous of degree m in each argument, so with every weight 1
        k(c x, y; 1) = k(x, y; sigma_m = c^m),     k(c x, c x; 1) = k(x, x; sigma_m = c^(2m)),
    and the normalised value of (c X, Y) is K(X, Y; c^m) / sqrt(k(X, X; c^(2m)) k(Y, Y; 1)) -- tested as that identity.  It is NOT invariant
    under c (the level-0 term 1 does not scale); exact invariance holds when ONE level m >= 1 carries all the weight, which is tested too."""
    import sigkernel_amd
    from sigkernel_amd.truncated import _truncated_paired_torch, _truncated_torch
    rng = np.random.default_rng(9)
    L = 4
    X, Y = torch.as_tensor(steps(rng, 3, 6, 2)), torch.as_tensor(steps(rng, 4, 5, 2))
    one = torch.ones(L + 1, dtype=torch.float64)
    base = sigkernel_amd.truncated_sig_kernel(X, Y, L, sigma=one, order=L, normalize=True)
    for c in (0.5, 3.0):
        got = sigkernel_amd.truncated_sig_kernel(c * X, Y, L, sigma=one, order=L, normalize=True)
        cm = torch.as_tensor([c ** m for m in range(L + 1)], dtype=torch.float64)
        want = _truncated_torch(X, Y, L, cm, L) / torch.sqrt(_truncated_paired_torch(X, X, L, cm * cm, L)[:, None] * _truncated_paired_torch(Y, Y, L, one, L)[None, :])
        assert rel(got, want) <= 1e-12
        assert (got - base).abs().max() > 1e-3          # ... and that is a different matrix
        for m in (1, 3):
            e = torch.zeros(L + 1, dtype=torch.float64)
            e[m] = 1.0
            a = sigkernel_amd.truncated_sig_kernel(X, Y, L, sigma=e, order=L, normalize=True)
            b = sigkernel_amd.truncated_sig_kernel(c * X, Y, L, sigma=e, order=L, normalize=True)
            assert (a - b).abs().max() <= 1e-12 * a.abs().max()


def test_normalising_needs_positive_self_kernels(torch_only):
    import sigkernel_amd
    rng = np.random.default_rng(10)
    small, large = torch.as_tensor(steps(rng, 3, 4, 2)), 10 * torch.as_tensor(steps(rng, 2, 4, 2))
    sig = torch.as_tensor([1.0, -1.0])          # k(x, x) = 1 - |sum of steps|^2
    assert (sigkernel_amd.truncated_sig_kernel_paired(small, small, 1, sigma=sig) > 0).all()
    assert (sigkernel_amd.truncated_sig_kernel_paired(large, large, 1, sigma=sig) < 0).all()
    with pytest.raises(ValueError, match="`X`"):
        sigkernel_amd.truncated_sig_kernel(large, small, 1, sigma=sig, normalize=True)
    with pytest.raises(ValueError, match="`Y`"):
        sigkernel_amd.truncated_sig_kernel(small, large, 1, sigma=sig, normalize=True)
    with pytest.raises(ValueError, match="`X`"):
        sigkernel_amd.truncated_sig_kernel(large, large, 1, sigma=sig, normalize=True)
    assert sigkernel_amd.truncated_sig_kernel(large, small, 1, sigma=sig).shape == (2, 3)      # the plain matrix does not care


def test_normalised_matrix_is_differentiable(torch_only):
    import sigkernel_amd
    rng = np.random.default_rng(12)
    X = torch.as_tensor(steps(rng, 2, 3, 2)).requires_grad_()
    Y = torch.as_tensor(steps(rng, 2, 3, 2)).requires_grad_()
    f = lambda x, y: sigkernel_amd.truncated_sig_kernel(x, y, 3, sigma=0.9, order=2, normalize=True)
    assert torch.autograd.gradcheck(f, (X, Y), eps=1e-6, atol=1e-7, rtol=1e-6)


def test_argument_errors(torch_only):
    import sigkernel_amd
    from sigkernel_amd.truncated import _truncated_paired_torch
    X, Y = torch.rand(3, 4, 3, dtype=torch.float64), torch.rand(3, 5, 3, dtype=torch.float64)
    for fn in (_truncated_paired_torch, sigkernel_amd.truncated_sig_kernel_paired):
        with pytest.raises(ValueError, match="same number of paths"):
            fn(X, Y[:2], 3)
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
            fn(X, Y, 3, 1., 4)
        with pytest.raises(ValueError, match="sigma"):
            fn(X, Y, 3, [1., 2., 3.])
        assert fn(X.float(), Y.float(), 3).dtype == torch.float32


def test_paired_function_is_a_product_path():
    """no stand-in: HIP devices only, like the rest of the library"""
    import sigkernel_amd
    X = torch.rand(2, 4, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sigkernel_amd.truncated_sig_kernel_paired(X, X, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sigkernel_amd.truncated_sig_kernel(X, X, 3, normalize=True)


def test_the_paired_entry_points_of_the_c_abi():
    from sigkernel_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sigkernel_amd.h")).read(), flags=re.S)
    lib = ctypes.CDLL(build.build())
    for name in ("sk_truncated_paired_f64", "sk_truncated_paired_f32"):
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[name.replace("paired", "gram")][1]) - 1
        assert hasattr(lib, name), name
    assert _lib.load().sk_version() == 340
    # argument errors before any HIP call, and the Gram entry points' scope
    p = ctypes.c_void_p(16)
    sg = (ctypes.c_double * 9)(*([1.0] * 9))
    f = _lib.load().sk_truncated_paired_f64
    assert f(None, p, 4, 8, 8, 8, 16, 3, 8, 2, 2, sg, p, None) == 1
    assert f(p, p, -1, 8, 8, 8, 16, 3, 8, 2, 2, sg, p, None) == 1
    assert f(p, p, 4, 7, 8, 8, 16, 3, 8, 2, 2, sg, p, None) == 1            # Mrows < M
    assert f(p, p, 0, 8, 8, 8, 16, 3, 8, 2, 2, sg, p, None) == 0            # no pairs: nothing to do
    assert f(p, p, 4, 65, 65, 8, 16, 3, 8, 2, 2, sg, p, None) == 2          # 65 rows at order 2: outside the route's scope
    assert f(p, p, 4, 8, 8, 8, 16, 17, 32, 2, 2, sg, p, None) == 2          # dim 17
    assert _lib.load().sk_truncated_paired_f32(p, p, 4, 8, 8, 8, 16, 3, 8, 9, 1, sg, p, None) == 2      # nine levels
