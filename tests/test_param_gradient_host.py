"""Gradients for the static kernel's own parameters under SigKernel(exact_gradient=True), the parts that need no GPU: the formula the
HIP kernel's parameter mode implements against torch autograd, the new C entry point's declaration / export / binding, and the host
plumbing -- parameter discovery, the gates, the trailing inputs of the three exact Functions, the tiling -- on an oracle-backed backend
without the one-launch method, i.e. through the generic branch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import sigkernel_amd
from sigkernel_amd import _lib
from sigkernel_amd import sigkernel as S
from conftest import ROOT
import exact_gradient_reference as R
import prefix_gradient_reference as PR
import param_gradient_reference as P


# ---- the formula (pins the reference, not the feature) -------------------------------------------------------------------------------

@pytest.mark.parametrize("naive", [False, True], ids=["default", "naive"])
@pytest.mark.parametrize("d", [0, 1])
@pytest.mark.parametrize("paired", [False, True], ids=["gram", "paired"])
def test_formula_equals_autograd_through_the_restatement(paired, d, naive):
    """sigma^-2 sum go dG G r2 against autograd of gram_torch with a tensor sigma: paths of 4 x 5 points, dim 2, 1e-12 relative"""
    X, Y = P.walks(3, 2, 4, 2), P.walks(4, 2 if paired else 3, 5, 2)
    go = torch.randn((2,) if paired else (2, 3), generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    s = torch.tensor(0.7, dtype=torch.float64, requires_grad=True)
    K = R.gram_torch(X, Y, sigkernel_amd.RBFKernel(s), d, naive, paired=paired)
    (want,) = torch.autograd.grad((K * go).sum(), s)
    got = P.formula_dsigma(X, Y, go, 0.7, d, naive, paired)
    print("formula %.17g autograd %.17g" % (got, float(want)))
    assert abs(got - float(want)) <= 1e-12 * abs(float(want))


# ---- the C entry point ------------------------------------------------------------------------------------------------------------------

def test_entry_point_is_declared_exported_and_bound_with_one_arity():
    name = "sk_static_adjoint_param_f64"
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sigkernel_amd.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, "not declared in the header"
    declared = len([a for a in m.group(1).split(",") if a.strip()])
    from sigkernel_amd import build
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, name), "not exported"
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == declared == 16
    assert _lib.load().sk_version() == 340
    # the older entry keeps its signature
    assert len(_lib.SIGNATURES["sk_static_adjoint_f64"][1]) == 14


def test_entry_point_refuses_by_argument_check_without_a_device():
    """kind 0 and D = 33: SK_ERR_UNSUPPORTED (2); null pointers, a wrong partial count, partials that do not follow dX: SK_ERR_BAD_ARG (1);
    the size query answers without touching memory.  No device exists here: every refusal is an argument check."""
    fn = _lib.load().sk_static_adjoint_param_f64
    p = ctypes.c_void_p(4096)
    A, B, M, N = 2, 3, 6, 5

    def call(kind=1, D=2, dX=4096, tail=None, count=None, X=p, n_ptr=True, sigma=0.7):
        need = ctypes.c_int64(0)
        if kind == 1 and D <= 32:
            assert fn(1, 0.7, None, None, None, 0, None, A, B, M, N, D, None, None, ctypes.byref(need), None) == 0
        n = ctypes.c_int64(need.value if count is None else count)
        tail = dX + 8 * A * M * D if tail is None else tail
        return fn(kind, sigma, X, p, p, 0, None, A, B, M, N, D, ctypes.c_void_p(dX), ctypes.c_void_p(tail) if tail else None,
                  ctypes.byref(n) if n_ptr else None, None), need.value

    assert call(kind=0)[0] == 2
    assert call(D=33)[0] == 2
    assert call(tail=0)[0] == 1                    # a null partial pointer
    assert call(count=5)[0] == 1                   # D = 2: four rows per block, 2 * ceil(6 / 4) = 4 partials
    assert call(D=2)[1] == 4 and call(D=11)[1] == 2 * 3 and call(D=20)[1] == 2 * 6
    assert call(tail=4096 + 8 * A * M * 2 + 8)[0] == 1      # partials not directly behind dX
    assert call(X=None)[0] == 1
    assert call(n_ptr=False)[0] == 1
    assert call(sigma=0.0)[0] == 1
    assert call(kind=2)[0] == 1


# ---- parameter discovery -------------------------------------------------------------------------------------------------------------------

def test_static_params():
    s = torch.tensor(0.7, dtype=torch.float64, requires_grad=True)
    assert S._static_params(sigkernel_amd.RBFKernel(s)) == (s,)
    assert S._static_params(sigkernel_amd.RBFKernel(torch.tensor([0.7], requires_grad=True)))[0].shape == (1,)
    assert S._static_params(sigkernel_amd.RBFKernel(0.7)) == ()
    assert S._static_params(sigkernel_amd.RBFKernel(torch.tensor(0.7))) == ()
    assert S._static_params(sigkernel_amd.RBFKernel(torch.tensor([0.7, 0.8], requires_grad=True))) == ()
    assert S._static_params(sigkernel_amd.LinearKernel(torch.tensor(0.7, requires_grad=True))) == ()      # out of scope
    k = P.LearnableCubic()
    assert [id(t) for t in S._static_params(k)] == [id(k.c), id(k.unused)]
    k.unused.requires_grad_(False)
    assert [id(t) for t in S._static_params(k)] == [id(k.c)]
    # the function-valued kernels hand a tensor sigma on unchanged
    assert sigkernel_amd.RBF_ID_Kernel(s).base_kernel.sigma is s
    assert sigkernel_amd.RBF_CEXP_Kernel(1.0, s, 3).base_kernel.sigma is s
    # a default object reads a tensor sigma as its value
    assert sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(s), 0)._params() == ()
    assert sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(s), 0, exact_gradient=True)._params() == (s,)


# ---- host plumbing through the generic branch ---------------------------------------------------------------------------------------

@pytest.fixture
def param_backend():
    prev = _lib.set_backend(P.ParamExactBackend())
    yield
    _lib.set_backend(prev)


LX, LY = [4, 2], [5, 3, 2]


def _call(method, sk, X, Y):
    if method == "gram":
        return sk.compute_Gram(X, Y)
    if method == "kernel":
        return sk.compute_kernel(X, Y[:X.shape[0]])
    if method == "ragged":
        return sk.compute_Gram_ragged(X, Y, LX, LY)
    return sk.compute_Gram_prefixes(X, Y, nodes="diagonal")


def _reference(method, kernel, X, Y, d):
    """(outputs, pair axes) of the restatement"""
    if method == "gram":
        return R.gram_torch(X, Y, kernel, d), 2
    if method == "kernel":
        return R.gram_torch(X, Y[:X.shape[0]], kernel, d, paired=True), 1
    if method == "ragged":
        return torch.stack([torch.stack([R.gram_torch(X[a:a + 1, :LX[a]], Y[b:b + 1, :LY[b]], kernel, d)[0, 0] for b in range(Y.shape[0])])
                            for a in range(X.shape[0])]), 2
    return PR.slice_nodes(PR.prefix_grid_torch(X, Y, kernel, d), "diagonal"), 2


@pytest.mark.parametrize("d", [0, 1])
@pytest.mark.parametrize("method", ["gram", "kernel", "ragged", "prefixes"])
def test_only_sigma_requires_grad(param_backend, method, d):
    """2 x 3 pairs of 4 x 5 points with sigma the only tensor requiring grad: the call is differentiated, the paths get no gradient,
    and sigma.grad is autograd's through the restatement to 1e-9 x sum_p |d L_p / d sigma|"""
    X, Y = P.walks(11, 2, 4, 2), P.walks(12, 3, 5, 2)
    s = torch.tensor(0.7, dtype=torch.float64, requires_grad=True)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(s), d, exact_gradient=True)
    out = _call(method, sk, X, Y)
    assert out.grad_fn is not None
    go = torch.randn(out.shape, generator=torch.Generator().manual_seed(13), dtype=torch.float64)
    (out * go).sum().backward()
    assert X.grad is None and Y.grad is None
    assert s.grad is not None and s.grad.shape == s.shape and s.grad.dtype == s.dtype
    sr = torch.tensor(0.7, dtype=torch.float64, requires_grad=True)
    ref, pair_dims = _reference(method, sigkernel_amd.RBFKernel(sr), X, Y, d)
    assert float((out.detach() - ref.detach()).abs().max()) <= 1e-12 * float(ref.detach().abs().max())
    (want, scale), = P.per_pair_gradients(ref, go, pair_dims, (sr,))
    err = abs(float(s.grad) - float(want))
    print("%s d=%d: sigma.grad %.15g, |error| / sum_p |terms| = %.3e" % (method, d, float(s.grad), err / scale))
    assert err <= P.GRAD_BAR * scale


def test_paths_and_sigma_together(param_backend):
    """with X, Y and sigma all requiring grad the three gradients are those of autograd, and the paths' are those of a float-sigma call"""
    Xc, Yc = P.walks(11, 2, 4, 2), P.walks(12, 3, 5, 2)
    go = torch.randn(2, 3, generator=torch.Generator().manual_seed(13), dtype=torch.float64)
    grads = []
    for sigma in (torch.tensor(0.7, dtype=torch.float64, requires_grad=True), 0.7):
        X, Y = Xc.clone().requires_grad_(True), Yc.clone().requires_grad_(True)
        sk = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(sigma), 1, exact_gradient=True)
        (sk.compute_Gram(X, Y) * go).sum().backward()
        grads.append((X.grad, Y.grad))
    s = sigma = None
    for a, b in zip(*grads):
        assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())
    Xr, Yr = Xc.clone().requires_grad_(True), Yc.clone().requires_grad_(True)
    sr = torch.tensor(0.7, dtype=torch.float64, requires_grad=True)
    wx, wy, ws = torch.autograd.grad((R.gram_torch(Xr, Yr, sigkernel_amd.RBFKernel(sr), 1) * go).sum(), (Xr, Yr, sr))
    assert float((grads[0][0] - wx).abs().max()) <= P.GRAD_BAR * float(wx.abs().max())
    assert float((grads[0][1] - wy).abs().max()) <= P.GRAD_BAR * float(wy.abs().max())


def test_sigma_gradient_keeps_shape_dtype_and_sums_over_the_loss_wrappers(param_backend):
    """a (1,) fp32 sigma with fp64 paths: its gradient has its shape and dtype; compute_mmd is a composition in this mode, so sigma.grad
    is autograd's sum over the three Gram matrices"""
    X, Y = P.walks(11, 3, 4, 2), P.walks(12, 3, 5, 2)
    s = torch.tensor([0.75], dtype=torch.float32, requires_grad=True)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(s), 0, exact_gradient=True)
    sk.compute_mmd(X, Y).backward()
    assert s.grad.shape == (1,) and s.grad.dtype == torch.float32

    def off_diagonal_mean(K):
        return (K.sum() - torch.diag(K).sum()) / (K.shape[0] * (K.shape[0] - 1.))
    sr = torch.tensor(0.75, dtype=torch.float64, requires_grad=True)
    k = sigkernel_amd.RBFKernel(sr)
    mmd = off_diagonal_mean(R.gram_torch(X, X, k, 0)) + off_diagonal_mean(R.gram_torch(Y, Y, k, 0)) - 2. * R.gram_torch(X, Y, k, 0).mean()
    (want,) = torch.autograd.grad(mmd, sr)
    assert abs(float(s.grad) - float(want)) <= 1e-6 * abs(float(want))          # (the gradient is rounded to fp32)


def test_default_object_reads_a_tensor_sigma_as_its_value(param_backend):
    s = torch.tensor(0.7, dtype=torch.float64, requires_grad=True)
    X, Y = P.walks(11, 2, 4, 2), P.walks(12, 3, 5, 2)
    K = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(s), 1).compute_Gram(X, Y)
    assert K.grad_fn is None and not K.requires_grad
    assert torch.equal(K, sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(0.7), 1).compute_Gram(X, Y))
    with torch.no_grad():        # and under no_grad the exact object does not build a graph either
        assert sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(s), 1, exact_gradient=True).compute_Gram(X, Y).grad_fn is None


def test_one_point_paths_give_the_parameters_zeros(param_backend):
    s = torch.tensor(0.7, dtype=torch.float64, requires_grad=True)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(s), 1, exact_gradient=True)
    sk.compute_Gram(P.walks(1, 2, 1, 2), P.walks(2, 3, 5, 2)).sum().backward()
    assert s.grad is not None and float(s.grad) == 0.0


@pytest.mark.parametrize("kernel", ["rbf", "module"])
def test_module_parameters_and_row_tiles(param_backend, kernel, monkeypatch):
    """a torch.nn.Module static kernel with a learnable coefficient (and a parameter it never uses: zeros), and RBFKernel's sigma: 7 x 3
    pairs with a workspace that holds 2 rows of a tile -- at least 3 row tiles, the same parameter gradients to 1e-12 -- and against
    autograd through the restatement"""
    Xc, Yc = 0.5 * P.walks(21, 7, 4, 2), 0.5 * P.walks(22, 3, 5, 2)
    go = torch.randn(7, 3, generator=torch.Generator().manual_seed(23), dtype=torch.float64)
    calls = []
    real = P.ParamExactBackend.solve_adj

    def counted(self, *a, **kw):
        calls.append(kw.get("discrete", False))
        return real(self, *a, **kw)
    monkeypatch.setattr(P.ParamExactBackend, "solve_adj", counted)

    def make():
        if kernel == "rbf":
            k = sigkernel_amd.RBFKernel(torch.tensor(0.7, dtype=torch.float64, requires_grad=True))
            return k, (k.sigma,)
        k = P.LearnableCubic()
        return k, (k.c, k.unused)
    out = []
    for ws in (None, 2 * 2 * (3 if kernel == "rbf" else 8) * 3 * 4 * 5 * 8):
        del calls[:]
        k, params = make()
        sk = sigkernel_amd.SigKernel(k, 1, workspace_bytes=ws, exact_gradient=True)
        X = Xc.clone().requires_grad_(True)
        (sk.compute_Gram(X, Yc) * go).sum().backward()
        assert all(calls)
        out.append(([p.grad for p in params] + [X.grad], len(calls)))
    assert out[0][1] == 1 and out[1][1] >= 3, (out[0][1], out[1][1])
    for a, b in zip(out[0][0], out[1][0]):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-12 * max(float(a.abs().max()), 1e-300)
    k, params = make()
    ref = R.gram_torch(Xc, Yc, k, 1)
    for got, (want, scale) in zip(out[0][0], P.per_pair_gradients(ref, go, 2, params)):
        assert got.shape == want.shape
        if scale == 0.0:
            assert not got.any()          # the unused parameter
        else:
            assert float((got - want).abs().max()) <= P.GRAD_BAR * scale
