"""(GPU) Paths of more than 32 dims and function-valued paths.

The HIP route for LinearKernel / RBFKernel beyond 32 dims (sk_static_increments_* / sk_static_adjoint_* through k_static_wide_mfma)
against the generic route (Gram_matrix in torch + sk_increments, autograd through the static kernel), and the kernels of
function-valued paths (Linear_ID_Kernel, RBF_ID_Kernel, RBF_CEXP_Kernel, RBF_SQR_Kernel) through every SigKernel method against the
CPU oracle applied to the class's own Gram_matrix on the 4-D paths."""
import numpy as np
import pytest
import torch

from conftest import rel_err, walk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def be():
    from sigkernel_amd import _lib
    return _lib.get_backend()


def _kernels():
    import sigkernel_amd as S
    return [S.Linear_ID_Kernel(), S.RBF_ID_Kernel(3.0), S.RBF_CEXP_Kernel(2.0, 1.5, 4), S.RBF_SQR_Kernel(2.5, 1.2)]


def _paths(gen, A, T, Lx, d, dtype=torch.float64):
    return (walk(gen, A, T, Lx * d) * 2).reshape(A, T, Lx, d).to(dtype)


# ---- the route ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["linear", "rbf"])
@pytest.mark.parametrize("D", [33, 40, 64, 100, 257])
def test_wide_static_increments_match_the_generic_route(be, kind, D):
    import sigkernel_amd
    gen = torch.Generator().manual_seed(D)
    for (A, B, M, N) in ((3, 5, 70, 66), (2, 2, 2, 2), (1, 6, 130, 20)):
        for dtype in (torch.float64, torch.float32):
            X = (walk(gen, A, M, D) * 3).to(dtype).to(DEV)
            Y = (walk(gen, B, N, D) * 3).to(dtype).to(DEV)
            for scale in ((1.0, 0.7) if kind == "linear" else (0.5, 2.0)):
                k = sigkernel_amd.LinearKernel(scale) if kind == "linear" else sigkernel_amd.RBFKernel(scale)
                code = 0 if kind == "linear" else 1
                tol = 1e-13 if dtype == torch.float64 else 2e-6
                G = k.Gram_matrix(X.double(), Y.double())
                want = be.increments(G.contiguous()).cpu().numpy()
                got = be.static_increments(code, 1.0 if kind == "linear" else scale, X, Y, gram=True)
                assert got is not None and got.dtype == X.dtype
                assert got.shape == (A, B, M - 1, N - 1) and got.stride(-2) * got.element_size() % 128 == 0
                assert np.max(np.abs(got.double().cpu().numpy() - want)) <= tol * max(1.0, float(G.abs().max()))
                base = got.as_strided((A, B, M - 1, got.stride(-2)), got.stride())
                assert torch.all(base[..., N - 1:] == 0)
                n = min(A, B)
                Gp = k.batch_kernel(X[:n].double(), Y[:n].double())
                wantp = be.increments(Gp.contiguous()).cpu().numpy()
                gotp = be.static_increments(code, scale, X[:n].contiguous(), Y[:n].contiguous(), gram=False)
                assert gotp.shape == (n, M - 1, N - 1)
                assert np.max(np.abs(gotp.double().cpu().numpy() - wantp)) <= tol * max(1.0, float(Gp.abs().max()))
                basep = gotp.as_strided((n, M - 1, gotp.stride(-2)), gotp.stride())
                assert torch.all(basep[..., N - 1:] == 0)


@pytest.mark.parametrize("kind", ["linear", "rbf"])
@pytest.mark.parametrize("D", [33, 64, 257])
@pytest.mark.parametrize("gram", [True, False])
def test_wide_static_adjoint_matches_autograd(be, kind, D, gram):
    import sigkernel_amd
    gen = torch.Generator().manual_seed(11 + D)
    A, B, M, N = 3, 4, 50, 70
    for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 1e-4)):
        X = (walk(gen, A, M, D) * 3).to(dtype).to(DEV)
        Y = (walk(gen, B if gram else A, N, D) * 3).to(dtype).to(DEV)
        k = sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(1.7)
        code, param = (0, 1.0) if kind == "linear" else (1, 1.7)
        P = (A, B) if gram else (A,)
        W = torch.randn(P + (M - 1, N - 1), generator=gen, dtype=torch.float64).to(dtype).to(DEV)
        go = torch.randn(P, generator=gen, dtype=torch.float64).to(dtype).to(DEV)
        Xd = X.double().clone().requires_grad_(True)
        with torch.enable_grad():
            G = k.Gram_matrix(Xd, Y.double()) if gram else k.batch_kernel(Xd, Y.double())
        dG = be.increments_adjoint(W.double().contiguous(), go.double())
        (want,) = torch.autograd.grad(G, Xd, dG)
        got = be.static_adjoint(code, param, X, Y, W.contiguous(), go, gram)
        assert got.shape == X.shape and got.dtype == X.dtype
        assert rel_err(got.double().cpu().numpy(), want.cpu().numpy()) <= tol


@pytest.mark.parametrize("kind", ["linear", "rbf"])
@pytest.mark.parametrize("sym", [False, True])
def test_wide_gram_backward_never_materialises_the_static_gram(be, kind, sym, monkeypatch):
    """compute_Gram(...).sum().backward() at 64 dims runs on the HIP route (be.increments is never called) and equals the generic route
    -- a subclass, which _fused_static sends there -- to 1e-12."""
    import sigkernel_amd
    from sigkernel_amd import _lib
    base = sigkernel_amd.LinearKernel if kind == "linear" else sigkernel_amd.RBFKernel
    args = () if kind == "linear" else (4.0,)

    class _Generic(base):
        pass

    gen = torch.Generator().manual_seed(5)
    X = (walk(gen, 6, 30, 64) * 2).to(DEV)
    Y = X if sym else (walk(gen, 5, 40, 64) * 2).to(DEV)
    res = []
    for k in (_Generic(*args), base(*args)):
        if type(k) is base:
            def boom(*a, **kw):
                raise AssertionError("the static Gram went through be.increments")
            monkeypatch.setattr(type(be), "increments", boom)
        sk = sigkernel_amd.SigKernel(k, 1)
        Xg = X.clone().requires_grad_(True)
        K = sk.compute_Gram(Xg, Xg if sym else Y, sym=sym)
        K.sum().backward()
        res.append((K.detach().cpu().numpy(), Xg.grad.cpu().numpy()))
    monkeypatch.undo()
    assert rel_err(res[1][0], res[0][0]) <= 1e-12
    # (linear: the generic route differences the Gram matrix <x_p, y_q> -- cancellation of a few ulps of |G| per increment -- where the
    # HIP route forms <dx_p, dy_q> directly; measured 1.3e-12 apart at 64 dims with sym=True)
    assert rel_err(res[1][1], res[0][1]) <= (1e-12 if kind == "rbf" else 5e-12)
    assert isinstance(_lib.get_backend(), _lib.HipBackend)


def test_wide_edges(be):
    """Empty batches, a non-contiguous 4-D view, and 32 dims (the fused kernels) next to 33 (the new route)."""
    import sigkernel_amd
    from oracle import oracle as O
    gen = torch.Generator().manual_seed(3)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(2.0), 1)
    X = walk(gen, 3, 20, 40).to(DEV)
    assert sk.compute_Gram(X[:0], X).shape == (0, 3)
    assert sk.compute_Gram(X, X[:0]).shape == (3, 0)
    assert sk.compute_kernel(X[:0], X[:0]).shape == (0,)
    # a non-contiguous 4-D view through a kernel of function-valued paths
    big = _paths(gen, 4, 24, 12, 6).to(DEV)
    Xv = big[:, ::2, :, ::2]
    Yv = big[:3, 1::2, :, 1::2]
    assert not Xv.is_contiguous()
    k = sigkernel_amd.RBF_ID_Kernel(2.0)
    K = sigkernel_amd.SigKernel(k, 1).compute_Gram(Xv, Yv)
    assert rel_err(K.cpu().numpy(), O.gram_forward(Xv.cpu(), Yv.cpu(), k, 1)) <= 1e-12
    # 32 dims next to 33
    for D in (32, 33):
        for kind in ("linear", "rbf"):
            kk = sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(3.0)
            Xa, Ya = walk(gen, 3, 25, D).to(DEV), walk(gen, 4, 30, D).to(DEV)
            Xg = Xa.clone().requires_grad_(True)
            K = sigkernel_amd.SigKernel(kk, 1).compute_Gram(Xg, Ya)
            K.sum().backward()
            assert rel_err(K.detach().cpu().numpy(), O.gram_forward(Xa.cpu(), Ya.cpu(), kk, 1)) <= 1e-12
            assert rel_err(Xg.grad.cpu().numpy(), O.gram_grad_points(Xa.cpu(), Ya.cpu(), kk, 1).sum(1)) <= 1e-9


# ---- kernels of function-valued paths through the API ------------------------------------------------------------------------------

def _oracle_grad(k, X, Y, d, w):
    """d sum_ab w_ab k(x_a, y_b) / dX through the oracle's adjoint and autograd of the class's own Gram_matrix on 4-D paths."""
    from oracle import oracle as O
    Xd = X.detach().double().cpu().requires_grad_(True)
    Yd = Y.detach().double().cpu()
    with torch.enable_grad():
        G = k.Gram_matrix(Xd, Yd)
    _, W = O.adjoint_coarse(O.increments(G.detach().numpy()), d)
    dG = torch.from_numpy(O.increments_adjoint(W)) * torch.as_tensor(np.asarray(w, dtype=np.float64))[:, :, None, None]
    (g,) = torch.autograd.grad(G, Xd, grad_outputs=dG)
    return g.numpy()


@pytest.mark.parametrize("ki", range(4))
@pytest.mark.parametrize("d", [0, 1, 2])
def test_function_valued_kernels_match_the_oracle(ki, d):
    import sigkernel_amd
    from oracle import oracle as O
    k = _kernels()[ki]
    gen = torch.Generator().manual_seed(100 * ki + d)
    A, B, T, Lx, dd = 4, 3, 12, 12, 3          # Lx * d = 36 (> 32: the matrix-core route; SQR: 72 features)
    X, Y = _paths(gen, A, T, Lx, dd), _paths(gen, B, T + 3, Lx, dd)
    Xc, Yc = X.clone(), Y.clone()
    X, Y = X.to(DEV), Y.to(DEV)
    sk = sigkernel_amd.SigKernel(k, d)
    want = O.gram_forward(Xc, Yc, k, d)
    want_xx = O.gram_forward(Xc, Xc, k, d)
    # compute_Gram, both sym settings, with gradients
    Xg = X.clone().requires_grad_(True)
    K = sk.compute_Gram(Xg, Y)
    w = torch.linspace(-1, 1, A * B, dtype=torch.float64).reshape(A, B)
    (K * w.to(DEV)).sum().backward()
    assert rel_err(K.detach().cpu().numpy(), want) <= 1e-12
    assert rel_err(Xg.grad.cpu().numpy(), _oracle_grad(k, Xc, Yc, d, w.numpy())) <= 1e-9
    Xg = X.clone().requires_grad_(True)
    Ks = sk.compute_Gram(Xg, Xg, sym=True)
    Ks.sum().backward()
    assert rel_err(Ks.detach().cpu().numpy(), want_xx) <= 1e-12
    # the reference's 2x rule for sym=True (sigkernel.py:721-726): twice the first-argument gradient of sum K(X, X)
    assert rel_err(Xg.grad.cpu().numpy(), 2 * _oracle_grad(k, Xc, Xc, d, np.ones((A, A)))) <= 1e-9
    # compute_kernel (paired)
    Yp = _paths(gen, A, T + 1, Lx, dd)
    Kp = sk.compute_kernel(X, Yp.to(DEV))
    wantp = np.array([O.gram_forward(Xc[i:i + 1], Yp[i:i + 1], k, d)[0, 0] for i in range(A)])
    assert rel_err(Kp.cpu().numpy(), wantp) <= 1e-12
    # the scoring rules and the MMD
    y1 = Y[:1]
    Xg = X.clone().requires_grad_(True)
    s = sk.compute_scoring_rule(Xg, y1)
    s.backward()
    s_want = (want_xx.sum() - np.trace(want_xx)) / (A * (A - 1)) - 2 * want[:, :1].mean()
    assert abs(float(s) - s_want) <= 1e-12 * max(1.0, abs(s_want))
    g_want = (2 * _oracle_grad(k, Xc, Xc, d, (1 - np.eye(A)) / (A * (A - 1)))
              - 2 * _oracle_grad(k, Xc, Yc[:1], d, np.full((A, 1), 1. / A)))
    assert rel_err(Xg.grad.cpu().numpy(), g_want) <= 1e-9
    es = sk.compute_expected_scoring_rule(X, Y)
    es_want = (want_xx.sum() - np.trace(want_xx)) / (A * (A - 1)) - 2 * want.mean()
    assert abs(float(es) - es_want) <= 1e-12 * max(1.0, abs(es_want))
    want_yy = O.gram_forward(Yc, Yc, k, d)
    mmd = sk.compute_mmd(X, Y)
    mmd_want = ((want_xx.sum() - np.trace(want_xx)) / (A * (A - 1)) + (want_yy.sum() - np.trace(want_yy)) / (B * (B - 1))
                - 2 * want.mean())
    assert abs(float(mmd) - mmd_want) <= 1e-12 * max(1.0, abs(mmd_want))
    # compute_kernel_and_derivatives_Gram
    gamma = _paths(gen, A, T, Lx, dd)
    kk = sk.compute_kernel_and_derivatives_Gram(X, Y, gamma.to(DEV))
    kw = O.kgrad(Xc, Yc, gamma, k, d)
    # (the derivatives are the reference's finite differences with eps = 1e-4: a node's rounding comes back times 1 / eps and 1 / eps^2;
    # tolerances of tests/test_derivatives.py)
    for a, b, tol in zip(kk, kw, (1e-12, 1e-9, 2e-6)):
        assert rel_err(a.cpu().numpy(), b) <= tol


@pytest.mark.parametrize("ki", [0, 1])
def test_function_valued_fp32(ki):
    import sigkernel_amd
    from oracle import oracle as O
    k = _kernels()[ki]
    gen = torch.Generator().manual_seed(7 + ki)
    X, Y = _paths(gen, 3, 10, 20, 2), _paths(gen, 4, 14, 20, 2)
    sk = sigkernel_amd.SigKernel(k, 1)
    Xg = X.float().to(DEV).requires_grad_(True)
    K = sk.compute_Gram(Xg, Y.float().to(DEV))
    K.sum().backward()
    assert K.dtype == torch.float32 and Xg.grad.dtype == torch.float32
    Xr, Yr = X.float().double(), Y.float().double()
    assert rel_err(K.detach().double().cpu().numpy(), O.gram_forward(Xr, Yr, k, 1)) <= 1e-4
    assert rel_err(Xg.grad.double().cpu().numpy(), _oracle_grad(k, Xr, Yr, 1, np.ones((3, 4)))) <= 1e-3


# ---- against the reference's own fixtures --------------------------------------------------------------------------------------

def test_function_valued_kernels_match_the_reference_fixtures():
    import sigkernel_amd as S
    from conftest import golden
    f = golden("functional")
    kernels = {"linear_id": S.Linear_ID_Kernel(), "rbf_id": S.RBF_ID_Kernel(float(f["sigma"])),
               "rbf_cexp": S.RBF_CEXP_Kernel(float(f["sigma1"]), float(f["sigma2"]), int(f["n_freqs"]))}
    X, Y = torch.from_numpy(f["X"]).to(DEV), torch.from_numpy(f["Y"]).to(DEV)
    d = int(f["dyadic"])
    for name, k in kernels.items():
        sk = S.SigKernel(k, d)
        assert rel_err(sk.compute_Gram(X, Y).cpu().numpy(), f["gram_" + name]) <= 1e-11
        assert rel_err(sk.compute_Gram(X, X, sym=True).cpu().numpy(), f["gram_sym_" + name]) <= 1e-11
    sr = float(S.SigKernel(kernels["rbf_cexp"], d).compute_scoring_rule(X, Y[:1]))
    assert abs(sr - float(f["scoring_rbf_cexp"])) <= 1e-11 * max(1.0, abs(float(f["scoring_rbf_cexp"])))
    # gradients of sum_b K(x_a, y_b) on the flattened paths, the reference's own finite differences
    for name in ("linear_id", "rbf_id"):
        sk = S.SigKernel(kernels[name], d)
        Xg = X.clone().requires_grad_(True)
        sk.compute_Gram(Xg, Y).sum().backward()
        g = Xg.grad.reshape(X.shape[0], X.shape[1], -1).cpu().numpy()
        # (the rule of conftest.grad_tol, with the noise make_golden_functional.py measured against the long-double formula)
        assert rel_err(g, f["grad_" + name]) <= max(1e-6, 1.25 * float(f["noise_grad_" + name]))
