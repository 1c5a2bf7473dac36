"""truncated_sig_kernel without a GPU: the torch restatement of the recursion (sigkernel_amd/truncated.py: _truncated_torch) on CPU
tensors against the reference's recorded outputs (tests/golden/truncated.npz, written by tests/golden/make_golden_truncated.py) and,
at full order, against an evaluation by Chen's identity written here -- explicit tensor levels of the piecewise-linear path with the
given steps, nothing shared with either implementation.

Bars: fp64 <= 1e-12 of the matrix's max-norm (the reference itself sits ~1e-15 from Chen on these shapes);
fp32 I/O rtol 1e-4 / atol 1e-5."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "truncated.npz")


def fixtures():
    z = np.load(GOLDEN)
    for c in range(int(z["n_cases"])):
        k = "c%02d_" % c
        yield c, z[k + "X"], z[k + "Y"], int(z[k + "num_levels"]), z[k + "sigma"], int(z[k + "order"]), z[k + "K"]


def sigma_arg(s):
    return float(s) if s.ndim == 0 else torch.as_tensor(s)


def assert_close(got, want, dtype, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if dtype == np.float64:
        err = np.abs(got - want).max() / np.abs(want).max()
        assert err <= 1e-12, (what, err)
    else:
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5, err_msg=str(what))


def chen_levels(steps, L):
    """levels 0..L of the signature of the piecewise-linear path with these steps: S <- S (x) exp(v), level by level"""
    D = steps.shape[1]
    S = [np.ones(())] + [np.zeros((D,) * m) for m in range(1, L + 1)]
    for v in steps:
        E = [np.ones(())]
        for m in range(1, L + 1):
            E.append(np.multiply.outer(E[-1], v) / m)
        S = [sum(np.multiply.outer(S[k], E[m - k]) for k in range(m + 1)) for m in range(L + 1)]
    return S


def chen_kernel(X, Y, L, sigma):
    sig = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (L + 1,))
    SX = [chen_levels(x, L) for x in X]
    SY = [chen_levels(y, L) for y in Y]
    return np.array([[sum(sig[m] * np.sum(sx[m] * sy[m]) for m in range(L + 1)) for sy in SY] for sx in SX])


def steps(rng, n, m, D, dtype=np.float64):
    v = rng.standard_normal((n, m, D))
    v *= rng.uniform(0.2, 0.5, (n, m, 1)) / np.linalg.norm(v, axis=2, keepdims=True)
    return v.astype(dtype)


def test_fixture_file_covers_what_it_should():
    cases = list(fixtures())
    assert {c[1].dtype for c in cases} == {np.dtype(np.float64), np.dtype(np.float32)}
    assert {c[3] for c in cases} == {1, 2, 3, 4, 5, 6}
    assert {c[5] for c in cases} >= {-1, 1, 2, 3}
    assert {c[1].shape[2] for c in cases} == {1, 3, 8, 12}
    assert {c[4].ndim for c in cases} == {0, 1}
    assert any(c[1].shape[0] != c[2].shape[0] for c in cases) and all(c[1].shape[1] != c[2].shape[1] for c in cases)
    assert all(max(c[1].shape[1], c[2].shape[1]) <= 12 for c in cases)


@pytest.mark.parametrize("case", range(17))
def test_torch_route_reproduces_the_reference(case):
    from sigkernel_amd.truncated import _truncated_torch
    c, X, Y, L, sigma, order, K = list(fixtures())[case]
    got = _truncated_torch(torch.as_tensor(X), torch.as_tensor(Y), L, sigma_arg(sigma), order)
    assert got.shape == K.shape and got.dtype == torch.as_tensor(X).dtype
    assert_close(got.numpy(), K, X.dtype.type, c)
    # tiled over rows of X by the workspace budget (one row per tile here): the same matrix, to the same bar
    tiled = _truncated_torch(torch.as_tensor(X), torch.as_tensor(Y), L, sigma_arg(sigma), order, workspace_bytes=1)
    assert_close(tiled.numpy(), K, X.dtype.type, (c, "tiled"))


@pytest.mark.parametrize("A,B,M,N,D,L,vector", [(3, 2, 7, 5, 2, 4, False), (3, 2, 7, 5, 2, 4, True), (2, 3, 20, 15, 3, 5, True),
                                                (2, 2, 4, 9, 1, 6, True), (2, 2, 1, 1, 3, 3, False), (1, 2, 3, 2, 5, 1, True)])
def test_full_order_is_the_truncated_signature_kernel(A, B, M, N, D, L, vector):
    from sigkernel_amd.truncated import _truncated_torch
    rng = np.random.default_rng(7 + M + 13 * N + L)
    X, Y = steps(rng, A, M, D), steps(rng, B, N, D)
    sigma = rng.uniform(0.5, 1.5, L + 1) if vector else 0.7
    want = chen_kernel(X, Y, L, sigma)
    for order in (-1, L):
        got = _truncated_torch(torch.as_tensor(X), torch.as_tensor(Y), L, torch.as_tensor(sigma) if vector else sigma, order)
        assert_close(got.numpy(), want, np.float64, (M, N, L, order))


def test_lower_orders_are_not_the_truncated_kernel():
    """order < num_levels is Kiraly and Oberhauser's approximation, a different number: the fixtures are its only truth"""
    from sigkernel_amd.truncated import _truncated_torch
    rng = np.random.default_rng(3)
    X, Y = torch.as_tensor(steps(rng, 3, 7, 2)), torch.as_tensor(steps(rng, 2, 5, 2))
    full = _truncated_torch(X, Y, 4, 1., -1)
    for order in (1, 2, 3):
        assert (full - _truncated_torch(X, Y, 4, 1., order)).abs().max() > 1e-6


def test_sigma_broadcasting_and_default_order():
    from sigkernel_amd.truncated import _truncated_torch
    rng = np.random.default_rng(5)
    X, Y = torch.as_tensor(steps(rng, 3, 6, 3)), torch.as_tensor(steps(rng, 2, 8, 3))
    L = 4
    base = _truncated_torch(X, Y, L, 0.9)
    for s in (np.float64(0.9), torch.tensor(0.9, dtype=torch.float64), np.full(L + 1, 0.9), torch.full((L + 1,), 0.9, dtype=torch.float64), [0.9] * (L + 1)):
        assert torch.allclose(_truncated_torch(X, Y, L, s), base, rtol=0, atol=1e-14)
    assert torch.equal(_truncated_torch(X, Y, L, 0.9, -1), _truncated_torch(X, Y, L, 0.9, L))
    assert torch.equal(_truncated_torch(X, Y, L, 0.9, 0), base)
    # a weight per level: linear in sigma
    e = torch.eye(L + 1, dtype=torch.float64)
    parts = [_truncated_torch(X, Y, L, e[m], 2) for m in range(L + 1)]
    w = torch.as_tensor(rng.uniform(0.5, 1.5, L + 1))
    assert torch.allclose(_truncated_torch(X, Y, L, w, 2), sum(w[m] * parts[m] for m in range(L + 1)), rtol=0, atol=1e-14)
    assert torch.equal(parts[0], torch.ones(3, 2, dtype=torch.float64))
    # K(X, Y) = K(Y, X)^T at every order (what the swapped HIP route rests on)
    for order in (1, 2, 3, 4):
        assert torch.allclose(_truncated_torch(X, Y, L, w, order), _truncated_torch(Y, X, L, w, order).t(), rtol=0, atol=1e-14)


def test_argument_errors():
    import sigkernel_amd
    from sigkernel_amd.truncated import _truncated_torch
    X, Y = torch.rand(2, 4, 3, dtype=torch.float64), torch.rand(3, 5, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="shape"):
        _truncated_torch(X[0], Y, 3)
    with pytest.raises(ValueError, match="same path dimension"):
        _truncated_torch(X, Y[..., :2], 3)
    with pytest.raises(ValueError, match="dtype and device"):
        _truncated_torch(X, Y.float(), 3)
    with pytest.raises(TypeError, match="float64 and float32"):
        _truncated_torch(X.half(), Y.half(), 3)
    with pytest.raises(ValueError, match="num_levels"):
        _truncated_torch(X, Y, 0)
    with pytest.raises(ValueError, match="order"):
        _truncated_torch(X, Y, 3, 1., 4)
    with pytest.raises(ValueError, match="sigma"):
        _truncated_torch(X, Y, 3, [1., 2., 3.])
    # the public function is a product path: HIP devices only, like the rest of the library
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sigkernel_amd.truncated_sig_kernel(X, Y, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sigkernel_amd.transforms.truncated_sig_kernel(X, Y, 3, sigma=0.5, order=1)


def test_route_table_states_the_kernel_scope():
    from sigkernel_amd import _lib
    from sigkernel_amd.truncated import truncated_route
    F, S, W = _lib.ROUTE_FUSED, _lib.ROUTE_STREAM, _lib.ROUTE_FUSED_SWAP
    for (D, M, N, L, order, es), want in {(8, 64, 64, 4, -1, 8): F, (8, 65, 64, 4, -1, 8): W, (8, 65, 65, 4, -1, 8): S, (8, 128, 128, 8, 1, 8): F,
                                          (8, 129, 128, 8, 1, 4): W, (8, 129, 130, 8, 1, 8): S, (16, 64, 128, 8, 4, 4): F, (16, 64, 129, 8, 4, 8): S,
                                          (17, 8, 8, 3, 1, 8): S, (4, 8, 8, 9, 1, 8): S, (4, 8, 8, 6, 5, 8): S, (4, 8, 8, 5, 5, 8): S,
                                          (4, 8, 8, 4, 4, 8): F, (1, 2, 3, 1, -1, 8): F, (8, 64, 256, 3, 2, 8): F, (8, 64, 257, 3, 2, 8): S,
                                          (4, 200, 40, 6, 3, 8): W, (4, 300, 40, 6, 3, 8): S}.items():
        assert truncated_route(D, M, N, L, order, es) == want, (D, M, N, L, order, es)


def test_torch_route_gradcheck():
    from sigkernel_amd.truncated import _truncated_torch
    rng = np.random.default_rng(11)
    X = torch.as_tensor(steps(rng, 2, 4, 2)).requires_grad_()
    Y = torch.as_tensor(steps(rng, 2, 3, 2)).requires_grad_()
    sig = torch.as_tensor(rng.uniform(0.5, 1.5, 5))
    for order in (-1, 1, 2):
        assert torch.autograd.gradcheck(lambda x, y: _truncated_torch(x, y, 4, sig, order), (X, Y), eps=1e-6, atol=1e-7, rtol=1e-6)
