"""(CPU) The kernels of function-valued paths against the reference's own outputs (tests/golden/functional.npz, written by
tests/golden/make_golden_functional.py): Gram_matrix, batch_kernel, features, CEXP / cos_exp_kernel; RBF_SQR_Kernel against the
product formula; and the host layer's dispatch, on the oracle-backed CPU back-end."""
import numpy as np
import pytest
import torch

from conftest import golden, rel_err, walk


def _f():
    return golden("functional")


def _kernels(f):
    import sigkernel_amd as S
    return {"linear_id": S.Linear_ID_Kernel(), "rbf_id": S.RBF_ID_Kernel(float(f["sigma"])),
            "rbf_cexp": S.RBF_CEXP_Kernel(float(f["sigma1"]), float(f["sigma2"]), int(f["n_freqs"]))}


def test_public_names_and_class_hierarchy():
    import sigkernel_amd as S
    for n in ("Linear_ID_Kernel", "RBF_ID_Kernel", "RBF_CEXP_Kernel", "RBF_SQR_Kernel", "CEXP", "cos_exp_kernel"):
        assert n in S.__all__ and hasattr(S, n)
    assert isinstance(S.RBF_ID_Kernel(1.0), S.RBFKernel) and isinstance(S.RBF_CEXP_Kernel(1.0, 2.0, 3), S.RBFKernel)
    assert isinstance(S.Linear_ID_Kernel(), S.LinearKernel)
    k = S.RBF_CEXP_Kernel(1.5, 2.5, 7)
    assert (k.sigma1, k.sigma, k.n_freqs) == (1.5, 2.5, 7)


@pytest.mark.parametrize("name", ["linear_id", "rbf_id", "rbf_cexp"])
def test_static_kernels_match_the_reference(name):
    f = _f()
    k = _kernels(f)[name]
    X, Y = torch.from_numpy(f["X"]), torch.from_numpy(f["Y"])
    A = X.shape[0]
    assert rel_err(k.Gram_matrix(X, Y).numpy(), f["static_gram_" + name]) <= 1e-14
    assert rel_err(k.batch_kernel(X, Y[:A]).numpy(), f["static_batch_" + name]) <= 1e-14
    # the feature map under the base kernel is the same static kernel
    Fx, Fy = k.features(X), k.features(Y)
    assert Fx.shape == (A, X.shape[1], X.shape[2] * X.shape[3])
    assert rel_err(k.base_kernel.Gram_matrix(Fx, Fy).numpy(), f["static_gram_" + name]) <= 1e-14


def test_cexp_matches_the_reference():
    import sigkernel_amd as S
    f = _f()
    X = torch.from_numpy(f["X"])
    n, s1 = int(f["n_freqs"]), float(f["sigma1"])
    assert rel_err(S.CEXP(X, n, s1).numpy(), f["cexp_X"]) <= 1e-14
    grid = torch.linspace(0, 1, X.shape[2], dtype=torch.float64)
    assert rel_err(S.cos_exp_kernel(grid[:, None] - grid[None, :], n_freqs=n, sigma=s1).numpy(), f["cos_exp"]) <= 1e-14
    # float32 paths: the operator matrix takes their dtype (the reference's float64 matrix fails in matmul there)
    c32 = S.CEXP(X.float(), n, s1)
    assert c32.dtype == torch.float32 and rel_err(c32.double().numpy(), f["cexp_X"]) <= 1e-5


def test_rbf_sqr_is_the_product_of_two_rbf_kernels():
    import sigkernel_amd as S
    gen = torch.Generator().manual_seed(1)
    X = walk(gen, 3, 7, 10).reshape(3, 7, 5, 2)
    Y = walk(gen, 4, 9, 10).reshape(4, 9, 5, 2)
    k = S.RBF_SQR_Kernel(2.0, 0.5)
    Xf, Yf = X.reshape(3, 7, -1), Y.reshape(4, 9, -1)
    d1 = ((Xf[:, None, :, None] - Yf[None, :, None]) ** 2).sum(-1)
    d2 = ((Xf[:, None, :, None] ** 2 - Yf[None, :, None] ** 2) ** 2).sum(-1)
    want = torch.exp(-d1 / 2.0) * torch.exp(-d2 / 0.5)
    assert rel_err(k.Gram_matrix(X, Y).numpy(), want.numpy()) <= 1e-14
    assert rel_err(k.batch_kernel(X, Y[:3]).numpy(), want[range(3), range(3)].numpy()) <= 1e-14
    assert rel_err(k.base_kernel.Gram_matrix(k.features(X), k.features(Y)).numpy(), want.numpy()) <= 1e-13


def test_four_d_paths_need_a_function_valued_kernel():
    import sigkernel_amd as S
    X = torch.zeros(2, 5, 3, 2, dtype=torch.float64)
    with pytest.raises(ValueError):
        S.SigKernel(S.LinearKernel(), 1).compute_Gram(X, X)
    with pytest.raises(ValueError, match="SigKernel"):
        S._SigKernelGram.apply(X, X, S.Linear_ID_Kernel(), 1)


def test_host_layer_maps_each_input_once(oracle_backend, monkeypatch):
    """The dispatch point: SigKernel runs the base kernel on features(X), mapping each distinct input once (X in
    compute_scoring_rule's K(X, X) and K(X, y) is one feature tensor); the values are those of the oracle on the 4-D class."""
    import sigkernel_amd as S
    from oracle import oracle as O
    f = _f()
    k = _kernels(f)["rbf_cexp"]
    X, Y = torch.from_numpy(f["X"]), torch.from_numpy(f["Y"])
    calls = []
    orig = type(k).features
    monkeypatch.setattr(type(k), "features", lambda self, t: calls.append(t) or orig(self, t))
    sk = S.SigKernel(k, int(f["dyadic"]))
    s = sk.compute_scoring_rule(X, Y[:1])
    assert len(calls) == 2 and calls[0] is X
    K_XX = O.gram_forward(X, X, k, int(f["dyadic"]))
    K_Xy = O.gram_forward(X, Y[:1], k, int(f["dyadic"]))
    A = X.shape[0]
    want = (K_XX.sum() - np.trace(K_XX)) / (A * (A - 1)) - 2 * K_Xy.mean()
    assert abs(float(s) - want) <= 1e-12 * max(1.0, abs(want))
    assert abs(float(s) - float(f["scoring_rbf_cexp"])) <= 1e-11 * max(1.0, abs(float(f["scoring_rbf_cexp"])))
