"""SigKernel(exact_gradient=True), the parts that need no GPU: the recurrence of the discrete solver's exact adjoint (restated in
tests/exact_gradient_reference.py) against torch autograd through the plain forward loop, how far the reference's adjoint formula is
from that gradient, and the constructor's contract."""
import numpy as np
import pytest
import torch

import sigkernel_amd
from oracle import oracle as O
import exact_gradient_reference as R


@pytest.mark.parametrize("naive", [False, True])
@pytest.mark.parametrize("d", [0, 1, 2])
@pytest.mark.parametrize("shape", [(5, 4), (1, 3)])
def test_recurrence_is_the_gradient_of_the_forward_loop(shape, d, naive):
    """The restatement's W against torch autograd through its forward loop: 1e-12 relative (both are fp64; the loop has at most
    20 x 16 cells)."""
    rng = np.random.default_rng(100 * shape[0] + 10 * d + naive)
    inc = rng.normal(scale=0.3, size=shape)
    k, W = R.exact_adjoint(inc, d, naive)
    t = torch.from_numpy(inc).requires_grad_(True)
    kt = R.forward_torch(t, d, naive)
    (want,) = torch.autograd.grad(kt, t)
    assert abs(k - float(kt.detach())) <= 1e-13 * abs(float(kt.detach()))
    err = np.max(np.abs(W - want.numpy())) / np.max(np.abs(want.numpy()))
    assert err <= 1e-12, err


def reference_formula_dx(X, Y, w, kernel, d, naive):
    """dL/dX by the reference's adjoint formula (oracle.adjoint_coarse + increments_adjoint + the static kernel's VJP)"""
    return O.gram_grad_weighted(X, Y, w.numpy(), kernel, d, naive=naive)


def exact_dx_dy(X, Y, w, kernel, d, naive):
    """(dL/dX, dL/dY), L = sum(w * Gram), by torch autograd through the restatement's forward loop"""
    Xg, Yg = X.clone().requires_grad_(True), Y.clone().requires_grad_(True)
    gx, gy = torch.autograd.grad((R.gram_torch(Xg, Yg, kernel, d, naive) * w).sum(), (Xg, Yg))
    return gx.numpy(), gy.numpy()


@pytest.mark.parametrize("naive", [False, True])
@pytest.mark.parametrize("d", [0, 1, 2])
def test_reference_formula_is_not_the_gradient(d, naive):
    """On the fixed random-walk inputs (setup_paths: the GPU tests reuse them) the reference formula's dX is more than 10 % away,
    norm-wise, from the gradient of the computed Gram matrix."""
    X, Y, w = R.setup_paths()
    k = sigkernel_amd.LinearKernel()
    ref = reference_formula_dx(X, Y, w, k, d, naive)
    exact, _ = exact_dx_dy(X, Y, w, k, d, naive)
    gap = np.linalg.norm(ref - exact) / np.linalg.norm(exact)
    print("d=%d naive=%d: reference formula vs exact dX, norm-wise %.3f" % (d, naive, gap))
    assert gap > 0.10, gap


def test_exact_gradient_with_a_process_group_raises():
    with pytest.raises(NotImplementedError):
        sigkernel_amd.SigKernel(sigkernel_amd.LinearKernel(), 0, process_group=object(), exact_gradient=True)


def test_default_object_keeps_the_reference_formula():
    sk = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(1.0), 1)
    assert sk.exact_gradient is False
    assert sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(1.0), 1, exact_gradient=True).exact_gradient is True
    fk = sigkernel_amd.SigKernel(sigkernel_amd.RBF_ID_Kernel(1.0), 0, exact_gradient=True)
    assert fk._on_features()[0].exact_gradient is True      # the object that runs on the features keeps the mode
