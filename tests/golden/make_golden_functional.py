"""Generate tests/golden/functional.npz by running the REAL reference: its kernels of function-valued paths
(Linear_ID_Kernel, RBF_ID_Kernel, RBF_CEXP_Kernel; static_kernels.py:76-213) on 4-D paths (batch, T, Lx, d) with Lx * d = 48.

Container-only, like make_golden.py (which it leaves alone): needs the reference and its Cython solver built into oracle/_ref/ by
oracle/build_ref.py.  Only the .npz (inputs and expected outputs, pure data) is committed.

    python tests/golden/make_golden_functional.py

Contents: forward Gram values of the three kernels (sym=False and sym=True), one compute_scoring_rule value, CEXP / cos_exp_kernel
outputs, and the reference's own finite-difference gradients of compute_Gram(X, Y).sum() for the two ID kernels -- taken on the
FLATTENED 3-D paths, which the reference can differentiate (its backward builds Xh from X.shape[2] and fails on 4-D paths) -- with
their round-off noise against the reference's formula in long double (tests/ld_reference.py, as measure_grad_noise.py measures it).
Every array is float64.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]

from oracle.build_ref import import_reference  # noqa: E402

ref = import_reference()
from sigkernel import static_kernels as ref_static  # noqa: E402
from ld_reference import reference_gradient_ld, rel_err_ld  # noqa: E402

A, B, T, LX, DD, DYADIC = 3, 4, 8, 12, 4, 1
SIGMA, SIGMA1, SIGMA2, N_FREQS = 6.0, 2.0, 4.0, 5


def main():
    gen = torch.Generator().manual_seed(707)
    walk = lambda n: (torch.cumsum(torch.randn(n, T, LX * DD, generator=gen, dtype=torch.float64), 1) / np.sqrt(T)).reshape(n, T, LX, DD)
    X, Y = walk(A), walk(B)
    out = dict(X=X, Y=Y, dyadic=DYADIC, sigma=SIGMA, sigma1=SIGMA1, sigma2=SIGMA2, n_freqs=N_FREQS)
    kernels = {"linear_id": ref_static.Linear_ID_Kernel(), "rbf_id": ref_static.RBF_ID_Kernel(SIGMA),
               "rbf_cexp": ref_static.RBF_CEXP_Kernel(SIGMA1, SIGMA2, N_FREQS)}
    for name, k in kernels.items():
        sk = ref.SigKernel(k, dyadic_order=DYADIC)
        out["gram_" + name] = sk.compute_Gram(X, Y, sym=False)
        out["gram_sym_" + name] = sk.compute_Gram(X, X, sym=True)
        out["static_gram_" + name] = k.Gram_matrix(X, Y)
        out["static_batch_" + name] = k.batch_kernel(X, Y[:A])
    out["scoring_rbf_cexp"] = ref.SigKernel(kernels["rbf_cexp"], dyadic_order=DYADIC).compute_scoring_rule(X, Y[:1])
    out["cexp_X"] = ref_static.CEXP(X, N_FREQS, SIGMA1)
    grid = torch.linspace(0, 1, LX, dtype=torch.float64)
    out["cos_exp"] = ref_static.cos_exp_kernel(grid[:, None] - grid[None, :], n_freqs=N_FREQS, sigma=SIGMA1)
    Xf, Yf = X.reshape(A, T, -1), Y.reshape(B, T, -1)
    for name, kind, param in (("linear_id", "linear", 0.0), ("rbf_id", "rbf", SIGMA)):
        sk = ref.SigKernel(kernels[name], dyadic_order=DYADIC)
        Xg = Xf.clone().requires_grad_(True)
        sk.compute_Gram(Xg, Yf, sym=False).sum().backward()
        out["grad_" + name] = Xg.grad.clone()
        c = dict(X=Xf.numpy(), Y=Yf.numpy(), kernel=kind, param=param, dyadic=DYADIC, w=np.ones((A, B)))
        out["noise_grad_" + name] = rel_err_ld(out["grad_" + name].numpy(), reference_gradient_ld(c, "grad_w"))
    path = os.path.join(HERE, "functional.npz")
    np.savez_compressed(path, **{k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()})
    print("functional.npz %.1f KB" % (os.path.getsize(path) / 1024), {k: float(out[k]) for k in out if k.startswith("noise_")})


if __name__ == "__main__":
    main()
