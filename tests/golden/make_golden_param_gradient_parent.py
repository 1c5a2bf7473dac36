"""Record tests/golden/param_gradient_parent.npz: the bits sk_static_adjoint_f64 (RBFKernel, a float sigma) returns on the commit BEFORE
k_static_rbf_adj got its parameter mode, so that the mode can be held to "off means the parent's dX, bit for bit".

Needs a GPU and a checkout of that parent commit with its library built:

    python tests/golden/make_golden_param_gradient_parent.py PARENT_CHECKOUT [OUT.npz]

The package is imported from PARENT_CHECKOUT; the cases and their inputs come from this checkout's test module
(tests/test_gpu_param_gradient.py: GOLDEN_CASES, golden_inputs), which replays them.  Every case must reproduce its own bits when called
again.  The file holds inputs and results -- data only."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main():
    parent = os.path.abspath(sys.argv[1])
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "param_gradient_parent.npz")
    sys.path.insert(0, parent)
    import torch
    import sigkernel_amd
    from sigkernel_amd import _lib
    assert os.path.abspath(sigkernel_amd.__file__).startswith(parent + os.sep), sigkernel_amd.__file__
    assert not hasattr(_lib.HipBackend, "static_adjoint_param"), "this is not the parent: it has the parameter mode"
    sys.path.insert(1, ROOT)
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import test_gpu_param_gradient as T

    be = _lib.HipBackend()
    record = {}
    for name in T.GOLDEN_CASES:
        X, Y, W, scale, sigma, gram = T.golden_inputs(name)
        args = (1, sigma, X.to(T.DEV), Y.to(T.DEV), W.to(T.DEV), scale.to(T.DEV), gram)
        dX, again = be.static_adjoint(*args), be.static_adjoint(*args)
        assert torch.equal(dX, again) and bool(torch.isfinite(dX).all()), name
        for key, t in (("X", X), ("Y", Y), ("W", W), ("scale", scale), ("dX", dX.cpu())):
            record[name + "/" + key] = t.numpy()
        record[name + "/sigma"] = np.float64(sigma)
        print(name, tuple(dX.shape), "max |dX| %.6g" % float(dX.abs().max()), flush=True)
    np.savez(out_path, **record)
    back = np.load(out_path)
    assert all(np.array_equal(back[k], v) for k, v in record.items()), "the file does not give back what was recorded"
    print("wrote", out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
