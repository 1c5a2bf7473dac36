"""Record tests/golden/truncated_refactor_parent.npz: the outputs and launch counts of the calls of
tests/test_gpu_truncated_refactor.py::CASES on the HIP route of the commit BEFORE the truncated kernel's host side was folded, so that
the folded code can be held to them bit for bit.

Needs a GPU and a checkout of that parent commit with its library built:

    python tests/golden/make_golden_truncated_refactor_parent.py PARENT_CHECKOUT [OUT.npz]

The package is imported from PARENT_CHECKOUT; the cases, their inputs and the way they are called come from this checkout's test
module, which the test itself replays.  The file holds inputs, arguments, outputs and launch counts -- data only."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main():
    parent = os.path.abspath(sys.argv[1])
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "truncated_refactor_parent.npz")
    sys.path.insert(0, parent)
    import torch
    import sigkernel_amd
    assert os.path.abspath(sigkernel_amd.__file__).startswith(parent + os.sep), sigkernel_amd.__file__
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import test_gpu_truncated_refactor as T

    out = {}
    for case in T.CASES:
        name = case[0]
        X, Y, sigma = T.inputs(case)
        Xd = torch.as_tensor(X).cuda()
        Yd = Xd if Y is None else torch.as_tensor(Y).cuda()
        got, hit = T.replay(sigkernel_amd, case, Xd, Yd, None if sigma is None else torch.as_tensor(sigma))
        again, _ = T.replay(sigkernel_amd, case, Xd, Yd, None if sigma is None else torch.as_tensor(sigma))
        assert torch.equal(got, again) and bool(torch.isfinite(got).all()), name
        out[name + "_X"], out[name + "_out"] = X, got.cpu().numpy()
        out[name + "_launches"] = np.array([hit.get(T.ORDER1, 0), hit.get(T.GENERAL, 0)], dtype=np.int64)
        if Y is not None:
            out[name + "_Y"] = Y
        if sigma is not None:
            out[name + "_sigma"] = sigma
        print(name, out[name + "_out"].shape, out[name + "_out"].dtype, hit, flush=True)
    np.savez_compressed(out_path, **out)
    print("wrote", out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
