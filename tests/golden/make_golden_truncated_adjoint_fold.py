"""Record the two fixtures that hold the truncated kernel's folded adjoint host code to the commit BEFORE the fold:

* tests/golden/truncated_adjoint_fold_plans.npz (no GPU needed): the four sk_truncated_*adjoint_plan entry points over the thinned grid of
  tests/test_truncated_adjoint_fold_host.py, and the return codes of the four launch entry points on the calls that module lists, all
  of which the parent rejects before any HIP call.  The plans depend on the CU count: recorded WITHOUT a device the library takes 256,
  the MI355X's own, and on a device the maker insists on 256 -- the file states the assumption (`cu_count`);
* tests/golden/truncated_adjoint_fold_parent.npz (GPU): values, gradients and launch counts of
  tests/test_gpu_truncated_adjoint_fold.py::CASES, each run twice and required to give equal bits.

Needs a checkout of that parent commit with its library built:

    python tests/golden/make_golden_truncated_adjoint_fold.py PARENT_CHECKOUT [OUT_DIR]

The package is imported from PARENT_CHECKOUT; the grid, the cases, their inputs and the way they are called come from this checkout's
test modules, which the tests themselves replay.  Without a GPU only the first file is written.  Data only: inputs, arguments, outputs,
return codes and launch counts (the gradient cases' inputs are exact small numbers the test module builds itself: not stored)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def record_plans(lib, out_dir, cu_count):
    import test_truncated_adjoint_fold_host as H
    plans = H.record_plans(lib)
    names, rcs = H.record_launch_rcs(lib)
    assert set(np.unique(rcs)) <= {1, 2}, "a call of the list was not rejected"
    path = os.path.join(out_dir, "truncated_adjoint_fold_plans.npz")
    np.savez_compressed(path, plans=plans, launch_cases=np.array(names), launch_rc=rcs, cu_count=np.int64(cu_count))
    print("wrote", path, os.path.getsize(path), "bytes;", plans.shape[0], "shapes,", len(names), "rejected calls", flush=True)


def record_gradients(sigkernel_amd, lib, out_dir):
    import torch
    import test_gpu_truncated_adjoint_fold as T
    out = {}
    for case in T.CASES:
        name, sym, ws = case[0], case[7], case[8]
        if ws == T.ONE_BLOCK:
            ws = T.one_block_workspace(lib, case)
            out[name + "_ws"] = np.int64(ws)
        X, Y, sigma, c = T.inputs(case)
        Xd = torch.as_tensor(X).cuda()
        Yd = Xd if sym else torch.as_tensor(Y).cuda()
        args = (torch.as_tensor(sigma), torch.as_tensor(c).cuda(), ws)
        got, hit = T.replay(sigkernel_amd, case, Xd, Yd, *args)
        again, hit2 = T.replay(sigkernel_amd, case, Xd, Yd, *args)
        assert hit == hit2, (name, hit, hit2)
        for key, a, b in zip(("_K", "_dX", "_dY"), got, again):
            assert (a is None) == (b is None), (name, key)
            if a is not None:
                assert torch.equal(a, b) and bool(torch.isfinite(a).all()), (name, key, "the two runs differ")
                out[name + key] = a.cpu().numpy()
        out[name + "_launches"] = np.array([hit.get(T.ORDER1, 0), hit.get(T.GENERAL, 0)], dtype=np.int64)
        print(name, out[name + "_K"].shape, out[name + "_K"].dtype, hit, flush=True)
    path = os.path.join(out_dir, "truncated_adjoint_fold_parent.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes", flush=True)


def main():
    parent = os.path.abspath(sys.argv[1])
    out_dir = sys.argv[2] if len(sys.argv) > 2 else HERE
    sys.path.insert(0, parent)
    import torch
    import sigkernel_amd
    from sigkernel_amd import _lib
    assert os.path.abspath(sigkernel_amd.__file__).startswith(parent + os.sep), sigkernel_amd.__file__
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    lib = _lib.load()
    gpu = torch.cuda.is_available()
    cu_count = torch.cuda.get_device_properties(0).multi_processor_count if gpu else 256
    assert cu_count == 256, "the plans are recorded for 256 CUs, this device has %d" % cu_count
    record_plans(lib, out_dir, cu_count)
    if gpu:
        record_gradients(sigkernel_amd, lib, out_dir)
    else:
        print("no GPU: truncated_adjoint_fold_parent.npz not written")


if __name__ == "__main__":
    main()
