"""Record tests/golden/stream_resume_parent.npz: the full prefix grid, its three slices and compute_Gram_ragged (the launches of
k_fwd_prefix that existed before the kernel learnt to resume a sweep from a kept column) on the commit BEFORE SigKernelStream, so that
the kernel with the resume mode in can be held to them bit for bit (tests/test_gpu_stream.py).

Needs a GPU and a checkout of that parent commit with its library built:

    python tests/golden/make_golden_stream_resume_parent.py PARENT_CHECKOUT [OUT.npz]

The package is imported from PARENT_CHECKOUT; the shapes, the seeded inputs and the calls come from this checkout's
tests/stream_resume_parent.py, which the test replays.  Every call must reproduce its own bits when made again.  The file holds
results and checksums of the inputs -- data only."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main():
    parent = os.path.abspath(sys.argv[1])
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "stream_resume_parent.npz")
    sys.path.insert(0, parent)
    import sigkernel_amd
    assert os.path.abspath(sigkernel_amd.__file__).startswith(parent + os.sep), sigkernel_amd.__file__
    assert not hasattr(sigkernel_amd, "open_stream"), "this is not the parent: it has streams already"
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import stream_resume_parent as R

    rec = R.record(sigkernel_amd)
    again = R.record(sigkernel_amd)
    assert sorted(rec) == sorted(again) and all(np.array_equal(rec[k], again[k]) for k in rec), "a call does not reproduce its own bits"
    assert all(np.isfinite(v).all() for v in rec.values())
    np.savez_compressed(out_path, **rec)
    back = dict(np.load(out_path, allow_pickle=False))
    assert sorted(back) == sorted(rec) and all(np.array_equal(back[k], rec[k]) for k in rec), "the file does not give back what was recorded"
    print("%s: %d arrays, %d bytes" % (out_path, len(rec), os.path.getsize(out_path)))


if __name__ == "__main__":
    main()
