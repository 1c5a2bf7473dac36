"""Record tests/golden/ragged_nodes_parent.npz: plain solve_fwd (sk_solve_fwd_*) on seeded increments -- fp64 and fp32, the streaming
kernel alone (SK_FLAG_FAST_ONLY) and the anti-diagonal kernel (SK_FLAG_SIMPLE), dyadic 0-3, both stencils, every geometry of
k_fwd_wave -- on the commit BEFORE the two solvers learnt to keep one node per pair (sk_solve_fwd_at_*), so that the kernels with the
mode in can be held to the launches that existed, bit for bit (tests/test_gpu_ragged_nodes.py).

Needs a GPU and a checkout of that parent commit with its library built:

    python tests/golden/make_golden_ragged_nodes_parent.py PARENT_CHECKOUT [OUT.npz]

The package is imported from PARENT_CHECKOUT; the shapes, the seeded inputs and the calls come from this checkout's
tests/ragged_nodes_cases.py, which the test replays.  Every call must reproduce its own bits when made again.  The file holds results
only -- data."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main():
    parent = os.path.abspath(sys.argv[1])
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "ragged_nodes_parent.npz")
    sys.path.insert(0, parent)
    import sigkernel_amd
    from sigkernel_amd import _lib
    assert os.path.abspath(sigkernel_amd.__file__).startswith(parent + os.sep), sigkernel_amd.__file__
    assert "sk_solve_fwd_at_f64" not in _lib.SIGNATURES, "this is not the parent: it has the per-pair end node already"
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import ragged_nodes_cases as R

    rec = R.record(_lib)
    again = R.record(_lib)
    assert sorted(rec) == sorted(again) and all(np.array_equal(rec[k], again[k]) for k in rec), "a call does not reproduce its own bits"
    assert all(np.isfinite(v).all() for v in rec.values())
    np.savez_compressed(out_path, **rec)
    back = dict(np.load(out_path, allow_pickle=False))
    assert sorted(back) == sorted(rec) and all(np.array_equal(back[k], rec[k]) for k in rec), "the file does not give back what was recorded"
    print("%s: %d arrays, %d bytes" % (out_path, len(rec), os.path.getsize(out_path)))


if __name__ == "__main__":
    main()
