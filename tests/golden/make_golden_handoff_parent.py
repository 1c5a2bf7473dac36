"""Record tests/golden/handoff_parent.npz: values, gradients, second gradients through the retained graph and per-instance launch
counts of the calls of tests/test_gpu_handoff_parent.py::CASES on the commit BEFORE the forward-to-backward hand-off became an
explicit record, so that the record can be held to them bit for bit.

Needs a GPU and a checkout of that parent commit with its library built:

    python tests/golden/make_golden_handoff_parent.py PARENT_CHECKOUT [OUT.npz]

The package is imported from PARENT_CHECKOUT; the cases, their inputs and the way they are called come from this checkout's test
module, which the test itself replays.  Every case must be on the routes it is named for and reproduce its own bits when called again.
The file holds inputs (the walks' integer steps), results and launch counts -- data only."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main():
    parent = os.path.abspath(sys.argv[1])
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "handoff_parent.npz")
    sys.path.insert(0, parent)
    import torch
    import sigkernel_amd
    assert os.path.abspath(sigkernel_amd.__file__).startswith(parent + os.sep), sigkernel_amd.__file__
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import test_gpu_handoff_parent as T

    record = {}
    for case in T.CASES:
        name = case[0]
        sx, sy, w = T.inputs(case)
        X, Y, wd = T.tensors(case, sx, sy, w)
        with T.overrides(sigkernel_amd, case):
            routes = T.on_route(sigkernel_amd, case, X, Y)
        assert routes == case[8], (name, routes)
        val, g1, g2, launches = T.replay(sigkernel_amd, case, X, Y, wd)
        again = T.replay(sigkernel_amd, case, X, Y, wd)
        assert all(torch.equal(a, b) and bool(torch.isfinite(a).all()) for a, b in zip((val, g1, g2), again[:3])), name
        assert launches == again[3], (name, launches, again[3])
        record[name] = {"X": sx, "Y": sy, "w": w, "value": val.cpu().numpy(), "grad": g1.cpu().numpy(), "grad2": g2.cpu().numpy(),
                        "routes": routes, "launches": launches}
        print(name, routes, "second gradient equal:", torch.equal(g1, g2), flush=True)
        for what, counts in zip(("forward", "backward", "backward again"), launches):
            print("   ", what, counts, flush=True)
    T.save(out_path, record)
    back = T.load(out_path)
    assert all(np.array_equal(back[n][k], record[n][k]) for n in record for k in ("value", "grad", "grad2")), "the file does not give back what was recorded"
    print("wrote", out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
