#!/usr/bin/env python3
"""The distance of the REFERENCE's arithmetic from the long-double yardstick on every case of tests/wide_value_regimes.py: its static
kernels as measure_value_regimes.py restates them (nodes from the points, in double), differenced in fp64 on the CPU, and autograd's
chain rule through them, against value_regimes.increments_ld / _chain_ld.  The GPU test's bound is base + 4 x this; nothing here imports
the product's kernels.  Increments: max |difference| / max(1, max |G|) (wide_value_regimes.scale_of); chain rule: per path relative to
the path's largest entry.  fv-* entries: the function-valued kernels of wide_value_regimes.FV_CASES through the oracle, in the instance
ledger's measures.  `offset` entries hold the maximum over value_regimes.OFFSET_SEEDS seeds, all others seed 0.

    python tests/golden/measure_wide_value_regimes.py        # rewrites tests/golden/wide_value_regimes.json
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import value_regimes as V  # noqa: E402
import wide_value_regimes as WV  # noqa: E402

PATH = os.path.join(HERE, "wide_value_regimes.json")


def main():
    out = {}
    for c in WV.CASES:
        key = WV.case_key(c)
        out[key] = WV.measure(c)
        print("%-64s r %.2e" % (key, out[key]), flush=True)
    for c in WV.FV_CASES:      # the function-valued kernels through the API: the oracle on the class's torch formula
        for key, r in WV.fv_measure(c).items():
            out[key] = r
            print("%-64s r %.2e" % (key, r), flush=True)
    out["_provenance"] = ("distance of the reference's arithmetic (fp64, nodes from the points) from the long-double yardstick; increments: "
                          "relative to max(1, max |G|), chain rule: value_regimes.grad_error; offset: maximum over %d seeds; "
                          "tests/golden/measure_wide_value_regimes.py" % V.OFFSET_SEEDS)
    with open(PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
