"""The instance ledger on the GPU: every case of tests/instance_cases.py makes its call under the launch trace, every instance the case
claims must be on that trace (a route change that moves the case off its kernel fails here, by name), and EVERY output of the call is
compared with the CPU oracle -- values per element, gradients per path (tests/instance_ledger.py).  tests/test_instance_ledger.py
proves, without a GPU, that the claims cover the whole variants table.

fp32 calls: the oracle is given the fp32-rounded inputs in fp64 and the bound is two fp32 ulps on top of the fp64 tolerance.  Where the
route hands fp32 arrays from launch to launch, or does the derivative Gram's finite differences in fp32 (the case's "f32_bound" names
the stage: instance_ledger.F32_STAGE_SOURCE has its source lines), the case adds 4 x the distance of instance_ledger.expected_f32_stage --
that stage restated in fp32 torch on the CPU, the rest in the oracle -- from the all-fp64 oracle; both numbers are in the case entry.
k' and k'' of fp32 paths get no such allowance (a finite difference of fp32 node values with eps = 1e-4 amplifies their rounding by
1e8): they are compared with the oracle's solve of the restated fp32 increments, at the derived bound, and the derivative solver's own
instances are claimed by calls of the solver on given increments (op "deriv").  The rescue kernels (k_screen, k_fused_rescue,
k_adj_rescue) are claimed only by cases with one legitimately large-kernel pair: with tame pairs they write nothing.
"""
import pytest
import torch

import instance_cases
import instance_ledger as L

pytestmark = pytest.mark.gpu

_NT = []


def _threads():
    if not _NT:
        from oracle import oracle as O
        _NT.append(max(1, min(16, O.max_threads(), torch.get_num_threads())))
    return _NT[0]


@pytest.mark.parametrize("case", instance_cases.CASES, ids=[c["label"].replace(" ", "_") for c in instance_cases.CASES])
def test_claimed_instances_are_launched_and_every_output_matches_the_oracle(case):
    import reach_sweep
    t = reach_sweep.inputs(case)
    out, names = L.traced(lambda: reach_sweep.execute(case, t))
    missing = [m for m in case["claims"] if m not in names]
    assert not missing, "case %r no longer launches %s" % (case["label"], missing)
    want = L.expected(case, t, _threads())
    bad = L.check_case(case, out, want)
    assert not bad, "case %r: %s" % (case["label"], "; ".join("%s worst at %s: %.3e > %.3e" % b for b in bad))
