"""The oracle against the REAL reference, on inputs of its own.

tests/golden/reference_checks.npz holds inputs drawn for these tests alone (seeds other than the other fixtures') and what the
reference's own code returned for them (tests/golden/make_golden.py, section 7: its Cython solver, compute_Gram + backward, the
derivative stencil), so the pin does not rest on the other fixtures alone.  CPU only.
"""
import numpy as np
import pytest
import torch

from conftest import golden


@pytest.fixture(scope="module")
def ref():
    return golden("reference_checks")


@pytest.mark.parametrize("naive", [False, True])
def test_solver_bit_identical_on_fresh_random_increments(ref, naive):
    from oracle import oracle as O
    n = int(naive)
    for i in range(3):
        inc = ref["solver_n%d_inc%d" % (n, i)]
        assert np.array_equal(O.solve_fine(inc, naive), ref["solver_n%d_grid%d" % (n, i)])
    assert np.array_equal(O.solve_fine(ref["solver_n%d_inc4" % n], naive), ref["solver_n%d_grid4" % n])
    assert np.array_equal(O.gram_sym_fine(ref["solver_n%d_incs" % n], naive), ref["solver_n%d_grids" % n])


@pytest.mark.parametrize("kind,d", [("linear", 0), ("linear", 2), ("rbf", 1), ("rbf", 3)])
def test_gram_and_gradient_against_the_live_reference(ref, kind, d):
    import sigkernel_amd
    from oracle import oracle as O
    key = "gram_%s_d%d_" % (kind, d)
    X, Y, w = (torch.from_numpy(ref[key + k]) for k in ("X", "Y", "w"))
    K, ref_grad = ref[key + "K"], ref[key + "grad"]
    ok = sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(0.8)
    got = O.gram_forward(X, Y, ok, d)
    assert np.max(np.abs(got - K)) <= 1e-13 * np.max(np.abs(got))
    gp = O.gram_grad_points(X, Y, ok, d)
    grad = np.einsum("ab,abmd->amd", w.numpy(), gp)
    # the reference differentiates by forward differences with h = 1e-9 in double: measure ITS round-off noise against its own
    # formula in long double (tests/ld_reference.py); the analytic adjoint must sit within 1e-7 of that formula, and the
    # reference within its measured noise of it
    from ld_reference import reference_gradient_ld, rel_err_ld
    ld = reference_gradient_ld(dict(X=X.numpy(), Y=Y.numpy(), w=w.numpy(), dyadic=d, naive=0), "grad_w",
                               kernel=kind, param=0.8)
    assert rel_err_ld(grad, ld) <= 1e-7
    noise = rel_err_ld(ref_grad, ld)
    assert noise <= 2e-5       # sanity bound on the reference's own noise, not a parity tolerance
    assert np.max(np.abs(grad - ref_grad)) <= (noise + 1e-7) * np.max(np.abs(grad)) * 1.01


def test_derivative_stencil_against_the_live_reference(ref):
    from oracle import oracle as O
    k, kd, kdd, grids = O.solve_deriv_coarse(ref["deriv_inc"], ref["deriv_inc_d"], ref["deriv_inc_dd"], 0, want_grid=True)
    assert np.array_equal(grids[0], ref["deriv_K"]) and np.array_equal(grids[1], ref["deriv_Kd"]) and \
        np.array_equal(grids[2], ref["deriv_Kdd"])
