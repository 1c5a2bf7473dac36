"""(GPU) k_static_wide_mfma in its three modes against the LONG-DOUBLE yardstick, launch by launch, on the value-regime families at the
kernel's tiling boundaries (tests/wide_value_regimes.py: the case table, the bounds and where they come from).

Each case calls be.static_increments or be.static_adjoint directly under the launch trace.  The bound is base + 4 x the recorded distance
of the reference's arithmetic from the yardstick (tests/golden/wide_value_regimes.json); LinearKernel gets the base alone on offset
paths.  Beside the bounds, bit for bit: the padding columns of every increment row are zero, increments whose four nodes lie below the
subnormal limit are zero, a repeated point gives zero LinearKernel increments, and a NaN or inf coordinate reaches exactly what touches
its node.

With SK_VALUE_REGIMES_REPORT=<file> every case appends its measured error and bound to that file (profiles/wide_value_regimes.txt)."""
import json
import os

import numpy as np
import pytest
import torch

import instance_ledger as L
import value_regimes as V
import wide_value_regimes as WV
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
CLAIM = "k_static_wide_mfma"

with open(os.path.join(GOLDEN, "wide_value_regimes.json")) as _f:
    RECORDED = json.load(_f)


def _report(line):
    print(line)
    path = os.environ.get("SK_VALUE_REGIMES_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.fixture(scope="module")
def be():
    from sigkernel_amd import _lib
    return _lib.get_backend()


def _dev(a, f32=False):
    return torch.from_numpy(np.array(a)).to(torch.float32 if f32 else torch.float64).cuda()      # (a copy: the table's inputs are read-only)


def _increments(be, kind, sigma, X, Y, gram, f32=False):
    """-> (increments numpy fp64, the padded rows [.., M-1, ld] as a tensor, launched names)"""
    inc, names = L.traced(lambda: be.static_increments(0 if kind == "linear" else 1, 1.0 if kind == "linear" else sigma, _dev(X, f32), _dev(Y, f32), gram))
    assert inc.dtype == (torch.float32 if f32 else torch.float64) and inc.stride(-2) * inc.element_size() % 128 == 0
    padded = inc.as_strided(inc.shape[:-1] + (inc.stride(-2),), inc.stride())
    return inc.double().cpu().numpy(), padded, names


def _adjoint(be, kind, sigma, X, Y, W, go, gram, f32=False):
    g, names = L.traced(lambda: be.static_adjoint(0 if kind == "linear" else 1, 1.0 if kind == "linear" else sigma, _dev(X, f32), _dev(Y, f32),
                                                  _dev(W, f32), _dev(go, f32), gram))
    assert g.shape == X.shape and g.dtype == (torch.float32 if f32 else torch.float64)
    return g.double().cpu().numpy(), names


@pytest.mark.parametrize("case", WV.CASES, ids=[WV.case_id(c) for c in WV.CASES])
def test_wide_kernel_matches_the_long_double_yardstick(be, case):
    mode, kind, fam, lab, st, g, f32 = case
    X, Y, W, go, sigma = WV.case_inputs(case)
    want, G = WV.case_want(case)
    tol = WV.tolerance(case, RECORDED)
    if mode == "inc":
        got, padded, names = _increments(be, kind, sigma, X, Y, g["gram"], f32)
        err = WV.increments_error(got, want, WV.scale_of(kind, want, G))
        assert torch.all(padded[..., g["N"] - 1:] == 0), "padding columns are not zero"
        if fam == "drift":
            dead = WV.dead_increments(X, Y, sigma, g["gram"])
            assert lab != "s=30" or dead.sum() >= 8
            assert np.all(got[dead] == 0), "an increment of four nodes below the subnormal limit is not exactly 0"
    else:
        got, names = _adjoint(be, kind, sigma, X, Y, W, go, g["gram"], f32)
        err = V.grad_error(got, want)
    _report("%-4s %-6s %-7s %-14s %-26s %.2e  bound %.2e%s" % (mode, kind, fam, lab, WV.geometry_key(g, f32), err, tol,
                                                             "  invariant" if WV.invariant(case) else ""))
    if mode == "inc" or kind == "rbf":      # (LinearKernel's chain rule beyond 32 dims is the library GEMM with dY)
        assert any(CLAIM in n for n in names), sorted(names)
    assert err <= tol, "%s: %.3e > %.3e" % (WV.case_id(case), err, tol)


# ------------------------------------------------------------------------------------------------------------------- exact claims
def _exact_bound(kind, sigma, X, Y, W, go):
    """base + 4 r of the exact-claim inputs (unit walks at +3: not a recorded case), r measured here on the CPU; LinearKernel: base alone
    -> (increments, chain rule)"""
    ref_inc, ref_g = WV.reference_arithmetic(kind, sigma, X, Y, W, go, True)
    inc, G = V.increments_ld(kind, sigma, X, Y)
    chain = WV.chain_ld(kind, sigma, X, Y, G, W, go, True)
    scale = WV.scale_of(kind, inc, G)
    k = 0.0 if kind == "linear" else 4.0
    return (inc, scale, WV.INC_BASE + k * WV.increments_error(ref_inc, inc, scale)), (chain, WV.GRAD_BASE + k * V.grad_error(ref_g, chain))


def test_a_repeated_point_gives_exactly_zero_linear_increments(be):
    X, Y, _, _ = WV.exact_inputs()
    X, Y = X.copy(), Y.copy()
    (a, p), (b, q) = WV.REPEAT_X, WV.REPEAT_Y
    X[a, p + 1], Y[b, q + 1] = X[a, p], Y[b, q]
    inc, _, names = _increments(be, "linear", None, X, Y, True)
    assert any(CLAIM in n for n in names)
    assert np.all(inc[a, :, p] == 0) and np.all(inc[:, b, :, q] == 0)
    assert np.count_nonzero(inc) == inc.size - inc[a, :, p].size - inc[:, b, :, q].size + inc[a, b, p, q].size


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("side", ["X", "Y"])
@pytest.mark.parametrize("kind, sigma", [("linear", None), ("rbf", 0.8)])
def test_a_non_finite_coordinate_reaches_exactly_what_touches_its_node(be, kind, sigma, side, bad):
    """One NaN or inf coordinate in one node of x_1 or y_4 (a dim of the last, partial chunk; the node on a tile's edge).  Increments: the two
    rows (columns) around the node are NaN in every pair of that path.  dL/dX, RBF: row `node` of x_1, or every row of every x for a node
    of y; LinearKernel: W @ dY never reads X -- a bad x leaves the gradient finite -- and a bad y reaches coordinate BAD_DIM of every
    row.  An inf coordinate gives NaN through inf - inf in |x|^2 - 2 <x, y> (RBF, coordinates of one sign, as in the reference) and +-inf or
    NaN through inf times a finite step (LinearKernel).  Everything else stays within its bound."""
    X, Y, W, go = WV.exact_inputs()
    (inc_want, scale, inc_tol), (g_want, g_tol) = _exact_bound(kind, sigma, X, Y, W, go)
    Xb, Yb = X.copy(), Y.copy()
    path, node = WV.BAD_X if side == "X" else WV.BAD_Y
    (Xb if side == "X" else Yb)[path, node, WV.BAD_DIM] = bad
    m_inc, m_rbf, m_lin = WV.touched(X.shape[1], Y.shape[1], WV.EXACT_GEOMETRY, side, path, node)
    hit = (lambda a: np.isnan(a)) if kind == "rbf" or np.isnan(bad) else (lambda a: ~np.isfinite(a))

    inc, padded, _ = _increments(be, kind, sigma, Xb, Yb, True)
    assert np.all(hit(inc[m_inc])), "a row around the node is not NaN"
    assert np.all(np.isfinite(inc[~m_inc]))
    err = float(np.max(np.abs(inc[~m_inc] - inc_want[~m_inc]))) / scale
    assert err <= inc_tol, (err, inc_tol)
    assert torch.all(padded[..., Y.shape[1] - 1:] == 0)

    g, _ = _adjoint(be, kind, sigma, Xb, Yb, W, go, True)
    m_g = np.zeros(g.shape, bool)
    if kind == "rbf":
        m_g[m_rbf] = True
    else:
        m_g[m_lin, WV.BAD_DIM] = True
    assert np.all(hit(g[m_g])), "a gradient row that touches the node is not NaN"
    assert np.all(np.isfinite(g[~m_g]))
    filled = np.where(m_g, g_want.astype(np.float64), g)      # (the measure is per path: the touched entries take the yardstick's values)
    gerr = V.grad_error(filled, g_want)
    _report("nonfinite %-6s %s %-3s increments %.2e (bound %.2e)  chain rule %.2e (bound %.2e)" % (kind, side, "nan" if np.isnan(bad) else "inf",
                                                                                                  err, inc_tol, gerr, g_tol))
    assert gerr <= g_tol, (gerr, g_tol)


# ------------------------------------------------------------------------------------------------------------------- function-valued kernels
@pytest.mark.parametrize("case", WV.FV_CASES, ids=["%s-%s-%s" % c[:3] for c in WV.FV_CASES])
def test_function_valued_kernels_match_their_formula_in_long_double(case):
    """RBF_ID_Kernel (values and gradient) and RBF_SQR_Kernel (values) through compute_Gram on 4-D paths with Lx d = 36, `scale` and `offset`
    families, against the class's own formula in long double from differences (RBF_SQR: x^2 - y^2 as (x - y)(x + y)).  Bound: the ledger's
    base + 4 x the recorded distance of the oracle on the class's torch formula."""
    import sigkernel_amd
    cls, fam, lab, st = case
    X, Y, w = WV.fv_inputs(case)
    k = sigkernel_amd.RBF_ID_Kernel(st["sigma"]) if cls == "rbf_id" else sigkernel_amd.RBF_SQR_Kernel(st["sigma"], WV.fv_sigma2(st))
    sk = sigkernel_amd.SigKernel(k, WV.FV_SHAPE["d"])

    def call():
        Xg = _dev(X).reshape(X.shape[0], X.shape[1], WV.FV_LX, WV.FV_D).requires_grad_(True)
        K = sk.compute_Gram(Xg, _dev(Y).reshape(Y.shape[0], Y.shape[1], WV.FV_LX, WV.FV_D))
        (K * _dev(w)).sum().backward()
        return K.detach().cpu().numpy(), Xg.grad.reshape(X.shape).cpu().numpy()

    (K, grad), names = L.traced(call)
    want_K, want_g = WV.fv_yardstick(case, X, Y, w)
    errs = {"value": V.value_error(K, want_K)}
    if cls == "rbf_id":
        errs["grad"] = V.grad_error(grad, want_g)
    bad = []
    for name in WV.fv_outputs(case):
        tol = V.BASE_TOL[name] + 4.0 * RECORDED[WV.fv_key(case, name)]
        _report("fv   %-8s %-7s %-10s %-5s %.2e  bound %.2e" % (cls, fam, lab, name, errs[name], tol))
        if not errs[name] <= tol:
            bad.append("%s: %.3e > %.3e" % (name, errs[name], tol))
    assert any(CLAIM in n for n in names), sorted(names)
    assert not bad, "; ".join(bad)
