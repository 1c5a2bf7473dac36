"""The upstream-gradient families on the GPU (tests/upstream_gradients.py): every gradient route with one-hot, zero, rescaled, non-finite,
misaligned and non-contiguous upstream gradients, against per-pair reference gradients contracted with the same weight.  Each case runs
under the launch trace and asserts that the row's kernel family was launched; a recording wrapper on the back-end's adjoint entry
points notes the address of every weight a launch received.

With SK_UPSTREAM_GRADIENTS_REPORT=<file> every case appends one line to that file -- the worst of its bounded comparisons with its bound,
the number of its exact ones -- and the address family the entry points that received a misaligned weight
(profiles/upstream_gradients.txt)."""
import inspect
import os

import pytest
import torch

import sigkernel_amd
from sigkernel_amd import _lib
import instance_ledger as L
import upstream_gradients as U
from poison import same_bits
from test_upstream_gradients_host import make_call, make_kernel, reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = U.cases()
WEIGHT_ARGS = ("scale", "weight", "w")


def _report(line):
    print(line)
    path = os.environ.get("SK_UPSTREAM_GRADIENTS_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _case_line(row, fam, seen, ppg):
    """one line per case: the worst of its bounded comparisons (error, bound) and the number of its exact ones (bit equalities, exact zeros)"""
    bounded = [(e, t, w) for w, e, t in seen if t > 0]
    exact = [e for w, e, t in seen if t == 0]
    line = "%-62s %-10s" % (row["id"], fam)
    if bounded:
        e, t, w = max(bounded, key=lambda c: c[0] / c[1])
        line += " %2d bounded, worst %.2e  bound %.2e (%s)" % (len(bounded), e, t, w)
    if exact:
        line += " %2d exact%s" % (len(exact), "" if not any(exact) else ", %d BROKEN" % sum(1 for e in exact if e))
    return line + ("  ppg %d" % ppg if ppg else "")


def _short(names):
    return sorted(n.split("_GLOBAL__N_1")[-1][:48] for n in names)


@pytest.fixture
def recorder(monkeypatch):
    """[(entry point, data_ptr() % 16 of the weight it received, or of `gscale` as "entry:gscale")] of every adjoint launch of the test"""
    be = _lib.get_backend()
    seen = []
    for name in U.ADJOINT_ENTRIES:
        raw = inspect.getattr_static(type(be), name)
        static = isinstance(raw, staticmethod)
        fn = raw.__func__ if static else raw
        sig = inspect.signature(fn)

        def wrapped(*a, _fn=fn, _sig=sig, _name=name, **kw):
            bound = _sig.bind(*a, **kw).arguments
            for arg in WEIGHT_ARGS:
                if torch.is_tensor(bound.get(arg)):
                    seen.append((_name, bound[arg].data_ptr() % 16))
            if torch.is_tensor(bound.get("gscale")):
                seen.append((_name + ":gscale", bound["gscale"].data_ptr() % 16))
            return _fn(*a, **kw)
        monkeypatch.setattr(type(be), name, staticmethod(wrapped) if static else wrapped)
    return seen


def _expects_an_odd_weight(row):
    """the rows whose adjoint entry point receives a view of the caller's gradient: the fused Gram and paired rows.  (The swapped route
    hands its kernel no weight and folds a transposed copy afterwards; the loss rows form wb * grad_output, or pass the scalar as gscale.)"""
    return row["fused"] and row["op"] in ("gram", "paired", "sym") and "swapped" not in row["name"]


@pytest.mark.parametrize("row, fam", CASES, ids=["%s-%s" % (r["id"], f) for r, f in CASES])
def test_family_on_the_gpu(row, fam, recorder, monkeypatch):
    be = _lib.get_backend()
    dtype = torch.float32 if row["f32"] else torch.float64
    call = make_call(row, DEV, dtype, monkeypatch)
    ref = lambda s: reference(row["id"], s)      # noqa: E731
    _, _, w0 = U.inputs(row)
    be.last_fused_ppg = None
    _, names = L.traced(lambda: call(w0))
    ppg = be.last_fused_ppg if row["fused"] and row["op"] in ("gram", "paired") else None
    entries_before = len(recorder)

    seen = []
    bad = U.run_family(row, fam, ref, call, DEV, report=lambda what, err, tol: seen.append((what, err, tol)), ppg=ppg)
    _report(_case_line(row, fam, seen, ppg))
    missing = [c for c in row["claims"] if not any(c in n for n in names)]
    assert not missing, "%s no longer launches %s (launched: %s)" % (row["id"], missing, _short(names))
    if row["ppg"]:
        assert ppg is not None and ppg > 1, "%s: one pair per lane-group chunk (last_fused_ppg = %r)" % (row["id"], ppg)
    if row["api"] == "trunc":
        assert any(n == row["entry"] for n, _ in recorder), "%s: %s was not called (%s)" % (row["id"], row["entry"], sorted(set(n for n, _ in recorder)))
    if fam == "address":
        odd = sorted(set(n for n, r in recorder[entries_before:] if r != 0))
        _report("%-62s %-10s weights off a 16-byte boundary reached: %s" % (row["id"], fam, ", ".join(odd) or "no entry point"))
        if _expects_an_odd_weight(row) or row["name"] == "one-launch loss" or row["route"] == "merged loss launch":
            assert odd, "%s: no adjoint launch received a weight with data_ptr() %% 16 != 0 (%s)" % (row["id"], recorder[entries_before:])
    assert not bad, "%s, %s: %s" % (row["id"], fam, "; ".join(bad))


@pytest.mark.parametrize("kind", ["linear", "rbf"])
def test_one_row_tiles_hand_the_kernels_both_parities(kind, recorder):
    """workspace_bytes small enough for one-row tiles of a 4 x 5 Gram block: the tile of row a0 starts at element 5 a0 of the upstream
    gradient, so the fused adjoint receives 16-byte-aligned and misaligned weights in turn; the gradient is the untiled call's."""
    row = U.ROW_BY_ID["F1/A1-3x3_20x17_D3_d1-%s" % kind]
    gen = torch.Generator().manual_seed(23)
    from conftest import walk
    X, Y = walk(gen, 4, 20, 3), walk(gen, 5, 17, 3)
    w = torch.randn(4, 5, generator=gen, dtype=torch.float64)
    k = make_kernel(row)
    from oracle import oracle as O
    want = O.gram_grad_weighted(X, Y, w.numpy(), k, 1)
    name = "%s_adjoint_fused" % kind
    got = {}
    for ws in (None, 60000):      # one row's edges and partial sums: 64 B + 2048 M = 41280 bytes
        del recorder[:]
        Xg = X.to(DEV).requires_grad_(True)
        sigkernel_amd.SigKernel(k, 1, workspace_bytes=ws).compute_Gram(Xg, Y.to(DEV)).backward(gradient=w.to(DEV))
        got[ws] = Xg.grad
        calls = [r for n, r in recorder if n == name]
        ok, idx, err = U.compare_grads(Xg.grad.cpu().numpy(), want, U.GRAD_TOL)
        _report("%-62s %-10s workspace_bytes %-61s %.2e  bound %.2e" % ("one-row tiles 4x5_20x17_D3_d1-" + kind, "address", ws, err, U.GRAD_TOL))
        assert ok, (ws, idx, err)
        if ws is None:
            assert calls == [0], calls
        else:
            assert len(calls) == 4 and set(calls) == {0, 8}, calls
    ok, msg = same_bits(got[None], got[60000])
    assert ok, msg


DIRECT = [("linear", False), ("rbf", False), ("linear", True), ("rbf", True)]


@pytest.mark.parametrize("kind, mb", DIRECT, ids=["%s%s" % (k, "_mb" if m else "") for k, m in DIRECT])
def test_fused_sweeps_read_a_misaligned_weight_themselves(kind, mb):
    """Without forward values the rescue's screen does not copy the weights, and the sweep kernels read the caller's array: the one-band
    RBF kernel and the multi-band kernels fetch the aligned 16 bytes that hold scale[p] and pick the half by (pointer >> 3) ^ pair.  The
    back-end entry points on a weight at element offset 1 of a NaN-filled buffer against the aligned copy: the same bits."""
    be = _lib.get_backend()
    gen = torch.Generator().manual_seed(29)
    from conftest import walk
    A, B, M, N, D, d = (2, 3, 150, 140, 3, 1) if mb else (3, 5, 20, 17, 3, 1)
    X, Y = walk(gen, A, M, D).to(DEV), walk(gen, B, N, D).to(DEV)
    w = torch.randn(A * B, generator=gen, dtype=torch.float64)
    code, param = (0, 1.0) if kind == "linear" else (1, U.SIGMA)
    if mb:
        fw = be.solve_fwd_fused_static(code, param, X, Y, d, False, True, keep_edges=True)
        adj = be.linear_adjoint_fused_mb if kind == "linear" else be.rbf_adjoint_fused_mb
    else:
        fw = (be.solve_fwd_fused_linear if kind == "linear" else be.solve_fwd_fused_rbf)(X, Y, param, d, False, True, keep_edges=True)
        adj = be.linear_adjoint_fused if kind == "linear" else be.rbf_adjoint_fused
    assert fw is not None and fw[1] is not None
    view, buf, guard = U.offset_view(w.numpy(), 1, torch.float64, DEV)
    assert view.data_ptr() % 16 == 8
    res, names = L.traced(lambda: (adj(X, Y, param, d, fw[1], w.to(DEV), gram=True, kfinal=None), adj(X, Y, param, d, fw[1], view, gram=True, kfinal=None)))
    assert res[0] is not None and res[1] is not None
    assert any(("k_adj_fused_%s%sI" % (kind, "_mb" if mb else "")) in n for n in names), _short(names)
    assert not any("k_screen" in n for n in names), _short(names)
    ok, msg = same_bits(res[0][0], res[1][0])
    _report("%-62s %-10s %-72s %.2e  bound %.2e" % ("back-end %s_adjoint_fused%s" % (kind, "_mb" if mb else ""), "address",
                                                     "scale at element offset 1, no forward values", 0.0 if ok else float("inf"), 0.0))
    assert ok, msg
    assert U.guards_intact(buf, guard)
    # no rescue armed: the host delivers a NaN weight that the sweep drops -- the NaN on every element of the pair's path, the bits of
    # the finite call on the others
    wn = w.clone()
    wn[1 * B + 2] = U.NAN
    gn = adj(X, Y, param, d, fw[1], wn.to(DEV), gram=True, kfinal=None)[0]
    assert bool(torch.isnan(gn[1]).all()), "a NaN weight without the rescue: %d of %d elements of the path are NaN" % (int(torch.isnan(gn[1]).sum()), gn[1].numel())
    keep = [a for a in range(A) if a != 1]
    ok, msg = same_bits(res[0][0][keep], gn[keep])
    assert ok, msg
    from oracle import oracle as O
    want = O.gram_grad_weighted(X.cpu(), Y.cpu(), w.view(A, B).numpy(), make_kernel({"kind": kind, "wild": False}), d)
    ok, idx, err = U.compare_grads(res[1][0].cpu().numpy(), want, U.GRAD_TOL)
    assert ok, (idx, err)
