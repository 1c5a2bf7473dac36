"""The upstream-gradient families without a GPU (tests/upstream_gradients.py): every SigKernel row on the oracle-backed back-end -- the
expectations themselves, the host layer's own arithmetic on grad_output (the loss weights, the 2x rule, the tiling of go, the
symmetric fold) and the offset-view builder -- and the truncated rows on CPU tensors, where TruncatedSigKernel is its torch restatement.

fp32 rows run their fp32-rounded inputs in fp64 here: the oracle back-end hands fp32 increments from stage to stage, which the instance
ledger bounds separately (instance_ledger.F32_STAGE_SOURCE); the GPU half runs them in fp32."""
import functools

import numpy as np
import pytest
import torch

import sigkernel_amd
from sigkernel_amd import _lib
import instance_ledger as L
import upstream_gradients as U
from test_ragged_gradient_host import RaggedExactBackend
from fake_backend import OracleBackend

CASES = U.cases()


def test_the_bounds_are_the_ledgers():
    assert (U.F32_ULPS2, U.GRAD_TOL, U.RESCUE_GRAD_TOL) == (L.F32_ULPS2, L.TOL64["grad"], L.RESCUE_GRAD_TOL)
    assert U.WILD_PAIR == (2, 5)


def make_kernel(row):
    return sigkernel_amd.LinearKernel() if row["kind"] == "linear" else sigkernel_amd.RBFKernel(1.0 if row["wild"] else U.SIGMA)


def make_truncated(row, sigma, **more):
    kw = dict(row["knobs"])
    s = kw.pop("rbf", None)
    if s is not None:
        kw["static_kernel"] = sigkernel_amd.RBFKernel(s)
    kw.update(more)
    return sigkernel_amd.TruncatedSigKernel(U.TRUNC_L, sigma, 1, **kw)


@functools.lru_cache(maxsize=None)
def reference(row_id, sigma="base"):
    """the per-pair gradients of a row: computed once, shared by the families"""
    row = U.ROW_BY_ID[row_id]
    if row["api"] == "trunc":
        return U.trunc_reference(row, lambda s: make_truncated(row, s), sigma)
    return U.sig_reference(row, make_kernel(row), L._Paired(make_kernel(row)))


def as_tensor(w, dtype, device):
    return w if torch.is_tensor(w) else torch.as_tensor(np.array(w)).to(dtype).to(device)


def make_call(row, device, dtype, monkeypatch, workspace_bytes=None):
    """upstream_gradients.run_family's call for a row on `device`"""
    Xn, Yn, _ = U.inputs(row)
    for knob, v in row["knobs"].items():
        if row["api"] == "sig":
            monkeypatch.setattr(sigkernel_amd.routes, knob, v)
    sh = row["shape"]

    def call(w, X=None, Y=None, sigma="base", expanded=False):
        Xg = X if X is not None else torch.from_numpy(np.array(Xn)).to(dtype).to(device).requires_grad_(True)
        need_y = "dY" in row["outputs"]
        if row["sym"]:
            Yg = Xg
        elif Y is not None:
            Yg = Y
        else:
            Yg = torch.from_numpy(np.array(Yn)).to(dtype).to(device).requires_grad_(need_y)
        if row["api"] == "trunc":
            obj = make_truncated(row, torch.from_numpy(U.trunc_sigma(row, sigma)).to(device), workspace_bytes=workspace_bytes)
            K = obj.compute_kernel(Xg, Yg) if row["op"] == "paired" else obj.compute_Gram(Xg, Yg, sym=row["sym"])
        else:
            sk = sigkernel_amd.SigKernel(make_kernel(row), sh["d"], exact_gradient=row["op"] in ("exact", "ragged"), workspace_bytes=workspace_bytes)
            if row["op"] == "loss":
                v = sk.compute_mmd(Xg, Yg)
                if torch.is_tensor(w):      # (the address family: the factor itself is the view)
                    v.backward(gradient=w)
                else:
                    (v * float(w)).backward()
                return {"dX": Xg.grad}
            if row["op"] == "paired":
                K = sk.compute_kernel(Xg, Yg)
            elif row["op"] == "ragged":
                K = sk.compute_Gram_ragged(Xg, Yg, list(row["lens"][0]), list(row["lens"][1]))
            else:
                K = sk.compute_Gram(Xg, Yg, sym=row["sym"])
        if expanded:
            K.sum().backward()
        else:
            K.backward(gradient=as_tensor(w, K.dtype, device))
        out = {"dX": Xg.grad}
        if need_y:
            out["dY"] = Yg.grad
        return out
    return call


@pytest.fixture
def host_backend():
    prev = _lib.set_backend(OracleBackend())
    yield
    _lib.set_backend(prev)


@pytest.mark.parametrize("row, fam", CASES, ids=["%s-%s" % (r["id"], f) for r, f in CASES])
def test_family_on_the_host(row, fam, host_backend, monkeypatch):
    if row["op"] in ("exact", "ragged"):
        _lib.set_backend(RaggedExactBackend())
    call = make_call(row, "cpu", torch.float64, monkeypatch)
    bad = U.run_family(row, fam, lambda s: reference(row["id"], s), call, "cpu", dtype=torch.float64,
                       report=lambda what, err, tol: print("%-60s %-10s %-70s %.2e  bound %.2e" % (row["id"], fam, what, err, tol)))
    assert not bad, "%s, %s: %s" % (row["id"], fam, "; ".join(bad))


NONFINITE_ROWS = [r for r in U.ROWS if r["op"] != "loss"]


@pytest.mark.parametrize("row", NONFINITE_ROWS, ids=[r["id"] for r in NONFINITE_ROWS])
def test_the_nonfinite_mask_is_at_most_one_point(row):
    """The non-finite family skips the elements of a reached path where the pair's own reference gradient is exactly zero: at most one
    point's worth (D elements) per output on every row's inputs (ragged padding, which the family leaves out by name, apart)."""
    ref = reference(row["id"])
    D = row["shape"]["D"]
    for label, idx in U.positions(row):
        if label not in ("middle", "wild"):
            continue
        sizes = U.mask_size(ref, idx)
        if row["lens"] is not None:
            a, b = idx
            sizes = {"dX": sizes["dX"] - (row["shape"]["M"] - row["lens"][0][a]) * D, "dY": sizes["dY"] - (row["shape"]["N"] - row["lens"][1][b]) * D}
        print(row["id"], label, idx, sizes)
        assert all(0 <= n <= D for n in sizes.values()), (row["id"], label, sizes)


def test_the_issues_probe():
    """4 x 5 pairs of 9 x 8 points, dim 3, d = 1, LinearKernel and RBFKernel(0.8): no element of a pair's gradient is exactly zero"""
    from conftest import walk
    from oracle import oracle as O
    gen = torch.Generator().manual_seed(0)
    X, Y = walk(gen, 4, 9, 3), walk(gen, 5, 8, 3)
    for k in (sigkernel_amd.LinearKernel(), sigkernel_amd.RBFKernel(0.8)):
        assert np.all(O.gram_grad_points(X, Y, k, 1) != 0.0)


def test_offset_views_are_what_they_claim():
    vals = np.arange(12.0).reshape(3, 4)
    for dtype, size in ((torch.float64, 8), (torch.float32, 4)):
        for off in (1, 2, 3):
            v, buf, guard = U.offset_view(vals, off, dtype, "cpu")
            assert v.storage_offset() == off and v.is_contiguous() and v.data_ptr() == buf.data_ptr() + off * size
            assert (v.data_ptr() - buf.data_ptr()) % 16 == (off * size) % 16
            assert torch.equal(v, torch.as_tensor(vals).to(dtype)) and int(guard.sum()) == off + 5 and U.guards_intact(buf, guard)
            leaf = v.detach().requires_grad_()
            assert leaf.is_leaf and leaf.data_ptr() == v.data_ptr() and leaf.storage_offset() == off
            buf[0] = 0.0
            assert not U.guards_intact(buf, guard)


def test_every_grad_row_of_the_value_regimes_is_reused():
    import value_regimes as V
    want = {(r["name"], V.shape_key(sh), k) for r in V.ROUTES if "grad" in r["outputs"] for sh in r["shapes"] for k in r["kinds"]}
    got = {(r["route"], V.shape_key(r["shape"]), r["kind"]) for r in U.ROWS if r["route"]}
    assert got == want
