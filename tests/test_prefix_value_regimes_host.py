"""The prefix / ragged value-regime table without a GPU (tests/prefix_value_regimes.py): the coverage of the table, the certificate of
its gradient yardstick, tests/golden/prefix_value_regimes.json recomputed, and the whole table -- with the slice / ragged bit-equalities
and the padding claims of the GPU test -- through the API on the oracle-backed back-end (RaggedExactBackend of
tests/test_ragged_gradient_host.py: the streamed route, the restated exact adjoint on every pair's sub-block).  That back-end IS the
reference's arithmetic, so here every case gets base + 4 r: the invariance on offsets is a claim about the HIP kernels.

The functions that make the calls (`run_case`, `check_slices_and_ragged`, `padding_forward`, `padding_gradient`) take the device and are
the GPU test's as well."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import prefix_value_regimes as PV
import value_regimes as V
from conftest import GOLDEN, walk

with open(os.path.join(GOLDEN, "prefix_value_regimes.json")) as _f:
    RECORDED = json.load(_f)
KD = [("linear", 0), ("rbf", 0), ("linear", 1), ("rbf", 1), ("linear", 2), ("rbf", 2)]


# ------------------------------------------------------------------------------------------------------------------- the calls (host and GPU)
def _kernel(kind, sigma):
    import sigkernel_amd
    return sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(sigma)


def _tensors(c, device):
    X, Y, w, sigma = PV.case_inputs(c)
    # (fp32 rows on the CPU: the oracle-backed back-end would run the static stage in fp32; the kernel stages fp32 paths as fp64 and
    # rounds its stores -- so the fp32-rounded inputs go in as fp64 and the host test rounds the values)
    dt = torch.float32 if c[0]["shape"]["f32"] and str(device) != "cpu" else torch.float64
    return tuple(torch.from_numpy(np.array(a)).to(dt).to(device) for a in (X, Y, w)) + (sigma,)


def run_case(c, device):
    """the row's call through the API -> ({output: tensor}, the SigKernel, X, Y on the device)"""
    import sigkernel_amd
    from sigkernel_amd import _lib
    row, kind, fam, lab, st = c
    Xd, Yd, wd, sigma = _tensors(c, device)
    op, d, gram = row["op"], row["shape"]["d"], row["gram"]
    sk = sigkernel_amd.SigKernel(_kernel(kind, sigma), d, exact_gradient=op in PV.GRAD_OPS)
    if op == "grid":
        out = {"value": sk.compute_Gram_prefixes(Xd, Yd) if gram else sk.compute_kernel_prefixes(Xd, Yd)}
    elif op == "grid_out":
        be = _lib.get_backend()
        if not hasattr(be, "solve_prefix_fused"):      # (the oracle-backed back-end has no fused sweep to hand a view to)
            out = {"value": sk.compute_Gram_prefixes(Xd, Yd)}
        else:
            A, B, M, N = Xd.shape[0], Yd.shape[0], Xd.shape[1], Yd.shape[1]
            buf = torch.empty(A * B * M * N + 1, dtype=Xd.dtype, device=device)
            view = buf[1:].view(A, B, M, N)
            assert buf.data_ptr() % (2 * Xd.element_size()) == 0 and view.data_ptr() % (2 * Xd.element_size()) == Xd.element_size()
            got = be.solve_prefix_fused(0 if kind == "linear" else 1, 1.0 if kind == "linear" else sigma, Xd, Yd, d, False, True, out=view)
            assert got is not None and got.data_ptr() == view.data_ptr()
            out = {"value": got}
    elif op == "mmd_prefixes":
        out = {"value": sk.compute_mmd_prefixes(Xd, Yd)}
    elif op == "mmd_ragged":
        lx, ly = PV.lens_of(row)
        out = {"value": sk.compute_mmd_ragged(Xd, lx, Yd, ly)}
    else:
        lx, ly = PV.lens_of(row)
        Xg, Yg = Xd.clone().requires_grad_(True), Yd.clone().requires_grad_(True)
        if op == "gram_ragged_grad":
            v = sk.compute_Gram_ragged(Xg, Yg, lx, ly)
        elif op == "kernel_ragged_grad":
            v = sk.compute_kernel_ragged(Xg, Yg, lx, ly)
        else:
            v = sk.compute_mmd_ragged(Xg, lx, Yg, ly)
        (v * wd).sum().backward()
        out = {"value": v.detach(), "grad_x": Xg.grad, "grad_y": Yg.grad}
    return out, sk, Xd, Yd


def check_slices_and_ragged(c, sk, Xd, Yd, grid):
    """the three slices and the ragged node against the grid the case has just compared, bit for bit (one call each).  The ragged call
    runs on nine paths per side -- the row's, repeated -- with every length ragged_lens aims at; a one-point path gives exactly 1.
    -> the calls' results, for the caller's trace"""
    row = c[0]
    gram = row["gram"]
    f = sk.compute_Gram_prefixes if gram else sk.compute_kernel_prefixes
    for nodes in ("diagonal", "last_row", "last_col"):
        got = f(Xd, Yd, nodes=nodes)
        want = torch.diagonal(grid, dim1=-2, dim2=-1) if nodes == "diagonal" else (grid[..., -1, :] if nodes == "last_row" else grid[..., :, -1])
        assert torch.equal(got, want), "%s is not the grid's slice bit for bit" % nodes
    ix, iy, lx, ly = PV.ragged_case(row["shape"], gram)
    tx, ty = torch.tensor(ix, device=grid.device), torch.tensor(iy, device=grid.device)
    ax, ay = torch.tensor(lx, device=grid.device) - 1, torch.tensor(ly, device=grid.device) - 1
    X9, Y9 = Xd[tx].contiguous(), Yd[ty if gram else tx].contiguous()
    if gram:
        K = sk.compute_Gram_ragged(X9, Y9, lx, ly)
        want = grid[tx[:, None], ty[None, :], ax[:, None], ay[None, :]]
        ones = (ax == 0)[:, None] | (ay == 0)[None, :]
    else:
        K = sk.compute_kernel_ragged(X9, Y9, lx, ly)
        want = grid[tx, ax, ay]
        ones = (ax == 0) | (ay == 0)
    assert torch.equal(K, want), "the ragged node is not the grid's node bit for bit"
    assert bool((K[ones] == 1).all()) and int(ones.sum()) >= 1
    return K


def assert_padding_is_zero(grad, lens):
    for i, n in enumerate(lens):
        assert bool((grad[i, n:] == 0.0).all()), (i, n, grad[i, n:])


def _true_points_equal(g, g0, lens):
    return all(torch.equal(g[i, :n], g0[i, :n]) for i, n in enumerate(lens))


def _padding_paths(A, B, M, N, D, f32, seed):
    gen = torch.Generator().manual_seed(seed)
    return walk(gen, A, M, D).numpy(), walk(gen, B, N, D).numpy()


def padding_forward(kind, d, D, gram, f32, device, M=20, N=17):
    """compute_Gram_ragged / compute_kernel_ragged on nine true paths per side under every padding variant: bit-identical values"""
    import sigkernel_amd
    n = PV.RAGGED_COUNT
    X, Y = _padding_paths(n, n, M, N, D, f32, 100 * d + D)
    lx, ly = PV.ragged_lens(M, n, M), PV.ragged_lens(N + 1, n, N)
    assert sum(v < M for v in lx) >= 6 and sum(v < N for v in ly) >= 6
    sk = sigkernel_amd.SigKernel(_kernel(kind, 1.0), d)
    dt = torch.float32 if f32 else torch.float64
    results = {}
    for variant in PV.PADDINGS:
        Xd, Yd = (torch.from_numpy(PV.padded(P, ln, variant, f32)).to(dt).to(device) for P, ln in ((X, lx), (Y, ly)))
        results[variant] = sk.compute_Gram_ragged(Xd, Yd, lx, ly) if gram else sk.compute_kernel_ragged(Xd, Yd, lx, ly)
    base = results["repeat"]
    assert bool(torch.isfinite(base).all())
    bad = [v for v in PV.PADDINGS if not torch.equal(results[v], base)]
    assert not bad, "the padding reaches the values under %s" % bad
    return base


def padding_gradient(kind, D, gram, f32, device, M=20, N=17, d=1):
    """the ragged exact gradient under every padding variant: values and the gradients of the true points bit-identical to those of the
    repeated last point, exactly 0.0 on every padded point.  -> (dL/dX, dL/dY) of the repeated-point call"""
    import sigkernel_amd
    X, Y = _padding_paths(3, 3, M, N, D, f32, 7 + D)
    lx, ly = PV.grad_lens(M, N)
    sk = sigkernel_amd.SigKernel(_kernel(kind, 1.0), d, exact_gradient=True)
    dt = torch.float32 if f32 else torch.float64
    gen = torch.Generator().manual_seed(11)
    w = torch.randn((3, 3) if gram else (3,), generator=gen, dtype=torch.float64).to(dt).to(device)
    res = {}
    for variant in PV.PADDINGS:
        Xg, Yg = (torch.from_numpy(PV.padded(P, ln, variant, f32)).to(dt).to(device).requires_grad_(True) for P, ln in ((X, lx), (Y, ly)))
        v = sk.compute_Gram_ragged(Xg, Yg, lx, ly) if gram else sk.compute_kernel_ragged(Xg, Yg, lx, ly)
        (v * w).sum().backward()
        res[variant] = (v.detach(), Xg.grad, Yg.grad)
    v0, gx0, gy0 = res["repeat"]
    assert bool(torch.isfinite(gx0).all()) and bool(torch.isfinite(gy0).all())
    assert float(gx0.abs().max()) > 0 and float(gy0.abs().max()) > 0
    bad = []
    for variant in PV.PADDINGS:
        v, gx, gy = res[variant]
        if not torch.equal(v, v0):
            bad.append("%s: values" % variant)
        for name, g, g0, lens in (("X", gx, gx0, lx), ("Y", gy, gy0, ly)):
            zero = all(bool((g[i, n:] == 0.0).all()) for i, n in enumerate(lens))
            if not zero:
                bad.append("%s: %d non-zero or non-finite entries on the padding of %s" % (variant, int(sum((g[i, n:] != 0.0).sum() for i, n in enumerate(lens))), name))
            if not _true_points_equal(g, g0, lens):
                bad.append("%s: true points of %s.grad" % (variant, name))
    assert not bad, "; ".join(bad)
    return gx0, gy0


PAD_FORWARD = [(kind, d, 3, gram, False) for kind, d in KD for gram in (True, False)] + \
              [("linear", 1, 12, True, False), ("rbf", 1, 12, False, False), ("rbf", 1, 3, True, True), ("linear", 0, 3, False, True)]
PAD_GRADIENT = [(kind, D, gram, False) for D in (3, 12, 40) for kind in V.KINDS for gram in (True, False)] + [("rbf", 3, True, True)]


def pad_id(t):
    return "-".join(str(v) for v in t)


# ------------------------------------------------------------------------------------------------------------------- the table
def _rows(**want):
    return [r for r in PV.ROWS if all(r[k] == v for k, v in want.items())]


def test_the_table_holds_every_item():
    grids = _rows(op="grid")
    fused = [r for r in grids if r["fused"] and not r["shape"]["f32"]]
    # the four instances, each at a few lanes (>= 2 lane groups) and at all 64; the launcher's rules say so for the row's shape
    for kind, d in KD:
        mine = [r for r in fused if kind in r["kinds"] and r["shape"]["d"] == d and r["gram"]]
        lanes = {PV.lanes_of(kind, d, r["shape"]["M"]) for r in mine}
        assert 64 in lanes and min(lanes) <= 32, (kind, d, lanes)
        for r in mine:
            assert PV.is_fused(kind, d, r["shape"]["M"], r["shape"]["D"])
            assert r["lanes"] is None or r["lanes"] == PV.lanes_of(kind, d, r["shape"]["M"]), r["name"]
    sh = {(k, d): [r["shape"] for r in fused if k in r["kinds"] and r["shape"]["d"] == d and PV.lanes_of(k, d, r["shape"]["M"]) == 64] for k, d in KD}
    assert any(s["M"] - 1 > 128 for s in sh[("linear", 0)]) and any(64 < s["M"] <= 128 for s in sh[("rbf", 0)])
    assert all(PV.rows_per_lane(k, 1) == 2 for k in V.KINDS) and sh[("linear", 1)] and sh[("rbf", 1)]
    assert any(32 < s["M"] - 1 <= 64 for s in sh[("linear", 2)]) and any(32 < s["M"] <= 64 for s in sh[("rbf", 2)])
    for r in PV.ROWS:
        if r["scheme"] is not None:
            assert r["scheme"] == PV.store_scheme(r["shape"]["M"], r["shape"]["N"], odd_view=r["op"] == "grid_out"), r["name"]
    for kind in V.KINDS:
        mine = [r for r in PV.ROWS if kind in r["kinds"] and r["fused"] and r["op"] in ("grid", "grid_out")]
        assert {r["scheme"] for r in mine} >= {2, 3}
        assert any(r["scheme"] == 2 and r["shape"]["N"] % 2 for r in mine) and any(r["op"] == "grid_out" and r["shape"]["N"] % 2 == 0 for r in mine)
        assert {r["shape"]["D"] for r in mine} >= {1, 3, 8}
        assert any(r["gram"] and (r["shape"]["A"], r["shape"]["B"]) == (3, 3) for r in mine) and any(not r["gram"] for r in mine)
        f32 = [r for r in mine if r["shape"]["f32"]]
        assert f32 and all(r["families"] == PV.F32_FAMILIES for r in f32) and {r["scheme"] for r in f32} == {2, 3}
        streamed = [r for r in grids if kind in r["kinds"] and not r["fused"]]
        assert any(r["shape"]["D"] == 12 for r in streamed)
        for op in ("mmd_prefixes", "mmd_ragged"):
            assert [r for r in _rows(op=op) if kind in r["kinds"] and r["families"] == PV.MMD_FAMILIES]
        for op in ("gram_ragged_grad", "kernel_ragged_grad"):
            assert {r["shape"]["D"] for r in _rows(op=op) if kind in r["kinds"]} == {3, 12, 40}
        assert {r["shape"]["D"] for r in _rows(op="mmd_ragged_grad") if kind in r["kinds"]} == {3, 12, 40}
    # one row just past a one-band limit (and within the staged dims): streamed
    past = [r for r in grids if not r["fused"] and r["shape"]["D"] <= PV.MAX_FUSED_D]
    assert past and all(r["shape"]["M"] == PV.LARGEST[(k, r["shape"]["d"])] + 1 for r in past for k in r["kinds"])
    # (3 x 3 pairs: no lane-group count divides 9)
    assert all(9 % g for g in (2, 4, 8))
    # LinearKernel's s = 10 only where a row names it
    wild = {c[0]["name"] for c in PV.CASES if c[4].get("wild")}
    assert wild == {r["name"] for r in PV.ROWS if r["wild"]} and len(wild) >= 1
    # the ragged launch of a grid row meets every aimed length
    for r in grids:
        ix, iy, lx, ly = PV.ragged_case(r["shape"], r["gram"])
        for lens, top in ((lx, r["shape"]["M"]), (ly, r["shape"]["N"])):
            assert {1, 2, top, 3, top - 1, 4, top - 2, 5, top - 3} == set(lens)
    assert 300 <= len(PV.CASES) <= 420, len(PV.CASES)


def test_offset_bounds():
    """base alone on offset: the values of the fused rows (either kernel), LinearKernel's gradients; everything else base + 4 r"""
    for c in PV.CASES:
        for name in PV.outputs_of(c[0]):
            base = V.BASE_TOL["value" if name == "value" else "grad"] + (2.0 ** -22 if c[0]["shape"]["f32"] else 0.0)
            tol = PV.tolerance(c, name, RECORDED)
            if c[2] == "offset" and ((name == "value" and c[0]["fused"]) or (name != "value" and c[1] == "linear")):
                assert tol == base
            else:
                assert tol == base + 4.0 * RECORDED[PV.golden_key(c)][name]


def test_recorded_entries_are_the_case_table():
    assert set(RECORDED) - {"_provenance"} == set(PV.golden_entries())


def _measure_module():
    spec = importlib.util.spec_from_file_location("measure_prefix_value_regimes", os.path.join(GOLDEN, "measure_prefix_value_regimes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MEASURE = _measure_module()
ENTRIES = PV.golden_entries()


@pytest.mark.parametrize("key", sorted(ENTRIES))
def test_recorded_reference_distance_reproduces(key):
    """prefix_value_regimes.json holds what the committed script measures here, within a factor 2 (the rounding of the restatements moves
    with the libm and the BLAS underneath them, not by more)"""
    got, rec = MEASURE.measure(ENTRIES[key]), RECORDED[key]
    print(key, got, rec)
    assert set(got) == set(rec)
    for name in got:
        floor = 1e-15
        assert got[name] <= 2 * rec[name] + floor and rec[name] <= 2 * got[name] + floor, (name, got, rec)


CERTIFIED = [("compute_Gram_ragged gradients D=3", "rbf", "sigma", "sigma=100"), ("compute_kernel_ragged gradients D=12", "linear", "scale", "s=3"),
             ("compute_mmd_ragged gradients D=3", "rbf", "drift", "s=5")]


@pytest.mark.parametrize("name, kind, fam, lab", CERTIFIED, ids=["-".join(t[1:]) for t in CERTIFIED])
def test_gradient_yardstick_against_a_central_difference(name, kind, fam, lab):
    """the ragged gradient yardstick (truncated paths, exact_weights_ld, _chain_ld for both arguments, the weights, zeros on the
    padding) against a central difference of the long-double VALUE along a random direction of every point of both batches: 1e-9 of
    sum |gradient x direction|.  With h = 1e-6 of the largest step the difference's truncation is h^2 f''' / 6 -- 1e-12 times the ratio
    of third to first derivative in units of the step, some tens at dyadic order 1 -- and its rounding 2^-64 |L| / h, below 1e-12."""
    c = next(c for c in PV.CASES if c[0]["name"] == name and c[1:4] == (kind, fam, lab))
    err = PV.fd_certificate(c)
    print(name, kind, fam, lab, err)
    assert err <= 1e-9, err
    want = PV.case_want(c)
    lx, ly = PV.lens_of(c[0])
    for g, lens in ((want["grad_x"], lx), (want["grad_y"], ly)):
        assert all(np.all(g[i, n:] == 0) for i, n in enumerate(lens)) and float(np.abs(g).max()) > 0


def test_ragged_lens_reach_every_aimed_row():
    lens = PV.ragged_lens(3, 9, 20)
    assert sorted(lens) == [1, 2, 3, 4, 5, 17, 18, 19, 20]
    assert sorted(PV.ragged_lens(3, 2, 20)) == [2, 20]


def test_padding_variants():
    P = np.arange(2 * 5 * 2, dtype=np.float64).reshape(2, 5, 2)
    for variant in PV.PADDINGS:
        for f32 in (False, True):
            Q = PV.padded(P, [2, 5], variant, f32)
            assert np.array_equal(Q[0, :2], P[0, :2]) and np.array_equal(Q[1], P[1])
            tail = Q[0, 2:]
            if variant == "repeat":
                assert np.all(tail == P[0, 1])
            elif variant == "walk":
                assert np.array_equal(tail, P[0, 2:])
            elif variant == "nan+inf":
                assert int(np.isnan(tail).sum()) == 1 and int(np.isposinf(tail).sum()) == 1
            else:
                assert np.all(np.isfinite(tail)) and not np.array_equal(tail, P[0, 2:])
            if variant == "+-1.5e308":
                with np.errstate(over="ignore"):
                    assert tail[0, 0] == -tail[1, 0] and not np.isfinite(np.float32(tail[0, 0]) - np.float32(tail[1, 0]) if f32 else tail[0, 0] - tail[1, 0])
            if variant == "1e200":
                with np.errstate(over="ignore"):
                    sq = np.float32(tail[0, 0]) ** 2 if f32 else tail[0, 0] ** 2
                assert np.isinf(sq)


# ------------------------------------------------------------------------------------------------------------------- through the API
@pytest.fixture
def backend():
    from sigkernel_amd import _lib
    from test_ragged_gradient_host import RaggedExactBackend
    prev = _lib.set_backend(RaggedExactBackend())
    yield
    _lib.set_backend(prev)


@pytest.mark.parametrize("case", PV.CASES, ids=[PV.case_id(c) for c in PV.CASES])
def test_table_through_the_api_on_the_oracle_backend(backend, case):
    out, sk, Xd, Yd = run_case(case, "cpu")
    want = PV.case_want(case)
    bad = []
    for name in PV.outputs_of(case[0]):
        got = out[name].detach().float() if case[0]["shape"]["f32"] else out[name].detach()
        err = PV.error(name, got.double().numpy(), want[name])
        tol = PV.tolerance(case, name, RECORDED, assume_invariant=False)
        if not err <= tol:
            bad.append("%s: %.3e > %.3e" % (name, err, tol))
    assert not bad, "; ".join(bad)
    if case[0]["op"] == "grid":
        check_slices_and_ragged(case, sk, Xd, Yd, out["value"])
    if case[0]["op"] in PV.GRAD_OPS:
        lx, ly = PV.lens_of(case[0])
        assert_padding_is_zero(out["grad_x"], lx)
        assert_padding_is_zero(out["grad_y"], ly)


@pytest.mark.parametrize("kind, d, D, gram, f32", PAD_FORWARD, ids=[pad_id(t) for t in PAD_FORWARD])
def test_padding_never_reaches_a_value(backend, kind, d, D, gram, f32):
    padding_forward(kind, d, D, gram, f32, "cpu")


@pytest.mark.parametrize("kind, D, gram, f32", PAD_GRADIENT, ids=[pad_id(t) for t in PAD_GRADIENT])
def test_padding_never_reaches_a_gradient(backend, kind, D, gram, f32):
    """(the host test's small paths: the restated adjoint is a Python loop)"""
    padding_gradient(kind, D, gram, f32, "cpu", M=6, N=5)
