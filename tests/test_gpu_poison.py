"""No result may depend on unwritten memory: every kernel instance, every mode of the truncated kernel and the tiled solver routes run
three times on workspaces and outputs that held 0x00, 0xFF (NaN / -1) and 0x55 (1.2e103 / large positive) bytes when the library took
them from torch.empty (tests/poison.py), and every output has the same bits each time.  The kernels are unmasked -- padding rows and
columns are zeros somebody wrote, slabs and carries are read back by the block that wrote them -- so one unwritten padded double shows
here as a NaN (0 * NaN) or as a quietly different value, which a fresh test process on fresh memory never shows.

Bit equality is the derived bar, not a tolerance: csrc has no floating-point atomic add (its atomics are the integer work counters and
an atomicMax on the residual words, order-independent), so every output is a deterministic function of what the kernels read.  The
VALUES of the same calls are held to the oracle by test_gpu_instances.py and to the restatement by the test_gpu_truncated*.py modules;
this module adds that they hold whatever the buffers held.  Every first run's outputs must be finite, so equal NaNs cannot pass.

The audit (by reading, before any of this ran): the allocation sites of sigkernel_amd whose dtype is integer or uint8, and the float
buffers that carry integer words.  For each, what a kernel reads AS AN INTEGER and the line that initialises it on the launch stream
before the first read.  Only the sites on this table are poisoned with non-zero bytes; an integer / byte allocation anywhere else
raises poison.UnauditedIntegerSite (AUDITED below is the table's first column).

  site (sigkernel_amd/_lib.py)                     integer words a kernel reads                 initialised by
  _queue: int64[8]                                 word 0, the launch's work counter            sk_wave_fused.hip:906 and sk_wave_prefix.hip:661 (hipMemsetAsync on the
    (one-band forward, prefix, ragged, loss and      (atomicAdd; draws become pair indices)       launch stream) when the plan draws from it; otherwise the launcher drops
    symmetric launches)                                                                           the pointer (sk_wave_fused.hip:908, sk_wave_prefix.hip:660) and nothing reads it
  solve_fwd_fused_static: ws uint8                 the counter behind the per-wave rows;         sk_wave_fused_mb.hip:864 (counter); split mode: :853 (progress words and
                                                   split mode: progress words [P], counter,       counter in one memset) and :857 (status word); every other byte is a
                                                   status word (last 8 bytes)                     double the wave that reads it has written
  linear_adjoint_fused_mb / rbf_adjoint_fused_mb:  the counter behind the boundary rows          sk_wave_adj_fused_mb.hip:1221, or the pointer is dropped (:1220)
    ws uint8
  solve_deriv_fused: ws uint8                      the counter behind the per-wave rows          sk_wave_deriv_fused.hip:683, or the pointer is dropped (:682)
  _fused_rescue_args: rescue ws uint8              none: [P] doubles of screened upstream        sk_adj_fused_rescue.hip:30 (k_screen writes all P entries before the sweep);
                                                   gradients, then stored grids per block         rescue_pair writes inc, G, Kf, Kr of its block before adj_pair reads them
  solve_adj: ws uint8 (fast adjoint)               none: strip edges and a dummy K vector,       launch_fwd_wave writes the edges the adjoint sweep reads (sk_abi.hip:77-78)
                                                   doubles
  _grid_scratch: uint8 (stored grids, rescue)      none: solution grids in the increments'       the stored-grid kernels write a slot's grids before reading them
                                                   dtype
  loss_forward / solve_fwd_fused_sym: `buf`,       the pair table [P][2] int32 behind the        sk_loss.hip:50-51 (k_prep_cat writes all P entries in the staging launch);
    float64 with an int32 tail                     staged columns: (a, b) of pair p, which        the sweeps clamp p to [0, P) before the look-up (sk_wave_fused.hip:262, :326, :352)
                                                   index the staged rows and columns
  err: float64 [P] residual words                  read and written by atomicMax on their        torch.zeros (_lib.py fused adjoints without a rescue), k_screen
    (atomicMax through an unsigned view)           unsigned view -- a value, never an address     (sk_adj_fused_rescue.hip:31, rescue armed), sk_abi.hip:69 (sk_solve_adj_*)

No other integer word exists in a workspace: the truncated kernel's slabs, carries and Tpart are doubles read back by the block that
wrote them, the ragged lengths are inputs, and sigkernel.py / distributed.py allocate floating-point outputs only."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import instance_cases
import instance_ledger      # (also puts tools/ on the path: reach_sweep)
from poison import PATTERNS, assert_same_bits, poisoned
from test_gpu_truncated import GENERAL, ORDER1, expected_instance, traced
from test_gpu_truncated_adjoint import paths
from test_truncated_host import steps

pytestmark = pytest.mark.gpu

AUDITED = frozenset(("_lib", f) for f in ("_queue", "solve_fwd_fused_static", "linear_adjoint_fused_mb", "rbf_adjoint_fused_mb", "solve_deriv_fused",
                                          "_fused_rescue_args", "solve_adj", "_grid_scratch"))
NO_ALLOCATION = ()      # labels of ledger cases whose call takes nothing from torch.empty: none
SITES = []              # (what, {(module, function): interceptions}) of every three_runs' first run


def _finite(out, what):
    vals = out.values() if isinstance(out, dict) else out
    for v in vals:
        if v is not None:
            assert bool(torch.isfinite(v).all()), "%s: a non-finite output on zeroed workspaces" % (what,)


def three_runs(call, what, launches=None):
    """call() under each pattern: the launch trace of every run (when given), finite outputs on the first, equal bits on the others;
    -> interceptions per run; SITES collects them per (module, function) for the record"""
    first, counts = None, []
    for byte in PATTERNS:
        with poisoned(byte, AUDITED) as p:
            if launches is None:
                out = call()
            else:
                out, hit = traced(call)
                assert hit == launches, "%s under 0x%02X: launches %s, expected %s" % (what, byte, hit, launches)
        torch.cuda.synchronize()
        counts.append(p.count)
        if first is None:
            first = out
            SITES.append((what, dict(p.sites)))
            _finite(first, what)
        else:
            assert_same_bits(first, out, "%s under 0x%02X against 0x00" % (what, byte))
    assert counts[0] == counts[1] == counts[2], (what, counts)
    return counts[0]


# ---- (a) every kernel instance of the build: the ledger's 426 calls ---------------------------------------------------------------------

@pytest.mark.parametrize("case", instance_cases.CASES, ids=[c["label"].replace(" ", "_") for c in instance_cases.CASES])
def test_every_instance_returns_the_same_bits_whatever_its_workspaces_held(case):
    import reach_sweep
    t = {k: v.cuda() for k, v in reach_sweep.inputs(case).items()}
    n = three_runs(lambda: reach_sweep.execute(case, t), case["label"])
    print("%s: %d allocations intercepted per run %s" % (case["label"], n, sorted(SITES[-1][1].items())))
    assert (n == 0) == (case["label"] in NO_ALLOCATION), "%s: %d allocations intercepted" % (case["label"], n)
    if case.get("free"):
        torch.cuda.empty_cache()


# ---- (b) the modes of k_trunc_sig ------------------------------------------------------------------------------------------------------
# Shapes are (A, B, M, N, D, L) in steps (points for the lifts).  Each has an odd row count, N no multiple of 16, D below the staging width
# (3 or 5 at width 8; 9 or 13 at width 16) and A no multiple of the lane groups per wave (a dead group): where a pad is read.

def _plan(name, n, A, B, M, N, D, L, paired, budget=1 << 30):
    from sigkernel_amd import _lib
    out = (ctypes.c_int64 * n)()
    assert getattr(_lib.load(), name)(A, B, M, N, D, L, int(paired), budget, ctypes.cast(out, ctypes.c_void_p)) == 0, name
    return tuple(out)


def _three_blocks(mode, A, B, M, N, D, L, paired=False):
    """a workspace of three blocks' slabs (+ 100 bytes) of an adjoint mode: the plan's bytes over its blocks at a large budget"""
    n_chunks, blocks, total = _plan("sk_truncated_%sadjoint_plan" % mode, 4, A, B, M, N, D, L, paired)[:3]
    assert blocks > 3 and total % blocks == 0, (blocks, total)
    ws = 3 * (total // blocks) + 100
    assert _plan("sk_truncated_%sadjoint_plan" % mode, 4, A, B, M, N, D, L, paired, ws)[1] == 3
    return ws


@functools.lru_cache(maxsize=None)
def _steps(A, B, M, N, D, dtype="float64"):
    rng = np.random.default_rng(9000 + 31 * M + 7 * N + D)
    dt = np.dtype(dtype).type
    return torch.as_tensor(steps(rng, A, M, D, dt)).cuda(), torch.as_tensor(steps(rng, B, N, D, dt)).cuda()


@functools.lru_cache(maxsize=None)
def _points(A, B, M, N, D, dtype="float64"):
    """paths of M and N POINTS"""
    rng = np.random.default_rng(9500 + 31 * M + 7 * N + D)
    dt = np.dtype(dtype).type
    return paths(rng, A, M - 1, D, dt).cuda(), paths(rng, B, N - 1, D, dt).cuda()


def _sigma(L, seed=3):
    return torch.as_tensor(np.random.default_rng(seed).uniform(0.5, 1.5, L + 1))


def forward_entry(mode, shape, order, dtype="float64"):
    """the four public forward calls on steps; paired modes: the pairs (X[p], Y'[p]) with as many second paths as first ones"""
    import sigkernel_amd
    A, B, M, N, D, L = shape
    paired = "paired" in mode
    X, Y = _steps(A, A if paired else B, M, N, D, dtype)
    sig = _sigma(L)
    call = {"gram": lambda: sigkernel_amd.truncated_sig_kernel(X, Y, L, sig, order),
            "paired": lambda: sigkernel_amd.truncated_sig_kernel_paired(X, Y, L, sig, order),
            "levels": lambda: sigkernel_amd.truncated_sig_kernel_levels(X, Y, L, order),
            "levels_paired": lambda: sigkernel_amd.truncated_sig_kernel_levels(X, Y, L, order, paired=True)}[mode]
    return (lambda: {"value": call()}), {expected_instance(L, order): 1}


def lift_entry(mode, shape, kernel, dtype="float64"):
    """TruncatedSigKernel with a static kernel, no gradient pending: the RBF lift is the kernel's points mode, the linear lift the plain
    kernel on the steps; "levels": the level terms of the points mode, by the backend's call"""
    import sigkernel_amd
    from sigkernel_amd import _lib
    A, B, M, N, D, L = shape
    X, Y = _points(A, A if mode == "paired" else B, M, N, D, dtype)
    static = sigkernel_amd.RBFKernel(0.7) if kernel == "rbf" else sigkernel_amd.LinearKernel()
    tk = sigkernel_amd.TruncatedSigKernel(L, _sigma(L).cuda(), 1, static_kernel=static)
    if mode == "levels":
        assert kernel == "rbf"
        return (lambda: {"value": _lib.get_backend().truncated_levels(X, Y, L, 1, kind=1, param=0.7)}), {GENERAL: 1}
    call = tk.compute_kernel if mode == "paired" else tk.compute_Gram
    return (lambda: {"value": call(X, Y)}), {(GENERAL if kernel == "rbf" else ORDER1): 1}


def long_entry(mode, shape, dtype="float64"):
    """the long mode in THIS orientation (no_swap) under a workspace of two blocks' slabs: a block carries several pairs through one slab"""
    from sigkernel_amd import _lib
    A, B, M, N, D, L = shape
    paired = mode == "paired"
    B = A if paired else B
    X, Y = _steps(A, B, M, N, D, dtype)
    positions, block, total = _plan("sk_truncated_long_plan", 3, A, B, M, N, D, L, paired)      # (a large budget: a block per position)
    n = min(2, positions - 1)              # two blocks; one where the batch has two pairs only
    assert n >= 1 and block > 0, (positions, block)
    assert _plan("sk_truncated_long_plan", 3, A, B, M, N, D, L, paired, n * block) == (n, block, n * block)
    weights = None if mode == "levels" else _sigma(L).tolist()
    return (lambda: {"value": _lib.get_backend().truncated_long(X, Y, L, weights, paired, n * block, no_swap=True)}), {GENERAL: 1}


def gradient_entry(route, call, shape, grads, workspace=None, dtype="float64"):
    """value and every gradient of (K * c).sum().backward() with a fixed random c, through TruncatedSigKernel on PATHS of M and N steps
    (points for the points-adjoint route).  call: gram / paired / sym / mmd."""
    import sigkernel_amd
    A, B, M, N, D, L = shape
    if call == "paired":
        B = A
    X, Y = _points(A, B, M, N, D, dtype) if route == "points" else _points(A, B, M + 1, N + 1, D, dtype)
    kw = {"plain": {}, "points": dict(static_kernel=sigkernel_amd.RBFKernel(0.7), points_adjoint=True), "long": dict(long_adjoint=True),
          "wide": dict(wide_adjoint=True)}[route]
    tk = sigkernel_amd.TruncatedSigKernel(L, _sigma(L).cuda(), 1, workspace_bytes=workspace, **kw)
    cshape = {"gram": (A, B), "paired": (A,), "sym": (A, A), "mmd": ()}[call]
    c = torch.as_tensor(np.random.default_rng(11).standard_normal(cshape)).cuda()

    def run():
        x, y = X.clone().requires_grad_("x" in grads), Y.clone().requires_grad_("y" in grads)
        K = {"gram": lambda: tk.compute_Gram(x, y), "paired": lambda: tk.compute_kernel(x, y), "sym": lambda: tk.compute_Gram(x, x, sym=True),
             "mmd": lambda: tk.compute_mmd(x, y)}[call]()
        (K * c.to(K.dtype)).sum().backward()
        return {"value": K.detach(), "dx": x.grad, "dy": y.grad}
    # forward launches + one adjoint launch per batch that needs a gradient; mmd: K_XX (sym), K_YY (forward only), K_XY
    sides = len(grads)
    fwd, adj = {"gram": (1, sides), "paired": (1, sides), "sym": (1, 1), "mmd": (3, 2)}[call]
    if route == "wide":
        launches = {ORDER1: fwd, GENERAL: adj}       # the levels launch every call takes at dims 9 .. 16, the wide-adjoint mode behind it
    else:
        launches = {(ORDER1 if route == "plain" else GENERAL): fwd + adj}
    return run, launches


def _table():
    T = []

    def add(label, make, *args, **kw):
        T.append(pytest.param(make, args, kw, id=label))
    for mode in ("gram", "levels", "paired", "levels_paired"):
        for shape, order in (((3, 2, 9, 6, 3, 4), 1), ((3, 2, 9, 6, 3, 4), 3), ((2, 3, 63, 33, 5, 8), 4), ((2049, 1, 70, 5, 2, 3), 1)):
            add("forward-%s-%dx%d-%dx%d-order%d" % ((mode,) + shape[:4] + (order,)), forward_entry, mode, shape, order)
    add("forward-gram-fp32", forward_entry, "gram", (3, 2, 9, 6, 3, 4), 1, "float32")
    for mode in ("gram", "paired", "levels"):
        add("points-%s" % mode, lift_entry, mode, (3, 2, 10, 7, 3, 4), "rbf")
    for mode in ("gram", "paired"):
        add("linear-lift-%s" % mode, lift_entry, mode, (3, 2, 10, 7, 3, 4), "linear")
    add("points-gram-fp32", lift_entry, "gram", (3, 2, 10, 7, 3, 4), "rbf", "float32")
    for shape in ((3, 2, 130, 257, 5, 3), (2, 2, 130, 129, 9, 3)):
        for mode in ("gram", "paired", "levels"):
            add("long-%s-D%d" % (mode, shape[4]), long_entry, mode, shape)
    add("long-gram-fp32", long_entry, "gram", (3, 2, 130, 257, 5, 3), "float32")
    small, big = (3, 2, 9, 6, 5, 4), (5, 37, 20, 33, 5, 6)
    for route, shapes in (("plain", (small, big)), ("points", (small, big, small[:5] + (1,)))):
        for shape in shapes:
            name = "%s-adjoint-%dx%d-L%d" % (route, shape[0], shape[1], shape[5])
            ws = (lambda s=shape, r=route: _three_blocks("points_" if r == "points" else "", *s)) if shape is big else None
            for grads in ("x", "y", "xy"):
                add("%s-gram-d%s" % (name, grads), gradient_entry, route, "gram", shape, grads, ws if grads != "y" else None)
            add(name + "-paired", gradient_entry, route, "paired", shape, "xy")
            add(name + "-sym", gradient_entry, route, "sym", shape, "x")
            add(name + "-mmd", gradient_entry, route, "mmd", shape, "x")
        add("%s-adjoint-fp32" % route, gradient_entry, route, "gram", small, "xy", None, "float32")
    lshape = (3, 2, 130, 257, 5, 3)
    two = lambda paired: (lambda: 2 * _plan("sk_truncated_long_adjoint_plan", 4, 3, 3 if paired else 2, 130, 257, 5, 3, paired)[3])
    add("long-adjoint-gram", gradient_entry, "long", "gram", lshape, "xy", two(False))
    add("long-adjoint-paired", gradient_entry, "long", "paired", lshape, "xy", two(True))
    add("long-adjoint-fp32", gradient_entry, "long", "gram", lshape, "x", two(False), "float32")
    wsmall, wbig = (3, 2, 9, 6, 9, 4), (5, 37, 20, 33, 13, 6)
    add("wide-adjoint-3x2-dxy", gradient_entry, "wide", "gram", wsmall, "xy")
    add("wide-adjoint-5x37-dx", gradient_entry, "wide", "gram", wbig, "x", lambda: _three_blocks("wide_", *wbig))
    add("wide-adjoint-5x37-dxy", gradient_entry, "wide", "gram", wbig, "xy", lambda: _three_blocks("wide_", *wbig))
    add("wide-adjoint-paired", gradient_entry, "wide", "paired", (5, 5, 9, 33, 16, 3), "xy")
    add("wide-adjoint-fp32", gradient_entry, "wide", "gram", wsmall, "xy", None, "float32")
    return T


@pytest.mark.parametrize("make,args,kw", _table())
def test_truncated_modes_return_the_same_bits_whatever_their_slabs_held(make, args, kw, request):
    args = tuple(a() if callable(a) and not isinstance(a, type) else a for a in args)      # (workspace rules: asked of the plan here)
    call, launches = make(*args, **kw)
    n = three_runs(call, request.node.callspec.id, launches)
    print("%s: %d allocations intercepted per run, launches %s" % (request.node.callspec.id, n, launches))
    assert n >= 1


# ---- (c) solver families the ledger reaches through one budget only ------------------------------------------------------------------------

def _walks(A, B, M, N, D, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda n, m: (torch.cumsum(torch.randn(n, m, D, generator=g, dtype=torch.float64), 1) / np.sqrt(m * D)).cuda()
    return mk(A, M), mk(B, N)


def test_gram_gradient_in_three_row_blocks_and_more(monkeypatch):
    """compute_Gram with backward under a budget that cuts the 20 rows into row blocks: every block's adjoint launch meets the buffers
    the previous block's launches freed"""
    import sigkernel_amd
    from sigkernel_amd import _lib
    X, Y = _walks(20, 18, 70, 66, 3, 5)
    w = torch.randn(20, 18, generator=torch.Generator().manual_seed(6), dtype=torch.float64).cuda()
    calls = []
    for name in ("rbf_adjoint_fused", "rbf_adjoint_fused_mb", "solve_adj"):
        real = getattr(_lib.HipBackend, name)
        monkeypatch.setattr(_lib.HipBackend, name, (lambda real, name: lambda self, *a, **k: (calls.append(name), real(self, *a, **k))[1])(real, name))
    sk = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(0.9), 1, workspace_bytes=1000000)

    def run():
        del calls[:]
        x = X.clone().requires_grad_(True)
        K = sk.compute_Gram(x, Y)
        (K * w).sum().backward()
        assert len(calls) >= 3, calls            # row blocks of the backward pass
        return {"value": K.detach(), "grad": x.grad}
    n = three_runs(run, "gram gradient in row blocks")
    print("row blocks: %d adjoint calls (%s), %d allocations intercepted per run" % (len(calls), sorted(set(calls)), n))
    assert n >= 1


@pytest.mark.parametrize("kind", ["linear", "rbf"])
def test_the_wide_static_route_and_its_adjoint(kind):
    """paths of 33 dims: the K-looped matrix-core node Gram, the streaming solver and the static adjoint's chain rule behind it"""
    import sigkernel_amd
    X, Y = _walks(3, 4, 50, 70, 33, 8)
    w = torch.randn(3, 4, generator=torch.Generator().manual_seed(9), dtype=torch.float64).cuda()
    sk = sigkernel_amd.SigKernel(sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(0.9), 1)

    def run():
        x = X.clone().requires_grad_(True)
        K = sk.compute_Gram(x, Y)
        (K * w).sum().backward()
        return {"value": K.detach(), "grad": x.grad}
    _, names = instance_ledger.traced(run)
    assert any("k_static_wide_mfma" in n for n in names), sorted(names)
    assert three_runs(run, "wide static route, %s" % kind) >= 1


@pytest.mark.parametrize("kind", ["linear", "rbf"])
def test_a_launch_that_draws_from_its_work_counter(kind):
    """No ledger call has the 16384 pairs from which _lib._queue hands a counter out at all, and none fills the chip with eight pairs and more
    per lane group, from where the one-band forward deals only a share out up front and draws the rest from the counter (sk_pair_stream.h:
    plan_pair_stream).  640 x 640 pairs of 16 points do; the loss wrappers' one-launch forward on 128 + 128 such paths takes a counter too."""
    import sigkernel_amd
    X, Y = _walks(640, 640, 16, 16, 3, 21)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.LinearKernel() if kind == "linear" else sigkernel_amd.RBFKernel(0.9), 1)

    def run():
        x = X[:128].clone().requires_grad_(True)
        mmd = sk.compute_mmd(x, Y[:128])
        mmd.backward()
        return {"gram": sk.compute_Gram(X, Y), "sym": sk.compute_Gram(X, X, sym=True), "mmd": mmd.detach(), "mmd.grad": x.grad}
    assert three_runs(run, "work counter, %s" % kind) >= 1
    assert SITES[-1][1].get(("_lib", "_queue"), 0) >= 3, SITES[-1][1]

