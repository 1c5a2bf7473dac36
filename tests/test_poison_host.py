"""The host layer under poisoned workspaces, no GPU (tests/poison.py has the method and the three patterns): the proxy reaches every
uninitialised allocation of the product, it shows a read-before-write, and sigkernel.py / distributed.py on the oracle-backed fake
back-end return the same bits whatever their torch.empty buffers held."""
import ast
import glob
import os
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import sigkernel_amd
from conftest import ROOT, golden, make_kernel
from poison import ALLOCATORS, PATTERNS, assert_same_bits, poisoned, same_bits
from sigkernel_amd import _lib

FIXTURES = ["gram_c2mini_rbf_d1", "gram_c3mini_lin_d1", "gram_lin_d0_ragged", "gram_lin_d2_ragged", "gram_len2", "gram_wide_lin_d0"]


def test_every_uninitialised_allocation_is_spelled_on_the_modules_torch_name():
    """The proxy replaces a module's `torch` attribute, so it sees exactly the calls spelled torch.<allocator>(...): no allocator may be
    imported from torch by name, and no Tensor.new_empty (a method: it would go past the proxy)."""
    names = set(ALLOCATORS) | {"new_empty"}
    total = 0
    for path in sorted(glob.glob(os.path.join(ROOT, "sigkernel_amd", "*.py"))):
        tree = ast.parse(open(path).read(), path)
        mod = os.path.basename(path)
        sites, bad = 0, []
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.module and node.module.split(".")[0] == "torch":
                bad += ["line %d: from %s import %s" % (node.lineno, node.module, a.name) for a in node.names if a.name in names]
            if isinstance(node, ast.Import):      # `import torch as <other name>` would hide the module from the proxy
                bad += ["line %d: import torch as %s" % (node.lineno, a.asname) for a in node.names if a.name == "torch" and a.asname not in (None, "torch")]
            if not isinstance(node, ast.Call):
                continue
            f = node.func
            callee = f.attr if isinstance(f, ast.Attribute) else f.id if isinstance(f, ast.Name) else None
            if callee not in names:
                continue
            sites += 1
            if not (isinstance(f, ast.Attribute) and callee in ALLOCATORS and isinstance(f.value, ast.Name) and f.value.id == "torch"):
                bad.append("line %d: %s" % (node.lineno, ast.unparse(f)))
        print("%-20s %3d uninitialised allocation sites" % (mod, sites))
        assert not bad, "%s: not spelled torch.<allocator>(...): %s" % (mod, "; ".join(bad))
        total += sites
    assert total >= 80, total      # (the three modules the issue counts hold about 90: an empty scan must not pass)


_TOY = """
import torch


def reads_first(x):
    buf = torch.empty(4, dtype=torch.float64)
    out = x + buf[3]            # read ...
    buf[:] = 1.0                # ... before the write
    return out + buf[0]


def writes_first(x):
    buf = torch.empty(4, dtype=torch.float64)
    buf[:] = 1.0
    return x + buf[3] + buf[0]
"""


def _toy_module():
    """a module of its own, given the proxy like a product module: one function reads a torch.empty word before writing it, one after"""
    m = types.ModuleType("sigkernel_amd._poison_toy")
    exec(compile(_TOY, "_poison_toy.py", "exec"), m.__dict__)
    return m


def test_a_read_before_the_write_is_caught_and_a_write_first_is_not(monkeypatch):
    import sys
    toy = _toy_module()
    monkeypatch.setitem(sys.modules, toy.__name__, toy)
    x = torch.arange(3, dtype=torch.float64)
    got = {}
    for byte in PATTERNS:
        with poisoned(byte) as p:
            got[byte] = (toy.reads_first(x), toy.writes_first(x))
        assert p.count == 2 and p.sites == {("_poison_toy", "reads_first"): 1, ("_poison_toy", "writes_first"): 1}
        assert toy.torch is torch                                    # restored
    for byte in PATTERNS[1:]:
        ok, msg = same_bits(got[0x00][0], got[byte][0])
        assert not ok and "first at (0,)" in msg, msg               # the three patterns give three different results
        assert same_bits(got[0x00][1], got[byte][1]) == (True, "")
    assert not same_bits(got[0xFF][0], got[0x55][0])[0]
    assert bool(torch.isnan(got[0xFF][0]).all()) and bool((got[0x55][0] > 1e100).all()) and torch.equal(got[0x00][0], x + 1.0)


def test_the_proxy_is_taken_away_after_an_exception_and_fills_every_allocator():
    from sigkernel_amd import distributed, sigkernel
    with pytest.raises(ZeroDivisionError):
        with poisoned(0x55):
            assert all(m.torch is not torch for m in (_lib, sigkernel, distributed))
            a = _lib.torch.empty(3, 5, dtype=torch.float32)
            b = _lib.torch.empty_like(a, dtype=torch.int16)
            c = _lib.torch.empty_strided((2, 3), (1, 2), dtype=torch.float64)
            d = _lib.torch.empty((), dtype=torch.float64)
            e = _lib.torch.empty(0, 4)
            z = _lib.torch.zeros(3)
            assert bool((a.view(torch.int32) == 0x55555555).all()) and bool((b == 0x5555).all()) and e.numel() == 0
            assert bool((c.view(torch.int64) == 0x5555555555555555).all()) and d.view(1).view(torch.int64).item() == 0x5555555555555555
            assert bool((z == 0).all()) and _lib.torch.float64 is torch.float64 and isinstance(a, _lib.torch.Tensor)
            1 / 0
    assert all(m.torch is torch for m in (_lib, sigkernel, distributed))
    # same_bits: equal NaNs are equal, -0.0 is not 0.0, and shape / dtype count
    nan = torch.tensor([float("nan"), 1.0])
    assert same_bits(nan, nan.clone())[0] and not same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))[0]
    assert not same_bits(torch.zeros(2), torch.zeros(2, 1))[0] and not same_bits(torch.zeros(2), torch.zeros(2, dtype=torch.float64))[0]


def _counting_backend():
    """the oracle-backed fake back-end, counting its forward solves: one per row tile of sigkernel._gram_block"""
    from fake_backend import OracleBackend

    class Counting(OracleBackend):
        solves = 0

        def solve_fwd(self, *a, **k):
            type(self).solves += 1
            return super().solve_fwd(*a, **k)
    return Counting()


def _host_calls(c, workspace_bytes, be):
    """every output and gradient of the host-layer calls on fixture c -> ({name: tensor}, forward solves of the first Gram call)"""
    X, Y, w = (torch.from_numpy(c[k]) for k in ("X", "Y", "w"))
    n = min(X.shape[0], Y.shape[0])
    sk = sigkernel_amd.SigKernel(make_kernel(c), int(c["dyadic"]), _naive_solver=bool(c["naive"]), workspace_bytes=workspace_bytes)
    out = {}

    def grad(name, fn, *weights):
        Xg = X.clone().requires_grad_(True)
        v = fn(Xg)
        ((v * weights[0]).sum() if weights else v.sum()).backward()
        out[name], out[name + ".grad"] = v.detach(), Xg.grad
    type(be).solves = 0
    out["gram_forward_only"] = sk.compute_Gram(X, Y)
    blocks = type(be).solves
    grad("gram", lambda Xg: sk.compute_Gram(Xg, Y), w)
    grad("gram_sym", lambda Xg: sk.compute_Gram(Xg, Xg, sym=True))
    grad("kernel", lambda Xg: sk.compute_kernel(Xg[:n], Y[:n]), torch.from_numpy(c["wp"]))
    if X.shape[1] == Y.shape[1]:      # (the reference's estimator concatenates the batches: one length)
        grad("mmd", lambda Xg: sk.compute_mmd(Xg, Y))
    out["gram_prefixes"] = sk.compute_Gram_prefixes(X, Y)
    out["kernel_prefixes"] = sk.compute_kernel_prefixes(X[:n], Y[:n])
    out["gram_prefixes.last_row"] = sk.compute_Gram_prefixes(X, Y, nodes="last_row")
    return out, blocks


@pytest.mark.parametrize("tiny", [False, True], ids=["default_budget", "one_row_per_tile"])
@pytest.mark.parametrize("name", FIXTURES)
def test_host_layer_results_do_not_depend_on_what_its_buffers_held(name, tiny):
    c = golden(name)
    be = _counting_backend()
    prev = _lib.set_backend(be)
    try:
        runs = {}
        for byte in PATTERNS:
            with poisoned(byte) as p:
                runs[byte], blocks = _host_calls(c, 1 if tiny else None, be)
            print("%s %s 0x%02X: %d allocations intercepted %s, %d row blocks in compute_Gram"
                  % (name, "workspace_bytes=1" if tiny else "default", byte, p.count, sorted(p.sites.items()), blocks))
            assert p.count >= 1
            A = c["X"].shape[0]
            # streamed rows: a budget of one byte leaves one row of X per tile; the default budget one tile (single points: no solve at all)
            assert blocks == (0 if c["X"].shape[1] < 2 else A if tiny else 1), blocks
    finally:
        _lib.set_backend(prev)
    for byte in PATTERNS[1:]:
        assert_same_bits(runs[0x00], runs[byte], "%s under 0x%02X against 0x00" % (name, byte))


def _distributed_runs(tmp_path, name, world):
    """{byte: [rank 0's results, rank 1's, ...]}: ONE group of `world` processes makes the calls under each pattern in turn"""
    from test_distributed import _free_port, _worker
    mp.spawn(_worker, args=(world, _free_port(), name, str(tmp_path), PATTERNS), nprocs=world, join=True)
    return {byte: [dict(np.load(tmp_path / ("rank%d.p%02x.npz" % (r, byte)))) for r in range(world)] for byte in PATTERNS}


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_results_do_not_depend_on_what_the_gather_buffers_held(tmp_path, world):
    """distributed.py under gloo, the worker of tests/test_distributed.py with the pattern passed in: five rows on two and on four ranks, so
    the padded all-gather has padding rows (and at world 4 a rank without rows).  Gram, gradient and MMD of every rank, bit for bit."""
    name = "gram_c3mini_lin_d1"
    rows = golden(name)["X"].shape[0]
    assert rows % world != 0
    runs = _distributed_runs(tmp_path, name, world)
    for r in range(world):
        first = runs[0x00][r]
        assert int(first["intercepted"]) >= 1, "rank %d intercepted no allocation" % r
        print("world %d rank %d: %d allocations intercepted" % (world, r, int(first["intercepted"])))
        for byte in PATTERNS[1:]:
            other = runs[byte][r]
            for key in ("gram", "grad_w", "grad_w_again", "mmd", "grad_mmd"):
                ok, msg = same_bits(torch.from_numpy(np.asarray(first[key])), torch.from_numpy(np.asarray(other[key])))
                assert ok, "world %d rank %d %s under 0x%02X: %s" % (world, r, key, byte, msg)
        for key in ("gram", "grad_w", "mmd", "grad_mmd"):      # every rank holds the same full results
            assert same_bits(torch.from_numpy(np.asarray(first[key])), torch.from_numpy(np.asarray(runs[0x00][0][key])))[0], (r, key)
