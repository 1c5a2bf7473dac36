"""Poisoned workspaces -- TESTS ONLY: control what every buffer the library takes from torch.empty holds when a kernel first sees it.

The kernels are unmasked by design (padding rows and columns hold zeros, no lane is masked), so a result is right only if every padded
word and every slab or carry word a block reads was WRITTEN by the same call; 0 * NaN is not zero.  A fresh test process never shows a
violation: the caching allocator hands out zero pages or the small finite numbers of the previous test.  `poisoned(byte)` makes the
contents deliberate:

    with poisoned(0xFF) as p:
        out = call()
    p.count, p.sites          # interceptions in all, and {(module, function): count}

For its duration the module attribute `torch` of every loaded sigkernel_amd module is a proxy that forwards everything to the real
torch except the uninitialised allocators (empty, empty_like, empty_strided): those allocate and then fill every byte of the new tensor
with `byte` on the current stream.  torch.zeros, the inputs, the test's own tensors and torch's internals never see the proxy.  What the
library caches across calls is dropped on entry and on exit, so a buffer built under one pattern is not reused under the next.

    byte   fp64 / fp32                   integers        why
    0x00   zero                          zero            what today's suite enjoys by luck, now deliberate
    0xFF   NaN                           -1              survives 0 * x
    0x55   1.19e103 / 1.47e13 (finite)   large positive  survives fmax / fmin, sums and comparisons that drop a NaN

`integer_sites` (GPU runs): the (module, function) pairs whose integer / byte allocations have been audited -- every word a kernel reads
AS AN INTEGER is initialised on the launch stream before its first read (the table is in tests/test_gpu_poison.py).  An integer or
byte allocation anywhere else raises: a counter that starts from garbage can send a wave outside its arrays, so such a site is read
first and run second.  None (CPU runs): every site is poisoned.

same_bits(a, b) compares tensors through their integer views (equal NaNs are equal), with shape and dtype."""
import contextlib
import sys

import numpy as np
import torch

PATTERNS = (0x00, 0xFF, 0x55)
ALLOCATORS = ("empty", "empty_like", "empty_strided")
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class UnauditedIntegerSite(AssertionError):
    pass


class _TorchProxy:
    """the real torch module with filling allocators; `log` is the poisoned() record"""

    def __init__(self, real, byte, log, integer_sites):
        self.__dict__.update(_real=real, _byte=int(byte), _log=log, _integer_sites=integer_sites)
        for name in ALLOCATORS:
            self.__dict__[name] = self._allocator(name)

    def __getattr__(self, name):
        return getattr(self._real, name)

    def __setattr__(self, name, value):
        setattr(self._real, name, value)

    def _allocator(self, name):
        alloc = getattr(self._real, name)

        def filled(*args, **kwargs):
            t = alloc(*args, **kwargs)
            frame = sys._getframe(1)
            site = (frame.f_globals.get("__name__", "?").rsplit(".", 1)[-1], frame.f_code.co_name)
            if self._integer_sites is not None and not t.dtype.is_floating_point and site not in self._integer_sites:
                raise UnauditedIntegerSite("%s.%s allocates an uninitialised %s buffer that is not on the audited table" % (site + (t.dtype,)))
            if t.numel():      # (a fresh allocation owns its storage: every byte of it, whatever the strides)
                self._real.empty(0, dtype=self._real.uint8, device=t.device).set_(t.untyped_storage()).fill_(self._byte)
            self._log.count += 1
            self._log.sites[site] = self._log.sites.get(site, 0) + 1
            return t
        filled.__name__ = name
        return filled


class _Record:
    def __init__(self, byte):
        self.byte, self.count, self.sites = byte, 0, {}


def product_modules():
    """the loaded sigkernel_amd modules that hold a `torch` attribute (all of them: the allocators of _lib, sigkernel and distributed, and
    whatever else might allocate one day)"""
    import sigkernel_amd  # noqa: F401
    for extra in ("sigkernel_amd.distributed",):
        __import__(extra)
    return [m for name, m in sorted(sys.modules.items())
            if (name == "sigkernel_amd" or name.startswith("sigkernel_amd.")) and m is not None and isinstance(getattr(m, "torch", None), (type(torch), _TorchProxy))]


def reset_caches():
    """what the library keeps from call to call: the loss wrappers' constant weights, the backend's last-launch records"""
    from sigkernel_amd import _lib, sigkernel
    sigkernel._LOSS_WEIGHTS.clear()
    be = _lib.get_backend()
    for name in ("last_split_status", "last_fused_err", "last_fused_ppg"):
        if hasattr(be, name):
            setattr(be, name, None)


@contextlib.contextmanager
def poisoned(byte, integer_sites=None):
    if not 0 <= int(byte) <= 0xFF:
        raise ValueError("a fill byte, got %r" % (byte,))
    rec = _Record(int(byte))
    mods = product_modules()
    was = [(m, m.torch) for m in mods]
    if any(isinstance(t, _TorchProxy) for _, t in was):
        raise RuntimeError("poisoned() does not nest")
    proxy = _TorchProxy(torch, byte, rec, None if integer_sites is None else frozenset(integer_sites))
    reset_caches()
    try:
        for m in mods:
            m.torch = proxy
        yield rec
    finally:
        for m, t in was:
            m.torch = t
        reset_caches()


def _bits(t):
    t = t.detach().contiguous()
    if t.is_complex():
        t = torch.view_as_real(t).contiguous()
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    return t.reshape(-1).view(_INT_VIEW[t.element_size()])


def same_bits(a, b):
    """(True, "") when a and b have one shape, one dtype and the same bits; else (False, the first differing flat index with both values)"""
    if isinstance(a, torch.Tensor) != isinstance(b, torch.Tensor):
        return False, "a tensor against %r" % (type(b if isinstance(a, torch.Tensor) else a),)
    if not isinstance(a, torch.Tensor):
        a, b = torch.as_tensor(a), torch.as_tensor(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False, "shape / dtype %s %s against %s %s" % (tuple(a.shape), a.dtype, tuple(b.shape), b.dtype)
    if a.numel() == 0:
        return True, ""
    ne = _bits(a) != _bits(b.to(a.device))
    if not bool(ne.any()):
        return True, ""
    i = int(torch.nonzero(ne)[0, 0])
    idx = tuple(int(v) for v in np.unravel_index(i, tuple(a.shape))) if a.dim() else ()
    va, vb = a.detach().contiguous().reshape(-1)[i].item(), b.detach().contiguous().reshape(-1)[i].item()
    return False, "%d of %d elements differ, the first at %s: %r against %r" % (int(ne.sum()), a.numel(), idx, va, vb)


def assert_same_bits(first, other, what):
    """every entry of the dict (or tuple) `other` has the bits of `first`'s; None entries must be None on both sides"""
    if not isinstance(first, dict):
        first, other = dict(enumerate(first)), dict(enumerate(other))
    assert first.keys() == other.keys(), (what, sorted(first), sorted(other))
    bad = []
    for k in first:
        if first[k] is None or other[k] is None:
            if first[k] is not other[k]:
                bad.append("%s: None on one side only" % (k,))
            continue
        ok, msg = same_bits(first[k], other[k])
        if not ok:
            bad.append("%s: %s" % (k, msg))
    assert not bad, "%s: %s" % (what, "; ".join(bad))
