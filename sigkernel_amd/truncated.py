"""truncated_sig_kernel -- the truncated signature kernel of Kiraly and Oberhauser with a weight per level and the lower-order
approximations (reference transformers.py:201-236, which builds six-dimensional numpy arrays and shifts them with a spline filter).

The rows of ``X (A, M, D)`` and ``Y (B, N, D)`` are used as STEPS (the function does not difference them): ``G[a,i,b,j] = <X[a,i], Y[b,j]>``.
Level m of a pair is a set of d x d planes ``R^m[p][q]``, ``d = min(m, order)``, over the M x N step grid::

    R^1[0][0]     = G
    R^{m+1}[0][0] = G * sum_{i'<i, j'<j} sum_{p,q} R^m[p][q]
    R^{m+1}[0][q] = G / (q+1) * sum_{i'<i} sum_p R^m[p][q-1]          (same j)
    R^{m+1}[p][0] = G / (p+1) * sum_{j'<j} sum_q R^m[p-1][q]          (same i)
    R^{m+1}[p][q] = G / ((p+1)(q+1)) * R^m[p-1][q-1]                  (same node)
    K = sigma[0] + sum_m sigma[m] * sum_{nodes, planes} R^m

Two routes, chosen by ``sk_route_query(SK_OP_TRUNCATED, ...)``:

* the HIP kernel ``k_trunc_sig`` (csrc/sk_truncated.hip): every level in ONE skewed sweep of the step grid, nothing of size pairs x M x N
  in HBM; forward only; also on (y, x) with the result transposed when only the second batch fits its lanes (the recursion is symmetric
  under swapping the batches together with the plane indices);
* ``_truncated_torch``: the same recursion as ``cumsum`` and slicing on the paths' device, tiled over rows of X by ``workspace_bytes``;
  differentiable by autograd -- it serves every input that requires grad and every shape outside the kernel's scope.

A third, OPT-IN route serves order 1 beyond that scope -- more than 128 steps on both sides, or a second side beyond the wave's y block:
the kernel's LONG mode (``HipBackend.truncated_long``, ``sk_route_query(SK_OP_TRUNCATED_LONG, ...)``: the rows in bands of 128 with the
last row's hand-down carried through a slab in HBM, the columns in tiles of the y block; any number of steps, path dim <= 16, forward
only).  With ``sigkernel_amd.routes.truncated_long`` on (environment ``SK_TRUNCATED_LONG``), the three functions and
``TruncatedSigKernel`` on its plain kernel ask it where the plain launch declined both orientations, the order is 1 and no gradient is
pending; the slabs stay within ``workspace_bytes``.  The switch is off by default -- every call then does what it did -- and flipping
it is left to a later change.

``truncated_sig_kernel_paired`` is the same kernel on P pairs ``(X[p], Y[p])``: the same two routes (the HIP kernel in its paired mode, one
pair per lane group; the torch restatement tiled over pairs), the same scope, and nothing of size P x P on either.  It is what
``truncated_sig_kernel(..., normalize=True)`` -- ``K[a, b] / sqrt(k(x_a, x_a) k(y_b, y_b))`` -- takes its two diagonals from.

``truncated_sig_kernel_levels`` returns the level terms ``k_m = sum_{nodes, planes} R^m`` themselves, ``(L + 1, A, B)`` with ``k_0 = 1``: the
sweep holds them all when it ends (the levels mode of ``k_trunc_sig``: an epilogue, no second sweep), and ``_truncated_levels_torch`` is the
restatement that keeps each level's sum.  ``K`` is linear in them -- ``truncated_from_levels`` forms ``sum_m sigma[m] k_m`` for any weights,
differentiably, and with per-path scales ``(lx[a] ly[b])^m`` in front, because ``k_m(c x, y) = c^m k_m(x, y)`` at every order: every
truncation below L, every choice of weights and every rescaling of the paths is a re-weighting of ONE sweep's output.
``truncated_robust_scales`` solves the scales of Chevyrev and Oberhauser's robust normalisation from the paired self levels.

Each thing is stated once.  ``_level_sums`` is the recursion on a given G and ``_restatement`` its tiling, behind all three torch routes
(``_step_gram``: G of steps; ``_lifted_gram``: G of points under a static kernel, TruncatedSigKernel's); the three public
functions share ``_prepare`` (stage, check) and ``_launched``: ``_routed`` (try (X, Y), then (Y, X)) on ``_chunked`` (paired launches within
the workspace, in ``_pair_slices`` runs); the ctypes call and the staging rule are the backend's (``_lib.HipBackend._truncated``,
``_lib._truncated_staging``).

``TruncatedSigKernel`` is the SigKernel-shaped front (paths in, ``compute_Gram`` / ``compute_kernel`` / ``compute_mmd``) and the one place where
a gradient stays on the HIP route: ``_RouteLevels`` is THE autograd function on the level terms, along one of four ``_AdjointRoute`` records,
and ``TruncatedSigKernel._route_serves`` THE predicate that says whether a route serves a call.  ``_PLAIN``: forward the levels mode,
backward the kernel's adjoint mode (``HipBackend.truncated_adjoint``: order 1, dim <= 8).  The three functions above keep their
rule -- a gradient pending means the torch restatement.  Its ``static_kernel`` is the one place where G is something other than inner
products of steps: an RBFKernel is the kernel's points mode -- forward only, unless ``points_adjoint=True`` asks for ``_POINTS``, whose
backward is the kernel's points-adjoint mode (``HipBackend.truncated_points_adjoint``) -- anything else the restatement on ``_lifted_gram``.
Beyond the adjoint mode's 128 steps a gradient takes the restatement too, unless ``long_adjoint=True`` asks for ``_LONG``: the long
mode's levels launch forward, the kernel's long-adjoint mode backward (``HipBackend.truncated_long_adjoint``: order 1, dim <= 8, any steps);
at path dims 9 .. 16, unless ``wide_adjoint=True`` asks for ``_WIDE``: the levels mode forward, the wide-adjoint mode backward
(``HipBackend.truncated_wide_adjoint``).
"""
import collections

import numpy as np
import torch

from . import _lib
from ._routes import routes
from .sigkernel import _functional
from .static_kernels import LinearKernel, RBFKernel

__all__ = ["truncated_sig_kernel", "truncated_sig_kernel_paired", "truncated_sig_kernel_levels", "truncated_from_levels",
           "truncated_robust_scales", "TruncatedSigKernel"]

_DEFAULT_WORKSPACE = 1 << 30


def _excl(t, dim):
    """exclusive prefix sum along `dim`: out[k] = sum_{k' < k} t[k']"""
    c = torch.cumsum(t, dim)
    return torch.cat([torch.zeros_like(c.narrow(dim, 0, 1)), c.narrow(dim, 0, c.shape[dim] - 1)], dim)


def _sigma_vector(sigma, num_levels, dtype, device):
    if isinstance(sigma, torch.Tensor):
        s = sigma.to(dtype=dtype, device=device)
    else:
        s = torch.as_tensor(np.asarray(sigma, dtype=np.float64), dtype=dtype, device=device)
    if s.dim() > 1 or (s.dim() == 1 and s.numel() not in (1, num_levels + 1)):
        raise ValueError("sigma must be a scalar or hold num_levels + 1 = %d values, got shape %s" % (num_levels + 1, tuple(s.shape)))
    return s.reshape(-1).expand(num_levels + 1) if s.numel() == 1 else s


def _check_args(X, Y, num_levels, order):
    if X.dim() != 3 or Y.dim() != 3:
        raise ValueError("X and Y must have shape (batch, length, dim)")
    if X.shape[2] != Y.shape[2]:
        raise ValueError("X and Y must have the same path dimension")
    if X.dtype != Y.dtype or X.device != Y.device:
        raise ValueError("X and Y must share dtype and device")
    if X.dtype not in (torch.float64, torch.float32):
        raise TypeError("sigkernel_amd supports float64 and float32 tensors, got %s" % X.dtype)
    if int(num_levels) != num_levels or num_levels < 1:
        raise ValueError("num_levels must be a positive integer, got %r" % (num_levels,))
    if int(order) != order:
        raise ValueError("order must be an integer, got %r" % (order,))
    num_levels, order = int(num_levels), int(order)
    if order > num_levels:
        raise ValueError("order must not exceed num_levels (%d), got %d" % (num_levels, order))
    return num_levels, (num_levels if order < 1 else order)


def _step_gram(X, Y, paired):
    """G of the plain kernel: inner products of the STEPS X (A, M, D) and Y (B, N, D) -> (A, B, M, N), paired (P, M, N)"""
    return torch.einsum("pid,pjd->pij", X, Y) if paired else torch.einsum("aid,bjd->abij", X, Y)


def _lifted_gram(static_kernel):
    """G of the kernel lifted through `static_kernel` (anything with Gram_matrix / batch_kernel): X and Y hold POINTS, and
    G[i][j] = k(x_{i+1}, y_{j+1}) - k(x_{i+1}, y_j) - k(x_i, y_{j+1}) + k(x_i, y_j), the second difference of the static Gram"""
    def gram(X, Y, paired):
        K = static_kernel.batch_kernel(X, Y) if paired else static_kernel.Gram_matrix(X, Y)
        return (K[..., 1:, 1:] - K[..., 1:, :-1]) - (K[..., :-1, 1:] - K[..., :-1, :-1])
    return gram


def _level_sums(G, L, order):
    """THE recursion on a given G -- (A, B, M, N) of all pairs, or (P, M, N) of the pairs (X[p], Y[p]): yields k_1 .. k_L, each level's
    planes summed over the step grid; everything works on G's last two axes, whatever static kernel G came from"""
    yield G.sum((-2, -1))
    R = [[G]]
    for m in range(1, L):
        d = min(m + 1, order)
        total = sum(sum(row) for row in R)
        nxt = [[None] * d for _ in range(d)]
        nxt[0][0] = G * _excl(_excl(total, -2), -1)
        for q in range(1, d):
            nxt[0][q] = G * _excl(sum(R[p][q - 1] for p in range(len(R))), -2) / (q + 1)
            nxt[q][0] = G * _excl(sum(R[q - 1]), -1) / (q + 1)
        for p in range(1, d):
            for q in range(1, d):
                nxt[p][q] = G * R[p - 1][q - 1] / ((p + 1) * (q + 1))
        R = nxt
        yield sum(sum(row) for row in R).sum((-2, -1))


def _block(G, L, order, sig):
    """one tile, from its G: the weighted value sig[0] + sum_m sig[m] k_m, folded level by level as the sums arrive; sig None: the sums
    themselves, stacked under the ones of level 0"""
    if sig is None:
        out = list(_level_sums(G, L, order))
        return torch.stack([torch.ones_like(out[0])] + out, 0)
    K = sig[0]
    for m, k in enumerate(_level_sums(G, L, order), 1):
        K = K + sig[m] * k
    return K


def _restatement(X, Y, num_levels, sigma, order, paired, workspace_bytes, gram=None):
    """The three torch routes: check, empty case, and the recursion tiled over rows of X (over pairs) so that a tile's (2 d^2 + 6) arrays
    of the step grid -- times the levels autograd keeps -- stay within `workspace_bytes`.  sigma None: the level terms, tiles joined along
    axis 1 under the level axis; else the weighted value.  `gram(X tile, Y, paired)` supplies a tile's G: None -- X and Y hold steps and G
    is their inner products; a _lifted_gram -- they hold POINTS, the grid has one row and column fewer, and the tile's static Gram is one
    more array of the workspace."""
    num_levels, order = _check_args(X, Y, num_levels, order)
    if paired and X.shape[0] != Y.shape[0]:
        raise ValueError("X and Y must hold the same number of paths, got %d and %d" % (X.shape[0], Y.shape[0]))
    sig = None if sigma is None else _sigma_vector(sigma, num_levels, X.dtype, X.device)
    lifted = gram is not None
    gram = gram or _step_gram
    A, M = X.shape[0], X.shape[1] - lifted
    B, N = Y.shape[0], Y.shape[1] - lifted
    shape = (A,) if paired else (A, B)
    if A == 0 or B == 0 or M <= 0 or N <= 0:
        if sig is not None:
            return sig[0] * torch.ones(shape, dtype=X.dtype, device=X.device)
        out = torch.zeros((num_levels + 1,) + shape, dtype=X.dtype, device=X.device)
        out[0] = 1
        return out
    d = min(num_levels, order)
    budget = _DEFAULT_WORKSPACE if workspace_bytes is None else int(workspace_bytes)
    kept = num_levels if torch.is_grad_enabled() and (X.requires_grad or Y.requires_grad) else 1
    per_row = (1 if paired else B) * M * N * X.element_size() * (2 * d * d + 6 + lifted) * kept
    rows = int(max(1, min(A, budget // max(1, per_row))))
    return torch.cat([_block(gram(X[a:a + rows], Y[a:a + rows] if paired else Y, paired), num_levels, order, sig) for a in range(0, A, rows)],
                     1 if sig is None else 0)


def _truncated_levels_torch(X, Y, num_levels, order=-1, paired=False, workspace_bytes=None, gram=None):
    """The level terms k_0 .. k_L in torch ops on the tensors' own device, differentiable: (L + 1, A, B), paired (L + 1, P).  The recursion
    of _truncated_torch with each level's sum kept, tiled over rows of X (over pairs) by `workspace_bytes` exactly as it is.  `gram`:
    _restatement's -- a _lifted_gram on POINTS."""
    return _restatement(X, Y, num_levels, None, order, paired, workspace_bytes, gram)


def _truncated_torch(X, Y, num_levels, sigma=1., order=-1, workspace_bytes=None):
    """The recursion in torch ops on the tensors' own device (any device: the tests drive it on the CPU), differentiable; (A, B)."""
    return _restatement(X, Y, num_levels, sigma, order, False, workspace_bytes)


def _truncated_paired_torch(X, Y, num_levels, sigma=1., order=-1, workspace_bytes=None):
    """The recursion on the P pairs (X[p], Y[p]) in torch ops, differentiable; (P,).  Tiled over pairs: nothing of size P x P."""
    return _restatement(X, Y, num_levels, sigma, order, True, workspace_bytes)


def truncated_route(D, M, N, num_levels, order, elem_size):
    """ROUTE_FUSED / ROUTE_FUSED_SWAP / ROUTE_STREAM (= the torch restatement) for step counts M, N (sk_route_query, csrc/sk_route.hip)."""
    return int(_lib.load().sk_route_query(_lib.OP_TRUNCATED, int(order), int(D), int(M), int(N), int(num_levels), 0, int(elem_size), 0))


def _pair_slices(P, M, N, D, workspace_bytes):
    """THE pairs-per-run rule: the pairs of a paired batch in runs whose fp64 staging (8 or 16 doubles per step) stays within
    `workspace_bytes` -- all of them in one run, usually"""
    budget = _DEFAULT_WORKSPACE if workspace_bytes is None else int(workspace_bytes)
    fd, Ncp = _lib._truncated_staging(D, N)
    pairs = int(max(1, min(P, budget // (8 * fd * (M + Ncp)))))
    return [slice(p, p + pairs) for p in range(0, P, pairs)]


def _chunked(call, workspace_bytes, axis):
    """`call(X, Y)` of a paired backend method, on _pair_slices' runs of the pairs and the parts joined along `axis`; None where `call`
    says None"""
    def run(X, Y):
        parts = []
        for sl in _pair_slices(X.shape[0], X.shape[1], Y.shape[1], X.shape[2], workspace_bytes):
            k = call(X[sl], Y[sl])
            if k is None:
                return None
            parts.append(k)
        return parts[0] if len(parts) == 1 else torch.cat(parts, axis)
    return run


def _routed(call, X, Y, gram):
    """`call(X, Y)`, or where it says None (SK_ROUTE_FUSED_SWAP: only the second batch fits the kernel's lanes) `call(Y, X)`: k_m(x, y) =
    k_m(y, x) at every order, so a Gram result has its last two axes transposed back and a paired one is taken as it is.  None when both
    decline."""
    K = call(X, Y)
    if K is None:
        K = call(Y, X)
        if K is not None and gram:
            K = K.transpose(-2, -1).contiguous()
    return K


def _launched(call, X, Y, paired, workspace_bytes, axis=1):
    """THE launch of a backend method `call(x, y)` on the detached batches: a paired batch in _chunked's runs joined along `axis` (1: level
    terms, 0: values), either orientation (_routed, a Gram result transposed back).  None where the method declines both."""
    return _routed(_chunked(call, workspace_bytes, axis) if paired else call, X.detach(), Y.detach(), not paired)


def _stage(X, Y):
    """numpy arrays to the current device; -> (X, Y, whether the result goes back as numpy)"""
    as_numpy = isinstance(X, np.ndarray) or isinstance(Y, np.ndarray)
    if as_numpy:
        X, Y = (t if isinstance(t, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(t)) for t in (X, Y))
        X, Y = X.to("cuda"), Y.to("cuda")
    return X, Y, as_numpy


def _needs_grad(X, Y, sigma):
    return torch.is_grad_enabled() and (X.requires_grad or Y.requires_grad or (isinstance(sigma, torch.Tensor) and sigma.requires_grad))


def _prepare(X, Y, num_levels, order, paired):
    """the public functions' preamble -> (X, Y contiguous on a HIP device, num_levels, order as checked, numpy out?, the backend)"""
    X, Y, as_numpy = _stage(X, Y)
    num_levels, order = _check_args(X, Y, num_levels, order)
    if paired and X.shape[0] != Y.shape[0]:
        raise ValueError("X and Y must hold the same number of paths, got %d and %d" % (X.shape[0], Y.shape[0]))
    X, Y = X.contiguous(), Y.contiguous()
    _lib._dev(X, "X")
    _lib._dev(Y, "Y")
    return X, Y, num_levels, order, as_numpy, _lib.get_backend()


def _hip_serves(be, method, X, Y, sigma):
    """no gradient pending, no empty axis, and a backend that has `method` (the HIP kernel is forward only)"""
    return not _needs_grad(X, Y, sigma) and min(X.shape[0], X.shape[1], Y.shape[0], Y.shape[1]) > 0 and hasattr(be, method)


def _long_serves(be, X, Y, sigma, order):
    """the kernel's LONG mode may be asked (after the plain launch declined both orientations): the opt-in switch routes.truncated_long is
    on, order 1, no gradient pending, no empty axis, and a backend that has the method (the mode is forward only)"""
    return bool(routes.truncated_long) and order == 1 and _hip_serves(be, "truncated_long", X, Y, sigma)


def _long(be, X, Y, num_levels, weights, paired, workspace_bytes):
    """HipBackend.truncated_long on (X, Y), or on (Y, X) where the route query says that sweep is the shorter one; paired batches in
    _chunked's runs; `weights` None: the level terms.  None where it declines (one block's slab beyond the workspace)."""
    call = lambda x, y: be.truncated_long(x, y, num_levels, weights, paired, workspace_bytes)
    return _launched(call, X, Y, paired, workspace_bytes, 0 if weights is not None else 1)


def truncated_sig_kernel_paired(X, Y, num_levels, sigma=1., order=-1, workspace_bytes=None):
    """The truncated signature kernel of the pairs (X[p], Y[p]): X (P, M, D) and Y (P, N, D) hold STEPS, the result is (P,) with
    ``out[p] = truncated_sig_kernel(X[p:p+1], Y[p:p+1], ...)[0, 0]`` -- the diagonal of the matrix without the matrix.  ``num_levels``,
    ``sigma``, ``order``, the dtypes and numpy in / numpy out are those of truncated_sig_kernel; unequal batch sizes raise ValueError.

    Inside the HIP kernel's scope (the Gram matrix's: sk_route_query(SK_OP_TRUNCATED)) this is ONE launch of k_trunc_sig in its paired mode,
    on (Y, X) when only the second batch fits the lanes.  Inputs that require grad and shapes outside the scope take the differentiable
    torch restatement.  Nothing of size P x P is built on either route, and ``workspace_bytes`` (default 1 GiB) bounds what is: the torch
    route is tiled over pairs by it, and the HIP route's fp64 staging of the paths (8 or 16 doubles per step) is too -- a batch whose
    staging exceeds it goes in several launches."""
    X, Y, num_levels, order, as_numpy, be = _prepare(X, Y, num_levels, order, True)
    sig = _sigma_vector(sigma, num_levels, X.dtype, X.device)
    k = None
    if _hip_serves(be, "truncated_paired", X, Y, sigma):
        weights = sig.detach().double().cpu().tolist()
        k = _launched(lambda x, y: be.truncated_paired(x, y, num_levels, weights, order), X, Y, True, workspace_bytes, 0)
    if k is None and _long_serves(be, X, Y, sigma, order):
        k = _long(be, X, Y, num_levels, sig.detach().double().cpu().tolist(), True, workspace_bytes)
    if k is None:
        k = _truncated_paired_torch(X, Y, num_levels, sig, order, workspace_bytes)
    return k.cpu().numpy() if as_numpy else k


def _normalizer(k, name):
    """a batch's own kernel values, which must be positive (ONE device-to-host check per batch)"""
    if not bool((k > 0).all()):
        raise ValueError("normalize=True needs k(x, x) > 0 for every path, but `%s` holds a path whose truncated kernel with itself is "
                         "not positive (negative level weights can do that)" % name)
    return k


def truncated_sig_kernel(X, Y, num_levels, sigma=1., order=-1, workspace_bytes=None, normalize=False):
    """The truncated signature kernel matrix (reference transformers.py:201-236), as there: X (A, M, D) and Y (B, N, D) hold STEPS,
    ``sigma`` is a scalar or num_levels + 1 weights, ``order = num_levels`` (the default, -1) is the signature kernel truncated at
    ``num_levels`` and smaller orders are Kiraly and Oberhauser's lower-order approximations.  Returns (A, B) in the inputs' dtype.

    torch tensors on a HIP device, fp64 or fp32; numpy arrays are staged to the current device and the result comes back as numpy.
    Inputs that require grad take the differentiable torch route; the HIP kernel is forward only.

    ``normalize=True`` returns ``K[a, b] / sqrt(kx[a] * ky[b])`` with ``kx = truncated_sig_kernel_paired(X, X, ...)`` and ``ky`` likewise
    (same levels, weights and order): one Gram launch and two paired ones, A + B extra pairs, not A^2 + B^2.  When ``Y is X`` one of them
    is saved and the diagonal is 1 to rounding.  A ``kx`` or ``ky`` that is not positive -- possible with negative level weights --
    raises ValueError naming the argument; that check reads one flag per batch back from the device, so a normalised call synchronises
    with the host where the plain one does not.  With a gradient both parts take the torch route and autograd covers the quotient."""
    same = Y is X
    X, Y, num_levels, order, as_numpy, be = _prepare(X, Y, num_levels, order, False)
    sig = _sigma_vector(sigma, num_levels, X.dtype, X.device)
    K = None
    if _hip_serves(be, "truncated_gram", X, Y, sigma):
        weights = sig.detach().double().cpu().tolist()
        K = _launched(lambda x, y: be.truncated_gram(x, y, num_levels, weights, order), X, Y, False, workspace_bytes)
    if K is None and _long_serves(be, X, Y, sigma, order):
        K = _long(be, X, Y, num_levels, sig.detach().double().cpu().tolist(), False, workspace_bytes)
    if K is None:
        K = _truncated_torch(X, Y, num_levels, sig, order, workspace_bytes)
    if normalize:
        kx = _normalizer(truncated_sig_kernel_paired(X, X, num_levels, sig, order, workspace_bytes), "X")
        ky = kx if same else _normalizer(truncated_sig_kernel_paired(Y, Y, num_levels, sig, order, workspace_bytes), "Y")
        K = K / torch.sqrt(kx[:, None] * ky[None, :])
    return K.cpu().numpy() if as_numpy else K


def truncated_sig_kernel_levels(X, Y, num_levels, order=-1, paired=False, workspace_bytes=None):
    """The level terms of the truncated signature kernel: ``(num_levels + 1, A, B)`` with ``out[m, a, b] = k_m(X[a], Y[b])``, the sum of
    level m's planes over the step grid, and ``out[0] = 1`` -- so ``truncated_sig_kernel(X, Y, L, sigma, order)`` is
    ``sum_m sigma[m] * out[m]`` (truncated_from_levels).  ``paired=True``: ``(num_levels + 1, P)`` of the pairs ``(X[p], Y[p])``.  Every
    level is a contiguous matrix.  X, Y, ``num_levels``, ``order``, the dtypes and numpy in / numpy out are those of truncated_sig_kernel.

    Inside the HIP kernel's scope this is ONE launch of k_trunc_sig in its levels mode -- the sweep of the plain call plus an epilogue --
    on (Y, X) with every level transposed when only the second batch fits the lanes.  Inputs that require grad and shapes outside the
    scope take the differentiable torch restatement, tiled by ``workspace_bytes`` (default 1 GiB) as truncated_sig_kernel's; the paired HIP
    route's staging is bounded by it as truncated_sig_kernel_paired's."""
    X, Y, num_levels, order, as_numpy, be = _prepare(X, Y, num_levels, order, paired)
    K = None
    if _hip_serves(be, "truncated_levels", X, Y, None):
        K = _launched(lambda x, y: be.truncated_levels(x, y, num_levels, order, paired=paired), X, Y, paired, workspace_bytes)
    if K is None and _long_serves(be, X, Y, None, order):
        K = _long(be, X, Y, num_levels, None, paired, workspace_bytes)
    if K is None:
        K = _truncated_levels_torch(X, Y, num_levels, order, paired, workspace_bytes)
    return K.cpu().numpy() if as_numpy else K


def _scale_vector(scale, n, like, name):
    s = scale if isinstance(scale, torch.Tensor) else torch.as_tensor(np.asarray(scale, dtype=np.float64))
    s = s.to(dtype=like.dtype, device=like.device)
    if s.dim() > 1 or (s.dim() == 1 and s.numel() not in (1, n)):
        raise ValueError("%s must be a scalar or hold one value per path (%d), got shape %s" % (name, n, tuple(s.shape)))
    return s.reshape(-1).expand(n) if s.numel() == 1 else s


def truncated_from_levels(levels, sigma=1., scale_x=None, scale_y=None):
    """``sum_m sigma[m] * (scale_x[:, None] * scale_y[None, :])**m * levels[m]`` for ``levels (L + 1, A, B)`` of
    truncated_sig_kernel_levels -- the truncated kernel of the paths ``scale_x[a] X[a]`` and ``scale_y[b] Y[b]`` with weights ``sigma``
    (a scalar or L + 1 values), without another sweep: level m is homogeneous of degree m in either path.  ``levels (L + 1, P)``: the
    elementwise analogue, ``(scale_x * scale_y)**m``.  No scales: ``sum_m sigma[m] levels[m]``, which is truncated_sig_kernel.  Plain torch
    ops on the tensors' device: differentiable in ``sigma``, the scales and ``levels``.  numpy levels give a numpy result."""
    as_numpy = isinstance(levels, np.ndarray)
    if as_numpy:
        levels = torch.as_tensor(levels)
    if not isinstance(levels, torch.Tensor) or levels.dim() not in (2, 3) or levels.shape[0] < 2:
        raise ValueError("levels must have shape (num_levels + 1, A, B) or (num_levels + 1, P)")
    L = levels.shape[0] - 1
    sig = _sigma_vector(sigma, L, levels.dtype, levels.device)
    w = sig.reshape((L + 1,) + (1,) * (levels.dim() - 1))
    if scale_x is not None or scale_y is not None:
        one = torch.ones((), dtype=levels.dtype, device=levels.device)
        sx = _scale_vector(one if scale_x is None else scale_x, levels.shape[1], levels, "scale_x")
        sy = _scale_vector(one if scale_y is None else scale_y, levels.shape[-1], levels, "scale_y")
        lam = sx[:, None] * sy[None, :] if levels.dim() == 3 else sx * sy
        w = w * torch.stack([lam ** m for m in range(L + 1)], 0)
    K = (w * levels).sum(0)
    return K.detach().cpu().numpy() if as_numpy else K


def _psi(s, C, a):
    """Chevyrev and Oberhauser's psi: s up to C, then C + C^(1+a) (C^-a - s^-a) / a -- increasing, bounded by C (1 + 1/a)"""
    big = s.clamp_min(C)
    return torch.where(s <= C, s, C + C ** (1 + a) * (C ** -a - big ** -a) / a)


def truncated_robust_scales(self_levels, C=4.0, a=1.0):
    """The per-path scales of the robust signature normalisation (Chevyrev and Oberhauser, "Signature moments to characterize laws of
    stochastic processes", section 5) at truncation L.  ``self_levels = truncated_sig_kernel_levels(X, X, L, order, paired=True)``,
    ``(L + 1, P)``: ``n_m = k_m(x, x)``, the squared norm of level m of the path's signature.  Returns ``lam (P,)`` in [0, 1] with

        sum_m lam^(2m) n_m = psi(sum_m n_m),    psi(s) = s for s <= C,  C + C^(1+a) (C^-a - s^-a) / a beyond,

    so that the rescaled path ``lam x`` has a self-kernel of at most ``C (1 + 1/a)``; ``truncated_from_levels(levels, sigma, lam_x, lam_y)``
    is then the robustly normalised kernel.  Paths with ``s <= C`` get exactly 1.  The left side increases in lam from n_0 = 1 <= psi(s) to
    s >= psi(s): 64 bisection steps on [0, 1] for all paths at once on the levels' device, no host read inside the loop.  A negative
    ``n_m`` (orders below num_levels are not inner products of signature levels: nothing keeps k_m(x, x) from it) raises ValueError after
    ONE flag read.  Not differentiated:
    the scales are returned detached."""
    as_numpy = isinstance(self_levels, np.ndarray)
    n = torch.as_tensor(self_levels) if as_numpy else self_levels
    if not isinstance(n, torch.Tensor) or n.dim() != 2 or n.shape[0] < 2:
        raise ValueError("self_levels must have shape (num_levels + 1, P): truncated_sig_kernel_levels(X, X, L, order, paired=True)")
    if not (C > 0 and a > 0):
        raise ValueError("C and a must be positive, got C = %r, a = %r" % (C, a))
    n, dtype = n.detach(), n.dtype
    if bool((n < 0).any()):
        raise ValueError("truncated_robust_scales needs k_m(x, x) >= 0 at every level, but a path's self level is negative (orders below "
                         "num_levels can do that: use order = num_levels)")
    n = n.double()
    L = n.shape[0] - 1
    s = n.sum(0)
    target = _psi(s, float(C), float(a))
    lo, hi = torch.zeros_like(s), torch.ones_like(s)
    for _ in range(64):
        mid = 0.5 * (lo + hi)
        m2 = mid * mid
        f = n[L]
        for m in range(L - 1, -1, -1):      # Horner in lam^2
            f = f * m2 + n[m]
        below = f < target
        lo, hi = torch.where(below, mid, lo), torch.where(below, hi, mid)
    lam = torch.where(s <= C, torch.ones_like(s), 0.5 * (lo + hi)).to(dtype)
    return lam.cpu().numpy() if as_numpy else lam


def _on_hip(t):
    """the tensor lives on a HIP device: the one place TruncatedSigKernel asks (and the seam where the host tests stand a backend in on CPU tensors)"""
    return t.is_cuda


class _AdjointRoute(collections.namedtuple("_AdjointRoute", "switch op needs fits adjoint forward")):
    """One way TruncatedSigKernel keeps a gradient on the HIP kernel: `switch` the keyword (attribute) that turns it on, None for the
    route every object has; `op` the route op of its FORWARD; `needs` the backend attributes that must exist; `fits` / `adjoint` the
    backend's scope-and-workspace predicate and adjoint method; `forward` how the level terms are launched -- "levels": truncated_levels on
    steps, "points": truncated_levels at kind 1 with the RBF parameter, "long": truncated_long."""
    __slots__ = ()


_PLAIN = _AdjointRoute(None, _lib.OP_TRUNCATED, ("truncated_levels", "truncated_adjoint_fits"),
                       "truncated_adjoint_fits", "truncated_adjoint", "levels")                     # order 1, dim <= 8, at most 128 steps
_WIDE = _AdjointRoute("wide_adjoint", _lib.OP_TRUNCATED, ("truncated_levels", "truncated_wide_adjoint", "truncated_wide_adjoint_fits"),
                      "truncated_wide_adjoint_fits", "truncated_wide_adjoint", "levels")             # path dims 9 .. 16
_LONG = _AdjointRoute("long_adjoint", _lib.OP_TRUNCATED_LONG, ("truncated_long", "truncated_long_adjoint", "truncated_long_adjoint_fits"),
                      "truncated_long_adjoint_fits", "truncated_long_adjoint", "long")               # any number of steps
_POINTS = _AdjointRoute("points_adjoint", _lib.OP_TRUNCATED_RBF, ("truncated_levels", "truncated_points_adjoint_fits"),
                        "truncated_points_adjoint_fits", "truncated_points_adjoint", "points")       # POINT tensors under RBFKernel(param)


def _route_levels(be, route, X, Y, L, order, param, paired, workspace_bytes):
    """the level terms by the route's forward launch, (L + 1, A, B) / paired (L + 1, P); None where the backend declines both orientations"""
    if route.forward == "long":
        return _long(be, X, Y, L, None, paired, workspace_bytes)
    kw = dict(kind=1, param=param) if route.forward == "points" else {}
    return _launched(lambda x, y: be.truncated_levels(x, y, L, order, paired=paired, **kw), X, Y, paired, workspace_bytes)


def _adjoint(be, route, X, Y, w, L, param, paired, workspace_bytes):
    """d / dX of sum_pairs sum_m w[m - 1, pair] k_m(pair) by the route's adjoint mode of the kernel, in X's dtype; paired batches in
    _pair_slices' runs.  The points route: X and Y hold POINTS and the k_m are those of the lift through RBFKernel(param)."""
    args = (param,) if route.forward == "points" else ()
    call = lambda x, y, v, p: getattr(be, route.adjoint)(x, y, v, L, *args, p, workspace_bytes)
    if not paired:
        parts = [call(X, Y, w, False)]
    else:
        parts = [call(X[sl], Y[sl], w[:, sl], True) for sl in _pair_slices(X.shape[0], X.shape[1], Y.shape[1], X.shape[2], workspace_bytes)]
    if any(t is None for t in parts):
        raise RuntimeError("the adjoint mode of k_trunc_sig declined a shape its route query accepted")
    return (parts[0] if len(parts) == 1 else torch.cat(parts, 0)).to(X.dtype)


class _RouteLevels(torch.autograd.Function):
    """The level terms of tensors on a HIP device -- (L + 1, A, B), paired (L + 1, P) -- with the HIP kernel on both sides (a gradient:
    order 1), along an _AdjointRoute: forward = the route's levels launch (on (Y, X), transposed, where only that orientation serves),
    backward = its adjoint mode with w = grad_levels[1:], one launch per batch that needs a gradient: dY is the adjoint on (Y, X) with w
    transposed, and a symmetric call (Y is X) is ONE launch with w + w^T, since k_m(x, y) = k_m(y, x).  The caller has asked the route
    table for every side it needs (TruncatedSigKernel._route_serves)."""

    @staticmethod
    def forward(ctx, X, Y, route, L, order, param, paired, sym, workspace_bytes):
        lev = _route_levels(_lib.get_backend(), route, X, Y, L, order, param, paired, workspace_bytes)
        if lev is None:
            raise RuntimeError("the %s launch of k_trunc_sig declined a shape its route query accepted" % route.forward)
        ctx.save_for_backward(X, Y)
        ctx.mode = (route, L, param, paired, sym, workspace_bytes)
        return lev

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        X, Y = ctx.saved_tensors
        route, L, param, paired, sym, workspace_bytes = ctx.mode
        be = _lib.get_backend()
        adjoint = lambda x, y, w, p: _adjoint(be, route, x, y, w, L, param, p, workspace_bytes)
        w = grad[1:].double()
        dX = dY = None
        if sym:
            if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
                dX = adjoint(X, X, w + w.transpose(1, 2), False)
        else:
            if ctx.needs_input_grad[0]:
                dX = adjoint(X, Y, w.contiguous(), paired)
            if ctx.needs_input_grad[1]:
                dY = adjoint(Y, X, (w if paired else w.transpose(1, 2)).contiguous(), paired)
        return (dX, dY) + (None,) * 7


class TruncatedSigKernel:
    """The truncated signature kernel behind SigKernel's interface: ``X`` and ``Y`` are PATHS ``(batch, length, dim)`` -- differenced here
    with torch ops, so a gradient reaches whatever produced them -- and the kernel is truncated_sig_kernel's on the steps, ``num_levels``
    levels with weights ``sigma`` (a scalar or num_levels + 1 values; a tensor that requires grad is differentiated) at ``order``
    (default 1; -1: num_levels).

    Every call works on the level terms of ONE sweep and forms ``sum_m sigma[m] k_m`` from them (truncated_from_levels).  On a HIP device
    the sweep is the HIP kernel's levels mode, and at order 1 WITH a gradient pending too: the backward is then the kernel's adjoint mode,
    one launch per batch that requires grad (one in all for ``sym=True``), nothing of size pairs x M x N allocated -- where the forward
    and every batch that needs a gradient are in the kernel's scope (path dim <= 8 and at most 128 steps on a side that needs a gradient:
    sk_route_query(SK_OP_TRUNCATED_ADJOINT)) and a block's slab of (num_levels - 1) x (steps of the other side + lanes - 1) KB fits
    ``workspace_bytes`` (default 1 GiB).  Everything else -- CPU tensors, other orders, wider or longer paths -- takes the torch
    restatement as a whole, tiled by ``workspace_bytes``: the values do not depend on the route beyond rounding.

    ``static_kernel`` lifts the kernel through a static kernel k on the paths' POINTS, as Kiraly and Oberhauser state it:
    ``G[i][j] = k(x_{i+1}, y_{j+1}) - k(x_{i+1}, y_j) - k(x_i, y_{j+1}) + k(x_i, y_j)`` takes the place of ``<dx_i, dy_j>``.  ``None`` (the
    default) and a ``LinearKernel`` -- whose second difference IS ``<dx_i, dy_j>``, and whose ``Gram_matrix`` ignores ``scale`` -- are the
    plain kernel on its own code path.  An ``RBFKernel(s)`` on a HIP device with no gradient pending is ONE launch of the same HIP kernel
    in its points mode (k evaluated in the sweep from differences of coordinates, nothing of size pairs x M x N allocated) at order 1,
    path dim <= 16, <= 8 levels and at most 128 POINTS on one side (sk_route_query(SK_OP_TRUNCATED_RBF)).  By default a gradient, like
    a CPU tensor or a shape outside that scope, takes the torch restatement on the second differences of ``k.Gram_matrix`` /
    ``k.batch_kernel`` -- as does every other duck-typed static kernel -- differentiable in the paths and in ``sigma`` and tiled by
    ``workspace_bytes``.  A function-valued kernel (``features`` and ``base_kernel``) maps the paths through ``features`` once and lifts
    its ``base_kernel``.

    ``points_adjoint=True`` keeps the RBF lift on the HIP route WITH a gradient pending: the forward is the points mode's launch and the
    backward the same kernel's points-adjoint mode, one launch per batch that requires grad (one in all for ``sym=True``), bit-reproducible,
    nothing of size pairs x M x N allocated.  It takes effect for ``type(static_kernel) is RBFKernel`` at order 1 on a HIP device when the
    forward is in the points mode's scope and every batch that requires grad has path dim <= 8, at most 128 points
    (sk_route_query(SK_OP_TRUNCATED_RBF_ADJOINT)) and a block's slab of num_levels x (points of the other side + lanes - 1) KB within
    ``workspace_bytes``; every other call takes the restatement as a whole, as without the keyword.  ``sigma`` keeps its gradient either way
    (the RBF bandwidth is a float and has none).  The default is False -- every call then does what it did before the keyword existed --
    and flipping it is left to a later change.

    ``long_adjoint=True`` keeps the PLAIN kernel (``static_kernel`` None or a LinearKernel) on the HIP route with a gradient pending beyond
    those 128 steps: the forward is the long mode's levels launch (row bands of 128 steps, column tiles of 256) and the backward the same
    kernel's long-adjoint mode -- the reverse sweep through the same bands and tiles -- one launch per batch that requires grad (one in all
    for ``sym=True``), bit-reproducible, nothing of size pairs x M x N allocated.  It takes effect at order 1 on a HIP device where the
    route above declined, the forward is in the long mode's scope (sk_route_query(SK_OP_TRUNCATED_LONG): path dim <= 16) and every batch
    that requires grad has path dim <= 8 (sk_route_query(SK_OP_TRUNCATED_LONG_ADJOINT)) and a block's slab within ``workspace_bytes``:
    (num_levels - 1) x (steps of the other side + 63 per tile of 256) KB, plus with more than 128 steps of its own
    (bands + 2) x (num_levels - 1) x ceil64(steps of the other side) doubles.  The launch takes 8 blocks per CU only if all their slabs
    fit: at the default 1 GiB a few hundred steps already lower the block count, so pass a larger ``workspace_bytes`` for speed.  Every
    other call takes the restatement as a whole, as without the keyword, and ``sigma`` keeps its gradient either way.  The keyword does
    not depend on ``routes.truncated_long``, which keeps governing the calls without a gradient.  The default is False -- every call then
    does what it did before the keyword existed -- and flipping it is left to a later change.

    ``wide_adjoint=True`` keeps the PLAIN kernel on the HIP route with a gradient pending at path dims 9 to 16 -- what lead-lag plus
    add-time makes of four to seven channels: the forward is the levels launch every call without a gradient already takes there and the
    backward the kernel's wide-adjoint mode -- the adjoint mode's two sweeps with rows and accumulators of 16 coordinates, the column of
    y read from LDS in halves -- one launch per batch that requires grad (one in all for ``sym=True``), bit-reproducible, nothing of size
    pairs x M x N allocated.  It takes effect at order 1 on a HIP device where the route above declined, the forward is in the kernel's
    scope (sk_route_query(SK_OP_TRUNCATED)) and every batch that requires grad has path dim 9 to 16, at most 128 steps, at most 128 steps
    on the other side (sk_route_query(SK_OP_TRUNCATED_WIDE_ADJOINT)) and a block's slab of (num_levels - 1) x (steps of the other side +
    lanes - 1) KB within ``workspace_bytes``.  Every other call takes the restatement as a whole, as without the keyword -- at path dim
    <= 8 the route above has taken the call before the keyword is looked at -- and ``sigma`` keeps its gradient either way.  The default
    is False -- every call then does what it did before the keyword existed -- and flipping it is left to a later change."""

    def __init__(self, num_levels, sigma=1., order=1, workspace_bytes=None, static_kernel=None, long_adjoint=False, wide_adjoint=False,
                 points_adjoint=False):
        self.num_levels, self.sigma, self.order, self.workspace_bytes = num_levels, sigma, order, workspace_bytes
        self.static_kernel = static_kernel
        self.points_adjoint = bool(points_adjoint)
        self.long_adjoint = bool(long_adjoint)
        self.wide_adjoint = bool(wide_adjoint)

    def _route_serves(self, route, dx, dy, L, order, paired, sym):
        """the HIP kernel serves the call along `route` (step tensors; the points route: POINT tensors): a HIP device, no empty axis, a
        backend that has what the route needs, the route's forward in scope on (dx, dy) or (dy, dx), and on every side that needs a
        gradient order 1 and the route's adjoint in scope, a block's slab within the workspace.  The plain route also serves calls with no
        gradient pending, at any order; an opt-in route applies only with its keyword, at order 1, with a gradient pending."""
        pending = torch.is_grad_enabled() and (dx.requires_grad or dy.requires_grad)
        if route.switch is not None and not (getattr(self, route.switch) and order == 1 and pending):
            return False
        if not _on_hip(dx) or min(dx.shape[0], dx.shape[1], dy.shape[0], dy.shape[1]) == 0:
            return False
        be = _lib.get_backend()
        if not all(hasattr(be, name) for name in route.needs):
            return False
        (A, M, D), (B, N), es = dx.shape, dy.shape[:2], dx.element_size()
        if be.route(route.op, order, D, M, N, L, False, es) == _lib.ROUTE_STREAM:
            return False
        if pending and order != 1:
            return False
        fits = getattr(be, route.fits)
        if pending and dx.requires_grad and not fits(A, B, M, N, D, L, paired, self.workspace_bytes, es):
            return False
        if pending and dy.requires_grad and not sym and not fits(B, A, N, M, D, L, paired, self.workspace_bytes, es):
            return False
        return True


    def _lifted_levels(self, X, Y, static_kernel, L, order, paired, sym=False):
        """the level terms of the POINTS X, Y under `static_kernel`: the HIP kernel's points mode for an RBFKernel where it serves (a HIP
        device, sk_route_query(SK_OP_TRUNCATED_RBF) on (X, Y) or (Y, X), and no gradient pending -- or points_adjoint=True and
        the _POINTS route serves: _RouteLevels), else the restatement on the lifted G"""
        param = static_kernel.sigma if type(static_kernel) is RBFKernel else None
        if param is not None and not isinstance(param, torch.Tensor) and float(param) > 0 and self._route_serves(_POINTS, X, Y, L, order, paired, sym):
            Xc = X.contiguous()
            return _RouteLevels.apply(Xc, Xc if Y is X else Y.contiguous(), _POINTS, L, order, float(param), paired, sym, self.workspace_bytes)
        if param is not None and _on_hip(X) and not _needs_grad(X, Y, param) and min(X.shape[0], Y.shape[0]) > 0:
            be = _lib.get_backend()
            if hasattr(be, "truncated_levels") and be.route(_lib.OP_TRUNCATED_RBF, order, X.shape[2], X.shape[1], Y.shape[1], L, False,
                                                            X.element_size()) != _lib.ROUTE_STREAM:
                lev = _route_levels(be, _POINTS, X.contiguous(), Y.contiguous(), L, order, float(param), paired, self.workspace_bytes)
                if lev is not None:
                    return lev
        return _truncated_levels_torch(X, Y, L, order, paired, self.workspace_bytes, _lifted_gram(static_kernel))

    def _levels(self, X, Y, paired, sym):
        static_kernel = self.static_kernel
        if static_kernel is not None and _functional(static_kernel):
            fX = static_kernel.features(X)      # function-valued paths: mapped once, as SigKernel does
            X, Y, static_kernel = fX, (fX if Y is X else static_kernel.features(Y)), static_kernel.base_kernel
        L, order = _check_args(X, Y, self.num_levels, self.order)
        if paired and X.shape[0] != Y.shape[0]:
            raise ValueError("X and Y must hold the same number of paths, got %d and %d" % (X.shape[0], Y.shape[0]))
        if sym and Y is not X:
            raise ValueError("sym=True needs Y is X")
        if static_kernel is not None and type(static_kernel) is not LinearKernel:
            return self._lifted_levels(X, Y, static_kernel, L, order, paired, sym)
        dx = X[:, 1:] - X[:, :-1]
        dy = dx if Y is X else Y[:, 1:] - Y[:, :-1]
        # the route every object has; opt-in with a gradient pending: path dims 9 .. 16, then steps beyond the adjoint mode's
        for route in (_PLAIN, _WIDE, _LONG):
            if self._route_serves(route, dx, dy, L, order, paired, sym):
                dx = dx.contiguous()
                return _RouteLevels.apply(dx, dx if dy is dx else dy.contiguous(), route, L, order, None, paired, sym, self.workspace_bytes)
        if _on_hip(dx) and _long_serves(_lib.get_backend(), dx, dy, None, order):     # opt-in: steps beyond the plain launch, no gradient pending
            lev = _long(_lib.get_backend(), dx.contiguous(), dy.contiguous(), L, None, paired, self.workspace_bytes)
            if lev is not None:
                return lev
        return _truncated_levels_torch(dx, dy, L, order, paired, self.workspace_bytes)

    def compute_Gram(self, X, Y, sym=False):
        """X (batch_X, len_x, dim), Y (batch_Y, len_y, dim) -> (batch_X, batch_Y): the truncated kernel of every pair of paths.
        ``sym=True`` needs ``Y is X``; with a gradient it costs one adjoint launch instead of two."""
        return truncated_from_levels(self._levels(X, Y, False, bool(sym)), self.sigma)

    def compute_kernel(self, X, Y):
        """X (batch, len_x, dim), Y (batch, len_y, dim) -> (batch,): the truncated kernel of the pairs (X[i], Y[i])."""
        return truncated_from_levels(self._levels(X, Y, True, False), self.sigma)

    def compute_mmd(self, X, Y):
        """The unbiased MMD^2 of the samples X and Y, SigKernel.compute_mmd's estimator: the means of K_XX and K_YY without their
        diagonals, minus twice the mean of K_XY.  A batch that does not require grad costs no adjoint launch."""
        K_XX = self.compute_Gram(X, X, sym=True)
        K_YY = self.compute_Gram(Y, Y, sym=True)
        K_XY = self.compute_Gram(X, Y)
        K_XX_m = (torch.sum(K_XX) - torch.sum(torch.diag(K_XX))) / (K_XX.shape[0] * (K_XX.shape[0] - 1.))
        K_YY_m = (torch.sum(K_YY) - torch.sum(torch.diag(K_YY))) / (K_YY.shape[0] * (K_YY.shape[0] - 1.))
        return K_XX_m + K_YY_m - 2. * torch.mean(K_XY)
