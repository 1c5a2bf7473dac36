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

``truncated_sig_kernel_paired`` is the same kernel on P pairs ``(X[p], Y[p])``: the same two routes (the HIP kernel in its paired mode, one
pair per lane group; the torch restatement tiled over pairs), the same scope, and nothing of size P x P on either.  It is what
``truncated_sig_kernel(..., normalize=True)`` -- ``K[a, b] / sqrt(k(x_a, x_a) k(y_b, y_b))`` -- takes its two diagonals from.
"""
import ctypes

import numpy as np
import torch

from . import _lib

__all__ = ["truncated_sig_kernel", "truncated_sig_kernel_paired"]

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


def _truncated_block(X, Y, L, sig, order, paired=False):
    """(A, B) of all pairs, or -- paired -- (P,) of the pairs (X[p], Y[p]): everything below G works on its last two axes"""
    G = torch.einsum("pid,pjd->pij", X, Y) if paired else torch.einsum("aid,bjd->abij", X, Y)
    K = sig[0] + sig[1] * G.sum((-2, -1))
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
        K = K + sig[m + 1] * sum(sum(row) for row in R).sum((-2, -1))
    return K


def _truncated_torch(X, Y, num_levels, sigma=1., order=-1, workspace_bytes=None):
    """The recursion in torch ops on the tensors' own device (any device: the tests drive it on the CPU), differentiable; (A, B)."""
    num_levels, order = _check_args(X, Y, num_levels, order)
    sig = _sigma_vector(sigma, num_levels, X.dtype, X.device)
    A, M = X.shape[0], X.shape[1]
    B, N = Y.shape[0], Y.shape[1]
    if A == 0 or B == 0 or M == 0 or N == 0:
        return sig[0] * torch.ones((A, B), dtype=X.dtype, device=X.device)
    d = min(num_levels, order)
    budget = _DEFAULT_WORKSPACE if workspace_bytes is None else int(workspace_bytes)
    per_row = B * M * N * X.element_size() * (2 * d * d + 6) * (num_levels if torch.is_grad_enabled() and (X.requires_grad or Y.requires_grad) else 1)
    rows = int(max(1, min(A, budget // max(1, per_row))))
    return torch.cat([_truncated_block(X[a:a + rows], Y, num_levels, sig, order) for a in range(0, A, rows)], 0)


def _truncated_paired_torch(X, Y, num_levels, sigma=1., order=-1, workspace_bytes=None):
    """The recursion on the P pairs (X[p], Y[p]) in torch ops, differentiable; (P,).  Tiled over pairs: nothing of size P x P."""
    num_levels, order = _check_args(X, Y, num_levels, order)
    if X.shape[0] != Y.shape[0]:
        raise ValueError("X and Y must hold the same number of paths, got %d and %d" % (X.shape[0], Y.shape[0]))
    sig = _sigma_vector(sigma, num_levels, X.dtype, X.device)
    P, M, N = X.shape[0], X.shape[1], Y.shape[1]
    if P == 0 or M == 0 or N == 0:
        return sig[0] * torch.ones((P,), dtype=X.dtype, device=X.device)
    d = min(num_levels, order)
    budget = _DEFAULT_WORKSPACE if workspace_bytes is None else int(workspace_bytes)
    per_pair = M * N * X.element_size() * (2 * d * d + 6) * (num_levels if torch.is_grad_enabled() and (X.requires_grad or Y.requires_grad) else 1)
    pairs = int(max(1, min(P, budget // max(1, per_pair))))
    return torch.cat([_truncated_block(X[p:p + pairs], Y[p:p + pairs], num_levels, sig, order, paired=True) for p in range(0, P, pairs)], 0)


def _truncated_hip(X, Y, num_levels, sig, order, paired=False):
    """(A, B) -- paired: (P,) -- through k_trunc_sig (the body of HipBackend.truncated_gram / truncated_paired, which have asked
    sk_route_query).  X, Y contiguous on a HIP device."""
    A, M, D = X.shape
    B, N = Y.shape[0], Y.shape[1]
    out = torch.empty((A,) if paired else (A, B), dtype=X.dtype, device=X.device)
    if A == 0 or B == 0:
        return out
    fd = 8 if D <= 8 else 16
    Ncp = (N + 15) // 16 * 16
    lib = _lib.load()
    sg = (ctypes.c_double * (num_levels + 1))(*[float(v) for v in sig])
    with _lib._device(X.device):
        Xr, Yt = _lib._prep_pair(X, Y, False, 1.0, M, Ncp, fd)
        if paired:
            fn = getattr(lib, "sk_truncated_paired_" + _lib._suffix(X))
            rc = fn(_lib._ptr(Xr), _lib._ptr(Yt), A, M, M, N, Ncp, D, fd, num_levels, order, sg, _lib._ptr(out), _lib._stream(X))
        else:
            fn = getattr(lib, "sk_truncated_gram_" + _lib._suffix(X))
            rc = fn(_lib._ptr(Xr), _lib._ptr(Yt), A, B, M, M, N, Ncp, D, fd, num_levels, order, sg, _lib._ptr(out), _lib._stream(X))
    _lib._check(rc, "sk_truncated_paired" if paired else "sk_truncated_gram")
    return out


def truncated_route(D, M, N, num_levels, order, elem_size):
    """ROUTE_FUSED / ROUTE_FUSED_SWAP / ROUTE_STREAM (= the torch restatement) for step counts M, N (sk_route_query, csrc/sk_route.hip)."""
    return int(_lib.load().sk_route_query(_lib.OP_TRUNCATED, int(order), int(D), int(M), int(N), int(num_levels), 0, int(elem_size), 0))


def _paired_hip(be, X, Y, num_levels, weights, order, budget):
    """be.truncated_paired on as many pairs at a time as `budget` bytes of staging hold (all of them, usually); None where it says None"""
    P, M, D = X.shape
    fd = 8 if D <= 8 else 16
    per_pair = 8 * fd * (M + (Y.shape[1] + 15) // 16 * 16)
    pairs = int(max(1, min(P, budget // per_pair)))
    parts = []
    for p in range(0, P, pairs):
        k = be.truncated_paired(X[p:p + pairs], Y[p:p + pairs], num_levels, weights, order)
        if k is None:
            return None
        parts.append(k)
    return parts[0] if len(parts) == 1 else torch.cat(parts, 0)


def _stage(X, Y):
    """numpy arrays to the current device; -> (X, Y, whether the result goes back as numpy)"""
    as_numpy = isinstance(X, np.ndarray) or isinstance(Y, np.ndarray)
    if as_numpy:
        X, Y = (t if isinstance(t, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(t)) for t in (X, Y))
        X, Y = X.to("cuda"), Y.to("cuda")
    return X, Y, as_numpy


def _needs_grad(X, Y, sigma):
    return torch.is_grad_enabled() and (X.requires_grad or Y.requires_grad or (isinstance(sigma, torch.Tensor) and sigma.requires_grad))


def truncated_sig_kernel_paired(X, Y, num_levels, sigma=1., order=-1, workspace_bytes=None):
    """The truncated signature kernel of the pairs (X[p], Y[p]): X (P, M, D) and Y (P, N, D) hold STEPS, the result is (P,) with
    ``out[p] = truncated_sig_kernel(X[p:p+1], Y[p:p+1], ...)[0, 0]`` -- the diagonal of the matrix without the matrix.  ``num_levels``,
    ``sigma``, ``order``, the dtypes and numpy in / numpy out are those of truncated_sig_kernel; unequal batch sizes raise ValueError.

    Inside the HIP kernel's scope (the Gram matrix's: sk_route_query(SK_OP_TRUNCATED)) this is ONE launch of k_trunc_sig in its paired mode,
    on (Y, X) when only the second batch fits the lanes.  Inputs that require grad and shapes outside the scope take the differentiable
    torch restatement.  Nothing of size P x P is built on either route, and ``workspace_bytes`` (default 1 GiB) bounds what is: the torch
    route is tiled over pairs by it, and the HIP route's fp64 staging of the paths (8 or 16 doubles per step) is too -- a batch whose
    staging exceeds it goes in several launches."""
    X, Y, as_numpy = _stage(X, Y)
    num_levels, order = _check_args(X, Y, num_levels, order)
    if X.shape[0] != Y.shape[0]:
        raise ValueError("X and Y must hold the same number of paths, got %d and %d" % (X.shape[0], Y.shape[0]))
    X, Y = X.contiguous(), Y.contiguous()
    _lib._dev(X, "X")
    _lib._dev(Y, "Y")
    sig = _sigma_vector(sigma, num_levels, X.dtype, X.device)
    be = _lib.get_backend()
    k = None
    if not _needs_grad(X, Y, sigma) and min(X.shape[0], X.shape[1], Y.shape[1]) > 0 and hasattr(be, "truncated_paired"):
        weights = sig.detach().double().cpu().tolist()
        budget = _DEFAULT_WORKSPACE if workspace_bytes is None else int(workspace_bytes)
        k = _paired_hip(be, X.detach(), Y.detach(), num_levels, weights, order, budget)
        if k is None:       # SK_ROUTE_FUSED_SWAP: k(x, y) = k(y, x) at every order, so the same launch on (Y, X) and nothing to transpose
            k = _paired_hip(be, Y.detach(), X.detach(), num_levels, weights, order, budget)
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
    X, Y, as_numpy = _stage(X, Y)
    num_levels, order = _check_args(X, Y, num_levels, order)
    X, Y = X.contiguous(), Y.contiguous()
    _lib._dev(X, "X")
    _lib._dev(Y, "Y")
    sig = _sigma_vector(sigma, num_levels, X.dtype, X.device)
    needs_grad = _needs_grad(X, Y, sigma)
    be = _lib.get_backend()
    K = None
    if not needs_grad and min(X.shape[0], X.shape[1], Y.shape[0], Y.shape[1]) > 0 and hasattr(be, "truncated_gram"):
        weights = sig.detach().double().cpu().tolist()
        K = be.truncated_gram(X.detach(), Y.detach(), num_levels, weights, order)
        if K is None:       # SK_ROUTE_FUSED_SWAP: only the second batch fits the kernel's lanes -- K(x, y) = K(y, x)^T at every order
            Kt = be.truncated_gram(Y.detach(), X.detach(), num_levels, weights, order)
            K = None if Kt is None else Kt.t().contiguous()
    if K is None:
        K = _truncated_torch(X, Y, num_levels, sig, order, workspace_bytes)
    if normalize:
        kx = _normalizer(truncated_sig_kernel_paired(X, X, num_levels, sig, order, workspace_bytes), "X")
        ky = kx if same else _normalizer(truncated_sig_kernel_paired(Y, Y, num_levels, sig, order, workspace_bytes), "Y")
        K = K / torch.sqrt(kx[:, None] * ky[None, :])
    return K.cpu().numpy() if as_numpy else K
