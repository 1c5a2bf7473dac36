"""Static kernels feeding the signature PDE (the reference's sigkernel/static_kernels.py:11-73).

Duck-typed like the reference: anything with ``batch_kernel(X, Y) -> (A, M, N)`` and
``Gram_matrix(X, Y) -> (A, B, M, N)`` works with :class:`sigkernel_amd.SigKernel`.

The kernels for FUNCTION-VALUED paths (``Linear_ID_Kernel``, ``RBF_ID_Kernel``, ``RBF_CEXP_Kernel``, ``RBF_SQR_Kernel``;
static_kernels.py:76-239) take paths of shape (batch, T, Lx, d): a function of space sampled on Lx points, observed at T times.
Each is a Linear / RBF kernel of a feature map: ``features(X) -> (batch, T, D_eff)`` (differentiable torch) and ``base_kernel``.
:class:`sigkernel_amd.SigKernel` maps its inputs through ``features`` once and runs the base kernel, whose increments are HIP
kernels at any width (beyond 32 dims on the fp64 matrix cores).
"""
import math

import numpy as np
import torch

__all__ = ["LinearKernel", "RBFKernel", "RBF_CEXP_Kernel", "RBF_SQR_Kernel", "Linear_ID_Kernel", "RBF_ID_Kernel", "CEXP",
           "cos_exp_kernel"]


class LinearKernel:
    """Linear kernel k(x, y) = <x, y>."""

    def __init__(self, scale=1.0):
        self.scale = scale

    def batch_kernel(self, X, Y):
        """(A,M,D), (A,N,D) -> (A,M,N); applies scale to both arguments (static_kernels.py:24)."""
        return torch.bmm(self.scale * X, (self.scale * Y).transpose(1, 2))

    def Gram_matrix(self, X, Y):
        """(A,M,D), (B,N,D) -> (A,B,M,N); like the reference this ignores ``scale`` (static_kernels.py:33).

        Same contraction as the reference's ``einsum('ipk,jqk->ijpq')``, issued as one broadcast batched GEMM so
        that the result is produced directly in (A,B,M,N) order (no 34 GB transpose copy at the headline size)."""
        return torch.matmul(X[:, None], Y[None].transpose(-1, -2))


class RBFKernel:
    """RBF kernel k(x, y) = exp(-|x - y|^2 / sigma)  (sigma, not 2 sigma^2: static_kernels.py:56,73)."""

    def __init__(self, sigma):
        self.sigma = sigma

    def batch_kernel(self, X, Y):
        A, M, N = X.shape[0], X.shape[1], Y.shape[1]
        Xs = torch.sum(X ** 2, dim=2)
        Ys = torch.sum(Y ** 2, dim=2)
        dist = -2. * torch.bmm(X, Y.permute(0, 2, 1))
        dist = dist + (torch.reshape(Xs, (A, M, 1)) + torch.reshape(Ys, (A, 1, N)))  # `dist += a + b` in the reference
        return torch.exp(-dist / self.sigma)

    def Gram_matrix(self, X, Y):
        A, B, M, N = X.shape[0], Y.shape[0], X.shape[1], Y.shape[1]
        Xs = torch.sum(X ** 2, dim=2)
        Ys = torch.sum(Y ** 2, dim=2)
        dist = -2. * torch.matmul(X[:, None], Y[None].transpose(-1, -2))   # einsum('ipk,jqk->ijpq') in (A,B,M,N) order
        dist = dist + (torch.reshape(Xs, (A, 1, M, 1)) + torch.reshape(Ys, (1, B, 1, N)))
        return torch.exp(-dist / self.sigma)


def _flat(X):
    """(batch, T, Lx, d) -> (batch, T, Lx * d); a 3-D path stays as it is (static_kernels.py:157-158)."""
    return X.reshape(X.shape[0], X.shape[1], -1)


class RBF_CEXP_Kernel(RBFKernel):
    """RBF kernel with bandwidth sigma2 on the paths passed through the cos-exp integral operator (``CEXP`` with n_freqs frequencies
    and bandwidth sigma1) along the space axis, flattened (static_kernels.py:76-116).  Paths (batch, T, Lx, d)."""

    def __init__(self, sigma1, sigma2, n_freqs):
        self.sigma1 = sigma1
        super().__init__(sigma2)
        self.n_freqs = n_freqs

    def features(self, X):
        """(batch, T, Lx, d) -> (batch, T, Lx * d): CEXP(X), flattened."""
        return _flat(CEXP(X, self.n_freqs, self.sigma1))

    @property
    def base_kernel(self):
        return RBFKernel(self.sigma)

    def batch_kernel(self, X, Y):
        return super().batch_kernel(self.features(X), self.features(Y))

    def Gram_matrix(self, X, Y):
        return super().Gram_matrix(self.features(X), self.features(Y))


class RBF_SQR_Kernel:
    """k(x, y) = exp(-|x - y|^2 / sigma1) * exp(-|x^2 - y^2|^2 / sigma2) on flattened paths (batch, T, Lx, d) (static_kernels.py:118-148).

    Deviation from the reference: its constructor raises NameError (it reads the undefined names ``sigma_1`` / ``sigma_2``); this
    class implements what the reference evidently intends, ``rbf1(X) * rbf2(X ** 2)`` with RBFKernel(sigma1) and RBFKernel(sigma2).
    ``features`` writes the product as one RBF kernel: cat([x / sqrt(sigma1), x^2 / sqrt(sigma2)]) under RBFKernel(1.0) -- the same
    function, evaluated with different rounding."""

    def __init__(self, sigma1, sigma2):
        self.sigma1, self.sigma2 = sigma1, sigma2
        self.rbf1 = RBFKernel(sigma1)
        self.rbf2 = RBFKernel(sigma2)

    def features(self, X):
        X = _flat(X)
        return torch.cat((X / math.sqrt(self.sigma1), X ** 2 / math.sqrt(self.sigma2)), dim=2)

    @property
    def base_kernel(self):
        return RBFKernel(1.0)

    def batch_kernel(self, X, Y):
        X, Y = _flat(X), _flat(Y)
        return self.rbf1.batch_kernel(X, Y) * self.rbf2.batch_kernel(X ** 2, Y ** 2)

    def Gram_matrix(self, X, Y):
        X, Y = _flat(X), _flat(Y)
        return self.rbf1.Gram_matrix(X, Y) * self.rbf2.Gram_matrix(X ** 2, Y ** 2)


class Linear_ID_Kernel(LinearKernel):
    """LinearKernel on the flattened paths: (batch, T, Lx, d) -> (batch, T, Lx * d) (static_kernels.py:150-180)."""

    def __init__(self):
        super().__init__()

    def features(self, X):
        return _flat(X)

    @property
    def base_kernel(self):
        return LinearKernel(self.scale)

    def batch_kernel(self, X, Y):
        return super().batch_kernel(_flat(X), _flat(Y))

    def Gram_matrix(self, X, Y):
        return super().Gram_matrix(_flat(X), _flat(Y))


class RBF_ID_Kernel(RBFKernel):
    """RBFKernel(sigma) on the flattened paths: (batch, T, Lx, d) -> (batch, T, Lx * d) (static_kernels.py:183-213)."""

    def __init__(self, sigma):
        super().__init__(sigma)

    def features(self, X):
        return _flat(X)

    @property
    def base_kernel(self):
        return RBFKernel(self.sigma)

    def batch_kernel(self, X, Y):
        return super().batch_kernel(_flat(X), _flat(Y))

    def Gram_matrix(self, X, Y):
        return super().Gram_matrix(_flat(X), _flat(Y))


def CEXP(X, n_freqs=20, sigma=np.sqrt(10)):
    """The cos-exp integral operator applied along the space axis (static_kernels.py:216-238): X (batch, T, Lx, d), function values on
    an even grid of [0, 1] -> (batch, T, Lx, d).  The operator matrix takes X's dtype (the reference builds it in float64 only, so
    float32 paths fail in its matmul)."""
    length_x = X.shape[2]
    obs_grid = torch.linspace(0, 1, length_x, dtype=torch.float64).to(X.device)
    x_y = obs_grid[:, None] - obs_grid[None, :]
    T_mat = cos_exp_kernel(x_y, n_freqs=n_freqs, sigma=sigma).to(X.dtype)
    cos_exp_X = (1. / length_x) * torch.matmul(X.permute(0, 1, 3, 2), T_mat)
    return cos_exp_X.permute(0, 1, 3, 2)


def cos_exp_kernel(x_y, n_freqs=5, sigma=1):
    """The cos-exp kernel on x_y[i, j] = x_i - y_j (static_kernels.py:240-256):
    sum_{n < n_freqs} cos(2 pi n x_y) * exp(-x_y^2 / sigma)."""
    cos_term = torch.cos(2 * torch.pi * x_y[:, :, None] * torch.arange(n_freqs)[None, None].to(x_y.device)).sum(dim=-1)
    return cos_term * torch.exp(-x_y ** 2 / sigma)
