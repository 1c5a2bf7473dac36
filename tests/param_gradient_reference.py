"""Gradients with respect to the static kernel's own parameters under SigKernel(exact_gradient=True) -- TESTS ONLY.

The yardstick is CPU fp64 torch autograd through exact_gradient_reference.gram_torch (prefix_gradient_reference.prefix_grid_torch for the
prefix calls) with the parameter a tensor: the very numbers the plain double loop computes, differentiated by torch.  A parameter's
gradient is ONE scalar summed over all pairs, so the bar is scaled by the pairs' own terms,

    |got - want| <= GRAD_BAR * sum over pairs p of |d L_p / d theta|,      L_p = sum(go_p * outputs of pair p),

the project's gradient bar (tests/test_gpu_exact_gradient.py) applied where cancellation between pairs can neither hide nor fake an error.

Also here: the shapes the GPU tests and the parent recording share (CASES), a torch.nn.Module static kernel with a learnable coefficient,
and an OracleBackend with the discrete adjoint in all its modes, for the host-logic tests."""
import functools

import numpy as np
import torch

import sigkernel_amd
from fake_backend import OracleBackend
import exact_gradient_reference as R
import prefix_gradient_reference as PR

GRAD_BAR = 1e-9

# name: (D, A, B (0: paired), M, N, d, naive) -- tests/test_gpu_param_gradient.py says what each can break
CASES = {
    "d2": (2, 2, 3, 6, 5, 1, False),
    "d2_naive": (2, 2, 3, 6, 5, 1, True),
    "d7": (7, 2, 3, 5, 70, 0, False),
    "d11": (11, 2, 2, 5, 83, 1, False),
    "d11_paired": (11, 2, 0, 5, 83, 1, False),
    "d20": (20, 2, 3, 4, 6, 1, False),
    "d32": (32, 1, 1, 3, 130, 0, False),
    "d40": (40, 2, 3, 4, 5, 1, False),
}


def walks(seed, batch, length, dim):
    """random walks with steps N(0, 0.25), torch CPU fp64"""
    gen = torch.Generator().manual_seed(seed)
    return torch.cumsum(0.5 * torch.randn(batch, length, dim, generator=gen, dtype=torch.float64), dim=1)


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(X, Y, go, sigma) of a case: walks, random upstream weights (A, B) or (A,), sigma = 0.35 D"""
    D, A, B, M, N, d, naive = CASES[name]
    seed = 1000 + 7 * D + (B == 0)
    X, Y = walks(seed, A, M, D), walks(seed + 1, B if B else A, N, D)
    go = torch.randn((A, B) if B else (A,), generator=torch.Generator().manual_seed(seed + 2), dtype=torch.float64)
    return X, Y, go, 0.35 * D


def per_pair_gradients(outputs, go, pair_dims, thetas):
    """outputs: a differentiable tensor whose first `pair_dims` axes index the pairs; go: its upstream weights.
    -> (want, scale) per theta: want = d sum(go * outputs) / d theta, scale = sum_p |d L_p / d theta| (max over theta's elements)"""
    Lp = (outputs * go).reshape(int(np.prod(outputs.shape[:pair_dims])), -1).sum(dim=1)
    rows = [torch.autograd.grad(Lp[p], thetas, retain_graph=True, allow_unused=True) for p in range(Lp.shape[0])]
    res = []
    for i, th in enumerate(thetas):
        g = torch.stack([torch.zeros_like(th) if r[i] is None else r[i] for r in rows])
        res.append((g.sum(dim=0), float(g.abs().sum(dim=0).max())))
    return res


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """(want d L / d sigma, sum_p |go_p dK_p / d sigma|) of a case by torch autograd through gram_torch, computed once"""
    D, A, B, M, N, d, naive = CASES[name]
    X, Y, go, sigma = case_inputs(name)
    s = torch.tensor(sigma, dtype=torch.float64, requires_grad=True)
    K = R.gram_torch(X, Y, sigkernel_amd.RBFKernel(s), d, naive, paired=B == 0)
    (want, scale), = per_pair_gradients(K, go, 1 if B == 0 else 2, (s,))
    return float(want), scale


def formula_dsigma(X, Y, go, sigma, d, naive=False, paired=False):
    """The formula the HIP kernel's parameter mode implements, in numpy:
        dL/dsigma = sigma^-2 sum_p go_p sum_{m,n} dG_p[m][n] G_p[m][n] r2_p[m][n],   dG = the 4-corner adjoint of W = dK / d inc"""
    X, Y = X.numpy(), Y.numpy()
    Xp, Yp = (X, Y) if paired else (np.repeat(X, Y.shape[0], axis=0), np.tile(Y, (X.shape[0], 1, 1)))
    r2 = ((Xp[:, :, None, :] - Yp[:, None, :, :]) ** 2).sum(-1)
    G = np.exp(-r2 / sigma)
    inc = G[:, 1:, 1:] + G[:, :-1, :-1] - G[:, 1:, :-1] - G[:, :-1, 1:]
    _, W = R.exact_adjoint_batch(inc, d, naive)
    dG = np.zeros_like(G)
    dG[:, 1:, 1:] += W
    dG[:, :-1, :-1] += W
    dG[:, 1:, :-1] -= W
    dG[:, :-1, 1:] -= W
    return float((go.numpy().reshape(-1) * (dG * G * r2).sum((1, 2))).sum() / sigma ** 2)


class LearnableCubic(torch.nn.Module):
    """a static kernel that is a torch.nn.Module: k(x, y) = (1 + c <x, y>)^3 with a learnable coefficient c, and a parameter the kernel
    never uses (its gradient must come back as zeros)"""

    def __init__(self, c=0.5):
        super().__init__()
        self.c = torch.nn.Parameter(torch.tensor(c, dtype=torch.float64))
        self.unused = torch.nn.Parameter(torch.zeros(2, dtype=torch.float64))

    def batch_kernel(self, X, Y):
        return (1. + self.c * torch.bmm(X, Y.transpose(1, 2))) ** 3

    def Gram_matrix(self, X, Y):
        return (1. + self.c * torch.matmul(X[:, None], Y[None].transpose(-1, -2))) ** 3


class ParamExactBackend(OracleBackend):
    """OracleBackend with the discrete adjoint in its plain, ragged (cells) and prefix (sources) modes, through the restatements.  It has
    no static_adjoint_param: a pending parameter takes the generic branch of the host code."""

    def solve_adj(self, inc_c, dyadic, naive=False, flags=0, edges=None, discrete=False, cells=None, sources=None):
        if not discrete:
            assert cells is None and sources is None
            return super().solve_adj(inc_c, dyadic, naive, flags, edges)
        a = inc_c.detach().double().numpy()
        Mc, Nc = a.shape[-2:]
        flat = a.reshape(-1, Mc, Nc)
        if sources is not None:
            assert cells is None and tuple(sources.shape) == tuple(inc_c.shape)
            k, W = PR.source_adjoint_batch(a, sources.detach().double().numpy(), dyadic, naive)
            return torch.from_numpy(np.asarray(k)).to(inc_c.dtype), torch.from_numpy(W).to(inc_c.dtype)
        tab = np.tile(np.array([[Mc, Nc]]), (flat.shape[0], 1)) if cells is None else np.clip(cells.numpy().reshape(-1, 2), 0, [Mc, Nc])
        k, W = np.ones(flat.shape[0]), np.zeros_like(flat)
        for p, (mc, nc) in enumerate(tab):
            if mc > 0 and nc > 0:
                k[p], W[p, :mc, :nc] = R.exact_adjoint(flat[p, :mc, :nc], dyadic, naive)
        return torch.from_numpy(k.reshape(a.shape[:-2])).to(inc_c.dtype), torch.from_numpy(W.reshape(a.shape)).to(inc_c.dtype)
