"""The discrete Goursat solver and its exact adjoint, restated in plain double loops -- TESTS ONLY (fp64, CPU).

Fine cells (i, j), 0 <= i < MM = Mc << d, 0 <= j < NN = Nc << d, with g_ij = inc_c[i >> d][j >> d] * 4^-d; nodes K[0][.] = K[.][0] = 1;

    K[i+1][j+1] = (K[i+1][j] + K[i][j+1]) P(g_ij) - K[i][j] Q(g_ij)
    default: P = 1 + g/2 + g^2/12, Q = 1 - g^2/12;   _naive_solver: P = 1 + g/2, Q = 1

    u[i][j] = dK[MM][NN] / dK[i+1][j+1]:   u[MM-1][NN-1] = 1,
    u[i][j] = P(g[i][j+1]) u[i][j+1] + P(g[i+1][j]) u[i+1][j] - Q(g[i+1][j+1]) u[i+1][j+1]      (cells outside the grid: dropped)
    W[a][b] = dK[MM][NN] / d inc_c[a][b] = 4^-d sum over the fine cells of (a, b) of u[i][j] ((K[i+1][j] + K[i][j+1]) P'(g_ij) - K[i][j] Q'(g_ij))

forward_torch is the same forward loop on torch scalars, so that torch autograd differentiates the very number the loop computes:
the recurrence above is checked against it (tests/test_exact_gradient_host.py), and the HIP sweep against the recurrence."""
import numpy as np
import torch


def _coeffs(g, naive):
    """P, Q, P', Q' of one cell"""
    if naive:
        return 1. + 0.5 * g, 1., 0.5, 0.
    return 1. + 0.5 * g + g * g / 12., 1. - g * g / 12., 0.5 + g / 6., -g / 6.


def forward_grid(inc_c, d, naive=False):
    """inc_c (Mc, Nc) numpy -> the node grid K (MM + 1, NN + 1)"""
    inc_c = np.asarray(inc_c, dtype=np.float64)
    Mc, Nc = inc_c.shape
    MM, NN, s = Mc << d, Nc << d, 0.25 ** d
    K = np.ones((MM + 1, NN + 1))
    for i in range(MM):
        for j in range(NN):
            P, Q, _, _ = _coeffs(inc_c[i >> d, j >> d] * s, naive)
            K[i + 1, j + 1] = (K[i + 1, j] + K[i, j + 1]) * P - K[i, j] * Q
    return K


def exact_adjoint(inc_c, d, naive=False):
    """inc_c (Mc, Nc) numpy -> (K[MM][NN], W (Mc, Nc) = dK[MM][NN] / d inc_c) by the recurrence of the module docstring"""
    inc_c = np.asarray(inc_c, dtype=np.float64)
    Mc, Nc = inc_c.shape
    MM, NN, s = Mc << d, Nc << d, 0.25 ** d
    K = forward_grid(inc_c, d, naive)
    g = np.repeat(np.repeat(inc_c, 1 << d, axis=0), 1 << d, axis=1) * s
    u = np.zeros((MM, NN))
    W = np.zeros((Mc, Nc))
    for i in range(MM - 1, -1, -1):
        for j in range(NN - 1, -1, -1):
            if i == MM - 1 and j == NN - 1:
                u[i, j] = 1.
            else:
                acc = 0.
                if j + 1 < NN:
                    acc += _coeffs(g[i, j + 1], naive)[0] * u[i, j + 1]
                if i + 1 < MM:
                    acc += _coeffs(g[i + 1, j], naive)[0] * u[i + 1, j]
                if i + 1 < MM and j + 1 < NN:
                    acc -= _coeffs(g[i + 1, j + 1], naive)[1] * u[i + 1, j + 1]
                u[i, j] = acc
            _, _, dP, dQ = _coeffs(g[i, j], naive)
            W[i >> d, j >> d] += s * u[i, j] * ((K[i + 1, j] + K[i, j + 1]) * dP - K[i, j] * dQ)
    return K[MM, NN], W


def exact_adjoint_batch(inc_c, d, naive=False):
    """inc_c (..., Mc, Nc) -> (final (...), W (..., Mc, Nc)), pair by pair"""
    inc_c = np.asarray(inc_c, dtype=np.float64)
    flat = inc_c.reshape((-1,) + inc_c.shape[-2:])
    res = [exact_adjoint(p, d, naive) for p in flat]
    return (np.array([r[0] for r in res]).reshape(inc_c.shape[:-2]), np.stack([r[1] for r in res]).reshape(inc_c.shape))


def forward_torch(inc_c, d, naive=False):
    """inc_c (Mc, Nc) torch fp64 (may require grad) -> K[MM][NN] as a torch scalar, through the plain double loop"""
    Mc, Nc = inc_c.shape
    MM, NN, s = Mc << d, Nc << d, 0.25 ** d
    one = torch.ones((), dtype=torch.float64)
    K = [[one] * (NN + 1) for _ in range(MM + 1)]
    for i in range(MM):
        for j in range(NN):
            P, Q, _, _ = _coeffs(inc_c[i >> d, j >> d] * s, naive)
            K[i + 1][j + 1] = (K[i + 1][j] + K[i][j + 1]) * P - K[i][j] * Q
    return K[MM][NN]


def gram_torch(X, Y, static_kernel, d, naive=False, paired=False):
    """torch CPU fp64 paths (may require grad) -> the (A, B) Gram matrix ((A,) paired) of the discrete solver, differentiable by torch
    autograd end to end: static kernel in torch, 4-corner increments, forward_torch per pair."""
    G = static_kernel.batch_kernel(X, Y) if paired else static_kernel.Gram_matrix(X, Y)
    inc = G[..., 1:, 1:] + G[..., :-1, :-1] - G[..., 1:, :-1] - G[..., :-1, 1:]
    if paired:
        return torch.stack([forward_torch(inc[a], d, naive) for a in range(inc.shape[0])])
    return torch.stack([torch.stack([forward_torch(inc[a, b], d, naive) for b in range(inc.shape[1])]) for a in range(inc.shape[0])])


def setup_paths(seed=0):
    """The fixed inputs of the 'reference formula is not the gradient' tests (host and GPU): paths of 6 and 5 points, dim 3, steps
    N(0, 0.25) -- X (2, 6, 3), Y (3, 5, 3) and an upstream gradient w (2, 3), torch CPU fp64."""
    gen = torch.Generator().manual_seed(seed)
    X = torch.cumsum(0.5 * torch.randn(2, 6, 3, generator=gen, dtype=torch.float64), dim=1)
    Y = torch.cumsum(0.5 * torch.randn(3, 5, 3, generator=gen, dtype=torch.float64), dim=1)
    w = torch.randn(2, 3, generator=gen, dtype=torch.float64)
    return X, Y, w
