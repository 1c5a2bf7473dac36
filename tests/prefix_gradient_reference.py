"""The exact adjoint of the discrete solver with a source per coarse node, restated in plain double loops -- TESTS ONLY (fp64, CPU).

Beside exact_gradient_reference.exact_adjoint (same cells, same coefficients, same operand order): for a weighted sum of prefix kernels

    L = sum over a < Mc, b < Nc of S[a][b] K[(a+1) << d][(b+1) << d]

the solver being a linear recursion in K, the adjoint is ONE reverse sweep with each weight injected at its own cell in place of the 1 at
the far corner:

    u[i][j] = src(i, j) + P(g[i][j+1]) u[i][j+1] + P(g[i+1][j]) u[i+1][j] - Q(g[i+1][j+1]) u[i+1][j+1]      (cells outside the grid: dropped)
    src(i, j) = S[((i+1) >> d) - 1][((j+1) >> d) - 1]   if (i+1) and (j+1) are both multiples of 2^d,   else 0
    W[a][b]   = dL / d inc_c[a][b] = 4^-d sum over the fine cells of (a, b) of u[i][j] ((K[i+1][j] + K[i][j+1]) P'(g_ij) - K[i][j] Q'(g_ij))

Row 0 and column 0 of a prefix grid are the constant 1 and carry no gradient: S has the shape of W.

prefix_nodes_torch is the forward loop on torch scalars returning ALL coarse nodes, so that torch autograd differentiates the very grid
the loop computes: the recurrence above is checked against it (tests/test_prefix_gradient_host.py), and the HIP sweep against the
recurrence (tests/test_gpu_prefix_gradient.py)."""
import numpy as np
import torch

from exact_gradient_reference import _coeffs, forward_grid


def source_adjoint(inc_c, S, d, naive=False):
    """inc_c (Mc, Nc), S (Mc, Nc) numpy -> (K[MM][NN], W (Mc, Nc) = d sum(S * coarse nodes) / d inc_c)"""
    inc_c = np.asarray(inc_c, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    Mc, Nc = inc_c.shape
    assert S.shape == (Mc, Nc)
    MM, NN, s, r = Mc << d, Nc << d, 0.25 ** d, 1 << d
    K = forward_grid(inc_c, d, naive)
    g = np.repeat(np.repeat(inc_c, r, axis=0), r, axis=1) * s
    u = np.zeros((MM, NN))
    W = np.zeros((Mc, Nc))
    for i in range(MM - 1, -1, -1):
        for j in range(NN - 1, -1, -1):
            acc = S[((i + 1) >> d) - 1, ((j + 1) >> d) - 1] if (i + 1) % r == 0 and (j + 1) % r == 0 else 0.
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


def source_adjoint_batch(inc_c, S, d, naive=False):
    """inc_c, S (..., Mc, Nc) -> (final (...), W (..., Mc, Nc)), pair by pair"""
    inc_c = np.asarray(inc_c, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    flat, sflat = inc_c.reshape((-1,) + inc_c.shape[-2:]), S.reshape((-1,) + inc_c.shape[-2:])
    res = [source_adjoint(p, q, d, naive) for p, q in zip(flat, sflat)]
    return (np.array([r[0] for r in res]).reshape(inc_c.shape[:-2]), np.stack([r[1] for r in res]).reshape(inc_c.shape))


def prefix_nodes_torch(inc_c, d, naive=False):
    """inc_c (Mc, Nc) torch fp64 (may require grad) -> the coarse nodes (Mc + 1, Nc + 1) of the solver's grid as one torch tensor,
    through the plain double loop: node (m, n) is the kernel of the paths cut after m + 1 and n + 1 points"""
    Mc, Nc = inc_c.shape
    MM, NN, s, r = Mc << d, Nc << d, 0.25 ** d, 1 << d
    one = torch.ones((), dtype=torch.float64)
    K = [[one] * (NN + 1) for _ in range(MM + 1)]
    for i in range(MM):
        for j in range(NN):
            P, Q, _, _ = _coeffs(inc_c[i >> d, j >> d] * s, naive)
            K[i + 1][j + 1] = (K[i + 1][j] + K[i][j + 1]) * P - K[i][j] * Q
    return torch.stack([torch.stack([K[m * r][n * r] for n in range(Nc + 1)]) for m in range(Mc + 1)])


def prefix_grid_torch(X, Y, static_kernel, d, naive=False, paired=False):
    """torch CPU fp64 paths (may require grad) -> the prefix grids (A, B, M, N) ((A, M, N) paired) of the discrete solver, differentiable
    by torch autograd end to end: static kernel in torch, 4-corner increments, prefix_nodes_torch per pair."""
    G = static_kernel.batch_kernel(X, Y) if paired else static_kernel.Gram_matrix(X, Y)
    inc = G[..., 1:, 1:] + G[..., :-1, :-1] - G[..., 1:, :-1] - G[..., :-1, 1:]
    if paired:
        return torch.stack([prefix_nodes_torch(inc[a], d, naive) for a in range(inc.shape[0])])
    return torch.stack([torch.stack([prefix_nodes_torch(inc[a, b], d, naive) for b in range(inc.shape[1])]) for a in range(inc.shape[0])])


def slice_nodes(grid, nodes):
    """the slice `nodes` of prefix grids (..., M, N), as compute_*_prefixes(nodes=...) returns it"""
    if nodes == "all":
        return grid
    if nodes == "diagonal":
        return torch.diagonal(grid, dim1=-2, dim2=-1)
    return grid[..., -1, :] if nodes == "last_row" else grid[..., :, -1]


def mmd_prefixes_torch(X, Y, static_kernel, d, naive=False):
    """compute_mmd_prefixes restated on prefix_grid_torch: (min(len_x, len_y),)"""
    T = min(X.shape[1], Y.shape[1])
    KXX = slice_nodes(prefix_grid_torch(X, X, static_kernel, d, naive), "diagonal")[..., :T]
    KYY = slice_nodes(prefix_grid_torch(Y, Y, static_kernel, d, naive), "diagonal")[..., :T]
    KXY = slice_nodes(prefix_grid_torch(X, Y, static_kernel, d, naive), "diagonal")
    A, B = X.shape[0], Y.shape[0]
    mxx = (KXX.sum(dim=(0, 1)) - torch.diagonal(KXX, dim1=0, dim2=1).sum(dim=-1)) / (A * (A - 1.))
    myy = (KYY.sum(dim=(0, 1)) - torch.diagonal(KYY, dim1=0, dim2=1).sum(dim=-1)) / (B * (B - 1.))
    return mxx + myy - 2. * KXY.mean(dim=(0, 1))
