// sk_pair_sweep.h -- one wavefront solves one pair with its grids stored: the anti-diagonal sweep of sk_simple.hip and the
// stored-grid adjoint built on it, shared with sk_adj_fused_rescue.hip (the fused adjoints' device-side rescue).
#pragma once
#include "sk_internal.h"

namespace sk {
namespace {

#ifndef SK_WAVE_DEFINED
#define SK_WAVE_DEFINED
constexpr int WAVE = 64;
#endif

// (k10 + k01)*(1. + 0.5*g + (1./12)*g**2) - k00*(1. - (1./12)*g**2), cython_backend.pyx:116;
// _naive_solver: (k10 + k01)*(1. + 0.5*g) - k00, cython_backend.pyx:114.
__device__ __forceinline__ double cell_exact(double k10, double k01, double k00, double g, int naive) {
    if (naive) return (k10 + k01) * (1. + 0.5 * g) - k00;
    return (k10 + k01) * ((1. + 0.5 * g) + (1. / 12.) * (g * g)) - k00 * (1. - (1. / 12.) * (g * g));
}

// Sweep one pair.  FLIP selects the doubly flipped increments (the reverse PDE of
// sigkernel.py:438).  `grid` (nullable) receives the full (MM+1)x(NN+1) node grid in the
// sweep's own coordinates; `edges` (nullable) the terminal row and column.
template <typename T, typename TG, bool FLIP>
__device__ double sweep_pair(const T *__restrict__ inc, int64_t ld, int Mc, int Nc, int d, int naive, double *lds,
                             TG *__restrict__ grid, double *__restrict__ edges) {
    const int lane = threadIdx.x;
    const int MM = Mc << d, NN = Nc << d;
    const double rs = 1.0 / (double)(1 << d);  // power of two: multiplying == the reference's division
    double *d0 = lds, *d1 = lds + (MM + 1), *d2 = lds + 2 * (MM + 1);
    const int64_t gw = NN + 1;

    if (grid) {
        for (int j = lane; j <= NN; j += WAVE) grid[j] = (TG)1.;
        for (int i = lane; i <= MM; i += WAVE) grid[(int64_t)i * gw] = (TG)1.;
    }
    if (edges) {
        if (lane == 0) { edges[0] = 1.; edges[NN + 1] = 1.; }
    }
    double last = 1.;
    for (int s = 2; s <= MM + NN; ++s) {
        const int ilo = max(1, s - NN), ihi = min(MM, s - 1);
        for (int i = ilo + lane; i <= ihi; i += WAVE) {
            const int j = s - i;
            const double k10 = (j == 1) ? 1. : d1[i];
            const double k01 = (i == 1) ? 1. : d1[i - 1];
            const double k00 = (i == 1 || j == 1) ? 1. : d0[i - 1];
            int ci = (i - 1) >> d, cj = (j - 1) >> d;
            if (FLIP) { ci = Mc - 1 - ci; cj = Nc - 1 - cj; }
            const double g = ((double)inc[(int64_t)ci * ld + cj] * rs) * rs;
            const double v = cell_exact(k10, k01, k00, g, naive);
            d2[i] = v;
            if (grid) grid[(int64_t)i * gw + j] = (TG)v;
            if (edges) {
                if (i == MM) edges[j] = v;
                if (j == NN) edges[NN + 1 + i] = v;
            }
            if (i == MM && j == NN) last = v;
        }
        __syncthreads();
        double *t = d0; d0 = d1; d1 = d2; d2 = t;
    }
    // broadcast K[MM][NN] (computed by exactly one lane at the last step)
    const int owner = (MM - max(1, MM)) % WAVE;  // lane of i == MM at s == MM+NN: ilo == MM there
    return __shfl(last, owner, WAVE);
}

// Sweep a PIECE of one pair: Nc coarse columns of a grid whose columns to the left have been swept before.  The left boundary comes from
// `col_in` (element i = K at fine row i of the column the piece starts at; element 0 is never read: row 0 is the constant 1) instead of the
// constant 1; the top boundary stays the literal 1.  Every cell is evaluated from the same operands in the same order as in sweep_pair
// over the whole grid, so the piece's cells are the one-shot sweep's bit for bit.  Outputs, fp64: row[j] = K[MM][j] for 1 <= j <= NN,
// col_out[i] = K[i][NN] for 1 <= i <= MM; element 0 of either is NOT written.  col_in and col_out must not overlap (with NN == 1 row
// i + 1 reads col_in[i] one anti-diagonal after row i stored col_out[i]).  The boundary is read from col_in, never from LDS, and every
// LDS word read at j > 1 was written for this pair: what the previous pair of the block left in LDS reaches nothing.
template <typename T>
__device__ void sweep_pair_resume(const T *__restrict__ inc, int64_t ld, int Mc, int Nc, int d, int naive, double *lds,
                                  const double *__restrict__ col_in, double *__restrict__ col_out, double *__restrict__ row) {
    const int lane = threadIdx.x;
    const int MM = Mc << d, NN = Nc << d;
    const double rs = 1.0 / (double)(1 << d);
    double *d0 = lds, *d1 = lds + (MM + 1), *d2 = lds + 2 * (MM + 1);
    for (int s = 2; s <= MM + NN; ++s) {
        const int ilo = max(1, s - NN), ihi = min(MM, s - 1);
        for (int i = ilo + lane; i <= ihi; i += WAVE) {
            const int j = s - i;
            const double k10 = (j == 1) ? col_in[i] : d1[i];
            const double k01 = (i == 1) ? 1. : d1[i - 1];
            const double k00 = (i == 1) ? 1. : (j == 1) ? col_in[i - 1] : d0[i - 1];
            const double g = ((double)inc[(int64_t)((i - 1) >> d) * ld + ((j - 1) >> d)] * rs) * rs;
            const double v = cell_exact(k10, k01, k00, g, naive);
            d2[i] = v;
            if (i == MM) row[j] = v;
            if (j == NN) col_out[i] = v;
        }
        __syncthreads();
        double *t = d0; d0 = d1; d1 = d2; d2 = t;
    }
}

// Robust adjoint of one pair: both solution grids are written to the block's scratch slot, then every
// coarse cell sums its r*r products in the oracle's order (i-major), so W is bit-identical
// to oracle/sigkernel_oracle.c:sk_oracle_adjoint_coarse.
template <typename T>
__device__ void adj_pair(const T *__restrict__ inc, int64_t ld, int Mc, int Nc, int d, int naive, double *lds, double *Kf,
                         double *Kr, T *__restrict__ out_final_p, T *__restrict__ Wp, int64_t ldw) {
    const int MM = Mc << d, NN = Nc << d, r = 1 << d;
    const double rs = 1.0 / (double)r;
    const double v = sweep_pair<T, double, false>(inc, ld, Mc, Nc, d, naive, lds, Kf, nullptr);
    sweep_pair<T, double, true>(inc, ld, Mc, Nc, d, naive, lds, Kr, nullptr);
    __syncthreads();
    if (threadIdx.x == 0 && out_final_p) *out_final_p = (T)v;
    for (int c = threadIdx.x; c < Mc * Nc; c += WAVE) {
        const int a = c / Nc, b = c - a * Nc;
        double acc = 0.;
        for (int ii = 0; ii < r; ++ii)
            for (int jj = 0; jj < r; ++jj) {
                const int i = a * r + ii, j = b * r + jj;
                acc += Kf[(int64_t)i * (NN + 1) + j] * Kr[(int64_t)(MM - 1 - i) * (NN + 1) + (NN - 1 - j)];
            }
        Wp[(int64_t)a * ldw + b] = (T)((acc * rs) * rs);
    }
    __syncthreads();
}

// Coefficients of the stencil K11 = (K10 + K01) P(g) - K00 Q(g) and their derivatives in g.
__device__ __forceinline__ double stencil_p(double g, int naive) { return naive ? 1. + 0.5 * g : (1. + 0.5 * g) + (1. / 12.) * (g * g); }
__device__ __forceinline__ double stencil_q(double g, int naive) { return naive ? 1. : 1. - (1. / 12.) * (g * g); }

// Exact adjoint of the DISCRETE solver for one pair: W = d K[MM][NN] / d inc_c, the derivative of the number sweep_pair returns (adj_pair's
// K * K~ is the continuous PDE's formula, an O(h) approximation of it).  With u[i][j] = d K[MM][NN] / d K[i+1][j+1] on the fine cells:
//   u[MM-1][NN-1] = 1,   u[i][j] = P(g[i][j+1]) u[i][j+1] + P(g[i+1][j]) u[i+1][j] - Q(g[i+1][j+1]) u[i+1][j+1]   (cells outside the grid: dropped)
//   W[a][b] = 4^-d sum over the fine cells of (a, b) of u[i][j] ((K[i+1][j] + K[i][j+1]) P'(g) - K[i][j] Q'(g))
// Phase 1 stores the node grid K (sweep_pair), phase 2 sweeps u over the anti-diagonals from the far corner -- three live diagonals in
// the same 3 (MM + 1) doubles of LDS, indexed by i -- and stores every cell's term to the slot's second grid (row stride NN), phase 3 sums
// each coarse cell's r * r terms in i-major order: no atomics, the same bits on every run.  Every word of both grids that is read was
// written for this pair, and a dropped term is never loaded.
// `src` (nullable, row stride `lds_src`; ADJ_SOURCES of k_adj_simple): the adjoint of L = sum S[a][b] K[(a+1) << d][(b+1) << d] over the coarse
// nodes instead of that of K[MM][NN] alone -- the same sweep with u started at src(i, j) = S[((i+1) >> d) - 1][((j+1) >> d) - 1] where
// (i+1) and (j+1) are both multiples of 2^d, 0 elsewhere, in place of the 1 at the far corner.  `src` may be `Wp` itself (W in/out): every
// source is read in phase 2, every store to Wp is in phase 3, and a barrier closes each diagonal in between -- hence no __restrict__ on Wp.
template <typename T>
__device__ void adj_pair_discrete(const T *__restrict__ inc, int64_t ld, int Mc, int Nc, int d, int naive, double *lds, double *Kf,
                                  double *Tm, T *__restrict__ out_final_p, T *Wp, int64_t ldw, const T *src = nullptr,
                                  int64_t lds_src = 0) {
    const int lane = threadIdx.x;
    const int MM = Mc << d, NN = Nc << d, r = 1 << d;
    const double rs = 1.0 / (double)r;
    const int64_t gw = NN + 1;
    const double v = sweep_pair<T, double, false>(inc, ld, Mc, Nc, d, naive, lds, Kf, nullptr);
    __syncthreads();
    if (lane == 0 && out_final_p) *out_final_p = (T)v;
    double *d0 = lds, *d1 = lds + (MM + 1), *d2 = lds + 2 * (MM + 1);   // diagonals t + 2, t + 1 and t of u
    for (int t = MM + NN - 2; t >= 0; --t) {
        const int ilo = max(0, t - (NN - 1)), ihi = min(MM - 1, t);
        for (int i = ilo + lane; i <= ihi; i += WAVE) {
            const int j = t - i;
            const bool down = i + 1 < MM, right = j + 1 < NN;
            const T *row = inc + (int64_t)(i >> d) * ld, *row1 = inc + (int64_t)((i + 1) >> d) * ld;
            double u = (down || right) ? 0. : 1.;
            if (src) {   // (wave-uniform)
                const bool node = (((i + 1) | (j + 1)) & (r - 1)) == 0;
                u = node ? (double)src[(int64_t)(((i + 1) >> d) - 1) * lds_src + (((j + 1) >> d) - 1)] : 0.;
            }
            if (right) u += stencil_p(((double)row[(j + 1) >> d] * rs) * rs, naive) * d1[i];
            if (down) u += stencil_p(((double)row1[j >> d] * rs) * rs, naive) * d1[i + 1];
            if (down && right) u -= stencil_q(((double)row1[(j + 1) >> d] * rs) * rs, naive) * d0[i + 1];
            d2[i] = u;
        }
        // (a pass of its own: each lane reads back the u it wrote itself, and the two passes' registers do not add up)
        for (int i = ilo + lane; i <= ihi; i += WAVE) {
            const int j = t - i;
            const double g = ((double)inc[(int64_t)(i >> d) * ld + (j >> d)] * rs) * rs;
            const double *kf = Kf + ((int64_t)i * gw + j);
            const double dp = naive ? 0.5 : 0.5 + (1. / 6.) * g, dq = naive ? 0. : -(1. / 6.) * g;
            Tm[(int64_t)i * NN + j] = d2[i] * ((kf[gw] + kf[1]) * dp - kf[0] * dq);
        }
        __syncthreads();
        double *s = d0; d0 = d1; d1 = d2; d2 = s;
    }
    for (int c = lane; c < Mc * Nc; c += WAVE) {
        const int a = c / Nc, b = c - a * Nc;
        double acc = 0.;
        for (int ii = 0; ii < r; ++ii)
            for (int jj = 0; jj < r; ++jj) acc += Tm[(int64_t)(a * r + ii) * NN + (b * r + jj)];
        Wp[(int64_t)a * ldw + b] = (T)((acc * rs) * rs);
    }
    __syncthreads();
}

}  // namespace
}  // namespace sk
