// sk_truncated.hip -- the truncated signature kernel of Kiraly and Oberhauser as ONE sweep of every pair's step grid
// (truncated_sig_kernel, reference sigkernel/transformers.py:201-236, which builds six-dimensional numpy arrays and shifts them with a
// spline filter).
//
// The rows of x (M steps) and y (N steps) are used as they are; G[i][j] = <x_i, y_j>.  Level m of a pair is a set of d x d planes
// R^m[p][q], d = min(m, order):
//     R^1[0][0]     = G
//     R^{m+1}[0][0] = G   sum_{i' < i, j' < j} sum_{p, q} R^m[p][q]                  (2-D exclusive prefix of the level below)
//     R^{m+1}[0][q] = G / (q + 1)   sum_{i' < i} sum_p R^m[p][q - 1]                 (column prefix, same j)
//     R^{m+1}[p][0] = G / (p + 1)   sum_{j' < j} sum_q R^m[p - 1][q]                 (row prefix, same i)
//     R^{m+1}[p][q] = G / ((p + 1)(q + 1))   R^m[p - 1][q - 1]                       (same node)
//     K = sigma[0] + sum_m sigma[m] sum_{nodes, planes} R^m
// Level m + 1 at a node needs level m at nodes <= it only, so ALL LEVELS TRAVEL TOGETHER in one skewed sweep: lane l of a lane group
// owns RC consecutive rows and runs one column behind lane l - 1.  Per level a lane keeps its running row sums (the j' < j prefixes) and
// receives from the lane above, by DPP wave_shr:1, the inclusive column prefixes and the 2-D prefix Q[i][j] = Q[i-1][j] + (row prefix
// of row i up to j).  The planes of a level live only while the node is computed.  Nothing of size pairs x M x N exists anywhere: G is
// formed in the kernel (fd FMAs per node) from the x rows in registers and the y columns in LDS, both staged in fp64 by the prep
// launch the fused solvers use (sk_prep_pair_*, points, fd = 8 or 16).
//
// Pairs: SHARED-Y order, as the fused forward's -- the G = 64 / W lane groups of a wave take rows a = G (q / B) + g of ONE column
// b = q % B, so a wave stages one y block per position q.  Every pair of a launch costs exactly the same (one M, N, level count), so
// the positions are dealt out statically (wave w takes q = w, w + waves, ...): a work counter would have nothing to even out.
// Padding rows and columns have G = 0 and therefore contribute nothing; no lane is ever masked.
// PAIRED mode (TruncParams::paired, launch-time and wave-uniform): a launch of P pairs (x_p, y_p), out[p].  Lane group g of position q
// takes pair p = G q + g and needs ITS OWN y block, at ylds + g fd Ncp: the y blocks of consecutive pairs are consecutive in Yt, so the
// wave stages those of its live groups as one run.  A lane's block never changes during a position, so the lane reads through a pointer
// to it that is formed before the step loop: the loop issues the instructions it issues in Gram mode, where the pointer is ylds itself.
// The launch widens the groups until G fd Ncp doubles fit the wave's 16 KB; lanes beyond the rows of x hold zero rows.
// LEVELS mode (TruncParams::levels, launch-time and wave-uniform, in Gram and paired mode): the pair's level terms k_0 = 1, k_1, .., k_L
// instead of their weighted sum, out[m][pair].  The step loop is the plain launch's, run with the weights (0, .., 0, 1): acc is then
// level L, and the totals of the levels below are the running row sums rowS the loop keeps anyway.  The mode is an epilogue: a sum over
// the lane's rows and the group's butterfly per level, and L + 1 stores per pair where the plain launch has one.
// ADJOINT mode (TruncParams::mode = TR_ADJOINT, launch-time and wave-uniform, the <1, 2> instance only: order 1, fd = 8): the gradient of a weighted
// sum of the pairs' level terms with respect to the rows of x, in Gram and paired mode -- trunc_adjoint below, with loops of its own; the
// forward launches run the step loop they ran.
// POINTS mode (TruncParams::mode = TR_POINTS, launch-time and wave-uniform; order 1; Gram, paired and levels): the kernel of Kiraly and Oberhauser
// lifted through the RBF static kernel -- x and y staged as POINTS, G the second difference of exp(-|x - y|^2 param) on the grid of points,
// evaluated in the sweep: trunc_points below, with a loop of its own, compiled into the <TR_OMAX, 1> instance; the forward launches run
// the step loop they ran.
// POINTS-ADJOINT mode (TruncParams::mode = TR_POINTS_ADJOINT, launch-time and wave-uniform; order 1, fd = 8; Gram and paired): the gradient of a weighted
// sum of the LIFTED kernel's level terms with respect to the points of x -- trunc_points_adjoint below, the two phases of trunc_adjoint on
// the grid of points with the chain rule through kap; hosted by the <TR_OMAX, 1> instance beside trunc_points.
// LONG mode (TruncParams::mode = TR_LONG, launch-time and wave-uniform; order 1, fd = 8 or 16; Gram, paired and levels; forward only): paths of
// any length -- trunc_long below: the rows in bands of 128 with the hand-down of a band's last row carried through HBM, the columns in tiles of
// the y block with the row sums kept in registers; hosted by the <TR_OMAX, 1> instance beside the points modes.
// LONG-ADJOINT mode (TruncParams::mode = TR_LONG_ADJOINT, launch-time and wave-uniform; order 1, fd = 8; Gram and paired): the adjoint mode's gradient on
// paths of any length -- trunc_long_adjoint below: the reverse recursion split as the long mode splits the forward, the forward carries kept
// per band, a reverse carry handed up between the bands; hosted by the <TR_OMAX, 1> instance beside the long mode.
// WIDE-ADJOINT mode (TruncParams::mode = TR_WIDE_ADJOINT, launch-time and wave-uniform; order 1, fd = 16; Gram and paired): the adjoint mode's gradient at
// path dims 9 .. 16 on at most 128 steps -- trunc_wide_adjoint below: trunc_adjoint's two phases with rows and dX of 16 coordinates, the
// column of y read from LDS in halves; hosted by the <TR_OMAX, 1> instance beside the other modes.
// The level loop is unrolled to TR_LMAX with wave-uniform guards (launch-time level count and order); the template holds the LARGEST
// order (1: one plane per level, or TR_OMAX) and the rows per lane.
#include "sk_wave_common.h"

namespace sk {
namespace {

constexpr int TR_LMAX = 8;            // levels the unrolled sweep holds
constexpr int TR_OMAX = 4;            // largest order of the general instance
constexpr int TR_LDS_DOUBLES = 2048;  // y block of a wave: fd x Ncp doubles, 16 KB -- eight single-wave workgroups per CU and more

struct TruncParams {
    const double *Xr;   // [A][Mrows][fd]
    const double *Yt;   // [B][fd][Ncp]
    void *out;          // [A][B], double or float; paired: [A]; levels: [L + 1][A][B], paired [L + 1][A]
    int64_t A, B, n_pos;
    int Mrows, Ncp, fd, M, N, L, order, logW, out_f32;
    int paired;         // 0: the Gram matrix of A x B pairs; 1: the A = B pairs (x_p, y_p), one per lane group
    int levels;         // 0: one weighted value per pair; 1: the pair's L + 1 level terms, one plane of `out` per level
    double sigma[TR_LMAX + 1];
    // ADJOINT mode (order 1, fd = 8: trunc_adjoint below).  `out` is not used.
    int mode;           // a TruncMode (sk_internal.h).  TR_FORWARD: a forward launch; TR_ADJOINT: dX of sum_pairs sum_m w[m][pair] k_m;
                        // TR_POINTS: the POINTS mode, a forward launch on points (below);
                        // TR_POINTS_ADJOINT: TR_ADJOINT for the lifted kernel (slab: L planes, the last one g)
                        // TR_LONG: the LONG mode, a forward launch on any number of steps (trunc_long; slab: [blocks][L - 1][ceil64(N)], the
                        // carry between a pair's row bands)
                        // TR_LONG_ADJOINT: TR_ADJOINT on any number of steps (trunc_long_adjoint; slab per block: the factors of one band,
                        // [N + tiles (W - 1)][L - 1][128], then with more than one band the forward carries [bands][ceil64(N)][L - 1] and the
                        // two halves of the reverse carry [2][ceil64(N)][L - 1])
                        // TR_WIDE_ADJOINT: TR_ADJOINT at fd = 16 (trunc_wide_adjoint; slab and w as there, Tpart [n_chunks][A][M][16])
    int64_t n_chunks;   // Gram: the B pairs of a row tile go to this many positions; paired: 1
    const double *w;    // [L][A][B], paired [L][A]: the weight of level m + 1 of every pair
    double *Tpart;      // [n_chunks][A][M][8]: the chunks' parts of dX, summed by the caller
    double *slab;       // [blocks][L - 1][N + W - 1][128]: a block's prefix factors between its two phases
    // POINTS mode (order 1: trunc_points below); behind everything else, so that no field the other modes read moves
    double param;       // TR_POINTS and its adjoint: one over the RBF kernel's sigma
};

// ADJOINT mode of k_trunc_sig<1, 2> (TruncParams::mode = TR_ADJOINT, launch-time and wave-uniform): the gradient with respect to the rows of x of
//     sum_pairs sum_{m = 1 .. L} w_m(pair) k_m(pair),      k_m = sum_nodes R^m,  R^1 = G,  R^{m+1} = G P^m,  P^m = exclusive 2-D prefix of R^m.
// With Rb^L = w_L and Rb^m = w_m + (exclusive 2-D SUFFIX of G Rb^{m+1}):  dG = sum_m Rb^m P^{m-1} (P^0 = 1),  dx_i = sum_j dG[i][j] y_j.
// Rb needs G and w only, so the reverse sweep is the forward one mirrored; what it needs from the forward are the L - 1 prefix factors
// of every node.  One position therefore runs two phases per pair, a lane keeping its two rows in both:
//   phase 1  the forward step loop without its sums, storing per step t and level s < L - 1 the lane's qin[s] of both rows as they are
//            BEFORE the node joins them (= P^{s+1}) to the block's slab in HBM, slab[(s steps + t) 128 + 2 lane + r]: one store
//            instruction writes 1 KB contiguously;
//   phase 2  steps backwards: lane l runs one column behind lane l + 1, row 1 before row 0, the hand-ups (per level the 2-D suffix of
//            U^m = G Rb^m, mirroring qio) come from the lane below by DPP wave_shl:1 with 0 into a group's last lane, rowT mirrors rowS.
//            Step t of phase 1 is step steps - 1 - t here for EVERY lane, so the lane reads back exactly the 16 bytes it wrote at that
//            step: nothing beyond program order is needed, and the loads are as contiguous as the stores.
// Pairs: a position keeps ONE tile of rows a (G lane groups) and walks a chunk of consecutive b, restaging the y block per b; dX stays in
// registers across the chunk and is stored once, with plain stores, to the chunk's plane of Tpart -- no atomics, and the result does not
// depend on scheduling.  Paired: one pair per lane group with its own y block as in the forward, chunks of one pair.
// Padding rows and columns have G = 0; dG is masked off the columns exactly as g is, and rows beyond M are never stored.
__device__ __forceinline__ void trunc_adjoint(const TruncParams &prm, double *ylds) {
    constexpr int NS = TR_LMAX - 1;
    const int lane = threadIdx.x;
    const int W = 1 << prm.logW, G = WAVE >> prm.logW;
    const int lam = lane & (W - 1), grp = lane >> prm.logW;
    const int N = prm.N, Ncp = prm.Ncp, L = prm.L;
    const int steps = N + W - 1;
    const bool paired = prm.paired != 0;
    const int64_t plane = paired ? prm.A : prm.A * prm.B;
    double2 *slab = reinterpret_cast<double2 *>(prm.slab + (int64_t)blockIdx.x * (L - 1) * steps * 128) + lane;
    for (int64_t pos = blockIdx.x; pos < prm.n_pos; pos += gridDim.x) {
        int64_t a, b0, b1, chunk = 0;
        int nblk = 1;
        if (paired) {
            b0 = pos * G;
            b1 = b0 + 1;
            a = b0 + grp;
            nblk = prm.A - b0 < G ? (int)(prm.A - b0) : G;
        } else {
            const int64_t at = pos / prm.n_chunks;
            chunk = pos - at * prm.n_chunks;
            b0 = chunk * prm.B / prm.n_chunks;
            b1 = (chunk + 1) * prm.B / prm.n_chunks;
            a = at * G + grp;
        }
        const bool live = a < prm.A;
        const double *yl = ylds + ((paired && live) ? grp * 8 * Ncp : 0);
        double xr[2][8], dX[2][8];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int row = lam * 2 + r;
            const bool ok = live && row < prm.M;
            const double *xp = prm.Xr + ((ok ? a : 0) * (int64_t)prm.Mrows + (ok ? row : 0)) * 8;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                xr[r][k] = ok ? xp[k] : 0.0;
                dX[r][k] = 0.0;
            }
        }
        for (int64_t b = b0; b < b1; ++b) {
            __syncthreads();
            {
                const double *yb = prm.Yt + b * (int64_t)8 * Ncp;
                for (int k = lane; k < nblk * 8 * Ncp; k += WAVE) ylds[k] = yb[k];
            }
            double w[TR_LMAX];
#pragma unroll
            for (int m = 0; m < TR_LMAX; ++m) w[m] = (live && m < L) ? prm.w[m * plane + (paired ? a : a * prm.B + b)] : 0.0;
            __syncthreads();
            {   // phase 1
                double rowS[2][NS], qio[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) qio[s] = rowS[0][s] = rowS[1][s] = 0.0;
                for (int t = 0; t < steps; ++t) {
                    const int j = t - lam;
                    const bool act = (unsigned)j < (unsigned)N;
                    const int jc = act ? j : 0;
                    double qin[NS], pf[2][NS], yv[8];
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        const double v = s < L - 1 ? dpp_shr1_zero(qio[s]) : 0.0;
                        qin[s] = lam == 0 ? 0.0 : v;
                    }
#pragma unroll
                    for (int k = 0; k < 8; ++k) yv[k] = yl[k * Ncp + jc];
                    asm volatile("s_waitcnt lgkmcnt(0)"
                                 : "+v"(yv[0]), "+v"(yv[1]), "+v"(yv[2]), "+v"(yv[3]), "+v"(yv[4]), "+v"(yv[5]), "+v"(yv[6]), "+v"(yv[7]));
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
                        double g = 0.0;
#pragma unroll
                        for (int k = 0; k < 8; ++k) g = fma(xr[r][k], yv[k], g);
                        g = act ? g : 0.0;
                        double prev = g;
#pragma unroll
                        for (int s = 0; s < NS; ++s) {
                            pf[r][s] = qin[s];
                            if (s < L - 1) {
                                const double next = g * qin[s];
                                qin[s] = qin[s] + rowS[r][s];
                                rowS[r][s] += prev;
                                prev = next;
                            }
                        }
                    }
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        if (s < L - 1) slab[((int64_t)s * steps + t) * 64] = make_double2(pf[0][s], pf[1][s]);
                        qio[s] = qin[s];
                    }
                }
            }
            {   // phase 2
                double rowT[2][NS], sio[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) sio[s] = rowT[0][s] = rowT[1][s] = 0.0;
                for (int t = steps - 1; t >= 0; --t) {
                    const int j = t - lam;
                    const bool act = (unsigned)j < (unsigned)N;
                    const int jc = act ? j : 0;
                    double sup[NS], yv[8];
                    double2 pf[NS];
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        pf[s] = s < L - 1 ? slab[((int64_t)s * steps + t) * 64] : make_double2(0.0, 0.0);
                        const double v = s < L - 1 ? dpp_shl1(sio[s], 0.0) : 0.0;
                        sup[s] = lam == W - 1 ? 0.0 : v;
                    }
#pragma unroll
                    for (int k = 0; k < 8; ++k) yv[k] = yl[k * Ncp + jc];
                    asm volatile("s_waitcnt lgkmcnt(0)"
                                 : "+v"(yv[0]), "+v"(yv[1]), "+v"(yv[2]), "+v"(yv[3]), "+v"(yv[4]), "+v"(yv[5]), "+v"(yv[6]), "+v"(yv[7]));
#pragma unroll
                    for (int r = 1; r >= 0; --r) {
                        double g = 0.0;
#pragma unroll
                        for (int k = 0; k < 8; ++k) g = fma(xr[r][k], yv[k], g);
                        g = act ? g : 0.0;
                        double rb = 0.0, dG = 0.0;
#pragma unroll
                        for (int m = TR_LMAX; m >= 1; --m)
                            if (m <= L) {
                                rb = m == L ? w[m - 1] : rb;
                                dG = m == 1 ? dG + rb : fma(rb, r ? pf[m > 1 ? m - 2 : 0].y : pf[m > 1 ? m - 2 : 0].x, dG);
                                if (m > 1) {
                                    const int s = m - 2;
                                    const double u = g * rb;
                                    rb = w[s] + sup[s];
                                    sup[s] = sup[s] + rowT[r][s];
                                    rowT[r][s] += u;
                                }
                            }
                        dG = act ? dG : 0.0;
#pragma unroll
                        for (int k = 0; k < 8; ++k) dX[r][k] = fma(dG, yv[k], dX[r][k]);
                    }
#pragma unroll
                    for (int s = 0; s < NS; ++s) sio[s] = sup[s];
                }
            }
        }
        if (live) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int row = lam * 2 + r;
                if (row < prm.M) {
                    double *tp = prm.Tpart + ((chunk * prm.A + a) * prm.M + row) * 8;
#pragma unroll
                    for (int k = 0; k < 8; ++k) tp[k] = dX[r][k];
                }
            }
        }
    }
}

// POINTS mode (TruncParams::mode = TR_POINTS, launch-time and wave-uniform; order 1, two rows per lane, fd = 8 or 16; Gram, paired and levels):
// the forward sweep on the M x N grid of POINTS with G the second difference of kap(x, y) = exp(-|x - y|^2 param).  The pair order, the
// staging, the skew, the hand-downs and both epilogues are the order-1 forward launches'; the loop is this mode's own, and it is compiled
// into k_trunc_sig<TR_OMAX, 1>, not into <1, 2> whose rows-per-lane it shares: the function does not depend on the template arguments, and
// <1, 2> sits at the limit of its scalar registers, where any code beside its step loop moved the plain, paired and levels launches by
// 1 - 4 % (inside the step loop: 12 - 15 %; profiles/truncated_static.txt).  So <1, 2> is the code it was, instruction for instruction, and
// <TR_OMAX, 1>, whose own loops need more registers than this one, carries the mode at 242 VGPRs (241 without).  What differs is how g forms:
//   X(i, c) = -|x_i - y_c|^2 param from differences of coordinates (a common offset of the paths costs no digits), kap = exp_nonpos(X);
//   D(i, c) = kap(i, c) - kap(i, c - 1) is NOT formed by subtracting -- at a wide bandwidth every kap is 1 - small and the difference would
//             keep 1e-16 absolute -- but as kap_low expm1(-|X(i, c) - X(i, c - 1)|), kap_low the one of the two with the smaller exponent
//             left over: the error of D is then 2^-53 |X| / |dX| relative to D (dX is itself a subtraction) -- what subtracting leaves
//             for |X| = O(1), far less where |X| << 1, the wide bandwidth, and nothing is lost where kap << 1;
//   g(i, c) = D(i, c) - D(i - 1, c), zero in row 0, in column 0, in padding rows and off the columns.  A zero row and a zero column in
//             front add nothing to any exclusive prefix, so the recursion below is the one of the steps.  D is rounded once before it is
//             used (no contraction of its product into this subtraction): two equal rows -- a repeated point, a constant path -- then
//             have equal D, bit for bit, and g is exactly 0 as it is for a zero step of the plain kernel.
//   An infinite coordinate makes d2 infinite, not NaN; d2 - d2 is added to X so that it becomes NaN as a NaN coordinate does (kap = 0 for a
//             point at infinity would give finite levels for an inf in y and NaN ones for the same inf in x).
// A lane carries kap and X of column c - 1 for each of its two rows and D of its second row: five doubles.  The row above a lane's first
// row is the lane above, one column ahead: its carried D, read by DPP at the top of the step before it is overwritten, is D(i - 1, c).
__device__ __forceinline__ void trunc_points(const TruncParams &prm, double *ylds) {
    constexpr int NS = TR_LMAX - 1;
    const int lane = threadIdx.x;
    const int W = 1 << prm.logW, G = WAVE >> prm.logW;
    const int lam = lane & (W - 1), grp = lane >> prm.logW;
    const int N = prm.N, Ncp = prm.Ncp, L = prm.L, fd = prm.fd;
    const bool wide = fd > 8;
    const int steps = N + W - 1;
    const bool paired = prm.paired != 0;
    const double nparam = -prm.param;
    for (int64_t pos = blockIdx.x; pos < prm.n_pos; pos += gridDim.x) {
        int64_t a, b;
        int nblk = 1;
        if (paired) {
            b = pos * G;
            a = b + grp;
            nblk = prm.A - b < G ? (int)(prm.A - b) : G;
        } else {
            const int64_t at = pos / prm.B;
            b = pos - at * prm.B;
            a = at * G + grp;
        }
        const bool live = a < prm.A;
        const double *yl = ylds + ((paired && live) ? grp * fd * Ncp : 0);
        __syncthreads();
        {
            const double *yb = prm.Yt + b * (int64_t)fd * Ncp;
            for (int k = lane; k < nblk * fd * Ncp; k += WAVE) ylds[k] = yb[k];
        }
        double xr[2][16];
        bool node[2];       // the row has nodes: not the first point, not padding
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int row = lam * 2 + r;
            const bool ok = live && row < prm.M;
            const double *xp = prm.Xr + ((ok ? a : 0) * (int64_t)prm.Mrows + (ok ? row : 0)) * fd;
#pragma unroll
            for (int k = 0; k < 16; ++k) xr[r][k] = (ok && k < fd) ? xp[k] : 0.0;
            node[r] = ok && row > 0;
        }
        __syncthreads();
        double rowS[2][NS], qio[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) qio[s] = rowS[0][s] = rowS[1][s] = 0.0;
        double acc = 0.0, kc[2] = {0.0, 0.0}, xc[2] = {0.0, 0.0}, dc = 0.0;
        for (int t = 0; t < steps; ++t) {
            const int j = t - lam;
            const bool act = (unsigned)j < (unsigned)N;
            const int jc = act ? j : 0;
            double dup = dpp_shr1_zero(dc);     // D(i - 1, c) of the lane's first row (row 0 of a group: masked below)
            double qin[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const double v = s < L - 1 ? dpp_shr1_zero(qio[s]) : 0.0;
                qin[s] = lam == 0 ? 0.0 : v;
            }
            double yv[16];
#pragma unroll
            for (int k = 0; k < 8; ++k) yv[k] = yl[k * Ncp + jc];
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+v"(yv[0]), "+v"(yv[1]), "+v"(yv[2]), "+v"(yv[3]), "+v"(yv[4]), "+v"(yv[5]), "+v"(yv[6]), "+v"(yv[7]));
            if (wide) {
#pragma unroll
                for (int k = 8; k < 16; ++k) yv[k] = yl[k * Ncp + jc];
                asm volatile("s_waitcnt lgkmcnt(0)"
                             : "+v"(yv[8]), "+v"(yv[9]), "+v"(yv[10]), "+v"(yv[11]), "+v"(yv[12]), "+v"(yv[13]), "+v"(yv[14]), "+v"(yv[15]));
            } else {
#pragma unroll
                for (int k = 8; k < 16; ++k) yv[k] = 0.0;
            }
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                double d2 = 0.0;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const double e = xr[r][k] - yv[k];
                    d2 = fma(e, e, d2);
                }
                if (wide) {
#pragma unroll
                    for (int k = 8; k < 16; ++k) {
                        const double e = xr[r][k] - yv[k];
                        d2 = fma(e, e, d2);
                    }
                }
                const double xn = d2 * nparam + (d2 - d2), kn = exp_nonpos(xn);     // (an infinite d2 -- an inf coordinate -- is NaN, not kap = 0)
                const double dx = xn - xc[r];
                double d;
                {       // rounded ONCE: contracted into g below, the product would stay exact there and rounded in dup, and equal rows give g != 0
#pragma clang fp contract(off)
                    d = (dx <= 0.0 ? kc[r] : -kn) * expm1_nonpos(-__builtin_fabs(dx));
                }
                double g = d - dup;
                g = (act && j > 0 && node[r]) ? g : 0.0;
                kc[r] = kn;
                xc[r] = xn;
                dup = d;        // the next row's row above is this one
                double prev = g;
#pragma unroll
                for (int lv = 1; lv <= TR_LMAX; ++lv)
                    if (lv <= L) {
                        acc = fma(prm.sigma[lv], prev, acc);
                        if (lv < TR_LMAX && lv < L) {
                            const int s = lv - 1;
                            const double next = g * qin[s];
                            qin[s] = qin[s] + rowS[r][s];
                            rowS[r][s] += prev;
                            prev = next;
                        }
                    }
            }
            dc = dup;
#pragma unroll
            for (int s = 0; s < NS; ++s) qio[s] = qin[s];
        }
        for (int off = 1; off < W; off <<= 1) acc += __shfl_xor(acc, off, WAVE);
        if (prm.levels) {       // the weights are (0, .., 0, 1): acc is level L, rowS[.][s] the total of level s + 1
            const int64_t plane = paired ? prm.A : prm.A * prm.B;
            const int64_t o = paired ? a : a * prm.B + b;
            const bool st = lam == 0 && live;
            if (st) {
                if (prm.out_f32) {
                    reinterpret_cast<float *>(prm.out)[o] = 1.0f;
                    reinterpret_cast<float *>(prm.out)[L * plane + o] = (float)acc;
                } else {
                    reinterpret_cast<double *>(prm.out)[o] = 1.0;
                    reinterpret_cast<double *>(prm.out)[L * plane + o] = acc;
                }
            }
#pragma unroll
            for (int s = 0; s < NS; ++s)
                if (s < L - 1) {
                    double v = rowS[0][s] + rowS[1][s];
                    for (int off = 1; off < W; off <<= 1) v += __shfl_xor(v, off, WAVE);
                    if (st) {
                        if (prm.out_f32) reinterpret_cast<float *>(prm.out)[(s + 1) * plane + o] = (float)v;
                        else reinterpret_cast<double *>(prm.out)[(s + 1) * plane + o] = v;
                    }
                }
        } else if (lam == 0 && live) {
            const double v = prm.sigma[0] + acc;
            const int64_t o = paired ? a : a * prm.B + b;
            if (prm.out_f32) reinterpret_cast<float *>(prm.out)[o] = (float)v;
            else reinterpret_cast<double *>(prm.out)[o] = v;
        }
    }
}

// POINTS-ADJOINT mode of k_trunc_sig<TR_OMAX, 1> (TruncParams::mode = TR_POINTS_ADJOINT, launch-time and wave-uniform; order 1, two rows per lane, fd = 8):
// the gradient with respect to the POINTS of x of  sum_pairs sum_m w_m(pair) k_m(pair)  for the lifted kernel of trunc_points.  With dG the
// gradient with respect to g on the nodes (i, c >= 1) -- trunc_adjoint's reverse recursion, word for word -- and zero everywhere else,
//     H(i, c) = dG(i, c) - dG(i, c + 1) - dG(i + 1, c) + dG(i + 1, c + 1)             is the gradient with respect to kap(i, c), and
//     dx_i    = sum_c H(i, c) kap(i, c) (-2 param) (x_i - y_c).
// Row 0 (a path's first point) and column 0 carry no node and DO receive a gradient: the sweep visits them with dG = 0.
// Pairs, chunks, Tpart and the two phases are trunc_adjoint's; what differs:
//   phase 1  is trunc_points' loop without its sums; beside the L - 1 prefix factors it stores the g of both rows as one more plane of the
//            slab (plane L - 1): in phase 2 the lane above has not reached column c yet, so D(i - 1, c) cannot come down by DPP, and a third
//            x row in registers (16 VGPRs and a second exp per node) costs more than 16 bytes of a store that is contiguous anyway;
//   phase 2  reads the factors and g, runs the mirrored recursion, and forms H as the forward's dup / dc mirrored: a lane carries
//            dG(i, c + 1) per row, E(i, c) = dG(i, c) - dG(i, c + 1); row 1 goes first and takes E(i + 1, c), the E of the lane below's first
//            row one step ago, by one DPP wave_shl:1 at the top of the step (0 into a group's last lane); row 0 takes row 1's E of this
//            step.  kap(i, c) is recomputed, one exp_nonpos per node, from the coordinate differences that then carry the gradient.
// The level guards of a step compare against Ls, the level count read through an empty asm at the top of the step: hoisted out of the
// step loops they are seven scalar register pairs per phase that live across the whole function, and this instance already spills scalar
// registers to vector lanes -- with them hoisted the general step loop gained four lane reads a step and orders 2 - 4 lost 1.0 - 1.3 %
// (profiles/truncated_static_adjoint.txt).
__device__ __forceinline__ void trunc_points_adjoint(const TruncParams &prm, double *ylds) {
    constexpr int NS = TR_LMAX - 1;
    const int lane = threadIdx.x;
    const int W = 1 << prm.logW, G = WAVE >> prm.logW;
    const int lam = lane & (W - 1), grp = lane >> prm.logW;
    const int N = prm.N, Ncp = prm.Ncp, L = prm.L;
    const int steps = N + W - 1;
    const bool paired = prm.paired != 0;
    const int64_t plane = paired ? prm.A : prm.A * prm.B;
    const double nparam = -prm.param;
    double2 *slab = reinterpret_cast<double2 *>(prm.slab + (int64_t)blockIdx.x * L * steps * 128) + lane;
    for (int64_t pos = blockIdx.x; pos < prm.n_pos; pos += gridDim.x) {
        int64_t a, b0, b1, chunk = 0;
        int nblk = 1;
        if (paired) {
            b0 = pos * G;
            b1 = b0 + 1;
            a = b0 + grp;
            nblk = prm.A - b0 < G ? (int)(prm.A - b0) : G;
        } else {
            const int64_t at = pos / prm.n_chunks;
            chunk = pos - at * prm.n_chunks;
            b0 = chunk * prm.B / prm.n_chunks;
            b1 = (chunk + 1) * prm.B / prm.n_chunks;
            a = at * G + grp;
        }
        const bool live = a < prm.A;
        const double *yl = ylds + ((paired && live) ? grp * 8 * Ncp : 0);
        double xr[2][8], dX[2][8];
        bool node[2];       // the row has nodes: not the first point, not padding
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int row = lam * 2 + r;
            const bool ok = live && row < prm.M;
            const double *xp = prm.Xr + ((ok ? a : 0) * (int64_t)prm.Mrows + (ok ? row : 0)) * 8;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                xr[r][k] = ok ? xp[k] : 0.0;
                dX[r][k] = 0.0;
            }
            node[r] = ok && row > 0;
        }
        for (int64_t b = b0; b < b1; ++b) {
            __syncthreads();
            {
                const double *yb = prm.Yt + b * (int64_t)8 * Ncp;
                for (int k = lane; k < nblk * 8 * Ncp; k += WAVE) ylds[k] = yb[k];
            }
            double w[TR_LMAX];
#pragma unroll
            for (int m = 0; m < TR_LMAX; ++m) w[m] = (live && m < L) ? prm.w[m * plane + (paired ? a : a * prm.B + b)] : 0.0;
            __syncthreads();
            {   // phase 1: trunc_points' loop
                double rowS[2][NS], qio[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) qio[s] = rowS[0][s] = rowS[1][s] = 0.0;
                double kc[2] = {0.0, 0.0}, xc[2] = {0.0, 0.0}, dc = 0.0;
                for (int t = 0; t < steps; ++t) {
                    int Ls = L;
                    asm volatile("" : "+s"(Ls));      // the level guards of a step are scalar compares of its own
                    const int j = t - lam;
                    const bool act = (unsigned)j < (unsigned)N;
                    const int jc = act ? j : 0;
                    double dup = dpp_shr1_zero(dc);
                    double qin[NS], pf[2][NS], gs[2], yv[8];
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        const double v = s < Ls - 1 ? dpp_shr1_zero(qio[s]) : 0.0;
                        qin[s] = lam == 0 ? 0.0 : v;
                    }
#pragma unroll
                    for (int k = 0; k < 8; ++k) yv[k] = yl[k * Ncp + jc];
                    asm volatile("s_waitcnt lgkmcnt(0)"
                                 : "+v"(yv[0]), "+v"(yv[1]), "+v"(yv[2]), "+v"(yv[3]), "+v"(yv[4]), "+v"(yv[5]), "+v"(yv[6]), "+v"(yv[7]));
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
                        double d2 = 0.0;
#pragma unroll
                        for (int k = 0; k < 8; ++k) {
                            const double e = xr[r][k] - yv[k];
                            d2 = fma(e, e, d2);
                        }
                        const double xn = d2 * nparam + (d2 - d2), kn = exp_nonpos(xn);     // (as trunc_points: inf is NaN)
                        const double dx = xn - xc[r];
                        double d;
                        {       // (as trunc_points: rounded once)
#pragma clang fp contract(off)
                            d = (dx <= 0.0 ? kc[r] : -kn) * expm1_nonpos(-__builtin_fabs(dx));
                        }
                        double g = d - dup;
                        g = (act && j > 0 && node[r]) ? g : 0.0;
                        kc[r] = kn;
                        xc[r] = xn;
                        dup = d;
                        gs[r] = g;
                        double prev = g;
#pragma unroll
                        for (int s = 0; s < NS; ++s) {
                            pf[r][s] = qin[s];
                            if (s < Ls - 1) {
                                const double next = g * qin[s];
                                qin[s] = qin[s] + rowS[r][s];
                                rowS[r][s] += prev;
                                prev = next;
                            }
                        }
                    }
                    dc = dup;
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        if (s < Ls - 1) slab[((int64_t)s * steps + t) * 64] = make_double2(pf[0][s], pf[1][s]);
                        qio[s] = qin[s];
                    }
                    slab[((int64_t)(Ls - 1) * steps + t) * 64] = make_double2(gs[0], gs[1]);
                }
            }
            {   // phase 2
                double rowT[2][NS], sio[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) sio[s] = rowT[0][s] = rowT[1][s] = 0.0;
                double dgn[2] = {0.0, 0.0};     // dG(i, c + 1) of the lane's two rows
                double ec = 0.0;                // E(i, c) of the lane's first row at the column of the step before
                for (int t = steps - 1; t >= 0; --t) {
                    int Ls = L;
                    asm volatile("" : "+s"(Ls));      // the level guards of a step are scalar compares of its own
                    const int j = t - lam;
                    const bool act = (unsigned)j < (unsigned)N;
                    const int jc = act ? j : 0;
                    double sup[NS], yv[8];
                    double2 pf[NS];
                    const double2 gg = slab[((int64_t)(Ls - 1) * steps + t) * 64];
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        pf[s] = s < Ls - 1 ? slab[((int64_t)s * steps + t) * 64] : make_double2(0.0, 0.0);
                        const double v = s < Ls - 1 ? dpp_shl1(sio[s], 0.0) : 0.0;
                        sup[s] = lam == W - 1 ? 0.0 : v;
                    }
                    double eb = dpp_shl1(ec, 0.0);      // E(i + 1, c) of the lane's second row: the lane below was at column c one step ago
                    eb = lam == W - 1 ? 0.0 : eb;
#pragma unroll
                    for (int k = 0; k < 8; ++k) yv[k] = yl[k * Ncp + jc];
                    asm volatile("s_waitcnt lgkmcnt(0)"
                                 : "+v"(yv[0]), "+v"(yv[1]), "+v"(yv[2]), "+v"(yv[3]), "+v"(yv[4]), "+v"(yv[5]), "+v"(yv[6]), "+v"(yv[7]));
#pragma unroll
                    for (int r = 1; r >= 0; --r) {
                        const double g = r ? gg.y : gg.x;
                        double rb = 0.0, dG = 0.0;
#pragma unroll
                        for (int m = TR_LMAX; m >= 1; --m)
                            if (m <= Ls) {
                                rb = m == Ls ? w[m - 1] : rb;
                                dG = m == 1 ? dG + rb : fma(rb, r ? pf[m > 1 ? m - 2 : 0].y : pf[m > 1 ? m - 2 : 0].x, dG);
                                if (m > 1) {
                                    const int s = m - 2;
                                    const double u = g * rb;
                                    rb = w[s] + sup[s];
                                    sup[s] = sup[s] + rowT[r][s];
                                    rowT[r][s] += u;
                                }
                            }
                        dG = (act && j > 0 && node[r]) ? dG : 0.0;
                        const double E = dG - dgn[r];
                        dgn[r] = dG;
                        const double H = E - eb;
                        eb = E;         // the row above's row below is this one
                        double e[8], d2 = 0.0;
#pragma unroll
                        for (int k = 0; k < 8; ++k) {
                            e[k] = xr[r][k] - yv[k];
                            d2 = fma(e[k], e[k], d2);
                        }
                        double cf = (H * exp_nonpos(d2 * nparam)) * (2.0 * nparam);
                        cf = act ? cf : 0.0;
#pragma unroll
                        for (int k = 0; k < 8; ++k) dX[r][k] = fma(cf, e[k], dX[r][k]);
                    }
                    ec = eb;
#pragma unroll
                    for (int s = 0; s < NS; ++s) sio[s] = sup[s];
                }
            }
        }
        if (live) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int row = lam * 2 + r;
                if (row < prm.M) {
                    double *tp = prm.Tpart + ((chunk * prm.A + a) * prm.M + row) * 8;
#pragma unroll
                    for (int k = 0; k < 8; ++k) tp[k] = dX[r][k];
                }
            }
        }
    }
}

// lane `l` (wave-uniform) of v, to every lane
__device__ __forceinline__ double lane_read(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

typedef double trunc_d2 __attribute__((ext_vector_type(2)));       // 16 bytes of LDS as one asm operand

// LONG mode of k_trunc_sig<TR_OMAX, 1> (TruncParams::mode = TR_LONG, launch-time and wave-uniform; order 1, two rows per lane, fd = 8 or 16; Gram,
// paired and levels; forward only): ANY number of steps on either side.  The node's recursion is the order-1 step loop's (phase 1 of
// trunc_adjoint with the sums kept); an order-1 level is G times the exclusive 2-D prefix of the level below, and that prefix splits exactly:
//   ROW BANDS  the rows go 2 W at a time (bands exist only beyond 128 rows: W = 64, one pair per wave; up to 128 rows the lane groups are
//              the plain launch's).  What the last row of a band would hand down at column j -- qin[s] after its node has joined it, the
//              exclusive prefix of level s + 1 at the first row of the next band -- is the CARRY: lane 63 stores it to the block's slab in HBM,
//              slab[s Ns + j] (Ns = ceil64(N); L - 1 planes), and in the next band lane 0 takes it where the other loops put 0.0.  Band 0 of
//              every position takes zeros.  Only the wave that wrote the slab reads it: program order and a vmcnt wait at a band's end are
//              all the ordering there is.  In place: the columns of a band come in 64 at a time, one load per level by all lanes, issued 64
//              steps before their first use (column j is read at step j - 64 at the earliest and overwritten at step j + 63), and lane 0
//              takes its step's value by a lane read -- no load is waited for in the step that uses it.
//              rowS restarts per band; acc runs on; the level totals of the levels mode add up per lane across the bands (in LDS, behind the y tiles).
//   COLUMN TILES  the y block of the wave holds Tc = min(Ncp, 2048 / fd) columns; a longer second side goes tile by tile with rowS kept in
//              registers -- at order 1 nothing else crosses a tile boundary.  The skew is drained at a tile's end and restarted: W - 1 idle
//              steps per tile.
// Padding rows and columns have G = 0, and every carry value a lane can see is finite (columns beyond N are loaded as zeros).
__device__ __forceinline__ void trunc_long(const TruncParams &prm, double *ylds) {
    constexpr int NS = TR_LMAX - 1;
    const int lane = threadIdx.x;
    const int W = 1 << prm.logW, G = WAVE >> prm.logW;
    const int lam = lane & (W - 1), grp = lane >> prm.logW;
    const int N = prm.N, Ncp = prm.Ncp, L = prm.L, fd = prm.fd;
    const bool wide = fd > 8;
    const bool paired = prm.paired != 0;
    const int Tc = Ncp < TR_LDS_DOUBLES / fd ? Ncp : TR_LDS_DOUBLES / fd;
    const int Ns = (N + 63) & ~63;
    const int bands = (prm.M + 2 * W - 1) / (2 * W);
    double *slab = prm.slab + (int64_t)blockIdx.x * (L - 1) * Ns;       // read and written only with more than one band
    // the lane's level totals over the bands (levels mode), behind the y tiles: 14 registers the step loop does not have; no other lane
    // reads them
    double *totl = ylds + (paired ? G : 1) * fd * Tc + lane;
    for (int64_t pos = blockIdx.x; pos < prm.n_pos; pos += gridDim.x) {
        int64_t a, b;
        int nblk = 1;
        if (paired) {
            b = pos * G;
            a = b + grp;
            nblk = prm.A - b < G ? (int)(prm.A - b) : G;
        } else {
            const int64_t at = pos / prm.B;
            b = pos - at * prm.B;
            a = at * G + grp;
        }
        const bool live = a < prm.A;
        const double *yl = ylds + ((paired && live) ? grp * fd * Tc : 0);
        const double *yb = prm.Yt + b * (int64_t)fd * Ncp;
        double rowS[2][NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) totl[s * WAVE] = 0.0;
        double acc = 0.0;
        for (int band = 0; band < bands; ++band) {
            const bool cin = band > 0, cout = band + 1 < bands;
            double xr[2][16];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int row = (band * W + lam) * 2 + r;
                const bool ok = live && row < prm.M;
                const double *xp = prm.Xr + ((ok ? a : 0) * (int64_t)prm.Mrows + (ok ? row : 0)) * fd;
#pragma unroll
                for (int k = 0; k < 16; ++k) xr[r][k] = (ok && k < fd) ? xp[k] : 0.0;
            }
            double qio[NS], cbuf[NS], cnext[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) qio[s] = rowS[0][s] = rowS[1][s] = cbuf[s] = cnext[s] = 0.0;
            for (int c0 = 0; c0 < N; c0 += Tc) {
                const int nt = N - c0 < Tc ? N - c0 : Tc;
                if (cin) {      // the carry of the tile's first 64 columns
#pragma unroll
                    for (int s = 0; s < NS; ++s)
                        if (s < L - 1) cnext[s] = c0 + lane < N ? slab[s * Ns + c0 + lane] : 0.0;
                }
                __syncthreads();
                for (int row = 0; row < nblk * fd; ++row)
                    for (int c = lane; c < Tc; c += WAVE) ylds[row * Tc + c] = c0 + c < Ncp ? yb[(int64_t)row * Ncp + c0 + c] : 0.0;
                __syncthreads();
                const int steps = nt + W - 1;
                for (int t0 = 0; t0 < steps; t0 += 64) {
                    if (cin) {  // the columns t0 .. t0 + 63 of the tile, asked for a chunk ago; ask for the next ones
#pragma unroll
                        for (int s = 0; s < NS; ++s) cbuf[s] = cnext[s];
                        if (t0 + 64 < nt) {
                            const int col = c0 + t0 + 64 + lane;
#pragma unroll
                            for (int s = 0; s < NS; ++s)
                                if (s < L - 1) cnext[s] = col < N ? slab[s * Ns + col] : 0.0;
                        }
                    }
                    const int t1 = t0 + 64 < steps ? t0 + 64 : steps;
                    for (int t = t0; t < t1; ++t) {
                        int Ls = L;
                        asm volatile("" : "+s"(Ls));      // the level guards of a step are scalar compares of its own
                        const int j = t - lam;
                        const bool act = (unsigned)j < (unsigned)nt;
                        const int jc = act ? j : 0;
                        double qin[NS];
#pragma unroll
                        for (int s = 0; s < NS; ++s) {
                            const double v = s < Ls - 1 ? dpp_shr1_zero(qio[s]) : 0.0;
                            const double c = s < Ls - 1 ? lane_read(cbuf[s], t - t0) : 0.0;
                            qin[s] = lam == 0 ? c : v;
                        }
                        // the column of y in two halves of eight: the second half reuses the registers of the first (the sums are the plain loop's, term by term)
                        double yv[8], gr[2] = {0.0, 0.0};
#pragma unroll
                        for (int k = 0; k < 8; ++k) yv[k] = yl[k * Tc + jc];
                        asm volatile("s_waitcnt lgkmcnt(0)"
                                     : "+v"(yv[0]), "+v"(yv[1]), "+v"(yv[2]), "+v"(yv[3]), "+v"(yv[4]), "+v"(yv[5]), "+v"(yv[6]), "+v"(yv[7]));
#pragma unroll
                        for (int r = 0; r < 2; ++r)
#pragma unroll
                            for (int k = 0; k < 8; ++k) gr[r] = fma(xr[r][k], yv[k], gr[r]);
                        if (wide) {
#pragma unroll
                            for (int k = 0; k < 8; ++k) yv[k] = yl[(k + 8) * Tc + jc];
                            asm volatile("s_waitcnt lgkmcnt(0)"
                                         : "+v"(yv[0]), "+v"(yv[1]), "+v"(yv[2]), "+v"(yv[3]), "+v"(yv[4]), "+v"(yv[5]), "+v"(yv[6]), "+v"(yv[7]));
#pragma unroll
                            for (int r = 0; r < 2; ++r)
#pragma unroll
                                for (int k = 0; k < 8; ++k) gr[r] = fma(xr[r][k + 8], yv[k], gr[r]);
                        }
#pragma unroll
                        for (int r = 0; r < 2; ++r) {
                            double g = gr[r];
                            g = act ? g : 0.0;
                            double prev = g;
#pragma unroll
                            for (int lv = 1; lv <= TR_LMAX; ++lv)
                                if (lv <= Ls) {
                                    acc = fma(prm.sigma[lv], prev, acc);
                                    if (lv < TR_LMAX && lv < Ls) {
                                        const int s = lv - 1;
                                        const double next = g * qin[s];
                                        qin[s] = qin[s] + rowS[r][s];
                                        rowS[r][s] += prev;
                                        prev = next;
                                    }
                                }
                        }
                        if (cout && lam == W - 1 && act) {      // more than one band: W = 64, the wave's last lane
#pragma unroll
                            for (int s = 0; s < NS; ++s)
                                if (s < Ls - 1) slab[s * Ns + c0 + j] = qin[s];
                        }
#pragma unroll
                        for (int s = 0; s < NS; ++s) qio[s] = qin[s];
                    }
                }
            }
            {   // (read, wait in one piece, write: the build's hazard lint holds every LDS read of this unit to a full wait)
                double tv[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) tv[s] = totl[s * WAVE];
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(tv[0]), "+v"(tv[1]), "+v"(tv[2]), "+v"(tv[3]), "+v"(tv[4]), "+v"(tv[5]), "+v"(tv[6]));
#pragma unroll
                for (int s = 0; s < NS; ++s) totl[s * WAVE] = tv[s] + (rowS[0][s] + rowS[1][s]);
            }
            // the band's carry is in memory before the next band asks for it
            if (cout) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        for (int off = 1; off < W; off <<= 1) acc += __shfl_xor(acc, off, WAVE);
        if (prm.levels) {       // the weights are (0, .., 0, 1): acc is level L, totl[s] the lane's total of level s + 1
            const int64_t plane = paired ? prm.A : prm.A * prm.B;
            const int64_t o = paired ? a : a * prm.B + b;
            const bool st = lam == 0 && live;
            if (st) {
                if (prm.out_f32) {
                    reinterpret_cast<float *>(prm.out)[o] = 1.0f;
                    reinterpret_cast<float *>(prm.out)[L * plane + o] = (float)acc;
                } else {
                    reinterpret_cast<double *>(prm.out)[o] = 1.0;
                    reinterpret_cast<double *>(prm.out)[L * plane + o] = acc;
                }
            }
#pragma unroll
            for (int s = 0; s < NS; ++s)
                if (s < L - 1) {
                    double v = totl[s * WAVE];
                    for (int off = 1; off < W; off <<= 1) v += __shfl_xor(v, off, WAVE);
                    if (st) {
                        if (prm.out_f32) reinterpret_cast<float *>(prm.out)[(s + 1) * plane + o] = (float)v;
                        else reinterpret_cast<double *>(prm.out)[(s + 1) * plane + o] = v;
                    }
                }
        } else if (lam == 0 && live) {
            const double v = prm.sigma[0] + acc;
            const int64_t o = paired ? a : a * prm.B + b;
            if (prm.out_f32) reinterpret_cast<float *>(prm.out)[o] = (float)v;
            else reinterpret_cast<double *>(prm.out)[o] = v;
        }
    }
}

// LONG-ADJOINT mode of k_trunc_sig<TR_OMAX, 1> (TruncParams::mode = TR_LONG_ADJOINT, launch-time and wave-uniform; order 1, two rows per lane, fd = 8; Gram
// and paired): trunc_adjoint's gradient -- dX of sum_pairs sum_m w_m(pair) k_m(pair) -- on ANY number of steps.  The reverse recursion is the
// forward one mirrored, so it splits as trunc_long splits the forward.  Per pair a block runs 2 bands - 1 JOBS:
//   bands - 1 CARRY jobs (bands 0 .. bands - 2; none with one band): trunc_long's band/tile loop without its sums.  What the last row of band
//              `band` hands down at column j goes to plane band + 1 of the block's forward-carry planes, fcar[band + 1][j][s] -- not in place:
//              every band's incoming carry is needed again below;
//   bands ADJOINT jobs, band = bands - 1 .. 0, each
//     (a) the band's forward sweep again from its stored incoming carry, through the column tiles left to right, storing per step and level
//         s < L - 1 the qin[s] of both rows before the node joins them (phase 1 of trunc_adjoint) to the block's factor slab at step counter u,
//         fac[(u (L - 1) + s) 64 + lane] as double2 -- 1 KB contiguous per store, the levels of a step side by side so that one running
//         address serves them all; u runs through the band's tiles, bsteps = N + tiles (W - 1) steps in all;
//     (b) the mirrored sweep: tiles right to left, steps downwards, u counted back, so that every lane reads the 16 bytes it wrote itself;
//         program order and the vmcnt(0) wait between (a) and (b) are all the ordering there is -- no other wave touches a block's slabs.
//         REVERSE CARRY: what lane 0 hands up at column j -- sup[s] after its node has joined it, the suffix of U^{s+2} over all later rows --
//         with the weight w_{s+1} folded in (below) -- goes to half band & 1 of rcar[2][j][s]; the band above reads the other half, lane W - 1
//         taking it where trunc_adjoint puts 0.0 (the last band: the weights).  It is fetched as trunc_long fetches its carry: one coalesced load per level for 64 steps, issued 64 steps
//         before their first use, and a lane read per step.  rowT stays in registers across the tiles; the skew drains and restarts per tile.
// dX: with one band it stays in registers over the chunk of b and is stored once, as trunc_adjoint's.  With bands a lane's rows change per
// band: at the start of (b) the lane loads its rows of the chunk's plane of Tpart (zeros for the chunk's first b), continues the FMAs on them
// and stores them at the band's end -- load, continue, store with plain stores: the summation order is that of uninterrupted accumulation.
// Pairs, chunks and Tpart are trunc_adjoint's; the lane groups and the y tiles are trunc_long's at fd = 8.  Padding rows and columns have
// G = 0; dG is masked off the columns exactly as g is, rows beyond M are never stored, and every value a lane can see is finite.
__device__ __forceinline__ void trunc_long_adjoint(const TruncParams &prm, double *ylds) {
    constexpr int NS = TR_LMAX - 1;
    const int lane = threadIdx.x;
    const int W = 1 << prm.logW, G = WAVE >> prm.logW;
    const int lam = lane & (W - 1), grp = lane >> prm.logW;
    const int N = prm.N, Ncp = prm.Ncp, L = prm.L;
    const bool paired = prm.paired != 0;
    const int Tc = Ncp < TR_LDS_DOUBLES / 8 ? Ncp : TR_LDS_DOUBLES / 8;
    const int Ns = (N + 63) & ~63;
    // the y tile in LDS: ylds[(k / 2) YS + 2 c + (k & 1)], coordinates in pairs at a constant stride -- a step's column is four 16-byte reads of one address
    constexpr int YS = TR_LDS_DOUBLES / 4;
    const int bands = (prm.M + 2 * W - 1) / (2 * W);
    const int tiles = (N + Tc - 1) / Tc;
    const int64_t bsteps = N + (int64_t)tiles * (W - 1);
    const int64_t plane = paired ? prm.A : prm.A * prm.B;
    const int64_t cplane = (int64_t)(L - 1) * Ns;               // one band's carry: L - 1 planes of ceil64(N)
    const int64_t fsize = (int64_t)(L - 1) * bsteps * 128;      // the factor slab, in doubles
    double *fcar = prm.slab + (int64_t)blockIdx.x * (fsize + (bands > 1 ? (bands + 2) * cplane : 0)) + fsize;    // [bands][Ns][L - 1]
    double *rcar = fcar + bands * cplane;                                                                         // [2][Ns][L - 1]
    double2 *fac = reinterpret_cast<double2 *>(fcar - fsize) + lane + 3 * 64;        // centred on level 3: the levels of a step are immediate offsets
    // what a group's last lane takes from below in (b), behind the y tiles: with a band below the reverse carry of the chunk's 64 steps,
    // rcl[k 8 + s], else the weights of the group's pair, rcl[grp 8 + s] -- every lane reads it with the step's column of y
    double *rcl = ylds + TR_LDS_DOUBLES;
    for (int64_t pos = blockIdx.x; pos < prm.n_pos; pos += gridDim.x) {
        int64_t a, b0, b1, chunk = 0;
        int nblk = 1;
        if (paired) {
            b0 = pos * G;
            b1 = b0 + 1;
            a = b0 + grp;
            nblk = prm.A - b0 < G ? (int)(prm.A - b0) : G;
        } else {
            const int64_t at = pos / prm.n_chunks;
            chunk = pos - at * prm.n_chunks;
            b0 = chunk * prm.B / prm.n_chunks;
            b1 = (chunk + 1) * prm.B / prm.n_chunks;
            a = at * G + grp;
        }
        const bool live = a < prm.A;
        const trunc_d2 *yl = reinterpret_cast<const trunc_d2 *>(ylds) + ((paired && live) ? grp * Tc : 0);      // paired: the groups' tiles side by side, G Tc <= 256
        double *tpl = prm.Tpart + (chunk * prm.A + (live ? a : 0)) * prm.M * 8;      // the lane group's rows of the chunk's plane
        double dX[2][8];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k = 0; k < 8; ++k) dX[r][k] = 0.0;
        for (int64_t b = b0; b < b1; ++b) {
            const double *yb = prm.Yt + b * (int64_t)8 * Ncp;
            for (int job = 0; job < 2 * bands - 1; ++job) {
                const bool keep = job >= bands - 1;             // an adjoint job: (a) stores the factors, then (b)
                const int band = keep ? 2 * bands - 2 - job : job;
                const bool cin = band > 0, rin = band + 1 < bands;
                const double *cinp = fcar + band * cplane;
                double *coutp = fcar + (band + 1) * cplane;     // written by the carry jobs only: band + 1 < bands
                double2 *fp = fac;      // the step's factors: (a) runs it up through the band's tiles, (b) back down
                double xr[2][8];
                bool rok[2];
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const int row = (band * W + lam) * 2 + r;
                    rok[r] = live && row < prm.M;
                    const double *xp = prm.Xr + ((rok[r] ? a : 0) * (int64_t)prm.Mrows + (rok[r] ? row : 0)) * 8;
#pragma unroll
                    for (int k = 0; k < 8; ++k) xr[r][k] = rok[r] ? xp[k] : 0.0;
                }
                {   // the band's forward sweep: trunc_long's loop without its sums
                    double rowS[2][NS], qio[NS], cbuf[NS], cnext[NS];
#pragma unroll
                    for (int s = 0; s < NS; ++s) qio[s] = rowS[0][s] = rowS[1][s] = cbuf[s] = cnext[s] = 0.0;
                    for (int c0 = 0; c0 < N; c0 += Tc) {
                        const int nt = N - c0 < Tc ? N - c0 : Tc;
                        if (cin) {      // the carry of the tile's first 64 columns
#pragma unroll
                            for (int s = 0; s < NS; ++s)
                                if (s < L - 1) cnext[s] = c0 + lane < N ? cinp[(c0 + lane) * (L - 1) + s] : 0.0;
                        }
                        __syncthreads();
                        for (int row = 0; row < nblk * 8; ++row)
                            for (int c = lane; c < Tc; c += WAVE)
                                ylds[((row & 7) >> 1) * YS + ((row >> 3) * Tc + c) * 2 + (row & 1)] = c0 + c < Ncp ? yb[(int64_t)row * Ncp + c0 + c] : 0.0;
                        __syncthreads();
                        const int steps = nt + W - 1;
                        for (int t0 = 0; t0 < steps; t0 += 64) {
                            if (cin) {  // the columns t0 .. t0 + 63 of the tile, asked for a chunk ago; ask for the next ones
#pragma unroll
                                for (int s = 0; s < NS; ++s) cbuf[s] = cnext[s];
                                if (t0 + 64 < nt) {
                                    const int col = c0 + t0 + 64 + lane;
#pragma unroll
                                    for (int s = 0; s < NS; ++s)
                                        if (s < L - 1) cnext[s] = col < N ? cinp[col * (L - 1) + s] : 0.0;
                                }
                            }
                            const int t1 = t0 + 64 < steps ? t0 + 64 : steps;
                            for (int t = t0; t < t1; ++t, fp += (L - 1) * 64) {
                                int Ls = L;
                                asm volatile("" : "+s"(Ls));      // the level guards of a step are scalar compares of its own
                                const int j = t - lam;
                                const bool act = (unsigned)j < (unsigned)nt;
                                const int jc = act ? j : 0;
                                double qin[NS], pf[2][NS], yv[8];
                                trunc_d2 yq[4];
#pragma unroll
                                for (int s = 0; s < NS; ++s) {
                                    const double v = s < Ls - 1 ? dpp_shr1_zero(qio[s]) : 0.0;
                                    const double c = s < Ls - 1 ? lane_read(cbuf[s], t - t0) : 0.0;
                                    qin[s] = lam == 0 ? c : v;
                                }
#pragma unroll
                                for (int k = 0; k < 4; ++k) yq[k] = yl[k * (YS / 2) + jc];
                                // (the wait takes the reads as they land, 16 bytes each: nothing copies a half out before it)
                                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(yq[0]), "+v"(yq[1]), "+v"(yq[2]), "+v"(yq[3]));
#pragma unroll
                                for (int k = 0; k < 4; ++k) {
                                    yv[2 * k] = yq[k].x;
                                    yv[2 * k + 1] = yq[k].y;
                                }
#pragma unroll
                                for (int r = 0; r < 2; ++r) {
                                    double g = 0.0;
#pragma unroll
                                    for (int k = 0; k < 8; ++k) g = fma(xr[r][k], yv[k], g);
                                    g = act ? g : 0.0;
                                    double prev = g;
#pragma unroll
                                    for (int s = 0; s < NS; ++s) {
                                        pf[r][s] = qin[s];
                                        if (s < Ls - 1) {
                                            const double next = g * qin[s];
                                            qin[s] = qin[s] + rowS[r][s];
                                            rowS[r][s] += prev;
                                            prev = next;
                                        }
                                    }
                                }
                                if (keep) {
#pragma unroll
                                    for (int s = 0; s < NS; ++s)
                                        if (s < Ls - 1) fp[(s - 3) * 64] = make_double2(pf[0][s], pf[1][s]);
                                } else if (lam == W - 1 && act) {       // a carry job: more than one band, W = 64, the wave's last lane
#pragma unroll
                                    for (int s = 0; s < NS; ++s)
                                        if (s < Ls - 1) coutp[(c0 + j) * (Ls - 1) + s] = qin[s];
                                }
#pragma unroll
                                for (int s = 0; s < NS; ++s) qio[s] = qin[s];
                            }
                        }
                    }
                }
                // the carry is in memory before the next band asks for it, the factors before (b) does
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (!keep) continue;
                {   // (b): the band's sweep mirrored
                    const double *rinp = rcar + ((band + 1) & 1) * cplane;
                    double *routp = rcar + (band & 1) * cplane;
                    // The hand-ups carry w_{s+1} + (suffix of U^{s+2}), not the suffix alone: Rb^{s+1} is then the hand-up as it arrives, and the
                    // weights below the top one enter once, where trunc_adjoint puts 0.0 -- at the last lane of the last band's group.
                    const int64_t pw = paired ? a : a * prm.B + b;
                    const double wtop = live ? prm.w[(L - 1) * plane + pw] : 0.0;
                    if (!rin && lam == 0) {
#pragma unroll
                        for (int s = 0; s < NS; ++s) rcl[grp * 8 + s] = (live && s < L - 1) ? prm.w[s * plane + pw] : 0.0;
                    }
                    if (bands > 1) {    // the lane's rows change per band: continue on what the chunk has left in its plane of Tpart
#pragma unroll
                        for (int r = 0; r < 2; ++r) {
                            const bool ld = rok[r] && b > b0;
                            const double *tp = tpl + (ld ? (int64_t)((band * W + lam) * 2 + r) * 8 : 0);
#pragma unroll
                            for (int k = 0; k < 8; ++k) dX[r][k] = ld ? tp[k] : 0.0;
                        }
                    }
                    double rowT[2][NS], sio[NS], cnext[NS];
#pragma unroll
                    for (int s = 0; s < NS; ++s) sio[s] = rowT[0][s] = rowT[1][s] = cnext[s] = 0.0;
                    for (int c0 = (tiles - 1) * Tc; c0 >= 0; c0 -= Tc) {
                        const int nt = N - c0 < Tc ? N - c0 : Tc;
                        if (rin) {      // the reverse carry of the tile's last 64 columns, lane k that of column nt - 1 - k
#pragma unroll
                            for (int s = 0; s < NS; ++s)
                                if (s < L - 1) cnext[s] = lane < nt ? rinp[(c0 + nt - 1 - lane) * (L - 1) + s] : 0.0;
                        }
                        __syncthreads();
                        for (int row = 0; row < nblk * 8; ++row)
                            for (int c = lane; c < Tc; c += WAVE)
                                ylds[((row & 7) >> 1) * YS + ((row >> 3) * Tc + c) * 2 + (row & 1)] = c0 + c < Ncp ? yb[(int64_t)row * Ncp + c0 + c] : 0.0;
                        __syncthreads();
                        const int steps = nt + W - 1;
                        for (int t0 = 0; t0 < steps; t0 += 64) {        // t0, tt count the steps of the mirrored sweep: step t = steps - 1 - tt
                            if (rin) {  // lane W - 1 is at column nt - 1 - tt: asked for a chunk ago, to LDS now; ask for the next 64
#pragma unroll
                                for (int s = 0; s < NS; ++s) rcl[lane * 8 + s] = cnext[s];
                                if (t0 + 64 < nt) {
                                    const int col = nt - 1 - (t0 + 64) - lane;
#pragma unroll
                                    for (int s = 0; s < NS; ++s)
                                        if (s < L - 1) cnext[s] = col >= 0 ? rinp[(c0 + col) * (L - 1) + s] : 0.0;
                                }
                            }
                            const int t1 = t0 + 64 < steps ? t0 + 64 : steps;
                            for (int tt = t0; tt < t1; ++tt) {
                                int Ls = L;
                                asm volatile("" : "+s"(Ls));      // the level guards of a step are scalar compares of its own
                                fp -= (L - 1) * 64;
                                const int j = steps - 1 - tt - lam;
                                const bool act = (unsigned)j < (unsigned)nt;
                                const int jc = act ? j : 0;
                                double sup[NS], yv[8], rc[NS];
                                trunc_d2 yq[4], rq[4];
                                double2 pf[NS];
#pragma unroll
                                for (int s = 0; s < NS; ++s) pf[s] = s < Ls - 1 ? fp[(s - 3) * 64] : make_double2(0.0, 0.0);
#pragma unroll
                                for (int k = 0; k < 4; ++k) yq[k] = yl[k * (YS / 2) + jc];
                                const trunc_d2 *rcp = reinterpret_cast<const trunc_d2 *>(rcl + (rin ? tt - t0 : grp) * 8);
#pragma unroll
                                for (int k = 0; k < 4; ++k) rq[k] = rcp[k];
                                asm volatile("s_waitcnt lgkmcnt(0)"
                                             : "+v"(yq[0]), "+v"(yq[1]), "+v"(yq[2]), "+v"(yq[3]), "+v"(rq[0]), "+v"(rq[1]), "+v"(rq[2]), "+v"(rq[3]));
#pragma unroll
                                for (int k = 0; k < 4; ++k) {
                                    yv[2 * k] = yq[k].x;
                                    yv[2 * k + 1] = yq[k].y;
                                    rc[2 * k] = rq[k].x;
                                    if (2 * k + 1 < NS) rc[2 * k + 1] = rq[k].y;
                                }
#pragma unroll
                                for (int s = 0; s < NS; ++s) {
                                    const double v = s < Ls - 1 ? dpp_shl1(sio[s], 0.0) : 0.0;
                                    sup[s] = lam == W - 1 ? rc[s] : v;
                                }
#pragma unroll
                                for (int r = 1; r >= 0; --r) {
                                    double g = 0.0;
#pragma unroll
                                    for (int k = 0; k < 8; ++k) g = fma(xr[r][k], yv[k], g);
                                    g = act ? g : 0.0;
                                    double rb = 0.0, dG = 0.0;
#pragma unroll
                                    for (int m = TR_LMAX; m >= 1; --m)
                                        if (m <= Ls) {
                                            rb = m == Ls ? wtop : rb;
                                            dG = m == 1 ? dG + rb : fma(rb, r ? pf[m > 1 ? m - 2 : 0].y : pf[m > 1 ? m - 2 : 0].x, dG);
                                            if (m > 1) {
                                                const int s = m - 2;
                                                const double uu = g * rb;
                                                rb = sup[s];
                                                sup[s] = sup[s] + rowT[r][s];
                                                rowT[r][s] += uu;
                                            }
                                        }
                                    dG = act ? dG : 0.0;
#pragma unroll
                                    for (int k = 0; k < 8; ++k) dX[r][k] = fma(dG, yv[k], dX[r][k]);
                                }
                                if (cin && lam == 0 && act) {       // a band above: W = 64, the wave's first lane
#pragma unroll
                                    for (int s = 0; s < NS; ++s)
                                        if (s < Ls - 1) routp[(c0 + j) * (Ls - 1) + s] = sup[s];
                                }
#pragma unroll
                                for (int s = 0; s < NS; ++s) sio[s] = sup[s];
                            }
                        }
                    }
                    if (bands > 1) {
#pragma unroll
                        for (int r = 0; r < 2; ++r)
                            if (rok[r]) {
                                double *tp = tpl + (int64_t)((band * W + lam) * 2 + r) * 8;
#pragma unroll
                                for (int k = 0; k < 8; ++k) tp[k] = dX[r][k];
                            }
                    }
                }
                // the reverse carry and the rows of dX are in memory before the next job asks for them
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
        }
        if (bands == 1 && live) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int row = lam * 2 + r;
                if (row < prm.M) {
                    double *tp = tpl + (int64_t)row * 8;
#pragma unroll
                    for (int k = 0; k < 8; ++k) tp[k] = dX[r][k];
                }
            }
        }
    }
}

// WIDE-ADJOINT mode of k_trunc_sig<TR_OMAX, 1> (TruncParams::mode = TR_WIDE_ADJOINT, launch-time and wave-uniform; order 1, two rows per lane, fd = 16;
// Gram and paired): trunc_adjoint's gradient at path dims 9 .. 16, on at most 128 steps.  Pairs, chunks, liveness, the two phases, the slab and
// its indexing, the hand-ups and Tpart (rows of 16 doubles here) are trunc_adjoint's, and so is the arithmetic, operation for operation (a
// batch padded with zero coordinates gives trunc_adjoint's bits).  What differs is what a lane keeps in registers: xr[2][16] and dX[2][16]
// are 128 of its 256, so
//   * the column of y is never there whole: it is read from LDS in two HALVES of eight coordinates, each gone before the next one comes --
//     both halves for g of the two rows, and both halves again for the dX update AFTER the level recursion, when its state is dead: 32 LDS
//     reads a step where a register copy would have 16, beside some 120 fp64 operations;
//   * both phases run LEVEL BY LEVEL with the lane's two rows side by side (rows couple only through a level's hand-down / hand-up, so the
//     level order can be the outer loop): a level's two prefix factors are stored the moment they exist (phase 1) or loaded inside the level
//     (phase 2), and no array of factors or hand-ups exists.
// Written as trunc_adjoint is -- factors and hand-ups fetched at the top of a step, one row's recursion after the other -- the instance
// needed 282 registers, one wave per SIMD for all its modes; as below it stays at 249.
__device__ __forceinline__ void trunc_wide_adjoint(const TruncParams &prm, double *ylds) {
    constexpr int NS = TR_LMAX - 1;
    const int lane = threadIdx.x;
    const int W = 1 << prm.logW, G = WAVE >> prm.logW;
    const int lam = lane & (W - 1), grp = lane >> prm.logW;
    const int N = prm.N, Ncp = prm.Ncp, L = prm.L;
    const int steps = N + W - 1;
    const bool paired = prm.paired != 0;
    const int64_t plane = paired ? prm.A : prm.A * prm.B;
    double2 *slab = reinterpret_cast<double2 *>(prm.slab + (int64_t)blockIdx.x * (L - 1) * steps * 128) + lane;
    for (int64_t pos = blockIdx.x; pos < prm.n_pos; pos += gridDim.x) {
        int64_t a, b0, b1, chunk = 0;
        int nblk = 1;
        if (paired) {
            b0 = pos * G;
            b1 = b0 + 1;
            a = b0 + grp;
            nblk = prm.A - b0 < G ? (int)(prm.A - b0) : G;
        } else {
            const int64_t at = pos / prm.n_chunks;
            chunk = pos - at * prm.n_chunks;
            b0 = chunk * prm.B / prm.n_chunks;
            b1 = (chunk + 1) * prm.B / prm.n_chunks;
            a = at * G + grp;
        }
        const bool live = a < prm.A;
        const double *yl = ylds + ((paired && live) ? grp * 16 * Ncp : 0);
        double xr[2][16], dX[2][16];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int row = lam * 2 + r;
            const bool ok = live && row < prm.M;
            const double *xp = prm.Xr + ((ok ? a : 0) * (int64_t)prm.Mrows + (ok ? row : 0)) * 16;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                xr[r][k] = ok ? xp[k] : 0.0;
                dX[r][k] = 0.0;
            }
        }
        for (int64_t b = b0; b < b1; ++b) {
            __syncthreads();
            {
                const double *yb = prm.Yt + b * (int64_t)16 * Ncp;
                for (int k = lane; k < nblk * 16 * Ncp; k += WAVE) ylds[k] = yb[k];
            }
            double w[TR_LMAX];
#pragma unroll
            for (int m = 0; m < TR_LMAX; ++m) w[m] = (live && m < L) ? prm.w[m * plane + (paired ? a : a * prm.B + b)] : 0.0;
            __syncthreads();
            {   // phase 1
                double rowS[2][NS], qio[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) qio[s] = rowS[0][s] = rowS[1][s] = 0.0;
                for (int t = 0; t < steps; ++t) {
                    const int j = t - lam;
                    const bool act = (unsigned)j < (unsigned)N;
                    const int jc = act ? j : 0;
                    double g[2] = {0.0, 0.0};
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        double yv[8];
#pragma unroll
                        for (int k = 0; k < 8; ++k) yv[k] = yl[(h * 8 + k) * Ncp + jc];
                        asm volatile("s_waitcnt lgkmcnt(0)"
                                     : "+v"(yv[0]), "+v"(yv[1]), "+v"(yv[2]), "+v"(yv[3]), "+v"(yv[4]), "+v"(yv[5]), "+v"(yv[6]), "+v"(yv[7]));
#pragma unroll
                        for (int r = 0; r < 2; ++r)
#pragma unroll
                            for (int k = 0; k < 8; ++k) g[r] = fma(xr[r][h * 8 + k], yv[k], g[r]);
                    }
                    // level by level, row 0 before row 1: a level's two factors are stored as soon as they exist
                    double prev[2] = {act ? g[0] : 0.0, act ? g[1] : 0.0};
                    const double g0 = prev[0], g1 = prev[1];
#pragma unroll
                    for (int s = 0; s < NS; ++s)
                        if (s < L - 1) {
                            const double v = dpp_shr1_zero(qio[s]);
                            const double p0 = lam == 0 ? 0.0 : v;
                            const double p1 = p0 + rowS[0][s];
                            slab[((int64_t)s * steps + t) * 64] = make_double2(p0, p1);
                            qio[s] = p1 + rowS[1][s];
                            rowS[0][s] += prev[0];
                            rowS[1][s] += prev[1];
                            prev[0] = g0 * p0;
                            prev[1] = g1 * p1;
                        }
                }
            }
            {   // phase 2
                double rowT[2][NS], sio[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) sio[s] = rowT[0][s] = rowT[1][s] = 0.0;
                for (int t = steps - 1; t >= 0; --t) {
                    const int j = t - lam;
                    const bool act = (unsigned)j < (unsigned)N;
                    const int jc = act ? j : 0;
                    double g[2] = {0.0, 0.0};
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        double yv[8];
#pragma unroll
                        for (int k = 0; k < 8; ++k) yv[k] = yl[(h * 8 + k) * Ncp + jc];
                        asm volatile("s_waitcnt lgkmcnt(0)"
                                     : "+v"(yv[0]), "+v"(yv[1]), "+v"(yv[2]), "+v"(yv[3]), "+v"(yv[4]), "+v"(yv[5]), "+v"(yv[6]), "+v"(yv[7]));
#pragma unroll
                        for (int r = 0; r < 2; ++r)
#pragma unroll
                            for (int k = 0; k < 8; ++k) g[r] = fma(xr[r][h * 8 + k], yv[k], g[r]);
                    }
                    // level by level downwards, row 1 before row 0: a level's factors and its hand-up live only while the level is computed
                    const double g0 = act ? g[0] : 0.0, g1 = act ? g[1] : 0.0;
                    double rb0 = 0.0, rb1 = 0.0, dG[2] = {0.0, 0.0};
#pragma unroll
                    for (int m = TR_LMAX; m >= 2; --m)
                        if (m <= L) {
                            const int s = m - 2;
                            rb0 = m == L ? w[m - 1] : rb0;
                            rb1 = m == L ? w[m - 1] : rb1;
                            const double2 pf = slab[((int64_t)s * steps + t) * 64];
                            dG[0] = fma(rb0, pf.x, dG[0]);
                            dG[1] = fma(rb1, pf.y, dG[1]);
                            const double v = dpp_shl1(sio[s], 0.0);
                            const double s1 = lam == W - 1 ? 0.0 : v;
                            const double s0 = s1 + rowT[1][s];
                            sio[s] = s0 + rowT[0][s];
                            rowT[1][s] += g1 * rb1;
                            rowT[0][s] += g0 * rb0;
                            rb1 = w[s] + s1;
                            rb0 = w[s] + s0;
                        }
                    dG[0] = act ? dG[0] + (L == 1 ? w[0] : rb0) : 0.0;
                    dG[1] = act ? dG[1] + (L == 1 ? w[0] : rb1) : 0.0;
                    // the column again, a half at a time: the column index is tied to the recursion's results, so the reads cannot be
                    // scheduled above it and no coordinate of y is in a register while the levels' factors and hand-ups are
                    int jd = jc;
                    asm volatile("" : "+v"(jd) : "v"(dG[0]), "v"(dG[1]));
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        double yv[8];
#pragma unroll
                        for (int k = 0; k < 8; ++k) yv[k] = yl[(h * 8 + k) * Ncp + jd];
                        asm volatile("s_waitcnt lgkmcnt(0)"
                                     : "+v"(yv[0]), "+v"(yv[1]), "+v"(yv[2]), "+v"(yv[3]), "+v"(yv[4]), "+v"(yv[5]), "+v"(yv[6]), "+v"(yv[7]));
#pragma unroll
                        for (int r = 0; r < 2; ++r)
#pragma unroll
                            for (int k = 0; k < 8; ++k) dX[r][h * 8 + k] = fma(dG[r], yv[k], dX[r][h * 8 + k]);
                    }
                }
            }
        }
        if (live) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int row = lam * 2 + r;
                if (row < prm.M) {
                    double *tp = prm.Tpart + ((chunk * prm.A + a) * prm.M + row) * 16;
#pragma unroll
                    for (int k = 0; k < 16; ++k) tp[k] = dX[r][k];
                }
            }
        }
    }
}

template <int OM, int RC>
__global__ __launch_bounds__(WAVE) void k_trunc_sig(const TruncParams prm) {
    extern __shared__ __attribute__((aligned(16))) double ylds[];   // [fd][Ncp]; paired: [G][fd][Ncp], one block per lane group
    constexpr int O1 = OM > 1 ? OM - 1 : 1;
    constexpr int NS = TR_LMAX - 1;      // levels that feed a next one
    const int lane = threadIdx.x;
    const int W = 1 << prm.logW, G = WAVE >> prm.logW;
    const int lam = lane & (W - 1), grp = lane >> prm.logW;
    const int N = prm.N, Ncp = prm.Ncp, L = prm.L, ord = prm.order, fd = prm.fd;
    const bool wide = fd > 8;
    const int steps = N + W - 1;
    const bool paired = prm.paired != 0;
    if constexpr (OM == 1 && RC == 2) {
        if (prm.mode != TR_FORWARD) {      // TR_ADJOINT, its own two loops: the forward launches' step loop below is as it was
            trunc_adjoint(prm, ylds);
            return;
        }
    }
    if constexpr (OM > 1) {
        if (prm.mode != TR_FORWARD) {      // the POINTS mode, its adjoint, the LONG mode, its adjoint, and the WIDE-ADJOINT mode: hosted by THIS instance (see trunc_points), so that <1, 2> stays the code it was
            if (prm.mode == TR_WIDE_ADJOINT) trunc_wide_adjoint(prm, ylds);        // (first: of the three placements tried the one the other modes pay least for, profiles/truncated_wide_adjoint.txt)
            else if (prm.mode == TR_POINTS_ADJOINT) trunc_points_adjoint(prm, ylds);
            else if (prm.mode == TR_LONG) trunc_long(prm, ylds);
            else if (prm.mode == TR_POINTS) trunc_points(prm, ylds);
            else trunc_long_adjoint(prm, ylds);        // (TR_LONG_ADJOINT, last: of the placements tried the one that moves the general loop least)
            return;
        }
    }
    for (int64_t pos = blockIdx.x; pos < prm.n_pos; pos += gridDim.x) {
        int64_t a, b;           // the lane group's row of Xr; the first y block the wave stages
        int nblk = 1;           // ... and how many: one per live group in paired mode
        if (paired) {
            b = pos * G;
            a = b + grp;
            nblk = prm.A - b < G ? (int)(prm.A - b) : G;
        } else {
            const int64_t at = pos / prm.B;
            b = pos - at * prm.B;
            a = at * G + grp;
        }
        const bool live = a < prm.A;
        // the y block the lane reads: its group's (a dead group reads block 0, which is always staged)
        const double *yl = ylds + ((paired && live) ? grp * fd * Ncp : 0);
        __syncthreads();
        {
            const double *yb = prm.Yt + b * (int64_t)fd * Ncp;
            for (int k = lane; k < nblk * fd * Ncp; k += WAVE) ylds[k] = yb[k];
        }
        double xr[RC][16];
#pragma unroll
        for (int r = 0; r < RC; ++r) {
            const int row = lam * RC + r;
            const bool ok = live && row < prm.M;
            const double *xp = prm.Xr + ((ok ? a : 0) * (int64_t)prm.Mrows + (ok ? row : 0)) * fd;
#pragma unroll
            for (int k = 0; k < 16; ++k) xr[r][k] = (ok && k < fd) ? xp[k] : 0.0;
        }
        __syncthreads();
        double rowS[RC][NS], rowW[RC][NS][O1], qio[NS], cpio[NS][O1];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            qio[s] = 0.0;
#pragma unroll
            for (int c = 0; c < O1; ++c) cpio[s][c] = 0.0;
#pragma unroll
            for (int r = 0; r < RC; ++r) {
                rowS[r][s] = 0.0;
#pragma unroll
                for (int c = 0; c < O1; ++c) rowW[r][s][c] = 0.0;
            }
        }
        double acc = 0.0;
        // <TR_OMAX, 1> only (<1, 2> is the code it was): its step loop, 7 KB of forward branches around the level and order guards, starts on
        // a cache line.  Where the loop starts moves with every mode compiled in front of it, and orders 3 and 4 follow the offset by 1 %
        // (offset 44 of 64: +0.9 %; 36, the offset before the points-adjoint mode: the time before it; here: profiles/truncated_static_adjoint.txt).
        if constexpr (OM > 1) asm volatile(".p2align 6");
        for (int t = 0; t < steps; ++t) {
            const int j = t - lam;
            const bool act = (unsigned)j < (unsigned)N;
            const int jc = act ? j : 0;
            // what the row above left at this column one step ago; the first lane of a group has no row above
            double qin[NS], cpin[NS][O1];
#pragma unroll
            for (int s = 0; s < NS; ++s)
                if (s < L - 1) {
                    const double v = dpp_shr1_zero(qio[s]);
                    qin[s] = lam == 0 ? 0.0 : v;
#pragma unroll
                    for (int c = 0; c < O1; ++c)
                        if (OM > 1 && c < ord - 1) {
                            const double u = dpp_shr1_zero(cpio[s][c]);
                            cpin[s][c] = lam == 0 ? 0.0 : u;
                        } else cpin[s][c] = 0.0;
                } else {
                    qin[s] = 0.0;
#pragma unroll
                    for (int c = 0; c < O1; ++c) cpin[s][c] = 0.0;
                }
            // the column of y, once for all rows of the lane: the reads go out back to back and are waited for in one piece (the wait
            // carries the values, so nothing that uses them can move above it -- the build's hazard lint holds this unit to that)
            double yv[16];
#pragma unroll
            for (int k = 0; k < 8; ++k) yv[k] = yl[k * Ncp + jc];
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+v"(yv[0]), "+v"(yv[1]), "+v"(yv[2]), "+v"(yv[3]), "+v"(yv[4]), "+v"(yv[5]), "+v"(yv[6]), "+v"(yv[7]));
            if (wide) {
#pragma unroll
                for (int k = 8; k < 16; ++k) yv[k] = yl[k * Ncp + jc];
                asm volatile("s_waitcnt lgkmcnt(0)"
                             : "+v"(yv[8]), "+v"(yv[9]), "+v"(yv[10]), "+v"(yv[11]), "+v"(yv[12]), "+v"(yv[13]), "+v"(yv[14]), "+v"(yv[15]));
            } else {
#pragma unroll
                for (int k = 8; k < 16; ++k) yv[k] = 0.0;
            }
#pragma unroll
            for (int r = 0; r < RC; ++r) {
                double g = 0.0;
#pragma unroll
                for (int k = 0; k < 8; ++k) g = fma(xr[r][k], yv[k], g);
                if (wide) {
#pragma unroll
                    for (int k = 8; k < 16; ++k) g = fma(xr[r][k], yv[k], g);
                }
                g = act ? g : 0.0;
                double prev[OM][OM];
#pragma unroll
                for (int p = 0; p < OM; ++p)
#pragma unroll
                    for (int q = 0; q < OM; ++q) prev[p][q] = 0.0;
                prev[0][0] = g;
#pragma unroll
                for (int lv = 1; lv <= TR_LMAX; ++lv) {
                    if (lv <= L) {
                        const int dm = lv < OM ? lv : OM;               // planes of this level (at most; fewer when order is smaller)
                        const int dn = lv + 1 < OM ? lv + 1 : OM;       // ... of the next
                        double S = 0.0, Cq[OM], Wp[OM];
#pragma unroll
                        for (int p = 0; p < OM; ++p) Cq[p] = Wp[p] = 0.0;
#pragma unroll
                        for (int p = 0; p < OM; ++p)
#pragma unroll
                            for (int q = 0; q < OM; ++q)
                                if (p < dm && q < dm) {
                                    S += prev[p][q];
                                    Cq[q] += prev[p][q];
                                    Wp[p] += prev[p][q];
                                }
                        acc = fma(prm.sigma[lv], S, acc);
                        if (lv < TR_LMAX && lv < L) {
                            const int s = lv - 1;
                            double next[OM][OM];
#pragma unroll
                            for (int p = 0; p < OM; ++p)
#pragma unroll
                                for (int q = 0; q < OM; ++q) {
                                    double v = 0.0;
                                    if (p < dn && q < dn) {
                                        if (p == 0 && q == 0) v = g * qin[s];
                                        else if (p == 0) v = (g * (1.0 / (q + 1))) * cpin[s][q > 0 ? q - 1 : 0];
                                        else if (q == 0) v = (g * (1.0 / (p + 1))) * rowW[r][s][p > 0 ? p - 1 : 0];
                                        else v = (g * (1.0 / ((p + 1) * (q + 1)))) * prev[p > 0 ? p - 1 : 0][q > 0 ? q - 1 : 0];
                                        v = (p < ord && q < ord) ? v : 0.0;
                                    }
                                    next[p][q] = v;
                                }
                            // this node joins the sums of its level: Q[i][j] for the row below, the row prefixes for column j + 1
                            qin[s] = qin[s] + rowS[r][s];
                            rowS[r][s] += S;
#pragma unroll
                            for (int c = 0; c < O1; ++c)
                                if (OM > 1 && c < dn - 1) {
                                    cpin[s][c] += Cq[c];
                                    rowW[r][s][c] += Wp[c];
                                }
#pragma unroll
                            for (int p = 0; p < OM; ++p)
#pragma unroll
                                for (int q = 0; q < OM; ++q) prev[p][q] = next[p][q];
                        }
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                qio[s] = qin[s];
#pragma unroll
                for (int c = 0; c < O1; ++c) cpio[s][c] = cpin[s][c];
            }
        }
        // the pair's total: a butterfly over the lanes of the group, the same order on every call
        for (int off = 1; off < W; off <<= 1) acc += __shfl_xor(acc, off, WAVE);
        if (prm.levels) {
            // LEVELS mode: the weights are (0, .., 0, 1), so acc is level L; the total of level s + 1 < L is what the rows' running
            // sums rowS[.][s] hold after the last step.  The same butterfly per level, then plane m of the output takes level m.
            const int64_t plane = paired ? prm.A : prm.A * prm.B;
            const int64_t o = paired ? a : a * prm.B + b;
            const bool st = lam == 0 && live;
            if (st) {
                if (prm.out_f32) {
                    reinterpret_cast<float *>(prm.out)[o] = 1.0f;
                    reinterpret_cast<float *>(prm.out)[L * plane + o] = (float)acc;
                } else {
                    reinterpret_cast<double *>(prm.out)[o] = 1.0;
                    reinterpret_cast<double *>(prm.out)[L * plane + o] = acc;
                }
            }
#pragma unroll
            for (int s = 0; s < NS; ++s)
                if (s < L - 1) {
                    double v = rowS[0][s];
#pragma unroll
                    for (int r = 1; r < RC; ++r) v += rowS[r][s];
                    for (int off = 1; off < W; off <<= 1) v += __shfl_xor(v, off, WAVE);
                    if (st) {
                        if (prm.out_f32) reinterpret_cast<float *>(prm.out)[(s + 1) * plane + o] = (float)v;
                        else reinterpret_cast<double *>(prm.out)[(s + 1) * plane + o] = v;
                    }
                }
        } else if (lam == 0 && live) {
            const double v = prm.sigma[0] + acc;
            const int64_t o = paired ? a : a * prm.B + b;
            if (prm.out_f32) reinterpret_cast<float *>(prm.out)[o] = (float)v;
            else reinterpret_cast<double *>(prm.out)[o] = v;
        }
    }
}

inline int trunc_fd(int D) { return D <= 8 ? 8 : 16; }
inline int trunc_order(int L, int order) { return (order < 1 || order > L) ? L : order; }

// log2 of the lanes of a pair's group: the power of two that holds `lanes`.  paired: every lane group of a wave keeps a y block of its own
// -- fewer, wider groups until they fit (one group always does)
inline int trunc_logw(int lanes, int fd, int Ncp, int paired) {
    int logW = 0;
    while ((1 << logW) < lanes) ++logW;
    while (paired && (int64_t)(WAVE >> logW) * fd * Ncp > TR_LDS_DOUBLES) ++logW;
    return logW;
}

// THE one place a launch's TruncParams is filled, whatever the mode: the shape and the flags; sigma[] -- one-hot at L in levels mode, else
// the caller's L + 1 weights, all zero where there are none (the adjoint modes); the adjoint modes' pointers.  logW and n_pos come from the
// launcher's plan.
TruncParams trunc_params(int mode, const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int M, int N, int Ncp, int fd, int L,
                         int order, int paired, double param, void *out, bool out_f32, int levels, const double *sigma, int64_t n_chunks,
                         const double *w, double *Tpart, double *slab) {
    TruncParams prm;
    prm.Xr = Xr; prm.Yt = Yt; prm.out = out;
    prm.A = A; prm.B = B; prm.n_pos = 0;
    prm.Mrows = Mrows; prm.Ncp = Ncp; prm.fd = fd; prm.M = M; prm.N = N; prm.L = L;
    prm.order = order; prm.logW = 0;
    prm.out_f32 = out_f32;
    prm.paired = paired != 0;
    prm.levels = levels != 0;
    for (int m = 0; m <= TR_LMAX; ++m) prm.sigma[m] = levels ? (m == L ? 1.0 : 0.0) : (sigma && m <= L ? sigma[m] : 0.0);
    prm.mode = mode; prm.n_chunks = n_chunks; prm.w = w; prm.Tpart = Tpart; prm.slab = slab;
    prm.param = param;
    return prm;
}

}  // namespace

// THE scope of the kernel (the SK_OP_TRUNCATED rule of sk_route_query): rows of the FIRST batch per pair M, columns N, path dim D.
// order 1: two rows per lane, M <= 128; orders 2 .. 4: one row per lane, M <= 64 (seven levels of row sums and hand-downs, three
// plane columns each, fill the 256 registers two waves per SIMD leave a lane); the y block of a wave, fd x ceil16(N) doubles, in 16 KB.
bool truncated_in_scope(int D, int M, int N, int L, int order) {
    if (D < 1 || D > 16 || M < 1 || N < 1 || L < 1 || L > TR_LMAX) return false;
    const int o = trunc_order(L, order);
    if (o > TR_OMAX) return false;
    if (M > (o == 1 ? 128 : 64)) return false;
    return (int64_t)trunc_fd(D) * ((N + 15) / 16 * 16) <= TR_LDS_DOUBLES;
}

// THE scope of the points mode (the SK_OP_TRUNCATED_RBF rule of sk_route_query): M and N are POINTS, the rows and columns of the sweep, so
// the rule is the one above on them, at order 1 only -- the mode is trunc_points, a loop of its own with two rows per lane; inside the
// shared step loop k_trunc_sig<TR_OMAX, 1>, at 241 registers without it, needed 264: one wave per SIMD -- and a path has at least one step.
bool truncated_points_in_scope(int D, int M, int N, int L, int order) {
    return M >= 2 && N >= 2 && trunc_order(L, order) == 1 && truncated_in_scope(D, M, N, L, order);
}

// THE scope of the long mode (the SK_OP_TRUNCATED_LONG rule of sk_route_query): order 1 and what the staging and the unrolled level loop
// hold; the steps of either side are bounded only by the indices (2^20: a slab plane, a row of Yt).  Every order-1 shape of
// truncated_in_scope is inside.
bool truncated_long_in_scope(int D, int M, int N, int L, int order) {
    if (D < 1 || D > 16 || L < 1 || L > TR_LMAX || M < 1 || N < 1 || M > (1 << 20) || N > (1 << 20)) return false;
    return trunc_order(L, order) == 1;
}

// THE scope of the adjoint mode (the SK_OP_TRUNCATED_ADJOINT rule of sk_route_query): order 1, and a path dim of at most 8 -- xr, yv, the
// dX accumulators and both phases' per-level state then stay within the 256 registers two waves per SIMD leave a lane.
bool truncated_adjoint_in_scope(int D, int M, int N, int L, int order) {
    return truncated_in_scope(D, M, N, L, order) && trunc_order(L, order) == 1 && D <= 8 && M <= 128;
}

// THE scope of the points-adjoint mode (the SK_OP_TRUNCATED_RBF_ADJOINT rule of sk_route_query; M and N are POINTS): the points mode's with
// a path dim of at most 8, for the reason the adjoint mode has -- xr, the dX accumulators and either phase's per-level state within 256 registers.
bool truncated_points_adjoint_in_scope(int D, int M, int N, int L, int order) {
    return truncated_points_in_scope(D, M, N, L, order) && D <= 8;
}

// THE scope of the wide-adjoint mode (the SK_OP_TRUNCATED_WIDE_ADJOINT rule of sk_route_query): the adjoint mode's at path dims 9 .. 16 -- the
// rows and the dX accumulators of 16 coordinates in registers, the column of y read from LDS in halves (trunc_wide_adjoint).  Dims up to 8
// are the adjoint mode's own and answer false here.
bool truncated_wide_adjoint_in_scope(int D, int M, int N, int L, int order) {
    return truncated_in_scope(D, M, N, L, order) && trunc_order(L, order) == 1 && D >= 9 && M <= 128;
}

// THE scope of the long-adjoint mode (the SK_OP_TRUNCATED_LONG_ADJOINT rule of sk_route_query): the long mode's with a path dim of at most 8,
// for the reason the adjoint mode has.  Every shape of truncated_adjoint_in_scope is inside.
bool truncated_long_adjoint_in_scope(int D, int M, int N, int L, int order) {
    return truncated_long_in_scope(D, M, N, L, order) && D <= 8;
}

// paired != 0: the A = B pairs (x_p, y_p), out [A].  levels != 0: sigma is not read, out [L + 1][A][B] (paired: [L + 1][A]).
// kind 1: M and N count POINTS, param = 1 / sigma of the RBF static kernel
template <typename TO>
int launch_truncated(const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int M, int N, int Ncp, int D, int fd, int L,
                     int order, const double *sigma, TO *out, hipStream_t s, int paired, int levels, int kind, double param) {
    if (kind != 0 && kind != 1) return SK_ERR_BAD_ARG;
    if (!(kind ? truncated_points_in_scope(D, M, N, L, order) : truncated_in_scope(D, M, N, L, order))) return SK_ERR_UNSUPPORTED;
    if (fd != trunc_fd(D) || Ncp < N || (int64_t)fd * Ncp > TR_LDS_DOUBLES || Mrows < M || (paired && A != B)) return SK_ERR_BAD_ARG;
    TruncParams prm = trunc_params(kind ? TR_POINTS : TR_FORWARD, Xr, Yt, A, B, Mrows, M, N, Ncp, fd, L, trunc_order(L, order), paired,
                                   kind ? param : 0.0, out, sizeof(TO) == 4, levels, sigma, 1, nullptr, nullptr, nullptr);
    const int RC = prm.order == 1 ? 2 : 1;
    prm.logW = trunc_logw((M + RC - 1) / RC, fd, Ncp, paired);
    const int G = WAVE >> prm.logW;
    prm.n_pos = paired ? (A + G - 1) / G : (A + G - 1) / G * B;
    int64_t blocks = (int64_t)device_cu_count() * 8;
    if (blocks > prm.n_pos) blocks = prm.n_pos;
    const size_t lds = sizeof(double) * (size_t)fd * Ncp * (paired ? G : 1);
    // the points mode is order 1 with two rows per lane (the plan above), but its loop is compiled into the <TR_OMAX, 1> instance
    if (RC == 2 && !kind) SK_LAUNCH((k_trunc_sig<1, 2>), dim3((unsigned)blocks), dim3(WAVE), lds, s, prm);
    else SK_LAUNCH((k_trunc_sig<TR_OMAX, 1>), dim3((unsigned)blocks), dim3(WAVE), lds, s, prm);
    return check_launch();
}

// lanes of a pair's group in the long mode: 64 beyond 128 rows; paired: every group keeps its own tile of y, so fewer, wider groups until
// G tiles of Tc = min(Ncp, 2048 / fd) columns fit the wave's 16 KB
int truncated_long_logw(int M, int Ncp, int fd, int paired) {
    const int Tc = Ncp < TR_LDS_DOUBLES / fd ? Ncp : TR_LDS_DOUBLES / fd;
    return trunc_logw(M > 128 ? 64 : (M + 1) / 2, fd, Tc, paired);
}

namespace {
struct LongPlan {
    int logW;
    int64_t n_pos, blocks;
    size_t block_bytes;     // a block's slab: L - 1 planes of ceil64(N) doubles; none with one band or one level
};
bool plan_long(int64_t A, int64_t B, int M, int N, int Ncp, int fd, int L, int paired, size_t workspace, LongPlan *pl) {
    pl->logW = truncated_long_logw(M, Ncp, fd, paired);
    const int G = WAVE >> pl->logW;
    pl->n_pos = paired ? (A + G - 1) / G : (A + G - 1) / G * B;
    pl->blocks = (int64_t)device_cu_count() * 8;
    if (pl->blocks > pl->n_pos) pl->blocks = pl->n_pos;
    pl->block_bytes = M > 128 ? (size_t)(L - 1) * (size_t)((N + 63) / 64 * 64) * sizeof(double) : 0;
    if (pl->block_bytes) {
        const int64_t fit = (int64_t)(workspace / pl->block_bytes);
        if (fit < 1) return false;
        if (pl->blocks > fit) pl->blocks = fit;
    }
    return true;
}
}  // namespace

int truncated_long_plan(int64_t A, int64_t B, int M, int N, int D, int L, int paired, size_t workspace, int64_t *blocks, size_t *block_bytes) {
    if (!truncated_long_in_scope(D, M, N, L, 1)) return SK_ERR_UNSUPPORTED;
    LongPlan pl;
    if (!plan_long(A, paired ? A : B, M, N, (N + 15) / 16 * 16, trunc_fd(D), L, paired, workspace, &pl)) return SK_ERR_UNSUPPORTED;
    *blocks = pl.blocks;
    *block_bytes = pl.block_bytes;
    return SK_OK;
}

// the long mode's launch: the modes of launch_truncated at kind 0 (paired, levels), order 1; slab: what truncated_long_plan asks for
template <typename TO>
int launch_truncated_long(const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int M, int N, int Ncp, int D, int fd, int L,
                          int order, const double *sigma, TO *out, hipStream_t s, int paired, int levels, double *slab, size_t slab_bytes) {
    if (!truncated_long_in_scope(D, M, N, L, order)) return SK_ERR_UNSUPPORTED;
    if (fd != trunc_fd(D) || Ncp < N || Ncp % 16 || Mrows < M || (paired && A != B)) return SK_ERR_BAD_ARG;
    LongPlan pl;
    if (!plan_long(A, B, M, N, Ncp, fd, L, paired, slab ? slab_bytes : 0, &pl)) return SK_ERR_UNSUPPORTED;
    TruncParams prm = trunc_params(TR_LONG, Xr, Yt, A, B, Mrows, M, N, Ncp, fd, L, 1, paired, 0.0, out, sizeof(TO) == 4, levels, sigma, 1,
                                   nullptr, nullptr, slab);
    prm.logW = pl.logW;
    prm.n_pos = pl.n_pos;
    const int G = WAVE >> pl.logW;
    const int Tc = Ncp < TR_LDS_DOUBLES / fd ? Ncp : TR_LDS_DOUBLES / fd;
    const size_t lds = sizeof(double) * ((size_t)fd * Tc * (paired ? G : 1) + (size_t)WAVE * (TR_LMAX - 1));   // the y tiles; the lanes' level totals
    SK_LAUNCH((k_trunc_sig<TR_OMAX, 1>), dim3((unsigned)pl.blocks), dim3(WAVE), lds, s, prm);
    return check_launch();
}

namespace {
// THE adjoint modes, one row each: everything the host does differently for them.  The device functions stay four (register pressure, DESIGN
// section 4); the plan and the launcher below are one.
struct AdjointMode {
    int mode;                                   // TruncParams::mode
    bool (*in_scope)(int, int, int, int, int);  // the mode's scope = its rule of sk_route_query
    int fd;                                     // the staging width it accepts: 8, or 16 (rows and dX of 16 coordinates, Tpart [..][16])
    int g_plane;                                // slab planes beside the L - 1 prefix factors: 1 in the points-adjoint mode, the node's g
    bool is_long;                               // any number of steps: the long mode's lane groups and y tiles, a slab of one band's factors and the carries
    bool needs_param;                           // param = 1 / sigma of the RBF kernel, positive; the others do not read it
};
const AdjointMode ADJOINT_MODES[] = {
    {TR_ADJOINT, truncated_adjoint_in_scope, 8, 0, false, false},
    {TR_POINTS_ADJOINT, truncated_points_adjoint_in_scope, 8, 1, false, true},
    {TR_LONG_ADJOINT, truncated_long_adjoint_in_scope, 8, 0, true, false},
    {TR_WIDE_ADJOINT, truncated_wide_adjoint_in_scope, 16, 0, false, false},
};
const AdjointMode *adjoint_mode(int mode) {
    for (const AdjointMode &am : ADJOINT_MODES)
        if (am.mode == mode) return &am;
    return nullptr;
}

struct AdjointPlan {
    int logW;
    int64_t n_pos, n_chunks, blocks;
    size_t block_bytes;     // ONE block's slab.  (L - 1 + g_plane) planes x (N + W - 1) steps x 1 KB; long: the factors of one band,
                            // (L - 1) x (N + tiles (W - 1)) KB, and with more than one band the forward carries and the two reverse-carry
                            // halves, (bands + 2) x (L - 1) x ceil64(N) doubles
};
// The split of an adjoint launch.  Gram: the B pairs of a row tile in as many chunks as fill the resident blocks (at most B; lengths
// differ by one at most).  The block count is lowered until blocks x slab fits `workspace`; false when one block does not.  The lane
// groups are the forward's at the mode's staging width (which the paired widening counts), the long mode's where the mode is long.
bool plan_adjoint(const AdjointMode &am, int64_t A, int64_t B, int M, int N, int Ncp, int L, int paired, size_t workspace, AdjointPlan *pl) {
    pl->logW = am.is_long ? truncated_long_logw(M, Ncp, am.fd, paired) : trunc_logw((M + 1) / 2, am.fd, Ncp, paired);
    const int W = 1 << pl->logW, G = WAVE >> pl->logW;
    const int64_t rtiles = (A + G - 1) / G, resident = (int64_t)device_cu_count() * 8;
    pl->n_chunks = 1;
    if (!paired) {
        pl->n_chunks = resident / rtiles;
        if (pl->n_chunks > B) pl->n_chunks = B;
        if (pl->n_chunks < 1) pl->n_chunks = 1;
    }
    pl->n_pos = rtiles * pl->n_chunks;
    pl->blocks = pl->n_pos < resident ? pl->n_pos : resident;
    if (am.is_long) {
        const int Tc = Ncp < TR_LDS_DOUBLES / 8 ? Ncp : TR_LDS_DOUBLES / 8;
        const int64_t ctiles = (N + Tc - 1) / Tc, bands = (M + 2 * W - 1) / (2 * W), Ns = (N + 63) / 64 * 64;
        pl->block_bytes = (size_t)(L - 1) * ((size_t)(N + ctiles * (W - 1)) * 1024 + (bands > 1 ? (size_t)(bands + 2) * Ns * sizeof(double) : 0));
    } else {
        pl->block_bytes = (size_t)(L - 1 + am.g_plane) * (size_t)(N + W - 1) * 1024;
    }
    if (pl->block_bytes) {
        const int64_t fit = (int64_t)(workspace / pl->block_bytes);
        if (fit < 1) return false;
        if (pl->blocks > fit) pl->blocks = fit;
    }
    return true;
}
}  // namespace

int truncated_adjoint_plan(int mode, int64_t A, int64_t B, int M, int N, int D, int L, int paired, size_t workspace, int64_t *n_chunks,
                           int64_t *blocks, size_t *block_bytes) {
    const AdjointMode *am = adjoint_mode(mode);
    if (!am) return SK_ERR_BAD_ARG;
    if (!am->in_scope(D, M, N, L, 1)) return SK_ERR_UNSUPPORTED;
    AdjointPlan pl;
    if (!plan_adjoint(*am, A, paired ? A : B, M, N, (N + 15) / 16 * 16, L, paired, workspace, &pl)) return SK_ERR_UNSUPPORTED;
    *n_chunks = pl.n_chunks;
    *blocks = pl.blocks;
    *block_bytes = pl.block_bytes;
    return SK_OK;
}

int launch_truncated_adjoint(int mode, const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int M, int N, int Ncp, int D, int fd,
                             int L, double param, const double *w, double *Tpart, int64_t n_chunks, double *slab, size_t slab_bytes,
                             hipStream_t s, int paired) {
    const AdjointMode *am = adjoint_mode(mode);
    if (!am) return SK_ERR_BAD_ARG;
    if (!am->in_scope(D, M, N, L, 1)) return SK_ERR_UNSUPPORTED;
    // the y block of a wave holds Ncp columns; the long mode tiles them, so any multiple of 16 goes
    if (fd != am->fd || Ncp < N || (am->is_long ? Ncp % 16 != 0 : (int64_t)fd * Ncp > TR_LDS_DOUBLES) || Mrows < M || (paired && A != B) ||
        (am->needs_param && !(param > 0.0)))
        return SK_ERR_BAD_ARG;
    if (n_chunks < 1 || n_chunks > (paired ? 1 : B)) return SK_ERR_BAD_ARG;
    AdjointPlan pl;
    if (!plan_adjoint(*am, A, B, M, N, Ncp, L, paired, slab ? slab_bytes : 0, &pl)) return SK_ERR_UNSUPPORTED;
    TruncParams prm = trunc_params(mode, Xr, Yt, A, B, Mrows, M, N, Ncp, fd, L, 1, paired, am->needs_param ? param : 0.0, nullptr, false, 0,
                                   nullptr, n_chunks, w, Tpart, slab);
    prm.logW = pl.logW;
    const int G = WAVE >> pl.logW;
    prm.n_pos = (A + G - 1) / G * n_chunks;     // the caller's chunk count (Tpart is sized by it); the plan's block count for the slab
    const int64_t blocks = pl.blocks < prm.n_pos ? pl.blocks : prm.n_pos;
    // long: the y tiles at their constant stride; the reverse carry of 64 steps, eight doubles a step
    const size_t lds = am->is_long ? sizeof(double) * ((size_t)TR_LDS_DOUBLES + (size_t)WAVE * TR_LMAX)
                                   : sizeof(double) * (size_t)fd * Ncp * (paired ? G : 1);
    // the adjoint mode is the <1, 2> instance's own; every other mode is hosted by <TR_OMAX, 1> (see trunc_points)
    if (mode == TR_ADJOINT) SK_LAUNCH((k_trunc_sig<1, 2>), dim3((unsigned)blocks), dim3(WAVE), lds, s, prm);
    else SK_LAUNCH((k_trunc_sig<TR_OMAX, 1>), dim3((unsigned)blocks), dim3(WAVE), lds, s, prm);
    return check_launch();
}

template int launch_truncated_long<double>(const double *, const double *, int64_t, int64_t, int, int, int, int, int, int, int, int, const double *,
                                           double *, hipStream_t, int, int, double *, size_t);
template int launch_truncated_long<float>(const double *, const double *, int64_t, int64_t, int, int, int, int, int, int, int, int, const double *,
                                          float *, hipStream_t, int, int, double *, size_t);
template int launch_truncated<double>(const double *, const double *, int64_t, int64_t, int, int, int, int, int, int, int, int, const double *,
                                      double *, hipStream_t, int, int, int, double);
template int launch_truncated<float>(const double *, const double *, int64_t, int64_t, int, int, int, int, int, int, int, int, const double *,
                                     float *, hipStream_t, int, int, int, double);

}  // namespace sk
