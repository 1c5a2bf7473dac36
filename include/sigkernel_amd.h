/*
 * sigkernel_amd.h -- C ABI of libsigkernel_amd.so, the MI355X (gfx950) engine for the
 * signature-PDE-kernel hot path of crispitagorico/sigkernel.
 *
 * The reference has no FFI: its boundary is the Python signature of the solver
 * back-ends called from sigkernel/sigkernel.py.  Each entry point below names
 * the reference call it replaces (paths relative to the reference checkout).
 *
 * Conventions
 *   - P independent problems ("pairs"): P = A for compute_kernel, P = A*B for
 *     compute_Gram with pair (a,b) at index a*B+b.
 *   - M, N   : number of points of the two paths; Mc = M-1, Nc = N-1 coarse cells.
 *   - dyadic : dyadic_order d; the fine grid has MM = Mc<<d by NN = Nc<<d cells.
 *     Dyadic refinement is index arithmetic inside the kernels
 *     (fine increment (i,j) = inc_c[i>>d][j>>d] / 4^d); the refined matrix that
 *     the reference materialises with tile() (sigkernel.py:218, :364) never exists.
 *   - all arrays are row-major device pointers owned by the caller; the library keeps no
 *     reference after return and allocates nothing.  Increment matrices carry a row stride
 *     `ld` (in elements, ld >= Nc; 0 means dense, ld = Nc): the fast kernels want 16-byte
 *     aligned rows (ld*sizeof(T) % 16 == 0, base pointer 16-byte aligned, which
 *     sk_increments_* produces when asked); any other layout is served by the simple
 *     kernels.  Everything else is dense.
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     every call only enqueues work on it -- no hidden synchronisation.
 *   - return value: SK_OK or an sk_status error code (see sk_status_string).
 *   - f32 entry points read/write float but carry the PDE state in double.
 */
#ifndef SIGKERNEL_AMD_H
#define SIGKERNEL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum sk_status {
    SK_OK = 0,
    SK_ERR_BAD_ARG = 1,      /* null pointer, non-positive size, unknown scheme/flag     */
    SK_ERR_UNSUPPORTED = 2,  /* shape outside what the kernels implement (see message)  */
    SK_ERR_LAUNCH = 3,       /* hipGetLastError() after the launch was not hipSuccess   */
    SK_ERR_WORKSPACE = 4,    /* workspace pointer null or too small                     */
    SK_ERR_NO_DEVICE = 5     /* no HIP device visible                                   */
} sk_status;

/* scheme: which finite-difference stencil (sigkernel/cython_backend.pyx:114-116,
 * sigkernel/cuda_backend.py:150-156). */
#define SK_SCHEME_DEFAULT 0 /* (k10+k01)(1+g/2+g^2/12) - k00(1-g^2/12)  -- _naive_solver=False */
#define SK_SCHEME_NAIVE 1   /* (k10+k01)(1+g/2) - k00                    -- _naive_solver=True  */

/* flags (bit-or) */
#define SK_FLAG_NONE 0
#define SK_FLAG_EXACT 1  /* FMA-free arithmetic in the reference's operand order: results are
                            bit-identical to the reference's Cython CPU solver (slower path)   */
#define SK_FLAG_SIMPLE 2 /* force the simple one-wavefront-per-pair anti-diagonal kernels       */
#define SK_FLAG_EDGES_GIVEN 8 /* sk_solve_adj_* only: `workspace` already holds the strip edges that
                               * sk_solve_fwd_edges_* wrote for these increments -- skip the forward sweep */
#define SK_FLAG_FAST_ONLY 4 /* never fall back: SK_ERR_UNSUPPORTED if the tiled kernels do not
                               cover the shape/layout (used by tests and benchmarks)            */
#define SK_FLAG_DISCRETE 16 /* sk_solve_adj_* only: W is the exact derivative of the returned value with respect to every coarse
                             * increment -- the adjoint of the DISCRETE solver, not the reference's formula (see sk_solve_adj_*) */
#define SK_FLAG_RAGGED 32 /* sk_solve_adj_* only, and only together with SK_FLAG_DISCRETE: every pair is differentiated on its own
                           * sub-grid, read from a table at the head of `workspace` (see sk_solve_adj_*) */
#define SK_FLAG_SOURCES 64 /* sk_solve_adj_* only, and only together with SK_FLAG_DISCRETE (never with SK_FLAG_RAGGED): W is in/out -- on
                            * entry the weight S of every coarse node in L = sum S K, on exit dL / d inc_c (see sk_solve_adj_*) */

/* 340.  The number moves whenever an exported signature changes incompatibly: 310 -> 320 gave sk_solve_fwd_{linear,rbf}_sym_* their
 * pair_tab argument (position 3) and added the sk_prep_cat_* / sk_solve_fwd_loss_f64 / sk_loss_* / sk_*_adjoint_finish_f64 family;
 * 320 -> 330 gave sk_linear_adjoint_fused_f64 its ypart / ypart_doubles / ycols_out arguments (the second-argument sums); 330 -> 340
 * widened sk_static_increments_* to any path dim and gave sk_static_adjoint_* kind 1 a different output beyond 32 dims (see there).  Entry
 * points that are only ADDED (the prefix slices, sk_truncated_paired_*, sk_truncated_levels_*, sk_truncated_adjoint*, sk_truncated_points_*, sk_truncated_points_adjoint*, sk_truncated_long_*, sk_truncated_long_adjoint*, sk_truncated_wide_adjoint*, sk_plan_adjoint_chunks, sk_plan_one_draw, sk_solve_prefix_resume_*, sk_prefix_state_pitch, sk_solve_fwd_resume_*, sk_solve_fwd_resume_fits) leave the number where it is.  A binding
 * written against an older number must not load this library silently (sigkernel_amd/_lib.py checks it at load). */
int sk_version(void);
/* "sigkernel_amd gfx950; sources <hash>; <hipcc --version>; ISA hazard lint passed at build": the sources and the toolchain this
 * binary was built from (static string).  The hand-scheduled kernels are linted at build time against the register allocator of
 * THAT compiler (csrc/Makefile); a deployment that rebuilds with another one gets a different string -- and a fresh lint. */
const char *sk_build_info(void);

/* ---- routing (host only: no device work) --------------------------------------------------------------------------------------
 * Which kernel family serves a call -- the ONE statement of the fused kernels' scope: the host layer asks it instead of keeping
 * its own predicates, and every launcher honours it (csrc/sk_route.hip holds the rules; tests pin them against a table).
 *   op     SK_OP_FORWARD: k_sig values (sigkernel.py:216-234, :362-382);  SK_OP_ADJOINT: the gradient (sigkernel.py:257-343, :404-502)
 *          -- the forward of a call with a gradient pending keeps the edges of the family the ADJOINT query names
 *   kind   0 = LinearKernel, 1 = RBFKernel (sigma > 0); anything else streams
 *   D, M, N, dyadic, scheme (SK_SCHEME_*), elem_size (8 / 4: the dtype of the caller's paths)
 *   flags  SK_ROUTE_NO_STREAM: never answer STREAM where a fused kernel exists (memory first).  Without it the multi-band kernels
 *          are only chosen where they are not mostly sweeping padding (short paths: the streaming route, whose transient memory the
 *          caller bounds by tiling over rows, is several times faster there -- csrc/sk_route.hip has the rule and the measurements)
 * Returns
 *   SK_ROUTE_STREAM         static kernel -> increments in HBM (pairs x M x N) -> sk_solve_fwd_* / sk_solve_adj_*
 *   SK_ROUTE_FUSED          one band per pair: sk_solve_fwd_linear_* / _rbf_* (+ _edges_f64), sk_linear_adjoint_fused_f64,
 *                           sk_rbf_adjoint_fused_f64 -- nothing of size pairs x M x N exists
 *   SK_ROUTE_FUSED_MB       several bands / wide paths: sk_solve_fwd_static_*, sk_linear_adjoint_fused_mb_f64, sk_rbf_adjoint_fused_mb_f64
 *   SK_ROUTE_FUSED_MB_SWAP  (forward only) sk_solve_fwd_static_* on (Y, X): k is symmetric and that orientation is cheaper
 *   SK_ROUTE_FUSED_SWAP     the one-band kernels on (Y, X): the second paths fit one band (rows <= 64 RC), the first do not; for the ADJOINT
 *                           (Gram; dim <= 8 -- rbf of dim 5..8 at dyadic 0 and 1; fp32 paths up-cast by the caller): sk_rbf_adjoint_fused_f64 / sk_linear_adjoint_fused_f64 on
 *                           (Y, X) with the second-argument sums (rbf, 128 x 128 pairs of 700 x 20 points: 0.41 ms against 1.56 ms
 *                           streamed); Gram callers transpose the result
 * For exactly LinearKernel / RBFKernel, D <= 16, dyadic <= 2, either scheme, the answer with SK_ROUTE_NO_STREAM is never
 * SK_ROUTE_STREAM: every such call CAN run with nothing of size pairs x M x N in HBM. */
#define SK_ROUTE_NO_STREAM 1
#define SK_ROUTE_NO_SWAP 2      /* never answer a swapped ADJOINT route (paired batches: the second-argument sums exist for Gram calls) */
/* The COST table: every measured crossover the library (sk_route_query, the launchers) and the host layer (symmetric blocks, merged
 * loss, paired merge) decide by, with the same-box A/B measurement each came from -- entries 0 .. n-1 (sk_cost_name returns NULL past
 * the end).  Scope rules say what a kernel CAN do; these say when it is the faster choice.  tools/crossovers.py re-measures them on
 * the box at hand.  The reference has no counterpart (it has one route per device, sigkernel.py:220-246). */
double sk_cost_query(int which);
const char *sk_cost_name(int which);
const char *sk_cost_note(int which);
#define SK_OP_FORWARD 0
#define SK_OP_ADJOINT 1
#define SK_OP_ADJOINT_SYM 2   /* compute_Gram(X, X, sym=True) with a gradient (sigkernel.py:404-416 on the symmetric call): SK_ROUTE_FUSED =
                                 the TRIANGLE through sk_rbf_adjoint_fused_f64 with the second-argument sums; else all pairs */
#define SK_OP_PREFIX 3        /* the grid of prefix kernels k_sig(x[:m+1], y[:n+1]) (compute_Gram_prefixes / compute_kernel_prefixes):
                                 SK_ROUTE_FUSED = sk_solve_prefix_linear_* / _rbf_* (one band per pair, path dim <= 8, dyadic <= 2: rows <= 64 RC,
                                 RC = 4 / 2 / 1 at dyadic 0 / 1 / 2, rows = M - 1 linear, M rbf; rbf at dyadic 0: two rows per lane, M <= 128);
                                 SK_ROUTE_STREAM = sk_static_increments_* + sk_solve_fwd_* with out_grid, sliced.  Never a swapped route:
                                 the grid of k(y, x) is the transpose. */
#define SK_OP_TRUNCATED 4     /* truncated_sig_kernel (transformers.py:201-236): kind = order (< 1: num_levels), dyadic = num_levels, M / N =
                                 STEPS per path of the two batches.  SK_ROUTE_FUSED = sk_truncated_gram_*: path dim <= 16, num_levels <= 8,
                                 order 1 with M <= 128 (two rows per lane) or order <= 4 with M <= 64 (one), and 8 (dim <= 8; else 16) x
                                 ceil16(N) <= 2048 (the y block of a wave in 16 KB of LDS); SK_ROUTE_FUSED_SWAP = the same on (y, x), the
                                 result transposed; SK_ROUTE_STREAM = the host layer's torch restatement (differentiable). */
#define SK_OP_TRUNCATED_ADJOINT 5 /* the gradient of the truncated kernel's level terms with respect to the FIRST batch (kind, dyadic, M, N as
                                 SK_OP_TRUNCATED): SK_ROUTE_FUSED = sk_truncated_adjoint: inside SK_OP_TRUNCATED's FUSED scope, order 1 (kind 1, or
                                 num_levels 1), path dim <= 8, M <= 128; SK_ROUTE_STREAM otherwise = autograd of the host layer's torch
                                 restatement.  Never swapped: the second batch's gradient is the same query on (N, M). */
#define SK_OP_TRUNCATED_RBF 6  /* the truncated kernel lifted through an RBF static kernel (TruncatedSigKernel(static_kernel=RBFKernel(s)); no
                                 counterpart in the reference): kind, dyadic as SK_OP_TRUNCATED, M / N = POINTS per path of the two batches, the
                                 rows and columns of the sweep.  SK_ROUTE_FUSED = sk_truncated_points_* with kind 1: SK_OP_TRUNCATED's rule on
                                 the points at order 1 (kind 1, or num_levels 1: M <= 128; 8 or 16 x ceil16(N) <= 2048) and M, N >= 2;
                                 SK_ROUTE_FUSED_SWAP = the same on (y, x), transposed; SK_ROUTE_STREAM = the host layer's torch restatement. */
#define SK_OP_TRUNCATED_RBF_ADJOINT 7 /* the gradient of the lifted kernel's level terms with respect to the POINTS of the FIRST batch (kind,
                                 dyadic, M, N as SK_OP_TRUNCATED_RBF: points): SK_ROUTE_FUSED = sk_truncated_points_adjoint: inside
                                 SK_OP_TRUNCATED_RBF's FUSED scope with path dim <= 8 (order 1, 2 <= M <= 128, N >= 2, 8 x ceil16(N) <= 2048);
                                 SK_ROUTE_STREAM otherwise = autograd of the host layer's torch restatement.  Never swapped: the second
                                 batch's gradient is the same query on (N, M). */
#define SK_OP_TRUNCATED_LONG 8 /* truncated_sig_kernel at order 1 on paths of ANY length (kind, dyadic, M, N as SK_OP_TRUNCATED: steps):
                                 SK_ROUTE_FUSED = sk_truncated_long_*: order 1 (kind 1, or num_levels 1), path dim <= 16, num_levels <= 8,
                                 1 <= M, N <= 2^20 -- every order-1 shape of SK_OP_TRUNCATED's FUSED scope is inside; SK_ROUTE_FUSED_SWAP = the
                                 same on (y, x), the result transposed, where that sweep takes fewer steps; SK_ROUTE_STREAM otherwise = the
                                 host layer's torch restatement.  The host layer asks only where SK_OP_TRUNCATED said STREAM, and only when
                                 its switch (sigkernel_amd.routes.truncated_long) is on. */
#define SK_OP_TRUNCATED_LONG_ADJOINT 9 /* the gradient of SK_OP_TRUNCATED_ADJOINT on paths of ANY length (kind, dyadic, M, N as SK_OP_TRUNCATED:
                                 steps): SK_ROUTE_FUSED = sk_truncated_long_adjoint: order 1 (kind 1, or num_levels 1), path dim <= 8,
                                 num_levels <= 8, 1 <= M, N <= 2^20 -- every shape of SK_OP_TRUNCATED_ADJOINT's FUSED scope is inside;
                                 SK_ROUTE_STREAM otherwise = autograd of the host layer's torch restatement.  Never swapped: the gradient goes
                                 to the rows, and the second batch's is the same query on (N, M).  The host layer asks only where
                                 SK_OP_TRUNCATED_ADJOINT's route declined, and only for TruncatedSigKernel(long_adjoint=True). */
#define SK_OP_TRUNCATED_WIDE_ADJOINT 10 /* the gradient of SK_OP_TRUNCATED_ADJOINT at path dims 9 .. 16 (kind, dyadic, M, N as SK_OP_TRUNCATED:
                                 steps): SK_ROUTE_FUSED = sk_truncated_wide_adjoint: inside SK_OP_TRUNCATED's FUSED scope, order 1 (kind 1, or
                                 num_levels 1), 9 <= path dim <= 16, M <= 128 (and 16 x ceil16(N) <= 2048: N <= 128); SK_ROUTE_STREAM otherwise
                                 -- path dims up to 8 included, which SK_OP_TRUNCATED_ADJOINT serves -- = autograd of the host layer's torch
                                 restatement.  Never swapped: the second batch's gradient is the same query on (N, M).  The host layer asks
                                 only where SK_OP_TRUNCATED_ADJOINT's route declined, and only for TruncatedSigKernel(wide_adjoint=True). */
#define SK_ROUTE_STREAM 0
#define SK_ROUTE_FUSED 1
#define SK_ROUTE_FUSED_MB 2
#define SK_ROUTE_FUSED_MB_SWAP 3
#define SK_ROUTE_FUSED_SWAP 4
int sk_route_query(int op, int kind, int D, int M, int N, int dyadic, int scheme, int elem_size, int flags);

/* Development hook: the SK_* tuning knobs are parsed from the environment ONCE, when the library is loaded; tools that sweep a
 * knob inside one process call this after changing it.  Not for product code (not thread-safe against concurrent launches). */
void sk_reload_knobs(void);

/* Diagnostics: which kernel instances does a workload launch?  Every launch of the library is counted per kernel instance while
 * tracing is on (enable: 1 on, 0 off, anything else: query; returns the previous state; SK_TRACE_LAUNCHES=1 in the environment
 * switches it on at load).  sk_launch_trace_dump writes "count<TAB>device symbol<NL>" per instance launched since the last reset into
 * buf (NUL-terminated, truncated to n bytes; buf may be NULL) and returns the bytes the whole list needs; reset != 0 clears the counts.
 * tools/reach_sweep.py + tests check the list of instances the build contains against it: no unreachable instance.  No counterpart in
 * the reference (its back-ends are JIT-compiled per call signature, cuda_backend.py:5). */
int sk_launch_trace(int enable);
size_t sk_launch_trace_dump(char *buf, size_t n, int reset);

/* kappa_d = 4^-d / sqrt(12), see sk_solve_fwd_linear_*. */
double sk_linear_prescale(int dyadic);
/* The multiplier and shift by which the fused forward divides a pair index by the Gram's column count B (host arithmetic only, no
 * device): floor(p / B) = (uint32_t)(((uint64_t)(2 p) * *mul) >> 32) >> *shift for every 0 <= p < 2^31.  SK_ERR_BAD_ARG unless
 * 1 <= B < 2^31. */
int sk_pair_div_magic(int64_t B, uint32_t *mul, int *shift);
const char *sk_status_string(int status);
/* Number of HIP devices visible, or a negative sk_status. */
int sk_device_count(void);

/* ---- increments ---------------------------------------------------------------------------
 * inc_c[p][i][j] = G[p][i+1][j+1] + G[p][i][j] - G[p][i+1][j] - G[p][i][j+1]
 * Replaces the 4-corner difference at sigkernel.py:217 (paired) and :363 (Gram); recomputed in
 * backward at :264 and :421.   G [P,M,N] -> inc_c [P,M-1,ld] (columns >= N-1 are zero-filled). */
int sk_increments_f64(const double *G, int64_t P, int M, int N, double *inc_c, int64_t ld, void *stream);
int sk_increments_f32(const float *G, int64_t P, int M, int N, float *inc_c, int64_t ld, void *stream);

/* Static kernel + increments in ONE pass for the reference's two standard static kernels, straight from the paths:
 * replaces static_kernel.Gram_matrix(X, Y) / batch_kernel(X, Y) (static_kernels.py:24,33,56,73) followed by the
 * 4-corner difference (sigkernel.py:216-217, :362-363) -- G_static is never materialised.
 *   kind 0: linear, inc = param^2 <dx_p, dy_q>  (param = 1 reproduces Gram_matrix, which ignores `scale`;
 *           param = scale reproduces batch_kernel).  9 <= D <= 32: on v_mfma_f64_16x16x4_f64, dims summed four at a time --
 *           equal to the D <= 8 form's left-to-right sum to rounding
 *   kind 1: rbf,    G = exp(-|x_p - y_q|^2 / param) (param = sigma), inc = ((G11 + G00) - G10) - G01
 *   X [A,M,D], Y [B,N,D] dense; B > 0: Gram, pair (a,b) at a*B+b; B == 0: paired, pair a = (x_a, y_a), Y [A,N,D].
 *   inc_c [P,M-1,ld] with zero-filled padding columns.  Any D >= 1: beyond 32 dims the node Gram runs as a K-looped GEMM on
 *   v_mfma_f64_16x16x4_f64 (one workgroup per 64-row tile of x_a and several y_b, dims staged through LDS; fp32 paths up-cast on
 *   load) -- dims summed in a different order than the generic route's, equal to it to rounding. */
int sk_static_increments_f64(int kind, double param, const double *X, const double *Y, int64_t A, int64_t B, int M, int N,
                             int D, double *inc_c, int64_t ld, void *stream);
int sk_static_increments_f32(int kind, double param, const float *X, const float *Y, int64_t A, int64_t B, int M, int N,
                             int D, float *inc_c, int64_t ld, void *stream);

/* Adjoint of sk_static_increments_*: dL/dX from W = dL/d inc_c and the per-pair upstream gradient, with neither G_static
 * nor dL/dG_static materialised.  Replaces the finite-difference contraction (sigkernel.py:313-341, :472-500) and the
 * `grad_output * grad_points` reduction over the second batch index (:343, :410-416) for these two static kernels.
 *   W [P,M-1,ldw]; scale [P] = upstream gradient per pair (NULL = 1); pairs as in sk_static_increments_*.
 *   kind 1 (rbf):    out = dL/dX [A,M,D] for D <= 32.  D > 32: out = H [P,M,ldh], ldh = N rounded up to whole 128-byte rows,
 *                    H[p][m][n] = scale_p dL/dG[m][n] G[m][n] (dL/dG: the 4-corner adjoint of W) -- the first pass of the chain rule;
 *                    the caller finishes dL/dx_a[m] = -(2/param) (sum_{b,n} H[a,b,m,n] x_m - sum_b H[a,b] @ y_b) with library GEMMs.
 *   kind 0 (linear): out = T [A,M-1,D], T[a][p] = sum_b scale_ab sum_q W[a,b,p,q] (y[b,q+1]-y[b,q]) (the caller differences it along
 *                    the path and applies scale^2), for 9 <= D <= 32 and N <= 128 (k_static_linear_adj_tiled: W read once, y_b through
 *                    LDS).  SK_ERR_UNSUPPORTED otherwise: dim <= 8 runs from pre-differenced paths in sk_linear_adjoint_*, wider or
 *                    longer paths as a plain batched GEMM in the caller.  X and param are not read. */
int sk_static_adjoint_f64(int kind, double param, const double *X, const double *Y, const double *W, int64_t ldw,
                          const double *scale, int64_t A, int64_t B, int M, int N, int D, double *out, void *stream);
int sk_static_adjoint_f32(int kind, double param, const float *X, const float *Y, const float *W, int64_t ldw,
                          const float *scale, int64_t A, int64_t B, int M, int N, int D, float *out, void *stream);

/* sk_static_adjoint_f64 for RBFKernel with the bandwidth's gradient from the same launch (k_static_rbf_adj's parameter mode: per node
 * the kernel already holds c = scale_p dL/dG[m][n] G[m][n] and r2 = |x_m - y_n|^2; dG/dsigma = G r2 / sigma^2).  An added entry: the
 * version number stays.  fp64; kind 1 and D <= 32 only (kind 0, D > 32: SK_ERR_UNSUPPORTED; the caller differentiates the static
 * kernel itself there).  Arguments up to D as for sk_static_adjoint_f64.
 *   out_dX [A,M,D] = dL/dX, bit for bit what sk_static_adjoint_f64 gives from k_static_rbf_adj (for 17 <= D <= 32 and N <= 128 that
 *   entry runs the tiled kernel instead: equal up to rounding);
 *   out_partials [*n_partials]: one sum of c r2 per block of the launch, every element written;
 *       dL/dparam = (out_partials[0] + out_partials[1] + ...) / param^2,
 *   added by the caller in index order -- no atomics, the same bits every time.  The kernel has ONE output pointer: both arrays are
 *   one allocation, out_partials == out_dX + A M D (anything else: SK_ERR_BAD_ARG).
 *   *n_partials: how many partials the caller allocated; it must equal what the shape needs.  out_dX == NULL and out_partials == NULL:
 *   size query, *n_partials receives that number (a function of A, M and D) and nothing is launched.
 * SK_ERR_BAD_ARG: a null pointer, a wrong count, non-adjacent outputs, param <= 0 -- all refused before any launch. */
int sk_static_adjoint_param_f64(int kind, double param, const double *X, const double *Y, const double *W, int64_t ldw,
                                const double *scale, int64_t A, int64_t B, int M, int N, int D, double *out_dX, double *out_partials,
                                int64_t *n_partials, void *stream);

/* LinearKernel adjoint from pre-differenced paths (the fast route for path dim <= 8; same contraction as
 * sk_static_adjoint_* with kind 0): dYt [Bn][8][ldy] fp64 = y[q+1]-y[q], dimension-major, zero-padded -- the array
 * sk_solve_fwd_linear_* takes; W [P, Mc, ldw]; scale [P] nullable; out [A, Mc, D] = sum_b scale_ab sum_q W[a,b,p,q] dy[b,q,:].
 * The caller differences `out` along the path (d inc[p,q]/d x[p+1] = +s^2 dy[q], d/d x[p] = -s^2 dy[q]).  B = 0: paired. */
int sk_linear_adjoint_f64(const double *dYt, int64_t ldy, const double *W, int64_t ldw, const double *scale, int64_t A,
                          int64_t B, int Mc, int Nc, int D, double *out, void *stream);
int sk_linear_adjoint_f32(const double *dYt, int64_t ldy, const float *W, int64_t ldw, const float *scale, int64_t A, int64_t B,
                          int Mc, int Nc, int D, float *out, void *stream);

/* Adjoint PDE AND LinearKernel contraction in one kernel (csrc/sk_wave_adj_fused.hip): the reverse sweep forms its increments
 * from the path differences, recomputes K from the terminal edges a forward with edges kept (sk_solve_fwd_linear_edges_f64),
 * and contracts W = d k / d inc with the y differences on the spot -- neither the increments nor W exist in HBM.  Replaces
 * sigkernel.py:438-500 for LinearKernel, i.e. sk_static_increments + sk_solve_adj(EDGES_GIVEN) + sk_linear_adjoint.
 *   dXr [A][Mrows][8] = s^2 (x[p+1]-x[p]) -- the LAYOUT of sk_solve_fwd_linear_*'s array but WITHOUT its kappa = sk_linear_prescale(dyadic)
 *   factor (this kernel forms inc = <dXr, dYt> itself, and so does its rescue: a forward's pre-scaled staging would give gradients
 *   wrong by kappa);  dYt [Bn][8][Ncp] = y[q+1]-y[q], Mrows, Ncp: as sk_solve_fwd_linear_* takes them;
 *   edges: sk_strip_edges_bytes layout;  scale [A*B] nullable;  either scheme.
 *   tpart [tpart_doubles] receives partial sums over b: viewed as [A][ceil(B / *ppg_out)][*rows_out][8] (the B pairs of an x_a are split
 *   into that many chunks, lengths differing by one where the number does not divide B; *ppg_out is the longest), sum over the chunk axis,
 *   then T[a][p][:] = that[a][*rows_out - 1 - p][:] for p < Mc is what sk_linear_adjoint_* returns.  tpart == NULL: only
 *   *ppg_out and *rows_out are set (size query: A * ceil(B / ppg) * rows * 8 doubles).  err [P] zero-initialised: per-pair
 *   self-check residual as for sk_solve_adj_*.  B == 0: paired batch (P = A, Bn = A, one chunk).  fp64, dyadic <= 2, Mc <= 128 (64 at dyadic 2),
 *   path dim <= 8; otherwise SK_ERR_UNSUPPORTED (sk_route_query(SK_OP_ADJOINT, 0, ...) == SK_ROUTE_FUSED says when it applies).
 *   ypart / ycols_out (either non-NULL; Gram only, B > 0): the SECOND-argument sums INSTEAD of tpart (which is not touched) --
 *   ypart viewed as [A][B][*ycols_out][8]: per pair and increment column q < Nc of y_b, sum_p W[a,b,p,q] dXr[a][p][:], WITHOUT the
 *   upstream gradient (`scale` then only marks screened pairs): d k(x_a, y_b) / d (y_b[q+1] - y_b[q]); the caller weights the pairs of
 *   a y_b, adds them and differences along the path.  Columns q >= Nc are padding and hold nothing meaningful.  ypart == NULL with
 *   ycols_out set: size query (A B *ycols_out 8 doubles).  This is what SK_ROUTE_FUSED_SWAP runs on (Y, X) for LinearKernel. */
int sk_linear_adjoint_fused_f64(const double *dXr, const double *dYt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp,
                                int dyadic, int scheme, const double *edges, const double *scale, double *tpart,
                                size_t tpart_doubles, double *err, double *ypart, size_t ypart_doubles, int *ppg_out, int *rows_out,
                                int *ycols_out, const double *kfinal, double screen, double tol, void *rescue_ws,
                                size_t rescue_ws_bytes, void *stream);

/* Adjoint PDE AND RBFKernel chain rule in one kernel (csrc/sk_wave_adj_fused_rbf.hip): the reverse sweep evaluates the nodes
 * G = exp(-|x - y|^2 / sigma) itself, forms its increments as their 4-corner differences, recomputes K from the terminal edges a
 * forward with edges kept (sk_solve_fwd_rbf_edges_f64), and pushes W = d k / d inc through the difference and the exponential on
 * the spot -- neither the increments nor W nor G_static exist in HBM.  Replaces sigkernel.py:419-502 + :404-416 for RBFKernel,
 * i.e. sk_static_increments + sk_solve_adj(EDGES_GIVEN) + sk_static_adjoint.
 *   Xr [A][Mrows][8], Yt [Bn][8][Ncp]: the POINT arrays sk_solve_fwd_rbf_* takes;  edges: sk_strip_edges_bytes layout;
 *   scale [P] nullable (upstream gradient per pair).  gpart [gpart_doubles] receives partial sums over b, viewed as
 *   [A][ceil(B / *ppg_out)][*rows_out][*outw_out]: summed over the chunk axis, row r < M holds cs = [..][0] and accd = [..][2 .. 2+D), and
 *   dL/dx_a[r] = (-2 / sigma) (x_a[r] cs - accd).  gpart == NULL: size query only.  err [P] zero-initialised: self-check residual
 *   as for sk_solve_adj_*.  B == 0: paired batch.  fp64, dyadic 1..2 (either scheme, path dim <= 8; dim 5..8 at dyadic 1: one coarse row per lane, M <= 64) and dyadic 0 (default scheme, path
 *   dim <= 8, M <= 128: two coarse rows per lane on the strip kernels' edge layout), one band per pair with
 *   M <= lanes x rows per lane (edges: sk_strip_edges_bytes(P, Mc, Nc, ...) -- with Nc + 1 in place of Nc when Nc is a multiple
 *   of 16: the sweep needs a padding NODE column behind the last unit, as sk_solve_fwd_rbf_edges_f64 keeps them); otherwise SK_ERR_UNSUPPORTED
 *   (sk_route_query(SK_OP_ADJOINT, 1, ...) == SK_ROUTE_FUSED says when the host layer takes it: path dim <= 4).
 *   ypart (nullable; Gram): the SECOND-argument sums of the same sweep, for compute_Gram(X, X, sym=True) with a
 *   gradient (compute_mmd's K_XX, sigkernel.py:190), where only the pairs on and above the diagonal are solved and a pair (a, b)
 *   also owes d1 k(x_b, x_a) = d2 k(x_a, x_b) to row b -- and for SK_ROUTE_FUSED_SWAP.  Viewed as [A*B][*ycols_out][W], W = 6 for
 *   path dim <= 4 and 10 for dim 5..8, node column c < N of pair (a, b) holds S0 = [..][0] and S1 = [..][2 .. 2+D), WITHOUT the
 *   upstream gradient: d k(x_a, y_b) / d y_b[c] = (-2 / sigma) (y_b[c] S0 - S1); the caller weights the pairs and folds them over a.
 *   gpart == NULL with ypart given, and always for path dim 5..8 (dyadic 0 and 1): the sums INSTEAD of gpart, which is not written
 *   then (all a swapped call needs -- fewer instructions per macro-step; the variant of dims 5..8 has registers for one of the two).
 *   ycols_out != NULL in the size query asks for that variant's sizes. */
int sk_rbf_adjoint_fused_f64(const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D,
                             int dyadic, int scheme, double sigma, const double *edges, const double *scale, double *gpart,
                             size_t gpart_doubles, double *err, double *ypart, size_t ypart_doubles, int *ppg_out, int *rows_out,
                             int *outw_out, int *ycols_out, const double *kfinal, double screen, double tol, void *rescue_ws,
                             size_t rescue_ws_bytes, void *stream);

/* k, d/dgamma k, d2/dgamma2 k with the static kernel fused in (csrc/sk_wave_deriv_fused.hip): the three increment arrays of k_kgrad
 * (sigkernel.py:526-541) are formed inside the solver from the point arrays of x, x + eps gamma, x + 2 eps gamma and y, in the
 * operand order of sk_static_deriv_increments_* (bit-identical increments), and never exist in HBM.  Replaces
 * sk_static_deriv_increments_* + sk_solve_deriv_* (cuda_backend.py:165-223, sigkernel.py:526-566) for LinearKernel (kind 0) and
 * RBFKernel (kind 1, param = sigma).
 *   X0r, X1r, X2r [A][Mrows][fd], Yt [Bn][fd][Ncp]: fp64 POINT arrays as sk_prep_paths_* builds them (fd = 8; D <= 8;
 *   Mrows >= *mrows of sk_solve_deriv_static_workspace_bytes; Ncp >= 2 NUp, NUp = ceil8((Nc + 2) / 2) >= 64);  B > 0: Gram, B == 0:
 *   paired;  out_* [P].  SK_ERR_UNSUPPORTED (workspace_bytes 0): dyadic > 2, D > 8, second path shorter than 126 points. */
size_t sk_solve_deriv_static_workspace_bytes(int64_t P, int Mc, int Nc, int dyadic, int D, int *mrows);
int sk_solve_deriv_static_f64(int kind, double param, const double *X0r, const double *X1r, const double *X2r, const double *Yt, int64_t A,
                              int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D, int fd, int dyadic, int scheme, double eps, double *out_k,
                              double *out_kd, double *out_kdd, void *workspace, size_t workspace_bytes, void *stream);

/* The fused RBF adjoint for LONG or WIDE paths (csrc/sk_wave_adj_fused_mb.hip): any number of bands per pair, path dimensions up to
 * 16 -- BASELINE configs[4]'s shape with a gradient runs in sk_solve_fwd_static_* (edges) + this kernel with nothing of size P*M*N
 * in HBM.  Replaces sigkernel.py:419-502 + :404-416 for RBFKernel there, i.e. sk_static_increments + sk_solve_fwd + sk_solve_adj +
 * sk_static_adjoint.
 *   sk_rbf_adjoint_fused_mb_layout: *mrows = rows of Xr per path, gpart = [P][*rows][*outw] doubles, n0 = [P][*ncols] doubles,
 *   *edge_doubles per pair, *workspace_bytes (one band-boundary row per resident wave); SK_ERR_UNSUPPORTED outside the scope
 *   (dyadic 0..2, D <= 16; any M, N: second paths shorter than ~160 points are swept with masked padding units, *ncols = 2 NUp = Ncp;
 *   at dyadic 0 the kernel gives a lane two coarse rows -- bands of 128 rows -- and sk_solve_fwd_static_* keeps its edges likewise).
 *   Xr [A][Mrows][fd] / Yt [Bn][fd][Ncp]: the fp64 POINT arrays of sk_solve_fwd_static_* (kind 1), fd = 8 or 16; yt_f32 = 1 (fd = 16,
 *   fp32 inputs): Yt is the packed fp32 array sk_solve_fwd_static_f32 takes -- half the LDS ring, two waves per SIMD at 16 dimensions;
 *   edges: what sk_solve_fwd_static_* kept;  scale [P] nullable.  gpart receives, per PAIR and node row 1 <= r < M, cs = [..][0]
 *   and accd = [..][2 .. 2+D): summed over the pairs of an x_a, dL/dx_a[r] = (-2 / sigma) (x_a[r] cs - accd).  Node row 0 (gpart's
 *   row 0 is written by the rescue only: zero it) comes as per-column weights n0[pair][c], c < N: cs += sum_c n0, accd += sum_c n0 y_b[c].
 *   rescue_ws / kfinal / screen / tol: the device-side rescue described below (sk_fused_rescue_workspace_bytes(1, ...)), with yt64 =
 *   the fp64 Yt [Bn][fd][Ncp] (the same array as Yt unless yt_f32).  err [P] zero-initialised:
 *   self-check residual as for sk_solve_adj_* (a pair whose scale is NaN is skipped and its sums stored as zeros). */
int sk_rbf_adjoint_fused_mb_layout(int64_t P, int Mc, int Nc, int dyadic, int D, int *mrows, int *rows, int *outw, int *ncols,
                                   int64_t *edge_doubles, size_t *workspace_bytes);
int sk_rbf_adjoint_fused_mb_f64(const double *Xr, const void *Yt, int yt_f32, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D, int fd,
                                int dyadic, int scheme, double sigma, const double *edges, const double *scale, double *gpart,
                                size_t gpart_doubles, double *n0, size_t n0_doubles, double *err, void *workspace, size_t workspace_bytes,
                                const double *yt64, const double *kfinal, double screen, double tol, void *rescue_ws, size_t rescue_ws_bytes,
                                void *stream);

/* The same for LinearKernel on long / wide paths (csrc/sk_wave_adj_fused_mb.hip: k_adj_fused_linear_mb): increments from the path
 * differences, W contracted with the y differences on the spot.  Replaces sigkernel.py:419-502 + :404-416 there, i.e.
 * sk_static_increments + sk_solve_fwd + sk_solve_adj + sk_linear_adjoint.
 *   dXr [A][Mrows][fd] = s^2 (x[p+1]-x[p]), dYt [Bn][fd][Ncp] = y[q+1]-y[q] (sk_solve_fwd_static_*'s kind-0 arrays; Ncp >=
 *   sk_solve_fwd_static_cols(0, Nc) = 2 NUp, NUp = max(80, ceil8((Nc + 1) / 2)));  edges: what sk_solve_fwd_static_* (kind 0, edges, Mrows = *mrows) kept, *edge_doubles per pair;
 *   gpart [P][*rows][*outw = fd]: per PAIR and FLIPPED coarse row (row *rows - 1 - p holds coarse row p); summed over the pairs of an
 *   x_a and flipped back it is the T of sk_linear_adjoint_*: dL/dx[m] = s^2 (T[m-1] - T[m]).  Rescue arguments as above.  dyadic 0..2. */
int sk_linear_adjoint_fused_mb_layout(int64_t P, int Mc, int Nc, int dyadic, int D, int *mrows, int *rows, int *outw, int64_t *edge_doubles,
                                      size_t *workspace_bytes);
int sk_linear_adjoint_fused_mb_f64(const double *dXr, const double *dYt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D, int fd,
                                   int dyadic, int scheme, const double *edges, const double *scale, double *gpart, size_t gpart_doubles,
                                   double *err, void *workspace, size_t workspace_bytes, const double *kfinal, double screen, double tol,
                                   void *rescue_ws, size_t rescue_ws_bytes, void *stream);

/* Device-side rescue of the two fused adjoints above (csrc/sk_adj_fused_rescue.hip) -- what makes a backward pass free of host
 * synchronisation.  The fused adjoints recompute K backwards from its terminal edges, which loses accuracy like 1e-16 K^2 and is
 * useless for exploding kernels; the reference stores both grids for every pair whatever K's size (sigkernel.py:438-470).
 *   rescue_ws (sk_fused_rescue_workspace_bytes; NULL: no rescue -- the residuals in err are then the caller's to act on), with
 *   kfinal [P] = the forward values K[MM][NN] (nullable): pairs with |kfinal| > screen are taken out of the sweep (their err entry
 *   becomes -1) and their EXACT contribution (stored-grid adjoint + static-kernel chain rule) is added to the partial sums after it;
 *   a chunk in which a pair that was not screened still ends with a residual above `tol` -- or with a NaN residual while its
 *   forward value is finite (an overflow of the recompute, not poisoned inputs) -- is recomputed exactly, all its pairs.
 *   With kfinal the library initialises err itself.  When nothing is screened or fails (the normal case) the rescue reads P
 *   doubles and returns.  `blocks` flagged chunks are processed concurrently (1..1024; the workspace grows with it). */
size_t sk_fused_rescue_workspace_bytes(int kind, int64_t P, int Mc, int Nc, int dyadic, int blocks);

/* Second-argument adjoint (Gram only): dL/dY from W for the pairs (a, b), b >= b0 -- the counterpart of sk_static_adjoint_*
 * that the reference never needs (it returns no gradient for its second argument, sigkernel.py:343, :412).  It exists for
 * compute_Gram(X, X, sym=True) with a gradient: only the blocks on and above the diagonal are solved, and a pair (a, b)
 * above the diagonal also stands for (b, a), whose first-argument gradient is this pair's second-argument one.
 *   W [A*B, M-1, ldw], scale [A*B] nullable (the caller passes the TRANSPOSED upstream gradient block).
 *   kind 0 (linear, D <= 8): dXr [A][Mrows][8] fp64 = param^2 (x[p+1]-x[p]) zero-padded (the layout of sk_solve_fwd_linear_*'s array,
 *                    WITHOUT its kappa = sk_linear_prescale(dyadic) factor), X, Y unused; out = T2 [B-b0, N-1, D], the caller forms dL/dy[b][n] = T2[b][n-1] - T2[b][n].
 *   kind 1 (rbf):    dXr unused; out = dL/dY [B-b0, N, D]. */
int sk_static_adjoint2_f64(int kind, double param, const double *X, const double *Y, const double *dXr, int Mrows,
                           const double *W, int64_t ldw, const double *scale, int64_t A, int64_t B, int b0, int M, int N, int D,
                           double *out, void *stream);
int sk_static_adjoint2_f32(int kind, double param, const float *X, const float *Y, const double *dXr, int Mrows, const float *W,
                           int64_t ldw, const float *scale, int64_t A, int64_t B, int b0, int M, int N, int D, float *out,
                           void *stream);

/* Transpose of sk_increments_*, used by the adjoint: dG[p][m][n] = s_p * (W[m-1][n-1] + W[m][n]
 * - W[m-1][n] - W[m][n-1]) with out-of-range W = 0 and s_p = scale[p] (or 1 if scale == NULL).
 * Replaces the finite-difference contraction at sigkernel.py:313-341 / :472-500 (the reference
 * differentiates the increments numerically with h = 1e-9; here dL/dG_static is formed
 * exactly and the static kernel is differentiated by the caller).
 * W [P,M-1,ldw] (row stride ldw >= N-1, 0 = dense), scale [P] -> dG [P,M,N]. */
int sk_increments_adjoint_f64(const double *W, int64_t ldw, const double *scale, int64_t P, int M, int N, double *dG,
                              void *stream);
int sk_increments_adjoint_f32(const float *W, int64_t ldw, const float *scale, int64_t P, int M, int N, float *dG,
                              void *stream);

/* ---- path staging for the fused solvers -----------------------------------------------------
 * Builds, in one launch, one of the two fp64 zero-padded arrays the fused kernels below read, from the caller's dense
 * X [A,M,D] of either precision (replaces the tensor arithmetic the reference runs before its solver launch,
 * static_kernels.py:26-33 / :58-73):
 *   diff = 1: scale * (x[p+1] - x[p]), p < M-1 (differences of the up-cast points);  diff = 0: scale * x[p], p < M;
 *   dim_major = 0: out [A][rows][fd] (the `dXr` / `Xr` layout);  dim_major = 1: out [A][fd][rows] (`dYt` / `Yt`, rows = Ncp);
 *   dim_major = 2 (f32 entry point, diff = 0, fd and rows even): per path fd/2 rows of FLOAT [rows/2][4], the 4 floats of a unit =
 *   {dim 2j col 2u, dim 2j col 2u+1, dim 2j+1 col 2u, dim 2j+1 col 2u+1}, then one row of DOUBLE |x_p|^2 [rows]: (fd/2 + 1) * rows * 8
 *   bytes per path (the fp32 ring of sk_solve_fwd_static_f32);
 *   rows >= M-1 (diff) or M; fd >= D; everything outside the valid range is written as zero. */
int sk_prep_paths_f64(const double *X, int64_t A, int M, int D, int diff, int dim_major, double scale, double *out, int rows, int fd,
                      void *stream);
int sk_prep_paths_f32(const float *X, int64_t A, int M, int D, int diff, int dim_major, double scale, double *out, int rows, int fd,
                      void *stream);
/* Both arrays of a call in ONE launch: out_x [A][rows_x][fd] (dim_major = 0) from X scaled by scale_x and out_y [B][fd][rows_y]
 * (dim_major = 1) from Y scaled by scale_y; small calls are launch-bound. */
int sk_prep_pair_f64(const double *X, int64_t A, int M, const double *Y, int64_t B, int N, int D, int diff, double scale_x, double scale_y,
                     double *out_x, int rows_x, double *out_y, int rows_y, int fd, void *stream);
int sk_prep_pair_f32(const float *X, int64_t A, int M, const float *Y, int64_t B, int N, int D, int diff, double scale_x, double scale_y,
                     double *out_x, int rows_x, double *out_y, int rows_y, int fd, void *stream);

/* ---- forward solve ------------------------------------------------------------------------
 * Solves the Goursat PDE for every pair and returns K[MM][NN].
 * Replaces sigkernel_cuda[A,T](...) (sigkernel.py:231; kernel cuda_backend.py:6-49),
 * sigkernel_Gram_cuda[(A,B),T](...) (sigkernel.py:378; cuda_backend.py:121-160) and their CPU
 * twins sigkernel_cython / sigkernel_Gram_cython (sigkernel.py:246, :395;
 * cython_backend.pyx:7-33, :64-119).  Unlike the reference there is no 1024-thread limit
 * (sigkernel.py:222, :368) and no out-of-bounds extra row/column.
 *   inc_c     [P,Mc,ld]  coarse increments, row stride ld
 *   out_final [P]        K[MM][NN]
 *   out_grid  nullable   [P,MM+1,NN+1] full solution grid (what the reference returns)
 *   out_edges nullable   [P,MM+NN+2]: K[MM][0..NN] followed by K[0..MM][NN] -- the terminal
 *                        row and column.  Like out_grid it is served by the anti-diagonal kernel
 *                        (bit-identical to the reference); sk_solve_adj_* obtains the edges it needs
 *                        from the strip kernel directly, in that kernel's own padded layout. */
int sk_solve_fwd_f64(const double *inc_c, int64_t ld, int64_t P, int Mc, int Nc, int dyadic, int scheme, int flags,
                     double *out_final, double *out_grid, double *out_edges, void *stream);
int sk_solve_fwd_f32(const float *inc_c, int64_t ld, int64_t P, int Mc, int Nc, int dyadic, int scheme, int flags,
                     float *out_final, float *out_grid, double *out_edges, void *stream);

/* Forward solve of pairs of UNEQUAL length in one padded batch: ONE node per pair, no grid.  out[p] = K_p at node (mc << dyadic,
 * nc << dyadic) of the padded pair's fine grid, i.e. the solution of pair p's own (mc, nc) coarse cells -- what sk_solve_fwd_* with
 * out_grid stores at that node, without the (MM+1)(NN+1) elements per pair around it.
 *   inc_c [P,Mc,ld]  as sk_solve_fwd_*: whatever cells a >= mc or b >= nc hold (NaN, inf) reaches no result
 *   cells [P][2]     device int32 {mc, nc}: the coarse cells of pair p's own sub-grid, len - 1 on either side (the layout of
 *                    SK_FLAG_RAGGED's table); values are clamped to [0, Mc] and [0, Nc]; the only address formed from an entry is out + p
 *   out   [P]        a pair with mc == 0 or nc == 0 is left alone or stored as exactly 1: the CALLER fills out with ones first (the
 *                    contract of sk_solve_prefix_at_*)
 *   flags 0: the streaming kernel (csrc/sk_wave.hip) where it serves the shape and layout (dyadic <= 3, 16-byte aligned rows, cells
 *            8-byte aligned) -- the PADDED sweep with the pair's own lane, unit and cell storing -- else the anti-diagonal kernel;
 *         SK_FLAG_SIMPLE / SK_FLAG_EXACT: the anti-diagonal kernel (csrc/sk_simple.hip) over each pair's own sub-grid: the cost of the
 *            pair's true lengths, and bit for bit the node of its stored grid;
 *         SK_FLAG_FAST_ONLY: SK_ERR_UNSUPPORTED where the streaming kernel declines.
 * No kernel instance of its own: a launch-time mode of k_fwd_wave's non-edge instances and of k_fwd_simple. */
int sk_solve_fwd_at_f64(const double *inc_c, int64_t ld, int64_t P, int Mc, int Nc, int dyadic, int scheme, int flags, const int *cells,
                        double *out, void *stream);
int sk_solve_fwd_at_f32(const float *inc_c, int64_t ld, int64_t P, int Mc, int Nc, int dyadic, int scheme, int flags, const int *cells,
                        float *out, void *stream);

/* Forward solve of a PIECE of Nc coarse columns that starts from a kept fine column instead of the constant 1: what a stream off the
 * fused prefix kernel's scope appends with.  Pair p's grid has been swept up to some coarse column before; col_in holds K on that fine
 * column, inc_c the increments of the Nc coarse columns behind it.  Every cell is evaluated from the same operands in the same order as
 * in sk_solve_fwd_*'s one-shot sweep of the whole grid with out_grid (the anti-diagonal kernel, csrc/sk_simple.hip, -ffp-contract=off),
 * so the piece's cells are that grid's bit for bit, any dyadic order, both schemes.  MM = Mc << dyadic, NN = Nc << dyadic.
 *   inc_c   [P,Mc,ld]    as sk_solve_fwd_* (ld = 0: Nc), the piece's columns only
 *   col_in  [P][MM + 1]  doubles (fp64 whatever the increments' type): element i = K at fine row i of the column the piece starts at,
 *                        1 <= i <= MM.  Element 0 of a slot is NEVER READ (row 0 of a grid is the constant 1).  A first piece starts
 *                        from a column of ones.
 *   col_out [P][MM + 1]  doubles: element i = K[i][NN], the piece's terminal column, written for 1 <= i <= MM.  Element 0 of a slot is
 *                        NOT WRITTEN: it is the caller's.  Must not overlap col_in (SK_ERR_BAD_ARG): callers alternate two arrays.
 *   row     [P][NN + 1]  doubles: element j = K[MM][j], the terminal row over the piece, written for 1 <= j <= NN; element 0 (the
 *                        corner K[MM][0] = col_in[MM]) is NOT WRITTEN.  The coarse nodes are elements (1..Nc) << dyadic.
 * SK_ERR_UNSUPPORTED where a bank path does not fit the kernel's three LDS diagonals (sk_solve_fwd_resume_fits says so beforehand);
 * every check comes before any device call.  No kernel instance of its own: a launch-time mode of k_fwd_simple. */
int sk_solve_fwd_resume_f64(const double *inc_c, int64_t ld, int64_t P, int Mc, int Nc, int dyadic, int scheme, const double *col_in,
                            double *col_out, double *row, void *stream);
int sk_solve_fwd_resume_f32(const float *inc_c, int64_t ld, int64_t P, int Mc, int Nc, int dyadic, int scheme, const double *col_in,
                            double *col_out, double *row, void *stream);
/* 1 where first paths of Mc coarse cells at this dyadic order fit sk_solve_fwd_resume_* (3 * 8 * ((Mc << dyadic) + 1) bytes of LDS
 * within 160 KiB), else 0.  Host only. */
int sk_solve_fwd_resume_fits(int Mc, int dyadic);

/* Forward solve with the LINEAR static kernel fused in (csrc/sk_wave_fused.hip): the increments
 * s^2 <x[p+1]-x[p], y[q+1]-y[q]> are formed inside the sweep, nothing of size P*M*N ever exists in HBM.
 * Replaces, for LinearKernel, the whole of sigkernel.py:362-382 (Gram) / :216-234 (paired).
 *   dXr [A][Mrows][8] fp64: kappa s^2 (x[p+1]-x[p]) for p < Mc, kappa = sk_linear_prescale(dyadic) = 4^-d / sqrt(12) (the
 *                           kernel's stencil coefficients take three operations per coarse cell on the pre-scaled increment);
 *                           zero for the padding rows (Mrows >= 256 is always enough) and padding dims (path dim <= 8);
 *   dYt [Bn][8][Ncp] fp64: y[q+1]-y[q], dimension-major, zero-padded; Ncp = Nc rounded up to a multiple of 16;
 *   B > 0: Gram (Bn = B, pair (a,b) at a*B+b); B == 0: paired (Bn = A).  out_final [P].
 *   D = the path dimension (1..8): dimensions >= D of dXr / dYt must be zero; D <= 4 selects kernels that skip them.
 *   queue: 64 bytes of device scratch for the launch's work counter (contents irrelevant, the library zeroes it on `stream`;
 *          not shared with a launch that may run concurrently).  The waves of these persistent kernels take a fixed first share
 *          of the pairs and draw the rest from that counter, so that they finish together whatever the SIMD arbitration, the
 *          XCDs' clocks or other work on the chip do.  NULL: a static, equal partition (the results are the same bit for bit).
 * SK_ERR_UNSUPPORTED when dyadic > 2 or a pair needs more than one band (M-1 > 256/128/64 for dyadic 0/1/2):
 * use sk_static_increments_* + sk_solve_fwd_*. */
int sk_solve_fwd_linear_f64(const double *dXr, const double *dYt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D,
                            int dyadic, int scheme, double *out_final, void *queue, void *stream);
int sk_solve_fwd_linear_f32(const double *dXr, const double *dYt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D,
                            int dyadic, int scheme, float *out_final, void *queue, void *stream);

/* Forward solve with the RBF static kernel fused in (csrc/sk_wave_fused.hip, KIND 1): the nodes
 * G[p][q] = exp(-|x_p - y_q|^2 / sigma) are evaluated inside the sweep (one exp per coarse cell; a lane takes the node row
 * under its last coarse row from the lane below by DPP) and differenced in the reference's order
 * ((G11 + G00) - G10) - G01; neither G_static nor the increments exist in HBM.  Replaces, for RBFKernel,
 * static_kernels.py:58-73 + sigkernel.py:362-382 (Gram) / static_kernels.py:43-56 + sigkernel.py:216-234 (paired).
 * |x - y|^2 is summed directly over the dimensions, not as |x|^2 + |y|^2 - 2<x,y>.
 *   Xr [A][Mrows][8] fp64: the path POINTS x_p, p < M = Mc + 1, zero padding rows / dims (path dim <= 8);
 *   Yt [Bn][8][Ncp] fp64: y_q, q < N = Nc + 1, dimension-major, zero-padded; Ncp = N rounded up to a multiple of 16;
 *   inv_sigma = 1 / sigma;  B > 0: Gram, B == 0: paired;  out_final [P];  D as for sk_solve_fwd_linear_*.
 * SK_ERR_UNSUPPORTED when dyadic > 2 or a pair needs more than one band (M > 256/128/64 for dyadic 0/1/2; at dyadic 0 the
 * four-rows-per-lane kernel is built for D <= 4, the default scheme and fp64 output: D 5..8, SK_SCHEME_NAIVE and sk_solve_fwd_rbf_f32
 * take two rows per lane there, M <= 128, and sk_solve_fwd_rbf_edges_f64 does not cover them): use sk_static_increments_* +
 * sk_solve_fwd_*, or sk_solve_fwd_static_*; sk_route_query says which. */
int sk_solve_fwd_rbf_f64(const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D,
                         int dyadic, int scheme, double inv_sigma, double *out_final, void *queue, void *stream);
int sk_solve_fwd_rbf_f32(const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D,
                         int dyadic, int scheme, double inv_sigma, float *out_final, void *queue, void *stream);
/* The same four calls for a caller whose `queue` holds queue_words >= 1 zero-initialisable 64-bit counters instead of one
 * (sk_solve_fwd_linear_* / sk_solve_fwd_rbf_* are these with queue_words = 1).  A plain Gram launch (B > 0) whose pairs share their
 * y columns across a wave's lane groups (two or more pairs per wave) is then dealt out BY GRAM ROW-BLOCK where ceil(A / G) counters
 * are there and the row-blocks divide the resident waves evenly (sk_plan_row_dealing says whether and how): a wave stays with the
 * x rows of one row-block for as long as that has work, and fetches them once.  The library zeroes the counters it uses.  Same
 * results, bit for bit.  A / 2 + 1 counters are always enough. */
int sk_solve_fwd_linear_rows_f64(const double *dXr, const double *dYt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D,
                                 int dyadic, int scheme, double *out_final, void *queue, int64_t queue_words, void *stream);
int sk_solve_fwd_linear_rows_f32(const double *dXr, const double *dYt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D,
                                 int dyadic, int scheme, float *out_final, void *queue, int64_t queue_words, void *stream);
int sk_solve_fwd_rbf_rows_f64(const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D,
                              int dyadic, int scheme, double inv_sigma, double *out_final, void *queue, int64_t queue_words, void *stream);
int sk_solve_fwd_rbf_rows_f32(const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D,
                              int dyadic, int scheme, double inv_sigma, float *out_final, void *queue, int64_t queue_words, void *stream);
/* Host only, no device call: how the one-band fused forward deals the stream positions of an A x B Gram launch to its waves
 * (csrc/sk_pair_stream.h: plan_pair_stream, plan_row_dealing).  G = 64 / L lane groups per wave of L lanes per pair, NUp padded
 * two-column units per pair, lag 0 (linear) or 2 (rbf), waves_per_cu resident waves on each of n_cu compute units, pct per cent of the
 * equal share dealt out up front, queue_words counters (0: no queue).  G >= 2: the shared-y order, ceil(A / G) B positions, position
 * q = row-block q / B, column q % B; G = 1: A B positions, no row-blocks.
 *   plan[0] mode (1: row-local dealing), [1] waves, [2] largest share per wave, [3] q_first, [4] C0, [5] n_big, [6] logC,
 *   [7] the counter is used, [8] waves per row-block, [9] row-blocks = counters used, [10] row_q0, [11] row_rem, [12] queues;
 *   static_first / static_end [waves_cap]: wave w's up-front positions [first, end) (NULL: not wanted; waves > waves_cap: SK_ERR_BAD_ARG);
 *   queue_first / queue_end [queues_cap]: the positions [first, end) each counter hands out, 2^logC at a time (mode 0: one counter
 *   from q_first to the end; no queue: none).
 * Together these ranges are every position exactly once.  Mode 0 is the plan of a launch without the *_rows_* counters, field for field. */
int sk_plan_row_dealing(int64_t A, int64_t B, int G, int NUp, int L, int lag, int waves_per_cu, int n_cu, int pct, int64_t queue_words,
                        int64_t *plan, int64_t waves_cap, int64_t *static_first, int64_t *static_end, int64_t queues_cap,
                        int64_t *queue_first, int64_t *queue_end);
/* The PREFIX GRID of every pair with the static kernel fused in (csrc/sk_wave_prefix.hip): the sweep of sk_solve_fwd_linear_* /
 * sk_solve_fwd_rbf_* that stores every coarse node instead of the last one,
 *     out[p ldo + m (Nc + 1) + n] = k_sig(x[:m+1], y[:n+1]),   1 <= m <= Mc, 0 <= n <= Nc
 * (node (m << dyadic, n << dyadic) of the reference's grid; column n = 0 is exactly 1).  Row m = 0 of every grid -- the ones of the
 * one-point prefix of x, Nc + 1 contiguous elements -- is NOT written: it is the caller's fill.  Nothing outside a pair's
 * (Mc + 1) x (Nc + 1) elements is written.  Where Nc + 1 and ldo are even and out is aligned to two elements the nodes are stored two
 * columns at a time (SK_PREFIX_STORE=1|2|3 in the environment selects a store scheme for measurements; the values are the same).
 * Node (Mc, Nc) is bit for bit the out_final of sk_solve_fwd_linear_* / sk_solve_fwd_rbf_* on the same staged arrays.
 *   dXr / dYt (Xr / Yt), A, B, Mrows, Mc, Nc, Ncp, D, dyadic, scheme, inv_sigma, queue: as sk_solve_fwd_linear_* / sk_solve_fwd_rbf_*;
 *   out: pair p's grid starts at out + p ldo, rows are dense (pitch Nc + 1); ldo >= (Mc + 1) (Nc + 1) elements, so that a caller
 *        can write into a slice of a larger tensor; _f32: the sweep is fp64, the nodes are stored as float.
 * SK_ERR_UNSUPPORTED outside sk_route_query(SK_OP_PREFIX, ...) == SK_ROUTE_FUSED: use sk_static_increments_* + sk_solve_fwd_*
 * with out_grid. */
int sk_solve_prefix_linear_f64(const double *dXr, const double *dYt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D,
                               int dyadic, int scheme, double *out, int64_t ldo, void *queue, void *stream);
int sk_solve_prefix_linear_f32(const double *dXr, const double *dYt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D,
                               int dyadic, int scheme, float *out, int64_t ldo, void *queue, void *stream);
int sk_solve_prefix_rbf_f64(const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D,
                            int dyadic, int scheme, double inv_sigma, double *out, int64_t ldo, void *queue, void *stream);
int sk_solve_prefix_rbf_f32(const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D,
                            int dyadic, int scheme, double inv_sigma, float *out, int64_t ldo, void *queue, void *stream);
/* A SLICE of the prefix grid alone -- the same sweep of the same kernel, storing only the nodes of the slice, so a call is not bound by
 * pairs x (Mc + 1) x (Nc + 1) stores nor by that much memory.  nodes:
 *   SK_NODES_DIAGONAL  out[p ldo + t] = k_sig(x[:t+1], y[:t+1]),  1 <= t <= min(Mc, Nc);   ldo >= min(Mc, Nc) + 1
 *   SK_NODES_LAST_ROW  out[p ldo + n] = k_sig(x, y[:n+1]),        1 <= n <= Nc;            ldo >= Nc + 1
 *   SK_NODES_LAST_COL  out[p ldo + m] = k_sig(x[:m+1], y),        1 <= m <= Mc;            ldo >= Mc + 1
 *   SK_NODES_ALL       the call above (out, ldo as there).
 * Element 0 of every slice -- exactly 1 -- is NOT written: it is the caller's fill.  Nothing else outside those elements is written.
 * Every element is bit for bit the node sk_solve_prefix_* stores there.  Other arguments, scope and errors: as sk_solve_prefix_*. */
#define SK_NODES_ALL 0
#define SK_NODES_DIAGONAL 1
#define SK_NODES_LAST_ROW 2
#define SK_NODES_LAST_COL 3
int sk_solve_prefix_nodes_linear_f64(const double *dXr, const double *dYt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D,
                                     int dyadic, int scheme, int nodes, double *out, int64_t ldo, void *queue, void *stream);
int sk_solve_prefix_nodes_linear_f32(const double *dXr, const double *dYt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D,
                                     int dyadic, int scheme, int nodes, float *out, int64_t ldo, void *queue, void *stream);
int sk_solve_prefix_nodes_rbf_f64(const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D,
                                  int dyadic, int scheme, double inv_sigma, int nodes, double *out, int64_t ldo, void *queue, void *stream);
int sk_solve_prefix_nodes_rbf_f32(const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D,
                                  int dyadic, int scheme, double inv_sigma, int nodes, float *out, int64_t ldo, void *queue, void *stream);
/* The LAST ROW over a second path that GROWS: the sweep of sk_solve_prefix_nodes_*(SK_NODES_LAST_ROW) RESUMED from a kept column, so
 * that a stream y scored against complete paths x costs its new points, not its history.  All that crosses a column of a pair is one
 * column of the fine grid; a launch over the piece y[s:] that starts from column s (col_in) instead of the ones repeats the cells of
 * a launch over the whole of y, with the same operands in the same order:
 *     out[p ldo + n] = k_sig(x, y[:s + n + 1]),   1 <= n <= Nc        (Nc + 1 = the points of the piece; Yt / dYt stage the PIECE)
 * -- every element bit for bit the node sk_solve_prefix_* stores at global column s + n of the whole stream.  Element 0 of every slice
 * is NOT written (with col_in it is not 1 but the last row's node at column s, which the caller has from the launch before).
 *   col_in:  null (a first launch: s = 0, the column of ones) or [pairs][ld_col] doubles, pair p = a B + b (Gram) or a (paired):
 *            element i of a slot = K at fine row i + 1, fine column s << dyadic, i < Mc << dyadic.  Read, never written.
 *   col_out: null, or the same layout: the column behind unit state_unit - 1 of the launch, i.e. global coarse column
 *            s + 2 state_unit, 1 <= state_unit <= Nc / 2 (SK_ERR_BAD_ARG otherwise; state_unit = 0 with col_out null).  The state sits at
 *            an EVEN coarse column of the piece, so s must stay even from launch to launch: a caller keeps the
 *            Nc + 1 - 2 state_unit (1 or 2) last points behind the state and passes them again in front of the next piece.
 *            Elements i < Mc << dyadic of every slot are written, plain stores; nothing else is.
 *   ld_col:  doubles between the slots, >= sk_prefix_state_pitch(Mc, dyadic, kind) and even; both arrays 16-byte aligned and not
 *            overlapping (SK_ERR_BAD_ARG).  Elements [Mc << dyadic, ld_col) of a slot are the caller's: the kernel may read them from
 *            col_in (any bits, uninitialised memory included: no result depends on them) and never writes them in col_out.
 *   The state is fp64 whatever the output dtype: _f32 streams resume bit for bit too.
 * Other arguments, scope and errors: as sk_solve_prefix_*. */
int sk_solve_prefix_resume_linear_f64(const double *dXr, const double *dYt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D,
                                      int dyadic, int scheme, double *out, int64_t ldo, const double *col_in, double *col_out, int64_t ld_col,
                                      int state_unit, void *queue, void *stream);
int sk_solve_prefix_resume_linear_f32(const double *dXr, const double *dYt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D,
                                      int dyadic, int scheme, float *out, int64_t ldo, const double *col_in, double *col_out, int64_t ld_col,
                                      int state_unit, void *queue, void *stream);
int sk_solve_prefix_resume_rbf_f64(const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D,
                                   int dyadic, int scheme, double inv_sigma, double *out, int64_t ldo, const double *col_in, double *col_out,
                                   int64_t ld_col, int state_unit, void *queue, void *stream);
int sk_solve_prefix_resume_rbf_f32(const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D,
                                   int dyadic, int scheme, double inv_sigma, float *out, int64_t ldo, const double *col_in, double *col_out,
                                   int64_t ld_col, int state_unit, void *queue, void *stream);
/* Doubles of one pair's kept column for sk_solve_prefix_resume_*: the Mc << dyadic fine rows rounded up to whole lanes of the kernel
 * (always even).  Host only.  0: dyadic outside 0 .. 2, kind outside 0 / 1 or Mc < 1. */
int64_t sk_prefix_state_pitch(int Mc, int dyadic, int kind);
/* ONE NODE per pair: batches of paths of unequal length, padded at their ends to a common length (any finite values).  The same sweep
 * of the same kernel over the padded pair, storing only
 *     out[p] = k_sig(x_a[:len_x[a]], y_b[:len_y[b]])        (node (len_x[a] - 1, len_y[b] - 1) of pair p's grid, bit for bit)
 * p = a B + b for a Gram launch (B > 0), p = a = b for a paired one (B == 0): A B resp. A elements, nothing else is written and nothing
 * of size pairs x (Mc + 1) x (Nc + 1) exists.  A pair with len_x[a] == 1 or len_y[b] == 1 -- value exactly 1 -- is NOT written: the
 * caller fills `out` with ones before the call.
 *   out: aligned to its element size (4 / 8 bytes), as any float * / double * is: the kernel keeps a row number in the two low bits of
 *   out + p.
 *   len_x: A device int32 point counts; len_y: B of them (paired launch: A, indexed by the pair).  Both required (SK_ERR_BAD_ARG).
 *   The lengths are NOT validated on the device: the caller guarantees 1 <= len_x[a] <= Mc + 1 and 1 <= len_y[b] <= Nc + 1.  A length
 *   outside that range leaves the pair's element unwritten or holding another node of the pair; nothing is accessed out of bounds, the
 *   only address formed is out + p.
 * Other arguments, scope and errors: as sk_solve_prefix_*.  SK_NODES_AT names the kernel's store mode; sk_solve_prefix_nodes_* does not
 * accept it (it has no length arguments). */
#define SK_NODES_AT 4
int sk_solve_prefix_at_linear_f64(const double *dXr, const double *dYt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D,
                                  int dyadic, int scheme, const int *len_x, const int *len_y, double *out, void *queue, void *stream);
int sk_solve_prefix_at_linear_f32(const double *dXr, const double *dYt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D,
                                  int dyadic, int scheme, const int *len_x, const int *len_y, float *out, void *queue, void *stream);
int sk_solve_prefix_at_rbf_f64(const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D,
                               int dyadic, int scheme, double inv_sigma, const int *len_x, const int *len_y, double *out, void *queue,
                               void *stream);
int sk_solve_prefix_at_rbf_f32(const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D,
                               int dyadic, int scheme, double inv_sigma, const int *len_x, const int *len_y, float *out, void *queue,
                               void *stream);
/* The truncated signature kernel of Kiraly and Oberhauser as ONE sweep per pair (replaces truncated_sig_kernel, transformers.py:201-236:
 * six-dimensional numpy arrays shifted by a spline filter): out[a][b] = sigma[0] + sum_{m = 1 .. num_levels} sigma[m] * (sum of level m's
 * planes over the step grid of (x_a, y_b)); the rows of the paths are used as STEPS (no differencing); order = num_levels (or < 1) is the
 * signature kernel truncated at num_levels, smaller orders are the reference's lower-order approximations.
 *   Xr [A][Mrows][fd] / Yt [B][fd][Ncp]: the path POINTS staged by sk_prep_pair_* (diff = 0, scales 1), fd = 8 for D <= 8 else 16,
 *   Mrows >= M, Ncp >= N;  sigma: num_levels + 1 doubles in HOST memory;  out [A][B]; _f32: the sweep is fp64, the result is stored as float.
 * Forward only.  SK_ERR_UNSUPPORTED outside sk_route_query(SK_OP_TRUNCATED, order, D, M, N, num_levels, ...) == SK_ROUTE_FUSED. */
int sk_truncated_gram_f64(const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int M, int N, int Ncp, int D, int fd,
                          int num_levels, int order, const double *sigma, double *out, void *stream);
int sk_truncated_gram_f32(const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int M, int N, int Ncp, int D, int fd,
                          int num_levels, int order, const double *sigma, float *out, void *stream);
/* The same sweep on P PAIRS: out[p] = the truncated kernel of (x_p, y_p) -- what a normalised kernel k(x, y) / sqrt(k(x, x) k(y, y))
 * needs of every path, without the P x P matrix around it.  A launch-time mode of the Gram kernel's instances: each lane group of a wave
 * takes a pair of its own and keeps that pair's y block in LDS (the groups are widened until the blocks of a wave fit its 16 KB).
 *   Xr [P][Mrows][fd] / Yt [P][fd][Ncp], sigma, order and the _f32 rule as above;  out [P].
 * Forward only.  The scope is the Gram entry points': SK_ERR_UNSUPPORTED outside sk_route_query(SK_OP_TRUNCATED, ...) == SK_ROUTE_FUSED;
 * for SK_ROUTE_FUSED_SWAP call it on (y, x): the recursion is symmetric, so the values need no transposing. */
int sk_truncated_paired_f64(const double *Xr, const double *Yt, int64_t P, int Mrows, int M, int N, int Ncp, int D, int fd, int num_levels,
                            int order, const double *sigma, double *out, void *stream);
int sk_truncated_paired_f32(const double *Xr, const double *Yt, int64_t P, int Mrows, int M, int N, int Ncp, int D, int fd, int num_levels,
                            int order, const double *sigma, float *out, void *stream);
/* The LEVEL TERMS of the truncated kernel, all of them from the one sweep: out[m][a][b] = k_m(x_a, y_b) = the sum of level m's planes over
 * the step grid, m = 1 .. num_levels, and out[0] = 1, so that sk_truncated_gram_* with weights sigma is sum_m sigma[m] out[m] (replaces
 * num_levels + 1 calls of truncated_sig_kernel, transformers.py:201-236, with unit-vector sigma: the reference has no per-level output).
 * Every truncation 1 .. num_levels, every choice of level weights and every rescaling of the paths (k_m(c x, y) = c^m k_m(x, y)) is a
 * weighted sum of these planes.  A launch-time mode of the Gram kernel's instances: the step loop is the plain launch's, the levels below
 * the last are the row sums it keeps anyway, reduced per level after the loop; num_levels + 1 stores per pair.
 *   Xr, Yt, order, the _f32 rule and the scope as sk_truncated_gram_*;  out [num_levels + 1][A][B], every plane a contiguous matrix. */
int sk_truncated_levels_f64(const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int M, int N, int Ncp, int D, int fd,
                            int num_levels, int order, double *out, void *stream);
int sk_truncated_levels_f32(const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int M, int N, int Ncp, int D, int fd,
                            int num_levels, int order, float *out, void *stream);
/* ... and of the P PAIRS (x_p, y_p): out [num_levels + 1][P], the paired mode of sk_truncated_paired_* with the level output above
 * (replaces num_levels + 1 calls of truncated_sig_kernel per pair with unit-vector sigma, transformers.py:201-236, keeping [0][0]).  With
 * y = x these are the squared norms of the signature levels of every path: what a per-path rescaling is solved from. */
int sk_truncated_levels_paired_f64(const double *Xr, const double *Yt, int64_t P, int Mrows, int M, int N, int Ncp, int D, int fd,
                                   int num_levels, int order, double *out, void *stream);
int sk_truncated_levels_paired_f32(const double *Xr, const double *Yt, int64_t P, int Mrows, int M, int N, int Ncp, int D, int fd,
                                   int num_levels, int order, float *out, void *stream);
/* The same sweep with the static kernel as a launch-time mode, every output mode behind ONE entry point (no counterpart in the reference,
 * whose truncated kernel knows inner products of steps only).  kind 0: Xr / Yt hold steps and the call is sk_truncated_gram_* (paired = 0,
 * levels = 0), _paired_* (paired = 1: A pairs, B ignored), _levels_* or _levels_paired_* (levels = 1: sigma is not read and may be NULL).
 * kind 1: Xr / Yt hold the M / N POINTS of the paths (at least 2 each) and the sweep runs on the M x N grid of points with
 * G[i][j] = kap(x_i, y_j) - kap(x_i, y_{j-1}) - kap(x_{i-1}, y_j) + kap(x_{i-1}, y_{j-1}), kap(x, y) = exp(-|x - y|^2 param), param = 1 / sigma
 * of RBFKernel > 0, zero in row 0 and column 0: the kernel of Kiraly and Oberhauser lifted through the RBF kernel.  kap is evaluated in
 * the sweep from differences of coordinates (two polynomials per node and row: exp of the node, expm1 of the exponents' difference along
 * the row); nothing of size pairs x M x N exists.
 *   Staging, sigma, order, out and the _f32 rule as the kind-0 entry points'.  Forward only.
 * Scope: kind 0 as sk_truncated_gram_*; kind 1: sk_route_query(SK_OP_TRUNCATED_RBF, order, D, M, N, num_levels, ...) == SK_ROUTE_FUSED. */
int sk_truncated_points_f64(const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int M, int N, int Ncp, int D, int fd,
                            int num_levels, int order, int kind, double param, int paired, int levels, const double *sigma, double *out,
                            void *stream);
int sk_truncated_points_f32(const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int M, int N, int Ncp, int D, int fd,
                            int num_levels, int order, int kind, double param, int paired, int levels, const double *sigma, float *out,
                            void *stream);
/* The same sweep on paths of ANY length, order 1, forward only (kind 0: Xr / Yt hold steps): the rows go in bands of 128 -- what the last
 * row of a band hands down is carried to the next band through `slab` -- and the columns in tiles of the wave's y block (2048 / fd).
 *   sk_truncated_long_plan  plan[0..2] = blocks, slab bytes of ONE block, slab bytes of the launch.  A block's slab is
 *                           (num_levels - 1) x ceil64(N) doubles, and none when M <= 128 (one band) or num_levels = 1; the blocks are
 *                           lowered from 8 per CU until their slabs fit workspace_bytes; SK_ERR_UNSUPPORTED when one does not, or outside
 *                           the scope.  Host only.
 *   sk_truncated_long_*     Xr, Yt, Mrows, Ncp (a multiple of 16), fd, sigma, order (must resolve to 1), paired, levels and out as
 *                           sk_truncated_points_* at kind 0; slab / slab_bytes: device scratch of at least one block's slab (the launch
 *                           takes as many blocks as fit), NULL / 0 where the plan says 0.
 * Scope: sk_route_query(SK_OP_TRUNCATED_LONG, order, D, M, N, num_levels, ...) != SK_ROUTE_STREAM; else SK_ERR_UNSUPPORTED. */
int sk_truncated_long_plan(int64_t A, int64_t B, int M, int N, int D, int num_levels, int paired, size_t workspace_bytes, int64_t *plan);
int sk_truncated_long_f64(const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int M, int N, int Ncp, int D, int fd,
                          int num_levels, int order, int paired, int levels, const double *sigma, double *slab, size_t slab_bytes, double *out,
                          void *stream);
int sk_truncated_long_f32(const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int M, int N, int Ncp, int D, int fd,
                          int num_levels, int order, int paired, int levels, const double *sigma, double *slab, size_t slab_bytes, float *out,
                          void *stream);
/* The gradient of sk_truncated_adjoint (below: w, Tpart, n_chunks, the staging and the reproducibility are its) on paths of ANY length,
 * order 1, D <= 8: the reverse sweep in the bands and tiles of sk_truncated_long_*.  Per pair, with more than one band of 128 rows, one forward
 * pass that keeps every band's incoming carry, then the bands from the last to the first: the band's forward sweep again, storing its prefix
 * factors, and its mirrored sweep, which hands a reverse carry up to the band above and continues the band's rows of dX in Tpart.
 * A block's slab, in this order (W the lanes of a pair's group: 64 beyond 128 rows; tiles = ceil(N / min(ceil16(N), 256))):
 *     factors        [num_levels - 1][N + tiles (W - 1)][128] doubles: 1 KB per level and step of ONE band
 *     forward carry  [bands][num_levels - 1][ceil64(N)] doubles          (only with more than one band; plane 0 is never touched)
 *     reverse carry  [2][num_levels - 1][ceil64(N)] doubles              (only with more than one band; band k writes half k & 1)
 *   sk_truncated_long_adjoint_plan  plan[0..3] = n_chunks, blocks, slab bytes of the launch (blocks x one block's), slab bytes of ONE block.
 *                                   The blocks are lowered from 8 per CU until their slabs fit workspace_bytes; SK_ERR_UNSUPPORTED when one
 *                                   block's does not, or outside the scope.  Host only.
 *   sk_truncated_long_adjoint       arguments as sk_truncated_adjoint's, Ncp a multiple of 16; slab / slab_bytes: device scratch of at least
 *                                   one block's slab (the launch takes as many blocks as fit), may be NULL / 0 at num_levels = 1.
 * Scope: sk_route_query(SK_OP_TRUNCATED_LONG_ADJOINT, 1, D, M, N, num_levels, ...) == SK_ROUTE_FUSED; else SK_ERR_UNSUPPORTED. */
int sk_truncated_long_adjoint_plan(int64_t A, int64_t B, int M, int N, int D, int num_levels, int paired, size_t workspace_bytes,
                                   int64_t *plan);
int sk_truncated_long_adjoint(const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int M, int N, int Ncp, int D, int fd,
                              int num_levels, const double *w, double *Tpart, int64_t n_chunks, double *slab, size_t slab_bytes, void *stream,
                              int paired);
/* The gradient of sk_truncated_adjoint (below: w, n_chunks, the staging, the slab and the reproducibility are its) at path dims 9 .. 16, order 1,
 * at most 128 steps on either side: the same two sweeps per pair with rows and accumulators of 16 coordinates, by k_trunc_sig<4, 1> in its
 * wide-adjoint mode.  The chunks' parts go to Tpart [n_chunks][A][M][16]; the caller adds the chunks and keeps the first D of the 16 columns.
 *   sk_truncated_wide_adjoint_plan  plan[0..2] = n_chunks, blocks, slab bytes of the shape, the slab within workspace_bytes (the block count
 *                                   is lowered until it fits); SK_ERR_UNSUPPORTED when one block's slab, (num_levels - 1) (N + W - 1) KB with
 *                                   W the lanes of a pair's group, does not.  paired: the groups widen until G x 16 x ceil16(N) doubles fit
 *                                   the wave's 16 KB of LDS, so W can exceed ceil(M / 2).  Host only.
 *   sk_truncated_wide_adjoint       Xr, Yt, Mrows, Ncp, fd as sk_truncated_gram_* (fd = 16 required: SK_ERR_BAD_ARG otherwise, as for
 *                                   Ncp < N, a paired call with A != B, or n_chunks outside 1 .. B (paired: 1)); slab / slab_bytes: device
 *                                   scratch, may be NULL / 0 at num_levels = 1.  Scope and arguments are checked before the device is touched.
 * Scope: sk_route_query(SK_OP_TRUNCATED_WIDE_ADJOINT, 1, D, M, N, num_levels, ...) == SK_ROUTE_FUSED -- order 1, 9 <= D <= 16; else
 * SK_ERR_UNSUPPORTED. */
int sk_truncated_wide_adjoint_plan(int64_t A, int64_t B, int M, int N, int D, int num_levels, int paired, size_t workspace_bytes,
                                   int64_t *plan);
int sk_truncated_wide_adjoint(const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int M, int N, int Ncp, int D, int fd,
                              int num_levels, const double *w, double *Tpart, int64_t n_chunks, double *slab, size_t slab_bytes, void *stream,
                              int paired);
/* The GRADIENT of the level terms with respect to the first batch, by the same kernel in its adjoint mode (no counterpart in the reference,
 * whose truncated kernel is numpy): for weights w [num_levels][A][B] (device fp64; paired: [num_levels][P]) -- the upstream gradient of level
 * m + 1 of every pair -- the chunks' parts of d / dX sum_pairs sum_m w[m][pair] k_{m+1}(pair) go to Tpart [n_chunks][A][M][8]; the caller
 * adds the chunks (dX = sum over the first axis, the first D of the 8 columns).  Per pair one forward sweep that stores the num_levels - 1
 * prefix factors of every node to `slab`, and one reverse sweep that reads them back; plain stores, no atomics: bit-reproducible.
 *   sk_truncated_adjoint_plan  plan[0..2] = n_chunks, blocks, slab bytes of the shape, the slab within workspace_bytes (the block count is
 *                              lowered until it fits); SK_ERR_UNSUPPORTED when one block's slab, (num_levels - 1) (N + W - 1) KB with W the
 *                              lanes of a pair's group, does not.  Host only.
 *   sk_truncated_adjoint       Xr, Yt, Mrows, Ncp, fd as sk_truncated_gram_* (fd = 8); n_chunks in 1 .. B (paired: 1), usually the plan's;
 *                              slab / slab_bytes: device scratch, may be NULL / 0 at num_levels = 1.
 * Scope: sk_route_query(SK_OP_TRUNCATED_ADJOINT, 1, D, M, N, num_levels, ...) == SK_ROUTE_FUSED -- order 1, D <= 8; else SK_ERR_UNSUPPORTED. */
int sk_truncated_adjoint_plan(int64_t A, int64_t B, int M, int N, int D, int num_levels, int paired, size_t workspace_bytes, int64_t *plan);
int sk_truncated_adjoint(const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int M, int N, int Ncp, int D, int fd,
                         int num_levels, const double *w, double *Tpart, int64_t n_chunks, double *slab, size_t slab_bytes, void *stream,
                         int paired);
/* The same gradient for the kernel lifted through the RBF static kernel (sk_truncated_points_* with kind 1), with respect to the POINTS of
 * the first batch: Xr / Yt hold the M / N points, param = 1 / sigma of RBFKernel > 0, w and Tpart [n_chunks][A][M][8] as above.  With
 * dG the plain adjoint's gradient with respect to G on the nodes (i, c >= 1; zero elsewhere) and
 * H(i, c) = dG(i, c) - dG(i, c + 1) - dG(i + 1, c) + dG(i + 1, c + 1):  dx_i = sum_c H(i, c) kap(i, c) (-2 param) (x_i - y_c) -- the first point of a
 * path and the first column carry no node and do receive a gradient.  Two sweeps per pair as above; the slab holds one plane more, the
 * node's G beside its prefix factors: num_levels (N + W - 1) KB per block.  Plain stores, no atomics: bit-reproducible.
 *   sk_truncated_points_adjoint_plan  plan[0..2] as sk_truncated_adjoint_plan's.  Host only.
 *   sk_truncated_points_adjoint       n_chunks in 1 .. B (paired: 1), usually the plan's; slab / slab_bytes: device scratch, never empty.
 * Scope: sk_route_query(SK_OP_TRUNCATED_RBF_ADJOINT, 1, D, M, N, num_levels, ...) == SK_ROUTE_FUSED; else SK_ERR_UNSUPPORTED. */
int sk_truncated_points_adjoint_plan(int64_t A, int64_t B, int M, int N, int D, int num_levels, int paired, size_t workspace_bytes,
                                     int64_t *plan);
int sk_truncated_points_adjoint(const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int M, int N, int Ncp, int D, int fd,
                                int num_levels, double param, const double *w, double *Tpart, int64_t n_chunks, double *slab,
                                size_t slab_bytes, void *stream, int paired);
/* Symmetric Gram matrix of ONE path batch with the fused kernels above: only the A (A + 1) / 2 pairs on and above the diagonal are
 * solved (what the reference's CPU solver does for sym=True, cython_backend.pyx:74-97; its GPU path ignores `sym`), in ONE launch,
 * and each value is written to out[a][b] and out[b][a]: out [A][A] is exactly symmetric.  dXr / dXt (Xr / Xt): the row-major and
 * the dimension-major staging of the SAME paths, as sk_solve_fwd_linear_* (sk_solve_fwd_rbf_*) take them; Mc = Nc = M - 1.
 * pair_tab: the triangle's pairs as [A (A + 1) / 2][2] int32 (a, b), written by sk_prep_cat_* (tri_n = -1) RIGHT BEHIND dXt / Xt
 * (pair_tab == (int *)(Xt + A 8 Ncp)): the kernel looks pairs up there instead of inverting the triangular numbering itself. */
int sk_solve_fwd_linear_sym_f64(const double *dXr, const double *dXt, const int *pair_tab, int64_t A, int Mrows, int Mc, int Nc, int Ncp, int D, int dyadic,
                                int scheme, double *out, void *queue, void *stream);
int sk_solve_fwd_linear_sym_f32(const double *dXr, const double *dXt, const int *pair_tab, int64_t A, int Mrows, int Mc, int Nc, int Ncp, int D, int dyadic,
                                int scheme, float *out, void *queue, void *stream);
int sk_solve_fwd_rbf_sym_f64(const double *Xr, const double *Xt, const int *pair_tab, int64_t A, int Mrows, int Mc, int Nc, int Ncp, int D, int dyadic,
                             int scheme, double inv_sigma, double *out, void *queue, void *stream);
int sk_solve_fwd_rbf_sym_f32(const double *Xr, const double *Xt, const int *pair_tab, int64_t A, int Mrows, int Mc, int Nc, int Ncp, int D, int dyadic,
                             int scheme, double inv_sigma, float *out, void *queue, void *stream);

/* Forward solve with the static kernel fused in for LONG or WIDE paths (csrc/sk_wave_fused_mb.hip): any number of bands per
 * pair (M - 1 beyond 256/128/64 at dyadic 0/1/2) and path dimensions up to 16 -- BASELINE configs[4] (len 512, dim 16,
 * RBF, dyadic 2) runs in this one kernel with nothing of size P*M*N in HBM.  Replaces, like the two families above,
 * static_kernels.py:26-33 / :58-73 + sigkernel.py:362-382 (Gram) / :216-234 (paired).
 *   kind 0 (linear, param unused): Xr [A][Mrows][fd] = s^2 (x[p+1]-x[p]), Yt [Bn][fd][Ncp] = y[q+1]-y[q];
 *   kind 1 (rbf, param = sigma):   Xr = the points x[p], Yt = the points y[q];  both fp64, zero-padded, as sk_prep_paths_* builds
 *   them;  fd = 8 for D <= 8, 16 for D <= 16;  Mrows >= sk_solve_fwd_static_rows(kind, Mc, dyadic);
 *   Ncp >= sk_solve_fwd_static_cols(kind, Nc) = 2 NUp, NUp = max(80, ceil8((Nc + 1 + kind) / 2)) (second paths shorter than ~160 points
 *   are swept with padding units behind them: wasted steps, same result -- swap the arguments when the first path is the longer
 *   one, the kernel is symmetric);  B > 0: Gram, B == 0: paired;  out_final [P];  either scheme;
 *   workspace: sk_solve_fwd_static_workspace_bytes(...) bytes (one band-boundary row per resident wave; 0 = unsupported).
 * SK_ERR_UNSUPPORTED: dyadic > 2, D > 16. */
size_t sk_solve_fwd_static_workspace_bytes(int kind, int64_t P, int Mc, int Nc, int dyadic, int D);
/* FEW pairs of LONG paths (fewer pairs than half the resident waves, second paths of ~500 points and more, no edges kept): the
 * BANDS of a pair run on different waves -- band b + 1 trails band b through the pair's boundary row in HBM and a progress
 * counter, work handed out band-major by one ticket counter (an item only waits for a smaller ticket: no deadlock whatever is
 * resident) -- instead of one wave sweeping the bands of its pair one after the other; the same arithmetic in the same order, bit
 * for bit.  The workspace above includes its rows.  Returns the bands per pair when a launch of P pairs takes that mode, else 0
 * (cython_backend.pyx:64-119 has no length limit; its one thread per pair is what this replaces).  SK_FUSEDMB_SPLIT=0 disables.
 * Status: a wave's wait for the band above is bounded (~2^22 polls: a stall -- queue preemption, a fault in another wave -- must
 * not hang the device); an item that gives up poisons ITS pair with NaN (the wave's other items are untouched) and counts in the
 * launch's status word, the LAST 8 bytes (uint64) of the workspace as passed: 0 after every normal launch. */
int sk_solve_fwd_static_split(int kind, int64_t P, int Mc, int Nc, int dyadic, int D);
int sk_solve_fwd_static_rows(int kind, int Mc, int dyadic);
/* Ncp = 2 NUp: columns per dimension row of Yt (zero-padded), the same for sk_rbf_adjoint_fused_mb_f64 / sk_linear_adjoint_fused_mb_f64. */
int sk_solve_fwd_static_cols(int kind, int Nc);
/* edges (nullable; dyadic 0..2, either kind): also keep, of the grid PADDED to the bands and units of sk_rbf_adjoint_fused_mb_f64 / sk_linear_adjoint_fused_mb_f64 (padding
 * carries no increments), the bottom row of every band of 64 lanes (the last one is the pair's terminal row) and the terminal column
 * -- *edge_doubles (sk_rbf_adjoint_fused_mb_layout) doubles per pair: what that adjoint recomputes K from, band by band.  Mrows must
 * then be the layout's *mrows. */
int sk_solve_fwd_static_f64(int kind, double param, const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int Mc, int Nc,
                            int Ncp, int D, int fd, int dyadic, int scheme, double *out_final, double *edges, void *workspace,
                            size_t workspace_bytes, void *stream);
/* f32: yt_f32 = 1 (kind 1, fd = 16 only): Yt holds the fp32 points packed as sk_prep_paths_f32 layout 2 writes them -- half
 * the LDS ring, twice the resident waves at 16 dimensions; arithmetic stays fp64 (dyadic >= 1).  yt_f32 = 0: Yt is the fp64 array above --
 * except for kind 1, fd = 16, dyadic >= 1, which this entry point serves in the packed form only (SK_ERR_UNSUPPORTED otherwise). */
int sk_solve_fwd_static_f32(int kind, double param, const double *Xr, const void *Yt, int yt_f32, int64_t A, int64_t B, int Mrows,
                            int Mc, int Nc, int Ncp, int D, int fd, int dyadic, int scheme, float *out_final, double *edges,
                            void *workspace, size_t workspace_bytes, void *stream);

/* The same, also keeping the terminal row/column of every pair (layout and size: sk_strip_edges_bytes) for a later
 * sk_solve_adj_* with SK_FLAG_EDGES_GIVEN on the increments of the same paths (sk_static_increments_*, kind 1). */
int sk_solve_fwd_rbf_edges_f64(const double *Xr, const double *Yt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D,
                               int dyadic, int scheme, double inv_sigma, double *out_final, double *edges, void *queue, void *stream);

/* The same, also keeping the terminal row/column of every pair for a later sk_solve_adj_* with SK_FLAG_EDGES_GIVEN
 * (`edges`: sk_strip_edges_bytes(P, Mc, Nc, dyadic, 8) bytes; fp64, dyadic 0..2). */
int sk_solve_fwd_linear_edges_f64(const double *dXr, const double *dYt, int64_t A, int64_t B, int Mrows, int Mc, int Nc, int Ncp, int D,
                                  int dyadic, int scheme, double *out_final, double *edges, void *queue, void *stream);

/* ---- adjoint solve ------------------------------------------------------------------------
 * W[p][a][b] = d K_p[MM][NN] / d inc_c[p][a][b] by the reference's variation-of-parameters
 * formula:  W = 4^-d * sum over the fine cells (i,j) of coarse cell (a,b) of
 * K[i][j] * Krev[MM-1-i][NN-1-j], Krev = solution on the doubly flipped increments.
 * Replaces the second solver launch and the KK product at sigkernel.py:282-311 (_SigKernel.backward)
 * and :438-470 (prep_backward).
 * Two implementations behind one entry point:
 *   fast   -- forward sweep emitting the terminal row/column of K, then ONE fused sweep that runs the reverse
 *             PDE and recomputes K backwards from those edges (no grid is stored; csrc/sk_wave_adj.hip).
 *             Needs dyadic 0..2 (fp32: 0..1), increment rows zero-padded to whole 128-byte lines
 *             (ld*sizeof(T) % 128 == 0, as sk_increments_* produces when given such an ld), ldw >= that padded
 *             width, and out_err != NULL; any grid size (no 1024-node limit).  out_err[p] receives the self-check residual
 *             max_i |K_recomputed[i][0] - 1| of pair p: the caller re-solves pairs whose residual is too
 *             large with SK_FLAG_SIMPLE (only ever seen when K explodes, |K| >~ 1e4).
 *   simple -- both grids stored in `workspace`, products summed in the reference's order: bit-identical to the
 *             reference formula evaluated by the CPU oracle (SK_FLAG_EXACT / SK_FLAG_SIMPLE, or any shape
 *             the fast path does not cover).  out_err is zero-filled.
 *   SK_FLAG_DISCRETE -- not the reference's formula (which discretises the continuous adjoint PDE and differs from the derivative of
 *             the computed number by O(h): tens of per cent of the path gradient at dyadic 0..2) but the exact adjoint of the solver's
 *             own recurrence K[i+1][j+1] = (K[i+1][j] + K[i][j+1]) P(g_ij) - K[i][j] Q(g_ij):  with u[i][j] = dK[MM][NN] / dK[i+1][j+1],
 *               u[MM-1][NN-1] = 1,  u[i][j] = P(g[i][j+1]) u[i][j+1] + P(g[i+1][j]) u[i+1][j] - Q(g[i+1][j+1]) u[i+1][j+1],
 *               W[a][b] = 4^-d * sum over the fine cells of (a,b) of u[i][j] ((K[i+1][j] + K[i][j+1]) P'(g_ij) - K[i][j] Q'(g_ij)).
 *             Always the stored-grid kernel (K and the cells' terms in `workspace`, the same size as for SK_FLAG_SIMPLE; summed in a
 *             fixed order: bit-reproducible, no atomics); out_err is zero-filled; SK_FLAG_EDGES_GIVEN is ignored (`workspace` is
 *             scratch, kept edges are of no use to it); with SK_FLAG_FAST_ONLY: SK_ERR_BAD_ARG.  Both schemes, fp64 and fp32
 *             increments (fp64 state either way).
 *   SK_FLAG_DISCRETE | SK_FLAG_RAGGED -- pairs of unequal length in one padded batch.  `workspace` begins with a table the caller has
 *             written (on `stream`, or before): P entries {int32 mc, int32 nc}, the coarse cells of pair p's own paths on either side
 *             (length - 1), then padding up to the next multiple of 256 bytes, then the k >= 1 scratch slots of
 *             sk_adj_rescue_slot_bytes(Mc, Nc, dyadic) bytes; sk_adj_workspace_bytes with both flags is the head plus min(P, 1024) slots.
 *             Each entry is clamped to [0, Mc] x [0, Nc].  out_final[p] = K at node (mc << dyadic, nc << dyadic) of the padded pair
 *             -- the kernel of the truncated paths -- and W[p] its exact derivative: the sweep above over the cells a < mc, b < nc
 *             alone (bit for bit what the contiguous sub-block inc_c[p][:mc][:nc] gives on its own), and 0 on every other cell of the
 *             Mc x Nc block; mc == 0 or nc == 0: out_final[p] = 1, W[p] = 0, nothing swept.  Columns b >= Nc of W (ldw padding) are
 *             not written.  SK_FLAG_RAGGED without SK_FLAG_DISCRETE, or with SK_FLAG_FAST_ONLY: SK_ERR_BAD_ARG; a workspace that
 *             holds the head but not one slot: SK_ERR_WORKSPACE.
 *   SK_FLAG_DISCRETE | SK_FLAG_SOURCES -- the adjoint of a weighted sum of prefix kernels, L_p = sum_{a,b} S_p[a][b] K_p[(a+1) << d][(b+1) << d]
 *             (the coarse nodes of pair p's grid: the kernels of its truncated paths; row 0 and column 0 of that grid are the constant 1
 *             and carry no gradient), in ONE reverse sweep per pair.  W is IN/OUT: on entry W[p][a][b] = S_p[a][b], on exit
 *             W[p][a][b] = dL_p / d inc_c[p][a][b].  The recurrence above with a source per node in place of the 1 at the far corner:
 *               u[i][j] = src(i, j) + P(g[i][j+1]) u[i][j+1] + P(g[i+1][j]) u[i+1][j] - Q(g[i+1][j+1]) u[i+1][j+1],
 *               src(i, j) = S[((i+1) >> d) - 1][((j+1) >> d) - 1] where (i+1) and (j+1) are both multiples of 2^d, else 0.
 *             Every source of a pair is read before the first store to its W block; columns b >= Nc of W (ldw padding) are neither
 *             read nor written.  A one-hot S at (Mc-1, Nc-1) gives the plain SK_FLAG_DISCRETE result bit for bit; a one-hot S at
 *             (mc-1, nc-1) what SK_FLAG_RAGGED gives for the entry (mc, nc), zeros included.  out_final[p] = K_p[MM][NN] as without the
 *             flag, out_err is zero-filled, the workspace is that of SK_FLAG_DISCRETE.  No atomics: bit-reproducible.
 *             SK_FLAG_SOURCES without SK_FLAG_DISCRETE, with SK_FLAG_RAGGED or with SK_FLAG_FAST_ONLY: SK_ERR_BAD_ARG.
 *   workspace: sk_adj_workspace_bytes(...) bytes of device scratch.
 *   inc_c [P,Mc,ld]; out_final nullable [P]; W [P,Mc,ldw] (ldw = 0: dense); out_err nullable [P] doubles. */
size_t sk_adj_workspace_bytes(int64_t P, int Mc, int Nc, int dyadic, int flags, int elem_size);
/*   flags = SK_FLAG_FAST_ONLY: what the fast implementation alone needs (P (edges + 1) doubles; 0 when it does not cover
 *   the shape) -- the stored-grid figure grows with min(P, 1024) whole grids and is only needed for SK_FLAG_SIMPLE /
 *   SK_FLAG_EXACT calls or shapes the fast kernels do not cover; SK_FLAG_DISCRETE: the stored-grid figure (any k >= 1 slots of
 *   sk_adj_rescue_slot_bytes(Mc, Nc, dyadic) bytes serve: the blocks stride over the pairs); SK_FLAG_DISCRETE | SK_FLAG_RAGGED: the
 *   table's head (8 P bytes rounded up to a multiple of 256) plus that figure; SK_FLAG_RAGGED without SK_FLAG_DISCRETE: 0;
 *   SK_FLAG_SOURCES changes nothing (SK_FLAG_DISCRETE | SK_FLAG_SOURCES: the figure of SK_FLAG_DISCRETE). */

/* Device-side rescue of the fast adjoint: re-solves with stored grids exactly the pairs whose self-check residual
 * err[p] (as written by sk_solve_adj_*) exceeds `tol`, overwriting their W (and out_final when non-NULL); a NaN residual is
 * left alone when the pair's increments are themselves not finite (NaN / inf coordinates: the re-solve could only reproduce the
 * NaN) and re-solved when they are finite (the backward recompute overflowed).
 * Enqueue it unconditionally right after sk_solve_adj_*: when no pair is flagged it reads P doubles and returns, so the
 * caller never has to read the residuals back (the reference has no such step: it stores both grids for every pair,
 * sigkernel.py:438-470).  workspace: k >= 1 slots of sk_adj_rescue_slot_bytes(Mc, Nc, dyadic) bytes; k slots re-solve k
 * flagged pairs concurrently.  sk_adj_rescue_slot_bytes is 0, and sk_adj_rescue_* returns SK_ERR_UNSUPPORTED, for grids
 * whose three live diagonals exceed the LDS (more than ~6800 fine rows): no rescue exists there. */
size_t sk_adj_rescue_slot_bytes(int Mc, int Nc, int dyadic);
int sk_adj_rescue_f64(const double *inc_c, int64_t ld, int64_t P, int Mc, int Nc, int dyadic, int scheme, const double *err,
                      double tol, double *out_final, double *W, int64_t ldw, void *workspace, size_t workspace_bytes, void *stream);
int sk_adj_rescue_f32(const float *inc_c, int64_t ld, int64_t P, int Mc, int Nc, int dyadic, int scheme, const double *err,
                      double tol, float *out_final, float *W, int64_t ldw, void *workspace, size_t workspace_bytes, void *stream);

/* Forward solve that also keeps what the fast adjoint needs -- the terminal row and column of K in the strip kernels'
 * padded layout -- so that a later sk_solve_adj_* with SK_FLAG_EDGES_GIVEN (workspace = `edges`) skips its forward sweep.
 * The reference keeps the whole solution grid between forward and backward (sigkernel.py:248, :397-399); this is
 * (MM+NN)/(MM*NN) of that.  sk_strip_edges_bytes: size of `edges` for P pairs, 0 when the strip kernels do not cover the
 * shape (then sk_solve_fwd_edges_* returns SK_ERR_UNSUPPORTED: use sk_solve_fwd_* and a plain sk_solve_adj_*).
 * Requires the layout of the fast adjoint (rows zero-padded to whole 128-byte lines). */
size_t sk_strip_edges_bytes(int64_t P, int Mc, int Nc, int dyadic, int elem_size);
int sk_solve_fwd_edges_f64(const double *inc_c, int64_t ld, int64_t P, int Mc, int Nc, int dyadic, int scheme, double *out_final,
                           double *edges, void *stream);
int sk_solve_fwd_edges_f32(const float *inc_c, int64_t ld, int64_t P, int Mc, int Nc, int dyadic, int scheme, float *out_final,
                           double *edges, void *stream);
int sk_solve_adj_f64(const double *inc_c, int64_t ld, int64_t P, int Mc, int Nc, int dyadic, int scheme, int flags,
                     double *out_final, double *W, int64_t ldw, double *out_err, void *workspace,
                     size_t workspace_bytes, void *stream);
int sk_solve_adj_f32(const float *inc_c, int64_t ld, int64_t P, int Mc, int Nc, int dyadic, int scheme, int flags,
                     float *out_final, float *W, int64_t ldw, double *out_err, void *workspace,
                     size_t workspace_bytes, void *stream);

/* ---- directional derivatives --------------------------------------------------------
 * Replaces: sigkernel_derivatives_Gram_cuda[(A,B),T](M_inc, M_inc_diff, M_inc_diffdiff, MM+1, NN+1, n_anti_diagonals,
 *           M_sol, M_sol_diff, M_sol_diffdiff)  (cuda_backend.py:166-223, launched at sigkernel.py:546-566) and the
 *           three tile() refinements before it (sigkernel.py:543-545).
 * inc, inc_d, inc_dd: [P, Mc, ld] COARSE increments of the static kernel, of its first and of its second
 * finite-difference derivative along gamma (what sigkernel.py:526-541 builds before refinement); all three share
 * `ld` (0 = Nc).  out_k / out_kd / out_kdd: [P] = K[MM][NN], K_gamma[MM][NN], K_gamma_gamma[MM][NN] (each
 * nullable, at least one non-null).  The scheme is the reference's (no _naive_solver variant exists for this
 * path).  flags: SK_FLAG_EXACT / SK_FLAG_SIMPLE = anti-diagonal kernel in the reference's operand order
 * (bit-identical to the CPU oracle); SK_FLAG_FAST_ONLY = fail with SK_ERR_UNSUPPORTED instead of falling back. */
/* Replaces: the finite-difference pre-processing of k_kgrad (sigkernel.py:526-541).  G0, G1, G2: [P, M, N] static Gram
 * matrices of (X, Y), (X + eps*gamma, Y), (X + 2*eps*gamma, Y); inc, inc_d, inc_dd: [P, M-1, ld] (ld 0 = N-1, padding
 * columns are zeroed) -- the inputs of sk_solve_deriv_*.  Operand order as in the reference (the sums cancel 1/eps^2). */
int sk_deriv_increments_f64(const double *G0, const double *G1, const double *G2, double eps, int64_t P, int M, int N,
                            double *inc, double *inc_d, double *inc_dd, int64_t ld, void *stream);
int sk_deriv_increments_f32(const float *G0, const float *G1, const float *G2, double eps, int64_t P, int M, int N,
                            float *inc, float *inc_d, float *inc_dd, int64_t ld, void *stream);
/* The same with the static kernel fused in (kind 0 = linear, 1 = rbf with param = sigma, like sk_static_increments_*):
 * replaces the three Gram_matrix calls of k_kgrad (sigkernel.py:526, :530, :537) as well.  X0 = X, X1 = X + eps*gamma,
 * X2 = X + 2*eps*gamma: [A, M, D] each (formed by the caller); Y [B, N, D]; outputs [A*B, M-1, ld].  D <= 32. */
int sk_static_deriv_increments_f64(int kind, double param, const double *X0, const double *X1, const double *X2,
                                   const double *Y, int64_t A, int64_t B, int M, int N, int D, double eps, double *inc,
                                   double *inc_d, double *inc_dd, int64_t ld, void *stream);
int sk_static_deriv_increments_f32(int kind, double param, const float *X0, const float *X1, const float *X2, const float *Y,
                                   int64_t A, int64_t B, int M, int N, int D, double eps, float *inc, float *inc_d,
                                   float *inc_dd, int64_t ld, void *stream);
int sk_solve_deriv_f64(const double *inc, const double *inc_d, const double *inc_dd, int64_t ld, int64_t P, int Mc, int Nc,
                       int dyadic, int flags, double *out_k, double *out_kd, double *out_kdd, void *stream);
int sk_solve_deriv_f32(const float *inc, const float *inc_d, const float *inc_dd, int64_t ld, int64_t P, int Mc, int Nc,
                       int dyadic, int flags, float *out_k, float *out_kd, float *out_kdd, void *stream);

/* ---- one-launch glue of the loss wrappers (csrc/sk_loss.hip) -----------------------------------------------------
 * compute_mmd / compute_scoring_rule / compute_expected_scoring_rule (sigkernel.py:146-197) assemble their value from two or
 * three compute_Gram calls and some twenty elementwise / reduction kernels; on MI355X every dispatch costs 4-5 us, a third of a
 * training-sized step.  These entry points make each stage ONE launch; all are deterministic (no atomics, fixed reduction order).
 *
 * sk_prep_cat_*: Z = [X; Y] (X [A,M,D], Y [B,M,D], same length) staged in BOTH layouts from the two batches -- no concatenated
 *   copy: out_rows [A+B][rows][fd] (scaled by scale_rows), optionally out_rows2 (the same scaled by scale_rows2: the linear
 *   adjoint's rows carry s^2, the forward's kappa s^2), out_cols [A+B][fd][cols] (unscaled); diff as sk_prep_paths_*.  pair_tab
 *   (nullable): the pairs of a triangular layout as [P][2] int32 (a, b), written by the same launch -- tri_n >= 0: the loss layout
 *   below; tri_n = -1: the inclusive upper triangle of all A + B paths (sk_solve_fwd_*_sym_*); sk_solve_fwd_loss_f64 wants it
 *   RIGHT BEHIND out_cols (pair_tab == (int *)(out_cols + (A+B) fd cols), fd = 8): its kernel finds the table from the columns' address.
 * sk_solve_fwd_loss_f64: ONE fused forward launch over the LOSS LAYOUT of pairs: the rectangle K(Z[0..A), Z) -- A (A+B) pairs,
 *   pair (a, b) at a (A+B) + b, whose column blocks are K(X, X) and K(X, Y) -- followed by the STRICT upper triangle (i < j,
 *   row-major) of K(Y, Y), tri_n (tri_n - 1) / 2 pairs (tri_n = B, or 0: no K_YY term; the diagonals never enter the unbiased
 *   statistics, sigkernel.py:194-197).  out [P] in pair order; edges (nullable) receives the terminal edges of the RECTANGLE pairs
 *   only, in the layout sk_solve_fwd_{linear,rbf}_edges_f64 writes (sk_strip_edges_bytes for A (A+B) pairs) -- the triangle
 *   carries no gradient (the second argument of compute_mmd must not require one, sigkernel.py:188).  Replaces the three
 *   _SigKernelGram.forward calls of sigkernel.py:190-192.  kind 0: Zr = kappa s^2 differences (sk_linear_prescale), Zt differences;
 *   kind 1: points, param = 1 / sigma.  SK_ERR_UNSUPPORTED outside the one-band kernels' scope.
 * sk_loss_value_f64: value[0] = sum_{a != b} K_XX[a,b] / (A (A-1)) - 2 mean(K_XY) [+ sum_{i != j} K_YY[i,j] / (B (B-1)) when
 *   with_yy] from that output (sigkernel.py:194-197, :160-161, :177-178); wb (nullable, [A (A+B)]): d value / dK of the rectangle
 *   with the K_XX block doubled (the reference's backward doubles a Gram whose both arguments require a gradient,
 *   sigkernel.py:410-412), written by the same launch -- the constant upstream weights of the adjoint.
 * sk_loss_weights_f64: go [A (A+B)] = grad_out[0] * those weights; grad_out: a DEVICE scalar (nullable = 1).  (The wrappers
 *   pass the scalar to sk_*_adjoint_finish_f64 instead -- the adjoint is linear in it -- and keep this for callers that need go.)
 * sk_rbf_adjoint_finish_f64 / sk_linear_adjoint_finish_f64: the partial sums of sk_rbf_adjoint_fused_f64 (gpart
 *   [A][chunks][rows][outw]) / sk_linear_adjoint_fused_f64 (tpart [A][chunks][rows][8]) -> dL/dX [A,M,D], chunks added in ascending
 *   order; X: the fp64 points (rbf); scale2 = s^4 / s^2-staging factor of the linear rows (the wrapper's `param ** 2`);
 *   gscale: a DEVICE scalar (nullable = 1) multiplied into the result. */
int sk_prep_cat_f64(const double *X, int64_t A, const double *Y, int64_t B, int M, int D, int diff, double scale_rows, double scale_rows2,
                    double *out_rows, double *out_rows2, int rows, double *out_cols, int cols, int fd, int *pair_tab, int64_t tri_n, void *stream);
int sk_prep_cat_f32(const float *X, int64_t A, const float *Y, int64_t B, int M, int D, int diff, double scale_rows, double scale_rows2,
                    double *out_rows, double *out_rows2, int rows, double *out_cols, int cols, int fd, int *pair_tab, int64_t tri_n, void *stream);
int sk_solve_fwd_loss_f64(int kind, double param, const double *Zr, const double *Zt, const int *pair_tab, int64_t A, int64_t B, int64_t tri_n,
                          int Mrows, int Mc, int Nc, int Ncp, int D, int dyadic, int scheme, double *out, double *edges, void *queue, void *stream);
int sk_loss_value_f64(const double *out, int64_t A, int64_t B, int with_yy, double *value, double *wb, void *stream);
int sk_loss_weights_f64(int64_t A, int64_t B, const double *grad_out, double *go, void *stream);
int sk_rbf_adjoint_finish_f64(const double *gpart, int64_t A, int64_t chunks, int rows, int outw, const double *X, int M, int D, double sigma,
                              const double *gscale, double *grad, void *stream);
int sk_linear_adjoint_finish_f64(const double *tpart, int64_t A, int64_t chunks, int rows, int M, int D, double scale2, const double *gscale,
                                 double *grad, void *stream);

/* ---- launch planning, host only (no device work; exposed so that the partition of the pairs can be tested without a GPU) ----
 * The persistent kernels share P pairs among `waves` waves of G lane groups each; when a launch fills the chip with whole
 * workgroups (waves == resident = n_cu * waves per CU) the shares depend on the wave's age rank.
 * sk_plan_wave_shares: for every wave w, first[w] = the first pair of its lane group 0, ppg[w] = pairs per lane group (group g
 * sweeps first + g * ppg ...), end[w] = the end of its rank's range (pairs >= end belong to other waves).  Returns the number
 * of ranks (1 = equal shares) or a negative sk_status.
 * sk_plan_group_chunks: the fused adjoints' split of an A x B Gram into chunks of one row a (PPG = the equal chunk size,
 * max_groups = resident lane groups): for every lane group gi < n_groups its first pair, its slot in the partial-sum array
 * (a * chunks_per_a + c) and its number of pairs.  Returns the number of ranks. */
int sk_plan_wave_shares(int64_t P, int G, int64_t waves, int64_t resident, int wpb, int n_cu, int64_t *first, int64_t *end, int *ppg);
int sk_plan_group_chunks(int64_t A, int64_t B, int64_t PPG, int64_t max_groups, int G, int wpb, int n_cu, int64_t n_groups,
                         int64_t *first, int64_t *slot, int *ppg);
/* sk_plan_adjoint_chunks: how the one-band fused adjoints launch an A x B Gram (B > 0) or a paired batch of A pairs (B == 0) on waves of
 * G lane groups, NUp units per row, of which n_cu * wpc are resident; wpb_knob: the waves-per-workgroup knob (0: the default), lds_bytes:
 * LDS of one wave, paired_form: the variant can sweep several consecutive pairs per lane group, force_nch > 0: the chunks per row are
 * given.  plan[5] = pairs per lane-group chunk (the longest), pairs per lane group of a paired batch, rows per launch (0: one launch;
 * else the Gram is swept in launches of that many rows, each filling the chip exactly), lane groups, chunks per row.
 * sk_plan_one_draw: the launch of the one-draw kernels (multi-band forward and adjoints, fused derivative solver) for P pairs: resident
 * waves per CU from a wave's LDS bytes, the waves per workgroup wpb0, the variant's VGPR count and the waves-per-CU knob (0: none), then
 * the shares for units = bands x units per row, pct per cent of the equal share dealt out up front, ws_stride workspace doubles per wave.
 * plan[7] = waves per CU, waves, pairs per wave (the equal share), pairs a wave takes up front, the first pair drawn from the counter,
 * whether the counter is used, workspace doubles in front of the counter.
 * Both return an sk_status (SK_ERR_UNSUPPORTED: a 32-bit index guard refuses the launch). */
int sk_plan_adjoint_chunks(int64_t A, int64_t B, int G, int NUp, int n_cu, int wpc, int wpb_knob, int64_t lds_bytes, int paired_form,
                           int64_t force_nch, int64_t *plan);
int sk_plan_one_draw(int64_t P, int64_t lds_bytes, int wpb0, int vgprs, int wpc_knob, int n_cu, int64_t units, int pct, int64_t ws_stride,
                     int64_t *plan);

#ifdef __cplusplus
}
#endif
#endif /* SIGKERNEL_AMD_H */
