// sk_wave_prefix.hip -- the one-band fused forward sweep of sk_wave_fused.hip that STORES EVERY COARSE NODE: out[p][m][n] =
// k_sig(x[:m+1], y[:n+1]) for all prefixes of a pair in one sweep (SigKernel.compute_Gram_prefixes / compute_kernel_prefixes).
//
// The sweep is k_fwd_fused's without edges: the same staged arrays (sk_prep_pair_*), the same rings (y slabs and x windows by
// LDS-DMA), the same increment formation and the same cell update in the same order, so node (M - 1, N - 1) of a pair is
// bit for bit what sk_solve_fwd_{linear,rbf}_* return.  The STEP LOOP is a copy and not more template parameters of that kernel because
// k_fwd_fused sits at its vector and scalar register limits; this one carries a per-lane output pointer and a column cursor more.
// What surrounds the loop is shared with it (sk_pair_stream.h): the LDS read helpers, the pair -> (a, b) split, and on the host the
// launch plan, the VGPR query and the geometry.  The chunked pair stream is a second copy as well (see there for why).
// Always 8 staged dims, never the full-wave DPP form (lane 0 selects its 1.0 instead), no triangular pair tables; the stencil, the
// output dtype and -- at dyadic 1 and 2 -- the static kernel are launch-time values: FOUR instances (the build's budget, tests/test_abi.py).
//
// THE STORE.  In a macro-step a lane finishes RC x 2 coarse nodes: rows lam RC + k (k < RC), columns 2 uk + q (q < 2) of its pair,
// i.e. out[p][1 + lam RC + k][1 + 2 uk + q], and stores them straight from the registers.  Three schemes, chosen per launch
// (SK_PREFIX_STORE = 1 / 2 / 3; kernel times from a kernel trace, profiles/r08_prefixes.txt, headline shape):
//   1  DIRECT: 2 RC one-element stores where the block is finished                                          36.0 ms
//   2  DEFERRED: the same stores issued at the end of the loop body, behind the window's vmcnt(0) wait       35.8 ms
//      (stores count in vmcnt like the DMA: the wait then never drains a store issued in the same step -- no gain: the drain is hidden
//      by the other waves of the SIMD)
//   3  TWO-COLUMN PIECES (the default where the grid allows it): grid column 1 sits at an odd element, so the piece is shifted by one
//      column -- (previous unit's second node, this unit's first) = grid columns 2 uk, 2 uk + 1, column 0 being the ones -- RC aligned
//      16-byte stores per macro-step (8-byte for float).  Needs an even N, an even distance between the grids and an aligned `out`;
//      anything else runs scheme 2.                                                                          28.2 ms
// Even scheme 3 reaches 1.2 TB/s, 0.15 of the HBM peak: every store instruction still touches one piece of up to 64 different rows, and
// a 128-byte line is completed by one lane over eight steps.  Staging the pieces in LDS so that eight lanes write a whole line per
// instruction is NOT built ("prefix grids").  Padding is never stored: rows >= Mc (the last lanes), columns >= Nc (the odd
// column of a half-filled unit, the padded units, the node column the RBF stream borrows) and stream positions without a pair are
// masked per lane.  Column 0 of rows >= 1 is written here (inside lines the kernel writes anyway); row 0 -- N contiguous ones per
// pair -- is the host's fill.
//
// SLICES (prm.slice, a launch-time wave-uniform value like the stencil and the output dtype: no instance more).  Most callers want a
// thin slice of the grid, and the full grid is what binds the kernel to its stores (and to the card's memory), so three more store
// modes keep only the nodes of a slice, out + p ldo + index with ldo = the slice's length:
//   1  DIAGONAL     out[p][t] = k(x[:t+1], y[:t+1]), t < min(M, N): the nodes whose row lam RC + k + 1 equals their column 2 uk + q + 1
//   2  LAST ROW     out[p][n] = k(x, y[:n+1]),       n < N:         row Mc, i.e. one row of one lane of the pair
//   3  LAST COLUMN  out[p][m] = k(x[:m+1], y),       m < M:         column Nc, i.e. one macro-step of every lane
// One-element stores straight from the registers, direct (where the block is finished), under the same masks as the full grid's
// (padding rows, padding columns, stream positions without a pair); element 0 -- exactly 1 in all three -- is the host's fill.  The
// sweep is the same code: every stored value is bit for bit the node the full grid holds there.  The slice modes branch around the
// full grid's store block (one scalar branch per macro-step), so that block and its registers are as they were.
//   4  NODES AT     out[p] = k(x[:len_x[a]], y[:len_y[b]]): ONE node per pair, (len_x[a] - 1, len_y[b] - 1) of its grid -- batches of
//      paths of unequal length, padded at the end to a common (M, N).  The wave sweeps the padded pair as ever; where the sweep enters a
//      pair the lane loads the two lengths (two global loads in a block that runs once per pair and lane).  n_cols -- per launch Nc in
//      every other mode -- becomes the pair's own len_y[b] - 1; the lane that holds row len_x[a] - 1 gets o_ptr = out + p with that row's
//      k < RC in the pointer's two low bits (elements are 4 or 8 bytes and `out` is aligned to them), every other lane nullptr.  The
//      store is the intersection of the last row's and the last column's conditions: that lane, row k, the node column with
//      col + q + 1 == n_cols.  o_rows stays the launch's (a per-pair o_rows costs registers across the loop: profiles/r12_ragged.txt).
//      A pair with a one-point path stores nothing (its value, exactly 1, is the host's fill of the whole of `out`); a length outside
//      [1, padded length] stores nothing or another node of the pair, never elsewhere: the only address formed is out + p.  No
//      per-lane state is added to the step loop.
//
// RESUME (prm.col_in / prm.col_out, launch-time wave-uniform values; the last row's store mode only: no instance more).  All that crosses
// a column of a pair is the lane's left[R] and its corner, so a stream y that GROWS is swept in pieces: a launch over y[s:] that loads
// the fine column K[.][s << dyadic] where the sweep enters a pair continues the sweep of y[:s + 1] cell for cell -- the same operands in the
// same order, so every node it stores is bit for bit the node a sweep of the whole of y stores there.
//   col_in   pair p's column at col_in + p ld_col: element i = K at fine row i + 1 of the pair (row 0 is the ones).  Lane lam loads
//            elements [lam R, lam R + R) into left[] -- the fine rows >= Mc << dyadic of the pair's last lane are not loaded: they keep
//            the 1.0 of a first launch -- and its corner from element lam R - 1 (lane 0: the top boundary, 1.0).  In the block that
//            runs once per pair and lane; nullptr: the ones.
//   col_out  the same layout: a lane that finishes unit state_unit - 1 of its pair stores left[] there -- the column behind that unit,
//            fine column 2 state_unit << dyadic of the launch, an even coarse column: a column inside a unit never exists as a whole in
//            registers, and the padded second column of a half-filled unit must not enter the state (its zero increment still changes
//            K).  Only the fine rows < Mc << dyadic are stored, two at a time (R is even, ld_col is even, the arrays 16-byte aligned).
//   ld_col >= ceil(Mc / RC) R (prefix_state_pitch: whole lanes) and even.  Elements [Mc << dyadic, ld_col) of a slot are neither read
//   nor written; lanes without rows of the pair, stream positions without a pair and the pairs of a padded lane group touch
//   nothing.  col_in and col_out must not overlap: a lane reads its corner from the slot of the lane above, which may have left the
//   state unit already.
// REGISTERS: k_fwd_prefix<1, 2, 0> sits AT 168 VGPRs, the three-wave line.  Deriving the pair again where the state is stored (from the
// stream cursor, or from o_ptr by a division) costs one register in that instance; so the block that opens a pair -- which has the
// pair -- forms the lane's store address there and parks it in prev[0], a register the slice modes carry through the loop unused.
// With that all four instances keep their counts (157 / 157 / 168 / 141, no scratch).
//
// Scope: kind 0 / 1, dim <= 8, one band per pair -- rows <= 64 RC with RC = 4 / 2 / 1 at dyadic 0 / 1 / 2, rows = M - 1 linear and
// M rbf; rbf at dyadic 0 sweeps two rows per lane (rows <= 128: the four-row form with 8 staged dims spills) -- dyadic <= 2, any N.
// PAIR ORDER, rings, producers: see sk_wave_fused.hip, whose comments are not repeated here.
#include "sk_pair_stream.h"
#include <algorithm>

namespace sk {
namespace {


constexpr int FD = 8, ND = 8;      // dims carried (inputs are zero-padded to 8)
constexpr int Y_SLAB_PITCH = y_slab_pitch(ND);   // 8 dimension rows of 8 units; odd slabs swap each pair of rows (sk_wave_fused.hip)
constexpr int XROW = x_row_bytes(ND);

struct PrefixParams {
    const double *dXr;   // [A][Mrows][8]: linear: kappa s^2 (x[p+1]-x[p]); rbf: x[p]  (sk_prep_pair_*, as sk_solve_fwd_{linear,rbf}_*)
    const double *dYt;   // [Bn][8][Ncp]: linear: y[q+1]-y[q]; rbf: y[q]; dimension-major
    void *out;           // pair p: (Mc + 1) x (Nc + 1) nodes at out + p ldo, row pitch Nc + 1; row 0 is not written here
                         // (slice != 0: the slice's min(Mc, Nc) + 1 / Nc + 1 / Mc + 1 elements at out + p ldo; element 0 is not written here)
    int64_t ldo;         // elements between the grids of consecutive pairs
    int64_t P, B;        // B > 0: Gram, pair p = (p / B, p % B); B == 0: paired, pair p = (p, p)
    int Mrows, Ncp;
    int Mc, Nc, NUp, logL;
    int kind, naive, f32;   // static kernel (0 linear, 1 rbf), first-order stencil, nodes stored as float
    int defer, wide;        // the store scheme (see THE STORE above): stores issued behind the window's DMA wait; shifted two-column pieces
    int slice;              // SK_NODES_*: 0 the full grid; 1 / 2 / 3: only the diagonal / the last row / the last column; 4: one node per
                            // pair, (len_x[a] - 1, len_y[b] - 1) (see SLICES above)
    // slice 4: points per path, [A] and [B] (paired launch: [A], indexed by the pair), nullptr otherwise.  Slice 2 reads the same two
    // kernel arguments as the RESUME mode's arrays (see RESUME above; kernel arguments live in scalar registers the loop has none to
    // spare of): the kept column the sweep of a pair starts from / the column it leaves behind, pair p's fine rows at col + p ld_col;
    // nullptr: start from the ones / keep nothing.  state_unit: col_out is the column behind unit state_unit - 1
    union { const int *len_x; const double *col_in; };
    union { const int *len_y; double *col_out; };
    int ld_col;
    int resume;          // RESUME: state_unit << 2 | (col_out != nullptr) << 1 | (col_in != nullptr); 0 in every other launch
    int u_f, lam_f;      // unit / lane of the last node (they end the wave's last pair)
    double inv_sigma;    // RBF: G = exp(-|x - y|^2 * inv_sigma)
    WaveGroup wg;
    // the stream of pairs (sk_wave_fused.hip; the plan: plan_pair_stream): chunk 0 of every wave is fixed (C0 pairs per lane group), the
    // rest drawn 2^logC at a time from `queue`; queue == nullptr: the first n_big waves take C0 + 1 pairs per lane group
    unsigned long long *queue;
    int64_t q_first;
    int C0, logC, n_big;
    int shy_A;           // > 0: SHARED-Y pair order (a Gram launch with G >= 2 lane groups): position q of lane group g is pair
                         // a = G (q / B) + g, b = q % B; P then counts positions, ceil(A / G) B
};

// RCX: coarse rows per lane when not the strip kernels' own (Tile<DY>::RC) -- 2 for the RBF kernel at dyadic 0, whose four-row form
// with 8 staged dims spills
// KIND 0 / 1: the static kernel is a compile-time constant (dyadic 0, where the two sweep different rows per lane); KIND 2: it is
// prm.kind -- one instance serves both (wave-uniform branches around the increment formation).  The stencil (prm.naive) and the output
// dtype (prm.f32) are launch-time values everywhere: the build's instance budget has room for four instances of this kernel, not 24.
template <int DY, int KIND, int RCX = 0>
__global__ __launch_bounds__(4 * WAVE) void k_fwd_prefix(const PrefixParams prm) {
    const bool RBF = KIND == 2 ? prm.kind == 1 : KIND == 1;
    const bool NAIVE = prm.naive != 0;
    const int LAG = RBF ? 2 : 0;   // macro-steps by which the block sweep trails the node evaluation (sk_wave_fused.hip)
    constexpr int CW = 2;
    constexpr int RC = RCX ? RCX : Tile<DY>::RC, R = RC << DY, S = CW << DY, r = 1 << DY;
    constexpr int XW = x_window(KIND, ND, RC, false);   // lanes (= macro-steps) per x window: four only for the linear four-row form (dyadic 0)
    constexpr int XSLAB = RC * XW * XROW;    // XW lanes x RC rows
    extern __shared__ __attribute__((aligned(16))) char lds_block[];
    char *lds;
    const int64_t wave_id = wave_slot(prm.wg, lds_block, lds);   // independent waves, see sk_wave_common.h
    if (wave_id < 0) return;
    const unsigned lds0 = lds_offset(lds);

    const int lane = threadIdx.x & (WAVE - 1);
    const int L = 1 << prm.logL, G = WAVE >> prm.logL;
    const int lam = lane & (L - 1), grp = lane >> prm.logL;
    const int NUp = prm.NUp;
    const int NSLAB = (L >> 3) + 2;                       // y slabs resident per lane group
    const unsigned y_bytes = (unsigned)(NSLAB * Y_SLAB_PITCH);
    const bool shy = prm.shy_A > 0;
    const int GY = shy ? 1 : G;                           // y rings of the wave = lane groups that own a stream of their own
    // inside the step loop's rare blocks the mode is re-derived from the ONE kernel argument behind an opaque move (sk_wave_fused.hip)
    auto shy_a = [&]() __attribute__((always_inline)) -> int {
        int v = prm.shy_A;
        asm volatile("" : "+s"(v));
        return v;
    };
    // RESUME: the mode's one word behind an opaque move, so that nothing derived from it is held in a scalar register of its own across the
    // loop (the two arrays share the kernel arguments of slice 4's lengths)
    auto resume_word = [&]() __attribute__((always_inline)) -> int {
        int v = prm.resume;
        asm volatile("" : "+s"(v));
        return v;
    };
    const unsigned x_base0 = (unsigned)GY * y_bytes;      // x rings behind all y rings
    const double sc = 1.0 / (double)(1 << (2 * DY));
    const double c_half = 0.5 * sc, c_12 = sc * sc / 12.0;

    // ---- consumer state: the step counter modulo NUp in scalar registers (tm, tq); a lane compares it with constants of its own --
    // u == 0 when tm == c_u0, uk == 0 when tm == c_uk0 -- and the y ring is walked by one running address
    int yslab, ypar;   // slab of the y ring holding virtual unit v = t - lam, and that slab's storage parity
    {
        const int s0 = floor_div(-lam, 8);
        yslab = ((s0 % NSLAB) + NSLAB) % NSLAB;
        ypar = (s0 + (shy ? 0 : grp)) & 1;
    }
    const int lam7 = lam & 7;
    int tm = 0, tq = 0;
    int c_u0 = lam % NUp, c_uk0 = (lam + LAG) % NUp;
    // t - lam - LAG = (tq + c_kq) NUp + tm + c_kr with c_kr = (NUp - c_uk0) % NUp: the remainder is not held, tm + c_kr wrapped into
    // [0, NUp) is tm - c_uk0 wrapped (a VGPR less across the loop: <1, 2, 0> sits AT the three-wave line, profiles/r12_ragged.txt)
    int c_kq = floor_div(-lam - LAG, NUp);
    int c_u0m1 = (c_u0 + NUp - 1) % NUp;                                        // tm of the step BEFORE the lane starts a pair
    asm volatile("" : "+v"(c_u0), "+v"(c_uk0), "+v"(c_kq), "+v"(c_u0m1));
    unsigned a_e;   // the odd rows are at a_e ^ 128: wave slices and slabs are 256-byte aligned, a slab row is 128 bytes
    // ---- the wave's stream of pairs: k_fwd_fused's chunked stream (the comments are there) with even shares or the queue, never
    // rank shares.  A COPY: as shared by-reference functions (sk_pair_stream.h) all four instances changed -- 3213 / 2804 / 2987 /
    // 2697 instructions became 3193 / 2759 / 2959 / 2669 and <1, 2, 0> went from 167 to 165 VGPRs (157 / 155 / 147 stayed); as a
    // struct with the state by value 157 -> 159, 155 -> 157, 147 -> 148 VGPRs.
    const unsigned P32 = (unsigned)prm.P;
    const int w32 = __builtin_amdgcn_readfirstlane((int)wave_id);
    const int c0_ = prm.C0 + (w32 < prm.n_big ? 1 : 0);
    const unsigned cb0_ = (unsigned)(GY * (w32 * prm.C0 + (w32 < prm.n_big ? w32 : prm.n_big)));
    const int C0 = __builtin_amdgcn_readfirstlane(c0_), logC = prm.logC, CQ = 1 << logC;
    unsigned cb0 = (unsigned)__builtin_amdgcn_readfirstlane((int)cb0_), cb1 = NOPAIR, cb2 = NOPAIR, cb3 = NOPAIR;   // chunk k in cb[k & 3]
    int have = 1;                     // chunks known so far
    int t_end = 0x7fffffff;           // macro-steps this wave runs: known once a draw comes back empty
    auto ring_at = [&](int kk) __attribute__((always_inline)) -> unsigned {
        return (cb0 & -(unsigned)(kk == 0)) | (cb1 & -(unsigned)(kk == 1)) | (cb2 & -(unsigned)(kk == 2)) | (cb3 & -(unsigned)(kk == 3));
    };
    auto chunk_of = [&](int i, int &off) __attribute__((always_inline)) -> int {
        if (i < C0) { off = i; return 0; }
        off = (i - C0) & (CQ - 1);
        return 1 + ((i - C0) >> logC);
    };
    // pair at stream position i of lane group g (NOPAIR: none); shared-y: the POSITION, the same for every lane group
    auto stream_pair = [&](int g, int i) __attribute__((always_inline)) -> unsigned {
        if (i < 0) return NOPAIR;
        int off;
        const int k = chunk_of(i, off);
        const int size = k == 0 ? C0 : CQ;
        const unsigned b = ring_at(k & 3);
        const unsigned p = b + (unsigned)((shy_a() > 0 ? 0 : g * size) + off);
        return (b >= P32 || p >= P32) ? NOPAIR : p;
    };
    // make sure the chunk of stream position f is known (the producers call this with the furthest position they touch)
    auto ensure = [&](int f) __attribute__((always_inline)) {
        int off;
        const int kf = chunk_of(f, off);
        while (have <= kf) {
            unsigned b = NOPAIR;
            if (prm.queue && t_end == 0x7fffffff) {
                unsigned long long v = 0;
                if (lane == 0) v = atomicAdd(prm.queue, (unsigned long long)((shy_a() > 0 ? 1 : G) * CQ));
                const unsigned long long q = (unsigned long long)prm.q_first +
                                             (((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
                                              (unsigned)__builtin_amdgcn_readfirstlane((int)v));
                b = q < (unsigned long long)P32 ? (unsigned)q : NOPAIR;
            }
            if (b == NOPAIR && t_end == 0x7fffffff)
                // the stream ends where chunk `have` would begin: a wave is done with the step in which the lane of the last row
                // finishes the last pair's last unit (u_f, not the padded NUp - 1); the lanes above it are there earlier
                t_end = (C0 + (have - 1) * CQ - 1) * NUp + prm.u_f + prm.lam_f + LAG + 1;
            const int kk = have & 3;
            const unsigned m0 = -(unsigned)(kk == 0), m1 = -(unsigned)(kk == 1), m2 = -(unsigned)(kk == 2), m3 = -(unsigned)(kk == 3);
            cb0 = (unsigned)__builtin_amdgcn_readfirstlane((int)((cb0 & ~m0) | (b & m0)));
            cb1 = (unsigned)__builtin_amdgcn_readfirstlane((int)((cb1 & ~m1) | (b & m1)));
            cb2 = (unsigned)__builtin_amdgcn_readfirstlane((int)((cb2 & ~m2) | (b & m2)));
            cb3 = (unsigned)__builtin_amdgcn_readfirstlane((int)((cb3 & ~m3) | (b & m3)));
            have += 1;
        }
    };
    const bool is_top = lam == 0;
    const unsigned my_y = lds0 + (shy ? 0u : (unsigned)grp * y_bytes);
    const unsigned y_lim = my_y + y_bytes;
    {
        const unsigned ya = my_y + (unsigned)(yslab * Y_SLAB_PITCH + ((-lam & 7) << 4));
        a_e = ya + (unsigned)(ypar << 7);
    }
    // lanes NUp apart start (different) pairs at the same macro-step: one x slab per such "lap" j = lam / NUp
    const int JMAX = (L + NUp - 1) / NUp;
    const unsigned my_x = lds0 + x_base0 + (unsigned)((grp * X_SLOTS * JMAX) * XSLAB + (lam / NUp) * XSLAB) +
                          (unsigned)((lam & (XW - 1)) * RC * XROW);

    // ---- producers (uniform control; per-lane source offsets): y slab s = virtual units [8s, 8s+8) of every lane group, dims
    // k = lane/8, unit x = lane%8; x windows for the lanes that start a pair during macro-steps [t0, t0+XW)
    int y_pi = 0, y_u0 = 0, y_slot = 0, y_par = 0;   // next y slab: pair-in-group, first unit, ring slot, parity of the virtual slab number
    auto issue_y = [&]() __attribute__((always_inline)) {
        ensure(y_pi);
        const int gy = shy_a() > 0 ? 1 : G;
        for (int g = 0; g < gy; ++g) {
            const unsigned sp = stream_pair(g, y_pi);
            const int64_t p = sp == NOPAIR ? 0 : (int64_t)sp;   // past the end: fetch something valid, never consumed
            const int64_t b = pair_split<false, FD>(prm, p, true);
            const int krow = (lane >> 3) ^ ((y_par + g) & 1);   // odd slabs (per group): dimension rows swapped in pairs
            const double *src = prm.dYt + ((b * FD + krow) * (int64_t)prm.Ncp + (int64_t)(y_u0 + (lane & 7)) * 2);
            __builtin_amdgcn_global_load_lds(src, (lds_void *)(lds + g * y_bytes + y_slot * Y_SLAB_PITCH), 16, 0, 0);
        }
        y_slot = y_slot + 1 == NSLAB ? 0 : y_slot + 1;
        y_par ^= 1;
        y_u0 += 8;
        if (y_u0 == NUp) { y_u0 = 0; y_pi += 1; }
    };
    int x_q0 = 0, x_lam0 = 0, x_slot = 0;   // next window: t0 / NUp, t0 % NUp, ring slot
    auto issue_x = [&]() __attribute__((always_inline)) {
        ensure(x_q0);
        for (int j = 0; j < JMAX; ++j) {
            const int lamj = x_lam0 + j * NUp, pi = x_q0 - j;
            if (lamj >= L) break;
            // shared-y: position pi is row a = G (pi's position / B) + g for lane group g (no such row: fetch something valid, never stored)
            const int sA = shy_a();
            const int64_t gm = sA > 0 ? G : 1, gs = sA > 0 ? 1 : 0, a_lim = sA > 0 ? sA : 0x7fffffff;
            for (int g = 0; g < G; ++g) {
                const unsigned sp = stream_pair(g, pi);
                const int64_t p = sp == NOPAIR ? 0 : (int64_t)sp;
                int64_t a = pair_split<false, FD>(prm, p, false);
                a = a * gm + gs * g;
                if (a >= a_lim) a = 0;
                const char *src = reinterpret_cast<const char *>(prm.dXr + (a * prm.Mrows + (int64_t)lamj * RC) * FD);
                char *dst = lds + x_base0 + ((g * X_SLOTS + x_slot) * JMAX + j) * XSLAB;
#pragma unroll
                for (int c = 0; c < (XSLAB + 1023) / 1024; ++c)
                    if (c * 1024 + lane * 16 < XSLAB)      // LDS-DMA lands lane l's 16 bytes at dst + 16 l
                        __builtin_amdgcn_global_load_lds(src + c * 1024 + lane * 16, (lds_void *)(dst + c * 1024), 16, 0, 0);
            }
        }
        x_slot = x_slot + 1 == X_SLOTS ? 0 : x_slot + 1;
        x_lam0 += XW;
        if (x_lam0 == NUp) { x_lam0 = 0; x_q0 += 1; }
    };

    // this lane's x rows as 16-byte register pairs: the reload's ds_read_b128 lands in them directly
    d2_t dxq[RC][ND / 2];
#pragma unroll
    for (int k = 0; k < RC; ++k)
#pragma unroll
        for (int j = 0; j < ND / 2; ++j) dxq[k][j] = d2_t{0.0, 0.0};
    auto load_x_rows = [&](unsigned xa) {
        if constexpr (RC % 2 == 0) {   // two rows per instruction group
#pragma unroll
            for (int k = 0; k < RC; k += 2) lds_load_line(dxq[k], dxq[k + 1], xa + k * 64u);
        } else {
#pragma unroll
            for (int k = 0; k < RC; ++k) lds_load_row(dxq[k], xa + k * (unsigned)XROW);
        }
    };
    // RBF: node values of this lane's rows at the columns of units uk, uk + 1, uk + 2 (the last two filled this step), and
    // of the first row of the lane below at the columns of units uk and uk + 1
    constexpr int OWN = KIND == 0 ? 1 : RC;
    double own[OWN][6], bel[4];
    ExpCoef expc;
    if (RBF) expc.init();
#pragma unroll
    for (int k = 0; k < OWN; ++k)
#pragma unroll
        for (int c = 0; c < 6; ++c) own[k][c] = 1.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) bel[c] = 1.0;
    double left[R], bot[S], corner = 1.0;
#pragma unroll
    for (int i = 0; i < R; ++i) left[i] = 1.0;
#pragma unroll
    for (int i = 0; i < S; ++i) bot[i] = 1.0;

    // ---- the store: node (1, 1) of this lane's rows in the grid of the pair its SWEEP is in (nullptr: no such pair, or only padding
    // rows), set where the sweep enters a pair; o_rows of the lane's RC rows exist
    const int64_t pitch = (int64_t)prm.Nc + 1;
    // (NOT clamped to RC: every use compares it with a k < RC, and the last-row store finds the lane of row Mc by 1 <= o_rows <= RC)
    int o_rows = prm.Mc - lam * RC;
    char *o_ptr = nullptr;      // (bytes: the element is a double or, prm.f32, a float)
    const int esz = prm.f32 ? 4 : 8;
    int n_cols = prm.Nc;
    asm volatile("" : "+v"(o_rows), "+v"(n_cols));
    // wide: node column 2 uk - 1 of the lane's rows, finished one macro-step ago (column 0 -- the ones -- when the sweep enters a pair)
    double prev[RC];
#pragma unroll
    for (int k = 0; k < RC; ++k) prev[k] = 1.0;
    const bool wide = prm.wide != 0, defer = prm.defer != 0;
    // a slice of the grid (prm.slice != 0): o_ptr is element 1 + lam RC of the pair's slice (diagonal, last column: element k from there
    // belongs to the lane's row k) or element 1 (last row: element 2 uk + q from there belongs to node column q of the step).
    // REGISTERS: k_fwd_prefix<1, 2, 0> has one VGPR to spare below three waves per SIMD, and whatever is invariant per lane gets hoisted
    // into a register of its own -- so nothing here forms one (no lam RC, no Nc - 1, no running pointer); the ISA is as the full grid's
    // alone (tools/variants.py: 157 / 155 / 167 / 147 VGPRs, no scratch).
    auto store_slice = [&](const double (&cand)[RC][CW], int uk) __attribute__((always_inline)) {
        if (o_ptr == nullptr) return;
        const int slice = prm.slice;
        const int col = 2 * uk;
        if (slice == 2) {
            // last row: only the lane that holds row Mc has a row k with k + 1 == o_rows
            if (o_rows <= RC) {
                asm volatile("");
                double v0 = cand[0][0], v1 = cand[0][1];
#pragma unroll
                for (int k = 1; k < RC; ++k) {
                    v0 = k + 1 == o_rows ? cand[k][0] : v0;
                    v1 = k + 1 == o_rows ? cand[k][1] : v1;
                }
                if (prm.f32) {
                    float *const o = reinterpret_cast<float *>(o_ptr) + col;
                    if (col < n_cols) o[0] = (float)v0;
                    if (col + 1 < n_cols) o[1] = (float)v1;
                } else {
                    double *const o = reinterpret_cast<double *>(o_ptr) + col;
                    if (col < n_cols) o[0] = v0;
                    if (col + 1 < n_cols) o[1] = v1;
                }
            }
        } else if (slice == 1) {
            // diagonal: node (k, q) lies on it where col + q == lam RC + k.  The lane's first row is re-derived from the lane number in
            // every step (behind an opaque zero, or it would be hoisted): no register is held for it across the sweep
            int z = 0;
            asm volatile("" : "+s"(z));
            const int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, (unsigned)z));
            const int d = col - (ln & ((1 << prm.logL) - 1)) * RC;
#pragma unroll
            for (int k = 0; k < RC; ++k)
#pragma unroll
                for (int q = 0; q < CW; ++q)
                    if (d == k - q && k < o_rows && col + q < n_cols) {
                        if (prm.f32) reinterpret_cast<float *>(o_ptr)[k] = (float)cand[k][q];
                        else reinterpret_cast<double *>(o_ptr)[k] = cand[k][q];
                    }
        } else if (slice == 4) {
            // the pair's end node: only the lane that holds its row has a pointer, the row k in its low bits; both columns are selected
            // before the column test (the select chain inside the test leaves <0, 0, 0> a private segment)
            asm volatile("");
            const int at = (int)(reinterpret_cast<uintptr_t>(o_ptr) & 3);
            char *const o = reinterpret_cast<char *>(reinterpret_cast<uintptr_t>(o_ptr) & ~(uintptr_t)3);
            double v0 = cand[0][0], v1 = cand[0][1];
#pragma unroll
            for (int k = 1; k < RC; ++k) {
                v0 = k == at ? cand[k][0] : v0;
                v1 = k == at ? cand[k][1] : v1;
            }
            const int dc = n_cols - col;
            if (dc == 1 || dc == 2) {
                const double v = dc == 2 ? v1 : v0;
                if (prm.f32) *reinterpret_cast<float *>(o) = (float)v;
                else *reinterpret_cast<double *>(o) = v;
            }
        } else {
            // last column: grid column Nc = node column Nc - 1 of the sweep
#pragma unroll
            for (int q = 0; q < CW; ++q)
                if (col + (q + 1) == n_cols) {
#pragma unroll
                    for (int k = 0; k < RC; ++k)
                        if (k < o_rows) {
                            if (prm.f32) reinterpret_cast<float *>(o_ptr)[k] = (float)cand[k][q];
                            else reinterpret_cast<double *>(o_ptr)[k] = cand[k][q];
                        }
                }
        }
    };
    // the nodes of one macro-step (uk: the sweep's unit, before the step counter moves on)
    auto store_nodes = [&](const double (&cand)[RC][CW], int uk) __attribute__((always_inline)) {
        if (o_ptr != nullptr) {
            const int col = 2 * uk;
            if (wide) {
                // grid columns 2 uk and 2 uk + 1 = the previous unit's second node and this unit's first: one aligned piece per row
                // (N is even here, so a unit with a first node inside the pair has both columns of its piece inside the row)
                if (col < n_cols) {
                    if (prm.f32) {
                        float *const o = reinterpret_cast<float *>(o_ptr) + (col - 1);
#pragma unroll
                        for (int k = 0; k < RC; ++k)
                            if (k < o_rows) *reinterpret_cast<float2 *>(o + k * pitch) = float2{(float)prev[k], (float)cand[k][0]};
                    } else {
                        double *const o = reinterpret_cast<double *>(o_ptr) + (col - 1);
#pragma unroll
                        for (int k = 0; k < RC; ++k)
                            if (k < o_rows) *reinterpret_cast<d2_t *>(o + k * pitch) = d2_t{prev[k], cand[k][0]};
                    }
                }
            } else if (prm.f32) {
                float *const o = reinterpret_cast<float *>(o_ptr) + col;
#pragma unroll
                for (int k = 0; k < RC; ++k)
                    if (k < o_rows) {
                        if (col == 0) o[k * pitch - 1] = 1.0f;      // column 0 of the grid: the one-point prefix of y
                        if (col < n_cols) o[k * pitch] = (float)cand[k][0];
                        if (col + 1 < n_cols) o[k * pitch + 1] = (float)cand[k][1];
                    }
            } else {
                double *const o = reinterpret_cast<double *>(o_ptr) + col;
#pragma unroll
                for (int k = 0; k < RC; ++k)
                    if (k < o_rows) {
                        if (col == 0) o[k * pitch - 1] = 1.0;
                        if (col < n_cols) o[k * pitch] = cand[k][0];
                        if (col + 1 < n_cols) o[k * pitch + 1] = cand[k][1];
                    }
            }
        }
        if (wide) {
#pragma unroll
            for (int k = 0; k < RC; ++k) prev[k] = cand[k][1];
        }
    };

    // RESUME: left[] -- the fine column behind the unit this lane has just finished -- to the lane's part of the pair's slot of col_out,
    // whose address the block that opened the pair left in prev[0].  Called by a lane with rows of a pair (o_ptr)
    auto store_state = [&]() __attribute__((always_inline)) {
        double *const co = reinterpret_cast<double *>(static_cast<uintptr_t>(__double_as_longlong(prev[0])));
        const int n_fine = o_rows << DY;
#pragma unroll
        for (int i = 0; i < R; i += 2) {
            if (i + 1 < n_fine) *reinterpret_cast<d2_t *>(co + i) = d2_t{left[i], left[i + 1]};
            else if (i < n_fine) co[i] = left[i];
        }
    };

    d2_t dyn[ND];
    auto read_y = [&]() { lds_read_dims_issue(dyn, a_e, a_e ^ 128u); };
    unsigned x_rd_off = 0;   // ring slot the x rows of this XW-step window are read from: ((t / XW) % X_SLOTS) * JMAX * XSLAB
    static_assert(X_SLOTS == 2, "x_rd_off toggles between two slots");
    issue_y();
    issue_x();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    issue_y();
    issue_x();
    if (c_u0 == 0) {   // lanes that start a pair in macro-step 0 (their K state is 1.0 already)
        load_x_rows(my_x);
#pragma unroll
        for (int k = 0; k < RC; ++k) lds_rows_wait(dxq[k]);
    }
    read_y();
    for (int t = 0; t < t_end; ++t) {
        // -- top row of the block from the lane above
        double top[S];
#pragma unroll
        for (int i = 0; i < S; ++i) {
            const double sh = dpp_shr1(bot[i], 1.0);
            top[i] = is_top ? 1.0 : sh;
        }

        // -- the sweep enters a pair: left boundary K[i][0] = 1, and where this lane's nodes of the pair go
        if (tm == c_uk0) {
            asm volatile("");   // a real branch
            corner = 1.0;
#pragma unroll
            for (int i = 0; i < R; ++i) left[i] = 1.0;
#pragma unroll
            for (int k = 0; k < RC; ++k) prev[k] = 1.0;
            const int pv = tq + c_kq + (tm != 0 ? 1 : 0);   // (tm == c_uk0 here: tm + c_kr is 0 or NUp)
            unsigned pair_u = stream_pair(grp, pv);
            const int sA = shy_a();
            if (sA > 0 && pair_u != NOPAIR) {   // position -> this lane group's pair: a = G (q / B) + grp, b = q % B, out index a B + b
                const unsigned Bu = (unsigned)prm.B, qa = pair_u / Bu, a = qa * (unsigned)G + (unsigned)grp;
                pair_u = a < (unsigned)sA ? a * Bu + (pair_u - qa * Bu) : NOPAIR;
            }
            // (a slice: see store_slice -- the same address arithmetic with a pitch of 1 or 0 in place of the grid's, all scalar)
            const int sl = prm.slice;
            // (slice 4: the pair's one element, ldo = 1)
            const int64_t o_pitch = sl == 0 ? pitch : (sl == 2 || sl == 4) ? 0 : 1, o_first = sl == 0 || sl == 2 ? 1 : 0;
            o_ptr = (pair_u != NOPAIR && o_rows > 0)
                        ? static_cast<char *>(prm.out) + ((int64_t)pair_u * prm.ldo + (int64_t)(1 + lam * RC) * o_pitch + o_first) * esz
                        : nullptr;
            if (sl == 4) {
                // the pair's own end node in place of the launch's: out index a B + b (Gram, either pair order) or the pair (paired).
                // The lane's first row is re-derived from the lane number behind an opaque zero, as the diagonal's store does: lam RC
                // held for this block alone is a register across the loop
                asm volatile("");
                int lx = 0, ly = 0;
                if (pair_u != NOPAIR) {
                    unsigned a = pair_u, b = pair_u;
                    if (prm.B > 0) { a = pair_u / (unsigned)prm.B; b = pair_u - a * (unsigned)prm.B; }
                    lx = prm.len_x[a];
                    ly = prm.len_y[b];
                }
                int z = 0;
                asm volatile("" : "+s"(z));
                const int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, (unsigned)z));
                const int at_k = (lx - 2) - (ln & ((1 << prm.logL) - 1)) * RC;
                n_cols = ly - 1;
                o_ptr = (pair_u != NOPAIR && at_k >= 0 && at_k < RC) ? static_cast<char *>(prm.out) + ((int64_t)pair_u * esz + at_k) : nullptr;
            }
            if (resume_word() != 0) {
                // RESUME: the pair's kept column in place of the ones, and where this lane's part of the next one goes (o_ptr: the
                // pair exists and this lane holds rows of it).  The lane number behind an opaque zero, as above; the rows are loaded
                // under their own masks, straight into left[]
                asm volatile("");
                if (o_ptr != nullptr) {
                    int z = 0;
                    asm volatile("" : "+s"(z));
                    const int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, (unsigned)z)) & ((1 << prm.logL) - 1);
                    const int64_t slot = (int64_t)pair_u * prm.ld_col + (int64_t)(ln * R);
                    const int rw = resume_word();
                    if (rw & 1) {
                        const double *const ci = prm.col_in + slot;
                        const int n_fine = o_rows << DY;
#pragma unroll
                        for (int i = 0; i < R; ++i)
                            if (i < n_fine) left[i] = ci[i];
                        if (ln != 0) corner = ci[-1];
                        // the loads are waited for HERE: left open, the compiler's wait for them lands in front of the block sweep
                        // of every macro-step, where it also drains the DMA and the deferred stores of the step before
#pragma unroll
                        for (int i = 0; i < R; ++i) asm volatile("" : "+v"(left[i]));
                        asm volatile("" : "+v"(corner));
                    }
                    // the slice modes never read prev[] (the full grid's two-column pieces): its first register carries the address
                    // through the pair's sweep, so that the store needs no pair and nothing new is held across the loop
                    if (rw & 2) prev[0] = __longlong_as_double((long long)reinterpret_cast<uintptr_t>(prm.col_out + slot));
                }
            }
        }

        // -- y differences of the two coarse columns of this macro-step, all 8 dims
        d2_t dyv[ND];
        lds_dims_wait(dyv, dyn);

        // -- increments and coefficients per coarse cell
        double ca[RC][CW], cbm[RC][CW];
        double ginc[RC][CW];
        if constexpr (KIND != 0) { if (RBF) {
            // nodes G[p][q] = exp(-|x_p - y_q|^2 / sigma) of this lane's RC top node rows at the two columns of unit u
#pragma unroll
            for (int k = 0; k < RC; ++k)
#pragma unroll
                for (int q = 0; q < CW; ++q) {
                    double d2 = 0.0;
#pragma unroll
                    for (int j = 0; j < ND; ++j) {
                        const double df = dxq[k][j >> 1][j & 1] - dyv[j][q];
                        d2 = fma(df, df, d2);
                    }
                    // d2 * 0 is 0 for finite distances and NaN for an infinite (or NaN) one, as the reference's exponent is
                    const double ex = fma(-d2, prm.inv_sigma, d2 * 0.0);
                    own[k][4 + q] = exp_nonpos(ex, expc);
                }
            // the node row below this lane's last coarse row is the first row of the lane below, which is one macro-step
            // behind: what it has just evaluated are the columns of unit u - 1 = uk + 1
            bel[2] = dpp_shl1(own[0][4], bel[2]);
            bel[3] = dpp_shl1(own[0][5], bel[3]);
            // 4-corner differences in the reference's order: G11 + G00 - G10 - G01
#pragma unroll
            for (int k = 0; k < RC; ++k)
#pragma unroll
                for (int q = 0; q < CW; ++q) {
                    const double t0 = own[k][q], t1 = own[k][q + 1];
                    const double b0 = k + 1 < RC ? own[(k + 1) % RC][q] : bel[q];
                    const double b1 = k + 1 < RC ? own[(k + 1) % RC][q + 1] : bel[q + 1];
                    ginc[k][q] = ((b1 + t0) - b0) - t1;
                }
#pragma unroll
            for (int k = 0; k < RC; ++k)
#pragma unroll
                for (int c = 0; c < 4; ++c) { own[k][c] = own[k][c + 2]; asm volatile("" : "+v"(own[k][c])); }
            bel[0] = bel[2];
            bel[1] = bel[3];
            asm volatile("" : "+v"(bel[0]), "+v"(bel[1]));
        } }
        if (KIND != 1 && !RBF) {
#pragma unroll
            for (int k = 0; k < RC; ++k)
#pragma unroll
                for (int q = 0; q < CW; ++q) {
                    double g = 0.0;
#pragma unroll
                    for (int j = 0; j < ND; ++j) g = fma(dxq[k][j >> 1][j & 1], dyv[j][q], g);
                    ginc[k][q] = g;
                }
        }
#pragma unroll
        for (int k = 0; k < RC; ++k)
#pragma unroll
            for (int q = 0; q < CW; ++q) {
                const double g = ginc[k][q];
                // the operations of k_fwd_fused's four compile-time cases, selected at run time: the same bits
                if (!RBF) {
                    // LINEAR: the staged x differences carry kappa = 4^-d / sqrt(12) (sk_linear_prescale): 1 + g (sqrt 3 + g), 1 - g g
                    ca[k][q] = fma(g, NAIVE ? 1.7320508075688772 : g + 1.7320508075688772, 1.0);
                    cbm[k][q] = NAIVE ? 1.0 : fma(-g, g, 1.0);
                } else {
                    const double g2 = g * g, lin = fma(g, c_half, 1.0);
                    ca[k][q] = NAIVE ? lin : fma(g2, c_12, lin);
                    cbm[k][q] = NAIVE ? 1.0 : fma(g2, -c_12, 1.0);
                }
            }

        // -- sweep the R x S block
        double cand[RC][CW];
#pragma unroll
        for (int cc = 0; cc < S; ++cc) {
            double above = top[cc];
            double diag = cc == 0 ? corner : top[cc - 1];
#pragma unroll
            for (int rr = 0; rr < R; ++rr) {
                const double a = ca[rr >> DY][cc >> DY], b = cbm[rr >> DY][cc >> DY];
                const double k10 = left[rr];
                // (the first-order stencil has b = 1: diag * 1 is diag, the same bits as k_fwd_fused's fma(k10, a, -diag))
                const double v = fma(above, a, fma(k10, a, -(diag * b)));
                diag = k10;
                above = v;
                left[rr] = v;
                if ((rr & (r - 1)) == r - 1 && (cc & (r - 1)) == r - 1) cand[rr >> DY][cc >> DY] = v;
            }
            bot[cc] = above;
        }
        corner = top[S - 1];

        // -- the RC x 2 coarse nodes this block finishes: rows lam RC + k, columns 2 uk + q of the pair (uk: the sweep's unit).
        // Stores count in vmcnt like the DMA, and loads and stores do not return in order among each other, so the window's DMA
        // wait below is vmcnt(0): stored HERE, the last step of a window pays its stores' whole round trip in that wait; DEFERRED,
        // they are issued behind it (end of the loop body) and have a whole window to land.
        int uk_now = tm - c_uk0;
        uk_now += uk_now < 0 ? NUp : 0;
        if (prm.slice != 0) {      // (the launcher clears defer and wide then: nothing of the full grid's block runs)
            asm volatile("");   // a real branch around the full grid's stores
            store_slice(cand, uk_now);
            if (resume_word() & 2) {
                asm volatile("");
                if (uk_now + 1 == (resume_word() >> 2) && o_ptr != nullptr) store_state();
            }
        } else if (!defer) {
            store_nodes(cand, uk_now);
        }

        // -- advance: the y units of the NEXT macro-step and the x rows of a lane that starts a pair in it, handed over by the single
        // LDS wait at the top of the next step
        {
            const bool turn = ((t + 1) & (XW - 1)) == 0;   // the next step opens an x window: its DMA was issued XW steps ago
            if (__builtin_expect(turn, 0)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            a_e += 16;
            if (((t + 1) & 7) == lam7) {   // next slab: the other parity, one slab less one row on, wrapping at the end of the ring
                asm volatile("");
                const unsigned e = (a_e + (unsigned)(Y_SLAB_PITCH - 128)) ^ 128u;
                a_e = e - (e >= y_lim ? y_bytes : 0u);
            }
            read_y();
            if (tm == c_u0m1) load_x_rows(my_x + (turn ? x_rd_off ^ (unsigned)(JMAX * XSLAB) : x_rd_off));
        }
        tm += 1;
        if (tm == NUp) { tm = 0; tq += 1; }
        if (__builtin_expect(((t + 1) & (XW - 1)) == 0, 0)) {
            // (nothing new is in flight since the wait above: this one is free)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (XW == 8 || ((t + 1) & 7) == 0) issue_y();       // slab ((t + 1) >> 3) + 1
            issue_x();       // window t + 1 + XW .. t + 2 XW
            x_rd_off ^= (unsigned)(JMAX * XSLAB);
        }
        if (defer) store_nodes(cand, uk_now);
    }
    // the last read-ahead is never used, but its registers are not free before it has landed
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// coarse rows per lane: the strip kernels' own (4 / 2 / 1), two for rbf at dyadic 0
constexpr int prefix_rc(int kind, int dy) { return (kind == 1 && dy == 0) ? 2 : (dy == 0 ? 4 : dy == 1 ? 2 : 1); }

constexpr int PREFIX_STORE_DEFAULT = 3;

struct PrefixPlan {
    int64_t P;          // stream positions (pairs; shared-y: ceil(A / G) B)
    int G, NUp, L, lag; // G: lane groups with a stream position of their own (shared-y: 1)
    size_t lds_bytes;   // per wave
    int waves_per_cu;   // from LDS; still to be capped by the variant's VGPR use
};

// KIND 0 / 1 at dyadic 0, 2 (= either, prm.kind) at dyadic 1 and 2: four instances
template <int DY, int KIND>
int launch_prefix_v(PrefixParams prm, const PrefixPlan &pl, hipStream_t s) {
    constexpr int RCX = (KIND == 1 && DY == 0) ? 2 : 0;
    auto kern = k_fwd_prefix<DY, KIND, RCX>;
    static const int vgprs = variant_vgprs(kern, 128);
    const int pct = (int)cost_by_name(prm.kind == 1 ? "fused_static_share_rbf" : "fused_static_share_linear");
    StreamPlan sp;
    if (const int rc = plan_pair_stream(pl.P, pl.G, pl.NUp, pl.L, pl.lag, waves_by_vgprs(pl.waves_per_cu, vgprs), device_cu_count(), pct,
                                        prm.queue != nullptr, sp))
        return rc;
    const int64_t waves = sp.waves;
    prm.C0 = sp.C0; prm.n_big = sp.n_big; prm.logC = sp.logC; prm.q_first = sp.q_first;
    if (!sp.queue) prm.queue = nullptr;
    else if (hipMemsetAsync(prm.queue, 0, sizeof(unsigned long long), s) != hipSuccess) return SK_ERR_LAUNCH;
    prm.wg = wave_group(pl.lds_bytes, waves, knobs().fused_wpb);
    const size_t lds_block = wave_group_lds(prm.wg);
    if (lds_block > 64 * 1024)
        (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_block);
    SK_LAUNCH(kern, dim3(wave_group_blocks(prm.wg)), dim3(WAVE * prm.wg.wpb), lds_block, s, prm);
    return check_launch();
}

}  // namespace

// rows a pair occupies on the lanes of the prefix kernel, and whether they fit one band (the SK_OP_PREFIX rule of sk_route.hip)
bool prefix_in_scope(int kind, int D, int Mc, int dyadic) {
    if ((kind != 0 && kind != 1) || D < 1 || D > FD || dyadic < 0 || dyadic > 2 || Mc < 1) return false;
    const int rows = kind == 1 ? Mc + 1 : Mc;
    return rows <= 64 * prefix_rc(kind, dyadic);
}

// doubles of one pair's kept column (RESUME): the fine rows of the lanes that hold rows of the pair, whole lanes -- ceil(Mc / RC) R
int64_t prefix_state_pitch(int kind, int Mc, int dyadic) {
    if ((kind != 0 && kind != 1) || dyadic < 0 || dyadic > 2 || Mc < 1) return 0;
    const int RC = prefix_rc(kind, dyadic);
    return ((int64_t)Mc + RC - 1) / RC * ((int64_t)RC << dyadic);
}

// KIND 0: dXr [A][Mrows][8] / dYt [Bn][8][Ncp] are path differences; KIND 1: the same layouts hold the path points.
// nodes: 0 the full grid (ldo >= (Mc + 1) (Nc + 1)); 1 / 2 / 3 the diagonal / last row / last column alone (ldo >= its length);
// 4 (SK_NODES_AT): node (len_x[a] - 1, len_y[b] - 1) of every pair alone, out + p (ldo is not used), len_x [A] / len_y [B] (paired: [A])
// device int32.  The wave sweeps the padded pair whatever the lengths: the plan is the padded shape's.
// col_in / col_out (nodes 2 only; either may be null): RESUME, see the head of this file -- [P][ld_col] doubles each, ld_col >=
// prefix_state_pitch and even, 16-byte aligned, not overlapping; col_out is the column behind unit state_unit - 1, 2 state_unit <= Nc.
// SK_ERR_UNSUPPORTED outside the kernel's scope.
template <typename TO>
int launch_fwd_prefix(int kind, const double *dXr, const double *dYt, int64_t A, int64_t B, int Mrows, int Ncp, int D, const Geom &g,
                      double inv_sigma, TO *out, int64_t ldo, void *queue, hipStream_t s, int nodes, const int *len_x, const int *len_y,
                      const double *col_in, double *col_out, int64_t ld_col, int state_unit) {
    const int DY = g.dyadic;
    if (nodes < 0 || nodes > 4) return SK_ERR_BAD_ARG;
    if (col_in || col_out) {
        // RESUME: the last row's store mode; whole lanes per slot, 16-byte aligned slots, a state column inside the launch, two arrays
        if (nodes != 2 || DY < 0 || DY > 2 || g.Mc < 1) return nodes != 2 ? SK_ERR_BAD_ARG : SK_ERR_UNSUPPORTED;
        if (ld_col < prefix_state_pitch(kind, g.Mc, DY) || ld_col > 0x7fffffff || (ld_col & 1) || ((uintptr_t)col_in | (uintptr_t)col_out) % 16) return SK_ERR_BAD_ARG;
        if (col_out && (state_unit < 1 || 2 * (int64_t)state_unit > g.Nc)) return SK_ERR_BAD_ARG;
        const int64_t span = g.P * ld_col;
        if (col_in && col_out && col_in < col_out + span && col_out < col_in + span) return SK_ERR_BAD_ARG;
    }
    if (nodes == 4 && (!len_x || !len_y)) return SK_ERR_BAD_ARG;
    if (nodes == 4) ldo = 1;
    if (!prefix_in_scope(kind, D, g.Mc, DY)) return SK_ERR_UNSUPPORTED;
    const int RC = prefix_rc(kind, DY);
    OneBandGeom og;
    OneBandShape sh{};   // (no edges, no triangular layouts, never a lane count of the caller's)
    sh.kind = kind, sh.Mc = g.Mc, sh.Nc = g.Nc, sh.Mrows = Mrows, sh.Ncp = Ncp, sh.RC = RC, sh.nd = ND, sh.A = A, sh.B = B, sh.P = g.P;
    if (const int rc = one_band_geometry(sh, og)) return rc;
    const int NUp = og.NUp, logL = og.logL, L = og.L;
    const bool shy = og.shy;
    const size_t lds_bytes = og.lds_bytes;
    const int64_t n_pos = og.n_pos;
    int waves_per_cu = (int)((160 * 1024) / lds_bytes);
    const int cap = DY == 0 ? 8 : 12;      // as the forward without stores (sk_wave_fused.hip)
    if (waves_per_cu > cap) waves_per_cu = cap;
    if (waves_per_cu > 4) waves_per_cu &= ~3;   // whole four-wave workgroups
    if (waves_per_cu < 1) waves_per_cu = 1;
    const PrefixPlan pl{n_pos, og.GY, NUp, L, kind == 1 ? 2 : 0, lds_bytes, waves_per_cu};

    PrefixParams prm;
    prm.dXr = dXr; prm.dYt = dYt; prm.out = out; prm.ldo = ldo; prm.P = n_pos; prm.B = B;
    prm.Mrows = Mrows; prm.Ncp = Ncp; prm.Mc = g.Mc; prm.Nc = g.Nc; prm.NUp = NUp; prm.logL = logL;
    prm.inv_sigma = inv_sigma;
    prm.kind = kind; prm.naive = g.naive; prm.f32 = sizeof(TO) == 4;
    // store scheme: SK_PREFIX_STORE = 1 direct, 2 deferred, 3 deferred + two-column pieces (where the grid allows them); 0: the default
    const int mode = knobs().prefix_store > 0 ? knobs().prefix_store : PREFIX_STORE_DEFAULT;
    const bool can_wide = ((g.Nc + 1) & 1) == 0 && (ldo & 1) == 0 && ((uintptr_t)out % (2 * sizeof(TO))) == 0;
    prm.slice = nodes;
    prm.len_x = nodes == 4 ? len_x : nullptr;
    prm.len_y = nodes == 4 ? len_y : nullptr;
    if (nodes == 2) { prm.col_in = col_in; prm.col_out = col_out; }      // (they share the lengths' kernel arguments)
    prm.ld_col = (int)ld_col;
    prm.resume = nodes == 2 ? ((col_out ? state_unit : 0) << 2 | (col_out ? 2 : 0) | (col_in ? 1 : 0)) : 0;
    // (a slice is stored direct, one element at a time: the deferred scheme and the two-column pieces belong to the full grid)
    prm.defer = nodes == 0 && mode >= 2;
    prm.wide = nodes == 0 && mode >= 3 && can_wide;
    // (shared-y: the kernel rebuilds the pair index a B + b from a position in 32 bits)
    if (B > 0 && A * B >= 0x7ff00000LL) return SK_ERR_UNSUPPORTED;
    prm.queue = (unsigned long long *)queue;
    prm.u_f = (g.Nc - 1) / 2;
    prm.lam_f = ((g.Mc - 1) / RC) % L;
    prm.shy_A = shy ? (int)A : 0;
    prm.q_first = 0; prm.C0 = 0; prm.logC = 0; prm.n_big = 0;
    switch (DY) {
        case 0: return kind == 0 ? launch_prefix_v<0, 0>(prm, pl, s) : launch_prefix_v<0, 1>(prm, pl, s);
        case 1: return launch_prefix_v<1, 2>(prm, pl, s);
        default: return launch_prefix_v<2, 2>(prm, pl, s);
    }
}

template int launch_fwd_prefix<double>(int, const double *, const double *, int64_t, int64_t, int, int, int, const Geom &, double, double *,
                                       int64_t, void *, hipStream_t, int, const int *, const int *, const double *, double *, int64_t, int);
template int launch_fwd_prefix<float>(int, const double *, const double *, int64_t, int64_t, int, int, int, const Geom &, double, float *,
                                      int64_t, void *, hipStream_t, int, const int *, const int *, const double *, double *, int64_t, int);

}  // namespace sk
