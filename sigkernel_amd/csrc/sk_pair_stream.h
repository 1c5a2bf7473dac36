// sk_pair_stream.h -- what the persistent-wave fused kernels share around their step loops: the LDS read helpers of the one-band
// sweeps (sk_wave_fused.hip, sk_wave_prefix.hip), their pair -> (a, b) split, and the host arithmetic of their launchers
// (launch plan, geometry; the VGPR query of every persistent-wave launcher is in sk_wave_common.h) -- and of the ONE-DRAW launchers
// (sk_wave_fused_mb.hip, sk_wave_adj_fused_mb.hip, sk_wave_deriv_fused.hip): one_draw_waves_per_cu, plan_one_draw.  The one-band fused
// adjoints' host arithmetic (plan_adjoint_chunks, sweep_gram_rows) is next to pick_chunk / chunk_split in sk_wave_common.h, the arming
// of their device-side rescue (arm_fused_rescue) in sk_adj_fused_rescue.hip.
// The step loops themselves are NOT shared: they sit at their kernels' register limits and are tuned per kernel.
// Everything device-side here is __forceinline__ and keeps the evaluation order and the opaque moves of the per-file copies
// it replaced, so the kernels' ISA is theirs: compare the ISA of the whole build when touching it.
// The host functions make no HIP call and read no global: device properties and cost-table values come in as arguments.
#pragma once
#include "sk_wave_common.h"

namespace sk {
namespace {

// ---- LDS reads of the one-band sweeps -----------------------------------------------------------------------------------------------
// y units of a macro-step: even dimensions at a_even + {0, 256, 512, 768}, odd ones at a_odd + the same; the two addresses
// differ by +-128 (parity swizzle of the slabs).
// The reads carry no wait: they are issued at the end of a macro-step for the next one, so that their round trip
// overlaps this wave's own block sweep.  `t` is written by the LDS and read by nothing until lds_dims_wait hands it
// over (outputs tied to the temporaries' registers; tools/check_async_hazards.py lints the ISA for early uses).
__device__ __forceinline__ void lds_read_dims_issue(d2_t (&t)[8], unsigned a_even, unsigned a_odd) {
    asm volatile("ds_read_b128 %0, %8\n\t"
                 "ds_read_b128 %1, %9\n\t"
                 "ds_read_b128 %2, %8 offset:256\n\t"
                 "ds_read_b128 %3, %9 offset:256\n\t"
                 "ds_read_b128 %4, %8 offset:512\n\t"
                 "ds_read_b128 %5, %9 offset:512\n\t"
                 "ds_read_b128 %6, %8 offset:768\n\t"
                 "ds_read_b128 %7, %9 offset:768"
                 : "=&v"(t[0]), "=&v"(t[1]), "=&v"(t[2]), "=&v"(t[3]), "=&v"(t[4]), "=&v"(t[5]), "=&v"(t[6]), "=&v"(t[7])
                 : "v"(a_even), "v"(a_odd)
                 : "memory");
}
// dims 0..3 only (ND = 4)
__device__ __forceinline__ void lds_read_dims_issue(d2_t (&t)[4], unsigned a_even, unsigned a_odd) {
    asm volatile("ds_read_b128 %0, %4\n\t"
                 "ds_read_b128 %1, %5\n\t"
                 "ds_read_b128 %2, %4 offset:256\n\t"
                 "ds_read_b128 %3, %5 offset:256"
                 : "=&v"(t[0]), "=&v"(t[1]), "=&v"(t[2]), "=&v"(t[3])
                 : "v"(a_even), "v"(a_odd)
                 : "memory");
}
__device__ __forceinline__ void lds_dims_wait(d2_t (&v)[4], d2_t (&t)[4]) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "=v"(v[0]), "=v"(v[1]), "=v"(v[2]), "=v"(v[3]) : "0"(t[0]), "1"(t[1]), "2"(t[2]), "3"(t[3]) : "memory");
}
__device__ __forceinline__ void lds_dims_wait(d2_t (&v)[8], d2_t (&t)[8]) {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "=v"(v[0]), "=v"(v[1]), "=v"(v[2]), "=v"(v[3]), "=v"(v[4]), "=v"(v[5]), "=v"(v[6]), "=v"(v[7])
                 : "0"(t[0]), "1"(t[1]), "2"(t[2]), "3"(t[3]), "4"(t[4]), "5"(t[5]), "6"(t[6]), "7"(t[7])
                 : "memory");
}
// x-row reloads straight into the row registers (read-write operands: under a divergent branch the inactive lanes keep theirs).
// No wait inside: lds_rows_wait (or any later s_waitcnt lgkmcnt(0) that precedes the first use) hands the rows over.
__device__ __forceinline__ void lds_rows_wait(d2_t (&r)[4]) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]) : : "memory");
}
__device__ __forceinline__ void lds_rows_wait(d2_t (&r)[2]) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(r[0]), "+v"(r[1]) : : "memory");
}
__device__ __forceinline__ void lds_load_line(d2_t (&r0)[4], d2_t (&r1)[4], unsigned a) {     // 128 contiguous bytes: two rows of 8 dims
    asm volatile("ds_read_b128 %0, %8\n\tds_read_b128 %1, %8 offset:16\n\tds_read_b128 %2, %8 offset:32\n\tds_read_b128 %3, %8 offset:48\n\t"
                 "ds_read_b128 %4, %8 offset:64\n\tds_read_b128 %5, %8 offset:80\n\tds_read_b128 %6, %8 offset:96\n\t"
                 "ds_read_b128 %7, %8 offset:112"
                 : "+v"(r0[0]), "+v"(r0[1]), "+v"(r0[2]), "+v"(r0[3]), "+v"(r1[0]), "+v"(r1[1]), "+v"(r1[2]), "+v"(r1[3])
                 : "v"(a) : "memory");
}
__device__ __forceinline__ void lds_load_two_half_rows(d2_t (&r0)[2], d2_t (&r1)[2], unsigned a) {   // two consecutive 32-byte rows
    asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:16\n\tds_read_b128 %2, %4 offset:32\n\tds_read_b128 %3, %4 offset:48"
                 : "+v"(r0[0]), "+v"(r0[1]), "+v"(r1[0]), "+v"(r1[1]) : "v"(a) : "memory");
}
__device__ __forceinline__ void lds_load_row(d2_t (&r)[4], unsigned a) {
    asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:16\n\tds_read_b128 %2, %4 offset:32\n\tds_read_b128 %3, %4 offset:48"
                 : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]) : "v"(a) : "memory");
}
__device__ __forceinline__ void lds_load_row(d2_t (&r)[2], unsigned a) {
    asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:16" : "+v"(r[0]), "+v"(r[1]) : "v"(a) : "memory");
}

// ---- a wave's stream of pairs ---------------------------------------------------------------------------------------------------------
// Pair indices are 32-bit inside the kernels (the launchers refuse P >= 2^31 - 2^20); NOPAIR marks "no such pair".
constexpr unsigned NOPAIR = 0xffffffffu;

// pair p of a Gram launch (prm.B > 0) -> its row a = p / B or column b = p % B; a paired launch (B == 0): p itself.
// 32-bit: B <= P < 2^31 in a Gram launch, and the 64-bit division sequence is ~150 scalar instructions per use.
// TRI: where prm.tri is set, the pairs of the triangular layouts -- symmetric Gram, loss layout -- come from a table [P][2] of
// int32 (a, b) that sk_prep_cat_* writes right BEHIND the staged columns: found from dYt, B and Ncp, which the producers hold
// anyway.  (The triangle arithmetic inside the kernel -- a square root and two correction loops per look-up, inlined four
// times -- sat in the scalar registers of EVERY launch: 25 v_readlane / v_writelane in the headline variant against 17
// without it, profiles/r05_ab_r04_vs_r05.txt)
template <bool TRI, int FD, class PRM>
__device__ __forceinline__ int64_t pair_split(const PRM &prm, int64_t p, bool want_b) {
    if (prm.B <= 0) return p;
    if constexpr (TRI) {
        if (prm.tri) {
            const int *tab = reinterpret_cast<const int *>(prm.dYt + prm.B * (int64_t)FD * prm.Ncp);
            return (int64_t)tab[2 * p + (want_b ? 1 : 0)];
        }
    }
    if (want_b) return (int64_t)((uint32_t)p % (uint32_t)prm.B);
    return (int64_t)((uint32_t)p / (uint32_t)prm.B);
}

// THE STREAMS THEMSELVES ARE NOT SHARED.  Every kernel keeps its own copy of its stream (the chunked one in k_fwd_fused and
// k_fwd_prefix, the one-draw one in k_fwd_fused_mb, k_deriv_fused and the two multi-band adjoints): moved into __forceinline__
// functions that take the ring, `have` and `t_end` by reference and the kernel's parts as callables, behind the kernels'
// unchanged lambdas, all 195 instances of these kernels came out with other ISA than the measured one; each file gives the
// register numbers seen.  A fix to one copy goes into the others.  (Their HOST arithmetic has one copy: plan_pair_stream, plan_one_draw.)

// ---- host: the launch arithmetic of these kernels ---------------------------------------------------------------------------------------
// lanes per x window of the one-band sweeps: 8 (one window per y slab period), or 4 where four lanes' rows fill a whole 1 KiB LDS-DMA
// instruction anyway (the linear four-row form with 8 dims and no edges: the headline's) -- half the x ring for the same number of DMA
// instructions, the window bookkeeping every fourth step instead of every eighth
constexpr int x_window(int kind, int nd, int rc, bool edges) { return (kind == 0 && nd == 8 && rc == 4 && !edges) ? 4 : 8; }
constexpr int y_slab_pitch(int nd) { return nd * 128; }   // ND dimension rows of 8 units (the four-dimension variants stage and keep
                                                          // dims 0..3 only); no padding (parity swizzle, sk_wave_fused.hip)
constexpr int X_SLOTS = 2;   // the window being consumed + the one in flight
constexpr int x_row_bytes(int nd) { return nd == 4 ? 32 : 64; }

// How a pair sits on the lanes of a one-band sweep (k_fwd_fused, k_fwd_prefix) and what a wave needs in LDS for it.
struct OneBandGeom {
    int NUp, logL, L, G, JMAX, GY;
    bool shy;           // shared-y pair order: a plain Gram launch without edges and two or more lane groups per wave -- one y ring per wave
    size_t lds_bytes;   // per wave (a multiple of 256: the y reads rely on 256-byte aligned slices)
    int64_t n_pos;      // stream positions: pairs, or (shared-y) pairs of one lane group
};
// linear: one unit = two increment columns.  RBF: one unit = two NODE columns, and the sweep of a pair's last unit reads one node
// column of the following unit, which therefore has to exist as padding inside the pair's stream; likewise the lanes of a pair
// must cover M node rows, not M - 1 increment rows.  RC: coarse rows per lane; nd: staged dims of the variant (4 or 8);
// logL_fixed > 0: the caller's own lane count.  SK_ERR_UNSUPPORTED: more than one band per pair, or staged arrays too small.
struct OneBandShape {   // the inputs, by name: eight of them are ints
    int kind, Mc, Nc, Mrows, Ncp, RC, nd;
    bool edges;
    int64_t A, B, P;
    int tri, logL_fixed;
};
inline int one_band_geometry(const OneBandShape &in, OneBandGeom &o) {
    const int NU = in.kind == 1 ? (in.Nc + 2) / 2 : (in.Nc + 1) / 2;
    const int rows = in.kind == 1 ? in.Mc + 1 : in.Mc;
    o.NUp = (NU + LINE_UNITS - 1) / LINE_UNITS * LINE_UNITS;
    if (in.Ncp < o.NUp * 2 || (in.Ncp & 1)) return SK_ERR_UNSUPPORTED;
    o.logL = 3;
    while (o.logL < 6 && (in.RC << o.logL) < rows) ++o.logL;
    if (in.logL_fixed > 0) o.logL = in.logL_fixed;
    o.L = 1 << o.logL;
    if (o.L * in.RC < rows) return SK_ERR_UNSUPPORTED;   // more than one band per pair
    if (in.Mrows < o.L * in.RC) return SK_ERR_UNSUPPORTED;
    o.G = WAVE / o.L;
    o.JMAX = (o.L + o.NUp - 1) / o.NUp;
    o.shy = in.B > 0 && in.tri == 0 && !in.edges && o.G >= 2 && in.A > 0 && in.A <= 0x7fffffff && in.P == in.A * in.B;
    o.GY = o.shy ? 1 : o.G;
    o.lds_bytes = (size_t)o.GY * (((o.L >> 3) + 2) * y_slab_pitch(in.nd)) +
                  (size_t)o.G * (X_SLOTS * o.JMAX * in.RC * x_window(in.kind, in.nd, in.RC, in.edges) * x_row_bytes(in.nd));
    o.n_pos = o.shy ? (in.A + o.G - 1) / o.G * in.B : in.P;
    if (o.lds_bytes > 160 * 1024) return SK_ERR_UNSUPPORTED;
    return SK_OK;
}

// Division of a pair index by the Gram's column count B as a multiply and a shift (Granlund & Montgomery 1994, round-up form for
// 31-bit dividends): with l = ceil(log2 B) and m = ceil(2^(31 + l) / B), 2^(31 + l) <= m B <= 2^(31 + l) + 2^l, hence
//     floor(p / B) = floor(p m / 2^(31 + l)) = mulhi(2 p, m) >> l      for every 0 <= p < 2^31,
// and m < 2^32 because B > 2^(l - 1).  The kernels form p < P <= 0x7ff00000 only.  Returns nonzero for a B outside [1, 2^31).
inline int div_magic(uint32_t B, unsigned &m, int &shift) {
    if (B < 1 || B >= 0x80000000u) return 1;
    int l = 0;
    while ((1ull << l) < B) ++l;
    const unsigned long long num = 1ull << (31 + l);
    const unsigned long long mm = (num + B - 1) / B;
    if (mm >> 32) return 1;
    m = (unsigned)mm;
    shift = l;
    return 0;
}

// The equal share of a launch of P stream positions on waves of G lane groups: as many waves as the positions need, at most max_waves.
inline void even_share(int64_t P, int G, int64_t max_waves, int64_t &waves, int64_t &per) {
    waves = (P + G - 1) / G;
    if (waves > max_waves) waves = max_waves;
    per = (P + waves * G - 1) / (waves * G);      // pairs per lane group
}

// The launch plan of a chunked stream (k_fwd_fused, k_fwd_prefix): what the kernel's C0 / n_big / logC / q_first are, and whether the launch draws
// from the counter at all.
struct StreamPlan {
    int64_t waves, per;   // waves launched; the largest share, pairs per lane group
    int64_t q_first;
    int C0, n_big, logC;
    bool queue;           // the counter is used: the caller zeroes it before the launch (else it passes queue = nullptr)
    // ROW-LOCAL dealing (plan_row_dealing; row_wprb == 0: off, and everything above is the plan it always was)
    int row_wprb;         // waves per row-block: wave w is at home in row-block w % n_rb
    int row_rem;          // positions the LAST wave of a row-block takes on top of C0, so that what is left is whole chunks
    int row_q0;           // a row-block's counter hands out its positions from this offset on (= row_wprb C0 + row_rem)
    int64_t n_rb;         // row-blocks = counters (the caller zeroes n_rb of them)
};
// waves_per_cu: resident waves per CU, already capped by LDS and registers; pct: per cent of the equal share dealt out up front
// when the counter is used (100: never use it); has_queue: the caller has a counter.
inline int plan_pair_stream(int64_t P, int G, int NUp, int L, int lag, int waves_per_cu, int n_cu, int pct, bool has_queue, StreamPlan &o) {
    const int64_t max_waves = (int64_t)n_cu * waves_per_cu;
    even_share(P, G, max_waves, o.waves, o.per);
    if (o.per > 0x1fffffff / NUp) return SK_ERR_UNSUPPORTED;
    if (P >= 0x7ff00000LL) return SK_ERR_UNSUPPORTED;           // (pair indices are 32-bit inside the kernel)
    // drawn chunks: small, but never so small that more than three of them are in flight between the producers' frontier and
    // the last lane of the sweep (the kernel keeps a ring of four chunk bases) ...
    const int span = (L - 1 + lag + 24) / NUp + 2;
    int logC = 0;
    while ((span >> logC) + 1 > 3) ++logC;
    // ... and not smaller than needed either: ~24 draws per lane group balance a launch to a per cent or two, while every
    // chunk costs each lane one look-up of its first pair (the variants that keep edges do that in the macro-step path)
    while ((o.per * (100 - pct) / 100) >> (logC + 1) >= 24 && logC < 8) ++logC;
    o.logC = logC;      // (without the counter the chunks after the first are all empty, but the ring must not wrap onto the first)
    o.queue = has_queue && o.waves == max_waves && o.per >= (8 << logC) && pct < 100;
    if (o.queue) {
        // the launch fills the chip: `pct` per cent of the equal share is dealt out up front, the rest is drawn from the counter
        o.C0 = (int)(o.per * pct / 100);
        o.n_big = 0;
        o.q_first = o.waves * G * (int64_t)o.C0;
    } else {
        // as even as whole pairs allow: every lane group takes floor(P / groups) pairs and the first n_big waves one more
        // (128 x 128 symmetric pairs: 8256 = 4096 groups x 2 + 64 -- an equal share of 3 would run a third fewer waves
        // for a third more macro-steps each)
        const int64_t base = P / (o.waves * G), rem = P - base * o.waves * G;
        o.C0 = (int)base;
        o.n_big = (int)((rem + G - 1) / G);
        if (base == 0) o.waves = o.n_big;                          // no more waves than the pairs need
        o.q_first = P;
    }
    o.row_wprb = 0; o.row_rem = 0; o.row_q0 = 0; o.n_rb = 0;
    return SK_OK;
}

// The launch plan of a ONE-DRAW stream (k_fwd_fused_mb outside split mode, k_deriv_fused, the two multi-band adjoints): a wave sweeps
// one pair at a time and draws pair by pair.  Resident waves per CU of a variant: whole workgroups of wpb0 waves by LDS, by its
// registers, by the family's knob (0: none), at most two per SIMD.
inline int one_draw_waves_per_cu(size_t lds_bytes, int wpb0, int vgprs, int wpc_knob) {
    int wpc = waves_by_vgprs((int)((160 * 1024) / (lds_bytes * wpb0)) * wpb0, vgprs);
    if (wpc_knob > 0 && wpc > wpc_knob) wpc = wpc_knob;
    if (wpc > 8) wpc = 8;
    if (wpc >= wpb0) wpc = wpc / wpb0 * wpb0;
    return wpc < 1 ? 1 : wpc;
}
struct OneDrawPlan {
    int64_t waves, per;       // waves launched; the equal share, pairs per wave
    int64_t q_first;          // the first pair the counter hands out
    int C0;                   // pairs a wave takes up front
    bool queue;               // the counter is used: the caller zeroes it before the launch (else it passes queue = nullptr)
    int64_t ws_waves, ws_doubles;   // the waves the workspace holds a row for, and the doubles that takes: the counter sits behind them
};
// units: bands x units per row of a pair (a wave's steps are counted in 32 bits); pct: per cent of the equal share dealt out up front
// when the launch fills the chip, the rest is drawn from the counter (100: never); ws_stride: workspace doubles per wave.
inline int plan_one_draw(int64_t P, int64_t max_waves, int64_t units, int pct, int64_t ws_stride, OneDrawPlan &o) {
    o.waves = o.ws_waves = P < max_waves ? P : max_waves;
    if (P >= 0x7ff00000LL) return SK_ERR_UNSUPPORTED;            // (pair indices are 32-bit inside the kernels)
    o.per = (P + o.waves - 1) / o.waves;
    if (o.per > 0x1fffffff / units) return SK_ERR_UNSUPPORTED;
    o.ws_doubles = o.waves * ws_stride;
    o.queue = o.waves == max_waves && o.per >= 8 && pct < 100;
    o.C0 = (int)(o.queue ? o.per * pct / 100 : o.per);
    o.q_first = o.queue ? o.waves * (int64_t)o.C0 : P;
    if (!o.queue) o.waves = (P + o.per - 1) / o.per;             // no more waves than the pairs need
    return SK_OK;
}

// ROW-LOCAL dealing: a second look at a plan that uses the counter, for the shared-y order (one_band_geometry: position q is Gram
// row-block q / row_len, column q % row_len; a wave's lane groups keep their x rows for as long as its positions stay inside one
// row-block).  Under the plan above a wave's draws lie `waves` tickets apart -- several row-blocks -- so nearly every drawn position
// brings new rows.  Here every row-block has waves of its own and a counter of its own:
//   * wave w is at home in row-block h = w % n_rb -- waves are dispatched oldest first and run the faster the older they are on
//     their SIMD, so every row-block gets waves of every age; there are wprb = waves / n_rb of them.  Its static share is C0
//     contiguous positions of h, from offset (w / n_rb) C0 on -- the same `pct` per cent of the equal share as above -- and the last wave of h takes row_rem more, so that
//     what is left of the row-block is a whole number of chunks;
//   * the rest of h, offsets [row_q0, row_len), is drawn one chunk at a time from counter h (n_rb counters, zeroed by the caller);
//   * a wave whose row-block is used up moves on to the first following one (wrapping) that has positions left; it finds it by looking
//     at the counters of 64 row-blocks at a time, a bounded number of looks (the kernel's argument), then ends.
// Every wave draws from its HOME counter until that is used up, and every row-block has wprb >= 1 waves at home, so every position is
// handed out -- by its own waves if by nobody else -- whatever the bound; a counter hands out every ticket once.
// Only where the row-blocks divide the launch cleanly: P = n_rb row_len, waves = n_rb wprb, one lap of lanes per position (L <= NUp:
// the lanes that start a pair in one step all start the same position), n_rb counters in the caller's buffer.  Everywhere else the
// plan stays what plan_pair_stream made it, field for field.
inline void plan_row_dealing(int64_t P, int64_t row_len, int NUp, int L, int64_t queue_words, StreamPlan &o) {
    if (!o.queue || row_len <= 0 || P <= 0 || P % row_len != 0 || L > NUp) return;
    const int64_t n_rb = P / row_len;
    if (n_rb > queue_words || o.waves % n_rb != 0 || row_len > 0x3fffffff) return;
    const int64_t wprb = o.waves / n_rb;
    if (wprb < 1 || wprb > 0x7fff) return;
    int64_t c0 = o.C0;
    if (c0 * wprb > row_len) c0 = row_len / wprb;      // (per = ceil(row_len / wprb): only a pct close to 100 gets here)
    const int64_t CQ = (int64_t)1 << o.logC;
    o.C0 = (int)c0;
    o.row_wprb = (int)wprb;
    o.row_rem = (int)((row_len - wprb * c0) % CQ);
    o.row_q0 = (int)(wprb * c0) + o.row_rem;
    o.n_rb = n_rb;
    o.q_first = 0;      // (unused: a draw is its row-block's first position + row_q0 + the ticket)
}

}  // namespace
}  // namespace sk
