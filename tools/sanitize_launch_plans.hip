// The two pure launch planners (csrc/sk_wave_common.h: plan_adjoint_chunks; csrc/sk_pair_stream.h: one_draw_waves_per_cu, plan_one_draw)
// over seeded random shapes, as a stand-alone HOST program for the address and undefined-behaviour sanitizers.  They make no HIP call and
// read no global, so the program needs no device:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I sigkernel_amd/csrc -I include tools/sanitize_launch_plans.hip -o /tmp/sanitize_launch_plans && /tmp/sanitize_launch_plans
// Prints the number of shapes and a checksum of the plans; any report of a sanitizer ends it with a nonzero status.
#include <cstdio>
#include <random>

#include "sk_pair_stream.h"

int main() {
    std::mt19937_64 rng(20240);
    auto pick = [&](std::initializer_list<int64_t> v) { return v.begin()[rng() % v.size()]; };
    auto below = [&](int64_t n) { return (int64_t)(rng() % (uint64_t)(n < 1 ? 1 : n)); };
    uint64_t sum = 0;
    int64_t refused = 0, multi = 0, drawn = 0;
    const int n = 200000;
    for (int i = 0; i < n; ++i) {
        // plan_adjoint_chunks: Grams and paired batches around the resident lane groups, and at the 32-bit guards
        const int G = (int)pick({1, 2, 4, 8}), NUp = (int)pick({8, 16, 24, 32, 64}), n_cu = (int)pick({256, 256, 64, 8, 1});
        const int wpc = (int)pick({1, 4, 8, 8, 12}), knob = (int)pick({0, 0, 1, 2, 4});
        const size_t lds = (size_t)pick({256, 9000, 20000, 45000, 60000, 90000, 160 * 1024});
        const int64_t mg = (int64_t)n_cu * wpc * G;
        int64_t A, B;
        switch (rng() % 5) {
            case 0: A = 1 + below(200 * mg); B = 0; break;
            case 1: A = pick({0x7ff00000LL - 1, 0x7ff00000LL, 0x7fffffffLL}); B = 0; break;
            case 2: B = 1 + below(1 << 12); A = 1 + below(0x7fffffff / B); break;      // (up to the pair-index guard and beyond)
            default: B = pick({1 + below(300), 1 + below(3000), 64, 128, 256, 512, 640, 768, 1536}); A = 1 + below(4 * mg / B + 50); break;
        }
        const int64_t force = B > 0 && rng() % 4 == 0 ? 1 + below(B) : 0;
        sk::AdjointChunks pc{};
        if (sk::plan_adjoint_chunks(A, B, G, NUp, n_cu, wpc, knob, lds, rng() & 1, force, pc)) ++refused;
        else {
            sum += (uint64_t)(pc.PPG + 3 * pc.ppp + 5 * pc.rows_per_launch + 7 * pc.groups);
            multi += pc.rows_per_launch > 0;
        }
        // plan_one_draw: every register count and LDS size a variant may have, pair counts around the resident waves and the guards
        const size_t lds1 = (size_t)pick({1, 9000, 14000, 21000, 41000, 100000, 160 * 1024});
        const int wpb0 = sk::wave_group(lds1, 1 << 20, (int)pick({0, 1, 2, 4})).wpb;
        const int vgprs = (int)pick({1, 64, 128, 129, 168, 169, 256, 300, 512}), wk = (int)pick({0, 0, 1, 2, 6, 8, 12});
        const int64_t mw = (int64_t)n_cu * sk::one_draw_waves_per_cu(lds1, wpb0, vgprs, wk);
        const int64_t P = pick({1 + below(mw + 5), 1 + below(20 * mw), 8 * mw, 8 * mw - 1 > 0 ? 8 * mw - 1 : 1, 0x7ff00000LL - 1, 0x7ff00000LL,
                                mw * (0x1fffffff / 640) + 1});
        sk::OneDrawPlan dp{};
        if (sk::plan_one_draw(P, mw, pick({8, 80, 96, 640, 0x1fffffff}), (int)pick({1, 35, 50, 99, 100}), pick({0, 1000, 1 << 20}), dp)) ++refused;
        else {
            sum += (uint64_t)(dp.waves + 3 * dp.per + 5 * dp.C0 + 7 * dp.q_first + 11 * dp.ws_doubles + (dp.queue ? 13 : 0));
            drawn += dp.queue;
        }
    }
    std::printf("%d shapes: %lld refused, %lld Grams in several launches, %lld launches with the counter, checksum %llu\n", n, (long long)refused,
                (long long)multi, (long long)drawn, (unsigned long long)sum);
    return 0;
}
