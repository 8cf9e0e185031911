// plan_cases.h -- the cases of tests/golden/plan_model_parent.json.gz and the stand-in device they were planned on.
// Shared by tests/helpers/plan_model_check.cpp and by whatever records the golden file from a commit's own planners,
// so the order and the content of the lists must never depend on anything but this file: its own small generator,
// no library distributions.
#pragma once

#include <string.h>

#include <vector>

#include "sm_plan_model.h"

struct PlanCase {
    PlanShape s;
    int cus;             // the stand-in device's CU count: 256 or 32
    int pairs;           // cost cases: pairs of this launch (<= s.max_pairs)
    int aligned4;        // cost cases: both images 4-byte aligned
};

struct PlanLcg {         // (Knuth's MMIX multiplier; the high bits are the random ones)
    unsigned long long x;
    explicit PlanLcg(unsigned long long seed) : x(seed) {}
    unsigned next() { x = x * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(x >> 33); }
    int below(int n) { return (int)(next() % (unsigned)n); }
    int range(int lo, int hi) { return lo + below(hi - lo + 1); }
    template <class T, size_t N> T pick(const T (&a)[N]) { return a[below((int)N)]; }
};

static const int PLAN_SHIFTS[] = {1, 15, 16, 17, 64, 100, 128, 256, 512, 513, 1024, 1025};
static const int PLAN_SIZES[][2] = {{1, 1}, {33, 70}, {384, 288}, {640, 480}, {1000, 37}, {1920, 1080}, {3840, 2160}, {7680, 4320}};
// synth.CONFIGS: C1, C2, C3, C4, C5, REF4K (w, h, D, window, border)
static const int PLAN_CONFIGS[][5] = {{384, 288, 16, 5, 0}, {1920, 1080, 64, 7, 0}, {3840, 2160, 128, 9, 0},
                                      {1920, 1080, 64, 7, 0}, {3840, 2160, 256, 11, 1}, {3840, 2160, 30, 21, 0}};

static inline PlanCase plan_case(int w, int h, int D, int window, int border, int max_pairs, int cus)
{
    PlanCase c;
    memset(&c, 0, sizeof c);
    c.s.w = w; c.s.h = h; c.s.D = D; c.s.border = border; c.s.max_pairs = max_pairs;
    c.s.square_width = std::min(window, std::min(w, h));     // (a plan's window is no larger than its image)
    c.s.opt.struct_size = (int)sizeof(sm_plan_options);
    c.cus = cus; c.pairs = max_pairs; c.aligned4 = 1;
    return c;
}

// option number `k` of the options the match planner reads, at value number `v` of it; false: no such value
static inline bool plan_match_option(sm_plan_options &o, int k, int v)
{
    static const int tile_h[] = {1, 2, 7, 24, 300}, three[] = {4, 8, 16}, two[] = {1, 2}, one[] = {1};
    struct { int *field; const int *values; int count; } t[] = {
        {&o.kernel_family, one, 1}, {&o.tile_h, tile_h, 5}, {&o.shifts_per_lane, three, 3}, {&o.workgroup_waves, two, 2},
        {&o.no_two_wave_cap, one, 1}, {&o.lane_merge, two, 2}, {&o.no_four_shift_lanes, one, 1}};
    if (k < 0 || k >= 7 || v >= t[k].count) return false;
    *t[k].field = t[k].values[v];
    return true;
}

static inline std::vector<PlanCase> plan_match_cases()
{
    std::vector<PlanCase> out;
    PlanLcg r(0x706c616eull);
    for (int cus : {256, 32})
        for (int i = 0; i < 6; i++)
            for (int pairs : {1, 8, 64})
                if (pairs < 64 || i == 3)
                    out.push_back(plan_case(PLAN_CONFIGS[i][0], PLAN_CONFIGS[i][1], PLAN_CONFIGS[i][2], PLAN_CONFIGS[i][3],
                                            PLAN_CONFIGS[i][4], pairs, cus));
    // every odd window x every shift count x both borders, on two sizes each
    for (int n = 1; n <= 27; n += 2)
        for (int D : PLAN_SHIFTS)
            for (int border = 0; border < 2; border++)
                for (int k = 0; k < 2; k++) {
                    const int *sz = PLAN_SIZES[1 + r.below(7)];
                    out.push_back(plan_case(sz[0], sz[1], D, n, border, r.below(4) ? 1 : 8, r.below(2) ? 256 : 32));
                }
    // every option at every value, on a few shapes and both devices
    const int shapes[][5] = {{640, 480, 64, 7, 0}, {640, 480, 128, 11, 1}, {1920, 1080, 64, 7, 0}, {3840, 2160, 256, 13, 1},
                             {384, 288, 16, 5, 0}, {1920, 1080, 100, 21, 0}};
    for (const auto &sh : shapes)
        for (int cus : {256, 32})
            for (int k = 0; k < 7; k++)
                for (int v = 0; v < 5; v++) {
                    PlanCase c = plan_case(sh[0], sh[1], sh[2], sh[3], sh[4], 1, cus);
                    if (plan_match_option(c.s.opt, k, v)) out.push_back(c);
                }
    // seeded shapes from 1 x 1 to 7680 x 4320, a third of them with one or two options set
    while (out.size() < 1500) {
        const bool fixed = r.below(3) == 0;
        const int *sz = PLAN_SIZES[r.below(8)];
        const int w = fixed ? sz[0] : r.range(1, r.below(4) ? 2000 : 7680), h = fixed ? sz[1] : r.range(1, r.below(4) ? 1200 : 4320);
        const int D = r.below(2) ? r.pick(PLAN_SHIFTS) : r.range(1, r.below(4) ? 300 : 1100);
        const int pairs_of[] = {1, 1, 2, 8, 64};
        PlanCase c = plan_case(w, h, D, r.range(0, 28), r.below(2), r.pick(pairs_of), r.below(2) ? 256 : 32);
        for (int k = r.below(3) ? 0 : r.range(1, 2); k > 0; k--) plan_match_option(c.s.opt, r.below(7), r.below(5));
        out.push_back(c);
    }
    return out;
}

static inline std::vector<PlanCase> plan_cost_cases()
{
    std::vector<PlanCase> out;
    PlanLcg r(0x636f7374ull);
    static const int shifts[] = {1, 15, 16, 17, 64, 100, 128, 239, 240, 241, 255, 256, 257, 511, 512, 513};
    static const int tile_h[] = {0, 0, 0, 1, 7, 40, 300}, waves[] = {0, 0, 0, 1, 2, 3, 4}, pairs_of[] = {1, 8, 64};
    // every window 1 .. 23 (across 11 / 13 and 15 / 17) x every shift count x both borders; pairs and alignment in turn
    for (int n = 1; n <= 23; n += 2)
        for (int D : shifts)
            for (int border = 0; border < 2; border++) {
                const int *sz = PLAN_SIZES[2 + r.below(6)];
                PlanCase c = plan_case(sz[0], sz[1], D, n, border, 64, 256);
                c.pairs = pairs_of[out.size() % 3];
                c.aligned4 = (out.size() / 3) % 2;
                out.push_back(c);
            }
    // the options the cost planners read, at each value, on shapes each kernel takes
    const int shapes[][4] = {{3840, 2160, 256, 11}, {1920, 1080, 64, 7}, {640, 480, 128, 15}, {1920, 1080, 100, 21},
                             {384, 288, 16, 5}, {100, 60, 512, 3}};
    for (const auto &sh : shapes)
        for (int pairs : pairs_of)
            for (int k = 0; k < 3; k++)
                for (int v = 0; v < 5; v++) {
                    PlanCase c = plan_case(sh[0], sh[1], sh[2], sh[3], (int)out.size() & 1, 64, 256);
                    c.pairs = pairs;
                    if (k == 0 && v < 2) c.s.opt.cost_kernel = 1 + v;
                    else if (k == 1) c.s.opt.cost_tile_h = tile_h[2 + v];
                    else if (k == 2 && v < 4) c.s.opt.cost_workgroup_waves = 1 + v;
                    else continue;
                    out.push_back(c);
                }
    // seeded shapes
    while (out.size() < 1500) {
        const int *sz = PLAN_SIZES[r.below(8)];
        const bool fixed = r.below(3) == 0;
        const int w = fixed ? sz[0] : r.range(1, r.below(4) ? 2000 : 7680), h = fixed ? sz[1] : r.range(1, r.below(4) ? 1200 : 4320);
        PlanCase c = plan_case(w, h, r.below(2) ? r.pick(shifts) : r.range(1, 520), r.range(1, 23), r.below(2), 64, 256);
        c.pairs = r.pick(pairs_of);
        c.aligned4 = r.below(4) != 0;
        c.s.opt.cost_tile_h = r.pick(tile_h);
        c.s.opt.cost_workgroup_waves = r.pick(waves);
        out.push_back(c);
    }
    return out;
}

// further seeded shapes for the property sweep (no golden): `i` of a stream of its own
static inline PlanCase plan_sweep_case(PlanLcg &r)
{
    const int w = r.range(1, r.below(8) ? 2500 : 7680), h = r.range(1, r.below(8) ? 1500 : 4320);
    const int pairs_of[] = {1, 1, 2, 8, 64};
    PlanCase c = plan_case(w, h, r.below(3) ? r.range(1, 520) : r.range(1, 1100), r.range(0, 28), r.below(2), r.pick(pairs_of),
                           r.below(2) ? 256 : 32);
    for (int k = r.below(2) ? 0 : r.range(1, 3); k > 0; k--) plan_match_option(c.s.opt, r.below(7), r.below(5));
    c.pairs = 1 + r.below(c.s.max_pairs);
    c.aligned4 = r.below(4) != 0;
    if (!r.below(3)) c.s.opt.cost_tile_h = r.range(1, 200);
    if (!r.below(3)) c.s.opt.cost_workgroup_waves = r.range(1, 4);
    if (!r.below(16)) c.s.opt.cost_kernel = 1;
    return c;
}

// ---------------------------------------------------------------------------
// The stand-in device.  Not a true one: a fixed formula of (kernel, threads, LDS) that both the recorded planners
// and the model are asked, varied enough to reach the planners' multi-round, two-wave-variant and LDS-pad branches.
// Workgroups per CU = the lesser of an LDS bound (160 KB over the request rounded up to 1280 bytes) and a register
// bound: 512 registers a SIMD over the kernel's VGPRs rounded up to 8, four SIMDs, over the workgroup's waves.
// VGPRs of k_match_bs<n, ds, full D, toroidal> from profiles/r06/resource_usage.txt; a ghost build takes ~9 more,
// a partial-D one 1 more, a two-wave variant or a two-wave workgroup at least 176.
// ---------------------------------------------------------------------------
static inline int standin_vgprs(const KernelKey &k)
{
    static const int v16[] = {162, 192, 210, 232, 238};
    static const int v8[] = {128, 139, 166, 174, 182, 198, 210, 227, 234, 242};
    static const int v4[] = {106, 118, 123, 138, 142, 154, 163, 175, 183, 191};
    if (k.family != SM_KERNEL_BS) return k.family == SM_KERNEL_A ? 64 : k.family == SM_KERNEL_B ? 96 : 128;
    const int i = (k.n - 3) / 2;
    int v = k.ds == 16 ? v16[std::min(i, 4)] : k.ds == 8 ? v8[std::min(i, 9)] : v4[std::min(i, 9)];
    v += (k.ghost ? 9 : 0) + (k.fulld ? 0 : 1);
    if (k.cap2 || k.duo) v = std::max(v, 176);
    return std::min(v, 256);
}

static inline int standin_occupancy(const KernelKey &k, int threads, int lds_bytes)
{
    const int per_simd = std::min(8, 512 / ((standin_vgprs(k) + 7) / 8 * 8));
    const int by_regs = 4 * per_simd / ((threads + 63) / 64);
    const int by_lds = lds_bytes > 0 ? 160 * 1024 / ((lds_bytes + 1279) / 1280 * 1280) : 32;
    return std::max(0, std::min(32, std::min(by_regs, by_lds)));
}
