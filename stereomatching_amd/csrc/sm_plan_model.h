// sm_plan_model.h -- launch planning as plain C++17: what kernel a plan runs and with what geometry, and the
// geometry of the SAD / SSD cost mode's fast kernels.  No HIP: the library (sm_match.hip, sm_cost_*.hip) wraps the
// runtime's answers into a PlanDevice and maps kernel keys to functions; tests/helpers/plan_model_check.cpp runs the
// same functions on the CPU against a stand-in device.  No heap, no std::function: the cost planners run per launch.
//
//   sm_lanes_for, sm_rows_for_grid        rules more than one planner applies
//   sm_bs_built, sm_bs_default_ds         which bit-sliced builds exist (the table sm_bs_kernel_ptr must agree with)
//   sm_plan_family                        popcount A / B / C, generic or bit-sliced
//   match_generic / match_row_layout / MatchLds / match_lane_merge / match_tile_search / match_spread /
//   match_configure / match_configure_best / match_shifts_per_lane / match_describe
//   sm_plan_match                         all of the above: shape + device -> kernel, MatchGeom, describe string
//   cost_tile_search                      the one tile-height search of the cost planners
//   sm_plan_sad_pc / sm_plan_sad_qs / sm_plan_ssd_mfma     shape -> SadGeom and the kernel's key
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdio.h>

#include <algorithm>

#include "sm_geom.h"
#include "stereo_hip.h"

// ---------------------------------------------------------------------------
// inputs
// ---------------------------------------------------------------------------

struct PlanShape {
    int w, h, D, square_width, border, max_pairs;
    sm_plan_options opt;
};

// a kernel as a value: the launch side maps it to a function (tiled_kernel_ptr, sm_bs_kernel_ptr)
struct KernelKey {
    int family;          // SM_KERNEL_*
    int n, ds;           // window, shifts per lane
    bool fulld, ghost, cap2, duo;
};

// the device's facts: the CU count, and how many workgroups of kernel `k` with `threads` threads and `lds_bytes` of
// LDS fit a CU (0: the runtime gave no answer)
struct PlanDevice {
    int cus;
    int (*occupancy)(void *ctx, const KernelKey &k, int threads, int lds_bytes);
    void *ctx;
    int fit(const KernelKey &k, int threads, int lds_bytes) const { return occupancy(ctx, k, threads, lds_bytes); }
};

// ---------------------------------------------------------------------------
// rules more than one planner applies
// ---------------------------------------------------------------------------

static inline int sm_ceil_div(int a, int b) { return (a + b - 1) / b; }

// lanes that split a range of `range` shifts (or shift quads) at `per_lane` each: the power of two that covers it
static inline int sm_lanes_for(int range, int per_lane, int *log2nl)
{
    int nl = 1;
    *log2nl = 0;
    while (nl * per_lane < range) { nl <<= 1; (*log2nl)++; }
    return nl;
}

// tile height of the kernels without a cost model (the general cost kernel, the census arg-min): 64 rows, halved
// (not below 8) while the grid has fewer than 1024 tiles
static inline int sm_rows_for_grid(int tiles_x, int h, int pairs)
{
    int th = 64;
    while (th > 8 && (long long)tiles_x * ((h + th - 1) / th) * pairs < 1024) th >>= 1;
    return th;
}

// Built combinations of the bit-sliced kernel (fulld and ghost: all four of each).  16 shifts per lane up to 11 x 11
// (the 16 x SB sum planes fit two waves per SIMD); 8 per lane for the larger windows (9 planes per sum) and, for the
// smaller ones, as the alternative for grids that would leave SIMDs with a single wave; 4 per lane for all.
// cap2: the two-waves-per-SIMD variant (none where the kernel is limited to two waves by its registers anyway).
// duo: two-wave workgroups -- one build per window, limited to two waves per SIMD wherever the registers would
// allow three (cap2 is not a choice there).
constexpr bool sm_bs_built(int n, int ds, bool cap2, bool duo)
{
    if (n < 3 || !(n & 1) || (duo && cap2)) return false;
    return ds == 16 ? n <= 11 && !(cap2 && n > 7)
         : ds == 8  ? n <= 21 && !(cap2 && n > 15)
         : ds == 4  ? n <= 21 : false;
}
constexpr bool sm_kernel_built(const KernelKey &k)
{
    return k.family == SM_KERNEL_BS ? sm_bs_built(k.n, k.ds, k.cap2, k.duo)
         : k.family >= SM_KERNEL_A && k.family <= SM_KERNEL_C && !k.cap2 && !k.duo;
}
// shifts per lane the plan should use for this window (0: not built)
constexpr int sm_bs_default_ds(int n) { return sm_bs_built(n, 16, false, false) ? 16 : sm_bs_built(n, 8, false, false) ? 8 : 0; }

// ---------------------------------------------------------------------------
// the match stage
// ---------------------------------------------------------------------------

// the bit-sliced kernel where it is built (common windows, D <= 512);
// sm_plan_options.kernel_family = 1 keeps the general kernels (A/B testing)
static inline int sm_plan_family(const PlanShape &s)
{
    const int n = 2 * (s.square_width / 2) + 1;
    int kernel;
    if (s.D > (1 << SM_KEY_DBITS) || n > 25) kernel = SM_KERNEL_GENERIC;
    else if (n <= 9) kernel = SM_KERNEL_A;
    else if (n <= 16) kernel = SM_KERNEL_B;
    else kernel = SM_KERNEL_C;
    int l2;
    const int ds0 = sm_bs_default_ds(n);
    if (s.opt.kernel_family != 1 && kernel != SM_KERNEL_GENERIC && ds0 && sm_lanes_for(s.D, ds0, &l2) <= 32)
        kernel = SM_KERNEL_BS;
    return kernel;
}

// what every step below reads: the shape, the device, the family, and the geometry's fields that no choice changes
struct MatchPlanner {
    const PlanShape &s;
    const PlanDevice &dev;
    int kernel;
    bool bs, ghost;
    MatchGeom base;          // w, h, D, n, half, pad_l; everything else 0
};

// generic kernel: 1 lane per pixel, no tiles
static inline void match_generic(MatchGeom &g)
{
    g.pad_l = 32 * sm_ceil_div(std::max(g.half, 1), 32);
    // word() reads 2 words starting at bit x+d+pad_l with x <= W-1+half
    g.ext_words = (g.pad_l + g.w + g.half + g.D + 31) / 32 + 2;
    g.ext_rows = g.h + 2 * g.half;
    g.ext_image_words = (long long)g.ext_words * g.ext_rows;
    g.edge_words_l = g.edge_words_r = g.ext_words;
}

// lanes, threads, tile width and staged-row words for `ds` shifts per lane; returns the words of one staged row pair
static inline int match_row_layout(const MatchPlanner &p, int ds, bool duo, MatchGeom &o)
{
    o.ds = ds;
    o.duo = duo ? 1 : 0;
    o.nl = sm_lanes_for(o.D, ds, &o.log2nl);
    int rows_words;
    if (p.bs) {
        // one wave per workgroup: 64/nl words of 32 pixels, nl shift-lanes each
        o.runs = 64 / o.nl;
        o.threads = duo ? 128 : 64;     // duo: two waves, the upper and the lower half of the tile
        o.tw = o.runs * 32;
        o.plw = o.runs + 2;
        o.prw = o.runs + (o.nl * ds + 31) / 32 + 4;
        rows_words = o.plw + o.prw;
    } else {
        o.runs = o.nl == 1 ? 64 : (o.nl <= 8 ? 32 : 256 / o.nl);
        o.threads = o.runs * o.nl;
        o.tw = o.runs * SM_P;
        o.plw = (SM_PADT + o.tw + o.half + 31) / 32 + 1;
        o.prw = (SM_PADT + o.tw + o.half + o.nl * ds + 31) / 32 + 1;
        rows_words = (o.plw + o.prw) * 3;     // plain + spread
    }
    o.tiles_x = sm_ceil_div(o.w, o.tw);
    return rows_words;
}

// Lane merge through LDS (k_match_bs, g.xmerge): where at least 4 lanes share a word.
// Taken where it pays: 16 shifts per lane and at least 8 lanes per word (C3: -4.3 % of the launch's
// VALU instructions, -3 % of its time; C5: -10 %).  With 4 lanes per word there are only two DPP levels
// to save and the batch's bursts of stores cost more than that (C4 x 8: +5 %); the 8-shifts-per-lane
// builds run 4- to 9-row tiles, whose last batch is mostly empty.  lane_merge = 2 forces it wherever
// it is possible (tests, measurements), 1 forbids it.  profiles/r04/ab_lane_merge.txt
static inline bool match_lane_merge(const MatchPlanner &p, const MatchGeom &o)
{
    const bool xm_possible = p.bs && o.log2nl >= 2 && o.nl <= 32;
    return xm_possible && p.s.opt.lane_merge != 1 &&
           (p.s.opt.lane_merge == 2 || ((o.ds == 16 || o.ds == 4) && o.log2nl >= 3));
}

// lane-row work relative to ds = 16: the per-row shared views and the merge levels weigh more the fewer
// shifts a lane carries (fitted to same-device timings: profiles/r02/ds8_small_grids_sweep.txt, r04/ab_ds4.txt)
// (round 4, tools/ds_choice_check.py over 14 shapes: 8 shifts per lane was the best of the three ONCE and
// was chosen seven times -- its weight went from 0.55 to 0.65, the LDS-merged 4-shift build's from 0.36 to
// 0.33, and a 16-shift row whose lanes are merged through LDS counts 0.95)
static inline double match_row_work(const MatchGeom &o)
{
    return o.ds == 16 ? (o.xmerge ? 0.95 : 1.0) : o.ds == 8 ? 0.5 * 1.30
         : o.xmerge ? 0.25 * 1.32 : 0.25 * (1.30 + 0.15 * o.log2nl);
}

// warm-up rows are cheaper than output rows (no arg-max, no output); the constant is
// the per-workgroup overhead (staging, lane set-up) in output-row units.  Refit on
// same-device tile-height sweeps (tools/tune_tile_h.py, C2 / C3 / C4 x 8).
// (duo: half the window rows + 1, and the exchange of the partial sums)
static inline double match_warm_rows(const MatchPlanner &p, const MatchGeom &o)
{
    return o.duo ? 0.42 * (o.half + 1) + 2.3 : p.bs ? 0.42 * (o.n - 1) + 1.8 : 0.4 * (o.n - 1) + 1.0;
}

// LDS words of a workgroup whose waves put out `th` rows each.
// duo: 2 * th rows per workgroup, and behind the staged rows the exchange block
// [2 halves of the shifts][ds / 2 * SB / 2 plane pairs][64 lanes] of 8 bytes.
// xmerge: per wave 4 x NPG blocks of 1 KB behind the staged rows, in a two-wave workgroup over the exchange slots
struct MatchLds {
    bool bs, duo;
    int n, ds, rows_words, rows_per_wg, sb, mb_words;

    MatchLds(const MatchPlanner &p, const MatchGeom &o, int rows_words_)
        : bs(p.bs), duo(o.duo != 0), n(o.n), ds(o.ds), rows_words(rows_words_), rows_per_wg(o.duo ? 2 : 1)
    {
        sb = 0;
        while ((1 << sb) <= n * n) sb++;
        const int ab = ds == 16 ? 4 : ds == 8 ? 3 : 2;
        const int npg = (sb + ab + 3) / 4;
        mb_words = o.xmerge ? npg * 1024 : 0;
    }
    int words(int th, int &xm_off) const
    {
        const int staged = ((rows_per_wg * th + n - 1) * rows_words + 3) & ~3;
        if (!bs) { xm_off = 0; return (rows_per_wg * th + n - 1) * rows_words; }
        if (duo) {
            const int slot = ds * sb * 32;                    // words of one exchange slot
            const int half = std::max(slot, mb_words);
            xm_off = staged + half;
            return staged + 2 * half;
        }
        xm_off = staged;
        return staged + mb_words;
    }
    int bytes(int th) const { int off; return words(th, off) * 4; }
};

// Tile height by a cost model.  Tall tiles amortise the n-1 warm-up rows, but the grid should fill the
// chip's resident slots in whole rounds: a tail round with a third of the CUs busy
// costs as much as a full one.  Model: a workgroup puts threads/256 waves on each
// SIMD; a SIMD issues one wave-instruction per 2 cycles, a single wave at most one
// per 4; rounds run back to back; the work of a lane-row is proportional to ds.
// Returns the height (0: none fits) and its cost.
static inline int match_tile_search(const MatchPlanner &p, const MatchGeom &o, const MatchLds &lds, const KernelKey &k,
                                    double *best_cost_o)
{
    const int H = o.h, cus = p.dev.cus;
    const double wps = o.threads / 256.0;            // waves per SIMD per workgroup
    const double warm = match_warm_rows(p, o), work = match_row_work(o);
    int th = 0;
    double best_cost = 0;
    for (int c = 2; c <= 256; c++) {
        if (c > H && c != 2) break;
        const int cand = std::min(c, H);
        if (lds.bytes(cand) > 64 * 1024) break;
        int per_cu = p.dev.fit(k, o.threads, lds.bytes(cand));
        if (per_cu < 1) per_cu = 1;
        const long long tiles = (long long)o.tiles_x * sm_ceil_div(H, lds.rows_per_wg * cand) * p.s.max_pairs;
        const long long slots = (long long)cus * per_cu;
        double cost = 0;
        for (long long left = tiles; left > 0; left -= slots) {
            const long long m = std::min(left, slots);
            // the busiest SIMD of this round hosts j waves; measured: one wave alone
            // retires an instruction every ~5.5 cycles (popcount kernels; ~4.3 for the
            // bit-sliced kernel), two co-resident waves ~5.5 each, beyond that they
            // share ~2.5 cycles/instr
            const long long wg_per_cu = (m + cus - 1) / cus;
            const int j = std::max(1, (int)ceil((double)wg_per_cu * wps - 1e-9));
            const double cpi = p.bs ? (j <= 1 ? 4.3 : std::max(5.5, 2.5 * j)) : std::max(5.5, 2.5 * j);
            cost += (cand + warm) * work * cpi;
        }
        if (th == 0 || cost < best_cost * 0.999) { th = cand; best_cost = cost; }
    }
    *best_cost_o = best_cost;
    return th;
}

// A grid that fits the chip in one round must also be SPREAD evenly: where the
// registers allow more resident workgroups than the round needs (7x7: 3 waves
// per SIMD, 2 needed) the dispatcher may stack 3 waves on some SIMDs and leave
// others with 1, and the launch then lasts as long as the crowded ones (measured
// at 8 x 1080p: 89 us spread evenly, 117 us not).  Two caps:
//  * per SIMD: a grid that fits at two waves per SIMD launches the kernel's
//    two-wave variant (k_match_bs<..., CAP2>), where one exists;
//  * per CU: an LDS request larger than the tile needs -- LDS per workgroup in
//    (160 KB / (cap + 1), 160 KB / cap] admits exactly `cap` workgroups per CU.
// Sets o.cap2 and may raise o.lds_bytes.
static inline void match_spread(const MatchPlanner &p, MatchGeom &o, const KernelKey &k)
{
    o.cap2 = 0;
    if (!p.bs) return;
    const int cus = p.dev.cus;
    const long long tiles = (long long)o.tiles_x * o.tiles_y * p.s.max_pairs;
    const int cap = (int)((tiles + cus - 1) / cus);
    KernelKey kuse = k;
    if (sm_bs_built(k.n, k.ds, true, k.duo) && cap <= 8 && !p.s.opt.no_two_wave_cap) { o.cap2 = 1; kuse.cap2 = true; }
    const int per_cu = p.dev.fit(kuse, o.threads, o.lds_bytes);
    if (cap >= 2 && cap < per_cu) {
        const int lds_cu = 160 * 1024, granule = 1280;
        const int want = std::min(64 * 1024, lds_cu / cap / granule * granule);
        if (want > o.lds_bytes && p.dev.fit(kuse, o.threads, want) == cap) o.lds_bytes = want;
    }
}

// the geometry for `ds` shifts per lane and this workgroup shape; returns the cost of its tile height
static inline double match_configure(const MatchPlanner &p, int ds, bool duo, MatchGeom &o)
{
    o = p.base;
    const int rows_words = match_row_layout(p, ds, duo, o);
    const KernelKey k = {p.kernel, o.n, ds, o.nl * ds == o.D, p.ghost, false, duo};
    o.xmerge = match_lane_merge(p, o);
    const MatchLds lds(p, o, rows_words);
    double best_cost;
    int th = match_tile_search(p, o, lds, k, &best_cost);
    if (th == 0) th = 1;
    if (p.s.opt.tile_h > 0) th = std::min(p.s.opt.tile_h, o.h);       // sm_plan_create_ex: tuning / tests only
    while (lds.bytes(th) > 64 * 1024 && th > 1) th--;
    o.tile_h = th;
    o.tiles_y = sm_ceil_div(o.h, lds.rows_per_wg * th);
    o.nsr = lds.rows_per_wg * th + o.n - 1;
    o.lds_bytes = lds.words(th, o.xm_off) * 4;
    o.xm_words = lds.mb_words;
    match_spread(p, o, k);
    o.ext_words = (o.tiles_x - 1) * (o.tw / 32) + o.prw;
    o.ext_rows = o.tiles_y * lds.rows_per_wg * th + o.n - 1;
    o.ext_image_words = (long long)o.ext_words * o.ext_rows;
    o.vec_ok = (o.w % 4) == 0;
    return best_cost;
}

// Two-wave workgroups with a shared warm-up (k_match_bs<..., DUO>): HALF + 1 warm-up rows
// per wave instead of N, for an exchange through LDS.  Measured on one device at the same
// tile height (tools/ab_duo.sh): C3 95.3 -> 92.1 us, C4 x 8 83.6 -> 80.5, C5 197.9 -> 185.9,
// C2 20.5 -> 19.4, 21 x 21 at 4K 88.5 -> 77.4, C1 9.9 -> 10.0: taken wherever the cost
// model says so (sm_plan_options.workgroup_waves overrides: tuning, tests).
// The lower-cost geometry of the two workgroup shapes for `d` shifts per lane.
static inline double match_configure_best(const MatchPlanner &p, int d, MatchGeom &o)
{
    const int duo_env = p.s.opt.workgroup_waves ? p.s.opt.workgroup_waves == 2 : -1;
    const bool can = p.bs && sm_bs_built(p.base.n, d, false, true);
    double c1 = 0, c2 = 0;
    if (!(can && duo_env == 1)) c1 = match_configure(p, d, false, o);
    if (can && duo_env != 0) {
        MatchGeom o2;
        c2 = match_configure(p, d, true, o2);
        if (duo_env == 1 || c2 < c1) { o = o2; return c2; }
    }
    return c1;
}

// Shifts per lane: 16 for the popcount kernels; for the bit-sliced kernel what is
// built for this window (16 where it exists: measured faster than 8, fewer shared
// views and merge levels), sm_plan_options.shifts_per_lane overrides for tuning.
static inline int match_shifts_per_lane(const MatchPlanner &p)
{
    if (!p.bs) return 16;
    const PlanShape &s = p.s;
    const int n = p.base.n, ds_env = s.opt.shifts_per_lane;
    int l2;
    auto usable = [&](int d) { return sm_bs_built(n, d, false, false) && sm_lanes_for(s.D, d, &l2) <= 32; };
    const int ds = sm_bs_default_ds(n);
    if ((ds_env == 4 || ds_env == 8 || ds_env == 16) && usable(ds_env)) return ds_env;
    // A grid that leaves most SIMDs with ONE wave (a single 1080p pair at 16 shifts per lane: 864
    // workgroups) runs at the rate of a lone wave; with 8 -- or 4 -- shifts per lane the same job is
    // more workgroups of less work each, on narrower tiles that can be taller for the same number of
    // waves (less warm-up per output row).  The cost model decides, with 5 % in favour of the wider
    // lane.  Measured: C2 29.6 (16) -> 19.1 (8) -> 16.5 us (4, lanes merged through LDS), C1 18.4 ->
    // 9.8 -> 7.2 us; the full-chip configurations stay at 16 (profiles/r04/ab_ds4.txt).
    // What the model cannot see -- the narrow lanes win by latency hiding on grids that leave the chip
    // partly empty, not by instruction count -- is put in as a rule taken from tools/ds_choice_check.py
    // (14 shapes, profiles/r04/ds_choice_*.txt): below 0.3 G pixel-shifts per launch, or for windows of
    // 13 x 13 and more (their warm-up weighs less on narrow, tall tiles), all three are candidates; above
    // it a window that has a 16-shift build takes it (the worst miss of this rule: 5 %).
    const double pxshifts = (double)s.w * s.h * s.D * s.max_pairs;
    const bool small_or_tall = pxshifts <= 0.3e9 || n >= 13;
    const bool has8 = usable(8);
    const bool has4 = s.opt.no_four_shift_lanes == 0 && small_or_tall && usable(4);
    double cbest = 0;
    int dbest = 0;
    for (int d : {16, 8, 4}) {
        if (d == 16 && ds != 16) continue;          // (windows whose 16-shift build does not exist)
        if (d == 8 && (!has8 || (ds == 16 && !small_or_tall))) continue;
        if (d == 4 && !has4) continue;
        MatchGeom gd = p.base;
        const double c = match_configure_best(p, d, gd);
        if (!dbest || c < 0.95 * cbest) { dbest = d; cbest = c; }
    }
    return dbest ? dbest : ds;
}

static inline void match_describe(const MatchPlanner &p, const MatchGeom &g, char *text, size_t size)
{
    if (p.kernel == SM_KERNEL_GENERIC) {
        snprintf(text, size, "generic kernel (n=%d, D=%d): 1 lane/pixel, direct window sums", g.n, g.D);
        return;
    }
    snprintf(text, size,
             "%s (n=%d, D=%d, %s): tile %dx%d px, %d threads "
             "(%d runs x %d shift-lanes of %d), grid %dx%d, LDS %d B/wg%s%s, ext %dx%d words",
             p.bs ? "bit-sliced kernel" : p.kernel == SM_KERNEL_A ? "tiled kernel A"
                  : p.kernel == SM_KERNEL_B ? "tiled kernel B" : "tiled kernel C",
             g.n, g.D, p.ghost ? "ghost" : "toroidal",
             g.tw, g.duo ? 2 * g.tile_h : g.tile_h, g.threads, g.runs, g.nl, g.ds, g.tiles_x, g.tiles_y, g.lds_bytes,
             g.duo ? ", two-wave workgroups" : g.cap2 ? ", 2 waves/SIMD variant" : "",
             g.xmerge ? ", lanes merged through LDS" : "",
             g.ext_words, g.ext_rows);
}

// the kernel a geometry launches
static inline KernelKey sm_match_kernel_key(int kernel, const MatchGeom &g, bool ghost)
{
    return {kernel, g.n, g.ds, g.nl * g.ds == g.D, ghost, g.cap2 != 0, g.duo != 0};
}

// shape + device -> the plan's kernel family (returned), geometry and describe string.  dev.cus and dev.occupancy are
// read only where sm_plan_family(s) is not SM_KERNEL_GENERIC.
static inline int sm_plan_match(const PlanShape &s, const PlanDevice &dev, MatchGeom *g, char *describe, size_t describe_size)
{
    const int kernel = sm_plan_family(s);
    MatchPlanner p = {s, dev, kernel, kernel == SM_KERNEL_BS, s.border == SM_GHOST, MatchGeom()};
    p.base.w = s.w; p.base.h = s.h; p.base.D = s.D;
    p.base.half = s.square_width / 2;
    p.base.n = 2 * p.base.half + 1;
    if (kernel == SM_KERNEL_GENERIC) {
        *g = p.base;
        match_generic(*g);
    } else {
        p.base.pad_l = SM_PADT;
        *g = p.base;
        match_configure_best(p, match_shifts_per_lane(p), *g);
        g->edge_words_l = std::min(g->ext_words, (g->pad_l + s.w + g->half - 1) / 32 + 1);
        g->edge_words_r = std::min(g->ext_words, (g->pad_l + s.w + g->half + s.D - 2) / 32 + 1);
    }
    match_describe(p, *g, describe, describe_size);
    return kernel;
}

// ---------------------------------------------------------------------------
// the SAD / SSD cost mode's fast kernels
// ---------------------------------------------------------------------------

enum { SM_COST_KERNEL_NONE = 0, SM_COST_KERNEL_SAD_PC, SM_COST_KERNEL_SAD_QS, SM_COST_KERNEL_SSD_MFMA };
// a fast cost kernel as a value: k_sad_pc<n, nql, px>, k_sad_qs<n, nql, px> or k_ssd_mfma<n, nb>; family NONE: the
// shape is not built (the caller falls back)
struct CostKernelKey {
    int family, n, nql, px, nb;
};

// k_ssd_mfma<N, NB>: waves per SIMD the register count allows (the NB x 16 accumulators are most of it); the
// kernel's __launch_bounds__ and the planner's resident slots
constexpr int mfma_waves(int nb) { return nb <= 3 ? 4 : nb <= 5 ? 3 : 2; }

struct CostRows { int lrow, rrow, tw, tail; };      // staged row bytes, tile width and LDS bytes behind the rows, for a width
struct CostTile { int th, wv; double cost; };       // th 0: no width fits
// what differs between the three planners (on purpose: each was fitted to its own kernel)
struct CostSearch {
    int n, w, h, pairs;
    int slots;               // resident waves of the chip
    double warm;             // cost of a warm-up row in output rows
    size_t cap_per_wave;     // LDS a workgroup may take, per wave of it ...
    size_t cap_total;        // ... and in all
    double wider;            // a wider workgroup is taken at this fraction of the best cost (0.97)
    bool skip_two;           // two-wave workgroups only when asked for
    bool wide_break;         // a workgroup wider than the image ends the search
    bool reach;              // the rows must be within the fast staging path's reach (4 dwords a lane)
};

// Tile height and workgroup width (1, 2 or 4 waves; only `only` if not 0) together: whole rounds of the resident waves;
// rows + weighted warm-up + staging per workgroup.  rows(wv) gives the staged rows of a width.
// (always inlined: the callers' values are literals, and `slots` a power of two in two of the three; out of line
// the search divides by it at run time, measured 80 -> 126 ns a call of k_sad_pc's planner, profiles/r07/ab_planner.txt)
template <class Rows>
#if defined(__GNUC__)
__attribute__((always_inline))
#endif
static inline CostTile cost_tile_search(const CostSearch &p, int only, Rows rows)
{
    CostTile best = {0, 0, 0};
    for (int wv = 1; wv <= 4; wv *= 2) {
        if (only ? only != wv : (p.skip_two && wv == 2)) continue;
        const CostRows r = rows(wv);
        if (p.wide_break && wv > 1 && r.tw / 2 >= p.w) break;              // (a workgroup wider than the image)
        if (p.reach && r.lrow + r.rrow > 4 * 4 * 64 * wv) continue;         // (the fast staging path's reach)
        const int tiles_x = (p.w + r.tw - 1) / r.tw;
        for (int th = 8; th <= 128; th += 4) {
            const size_t lds = (size_t)(th + p.n - 1) * (r.lrow + r.rrow) + (size_t)r.tail;
            if (lds > (size_t)wv * p.cap_per_wave || lds > p.cap_total) break;
            const long long waves = (long long)tiles_x * ((p.h + th - 1) / th) * p.pairs * wv;
            const long long rounds = (waves + p.slots - 1) / p.slots;
            const double cost = (double)rounds * (th + p.warm * (p.n - 1) + 2.0);
            if (!best.th || cost < best.cost * (wv > best.wv ? p.wider : 1.0)) best = {th, wv, cost};
        }
    }
    return best;
}

// what the two quad-SAD planners share: the quads of a lane, the lanes, the pad and the quad bounds
static inline void cost_sad_lanes(SadGeom &g, int half, int nql)
{
    const int nq = (g.D + 3 + 3) / 4;               // quads that cover shifts -3 .. D-1
    g.nl = sm_lanes_for(nq, nql, &g.log2nl);
    g.padl = 4 * ((half + 3 + 3) / 4);
    // last quad (of the last shift-lane) whose four shifts are all below D for every lane: rho <= 3
    g.q_tail = (g.D - 4 * (g.nl - 1) * nql) / 4;
    if (g.q_tail < 0) g.q_tail = 0;
    // ... and the last quad that holds a shift below D for some lane (rho = 3); with several
    // shift-lanes the lower ones need all their quads
    g.q_last = g.nl > 1 ? nql - 1 : (g.D + 2) / 4;
    if (g.q_last > nql - 1) g.q_last = nql - 1;
}

// the fields every planner sets once height and width are known; lds_tail: the bytes behind the staged rows
static inline void cost_finish(SadGeom &g, int n, int th, bool aligned4, int reach, int lds_tail)
{
    g.tile_h = th < g.h ? th : g.h;
    g.tiles_y = (g.h + g.tile_h - 1) / g.tile_h;
    g.nsr = g.tile_h + n - 1;
    g.fast_stage = g.w % 4 == 0 && aligned4 && g.lrow + g.rrow <= reach;
    g.lds_bytes = g.nsr * (g.lrow + g.rrow) + lds_tail;
}

// k_sad_pc: SAD with the window rows formed by prefix chains along the row (windows up to 15 x 15, up to 512 shifts).
// aligned4: both images are 4-byte aligned.
static inline CostKernelKey sm_plan_sad_pc(const PlanShape &s, int pairs, bool aligned4, SadGeom *out)
{
    const CostKernelKey none = {SM_COST_KERNEL_NONE, 0, 0, 0, 0};
    SadGeom g;
    g.tbl_pad = 0;                          // (the SSD kernel's)
    g.w = s.w; g.h = s.h; g.D = s.D;
    const int half = s.square_width / 2, n = 2 * half + 1;
    g.ghost = s.border == SM_GHOST;
    if (n < 3 || n > 15 || g.D > 512 || s.opt.cost_kernel == 1) return none;
    const int nq0 = (g.D + 3 + 3) / 4;
    const int px = 4;
    const int nql = nq0 <= 5 ? 5 : nq0 <= 9 ? 9 : 17;
    cost_sad_lanes(g, half, nql);
    if (g.nl > 16) return none;
    const int ng = n / 4 + 1;
    // Workgroup = 1, 2 or 4 waves side by side (each its own 64 / nl pixel groups) sharing the staged rows: with many
    // shifts a lone wave's tile is narrow (64 pixels at 256 shifts) under a right-image span of 4 (nl nql + ..) bytes,
    // its 20 KB of LDS hold few rows and the n - 1 warm-up rows weigh a quarter of the launch (C5: 16-row tiles);
    // four waves share one span and slide 64 rows.  Tile height and workgroup width together: whole rounds of two
    // waves per SIMD, rows + warm-up (a warm-up row costs ~0.41 of an output row here) + staging per workgroup.
    auto rows = [&](int wv) {
        CostRows r;
        r.tw = 4 * px * (16 / g.nl) * wv;
        // left row: dwords up to bL2 + PX - 1 (<= bL + FG + PX) of the last pixel group; right: aligned up to
        // bR + NQL - 1 + max(NG, PX - 1) + 1, shifted up to bR + NQL - 1 + FG + PX - 1 + 1 (+1: the bytes they are cut from)
        r.lrow = 8 * ((g.padl + r.tw + 4 * (ng + 3) + 7) / 8);
        r.rrow = 8 * ((g.padl + r.tw + 4 * (g.nl * nql + ng + px + 2) + 7) / 8);
        r.tail = 4 * r.rrow;
        return r;
    };
    CostSearch p = {n, g.w, g.h, pairs, 256 * 4 * 2, 0.41, 160 * 1024 / 8, (size_t)-1, 0.97, false, true, true};
    CostTile best = cost_tile_search(p, 0, rows);
    if (!best.th) return none;
    const int asked = s.opt.cost_workgroup_waves;
    if ((asked == 1 || asked == 2 || asked == 4) && asked != best.wv) {
        // an explicit width applies where the staging path reaches it (the height the model gives that width)
        const CostRows r = rows(asked);
        if (r.lrow + r.rrow <= 4 * 4 * 64 * asked) {
            p.wide_break = false;
            best = cost_tile_search(p, asked, rows);
            if (!best.th) best.th = 8;
            best.wv = asked;
        }
    }
    g.waves = best.wv;
    const CostRows r = rows(g.waves);
    g.tw = r.tw; g.lrow = r.lrow; g.rrow = r.rrow;
    g.tiles_x = (g.w + g.tw - 1) / g.tw;
    const size_t lds_cap = (size_t)g.waves * 160 * 1024 / 8;      // (beyond 64 KB: sm_cost_wta raises the kernel's limit)
    int th = best.th;
    if (s.opt.cost_tile_h > 0) th = s.opt.cost_tile_h;      // an explicit tile height, clamped to what a workgroup's LDS holds
    while (th > 1 && (size_t)(th + n - 1) * (g.lrow + g.rrow) + 4 * (size_t)g.rrow > lds_cap) th--;
    cost_finish(g, n, th, aligned4, 4 * 4 * 64 * g.waves, 4 * g.rrow);
    g.nql = nql; g.px = px;
    *out = g;
    return {SM_COST_KERNEL_SAD_PC, n, nql, px, 0};
}

// k_sad_qs: SAD windows 17 .. 21 (two packed sums per shift), up to 240 shifts (8 key bits for the shift)
static inline CostKernelKey sm_plan_sad_qs(const PlanShape &s, int pairs, bool aligned4, SadGeom *out)
{
    const CostKernelKey none = {SM_COST_KERNEL_NONE, 0, 0, 0, 0};
    SadGeom g;
    g.tbl_pad = 0;                          // (the SSD kernel's)
    g.w = s.w; g.h = s.h; g.D = s.D; g.waves = 1;
    const int half = s.square_width / 2, n = 2 * half + 1;
    g.ghost = s.border == SM_GHOST;
    if (n < 17 || n > 21 || g.D > 240 || s.opt.cost_kernel == 1) return none;
    const int nq0 = (g.D + 3 + 3) / 4;
    // the lane shapes the registers of two packed sums per shift allow
    const int nql = nq0 <= 5 ? 5 : nq0 <= 9 ? 9 : 17, px = nq0 <= 5 ? 4 : 2;
    cost_sad_lanes(g, half, nql);
    g.tw = 4 * px * (16 / g.nl);
    g.tiles_x = (g.w + g.tw - 1) / g.tw;
    const int ng = n / 4 + 1;
    // left row: dwords bL .. bL + NG + PX - 1 of the last pixel group; right: up to bR + NQL - 1 + NG + PX - 1 (+1 for the pair)
    g.lrow = 8 * ((g.padl + g.tw + 4 * (ng + 1) + 7) / 8);
    g.rrow = 8 * ((g.padl + g.tw + 4 * (g.nl * nql + ng + 2) + 7) / 8);
    // tile height: whole rounds of two waves per SIMD; rows + warm-up + staging per workgroup
    const CostSearch p = {n, g.w, g.h, pairs, 256 * 4 * 2, 0.45, 160 * 1024 / 8, (size_t)-1, 1.0, false, false, false};
    const CostTile best = cost_tile_search(p, 1, [&](int) { return CostRows{g.lrow, g.rrow, g.tw, 2 * g.rrow}; });
    if (!best.th) return none;
    int th = best.th;
    if (s.opt.cost_tile_h > 0) {         // an explicit tile height, clamped to what a workgroup's LDS holds
        th = s.opt.cost_tile_h;
        while (th > 1 && (size_t)(th + n - 1) * (g.lrow + g.rrow) + 2 * (size_t)g.rrow > 64 * 1024) th--;
    }
    cost_finish(g, n, th, aligned4, 4 * 256, 2 * g.rrow);
    g.nql = nql; g.px = px;
    *out = g;
    return {SM_COST_KERNEL_SAD_QS, n, nql, px, 0};
}

// k_ssd_mfma: SSD on the matrix cores (windows up to 11 x 11, up to 256 shifts)
static inline CostKernelKey sm_plan_ssd_mfma(const PlanShape &s, int pairs, bool aligned4, SadGeom *out)
{
    const CostKernelKey none = {SM_COST_KERNEL_NONE, 0, 0, 0, 0};
    SadGeom g;
    g.w = s.w; g.h = s.h; g.D = s.D; g.waves = 1;
    const int half = s.square_width / 2, n = 2 * half + 1;
    g.ghost = s.border == SM_GHOST;
    if (n < 3 || n > 11 || g.D > 256 || s.opt.cost_kernel == 1) return none;
    const int nb = (g.D + 31 + 31) / 32;                // right positions 0 .. D + 30
    g.nl = 1; g.log2nl = 0; g.nql = 0; g.px = 1; g.q_tail = 0; g.q_last = 0;
    g.padl = 4 * ((half + 3 + 3) / 4);
    const int per_simd = mfma_waves(nb);
    // workgroup width (1, 2 or 4 waves sharing the staged rows) and tile height together: whole rounds of the waves
    // the registers allow per SIMD; rows + warm-up (a warm-up row costs ~0.6 of an output row) + staging per wave
    auto rows = [&](int wv) {
        CostRows r;
        // a lane reads 5 dwords from dword (padl + 32 wave + xl - half) / 4 (+ 8 b in the right row)
        r.lrow = 8 * ((g.padl + 32 * wv + 24 + 7) / 8);
        r.rrow = 8 * ((g.padl + 32 * (nb + wv - 1) + 24 + 7) / 8);
        r.tw = 32 * wv;
        r.tail = wv * (4 * 32 * nb + 16);      // the tables: 32 nb entries per wave, 16-byte aligned behind the staged rows
        return r;
    };
    // (the plan's own choice is between ONE and FOUR waves: two were measured no better than one at equal tile heights and
    // slower at the taller tiles the model gives them -- C5: 0.427 / 0.447 / 0.391 ms at 1 / 2 / 4 waves,
    // profiles/r05/ab_ssd_workgroup_waves.txt -- for a reason that was not found; an explicit 2 is honoured)
    const CostSearch p = {n, g.w, g.h, pairs, 256 * 4 * per_simd, 0.6, (size_t)(160 * 1024 / (4 * per_simd)), 64 * 1024,
                          0.97, true, true, true};
    // an explicit width where it applies; one that does not (not 1, 2 or 4, or wider than the image) is ignored, as
    // k_sad_pc ignores it.  The plan's own choice always finds the one-wave shape (D <= 256: at most ~8 KB of LDS).
    CostTile best = cost_tile_search(p, s.opt.cost_workgroup_waves, rows);
    if (!best.th) best = cost_tile_search(p, 0, rows);
    if (!best.th) return none;
    g.waves = best.wv;
    const CostRows r = rows(g.waves);
    g.lrow = r.lrow; g.rrow = r.rrow; g.tw = r.tw;
    g.tiles_x = (g.w + g.tw - 1) / g.tw;
    int th = best.th;
    if (s.opt.cost_tile_h > 0) {         // an explicit tile height, clamped to what a workgroup's LDS holds
        th = s.opt.cost_tile_h;
        while (th > 1 && (size_t)(th + n - 1) * (g.lrow + g.rrow) + r.tail > 64 * 1024) th--;
    }
    cost_finish(g, n, th, aligned4, 4 * 4 * 64 * g.waves, r.tail);
    // dwords between the end of the staged rows and the table: whatever makes the table 16-byte aligned
    g.tbl_pad = (4 - (g.nsr * ((g.lrow + g.rrow) >> 2)) % 4) % 4;
    *out = g;
    return {SM_COST_KERNEL_SSD_MFMA, n, 0, 0, nb};
}
