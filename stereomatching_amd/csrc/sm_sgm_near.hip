// sm_sgm_near.hip -- banded SGM: semi-global aggregation of the census data term over the shifts within `radius` of a
// prior map (include/stereo_hip.h): the fine step of the half-resolution path with SGM's smoothness
// term, at a volume that does not grow with D.  It uses the census mode's descriptors (sm_census.h; the workspace is
// filled by sm_census_descriptors) and one workspace row of its own, SM_WS_SGM_NEAR; the full SGM volumes are never
// touched.
//
// PARITY UNPINNED.  Definition (tests/sgm_near_reference.py is its executable form; r = radius, prior a web map):
//   K(p)      = { d : 0 <= d <= D - 1, |d - (prior(p) - 1)| <= r }, empty for prior(p) = 0
//   A(p, d)   = sm_census_wta's window cost, d in K(p)
//   L_r(p, d) = A(p, d) where q = p - r lies outside the image or K(q) is empty (the path restarts), else
//               A(p, d) + min(L_r(q, d), L_r(q, d -+ 1) + P1, m_q + P2) - m_q,  m_q = min over K(q) of L_r(q, k);
//               terms whose shift is not in K(q) dropped.  A <= L_r <= A + P2 <= 62767.
//   S(p, d)   = sum of L_r over the 4 or 8 directions of sm_sgm_wta; best = min over K(p) of S, web = 1 + the least d
//               reaching it; sub = sm_sgm_wta's parabola on S(d - 1), S(d), S(d + 1) where both neighbours are in K(p),
//               else 16 web.  K(p) empty: web = best = sub = 0.
//
// Volumes (SM_WS_SGM_NEAR, one pair at a time): A_b [H][W][16] u16 and S_b [H][W][16] i32, 96 W H bytes, slot innermost.
// Slot k of pixel p is shift prior(p) - 2 - r + k: the band sits in slots 1 .. 2r + 1 (at most 9), with a guard slot on
// either side of it, so that L(q, d - 1) and L(q, d + 1) are the row neighbours of the ONE fetched value L(q, d)
// (below).  Slots outside K(p) are never written by the data term and never read as costs: every kernel derives a
// slot's validity from the prior itself.  The volumes are in the pass's columns (the right-reference pass: mirrored),
// the prior and the maps in natural ones.
//
// Kernels:
//   k_sgm_near_cost<NW, GHOST, MIRROR>  the data term: the tile walk that k_census_near makes, one text for both
//                  (sm_near_tile_body.h): a 64 x 16 tile's positions in registers, the OR of the wanted shifts in LDS,
//                  a uniform walk of its set bits, row sums then column sums through LDS, the next shift's loads in
//                  flight meanwhile.  Here a pixel stores A to its slot of the shift.
//   k_sgm_near_path<MODE>  one direction.  A DPP row of 16 lanes owns a line, lane = slot: four lines per wave, 16 per
//                  workgroup (a horizontal direction is bound by the latency of its chain, not by lanes).
//                  Step p: b_p - b_q slots lie between the two bands, so L(q, d) is one ds_bpermute within the row
//                  (SGN_INF outside the row or outside K(q)), L(q, d -+ 1) its row_shr:1 / row_shl:1, m_q four DPP min
//                  steps.  FIRST / MID / LAST as in sm_sgm.hip: LAST emits web / best / sub from registers.  The data
//                  term, S and the prior of step i + SGN_PF are loaded while step i is computed, by every lane and
//                  under no branch that differs between the rows (see the loop).

#include "sm_device.h"
#include "sm_census.h"

typedef unsigned short u16;

#define SGN_NS 16                 // slots per pixel: guard, 2r + 1 <= 9 shifts, guard, padding to a DPP row
#define SGN_INF 0x3fffffff        // L of a slot outside K: never a minimum, + P2 cannot wrap
#define SGN_PF 12                 // path kernel: steps loaded ahead

struct SgmNearCostGeom : NearTileGeom {
    long long pair;               // pixels from the first pair's to this pair's (descriptors, prior)
};

template <int NW, bool GHOST, bool MIRROR>
__global__ __launch_bounds__(256) void k_sgm_near_cost(const u32 *__restrict__ desc, const i32 *__restrict__ prior,
                                                       u16 *__restrict__ A, const SgmNearCostGeom g)
{
#define SMN_TILE_PAIR ((size_t)g.pair)
#define SMN_TILE_STATE int b0[4];                          // the shift of the pixel's slot 0
#define SMN_TILE_NONE(j) b0[j] = 0;
#define SMN_TILE_BAND(j, s) b0[j] = (s) - 2 - g.radius;
// the pixel's slots in A_b (a pixel outside the image has no band and stores nothing: clamped)
#define SMN_TILE_SETUP                                                          \
    u16 *out[4];                                                                \
    _Pragma("unroll") for (int j = 0; j < 4; j++) {                             \
        const int y = min(y0 + 4 * ly + j, H - 1);                              \
        out[j] = A + ((size_t)y * W + min(x, W - 1)) * SGN_NS;                  \
    }
// (d - b0 is in 1 .. 2r + 1)
#define SMN_TILE_TAKE(j, d, a) out[j][(d) - b0[j]] = (u16)(a);
#include "sm_near_tile_body.h"
#undef SMN_TILE_PAIR
#undef SMN_TILE_STATE
#undef SMN_TILE_NONE
#undef SMN_TILE_BAND
#undef SMN_TILE_SETUP
#undef SMN_TILE_TAKE
}

struct SgmNearPathGeom {
    int w, h, D;
    int radius;
    int p1, p2;
    int dx, dy;                   // the direction r
    int lines;
    int mirror;                   // the pass is the right-reference one: volume column x is natural W - 1 - x
    long long map;                // element offset of the pair's prior and maps
};

enum { SGN_FIRST = 0, SGN_MID = 1, SGN_LAST = 2 };

// the minimum over a DPP row of 16 lanes, in every lane of it
__device__ __forceinline__ i32 sgn_row_min(i32 v)
{
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xf, 0xf, false));     // quad_perm [1, 0, 3, 2]
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xf, 0xf, false));     // quad_perm [2, 3, 0, 1]
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xf, 0xf, false));    // row_half_mirror
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xf, 0xf, false));    // row_mirror
    return v;
}
// the value of the lane below / above in the row; `edge` in the row's first / last lane
__device__ __forceinline__ i32 sgn_from_below(i32 v, i32 edge)
{
    return __builtin_amdgcn_update_dpp(edge, v, 0x111, 0xf, 0xf, false);      // row_shr:1
}
__device__ __forceinline__ i32 sgn_from_above(i32 v, i32 edge)
{
    return __builtin_amdgcn_update_dpp(edge, v, 0x101, 0xf, 0xf, false);      // row_shl:1
}

// grid ceil(lines / 16), block 256: one line per row of 16 lanes
template <int MODE>
__global__ __launch_bounds__(256) void k_sgm_near_path(const u16 *__restrict__ A, i32 *__restrict__ S,
                                                       const i32 *__restrict__ prior, i32 *web, i32 *best,
                                                       int16_t *sub, const SgmNearPathGeom g)
{
    const int l = threadIdx.x & 15;                              // slot
    const int rowbase = threadIdx.x & 48;                        // first lane of the row in its wave
    const int line = blockIdx.x * 16 + (threadIdx.x >> 4);
    const int W = g.w, H = g.h, D = g.D, R = g.radius;
    // the line's first pixel: its predecessor lies outside the image (a row past the last line: no steps)
    int x0 = 0, y0 = 0, len = 0;
    if (line < g.lines) {
        if (g.dy == 0) {
            y0 = line; x0 = g.dx > 0 ? 0 : W - 1;
        } else if (g.dx == 0) {
            x0 = line; y0 = g.dy > 0 ? 0 : H - 1;
        } else if (line < W) {
            x0 = line; y0 = g.dy > 0 ? 0 : H - 1;
        } else {
            const int j = line - W + 1;
            x0 = g.dx > 0 ? 0 : W - 1; y0 = g.dy > 0 ? j : H - 1 - j;
        }
        const int lx = g.dx > 0 ? W - x0 : g.dx < 0 ? x0 + 1 : 0x7fffffff;
        const int ly = g.dy > 0 ? H - y0 : g.dy < 0 ? y0 + 1 : 0x7fffffff;
        len = min(lx, ly);
    }
    const long long pstep = (long long)g.dy * W + g.dx;          // pixels per step in the volumes
    const long long p0 = (long long)y0 * W + x0;
    const u16 *a0 = A + (size_t)p0 * SGN_NS + l;
    i32 *s0 = S + (size_t)p0 * SGN_NS + l;
    const long long vstep = pstep * SGN_NS;
    // the prior and the maps are in natural columns
    const long long mstep = (long long)g.dy * W + (g.mirror ? -g.dx : g.dx);
    const long long m0 = g.map + (long long)y0 * W + (g.mirror ? W - 1 - x0 : x0);

    // The loop's trip count is the longest line of the wave and every load is issued by every lane, at a step clamped
    // to its own line (a row without a line reads pixel 0): with a branch that differs between the rows around them the
    // loads are waited for where they are issued, and every step pays a trip to memory.  `act`: this row's line has a
    // step i; what a row computes past its end is never stored.
    const int lenw = max(max(__builtin_amdgcn_readlane(len, 0), __builtin_amdgcn_readlane(len, 16)),
                         max(__builtin_amdgcn_readlane(len, 32), __builtin_amdgcn_readlane(len, 48)));
    const int last = max(len - 1, 0);
    i32 ar[SGN_PF], sr[SGN_PF], pr[SGN_PF];
    auto load = [&](int i, i32 &av, i32 &sv, i32 &pv) {
        i = min(i, last);
        av = a0[i * vstep];
        if (MODE != SGN_FIRST) sv = s0[i * vstep];
        else sv = 0;
        pv = prior[m0 + i * mstep];
    };
#pragma unroll
    for (int j = 0; j < SGN_PF; j++) load(j, ar[j], sr[j], pr[j]);

    i32 L = SGN_INF, m = SGN_INF;                                // of the previous pixel q: no band yet
    int bq = 0;
    const i32 P1 = g.p1, P2 = g.p2;
    for (int base = 0; base < lenw; base += SGN_PF) {
#pragma unroll
        for (int j = 0; j < SGN_PF; j++) {
            const int i = base + j;                              // (past lenw in the last turn: no row is active)
            const bool act = i < len;
            const i32 av = ar[j], sv = sr[j], s = pr[j];
            load(i + SGN_PF, ar[j], sr[j], pr[j]);
            // (s compared before any arithmetic on it: INT32_MIN and INT32_MAX are legal)
            const bool has = s != 0 && s >= 1 - R && s <= D + R;
            const int b = has ? s - 2 - R : 0;                   // the shift of slot 0
            const int d = b + l;
            const bool valid = has && l >= 1 && l <= 2 * R + 1 && d >= 0 && d < D;
            // L(q, d): b - bq slots further up q's row.  q without a band (or outside the image): L = m = SGN_INF in
            // every lane, every fetched value is SGN_INF as well and t below is SGN_INF - SGN_INF = 0: L = A, the path
            // restarts without a branch
            const int idx = l + (b - bq);
            i32 Ld = __builtin_amdgcn_ds_bpermute((rowbase + (idx & 15)) << 2, L);
            if ((unsigned)idx > 15u) Ld = SGN_INF;
            const i32 dm = sgn_from_below(Ld, SGN_INF), dp = sgn_from_above(Ld, SGN_INF);
            const i32 t = min(min(Ld, min(dm, dp) + P1), m + P2) - m;
            L = valid ? av + t : SGN_INF;
            m = sgn_row_min(L);
            bq = b;

            if (MODE == SGN_FIRST) {
                if (act) s0[i * vstep] = L;
            } else if (MODE == SGN_MID) {
                if (act) s0[i * vstep] = valid ? sv + L : SGN_INF;
            } else {
                // S <= 8 * 62767 < 2^19: keys S << 8 | slot; the least slot (the least d) wins a tie
                const i32 tot = valid ? sv + L : 0;
                const i32 key = sgn_row_min(valid ? (tot << 8) | l : 0x7fffffff);
                const int slot = key & 0xff;
                const i32 bst = key >> 8;
                const i32 tm = sgn_from_below(tot, 0), tp = sgn_from_above(tot, 0);
                const i32 vm = sgn_from_below((i32)valid, 0), vp = sgn_from_above((i32)valid, 0);
                if (act && (has ? l == slot : l == 0)) {
                    const size_t o = (size_t)(m0 + i * mstep);
                    const int sw = has ? d + 1 : 0;
                    int q = 0;
                    if (sub && has && vm && vp) {
                        const i32 a = tm - bst, c = tp - bst, den = a + c;
                        if (den > 0) q = min(8, max(-8, smn_floordiv(16 * (a - c) + den, 2 * den)));
                    }
                    web[o] = sw;
                    if (best) best[o] = has ? bst : 0;
                    if (sub) sub[o] = (int16_t)(16 * sw + q);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

// one pair's banded volumes: 16 slots of u16 and of i32 a pixel, whatever the call's radius
size_t sm_sgm_near_volume_bytes(const sm_plan *plan)
{
    return (size_t)6 * SGN_NS * plan->width * plan->height;
}

extern "C" int sm_plan_reserve_sgm_near(sm_plan *plan)
{
    if (!plan) return sm_fail(SM_ERR_ARG, "sm_plan_reserve_sgm_near: plan is NULL");
    SM_TRY(sm_use_device(plan->device));
    return sm_ws_reserve(plan, SM_WS_SET_SGM_NEAR, "sm_plan_reserve_sgm_near");
}

static u16 *sgn_volume_a(const sm_plan *plan) { return (u16 *)plan->d_sgm_near; }
static i32 *sgn_volume_s(const sm_plan *plan)
{
    return (i32 *)((char *)plan->d_sgm_near + (size_t)2 * SGN_NS * plan->width * plan->height);
}

// the data term of one pair into A_b
static int sgn_cost_launch(const sm_plan *plan, int cw, bool mirror, int pair, const i32 *d_prior, int radius,
                           hipStream_t st)
{
    SgmNearCostGeom g;
    size_t lds;
    SM_TRY(sm_near_tile_geom(plan, radius, "sgm near", &g, &lds));
    g.pair = (long long)pair * g.w * g.h;
    const bool ghost = plan->border == SM_GHOST;
    const void *fn = cw == 7 ? SM_PASS_KERNEL(k_sgm_near_cost, 2, ghost, mirror)
                             : SM_PASS_KERNEL(k_sgm_near_cost, 1, ghost, mirror);
    u16 *A = sgn_volume_a(plan);
    void *args[] = {(void *)&plan->d_census, (void *)&d_prior, (void *)&A, (void *)&g};
    const hipError_t e = hipLaunchKernel(fn, dim3(g.tiles_x, g.tiles_y), dim3(256), args, lds, st);
    if (e != hipSuccess) return sm_fail(SM_ERR_HIP, "launch of k_sgm_near_cost failed: %s", hipGetErrorString(e));
    return SM_OK;
}

// the directions in sm_sgm.hip's stream order; the last one emits the maps
static int sgn_paths_launch(const sm_plan *plan, int p1, int p2, int paths, bool mirror, int pair, const i32 *d_prior,
                            int radius, i32 *web, i32 *best, int16_t *sub, hipStream_t st)
{
    SgmNearPathGeom g;
    g.w = plan->width; g.h = plan->height; g.D = plan->num_shifts;
    g.radius = radius;
    g.p1 = p1; g.p2 = p2;
    g.mirror = mirror;
    g.map = (long long)pair * g.w * g.h;
    const u16 *A = sgn_volume_a(plan);
    i32 *S = sgn_volume_s(plan);
    for (int r = 0; r < paths; r++) {
        sm_sgm_direction(paths, r, g.w, g.h, &g.dx, &g.dy, &g.lines);
        const void *fn = r == 0 ? (const void *)k_sgm_near_path<SGN_FIRST>
                       : r == paths - 1 ? (const void *)k_sgm_near_path<SGN_LAST> : (const void *)k_sgm_near_path<SGN_MID>;
        void *args[] = {(void *)&A, (void *)&S, (void *)&d_prior, (void *)&web, (void *)&best, (void *)&sub, (void *)&g};
        const hipError_t e = hipLaunchKernel(fn, dim3((g.lines + 15) / 16), dim3(256), args, 0, st);
        if (e != hipSuccess) return sm_fail(SM_ERR_HIP, "launch of k_sgm_near_path failed: %s", hipGetErrorString(e));
    }
    return SM_OK;
}

// the mode as the entry driver sees it (sm_entry.h): the guided re-search's inputs and overlap rules
// with SGM's scalars
struct SgmNearMode : sm_mode, NearPriors {
    using NearPriors::inputs;
    static constexpr const sm_ws_set &ws = SM_WS_SET_SGM_NEAR;
    int cw, p1, p2, paths;
    const int16_t *sub;                 // the call's d_sub (NULL: none): an output like the maps the driver hands to apart
    SgmNearMode(int census_width, int p1_, int p2_, int paths_, int radius_, const i32 *p, const i32 *p_right,
                const int16_t *d_sub)
        : NearPriors{radius_, p, p_right}, cw(census_width), p1(p1_), p2(p2_), paths(paths_), sub(d_sub) {}
    // SGM's plan-free checks (sm_sgm_scalar_args: the one copy of their messages) and the radius, then the census
    // mode's, whose reach of 512 shifts stands in place of SGM's 256 (nothing here grows with D)
    int args(const sm_call &c) const
    {
        SM_TRY(sm_sgm_scalar_args(cw, p1, p2, paths, c.me));
        SM_TRY(radius_arg(c.me));
        return sm_census_args(c.plan, cw, c.pairs, c.me);
    }
    // the int16 subpixel map as well, which the driver compares with the other maps only
    int apart(const sm_call &c, const i32 *const *outs, int n_outs, const i32 *rejected) const
    {
        return NearPriors::apart(c, outs, n_outs, rejected, sub,
                                 (size_t)c.pairs * c.plan->width * c.plan->height * sizeof(int16_t));
    }
    int prepare(const sm_call &c) const { return sm_census_descriptors(c.plan, cw, c.left, c.right, c.pairs, c.st); }
    // one pair at a time through the volumes
    int pass(const sm_call &c, bool mirror, i32 *web, i32 *best, int16_t *sub) const
    {
        const i32 *p = mirror ? prior_right : prior;
        for (int q = 0; q < c.pairs; q++) {
            SM_TRY(sgn_cost_launch(c.plan, cw, mirror, q, p, radius, c.st));
            SM_TRY(sgn_paths_launch(c.plan, p1, p2, paths, mirror, q, p, radius, web, best, sub, c.st));
        }
        return SM_OK;
    }
};

extern "C" int sm_sgm_wta_near(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right,
                               int census_width, int p1, int p2, int paths, int pairs, const int32_t *d_prior,
                               int radius, int32_t *d_web, int32_t *d_best, int16_t *d_sub, void *stream)
{
    return sm_entry_one({"sm_sgm_wta_near", plan, d_gray_left, d_gray_right, pairs, (hipStream_t)stream},
                        SgmNearMode(census_width, p1, p2, paths, radius, d_prior, nullptr, d_sub), false, d_web, d_best,
                        d_sub);
}

extern "C" int sm_sgm_wta_near_right(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right,
                                     int census_width, int p1, int p2, int paths, int pairs,
                                     const int32_t *d_prior_right, int radius, int32_t *d_web_right,
                                     int32_t *d_best_right, void *stream)
{
    return sm_entry_one({"sm_sgm_wta_near_right", plan, d_gray_left, d_gray_right, pairs, (hipStream_t)stream},
                        SgmNearMode(census_width, p1, p2, paths, radius, nullptr, d_prior_right, nullptr), true, d_web_right,
                        d_best_right, nullptr);
}

extern "C" int sm_sgm_near_lr(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right,
                              int census_width, int p1, int p2, int paths, int pairs, const int32_t *d_prior,
                              const int32_t *d_prior_right, int radius, int max_diff, int32_t *d_web, int32_t *d_best,
                              int32_t *d_web_right, int32_t *d_rejected, int16_t *d_sub, void *stream)
{
    return sm_entry_lr({"sm_sgm_near_lr", plan, d_gray_left, d_gray_right, pairs, (hipStream_t)stream},
                       SgmNearMode(census_width, p1, p2, paths, radius, d_prior, d_prior_right, d_sub), max_diff, d_web,
                       d_best, d_web_right, d_rejected, d_sub);
}
