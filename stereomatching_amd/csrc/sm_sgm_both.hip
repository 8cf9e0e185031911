// sm_sgm_both.hip -- SGM's left-right check from ONE aggregated volume (include/stereo_hip.h).
//
// PARITY UNPINNED, like all of SGM.  Definition (tests/sgm_single_reference.py is its executable form), S = sm_sgm_wta's
// aggregate of the LEFT pass, d = 0 .. D - 1:
//   left maps   web / best / sub: sm_sgm_wta's, bit for bit;
//   right map   best_right(u, y) = min over the candidates d of S(y, x, d), x = u - d, web_right = 1 + the least d
//               reaching it.  Toroidal: every d, x = (u - d) mod W.  Ghost: only d <= u (S has no column left of 0).
//   check       sm_lr_check's rule between web and this web_right; sub = 0 where it rejected.
// (OpenCV's SGBM and libSGM read their right-reference disparity off the left aggregate in the same way.)  It is another
// right map than sm_sgm_wta_right's: paths and box window belong to the left image only.
//
// Per pair: sm_sgm_volume_pass (sm_sgm.hip: the data term and all directions, the last one as k_sgm_path<K, SGM_MID>, so
// that S is complete in the volume), then
//   k_sgm_both<K, GHOST>  one read of S for the left arg-min, the subpixel fit and the diagonal right arg-min.  A wave owns
//                  a row y and SGB_X = 256 K right pixels u0 .. u0 + SGB_X - 1 and walks t = u0 - (D - 1) .. u0 + SGB_X - 1
//                  (ghost: from max(0, .)), reading column x = t mod W of S: Dp contiguous int32, lane l holding shifts
//                  K l .. K l + K - 1 (the path kernel's layout).  No step's load depends on a result, so SGB_PF loads are in
//                  flight.  Keys S << 8 | d (S <= 8 * 62767 < 2^19); entries d >= D, which hold wrapped sums of the path
//                  kernel's padding value, are replaced by SGB_NONE before any decision.
//                  Right map, a systolic arg-min: slot d carries the running key of right pixel u = t + d over the shifts
//                  above d; per step r[d] = min(r[d + 1], key(x, d)): one move inside the lane and one shift by a lane.
//                  What leaves slot 0 at step t is the finished key of u = t, the least d on ties.  The D - 1 steps
//                  before u0 only feed the chain: (D - 1) / SGB_X extra reads.
//                  Left maps at the steps t >= u0: SGM_LAST's formulas (a wave min, two picks for sub).
//                  Results gather in lane (t - u0) mod 64 and leave as one store of 64 pixels per map.

#include "sm_device.h"

// right pixels per wave, SGB_X: 256 per shift a lane holds, 4 Dp.  The warm-up then re-reads less than a quarter of S at
// every D, and a 1920-wide row is still 8 waves.  (Measured at 128 .. 1024 for each K: profiles/sgm_single/x_sweep.json)
#ifndef SGB_XK
#define SGB_XK 256
#endif
#define SGB_X (SGB_XK * K)
#define SGB_PF 8                  // columns loaded ahead
#define SGB_NONE 0x7fffffff       // the key of no candidate

struct SgmBothGeom {
    int w, h, D, Dp;
    int segs;                     // segments of SGB_X right pixels per row
    long long map;                // element offset of the pair's maps
};

template <int K>
__device__ __forceinline__ void sgb_load(const i32 *p, i32 (&v)[K])
{
    if constexpr (K == 1) {
        v[0] = p[0];
    } else if constexpr (K == 2) {
        const int2 t = *reinterpret_cast<const int2 *>(p);
        v[0] = t.x; v[1] = t.y;
    } else {
        const int4 t = *reinterpret_cast<const int4 *>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
}

// the minimum over the wave (uniform)
__device__ __forceinline__ i32 sgb_wave_min(i32 v)
{
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xf, 0xf, false));     // quad_perm [1, 0, 3, 2]
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xf, 0xf, false));     // quad_perm [2, 3, 0, 1]
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xf, 0xf, false));    // row_half_mirror
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xf, 0xf, false));    // row_mirror
    return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// entry k of lane `lane` (both uniform) of a K-vector
template <int K>
__device__ __forceinline__ i32 sgb_pick(const i32 (&v)[K], int lane, int k)
{
    i32 t = v[0];
#pragma unroll
    for (int j = 1; j < K; j++) t = k == j ? v[j] : t;
    return __builtin_amdgcn_readlane(t, lane);
}

// grid ceil(H * segs / 4), block 256: one segment of one row per wave
template <int K, bool GHOST>
__global__ __launch_bounds__(256) void k_sgm_both(const i32 *__restrict__ S, i32 *__restrict__ web,
                                                  i32 *__restrict__ best, int16_t *__restrict__ sub,
                                                  i32 *__restrict__ web_right, i32 *__restrict__ best_right,
                                                  const SgmBothGeom g)
{
    const int lane = threadIdx.x & 63;
    const int id = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (id >= g.h * g.segs) return;
    const int W = g.w, D = g.D;
    const int y = id / g.segs, u0 = (id - y * g.segs) * SGB_X;
    const int u1 = min(u0 + SGB_X, W);                           // one past the segment's last right pixel
    const int t0 = GHOST ? max(u0 - (D - 1), 0) : u0 - (D - 1);  // the first column of the walk (linear index)
    const int n = u1 - t0, warm = u0 - t0;                       // steps, and those that only feed the chain
    const int dl = lane * K;                                     // this lane's first shift
    const i32 *row = S + (size_t)y * W * g.Dp + dl;
    const size_t orow = (size_t)g.map + (size_t)y * W;

    i32 sr[SGB_PF][K];
    int xl = GHOST ? t0 : smn_mod(t0, W);                        // the column of the next load
    auto load = [&](i32 (&sv)[K]) {
        sgb_load<K>(row + (size_t)xl * g.Dp, sv);
        xl = xl + 1 == W ? 0 : xl + 1;
    };
#pragma unroll
    for (int j = 0; j < SGB_PF; j++)
        if (j < n) load(sr[j]);

    i32 r[K];
#pragma unroll
    for (int k = 0; k < K; k++) r[k] = SGB_NONE;
    i32 o_web = 0, o_best = 0, o_sub = 0, o_wr = 0, o_br = 0;    // of right / left pixel u0 + 64 c + lane
    for (int base = 0; base < n; base += SGB_PF) {
#pragma unroll
        for (int j = 0; j < SGB_PF; j++) {
            const int i = base + j;
            if (i >= n) break;
            i32 sv[K], key[K];
#pragma unroll
            for (int k = 0; k < K; k++) sv[k] = sr[j][k];
            if (i + SGB_PF < n) load(sr[j]);
            // entries d >= D are not costs: never into a decision
#pragma unroll
            for (int k = 0; k < K; k++) key[k] = dl + k < D ? (i32)((u32)sv[k] << 8) | (dl + k) : SGB_NONE;
            i32 hi = __shfl_down(r[0], 1);                        // slot d + 1 of entry K - 1
            if (lane == 63) hi = SGB_NONE;
#pragma unroll
            for (int k = 0; k < K; k++) r[k] = min(k == K - 1 ? hi : r[k + 1], key[k]);
            if (i < warm) continue;
            const int p = i - warm, slot = p & 63;                // pixel u0 + p, right and left
            const i32 fin = __builtin_amdgcn_readlane(r[0], 0);   // d = 0 is always a candidate
            i32 km = key[0];
#pragma unroll
            for (int k = 1; k < K; k++) km = min(km, key[k]);
            km = sgb_wave_min(km);
            const int s = (km & 0xff) + 1;
            const i32 b = km >> 8;
            i32 q16 = 16 * s;
            if (sub && s > 1 && s < D) {
                const i32 sm2 = sgb_pick<K>(sv, (s - 2) / K, (s - 2) % K);
                const i32 sp = sgb_pick<K>(sv, s / K, s % K);
                const i32 a = sm2 - b, c = sp - b, den = a + c;
                int q = 0;
                if (den > 0) q = min(8, max(-8, smn_floordiv(16 * (a - c) + den, 2 * den)));
                q16 = 16 * s + q;
            }
            if (lane == slot) {
                o_web = s; o_best = b; o_sub = q16;
                o_wr = (fin & 0xff) + 1; o_br = fin >> 8;
            }
            if (slot == 63 || i == n - 1) {
                const int u = u0 + (p & ~63) + lane;
                if (u <= u0 + p) {
                    web[orow + u] = o_web;
                    if (best) best[orow + u] = o_best;
                    if (sub) sub[orow + u] = (int16_t)o_sub;
                    web_right[orow + u] = o_wr;
                    if (best_right) best_right[orow + u] = o_br;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

static int sgm_both_launch(const sm_plan *plan, const i32 *S, int Dp, int pair, i32 *web, i32 *best, int16_t *sub,
                           i32 *web_right, i32 *best_right, hipStream_t st)
{
    SgmBothGeom g;
    g.w = plan->width; g.h = plan->height; g.D = plan->num_shifts; g.Dp = Dp;
    g.map = (long long)pair * g.w * g.h;
    const bool ghost = plan->border == SM_GHOST;
    const int K = Dp / 64;
    g.segs = (g.w + SGB_X - 1) / SGB_X;
    const void *fn = Dp == 64 ? (ghost ? (const void *)k_sgm_both<1, true> : (const void *)k_sgm_both<1, false>)
                   : Dp == 128 ? (ghost ? (const void *)k_sgm_both<2, true> : (const void *)k_sgm_both<2, false>)
                               : (ghost ? (const void *)k_sgm_both<4, true> : (const void *)k_sgm_both<4, false>);
    void *args[] = {(void *)&S, (void *)&web, (void *)&best, (void *)&sub, (void *)&web_right, (void *)&best_right,
                    (void *)&g};
    const hipError_t e = hipLaunchKernel(fn, dim3((g.h * g.segs + 3) / 4), dim3(256), args, 0, st);
    if (e != hipSuccess) return sm_fail(SM_ERR_HIP, "launch of k_sgm_both failed: %s", hipGetErrorString(e));
    return SM_OK;
}

// the descriptors of every pair once; then, one pair at a time through the volumes, the full aggregate and its maps
static int sgm_both_pass(sm_plan *plan, const uint8_t *left, const uint8_t *right, int cw, int p1, int p2, int paths,
                         int pairs, i32 *web, i32 *best, int16_t *sub, i32 *web_right, i32 *best_right, hipStream_t st)
{
    SM_TRY(sm_census_descriptors(plan, cw, left, right, pairs, st));
    for (int q = 0; q < pairs; q++) {
        const i32 *S;
        int Dp;
        SM_TRY(sm_sgm_volume_pass(plan, cw, p1, p2, paths, q, &S, &Dp, st));
        SM_TRY(sgm_both_launch(plan, S, Dp, q, web, best, sub, web_right, best_right, st));
    }
    return SM_OK;
}

extern "C" int sm_sgm_wta_both(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width,
                               int p1, int p2, int paths, int pairs, int32_t *d_web, int32_t *d_best, int16_t *d_sub,
                               int32_t *d_web_right, int32_t *d_best_right, void *stream)
{
    const char *me = "sm_sgm_wta_both";
    if (!d_gray_left || !d_gray_right) return sm_fail(SM_ERR_ARG, "%s: input image pointer is NULL", me);
    if (!d_web) return sm_fail(SM_ERR_ARG, "%s: d_web is NULL", me);
    if (!d_web_right) return sm_fail(SM_ERR_ARG, "%s: d_web_right is NULL", me);
    SM_TRY(sm_sgm_args(plan, census_width, p1, p2, paths, pairs, me));
    const size_t map = (size_t)pairs * plan->width * plan->height * sizeof(i32);
    const void *outs[] = {d_web, d_best, d_web_right, d_best_right, d_sub};
    const size_t bytes[] = {map, map, map, map, map / 2};
    for (int a = 0; a < 5; a++)
        for (int b = a + 1; b < 5; b++)
            if (outs[a] && outs[b] && overlap(outs[a], outs[b], bytes[a], bytes[b]))
                return sm_fail(SM_ERR_ARG, "%s: result maps overlap", me);
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    SM_TRY(sm_ws_need(plan, SM_WS_SET_SGM, st, me));
    return sgm_both_pass(plan, d_gray_left, d_gray_right, census_width, p1, p2, paths, pairs, d_web, d_best, d_sub,
                         d_web_right, d_best_right, st);
}

// sm_sgm_lr's checks in sm_sgm_lr's order (sm_entry_lr, sm_entry.h): the first failure is the message
extern "C" int sm_sgm_lr_single(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right,
                                int census_width, int p1, int p2, int paths, int pairs, int max_diff, int32_t *d_web,
                                int32_t *d_best, int32_t *d_web_right, int32_t *d_rejected, int16_t *d_sub,
                                void *stream)
{
    const char *me = "sm_sgm_lr_single";
    if (!d_gray_left || !d_gray_right) return sm_fail(SM_ERR_ARG, "%s: input image pointer is NULL", me);
    if (!d_web) return sm_fail(SM_ERR_ARG, "%s: d_web is NULL", me);
    if (max_diff < 0) return sm_fail(SM_ERR_ARG, "%s: max_diff %d is negative", me, max_diff);
    SM_TRY(sm_sgm_args(plan, census_width, p1, p2, paths, pairs, me));
    SM_TRY(sm_check_lr_maps(plan, pairs, d_web, d_best, d_web_right, d_sub, d_rejected, me));
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    SM_TRY(sm_ws_need(plan, SM_WS_SET_SGM, st, me));
    // the right map in natural order: the caller's, or the plan's mirrored-order map as scratch (as sm_entry_lr)
    i32 *right = d_web_right ? d_web_right : plan->d_web_lr;
    SM_TRY(sgm_both_pass(plan, d_gray_left, d_gray_right, census_width, p1, p2, paths, pairs, d_web, d_best, d_sub, right,
                         nullptr, st));
    SM_TRY(sm_lr_check_launch(plan, false, d_web, right, d_web, nullptr, d_rejected, max_diff, pairs, st));
    return d_sub ? sm_sub_mask_launch(d_web, d_sub, (long long)pairs * plan->width * plan->height, st) : SM_OK;
}
