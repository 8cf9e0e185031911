// sm_unique.hip -- match uniqueness: the runner-up of a census or SGM search, the ratio filter over winner and runner-up
// and the confidence map (include/stereo_hip.h).
//
// PARITY UNPINNED: the reference has no such stage.  Definition (tests/unique_reference.py is its executable form;
// D = the plan's shifts, web = 1 + shift, 0 = invalid):
//   runner-up of a volume V(p, d) against a map web: s = web(p); E(p) = { d in 0 .. D - 1 : |d - (s - 1)| >= 2 } for s
//   in 1 .. D, all of 0 .. D - 1 for any other s.  best2 = min over E(p) of V, web2 = 1 + the first d of E(p) reaching
//   it; E(p) empty: web2 = 0, best2 = -1.
//   sm_census_second: V = sm_census_wta's window cost A_d, the map is the caller's.   k_census_second, sm_census.hip
//   sm_sgm_wta2:      V = SGM's S, the map is the call's own winner.                   k_sgm_path_second, sm_sgm.hip
//   filter:     out = web iff web != 0 and (best2 < 0 or best2 (100 - ratio) >= 100 best), else 0   (64-bit products)
//   confidence: 0 where web = 0; else 255 where best2 < 0; else 0 where best2 <= best; else
//               min(255, floor(255 (best2 - best) / best2)) in 64 bits (best2 = 0 there means best < 0: 255)
//
// The two searches live in their modes' units (a kernel that two units need stays in one: DESIGN.md 9a) and are reached
// through sm_census_second_launch (sm_census.h) and sm_sgm_second_pass (sm_internal.h); this unit holds the four entry
// points and the two element-wise kernels:
//   k_unique_filter   grid (up to SM_LR_BLOCKS, pairs), block 256, striding over the pair's pixels; the rejections are
//                     counted as the check counts them (lr_count: one atomic per workgroup).  out may be web: a lane
//                     reads a pixel before it writes it and touches no other.
//   k_confidence      the same grid, one byte per pixel out.

#include "sm_device.h"
#include "sm_census.h"

typedef long long i64;

__global__ __launch_bounds__(256) void k_unique_filter(const i32 *web, const i32 *__restrict__ best,
                                                       const i32 *__restrict__ best2, i32 *out, i32 *rejected,
                                                       unsigned npx, int ratio)
{
    const size_t base = (size_t)blockIdx.y * npx;
    int cnt = 0;
    for (unsigned t = blockIdx.x * 256u + threadIdx.x; t < npx; t += gridDim.x * 256u) {
        const i32 s = web[base + t];
        const i64 b = best[base + t], b2 = best2[base + t];
        const bool keep = s != 0 && (b2 < 0 || b2 * (100 - ratio) >= b * 100);
        cnt += s != 0 && !keep;
        out[base + t] = keep ? s : 0;
    }
    if (rejected) lr_count(rejected + blockIdx.y, cnt);
}

__global__ __launch_bounds__(256) void k_confidence(const i32 *__restrict__ web, const i32 *__restrict__ best,
                                                    const i32 *__restrict__ best2, u8 *__restrict__ conf, unsigned npx)
{
    const size_t base = (size_t)blockIdx.y * npx;
    for (unsigned t = blockIdx.x * 256u + threadIdx.x; t < npx; t += gridDim.x * 256u) {
        const i32 s = web[base + t], b = best[base + t], b2 = best2[base + t];
        u32 c;
        if (s == 0) c = 0;
        else if (b2 < 0) c = 255;
        else if (b2 <= b) c = 0;
        else if (b < 0) c = 255;                      // (b2 - b) / b2 > 1, and b2 = 0 never divides
        else {
            // 0 <= b < b2: the quotient is below 255.  Costs are far below 2^23 (A <= 30000, S < 2^19), where the
            // numerator fits 32 bits and the division is the short one; any int32 is still exact
            const unsigned long long num = 255ull * (u32)(b2 - b);
            c = num <= 0xffffffffull ? (u32)num / (u32)b2 : (u32)(num / (u32)b2);
        }
        conf[base + t] = (u8)c;
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

// an output of `ob` bytes against both input images of `pairs` pairs
static bool on_an_image(const sm_plan *plan, int pairs, const void *o, size_t ob, const uint8_t *left, const uint8_t *right)
{
    const size_t px = (size_t)pairs * plan->width * plan->height;
    return o && (overlap(o, left, ob, px) || overlap(o, right, ob, px));
}

extern "C" int sm_census_second(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width,
                                int pairs, const int32_t *d_web, int32_t *d_web2, int32_t *d_best2, void *stream)
{
    const char *me = "sm_census_second";
    if (!d_gray_left || !d_gray_right) return sm_fail(SM_ERR_ARG, "%s: input image pointer is NULL", me);
    if (!d_web) return sm_fail(SM_ERR_ARG, "%s: d_web is NULL", me);
    if (!d_web2) return sm_fail(SM_ERR_ARG, "%s: d_web2 is NULL", me);
    SM_TRY(sm_census_args(plan, census_width, pairs, me));
    const size_t map = (size_t)pairs * plan->width * plan->height * sizeof(i32);
    if (d_best2 && overlap(d_web2, d_best2, map)) return sm_fail(SM_ERR_ARG, "%s: d_web2 and d_best2 overlap", me);
    if (on_an_image(plan, pairs, d_web2, map, d_gray_left, d_gray_right) ||
        on_an_image(plan, pairs, d_best2, map, d_gray_left, d_gray_right))
        return sm_fail(SM_ERR_ARG, "%s: an output overlaps an input image", me);
    if (overlap(d_web2, d_web, map) || (d_best2 && overlap(d_best2, d_web, map)))
        return sm_fail(SM_ERR_ARG, "%s: an output overlaps the input map", me);
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    SM_TRY(sm_ws_need(plan, SM_WS_SET_CENSUS, st, me));
    SM_TRY(sm_census_descriptors(plan, census_width, d_gray_left, d_gray_right, pairs, st));
    return sm_census_second_launch(plan, census_width, pairs, d_web, d_web2, d_best2, st);
}

extern "C" int sm_sgm_wta2(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width,
                           int p1, int p2, int paths, int pairs, int32_t *d_web, int32_t *d_best, int16_t *d_sub,
                           int32_t *d_web2, int32_t *d_best2, void *stream)
{
    const char *me = "sm_sgm_wta2";
    if (!d_gray_left || !d_gray_right) return sm_fail(SM_ERR_ARG, "%s: input image pointer is NULL", me);
    if (!d_web) return sm_fail(SM_ERR_ARG, "%s: d_web is NULL", me);
    if (!d_web2) return sm_fail(SM_ERR_ARG, "%s: d_web2 is NULL", me);
    SM_TRY(sm_sgm_args(plan, census_width, p1, p2, paths, pairs, me));
    const size_t map = (size_t)pairs * plan->width * plan->height * sizeof(i32);
    const void *outs[] = {d_web, d_best, d_web2, d_best2, d_sub};
    const size_t bytes[] = {map, map, map, map, map / 2};
    for (int a = 0; a < 5; a++)
        for (int b = a + 1; b < 5; b++)
            if (outs[a] && outs[b] && overlap(outs[a], outs[b], bytes[a], bytes[b]))
                return sm_fail(SM_ERR_ARG, "%s: result maps overlap", me);
    for (int a = 0; a < 5; a++)
        if (on_an_image(plan, pairs, outs[a], bytes[a], d_gray_left, d_gray_right))
            return sm_fail(SM_ERR_ARG, "%s: an output overlaps an input image", me);
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    SM_TRY(sm_ws_need(plan, SM_WS_SET_SGM, st, me));
    SM_TRY(sm_census_descriptors(plan, census_width, d_gray_left, d_gray_right, pairs, st));
    return sm_sgm_second_pass(plan, census_width, p1, p2, paths, pairs, d_web, d_best, d_sub, d_web2, d_best2, st);
}

extern "C" int sm_uniqueness_filter(sm_plan *plan, const int32_t *d_web, const int32_t *d_best, const int32_t *d_best2,
                                    int ratio, int pairs, int32_t *d_out, int32_t *d_rejected, void *stream)
{
    const char *me = "sm_uniqueness_filter";
    if (!d_web || !d_best || !d_best2 || !d_out) return sm_fail(SM_ERR_ARG, "%s: a map pointer is NULL", me);
    if (ratio < 0 || ratio > 100) return sm_fail(SM_ERR_ARG, "%s: ratio %d outside 0..100", me, ratio);
    SM_TRY(sm_check_pairs(plan, pairs, me));
    const size_t map = (size_t)pairs * plan->width * plan->height * sizeof(i32);
    if ((d_out != d_web && overlap(d_out, d_web, map)) || overlap(d_out, d_best, map) || overlap(d_out, d_best2, map))
        return sm_fail(SM_ERR_ARG, "%s: maps overlap without d_out being d_web", me);
    const size_t counts = (size_t)pairs * sizeof(i32);
    if (d_rejected && (overlap(d_rejected, d_web, counts, map) || overlap(d_rejected, d_best, counts, map) ||
                       overlap(d_rejected, d_best2, counts, map) || overlap(d_rejected, d_out, counts, map)))
        return sm_fail(SM_ERR_ARG, "%s: d_rejected overlaps a map", me);
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    if (d_rejected) SM_TRY(sm_lr_zero_counts(d_rejected, pairs, st));
    const unsigned npx = (unsigned)plan->width * plan->height;
    hipLaunchKernelGGL(k_unique_filter, dim3(std::min((npx + 255) / 256, (unsigned)SM_LR_BLOCKS), pairs), dim3(256), 0, st,
                       d_web, d_best, d_best2, d_out, d_rejected, npx, ratio);
    SM_LAUNCH_CHECK("k_unique_filter");
    return SM_OK;
}

extern "C" int sm_confidence(sm_plan *plan, const int32_t *d_web, const int32_t *d_best, const int32_t *d_best2, int pairs,
                             uint8_t *d_conf, void *stream)
{
    const char *me = "sm_confidence";
    if (!d_web || !d_best || !d_best2 || !d_conf) return sm_fail(SM_ERR_ARG, "%s: a map pointer is NULL", me);
    SM_TRY(sm_check_pairs(plan, pairs, me));
    const size_t map = (size_t)pairs * plan->width * plan->height * sizeof(i32);
    if (overlap(d_conf, d_web, map / 4, map) || overlap(d_conf, d_best, map / 4, map) ||
        overlap(d_conf, d_best2, map / 4, map))
        return sm_fail(SM_ERR_ARG, "%s: d_conf overlaps a map", me);
    SM_TRY(sm_use_device(plan->device));
    const unsigned npx = (unsigned)plan->width * plan->height;
    hipLaunchKernelGGL(k_confidence, dim3(std::min((npx + 255) / 256, (unsigned)SM_LR_BLOCKS), pairs), dim3(256), 0,
                       (hipStream_t)stream, d_web, d_best, d_best2, d_conf, npx);
    SM_LAUNCH_CHECK("k_confidence");
    return SM_OK;
}
