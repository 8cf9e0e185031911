// sm_wmedian.hip -- guided weighted median (include/stereo_hip.h "guided weighted median"): the
// edge-aware refinement of a disparity map between the speckle filter and the interpolation.  The only post-filter
// that looks at the image: a tap counts with a weight taken from how close the guide's gray value there is to the
// guide's gray value at the centre, so the median is taken among the pixels of the centre's own surface.
//
// PARITY UNPINNED: the reference has no such stage.  Definition (tests/wmedian_reference.py is its executable form).
// Maps, validity and borders as for the post-filters (sm_filter.hip); the guide g is u8 [pairs][H][W]; radius r in
// 1 .. 7; weights: 256 uint16 on the host, weights[0] >= 1.
//   taps of p: the pixels q of the (2r + 1)^2 window around p that lie in the image and have in(q) != 0, each with
//     w_q = weights[|g(p) - g(q)|]; T = the sum of the w_q (at most 225 * 65535).
//   wmed(p) = the smallest tap value v (signed order) with 2 * sum{w_q : in(q) <= v} >= T: the lower weighted median.
//   flags = 0:            out(p) = 0 where in(p) = 0, else wmed(p)
//   flags = SM_WMED_FILL: where in(p) = 0, out(p) = wmed(p) if T >= fill_min_weight, else 0 (taps are read from the
//     input: a filled pixel is no source); filled = the pixels that were 0 and are no longer, per pair.
//
// Kernel:
//   k_wmedian<T, R>  k_median's layout: a 64 x 16 tile, 256 lanes, the halo of R staged in LDS, values as int32 (0 for
//                    a tap outside the image: a missing tap and an invalid one are treated alike) and the guide as
//                    bytes; a lane owns a column of the tile and four of its rows.  The weight table travels by value
//                    in the kernel's arguments (512 bytes: no copy to the device, so the call can be captured from
//                    pageable memory, and a graph holds the table of capture time) and is staged into LDS once per
//                    workgroup.  The rank costs no sort: one pass over the window gives T and the least and greatest
//                    tap value, then the integer interval between them is bisected for the smallest x with
//                    2 * cum(<= x) >= T.  cum only steps at tap values, so that x is one: exact for any int32 values,
//                    in at most 32 passes (log2 of the window's value range: 7 for 128 shifts, 11 for a subpixel map
//                    of 2048 steps).  The midpoint is taken on the unsigned difference: hi - lo can be 2^32 - 2.
//                    R <= 3: the window's values and weights stay in registers over the passes; above, every pass
//                    reads the tile again (value, guide byte, weight) row by row, the rows NOT unrolled -- unrolled,
//                    the compiler keeps the first pass's loads alive over the bisection (256 registers at R = 5, one
//                    wave per SIMD), and 225 taps do not fit a lane's registers at all.
//                    Filled pixels are counted as the other stages count (lr_count: one atomic per workgroup).

#include "sm_device.h"

#define WMED_MAX_R 7
#define WMED_REG_R 3       // up to this radius a lane keeps its window in registers (49 values, 49 weights)

// the smallest x in lo .. hi with 2 * cum(x) >= total, where cum(hi) = total (so one exists)
template <typename Cum>
__device__ __forceinline__ i32 wmed_bisect(i32 lo, i32 hi, u32 total, Cum cum)
{
    while (lo < hi) {
        const i32 mid = (i32)((u32)lo + (((u32)hi - (u32)lo) >> 1));      // lo <= mid < hi
        if (2u * cum(mid) >= total) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// grid (ceil(W / 64), ceil(H / 16), pairs), block 256.  fill_min: 0 = invalid pixels stay 0; else the least T that
// fills one.  filled: NULL or the pairs' counts, zeroed before the launch.
template <typename T, int R>
__global__ __launch_bounds__(256) void k_wmedian(const T *__restrict__ in, const u8 *__restrict__ guide, WmedTable table,
                                                 T *__restrict__ out, i32 *filled, int W, int H, u32 fill_min)
{
    constexpr int K = 2 * R + 1, SW = FLT_TW + 2 * R, SH = FLT_TH + 2 * R, N = K * K;
    constexpr bool IN_REGS = R <= WMED_REG_R;
    __shared__ i32 tile[SH * SW];
    __shared__ u8 gray[SH * SW];
    __shared__ uint16_t wt[256];
    const int tx0 = blockIdx.x * FLT_TW, ty0 = blockIdx.y * FLT_TH;
    const size_t base = (size_t)blockIdx.z * W * H;
    wt[threadIdx.x] = table.w[threadIdx.x];
    for (int i = threadIdx.x; i < SH * SW; i += 256) {
        const int sy = i / SW, sx = i - sy * SW;
        const int gx = tx0 + sx - R, gy = ty0 + sy - R;
        const bool inside = gx >= 0 && gx < W && gy >= 0 && gy < H;
        tile[i] = inside ? (i32)in[base + (size_t)gy * W + gx] : 0;
        gray[i] = inside ? guide[base + (size_t)gy * W + gx] : (u8)0;
    }
    __syncthreads();
    const int lx = threadIdx.x & 63, gx = tx0 + lx;
    int cnt = 0;
    for (int ly = threadIdx.x >> 6; ly < FLT_TH; ly += 4) {
        const int gy = ty0 + ly;
        if (gx >= W || gy >= H) continue;
        const i32 c = tile[(ly + R) * SW + lx + R];
        i32 res = 0;
        if (c != 0 || fill_min) {
            const int gc = gray[(ly + R) * SW + lx + R];
            u32 total = 0;
            i32 lo = 0x7fffffff, hi = (i32)0x80000000;
            if constexpr (IN_REGS) {
                i32 v[N];
                u32 w[N];
#pragma unroll
                for (int dy = 0; dy < K; dy++)
#pragma unroll
                    for (int dx = 0; dx < K; dx++) {
                        const int s = (ly + dy) * SW + lx + dx, j = dy * K + dx;
                        v[j] = tile[s];
                        w[j] = v[j] != 0 ? wt[abs(gc - (int)gray[s])] : 0u;
                        total += w[j];
                        lo = v[j] != 0 && v[j] < lo ? v[j] : lo;
                        hi = v[j] != 0 && v[j] > hi ? v[j] : hi;
                    }
                // (an invalid tap has weight 0: its value 0 may be counted at will)
                if (total) res = wmed_bisect(lo, hi, total, [&](i32 x) {
                    u32 cum = 0;
#pragma unroll
                    for (int j = 0; j < N; j++) cum += v[j] <= x ? w[j] : 0u;
                    return cum;
                });
            } else {
#pragma unroll 1
                for (int dy = 0; dy < K; dy++)
#pragma unroll
                    for (int dx = 0; dx < K; dx++) {
                        const int s = (ly + dy) * SW + lx + dx;
                        const i32 v = tile[s];
                        const u32 w = v != 0 ? wt[abs(gc - (int)gray[s])] : 0u;
                        total += w;
                        lo = v != 0 && v < lo ? v : lo;
                        hi = v != 0 && v > hi ? v : hi;
                    }
                if (total) res = wmed_bisect(lo, hi, total, [&](i32 x) {
                    u32 cum = 0;
#pragma unroll 1
                    for (int dy = 0; dy < K; dy++)
#pragma unroll
                        for (int dx = 0; dx < K; dx++) {
                            const int s = (ly + dy) * SW + lx + dx;
                            const i32 v = tile[s];
                            cum += v != 0 && v <= x ? wt[abs(gc - (int)gray[s])] : 0u;
                        }
                    return cum;
                });
            }
            if (c == 0) {
                res = total >= fill_min ? res : 0;      // (total = 0: res = 0; fill_min >= 1 here)
                cnt += res != 0;
            }
        }
        out[base + (size_t)gy * W + gx] = (T)res;
    }
    if (filled) lr_count(filled + blockIdx.z, cnt);
}

template <typename T, int R>
static void wmed_go(const void *in, const u8 *guide, const WmedTable &table, void *out, i32 *filled, int W, int H, int pairs,
                    u32 fill_min, hipStream_t st)
{
    const dim3 grid((W + FLT_TW - 1) / FLT_TW, (H + FLT_TH - 1) / FLT_TH, pairs), block(256);
    hipLaunchKernelGGL((k_wmedian<T, R>), grid, block, 0, st, (const T *)in, guide, table, (T *)out, filled, W, H, fill_min);
}

template <typename T>
static void wmed_radius(int radius, const void *in, const u8 *guide, const WmedTable &table, void *out, i32 *filled, int W,
                        int H, int pairs, u32 fill_min, hipStream_t st)
{
    switch (radius) {
#define SM_WMED_GO(R_) case R_: wmed_go<T, R_>(in, guide, table, out, filled, W, H, pairs, fill_min, st); break
        SM_WMED_GO(1); SM_WMED_GO(2); SM_WMED_GO(3); SM_WMED_GO(4); SM_WMED_GO(5); SM_WMED_GO(6); SM_WMED_GO(7);
#undef SM_WMED_GO
    }
}

extern "C" int sm_weighted_median(sm_plan *plan, const void *d_in, int map_type, const uint8_t *d_guide, int radius,
                                  const uint16_t weights[256], int flags, int fill_min_weight, int pairs, void *d_out,
                                  int32_t *d_filled, void *stream)
{
    const char *me = "sm_weighted_median";
    size_t elem;
    if (!d_in || !d_out) return sm_fail(SM_ERR_ARG, "%s: a map pointer is NULL", me);
    if (!d_guide) return sm_fail(SM_ERR_ARG, "%s: d_guide is NULL", me);
    if (!weights) return sm_fail(SM_ERR_ARG, "%s: weights is NULL", me);
    SM_TRY(sm_check_map_type(map_type, me, &elem));
    if (radius < 1 || radius > WMED_MAX_R) return sm_fail(SM_ERR_ARG, "%s: radius %d outside 1..%d", me, radius, WMED_MAX_R);
    if (weights[0] == 0) return sm_fail(SM_ERR_ARG, "%s: weights[0] is 0 (the centre of a valid pixel must count)", me);
    if (flags & ~SM_WMED_FILL) return sm_fail(SM_ERR_ARG, "%s: flags 0x%x has bits this library does not know", me, flags);
    const bool fill = (flags & SM_WMED_FILL) != 0;
    if (fill && fill_min_weight < 1) return sm_fail(SM_ERR_ARG, "%s: fill_min_weight %d is below 1", me, fill_min_weight);
    SM_TRY(sm_check_pairs(plan, pairs, me));
    const int W = plan->width, H = plan->height;
    const size_t n = (size_t)pairs * W * H, map = n * elem;
    if (overlap(d_in, d_out, map))
        return sm_fail(SM_ERR_ARG, "%s: maps overlap (every output pixel reads its neighbours' inputs)", me);
    if (overlap(d_guide, d_out, n, map)) return sm_fail(SM_ERR_ARG, "%s: d_guide overlaps the output map", me);
    const size_t counts = (size_t)pairs * sizeof(i32);
    if (d_filled && (overlap(d_filled, d_in, counts, map) || overlap(d_filled, d_out, counts, map) ||
                     overlap(d_filled, d_guide, counts, n)))
        return sm_fail(SM_ERR_ARG, "%s: d_filled overlaps a map", me);
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    const WmedTable table = wmed_table(weights);
    if (d_filled) SM_TRY(sm_lr_zero_counts(d_filled, pairs, st));
    // (without the flag nothing is filled: the counts stay 0 and the kernel counts nothing)
    i32 *filled = fill ? d_filled : nullptr;
    const u32 fill_min = fill ? (u32)fill_min_weight : 0u;
    if (map_type == SM_MAP_I32) wmed_radius<i32>(radius, d_in, d_guide, table, d_out, filled, W, H, pairs, fill_min, st);
    else wmed_radius<int16_t>(radius, d_in, d_guide, table, d_out, filled, W, H, pairs, fill_min, st);
    SM_LAUNCH_CHECK("k_wmedian");
    return SM_OK;
}
