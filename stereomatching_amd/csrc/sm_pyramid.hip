// sm_pyramid.hip -- the half-resolution path (include/stereo_hip.h "half-resolution path"): an
// image is reduced by two in each direction, the matcher runs on the reduced pair with half the shifts (an eighth of
// the cost volume), and the coarse map is brought back to the fine size along the edges of the fine image.
//
// PARITY UNPINNED: the reference has no such stage.  Definition (tests/pyramid_reference.py is its executable form).
// Both calls take the plan of the FINE size W x H; the coarse size is cw = (W + 1) >> 1, ch = (H + 1) >> 1.  Nothing
// wraps, in either border mode; pairs are independent.
//   sm_reduce_half: u8 [images][H][W] -> u8 [images][ch][cw], exact integers, cx(u) = min(max(u, 0), W - 1), cy alike:
//     SM_REDUCE_BOX:      dst(X, Y) = (sum{i, j in 0..1} src(cx(2X + i), cy(2Y + j)) + 2) >> 2
//     SM_REDUCE_BINOMIAL: k = [1, 3, 3, 1], dst = (sum{i, j in 0..3} k_i k_j src(cx(2X - 1 + i), cy(2Y - 1 + j)) + 32) >> 6
//   sm_upsample_double: map [pairs][ch][cw] -> [pairs][H][W] of the same type; a pixel is valid iff != 0.
//     v(c) = clamp(2 in(c) - 1) for int32 (web = 1 + shift), clamp(2 in(c) - 16) for int16 (sub = 16 web + fraction).
//     fine pixel p = (x, y): home (X, Y) = (x >> 1, y >> 1), px = x & 1, py = y & 1.  Taps: the coarse pixels
//     c = (X + i, Y + j), i, j in -1..1, that lie in the coarse image and have in(c) != 0, each with
//     w_c = weights[|g(p) - gc(c)|] s(i, px) s(j, py), where s = 4, 2, 1 for |4i + 1 - 2px| = 1, 3, 5.  T = sum w_c.
//     wmed(p) = the smallest v(c), signed order, with 2 sum{w_c' : v(c') <= v(c)} >= T (the lower weighted median).
//     flags = 0: out(p) = 0 where in(home) = 0, else wmed(p).  SM_UP_FILL: where in(home) = 0, wmed(p) if there is a
//     tap, else 0.
//
// Kernels:
//   k_reduce_half<FILTER>  a lane owns four adjacent coarse pixels of one coarse row: dword loads of the source rows
//                          (two a row for the box, three for the binomial's ten columns), one dword store.  The
//                          vertical replicate is a clamp of the row index, so only the lanes whose columns touch the
//                          left or right end of a row (one at the left, at most two at the right) leave that path:
//                          they gather their ten columns through cx, byte by byte, and store as many bytes as the row
//                          has left.  Rows of an odd width are not dword-aligned: the loads and the store are typed as
//                          unaligned dwords, which global memory takes as they are on gfx950.
//   k_upsample_double<T>   the post-filters' 64 x 16 fine tile, 256 lanes: the 34 x 10 coarse pixels under it and
//                          around it staged in LDS, values as int32 (0 for a tap outside the coarse image: a missing
//                          tap and an invalid one are treated alike) and the coarse guide as bytes; the weight table
//                          by value in the arguments, staged in LDS once per workgroup, as k_wmedian takes it.  A lane
//                          owns a column of the tile and four of its rows.  Nine values and nine weights in registers;
//                          every tap sums the weights of the taps <= it (81 compare-adds) and the least tap that
//                          reaches half of T is the result: no bisection, no sort.

#include "sm_device.h"

typedef u32 __attribute__((aligned(1))) u32_unaligned;

// the four outputs of a lane from the ten (binomial) or eight (box) vertical column sums c[0..]: packed low byte first
template <int FILTER>
__device__ __forceinline__ u32 red_pack(const u32 *c)
{
    u32 r = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const u32 v = FILTER == SM_REDUCE_BOX ? (c[2 * k] + c[2 * k + 1] + 2u) >> 2
                                              : (c[2 * k] + 3u * (c[2 * k + 1] + c[2 * k + 2]) + c[2 * k + 3] + 32u) >> 6;
        r |= v << (8 * k);
    }
    return r;
}

// grid (ceil(ceil(cw / 4) / 64), ceil(ch / 4), images), block (64, 4): lane (x, y) owns coarse pixels 4 x .. 4 x + 3 of row y
template <int FILTER>
__global__ __launch_bounds__(256) void k_reduce_half(const u8 *__restrict__ src, u8 *__restrict__ dst, int W, int H, int cw,
                                                     int ch)
{
    constexpr bool BOX = FILTER == SM_REDUCE_BOX;
    constexpr int ROWS = BOX ? 2 : 4, COLS = BOX ? 8 : 10, LEFT = BOX ? 0 : 1;
    const int X0 = 4 * (blockIdx.x * 64 + threadIdx.x), Y = blockIdx.y * 4 + threadIdx.y;
    if (X0 >= cw || Y >= ch) return;
    const u8 *img = src + (size_t)blockIdx.z * W * H;
    u8 *o = dst + ((size_t)blockIdx.z * ch + Y) * cw + X0;
    const int u0 = 2 * X0 - LEFT;                                     // the lane's first source column
    u32 c[COLS];
#pragma unroll
    for (int k = 0; k < COLS; k++) c[k] = 0;
    if (u0 >= 0 && u0 + COLS <= W) {
#pragma unroll
        for (int j = 0; j < ROWS; j++) {
            const int v = min(max(2 * Y - LEFT + j, 0), H - 1);
            const u8 *row = img + (size_t)v * W + u0;
            const u32 kj = BOX || j == 0 || j == 3 ? 1u : 3u;
            // columns 0..3, 4..7 and (binomial) 6..9 of the lane: the third dword overlaps the second by two bytes
            const u32 a = *(const u32_unaligned *)row, b = *(const u32_unaligned *)(row + 4);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                c[k] += kj * ((a >> (8 * k)) & 255u);
                c[4 + k] += kj * ((b >> (8 * k)) & 255u);
            }
            if constexpr (!BOX) {
                const u32 e = *(const u32_unaligned *)(row + 6);
                c[8] += kj * ((e >> 16) & 255u);
                c[9] += kj * (e >> 24);
            }
        }
        *(u32_unaligned *)o = red_pack<FILTER>(c);
        return;
    }
    // a lane at the left or right end of the row: its columns through cx, and the bytes the row has left
#pragma unroll
    for (int j = 0; j < ROWS; j++) {
        const int v = min(max(2 * Y - LEFT + j, 0), H - 1);
        const u8 *row = img + (size_t)v * W;
        const u32 kj = BOX || j == 0 || j == 3 ? 1u : 3u;
#pragma unroll
        for (int k = 0; k < COLS; k++) c[k] += kj * row[min(max(u0 + k, 0), W - 1)];
    }
    const u32 r = red_pack<FILTER>(c);
    const int n = min(4, cw - X0);
    for (int k = 0; k < n; k++) o[k] = (u8)(r >> (8 * k));
}

// v(c): the coarse value on the fine scale
template <typename T>
__device__ __forceinline__ i32 up_scale(i32 in)
{
    if constexpr (sizeof(T) == 4) {
        const long long v = 2ll * in - 1;
        return (i32)(v < -2147483648ll ? -2147483648ll : v > 2147483647ll ? 2147483647ll : v);
    } else {
        const i32 v = 2 * in - 16;
        return v < -32768 ? -32768 : v > 32767 ? 32767 : v;
    }
}

#define UP_SW (FLT_TW / 2 + 2)
#define UP_SH (FLT_TH / 2 + 2)

// grid (ceil(W / 64), ceil(H / 16), pairs), block 256.  fill: an invalid home takes the median of its taps.
template <typename T>
__global__ __launch_bounds__(256) void k_upsample_double(const T *__restrict__ in, const u8 *__restrict__ guide,
                                                         const u8 *__restrict__ guide_coarse, WmedTable table,
                                                         T *__restrict__ out, int W, int H, int cw, int ch, int fill)
{
    __shared__ i32 tile[UP_SH * UP_SW];
    __shared__ u8 gray[UP_SH * UP_SW];
    __shared__ uint16_t wt[256];
    const int tx0 = blockIdx.x * FLT_TW, ty0 = blockIdx.y * FLT_TH;
    const size_t base = (size_t)blockIdx.z * W * H, cbase = (size_t)blockIdx.z * cw * ch;
    wt[threadIdx.x] = table.w[threadIdx.x];
    for (int i = threadIdx.x; i < UP_SH * UP_SW; i += 256) {
        const int sy = i / UP_SW, sx = i - sy * UP_SW;
        const int cx = tx0 / 2 + sx - 1, cy = ty0 / 2 + sy - 1;
        const bool inside = cx >= 0 && cx < cw && cy >= 0 && cy < ch;
        tile[i] = inside ? (i32)in[cbase + (size_t)cy * cw + cx] : 0;
        gray[i] = inside ? guide_coarse[cbase + (size_t)cy * cw + cx] : (u8)0;
    }
    __syncthreads();
    const int lx = threadIdx.x & 63, gx = tx0 + lx;
    if (gx >= W) return;
    const int px = lx & 1, hx = (lx >> 1) + 1;                        // the home's column in the staged tile
    // s(i, px) for i = -1, 0, 1
    const u32 sxw[3] = {px ? 1u : 2u, 4u, px ? 2u : 1u};
    for (int ly = threadIdx.x >> 6; ly < FLT_TH; ly += 4) {
        const int gy = ty0 + ly;
        if (gy >= H) break;
        const int py = ly & 1, hy = (ly >> 1) + 1;
        const i32 home = tile[hy * UP_SW + hx];
        i32 res = 0;
        if (home != 0 || fill) {
            const int g = guide[base + (size_t)gy * W + gx];
            i32 v[9];
            u32 w[9], total = 0;
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const u32 syw = j == 1 ? 4u : (j == 0) == (py == 0) ? 2u : 1u;
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    const int s = (hy + j - 1) * UP_SW + hx + i - 1, t = j * 3 + i;
                    const i32 raw = tile[s];
                    v[t] = up_scale<T>(raw);
                    w[t] = raw != 0 ? (u32)wt[abs(g - (int)gray[s])] * sxw[i] * syw : 0u;
                    total += w[t];
                }
            }
            // (an absent tap has weight 0: it is no candidate, and what it adds to a sum is 0)
            bool any = false;
#pragma unroll
            for (int t = 0; t < 9; t++) {
                u32 cum = 0;
#pragma unroll
                for (int u = 0; u < 9; u++) cum += v[u] <= v[t] ? w[u] : 0u;
                const bool ok = w[t] != 0 && 2u * cum >= total;
                res = ok && (!any || v[t] < res) ? v[t] : res;
                any |= ok;
            }
        }
        out[base + (size_t)gy * W + gx] = (T)res;
    }
}

extern "C" int sm_reduce_half(sm_plan *plan, const uint8_t *d_src, int filter, int images, uint8_t *d_dst, void *stream)
{
    const char *me = "sm_reduce_half";
    if (!d_src || !d_dst) return sm_fail(SM_ERR_ARG, "%s: an image pointer is NULL", me);
    if (filter != SM_REDUCE_BOX && filter != SM_REDUCE_BINOMIAL)
        return sm_fail(SM_ERR_ARG, "%s: filter %d is neither SM_REDUCE_BOX nor SM_REDUCE_BINOMIAL", me, filter);
    if (!plan) return sm_fail(SM_ERR_ARG, "%s: plan is NULL", me);
    if (images < 1 || images > 2 * plan->max_pairs)
        return sm_fail(SM_ERR_ARG, "%s: images %d outside 1..%d (twice max_pairs of the plan)", me, images, 2 * plan->max_pairs);
    const int W = plan->width, H = plan->height, cw = (W + 1) >> 1, ch = (H + 1) >> 1;
    if (overlap(d_src, d_dst, (size_t)images * W * H, (size_t)images * cw * ch))
        return sm_fail(SM_ERR_ARG, "%s: images overlap", me);
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(((cw + 3) / 4 + 63) / 64, (ch + 3) / 4, images), block(64, 4);
    if (filter == SM_REDUCE_BOX) hipLaunchKernelGGL(k_reduce_half<SM_REDUCE_BOX>, grid, block, 0, st, d_src, d_dst, W, H, cw, ch);
    else hipLaunchKernelGGL(k_reduce_half<SM_REDUCE_BINOMIAL>, grid, block, 0, st, d_src, d_dst, W, H, cw, ch);
    SM_LAUNCH_CHECK("k_reduce_half");
    return SM_OK;
}

extern "C" int sm_upsample_double(sm_plan *plan, const void *d_in, int map_type, const uint8_t *d_guide,
                                  const uint8_t *d_guide_coarse, const uint16_t weights[256], int flags, int pairs,
                                  void *d_out, void *stream)
{
    const char *me = "sm_upsample_double";
    size_t elem;
    if (!d_in || !d_out) return sm_fail(SM_ERR_ARG, "%s: a map pointer is NULL", me);
    if (!d_guide || !d_guide_coarse) return sm_fail(SM_ERR_ARG, "%s: a guide pointer is NULL", me);
    if (!weights) return sm_fail(SM_ERR_ARG, "%s: weights is NULL", me);
    SM_TRY(sm_check_map_type(map_type, me, &elem));
    for (int i = 0; i < 256; i++)
        if (weights[i] == 0) return sm_fail(SM_ERR_ARG, "%s: weights[%d] is 0 (no tap is the centre: every weight must be >= 1)", me, i);
    if (flags & ~SM_UP_FILL) return sm_fail(SM_ERR_ARG, "%s: flags 0x%x has bits this library does not know", me, flags);
    SM_TRY(sm_check_pairs(plan, pairs, me));
    const int W = plan->width, H = plan->height, cw = (W + 1) >> 1, ch = (H + 1) >> 1;
    const size_t n = (size_t)pairs * W * H, cn = (size_t)pairs * cw * ch;
    if (overlap(d_in, d_out, cn * elem, n * elem))
        return sm_fail(SM_ERR_ARG, "%s: maps overlap (every output pixel reads its neighbours' inputs)", me);
    if (overlap(d_guide, d_out, n, n * elem) || overlap(d_guide_coarse, d_out, cn, n * elem))
        return sm_fail(SM_ERR_ARG, "%s: a guide overlaps the output map", me);
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    const WmedTable table = wmed_table(weights);
    const dim3 grid((W + FLT_TW - 1) / FLT_TW, (H + FLT_TH - 1) / FLT_TH, pairs), block(256);
    const int fill = (flags & SM_UP_FILL) != 0;
    if (map_type == SM_MAP_I32)
        hipLaunchKernelGGL(k_upsample_double<i32>, grid, block, 0, st, (const i32 *)d_in, d_guide, d_guide_coarse, table,
                           (i32 *)d_out, W, H, cw, ch, fill);
    else
        hipLaunchKernelGGL(k_upsample_double<int16_t>, grid, block, 0, st, (const int16_t *)d_in, d_guide, d_guide_coarse,
                           table, (int16_t *)d_out, W, H, cw, ch, fill);
    SM_LAUNCH_CHECK("k_upsample_double");
    return SM_OK;
}
