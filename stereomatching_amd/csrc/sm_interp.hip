// sm_interp.hip -- occlusion-aware interpolation of checked disparity maps: classification of the invalid pixels and
// the discontinuity-preserving fill (include/stereo_hip.h).  It reuses flt_sort (the exchange network) and
// lr_count of sm_device.h, and k_lr_zero_counts through sm_lr_zero_counts.
//
// PARITY UNPINNED: the reference has no such stage.  Definition (tests/interp_reference.py is its executable form).
// Maps are [pairs][H][W] of int32 (a web map) or int16 (a sub map); a pixel is valid iff its value != 0; pairs are
// independent.
//   classify: 0 where web != 0; else 2 (mismatched) if some d in 0 .. D-1 has u = x + d inside the row (toroidal:
//     u mod W; ghost: u < W) and web_right(u, y) = d + 1; else 1 (occluded).
//   interpolate: out(p) = in(p) where in(p) != 0.  Else the candidates c_0 <= ... <= c_{m-1} are the first valid
//     values of the INPUT met walking from p in each of the eight directions (no wrapping); out(p) = 0 if m = 0,
//     c_{min(1, m-1)} if class(p) = 1, else the lower median c_{(m-1)/2}.
//
// No loop here has a trip count that depends on the distance to a valid pixel: every direction is a sweep that
// carries the last valid value along a line, cut into pieces that run side by side and are joined by their carries.
//   horizontal   a wave owns a chunk of 64 pixels of a row: the nearest valid lane on either side is a bit scan of the
//                ballot and one ds_bpermute.  k_itp_rowsum writes every chunk's first and last valid value,
//                k_itp_rowscan (a wave per row, a lane per chunk, the same bit scan) turns them into the value that
//                enters each chunk from the right and from the left.
//   vertical and diagonal: direction dir = 0 .. 5 sweeps down (dir < 3) or up, dx = 0, +1, -1.  Pixel (x, y) lies on
//                line l = x - dx * y (+ H - 1 for dx > 0) of W (dx = 0) or W + H - 1 lines; a lane owns a line, adjacent
//                lanes adjacent lines, so the loads of a step are coalesced.  k_itp_sweep does one segment of 64 rows
//                of 256 lines: the loads do not depend on the carry and are issued eight rows ahead.  It stores the
//                segment-local value for every invalid pixel (0: none met inside the segment) and the segment's
//                outgoing carry; k_itp_resolve scans the carries of a line over the segments (H / 64 steps) into the
//                value that enters each segment.
//   k_itp_combine  a wave per row chunk: the two horizontal candidates from the ballot, six from the directional maps
//                (where 0: from the carry entering the pixel's segment on its line), sorted by the 19-exchange network
//                with missing candidates as INT_MAX, the rank picked, the filled pixels counted per workgroup.
// Workspace per pair, 4 bytes an element: directional maps [6][H][W] (int16 maps use the first half), line carries
// [6][segments][W + H - 1], row carries [2][H][chunks].


#include "sm_device.h"

#include <algorithm>

#define ITP_SEG 64      // rows of a line segment (k_itp_sweep)
#define ITP_CW 64       // pixels of a row chunk: one wave

__host__ __device__ __forceinline__ int itp_dx(int dir) { return dir % 3 == 0 ? 0 : dir % 3 == 1 ? 1 : -1; }

// the value of the nearest lane below / above this one that holds a valid value (mask = ballot(v != 0)), `carry` if
// there is none; called by all 64 lanes
__device__ __forceinline__ i32 itp_from_left(i32 v, unsigned long long mask, int lane, i32 carry)
{
    const unsigned long long below = mask & ((1ull << lane) - 1);
    const i32 got = __shfl(v, below ? 63 - __clzll((long long)below) : lane);
    return below ? got : carry;
}

__device__ __forceinline__ i32 itp_from_right(i32 v, unsigned long long mask, int lane, i32 carry)
{
    const unsigned long long above = lane == 63 ? 0ull : mask >> (lane + 1);
    const i32 got = __shfl(v, above ? lane + __ffsll((long long)above) : lane);
    return above ? got : carry;
}

// ---------------------------------------------------------------------------
// classification
// ---------------------------------------------------------------------------

// grid (ceil(npx / 256), pairs), block 256: a lane per pixel; an invalid pixel reads up to D values of its own row
__global__ __launch_bounds__(256) void k_itp_classify(const i32 *__restrict__ web, const i32 *__restrict__ right,
                                                      u8 *__restrict__ cls, int W, unsigned npx, int D, int ghost)
{
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p >= npx) return;
    const size_t base = (size_t)blockIdx.y * npx;
    u8 c = 0;
    if (web[base + p] == 0) {
        const unsigned y = p / (unsigned)W;
        const i32 *rrow = right + base + (size_t)y * W;
        int u = (int)(p - y * (unsigned)W);
        bool hit = false;
        for (int d = 0; d < D; d++) {
            if (u == W) {
                if (ghost) break;
                u = 0;
            }
            hit |= rrow[u] == d + 1;
            u++;
        }
        c = hit ? 2 : 1;
    }
    cls[base + p] = c;
}

// ---------------------------------------------------------------------------
// interpolation
// ---------------------------------------------------------------------------

// grid (ceil(H * chunks / 4), pairs), block 256: a wave per row chunk -> its first and last valid value (0: none)
template <typename T>
__global__ __launch_bounds__(256) void k_itp_rowsum(const T *__restrict__ in, i32 *__restrict__ rows, int W, int H,
                                                    int chunks)
{
    const unsigned t = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (t >= (unsigned)H * chunks) return;
    const int lane = threadIdx.x & 63;
    const unsigned y = t / (unsigned)chunks, c = t - y * (unsigned)chunks;
    const int x = (int)c * ITP_CW + lane;
    const i32 v = x < W ? (i32)in[((size_t)blockIdx.y * H + y) * W + x] : 0;
    const unsigned long long mask = __ballot(v != 0);
    const i32 first = __shfl(v, mask ? __ffsll((long long)mask) - 1 : 0);
    const i32 last = __shfl(v, mask ? 63 - __clzll((long long)mask) : 0);
    if (lane == 0) {
        i32 *r = rows + (size_t)blockIdx.y * 2 * H * chunks + (size_t)y * chunks + c;
        r[0] = first;                                   // (no valid lane: lane 0's own 0)
        r[(size_t)H * chunks] = last;
    }
}

// grid (ceil(H / 4), pairs), block 256: a wave per row, a lane per chunk, 64 chunks a step.  In place: a chunk's last
// valid value becomes the value entering it from the left, its first valid value the one entering from the right.
__global__ __launch_bounds__(256) void k_itp_rowscan(i32 *rows, int H, int chunks)
{
    const unsigned y = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (y >= (unsigned)H) return;
    const int lane = threadIdx.x & 63;
    i32 *first = rows + (size_t)blockIdx.y * 2 * H * chunks + (size_t)y * chunks, *last = first + (size_t)H * chunks;
    i32 carry = 0;
    for (int c0 = 0; c0 < chunks; c0 += 64) {
        const int c = c0 + lane;
        const i32 v = c < chunks ? last[c] : 0;
        const unsigned long long mask = __ballot(v != 0);
        const i32 got = itp_from_left(v, mask, lane, carry);
        if (c < chunks) last[c] = got;
        if (mask) carry = __shfl(v, 63 - __clzll((long long)mask));
    }
    carry = 0;
    for (int c0 = (chunks - 1) / 64 * 64; c0 >= 0; c0 -= 64) {
        const int c = c0 + lane;
        const i32 v = c < chunks ? first[c] : 0;
        const unsigned long long mask = __ballot(v != 0);
        const i32 got = itp_from_right(v, mask, lane, carry);
        if (c < chunks) first[c] = got;
        if (mask) carry = __shfl(v, __ffsll((long long)mask) - 1);
    }
}

// grid (ceil(lines / 256), segments, 6 * pairs), block 256: lane = line, one segment of one direction.  A line of a
// diagonal direction is inside the image for one run of rows only; outside it reads as invalid, which leaves the carry
// what it was: 0 before the line enters the image, and of no use after it has left.
template <typename T>
__global__ __launch_bounds__(256) void k_itp_sweep(const T *__restrict__ in, T *__restrict__ loc, i32 *__restrict__ car,
                                                   int W, int H, int segs)
{
    const int dir = blockIdx.z % 6, pair = blockIdx.z / 6;
    const int dx = itp_dx(dir), lines = W + H - 1;
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= (dx ? lines : W)) return;
    const bool down = dir < 3;
    const int y0 = blockIdx.y * ITP_SEG, xoff = l - (dx > 0 ? H - 1 : 0);
    const size_t npx = (size_t)W * H;
    const T *src = in + pair * npx;
    T *dst = loc + ((size_t)pair * 6 + dir) * npx;
    i32 run = 0;
    for (int b = 0; b < ITP_SEG; b += 8) {
        i32 v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int y = down ? y0 + b + j : y0 + ITP_SEG - 1 - b - j, x = xoff + dx * y;
            v[j] = y < H && x >= 0 && x < W ? (i32)src[(size_t)y * W + x] : 0;
        }
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int y = down ? y0 + b + j : y0 + ITP_SEG - 1 - b - j, x = xoff + dx * y;
            if (v[j] != 0) run = v[j];
            else if (y < H && x >= 0 && x < W) dst[(size_t)y * W + x] = (T)run;
        }
    }
    car[(((size_t)pair * 6 + dir) * segs + blockIdx.y) * lines + l] = run;
}

// grid (ceil(lines / 256), 6, pairs), block 256: lane = line; a segment's outgoing carry becomes, in place, the value
// that enters it (from the segments above for a downward direction, from those below for an upward one)
__global__ __launch_bounds__(256) void k_itp_resolve(i32 *car, int W, int H, int segs)
{
    const int dir = blockIdx.y, lines = W + H - 1;
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= (itp_dx(dir) ? lines : W)) return;
    i32 *c = car + ((size_t)blockIdx.z * 6 + dir) * segs * lines + l;
    i32 run = 0;
    for (int k = 0; k < segs; k++) {
        const size_t s = (size_t)(dir < 3 ? k : segs - 1 - k) * lines;
        const i32 t = c[s];
        c[s] = run;
        if (t != 0) run = t;
    }
}

// grid (up to SM_LR_BLOCKS, pairs), block 256, the four waves striding over the row chunks of the pair
template <typename T>
__global__ __launch_bounds__(256) void k_itp_combine(const T *__restrict__ in, const u8 *__restrict__ cls,
                                                     T *__restrict__ out, const T *__restrict__ loc,
                                                     const i32 *__restrict__ car, const i32 *__restrict__ rows,
                                                     i32 *filled, int W, int H, int segs, int chunks)
{
    const int lane = threadIdx.x & 63, pair = blockIdx.y, lines = W + H - 1;
    const size_t npx = (size_t)W * H, base = pair * npx;
    const i32 *first = rows + (size_t)pair * 2 * H * chunks, *last = first + (size_t)H * chunks;
    const unsigned items = (unsigned)H * chunks;
    int cnt = 0;
    for (unsigned t = blockIdx.x * 4u + (threadIdx.x >> 6); t < items; t += gridDim.x * 4u) {
        const unsigned uy = t / (unsigned)chunks, c = t - uy * (unsigned)chunks;
        const int y = (int)uy, x = (int)c * ITP_CW + lane;
        const bool inb = x < W;
        const size_t p = (size_t)y * W + x;
        const i32 v = inb ? (i32)in[base + p] : 0;
        const unsigned long long mask = __ballot(v != 0);
        i32 cand[8];
        cand[0] = itp_from_left(v, mask, lane, last[t]);
        cand[1] = itp_from_right(v, mask, lane, first[t]);
        i32 res = v;
        if (inb && v == 0) {
            const int seg = y / ITP_SEG;
#pragma unroll
            for (int dir = 0; dir < 6; dir++) {
                const int dx = itp_dx(dir), l = x - dx * y + (dx > 0 ? H - 1 : 0);
                i32 q = (i32)loc[((size_t)pair * 6 + dir) * npx + p];
                if (q == 0) q = car[(((size_t)pair * 6 + dir) * segs + seg) * lines + l];
                cand[2 + dir] = q;
            }
            int m = 0;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                m += cand[j] != 0;
                cand[j] = cand[j] != 0 ? cand[j] : (i32)0x7fffffff;         // the candidates first, ascending
            }
            flt_sort<8>(cand);
            const bool occluded = cls && cls[base + p] == 1;
            const int r = occluded ? (m > 1 ? 1 : 0) : (m - 1) / 2;
            res = m == 0 ? 0 : r <= 0 ? cand[0] : r == 1 ? cand[1] : r == 2 ? cand[2] : cand[3];
            cnt += res != 0;
        }
        if (inb) out[base + p] = (T)res;
    }
    if (filled) lr_count(filled + pair, cnt);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

// sm_interpolate's workspace (layout above), in 4-byte elements per pair: six directional maps, the carries of
// W + H - 1 lines for six directions and every segment, the carries of every row chunk from either side
static int itp_segs(const sm_plan *plan) { return (plan->height + ITP_SEG - 1) / ITP_SEG; }
static int itp_chunks(const sm_plan *plan) { return (plan->width + ITP_CW - 1) / ITP_CW; }
static size_t itp_loc_elems(const sm_plan *plan) { return (size_t)6 * plan->width * plan->height; }
static size_t itp_car_elems(const sm_plan *plan)
{
    return (size_t)6 * itp_segs(plan) * (plan->width + plan->height - 1);
}
static size_t itp_row_elems(const sm_plan *plan) { return (size_t)2 * plan->height * itp_chunks(plan); }
size_t sm_itp_bytes(const sm_plan *plan)
{
    return (size_t)plan->max_pairs * sizeof(i32) * (itp_loc_elems(plan) + itp_car_elems(plan) + itp_row_elems(plan));
}

extern "C" int sm_occlusion_classify(sm_plan *plan, const int32_t *d_web, const int32_t *d_web_right, int pairs,
                                     uint8_t *d_class, void *stream)
{
    const char *me = "sm_occlusion_classify";
    if (!d_web || !d_web_right || !d_class) return sm_fail(SM_ERR_ARG, "%s: a map pointer is NULL", me);
    SM_TRY(sm_check_pairs(plan, pairs, me));
    const unsigned npx = (unsigned)plan->width * plan->height;
    const size_t map = (size_t)pairs * npx * sizeof(i32);
    if (overlap(d_class, d_web, map / 4, map) || overlap(d_class, d_web_right, map / 4, map))
        return sm_fail(SM_ERR_ARG, "%s: d_class overlaps a map", me);
    SM_TRY(sm_use_device(plan->device));
    hipLaunchKernelGGL(k_itp_classify, dim3((npx + 255) / 256, pairs), dim3(256), 0, (hipStream_t)stream, d_web,
                       d_web_right, d_class, plan->width, npx, plan->num_shifts, plan->border == SM_GHOST ? 1 : 0);
    SM_LAUNCH_CHECK("k_itp_classify");
    return SM_OK;
}

extern "C" int sm_plan_reserve_interp(sm_plan *plan)
{
    if (!plan) return sm_fail(SM_ERR_ARG, "sm_plan_reserve_interp: plan is NULL");
    SM_TRY(sm_use_device(plan->device));
    return sm_ws_reserve(plan, SM_WS_SET_INTERP, "sm_plan_reserve_interp");
}

template <typename T>
static int interp_launch(const sm_plan *plan, const T *in, const u8 *cls, T *out, int pairs, i32 *filled, hipStream_t st)
{
    const int W = plan->width, H = plan->height, segs = itp_segs(plan), chunks = itp_chunks(plan);
    T *loc = (T *)plan->d_interp;
    i32 *car = plan->d_interp + plan->max_pairs * itp_loc_elems(plan);
    i32 *rows = car + plan->max_pairs * itp_car_elems(plan);
    const unsigned items = (unsigned)H * chunks, lines = W + H - 1;
    if (filled) SM_TRY(sm_lr_zero_counts(filled, pairs, st));
    hipLaunchKernelGGL(k_itp_rowsum<T>, dim3((items + 3) / 4, pairs), dim3(256), 0, st, in, rows, W, H, chunks);
    SM_LAUNCH_CHECK("k_itp_rowsum");
    hipLaunchKernelGGL(k_itp_rowscan, dim3((H + 3) / 4, pairs), dim3(256), 0, st, rows, H, chunks);
    SM_LAUNCH_CHECK("k_itp_rowscan");
    hipLaunchKernelGGL(k_itp_sweep<T>, dim3((lines + 255) / 256, segs, 6 * pairs), dim3(256), 0, st, in, loc, car, W, H,
                       segs);
    SM_LAUNCH_CHECK("k_itp_sweep");
    hipLaunchKernelGGL(k_itp_resolve, dim3((lines + 255) / 256, 6, pairs), dim3(256), 0, st, car, W, H, segs);
    SM_LAUNCH_CHECK("k_itp_resolve");
    hipLaunchKernelGGL(k_itp_combine<T>, dim3(std::min((items + 3) / 4, (unsigned)SM_LR_BLOCKS), pairs), dim3(256), 0, st,
                       in, cls, out, (const T *)loc, (const i32 *)car, (const i32 *)rows, filled, W, H, segs, chunks);
    SM_LAUNCH_CHECK("k_itp_combine");
    return SM_OK;
}

extern "C" int sm_interpolate(sm_plan *plan, const void *d_in, int map_type, const uint8_t *d_class, int pairs,
                              void *d_out, int32_t *d_filled, void *stream)
{
    const char *me = "sm_interpolate";
    size_t elem;
    if (!d_in || !d_out) return sm_fail(SM_ERR_ARG, "%s: a map pointer is NULL", me);
    SM_TRY(sm_check_map_type(map_type, me, &elem));
    SM_TRY(sm_check_pairs(plan, pairs, me));
    const size_t px = (size_t)pairs * plan->width * plan->height, map = px * elem;
    if (overlap(d_in, d_out, map))
        return sm_fail(SM_ERR_ARG, "%s: maps overlap (every candidate is read from the input)", me);
    if (d_class && overlap(d_class, d_out, px, map)) return sm_fail(SM_ERR_ARG, "%s: d_class overlaps d_out", me);
    const size_t counts = (size_t)pairs * sizeof(i32);
    if (d_filled && (overlap(d_filled, d_in, counts, map) || overlap(d_filled, d_out, counts, map) ||
                     (d_class && overlap(d_filled, d_class, counts, px))))
        return sm_fail(SM_ERR_ARG, "%s: d_filled overlaps a map", me);
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    SM_TRY(sm_ws_need(plan, SM_WS_SET_INTERP, st, me));
    if (map_type == SM_MAP_I32)
        return interp_launch<i32>(plan, (const i32 *)d_in, d_class, (i32 *)d_out, pairs, d_filled, st);
    return interp_launch<int16_t>(plan, (const int16_t *)d_in, d_class, (int16_t *)d_out, pairs, d_filled, st);
}
