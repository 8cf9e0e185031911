// sm_reproject.hip -- disparity reprojection (include/stereo_hip.h "reprojection"): the stage
// BEHIND the matchers, the check, the filters and the interpolation.
//
//   k_reproject      the dense maps: every pixel of a disparity map through the 4 x 4 matrix Q to (X, Y, Z) in float,
//                    depth [pairs][H][W] and / or XYZ [pairs][H][W][3], `missing` where the pixel is not kept, and the
//                    kept pixels of each pair counted (lr_count's pattern: one atomic per workgroup)
//   k_cloud_count    the compacted cloud, launch 1 of 3: the kept pixels of every tile of SM_CLOUD_TILE pixels
//   k_cloud_scan     launch 2: one workgroup per pair turns the tile counts into exclusive offsets, and writes the total
//   k_cloud_write    launch 3: every pixel once more; a kept one finds its place from its rank in the wave (ballot),
//                    the waves before it in the tile (LDS) and the tile's offset, and stores one 16-byte record
// The three launches are ordered by the stream: no workgroup waits for another, there is no flag and no look-back.
//
// The arithmetic is IEEE double, one operation at a time in the order tests/reproject_reference.py fixes (this file
// is compiled with -ffp-contract=off, as every file of the library is): four rows ((Qi0 x + Qi1 y) + Qi2 d) + Qi3,
// three divisions by the fourth, three conversions to float.  Q travels by value as a kernel argument.  Nothing may
// be hoisted across pixels: Qi0 x + Qi1 y of a pixel is rounded before Qi2 d is added, and so it is here.
//
// The dense kernel is a stream: 2 or 4 map bytes in, 4 / 12 / 16 bytes out per pixel.  A lane owns four consecutive
// pixels of a row (V = 4: W % 4 == 0, map and outputs 16-byte aligned, the int16 map 8): one 16- or 8-byte load, one
// 16-byte depth store, three 16-byte stores for the 48 contiguous bytes of its four triples.  Other widths and
// alignments take one pixel per lane (V = 1).  The cloud reads one element per lane and iteration (the order of the
// records is the order of the lanes) and computes the arithmetic twice instead of storing a dense XYZ map in between.

#include "sm_device.h"

#include <algorithm>
#include <cmath>

#define SM_CLOUD_TILE 1024      // pixels per tile of the compaction: 256 lanes, four pixels each
#define SM_CLOUD_SCAN 256       // lanes of k_cloud_scan's one workgroup per pair

struct RpjQ {
    double q[16];
};

template <typename T>
__device__ __forceinline__ double rpj_disparity(T v)
{
    if constexpr (sizeof(T) == 2) return (double)v / 16.0 - 1.0;      // (exact: a power of two)
    else return (double)v - 1.0;
}

// one pixel: (X, Y, Z) in float, and whether it is kept (valid, all three finite, z_min <= Z <= z_max)
__device__ __forceinline__ bool rpj_pixel(const RpjQ &Q, int x, int y, double d, bool valid, float z_min, float z_max,
                                          float &X, float &Y, float &Z)
{
    const double xd = (double)x, yd = (double)y;
    const double r0 = ((Q.q[0] * xd + Q.q[1] * yd) + Q.q[2] * d) + Q.q[3];
    const double r1 = ((Q.q[4] * xd + Q.q[5] * yd) + Q.q[6] * d) + Q.q[7];
    const double r2 = ((Q.q[8] * xd + Q.q[9] * yd) + Q.q[10] * d) + Q.q[11];
    const double wh = ((Q.q[12] * xd + Q.q[13] * yd) + Q.q[14] * d) + Q.q[15];
    X = (float)(r0 / wh);
    Y = (float)(r1 / wh);
    Z = (float)(r2 / wh);
    return valid && __builtin_isfinite(X) && __builtin_isfinite(Y) && __builtin_isfinite(Z) && z_min <= Z && Z <= z_max;
}

// Grid: x strides over the lanes of one pair (at most SM_LR_BLOCKS workgroups: lr_count's one atomic each), y = pair.
template <typename T, int V>
__global__ __launch_bounds__(256) void k_reproject(const T *__restrict__ map, RpjQ Q, float z_min, float z_max, float missing,
                                                   float *__restrict__ depth, float *__restrict__ xyz, i32 *count, int W,
                                                   unsigned npx)
{
    const size_t base = (size_t)blockIdx.y * npx;
    const unsigned lanes = npx / V;
    int cnt = 0;
    for (unsigned t = blockIdx.x * 256u + threadIdx.x; t < lanes; t += gridDim.x * 256u) {
        const unsigned p = t * V;
        const unsigned row = p / (unsigned)W;
        const int x = (int)(p - row * (unsigned)W), y = (int)row;
        T v[V];
        if constexpr (V == 4 && sizeof(T) == 4) {
            const int4 e = *(const int4 *)(map + base + p);
            v[0] = e.x; v[1] = e.y; v[2] = e.z; v[3] = e.w;
        } else if constexpr (V == 4) {
            const uint2 e = *(const uint2 *)(map + base + p);
            v[0] = (T)(e.x & 0xffffu); v[1] = (T)(e.x >> 16); v[2] = (T)(e.y & 0xffffu); v[3] = (T)(e.y >> 16);
        } else {
            v[0] = map[base + p];
        }
        float o[3 * V], z[V];
#pragma unroll
        for (int i = 0; i < V; i++) {
            float X, Y, Z;
            const bool kept = rpj_pixel(Q, x + i, y, rpj_disparity<T>(v[i]), v[i] != 0, z_min, z_max, X, Y, Z);
            cnt += kept;
            o[3 * i] = kept ? X : missing;
            o[3 * i + 1] = kept ? Y : missing;
            o[3 * i + 2] = z[i] = kept ? Z : missing;
        }
        if constexpr (V == 4) {
            if (depth) *(float4 *)(depth + base + p) = make_float4(z[0], z[1], z[2], z[3]);
            if (xyz) {
                float4 *q = (float4 *)(xyz + (base + p) * 3);
                q[0] = make_float4(o[0], o[1], o[2], o[3]);
                q[1] = make_float4(o[4], o[5], o[6], o[7]);
                q[2] = make_float4(o[8], o[9], o[10], o[11]);
            }
        } else {
            if (depth) depth[base + p] = z[0];
            if (xyz) {
                float *q = xyz + (base + p) * 3;
                q[0] = o[0];
                q[1] = o[1];
                q[2] = o[2];
            }
        }
    }
    if (count) lr_count(count + blockIdx.y, cnt);
}

// The pixels of a tile in the order of the records: iteration j (0 .. 3) of lane t (0 .. 255) is pixel
// tile * 1024 + 256 j + t, so the order is (j, wave, lane).  -> kept; (X, Y, Z) and the pixel's number where kept.
template <typename T>
__device__ __forceinline__ bool cloud_pixel(const T *__restrict__ map, const RpjQ &Q, float z_min, float z_max, int W,
                                            unsigned npx, int j, unsigned &p, float &X, float &Y, float &Z)
{
    p = blockIdx.x * (unsigned)SM_CLOUD_TILE + j * 256u + threadIdx.x;
    const bool in = p < npx;
    const T v = in ? map[(size_t)blockIdx.y * npx + p] : (T)0;
    const unsigned row = p / (unsigned)W;
    return rpj_pixel(Q, (int)(p - row * (unsigned)W), (int)row, rpj_disparity<T>(v), v != 0, z_min, z_max, X, Y, Z);
}

// Grid: x = tile, y = pair.  counts: [pair][tiles].  Every tile's count is stored (a plain store, no atomic).
template <typename T>
__global__ __launch_bounds__(256) void k_cloud_count(const T *__restrict__ map, RpjQ Q, float z_min, float z_max,
                                                     i32 *__restrict__ counts, int W, unsigned npx)
{
    __shared__ int part[4];
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < SM_CLOUD_TILE / 256; j++) {
        unsigned p;
        float X, Y, Z;
        cnt += cloud_pixel<T>(map, Q, z_min, z_max, W, npx, j, p, X, Y, Z);
    }
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) counts[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// One workgroup per pair: counts[pair][0 .. tiles) -> their exclusive prefix sums, in place, SM_CLOUD_SCAN tiles a
// turn with the sum of the turns before carried along; total[pair] = the sum of all.
__global__ __launch_bounds__(SM_CLOUD_SCAN) void k_cloud_scan(i32 *__restrict__ counts, unsigned tiles, i32 *__restrict__ total)
{
    __shared__ int wsum[SM_CLOUD_SCAN / 64];
    i32 *c = counts + (size_t)blockIdx.x * tiles;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (unsigned first = 0; first < tiles; first += SM_CLOUD_SCAN) {
        const unsigned i = first + threadIdx.x;
        const int v = i < tiles ? c[i] : 0;
        int s = v;                                       // inclusive sum over the wave
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(s, off);
            if (lane >= off) s += t;
        }
        if (lane == 63) wsum[wave] = s;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < SM_CLOUD_SCAN / 64; k++) {
            before += k < wave ? wsum[k] : 0;
            all += wsum[k];
        }
        if (i < tiles) c[i] = carry + before + s - v;
        carry += all;
        __syncthreads();                                 // wsum is rewritten by the next turn
    }
    if (threadIdx.x == 0) total[blockIdx.x] = carry;
}

// Grid: x = tile, y = pair.  offsets: k_cloud_scan's.  VEC: d_points is 16-byte aligned (one 16-byte store a record).
template <typename T>
__global__ __launch_bounds__(256) void k_cloud_write(const T *__restrict__ map, const u8 *__restrict__ gray, RpjQ Q,
                                                     float z_min, float z_max, const i32 *__restrict__ offsets,
                                                     float *__restrict__ points, i32 *__restrict__ index, int capacity,
                                                     int vec, int W, unsigned npx)
{
    constexpr int J = SM_CLOUD_TILE / 256;
    __shared__ int wc[J * 4];                            // kept pixels of (iteration, wave), in the records' order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned p[J];
    float X[J], Y[J], Z[J], I[J];
    bool kept[J];
    int rank[J];
#pragma unroll
    for (int j = 0; j < J; j++) {
        kept[j] = cloud_pixel<T>(map, Q, z_min, z_max, W, npx, j, p[j], X[j], Y[j], Z[j]);
        I[j] = gray && kept[j] ? (float)gray[(size_t)blockIdx.y * npx + p[j]] : 0.0f;
        const unsigned long long b = __ballot(kept[j]);
        rank[j] = (int)__builtin_amdgcn_mbcnt_hi((u32)(b >> 32), __builtin_amdgcn_mbcnt_lo((u32)b, 0u));
        if (lane == 0) wc[j * 4 + wave] = __popcll(b);
    }
    __syncthreads();
    int acc = offsets[(size_t)blockIdx.y * gridDim.x + blockIdx.x], start[J] = {};
#pragma unroll
    for (int e = 0; e < J * 4; e++) {
#pragma unroll
        for (int j = 0; j < J; j++)
            if (e == j * 4 + wave) start[j] = acc;
        acc += wc[e];
    }
    const size_t slot0 = (size_t)blockIdx.y * (size_t)capacity;
#pragma unroll
    for (int j = 0; j < J; j++) {
        const int k = start[j] + rank[j];
        if (!kept[j] || k >= capacity) continue;
        float *r = points + (slot0 + k) * 4;
        if (vec) {
            *(float4 *)r = make_float4(X[j], Y[j], Z[j], I[j]);
        } else {
            r[0] = X[j];
            r[1] = Y[j];
            r[2] = Z[j];
            r[3] = I[j];
        }
        if (index) index[slot0 + k] = (i32)p[j];
    }
}


// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

static unsigned rpj_tiles(const sm_plan *plan)
{
    return (unsigned)(((long long)plan->width * plan->height + SM_CLOUD_TILE - 1) / SM_CLOUD_TILE);
}

// SM_WS_CLOUD (sm_api.hip's table): one int32 per tile and pair slot
size_t sm_cloud_bytes(const sm_plan *plan) { return (size_t)plan->max_pairs * rpj_tiles(plan) * sizeof(i32); }

// what sm_reproject and sm_point_cloud check alike, before the plan is looked at
static int rpj_check_common(const void *d_map, int map_type, const double *q, float z_min, float z_max, const char *me,
                            size_t *elem)
{
    if (!d_map) return sm_fail(SM_ERR_ARG, "%s: a map pointer is NULL", me);
    SM_TRY(sm_check_map_type(map_type, me, elem));
    if (!q) return sm_fail(SM_ERR_ARG, "%s: q is NULL", me);
    for (int i = 0; i < 16; i++)
        if (!std::isfinite(q[i])) return sm_fail(SM_ERR_ARG, "%s: q[%d] = %g is not finite", me, i, q[i]);
    if (std::isnan(z_min) || std::isnan(z_max)) return sm_fail(SM_ERR_ARG, "%s: a bound of the z range is NaN", me);
    if (z_min > z_max) return sm_fail(SM_ERR_ARG, "%s: z_min %g is above z_max %g", me, (double)z_min, (double)z_max);
    if ((uintptr_t)d_map & (*elem - 1))
        return sm_fail(SM_ERR_ARG, "%s: the map pointer is not aligned to its %zu-byte elements", me, *elem);
    return SM_OK;
}

// the pixel number y W + x is an int32 (d_index, and the kernels' unsigned arithmetic on 4 * it)
static int rpj_plan_size(const sm_plan *plan, const char *me)
{
    if ((long long)plan->width * plan->height > (1ll << 30))
        return sm_fail(SM_ERR_ARG, "%s: built for images of up to 2^30 pixels (got %dx%d)", me, plan->width, plan->height);
    return SM_OK;
}

struct RpjRange {
    const void *p;
    size_t bytes;
};

// does an output share a byte with the input map, d_gray or another output?  (ins / outs: NULL or empty = absent)
static int rpj_check_ranges(const RpjRange *ins, int n_in, const RpjRange *outs, int n_out, const char *me)
{
    for (int i = 0; i < n_out; i++) {
        if (!outs[i].p || !outs[i].bytes) continue;
        for (int j = 0; j < n_in; j++)
            if (ins[j].p && ins[j].bytes && overlap(outs[i].p, ins[j].p, outs[i].bytes, ins[j].bytes))
                return sm_fail(SM_ERR_ARG, "%s: an output overlaps an input", me);
        for (int j = 0; j < i; j++)
            if (outs[j].p && outs[j].bytes && overlap(outs[i].p, outs[j].p, outs[i].bytes, outs[j].bytes))
                return sm_fail(SM_ERR_ARG, "%s: outputs overlap", me);
    }
    return SM_OK;
}

extern "C" int sm_reproject(sm_plan *plan, const void *d_map, int map_type, const double *q, float z_min, float z_max,
                            float missing, int pairs, float *d_depth, float *d_xyz, int32_t *d_count, void *stream)
{
    const char *me = "sm_reproject";
    size_t elem;
    SM_TRY(rpj_check_common(d_map, map_type, q, z_min, z_max, me, &elem));
    if (!d_depth && !d_xyz) return sm_fail(SM_ERR_ARG, "%s: d_depth and d_xyz are both NULL", me);
    if ((((uintptr_t)d_depth | (uintptr_t)d_xyz | (uintptr_t)d_count) & 3) != 0)
        return sm_fail(SM_ERR_ARG, "%s: an output pointer is not aligned to its 4-byte elements", me);
    // an output that IS the input or another output overlaps it whatever the sizes are (the ranges follow, with the plan)
    const RpjRange in1 = {d_map, 1}, out1[3] = {{d_depth, 1}, {d_xyz, 1}, {d_count, 1}};
    SM_TRY(rpj_check_ranges(&in1, 1, out1, 3, me));
    SM_TRY(sm_check_pairs(plan, pairs, me));
    SM_TRY(rpj_plan_size(plan, me));
    const int W = plan->width;
    const unsigned npx = (unsigned)W * plan->height;
    const size_t n = (size_t)pairs * npx;
    const RpjRange in = {d_map, n * elem};
    const RpjRange outs[3] = {{d_depth, n * sizeof(float)}, {d_xyz, 3 * n * sizeof(float)}, {d_count, pairs * sizeof(i32)}};
    SM_TRY(rpj_check_ranges(&in, 1, outs, 3, me));
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    RpjQ Q;
    for (int i = 0; i < 16; i++) Q.q[i] = q[i];
    if (d_count) SM_TRY(sm_lr_zero_counts(d_count, pairs, st));
    const bool vec = W % 4 == 0 && ((uintptr_t)d_map & (4 * elem - 1)) == 0 && (((uintptr_t)d_depth | (uintptr_t)d_xyz) & 15) == 0;
    const unsigned lanes = vec ? npx / 4 : npx;
    const dim3 grid(std::min((lanes + 255) / 256, (unsigned)SM_LR_BLOCKS), pairs), block(256);
#define SM_RPJ_GO(T, V) hipLaunchKernelGGL((k_reproject<T, V>), grid, block, 0, st, (const T *)d_map, Q, z_min, z_max, missing, \
                                           d_depth, d_xyz, d_count, W, npx)
    if (map_type == SM_MAP_I32) { if (vec) SM_RPJ_GO(i32, 4); else SM_RPJ_GO(i32, 1); }
    else                        { if (vec) SM_RPJ_GO(int16_t, 4); else SM_RPJ_GO(int16_t, 1); }
#undef SM_RPJ_GO
    SM_LAUNCH_CHECK("k_reproject");
    return SM_OK;
}

extern "C" int sm_plan_reserve_cloud(sm_plan *plan)
{
    if (!plan) return sm_fail(SM_ERR_ARG, "sm_plan_reserve_cloud: plan is NULL");
    SM_TRY(sm_use_device(plan->device));
    return sm_ws_reserve(plan, SM_WS_SET_CLOUD, "sm_plan_reserve_cloud");
}

template <typename T>
static int cloud_launch(const sm_plan *plan, const T *map, const RpjQ &Q, float z_min, float z_max, const u8 *gray, int pairs,
                        int capacity, float *points, i32 *index, i32 *count, hipStream_t st)
{
    const int W = plan->width;
    const unsigned npx = (unsigned)W * plan->height, tiles = rpj_tiles(plan);
    // (a batch of `pairs` uses the first pairs * tiles counts: the stride of a pair is the launch's tile count)
    const dim3 grid(tiles, pairs), block(256);
    hipLaunchKernelGGL(k_cloud_count<T>, grid, block, 0, st, map, Q, z_min, z_max, plan->d_cloud, W, npx);
    SM_LAUNCH_CHECK("k_cloud_count");
    hipLaunchKernelGGL(k_cloud_scan, dim3(pairs), dim3(SM_CLOUD_SCAN), 0, st, plan->d_cloud, tiles, count);
    SM_LAUNCH_CHECK("k_cloud_scan");
    if (capacity > 0) {
        hipLaunchKernelGGL(k_cloud_write<T>, grid, block, 0, st, map, gray, Q, z_min, z_max, (const i32 *)plan->d_cloud, points,
                           index, capacity, ((uintptr_t)points & 15) == 0 ? 1 : 0, W, npx);
        SM_LAUNCH_CHECK("k_cloud_write");
    }
    return SM_OK;
}

extern "C" int sm_point_cloud(sm_plan *plan, const void *d_map, int map_type, const double *q, float z_min, float z_max,
                              const uint8_t *d_gray, int pairs, int capacity, float *d_points, int32_t *d_index,
                              int32_t *d_count, void *stream)
{
    const char *me = "sm_point_cloud";
    size_t elem;
    SM_TRY(rpj_check_common(d_map, map_type, q, z_min, z_max, me, &elem));
    if (capacity < 0) return sm_fail(SM_ERR_ARG, "%s: capacity %d is negative", me, capacity);
    if (!d_points && capacity > 0)
        return sm_fail(SM_ERR_ARG, "%s: d_points is NULL and capacity is %d (a count-only call has capacity 0)", me, capacity);
    if (!d_count) return sm_fail(SM_ERR_ARG, "%s: d_count is NULL", me);
    if ((((uintptr_t)d_points | (uintptr_t)d_index | (uintptr_t)d_count) & 3) != 0)
        return sm_fail(SM_ERR_ARG, "%s: an output pointer is not aligned to its 4-byte elements", me);
    const RpjRange in1[2] = {{d_map, 1}, {d_gray, 1}}, out1[3] = {{d_points, 1}, {d_index, 1}, {d_count, 1}};
    SM_TRY(rpj_check_ranges(in1, 2, out1, 3, me));
    SM_TRY(sm_check_pairs(plan, pairs, me));
    SM_TRY(rpj_plan_size(plan, me));
    const size_t n = (size_t)pairs * plan->width * plan->height, slots = (size_t)pairs * capacity;
    const RpjRange ins[2] = {{d_map, n * elem}, {d_gray, n}};
    const RpjRange outs[3] = {{d_points, 4 * slots * sizeof(float)}, {d_index, slots * sizeof(i32)}, {d_count, pairs * sizeof(i32)}};
    SM_TRY(rpj_check_ranges(ins, 2, outs, 3, me));
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    SM_TRY(sm_ws_need(plan, SM_WS_SET_CLOUD, st, me));
    RpjQ Q;
    for (int i = 0; i < 16; i++) Q.q[i] = q[i];
    if (map_type == SM_MAP_I32)
        return cloud_launch<i32>(plan, (const i32 *)d_map, Q, z_min, z_max, d_gray, pairs, capacity, d_points, d_index, d_count, st);
    return cloud_launch<int16_t>(plan, (const int16_t *)d_map, Q, z_min, z_max, d_gray, pairs, capacity, d_points, d_index,
                                 d_count, st);
}

// host only: the matrix of a rectified rig (the order of the operations is the header's)
extern "C" int sm_reproject_q(const sm_rectify_calib *first, const sm_rectify_calib *second, double baseline, double q[16])
{
    const char *me = "sm_reproject_q";
    if (!first || !second) return sm_fail(SM_ERR_ARG, "%s: calib is NULL", me);
    if (!q) return sm_fail(SM_ERR_ARG, "%s: q is NULL", me);
    for (const sm_rectify_calib *c : {first, second})
        if (c->struct_size < (int)sizeof(sm_rectify_calib))
            return sm_fail(SM_ERR_ARG, "%s: calib->struct_size %d is not that of a sm_rectify_calib (this library: %d bytes)", me,
                           c->struct_size, (int)sizeof(sm_rectify_calib));
    if (!std::isfinite(baseline) || baseline == 0.0)
        return sm_fail(SM_ERR_ARG, "%s: baseline %g is zero or not finite", me, baseline);
    if (!(std::isfinite(first->new_fx) && first->new_fx > 0.0 && std::isfinite(first->new_fy) && first->new_fy > 0.0))
        return sm_fail(SM_ERR_ARG, "%s: new_fx %g / new_fy %g of the first calibration are not positive and finite", me,
                       first->new_fx, first->new_fy);
    const double f = first->new_fx, t = baseline;
    const double r = f / first->new_fy;
    for (int i = 0; i < 16; i++) q[i] = 0.0;
    q[0] = 1.0;
    q[3] = -first->new_cx;
    q[5] = r;
    q[7] = -(first->new_cy * r);
    q[11] = f;
    q[14] = 1.0 / t;
    q[15] = -((second->new_cx - first->new_cx) / t);
    return SM_OK;
}
