// sm_filter.hip -- disparity post-filters on the maps the library produces: a validity-aware median and speckle
// removal (include/stereo_hip.h), and the two masks
// that carry validity from one map to another (sm_sub_mask, sm_valid_mask).  The per-pair counts of the consistency
// check are reused (lr_count of sm_device.h; k_lr_zero_counts through sm_lr_zero_counts).
//
// PARITY UNPINNED: the reference has no such stage.  Definition (tests/filter_reference.py is its executable form).
// Maps are [pairs][H][W] of int32 (a web map) or int16 (a sub map); a pixel is valid iff its value != 0; a tap
// outside the image does not exist, in either border mode; pairs are independent.
//   median, k in {3, 5}: out(p) = 0 where in(p) = 0; else the lower median v[(m - 1) / 2] of the m valid values
//     v[0] <= ... <= v[m - 1] of the k x k window around p (signed order).
//   speckle removal (max_size, max_diff >= 0): the valid pixels are a graph, two 4-neighbours joined iff
//     |in(a) - in(b)| <= max_diff; out(p) = in(p) if p is valid and its component has more than max_size pixels,
//     else 0; removed = the valid pixels set to 0, per pair.
//
// Kernels:
//   k_median<T, K>   a 64 x 16 tile with its halo staged in LDS as int32, 0 for a tap outside the image (a missing tap
//                    and an invalid one are treated alike).  A lane owns a column of the tile and four of its rows.
//                    The variable rank costs no full sort of a variable count: of the k^2 - m missing taps the first
//                    (k^2 - 1) / 2 - (m - 1) / 2 become INT_MIN and the rest INT_MAX, after which the element at rank
//                    (k^2 - 1) / 2 of all k^2 is v[(m - 1) / 2].  The rank is taken by Batcher's merge-exchange
//                    network, generated at compile time and fully unrolled; the compiler drops the exchanges
//                    the middle output does not depend on.
//   k_spk_local<T>   union-find over one 64 x 16 tile in LDS (links to the left, a compression, links upwards), then
//                    every pixel's label = the pair-relative index of its tile-local root (-1: invalid); sizes zeroed.
//   k_spk_merge<T>   one lane per pixel pair across a tile border: union on the global labels.  Labels are touched by
//                    agent-scope atomics only (a plain store is not seen across XCDs inside a launch).
//   k_spk_count      every pixel finds its root, stores it as its label and counts itself there: one atomic add per
//                    wave and root (lanes that agree are counted by a ballot).
//   k_spk_apply<T>   out = in where the root's size > max_size, else 0; the removed pixels counted per pair.
// The phases are separate launches: a kernel boundary makes the labels of one phase visible to the next.  Every loop
// terminates on every input: a label only ever decreases (it is replaced by the label of an ancestor, or by a smaller
// root), a find follows strictly decreasing labels, and a union retries only when its compare-and-swap (an atomic
// min whose old value is not the root it meant to link) lost to a smaller label.


#include "sm_device.h"

#include <algorithm>

// ---------------------------------------------------------------------------
// median (the exchange network, flt_sort, is in sm_device.h: the interpolation sorts its candidates with it)
// ---------------------------------------------------------------------------

// the lower median of the non-zero entries of v (at least one); v is consumed
template <int N>
__host__ __device__ __forceinline__ i32 flt_valid_median(i32 (&v)[N])
{
    int m = 0;
#pragma unroll
    for (int j = 0; j < N; j++) m += v[j] != 0;
    const int lows = (N - 1) / 2 - (m - 1) / 2;
    int miss = 0;
#pragma unroll
    for (int j = 0; j < N; j++) {
        const bool gone = v[j] == 0;
        v[j] = gone ? (miss < lows ? (i32)0x80000000 : (i32)0x7fffffff) : v[j];
        miss += gone;
    }
    flt_sort<N>(v);
    return v[(N - 1) / 2];
}

// grid (ceil(W / 64), ceil(H / 16), pairs), block 256
template <typename T, int K>
__global__ __launch_bounds__(256) void k_median(const T *__restrict__ in, T *__restrict__ out, int W, int H)
{
    constexpr int R = K / 2, SW = FLT_TW + 2 * R, SH = FLT_TH + 2 * R, N = K * K;
    __shared__ i32 tile[SH * SW];
    const int tx0 = blockIdx.x * FLT_TW, ty0 = blockIdx.y * FLT_TH;
    const size_t base = (size_t)blockIdx.z * W * H;
    for (int i = threadIdx.x; i < SH * SW; i += 256) {
        const int sy = i / SW, sx = i - sy * SW;
        const int gx = tx0 + sx - R, gy = ty0 + sy - R;
        tile[i] = gx >= 0 && gx < W && gy >= 0 && gy < H ? (i32)in[base + (size_t)gy * W + gx] : 0;
    }
    __syncthreads();
    const int lx = threadIdx.x & 63, gx = tx0 + lx;
    if (gx >= W) return;
    for (int ly = threadIdx.x >> 6; ly < FLT_TH; ly += 4) {
        const int gy = ty0 + ly;
        if (gy >= H) break;
        i32 v[N];
#pragma unroll
        for (int dy = 0; dy < K; dy++)
#pragma unroll
            for (int dx = 0; dx < K; dx++) v[dy * K + dx] = tile[(ly + dy) * SW + lx + dx];
        const i32 c = v[R * K + R];
        const i32 med = flt_valid_median<N>(v);
        out[base + (size_t)gy * W + gx] = c == 0 ? (T)0 : (T)med;
    }
}

// ---------------------------------------------------------------------------
// speckle removal
// ---------------------------------------------------------------------------

// are two valid 4-neighbours joined?  (64-bit: the difference of two int32 need not be one)
__device__ __forceinline__ bool spk_joined(i32 a, i32 b, int max_diff)
{
    const long long d = (long long)a - b;
    return (d < 0 ? -d : d) <= max_diff;
}

// union-find on labels in LDS: lab[x] <= x, a root has lab[x] == x
__device__ __forceinline__ int spk_find_lds(int *lab, int x)
{
    int p;
    while ((p = __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != x) x = p;
    return x;
}

__device__ __forceinline__ void spk_union_lds(int *lab, int a, int b)
{
    for (;;) {
        a = spk_find_lds(lab, a);
        b = spk_find_lds(lab, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        // a was a root: link it below b.  old != a: another lane linked it first (to old < a); the min keeps a
        // below both, and the pair (old, b) is what remains to be joined
        const int old = __hip_atomic_fetch_min(lab + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == a) return;
        a = old;
    }
}

// grid (ceil(W / 64), ceil(H / 16), pairs), block 256: lane t owns tile pixels t, t + 256, t + 512, t + 768
template <typename T>
__global__ __launch_bounds__(256) void k_spk_local(const T *__restrict__ in, i32 *__restrict__ labels,
                                                   i32 *__restrict__ sizes, int W, int H, int max_diff)
{
    __shared__ i32 val[FLT_PX];
    __shared__ int lab[FLT_PX];
    const int tx0 = blockIdx.x * FLT_TW, ty0 = blockIdx.y * FLT_TH;
    const size_t base = (size_t)blockIdx.z * W * H;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int i = threadIdx.x + 256 * r, gx = tx0 + (i & 63), gy = ty0 + (i >> 6);
        val[i] = gx < W && gy < H ? (i32)in[base + (size_t)gy * W + gx] : 0;
        lab[i] = i;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int i = threadIdx.x + 256 * r;
        const i32 v = val[i];
        if (v != 0 && (i & 63) > 0) {
            const i32 u = val[i - 1];
            if (u != 0 && spk_joined(v, u, max_diff)) spk_union_lds(lab, i, i - 1);
        }
    }
    __syncthreads();
    // (a row's links form chains: shorten them before the links upwards walk them)
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int i = threadIdx.x + 256 * r;
        __hip_atomic_fetch_min(lab + i, spk_find_lds(lab, i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int i = threadIdx.x + 256 * r;
        const i32 v = val[i];
        if (v != 0 && i >= FLT_TW) {
            const i32 u = val[i - FLT_TW];
            if (u != 0 && spk_joined(v, u, max_diff)) spk_union_lds(lab, i, i - FLT_TW);
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int i = threadIdx.x + 256 * r, gx = tx0 + (i & 63), gy = ty0 + (i >> 6);
        if (gx >= W || gy >= H) continue;
        const int root = spk_find_lds(lab, i);
        const size_t o = base + (size_t)gy * W + gx;
        labels[o] = val[i] != 0 ? (ty0 + (root >> 6)) * W + tx0 + (root & 63) : -1;
        sizes[o] = 0;
    }
}

// union-find on the global labels of one pair, inside k_spk_merge: agent-scope atomics only
__device__ __forceinline__ int spk_find(i32 *lab, int x)
{
    int p;
    while ((p = __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != x) x = p;
    return x;
}

__device__ __forceinline__ void spk_union(i32 *lab, int a, int b)
{
    for (;;) {
        a = spk_find(lab, a);
        b = spk_find(lab, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(lab + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return;
        a = old;
    }
}

// Lanes 0 .. n_h - 1: pixel x of row 16 (j + 1) against the pixel above it; lanes n_h .. n_all - 1: pixel y of column
// 64 (j + 1) against the pixel to its left.  grid (ceil(n_all / 256), pairs), block 256.
template <typename T>
__global__ __launch_bounds__(256) void k_spk_merge(const T *__restrict__ in, i32 *labels, int W, int H, int max_diff,
                                                   unsigned n_h, unsigned n_all)
{
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_all) return;
    int x, y, q;
    if (t < n_h) {
        const unsigned j = t / (unsigned)W;
        x = (int)(t - j * (unsigned)W); y = (int)(j + 1) * FLT_TH; q = W;
    } else {
        const unsigned s = t - n_h, j = s / (unsigned)H;
        y = (int)(s - j * (unsigned)H); x = (int)(j + 1) * FLT_TW; q = 1;
    }
    const size_t base = (size_t)blockIdx.y * W * H;
    const int p = y * W + x;
    const i32 a = (i32)in[base + p], b = (i32)in[base + p - q];
    if (a == 0 || b == 0 || !spk_joined(a, b, max_diff)) return;
    i32 *lab = labels + base;
    // the two tile-local roots: one step each, and what the union then walks is the tree of tile roots
    spk_union(lab, p, p - q);
}

// grid (ceil(npx / 256), pairs), block 256.  Plain loads and stores: a label read here is either the one the
// merge left or a root another lane has stored over it since, and both are ancestors of the pixel.
__global__ __launch_bounds__(256) void k_spk_count(i32 *labels, i32 *sizes, unsigned npx)
{
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    i32 *lab = labels + (size_t)blockIdx.y * npx;
    int root = -1;
    if (p < npx) {
        int l = lab[p];
        if (l >= 0) {
            root = l;
            while ((l = lab[root]) != root) root = l;
            lab[p] = root;
        }
    }
    // one add per wave and root: the first lane still to be counted names its root, the lanes that agree are counted
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(root >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int r = __shfl(root, leader);
        const unsigned long long same = __ballot(root == r);
        if (lane == leader) atomicAdd(sizes + (size_t)blockIdx.y * npx + r, (i32)__popcll(same));
        todo &= ~same;
    }
}

// grid (up to SM_LR_BLOCKS, pairs), block 256, striding over the pair's pixels.  out may be in: a lane reads a pixel
// before it writes it and touches no other.
template <typename T>
__global__ __launch_bounds__(256) void k_spk_apply(const T *in, T *out, const i32 *__restrict__ labels,
                                                   const i32 *__restrict__ sizes, i32 *removed, unsigned npx,
                                                   int max_size)
{
    const size_t base = (size_t)blockIdx.y * npx;
    int cnt = 0;
    for (unsigned t = blockIdx.x * 256u + threadIdx.x; t < npx; t += gridDim.x * 256u) {
        const T v = in[base + t];
        bool keep = false;
        if (v != 0) {
            keep = sizes[base + labels[base + t]] > max_size;
            cnt += !keep;
        }
        out[base + t] = keep ? v : (T)0;
    }
    if (removed) lr_count(removed + blockIdx.y, cnt);
}

// ---------------------------------------------------------------------------
// masks
// ---------------------------------------------------------------------------

// sub = 0 where the checked map is 0
__global__ __launch_bounds__(256) void k_sgm_sub_mask(const i32 *__restrict__ web, int16_t *__restrict__ sub, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n && web[i] == 0) sub[i] = 0;
}

// map = 0 where valid = 0, in place, one element per lane over all pairs
template <typename T>
__global__ __launch_bounds__(256) void k_valid_mask(T *map, const u8 *__restrict__ valid, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n && valid[i] == 0) map[i] = 0;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

extern "C" int sm_median_filter(sm_plan *plan, const void *d_in, int map_type, int k, int pairs, void *d_out, void *stream)
{
    const char *me = "sm_median_filter";
    size_t elem;
    if (!d_in || !d_out) return sm_fail(SM_ERR_ARG, "%s: a map pointer is NULL", me);
    SM_TRY(sm_check_map_type(map_type, me, &elem));
    if (k != 3 && k != 5) return sm_fail(SM_ERR_ARG, "%s: k %d is not 3 or 5", me, k);
    SM_TRY(sm_check_pairs(plan, pairs, me));
    const int W = plan->width, H = plan->height;
    if (overlap(d_in, d_out, (size_t)pairs * W * H * elem))
        return sm_fail(SM_ERR_ARG, "%s: maps overlap (every output pixel reads its neighbours' inputs)", me);
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((W + FLT_TW - 1) / FLT_TW, (H + FLT_TH - 1) / FLT_TH, pairs), block(256);
#define SM_MED_GO(T, K) hipLaunchKernelGGL((k_median<T, K>), grid, block, 0, st, (const T *)d_in, (T *)d_out, W, H)
    if (map_type == SM_MAP_I32) { if (k == 3) SM_MED_GO(i32, 3); else SM_MED_GO(i32, 5); }
    else                        { if (k == 3) SM_MED_GO(int16_t, 3); else SM_MED_GO(int16_t, 5); }
#undef SM_MED_GO
    SM_LAUNCH_CHECK("k_median");
    return SM_OK;
}

extern "C" int sm_plan_reserve_filter(sm_plan *plan)
{
    if (!plan) return sm_fail(SM_ERR_ARG, "sm_plan_reserve_filter: plan is NULL");
    SM_TRY(sm_use_device(plan->device));
    return sm_ws_reserve(plan, SM_WS_SET_FILTER, "sm_plan_reserve_filter");
}

template <typename T>
static int speckle_launch(const sm_plan *plan, const T *in, T *out, int max_size, int max_diff, int pairs, i32 *removed,
                          hipStream_t st)
{
    const int W = plan->width, H = plan->height;
    const unsigned npx = (unsigned)W * H;
    i32 *labels = plan->d_filter, *sizes = plan->d_filter + (size_t)plan->max_pairs * npx;
    const unsigned tiles_x = (W + FLT_TW - 1) / FLT_TW, tiles_y = (H + FLT_TH - 1) / FLT_TH;
    if (removed) SM_TRY(sm_lr_zero_counts(removed, pairs, st));
    hipLaunchKernelGGL(k_spk_local<T>, dim3(tiles_x, tiles_y, pairs), dim3(256), 0, st, in, labels, sizes, W, H, max_diff);
    SM_LAUNCH_CHECK("k_spk_local");
    const unsigned n_h = (tiles_y - 1) * (unsigned)W, n_all = n_h + (tiles_x - 1) * (unsigned)H;
    if (n_all) {
        hipLaunchKernelGGL(k_spk_merge<T>, dim3((n_all + 255) / 256, pairs), dim3(256), 0, st, in, labels, W, H, max_diff,
                           n_h, n_all);
        SM_LAUNCH_CHECK("k_spk_merge");
    }
    hipLaunchKernelGGL(k_spk_count, dim3((npx + 255) / 256, pairs), dim3(256), 0, st, labels, sizes, npx);
    SM_LAUNCH_CHECK("k_spk_count");
    hipLaunchKernelGGL(k_spk_apply<T>, dim3(std::min((npx + 255) / 256, (unsigned)SM_LR_BLOCKS), pairs), dim3(256), 0, st,
                       in, out, labels, sizes, removed, npx, max_size);
    SM_LAUNCH_CHECK("k_spk_apply");
    return SM_OK;
}

extern "C" int sm_speckle_filter(sm_plan *plan, const void *d_in, int map_type, int max_size, int max_diff, int pairs,
                                 void *d_out, int32_t *d_removed, void *stream)
{
    const char *me = "sm_speckle_filter";
    size_t elem;
    if (!d_in || !d_out) return sm_fail(SM_ERR_ARG, "%s: a map pointer is NULL", me);
    SM_TRY(sm_check_map_type(map_type, me, &elem));
    if (max_size < 0) return sm_fail(SM_ERR_ARG, "%s: max_size %d is negative", me, max_size);
    if (max_diff < 0) return sm_fail(SM_ERR_ARG, "%s: max_diff %d is negative", me, max_diff);
    SM_TRY(sm_check_pairs(plan, pairs, me));
    const size_t map = (size_t)pairs * plan->width * plan->height * elem;
    if (d_in != d_out && overlap(d_in, d_out, map))
        return sm_fail(SM_ERR_ARG, "%s: maps overlap without d_out being d_in", me);
    const size_t counts = (size_t)pairs * sizeof(i32);
    if (d_removed && (overlap(d_removed, d_in, counts, map) || overlap(d_removed, d_out, counts, map)))
        return sm_fail(SM_ERR_ARG, "%s: d_removed overlaps a map", me);
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    SM_TRY(sm_ws_need(plan, SM_WS_SET_FILTER, st, me));
    if (map_type == SM_MAP_I32)
        return speckle_launch<i32>(plan, (const i32 *)d_in, (i32 *)d_out, max_size, max_diff, pairs, d_removed, st);
    return speckle_launch<int16_t>(plan, (const int16_t *)d_in, (int16_t *)d_out, max_size, max_diff, pairs, d_removed, st);
}

// k_sgm_sub_mask over n elements: sm_sub_mask below, and sm_sgm_lr (sm_sgm.hip) behind its check
int sm_sub_mask_launch(const i32 *web, int16_t *sub, long long n, hipStream_t st)
{
    void *args[] = {(void *)&web, (void *)&sub, (void *)&n};
    const hipError_t e = hipLaunchKernel((const void *)k_sgm_sub_mask, dim3((unsigned)((n + 255) / 256)), dim3(256), args,
                                         0, st);
    if (e != hipSuccess) return sm_fail(SM_ERR_HIP, "launch of k_sgm_sub_mask failed: %s", hipGetErrorString(e));
    return SM_OK;
}

// sub = 0 where web = 0, for maps of the caller's: k_sgm_sub_mask as sm_sgm_lr launches it (a sub map follows a web map
// that sm_speckle_filter has thinned)
extern "C" int sm_sub_mask(sm_plan *plan, const int32_t *d_web, int16_t *d_sub, int pairs, void *stream)
{
    const char *me = "sm_sub_mask";
    if (!d_web || !d_sub) return sm_fail(SM_ERR_ARG, "%s: a map pointer is NULL", me);
    SM_TRY(sm_check_pairs(plan, pairs, me));
    const size_t map = (size_t)pairs * plan->width * plan->height * sizeof(i32);
    if (overlap(d_sub, d_web, map / 2, map)) return sm_fail(SM_ERR_ARG, "%s: maps overlap", me);
    SM_TRY(sm_use_device(plan->device));
    return sm_sub_mask_launch(d_web, d_sub, (long long)pairs * plan->width * plan->height, (hipStream_t)stream);
}

// map = 0 where valid = 0 (the validity sm_rectify writes, carried to a disparity map)
extern "C" int sm_valid_mask(sm_plan *plan, void *d_map, int map_type, const uint8_t *d_valid, int pairs, void *stream)
{
    const char *me = "sm_valid_mask";
    size_t elem;
    if (!d_map) return sm_fail(SM_ERR_ARG, "%s: a map pointer is NULL", me);
    if (!d_valid) return sm_fail(SM_ERR_ARG, "%s: d_valid is NULL", me);
    SM_TRY(sm_check_map_type(map_type, me, &elem));
    if ((const void *)d_valid == d_map) return sm_fail(SM_ERR_ARG, "%s: d_valid overlaps the map", me);
    SM_TRY(sm_check_pairs(plan, pairs, me));
    const size_t n = (size_t)pairs * plan->width * plan->height;
    if (overlap(d_valid, d_map, n, n * elem)) return sm_fail(SM_ERR_ARG, "%s: d_valid overlaps the map", me);
    SM_TRY(sm_use_device(plan->device));
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (map_type == SM_MAP_I32) hipLaunchKernelGGL(k_valid_mask<i32>, grid, block, 0, (hipStream_t)stream, (i32 *)d_map, d_valid, n);
    else hipLaunchKernelGGL(k_valid_mask<int16_t>, grid, block, 0, (hipStream_t)stream, (int16_t *)d_map, d_valid, n);
    SM_LAUNCH_CHECK("k_valid_mask");
    return SM_OK;
}
