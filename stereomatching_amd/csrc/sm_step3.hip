// sm_step3.hip -- step 3 (include/stereo_hip.h): hole filling, min / max and the contour map,
// one entry point each and sm_step3 for all three behind one synchronisation, and sm_plan_status.

#include "sm_internal.h"

#include <limits.h>

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------

// the sweep of src/stereo.cu:235-245: read `oth`, write `cur` where oth == 0.
// Neighbours at flat offsets +-1, +-w (the reference's unwrapped IDX); offsets
// that leave the image array are undefined in the reference and read as 0 here
// (SURVEY.md section 8f).
__global__ __launch_bounds__(256) void k_fill_holes_step(i32 *__restrict__ cur,
                                                         const i32 *__restrict__ oth, int w,
                                                         long long n)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const size_t base = (size_t)blockIdx.y * n;
    if (oth[base + p] == 0) {
        const i32 r = p + 1 < n ? oth[base + p + 1] : 0;
        const i32 u = p + w < n ? oth[base + p + w] : 0;
        const i32 l = p - 1 >= 0 ? oth[base + p - 1] : 0;
        const i32 d = p - w >= 0 ? oth[base + p - w] : 0;
        cur[base + p] = (r + u + l + d) / 4;
    }
}

__global__ void k_count_zeros(const i32 *__restrict__ a, long long total, i32 *__restrict__ flag)
{
    bool z = false;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < total;
         p += (long long)gridDim.x * blockDim.x)
        z |= a[p] == 0;
    if (__ballot(z) != 0 && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// min / max of each pair's image AND "some pixel is 0" (the hole-fill stage only ever
// changes pixels that are 0), in one pass over the maps.  HBM-bound: 16-byte loads where
// the image allows, one atomic pair per WORKGROUP (atomics on one address serialise at
// ~12 ns each: one pair per wave of a 2048-block grid cost 190 us at 4K)
__global__ __launch_bounds__(256) void k_minmax_zero(const i32 *__restrict__ a, long long n,
                                                     i32 *__restrict__ mm, i32 *__restrict__ zero_flag)
{
    __shared__ i32 s_lo[4], s_hi[4], s_z[4];
    const i32 *img = a + (size_t)blockIdx.y * n;
    i32 lo = INT_MAX, hi = INT_MIN;
    bool z = false;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    long long done = 0;
    if ((((uintptr_t)img) & 15) == 0) {
        typedef int v4i_ __attribute__((ext_vector_type(4)));
        const v4i_ *q = reinterpret_cast<const v4i_ *>(img);
        const long long nq = n >> 2;
        for (long long p = tid; p < nq; p += stride) {
            const v4i_ v = q[p];
            lo = min(min(lo, v.x), min(v.y, min(v.z, v.w)));
            hi = max(max(hi, v.x), max(v.y, max(v.z, v.w)));
            z |= v.x == 0 || v.y == 0 || v.z == 0 || v.w == 0;
        }
        done = nq << 2;
    }
    for (long long p = done + tid; p < n; p += stride) {
        const i32 v = img[p];
        lo = min(lo, v);
        hi = max(hi, v);
        z |= v == 0;
    }
    for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, __shfl_xor(lo, off));
        hi = max(hi, __shfl_xor(hi, off));
    }
    const bool any_z = __ballot(z) != 0;
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_lo[wv] = lo; s_hi[wv] = hi; s_z[wv] = any_z; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int nw = blockDim.x >> 6;
        bool zz = false;
        for (int k = 0; k < nw; k++) { lo = min(lo, s_lo[k]); hi = max(hi, s_hi[k]); zz |= s_z[k] != 0; }
        atomicMin(&mm[2 * blockIdx.y], lo);
        atomicMax(&mm[2 * blockIdx.y + 1], hi);
        if (zz && zero_flag) atomicOr(zero_flag, 1);
    }
}

// {INT_MAX, INT_MIN} per pair, and the "has a zero pixel" flag cleared
__global__ void k_step3_init(i32 *__restrict__ mm, int pairs, i32 *__restrict__ zero_flag)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < pairs) { mm[2 * i] = INT_MAX; mm[2 * i + 1] = INT_MIN; }
    if (i == 0 && zero_flag) *zero_flag = 0;
}

// src/stereo.cu:261-274
__global__ __launch_bounds__(256) void k_contour(const i32 *__restrict__ web,
                                                 const i32 *__restrict__ mm, int lines,
                                                 long long n, u8 *__restrict__ out,
                                                 i32 *__restrict__ flags)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const size_t base = (size_t)blockIdx.y * n;
    const i32 lo = mm[2 * blockIdx.y], hi = mm[2 * blockIdx.y + 1];
    const i32 interval = lines != 0 ? (hi - lo) / lines : 0;
    if (interval == 0) {
        if (p == 0) atomicOr(&flags[0], 1);
        out[base + p] = 0;
        return;
    }
    out[base + p] = (u8)(((web[base + p] - lo) % interval) == 0);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

void sm_step3_resolve_kernels(void)
{
    hipFuncAttributes fa;
    for (const void *f : {(const void *)k_fill_holes_step, (const void *)k_count_zeros, (const void *)k_step3_init,
                          (const void *)k_contour, (const void *)k_minmax_zero})
        (void)hipFuncGetAttributes(&fa, f);
}

static int run_sweeps(sm_plan *plan, i32 *d_web, i32 *d_tmp, int times, int pairs, int *result_in_tmp,
                      hipStream_t st)
{
    // tmp <- web (src/stereo.cu:328), then the reference's `times` sweeps
    // (:247-256).  Its SWAP(i32 *, web, tmp) (src/util.h:27-32) declares a local
    // named `tmp` that shadows the buffer: the macro swaps nothing, so every sweep
    // reads the untouched copy and writes the same values into web.  `times` >= 1
    // sweeps are ONE sweep over the original map, and web is the returned buffer
    // (pinned to the reference's own functions by tests/golden/step3/).
    const long long n = (long long)plan->width * plan->height;
    *result_in_tmp = 0;
    if (times <= 0) return SM_OK;
    SM_HIP(hipMemcpyAsync(d_tmp, d_web, sizeof(i32) * n * pairs, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_fill_holes_step, dim3((unsigned)((n + 255) / 256), pairs), dim3(256), 0, st, d_web,
                       d_tmp, plan->width, n);
    SM_LAUNCH_CHECK("k_fill_holes_step");
    return SM_OK;
}

extern "C" int sm_fill_web_holes(sm_plan *plan, int32_t *d_web, int32_t *d_tmp, int times,
                                 int pairs, int *result_in_tmp, void *stream)
{
    SM_TRY(sm_check_pairs(plan, pairs, "sm_fill_web_holes"));
    if (!d_web || !d_tmp || !result_in_tmp)
        return sm_fail(SM_ERR_ARG, "sm_fill_web_holes: NULL argument");
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    const long long n = (long long)plan->width * plan->height;
    *result_in_tmp = 0;
    if (times <= 0) return SM_OK;

    // The sweeps only ever change pixels that are 0.  The web the hot path
    // produces is >= 1 everywhere (a winning shift is recorded as shift+1), so
    // in the pipeline this stage is the identity; one
    // pass over the image decides that, as the reference's array_min_gpu
    // round trip does for the contour stage.
    SM_HIP(hipMemsetAsync(&plan->d_flags[1], 0, sizeof(i32), st));
    hipLaunchKernelGGL(k_count_zeros, dim3(1024), dim3(256), 0, st, d_web, n * pairs,
                       &plan->d_flags[1]);
    SM_LAUNCH_CHECK("k_count_zeros");
    i32 f[4];
    SM_TRY(sm_read_flags(plan, st, 0, f));
    if (!f[1]) return SM_OK;

    return run_sweeps(plan, d_web, d_tmp, times, pairs, result_in_tmp, st);
}

// one workgroup of 4 waves per 64 K pixels, at most 1024 of them per pair: enough loads in
// flight to stream from HBM, few enough atomics
static dim3 minmax_grid(long long n, int pairs)
{
    long long blocks = (n + 65535) / 65536;
    blocks = blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks);
    return dim3((unsigned)blocks, pairs);
}

extern "C" int sm_min_max(sm_plan *plan, const int32_t *d_image, int pairs, int32_t *d_minmax,
                          void *stream)
{
    SM_TRY(sm_check_pairs(plan, pairs, "sm_min_max"));
    if (!d_image || !d_minmax) return sm_fail(SM_ERR_ARG, "sm_min_max: NULL argument");
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    const long long n = (long long)plan->width * plan->height;
    hipLaunchKernelGGL(k_step3_init, dim3((pairs + 63) / 64), dim3(64), 0, st, d_minmax, pairs, (i32 *)nullptr);
    hipLaunchKernelGGL(k_minmax_zero, minmax_grid(n, pairs), dim3(256), 0, st, d_image, n, d_minmax,
                       (i32 *)nullptr);
    SM_LAUNCH_CHECK("k_minmax_zero");
    return SM_OK;
}

extern "C" int sm_draw_contour_map(sm_plan *plan, const int32_t *d_web, const int32_t *d_minmax,
                                   int num_lines, int pairs, uint8_t *d_out, void *stream)
{
    SM_TRY(sm_check_pairs(plan, pairs, "sm_draw_contour_map"));
    if (!d_web || !d_minmax || !d_out)
        return sm_fail(SM_ERR_ARG, "sm_draw_contour_map: NULL argument");
    SM_TRY(sm_use_device(plan->device));
    const long long n = (long long)plan->width * plan->height;
    hipLaunchKernelGGL(k_contour, dim3((unsigned)((n + 255) / 256), pairs), dim3(256), 0,
                       (hipStream_t)stream, d_web, d_minmax, num_lines, n, d_out, plan->d_flags);
    SM_LAUNCH_CHECK("k_contour");
    return SM_OK;
}

extern "C" int sm_step3(sm_plan *plan, int32_t *d_web, int32_t *d_tmp, int times, int num_lines,
                        int pairs, int32_t *d_minmax, uint8_t *d_out, int *result_in_tmp, void *stream)
{
    SM_TRY(sm_check_pairs(plan, pairs, "sm_step3"));
    if (!d_web || !d_tmp || !d_minmax || !d_out || !result_in_tmp)
        return sm_fail(SM_ERR_ARG, "sm_step3: NULL argument");
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    const long long n = (long long)plan->width * plan->height;
    *result_in_tmp = 0;
    const dim3 mm_grid = minmax_grid(n, pairs);
    const dim3 px_grid((unsigned)((n + 255) / 256), pairs);

    // Speculate that the map has no zero pixel (a web from the hot path never has: a
    // winning shift is stored as shift + 1): then hole filling is the identity, the
    // min/max pass over the unfilled map is the one the contour stage needs, and ONE
    // pass also proves the speculation.  Everything is queued before the only sync.
    hipLaunchKernelGGL(k_step3_init, dim3((pairs + 63) / 64), dim3(64), 0, st, d_minmax, pairs, &plan->d_flags[1]);
    hipLaunchKernelGGL(k_minmax_zero, mm_grid, dim3(256), 0, st, d_web, n, d_minmax, &plan->d_flags[1]);
    hipLaunchKernelGGL(k_contour, px_grid, dim3(256), 0, st, d_web, d_minmax, num_lines, n, d_out,
                       plan->d_flags);
    SM_LAUNCH_CHECK("k_contour");
    i32 f[4];
    SM_TRY(sm_read_flags(plan, st, 1, f));
    if (f[1] && times > 0) {
        // there ARE holes: do it the long way (sweeps, then min/max and contour again)
        SM_TRY(run_sweeps(plan, d_web, d_tmp, times, pairs, result_in_tmp, st));
        const i32 *filled = *result_in_tmp ? d_tmp : d_web;
        hipLaunchKernelGGL(k_step3_init, dim3((pairs + 63) / 64), dim3(64), 0, st, d_minmax, pairs, (i32 *)nullptr);
        hipLaunchKernelGGL(k_minmax_zero, mm_grid, dim3(256), 0, st, filled, n, d_minmax, (i32 *)nullptr);
        hipLaunchKernelGGL(k_contour, px_grid, dim3(256), 0, st, filled, d_minmax, num_lines, n, d_out,
                           plan->d_flags);
        SM_LAUNCH_CHECK("k_contour");
        SM_TRY(sm_read_flags(plan, st, 1, f));
    }
    if (f[0])
        return sm_fail(SM_ERR_ZERO_DIV, "contour interval is zero ((max-min)/lines == 0): the "
                       "reference divides by it");
    return SM_OK;
}

extern "C" int sm_plan_status(sm_plan *plan, void *stream)
{
    if (!plan) return sm_fail(SM_ERR_ARG, "sm_plan_status: plan is NULL");
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    i32 f[4];
    SM_TRY(sm_read_flags(plan, st, 1, f));
    if (f[0])
        return sm_fail(SM_ERR_ZERO_DIV, "contour interval is zero ((max-min)/lines == 0): the "
                       "reference divides by it");
    return SM_OK;
}
