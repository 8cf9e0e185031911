// sm_device.h -- the device-side helpers that more than one translation unit uses.  Only __forceinline__ functions
// (and what they are made of) live here: a __global__ defined in a header that two units include would be two
// kernels, so a kernel that stages share is reached through a host function of the unit that holds it
// (sm_internal.h: sm_lr_zero_counts, sm_sub_mask_launch).
#pragma once

#include "sm_internal.h"

// v mod m in 0 .. m - 1 (the toroidal border), and floor(num / den) for den > 0: census, SGM
__device__ __forceinline__ int smn_mod(int v, int m)
{
    int r = v % m;
    return r < 0 ? r + m : r;
}

__device__ __forceinline__ int smn_floordiv(int num, int den)      // den > 0
{
    const int q = num / den;
    return (num % den != 0 && num < 0) ? q - 1 : q;
}

// The workgroup's rejections, added to the pair's count with ONE atomic: a sum across each wave (DPP / shuffles),
// then across the four waves in LDS.  All atomics of a pair go to one address, where they serialise: one per
// wave of four pixels per lane cost ~11 ns each, 0.35 ms at 4K (32 K waves) -- hence workgroups that stride
// over the map (SM_LR_BLOCKS per pair) and one atomic per workgroup.  (k_lr_check, k_spk_apply, k_itp_combine)
#define SM_LR_BLOCKS 1024
__device__ __forceinline__ void lr_count(i32 *rejected, int cnt)
{
    __shared__ int part[4];
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int total = part[0] + part[1] + part[2] + part[3];
        if (total) atomicAdd(rejected, total);
    }
}

// The post-filters' tile (sm_filter.hip, sm_wmedian.hip, sm_pyramid.hip): 64 columns x 16 rows per workgroup of 256 lanes
#define FLT_TW 64
#define FLT_TH 16
#define FLT_PX (FLT_TW * FLT_TH)

// the weight table of the guided filters, passed by value in the kernel's arguments (k_wmedian, k_upsample_double)
struct WmedTable {
    uint16_t w[256];
};

static inline WmedTable wmed_table(const uint16_t weights[256])
{
    WmedTable table;
    for (int i = 0; i < 256; i++) table.w[i] = weights[i];
    return table;
}

// Batcher's merge exchange (Knuth 5.2.2 M) for N elements: the comparators in order (the median, k_itp_combine)
template <int N>
struct FltNet {
    int n;
    unsigned char a[N * 8], b[N * 8];
};

template <int N>
constexpr FltNet<N> flt_make_net()
{
    FltNet<N> net{};
    for (int p = 1; p < N; p *= 2)
        for (int k = p; k >= 1; k /= 2)
            for (int j = k % p; j <= N - 1 - k; j += 2 * k)
                for (int i = 0; i <= (k - 1 < N - j - k - 1 ? k - 1 : N - j - k - 1); i++)
                    if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
                        net.a[net.n] = (unsigned char)(i + j);
                        net.b[net.n] = (unsigned char)(i + j + k);
                        net.n++;
                    }
    return net;
}

// v sorted ascending (every use reads v[(N - 1) / 2] only)
template <int N>
__host__ __device__ __forceinline__ void flt_sort(i32 (&v)[N])
{
    constexpr FltNet<N> net = flt_make_net<N>();
#pragma unroll
    for (int c = 0; c < net.n; c++) {
        const i32 x = v[net.a[c]], y = v[net.b[c]];
        v[net.a[c]] = x < y ? x : y;
        v[net.b[c]] = x < y ? y : x;
    }
}
