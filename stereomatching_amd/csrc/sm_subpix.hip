// sm_subpix.hip -- subpixel refinement of the SAD / SSD cost mode (sm_cost_refine).
//
// Input: a whole-pixel map web of sm_cost_wta and the same gray pair.  Per pixel (x, y), s = web(x, y), and
// C(d) = the n x n window cost at shift index d, summed exactly as sm_cost_wta sums it (border rules included).
// Output: sub, int16, in 1/16 of a shift:
//     s outside 1..D               sub = 0 (no taps, no read outside the row)
//     s == 1 or s == D             sub = 16 s
//     otherwise                    a = C(s-2) - C(s-1), b = C(s) - C(s-1)       (the winner's index is s - 1)
//                                  SSD (parabola):    den = a + b,    q = floor((16 (a - b) + den) / (2 den))
//                                  SAD (equiangular): m = max(a, b),  q = floor((16 (a - b) + m) / (2 m))
//                                  denominator <= 0: q = 0, else q clamped to [-8, 8];   sub = 16 s + q
// For a web of sm_cost_wta on the same images first-wins gives a >= 1, b >= 0: the denominator is positive and
// |q| <= 8 without the clamp (it is there for caller-made maps).  sub / 16 - 1 is the subpixel shift: left x
// matches right x + d.
//
// int32 suffices: a window cost is at most 625 * 65025 = 40 640 625 (25 x 25 SSD), so |a|, |b| < 2^26,
// |16 (a - b)| < 2^31 - 2^30 and 16 (a - b) + den, 2 den stay below 2^31 as well.  16 * 512 + 8 fits int16.
//
// Kernel: workgroups of four waves own 64 columns x TH rows of one pair, one pixel per lane and TH / 4 rows per
// lane.  The left rows of the tile and its window halo are staged once in LDS; the right rows only over the
// columns the tile's shifts reach -- [min s, max s] of its valid pixels, found by a workgroup reduction before
// staging (a smooth map spans a few shifts, so a tile stages about its own width; the LDS is sized for the
// full span D, which at D = 512 and 25 x 25 is 31 KB, so the span always fits).  Work per pixel is three
// shifts x n^2 taps, independent of D:
//   SAD: v_qsad_pk_u16_u8 adds four consecutive shifts s-2 .. s+1 of a 4-pixel group at once; three of its
//        four fields are used.  The last group of a window row holds n mod 4 pixels: its other left bytes are
//        zeroed, which adds the plain right bytes there, and one v_mqsad_pk_u16_u8 against 255 on exactly
//        those bytes adds 255 minus them -- together a constant 255 (4 - n mod 4) per row, subtracted at the
//        end.  The packed fields are exact modulo 2^16, so rows are summed in chunks whose true sum stays
//        below 2^16 (chunk rows x n x 255 < 65536) and each chunk is added into 32-bit sums.
//   SSD: per shift LL + RR - 2 LR on v_dot4_u32_u8, the right window cut with v_alignbyte per shift.
// Ghost border: rows and columns outside the image are staged as zeros, which is the definition everywhere
// except at taps left of the image (left 0, right x' + d inside): pixels x < half take a masked variant whose
// left bytes outside the image are zeroed and cancelled by v_mqsad (SAD) or masked on both sides (SSD).

#include "sm_internal.h"

typedef unsigned long long u64;

#define SMR_TW 64        // columns per workgroup (one per lane)
#define SMR_WAVES 4
#define SMR_TH 16        // rows per workgroup at most (fewer on short images)

struct RefineGeom {
    int w, h, D, ghost;
    int th;              // rows per workgroup (a multiple of SMR_WAVES)
    int tiles_x, tiles_y;
    int padl;            // bytes left of the tile in a staged left row (multiple of 4, >= half)
    int lrow;            // bytes per staged left row (multiple of 16)
    int rcap;            // bytes per staged right row (multiple of 16): room for the full shift span
    int nsr;             // staged rows = th + n - 1
    int fast;            // w % 4 == 0 and dword-aligned images: a staged dword never straddles a border
    int want_costs;
};

__device__ __forceinline__ int smr_floordiv(int num, int den)      // den > 0
{
    const int q = num / den;
    return (num % den != 0 && num < 0) ? q - 1 : q;
}

// v mod n for n > 0: one add or subtract for the rows and columns next to the image (a division only on images
// narrower or shorter than the window reaches, where the staged halo wraps more than once)
__device__ __forceinline__ int smr_wrap(int v, int n)
{
    if (v < 0) v += n;
    if (v >= n) v -= n;
    if ((unsigned)v >= (unsigned)n) v = ((v % n) + n) % n;
    return v;
}

// Stage `rows` rows starting at image row y0 of one image, `dwords` dwords per row starting at image column c0
// (a multiple of 4), with the border rule applied, into dst[row * stride_dw + k].  All 256 threads take part:
// a lane owns dword columns tid & 63 (+ 64 ...), the four waves split the rows.
__device__ __forceinline__ void smr_stage(u32 *dst, int stride_dw, const u8 *__restrict__ img, const RefineGeom &g,
                                          int c0, int y0, int rows, int dwords, int tid)
{
    for (int k = tid & 63; k < dwords; k += 64) {
        const int c = c0 + 4 * k;
        if (g.fast) {
            const bool vx = !g.ghost || (c >= 0 && c < g.w);
            const int cs = g.ghost ? (vx ? c : 0) : smr_wrap(c, g.w);
            for (int r = tid >> 6; r < rows; r += SMR_WAVES) {
                const int y = y0 + r;
                const bool vy = !g.ghost || (y >= 0 && y < g.h);
                const int ys = g.ghost ? (vy ? y : 0) : smr_wrap(y, g.h);
                u32 v = 0;
                if (vx && vy) v = *reinterpret_cast<const u32 *>(img + (size_t)ys * g.w + cs);
                dst[r * stride_dw + k] = v;
            }
        } else {
            int cs[4];
            bool vx[4];
#pragma unroll
            for (int b = 0; b < 4; b++) {
                vx[b] = !g.ghost || (c + b >= 0 && c + b < g.w);
                cs[b] = g.ghost ? (vx[b] ? c + b : 0) : smr_wrap(c + b, g.w);
            }
            for (int r = tid >> 6; r < rows; r += SMR_WAVES) {
                const int y = y0 + r;
                const bool vy = !g.ghost || (y >= 0 && y < g.h);
                const int ys = g.ghost ? (vy ? y : 0) : smr_wrap(y, g.h);
                const u8 *src = img + (size_t)ys * g.w;
                u32 v = 0;
#pragma unroll
                for (int b = 0; b < 4; b++)
                    if (vx[b] && vy) v |= (u32)src[cs[b]] << (8 * b);
                dst[r * stride_dw + k] = v;
            }
        }
    }
}

// The three window costs C(s-2), C(s-1), C(s) of one pixel.  rowL / rowR: its first window row in the staged
// left / right rows; lb: byte of its window's first column in a staged left row; rb: byte of that column + s - 2
// in a staged right row.  MASKED: ghost pixels x < half (xl = x - half: image column of window byte 0).
template <int N, bool SSD, bool MASKED>
__device__ __forceinline__ void smr_costs(const u32 *rowL, int lstride, const u32 *rowR, int rstride, int lb, int rb,
                                          int xl, u32 out[3])
{
    constexpr int NG = (N + 3) / 4, RB = N % 4;
    constexpr u32 MASKR = RB == 1 ? 0x000000ffu : 0x00ffffffu;     // bytes of the last group inside the window
    u32 M[NG];
    int masked = 4 * NG - N;                                       // bytes per row outside the window or image
#pragma unroll
    for (int gp = 0; gp < NG; gp++) {
        u32 m = gp == NG - 1 ? MASKR : 0xffffffffu;
        if (MASKED) {
#pragma unroll
            for (int b = 0; b < 4; b++)
                if (xl + 4 * gp + b < 0 && ((m >> (8 * b)) & 0xff)) { m &= ~(0xffu << (8 * b)); masked++; }
        }
        M[gp] = m;
    }
    const int lw0 = lb >> 2, ls = lb & 3;
    if (!SSD) {
        // rows in chunks whose packed 16-bit sums cannot exceed 2^16 (the fields are exact modulo 2^16)
        constexpr int CHUNK = 257 / N < N ? 257 / N : N;
        const int rw0 = rb >> 2, rs = rb & 3;
        u32 c0 = 0, c1 = 0, c2 = 0;
        for (int r0 = 0; r0 < N; r0 += CHUNK) {
            const int nr = N - r0 < CHUNK ? N - r0 : CHUNK;
            // two independent chains (even / odd rows): the quad-SAD chain of one pixel is otherwise 4 n dependent
            // quarter-rate instructions long
            u64 acc[2] = {0, 0};
            for (int r = r0; r < r0 + nr; r++) {
                const u32 *pl = rowL + r * lstride + lw0, *pr = rowR + r * rstride + rw0;
                u32 t[NG + 1], u[NG + 2], rr[NG + 1];
#pragma unroll
                for (int m = 0; m <= NG; m++) t[m] = pl[m];
#pragma unroll
                for (int m = 0; m < NG + 2; m++) u[m] = pr[m];
#pragma unroll
                for (int m = 0; m <= NG; m++) rr[m] = __builtin_amdgcn_alignbyte(u[m + 1], u[m], rs);
                u64 a = acc[(r - r0) & 1];
#pragma unroll
                for (int gp = 0; gp < NG; gp++) {
                    const u32 l = __builtin_amdgcn_alignbyte(t[gp + 1], t[gp], ls) & M[gp];
                    const u64 s8 = (u64)rr[gp] | ((u64)rr[gp + 1] << 32);
                    a = __builtin_amdgcn_qsad_pk_u16_u8(s8, l, a);
                    // zeroed left bytes added the right bytes there; 255 - those bytes makes it a constant
                    if (MASKED || gp == NG - 1) a = __builtin_amdgcn_mqsad_pk_u16_u8(s8, ~M[gp], a);
                }
                acc[(r - r0) & 1] = a;
            }
            // (each chain holds at most nr rows, so each is exact modulo 2^16 on its own)
            const int ne = (nr + 1) / 2, no = nr / 2;
            const u32 ce = (u32)(ne * masked * 255), co = (u32)(no * masked * 255);
            const u32 lo = (u32)acc[0], hi = (u32)(acc[0] >> 32), lo2 = (u32)acc[1], hi2 = (u32)(acc[1] >> 32);
            c0 += ((lo - ce) & 0xffffu) + ((lo2 - co) & 0xffffu);
            c1 += (((lo >> 16) - ce) & 0xffffu) + (((lo2 >> 16) - co) & 0xffffu);
            c2 += ((hi - ce) & 0xffffu) + ((hi2 - co) & 0xffffu);
        }
        out[0] = c0; out[1] = c1; out[2] = c2;
    } else {
        u32 ll = 0, rrs[3] = {0, 0, 0}, lr[3] = {0, 0, 0};
        for (int r = 0; r < N; r++) {
            const u32 *pl = rowL + r * lstride + lw0;
            u32 t[NG + 1], l[NG];
#pragma unroll
            for (int m = 0; m <= NG; m++) t[m] = pl[m];
#pragma unroll
            for (int gp = 0; gp < NG; gp++) {
                l[gp] = __builtin_amdgcn_alignbyte(t[gp + 1], t[gp], ls) & M[gp];
                ll = __builtin_amdgcn_udot4(l[gp], l[gp], ll, false);
            }
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const int b = rb + i;
                const u32 *pr = rowR + r * rstride + (b >> 2);
                u32 u[NG + 1];
#pragma unroll
                for (int m = 0; m <= NG; m++) u[m] = pr[m];
#pragma unroll
                for (int gp = 0; gp < NG; gp++) {
                    const u32 rm = __builtin_amdgcn_alignbyte(u[gp + 1], u[gp], b & 3) & M[gp];
                    rrs[i] = __builtin_amdgcn_udot4(rm, rm, rrs[i], false);
                    lr[i] = __builtin_amdgcn_udot4(l[gp], rm, lr[i], false);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 3; i++) out[i] = ll + rrs[i] - 2u * lr[i];
    }
}

template <int N, bool SSD, bool GHOST>
__global__ __launch_bounds__(256) void k_cost_refine(const u8 *__restrict__ left, const u8 *__restrict__ right,
                                                     const i32 *__restrict__ web, int16_t *__restrict__ sub,
                                                     i32 *__restrict__ costs, const RefineGeom g)
{
    constexpr int HALF = N / 2, NG = (N + 3) / 4;
    // (Guideline 17: no static LDS; every carve offset a multiple of 16)
    extern __shared__ __attribute__((aligned(16))) u32 lds[];
    i32 *red = reinterpret_cast<i32 *>(lds);                         // [2][SMR_WAVES]: min / max s per wave
    u32 *sL = lds + 8;                                               // [nsr][lrow / 4]
    u32 *sR = sL + g.nsr * (g.lrow >> 2);                            // [nsr][rcap / 4]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pair = blockIdx.z;
    const int tx0 = blockIdx.x * SMR_TW, ty0 = blockIdx.y * g.th;
    const size_t img = (size_t)pair * g.w * g.h;
    const int x = tx0 + lane;
    const int rpt = g.th / SMR_WAVES;                                // rows per lane: wave + 4 k

    // ---- the tile's shift span over its valid pixels (s in 1..D)
    // (the values are kept for the pixel loop: a load there would be waited for before every pixel)
    int smin = 0x7fffffff, smax = -1;
    int sv[SMR_TH / SMR_WAVES];
#pragma unroll
    for (int k = 0; k < SMR_TH / SMR_WAVES; k++) {
        const int y = ty0 + wave + SMR_WAVES * k;
        sv[k] = 0;
        if (k < rpt && x < g.w && y < g.h) sv[k] = web[img + (size_t)y * g.w + x];
        if (sv[k] >= 1 && sv[k] <= g.D) { smin = min(smin, sv[k]); smax = max(smax, sv[k]); }
    }
    for (int o = 32; o >= 1; o >>= 1) {
        smin = min(smin, __shfl_xor(smin, o));
        smax = max(smax, __shfl_xor(smax, o));
    }
    if (lane == 0) { red[wave] = smin; red[SMR_WAVES + wave] = smax; }
    __syncthreads();
    smin = min(min(red[0], red[1]), min(red[2], red[3]));
    smax = max(max(red[4], red[5]), max(red[6], red[7]));

    if (smax >= 1) {                                                 // (uniform: some pixel of the tile has taps)
        const int lw = g.lrow >> 2, rw = g.rcap >> 2;
        const int cl0 = tx0 - g.padl;                                // image column of staged left byte 0
        const int cr0 = (tx0 - HALF + smin - 2) & ~3;                // ... right byte 0 (floor to a dword)
        // right bytes read: up to column tx0 + 63 - HALF + smax + 4 NG + 6 (SAD's eight-byte operands, one
        // dword beyond for the byte alignment; SSD's third shift)
        int rdw = (tx0 + SMR_TW - HALF + smax + 4 * NG + 6 - cr0 + 3) >> 2;
        rdw = min(rdw, rw);                                          // (never binds: rcap is sized for span D)
        smr_stage(sL, lw, left + img, g, cl0, ty0 - HALF, g.nsr, lw, tid);
        smr_stage(sR, rw, right + img, g, cr0, ty0 - HALF, g.nsr, rdw, tid);
    }
    __syncthreads();
    if (x >= g.w) return;

    const size_t plane = (size_t)g.w * g.h;
#pragma unroll
    for (int k = 0; k < SMR_TH / SMR_WAVES; k++) {
        const int yr = wave + SMR_WAVES * k;                         // row within the tile
        const int y = ty0 + yr;
        if (k >= rpt || y >= g.h) break;
        const size_t o = img + (size_t)y * g.w + x;
        const int s = sv[k];
        i32 c[3] = {-1, -1, -1};
        int16_t out = 0;
        if (s >= 1 && s <= g.D) {
            const u32 *rowL = sL + yr * (g.lrow >> 2), *rowR = sR + yr * (g.rcap >> 2);
            const int lb = x - HALF - (tx0 - g.padl);
            const int rb = x - HALF + s - 2 - ((tx0 - HALF + smin - 2) & ~3);
            u32 v[3];
            if (GHOST && x < HALF)
                smr_costs<N, SSD, true>(rowL, g.lrow >> 2, rowR, g.rcap >> 2, lb, rb, x - HALF, v);
            else
                smr_costs<N, SSD, false>(rowL, g.lrow >> 2, rowR, g.rcap >> 2, lb, rb, x - HALF, v);
            c[1] = (i32)v[1];
            if (s >= 2) c[0] = (i32)v[0];
            if (s <= g.D - 1) c[2] = (i32)v[2];
            int q = 0;
            if (s >= 2 && s <= g.D - 1) {
                const int a = c[0] - c[1], b = c[2] - c[1];
                const int den = SSD ? a + b : max(a, b);
                if (den > 0) q = min(8, max(-8, smr_floordiv(16 * (a - b) + den, 2 * den)));
            }
            out = (int16_t)(16 * s + q);
        }
        sub[o] = out;
        if (g.want_costs) {
            const size_t oc = (size_t)pair * 3 * plane + (size_t)y * g.w + x;
            costs[oc] = c[0];
            costs[oc + plane] = c[1];
            costs[oc + 2 * plane] = c[2];
        }
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------

template <int N>
static const void *refine_ptr(bool ssd, bool ghost)
{
    return ssd ? (ghost ? (const void *)k_cost_refine<N, true, true> : (const void *)k_cost_refine<N, true, false>)
               : (ghost ? (const void *)k_cost_refine<N, false, true> : (const void *)k_cost_refine<N, false, false>);
}

extern "C" int sm_cost_refine(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int cost,
                              int pairs, const int32_t *d_web, int16_t *d_sub, int32_t *d_costs, void *stream)
{
    SM_TRY(sm_check_pairs(plan, pairs, "sm_cost_refine"));
    if (!d_gray_left || !d_gray_right || !d_web || !d_sub)
        return sm_fail(SM_ERR_ARG, "sm_cost_refine: NULL argument");
    if (cost != SM_COST_SAD && cost != SM_COST_SSD)
        return sm_fail(SM_ERR_ARG, "sm_cost_refine: cost %d is neither SM_COST_SAD nor SM_COST_SSD", cost);
    const int half = plan->square_width / 2, n = 2 * half + 1;
    SM_TRY(sm_check_reach(plan, 512, "sm_cost_refine"));
    SM_TRY(sm_use_device(plan->device));

    RefineGeom g;
    g.w = plan->width; g.h = plan->height; g.D = plan->num_shifts;
    g.ghost = plan->border == SM_GHOST;
    const int ng = (n + 3) / 4;
    g.th = SMR_TH;
    while (g.th > SMR_WAVES && g.th / 2 >= g.h) g.th /= 2;         // (short images: fewer idle rows)
    g.tiles_x = (g.w + SMR_TW - 1) / SMR_TW;
    g.tiles_y = (g.h + g.th - 1) / g.th;
    g.padl = 4 * ((half + 3) / 4);
    // left: the last lane reads dwords up to byte 63 + padl - half + 4 ng + 3
    g.lrow = 16 * ((SMR_TW + g.padl + 4 * ng + 4 + 15) / 16);
    // right: (tx0 + 64 - half + smax + 4 ng + 6) - (tx0 - half + smin - 2 - 3), smax - smin <= D - 1
    g.rcap = 16 * ((SMR_TW + g.D - 1 + 4 * ng + 11 + 4 + 15) / 16);
    g.nsr = g.th + n - 1;
    g.fast = g.w % 4 == 0 && ((uintptr_t)d_gray_left & 3) == 0 && ((uintptr_t)d_gray_right & 3) == 0;
    g.want_costs = d_costs != nullptr;
    const size_t lds = 32 + (size_t)g.nsr * (g.lrow + g.rcap);
    const bool ssd = cost == SM_COST_SSD;
    const void *fn = nullptr;
    switch (n) {
    case 1: fn = refine_ptr<1>(ssd, g.ghost); break;
    case 3: fn = refine_ptr<3>(ssd, g.ghost); break;
    case 5: fn = refine_ptr<5>(ssd, g.ghost); break;
    case 7: fn = refine_ptr<7>(ssd, g.ghost); break;
    case 9: fn = refine_ptr<9>(ssd, g.ghost); break;
    case 11: fn = refine_ptr<11>(ssd, g.ghost); break;
    case 13: fn = refine_ptr<13>(ssd, g.ghost); break;
    case 15: fn = refine_ptr<15>(ssd, g.ghost); break;
    case 17: fn = refine_ptr<17>(ssd, g.ghost); break;
    case 19: fn = refine_ptr<19>(ssd, g.ghost); break;
    case 21: fn = refine_ptr<21>(ssd, g.ghost); break;
    case 23: fn = refine_ptr<23>(ssd, g.ghost); break;
    default: fn = refine_ptr<25>(ssd, g.ghost); break;
    }
    void *args[] = {(void *)&d_gray_left, (void *)&d_gray_right, (void *)&d_web, (void *)&d_sub, (void *)&d_costs,
                    (void *)&g};
    const hipError_t e = hipLaunchKernel(fn, dim3(g.tiles_x, g.tiles_y, pairs), dim3(64 * SMR_WAVES), args, lds,
                                         (hipStream_t)stream);
    if (e != hipSuccess) return sm_fail(SM_ERR_HIP, "sm_cost_refine: %s", hipGetErrorString(e));
    return SM_OK;
}
