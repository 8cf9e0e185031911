// sm_census.hip -- census cost mode: census transform, Hamming-distance cost, n x n box sum, first-minimum arg-min,
// the right-reference pass and the check, and the equiangular subpixel fit (include/stereo_hip.h).
//
// PARITY UNPINNED, like SAD / SSD: the reference has no census mode.  Definition (census width c in {3, 5, 7}):
//   C_I(x, y) bit k = I(x + dx, y + dy) < I(x, y), the k-th neighbour of the c x c window in row-major order without
//   (0, 0); toroidal: coordinates wrap; ghost: a neighbour outside the image reads 0 (a halo pixel's descriptor is 0);
//   c_d(x, y) = popcount(C_L(x, y) ^ C_R(x + d, y)) (toroidal: x + d mod W; ghost: C_R = 0 past the right border);
//   A_d = n x n window sum of c_d (toroidal: taps wrap; ghost: taps outside the image count 0);
//   best = min_d A_d, web = 1 + the first d reaching it.
//
// Kernels:
//   k_census_transform  descriptors of a batch of images, a 64 x 16 tile per workgroup from gray rows staged in LDS
//                       with the border rule applied (coalesced row loads; 64 consecutive descriptors per wave store).
//   k_census_wta        the cost, the box sum and the arg-min.  The descriptor rows stream through a ring of n + 1 rows
//                       in LDS while the tile marches down.  A lane owns 4 columns x 8 shifts and keeps their VERTICAL
//                       window sums in VGPRs: per row it adds the Hamming costs of the row that enters and subtracts
//                       those of the row that leaves -- each (column, shift, row) cost is computed once per slide, one
//                       v_bcnt per descriptor dword.  The horizontal sums go through LDS as packed u16 (A_d <= 48 * 625
//                       = 30000): every lane publishes its 4 x 8 column sums, and the lanes of the tile's output columns
//                       slide an n-wide window over them with v_pk_add_u16 / v_pk_sub_u16.  The shift range of a column
//                       group is split over nl adjacent lanes whose keys (A << 16 | d) are merged with DPP.  At most 128
//                       shifts per launch: wider ranges take several launches, each merging its keys into the web map
//                       (first-wins: the smaller key), the last one writing web and best.  MIRROR: the right-reference
//                       pass, the left pass over mirror(R), mirror(L).  Mirroring an image permutes every descriptor's
//                       bits the same way, and Hamming distance is blind to that, so the pass reads the left pass's
//                       descriptors in mirrored order and writes its maps in natural order.
//   k_census_second     the same march (the same text, sm_census_wta_body.h) for the runner-up of DESIGN.md 22: a shift
//                       within one of a given map's shift at the pixel gets the bias of an out-of-range shift, once.
//   k_census_refine     the three window costs C(s-2), C(s-1), C(s) of each pixel, 3 n^2 taps, and sm_cost_refine's
//                       equiangular fit.

#include "sm_device.h"
#include "sm_census.h"
#include "sm_plan_model.h"

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

#define SMN_DS 8           // wta: shifts per lane
#define SMN_DCHUNK 128     // wta: shifts per launch at most
#define SMN_PFMAX 9        // wta: descriptors one lane fetches per ring row at most (checked by the host)
#define SMN_THREADS 512    // wta: threads per workgroup at most

// ---------------------------------------------------------------------------
// transform
// ---------------------------------------------------------------------------

// Images z < n_a come from src_a and go to dst + z * W * H; the others from src_b, to dst + dst_b + (z - n_a) * W * H
// (in descriptors of NW dwords).  Workgroup 64 x 4 threads, a tile of 64 columns x 16 rows.
template <int CW, int NW, bool GHOST>
__global__ __launch_bounds__(256) void k_census_transform(const u8 *__restrict__ src_a, const u8 *__restrict__ src_b,
                                                          int n_a, u32 *__restrict__ dst, long long dst_b, int W, int H)
{
    constexpr int HC = CW / 2, SW = SMN_TX + 2 * HC, SH = SMN_TR + 2 * HC;
    __shared__ u8 tile[SH][SW + 1];
    const int z = blockIdx.z;
    const bool b = z >= n_a;
    const size_t npx = (size_t)W * H;
    const u8 *src = b ? src_b + (size_t)(z - n_a) * npx : src_a + (size_t)z * npx;
    u32 *out = dst + (size_t)NW * ((b ? (size_t)dst_b : 0) + (size_t)(b ? z - n_a : z) * npx);
    const int x0 = blockIdx.x * SMN_TX, y0 = blockIdx.y * SMN_TR;
    const int tid = threadIdx.y * SMN_TX + threadIdx.x;
    for (int i = tid; i < SH * SW; i += 256) {
        const int r = i / SW, c = i - r * SW;
        const int x = x0 - HC + c, y = y0 - HC + r;
        u8 v = 0;
        if (GHOST) {
            if (x >= 0 && x < W && y >= 0 && y < H) v = src[(size_t)y * W + x];
        } else {
            v = src[(size_t)smn_mod(y, H) * W + smn_mod(x, W)];
        }
        tile[r][c] = v;
    }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= W) return;
#pragma unroll
    for (int q = 0; q < SMN_TR / 4; q++) {
        const int ry = threadIdx.y + 4 * q;
        const int y = y0 + ry;
        if (y >= H) break;
        const u32 c = tile[ry + HC][threadIdx.x + HC];
        u32 lo = 0, hi = 0;
        int k = 0;
#pragma unroll
        for (int dy = -HC; dy <= HC; dy++)
#pragma unroll
            for (int dx = -HC; dx <= HC; dx++) {
                if (dy == 0 && dx == 0) continue;
                const u32 bit = (u32)tile[ry + HC + dy][threadIdx.x + HC + dx] < c ? 1u : 0u;
                if (k < 32) lo |= bit << k; else hi |= bit << (k - 32);
                k++;
            }
        const size_t o = (size_t)y * W + x;
        if constexpr (NW == 2) reinterpret_cast<u64 *>(out)[o] = (u64)lo | ((u64)hi << 32);
        else out[o] = lo;
    }
}

// ---------------------------------------------------------------------------
// cost, box sum, arg-min
// ---------------------------------------------------------------------------

struct CensusGeom {
    int w, h, D;
    int n, half;
    int dlo, dc;            // this launch's shifts: dlo .. dlo + dc - 1
    int nl, log2nl;         // lanes that split a column group's shift range (8 shifts each)
    int cg, hg;             // column groups of 4 per workgroup, of which hg on each side are halo only
    int tw, th;             // output columns / rows per workgroup (tw = 4 (cg - 2 hg))
    int tiles_x, tiles_y;
    int lw, rw;             // descriptors per ring row, left / right
    int xs;                 // u32 per exchange row (4 cg + 4: rows of consecutive shift lanes start 4 banks apart)
    int first, last;        // the launch's place in the shift range (keys are merged through the web map)
    int vec_ok;             // W % 4 == 0 and 16-byte aligned maps: int4 stores
    int pf;                 // descriptors one lane fetches per ring row
    long long side;         // descriptors from side 0 (left) to side 1 (right) of the workspace
};

template <int K>
__device__ __forceinline__ u32 smn_partner(u32 v)
{
    if (K == 0) return (u32)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xf, 0xf, false);
    if (K == 1) return (u32)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xf, 0xf, false);
    if (K == 2) return (u32)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x141, 0xf, 0xf, false);
    return (u32)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x140, 0xf, 0xf, false);
}

// one ring row of descriptors for this lane: as many as the host counted (g.pf), NW dwords each
template <int NW>
struct SmnRow {
    u32 v[SMN_PFMAX][NW];
};

// k_census_wta<NW, GHOST, MIRROR> and k_census_second<NW, GHOST>: one text, sm_census_wta_body.h, expanded twice.  (As a
// __forceinline__ template with a flag the march compiled to other instructions and register counts in k_census_wta
// itself; expanded by the preprocessor, the existing kernel's tokens are what they were.)
#define SMN_SECOND 0
#include "sm_census_wta_body.h"
#undef SMN_SECOND
#define SMN_SECOND 1
#include "sm_census_wta_body.h"
#undef SMN_SECOND

// ---------------------------------------------------------------------------
// subpixel refinement
// ---------------------------------------------------------------------------

struct CensusRefineGeom {
    int w, h, D, n, half;
    int want_costs;
    long long side;
};

template <int NW>
__device__ __forceinline__ u32 smn_load(const u32 *img, size_t i)
{
    return img[NW * i];
}

template <int NW>
__device__ __forceinline__ u32 smn_load_hi(const u32 *img, size_t i)
{
    return NW == 2 ? img[NW * i + 1] : 0u;
}

// One lane per pixel: s = web(x, y); for s in 1..D the window costs C(s-2), C(s-1), C(s) summed tap by tap (each tap
// one left descriptor and one right one: the three right descriptors of a tap slide along the window row).
template <int NW, bool GHOST>
__global__ __launch_bounds__(256) void k_census_refine(const u32 *__restrict__ desc, const i32 *__restrict__ web,
                                                       int16_t *__restrict__ sub, i32 *__restrict__ costs,
                                                       const CensusRefineGeom g)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    const int pair = blockIdx.z;
    if (x >= g.w || y >= g.h) return;
    const int W = g.w, H = g.h;
    const size_t npx = (size_t)W * H;
    const u32 *dL = desc + (size_t)NW * ((size_t)pair * npx);
    const u32 *dR = desc + (size_t)NW * ((size_t)g.side + (size_t)pair * npx);
    const size_t o = (size_t)pair * npx + (size_t)y * W + x;
    const int s = web[o];
    i32 c[3] = {-1, -1, -1};
    int16_t out = 0;
    if (s >= 1 && s <= g.D) {
        u32 acc[3] = {0, 0, 0};
        for (int ty = -g.half; ty <= g.half; ty++) {
            int yy = y + ty;
            if (GHOST) { if (yy < 0 || yy >= H) continue; }
            else yy = smn_mod(yy, H);
            const size_t rowo = (size_t)yy * W;
            // right columns xx + s - 2 + i of the taps xx = x - half ..: r[i] slides one column per tap
            auto rload = [&](int xr, u32 &lo, u32 &hi) {
                lo = hi = 0;
                if (GHOST) { if (xr < 0 || xr >= W) return; }
                else xr = smn_mod(xr, W);
                lo = smn_load<NW>(dR, rowo + xr);
                hi = smn_load_hi<NW>(dR, rowo + xr);
            };
            const int xs0 = x - g.half;
            u32 r0l, r0h, r1l, r1h, r2l, r2h;
            rload(xs0 + s - 2, r0l, r0h);
            rload(xs0 + s - 1, r1l, r1h);
            for (int tx = 0; tx < g.n; tx++) {
                rload(xs0 + tx + s, r2l, r2h);
                int xx = xs0 + tx;
                bool on = true;
                if (GHOST) on = xx >= 0 && xx < W;
                else xx = smn_mod(xx, W);
                if (on) {
                    const u32 ll = smn_load<NW>(dL, rowo + xx), lh = smn_load_hi<NW>(dL, rowo + xx);
                    acc[0] += (u32)__builtin_popcount(ll ^ r0l) + (u32)__builtin_popcount(lh ^ r0h);
                    acc[1] += (u32)__builtin_popcount(ll ^ r1l) + (u32)__builtin_popcount(lh ^ r1h);
                    acc[2] += (u32)__builtin_popcount(ll ^ r2l) + (u32)__builtin_popcount(lh ^ r2h);
                }
                r0l = r1l; r0h = r1h; r1l = r2l; r1h = r2h;
            }
        }
        c[1] = (i32)acc[1];
        if (s >= 2) c[0] = (i32)acc[0];
        if (s <= g.D - 1) c[2] = (i32)acc[2];
        int q = 0;
        if (s >= 2 && s <= g.D - 1) {
            const int a = c[0] - c[1], b = c[2] - c[1];
            const int den = max(a, b);
            if (den > 0) q = min(8, max(-8, smn_floordiv(16 * (a - b) + den, 2 * den)));
        }
        out = (int16_t)(16 * s + q);
    }
    sub[o] = out;
    if (g.want_costs) {
        const size_t oc = (size_t)pair * 3 * npx + (size_t)y * W + x;
        costs[oc] = c[0];
        costs[oc + npx] = c[1];
        costs[oc + 2 * npx] = c[2];
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------

extern "C" int sm_plan_reserve_census(sm_plan *plan)
{
    if (!plan) return sm_fail(SM_ERR_ARG, "sm_plan_reserve_census: plan is NULL");
    SM_TRY(sm_use_device(plan->device));
    return sm_ws_reserve(plan, SM_WS_SET_CENSUS, "sm_plan_reserve_census");
}

// what every census entry checks besides its pointers (before any device call)
int sm_census_args(const sm_plan *plan, int census_width, int pairs, const char *me)
{
    SM_TRY(sm_check_census_width(census_width, me));
    SM_TRY(sm_check_pairs(plan, pairs, me));
    return sm_check_reach(plan, 512, me);
}

template <int CW, int NW>
static const void *transform_ptr(bool ghost)
{
    return ghost ? (const void *)k_census_transform<CW, NW, true> : (const void *)k_census_transform<CW, NW, false>;
}

// descriptors of images_a images at src_a (to dst) and images_b at src_b (to dst + dst_b descriptors), NW dwords each
static int transform_launch(const sm_plan *plan, int cw, int nw, const uint8_t *src_a, int images_a,
                            const uint8_t *src_b, int images_b, u32 *dst, long long dst_b, hipStream_t st)
{
    const bool ghost = plan->border == SM_GHOST;
    const void *fn;
    if (nw == 2) fn = cw == 3 ? transform_ptr<3, 2>(ghost) : cw == 5 ? transform_ptr<5, 2>(ghost) : transform_ptr<7, 2>(ghost);
    else fn = cw == 3 ? transform_ptr<3, 1>(ghost) : transform_ptr<5, 1>(ghost);
    int W = plan->width, H = plan->height;
    if (!src_b) src_b = src_a;
    void *args[] = {(void *)&src_a, (void *)&src_b, (void *)&images_a, (void *)&dst, (void *)&dst_b, (void *)&W,
                    (void *)&H};
    const dim3 grid((W + SMN_TX - 1) / SMN_TX, (H + SMN_TR - 1) / SMN_TR, images_a + images_b), block(SMN_TX, 4);
    const hipError_t e = hipLaunchKernel(fn, grid, block, args, 0, st);
    if (e != hipSuccess) return sm_fail(SM_ERR_HIP, "launch of k_census_transform failed: %s", hipGetErrorString(e));
    return SM_OK;
}

// both images of `pairs` pairs into the workspace: 4-byte descriptors for c <= 5, 8-byte for c = 7
int sm_census_descriptors(sm_plan *plan, int cw, const uint8_t *left, const uint8_t *right, int pairs, hipStream_t st)
{
    const long long side = (long long)plan->max_pairs * plan->width * plan->height;
    return transform_launch(plan, cw, cw == 7 ? 2 : 1, left, pairs, right, pairs, plan->d_census, side, st);
}

// the arg-min over the plan's shifts from the workspace's descriptors, in launches of at most SMN_DCHUNK shifts;
// d_map: k_census_second (left reference only), which keeps the shifts within one of the map's out of it
static int wta_launch(const sm_plan *plan, int cw, bool mirror, int pairs, const i32 *d_map, i32 *d_web, i32 *d_best,
                      hipStream_t st)
{
    const int nw = cw == 7 ? 2 : 1;
    CensusGeom g;
    g.w = plan->width; g.h = plan->height; g.D = plan->num_shifts;
    g.half = plan->square_width / 2; g.n = 2 * g.half + 1;
    g.hg = (g.half + 3) / 4;
    g.side = (long long)plan->max_pairs * g.w * g.h;
    g.vec_ok = g.w % 4 == 0 && (((uintptr_t)d_web | (uintptr_t)d_best) & 15) == 0;
    const bool ghost = plan->border == SM_GHOST;
    const void *fn = nw == 2 ? SM_PASS_KERNEL(k_census_wta, 2, ghost, mirror) : SM_PASS_KERNEL(k_census_wta, 1, ghost, mirror);
    if (d_map)
        fn = nw == 2 ? (ghost ? (const void *)k_census_second<2, true> : (const void *)k_census_second<2, false>)
                     : (ghost ? (const void *)k_census_second<1, true> : (const void *)k_census_second<1, false>);
    for (int dlo = 0; dlo < g.D; dlo += SMN_DCHUNK) {
        g.dlo = dlo;
        g.dc = min(SMN_DCHUNK, g.D - dlo);
        g.first = dlo == 0;
        g.last = dlo + g.dc >= g.D;
        g.nl = sm_lanes_for(g.dc, SMN_DS, &g.log2nl);
        // column groups: up to 64 (256 columns) and 512 threads, fewer while the LDS request exceeds 64 KiB; at least one
        // output group between the halo groups
        g.cg = min(64, SMN_THREADS / g.nl);
        size_t lds;
        for (;;) {
            g.lw = 4 * g.cg;
            g.rw = 4 * g.cg + SMN_DS * g.nl;
            g.xs = 4 * g.cg + 4;
            lds = 4 * ((size_t)(g.n + 1) * (g.lw + g.rw) * nw + (size_t)4 * g.nl * g.xs);
            if (lds <= 64 * 1024 || g.cg <= 2 * g.hg + 1) break;
            g.cg = max(2 * g.hg + 1, g.cg / 2);
        }
        if (g.cg <= 2 * g.hg) g.cg = 2 * g.hg + 1;
        const int T = g.cg * g.nl;
        g.pf = (g.lw + g.rw + T - 1) / T;
        if (g.pf > SMN_PFMAX || lds > 64 * 1024)
            return sm_fail(SM_ERR_HIP, "census: internal tiling error (pf %d, %zu bytes of LDS)", g.pf, lds);
        g.tw = 4 * (g.cg - 2 * g.hg);
        g.tiles_x = (g.w + g.tw - 1) / g.tw;
        g.th = min(sm_rows_for_grid(g.tiles_x, g.h, pairs), g.h);
        g.tiles_y = (g.h + g.th - 1) / g.th;
        void *args[] = {(void *)&plan->d_census, (void *)&d_web, (void *)&d_best, (void *)&g};
        void *args_second[] = {(void *)&plan->d_census, (void *)&d_map, (void *)&d_web, (void *)&d_best, (void *)&g};
        const hipError_t e = hipLaunchKernel(fn, dim3(g.tiles_x, g.tiles_y, pairs), dim3(T), d_map ? args_second : args,
                                             lds, st);
        if (e != hipSuccess)
            return sm_fail(SM_ERR_HIP, "launch of %s failed: %s", d_map ? "k_census_second" : "k_census_wta",
                           hipGetErrorString(e));
    }
    return SM_OK;
}

int sm_census_wta_launch(const sm_plan *plan, int cw, bool mirror, int pairs, i32 *d_web, i32 *d_best, hipStream_t st)
{
    return wta_launch(plan, cw, mirror, pairs, nullptr, d_web, d_best, st);
}

int sm_census_second_launch(const sm_plan *plan, int cw, int pairs, const i32 *d_map, i32 *d_web2, i32 *d_best2,
                            hipStream_t st)
{
    return wta_launch(plan, cw, false, pairs, d_map, d_web2, d_best2, st);
}

extern "C" int sm_census_transform(sm_plan *plan, const uint8_t *d_gray, int census_width, int images, uint64_t *d_desc,
                                   void *stream)
{
    const char *me = "sm_census_transform";
    if (!d_gray || !d_desc) return sm_fail(SM_ERR_ARG, "%s: NULL argument", me);
    SM_TRY(sm_check_census_width(census_width, me));
    if (!plan) return sm_fail(SM_ERR_ARG, "%s: plan is NULL", me);
    if (images < 1 || images > 2 * plan->max_pairs)
        return sm_fail(SM_ERR_ARG, "%s: images %d outside 1..%d (2 * max_pairs of the plan)", me, images,
                       2 * plan->max_pairs);
    SM_TRY(sm_use_device(plan->device));
    return transform_launch(plan, census_width, 2, d_gray, images, nullptr, 0, (u32 *)d_desc, 0, (hipStream_t)stream);
}

extern "C" int sm_census_wta(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width,
                             int pairs, int32_t *d_web, int32_t *d_best, void *stream)
{
    return sm_entry_one({"sm_census_wta", plan, d_gray_left, d_gray_right, pairs, (hipStream_t)stream},
                        CensusMode(census_width), false, d_web, d_best, nullptr);
}

extern "C" int sm_census_wta_right(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right,
                                   int census_width, int pairs, int32_t *d_web_right, int32_t *d_best_right, void *stream)
{
    return sm_entry_one({"sm_census_wta_right", plan, d_gray_left, d_gray_right, pairs, (hipStream_t)stream},
                        CensusMode(census_width), true, d_web_right, d_best_right, nullptr);
}

extern "C" int sm_census_lr(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width,
                            int pairs, int max_diff, int32_t *d_web, int32_t *d_best, int32_t *d_web_right,
                            int32_t *d_rejected, void *stream)
{
    return sm_entry_lr({"sm_census_lr", plan, d_gray_left, d_gray_right, pairs, (hipStream_t)stream},
                       CensusMode(census_width), max_diff, d_web, d_best, d_web_right, d_rejected, nullptr);
}

extern "C" int sm_census_refine(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right,
                                int census_width, int pairs, const int32_t *d_web, int16_t *d_sub, int32_t *d_costs,
                                void *stream)
{
    const char *me = "sm_census_refine";
    if (!d_gray_left || !d_gray_right || !d_web || !d_sub) return sm_fail(SM_ERR_ARG, "%s: NULL argument", me);
    SM_TRY(sm_census_args(plan, census_width, pairs, me));
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    SM_TRY(sm_ws_need(plan, SM_WS_SET_CENSUS, st, me));
    SM_TRY(sm_census_descriptors(plan, census_width, d_gray_left, d_gray_right, pairs, st));
    CensusRefineGeom g;
    g.w = plan->width; g.h = plan->height; g.D = plan->num_shifts;
    g.half = plan->square_width / 2; g.n = 2 * g.half + 1;
    g.want_costs = d_costs != nullptr;
    g.side = (long long)plan->max_pairs * g.w * g.h;
    const bool ghost = plan->border == SM_GHOST;
    const void *fn = census_width == 7 ? (ghost ? (const void *)k_census_refine<2, true> : (const void *)k_census_refine<2, false>)
                                       : (ghost ? (const void *)k_census_refine<1, true> : (const void *)k_census_refine<1, false>);
    void *args[] = {(void *)&plan->d_census, (void *)&d_web, (void *)&d_sub, (void *)&d_costs, (void *)&g};
    const hipError_t e = hipLaunchKernel(fn, dim3((g.w + 63) / 64, (g.h + 3) / 4, pairs), dim3(64, 4), args, 0, st);
    if (e != hipSuccess) return sm_fail(SM_ERR_HIP, "launch of k_census_refine failed: %s", hipGetErrorString(e));
    return SM_OK;
}
