// sm_sgm.hip -- semi-global matching over the census data term (include/stereo_hip.h).  The
// kernels read the census workspace's descriptors, which sm_census_descriptors (sm_census.hip) writes.
//
// PARITY UNPINNED, like census: the reference has no SGM.  Definition (tests/sgm_reference.py is its executable form):
//   A(p, d)   = the census window cost of sm_census_wta (d = 0 .. D - 1), A <= 48 * 625
//   L_r(p, d) = A(p, d) where q = p - r lies outside the image (paths never wrap, in either border mode), else
//               A(p, d) + min(L_r(q, d), L_r(q, d -+ 1) + P1, m_q + P2) - m_q,  m_q = min_k L_r(q, k);
//               terms with d -+ 1 outside 0 .. D - 1 dropped.  A <= L_r <= A + P2 <= 62767 (u16 bound).
//               (62767 is reached by tests/test_census_extremes_gpu.py test_sgm_at_its_u16_and_key_bounds)
//   S(p, d)   = sum of L_r over the 4 or 8 directions r; best = min_d S, web = 1 + the first d reaching it;
//   sub       = sm_cost_refine's SSD (parabola) rule on S(s-2), S(s-1), S(s), s = web.
//
// Volumes (the plan's SGM workspace, one pair at a time): A [H][W][Dp] u16 and S [H][W][Dp] i32, Dp = 64, 128 or 256 (the
// least that holds D), d innermost.  The path kernels give a line to a wave, lane l holding shifts K l .. K l + K - 1
// (K = Dp / 64), so that every step reads and writes Dp contiguous entries; entries d >= D are never read as costs.
//
// Kernels:
//   k_sgm_cost_h   the horizontal window sums of the Hamming costs of one row (n = 1: A itself): a lane owns one shift
//                  and slides an n-wide window along a run of columns (two v_bcnt per output after the first).
//                  MIRROR: the right-reference data term, the descriptors read in mirrored order (as k_census_wta).
//   k_sgm_cost_v   the vertical window sums of those (n > 1), a lane per (column, shift) sliding down a run of rows.
//   k_sgm_path     one direction of the recurrence.  FIRST writes S = L_r, MID adds L_r into S, LAST adds it in
//                  registers and emits web / best / sub, so the final S is never stored.  The data term (and S) of
//                  step i + SGP_PF is loaded while step i is computed: the chain of a line is thousands of steps long,
//                  and without that it waits on memory at every one.  d -+ 1 are ds_bpermute shifts of one lane's end
//                  values; m_q is an in-lane min, four DPP min steps within each row of 16 lanes and four readlanes.
//   k_sgm_path_second  LAST with a second reduction (the same text, sm_sgm_path_body.h): the keys of the shifts further
//                  than 1 from the winner's go through sgm_wave_min once more, and the runner-up maps of DESIGN.md 22
//                  come out beside web / best / sub.  S is still never stored.
// (k_sgm_sub_mask, sub = 0 where the checked map is 0, is a post-filter: sm_filter.hip, sm_sub_mask_launch)


#include "sm_device.h"
#include "sm_entry.h"

typedef unsigned long long u64;
typedef unsigned short u16;

#define SGM_MAX_SHIFTS 256
#define SGM_INF 0x3fffffff        // L of a shift outside 0 .. D - 1: never a minimum, + P1 cannot wrap
#define SGP_PF 8                  // path kernel: steps loaded ahead
#define SGC_XR 32                 // k_sgm_cost_h: columns per lane
#define SGC_YR 64                 // k_sgm_cost_v: rows per lane

struct SgmCostGeom {
    int w, h, D, Dp, half;
    long long side;               // descriptors from side 0 (left) to side 1 (right) of the census workspace
    long long pair;               // descriptors of the pair's left image from the start of its side
};

// descriptor of column c (pass coordinates; MIRROR: natural column W - 1 - c) of row y of an image
template <int NW, bool MIRROR>
__device__ __forceinline__ u64 sgm_desc(const u32 *img, int W, int y, int c)
{
    const size_t i = (size_t)y * W + (MIRROR ? W - 1 - c : c);
    if constexpr (NW == 2) return reinterpret_cast<const u64 *>(img)[i];
    else return img[i];
}

// grid (ceil(W / SGC_XR), ceil(H / 4), Dp / 64), block (64, 4): lane = shift, threadIdx.y = row
template <int NW, bool GHOST, bool MIRROR>
__global__ __launch_bounds__(256) void k_sgm_cost_h(const u32 *__restrict__ desc, u16 *__restrict__ out,
                                                    const SgmCostGeom g)
{
    const int d = blockIdx.z * 64 + threadIdx.x;
    const int y = blockIdx.y * 4 + threadIdx.y;
    const int x0 = blockIdx.x * SGC_XR;
    const int W = g.w;
    if (y >= g.h) return;
    const int x1 = min(x0 + SGC_XR, W);
    u16 *o = out + ((size_t)y * W) * g.Dp + d;
    if (d >= g.D) {
        for (int x = x0; x < x1; x++) o[(size_t)x * g.Dp] = 0;
        return;
    }
    // MIRROR: the pass's left image is mirror(R), its right image mirror(L)
    const u32 *dL = desc + (size_t)NW * ((MIRROR ? (size_t)g.side : 0) + (size_t)g.pair);
    const u32 *dR = desc + (size_t)NW * ((MIRROR ? 0 : (size_t)g.side) + (size_t)g.pair);
    // the Hamming cost of tap column xx (pass coordinates) at shift d
    auto cost = [&](int xx) -> u32 {
        u64 l, r = 0;
        if (GHOST) {
            if (xx < 0 || xx >= W) return 0u;
            l = sgm_desc<NW, MIRROR>(dL, W, y, xx);
            if (xx + d < W) r = sgm_desc<NW, MIRROR>(dR, W, y, xx + d);
        } else {
            xx = smn_mod(xx, W);
            l = sgm_desc<NW, MIRROR>(dL, W, y, xx);
            r = sgm_desc<NW, MIRROR>(dR, W, y, smn_mod(xx + d, W));
        }
        return (u32)__builtin_popcountll(l ^ r);
    };
    u32 s = 0;
    for (int t = -g.half; t <= g.half; t++) s += cost(x0 + t);
    o[(size_t)x0 * g.Dp] = (u16)s;
    for (int x = x0 + 1; x < x1; x++) {
        s += cost(x + g.half);
        s -= cost(x - 1 - g.half);
        o[(size_t)x * g.Dp] = (u16)s;
    }
}

// grid (ceil(W / 4), ceil(H / SGC_YR), Dp / 64), block (64, 4): lane = shift, threadIdx.y = column
template <bool GHOST>
__global__ __launch_bounds__(256) void k_sgm_cost_v(const u16 *__restrict__ hs, u16 *__restrict__ out,
                                                    const SgmCostGeom g)
{
    const int d = blockIdx.z * 64 + threadIdx.x;
    const int x = blockIdx.x * 4 + threadIdx.y;
    const int y0 = blockIdx.y * SGC_YR;
    const int W = g.w, H = g.h;
    if (x >= W) return;
    const int y1 = min(y0 + SGC_YR, H);
    const size_t col = (size_t)x * g.Dp + d, row = (size_t)W * g.Dp;
    auto tap = [&](int yy) -> u32 {
        if (GHOST) {
            if (yy < 0 || yy >= H) return 0u;
        } else {
            yy = smn_mod(yy, H);
        }
        return hs[(size_t)yy * row + col];
    };
    u32 s = 0;
    for (int t = -g.half; t <= g.half; t++) s += tap(y0 + t);
    out[(size_t)y0 * row + col] = (u16)s;
    for (int y = y0 + 1; y < y1; y++) {
        s += tap(y + g.half);
        s -= tap(y - 1 - g.half);
        out[(size_t)y * row + col] = (u16)s;
    }
}

struct SgmPathGeom {
    int w, h, D, Dp;
    int p1, p2;
    int dx, dy;                   // the direction r
    int lines;
    int mirror;                   // LAST: the pass is the right-reference one: map column x is natural W - 1 - x
    long long map;                // LAST: element offset of the pair's maps
};

enum { SGM_FIRST = 0, SGM_MID = 1, SGM_LAST = 2 };

template <int K> struct SgmVec;
template <> struct SgmVec<1> {
    static __device__ __forceinline__ void load_a(const u16 *p, i32 (&v)[1]) { v[0] = p[0]; }
    static __device__ __forceinline__ void load_s(const i32 *p, i32 (&v)[1]) { v[0] = p[0]; }
    static __device__ __forceinline__ void store_s(i32 *p, const i32 (&v)[1]) { p[0] = v[0]; }
};
template <> struct SgmVec<2> {
    static __device__ __forceinline__ void load_a(const u16 *p, i32 (&v)[2])
    {
        const u32 t = *reinterpret_cast<const u32 *>(p);
        v[0] = (i32)(t & 0xffff); v[1] = (i32)(t >> 16);
    }
    static __device__ __forceinline__ void load_s(const i32 *p, i32 (&v)[2])
    {
        const int2 t = *reinterpret_cast<const int2 *>(p);
        v[0] = t.x; v[1] = t.y;
    }
    static __device__ __forceinline__ void store_s(i32 *p, const i32 (&v)[2])
    {
        *reinterpret_cast<int2 *>(p) = make_int2(v[0], v[1]);
    }
};
template <> struct SgmVec<4> {
    static __device__ __forceinline__ void load_a(const u16 *p, i32 (&v)[4])
    {
        const uint2 t = *reinterpret_cast<const uint2 *>(p);
        v[0] = (i32)(t.x & 0xffff); v[1] = (i32)(t.x >> 16); v[2] = (i32)(t.y & 0xffff); v[3] = (i32)(t.y >> 16);
    }
    static __device__ __forceinline__ void load_s(const i32 *p, i32 (&v)[4])
    {
        const int4 t = *reinterpret_cast<const int4 *>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
    static __device__ __forceinline__ void store_s(i32 *p, const i32 (&v)[4])
    {
        *reinterpret_cast<int4 *>(p) = make_int4(v[0], v[1], v[2], v[3]);
    }
};

// the minimum over the wave (uniform): in-lane values already merged into v
__device__ __forceinline__ i32 sgm_wave_min(i32 v)
{
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xf, 0xf, false));     // quad_perm [1, 0, 3, 2]
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xf, 0xf, false));     // quad_perm [2, 3, 0, 1]
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xf, 0xf, false));    // row_half_mirror
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xf, 0xf, false));    // row_mirror
    return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// entry k of lane `lane` (both uniform) of a K-vector
template <int K>
__device__ __forceinline__ i32 sgm_pick(const i32 (&v)[K], int lane, int k)
{
    i32 t = v[0];
#pragma unroll
    for (int j = 1; j < K; j++) t = k == j ? v[j] : t;
    return __builtin_amdgcn_readlane(t, lane);
}

// k_sgm_path<K, MODE> and k_sgm_path_second<K>: one text, sm_sgm_path_body.h, expanded twice (as in sm_census.hip: the
// existing kernels' tokens are what they were, and so are their instructions and register counts)
#define SGM_SECOND 0
#include "sm_sgm_path_body.h"
#undef SGM_SECOND
#define SGM_SECOND 1
#include "sm_sgm_path_body.h"
#undef SGM_SECOND

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

// 64, 128 or 256: the path kernel's lanes hold 1, 2 or 4 shifts each
static int sgm_padded_shifts(const sm_plan *plan)
{
    return plan->num_shifts <= 64 ? 64 : plan->num_shifts <= 128 ? 128 : 256;
}

// one pair's data-term volume (u16) and aggregate volume (i32), Dp entries per pixel each
size_t sm_sgm_volume_bytes(const sm_plan *plan)
{
    return (size_t)6 * plan->width * plan->height * sgm_padded_shifts(plan);
}

// the census workspace (descriptors, and the mirrored-order map if the plan has none yet) and one pair's volumes; on
// failure the volumes are not kept (a census workspace reserved on the way stays)
extern "C" int sm_plan_reserve_sgm(sm_plan *plan)
{
    if (!plan) return sm_fail(SM_ERR_ARG, "sm_plan_reserve_sgm: plan is NULL");
    SM_TRY(sm_use_device(plan->device));
    return sm_ws_reserve(plan, SM_WS_SET_SGM, "sm_plan_reserve_sgm");
}

// what every SGM entry checks besides its pointers (before any device call; the checks that need no plan first)
// (the checks that need no plan: also banded SGM's, sm_sgm_near.hip)
int sm_sgm_scalar_args(int census_width, int p1, int p2, int paths, const char *me)
{
    SM_TRY(sm_check_census_width(census_width, me));
    if (paths != 4 && paths != 8) return sm_fail(SM_ERR_ARG, "%s: paths %d is not 4 or 8", me, paths);
    if (p1 < 0 || p2 < p1 || p2 > 32767)
        return sm_fail(SM_ERR_ARG, "%s: penalties p1 %d, p2 %d break 0 <= p1 <= p2 <= 32767", me, p1, p2);
    return SM_OK;
}

static int sgm_args(const sm_plan *plan, int census_width, int p1, int p2, int paths, int pairs, const char *me)
{
    SM_TRY(sm_sgm_scalar_args(census_width, p1, p2, paths, me));
    SM_TRY(sm_check_pairs(plan, pairs, me));
    return sm_check_reach(plan, SGM_MAX_SHIFTS, me);
}

// the data term of one pair into the A volume (S's memory holds the horizontal sums for n > 1)
static int sgm_cost_launch(const sm_plan *plan, int cw, bool mirror, int pair, hipStream_t st)
{
    SgmCostGeom g;
    g.w = plan->width; g.h = plan->height; g.D = plan->num_shifts; g.Dp = sgm_padded_shifts(plan);
    g.half = plan->square_width / 2;
    g.side = (long long)plan->max_pairs * g.w * g.h;
    g.pair = (long long)pair * g.w * g.h;
    u16 *A = (u16 *)plan->d_sgm;
    u16 *hs = g.half ? (u16 *)((char *)plan->d_sgm + (size_t)2 * g.w * g.h * g.Dp) : A;
    const bool ghost = plan->border == SM_GHOST;
    const void *fn;
    fn = cw == 7 ? SM_PASS_KERNEL(k_sgm_cost_h, 2, ghost, mirror) : SM_PASS_KERNEL(k_sgm_cost_h, 1, ghost, mirror);
    {
        void *args[] = {(void *)&plan->d_census, (void *)&hs, (void *)&g};
        const hipError_t e = hipLaunchKernel(fn, dim3((g.w + SGC_XR - 1) / SGC_XR, (g.h + 3) / 4, g.Dp / 64),
                                             dim3(64, 4), args, 0, st);
        if (e != hipSuccess) return sm_fail(SM_ERR_HIP, "launch of k_sgm_cost_h failed: %s", hipGetErrorString(e));
    }
    if (!g.half) return SM_OK;
    fn = ghost ? (const void *)k_sgm_cost_v<true> : (const void *)k_sgm_cost_v<false>;
    void *args[] = {(void *)&hs, (void *)&A, (void *)&g};
    const hipError_t e = hipLaunchKernel(fn, dim3((g.w + 3) / 4, (g.h + SGC_YR - 1) / SGC_YR, g.Dp / 64), dim3(64, 4),
                                         args, 0, st);
    if (e != hipSuccess) return sm_fail(SM_ERR_HIP, "launch of k_sgm_cost_v failed: %s", hipGetErrorString(e));
    return SM_OK;
}

template <int K>
static const void *sgm_path_ptr(int mode)
{
    return mode == SGM_FIRST ? (const void *)k_sgm_path<K, SGM_FIRST>
         : mode == SGM_MID ? (const void *)k_sgm_path<K, SGM_MID> : (const void *)k_sgm_path<K, SGM_LAST>;
}

// the directions in stream order (integer sums: the order changes nothing); the last one emits the maps
// (web2: the last direction is k_sgm_path_second, which writes the runner-up maps as well)
// (keep: the last direction is SGM_MID as well, so the full S is left in the volume and no map is written)
static int sgm_paths_launch(const sm_plan *plan, int p1, int p2, int paths, bool mirror, int pair, i32 *web, i32 *best,
                            int16_t *sub, i32 *web2, i32 *best2, hipStream_t st, bool keep = false)
{
    SgmPathGeom g;
    g.w = plan->width; g.h = plan->height; g.D = plan->num_shifts; g.Dp = sgm_padded_shifts(plan);
    g.p1 = p1; g.p2 = p2;
    g.mirror = mirror;
    g.map = (long long)pair * g.w * g.h;
    const int K = g.Dp / 64;
    const u16 *A = (const u16 *)plan->d_sgm;
    i32 *S = (i32 *)((char *)plan->d_sgm + (size_t)2 * g.w * g.h * g.Dp);
    for (int r = 0; r < paths; r++) {
        sm_sgm_direction(paths, r, g.w, g.h, &g.dx, &g.dy, &g.lines);
        const int mode = r == 0 ? SGM_FIRST : r == paths - 1 && !keep ? SGM_LAST : SGM_MID;
        const void *fn = K == 1 ? sgm_path_ptr<1>(mode) : K == 2 ? sgm_path_ptr<2>(mode) : sgm_path_ptr<4>(mode);
        // (paths >= 4: the last direction is never the first, so S always holds the other directions' sum)
        void *args[] = {(void *)&A, (void *)&S, (void *)&web, (void *)&best, (void *)&sub, (void *)&g};
        void *args_second[] = {(void *)&A, (void *)&S, (void *)&web, (void *)&best, (void *)&sub, (void *)&web2,
                               (void *)&best2, (void *)&g};
        const bool second = web2 && mode == SGM_LAST;
        if (second)
            fn = K == 1 ? (const void *)k_sgm_path_second<1> : K == 2 ? (const void *)k_sgm_path_second<2>
                                                                      : (const void *)k_sgm_path_second<4>;
        const hipError_t e = hipLaunchKernel(fn, dim3((g.lines + 3) / 4), dim3(256), second ? args_second : args, 0, st);
        if (e != hipSuccess)
            return sm_fail(SM_ERR_HIP, "launch of %s failed: %s", second ? "k_sgm_path_second" : "k_sgm_path",
                           hipGetErrorString(e));
    }
    return SM_OK;
}

// the left (or right-reference) SGM maps of `pairs` pairs, one pair at a time through the volumes
static int sgm_pass(const sm_plan *plan, int cw, int p1, int p2, int paths, bool mirror, int pairs, i32 *web, i32 *best,
                    int16_t *sub, hipStream_t st, i32 *web2 = nullptr, i32 *best2 = nullptr)
{
    for (int q = 0; q < pairs; q++) {
        SM_TRY(sgm_cost_launch(plan, cw, mirror, q, st));
        SM_TRY(sgm_paths_launch(plan, p1, p2, paths, mirror, q, web, best, sub, web2, best2, st));
    }
    return SM_OK;
}

// for sm_unique.hip (sm_sgm_wta2): the checks of every SGM entry, and the left pass with the runner-up maps
int sm_sgm_args(const sm_plan *plan, int census_width, int p1, int p2, int paths, int pairs, const char *me)
{
    return sgm_args(plan, census_width, p1, p2, paths, pairs, me);
}

int sm_sgm_second_pass(const sm_plan *plan, int cw, int p1, int p2, int paths, int pairs, i32 *web, i32 *best,
                       int16_t *sub, i32 *web2, i32 *best2, hipStream_t st)
{
    return sgm_pass(plan, cw, p1, p2, paths, false, pairs, web, best, sub, st, web2, best2);
}

// for sm_sgm_both.hip: the data term and every direction of pair `pair`, the last one as k_sgm_path<K, SGM_MID>, so that
// the aggregate volume holds the full S afterwards: *S its [H][W][*Dp] int32 entries (entries d >= D are not costs)
int sm_sgm_volume_pass(const sm_plan *plan, int cw, int p1, int p2, int paths, int pair, const i32 **S, int *Dp,
                       hipStream_t st)
{
    *Dp = sgm_padded_shifts(plan);
    *S = (const i32 *)((const char *)plan->d_sgm + (size_t)2 * plan->width * plan->height * *Dp);
    SM_TRY(sgm_cost_launch(plan, cw, false, pair, st));
    return sgm_paths_launch(plan, p1, p2, paths, false, pair, nullptr, nullptr, nullptr, nullptr, nullptr, st, true);
}

// the mode as the entry driver sees it (sm_entry.h)
struct SgmMode : sm_mode {
    static constexpr const sm_ws_set &ws = SM_WS_SET_SGM;
    static constexpr bool overlap_names_maps = false;
    int cw, p1, p2, paths;
    SgmMode(int census_width, int p1_, int p2_, int paths_) : cw(census_width), p1(p1_), p2(p2_), paths(paths_) {}
    int args(const sm_call &c) const { return sgm_args(c.plan, cw, p1, p2, paths, c.pairs, c.me); }
    int prepare(const sm_call &c) const { return sm_census_descriptors(c.plan, cw, c.left, c.right, c.pairs, c.st); }
    int pass(const sm_call &c, bool mirror, i32 *web, i32 *best, int16_t *sub) const
    {
        return sgm_pass(c.plan, cw, p1, p2, paths, mirror, c.pairs, web, best, sub, c.st);
    }
};

extern "C" int sm_sgm_wta(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width,
                          int p1, int p2, int paths, int pairs, int32_t *d_web, int32_t *d_best, int16_t *d_sub,
                          void *stream)
{
    return sm_entry_one({"sm_sgm_wta", plan, d_gray_left, d_gray_right, pairs, (hipStream_t)stream},
                        SgmMode(census_width, p1, p2, paths), false, d_web, d_best, d_sub);
}

extern "C" int sm_sgm_wta_right(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right,
                                int census_width, int p1, int p2, int paths, int pairs, int32_t *d_web_right,
                                int32_t *d_best_right, void *stream)
{
    return sm_entry_one({"sm_sgm_wta_right", plan, d_gray_left, d_gray_right, pairs, (hipStream_t)stream},
                        SgmMode(census_width, p1, p2, paths), true, d_web_right, d_best_right, nullptr);
}

extern "C" int sm_sgm_lr(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width,
                         int p1, int p2, int paths, int pairs, int max_diff, int32_t *d_web, int32_t *d_best,
                         int32_t *d_web_right, int32_t *d_rejected, int16_t *d_sub, void *stream)
{
    return sm_entry_lr({"sm_sgm_lr", plan, d_gray_left, d_gray_right, pairs, (hipStream_t)stream},
                       SgmMode(census_width, p1, p2, paths), max_diff, d_web, d_best, d_web_right, d_rejected, d_sub);
}
