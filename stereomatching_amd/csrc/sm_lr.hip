// sm_lr.hip -- left-right consistency check: the right-reference map and the check that hands
// the rejected pixels of the left map to hole filling (include/stereo_hip.h).
//
// The right-reference map is the plan's own match launch run over MIRRORED packed images:
//     web_right = mirror(hot_path(mirror(eR), mirror(eL)))
// (mirror(a)(x) = a(W-1-x)).  Both borders are symmetric under mirroring -- the ghost border's zero
// halo and "no taps outside the image", the centre-match mask, last-shift-wins ties -- so every
// kernel variant the plan can choose gets a right-reference mode without a new instantiation.
// The new kernels: k_mirror_ext (packed images -> mirrored packed images, a row of words in
// reverse order, each bit-reversed) and k_lr_check (one pass over the left map, bandwidth bound).
//
// The SAD / SSD cost mode's check is the same construction on the gray images:
//     web_right = mirror(cost_hot_path(mirror(R), mirror(L)))
// by the plan's own sm_cost_wta launch over the images k_mirror_gray writes -- every cost kernel
// (quad-SAD, matrix-core SSD, the ghost strip, the general kernel) without a new instantiation --
// then the same k_lr_check.

#include "sm_device.h"
#include "sm_entry.h"

#include <algorithm>

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------

__device__ __forceinline__ int lr_pos_mod(int v, int m)
{
    int r = v % m;
    return r < 0 ? r + m : r;
}

// Mirrored packed images from the plan's packed images (layout in sm_internal.h), one lane per
// output word.  Output side 0 (the reference image of the right-reference pass) is mirror(right),
// side 1 is mirror(left); each keeps the row extents the edge kernels give the side it stands in
// for (edge_words_l / _r: the words beyond stay zero, as in the plan's own images).
//
// Output bit b of word k is image column x = 32k + b - pad_l and takes source column W-1-x.  Where
// all 32 columns of the word lie inside the image, those are 32 consecutive source bits, read from
// two neighbouring words (realigned by W mod 32 -- pad_l is a multiple of 32 -- with v_alignbit_b32)
// and reversed with v_bfrev_b32.  The few words that reach into the halo apply the border bit by
// bit: the toroidal halo wraps (mod W), the ghost halo is zero.  Rows need nothing: the halo rows
// of the source are already the border's, and mirroring is horizontal.  Every source read is of a
// column in [0, W), i.e. bit pad_l .. pad_l + W - 1 of the row, inside edge_words_l words.
__global__ __launch_bounds__(64) void k_mirror_ext(const u32 *__restrict__ src, u32 *__restrict__ dst,
                                                    MatchGeom g, int ghost)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int e = blockIdx.y;
    const int side = blockIdx.z & 1, pair = blockIdx.z >> 1;
    if (k >= (side ? g.edge_words_r : g.edge_words_l)) return;
    const u32 *s = src + ((long long)(2 * pair + (side ^ 1)) * g.ext_rows + e) * g.ext_words;
    u32 *d = dst + ((long long)(2 * pair + side) * g.ext_rows + e) * g.ext_words;
    const int W = g.w;
    const int x0 = 32 * k - g.pad_l;
    u32 v = 0;
    if (x0 >= 0 && x0 + 31 < W) {
        const int p = W - 32 - x0 + g.pad_l;           // source bit of output bit 31
        const int lo = p >> 5, sh = p & 31;
        const u32 a = s[lo];
        const u32 b = sh ? s[lo + 1] : 0u;             // (p + 31 <= pad_l + W - 1: inside the row)
        v = __builtin_bitreverse32(__builtin_amdgcn_alignbit(b, a, sh));
    } else {
        // source column of bit 0, then one column to the left per bit (toroidal: wrapping round; ghost: columns
        // outside the image are 0): no division per bit, and 32 independent loads
        int xs = ghost ? W - 1 - x0 : lr_pos_mod(W - 1 - x0, W);
#pragma unroll
        for (int b = 0; b < 32; b++) {
            const bool in = !ghost || (xs >= 0 && xs < W);
            const int q = (in ? xs : 0) + g.pad_l;
            v |= (in ? (s[q >> 5] >> (q & 31)) & 1u : 0u) << b;
            xs = (!ghost && xs == 0) ? W - 1 : xs - 1;
        }
    }
    d[k] = v;
}

// Is left pixel x of a row, whose map value is s, consistent with the right-reference row `rrow`?
// u = x + s - 1 is the right pixel it matched: toroidal u mod W; ghost: past the row (the halo, or
// before column 0 for values no match produces) = rejected.  MIRRORED: rrow is in mirrored order.
template <bool MIRRORED>
__device__ __forceinline__ bool lr_keep(const i32 *rrow, int x, i32 s, int W, int ghost, int max_diff)
{
    long long u = (long long)x + s - 1;
    if (u < 0 || u >= W) {
        if (ghost) return false;
        u %= W;
        if (u < 0) u += W;
    }
    const int ui = (int)u;
    const long long diff = (long long)rrow[MIRRORED ? W - 1 - ui : ui] - s;
    return (diff < 0 ? -diff : diff) <= max_diff;
}


// the per-pair counts k_lr_check adds to, zeroed by a kernel rather than hipMemsetAsync: captured into a graph, the
// memset of these 4-byte counts filled them with 0x08080808 instead of 0 on the second replay (measured on MI355X,
// DESIGN.md section 12); a kernel node replays as captured
__global__ __launch_bounds__(64) void k_lr_zero_counts(i32 *rejected, int pairs)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < pairs) rejected[i] = 0;
}

// The check, one pass over the left map: web (in place allowed: out == web, so neither is
// __restrict__), the gather from the right-reference row, out, and -- MIRRORED, right_out
// non-NULL -- the right-reference map in natural order.  Grid: x strides over the pixels of one
// pair, four per lane (VEC: W % 4 == 0 and 16-byte aligned maps: one int4 per map) or one; y = pair.
template <bool MIRRORED, bool VEC>
__global__ __launch_bounds__(256) void k_lr_check(const i32 *web, const i32 *right, i32 *out, i32 *right_out,
                                                  i32 *rejected, int W, unsigned npx, int max_diff, int ghost)
{
    const size_t base = (size_t)blockIdx.y * npx;
    constexpr int P = VEC ? 4 : 1;
    const unsigned lanes = npx / P;
    int cnt = 0;
    for (unsigned t = blockIdx.x * 256u + threadIdx.x; t < lanes; t += gridDim.x * 256u) {
        const unsigned p = t * P;
        const unsigned row = p / (unsigned)W;
        const int x = (int)(p - row * (unsigned)W);
        const i32 *rrow = right + base + (size_t)row * W;
        if (VEC) {
            const int4 s = *(const int4 *)(web + base + p);
            const bool k0 = lr_keep<MIRRORED>(rrow, x, s.x, W, ghost, max_diff);
            const bool k1 = lr_keep<MIRRORED>(rrow, x + 1, s.y, W, ghost, max_diff);
            const bool k2 = lr_keep<MIRRORED>(rrow, x + 2, s.z, W, ghost, max_diff);
            const bool k3 = lr_keep<MIRRORED>(rrow, x + 3, s.w, W, ghost, max_diff);
            *(int4 *)(out + base + p) = make_int4(k0 ? s.x : 0, k1 ? s.y : 0, k2 ? s.z : 0, k3 ? s.w : 0);
            cnt += 4 - (int)k0 - (int)k1 - (int)k2 - (int)k3;
            if (MIRRORED && right_out) {
                const int4 r = *(const int4 *)(rrow + (W - 4 - x));
                *(int4 *)(right_out + base + p) = make_int4(r.w, r.z, r.y, r.x);
            }
        } else {
            const i32 s = web[base + p];
            const bool keep = lr_keep<MIRRORED>(rrow, x, s, W, ghost, max_diff);
            out[base + p] = keep ? s : 0;
            cnt += !keep;
            if (MIRRORED && right_out) right_out[base + p] = rrow[W - 1 - x];
        }
    }
    if (rejected) lr_count(rejected + blockIdx.y, cnt);
}

// sm_match_wta_right: the match launch wrote both maps in mirrored order; reverse every row in place
__global__ __launch_bounds__(256) void k_lr_unmirror(i32 *web, i32 *best, int W, unsigned npx, unsigned half_w,
                                                     unsigned half_px)
{
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= half_px) return;
    const unsigned row = t / half_w;
    const int x = (int)(t - row * half_w);
    const size_t o = (size_t)blockIdx.y * npx + (size_t)row * W;
    i32 *r = web + o;
    const i32 a = r[x], b = r[W - 1 - x];
    r[x] = b;
    r[W - 1 - x] = a;
    if (best) {
        i32 *q = best + o;
        const i32 c = q[x], d = q[W - 1 - x];
        q[x] = d;
        q[W - 1 - x] = c;
    }
}

// Mirrored gray images for the cost mode's right-reference pass (sm_cost_wta_right, sm_cost_lr): output
// side 0 (the pass's "left" batch) is mirror(R), side 1 is mirror(L), each row reversed byte by byte.
// Grid: x = image row of the batch (pair * H + y), y = 256-unit segment of the row, z = side.  A lane
// moves V bytes: 16 where W % 16 == 0 (and the inputs are 16-byte aligned; 4K rows), 4 where
// W % 4 == 0, else 1.  Lane j of a row writes unit j and reads unit W/V - 1 - j: the wave's loads and
// its stores each cover one contiguous span (1 KiB at V = 16), the loads in descending order.  A unit
// is reversed in registers: the dwords in reverse order, each byte-reversed with v_perm_b32.  Rows of
// V = 16 and V = 4 start V-aligned because W is a multiple of V and the bases are (checked by the host;
// the output batches are 256-byte aligned).
__device__ __forceinline__ u32 lr_bswap(u32 v) { return __builtin_amdgcn_perm(v, v, 0x00010203u); }

template <int V>
__global__ __launch_bounds__(256) void k_mirror_gray(const u8 *__restrict__ left, const u8 *__restrict__ right,
                                                     u8 *__restrict__ dst, size_t batch_stride, int W)
{
    const int units = W / V;
    const int j = blockIdx.y * 256 + threadIdx.x;
    if (j >= units) return;
    const int side = blockIdx.z;
    const size_t row = (size_t)blockIdx.x * W;
    const u8 *s = (side ? left : right) + row;
    u8 *d = dst + side * batch_stride + row;
    const int k = units - 1 - j;
    if constexpr (V == 16) {
        const uint4 v = reinterpret_cast<const uint4 *>(s)[k];
        reinterpret_cast<uint4 *>(d)[j] = make_uint4(lr_bswap(v.w), lr_bswap(v.z), lr_bswap(v.y), lr_bswap(v.x));
    } else if constexpr (V == 4) {
        reinterpret_cast<u32 *>(d)[j] = lr_bswap(reinterpret_cast<const u32 *>(s)[k]);
    } else {
        d[j] = s[k];
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

extern "C" int sm_plan_reserve_lr(sm_plan *plan)
{
    if (!plan) return sm_fail(SM_ERR_ARG, "sm_plan_reserve_lr: plan is NULL");
    SM_TRY(sm_use_device(plan->device));
    return sm_ws_reserve(plan, SM_WS_SET_LR, "sm_plan_reserve_lr");
}

// one launch of the plan's match kernel over other packed images (the plan is not modified)
static int lr_match(const sm_plan *plan, u32 *ext, int pairs, i32 *d_web, i32 *d_best, hipStream_t st)
{
    sm_plan view = *plan;
    view.d_ext = ext;
    return sm_match_launch(&view, sm_match_launch_args(plan, d_web, d_best, 4), pairs, d_web, d_best, st);
}

static int lr_mirror(sm_plan *plan, int pairs, hipStream_t st)
{
    const MatchGeom &g = plan->g;
    // one wave per row segment of 64 words (a row is 2 -- 4K, 128 shifts -- to ~70 words: wider workgroups idle)
    const dim3 grid((g.edge_words_r + 63) / 64, g.ext_rows, pairs * 2), block(64);
    hipLaunchKernelGGL(k_mirror_ext, grid, block, 0, st, plan->d_ext, plan->d_ext_lr, g, plan->border == SM_GHOST ? 1 : 0);
    SM_LAUNCH_CHECK("k_mirror_ext");
    return SM_OK;
}

// the per-pair counts a kernel adds to, zeroed (k_lr_zero_counts: a kernel launch, also inside a capture)
int sm_lr_zero_counts(i32 *counts, int pairs, hipStream_t st)
{
    hipLaunchKernelGGL(k_lr_zero_counts, dim3((pairs + 63) / 64), dim3(64), 0, st, counts, pairs);
    SM_LAUNCH_CHECK("k_lr_zero_counts");
    return SM_OK;
}

int sm_lr_check_launch(const sm_plan *plan, bool mirrored, const i32 *web, const i32 *right, i32 *out, i32 *right_out,
                       i32 *rejected, int max_diff, int pairs, hipStream_t st)
{
    const int W = plan->width;
    const unsigned npx = (unsigned)W * plan->height;
    const int ghost = plan->border == SM_GHOST;
    if (rejected) SM_TRY(sm_lr_zero_counts(rejected, pairs, st));
    const bool vec = W % 4 == 0 && (((uintptr_t)web | (uintptr_t)right | (uintptr_t)out | (uintptr_t)right_out) & 15) == 0;
    const unsigned lanes = vec ? npx / 4 : npx;
    const dim3 grid(std::min((lanes + 255) / 256, (unsigned)SM_LR_BLOCKS), pairs), block(256);
#define SM_LR_GO(M, V) hipLaunchKernelGGL((k_lr_check<M, V>), grid, block, 0, st, web, right, out, right_out, rejected, \
                                          W, npx, max_diff, ghost)
    if (mirrored) { if (vec) SM_LR_GO(true, true); else SM_LR_GO(true, false); }
    else          { if (vec) SM_LR_GO(false, true); else SM_LR_GO(false, false); }
#undef SM_LR_GO
    SM_LAUNCH_CHECK("k_lr_check");
    return SM_OK;
}

// a right-reference launch wrote both maps in mirrored order: every row is turned round in place
int sm_lr_unmirror(const sm_plan *plan, int pairs, i32 *d_web_right, i32 *d_best_right, hipStream_t st)
{
    const int W = plan->width;
    const unsigned half_w = (unsigned)(W + 1) / 2, half_px = half_w * plan->height;
    hipLaunchKernelGGL(k_lr_unmirror, dim3((half_px + 255) / 256, pairs), dim3(256), 0, st, d_web_right, d_best_right,
                       W, (unsigned)W * plan->height, half_w, half_px);
    SM_LAUNCH_CHECK("k_lr_unmirror");
    return SM_OK;
}

extern "C" int sm_match_wta_right(sm_plan *plan, int pairs, int32_t *d_web_right, int32_t *d_best_right, void *stream)
{
    const char *me = "sm_match_wta_right";
    if (!d_web_right) return sm_fail(SM_ERR_ARG, "%s: d_web_right is NULL", me);
    SM_TRY(sm_check_pairs(plan, pairs, me));
    SM_TRY(sm_check_pairs_loaded(plan, pairs, me));
    const size_t map = (size_t)pairs * plan->width * plan->height * sizeof(i32);
    if (d_best_right && overlap(d_web_right, d_best_right, map))
        return sm_fail(SM_ERR_ARG, "%s: d_web_right and d_best_right overlap", me);
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    SM_TRY(sm_ws_need(plan, SM_WS_SET_LR, st, me));
    SM_TRY(sm_lanes_fence(plan, st));
    sm_lanes_release(plan);
    SM_TRY(lr_mirror(plan, pairs, st));
    // the maps come out in mirrored order, and are turned round in place
    SM_TRY(lr_match(plan, plan->d_ext_lr, pairs, d_web_right, d_best_right, st));
    return sm_lr_unmirror(plan, pairs, d_web_right, d_best_right, st);
}

extern "C" int sm_lr_check(sm_plan *plan, const int32_t *d_web, const int32_t *d_web_right, int max_diff,
                           int pairs, int32_t *d_web_out, int32_t *d_rejected, void *stream)
{
    const char *me = "sm_lr_check";
    if (!d_web || !d_web_right || !d_web_out) return sm_fail(SM_ERR_ARG, "%s: a map pointer is NULL", me);
    if (max_diff < 0) return sm_fail(SM_ERR_ARG, "%s: max_diff %d is negative", me, max_diff);
    SM_TRY(sm_check_pairs(plan, pairs, me));
    const size_t map = (size_t)pairs * plan->width * plan->height * sizeof(i32);
    if (overlap(d_web_right, d_web_out, map))
        return sm_fail(SM_ERR_ARG, "%s: d_web_right overlaps d_web_out (the check gathers from it while writing)", me);
    if (d_web != d_web_out && overlap(d_web, d_web_out, map))
        return sm_fail(SM_ERR_ARG, "%s: d_web_out overlaps d_web without being it", me);
    const size_t counts = (size_t)pairs * sizeof(i32);
    if (d_rejected && (overlap(d_rejected, d_web_out, counts, map) || overlap(d_rejected, d_web_right, counts, map) ||
                       overlap(d_rejected, d_web, counts, map)))
        return sm_fail(SM_ERR_ARG, "%s: d_rejected overlaps a map", me);
    SM_TRY(sm_use_device(plan->device));
    return sm_lr_check_launch(plan, false, d_web, d_web_right, d_web_out, nullptr, d_rejected, max_diff, pairs,
                              (hipStream_t)stream);
}

extern "C" int sm_run_lr(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, double threshold,
                         int pairs, int max_diff, int32_t *d_web, int32_t *d_best, int32_t *d_web_right,
                         int32_t *d_rejected, void *stream)
{
    const char *me = "sm_run_lr";
    if (!d_gray_left || !d_gray_right) return sm_fail(SM_ERR_ARG, "%s: input image pointer is NULL", me);
    SM_TRY(sm_check_threshold(threshold, me));
    if (!d_web) return sm_fail(SM_ERR_ARG, "%s: d_web is NULL", me);
    if (max_diff < 0) return sm_fail(SM_ERR_ARG, "%s: max_diff %d is negative", me, max_diff);
    SM_TRY(sm_check_pairs(plan, pairs, me));
    SM_TRY(sm_check_lr_maps(plan, pairs, d_web, d_best, d_web_right, nullptr, d_rejected, me));
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    if (sm_stream_capturing(st)) SM_TRY(sm_check_tables_prepared(plan, threshold, me));
    SM_TRY(sm_ws_need(plan, SM_WS_SET_LR, st, me));
    SM_TRY(sm_lanes_fence(plan, st));
    sm_lanes_release(plan);
    // edges into the plan's packed images (as sm_run; they stay loaded), the left match, the mirrored images,
    // the right match into the mirrored-order map, and the check, which gathers from that map
    SM_TRY(sm_find_edges(plan, d_gray_left, d_gray_right, threshold, pairs, nullptr, nullptr, stream));
    SM_TRY(lr_match(plan, plan->d_ext, pairs, d_web, d_best, st));
    SM_TRY(lr_mirror(plan, pairs, st));
    SM_TRY(lr_match(plan, plan->d_ext_lr, pairs, plan->d_web_lr, nullptr, st));
    return sm_lr_check_launch(plan, true, d_web, plan->d_web_lr, d_web, d_web_right, d_rejected, max_diff, pairs, st);
}

// ---------------------------------------------------------------------------
// the SAD / SSD cost mode's check
// ---------------------------------------------------------------------------

extern "C" int sm_plan_reserve_cost_lr(sm_plan *plan)
{
    if (!plan) return sm_fail(SM_ERR_ARG, "sm_plan_reserve_cost_lr: plan is NULL");
    SM_TRY(sm_use_device(plan->device));
    return sm_ws_reserve(plan, SM_WS_SET_COST_LR, "sm_plan_reserve_cost_lr");
}

// what the cost entries check besides their maps (before any device call): cost, plan, pairs, the general kernel's reach
static int cost_lr_args(const sm_plan *plan, int cost, int pairs, const char *me)
{
    if (cost != SM_COST_SAD && cost != SM_COST_SSD)
        return sm_fail(SM_ERR_ARG, "%s: cost %d is neither SM_COST_SAD nor SM_COST_SSD", me, cost);
    SM_TRY(sm_check_pairs(plan, pairs, me));
    return sm_check_reach(plan, 512, me);
}

// k_mirror_gray: mirror(right) into the workspace's first batch, mirror(left) into its second; returns the two
static int cost_lr_mirror(sm_plan *plan, const uint8_t *left, const uint8_t *right, int pairs, hipStream_t st,
                          const u8 **mleft, const u8 **mright)
{
    const int W = plan->width;
    const size_t batch = sm_lr_gray_batch_bytes(plan);
    const uintptr_t a = (uintptr_t)left | (uintptr_t)right;
    const int v = W % 16 == 0 && (a & 15) == 0 ? 16 : W % 4 == 0 && (a & 3) == 0 ? 4 : 1;
    const dim3 grid((unsigned)pairs * plan->height, (W / v + 255) / 256, 2), block(256);
    if (v == 16) hipLaunchKernelGGL(k_mirror_gray<16>, grid, block, 0, st, left, right, plan->d_gray_lr, batch, W);
    else if (v == 4) hipLaunchKernelGGL(k_mirror_gray<4>, grid, block, 0, st, left, right, plan->d_gray_lr, batch, W);
    else hipLaunchKernelGGL(k_mirror_gray<1>, grid, block, 0, st, left, right, plan->d_gray_lr, batch, W);
    SM_LAUNCH_CHECK("k_mirror_gray");
    *mleft = plan->d_gray_lr;
    *mright = plan->d_gray_lr + batch;
    return SM_OK;
}

// the mode as the entry driver sees it (sm_entry.h): nothing shared between the directions; the right-reference pass
// is the plan's cost launch over the mirrored images, which leaves its maps in mirrored order
struct CostMode : sm_mode {
    static constexpr const sm_ws_set &ws = SM_WS_SET_COST_LR;
    static constexpr bool right_mirrored = true;
    int cost;
    explicit CostMode(int cost_) : cost(cost_) {}
    // (the modes differ here: sm_check_reach runs in cost_lr_args and again inside every sm_cost_wta of a pass)
    int args(const sm_call &c) const { return cost_lr_args(c.plan, cost, c.pairs, c.me); }
    int pass(const sm_call &c, bool mirror, i32 *web, i32 *best, int16_t *) const
    {
        const u8 *l = c.left, *r = c.right;
        if (mirror) SM_TRY(cost_lr_mirror(c.plan, c.left, c.right, c.pairs, c.st, &l, &r));
        return sm_cost_wta(c.plan, l, r, cost, c.pairs, web, best, c.st);
    }
};

extern "C" int sm_cost_wta_right(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int cost,
                                 int pairs, int32_t *d_web_right, int32_t *d_best_right, void *stream)
{
    return sm_entry_one({"sm_cost_wta_right", plan, d_gray_left, d_gray_right, pairs, (hipStream_t)stream},
                        CostMode(cost), true, d_web_right, d_best_right, nullptr);
}

extern "C" int sm_cost_lr(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int cost, int pairs,
                          int max_diff, int32_t *d_web, int32_t *d_best, int32_t *d_web_right, int32_t *d_rejected,
                          void *stream)
{
    return sm_entry_lr({"sm_cost_lr", plan, d_gray_left, d_gray_right, pairs, (hipStream_t)stream}, CostMode(cost),
                       max_diff, d_web, d_best, d_web_right, d_rejected, nullptr);
}
