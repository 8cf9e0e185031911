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

#include "sm_internal.h"

#include <string.h>

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

// The workgroup's rejections, added to the pair's count with ONE atomic: a sum across each wave (DPP / shuffles),
// then across the four waves in LDS.  All atomics of a pair go to one address, where they serialise: one per
// wave of four pixels per lane cost ~11 ns each, 0.35 ms at 4K (32 K waves) -- hence workgroups that stride
// over the map (SM_LR_BLOCKS per pair) and one atomic per workgroup.
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

// the post-filters (median, speckle removal): kernels; their entry points are at the end of this file
#include "sm_filter.h"
// occlusion-aware interpolation: kernels; their entry points follow the post-filters'
#include "sm_interp.h"
// rectification (the stage in front of the matchers): kernels; their entry points are the last of this file
#include "sm_rectify.h"

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

static size_t lr_map_bytes(const sm_plan *plan)
{
    return (size_t)plan->max_pairs * plan->width * plan->height * sizeof(i32);
}

// one batch of mirrored gray images (sm_cost_lr), rounded up so that the second batch starts 256-byte aligned
static size_t lr_gray_batch_bytes(const sm_plan *plan)
{
    return ((size_t)plan->max_pairs * plan->width * plan->height + 255) & ~(size_t)255;
}

// sm_interpolate's workspace (sm_interp.h), in 4-byte elements per pair: six directional maps, the carries of
// W + H - 1 lines for six directions and every segment, the carries of every row chunk from either side
static int itp_segs(const sm_plan *plan) { return (plan->height + ITP_SEG - 1) / ITP_SEG; }
static int itp_chunks(const sm_plan *plan) { return (plan->width + ITP_CW - 1) / ITP_CW; }
static size_t itp_loc_elems(const sm_plan *plan) { return (size_t)6 * plan->width * plan->height; }
static size_t itp_car_elems(const sm_plan *plan)
{
    return (size_t)6 * itp_segs(plan) * (plan->width + plan->height - 1);
}
static size_t itp_row_elems(const sm_plan *plan) { return (size_t)2 * plan->height * itp_chunks(plan); }
static size_t itp_bytes(const sm_plan *plan)
{
    return (size_t)plan->max_pairs * sizeof(i32) * (itp_loc_elems(plan) + itp_car_elems(plan) + itp_row_elems(plan));
}

size_t sm_lr_workspace_bytes(const sm_plan *plan)
{
    return (plan->d_ext_lr ? plan->ext_bytes : 0) + (plan->d_web_lr ? lr_map_bytes(plan) : 0) +
           (plan->d_gray_lr ? 2 * lr_gray_batch_bytes(plan) : 0) + (plan->d_filter ? 2 * lr_map_bytes(plan) : 0) +
           (plan->d_interp ? itp_bytes(plan) : 0);
}

void sm_lr_free(sm_plan *plan)
{
    if (plan->d_ext_lr) (void)hipFree(plan->d_ext_lr);
    if (plan->d_web_lr) (void)hipFree(plan->d_web_lr);
    if (plan->d_gray_lr) (void)hipFree(plan->d_gray_lr);
    plan->d_ext_lr = nullptr;
    plan->d_web_lr = nullptr;
    plan->d_gray_lr = nullptr;
    if (plan->d_filter) (void)hipFree(plan->d_filter);
    plan->d_filter = nullptr;
    if (plan->d_interp) (void)hipFree(plan->d_interp);
    plan->d_interp = nullptr;
}

// `*buf` (bytes long) and, if the plan has none yet, the mirrored-order map shared by both checks; on failure
// neither is kept (what the plan had before stays)
static int reserve_with_map(sm_plan *plan, void **buf, size_t bytes, bool zero, const char *what, const char *me)
{
    void *b = nullptr, *map = nullptr;
    const bool need_map = !plan->d_web_lr;
    hipError_t e = hipMalloc(&b, bytes);
    if (e == hipSuccess && zero) e = hipMemset(b, 0, bytes);
    if (e == hipSuccess && need_map) e = hipMalloc(&map, lr_map_bytes(plan));
    if (e != hipSuccess) {
        if (b) (void)hipFree(b);
        if (map) (void)hipFree(map);
        return sm_fail(e == hipErrorOutOfMemory ? SM_ERR_NOMEM : SM_ERR_HIP, "%s: %zu bytes for the %s and map of the "
                       "consistency check: %s", me, bytes + (need_map ? lr_map_bytes(plan) : 0), what, hipGetErrorString(e));
    }
    *buf = b;
    if (need_map) plan->d_web_lr = (i32 *)map;
    return SM_OK;
}

// the mirrored packed images (zero-filled: the words beyond each side's row extent stay zero) and the
// mirrored-order map
static int reserve_lr(sm_plan *plan, const char *me)
{
    if (plan->d_ext_lr) return SM_OK;
    return reserve_with_map(plan, (void **)&plan->d_ext_lr, plan->ext_bytes, true, "mirrored images", me);
}

// the mirrored gray images (every byte a cost launch reads is written by k_mirror_gray first) and the map
static int reserve_cost_lr(sm_plan *plan, const char *me)
{
    if (plan->d_gray_lr) return SM_OK;
    return reserve_with_map(plan, (void **)&plan->d_gray_lr, 2 * lr_gray_batch_bytes(plan), false,
                            "mirrored gray images", me);
}

extern "C" int sm_plan_reserve_lr(sm_plan *plan)
{
    if (!plan) return sm_fail(SM_ERR_ARG, "sm_plan_reserve_lr: plan is NULL");
    SM_TRY(sm_use_device(plan->device));
    return reserve_lr(plan, "sm_plan_reserve_lr");
}

static int check_pairs(const sm_plan *plan, int pairs, const char *me)
{
    if (!plan) return sm_fail(SM_ERR_ARG, "%s: plan is NULL", me);
    if (pairs < 1 || pairs > plan->max_pairs)
        return sm_fail(SM_ERR_ARG, "%s: pairs %d outside 1..%d (max_pairs of the plan)", me, pairs, plan->max_pairs);
    return SM_OK;
}

// the workspace, allocated here when sm_plan_reserve_lr was not called -- unless the stream is capturing
static int need_lr(sm_plan *plan, hipStream_t st, const char *me)
{
    if (plan->d_ext_lr) return SM_OK;
    if (sm_stream_capturing(st))
        return sm_fail(SM_ERR_ARG, "%s: the workspace of the consistency check is not allocated and the stream is capturing "
                       "(an allocation cannot be captured): call sm_plan_reserve_lr(plan) first", me);
    return reserve_lr(plan, me);
}

// A call that reads or rewrites the packed images runs on `stream`; the pipelined calls before it may
// still be running on the plan's lanes (sm_plan_set_pipelined, sm_run_after): `stream` waits for all of
// them.  Inside a capture the captured calls have joined `stream` already (and events of eager calls
// must not be waited for there).
static int lr_fence_lanes(sm_plan *plan, hipStream_t st)
{
    if (sm_stream_capturing(st)) return SM_OK;
    for (int i = 0; i < 4; i++)
        if (plan->ev_free_set[i]) SM_HIP(hipStreamWaitEvent(st, plan->ev_free[i], 0));
    return SM_OK;
}

// ... and the next pipelined call must not overtake it: as after any sequential launch, its lanes wait for
// `stream` first (a captured one leaves `stream` after this call, not where the previous captured call ended)
static void lr_release_lanes(sm_plan *plan)
{
    plan->unfenced = 1;
    plan->cap_live = 0;
}

// one launch of the plan's match kernel over other packed images (the plan is not modified)
static int lr_match(const sm_plan *plan, u32 *ext, int pairs, i32 *d_web, i32 *d_best, hipStream_t st)
{
    sm_plan view = *plan;
    view.d_ext = ext;
    MatchLaunch l;
    l.g = plan->g;
    if (((uintptr_t)d_web & 15) != 0 || ((uintptr_t)d_best & 15) != 0) l.g.vec_ok = 0;
    l.g.web_bytes = 4;
    l.ev_begin = l.ev_end = nullptr;
    return sm_match_launch(&view, l, pairs, d_web, d_best, st);
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

static int lr_check_launch(const sm_plan *plan, bool mirrored, const i32 *web, const i32 *right, i32 *out,
                           i32 *right_out, i32 *rejected, int max_diff, int pairs, hipStream_t st)
{
    const int W = plan->width;
    const unsigned npx = (unsigned)W * plan->height;
    const int ghost = plan->border == SM_GHOST;
    if (rejected) {
        hipLaunchKernelGGL(k_lr_zero_counts, dim3((pairs + 63) / 64), dim3(64), 0, st, rejected, pairs);
        SM_LAUNCH_CHECK("k_lr_zero_counts");
    }
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

// do [a, a + a_bytes) and [b, b + b_bytes) share a byte?  (b_bytes = 0: as many as a)
static bool overlap(const void *a, const void *b, size_t a_bytes, size_t b_bytes = 0)
{
    return (uintptr_t)a < (uintptr_t)b + (b_bytes ? b_bytes : a_bytes) && (uintptr_t)b < (uintptr_t)a + a_bytes;
}

extern "C" int sm_match_wta_right(sm_plan *plan, int pairs, int32_t *d_web_right, int32_t *d_best_right, void *stream)
{
    const char *me = "sm_match_wta_right";
    if (!d_web_right) return sm_fail(SM_ERR_ARG, "%s: d_web_right is NULL", me);
    SM_TRY(check_pairs(plan, pairs, me));
    if (pairs > plan->pairs_loaded)
        return sm_fail(SM_ERR_ARG, "%s: %d pairs requested but edges of only %d are loaded "
                       "(call sm_find_edges or sm_load_edges first)", me, pairs, plan->pairs_loaded);
    const size_t map = (size_t)pairs * plan->width * plan->height * sizeof(i32);
    if (d_best_right && overlap(d_web_right, d_best_right, map))
        return sm_fail(SM_ERR_ARG, "%s: d_web_right and d_best_right overlap", me);
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    SM_TRY(need_lr(plan, st, me));
    SM_TRY(lr_fence_lanes(plan, st));
    lr_release_lanes(plan);
    SM_TRY(lr_mirror(plan, pairs, st));
    // the maps come out in mirrored order, and are turned round in place
    SM_TRY(lr_match(plan, plan->d_ext_lr, pairs, d_web_right, d_best_right, st));
    const int W = plan->width;
    const unsigned half_w = (unsigned)(W + 1) / 2, half_px = half_w * plan->height;
    hipLaunchKernelGGL(k_lr_unmirror, dim3((half_px + 255) / 256, pairs), dim3(256), 0, st, d_web_right, d_best_right,
                       W, (unsigned)W * plan->height, half_w, half_px);
    SM_LAUNCH_CHECK("k_lr_unmirror");
    return SM_OK;
}

extern "C" int sm_lr_check(sm_plan *plan, const int32_t *d_web, const int32_t *d_web_right, int max_diff,
                           int pairs, int32_t *d_web_out, int32_t *d_rejected, void *stream)
{
    const char *me = "sm_lr_check";
    if (!d_web || !d_web_right || !d_web_out) return sm_fail(SM_ERR_ARG, "%s: a map pointer is NULL", me);
    if (max_diff < 0) return sm_fail(SM_ERR_ARG, "%s: max_diff %d is negative", me, max_diff);
    SM_TRY(check_pairs(plan, pairs, me));
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
    return lr_check_launch(plan, false, d_web, d_web_right, d_web_out, nullptr, d_rejected, max_diff, pairs,
                           (hipStream_t)stream);
}

extern "C" int sm_run_lr(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, double threshold,
                         int pairs, int max_diff, int32_t *d_web, int32_t *d_best, int32_t *d_web_right,
                         int32_t *d_rejected, void *stream)
{
    const char *me = "sm_run_lr";
    if (!d_gray_left || !d_gray_right) return sm_fail(SM_ERR_ARG, "%s: input image pointer is NULL", me);
    if (!(threshold >= 0.0 && threshold <= 1.0)) return sm_fail(SM_ERR_ARG, "error: threshold must be between 0 and 1");
    if (!d_web) return sm_fail(SM_ERR_ARG, "%s: d_web is NULL", me);
    if (max_diff < 0) return sm_fail(SM_ERR_ARG, "%s: max_diff %d is negative", me, max_diff);
    SM_TRY(check_pairs(plan, pairs, me));
    const size_t map = (size_t)pairs * plan->width * plan->height * sizeof(i32);
    if ((d_best && overlap(d_best, d_web, map)) || (d_web_right && overlap(d_web_right, d_web, map)) ||
        (d_best && d_web_right && overlap(d_best, d_web_right, map)))
        return sm_fail(SM_ERR_ARG, "%s: result maps overlap", me);
    const size_t counts = (size_t)pairs * sizeof(i32);
    if (d_rejected && (overlap(d_rejected, d_web, counts, map) || (d_best && overlap(d_rejected, d_best, counts, map)) ||
                       (d_web_right && overlap(d_rejected, d_web_right, counts, map))))
        return sm_fail(SM_ERR_ARG, "%s: d_rejected overlaps a map", me);
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    if (sm_stream_capturing(st) && !(plan->tab_valid && memcmp(&plan->tab_threshold, &threshold, sizeof threshold) == 0))
        return sm_fail(SM_ERR_ARG, "%s: the decision tables of threshold %g are not prepared and the stream is capturing: "
                       "call sm_plan_prepare_threshold(plan, threshold, stream) before the capture begins", me, threshold);
    SM_TRY(need_lr(plan, st, me));
    SM_TRY(lr_fence_lanes(plan, st));
    lr_release_lanes(plan);
    // edges into the plan's packed images (as sm_run; they stay loaded), the left match, the mirrored images,
    // the right match into the mirrored-order map, and the check, which gathers from that map
    SM_TRY(sm_find_edges(plan, d_gray_left, d_gray_right, threshold, pairs, nullptr, nullptr, stream));
    SM_TRY(lr_match(plan, plan->d_ext, pairs, d_web, d_best, st));
    SM_TRY(lr_mirror(plan, pairs, st));
    SM_TRY(lr_match(plan, plan->d_ext_lr, pairs, plan->d_web_lr, nullptr, st));
    return lr_check_launch(plan, true, d_web, plan->d_web_lr, d_web, d_web_right, d_rejected, max_diff, pairs, st);
}

// ---------------------------------------------------------------------------
// the SAD / SSD cost mode's check
// ---------------------------------------------------------------------------

extern "C" int sm_plan_reserve_cost_lr(sm_plan *plan)
{
    if (!plan) return sm_fail(SM_ERR_ARG, "sm_plan_reserve_cost_lr: plan is NULL");
    SM_TRY(sm_use_device(plan->device));
    return reserve_cost_lr(plan, "sm_plan_reserve_cost_lr");
}

// what the cost entries check besides their maps (before any device call): cost, plan, pairs, the general kernel's reach
static int cost_lr_args(const sm_plan *plan, int cost, int pairs, const char *me)
{
    if (cost != SM_COST_SAD && cost != SM_COST_SSD)
        return sm_fail(SM_ERR_ARG, "%s: cost %d is neither SM_COST_SAD nor SM_COST_SSD", me, cost);
    SM_TRY(check_pairs(plan, pairs, me));
    const int n = 2 * (plan->square_width / 2) + 1;
    if (n > 25 || plan->num_shifts > 512)
        return sm_fail(SM_ERR_ARG, "%s: built for windows up to 25x25 and at most 512 shifts (got %dx%d, %d)", me, n, n,
                       plan->num_shifts);
    return SM_OK;
}

// the workspace, allocated here when sm_plan_reserve_cost_lr was not called -- unless the stream is capturing
static int need_cost_lr(sm_plan *plan, hipStream_t st, const char *me)
{
    if (plan->d_gray_lr) return SM_OK;
    if (sm_stream_capturing(st))
        return sm_fail(SM_ERR_ARG, "%s: the workspace of the cost mode's consistency check is not allocated and the stream "
                       "is capturing (an allocation cannot be captured): call sm_plan_reserve_cost_lr(plan) first", me);
    return reserve_cost_lr(plan, me);
}

// k_mirror_gray: mirror(right) into the workspace's first batch, mirror(left) into its second; returns the two
static int cost_lr_mirror(sm_plan *plan, const uint8_t *left, const uint8_t *right, int pairs, hipStream_t st,
                          const u8 **mleft, const u8 **mright)
{
    const int W = plan->width;
    const size_t batch = lr_gray_batch_bytes(plan);
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

extern "C" int sm_cost_wta_right(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int cost,
                                 int pairs, int32_t *d_web_right, int32_t *d_best_right, void *stream)
{
    const char *me = "sm_cost_wta_right";
    if (!d_gray_left || !d_gray_right) return sm_fail(SM_ERR_ARG, "%s: input image pointer is NULL", me);
    if (!d_web_right) return sm_fail(SM_ERR_ARG, "%s: d_web_right is NULL", me);
    SM_TRY(cost_lr_args(plan, cost, pairs, me));
    const size_t map = (size_t)pairs * plan->width * plan->height * sizeof(i32);
    if (d_best_right && overlap(d_web_right, d_best_right, map))
        return sm_fail(SM_ERR_ARG, "%s: d_web_right and d_best_right overlap", me);
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    SM_TRY(need_cost_lr(plan, st, me));
    const u8 *ml, *mr;
    SM_TRY(cost_lr_mirror(plan, d_gray_left, d_gray_right, pairs, st, &ml, &mr));
    // the plan's cost launch over the mirrored images writes the maps in mirrored order; they are turned round in place
    SM_TRY(sm_cost_wta(plan, ml, mr, cost, pairs, d_web_right, d_best_right, stream));
    const int W = plan->width;
    const unsigned half_w = (unsigned)(W + 1) / 2, half_px = half_w * plan->height;
    hipLaunchKernelGGL(k_lr_unmirror, dim3((half_px + 255) / 256, pairs), dim3(256), 0, st, d_web_right, d_best_right,
                       W, (unsigned)W * plan->height, half_w, half_px);
    SM_LAUNCH_CHECK("k_lr_unmirror");
    return SM_OK;
}

extern "C" int sm_cost_lr(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int cost, int pairs,
                          int max_diff, int32_t *d_web, int32_t *d_best, int32_t *d_web_right, int32_t *d_rejected,
                          void *stream)
{
    const char *me = "sm_cost_lr";
    if (!d_gray_left || !d_gray_right) return sm_fail(SM_ERR_ARG, "%s: input image pointer is NULL", me);
    if (!d_web) return sm_fail(SM_ERR_ARG, "%s: d_web is NULL", me);
    if (max_diff < 0) return sm_fail(SM_ERR_ARG, "%s: max_diff %d is negative", me, max_diff);
    SM_TRY(cost_lr_args(plan, cost, pairs, me));
    const size_t map = (size_t)pairs * plan->width * plan->height * sizeof(i32);
    if ((d_best && overlap(d_best, d_web, map)) || (d_web_right && overlap(d_web_right, d_web, map)) ||
        (d_best && d_web_right && overlap(d_best, d_web_right, map)))
        return sm_fail(SM_ERR_ARG, "%s: result maps overlap", me);
    const size_t counts = (size_t)pairs * sizeof(i32);
    if (d_rejected && (overlap(d_rejected, d_web, counts, map) || (d_best && overlap(d_rejected, d_best, counts, map)) ||
                       (d_web_right && overlap(d_rejected, d_web_right, counts, map))))
        return sm_fail(SM_ERR_ARG, "%s: d_rejected overlaps a map", me);
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    SM_TRY(need_cost_lr(plan, st, me));
    // the left cost launch (sm_cost_wta's maps exactly), the mirrored images, the right launch into the mirrored-order
    // map, and the check, which gathers from that map
    SM_TRY(sm_cost_wta(plan, d_gray_left, d_gray_right, cost, pairs, d_web, d_best, stream));
    const u8 *ml, *mr;
    SM_TRY(cost_lr_mirror(plan, d_gray_left, d_gray_right, pairs, st, &ml, &mr));
    SM_TRY(sm_cost_wta(plan, ml, mr, cost, pairs, plan->d_web_lr, nullptr, stream));
    return lr_check_launch(plan, true, d_web, plan->d_web_lr, d_web, d_web_right, d_rejected, max_diff, pairs, st);
}

// ---------------------------------------------------------------------------
// for the census mode (sm_census.hip)
// ---------------------------------------------------------------------------

int sm_lr_reserve_map(sm_plan *plan, const char *me)
{
    if (plan->d_web_lr) return SM_OK;
    void *map = nullptr;
    const hipError_t e = hipMalloc(&map, lr_map_bytes(plan));
    if (e != hipSuccess)
        return sm_fail(e == hipErrorOutOfMemory ? SM_ERR_NOMEM : SM_ERR_HIP, "%s: %zu bytes for the map of the "
                       "consistency check: %s", me, lr_map_bytes(plan), hipGetErrorString(e));
    plan->d_web_lr = (i32 *)map;
    return SM_OK;
}

int sm_lr_check_natural(const sm_plan *plan, const i32 *web, const i32 *right, i32 *out, i32 *rejected, int max_diff,
                        int pairs, hipStream_t st)
{
    return lr_check_launch(plan, false, web, right, out, nullptr, rejected, max_diff, pairs, st);
}

// ---------------------------------------------------------------------------
// post-filters (sm_filter.h): validity-aware median, speckle removal
// ---------------------------------------------------------------------------

static int filter_map_type(int map_type, const char *me, size_t *elem)
{
    if (map_type != SM_MAP_I32 && map_type != SM_MAP_I16)
        return sm_fail(SM_ERR_ARG, "%s: map_type %d is neither SM_MAP_I32 nor SM_MAP_I16", me, map_type);
    *elem = map_type == SM_MAP_I32 ? sizeof(i32) : sizeof(int16_t);
    return SM_OK;
}

extern "C" int sm_median_filter(sm_plan *plan, const void *d_in, int map_type, int k, int pairs, void *d_out, void *stream)
{
    const char *me = "sm_median_filter";
    size_t elem;
    if (!d_in || !d_out) return sm_fail(SM_ERR_ARG, "%s: a map pointer is NULL", me);
    SM_TRY(filter_map_type(map_type, me, &elem));
    if (k != 3 && k != 5) return sm_fail(SM_ERR_ARG, "%s: k %d is not 3 or 5", me, k);
    SM_TRY(check_pairs(plan, pairs, me));
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

// labels and component sizes, one int32 each per pixel of max_pairs maps (every word a call reads is written by
// k_spk_local first)
static int reserve_filter(sm_plan *plan, const char *me)
{
    if (plan->d_filter) return SM_OK;
    void *b = nullptr;
    const hipError_t e = hipMalloc(&b, 2 * lr_map_bytes(plan));
    if (e != hipSuccess)
        return sm_fail(e == hipErrorOutOfMemory ? SM_ERR_NOMEM : SM_ERR_HIP, "%s: %zu bytes for the labels and sizes of the "
                       "speckle filter: %s", me, 2 * lr_map_bytes(plan), hipGetErrorString(e));
    plan->d_filter = (i32 *)b;
    return SM_OK;
}

extern "C" int sm_plan_reserve_filter(sm_plan *plan)
{
    if (!plan) return sm_fail(SM_ERR_ARG, "sm_plan_reserve_filter: plan is NULL");
    SM_TRY(sm_use_device(plan->device));
    return reserve_filter(plan, "sm_plan_reserve_filter");
}

template <typename T>
static int speckle_launch(const sm_plan *plan, const T *in, T *out, int max_size, int max_diff, int pairs, i32 *removed,
                          hipStream_t st)
{
    const int W = plan->width, H = plan->height;
    const unsigned npx = (unsigned)W * H;
    i32 *labels = plan->d_filter, *sizes = plan->d_filter + (size_t)plan->max_pairs * npx;
    const unsigned tiles_x = (W + FLT_TW - 1) / FLT_TW, tiles_y = (H + FLT_TH - 1) / FLT_TH;
    if (removed) {
        hipLaunchKernelGGL(k_lr_zero_counts, dim3((pairs + 63) / 64), dim3(64), 0, st, removed, pairs);
        SM_LAUNCH_CHECK("k_lr_zero_counts");
    }
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
    SM_TRY(filter_map_type(map_type, me, &elem));
    if (max_size < 0) return sm_fail(SM_ERR_ARG, "%s: max_size %d is negative", me, max_size);
    if (max_diff < 0) return sm_fail(SM_ERR_ARG, "%s: max_diff %d is negative", me, max_diff);
    SM_TRY(check_pairs(plan, pairs, me));
    const size_t map = (size_t)pairs * plan->width * plan->height * elem;
    if (d_in != d_out && overlap(d_in, d_out, map))
        return sm_fail(SM_ERR_ARG, "%s: maps overlap without d_out being d_in", me);
    const size_t counts = (size_t)pairs * sizeof(i32);
    if (d_removed && (overlap(d_removed, d_in, counts, map) || overlap(d_removed, d_out, counts, map)))
        return sm_fail(SM_ERR_ARG, "%s: d_removed overlaps a map", me);
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    if (!plan->d_filter) {
        if (sm_stream_capturing(st))
            return sm_fail(SM_ERR_ARG, "%s: the workspace of the speckle filter is not allocated and the stream is capturing "
                           "(an allocation cannot be captured): call sm_plan_reserve_filter(plan) first", me);
        SM_TRY(reserve_filter(plan, me));
    }
    if (map_type == SM_MAP_I32)
        return speckle_launch<i32>(plan, (const i32 *)d_in, (i32 *)d_out, max_size, max_diff, pairs, d_removed, st);
    return speckle_launch<int16_t>(plan, (const int16_t *)d_in, (int16_t *)d_out, max_size, max_diff, pairs, d_removed, st);
}

// ---------------------------------------------------------------------------
// occlusion-aware interpolation (sm_interp.h): classification of the invalid pixels, discontinuity-preserving fill
// ---------------------------------------------------------------------------

extern "C" int sm_occlusion_classify(sm_plan *plan, const int32_t *d_web, const int32_t *d_web_right, int pairs,
                                     uint8_t *d_class, void *stream)
{
    const char *me = "sm_occlusion_classify";
    if (!d_web || !d_web_right || !d_class) return sm_fail(SM_ERR_ARG, "%s: a map pointer is NULL", me);
    SM_TRY(check_pairs(plan, pairs, me));
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

// (every element a call reads is written by a kernel of the same call first)
static int reserve_interp(sm_plan *plan, const char *me)
{
    if (plan->d_interp) return SM_OK;
    void *b = nullptr;
    const hipError_t e = hipMalloc(&b, itp_bytes(plan));
    if (e != hipSuccess)
        return sm_fail(e == hipErrorOutOfMemory ? SM_ERR_NOMEM : SM_ERR_HIP, "%s: %zu bytes for the directional maps and "
                       "carries of the interpolation: %s", me, itp_bytes(plan), hipGetErrorString(e));
    plan->d_interp = (i32 *)b;
    return SM_OK;
}

extern "C" int sm_plan_reserve_interp(sm_plan *plan)
{
    if (!plan) return sm_fail(SM_ERR_ARG, "sm_plan_reserve_interp: plan is NULL");
    SM_TRY(sm_use_device(plan->device));
    return reserve_interp(plan, "sm_plan_reserve_interp");
}

template <typename T>
static int interp_launch(const sm_plan *plan, const T *in, const u8 *cls, T *out, int pairs, i32 *filled, hipStream_t st)
{
    const int W = plan->width, H = plan->height, segs = itp_segs(plan), chunks = itp_chunks(plan);
    T *loc = (T *)plan->d_interp;
    i32 *car = plan->d_interp + plan->max_pairs * itp_loc_elems(plan);
    i32 *rows = car + plan->max_pairs * itp_car_elems(plan);
    const unsigned items = (unsigned)H * chunks, lines = W + H - 1;
    if (filled) {
        hipLaunchKernelGGL(k_lr_zero_counts, dim3((pairs + 63) / 64), dim3(64), 0, st, filled, pairs);
        SM_LAUNCH_CHECK("k_lr_zero_counts");
    }
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
    SM_TRY(filter_map_type(map_type, me, &elem));
    SM_TRY(check_pairs(plan, pairs, me));
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
    if (!plan->d_interp) {
        if (sm_stream_capturing(st))
            return sm_fail(SM_ERR_ARG, "%s: the workspace of the interpolation is not allocated and the stream is capturing "
                           "(an allocation cannot be captured): call sm_plan_reserve_interp(plan) first", me);
        SM_TRY(reserve_interp(plan, me));
    }
    if (map_type == SM_MAP_I32)
        return interp_launch<i32>(plan, (const i32 *)d_in, d_class, (i32 *)d_out, pairs, d_filled, st);
    return interp_launch<int16_t>(plan, (const int16_t *)d_in, d_class, (int16_t *)d_out, pairs, d_filled, st);
}

// ---------------------------------------------------------------------------
// rectification (sm_rectify.h): the remap, the map of a calibration, validity carried to the disparity maps
// ---------------------------------------------------------------------------

static int rect_format(int map_format, const char *me, size_t *entry)
{
    if (map_format != SM_RMAP_ABS32 && map_format != SM_RMAP_REL16)
        return sm_fail(SM_ERR_ARG, "%s: map_format %d is neither SM_RMAP_ABS32 nor SM_RMAP_REL16", me, map_format);
    *entry = map_format == SM_RMAP_ABS32 ? 2 * sizeof(i32) : 2 * sizeof(int16_t);
    return SM_OK;
}

// 32 * x + dx of a REL16 map is formed in 32 bits
static int rect_plan_size(const sm_plan *plan, const char *me)
{
    if (plan->width > (1 << 25) || plan->height > (1 << 25))
        return sm_fail(SM_ERR_ARG, "%s: built for images of up to %d pixels a side (got %dx%d)", me, 1 << 25, plan->width,
                       plan->height);
    return SM_OK;
}

extern "C" int sm_rectify(sm_plan *plan, const uint8_t *d_raw_left, const uint8_t *d_raw_right, int src_w, int src_h,
                          const void *d_map_left, const void *d_map_right, int map_format, int interp, int border,
                          int pairs, uint8_t *d_left, uint8_t *d_right, uint8_t *d_valid_left, uint8_t *d_valid_right,
                          void *stream)
{
    const char *me = "sm_rectify";
    size_t entry;
    if (!d_raw_left || !d_raw_right) return sm_fail(SM_ERR_ARG, "%s: input image pointer is NULL", me);
    if (!d_map_left || !d_map_right) return sm_fail(SM_ERR_ARG, "%s: a map pointer is NULL", me);
    if (!d_left || !d_right) return sm_fail(SM_ERR_ARG, "%s: output image pointer is NULL", me);
    SM_TRY(rect_format(map_format, me, &entry));
    if (interp != SM_INTERP_BILINEAR && interp != SM_INTERP_NEAREST)
        return sm_fail(SM_ERR_ARG, "%s: interp %d is neither SM_INTERP_BILINEAR nor SM_INTERP_NEAREST", me, interp);
    if (border < 0 || border > 255) return sm_fail(SM_ERR_ARG, "%s: border %d outside 0..255", me, border);
    if (src_w < 1 || src_h < 1 || (long long)src_w * src_h > INT32_MAX)
        return sm_fail(SM_ERR_ARG, "%s: source size %dx%d is not positive or has more than 2^31 - 1 pixels", me, src_w, src_h);
    // an output that IS an input or another output overlaps it whatever the sizes are (the ranges follow, with the plan)
    const void *outs[4] = {d_left, d_right, d_valid_left, d_valid_right};
    for (int i = 0; i < 4; i++) {
        if (!outs[i]) continue;
        if (outs[i] == d_raw_left || outs[i] == d_raw_right || outs[i] == d_map_left || outs[i] == d_map_right)
            return sm_fail(SM_ERR_ARG, "%s: an output overlaps an input (every tap is read from the raw images)", me);
        for (int j = 0; j < i; j++)
            if (outs[i] == outs[j]) return sm_fail(SM_ERR_ARG, "%s: outputs overlap", me);
    }
    SM_TRY(check_pairs(plan, pairs, me));
    SM_TRY(rect_plan_size(plan, me));
    if ((((uintptr_t)d_map_left | (uintptr_t)d_map_right) & (entry / 2 - 1)) != 0)
        return sm_fail(SM_ERR_ARG, "%s: a map pointer is not aligned to its %zu-byte elements", me, entry / 2);
    const int W = plan->width;
    const unsigned npx = (unsigned)W * plan->height;
    const size_t raw = (size_t)pairs * src_w * src_h, img = (size_t)pairs * npx, map = (size_t)npx * entry;
    for (int i = 0; i < 4; i++) {
        if (!outs[i]) continue;
        if (overlap(outs[i], d_raw_left, img, raw) || overlap(outs[i], d_raw_right, img, raw) ||
            overlap(outs[i], d_map_left, img, map) || overlap(outs[i], d_map_right, img, map))
            return sm_fail(SM_ERR_ARG, "%s: an output overlaps an input (every tap is read from the raw images)", me);
        for (int j = 0; j < i; j++)
            if (outs[j] && overlap(outs[i], outs[j], img)) return sm_fail(SM_ERR_ARG, "%s: outputs overlap", me);
    }
    SM_TRY(sm_use_device(plan->device));
    const RectSide l = {d_raw_left, d_map_left, d_left, d_valid_left}, r = {d_raw_right, d_map_right, d_right, d_valid_right};
    const bool vec = W % 4 == 0 && (((uintptr_t)d_map_left | (uintptr_t)d_map_right) & 15) == 0 &&
                     (((uintptr_t)d_left | (uintptr_t)d_right | (uintptr_t)d_valid_left | (uintptr_t)d_valid_right) & 3) == 0;
    const unsigned lanes = vec ? npx / 4 : npx;
    const dim3 grid((lanes + 255) / 256, 2), block(256);
#define SM_RECT_GO(REL, V) hipLaunchKernelGGL((k_rectify<REL, V>), grid, block, 0, (hipStream_t)stream, l, r, W, npx, src_w, \
                                              src_h, pairs, interp == SM_INTERP_NEAREST ? 1 : 0, (u32)border)
    if (map_format == SM_RMAP_REL16) { if (vec) SM_RECT_GO(true, 4); else SM_RECT_GO(true, 1); }
    else                             { if (vec) SM_RECT_GO(false, 4); else SM_RECT_GO(false, 1); }
#undef SM_RECT_GO
    SM_LAUNCH_CHECK("k_rectify");
    return SM_OK;
}

extern "C" int sm_rectify_map_build(sm_plan *plan, const sm_rectify_calib *calib, int map_format, void *d_map, void *stream)
{
    const char *me = "sm_rectify_map_build";
    size_t entry;
    if (!plan) return sm_fail(SM_ERR_ARG, "%s: plan is NULL", me);
    if (!calib) return sm_fail(SM_ERR_ARG, "%s: calib is NULL", me);
    if (!d_map) return sm_fail(SM_ERR_ARG, "%s: a map pointer is NULL", me);
    // every field is needed: a shorter struct is refused; of a longer (newer) one the fields this library knows are taken
    if (calib->struct_size < (int)sizeof(sm_rectify_calib))
        return sm_fail(SM_ERR_ARG, "%s: calib->struct_size %d is not that of a sm_rectify_calib (this library: %d bytes)", me,
                       calib->struct_size, (int)sizeof(sm_rectify_calib));
    SM_TRY(rect_format(map_format, me, &entry));
    SM_TRY(rect_plan_size(plan, me));
    if (((uintptr_t)d_map & (entry / 2 - 1)) != 0)
        return sm_fail(SM_ERR_ARG, "%s: the map pointer is not aligned to its %zu-byte elements", me, entry / 2);
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    if (sm_stream_capturing(st))
        return sm_fail(SM_ERR_ARG, "%s: the stream is capturing and the builder reads a flag back (it synchronises): build "
                       "the maps before the capture begins", me);
    RectCalib c;
    c.fx = calib->fx; c.fy = calib->fy; c.cx = calib->cx; c.cy = calib->cy;
    c.k1 = calib->k1; c.k2 = calib->k2; c.p1 = calib->p1; c.p2 = calib->p2; c.k3 = calib->k3;
    for (int i = 0; i < 9; i++) c.R[i] = calib->R[i / 3][i % 3];
    c.nfx = calib->new_fx; c.nfy = calib->new_fy; c.ncx = calib->new_cx; c.ncy = calib->new_cy;
    const int W = plan->width;
    const unsigned npx = (unsigned)W * plan->height;
    const dim3 grid((npx + 255) / 256), block(256);
    if (map_format == SM_RMAP_ABS32) {
        hipLaunchKernelGGL(k_rmap_build<false>, grid, block, 0, st, c, d_map, W, npx, (i32 *)nullptr);
        SM_LAUNCH_CHECK("k_rmap_build");
        return SM_OK;
    }
    // REL16: one flag, raised by every displacement that does not fit, read back
    i32 *flag = nullptr, over = 0;
    SM_HIP(hipMalloc((void **)&flag, sizeof(i32)));
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(i32), st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_rmap_build<true>, grid, block, 0, st, c, d_map, W, npx, flag);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&over, flag, sizeof(i32), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(flag);
    if (e != hipSuccess) return sm_fail(SM_ERR_HIP, "%s: building the map failed: %s", me, hipGetErrorString(e));
    if (over)
        return sm_fail(SM_ERR_ARG, "%s: a displacement of this calibration does not fit the int16 of SM_RMAP_REL16 (more than "
                       "1023 pixels, or a point at infinity): build the map with SM_RMAP_ABS32 (the contents of d_map are "
                       "not a map)", me);
    return SM_OK;
}

extern "C" int sm_valid_mask(sm_plan *plan, void *d_map, int map_type, const uint8_t *d_valid, int pairs, void *stream)
{
    const char *me = "sm_valid_mask";
    size_t elem;
    if (!d_map) return sm_fail(SM_ERR_ARG, "%s: a map pointer is NULL", me);
    if (!d_valid) return sm_fail(SM_ERR_ARG, "%s: d_valid is NULL", me);
    SM_TRY(filter_map_type(map_type, me, &elem));
    if ((const void *)d_valid == d_map) return sm_fail(SM_ERR_ARG, "%s: d_valid overlaps the map", me);
    SM_TRY(check_pairs(plan, pairs, me));
    const size_t n = (size_t)pairs * plan->width * plan->height;
    if (overlap(d_valid, d_map, n, n * elem)) return sm_fail(SM_ERR_ARG, "%s: d_valid overlaps the map", me);
    SM_TRY(sm_use_device(plan->device));
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (map_type == SM_MAP_I32) hipLaunchKernelGGL(k_valid_mask<i32>, grid, block, 0, (hipStream_t)stream, (i32 *)d_map, d_valid, n);
    else hipLaunchKernelGGL(k_valid_mask<int16_t>, grid, block, 0, (hipStream_t)stream, (int16_t *)d_map, d_valid, n);
    SM_LAUNCH_CHECK("k_valid_mask");
    return SM_OK;
}
