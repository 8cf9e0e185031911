// sm_internal.h -- shared between the translation units of libstereo_hip.so.
// Not part of the public boundary (that is include/stereo_hip.h).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdio.h>

#include "stereo_hip.h"
#include "sm_geom.h"

typedef uint32_t u32;
typedef uint8_t u8;
typedef int32_t i32;

// ---------------------------------------------------------------------------
// Packed edge image ("ext image"), the hot path's input format in HBM.
//
// One bit per pixel, 32 pixels per u32 word, bit b of word k of ext row e is
// the edge value at image coordinate
//        x = 32*k + b - pad_l,        y = e - half.
// The image is stored with its border already applied, so the hot kernel is
// border-mode agnostic for everything except the window's validity mask:
//   toroidal: ext(x, y) = E(x mod W, y mod H)       (idx(), src/util.h:42-47)
//   ghost:    ext(x, y) = E(x, y) inside the image, 0 outside
//                                              (src/stereo-ghost.c:286-287)
// Rows cover y in [-half, rows_needed) and x in [-pad_l, cols_needed) where
// the needed extents include the D-shift, the window halo and tile round-up.
// Workspace layout: [pair][side: 0 = left, 1 = right][ext_rows][ext_words].
// ---------------------------------------------------------------------------

struct sm_plan {
    int device;
    sm_plan_options opt;     // sm_plan_create_ex: explicit variant choices (all 0 = the plan's own)
    int width, height, num_shifts, square_width, border, max_pairs;
    int kernel;          // SM_KERNEL_*
    MatchGeom g;
    u32 *d_ext;          // packed edge images: the buffer in use (one of d_ext_buf)
    u32 *d_ext_buf[2];   // double buffer, so that sm_run can pipeline consecutive calls
    size_t ext_bytes;    // of one buffer
    int cur;             // index of d_ext in d_ext_buf
    int pipelined;       // sm_plan_set_pipelined: 0 off, 1 on, 2 on + inputs ordered behind `stream`
    hipStream_t lane[2];         // internal: pipelined sm_run i runs (edges, match) on lane i & 1, into buffer i & 1
    hipEvent_t ev_free[4];       // pipelined call number q has finished: ev_free[q & 3]
    hipEvent_t ev_inputs;        // the caller's stream up to this sm_run (pipelined == 2, or after a sequential phase)
    hipEvent_t ev_fork[2];       // pipelined sm_run INSIDE A STREAM CAPTURE: where lane b leaves the capturing stream
    unsigned long long cap_id;   // ... the capture these belong to (hipStreamGetCaptureInfo)
    int cap_live;                // ... the last pipelined sm_run was captured
    int ev_free_set[4];
    unsigned seq;                // number of the current / last pipelined sm_run
    int unfenced;                // match launches went out without a release event
    uintptr_t out_lo[2], out_hi[2];   // [web, best]: what the last pipelined call writes
    // optional timing of the match launches (sm_plan_time_kernels)
    int timing_cap, timing_n, timing_every, timing_seen;
    hipEvent_t *t_begin, *t_end;
    i32 *d_flags;        // [0] = zero-interval flag, [1] = has-zero scratch,
                         // [2] = edge table is not of threshold form
    i32 *h_flags;        // pinned host copy of d_flags (k_publish_flags)
    u32 *d_edge_tab;     // 766 x {lo | hi << 16}: edge iff sb <= lo || sb >= hi
    double tab_threshold;  // threshold d_edge_tab was built for
    int tab_valid;
    int tab_ok;          // tables verified to be of threshold form
    int pairs_loaded;    // batch size of the edges currently in d_ext
    // the lazily allocated workspaces (the table `sm_ws` below): NOT allocated with the plan, but by a
    // sm_plan_reserve_* or by the first call that needs them; part of the workspace from then on
    i32 *d_web_tmp;      // int32 map for narrow results of kernels without a narrow store path (sm_plan_reserve_narrow)
    u32 *d_ext_lr;       // sm_lr.hip: mirrored packed images, d_ext's layout: side 0 = mirror(right), side 1 = mirror(left)
    i32 *d_web_lr;       // right-reference map of sm_run_lr / sm_cost_lr in mirrored order: max_pairs * W * H
                         // (shared by the checks of every cost mode: allocated by whichever reserves first)
    u8 *d_gray_lr;       // sm_cost_lr: mirrored gray images, batch 0 = mirror(right), batch 1 = mirror(left),
                         // each of max_pairs * W * H bytes starting 256-byte aligned (sm_plan_reserve_cost_lr)
    u32 *d_census;       // sm_census.hip: descriptors [side: 0 = left, 1 = right][max_pairs][H][W], 8 bytes each (4 for c <= 5)
    void *d_sgm;         // sm_sgm.hip: one pair's volumes: A [H][W][Dp] u16, then S [H][W][Dp] i32 (Dp = 64, 128 or 256 >= num_shifts)
    i32 *d_filter;       // sm_filter.hip, speckle filter: labels [max_pairs][H][W] int32, then component sizes [max_pairs][H][W] int32
    i32 *d_interp;       // sm_interp.hip: per pair six directional maps [6][H][W], line carries [6][segments][W + H - 1], row
                         // carries [2][H][chunks], 4 bytes an element (layout at the top of sm_interp.hip)
    i32 *d_cloud;        // sm_reproject.hip, sm_point_cloud: kept pixels per tile of 1024 pixels, then their offsets: [max_pairs][tiles]
    void *d_sgm_near;    // sm_sgm_near.hip: one pair's banded volumes: A_b [H][W][16] u16, then S_b [H][W][16] i32 (slot innermost)
    double *d_wls;       // sm_wls.hip: three double planes, N, M and cp, each [max_pairs][H][W]
    uint16_t *d_cross;   // sm_cross.hip: packed arms [side: 0 = left, 1 = right][max_pairs][H][W], l | r << 4 | u << 8 | d << 12
    int cost_lds_raised; // sm_cost_wta: the LDS limit of this plan's four-wave SAD kernel is raised (on `device`)
    char describe[512];
};

// XCD-aware tile order (device side).  Workgroups are dealt round-robin to the 8
// XCDs by their linear id, so ids b and b+8 share an L2.  Mapping linear id ->
// tile so that every XCD owns ONE contiguous run of tiles (row-major: a band of
// image rows) lets the halo rows neighbouring tiles share, and the rows of the
// packed image themselves, be fetched into one L2 instead of eight.  Bijective for
// any tile count (MI355X guide, T1); placement is a speed matter only.
#ifdef __HIPCC__
// linear workgroup id -> position in an XCD-contiguous order over n items
__device__ __forceinline__ int sm_xcd_order(int lin, int n)
{
    const int xcd = lin & 7, j = lin >> 3;
    const int q = n >> 3, r = n & 7;                  // r XCDs get q + 1 items
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
}
__device__ __forceinline__ void sm_xcd_tile(int tiles_x, int tiles_y, int &tx, int &ty)
{
    const int t = sm_xcd_order(blockIdx.y * gridDim.x + blockIdx.x, tiles_x * tiles_y);
    ty = t / tiles_x;
    tx = t - ty * tiles_x;
}
#endif

// error plumbing (sm_fail: sm_api.hip)
int sm_fail(int code, const char *fmt, ...);
#define SM_HIP(call)                                                          \
    do {                                                                      \
        hipError_t e_ = (call);                                               \
        if (e_ != hipSuccess)                                                 \
            return sm_fail(e_ == hipErrorOutOfMemory ? SM_ERR_NOMEM : SM_ERR_HIP, \
                           "%s failed: %s (%s:%d)", #call,                    \
                           hipGetErrorString(e_), __FILE__, __LINE__);        \
    } while (0)
#define SM_TRY(expr) do { int rc_ = (expr); if (rc_) return rc_; } while (0)
#define SM_LAUNCH_CHECK(name)                                                 \
    do {                                                                      \
        hipError_t e_ = hipGetLastError();                                    \
        if (e_ != hipSuccess)                                                 \
            return sm_fail(SM_ERR_HIP, "launch of %s failed: %s", name,       \
                           hipGetErrorString(e_));                            \
    } while (0)

// sm_api.hip
int sm_use_device(int device);                    // hipSetDevice, failure as SM_ERR_HIP
bool sm_stream_capturing(hipStream_t st, unsigned long long *id = nullptr);   // is `st` recording into a graph (and which)?
// synchronise `st` and return the plan's flags (d_flags) as they were at that point; those in clear_mask are reset
int sm_read_flags(sm_plan *plan, hipStream_t st, int clear_mask, i32 out[4]);
// sm_plan_create: the code objects of a unit's kernels resolved at set-up, not by the first timed launch
void sm_edges_resolve_kernels(bool ghost);        // sm_edges.hip
void sm_run_resolve_kernels(void);                // sm_run.hip
void sm_step3_resolve_kernels(void);              // sm_step3.hip

// ---------------------------------------------------------------------------
// The lazily allocated workspaces: one table in sm_api.hip, one row per buffer (the sm_plan member, its bytes for
// this plan, whether it is zero-filled, its name in a message).  A stage names the SET of rows it needs; a new stage
// adds a member, a row and a set, and nothing else.  A row of 0 bytes is never allocated and never missing.
// ---------------------------------------------------------------------------
enum { SM_WS_NARROW, SM_WS_EXT_LR, SM_WS_WEB_LR, SM_WS_GRAY_LR, SM_WS_CENSUS, SM_WS_SGM, SM_WS_FILTER, SM_WS_INTERP,
       SM_WS_CLOUD, SM_WS_SGM_NEAR, SM_WS_WLS, SM_WS_CROSS, SM_WS_ROWS };
struct sm_ws_set {
    unsigned rows;             // bit r = row r
    const char *what;          // "the workspace of <what> is not allocated"
    const char *reserve;       // the public function a refusal inside a stream capture points to
    const sm_ws_set *first;    // a set reserved before this one, and kept where this one then fails
};
static const sm_ws_set SM_WS_SET_NARROW = {1u << SM_WS_NARROW, "narrow results (the int32 staging map)", "sm_plan_reserve_narrow", nullptr};
static const sm_ws_set SM_WS_SET_LR = {1u << SM_WS_EXT_LR | 1u << SM_WS_WEB_LR, "the consistency check", "sm_plan_reserve_lr", nullptr};
static const sm_ws_set SM_WS_SET_COST_LR = {1u << SM_WS_GRAY_LR | 1u << SM_WS_WEB_LR, "the cost mode's consistency check", "sm_plan_reserve_cost_lr", nullptr};
static const sm_ws_set SM_WS_SET_CENSUS = {1u << SM_WS_CENSUS | 1u << SM_WS_WEB_LR, "the census mode", "sm_plan_reserve_census", nullptr};
static const sm_ws_set SM_WS_SET_SGM = {1u << SM_WS_SGM, "SGM", "sm_plan_reserve_sgm", &SM_WS_SET_CENSUS};
static const sm_ws_set SM_WS_SET_FILTER = {1u << SM_WS_FILTER, "the speckle filter", "sm_plan_reserve_filter", nullptr};
static const sm_ws_set SM_WS_SET_INTERP = {1u << SM_WS_INTERP, "the interpolation", "sm_plan_reserve_interp", nullptr};
static const sm_ws_set SM_WS_SET_SGM_NEAR = {1u << SM_WS_SGM_NEAR, "banded SGM", "sm_plan_reserve_sgm_near", &SM_WS_SET_CENSUS};
static const sm_ws_set SM_WS_SET_CLOUD = {1u << SM_WS_CLOUD, "the point cloud", "sm_plan_reserve_cloud", nullptr};
static const sm_ws_set SM_WS_SET_WLS = {1u << SM_WS_WLS, "the edge-aware smoother", "sm_plan_reserve_wls", nullptr};
static const sm_ws_set SM_WS_SET_CROSS = {1u << SM_WS_CROSS, "the cross-based mode", "sm_plan_reserve_cross", &SM_WS_SET_CENSUS};
// all or nothing: on a failure every buffer this call allocated is freed and the plan is as before (but `first` stays)
int sm_ws_reserve(sm_plan *plan, const sm_ws_set &set, const char *me);
// from an entry point: nothing if present; SM_ERR_ARG naming set.reserve if `st` is capturing; otherwise reserve
int sm_ws_need(sm_plan *plan, const sm_ws_set &set, hipStream_t st, const char *me);
size_t sm_ws_bytes(const sm_plan *plan);          // of the rows that are allocated (sm_plan_workspace_bytes)
void sm_ws_free(sm_plan *plan);                   // all rows (sm_plan_destroy)
size_t sm_lr_map_bytes(const sm_plan *plan);      // one int32 map of max_pairs pairs
size_t sm_lr_gray_batch_bytes(const sm_plan *plan);   // one batch of mirrored gray images, rounded up to 256 bytes
size_t sm_itp_bytes(const sm_plan *plan);         // sm_interp.hip (its tile constants decide)
size_t sm_sgm_volume_bytes(const sm_plan *plan);  // sm_sgm.hip (its padded shift count decides)
size_t sm_cloud_bytes(const sm_plan *plan);       // sm_reproject.hip (its tile size decides)
size_t sm_sgm_near_volume_bytes(const sm_plan *plan);   // sm_sgm_near.hip (its slot count decides)

// ---------------------------------------------------------------------------
// Argument rules that more than one entry point applies (sm_api.hip; the two on the decision tables: sm_edges.hip).
// Each reports as `me`, the entry point's name.
// ---------------------------------------------------------------------------
// do [a, a + a_bytes) and [b, b + b_bytes) share a byte?  (b_bytes = 0: as many as a)
static inline bool overlap(const void *a, const void *b, size_t a_bytes, size_t b_bytes = 0)
{
    return (uintptr_t)a < (uintptr_t)b + (b_bytes ? b_bytes : a_bytes) && (uintptr_t)b < (uintptr_t)a + a_bytes;
}
int sm_check_pairs(const sm_plan *plan, int pairs, const char *me);       // plan is NULL; pairs outside 1..max_pairs
int sm_check_pairs_loaded(const sm_plan *plan, int pairs, const char *me);   // more pairs than the loaded edges are of
int sm_check_threshold(double threshold, const char *me);                 // outside 0..1 (the reference's message: no name in it)
int sm_check_web_type(const sm_plan *plan, int web_type, const char *me); // SM_WEB_I32 / U16 / U8, and the shifts fit it
bool sm_edge_tables_prepared(const sm_plan *plan, double threshold);      // the decision tables are those of `threshold`
int sm_check_tables_prepared(const sm_plan *plan, double threshold, const char *me);   // ... refused where they are not
                                                                          // and `me` is being captured (no set-up there)
int sm_check_reach(const sm_plan *plan, int max_shifts, const char *me);  // windows up to 25x25, at most max_shifts shifts
int sm_check_census_width(int census_width, const char *me);              // 3, 5 or 7
int sm_check_map_type(int map_type, const char *me, size_t *elem);        // SM_MAP_I32 / SM_MAP_I16 and its element size
// the result maps of a *_lr entry (d_best, d_web_right, d_sub, d_rejected may be NULL): "result maps overlap", then
// "d_rejected overlaps a map"
int sm_check_lr_maps(const sm_plan *plan, int pairs, const int32_t *d_web, const int32_t *d_best,
                     const int32_t *d_web_right, const int16_t *d_sub, const int32_t *d_rejected, const char *me);

// sm_edges.hip, for sm_plan_geometry: ext rows a wave of this plan's edge kernel walks down
int sm_edges_rows_per_wave(const sm_plan *plan);

// sm_run.hip.  The lanes of pipelined calls, for a call of another unit that reads or rewrites the packed images on
// `st`: `st` waits for every pipelined call before it (nothing inside a capture, where they have joined `st`), and
// the next pipelined call waits for `st` as after any sequential launch
int sm_lanes_fence(sm_plan *plan, hipStream_t st);
void sm_lanes_release(sm_plan *plan);
void sm_timing_free(sm_plan *plan);               // the timing events (sm_plan_time_kernels(plan, 0), sm_plan_destroy)

// sm_lr.hip, for the other stages: the per-pair counts zeroed by k_lr_zero_counts (a kernel: a captured memset of them
// replayed wrongly); k_lr_check on a right-reference map in natural or mirrored order (the rejection counts zeroed
// first; mirrored: right_out, if not NULL, gets the map in natural order); k_lr_unmirror, which turns the maps of a
// mirrored-order right-reference pass round in place
int sm_lr_zero_counts(i32 *counts, int pairs, hipStream_t st);
int sm_lr_check_launch(const sm_plan *plan, bool mirrored, const i32 *web, const i32 *right, i32 *out, i32 *right_out,
                       i32 *rejected, int max_diff, int pairs, hipStream_t st);
int sm_lr_unmirror(const sm_plan *plan, int pairs, i32 *d_web_right, i32 *d_best_right, hipStream_t st);
// sm_census.hip, for SGM: both images of `pairs` pairs into the census workspace (4-byte descriptors for c <= 5, 8 for 7)
int sm_census_descriptors(sm_plan *plan, int cw, const uint8_t *left, const uint8_t *right, int pairs, hipStream_t st);
// sm_sgm.hip, for sm_sgm_wta2 (sm_unique.hip): the checks every SGM entry makes besides its pointers, and the left pass
// whose last direction (k_sgm_path_second) writes the runner-up maps beside web / best / sub (best, sub, best2: NULL ok)
int sm_sgm_args(const sm_plan *plan, int census_width, int p1, int p2, int paths, int pairs, const char *me);
// ... those of them that need no plan (census width, paths, penalties), for banded SGM, whose shift limit is the census mode's
int sm_sgm_scalar_args(int census_width, int p1, int p2, int paths, const char *me);
int sm_sgm_second_pass(const sm_plan *plan, int cw, int p1, int p2, int paths, int pairs, i32 *web, i32 *best,
                       int16_t *sub, i32 *web2, i32 *best2, hipStream_t st);
// sm_sgm.hip, for the single-volume check (sm_sgm_both.hip): the data term and all directions of ONE pair with the last
// direction launched as k_sgm_path<K, SGM_MID>: afterwards *S, [H][W][*Dp] int32 in the plan's SGM workspace, holds the
// full aggregate (entries d >= num_shifts are not costs: wrapped sums of the path kernel's padding value)
int sm_sgm_volume_pass(const sm_plan *plan, int cw, int p1, int p2, int paths, int pair, const i32 **S, int *Dp,
                       hipStream_t st);
// SGM's directions in stream order, for sm_sgm.hip and sm_sgm_near.hip (integer sums: the order changes nothing):
// direction r of `paths` (8: all of them; 4: the two axes, both ways) and the lines it has in a w x h image
static inline void sm_sgm_direction(int paths, int r, int w, int h, int *dx, int *dy, int *lines)
{
    static const int dirs[8][2] = {{1, 0}, {0, 1}, {1, 1}, {-1, 1}, {1, -1}, {-1, -1}, {0, -1}, {-1, 0}};
    static const int four[4] = {0, 1, 6, 7};
    const int *dir = dirs[paths == 4 ? four[r] : r];
    *dx = dir[0]; *dy = dir[1];
    *lines = *dy == 0 ? h : *dx == 0 ? w : w + h - 1;
}
// sm_filter.hip, for sm_sgm_lr: k_sgm_sub_mask, sub = 0 where web = 0, over n elements
int sm_sub_mask_launch(const i32 *web, int16_t *sub, long long n, hipStream_t st);

// the instantiation K<NW, GHOST, MIRROR> of a cost mode's pass kernel for a plan's border and a pass's direction
#define SM_PASS_KERNEL(K, NW, ghost, mirror)                                                                  \
    ((ghost) ? ((mirror) ? (const void *)K<NW, true, true> : (const void *)K<NW, true, false>)                \
             : ((mirror) ? (const void *)K<NW, false, true> : (const void *)K<NW, false, false>))

// sm_match_bs.hip (bit-sliced kernel; nullptr if not built for this window: sm_bs_built of sm_plan_model.h says which are)
const void *sm_bs_kernel_ptr(int n, int ds, bool fulld, bool ghost, bool cap2, bool duo = false);
// what ONE launch adds to the plan's geometry: passed by value, the plan is not modified
struct MatchLaunch {
    MatchGeom g;                        // plan->g with vec_ok / web_bytes of this launch
    hipEvent_t ev_begin, ev_end;        // non-null: attach these events to the dispatch itself
};
// sm_run.hip: plan->g for maps of web_bytes an element (vec_ok cleared unless both are aligned for int4 stores), no events
MatchLaunch sm_match_launch_args(const sm_plan *plan, const void *d_web, const void *d_best, int web_bytes);
int sm_bs_launch(const sm_plan *plan, const MatchLaunch &l, int pairs, i32 *d_web, i32 *d_best, hipStream_t st);
int sm_bs_prepare(sm_plan *plan);        // set-up launch: code object loaded before the first real one

// sm_match.hip
int sm_match_configure(sm_plan *plan);   // fills plan->kernel / plan->g
int sm_match_launch(const sm_plan *plan, const MatchLaunch &l, int pairs, i32 *d_web, i32 *d_best, hipStream_t st);
