// sm_api.hip -- the plan and what every stage shares (include/stereo_hip.h): error text, the device, memory,
// stream and event wrappers, plan creation / destruction / geometry, the table of lazily allocated workspaces,
// the argument rules of more than one entry point, the plan's flags read back, and the capture query.  The stages
// are units of their own: sm_edges.hip (step 1), sm_run.hip and sm_match.hip (step 2), sm_step3.hip, and the later ones.

#include "sm_internal.h"

#include <stdarg.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------

static thread_local char g_err[512] = "";

int sm_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

extern "C" const char *sm_last_error(void) { return g_err; }

// hand the plan's flags to the host: one lane copies them into pinned host memory the
// host reads after synchronising the stream (no 4-byte hipMemcpy to pageable memory,
// which costs tens of microseconds), and clears the ones in `clear_mask`
__global__ void k_publish_flags(i32 *__restrict__ d_flags, i32 *__restrict__ h_flags, int clear_mask)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        for (int i = 0; i < 4; i++) {
            h_flags[i] = d_flags[i];
            if ((clear_mask >> i) & 1) d_flags[i] = 0;
        }
    }
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------

int sm_use_device(int device)
{
    SM_HIP(hipSetDevice(device));
    return SM_OK;
}

extern "C" int sm_device_count(int *count)
{
    if (!count) return sm_fail(SM_ERR_ARG, "sm_device_count: count is NULL");
    SM_HIP(hipGetDeviceCount(count));
    return SM_OK;
}

extern "C" int sm_malloc(int device, size_t bytes, void **d_ptr)
{
    if (!d_ptr) return sm_fail(SM_ERR_ARG, "sm_malloc: d_ptr is NULL");
    SM_TRY(sm_use_device(device));
    *d_ptr = nullptr;
    SM_HIP(hipMalloc(d_ptr, bytes ? bytes : 1));
    SM_HIP(hipMemset(*d_ptr, 0, bytes ? bytes : 1));
    return SM_OK;
}

extern "C" int sm_free(int device, void *d_ptr)
{
    SM_TRY(sm_use_device(device));
    SM_HIP(hipFree(d_ptr));
    return SM_OK;
}

extern "C" int sm_memcpy_h2d(int device, void *d_dst, const void *h_src, size_t bytes)
{
    SM_TRY(sm_use_device(device));
    SM_HIP(hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice));
    return SM_OK;
}

extern "C" int sm_memcpy_d2h(int device, void *h_dst, const void *d_src, size_t bytes)
{
    SM_TRY(sm_use_device(device));
    SM_HIP(hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost));
    return SM_OK;
}

extern "C" int sm_stream_sync(int device, void *stream)
{
    SM_TRY(sm_use_device(device));
    SM_HIP(hipStreamSynchronize((hipStream_t)stream));
    return SM_OK;
}

extern "C" int sm_host_alloc(size_t bytes, void **h_ptr)
{
    if (!h_ptr) return sm_fail(SM_ERR_ARG, "sm_host_alloc: h_ptr is NULL");
    *h_ptr = nullptr;
    SM_HIP(hipHostMalloc(h_ptr, bytes ? bytes : 1, hipHostMallocDefault));
    return SM_OK;
}

extern "C" int sm_host_free(void *h_ptr)
{
    SM_HIP(hipHostFree(h_ptr));
    return SM_OK;
}

extern "C" int sm_memcpy_h2d_async(int device, void *d_dst, const void *h_src, size_t bytes, void *stream)
{
    SM_TRY(sm_use_device(device));
    SM_HIP(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return SM_OK;
}

extern "C" int sm_memcpy_d2h_async(int device, void *h_dst, const void *d_src, size_t bytes, void *stream)
{
    SM_TRY(sm_use_device(device));
    SM_HIP(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return SM_OK;
}

extern "C" int sm_stream_create(int device, void **stream)
{
    if (!stream) return sm_fail(SM_ERR_ARG, "sm_stream_create: stream is NULL");
    SM_TRY(sm_use_device(device));
    hipStream_t st = nullptr;
    SM_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    *stream = (void *)st;
    return SM_OK;
}

extern "C" int sm_stream_destroy(int device, void *stream)
{
    SM_TRY(sm_use_device(device));
    SM_HIP(hipStreamDestroy((hipStream_t)stream));
    return SM_OK;
}

extern "C" int sm_event_create(int device, void **event)
{
    if (!event) return sm_fail(SM_ERR_ARG, "sm_event_create: event is NULL");
    SM_TRY(sm_use_device(device));
    hipEvent_t ev = nullptr;
    SM_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    *event = (void *)ev;
    return SM_OK;
}

extern "C" int sm_event_destroy(int device, void *event)
{
    SM_TRY(sm_use_device(device));
    SM_HIP(hipEventDestroy((hipEvent_t)event));
    return SM_OK;
}

extern "C" int sm_event_record(int device, void *event, void *stream)
{
    if (!event) return sm_fail(SM_ERR_ARG, "sm_event_record: event is NULL");
    SM_TRY(sm_use_device(device));
    SM_HIP(hipEventRecord((hipEvent_t)event, (hipStream_t)stream));
    return SM_OK;
}

extern "C" int sm_stream_wait_event(int device, void *stream, void *event)
{
    if (!event) return sm_fail(SM_ERR_ARG, "sm_stream_wait_event: event is NULL");
    SM_TRY(sm_use_device(device));
    SM_HIP(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)event, 0));
    return SM_OK;
}

extern "C" int sm_event_sync(int device, void *event)
{
    if (!event) return sm_fail(SM_ERR_ARG, "sm_event_sync: event is NULL");
    SM_TRY(sm_use_device(device));
    SM_HIP(hipEventSynchronize((hipEvent_t)event));
    return SM_OK;
}

extern "C" int sm_plan_create(int device, int width, int height, int num_shifts,
                              int square_width, int border, int max_pairs, sm_plan **out)
{
    return sm_plan_create_ex(device, width, height, num_shifts, square_width, border, max_pairs, nullptr, out);
}

extern "C" int sm_plan_create_ex(int device, int width, int height, int num_shifts, int square_width,
                                 int border, int max_pairs, const sm_plan_options *options, sm_plan **out)
{
    if (!out) return sm_fail(SM_ERR_ARG, "sm_plan_create: out is NULL");
    // struct_size: 0 = "nothing but the size field" (an all-zero struct is the plan's own choice throughout);
    // a LARGER struct comes from a caller built against a newer header: the prefix this library knows is taken
    if (options && (options->struct_size < 0 || (options->struct_size > 0 && options->struct_size < (int)sizeof(int))))
        return sm_fail(SM_ERR_ARG, "sm_plan_create_ex: options->struct_size %d is not that of a sm_plan_options "
                       "(this library: %d bytes)", options->struct_size, (int)sizeof(sm_plan_options));
    *out = nullptr;
    if (width < 1 || height < 1)
        return sm_fail(SM_ERR_ARG, "sm_plan_create: image size %dx%d is not positive", width, height);
    if ((long long)width * height > (1ll << 30))
        return sm_fail(SM_ERR_ARG, "sm_plan_create: image of %dx%d pixels is too large", width, height);
    if (num_shifts < 1 || num_shifts > 65535)
        return sm_fail(SM_ERR_ARG, "sm_plan_create: num_shifts %d outside 1..65535", num_shifts);
    if (square_width < 0)
        return sm_fail(SM_ERR_ARG, "sm_plan_create: square_width %d is negative "
                       "(undefined in the reference)", square_width);
    if (square_width > width || square_width > height)
        return sm_fail(SM_ERR_ARG, "error: square width must not be higher than image width/height");
    if (border != SM_TOROIDAL && border != SM_GHOST)
        return sm_fail(SM_ERR_ARG, "sm_plan_create: border %d is neither SM_TOROIDAL nor SM_GHOST", border);
    if (max_pairs < 1)
        return sm_fail(SM_ERR_ARG, "sm_plan_create: max_pairs %d < 1", max_pairs);
    SM_TRY(sm_use_device(device));

    sm_plan *p = (sm_plan *)calloc(1, sizeof *p);
    if (p) p->timing_every = 1;
    if (!p) return sm_fail(SM_ERR_NOMEM, "error: out of memory");
    p->device = device;
    p->width = width; p->height = height;
    p->num_shifts = num_shifts; p->square_width = square_width;
    p->border = border; p->max_pairs = max_pairs;
    if (options && options->struct_size > 0)      // a shorter (older) struct: the rest stays 0; a longer one: the known prefix
        memcpy(&p->opt, options, std::min((size_t)options->struct_size, sizeof(sm_plan_options)));
    p->opt.struct_size = (int)sizeof(sm_plan_options);
    int rc = sm_match_configure(p);
    if (rc) { free(p); return rc; }
    p->g.web_bytes = 4;

    p->ext_bytes = (size_t)max_pairs * 2 * (size_t)p->g.ext_image_words * sizeof(u32);
    hipError_t e = hipMalloc((void **)&p->d_ext_buf[0], p->ext_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&p->d_ext_buf[1], p->ext_bytes);
    if (e == hipSuccess) e = hipMemset(p->d_ext_buf[1], 0, p->ext_bytes);
    for (int b = 0; b < 2 && e == hipSuccess; b++) e = hipStreamCreateWithFlags(&p->lane[b], hipStreamNonBlocking);
    for (int q = 0; q < 4 && e == hipSuccess; q++) e = hipEventCreateWithFlags(&p->ev_free[q], hipEventDisableTiming);
    p->d_ext = p->d_ext_buf[0];
    if (e == hipSuccess) e = hipEventCreateWithFlags(&p->ev_inputs, hipEventDisableTiming);
    for (int b = 0; b < 2 && e == hipSuccess; b++) e = hipEventCreateWithFlags(&p->ev_fork[b], hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc((void **)&p->d_flags, 4 * sizeof(i32));
    if (e == hipSuccess) e = hipMalloc((void **)&p->d_edge_tab, 768 * sizeof(u32));
    if (e == hipSuccess) e = hipHostMalloc((void **)&p->h_flags, 4 * sizeof(i32), hipHostMallocDefault);
    if (e == hipSuccess) e = hipMemset(p->d_ext, 0, p->ext_bytes);
    if (e == hipSuccess) e = hipMemset(p->d_flags, 0, 4 * sizeof(i32));
    // (kernels without a narrow store path write narrow maps through an int32 staging map,
    // max_pairs * W * H * 4 bytes: NOT allocated here -- a plan whose caller only ever asks for
    // int32 maps must not pay for it -- but by sm_plan_reserve_narrow, or by the first narrow request)
    if (e != hipSuccess) {
        for (int b = 0; b < 2; b++) {
            if (p->d_ext_buf[b]) (void)hipFree(p->d_ext_buf[b]);
            if (p->lane[b]) (void)hipStreamDestroy(p->lane[b]);
        }
        for (int q = 0; q < 4; q++)
            if (p->ev_free[q]) (void)hipEventDestroy(p->ev_free[q]);
        if (p->ev_inputs) (void)hipEventDestroy(p->ev_inputs);
        for (int b = 0; b < 2; b++)
            if (p->ev_fork[b]) (void)hipEventDestroy(p->ev_fork[b]);
        if (p->d_flags) (void)hipFree(p->d_flags);
        if (p->d_edge_tab) (void)hipFree(p->d_edge_tab);
        if (p->h_flags) (void)hipHostFree(p->h_flags);
        free(p);
        return sm_fail(e == hipErrorOutOfMemory ? SM_ERR_NOMEM : SM_ERR_HIP,
                       "sm_plan_create: workspace allocation failed: %s", hipGetErrorString(e));
    }
    // Resolve the code objects of the kernels this plan will launch now (setup),
    // so that the first timed launch does not pay the runtime's lazy loading.
    {
        hipFuncAttributes fa;
        (void)hipFuncGetAttributes(&fa, (const void *)k_publish_flags);
        sm_edges_resolve_kernels(border == SM_GHOST);
        sm_run_resolve_kernels();
        sm_step3_resolve_kernels();
    }
    if (p->kernel == SM_KERNEL_BS) {
        rc = sm_bs_prepare(p);
        if (rc) { sm_plan_destroy(p); return rc; }
    }
    *out = p;
    return SM_OK;
}

// ---------------------------------------------------------------------------
// the lazily allocated workspaces (sm_internal.h): the table, and the four functions on it
// ---------------------------------------------------------------------------

size_t sm_lr_map_bytes(const sm_plan *plan) { return (size_t)plan->max_pairs * plan->width * plan->height * sizeof(i32); }
size_t sm_lr_gray_batch_bytes(const sm_plan *plan)
{
    return ((size_t)plan->max_pairs * plan->width * plan->height + 255) & ~(size_t)255;
}
// (the bit-sliced kernel stores narrow maps itself: its plans never need the staging map)
static size_t ws_narrow_bytes(const sm_plan *plan) { return plan->kernel == SM_KERNEL_BS ? 0 : sm_lr_map_bytes(plan); }
static size_t ws_ext_bytes(const sm_plan *plan) { return plan->ext_bytes; }
static size_t ws_gray_bytes(const sm_plan *plan) { return 2 * sm_lr_gray_batch_bytes(plan); }
static size_t ws_census_bytes(const sm_plan *plan)      // both images of max_pairs pairs, 8 bytes a descriptor
{
    return (size_t)2 * plan->max_pairs * plan->width * plan->height * sizeof(uint64_t);
}
static size_t ws_filter_bytes(const sm_plan *plan) { return 2 * sm_lr_map_bytes(plan); }
static size_t ws_wls_bytes(const sm_plan *plan)         // N, M and cp: a double each per pixel of max_pairs maps
{
    return (size_t)3 * plan->max_pairs * plan->width * plan->height * sizeof(double);
}
static size_t ws_cross_bytes(const sm_plan *plan)       // the packed arms of both images of max_pairs pairs
{
    return (size_t)2 * plan->max_pairs * plan->width * plan->height * sizeof(uint16_t);
}

static const struct {
    size_t member;                          // offsetof(sm_plan, the pointer)
    size_t (*bytes)(const sm_plan *);
    bool zero;                              // filled with zeros when allocated
    const char *what;
} ws_rows[SM_WS_ROWS] = {
    /* SM_WS_NARROW  */ {offsetof(sm_plan, d_web_tmp), ws_narrow_bytes, false, "int32 staging map of narrow results"},
    // (zero-filled: the words beyond each side's row extent stay zero, as in the plan's own images)
    /* SM_WS_EXT_LR  */ {offsetof(sm_plan, d_ext_lr), ws_ext_bytes, true, "mirrored images of the consistency check"},
    /* SM_WS_WEB_LR  */ {offsetof(sm_plan, d_web_lr), sm_lr_map_bytes, false, "map of the consistency check"},
    /* SM_WS_GRAY_LR */ {offsetof(sm_plan, d_gray_lr), ws_gray_bytes, false, "mirrored gray images of the consistency check"},
    /* SM_WS_CENSUS  */ {offsetof(sm_plan, d_census), ws_census_bytes, false, "census descriptors"},
    /* SM_WS_SGM     */ {offsetof(sm_plan, d_sgm), sm_sgm_volume_bytes, false, "SGM volumes"},
    /* SM_WS_FILTER  */ {offsetof(sm_plan, d_filter), ws_filter_bytes, false, "labels and sizes of the speckle filter"},
    /* SM_WS_INTERP  */ {offsetof(sm_plan, d_interp), sm_itp_bytes, false, "directional maps and carries of the interpolation"},
    /* SM_WS_CLOUD   */ {offsetof(sm_plan, d_cloud), sm_cloud_bytes, false, "tile counts of the point cloud"},
    /* SM_WS_SGM_NEAR */ {offsetof(sm_plan, d_sgm_near), sm_sgm_near_volume_bytes, false, "banded SGM volumes"},
    /* SM_WS_WLS     */ {offsetof(sm_plan, d_wls), ws_wls_bytes, false, "planes of the edge-aware smoother"},
    /* SM_WS_CROSS   */ {offsetof(sm_plan, d_cross), ws_cross_bytes, false, "arms of the cross-based mode"},
};

static void *&ws_ptr(const sm_plan *plan, int r) { return *(void **)((char *)plan + ws_rows[r].member); }

// the rows of `set` (and of the sets before it) that this plan needs and does not have
static unsigned ws_missing(const sm_plan *plan, const sm_ws_set &set)
{
    unsigned m = set.first ? ws_missing(plan, *set.first) : 0;
    for (int r = 0; r < SM_WS_ROWS; r++)
        if ((set.rows >> r & 1) && !ws_ptr(plan, r) && ws_rows[r].bytes(plan)) m |= 1u << r;
    return m;
}

int sm_ws_reserve(sm_plan *plan, const sm_ws_set &set, const char *me)
{
    if (set.first) SM_TRY(sm_ws_reserve(plan, *set.first, me));
    const unsigned todo = ws_missing(plan, set);
    for (int r = 0; r < SM_WS_ROWS; r++) {
        if (!(todo >> r & 1)) continue;
        const size_t bytes = ws_rows[r].bytes(plan);
        hipError_t e = hipMalloc(&ws_ptr(plan, r), bytes);
        if (e != hipSuccess) ws_ptr(plan, r) = nullptr;
        else if (ws_rows[r].zero) e = hipMemset(ws_ptr(plan, r), 0, bytes);
        if (e == hipSuccess) continue;
        for (int q = 0; q <= r; q++)
            if ((todo >> q & 1) && ws_ptr(plan, q)) {
                (void)hipFree(ws_ptr(plan, q));
                ws_ptr(plan, q) = nullptr;
            }
        return sm_fail(e == hipErrorOutOfMemory ? SM_ERR_NOMEM : SM_ERR_HIP, "%s: %zu bytes for the %s: %s", me, bytes,
                       ws_rows[r].what, hipGetErrorString(e));
    }
    return SM_OK;
}

int sm_ws_need(sm_plan *plan, const sm_ws_set &set, hipStream_t st, const char *me)
{
    if (!ws_missing(plan, set)) return SM_OK;
    if (sm_stream_capturing(st))
        return sm_fail(SM_ERR_ARG, "%s: the workspace of %s is not allocated and the stream is capturing (an allocation "
                       "cannot be captured): call %s(plan) first", me, set.what, set.reserve);
    return sm_ws_reserve(plan, set, me);
}

size_t sm_ws_bytes(const sm_plan *plan)
{
    size_t sum = 0;
    for (int r = 0; r < SM_WS_ROWS; r++)
        if (ws_ptr(plan, r)) sum += ws_rows[r].bytes(plan);
    return sum;
}

void sm_ws_free(sm_plan *plan)
{
    for (int r = 0; r < SM_WS_ROWS; r++) {
        if (ws_ptr(plan, r)) (void)hipFree(ws_ptr(plan, r));
        ws_ptr(plan, r) = nullptr;
    }
}

// test only (stereo_hip.h): every allocated row that is NOT zero-filled on allocation, filled with `word` over its whole
// extent.  A zero == true row is left alone: its zero words are an invariant no call restores (SM_WS_EXT_LR: the
// words beyond each side's row extent), so poisoning it would break the plan rather than test a stage.
extern "C" int sm_debug_poison_workspace(sm_plan *plan, uint32_t word)
{
    const char *me = "sm_debug_poison_workspace";
    if (!plan) return sm_fail(SM_ERR_ARG, "%s: plan is NULL", me);
    SM_TRY(sm_use_device(plan->device));
    hipError_t e = hipDeviceSynchronize();              // both lanes, and every stream a stage was given
    for (int r = 0; r < SM_WS_ROWS && e == hipSuccess; r++) {
        if (ws_rows[r].zero || !ws_ptr(plan, r)) continue;
        e = hipMemsetD32((hipDeviceptr_t)ws_ptr(plan, r), (int)word, ws_rows[r].bytes(plan) / sizeof(u32));
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return sm_fail(SM_ERR_HIP, "%s: %s", me, hipGetErrorString(e));
    return SM_OK;
}

extern "C" int sm_plan_reserve_narrow(sm_plan *plan)
{
    if (!plan) return sm_fail(SM_ERR_ARG, "sm_plan_reserve_narrow: plan is NULL");
    SM_TRY(sm_use_device(plan->device));
    return sm_ws_reserve(plan, SM_WS_SET_NARROW, "sm_plan_reserve_narrow");
}

extern "C" void sm_plan_destroy(sm_plan *plan)
{
    if (!plan) return;
    (void)hipSetDevice(plan->device);
    for (int b = 0; b < 2; b++) (void)hipStreamSynchronize(plan->lane[b]);
    sm_timing_free(plan);
    for (int b = 0; b < 2; b++) {
        (void)hipFree(plan->d_ext_buf[b]);
        (void)hipStreamDestroy(plan->lane[b]);
    }
    for (int q = 0; q < 4; q++) (void)hipEventDestroy(plan->ev_free[q]);
    (void)hipEventDestroy(plan->ev_inputs);
    for (int b = 0; b < 2; b++) (void)hipEventDestroy(plan->ev_fork[b]);
    sm_ws_free(plan);
    (void)hipFree(plan->d_flags);
    (void)hipFree(plan->d_edge_tab);
    (void)hipHostFree(plan->h_flags);
    free(plan);
}

extern "C" const char *sm_plan_describe(const sm_plan *plan) { return plan ? plan->describe : ""; }

extern "C" int sm_plan_geometry_sized(const sm_plan *plan, sm_geometry *out_any, size_t size)
{
    if (!plan || !out_any) return sm_fail(SM_ERR_ARG, "sm_plan_geometry: NULL argument");
    if (size < sizeof(int)) return sm_fail(SM_ERR_ARG, "sm_plan_geometry_sized: size %zu is not that of a sm_geometry", size);
    sm_geometry full, *out = &full;
    memset(&full, 0, sizeof full);
    const MatchGeom &g = plan->g;
    out->kernel = plan->kernel;
    out->window = g.n;
    out->shifts_per_lane = g.ds;
    out->shift_lanes = g.nl;
    out->threads = g.threads;
    out->tile_w = g.tw;
    out->tile_h = g.duo ? 2 * g.tile_h : g.tile_h;
    out->tiles_x = g.tiles_x;
    out->tiles_y = g.tiles_y;
    out->ext_words = g.ext_words;
    out->ext_rows = g.ext_rows;
    out->pad_l = g.pad_l;
    out->lds_bytes = g.lds_bytes;
    out->two_wave_variant = g.cap2;
    out->edge_rows_per_wave = sm_edges_rows_per_wave(plan);
    out->waves_per_workgroup = plan->kernel == SM_KERNEL_BS ? (g.duo ? 2 : 1) : (g.threads + 63) / 64;
    out->lane_merge_lds = plan->kernel == SM_KERNEL_BS && g.xmerge;
    // the caller's struct may be older (shorter: it gets the fields it knows) or newer (longer: the rest is zeroed)
    memset(out_any, 0, size);
    memcpy(out_any, &full, size < sizeof full ? size : sizeof full);
    return SM_OK;
}

extern "C" int sm_plan_geometry(const sm_plan *plan, sm_geometry *out)
{
    return sm_plan_geometry_sized(plan, out, sizeof(sm_geometry));
}

extern "C" size_t sm_plan_workspace_bytes(const sm_plan *plan)
{
    if (!plan) return 0;
    return 2 * plan->ext_bytes + 4 * sizeof(i32) + 768 * sizeof(u32) + sm_ws_bytes(plan);
}

// synchronise `st` and return the plan's flags as they were at that point; flags in
// clear_mask are reset on the device
int sm_read_flags(sm_plan *plan, hipStream_t st, int clear_mask, i32 out[4])
{
    hipLaunchKernelGGL(k_publish_flags, dim3(1), dim3(64), 0, st, plan->d_flags, plan->h_flags, clear_mask);
    SM_LAUNCH_CHECK("k_publish_flags");
    SM_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < 4; i++) out[i] = plan->h_flags[i];
    return SM_OK;
}

// Is `st` recording into a graph (hipStreamBeginCapture, torch.cuda.graph)?  Asked only on the paths that cannot be
// captured or need another protocol inside a capture: the steady state of a plain plan never calls it.
bool sm_stream_capturing(hipStream_t st, unsigned long long *id)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    unsigned long long cid = 0;
    if (hipStreamGetCaptureInfo(st, &cs, &cid) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (id) *id = cid;
    return cs != hipStreamCaptureStatusNone;
}

// ---------------------------------------------------------------------------
// argument rules shared by the entry points of every unit (sm_internal.h)
// ---------------------------------------------------------------------------

int sm_check_pairs(const sm_plan *plan, int pairs, const char *me)
{
    if (!plan) return sm_fail(SM_ERR_ARG, "%s: plan is NULL", me);
    if (pairs < 1 || pairs > plan->max_pairs)
        return sm_fail(SM_ERR_ARG, "%s: pairs %d outside 1..%d (max_pairs of the plan)", me, pairs, plan->max_pairs);
    return SM_OK;
}

int sm_check_pairs_loaded(const sm_plan *plan, int pairs, const char *me)
{
    if (pairs > plan->pairs_loaded)
        return sm_fail(SM_ERR_ARG, "%s: %d pairs requested but edges of only %d are loaded "
                       "(call sm_find_edges or sm_load_edges first)", me, pairs, plan->pairs_loaded);
    return SM_OK;
}

int sm_check_threshold(double threshold, const char *)
{
    if (!(threshold >= 0.0 && threshold <= 1.0)) return sm_fail(SM_ERR_ARG, "error: threshold must be between 0 and 1");
    return SM_OK;
}

int sm_check_web_type(const sm_plan *plan, int web_type, const char *me)
{
    if (web_type != SM_WEB_I32 && web_type != SM_WEB_U16 && web_type != SM_WEB_U8)
        return sm_fail(SM_ERR_ARG, "%s: web_type %d is not SM_WEB_I32/U16/U8", me, web_type);
    if ((web_type == SM_WEB_U8 && plan->num_shifts > 255) || (web_type == SM_WEB_U16 && plan->num_shifts > 65535))
        return sm_fail(SM_ERR_ARG, "%s: %d shifts do not fit the requested web type", me, plan->num_shifts);
    return SM_OK;
}

int sm_check_reach(const sm_plan *plan, int max_shifts, const char *me)
{
    const int n = 2 * (plan->square_width / 2) + 1;
    if (n > 25 || plan->num_shifts > max_shifts)
        return sm_fail(SM_ERR_ARG, "%s: built for windows up to 25x25 and at most %d shifts (got %dx%d, %d)", me, max_shifts,
                       n, n, plan->num_shifts);
    return SM_OK;
}

int sm_check_census_width(int census_width, const char *me)
{
    if (census_width != 3 && census_width != 5 && census_width != 7)
        return sm_fail(SM_ERR_ARG, "%s: census_width %d is not 3, 5 or 7", me, census_width);
    return SM_OK;
}

int sm_check_map_type(int map_type, const char *me, size_t *elem)
{
    if (map_type != SM_MAP_I32 && map_type != SM_MAP_I16)
        return sm_fail(SM_ERR_ARG, "%s: map_type %d is neither SM_MAP_I32 nor SM_MAP_I16", me, map_type);
    *elem = map_type == SM_MAP_I32 ? sizeof(i32) : sizeof(int16_t);
    return SM_OK;
}

int sm_check_lr_maps(const sm_plan *plan, int pairs, const int32_t *d_web, const int32_t *d_best,
                     const int32_t *d_web_right, const int16_t *d_sub, const int32_t *d_rejected, const char *me)
{
    const size_t map = (size_t)pairs * plan->width * plan->height * sizeof(i32);
    if ((d_best && overlap(d_best, d_web, map)) || (d_web_right && overlap(d_web_right, d_web, map)) ||
        (d_best && d_web_right && overlap(d_best, d_web_right, map)) ||
        (d_sub && (overlap(d_sub, d_web, map / 2, map) || (d_best && overlap(d_sub, d_best, map / 2, map)) ||
                   (d_web_right && overlap(d_sub, d_web_right, map / 2, map)))))
        return sm_fail(SM_ERR_ARG, "%s: result maps overlap", me);
    const size_t counts = (size_t)pairs * sizeof(i32);
    if (d_rejected && (overlap(d_rejected, d_web, counts, map) || (d_best && overlap(d_rejected, d_best, counts, map)) ||
                       (d_web_right && overlap(d_rejected, d_web_right, counts, map)) ||
                       (d_sub && overlap(d_rejected, d_sub, counts, map / 2))))
        return sm_fail(SM_ERR_ARG, "%s: d_rejected overlaps a map", me);
    return SM_OK;
}
