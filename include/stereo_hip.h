/*
 * stereo_hip.h -- C ABI of the MI355X (gfx950) stereo-matching layer.
 *
 * This is the drop-in boundary for the reference's one data-parallel hot path
 * (per-shift match cost -> S x S window aggregation -> winner-take-all) plus
 * the stages either side of it.  Plain C: opaque plan handle, raw pointers,
 * sizes and a stream handle (a hipStream_t passed as void *, NULL = default
 * stream).  No C++ or torch types cross it.  The reference has no FFI of its
 * own: its boundary is main()/algorithm() calling file-local kernels, so each
 * entry point names the reference code it replaces (paths relative to
 * /root/reference).  INTEGRATION.md shows the reference-side call sites.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero (an SM_ERR_* code) on
 *     failure; sm_last_error() then returns a message for the calling thread.
 *     The reference's convention on any GPU API failure is "message on
 *     stderr, exit(EXIT_FAILURE)" (src/helper_cuda.h:890-901); callers keep
 *     that by printing sm_last_error() and exiting 1.
 *   - d_* pointers are device (HBM) addresses owned by the caller; the plan
 *     owns only its private workspace.
 *   - launches are asynchronous on the given stream; nothing here
 *     synchronises except sm_stream_sync, sm_memcpy_* and sm_plan_status.
 *   - a plan is a single-threaded, single-stream object: its workspace (the packed edge images,
 *     the staging map of the narrow results of the fallback kernels, the timing events) is shared
 *     by all calls on it, so calls on ONE plan must come from one thread at a time and their
 *     launches must be ordered (one stream, or streams chained with events).  Concurrency comes
 *     from several plans (stereopar-batch: one per device thread), not from sharing one.
 *   - images are row-major, W*H elements, no padding.  A batch of pairs is
 *     `pairs` consecutive images.  The ghost-border variant needs no padded
 *     arrays (src/ghost.h): the halo is synthesised inside the kernels.
 */
#ifndef STEREO_HIP_H
#define STEREO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SM_OK            0
#define SM_ERR_ARG       1 /* invalid argument */
#define SM_ERR_HIP       2 /* a HIP runtime call or a launch failed */
#define SM_ERR_NOMEM     3 /* device or host allocation failed */
#define SM_ERR_ZERO_DIV  4 /* contour interval is 0 (the reference traps: SIGFPE) */

/* border handling: stereo.c (wrap-around idx(), src/util.h:42-47) or
 * stereo-ghost.c (zero / 128.0 halos, src/stereo-ghost.c:286-287,:384-385) */
enum sm_border { SM_TOROIDAL = 0, SM_GHOST = 1 };

typedef struct sm_plan sm_plan;

/* message for the last failure on this thread ("" if none) */
const char *sm_last_error(void);

/* number of visible HIP devices */
int sm_device_count(int *count);

/* ---- device memory helpers (what ALLOCATE_GPU / MAKE_GPU_COPY /
 * MAKE_HOST_COPY of src/util.h:119-152 did; buffers come back zero-filled
 * like cuda_xmalloc, src/util.h:119-129) -------------------------------- */
int sm_malloc(int device, size_t bytes, void **d_ptr);
int sm_free(int device, void *d_ptr);
int sm_memcpy_h2d(int device, void *d_dst, const void *h_src, size_t bytes);
int sm_memcpy_d2h(int device, void *h_dst, const void *d_src, size_t bytes);
int sm_stream_sync(int device, void *stream);

/* pinned (page-locked) host buffers and asynchronous copies on a stream, for
 * callers that feed pairs from host memory and want the transfers to overlap
 * the kernels of neighbouring pairs (the reference copies synchronously from
 * pageable memory, src/util.h:131-143).  sm_stream_create/destroy hand out
 * plain hipStream_t handles for callers without a HIP runtime of their own.  */
int sm_host_alloc(size_t bytes, void **h_ptr);
int sm_host_free(void *h_ptr);
int sm_memcpy_h2d_async(int device, void *d_dst, const void *h_src, size_t bytes, void *stream);
int sm_memcpy_d2h_async(int device, void *h_dst, const void *d_src, size_t bytes, void *stream);
int sm_stream_create(int device, void **stream);
int sm_stream_destroy(int device, void *stream);
/* events order work ACROSS streams: a host that keeps uploads, kernels and downloads on three
 * streams of their own (each copy direction then has a DMA queue to itself and the two
 * directions of the link run at the same time) chains them with these.  sm_event_sync blocks
 * the calling thread until the recorded work has finished.                                  */
int sm_event_create(int device, void **event);
int sm_event_destroy(int device, void *event);
int sm_event_record(int device, void *event, void *stream);
int sm_stream_wait_event(int device, void *stream, void *event);
int sm_event_sync(int device, void *event);

/* ---- result collection across the GPUs of one node: RCCL over xGMI ------- *
 * New work (the reference drives one GPU and copies its map to the host: src/stereo.cu:402-403,
 * src/image.cu:15-23).  The hot path shards with no data-path collective -- pair j -> device j mod n,
 * SURVEY.md 8e -- and these calls are what BASELINE.json's north star names RCCL for: a broadcast of a
 * parameter block and the collection of the result maps on one GPU.  ONE process drives the n devices
 * (ncclCommInitAll; each call below enqueues the operations of all ranks inside one ncclGroupStart /
 * ncclGroupEnd); rank r is devices[r], the root is rank 0.  All calls are asynchronous on the streams
 * given (streams[r] on device r; NULL = every default stream).  librccl.so is loaded by sm_comm_create,
 * not with this library.  (A host that wants its maps in HOST memory is better served by one download
 * per device -- n PCIe links instead of one -- which is what host/stereopar_batch.c does.)            */
typedef struct sm_comm sm_comm;
/* The RCCL build to load instead of the default names (librccl.so.1, librccl.so, /opt/rocm/lib/librccl.so.1): a path,
 * before the first sm_comm_create of the process.  A library that exports the symbol sm_rccl_host_stand_in is taken
 * for a HOST stand-in (tests/rccl_stub.c): its communicators are driven with host buffers and no device is touched,
 * which is how the grouped send / receive order of sm_gather_maps is rehearsed where fewer than two GPUs exist.      */
int sm_comm_set_rccl_library(const char *path);
int sm_comm_create(const int *devices, int n, sm_comm **out);     /* every device at most once */
void sm_comm_destroy(sm_comm *comm);
int sm_comm_size(const sm_comm *comm);
/* bytes at d_buf[0] (device 0 of the communicator) -> d_buf[r] on every device r */
int sm_broadcast(sm_comm *comm, void *const *d_buf, size_t bytes, void *const *streams);
/* rank r contributes bytes[r] bytes at d_src[r]; the root receives them back to back, in rank order, at
 * d_dst (its own share is a copy on its device; ranks with bytes[r] == 0 take no part): point-to-point
 * ncclSend / ncclRecv, all in flight together.  The caller maps rank order to pair order (pair j -> rank
 * j mod n: host/batch_index.h).                                                                       */
int sm_gather_maps(sm_comm *comm, void *const *d_src, const size_t *bytes, void *d_dst, void *const *streams);

/* ---- plan: geometry + private workspace for one image size ------------- *
 * num_shifts  = the reference's compile-time NUM_SHIFTS (src/stereo.c:6),
 *               here a run-time value, 1..65535
 * square_width = argv[4] of the reference (src/stereo.c:365); the window is
 *               (2*(square_width/2)+1)^2; 0 <= square_width <= min(W,H)
 *               (src/stereo.c:382-385)
 * max_pairs   = largest batch a single call will be given (>= 1)          */
int sm_plan_create(int device, int width, int height, int num_shifts,
                   int square_width, int border, int max_pairs, sm_plan **out);
void sm_plan_destroy(sm_plan *plan);

/* The same with an explicit choice of kernel variant and tiling: what tuning runs, same-device
 * A/B measurements and the tests that walk every built kernel need.  Every field 0 (or a NULL
 * `options`) = the plan's own choice, which is what sm_plan_create takes; a choice that does not
 * apply to the kernel the plan uses is ignored (sm_plan_describe / sm_plan_geometry say what was
 * taken).  The library reads no environment variable.                                      */
typedef struct sm_plan_options {
    int struct_size;            /* sizeof(sm_plan_options) as the caller compiled it: a shorter (older) struct leaves the
                                 * missing fields 0, of a longer (newer) one the fields this library knows are taken;
                                 * 0 is read as "no field set" (so `sm_plan_options o = {0}` is valid) */
    int kernel_family;          /* 1 = the popcount kernels (general fallback) even where the bit-sliced one is built */
    int tile_h;                 /* match kernel: output rows per wave */
    int shifts_per_lane;        /* bit-sliced kernel: 4, 8 or 16 */
    int workgroup_waves;        /* bit-sliced kernel: 1 = one-wave workgroups, 2 = two-wave workgroups (shared warm-up) */
    int no_two_wave_cap;        /* 1 = never launch the variant capped at two waves per SIMD */
    unsigned priority_pattern;  /* no effect; kept for the struct layout */
    int edge_kernel;            /* 1 = the one-pixel-per-lane edge kernel even where the four-pixel one applies */
    int timing_by_records;      /* 1 = sm_plan_time_kernels brackets launches with event records instead of
                                 *     reading the dispatch's own time stamps */
    int cost_pixels_per_lane;   /* no effect; kept for the struct layout */
    int cost_tile_h;            /* SAD / SSD kernels: output rows per wave */
    int cost_kernel;            /* 1 = the general masked kernel even where the quad-SAD / MFMA kernels apply;
                                   any other value = the plan's choice */
    int priority_class;         /* no effect; kept for the struct layout */
    int priority_on_change;     /* no effect; kept for the struct layout */
    int lane_merge;             /* bit-sliced kernel: how the lanes that split a word's shift range are merged:
                                 * 1 = per row with DPP, 2 = through LDS every four rows (where >= 4 lanes share a word);
                                 * 0 = the plan's choice */
    int no_four_shift_lanes;    /* bit-sliced kernel: 1 = never 4 shifts per lane (the plan's own choice is between 16, 8
                                 * and 4); shifts_per_lane = 4 forces them where they are built */
    int priority_unit_log2;     /* no effect; kept for the struct layout */
    int cost_workgroup_waves;   /* SAD kernel of round 5 (prefix chains) and SSD matrix-core kernel: 1, 2 or 4 waves per
                                 * workgroup sharing the staged rows; 0 = the plan's choice */
} sm_plan_options;
int sm_plan_create_ex(int device, int width, int height, int num_shifts, int square_width,
                      int border, int max_pairs, const sm_plan_options *options, sm_plan **out);

/* human-readable description of the kernel variant and tiling the plan
 * selected (for logs / bench.py); the string lives as long as the plan */
const char *sm_plan_describe(const sm_plan *plan);
/* the geometry the plan selected (kernel variant, tiling, packed-image extents):
 * what analytic cost models and tests need; plain ints only */
typedef struct sm_geometry {
    int kernel;            /* 0..2 popcount kernels A/B/C, 3 generic, 4 bit-sliced */
    int window;            /* n = 2*(square_width/2)+1 */
    int shifts_per_lane;   /* shifts one lane carries */
    int shift_lanes;       /* lanes that split one pixel group's shift range */
    int threads;           /* per workgroup */
    int tile_w, tile_h;    /* output pixels per workgroup (tile_h / waves_per_workgroup rows per wave) */
    int tiles_x, tiles_y;  /* grid (x pairs in z) */
    int ext_words, ext_rows, pad_l;   /* packed edge image: u32 words per row, rows, left pad px */
    int lds_bytes;         /* dynamic LDS request per workgroup */
    int two_wave_variant;  /* bit-sliced kernel capped at two waves per SIMD */
    int edge_rows_per_wave;/* packed-image rows one wave of the edge kernel produces */
    int waves_per_workgroup; /* bit-sliced kernel: 1, or 2 = the upper and the lower half of a tile,
                              * sharing the window rows around the middle */
    int lane_merge_lds;      /* bit-sliced kernel: the lanes that split a word's shift range are merged through LDS
                              * every four rows (1) or per row with DPP (0) */
} sm_geometry;
/* sm_plan_geometry writes sizeof(sm_geometry) bytes AS THIS HEADER DECLARES IT: the struct grows at its end from
 * release to release, so a caller that may meet a newer library than the header it was compiled against (bindings,
 * plug-ins) passes the size of ITS struct to sm_plan_geometry_sized -- the fields it knows are filled in, nothing is
 * written past them; a struct newer than the library gets its unknown tail zeroed.                               */
int sm_plan_geometry(const sm_plan *plan, sm_geometry *out);
int sm_plan_geometry_sized(const sm_plan *plan, sm_geometry *out, size_t size_of_callers_struct);
/* bytes of private device workspace */
size_t sm_plan_workspace_bytes(const sm_plan *plan);
/* Narrow result maps (sm_match_wta_typed / sm_run_typed with SM_WEB_U8 / SM_WEB_U16) of the kernels that
 * have no narrow store path of their own -- every kernel but the bit-sliced one, see sm_plan_describe --
 * go through an int32 staging map of max_pairs * W * H * 4 bytes (about 265 MB for 8 pairs at 4K).  It is
 * NOT part of a new plan: a caller that only ever asks for int32 maps never pays for it.  This call
 * allocates it (counted in sm_plan_workspace_bytes from then on); without it the first narrow request does,
 * inside that call -- a hipMalloc, which synchronises the device, so callers that time their launches call
 * this next to their own allocations.  A no-op for plans that do not need the map.  SM_ERR_NOMEM on failure. */
int sm_plan_reserve_narrow(sm_plan *plan);

/* ---- step 1: edges ------------------------------------------------------ *
 * replaces find_all_edges<<<>>> (src/stereo.cu:27-92, ghost twin
 * src/stereo-ghost.cu) for `pairs` x 2 images.  Input is uint8 gray (the
 * reference's double brightness is k/256.0, src/image.c:9-15; the decision
 * is evaluated in the same IEEE double arithmetic).  Writes the packed edge
 * bits the hot path consumes into the plan workspace and, when d_edges_* are
 * non-NULL, the reference's u8 {0,1} edge images as well.                  */
int sm_find_edges(sm_plan *plan, const uint8_t *d_gray_left,
                  const uint8_t *d_gray_right, double threshold, int pairs,
                  uint8_t *d_edges_left, uint8_t *d_edges_right, void *stream);

/* Set-up for sm_find_edges that depends on the threshold only (the decision
 * tables, built and verified on the device, with one host read-back of the
 * verdict).  sm_find_edges does this by itself the first time it sees a
 * threshold; a caller that knows the threshold in advance calls this next to
 * its allocations, as the reference allocates before its timed region
 * (src/stereo.cu:296-308).                                                  */
int sm_plan_prepare_threshold(sm_plan *plan, double threshold, void *stream);

/* alternative entry to the hot path for callers that already hold u8 {0,1}
 * edge images (the arguments of fillup_matches, src/stereo.cu:127): packs
 * them into the plan workspace                                              */
int sm_load_edges(sm_plan *plan, const uint8_t *d_edges_left,
                  const uint8_t *d_edges_right, int pairs, void *stream);

/* ---- step 2: THE HOT PATH ---------------------------------------------- *
 * one fused launch that replaces fillup_matches (src/stereo.cu:127-137),
 * the NUM_SHIFTS x {cudaMemset, addup_pixels_in_square, record_score} loop
 * (src/stereo.cu:142-207) and find_highest_scoring_shifts
 * (src/stereo.cu:211-225), for the edges last given to sm_find_edges /
 * sm_load_edges.  d_web receives the winning shift 1..num_shifts per pixel
 * (int32, the reference's `web`); d_best, if non-NULL, the winning masked
 * score (the reference's `buf`, dumped as score_best-0).                    */
int sm_match_wta(sm_plan *plan, int pairs, int32_t *d_web, int32_t *d_best,
                 void *stream);

/* The same launch with a NARROW web map: the values are shift indices 1..num_shifts, so
 * they fit uint8 (num_shifts <= 255) or uint16; d_web then points to W*H elements of that
 * type per pair.  The reference's type is int32 (src/stereo.cu:304, the D2H copy of
 * src/image.cu:15-23 moves 4 bytes per pixel); a caller that takes its results to the
 * host moves 4x / 2x fewer bytes over PCIe this way.  d_best stays int32.              */
#define SM_WEB_I32 0
#define SM_WEB_U16 1
#define SM_WEB_U8  2
int sm_match_wta_typed(sm_plan *plan, int pairs, void *d_web, int web_type,
                       int32_t *d_best, void *stream);

/* Let consecutive sm_run calls overlap.  With the flag set, call i runs on one of two
 * internal streams ("lanes", i & 1), edge detection and match launch in order, into the
 * lane's own half of a double-buffered workspace; nothing orders the lanes against each
 * other, so the edge detection of call i + 1 runs beside the match kernel of call i and
 * the first waves of match i + 1 take the SIMD slots the early finishers of match i
 * leave.  `stream` waits for the call's release event: synchronising `stream` still
 * means "all results are there", and work put on `stream` after the call sees them.
 * Two consecutive calls that share anything -- overlapping result maps, a changed
 * threshold (the decision tables are rebuilt), the staging map of a narrow result from
 * a fallback kernel -- are put in order by the library; give consecutive calls their
 * own result maps to get the overlap.  At most two calls are in flight.  The caller
 * promises that, when sm_run is called, the input images are complete in memory and no
 * work of its own that is still pending (on `stream` or elsewhere) reads or writes the
 * result maps it hands over: the call is no longer ordered behind earlier work on
 * `stream`, only behind earlier sm_run calls.  enabled = 2 keeps that ordering too (one
 * more event per call, and no overlap with the call before, whose results `stream`
 * waits for): use it when the inputs are uploaded asynchronously on `stream` just
 * before sm_run.  sm_plan_kernel_ms then measures launches that share the chip with
 * their neighbours: longer each, shorter together.  Off by default.                  */
int sm_plan_set_pipelined(sm_plan *plan, int enabled);

/* Measurement aid: with capacity > 0 the plan brackets each of the next
 * `capacity` sm_match_wta / sm_run match launches with HIP events ON THE STREAM
 * THE KERNEL IS LAUNCHED ON (capacity 0 turns it off and frees the events).
 * sm_plan_kernel_ms synchronises those events and returns the mean duration
 * in milliseconds and the number of launches recorded since the last reset.  */
int sm_plan_time_kernels(sm_plan *plan, int capacity);
int sm_plan_kernel_ms(sm_plan *plan, double *mean_ms, int *launches);
/* An event record costs a few microseconds on the launch stream (measured:
 * 8 us per step with both brackets on every launch, 6 % of a 4K step), so a
 * throughput measurement brackets only every `every`-th match launch (default
 * 1 = all of them).  Resets the launch counter.                              */
int sm_plan_time_stride(sm_plan *plan, int every);

/* steps 1 + 2 back to back: uint8 pairs in, web out */
int sm_run(sm_plan *plan, const uint8_t *d_gray_left,
           const uint8_t *d_gray_right, double threshold, int pairs,
           int32_t *d_web, int32_t *d_best, void *stream);

/* sm_run_typed whose only INPUT dependency is an event -- instead of "everything enqueued on `stream` before the call"
 * (the reference synchronises on its uploads before every pair: src/stereo.cu:402-403).  `inputs_ready_event` (a
 * hipEvent_t, e.g. recorded behind the upload of this pair on a copy stream; NULL = the images are complete now) is all
 * the call waits for besides earlier calls on the same plan that share something with it (result maps, the threshold
 * tables, the narrow staging map: put in order by the library); work enqueued on `stream` AFTER the call sees the
 * results.  That freedom is what lets consecutive calls overlap, and the plan takes it by itself: a match launch of
 * fewer than 2 x 1024 waves (a lone pair up to 4K: it cannot fill the chip twice over, and the next call's edge
 * detection and first waves fit beside its tail) runs on the plan's two internal lanes as under
 * sm_plan_set_pipelined(1); larger launches, and plans of more than 128 shifts (the edge detection the overlap hides is a small
 * part of their step, and two calls sharing the chip cost more than it), run in `stream` order behind the event.  Give consecutive calls their
 * own result maps.  Inside a stream capture the event must be one recorded in the same capture.                    */
int sm_run_after(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right,
                 double threshold, int pairs, void *d_web, int web_type, int32_t *d_best,
                 void *stream, void *inputs_ready_event);

/* STREAM CAPTURE (hipStreamBeginCapture on `stream`, torch.cuda.graph): sm_run, sm_find_edges, sm_match_wta and
 * sm_cost_wta may be recorded into a graph and replayed; a plan is single-stream, so do not run it eagerly while a
 * graph that holds its launches is in flight.  What cannot be captured returns SM_ERR_ARG with a message that names
 * the remedy, and leaves the capture valid:
 *   - a threshold whose decision tables are not built yet (their set-up reads a verdict back to the host):
 *     call sm_plan_prepare_threshold before the capture begins;
 *   - a match launch with kernel timing armed (its events cannot be read back from a graph):
 *     sm_plan_time_kernels(plan, 0) before the capture;
 *   - the first narrow result of a plan whose kernel needs the int32 staging map (an allocation):
 *     sm_plan_reserve_narrow before the capture.
 * A bad argument (a NULL image or map, an unknown web_type, a narrow map too small for the shift count) is refused
 * after those conditions, likewise before anything is captured, and leaves the capture valid.
 * A PIPELINED plan is captured with a protocol of its own: the lane of a call leaves `stream` at an event the
 * previous captured call recorded before it joined its own lane back, so consecutive calls still run side by side
 * inside the graph, every call joins at once (a capture may end after any call), and -- unlike outside a capture --
 * every call is ordered behind the work captured on `stream` before the capture's FIRST sm_run.  (Round 4 saw a
 * crash here: its lanes waited for release events recorded before the capture began, which the runtime answers with
 * hipErrorStreamCaptureIsolation; tools/capture_probe.hip.)                                                        */

/* sm_run with a narrow web map (see sm_match_wta_typed) */
int sm_run_typed(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right,
                 double threshold, int pairs, void *d_web, int web_type, int32_t *d_best,
                 void *stream);

/* ---- SAD / SSD cost mode: PARITY UNPINNED ---------------------------------- *
 * BASELINE.json words the hot path as "SAD/SSD cost, window aggregation,
 * arg-min"; the reference implements the edge-equality cost above and nothing
 * else, so this entry has NO reference counterpart.  Same skeleton on the uint8
 * gray images themselves: c_d = |L(x,y) - R(x+d,y)| or its square, n x n box
 * sum, best = min over d, web = 1 + the FIRST d reaching it; borders as the
 * reference treats its edge images (wrap, or zeros past the border and no taps
 * outside the image).  Defined by oracle/stereo_oracle.c smo_cost_hot_path.
 * Windows up to 25 x 25, num_shifts <= 512.  SAD windows 3 .. 21 run on the
 * quad-SAD unit, SSD windows 3 .. 11 with up to 256 shifts on the matrix cores,
 * the ghost border's columns x < half behind them on a kernel of their own
 * (DESIGN.md 5.4); everything else on a general kernel -- the same results by
 * definition (tests: every path against the definition).                     */
#define SM_COST_SAD 1
#define SM_COST_SSD 2
int sm_cost_wta(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right,
                int cost, int pairs, int32_t *d_web, int32_t *d_best, void *stream);

/* Subpixel refinement of the cost mode: from a whole-pixel map d_web of sm_cost_wta and the
 * same gray pair, d_sub (int16, [pairs][H][W]) receives the disparity in 1/16 of a shift.  Per pixel, with
 * s = web(x, y) and C(d) the window cost at shift index d exactly as sm_cost_wta sums it:
 *   s outside 1..D: sub = 0 (no taps);   s == 1 or s == D: sub = 16 s;
 *   otherwise a = C(s-2) - C(s-1), b = C(s) - C(s-1) and
 *     SM_COST_SSD (parabola):    q = floor((16 (a - b) + den) / (2 den)), den = a + b,
 *     SM_COST_SAD (equiangular): q = floor((16 (a - b) + m) / (2 m)),     m = max(a, b),
 *   q = 0 where the denominator is <= 0, else clamped to [-8, 8];  sub = 16 s + q.
 * sub / 16 - 1 is the subpixel shift (left x matches right x + d).  For a map of sm_cost_wta on the same
 * images a >= 1 and b >= 0 (first wins), so the clamp never applies.  Work per pixel is 3 n^2 taps, not
 * D n^2.  d_costs: NULL, or [pairs][3][H][W] int32 receiving C(s-2), C(s-1), C(s), -1 where a shift or the
 * pixel has no cost.  Arguments are checked as sm_cost_wta checks them; runs in `stream` order and allocates
 * nothing, so it may be captured.                                                                      */
int sm_cost_refine(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int cost, int pairs,
                   const int32_t *d_web, int16_t *d_sub, int32_t *d_costs, void *stream);

/* debug tap: materialise the per-shift planes the reference dumps in debug
 * builds (matches-i, score_all-i, scores-i; src/stereo.c:98-104,:158-164,
 * :189) for one shift of one pair.  Any output may be NULL.  Slow path.    */
int sm_debug_planes(sm_plan *plan, int pair, int shift, uint8_t *d_match,
                    int32_t *d_score_all, int32_t *d_scores, void *stream);

/* debug tap: the device's edge decision (the 3-vs-3 contrast test of
 * src/stereo.c:19-27) for EVERY pair of in-image side sums: d_table receives
 * 766*766 bytes, table[sa*766+sb] in {0,1}, sums in units of 1/256.  Lets a
 * test prove the device arithmetic equals the host's for a threshold.       */
int sm_debug_edge_table(int device, double threshold, uint8_t *d_table, void *stream);

/* debug tap: the same table, but decided the way sm_find_edges decides it --
 * through the per-threshold integer lo/hi tables.
 * *not_threshold_form is set to 1 if the exact test was found not to be of
 * "true prefix / false middle / true suffix" form for some left sum, in which
 * case sm_find_edges falls back to the double arithmetic.  Synchronises.     */
int sm_debug_edge_table_fast(sm_plan *plan, double threshold, uint8_t *d_table,
                             int *not_threshold_form, void *stream);

/* debug tap, for tests only: fill the plan's lazily allocated workspaces with `word`, so that a stage which
 * reads a workspace word before it has written it in the same call gives a wrong result instead of one that is
 * right by luck (fresh device memory is very often zero).  Makes the plan's device current, synchronises the
 * device (both lanes of the plan with it), fills every workspace that is allocated and is NOT zero-filled on
 * allocation over its whole extent with the 32-bit word, and synchronises again.  The zero-filled workspace
 * (the mirrored packed images of the consistency check) is left alone: the words beyond each side's row
 * extent are zero by invariant, written by no call, and every match launch reads them, so poisoning them would
 * break the plan instead of testing a stage.  Workspaces that are not allocated are skipped and nothing is
 * allocated (reserve them first: sm_plan_reserve_*); the plan's permanent buffers -- packed images, tables,
 * lane state -- are not touched.  SM_ERR_ARG for a NULL plan.  Must NOT be called while a stream is capturing
 * (it synchronises the device), nor while another thread uses the plan.                                    */
int sm_debug_poison_workspace(sm_plan *plan, uint32_t word);

/* ---- left-right consistency check ---------------------------------------- *
 * New work (the reference matches one way only: each LEFT pixel's winning shift, src/stereo.cu:211-225).
 * The check marks the left pixels whose match does not point back to them with 0 -- the value
 * fill_web_holes (src/stereo.cu:235-256, sm_fill_web_holes, sm_step3's staged route) fills, and one the
 * reference's matcher never produces.  Definition (oracle/stereo_oracle.c notation):
 *   web_right = mirror(smo_hot_path(mirror(eR), mirror(eL))), mirror(a)(x) = a(W-1-x), and likewise
 *   best_right: web_right(u,y) = s' means right pixel u matched left pixel u - (s'-1);
 *   left pixel (x,y) with s = web(x,y) matched right pixel u = x + s - 1 (toroidal: mod W; ghost: u >= W
 *   is the halo, and the pixel is rejected); it is kept iff |web_right(u,y) - s| <= max_diff, and the
 *   checked map holds s where kept, 0 where rejected.
 * The maps given to sm_lr_check come from the same plan and pairs (every value in 1..num_shifts); other
 * values get what the formula gives (ghost: u outside 0..W-1 is rejected) and no read outside a row.
 * Narrow maps have no consistency check; the SAD / SSD cost mode has its own (sm_cost_lr, below).  The
 * workspace (mirrored packed images and one mirrored-order map per pair) is allocated by sm_plan_reserve_lr or, without it, by the
 * first call that needs it (a hipMalloc, which synchronises the device).  All calls run in `stream`
 * order; on a pipelined plan (sm_plan_set_pipelined, sm_run_after) `stream` first waits for every
 * earlier call on the lanes, and the next call on the lanes waits for this one.  STREAM CAPTURE: as
 * sm_run, once sm_plan_reserve_lr (and, for sm_run_lr, sm_plan_prepare_threshold) has been called;
 * before, the call is refused with SM_ERR_ARG, a message naming the remedy, and the capture valid.     */
/* adds: the right-reference map (and, d_best_right non-NULL, its winning scores) for the edges last given to
 * sm_find_edges / sm_load_edges, in natural order -- the plan's match launch over mirrored packed images */
int sm_match_wta_right(sm_plan *plan, int pairs, int32_t *d_web_right, int32_t *d_best_right, void *stream);
/* adds: the check of d_web against d_web_right (both natural order) with tolerance max_diff >= 0 into
 * d_web_out, which may equal d_web (in place) and must not overlap d_web_right; d_rejected: NULL or one
 * int32 per pair, the number of rejected pixels                                                          */
int sm_lr_check(sm_plan *plan, const int32_t *d_web, const int32_t *d_web_right, int max_diff,
                int pairs, int32_t *d_web_out, int32_t *d_rejected, void *stream);
/* adds: edges (as sm_find_edges: they stay loaded) + left match + right match + check in one call; d_web
 * receives the checked map (0 = rejected), d_best the left match's scores; d_best / d_web_right (the
 * right-reference map, natural order) / d_rejected may be NULL                                          */
int sm_run_lr(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, double threshold,
              int pairs, int max_diff, int32_t *d_web, int32_t *d_best, int32_t *d_web_right,
              int32_t *d_rejected, void *stream);
/* adds: allocates the mirrored packed images and the mirrored-order map of the calls above (counted in
 * sm_plan_workspace_bytes from then on); a plan that never calls them allocates neither.  Idempotent.
 * The map is shared with the cost mode's check below: if sm_plan_reserve_cost_lr came first, only the
 * mirrored packed images are added.                                                                    */
int sm_plan_reserve_lr(sm_plan *plan);

/* ---- left-right consistency check of the SAD / SSD cost mode --------------- *
 * The same check with sm_cost_wta's map in place of the edge matcher's:
 *   (best_right, web_right) = mirror(smo_cost_hot_path(mirror(R), mirror(L), D, S, border, cost)),
 * i.e. right pixel u is scored against left pixel u - d: |R(u) - L(u - d)| or its square, toroidal:
 * u - d mod W, ghost: L is 0 left of column 0 and window taps outside the image count 0; the minimum
 * wins, the first shift on a tie.  The check of sm_lr_check then keeps left pixel x with s = web(x,y)
 * iff |web_right(x + s - 1, y) - s| <= max_diff (toroidal: mod W; ghost: a match into the halo is
 * rejected) and writes 0 for the others.  int32 maps only; windows up to 25 x 25 and at most 512 shifts
 * (as sm_cost_wta's general kernel).  The right-reference map is the plan's own cost launch over the
 * mirrored gray images, so every cost kernel sm_cost_wta can choose has a right-reference mode.
 * Workspace: the mirrored gray images, 2 * round_up(max_pairs * W * H, 256) bytes, and the mirrored-order
 * map of sm_plan_reserve_lr (max_pairs * W * H int32; allocated here unless the edge check has it
 * already); allocated by sm_plan_reserve_cost_lr or, without it, by the first call that needs it (a
 * hipMalloc, which synchronises the device), counted in sm_plan_workspace_bytes from then on, freed by
 * sm_plan_destroy.  Arguments are checked before any device call.  All calls run in `stream` order; they
 * use nothing the pipelined lanes use (sm_plan_set_pipelined, sm_run_after), so they neither wait for
 * the lanes nor hold the next call on the lanes back.  The plan's calls share the mirrored-order map
 * (and sm_cost_wta's LDS set-up): keep them on one stream.  STREAM CAPTURE: as sm_cost_wta, once
 * sm_plan_reserve_cost_lr has been called; before, the call is refused with SM_ERR_ARG, a message naming
 * it, and the capture valid.                                                                            */
/* adds: the cost mode's right-reference map (and, d_best_right non-NULL, its winning costs), natural order */
int sm_cost_wta_right(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int cost,
                      int pairs, int32_t *d_web_right, int32_t *d_best_right, void *stream);
/* adds: left cost WTA + right cost WTA + check in one call; d_web = checked map (0 = rejected),
 * d_best = the left costs (exactly sm_cost_wta's); d_best / d_web_right / d_rejected may be NULL;
 * d_rejected: one int32 per pair, the number of rejected pixels                                          */
int sm_cost_lr(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int cost, int pairs,
               int max_diff, int32_t *d_web, int32_t *d_best, int32_t *d_web_right, int32_t *d_rejected,
               void *stream);
/* adds: allocates the mirrored gray images (and the mirrored-order map) of the two calls above; idempotent */
int sm_plan_reserve_cost_lr(sm_plan *plan);

/* ---- census cost mode: PARITY UNPINNED ------------------------------------- *
 * New work (no reference counterpart, like SAD / SSD).  A matching cost that only sees the ORDER of a
 * pixel against its neighbours, so a strictly increasing change of either image's intensities (gain, offset, gamma
 * of one camera) leaves every descriptor, and so every map, exactly as it was.  census_width c in {3, 5, 7} is a
 * per-call argument, independent of square_width; h = c / 2.
 *   descriptor C_I(x, y): a uint64; the neighbours (dx, dy) of the c x c window in row-major order (dy outer, dx
 *     inner) without (0, 0), the k-th gives bit k (bit 0 least significant) = I(x+dx, y+dy) < I(x, y), strictly;
 *     8, 24 or 48 bits, the higher ones 0.  Toroidal: neighbour coordinates wrap (mod W, mod H); ghost: a neighbour
 *     outside the image reads 0, so a halo pixel's descriptor is 0.
 *   cost c_d(x, y) = popcount(C_L(x, y) XOR C_R(x + d, y)); toroidal: x + d mod W; ghost: C_R = 0 for x + d >= W.
 *   A_d = n x n window sum of c_d (toroidal: taps wrap; ghost: taps outside the image count 0), A_d <= 48 * 625;
 *   best = min_d A_d, web = 1 + the FIRST d reaching it.
 *   right reference: (best_right, web_right) = mirror(census_wta(mirror(R), mirror(L))), mirror(a)(x) = a(W-1-x);
 *     mirroring permutes the bits of every descriptor alike, so the pass reads the left pass's descriptors in
 *     mirrored order.  The check is sm_lr_check's (section 10).
 *   subpixel: sm_cost_refine's SM_COST_SAD (equiangular) formula and edge rules on the census window costs
 *     C(s-2), C(s-1), C(s); d_costs -1 where a cost does not exist.
 * Windows up to 25 x 25 and at most 512 shifts.  Arguments are checked before any device call; a refusal names the
 * function.  Workspace: the descriptors of both images of max_pairs pairs (8 bytes per pixel, 133 MB per 4K pair;
 * 4-byte descriptors inside it for c <= 5) and the mirrored-order map of sm_plan_reserve_lr (added only if the plan has
 * none yet); allocated by sm_plan_reserve_census or, without it, by the first call that needs it (a hipMalloc, which
 * synchronises the device), counted in sm_plan_workspace_bytes from then on, freed by sm_plan_destroy.  A plan that
 * never calls these allocates nothing.  All calls run in `stream` order and use nothing the pipelined lanes use.
 * STREAM CAPTURE: once sm_plan_reserve_census has been called; before, a call that needs the workspace is refused
 * with SM_ERR_ARG, a message naming it, and the capture valid.                                                  */
/* adds: the descriptors of `images` consecutive gray images (images <= 2 * max_pairs) into d_desc, one uint64 per
 * pixel; needs no workspace                                                                                      */
int sm_census_transform(sm_plan *plan, const uint8_t *d_gray, int census_width, int images, uint64_t *d_desc,
                        void *stream);
/* adds: the census arg-min -> d_web (and, d_best non-NULL, the window costs), int32 maps */
int sm_census_wta(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width, int pairs,
                  int32_t *d_web, int32_t *d_best, void *stream);
/* adds: the right-reference map (and, d_best_right non-NULL, its costs), natural order */
int sm_census_wta_right(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width,
                        int pairs, int32_t *d_web_right, int32_t *d_best_right, void *stream);
/* adds: the descriptors once, left and right arg-min and the check (tolerance max_diff >= 0): d_web = checked map
 * (0 = rejected), d_best = the left costs; d_best / d_web_right / d_rejected (one int32 per pair) may be NULL    */
int sm_census_lr(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width, int pairs,
                 int max_diff, int32_t *d_web, int32_t *d_best, int32_t *d_web_right, int32_t *d_rejected,
                 void *stream);
/* adds: subpixel refinement of a census map: d_sub int16 in 1/16 of a shift; d_costs NULL or [pairs][3][H][W] */
int sm_census_refine(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width,
                     int pairs, const int32_t *d_web, int16_t *d_sub, int32_t *d_costs, void *stream);
/* adds: allocates the census workspace now; idempotent */
int sm_plan_reserve_census(sm_plan *plan);
/* ---- census cost mode, guided re-search: PARITY UNPINNED ---- *
 * The second step of a coarse-to-fine search: sm_census_wta's arg-min, but only over the shifts within `radius` of a
 * prior map -- the upsampled map of the half-resolution path, whose shifts are all even (sm_upsample_double).
 *   d_prior: an int32 web map [pairs][H][W], 1 + shift, 0 = invalid; any int32 value is legal.  radius r in 1..4.
 *   K(p) = { d : 0 <= d <= D - 1, |d - (prior(p) - 1)| <= r }; empty for prior(p) = 0 and for every prior so far
 *     outside 1 - r .. D + r that no d qualifies.
 *   K(p) empty: web = best = 0.  Otherwise best = min over K(p) of A_d(p), A_d sm_census_wta's window cost (all n x n
 *     taps with p's own d: the priors of the neighbours play no part), web = 1 + the least d of K(p) reaching it.
 *   So wherever |prior - sm_census_wta's web| <= r the two calls agree in web and best, and best is never smaller.
 *   right reference: mirror(near(mirror(R), mirror(L), mirror(prior_right))): the cost of right pixel u at d is
 *     popcount(C_R(u) XOR C_L(u - d)), toroidal u - d mod W, ghost C_L = 0 for u - d < 0.
 *   sm_census_near_lr: the descriptors once, both searches, then sm_lr_check's rule; NULL and overlap rules of
 *     sm_census_lr.  Subpixel: sm_census_refine takes the result as it takes any web map.
 * Both border modes, windows, shifts, workspace (sm_plan_reserve_census, nothing added) and STREAM CAPTURE as for the
 * calls above.  Refused before any device call: a NULL plan or required pointer, census_width, radius, pairs, the
 * window and shift limits, and an output that overlaps an image, a prior or another output (no in-place operation). */
/* adds: the left re-search -> d_web (and, d_best non-NULL, the window costs) */
int sm_census_wta_near(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width,
                       int pairs, const int32_t *d_prior, int radius, int32_t *d_web, int32_t *d_best, void *stream);
/* adds: the right-reference re-search around d_prior_right (a right-reference map), natural order */
int sm_census_wta_near_right(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width,
                             int pairs, const int32_t *d_prior_right, int radius, int32_t *d_web_right,
                             int32_t *d_best_right, void *stream);
/* adds: both re-searches and the check: d_web = checked map; d_best / d_web_right / d_rejected may be NULL */
int sm_census_near_lr(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width,
                      int pairs, const int32_t *d_prior, const int32_t *d_prior_right, int radius, int max_diff,
                      int32_t *d_web, int32_t *d_best, int32_t *d_web_right, int32_t *d_rejected, void *stream);

/* ---- semi-global matching over the census data term: PARITY UNPINNED ------ *
 * New work (no reference counterpart).  The census window cost aggregated along 4 or 8 image lines
 * instead of arg-minned directly, so depth follows the image across flat regions and stops at object boundaries.
 * Arguments: census_width c in {3, 5, 7}, penalties 0 <= p1 <= p2 <= 32767, paths in {4, 8}.  Definition:
 *   A(p, d)   = sm_census_wta's window cost (the plan's n x n box sum and border rules), d = 0 .. D - 1;
 *   directions r: (1,0) (-1,0) (0,1) (0,-1), and for 8 paths also (1,1) (-1,1) (1,-1) (-1,-1);
 *   L_r(p, d) = A(p, d) if q = p - r lies outside the image (paths never wrap, in either border mode), else
 *               A(p, d) + min(L_r(q, d), L_r(q, d-1) + p1, L_r(q, d+1) + p1, m_q + p2) - m_q, m_q = min_k L_r(q, k),
 *               terms with d-1 or d+1 outside 0 .. D - 1 dropped;  A <= L_r <= A + p2 (a u16 at every window size);
 *   S(p, d)   = sum over r of L_r(p, d); best = min_d S, web = 1 + the FIRST d reaching it;
 *   sub       = 16 s at s = web = 1 or D, else a = S(s-2) - S(s-1), b = S(s) - S(s-1), den = a + b,
 *               q = floor((16 (a - b) + den) / (2 den)) (0 if den <= 0), clamped to -8 .. 8, sub = 16 s + q
 *               (int16, 1/16 of a shift; sm_cost_refine's SSD rule on S);
 *   right reference: (best_right, web_right) = mirror(sgm(mirror(R), mirror(L))); the check is sm_lr_check's.
 * With p1 = p2 = 0, web is sm_census_wta's and best = paths * its best.  Windows up to 25 x 25 and at most 256
 * shifts.  Arguments are checked before any device call; a refusal names the function.  Workspace: the census
 * workspace (sm_plan_reserve_census: 16 * max_pairs * W * H bytes of descriptors, and the mirrored-order map,
 * 4 * max_pairs * W * H bytes, if the plan has none yet) and the volumes of ONE pair, 6 * W * H * Dp bytes with Dp =
 * the least of 64, 128 and 256 that holds num_shifts (12.7 GB at 3840 x 2160 and 256 shifts); a call of `pairs` pairs works
 * through them in turn, in stream order.  Allocated by sm_plan_reserve_sgm or, without it, by the first call that
 * needs it (a hipMalloc, which synchronises the device; SM_ERR_NOMEM if the device has not the room), counted in
 * sm_plan_workspace_bytes from then on, freed by sm_plan_destroy.  A plan that never calls these allocates none of
 * it.  All calls run in `stream` order and use nothing the pipelined lanes use.  STREAM CAPTURE: once
 * sm_plan_reserve_sgm has been called; before, the call is refused with SM_ERR_ARG, a message naming it, and the
 * capture valid.                                                                                                  */
/* adds: SGM arg-min -> d_web; d_best (min_d S) and d_sub (int16, 1/16 shift) may be NULL */
int sm_sgm_wta(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width,
               int p1, int p2, int paths, int pairs, int32_t *d_web, int32_t *d_best, int16_t *d_sub, void *stream);
/* adds: the right-reference map (and, non-NULL, its minima), natural order */
int sm_sgm_wta_right(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width,
                     int p1, int p2, int paths, int pairs, int32_t *d_web_right, int32_t *d_best_right, void *stream);
/* adds: descriptors once, left + right aggregation, check; d_web = checked map (0 = rejected); d_sub = the left
 * pass's subpixel map with 0 where rejected; d_best / d_web_right / d_rejected / d_sub may be NULL */
int sm_sgm_lr(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width,
              int p1, int p2, int paths, int pairs, int max_diff, int32_t *d_web, int32_t *d_best,
              int32_t *d_web_right, int32_t *d_rejected, int16_t *d_sub, void *stream);
/* adds: allocates the SGM workspace now; idempotent */
int sm_plan_reserve_sgm(sm_plan *plan);

/* ---- SGM: the left-right check from one aggregated volume: PARITY UNPINNED -- *
 * New work (no reference counterpart; how OpenCV's SGBM and libSGM get their right-reference disparity).
 * sm_sgm_lr aggregates twice, once per reference image.  Here the right map is read off the LEFT pass's aggregate S
 * along its diagonals, so one aggregation serves both maps.  Arguments and S as sm_sgm_wta's.  Definition:
 *   left maps   d_web / d_best / d_sub exactly as from sm_sgm_wta;
 *   right map   right pixel (u, y) takes candidate d from left pixel x = u - d:
 *               toroidal: every d = 0 .. D - 1, x = (u - d) mod W (D > W: the same x serves several d);
 *               ghost:    only d <= u (S has no column left of 0); d = 0 is always a candidate;
 *               best_right(u, y) = min over the candidates of S(y, x, d), web_right = 1 + the LEAST d reaching it;
 *   check       sm_lr_check's rule between web and this web_right; d_sub is 0 where it rejected.
 * This is ANOTHER right map than sm_sgm_wta_right's, not a faster route to it: the paths and the box window belong to
 * the left image only.  With p1 = p2 = 0 in toroidal mode web_right is sm_census_wta_right's.  Refusals: sm_sgm_wta's
 * and sm_sgm_lr's, in their order, with these names in them.  Workspace: the SGM workspace as it is (nothing new;
 * sm_plan_reserve_sgm), pairs going through the one volume in turn.  STREAM CAPTURE: as sm_sgm_wta.                */
/* adds: the unchecked left maps and the single-volume right maps, natural order; d_best, d_sub, d_best_right may be NULL */
int sm_sgm_wta_both(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width,
                    int p1, int p2, int paths, int pairs, int32_t *d_web, int32_t *d_best, int16_t *d_sub,
                    int32_t *d_web_right, int32_t *d_best_right, void *stream);
/* adds: sm_sgm_lr with the single-volume right map: one aggregation, then the check; parameters and NULL rules as
 * sm_sgm_lr's; d_web_right, where given, receives the single-volume map */
int sm_sgm_lr_single(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width,
                     int p1, int p2, int paths, int pairs, int max_diff, int32_t *d_web, int32_t *d_best,
                     int32_t *d_web_right, int32_t *d_rejected, int16_t *d_sub, void *stream);

/* ---- banded SGM: semi-global aggregation within +-r of a prior map: PARITY UNPINNED -- *
 * New work (no reference counterpart; the tSGM idea of coarse-to-fine SGM pipelines).  The guided
 * re-search above with SGM's smoothness term: the last step of the half-resolution path becomes coarse SGM, upsample,
 * fine SGM in a band.  Arguments as sm_sgm_wta's (census_width, p1, p2, paths) and sm_census_wta_near's (d_prior,
 * radius r in 1..4; any int32 is a legal prior).  Definition:
 *   K(p)      = sm_census_wta_near's: { d : 0 <= d <= D - 1, |d - (prior(p) - 1)| <= r }, empty for prior(p) = 0;
 *   A(p, d)   = sm_census_wta's window cost, d in K(p) (all n x n taps with p's own d);
 *   L_r(p, d) = A(p, d) if q = p - r lies outside the image (paths never wrap) or K(q) is empty (a pixel without a
 *               band breaks the path, which restarts after it), else
 *               A(p, d) + min(L_r(q, d), L_r(q, d-1) + p1, L_r(q, d+1) + p1, m_q + p2) - m_q, m_q = min over K(q) of
 *               L_r(q, k), terms whose shift is not in K(q) dropped;  A <= L_r <= A + p2;
 *   S(p, d)   = sum over sm_sgm_wta's directions of L_r(p, d); best = min over K(p) of S, web = 1 + the LEAST d of
 *               K(p) reaching it; K(p) empty: web = best = sub = 0;
 *   sub       = with d = web - 1: d - 1 and d + 1 both in K(p): sm_sgm_wta's rule on S(d-1), S(d), S(d+1); otherwise
 *               (the winner at a band end, at 0 or at D - 1) 16 web;
 *   right reference: mirror(sgm_near(mirror(R), mirror(L), mirror(prior_right))); the check is sm_lr_check's, and
 *               sm_sgm_near_lr's d_sub is 0 where it rejected.
 * Where K(p) is all of 0 .. D - 1 at every pixel the maps are sm_sgm_wta's; with p1 = p2 = 0 web is
 * sm_census_wta_near's and best = paths * its best.  Windows up to 25 x 25 and up to 512 shifts (the census limits:
 * nothing here grows with D).  Refused before any device call, naming the function: a NULL plan or required pointer,
 * census_width, paths, penalties, radius, pairs, the window and shift limits, and an output that overlaps an image, a
 * prior or another output.  Workspace: the census workspace and the banded volumes of ONE pair, 96 * W * H bytes
 * whatever the radius (16 slots a pixel of u16 data term and int32 aggregate; 0.8 GB at 3840 x 2160); pairs go
 * through them in turn.  The full SGM volumes are neither needed nor touched.  Allocated by sm_plan_reserve_sgm_near
 * or by the first call that needs it, counted in sm_plan_workspace_bytes, freed by sm_plan_destroy.  STREAM CAPTURE:
 * once sm_plan_reserve_sgm_near has been called; before, the call is refused with SM_ERR_ARG, a message naming it,
 * and the capture valid.                                                                                           */
/* adds: banded SGM arg-min -> d_web; d_best (min over K of S) and d_sub (int16, 1/16 shift) may be NULL */
int sm_sgm_wta_near(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width,
                    int p1, int p2, int paths, int pairs, const int32_t *d_prior, int radius, int32_t *d_web,
                    int32_t *d_best, int16_t *d_sub, void *stream);
/* adds: the right-reference map around d_prior_right (a right-reference map), natural order */
int sm_sgm_wta_near_right(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width,
                          int p1, int p2, int paths, int pairs, const int32_t *d_prior_right, int radius,
                          int32_t *d_web_right, int32_t *d_best_right, void *stream);
/* adds: descriptors once, both passes, check; d_web = checked map; d_best / d_web_right / d_rejected / d_sub may be NULL */
int sm_sgm_near_lr(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width,
                   int p1, int p2, int paths, int pairs, const int32_t *d_prior, const int32_t *d_prior_right,
                   int radius, int max_diff, int32_t *d_web, int32_t *d_best, int32_t *d_web_right,
                   int32_t *d_rejected, int16_t *d_sub, void *stream);
/* adds: allocates the banded SGM workspace (and the census workspace) now; idempotent */
int sm_plan_reserve_sgm_near(sm_plan *plan);

/* ---- cross-based adaptive support over the census cost: PARITY UNPINNED ---- *
 * New work (no reference counterpart; the cross-based aggregation of Zhang et al. 2009, the aggregation
 * step of AD-Census).  Every other matcher sums its cost over a square box, so its disparity edges lie up to half a
 * window beside the object edges.  Here a pixel's support is a union of horizontal segments whose extents ("arms")
 * stop where the REFERENCE image changes: a support never straddles an intensity edge, and flat regions still get up
 * to 31 x 31 taps.  Arguments: census_width c in {3, 5, 7}, tau in 0 .. 255, arm L in 0 .. 15.  The plan gives W, H, D
 * and the border mode; ITS square_width PLAYS NO PART.  Definition (tests/cross_reference.py in numpy):
 *   arms a_dir(p) of a gray image I, dir in left, right, up, down: the largest l in 0 .. L such that every k = 1 .. l
 *     has p + k dir inside the image and |I(p + k dir) - I(p)| <= tau.  Arms never leave the image, in either border
 *     mode (the choice of SGM's paths).  Packed: uint16 = l | r << 4 | u << 8 | d << 12.
 *   support size N(x, y) = sum over y' = y - u(x, y) .. y + d(x, y) of l(x, y') + r(x, y') + 1; N <= 961.
 *   cost c_d(x, y) = sm_census_wta's: popcount(C_L(x, y) XOR C_R(x + d, y)); toroidal: x + d mod W; ghost: C_R = 0 for
 *     x + d >= W.  With the arms of the LEFT image:
 *     H_d(x, y) = sum over x' = x - l(x, y) .. x + r(x, y) of c_d(x', y),
 *     E_d(x, y) = sum over y' = y - u(x, y) .. y + d(x, y) of H_d(x, y');  E <= 48 * 961 = 46128.
 *   best = min_d E_d, web = 1 + the FIRST d reaching it.  The support does not depend on d, so this is the arg-min of
 *     the normalised costs E_d / N as well.
 *   subpixel: sm_cost_refine's SM_COST_SAD (equiangular) formula and edge rules on E(s-2), E(s-1), E(s).
 *   right reference: (best_right, web_right) = mirror(cross(mirror(R), mirror(L))), mirror(a)(x) = a(W-1-x): the arms
 *     of the RIGHT image.  The check is sm_lr_check's (section 10); in sm_cross_lr d_sub is 0 where it rejected.
 * arm = 0 gives sm_census_wta at a 1 x 1 window; in ghost mode tau = 255 gives sm_census_wta's web and best at the
 * window 2 L + 1 (L <= 12).  At most 512 shifts.  Arguments are checked before any device call; a refusal names the
 * function: a NULL plan or required pointer, max_diff < 0, census_width, tau, arm, pairs, the shift limit, result maps
 * that overlap each other, and an output that overlaps an input image.  Workspace: the census workspace
 * (sm_plan_reserve_census) and the packed arms of both images of max_pairs pairs, 4 * max_pairs * W * H bytes (33 MB
 * per 4K pair); nothing grows with D.  Allocated by sm_plan_reserve_cross or, without it, by the first call that
 * needs it (a hipMalloc, which synchronises the device), counted in sm_plan_workspace_bytes from then on, freed by
 * sm_plan_destroy.  All calls run in `stream` order and use nothing the pipelined lanes use.  STREAM CAPTURE: once
 * sm_plan_reserve_cross has been called; before, a matching call is refused with SM_ERR_ARG, a message naming it,
 * and the capture valid.                                                                                          */
/* adds: the packed arms of `images` consecutive gray images (images <= 2 * max_pairs) into d_arms, one uint16 per
 * pixel, and, d_support non-NULL, N as int32; needs no workspace                                                  */
int sm_cross_arms(sm_plan *plan, const uint8_t *d_gray, int tau, int arm, int images, uint16_t *d_arms,
                  int32_t *d_support, void *stream);
/* adds: the cross-based arg-min -> d_web (and, non-NULL, d_best = the costs E, d_sub int16 in 1/16 of a shift) */
int sm_cross_wta(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width, int tau,
                 int arm, int pairs, int32_t *d_web, int32_t *d_best, int16_t *d_sub, void *stream);
/* adds: the right-reference map (and, d_best_right non-NULL, its costs), natural order */
int sm_cross_wta_right(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width,
                       int tau, int arm, int pairs, int32_t *d_web_right, int32_t *d_best_right, void *stream);
/* adds: descriptors and arms once, left and right arg-min and the check (tolerance max_diff >= 0): d_web = checked
 * map (0 = rejected), d_best = the left costs, d_sub = the left subpixel map with 0 where rejected; d_best /
 * d_web_right / d_rejected (one int32 per pair) / d_sub may be NULL                                               */
int sm_cross_lr(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width, int tau,
                int arm, int pairs, int max_diff, int32_t *d_web, int32_t *d_best, int32_t *d_web_right,
                int32_t *d_rejected, int16_t *d_sub, void *stream);
/* adds: allocates the workspace of the calls above (and the census workspace) now; idempotent */
int sm_plan_reserve_cross(sm_plan *plan);

/* ---- match uniqueness: runner-up, ratio filter, confidence: PARITY UNPINNED -- *
 * New work (no reference counterpart; the uniquenessRatio test of OpenCV's StereoBM / SGBM).  Every
 * matcher returns how good its winner is, not by how much it won; the left-right check finds occlusions, not the
 * ambiguous matches on repeated structure, where both searches agree on the same wrong period.  The runner-up is the
 * best shift OUTSIDE the winner's +-1 neighbourhood (the neighbours of a true minimum are always nearly as good):
 *   runner-up of a volume V(p, d), d = 0 .. D - 1, against a web map (1 + shift, 0 = invalid): with s = web(p),
 *     E(p) = { d : |d - (s - 1)| >= 2 } for s in 1 .. D; for every other s (0 included; any int32 is legal) E(p) is
 *     all of 0 .. D - 1: a pixel without a winner has no neighbourhood.
 *     best2 = min over E(p) of V(p, d), web2 = 1 + the FIRST d of E(p) reaching it;
 *     E(p) empty (D <= 2, or D = 3 and the winner in the middle): web2 = 0, best2 = -1 ("no rival").
 *   sm_census_second: V = sm_census_wta's window cost A_d (same box, border rules, limits of 25 x 25 and 512 shifts);
 *     the map is the caller's: sm_census_wta's own, a checked map, a re-search map.  With an all-zero map the call
 *     returns sm_census_wta's web and best.
 *   sm_sgm_wta2: V = SGM's S.  d_web / d_best / d_sub exactly as from sm_sgm_wta, d_web2 / d_best2 the runner-up of S
 *     against that d_web; winner and runner-up in one call because S is never stored.  Left reference only.
 *   sm_uniqueness_filter, ratio in 0 .. 100: out(p) = web(p) iff web(p) != 0 and (best2(p) < 0 or
 *     best2(p) (100 - ratio) >= 100 best(p)), in 64-bit arithmetic; else 0.  OpenCV's rule, "no rival" kept.  ratio 0
 *     keeps every pixel whose best2 >= best.  d_rejected: NULL or one int32 per pair, the pixels that were not 0 and
 *     now are.  d_out may equal d_web; every other overlap is refused.  A sub map follows through sm_sub_mask.
 *   sm_confidence -> uint8 [pairs][H][W], the cases in this order: 0 where web = 0; 255 where best2 < 0; 0 where
 *     best2 <= best; else min(255, floor(255 (best2 - best) / best2)) in 64-bit arithmetic (best2 = 0 there means
 *     best < 0: 255).  So 255 means "no rival" only where best > 0: a winner of cost best <= 0 with any rival of
 *     positive cost gets 255 as well (the quotient is 1 or more).  Any int32 input is legal.
 * Arguments are checked before any device call; a refusal names the function: a NULL plan or required pointer,
 * census_width, the penalties and paths (sm_sgm_wta's messages), pairs, the window and shift limits, a ratio outside
 * 0 .. 100, an output that overlaps an input image or the input map, outputs that overlap one another.  Workspace:
 * nothing new.  sm_census_second uses the census workspace and sm_sgm_wta2 the SGM workspace, allocated and captured
 * as for sm_census_wta and sm_sgm_wta (STREAM CAPTURE once sm_plan_reserve_census / sm_plan_reserve_sgm has been
 * called; before, refused with SM_ERR_ARG, a message naming it, and the capture valid).  The filter and the
 * confidence map need no workspace and can always be captured.  All calls run in `stream` order and use nothing the
 * pipelined lanes use.                                                                                            */
/* adds: the runner-up of the census search against d_web -> d_web2 (and, d_best2 non-NULL, its window costs) */
int sm_census_second(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width, int pairs,
                     const int32_t *d_web, int32_t *d_web2, int32_t *d_best2, void *stream);
/* adds: sm_sgm_wta with the runner-up of S beside it; d_best, d_sub and d_best2 may be NULL */
int sm_sgm_wta2(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width, int p1, int p2,
                int paths, int pairs, int32_t *d_web, int32_t *d_best, int16_t *d_sub, int32_t *d_web2,
                int32_t *d_best2, void *stream);
/* adds: the ratio test -> d_out (in place allowed); d_rejected may be NULL */
int sm_uniqueness_filter(sm_plan *plan, const int32_t *d_web, const int32_t *d_best, const int32_t *d_best2, int ratio,
                         int pairs, int32_t *d_out, int32_t *d_rejected, void *stream);
/* adds: the confidence map, one byte per pixel */
int sm_confidence(sm_plan *plan, const int32_t *d_web, const int32_t *d_best, const int32_t *d_best2, int pairs,
                  uint8_t *d_conf, void *stream);

/* ---- disparity post-filters: PARITY UNPINNED ------------------------------ *
 * New work (no reference counterpart).  Two filters on the maps the calls above produce, between the
 * consistency check and step 3: cost -> check -> speckle / median -> hole filling.  Maps are [pairs][H][W] of type
 * SM_MAP_I32 (a web map) or SM_MAP_I16 (a sub map); a pixel is VALID iff its value != 0 (the check's convention).
 * Neighbourhoods never wrap, in either border mode: a tap outside the image does not exist.  Pairs are independent.
 *   median, window k in {3, 5}: out(p) = 0 where in(p) = 0 (holes are step 3's to fill); else, with v_0 <= ... <=
 *     v_(m-1) the valid values of the k x k window around p that lie in the image (m >= 1: the centre is one),
 *     out(p) = v_((m-1)/2), integer division: the lower median.  Negative values are valid and order as signed
 *     integers.  d_in and d_out must not overlap.
 *   speckle removal, max_size >= 0, max_diff >= 0: the valid pixels form a graph in which two 4-neighbours a, b are
 *     joined iff |in(a) - in(b)| <= max_diff; out(p) = in(p) if p is valid and its connected component has more
 *     than max_size pixels, else 0.  d_removed: NULL or one int32 per pair, the number of valid pixels set to 0.
 *     (OpenCV's filterSpeckles with newVal = 0 and 0 as "already invalid".)  The result does not depend on the
 *     order in which the graph is explored.  d_out may equal d_in (the labels are complete before anything is
 *     written); any other overlap is refused.
 *   sub mask: d_sub = 0 where d_web = 0, so that a sub map follows a web map the speckle filter has thinned.
 * Arguments are checked before any device call; a refusal names the function.  All calls run in `stream` order and
 * use nothing the pipelined lanes use.  sm_median_filter and sm_sub_mask need no workspace and can always be
 * captured.  sm_speckle_filter's workspace is one int32 label and one int32 component size per pixel,
 * 8 * max_pairs * W * H bytes; allocated by sm_plan_reserve_filter or, without it, by the first sm_speckle_filter (a
 * hipMalloc, which synchronises the device), counted in sm_plan_workspace_bytes from then on, freed by
 * sm_plan_destroy; a plan that never filters allocates nothing.  STREAM CAPTURE: sm_speckle_filter once
 * sm_plan_reserve_filter has been called; before, it is refused with SM_ERR_ARG, a message naming it, and the
 * capture valid.                                                                                              */
#define SM_MAP_I32 0
#define SM_MAP_I16 1
/* adds: the validity-aware k x k median of d_in -> d_out (same type) */
int sm_median_filter(sm_plan *plan, const void *d_in, int map_type, int k, int pairs, void *d_out, void *stream);
/* adds: speckle removal of d_in -> d_out (same type; in place allowed) */
int sm_speckle_filter(sm_plan *plan, const void *d_in, int map_type, int max_size, int max_diff, int pairs,
                      void *d_out, int32_t *d_removed, void *stream);
/* adds: d_sub = 0 where d_web = 0 */
int sm_sub_mask(sm_plan *plan, const int32_t *d_web, int16_t *d_sub, int pairs, void *stream);
/* adds: allocates the speckle filter's workspace now; idempotent */
int sm_plan_reserve_filter(sm_plan *plan);

/* ---- guided weighted median: PARITY UNPINNED ------------------------------ *
 * New work (no reference counterpart; Ma et al., ICCV 2013): the one post-filter that looks at the
 * image.  Every matcher aggregates over a square box, so its disparity edges lie up to half a window beside the
 * image's; a median whose taps are weighted by how alike the GUIDE image is at the tap and at the centre moves them
 * back.  cost -> check -> speckle -> weighted median (optionally filling) -> interpolate -> step 3 -> reproject.
 * Maps, validity and borders follow the post-filters: [pairs][H][W] of SM_MAP_I32 or SM_MAP_I16; a pixel is valid iff
 * its value != 0; a tap outside the image does not exist, in either border mode; pairs are independent.
 *   guide g: u8 [pairs][H][W], typically the rectified left image.  radius r: 1 .. 7.  weights: 256 uint16_t ON THE
 *     HOST (as q[16] of sm_reproject is), weights[0] >= 1.
 *   For pixel p the taps are the pixels q of the (2r+1) x (2r+1) window around p that lie in the image and have
 *     in(q) != 0; tap q has the weight w_q = weights[|g(p) - g(q)|]; T = the sum of the w_q (at most 225 * 65535: it
 *     fits 32 bits).
 *   wmed(p) = the smallest tap value v, in signed order, with 2 * sum{w_q : in(q) <= v} >= T: the lower weighted
 *     median.  With all weights equal it is sm_median_filter's v_((m-1)/2).
 *   flags = 0: out(p) = 0 where in(p) = 0; otherwise out(p) = wmed(p) (T >= 1: the centre is a tap).
 *   flags = SM_WMED_FILL: where in(p) = 0, out(p) = wmed(p) if T >= fill_min_weight, otherwise 0.  fill_min_weight >=
 *     1; it is ignored without the flag.  Taps are always read from the input: a filled pixel is no source.
 *   d_filled: NULL or one int32 per pair, the number of pixels that were 0 and are no longer (0 without the flag).
 *   d_in and d_out must not overlap: any overlap is refused (so is an output that overlaps the guide, and a d_filled
 *     that overlaps a map).
 * Arguments are checked before any device call; a refusal names the function.  The call runs in `stream` order and
 * uses nothing the pipelined lanes use.  It needs no workspace and can always be captured; the weight table travels
 * in the kernel's arguments, so in a captured graph its values are those at capture time.  Images smaller than the
 * window are fine.                                                                                              */
#define SM_WMED_FILL 1
/* adds: the guided weighted median of d_in -> d_out (same type) */
int sm_weighted_median(sm_plan *plan, const void *d_in, int map_type, const uint8_t *d_guide, int radius,
                       const uint16_t weights[256], int flags, int fill_min_weight, int pairs,
                       void *d_out, int32_t *d_filled, void *stream);

/* ---- edge-aware smoother: PARITY UNPINNED --------------------------------- *
 * New work (no reference counterpart): the global, edge-aware, confidence-weighted filter beside the
 * local ones above.  The fast global smoother (Min et al., TIP 2014) used the way OpenCV's DisparityWLSFilter uses it:
 * a weighted-least-squares problem whose smoothness weights come from the guide image is solved for confidence x
 * disparity and for confidence, and the first result is divided by the second.  The result is a dense subpixel map,
 * smooth inside surfaces, broken at the image's edges, deaf to low-confidence outliers, with holes filled from their
 * own surface at any distance.  matcher (+ runner-up) -> sm_confidence -> check -> speckle -> smoother -> reproject.
 * tests/wls_reference.py is the executable form of this definition; the library equals it bit for bit.
 *   Maps are [pairs][H][W]; map_type and out_type are each SM_MAP_I32 (web) or SM_MAP_I16 (sub), in any combination.  A
 *     pixel is valid iff its value v != 0; its value in 1/16 steps is the exact double u = 16 v (int32) or u = v
 *     (int16); any value is legal.  d_guide: u8 [pairs][H][W].  d_conf: u8 [pairs][H][W], or NULL for a map of 255s.
 *   weights: 256 uint16_t ON THE HOST, as for sm_weighted_median; any table is legal, zeros included.  It is passed to
 *     the kernels by value: a captured graph holds the table of capture time.  lambda: finite, 0 <= lambda <= 2^20; it
 *     multiplies the table's entries as they are (with guide_weights(sigma, peak) pass lambda / peak).  iterations T:
 *     1 .. 8.
 *   Start: c(p) = (double)conf(p) where in(p) != 0, else 0; N = c u, M = c (exact integers).
 *   For t = 0 .. T-1, with lambda_t = ((1.5 lambda) 4^(T-1-t)) / (4^T - 1.0) computed on the host in double in that
 *     order: every row is solved, then every column, for N and M alike.
 *   One line f_0 .. f_(n-1): links l_i = lambda_t * (double)weights[|g_i - g_(i+1)|] for i = 0 .. n-2, l_(-1) = l_(n-1)
 *     = 0; a_i = -l_(i-1), k_i = -l_i, b_i = (1.0 + l_(i-1)) + l_i.
 *     Forward, i = 0 .. n-1: den_i = b_i - cp_(i-1) a_i; inv_i = 1.0 / den_i; cp_i = k_i inv_i; f'_i = (f_i - f'_(i-1)
 *     a_i) inv_i (the terms with index -1 are absent at i = 0: den_0 = b_0, f'_0 = f_0 inv_0).
 *     Backward: U_(n-1) = f'_(n-1); U_i = f'_i - cp_i U_(i+1).
 *     Every operation is an IEEE double operation rounded on its own, in the order written.  den_i >= 1 always; no
 *     intermediate of M is negative.  A line of one element is returned unchanged.
 *   r(p) = N(p) / M(p) where M(p) > 0, else r = 0.0.  An int16 output receives rint(r) (ties to even) saturated to
 *     int16; an int32 output rint(r / 16), saturated.  A result of 0 reads as invalid, as everywhere (maps of the
 *     library's matchers have u >= 16 at valid pixels, and so have their averages).
 *   flags = SM_WLS_NO_FILL: the output and d_raw are 0 where in(p) = 0.
 *   d_raw: NULL or [pairs][H][W] doubles that receive r.  d_filled: NULL or one int32 per pair, the number of pixels
 *     that were 0 and are no longer.
 * Refused before any device call, naming the function: a NULL plan, map, guide, weights or output; an unknown map_type
 * or out_type; a lambda that is not finite or outside the range; iterations outside 1 .. 8; unknown flag bits; pairs
 * outside 1 .. max_pairs; any overlap among the buffers, except that d_out == d_in is allowed when the two types are
 * equal (a pixel's input is read before its output is written).
 * Workspace: three double planes per pair slot (N, M, cp), 24 * max_pairs * W * H bytes (199 MB for one 4K pair),
 * allocated by sm_plan_reserve_wls or by the first call and counted in sm_plan_workspace_bytes from then on.  Inside
 * a stream capture before the reservation the call is refused with SM_ERR_ARG (the capture stays valid); after it the
 * call can be captured: no copy, no synchronisation.  The call runs in `stream` order and uses nothing the pipelined
 * lanes use.                                                                                                       */
#define SM_WLS_NO_FILL 1
/* adds: the smoothed map of d_in -> d_out (of out_type) */
int sm_wls_filter(sm_plan *plan, const void *d_in, int map_type, const uint8_t *d_conf, const uint8_t *d_guide,
                  const uint16_t weights[256], double lambda, int iterations, int flags, int pairs,
                  void *d_out, int out_type, double *d_raw, int32_t *d_filled, void *stream);
/* adds: allocates the smoother's workspace now; idempotent */
int sm_plan_reserve_wls(sm_plan *plan);

/* ---- half-resolution path: PARITY UNPINNED -------------------------------- *
 * New work (no reference counterpart): SGM on a large pair costs a volume of W x H x shifts.  Matching
 * at half the size with half the shifts is an eighth of it; the coarse map is then brought back to the fine size
 * along the edges of the fine image (joint upsampling: Kopf et al., SIGGRAPH 2007, with the weighted median of the
 * section above in place of the mean).  reduce both sides -> any matcher on a plan of the coarse size with half the
 * shifts -> check / filters at the coarse size -> upsample -> filters at the fine size -> interpolate -> reproject.
 * Both calls take the plan of the FINE size W x H.  The coarse size is fixed by it: cw = (W + 1) >> 1, ch = (H + 1) >> 1;
 * the coarse matcher runs on a second plan of cw x ch that the caller makes.  Nothing wraps, in either border mode;
 * pairs are independent.
 *   sm_reduce_half: d_src u8 [images][H][W] -> d_dst u8 [images][ch][cw]; images is 1 .. 2 * max_pairs, so both sides
 *     of a batch go in one call.  Exact integers, with cx(u) = min(max(u, 0), W - 1) and cy likewise (replicate):
 *       SM_REDUCE_BOX:      dst(X, Y) = (sum{i, j in 0..1} src(cx(2X + i), cy(2Y + j)) + 2) >> 2
 *       SM_REDUCE_BINOMIAL: k = [1, 3, 3, 1]; dst(X, Y) = (sum{i, j in 0..3} k_i k_j src(cx(2X - 1 + i), cy(2Y - 1 + j)) + 32) >> 6
 *     Both are centred on the 2 x 2 block: coarse pixel (X, Y) stands for the fine pixels (2X .. 2X + 1, 2Y .. 2Y + 1),
 *     and a fine shift d is a coarse shift d / 2.
 *   sm_upsample_double: d_in [pairs][ch][cw] -> d_out [pairs][H][W], both SM_MAP_I32 or both SM_MAP_I16; a pixel is
 *     valid iff its value != 0.  d_guide: u8 [pairs][H][W]; d_guide_coarse: u8 [pairs][ch][cw], typically
 *     sm_reduce_half of d_guide.  weights: 256 uint16_t ON THE HOST, every one >= 1 (no tap is the centre here, so a 0
 *     anywhere could leave a valid pixel without weight: it is refused).
 *     Values change scale, web = 1 + shift and sub = 16 web + fraction:
 *       SM_MAP_I32: v(c) = 2 in(c) - 1, computed in 64 bits and clamped to int32
 *       SM_MAP_I16: v(c) = 2 in(c) - 16, clamped to int16.  An input of 8 becomes 0, which reads as invalid; the
 *         sub values the library writes are >= 16.
 *     For the fine pixel p = (x, y): home (X, Y) = (x >> 1, y >> 1), px = x & 1, py = y & 1.  The taps are the coarse
 *     pixels c = (X + i, Y + j), i, j in {-1, 0, 1}, that lie in the coarse image and have in(c) != 0.  Tap c has the
 *     weight w_c = weights[|g(p) - gc(c)|] * s(i, px) * s(j, py), where s(i, 0) = 2, 4, 1 and s(i, 1) = 1, 4, 2 for
 *     i = -1, 0, 1 (4, 2, 1 by the distance |4i + 1 - 2px| = 1, 3, 5 of the tap's centre, in quarter coarse pixels).
 *     T = the sum of the w_c (at most 49 * 65535).  wmed(p) = the smallest v(c), in signed order, with
 *     2 * sum{w_c' : v(c') <= v(c)} >= T: the lower weighted median.
 *       flags = 0:          out(p) = 0 where in(home) = 0; otherwise wmed(p)
 *       flags = SM_UP_FILL: where in(home) = 0, out(p) = wmed(p) if p has a tap, otherwise 0
 *     Taps are always read from the input.
 *   An output that overlaps an input or a guide is refused.
 * Arguments are checked before any device call; a refusal names the function.  The calls run in `stream` order and
 * use nothing the pipelined lanes use.  They need no workspace and can always be captured; the weight table travels
 * in the kernel's arguments, so in a captured graph its values are those at capture time.                        */
#define SM_REDUCE_BOX 0
#define SM_REDUCE_BINOMIAL 1
#define SM_UP_FILL 1
/* adds: images of the plan's size reduced by two in each direction */
int sm_reduce_half(sm_plan *plan, const uint8_t *d_src, int filter, int images, uint8_t *d_dst, void *stream);
/* adds: a map of the half size brought to the plan's size along the edges of d_guide */
int sm_upsample_double(sm_plan *plan, const void *d_in, int map_type, const uint8_t *d_guide,
                       const uint8_t *d_guide_coarse, const uint16_t weights[256], int flags, int pairs,
                       void *d_out, void *stream);

/* ---- occlusion-aware interpolation: PARITY UNPINNED ----------------------- *
 * New work (no reference counterpart): Hirschmueller's discontinuity-preserving interpolation (PAMI
 * 2008) of the 0s the check and the speckle filter leave: cost -> check -> speckle / median -> interpolate -> step 3.
 * Maps and validity as for the post-filters; nothing wraps in the interpolation, in either border mode; pairs are
 * independent.  web = 1 + shift: left pixel (x, y) with web = s matched right pixel u = x + s - 1, and
 * web_right(u, y) = s' means right pixel u matched left pixel u - (s' - 1); a smaller value is farther away.
 *   classification, from the right-reference map of the check, with the plan's W, H, D and border mode:
 *     class(x, y) = 0 where web(x, y) != 0; else 2 (MISMATCHED) if there is a d in 0 .. D-1 with u = x + d inside the
 *     row (toroidal: u mod W, always inside; ghost: u < W) and web_right(u, y) = d + 1; else 1 (OCCLUDED).  Values
 *     of web_right outside 1 .. D match no d; no read leaves the row.
 *   interpolation: out(p) = in(p) where in(p) != 0.  Else walk from p in each of the eight directions (+-1, 0),
 *     (0, +-1), (+-1, +-1) to the first valid pixel of d_in or the image edge; the values found, c_0 <= ... <= c_(m-1)
 *     in signed order, 0 <= m <= 8, are the candidates (always read from the input: a filled pixel is no source).
 *     m = 0: out(p) = 0.  class(p) = 1: out(p) = c_(min(1, m-1)), the second lowest: background, robust to one
 *     outlier.  Otherwise (class 0 or 2, or d_class NULL): out(p) = c_((m-1)/2), the lower median.  d_class is read
 *     where in(p) = 0 only.  d_filled: NULL or one int32 per pair, the pixels that were 0 and are not any more.
 *     d_in and d_out must not overlap.
 * Arguments are checked before any device call; a refusal names the function.  All calls run in `stream` order and
 * use nothing the pipelined lanes use.  sm_occlusion_classify needs no workspace and can always be captured.
 * sm_interpolate's workspace is, with S = ceil(H / 64) and C = ceil(W / 64),
 *     4 * max_pairs * (6 * W * H + 6 * S * (W + H - 1) + 2 * H * C) bytes
 * (six directional maps, the carries of every line segment and of every row chunk); allocated by
 * sm_plan_reserve_interp or, without it, by the first sm_interpolate (a hipMalloc, which synchronises the device;
 * SM_ERR_NOMEM on failure), counted in sm_plan_workspace_bytes from then on, freed by sm_plan_destroy; a plan that
 * never interpolates allocates nothing.  STREAM CAPTURE: sm_interpolate once sm_plan_reserve_interp has been called;
 * before, it is refused with SM_ERR_ARG, a message naming it, and the capture valid.                              */
#define SM_CLASS_VALID 0
#define SM_CLASS_OCCLUDED 1
#define SM_CLASS_MISMATCHED 2
/* adds: 0 valid / 1 occluded / 2 mismatched for every pixel of the checked map d_web */
int sm_occlusion_classify(sm_plan *plan, const int32_t *d_web, const int32_t *d_web_right, int pairs,
                          uint8_t *d_class, void *stream);
/* adds: discontinuity-preserving fill of the 0s of d_in -> d_out (same type); d_class may be NULL */
int sm_interpolate(sm_plan *plan, const void *d_in, int map_type, const uint8_t *d_class, int pairs, void *d_out,
                   int32_t *d_filled, void *stream);
/* adds: allocates sm_interpolate's workspace now; idempotent */
int sm_plan_reserve_interp(sm_plan *plan);

/* ---- rectification: PARITY UNPINNED -------------------------------------- *
 * New work (no reference counterpart): the stage in FRONT of the matchers.  Every matcher searches along
 * the image row, which is right on a rectified pair only; these calls make one from raw camera images and a
 * calibration: map build (once) -> rectify (every frame) -> any matcher -> valid mask -> filters / interpolation.
 * The rectified images are the plan's W x H; the raw images are src_w x src_h, given per call, tightly packed u8.
 *   map: tells every destination pixel where to read in the source, in fixed point with SM_RMAP_FRAC_BITS fraction
 *     bits (1/32 pixel).  SM_RMAP_ABS32: [H][W][2] int32 (mx, my), the source position times 32; any int32 value is
 *     legal.  SM_RMAP_REL16: [H][W][2] int16 (dx, dy) with mx = 32 x + dx, my = 32 y + dy: half the bytes,
 *     displacements of up to +-1023 pixels.  A map pointer is aligned to its element (4 or 2 bytes).
 *   remap, per destination pixel, exact integer arithmetic: x0 = mx >> 5 (arithmetic: floor), fx = mx & 31, likewise
 *     y0, fy.  tap(i, j) = src(x0 + i, y0 + j) if 0 <= x0 + i < src_w and 0 <= y0 + j < src_h, else `border`
 *     (0 .. 255).  Nothing wraps, in either border mode of the plan.
 *     SM_INTERP_BILINEAR: w00 = (32-fx)(32-fy), w10 = fx (32-fy), w01 = (32-fx) fy, w11 = fx fy (sum 1024);
 *       out = (sum of w_ij tap(i, j) + 512) >> 10.
 *     SM_INTERP_NEAREST: out = the one tap at (floor((mx + 16) / 32), floor((my + 16) / 32)), same border rule.
 *     validity (optional, one u8 image per side): 1 iff every tap whose weight is not 0 lies inside the source
 *     (nearest: the one tap), else 0.  The identity map is valid everywhere.
 *   one sm_rectify call does both sides of `pairs` pairs: raw left / right [pairs][src_h][src_w], one map per SIDE
 *     shared by all pairs (the two map pointers may be equal), rectified left / right [pairs][H][W], validity
 *     [pairs][H][W] per side or NULL.  Outputs must not overlap inputs or one another.
 *   map build, from one side's calibration (sm_rectify_calib: camera matrix fx, fy, cx, cy; Brown-Conrady distortion
 *     k1, k2, p1, p2, k3 in OpenCV's order; rectifying rotation R; new projection new_fx, new_fy, new_cx, new_cy),
 *     IEEE double, every operation rounded on its own, in this order, for destination pixel (x, y):
 *       xn = (x - new_cx) / new_fx, yn = (y - new_cy) / new_fy;
 *       X = R00 xn + R10 yn + R20, Y = R01 xn + R11 yn + R21, Z = R02 xn + R12 yn + R22 (R transposed; left to right);
 *       a = X / Z, b = Y / Z; r2 = a a + b b; rad = 1 + r2 (k1 + r2 (k2 + r2 k3));
 *       ad = a rad + (((2 p1) a) b + p2 (r2 + (2 a) a)), bd = b rad + (p1 (r2 + (2 b) b) + ((2 p2) a) b);
 *       u = fx ad + cx, v = fy bd + cy; mx = floor(u 32 + 0.5), my = floor(v 32 + 0.5), saturated to int32;
 *       a non-finite u or v (Z = 0) gives mx = my = INT32_MIN (far outside: border).
 *     SM_RMAP_REL16 is refused with SM_ERR_ARG, and a message naming SM_RMAP_ABS32 as the remedy, if a displacement
 *     does not fit int16; d_map then holds no map.  The builder reads that flag back: it SYNCHRONISES `stream`,
 *     allocates and frees four bytes, and CANNOT BE CAPTURED (refused with SM_ERR_ARG, the capture left valid).
 *   valid mask: d_map = 0 where d_valid = 0, else unchanged, in place, on an SM_MAP_I32 web map or an SM_MAP_I16 sub
 *     map [pairs][H][W]: the wedges a rectification leaves empty become 0s, which the check, the filters,
 *     sm_interpolate and step 3 treat as "invalid".
 * Arguments are checked before any device call; a refusal names the function.  All calls run in `stream` order and
 * use nothing the pipelined lanes use.  None needs workspace: a plan that rectifies reports the same
 * sm_plan_workspace_bytes.  STREAM CAPTURE: sm_rectify and sm_valid_mask always; sm_rectify_map_build never.   */
#define SM_RMAP_FRAC_BITS 5
#define SM_RMAP_ABS32 0
#define SM_RMAP_REL16 1
#define SM_INTERP_BILINEAR 0
#define SM_INTERP_NEAREST 1
typedef struct sm_rectify_calib {
    int struct_size;            /* sizeof(sm_rectify_calib) as the caller compiled it; a shorter struct is refused (every
                                 * field is needed), of a longer (newer) one the fields this library knows are taken */
    int reserved;               /* 0 */
    double fx, fy, cx, cy;      /* camera matrix of the raw image */
    double k1, k2, p1, p2, k3;  /* distortion */
    double R[3][3];             /* rectifying rotation, row-major (OpenCV's R1 / R2) */
    double new_fx, new_fy, new_cx, new_cy;   /* projection of the rectified image (OpenCV's P1 / P2, left 3 x 3) */
} sm_rectify_calib;
/* adds: rectified left / right images (and validity) of raw pairs through one map per side */
int sm_rectify(sm_plan *plan, const uint8_t *d_raw_left, const uint8_t *d_raw_right, int src_w, int src_h,
               const void *d_map_left, const void *d_map_right, int map_format, int interp, int border, int pairs,
               uint8_t *d_left, uint8_t *d_right, uint8_t *d_valid_left, uint8_t *d_valid_right, void *stream);
/* adds: the W x H map of one side's calibration, in either format, on the device; synchronises, not capturable */
int sm_rectify_map_build(sm_plan *plan, const sm_rectify_calib *calib, int map_format, void *d_map, void *stream);
/* adds: d_map = 0 where d_valid = 0, in place */
int sm_valid_mask(sm_plan *plan, void *d_map, int map_type, const uint8_t *d_valid, int pairs, void *stream);

/* ---- reprojection: PARITY UNPINNED ---------------------------------------- *
 * New work (no reference counterpart): the stage BEHIND the matchers, from a disparity map in shifts to
 * depth in metres and 3-D points: map build -> rectify -> any matcher -> check -> filters -> interpolate -> reproject.
 *   map: [pairs][H][W] of type SM_MAP_I32 (a web map) or SM_MAP_I16 (a sub map, 1/16 shift), the plan's W and H; a
 *     pixel is VALID iff its value v != 0; any int32 / int16 value is legal.  Its disparity is the exact double
 *     d = v - 1 (SM_MAP_I32) or d = v / 16 - 1 (SM_MAP_I16).
 *   Q: 16 doubles, row-major 4 x 4, read from a HOST array at call time and passed to the kernels by value (no
 *     upload, no synchronisation; the array may be reused at once).  Every entry must be finite.
 *     [X Y Z Wh]' = Q [x y d 1]' with x, y the pixel's integer coordinates.
 *   arithmetic, IEEE double, every operation rounded on its own (nothing fused, nothing reassociated), for each row i:
 *       r_i = ((Qi0 x + Qi1 y) + Qi2 d) + Qi3          (left to right; r_3 = Wh)
 *       Xf = (float)(r_0 / Wh), Yf = (float)(r_1 / Wh), Zf = (float)(r_2 / Wh)
 *     division and double -> float round to nearest even.  (A result that is subnormal in float may be flushed to
 *     zero on the device.)
 *   a pixel is KEPT iff it is valid, Xf, Yf and Zf are all finite (Wh = 0 and float overflow drop it), and
 *     z_min <= Zf <= z_max (float; -inf / +inf: no gate; a NaN bound or z_min > z_max is refused).
 *   sm_reproject (dense): d_depth [pairs][H][W] receives Zf, d_xyz [pairs][H][W][3] the interleaved Xf, Yf, Zf; a pixel
 *     that is not kept receives the float `missing` (0, +inf, a NaN, ...) in every channel.  Either may be NULL, not
 *     both.  d_count: NULL or one int32 per pair, the number of kept pixels.  Outputs must not overlap the map or one
 *     another.
 *   sm_point_cloud (compacted): the kept pixels of each pair in RASTER ORDER (y outer, x inner); the k-th of pair p
 *     writes the record d_points[p][k] = (Xf, Yf, Zf, I) of a [pairs][capacity][4] float array, I = (float)d_gray[p][y][x]
 *     (d_gray: u8 [pairs][H][W], typically the rectified left image) or 0.0f where d_gray is NULL, and, where d_index
 *     is not NULL, d_index[p][k] = y W + x ([pairs][capacity] int32).  d_count[p] (required) ALWAYS receives the total
 *     number of kept pixels of pair p, also beyond `capacity`; records and indices with k >= capacity are not written,
 *     slots count <= k < capacity are left untouched.  capacity >= 0; d_points may be NULL only with capacity = 0 (a
 *     count-only call).  The order makes the result deterministic: two runs give identical bytes.
 *   sm_reproject_q (host only; no plan, no device): the Q of a rectified rig.  This library's maps say that pixel x of
 *     the first image matches pixel x + d of the second; with X_second = X_first + t, t = baseline,
 *     f = first->new_fx, c1 = first->new_cx / new_cy, c2x = second->new_cx, each entry one or two rounded operations:
 *       r = f / first->new_fy;
 *       Q = [ 1  0  0    -c1x               ]      so that  Z = f t / (d - (c2x - c1x)),  X = (x - c1x) Z / f,
 *           [ 0  r  0    -(c1y r)           ]               Y = (y - c1y) Z / new_fy,
 *           [ 0  0  0     f                 ]      in the baseline's unit.
 *           [ 0  0  1/t  -((c2x - c1x) / t) ]
 *     Refused: a NULL pointer, a struct_size too short, a baseline that is 0 or not finite, new_fx / new_fy of the
 *     first calibration not positive and finite.
 * Pointers are aligned to their elements.  Arguments are checked before any device call; a refusal names the
 * function.  All calls run in `stream` order and use nothing the pipelined lanes use.  sm_reproject needs no workspace
 * and can always be captured.  sm_point_cloud's workspace is one int32 per tile of 1024 pixels and pair slot,
 *     4 * max_pairs * ceil(W * H / 1024) bytes
 * (tile counts, turned into offsets in place); allocated by sm_plan_reserve_cloud or, without it, by the first
 * sm_point_cloud (a hipMalloc, which synchronises the device; SM_ERR_NOMEM on failure), counted in
 * sm_plan_workspace_bytes from then on, freed by sm_plan_destroy; a plan that never builds a cloud allocates nothing.
 * STREAM CAPTURE: sm_point_cloud once sm_plan_reserve_cloud has been called; before, it is refused with SM_ERR_ARG, a
 * message naming it, and the capture valid.  Images of up to 2^30 pixels.                                            */
/* adds: depth and / or XYZ of every pixel of a disparity map; d_depth or d_xyz and d_count may be NULL */
int sm_reproject(sm_plan *plan, const void *d_map, int map_type, const double q[16], float z_min, float z_max,
                 float missing, int pairs, float *d_depth, float *d_xyz, int32_t *d_count, void *stream);
/* adds: the kept pixels of a disparity map as (X, Y, Z, I) records in raster order; d_gray and d_index may be NULL */
int sm_point_cloud(sm_plan *plan, const void *d_map, int map_type, const double q[16], float z_min, float z_max,
                   const uint8_t *d_gray, int pairs, int capacity, float *d_points, int32_t *d_index, int32_t *d_count,
                   void *stream);
/* adds: allocates sm_point_cloud's workspace now; idempotent */
int sm_plan_reserve_cloud(sm_plan *plan);
/* adds: the reprojection matrix of a rectified pair of calibrations and a baseline; host only */
int sm_reproject_q(const sm_rectify_calib *first, const sm_rectify_calib *second, double baseline, double q[16]);

/* ---- step 3 -------------------------------------------------------------- *
 * fill_web_holes (src/stereo.cu:235-256): every pixel that is 0 becomes the
 * truncated mean of its four flat-index neighbours.  The reference's pointer
 * SWAP is a no-op (its macro's local `tmp` shadows the buffer), so each of its
 * `times` sweeps reads the unfilled map: times >= 1 is one sweep, times <= 0
 * none.  d_tmp is workspace; *result_in_tmp tells which buffer holds the
 * returned image (d_web: it is 0).  Both buffers are W*H int32 per pair.    */
int sm_fill_web_holes(sm_plan *plan, int32_t *d_web, int32_t *d_tmp, int times,
                      int pairs, int *result_in_tmp, void *stream);

/* array_min_gpu / array_max_gpu (src/util.cu:15-45) of each pair's image;
 * d_minmax receives 2 int32 per pair: {min, max}                            */
int sm_min_max(sm_plan *plan, const int32_t *d_image, int pairs,
               int32_t *d_minmax, void *stream);

/* draw_contour_map_kernel (src/stereo.cu:261-285) with the min/max taken
 * from d_minmax (as written by sm_min_max).  A zero interval (the reference
 * divides by it) is recorded in the plan and reported by sm_plan_status.    */
int sm_draw_contour_map(sm_plan *plan, const int32_t *d_web,
                        const int32_t *d_minmax, int num_lines, int pairs,
                        uint8_t *d_out, void *stream);

/* The whole of step 3 (fill_web_holes, image min/max, draw_contour_map:
 * src/stereo.cu:325-333) with ONE synchronisation instead of one per stage.  Same
 * results as sm_fill_web_holes + sm_min_max + sm_draw_contour_map + sm_plan_status:
 * d_out receives the contour image of the hole-filled map, d_minmax its {min, max},
 * *result_in_tmp tells which of d_web / d_tmp holds the hole-filled map.  The stages
 * are queued speculating that the map has no zero pixel (hole filling then is the
 * identity; a web from sm_match_wta never has one) and one pass over the map verifies
 * it; a map that does have holes takes the staged route.  Returns SM_ERR_ZERO_DIV
 * for a zero contour interval.  Synchronises the stream.                            */
int sm_step3(sm_plan *plan, int32_t *d_web, int32_t *d_tmp, int times, int num_lines,
             int pairs, int32_t *d_minmax, uint8_t *d_out, int *result_in_tmp, void *stream);

/* synchronises the stream and returns SM_ERR_ZERO_DIV if a contour launch
 * since the last call met a zero interval, else SM_OK                       */
int sm_plan_status(sm_plan *plan, void *stream);

#ifdef __cplusplus
}
#endif
#endif
