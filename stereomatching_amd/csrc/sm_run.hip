// sm_run.hip -- step 2's entry points and the scheduler (include/stereo_hip.h): sm_match_wta*
// (the launch itself is sm_match.hip's) with the optional kernel timing, sm_run* on `stream` or on the plan's two
// lanes (run_on_lanes), the fences other units put between their own launches and the lanes, and the debug tap.
// The lane state (ev_free_set, unfenced, cap_live, cap_id, ev_fork, out_lo, out_hi) is written here and nowhere else.

#include "sm_internal.h"

#include <stdlib.h>

// int32 web -> uint16 / uint8 (the kernels that have no narrow store path of their own)
__global__ __launch_bounds__(256) void k_narrow_web(const i32 *__restrict__ src, void *__restrict__ dst,
                                                   long long n, int bytes)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    if (bytes == 1) ((u8 *)dst)[p] = (u8)src[p];
    else ((unsigned short *)dst)[p] = (unsigned short)src[p];
}

// ---------------------------------------------------------------------------
// debug tap: the per-shift planes of the reference's debug build
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_debug_planes(const u32 *__restrict__ ext, int pair,
                                                      int shift, u8 *__restrict__ match,
                                                      i32 *__restrict__ score_all,
                                                      i32 *__restrict__ scores, const MatchGeom g,
                                                      int ghost)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= g.w) return;
    const u32 *ext_l = ext + (size_t)pair * 2 * g.ext_image_words;
    const u32 *ext_r = ext_l + g.ext_image_words;
    auto bit = [&](const u32 *im, int xx, int yy) -> u32 {
        const int b = xx + g.pad_l;
        return (im[(size_t)(yy + g.half) * g.ext_words + (b >> 5)] >> (b & 31)) & 1u;
    };
    int xa = x - g.half, xb = x + g.half, ya = y - g.half, yb = y + g.half;
    if (ghost) {
        xa = max(xa, 0); xb = min(xb, g.w - 1);
        ya = max(ya, 0); yb = min(yb, g.h - 1);
    }
    i32 sum = 0;
    for (int yy = ya; yy <= yb; yy++)
        for (int xx = xa; xx <= xb; xx++)
            sum += bit(ext_l, xx, yy) == bit(ext_r, xx + shift, yy);
    const u32 m = bit(ext_l, x, y) == bit(ext_r, x + shift, y);
    const size_t o = (size_t)y * g.w + x;
    if (match) match[o] = (u8)m;
    if (score_all) score_all[o] = sum;
    if (scores) scores[o] = m ? sum : 0;
}

void sm_run_resolve_kernels(void)
{
    hipFuncAttributes fa;
    (void)hipFuncGetAttributes(&fa, (const void *)k_debug_planes);
}

// ---------------------------------------------------------------------------
// the match entry point, and the timing of its launches
// ---------------------------------------------------------------------------

MatchLaunch sm_match_launch_args(const sm_plan *plan, const void *d_web, const void *d_best, int web_bytes)
{
    MatchLaunch l;
    l.g = plan->g;
    if (((uintptr_t)d_web & (4 * web_bytes - 1)) != 0 || ((uintptr_t)d_best & 15) != 0) l.g.vec_ok = 0;
    l.g.web_bytes = web_bytes;
    l.ev_begin = l.ev_end = nullptr;
    return l;
}

extern "C" int sm_match_wta(sm_plan *plan, int pairs, int32_t *d_web, int32_t *d_best,
                            void *stream)
{
    return sm_match_wta_typed(plan, pairs, d_web, SM_WEB_I32, d_best, stream);
}

extern "C" int sm_match_wta_typed(sm_plan *plan, int pairs, void *d_web_any, int web_type,
                                  int32_t *d_best, void *stream)
{
    const char *me = web_type == SM_WEB_I32 ? "sm_match_wta" : "sm_match_wta_typed";
    SM_TRY(sm_check_pairs(plan, pairs, me));
    if (!d_web_any) return sm_fail(SM_ERR_ARG, "%s: d_web is NULL", me);
    SM_TRY(sm_check_web_type(plan, web_type, me));
    const int web_bytes = web_type == SM_WEB_I32 ? 4 : web_type == SM_WEB_U16 ? 2 : 1;
    int32_t *d_web = (int32_t *)d_web_any;
    // kernels without a narrow store path: int32 into the plan's staging map (allocated with the
    // plan), then narrow.  ONE staging map per plan: see the threading note in stereo_hip.h
    const bool via_tmp = web_bytes != 4 && plan->kernel != SM_KERNEL_BS;
    if (via_tmp) {
        if (!plan->d_web_tmp) {         // the first narrow request on such a plan (sm_plan_reserve_narrow keeps
            SM_TRY(sm_use_device(plan->device));      // this allocation, which synchronises the device, out of a timed path)
            SM_TRY(sm_ws_need(plan, SM_WS_SET_NARROW, (hipStream_t)stream, me));
        }
        d_web = plan->d_web_tmp;
    }
    SM_TRY(sm_check_pairs_loaded(plan, pairs, me));
    SM_TRY(sm_use_device(plan->device));
    // event records are not free (~4 us each on the launch stream): time a sample of
    // the launches, and record the buffer-release event only when someone can wait on it
    const bool timed = plan->timing_n < plan->timing_cap &&
                       plan->timing_seen++ % plan->timing_every == 0;
    if (timed && sm_stream_capturing((hipStream_t)stream))
        return sm_fail(SM_ERR_ARG, "%s: kernel timing is armed (sm_plan_time_kernels) and the stream is capturing: the "
                       "timing events of a launch cannot be read back from a graph -- disarm with "
                       "sm_plan_time_kernels(plan, 0) before the capture begins", me);
    // The bit-sliced kernel's launcher attaches the two events to the dispatch packet itself
    // (the completion signal's own start / end time stamps): no extra packets on the stream.
    // Separate event records cost ~4 us each there, 6 % of a 4K step when every second launch
    // is timed (bench.py at --steps 20).  Other kernels keep the bracketing records.
    const bool attach = timed && plan->kernel == SM_KERNEL_BS && !via_tmp && !plan->opt.timing_by_records;
    if (timed && !attach) SM_HIP(hipEventRecord(plan->t_begin[plan->timing_n], (hipStream_t)stream));
    {
        // what this launch adds to the plan's geometry, by value (the plan itself is not touched):
        // int4 stores need 16-byte aligned maps, otherwise this launch stores scalars; the element
        // size of the web map; the events of a timed launch
        MatchLaunch l = sm_match_launch_args(plan, d_web, d_best, via_tmp ? 4 : web_bytes);
        if (attach) { l.ev_begin = plan->t_begin[plan->timing_n]; l.ev_end = plan->t_end[plan->timing_n]; }
        const int rc = sm_match_launch(plan, l, pairs, d_web, d_best, (hipStream_t)stream);
        if (rc) return rc;
        if (via_tmp) {
            const long long n = (long long)pairs * plan->width * plan->height;
            hipLaunchKernelGGL(k_narrow_web, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                               (hipStream_t)stream, d_web, d_web_any, n, web_bytes);
            SM_LAUNCH_CHECK("k_narrow_web");
        }
    }
    if (timed && !attach) SM_HIP(hipEventRecord(plan->t_end[plan->timing_n], (hipStream_t)stream));
    if (timed) plan->timing_n++;
    if (plan->pipelined) {
        // the release event of pipelined call number seq: `stream` of sm_run waits for it, and so do
        // later calls that must not overtake this one
        SM_HIP(hipEventRecord(plan->ev_free[plan->seq & 3], (hipStream_t)stream));
        plan->ev_free_set[plan->seq & 3] = 1;
    } else {
        plan->unfenced = 1;                // launches a later pipelined phase has no event for
    }
    return SM_OK;
}

void sm_timing_free(sm_plan *plan)
{
    for (int i = 0; i < plan->timing_cap; i++) {
        (void)hipEventDestroy(plan->t_begin[i]);
        (void)hipEventDestroy(plan->t_end[i]);
    }
    free(plan->t_begin);
    free(plan->t_end);
    plan->t_begin = plan->t_end = nullptr;
    plan->timing_cap = plan->timing_n = 0;
}

extern "C" int sm_plan_time_kernels(sm_plan *plan, int capacity)
{
    if (!plan || capacity < 0 || capacity > (1 << 20))
        return sm_fail(SM_ERR_ARG, "sm_plan_time_kernels: bad argument");
    SM_TRY(sm_use_device(plan->device));
    plan->timing_seen = 0;
    if (capacity == plan->timing_cap) { plan->timing_n = 0; return SM_OK; }
    sm_timing_free(plan);
    if (capacity == 0) return SM_OK;
    plan->t_begin = (hipEvent_t *)calloc(capacity, sizeof(hipEvent_t));
    plan->t_end = (hipEvent_t *)calloc(capacity, sizeof(hipEvent_t));
    if (!plan->t_begin || !plan->t_end) return sm_fail(SM_ERR_NOMEM, "error: out of memory");
    for (int i = 0; i < capacity; i++) {
        SM_HIP(hipEventCreate(&plan->t_begin[i]));
        SM_HIP(hipEventCreate(&plan->t_end[i]));
        plan->timing_cap = i + 1;
    }
    return SM_OK;
}

extern "C" int sm_plan_time_stride(sm_plan *plan, int every)
{
    if (!plan || every < 1) return sm_fail(SM_ERR_ARG, "sm_plan_time_stride: bad argument");
    plan->timing_every = every;
    plan->timing_seen = 0;
    return SM_OK;
}

extern "C" int sm_plan_kernel_ms(sm_plan *plan, double *mean_ms, int *launches)
{
    if (!plan || !mean_ms || !launches) return sm_fail(SM_ERR_ARG, "sm_plan_kernel_ms: NULL argument");
    SM_TRY(sm_use_device(plan->device));
    double sum = 0;
    for (int i = 0; i < plan->timing_n; i++) {
        float ms = 0;
        SM_HIP(hipEventSynchronize(plan->t_end[i]));
        SM_HIP(hipEventElapsedTime(&ms, plan->t_begin[i], plan->t_end[i]));
        sum += ms;
    }
    *launches = plan->timing_n;
    *mean_ms = plan->timing_n ? sum / plan->timing_n : 0.0;
    return SM_OK;
}

// ---------------------------------------------------------------------------
// the scheduler: sm_run on `stream`, or on the plan's two lanes
// ---------------------------------------------------------------------------

extern "C" int sm_plan_set_pipelined(sm_plan *plan, int enabled)
{
    if (!plan) return sm_fail(SM_ERR_ARG, "sm_plan_set_pipelined: plan is NULL");
    plan->pipelined = enabled == 2 ? 2 : (enabled != 0);
    return SM_OK;
}

extern "C" int sm_run(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right,
                      double threshold, int pairs, int32_t *d_web, int32_t *d_best, void *stream)
{
    return sm_run_typed(plan, d_gray_left, d_gray_right, threshold, pairs, d_web, SM_WEB_I32, d_best, stream);
}

static int run_on_lanes(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right,
                        double threshold, int pairs, void *d_web, int web_type, int32_t *d_best,
                        void *stream, hipEvent_t inputs_ready);

extern "C" int sm_run_typed(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right,
                            double threshold, int pairs, void *d_web, int web_type, int32_t *d_best,
                            void *stream)
{
    if (!plan || !plan->pipelined) {
        SM_TRY(sm_find_edges(plan, d_gray_left, d_gray_right, threshold, pairs, nullptr, nullptr, stream));
        return sm_match_wta_typed(plan, pairs, d_web, web_type, d_best, stream);
    }
    return run_on_lanes(plan, d_gray_left, d_gray_right, threshold, pairs, d_web, web_type, d_best, stream, nullptr);
}

// every argument sm_find_edges and sm_match_wta_typed would refuse, refused before a call that runs them on a lane (or
// behind an event) waits for anything or moves the plan's state: a refusal after a lane's fork would leave a capture
// unjoined (hipStreamEndCapture fails) and, outside a capture, the edges of a call that never matches queued on the lane
static int check_run_args(const sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, double threshold,
                          const void *d_web, int web_type, const char *me)
{
    if (!d_gray_left || !d_gray_right) return sm_fail(SM_ERR_ARG, "%s: input image pointer is NULL", me);
    SM_TRY(sm_check_threshold(threshold, me));
    if (!d_web) return sm_fail(SM_ERR_ARG, "%s: d_web is NULL", me);
    return sm_check_web_type(plan, web_type, me);
}

// sm_run whose ONLY input dependency is an event (DESIGN.md 9.4 of round 4; replaces the synchronous upload in front of
// every call, src/stereo.cu:402-403): the call is free to overlap with the one before it, and the plan takes the two
// lanes by itself where that pays -- a match launch that does not fill the chip twice over (fewer than 2 x 1024 waves:
// a lone pair up to 4K), or a plan set pipelined.
extern "C" int sm_run_after(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right,
                            double threshold, int pairs, void *d_web, int web_type, int32_t *d_best,
                            void *stream, void *inputs_ready_event)
{
    SM_TRY(sm_check_pairs(plan, pairs, "sm_run_after"));
    const MatchGeom &g = plan->g;
    const long long waves = (long long)g.tiles_x * g.tiles_y * pairs * ((g.threads + 63) / 64);
    // (... and no more than 128 shifts: the edge detection the overlap hides is then a ninth of a step or more.  At 256 shifts --
    // C5: a 158 us match launch beside 15 us of edges -- two calls sharing the chip cost more than that: 0.1782 against 0.1755 ms
    // per step, where C3 gains 2.6 % and C1 / C2 9-19 %: profiles/r05/bench_all_configs.txt)
    if (!plan->pipelined && (waves >= 2 * 1024 || plan->num_shifts > 128)) {
        SM_TRY(check_run_args(plan, d_gray_left, d_gray_right, threshold, d_web, web_type, "sm_run_after"));
        SM_TRY(sm_use_device(plan->device));
        if (inputs_ready_event) SM_HIP(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)inputs_ready_event, 0));
        SM_TRY(sm_find_edges(plan, d_gray_left, d_gray_right, threshold, pairs, nullptr, nullptr, stream));
        return sm_match_wta_typed(plan, pairs, d_web, web_type, d_best, stream);
    }
    const int was = plan->pipelined;
    if (!was) plan->pipelined = 1;          // (the match launch records the call's release event when the plan is pipelined)
    const int rc = run_on_lanes(plan, d_gray_left, d_gray_right, threshold, pairs, d_web, web_type, d_best, stream,
                                (hipEvent_t)inputs_ready_event);
    plan->pipelined = was;
    return rc;
}

static int run_on_lanes(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right,
                        double threshold, int pairs, void *d_web, int web_type, int32_t *d_best,
                        void *stream, hipEvent_t inputs_ready)
{
    // pipelined: call q runs on one of two lanes (internal streams, alternating): its edge detection
    // into the lane's own ext buffer, then its match launch, in stream order.  Nothing orders call q
    // against call q - 1 on the other lane, so the edges of call q run beside the match of call q - 1,
    // and the first waves of match q take the SIMD slots that the early finishers of match q - 1 leave
    // (the younger wave of every SIMD pair ends alone).  Call q - 3 (the one before q - 1
    // on the other lane) has finished before q starts: at most two calls are in flight.  `stream`
    // waits for the call's release event: work the caller puts on it afterwards sees the results.
    SM_TRY(sm_check_pairs(plan, pairs, "sm_run"));
    SM_TRY(sm_use_device(plan->device));
    hipStream_t user = (hipStream_t)stream;
    unsigned long long cap_id = 0;
    const bool capturing = sm_stream_capturing(user, &cap_id);
    if (capturing) {
        // what cannot be captured is refused first (and, as every bad argument below, before the lane leaves `stream`:
        // an error must not leave the capture unjoined)
        SM_TRY(sm_check_tables_prepared(plan, threshold, "sm_run"));
        if (plan->timing_n < plan->timing_cap)
            return sm_fail(SM_ERR_ARG, "sm_run: kernel timing is armed (sm_plan_time_kernels) and the stream is capturing: "
                           "disarm with sm_plan_time_kernels(plan, 0) before the capture begins");
        if (web_type != SM_WEB_I32) SM_TRY(sm_ws_need(plan, SM_WS_SET_NARROW, user, "sm_run"));   // (capturing: a refusal)
    }
    SM_TRY(check_run_args(plan, d_gray_left, d_gray_right, threshold, d_web, web_type, "sm_run"));
    const int b = plan->cur ^ 1;
    hipStream_t lane = plan->lane[b];
    const unsigned q = plan->seq + 1;
    // what two calls in flight could share: the threshold tables (rebuilt when the threshold
    // changes), the one int32 staging map of the kernels without a narrow store path, and result
    // maps the caller hands to consecutive calls -- any of these puts call q behind call q - 1
    const size_t px = (size_t)pairs * plan->width * plan->height;
    const uintptr_t lo[2] = {(uintptr_t)d_web, (uintptr_t)d_best};
    const uintptr_t hi[2] = {lo[0] + px * (web_type == SM_WEB_I32 ? 4 : web_type == SM_WEB_U16 ? 2 : 1),
                             d_best ? lo[1] + px * 4 : 0};
    bool shared = !sm_edge_tables_prepared(plan, threshold) ||
                  (web_type != SM_WEB_I32 && plan->kernel != SM_KERNEL_BS);
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 2; j++)
            if (lo[i] < plan->out_hi[j] && plan->out_lo[j] < hi[i]) shared = true;

    if (capturing) {
        // INSIDE A STREAM CAPTURE every operation must descend from the capturing stream and join it again, and no
        // event recorded outside the capture may be waited for (hipErrorStreamCaptureIsolation -- what round 4's
        // attempt ran into: its lanes waited for the release events of calls made before the capture began;
        // tools/capture_probe.hip, profiles/r05/capture_probe.txt).  Protocol: lane b leaves `stream` at ev_fork[b],
        // which the PREVIOUS captured call recorded before it joined its own lane back -- so call q depends on
        // everything up to call q - 2 and runs beside call q - 1 in the graph, as outside a capture -- and every
        // call joins its lane back at once (`stream` waits for its release event), so the capture can end anywhere.
        // (what cannot be captured, and every bad argument, was refused above, before the lane leaves `stream`)
        const bool first = !plan->cap_live || plan->cap_id != cap_id;
        if (first) {
            plan->cap_live = 1;
            plan->cap_id = cap_id;
            SM_HIP(hipEventRecord(plan->ev_fork[b], user));
        }
        SM_HIP(hipStreamWaitEvent(lane, plan->ev_fork[b], 0));
        if (inputs_ready) SM_HIP(hipStreamWaitEvent(lane, inputs_ready, 0));     // (an event of this capture, or the call fails)
        if (shared && !first) SM_HIP(hipStreamWaitEvent(lane, plan->ev_free[(q - 1) & 3], 0));
    } else {
        plan->cap_live = 0;
        if (plan->unfenced || plan->pipelined == 2) {
            // work already on `stream` that a lane must not overtake: the launches of a sequential phase
            // (once, both lanes) or, in ordered mode, whatever produces this call's inputs (this lane)
            SM_HIP(hipEventRecord(plan->ev_inputs, user));
            SM_HIP(hipStreamWaitEvent(lane, plan->ev_inputs, 0));
            if (plan->unfenced) SM_HIP(hipStreamWaitEvent(plan->lane[b ^ 1], plan->ev_inputs, 0));
            plan->unfenced = 0;
        }
        if (inputs_ready) SM_HIP(hipStreamWaitEvent(lane, inputs_ready, 0));
        if (plan->ev_free_set[(q - 3) & 3]) SM_HIP(hipStreamWaitEvent(lane, plan->ev_free[(q - 3) & 3], 0));
        if (shared && plan->ev_free_set[(q - 1) & 3]) SM_HIP(hipStreamWaitEvent(lane, plan->ev_free[(q - 1) & 3], 0));
    }
    plan->seq = q;
    plan->cur = b;
    plan->d_ext = plan->d_ext_buf[b];
    for (int i = 0; i < 2; i++) { plan->out_lo[i] = lo[i]; plan->out_hi[i] = hi[i]; }
    SM_TRY(sm_find_edges(plan, d_gray_left, d_gray_right, threshold, pairs, nullptr, nullptr, (void *)lane));
    SM_TRY(sm_match_wta_typed(plan, pairs, d_web, web_type, d_best, (void *)lane));   // records ev_free[q & 3] on the lane
    if (capturing) SM_HIP(hipEventRecord(plan->ev_fork[b ^ 1], user));     // (where the next captured call's lane leaves)
    SM_HIP(hipStreamWaitEvent(user, plan->ev_free[q & 3], 0));
    if (capturing) {
        // the events of a capture are nodes of its graph: nothing outside it waits for them, and the next call outside a
        // capture orders its lanes behind `stream` (where the graph is launched, if it is)
        for (int i = 0; i < 4; i++) plan->ev_free_set[i] = 0;
        plan->unfenced = 1;
    }
    return SM_OK;
}

// A call of another unit that reads or rewrites the packed images runs on `stream`; the pipelined calls before it may
// still be running on the plan's lanes (sm_plan_set_pipelined, sm_run_after): `stream` waits for all of
// them.  Inside a capture the captured calls have joined `stream` already (and events of eager calls
// must not be waited for there).
int sm_lanes_fence(sm_plan *plan, hipStream_t st)
{
    if (sm_stream_capturing(st)) return SM_OK;
    for (int i = 0; i < 4; i++)
        if (plan->ev_free_set[i]) SM_HIP(hipStreamWaitEvent(st, plan->ev_free[i], 0));
    return SM_OK;
}

// ... and the next pipelined call must not overtake it: as after any sequential launch, its lanes wait for
// `stream` first (a captured one leaves `stream` after this call, not where the previous captured call ended)
void sm_lanes_release(sm_plan *plan)
{
    plan->unfenced = 1;
    plan->cap_live = 0;
}

// the debug tap (k_debug_planes above)
extern "C" int sm_debug_planes(sm_plan *plan, int pair, int shift, uint8_t *d_match,
                               int32_t *d_score_all, int32_t *d_scores, void *stream)
{
    if (!plan) return sm_fail(SM_ERR_ARG, "sm_debug_planes: plan is NULL");
    if (pair < 0 || pair >= plan->pairs_loaded)
        return sm_fail(SM_ERR_ARG, "sm_debug_planes: pair %d not loaded (%d loaded)", pair,
                       plan->pairs_loaded);
    if (shift < 0 || shift >= plan->num_shifts)
        return sm_fail(SM_ERR_ARG, "sm_debug_planes: shift %d outside 0..%d", shift,
                       plan->num_shifts - 1);
    SM_TRY(sm_use_device(plan->device));
    const MatchGeom &g = plan->g;
    const dim3 grid((g.w + 255) / 256, g.h), block(256);
    hipLaunchKernelGGL(k_debug_planes, grid, block, 0, (hipStream_t)stream, plan->d_ext, pair, shift,
                       d_match, d_score_all, d_scores, g, plan->border == SM_GHOST ? 1 : 0);
    SM_LAUNCH_CHECK("k_debug_planes");
    return SM_OK;
}
