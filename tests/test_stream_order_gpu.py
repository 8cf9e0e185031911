"""Stream ordering of the calls that run on a plan's two internal lanes (run_on_lanes in csrc/sm_run.hip: sm_run_after on
small launches, sm_run on a pipelined plan).  Such a call is ordered by events alone -- `inputs_ready`, the release
events, the `ev_inputs` fence, the fork events of a capture -- so a missing or misplaced wait only shows when the work
on the other side of the event is still running when the lane starts.  Every producer and consumer here is therefore
held back by a spin kernel (torch.cuda._sleep) that lasts many times a whole call, and every map is compared with the
CPU oracle of its own pair."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from stereomatching_amd.synth import make_pair
from tests import oracle

pytestmark = pytest.mark.gpu

W, H, D, SW, THR = 320, 200, 64, 7, 0.15
SPIN_MIN_MS = 20.0          # a spin shorter than this, or than 20 match launches, proves nothing
SPIN_CAP_MS = 200.0         # ... and a miscalibrated one must not run long
NPAIRS = 8


@functools.lru_cache(maxsize=None)
def pair(i):
    return make_pair(W, H, D, seed=600 + i)


@functools.lru_cache(maxsize=None)
def want(i, d=D):
    """(web-1, score_best-0) of the oracle for pair i at d shifts"""
    o = oracle.pipeline(*pair(i), THR, d, SW, step3=False)
    return o["web-1"], o["score_best-0"]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def unset(dtype=torch.int32):
    """a result map that no correct call leaves as it is"""
    return torch.full((1, H, W), -1, dtype=dtype, device="cuda")


def check_maps(tag, i, web, best=None, d=D):
    w, b = want(i, d)
    assert np.array_equal(host(web)[0], w), f"{tag}: web of pair {i}"
    if best is not None:
        assert np.array_equal(host(best)[0], b), f"{tag}: best of pair {i}"


def lane_plan(hip, d=D):
    """A plan whose sm_run_after takes the lanes by itself (fewer than 2 x 1024 waves, at most 128 shifts): asserted,
    so that a change of that rule cannot turn these tests into tests of plain stream order."""
    plan = hip.StereoPlan(W, H, d, SW)
    g = plan.geometry()
    waves = g["tiles_x"] * g["tiles_y"] * ((g["threads"] + 63) // 64)
    assert waves < 2 * 1024 and d <= 128, (waves, d)
    plan.prepare_threshold(THR)
    return plan


class Spin:
    def __init__(self, cycles, ms):
        self.cycles, self.ms = cycles, ms

    def __call__(self):
        """queue the spin on the current stream"""
        torch.cuda._sleep(self.cycles)


def _elapsed_ms(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


@pytest.fixture(scope="session")
def spin(hip):
    """A spin of at least 20 ms and at least 20 x the match launch of the test geometry, measured here (fails, not
    skips, if it cannot be had: a shorter spin would leave every test below without its point)."""
    assert hasattr(torch.cuda, "_sleep"), "torch.cuda._sleep is missing: nothing can hold a stream back"
    plan = lane_plan(hip)
    a, b = dev(pair(0)[0]), dev(pair(0)[1])
    web, best = unset(), unset()
    plan.run(a, b, THR, want_best=True, web=web, best=best)
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    match_ms = _elapsed_ms(lambda: plan.match_wta(1, want_best=True, web=web, best=best), 50)
    run_ms = _elapsed_ms(lambda: plan.run(a, b, THR, want_best=True, web=web, best=best), 50)
    plan.close()
    cycles, ms = 1 << 20, 0.0
    for _ in range(6):                  # (each step at most 8 x a spin of < 2 ms)
        ms = _elapsed_ms(lambda: torch.cuda._sleep(cycles))
        if ms >= 2.0:
            break
        cycles *= 8
    assert ms >= 2.0, f"torch.cuda._sleep({cycles}) took {ms} ms: cannot calibrate"
    per_ms = cycles / ms
    target = min(0.75 * SPIN_CAP_MS, max(1.5 * SPIN_MIN_MS, 30 * run_ms))
    cycles = int(target * per_ms)
    ms = _elapsed_ms(lambda: torch.cuda._sleep(cycles))
    print(f"\nspin calibration: {per_ms:.0f} cycles/ms; match_wta {1e3 * match_ms:.1f} us, run {1e3 * run_ms:.1f} us "
          f"({W}x{H}, {D} shifts, {SW}x{SW}); spin of {cycles} cycles = {ms:.1f} ms")
    assert ms >= SPIN_MIN_MS, ms
    assert ms >= 20 * match_ms, (ms, match_ms)
    assert ms <= 1.25 * SPIN_CAP_MS, ms
    return Spin(cycles, ms)


def _late_uploads(spin, n):
    """n input pairs whose uploads go out on a copy stream behind a spin (zeros first, then the pair), an event behind
    each; until then the buffers hold a neighbour's pair"""
    hl = [torch.from_numpy(pair(i)[0]).pin_memory() for i in range(n)]
    hr = [torch.from_numpy(pair(i)[1]).pin_memory() for i in range(n)]
    dl = [dev(pair((i + 1) % n)[0]) for i in range(n)]
    dr = [dev(pair((i + 1) % n)[1]) for i in range(n)]
    copy = torch.cuda.Stream()
    torch.cuda.synchronize()
    evs = []
    with torch.cuda.stream(copy):
        spin()
        for i in range(n):
            dl[i].zero_()
            dr[i].zero_()
            dl[i].copy_(hl[i], non_blocking=True)
            dr[i].copy_(hr[i], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(copy)
            evs.append(ev)
    return dl, dr, evs, (hl, hr)


def test_e1_lane_waits_for_inputs_ready(hip, spin):
    """E1: six calls go out at once, each behind the event of its late upload.  A lane that did not wait for its event
    reads a neighbour's pair or zeros."""
    plan = lane_plan(hip)
    n = 6
    webs, bests = [unset() for _ in range(n)], [unset() for _ in range(n)]
    dl, dr, evs, pinned = _late_uploads(spin, n)
    for i in range(n):
        plan.run_after(dl[i], dr[i], THR, inputs_ready=evs[i], want_best=True, web=webs[i], best=bests[i])
    torch.cuda.synchronize()
    for i in range(n):
        check_maps("E1", i, webs[i], bests[i])
    plan.close()


@pytest.mark.parametrize("user", ["default stream", "side stream"])
def test_e2_work_after_the_call_sees_the_results(hip, spin, user):
    """E2: as E1, and a clone of each map queued on the caller's stream right after its call: the clone must wait for
    the call's release event (the join of the lane back into `stream`), not run while the lane waits for its inputs.
    Also from a torch side stream: the default stream may be ordered against other streams by the runtime itself."""
    plan = lane_plan(hip)
    n = 6
    webs, bests = [unset() for _ in range(n)], [unset() for _ in range(n)]
    s = torch.cuda.current_stream() if user == "default stream" else torch.cuda.Stream()
    dl, dr, evs, pinned = _late_uploads(spin, n)
    clones = []
    with torch.cuda.stream(s):
        for i in range(n):
            plan.run_after(dl[i], dr[i], THR, inputs_ready=evs[i], want_best=True, web=webs[i], best=bests[i])
            clones.append((webs[i].clone(), bests[i].clone()))
    torch.cuda.synchronize()
    for i, (w, b) in enumerate(clones):
        check_maps(f"E2 {user}", i, w, b)
    plan.close()


def test_e3_ordered_pipelining_waits_for_producers_on_stream(hip, spin):
    """E3: set_pipelined(2): the inputs of every call are copied into the SAME buffers on the current stream behind a
    spin, just before the call; ten calls without a synchronisation in between."""
    plan = lane_plan(hip)
    plan.set_pipelined(2)
    n = 10
    src = [(dev(pair(i % NPAIRS)[0]), dev(pair(i % NPAIRS)[1])) for i in range(n)]
    bl, br = dev(pair(NPAIRS - 1)[1]), dev(pair(NPAIRS - 1)[0])  # a swapped pair: no call's inputs
    webs = [unset() for _ in range(n)]
    torch.cuda.synchronize()
    for i in range(n):
        spin()
        bl.copy_(src[i][0], non_blocking=True)
        br.copy_(src[i][1], non_blocking=True)
        plan.run(bl, br, THR, web=webs[i])
    torch.cuda.synchronize()
    for i in range(n):
        check_maps("E3", i % NPAIRS, webs[i])
    plan.close()


@pytest.mark.parametrize("user", ["default stream", "side stream"])
def test_e4_first_lane_call_after_a_sequential_phase_is_fenced(hip, spin, user):
    """E4: on the caller's stream, the replay of a graph of captured calls, then a plain (not pipelined) run whose match
    is held back by a spin -- find_all_edges, the spin, match_wta: sm_run's two stages -- then lane calls.  The lanes
    share the plan's edge workspace with that sequential phase: the first lane call must be ordered behind it (the
    `ev_inputs` fence of an `unfenced` plan), or the second lane call overwrites the edges the held-back match has yet
    to read.  (The replay comes first: a graph launch behind a pending spin may hold the host until the spin is over,
    and the lane calls would then be issued too late to overtake anything.)"""
    plan = lane_plan(hip)
    ins = [(dev(l), dev(r)) for l, r in map(pair, range(6))]
    gw = [unset(), unset()]
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        plan.run_after(*ins[1], THR, web=gw[0])
        plan.run_after(*ins[2], THR, web=gw[1])
    s = torch.cuda.current_stream() if user == "default stream" else torch.cuda.Stream()
    for rep in range(2):            # (three lane calls per rep: the lane that would overwrite the edges alternates)
        seq, seq_best, after = unset(), unset(), [unset() for _ in range(3)]
        for t in gw:
            t.fill_(-1)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
            plan.find_all_edges(*ins[0], THR, want_edges=False)
            spin()
            plan.match_wta(1, want_best=True, web=seq, best=seq_best)
            for k in range(3):
                plan.run_after(*ins[3 + k], THR, web=after[k])
        torch.cuda.synchronize()
        check_maps(f"E4 {user} plain run, rep {rep}", 0, seq, seq_best)
        for k in range(2):
            check_maps(f"E4 {user} graph, rep {rep}", 1 + k, gw[k])
        for k in range(3):
            check_maps(f"E4 {user} run_after, rep {rep}", 3 + k, after[k])
    plan.close()


def test_e5_maps_the_wrapper_allocates_outlive_their_consumers(hip, spin):
    """E5: `web, best = run_after(...)`, a consumer of the map queued on the current stream behind a spin, `del web,
    best`, eight times.  A freed block of the current stream's pool may be handed straight to the next call, whose
    lane is not ordered behind that stream: the wrapper's maps must not be reused before their consumers have run."""
    ins = [(dev(l), dev(r)) for l, r in map(pair, range(NPAIRS))]
    for mode in ("run_after", "pipelined run"):
        plan = lane_plan(hip)
        call = plan.run_after
        if mode == "pipelined run":
            plan.set_pipelined(True)
            call = plan.run
        torch.cuda.synchronize()
        keep, seen, reused = [], set(), 0
        for i in range(NPAIRS):
            web, best = call(*ins[i], THR, want_best=True)
            reused += web.data_ptr() in seen
            seen.add(web.data_ptr())
            spin()
            keep.append((web.clone(), best.clone()))
            del web, best
        torch.cuda.synchronize()
        print(f"\nE5 {mode}: {reused} of {NPAIRS - 1} result maps took a block an earlier call's map was freed from")
        for i, (w, b) in enumerate(keep):
            check_maps(f"E5 {mode}", i, w, b)
        plan.close()


def test_e6_captured_producers_and_consumers(hip, spin):
    """E6: inside a capture, per pair: a spin, the copy of its inputs into the one input buffer pair, an event, the
    call waiting for that event, a spin and a clone of the maps.  Replayed three times."""
    plan = lane_plan(hip)
    n = 4
    src = [(dev(l), dev(r)) for l, r in map(pair, range(n))]
    bl, br = torch.zeros((H, W), dtype=torch.uint8, device="cuda"), torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    webs, bests = [unset() for _ in range(n)], [unset() for _ in range(n)]
    clones = []
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        for i in range(n):
            spin()
            bl.copy_(src[i][0])
            br.copy_(src[i][1])
            ev = torch.cuda.Event()
            ev.record()
            plan.run_after(bl, br, THR, inputs_ready=ev, want_best=True, web=webs[i], best=bests[i])
            spin()
            clones.append((webs[i].clone(), bests[i].clone()))
    for rep in range(3):
        for t in webs + bests + [c for wb in clones for c in wb]:
            t.fill_(-1)
        bl.copy_(src[n - 1][1])
        br.copy_(src[n - 1][0])
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for i in range(n):
            check_maps(f"E6 clone, replay {rep}", i, *clones[i])
            check_maps(f"E6 map, replay {rep}", i, webs[i], bests[i])
    # a map the wrapper would allocate inside the capture could be a block freed there whose consumer the lane is not
    # ordered behind: refused, naming the remedy
    with pytest.raises(ValueError, match="web="):
        with torch.cuda.graph(torch.cuda.CUDAGraph(), capture_error_mode="thread_local"):
            plan.run_after(*src[0], THR)
    # ... after what cannot be captured at all, which the library names first
    plan.time_kernels(2)
    with pytest.raises(hip.capi.StereoHipError, match="sm_plan_time_kernels"):
        with torch.cuda.graph(torch.cuda.CUDAGraph(), capture_error_mode="thread_local"):
            plan.run_after(*src[0], THR)
    plan.time_kernels(0)
    plan.set_pipelined(True)
    with pytest.raises(ValueError, match="best="):
        with torch.cuda.graph(torch.cuda.CUDAGraph(), capture_error_mode="thread_local"):
            plan.run(*src[0], THR, want_best=True, web=webs[0])
    plan.close()


# the argument errors sm_find_edges / sm_match_wta_typed would find: run_on_lanes must refuse them before its lane
# leaves the stream (a u8 map of more than 255 shifts needs a plan of 256 shifts, whose sm_run_after stays in stream
# order: there only the pipelined plan takes the lanes)
LATE_REFUSALS = ["null_left", "null_right", "null_web", "web_type", "u8_over_255_shifts"]


def _refused_call(hip, plan, lanes, l, r, web, kind):
    lib, capi = hip.capi.lib, hip.capi
    lp, rp, wp = C.c_void_p(l.data_ptr()), C.c_void_p(r.data_ptr()), C.c_void_p(web.data_ptr())
    wt = capi.SM_WEB_I32
    if kind == "null_left":
        lp = None
    elif kind == "null_right":
        rp = None
    elif kind == "null_web":
        wp = None
    elif kind == "web_type":
        wt = 3
    else:
        wt = capi.SM_WEB_U8                 # (the int32 map has room for it)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if lanes == "pipelined run":
        rc = lib.sm_run_typed(plan._h, lp, rp, THR, 1, wp, wt, None, st)
    else:
        rc = lib.sm_run_after(plan._h, lp, rp, THR, 1, wp, wt, None, st, None)
    assert rc == capi.SM_ERR_ARG, (lanes, kind, rc)


@pytest.mark.parametrize("kind", LATE_REFUSALS)
def test_e7_refusals_leave_the_capture_valid(hip, kind):
    """E7: valid call, refused call, valid call -- inside a capture on a pipelined plan and through run_after on a plain
    one, then the same outside a capture.  The capture ends without error, its replay gives the oracle maps of the
    two valid calls, and the plan goes on giving them."""
    d = 256 if kind == "u8_over_255_shifts" else D
    ins = [(dev(l), dev(r)) for l, r in map(pair, range(2))]
    for lanes in ("pipelined run", "run_after"):
        if d <= 128:
            plan = lane_plan(hip, d)
        else:
            plan = hip.StereoPlan(W, H, d, SW)
            plan.prepare_threshold(THR)
        call = plan.run_after
        if lanes == "pipelined run":
            plan.set_pipelined(True)
            call = plan.run
        wa, wb, junk = unset(), unset(), unset()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            call(*ins[0], THR, web=wa)
            _refused_call(hip, plan, lanes, *ins[1], junk, kind)
            call(*ins[1], THR, web=wb)
        for rep in range(2):
            wa.fill_(-1)
            wb.fill_(-1)
            g.replay()
            torch.cuda.synchronize()
            check_maps(f"E7 {lanes} {kind}, replay {rep}", 0, wa, d=d)
            check_maps(f"E7 {lanes} {kind}, replay {rep}", 1, wb, d=d)
        for rep in range(2):
            wa.fill_(-1)
            wb.fill_(-1)
            call(*ins[0], THR, web=wa)
            _refused_call(hip, plan, lanes, *ins[1], junk, kind)
            call(*ins[1], THR, web=wb)
            torch.cuda.synchronize()
            check_maps(f"E7 {lanes} {kind}, eager {rep}", 0, wa, d=d)
            check_maps(f"E7 {lanes} {kind}, eager {rep}", 1, wb, d=d)
        plan.close()
