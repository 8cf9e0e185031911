"""The guided weighted median on the GPU: sm_weighted_median against the numpy definition (tests/wmedian_reference.py),
exactly.  Every expected value comes from the CPU definition; none from the HIP path.  The cases are those of
tests/wmedian_patterns.py (test_wmedian_cpu.py shows what they can tell): the kernel works on 64 x 16 tiles, keeps the
window in registers up to radius 3 and reads it from LDS above, and the sizes sit on and around every tile edge."""
import ctypes as C

import numpy as np
import pytest
import torch

from stereomatching_amd import capi
from stereomatching_amd.capi import lib
from tests import wmedian_patterns as wp
from tests import wmedian_reference as wr
from tests.guarded import guarded_input
from tests.test_write_bounds_gpu import P, Plan, expect, out, report, stream, twice

pytestmark = pytest.mark.gpu
DTYPES = [np.int32, np.int16]
TORCH = {np.int32: torch.int32, np.int16: torch.int16}
TYPE = {np.int32: capi.SM_MAP_I32, np.int16: capi.SM_MAP_I16}


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                       # (a copy: the shared inputs are read-only)


def host(t):
    return t.cpu().numpy()


def plan_for(hip, w, h, max_pairs=1):
    """the filter reads W, H and max_pairs of the plan only"""
    return hip.StereoPlan(w, h, 4, 1, "ghost", max_pairs=max_pairs)


def run_cases(hip, cases):
    """every case through StereoPlan.weighted_median (one plan per size and batch limit) -> problems"""
    bad, plans = [], {}
    try:
        for c in cases:
            key = (c["w"], c["h"], c["max_pairs"])
            if key not in plans:
                plans[key] = plan_for(hip, *key)
            maps, guides, weights, fill, fmw = wp.inputs(c["name"])
            want, want_filled = wp.expected(c["name"])
            got, filled = plans[key].weighted_median(dev(maps), dev(guides), c["radius"], weights, fill=fill,
                                                     fill_min_weight=fmw, want_filled=True)
            got, filled = host(got), host(filled)
            for q in range(c["pairs"]):
                diff = np.argwhere(got[q] != want[q])
                if len(diff):
                    y, x = (int(v) for v in diff[0])
                    bad.append(f"{c['name']} pair {q}: {len(diff)} pixels differ, first (x={x}, y={y}): "
                               f"{got[q][y, x]} != {want[q][y, x]} (in {maps[q][y, x]})")
                if int(filled[q]) != int(want_filled[q]):
                    bad.append(f"{c['name']} pair {q}: filled {int(filled[q])} != {int(want_filled[q])}")
    finally:
        for p in plans.values():
            p.close()
    return bad


@pytest.mark.parametrize("dtype", ["int32", "int16"])
@pytest.mark.parametrize("radius", [1, 2, 3, 4, 5, 6, 7])
def test_random_maps(hip, dtype, radius):
    cases = [c for c in wp.CASES if c["kind"] == "random" and c["dtype"] == dtype and c["radius"] == radius]
    assert len(cases) >= 3
    report(run_cases(hip, cases))


@pytest.mark.parametrize("kind", ["extremes", "step"])
def test_special_cases(hip, kind):
    """the ends of the types mixed in one window; a guide whose step lies on x = 64 and on y = 16"""
    cases = [c for c in wp.CASES if c["kind"] == kind]
    assert len(cases) >= 4
    report(run_cases(hip, cases))


def test_without_the_flag_nothing_is_filled_and_the_count_is_zero(hip):
    c = wp.BY_NAME["random int32 65x17 r3"]
    maps, guides, weights, _, _ = wp.inputs(c["name"])
    plan = plan_for(hip, c["w"], c["h"], c["max_pairs"])
    try:
        got, filled = plan.weighted_median(dev(maps), dev(guides), 3, weights, fill=False, fill_min_weight=0, want_filled=True)
        want = np.stack([wr.weighted_median(m, g, 3, weights)[0] for m, g in zip(maps, guides)])
        assert np.array_equal(host(got), want) and not host(filled).any()
        assert (maps == 0).any() and not host(got)[maps == 0].any()
        with pytest.raises(ValueError, match="guide"):
            plan.weighted_median(dev(maps), dev(guides).to(torch.int32), 3, weights)
    finally:
        plan.close()


# ---------------------------------------------------------------------------
# write bounds (tests/guarded.py)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_writes_its_map_and_nothing_else(dtype):
    bad = []
    td, ty = TORCH[dtype], TYPE[dtype]
    odd = 4 if dtype is np.int32 else 2
    weights = capi.w256(wp.guide_weights(8))
    for idx, (w, h, radius) in enumerate([(33, 17, 2), (64, 16, 7), (130, 35, 5), (1, 5, 3)]):
        pairs, maxp = (2, 3) if idx % 2 == 0 else (1, 2)
        plan = Plan(w, h, 4, 1, "toroidal", maxp)
        maps = np.stack([wp.random_map(w, h, dtype, 9 * idx + q, 0.3, 6, True) for q in range(pairs)])
        guides = np.stack([wp.random_guide(w, h, 9 * idx + q) for q in range(pairs)])
        shp, s = (pairs, h, w), stream()
        tag = f"{np.dtype(dtype).name} W={w} H={h} r={radius} pairs={pairs}/{maxp}"
        for off in (0, odd):
            gi, gg = guarded_input(maps, "cuda", off, "in"), guarded_input(guides, "cuda", (1, 3)[idx % 2] if off else 0, "guide")
            for fill, fmw in ((0, 1), (capi.SM_WMED_FILL, 700)):
                want = [wr.weighted_median(m, g, radius, wp.guide_weights(8), bool(fill), fmw) for m, g in zip(maps, guides)]
                t = f"{tag} flags={fill} offset {off}"
                om, of = out(shp, td, odd - off, maxp, "out"), out((pairs,), torch.int32, off and 4, maxp, "filled")
                bad += twice(t, lambda r: lib.sm_weighted_median(plan.h, P(gi.t), ty, P(gg.t), radius, weights, fill, fmw,
                                                                 pairs, P(om.t), P(of.t), s), [om, of], [gi, gg])
                bad += expect(t, om, np.stack([x[0] for x in want])) + expect(t, of, [x[1] for x in want])
                t += " (no count)"
                om = out(shp, td, off, maxp, "out")
                bad += twice(t, lambda r: lib.sm_weighted_median(plan.h, P(gi.t), ty, P(gg.t), radius, weights, fill, fmw,
                                                                 pairs, P(om.t), None, s), [om], [gi, gg])
                bad += expect(t, om, np.stack([x[0] for x in want]))
        plan.close()
    report(bad)


# ---------------------------------------------------------------------------
# capture, arguments
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_captured_into_a_graph(hip, dtype):
    """no workspace, no copy: captured as it is on a plan with the default queue settings; the replays use the weight
    table of capture time, whatever the host array holds by then"""
    w, h, radius = 200, 90, 4
    maps = [wp.random_map(w, h, dtype, 40 + i, 0.3, 2000, True) for i in range(2)]
    guides = [wp.random_guide(w, h, 40 + i) for i in range(2)]
    table = wp.guide_weights(8)
    weights = capi.w256(table)
    plan = plan_for(hip, w, h)
    try:
        base = plan.workspace_bytes()
        src = torch.zeros((1, h, w), dtype=TORCH[dtype], device="cuda")
        gsrc = torch.zeros((1, h, w), dtype=torch.uint8, device="cuda")
        res = torch.zeros_like(src)
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            capi.check(lib.sm_weighted_median(plan._h, P(src), TYPE[dtype], P(gsrc), radius, weights, capi.SM_WMED_FILL, 900, 1,
                                              P(res), P(cnt), plan._stream()))
        for i in range(256):
            weights[i] = 1                                            # the host's table changes after the capture
        assert plan.workspace_bytes() == base
        seen = []
        for rep in (0, 0, 1):                                         # the same input twice, then another
            src.copy_(dev(maps[rep])[None])
            gsrc.copy_(dev(guides[rep])[None])
            res.zero_()
            cnt.fill_(12345)
            g.replay()
            torch.cuda.synchronize()
            want, n = wr.weighted_median(maps[rep], guides[rep], radius, table, True, 900)
            assert np.array_equal(host(res)[0], want), rep
            assert int(cnt[0]) == n and n > 0, rep
            seen.append(host(res).copy())
        assert np.array_equal(seen[0], seen[1])
        assert not np.array_equal(seen[0][0], wr.weighted_median(maps[0], guides[0], radius, np.ones(256, np.uint16), True, 900)[0])
    finally:
        plan.close()


def test_argument_checks_on_a_plan(hip):
    w, h = 64, 32
    plan = plan_for(hip, w, h, 2)
    base = plan.workspace_bytes()
    m = [torch.full((2, h, w), 77, dtype=torch.int32, device="cuda") for _ in range(2)]
    guide = torch.zeros((2, h, w), dtype=torch.uint8, device="cuda")
    cnt = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    p, pg, pc = [C.c_void_p(t.data_ptr()) for t in m], C.c_void_p(guide.data_ptr()), C.c_void_p(cnt.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    inside = C.c_void_p(m[0].data_ptr() + 4)
    I32, I16, FILL = capi.SM_MAP_I32, capi.SM_MAP_I16, capi.SM_WMED_FILL
    wt = capi.w256(wp.guide_weights(8))
    zero = capi.w256([0] + [9] * 255)

    def refused(rc, text):
        assert rc == capi.SM_ERR_ARG and b"sm_weighted_median: " + text in lib.sm_last_error(), lib.sm_last_error()
        torch.cuda.synchronize()
        assert bool((m[1] == 77).all()) and bool((cnt == 77).all())   # the output and the counts are untouched
    refused(lib.sm_weighted_median(plan._h, p[0], I32, pg, 3, wt, 0, 1, 2, p[0], pc, st), b"maps overlap")
    refused(lib.sm_weighted_median(plan._h, inside, I32, pg, 3, wt, 0, 1, 1, p[0], pc, st), b"maps overlap")
    refused(lib.sm_weighted_median(plan._h, p[0], I16, pg, 3, wt, 0, 1, 2, C.c_void_p(m[0].data_ptr() + 2 * h * w), pc, st),
            b"maps overlap")
    refused(lib.sm_weighted_median(plan._h, p[0], I32, p[1], 3, wt, 0, 1, 1, p[1], pc, st), b"d_guide overlaps the output map")
    refused(lib.sm_weighted_median(plan._h, p[0], I32, pg, 3, wt, FILL, 1, 2, p[1], C.c_void_p(m[1].data_ptr() + 8), st),
            b"d_filled overlaps a map")
    refused(lib.sm_weighted_median(plan._h, p[0], I32, pg, 0, wt, 0, 1, 1, p[1], pc, st), b"radius 0 outside 1..7")
    refused(lib.sm_weighted_median(plan._h, p[0], I32, pg, 8, wt, 0, 1, 1, p[1], pc, st), b"radius 8 outside 1..7")
    refused(lib.sm_weighted_median(plan._h, p[0], I32, pg, 3, zero, 0, 1, 1, p[1], pc, st), b"weights[0] is 0")
    refused(lib.sm_weighted_median(plan._h, p[0], I32, pg, 3, wt, 4, 1, 1, p[1], pc, st), b"flags 0x4")
    refused(lib.sm_weighted_median(plan._h, p[0], I32, pg, 3, wt, FILL | 2, 1, 1, p[1], pc, st), b"flags 0x3")
    refused(lib.sm_weighted_median(plan._h, p[0], I32, pg, 3, wt, FILL, 0, 1, p[1], pc, st), b"fill_min_weight 0 is below 1")
    refused(lib.sm_weighted_median(plan._h, p[0], I32, pg, 3, wt, 0, 1, 3, p[1], pc, st), b"pairs 3 outside 1..2")
    refused(lib.sm_weighted_median(plan._h, p[0], 5, pg, 3, wt, 0, 1, 1, p[1], pc, st), b"map_type 5")
    refused(lib.sm_weighted_median(plan._h, p[0], I32, None, 3, wt, 0, 1, 1, p[1], pc, st), b"d_guide is NULL")
    refused(lib.sm_weighted_median(plan._h, p[0], I32, pg, 3, None, 0, 1, 1, p[1], pc, st), b"weights is NULL")
    refused(lib.sm_weighted_median(plan._h, p[0], I32, pg, 3, wt, 0, 1, 1, None, pc, st), b"a map pointer is NULL")
    assert plan.workspace_bytes() == base
    with pytest.raises(capi.StereoHipError, match="sm_weighted_median: radius 9"):
        plan.weighted_median(m[0], guide, 9, wp.guide_weights(8))
    with pytest.raises(ValueError, match="int32 .* or int16"):
        plan.weighted_median(guide, guide, 3, wp.guide_weights(8))
    plan.close()
