"""The half-resolution path on the GPU: sm_reduce_half and sm_upsample_double against the numpy definition
(tests/pyramid_reference.py), exactly.  Every expected value comes from the CPU definition; none from the HIP path.
The cases are those of tests/pyramid_patterns.py (test_pyramid_cpu.py shows what they can tell): k_reduce_half gives a
lane four coarse pixels and sends the lanes at the ends of a row down another path, k_upsample_double works on
64 x 16 fine tiles, and the sizes sit on and around every such edge."""
import ctypes as C

import numpy as np
import pytest
import torch

from stereomatching_amd import capi
from stereomatching_amd.capi import lib
from stereomatching_amd.synth import make_pair
from tests import census_reference as cr
from tests import pyramid_patterns as pp
from tests import pyramid_reference as pr
from tests.guarded import guarded_input
from tests.test_write_bounds_gpu import P, Plan, expect, out, report, stream, twice

pytestmark = pytest.mark.gpu
DTYPES = [np.int32, np.int16]
TORCH = {np.int32: torch.int32, np.int16: torch.int16}
TYPE = {np.int32: capi.SM_MAP_I32, np.int16: capi.SM_MAP_I16}
FILTER = {"box": capi.SM_REDUCE_BOX, "binomial": capi.SM_REDUCE_BINOMIAL}


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                       # (a copy: the shared inputs are read-only)


def host(t):
    return t.cpu().numpy()


def plan_for(hip, w, h, max_pairs=pp.MAX_PAIRS):
    """both stages read W, H and max_pairs of the plan only"""
    return hip.StereoPlan(w, h, 4, 1, "ghost", max_pairs=max_pairs)


def first_difference(tag, got, want):
    diff = np.argwhere(got != want)
    if not len(diff):
        return []
    i = tuple(int(v) for v in diff[0])
    return [f"{tag}: {len(diff)} pixels differ, first (image, y, x) = {i}: {got[i]} != {want[i]}"]


@pytest.mark.parametrize("filter", pp.FILTERS)
def test_reduce(hip, filter):
    bad = []
    for c in pp.REDUCE_CASES:
        w, h = c["w"], c["h"]
        plan = plan_for(hip, w, h)
        try:
            assert plan.half_shape() == pr.half_shape(w, h)
            images, want = pp.reduce_images(w, h), pp.reduce_expected(w, h, filter)
            for first, n in pp.REDUCE_CALLS:
                got = host(plan.reduce_half(dev(images[first:first + n]), filter))
                bad += first_difference(f"{c['name']} {filter} images {first}..{first + n - 1}", got, want[first:first + n])
        finally:
            plan.close()
    report(bad)


@pytest.mark.parametrize("dtype", ["int32", "int16"])
def test_upsample(hip, dtype):
    cases = [c for c in pp.UP_CASES if c["dtype"] == dtype]
    assert len(cases) >= 50
    bad, plans = [], {}
    try:
        for c in cases:
            key = (c["w"], c["h"])
            if key not in plans:
                plans[key] = plan_for(hip, *key)
            maps, guides, coarse, weights, fill = pp.up_inputs(c["name"])
            got = host(plans[key].upsample_double(dev(maps), dev(guides), dev(coarse), weights, fill=fill))
            bad += first_difference(c["name"], got, pp.up_expected(c["name"]))
    finally:
        for p in plans.values():
            p.close()
    report(bad)


# ---------------------------------------------------------------------------
# write bounds (tests/guarded.py)
# ---------------------------------------------------------------------------

def test_reduce_writes_its_images_and_nothing_else():
    bad = []
    for idx, (w, h) in enumerate([(33, 17), (64, 16), (257, 3), (1, 5), (9, 2), (514, 9)]):
        images, maxp = (3, 2) if idx % 2 == 0 else (4, 2)
        cw, ch = pr.half_shape(w, h)
        plan = Plan(w, h, 4, 1, "toroidal", maxp)
        src = np.random.default_rng(idx).integers(0, 256, (images, h, w)).astype(np.uint8)
        s = stream()
        for off in (0, 1, 3):
            gi = guarded_input(src, "cuda", off, "src")
            for name in pp.FILTERS:
                t = f"reduce {name} W={w} H={h} images={images}/{2 * maxp} offset {off}"
                od = out((images, ch, cw), torch.uint8, (off * 2) % 4, 2 * maxp, "dst")
                bad += twice(t, lambda r: lib.sm_reduce_half(plan.h, P(gi.t), FILTER[name], images, P(od.t), s), [od], [gi])
                bad += expect(t, od, np.stack([pr.reduce_half(img, name) for img in src]))
        plan.close()
    report(bad)


@pytest.mark.parametrize("dtype", DTYPES)
def test_upsample_writes_its_map_and_nothing_else(dtype):
    bad = []
    td, ty = TORCH[dtype], TYPE[dtype]
    odd = 4 if dtype is np.int32 else 2
    table = pp.guide_weights(8)
    weights = capi.w256(table)
    for idx, (w, h) in enumerate([(33, 17), (64, 16), (130, 35), (1, 5)]):
        pairs, maxp = (2, 3) if idx % 2 == 0 else (1, 2)
        cw, ch = pr.half_shape(w, h)
        plan = Plan(w, h, 4, 1, "toroidal", maxp)
        maps = np.stack([pp.random_map(cw, ch, dtype, 9 * idx + q, 0.3, 6, True) for q in range(pairs)])
        guides = np.stack([pp.random_guide(w, h, 9 * idx + q) for q in range(pairs)])
        coarse = np.stack([pr.reduce_half(g, "binomial") for g in guides])
        s = stream()
        for off in (0, odd):
            gi = guarded_input(maps, "cuda", off, "in")
            gg = guarded_input(guides, "cuda", (1, 3)[idx % 2] if off else 0, "guide")
            gc = guarded_input(coarse, "cuda", (3, 1)[idx % 2] if off else 0, "guide_coarse")
            for fill in (0, capi.SM_UP_FILL):
                t = f"upsample {np.dtype(dtype).name} W={w} H={h} pairs={pairs}/{maxp} flags={fill} offset {off}"
                om = out((pairs, h, w), td, odd - off, maxp, "out")
                bad += twice(t, lambda r: lib.sm_upsample_double(plan.h, P(gi.t), ty, P(gg.t), P(gc.t), weights, fill, pairs,
                                                                 P(om.t), s), [om], [gi, gg, gc])
                bad += expect(t, om, np.stack([pr.upsample_double(m, g, c, table, bool(fill))
                                               for m, g, c in zip(maps, guides, coarse)]))
        plan.close()
    report(bad)


# ---------------------------------------------------------------------------
# capture, the chain, arguments
# ---------------------------------------------------------------------------

def test_captured_into_a_graph(hip):
    """no workspace, no copy: both calls captured as they are; the replays use the weight table of capture time,
    whatever the host array holds by then"""
    w, h = 200, 90
    cw, ch = pr.half_shape(w, h)
    guides = [pp.random_guide(w, h, 40 + i) for i in range(2)]
    maps = [pp.random_map(cw, ch, np.int32, 40 + i, 0.3, 2000, True) for i in range(2)]
    table = pp.guide_weights(8)
    weights = capi.w256(table)
    plan = plan_for(hip, w, h, 1)
    try:
        base = plan.workspace_bytes()
        src = torch.zeros((1, ch, cw), dtype=torch.int32, device="cuda")
        gsrc = torch.zeros((1, h, w), dtype=torch.uint8, device="cuda")
        gco = torch.zeros((1, ch, cw), dtype=torch.uint8, device="cuda")
        res = torch.zeros((1, h, w), dtype=torch.int32, device="cuda")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            capi.check(lib.sm_reduce_half(plan._h, P(gsrc), capi.SM_REDUCE_BINOMIAL, 1, P(gco), plan._stream()))
            capi.check(lib.sm_upsample_double(plan._h, P(src), capi.SM_MAP_I32, P(gsrc), P(gco), weights, capi.SM_UP_FILL, 1,
                                              P(res), plan._stream()))
        for i in range(256):
            weights[i] = 1                                            # the host's table changes after the capture
        assert plan.workspace_bytes() == base
        seen = []
        for rep in (0, 0, 1):                                         # the same input twice, then another
            src.copy_(dev(maps[rep])[None])
            gsrc.copy_(dev(guides[rep])[None])
            res.zero_()
            gco.zero_()
            g.replay()
            torch.cuda.synchronize()
            small = pr.reduce_half(guides[rep], "binomial")
            assert np.array_equal(host(gco)[0], small), rep
            assert np.array_equal(host(res)[0], pr.upsample_double(maps[rep], guides[rep], small, table, True)), rep
            seen.append(host(res).copy())
        assert np.array_equal(seen[0], seen[1])
        ones = pr.upsample_double(maps[0], guides[0], pr.reduce_half(guides[0], "binomial"), np.ones(256, np.uint16), True)
        assert not np.array_equal(seen[0][0], ones)
    finally:
        plan.close()


def test_the_chain_on_a_small_pair(hip):
    """reduce both sides -> census_wta on a plan of the coarse size with half the shifts -> upsample: every stage's
    expectation from its numpy definition, fed with the stage before's expectation"""
    w, h, d, n, census = 70, 38, 16, 5, 5
    left, right = make_pair(w, h, d, seed=11)
    cw, ch = pr.half_shape(w, h)
    fine, coarse = hip.StereoPlan(w, h, d, n, "ghost"), hip.StereoPlan(cw, ch, d // 2, n, "ghost")
    try:
        small = host(fine.reduce_half(dev(np.stack([left, right]))))
        want_small = np.stack([pr.reduce_half(left, "binomial"), pr.reduce_half(right, "binomial")])
        assert np.array_equal(small, want_small)
        web, _ = coarse.census_wta(dev(want_small[0:1]), dev(want_small[1:2]), census=census)
        want_web = cr.wta(want_small[0], want_small[1], d // 2, n, census, "ghost")[1]
        assert np.array_equal(host(web)[0], want_web)
        weights = pp.guide_weights(8)
        for fill in (False, True):
            up = fine.upsample_double(dev(want_web[None]), dev(left[None]), dev(want_small[0:1]), weights, fill=fill)
            want_up = pr.upsample_double(want_web.astype(np.int32), left, want_small[0], weights, fill)
            assert np.array_equal(host(up)[0], want_up), fill
        assert (want_up != 0).any() and int(want_up.max()) <= 2 * (d // 2) - 1
    finally:
        fine.close()
        coarse.close()


def test_argument_checks_on_a_plan(hip):
    w, h = 64, 32
    cw, ch = pr.half_shape(w, h)
    plan = plan_for(hip, w, h, 2)
    base = plan.workspace_bytes()
    big = [torch.full((2 * h * w,), 77, dtype=torch.int32, device="cuda") for _ in range(2)]       # 16 KiB each
    guide = torch.zeros((2, h, w), dtype=torch.uint8, device="cuda")
    gco = torch.zeros((2, ch, cw), dtype=torch.uint8, device="cuda")
    at = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    I32, I16 = capi.SM_MAP_I32, capi.SM_MAP_I16
    wt = capi.w256(pp.guide_weights(8))
    zero = capi.w256([9] * 200 + [0] + [9] * 55)

    def refused(rc, text):
        assert rc == capi.SM_ERR_ARG and text in lib.sm_last_error(), lib.sm_last_error()
        torch.cuda.synchronize()
        assert bool((big[0] == 77).all()) and bool((big[1] == 77).all())      # nothing was written
    me = b"sm_reduce_half: "
    refused(lib.sm_reduce_half(plan._h, at(guide), 0, 0, at(big[1]), st), me + b"images 0 outside 1..4")
    refused(lib.sm_reduce_half(plan._h, at(guide), 0, 5, at(big[1]), st), me + b"images 5 outside 1..4")
    refused(lib.sm_reduce_half(plan._h, at(guide), 2, 1, at(big[1]), st), me + b"filter 2 is neither")
    refused(lib.sm_reduce_half(plan._h, None, 0, 1, at(big[1]), st), me + b"an image pointer is NULL")
    refused(lib.sm_reduce_half(plan._h, at(big[0]), 0, 1, at(big[0]), st), me + b"images overlap")
    refused(lib.sm_reduce_half(plan._h, at(big[0]), 1, 1, at(big[0], h * w - 1), st), me + b"images overlap")
    refused(lib.sm_reduce_half(plan._h, at(big[0], ch * cw - 1), 1, 1, at(big[0]), st), me + b"images overlap")
    refused(lib.sm_reduce_half(plan._h, at(big[0]), 1, 2, at(big[0], 2 * h * w - 1), st), me + b"images overlap")
    me = b"sm_upsample_double: "
    up = lambda *a: lib.sm_upsample_double(plan._h, *a, st)
    refused(up(at(big[0]), I32, at(guide), at(gco), wt, 0, 0, at(big[1])), me + b"pairs 0 outside 1..2")
    refused(up(at(big[0]), I32, at(guide), at(gco), wt, 0, 3, at(big[1])), me + b"pairs 3 outside 1..2")
    refused(up(at(big[0]), 5, at(guide), at(gco), wt, 0, 1, at(big[1])), me + b"map_type 5")
    refused(up(at(big[0]), I32, at(guide), at(gco), wt, 2, 1, at(big[1])), me + b"flags 0x2")
    refused(up(at(big[0]), I32, at(guide), at(gco), wt, 3, 1, at(big[1])), me + b"flags 0x3")
    refused(up(at(big[0]), I32, at(guide), at(gco), zero, 0, 1, at(big[1])), me + b"weights[200] is 0")
    refused(up(at(big[0]), I32, at(guide), at(gco), None, 0, 1, at(big[1])), me + b"weights is NULL")
    refused(up(at(big[0]), I32, None, at(gco), wt, 0, 1, at(big[1])), me + b"a guide pointer is NULL")
    refused(up(at(big[0]), I32, at(guide), None, wt, 0, 1, at(big[1])), me + b"a guide pointer is NULL")
    refused(up(at(big[0]), I32, at(guide), at(gco), wt, 0, 1, None), me + b"a map pointer is NULL")
    refused(up(at(big[0]), I32, at(guide), at(gco), wt, 0, 1, at(big[0])), me + b"maps overlap")
    refused(up(at(big[0], 4 * h * w - 4), I32, at(guide), at(gco), wt, 0, 1, at(big[0])), me + b"maps overlap")
    refused(up(at(big[0]), I16, at(guide), at(gco), wt, 0, 1, at(big[0], 2 * ch * cw - 2)), me + b"maps overlap")
    refused(up(at(big[0]), I32, at(big[1], 4 * h * w - 1), at(gco), wt, 0, 1, at(big[1])), me + b"a guide overlaps the output map")
    refused(up(at(big[0]), I32, at(guide), at(big[1], 4 * h * w - 1), wt, 0, 1, at(big[1])), me + b"a guide overlaps the output map")
    refused(up(at(big[0]), I16, at(guide), at(big[1]), wt, 0, 2, at(big[1], ch * cw * 2 - 2)), me + b"a guide overlaps the output map")
    assert plan.workspace_bytes() == base
    m = torch.ones((1, ch, cw), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="filter"):
        plan.reduce_half(guide, "gauss")
    with pytest.raises(ValueError, match=r"shape .* is not \(pairs, 16, 32\)"):
        plan.upsample_double(torch.ones((1, h, w), dtype=torch.int32, device="cuda"), guide[:1], gco[:1], pp.guide_weights(8))
    with pytest.raises(ValueError, match="int32 .* or int16"):
        plan.upsample_double(gco[:1], guide[:1], gco[:1], pp.guide_weights(8))
    with pytest.raises(ValueError, match="images for 1 pairs"):
        plan.upsample_double(m, guide, gco[:1], pp.guide_weights(8))
    with pytest.raises(capi.StereoHipError, match=r"sm_upsample_double: weights\[255\] is 0"):
        plan.upsample_double(m, guide[:1], gco[:1], [1] * 255 + [0])
    plan.close()
