"""The disparity post-filters on the GPU: sm_median_filter, sm_speckle_filter, sm_sub_mask and sm_plan_reserve_filter
against the numpy definition (tests/filter_reference.py).  Every expected value comes from the CPU definitions; none
from the HIP path.  The kernels work on 64 x 16 tiles (filter_patterns.TILE_W / TILE_H): the sizes below sit on and
around those edges."""
import ctypes as C

import numpy as np
import pytest
import torch

from stereomatching_amd import capi
from stereomatching_amd.capi import lib
from stereomatching_amd.synth import make_pair
from tests import filter_patterns as fp
from tests import filter_reference as fr
from tests import oracle
from tests import sgm_reference as sr
from tests.guarded import guarded_input
from tests.test_write_bounds_gpu import P, Plan, expect, out, report, stream, twice

pytestmark = pytest.mark.gpu
DTYPES = [np.int32, np.int16]
TORCH = {np.int32: torch.int32, np.int16: torch.int16}
TYPE = {np.int32: capi.SM_MAP_I32, np.int16: capi.SM_MAP_I16}
# widths and heights on and around every tile edge (64, 128; 16, 32), and 1 and 2
SIZES = [(1, 1), (1, 40), (70, 1), (2, 2), (63, 15), (64, 16), (65, 17), (127, 31), (128, 32), (129, 33), (200, 50),
         (66, 2), (3, 70)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def plan_for(hip, w, h, max_pairs=1):
    """the filters read W, H and max_pairs of the plan only; the window must fit the image"""
    return hip.StereoPlan(w, h, 4, 1, "ghost", max_pairs=max_pairs)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [3, 5])
def test_median_random_maps(hip, dtype, k):
    for i, (w, h) in enumerate(SIZES):
        for pairs, maxp in ((2, 2), (1, 3)):                          # a full and a partial batch
            invalid = (0.0, 0.3, 0.7, 0.95)[(i + pairs) % 4]
            maps = np.stack([fp.random_map(w, h, dtype, 50 * i + q + k, invalid, 1, (6, 2000)[i % 2], negative=i % 3 == 0)
                             for q in range(pairs)])
            plan = plan_for(hip, w, h, maxp)
            try:
                got = host(plan.median_filter(dev(maps), k))
            finally:
                plan.close()
            for q in range(pairs):
                assert np.array_equal(got[q], fr.median(maps[q], k)), (w, h, pairs, maxp, q)


@pytest.mark.parametrize("dtype", DTYPES)
def test_speckle_random_maps(hip, dtype):
    for i, (w, h) in enumerate(SIZES):
        for pairs, maxp in ((2, 2), (1, 3)):
            invalid = (0.0, 0.2, 0.45, 0.8)[(i + pairs) % 4]
            max_size, max_diff = (0, 2, 5, 30)[i % 4], (0, 1, 2)[(i + pairs) % 3]
            maps = np.stack([fp.random_map(w, h, dtype, 31 * i + q, invalid, 1, 5, negative=i % 2 == 0)
                             for q in range(pairs)])
            plan = plan_for(hip, w, h, maxp)
            try:
                got, removed = plan.speckle_filter(dev(maps), max_size, max_diff, want_removed=True)
                got, removed = host(got), host(removed)
            finally:
                plan.close()
            for q in range(pairs):
                want, n = fr.speckle(maps[q], max_size, max_diff)
                assert np.array_equal(got[q], want), (w, h, pairs, maxp, q)
                assert int(removed[q]) == n, (w, h, pairs, maxp, q)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(fp.PATTERNS))
def test_speckle_component_shapes(hip, name, dtype):
    """shapes that stress the merge of tile borders, each across many tiles; two pairs: the pattern and its transpose
    laid into the same frame would need another plan, so the second pair is the pattern flipped both ways"""
    w, h = 457, 211
    a, max_size, max_diff = fp.PATTERNS[name](w, h, dtype)
    fp.informative(a, max_size, max_diff)
    maps = np.stack([a, a[::-1, ::-1]])
    plan = plan_for(hip, w, h, 2)
    try:
        got, removed = plan.speckle_filter(dev(maps), max_size, max_diff, want_removed=True)
        for q in range(2):
            want, n = fr.speckle(maps[q], max_size, max_diff)
            assert 0 < n < int((maps[q] != 0).sum())
            assert np.array_equal(host(got)[q], want), (name, q)
            assert int(removed[q]) == n, (name, q)
        # ... and the median of the same maps
        for k in (3, 5):
            med = host(plan.median_filter(dev(maps), k))
            assert np.array_equal(med[0], fr.median(maps[0], k)), (name, k)
    finally:
        plan.close()


def test_speckle_one_component_over_a_4k_map(hip):
    w, h = 3840, 2160
    a, max_size, max_diff = fp.whole(w, h, np.int32)
    sizes = fp.informative(a, max_size, max_diff)
    assert max(sizes.values()) == w * h - 5 * 9
    want, n = fr.speckle(a, max_size, max_diff)
    assert n == 5
    plan = plan_for(hip, w, h)
    try:
        got, removed = plan.speckle_filter(dev(a), max_size, max_diff, want_removed=True)
        assert np.array_equal(host(got)[0], want)
        assert int(removed[0]) == n
        # the serpentine at full size: a path of four million pixels through every tile
        b, max_size, max_diff = fp.serpentine(w, h, np.int32)
        want, n = fr.speckle(b, max_size, max_diff)
        got, removed = plan.speckle_filter(dev(b), max_size, max_diff, want_removed=True)
        assert np.array_equal(host(got)[0], want)
        assert int(removed[0]) == n and n > 0
        # ... and the 3 x 3 median of a 4K int16 map, the shape the timing tool measures
        c = fp.random_map(w, h, np.int16, 4, 0.25, 1, 3000, negative=True)
        assert np.array_equal(host(plan.median_filter(dev(c), 3))[0], fr.median(c, 3))
    finally:
        plan.close()


def test_value_extremes(hip):
    """int32 maps with values up to 65535 (and the ends of the type), int16 maps at -32768 / 32767"""
    w, h = 131, 37
    rng = np.random.default_rng(8)
    cases = [(np.int32, np.array([0, 1, 65535, 65534, 40000], np.int32)),
             (np.int32, np.array([0, -2**31, 2**31 - 1, -1, 1], np.int32)),
             (np.int16, np.array([0, -32768, 32767, -32767, 32766], np.int16)),
             (np.int16, np.array([-32768, 32767], np.int16))]
    for dtype, values in cases:
        a = rng.choice(values, (h, w))
        plan = plan_for(hip, w, h)
        try:
            for k in (3, 5):
                assert np.array_equal(host(plan.median_filter(dev(a), k))[0], fr.median(a, k)), (dtype, k)
            for max_size, max_diff in ((2, 0), (4, 1), (3, 65535), (6, 2**31 - 1)):
                got, removed = plan.speckle_filter(dev(a), max_size, max_diff, want_removed=True)
                want, n = fr.speckle(a, max_size, max_diff)
                assert np.array_equal(host(got)[0], want), (dtype, max_size, max_diff)
                assert int(removed[0]) == n
        finally:
            plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_identities_on_the_gpu(hip, dtype):
    w, h = 150, 40
    a = fp.random_map(w, h, dtype, 3, 0.3, 1, 5, negative=True)
    plan = plan_for(hip, w, h)
    try:
        const = np.full((h, w), -9, dtype)
        assert np.array_equal(host(plan.median_filter(dev(const), 5))[0], const)
        zero = np.zeros((h, w), dtype)
        assert not host(plan.median_filter(dev(zero), 3)).any()
        kept, removed = plan.speckle_filter(dev(a), 0, 1, want_removed=True)
        assert np.array_equal(host(kept)[0], a) and int(removed[0]) == 0
        gone, removed = plan.speckle_filter(dev(a), w * h, 1, want_removed=True)
        assert not host(gone).any() and int(removed[0]) == int((a != 0).sum())
        none, removed = plan.speckle_filter(dev(zero), 3, 1, want_removed=True)
        assert not host(none).any() and int(removed[0]) == 0
        once = plan.speckle_filter(dev(a), 6, 1)
        assert torch.equal(plan.speckle_filter(once, 6, 1), once)
    finally:
        plan.close()


# ---------------------------------------------------------------------------
# write bounds (tests/guarded.py)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_filters_write_their_maps_and_nothing_else(dtype):
    bad = []
    td, ty = TORCH[dtype], TYPE[dtype]
    odd = 4 if dtype is np.int32 else 2
    for idx, (w, h) in enumerate([(33, 17), (64, 16), (130, 35), (1, 5)]):
        pairs, maxp = (2, 3) if idx % 2 == 0 else (1, 2)
        plan = Plan(w, h, 4, 1, "toroidal", maxp)
        maps = np.stack([fp.random_map(w, h, dtype, 9 * idx + q, 0.3, 1, 5, negative=True) for q in range(pairs)])
        shp, s = (pairs, h, w), stream()
        tag = f"{np.dtype(dtype).name} W={w} H={h} pairs={pairs}/{maxp}"
        for off in (0, odd):
            gi = guarded_input(maps, "cuda", off, "in")
            for k in (3, 5):
                t = f"{tag} sm_median_filter k={k} offset {off}"
                om = out(shp, td, odd - off, maxp, "out")
                bad += twice(t, lambda r: lib.sm_median_filter(plan.h, P(gi.t), ty, k, pairs, P(om.t), s), [om], [gi])
                bad += expect(t, om, np.stack([fr.median(m, k) for m in maps]))
            want = [fr.speckle(m, 4, 1) for m in maps]
            t = f"{tag} sm_speckle_filter offset {off}"
            osp, orm = out(shp, td, off, maxp, "out"), out((pairs,), torch.int32, off and 4, maxp, "removed")
            bad += twice(t, lambda r: lib.sm_speckle_filter(plan.h, P(gi.t), ty, 4, 1, pairs, P(osp.t), P(orm.t), s),
                         [osp, orm], [gi])
            bad += expect(t, osp, np.stack([x[0] for x in want])) + expect(t, orm, [x[1] for x in want])
            t = f"{tag} sm_speckle_filter (no count) offset {off}"
            osp = out(shp, td, odd - off, maxp, "out")
            bad += twice(t, lambda r: lib.sm_speckle_filter(plan.h, P(gi.t), ty, 4, 1, pairs, P(osp.t), None, s), [osp],
                         [gi])
            bad += expect(t, osp, np.stack([x[0] for x in want]))
            # in place: the map is input and output; its guards must hold and every pixel be the definition's
            t = f"{tag} sm_speckle_filter in place offset {off}"
            oip = out(shp, td, off, maxp, "map")
            oip.fill(0)
            oip.t.copy_(dev(maps))
            rc = lib.sm_speckle_filter(plan.h, P(oip.t), ty, 4, 1, pairs, P(oip.t), None, s)
            torch.cuda.synchronize()
            if rc != capi.SM_OK:
                bad.append(f"{t}: returned {rc}: {lib.sm_last_error().decode(errors='replace')}")
            bad += [f"{t}: {p}" for p in oip._guard_problems(0)] + expect(t, oip, np.stack([x[0] for x in want]))
        if dtype is np.int16:
            web = np.stack([fp.random_map(w, h, np.int32, idx + q, 0.5, 1, 9) for q in range(pairs)])
            t = f"{tag} sm_sub_mask"
            gw = guarded_input(web, "cuda", 4, "web")
            osb = out(shp, torch.int16, 2, maxp, "sub")
            osb.fill(0)
            osb.t.copy_(dev(maps))
            rc = lib.sm_sub_mask(plan.h, P(gw.t), P(osb.t), pairs, s)
            torch.cuda.synchronize()
            if rc != capi.SM_OK:
                bad.append(f"{t}: returned {rc}: {lib.sm_last_error().decode(errors='replace')}")
            bad += [f"{t}: {p}" for p in osb._guard_problems(0) + gw.problems()]
            bad += expect(t, osb, np.where(web == 0, 0, maps))
        plan.close()
    report(bad)


# ---------------------------------------------------------------------------
# arguments, workspace, capture
# ---------------------------------------------------------------------------

def test_argument_checks_on_a_plan(hip):
    w, h = 64, 32
    plan = plan_for(hip, w, h, 2)
    base = plan.workspace_bytes()
    m = [torch.zeros((2, h, w), dtype=torch.int32, device="cuda") for _ in range(2)]
    p = [C.c_void_p(t.data_ptr()) for t in m]
    sub = torch.zeros((2, h, w), dtype=torch.int16, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    inside = C.c_void_p(m[0].data_ptr() + 4)
    I32, I16 = capi.SM_MAP_I32, capi.SM_MAP_I16

    def refused(rc, text):
        assert rc == capi.SM_ERR_ARG and text in lib.sm_last_error(), lib.sm_last_error()
    refused(lib.sm_median_filter(plan._h, p[0], I32, 3, 3, p[1], st), b"sm_median_filter: pairs 3 outside 1..2")
    refused(lib.sm_median_filter(plan._h, p[0], I32, 3, 0, p[1], st), b"sm_median_filter: pairs 0 outside 1..2")
    refused(lib.sm_median_filter(plan._h, p[0], I32, 4, 1, p[1], st), b"sm_median_filter: k 4 is not 3 or 5")
    refused(lib.sm_median_filter(plan._h, p[0], 2, 3, 1, p[1], st), b"sm_median_filter: map_type 2")
    refused(lib.sm_median_filter(plan._h, None, I32, 3, 1, p[1], st), b"sm_median_filter: a map pointer is NULL")
    refused(lib.sm_median_filter(plan._h, p[0], I32, 3, 1, None, st), b"sm_median_filter: a map pointer is NULL")
    refused(lib.sm_median_filter(plan._h, p[0], I32, 3, 1, p[0], st), b"sm_median_filter: maps overlap")
    refused(lib.sm_median_filter(plan._h, p[0], I16, 5, 1, inside, st), b"sm_median_filter: maps overlap")
    refused(lib.sm_median_filter(None, p[0], I32, 3, 1, p[1], st), b"sm_median_filter: plan is NULL")
    refused(lib.sm_speckle_filter(plan._h, p[0], I32, 5, 1, 3, p[1], None, st), b"sm_speckle_filter: pairs 3 outside 1..2")
    refused(lib.sm_speckle_filter(plan._h, p[0], -1, 5, 1, 1, p[1], None, st), b"sm_speckle_filter: map_type -1")
    refused(lib.sm_speckle_filter(plan._h, p[0], I32, -1, 1, 1, p[1], None, st),
            b"sm_speckle_filter: max_size -1 is negative")
    refused(lib.sm_speckle_filter(plan._h, p[0], I32, 5, -3, 1, p[1], None, st),
            b"sm_speckle_filter: max_diff -3 is negative")
    refused(lib.sm_speckle_filter(plan._h, None, I32, 5, 1, 1, p[1], None, st), b"sm_speckle_filter: a map pointer is NULL")
    refused(lib.sm_speckle_filter(plan._h, p[0], I32, 5, 1, 1, inside, None, st), b"sm_speckle_filter: maps overlap")
    refused(lib.sm_speckle_filter(plan._h, p[0], I32, 5, 1, 2, p[1], inside, st),
            b"sm_speckle_filter: d_removed overlaps a map")
    refused(lib.sm_speckle_filter(plan._h, p[0], I32, 5, 1, 2, p[0], C.c_void_p(m[0].data_ptr() + 8), st),
            b"sm_speckle_filter: d_removed overlaps a map")
    refused(lib.sm_speckle_filter(None, p[0], I32, 5, 1, 1, p[1], None, st), b"sm_speckle_filter: plan is NULL")
    refused(lib.sm_sub_mask(plan._h, p[0], C.c_void_p(sub.data_ptr()), 3, st), b"sm_sub_mask: pairs 3 outside 1..2")
    refused(lib.sm_sub_mask(plan._h, None, C.c_void_p(sub.data_ptr()), 1, st), b"sm_sub_mask: a map pointer is NULL")
    refused(lib.sm_sub_mask(plan._h, p[0], C.c_void_p(m[0].data_ptr() + 2), 1, st), b"sm_sub_mask: maps overlap")
    refused(lib.sm_plan_reserve_filter(None), b"sm_plan_reserve_filter: plan is NULL")
    assert plan.workspace_bytes() == base
    with pytest.raises(ValueError, match="int32 .* or int16"):
        plan.median_filter(torch.zeros((1, h, w), dtype=torch.uint8, device="cuda"))
    plan.close()


def test_workspace_is_allocated_only_for_the_speckle_filter(hip):
    w, h, mp = 300, 150, 2
    a = fp.random_map(w, h, np.int32, 1, 0.3)
    need = 8 * mp * w * h
    plan = plan_for(hip, w, h, mp)
    base, describe = plan.workspace_bytes(), plan.describe()
    plan.median_filter(dev(a), 3)
    plan.median_filter(dev(a.astype(np.int16)), 5)
    plan.sub_mask(dev(a), dev(a.astype(np.int16)))
    torch.cuda.synchronize()
    assert plan.workspace_bytes() == base                      # the median and the mask allocate nothing
    plan.reserve_filter()
    plan.reserve_filter()                                       # idempotent
    assert plan.workspace_bytes() == base + need
    assert plan.describe() == describe
    plan.speckle_filter(dev(a), 5, 1)
    assert plan.workspace_bytes() == base + need
    plan.close()
    plan = plan_for(hip, w, h, mp)                              # the first call allocates
    got = plan.speckle_filter(dev(a), 5, 1)
    assert plan.workspace_bytes() == base + need
    assert np.array_equal(host(got)[0], fr.speckle(a, 5, 1)[0])
    plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_filters_captured_into_a_graph(hip, dtype):
    w, h = 200, 90
    maps = [fp.random_map(w, h, dtype, 40 + i, 0.3, 1, 5, negative=True) for i in range(3)]
    plan = plan_for(hip, w, h)
    try:
        base = plan.workspace_bytes()
        src = torch.zeros((1, h, w), dtype=TORCH[dtype], device="cuda")
        spk, med = torch.zeros_like(src), torch.zeros_like(src)
        rem = torch.zeros(1, dtype=torch.int32, device="cuda")
        with pytest.raises(capi.StereoHipError, match="sm_plan_reserve_filter"):
            with torch.cuda.graph(torch.cuda.CUDAGraph(), capture_error_mode="thread_local"):
                plan.speckle_filter(src, 4, 1, out=spk)
        assert plan.workspace_bytes() == base
        # the capture stayed valid in the library's eyes: the median needs no reservation and is captured as it is
        g0 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g0, capture_error_mode="thread_local"):
            plan.median_filter(src, 3, out=med)
        src.copy_(dev(maps[0])[None])
        g0.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(med)[0], fr.median(maps[0], 3))
        assert plan.workspace_bytes() == base
        plan.reserve_filter()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            capi.check(lib.sm_speckle_filter(plan._h, P(src), TYPE[dtype], 4, 1, 1, P(spk), P(rem), plan._stream()))
            capi.check(lib.sm_median_filter(plan._h, P(spk), TYPE[dtype], 5, 1, P(med), plan._stream()))
        for rep, a in enumerate(maps[1:] + maps[:1]):
            src.copy_(dev(a)[None])
            spk.zero_()
            med.zero_()
            rem.fill_(12345)
            g.replay()
            torch.cuda.synchronize()
            want, n = fr.speckle(a, 4, 1)
            assert np.array_equal(host(spk)[0], want), rep
            assert int(rem[0]) == n, rep
            assert np.array_equal(host(med)[0], fr.median(want, 5)), rep
    finally:
        plan.close()


# ---------------------------------------------------------------------------
# the chain: cost -> check -> speckle / median -> hole filling
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode,w,h,d,sw,census,times", [("toroidal", 160, 64, 48, 3, 7, 4), ("ghost", 120, 50, 30, 5, 5, 1)])
def test_sgm_lr_through_the_filters_and_step3(hip, mode, w, h, d, sw, census, times):
    left, right = make_pair(w, h, d, seed=9)
    e = sr.expected(left, right, d, sw, census, 10, 120, 8, mode, 0)
    max_size, max_diff = 12, 1
    web, removed = fr.speckle(e["checked"], max_size, max_diff)
    assert removed > 0 and web.any()                              # the definition removes a component of this scene
    sub = np.where(web == 0, 0, e["sub_checked"]).astype(np.int16)
    sub_med = fr.median(sub, 3)
    filled = oracle.fill_web_holes(web, times)
    contour = oracle.draw_contour_map(filled, 5)
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        res = plan.sgm_lr(dev(left), dev(right), census, 10, 120, 8, max_diff=0, want_sub=True)
        assert np.array_equal(host(res.web)[0], e["checked"])
        got_web, got_removed = plan.speckle_filter(res.web, max_size, max_diff, out=res.web, want_removed=True)
        assert got_web is res.web and np.array_equal(host(got_web)[0], web) and int(got_removed[0]) == removed
        got_sub = plan.sub_mask(got_web, res.sub)
        assert np.array_equal(host(got_sub)[0], sub)
        assert np.array_equal(host(plan.median_filter(got_sub, 3))[0], sub_med)
        f, c, mm = plan.step3(got_web, times, 5)
        assert np.array_equal(host(f)[0], filled)
        assert np.array_equal(host(c)[0], contour)
        assert host(mm)[0].tolist() == [int(filled.min()), int(filled.max())]
    finally:
        plan.close()
