"""Occlusion-aware interpolation on the GPU: sm_occlusion_classify, sm_interpolate and sm_plan_reserve_interp against
the numpy definition (tests/interp_reference.py).  Every expected value comes from the CPU definitions; none from the
HIP path; every comparison is bit for bit.  The sweeps work on segments of 64 rows and chunks of 64 pixels
(interp_patterns.SEG_H / CHUNK_W): the sizes sit on and around those edges and the post-filters' tile edges."""
import ctypes as C

import numpy as np
import pytest
import torch

from stereomatching_amd import capi
from stereomatching_amd.capi import lib
from stereomatching_amd.synth import make_pair
from tests import filter_reference as fr
from tests import interp_patterns as ip
from tests import interp_reference as ir
from tests import sgm_reference as sr
from tests.guarded import guarded_input
from tests.test_filter_gpu import SIZES as FILTER_SIZES
from tests.test_write_bounds_gpu import P, Plan, expect, out, report, stream, twice

pytestmark = pytest.mark.gpu
DTYPES = [np.int32, np.int16]
TORCH = {np.int32: torch.int32, np.int16: torch.int16}
TYPE = {np.int32: capi.SM_MAP_I32, np.int16: capi.SM_MAP_I16}
SIZES = FILTER_SIZES + ip.SIZES
INVALID = (0.0, 0.3, 0.7, 0.95, 1.0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def plan_for(hip, w, h, max_pairs=1, d=4, mode="ghost"):
    """interpolation reads W, H and max_pairs of the plan only, classification also D and the border; the window
    (1) fits every image"""
    return hip.StereoPlan(w, h, d, 1, mode, max_pairs=max_pairs)


def check_interpolate(plan, maps, cls, tag):
    """maps [pairs][H][W], cls None or [pairs][H][W] -> asserts the map and the count of every pair"""
    got, filled = plan.interpolate(dev(maps), None if cls is None else dev(cls), want_filled=True)
    got, filled = host(got), host(filled)
    for q in range(maps.shape[0]):
        want = ir.interpolate(maps[q], None if cls is None else cls[q])
        assert np.array_equal(got[q], want), (tag, q, np.argwhere(got[q] != want)[:4].tolist())
        assert int(filled[q]) == ir.filled(maps[q], want) == int((got[q] != maps[q]).sum()), (tag, q)


@pytest.mark.parametrize("dtype", DTYPES)
def test_interpolate_random_maps(hip, dtype):
    for i, (w, h) in enumerate(SIZES):
        for pairs, maxp in ((2, 2), (1, 3)):                          # a full and a partial batch
            for j, invalid in enumerate(INVALID):
                maps = np.stack([ip.random_map(w, h, dtype, 50 * i + 7 * j + q, invalid, 1, (6, 2000)[i % 2],
                                               negative=i % 3 == 0) for q in range(pairs)])
                kind = (i + j + pairs) % 3                            # cls NULL / random / all 1
                cls = None if kind == 0 else np.stack([ip.random_class(w, h, i + q, ones=kind == 2)
                                                       for q in range(pairs)])
                plan = plan_for(hip, w, h, maxp)
                try:
                    check_interpolate(plan, maps, cls, (w, h, pairs, maxp, invalid, kind))
                finally:
                    plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(ip.PATTERNS))
def test_interpolate_structured_holes(hip, name, dtype):
    """holes that cross every segment and chunk border; the second pair is the pattern flipped both ways"""
    for w, h in ((457, 211), (130, 200)):
        a = ip.PATTERNS[name](w, h, dtype)
        ip.informative(name, a)
        maps = np.stack([a, a[::-1, ::-1]])
        plan = plan_for(hip, w, h, 2)
        try:
            check_interpolate(plan, maps, None, (name, "median"))
            check_interpolate(plan, maps, np.ones(maps.shape, np.uint8), (name, "occluded"))
            check_interpolate(plan, maps, np.stack([ip.random_class(w, h, 3), ip.random_class(w, h, 4)]), (name, "mixed"))
        finally:
            plan.close()


def test_interpolate_lone_and_band_at_4k(hip):
    w, h = 3840, 2160
    plan = plan_for(hip, w, h)
    try:
        for name, dtype in (("lone", np.int32), ("band_v", np.int16), ("band_v", np.int32)):
            a = ip.PATTERNS[name](w, h, dtype)
            want = ir.interpolate(a)
            # the band is filled whole; the lone pixel reaches its row, its column and its diagonal
            assert ir.filled(a, want) == (int((a == 0).sum()) if name == "band_v" else w - 1 + h - 1 + min(w, h) - 1)
            got, filled = plan.interpolate(dev(a), want_filled=True)
            assert np.array_equal(host(got)[0], want), name
            assert int(filled[0]) == ir.filled(a, want)
        # the lone pixel in the other three corners, with every pixel occluded: still that one value or nothing
        a = ip.lone(w, h, np.int32)
        ones = np.ones((h, w), np.uint8)
        for b in (a[::-1], a[:, ::-1], a[::-1, ::-1]):
            got = host(plan.interpolate(dev(b), dev(ones)))[0]
            assert np.array_equal(got, ir.interpolate(b, ones))
    finally:
        plan.close()


def test_value_extremes(hip):
    w, h = 131, 70
    rng = np.random.default_rng(8)
    cases = [(np.int32, np.array([0, 0, 0, -2**31, 2**31 - 1, -1, 1], np.int32)),
             (np.int32, np.array([0, 0, 2**31 - 1], np.int32)),
             (np.int16, np.array([0, 0, 0, -32768, 32767, -32767, 32766], np.int16)),
             (np.int16, np.array([0, -32768, 32767], np.int16))]
    for dtype, values in cases:
        a = rng.choice(values, (1, h, w))
        plan = plan_for(hip, w, h)
        try:
            check_interpolate(plan, a, None, dtype)
            check_interpolate(plan, a, ip.random_class(w, h, 1)[None], dtype)
        finally:
            plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_identities_on_the_gpu(hip, dtype):
    w, h = 150, 90
    plan = plan_for(hip, w, h)
    try:
        full = ip.random_map(w, h, dtype, 3, 0.0, 1, 5, negative=True)
        got, filled = plan.interpolate(dev(full), want_filled=True)
        assert np.array_equal(host(got)[0], full) and int(filled[0]) == 0
        zero = np.zeros((h, w), dtype)
        got, filled = plan.interpolate(dev(zero), dev(np.ones((h, w), np.uint8)), want_filled=True)
        assert not host(got).any() and int(filled[0]) == 0
        a = ip.random_map(w, h, dtype, 4, 0.8, 1, 9, negative=True)
        const = np.where(a != 0, -9, 0).astype(dtype)
        got = host(plan.interpolate(dev(const)))[0]
        assert np.array_equal(got, np.where(ir.candidate_count(a) > 0, -9, const))
        # [H][W] tensors are one pair
        assert np.array_equal(host(plan.interpolate(dev(a)))[0], ir.interpolate(a))
    finally:
        plan.close()


def test_sub_map_follows_the_web_map_on_the_gpu(hip):
    w, h = 200, 130
    rng = np.random.default_rng(2)
    web = ip.random_map(w, h, np.int32, 5, 0.6, 1, 60)
    sub = np.where(web != 0, 16 * web + rng.integers(-8, 9, (h, w)), 0).astype(np.int16)
    cls = ip.random_class(w, h, 6)
    plan = plan_for(hip, w, h)
    try:
        fw, fs = host(plan.interpolate(dev(web), dev(cls)))[0], host(plan.interpolate(dev(sub), dev(cls)))[0]
    finally:
        plan.close()
    assert np.array_equal(fw, ir.interpolate(web, cls)) and np.array_equal(fs, ir.interpolate(sub, cls))
    assert (np.abs(fs.astype(np.int64) - 16 * fw.astype(np.int64)) <= 8).all()


# ---------------------------------------------------------------------------
# classification
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
def test_classify_random_maps(hip, mode):
    rng = np.random.default_rng(4)
    for i, (w, h) in enumerate([(63, 5), (64, 7), (65, 3), (127, 4), (129, 9), (1, 6), (2, 2), (40, 33), (200, 50)]):
        for d in (1, 4, 64, 128, 256):                                # D > W for most of these widths
            pairs, maxp = ((2, 2), (1, 3))[(i + d) % 2]
            web = np.stack([ip.random_map(w, h, np.int32, i + d + q, (0.5, 0.9, 1.0)[(i + q) % 3], 1, d)
                            for q in range(pairs)])
            # values around 1 .. D (0 and D + 1, D + 2 match no d), dense enough that both classes occur
            right = rng.integers(0, d + 3, (pairs, h, w)).astype(np.int32)
            if i % 2:
                right[rng.random(right.shape) < 0.8] = 0
            plan = plan_for(hip, w, h, maxp, d, mode)
            try:
                got = host(plan.occlusion_classify(dev(web), dev(right)))
            finally:
                plan.close()
            assert got.dtype == np.uint8
            for q in range(pairs):
                assert np.array_equal(got[q], ir.classify(web[q], right[q], d, mode)), (w, h, d, q)


def test_classify_across_the_wrap(hip):
    """rows whose only intersection lies across the toroidal wrap: mismatched there, occluded under the ghost border"""
    w, h, d = 70, 4, 16
    web = np.zeros((h, w), np.int32)
    right = np.zeros((h, w), np.int32)
    for y in range(h):
        right[y, y] = 5 + y                                               # met from x = y - (4 + y) = -4 -> W - 4
    for mode in ("toroidal", "ghost"):
        want = ir.classify(web, right, d, mode)
        assert (want == 2).sum() == (h if mode == "toroidal" else 0)
        assert mode == "ghost" or (want[:, w - 4] == 2).all()
        plan = plan_for(hip, w, h, 1, d, mode)
        try:
            assert np.array_equal(host(plan.occlusion_classify(dev(web), dev(right)))[0], want)
        finally:
            plan.close()


# ---------------------------------------------------------------------------
# the chain: sgm_lr -> speckle -> classify -> interpolate (web and sub)
# ---------------------------------------------------------------------------

# chosen on the CPU, with tests/sgm_reference.py alone: (mode, W, H, D, window, census, seed)
CHAIN = [("toroidal", 160, 64, 48, 3, 7, 9), ("ghost", 120, 50, 30, 5, 5, 9)]


def widest_hole(a):
    """the longest horizontal run of invalid pixels"""
    best = 0
    for row in a == 0:
        run = 0
        for v in row:
            run = run + 1 if v else 0
            best = max(best, run)
    return best


@pytest.mark.parametrize("mode,w,h,d,sw,census,seed", CHAIN)
def test_sgm_lr_through_speckle_classify_and_interpolate(hip, mode, w, h, d, sw, census, seed):
    left, right = make_pair(w, h, d, seed=seed)
    e = sr.expected(left, right, d, sw, census, 10, 120, 8, mode, 0)
    web, removed = fr.speckle(e["checked"], 12, 1)
    sub = np.where(web == 0, 0, e["sub_checked"]).astype(np.int16)
    cls = ir.classify(web, e["web_right"], d, mode)
    # the condition on the input, from the definitions alone
    assert (cls == ir.OCCLUDED).sum() >= 50 and (cls == ir.MISMATCHED).sum() >= 50, np.bincount(cls.ravel())
    assert widest_hole(web) > 8
    fweb, fsub = ir.interpolate(web, cls), ir.interpolate(sub, cls)
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        res = plan.sgm_lr(dev(left), dev(right), census, 10, 120, 8, max_diff=0, want_right=True, want_sub=True)
        assert np.array_equal(host(res.web)[0], e["checked"])
        assert np.array_equal(host(res.web_right)[0], e["web_right"])
        got_web, got_removed = plan.speckle_filter(res.web, 12, 1, out=res.web, want_removed=True)
        assert np.array_equal(host(got_web)[0], web) and int(got_removed[0]) == removed
        got_sub = plan.sub_mask(got_web, res.sub)
        assert np.array_equal(host(got_sub)[0], sub)
        got_cls = plan.occlusion_classify(got_web, res.web_right)
        assert np.array_equal(host(got_cls)[0], cls)
        got_fweb, n = plan.interpolate(got_web, got_cls, want_filled=True)
        assert np.array_equal(host(got_fweb)[0], fweb) and int(n[0]) == ir.filled(web, fweb)
        got_fsub = plan.interpolate(got_sub, got_cls)
        assert np.array_equal(host(got_fsub)[0], fsub)
        assert (np.abs(fsub.astype(np.int64) - 16 * fweb.astype(np.int64)) <= 8).all()
    finally:
        plan.close()


# ---------------------------------------------------------------------------
# write bounds (tests/guarded.py)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_interpolation_writes_its_maps_and_nothing_else(dtype):
    bad = []
    td, ty = TORCH[dtype], TYPE[dtype]
    odd = 4 if dtype is np.int32 else 2
    for idx, (w, h) in enumerate([(33, 17), (64, 64), (130, 67), (1, 5), (65, 130)]):
        pairs, maxp = (2, 3) if idx % 2 == 0 else (1, 2)
        d = (4, 70)[idx % 2]
        mode = ("toroidal", "ghost")[idx % 2]
        plan = Plan(w, h, d, 1, mode, maxp)
        maps = np.stack([ip.random_map(w, h, dtype, 9 * idx + q, 0.6, 1, 5, negative=True) for q in range(pairs)])
        cls = np.stack([ip.random_class(w, h, idx + q) for q in range(pairs)])
        shp, s = (pairs, h, w), stream()
        tag = f"{np.dtype(dtype).name} W={w} H={h} pairs={pairs}/{maxp}"
        for off in (0, odd):
            gi, gc = guarded_input(maps, "cuda", off, "in"), guarded_input(cls, "cuda", off and 1, "class")
            want = np.stack([ir.interpolate(m, c) for m, c in zip(maps, cls)])
            t = f"{tag} sm_interpolate offset {off}"
            om, of = out(shp, td, odd - off, maxp, "out"), out((pairs,), torch.int32, off and 4, maxp, "filled")
            bad += twice(t, lambda r: lib.sm_interpolate(plan.h, P(gi.t), ty, P(gc.t), pairs, P(om.t), P(of.t), s),
                         [om, of], [gi, gc])
            bad += expect(t, om, want) + expect(t, of, [ir.filled(m, x) for m, x in zip(maps, want)])
            t = f"{tag} sm_interpolate (no class, no count) offset {off}"
            om = out(shp, td, off, maxp, "out")
            bad += twice(t, lambda r: lib.sm_interpolate(plan.h, P(gi.t), ty, None, pairs, P(om.t), None, s), [om], [gi])
            bad += expect(t, om, np.stack([ir.interpolate(m) for m in maps]))
        if dtype is np.int32:
            rng = np.random.default_rng(idx)
            right = rng.integers(0, d + 2, shp).astype(np.int32)
            for off in (0, 4):
                gw, gr = guarded_input(maps, "cuda", off, "web"), guarded_input(right, "cuda", 4 - off, "web_right")
                t = f"{tag} sm_occlusion_classify offset {off}"
                oc = out(shp, torch.uint8, off and 1, maxp, "class")
                bad += twice(t, lambda r: lib.sm_occlusion_classify(plan.h, P(gw.t), P(gr.t), pairs, P(oc.t), s), [oc],
                             [gw, gr])
                bad += expect(t, oc, np.stack([ir.classify(m, r, d, mode) for m, r in zip(maps, right)]))
        plan.close()
    report(bad)


# ---------------------------------------------------------------------------
# arguments, workspace, capture
# ---------------------------------------------------------------------------

def workspace_need(w, h, max_pairs):
    """the amount include/stereo_hip.h documents"""
    s, c = -(-h // ip.SEG_H), -(-w // ip.CHUNK_W)
    return 4 * max_pairs * (6 * w * h + 6 * s * (w + h - 1) + 2 * h * c)


def test_argument_checks_on_a_plan(hip):
    w, h = 64, 32
    plan = plan_for(hip, w, h, 2)
    base = plan.workspace_bytes()
    m = [torch.full((2, h, w), 77, dtype=torch.int32, device="cuda") for _ in range(3)]
    m[0].zero_()
    p = [C.c_void_p(t.data_ptr()) for t in m]
    cls = torch.full((2, h, w), 9, dtype=torch.uint8, device="cuda")
    cnt = torch.full((2,), 12345, dtype=torch.int32, device="cuda")
    pc, pn = C.c_void_p(cls.data_ptr()), C.c_void_p(cnt.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    inside = C.c_void_p(m[0].data_ptr() + 4)
    I32, I16 = capi.SM_MAP_I32, capi.SM_MAP_I16

    def refused(rc, text):
        assert rc == capi.SM_ERR_ARG and text in lib.sm_last_error(), lib.sm_last_error()
    refused(lib.sm_interpolate(plan._h, p[0], I32, pc, 3, p[1], pn, st), b"sm_interpolate: pairs 3 outside 1..2")
    refused(lib.sm_interpolate(plan._h, p[0], I32, pc, 0, p[1], pn, st), b"sm_interpolate: pairs 0 outside 1..2")
    refused(lib.sm_interpolate(plan._h, p[0], 2, pc, 1, p[1], pn, st), b"sm_interpolate: map_type 2")
    refused(lib.sm_interpolate(plan._h, p[0], -1, None, 1, p[1], pn, st), b"sm_interpolate: map_type -1")
    refused(lib.sm_interpolate(plan._h, None, I32, pc, 1, p[1], pn, st), b"sm_interpolate: a map pointer is NULL")
    refused(lib.sm_interpolate(plan._h, p[0], I32, pc, 1, None, pn, st), b"sm_interpolate: a map pointer is NULL")
    refused(lib.sm_interpolate(plan._h, p[1], I32, pc, 1, p[1], pn, st), b"sm_interpolate: maps overlap")
    refused(lib.sm_interpolate(plan._h, p[1], I16, None, 2, C.c_void_p(m[1].data_ptr() + 2), pn, st),
            b"sm_interpolate: maps overlap")
    refused(lib.sm_interpolate(plan._h, p[0], I32, pc, 2, p[1], C.c_void_p(m[1].data_ptr() + 8), st),
            b"sm_interpolate: d_filled overlaps a map")
    refused(lib.sm_interpolate(None, p[0], I32, pc, 1, p[1], pn, st), b"sm_interpolate: plan is NULL")
    refused(lib.sm_occlusion_classify(plan._h, p[0], p[2], 3, pc, st), b"sm_occlusion_classify: pairs 3 outside 1..2")
    refused(lib.sm_occlusion_classify(plan._h, None, p[2], 1, pc, st), b"sm_occlusion_classify: a map pointer is NULL")
    refused(lib.sm_occlusion_classify(plan._h, p[0], None, 1, pc, st), b"sm_occlusion_classify: a map pointer is NULL")
    refused(lib.sm_occlusion_classify(plan._h, p[0], p[2], 1, None, st), b"sm_occlusion_classify: a map pointer is NULL")
    refused(lib.sm_occlusion_classify(plan._h, p[0], p[2], 1, C.c_void_p(m[2].data_ptr() + 5), st),
            b"sm_occlusion_classify: d_class overlaps a map")
    refused(lib.sm_occlusion_classify(None, p[0], p[2], 1, pc, st), b"sm_occlusion_classify: plan is NULL")
    refused(lib.sm_plan_reserve_interp(None), b"sm_plan_reserve_interp: plan is NULL")
    torch.cuda.synchronize()
    # refused before any device call: no workspace, and every output as it was
    assert plan.workspace_bytes() == base
    assert (m[1] == 77).all() and (m[2] == 77).all() and (cls == 9).all() and (cnt == 12345).all()
    with pytest.raises(ValueError, match="int32 .* or int16"):
        plan.interpolate(torch.zeros((1, h, w), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="cls"):
        plan.interpolate(m[0], torch.zeros((2, h, w), dtype=torch.int32, device="cuda"))
    plan.close()


def test_workspace_is_allocated_only_for_the_interpolation(hip):
    w, h, mp = 300, 150, 2
    a = ip.random_map(w, h, np.int32, 1, 0.5)
    need = workspace_need(w, h, mp)
    plan = plan_for(hip, w, h, mp)
    base, describe = plan.workspace_bytes(), plan.describe()
    plan.occlusion_classify(dev(a), dev(a))
    torch.cuda.synchronize()
    assert plan.workspace_bytes() == base                      # the classification allocates nothing
    plan.reserve_interp()
    plan.reserve_interp()                                       # idempotent
    assert plan.workspace_bytes() == base + need
    assert plan.describe() == describe
    plan.interpolate(dev(a))
    plan.interpolate(dev(a.astype(np.int16)))
    assert plan.workspace_bytes() == base + need
    plan.close()
    plan = plan_for(hip, w, h, mp)                              # the first call allocates
    got = plan.interpolate(dev(a))
    assert plan.workspace_bytes() == base + need
    assert np.array_equal(host(got)[0], ir.interpolate(a))
    plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_classify_and_interpolate_captured_into_a_graph(hip, dtype):
    w, h, d = 200, 90, 16
    rng = np.random.default_rng(3)
    webs = [ip.random_map(w, h, np.int32, 40 + i, 0.6, 1, d) for i in range(3)]
    rights = [rng.integers(0, d + 1, (h, w)).astype(np.int32) for _ in range(3)]
    scale = 1 if dtype is np.int32 else 16
    plan = plan_for(hip, w, h, 1, d, "toroidal")
    try:
        base = plan.workspace_bytes()
        web = torch.zeros((1, h, w), dtype=torch.int32, device="cuda")
        right = torch.zeros_like(web)
        src = torch.zeros((1, h, w), dtype=TORCH[dtype], device="cuda")
        dst = torch.zeros_like(src)
        cls = torch.zeros((1, h, w), dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        with pytest.raises(capi.StereoHipError, match="sm_plan_reserve_interp") as err:
            with torch.cuda.graph(torch.cuda.CUDAGraph(), capture_error_mode="thread_local"):
                plan.interpolate(src, out=dst)
        assert err.value.code == capi.SM_ERR_ARG and "sm_interpolate" in err.value.message
        assert plan.workspace_bytes() == base
        # the capture stayed valid in the library's eyes: the classification needs no reservation
        g0 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g0, capture_error_mode="thread_local"):
            plan.occlusion_classify(web, right, out=cls)
        web.copy_(dev(webs[0])[None])
        right.copy_(dev(rights[0])[None])
        g0.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(cls)[0], ir.classify(webs[0], rights[0], d, "toroidal"))
        assert plan.workspace_bytes() == base
        plan.reserve_interp()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            capi.check(lib.sm_occlusion_classify(plan._h, P(web), P(right), 1, P(cls), plan._stream()))
            capi.check(lib.sm_interpolate(plan._h, P(src), TYPE[dtype], P(cls), 1, P(dst), P(cnt), plan._stream()))
        for rep, (a, r) in enumerate(zip(webs[1:] + webs[:1], rights[1:] + rights[:1])):
            web.copy_(dev(a)[None])
            right.copy_(dev(r)[None])
            src.copy_(dev((scale * a).astype(dtype))[None])
            dst.zero_()
            cls.fill_(7)
            cnt.fill_(12345)
            for _ in range(2):                                    # replayed twice: the count is zeroed by a kernel
                g.replay()
            torch.cuda.synchronize()
            want_cls = ir.classify(a, r, d, "toroidal")
            want = ir.interpolate((scale * a).astype(dtype), want_cls)
            assert np.array_equal(host(cls)[0], want_cls), rep
            assert np.array_equal(host(dst)[0], want), rep
            assert int(cnt[0]) == ir.filled(a, want), rep
    finally:
        plan.close()
