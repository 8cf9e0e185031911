"""Rectification on the GPU: sm_rectify, sm_rectify_map_build and sm_valid_mask against the numpy definition
(tests/rectify_reference.py).  Every expected value comes from the CPU definitions, none from the HIP path; every
comparison is bit for bit.  The remap gives a lane four consecutive pixels where W % 4 == 0 and the pointers allow it,
one otherwise, 256 lanes a workgroup: the sizes sit on and around those edges and the filters' and the interpolation's."""
import ctypes as C

import numpy as np
import pytest
import torch

from stereomatching_amd import capi
from stereomatching_amd.capi import lib
from stereomatching_amd.synth import make_pair
from tests import cost_lr_reference as clr
from tests import filter_reference as fr
from tests import interp_reference as ir
from tests import rectify_patterns as rp
from tests import rectify_reference as rr
from tests.guarded import guarded_input
from tests.test_filter_gpu import SIZES as FILTER_SIZES
from tests.test_interp_gpu import SIZES as INTERP_SIZES
from tests.test_write_bounds_gpu import P, Plan, expect, out, report, stream, twice

pytestmark = pytest.mark.gpu
FMTS = ["abs32", "rel16"]
INTERPS = ["bilinear", "nearest"]
FMT = {"abs32": capi.SM_RMAP_ABS32, "rel16": capi.SM_RMAP_REL16}
ITP = {"bilinear": capi.SM_INTERP_BILINEAR, "nearest": capi.SM_INTERP_NEAREST}
SIZES = sorted(set(FILTER_SIZES + INTERP_SIZES + rp.SIZES))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def plan_for(hip, w, h, max_pairs=1, d=4, mode="ghost"):
    """the stage reads W, H and max_pairs of the plan only; the window (1) fits every image"""
    return hip.StereoPlan(w, h, d, 1, mode, max_pairs=max_pairs)


def check_rectify(plan, raw_l, raw_r, ml, mr, interp, border, want_valid, tag):
    want = rr.rectify(raw_l, raw_r, ml, mr, interp, border)
    dl = dev(ml)
    got = plan.rectify(dev(raw_l), dev(raw_r), dl, dl if mr is ml else dev(mr), interp, border, want_valid)
    assert len(got) == (4 if want_valid else 2)
    for name, g, w_ in zip(("left", "right", "valid_left", "valid_right"), got, want):
        g = host(g)
        assert g.dtype == np.uint8 and np.array_equal(g, w_), (tag, name, np.argwhere(g != w_)[:4].tolist())


def source_size(w, h, k):
    """equal to, larger and smaller than the destination"""
    return ((w, h), (w + 5, h + 3), (max(1, w // 2), max(1, h - 1)), (2 * w + 1, max(1, h // 3)))[k % 4]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("interp", INTERPS)
def test_rectify_random_maps_at_every_size(hip, fmt, interp):
    """every pixel somewhere else, inside and a little outside the source: the worst case for locality"""
    for i, (w, h) in enumerate(SIZES):
        for k, (pairs, maxp) in enumerate(((2, 2), (1, 3))):              # a full and a partial batch
            sw, sh = source_size(w, h, i + k)
            raw_l, raw_r = rp.images(pairs, sw, sh, 10 * i), rp.images(pairs, sw, sh, 10 * i + 5)
            ml = rp.random_map(w, h, sw, sh, 3 * i + k, fmt)
            mr = ml if (i + k) % 3 == 0 else rp.random_map(w, h, sw, sh, 3 * i + k + 100, fmt)
            plan = plan_for(hip, w, h, maxp)
            try:
                check_rectify(plan, raw_l, raw_r, ml, mr, interp, (0, 255, 101)[i % 3], (i + k) % 2 == 0,
                              (w, h, sw, sh, pairs, maxp))
            finally:
                plan.close()


@pytest.mark.parametrize("fmt", FMTS)
def test_rectify_smooth_maps_of_calibrations(hip, fmt):
    for w, h in ((640, 360), (333, 187), (1024, 64)):
        raw_l, raw_r = rp.images(2, w + 16, h + 8, w), rp.images(2, w + 16, h + 8, w + 9)
        ml = rr.build_map(rp.smooth_calibration(w, h, 0), w, h, fmt)
        mr = rr.build_map(rp.smooth_calibration(w, h, 1), w, h, fmt)
        plan = plan_for(hip, w, h, 2)
        try:
            for interp in INTERPS:
                check_rectify(plan, raw_l, raw_r, ml, mr, interp, 7, True, (w, h, interp))
                check_rectify(plan, raw_l, raw_r, ml, mr, interp, 7, False, (w, h, interp))
        finally:
            plan.close()


@pytest.mark.parametrize("interp", INTERPS)
def test_rectify_outside_and_extreme_maps(hip, interp):
    for w, h in ((64, 9), (37, 5), (3, 3)):
        sw, sh = w + 2, h + 1
        raw_l, raw_r = rp.images(1, sw, sh, 1), rp.images(1, sw, sh, 2)
        plan = plan_for(hip, w, h)
        try:
            for which in range(5):
                m = rp.outside_map(w, h, sw, sh, which)
                check_rectify(plan, raw_l, raw_r, m, rp.outside_map(w, h, sw, sh, (which + 1) % 5), interp, 200, True,
                              (w, h, which))
                if which < 4:
                    assert (rr.remap(raw_l[0], m, interp, 200)[0] == 200).all()
            for which in (0, 1):
                m = rp.outside_map(w, h, sw, sh, which, "rel16")
                check_rectify(plan, raw_l, raw_r, m, m, interp, 31, True, (w, h, which, "rel16"))
        finally:
            plan.close()


@pytest.mark.parametrize("fmt", FMTS)
def test_identities_on_the_gpu(hip, fmt):
    w, h = 256, 40
    raw = rp.images(2, w, h, 3)
    plan = plan_for(hip, w, h, 2)
    try:
        ident = dev(rr.identity_map(w, h, fmt))
        for interp in INTERPS:
            l, r, vl, vr = plan.rectify(dev(raw), dev(raw[::-1]), ident, ident, interp, 99, want_valid=True)
            assert np.array_equal(host(l), raw) and np.array_equal(host(r), raw[::-1])
            assert host(vl).all() and host(vr).all()
        # one [src_h][src_w] image is one pair; caller-supplied outputs are used
        left = torch.zeros((1, h, w), dtype=torch.uint8, device="cuda")
        right = torch.zeros_like(left)
        half = dev(rp.translation_map(w, h, 0, 0, fmt, fx=16))
        l, r = plan.rectify(dev(raw[0]), dev(raw[1]), half, ident, left=left, right=right)
        assert l.data_ptr() == left.data_ptr() and r.data_ptr() == right.data_ptr()
        a = raw[0].astype(int)
        assert np.array_equal(host(l)[0, :, :-1], (a[:, :-1] + a[:, 1:] + 1) >> 1)
        assert np.array_equal(host(r)[0], raw[1])
    finally:
        plan.close()


# ---------------------------------------------------------------------------
# write bounds (tests/guarded.py), misaligned pointers
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FMTS)
def test_rectify_writes_its_images_and_nothing_else(fmt):
    bad = []
    elem = 4 if fmt == "abs32" else 2
    for idx, (w, h) in enumerate([(33, 17), (64, 16), (128, 9), (1, 5), (1024, 3), (4, 4), (66, 7)]):
        pairs, maxp = (2, 3) if idx % 2 == 0 else (1, 2)
        sw, sh = source_size(w, h, idx)
        plan = Plan(w, h, 4, 1, ("toroidal", "ghost")[idx % 2], maxp)
        raw_l, raw_r = rp.images(pairs, sw, sh, idx), rp.images(pairs, sw, sh, idx + 50)
        ml = rr.build_map(rp.smooth_calibration(w, h), w, h, fmt) if w >= 33 and idx % 3 == 0 else rp.random_map(w, h, sw, sh, idx, fmt)
        mr = rp.random_map(w, h, sw, sh, idx + 9, fmt)
        shp, s = (pairs, h, w), stream()
        # images 1 - 3 bytes off 256-byte alignment, maps one element off; 0 = everything aligned (the four-pixel lanes)
        for img_off, map_off in ((0, 0), (1, elem), (2, 0), (3, elem), (0, elem), (4, 0)):
            gl, gr = guarded_input(raw_l, "cuda", img_off, "raw_left"), guarded_input(raw_r, "cuda", (img_off + 1) % 4, "raw_right")
            gml, gmr = guarded_input(ml, "cuda", map_off, "map_left"), guarded_input(mr, "cuda", map_off, "map_right")
            for interp in INTERPS:
                border = 7 + 31 * idx
                want = rr.rectify(raw_l, raw_r, ml, mr, interp, border)
                t = f"{fmt} {interp} W={w} H={h} src={sw}x{sh} pairs={pairs}/{maxp} offsets {img_off}/{map_off}"
                ol, orr = out(shp, torch.uint8, img_off, maxp, "left"), out(shp, torch.uint8, img_off, maxp, "right")
                vl, vr = out(shp, torch.uint8, img_off, maxp, "valid_left"), out(shp, torch.uint8, img_off, maxp, "valid_right")
                bad += twice(t, lambda r: lib.sm_rectify(plan.h, P(gl.t), P(gr.t), sw, sh, P(gml.t), P(gmr.t), FMT[fmt],
                                                         ITP[interp], border, pairs, P(ol.t), P(orr.t), P(vl.t), P(vr.t), s),
                             [ol, orr, vl, vr], [gl, gr, gml, gmr])
                for g, w_ in zip((ol, orr, vl, vr), want):
                    bad += expect(t, g, w_)
                # no validity, then one side's only; the same map for both sides
                t += " (one validity image, one map)"
                want = rr.rectify(raw_l, raw_r, ml, ml, interp, border)
                ol, orr = out(shp, torch.uint8, img_off, maxp, "left"), out(shp, torch.uint8, 0, maxp, "right")
                vr = out(shp, torch.uint8, img_off, maxp, "valid_right")
                bad += twice(t, lambda r: lib.sm_rectify(plan.h, P(gl.t), P(gr.t), sw, sh, P(gml.t), P(gml.t), FMT[fmt],
                                                         ITP[interp], border, pairs, P(ol.t), P(orr.t), None, P(vr.t), s),
                             [ol, orr, vr], [gl, gr, gml])
                bad += expect(t, ol, want[0]) + expect(t, orr, want[1]) + expect(t, vr, want[3])
        plan.close()
    report(bad)


def test_valid_mask_and_map_build_write_their_maps_and_nothing_else():
    bad = []
    rng = np.random.default_rng(5)
    for idx, (w, h) in enumerate([(33, 17), (64, 16), (1, 5), (130, 7)]):
        pairs, maxp = (2, 3) if idx % 2 == 0 else (1, 2)
        plan = Plan(w, h, 4, 1, "ghost", maxp)
        s = stream()
        valid = (rng.random((pairs, h, w)) < 0.5).astype(np.uint8) * rng.integers(1, 256, (pairs, h, w)).astype(np.uint8)
        for dtype, td, ty, odd in ((np.int32, torch.int32, capi.SM_MAP_I32, 4), (np.int16, torch.int16, capi.SM_MAP_I16, 2)):
            for off in (0, odd):
                gv = guarded_input(valid, "cuda", off and 3, "valid")
                gm = out((pairs, h, w), td, off, maxp, "map")
                t = f"sm_valid_mask {np.dtype(dtype).name} W={w} H={h} pairs={pairs}/{maxp} offset {off}"
                # in place: the poison is the input (all 0 bits, then all 1 bits = -1), so only the guards are checked here
                bad += twice(t, lambda r: lib.sm_valid_mask(plan.h, P(gm.t), ty, P(gv.t), pairs, s), [gm], [gv], partial=[gm])
                bad += expect(t, gm, np.where(valid != 0, -1, 0))
        for fmt, td, elem in (("abs32", torch.int32, 4), ("rel16", torch.int16, 2)):
            for name in ("identity", "barrel", "smooth_right"):
                c = rp.calibrations(w, h)[name]
                calib = capi.RectifyCalib.make(**c)
                for off in (0, elem):
                    gm = out((1, h, w, 2), td, off, 1, "rmap")
                    t = f"sm_rectify_map_build {fmt} {name} W={w} H={h} offset {off}"
                    bad += twice(t, lambda r: lib.sm_rectify_map_build(plan.h, C.byref(calib), FMT[fmt], P(gm.t), s), [gm])
                    bad += expect(t, gm, rr.build_map(c, w, h, fmt))
        plan.close()
    report(bad)


# ---------------------------------------------------------------------------
# the map of a calibration
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FMTS)
def test_map_build_equals_the_numpy_map(hip, fmt):
    for w, h in ((640, 360), (37, 19), (1000, 3), (1920, 1080)):
        plan = plan_for(hip, w, h)
        try:
            for name, c in rp.calibrations(w, h).items():
                want = rr.build_map(c, w, h, fmt)
                got = host(plan.rectify_map(c, fmt))
                assert got.dtype == want.dtype and got.shape == (h, w, 2)
                assert np.array_equal(got, want), (name, w, h, np.argwhere(got != want)[:4].tolist())
                if name == "identity":
                    assert np.array_equal(got, rr.identity_map(w, h, fmt))
        finally:
            plan.close()


def test_map_build_where_z_crosses_zero_and_the_rel16_refusal(hip):
    w, h = 320, 48
    plan = plan_for(hip, w, h)
    try:
        for c in (rp.z_crossing_calibration(w, h), rp.far_calibration(w, h)):
            want = rr.build_map(c, w, h, "abs32")
            got = host(plan.rectify_map(capi.RectifyCalib.make(**c), "abs32"))
            assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
            with pytest.raises(ValueError):
                rr.build_map(c, w, h, "rel16")
            with pytest.raises(capi.StereoHipError, match="SM_RMAP_ABS32") as err:
                plan.rectify_map(c, "rel16")
            assert err.value.code == capi.SM_ERR_ARG and "sm_rectify_map_build" in err.value.message
        z = rr.build_map(rp.z_crossing_calibration(w, h), w, h, "abs32")
        assert (z[:, w // 2] == rr.INT32_MIN).all()
        # the plan still works after a refusal
        assert np.array_equal(host(plan.rectify_map(rp.calibrations(w, h)["barrel"], "rel16")),
                              rr.build_map(rp.calibrations(w, h)["barrel"], w, h, "rel16"))
    finally:
        plan.close()


def test_rel16_refusal_looks_at_each_axis_on_its_own(hip):
    """A displacement on either side of each end of int16 along ONE axis, the other at 0 (rp.refusal_edges;
    test_rectify_cpu.py shows that a flag which looks at one axis alone gets these wrong).  The cases above overflow
    along x or along both: a builder that never looked at dy passed them (profiles/mutants/README.md, R7)."""
    w, h = rp.EDGE_W, rp.EDGE_H
    plan = plan_for(hip, w, h)
    try:
        for name, (c, fits) in rp.refusal_edges().items():
            want = rr.build_map(c, w, h, "abs32")
            got = host(plan.rectify_map(c, "abs32"))
            assert np.array_equal(got, want), (name, np.argwhere(got != want)[:4].tolist())
            if fits:
                want = rr.build_map(c, w, h, "rel16")
                got = host(plan.rectify_map(c, "rel16"))
                assert got.dtype == np.int16 and np.array_equal(got, want), (name, np.argwhere(got != want)[:4].tolist())
            else:
                with pytest.raises(ValueError):
                    rr.build_map(c, w, h, "rel16")
                with pytest.raises(capi.StereoHipError, match="SM_RMAP_ABS32") as err:
                    plan.rectify_map(c, "rel16")
                assert err.value.code == capi.SM_ERR_ARG, name
    finally:
        plan.close()


def test_smooth_calibration_at_4k(hip):
    w, h = 3840, 2160
    plan = plan_for(hip, w, h)
    try:
        raw = rp.images(1, w, h, 8)
        maps = []
        for side in (0, 1):
            c = rp.smooth_calibration(w, h, side)
            want = rr.build_map(c, w, h, "rel16")
            got = plan.rectify_map(c, "rel16")
            assert np.array_equal(host(got), want), side
            maps.append((got, want))
        got = plan.rectify(dev(raw), dev(raw), maps[0][0], maps[1][0], "bilinear", 0, want_valid=True)
        want = rr.rectify(raw, raw, maps[0][1], maps[1][1], "bilinear", 0)
        for g, w_ in zip(got, want):
            assert np.array_equal(host(g), w_)
        assert 0 < want[2].mean() < 1                     # the rectification leaves empty wedges
    finally:
        plan.close()


# ---------------------------------------------------------------------------
# valid mask
# ---------------------------------------------------------------------------

def test_valid_mask_on_both_map_types(hip):
    rng = np.random.default_rng(2)
    for w, h in ((1, 1), (63, 5), (256, 9), (130, 33)):
        for pairs, maxp in ((2, 2), (1, 3)):
            plan = plan_for(hip, w, h, maxp)
            try:
                valid = (rng.random((pairs, h, w)) < 0.6).astype(np.uint8) * rng.integers(1, 256, (pairs, h, w)).astype(np.uint8)
                for dtype, lo, hi in ((np.int32, -2**31, 2**31), (np.int16, -32768, 32768)):
                    m = rng.integers(lo, hi, (pairs, h, w)).astype(dtype)
                    t = dev(m)
                    got = plan.valid_mask(t, dev(valid))
                    assert got.data_ptr() == t.data_ptr()                      # in place
                    assert np.array_equal(host(got), rr.valid_mask(m, valid)), (w, h, dtype)
            finally:
                plan.close()


# ---------------------------------------------------------------------------
# arguments, workspace, capture, determinism
# ---------------------------------------------------------------------------

def test_argument_checks_on_a_plan(hip):
    w, h = 64, 32
    plan = plan_for(hip, w, h, 2)
    base, describe, geometry = plan.workspace_bytes(), plan.describe(), plan.geometry()
    raw = torch.full((2, h + 4, w + 4), 5, dtype=torch.uint8, device="cuda")
    o = [torch.full((2, h, w), 77, dtype=torch.uint8, device="cuda") for _ in range(4)]
    m = dev(rr.identity_map(w, h, "abs32"))
    web = torch.full((2, h, w), 9, dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    A, B = capi.SM_RMAP_ABS32, capi.SM_INTERP_BILINEAR
    pr, pm, po = P(raw), P(m), [P(t) for t in o]

    def refused(rc, text):
        assert rc == capi.SM_ERR_ARG and text in lib.sm_last_error(), lib.sm_last_error()
    sw, sh = w + 4, h + 4
    refused(lib.sm_rectify(plan._h, pr, pr, sw, sh, pm, pm, A, B, 0, 3, po[0], po[1], po[2], po[3], st),
            b"sm_rectify: pairs 3 outside 1..2")
    refused(lib.sm_rectify(plan._h, pr, pr, sw, sh, pm, pm, A, B, 0, 0, po[0], po[1], None, None, st),
            b"sm_rectify: pairs 0 outside 1..2")
    refused(lib.sm_rectify(plan._h, pr, pr, sw, sh, pm, pm, 5, B, 0, 1, po[0], po[1], None, None, st), b"sm_rectify: map_format 5")
    refused(lib.sm_rectify(plan._h, pr, pr, sw, sh, pm, pm, A, 7, 0, 1, po[0], po[1], None, None, st), b"sm_rectify: interp 7")
    refused(lib.sm_rectify(plan._h, pr, pr, sw, sh, pm, pm, A, B, 256, 1, po[0], po[1], None, None, st), b"sm_rectify: border 256")
    refused(lib.sm_rectify(plan._h, pr, pr, -1, sh, pm, pm, A, B, 0, 1, po[0], po[1], None, None, st), b"sm_rectify: source size")
    # ranges that overlap without being equal
    refused(lib.sm_rectify(plan._h, pr, pr, sw, sh, pm, pm, A, B, 0, 2, po[0], C.c_void_p(o[0].data_ptr() + 100), None, None, st),
            b"sm_rectify: outputs overlap")
    refused(lib.sm_rectify(plan._h, pr, pr, sw, sh, pm, pm, A, B, 0, 2, C.c_void_p(raw.data_ptr() + 64), po[1], None, None, st),
            b"sm_rectify: an output overlaps an input")
    refused(lib.sm_rectify(plan._h, pr, pr, sw, sh, pm, pm, A, B, 0, 1, po[0], po[1], None, C.c_void_p(m.data_ptr() + 8), st),
            b"sm_rectify: an output overlaps an input")
    refused(lib.sm_rectify(plan._h, pr, pr, sw, sh, C.c_void_p(m.data_ptr() + 2), pm, A, B, 0, 1, po[0], po[1], None, None, st),
            b"sm_rectify: a map pointer is not aligned")
    calib = capi.RectifyCalib.make(50.0, 50.0, 32.0, 16.0)
    refused(lib.sm_rectify_map_build(plan._h, None, A, pm, st), b"sm_rectify_map_build: calib is NULL")
    refused(lib.sm_rectify_map_build(plan._h, C.byref(calib), A, None, st), b"sm_rectify_map_build: a map pointer is NULL")
    refused(lib.sm_rectify_map_build(plan._h, C.byref(calib), 2, pm, st), b"sm_rectify_map_build: map_format 2")
    calib.struct_size = 16
    refused(lib.sm_rectify_map_build(plan._h, C.byref(calib), A, pm, st), b"sm_rectify_map_build: calib->struct_size 16")
    refused(lib.sm_valid_mask(plan._h, P(web), capi.SM_MAP_I32, po[0], 3, st), b"sm_valid_mask: pairs 3 outside 1..2")
    refused(lib.sm_valid_mask(plan._h, P(web), capi.SM_MAP_I32, C.c_void_p(web.data_ptr() + 12), 1, st),
            b"sm_valid_mask: d_valid overlaps the map")
    torch.cuda.synchronize()
    # refused before any device call: every output as it was, and the map still the identity
    assert all((t == 77).all() for t in o) and (web == 9).all()
    assert np.array_equal(host(m), rr.identity_map(w, h, "abs32"))
    with pytest.raises(ValueError, match="interp"):
        plan.rectify(raw, raw, m, m, interp="cubic")
    with pytest.raises(ValueError, match="map_right"):
        plan.rectify(raw, raw, m, dev(rr.identity_map(w, h, "rel16")))
    with pytest.raises(ValueError, match="map_left"):
        plan.rectify(raw, raw, dev(rr.identity_map(w + 1, h, "abs32")), m)
    with pytest.raises(ValueError, match="raw_right"):
        plan.rectify(raw, raw[:1], m, m)
    with pytest.raises(ValueError, match="fmt"):
        plan.rectify_map(dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0), "abs16")
    with pytest.raises(ValueError, match="valid"):
        plan.valid_mask(web, o[0][:1])
    # a plan that rectifies needs no workspace and stays the plan it was
    plan.rectify(raw, raw, m, m, want_valid=True)
    plan.rectify_map(dict(fx=50.0, fy=50.0, cx=32.0, cy=16.0), "rel16")
    plan.valid_mask(web, o[0])
    torch.cuda.synchronize()
    assert plan.workspace_bytes() == base and plan.describe() == describe and plan.geometry() == geometry
    plan.close()


def test_rectify_and_valid_mask_captured_into_a_graph(hip):
    w, h, sw, sh = 200, 90, 211, 97
    plan = plan_for(hip, w, h)
    try:
        ml, mr = rp.random_map(w, h, sw, sh, 1, "rel16"), rr.build_map(rp.smooth_calibration(w, h, 1), w, h, "rel16")
        dml, dmr = dev(ml), dev(mr)
        raw_l = torch.zeros((1, sh, sw), dtype=torch.uint8, device="cuda")
        raw_r = torch.zeros_like(raw_l)
        left = torch.zeros((1, h, w), dtype=torch.uint8, device="cuda")
        right, vl, vr = torch.zeros_like(left), torch.zeros_like(left), torch.zeros_like(left)
        web = torch.zeros((1, h, w), dtype=torch.int32, device="cuda")
        spare = torch.zeros((h, w, 2), dtype=torch.int16, device="cuda")
        calib = capi.RectifyCalib.make(**rp.smooth_calibration(w, h, 0))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            # the builder is refused, and the capture goes on
            rc = lib.sm_rectify_map_build(plan._h, C.byref(calib), capi.SM_RMAP_REL16, P(spare), plan._stream())
            assert rc == capi.SM_ERR_ARG and b"sm_rectify_map_build: the stream is capturing" in lib.sm_last_error()
            capi.check(lib.sm_rectify(plan._h, P(raw_l), P(raw_r), sw, sh, P(dml), P(dmr), capi.SM_RMAP_REL16,
                                      capi.SM_INTERP_BILINEAR, 40, 1, P(left), P(right), P(vl), P(vr), plan._stream()))
            capi.check(lib.sm_valid_mask(plan._h, P(web), capi.SM_MAP_I32, P(vl), 1, plan._stream()))
        assert not host(spare).any()
        rng = np.random.default_rng(7)
        for rep in range(3):
            a, b = rp.images(1, sw, sh, 20 + rep), rp.images(1, sw, sh, 30 + rep)
            disp = rng.integers(-5, 60, (1, h, w)).astype(np.int32)
            raw_l.copy_(dev(a))
            raw_r.copy_(dev(b))
            web.copy_(dev(disp))
            for t in (left, right, vl, vr):
                t.fill_(123)
            g.replay()
            torch.cuda.synchronize()
            want = rr.rectify(a, b, ml, mr, "bilinear", 40)
            for name, t, w_ in zip(("left", "right", "valid_left", "valid_right"), (left, right, vl, vr), want):
                assert np.array_equal(host(t), w_), (rep, name)
            assert np.array_equal(host(web), rr.valid_mask(disp, want[2])), rep
            # an eager call between replays, other arguments
            e = plan.rectify(dev(b), dev(a), dmr, dml, "nearest", 3, want_valid=True)
            for t, w_ in zip(e, rr.rectify(b, a, mr, ml, "nearest", 3)):
                assert np.array_equal(host(t), w_), rep
    finally:
        plan.close()


def test_fifty_launches_give_identical_bytes(hip):
    w, h, sw, sh = 640, 360, 700, 380
    plan = plan_for(hip, w, h, 2)
    try:
        raw_l, raw_r = dev(rp.images(2, sw, sh, 1)), dev(rp.images(2, sw, sh, 2))
        ml, mr = dev(rp.random_map(w, h, sw, sh, 4, "abs32")), dev(rr.build_map(rp.smooth_calibration(w, h), w, h, "abs32"))
        first = [t.clone() for t in plan.rectify(raw_l, raw_r, ml, mr, want_valid=True)]
        for _ in range(50):
            got = plan.rectify(raw_l, raw_r, ml, mr, want_valid=True)
            assert all(torch.equal(a, b) for a, b in zip(first, got))
    finally:
        plan.close()


# ---------------------------------------------------------------------------
# the chain: raw scene -> rectify -> cost_lr -> valid_mask -> speckle -> interpolate
# ---------------------------------------------------------------------------

def moved(img, dx, dy, border):
    """out(x + dx, y + dy) = img(x, y), `border` where nothing lands"""
    h, w = img.shape
    res = np.full((h, w), border, np.uint8)
    ys, xs = np.arange(h), np.arange(w)
    ys, xs = ys[(ys + dy >= 0) & (ys + dy < h)], xs[(xs + dx >= 0) & (xs + dx < w)]
    res[np.ix_(ys + dy, xs + dx)] = img[np.ix_(ys, xs)]
    return res


@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
def test_raw_scene_through_rectify_check_mask_speckle_and_interpolate(hip, mode):
    w, h, d, sw = 160, 64, 24, 5
    left, right = make_pair(w, h, d, seed=11)
    # the cameras: the left image 3 rows down and 2 columns right, the right one 2 rows up and 1 column left, and a
    # quarter-pixel shear on the right one so that the bilinear weights take part
    raw_l, raw_r = moved(left, 2, 3, 255), moved(right, -1, -2, 0)
    ml = rp.translation_map(w, h, 2, 3, "rel16")
    mx, my = rr.positions(rp.translation_map(w, h, -1, -2, "abs32"))
    mr = rr.rel_map(mx + (np.arange(h)[:, None] % 3) * 8, my)
    rl, rright, vl, vr = rr.rectify(raw_l[None], raw_r[None], ml, mr, "bilinear", 0)
    e = clr.expected(rl[0], rright[0], d, sw, mode, "sad", 1)
    masked = rr.valid_mask(e["checked"], vl[0] & vr[0])
    assert 0 < (masked != e["checked"]).sum()
    speckled, removed = fr.speckle(masked, 20, 1)
    cls = ir.classify(speckled, e["web_right"], d, mode)
    filled = ir.interpolate(speckled, cls)
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        gl, gr, gvl, gvr = plan.rectify(dev(raw_l), dev(raw_r), dev(ml), dev(mr), "bilinear", 0, want_valid=True)
        assert np.array_equal(host(gl), rl) and np.array_equal(host(gr), rright)
        assert np.array_equal(host(gvl), vl) and np.array_equal(host(gvr), vr)
        res = plan.cost_lr(gl, gr, "sad", max_diff=1, want_right=True)
        assert np.array_equal(host(res.web)[0], e["checked"])
        assert np.array_equal(host(res.web_right)[0], e["web_right"])
        both = gvl & gvr
        got = plan.valid_mask(res.web, both)
        assert np.array_equal(host(got)[0], masked)
        got, n = plan.speckle_filter(got, 20, 1, out=got, want_removed=True)
        assert np.array_equal(host(got)[0], speckled) and int(n[0]) == removed
        got_cls = plan.occlusion_classify(got, res.web_right)
        assert np.array_equal(host(got_cls)[0], cls)
        assert np.array_equal(host(plan.interpolate(got, got_cls))[0], filled)
    finally:
        plan.close()
