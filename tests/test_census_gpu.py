"""Census cost mode on the GPU: sm_census_transform, sm_census_wta, sm_census_wta_right, sm_census_lr and
sm_census_refine against the numpy definition (tests/census_reference.py).  Every expected value comes from the CPU
definitions; none from the HIP path."""
import ctypes as C

import numpy as np
import pytest
import torch

from stereomatching_amd import capi
from stereomatching_amd.capi import lib
from stereomatching_amd.synth import CONFIGS, make_pair
from tests import census_reference as cr
from tests import oracle
from tests.guarded import guarded_input
from tests.test_write_bounds_gpu import P, Plan, expect, out, report, stream, twice

pytestmark = pytest.mark.gpu
CENSUS = [3, 5, 7]
MODES = ["toroidal", "ghost"]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def batch(w, h, pairs, seed, levels=256):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, levels, (pairs, h, w)).astype(np.uint8),
            rng.integers(0, levels, (pairs, h, w)).astype(np.uint8))


# n = 1 .. 25 and D = 1 .. 512 (up to four launches of 128 shifts), D >= W, W < n (an even square_width equal to W),
# W < c, H < c, W % 4 != 0
SHAPES = [(40, 23, 1, 1), (33, 17, 45, 3), (64, 30, 130, 9), (70, 26, 300, 25), (52, 20, 512, 9), (12, 11, 30, 3),
          (6, 8, 19, 6), (2, 5, 6, 1), (9, 3, 12, 3), (97, 29, 64, 11), (30, 27, 20, 25)]


@pytest.mark.parametrize("census", CENSUS)
@pytest.mark.parametrize("mode", MODES)
def test_transform_is_bit_exact(hip, census, mode):
    for w, h in ((64, 16), (67, 19), (3, 2), (1, 1), (130, 40)):
        plan = hip.StereoPlan(w, h, 4, 1, mode, max_pairs=2)
        try:
            imgs = np.concatenate(batch(w, h, 2, w * h + census))          # 4 images = 2 * max_pairs
            got = plan.census_transform(dev(imgs), census)
            assert got.dtype == torch.int64 and tuple(got.shape) == (4, h, w)
            g = host(got).view(np.uint64)
            for i in range(4):
                assert np.array_equal(g[i], cr.transform(imgs[i], census, mode)), (w, h, i)
        finally:
            plan.close()


@pytest.mark.parametrize("census", CENSUS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("w,h,d,sw", SHAPES)
def test_every_map_is_exact(hip, census, mode, w, h, d, sw):
    """web / best, web_right / best_right, the checked map and rejected, sub and costs, on a full and a partial batch
    with a distinct image in every pair slot"""
    for pairs, maxp in ((3, 3), (2, 3)):
        left, right = batch(w, h, pairs, 1000 * census + w + d + pairs, levels=(256, 5)[pairs % 2])
        plan = hip.StereoPlan(w, h, d, sw, mode, max_pairs=maxp)
        try:
            gl, gr = dev(left), dev(right)
            web, best = plan.census_wta(gl, gr, census)
            web_right, best_right = plan.census_wta_right(gl, gr, census)
            md = (w + d) % 2
            res = plan.census_lr(gl, gr, census, max_diff=md, want_right=True, want_best=True)
            # refine on the left map with a few values outside 1..D besides
            web_in = host(web).copy()
            web_in.reshape(-1)[::7] = d + 1
            web_in.reshape(-1)[3::11] = -3
            web_in.reshape(-1)[5::13] = 1
            web_in.reshape(-1)[6::13] = d
            sub, costs = plan.census_refine(gl, gr, dev(web_in), census, want_costs=True)
            torch.cuda.synchronize()
            for q in range(pairs):
                tag = (census, mode, w, h, d, sw, pairs, q)
                e = cr.expected(left[q], right[q], d, sw, census, mode, md)
                assert np.array_equal(host(web)[q], e["web"]), tag
                assert np.array_equal(host(best)[q], e["best"]), tag
                assert np.array_equal(host(web_right)[q], e["web_right"]), tag
                assert np.array_equal(host(best_right)[q], e["best_right"]), tag
                assert np.array_equal(host(res.web)[q], e["checked"]), tag
                assert np.array_equal(host(res.web_right)[q], e["web_right"]), tag
                assert np.array_equal(host(res.best)[q], e["best"]), tag
                assert int(res.rejected[q]) == e["rejected"], tag
                want_sub, want_costs = cr.refine(left[q], right[q], web_in[q], d, sw, census, mode)
                assert np.array_equal(host(sub)[q], want_sub), tag
                assert np.array_equal(host(costs)[q], want_costs), tag
        finally:
            plan.close()


def patterns(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    stripes = np.where((xx // 3) % 2 == 0, 200, 40).astype(np.uint8)
    checker = np.where((xx + yy) % 2 == 0, 255, 0).astype(np.uint8)
    lone = np.full((h, w), 30, np.uint8)
    lone[::5, ::7] = 250
    return {"stripes": (stripes, np.roll(stripes, 2, axis=1)), "checker": (checker, checker[:, ::-1].copy()),
            "lone": (lone, np.roll(lone, 3, axis=1)), "lone_vs_stripes": (lone, stripes)}


@pytest.mark.parametrize("census", CENSUS)
@pytest.mark.parametrize("mode", MODES)
def test_patterns(hip, census, mode):
    w, h, d, sw = 45, 21, 24, 5
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        z = dev(np.full((h, w), 97, np.uint8))
        web, best = plan.census_wta(z, z, census)
        assert (host(web) == 1).all() and (host(best) == 0).all()
        for name, (l, r) in patterns(w, h).items():
            e = cr.expected(l, r, d, sw, census, mode, 0)
            res = plan.census_lr(dev(l), dev(r), census, max_diff=0, want_right=True, want_best=True)
            torch.cuda.synchronize()
            assert np.array_equal(host(res.best)[0], e["best"]), name
            assert np.array_equal(host(res.web_right)[0], e["web_right"]), name
            assert np.array_equal(host(res.web)[0], e["checked"]), name
            assert int(res.rejected[0]) == e["rejected"], name
    finally:
        plan.close()


@pytest.mark.parametrize("mode,w,h,d,sw,census,times", [("toroidal", 320, 96, 128, 5, 7, 4),
                                                         ("ghost", 200, 70, 30, 9, 5, 32),
                                                         ("ghost", 161, 48, 64, 11, 3, 1)])
def test_census_lr_through_hole_filling_and_refine(hip, mode, w, h, d, sw, census, times):
    left, right = make_pair(w, h, d, seed=7)
    e = cr.expected(left, right, d, sw, census, mode, 0)
    assert (e["checked"] == 0).any()
    filled = oracle.fill_web_holes(e["checked"], times)
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        gl, gr = dev(left), dev(right)
        res = plan.census_lr(gl, gr, census, max_diff=0)
        assert np.array_equal(host(res.web)[0], e["checked"])
        f = plan.fill_web_holes(res.web, times)
        assert np.array_equal(host(f)[0], filled)
        sub, _ = plan.census_refine(gl, gr, f, census)
        assert np.array_equal(host(sub)[0], cr.refine(left, right, filled, d, sw, census, mode)[0])
    finally:
        plan.close()


@pytest.mark.parametrize("census", CENSUS)
@pytest.mark.parametrize("mode", MODES)
def test_intensity_invariance(hip, census, mode):
    """R' = 2 R + 1 (values 1..127, strictly increasing): census_wta and census_lr give the same maps; SAD does not"""
    w, h, d, sw = 96, 40, 32, 7
    l, r = make_pair(w, h, d, seed=21)
    l, r = (1 + l // 2).astype(np.uint8), (1 + r // 2).astype(np.uint8)
    l2, r2 = (2 * l.astype(np.int32) + 1).astype(np.uint8), (2 * r.astype(np.int32) + 1).astype(np.uint8)
    # one camera brighter: only the right image changes
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        a_web, a_best = plan.census_wta(dev(l), dev(r), census)
        b_web, b_best = plan.census_wta(dev(l), dev(r2), census)
        c_web, _ = plan.census_wta(dev(l2), dev(r2), census)
        assert torch.equal(a_web, b_web) and torch.equal(a_best, b_best) and torch.equal(a_web, c_web)
        assert np.array_equal(host(a_web)[0], cr.wta(l, r, d, sw, census, mode)[1])
        ra = plan.census_lr(dev(l), dev(r), census, max_diff=1, want_right=True)
        rb = plan.census_lr(dev(l), dev(r2), census, max_diff=1, want_right=True)
        assert torch.equal(ra.web, rb.web) and torch.equal(ra.web_right, rb.web_right)
        assert int(ra.rejected[0]) == int(rb.rejected[0])
        sa, _ = plan.cost_wta(dev(l), dev(r), "sad")
        sb, _ = plan.cost_wta(dev(l), dev(r2), "sad")
        assert not torch.equal(sa, sb), "the SAD maps agree: the pair does not show the invariance"
    finally:
        plan.close()


@pytest.mark.parametrize("cfg,census", [("C2", 7), ("C3", 7), ("C5", 5)])
def test_large_images_by_bands(hip, cfg, census):
    w, h, d, sw, mode = CONFIGS[cfg]
    left, right = make_pair(w, h, d, seed=3)
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        res = plan.census_lr(dev(left), dev(right), census, max_diff=0, want_right=True, want_best=True)
        torch.cuda.synchronize()
        web, best, web_right = host(res.web)[0], host(res.best)[0], host(res.web_right)[0]
        assert int(res.rejected[0]) == int((web == 0).sum())
        for y0, y1 in ((0, 12), (h // 2 - 5, h // 2 + 7), (h - 12, h)):
            e = cr.expected_rows(left, right, d, sw, census, mode, y0, y1)
            assert np.array_equal(e["best"], best[y0:y1]), (cfg, y0)
            assert np.array_equal(e["web_right"], web_right[y0:y1]), (cfg, y0)
            checked, _ = cr.lr_check(e["web"], e["web_right"], 0, mode)
            assert np.array_equal(checked, web[y0:y1]), (cfg, y0)
    finally:
        plan.close()


# ---------------------------------------------------------------------------
# write bounds (tests/guarded.py)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_census_writes_its_maps_and_nothing_else(mode):
    """every census entry, each output at a 16-byte aligned and a 4-byte-but-not-16 offset, partial batches, d_web in
    place for the check"""
    bad = []
    for idx, (w, h, d, sw, census) in enumerate([(33, 17, 45, 3, 7), (64, 12, 130, 5, 3), (10, 9, 24, 9, 5),
                                                 (65, 20, 16, 1, 7)]):
        pairs, maxp = (2, 3) if idx % 2 == 0 else (1, 2)
        plan = Plan(w, h, d, sw, mode, maxp)
        tag = f"{mode} c={census} W={w} H={h} D={d} S={sw} pairs={pairs}/{maxp}"
        left, right = batch(w, h, pairs, idx + 40)
        want = [cr.expected(left[q], right[q], d, sw, census, mode, 1) for q in range(pairs)]
        Wt = lambda k: np.stack([x[k] for x in want])     # noqa: E731
        shp, s = (pairs, h, w), stream()
        gl, gr = guarded_input(left, "cuda", idx % 2, "left"), guarded_input(right, "cuda", 0, "right")
        # transform: both images of the batch
        both = np.concatenate([left, right])
        gb = guarded_input(both, "cuda", 1, "gray")
        od = out((2 * pairs, h, w), torch.int64, 0, 2 * maxp, "desc")
        t = f"{tag} sm_census_transform"
        bad += twice(t, lambda r: lib.sm_census_transform(plan.h, P(gb.t), census, 2 * pairs, P(od.t), s), [od], [gb])
        bad += expect(t, od, np.stack([cr.transform(x, census, mode) for x in both]).view(np.int64))
        for off in (0, 4):
            t = f"{tag} sm_census_wta offset {off}"
            ow, ob = out(shp, torch.int32, off, maxp, "web"), out(shp, torch.int32, 4 - off, maxp, "best")
            bad += twice(t, lambda r: lib.sm_census_wta(plan.h, P(gl.t), P(gr.t), census, pairs, P(ow.t), P(ob.t), s),
                         [ow, ob], [gl, gr])
            bad += expect(t, ow, Wt("web")) + expect(t, ob, Wt("best"))
            t = f"{tag} sm_census_wta_right offset {off}"
            owr, obr = out(shp, torch.int32, off, maxp, "web_right"), out(shp, torch.int32, off, maxp, "best_right")
            bad += twice(t, lambda r: lib.sm_census_wta_right(plan.h, P(gl.t), P(gr.t), census, pairs, P(owr.t),
                                                              P(obr.t), s), [owr, obr], [gl, gr])
            bad += expect(t, owr, Wt("web_right")) + expect(t, obr, Wt("best_right"))
            t = f"{tag} sm_census_lr offset {off}"
            ow, ob, owr = (out(shp, torch.int32, o, maxp, n) for o, n in ((off, "web"), (4 - off, "best"),
                                                                          (off, "web_right")))
            orj = out((pairs,), torch.int32, off, maxp, "rejected")
            bad += twice(t, lambda r: lib.sm_census_lr(plan.h, P(gl.t), P(gr.t), census, pairs, 1, P(ow.t), P(ob.t),
                                                       P(owr.t), P(orj.t), s), [ow, ob, owr, orj], [gl, gr])
            bad += expect(t, ow, Wt("checked")) + expect(t, ob, Wt("best")) + expect(t, owr, Wt("web_right"))
            bad += expect(t, orj, Wt("rejected"))
            # without the optional maps: the right-reference map goes through the plan's workspace
            t = f"{tag} sm_census_lr (web only) offset {off}"
            ow = out(shp, torch.int32, off, maxp, "web")
            bad += twice(t, lambda r: lib.sm_census_lr(plan.h, P(gl.t), P(gr.t), census, pairs, 1, P(ow.t), None, None,
                                                       None, s), [ow], [gl, gr])
            bad += expect(t, ow, Wt("checked"))
        web_in = Wt("checked").copy()
        web_in.reshape(-1)[::7] = d + 1
        web_in.reshape(-1)[3::11] = -3
        ref = [cr.refine(left[q], right[q], web_in[q], d, sw, census, mode) for q in range(pairs)]
        t = f"{tag} sm_census_refine"
        gw = guarded_input(web_in, "cuda", 4, "web")
        osub = out(shp, torch.int16, 2, maxp, "sub")
        ocs = out((pairs, 3, h, w), torch.int32, 4, maxp, "costs")
        bad += twice(t, lambda r: lib.sm_census_refine(plan.h, P(gl.t), P(gr.t), census, pairs, P(gw.t), P(osub.t),
                                                       P(ocs.t), s), [osub, ocs], [gl, gr, gw])
        bad += expect(t, osub, np.stack([x[0] for x in ref])) + expect(t, ocs, np.stack([x[1] for x in ref]))
        plan.close()
    report(bad)


# ---------------------------------------------------------------------------
# arguments, workspace, capture
# ---------------------------------------------------------------------------

def test_argument_checks_on_a_plan(hip):
    w, h, d = 64, 32, 16
    plan = hip.StereoPlan(w, h, d, 5, "toroidal", max_pairs=2)
    base = plan.workspace_bytes()
    m = [torch.zeros((2, h, w), dtype=torch.int32, device="cuda") for _ in range(3)]
    p = [C.c_void_p(t.data_ptr()) for t in m]
    g = torch.zeros((4, h, w), dtype=torch.uint8, device="cuda")
    gp = C.c_void_p(g.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    inside = C.c_void_p(m[0].data_ptr() + 4)

    def refused(rc, text):
        assert rc == capi.SM_ERR_ARG and text in lib.sm_last_error(), lib.sm_last_error()
    refused(lib.sm_census_transform(plan._h, gp, 7, 5, p[0], st), b"sm_census_transform: images 5 outside 1..4")
    refused(lib.sm_census_transform(plan._h, gp, 7, 0, p[0], st), b"images 0 outside 1..4")
    refused(lib.sm_census_wta(plan._h, gp, gp, 7, 3, p[0], None, st), b"sm_census_wta: pairs 3 outside 1..2")
    refused(lib.sm_census_wta(plan._h, gp, gp, 7, 1, p[0], inside, st), b"sm_census_wta: d_web and d_best overlap")
    refused(lib.sm_census_wta_right(plan._h, gp, gp, 7, 0, p[0], None, st), b"sm_census_wta_right: pairs 0 outside")
    refused(lib.sm_census_wta_right(plan._h, gp, gp, 5, 1, p[0], inside, st), b"d_web_right and d_best_right overlap")
    refused(lib.sm_census_lr(plan._h, gp, gp, 3, 3, 0, p[0], None, None, None, st), b"sm_census_lr: pairs 3 outside")
    refused(lib.sm_census_lr(plan._h, gp, gp, 3, 1, 0, p[0], p[0], None, None, st), b"sm_census_lr: result maps overlap")
    refused(lib.sm_census_lr(plan._h, gp, gp, 3, 1, 0, p[0], None, inside, None, st), b"result maps overlap")
    refused(lib.sm_census_lr(plan._h, gp, gp, 3, 2, 0, p[0], p[1], None, inside, st), b"d_rejected overlaps a map")
    refused(lib.sm_census_refine(plan._h, gp, gp, 7, 3, p[0], p[1], None, st), b"sm_census_refine: pairs 3 outside")
    assert plan.workspace_bytes() == base
    plan.close()
    for pw, ph, pd, psw, text in ((64, 32, 16, 27, b"windows up to 25x25"), (64, 32, 513, 5, b"at most 512 shifts")):
        plan = hip.StereoPlan(pw, ph, pd, psw, "toroidal")
        base = plan.workspace_bytes()
        q = torch.zeros((1, ph, pw), dtype=torch.int32, device="cuda")
        gq = torch.zeros((1, ph, pw), dtype=torch.uint8, device="cuda")
        qp, gqp = C.c_void_p(q.data_ptr()), C.c_void_p(gq.data_ptr())
        for name, call in ((b"sm_census_wta", lambda: lib.sm_census_wta(plan._h, gqp, gqp, 7, 1, qp, None, st)),
                           (b"sm_census_wta_right",
                            lambda: lib.sm_census_wta_right(plan._h, gqp, gqp, 7, 1, qp, None, st)),
                           (b"sm_census_lr", lambda: lib.sm_census_lr(plan._h, gqp, gqp, 5, 1, 0, qp, None, None, None,
                                                                      st)),
                           (b"sm_census_refine", lambda: lib.sm_census_refine(plan._h, gqp, gqp, 3, 1, qp, qp, None,
                                                                              st))):
            refused(call(), name + b": built for windows up to 25x25 and at most 512 shifts")
            assert text in lib.sm_last_error()
        assert plan.workspace_bytes() == base
        plan.close()


def test_workspace_is_allocated_only_for_census(hip):
    w, h, d, sw, mp = 300, 150, 128, 9, 2
    left, right = make_pair(w, h, d, seed=3)
    gl, gr = dev(left), dev(right)
    desc = 2 * mp * w * h * 8
    mapb = mp * w * h * 4
    plan = hip.StereoPlan(w, h, d, sw, "toroidal", max_pairs=mp)
    base, describe, geom = plan.workspace_bytes(), plan.describe(), plan.geometry()
    web, _ = plan.cost_wta(gl, gr, "sad")
    plan.cost_refine(gl, gr, web, "sad")
    plan.census_transform(gl, 7)                                         # needs no workspace
    torch.cuda.synchronize()
    assert plan.workspace_bytes() == base and plan.describe() == describe and plan.geometry() == geom
    plan.reserve_census()
    plan.reserve_census()                                                # idempotent
    assert plan.workspace_bytes() == base + desc + mapb
    assert plan.describe() == describe and plan.geometry() == geom
    plan.reserve_cost_lr()                                               # the map is shared
    assert plan.workspace_bytes() == base + desc + mapb + 2 * ((mp * w * h + 255) // 256 * 256)
    plan.close()
    # allocated by the first call that needs it; reserve_lr first: only the descriptors are added
    plan = hip.StereoPlan(w, h, d, sw, "toroidal", max_pairs=mp)
    base = plan.workspace_bytes()
    web, _ = plan.census_wta(gl, gr, 5)
    torch.cuda.synchronize()
    assert plan.workspace_bytes() == base + desc + mapb
    assert np.array_equal(host(web)[0], cr.wta(left, right, d, sw, 5, "toroidal")[1])
    plan.close()
    plan = hip.StereoPlan(w, h, d, sw, "toroidal", max_pairs=mp)
    base = plan.workspace_bytes()
    plan.reserve_lr()
    with_lr = plan.workspace_bytes()
    plan.reserve_census()
    assert plan.workspace_bytes() == with_lr + desc and with_lr > base + mapb
    plan.close()


@pytest.mark.parametrize("mode,census", [("ghost", 7), ("toroidal", 5)])
def test_census_lr_and_refine_captured_into_a_graph(hip, mode, census):
    w, h, d, sw = 320, 200, 160, 7
    pairs = [make_pair(w, h, d, seed=80 + i) for i in range(3)]
    inputs = [(dev(l), dev(r)) for l, r in pairs]
    left_in, right_in = torch.zeros_like(inputs[0][0]), torch.zeros_like(inputs[0][1])
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        base = plan.workspace_bytes()
        web = torch.zeros((1, h, w), dtype=torch.int32, device="cuda")
        right = torch.zeros_like(web)
        best = torch.zeros_like(web)
        sub = torch.zeros((1, h, w), dtype=torch.int16, device="cuda")
        rej = torch.zeros(1, dtype=torch.int32, device="cuda")
        # refused before reserve_census, and the capture stays valid (it ends cleanly; the pending error is raised)
        for call in (lambda: plan.census_lr(left_in, right_in, census, web=web),
                     lambda: plan.census_wta(left_in, right_in, census, want_best=False, web=web),
                     lambda: plan.census_wta_right(left_in, right_in, census, want_best=False, web_right=right),
                     lambda: plan.census_refine(left_in, right_in, web, census, out=sub)):
            with pytest.raises(capi.StereoHipError, match="sm_plan_reserve_census"):
                with torch.cuda.graph(torch.cuda.CUDAGraph(), capture_error_mode="thread_local"):
                    call()
        assert plan.workspace_bytes() == base
        plan.reserve_census()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        from stereomatching_amd import pipeline
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            pipeline.check(lib.sm_census_lr(plan._h, P(left_in), P(right_in), census, 1, 0, P(web), P(best), P(right),
                                            P(rej), plan._stream()))
            plan.census_refine(left_in, right_in, web, census, out=sub)
        for rep, (l, r) in enumerate(pairs[1:] + pairs[:1]):
            left_in.copy_(dev(l))
            right_in.copy_(dev(r))
            for t in (web, right, best, sub):
                t.zero_()
            rej.fill_(12345)
            g.replay()
            torch.cuda.synchronize()
            e = cr.expected(l, r, d, sw, census, mode, 0)
            assert np.array_equal(host(web)[0], e["checked"]), rep
            assert np.array_equal(host(right)[0], e["web_right"]), rep
            assert np.array_equal(host(best)[0], e["best"]), rep
            assert int(rej[0]) == e["rejected"], rep
            assert np.array_equal(host(sub)[0], cr.refine(l, r, e["checked"], d, sw, census, mode)[0]), rep
    finally:
        plan.close()
