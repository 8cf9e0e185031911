"""SGM over the census data term on the GPU: sm_sgm_wta, sm_sgm_wta_right and sm_sgm_lr against the numpy definition
(tests/sgm_reference.py).  Every expected value comes from the CPU definitions; none from the HIP path."""
import ctypes as C

import numpy as np
import pytest
import torch

from stereomatching_amd import capi
from stereomatching_amd.capi import lib
from stereomatching_amd.synth import CONFIGS, make_pair
from tests import oracle
from tests import sgm_reference as sr
from tests.guarded import guarded_input
from tests.test_write_bounds_gpu import P, Plan, expect, out, report, stream, twice

pytestmark = pytest.mark.gpu
MODES = ["toroidal", "ghost"]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def batch(w, h, pairs, seed, levels=256):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, levels, (pairs, h, w)).astype(np.uint8),
            rng.integers(0, levels, (pairs, h, w)).astype(np.uint8))


def check_all(plan, left, right, d, sw, census, p1, p2, paths, mode, pairs, md, tag):
    """sgm_wta (web, best, sub), sgm_wta_right and sgm_lr (every map) against the definition, pair by pair"""
    gl, gr = dev(left), dev(right)
    web, best, sub = plan.sgm_wta(gl, gr, census, p1, p2, paths, want_sub=True)
    web_right, best_right = plan.sgm_wta_right(gl, gr, census, p1, p2, paths)
    res = plan.sgm_lr(gl, gr, census, p1, p2, paths, max_diff=md, want_right=True, want_best=True, want_sub=True)
    torch.cuda.synchronize()
    for q in range(pairs):
        e = sr.expected(left[q], right[q], d, sw, census, p1, p2, paths, mode, md)
        t = tag + (q,)
        assert np.array_equal(host(web)[q], e["web"]), t
        assert np.array_equal(host(best)[q], e["best"]), t
        assert np.array_equal(host(sub)[q], e["sub"]), t
        assert np.array_equal(host(web_right)[q], e["web_right"]), t
        assert np.array_equal(host(best_right)[q], e["best_right"]), t
        assert np.array_equal(host(res.web)[q], e["checked"]), t
        assert np.array_equal(host(res.web_right)[q], e["web_right"]), t
        assert np.array_equal(host(res.best)[q], e["best"]), t
        assert np.array_equal(host(res.sub)[q], e["sub_checked"]), t
        assert int(res.rejected[q]) == e["rejected"], t


@pytest.mark.parametrize("census", [3, 5, 7])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("paths", [4, 8])
def test_borders_paths_and_census_widths(hip, census, mode, paths):
    w, h, d, sw = 37, 19, 24, 3
    left, right = batch(w, h, 1, 10 * census + paths, levels=(256, 6)[census == 5])
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        check_all(plan, left, right, d, sw, census, 12, 90, paths, mode, 1, 1, (census, mode, paths))
    finally:
        plan.close()


# windows 1, 3, 9, 25; shifts 1, 2, 63, 64, 65, 128, 256; odd W and H; W < D
SHAPES = [(41, 13, 1, 1), (33, 17, 2, 3), (29, 31, 63, 9), (64, 20, 64, 1), (45, 27, 65, 25), (70, 9, 128, 3),
          (30, 11, 256, 9), (25, 29, 40, 25)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("w,h,d,sw", SHAPES)
def test_windows_and_shift_counts(hip, mode, w, h, d, sw):
    census, paths = (7, 8) if d % 2 else (5, 4)
    p1, p2 = (8 * (sw // 2 + 1), 100 * (sw // 2 + 1))
    for pairs, maxp in ((2, 2), (1, 3)):                     # a full and a partial batch
        left, right = batch(w, h, pairs, w + d + pairs, levels=(256, 4)[pairs % 2])
        plan = hip.StereoPlan(w, h, d, sw, mode, max_pairs=maxp)
        try:
            check_all(plan, left, right, d, sw, census, p1, p2, paths, mode, pairs, d % 2,
                      (mode, w, h, d, sw, pairs, maxp))
        finally:
            plan.close()


@pytest.mark.parametrize("mode", MODES)
def test_penalty_extremes(hip, mode):
    cases = [(40, 15, 20, 3, 5, 0, 0), (40, 15, 20, 3, 3, 50, 50), (33, 27, 16, 25, 7, 0, 32767),
             (26, 27, 70, 25, 7, 32767, 32767)]
    for w, h, d, sw, census, p1, p2 in cases:
        left, right = batch(w, h, 1, p1 + p2 + w)
        plan = hip.StereoPlan(w, h, d, sw, mode)
        try:
            check_all(plan, left, right, d, sw, census, p1, p2, 8, mode, 1, 0, (mode, w, d, sw, p1, p2))
        finally:
            plan.close()


@pytest.mark.parametrize("mode", MODES)
def test_zero_penalties_give_census_wta_and_constant_images_give_one(hip, mode):
    from tests import census_reference as cr
    w, h, d, sw = 50, 21, 30, 5
    left, right = batch(w, h, 1, 3)
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        for paths in (4, 8):
            web, best, _ = plan.sgm_wta(dev(left), dev(right), 7, 0, 0, paths)
            cweb, cbest = plan.census_wta(dev(left), dev(right), 7)
            assert torch.equal(web, cweb) and torch.equal(best, paths * cbest)
            assert np.array_equal(host(web)[0], cr.wta(left[0], right[0], d, sw, 7, mode)[1])
        z = dev(np.full((1, h, w), 131, np.uint8))
        web, best, sub = plan.sgm_wta(z, z, 5, 10, 120, 8, want_sub=True)
        assert (host(web) == 1).all() and (host(best) == 0).all() and (host(sub) == 16).all()
        # all-tie: a flat left image against a flat right one of another level
        web, best, sub = plan.sgm_wta(z, dev(np.full((1, h, w), 7, np.uint8)), 3, 10, 120, 4, want_sub=True)
        e = sr.sgm(np.full((h, w), 131, np.uint8), np.full((h, w), 7, np.uint8), d, sw, 3, 10, 120, 4, mode)
        assert np.array_equal(host(web)[0], e[1]) and np.array_equal(host(best)[0], e[0])
        assert np.array_equal(host(sub)[0], e[2])
    finally:
        plan.close()


@pytest.mark.parametrize("mode", MODES)
def test_intensity_invariance(hip, mode):
    w, h, d, sw = 96, 40, 32, 3
    l, r = make_pair(w, h, d, seed=21)
    l, r = (1 + l // 2).astype(np.uint8), (1 + r // 2).astype(np.uint8)
    r2 = (2 * r.astype(np.int32) + 1).astype(np.uint8)
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        a = plan.sgm_lr(dev(l), dev(r), 7, 20, 200, 8, max_diff=1, want_right=True, want_sub=True)
        b = plan.sgm_lr(dev(l), dev(r2), 7, 20, 200, 8, max_diff=1, want_right=True, want_sub=True)
        assert torch.equal(a.web, b.web) and torch.equal(a.web_right, b.web_right) and torch.equal(a.sub, b.sub)
        assert int(a.rejected[0]) == int(b.rejected[0])
    finally:
        plan.close()


@pytest.mark.parametrize("mode,w,h,d,sw,census,times", [("toroidal", 160, 64, 48, 3, 7, 4),
                                                         ("ghost", 120, 50, 30, 5, 5, 1)])
def test_sgm_lr_through_step3(hip, mode, w, h, d, sw, census, times):
    left, right = make_pair(w, h, d, seed=9)
    e = sr.expected(left, right, d, sw, census, 10, 120, 8, mode, 0)
    assert (e["checked"] == 0).any()
    filled = oracle.fill_web_holes(e["checked"], times)
    contour = oracle.draw_contour_map(filled, 5)
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        res = plan.sgm_lr(dev(left), dev(right), census, 10, 120, 8, max_diff=0)
        assert np.array_equal(host(res.web)[0], e["checked"])
        f, c, mm = plan.step3(res.web, times, 5)
        assert np.array_equal(host(f)[0], filled)
        assert np.array_equal(host(c)[0], contour)
        assert host(mm)[0].tolist() == [int(filled.min()), int(filled.max())]
    finally:
        plan.close()


def test_full_c2_pair(hip):
    """one 1920 x 1080 pair, 64 shifts, 7 x 7, 8 paths, every map against numpy"""
    w, h, d, sw, mode = CONFIGS["C2"]
    left, right = make_pair(w, h, d, seed=3)
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        p1, p2 = 8 * 16, 96 * 16
        web, best, sub = plan.sgm_wta(dev(left), dev(right), 7, p1, p2, 8, want_sub=True)
        torch.cuda.synchronize()
        b, wb, s = sr.sgm(left, right, d, sw, 7, p1, p2, 8, mode)
        assert np.array_equal(host(web)[0], wb)
        assert np.array_equal(host(best)[0], b)
        assert np.array_equal(host(sub)[0], s)
    finally:
        plan.close()


# ---------------------------------------------------------------------------
# write bounds (tests/guarded.py)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_sgm_writes_its_maps_and_nothing_else(mode):
    bad = []
    for idx, (w, h, d, sw, census, paths) in enumerate([(33, 17, 45, 3, 7, 8), (64, 12, 130, 1, 3, 4),
                                                        (10, 9, 24, 9, 5, 8)]):
        pairs, maxp = (2, 3) if idx % 2 == 0 else (1, 2)
        plan = Plan(w, h, d, sw, mode, maxp)
        tag = f"{mode} c={census} W={w} H={h} D={d} S={sw} paths={paths} pairs={pairs}/{maxp}"
        left, right = batch(w, h, pairs, idx + 70)
        p1, p2 = 9, 99
        want = [sr.expected(left[q], right[q], d, sw, census, p1, p2, paths, mode, 1) for q in range(pairs)]
        Wt = lambda k: np.stack([x[k] for x in want])     # noqa: E731
        shp, s = (pairs, h, w), stream()
        gl, gr = guarded_input(left, "cuda", idx % 2, "left"), guarded_input(right, "cuda", 0, "right")
        for off in (0, 4):
            t = f"{tag} sm_sgm_wta offset {off}"
            ow, ob = out(shp, torch.int32, off, maxp, "web"), out(shp, torch.int32, 4 - off, maxp, "best")
            osb = out(shp, torch.int16, 2, maxp, "sub")
            bad += twice(t, lambda r: lib.sm_sgm_wta(plan.h, P(gl.t), P(gr.t), census, p1, p2, paths, pairs, P(ow.t),
                                                     P(ob.t), P(osb.t), s), [ow, ob, osb], [gl, gr])
            bad += expect(t, ow, Wt("web")) + expect(t, ob, Wt("best")) + expect(t, osb, Wt("sub"))
            t = f"{tag} sm_sgm_wta_right offset {off}"
            owr, obr = out(shp, torch.int32, off, maxp, "web_right"), out(shp, torch.int32, off, maxp, "best_right")
            bad += twice(t, lambda r: lib.sm_sgm_wta_right(plan.h, P(gl.t), P(gr.t), census, p1, p2, paths, pairs,
                                                           P(owr.t), P(obr.t), s), [owr, obr], [gl, gr])
            bad += expect(t, owr, Wt("web_right")) + expect(t, obr, Wt("best_right"))
            t = f"{tag} sm_sgm_lr offset {off}"
            ow, ob, owr = (out(shp, torch.int32, o, maxp, n) for o, n in ((off, "web"), (4 - off, "best"),
                                                                          (off, "web_right")))
            orj = out((pairs,), torch.int32, off, maxp, "rejected")
            osb = out(shp, torch.int16, 2, maxp, "sub")
            bad += twice(t, lambda r: lib.sm_sgm_lr(plan.h, P(gl.t), P(gr.t), census, p1, p2, paths, pairs, 1, P(ow.t),
                                                    P(ob.t), P(owr.t), P(orj.t), P(osb.t), s),
                         [ow, ob, owr, orj, osb], [gl, gr])
            bad += expect(t, ow, Wt("checked")) + expect(t, ob, Wt("best")) + expect(t, owr, Wt("web_right"))
            bad += expect(t, orj, Wt("rejected")) + expect(t, osb, Wt("sub_checked"))
            t = f"{tag} sm_sgm_lr (web only) offset {off}"
            ow = out(shp, torch.int32, off, maxp, "web")
            bad += twice(t, lambda r: lib.sm_sgm_lr(plan.h, P(gl.t), P(gr.t), census, p1, p2, paths, pairs, 1, P(ow.t),
                                                    None, None, None, None, s), [ow], [gl, gr])
            bad += expect(t, ow, Wt("checked"))
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
    refused(lib.sm_sgm_wta(plan._h, gp, gp, 7, 10, 120, 8, 3, p[0], None, None, st), b"sm_sgm_wta: pairs 3 outside 1..2")
    refused(lib.sm_sgm_wta(plan._h, gp, gp, 7, 10, 120, 8, 0, p[0], None, None, st), b"sm_sgm_wta: pairs 0 outside")
    refused(lib.sm_sgm_wta(plan._h, gp, gp, 7, 10, 120, 8, 1, p[0], inside, None, st),
            b"sm_sgm_wta: result maps overlap")
    refused(lib.sm_sgm_wta(plan._h, gp, gp, 7, 10, 120, 8, 1, p[0], p[1], inside, st),
            b"sm_sgm_wta: result maps overlap")            # d_sub inside d_web
    refused(lib.sm_sgm_wta(plan._h, gp, gp, 7, 10, 120, 8, 1, p[0], p[1], C.c_void_p(m[1].data_ptr() + 2), st),
            b"sm_sgm_wta: result maps overlap")            # d_sub inside d_best
    refused(lib.sm_sgm_wta(plan._h, gp, gp, 7, 10, 120, 6, 1, p[0], None, None, st), b"sm_sgm_wta: paths 6 is not")
    refused(lib.sm_sgm_wta(plan._h, gp, gp, 7, 130, 120, 8, 1, p[0], None, None, st), b"sm_sgm_wta: penalties")
    refused(lib.sm_sgm_wta_right(plan._h, gp, gp, 5, 10, 120, 4, 3, p[0], None, st), b"sm_sgm_wta_right: pairs 3")
    refused(lib.sm_sgm_wta_right(plan._h, gp, gp, 5, 10, 120, 4, 1, p[0], inside, st),
            b"sm_sgm_wta_right: result maps overlap")
    refused(lib.sm_sgm_lr(plan._h, gp, gp, 3, 10, 120, 8, 3, 0, p[0], None, None, None, None, st),
            b"sm_sgm_lr: pairs 3 outside")
    refused(lib.sm_sgm_lr(plan._h, gp, gp, 3, 10, 120, 8, 1, 0, p[0], p[0], None, None, None, st),
            b"sm_sgm_lr: result maps overlap")
    refused(lib.sm_sgm_lr(plan._h, gp, gp, 3, 10, 120, 8, 1, 0, p[0], None, inside, None, None, st),
            b"sm_sgm_lr: result maps overlap")
    refused(lib.sm_sgm_lr(plan._h, gp, gp, 3, 10, 120, 8, 1, 0, p[0], None, p[1], None, C.c_void_p(m[1].data_ptr()),
                          st), b"sm_sgm_lr: result maps overlap")
    refused(lib.sm_sgm_lr(plan._h, gp, gp, 3, 10, 120, 8, 2, 0, p[0], p[1], None, inside, None, st),
            b"sm_sgm_lr: d_rejected overlaps a map")
    refused(lib.sm_sgm_lr(plan._h, gp, gp, 3, 10, 120, 8, 1, 0, p[0], None, None, p[2], C.c_void_p(m[2].data_ptr()),
                          st), b"sm_sgm_lr: d_rejected overlaps a map")
    refused(lib.sm_sgm_lr(plan._h, gp, gp, 3, 10, 120, 8, 1, -2, p[0], None, None, None, None, st),
            b"sm_sgm_lr: max_diff -2 is negative")
    assert plan.workspace_bytes() == base
    plan.close()
    for pw, ph, pd, psw, text in ((64, 32, 16, 27, b"(got 27x27, 16)"), (64, 32, 257, 5, b"(got 5x5, 257)")):
        plan = hip.StereoPlan(pw, ph, pd, psw, "toroidal")
        base = plan.workspace_bytes()
        q = torch.zeros((1, ph, pw), dtype=torch.int32, device="cuda")
        gq = torch.zeros((1, ph, pw), dtype=torch.uint8, device="cuda")
        qp, gqp = C.c_void_p(q.data_ptr()), C.c_void_p(gq.data_ptr())
        for name, call in ((b"sm_sgm_wta", lambda: lib.sm_sgm_wta(plan._h, gqp, gqp, 7, 1, 2, 8, 1, qp, None, None, st)),
                           (b"sm_sgm_wta_right",
                            lambda: lib.sm_sgm_wta_right(plan._h, gqp, gqp, 7, 1, 2, 4, 1, qp, None, st)),
                           (b"sm_sgm_lr", lambda: lib.sm_sgm_lr(plan._h, gqp, gqp, 5, 1, 2, 8, 1, 0, qp, None, None,
                                                                None, None, st))):
            refused(call(), name + b": built for windows up to 25x25 and at most 256 shifts")
            assert text in lib.sm_last_error()
        assert plan.workspace_bytes() == base
        plan.close()


def test_workspace_is_allocated_only_for_sgm(hip):
    w, h, d, sw, mp = 300, 150, 100, 9, 2
    left, right = make_pair(w, h, d, seed=3)
    gl, gr = dev(left), dev(right)
    desc = 2 * mp * w * h * 8
    mapb = mp * w * h * 4
    vol = 6 * w * h * 128                                  # 100 shifts padded to 128
    plan = hip.StereoPlan(w, h, d, sw, "toroidal", max_pairs=mp)
    base, describe, geom = plan.workspace_bytes(), plan.describe(), plan.geometry()
    plan.census_wta(gl, gr, 7)                              # census alone: no volumes
    torch.cuda.synchronize()
    assert plan.workspace_bytes() == base + desc + mapb
    plan.reserve_sgm()
    plan.reserve_sgm()                                      # idempotent
    assert plan.workspace_bytes() == base + desc + mapb + vol
    assert plan.describe() == describe and plan.geometry() == geom
    plan.reserve_lr()                                       # the map is shared: only the mirrored packed images added
    plan.close()
    # allocated by the first call that needs it, census workspace included
    plan = hip.StereoPlan(w, h, d, sw, "toroidal", max_pairs=mp)
    base = plan.workspace_bytes()
    web, _, _ = plan.sgm_wta(gl, gr, 5, 10, 120, 4, want_best=False)
    torch.cuda.synchronize()
    assert plan.workspace_bytes() == base + desc + mapb + vol
    assert np.array_equal(host(web)[0], sr.sgm(left, right, d, sw, 5, 10, 120, 4, "toroidal")[1])
    plan.close()
    # reserve_lr first: the map is not allocated twice
    plan = hip.StereoPlan(w, h, d, sw, "toroidal", max_pairs=mp)
    plan.reserve_lr()
    with_lr = plan.workspace_bytes()
    plan.reserve_sgm()
    assert plan.workspace_bytes() == with_lr + desc + vol
    plan.close()
    # reserve_census first: only the volumes are added
    plan = hip.StereoPlan(w, h, d, sw, "toroidal", max_pairs=mp)
    plan.reserve_census()
    with_census = plan.workspace_bytes()
    plan.reserve_sgm()
    assert plan.workspace_bytes() == with_census + vol
    plan.close()


@pytest.mark.parametrize("mode,census,paths", [("ghost", 7, 8), ("toroidal", 5, 4)])
def test_sgm_captured_into_a_graph(hip, mode, census, paths):
    w, h, d, sw = 160, 90, 64, 3
    pairs = [make_pair(w, h, d, seed=60 + i) for i in range(3)]
    left_in, right_in = torch.zeros((1, h, w), dtype=torch.uint8, device="cuda"), torch.zeros((1, h, w),
                                                                                             dtype=torch.uint8,
                                                                                             device="cuda")
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        base = plan.workspace_bytes()
        web = torch.zeros((1, h, w), dtype=torch.int32, device="cuda")
        right = torch.zeros_like(web)
        best = torch.zeros_like(web)
        sub = torch.zeros((1, h, w), dtype=torch.int16, device="cuda")
        rej = torch.zeros(1, dtype=torch.int32, device="cuda")
        for call in (lambda: plan.sgm_lr(left_in, right_in, census, 10, 120, paths, web=web),
                     lambda: plan.sgm_wta(left_in, right_in, census, 10, 120, paths, want_best=False, web=web),
                     lambda: plan.sgm_wta_right(left_in, right_in, census, 10, 120, paths, want_best=False,
                                                web_right=right)):
            with pytest.raises(capi.StereoHipError, match="sm_plan_reserve_sgm"):
                with torch.cuda.graph(torch.cuda.CUDAGraph(), capture_error_mode="thread_local"):
                    call()
        assert plan.workspace_bytes() == base
        plan.reserve_sgm()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        from stereomatching_amd import pipeline
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            pipeline.check(lib.sm_sgm_lr(plan._h, P(left_in), P(right_in), census, 10, 120, paths, 1, 0, P(web),
                                         P(best), P(right), P(rej), P(sub), plan._stream()))
        for rep, (l, r) in enumerate(pairs[1:] + pairs[:1]):
            left_in.copy_(dev(l))
            right_in.copy_(dev(r))
            for t in (web, right, best, sub):
                t.zero_()
            rej.fill_(12345)
            g.replay()
            torch.cuda.synchronize()
            e = sr.expected(l, r, d, sw, census, 10, 120, paths, mode, 0)
            assert np.array_equal(host(web)[0], e["checked"]), rep
            assert np.array_equal(host(right)[0], e["web_right"]), rep
            assert np.array_equal(host(best)[0], e["best"]), rep
            assert np.array_equal(host(sub)[0], e["sub_checked"]), rep
            assert int(rej[0]) == e["rejected"], rep
            # the eager call gives the same maps
            eager = plan.sgm_lr(dev(l)[None][0], dev(r)[None][0], census, 10, 120, paths, want_right=True,
                                want_best=True, want_sub=True)
            assert torch.equal(eager.web, web) and torch.equal(eager.sub, sub) and torch.equal(eager.best, best)
    finally:
        plan.close()
