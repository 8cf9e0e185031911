"""Match uniqueness on the GPU: sm_census_second, sm_sgm_wta2, sm_uniqueness_filter and sm_confidence against the numpy
definition (tests/unique_reference.py), exactly, on the cases of tests/unique_patterns.py (test_unique_cpu.py shows
what they can tell).  Every expected value comes from the CPU definitions; none from the HIP path."""
import ctypes as C

import numpy as np
import pytest
import torch

from stereomatching_amd import capi
from stereomatching_amd.capi import lib
from stereomatching_amd.synth import make_pair
from tests import census_reference as cr
from tests import unique_patterns as up
from tests import unique_reference as ur
from tests.guarded import guarded_input
from tests.test_write_bounds_gpu import P, Plan, expect, out, report, stream, twice

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()             # (a copy: the cases' arrays are read-only)


def host(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------------------
# exactness
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(up.CENSUS_CASES))
def test_census_second_is_exact(hip, name):
    """web2 / best2 against four maps, on 2 pairs of a plan of 3; the zero map gives census_wta's own maps"""
    c, e = up.CENSUS_CASES[name], up.census_case(name)
    plan = hip.StereoPlan(c["w"], c["h"], c["d"], c["sw"], c["mode"], max_pairs=up.MAX_PAIRS)
    try:
        gl, gr = dev(e["left"]), dev(e["right"])
        web, best = plan.census_wta(gl, gr, c["census"])
        assert np.array_equal(host(web), e["web"]) and np.array_equal(host(best), e["best"])
        for kind in up.MAPS:
            gm = dev(e["maps"][kind])
            web2, best2 = plan.census_second(gl, gr, gm, c["census"])
            torch.cuda.synchronize()
            assert np.array_equal(host(web2), e["second"][kind][1]), kind
            assert np.array_equal(host(best2), e["second"][kind][0]), kind
            assert np.array_equal(host(gm), e["maps"][kind]), kind
            only, none = plan.census_second(gl, gr, gm, c["census"], want_best=False)
            assert none is None and torch.equal(only, web2), kind
            if kind == "zeros":
                assert torch.equal(web2, web) and torch.equal(best2, best)
    finally:
        plan.close()


@pytest.mark.parametrize("name", list(up.SGM_CASES))
def test_sgm_wta2_is_exact(hip, name):
    """all five maps, and web / best / sub against sm_sgm_wta on the same plan"""
    c, e = up.SGM_CASES[name], up.sgm_case(name)
    plan = hip.StereoPlan(c["w"], c["h"], c["d"], c["sw"], c["mode"])
    try:
        gl, gr = dev(e["left"]), dev(e["right"])
        args = dict(census=c["census"], p1=c["p1"], p2=c["p2"], paths=c["paths"], want_sub=True)
        web, best, sub, web2, best2 = plan.sgm_wta2(gl, gr, **args)
        torch.cuda.synchronize()
        for key, got in (("web", web), ("best", best), ("sub", sub), ("web2", web2), ("best2", best2)):
            assert np.array_equal(host(got), e[key]), key
        one = plan.sgm_wta(gl, gr, **args)
        assert torch.equal(one[0], web) and torch.equal(one[1], best) and torch.equal(one[2], sub)
        only = plan.sgm_wta2(gl, gr, want_best=False, want_best2=False, **{**args, "want_sub": False})
        assert only[1] is None and only[2] is None and only[4] is None
        assert torch.equal(only[0], web) and torch.equal(only[3], web2)
    finally:
        plan.close()


def check_filter_and_confidence(plan, web, best, best2):
    """every ratio, out of place and in place, with and without the count; the confidence map"""
    gw, gb, gb2 = dev(web), dev(best), dev(best2)
    for ratio in up.RATIOS:
        want, rejected = ur.uniqueness_filter(web, best, best2, ratio)
        per_pair = [ur.uniqueness_filter(web[q], best[q], best2[q], ratio)[1] for q in range(web.shape[0])]
        assert sum(per_pair) == rejected
        got, rej = plan.uniqueness_filter(gw, gb, gb2, ratio, want_rejected=True)
        assert np.array_equal(host(got), want) and host(rej).tolist() == per_pair, ratio
        assert np.array_equal(host(plan.uniqueness_filter(gw, gb, gb2, ratio)), want), ratio
        place = gw.clone()
        same, rej = plan.uniqueness_filter(place, gb, gb2, ratio, out=place, want_rejected=True)
        assert same.data_ptr() == place.data_ptr()
        assert np.array_equal(host(place), want) and host(rej).tolist() == per_pair, ratio
    assert np.array_equal(host(plan.confidence(gw, gb, gb2)), ur.confidence(web, best, best2))
    assert np.array_equal(host(gw), web) and np.array_equal(host(gb), best) and np.array_equal(host(gb2), best2)


@pytest.mark.parametrize("case", up.FILTER_CASES, ids=up.filter_id)
def test_filter_and_confidence_are_exact(hip, case):
    web, best, best2, w, h, d = up.filter_inputs(case)
    plan = hip.StereoPlan(w, h, d, 1, "ghost", max_pairs=up.MAX_PAIRS)
    try:
        check_filter_and_confidence(plan, web, best, best2)
    finally:
        plan.close()


def test_filter_and_confidence_on_the_extremes_of_int32(hip):
    """INT32_MIN, INT32_MAX, negative best, best2 = 0: the products and the quotient are 64-bit"""
    web, best, best2 = up.extremes()
    plan = hip.StereoPlan(web.shape[2], web.shape[1], 5, 1, "toroidal", max_pairs=2)
    try:
        check_filter_and_confidence(plan, web, best, best2)
    finally:
        plan.close()


# ---------------------------------------------------------------------------
# write bounds (tests/guarded.py)
# ---------------------------------------------------------------------------

def test_every_entry_writes_its_maps_and_nothing_else():
    """each output at a 16-byte aligned and at a 4-mod-16 offset, partial batches; NULL optional maps write nothing;
    the inputs stay as they were"""
    bad = []
    pairs, maxp = up.PAIRS, up.MAX_PAIRS
    for name in ("33x17 D45", "64x16 D130", "65x20 D16"):
        c, e = up.CENSUS_CASES[name], up.census_case(name)
        w, h = c["w"], c["h"]
        plan = Plan(w, h, c["d"], c["sw"], c["mode"], maxp)
        shp, s = (pairs, h, w), stream()
        gl, gr = guarded_input(e["left"], "cuda", 0, "left"), guarded_input(e["right"], "cuda", 1, "right")
        gm = guarded_input(e["maps"]["checked"], "cuda", 4, "map")
        gb = guarded_input(e["best"], "cuda", 0, "best")
        gb2 = guarded_input(e["second"]["checked"][0], "cuda", 4, "best2")
        want_f, _ = ur.uniqueness_filter(e["maps"]["checked"], e["best"], e["second"]["checked"][0], 15)
        want_r = [ur.uniqueness_filter(e["maps"]["checked"][q], e["best"][q], e["second"]["checked"][0][q], 15)[1]
                  for q in range(pairs)]
        want_c = ur.confidence(e["maps"]["checked"], e["best"], e["second"]["checked"][0])
        for off in (0, 4):
            t = f"{name} sm_census_second offset {off}"
            ow, ob = out(shp, torch.int32, off, maxp, "web2"), out(shp, torch.int32, 4 - off, maxp, "best2")
            bad += twice(t, lambda r: lib.sm_census_second(plan.h, P(gl.t), P(gr.t), c["census"], pairs, P(gm.t), P(ow.t),
                                                           P(ob.t), s), [ow, ob], [gl, gr, gm])
            bad += expect(t, ow, e["second"]["checked"][1]) + expect(t, ob, e["second"]["checked"][0])
            t = f"{name} sm_census_second (no best2) offset {off}"
            ow = out(shp, torch.int32, off, maxp, "web2")
            bad += twice(t, lambda r: lib.sm_census_second(plan.h, P(gl.t), P(gr.t), c["census"], pairs, P(gm.t), P(ow.t),
                                                           None, s), [ow], [gl, gr, gm])
            bad += expect(t, ow, e["second"]["checked"][1])
            t = f"{name} sm_uniqueness_filter offset {off}"
            oo, orj = out(shp, torch.int32, off, maxp, "out"), out((pairs,), torch.int32, off, maxp, "rejected")
            bad += twice(t, lambda r: lib.sm_uniqueness_filter(plan.h, P(gm.t), P(gb.t), P(gb2.t), 15, pairs, P(oo.t),
                                                               P(orj.t), s), [oo, orj], [gm, gb, gb2])
            bad += expect(t, oo, want_f) + expect(t, orj, want_r)
            t = f"{name} sm_uniqueness_filter (no count) offset {off}"
            oo = out(shp, torch.int32, off, maxp, "out")
            bad += twice(t, lambda r: lib.sm_uniqueness_filter(plan.h, P(gm.t), P(gb.t), P(gb2.t), 15, pairs, P(oo.t),
                                                               None, s), [oo], [gm, gb, gb2])
            bad += expect(t, oo, want_f)
            t = f"{name} sm_confidence offset {off}"
            oc = out(shp, torch.uint8, 1 if off == 0 else 4, maxp, "conf")       # (a byte map: odd, and 4 mod 16)
            bad += twice(t, lambda r: lib.sm_confidence(plan.h, P(gm.t), P(gb.t), P(gb2.t), pairs, P(oc.t), s), [oc],
                         [gm, gb, gb2])
            bad += expect(t, oc, want_c)
        oc = out(shp, torch.uint8, 0, maxp, "conf")
        bad += twice(f"{name} sm_confidence aligned", lambda r: lib.sm_confidence(plan.h, P(gm.t), P(gb.t), P(gb2.t), pairs,
                                                                                   P(oc.t), s), [oc], [gm, gb, gb2])
        bad += expect(f"{name} sm_confidence aligned", oc, want_c)
        plan.close()
    for name in ("70x20 D24 K1", "70x20 D200 K4", "20x9 D3"):
        c, e = up.SGM_CASES[name], up.sgm_case(name)
        w, h = c["w"], c["h"]
        plan = Plan(w, h, c["d"], c["sw"], c["mode"], 2)
        shp, s = (1, h, w), stream()
        gl, gr = guarded_input(e["left"], "cuda", 1, "left"), guarded_input(e["right"], "cuda", 0, "right")
        call = lambda m: lib.sm_sgm_wta2(plan.h, P(gl.t), P(gr.t), c["census"], c["p1"], c["p2"], c["paths"], 1, *m, s)   # noqa: E731
        for off in (0, 4):
            t = f"{name} sm_sgm_wta2 offset {off}"
            ow, ob, ow2, ob2 = (out(shp, torch.int32, o, 2, n) for o, n in ((off, "web"), (4 - off, "best"),
                                                                           (4 - off, "web2"), (off, "best2")))
            osb = out(shp, torch.int16, off // 2, 2, "sub")
            bad += twice(t, lambda r: call([P(ow.t), P(ob.t), P(osb.t), P(ow2.t), P(ob2.t)]), [ow, ob, osb, ow2, ob2],
                         [gl, gr])
            for g, key in ((ow, "web"), (ob, "best"), (osb, "sub"), (ow2, "web2"), (ob2, "best2")):
                bad += expect(t, g, e[key])
            t = f"{name} sm_sgm_wta2 (web and web2 only) offset {off}"
            ow, ow2 = out(shp, torch.int32, off, 2, "web"), out(shp, torch.int32, off, 2, "web2")
            bad += twice(t, lambda r: call([P(ow.t), None, None, P(ow2.t), None]), [ow, ow2], [gl, gr])
            bad += expect(t, ow, e["web"]) + expect(t, ow2, e["web2"])
        plan.close()
    report(bad)


# ---------------------------------------------------------------------------
# arguments, workspace, capture
# ---------------------------------------------------------------------------

def test_argument_checks_on_a_plan(hip):
    w, h, d = 64, 32, 16
    plan = hip.StereoPlan(w, h, d, 5, "toroidal", max_pairs=2)
    base = plan.workspace_bytes()
    m = [torch.zeros((2, h, w), dtype=torch.int32, device="cuda") for _ in range(6)]
    p = [C.c_void_p(t.data_ptr()) for t in m]
    g = torch.zeros((4, h, w), dtype=torch.uint8, device="cuda")
    gp, gq = C.c_void_p(g.data_ptr()), C.c_void_p(g.data_ptr() + 2 * w * h)
    cf = torch.zeros((2, h, w), dtype=torch.uint8, device="cuda")
    sb = torch.zeros((2, h, w), dtype=torch.int16, device="cuda")
    pc, ps = C.c_void_p(cf.data_ptr()), C.c_void_p(sb.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    inside = C.c_void_p(m[0].data_ptr() + 4)
    in_image = C.c_void_p(g.data_ptr() + 2 * w * h - 4)      # starts inside the left images, ends inside the right ones
    in_map = C.c_void_p(m[3].data_ptr() + 2 * w * h * 4 - 4)     # shares the last element of m[3]
    null = None

    def refused(rc, text):
        assert rc == capi.SM_ERR_ARG and text in lib.sm_last_error(), lib.sm_last_error()

    f, me = lib.sm_census_second, b"sm_census_second"
    refused(f(plan._h, null, gq, 7, 1, p[3], p[0], null, st), me + b": input image pointer is NULL")
    refused(f(plan._h, gp, gq, 7, 1, null, p[0], null, st), me + b": d_web is NULL")
    refused(f(plan._h, gp, gq, 7, 1, p[3], null, null, st), me + b": d_web2 is NULL")
    refused(f(plan._h, gp, gq, 4, 1, p[3], p[0], null, st), me + b": census_width 4 is not 3, 5 or 7")
    refused(f(None, gp, gq, 7, 1, p[3], p[0], null, st), me)
    refused(f(plan._h, gp, gq, 7, 3, p[3], p[0], null, st), me + b": pairs 3 outside 1..2")
    refused(f(plan._h, gp, gq, 7, 0, p[3], p[0], null, st), me + b": pairs 0 outside 1..2")
    refused(f(plan._h, gp, gq, 7, 1, p[3], p[0], inside, st), me + b": d_web2 and d_best2 overlap")
    refused(f(plan._h, gp, gq, 7, 2, p[3], in_image, null, st), me + b": an output overlaps an input image")
    refused(f(plan._h, gp, gq, 7, 2, p[3], p[0], gq, st), me + b": an output overlaps an input image")
    refused(f(plan._h, gp, gq, 7, 2, p[3], p[3], null, st), me + b": an output overlaps the input map")
    refused(f(plan._h, gp, gq, 7, 2, p[3], in_map, null, st), me + b": an output overlaps the input map")
    refused(f(plan._h, gp, gq, 7, 2, p[3], p[0], p[3], st), me + b": an output overlaps the input map")

    f, me = lib.sm_sgm_wta2, b"sm_sgm_wta2"
    refused(f(plan._h, gp, null, 7, 10, 120, 8, 1, p[0], null, null, p[1], null, st), me + b": input image pointer is NULL")
    refused(f(plan._h, gp, gq, 7, 10, 120, 8, 1, null, null, null, p[1], null, st), me + b": d_web is NULL")
    refused(f(plan._h, gp, gq, 7, 10, 120, 8, 1, p[0], null, null, null, null, st), me + b": d_web2 is NULL")
    refused(f(plan._h, gp, gq, 6, 10, 120, 8, 1, p[0], null, null, p[1], null, st), me + b": census_width 6 is not 3, 5 or 7")
    refused(f(plan._h, gp, gq, 7, 10, 120, 5, 1, p[0], null, null, p[1], null, st), me + b": paths 5 is not 4 or 8")
    refused(f(plan._h, gp, gq, 7, 10, 5, 8, 1, p[0], null, null, p[1], null, st), me + b": penalties p1 10, p2 5 break")
    refused(f(plan._h, gp, gq, 7, 10, 40000, 8, 1, p[0], null, null, p[1], null, st), me + b": penalties p1 10, p2 40000")
    refused(f(plan._h, gp, gq, 7, 10, 120, 8, 3, p[0], null, null, p[1], null, st), me + b": pairs 3 outside 1..2")
    for maps in ((p[0], null, null, p[0], null), (p[0], null, null, inside, null), (p[0], p[1], null, p[2], p[1]),
                 (p[0], p[1], null, p[2], inside), (p[0], null, ps, p[2], ps), (p[0], p[1], null, p[1], null),
                 (p[0], null, C.c_void_p(m[2].data_ptr() + 8), p[2], null)):
        refused(f(plan._h, gp, gq, 7, 10, 120, 8, 1, *maps, st), me + b": result maps overlap")
    for maps in ((p[0], null, null, in_image, null), (p[0], null, null, p[1], gq), (in_image, null, null, p[1], null),
                 (p[0], null, gp, p[1], null)):
        refused(f(plan._h, gp, gq, 7, 10, 120, 8, 2, *maps, st), me + b": an output overlaps an input image")

    f, me = lib.sm_uniqueness_filter, b"sm_uniqueness_filter"
    for k in range(4):
        a = [p[0], p[1], p[2], p[3]]
        a[k] = null
        refused(f(plan._h, a[0], a[1], a[2], 15, 2, a[3], null, st), me + b": a map pointer is NULL")
    refused(f(plan._h, p[0], p[1], p[2], -1, 2, p[3], null, st), me + b": ratio -1 outside 0..100")
    refused(f(plan._h, p[0], p[1], p[2], 101, 2, p[3], null, st), me + b": ratio 101 outside 0..100")
    refused(f(None, p[0], p[1], p[2], 15, 2, p[3], null, st), me)
    refused(f(plan._h, p[0], p[1], p[2], 15, 3, p[3], null, st), me + b": pairs 3 outside 1..2")
    refused(f(plan._h, p[0], p[1], p[2], 15, 1, inside, null, st), me + b": maps overlap without d_out being d_web")
    refused(f(plan._h, p[0], p[1], p[2], 15, 2, p[1], null, st), me + b": maps overlap without d_out being d_web")
    refused(f(plan._h, p[0], p[1], p[3], 15, 2, in_map, null, st), me + b": maps overlap without d_out being d_web")
    for k in (0, 1, 2, 4):
        refused(f(plan._h, p[0], p[1], p[2], 15, 2, p[4], C.c_void_p(m[k].data_ptr() + 16), st),
                me + b": d_rejected overlaps a map")
    assert f(plan._h, p[0], p[1], p[2], 15, 2, p[0], p[5], st) == capi.SM_OK          # in place is accepted

    f, me = lib.sm_confidence, b"sm_confidence"
    for k in range(4):
        a = [p[0], p[1], p[2], pc]
        a[k] = null
        refused(f(plan._h, a[0], a[1], a[2], 2, a[3], st), me + b": a map pointer is NULL")
    refused(f(None, p[0], p[1], p[2], 2, pc, st), me)
    refused(f(plan._h, p[0], p[1], p[2], 0, pc, st), me + b": pairs 0 outside 1..2")
    for k in range(3):
        refused(f(plan._h, p[0], p[1], p[2], 2, C.c_void_p(m[k].data_ptr() + 2 * w * h * 4 - 1), st),
                me + b": d_conf overlaps a map")
    torch.cuda.synchronize()
    assert plan.workspace_bytes() == base
    plan.close()
    for pw, ph, pd, psw, text, which in ((64, 32, 16, 27, b"windows up to 25x25", "both"),
                                         (64, 32, 513, 5, b"at most 512 shifts", "census"),
                                         (64, 32, 257, 5, b"at most 256 shifts", "sgm")):
        plan = hip.StereoPlan(pw, ph, pd, psw, "toroidal")
        base = plan.workspace_bytes()
        q = [C.c_void_p(t.data_ptr()) for t in (torch.zeros((1, ph, pw), dtype=torch.int32, device="cuda") for _ in range(3))]
        gg = torch.zeros((2, ph, pw), dtype=torch.uint8, device="cuda")
        a, b = C.c_void_p(gg.data_ptr()), C.c_void_p(gg.data_ptr() + pw * ph)
        if which in ("both", "census"):
            refused(lib.sm_census_second(plan._h, a, b, 7, 1, q[0], q[1], null, st), b"sm_census_second: built for")
            assert text in lib.sm_last_error()
        if which in ("both", "sgm"):
            refused(lib.sm_sgm_wta2(plan._h, a, b, 7, 10, 120, 8, 1, q[0], null, null, q[1], null, st), b"sm_sgm_wta2: built for")
            assert text in lib.sm_last_error()
        assert plan.workspace_bytes() == base
        plan.close()


def test_workspace_contents_do_not_matter(hip):
    """sm_census_second and sm_sgm_wta2 give the same maps whatever the workspace held"""
    name = "33x17 D45"
    c, e = up.CENSUS_CASES[name], up.census_case(name)
    plan = hip.StereoPlan(c["w"], c["h"], c["d"], c["sw"], c["mode"], max_pairs=up.MAX_PAIRS)
    try:
        gl, gr, gm = dev(e["left"]), dev(e["right"]), dev(e["maps"]["own"])
        plan.reserve_census()
        for word in (0xFFFFFFFF, 0x00000000, 0xA5A5A5A5):
            plan._poison_workspace(word)
            web2, best2 = plan.census_second(gl, gr, gm, c["census"])
            assert np.array_equal(host(web2), e["second"]["own"][1]), hex(word)
            assert np.array_equal(host(best2), e["second"]["own"][0]), hex(word)
    finally:
        plan.close()
    name = "70x20 D24 K1"
    c, e = up.SGM_CASES[name], up.sgm_case(name)
    plan = hip.StereoPlan(c["w"], c["h"], c["d"], c["sw"], c["mode"])
    try:
        gl, gr = dev(e["left"]), dev(e["right"])
        plan.reserve_sgm()
        for word in (0xFFFFFFFF, 0x00000000, 0xA5A5A5A5):
            plan._poison_workspace(word)
            got = plan.sgm_wta2(gl, gr, c["census"], c["p1"], c["p2"], c["paths"], want_sub=True)
            for key, t in zip(("web", "best", "sub", "web2", "best2"), got):
                assert np.array_equal(host(t), e[key]), (key, hex(word))
    finally:
        plan.close()


def test_captured_into_a_graph(hip):
    """refused before the reservations with the capture left valid; then census_second -> uniqueness_filter ->
    confidence captured once and replayed on three inputs"""
    from stereomatching_amd import pipeline
    w, h, d, sw, census, mode = 130, 40, 48, 5, 7, "ghost"
    pairs = [make_pair(w, h, d, seed=90 + i) for i in range(3)]
    left_in = torch.zeros((1, h, w), dtype=torch.uint8, device="cuda")
    right_in = torch.zeros_like(left_in)
    web_in, best_in = (torch.zeros((1, h, w), dtype=torch.int32, device="cuda") for _ in range(2))
    web2, best2, kept, web_s, best_s = (torch.zeros((1, h, w), dtype=torch.int32, device="cuda") for _ in range(5))
    conf = torch.zeros((1, h, w), dtype=torch.uint8, device="cuda")
    rej = torch.zeros(1, dtype=torch.int32, device="cuda")
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        base = plan.workspace_bytes()
        for call, text in ((lambda: plan.census_second(left_in, right_in, web_in, census, web2=web2, best2=best2),
                            "sm_plan_reserve_census"),
                           (lambda: plan.sgm_wta2(left_in, right_in, census, web=web_s, best=best_s, web2=web2, best2=best2),
                            "sm_plan_reserve_sgm")):
            with pytest.raises(capi.StereoHipError, match=text):
                with torch.cuda.graph(torch.cuda.CUDAGraph(), capture_error_mode="thread_local"):
                    call()
        assert plan.workspace_bytes() == base
        plan.reserve_census()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            pipeline.check(lib.sm_census_second(plan._h, P(left_in), P(right_in), census, 1, P(web_in), P(web2), P(best2),
                                                plan._stream()))
            pipeline.check(lib.sm_uniqueness_filter(plan._h, P(web_in), P(best_in), P(best2), 15, 1, P(kept), P(rej),
                                                    plan._stream()))
            pipeline.check(lib.sm_confidence(plan._h, P(kept), P(best_in), P(best2), 1, P(conf), plan._stream()))
        for rep in (1, 2, 0):
            l, r = pairs[rep]
            best, web = cr.wta(l, r, d, sw, census, mode)
            left_in.copy_(dev(l))
            right_in.copy_(dev(r))
            web_in.copy_(dev(web))
            best_in.copy_(dev(best))
            for t in (web2, best2, kept, conf):
                t.zero_()
            rej.fill_(12345)
            g.replay()
            torch.cuda.synchronize()
            b2, w2 = ur.census_second(l, r, web, d, sw, census, mode)
            want, rejected = ur.uniqueness_filter(web, best, b2, 15)
            assert np.array_equal(host(web2)[0], w2) and np.array_equal(host(best2)[0], b2), rep
            assert np.array_equal(host(kept)[0], want) and int(rej[0]) == rejected and rejected > 0, rep
            assert np.array_equal(host(conf)[0], ur.confidence(want, best, b2)), rep
    finally:
        plan.close()


def test_chain_through_the_binding(hip):
    """census_lr -> census_second -> uniqueness_filter -> sub_mask -> confidence, every stage against its CPU
    definition"""
    w, h, d, n, census, mode = 130, 34, 24, 5, 7, "ghost"
    left, right = make_pair(w, h, d, seed=5)
    plan = hip.StereoPlan(w, h, d, n, mode)
    try:
        gl, gr = dev(left[None]), dev(right[None])
        res = plan.census_lr(gl, gr, census, max_diff=1, want_best=True)
        e = cr.expected(left, right, d, n, census, mode, 1)
        assert np.array_equal(host(res.web)[0], e["checked"]) and np.array_equal(host(res.best)[0], e["best"])
        web2, best2 = plan.census_second(gl, gr, res.web, census)
        b2, w2 = ur.census_second(left, right, e["checked"], d, n, census, mode)
        assert np.array_equal(host(web2)[0], w2) and np.array_equal(host(best2)[0], b2)
        kept, rej = plan.uniqueness_filter(res.web, res.best, best2, 15, want_rejected=True)
        want, rejected = ur.uniqueness_filter(e["checked"], e["best"], b2, 15)
        assert np.array_equal(host(kept)[0], want) and int(rej[0]) == rejected and 0 < rejected < (want != 0).sum()
        sub, _ = plan.census_refine(gl, gr, res.web, census)
        sub = plan.sub_mask(kept, sub)
        want_sub = np.where(want == 0, 0, cr.refine(left, right, e["checked"], d, n, census, mode)[0])
        assert np.array_equal(host(sub)[0], want_sub)
        conf = plan.confidence(kept, res.best, best2)
        assert np.array_equal(host(conf)[0], ur.confidence(want, e["best"], b2))
        # SGM: winner and runner-up in one call feed the same filter
        web, best, _, web2, best2 = plan.sgm_wta2(gl, gr, census, p1=60, p2=600, paths=8)
        s = ur.sgm_wta2(left, right, d, n, census, 60, 600, 8, mode)
        assert np.array_equal(host(web)[0], s["web"]) and np.array_equal(host(best2)[0], s["best2"])
        assert np.array_equal(host(web2)[0], s["web2"])
        kept = plan.uniqueness_filter(web, best, best2, 10)
        assert np.array_equal(host(kept)[0], ur.uniqueness_filter(s["web"], s["best"], s["best2"], 10)[0])
    finally:
        plan.close()
