"""The cross-based matcher on the GPU: sm_cross_arms, sm_cross_wta, sm_cross_wta_right and sm_cross_lr against the numpy
definition (tests/cross_reference.py).  Every comparison is exact equality; every expected value
comes from the CPU definitions, none from the HIP path (but the identity test, which holds the GPU's cross matcher
against the GPU's census matcher)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from stereomatching_amd import capi
from stereomatching_amd.capi import lib
from tests import census_reference as cr
from tests import cross_patterns as cp
from tests import cross_reference as x
from tests import workspace_poison_cases as wc

pytestmark = pytest.mark.gpu
MODES = ["toroidal", "ghost"]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


regions = cp.regions


@functools.lru_cache(maxsize=None)
def expected(w, h, d, census, tau, arm, mode, md, pairs, seed):
    left, right = cp.related_pairs(w, h, pairs, seed)
    rows = [x.expected(left[q], right[q], d, census, tau, arm, mode, md) for q in range(pairs)]
    return left, right, {k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0]}


@pytest.mark.parametrize("w,h", [(70, 45), (64, 16), (65, 17), (9, 40), (1, 1)])
def test_arms_and_support_are_exact(hip, w, h):
    imgs = regions(w, h, 3, 7 * w + h)
    plan = hip.StereoPlan(w, h, 4, 1, "toroidal", max_pairs=2)
    try:
        base = plan.workspace_bytes()
        g = dev(imgs)
        for tau in (0, 12, 255):
            for arm in (0, 1, 7, 15):
                arms, support = plan.cross_arms(g, tau, arm, want_support=True)
                only, none = plan.cross_arms(g, tau, arm)
                assert none is None and arms.dtype == torch.uint16 and tuple(arms.shape) == (3, h, w)
                ga, gs, go = host(arms), host(support), host(only)
                for i in range(3):
                    a = x.arms(imgs[i], tau, arm)
                    assert np.array_equal(ga[i], x.pack(a)), (tau, arm, i)
                    assert np.array_equal(go[i], x.pack(a)), (tau, arm, i)
                    assert np.array_equal(gs[i], x.support(a)), (tau, arm, i)
        assert plan.workspace_bytes() == base                # needs no workspace
    finally:
        plan.close()


CASES = cp.CASES


@pytest.mark.parametrize("census", [3, 5, 7])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("w,h,d,arm,tau", CASES)
def test_every_map_is_exact(hip, census, mode, w, h, d, arm, tau):
    """web / best / sub, web_right / best_right, the checked map, rejected and sub with 0 where rejected: three pairs
    with a distinct image in every slot, on a plan of four"""
    pairs, md = 3, (w + d) % 2
    left, right, e = expected(w, h, d, census, tau, arm, mode, md, pairs, 100 * census + d + arm)
    plan = hip.StereoPlan(w, h, d, 9, mode, max_pairs=4)
    try:
        gl, gr = dev(left), dev(right)
        web, best, sub = plan.cross_wta(gl, gr, census, tau, arm, want_sub=True)
        web_right, best_right = plan.cross_wta_right(gl, gr, census, tau, arm)
        res = plan.cross_lr(gl, gr, census, tau, arm, max_diff=md, want_right=True, want_best=True, want_sub=True)
        torch.cuda.synchronize()
        tag = (census, mode, w, h, d, arm, tau)
        assert np.array_equal(host(web), e["web"]), tag
        assert np.array_equal(host(best), e["best"]), tag
        assert np.array_equal(host(sub), e["sub"]), tag
        assert np.array_equal(host(web_right), e["web_right"]), tag
        assert np.array_equal(host(best_right), e["best_right"]), tag
        assert np.array_equal(host(res.web), e["checked"]), tag
        assert np.array_equal(host(res.web_right), e["web_right"]), tag
        assert np.array_equal(host(res.best), e["best"]), tag
        assert host(res.rejected).tolist() == e["rejected"].tolist(), tag
        assert np.array_equal(host(res.sub), e["sub_checked"]), tag
    finally:
        plan.close()


@pytest.mark.parametrize("arm", [1, 4, 12])
def test_ghost_without_a_threshold_is_the_gpus_box_matcher(hip, arm):
    w, h, d = 70, 45, 20
    left, right = regions(w, h, 2, arm), regions(w, h, 2, 50 + arm)
    plan = hip.StereoPlan(w, h, d, 2 * arm + 1, "ghost", max_pairs=2)
    try:
        gl, gr = dev(left), dev(right)
        web, best, _ = plan.cross_wta(gl, gr, 7, 255, arm)
        box_web, box_best = plan.census_wta(gl, gr, 7)
        torch.cuda.synchronize()
        assert torch.equal(web, box_web) and torch.equal(best, box_best)
        assert host(best).max() > 0
    finally:
        plan.close()


EXTREMES = [("anti_0", 1), ("anti_D", 5), ("rows_anti", 20)]


# (the three cases of census 7, toroidal keep their ids; the others are the kernel's other instances: NW = 1, GHOST)
@pytest.mark.parametrize("name,d,census,mode",
                         [pytest.param(n, d, 7, "toroidal", id=f"{n}-{d}") for n, d in EXTREMES]
                         + [pytest.param(n, d, c, m, id=f"{n}-{d}-{c}-{m}") for c, m in ((5, "toroidal"), (7, "ghost"),
                                                                                         (5, "ghost")) for n, d in EXTREMES])
def test_extreme_pairs(hip, name, d, census, mode):
    """the bounds of the u16 fields, of the prefix sums and of the keys: E = (c^2 - 1) * 961 (48 * 961 at c = 7) at every
    pixel with a full support, the same value just past the range, and an all-tie map (above 2^15 at c = 7).  Ghost: what
    the definition gives, nothing more"""
    w, h = cp.EXTREME_W, cp.EXTREME_H
    left, right = {"anti_0": lambda: cp.anti(w, h, 0), "anti_D": lambda: cp.anti(w, h, d),
                   "rows_anti": lambda: cp.rows_anti(w, h)}[name]()
    e = x.expected(left, right, d, census, 255, 15, mode, 0)
    if mode == "toroidal":
        if name == "anti_0":
            assert int((e["best"] == (census * census - 1) * 961).sum()) == cp.EXTREME_INTERIOR
        if name == "rows_anti":
            assert (e["web"] == 1).all() and e["best"].max() == (census * census - census) * 961
            assert census != 7 or e["best"].max() > 2 ** 15
    plan = hip.StereoPlan(w, h, d, 1, mode)
    try:
        res = plan.cross_lr(dev(left), dev(right), census, 255, 15, max_diff=0, want_right=True, want_best=True,
                            want_sub=True)
        web, best, sub = plan.cross_wta(dev(left), dev(right), census, 255, 15, want_sub=True)
        web_right, best_right = plan.cross_wta_right(dev(left), dev(right), census, 255, 15)
        torch.cuda.synchronize()
        assert np.array_equal(host(web)[0], e["web"]) and np.array_equal(host(best)[0], e["best"])
        assert np.array_equal(host(sub)[0], e["sub"])
        assert np.array_equal(host(web_right)[0], e["web_right"]) and np.array_equal(host(best_right)[0], e["best_right"])
        assert np.array_equal(host(res.web)[0], e["checked"]) and np.array_equal(host(res.best)[0], e["best"])
        assert np.array_equal(host(res.web_right)[0], e["web_right"])
        assert np.array_equal(host(res.sub)[0], e["sub_checked"]) and int(res.rejected[0]) == e["rejected"]
    finally:
        plan.close()


def test_occluder_scene(hip):
    scenes = [cp.occluder_scene(96, 64, seed, 3, 11) for seed in (1, 2, 3)]
    left, right = np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes])
    plan = hip.StereoPlan(96, 64, 16, 9, "ghost", max_pairs=3)
    try:
        res = plan.cross_lr(dev(left), dev(right), 7, 20, 10, max_diff=1, want_right=True, want_best=True, want_sub=True)
        torch.cuda.synchronize()
        for q, (l, r, truth) in enumerate(scenes):
            e = x.expected(l, r, 16, 7, 20, 10, "ghost", 1)
            assert np.array_equal(host(res.web)[q], e["checked"]) and np.array_equal(host(res.best)[q], e["best"])
            assert np.array_equal(host(res.web_right)[q], e["web_right"])
            assert np.array_equal(host(res.sub)[q], e["sub_checked"]) and int(res.rejected[q]) == e["rejected"]
    finally:
        plan.close()


@pytest.mark.parametrize("mode", MODES)
def test_results_do_not_depend_on_what_the_workspace_held(hip, mode):
    """poisoned before every call with each word of the list; cross and census_wta at widths 5 and 7 take turns on one
    plan: they share the descriptor row, 4-byte and 8-byte descriptors in the same memory"""
    w, h, d, sw, tau, arm, pairs = 70, 45, 12, 5, 40, 7, 2
    want = {c: expected(w, h, d, c, tau, arm, mode, 1, pairs, 900) for c in (5, 7)}
    left, right = want[5][0], want[5][1]
    box = {c: [cr.wta(left[q], right[q], d, sw, c, mode) for q in range(pairs)] for c in (5, 7)}
    plan = hip.StereoPlan(w, h, d, sw, mode, max_pairs=3)
    try:
        gl, gr = dev(left), dev(right)
        plan.reserve_cross()
        for word in wc.WORDS:
            for c in (7, 5):
                e = want[c][2]
                plan._poison_workspace(word)
                res = plan.cross_lr(gl, gr, c, tau, arm, max_diff=1, want_right=True, want_best=True, want_sub=True)
                torch.cuda.synchronize()
                tag = (hex(word), c)
                assert np.array_equal(host(res.web), e["checked"]), tag
                assert np.array_equal(host(res.web_right), e["web_right"]), tag
                assert np.array_equal(host(res.best), e["best"]), tag
                assert np.array_equal(host(res.sub), e["sub_checked"]), tag
                assert host(res.rejected).tolist() == e["rejected"].tolist(), tag
                plan._poison_workspace(word)
                web, best = plan.census_wta(gl, gr, 12 - c)          # the other descriptor size
                torch.cuda.synchronize()
                for q in range(pairs):
                    assert np.array_equal(host(best)[q], box[12 - c][q][0]), tag
                    assert np.array_equal(host(web)[q], box[12 - c][q][1]), tag
                plan._poison_workspace(word)
                web_right, best_right = plan.cross_wta_right(gl, gr, c, tau, arm)
                torch.cuda.synchronize()
                assert np.array_equal(host(web_right), e["web_right"]), tag
                assert np.array_equal(host(best_right), e["best_right"]), tag
    finally:
        plan.close()


def test_refusals_name_the_function_and_allocate_nothing(hip):
    w, h, d = 64, 32, 16
    plan = hip.StereoPlan(w, h, d, 5, "toroidal", max_pairs=2)
    base = plan.workspace_bytes()
    m = [torch.zeros((2, h, w), dtype=torch.int32, device="cuda") for _ in range(4)]
    p = [P(t) for t in m]
    g = torch.zeros((4, h, w), dtype=torch.uint8, device="cuda")
    gp, gq = P(g), C.c_void_p(g.data_ptr() + 2 * w * h)
    a16 = torch.zeros((4, h, w), dtype=torch.uint16, device="cuda")
    s16 = torch.zeros((2, h, w), dtype=torch.int16, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    inside = C.c_void_p(m[0].data_ptr() + 4)
    in_image = C.c_void_p(g.data_ptr() + 8)
    H = plan._h

    def refused(rc, text):
        assert rc == capi.SM_ERR_ARG and text in lib.sm_last_error(), lib.sm_last_error()
    # NULL pointers
    refused(lib.sm_cross_wta(H, None, gq, 7, 20, 10, 1, p[0], None, None, st), b"sm_cross_wta: input image pointer is NULL")
    refused(lib.sm_cross_wta(H, gp, gq, 7, 20, 10, 1, None, None, None, st), b"sm_cross_wta: d_web is NULL")
    refused(lib.sm_cross_wta_right(H, gp, None, 7, 20, 10, 1, p[0], None, st), b"sm_cross_wta_right: input image pointer is NULL")
    refused(lib.sm_cross_wta_right(H, gp, gq, 7, 20, 10, 1, None, None, st), b"sm_cross_wta_right: d_web_right is NULL")
    refused(lib.sm_cross_lr(H, gp, gq, 7, 20, 10, 1, 0, None, None, None, None, None, st), b"sm_cross_lr: d_web is NULL")
    refused(lib.sm_cross_wta(None, gp, gq, 7, 20, 10, 1, p[0], None, None, st), b"sm_cross_wta: plan is NULL")
    refused(lib.sm_cross_arms(H, None, 20, 10, 1, P(a16), None, st), b"sm_cross_arms: NULL argument")
    refused(lib.sm_cross_arms(H, gp, 20, 10, 1, None, None, st), b"sm_cross_arms: NULL argument")
    refused(lib.sm_cross_arms(None, gp, 20, 10, 1, P(a16), None, st), b"sm_cross_arms: plan is NULL")
    assert lib.sm_plan_reserve_cross(None) == capi.SM_ERR_ARG and b"sm_plan_reserve_cross: plan is NULL" in lib.sm_last_error()
    # the scalars, in the order of the checks: max_diff, census width, tau, arm, pairs
    refused(lib.sm_cross_lr(H, gp, gq, 4, -1, 16, 0, -1, p[0], None, None, None, None, st), b"sm_cross_lr: max_diff -1 is negative")
    refused(lib.sm_cross_lr(H, gp, gq, 4, -1, 16, 0, 0, p[0], None, None, None, None, st), b"sm_cross_lr: census_width 4 is not 3, 5 or 7")
    refused(lib.sm_cross_wta(H, gp, gq, 4, 20, 10, 1, p[0], None, None, st), b"sm_cross_wta: census_width 4 is not 3, 5 or 7")
    refused(lib.sm_cross_wta(H, gp, gq, 7, -1, 16, 0, p[0], None, None, st), b"sm_cross_wta: tau -1 outside 0..255")
    refused(lib.sm_cross_wta(H, gp, gq, 7, 256, 10, 1, p[0], None, None, st), b"sm_cross_wta: tau 256 outside 0..255")
    refused(lib.sm_cross_wta_right(H, gp, gq, 7, 20, -1, 0, p[0], None, st), b"sm_cross_wta_right: arm -1 outside 0..15")
    refused(lib.sm_cross_wta_right(H, gp, gq, 7, 20, 16, 1, p[0], None, st), b"sm_cross_wta_right: arm 16 outside 0..15")
    refused(lib.sm_cross_lr(H, gp, gq, 7, 20, 10, 0, 0, p[0], None, None, None, None, st), b"sm_cross_lr: pairs 0 outside 1..2")
    refused(lib.sm_cross_wta(H, gp, gq, 7, 20, 10, 3, p[0], None, None, st), b"sm_cross_wta: pairs 3 outside 1..2")
    refused(lib.sm_cross_arms(H, gp, -1, 10, 1, P(a16), None, st), b"sm_cross_arms: tau -1 outside 0..255")
    refused(lib.sm_cross_arms(H, gp, 256, 10, 1, P(a16), None, st), b"sm_cross_arms: tau 256")
    refused(lib.sm_cross_arms(H, gp, 20, 16, 1, P(a16), None, st), b"sm_cross_arms: arm 16 outside 0..15")
    refused(lib.sm_cross_arms(H, gp, 20, -1, 1, P(a16), None, st), b"sm_cross_arms: arm -1")
    refused(lib.sm_cross_arms(H, gp, 20, 10, 0, P(a16), None, st), b"sm_cross_arms: images 0 outside 1..4")
    refused(lib.sm_cross_arms(H, gp, 20, 10, 5, P(a16), None, st), b"sm_cross_arms: images 5 outside 1..4")
    # overlaps: an output with another output, with an image
    refused(lib.sm_cross_wta(H, gp, gq, 7, 20, 10, 1, p[0], inside, None, st), b"sm_cross_wta: result maps overlap")
    refused(lib.sm_cross_wta(H, gp, gq, 7, 20, 10, 1, p[0], None, inside, st), b"sm_cross_wta: result maps overlap")
    refused(lib.sm_cross_wta_right(H, gp, gq, 7, 20, 10, 1, p[0], inside, st), b"sm_cross_wta_right: result maps overlap")
    refused(lib.sm_cross_lr(H, gp, gq, 7, 20, 10, 1, 0, p[0], None, inside, None, None, st), b"sm_cross_lr: result maps overlap")
    refused(lib.sm_cross_lr(H, gp, gq, 7, 20, 10, 2, 0, p[0], p[1], None, inside, None, st), b"sm_cross_lr: d_rejected overlaps a map")
    refused(lib.sm_cross_wta(H, gp, gq, 7, 20, 10, 1, in_image, None, None, st), b"sm_cross_wta: an output overlaps an input image")
    refused(lib.sm_cross_wta(H, gp, gq, 7, 20, 10, 1, p[0], None, in_image, st), b"sm_cross_wta: an output overlaps an input image")
    refused(lib.sm_cross_wta_right(H, gp, gq, 7, 20, 10, 1, p[0], gq, st), b"sm_cross_wta_right: an output overlaps an input image")
    refused(lib.sm_cross_lr(H, gp, gq, 7, 20, 10, 1, 0, p[0], None, None, in_image, None, st), b"sm_cross_lr: an output overlaps an input image")
    refused(lib.sm_cross_lr(H, gp, gq, 7, 20, 10, 1, 0, p[0], None, None, None, in_image, st), b"sm_cross_lr: an output overlaps an input image")
    refused(lib.sm_cross_arms(H, gp, 20, 10, 1, in_image, None, st), b"sm_cross_arms: an output overlaps the input images")
    refused(lib.sm_cross_arms(H, gp, 20, 10, 1, P(a16), C.c_void_p(a16.data_ptr() + 4), st), b"sm_cross_arms: d_arms and d_support overlap")
    assert plan.workspace_bytes() == base and s16 is not None
    plan.close()
    # more shifts than the mode is built for; a window beyond the census limit is no obstacle (it plays no part)
    plan = hip.StereoPlan(64, 32, 513, 5, "toroidal")
    base = plan.workspace_bytes()
    for name, call in ((b"sm_cross_wta", lambda: lib.sm_cross_wta(plan._h, gp, gq, 7, 20, 10, 1, p[0], None, None, st)),
                       (b"sm_cross_wta_right", lambda: lib.sm_cross_wta_right(plan._h, gp, gq, 7, 20, 10, 1, p[0], None, st)),
                       (b"sm_cross_lr", lambda: lib.sm_cross_lr(plan._h, gp, gq, 7, 20, 10, 1, 0, p[0], None, None, None, None, st))):
        refused(call(), name + b": built for at most 512 shifts (got 513)")
    assert plan.workspace_bytes() == base
    plan.close()
    plan = hip.StereoPlan(64, 32, 8, 27, "ghost")
    try:
        l, r = regions(64, 32, 1, 1), regions(64, 32, 1, 2)
        web, best, _ = plan.cross_wta(dev(l), dev(r), 5, 20, 4)
        torch.cuda.synchronize()
        want_best, want_web = x.wta(l[0], r[0], 8, 5, 20, 4, "ghost")
        assert np.array_equal(host(web)[0], want_web) and np.array_equal(host(best)[0], want_best)
    finally:
        plan.close()


def test_workspace_is_the_census_one_and_the_arms(hip):
    w, h, d, mp = 70, 45, 12, 3
    plan = hip.StereoPlan(w, h, d, 5, "toroidal", max_pairs=mp)
    try:
        base = plan.workspace_bytes()
        plan.reserve_cross()
        plan.reserve_cross()                                 # idempotent
        census = 2 * mp * w * h * 8 + mp * w * h * 4         # descriptors and the mirrored-order map
        assert plan.workspace_bytes() == base + census + 4 * mp * w * h
        plan.reserve_census()                                # a part of it
        assert plan.workspace_bytes() == base + census + 4 * mp * w * h
    finally:
        plan.close()


def test_cross_lr_captured_into_a_graph(hip):
    w, h, d, census, tau, arm, mode = 130, 37, 24, 7, 40, 7, "ghost"
    left, right, e = expected(w, h, d, census, tau, arm, mode, 0, 3, 4000)
    left_in, right_in = torch.zeros_like(dev(left[:1])), torch.zeros_like(dev(right[:1]))
    plan = hip.StereoPlan(w, h, d, 5, mode)
    try:
        base = plan.workspace_bytes()
        web = torch.zeros((1, h, w), dtype=torch.int32, device="cuda")
        web_right, best = torch.zeros_like(web), torch.zeros_like(web)
        sub = torch.zeros((1, h, w), dtype=torch.int16, device="cuda")
        # refused before reserve_cross, and the capture stays valid (it ends cleanly; the pending error is raised)
        for call in (lambda: plan.cross_lr(left_in, right_in, census, tau, arm, web=web),
                     lambda: plan.cross_wta(left_in, right_in, census, tau, arm, want_best=False, web=web),
                     lambda: plan.cross_wta_right(left_in, right_in, census, tau, arm, want_best=False, web_right=web_right)):
            with pytest.raises(capi.StereoHipError, match="sm_plan_reserve_cross"):
                with torch.cuda.graph(torch.cuda.CUDAGraph(), capture_error_mode="thread_local"):
                    call()
        assert plan.workspace_bytes() == base
        plan.reserve_cross()
        rej = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        from stereomatching_amd import pipeline
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            pipeline.check(lib.sm_cross_lr(plan._h, P(left_in), P(right_in), census, tau, arm, 1, 0, P(web), P(best),
                                           P(web_right), P(rej), P(sub), plan._stream()))
        for q in (1, 2, 0):
            left_in.copy_(dev(left[q:q + 1]))
            right_in.copy_(dev(right[q:q + 1]))
            for t in (web, web_right, best, sub):
                t.zero_()
            rej.fill_(12345)
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(host(web)[0], e["checked"][q]), q
            assert np.array_equal(host(web_right)[0], e["web_right"][q]), q
            assert np.array_equal(host(best)[0], e["best"][q]), q
            assert np.array_equal(host(sub)[0], e["sub_checked"][q]), q
            assert int(rej[0]) == int(e["rejected"][q]), q
    finally:
        plan.close()
