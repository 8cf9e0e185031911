"""The guided census re-search on the GPU: sm_census_wta_near, sm_census_wta_near_right and sm_census_near_lr against
the numpy definition (tests/near_reference.py), exactly, on the cases of tests/near_patterns.py (test_near_cpu.py
shows what they can tell).  Every expected value comes from the CPU definitions; none from the HIP path."""
import ctypes as C

import numpy as np
import pytest
import torch

from stereomatching_amd import capi
from stereomatching_amd.capi import lib
from stereomatching_amd.synth import make_pair
from tests import census_reference as cr
from tests import near_patterns as npat
from tests import near_reference as nr
from tests import pyramid_reference as pr
from tests.guarded import guarded_input
from tests.test_write_bounds_gpu import P, Plan, expect, out, report, stream, twice

pytestmark = pytest.mark.gpu
MODES = ["toroidal", "ghost"]


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()             # (a copy: the cases' arrays are read-only)


def host(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("name", [c["name"] for c in npat.CASES])
def test_every_map_is_exact(hip, name):
    """web / best of the left and of the right search, and the checked map, the right map, the costs and the count of
    sm_census_near_lr, on a full or a partial batch of a plan of three pairs"""
    c = npat.BY_NAME[name]
    left, right, prior, prior_right = npat.inputs(name)
    plan = hip.StereoPlan(c["w"], c["h"], c["d"], c["sw"], c["mode"], max_pairs=npat.MAX_PAIRS)
    try:
        gl, gr, gp, gpr = dev(left), dev(right), dev(prior), dev(prior_right)
        web, best = plan.census_wta_near(gl, gr, gp, c["census"], c["radius"])
        web_right, best_right = plan.census_wta_near_right(gl, gr, gpr, c["census"], c["radius"])
        res = plan.census_near_lr(gl, gr, gp, gpr, c["census"], c["radius"], max_diff=c["max_diff"], want_right=True,
                                  want_best=True)
        torch.cuda.synchronize()
        assert np.array_equal(host(web), npat.stacked(name, "web"))
        assert np.array_equal(host(best), npat.stacked(name, "best"))
        assert np.array_equal(host(web_right), npat.stacked(name, "web_right"))
        assert np.array_equal(host(best_right), npat.stacked(name, "best_right"))
        assert np.array_equal(host(res.web), npat.stacked(name, "checked"))
        assert np.array_equal(host(res.web_right), npat.stacked(name, "web_right"))
        assert np.array_equal(host(res.best), npat.stacked(name, "best"))
        assert host(res.rejected).tolist() == [e["rejected"] for e in npat.expected(name)]
        assert np.array_equal(host(gp), prior) and np.array_equal(host(gpr), prior_right)
    finally:
        plan.close()


# ---------------------------------------------------------------------------
# write bounds (tests/guarded.py)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_near_writes_its_maps_and_nothing_else(mode):
    """every entry, each output at a 16-byte aligned and a 4-byte-but-not-16 offset, partial batches; a NULL d_best
    writes nothing"""
    bad = []
    for idx, (w, h, d, sw, census, radius) in enumerate([(33, 17, 45, 3, 7, 1), (64, 16, 130, 5, 3, 2),
                                                         (65, 20, 16, 9, 5, 4), (129, 5, 40, 1, 7, 2)]):
        pairs, maxp = (2, 3) if idx % 2 == 0 else (1, 2)
        plan = Plan(w, h, d, sw, mode, maxp)
        tag = f"{mode} c={census} r={radius} W={w} H={h} D={d} S={sw} pairs={pairs}/{maxp}"
        rng = np.random.default_rng(idx + 60)
        left = rng.integers(0, 256, (pairs, h, w)).astype(np.uint8)
        right = rng.integers(0, 256, (pairs, h, w)).astype(np.uint8)
        prior = np.stack([npat.make_prior(("zeros30", "noise")[idx % 2], w, h, d, radius, rng) for _ in range(pairs)])
        prior_right = np.stack([npat.make_prior("extremes", w, h, d, radius, rng) for _ in range(pairs)])
        want = [nr.expected(left[q], right[q], prior[q], prior_right[q], d, sw, census, radius, mode, 1)
                for q in range(pairs)]
        Wt = lambda k: np.stack([x[k] for x in want])     # noqa: E731
        shp, s = (pairs, h, w), stream()
        gl, gr = guarded_input(left, "cuda", idx % 2, "left"), guarded_input(right, "cuda", 0, "right")
        gp, gpr = guarded_input(prior, "cuda", 4, "prior"), guarded_input(prior_right, "cuda", 0, "prior_right")
        for off in (0, 4):
            t = f"{tag} sm_census_wta_near offset {off}"
            ow, ob = out(shp, torch.int32, off, maxp, "web"), out(shp, torch.int32, 4 - off, maxp, "best")
            bad += twice(t, lambda r: lib.sm_census_wta_near(plan.h, P(gl.t), P(gr.t), census, pairs, P(gp.t), radius,
                                                             P(ow.t), P(ob.t), s), [ow, ob], [gl, gr, gp])
            bad += expect(t, ow, Wt("web")) + expect(t, ob, Wt("best"))
            t = f"{tag} sm_census_wta_near (no best) offset {off}"
            ow = out(shp, torch.int32, off, maxp, "web")
            bad += twice(t, lambda r: lib.sm_census_wta_near(plan.h, P(gl.t), P(gr.t), census, pairs, P(gp.t), radius,
                                                             P(ow.t), None, s), [ow], [gl, gr, gp])
            bad += expect(t, ow, Wt("web"))
            t = f"{tag} sm_census_wta_near_right offset {off}"
            owr, obr = out(shp, torch.int32, off, maxp, "web_right"), out(shp, torch.int32, off, maxp, "best_right")
            bad += twice(t, lambda r: lib.sm_census_wta_near_right(plan.h, P(gl.t), P(gr.t), census, pairs, P(gpr.t),
                                                                   radius, P(owr.t), P(obr.t), s), [owr, obr], [gl, gr, gpr])
            bad += expect(t, owr, Wt("web_right")) + expect(t, obr, Wt("best_right"))
            t = f"{tag} sm_census_near_lr offset {off}"
            ow, ob, owr = (out(shp, torch.int32, o, maxp, n) for o, n in ((off, "web"), (4 - off, "best"),
                                                                          (off, "web_right")))
            orj = out((pairs,), torch.int32, off, maxp, "rejected")
            bad += twice(t, lambda r: lib.sm_census_near_lr(plan.h, P(gl.t), P(gr.t), census, pairs, P(gp.t), P(gpr.t),
                                                            radius, 1, P(ow.t), P(ob.t), P(owr.t), P(orj.t), s),
                         [ow, ob, owr, orj], [gl, gr, gp, gpr])
            bad += expect(t, ow, Wt("checked")) + expect(t, ob, Wt("best")) + expect(t, owr, Wt("web_right"))
            bad += expect(t, orj, Wt("rejected"))
            # without the optional maps: the right-reference map goes through the plan's workspace
            t = f"{tag} sm_census_near_lr (web only) offset {off}"
            ow = out(shp, torch.int32, off, maxp, "web")
            bad += twice(t, lambda r: lib.sm_census_near_lr(plan.h, P(gl.t), P(gr.t), census, pairs, P(gp.t), P(gpr.t),
                                                            radius, 1, P(ow.t), None, None, None, s), [ow],
                         [gl, gr, gp, gpr])
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
    m = [torch.zeros((2, h, w), dtype=torch.int32, device="cuda") for _ in range(5)]
    p = [C.c_void_p(t.data_ptr()) for t in m]
    g = torch.zeros((4, h, w), dtype=torch.uint8, device="cuda")
    gp, gq = C.c_void_p(g.data_ptr()), C.c_void_p(g.data_ptr() + 2 * w * h)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    inside = C.c_void_p(m[0].data_ptr() + 4)
    in_image = C.c_void_p(g.data_ptr() + 2 * w * h - 4)      # starts inside the left images, ends inside the right ones
    in_prior = C.c_void_p(m[3].data_ptr() + 2 * w * h * 4 - 4)   # shares the last element of the prior m[3]

    def refused(rc, text):
        assert rc == capi.SM_ERR_ARG and text in lib.sm_last_error(), lib.sm_last_error()
    for f, me in ((lib.sm_census_wta_near, b"sm_census_wta_near"), (lib.sm_census_wta_near_right, b"sm_census_wta_near_right")):
        refused(f(plan._h, gp, gq, 7, 3, p[3], 1, p[0], None, st), me + b": pairs 3 outside 1..2")
        refused(f(plan._h, gp, gq, 7, 0, p[3], 1, p[0], None, st), me + b": pairs 0 outside 1..2")
        refused(f(plan._h, gp, gq, 7, 1, p[3], 0, p[0], None, st), me + b": radius 0 outside 1..4")
        refused(f(plan._h, gp, gq, 7, 1, p[3], 5, p[0], None, st), me + b": radius 5 outside 1..4")
        refused(f(plan._h, gp, gq, 7, 1, p[3], 1, p[0], inside, st), b" overlap")
        refused(f(plan._h, gp, gq, 7, 2, p[3], 1, p[3], None, st), me + b": an output overlaps a prior map")
        refused(f(plan._h, gp, gq, 7, 2, p[3], 1, in_prior, None, st), me + b": an output overlaps a prior map")
        refused(f(plan._h, gp, gq, 7, 2, p[3], 1, p[0], p[3], st), me + b": an output overlaps a prior map")
        refused(f(plan._h, gp, gq, 7, 2, p[3], 1, in_image, None, st), me + b": an output overlaps an input image")
        refused(f(plan._h, gp, gq, 7, 2, p[3], 1, p[0], gq, st), me + b": an output overlaps an input image")
    f, me = lib.sm_census_near_lr, b"sm_census_near_lr"
    refused(f(plan._h, gp, gq, 3, 3, p[3], p[4], 1, 0, p[0], None, None, None, st), me + b": pairs 3 outside")
    refused(f(plan._h, gp, gq, 3, 1, p[3], p[4], 0, 0, p[0], None, None, None, st), me + b": radius 0 outside 1..4")
    refused(f(plan._h, gp, gq, 3, 1, p[3], p[4], 5, 0, p[0], None, None, None, st), me + b": radius 5 outside 1..4")
    refused(f(plan._h, gp, gq, 3, 1, p[3], p[4], 1, 0, p[0], p[0], None, None, st), me + b": result maps overlap")
    refused(f(plan._h, gp, gq, 3, 1, p[3], p[4], 1, 0, p[0], None, inside, None, st), b"result maps overlap")
    refused(f(plan._h, gp, gq, 3, 2, p[3], p[4], 1, 0, p[0], p[1], None, inside, st), b"d_rejected overlaps a map")
    refused(f(plan._h, gp, gq, 3, 2, p[3], p[4], 1, 0, p[3], None, None, None, st), me + b": an output overlaps a prior map")
    refused(f(plan._h, gp, gq, 3, 2, p[3], p[4], 1, 0, p[4], None, None, None, st), me + b": an output overlaps a prior map")
    refused(f(plan._h, gp, gq, 3, 2, p[3], p[4], 1, 0, p[0], None, p[4], None, st), me + b": an output overlaps a prior map")
    refused(f(plan._h, gp, gq, 3, 2, p[3], p[4], 1, 0, p[0], None, None, in_prior, st), me + b": an output overlaps a prior map")
    refused(f(plan._h, gp, gq, 3, 2, p[3], p[4], 1, 0, p[0], gp, None, None, st), me + b": an output overlaps an input image")
    assert plan.workspace_bytes() == base
    plan.close()
    for pw, ph, pd, psw, text in ((64, 32, 16, 27, b"windows up to 25x25"), (64, 32, 513, 5, b"at most 512 shifts")):
        plan = hip.StereoPlan(pw, ph, pd, psw, "toroidal")
        base = plan.workspace_bytes()
        q = [torch.zeros((1, ph, pw), dtype=torch.int32, device="cuda") for _ in range(3)]
        gg = torch.zeros((2, ph, pw), dtype=torch.uint8, device="cuda")
        a, b = C.c_void_p(gg.data_ptr()), C.c_void_p(gg.data_ptr() + pw * ph)
        q0, q1, q2 = (C.c_void_p(t.data_ptr()) for t in q)
        for name, call in ((b"sm_census_wta_near", lambda: lib.sm_census_wta_near(plan._h, a, b, 7, 1, q1, 1, q0, None, st)),
                           (b"sm_census_wta_near_right",
                            lambda: lib.sm_census_wta_near_right(plan._h, a, b, 7, 1, q1, 1, q0, None, st)),
                           (b"sm_census_near_lr", lambda: lib.sm_census_near_lr(plan._h, a, b, 5, 1, q1, q2, 1, 0, q0, None,
                                                                                None, None, st))):
            refused(call(), name + b": built for windows up to 25x25 and at most 512 shifts")
            assert text in lib.sm_last_error()
        assert plan.workspace_bytes() == base
        plan.close()


def test_workspace_contents_and_descriptor_width_do_not_matter(hip):
    """a poisoned workspace changes nothing; census_wta (c = 7), near (c = 5), near (c = 7) on one plan each equal the
    definition (the workspace holds 8-byte, then 4-byte, then 8-byte descriptors); and census_wta's own map as prior
    returns that map and its costs"""
    w, h, d, sw, mode, radius = 130, 35, 40, 5, "ghost", 2
    left, right = make_pair(w, h, d, seed=11)
    rng = np.random.default_rng(4)
    prior = npat.make_prior("surfaces", w, h, d, radius, rng)
    prior_right = npat.make_prior("zeros30", w, h, d, radius, rng)
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        gl, gr, gp, gpr = dev(left), dev(right), dev(prior), dev(prior_right)
        web7, best7 = plan.census_wta(gl, gr, 7)
        want7 = cr.wta(left, right, d, sw, 7, mode)
        assert np.array_equal(host(web7)[0], want7[1]) and np.array_equal(host(best7)[0], want7[0])
        for census in (5, 7):
            e = nr.expected(left, right, prior, prior_right, d, sw, census, radius, mode, 1)
            web, best = plan.census_wta_near(gl, gr, gp, census, radius)
            assert np.array_equal(host(web)[0], e["web"]) and np.array_equal(host(best)[0], e["best"]), census
        for word in (0xFFFFFFFF, 0x00000000, 0xA5A5A5A5):
            plan._poison_workspace(word)
            res = plan.census_near_lr(gl, gr, gp, gpr, 7, radius, max_diff=1, want_right=True, want_best=True)
            assert np.array_equal(host(res.web)[0], e["checked"]), hex(word)
            assert np.array_equal(host(res.web_right)[0], e["web_right"]), hex(word)
            assert np.array_equal(host(res.best)[0], e["best"]) and int(res.rejected[0]) == e["rejected"], hex(word)
            plan._poison_workspace(word)
            res = plan.census_near_lr(gl, gr, gp, gpr, 7, radius, max_diff=1)      # the right map in the workspace
            assert np.array_equal(host(res.web)[0], e["checked"]), hex(word)
        for r in (1, 2, 4):
            web, best = plan.census_wta_near(gl, gr, web7, 7, r)
            assert torch.equal(web, web7) and torch.equal(best, best7), r
    finally:
        plan.close()


@pytest.mark.parametrize("mode,census", [("ghost", 7), ("toroidal", 5)])
def test_near_lr_captured_into_a_graph(hip, mode, census):
    w, h, d, sw, radius = 130, 40, 48, 7, 1
    pairs = [make_pair(w, h, d, seed=90 + i) for i in range(3)]
    rng = np.random.default_rng(9)
    priors = [(npat.make_prior("surfaces", w, h, d, radius, rng), npat.make_prior("zeros30", w, h, d, radius, rng))
              for _ in range(3)]
    left_in = torch.zeros((1, h, w), dtype=torch.uint8, device="cuda")
    right_in = torch.zeros_like(left_in)
    prior_in = torch.zeros((1, h, w), dtype=torch.int32, device="cuda")
    prior_right_in = torch.zeros_like(prior_in)
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        base = plan.workspace_bytes()
        web, right, best = (torch.zeros((1, h, w), dtype=torch.int32, device="cuda") for _ in range(3))
        rej = torch.zeros(1, dtype=torch.int32, device="cuda")
        # refused before reserve_census, and the capture stays valid (it ends cleanly; the pending error is raised)
        for call in (lambda: plan.census_near_lr(left_in, right_in, prior_in, prior_right_in, census, radius, web=web),
                     lambda: plan.census_wta_near(left_in, right_in, prior_in, census, radius, want_best=False, web=web),
                     lambda: plan.census_wta_near_right(left_in, right_in, prior_right_in, census, radius,
                                                        want_best=False, web_right=right)):
            with pytest.raises(capi.StereoHipError, match="sm_plan_reserve_census"):
                with torch.cuda.graph(torch.cuda.CUDAGraph(), capture_error_mode="thread_local"):
                    call()
        assert plan.workspace_bytes() == base
        plan.reserve_census()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        from stereomatching_amd import pipeline
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            pipeline.check(lib.sm_census_near_lr(plan._h, P(left_in), P(right_in), census, 1, P(prior_in), P(prior_right_in),
                                                 radius, 0, P(web), P(best), P(right), P(rej), plan._stream()))
        for rep in (1, 2, 0):
            (l, r), (pl, prr) = pairs[rep], priors[rep]
            left_in.copy_(dev(l))
            right_in.copy_(dev(r))
            prior_in.copy_(dev(pl))
            prior_right_in.copy_(dev(prr))
            for t in (web, right, best):
                t.zero_()
            rej.fill_(12345)
            g.replay()
            torch.cuda.synchronize()
            e = nr.expected(l, r, pl, prr, d, sw, census, radius, mode, 0)
            assert np.array_equal(host(web)[0], e["checked"]), rep
            assert np.array_equal(host(right)[0], e["web_right"]), rep
            assert np.array_equal(host(best)[0], e["best"]), rep
            assert int(rej[0]) == e["rejected"], rep
    finally:
        plan.close()


def test_half_resolution_chain_through_the_binding(hip):
    """reduce_half -> census_lr on a half plan -> upsample_double of both maps (the right one along the right image)
    -> census_near_lr(radius = 1) -> census_refine, every stage against its CPU definition"""
    w, h, d, n, census, mode = 130, 66, 24, 5, 7, "ghost"
    left, right = make_pair(w, h, d, seed=5)
    cw, ch = pr.half_shape(w, h)
    weights = hip.guide_weights(8)
    fine, coarse = hip.StereoPlan(w, h, d, n, mode), hip.StereoPlan(cw, ch, d // 2, n, mode)
    try:
        gl, gr = dev(left[None]), dev(right[None])
        small = fine.reduce_half(dev(np.stack([left, right])))
        want_small = np.stack([pr.reduce_half(left, "binomial"), pr.reduce_half(right, "binomial")])
        assert np.array_equal(host(small), want_small)
        half = coarse.census_lr(small[0:1], small[1:2], census, max_diff=1, want_right=True)
        e_half = cr.expected(want_small[0], want_small[1], d // 2, n, census, mode, 1)
        assert np.array_equal(host(half.web)[0], e_half["checked"])
        assert np.array_equal(host(half.web_right)[0], e_half["web_right"])
        up = fine.upsample_double(half.web, gl, small[0:1], weights, fill=True)
        up_right = fine.upsample_double(half.web_right, gr, small[1:2], weights, fill=True)
        want_up = pr.upsample_double(e_half["checked"], left, want_small[0], weights, True)
        want_up_right = pr.upsample_double(e_half["web_right"], right, want_small[1], weights, True)
        assert np.array_equal(host(up)[0], want_up) and np.array_equal(host(up_right)[0], want_up_right)
        assert (want_up[want_up != 0] % 2 == 1).all()      # every shift the half path reports is even
        res = fine.census_near_lr(gl, gr, up, up_right, census, radius=1, max_diff=1, want_right=True, want_best=True)
        e = nr.expected(left, right, want_up, want_up_right, d, n, census, 1, mode, 1)
        assert np.array_equal(host(res.web)[0], e["checked"])
        assert np.array_equal(host(res.web_right)[0], e["web_right"])
        assert np.array_equal(host(res.best)[0], e["best"]) and int(res.rejected[0]) == e["rejected"]
        assert ((e["checked"] - 1) % 2 == 1).any()          # odd shifts: what the half path alone cannot say
        sub, _ = fine.census_refine(gl, gr, res.web, census)
        assert np.array_equal(host(sub)[0], cr.refine(left, right, e["checked"], d, n, census, mode)[0])
    finally:
        fine.close()
        coarse.close()
