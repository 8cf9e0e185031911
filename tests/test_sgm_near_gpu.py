"""Banded SGM on the GPU: sm_sgm_wta_near, sm_sgm_wta_near_right and sm_sgm_near_lr against the numpy definition
(tests/sgm_near_reference.py), exactly, on the cases of tests/sgm_near_patterns.py (test_sgm_near_cpu.py shows what
they can tell), and against sm_sgm_wta on the same plan where the band holds every shift.  Every expected value comes
from the CPU definitions or from the existing SGM kernels; none from the new path."""
import ctypes as C

import numpy as np
import pytest
import torch

from stereomatching_amd import capi
from stereomatching_amd.capi import lib
from stereomatching_amd.synth import make_pair
from tests import sgm_near_patterns as sp
from tests import sgm_near_reference as sn
from tests.guarded import guarded_input
from tests.test_write_bounds_gpu import P, Plan, expect, out, report, stream, twice

pytestmark = pytest.mark.gpu
MODES = ["toroidal", "ghost"]


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()             # (a copy: the cases' arrays are read-only)


def host(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("name", [c["name"] for c in sp.CASES])
def test_every_map_is_exact(hip, name):
    """web / best / sub of the left pass, web / best of the right pass, and the checked map, the right map, the minima,
    the count and the masked subpixel map of sm_sgm_near_lr, on a full or a partial batch of a plan of three pairs;
    the priors come back as they went in"""
    c = sp.BY_NAME[name]
    left, right, prior, prior_right = sp.inputs(name)
    kw = dict(census=c["census"], p1=c["p1"], p2=c["p2"], paths=c["paths"], radius=c["radius"])
    plan = hip.StereoPlan(c["w"], c["h"], c["d"], c["sw"], c["mode"], max_pairs=sp.MAX_PAIRS)
    try:
        gl, gr, gp, gpr = dev(left), dev(right), dev(prior), dev(prior_right)
        web, best, sub = plan.sgm_wta_near(gl, gr, gp, want_sub=True, **kw)
        web_right, best_right = plan.sgm_wta_near_right(gl, gr, gpr, **kw)
        res = plan.sgm_near_lr(gl, gr, gp, gpr, max_diff=c["max_diff"], want_right=True, want_best=True, want_sub=True,
                               **kw)
        torch.cuda.synchronize()
        assert np.array_equal(host(web), sp.stacked(name, "web"))
        assert np.array_equal(host(best), sp.stacked(name, "best"))
        assert np.array_equal(host(sub), sp.stacked(name, "sub"))
        assert np.array_equal(host(web_right), sp.stacked(name, "web_right"))
        assert np.array_equal(host(best_right), sp.stacked(name, "best_right"))
        assert np.array_equal(host(res.web), sp.stacked(name, "checked"))
        assert np.array_equal(host(res.web_right), sp.stacked(name, "web_right"))
        assert np.array_equal(host(res.best), sp.stacked(name, "best"))
        assert np.array_equal(host(res.sub), sp.stacked(name, "sub_checked"))
        assert host(res.rejected).tolist() == [e["rejected"] for e in sp.expected(name)]
        assert np.array_equal(host(gp), prior) and np.array_equal(host(gpr), prior_right)
    finally:
        plan.close()


@pytest.mark.parametrize("mode", MODES)
def test_a_band_that_holds_every_shift_is_sgm_on_the_device(hip, mode):
    """consequence 1 against the existing kernels: D = 9, r = 4, prior 5 everywhere, and D = 3, r = 2 with noise priors
    in 1 .. 3: web, best and sub equal plan.sgm_wta's on the same plan (8 and 4 paths, two pairs)"""
    w, h = 130, 37
    for d, radius, paths in ((9, 4, 8), (3, 2, 4)):
        rng = np.random.default_rng(d)
        left = rng.integers(0, 256, (2, h, w)).astype(np.uint8)
        right = rng.integers(0, 256, (2, h, w)).astype(np.uint8)
        prior = np.full((2, h, w), 5, np.int32) if d == 9 else rng.integers(1, 4, (2, h, w)).astype(np.int32)
        plan = hip.StereoPlan(w, h, d, 5, mode, max_pairs=2)
        try:
            gl, gr = dev(left), dev(right)
            want = plan.sgm_wta(gl, gr, 7, 30, 250, paths, want_sub=True)
            got = plan.sgm_wta_near(gl, gr, dev(prior), 7, 30, 250, paths, radius, want_sub=True)
            for a, b, what in zip(got, want, ("web", "best", "sub")):
                assert torch.equal(a, b), (d, what)
        finally:
            plan.close()


# ---------------------------------------------------------------------------
# write bounds (tests/guarded.py)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_sgm_near_writes_its_maps_and_nothing_else(mode):
    """every entry, each output at a 16-byte aligned and a 4-byte-but-not-16 offset, partial batches; NULL optional
    maps write nothing"""
    bad = []
    for idx, (w, h, d, sw, census, radius, paths) in enumerate([(33, 17, 45, 3, 7, 1, 8), (64, 16, 130, 5, 3, 2, 4),
                                                                (65, 20, 16, 9, 5, 4, 8), (129, 5, 40, 1, 7, 3, 4)]):
        pairs, maxp = (2, 3) if idx % 2 == 0 else (1, 2)
        plan = Plan(w, h, d, sw, mode, maxp)
        tag = f"{mode} c={census} r={radius} paths={paths} W={w} H={h} D={d} S={sw} pairs={pairs}/{maxp}"
        rng = np.random.default_rng(idx + 80)
        left = rng.integers(0, 256, (pairs, h, w)).astype(np.uint8)
        right = rng.integers(0, 256, (pairs, h, w)).astype(np.uint8)
        prior = np.stack([sp.make_prior(("zeros30", "noise")[idx % 2], w, h, d, radius, rng) for _ in range(pairs)])
        prior_right = np.stack([sp.make_prior("extremes", w, h, d, radius, rng) for _ in range(pairs)])
        p1, p2 = 12, 150
        want = [sn.expected(left[q], right[q], prior[q], prior_right[q], d, sw, census, p1, p2, paths, radius, mode, 1)
                for q in range(pairs)]
        Wt = lambda k: np.stack([x[k] for x in want])     # noqa: E731
        shp, s = (pairs, h, w), stream()
        gl, gr = guarded_input(left, "cuda", idx % 2, "left"), guarded_input(right, "cuda", 0, "right")
        gp, gpr = guarded_input(prior, "cuda", 4, "prior"), guarded_input(prior_right, "cuda", 0, "prior_right")
        head = lambda: (plan.h, P(gl.t), P(gr.t), census, p1, p2, paths, pairs)     # noqa: E731
        for off in (0, 4):
            t = f"{tag} sm_sgm_wta_near offset {off}"
            ow, ob = out(shp, torch.int32, off, maxp, "web"), out(shp, torch.int32, 4 - off, maxp, "best")
            os_ = out(shp, torch.int16, off, maxp, "sub")
            bad += twice(t, lambda r: lib.sm_sgm_wta_near(*head(), P(gp.t), radius, P(ow.t), P(ob.t), P(os_.t), s),
                         [ow, ob, os_], [gl, gr, gp])
            bad += expect(t, ow, Wt("web")) + expect(t, ob, Wt("best")) + expect(t, os_, Wt("sub"))
            t = f"{tag} sm_sgm_wta_near (web only) offset {off}"
            ow = out(shp, torch.int32, off, maxp, "web")
            bad += twice(t, lambda r: lib.sm_sgm_wta_near(*head(), P(gp.t), radius, P(ow.t), None, None, s), [ow],
                         [gl, gr, gp])
            bad += expect(t, ow, Wt("web"))
            t = f"{tag} sm_sgm_wta_near_right offset {off}"
            owr, obr = out(shp, torch.int32, off, maxp, "web_right"), out(shp, torch.int32, off, maxp, "best_right")
            bad += twice(t, lambda r: lib.sm_sgm_wta_near_right(*head(), P(gpr.t), radius, P(owr.t), P(obr.t), s),
                         [owr, obr], [gl, gr, gpr])
            bad += expect(t, owr, Wt("web_right")) + expect(t, obr, Wt("best_right"))
            t = f"{tag} sm_sgm_near_lr offset {off}"
            ow, ob, owr = (out(shp, torch.int32, o, maxp, n) for o, n in ((off, "web"), (4 - off, "best"),
                                                                          (off, "web_right")))
            orj = out((pairs,), torch.int32, off, maxp, "rejected")
            os_ = out(shp, torch.int16, 4 - off, maxp, "sub")
            bad += twice(t, lambda r: lib.sm_sgm_near_lr(*head(), P(gp.t), P(gpr.t), radius, 1, P(ow.t), P(ob.t),
                                                         P(owr.t), P(orj.t), P(os_.t), s),
                         [ow, ob, owr, orj, os_], [gl, gr, gp, gpr])
            bad += expect(t, ow, Wt("checked")) + expect(t, ob, Wt("best")) + expect(t, owr, Wt("web_right"))
            bad += expect(t, orj, Wt("rejected")) + expect(t, os_, Wt("sub_checked"))
            # without the optional maps: the right-reference map goes through the plan's workspace
            t = f"{tag} sm_sgm_near_lr (web only) offset {off}"
            ow = out(shp, torch.int32, off, maxp, "web")
            bad += twice(t, lambda r: lib.sm_sgm_near_lr(*head(), P(gp.t), P(gpr.t), radius, 1, P(ow.t), None, None,
                                                         None, None, s), [ow], [gl, gr, gp, gpr])
            bad += expect(t, ow, Wt("checked"))
        plan.close()
    report(bad)


# ---------------------------------------------------------------------------
# arguments, workspace, capture
# ---------------------------------------------------------------------------

def test_argument_checks_on_a_plan(hip):
    """refusals that read the plan, every overlap among them, before any device call: the workspace stays as it was"""
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
    sub_in_web = C.c_void_p(m[0].data_ptr() + 2)

    def refused(rc, text):
        assert rc == capi.SM_ERR_ARG and text in lib.sm_last_error(), lib.sm_last_error()
    for name in ("sm_sgm_wta_near", "sm_sgm_wta_near_right"):
        fn, me = getattr(lib, name), name.encode()
        tail = (st,) if name.endswith("right") else (None, st)

        def f(pairs, prior, radius, web, best, fn=fn, tail=tail):
            return fn(plan._h, gp, gq, 7, 10, 120, 8, pairs, prior, radius, web, best, *tail)
        refused(f(3, p[3], 1, p[0], None), me + b": pairs 3 outside 1..2")
        refused(f(0, p[3], 1, p[0], None), me + b": pairs 0 outside 1..2")
        refused(f(1, p[3], 0, p[0], None), me + b": radius 0 outside 1..4")
        refused(f(1, p[3], 5, p[0], None), me + b": radius 5 outside 1..4")
        refused(f(1, p[3], 1, p[0], inside), b" overlap")
        refused(f(2, p[3], 1, p[3], None), me + b": an output overlaps a prior map")
        refused(f(2, p[3], 1, in_prior, None), me + b": an output overlaps a prior map")
        refused(f(2, p[3], 1, p[0], p[3]), me + b": an output overlaps a prior map")
        refused(f(2, p[3], 1, in_image, None), me + b": an output overlaps an input image")
        refused(f(2, p[3], 1, p[0], gq), me + b": an output overlaps an input image")
    refused(lib.sm_sgm_wta_near(plan._h, gp, gq, 7, 10, 120, 8, 1, p[3], 1, p[0], None, sub_in_web, st), b" overlap")
    refused(lib.sm_sgm_wta_near(plan._h, gp, gq, 7, 10, 120, 8, 1, p[3], 1, p[0], p[1], p[1], st), b" overlap")
    # the int16 subpixel map is an output like the others: apart from the prior and from both images
    sub_in_prior = C.c_void_p(m[3].data_ptr() + 2 * w * h * 4 - 2)   # shares the last two bytes of the prior m[3]
    sub_in_image = C.c_void_p(g.data_ptr() + 2 * w * h - 2)          # ends inside the right images
    me = b"sm_sgm_wta_near"

    def fs(pairs, sub, best=None):
        return lib.sm_sgm_wta_near(plan._h, gp, gq, 7, 10, 120, 8, pairs, p[3], 1, p[0], best, sub, st)
    refused(fs(2, p[3]), me + b": an output overlaps a prior map")
    refused(fs(2, sub_in_prior, p[1]), me + b": an output overlaps a prior map")
    refused(fs(2, gp), me + b": an output overlaps an input image")
    refused(fs(2, gq, p[1]), me + b": an output overlaps an input image")
    refused(fs(2, sub_in_image), me + b": an output overlaps an input image")
    me = b"sm_sgm_near_lr"

    def f(cw, pairs, radius, web, best, right, rejected, sub=None):
        return lib.sm_sgm_near_lr(plan._h, gp, gq, cw, 10, 120, 4, pairs, p[3], p[4], radius, 0, web, best, right,
                                  rejected, sub, st)
    refused(f(3, 3, 1, p[0], None, None, None), me + b": pairs 3 outside")
    refused(f(3, 1, 0, p[0], None, None, None), me + b": radius 0 outside 1..4")
    refused(f(3, 1, 5, p[0], None, None, None), me + b": radius 5 outside 1..4")
    refused(f(3, 1, 1, p[0], p[0], None, None), me + b": result maps overlap")
    refused(f(3, 1, 1, p[0], None, inside, None), b"result maps overlap")
    refused(f(3, 1, 1, p[0], None, None, None, sub_in_web), b"result maps overlap")
    refused(f(3, 2, 1, p[0], p[1], None, inside), b"d_rejected overlaps a map")
    refused(f(3, 2, 1, p[3], None, None, None), me + b": an output overlaps a prior map")
    refused(f(3, 2, 1, p[4], None, None, None), me + b": an output overlaps a prior map")
    refused(f(3, 2, 1, p[0], None, p[4], None), me + b": an output overlaps a prior map")
    refused(f(3, 2, 1, p[0], None, None, in_prior), me + b": an output overlaps a prior map")
    refused(f(3, 2, 1, p[0], gp, None, None), me + b": an output overlaps an input image")
    refused(f(3, 2, 1, p[0], None, None, None, p[3]), me + b": an output overlaps a prior map")
    refused(f(3, 2, 1, p[0], p[1], p[2], None, p[4]), me + b": an output overlaps a prior map")
    refused(f(3, 2, 1, p[0], None, None, None, sub_in_prior), me + b": an output overlaps a prior map")
    refused(f(3, 2, 1, p[0], None, None, None, gp), me + b": an output overlaps an input image")
    refused(f(3, 2, 1, p[0], None, None, None, gq), me + b": an output overlaps an input image")
    refused(f(3, 2, 1, p[0], None, None, None, sub_in_image), me + b": an output overlaps an input image")
    assert plan.workspace_bytes() == base
    plan.close()
    # the census reach, not SGM's 256 shifts: 512 shifts are taken (the next test runs them), 513 and a 27 x 27 window are not
    for pw, ph, pd, psw, text in ((64, 32, 16, 27, b"windows up to 25x25"), (64, 32, 513, 5, b"at most 512 shifts")):
        plan = hip.StereoPlan(pw, ph, pd, psw, "toroidal")
        base = plan.workspace_bytes()
        q = [torch.zeros((1, ph, pw), dtype=torch.int32, device="cuda") for _ in range(3)]
        gg = torch.zeros((2, ph, pw), dtype=torch.uint8, device="cuda")
        a, b = C.c_void_p(gg.data_ptr()), C.c_void_p(gg.data_ptr() + pw * ph)
        q0, q1, q2 = (C.c_void_p(t.data_ptr()) for t in q)
        for name, call in ((b"sm_sgm_wta_near", lambda: lib.sm_sgm_wta_near(plan._h, a, b, 7, 1, 2, 8, 1, q1, 1, q0, None,
                                                                            None, st)),
                           (b"sm_sgm_wta_near_right",
                            lambda: lib.sm_sgm_wta_near_right(plan._h, a, b, 7, 1, 2, 8, 1, q1, 1, q0, None, st)),
                           (b"sm_sgm_near_lr", lambda: lib.sm_sgm_near_lr(plan._h, a, b, 5, 1, 2, 8, 1, q1, q2, 1, 0, q0,
                                                                          None, None, None, None, st))):
            refused(call(), name + b": built for windows up to 25x25 and at most 512 shifts")
            assert text in lib.sm_last_error()
        assert plan.workspace_bytes() == base
        plan.close()


def test_workspace_bytes_poison_and_no_full_volumes(hip):
    """the calls allocate the census workspace and 96 W H bytes of banded volumes, not SGM's volumes (at D = 300 a
    plan that sm_sgm_wta refuses); reserve_sgm_near is the same allocation; a poisoned workspace changes nothing"""
    w, h, d, sw, mode, radius = 130, 35, 300, 5, "ghost", 2
    left, right = make_pair(w, h, 40, seed=11)
    rng = np.random.default_rng(4)
    prior = sp.make_prior("jumps", w, h, d, radius, rng)
    prior_right = sp.make_prior("zeros30", w, h, d, radius, rng)
    e = sn.expected(left, right, prior, prior_right, d, sw, 7, 25, 300, 8, radius, mode, 1)
    for reserve in (False, True):
        plan = hip.StereoPlan(w, h, d, sw, mode, max_pairs=2)
        try:
            base = plan.workspace_bytes()
            gl, gr, gp, gpr = dev(left[None]), dev(right[None]), dev(prior[None]), dev(prior_right[None])
            if reserve:
                plan.reserve_sgm_near()
                plan.reserve_sgm_near()
            else:
                plan.sgm_wta_near(gl, gr, gp, 7, 25, 300, 8, radius)
            census = 16 * 2 * w * h + 4 * 2 * w * h         # descriptors of max_pairs pairs and the mirrored-order map
            assert plan.workspace_bytes() == base + census + 96 * w * h
            with pytest.raises(capi.StereoHipError, match="at most 256 shifts"):
                plan.sgm_wta(gl, gr, 7, 25, 300, 8)
            for word in (0xFFFFFFFF, 0x00000000):
                plan._poison_workspace(word)
                res = plan.sgm_near_lr(gl, gr, gp, gpr, 7, 25, 300, 8, radius, max_diff=1, want_right=True,
                                       want_best=True, want_sub=True)
                assert np.array_equal(host(res.web)[0], e["checked"]), hex(word)
                assert np.array_equal(host(res.web_right)[0], e["web_right"]), hex(word)
                assert np.array_equal(host(res.best)[0], e["best"]) and int(res.rejected[0]) == e["rejected"], hex(word)
                assert np.array_equal(host(res.sub)[0], e["sub_checked"]), hex(word)
                plan._poison_workspace(word)
                web, best, sub = plan.sgm_wta_near(gl, gr, gp, 7, 25, 300, 8, radius, want_sub=True)
                assert np.array_equal(host(web)[0], e["web"]) and np.array_equal(host(sub)[0], e["sub"]), hex(word)
            assert plan.workspace_bytes() == base + census + 96 * w * h
        finally:
            plan.close()


@pytest.mark.parametrize("mode,census", [("ghost", 7), ("toroidal", 5)])
def test_sgm_near_lr_captured_into_a_graph(hip, mode, census):
    w, h, d, sw, radius = 130, 40, 48, 7, 1
    pairs = [make_pair(w, h, d, seed=90 + i) for i in range(3)]
    rng = np.random.default_rng(9)
    priors = [(sp.make_prior("jumps", w, h, d, radius, rng), sp.make_prior("zeros30", w, h, d, radius, rng))
              for _ in range(3)]
    left_in = torch.zeros((1, h, w), dtype=torch.uint8, device="cuda")
    right_in = torch.zeros_like(left_in)
    prior_in = torch.zeros((1, h, w), dtype=torch.int32, device="cuda")
    prior_right_in = torch.zeros_like(prior_in)
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        base = plan.workspace_bytes()
        web, right, best = (torch.zeros((1, h, w), dtype=torch.int32, device="cuda") for _ in range(3))
        sub = torch.zeros((1, h, w), dtype=torch.int16, device="cuda")
        rej = torch.zeros(1, dtype=torch.int32, device="cuda")
        # refused before reserve_sgm_near, and the capture stays valid (it ends cleanly; the pending error is raised)
        for call in (lambda: plan.sgm_near_lr(left_in, right_in, prior_in, prior_right_in, census, radius=radius, web=web),
                     lambda: plan.sgm_wta_near(left_in, right_in, prior_in, census, radius=radius, want_best=False,
                                               web=web),
                     lambda: plan.sgm_wta_near_right(left_in, right_in, prior_right_in, census, radius=radius,
                                                     want_best=False, web_right=right)):
            with pytest.raises(capi.StereoHipError, match="sm_plan_reserve_sgm_near"):
                with torch.cuda.graph(torch.cuda.CUDAGraph(), capture_error_mode="thread_local"):
                    call()
        assert plan.workspace_bytes() == base
        plan.reserve_sgm_near()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        from stereomatching_amd import pipeline
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            pipeline.check(lib.sm_sgm_near_lr(plan._h, P(left_in), P(right_in), census, 20, 180, 8, 1, P(prior_in),
                                              P(prior_right_in), radius, 0, P(web), P(best), P(right), P(rej), P(sub),
                                              plan._stream()))
        for rep in (1, 2, 0):
            (l, r), (pl, prr) = pairs[rep], priors[rep]
            left_in.copy_(dev(l))
            right_in.copy_(dev(r))
            prior_in.copy_(dev(pl))
            prior_right_in.copy_(dev(prr))
            for t in (web, right, best, sub):
                t.zero_()
            rej.fill_(12345)
            g.replay()
            torch.cuda.synchronize()
            eager = plan.sgm_near_lr(left_in, right_in, prior_in, prior_right_in, census, 20, 180, 8, radius, max_diff=0,
                                     want_right=True, want_best=True, want_sub=True)
            e = sn.expected(l, r, pl, prr, d, sw, census, 20, 180, 8, radius, mode, 0)
            assert np.array_equal(host(web)[0], e["checked"]), rep
            assert np.array_equal(host(right)[0], e["web_right"]), rep
            assert np.array_equal(host(best)[0], e["best"]), rep
            assert np.array_equal(host(sub)[0], e["sub_checked"]), rep
            assert int(rej[0]) == e["rejected"], rep
            assert torch.equal(eager.web, web) and torch.equal(eager.web_right, right) and torch.equal(eager.best, best)
            assert torch.equal(eager.sub, sub) and torch.equal(eager.rejected, rej)
    finally:
        plan.close()


def test_the_sgm_map_as_prior_and_the_half_resolution_chain(hip):
    """consequence 3 and the path the feature completes: plan.sgm_wta's own map as prior gives a shift of its band at
    every pixel, at every radius; half-size sgm_lr -> upsample_double -> sgm_near_lr (r = 1) equals the definition on
    the upsampled maps"""
    from tests import pyramid_reference as pr
    w, h, d, n, census, mode = 130, 66, 24, 5, 7, "ghost"
    left, right = make_pair(w, h, d, seed=5)
    cw, ch = pr.half_shape(w, h)
    weights = hip.guide_weights(8)
    fine, coarse = hip.StereoPlan(w, h, d, n, mode), hip.StereoPlan(cw, ch, d // 2, n, mode)
    try:
        gl, gr = dev(left[None]), dev(right[None])
        full, _, _ = fine.sgm_wta(gl, gr, census, 100, 1200, 8)
        for radius in (1, 2, 4):
            web, best, sub = fine.sgm_wta_near(gl, gr, full, census, 100, 1200, 8, radius, want_sub=True)
            assert bool(((web - full).abs() <= radius).all()) and bool((web >= 1).all()) and bool((web <= d).all())
            e = sn.sgm_near(left, right, host(full)[0], d, n, census, 100, 1200, 8, radius, mode)
            assert np.array_equal(host(web)[0], e[1]) and np.array_equal(host(best)[0], e[0])
            assert np.array_equal(host(sub)[0], e[2])
        small = fine.reduce_half(dev(np.stack([left, right])))
        half = coarse.sgm_lr(small[0:1], small[1:2], census, 100, 1200, 8, max_diff=1, want_right=True)
        up = fine.upsample_double(half.web, gl, small[0:1], weights, fill=True)
        up_right = fine.upsample_double(half.web_right, gr, small[1:2], weights, fill=True)
        res = fine.sgm_near_lr(gl, gr, up, up_right, census, 100, 1200, 8, 1, max_diff=1, want_right=True, want_best=True,
                               want_sub=True)
        e = sn.expected(left, right, host(up)[0], host(up_right)[0], d, n, census, 100, 1200, 8, 1, mode, 1)
        assert np.array_equal(host(res.web)[0], e["checked"]) and np.array_equal(host(res.web_right)[0], e["web_right"])
        assert np.array_equal(host(res.best)[0], e["best"]) and int(res.rejected[0]) == e["rejected"]
        assert np.array_equal(host(res.sub)[0], e["sub_checked"])
        assert ((e["checked"] - 1) % 2 == 1).any()          # odd shifts: what the half path alone cannot say
    finally:
        fine.close()
        coarse.close()
