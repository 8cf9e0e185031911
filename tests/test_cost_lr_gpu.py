"""Left-right consistency check of the SAD / SSD cost mode on the GPU: sm_cost_wta_right and sm_cost_lr against the
oracle's cost mode on mirrored images and the numpy definition of the check (tests/cost_lr_reference.py).  Every
expected value comes from the CPU definitions; none from the HIP path."""
import ctypes as C

import numpy as np
import pytest
import torch

from stereomatching_amd.synth import CONFIGS, make_pair
from tests import cost_lr_reference as clr
from tests import extreme_patterns as xp
from tests import lr_reference as lr
from tests import oracle
from tests import subpix_reference as sr

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def gray_batch_bytes(w, h, max_pairs):
    """one batch of the mirrored gray images: max_pairs * W * H rounded up to 256 bytes"""
    return (max_pairs * w * h + 255) // 256 * 256


# ---------------------------------------------------------------------------
# every cost path, both directions
# ---------------------------------------------------------------------------

COST_CHOICES = [None, dict(cost_kernel=1), dict(cost_workgroup_waves=1), dict(cost_workgroup_waves=2),
                dict(cost_workgroup_waves=4)]

# k_sad_pc: windows 3 .. 15; k_sad_qs: 17 .. 21 with D <= 240; k_ssd_mfma: 3 .. 11 with D <= 256; the general kernel:
# SSD windows over 11, and 23 / 25 with D > 256; W % 4 != 0 takes the mirror kernel's byte path (and the cost kernels'
# slow staging); ghost windows of half > 0 take the strip kernel behind a fast one
COST_SHAPES = [(96, 40, 30, 3), (130, 37, 64, 9), (97, 23, 40, 15), (100, 30, 48, 19), (64, 24, 240, 21),
               (120, 20, 256, 11), (70, 26, 300, 23), (52, 30, 260, 25)]


@pytest.mark.parametrize("cost", ["sad", "ssd"])
@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
@pytest.mark.parametrize("w,h,d,sw", COST_SHAPES)
@pytest.mark.parametrize("opts", COST_CHOICES, ids=lambda o: "default" if o is None else
                         "-".join(f"{k}{v}" for k, v in o.items()))
def test_every_cost_path_has_a_right_reference_mode(hip, opts, w, h, d, sw, mode, cost):
    left, right = make_pair(w, h, d, seed=w + d)
    want = clr.expected(left, right, d, sw, mode, cost, max_diff=1)
    plan = hip.StereoPlan(w, h, d, sw, mode, options=opts)
    try:
        gl, gr = dev(left), dev(right)
        web, best = plan.cost_wta(gl, gr, cost)
        web_right, best_right = plan.cost_wta_right(gl, gr, cost)
        assert np.array_equal(host(web)[0], want["web"]), plan.describe()
        assert np.array_equal(host(best)[0], want["best"])
        assert np.array_equal(host(web_right)[0], want["web_right"]), (opts, w, h, d, sw, mode, cost)
        assert np.array_equal(host(best_right)[0], want["best_right"]), (opts, w, h, d, sw, mode, cost)
        res = plan.cost_lr(gl, gr, cost, max_diff=1, want_right=True, want_best=True)
        assert np.array_equal(host(res.web)[0], want["checked"])
        assert np.array_equal(host(res.web_right)[0], want["web_right"])
        assert np.array_equal(host(res.best)[0], want["best"])
        assert int(res.rejected[0]) == want["rejected"]
    finally:
        plan.close()


# ---------------------------------------------------------------------------
# sm_cost_lr on the extreme gray patterns, small and odd widths, batches short of max_pairs
# ---------------------------------------------------------------------------

SMALL_SHAPES = [(1, 6, 3, 1), (2, 5, 6, 1), (3, 7, 9, 3), (4, 5, 12, 3), (5, 9, 15, 5), (6, 8, 19, 6), (7, 7, 21, 7),
                (8, 11, 24, 7), (9, 9, 27, 9), (13, 10, 20, 5), (67, 13, 40, 7)]


@pytest.mark.parametrize("cost", ["sad", "ssd"])
@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
@pytest.mark.parametrize("w,h,d,sw", SMALL_SHAPES)
def test_cost_lr_on_extreme_patterns_and_small_widths(hip, w, h, d, sw, mode, cost):
    names, lefts, rights = xp.gray_batch(w, h)
    rng = np.random.default_rng(w * 31 + h)
    # and two textured pairs (one of three grey levels: ties everywhere)
    lefts = np.concatenate([lefts, rng.integers(0, 256, (1, h, w)), rng.integers(0, 3, (1, h, w))]).astype(np.uint8)
    rights = np.concatenate([rights, rng.integers(0, 256, (1, h, w)), rng.integers(0, 3, (1, h, w))]).astype(np.uint8)
    pairs = lefts.shape[0]
    plan = hip.StereoPlan(w, h, d, sw, mode, max_pairs=pairs + 2)
    try:
        gl, gr = dev(lefts), dev(rights)
        web0, best0 = plan.cost_wta(gl, gr, cost)
        for max_diff in (0, 1, 2, 10**6):
            res = plan.cost_lr(gl, gr, cost, max_diff=max_diff, want_right=True, want_best=True)
            torch.cuda.synchronize()
            assert torch.equal(res.best, best0)                         # exactly sm_cost_wta's costs
            for q in range(pairs):
                want = clr.expected(lefts[q], rights[q], d, sw, mode, cost, max_diff)
                tag = (q if q >= len(names) else names[q], max_diff)
                assert np.array_equal(host(web0)[q], want["web"]), tag
                assert np.array_equal(host(res.best)[q], want["best"]), tag
                assert np.array_equal(host(res.web_right)[q], want["web_right"]), tag
                assert np.array_equal(host(res.web)[q], want["checked"]), tag
                assert int(res.rejected[q]) == want["rejected"], tag
        # the right-reference entry alone, without costs
        web_right, best_right = plan.cost_wta_right(gl, gr, cost, want_best=False)
        assert best_right is None
        for q in range(pairs):
            assert np.array_equal(host(web_right)[q], clr.right_reference(lefts[q], rights[q], d, sw, mode, cost)[1])
    finally:
        plan.close()


def test_unaligned_images_and_maps(hip):
    """images that start off a 16- or 4-byte boundary take the mirror kernel's narrower paths (and the quad-SAD
    kernel its byte staging), a right-reference map off a 16-byte boundary the check's scalar path: the same
    results"""
    w, h, d, sw = 64, 20, 30, 5
    left, right = make_pair(w, h, d, seed=5)
    want = clr.expected(left, right, d, sw, "toroidal", "sad", 0)
    plan = hip.StereoPlan(w, h, d, sw)
    try:
        for off in (4, 1):
            buf = torch.zeros(2 * w * h + off, dtype=torch.uint8, device="cuda")
            gl = buf[off:off + w * h].view(1, h, w)
            gr = buf[off + w * h:off + 2 * w * h].view(1, h, w)
            gl.copy_(dev(left)[None])
            gr.copy_(dev(right)[None])
            mbuf = torch.zeros(w * h + 1, dtype=torch.int32, device="cuda")
            web_right = mbuf[1:].view(1, h, w)
            res = plan.cost_lr(gl, gr, "sad", max_diff=0, want_right=True, web_right=web_right)
            torch.cuda.synchronize()
            assert np.array_equal(host(res.web)[0], want["checked"]), off
            assert np.array_equal(host(res.web_right)[0], want["web_right"]), off
            assert int(res.rejected[0]) == want["rejected"], off
    finally:
        plan.close()


# ---------------------------------------------------------------------------
# full size, on bands of rows
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("cfg,cost", [("C3", "sad"), ("C3", "ssd"), ("C5", "ssd")])
def test_full_size_on_bands_of_rows(hip, cfg, cost):
    """the check reads only its own row, so bands of rows (with their window halo for the two cost maps) can be
    checked alone"""
    w, h, d, sw, mode = CONFIGS[cfg]
    left, right = make_pair(w, h, d, seed=3)
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        res = plan.cost_lr(dev(left), dev(right), cost, max_diff=0, want_right=True, want_best=True)
        torch.cuda.synchronize()
        web, best, web_right = host(res.web)[0], host(res.best)[0], host(res.web_right)[0]
        assert int(res.rejected[0]) == int((web == 0).sum()) > 0, plan.describe()
        half = sw // 2
        for y0, y1 in ((0, 20), (h // 2 - 7, h // 2 + 9), (h - 20, h)):
            if mode == "toroidal":
                rows, lo = np.arange(y0 - half, y1 + half) % h, half
            else:
                a, b = max(0, y0 - half), min(h, y1 + half)
                rows, lo = np.arange(a, b), y0 - a
            want = clr.expected(left[rows], right[rows], d, sw, mode, cost, 0)
            band = slice(lo, lo + y1 - y0)
            assert np.array_equal(want["best"][band], best[y0:y1]), (cfg, cost, y0)
            assert np.array_equal(want["web_right"][band], web_right[y0:y1]), (cfg, cost, y0)
            checked, _ = clr.lr_check(want["web"][band], want["web_right"][band], 0, mode)
            assert np.array_equal(checked, web[y0:y1]), (cfg, cost, y0)
    finally:
        plan.close()


# ---------------------------------------------------------------------------
# the whole chain: cost -> check -> hole filling -> subpixel
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode,w,h,d,sw,cost,times,lines", [("toroidal", 320, 96, 128, 5, "sad", 4, 5),
                                                            ("ghost", 200, 70, 30, 9, "sad", 32, 10),
                                                            ("toroidal", 257, 61, 64, 7, "ssd", 2, 7),
                                                            ("ghost", 160, 48, 64, 11, "ssd", 1, 6)])
@pytest.mark.parametrize("max_diff", [0, 1])
def test_cost_lr_through_step3_and_refine(hip, mode, w, h, d, sw, cost, times, lines, max_diff):
    left, right = make_pair(w, h, d, seed=7)
    want = clr.expected(left, right, d, sw, mode, cost, max_diff)
    assert (want["checked"] == 0).any()                 # holes, so that hole filling does work
    filled = oracle.fill_web_holes(want["checked"], times)
    contour = oracle.draw_contour_map(filled, lines)
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        gl, gr = dev(left), dev(right)
        res = plan.cost_lr(gl, gr, cost, max_diff=max_diff)
        assert np.array_equal(host(res.web)[0], want["checked"])
        # the rejected pixels refine to 0 before filling; the others as the definition says
        sub0, _ = plan.cost_refine(gl, gr, res.web, cost)
        want_sub0, _ = sr.refine(left, right, want["checked"], d, sw, mode, cost)
        assert np.array_equal(host(sub0)[0], want_sub0)
        assert (host(sub0)[0][want["checked"] == 0] == 0).all()
        # hole filling, on its own and as the one-synchronisation step 3 (its staged route on a map with holes)
        f1 = plan.fill_web_holes(res.web, times)
        assert np.array_equal(host(f1)[0], filled)
        f2, c2, mm = plan.step3(res.web, times, lines)
        assert np.array_equal(host(f2)[0], filled) and np.array_equal(host(c2)[0], contour)
        assert host(mm)[0].tolist() == [int(filled.min()), int(filled.max())]
        # subpixel on the filled map
        sub, _ = plan.cost_refine(gl, gr, f2, cost)
        want_sub, _ = sr.refine(left, right, filled, d, sw, mode, cost)
        assert np.array_equal(host(sub)[0], want_sub)
    finally:
        plan.close()


# ---------------------------------------------------------------------------
# arguments, workspace, isolation, ordering, capture
# ---------------------------------------------------------------------------

def test_argument_checks_on_a_plan(hip):
    from stereomatching_amd import capi
    lib = capi.lib
    w, h, d = 64, 32, 16
    plan = hip.StereoPlan(w, h, d, 5, "toroidal", max_pairs=2)
    base = plan.workspace_bytes()
    m = [torch.zeros((2, h, w), dtype=torch.int32, device="cuda") for _ in range(3)]
    p = [C.c_void_p(t.data_ptr()) for t in m]
    g = torch.zeros((2, h, w), dtype=torch.uint8, device="cuda")
    gp = C.c_void_p(g.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    inside = C.c_void_p(m[0].data_ptr() + 4)                            # a map that starts inside m[0]

    def refused(rc, text):
        assert rc == capi.SM_ERR_ARG and text in lib.sm_last_error(), lib.sm_last_error()
    refused(lib.sm_cost_wta_right(plan._h, gp, gp, 1, 0, p[0], None, st), b"outside 1..2")
    refused(lib.sm_cost_wta_right(plan._h, gp, gp, 1, 3, p[0], None, st), b"outside 1..2")
    refused(lib.sm_cost_wta_right(plan._h, gp, gp, 2, 1, p[0], inside, st), b"d_web_right and d_best_right overlap")
    refused(lib.sm_cost_wta_right(plan._h, gp, gp, 4, 1, p[0], None, st), b"cost 4 is neither")
    refused(lib.sm_cost_lr(plan._h, gp, gp, 1, 3, 0, p[0], None, None, None, st), b"outside 1..2")
    refused(lib.sm_cost_lr(plan._h, gp, gp, 1, 1, -3, p[0], None, None, None, st), b"max_diff -3 is negative")
    refused(lib.sm_cost_lr(plan._h, gp, gp, 1, 1, 0, p[0], p[0], None, None, st), b"result maps overlap")
    refused(lib.sm_cost_lr(plan._h, gp, gp, 1, 1, 0, p[0], None, inside, None, st), b"result maps overlap")
    refused(lib.sm_cost_lr(plan._h, gp, gp, 1, 1, 0, p[0], p[1], p[1], None, st), b"result maps overlap")
    refused(lib.sm_cost_lr(plan._h, gp, gp, 1, 2, 0, p[0], p[1], None, inside, st), b"d_rejected overlaps a map")
    refused(lib.sm_cost_lr(plan._h, gp, gp, 1, 1, 0, p[0], None, p[1], p[1], st), b"d_rejected overlaps a map")
    assert plan.workspace_bytes() == base
    plan.close()
    # windows over 25 x 25 and more than 512 shifts (plans of the edge matcher take them)
    for pw, ph, pd, psw, text in ((64, 32, 16, 27, b"windows up to 25x25"), (64, 32, 513, 5, b"at most 512 shifts")):
        plan = hip.StereoPlan(pw, ph, pd, psw, "toroidal")
        base = plan.workspace_bytes()
        q = torch.zeros((1, ph, pw), dtype=torch.int32, device="cuda")
        gq = torch.zeros((1, ph, pw), dtype=torch.uint8, device="cuda")
        refused(lib.sm_cost_wta_right(plan._h, C.c_void_p(gq.data_ptr()), C.c_void_p(gq.data_ptr()), 1, 1,
                                      C.c_void_p(q.data_ptr()), None, st), text)
        refused(lib.sm_cost_lr(plan._h, C.c_void_p(gq.data_ptr()), C.c_void_p(gq.data_ptr()), 2, 1, 0,
                               C.c_void_p(q.data_ptr()), None, None, None, st), text)
        assert plan.workspace_bytes() == base
        plan.close()


def test_workspace_is_allocated_only_for_the_check(hip):
    w, h, d, sw, mp = 300, 150, 128, 9, 2
    left, right = make_pair(w, h, d, seed=3)
    gl, gr = dev(left), dev(right)
    gray = 2 * gray_batch_bytes(w, h, mp)
    mapb = mp * w * h * 4
    # reserve_cost_lr: the mirrored gray images and the map
    plan = hip.StereoPlan(w, h, d, sw, "toroidal", max_pairs=mp)
    base, desc, geom = plan.workspace_bytes(), plan.describe(), plan.geometry()
    web, _ = plan.cost_wta(gl, gr, "sad")
    plan.cost_refine(gl, gr, web, "sad")
    plan.lr_check(web, web, 0)                                           # no workspace needed
    torch.cuda.synchronize()
    assert plan.workspace_bytes() == base and plan.describe() == desc and plan.geometry() == geom
    plan.reserve_cost_lr()
    plan.reserve_cost_lr()                                               # idempotent
    assert plan.workspace_bytes() == base + gray + mapb
    assert plan.describe() == desc and plan.geometry() == geom
    # ... then reserve_lr adds only the mirrored packed images: the map is shared
    ext = mp * 2 * geom["ext_words"] * geom["ext_rows"] * 4
    plan.reserve_lr()
    assert plan.workspace_bytes() == base + gray + mapb + ext
    # both checks on the one plan, in either order
    want = clr.expected(left, right, d, sw, "toroidal", "sad", 0)
    r1 = plan.cost_lr(gl, gr, "sad")
    r2 = plan.run_lr(gl, gr, 0.15)
    r3 = plan.cost_lr(gl, gr, "sad")
    torch.cuda.synchronize()
    assert np.array_equal(host(r1.web)[0], want["checked"]) and torch.equal(r1.web, r3.web)
    el, er = oracle.find_all_edges(left, 0.15, "toroidal"), oracle.find_all_edges(right, 0.15, "toroidal")
    edge_web = oracle.hot_path(el, er, d, sw, "toroidal")[1]
    edge_right = lr.right_reference(el, er, d, sw, "toroidal")[1]
    assert np.array_equal(host(r2.web)[0], lr.lr_check(edge_web, edge_right, 0, "toroidal")[0])
    plan.close()
    # reserve_lr first: reserve_cost_lr adds only the mirrored gray images
    plan = hip.StereoPlan(w, h, d, sw, "toroidal", max_pairs=mp)
    base = plan.workspace_bytes()
    plan.reserve_lr()
    assert plan.workspace_bytes() == base + ext + mapb
    plan.reserve_cost_lr()
    assert plan.workspace_bytes() == base + ext + mapb + gray
    plan.close()
    # allocated by the first call that needs it
    plan = hip.StereoPlan(w, h, d, sw, "toroidal", max_pairs=mp)
    base = plan.workspace_bytes()
    web_right, _ = plan.cost_wta_right(gl, gr, "ssd")
    torch.cuda.synchronize()
    assert plan.workspace_bytes() == base + gray + mapb
    assert np.array_equal(host(web_right)[0], clr.right_reference(left, right, d, sw, "toroidal", "ssd")[1])
    plan.close()


def test_cost_wta_is_bit_identical_before_and_after_cost_lr(hip):
    w, h, d, sw = 320, 200, 64, 7
    a = make_pair(w, h, d, seed=11)
    b = make_pair(w, h, d, seed=12)
    plan = hip.StereoPlan(w, h, d, sw, "ghost")
    try:
        for cost in ("sad", "ssd"):
            ga = dev(a[0]), dev(a[1])
            before = [host(t) for t in plan.cost_wta(*ga, cost)]
            res = plan.cost_lr(dev(b[0]), dev(b[1]), cost, max_diff=0, want_best=True)
            plan.cost_wta_right(dev(b[0]), dev(b[1]), cost)
            after = [host(t) for t in plan.cost_wta(*ga, cost)]
            want_a = oracle.cost_hot_path(a[0], a[1], d, sw, "ghost", cost)
            assert all(np.array_equal(x, y) for x, y in zip(before, after))
            assert np.array_equal(after[0][0], want_a[1]) and np.array_equal(after[1][0], want_a[0])
            want_b = clr.expected(*b, d, sw, "ghost", cost, 0)
            assert np.array_equal(host(res.web)[0], want_b["checked"])
            assert np.array_equal(host(res.best)[0], want_b["best"])
    finally:
        plan.close()


@pytest.mark.parametrize("pipelined", [1, 2, "after"])
def test_pipelined_plan_interleaving_run_and_cost_lr(hip, pipelined):
    """calls on the lanes (a pipelined plan's run, sm_run_after) and sm_cost_lr on one plan, back to back without a
    synchronisation: every result equals the serial one"""
    w, h, d, sw = 320, 200, 64, 7
    pairs = [make_pair(w, h, d, seed=50 + i) for i in range(6)]
    want_run = [oracle.pipeline(l, r, 0.15, d, sw, step3=False)["web-1"] for l, r in pairs]
    want_lr = [clr.expected(l, r, d, sw, "toroidal", "sad", 1) for l, r in pairs]
    inputs = [(dev(l), dev(r)) for l, r in pairs]
    torch.cuda.synchronize()
    plan = hip.StereoPlan(w, h, d, sw)
    try:
        plan.prepare_threshold(0.15)
        plan.reserve_cost_lr()
        if pipelined != "after":
            plan.set_pipelined(pipelined)
        got = []
        for rep in range(2):
            for i, (l, r) in enumerate(inputs):
                if i % 3 == 2:
                    got.append(("lr", i, plan.cost_lr(l, r, "sad", max_diff=1, want_right=True)))
                elif pipelined == "after":
                    got.append(("run", i, plan.run_after(l, r, 0.15)[0]))
                else:
                    got.append(("run", i, plan.run(l, r, 0.15)[0]))
        torch.cuda.synchronize()
        for kind, i, res in got:
            if kind == "lr":
                assert np.array_equal(host(res.web)[0], want_lr[i]["checked"]), (pipelined, i)
                assert np.array_equal(host(res.web_right)[0], want_lr[i]["web_right"]), (pipelined, i)
                assert int(res.rejected[0]) == want_lr[i]["rejected"]
            else:
                assert np.array_equal(host(res)[0], want_run[i]), (pipelined, i)
    finally:
        plan.close()


@pytest.mark.parametrize("cost", ["sad", "ssd"])
def test_cost_lr_and_refine_captured_into_a_graph(hip, cost):
    w, h, d, sw, mode = 320, 200, 64, 7, "ghost"
    pairs = [make_pair(w, h, d, seed=80 + i) for i in range(3)]
    inputs = [(dev(l), dev(r)) for l, r in pairs]
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        plan.cost_wta(*inputs[0], cost)                 # (the first cost launch sets up the kernel, outside the capture)
        torch.cuda.synchronize()
        base = plan.workspace_bytes()
        webs = [torch.zeros((1, h, w), dtype=torch.int32, device="cuda") for _ in range(3)]
        rights = [torch.zeros_like(webs[0]) for _ in range(3)]
        bests = [torch.zeros_like(webs[0]) for _ in range(3)]
        subs = [torch.zeros((1, h, w), dtype=torch.int16, device="cuda") for _ in range(3)]
        # refused before reserve_cost_lr, and the capture stays valid (it ends cleanly, with the pending error the one
        # raised)
        with pytest.raises(hip.capi.StereoHipError, match="sm_plan_reserve_cost_lr"):
            with torch.cuda.graph(torch.cuda.CUDAGraph(), capture_error_mode="thread_local"):
                plan.cost_lr(*inputs[0], cost, web=webs[0])
        with pytest.raises(hip.capi.StereoHipError, match="sm_plan_reserve_cost_lr"):
            with torch.cuda.graph(torch.cuda.CUDAGraph(), capture_error_mode="thread_local"):
                plan.cost_wta_right(*inputs[0], cost, want_best=False, web_right=rights[0])
        assert plan.workspace_bytes() == base
        plan.reserve_cost_lr()
        # eager references on the reserved plan
        want = []
        for l, r in inputs:
            res = plan.cost_lr(l, r, cost, max_diff=0, want_right=True, want_best=True)
            sub, _ = plan.cost_refine(l, r, res.web, cost)
            want.append([host(t)[0] for t in (res.web, res.web_right, res.best, sub)] + [int(res.rejected[0])])
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        rej = torch.zeros(3, dtype=torch.int32, device="cuda")
        from stereomatching_amd import pipeline
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            for i, (l, r) in enumerate(inputs):
                pipeline.check(pipeline.lib.sm_cost_lr(plan._h, pipeline._ptr(l), pipeline._ptr(r),
                                                       {"sad": 1, "ssd": 2}[cost], 1, 0, pipeline._ptr(webs[i]),
                                                       pipeline._ptr(bests[i]), pipeline._ptr(rights[i]),
                                                       C.c_void_p(rej.data_ptr() + 4 * i), plan._stream()))
                plan.cost_refine(l, r, webs[i], cost, out=subs[i])
        for rep in range(2):
            for t in webs + rights + bests + subs + [rej]:
                t.zero_()
            g.replay()
            torch.cuda.synchronize()
            for i in range(3):
                got = [host(t)[0] for t in (webs[i], rights[i], bests[i], subs[i])] + [int(rej[i])]
                for k, (x, y) in enumerate(zip(got[:4], want[i][:4])):
                    assert np.array_equal(x, y), (cost, rep, i, k)
                assert got[4] == want[i][4], (cost, rep, i)
        # and the eager references are the definition's
        for i, (l, r) in enumerate(pairs):
            e = clr.expected(l, r, d, sw, mode, cost, 0)
            assert np.array_equal(want[i][0], e["checked"]) and np.array_equal(want[i][1], e["web_right"])
            assert np.array_equal(want[i][2], e["best"]) and want[i][4] == e["rejected"]
            assert np.array_equal(want[i][3], sr.refine(l, r, e["checked"], d, sw, mode, cost)[0])
    finally:
        plan.close()


@pytest.mark.parametrize("check", ["edge", "cost"])
def test_rejection_counts_are_zeroed_on_every_replay(hip, check):
    """the per-pair rejection counts start from 0 on every replay of a captured check, whatever they held before"""
    w, h, d, sw, mode = 320, 200, 64, 7, "toroidal"
    left, right = make_pair(w, h, d, seed=90)
    gl, gr = dev(left), dev(right)
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        if check == "edge":
            el, er = oracle.find_all_edges(left, 0.15, mode), oracle.find_all_edges(right, 0.15, mode)
            want = lr.lr_check(oracle.hot_path(el, er, d, sw, mode)[1], lr.right_reference(el, er, d, sw, mode)[1],
                               0, mode)
            plan.prepare_threshold(0.15)
            plan.reserve_lr()
            plan.run_lr(gl, gr, 0.15)

            def call(web):
                return plan.run_lr(gl, gr, 0.15, max_diff=0, web=web)
        else:
            want = lr.lr_check(*[clr.expected(left, right, d, sw, mode, "sad", 0)[k] for k in ("web", "web_right")],
                               0, mode)
            plan.reserve_cost_lr()
            plan.cost_lr(gl, gr, "sad")

            def call(web):
                return plan.cost_lr(gl, gr, "sad", max_diff=0, web=web)
        web = torch.zeros((1, h, w), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            res = call(web)
        for rep in range(3):
            res.rejected.fill_(12345 + rep)
            web.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(host(web)[0], want[0]), (check, rep)
            assert int(res.rejected[0]) == want[1], (check, rep)
    finally:
        plan.close()
