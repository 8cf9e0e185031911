"""Left-right consistency check on the GPU: sm_match_wta_right, sm_lr_check and sm_run_lr against the oracle on
mirrored edge images and the numpy definition of the check (tests/lr_reference.py).  Every expected value comes
from the oracle; none from the HIP path."""
import ctypes as C

import numpy as np
import pytest
import torch

from stereomatching_amd.synth import CONFIGS, make_pair
from tests import lr_reference as lr
from tests import oracle
from tests.conftest import golden_cases, load_golden

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def expected_lr(left, right, d, sw, mode, max_diff, threshold=0.15, banded=False):
    """the oracle's edges, left map / scores, right-reference map and the checked map of one gray pair"""
    fe = oracle.find_all_edges_banded if banded else oracle.find_all_edges
    el, er = fe(left, threshold, mode), fe(right, threshold, mode)
    hot = oracle.hot_path_banded if banded else oracle.hot_path
    best, web = hot(el, er, d, sw, mode)
    best_right, web_right = lr.right_reference(el, er, d, sw, mode, banded=banded)
    checked, rejected = lr.lr_check(web, web_right, max_diff, mode)
    return dict(best=best, web=web, web_right=web_right, best_right=best_right, checked=checked, rejected=rejected)


# ---------------------------------------------------------------------------
# sm_match_wta_right
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
@pytest.mark.parametrize("name", golden_cases())
def test_right_reference_map_on_golden_geometries(hip, name, mode):
    z, p = load_golden(name)
    el, er = z["edges-1"], z["edges-2"]
    h, w = el.shape
    plan = hip.StereoPlan(w, h, 30, p["square_width"], mode)
    plan.load_edges(dev(el), dev(er))
    web_right, best_right = plan.match_wta_right(1)
    ob, ow = lr.right_reference(el, er, 30, p["square_width"], mode)
    assert np.array_equal(host(web_right)[0], ow), (name, mode, plan.describe())
    assert np.array_equal(host(best_right)[0], ob), (name, mode)
    # the left map of the same plan is untouched by the right-reference pass
    web, _ = plan.match_wta(1, want_best=False)
    assert np.array_equal(host(web)[0], oracle.hot_path(el, er, 30, p["square_width"], mode)[1])
    plan.close()


KERNEL_CHOICES = [dict(kernel_family=1), dict(shifts_per_lane=4), dict(shifts_per_lane=8), dict(shifts_per_lane=16),
                  dict(workgroup_waves=1), dict(workgroup_waves=2), dict(lane_merge=1), dict(lane_merge=2),
                  dict(edge_kernel=1), None]


@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
@pytest.mark.parametrize("w,h,d,sw", [(300, 150, 128, 9), (71, 53, 30, 5), (130, 70, 64, 7), (90, 61, 64, 11),
                                      (257, 61, 64, 7), (64, 40, 100, 3)])
@pytest.mark.parametrize("opts", KERNEL_CHOICES, ids=lambda o: "default" if o is None else
                         "-".join(f"{k}{v}" for k, v in o.items()))
def test_every_kernel_choice_has_a_right_reference_mode(hip, opts, w, h, d, sw, mode):
    left, right = make_pair(w, h, d, seed=w + d)
    want = expected_lr(left, right, d, sw, mode, max_diff=1)
    plan = hip.StereoPlan(w, h, d, sw, mode, options=opts)
    plan.find_all_edges(dev(left), dev(right), 0.15, want_edges=False)
    web_right, best_right = plan.match_wta_right(1)
    assert np.array_equal(host(web_right)[0], want["web_right"]), plan.describe()
    assert np.array_equal(host(best_right)[0], want["best_right"]), plan.describe()
    res = plan.run_lr(dev(left), dev(right), 0.15, max_diff=1, want_right=True, want_best=True)
    assert np.array_equal(host(res.web)[0], want["checked"]), plan.describe()
    assert np.array_equal(host(res.web_right)[0], want["web_right"])
    assert np.array_equal(host(res.best)[0], want["best"])
    assert int(res.rejected[0]) == want["rejected"]
    plan.close()


# ---------------------------------------------------------------------------
# sm_lr_check
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
@pytest.mark.parametrize("w,h,d,pairs", [(64, 20, 30, 1), (67, 13, 16, 3), (128, 9, 200, 4), (5, 7, 3, 2)])
@pytest.mark.parametrize("max_diff", [0, 1, 3, 1000])
def test_check_against_the_definition(hip, mode, w, h, d, pairs, max_diff):
    rng = np.random.default_rng(w * 7 + pairs)
    web = rng.integers(1, d + 1, (pairs, h, w)).astype(np.int32)
    web_right = rng.integers(1, d + 1, (pairs, h, w)).astype(np.int32)
    # a share of consistent pixels, so that both outcomes occur
    for q in range(pairs):
        x = np.arange(w)[None, :]
        u = (x + web[q] - 1) % w if mode == "toroidal" else np.clip(x + web[q] - 1, 0, w - 1)
        agree = rng.random((h, w)) < 0.5
        np.put_along_axis(web_right[q], u, np.where(agree, web[q], np.take_along_axis(web_right[q], u, 1)), 1)
    want = [lr.lr_check(web[q], web_right[q], max_diff, mode) for q in range(pairs)]
    plan = hip.StereoPlan(w, h, d, 0, mode, max_pairs=pairs)
    gw, gr = dev(web), dev(web_right)
    out, rejected = plan.lr_check(gw, gr, max_diff)                      # out of place
    for q in range(pairs):
        assert np.array_equal(host(out)[q], want[q][0]), q
        assert int(rejected[q]) == want[q][1] == int((host(out)[q] == 0).sum())
    assert np.array_equal(host(gw), web)                                 # the input is untouched
    inplace, rej2 = plan.lr_check(gw, gr, max_diff, out=gw)              # in place
    assert inplace.data_ptr() == gw.data_ptr()
    assert np.array_equal(host(gw), host(out)) and torch.equal(rej2, rejected)
    # maps that do not start on a 16-byte boundary take the scalar path: the same results
    buf = torch.zeros(pairs * h * w + 1, dtype=torch.int32, device="cuda")
    shifted = buf[1:].view(pairs, h, w)
    shifted.copy_(dev(web))
    out3, rej3 = plan.lr_check(shifted, gr, max_diff)
    assert np.array_equal(host(out3), host(out)) and torch.equal(rej3, rejected)
    plan.close()


def test_check_of_values_no_match_produces(hip):
    """0, negative and huge values: what the formula gives (ghost: a partner outside the row is a rejection),
    and no read outside the row"""
    w, h = 37, 5
    rng = np.random.default_rng(9)
    web = rng.integers(-3 * w, 3 * w, (h, w)).astype(np.int32)
    web[0, :4] = [0, -1, 2**31 - 1, -2**31]
    web_right = rng.integers(-3 * w, 3 * w, (h, w)).astype(np.int32)
    for mode in ("toroidal", "ghost"):
        plan = hip.StereoPlan(w, h, 30, 3, mode)
        out, rejected = plan.lr_check(dev(web), dev(web_right), 2)
        want, nrej = lr.lr_check(web, web_right, 2, mode)
        assert np.array_equal(host(out)[0], want), mode
        assert int(rejected[0]) == nrej, mode
        plan.close()


@pytest.mark.parametrize("w", [8, 7])
def test_check_of_differences_past_32_bits(hip, w):
    """web_right(u) - web(x) is a 33-bit number and is compared as one (the mutation audit's L2: a subtraction modulo
    2^32 passed every other test here; tests/lr_patterns.py, with the CPU proof in tests/test_lr_cpu.py).  Pairs of
    values 2^32 - 2 and 2^32 - 1 apart are rejected at max_diff = 2 although modulo 2^32 they differ by 2 and 1, and a
    partner 2^31 + 1 .. 2^31 + 3 away is rejected at max_diff = 2^31 - 1, the largest there is, in both border modes.
    Two rows of 8 columns take the four-pixel lanes, of 7 the one-pixel lanes; 7 is the least width whose row holds the
    three planted pixels and their partners apart."""
    from tests import lr_patterns as lp
    web, right = lp.wide_difference_maps(w)
    for max_diff, mode in lp.WIDE_CHECKS:
        plan = hip.StereoPlan(w, lp.WIDE_H, 4, 1, mode)
        out, rejected = plan.lr_check(dev(web[None]), dev(right[None]), max_diff)
        want, nrej = lr.lr_check(web, right, max_diff, mode)
        assert np.array_equal(host(out)[0], want), (max_diff, mode)
        assert int(rejected[0]) == nrej, (max_diff, mode)
        plan.close()


# ---------------------------------------------------------------------------
# sm_run_lr at full size, every pixel
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("cfg,pairs,max_diff", [("C3", 1, 0), ("C5", 1, 1), ("REF1080", 1, 0), ("C4", 8, 2)])
def test_run_lr_full_size_every_pixel(hip, cfg, pairs, max_diff):
    w, h, d, sw, mode = (1920, 1080, 30, 21, "toroidal") if cfg == "REF1080" else CONFIGS[cfg]
    imgs = [make_pair(w, h, d, seed=40 + q) for q in range(pairs)]
    plan = hip.StereoPlan(w, h, d, sw, mode, max_pairs=pairs)
    left = dev(np.stack([a for a, _ in imgs]))
    right = dev(np.stack([b for _, b in imgs]))
    res = plan.run_lr(left, right, 0.15, max_diff=max_diff, want_right=True, want_best=True)
    torch.cuda.synchronize()
    for q, (a, b) in enumerate(imgs):
        want = expected_lr(a, b, d, sw, mode, max_diff, banded=True)
        assert np.array_equal(host(res.web_right[q]), want["web_right"]), (cfg, q, plan.describe())
        assert np.array_equal(host(res.best[q]), want["best"]), (cfg, q)
        assert np.array_equal(host(res.web[q]), want["checked"]), (cfg, q)
        assert int(res.rejected[q]) == want["rejected"] > 0, (cfg, q)
    plan.close()


# ---------------------------------------------------------------------------
# end to end: the rejected pixels go through step 3
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode,w,h,d,sw,times,lines", [("toroidal", 320, 96, 128, 9, 4, 5), ("ghost", 200, 70, 30, 21, 32, 10),
                                                       ("toroidal", 257, 61, 64, 7, 2, 7)])
@pytest.mark.parametrize("max_diff", [0, 1])
def test_checked_map_through_step3(hip, mode, w, h, d, sw, times, lines, max_diff):
    left, right = make_pair(w, h, d, seed=7)
    want = expected_lr(left, right, d, sw, mode, max_diff)
    assert (want["checked"] == 0).any()                 # holes, so that hole filling does work
    web2 = oracle.fill_web_holes(want["checked"], times)
    out = oracle.draw_contour_map(web2, lines)
    plan = hip.StereoPlan(w, h, d, sw, mode)
    res = plan.algorithm(dev(left), dev(right), hip.AlgorithmParams(0.15, sw, times, lines), lr_max_diff=max_diff)
    assert np.array_equal(host(res["web-1"])[0], want["checked"])
    assert np.array_equal(host(res["web_right-1"])[0], want["web_right"])
    assert int(res["lr_rejected"][0]) == want["rejected"]
    assert np.array_equal(host(res["web-2"])[0], web2)
    assert np.array_equal(host(res["output-0"])[0], out)
    # sm_run_lr, then the one-synchronisation step 3 (which takes its staged route on a map with holes)
    r = plan.run_lr(dev(left), dev(right), 0.15, max_diff=max_diff)
    filled, contour, mm = plan.step3(r.web, times, lines)
    assert np.array_equal(host(filled)[0], web2) and np.array_equal(host(contour)[0], out)
    assert host(mm)[0].tolist() == [int(web2.min()), int(web2.max())]
    # without lr_max_diff nothing changes
    res0 = plan.algorithm(dev(left), dev(right), hip.AlgorithmParams(0.15, sw, times, lines))
    assert np.array_equal(host(res0["web-1"])[0], want["web"]) and "web_right-1" not in res0
    plan.close()


# ---------------------------------------------------------------------------
# workspace, arguments, isolation, ordering, capture
# ---------------------------------------------------------------------------

def test_workspace_is_allocated_only_for_the_check(hip):
    w, h, d, sw = 300, 150, 128, 9
    plan = hip.StereoPlan(w, h, d, sw, "toroidal", max_pairs=2)
    base, desc, geom = plan.workspace_bytes(), plan.describe(), plan.geometry()
    left, right = make_pair(w, h, d, seed=3)
    plan.run(dev(left), dev(right), 0.15)
    plan.lr_check(dev(np.ones((h, w), np.int32)), dev(np.ones((h, w), np.int32)), 0)   # no workspace needed
    torch.cuda.synchronize()
    assert plan.workspace_bytes() == base and plan.describe() == desc and plan.geometry() == geom
    plan.reserve_lr()
    plan.reserve_lr()                                                    # idempotent
    ext = 2 * 2 * geom["ext_words"] * geom["ext_rows"] * 4               # max_pairs x two mirrored packed images
    assert plan.workspace_bytes() == base + ext + 2 * w * h * 4
    assert plan.describe() == desc and plan.geometry() == geom
    plan.close()
    plan = hip.StereoPlan(w, h, d, sw, "toroidal")                       # allocated by the first call that needs it
    base = plan.workspace_bytes()
    plan.run_lr(dev(left), dev(right), 0.15)
    torch.cuda.synchronize()
    assert plan.workspace_bytes() > base
    plan.close()


def test_argument_checks_on_a_plan(hip):
    from stereomatching_amd import capi
    lib = capi.lib
    w, h, d = 64, 32, 16
    plan = hip.StereoPlan(w, h, d, 5, "toroidal", max_pairs=2)
    m = [torch.zeros((2, h, w), dtype=torch.int32, device="cuda") for _ in range(3)]
    p = [C.c_void_p(t.data_ptr()) for t in m]
    g = torch.zeros((2, h, w), dtype=torch.uint8, device="cuda")
    gp = C.c_void_p(g.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def refused(rc, text):
        assert rc == capi.SM_ERR_ARG and text in lib.sm_last_error(), lib.sm_last_error()
    refused(lib.sm_match_wta_right(plan._h, 1, p[0], None, st), b"edges of only 0 are loaded")
    refused(lib.sm_match_wta_right(plan._h, 3, p[0], None, st), b"outside 1..2")
    refused(lib.sm_lr_check(plan._h, p[0], p[1], -1, 1, p[2], None, st), b"max_diff")
    refused(lib.sm_lr_check(plan._h, p[0], p[1], 0, 0, p[2], None, st), b"outside 1..2")
    refused(lib.sm_lr_check(plan._h, p[0], p[1], 0, 1, p[1], None, st), b"d_web_right overlaps d_web_out")
    refused(lib.sm_run_lr(plan._h, gp, gp, 0.15, 3, 0, p[0], None, None, None, st), b"outside 1..2")
    refused(lib.sm_run_lr(plan._h, gp, gp, 0.15, 1, 0, p[0], p[0], None, None, st), b"overlap")
    assert plan.workspace_bytes() == hip.StereoPlan(w, h, d, 5, "toroidal", max_pairs=2).workspace_bytes()
    with pytest.raises(ValueError):
        plan.lr_check(m[0][:1], m[1], 0)                                  # pairs differ
    plan.close()


def test_run_is_bit_identical_before_and_after_run_lr(hip):
    w, h, d, sw = 320, 200, 64, 7
    a = make_pair(w, h, d, seed=11)
    b = make_pair(w, h, d, seed=12)
    want_a = oracle.pipeline(*a, 0.15, d, sw, step3=False)["web-1"]
    plan = hip.StereoPlan(w, h, d, sw)
    before = host(plan.run(dev(a[0]), dev(a[1]), 0.15)[0])
    lrres = plan.run_lr(dev(b[0]), dev(b[1]), 0.15, max_diff=0)
    # the edges sm_run_lr loaded are the plan's now (as after sm_run): the left match of pair b
    web_b, _ = plan.match_wta(1, want_best=False)
    after = host(plan.run(dev(a[0]), dev(a[1]), 0.15)[0])
    torch.cuda.synchronize()
    assert np.array_equal(before, after) and np.array_equal(after[0], want_a)
    want_b = expected_lr(*b, d, sw, "toroidal", 0)
    assert np.array_equal(host(web_b)[0], want_b["web"]) and np.array_equal(host(lrres.web)[0], want_b["checked"])
    plan.close()


@pytest.mark.parametrize("pipelined", [1, 2, "after"])
def test_pipelined_plan_interleaving_run_and_run_lr(hip, pipelined):
    """calls on the lanes (a pipelined plan's run, sm_run_after) and sm_run_lr on one plan, back to back without a
    synchronisation: every result equals the serial one"""
    w, h, d, sw = 320, 200, 64, 7
    pairs = [make_pair(w, h, d, seed=50 + i) for i in range(6)]
    want = [expected_lr(l, r, d, sw, "toroidal", 1) for l, r in pairs]
    inputs = [(dev(l), dev(r)) for l, r in pairs]
    torch.cuda.synchronize()
    plan = hip.StereoPlan(w, h, d, sw)
    plan.prepare_threshold(0.15)
    if pipelined != "after":
        plan.set_pipelined(pipelined)
    got = []
    for rep in range(2):
        for i, (l, r) in enumerate(inputs):
            if i % 3 == 2:
                got.append(("lr", i, plan.run_lr(l, r, 0.15, max_diff=1, want_right=True)))
            elif pipelined == "after":
                got.append(("run", i, plan.run_after(l, r, 0.15)[0]))
            else:
                got.append(("run", i, plan.run(l, r, 0.15)[0]))
    torch.cuda.synchronize()
    for kind, i, res in got:
        if kind == "lr":
            assert np.array_equal(host(res.web)[0], want[i]["checked"]), (pipelined, i)
            assert np.array_equal(host(res.web_right)[0], want[i]["web_right"]), (pipelined, i)
            assert int(res.rejected[0]) == want[i]["rejected"]
        else:
            assert np.array_equal(host(res)[0], want[i]["web"]), (pipelined, i)
    plan.close()


@pytest.mark.parametrize("pipelined", [False, True])
def test_run_lr_captured_into_a_graph(hip, pipelined):
    w, h, d, sw = 320, 200, 64, 7
    pairs = [make_pair(w, h, d, seed=80 + i) for i in range(3)]
    want = [expected_lr(l, r, d, sw, "toroidal", 0) for l, r in pairs]
    inputs = [(dev(l), dev(r)) for l, r in pairs]
    plan = hip.StereoPlan(w, h, d, sw)
    plan.prepare_threshold(0.15)
    plan.run(*inputs[0], 0.15)                                        # edges loaded
    plan.set_pipelined(pipelined)
    webs = [torch.zeros((1, h, w), dtype=torch.int32, device="cuda") for _ in range(3)]
    rights = [torch.zeros_like(webs[0]) for _ in range(3)]
    torch.cuda.synchronize()
    # refused before reserve_lr, and the capture stays valid (it ends cleanly, with the pending error the one raised)
    with pytest.raises(hip.capi.StereoHipError, match="sm_plan_reserve_lr"):
        with torch.cuda.graph(torch.cuda.CUDAGraph(), capture_error_mode="thread_local"):
            plan.run_lr(*inputs[0], 0.15, web=webs[0])
    with pytest.raises(hip.capi.StereoHipError, match="sm_plan_reserve_lr"):
        with torch.cuda.graph(torch.cuda.CUDAGraph(), capture_error_mode="thread_local"):
            plan.match_wta_right(1, want_best=False, web_right=rights[0])
    assert plan.workspace_bytes() == hip.StereoPlan(w, h, d, sw).workspace_bytes()
    plan.reserve_lr()
    with pytest.raises(hip.capi.StereoHipError, match="sm_plan_prepare_threshold"):
        with torch.cuda.graph(torch.cuda.CUDAGraph(), capture_error_mode="thread_local"):
            plan.run_lr(*inputs[0], 0.33, web=webs[0])
    g = torch.cuda.CUDAGraph()
    others = [torch.zeros_like(webs[0]) for _ in range(3)]
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        for i, (l, r) in enumerate(inputs):
            plan.run(l, r, 0.15, web=others[i])                       # (pipelined: on the lanes, inside the graph)
            plan.run_lr(l, r, 0.15, max_diff=0, web=webs[i], web_right=rights[i], want_right=True)
    for rep in range(2):
        for t in webs + rights + others:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for i in range(3):
            assert np.array_equal(host(webs[i])[0], want[i]["checked"]), (pipelined, rep, i)
            assert np.array_equal(host(rights[i])[0], want[i]["web_right"]), (pipelined, rep, i)
            assert np.array_equal(host(others[i])[0], want[i]["web"]), (pipelined, rep, i)
        # eager calls between replays
        r = plan.run_lr(*inputs[rep], 0.15, max_diff=0)
        torch.cuda.synchronize()
        assert np.array_equal(host(r.web)[0], want[rep]["checked"])
    plan.close()
