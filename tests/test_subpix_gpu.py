"""Subpixel refinement of the cost mode on the GPU (sm_cost_refine, StereoPlan.cost_refine) against the numpy
definition of tests/subpix_reference.py.  sub and the three costs must EQUAL the definition.  The whole-pixel maps
come from the plan's cost_wta (itself checked against the oracle elsewhere); every expected value is computed from
those maps and the images by the definition, none by the HIP path."""
import ctypes as C

import numpy as np
import pytest
import torch

from stereomatching_amd import capi
from stereomatching_amd.synth import CONFIGS, make_pair
from tests import extreme_patterns as ep
from tests import oracle
from tests import subpix_reference as sr
from tests.test_subpix_cpu import ACCURACY_T, accuracy

pytestmark = pytest.mark.gpu

SWEEP_PATTERNS = ("black_white", "white_black", "both_0", "both_77", "checker_2", "zero_cost_column")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def gpu_pairs(w, h, d, seed, patterns=SWEEP_PATTERNS):
    """random pairs, a scene with real disparities, and the named gray patterns, stacked"""
    rng = np.random.default_rng(seed)
    left = [rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 4, (h, w), dtype=np.uint8) * 60]
    right = [rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 4, (h, w), dtype=np.uint8) * 60]
    sl, sr_ = make_pair(w, h, max(1, d), seed=seed)
    left.append(sl)
    right.append(sr_)
    for p in patterns:
        a, b = ep.gray_pattern(p, w, h)
        left.append(a)
        right.append(b)
    return np.stack(left), np.stack(right)


def check_against_definition(plan, left, right, web, cost, d, sw, mode, what):
    sub, costs = plan.cost_refine(dev(left), dev(right), web, cost, want_costs=True)
    torch.cuda.synchronize()
    sub, costs, web = host(sub), host(costs), host(web)
    for p in range(left.shape[0]):
        want_sub, want_costs = sr.refine(left[p], right[p], web[p], d, sw, mode, cost)
        for k in range(3):
            bad = np.argwhere(costs[p, k] != want_costs[k])
            assert bad.size == 0, (what, p, k, bad[:4].tolist(), plan.describe())
        bad = np.argwhere(sub[p] != want_sub)
        assert bad.size == 0, (what, p, bad[:4].tolist(), plan.describe())
    return sub, costs


@pytest.mark.parametrize("d", [1, 2, 3, 64, 128, 256, 512])
@pytest.mark.parametrize("n", [1, 3, 5, 9, 11, 13, 15, 17, 19, 21, 23, 25])
@pytest.mark.parametrize("cost", ["sad", "ssd"])
@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
def test_sweep_against_the_definition(hip, mode, cost, n, d):
    w, h = 64 + n % 7, n + 6                       # (w % 4 takes 0 .. 3 over the windows)
    left, right = gpu_pairs(w, h, d, seed=n * 1000 + d)
    plan = hip.StereoPlan(w, h, d, n, mode, max_pairs=left.shape[0])
    try:
        web, best = plan.cost_wta(dev(left), dev(right), cost)
        _, costs = check_against_definition(plan, left, right, web, cost, d, n, mode, (mode, cost, n, d))
        assert np.array_equal(costs[:, 1], host(best))
    finally:
        plan.close()


# the plan's choice, the general masked kernel (cost_kernel = 1) and the fast kernels in workgroups of 1, 2 and 4 waves
KERNEL_CHOICES = ([(c, dict(cost_kernel=k)) for c in ("sad", "ssd") for k in (0, 1)] +
                  [(c, dict(cost_kernel=0, cost_workgroup_waves=wv)) for c in ("sad", "ssd") for wv in (1, 2, 4)])


@pytest.mark.parametrize("cost,opts", KERNEL_CHOICES,
                         ids=lambda v: v if isinstance(v, str) else "-".join(f"{k}{x}" for k, x in v.items()))
@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
@pytest.mark.parametrize("w,h,d,n", [(160, 40, 64, 9), (132, 36, 256, 11), (100, 30, 30, 5)])
def test_winner_cost_equals_best_of_every_cost_kernel(hip, mode, cost, opts, w, h, d, n):
    """C(s - 1) recomputed by the refinement equals best of cost_wta, whichever kernel the plan options pick for
    cost_wta: two independent computations of one window sum"""
    left, right = gpu_pairs(w, h, d, seed=d + n, patterns=("black_white", "both_77"))
    plan = hip.StereoPlan(w, h, d, n, mode, max_pairs=left.shape[0], options=opts)
    try:
        web, best = plan.cost_wta(dev(left), dev(right), cost)
        sub, costs = plan.cost_refine(dev(left), dev(right), web, cost, want_costs=True)
        assert np.array_equal(host(costs)[:, 1], host(best)), plan.describe()
        assert (np.abs(host(sub).astype(np.int32) - 16 * host(web)) <= 8).all()
    finally:
        plan.close()


@pytest.mark.parametrize("cost", ["sad", "ssd"])
@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
def test_caller_made_maps(hip, mode, cost):
    """0, -1, D + 1 get no taps (sub 0, costs -1); 1 and D only their existing neighbours; random values in
    1..D exercise the clamp and the non-positive denominators"""
    w, h, d, n = 67, 23, 40, 7
    rng = np.random.default_rng(9)
    left, right = rng.integers(0, 256, (2, 2, h, w), dtype=np.uint8)
    web = np.stack([np.array([0, -1, d + 1, 1, d, 2, d - 1], np.int32)[rng.integers(0, 7, (h, w))],
                    rng.integers(1, d + 1, (h, w)).astype(np.int32)])
    plan = hip.StereoPlan(w, h, d, n, mode, max_pairs=2)
    try:
        sub, costs = check_against_definition(plan, left, right, dev(web), cost, d, n, mode, "caller maps")
        m = np.isin(web[0], (0, -1, d + 1))
        assert (sub[0][m] == 0).all() and (costs[0][:, m] == -1).all()
        assert (sub[0][web[0] == 1] == 16).all() and (sub[0][web[0] == d] == 16 * d).all()
        assert (np.abs(sub[1] - 16 * web[1]) == 8).any()             # (the clamp is reached)
    finally:
        plan.close()


def test_argument_checks_on_a_plan(hip):
    w, h, d, n = 64, 24, 16, 5
    plan = hip.StereoPlan(w, h, d, n, "toroidal", max_pairs=2)
    try:
        l = dev(np.zeros((2, h, w), np.uint8))
        web = dev(np.ones((2, h, w), np.int32))
        sub = torch.full((2, h, w), 1234, dtype=torch.int16, device="cuda")
        P = lambda t: C.c_void_p(t.data_ptr())
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        calls = {
            "pairs 0": (0, P(web), P(sub), 1),
            "pairs 3": (3, P(web), P(sub), 1),
            "NULL web": (1, None, P(sub), 1),
            "NULL sub": (1, P(web), None, 1),
            "bad cost": (1, P(web), P(sub), 3),
        }
        for what, (pairs, pw, ps, cost) in calls.items():
            with pytest.raises(capi.StereoHipError) as e:
                capi.check(capi.lib.sm_cost_refine(plan._h, P(l), P(l), cost, pairs, pw, ps, None, st))
            assert e.value.code == capi.SM_ERR_ARG, what
            assert "sm_cost_refine" in e.value.message, what
        torch.cuda.synchronize()
        assert (host(sub) == 1234).all()
        with pytest.raises(ValueError):
            plan.cost_refine(l, l, web[:, :, :-1])
    finally:
        plan.close()


@pytest.mark.parametrize("cost", ["sad", "ssd"])
@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
@pytest.mark.parametrize("w,h,d,sw,pairs", [
    (61, 17, 20, 9, 3),         # w % 4 == 1
    (62, 33, 100, 11, 2),       # w % 4 == 2, the span wider than the image
    (131, 9, 7, 5, 4),          # w % 4 == 3, shorter than a tile
    (24, 24, 12, 24, 2),        # a 25 x 25 window on a 24 x 24 image: narrower and shorter than the window
    (9, 30, 5, 8, 2),           # a 9 x 9 window on 9 columns
    (257, 5, 300, 4, 3),        # more shifts than columns
])
def test_unaligned_small_and_batched(hip, mode, cost, w, h, d, sw, pairs):
    rng = np.random.default_rng(w * h)
    left, right = rng.integers(0, 256, (2, pairs, h, w), dtype=np.uint8)
    left[-1] = 200
    right[-1] = 3
    plan = hip.StereoPlan(w, h, d, sw, mode, max_pairs=pairs)
    try:
        web, best = plan.cost_wta(dev(left), dev(right), cost)
        _, costs = check_against_definition(plan, left, right, web, cost, d, sw, mode, (w, h, d, sw))
        assert np.array_equal(costs[:, 1], host(best))
    finally:
        plan.close()


@pytest.mark.parametrize("cfg,cost", [("C3", "sad"), ("C3", "ssd"), ("C5", "ssd")])
def test_full_size_on_bands_of_rows(hip, cfg, cost):
    w, h, d, sw, mode = CONFIGS[cfg]
    left, right = make_pair(w, h, d, seed=3)
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        web, best = plan.cost_wta(dev(left), dev(right), cost)
        sub, costs = plan.cost_refine(dev(left), dev(right), web, cost, want_costs=True)
        torch.cuda.synchronize()
        web, best, sub, costs = host(web)[0], host(best)[0], host(sub)[0], host(costs)[0]
        assert np.array_equal(costs[1], best)
        # rows of the first and last tiles and a band in the middle; the whole-pixel maps of those rows from the
        # oracle, on the band and its window halo (as oracle.cost_hot_path_banded does it)
        half = sw // 2
        for y0, y1 in ((0, 20), (h // 2 - 7, h // 2 + 9), (h - 20, h)):
            if mode == "toroidal":
                rows, lo = np.arange(y0 - half, y1 + half) % h, half
            else:
                a, b = max(0, y0 - half), min(h, y1 + half)
                rows, lo = np.arange(a, b), y0 - a
            ob, ow = oracle.cost_hot_path(left[rows], right[rows], d, sw, mode, cost)
            assert np.array_equal(ow[lo:lo + y1 - y0], web[y0:y1]), (cfg, cost, y0)
            assert np.array_equal(ob[lo:lo + y1 - y0], best[y0:y1]), (cfg, cost, y0)
            want_sub, want_costs = sr.refine(left, right, web, d, sw, mode, cost, rows=(y0, y1))
            assert np.array_equal(costs[:, y0:y1], want_costs), (cfg, cost, y0)
            assert np.array_equal(sub[y0:y1], want_sub), (cfg, cost, y0)
    finally:
        plan.close()


def _gpu_refine(hip):
    plans = {}

    def refine(left, right, web, d, sw, mode, cost):
        h, w = left.shape
        plan = plans.setdefault((w, h, d, sw, mode), hip.StereoPlan(w, h, d, sw, mode))
        gl, gr = dev(left), dev(right)
        gweb, _ = plan.cost_wta(gl, gr, cost)
        assert np.array_equal(host(gweb)[0], web)
        sub, _ = plan.cost_refine(gl, gr, gweb, cost)
        return host(sub)[0], None
    return refine, plans


@pytest.mark.parametrize("cost", ["sad", "ssd"])
@pytest.mark.parametrize("t", ACCURACY_T)
def test_accuracy_through_the_gpu(hip, cost, t):
    refine, plans = _gpu_refine(hip)
    try:
        sub_err, int_err = accuracy(cost, t, refine=refine)
    finally:
        for p in plans.values():
            p.close()
    assert sub_err <= 0.15
    if t != int(t):
        assert sub_err < 0.5 * int_err


@pytest.mark.parametrize("cost", ["sad", "ssd"])
def test_cost_wta_and_refine_captured_in_one_graph(hip, cost):
    w, h, d, sw, mode = 200, 70, 48, 9, "ghost"
    inputs = [make_pair(w, h, d, seed=s) for s in (1, 2)]
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        gl, gr = dev(inputs[0][0]), dev(inputs[0][1])
        web = torch.empty((1, h, w), dtype=torch.int32, device="cuda")
        best = torch.empty_like(web)
        sub = torch.empty((1, h, w), dtype=torch.int16, device="cuda")
        plan.cost_wta(gl, gr, cost, web=web, best=best)              # (warm-up outside the capture)
        plan.cost_refine(gl, gr, web, cost, out=sub)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                plan.cost_wta(gl, gr, cost, web=web, best=best)
                plan.cost_refine(gl, gr, web, cost, out=sub)
        torch.cuda.current_stream().wait_stream(s)
        for left, right in inputs:
            gl.copy_(dev(left))
            gr.copy_(dev(right))
            g.replay()
            torch.cuda.synchronize()
            got = host(sub).copy()
            want_web, _ = plan.cost_wta(dev(left), dev(right), cost)
            want_sub, _ = plan.cost_refine(dev(left), dev(right), want_web, cost)
            torch.cuda.synchronize()
            assert np.array_equal(got, host(want_sub))
            assert np.array_equal(host(web), host(want_web))
            ref_sub, _ = sr.refine(left, right, host(want_web)[0], d, sw, mode, cost)
            assert np.array_equal(got[0], ref_sub)
        del g
    finally:
        plan.close()
