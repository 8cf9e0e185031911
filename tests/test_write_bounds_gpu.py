"""Every GPU entry point writes all of its maps and nothing else (tests/guarded.py).

The C ABI is called directly (stereomatching_amd.capi.lib), every output and input inside guards at offset 0 and at
its misaligned offset.  Each call is made twice, once per poison: the guards must be intact, the owned elements the
same in both runs (an element that differs was not written), equal to the CPU definition, and the inputs unchanged.
Parity tests elsewhere compare values only, on maps from the caching allocator that may already hold the answer.

Each test walks its cases and reports every failing (entry point, output, case) in one assertion message."""
import ctypes as C

import numpy as np
import pytest
import torch

from stereomatching_amd import capi
from stereomatching_amd.capi import lib
from stereomatching_amd.synth import make_pair
from tests import cost_lr_reference as clr
from tests import lr_reference as lr
from tests import oracle
from tests import subpix_reference as sr
from tests.guarded import guarded, guarded_input
from tests.test_cost_lr_gpu import COST_CHOICES, COST_SHAPES
from tests.test_hip_gpu import BUILT_BS, NO_CAP2, ONE_WAVE, TWO_WAVES
from tests.test_lr_gpu import KERNEL_CHOICES
from tests.test_lr_sweep_gpu import POPCOUNT

pytestmark = pytest.mark.gpu
MODES = ["toroidal", "ghost"]
DEV = "cuda"
THR = 0.15
WIDTHS = [1, 3, 31, 33, 65, 130, 257, 64]     # every int4 / dword / packed-store tail ragged, and one multiple of 64
NARROW = {capi.SM_WEB_I32: (torch.int32, 4), capi.SM_WEB_U16: (torch.uint16, 2), capi.SM_WEB_U8: (torch.uint8, 1)}
COSTS = {"sad": 1, "ssd": 2}


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Plan:
    def __init__(self, w, h, d, sw, mode, max_pairs, options=None):
        self.h = C.c_void_p(0)
        opts = capi.PlanOptions.make(**options) if options else None
        capi.check(lib.sm_plan_create_ex(0, w, h, d, sw, capi.BORDERS[mode], max_pairs,
                                         C.byref(opts) if opts is not None else None, C.byref(self.h)))
        self.desc = lib.sm_plan_describe(self.h).decode()

    def close(self):
        lib.sm_plan_destroy(self.h)


def twice(tag, call, outs, ins=(), partial=()):
    """call() once per poison -> problems; `partial`: outputs checked for their guards only"""
    bad = []
    for run in (0, 1):
        for g in outs:
            g.fill(run)
        rc = call(run)
        if rc != capi.SM_OK:
            return [f"{tag}: returned {rc}: {lib.sm_last_error().decode(errors='replace')}"]
        torch.cuda.synchronize()
        for g in outs:
            bad += [f"{tag}: {p}" for p in g.problems() if not (g in partial and "not written" in p)]
    for i in ins:
        bad += [f"{tag}: {p}" for p in i.problems()]
    return bad


def expect(tag, g, want):
    got = g.value()
    want = np.asarray(want).reshape(got.shape)
    bad = np.argwhere(got != want)
    if len(bad):
        i = tuple(int(v) for v in bad[0])
        return [f"{tag}: {g.name}: {len(bad)} elements differ from the definition, first {i}: {got[i]} != {want[i]}"]
    return []


def out(shape, dtype, off, max_pairs, name):
    return guarded(shape, dtype, DEV, offset=off, max_pairs=max_pairs, name=name)


def report(bad):
    assert not bad, f"{len(bad)} problems:\n" + "\n".join(bad[:200])


# ---------------------------------------------------------------------------
# the edge matcher
# ---------------------------------------------------------------------------

def edge_cases(mode):
    """(options, w, h, d, sw, pairs, max_pairs, must_say)"""
    cases = []
    for i, (n, ds) in enumerate(BUILT_BS):
        for merge in (1, 2):
            shape = (ONE_WAVE, TWO_WAVES, dict(ONE_WAVE, **NO_CAP2))[(i + merge) % 3]
            ws = [w for w in WIDTHS if w >= n]
            w = ws[(i + merge) % len(ws)]
            d = 2 * ds - (i % 2) * 3
            opts = dict(shape, shifts_per_lane=ds, tile_h=4, lane_merge=merge)
            say = [f"lanes of {ds})"] + (["two-wave workgroups"] if shape is TWO_WAVES else [])
            cases.append((opts, w, n + 3 + (i % 4), d, n, 2, 3, say))
    for j, opts in enumerate(KERNEL_CHOICES):
        for k, w in enumerate(WIDTHS):
            if (j + k) % 3:
                continue
            sw = min(w, (3, 5, 7, 9)[k % 4])
            cases.append((opts, w, 13 + k, (30, 64, 100)[j % 3], sw, 1 if k % 2 else 2, 1 if k % 2 else 3, []))
    for fam, windows in POPCOUNT.items():
        for k, sw in enumerate(windows):
            w = [x for x in WIDTHS if x >= max(sw, 1)][k % 4]
            cases.append((dict(kernel_family=1), w, max(sw, 1) + 2 + k, (16, 17, 200)[k % 3], sw, 2, 3,
                          [f"tiled kernel {fam}"]))
    for sw, w, d in ((27, 33, 30), (31, 64, 65), (5, 31, 1100)):
        cases.append((None, w, sw + 2, d, sw, 2, 3, ["generic kernel"]))
    return cases


def edge_inputs(w, h, d, pairs, seed):
    imgs = [make_pair(w, h, d, seed=seed + q, kind="noise" if q % 2 else "scene") for q in range(pairs)]
    return np.stack([a for a, _ in imgs]), np.stack([b for _, b in imgs])


def check_edge_case(mode, case, idx):
    opts, w, h, d, sw, pairs, maxp, say = case
    tag = f"{mode} W={w} H={h} D={d} S={sw} pairs={pairs}/{maxp} {opts or 'default'}"
    plan = Plan(w, h, d, sw, mode, maxp, opts)
    bad = [f"{tag}: plan is not the one named ('{s}' missing): {plan.desc}" for s in say if s not in plan.desc]
    tag += f" [{plan.desc}]"
    left, right = edge_inputs(w, h, d, pairs, 100 * idx)
    in_off = (0, 1, 3)[idx % 3]
    m_off, n_off = (0, 4)[idx % 2], (0, 1, 3)[(idx + 1) % 3]
    gl, gr = guarded_input(left, DEV, in_off, "left"), guarded_input(right, DEV, in_off, "right")
    el = np.stack([oracle.find_all_edges(a, THR, mode) for a in left])
    er = np.stack([oracle.find_all_edges(a, THR, mode) for a in right])
    hot = [oracle.hot_path(el[q], er[q], d, sw, mode) for q in range(pairs)]
    best, web = np.stack([x[0] for x in hot]), np.stack([x[1] for x in hot])
    shp = (pairs, h, w)
    s = stream()

    # sm_find_edges: both edge images
    oel, oer = out(shp, torch.uint8, n_off, maxp, "edges_left"), out(shp, torch.uint8, n_off, maxp, "edges_right")
    bad += twice(f"{tag} sm_find_edges", lambda r: lib.sm_find_edges(plan.h, P(gl.t), P(gr.t), THR, pairs, P(oel.t),
                                                                     P(oer.t), s), [oel, oer], [gl, gr])
    bad += expect(f"{tag} sm_find_edges", oel, el) + expect(f"{tag} sm_find_edges", oer, er)
    # sm_match_wta (edges of sm_find_edges) and the typed maps
    ow, ob = out(shp, torch.int32, m_off, maxp, "web"), out(shp, torch.int32, m_off, maxp, "best")
    bad += twice(f"{tag} sm_match_wta", lambda r: lib.sm_match_wta(plan.h, pairs, P(ow.t), P(ob.t), s), [ow, ob])
    bad += expect(f"{tag} sm_match_wta", ow, web) + expect(f"{tag} sm_match_wta", ob, best)
    types = [capi.SM_WEB_I32, capi.SM_WEB_U16] + ([capi.SM_WEB_U8] if d <= 255 else [])
    capi.check(lib.sm_plan_reserve_narrow(plan.h))
    for ty in types:
        dt, size = NARROW[ty]
        off = m_off if size == 4 else (2 if size == 2 else n_off) * (idx % 2)
        tw, tb = out(shp, dt, off, maxp, f"web[{dt}]"), out(shp, torch.int32, m_off, maxp, "best")
        bad += twice(f"{tag} sm_match_wta_typed", lambda r: lib.sm_match_wta_typed(plan.h, pairs, P(tw.t), ty, P(tb.t), s),
                     [tw, tb])
        bad += expect(f"{tag} sm_match_wta_typed", tw, web) + expect(f"{tag} sm_match_wta_typed", tb, best)
        tw, tb = out(shp, dt, off, maxp, f"web[{dt}]"), out(shp, torch.int32, 4 - m_off, maxp, "best")
        bad += twice(f"{tag} sm_run_typed", lambda r: lib.sm_run_typed(plan.h, P(gl.t), P(gr.t), THR, pairs, P(tw.t), ty,
                                                                       P(tb.t), s), [tw, tb], [gl, gr])
        bad += expect(f"{tag} sm_run_typed", tw, web) + expect(f"{tag} sm_run_typed", tb, best)
    # sm_run: web only
    ow = out(shp, torch.int32, 4 - m_off, maxp, "web")
    bad += twice(f"{tag} sm_run", lambda r: lib.sm_run(plan.h, P(gl.t), P(gr.t), THR, pairs, P(ow.t), P(None), s), [ow],
                 [gl, gr])
    bad += expect(f"{tag} sm_run", ow, web)
    # sm_load_edges of other edge images: the inputs stay unchanged, the match follows them
    rng = np.random.default_rng(idx)
    le2, re2 = ((rng.random((2,) + shp) < 0.4).astype(np.uint8))
    gle, gre = guarded_input(le2, DEV, n_off, "left_edges"), guarded_input(re2, DEV, n_off, "right_edges")
    capi.check(lib.sm_load_edges(plan.h, P(gle.t), P(gre.t), pairs, s))
    torch.cuda.synchronize()
    bad += [f"{tag} sm_load_edges: {p}" for p in gle.problems() + gre.problems()]
    hot2 = [oracle.hot_path(le2[q], re2[q], d, sw, mode) for q in range(pairs)]
    ow, ob = out(shp, torch.int32, m_off, maxp, "web"), out(shp, torch.int32, m_off, maxp, "best")
    bad += twice(f"{tag} sm_load_edges + sm_match_wta", lambda r: lib.sm_match_wta(plan.h, pairs, P(ow.t), P(ob.t), s),
                 [ow, ob], [gle, gre])
    bad += expect(f"{tag} sm_load_edges + sm_match_wta", ow, np.stack([x[1] for x in hot2]))
    bad += expect(f"{tag} sm_load_edges + sm_match_wta", ob, np.stack([x[0] for x in hot2]))
    plan.close()
    return bad


@pytest.mark.parametrize("mode", MODES)
def test_edge_matcher_writes_its_maps_and_nothing_else(mode):
    """sm_find_edges, sm_load_edges, sm_match_wta(_typed), sm_run(_typed) on every built bit-sliced kernel x lane merge,
    the kernel choices of the right-reference tests, the popcount kernels A / B / C and the generic kernel"""
    bad = []
    for idx, case in enumerate(edge_cases(mode)):
        bad += check_edge_case(mode, case, idx)
    report(bad)


@pytest.mark.parametrize("mode", MODES)
def test_lanes_of_run_after_and_pipelined_runs(mode):
    """sm_run_after on a plan that takes its lanes, and sm_run on a pipelined plan: int32 and narrow maps"""
    bad = []
    for idx, (w, h, d, sw, opts) in enumerate([(33, 20, 30, 5, None), (130, 17, 64, 9, dict(kernel_family=1)),
                                                (257, 23, 100, 7, None), (64, 9, 16, 3, dict(edge_kernel=1))]):
        pairs, maxp = (2, 3) if idx % 2 else (1, 1)
        plan = Plan(w, h, d, sw, mode, maxp, opts)
        tag = f"{mode} W={w} H={h} D={d} S={sw} pairs={pairs}/{maxp} [{plan.desc}]"
        left, right = edge_inputs(w, h, d, pairs, 7 * idx)
        gl, gr = guarded_input(left, DEV, idx % 2, "left"), guarded_input(right, DEV, 0, "right")
        hot = [oracle.hot_path(oracle.find_all_edges(left[q], THR, mode), oracle.find_all_edges(right[q], THR, mode),
                               d, sw, mode) for q in range(pairs)]
        best, web = np.stack([x[0] for x in hot]), np.stack([x[1] for x in hot])
        shp = (pairs, h, w)
        capi.check(lib.sm_plan_prepare_threshold(plan.h, THR, stream()))
        capi.check(lib.sm_plan_reserve_narrow(plan.h))
        for ty in (capi.SM_WEB_I32, capi.SM_WEB_U16, capi.SM_WEB_U8):
            dt, size = NARROW[ty]
            tw = out(shp, dt, (4, 2, 3)[ty] if idx % 2 else 0, maxp, f"web[{dt}]")
            tb = out(shp, torch.int32, 4 * (idx % 2), maxp, "best")
            bad += twice(f"{tag} sm_run_after", lambda r: lib.sm_run_after(plan.h, P(gl.t), P(gr.t), THR, pairs, P(tw.t),
                                                                           ty, P(tb.t), stream(), None), [tw, tb], [gl, gr])
            bad += expect(f"{tag} sm_run_after", tw, web) + expect(f"{tag} sm_run_after", tb, best)
        capi.check(lib.sm_plan_set_pipelined(plan.h, 1))
        for ty in (capi.SM_WEB_I32, capi.SM_WEB_U8):
            dt, size = NARROW[ty]
            tw = out(shp, dt, (4, 2, 1)[ty] * (idx % 2), maxp, f"web[{dt}]")
            tb = out(shp, torch.int32, 0, maxp, "best")
            bad += twice(f"{tag} pipelined sm_run_typed",
                         lambda r: lib.sm_run_typed(plan.h, P(gl.t), P(gr.t), THR, pairs, P(tw.t), ty, P(tb.t), stream()),
                         [tw, tb], [gl, gr])
            bad += expect(f"{tag} pipelined sm_run_typed", tw, web) + expect(f"{tag} pipelined sm_run_typed", tb, best)
        ow = out(shp, torch.int32, 4, maxp, "web")
        bad += twice(f"{tag} pipelined sm_run", lambda r: lib.sm_run(plan.h, P(gl.t), P(gr.t), THR, pairs, P(ow.t),
                                                                     P(None), stream()), [ow], [gl, gr])
        bad += expect(f"{tag} pipelined sm_run", ow, web)
        plan.close()
    report(bad)


# ---------------------------------------------------------------------------
# left-right check of the edge matcher
# ---------------------------------------------------------------------------

def lr_cases():
    cases = []
    for j, opts in enumerate(KERNEL_CHOICES):
        for k, w in enumerate(WIDTHS):
            if (j + k) % 2:
                continue
            sw = min(w, (3, 5, 7, 9, 11)[k % 5])
            cases.append((opts, w, 9 + k, (16, 30, 64, 130)[(j + k) % 4], sw))
    for fam, windows in POPCOUNT.items():
        for k, sw in enumerate(windows[:3]):
            cases.append((dict(kernel_family=1), (33, 65, 130)[k], max(sw, 1) + 3, 40, sw))
    cases.append((None, 33, 29, 30, 27))
    return cases


@pytest.mark.parametrize("mode", MODES)
def test_lr_check_writes_its_maps_and_nothing_else(mode):
    """sm_run_lr (web, best, web_right, rejected), sm_match_wta_right, sm_lr_check into a separate map and in place"""
    bad = []
    for idx, (opts, w, h, d, sw) in enumerate(lr_cases()):
        pairs, maxp = (1, 1) if idx % 3 == 2 else (2, 3)
        plan = Plan(w, h, d, sw, mode, maxp, opts)
        tag = f"{mode} W={w} H={h} D={d} S={sw} pairs={pairs}/{maxp} {opts or 'default'} [{plan.desc}]"
        left, right = edge_inputs(w, h, d, pairs, 31 * idx)
        md = (0, 1, 3)[idx % 3]
        want = []
        for q in range(pairs):
            el, er = oracle.find_all_edges(left[q], THR, mode), oracle.find_all_edges(right[q], THR, mode)
            best, web = oracle.hot_path(el, er, d, sw, mode)
            best_r, web_r = lr.right_reference(el, er, d, sw, mode)
            want.append((best, web, best_r, web_r) + lr.lr_check(web, web_r, md, mode))
        W = lambda k: np.stack([x[k] for x in want])     # noqa: E731
        shp, off = (pairs, h, w), 4 * (idx % 2)
        gl, gr = guarded_input(left, DEV, idx % 2, "left"), guarded_input(right, DEV, 3 * (idx % 2), "right")
        ow, ob, owr = (out(shp, torch.int32, off, maxp, n) for n in ("web", "best", "web_right"))
        orj = out((pairs,), torch.int32, 0, maxp, "rejected")
        s = stream()
        t = f"{tag} sm_run_lr"
        bad += twice(t, lambda r: lib.sm_run_lr(plan.h, P(gl.t), P(gr.t), THR, pairs, md, P(ow.t), P(ob.t), P(owr.t),
                                                P(orj.t), s), [ow, ob, owr, orj], [gl, gr])
        bad += expect(t, ow, W(4)) + expect(t, ob, W(0)) + expect(t, owr, W(3)) + expect(t, orj, W(5))
        t = f"{tag} sm_match_wta_right"
        owr, obr = out(shp, torch.int32, 4 - off, maxp, "web_right"), out(shp, torch.int32, off, maxp, "best_right")
        bad += twice(t, lambda r: lib.sm_match_wta_right(plan.h, pairs, P(owr.t), P(obr.t), s), [owr, obr])
        bad += expect(t, owr, W(3)) + expect(t, obr, W(2))
        t = f"{tag} sm_lr_check"
        gw, gwr = guarded_input(W(1), DEV, off, "web"), guarded_input(W(3), DEV, 4 - off, "web_right")
        oo = out(shp, torch.int32, 4 - off, maxp, "out")
        bad += twice(t, lambda r: lib.sm_lr_check(plan.h, P(gw.t), P(gwr.t), md, pairs, P(oo.t), P(orj.t), s),
                     [oo, orj], [gw, gwr])
        bad += expect(t, oo, W(4)) + expect(t, orj, W(5))
        t = f"{tag} sm_lr_check in place"
        io = out(shp, torch.int32, off, maxp, "web (in place)")

        def in_place(run):
            io.t.copy_(torch.from_numpy(W(1)).to(DEV))
            return lib.sm_lr_check(plan.h, P(io.t), P(gwr.t), md, pairs, P(io.t), P(orj.t), s)
        bad += twice(t, in_place, [io, orj], [gwr], partial=(io,))
        bad += expect(t, io, W(4)) + expect(t, orj, W(5))
        plan.close()
    report(bad)


# ---------------------------------------------------------------------------
# the SAD / SSD cost mode
# ---------------------------------------------------------------------------

EXTRA_COST_SHAPES = [(1, 6, 3, 1), (3, 7, 9, 3), (31, 19, 30, 5), (33, 21, 40, 11), (65, 17, 30, 7), (257, 23, 64, 9),
                     (128, 19, 33, 13)]
_cost_cache = {}


def cost_expected(left, right, d, sw, mode, cost, md):
    """clr.expected(), the two cost maps of a pair computed once for every kernel choice and max_diff"""
    key = (left.tobytes(), right.tobytes(), d, sw, mode, cost)
    if key not in _cost_cache:
        best, web = oracle.cost_hot_path(left, right, d, sw, mode, cost)
        _cost_cache[key] = dict(best=best, web=web, **dict(zip(("best_right", "web_right"),
                                                               clr.right_reference(left, right, d, sw, mode, cost))))
    want = dict(_cost_cache[key])
    want["checked"], want["rejected"] = lr.lr_check(want["web"], want["web_right"], md, mode)
    return want


def cost_cases():
    cases = [(opts, shape) for shape in COST_SHAPES for opts in COST_CHOICES + [dict(cost_tile_h=3)]]
    cases += [(opts, shape) for shape in EXTRA_COST_SHAPES for opts in (None, dict(cost_kernel=1), dict(cost_tile_h=3))]
    return cases


@pytest.mark.parametrize("cost", ["sad", "ssd"])
@pytest.mark.parametrize("mode", MODES)
def test_cost_mode_writes_its_maps_and_nothing_else(mode, cost):
    """sm_cost_wta (every map at offset 0 and 4), sm_cost_wta_right, sm_cost_lr (all four outputs), sm_cost_refine
    (sub and costs, with pixels whose web is outside 1..D) on COST_CHOICES x COST_SHAPES: k_sad_pc, k_sad_qs,
    k_ssd_mfma, k_cost_strip behind them (ghost) and the general kernel, tiles of 3 rows"""
    bad = []
    cv = COSTS[cost]
    for idx, (opts, (w, h, d, sw)) in enumerate(cost_cases()):
        pairs, maxp = (1, 1) if idx % 4 == 3 else (2, 3)
        plan = Plan(w, h, d, sw, mode, maxp, opts)
        tag = f"{mode} {cost} W={w} H={h} D={d} S={sw} pairs={pairs}/{maxp} {opts or 'default'}"
        imgs = [make_pair(w, h, d, seed=w + d + q, kind="noise" if q % 2 else "scene") for q in range(pairs)]
        left, right = np.stack([a for a, _ in imgs]), np.stack([b for _, b in imgs])
        md = idx % 3
        want = [cost_expected(left[q], right[q], d, sw, mode, cost, md) for q in range(pairs)]
        W = lambda k: np.stack([x[k] for x in want])     # noqa: E731
        shp, s = (pairs, h, w), stream()
        gl, gr = guarded_input(left, DEV, idx % 2, "left"), guarded_input(right, DEV, 0, "right")
        for off in (0, 4):
            t = f"{tag} sm_cost_wta offset {off}"
            ow, ob = out(shp, torch.int32, off, maxp, "web"), out(shp, torch.int32, off, maxp, "best")
            bad += twice(t, lambda r: lib.sm_cost_wta(plan.h, P(gl.t), P(gr.t), cv, pairs, P(ow.t), P(ob.t), s),
                         [ow, ob], [gl, gr])
            bad += expect(t, ow, W("web")) + expect(t, ob, W("best"))
        off = 4 * (idx % 2)
        capi.check(lib.sm_plan_reserve_cost_lr(plan.h))
        t = f"{tag} sm_cost_wta_right"
        owr, obr = out(shp, torch.int32, off, maxp, "web_right"), out(shp, torch.int32, 4 - off, maxp, "best_right")
        bad += twice(t, lambda r: lib.sm_cost_wta_right(plan.h, P(gl.t), P(gr.t), cv, pairs, P(owr.t), P(obr.t), s),
                     [owr, obr], [gl, gr])
        bad += expect(t, owr, W("web_right")) + expect(t, obr, W("best_right"))
        t = f"{tag} sm_cost_lr"
        ow, ob, owr = (out(shp, torch.int32, o, maxp, n) for o, n in ((off, "web"), (4 - off, "best"), (off, "web_right")))
        orj = out((pairs,), torch.int32, 0, maxp, "rejected")
        bad += twice(t, lambda r: lib.sm_cost_lr(plan.h, P(gl.t), P(gr.t), cv, pairs, md, P(ow.t), P(ob.t), P(owr.t),
                                                 P(orj.t), s), [ow, ob, owr, orj], [gl, gr])
        bad += expect(t, ow, W("checked")) + expect(t, ob, W("best")) + expect(t, owr, W("web_right"))
        bad += expect(t, orj, W("rejected"))
        # sm_cost_refine on the checked map (0 = rejected) with a few values outside 1..D besides
        if opts is None:                # (k_cost_refine takes none of the cost kernels' options)
            web_in = W("checked").copy()
            web_in.reshape(-1)[::7] = d + 1
            web_in.reshape(-1)[3::11] = -3
            ref = [sr.refine(left[q], right[q], web_in[q], d, sw, mode, cost) for q in range(pairs)]
            t = f"{tag} sm_cost_refine"
            gw = guarded_input(web_in, DEV, off, "web")
            osub = out(shp, torch.int16, 2 * (idx % 4 == 0), maxp, "sub")
            ocs = out((pairs, 3, h, w), torch.int32, off, maxp, "costs")
            bad += twice(t, lambda r: lib.sm_cost_refine(plan.h, P(gl.t), P(gr.t), cv, pairs, P(gw.t), P(osub.t),
                                                         P(ocs.t), s), [osub, ocs], [gl, gr, gw])
            bad += expect(t, osub, np.stack([x[0] for x in ref])) + expect(t, ocs, np.stack([x[1] for x in ref]))
        plan.close()
    report(bad)


# ---------------------------------------------------------------------------
# step 3
# ---------------------------------------------------------------------------

def step3_maps(pairs, h, w, holes, seed):
    rng = np.random.default_rng(seed)
    web = rng.integers(1, 31, (pairs, h, w)).astype(np.int32)
    web[:, 0, 0], web[:, -1, -1] = 1, 30           # a contour interval of 29 / lines
    if holes:
        web[rng.random((pairs, h, w)) < 0.2] = 0
        web[:, -1, :] = 0                          # a whole last row
        web[:, :, 0] = 0                           # ... and the first column
        web[:, -1, -1] = 30
    return web


@pytest.mark.parametrize("holes", [False, True])
def test_step3_writes_its_maps_and_nothing_else(holes):
    """sm_fill_web_holes (times 0, 1, 2: only the buffer *result_in_tmp names must be written), sm_min_max,
    sm_draw_contour_map, and sm_step3 on its speculative (no holes) and staged (holes) routes"""
    bad = []
    for idx, w in enumerate(WIDTHS):
        h = (5, 17, 40)[idx % 3]
        pairs, maxp = (1, 1) if idx % 3 == 2 else (2, 3)
        plan = Plan(w, h, 30, min(3, w), "toroidal", maxp)
        tag = f"W={w} H={h} pairs={pairs}/{maxp} holes={holes}"
        web = step3_maps(pairs, h, w, holes, idx)
        shp, off, s = (pairs, h, w), 4 * (idx % 2), stream()
        lines = (4, 10)[idx % 2]
        for times in (0, 1, 2):
            t = f"{tag} sm_fill_web_holes times={times}"
            iw, tmp = out(shp, torch.int32, off, maxp, "web"), out(shp, torch.int32, 4 - off, maxp, "tmp")
            which = C.c_int(-1)

            def fill(run):
                iw.t.copy_(torch.from_numpy(web).to(DEV))
                return lib.sm_fill_web_holes(plan.h, P(iw.t), P(tmp.t), times, pairs, C.byref(which), s)
            bad += twice(t, fill, [iw, tmp], partial=(iw, tmp))
            filled = np.stack([oracle.fill_web_holes(web[q], times) for q in range(pairs)])
            res = tmp if which.value else iw
            if which.value:             # the named buffer must be written in full
                bad += [f"{t}: {p}" for p in tmp.unwritten()]
            bad += expect(t, res, filled)
        filled = np.stack([oracle.fill_web_holes(web[q], 32) for q in range(pairs)])
        mm = np.stack([[f.min(), f.max()] for f in filled]).astype(np.int32)
        contour = np.stack([oracle.draw_contour_map(f, lines) for f in filled])
        gf = guarded_input(filled, DEV, off, "web")
        t = f"{tag} sm_min_max"
        omm = out((pairs, 2), torch.int32, 4 * (idx % 3 == 1), maxp, "minmax")
        bad += twice(t, lambda r: lib.sm_min_max(plan.h, P(gf.t), pairs, P(omm.t), s), [omm], [gf])
        bad += expect(t, omm, mm)
        t = f"{tag} sm_draw_contour_map"
        gmm = guarded_input(mm, DEV, 0, "minmax")
        oc = out(shp, torch.uint8, (0, 1, 3)[idx % 3], maxp, "contour")
        bad += twice(t, lambda r: lib.sm_draw_contour_map(plan.h, P(gf.t), P(gmm.t), lines, pairs, P(oc.t), s), [oc],
                     [gf, gmm])
        capi.check(lib.sm_plan_status(plan.h, s))
        bad += expect(t, oc, contour)
        t = f"{tag} sm_step3 ({'staged' if holes else 'speculative'} route)"
        iw, tmp = out(shp, torch.int32, off, maxp, "web"), out(shp, torch.int32, 4 - off, maxp, "tmp")
        omm = out((pairs, 2), torch.int32, 0, maxp, "minmax")
        oc = out(shp, torch.uint8, (0, 1, 3)[idx % 3], maxp, "contour")
        which = C.c_int(-1)

        def step3(run):
            iw.t.copy_(torch.from_numpy(web).to(DEV))
            return lib.sm_step3(plan.h, P(iw.t), P(tmp.t), 32, lines, pairs, P(omm.t), P(oc.t), C.byref(which), s)
        bad += twice(t, step3, [iw, tmp, omm, oc], partial=(iw, tmp))
        if which.value:
            bad += [f"{t}: {p}" for p in tmp.unwritten()]
        bad += expect(t, tmp if which.value else iw, filled) + expect(t, omm, mm) + expect(t, oc, contour)
        plan.close()
    report(bad)


# ---------------------------------------------------------------------------
# debug taps
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_debug_taps_write_their_planes_and_nothing_else(mode):
    """sm_debug_planes (all three planes of one pair and shift), sm_debug_edge_table and sm_debug_edge_table_fast
    (766 x 766 bytes each)"""
    bad = []
    for idx, (w, h, d, sw) in enumerate([(33, 11, 30, 5), (130, 9, 16, 9), (1, 4, 3, 1), (257, 7, 40, 3)]):
        plan = Plan(w, h, d, sw, mode, 3)
        tag = f"{mode} W={w} H={h} D={d} S={sw}"
        rng = np.random.default_rng(idx)
        le, re = (rng.random((2, 2, h, w)) < 0.5).astype(np.uint8)
        gle, gre = guarded_input(le, DEV, 1, "left_edges"), guarded_input(re, DEV, 0, "right_edges")
        capi.check(lib.sm_load_edges(plan.h, P(gle.t), P(gre.t), 2, stream()))
        for shift in (0, d // 2, d - 1):
            t = f"{tag} sm_debug_planes pair 1 shift {shift}"
            m = guarded((h, w), torch.uint8, DEV, offset=idx % 2 * 3, name="matches")
            sa = guarded((h, w), torch.int32, DEV, offset=4 * (idx % 2), name="score_all")
            sc = guarded((h, w), torch.int32, DEV, offset=4 * (1 - idx % 2), name="scores")
            bad += twice(t, lambda r: lib.sm_debug_planes(plan.h, 1, shift, P(m.t), P(sa.t), P(sc.t), stream()),
                         [m, sa, sc], [gle, gre])
            mp = oracle.match_plane(le[1], re[1], shift, mode)
            total = oracle.addup(mp, sw, mode)
            bad += expect(t, m, mp) + expect(t, sa, total) + expect(t, sc, oracle.record_score(mp, total))
        plan.close()
    plan = Plan(64, 16, 30, 3, mode, 1)
    for thr in (0.15, 0.4):
        want = oracle.edge_table(thr)
        t = f"{mode} sm_debug_edge_table threshold {thr}"
        tb = guarded((766, 766), torch.uint8, DEV, offset=(0, 1)[thr > 0.2], name="table")
        bad += twice(t, lambda r: lib.sm_debug_edge_table(0, thr, P(tb.t), stream()), [tb])
        bad += expect(t, tb, want)
        t = f"{mode} sm_debug_edge_table_fast threshold {thr}"
        flag = C.c_int(-1)
        tb = guarded((766, 766), torch.uint8, DEV, offset=(3, 0)[thr > 0.2], name="table")
        bad += twice(t, lambda r: lib.sm_debug_edge_table_fast(plan.h, thr, P(tb.t), C.byref(flag), stream()), [tb])
        bad += expect(t, tb, want)
    plan.close()
    report(bad)


# ---------------------------------------------------------------------------
# graph replay: caller-owned guarded maps, refilled with the other poison between replays
# ---------------------------------------------------------------------------

def replayed(tag, graph, outs, partial=()):
    bad = []
    for rep, run in enumerate((1, 0, 1)):
        for g in outs:
            g.fill(run)
        graph.replay()
        torch.cuda.synchronize()
        for g in outs:
            bad += [f"{tag} replay {rep}: {p}" for p in g.problems() if not (g in partial and "not written" in p)]
        if rep == 0:
            for g in outs:
                g.owned.pop(0, None)      # (the first replay compares with the second, not with the capture run)
    return bad


def capture(fn):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        capi.check(fn())
    return g


@pytest.mark.parametrize("mode", MODES)
def test_graph_replays_write_their_maps_and_nothing_else(mode):
    """sm_run (plain and pipelined), sm_cost_wta followed by sm_cost_refine, sm_run_lr and sm_cost_lr captured after
    the reserve / prepare calls, on caller-owned guarded maps; every replay refilled with the other poison (the class
    of the rejection counts that a replay left as they were)"""
    bad = []
    w, h, d, sw, pairs, maxp = 65, 19, 30, 5, 2, 3
    left, right = edge_inputs(w, h, d, pairs, 5)
    gl, gr = guarded_input(left, DEV, 1, "left"), guarded_input(right, DEV, 0, "right")
    shp = (pairs, h, w)
    want = []
    for q in range(pairs):
        el, er = oracle.find_all_edges(left[q], THR, mode), oracle.find_all_edges(right[q], THR, mode)
        best, web = oracle.hot_path(el, er, d, sw, mode)
        best_r, web_r = lr.right_reference(el, er, d, sw, mode)
        want.append(dict(web=web, best=best, web_right=web_r) | dict(zip(("checked", "rejected"),
                                                                            lr.lr_check(web, web_r, 1, mode))))
    W = lambda k: np.stack([x[k] for x in want])     # noqa: E731
    for pipelined in (0, 1):
        plan = Plan(w, h, d, sw, mode, maxp)
        capi.check(lib.sm_plan_prepare_threshold(plan.h, THR, stream()))
        capi.check(lib.sm_plan_reserve_lr(plan.h))
        capi.check(lib.sm_plan_set_pipelined(plan.h, pipelined))
        torch.cuda.synchronize()
        tag = f"{mode} graph of sm_run (pipelined={pipelined})"
        ow, ob = out(shp, torch.int32, 4, maxp, "web"), out(shp, torch.int32, 0, maxp, "best")
        g = capture(lambda: lib.sm_run(plan.h, P(gl.t), P(gr.t), THR, pairs, P(ow.t), P(ob.t), stream()))
        bad += replayed(tag, g, [ow, ob]) + expect(tag, ow, W("web")) + expect(tag, ob, W("best"))
        if not pipelined:
            tag = f"{mode} graph of sm_run_lr"
            ow, ob, owr = (out(shp, torch.int32, o, maxp, n) for o, n in ((0, "web"), (4, "best"), (4, "web_right")))
            orj = out((pairs,), torch.int32, 0, maxp, "rejected")
            g = capture(lambda: lib.sm_run_lr(plan.h, P(gl.t), P(gr.t), THR, pairs, 1, P(ow.t), P(ob.t), P(owr.t),
                                              P(orj.t), stream()))
            bad += replayed(tag, g, [ow, ob, owr, orj])
            bad += expect(tag, ow, W("checked")) + expect(tag, ob, W("best")) + expect(tag, owr, W("web_right"))
            bad += expect(tag, orj, W("rejected"))
        torch.cuda.synchronize()
        plan.close()
    for cost in ("sad", "ssd"):
        cw, ch, cd, csw = 97, 23, 40, 7
        imgs = [make_pair(cw, ch, cd, seed=11 + q) for q in range(pairs)]
        cl, cr = np.stack([a for a, _ in imgs]), np.stack([b for _, b in imgs])
        cwant = [cost_expected(cl[q], cr[q], cd, csw, mode, cost, 1) for q in range(pairs)]
        CW = lambda k: np.stack([x[k] for x in cwant])     # noqa: E731
        ref = [sr.refine(cl[q], cr[q], cwant[q]["web"], cd, csw, mode, cost) for q in range(pairs)]
        gcl, gcr = guarded_input(cl, DEV, 3, "left"), guarded_input(cr, DEV, 0, "right")
        plan = Plan(cw, ch, cd, csw, mode, maxp)
        capi.check(lib.sm_plan_reserve_cost_lr(plan.h))
        torch.cuda.synchronize()
        cshp, cv = (pairs, ch, cw), COSTS[cost]
        tag = f"{mode} {cost} graph of sm_cost_wta + sm_cost_refine"
        ow, ob = out(cshp, torch.int32, 4, maxp, "web"), out(cshp, torch.int32, 4, maxp, "best")
        osub, ocs = out(cshp, torch.int16, 2, maxp, "sub"), out((pairs, 3, ch, cw), torch.int32, 4, maxp, "costs")

        def both():
            rc = lib.sm_cost_wta(plan.h, P(gcl.t), P(gcr.t), cv, pairs, P(ow.t), P(ob.t), stream())
            return rc or lib.sm_cost_refine(plan.h, P(gcl.t), P(gcr.t), cv, pairs, P(ow.t), P(osub.t), P(ocs.t),
                                            stream())
        g = capture(both)
        bad += replayed(tag, g, [ow, ob, osub, ocs])
        bad += expect(tag, ow, CW("web")) + expect(tag, ob, CW("best"))
        bad += expect(tag, osub, np.stack([x[0] for x in ref])) + expect(tag, ocs, np.stack([x[1] for x in ref]))
        tag = f"{mode} {cost} graph of sm_cost_lr"
        ow, ob, owr = (out(cshp, torch.int32, o, maxp, n) for o, n in ((4, "web"), (0, "best"), (4, "web_right")))
        orj = out((pairs,), torch.int32, 0, maxp, "rejected")
        g = capture(lambda: lib.sm_cost_lr(plan.h, P(gcl.t), P(gcr.t), cv, pairs, 1, P(ow.t), P(ob.t), P(owr.t),
                                           P(orj.t), stream()))
        bad += replayed(tag, g, [ow, ob, owr, orj])
        bad += expect(tag, ow, CW("checked")) + expect(tag, ob, CW("best")) + expect(tag, owr, CW("web_right"))
        bad += expect(tag, orj, CW("rejected"))
        bad += [f"{tag}: {p}" for p in gcl.problems() + gcr.problems()]
        torch.cuda.synchronize()
        plan.close()
    bad += [f"{mode} graphs: {p}" for p in gl.problems() + gr.problems()]
    report(bad)
