"""No stage depends on what its workspace held before the call.

The plan's lazily allocated workspaces (sm_api.hip's table) are not cleared between calls, and all but one are not
cleared when they are allocated: a kernel that reads such a word must have written it in the same call.  The other GPU
modules build a fresh plan per case, whose first allocation is very often zero pages, so a forgotten clear of a count, a
carry, a label size or a border entry passes them.  Here sm_debug_poison_workspace fills the workspaces with each word of
workspace_poison_cases.WORDS in turn, the stage runs (a batch of one pair, the full batch, and a batch of one again with
the other pairs' residue behind it), and every output map, count and total must be bit-identical to the CPU definition.
The outputs sit in guarded buffers (tests/guarded.py), so a stray store shows too.  All comparisons are exact.

The assertion comes after each word: a harsher word never runs once a milder one has shown a difference."""
import math

import numpy as np
import pytest
import torch

from stereomatching_amd import capi
from stereomatching_amd.capi import lib
from tests import filter_reference as fr
from tests import interp_reference as ir
from tests import workspace_poison_cases as wc
from tests.guarded import POISON
from tests.test_write_bounds_gpu import P, Plan, expect, out, report, stream

pytestmark = pytest.mark.gpu
MAXP = wc.MAXP
I32, I16, U8, U16 = torch.int32, torch.int16, torch.uint8, torch.uint16
TORCH = {np.int32: I32, np.int16: I16}
TYPE = {np.int32: capi.SM_MAP_I32, np.int16: capi.SM_MAP_I16}
COSTS = {"sad": 1, "ssd": 2}
INF = math.inf


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()             # (a copy: the cases' arrays are read-only)


def go(tag, run, fn, outs_wants):
    """fill every guarded output with the poison of `run`, call, and compare: guards intact, values the definition's"""
    for g, _ in outs_wants:
        g.fill(run)
    rc = fn()
    if rc != capi.SM_OK:
        return [f"{tag}: returned {rc}: {lib.sm_last_error().decode(errors='replace')}"]
    torch.cuda.synchronize()
    bad = []
    for g, want in outs_wants:
        bad += [f"{tag}: {p}" for p in g._guard_problems(run)]
        bad += expect(tag, g, want)
    return bad


def drive(tag, plan, reserve, stage):
    """stage(pairs, run) -> problems.  A fresh plan first; then the reservation, and per word: poison, a batch of one,
    the full batch, a batch of one; the assertion after each word."""
    try:
        report([f"{tag} fresh plan: {p}" for p in stage(MAXP, 0)])
        capi.check(reserve(plan.h))
        for i, word in enumerate(wc.WORDS):
            capi.check(lib.sm_debug_poison_workspace(plan.h, word))
            bad = []
            for k, pairs in enumerate((1, MAXP, 1)):
                bad += [f"{tag} poison {word:#010x} call {k}: {p}" for p in stage(pairs, (i + k + 1) % 2)]
            report(bad)
    finally:
        torch.cuda.synchronize()
        plan.close()


def maps(pairs, h, w, names, dtype=I32, off=0):
    return [out((pairs, h, w), dtype, off, MAXP, n) for n in names]


def counts(pairs, name):
    return out((pairs,), I32, 0, MAXP, name)


# ---------------------------------------------------------------------------
# the entry point itself
# ---------------------------------------------------------------------------

def test_poison_allocates_nothing_and_refuses_no_plan(hip):
    assert lib.sm_debug_poison_workspace(None, 1) == capi.SM_ERR_ARG
    assert b"sm_debug_poison_workspace: plan is NULL" in lib.sm_last_error()
    w, h, d, sw = 129, 33, 16, 3
    plan = hip.StereoPlan(w, h, d, sw, "toroidal", max_pairs=2)
    try:
        base = plan.workspace_bytes()
        plan._poison_workspace(0xA5A5A5A5)                          # nothing allocated: nothing to fill
        assert plan.workspace_bytes() == base
        plan.reserve_filter()
        reserved = plan.workspace_bytes()
        plan._poison_workspace(0xFFFFFFFF)
        assert plan.workspace_bytes() == reserved
        # the plan's permanent buffers are not the workspace's: a plain run after the poison is the definition's
        left, right = wc.images(w, h, d, 2)
        want = wc.edge_expected("toroidal", w, h, d, sw, 1, pairs=2)
        web, _ = plan.run(dev(left), dev(right), wc.THR)
        assert np.array_equal(web.cpu().numpy(), want["web"])
    finally:
        plan.close()


# ---------------------------------------------------------------------------
# NARROW: the int32 staging map of narrow results
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", wc.MODES)
def test_narrow_maps_of_a_poisoned_staging_map(mode):
    """sm_run_typed with a u8 and a u16 web on a plan of the tiled popcount family (it has no narrow store path)"""
    for w, h, d, sw in wc.IMAGE_CASES[mode]:
        plan = Plan(w, h, d, sw, mode, MAXP, dict(kernel_family=1))
        base = lib.sm_plan_workspace_bytes(plan.h)
        left, right = (dev(a) for a in wc.images(w, h, d))
        want = wc.edge_expected(mode, w, h, d, sw, 1)

        def stage(pairs, run):
            bad = []
            for ty, dt in ((capi.SM_WEB_U8, U8), (capi.SM_WEB_U16, U16)):
                tw, = maps(pairs, h, w, [f"web[{dt}]"], dt)
                tb, = maps(pairs, h, w, ["best"])
                bad += go(f"sm_run_typed {dt} pairs {pairs}", run,
                          lambda: lib.sm_run_typed(plan.h, P(left), P(right), wc.THR, pairs, P(tw.t), ty, P(tb.t), stream()),
                          [(tw, want["web"][:pairs]), (tb, want["best"][:pairs])])
            return bad

        def reserve(handle):
            rc = lib.sm_plan_reserve_narrow(handle)
            # (the plan does stage its narrow maps: a bit-sliced plan would have no such row to poison)
            assert lib.sm_plan_workspace_bytes(handle) == base + MAXP * w * h * 4, plan.desc
            return rc
        drive(f"{mode} {w}x{h} D={d} S={sw} [{plan.desc}]", plan, reserve, stage)


# ---------------------------------------------------------------------------
# EXT_LR, WEB_LR: the edge matcher's consistency check
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", wc.MODES)
def test_edge_lr_check_of_a_poisoned_workspace(mode):
    """sm_run_lr (with and without the caller's right map), then sm_match_wta_right + sm_lr_check"""
    md = 1
    for w, h, d, sw in wc.IMAGE_CASES[mode]:
        plan = Plan(w, h, d, sw, mode, MAXP)
        left, right = (dev(a) for a in wc.images(w, h, d))
        want = wc.edge_expected(mode, w, h, d, sw, md)

        def stage(pairs, run):
            W = lambda k: want[k][:pairs]     # noqa: E731
            s = stream()
            ow, ob, owr = maps(pairs, h, w, ["web", "best", "web_right"])
            orj = counts(pairs, "rejected")
            bad = go(f"sm_run_lr pairs {pairs}", run,
                     lambda: lib.sm_run_lr(plan.h, P(left), P(right), wc.THR, pairs, md, P(ow.t), P(ob.t), P(owr.t),
                                           P(orj.t), s),
                     [(ow, W("checked")), (ob, W("best")), (owr, W("web_right")), (orj, W("rejected"))])
            bad += go(f"sm_run_lr (web only) pairs {pairs}", run,
                      lambda: lib.sm_run_lr(plan.h, P(left), P(right), wc.THR, pairs, md, P(ow.t), None, None, P(orj.t), s),
                      [(ow, W("checked")), (orj, W("rejected"))])
            obr, = maps(pairs, h, w, ["best_right"])
            bad += go(f"sm_match_wta_right pairs {pairs}", run,
                      lambda: lib.sm_match_wta_right(plan.h, pairs, P(owr.t), P(obr.t), s),
                      [(owr, W("web_right")), (obr, W("best_right"))])
            web_in = dev(W("web"))
            oo, = maps(pairs, h, w, ["out"])
            bad += go(f"sm_lr_check pairs {pairs}", run,
                      lambda: lib.sm_lr_check(plan.h, P(web_in), P(owr.t), md, pairs, P(oo.t), P(orj.t), s),
                      [(oo, W("checked")), (orj, W("rejected"))])
            return bad
        drive(f"{mode} {w}x{h} D={d} S={sw}", plan, lib.sm_plan_reserve_lr, stage)


# ---------------------------------------------------------------------------
# GRAY_LR, WEB_LR: the SAD / SSD cost mode's check
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", wc.MODES)
def test_cost_lr_check_of_a_poisoned_workspace(mode):
    """sm_cost_lr for sad and ssd (with and without the caller's right map) and sm_cost_wta_right"""
    md = 1
    for w, h, d, sw in wc.IMAGE_CASES[mode]:
        plan = Plan(w, h, d, sw, mode, MAXP)
        left, right = (dev(a) for a in wc.images(w, h, d))

        def stage(pairs, run):
            bad, s = [], stream()
            for cost, cv in COSTS.items():
                want = wc.cost_expected(mode, w, h, d, sw, cost, md)
                W = lambda k: want[k][:pairs]     # noqa: E731
                ow, ob, owr = maps(pairs, h, w, ["web", "best", "web_right"])
                orj = counts(pairs, "rejected")
                bad += go(f"sm_cost_lr {cost} pairs {pairs}", run,
                          lambda: lib.sm_cost_lr(plan.h, P(left), P(right), cv, pairs, md, P(ow.t), P(ob.t), P(owr.t),
                                                 P(orj.t), s),
                          [(ow, W("checked")), (ob, W("best")), (owr, W("web_right")), (orj, W("rejected"))])
                bad += go(f"sm_cost_lr {cost} (web only) pairs {pairs}", run,
                          lambda: lib.sm_cost_lr(plan.h, P(left), P(right), cv, pairs, md, P(ow.t), None, None, P(orj.t), s),
                          [(ow, W("checked")), (orj, W("rejected"))])
                obr, = maps(pairs, h, w, ["best_right"])
                bad += go(f"sm_cost_wta_right {cost} pairs {pairs}", run,
                          lambda: lib.sm_cost_wta_right(plan.h, P(left), P(right), cv, pairs, P(owr.t), P(obr.t), s),
                          [(owr, W("web_right")), (obr, W("best_right"))])
            return bad
        drive(f"{mode} {w}x{h} D={d} S={sw}", plan, lib.sm_plan_reserve_cost_lr, stage)


# ---------------------------------------------------------------------------
# CENSUS, WEB_LR: the census mode
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", wc.MODES)
def test_census_mode_of_a_poisoned_workspace(mode):
    """sm_census_wta, _wta_right, _lr (with and without the caller's right map) and _refine at census widths 5 and 7:
    the 4-byte descriptors of width 5 are written over the 8-byte ones of width 7 and the other way round"""
    md = 1
    for w, h, d, sw in wc.IMAGE_CASES[mode]:
        plan = Plan(w, h, d, sw, mode, MAXP)
        left, right = (dev(a) for a in wc.images(w, h, d))

        def stage(pairs, run):
            bad, s = [], stream()
            for cw in (5, 7):
                want = wc.census_expected(mode, w, h, d, sw, cw, md)
                W = lambda k: want[k][:pairs]     # noqa: E731
                t = f"census {cw} pairs {pairs}"
                ow, ob, owr, obr = maps(pairs, h, w, ["web", "best", "web_right", "best_right"])
                orj = counts(pairs, "rejected")
                bad += go(f"sm_census_wta {t}", run,
                          lambda: lib.sm_census_wta(plan.h, P(left), P(right), cw, pairs, P(ow.t), P(ob.t), s),
                          [(ow, W("web")), (ob, W("best"))])
                bad += go(f"sm_census_wta_right {t}", run,
                          lambda: lib.sm_census_wta_right(plan.h, P(left), P(right), cw, pairs, P(owr.t), P(obr.t), s),
                          [(owr, W("web_right")), (obr, W("best_right"))])
                bad += go(f"sm_census_lr {t}", run,
                          lambda: lib.sm_census_lr(plan.h, P(left), P(right), cw, pairs, md, P(ow.t), P(ob.t), P(owr.t),
                                                   P(orj.t), s),
                          [(ow, W("checked")), (ob, W("best")), (owr, W("web_right")), (orj, W("rejected"))])
                bad += go(f"sm_census_lr (web only) {t}", run,
                          lambda: lib.sm_census_lr(plan.h, P(left), P(right), cw, pairs, md, P(ow.t), None, None,
                                                   P(orj.t), s),
                          [(ow, W("checked")), (orj, W("rejected"))])
                web_in = dev(W("web"))
                osub, = maps(pairs, h, w, ["sub"], I16)
                ocs = out((pairs, 3, h, w), I32, 0, MAXP, "costs")
                bad += go(f"sm_census_refine {t}", run,
                          lambda: lib.sm_census_refine(plan.h, P(left), P(right), cw, pairs, P(web_in), P(osub.t),
                                                       P(ocs.t), s),
                          [(osub, W("sub")), (ocs, W("costs"))])
            return bad
        drive(f"{mode} {w}x{h} D={d} S={sw}", plan, lib.sm_plan_reserve_census, stage)


# ---------------------------------------------------------------------------
# SGM (with CENSUS)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", wc.MODES)
def test_sgm_of_a_poisoned_workspace(mode):
    """sm_sgm_wta, _wta_right and _lr with 8 paths (census 7) and 4 paths (census 5) through the same volumes.  With a
    window of 1 (the 66 x 2 case) the aggregate volume is not used for the horizontal sums first: whatever the paths
    find in it is the workspace's residue."""
    md = 1
    for w, h, d, sw in wc.IMAGE_CASES[mode]:
        plan = Plan(w, h, d, sw, mode, MAXP)
        left, right = (dev(a) for a in wc.images(w, h, d))

        def stage(pairs, run):
            bad, s = [], stream()
            for paths, cw, p1, p2 in ((8, 7, 10, 120), (4, 5, 3, 40)):
                want = wc.sgm_expected(mode, w, h, d, sw, cw, p1, p2, paths, md)
                W = lambda k: want[k][:pairs]     # noqa: E731
                t = f"{paths} paths pairs {pairs}"
                ow, ob, owr, obr = maps(pairs, h, w, ["web", "best", "web_right", "best_right"])
                osub, = maps(pairs, h, w, ["sub"], I16)
                orj = counts(pairs, "rejected")
                bad += go(f"sm_sgm_wta {t}", run,
                          lambda: lib.sm_sgm_wta(plan.h, P(left), P(right), cw, p1, p2, paths, pairs, P(ow.t), P(ob.t),
                                                 P(osub.t), s),
                          [(ow, W("web")), (ob, W("best")), (osub, W("sub"))])
                bad += go(f"sm_sgm_wta_right {t}", run,
                          lambda: lib.sm_sgm_wta_right(plan.h, P(left), P(right), cw, p1, p2, paths, pairs, P(owr.t),
                                                       P(obr.t), s),
                          [(owr, W("web_right")), (obr, W("best_right"))])
                bad += go(f"sm_sgm_lr {t}", run,
                          lambda: lib.sm_sgm_lr(plan.h, P(left), P(right), cw, p1, p2, paths, pairs, md, P(ow.t), P(ob.t),
                                                P(owr.t), P(orj.t), P(osub.t), s),
                          [(ow, W("checked")), (ob, W("best")), (owr, W("web_right")), (orj, W("rejected")),
                           (osub, W("sub_checked"))])
                bad += go(f"sm_sgm_lr (web only) {t}", run,
                          lambda: lib.sm_sgm_lr(plan.h, P(left), P(right), cw, p1, p2, paths, pairs, md, P(ow.t), None,
                                                None, P(orj.t), None, s),
                          [(ow, W("checked")), (orj, W("rejected"))])
            return bad
        drive(f"{mode} {w}x{h} D={d} S={sw}", plan, lib.sm_plan_reserve_sgm, stage)


# ---------------------------------------------------------------------------
# FILTER: labels and sizes of the speckle filter
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.int32, np.int16])
def test_speckle_filter_of_a_poisoned_workspace(dtype):
    """sm_speckle_filter with the removed counts, into another map and in place"""
    td, ty = TORCH[dtype], TYPE[dtype]
    max_size, max_diff = wc.SPECKLE
    for w, h in wc.MAP_SIZES:
        plan = Plan(w, h, 4, 1, "ghost", MAXP)
        src, kept, removed = wc.speckle_case(w, h, dtype)
        gin = dev(src)

        def stage(pairs, run):
            s = stream()
            osp, = maps(pairs, h, w, ["out"], td)
            orm = counts(pairs, "removed")
            bad = go(f"sm_speckle_filter pairs {pairs}", run,
                     lambda: lib.sm_speckle_filter(plan.h, P(gin), ty, max_size, max_diff, pairs, P(osp.t), P(orm.t), s),
                     [(osp, kept[:pairs]), (orm, removed[:pairs])])
            oip, = maps(pairs, h, w, ["map (in place)"], td)

            def in_place():
                oip.t.copy_(gin[:pairs])
                return lib.sm_speckle_filter(plan.h, P(oip.t), ty, max_size, max_diff, pairs, P(oip.t), P(orm.t), s)
            bad += go(f"sm_speckle_filter in place pairs {pairs}", run, in_place,
                      [(oip, kept[:pairs]), (orm, removed[:pairs])])
            return bad
        drive(f"{np.dtype(dtype).name} {w}x{h}", plan, lib.sm_plan_reserve_filter, stage)


# ---------------------------------------------------------------------------
# INTERP: directional maps and carries
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.int32, np.int16])
def test_interpolation_of_a_poisoned_workspace(dtype):
    """sm_interpolate with classes and the filled counts, and without either.  Maps with so few valid pixels that whole
    row chunks and line segments hold none: their carries are what the workspace must not supply."""
    td, ty = TORCH[dtype], TYPE[dtype]
    for w, h in wc.INTERP_SIZES:
        plan = Plan(w, h, 4, 1, "ghost", MAXP)
        src, cls, want, filled = wc.interp_case(w, h, dtype)
        plain = np.stack([ir.interpolate(m) for m in src])
        gin, gcls = dev(src), dev(cls)

        def stage(pairs, run):
            s = stream()
            oo, = maps(pairs, h, w, ["out"], td)
            ofl = counts(pairs, "filled")
            bad = go(f"sm_interpolate pairs {pairs}", run,
                     lambda: lib.sm_interpolate(plan.h, P(gin), ty, P(gcls), pairs, P(oo.t), P(ofl.t), s),
                     [(oo, want[:pairs]), (ofl, filled[:pairs])])
            bad += go(f"sm_interpolate (no classes, no count) pairs {pairs}", run,
                      lambda: lib.sm_interpolate(plan.h, P(gin), ty, None, pairs, P(oo.t), None, s), [(oo, plain[:pairs])])
            return bad
        drive(f"{np.dtype(dtype).name} {w}x{h}", plan, lib.sm_plan_reserve_interp, stage)


# ---------------------------------------------------------------------------
# CLOUD: tile counts
# ---------------------------------------------------------------------------

def cloud_call(plan, tag, run, m, ty, q, gate, g, pairs, cap, wants, want_index):
    """one sm_point_cloud into guarded records / index / count: the first min(count, cap) records and indices are the
    definition's, the slots behind them keep the poison, the counts are the totals"""
    lo, hi = (-INF, INF) if gate is None else gate
    pts = out((pairs, cap, 4), I32, 0, MAXP, "points")
    idx = out((pairs, cap), I32, 0, MAXP, "index") if want_index else None
    cnt = counts(pairs, "count")
    for o in (pts, idx, cnt):
        if o is not None:
            o.fill(run)
    rc = lib.sm_point_cloud(plan.h, P(m), ty, capi.q16(q), lo, hi, P(g), pairs, cap, P(pts.t),
                            P(idx.t) if want_index else None, P(cnt.t), stream())
    if rc != capi.SM_OK:
        return [f"{tag}: returned {rc}: {lib.sm_last_error().decode(errors='replace')}"]
    torch.cuda.synchronize()
    bad = expect(tag, cnt, [len(i) for _, i in wants[:pairs]])
    for o in (pts, idx, cnt):
        if o is not None:
            bad += [f"{tag}: {p}" for p in o._guard_problems(run)]
    got_p, got_i = pts.value(), idx.value() if want_index else None
    fill = np.frombuffer(bytes([POISON[run]] * 4), np.int32)[0]
    for p in range(pairs):
        k = min(len(wants[p][1]), cap)
        if not np.array_equal(got_p[p, :k], wants[p][0][:k].view(np.int32)):
            bad.append(f"{tag}: records of pair {p} differ from the definition")
        if not (got_p[p, k:] == fill).all():
            bad.append(f"{tag}: record slots of pair {p} from {k} on were written")
        if want_index and not np.array_equal(got_i[p, :k], wants[p][1][:k]):
            bad.append(f"{tag}: indices of pair {p} differ from the definition")
        if want_index and not (got_i[p, k:] == fill).all():
            bad.append(f"{tag}: index slots of pair {p} from {k} on were written")
    return bad


@pytest.mark.parametrize("dtype", [np.int32, np.int16])
def test_point_cloud_of_a_poisoned_workspace(dtype):
    """sm_point_cloud with and without d_index and d_gray, both z gates, a capacity above every count and one below"""
    ty = TYPE[dtype]
    for w, h in wc.MAP_SIZES:
        plan = Plan(w, h, 4, 1, "ghost", MAXP)

        def stage(pairs, run):
            bad = []
            for gi, with_gray, want_index, below in ((0, True, True, False), (1, False, False, True), (1, True, True, True)):
                m, g, q, wants = wc.cloud_case(w, h, dtype, gi, with_gray)
                most = max(len(i) for _, i in wants[:pairs])
                cap = max(1, most - 3) if below else most + 5
                bad += cloud_call(plan, f"gate {gi} gray {with_gray} index {want_index} capacity {cap} pairs {pairs}", run,
                                  dev(m), ty, q, wc.Z_GATES[gi], dev(g) if with_gray else None, pairs, cap, wants, want_index)
            return bad
        drive(f"{np.dtype(dtype).name} {w}x{h}", plan, lib.sm_plan_reserve_cloud, stage)


def test_point_cloud_with_more_tiles_than_the_scan_has_lanes():
    """640 x 420 = 263 tiles: k_cloud_scan takes a second turn and carries the first turn's sum into it.  Two pairs, one
    map in which every pixel is kept and one in which none is, then the two the other way round in the same slots."""
    w, h = wc.CLOUD_BIG
    full, none, q, want_full = wc.cloud_big_case()
    empty = (np.zeros((0, 4), np.float32), np.zeros(0, np.int32))
    orders = [(dev(np.stack([full, none])), (want_full, empty)), (dev(np.stack([none, full])), (empty, want_full))]
    plan = Plan(w, h, 4, 1, "ghost", 2)
    try:
        def both(run):
            bad = []
            for k, (m, wants) in enumerate(orders):
                bad += cloud_call(plan, f"order {k}", run, m, capi.SM_MAP_I32, q, None, None, 2, w * h, wants, True)
            return bad
        report([f"fresh plan: {p}" for p in both(0)])
        capi.check(lib.sm_plan_reserve_cloud(plan.h))
        for i, word in enumerate(wc.WORDS):
            capi.check(lib.sm_debug_poison_workspace(plan.h, word))
            report([f"poison {word:#010x}: {p}" for p in both((i + 1) % 2)])
    finally:
        torch.cuda.synchronize()
        plan.close()


# ---------------------------------------------------------------------------
# interleaving: host-side state that poison cannot reach
# ---------------------------------------------------------------------------

def test_stages_interleaved_on_one_plan(hip):
    """Every stage with two settings on ONE plan, in two fixed orders; the second starts with the stages that share the
    mirrored-order map, back to back.  No poison: what could go stale here is what the plan remembers on the host
    (threshold tables, the loaded batch, which descriptors and volumes a workspace holds)."""
    c = wc.INTERLEAVE
    w, h, d, sw = c["size"]
    mode, mp, md = c["mode"], c["max_pairs"], c["max_diff"]
    left_h, right_h = wc.images(w, h, d, mp)
    left, right = dev(left_h), dev(right_h)
    host = lambda t: t.cpu().numpy()     # noqa: E731
    plan = hip.StereoPlan(w, h, d, sw, mode, max_pairs=mp)
    smap, skept, _ = wc.speckle_case(w, h, np.int32, pairs=mp)
    imap, icls, iwant, ifilled = wc.interp_case(w, h, np.int32, pairs=mp)

    def same(name, got, want):
        assert np.array_equal(host(got), np.asarray(want).reshape(tuple(got.shape))), name

    def run_lr():
        e = wc.edge_expected(mode, w, h, d, sw, md, pairs=mp)
        res = plan.run_lr(left, right, c["thresholds"][0], md, want_right=True, want_best=True)
        same("run_lr web", res.web, e["checked"]), same("run_lr right", res.web_right, e["web_right"])
        same("run_lr best", res.best, e["best"]), same("run_lr rejected", res.rejected, e["rejected"])

    def census_lr(cw):
        def f():
            e = wc.census_expected(mode, w, h, d, sw, cw, md, pairs=mp)
            res = plan.census_lr(left, right, cw, md, want_best=True)
            same(f"census_lr {cw} web", res.web, e["checked"]), same(f"census_lr {cw} best", res.best, e["best"])
            same(f"census_lr {cw} rejected", res.rejected, e["rejected"])
        return f

    def cost_lr():
        e = wc.cost_expected(mode, w, h, d, sw, c["cost"], md, pairs=mp)
        res = plan.cost_lr(left, right, c["cost"], md, want_best=True)
        same("cost_lr web", res.web, e["checked"]), same("cost_lr best", res.best, e["best"])
        same("cost_lr rejected", res.rejected, e["rejected"])

    def sgm_lr(k):
        paths, p1, p2 = c["sgm"][k]

        def f():
            e = wc.sgm_expected(mode, w, h, d, sw, 7, p1, p2, paths, md, pairs=mp)
            res = plan.sgm_lr(left, right, 7, p1, p2, paths, max_diff=md, want_best=True, want_sub=True)
            same(f"sgm_lr {paths} web", res.web, e["checked"]), same(f"sgm_lr {paths} best", res.best, e["best"])
            same(f"sgm_lr {paths} sub", res.sub, e["sub_checked"]), same(f"sgm_lr {paths} rejected", res.rejected, e["rejected"])
        return f

    def speckle(k):
        max_size, max_diff = c["speckle"][k]

        def f():
            want = [fr.speckle(m, max_size, max_diff) for m in smap]
            got, removed = plan.speckle_filter(dev(smap), max_size, max_diff, want_removed=True)
            same(f"speckle {k}", got, np.stack([x[0] for x in want]))
            same(f"speckle {k} removed", removed, [x[1] for x in want])
        return f

    def interpolate():
        got, filled = plan.interpolate(dev(imap), dev(icls), want_filled=True)
        same("interpolate", got, iwant), same("interpolate filled", filled, ifilled)

    def cloud(gi):
        def f():
            m, g, q, wants = wc.cloud_case(w, h, np.int32, gi, True, pairs=mp)
            pts, n, idx = plan.point_cloud(dev(m), q, dev(g), z_range=c["z_gates"][gi], want_index=True)
            assert host(n).tolist() == [len(i) for _, i in wants], f"cloud gate {gi} counts"
            for p, (rec, index) in enumerate(wants):
                assert np.array_equal(host(pts)[p, :len(index)].view(np.int32), rec.view(np.int32)), f"cloud gate {gi} records"
                assert np.array_equal(host(idx)[p, :len(index)], index), f"cloud gate {gi} index"
        return f

    def run(k):
        def f():
            e = wc.edge_expected(mode, w, h, d, sw, md, thr=c["thresholds"][k], pairs=mp)
            same(f"run threshold {k}", plan.run(left, right, c["thresholds"][k])[0], e["web"])
        return f

    first = [run_lr, census_lr(7), cost_lr, census_lr(5), sgm_lr(0), sgm_lr(1), speckle(0), speckle(1), interpolate,
             cloud(0), cloud(1), run(1), run(0)]
    second = [census_lr(5), cost_lr, run_lr, census_lr(7), sgm_lr(1), run(1), sgm_lr(0), cloud(1), interpolate, speckle(1),
              cloud(0), speckle(0), run(0), run_lr]
    try:
        for order in (first, second):
            for step in order:
                step()
    finally:
        torch.cuda.synchronize()
        plan.close()
