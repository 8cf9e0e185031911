"""The edge-aware smoother on the GPU: sm_wls_filter against the numpy definition (tests/wls_reference.py), bit for
bit -- both output types as integers, d_raw's doubles as uint64, no tolerance anywhere.  Every expected value comes
from the CPU definition; none from the HIP path.  The cases are those of tests/wls_patterns.py (test_wls_cpu.py shows
what they can tell): a lane owns a line, 64 lines make a wave, the row kernels work in chunks of 16 columns, and the sizes
sit on and around those edges, down to lines of one element."""
import ctypes as C

import numpy as np
import pytest
import torch

from stereomatching_amd import capi
from stereomatching_amd.capi import lib
from tests import wls_patterns as wp
from tests import wls_reference as wr
from tests import workspace_poison_cases as wc
from tests.guarded import guarded_input
from tests.test_write_bounds_gpu import P, Plan, expect, out, report, stream, twice

pytestmark = pytest.mark.gpu
TORCH = {"int32": torch.int32, "int16": torch.int16}
TYPE = {"int32": capi.SM_MAP_I32, "int16": capi.SM_MAP_I16}
MAXP = 3


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()      # (a copy: the shared inputs are read-only)


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def plan_for(hip, w, h, max_pairs=MAXP):
    """the smoother reads W, H and max_pairs of the plan only"""
    return hip.StereoPlan(w, h, 4, 1, "ghost", max_pairs=max_pairs)


def differences(tag, got, want, maps):
    """(out, raw, filled) of the call against the definition's -> problems"""
    bad = []
    for q in range(len(maps)):
        for name, g, w in (("out", got[0][q], want[0][q]), ("raw", bits(got[1][q]), bits(want[1][q]))):
            diff = np.argwhere(g != w)
            if len(diff):
                y, x = (int(v) for v in diff[0])
                bad.append(f"{tag} pair {q}: {name}: {len(diff)} pixels differ, first (x={x}, y={y}): "
                           f"{got[0][q][y, x]} / {got[1][q][y, x]!r} != {want[0][q][y, x]} / {want[1][q][y, x]!r} "
                           f"(in {maps[q][y, x]})")
        if int(got[2][q]) != int(want[2][q]):
            bad.append(f"{tag} pair {q}: filled {int(got[2][q])} != {int(want[2][q])}")
    return bad


def run_cases(hip, cases):
    """every case through StereoPlan.wls_filter (one plan per size) -> problems"""
    bad, plans = [], {}
    try:
        for c in cases:
            key = (c["w"], c["h"], c["max_pairs"])
            if key not in plans:
                plans[key] = plan_for(hip, *key)
            maps, guides, conf, weights = wp.inputs(c["name"])
            got = plans[key].wls_filter(dev(maps), dev(guides), weights, c["lam"], c["T"], conf=dev(conf),
                                        fill=not c["flags"], out_dtype=TORCH[c["tout"]], want_raw=True, want_filled=True)
            assert got[0].dtype == TORCH[c["tout"]] and got[1].dtype == torch.float64
            bad += differences(c["name"], [host(t) for t in got], wp.expected(c["name"]), maps)
    finally:
        for p in plans.values():
            p.close()
    return bad


@pytest.mark.parametrize("size", wp.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_random_maps(hip, size):
    cases = [c for c in wp.CASES if c["kind"] == "random" and (c["w"], c["h"]) == size]
    assert len(cases) == 2
    report(run_cases(hip, cases))


@pytest.mark.parametrize("kind", ["special", "bands", "extremes"])
def test_special_cases(hip, kind):
    """eight passes, no links (lambda 0, a zero table), the largest links; whole rows and columns without a valid pixel;
    the ends of both types in every combination, where an int16 output saturates"""
    cases = [c for c in wp.CASES if c["kind"] == kind]
    assert len(cases) >= 2
    report(run_cases(hip, cases))


def test_python_layer_shapes_its_results_and_refuses_wrong_tensors(hip):
    c = wp.BY_NAME["eight passes"]
    maps, guides, conf, weights = wp.inputs(c["name"])
    plan = plan_for(hip, c["w"], c["h"])
    try:
        m, g, cf = dev(maps), dev(guides), dev(conf)
        only = plan.wls_filter(m, g, weights, c["lam"], 2, conf=cf)
        assert isinstance(only, torch.Tensor) and only.dtype == m.dtype
        o, filled = plan.wls_filter(m, g, weights, c["lam"], 2, conf=cf, want_filled=True)
        assert torch.equal(o, only) and filled.dtype == torch.int32 and filled.shape == (c["pairs"],)
        want = [wr.wls_filter(maps[q], guides[q], weights, c["lam"], 2, conf[q]) for q in range(c["pairs"])]
        assert np.array_equal(host(o), np.stack([x[0] for x in want])) and host(filled).tolist() == [x[2] for x in want]
        given = torch.zeros((c["pairs"], c["h"], c["w"]), dtype=torch.int16, device="cuda")
        assert plan.wls_filter(m, g, weights, c["lam"], 2, conf=cf, out=given) is given
        with pytest.raises(ValueError, match="guide"):
            plan.wls_filter(m, g.to(torch.int32), weights, 0.5)
        with pytest.raises(ValueError, match="conf"):
            plan.wls_filter(m, g, weights, 0.5, conf=cf[:1])
        with pytest.raises(ValueError, match="int32 .* or int16"):
            plan.wls_filter(g, g, weights, 0.5)
        with pytest.raises(ValueError, match="out_dtype"):
            plan.wls_filter(m, g, weights, 0.5, out_dtype=torch.float32)
        with pytest.raises(capi.StereoHipError, match="sm_wls_filter: iterations 9"):
            plan.wls_filter(m, g, weights, 0.5, iterations=9)
    finally:
        plan.close()


# ---------------------------------------------------------------------------
# write bounds (tests/guarded.py), in place
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("tin,tout", wp.TYPES)
def test_writes_its_maps_and_nothing_else(tin, tout):
    bad = []
    weights, table = capi.w256(wp.guide_weights(8)), wp.guide_weights(8)
    odd = {"int32": 4, "int16": 2}
    for idx, (w, h, T) in enumerate([(33, 17, 2), (64, 16, 1), (130, 67, 3), (1, 5, 2), (5, 1, 2)]):
        pairs = (2, 1, 3)[idx % 3]
        plan = Plan(w, h, 4, 1, "toroidal", MAXP)
        maps = np.stack([wp.random_map(w, h, np.dtype(tin), 9 * idx + q, 0.3, False) for q in range(pairs)])
        guides = np.stack([wp.random_guide(w, h, 9 * idx + q) for q in range(pairs)])
        conf = np.stack([wp.random_conf(w, h, 9 * idx + q) for q in range(pairs)])
        shp, s = (pairs, h, w), stream()
        for off in (0, 1):
            gi = guarded_input(maps, "cuda", off * odd[tin], "in")
            gg, gc = guarded_input(guides, "cuda", off * 3, "guide"), guarded_input(conf, "cuda", off, "conf")
            for flags in (0, capi.SM_WLS_NO_FILL):
                want = [wr.wls_filter(maps[q], guides[q], table, 0.25, T, conf[q], flags, tout) for q in range(pairs)]
                t = f"{tin}->{tout} W={w} H={h} T={T} pairs={pairs}/{MAXP} flags={flags} offset {off}"
                om, orw = out(shp, TORCH[tout], (1 - off) * odd[tout], MAXP, "out"), out(shp, torch.float64, off * 8, MAXP, "raw")
                of = out((pairs,), torch.int32, off * 4, MAXP, "filled")
                bad += twice(t, lambda r: lib.sm_wls_filter(plan.h, P(gi.t), TYPE[tin], P(gc.t), P(gg.t), weights, 0.25, T, flags,
                                                            pairs, P(om.t), TYPE[tout], P(orw.t), P(of.t), s),
                             [om, orw, of], [gi, gg, gc])
                bad += expect(t, om, np.stack([x[0] for x in want])) + expect(t, of, [x[2] for x in want])
                if not np.array_equal(bits(orw.value()), bits(np.stack([x[1] for x in want]))):
                    bad.append(f"{t}: raw differs from the definition")
                t += " (out alone)"
                om = out(shp, TORCH[tout], off * odd[tout], MAXP, "out")
                bad += twice(t, lambda r: lib.sm_wls_filter(plan.h, P(gi.t), TYPE[tin], P(gc.t), P(gg.t), weights, 0.25, T, flags,
                                                            pairs, P(om.t), TYPE[tout], None, None, s), [om], [gi, gg, gc])
                bad += expect(t, om, np.stack([x[0] for x in want]))
        plan.close()
    report(bad)


@pytest.mark.parametrize("dtype", ["int32", "int16"])
def test_in_place(hip, dtype):
    """d_out == d_in of one type: a pixel's input is read (for its validity) before its output is written"""
    w, h = 70, 33
    maps = np.stack([wp.random_map(w, h, np.dtype(dtype), 70 + q, 0.4, False) for q in range(2)])
    guides = np.stack([wp.random_guide(w, h, 70 + q) for q in range(2)])
    table = wp.guide_weights(8)
    plan = plan_for(hip, w, h)
    try:
        for fill in (True, False):
            m = dev(maps)
            got = plan.wls_filter(m, dev(guides), table, 0.25, 2, fill=fill, out=m, want_raw=True, want_filled=True)
            assert got[0] is m
            want = [wr.wls_filter(maps[q], guides[q], table, 0.25, 2, None, 0 if fill else wr.NO_FILL) for q in range(2)]
            report(differences(f"in place fill={fill}", [host(t) for t in got], [np.stack([x[i] for x in want]) for i in range(2)]
                               + [[x[2] for x in want]], maps))
    finally:
        plan.close()


# ---------------------------------------------------------------------------
# second turn and residue
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("tin,tout", [("int32", "int16"), ("int16", "int32")])
def test_second_calls_and_a_poisoned_workspace(hip, tin, tout):
    """one plan: a call, another map, then per poison word a batch of one, the full batch and a batch of one again.  As
    doubles the words are small subnormals, NaNs and large numbers: a plane element read before it is written shows"""
    w, h, T = 129, 33, 2
    maps = np.stack([wp.random_map(w, h, np.dtype(tin), 200 + q, (0.3, 0.6, 0.1)[q], False) for q in range(MAXP)])
    guides = np.stack([wp.random_guide(w, h, 200 + q) for q in range(MAXP)])
    conf = np.stack([wp.random_conf(w, h, 200 + q) for q in range(MAXP)])
    table = wp.guide_weights(32)
    want = [wr.wls_filter(maps[q], guides[q], table, 1.0, T, conf[q], 0, tout) for q in range(MAXP)]
    other = [wr.wls_filter(maps[2 - q], guides[q], table, 1.0, T, None, 0, tout) for q in range(MAXP)]
    plan = plan_for(hip, w, h)

    def stage(tag, pairs, order=None, cf=conf, ref=want):
        m = maps if order is None else maps[order]
        got = plan.wls_filter(dev(m[:pairs]), dev(guides[:pairs]), table, 1.0, T, conf=dev(None if cf is None else cf[:pairs]),
                              out_dtype=TORCH[tout], want_raw=True, want_filled=True)
        return differences(tag, [host(t) for t in got], [np.stack([x[i] for x in ref[:pairs]]) for i in range(2)]
                           + [[x[2] for x in ref[:pairs]]], m[:pairs])
    try:
        base = plan.workspace_bytes()
        report(stage("first call", MAXP))
        assert plan.workspace_bytes() == base + 24 * MAXP * w * h
        report(stage("another map", MAXP, [2, 1, 0], None, other) + stage("the first again", MAXP))
        for word in wc.WORDS:
            plan._poison_workspace(word)
            bad = []
            for k, pairs in enumerate((1, MAXP, 1)):
                bad += stage(f"poison {word:#010x} call {k}", pairs)
            report(bad)
        assert plan.workspace_bytes() == base + 24 * MAXP * w * h
    finally:
        plan.close()


# ---------------------------------------------------------------------------
# capture, arguments
# ---------------------------------------------------------------------------

def test_capture_is_refused_before_the_reservation_and_holds_the_table_after_it(hip):
    w, h, T = 100, 45, 2
    maps = [wp.random_map(w, h, np.int16, 40 + i, 0.3, False) for i in range(2)]
    guides = [wp.random_guide(w, h, 40 + i) for i in range(2)]
    table = wp.guide_weights(8)
    weights = capi.w256(table)
    plan = plan_for(hip, w, h, 1)
    try:
        base = plan.workspace_bytes()
        src = torch.zeros((1, h, w), dtype=torch.int16, device="cuda")
        gsrc = torch.zeros((1, h, w), dtype=torch.uint8, device="cuda")
        res = torch.zeros((1, h, w), dtype=torch.int32, device="cuda")
        raw = torch.zeros((1, h, w), dtype=torch.float64, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        mark = torch.zeros(4, dtype=torch.int32, device="cuda")

        def call():
            return lib.sm_wls_filter(plan._h, P(src), capi.SM_MAP_I16, None, P(gsrc), weights, 0.25, T, 0, 1, P(res),
                                     capi.SM_MAP_I32, P(raw), P(cnt), plan._stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            rc = call()
            text = lib.sm_last_error()
            mark.add_(1)                                              # the capture is still valid: this is recorded
        assert rc == capi.SM_ERR_ARG and b"sm_wls_filter: " in text and b"sm_plan_reserve_wls" in text, text
        assert plan.workspace_bytes() == base
        g.replay()
        torch.cuda.synchronize()
        assert mark.tolist() == [1, 1, 1, 1] and not res.any()
        plan.reserve_wls()
        assert plan.workspace_bytes() == base + 24 * w * h
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            capi.check(call())
        for i in range(256):
            weights[i] = 1                                            # the host's table changes after the capture
        assert plan.workspace_bytes() == base + 24 * w * h
        seen = []
        for rep in (0, 0, 1):                                         # the same input twice, then another
            src.copy_(dev(maps[rep])[None])
            gsrc.copy_(dev(guides[rep])[None])
            res.zero_()
            raw.zero_()
            cnt.fill_(12345)
            g.replay()
            torch.cuda.synchronize()
            want = wr.wls_filter(maps[rep], guides[rep], table, 0.25, T, None, 0, np.int32)
            assert np.array_equal(host(res)[0], want[0]) and np.array_equal(bits(host(raw)[0]), bits(want[1])), rep
            assert int(cnt[0]) == want[2] and want[2] > 0, rep
            seen.append(host(raw).copy())
        assert np.array_equal(seen[0], seen[1])
        assert not np.array_equal(seen[0][0], wr.wls_filter(maps[0], guides[0], np.ones(256, np.uint16), 0.25, T)[1])
    finally:
        plan.close()


def test_argument_checks_on_a_plan(hip):
    w, h = 64, 32
    plan = plan_for(hip, w, h, 2)
    base = plan.workspace_bytes()
    n = 2 * h * w
    big = torch.full((8 * n,), 77, dtype=torch.int32, device="cuda")    # (the maps far apart: a range of doubles that
    m = [big[:n].view(2, h, w), big[3 * n:4 * n].view(2, h, w)]          #  starts in one cannot reach the other)
    guide = torch.zeros((2, h, w), dtype=torch.uint8, device="cuda")
    conf = torch.full((2, h, w), 9, dtype=torch.uint8, device="cuda")
    raw = torch.full((2, h, w), 77.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    p, pg, pcf, pr, pc = [P(t) for t in m], P(guide), P(conf), P(raw), P(cnt)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    I32, I16 = capi.SM_MAP_I32, capi.SM_MAP_I16
    wt = capi.w256(wp.guide_weights(8))

    def at(t, off):
        return C.c_void_p(t.data_ptr() + off)

    def call(d_in=p[0], map_type=I32, cf=pcf, g=pg, weights=wt, lam=0.5, T=2, flags=0, pairs=2, d_out=p[1], out_type=I32,
             d_raw=pr, d_filled=pc):
        return lib.sm_wls_filter(plan._h, d_in, map_type, cf, g, weights, lam, T, flags, pairs, d_out, out_type, d_raw,
                                 d_filled, st)

    def refused(rc, text):
        assert rc == capi.SM_ERR_ARG and b"sm_wls_filter: " + text in lib.sm_last_error(), lib.sm_last_error()
        torch.cuda.synchronize()
        assert bool((m[1] == 77).all()) and bool((cnt == 77).all()) and bool((raw == 77.0).all())      # nothing is written
    refused(call(pairs=0), b"pairs 0 outside 1..2")
    refused(call(pairs=3), b"pairs 3 outside 1..2")
    refused(call(d_out=at(m[0], 4), pairs=1), b"d_out overlaps d_in")
    refused(call(d_out=p[0], out_type=I16), b"d_out overlaps d_in")                   # in place, but not of one type
    refused(call(d_in=at(m[1], 2 * h * w), map_type=I16), b"d_out overlaps d_in")
    refused(call(g=p[0]), b"d_guide overlaps d_in")
    refused(call(g=at(m[1], 16)), b"d_guide overlaps d_out")
    refused(call(cf=p[0]), b"d_conf overlaps d_in")
    refused(call(cf=p[1]), b"d_conf overlaps d_out")
    refused(call(cf=pg), b"d_conf overlaps d_guide")
    refused(call(d_raw=p[0]), b"d_raw overlaps d_in")
    refused(call(d_raw=at(m[1], 8)), b"d_raw overlaps d_out")
    refused(call(d_raw=pg), b"d_raw overlaps d_guide")
    refused(call(d_raw=pcf), b"d_raw overlaps d_conf")
    refused(call(d_filled=at(m[0], 8)), b"d_filled overlaps d_in")
    refused(call(d_filled=at(m[1], 8)), b"d_filled overlaps d_out")
    refused(call(d_filled=at(guide, 8)), b"d_filled overlaps d_guide")
    refused(call(d_filled=at(conf, 8)), b"d_filled overlaps d_conf")
    refused(call(d_filled=at(raw, 8)), b"d_filled overlaps d_raw")
    refused(call(lam=-1.0), b"lambda -1")
    refused(call(T=0), b"iterations 0 outside 1..8")
    refused(call(flags=6), b"flags 0x6")
    refused(call(map_type=7), b"map_type 7")
    refused(call(out_type=7), b"out_type 7")
    refused(call(g=None), b"d_guide is NULL")
    refused(call(weights=None), b"weights is NULL")
    refused(call(d_out=None), b"a map pointer is NULL")
    assert plan.workspace_bytes() == base                             # no refusal allocates
    plan.close()
