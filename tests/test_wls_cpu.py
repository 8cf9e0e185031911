"""The edge-aware smoother without a device: the two forms of the definition (tests/wls_reference.py) agree bit for
bit; the definition keeps the identities that follow from it; it does what the stage is for on one scene; the cases the
GPU runs (tests/wls_patterns.py) can tell single roundings apart and stay clear of subnormal numbers; and sm_wls_filter
refuses what needs no plan to refuse."""
import ctypes as C
import math
import re

import numpy as np
import pytest

from tests import wls_patterns as wp
from tests import wls_reference as wr

DTYPES = [np.int32, np.int16]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def rms(x, truth, mask=None):
    d = (np.asarray(x, np.float64) - truth)
    return float(np.sqrt(np.mean((d[mask] if mask is not None else d) ** 2)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_both_forms_of_the_definition_agree(dtype):
    n = 0
    for i, (w, h) in enumerate([(1, 1), (1, 4), (5, 1), (2, 2), (9, 7), (17, 3)]):
        for T in (1, 2, 3, 4):
            a = wp.random_map(w, h, dtype, 10 * i + T, (0.0, 0.3, 0.6)[(i + T) % 3], (i + T) % 2 == 0)
            g, conf = wp.random_guide(w, h, i + T), wp.random_conf(w, h, i + T) if T % 2 else None
            weights = wp.table(("gw8", "holes", "gw32")[(i + T) % 3])
            for flags, out_dtype in ((0, None), (wr.NO_FILL, np.int16), (0, np.int32)):
                fast = wr.wls_filter(a, g, weights, 0.5, T, conf, flags, out_dtype)
                slow = wr.wls_filter_naive(a, g, weights, 0.5, T, conf, flags, out_dtype)
                assert fast[0].dtype == (out_dtype or dtype) and np.array_equal(fast[0], slow[0]), (w, h, T, flags)
                assert np.array_equal(bits(fast[1]), bits(slow[1])) and fast[2] == slow[2], (w, h, T, flags)
                assert np.array_equal(bits(fast[1]), bits(wp.mutant(a, g, weights, 0.5, T, conf, flags, None)))
                n += fast[2]
    assert n > 0                                                      # something was filled


def test_lambdas_are_the_formula_and_sum_to_half_of_lambda():
    assert wr.lambdas(3.0, 1) == [(1.5 * 3.0) * 1.0 / 3.0]
    assert wr.lambdas(0.7, 3) == [(1.5 * 0.7) * 16.0 / 63.0, (1.5 * 0.7) * 4.0 / 63.0, (1.5 * 0.7) * 1.0 / 63.0]
    for T in range(1, 9):
        lams = wr.lambdas(1.0, T)
        assert all(a == 4.0 * b or math.isclose(a, 4.0 * b, rel_tol=1e-15) for a, b in zip(lams, lams[1:]))
        assert math.isclose(sum(lams), 0.5, rel_tol=1e-12)


@pytest.mark.parametrize("dtype", DTYPES)
def test_identities(dtype):
    w, h = 23, 11
    a = wp.random_map(w, h, dtype, 5, 0.3, True)
    g, conf = wp.random_guide(w, h, 5), wp.random_conf(w, h, 5)
    u = wr.units(a)
    # no links: every pixel is its own average
    for weights, lam in ((wp.table("zero"), 0.5), (wp.table("gw8"), 0.0)):
        out, raw, filled = wr.wls_filter(a, g, weights, lam, 3, conf)
        keeps = (a != 0) & (conf > 0)
        assert np.array_equal(raw[keeps], u[keeps]) and not raw[~keeps].any() and filled == 0
        assert np.array_equal(out[keeps], a[keeps])
    # a constant map stays that constant wherever anything arrives, whatever the confidence (both planes take the
    # same path: N = k M exactly for a power of two, and to the last bit's rounding otherwise)
    const = np.where(a != 0, 64, 0).astype(dtype)
    out, raw, _ = wr.wls_filter(const, g, wp.table("gw8"), 0.5, 3, conf)
    assert (out == 64).all()
    assert np.array_equal(raw, np.full((h, w), wr.units(np.array([64], dtype))[0]))
    # pairs are independent, and NULL confidence is a map of 255s
    b = wp.random_map(w, h, dtype, 6, 0.3, False)
    one = wr.wls_filter(b, g, wp.table("gw8"), 0.5, 2, None)
    assert np.array_equal(bits(one[1]), bits(wr.wls_filter(b, g, wp.table("gw8"), 0.5, 2, np.full((h, w), 255, np.uint8))[1]))
    assert not np.array_equal(bits(one[1]), bits(wr.wls_filter(a, g, wp.table("gw8"), 0.5, 2, None)[1]))
    # NO_FILL only zeroes
    full, nofill = wr.wls_filter(a, g, wp.table("gw8"), 0.5, 2, conf), wr.wls_filter(a, g, wp.table("gw8"), 0.5, 2, conf, wr.NO_FILL)
    assert np.array_equal(nofill[1], np.where(a != 0, full[1], 0.0)) and nofill[2] == 0 and full[2] > 0


def test_the_scene_is_smoothed_filled_and_keeps_its_edge():
    """80 x 33, a gray step at x = 40 over a disparity step of 320 sixteenths; 30 % holes, 5 % outliers of low
    confidence.  Measured with this definition: RMS error against the truth 1.63 over all pixels (the valid inliers of
    the input: 7.31; without the confidence map: 25.9); largest error in columns 36 .. 43: 6.1; no output pixel 0."""
    a, g, conf, truth, outlier = wp.scene()
    assert a.shape == (33, 80) and 0.25 < (a == 0).mean() < 0.35 and 0.03 < outlier.mean() < 0.07
    weights = wp.guide_weights(8)
    out, raw, filled = wr.wls_filter(a, g, weights, 64 / 1024, 3, conf)
    inliers = (a != 0) & ~outlier
    rms_in, rms_out = rms(a, truth, inliers), rms(raw, truth)
    rms_null = rms(wr.wls_filter(a, g, weights, 64 / 1024, 3, None)[1], truth)
    edge = float(np.abs(raw - truth)[:, 36:44].max())
    print(f"rms: input inliers {rms_in:.2f}, output {rms_out:.2f}, without confidence {rms_null:.2f}; beside the step {edge:.2f}")
    assert (out != 0).all() and filled == int((a == 0).sum())                   # dense
    assert rms_out < rms_in / 2
    assert rms_null > rms_out
    assert edge < 16
    assert np.array_equal(out, np.rint(raw).astype(np.int16))


def test_the_gpu_cases_cover_what_they_should():
    cs = wp.CASES
    rnd = [c for c in cs if c["kind"] == "random"]
    assert {(c["w"], c["h"]) for c in rnd} == set(wp.SIZES)
    assert {(1, 1), (1, 5), (5, 1), (2, 2), (16, 64), (17, 65), (33, 70), (80, 33), (130, 67), (257, 3)} <= set(wp.SIZES)
    assert {(c["tin"], c["tout"]) for c in rnd} == set(wp.TYPES)
    assert {c["pairs"] for c in rnd} == {1, 2, 3} and {c["max_pairs"] for c in cs} == {3}
    assert {c["T"] for c in rnd} == {1, 2, 3, 4} and {c["conf"] for c in rnd} == {True, False}
    assert {c["flags"] for c in rnd} == {0, wr.NO_FILL} and {c["table"] for c in rnd} == {"gw8", "gw32", "holes"}
    assert [c["T"] for c in cs].count(8) == 1
    assert any(c["lam"] == 0.0 for c in cs) and any(c["table"] == "zero" for c in cs)
    assert (wp.table("holes") == 0).sum() > 40 and (wp.table("holes") != 0).sum() > 200
    # whole rows and columns without a valid pixel get a value all the same, unless filling is off
    maps, _, _, _ = wp.inputs("invalid rows and columns")
    assert not maps[:, 0].any() and not maps[:, 21].any() and not maps[:, :, 7].any() and not maps[:, :, -1].any()
    assert (wp.expected("invalid rows and columns")[0] != 0).all()
    out = wp.expected("invalid rows and columns, no fill")[0]
    assert not out[:, 21].any() and not out[:, :, 7].any() and out.any()
    # the extremes saturate an int16 output and reach the ends of an int32 one
    assert {-32768, 32767} <= set(np.unique(wp.expected("extremes int32->int16")[0]).tolist())
    assert wp.expected("extremes int32->int32")[0].max() > 2**30 and wp.expected("extremes int32->int32")[0].min() < -2**30
    assert wp.expected("extremes int16->int32")[0].max() > 1500


def test_no_case_comes_near_a_subnormal_or_a_non_finite_number():
    seen = {}
    wr.WATCH = seen
    try:
        for c in wp.CASES:
            maps, guides, conf, weights = wp.inputs(c["name"])
            wr.wls_filter(maps[0], guides[0], weights, c["lam"], c["T"], None if conf is None else conf[0], c["flags"], c["tout"])
    finally:
        wr.WATCH = None
    assert seen["finite"] and seen["tiny"] > 1e-100, seen


@pytest.mark.parametrize("mistake", wp.MISTAKES)
def test_the_gpu_cases_tell_each_mistake(mistake):
    """the definition with one mistake differs from the definition in d_raw on named GPU cases"""
    found = []
    for c in wp.CASES:
        if c["w"] * c["h"] > 80 * 33 or c["w"] < 2 or c["h"] < 2:
            continue
        maps, guides, conf, weights = wp.inputs(c["name"])
        want = wp.expected(c["name"])[1]
        got = wp.mutant(maps[0], guides[0], weights, c["lam"], c["T"], None if conf is None else conf[0], c["flags"], mistake)
        if not np.array_equal(bits(got), bits(want[0])):
            found.append(c["name"])
        if len(found) >= 3:
            break
    assert len(found) >= 3, (mistake, found)


def test_argument_checks_without_a_plan():
    from stereomatching_amd import capi
    lib = capi.lib
    assert {"sm_wls_filter", "sm_plan_reserve_wls"} <= set(capi.declared_symbols()) and capi.SM_WLS_NO_FILL == 1
    assert re.search(r"#define SM_WLS_NO_FILL 1\b", capi.HEADER.read_text())
    buf = [(C.c_char * 64)() for _ in range(3)]
    p = [C.cast(b, C.c_void_p) for b in buf]
    w = capi.w256(wp.guide_weights(8))
    I32, I16 = capi.SM_MAP_I32, capi.SM_MAP_I16
    me = b"sm_wls_filter: "

    def call(plan=None, d_in=p[0], map_type=I32, conf=None, guide=p[1], weights=w, lam=0.5, T=3, flags=0, pairs=1, out=p[2],
             out_type=I16):
        return lib.sm_wls_filter(plan, d_in, map_type, conf, guide, weights, lam, T, flags, pairs, out, out_type, None, None, None)

    def refused(rc, text):
        assert rc == capi.SM_ERR_ARG and me + text in lib.sm_last_error(), lib.sm_last_error()
    refused(call(), b"plan is NULL")
    refused(call(d_in=None), b"a map pointer is NULL")
    refused(call(out=None), b"a map pointer is NULL")
    refused(call(guide=None), b"d_guide is NULL")
    refused(call(weights=None), b"weights is NULL")
    refused(call(map_type=2), b"map_type 2")
    refused(call(out_type=-1), b"out_type -1")
    for lam in (-1e-9, float(2**20) + 1, float("inf"), float("nan")):
        refused(call(lam=lam), b"lambda ")
    refused(call(lam=0.0), b"plan is NULL")
    refused(call(lam=float(2**20)), b"plan is NULL")
    refused(call(T=0), b"iterations 0 outside 1..8")
    refused(call(T=9), b"iterations 9 outside 1..8")
    refused(call(T=8), b"plan is NULL")
    refused(call(flags=2), b"flags 0x2")
    refused(call(flags=capi.SM_WLS_NO_FILL), b"plan is NULL")
    rc = lib.sm_plan_reserve_wls(None)
    assert rc == capi.SM_ERR_ARG and b"sm_plan_reserve_wls: plan is NULL" in lib.sm_last_error()
