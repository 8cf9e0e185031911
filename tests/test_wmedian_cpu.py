"""The guided weighted median without a device: the two forms of the definition (tests/wmedian_reference.py) agree
with each other and, with equal weights, with the post-filters' median; the definition does what the stage is for (it
moves a fattened disparity edge back to the image's edge); the cases the GPU runs (tests/wmedian_patterns.py) can
tell the mistakes a kernel is likely to make; and sm_weighted_median refuses what needs no device to refuse."""
import ctypes as C

import numpy as np
import pytest

from tests import filter_reference as fr
from tests import wmedian_patterns as wp
from tests import wmedian_reference as wr

DTYPES = [np.int32, np.int16]


@pytest.mark.parametrize("dtype", DTYPES)
def test_both_forms_of_the_definition_agree(dtype):
    n = 0
    for i, (w, h) in enumerate([(1, 1), (1, 40), (70, 1), (15, 9), (65, 17)]):
        for radius in (1, 4, 7):
            a = wp.random_map(w, h, dtype, 10 * i + radius, (0.0, 0.3, 0.7)[(i + radius) % 3], (6, 2000)[i % 2], i % 2 == 0)
            g = wp.random_guide(w, h, i + radius)
            weights = wp.table(("gw8", "nonmono", "gw32", "ones")[(i + radius) % 4])
            t = np.sort(wr.totals(a, g, radius, weights)[a == 0])
            near_median = max(1, int(t[(len(t) - 1) // 2])) if len(t) else 1
            for fill, fmw in ((False, 1), (True, 1), (True, near_median)):
                fast, nf = wr.weighted_median(a, g, radius, weights, fill, fmw)
                slow, ns = wr.weighted_median_naive(a, g, radius, weights, fill, fmw)
                assert fast.dtype == a.dtype and np.array_equal(fast, slow) and nf == ns, (w, h, radius, fill, fmw)
                assert np.array_equal(fast, wp.mutant(a, g, radius, weights, fill, fmw, None))
                assert not fill or np.array_equal(fast[a != 0], wr.weighted_median(a, g, radius, weights)[0][a != 0])
                n += nf
    assert n > 0                                                      # something was filled


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [3, 5])
def test_unit_weights_give_the_plain_median(dtype, k):
    for i, (w, h) in enumerate([(1, 1), (40, 1), (15, 9), (65, 17)]):
        a = wp.random_map(w, h, dtype, 3 * i + k, (0.0, 0.3, 0.7, 0.95)[i], (6, 2000)[i % 2], True)
        got, filled = wr.weighted_median(a, wp.random_guide(w, h, i), k // 2, wp.table("ones"))
        assert np.array_equal(got, fr.median(a, k)) and filled == 0, (w, h)


def test_the_fattened_edge_moves_back_to_the_image_edge():
    """80 x 33: a gray step at x = 40 with noise of +-3, the disparity step at x = 44: 4 x 33 = 132 fattened pixels"""
    a, g, fat = wp.step_scene(80, 33, 40, 4, seed=1)
    assert int(fat.sum()) == 132 and (a[fat] == 40).all() and (a[:, 44:] == 24).all()
    weights = wp.guide_weights(8)
    assert weights[0] == 1024 and weights[255] == 1 and weights.dtype == np.uint16
    left = {r: int((wr.weighted_median(a, g, r, weights)[0][fat] == 40).sum()) for r in (2, 5, 7)}
    assert left[2] == 132 and left[5] < 132 and left[7] < 66, left
    for r in (1, 2, 5, 7):                                            # the plain median of any radius moves nothing
        assert int((wr.weighted_median(a, g, r, wp.table("ones"))[0][fat] == 40).sum()) == 132, r
    # ... and the weighted median leaves what was right as it was
    out = wr.weighted_median(a, g, 7, weights)[0]
    assert np.array_equal(out[~fat], a[~fat])


def test_the_gpu_cases_cover_what_they_should():
    cs = wp.CASES
    rnd = [c for c in cs if c["kind"] == "random" and c["table"] != "max"]
    assert {(c["w"], c["h"]) for c in rnd} == set(wp.SIZES)
    for dtype in ("int32", "int16"):
        for size in wp.SIZES:
            radii = {c["radius"] for c in rnd if (c["w"], c["h"]) == size and c["dtype"] == dtype}
            assert radii == ({1, 2, 3, 4, 5, 6, 7} if size in wp.ALL_RADII else {1, 3, 7}), (dtype, size)
        mine = [c for c in rnd if c["dtype"] == dtype]
        assert {c["invalid"] for c in mine} == {0.0, 0.3, 0.7, 0.95}
        assert {(c["pairs"], c["max_pairs"]) for c in mine} == {(2, 2), (1, 3)}
        assert {c["fill"] for c in mine} == {"off", "one", "median"}
        assert {c["table"] for c in mine} == {"gw8", "gw32", "ones", "nonmono"}
        assert {c["negative"] for c in mine} == {True, False}
        for fill in ("off", "one", "median"):                         # every mode in the register and in the LDS path
            assert {c["radius"] <= 3 for c in mine if c["fill"] == fill} == {True, False}
    # the largest sum occurs
    maps, guides, weights, _, _ = wp.inputs("max sum int32")
    assert int(wr.totals(maps[0], guides[0], 7, weights).max()) == 225 * 65535
    # a fill threshold near the median of T is one that decides: pixels are filled, and pixels are not
    decided = 0
    for c in cs:
        if c["fill"] == "median":
            maps, guides, weights, fill, fmw = wp.inputs(c["name"])
            out, filled = wp.expected(c["name"])
            holes = int((maps[0] == 0).sum())
            decided += fmw > 1 and 0 < int(filled[0]) < holes
    assert decided >= 10
    # the guide-step cases lie on the tile borders and have something to move
    maps, guides, _, _, _ = wp.inputs("guide step int32 r7")
    assert abs(int(guides[0][:, 63].mean()) - int(guides[0][:, 64].mean())) > 100
    assert abs(int(guides[1][15].mean()) - int(guides[1][16].mean())) > 100
    out, _ = wp.expected("guide step int32 r7")
    assert (out != maps)[maps != 0].any()


@pytest.mark.parametrize("mistake", wp.MISTAKES)
def test_the_gpu_cases_tell_each_mistake(mistake):
    """the definition with one mistake differs from the definition on a named GPU case (on several: the first few
    are listed in the assertion's message when there are too few)"""
    found = []
    for c in wp.CASES:
        if c["w"] * c["h"] > 70 * 20 or (mistake.startswith("fill") or mistake.startswith("invalid centre")) and c["fill"] == "off":
            continue                                                  # (the small cases suffice, and are quick)
        maps, guides, weights, fill, fmw = wp.inputs(c["name"])
        want, _ = wp.expected(c["name"])
        got = np.stack([wp.mutant(m, g, c["radius"], weights, fill, fmw, mistake) for m, g in zip(maps, guides)])
        if not np.array_equal(got, want):
            found.append(c["name"])
        if len(found) >= 3:
            break
    assert len(found) >= 3, (mistake, found)


def test_the_midpoint_must_not_be_taken_in_32_bits():
    """a window that spans INT32_MIN + 1 .. INT32_MAX: the bisection with the unsigned midpoint finds the
    definition's value, with either 32-bit signed formula it finds another"""
    name = "extremes int32 r2 ones"
    maps, guides, weights, fill, fmw = wp.inputs(name)
    want, _ = wp.expected(name)
    a, g = maps[0], guides[0]
    seen = {"difference": 0, "sum": 0, "windows": 0}
    for y in range(2, a.shape[0] - 2):
        for x in range(2, a.shape[1] - 2, 3):
            values, wts = wp.window(a, g, 2, weights, x, y)
            if not values or min(values) != wp.I32_MIN + 1 or max(values) != wp.I32_MAX:
                continue
            seen["windows"] += 1
            truth = int(want[0][y, x]) if a[y, x] != 0 or sum(wts) >= fmw else None
            if truth is None:
                continue
            assert wp.bisect(values, wts, wp.mid_unsigned) == truth, (x, y)
            seen["difference"] += wp.bisect(values, wts, wp.mid_int32_difference) != truth
            seen["sum"] += wp.bisect(values, wts, wp.mid_int32_sum) != truth
    assert seen["windows"] > 50 and seen["difference"] > 0 and seen["sum"] > 0, seen
    # the first step alone: hi - lo = 2^32 - 2 wraps to -2, and the "midpoint" leaves the interval
    assert wp.mid_unsigned(wp.I32_MIN + 1, wp.I32_MAX) == 0
    assert wp.mid_int32_difference(wp.I32_MIN + 1, wp.I32_MAX) == wp.I32_MIN
    assert wp.mid_int32_sum(1, wp.I32_MAX) < 1


def test_guide_weights_helper_is_the_formula():
    from stereomatching_amd import pipeline
    for sigma, peak in ((8, 1024), (32, 1024), (3.5, 65535), (100, 7)):
        want = np.maximum(1, np.rint(peak * np.exp(-np.arange(256) / sigma))).astype(np.uint16)
        got = pipeline.guide_weights(sigma, peak) if peak != 1024 else pipeline.guide_weights(sigma)
        assert got.dtype == np.uint16 and got.shape == (256,) and np.array_equal(got, want)
    assert np.array_equal(pipeline.guide_weights(8), wp.guide_weights(8))


def test_argument_checks_without_a_device():
    from stereomatching_amd import capi
    lib = capi.lib
    assert "sm_weighted_median" in capi.declared_symbols() and capi.SM_WMED_FILL == 1
    import re
    assert re.search(r"#define SM_WMED_FILL 1\b", capi.HEADER.read_text())
    buf = [(C.c_char * 64)() for _ in range(3)]
    p = [C.cast(b, C.c_void_p) for b in buf]
    w = capi.w256(wp.guide_weights(8))
    I32 = capi.SM_MAP_I32

    def refused(rc, text):
        assert rc == capi.SM_ERR_ARG and text in lib.sm_last_error(), lib.sm_last_error()
    me = b"sm_weighted_median: "
    refused(lib.sm_weighted_median(None, p[0], I32, p[1], 3, w, 0, 1, 1, p[2], None, None), me + b"plan is NULL")
    refused(lib.sm_weighted_median(None, None, I32, p[1], 3, w, 0, 1, 1, p[2], None, None), me + b"a map pointer is NULL")
    refused(lib.sm_weighted_median(None, p[0], I32, p[1], 3, w, 0, 1, 1, None, None, None), me + b"a map pointer is NULL")
    refused(lib.sm_weighted_median(None, p[0], I32, None, 3, w, 0, 1, 1, p[2], None, None), me + b"d_guide is NULL")
    refused(lib.sm_weighted_median(None, p[0], I32, p[1], 3, None, 0, 1, 1, p[2], None, None), me + b"weights is NULL")
    refused(lib.sm_weighted_median(None, p[0], 2, p[1], 3, w, 0, 1, 1, p[2], None, None), me + b"map_type 2")
    refused(lib.sm_weighted_median(None, p[0], I32, p[1], 0, w, 0, 1, 1, p[2], None, None), me + b"radius 0 outside 1..7")
    refused(lib.sm_weighted_median(None, p[0], I32, p[1], 8, w, 0, 1, 1, p[2], None, None), me + b"radius 8 outside 1..7")
    zero = capi.w256([0] + [5] * 255)
    refused(lib.sm_weighted_median(None, p[0], I32, p[1], 3, zero, 0, 1, 1, p[2], None, None), me + b"weights[0] is 0")
    refused(lib.sm_weighted_median(None, p[0], I32, p[1], 3, w, 2, 1, 1, p[2], None, None), me + b"flags 0x2")
    refused(lib.sm_weighted_median(None, p[0], I32, p[1], 3, w, capi.SM_WMED_FILL, 0, 1, p[2], None, None),
            me + b"fill_min_weight 0 is below 1")
    # (without the flag fill_min_weight is ignored: the call gets as far as the plan)
    refused(lib.sm_weighted_median(None, p[0], I32, p[1], 3, w, 0, 0, 1, p[2], None, None), me + b"plan is NULL")
    with pytest.raises(ValueError, match="256 numbers"):
        capi.w256([1] * 255)
    with pytest.raises(ValueError, match="0 .. 65535"):
        capi.w256([1] * 255 + [65536])
