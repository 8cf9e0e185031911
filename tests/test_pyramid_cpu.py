"""The half-resolution path without a device: the two forms of the definition (tests/pyramid_reference.py) agree with
each other; the definition has the identities it should have and does what the stage is for (a coarse map comes back
to the fine size with its edge on the image's edge); the cases the GPU runs (tests/pyramid_patterns.py) can tell the
mistakes a kernel is likely to make; and both entry points refuse what needs no device to refuse."""
import ctypes as C
import re

import numpy as np
import pytest

from tests import pyramid_patterns as pp
from tests import pyramid_reference as pr

DTYPES = [np.int32, np.int16]
SMALL = [(1, 1), (2, 1), (1, 2), (2, 2), (3, 3), (5, 2), (8, 7), (9, 4), (21, 11)]


def test_new_symbols_are_declared_bound_and_exported():
    from stereomatching_amd import capi, pipeline
    syms = capi.declared_symbols()
    for name in ("sm_reduce_half", "sm_upsample_double"):
        assert name in syms and name in capi._SIGNATURES and hasattr(capi.lib, name), name
    text = capi.HEADER.read_text()
    for name, value in (("SM_REDUCE_BOX", 0), ("SM_REDUCE_BINOMIAL", 1), ("SM_UP_FILL", 1)):
        assert getattr(capi, name) == value and re.search(rf"#define {name} {value}\b", text), name
    for name in ("half_shape", "reduce_half", "upsample_double"):
        assert callable(getattr(pipeline.StereoPlan, name)), name
    assert pipeline.REDUCE_FILTERS == {"box": 0, "binomial": 1}


@pytest.mark.parametrize("filter", pp.FILTERS)
def test_both_forms_of_reduce_agree(filter):
    for i, (w, h) in enumerate(SMALL + [(33, 6)]):
        src = np.random.default_rng(i).integers(0, 256, (h, w)).astype(np.uint8)
        fast, slow = pr.reduce_half(src, filter), pr.reduce_half_naive(src, filter)
        assert fast.dtype == np.uint8 and fast.shape == pr.half_shape(w, h)[::-1] and np.array_equal(fast, slow), (w, h)
        assert np.array_equal(fast, pp.reduce_mutant(src, filter, None))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fill", [False, True])
def test_both_forms_of_upsample_agree(dtype, fill):
    for i, (w, h) in enumerate(SMALL + [(33, 6)]):
        cw, ch = pr.half_shape(w, h)
        for invalid in (0.0, 0.4, 0.9):
            a = pp.random_map(cw, ch, dtype, 7 * i + int(10 * invalid), invalid, (6, 2000)[i % 2], i % 2 == 0)
            g, gc = pp.random_guide(w, h, i), pp.random_guide(cw, ch, i + 1)
            weights = pp.table(pp.TABLES[i % 3])
            fast, slow = pr.upsample_double(a, g, gc, weights, fill), pr.upsample_double_naive(a, g, gc, weights, fill)
            assert fast.dtype == a.dtype and fast.shape == (h, w) and np.array_equal(fast, slow), (w, h, invalid)
            assert np.array_equal(fast, pp.upsample_mutant(a, g, gc, weights, fill, None))
    for name in [n for n in pp.UP_BY_NAME if "extremes" in n and np.dtype(dtype).name in n and f"fill={int(fill)}" in n]:
        maps, guides, coarse, weights, f = pp.up_inputs(name)
        assert np.array_equal(pr.upsample_double_naive(maps[0], guides[0], coarse[0], weights, f), pp.up_expected(name)[0])


def test_identities():
    for w, h in SMALL + [(64, 16), (65, 17)]:
        cw, ch = pr.half_shape(w, h)
        for level in (0, 1, 77, 255):
            for filter in pp.FILTERS:                                 # a constant image reduces to itself
                assert (pr.reduce_half(np.full((h, w), level, np.uint8), filter) == level).all(), (w, h, level, filter)
        g, gc = pp.random_guide(w, h, w), pp.random_guide(cw, ch, h)
        for dtype, off in ((np.int32, 1), (np.int16, 16)):
            for weights in (pp.table("ones"), pp.table("gw8")):
                for fill in (False, True):                            # a constant valid map, an all-invalid map
                    for v in (-5, 9, 700):
                        out = pr.upsample_double(np.full((ch, cw), v, dtype), g, gc, weights, fill)
                        assert (out == 2 * v - off).all(), (w, h, dtype, v)
                    assert not pr.upsample_double(np.zeros((ch, cw), dtype), g, gc, weights, fill).any()
    # the int16 input 8 becomes 0: the documented exception
    assert not pr.upsample_double(np.full((2, 2), 8, np.int16), np.zeros((4, 4), np.uint8), np.zeros((2, 2), np.uint8),
                                  pp.table("ones")).any()


def test_unit_weights_and_a_constant_guide_give_the_spatially_weighted_median():
    w, h = 22, 14
    cw, ch = pr.half_shape(w, h)
    a = pp.random_map(cw, ch, np.int32, 3, 0.0, 9, False)
    flat = np.full((h, w), 50, np.uint8)
    out = pr.upsample_double(a, flat, np.full((ch, cw), 200, np.uint8), pp.table("ones"))
    seen = 0
    for y in range(2, h - 2):
        for x in range(2, w - 2):
            X, Y = x >> 1, y >> 1
            rep = []                                                  # every tap repeated as often as it weighs
            for j in (-1, 0, 1):
                for i in (-1, 0, 1):
                    sx = {1: 4, 3: 2, 5: 1}[abs(4 * i + 1 - 2 * (x & 1))]
                    sy = {1: 4, 3: 2, 5: 1}[abs(4 * j + 1 - 2 * (y & 1))]
                    rep += [2 * int(a[Y + j, X + i]) - 1] * (sx * sy)
            assert len(rep) == 49
            assert out[y, x] == sorted(rep)[24], (x, y)               # 49 entries: the lower median is the middle one
            seen += 1
    assert seen > 100


def test_the_edge_comes_back_on_the_image_edge():
    """82 x 34, the gray and the disparity step at x = 41: the coarse pixel of x = 40, 41 carries the near side's
    value, so a plain upsampling leaves column 41 wrong; the guide puts it right"""
    truth, g, coarse = pp.step_scene()
    assert truth.shape == (34, 82) and coarse.shape == (17, 41) and truth[0, 40] != truth[0, 41]
    assert abs(int(g[:, 40].astype(int).mean()) - int(g[:, 41].astype(int).mean())) in range(57, 64)
    gc = pr.reduce_half(g, "binomial")
    guided = pr.upsample_double(coarse, g, gc, pp.guide_weights(8))
    plain = pr.upsample_double(coarse, g, gc, pp.table("ones"))
    wrong_guided, wrong_plain = int((guided != truth).sum()), int((plain != truth).sum())
    print(f"pixels different from the fine truth: guided {wrong_guided}, unit weights {wrong_plain}")
    assert wrong_plain >= 1 and wrong_guided < wrong_plain, (wrong_guided, wrong_plain)


def test_the_gpu_cases_cover_what_they_should():
    assert {(c["w"], c["h"]) for c in pp.REDUCE_CASES} == {(w, h) for w in pp.REDUCE_W for h in pp.REDUCE_H}
    assert pp.REDUCE_W == [1, 2, 3, 7, 8, 9, 63, 64, 65, 255, 257] and pp.REDUCE_H == [1, 2, 3, 16, 17]
    assert {n for _, n in pp.REDUCE_CALLS} == {1, 2 * pp.MAX_PAIRS, 3} and len(pp.CONTENTS) == 2 * pp.MAX_PAIRS
    imgs = pp.reduce_images(9, 3)
    assert (imgs[1] == 255).all() and set(np.unique(imgs[2])) == {0, 255} and imgs[2][0, 0] != imgs[2][0, 1]
    assert pp.UP_W == [1, 2, 3, 63, 64, 65, 127, 129] and pp.UP_H == [1, 2, 15, 16, 17, 33]
    for dtype in ("int32", "int16"):
        mine = [c for c in pp.UP_CASES if c["dtype"] == dtype and c["kind"] == "random" and "max sum" not in c["name"]]
        assert {(c["w"], c["h"]) for c in mine} == {(w, h) for w in pp.UP_W for h in pp.UP_H}
        assert {(c["invalid"], c["fill"]) for c in mine} == {(i, f) for i in (0.0, 0.3, 1.0) for f in (False, True)}
        assert {c["table"] for c in mine} == set(pp.TABLES) and {c["pairs"] for c in mine} == {1, 2, 3}
        assert {c["reduced_guide"] for c in mine} == {True, False}
        maps = np.concatenate([pp.up_inputs(n)[0].ravel() for n in pp.UP_BY_NAME if f"extremes {dtype}" in n])
        assert set(pp.EXTREMES[dtype]) | {0} == set(np.unique(maps).tolist())
    assert {I for I in (pp.I32_MIN, pp.I32_MAX)} <= set(pp.EXTREMES["int32"]) and {-32768, 32767, 8} <= set(pp.EXTREMES["int16"])
    # the largest sum occurs: all nine taps valid, every weight 65535
    maps, guides, coarse, weights, _ = pp.up_inputs("up max sum int32")
    assert (maps != 0).all() and (weights == 65535).all() and maps.shape[1] >= 3 and maps.shape[2] >= 3
    # with fill, pixels whose home is invalid are filled, and without they are not
    filled = kept = 0
    for c in pp.UP_CASES:
        if c["kind"] == "random" and c["invalid"] == 0.3:
            maps, guides, _, _, fill = pp.up_inputs(c["name"])
            h, w = guides.shape[1:]
            home0 = np.repeat(np.repeat(maps, 2, axis=1), 2, axis=2)[:, :h, :w] == 0
            n = int((pp.up_expected(c["name"])[home0] != 0).sum())
            filled += fill and n > 0
            kept += (not fill) and n == 0 and bool(home0.any())
    assert filled >= 5 and kept >= 5


@pytest.mark.parametrize("mistake", pp.REDUCE_MISTAKES)
def test_the_reduce_cases_tell_each_mistake(mistake):
    found = []
    for c in pp.REDUCE_CASES:
        for filter in pp.FILTERS:
            want = pp.reduce_expected(c["w"], c["h"], filter)
            got = np.stack([pp.reduce_mutant(img, filter, mistake) for img in pp.reduce_images(c["w"], c["h"])])
            if not np.array_equal(got, want):
                found.append(f"{c['name']} {filter}")
    assert len(found) >= (3 if mistake != "clamp at 255" else 1), (mistake, found)


@pytest.mark.parametrize("mistake", pp.UP_MISTAKES)
def test_the_upsample_cases_tell_each_mistake(mistake):
    found = []
    for c in pp.UP_CASES:
        if c["w"] * c["h"] > 70 * 20:
            continue                                                  # (the small cases suffice, and are quick)
        maps, guides, coarse, weights, fill = pp.up_inputs(c["name"])
        got = np.stack([pp.upsample_mutant(m, g, gc, weights, fill, mistake) for m, g, gc in zip(maps, guides, coarse)])
        if not np.array_equal(got, pp.up_expected(c["name"])):
            found.append(c["name"])
        if len(found) >= 3:
            break
    assert len(found) >= 3, (mistake, found)


def test_argument_checks_without_a_device():
    from stereomatching_amd import capi
    lib = capi.lib
    buf = [(C.c_char * 64)() for _ in range(4)]
    p = [C.cast(b, C.c_void_p) for b in buf]
    w = capi.w256(pp.guide_weights(8))
    I32 = capi.SM_MAP_I32

    def refused(rc, text):
        assert rc == capi.SM_ERR_ARG and text in lib.sm_last_error(), lib.sm_last_error()
    me = b"sm_reduce_half: "
    refused(lib.sm_reduce_half(None, p[0], 0, 1, p[1], None), me + b"plan is NULL")
    refused(lib.sm_reduce_half(None, None, 0, 1, p[1], None), me + b"an image pointer is NULL")
    refused(lib.sm_reduce_half(None, p[0], 0, 1, None, None), me + b"an image pointer is NULL")
    refused(lib.sm_reduce_half(None, p[0], 2, 1, p[1], None), me + b"filter 2 is neither")
    refused(lib.sm_reduce_half(None, p[0], -1, 1, p[1], None), me + b"filter -1 is neither")
    me = b"sm_upsample_double: "
    refused(lib.sm_upsample_double(None, p[0], I32, p[1], p[2], w, 0, 1, p[3], None), me + b"plan is NULL")
    refused(lib.sm_upsample_double(None, None, I32, p[1], p[2], w, 0, 1, p[3], None), me + b"a map pointer is NULL")
    refused(lib.sm_upsample_double(None, p[0], I32, p[1], p[2], w, 0, 1, None, None), me + b"a map pointer is NULL")
    refused(lib.sm_upsample_double(None, p[0], I32, None, p[2], w, 0, 1, p[3], None), me + b"a guide pointer is NULL")
    refused(lib.sm_upsample_double(None, p[0], I32, p[1], None, w, 0, 1, p[3], None), me + b"a guide pointer is NULL")
    refused(lib.sm_upsample_double(None, p[0], I32, p[1], p[2], None, 0, 1, p[3], None), me + b"weights is NULL")
    refused(lib.sm_upsample_double(None, p[0], 2, p[1], p[2], w, 0, 1, p[3], None), me + b"map_type 2")
    refused(lib.sm_upsample_double(None, p[0], I32, p[1], p[2], w, 2, 1, p[3], None), me + b"flags 0x2")
    for at in (0, 100, 255):
        zero = capi.w256([0 if i == at else 7 for i in range(256)])
        refused(lib.sm_upsample_double(None, p[0], I32, p[1], p[2], zero, 0, 1, p[3], None), me + b"weights[%d] is 0" % at)
    # (a count out of range and an overlap are measured against the plan: test_pyramid_gpu.py refuses them on one)
    with pytest.raises(ValueError, match="256 numbers"):
        capi.w256([1] * 255)
