"""The definition of occlusion-aware interpolation (tests/interp_reference.py) against itself: the vectorised forms
against the per-pixel walks, the identities the definition promises, and its meaning on a hand-built scene with a true
occlusion band.  No GPU."""
import numpy as np
import pytest

from tests import interp_patterns as ip
from tests import interp_reference as ir
from tests import oracle

DTYPES = [np.int32, np.int16]
BORDERS = ["toroidal", "ghost"]
SMALL = [(1, 1), (1, 9), (9, 1), (2, 2), (2, 7), (7, 2), (13, 11), (31, 17)]
EXTREMES = {np.int32: [-2**31, 2**31 - 1, -1, 1], np.int16: [-32768, 32767, -32767, 1]}


def maps_for(dtype):
    """(name, map) over the small sizes: random with negative values, type extremes, all-invalid, all-valid, a
    single valid pixel at each corner and in the middle"""
    out = []
    rng = np.random.default_rng(3)
    for i, (w, h) in enumerate(SMALL):
        for invalid in (0.3, 0.7, 0.95):
            out.append((f"random {w}x{h} {invalid}", ip.random_map(w, h, dtype, 10 * i + int(10 * invalid), invalid,
                                                                   1, 9, negative=True)))
        ext = rng.choice(np.array([0, 0] + EXTREMES[dtype], dtype), (h, w))
        out.append((f"extremes {w}x{h}", ext))
        out.append((f"all-invalid {w}x{h}", np.zeros((h, w), dtype)))
        out.append((f"all-valid {w}x{h}", ip.random_map(w, h, dtype, i, 0.0)))
        for y, x in {(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2)}:
            one = np.zeros((h, w), dtype)
            one[y, x] = -4
            out.append((f"single {w}x{h} at {x},{y}", one))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_interpolate_forms_agree(dtype):
    for i, (name, a) in enumerate(maps_for(dtype)):
        h, w = a.shape
        for cls in (None, ip.random_class(w, h, i), ip.random_class(w, h, i, ones=True)):
            got = ir.interpolate(a, cls)
            assert got.dtype == a.dtype
            assert np.array_equal(got, ir.interpolate_naive(a, cls)), name
    for name, make in ip.PATTERNS.items():
        a = make(45, 37, dtype)
        assert np.array_equal(ir.interpolate(a, ip.random_class(45, 37, 1)),
                              ir.interpolate_naive(a, ip.random_class(45, 37, 1))), name


@pytest.mark.parametrize("border", BORDERS)
def test_classify_forms_agree(border):
    rng = np.random.default_rng(5)
    for i, (w, h) in enumerate(SMALL + [(70, 5), (64, 3)]):
        for d in (1, 4, w, w + 3, 2 * w + 1, 64):
            web = ip.random_map(w, h, np.int32, i + d, 0.6, 1, d)
            right = rng.integers(-1, d + 3, (h, w)).astype(np.int32)      # with values outside 1 .. D
            got = ir.classify(web, right, d, border)
            assert got.dtype == np.uint8
            assert np.array_equal(got, ir.classify_naive(web, right, d, border)), (w, h, d)


@pytest.mark.parametrize("border", BORDERS)
def test_classify_is_the_intersection_test(border):
    """a pixel is 2 iff a brute-force loop over d finds the line of sight meeting the right map; ghost never reads
    u >= W; toroidal wraps; web_right = 0 -> every invalid pixel occluded"""
    rng = np.random.default_rng(11)
    w, h, d = 23, 6, 30                                                     # D > W: the toroidal row is met twice
    web = ip.random_map(w, h, np.int32, 2, 0.7, 1, d)
    right = rng.integers(0, d + 1, (h, w)).astype(np.int32)
    got = ir.classify(web, right, d, border)
    for y in range(h):
        for x in range(w):
            if web[y, x] != 0:
                assert got[y, x] == ir.VALID
                continue
            meets = False
            for k in range(d):
                u = x + k
                if border == "ghost" and u >= w:
                    continue
                meets |= int(right[y, u % w]) == k + 1
            assert got[y, x] == (ir.MISMATCHED if meets else ir.OCCLUDED), (x, y)
    assert np.array_equal(ir.classify(web, np.zeros_like(right), d, border), np.where(web != 0, 0, 1))
    # one row whose only intersection lies across the wrap: pixel W-2, d = 3 -> u = 1
    web = np.zeros((1, 8), np.int32)
    right = np.zeros((1, 8), np.int32)
    right[0, 1] = 4
    got = ir.classify(web, right, 6, border)
    assert got[0, 6] == (ir.MISMATCHED if border == "toroidal" else ir.OCCLUDED)
    assert (got == ir.MISMATCHED).sum() == (border == "toroidal")
    # ghost: a value that would match at u = W (outside) does not count; the same value one pixel inside does
    right = np.zeros((1, 8), np.int32)
    right[0, 7] = 3
    got = ir.classify(web, right, 6, "ghost")
    assert got[0, 5] == ir.MISMATCHED and (got == ir.MISMATCHED).sum() == 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_interpolate_identities(dtype):
    w, h = 29, 19
    a = ip.random_map(w, h, dtype, 7, 0.6, 1, 9, negative=True)
    ones, twos = np.ones((h, w), np.uint8), np.full((h, w), 2, np.uint8)
    occ, med = ir.interpolate(a, ones), ir.interpolate(a, twos)
    # valid pixels unchanged; class 0, class 2 and no class are one rule; the class of a valid pixel is not read
    for out in (occ, med):
        assert np.array_equal(out[a != 0], a[a != 0])
    assert np.array_equal(med, ir.interpolate(a)) and np.array_equal(med, ir.interpolate(a, np.zeros((h, w), np.uint8)))
    assert np.array_equal(occ, ir.interpolate(a, np.where(a != 0, 2, 1).astype(np.uint8)))
    full = ip.random_map(w, h, dtype, 8, 0.0)
    assert np.array_equal(ir.interpolate(full, ones), full) and ir.filled(full, full) == 0
    none = np.zeros((h, w), dtype)
    assert not ir.interpolate(none, ones).any() and not ir.interpolate(none).any()
    # the two rules by candidate count m, over maps dense and sparse enough to show every m
    seen = set()
    for seed, invalid in ((7, 0.6), (8, 0.9), (9, 0.97), (10, 0.985), (11, 0.985)):
        b = ip.random_map(w, h, dtype, seed, invalid, 1, 9, negative=True)
        occ_b, med_b = ir.interpolate(b, ones), ir.interpolate(b, twos)
        m = ir.candidate_count(b)
        hole = b == 0
        seen |= set(np.unique(m[hole]).tolist())
        assert not occ_b[hole & (m == 0)].any() and not med_b[hole & (m == 0)].any()
        for k in (1, 3, 4):
            assert np.array_equal(occ_b[hole & (m == k)], med_b[hole & (m == k)]), k
        assert (occ_b[hole & (m >= 5)] <= med_b[hole & (m >= 5)]).all()
        # m = 2: c_1 against c_0 -- the paper's second lowest is the LARGER of two candidates.  Pinned on purpose.
        # m = 1: that one value under either rule
        for y, x in np.argwhere(hole & (m <= 2) & (m >= 1)):
            c = ir.candidates_naive(b, x, y)
            assert len(c) == m[y, x]
            assert occ_b[y, x] == c[-1] and med_b[y, x] == c[0]
        assert (occ_b[hole & (m == 2)] >= med_b[hole & (m == 2)]).all()
    assert seen >= {0, 1, 2, 3, 4, 5, 8}, f"the maps do not show every case: {sorted(seen)}"
    m = ir.candidate_count(a)
    # a map constant where valid fills every reachable hole with the constant
    const = np.where(a != 0, -9, 0).astype(dtype)
    for cls in (None, ones):
        out = ir.interpolate(const, cls)
        assert np.array_equal(out, np.where(m > 0, -9, const))
    # the eight directions are closed under transposing and flipping
    cls = ip.random_class(w, h, 4)
    want = ir.interpolate(a, cls)
    assert np.array_equal(ir.interpolate(a.T, cls.T), want.T)
    assert np.array_equal(ir.interpolate(a[::-1], cls[::-1]), want[::-1])
    assert np.array_equal(ir.interpolate(a[:, ::-1], cls[:, ::-1]), want[:, ::-1])


def test_sub_map_follows_the_web_map():
    """same validity mask and |sub - 16 web| <= 8 at every valid pixel -> the same bound at every filled pixel"""
    rng = np.random.default_rng(2)
    for seed in range(4):
        w, h = 41, 23
        web = ip.random_map(w, h, np.int32, seed, 0.6, 1, 60)
        sub = np.where(web != 0, 16 * web + rng.integers(-8, 9, (h, w)), 0).astype(np.int16)
        assert ((sub != 0) == (web != 0)).all()
        cls = ip.random_class(w, h, seed)
        fw, fs = ir.interpolate(web, cls), ir.interpolate(sub, cls)
        assert ((fs != 0) == (fw != 0)).all()
        assert (np.abs(fs.astype(np.int64) - 16 * fw.astype(np.int64)) <= 8).all()
        assert ir.filled(web, fw) == ir.filled(sub, fs) > 0


def test_patterns_say_what_they_claim():
    for name, make in ip.PATTERNS.items():
        for w, h in ((150, 140), (45, 37)):
            ip.informative(name, make(w, h, np.int32))
    a = ip.band_v(400, 30, np.int16)
    assert (a == 0).all(axis=0).sum() == 100                      # a quarter of the width
    assert (ip.lone(9, 5, np.int32) != 0).sum() == 1 and (ip.anti_frame(9, 5, np.int32) != 0).sum() == 1


def test_the_binding_declares_the_feature():
    """the C ABI, its ctypes signatures and the StereoPlan methods of the feature exist, with the definition's classes"""
    from stereomatching_amd import capi, pipeline
    for name in ("sm_occlusion_classify", "sm_interpolate", "sm_plan_reserve_interp"):
        assert name in capi.declared_symbols() and name in capi._SIGNATURES, name
        assert hasattr(capi.lib, name), name
    for name in ("occlusion_classify", "interpolate", "reserve_interp"):
        assert callable(getattr(pipeline.StereoPlan, name, None)), name
    assert (capi.SM_CLASS_VALID, capi.SM_CLASS_OCCLUDED, capi.SM_CLASS_MISMATCHED) == \
        (ir.VALID, ir.OCCLUDED, ir.MISMATCHED)


def test_semantics_on_a_hand_built_scene():
    """No matcher involved.  Background web = 3, a foreground rectangle web = 20, the right map consistent with both,
    the occlusion band (to the right of the rectangle: derived in interp_patterns.occlusion_scene) and a few isolated
    pixels set to 0.  The band is occluded and filled with background; the isolated pixels are mismatches and take their
    surface's value; the reference's hole filling on the same input does neither."""
    from stereomatching_amd import pipeline                         # the feature's binding: absent before it
    assert callable(getattr(pipeline.StereoPlan, "interpolate", None))
    for border in BORDERS:
        s = ip.occlusion_scene(border=border)
        web, band, bg, fg = s["web"], s["band"], s["bg"], s["fg"]
        x0, x1, y0, y1 = s["rect"]
        assert band[y0:y1, x1:].any() and not band[:, :x1].any()   # the band lies to the right of the rectangle
        cls = ir.classify(web, s["web_right"], s["d"], border)
        assert (cls[band] == ir.OCCLUDED).all()
        for y, x in s["isolated"]:
            assert cls[y, x] == ir.MISMATCHED, (x, y)
        assert ((cls != 0) == (web == 0)).all()
        out = ir.interpolate(web, cls)
        assert (out[band] == bg).all()
        assert set(np.unique(out).tolist()) == {bg, fg}            # dense, and nothing strictly between
        for y, x in s["isolated"]:
            assert out[y, x] == (fg if x0 <= x < x1 and y0 <= y < y1 else bg)
        # the contrast: every 0 -> the truncated mean of its four flat-index neighbours, once
        old = oracle.fill_web_holes(web, 3)
        assert (old[band] == 0).any() or ((old > bg) & (old < fg)).any()
        assert (old[band] == 0).sum() > band.sum() // 2            # most of the band stays a hole
