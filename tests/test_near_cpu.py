"""The guided census re-search without a device: the C ABI declares, binds and exports the three entries and refuses
bad arguments before it touches a device; the numpy definition (tests/near_reference.py) agrees with a pixel-by-pixel
restatement; the two consequences of the definition the GPU tests lean on hold; the right-reference search written
out without mirrors is the definition's; the cases the GPU runs (tests/near_patterns.py) can tell the definition from
the definition with one mistake; and the scene the feature is for: a half-resolution prior that is right nowhere,
re-searched to the truth."""
import ctypes as C

import numpy as np
import pytest

from tests import census_reference as cr
from tests import near_patterns as npat
from tests import near_reference as nr

NEW = ("sm_census_wta_near", "sm_census_wta_near_right", "sm_census_near_lr")


def test_new_symbols_are_declared_bound_and_exported():
    from stereomatching_amd import capi
    syms = capi.declared_symbols()
    for s in NEW:
        assert s in syms and s in capi._SIGNATURES and hasattr(capi.lib, s), s
    from stereomatching_amd import pipeline
    for m in ("census_wta_near", "census_wta_near_right", "census_near_lr"):
        assert callable(getattr(pipeline.StereoPlan, m)), m


def test_argument_checks_precede_device_use():
    """every check that needs no plan, on a NULL plan (pairs, overlaps and the window and shift limits read the plan:
    tests/test_near_gpu.py covers them on a real one)"""
    from stereomatching_amd import capi
    lib = capi.lib
    px = C.c_void_p(16)           # never dereferenced: every call below is refused first

    def refused(rc, text):
        assert rc == capi.SM_ERR_ARG
        assert text in lib.sm_last_error(), lib.sm_last_error()

    for name in ("sm_census_wta_near", "sm_census_wta_near_right"):
        f, me = getattr(lib, name), name.encode()
        out = b"d_web_right" if name.endswith("right") else b"d_web"
        prior = b"d_prior_right" if name.endswith("right") else b"d_prior"
        refused(f(None, px, px, 7, 1, px, 1, px, None, None), me + b": plan is NULL")
        refused(f(None, None, px, 7, 1, px, 1, px, None, None), me + b": input image pointer is NULL")
        refused(f(None, px, None, 7, 1, px, 1, px, px, None), me + b": input image pointer is NULL")
        refused(f(None, px, px, 7, 1, None, 1, px, None, None), me + b": " + prior + b" is NULL")
        refused(f(None, px, px, 7, 1, px, 1, None, px, None), me + b": " + out + b" is NULL")
        refused(f(None, px, px, 4, 1, px, 1, px, None, None), me + b": census_width 4 is not 3, 5 or 7")
        refused(f(None, px, px, 7, 1, px, 0, px, None, None), me + b": radius 0 outside 1..4")
        refused(f(None, px, px, 7, 1, px, 5, px, None, None), me + b": radius 5 outside 1..4")
        refused(f(None, px, px, 7, 1, px, -1, px, None, None), me + b": radius -1 outside 1..4")
    f, me = lib.sm_census_near_lr, b"sm_census_near_lr"
    refused(f(None, px, px, 7, 1, px, px, 1, 0, px, None, None, None, None), me + b": plan is NULL")
    refused(f(None, None, px, 7, 1, px, px, 1, 0, px, None, None, None, None), me + b": input image pointer is NULL")
    refused(f(None, px, px, 7, 1, None, px, 1, 0, px, None, None, None, None), me + b": prior map pointer is NULL")
    refused(f(None, px, px, 7, 1, px, None, 1, 0, px, None, None, None, None), me + b": prior map pointer is NULL")
    refused(f(None, px, px, 7, 1, px, px, 1, 0, None, px, px, px, None), me + b": d_web is NULL")
    refused(f(None, px, px, 7, 1, px, px, 1, -1, px, None, None, None, None), me + b": max_diff -1 is negative")
    refused(f(None, px, px, 6, 1, px, px, 1, 0, px, None, None, None, None), me + b": census_width 6 is not 3, 5 or 7")
    refused(f(None, px, px, 7, 1, px, px, 0, 0, px, None, None, None, None), me + b": radius 0 outside 1..4")
    refused(f(None, px, px, 7, 1, px, px, 5, 0, px, None, None, None, None), me + b": radius 5 outside 1..4")


def rand_gray(w, h, seed, levels=256):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, levels, (h, w)).astype(np.uint8), rng.integers(0, levels, (h, w)).astype(np.uint8))


@pytest.mark.parametrize("census", [3, 5, 7])
@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
@pytest.mark.parametrize("w,h,d,sw", [(7, 5, 6, 3), (4, 3, 9, 1), (9, 6, 5, 5), (3, 2, 4, 1), (1, 1, 3, 3), (2, 7, 5, 5),
                                      (6, 2, 7, 3)])
def test_numpy_definition_equals_the_pixel_loop(census, mode, w, h, d, sw):
    """the vectorised search against a per-pixel, per-tap loop on tiny images (1 x 1, W < n, H < n among them), with
    zeros, priors outside 1 .. D and the ends of int32 in the prior"""
    for seed, levels, radius in ((1, 256, 1), (2, 3, 2), (3, 2, 4)):
        left, right = rand_gray(w, h, seed + 7 * w + census, levels)
        rng = np.random.default_rng(seed + w + h)
        prior = rng.integers(-radius - 1, d + radius + 3, (h, w)).astype(np.int32)
        prior.reshape(-1)[::5] = 0
        if prior.size > 3:
            prior.reshape(-1)[1], prior.reshape(-1)[2] = npat.I32_MIN, npat.I32_MAX
        want = nr.near_bruteforce(left, right, prior, d, sw, census, radius, mode)
        got = nr.near(left, right, prior, d, sw, census, radius, mode)
        assert np.array_equal(got[1], want[1]), (census, mode, w, h, d, sw, seed)
        assert np.array_equal(got[0], want[0]), (census, mode, w, h, d, sw, seed)


SHAPES = [(24, 9, 12, 3, 5, "toroidal"), (24, 9, 12, 3, 5, "ghost"), (17, 12, 20, 5, 7, "toroidal"),
          (17, 12, 20, 5, 7, "ghost"), (30, 7, 40, 1, 3, "ghost"), (11, 13, 6, 9, 3, "toroidal")]


@pytest.mark.parametrize("w,h,d,sw,census,mode", SHAPES)
@pytest.mark.parametrize("radius", [1, 2, 4])
def test_near_agrees_with_the_full_search_wherever_the_prior_is_close(w, h, d, sw, census, mode, radius):
    """|prior - web_full| <= r: web and best are the full search's (its first minimum lies in K and no smaller d
    ties); elsewhere best_near >= best_full.  So the full map as prior returns itself and its costs"""
    left, right = rand_gray(w, h, 11 * w + d, 4)            # (few grey levels: ties between shifts)
    best_full, web_full = cr.wta(left, right, d, sw, census, mode)
    rng = np.random.default_rng(w + radius)
    prior = (web_full + rng.integers(-radius - 2, radius + 3, web_full.shape)).astype(np.int32)
    best, web = nr.near(left, right, prior, d, sw, census, radius, mode)
    close = np.abs(prior.astype(np.int64) - web_full) <= radius
    # (a prior of 0 within r of the truth is still invalid)
    close &= prior != 0
    assert close.any() and (~close).any()
    assert np.array_equal(web[close], web_full[close]) and np.array_equal(best[close], best_full[close])
    has = nr.candidates(prior, d, radius)[2]
    assert (best[has] >= best_full[has]).all()
    assert (web[~has] == 0).all() and (best[~has] == 0).all()
    best, web = nr.near(left, right, web_full, d, sw, census, radius, mode)
    assert np.array_equal(web, web_full) and np.array_equal(best, best_full)


@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
@pytest.mark.parametrize("radius", [1, 2, 4])
def test_few_shifts_make_every_prior_a_full_search(mode, radius):
    """D <= r + 1: any prior in 1 .. D gives census_wta's result"""
    for d in range(1, radius + 2):
        left, right = rand_gray(19, 8, d + radius, 3)
        prior = np.random.default_rng(d).integers(1, d + 1, (8, 19)).astype(np.int32)
        best, web = nr.near(left, right, prior, d, 3, 5, radius, mode)
        best_full, web_full = cr.wta(left, right, d, 3, 5, mode)
        assert np.array_equal(web, web_full) and np.array_equal(best, best_full)


@pytest.mark.parametrize("census", [3, 5, 7])
@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
@pytest.mark.parametrize("w,h,d,sw,radius", [(12, 9, 8, 3, 1), (10, 7, 15, 5, 2), (5, 4, 9, 1, 4), (16, 11, 20, 9, 2)])
def test_the_right_search_written_out_is_the_mirrored_definition(census, mode, w, h, d, sw, radius):
    """popcount(C_R(u) ^ C_L(u - d)), u - d mod W / C_L = 0 left of column 0, is mirror(near(mirror(R), mirror(L),
    mirror(prior_right))) -- and so is the search on the left pass's descriptors read in mirrored order, which is what
    the kernel does (Hamming distance is blind to the permutation of bits that mirroring an image causes)"""
    left, right = rand_gray(w, h, 3 * w + census, 256)
    prior = np.random.default_rng(w + d).integers(-radius, d + radius + 2, (h, w)).astype(np.int32)
    want = nr.near_right(left, right, prior, d, sw, census, radius, mode)
    got = nr.near_right_direct(left, right, prior, d, sw, census, radius, mode)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])


@pytest.mark.parametrize("mutant", npat.MUTANTS)
def test_the_cases_tell_every_mutant_from_the_definition(mutant):
    name = npat.MUTANT_CASE[mutant]
    c = npat.BY_NAME[name]
    left, right, prior, prior_right = npat.inputs(name)
    args = (c["d"], c["sw"], c["census"], c["radius"], c["mode"])
    differs = False
    for q in range(c["pairs"]):
        e = npat.expected(name)[q]
        if mutant == "mirror_plus":
            best, web = npat.mutant_near_right(left[q], right[q], prior_right[q], *args)
            differs |= not (np.array_equal(web, e["web_right"]) and np.array_equal(best, e["best_right"]))
        else:
            best, web = npat.mutant_near(left[q], right[q], prior[q], *args, mutant)
            differs |= not (np.array_equal(web, e["web"]) and np.array_equal(best, e["best"]))
    assert differs, (mutant, name)


def test_the_mutant_machinery_without_a_mistake_is_the_definition():
    """mutant_near differs from near by its mistake alone: with the mistake that cannot show (sentinel_best on a
    prior without empty K) it is the definition"""
    left, right = rand_gray(20, 9, 5, 4)
    prior = np.random.default_rng(1).integers(1, 13, (9, 20)).astype(np.int32)
    for mode in ("toroidal", "ghost"):
        want = nr.near(left, right, prior, 12, 3, 5, 2, mode)
        got = npat.mutant_near(left, right, prior, 12, 3, 5, 2, mode, "sentinel_best")
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_case_list_covers_every_factor():
    cs = npat.CASES
    assert 90 <= len(cs) <= 120
    for key, values in (("w", npat.WIDTHS), ("h", npat.HEIGHTS), ("sw", npat.WINDOWS), ("d", npat.SHIFTS),
                        ("census", npat.CENSUS), ("radius", npat.RADII), ("mode", npat.MODES), ("pairs", [1, 2, 3]),
                        ("prior", npat.PRIORS)):
        assert {c[key] for c in cs} >= set(values), key
    # every prior kind in both border modes, every window with every census width
    assert {(c["prior"], c["mode"]) for c in cs} >= {(p, m) for p in npat.PRIORS for m in npat.MODES}
    assert {(c["sw"], c["census"]) for c in cs} >= {(s, c) for s in npat.WINDOWS for c in npat.CENSUS}


def test_all_tie_maps_take_the_first_candidate():
    """the GPU's arithmetic extremes say what they are meant to.  A constant gray pair: every cost ties at 0, so web = 1 + max(0, s - 1 - r) wherever K is not empty"""
    for name in ("all tie toroidal", "all tie ghost"):
        c = npat.BY_NAME[name]
        _, _, prior, _ = npat.inputs(name)
        web = npat.stacked(name, "web")
        s = prior.astype(np.int64)
        assert np.array_equal(web, np.where(s == 0, 0, 1 + np.maximum(0, s - 1 - c["radius"])))
        assert (npat.stacked(name, "best") == 0).all()
    # ... and the lattice against its inverse costs A = 30000 (the key's top field, the packed u16 sums) at the last
    # shift of every pixel, in both directions: the result wherever that shift is the only candidate
    c = npat.BY_NAME["maximum cost"]
    _, _, prior, prior_right = npat.inputs("maximum cost")
    for p, key in ((prior, "best"), (prior_right, "best_right")):
        alone = p == c["d"] + c["radius"]
        assert alone.any() and (npat.stacked("maximum cost", key)[alone] == 30000).all()


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_what_it_is_for(seed):
    """96 x 40, D = 32, window 5, census 5, ghost: true shift 9 left of column 48 and 21 from it on.  The half path's
    prior (the even shift below the truth) is right at 0 of 3840 pixels; the re-search at r = 1 is right at all 2200
    pixels of columns 2 .. 33 and 50 .. 72 (off the step, the occluded band and the right border), as the full search is"""
    left, right, truth, prior = npat.step_scene(seed)
    assert int((prior == truth).sum()) == 0 and truth.size == 3840
    cols = np.r_[2:34, 50:73]
    _, web = nr.near(left, right, prior, 32, 5, 5, 1, "ghost")
    assert int((web[:, cols] == truth[:, cols]).sum()) == 2200 == truth[:, cols].size
    _, full = cr.wta(left, right, 32, 5, 5, "ghost")
    assert int((full[:, cols] == truth[:, cols]).sum()) == 2200
