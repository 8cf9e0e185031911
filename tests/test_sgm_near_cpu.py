"""Banded SGM without a device: the C ABI declares, binds and exports the four entries and refuses bad arguments before
it touches a device; the numpy definition (tests/sgm_near_reference.py) agrees with its path-by-path loop form; the
consequences of the definition that pin it to sm_sgm_wta and to sm_census_wta_near hold; the right-reference pass
written out is the mirrored left pass; a monotone intensity change alters nothing; the cases the GPU runs
(tests/sgm_near_patterns.py) can tell the definition from ten mistaken ones; and the scene the feature is for."""
import ctypes as C

import numpy as np
import pytest

from tests import near_reference as nr
from tests import sgm_near_patterns as sp
from tests import sgm_near_reference as sn
from tests import sgm_reference as sg

NEW = ("sm_sgm_wta_near", "sm_sgm_wta_near_right", "sm_sgm_near_lr", "sm_plan_reserve_sgm_near")


def test_new_symbols_are_declared_bound_and_exported():
    from stereomatching_amd import capi
    syms = capi.declared_symbols()
    for s in NEW:
        assert s in syms and s in capi._SIGNATURES and hasattr(capi.lib, s), s
    from stereomatching_amd import pipeline
    for m in ("sgm_wta_near", "sgm_wta_near_right", "sgm_near_lr", "reserve_sgm_near"):
        assert callable(getattr(pipeline.StereoPlan, m)), m


def test_argument_checks_precede_device_use():
    """every check that needs no plan, on a NULL plan, with sm_sgm_wta's messages for census width, paths and penalties
    and sm_census_wta_near's for the radius and the priors (pairs, overlaps and the window and shift limits read the
    plan: tests/test_sgm_near_gpu.py covers them on a real one)"""
    from stereomatching_amd import capi
    lib = capi.lib
    px = C.c_void_p(16)           # never dereferenced: every call below is refused first

    def refused(rc, text):
        assert rc == capi.SM_ERR_ARG
        assert text in lib.sm_last_error(), lib.sm_last_error()

    def one(name, cw=7, p1=10, p2=120, paths=8, prior=px, radius=1, left=px, right=px, web=px):
        f = getattr(lib, name)
        if name.endswith("right"):
            return f(None, left, right, cw, p1, p2, paths, 1, prior, radius, web, None, None)
        return f(None, left, right, cw, p1, p2, paths, 1, prior, radius, web, None, None, None)
    for name in ("sm_sgm_wta_near", "sm_sgm_wta_near_right"):
        me = name.encode()
        out = b"d_web_right" if name.endswith("right") else b"d_web"
        prior = b"d_prior_right" if name.endswith("right") else b"d_prior"
        refused(one(name), me + b": plan is NULL")
        refused(one(name, left=None), me + b": input image pointer is NULL")
        refused(one(name, right=None), me + b": input image pointer is NULL")
        refused(one(name, prior=None), me + b": " + prior + b" is NULL")
        refused(one(name, web=None), me + b": " + out + b" is NULL")
        refused(one(name, cw=4), me + b": census_width 4 is not 3, 5 or 7")
        refused(one(name, paths=5), me + b": paths 5 is not 4 or 8")
        refused(one(name, paths=16), me + b": paths 16 is not 4 or 8")
        refused(one(name, p1=-1), me + b": penalties p1 -1, p2 120 break 0 <= p1 <= p2 <= 32767")
        refused(one(name, p1=121), me + b": penalties p1 121, p2 120 break")
        refused(one(name, p2=32768), me + b": penalties p1 10, p2 32768 break")
        for r in (0, 5, -1):
            refused(one(name, radius=r), me + b": radius %d outside 1..4" % r)

    def lr(cw=7, p1=10, p2=120, paths=8, prior=px, prior_right=px, radius=1, max_diff=0, left=px, web=px):
        return lib.sm_sgm_near_lr(None, left, px, cw, p1, p2, paths, 1, prior, prior_right, radius, max_diff, web, None,
                                  None, None, None, None)
    me = b"sm_sgm_near_lr"
    refused(lr(), me + b": plan is NULL")
    refused(lr(left=None), me + b": input image pointer is NULL")
    refused(lr(prior=None), me + b": prior map pointer is NULL")
    refused(lr(prior_right=None), me + b": prior map pointer is NULL")
    refused(lr(web=None), me + b": d_web is NULL")
    refused(lr(max_diff=-1), me + b": max_diff -1 is negative")
    refused(lr(cw=6), me + b": census_width 6 is not 3, 5 or 7")
    refused(lr(paths=6), me + b": paths 6 is not 4 or 8")
    refused(lr(p1=5, p2=4), me + b": penalties p1 5, p2 4 break")
    refused(lr(radius=0), me + b": radius 0 outside 1..4")
    refused(lr(radius=5), me + b": radius 5 outside 1..4")
    assert lib.sm_plan_reserve_sgm_near(None) == capi.SM_ERR_ARG
    assert b"sm_plan_reserve_sgm_near: plan is NULL" in lib.sm_last_error()


def rand_gray(w, h, seed, levels=256):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, levels, (h, w)).astype(np.uint8), rng.integers(0, levels, (h, w)).astype(np.uint8))


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


PRIOR_KINDS = ("noise", "jumps", "zero_ends", "extremes", "clipped", "zeros30")


@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
@pytest.mark.parametrize("w,h,d,sw,census", [(7, 5, 6, 3, 7), (4, 3, 9, 1, 3), (9, 6, 12, 5, 5), (3, 2, 4, 1, 7),
                                            (1, 1, 3, 1, 5), (2, 7, 5, 1, 3), (11, 9, 20, 3, 7)])
def test_vectorised_definition_equals_the_path_loop(mode, w, h, d, sw, census):
    """the dense form against the loop that follows every path with the band as a dict, on tiny images (1 x 1, one row
    of lines, diagonals of length 1 among them), every kind of prior, 4 and 8 paths, p1 = 0 and p1 = p2"""
    for i, kind in enumerate(PRIOR_KINDS):
        left, right = rand_gray(w, h, 31 * w + d + i, (256, 3)[i % 2])
        radius = 1 + (i + w) % 4
        prior = sp.make_prior(kind, w, h, d, radius, np.random.default_rng(i))
        p1, p2 = sp.PENALTIES[(i + h) % 4]
        args = (left, right, prior, d, sw, census, p1, p2, (8, 4)[i % 2], radius, mode)
        assert same(sn.sgm_near(*args), sn.sgm_near_loop(*args)), (kind, radius, p1, p2)


@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
@pytest.mark.parametrize("paths", [4, 8])
def test_a_band_that_holds_every_shift_gives_sgm(mode, paths):
    """consequence 1: K(p) = 0 .. D - 1 at every pixel (D <= r + 1 with any prior in 1 .. D; D = 2r + 1 with the prior
    r + 1 everywhere): web, best and sub are sm_sgm_wta's"""
    for radius in (1, 2, 3, 4):
        for d, kind in [(k, "noise1") for k in range(1, radius + 2)] + [(2 * radius + 1, "centre")]:
            left, right = rand_gray(17, 9, 7 * d + radius, 4)
            prior = sp.make_prior(kind, 17, 9, d, radius, np.random.default_rng(d))
            want = sg.sgm(left, right, d, 3, 7, 9, 70, paths, mode)
            assert same(sn.sgm_near(left, right, prior, d, 3, 7, 9, 70, paths, radius, mode), want), (radius, d)


@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
@pytest.mark.parametrize("kind", PRIOR_KINDS)
def test_without_penalties_it_is_the_census_re_search(mode, kind):
    """consequence 2: p1 = p2 = 0 gives sm_census_wta_near's web and paths times its best"""
    w, h, d = 21, 10, 33
    for radius, paths in ((1, 8), (2, 4), (4, 8)):
        left, right = rand_gray(w, h, radius, 4)
        prior = sp.make_prior(kind, w, h, d, radius, np.random.default_rng(radius))
        best, web, _ = sn.sgm_near(left, right, prior, d, 5, 5, 0, 0, paths, radius, mode)
        nbest, nweb = nr.near(left, right, prior, d, 5, 5, radius, mode)
        assert np.array_equal(web, nweb) and np.array_equal(best, paths * nbest)


def test_the_full_map_as_prior_gives_a_valid_result():
    """consequence 3 asserts no ordering (the penalties differ): every pixel gets a shift of its band"""
    left, right = rand_gray(30, 12, 3, 8)
    _, web, _ = sg.sgm(left, right, 20, 3, 7, 10, 120, 8, "ghost")
    for radius in (1, 2, 4):
        best, near, sub = sn.sgm_near(left, right, web, 20, 3, 7, 10, 120, 8, radius, "ghost")
        assert (near >= 1).all() and (near <= 20).all() and (np.abs(near - web) <= radius).all()
        assert (np.abs(sub.astype(int) - 16 * near) <= 8).all()


@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
def test_the_right_pass_written_out_is_the_mirrored_left_pass(mode):
    """the pass over right pixels u with L's paths in the right image's own coordinates, cost popcount(C_R(u) ^
    C_L(u - d)), equals mirror(sgm_near(mirror(R), mirror(L), mirror(prior_right))): mirroring maps the direction set
    onto itself"""
    from tests.census_reference import transform
    from tests.cost_lr_reference import _box
    w, h, d, sw, census, radius = 19, 8, 14, 3, 7, 2
    left, right = rand_gray(w, h, 5, 4)
    prior_right = sp.make_prior("noise", w, h, d, radius, np.random.default_rng(1))
    cl, cr = transform(left, census, mode), transform(right, census, mode)
    ink = sn.band(prior_right, d, radius)
    a = np.zeros(ink.shape, np.int64)
    for k in range(d):
        if mode == "toroidal":
            other = np.roll(cl, k, axis=1)                  # other(u) = C_L((u - k) mod W)
        else:
            other = np.zeros_like(cl)
            other[:, k:] = cl[:, :w - k]
        a[..., k] = np.where(ink[..., k], _box(np.bitwise_count(cr ^ other).astype(np.int64), 2 * (sw // 2) + 1, mode), 0)
    for paths in (4, 8):
        best, web, _ = sn.winner(sn.aggregate(a, ink, 12, 90, paths), ink)
        want = sn.sgm_near_right(left, right, prior_right, d, sw, census, 12, 90, paths, radius, mode)
        assert np.array_equal(best, want[0]) and np.array_equal(web, want[1])


def test_a_monotone_intensity_change_alters_nothing():
    left, right = rand_gray(23, 11, 8, 64)
    prior = sp.make_prior("noise", 23, 11, 16, 2, np.random.default_rng(2))
    lut = np.sort(np.random.default_rng(3).choice(256, 64, replace=False)).astype(np.uint8)
    a = sn.sgm_near(left, right, prior, 16, 3, 5, 10, 120, 8, 2, "ghost")
    b = sn.sgm_near(lut[left], lut[right], prior, 16, 3, 5, 10, 120, 8, 2, "ghost")
    assert same(a, b)


@pytest.mark.parametrize("mutant", sp.MUTANTS)
def test_the_cases_tell_every_mutant_from_the_definition(mutant):
    name = sp.MUTANT_CASE[mutant]
    c = sp.BY_NAME[name]
    left, right, prior, prior_right = sp.inputs(name)
    e = sp.expected(name)[0]
    if mutant == "prior_not_mirrored":
        got = sp.mutant_sgm_near_right(left[0], right[0], prior_right[0], *sp.args(c))
        assert not (np.array_equal(got[0], e["best_right"]) and np.array_equal(got[1], e["web_right"]))
    else:
        got = sp.mutant_sgm_near(left[0], right[0], prior[0], *sp.args(c), mutant)
        assert not same(got, (e["best"], e["web"], e["sub"]))


def test_the_mutant_machinery_without_a_mistake_is_the_definition():
    """mutant_sgm_near differs from sgm_near by its mistake alone: where the mistake cannot show (last_wins on random
    256-level images without ties; no_clip on a prior whose bands stay inside 0 .. D - 1) it is the definition"""
    left, right = rand_gray(20, 9, 5)
    rng = np.random.default_rng(6)
    prior = rng.integers(5, 12, (9, 20)).astype(np.int32)
    want = sn.sgm_near(left, right, prior, 16, 3, 7, 10, 120, 8, 2, "toroidal")
    for kind in ("no_clip_lo", "no_clip_hi", "m_clipped", "no_restart", "last_wins"):
        assert same(sp.mutant_sgm_near(left, right, prior, 16, 3, 7, 10, 120, 8, 2, "toroidal", kind), want), kind


def test_case_list_covers_every_factor():
    cs = sp.CASES
    assert 80 <= len(cs) <= 110
    sizes = {(c["w"], c["h"]) for c in cs}
    assert {(w, h) for w in sp.SIZES for h in sp.SIZES} <= sizes and (129, 5) in sizes
    assert {(13, 12), (12, 13), (13, 13)} <= sizes         # lines of the prefetch depth and one longer
    for key, values in (("sw", sp.WINDOWS), ("d", sp.SHIFTS), ("census", sp.CENSUS), ("radius", sp.RADII),
                        ("mode", sp.MODES), ("prior", sp.PRIORS), ("pairs", [1, 2, 3]), ("paths", [4, 8])):
        assert set(values) <= {c[key] for c in cs}, key
    assert any(c["d"] > c["w"] for c in cs) and any(c["p1"] == c["p2"] > 0 for c in cs)
    assert any(c["p1"] == 0 < c["p2"] for c in cs)
    # jumps of exactly 2r - 1 .. 2r + 2 between horizontal neighbours, at every radius
    for r in sp.RADII:
        seen = set()
        for mode in sp.MODES:
            prior = sp.inputs(f"jumps {mode} r={r}")[2][0].astype(np.int64)
            seen |= set(np.abs(np.diff(prior, axis=1)).ravel().tolist()) | set(np.abs(np.diff(prior, axis=0)).ravel().tolist())
        assert {2 * r - 1, 2 * r, 2 * r + 1, 2 * r + 2} <= seen, (r, sorted(seen))


def test_the_extremes_say_what_they_are_meant_to():
    """a constant gray pair: the data term is 0 at every pixel and shift, so the maps are those of the penalties alone
    (a shift that the neighbours' bands hold as well wins; best <= paths * p2); the lattice of the census extremes:
    L_r = 62767 in all eight directions and S = 8 * 62767 at the lattice's interior pixels"""
    for name in ("all tie toroidal", "all tie ghost"):
        c = sp.BY_NAME[name]
        prior = sp.inputs(name)[2][0]
        e = sp.expected(name)[0]
        ink = sn.band(prior, c["d"], c["radius"])
        want = sn.winner(sn.aggregate(np.zeros(ink.shape, np.int64), ink, c["p1"], c["p2"], c["paths"]), ink)
        assert same(want, (e["best"], e["web"], e["sub"]))
        assert 0 < e["best"].max() <= c["paths"] * c["p2"]
    c = sp.BY_NAME["maximum cost"]
    prior = sp.inputs("maximum cost")[2][0]
    e = sp.expected("maximum cost")[0]
    peak = prior == c["d"] + c["radius"]
    peak[[0, -1], :] = False
    peak[:, [0, -1]] = False
    assert peak.sum() > 100 and (e["best"][peak] == 8 * 62767).all() and (e["web"][peak] == c["d"]).all()
    assert e["best"].max() == 8 * 62767


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_what_it_is_for(seed):
    """96 x 40, D = 24, window 5, census 7, ghost, p1 = 100, p2 = 1200, r = 1: a depth step (shift 9 | 21) with a
    textureless band of 12 rows across it; the prior is the even shift below the truth.  Region: the band's 900 pixels
    whose match lies inside the right image.  The census re-search has three tying candidates there and is right at
    734 / 726 / 732 / 735 of them (seeds 0 .. 3); banded SGM carries the textured rows' answer across the band and is
    right at 865 / 852 / 863 / 865"""
    left, right, truth, prior, region = sp.band_scene(seed)
    assert region.sum() == 900
    _, web, _ = sn.sgm_near(left, right, prior, 24, 5, 7, 100, 1200, 8, 1, "ghost")
    _, census = nr.near(left, right, prior, 24, 5, 7, 1, "ghost")
    good, before = int((web == truth)[region].sum()), int((census == truth)[region].sum())
    assert (good, before) == ((865, 734), (852, 726), (863, 732), (865, 735))[seed]
    assert good > before
