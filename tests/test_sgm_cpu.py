"""SGM over the census data term, CPU side: the C ABI declares, binds and exports the new entries and refuses bad
arguments before it touches a device; the vectorised numpy definition (tests/sgm_reference.py) agrees with a
path-by-path restatement; the identities the GPU tests lean on hold (zero penalties give the census arg-min, the
right reference is the mirror of the left pass, a strictly increasing intensity map changes nothing)."""
import ctypes as C

import numpy as np
import pytest

from tests import census_reference as cr
from tests import sgm_reference as sr

NEW = ("sm_sgm_wta", "sm_sgm_wta_right", "sm_sgm_lr", "sm_plan_reserve_sgm")


def test_new_symbols_are_declared_bound_and_exported():
    from stereomatching_amd import capi
    syms = capi.declared_symbols()
    for s in NEW:
        assert s in syms and s in capi._SIGNATURES and hasattr(capi.lib, s), s


def test_argument_checks_precede_device_use():
    """every check that needs no plan, on a NULL plan: census width, paths and penalties are refused even so (pairs,
    overlaps, window and shift limits read the plan: tests/test_sgm_gpu.py covers them on a real one)"""
    from stereomatching_amd import capi
    lib = capi.lib
    px = C.c_void_p(16)           # never dereferenced: every call below is refused first

    def refused(rc, text):
        assert rc == capi.SM_ERR_ARG
        assert text in lib.sm_last_error(), lib.sm_last_error()

    refused(lib.sm_plan_reserve_sgm(None), b"sm_plan_reserve_sgm: plan is NULL")
    # sm_sgm_wta
    refused(lib.sm_sgm_wta(None, px, px, 7, 10, 120, 8, 1, px, None, None, None), b"sm_sgm_wta: plan is NULL")
    refused(lib.sm_sgm_wta(None, None, px, 7, 10, 120, 8, 1, px, None, None, None),
            b"sm_sgm_wta: input image pointer is NULL")
    refused(lib.sm_sgm_wta(None, px, px, 7, 10, 120, 8, 1, None, px, px, None), b"sm_sgm_wta: d_web is NULL")
    refused(lib.sm_sgm_wta(None, px, px, 9, 10, 120, 8, 1, px, None, None, None),
            b"sm_sgm_wta: census_width 9 is not 3, 5 or 7")
    for paths in (0, 2, 6, 16, -4):
        refused(lib.sm_sgm_wta(None, px, px, 5, 10, 120, paths, 1, px, None, None, None),
                b"sm_sgm_wta: paths %d is not 4 or 8" % paths)
    for p1, p2 in ((-1, 10), (11, 10), (0, 32768), (40000, 40000), (5, -1)):
        refused(lib.sm_sgm_wta(None, px, px, 3, p1, p2, 4, 1, px, None, None, None),
                b"sm_sgm_wta: penalties p1 %d, p2 %d break 0 <= p1 <= p2 <= 32767" % (p1, p2))
    # sm_sgm_wta_right
    refused(lib.sm_sgm_wta_right(None, px, px, 7, 10, 120, 8, 1, px, None, None), b"sm_sgm_wta_right: plan is NULL")
    refused(lib.sm_sgm_wta_right(None, px, None, 7, 10, 120, 8, 1, px, None, None),
            b"sm_sgm_wta_right: input image pointer is NULL")
    refused(lib.sm_sgm_wta_right(None, px, px, 7, 10, 120, 8, 1, None, None, None),
            b"sm_sgm_wta_right: d_web_right is NULL")
    refused(lib.sm_sgm_wta_right(None, px, px, 7, 10, 120, 5, 1, px, None, None), b"sm_sgm_wta_right: paths 5 is not")
    refused(lib.sm_sgm_wta_right(None, px, px, 7, 121, 120, 8, 1, px, None, None),
            b"sm_sgm_wta_right: penalties p1 121, p2 120 break")
    refused(lib.sm_sgm_wta_right(None, px, px, 4, 10, 120, 8, 1, px, None, None),
            b"sm_sgm_wta_right: census_width 4 is not 3, 5 or 7")
    # sm_sgm_lr
    refused(lib.sm_sgm_lr(None, px, px, 7, 10, 120, 8, 1, 0, px, None, None, None, None, None),
            b"sm_sgm_lr: plan is NULL")
    refused(lib.sm_sgm_lr(None, None, px, 7, 10, 120, 8, 1, 0, px, None, None, None, None, None),
            b"sm_sgm_lr: input image pointer is NULL")
    refused(lib.sm_sgm_lr(None, px, px, 7, 10, 120, 8, 1, 0, None, px, px, px, px, None), b"sm_sgm_lr: d_web is NULL")
    refused(lib.sm_sgm_lr(None, px, px, 7, 10, 120, 8, 1, -1, px, None, None, None, None, None),
            b"sm_sgm_lr: max_diff -1 is negative")
    refused(lib.sm_sgm_lr(None, px, px, 7, 10, 120, 3, 1, 0, px, None, None, None, None, None),
            b"sm_sgm_lr: paths 3 is not 4 or 8")
    refused(lib.sm_sgm_lr(None, px, px, 7, 10, 32768, 8, 1, 0, px, None, None, None, None, None),
            b"sm_sgm_lr: penalties p1 10, p2 32768 break")
    refused(lib.sm_sgm_lr(None, px, px, 2, 10, 120, 8, 1, 0, px, None, None, None, None, None),
            b"sm_sgm_lr: census_width 2 is not 3, 5 or 7")


def rand_gray(w, h, seed, levels=256):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, levels, (h, w)).astype(np.uint8), rng.integers(0, levels, (h, w)).astype(np.uint8))


# (w, h, D, square_width, p1, p2): W < c, H < c, D = 1, D > W, P2 = P1, zero penalties
CASES = [(6, 5, 4, 1, 3, 20), (5, 4, 3, 3, 7, 7), (2, 6, 4, 1, 1, 9), (7, 2, 1, 3, 4, 30), (4, 3, 7, 1, 2, 11),
         (3, 3, 5, 3, 0, 0), (8, 5, 3, 1, 20, 40)]


@pytest.mark.parametrize("census", [3, 5, 7])
@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("w,h,d,sw,p1,p2", CASES)
def test_numpy_definition_equals_the_path_loop(census, mode, paths, w, h, d, sw, p1, p2):
    for seed, levels in ((1, 256), (2, 3)):                 # few grey levels: ties in the minima and the arg-min
        left, right = rand_gray(w, h, seed + 11 * w + census + paths, levels)
        a = sr.data_term(left, right, d, sw, census, mode)
        assert np.array_equal(a, sr.data_term_bruteforce(left, right, d, sw, census, mode))
        want = sr.sgm_bruteforce(left, right, d, sw, census, p1, p2, paths, mode)
        got = sr.sgm(left, right, d, sw, census, p1, p2, paths, mode)
        tag = (census, mode, paths, w, h, d, sw, p1, p2, seed)
        for g, e, name in zip(got, want, ("best", "web", "sub")):
            assert g.dtype == e.dtype and np.array_equal(g, e), (name, tag)


@pytest.mark.parametrize("census", [3, 7])
@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
@pytest.mark.parametrize("paths", [4, 8])
def test_zero_penalties_give_the_census_arg_min(census, mode, paths):
    w, h, d, sw = 17, 9, 11, 3
    left, right = rand_gray(w, h, 5 * census + paths, 256)
    best, web, _ = sr.sgm(left, right, d, sw, census, 0, 0, paths, mode)
    cbest, cweb = cr.wta(left, right, d, sw, census, mode)
    assert np.array_equal(web, cweb)
    assert np.array_equal(best, paths * cbest)


@pytest.mark.parametrize("census", [3, 5, 7])
@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
def test_right_reference_is_the_left_pass_on_the_mirrored_data_term(census, mode):
    """the right-reference data term is the mirrored one of the swapped images, and the direction sets are closed under
    horizontal mirroring: aggregating the mirrored volume gives the definition's maps"""
    w, h, d, sw, p1, p2 = 14, 8, 9, 3, 6, 50
    left, right = rand_gray(w, h, 9 * census, 256)
    a = sr.data_term(sr.mirror(right), sr.mirror(left), d, sw, census, mode)
    for paths in (4, 8):
        assert sorted((-dx, dy) for dx, dy in sr.DIRS[paths]) == sorted(sr.DIRS[paths])
        best, web, _ = sr.winner(sr.aggregate(a, p1, p2, paths))
        want = sr.right_reference(left, right, d, sw, census, p1, p2, paths, mode)
        assert np.array_equal(sr.mirror(best), want[0]) and np.array_equal(sr.mirror(web), want[1])
        # mirroring the volume and the directions together changes nothing
        m = a[:, ::-1]
        s1 = sr.aggregate(np.ascontiguousarray(m), p1, p2, paths)
        assert np.array_equal(s1[:, ::-1], sr.aggregate(a, p1, p2, paths))


@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
def test_intensity_invariance_and_constant_images(mode):
    w, h, d, sw = 20, 10, 8, 3
    left, right = (1 + x for x in rand_gray(w, h, 31, 127))            # 1 .. 127: ghost halo pixels stay darker
    l2 = (2 * left.astype(np.int32) + 1).astype(np.uint8)
    r2 = (2 * right.astype(np.int32)).astype(np.uint8)
    a = sr.expected(left, right, d, sw, 5, 8, 90, 8, mode, 1)
    b = sr.expected(l2, r2, d, sw, 5, 8, 90, 8, mode, 1)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    z = np.full((h, w), 77, np.uint8)
    best, web, sub = sr.sgm(z, z, d, sw, 7, 10, 120, 4, mode)
    assert (web == 1).all() and (sub == 16).all() and (best == 0).all()


def test_u16_bound():
    """A <= L_r <= A + P2: at the largest window cost and penalty every L_r fits a u16"""
    rng = np.random.default_rng(4)
    a = rng.integers(0, 30001, (6, 7, 5)).astype(np.int32)
    for dx, dy in sr.DIRS[8]:
        L = sr.path(a, dx, dy, 0, 32767)
        assert (L >= a).all() and (L <= a + 32767).all() and L.max() <= 62767
