"""Left-right consistency check, CPU side: the C ABI declares and exports the new entries and refuses bad
arguments before it touches a device; the mirror identity that defines the right-reference map holds against
a direct restatement; the check's definition on hand-built maps."""
import ctypes as C

import numpy as np
import pytest

from tests import lr_reference as lr
from tests import oracle

NEW = ("sm_match_wta_right", "sm_lr_check", "sm_run_lr", "sm_plan_reserve_lr")


def test_new_symbols_are_declared_bound_and_exported():
    from stereomatching_amd import capi
    syms = capi.declared_symbols()
    for s in NEW:
        assert s in syms and s in capi._SIGNATURES and hasattr(capi.lib, s), s


def test_argument_checks_precede_device_use():
    from stereomatching_amd import capi
    lib = capi.lib
    px = C.c_void_p(16)           # never dereferenced: every call below is refused first

    def refused(rc, text):
        assert rc == capi.SM_ERR_ARG
        assert text in lib.sm_last_error(), lib.sm_last_error()

    refused(lib.sm_plan_reserve_lr(None), b"plan is NULL")
    refused(lib.sm_match_wta_right(None, 1, px, None, None), b"plan is NULL")
    refused(lib.sm_match_wta_right(None, 1, None, None, None), b"d_web_right is NULL")
    refused(lib.sm_lr_check(None, px, px, 0, 1, px, None, None), b"plan is NULL")
    refused(lib.sm_lr_check(None, px, px, -1, 1, px, None, None), b"max_diff -1 is negative")
    refused(lib.sm_lr_check(None, None, px, 0, 1, px, None, None), b"NULL")
    refused(lib.sm_lr_check(None, px, None, 0, 1, px, None, None), b"NULL")
    refused(lib.sm_lr_check(None, px, px, 0, 1, None, None, None), b"NULL")
    refused(lib.sm_run_lr(None, px, px, 0.15, 1, 0, px, None, None, None, None), b"plan is NULL")
    refused(lib.sm_run_lr(None, px, px, 0.15, 1, -2, px, None, None, None, None), b"max_diff -2 is negative")
    refused(lib.sm_run_lr(None, None, px, 0.15, 1, 0, px, None, None, None, None), b"input image pointer is NULL")
    refused(lib.sm_run_lr(None, px, px, 1.5, 1, 0, px, None, None, None, None), b"threshold must be between 0 and 1")
    refused(lib.sm_run_lr(None, px, px, 0.15, 1, 0, None, None, None, None, None), b"d_web is NULL")


def rand_edges(w, h, seed, density=0.5):
    rng = np.random.default_rng(seed)
    return ((rng.random((h, w)) < density).astype(np.uint8),
            (rng.random((h, w)) < density).astype(np.uint8))


@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
@pytest.mark.parametrize("w,h,d,sw", [(40, 23, 12, 5), (33, 17, 45, 3), (31, 21, 7, 0), (17, 9, 9, 1),
                                      (29, 30, 16, 9), (12, 11, 30, 7),
                                      # the shapes the GPU sweeps reach (tests/test_lr_sweep_gpu.py): widths 1 to 9,
                                      # D >= 3W, and the generic kernel's windows 27 and 31
                                      (1, 6, 3, 0), (1, 4, 5, 1), (2, 5, 6, 1), (3, 7, 9, 3), (4, 3, 12, 3),
                                      (5, 9, 15, 5), (6, 8, 19, 4), (7, 7, 21, 7), (8, 11, 24, 7), (9, 9, 27, 9),
                                      (9, 4, 40, 3), (16, 12, 48, 11), (23, 5, 70, 5), (40, 27, 30, 27),
                                      (27, 29, 81, 27), (31, 33, 93, 31)])
def test_mirror_identity_equals_the_right_reference_definition(mode, w, h, d, sw):
    """mirror(hot_path(mirror(eR), mirror(eL))) is the right-reference match written out -- widths from one
    column, odd widths, more shifts than columns (up to 3W and more), windows of one pixel (S = 0 and 1) up to
    the whole image (27 and 31) -- for both borders"""
    for seed, dens in ((1, 0.5), (2, 0.15)):
        el, er = rand_edges(w, h, seed + 10 * w, dens)
        ob, ow = lr.right_reference(el, er, d, sw, mode)
        bb, bw = lr.right_reference_bruteforce(el, er, d, sw, mode)
        assert np.array_equal(ow, bw), (mode, w, h, d, sw, seed)
        assert np.array_equal(ob, bb), (mode, w, h, d, sw, seed)
        # a pixel whose neighbourhood holds no edge at all matches every shift: the last one, D, wins
        z = np.zeros((h, w), np.uint8)
        assert (lr.right_reference(z, z, d, sw, mode)[1] == d).all()


def test_right_reference_of_a_shifted_pair_points_back():
    """the right image is the left one moved by 5 columns: both directions find the shift, and the check
    keeps every pixel of the textured image (toroidal)"""
    rng = np.random.default_rng(4)
    el = (rng.random((24, 64)) < 0.5).astype(np.uint8)
    er = np.roll(el, 5, axis=1)                  # eR(u) = eL(u - 5): left pixel x matches right pixel x + 5
    _, web = oracle.hot_path(el, er, 8, 5, "toroidal")
    _, web_right = lr.right_reference(el, er, 8, 5, "toroidal")
    assert (web == 6).all() and (web_right == 6).all()
    checked, rejected = lr.lr_check(web, web_right, 0, "toroidal")
    assert rejected == 0 and np.array_equal(checked, web)


def test_check_definition_on_hand_built_maps():
    w = 8
    # ghost: x = 6 with s = 3 matched u = 8, the halo -> rejected whatever the right map says
    web = np.array([[1, 1, 1, 1, 1, 1, 3, 1]], np.int32)
    wr = np.ones((1, w), np.int32)
    wr[0, 0] = 3
    out, rej = lr.lr_check(web, wr, 8, "ghost")
    assert out[0, 6] == 0 and rej == 1 and (np.delete(out[0], 6) == 1).all()
    # toroidal: the same pixel wraps round to u = 0, where the right map says 3 -> kept (and x = 0, s = 1,
    # which matched u = 0 as well, is not)
    out, rej = lr.lr_check(web, wr, 0, "toroidal")
    assert out[0, 6] == 3 and out[0, 0] == 0 and rej == 1
    # tolerance: right map off by one at u = 2 (x = 2, s = 1)
    wr2 = wr.copy()
    wr2[0, 0] = 1
    wr2[0, 2] = 2
    web2 = np.ones((1, w), np.int32)
    out, rej = lr.lr_check(web2, wr2, 0, "toroidal")
    assert out[0, 2] == 0 and rej == 1
    out, rej = lr.lr_check(web2, wr2, 1, "toroidal")
    assert rej == 0 and np.array_equal(out, web2)
    # max_diff = D keeps every pixel whose match lands in the image
    D = 4
    rng = np.random.default_rng(3)
    webr = rng.integers(1, D + 1, (5, 13)).astype(np.int32)
    wrr = rng.integers(1, D + 1, (5, 13)).astype(np.int32)
    out, rej = lr.lr_check(webr, wrr, D, "toroidal")
    assert rej == 0 and np.array_equal(out, webr)
    out, rej = lr.lr_check(webr, wrr, D, "ghost")
    past = np.arange(13)[None, :] + webr - 1 >= 13
    assert rej == past.sum() and (out[past] == 0).all() and np.array_equal(out[~past], webr[~past])
    # and max_diff = 0 keeps exactly the pixels whose partner agrees
    out, rej = lr.lr_check(webr, wrr, 0, "toroidal")
    u = (np.arange(13)[None, :] + webr - 1) % 13
    agree = np.take_along_axis(wrr, u, axis=1) == webr
    assert rej == (~agree).sum() and np.array_equal(out, np.where(agree, webr, 0))


def test_wide_differences_tell_a_32_bit_subtraction_and_the_older_maps_do_not():
    """(the mutation audit's L2: a check that takes web_right(u) - web(x) modulo 2^32 passed tests/test_lr_gpu.py)"""
    from tests import lr_patterns as lp
    mistake = lp.MISTAKES[0]
    for w in (8, 7):
        web, right = lp.wide_difference_maps(w)
        for max_diff, mode in lp.WIDE_CHECKS:
            want, nrej = lr.lr_check(web, right, max_diff, mode)
            got, nmis = lp.lr_check_with(web, right, max_diff, mode, mistake)
            assert not np.array_equal(want, got) and nrej > nmis, (w, max_diff, mode)       # the mistake keeps too many
            assert (want[got != want] == 0).all()
        # both outcomes occur, so a check that rejects everything fails as well
        want, nrej = lr.lr_check(web, right, 2, "toroidal")
        assert 0 < nrej < web.size
    # the maps of test_check_of_values_no_match_produces (every int32 extreme among them) cannot tell
    w, h = 37, 5
    rng = np.random.default_rng(9)
    web = rng.integers(-3 * w, 3 * w, (h, w)).astype(np.int32)
    web[0, :4] = [0, -1, 2**31 - 1, -2**31]
    right = rng.integers(-3 * w, 3 * w, (h, w)).astype(np.int32)
    for mode in ("toroidal", "ghost"):
        a, b = lr.lr_check(web, right, 2, mode), lp.lr_check_with(web, right, 2, mode, mistake)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1], mode
    # nor maps of shifts 1 .. D, whatever max_diff (test_check_against_the_definition)
    web = rng.integers(1, 201, (9, 128)).astype(np.int32)
    right = rng.integers(1, 201, (9, 128)).astype(np.int32)
    for mode in ("toroidal", "ghost"):
        for max_diff in (0, 1, 3, 1000):
            a, b = lr.lr_check(web, right, max_diff, mode), lp.lr_check_with(web, right, max_diff, mode, mistake)
            assert np.array_equal(a[0], b[0]) and a[1] == b[1], (mode, max_diff)
