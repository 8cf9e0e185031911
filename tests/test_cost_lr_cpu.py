"""Left-right consistency check of the SAD / SSD cost mode, CPU side: the C ABI declares and exports the new entries
and refuses bad arguments before it touches a device; the mirror identity that defines the cost mode's
right-reference map holds against a direct restatement; a shifted textured pair points back to itself."""
import ctypes as C

import numpy as np
import pytest

from tests import cost_lr_reference as clr
from tests import oracle

NEW = ("sm_cost_wta_right", "sm_cost_lr", "sm_plan_reserve_cost_lr")


def test_new_symbols_are_declared_bound_and_exported():
    from stereomatching_amd import capi
    syms = capi.declared_symbols()
    for s in NEW:
        assert s in syms and s in capi._SIGNATURES and hasattr(capi.lib, s), s


def test_argument_checks_precede_device_use():
    """every check that needs no plan, on a NULL plan (the ones that read the plan's geometry -- pairs, overlaps,
    window and shift limits -- are covered on a real plan in tests/test_cost_lr_gpu.py)"""
    from stereomatching_amd import capi
    lib = capi.lib
    px = C.c_void_p(16)           # never dereferenced: every call below is refused first
    sad, ssd = 1, 2

    def refused(rc, text):
        assert rc == capi.SM_ERR_ARG
        assert text in lib.sm_last_error(), lib.sm_last_error()

    refused(lib.sm_plan_reserve_cost_lr(None), b"plan is NULL")
    refused(lib.sm_cost_wta_right(None, px, px, sad, 1, px, None, None), b"sm_cost_wta_right: plan is NULL")
    refused(lib.sm_cost_wta_right(None, px, px, ssd, 1, px, px, None), b"plan is NULL")
    refused(lib.sm_cost_wta_right(None, None, px, sad, 1, px, None, None), b"input image pointer is NULL")
    refused(lib.sm_cost_wta_right(None, px, None, sad, 1, px, None, None), b"input image pointer is NULL")
    refused(lib.sm_cost_wta_right(None, px, px, sad, 1, None, None, None), b"d_web_right is NULL")
    refused(lib.sm_cost_wta_right(None, px, px, 3, 1, px, None, None), b"cost 3 is neither SM_COST_SAD nor SM_COST_SSD")
    refused(lib.sm_cost_wta_right(None, px, px, 0, 1, px, None, None), b"cost 0 is neither")
    refused(lib.sm_cost_lr(None, px, px, sad, 1, 0, px, None, None, None, None), b"sm_cost_lr: plan is NULL")
    refused(lib.sm_cost_lr(None, None, px, sad, 1, 0, px, None, None, None, None), b"input image pointer is NULL")
    refused(lib.sm_cost_lr(None, px, None, sad, 1, 0, px, None, None, None, None), b"input image pointer is NULL")
    refused(lib.sm_cost_lr(None, px, px, sad, 1, 0, None, px, px, px, None), b"d_web is NULL")
    refused(lib.sm_cost_lr(None, px, px, sad, 1, -1, px, None, None, None, None), b"max_diff -1 is negative")
    refused(lib.sm_cost_lr(None, px, px, 7, 1, 0, px, None, None, None, None), b"cost 7 is neither")


def rand_gray(w, h, seed, levels=256):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, levels, (h, w)).astype(np.uint8), rng.integers(0, levels, (h, w)).astype(np.uint8))


@pytest.mark.parametrize("cost", ["sad", "ssd"])
@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
@pytest.mark.parametrize("w,h,d,sw", [(40, 23, 12, 5), (33, 17, 45, 3), (31, 21, 7, 0), (17, 9, 9, 1),
                                      (29, 30, 16, 9), (12, 11, 30, 7),
                                      # n = 1, W < n (an even square_width equal to W: n = W + 1), D >= W (up to 3W
                                      # and more), W % 4 != 0, the widest windows; every shape one a plan accepts
                                      # (square_width <= W, H)
                                      (1, 6, 3, 0), (2, 5, 6, 1), (3, 7, 9, 3), (4, 3, 12, 3), (5, 9, 15, 5),
                                      (6, 8, 19, 6), (7, 7, 21, 7), (9, 4, 40, 3), (10, 26, 33, 10),
                                      (23, 25, 70, 23), (30, 27, 20, 25), (26, 30, 300, 25)])
def test_mirror_identity_equals_the_right_reference_definition(cost, mode, w, h, d, sw):
    """mirror(cost_hot_path(mirror(R), mirror(L))) is the right-reference cost match written out"""
    for seed, levels in ((1, 256), (2, 3)):              # (few grey levels: many ties, so first-wins is exercised)
        left, right = rand_gray(w, h, seed + 10 * w, levels)
        ob, ow = clr.right_reference(left, right, d, sw, mode, cost)
        bb, bw = clr.right_reference_bruteforce(left, right, d, sw, mode, cost)
        assert np.array_equal(ow, bw), (cost, mode, w, h, d, sw, seed)
        assert np.array_equal(ob, bb), (cost, mode, w, h, d, sw, seed)
    # equal images of one grey value: every shift costs 0 (toroidal), and the first one wins
    z = np.full((h, w), 77, np.uint8)
    if mode == "toroidal":
        assert (clr.right_reference(z, z, d, sw, mode, cost)[1] == 1).all()


def test_left_restatement_agrees_with_the_oracle():
    """the left direction of the same restatement (R(x + d) read for left pixel x) is the oracle's cost mode: the
    restatement and the oracle share their conventions"""
    for mode in ("toroidal", "ghost"):
        for cost in ("sad", "ssd"):
            left, right = rand_gray(21, 13, 5, 7)
            want = oracle.cost_hot_path(left, right, 11, 5, mode, cost)
            # left pixel x against right x + d is the right-reference match of the mirrored pair
            got = clr.right_reference_bruteforce(clr.mirror(right), clr.mirror(left), 11, 5, mode, cost)
            assert np.array_equal(clr.mirror(got[1]), want[1]) and np.array_equal(clr.mirror(got[0]), want[0])


@pytest.mark.parametrize("cost", ["sad", "ssd"])
def test_shifted_textured_pair_points_back(cost):
    """the right image is the left one moved by 5 columns: both directions find the shift, and the check keeps
    every interior pixel at max_diff = 0; with the ghost border the columns that matched into the halo are
    rejected"""
    rng = np.random.default_rng(4)
    w, h, d, sw, s = 64, 24, 12, 5, 5
    left = rng.integers(0, 256, (h, w)).astype(np.uint8)
    half = sw // 2
    # toroidal: R(u) = L(u - 5) everywhere
    right = np.roll(left, s, axis=1)
    e = clr.expected(left, right, d, sw, "toroidal", cost, 0)
    assert (e["web"] == s + 1).all() and (e["web_right"] == s + 1).all()
    assert e["rejected"] == 0 and np.array_equal(e["checked"], e["web"])
    # ghost: the same inside the image, fresh texture in the columns the shift uncovers
    right = np.concatenate([rng.integers(0, 256, (h, s)).astype(np.uint8), left[:, :w - s]], axis=1)
    e = clr.expected(left, right, d, sw, "ghost", cost, 0)
    interior = np.zeros((h, w), bool)
    interior[:, half:w - s - half] = True              # the window of x and of its partner x + 5 inside the image
    assert (e["web"][interior] == s + 1).all()
    assert (e["checked"][interior] == s + 1).all()
    u = np.arange(w)[None, :] + e["web"] - 1
    halo = u >= w
    assert halo.any(), "no column matched into the halo: the pattern no longer covers the rule"
    assert (e["checked"][halo] == 0).all()
    assert e["rejected"] == int((e["checked"] == 0).sum()) >= int(halo.sum())
