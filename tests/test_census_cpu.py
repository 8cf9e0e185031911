"""Census cost mode, CPU side: the C ABI declares, binds and exports the new entries and refuses bad arguments before
it touches a device; the numpy definition (tests/census_reference.py) agrees with a pixel-by-pixel restatement; the
mirror identity the right-reference pass relies on holds; a strictly increasing intensity map changes nothing."""
import ctypes as C

import numpy as np
import pytest

from tests import census_reference as cr

NEW = ("sm_census_transform", "sm_census_wta", "sm_census_wta_right", "sm_census_lr", "sm_census_refine",
       "sm_plan_reserve_census")


def test_new_symbols_are_declared_bound_and_exported():
    from stereomatching_amd import capi
    syms = capi.declared_symbols()
    for s in NEW:
        assert s in syms and s in capi._SIGNATURES and hasattr(capi.lib, s), s


def test_argument_checks_precede_device_use():
    """every check that needs no plan, on a NULL plan (pairs, images, overlaps and the window and shift limits read
    the plan: tests/test_census_gpu.py covers them on a real one)"""
    from stereomatching_amd import capi
    lib = capi.lib
    px = C.c_void_p(16)           # never dereferenced: every call below is refused first

    def refused(rc, text):
        assert rc == capi.SM_ERR_ARG
        assert text in lib.sm_last_error(), lib.sm_last_error()

    refused(lib.sm_plan_reserve_census(None), b"sm_plan_reserve_census: plan is NULL")
    # sm_census_transform
    refused(lib.sm_census_transform(None, px, 7, 1, px, None), b"sm_census_transform: plan is NULL")
    refused(lib.sm_census_transform(None, None, 7, 1, px, None), b"sm_census_transform: NULL argument")
    refused(lib.sm_census_transform(None, px, 7, 1, None, None), b"sm_census_transform: NULL argument")
    refused(lib.sm_census_transform(None, px, 4, 1, px, None), b"sm_census_transform: census_width 4 is not 3, 5 or 7")
    # sm_census_wta
    refused(lib.sm_census_wta(None, px, px, 7, 1, px, None, None), b"sm_census_wta: plan is NULL")
    refused(lib.sm_census_wta(None, None, px, 7, 1, px, None, None), b"sm_census_wta: input image pointer is NULL")
    refused(lib.sm_census_wta(None, px, None, 3, 1, px, px, None), b"sm_census_wta: input image pointer is NULL")
    refused(lib.sm_census_wta(None, px, px, 5, 1, None, px, None), b"sm_census_wta: d_web is NULL")
    refused(lib.sm_census_wta(None, px, px, 9, 1, px, None, None), b"sm_census_wta: census_width 9 is not 3, 5 or 7")
    refused(lib.sm_census_wta(None, px, px, 1, 1, px, None, None), b"census_width 1 is not")
    # sm_census_wta_right
    refused(lib.sm_census_wta_right(None, px, px, 7, 1, px, None, None), b"sm_census_wta_right: plan is NULL")
    refused(lib.sm_census_wta_right(None, None, px, 7, 1, px, None, None),
            b"sm_census_wta_right: input image pointer is NULL")
    refused(lib.sm_census_wta_right(None, px, px, 7, 1, None, None, None), b"sm_census_wta_right: d_web_right is NULL")
    refused(lib.sm_census_wta_right(None, px, px, 0, 1, px, None, None),
            b"sm_census_wta_right: census_width 0 is not 3, 5 or 7")
    # sm_census_lr
    refused(lib.sm_census_lr(None, px, px, 7, 1, 0, px, None, None, None, None), b"sm_census_lr: plan is NULL")
    refused(lib.sm_census_lr(None, px, None, 7, 1, 0, px, None, None, None, None),
            b"sm_census_lr: input image pointer is NULL")
    refused(lib.sm_census_lr(None, px, px, 7, 1, 0, None, px, px, px, None), b"sm_census_lr: d_web is NULL")
    refused(lib.sm_census_lr(None, px, px, 7, 1, -1, px, None, None, None, None), b"sm_census_lr: max_diff -1 is negative")
    refused(lib.sm_census_lr(None, px, px, 6, 1, 0, px, None, None, None, None),
            b"sm_census_lr: census_width 6 is not 3, 5 or 7")
    # sm_census_refine
    refused(lib.sm_census_refine(None, px, px, 7, 1, px, px, None, None), b"sm_census_refine: plan is NULL")
    for args in ((None, px, px, px), (px, None, px, px), (px, px, None, px), (px, px, px, None)):
        l, r, web, sub = args
        refused(lib.sm_census_refine(None, l, r, 7, 1, web, sub, None, None), b"sm_census_refine: NULL argument")
    refused(lib.sm_census_refine(None, px, px, 8, 1, px, px, None, None),
            b"sm_census_refine: census_width 8 is not 3, 5 or 7")


def rand_gray(w, h, seed, levels=256):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, levels, (h, w)).astype(np.uint8), rng.integers(0, levels, (h, w)).astype(np.uint8))


@pytest.mark.parametrize("census", [3, 5, 7])
@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
@pytest.mark.parametrize("w,h,d,sw", [(7, 5, 4, 3), (4, 3, 6, 1), (9, 6, 3, 5), (3, 2, 2, 1)])
def test_numpy_definition_equals_the_pixel_loop(census, mode, w, h, d, sw):
    """the vectorised transform and arg-min against a per-pixel loop, on tiny images (W < c, H < c among them)"""
    for seed, levels in ((1, 256), (2, 3)):              # (few grey levels: ties in the comparisons and the arg-min)
        left, right = rand_gray(w, h, seed + 7 * w + census, levels)
        assert np.array_equal(cr.transform(left, census, mode), cr.transform_bruteforce(left, census, mode))
        want = cr.wta_bruteforce(left, right, d, sw, census, mode)
        got = cr.wta(left, right, d, sw, census, mode)
        assert np.array_equal(got[1], want[1]), (census, mode, w, h, d, sw, seed)
        assert np.array_equal(got[0], want[0]), (census, mode, w, h, d, sw, seed)


@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
def test_descriptor_bits(mode):
    """bit k is the k-th neighbour in row-major order, the centre skipped; 8 / 24 / 48 bits; ghost halo reads 0"""
    img = np.zeros((9, 9), np.uint8)
    img[4, 4] = 100
    img[3, 3] = 200                      # the first neighbour of the 3 x 3 window of (4, 4) is brighter
    for c, nbits in ((3, 8), (5, 24), (7, 48)):
        d = cr.transform(img, c, mode)
        # the brighter pixel (-1, -1) is neighbour number (h - 1) * c + (h - 1) of the c x c window, h = c // 2
        hc = c // 2
        k = (hc - 1) * c + (hc - 1)
        want = ((1 << nbits) - 1) & ~(1 << k)
        assert int(d[4, 4]) == want, (c, hex(int(d[4, 4])))
        assert int(d.max()) < (1 << nbits)
    # a lone dark pixel at the corner: toroidal neighbours wrap round into the image (all brighter), ghost ones
    # outside read 0 (darker: bits (-1,-1) (-1,0) (-1,1) (0,-1) (1,-1) = 0, 1, 2, 3, 5)
    img = np.full((6, 6), 50, np.uint8)
    img[0, 0] = 10
    t = cr.transform(img, 3, mode)
    assert int(t[0, 0]) == (0 if mode == "toroidal" else 0b00101111)
    assert np.array_equal(t, cr.transform_bruteforce(img, 3, mode))


@pytest.mark.parametrize("census", [3, 5, 7])
@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
@pytest.mark.parametrize("w,h,d,sw", [(12, 9, 8, 3), (10, 7, 15, 5), (5, 4, 9, 1), (16, 11, 20, 9)])
def test_mirror_identity(census, mode, w, h, d, sw):
    """mirroring an image permutes the bits of every descriptor alike: the descriptors of mirror(I), read through the
    permutation, are the mirrored descriptors of I -- so the right-reference arg-min from the left pass's descriptors
    read in mirrored order is the definition's (the arg-min of the mirrored images)"""
    left, right = rand_gray(w, h, 3 * w + census, 256)
    c = census
    hc = c // 2
    # the permutation: neighbour (dx, dy) of mirror(I) is neighbour (-dx, dy) of I
    order = [(dx, dy) for dy in range(-hc, hc + 1) for dx in range(-hc, hc + 1) if (dx, dy) != (0, 0)]
    perm = [order.index((-dx, dy)) for dx, dy in order]
    dl, dm = cr.transform(left, c, mode), cr.transform(cr.mirror(left), c, mode)
    md = cr.mirror(dl)
    permuted = np.zeros_like(md)
    for k, j in enumerate(perm):
        permuted |= ((md >> np.uint64(j)) & np.uint64(1)) << np.uint64(k)
    assert np.array_equal(permuted, dm)
    # Hamming distance is blind to the permutation: the right pass on mirrored-order descriptors is the definition's
    want = cr.right_reference(left, right, d, sw, c, mode)
    dr = cr.transform(right, c, mode)
    best, web = cr.wta_from_descriptors(cr.mirror(dr), cr.mirror(dl), d, sw, mode)
    assert np.array_equal(cr.mirror(web), want[1]) and np.array_equal(cr.mirror(best), want[0])


@pytest.mark.parametrize("census", [3, 5, 7])
@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
def test_strictly_increasing_map_leaves_the_descriptors(census, mode):
    """R' = 2 R + 1 on values 0..127 is strictly increasing: descriptors (so every map) unchanged.  The ghost halo
    reads 0 for both, which is below every value of R' but equal to R = 0 -- there '0 < 0' and '0 < 1' differ, so the
    ghost case keeps R >= 1"""
    rng = np.random.default_rng(census)
    lo = 1 if mode == "ghost" else 0
    r = rng.integers(lo, 128, (13, 17)).astype(np.uint8)
    r2 = (2 * r.astype(np.int32) + 1).astype(np.uint8)
    assert np.array_equal(cr.transform(r, census, mode), cr.transform(r2, census, mode))
    left = rng.integers(lo, 128, (13, 17)).astype(np.uint8)
    a = cr.wta(left, r, 9, 5, census, mode)
    b = cr.wta((2 * left.astype(np.int32) + 1).astype(np.uint8), r2, 9, 5, census, mode)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
def test_constant_images_give_web_1_best_0(mode):
    z = np.full((8, 11), 77, np.uint8)
    best, web = cr.wta(z, z, 6, 3, 5, mode)
    assert (web == 1).all() and (best == 0).all()


def test_refine_uses_the_equiangular_fit():
    left, right = rand_gray(20, 12, 9, 256)
    best, web = cr.wta(left, right, 10, 3, 5, "toroidal")
    sub, c = cr.refine(left, right, web, 10, 3, 5, "toroidal")
    assert np.array_equal(c[1], best)                   # C(s - 1) is the winner's cost
    s = web.astype(np.int64)
    inner = (s >= 2) & (s <= 9)
    q = sub.astype(np.int64) - 16 * s
    assert (np.abs(q) <= 8).all() and (q[~inner] == 0).all()
    assert (c[0][s == 1] == -1).all() and (c[2][s == 10] == -1).all()
