"""The numpy definition of the cross-based matcher (tests/cross_reference.py) against its own
pixel-by-pixel restatement, the identities that tie it to the census box matcher, the bounds its kernels' fields rest
on, and what it is for: fewer wrong pixels beside depth edges than any box."""
import numpy as np
import pytest

from tests import census_reference as cr
from tests import cross_patterns as cp
from tests import cross_reference as x

MODES = ("toroidal", "ghost")


def noise(w, h, seed, levels=256):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, levels, (h, w)).astype(np.uint8) * (256 // levels)).astype(np.uint8)


# (w, h, D, census, tau, arm, mode): both borders, every census width, arm and tau of the issue's lists, images no
# wider / higher than the arm, D = 1 and D > W
BRUTE = [(13, 9, 5, 7, 12, 1, "toroidal"), (13, 9, 5, 7, 12, 1, "ghost"), (13, 9, 1, 5, 0, 7, "toroidal"),
         (13, 9, 15, 3, 255, 15, "ghost"), (11, 8, 4, 3, 12, 0, "toroidal"), (11, 8, 4, 5, 12, 0, "ghost"),
         (7, 5, 3, 7, 255, 7, "toroidal"), (7, 5, 9, 5, 12, 7, "ghost"), (6, 15, 2, 7, 12, 15, "ghost"),
         (15, 4, 17, 3, 0, 15, "toroidal"), (12, 10, 6, 5, 255, 7, "toroidal"), (12, 10, 6, 7, 0, 1, "ghost"),
         (1, 1, 3, 7, 12, 15, "toroidal"), (1, 6, 2, 3, 255, 7, "ghost"), (9, 1, 12, 5, 12, 15, "toroidal")]


@pytest.mark.parametrize("w,h,D,census,tau,arm,mode", BRUTE)
def test_vectorised_form_is_the_bruteforce(w, h, D, census, tau, arm, mode):
    # few gray levels: differences at, below and above tau all occur, and shifts tie
    left, right = noise(w, h, 100 + w + arm, 16), noise(w, h, 200 + h + tau, 16)
    a = x.arms(left, tau, arm)
    ab = x.arms_bruteforce(left, tau, arm)
    for got, want in zip(a, ab):
        assert np.array_equal(got, want)
    assert all(np.array_equal(g, wnt) for g, wnt in zip(x.unpack(x.pack(a)), a))
    best, web = x.wta(left, right, D, census, tau, arm, mode)
    bb, wb, size = x.wta_bruteforce(left, right, D, census, tau, arm, mode)
    assert np.array_equal(best, bb) and np.array_equal(web, wb)
    n = x.support(a)
    assert np.array_equal(n, size) and n.min() >= 1 and n.max() <= min(961, w * h)


def test_arms_stop_at_the_first_failure_and_at_the_border():
    img = np.array([[10, 12, 30, 11, 10, 10, 10]], np.uint8)
    l, r, u, d = x.arms(img, 5, 15)
    assert l.tolist() == [[0, 1, 0, 0, 1, 2, 3]]         # pixel 3 never reaches back over the 30
    assert r.tolist() == [[1, 0, 0, 3, 2, 1, 0]]
    assert not u.any() and not d.any()
    flat = np.full((40, 50), 7, np.uint8)
    l, r, u, d = x.arms(flat, 0, 15)
    xx, yy = np.arange(50)[None, :], np.arange(40)[:, None]
    assert np.array_equal(l, np.minimum(xx, 15) + 0 * yy) and np.array_equal(r, np.minimum(49 - xx, 15) + 0 * yy)
    assert np.array_equal(u, np.minimum(yy, 15) + 0 * xx) and np.array_equal(d, np.minimum(39 - yy, 15) + 0 * xx)
    assert x.support((l, r, u, d)).max() == 961


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("census", (3, 5, 7))
def test_arm_zero_is_the_pixelwise_census_matcher(mode, census):
    left, right = noise(33, 20, 1), noise(33, 20, 2)
    best, web = x.wta(left, right, 9, census, 12, 0, mode)
    want_best, want_web = cr.wta(left, right, 9, 1, census, mode)
    assert np.array_equal(best, want_best) and np.array_equal(web, want_web)


@pytest.mark.parametrize("arm", (1, 4, 12))
def test_ghost_without_a_threshold_is_the_box_matcher(arm):
    """tau = 255: the arms stop at the image border only, where the ghost box's taps count 0"""
    left, right = noise(37, 29, 3), noise(37, 29, 4)
    best, web = x.wta(left, right, 11, 7, 255, arm, "ghost")
    want_best, want_web = cr.wta(left, right, 11, 2 * arm + 1, 7, "ghost")
    assert np.array_equal(best, want_best) and np.array_equal(web, want_web)


@pytest.mark.parametrize("mode", MODES)
def test_best_is_bounded_by_the_support(mode):
    left, right = noise(41, 30, 5, 8), noise(41, 30, 6, 8)
    best, _ = x.wta(left, right, 7, 7, 40, 15, mode)
    assert (best <= 48 * x.support(x.arms(left, 40, 15))).all() and (best >= 0).all()


@pytest.mark.parametrize("mode", MODES)
def test_constant_pair_gives_the_first_shift_at_no_cost(mode):
    flat = np.full((21, 34), 90, np.uint8)
    best, web, sub = x.wta(flat, flat, 12, 7, 20, 15, mode, want_sub=True)
    assert (web == 1).all() and (best == 0).all() and (sub == 16).all()


@pytest.mark.parametrize("mode", MODES)
def test_right_reference_is_the_mirrored_left_pass(mode):
    left, right = noise(35, 18, 7, 16), noise(35, 18, 8, 16)
    best_right, web_right = x.right_reference(left, right, 8, 5, 12, 7, mode)
    b, w = x.wta(x.mirror(right), x.mirror(left), 8, 5, 12, 7, mode)
    assert np.array_equal(x.mirror(best_right), b) and np.array_equal(x.mirror(web_right), w)
    # a pair that is one image moved by 3 (right(x + 3) = left(x), toroidal): both maps find the move at every pixel
    tex = noise(35, 18, 9)
    moved = np.roll(tex, 3, axis=1)
    bl, wl = x.wta(tex, moved, 8, 7, 12, 7, "toroidal")
    br, wr = x.right_reference(tex, moved, 8, 7, 12, 7, "toroidal")
    assert (wl == 4).all() and (wr == 4).all() and not bl.any() and not br.any()
    e = x.expected(left, right, 8, 5, 12, 7, mode, 1)
    assert e["rejected"] == int((e["checked"] == 0).sum()) and (e["sub_checked"][e["checked"] == 0] == 0).all()
    assert np.array_equal(e["sub_checked"][e["checked"] != 0], e["sub"][e["checked"] != 0])


def test_extreme_pair_reaches_the_bound_of_the_fields():
    """anti(98, 42, 0), toroidal, c = 7, tau = 255, arm 15, D = 1: E = 48 * 961 at exactly the pixels whose support is
    the full cross -- the largest value of the u16 fields, of the prefix sums and of the keys"""
    left, right = cp.anti(cp.EXTREME_W, cp.EXTREME_H, 0)
    best, web = x.wta(left, right, 1, 7, 255, 15, "toroidal")
    n = x.support(x.arms(left, 255, 15))
    assert cp.E_MAX == 46128 < 2 ** 16
    assert int((best == cp.E_MAX).sum()) == cp.EXTREME_INTERIOR == 816
    assert np.array_equal(best == cp.E_MAX, n == 961) and best.max() == cp.E_MAX and (web == 1).all()


def test_extreme_pair_with_the_maximum_just_past_the_range():
    D = 5
    left, right = cp.anti(cp.EXTREME_W, cp.EXTREME_H, D)
    e = x.volume(left, right, D + 1, 7, 255, 15, "toroidal")
    assert e[D].max() == cp.E_MAX and e[:D].max() < cp.E_MAX
    best, web = x.wta(left, right, D, 7, 255, 15, "toroidal")
    assert np.array_equal(best, e[:D].min(0)) and web.max() <= D


def test_rows_pair_ties_at_every_shift():
    left, right = cp.rows_anti(cp.EXTREME_W, cp.EXTREME_H)
    best, web = x.wta(left, right, 20, 7, 255, 15, "toroidal")
    assert (web == 1).all() and best.max() > 2 ** 15      # an all-tie map at a cost above the sign bit of a u16


def band_error(web, truth, band):
    return float(((web - 1) != truth)[band].mean())


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_cross_support_keeps_depth_edges_where_boxes_smear_them(seed):
    """occluder_scene(96, 64, seed, 3, 11), ghost, D = 16, c = 7: the share of wrong pixels within 4 of a depth edge.
    Measured: box 9 x 9 0.178 / 0.210 / 0.177, box 21 x 21 0.119 / 0.154 / 0.158, cross (tau 20, arm 10) 0.000 / 0.007 /
    0.002 for seeds 1 / 2 / 3."""
    left, right, truth = cp.occluder_scene(96, 64, seed, 3, 11)
    band = cp.edge_band(truth, 4, 12)
    assert int(band.sum()) == 1441
    _, web = x.wta(left, right, 16, 7, 20, 10, "ghost")
    cross = band_error(web, truth, band)
    box9 = band_error(cr.wta(left, right, 16, 9, 7, "ghost")[1], truth, band)
    box21 = band_error(cr.wta(left, right, 16, 21, 7, "ghost")[1], truth, band)
    print(f"seed {seed}: box 9 {box9:.3f}, box 21 {box21:.3f}, cross {cross:.3f}")
    assert box9 > 0.1 and box21 > 0.1
    assert cross <= box9 / 4 and cross <= box21 / 4


# ---------------------------------------------------------------------------
# the shapes of tests/test_cross_shapes_gpu.py: what the expected maps must hold for the cases to mean anything
# ---------------------------------------------------------------------------

def test_small_shapes_cover_what_they_are_there_for():
    tiles = {(w, h): (-(-w // (64 - 2 * arm)), -(-h // 32), 64 - 2 * arm) for w, h, d, arm in cp.SMALL}
    assert any(w == 1 and d > 8 for w, h, d, arm in cp.SMALL)                        # smn_mod(x + dlo, 1), dlo > 0
    # x + dlo mod W < W, at most 7 is added: W < 8 for a second wrap, and a shift 2 W + (W - 1 - x) <= 7 inside D
    assert sum(1 for w, h, d, arm in cp.SMALL if w < 8 and d > 2 * w and 2 * w <= 7) >= 2
    assert any(h < 32 and tiles[(w, h)][:2] == (1, 1) for w, h, d, arm in cp.SMALL)
    assert any(w <= arm == 15 and h <= arm for w, h, d, arm in cp.SMALL)
    assert any(w <= arm and h > 32 for w, h, d, arm in cp.SMALL)
    assert {(w, arm) for w, h, d, arm in cp.SMALL if w == tiles[(w, h)][2] + 1} == {(35, 15), (65, 0)}
    assert all(w < 64 + d for w, h, d, arm in cp.SMALL)                              # ghost: `xr < W` decides
    w, h, d, arm, tau = cp.MANY_TILES
    tx, ty = -(-w // (64 - 2 * arm)), -(-h // 32)
    assert tx >= 3 and ty >= 3 and tx * ty > 8 and tx * ty % 8 and d >= 9 and d % 2 == 1 and d % 8 == 3


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("w,h,d,arm", [c for c in cp.SMALL if c[0] * c[1] <= 45])
def test_small_shapes_vectorised_form_is_the_bruteforce(w, h, d, arm, mode):
    """the definition itself at W = 1, W < 8 and D > 2 W, where the toroidal shift wraps several times"""
    left, right = cp.related_pairs(w, h, 1, 7)
    for tau in cp.SMALL_TAUS:
        best, web = x.wta(left[0], right[0], d, 7, tau, arm, mode)
        bb, wb, _ = x.wta_bruteforce(left[0], right[0], d, 7, tau, arm, mode)
        assert np.array_equal(best, bb) and np.array_equal(web, wb)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("census", (3, 7))
@pytest.mark.parametrize("D", sorted(cp.MANY_SHIFTS))
def test_many_shifts_maps_hold_answers_above_256(D, census, mode):
    """from the reference alone.  D = 512 as the conditions stand; D = 257 has no shift between 256 and D, so there
    `web == D` is the only answer above 256 and carries both conditions"""
    left, right = cp.many_shifts_pair(D)
    e = x.expected(left, right, D, census, cp.MANY_SHIFTS_TAU, cp.MANY_SHIFTS_ARM, mode, 1)
    web, checked = e["web"], e["checked"]
    counts = dict(top=int((web == D).sum()), between=int(((web > 256) & (web < D)).sum()), above=int((web > 256).sum()),
                  right=int((e["web_right"] > 256).sum()), accepted=int((checked > 256).sum()),
                  at_256=int((web == 256).sum()))
    print(D, census, mode, counts)
    if mode == "toroidal":
        assert counts["top"] >= 100
        assert counts["between"] >= 100 or D == 257
    assert counts["above"] >= 100
    assert counts["right"] >= 100
    assert counts["accepted"] >= 1
    assert counts["at_256"] >= 1                          # (the last index of 8 bits is an answer too, in both modes)


def test_index_of_8_bits_shows_on_many_shifts_only():
    """MISTAKES["index of 8 bits"]: the same maps as the definition on every case of CASES (three pairs, every census
    width, both modes), other maps on every many-shifts case"""
    wrong = cp.MISTAKES["index of 8 bits"]
    for w, h, d, arm, tau in cp.CASES:
        for census in (3, 5, 7):
            left, right = cp.related_pairs(w, h, 3, 100 * census + d + arm)
            for mode in MODES:
                for q in range(3):
                    e = x.volume(left[q], right[q], d, census, tau, arm, mode)
                    assert all(np.array_equal(a, b) for a, b in zip(wrong(e), x._wta(e)))
    for D in cp.MANY_SHIFTS:
        left, right = cp.many_shifts_pair(D)
        for census in (3, 7):
            for mode in MODES:
                e = x.volume(left, right, D, census, cp.MANY_SHIFTS_TAU, cp.MANY_SHIFTS_ARM, mode)
                (b8, w8), (b, wb) = wrong(e), x._wta(e)
                assert np.array_equal(b8, b) and int((w8 != wb).sum()) >= 100 and w8.max() <= 256


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("census", (5, 7))
def test_extreme_pairs_at_the_other_instances(census, mode):
    """what tests/test_cross_gpu.py::test_extreme_pairs asserts of its new cases, and that each still is an extreme"""
    w, h = cp.EXTREME_W, cp.EXTREME_H
    full = (census * census - 1) * 961
    left, right = cp.anti(w, h, 0)
    best, web = x.wta(left, right, 1, census, 255, 15, mode)
    if mode == "toroidal":
        assert int((best == full).sum()) == cp.EXTREME_INTERIOR and best.max() == full
    else:
        assert best.max() <= full and best.max() > full // 2
    left, right = cp.rows_anti(w, h)
    best, web = x.wta(left, right, 20, census, 255, 15, mode)
    if mode == "toroidal":
        assert (web == 1).all() and best.max() == (census * census - census) * 961


def test_tall_extreme_makes_the_column_sums_pass_16_bits():
    """the existing extremes cannot (42 rows); anti(98, 77, 0) can: full rows of H = 1488 in 60 rows of one tile"""
    assert cp.EXTREME_H * 31 * 48 < 2 ** 16 < 60 * 31 * 48
    left, right = cp.anti(cp.TALL_W, cp.TALL_H, 0)
    a = x.arms(left, 255, 15)
    flat = (np.zeros_like(a[0]), np.zeros_like(a[0]))
    for mode in MODES:
        cl, crr = cr.transform(left, 7, mode), cr.transform(right, 7, mode)
        rows = x.aggregate(cr.costs(cl, crr, 0, mode), (a[0], a[1]) + flat)      # H_0: the horizontal spans alone
        # tile row 1 of arm 15 starts at image row 32 - 15 = 17 and has 62 rows
        q = rows[17:17 + 62].cumsum(0)
        assert q.max() > 2 ** 16 and int((q[-1] > 2 ** 16).sum()) >= 30, mode
        best, web = x.wta(left, right, cp.TALL_D, 7, 255, 15, mode)
        assert best.max() <= cp.E_MAX and (mode == "ghost" or best.max() > 2 ** 15)


def test_tile_walk_is_the_definition():
    """cp.wta_tile_walk without a mistake (the kernel's packed pairs, tile rows and sums modulo 2^16) gives the maps of
    the definition: on small shapes of every kind, on the tall extreme, and pixel by pixel on a tiny one"""
    for w, h, d, arm in cp.SMALL:
        left, right = cp.related_pairs(w, h, 1, 3)
        for mode in MODES:
            got = cp.wta_tile_walk(left[0], right[0], d, 7, 12, arm, mode)
            assert all(np.array_equal(a, b) for a, b in zip(got, x.wta(left[0], right[0], d, 7, 12, arm, mode)))
    left, right = cp.related_pairs(5, 3, 1, 3)
    bb, wb, _ = x.wta_bruteforce(left[0], right[0], 20, 7, 255, 15, "toroidal")
    got = cp.wta_tile_walk(left[0], right[0], 20, 7, 255, 15, "toroidal")
    assert np.array_equal(got[0], bb) and np.array_equal(got[1], wb)


@pytest.mark.parametrize("mistake", cp.WALK_MISTAKES)
def test_carry_and_borrow_between_the_halves_show_on_the_tall_extreme_only(mistake):
    """WALK_MISTAKES: the same maps as the definition on every case of CASES (every census width, both modes) and on
    the 42-row extremes in every instance, where no tile's column sums pass 2^16; other maps on the tall extreme, where
    the SECOND shift of the pair wins at every pixel (web == 2) while the first one's sums wrap: best is off by one"""
    for w, h, d, arm, tau in cp.CASES:
        for census in (3, 5, 7):
            left, right = cp.related_pairs(w, h, 1, 100 * census + d + arm)
            for mode in MODES:
                got = cp.wta_tile_walk(left[0], right[0], d, census, tau, arm, mode, mistake)
                assert all(np.array_equal(a, b) for a, b in zip(got, x.wta(left[0], right[0], d, census, tau, arm, mode)))
    w, h = cp.EXTREME_W, cp.EXTREME_H
    for name, d in (("anti_0", 1), ("anti_D", 5), ("rows_anti", 20)):
        left, right = cp.rows_anti(w, h) if name == "rows_anti" else cp.anti(w, h, 0 if name == "anti_0" else d)
        for census, mode in ((7, "toroidal"), (5, "toroidal"), (7, "ghost"), (5, "ghost")):
            got = cp.wta_tile_walk(left, right, d, census, 255, 15, mode, mistake)
            assert all(np.array_equal(a, b) for a, b in zip(got, x.wta(left, right, d, census, 255, 15, mode))), (name, census, mode)
    left, right = cp.anti(cp.TALL_W, cp.TALL_H, 0)
    for mode in MODES:
        best, web = x.wta(left, right, cp.TALL_D, 7, 255, 15, mode)
        assert (web == 2).all()
        right_form = cp.wta_tile_walk(left, right, cp.TALL_D, 7, 255, 15, mode)
        assert np.array_equal(right_form[0], best) and np.array_equal(right_form[1], web)
        b, wb = cp.wta_tile_walk(left, right, cp.TALL_D, 7, 255, 15, mode, mistake)
        off = b.astype(np.int64) - best
        assert np.array_equal(wb, web) and int((off != 0).sum()) >= 1000
        assert set(np.unique(off)) == {0, 1 if mistake == "carry" else -1}
