"""The extreme inputs of tests/census_extreme_patterns.py on the CPU: that they reach the bounds they are named
after -- A = 30000 and 26250, L_r = 62767, S = 502136 -- by the numpy definitions (tests/census_reference.py,
tests/sgm_reference.py), never by the HIP path, so that no later edit of a generator or of a shape quietly takes the
GPU tests of tests/test_census_extremes_gpu.py off the bounds; and that the vectorised definitions agree with the
pixel-by-pixel ones on tiny versions of every pattern."""
import numpy as np
import pytest

from tests import census_extreme_patterns as cx
from tests import census_reference as cr
from tests import sgm_reference as sr

MODES = ["toroidal", "ghost"]
CENSUS = [3, 5, 7]
W, H = 98, 28                      # the GPU tests' lattice shape: W % 49 == 0, H % 7 == 0
A_MAX = 30000                      # 48 * 625
L_MAX = 62767                      # A_MAX + 32767
S_MAX = 502136                     # 8 * L_MAX


def test_the_bounds_are_the_kernels():
    assert A_MAX == cx.bits(7) * 25 * 25 and L_MAX == A_MAX + 32767 and S_MAX == 8 * L_MAX
    assert A_MAX + 0x8000 < 1 << 16 and S_MAX < 1 << 19 and (S_MAX << 8 | 255) < 1 << 31


def test_lattice_windows_hold_distinct_values():
    """every 7 x 7 window of the lattice, the toroidal wrap included, holds 49 distinct values"""
    img = cx.lattice(W, H).astype(np.int64)
    assert img.min() == 0 and img.max() == 240
    p = img[np.arange(-3, H + 3) % H][:, np.arange(-3, W + 3) % W]
    for y in range(H):
        for x in range(W):
            assert np.unique(p[y:y + 7, x:x + 7]).size == 49, (x, y)
    # every descriptor bit differs between the lattice and its inverse
    for c in CENSUS:
        a, b = cr.transform(img, c), cr.transform(255 - img, c)
        assert (np.bitwise_count(a ^ b) == cx.bits(c)).all(), c
        assert ((a | b) == np.uint64((1 << cx.bits(c)) - 1)).all() and ((a & b) == 0).all(), c


@pytest.mark.parametrize("census", CENSUS)
@pytest.mark.parametrize("sw", [1, 25])
def test_anti_reaches_the_full_window_cost(census, sw):
    """anti(98, 28, 0), toroidal, D = 1: best is (c^2 - 1) n^2 at every pixel -- 30000 for c = 7, n = 25"""
    n = cx.window(sw)
    full = cx.bits(census) * n * n
    left, right = cx.anti(W, H, 0)
    best, web = cr.wta(left, right, 1, sw, census, "toroidal")
    assert (best == full).all() and (web == 1).all()
    if census == 7 and sw == 25:
        assert full == A_MAX
    # k = D: the first shift past the range has that cost (k_census_wta adds 0x8000 to it), at every pixel
    for d in (1, 8, 9, 128, 129, 256, 257, 512):
        left, right = cx.anti(W, H, d % W)
        assert (cr.window_costs(left, right, d, sw, census, "toroidal") == full).all(), d
        assert (cr.window_costs(left, right, d % W, sw, census, "toroidal") == full).all(), d


def test_anti_profile_has_period_49_and_the_measured_ends():
    """c = 7, n = 25: A is 30000 at every pixel at d = k and falls to 14669 .. 14720 at (d - k) mod 49 = 24; the
    lattice has period 49 in x, so every pixel's profile has period 49 in d: for D > 49 shifts 49 apart tie exactly,
    at a non-zero cost"""
    k = 5
    left, right = cx.anti(W, H, k)
    a = sr.data_term(left, right, 2 * 49 + 3, 25, 7, "toroidal").astype(np.int64)
    assert (a[..., k] == A_MAX).all() and a.max() == A_MAX
    assert (a[..., [d for d in range(a.shape[-1]) if d % 49 != k]] < A_MAX).all()
    low = a[..., k + 24]
    assert low.max() == 14720 and low.min() == 14669 == a.min()
    assert np.array_equal(a[..., 49:], a[..., :-49])
    # the first minimum wins, however many later shifts tie with it, in one launch and across launches
    first = cr.wta(left, right, 49, 25, 7, "toroidal")
    assert (first[0] > 0).all() and first[1].max() <= 49
    for d in (64, 129, 200, 512):
        best, web = cr.wta(left, right, d, 25, 7, "toroidal")
        assert np.array_equal(web, first[1]) and np.array_equal(best, first[0]), d


@pytest.mark.parametrize("census", CENSUS)
@pytest.mark.parametrize("sw", [1, 25])
def test_rows_anti_is_one_constant(census, sw):
    """window_costs is one constant over all d and all pixels, toroidal: 42 n^2 = 26250 for c = 7, n = 25"""
    n = cx.window(sw)
    left, right = cx.rows_anti(56, 49)
    cl, cr_ = cr.transform(left, census), cr.transform(right, census)
    want = (census * census - census) * n * n
    if census == 7 and sw == 25:
        assert want == 26250
    for d in list(range(0, 512, 37)) + [1, 55, 56, 57, 129, 299, 511]:
        assert (cr.window_costs(left, right, d, sw, census, "toroidal", cl, cr_) == want).all(), d
    best, web = cr.wta_from_descriptors(cl, cr_, 512, sw, "toroidal")
    assert (web == 1).all() and (best == want).all()


def test_comb_puts_cheap_shifts_just_past_a_full_cost():
    """comb(98, 28), c = 7, n = 25, toroidal: shift 0 costs 30000 at every pixel; shifts 1, 3, 5, 7 -- past the range
    for D = 1, in the same lane -- cost so little that 0x8000 is the bias they need to lose: A + 0x4000 < 30000"""
    left, right = cx.comb(W, H)
    cl, cr_ = cr.transform(left, 7), cr.transform(right, 7)
    assert (cr.window_costs(left, right, 0, 25, 7, "toroidal", cl, cr_) == A_MAX).all()
    for d in (1, 3, 5, 7):
        a = cr.window_costs(left, right, d, 25, 7, "toroidal", cl, cr_)
        assert a.max() + 0x4000 < A_MAX and a.max() + 0x8000 > A_MAX, d
    best, web = cr.wta(left, right, 1, 25, 7, "toroidal")
    assert (best == A_MAX).all() and (web == 1).all()


@pytest.mark.parametrize("p1,p2", [(32767, 32767), (0, 32767)])
def test_sgm_reaches_its_u16_and_key_bounds(p1, p2):
    """anti(98, 28, 5), D = 256, n = 25, c = 7, toroidal: some L_r of every direction is exactly 62767, and S is
    exactly 8 * 62767 = 502136 (4 * 62767 with 4 paths) somewhere"""
    left, right = cx.anti(W, H, 5)
    a = sr.data_term(left, right, 256, 25, 7, "toroidal")
    assert a.max() == A_MAX and a.dtype == np.int32
    vols = [sr.path(a, dx, dy, p1, p2) for dx, dy in sr.DIRS[8]]
    for (dx, dy), L in zip(sr.DIRS[8], vols):
        assert L.max() == L_MAX, (dx, dy)
        assert (L >= a).all()
    assert max(int(L.max()) for L in vols) == L_MAX
    assert sr.aggregate(a, p1, p2, 8).max() == S_MAX == 8 * L_MAX
    assert sr.aggregate(a, p1, p2, 4).max() == 4 * L_MAX


def test_sgm_shows_the_full_cost_only_where_it_is_the_only_shift():
    """anti's shift k costs 30000 everywhere, but a cheaper shift wins and the path minimum never passes through k: with
    the data term saturated at 0x7000 = 28672 (profiles/mutants: census_c, a mutant of k_sgm_cost_v's stores) the maps
    of anti(98, 28, 5) are what they were, so that case cannot tell.  At D = 1 the full cost is the winner itself:
    best = paths * 30000 at every pixel, which the saturated data term misses (test_census_extremes_gpu.py
    test_sgm_full_cost_at_the_only_shift)"""
    left, right = cx.anti(W, H, 5)
    a = sr.data_term(left, right, 64, 25, 7, "toroidal")
    assert a.max() == A_MAX and (a > 0x7000).any()
    for p1, p2 in ((32767, 32767), (0, 0)):
        want, sat = sr.winner(sr.aggregate(a, p1, p2, 8)), sr.winner(sr.aggregate(np.minimum(a, 0x7000), p1, p2, 8))
        assert all(np.array_equal(x, y) for x, y in zip(want, sat)), (p1, p2)
    left, right = cx.anti(W, H, 0)
    for mode in ("toroidal", "ghost"):
        a = sr.data_term(left, right, 1, 25, 7, mode)
        # (ghost: a window on the border holds fewer pixels; the interior still lies above 0x7000)
        assert (a == A_MAX).all() if mode == "toroidal" else 0x7000 < a.max() < A_MAX
        for paths in (4, 8):
            best, web, sub = sr.winner(sr.aggregate(a, 32767, 32767, paths))
            assert best.max() == paths * a.max() and (web == 1).all() and (sub == 16).all()
            assert not np.array_equal(sr.winner(sr.aggregate(np.minimum(a, 0x7000), 32767, 32767, paths))[0], best)


def test_sgm_of_rows_anti_is_constant_over_d():
    """every A, so every L_r and S, is the same at all shifts of a pixel, whatever the penalties: web 1, sub 16,
    best = paths * 26250 (toroidal)"""
    left, right = cx.rows_anti(56, 49)
    a = sr.data_term(left, right, 40, 25, 7, "toroidal")
    assert (a == 26250).all()
    for p1, p2 in ((32767, 32767), (0, 32767), (0, 0)):
        for paths in (4, 8):
            s = sr.aggregate(a, p1, p2, paths)
            assert (s == paths * 26250).all()
            best, web, sub = sr.winner(s)
            assert (web == 1).all() and (sub == 16).all() and (best == paths * 26250).all()


def test_low_end_of_anti():
    """n = 1, c = 3: A <= 8, reached, with ties between shifts at most pixels"""
    left, right = cx.anti(W, H, 3)
    a = sr.data_term(left, right, 64, 1, 3, "toroidal")
    assert a.max() == 8 and a.min() == 0
    low = np.sort(a, axis=-1)
    assert (low[..., 0] == low[..., 1]).mean() > 0.8         # the minimum is reached twice or more at most pixels


@pytest.mark.parametrize("mode", MODES)
def test_level_pairs_meet_the_strict_compare(mode):
    w, h = 12, 9
    for c in CENSUS:
        z = cr.transform(np.zeros((h, w), np.uint8), c, mode)
        assert (z == 0).all()                            # halo 0 against pixel 0: `<` is strict
        t = cr.transform(np.full((h, w), 255, np.uint8), c, mode)
        assert (t == 0).all() if mode == "toroidal" else (t[0, 0] != 0 and t[h // 2, w // 2] == 0)
    # rows of 0 and 255 against their inverse: the rows at dy = -3, -1, 1, 3 differ from the centre's, 4 * 7 bits
    left, right = cx.level_pair("two_level_rows", w, 8)
    a = cr.window_costs(left, right, 0, 1, 7, mode)
    assert (a == 28).all() if mode == "toroidal" else a[4, 6] == 28


# ---------------------------------------------------------------------------
# tiny versions: the vectorised definitions against the pixel-by-pixel ones
# ---------------------------------------------------------------------------

def tiny_pairs():
    out = [("anti_%d" % k, cx.anti(49, 7, k)) for k in (0, 2, 5)]
    out.append(("anti_seam", cx.anti(20, 6, 3)))
    out.append(("rows_anti", cx.rows_anti(5, 49)))
    out.append(("comb", cx.comb(14, 7)))
    out.append(("rows_anti_seam", cx.rows_anti(6, 9)))
    out += [(name, cx.level_pair(name, 9, 6)) for name in cx.LEVEL_PATTERNS]
    return out


TINY = tiny_pairs()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", [n for n, _ in TINY])
def test_census_definition_equals_the_pixel_loop_on_tiny_patterns(mode, name):
    left, right = dict(TINY)[name]
    for census, sw, d in ((7, 3, 6), (5, 1, 4), (3, 3, 3)):
        assert np.array_equal(cr.transform(left, census, mode), cr.transform_bruteforce(left, census, mode))
        assert np.array_equal(cr.transform(right, census, mode), cr.transform_bruteforce(right, census, mode))
        want = cr.wta_bruteforce(left, right, d, sw, census, mode)
        got = cr.wta(left, right, d, sw, census, mode)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, mode, census)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", [n for n, _ in TINY])
def test_sgm_definition_equals_the_path_loop_on_tiny_patterns(mode, name):
    left, right = dict(TINY)[name]
    for census, sw, d, p1, p2, paths in ((7, 3, 5, 32767, 32767, 8), (7, 1, 6, 0, 32767, 4), (3, 1, 4, 0, 0, 8)):
        want = sr.sgm_bruteforce(left, right, d, sw, census, p1, p2, paths, mode)
        got = sr.sgm(left, right, d, sw, census, p1, p2, paths, mode)
        for g, e, what in zip(got, want, ("best", "web", "sub")):
            assert g.dtype == e.dtype and np.array_equal(g, e), (what, name, mode, census, p1, p2, paths)
