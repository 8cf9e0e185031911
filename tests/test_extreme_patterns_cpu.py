"""The extreme inputs of tests/extreme_patterns.py on the CPU: that they reach the corners of the arithmetic they
are named after (so that no later edit of a generator quietly weakens the GPU sweeps of tests/test_extremes_gpu.py),
and that the oracle's match and cost definitions agree on them with the numpy restatements."""
import numpy as np
import pytest

from tests import extreme_patterns as xp
from tests import oracle

MODES = ["toroidal", "ghost"]


def oracle_bests(names, le, re, d, n, mode):
    return np.stack([oracle.hot_path(le[i], re[i], d, n, mode)[0] for i in range(len(names))])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sw", range(1, 26))
def test_patterns_reach_every_plane_of_the_count(mode, sw):
    """every window 1 .. 25 (even widths are the next odd window), on the shapes the GPU sweeps use: the winning
    mismatch counts of the batch set every bit plane below SB = bits_for(n^2), and (toroidal) both 0 and n^2 - 1
    win somewhere"""
    n = xp.window(sw)
    for d in (13, 32):
        w, h = 150, n + 10
        names, le, re = xp.edge_batch(w, h, n, d)
        bests = oracle_bests(names, le, re, d, sw, mode)
        assert xp.coverage_gaps(bests, n, mode) == [], (n, d, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sw", [1, 3, 9, 21])
def test_patterns_hit_the_corners_they_are_named_after(mode, sw):
    n = xp.window(sw)
    w, h, d = 150, n + 12, 40
    taps = xp.taps(w, h, n, mode)
    names, le, re = xp.edge_batch(w, h, n, d)
    res = {p: oracle.hot_path(le[i], re[i], d, sw, mode) for i, p in enumerate(names)}
    for p in ("all_match_0", "all_match_1"):            # every shift ties at count 0: the last wins
        if p == "all_match_1" and mode == "ghost":
            continue                                    # (ghost: ones meet the zeros beyond the right border)
        best, web = res[p]
        assert (web == d).all() and np.array_equal(best, taps), p
    best, web = res["no_centre_match"]
    if mode == "toroidal":
        assert (web == d).all() and (best == 0).all()
    for p in ("lone_match", "lone_match_n1"):           # one match per window, the rows off the lattice: none
        best, web = res[p]
        counts = xp.winning_counts(best, n, mode)
        assert counts.size and ((best == 0).any() or (n == 1 and p == "lone_match")), p
        if mode == "toroidal":
            assert (counts == n * n - 1).all(), p
    for p in ("true_shift_1", "true_shift_mid", "true_shift_last"):
        k = {"true_shift_1": 1, "true_shift_mid": d // 2, "true_shift_last": d - 1}[p]
        best, web = res[p]
        if mode == "toroidal":                          # the true shift matches everywhere, uniquely in most pixels
            assert np.array_equal(best, taps) and ((web == k + 1).mean() > 0.9 or n == 1), p
    best, _ = res["col_bands"]
    assert (xp.winning_counts(best, n, mode) == 0).any()
    assert (xp.winning_counts(res["skewed_98_02"][0], n, mode) >= (n * n) // 2).any() or n == 1


def test_cost_patterns_reach_the_largest_sums():
    """black against white: every tap of every shift costs 255 (SAD) / 65025 (SSD) -- the largest window sums"""
    for sw in (3, 11, 21):
        w, h, d = 150, sw + 10, 40
        left, right = xp.gray_pattern("black_white", w, h)
        for cost, tap in (("sad", 255), ("ssd", 65025)):
            best, web = oracle.cost_hot_path(left, right, d, sw, "toroidal", cost)
            assert (best == sw * sw * tap).all() and (web == 1).all(), (sw, cost)
        left, right = xp.gray_pattern("both_77", w, h)
        best, web = oracle.cost_hot_path(left, right, d, sw, "ghost", "ssd")
        assert (best == 0).all() and (web == 1).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mistake,windows", [("poison one short", (3, 5, 7, 9)), ("poison below a full cost", (13,))])
def test_a_free_shift_below_zero_tells_a_poison_constant_that_is_too_small(mistake, windows, mode):
    """(the mutation audit's S1 and S3: k_sad_pc with BIG one short of a tie, and with the small windows' scheme at
    13 x 13, passed every SAD test.)  The position below shift 0 takes the arg-min only where EVERY real shift costs at
    least BIG more than it does: with the stripes moved by one column and D = 1 the only real shift costs n^2 255 and
    the shift -1 nothing.  No gray pattern of test_sad_kernels_at_the_extremes, at any of its shift counts, has such a pixel."""
    for sw in windows:
        w, h = xp.FREE_SHIFT_SHAPE[0], sw + xp.FREE_SHIFT_SHAPE[1]
        left, right = xp.gray_pattern(xp.FREE_SHIFT_BELOW_ZERO, w, h)
        best, web = oracle.cost_hot_path(left, right, 1, sw, mode, "sad")
        wins = xp.wins_below_zero(left, right, best, sw, mode, mistake)
        if mode == "toroidal":
            three_of_four = ((np.arange(w) - sw // 2) & 3) != 0         # the column residues that have a position -1
            assert (best == sw * sw * 255).all() and (wins == three_of_four[None, :]).all(), sw
        else:
            # (only where no tap is missing: a window cut by the border costs less than BIG, as in the kernel, which
            # stages zeros there in both images)
            half = sw // 2
            three_of_four = ((np.arange(w) - half) & 3) != 0
            assert (wins[half:h - half, sw:w - sw] == three_of_four[None, sw:w - sw]).all() and h - 2 * half == 3, sw
        assert (web == 1).all()
        bb, bw = xp.cost_hot_path_bruteforce(left, right, 1, sw, mode, "sad")
        assert np.array_equal(bb, best) and np.array_equal(bw, web)
        for d in (1, 33, 500):
            for name in xp.GRAY_PATTERNS:
                left, right = xp.gray_pattern(name, 150, sw + 10)
                best, _ = oracle.cost_hot_path(left, right, d, sw, mode, "sad")
                assert not xp.wins_below_zero(left, right, best, sw, mode, mistake).any(), (sw, d, name)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sw,d", [(1, 9), (3, 33), (4, 7), (5, 20), (9, 17)])
def test_oracle_hot_path_equals_the_bruteforce_on_every_pattern(mode, sw, d):
    n = xp.window(sw)
    w, h = 45, n + 7
    names, le, re = xp.edge_batch(w, h, n, d)
    for i, p in enumerate(names):
        ob, ow = oracle.hot_path(le[i], re[i], d, sw, mode)
        bb, bw = xp.hot_path_bruteforce(le[i], re[i], d, sw, mode)
        assert np.array_equal(ow, bw), (p, mode, sw, d)
        assert np.array_equal(ob, bb), (p, mode, sw, d)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cost", ["sad", "ssd"])
@pytest.mark.parametrize("sw,d", [(3, 1), (3, 70), (5, 33), (11, 40)])
def test_oracle_cost_hot_path_equals_the_bruteforce_on_every_pattern(mode, cost, sw, d):
    w, h = 66, sw + 5
    names, left, right = xp.gray_batch(w, h)
    for i, p in enumerate(names):
        ob, ow = oracle.cost_hot_path(left[i], right[i], d, sw, mode, cost)
        bb, bw = xp.cost_hot_path_bruteforce(left[i], right[i], d, sw, mode, cost)
        assert np.array_equal(ow, bw), (p, mode, cost, sw, d)
        assert np.array_equal(ob, bb), (p, mode, cost, sw, d)


def test_bruteforce_restatements_are_not_vacuous():
    """the restatements tell a wrong tie rule from the right one: on all-tie inputs the last shift wins the match,
    the first the cost"""
    le = np.ones((12, 20), np.uint8)
    _, web = xp.hot_path_bruteforce(le, le, 9, 3)
    assert (web == 9).all()
    g = np.full((12, 20), 5, np.uint8)
    _, web = xp.cost_hot_path_bruteforce(g, g, 9, 3, cost="ssd")
    assert (web == 1).all()
