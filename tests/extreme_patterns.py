"""Inputs built to reach the extremes of the match and cost kernels' arithmetic, and the numpy restatements that
pin the oracle on them.  Checker only: imported by tests/, never by the product package.

The edge patterns are u8 {0, 1} pairs (eL, eR).  The kernels keep a window's MISMATCH count, taps - best
(k_match_bs: on SB = bits_for(n * n) bit planes, B = 2^SB - 1 marking "no shift matched"; the popcount kernels:
in keys A << 10 | d), so each pattern is named after the corner of that count it drives:

    all_match_0 / all_match_1   both images 0 / 1: every shift ties at count 0 -> web = D, best = taps
    no_centre_match             eL 1, eR 0: no shift ever matches (toroidal) -> web = D, best = 0 (the marker)
    lone_match / lone_match_n1  eL 1, eR 1 on a lattice of spacing n / n + 1: a winning count of n^2 - 1 against
                                a nearly full B; the rows off the lattice carry the marker
    row_bands                   eL 1, eR rows in bands of 1 / 0 of heights 1, n // 2, n, n + 1 and around the
                                tile heights: a window row goes from all-match to all-mismatch in one slide
    col_bands                   eL 1, eR column bands of widths n - 1, n, n + 1, 31, 32, 33: row counts of
                                exactly n, at and across 32-pixel words
    skewed_*                    i.i.d. at densities (0.95, 0.05), (0.05, 0.95), (0.98, 0.02): winning counts
                                near n^2 at every plane
    true_shift_*                eL i.i.d. 0.5, eR = eL moved right by k (1, D // 2, D - 1): a unique count 0

The gray patterns (cost mode) are u8 pairs (left, right) at the ends of the SAD / SSD sums: black against white
both ways, constant images where every shift ties (the first must win), 0 / 255 column checkerboards and one
zero-cost column in a white image."""
from __future__ import annotations

import numpy as np

EDGE_PATTERNS = ("all_match_0", "all_match_1", "no_centre_match", "lone_match", "lone_match_n1", "row_bands",
                 "col_bands", "skewed_95_05", "skewed_05_95", "skewed_98_02", "true_shift_1", "true_shift_mid",
                 "true_shift_last")
TIE_PATTERNS = ("all_match_0", "all_match_1", "no_centre_match")

GRAY_PATTERNS = ("black_white", "white_black", "both_0", "both_255", "both_77", "checker_2", "checker_64",
                 "zero_cost_column")
SKEW = {"skewed_95_05": (0.95, 0.05), "skewed_05_95": (0.05, 0.95), "skewed_98_02": (0.98, 0.02)}
# not one of GRAY_PATTERNS: it is for one shift count only (D = 1), tests/test_extremes_gpu.py
# test_sad_full_cost_beside_a_free_shift_below_zero (the mutation audit's S1 and S3, profiles/mutants/README.md)
FREE_SHIFT_BELOW_ZERO = "stripes_off_by_one"
FREE_SHIFT_SHAPE = (32, 2)                  # width (even, above every window), rows beyond the window


def bits_for(v):
    """planes needed for 0 .. v (v < 2^bits), as k_match_bs's bits_for"""
    return int(v).bit_length()


def window(square_width):
    """the side of the window a square_width gives (even widths round up, as the reference's half = sw / 2)"""
    return 2 * (square_width // 2) + 1


def _bands(length, sizes):
    """0 / 1 labels of `length` cells in bands of the given sizes, repeated, alternating 1, 0, 1, ..."""
    out = np.zeros(length, np.uint8)
    pos, i = 0, 0
    while pos < length:
        size = max(1, int(sizes[i % len(sizes)]))
        out[pos:pos + size] = 1 - (i & 1)
        pos += size
        i += 1
    return out


def edge_pattern(name, w, h, n, d, seed=0):
    """one named (eL, eR) pair of u8 {0, 1} images, h x w, for an n x n window and d shifts"""
    rng = np.random.default_rng([seed, w, h, n, d, EDGE_PATTERNS.index(name)])
    ones = np.ones((h, w), np.uint8)
    zeros = np.zeros((h, w), np.uint8)
    if name == "all_match_0":
        return zeros, zeros.copy()
    if name == "all_match_1":
        return ones, ones.copy()
    if name == "no_centre_match":
        return ones, zeros
    if name in ("lone_match", "lone_match_n1"):
        p = n if name == "lone_match" else n + 1
        er = zeros.copy()
        # no two lattice points closer than p across the wrap either: one point per window
        er[np.ix_(np.arange(0, max(1, h - p + 1), p), np.arange(0, max(1, w - p + 1), p))] = 1
        return ones, er
    if name == "row_bands":
        rows = _bands(h, [1, n // 2, n, n + 1, 3, 4, 5, 2 * n, 7, 8, 9])
        return ones, np.repeat(rows[:, None], w, axis=1)
    if name == "col_bands":
        cols = _bands(w, [n - 1, n, n + 1, 31, 32, 33, n, 1])
        return ones, np.repeat(cols[None, :], h, axis=0)
    if name in SKEW:
        pl, pr = SKEW[name]
        return ((rng.random((h, w)) < pl).astype(np.uint8), (rng.random((h, w)) < pr).astype(np.uint8))
    if name.startswith("true_shift"):
        k = {"true_shift_1": 1, "true_shift_mid": d // 2, "true_shift_last": d - 1}[name]
        el = (rng.random((h, w)) < 0.5).astype(np.uint8)
        return el, np.roll(el, min(k, d - 1), axis=1)
    raise KeyError(name)


def edge_batch(w, h, n, d, names=EDGE_PATTERNS, seed=0):
    """-> (names, eL stack, eR stack): the patterns as the pairs of one batch"""
    pairs = [edge_pattern(p, w, h, n, d, seed) for p in names]
    return list(names), np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def gray_pattern(name, w, h, c=77):
    """one named (left, right) pair of u8 gray images"""
    black = np.zeros((h, w), np.uint8)
    white = np.full((h, w), 255, np.uint8)
    if name == "black_white":
        return black, white
    if name == "white_black":
        return white, black
    if name == "both_0":
        return black, black.copy()
    if name == "both_255":
        return white, white.copy()
    if name.startswith("both_"):
        v = np.full((h, w), int(name[5:]), np.uint8)
        return v, v.copy()
    if name.startswith("checker_"):
        period = int(name[8:])
        cols = np.where((np.arange(w) % period) < period // 2, 0, 255).astype(np.uint8)
        img = np.repeat(cols[None, :], h, axis=0)
        return img, img.copy()
    if name == FREE_SHIFT_BELOW_ZERO:
        # columns 0, 255, 0, 255, .. on the right, the same one column further on the left: L(x) = R(x - 1), so the
        # shift -1, which does not exist, would cost 0, and the shift 0 costs 255 at every tap (w even: also across
        # the wrap).  With D = 1 nothing else competes.
        assert w % 2 == 0
        img = np.repeat(np.where(np.arange(w) % 2, 255, 0).astype(np.uint8)[None, :], h, axis=0)
        return np.roll(img, 1, axis=1), img
    if name == "zero_cost_column":          # the layout of test_quad_sad_largest_possible_sums
        right = white.copy()
        right[:, min(60, w - 1)] = 0
        return black, right
    raise KeyError(name)


def gray_batch(w, h, names=GRAY_PATTERNS):
    pairs = [gray_pattern(p, w, h) for p in names]
    return list(names), np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


# ---------------------------------------------------------------------------
# what the patterns reach: the winning mismatch counts
# ---------------------------------------------------------------------------

def taps(w, h, n, mode):
    """valid window taps per pixel: n^2 (toroidal) or the in-image part of the window (ghost)"""
    half = n // 2
    if mode == "toroidal":
        return np.full((h, w), n * n, np.int64)
    x, y = np.arange(w), np.arange(h)
    cols = np.minimum(w - 1, x + half) - np.maximum(0, x - half) + 1
    rows = np.minimum(h - 1, y + half) - np.maximum(0, y - half) + 1
    return rows[:, None].astype(np.int64) * cols[None, :]


def winning_counts(bests, n, mode):
    """the winning mismatch counts taps - best of every matched pixel (best > 0) of a stack of best maps"""
    bests = np.asarray(bests, np.int64)
    h, w = bests.shape[-2:]
    t = np.broadcast_to(taps(w, h, n, mode), bests.shape)
    return (t - bests)[bests > 0]


def coverage_gaps(bests, n, mode):
    """-> a list of what the winning counts of `bests` fail to reach (empty: every extreme is reached):
    every bit plane below SB = bits_for(n^2) that a count of at most n^2 - 1 can hold is set in some count,
    and (toroidal) counts 0 and n^2 - 1 both occur"""
    counts = winning_counts(bests, n, mode)
    gaps = []
    if counts.size == 0:
        return ["no matched pixel"]
    seen = int(np.bitwise_or.reduce(counts))
    for k in range(bits_for(n * n)):
        if (1 << k) <= n * n - 1 and not (seen >> k) & 1:
            gaps.append(f"plane {k} of the count never set")
    if mode == "toroidal":
        for c in (0, n * n - 1):
            if not (counts == c).any():
                gaps.append(f"count {c} never wins")
    return gaps


# ---------------------------------------------------------------------------
# the definitions written out in numpy, independent of the oracle
# ---------------------------------------------------------------------------

def _shifted_right(img, d, mode):
    """the right image read at x + d: toroidal wraps, ghost reads 0 beyond the last column"""
    if mode == "toroidal":
        return np.roll(img, -d, axis=1)
    out = np.zeros_like(img)
    if d < img.shape[1]:
        out[:, :img.shape[1] - d] = img[:, d:]
    return out


def _window_sums(a, n, mode):
    half = n // 2
    h, w = a.shape
    total = np.zeros((h, w), np.int64)
    if mode == "toroidal":
        for ty in range(-half, half + 1):
            for tx in range(-half, half + 1):
                total += np.roll(a, (-ty, -tx), axis=(0, 1))
    else:
        p = np.pad(a, half)
        for ty in range(n):
            for tx in range(n):
                total += p[ty:ty + h, tx:tx + w]
    return total


def hot_path_bruteforce(el, er, num_shifts, square_width, mode="toroidal"):
    """The match definition written out: for shift d, left pixel x matches iff eL(x) == eR(x + d); the window
    count of matches is a score only where the pixel itself matched; the last shift reaching the maximum wins
    (web = d + 1), and where nothing matched web = D, best = 0."""
    el = np.asarray(el, np.int64)
    er = np.asarray(er, np.int64)
    n = window(square_width)
    best = np.zeros(el.shape, np.int64)
    web = np.zeros(el.shape, np.int32)
    for d in range(num_shifts):
        m = (el == _shifted_right(er, d, mode)).astype(np.int64)
        score = np.where(m == 1, _window_sums(m, n, mode), 0)
        upd = score >= best
        best[upd] = score[upd]
        web[upd] = d + 1
    return best.astype(np.int32), web


def cost_hot_path_bruteforce(left, right, num_shifts, square_width, mode="toroidal", cost="sad"):
    """The cost definition written out: per shift the window sum of |L(x) - R(x + d)| (or its square; ghost:
    R = 0 beyond the last column, taps outside the image cost nothing); the FIRST shift reaching the minimum
    wins."""
    left = np.asarray(left, np.int64)
    right = np.asarray(right, np.int64)
    n = window(square_width)
    best = np.full(left.shape, np.iinfo(np.int64).max, np.int64)
    web = np.zeros(left.shape, np.int32)
    for d in range(num_shifts):
        diff = left - _shifted_right(right, d, mode)
        c = diff * diff if cost == "ssd" else np.abs(diff)
        s = _window_sums(c, n, mode)
        upd = s < best
        best[upd] = s[upd]
        web[upd] = d + 1
    return best.astype(np.int32), web


# ---------------------------------------------------------------------------
# the mutation audit's S1 and S3: the constant that keeps shifts which do not exist from winning
# ---------------------------------------------------------------------------

# k_sad_pc's packed sums of the positions below shift 0 (a lane's first quad starts up to 3 positions early) start at a
# constant BIG, so that they lose to every real sum without a test in the row loop.  The mistakes: one short of what a
# tie needs (windows up to 9 x 9), and the constant of the larger windows' builds, which is no bound at 13 x 13.
MISTAKES = {"poison one short": lambda n: n * n * 255, "poison below a full cost": lambda n: 65535 - n * n * 255}


def sums_below_zero(left, right, n, mode):
    """the SAD window sums of the shifts -1, -2, -3 as the kernel forms them: R(x + d) with the border applied
    (ghost: 0 left of the image), every tap inside the image counted -> [3][H][W]"""
    left = np.asarray(left, np.int64)
    right = np.asarray(right, np.int64)
    out = []
    for d in (1, 2, 3):
        if mode == "toroidal":
            r = np.roll(right, d, axis=1)
        else:
            r = np.zeros_like(right)
            r[:, d:] = right[:, :right.shape[1] - d]
        out.append(_window_sums(np.abs(left - r), n, mode))
    return np.stack(out)


def wins_below_zero(left, right, best, square_width, mode, mistake):
    """the pixels where a position below shift 0 would take the arg-min (at equal sums its key is the smaller) if its sum
    started at MISTAKES[mistake](n) instead of above every real sum; `best` is the definition's best map -> bool [H][W].
    Pixel x has the positions -1 .. -((x - half) mod 4): its quads start at the dword that holds its window's first
    column.  (Ghost: the columns x < half are the strip kernel's, which has none.)"""
    n = window(square_width)
    half = n // 2
    x = np.arange(np.asarray(left).shape[1])
    has = np.stack([k <= ((x - half) & 3) for k in (1, 2, 3)])
    if mode != "toroidal":
        has &= x >= half
    bad = MISTAKES[mistake](n) + sums_below_zero(left, right, n, mode)
    return ((bad <= np.asarray(best, np.int64)[None]) & has[:, None, :]).any(axis=0)
