"""Gray pairs built to reach the bounds the census and SGM kernels rest on (sm_census.hip, sm_sgm.hip; DESIGN.md
sections 13 and 14).  Checker only, numpy only: imported by tests/, never by the product package.

A census window cost is A <= (c^2 - 1) n^2: 48 * 625 = 30000 for the 7 x 7 census under a 25 x 25 window.
k_census_wta carries A in packed u16 fields (a shift outside a launch's range gets 0x8000 added to its field) and in
keys A << 16 | d; the SGM kernels store A as u16, carry L_r <= A + P2 <= 62767 and S <= 8 * 62767 = 502136 < 2^19 in
keys S << 8 | d.  Noise and natural scenes sit near half of A's range and far below the SGM bounds; the pairs here
sit on them:

    lattice      every 7 x 7 window holds 49 distinct values: no comparison of the transform ties
    anti         the right image is the inverted lattice moved by k: shift k costs (c^2 - 1) n^2 at every pixel
    rows_anti    rows of one value each, against their inverse: every shift of every pixel costs 42 n^2 (c = 7)
    comb         columns of two interleaved classes against their inverse: even shifts cost (about) the full window,
                 odd shifts next to nothing -- a cheap shift just past a range whose only shift costs 30000
    level pairs  all 0, all 255 and 0 / 255 images: the strict `<` against equal values and against the ghost halo

tests/test_census_extremes_cpu.py pins, against the numpy definitions, that these reach the bounds they name."""
from __future__ import annotations

import numpy as np

LEVEL_PATTERNS = ("both_0", "both_255", "black_white", "white_black", "two_level", "two_level_inverse",
                  "two_level_rows")


def lattice(w, h):
    """I(x, y) = 5 ((x + 7 y) mod 49), values 0 .. 240.

    The 49 pixels of a 7 x 7 window have x + 7 y running over 49 consecutive integers, so they hold 49 distinct
    values (and so do the 25 / 9 of every 5 x 5 / 3 x 3 window): no `<` of the transform compares equal values, and
    every descriptor bit is decided.  For w % 49 == 0 and h % 7 == 0 the image continues itself across the toroidal
    wrap (x + w and y + h leave (x + 7 y) mod 49 unchanged), so this holds at the borders too."""
    yy, xx = np.mgrid[0:h, 0:w]
    return (5 * ((xx + 7 * yy) % 49)).astype(np.uint8)


def anti(w, h, k):
    """left = lattice, right = the inverted lattice (255 - lattice, values 15 .. 255) rolled right by k columns.

    right(x + k) = 255 - left(x): all values of a window being distinct, every comparison of the right descriptor at
    x + k is the opposite of the left one's at x, so shift k costs c^2 - 1 bits at every pixel and, toroidal with
    w % 49 == 0 and h % 7 == 0, A_k = (c^2 - 1) n^2 everywhere: 30000 for c = 7, n = 25, the bound of the u16 fields
    of k_census_wta and of the u16 data term of SGM.  The lattice has period 49 in x, so every pixel's cost profile
    has period 49 in d (for c = 7, n = 25 it falls from 30000 at d = k to 14669 .. 14720 at (d - k) mod 49 = 24), and
    for D > 49 shifts 49 apart tie exactly, at a non-zero cost and, for D > 128, across the launches of k_census_wta:
    the first must win.  With k = D (mod w) the first shift past the range carries the maximum plus the 0x8000 bias;
    with k = 0 and k = D - 1 the maximum sits in the first and in the last lane of a launch.  In ghost mode, and at
    widths that break the lattice at the seam (100 x 30), the costs are lower near the borders but stay exact
    against the reference."""
    left = lattice(w, h)
    return left, np.ascontiguousarray(np.roll(255 - left, k % w, axis=1))


def rows_anti(w, h):
    """left(x, y) = 5 ((3 y) mod 49), right = 255 - left.

    A row holds one value: the 6 (c = 7) same-row comparisons of a descriptor are equal values, bit 0 in both images
    (the `<` is strict).  3 dy mod 49 != 0 for 0 < |dy| <= 6, so any 7 consecutive rows differ (for h % 49 == 0 across
    the wrap as well) and the other 42 comparisons are opposite in the two images.  Neither image depends on x, so
    toroidal every shift of every pixel costs (c^2 - c) n^2: 42 * 625 = 26250 for c = 7, n = 25.  An all-tie map at
    a high cost: web is 1 everywhere and best that constant for every D up to 512; under SGM every L_r, so S, is
    constant over d."""
    yy, _ = np.mgrid[0:h, 0:w]
    left = (5 * ((3 * yy) % 49)).astype(np.uint8)
    return left, (255 - left).astype(np.uint8)


def comb(w, h):
    """left(x, y) = 128 + 2 t at even x, 127 - 2 t at odd x, t = (x // 2 + 7 y) mod 49; right = 255 - left.

    The even columns lie above the odd ones, and t rises along one class where it falls along the other, so (away
    from the jumps of the mod) the descriptor of column x + 1 is the complement of that of column x; the right image
    complements them once more.  Toroidal with w % 98 == 0 and h % 7 == 0, shift 0 costs (c^2 - 1) n^2 at every pixel
    (30000 for c = 7, n = 25) and shift 1 a few hundred.  With D = 1 the only shift of the range costs 30000 while the
    unused shifts of the lane cost almost nothing: their biased fields (0x8000 + A) must still lose, which a smaller
    bias (0x4000 + 302 < 30000) would not manage."""
    yy, xx = np.mgrid[0:h, 0:w]
    t = (xx // 2 + 7 * yy) % 49
    left = np.where(xx % 2 == 0, 128 + 2 * t, 127 - 2 * t).astype(np.uint8)
    return left, (255 - left).astype(np.uint8)


def level_pair(name, w, h):
    """Pairs of images that hold only the levels 0 and 255.

    Equal neighbours give bit 0 on both sides of the strict `<`; in ghost mode the halo reads 0, which ties with a
    pixel of value 0 (bit 0) and is below 255 (bit 1: the border descriptors of a white image are not 0).  The
    two-level images (2 x 2 blocks / rows of 0 and 255) put the largest step of the value range into every
    comparison; against their inverse every comparison of unequal values differs."""
    yy, xx = np.mgrid[0:h, 0:w]
    zero = np.zeros((h, w), np.uint8)
    white = np.full((h, w), 255, np.uint8)
    blocks = np.where(((xx // 2) + (yy // 2)) % 2 == 0, 255, 0).astype(np.uint8)
    rows = np.where(yy % 2 == 0, 255, 0).astype(np.uint8)
    pairs = {"both_0": (zero, zero), "both_255": (white, white), "black_white": (zero, white),
             "white_black": (white, zero), "two_level": (blocks, np.roll(blocks, 1, axis=1)),
             "two_level_inverse": (blocks, (255 - blocks).astype(np.uint8)),
             "two_level_rows": (rows, (255 - rows).astype(np.uint8))}
    left, right = pairs[name]
    return np.ascontiguousarray(left), np.ascontiguousarray(right)


def bits(census):
    """descriptor bits of a census width: c^2 - 1"""
    return census * census - 1


def window(square_width):
    """the side of the window a square_width gives (even widths round up)"""
    return 2 * (square_width // 2) + 1
