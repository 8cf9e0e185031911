"""Gray pairs for the cross-based matcher (sm_cross.hip).  Checker only, numpy only: imported by
tests/, never by the product package.

    occluder_scene   a textured ellipse (disparity d_front) in front of a textured background (d_back): the depth edge
                     is an intensity edge, which the arms stop at and a box window straddles
    edge_band        the pixels near a change of the true disparity, where the two kinds of support differ
    extremes         tests/census_extreme_patterns's pairs at the shapes that put E on 48 * 961 = 46128: the bound of
                     the u16 fields of the prefix sums and of the keys E << 16 | d"""
from __future__ import annotations

import numpy as np

from tests.census_extreme_patterns import anti, lattice, rows_anti          # noqa: F401  (reused as they are)

# anti(98, 42, k), toroidal, c = 7, tau = 255, L = 15: every interior pixel's support is the full 31 x 31 cross
EXTREME_W, EXTREME_H = 98, 42
EXTREME_INTERIOR = (EXTREME_W - 30) * (EXTREME_H - 30)   # 816 pixels at least 15 from every image border
E_MAX = 48 * 961


def occluder_scene(w, h, seed, d_back, d_front):
    """-> (left, right, true disparity)"""
    rng = np.random.default_rng(seed)

    def tex(base):
        t = rng.integers(-24, 25, (h, w))
        return base + (t + np.roll(t, 1, 1) + np.roll(t, 1, 0) + np.roll(t, (1, 1), (0, 1))) // 4
    back, front = tex(80), tex(170)
    yy, xx = np.mgrid[0:h, 0:w]
    inside = ((xx - 0.5 * w) / (0.22 * w)) ** 2 + ((yy - 0.5 * h) / (0.3 * h)) ** 2 < 1
    left = np.where(inside, front, back)
    moved = np.roll(np.where(inside, front, -1), d_front, axis=1)
    right = np.where(moved >= 0, moved, np.roll(back, d_back, axis=1)) + rng.integers(-2, 3, (h, w))
    return left.astype(np.uint8), np.clip(right, 0, 255).astype(np.uint8), np.where(inside, d_front, d_back)


def edge_band(truth, reach=4, margin=12):
    """the pixels within `reach` (Chebyshev) of a change of the true disparity -- a pixel whose disparity differs from
    that of its left or of its upper neighbour -- without `margin` outer columns a side"""
    t = np.asarray(truth)
    h, w = t.shape
    change = np.zeros((h, w), bool)
    change[:, 1:] |= t[:, 1:] != t[:, :-1]
    change[1:] |= t[1:] != t[:-1]
    p = np.pad(change, reach)
    near = np.zeros((h, w), bool)
    for dy in range(2 * reach + 1):
        for dx in range(2 * reach + 1):
            near |= p[dy:dy + h, dx:dx + w]
    near[:, :margin] = False
    near[:, w - margin:] = False
    return near
