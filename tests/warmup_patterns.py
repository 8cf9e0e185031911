"""Edge images aimed at the warm-up of the bit-sliced match kernel's two-wave workgroups (csrc/sm_match_bs_kernel.h,
WT: a wave counts its half of the workgroup's shared window rows in one carry-save counter per shift, the two waves
swap their partial sums).  Checker only: imported by tests/, never by the product package.  The idea of
tests/extreme_patterns.py -- name a pattern after the corner of the mismatch count it drives -- applied to that
counter, whose wires are the taps (row r, column i) of the shared rows:

    none                both images 0: every count is 0 (best = taps, web = D)
    one_tap_k           eL has single 1s, eR is 0: a pixel whose window holds such a point matches at EVERY shift
                        with exactly one mismatching tap, so best = taps - 1 whichever shift wins; a dropped wire
                        gives taps, a wire counted at weight 2^k gives taps - 2^k.  The points of one image are
                        more than a window apart (no window holds two), and the images of a set together put one
                        on every image row: whichever rows a workgroup's waves share, every tap (r, i) of both
                        halves is the lone mismatch of some pixel.
    all_but_centre_k    the same points inverted (eL 1 except at the points, eR 0): only a point itself matches,
                        with ALL other taps mismatching -- count n^2 - 1, best = 1, and the half of the shared rows
                        that lies off the point's own row counts HALF * n, the counter's largest value, which
                        reaches its top plane.  With a point on every row both waves' halves get there.
    random_30, random_50_shift, skewed
                        i.i.d. images (0.3 against 0.3; 0.5 against itself moved by one shift less than the lane
                        count; 0.95 against 0.05): every view and shift index at once
"""
from __future__ import annotations

import numpy as np


def point_sets(w, h, n):
    """-> a list of (ys, xs) index arrays: single points, one on every image row, those of one set more than a
    window apart in x (also across the toroidal wrap), so that no n x n window holds two points of a set"""
    step = n + 1
    first = n // 2
    per = max(1, (w - first) // step)        # first + per * step <= w: the wrap keeps the distance as well
    xs_all = first + step * np.arange(per)
    sets = []
    for y0 in range(0, h, per):
        ys = np.arange(y0, min(h, y0 + per))
        sets.append((ys, xs_all[:len(ys)]))
    return sets


def warmup_batch(w, h, n, d, seed=0):
    """-> (names, eL stack, eR stack) of u8 {0, 1} images, h x w, for an n x n window and d shifts"""
    rng = np.random.default_rng([seed, w, h, n, d])
    zeros = np.zeros((h, w), np.uint8)
    names, left, right = ["none"], [zeros], [zeros]
    for k, (ys, xs) in enumerate(point_sets(w, h, n)):
        pts = zeros.copy()
        pts[ys, xs] = 1
        names += [f"one_tap_{k}", f"all_but_centre_{k}"]
        left += [pts, 1 - pts]
        right += [zeros, zeros]
    a = (rng.random((h, w)) < 0.5).astype(np.uint8)
    names += ["random_30", "random_50_shift", "skewed"]
    left += [(rng.random((h, w)) < 0.3).astype(np.uint8), a, (rng.random((h, w)) < 0.95).astype(np.uint8)]
    right += [(rng.random((h, w)) < 0.3).astype(np.uint8), np.roll(a, max(1, d - 2), axis=1),
              (rng.random((h, w)) < 0.05).astype(np.uint8)]
    return names, np.stack(left), np.stack(right)
