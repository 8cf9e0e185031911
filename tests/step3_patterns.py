"""Maps with holes (0 pixels) for step 3 (fill_web_holes, min/max, draw_contour_map), shared by
tests/golden/make_golden.py --step3, which runs the reference's own step-3 functions on them
(oracle/ref_step3_driver.c), and by tests/test_step3_*.py.  Checker only: never imported by the
product package.

Every generator is a closed-form function of its arguments (numpy's seeded PCG64 included), so the
tests regenerate each fixture's input exactly.  Rows 0 and h - 1 of every map in CASES are free of
zeros: a hole there reads outside the array in the reference (undefined behaviour; the restatement
reads 0), so those rows are pinned to the restatement only (border_holes).  Values stay below 2^29
in magnitude, so no sum of four neighbours overflows."""
from __future__ import annotations

import numpy as np

LIMIT = 1 << 29          # |value| < LIMIT everywhere


def _base(w, h, seed, lo=1, hi=31):
    """a web-like map: values lo..hi-1, no zeros (lo >= 1 or hi <= 0)"""
    return np.random.default_rng(seed).integers(lo, hi, (h, w)).astype(np.int32)


def _interior(web):
    """the map with rows 0 and h - 1 made hole-free (a zero there becomes 1)"""
    for y in (0, web.shape[0] - 1):
        web[y][web[y] == 0] = 1
    return web


def edge_columns(w, h, seed):
    """holes in column 0 and column w - 1: the flat-index neighbour x - 1 of x = 0 is the previous
    row's last pixel, x + 1 of x = w - 1 the next row's first; some pairs of them are holes too"""
    web = _base(w, h, seed)
    web[1:h - 1:2, 0] = 0
    web[2:h - 1:3, w - 1] = 0
    web[4, w - 1] = web[5, 0] = 0            # (w-1, 4) and (0, 5) are flat neighbours
    web[7, w - 1] = 0
    web[8, 0] = 0
    web[7, w - 2] = 0                        # and a run across the wrap
    return web


def singles(w, h, seed):
    """isolated single holes"""
    web = _base(w, h, seed)
    rng = np.random.default_rng(seed + 1)
    ys = rng.integers(1, h - 1, 40)
    xs = rng.integers(0, w, 40)
    web[ys, xs] = 0
    return web


def blocks2x2(w, h, seed):
    web = _base(w, h, seed)
    for y, x in ((1, 0), (3, 5), (10, 11), (h - 3, w - 2), (6, w // 2)):
        web[y:y + 2, x:x + 2] = 0
    return web


def runs(w, h, seed):
    """a horizontal run over almost a whole row, a whole interior row, and vertical runs"""
    web = _base(w, h, seed)
    web[3, 1:w - 1] = 0
    web[h // 2, :] = 0
    web[1:h - 1, 4] = 0
    web[2:h - 2, w - 1] = 0
    return web


def big_block(w, h, seed):
    """one large block: `times` sweeps leave its middle 0"""
    web = _base(w, h, seed)
    web[5:h - 5, 6:w - 6] = 0
    return web


def persisting(w, h, seed):
    """holes whose four neighbours sum to less than 4 stay 0 through every sweep: dominoes in a
    field of 1s; beside them lone holes among 1s (filled to 1) and ordinary holes in a region of
    larger values"""
    web = np.ones((h, w), np.int32)
    web[1:h - 1:4, 2:w - 2:5] = 0            # lone holes among 1s: (1+1+1+1)/4 = 1, filled
    web[2:h - 1:4, 3:w - 3:6] = 0            # dominoes among 1s: (1+1+1+0)/4 = 0, persist
    web[2:h - 1:4, 4:w - 2:6] = 0
    web[h // 2:, w // 2:] = _base(w - w // 2, h - h // 2, seed, 2, 40)
    web[h // 2 + 2:h - 2:3, w // 2 + 1:w:4] = 0
    return _interior(web)


def checkerboard(w, h, seed):
    """holes on (x + y) even in rows 1 .. h - 2: for even w the flat neighbour x - 1 of x = 0 is a
    hole as well"""
    web = _base(w, h, seed)
    yy, xx = np.mgrid[0:h, 0:w]
    web[((xx + yy) % 2 == 0) & (yy > 0) & (yy < h - 1)] = 0
    return web


def negative(w, h, seed):
    """a caller-made map with negative values: the sums of many holes' neighbours are negative
    and not multiples of 4, where truncation toward zero (C's /) and >> 2 differ"""
    web = np.random.default_rng(seed).integers(-1000, 1000, (h, w)).astype(np.int32)
    web[web == 0] = -3
    rng = np.random.default_rng(seed + 1)
    web[rng.integers(1, h - 1, 60), rng.integers(0, w, 60)] = 0
    web[2, 0:3] = (-5, 0, -2)                # (x=1, y=2): a hole whose neighbours sum to -5 - 2 + ...
    web[1, 1] = -1
    web[3, 1] = 3
    return _interior(web)


def extreme(w, h, seed):
    """values at +-(2^29 - 1): sums of four reach +-(2^31 - 4), the contour range 2^30 - 2"""
    web = np.where(np.random.default_rng(seed).random((h, w)) < 0.5, LIMIT - 1, -(LIMIT - 1)).astype(np.int32)
    web[1:h - 1:3, ::4] = 0
    web[2:h - 1:5, 1::3] = 0
    return _interior(web)


def constant(w, h, seed, value=5):
    """a constant map with lone holes: the holes fill to `value`, so the filled map's contour
    interval is 0 (the reference traps) while the unfilled map's, with its 0s, need not be"""
    web = np.full((h, w), value, np.int32)
    web[2:h - 1:3, 1::4] = 0
    return web


def mixed(w, h, seed):
    """everything at once: edge columns, singles, a block, a run, dominoes of 1s"""
    web = singles(w, h, seed)
    web[1:h - 1:3, 0] = 0
    web[2:h - 1:4, w - 1] = 0
    web[4:9, 6:14] = 0
    web[h - 3, 2:w - 2] = 0
    web[h - 5, 1:4] = 1
    web[h - 5, 2] = 0
    return web


def lr_scene(w, h, seed, num_shifts=64, square_width=9, mode="toroidal", max_diff=0):
    """a real left-right-checked map of a make_pair scene, computed on the CPU (oracle + the numpy
    check of tests/lr_reference.py); its rejected pixels in rows 0 and h - 1 are given back their
    unchecked value"""
    from stereomatching_amd.synth import make_pair
    from tests import lr_reference as lr
    from tests import oracle
    left, right = make_pair(w, h, num_shifts, seed=seed)
    el = oracle.find_all_edges(left, 0.15, mode)
    er = oracle.find_all_edges(right, 0.15, mode)
    _, web = oracle.hot_path(el, er, num_shifts, square_width, mode)
    _, web_right = lr.right_reference(el, er, num_shifts, square_width, mode)
    checked, _ = lr.lr_check(web, web_right, max_diff, mode)
    for y in (0, h - 1):
        checked[y] = web[y]
    return checked


def no_positive(w, h, seed):
    """a caller-made map whose every value is below 0 (-1000 .. -11, both present): its maximum is negative, which a
    running maximum that starts at 0 instead of INT_MIN never reports (the mutation audit's Z4); with 10 lines the
    contour interval is 98, and 100 if the maximum were 0"""
    web = np.random.default_rng(seed).integers(-1000, -10, (h, w)).astype(np.int32)
    web[0, 0], web[-1, -1] = -1000, -11
    return web


# n = 185 (n % 4 = 1: k_minmax_zero's scalar tail, and the scalar loop for the second pair of a stack) and n = 256
# (16-byte loads throughout)
NO_POSITIVE_SHAPES = ((37, 5), (64, 4))
MISTAKES = ("maximum starts at 0",)


def min_max_with(web, mistake):
    """(min, max) of a map with the mistake made"""
    assert mistake in MISTAKES
    return int(web.min()), max(int(web.max()), 0)


def with_pattern(fn, w, h, seed):
    return np.ascontiguousarray(fn(w, h, seed), np.int32)


# name: (generator, w, h, seed, times, lines).  Shapes: n = w * h covers n % 4 = 0, 1, 2, 3
# (37x23: 3, 41x29: 1, 50x31: 2, 64x48: 0, 33x35: 3, 256x192: 0).
CASES = {
    "edge_columns_t1":   (edge_columns, 37, 23, 1, 1, 10),
    "edge_columns_t2":   (edge_columns, 37, 23, 1, 2, 10),
    "edge_columns_t3":   (edge_columns, 64, 48, 2, 3, 7),
    "singles_t2":        (singles, 41, 29, 3, 2, 10),
    "singles_t32":       (singles, 41, 29, 3, 32, 10),
    "blocks2x2_t3":      (blocks2x2, 50, 31, 4, 3, 5),
    "blocks2x2_t32":     (blocks2x2, 50, 31, 4, 32, 10),
    "runs_t2":           (runs, 64, 48, 5, 2, 10),
    "runs_t101":         (runs, 64, 48, 5, 101, 10),
    "big_block_t32":     (big_block, 64, 48, 6, 32, 10),
    "big_block_t3":      (big_block, 33, 35, 6, 3, 4),
    "persisting_t2":     (persisting, 64, 48, 7, 2, 3),
    "persisting_t101":   (persisting, 50, 31, 7, 101, 3),
    "checkerboard_t1":   (checkerboard, 37, 23, 8, 1, 10),
    "checkerboard_t2":   (checkerboard, 64, 48, 8, 2, 10),
    "checkerboard_t32":  (checkerboard, 41, 29, 8, 32, 10),
    "negative_t2":       (negative, 41, 29, 9, 2, 10),
    "negative_t3":       (negative, 50, 31, 9, 3, 13),
    "negative_t32":      (negative, 37, 23, 9, 32, 10),
    "extreme_t2":        (extreme, 33, 35, 10, 2, 10),
    "extreme_t101":      (extreme, 41, 29, 10, 101, 3),
    "mixed_t0":          (mixed, 37, 23, 11, 0, 10),
    "mixed_t1":          (mixed, 37, 23, 11, 1, 10),
    "mixed_t2":          (mixed, 37, 23, 11, 2, 10),
    "mixed_t3":          (mixed, 37, 23, 11, 3, 10),
    "mixed_t32":         (mixed, 37, 23, 11, 32, 10),
    "mixed_t101":        (mixed, 37, 23, 11, 101, 10),
    # zero contour intervals (the reference traps): filled range 0 with an unfilled range of 5
    # (lines 2: interval 2 before filling); the unfilled map itself (times 0: range 5, lines 10); lines 0
    "zero_after_fill_t2":  (constant, 41, 29, 12, 2, 2),
    "zero_unfilled_t0":    (constant, 41, 29, 12, 0, 10),
    "zero_lines_t2":       (mixed, 37, 23, 11, 2, 0),
    "lr_scene_t32":      (lr_scene, 256, 192, 13, 32, 10),
    "lr_scene_t3":       (lr_scene, 256, 192, 13, 3, 10),
}


def case(name):
    """-> (map, times, lines) of one named case"""
    fn, w, h, seed, times, lines = CASES[name]
    return with_pattern(fn, w, h, seed), times, lines


def border_holes(w, h, seed):
    """holes in rows 0 and h - 1 and at the very first and last pixel: neighbours outside the
    array, undefined in the reference, read as 0 by the restatement and the kernels"""
    web = _base(w, h, seed)
    web[0, ::3] = 0
    web[h - 1, 1::4] = 0
    web[0, 0] = web[h - 1, w - 1] = 0
    web[0, w - 1] = web[h - 1, 0] = 0
    web[1, 0] = web[h - 2, w - 1] = 0
    return web
