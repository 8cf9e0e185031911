"""Gray pairs for the cross-based matcher (sm_cross.hip).  Checker only, numpy only: imported by
tests/, never by the product package.

    occluder_scene   a textured ellipse (disparity d_front) in front of a textured background (d_back): the depth edge
                     is an intensity edge, which the arms stop at and a box window straddles
    edge_band        the pixels near a change of the true disparity, where the two kinds of support differ
    extremes         tests/census_extreme_patterns's pairs at the shapes that put E on 48 * 961 = 46128: the bound of
                     the u16 fields of the prefix sums and of the keys E << 16 | d
    regions          flat-ish blocks under a fine texture: arms of every length
    SMALL / MANY_TILES / MANY_SHIFTS   the shapes of tests/test_cross_shapes_gpu.py, with what each is there for
    MISTAKES         numpy forms of kernel mistakes that only a shape can tell (tests/test_cross_cpu.py proves it)
    wta_tile_walk    the left pass as k_cross_wta walks it (packed pairs, tile rows, sums modulo 2^16), with WALK_MISTAKES:
                     a carry or a borrow between the halves of a pair, which only the tall extreme can tell"""
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


def regions(w, h, n, seed):
    """n images of flat-ish blocks (5 x 3 pixels, four levels 50 apart) under a fine texture of 0 .. 11: gray
    differences at, below and above every tau of the tests, so arms of every length"""
    rng = np.random.default_rng(seed)
    blocks = np.kron(rng.integers(0, 4, (n, (h + 2) // 3, (w + 4) // 5)), np.ones((3, 5), np.int64))[:, :h, :w]
    return (50 * blocks + rng.integers(0, 12, (n, h, w))).astype(np.uint8)


def related_pairs(w, h, pairs, seed):
    """-> (left, right), uint8 (pairs, h, w): the right images are related to the left ones in half of the rows (real
    minima beside noise)"""
    left, right = regions(w, h, pairs, seed), regions(w, h, pairs, seed + 1)
    right[:, ::2] = np.roll(left, 2, axis=2)[:, ::2]
    return left, right


# (w, h, D, arm, tau) of tests/test_cross_gpu.py::test_every_map_is_exact: D in {1, 12, 130, 200} and D > W, both sizes
# (several tiles each way, ragged edges), every arm and tau of the lists
CASES = [(70, 45, 1, 3, 8), (70, 45, 12, 15, 255), (130, 37, 130, 0, 255), (130, 37, 200, 3, 40), (70, 45, 200, 15, 40),
         (130, 37, 12, 15, 8)]

# Small images, (w, h, D, arm): what k_cross_wta is never asked for from 64 columns on.  tw = 64 - 2 arm output columns
# and 32 rows a tile.
#   1 x 1, 1 x 40   W = 1: smn_mod(x + dlo, 1) in a second turn (D > 8), one and two tile rows
#   2 x 1, 5 x 3    W < 8 and D > 2 W: `while (xr >= W) xr -= W` runs up to 8 and 3 times; H < 32; W <= arm, H <= arm
#   7 x 33          W < 8, D > 2 W, a second tile row of one row
#   9 x 40          W <= arm: every output column within an arm's length of both borders; D > 3 W
#   33 x 31         one tile, one partial tile row (H < 32) and nothing else
#   35 x 33         arm 15: tw = 34, so a second tile of ONE column (and a second tile row of one row)
#   65 x 33         arm 0: tw = 64, a second tile of one column
# Ghost: at every one of these W < 64 + D, so the test `xr < W` in front of the right-descriptor load decides.
SMALL = [(1, 1, 11, 15), (2, 1, 20, 15), (1, 40, 9, 15), (5, 3, 20, 15), (7, 33, 17, 15), (9, 40, 30, 15),
         (33, 31, 12, 15), (35, 33, 12, 15), (65, 33, 9, 0)]
SMALL_TAUS = (12, 255)

# Many tiles: 200 x 70 at arm 15 is 6 x 3 = 18 tiles a pair, above 8 and no multiple of 8 (sm_xcd_tile permutes them);
# D = 11 is odd, so the second turn is partial (shifts 8, 9 and a lone 10: `two == false` in a turn after the first)
MANY_TILES = (200, 70, 11, 15, 40)

# Many shifts, (D, true move of each of the 5 rows): 530 x 5, arm 15, tau 40.  right(x + m) = left(x) in a row moved by
# m, so web = m + 1 where the row's neighbours do not spoil the descriptor: 512 = D, 301, 256 (the last index of 8 bits)
# and, at D = 257, 257 = D
MANY_SHIFTS_W, MANY_SHIFTS_H, MANY_SHIFTS_ARM, MANY_SHIFTS_TAU = 530, 5, 15, 40
MANY_SHIFTS = {512: (511, 511, 300, 300, 255), 257: (256, 256, 100, 255, 255)}


def many_shifts_pair(num_shifts):
    """-> (left, right) uint8 (5, 530): noise, each row of the right image the left row moved by its own shift"""
    rng = np.random.default_rng(num_shifts)
    left = rng.integers(0, 256, (MANY_SHIFTS_H, MANY_SHIFTS_W)).astype(np.uint8)
    right = np.stack([np.roll(left[r], m) for r, m in enumerate(MANY_SHIFTS[num_shifts])])
    return left, right


def wta_index_of_8_bits(e):
    """the arg-min of a volume e (D, h, w) by keys E << 16 | (d & 255): what k_cross_wta would give if its key kept
    eight bits of the shift -> (best, web)"""
    e = np.asarray(e, np.int64)
    d = np.arange(e.shape[0], dtype=np.int64) & 255
    k = (e << 16 | d[:, None, None]).min(0)
    return (k >> 16).astype(np.int32), ((k & 0xffff) + 1).astype(np.int32)


# a mistake no map of D <= 256 can show: tests/test_cross_cpu.py holds it against CASES (the same maps) and MANY_SHIFTS
# (other maps)
MISTAKES = {"index of 8 bits": wta_index_of_8_bits}

# Column sums past 2^16: k_cross_wta walks a tile's 32 + 2 arm rows with prefix sums Q modulo 2^16.  A tile holds at most
# H rows of the image, and the extremes above have 42: 42 * 31 * 48 = 62496 < 2^16, so their Q never wraps.  At 77 rows
# (a multiple of 7, so the lattice still continues itself) the second tile row holds 60 image rows of H = 31 * 48 = 1488:
# Q reaches 89280 and both the wrapped and the unwrapped differences occur.  D = 2 puts a second shift into the high half.
TALL_W, TALL_H, TALL_D = 98, 77, 2


def wta_tile_walk(left, right, num_shifts, census, tau, arm, mode, mistake=None):
    """the left pass as k_cross_wta walks it, in numpy: shifts in packed pairs (d | d + 1 << 16), a tile row of 32 output
    rows with a halo of `arm`, the pair's row sums H summed down the tile's 32 + 2 arm rows into Q modulo 2^16 in each
    half, E = Q[r + dn] - Q[r - u - 1] in each half, keys E << 16 | d -> (best, web).  mistake: None (the kernel; equal to
    tests/cross_reference.wta wherever E < 2^16), "carry" (Q summed as one 32-bit word: the first shift's half carries
    into the second's) or "borrow" (the difference taken as one 32-bit subtraction: it borrows from the second's)."""
    from tests import census_reference as cr
    from tests import cross_reference as x
    l, r, u, dn = x.arms(left, tau, arm)
    h, w = l.shape
    zero = np.zeros_like(l)
    cl, crr = cr.transform(left, census, mode), cr.transform(right, census, mode)
    sh = 32 + 2 * arm
    key = np.full((h, w), 0xffffffff, np.int64)
    for d in range(0, num_shifts, 2):
        two = d + 1 < num_shifts
        rows = [x.aggregate(cr.costs(cl, crr, s, mode), (l, r, zero, zero)) if s < num_shifts else zero for s in (d, d + 1)]
        for y_out in range(0, h, 32):
            ys = np.arange(y_out - arm, y_out - arm + sh)
            inside = (ys >= 0) & (ys < h)
            hs = [np.where(inside[:, None], rw[np.clip(ys, 0, h - 1)], 0) for rw in rows]
            if mistake == "carry":
                q = (hs[0] | hs[1] << 16).cumsum(0) & 0xffffffff
            else:
                q = (hs[0].cumsum(0) & 0xffff) | (hs[1].cumsum(0) & 0xffff) << 16
            q = np.concatenate([np.zeros((1, w), np.int64), q])              # q[k + 1] is tile row k; q[0]: rl < 0
            n = min(32, h - y_out)
            rr = arm + np.arange(n)[:, None]
            hi = np.take_along_axis(q, rr + dn[y_out:y_out + n] + 1, 0)
            lo = np.take_along_axis(q, rr - u[y_out:y_out + n], 0)
            if mistake == "borrow":
                e = (hi - lo) & 0xffffffff
            else:
                e = ((hi & 0xffff) - (lo & 0xffff) & 0xffff) | ((hi >> 16) - (lo >> 16) & 0xffff) << 16
            k0, k1 = (e & 0xffff) << 16 | d, (e & 0xffff0000) | (d + 1) if two else 0xffffffff
            key[y_out:y_out + n] = np.minimum(key[y_out:y_out + n], np.minimum(k0, k1))
    return (key >> 16).astype(np.int32), ((key & 0xffff) + 1).astype(np.int32)


# mistakes in the modular walk that show only where a tile's column sums pass 2^16 AND the second shift of a pair wins:
# tests/test_cross_cpu.py holds them against CASES and the 42-row extremes (the same maps) and the tall extreme (others)
WALK_MISTAKES = ("carry", "borrow")
