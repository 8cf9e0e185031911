"""The census cost mode written out in numpy (include/stereo_hip.h sm_census_*).  Checker only:
imported by tests/, never by the product package.

    C_I(x, y) bit k = I(x + dx, y + dy) < I(x, y), the k-th neighbour of the c x c window (row-major, (0, 0) skipped)
                      toroidal: coordinates wrap;  ghost: a neighbour outside the image reads 0
    c_d(x, y)       = popcount(C_L(x, y) ^ C_R(x + d, y))      toroidal: x + d mod W;  ghost: C_R = 0 for x + d >= W
    A_d             = n x n window sum of c_d (toroidal: taps wrap; ghost: taps outside the image count 0)
    best = min_d A_d, web = 1 + the first d reaching it
    (best_right, web_right) = mirror(wta(mirror(R), mirror(L)))             mirror(a)(x) = a(W-1-x)
    refine: tests/subpix_reference's SAD (equiangular) fit on C(s-2), C(s-1), C(s)

The *_bruteforce functions restate the transform and the arg-min pixel by pixel, so that the CPU suite can pin the
vectorised forms on tiny images."""
from __future__ import annotations

import numpy as np

from tests import subpix_reference as sr
from tests.cost_lr_reference import _box
from tests.lr_reference import lr_check, mirror

__all__ = ["transform", "costs", "wta", "wta_from_descriptors", "right_reference", "refine", "expected",
           "expected_rows", "lr_check", "mirror", "transform_bruteforce", "wta_bruteforce"]


def transform(img, c, mode="toroidal"):
    """-> uint64 (h, w) descriptors of one gray image"""
    img = np.asarray(img, np.int32)
    h, w = img.shape
    hc = c // 2
    if mode == "toroidal":
        p = img[np.arange(-hc, h + hc) % h][:, np.arange(-hc, w + hc) % w]
    else:
        p = np.pad(img, hc)
    out = np.zeros((h, w), np.uint64)
    k = 0
    for dy in range(-hc, hc + 1):
        for dx in range(-hc, hc + 1):
            if dy == 0 and dx == 0:
                continue
            nb = p[hc + dy:hc + dy + h, hc + dx:hc + dx + w]
            out |= (nb < img).astype(np.uint64) << np.uint64(k)
            k += 1
    return out


def costs(cl, cr, d, mode="toroidal"):
    """-> int64 (h, w) Hamming costs c_d of two descriptor images"""
    h, w = cl.shape
    if mode == "toroidal":
        r = np.roll(cr, -d, axis=1)                      # r(x) = C_R((x + d) mod W)
    else:
        r = np.zeros_like(cr)
        if d < w:
            r[:, :w - d] = cr[:, d:]
    return np.bitwise_count(cl ^ r).astype(np.int64)


def wta_from_descriptors(cl, cr, num_shifts, square_width, mode="toroidal"):
    """-> (best int32, web int32) of the arg-min over the shifts, first shift wins"""
    n = 2 * (square_width // 2) + 1
    h, w = cl.shape
    best = np.full((h, w), np.iinfo(np.int64).max, np.int64)
    web = np.zeros((h, w), np.int32)
    for d in range(num_shifts):
        total = _box(costs(cl, cr, d, mode), n, mode)
        upd = total < best
        best[upd] = total[upd]
        web[upd] = d + 1
    return best.astype(np.int32), web


def wta(left, right, num_shifts, square_width, census, mode="toroidal"):
    return wta_from_descriptors(transform(left, census, mode), transform(right, census, mode), num_shifts,
                                square_width, mode)


def right_reference(left, right, num_shifts, square_width, census, mode="toroidal"):
    """-> (best_right, web_right), by the definition: the arg-min of the mirrored images, mirrored back"""
    best, web = wta(mirror(right), mirror(left), num_shifts, square_width, census, mode)
    return mirror(best), mirror(web)


def window_costs(left, right, d, square_width, census, mode="toroidal", cl=None, cr=None):
    """-> int64 (h, w) window costs A_d"""
    n = 2 * (square_width // 2) + 1
    cl = transform(left, census, mode) if cl is None else cl
    cr = transform(right, census, mode) if cr is None else cr
    return _box(costs(cl, cr, d, mode), n, mode)


def refine(left, right, web, num_shifts, square_width, census, mode="toroidal"):
    """-> (sub int16, costs int32 (3, h, w)) of one pair: C(s-2), C(s-1), C(s), -1 where a shift or the pixel has none"""
    cl, cr = transform(left, census, mode), transform(right, census, mode)
    s = np.asarray(web, np.int64)
    valid = (s >= 1) & (s <= num_shifts)
    c = np.full((3,) + s.shape, -1, np.int64)
    for k in range(3):
        d = s - 2 + k
        ok = valid & (d >= 0) & (d < num_shifts)
        for dv in np.unique(d[ok]):
            m = ok & (d == dv)
            c[k][m] = window_costs(left, right, int(dv), square_width, census, mode, cl, cr)[m]
    sub = sr.subpixel(c[0], c[1], c[2], s, num_shifts, "sad")
    return sub, c.astype(np.int32)


def expected(left, right, num_shifts, square_width, census, mode, max_diff):
    """the left map / costs, the right-reference map / costs and the checked map of one gray pair"""
    best, web = wta(left, right, num_shifts, square_width, census, mode)
    best_right, web_right = right_reference(left, right, num_shifts, square_width, census, mode)
    checked, rejected = lr_check(web, web_right, max_diff, mode)
    return dict(best=best, web=web, best_right=best_right, web_right=web_right, checked=checked, rejected=rejected)


def expected_rows(left, right, num_shifts, square_width, census, mode, y0, y1):
    """best / web / web_right of rows y0 .. y1 - 1 of a large pair, from a band with the rows the descriptors and the
    window reach (a band's own border rows are wrong, and cut off)"""
    h = left.shape[0]
    m = square_width // 2 + census // 2
    if mode == "toroidal":
        rows, lo = np.arange(y0 - m, y1 + m) % h, m
    else:
        a, b = max(0, y0 - m), min(h, y1 + m)
        rows, lo = np.arange(a, b), y0 - a
    bl, br = left[rows], right[rows]
    best, web = wta(bl, br, num_shifts, square_width, census, mode)
    best_right, web_right = right_reference(bl, br, num_shifts, square_width, census, mode)
    band = slice(lo, lo + y1 - y0)
    return dict(best=best[band], web=web[band], best_right=best_right[band], web_right=web_right[band])


# ---------------------------------------------------------------------------
# pixel by pixel
# ---------------------------------------------------------------------------

def transform_bruteforce(img, c, mode="toroidal"):
    img = np.asarray(img, np.int64)
    h, w = img.shape
    hc = c // 2
    out = np.zeros((h, w), np.uint64)
    for y in range(h):
        for x in range(w):
            bits, k = 0, 0
            for dy in range(-hc, hc + 1):
                for dx in range(-hc, hc + 1):
                    if dy == 0 and dx == 0:
                        continue
                    yy, xx = y + dy, x + dx
                    if mode == "toroidal":
                        v = img[yy % h, xx % w]
                    else:
                        v = img[yy, xx] if 0 <= yy < h and 0 <= xx < w else 0
                    if v < img[y, x]:
                        bits |= 1 << k
                    k += 1
            out[y, x] = bits
    return out


def wta_bruteforce(left, right, num_shifts, square_width, census, mode="toroidal"):
    cl, cr = transform_bruteforce(left, census, mode), transform_bruteforce(right, census, mode)
    h, w = cl.shape
    half = square_width // 2

    def cost(x, y, d):
        if mode == "toroidal":
            r = int(cr[y % h, (x + d) % w])
            return bin(int(cl[y % h, x % w]) ^ r).count("1")
        if not (0 <= x < w and 0 <= y < h):
            return 0
        r = int(cr[y, x + d]) if x + d < w else 0
        return bin(int(cl[y, x]) ^ r).count("1")

    best = np.zeros((h, w), np.int32)
    web = np.zeros((h, w), np.int32)
    for y in range(h):
        for x in range(w):
            b, s = None, 0
            for d in range(num_shifts):
                a = sum(cost(x + tx, y + ty, d) for ty in range(-half, half + 1) for tx in range(-half, half + 1))
                if b is None or a < b:
                    b, s = a, d + 1
            best[y, x], web[y, x] = b, s
    return best, web
