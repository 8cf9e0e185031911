"""Cross-based adaptive support over the census cost, written out in numpy (include/stereo_hip.h sm_cross_*, DESIGN.md
section 26).  Checker only: imported by tests/, never by the product package.  This file is the definition.

    arms      a_dir(p), dir in left, right, up, down: the largest l in 0 .. L such that every k = 1 .. l has p + k dir
              inside the image and |I(p + k dir) - I(p)| <= tau.  Arms never leave the image, in either border mode.
              packed: uint16 = l | r << 4 | u << 8 | d << 12
    support   N(x, y) = sum over y' = y - u(x, y) .. y + d(x, y) of l(x, y') + r(x, y') + 1          (N <= 961)
    cost      c_d = tests/census_reference.costs (toroidal: x + d wraps; ghost: C_R = 0 for x + d >= W)
              H_d(x, y) = sum over x' = x - l(x, y) .. x + r(x, y) of c_d(x', y)      arms of the LEFT image
              E_d(x, y) = sum over y' = y - u(x, y) .. y + d(x, y) of H_d(x, y')      E <= 48 * 961 = 46128
    results   best = min_d E_d, web = 1 + the first d reaching it,
              sub = tests/subpix_reference.subpixel(E(s-2), E(s-1), E(s), s, D, "sad")
    right     (best_right, web_right) = mirror(cross(mirror(R), mirror(L))): the arms of the right image

The *_bruteforce functions restate arms and arg-min pixel by pixel, so that the CPU suite can pin the vectorised
forms on tiny images."""
from __future__ import annotations

import numpy as np

from tests import census_reference as cr
from tests import subpix_reference as sr
from tests.lr_reference import lr_check, mirror

__all__ = ["arms", "pack", "unpack", "support", "aggregate", "volume", "wta", "right_reference", "expected",
           "arms_bruteforce", "wta_bruteforce", "lr_check", "mirror"]

MAX_ARM = 15
DIRS = ((0, -1), (0, 1), (-1, 0), (1, 0))                # (dy, dx) of left, right, up, down


def arms(img, tau, arm):
    """-> (l, r, u, d), int64 (h, w) each, by a loop over k"""
    img = np.asarray(img, np.int64)
    h, w = img.shape
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for dy, dx in DIRS:
        a = np.zeros((h, w), np.int64)
        alive = np.ones((h, w), bool)
        for k in range(1, arm + 1):
            y, x = yy + k * dy, xx + k * dx
            inside = (y >= 0) & (y < h) & (x >= 0) & (x < w)
            v = img[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]
            alive = alive & inside & (np.abs(v - img) <= tau)
            a += alive
        out.append(a)
    return tuple(out)


def pack(a):
    l, r, u, d = a
    return (l | r << 4 | u << 8 | d << 12).astype(np.uint16)


def unpack(p):
    p = np.asarray(p, np.int64)
    return p & 15, p >> 4 & 15, p >> 8 & 15, p >> 12 & 15


def aggregate(c, a):
    """the span sums of a plane c (h, w) over the supports of the arms a, by prefix sums -> int64 (h, w)"""
    l, r, u, d = a
    c = np.asarray(c, np.int64)
    h, w = c.shape
    yy, xx = np.mgrid[0:h, 0:w]
    p = np.zeros((h, w + 1), np.int64)
    p[:, 1:] = c.cumsum(1)
    hs = p[yy, xx + r + 1] - p[yy, xx - l]
    q = np.zeros((h + 1, w), np.int64)
    q[1:] = hs.cumsum(0)
    return q[yy + d + 1, xx] - q[yy - u, xx]


def support(a):
    """N of the definition -> int32 (h, w)"""
    return aggregate(np.ones(a[0].shape, np.int64), a).astype(np.int32)


def volume(left, right, num_shifts, census, tau, arm, mode="toroidal"):
    """-> E, int64 (D, h, w)"""
    cl, crr = cr.transform(left, census, mode), cr.transform(right, census, mode)
    a = arms(left, tau, arm)
    return np.stack([aggregate(cr.costs(cl, crr, d, mode), a) for d in range(num_shifts)])


def _wta(e):
    web0 = e.argmin(0)                                   # the first minimum
    best = np.take_along_axis(e, web0[None], 0)[0]
    return best.astype(np.int32), (web0 + 1).astype(np.int32)


def _sub(e, web):
    s = np.asarray(web, np.int64)
    num_shifts = e.shape[0]
    c = [np.take_along_axis(e, np.clip(s - 2 + k, 0, num_shifts - 1)[None], 0)[0] for k in range(3)]
    return sr.subpixel(c[0], c[1], c[2], s, num_shifts, "sad")


def wta(left, right, num_shifts, census, tau, arm, mode="toroidal", want_sub=False):
    """-> (best int32, web int32[, sub int16]) of one gray pair"""
    e = volume(left, right, num_shifts, census, tau, arm, mode)
    best, web = _wta(e)
    return (best, web, _sub(e, web)) if want_sub else (best, web)


def right_reference(left, right, num_shifts, census, tau, arm, mode="toroidal"):
    """-> (best_right, web_right), by the definition: the arg-min of the mirrored images, mirrored back"""
    best, web = wta(mirror(right), mirror(left), num_shifts, census, tau, arm, mode)
    return mirror(best), mirror(web)


def expected(left, right, num_shifts, census, tau, arm, mode, max_diff):
    """the left maps, the right-reference maps, the checked map and the subpixel map with 0 where rejected"""
    best, web, sub = wta(left, right, num_shifts, census, tau, arm, mode, want_sub=True)
    best_right, web_right = right_reference(left, right, num_shifts, census, tau, arm, mode)
    checked, rejected = lr_check(web, web_right, max_diff, mode)
    return dict(best=best, web=web, sub=sub, best_right=best_right, web_right=web_right, checked=checked,
                rejected=rejected, sub_checked=np.where(checked == 0, 0, sub).astype(np.int16))


# ---------------------------------------------------------------------------
# pixel by pixel
# ---------------------------------------------------------------------------

def arms_bruteforce(img, tau, arm):
    img = np.asarray(img, np.int64)
    h, w = img.shape
    out = np.zeros((4, h, w), np.int64)
    for y in range(h):
        for x in range(w):
            for i, (dy, dx) in enumerate(DIRS):
                n = 0
                while n < arm:
                    yy, xx = y + (n + 1) * dy, x + (n + 1) * dx
                    if not (0 <= yy < h and 0 <= xx < w) or abs(int(img[yy, xx]) - int(img[y, x])) > tau:
                        break
                    n += 1
                out[i, y, x] = n
    return tuple(out)


def wta_bruteforce(left, right, num_shifts, census, tau, arm, mode="toroidal"):
    """-> (best, web, support) with every sum taken tap by tap"""
    cl, crr = cr.transform_bruteforce(left, census, mode), cr.transform_bruteforce(right, census, mode)
    l, r, u, d = arms_bruteforce(left, tau, arm)
    h, w = cl.shape

    def cost(x, y, s):
        if mode == "toroidal":
            v = int(crr[y, (x + s) % w])
        else:
            v = int(crr[y, x + s]) if x + s < w else 0
        return bin(int(cl[y, x]) ^ v).count("1")

    best = np.zeros((h, w), np.int32)
    web = np.zeros((h, w), np.int32)
    size = np.zeros((h, w), np.int32)
    for y in range(h):
        for x in range(w):
            taps = [(xx, yy) for yy in range(y - u[y, x], y + d[y, x] + 1)
                    for xx in range(x - l[yy, x], x + r[yy, x] + 1)]
            size[y, x] = len(taps)
            b, s = None, 0
            for sh in range(num_shifts):
                e = sum(cost(xx, yy, sh) for xx, yy in taps)
                if b is None or e < b:
                    b, s = e, sh + 1
            best[y, x], web[y, x] = b, s
    return best, web, size
