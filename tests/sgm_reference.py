"""Semi-global matching over the census data term written out in numpy (include/stereo_hip.h sm_sgm_*, DESIGN.md
section 14).  Checker only: imported by tests/, never by the product package.

    A(p, d)   = census window cost (tests/census_reference.window_costs), d = 0 .. D - 1
    L_r(p, d) = A(p, d)                                                          if q = p - r lies outside the image
              = A(p, d) + min(L_r(q, d), L_r(q, d -+ 1) + P1, m_q + P2) - m_q    else, m_q = min_k L_r(q, k)
                (terms with d -+ 1 outside 0 .. D - 1 dropped; paths never wrap, in either border mode)
    S = sum of L_r over the 4 or 8 directions; best = min_d S, web = 1 + the first d reaching it
    sub = the SSD (parabola) rule of tests/subpix_reference on S(s-2), S(s-1), S(s), s = web
    (best_right, web_right) = mirror(sgm(mirror(R), mirror(L)))

The vectorised form loops over the steps along a direction and works on whole rows (or columns) of lines x shifts at
once, in int32.  The *_bruteforce functions follow every path pixel by pixel, so that the CPU suite can pin the
vectorised form on tiny images."""
from __future__ import annotations

import numpy as np

from tests import census_reference as cr
from tests.lr_reference import lr_check, mirror

__all__ = ["DIRS", "data_term", "aggregate", "sgm", "right_reference", "expected", "lr_check", "mirror",
           "data_term_bruteforce", "sgm_bruteforce"]

DIRS = {4: [(1, 0), (-1, 0), (0, 1), (0, -1)],
        8: [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1)]}
BIG = np.int32(1 << 29)


def data_term(left, right, num_shifts, square_width, census, mode="toroidal"):
    """-> int32 (h, w, D) census window costs"""
    cl, cr_ = cr.transform(left, census, mode), cr.transform(right, census, mode)
    return np.stack([cr.window_costs(left, right, d, square_width, census, mode, cl, cr_)
                     for d in range(num_shifts)], axis=-1).astype(np.int32)


def _step(a, lq, valid, p1, p2):
    """L of a slice of pixels (n, D) from their predecessors' L (n, D); valid: the predecessor is in the image"""
    m = lq.min(axis=1, keepdims=True)
    lo = np.full_like(lq, BIG)
    hi = np.full_like(lq, BIG)
    lo[:, 1:] = lq[:, :-1]
    hi[:, :-1] = lq[:, 1:]
    t = np.minimum(np.minimum(lq, np.minimum(lo, hi) + p1), m + p2) - m
    return np.where(valid[:, None], a + t, a)


def path(a, dx, dy, p1, p2):
    """-> int32 (h, w, D) L_r of one direction r = (dx, dy)"""
    h, w, _ = a.shape
    L = np.zeros_like(a)
    if dy != 0:
        ys = range(h) if dy > 0 else range(h - 1, -1, -1)
        xs = np.arange(w)
        xq = xs - dx
        inside = (xq >= 0) & (xq < w)
        for y in ys:
            yq = y - dy
            if not 0 <= yq < h:
                L[y] = a[y]
                continue
            lq = L[yq][np.clip(xq, 0, w - 1)]
            L[y] = _step(a[y], lq, inside, p1, p2)
    else:
        xs = range(w) if dx > 0 else range(w - 1, -1, -1)
        for x in xs:
            xq = x - dx
            if not 0 <= xq < w:
                L[:, x] = a[:, x]
                continue
            L[:, x] = _step(a[:, x], L[:, xq], np.ones(h, bool), p1, p2)
    return L


def aggregate(a, p1, p2, paths):
    """-> int32 (h, w, D) S"""
    return sum(path(a, dx, dy, p1, p2) for dx, dy in DIRS[paths]).astype(np.int32)


def winner(s):
    """-> (best, web, sub) of an aggregate volume S (h, w, D)"""
    D = s.shape[-1]
    d = np.argmin(s, axis=-1)
    best = np.take_along_axis(s, d[..., None], -1)[..., 0].astype(np.int64)
    web = (d + 1).astype(np.int32)
    sub = 16 * web.astype(np.int64)
    inner = (web > 1) & (web < D)
    if inner.any():
        dm = np.clip(d - 1, 0, D - 1)
        dp = np.clip(d + 1, 0, D - 1)
        a = np.take_along_axis(s, dm[..., None], -1)[..., 0].astype(np.int64) - best
        b = np.take_along_axis(s, dp[..., None], -1)[..., 0].astype(np.int64) - best
        den = a + b
        ok = inner & (den > 0)
        q = np.zeros_like(sub)
        q[ok] = np.floor_divide(16 * (a[ok] - b[ok]) + den[ok], 2 * den[ok])
        sub = sub + np.clip(q, -8, 8)
    return best.astype(np.int32), web, sub.astype(np.int16)


def sgm(left, right, num_shifts, square_width, census, p1, p2, paths, mode="toroidal"):
    """-> (best int32, web int32, sub int16) of one gray pair"""
    a = data_term(left, right, num_shifts, square_width, census, mode)
    return winner(aggregate(a, p1, p2, paths))


def right_reference(left, right, num_shifts, square_width, census, p1, p2, paths, mode="toroidal"):
    """-> (best_right, web_right), by the definition: SGM of the mirrored images, mirrored back"""
    best, web, _ = sgm(mirror(right), mirror(left), num_shifts, square_width, census, p1, p2, paths, mode)
    return mirror(best), mirror(web)


def expected(left, right, num_shifts, square_width, census, p1, p2, paths, mode, max_diff):
    """every map of sm_sgm_wta / sm_sgm_wta_right / sm_sgm_lr for one gray pair"""
    best, web, sub = sgm(left, right, num_shifts, square_width, census, p1, p2, paths, mode)
    best_right, web_right = right_reference(left, right, num_shifts, square_width, census, p1, p2, paths, mode)
    checked, rejected = lr_check(web, web_right, max_diff, mode)
    sub_checked = np.where(checked == 0, 0, sub).astype(np.int16)
    return dict(best=best, web=web, sub=sub, best_right=best_right, web_right=web_right, checked=checked,
                rejected=rejected, sub_checked=sub_checked)


# ---------------------------------------------------------------------------
# pixel by pixel
# ---------------------------------------------------------------------------

def data_term_bruteforce(left, right, num_shifts, square_width, census, mode="toroidal"):
    cl, cr_ = cr.transform_bruteforce(left, census, mode), cr.transform_bruteforce(right, census, mode)
    h, w = cl.shape
    half = square_width // 2

    def cost(x, y, d):
        if mode == "toroidal":
            return bin(int(cl[y % h, x % w]) ^ int(cr_[y % h, (x % w + d) % w])).count("1")
        if not (0 <= x < w and 0 <= y < h):
            return 0
        r = int(cr_[y, x + d]) if x + d < w else 0
        return bin(int(cl[y, x]) ^ r).count("1")

    a = np.zeros((h, w, num_shifts), np.int64)
    for y in range(h):
        for x in range(w):
            for d in range(num_shifts):
                a[y, x, d] = sum(cost(x + tx, y + ty, d) for ty in range(-half, half + 1)
                                 for tx in range(-half, half + 1))
    return a


def sgm_bruteforce(left, right, num_shifts, square_width, census, p1, p2, paths, mode="toroidal"):
    """-> (best, web, sub): every path followed from its first pixel, one pixel and one shift at a time"""
    a = data_term_bruteforce(left, right, num_shifts, square_width, census, mode)
    h, w, D = a.shape
    s = np.zeros((h, w, D), np.int64)
    for dx, dy in DIRS[paths]:
        for y0 in range(h):
            for x0 in range(w):
                if 0 <= x0 - dx < w and 0 <= y0 - dy < h:
                    continue                                # not the first pixel of a line
                x, y, prev = x0, y0, None
                while 0 <= x < w and 0 <= y < h:
                    cur = []
                    for d in range(D):
                        if prev is None:
                            cur.append(int(a[y, x, d]))
                            continue
                        m = min(prev)
                        c = [prev[d], m + p2]
                        if d > 0:
                            c.append(prev[d - 1] + p1)
                        if d < D - 1:
                            c.append(prev[d + 1] + p1)
                        cur.append(int(a[y, x, d]) + min(c) - m)
                    for d in range(D):
                        s[y, x, d] += cur[d]
                    prev = cur
                    x, y = x + dx, y + dy
    best = np.zeros((h, w), np.int32)
    web = np.zeros((h, w), np.int32)
    sub = np.zeros((h, w), np.int16)
    for y in range(h):
        for x in range(w):
            v = [int(t) for t in s[y, x]]
            b = min(v)
            k = v.index(b)
            sv = k + 1
            q = 0
            if 1 < sv < D:
                aa, bb = v[k - 1] - b, v[k + 1] - b
                den = aa + bb
                if den > 0:
                    q = max(-8, min(8, (16 * (aa - bb) + den) // (2 * den)))
            best[y, x], web[y, x], sub[y, x] = b, sv, 16 * sv + q
    return best, web, sub
