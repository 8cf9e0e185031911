"""Banded SGM written out in numpy (include/stereo_hip.h sm_sgm_wta_near / _near_right / sm_sgm_near_lr, DESIGN.md
section 23).  Checker only: imported by tests/, never by the product package.  This file is the definition.

    prior     = an int32 web map: 1 + shift, 0 invalid; radius r in 1 .. 4
    K(p)      = { d : 0 <= d <= D - 1, |d - (prior(p) - 1)| <= r }, empty for prior(p) = 0   (near_reference.candidates)
    A(p, d)   = census window cost (tests/census_reference.window_costs), d in K(p)
    L_r(p, d) = A(p, d)                                   if q = p - r lies outside the image or K(q) is empty
              = A(p, d) + min(L_r(q, d)       if d in K(q),
                              L_r(q, d-1) + P1 if d-1 in K(q),
                              L_r(q, d+1) + P1 if d+1 in K(q),
                              m_q + P2) - m_q             else, m_q = min over K(q) of L_r(q, k)
                (paths never wrap, in either border mode; a pixel without a band breaks the path)
    S = sum of L_r over the 4 or 8 directions of sgm_reference.DIRS; best = min over K(p) of S, web = 1 + the least d
        of K(p) reaching it; K(p) empty: web = best = sub = 0
    sub = with d = web - 1: d - 1 and d + 1 both in K(p): the parabola rule of sgm_reference.winner on S(d-1), S(d),
          S(d+1); otherwise 16 web
    (best_right, web_right) = mirror(sgm_near(mirror(R), mirror(L), mirror(prior_right)))

The vectorised form holds L densely over d = 0 .. D - 1 with BIG outside K, and works on whole rows (or columns) of
lines at once.  sgm_near_loop follows every path pixel by pixel with the band as a dict, so that the CPU suite can pin
the vectorised form."""
from __future__ import annotations

import numpy as np

from tests import census_reference as cr
from tests.lr_reference import lr_check, mirror
from tests.near_reference import candidates
from tests.sgm_reference import DIRS

__all__ = ["BIG", "band", "data_term", "path", "aggregate", "winner", "sgm_near", "sgm_near_right", "expected",
           "sgm_near_loop", "mirror", "lr_check"]

BIG = np.int64(1) << 40


def band(prior, num_shifts, radius):
    """-> bool (h, w, D): d in K(p)"""
    lo, hi, has = candidates(prior, num_shifts, radius)
    d = np.arange(num_shifts)
    return has[..., None] & (lo[..., None] <= d) & (d <= hi[..., None])


def data_term(left, right, ink, square_width, census, mode="toroidal"):
    """-> int64 (h, w, D): the census window cost where d in K(p), 0 elsewhere"""
    cl, cr_ = cr.transform(left, census, mode), cr.transform(right, census, mode)
    a = np.zeros(ink.shape, np.int64)
    for d in range(ink.shape[-1]):
        m = ink[..., d]
        if m.any():
            a[..., d][m] = cr.window_costs(left, right, d, square_width, census, mode, cl, cr_)[m]
    return a


def _step(a, ink, lq, ok, p1, p2):
    """L (BIG outside K) of a slice of pixels (n, D) from their predecessors' lq; ok: the predecessor is in the image
    and has a band"""
    m = lq.min(axis=1, keepdims=True)
    lo = np.full_like(lq, BIG)
    hi = np.full_like(lq, BIG)
    lo[:, 1:] = lq[:, :-1]
    hi[:, :-1] = lq[:, 1:]
    t = np.minimum(np.minimum(lq, np.minimum(lo, hi) + p1), m + p2) - m
    return np.where(ink, np.where(ok[:, None], a + t, a), BIG)


def path(a, ink, dx, dy, p1, p2):
    """-> int64 (h, w, D): L_r of one direction r = (dx, dy), 0 outside K"""
    h, w, _ = a.shape
    has = ink.any(axis=-1)
    L = np.full(a.shape, BIG, np.int64)
    none = np.zeros(max(h, w), bool)
    if dy != 0:
        xq = np.arange(w) - dx
        inside = (xq >= 0) & (xq < w)
        xc = np.clip(xq, 0, w - 1)
        for y in (range(h) if dy > 0 else range(h - 1, -1, -1)):
            yq = y - dy
            if 0 <= yq < h:
                L[y] = _step(a[y], ink[y], L[yq][xc], inside & has[yq][xc], p1, p2)
            else:
                L[y] = _step(a[y], ink[y], L[y], none[:w], p1, p2)
    else:
        for x in (range(w) if dx > 0 else range(w - 1, -1, -1)):
            xq = x - dx
            if 0 <= xq < w:
                L[:, x] = _step(a[:, x], ink[:, x], L[:, xq], has[:, xq], p1, p2)
            else:
                L[:, x] = _step(a[:, x], ink[:, x], L[:, x], none[:h], p1, p2)
    return np.where(ink, L, 0)


def aggregate(a, ink, p1, p2, paths):
    """-> int64 (h, w, D): S, 0 outside K"""
    return sum(path(a, ink, dx, dy, p1, p2) for dx, dy in DIRS[paths])


def winner(s, ink):
    """-> (best int32, web int32, sub int16) of an aggregate volume S (h, w, D) and its bands"""
    D = s.shape[-1]
    has = ink.any(axis=-1)
    d = np.argmin(np.where(ink, s, BIG), axis=-1)           # the first minimum: the least d

    def at(k):
        return np.take_along_axis(s, np.clip(k, 0, D - 1)[..., None], -1)[..., 0]

    def inside(k):
        return (k >= 0) & (k < D) & np.take_along_axis(ink, np.clip(k, 0, D - 1)[..., None], -1)[..., 0]
    best = at(d)
    web = d + 1
    a, b = at(d - 1) - best, at(d + 1) - best
    den = a + b
    ok = has & inside(d - 1) & inside(d + 1) & (den > 0)
    q = np.zeros_like(best)
    q[ok] = np.floor_divide(16 * (a[ok] - b[ok]) + den[ok], 2 * den[ok])
    sub = 16 * web + np.clip(q, -8, 8)
    return (np.where(has, best, 0).astype(np.int32), np.where(has, web, 0).astype(np.int32),
            np.where(has, sub, 0).astype(np.int16))


def sgm_near(left, right, prior, num_shifts, square_width, census, p1, p2, paths, radius, mode="toroidal"):
    """-> (best int32, web int32, sub int16) of one gray pair and its prior map"""
    ink = band(prior, num_shifts, radius)
    a = data_term(left, right, ink, square_width, census, mode)
    return winner(aggregate(a, ink, p1, p2, paths), ink)


def sgm_near_right(left, right, prior_right, num_shifts, square_width, census, p1, p2, paths, radius, mode="toroidal"):
    """-> (best_right, web_right), by the definition: the mirrored images around the mirrored prior, mirrored back"""
    best, web, _ = sgm_near(mirror(right), mirror(left), mirror(np.asarray(prior_right)), num_shifts, square_width,
                            census, p1, p2, paths, radius, mode)
    return mirror(best), mirror(web)


def expected(left, right, prior, prior_right, num_shifts, square_width, census, p1, p2, paths, radius, mode, max_diff):
    """every map of sm_sgm_wta_near / sm_sgm_wta_near_right / sm_sgm_near_lr for one gray pair"""
    best, web, sub = sgm_near(left, right, prior, num_shifts, square_width, census, p1, p2, paths, radius, mode)
    best_right, web_right = sgm_near_right(left, right, prior_right, num_shifts, square_width, census, p1, p2, paths,
                                           radius, mode)
    checked, rejected = lr_check(web, web_right, max_diff, mode)
    sub_checked = np.where(checked == 0, 0, sub).astype(np.int16)
    return dict(best=best, web=web, sub=sub, best_right=best_right, web_right=web_right, checked=checked,
                rejected=rejected, sub_checked=sub_checked)


# ---------------------------------------------------------------------------
# path by path, pixel by pixel
# ---------------------------------------------------------------------------

def sgm_near_loop(left, right, prior, num_shifts, square_width, census, p1, p2, paths, radius, mode="toroidal"):
    """-> (best, web, sub): every path followed from its first pixel, a pixel and a shift of its band at a time"""
    h, w = np.asarray(prior).shape
    D = num_shifts
    a = data_term(left, right, band(prior, D, radius), square_width, census, mode)

    def K(x, y):
        s = int(prior[y, x])
        return [] if s == 0 else [d for d in range(max(0, s - 1 - radius), min(D - 1, s - 1 + radius) + 1)]
    total = {}
    for dx, dy in DIRS[paths]:
        for y0 in range(h):
            for x0 in range(w):
                if 0 <= x0 - dx < w and 0 <= y0 - dy < h:
                    continue                                # not the first pixel of a line
                x, y, prev = x0, y0, None
                while 0 <= x < w and 0 <= y < h:
                    cur = {}
                    for d in K(x, y):
                        cur[d] = int(a[y, x, d])
                        if prev:
                            m = min(prev.values())
                            c = [m + p2]
                            if d in prev:
                                c.append(prev[d])
                            c += [prev[k] + p1 for k in (d - 1, d + 1) if k in prev]
                            cur[d] += min(c) - m
                        total[y, x, d] = total.get((y, x, d), 0) + cur[d]
                    prev = cur                              # empty: the path restarts at the next pixel
                    x, y = x + dx, y + dy
    best = np.zeros((h, w), np.int32)
    web = np.zeros((h, w), np.int32)
    sub = np.zeros((h, w), np.int16)
    for y in range(h):
        for x in range(w):
            ks = K(x, y)
            if not ks:
                continue
            v = {d: total[y, x, d] for d in ks}
            b = min(v.values())
            d = min(k for k in ks if v[k] == b)
            q = 0
            if d - 1 in v and d + 1 in v:
                aa, bb = v[d - 1] - b, v[d + 1] - b
                if aa + bb > 0:
                    q = max(-8, min(8, (16 * (aa - bb) + aa + bb) // (2 * (aa + bb))))
            best[y, x], web[y, x], sub[y, x] = b, d + 1, 16 * (d + 1) + q
    return best, web, sub
