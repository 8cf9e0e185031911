"""Match uniqueness written out in numpy (include/stereo_hip.h sm_census_second / sm_sgm_wta2 / sm_uniqueness_filter /
sm_confidence).  Checker only: imported by tests/, never by the product package.

    runner-up of a volume V (h, w, D) against a map web (1 + shift; any int32): s = web(p);
        E(p) = { d in 0 .. D - 1 : |d - (s - 1)| >= 2 }  for s in 1 .. D,  all of 0 .. D - 1 for every other s;
        best2 = min over E(p) of V(p, d), web2 = 1 + the first d of E(p) reaching it;  E(p) empty: web2 = 0, best2 = -1
    census_second: V = the census window costs (tests/sgm_reference.data_term), the map is given
    sgm_wta2:      V = S (tests/sgm_reference.aggregate), the map is S's own winner
    filter:        out = web iff web != 0 and (best2 < 0 or best2 (100 - ratio) >= 100 best), else 0
    confidence:    0 where web = 0; else 255 where best2 < 0; else 0 where best2 <= best; else
                   min(255, floor(255 (best2 - best) / best2))  (best2 = 0 there means best < 0: the quotient is
                   unbounded, 255)

The *_bruteforce functions restate each of them pixel by pixel in Python integers, so that the CPU suite can pin the
vectorised forms."""
from __future__ import annotations

import numpy as np

from tests import census_reference as cr
from tests import sgm_reference as sg

__all__ = ["runner_up", "census_volume", "census_second", "sgm_wta2", "uniqueness_filter", "confidence",
           "runner_up_bruteforce", "uniqueness_filter_bruteforce", "confidence_bruteforce"]

NONE = np.iinfo(np.int64).max


def runner_up(vol, web):
    """-> (best2 int32, web2 int32) of a volume (h, w, D) against a map (h, w)"""
    vol = np.asarray(vol, np.int64)
    D = vol.shape[-1]
    s = np.asarray(web).astype(np.int64)
    has = (s >= 1) & (s <= D)
    d = np.arange(D, dtype=np.int64)
    near = has[..., None] & (np.abs(d - (s[..., None] - 1)) <= 1)
    v = np.where(near, NONE, vol)
    k = np.argmin(v, axis=-1)                               # the first d reaching the minimum
    b = np.take_along_axis(v, k[..., None], -1)[..., 0]
    none = b == NONE
    return np.where(none, -1, b).astype(np.int32), np.where(none, 0, k + 1).astype(np.int32)


def census_volume(left, right, num_shifts, square_width, census, mode="toroidal"):
    """-> int32 (h, w, D): sm_census_wta's window costs A_d"""
    return sg.data_term(left, right, num_shifts, square_width, census, mode)


def census_second(left, right, web, num_shifts, square_width, census, mode="toroidal", volume=None):
    """-> (best2, web2) of one gray pair against the map `web`"""
    if volume is None:
        volume = census_volume(left, right, num_shifts, square_width, census, mode)
    return runner_up(volume, web)


def sgm_wta2(left, right, num_shifts, square_width, census, p1, p2, paths, mode="toroidal"):
    """-> dict(best, web, sub, best2, web2) of one gray pair"""
    s = sg.aggregate(sg.data_term(left, right, num_shifts, square_width, census, mode), p1, p2, paths)
    best, web, sub = sg.winner(s)
    best2, web2 = runner_up(s, web)
    return dict(best=best, web=web, sub=sub, best2=best2, web2=web2)


def uniqueness_filter(web, best, best2, ratio):
    """-> (out int32, rejected: the pixels that were not 0 and now are)"""
    web = np.asarray(web, np.int32)
    b, b2 = np.asarray(best).astype(np.int64), np.asarray(best2).astype(np.int64)
    keep = (web != 0) & ((b2 < 0) | (b2 * (100 - ratio) >= b * 100))
    return np.where(keep, web, 0).astype(np.int32), int(((web != 0) & ~keep).sum())


def confidence(web, best, best2):
    """-> uint8"""
    web = np.asarray(web)
    b, b2 = np.asarray(best).astype(np.int64), np.asarray(best2).astype(np.int64)
    q = np.where(b2 > 0, (255 * (b2 - b)) // np.maximum(b2, 1), 255)     # b2 = 0 behind the third case: best < 0
    c = np.minimum(255, q)
    c = np.where(b2 <= b, 0, c)
    c = np.where(b2 < 0, 255, c)
    c = np.where(web == 0, 0, c)
    return c.astype(np.uint8)


# ---------------------------------------------------------------------------
# pixel by pixel
# ---------------------------------------------------------------------------

def runner_up_bruteforce(vol, web):
    h, w, D = vol.shape
    best2 = np.zeros((h, w), np.int32)
    web2 = np.zeros((h, w), np.int32)
    for y in range(h):
        for x in range(w):
            s = int(web[y, x])
            b, k = None, 0
            for d in range(D):
                if 1 <= s <= D and abs(d - (s - 1)) < 2:
                    continue
                v = int(vol[y, x, d])
                if b is None or v < b:
                    b, k = v, d + 1
            best2[y, x], web2[y, x] = (-1, 0) if b is None else (b, k)
    return best2, web2


def uniqueness_filter_bruteforce(web, best, best2, ratio):
    out = np.zeros(np.shape(web), np.int32)
    rejected = 0
    for i in np.ndindex(*np.shape(web)):
        s, b, b2 = int(web[i]), int(best[i]), int(best2[i])
        if s != 0 and (b2 < 0 or b2 * (100 - ratio) >= b * 100):
            out[i] = s
        elif s != 0:
            rejected += 1
    return out, rejected


def confidence_bruteforce(web, best, best2):
    out = np.zeros(np.shape(web), np.uint8)
    for i in np.ndindex(*np.shape(web)):
        s, b, b2 = int(web[i]), int(best[i]), int(best2[i])
        if s == 0:
            c = 0
        elif b2 < 0:
            c = 255
        elif b2 <= b:
            c = 0
        elif b2 == 0:
            c = 255
        else:
            c = min(255, (255 * (b2 - b)) // b2)
        out[i] = c
    return out
