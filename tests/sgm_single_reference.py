"""SGM's left-right check from ONE aggregated volume written out in numpy (include/stereo_hip.h sm_sgm_wta_both /
sm_sgm_lr_single), on tests/sgm_reference.py.  Checker only: imported by tests/, never by the
product package.

    S(y, x, d)       = sgm_reference.aggregate of the LEFT pass, d = 0 .. D - 1
    best, web, sub   = sgm_reference.winner(S): what sm_sgm_wta writes
    right pixel (u, y) takes candidate d from left pixel x = u - d:
        toroidal: every d, x = (u - d) mod W (D > W: the same x serves several d)
        ghost:    only d <= u (S has no column left of 0); d = 0 is always a candidate
    best_right(u, y) = min over the candidates of S(y, x, d); web_right = 1 + the least d reaching it
    check            = tests/lr_reference.lr_check between web and this web_right; sub = 0 where it rejected

right_from_volume is the vectorised form (one gather per shift); right_from_volume_bruteforce loops over (u, d), so that
the CPU suite can pin the vectorised form on tiny volumes."""
from __future__ import annotations

import numpy as np

from tests import sgm_reference as sr
from tests.lr_reference import lr_check

__all__ = ["right_from_volume", "right_from_volume_bruteforce", "both", "expected"]

NONE = np.int64(1) << 40


def right_from_volume(s, mode="toroidal"):
    """-> (best_right int32, web_right int32) of an aggregate volume S (h, w, D)"""
    h, w, D = s.shape
    u = np.arange(w)
    cand = np.full((h, w, D), NONE, np.int64)
    for d in range(D):
        if mode == "toroidal":
            cand[:, :, d] = s[:, (u - d) % w, d]
        elif d < w:
            cand[:, d:, d] = s[:, :w - d, d]
    d = np.argmin(cand, axis=-1)                              # the first minimum: the least d
    best = np.take_along_axis(cand, d[..., None], -1)[..., 0]
    return best.astype(np.int32), (d + 1).astype(np.int32)


def right_from_volume_bruteforce(s, mode="toroidal"):
    h, w, D = s.shape
    best = np.zeros((h, w), np.int32)
    web = np.zeros((h, w), np.int32)
    for y in range(h):
        for u in range(w):
            b, k = None, None
            for d in range(D):
                if mode != "toroidal" and d > u:
                    continue
                v = int(s[y, (u - d) % w, d])
                if b is None or v < b:
                    b, k = v, d
            best[y, u], web[y, u] = b, k + 1
    return best, web


def both(left, right, num_shifts, square_width, census, p1, p2, paths, mode="toroidal"):
    """-> (best, web, sub, best_right, web_right) of one gray pair: sm_sgm_wta_both's maps"""
    s = sr.aggregate(sr.data_term(left, right, num_shifts, square_width, census, mode), p1, p2, paths)
    return (*sr.winner(s), *right_from_volume(s, mode))


def expected(left, right, num_shifts, square_width, census, p1, p2, paths, mode, max_diffs=(0,)):
    """every map of sm_sgm_wta_both, and for each max_diff those of sm_sgm_lr_single, for one gray pair"""
    best, web, sub, best_right, web_right = both(left, right, num_shifts, square_width, census, p1, p2, paths, mode)
    e = dict(best=best, web=web, sub=sub, best_right=best_right, web_right=web_right)
    for md in max_diffs:
        checked, rejected = lr_check(web, web_right, md, mode)
        e[md] = dict(checked=checked, rejected=rejected, sub_checked=np.where(checked == 0, 0, sub).astype(np.int16))
    return e
