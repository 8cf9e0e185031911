"""The guided census re-search written out in numpy (include/stereo_hip.h sm_census_wta_near / _near_right / _near_lr,
DESIGN.md section 21).  Checker only: imported by tests/, never by the product package.

    A_d(p)  = tests/census_reference.window_costs: sm_census_wta's window cost of shift d
    prior   = an int32 web map: 1 + shift, 0 invalid; radius r in 1 .. 4
    K(p)    = { d : 0 <= d <= D - 1, |d - (prior(p) - 1)| <= r }, empty for prior(p) = 0
    K empty: web = best = 0; otherwise best = min over K of A_d(p), web = 1 + the least d of K reaching it
    right reference = mirror(near(mirror(R), mirror(L), mirror(prior_right)))          mirror(a)(x) = a(W-1-x)

near_bruteforce restates the left search pixel by pixel and near_right_direct the right one without mirrors, so that
the CPU suite can pin the vectorised forms (tests/test_near_cpu.py)."""
from __future__ import annotations

import numpy as np

from tests.census_reference import mirror, transform, window_costs
from tests.cost_lr_reference import _box
from tests.lr_reference import lr_check

__all__ = ["candidates", "near", "near_right", "near_right_direct", "near_bruteforce", "expected"]


def candidates(prior, num_shifts, radius):
    """-> (lo, hi, has): K(p) = lo .. hi where has, in int64 (INT32_MIN and INT32_MAX are legal priors)"""
    s = np.asarray(prior).astype(np.int64)
    lo = np.maximum(0, s - 1 - radius)
    hi = np.minimum(num_shifts - 1, s - 1 + radius)
    return lo, hi, (s != 0) & (lo <= hi)


def near(left, right, prior, num_shifts, square_width, census, radius, mode="toroidal"):
    """-> (best int32, web int32) of one pair"""
    cl, cr = transform(left, census, mode), transform(right, census, mode)
    lo, hi, has = candidates(prior, num_shifts, radius)
    best = np.full(cl.shape, np.iinfo(np.int64).max, np.int64)
    web = np.zeros(cl.shape, np.int32)
    for d in range(num_shifts):
        m = has & (lo <= d) & (d <= hi)
        if not m.any():
            continue
        total = window_costs(left, right, d, square_width, census, mode, cl, cr)
        upd = m & (total < best)
        best[upd] = total[upd]
        web[upd] = d + 1
    best[~has] = 0
    return best.astype(np.int32), web


def near_right(left, right, prior_right, num_shifts, square_width, census, radius, mode="toroidal"):
    """-> (best_right, web_right), by the definition: the search of the mirrored images around the mirrored prior,
    mirrored back"""
    best, web = near(mirror(right), mirror(left), mirror(np.asarray(prior_right)), num_shifts, square_width, census,
                     radius, mode)
    return mirror(best), mirror(web)


def near_right_direct(left, right, prior_right, num_shifts, square_width, census, radius, mode="toroidal"):
    """the right search without mirrors: the cost of right pixel u at d is popcount(C_R(u) ^ C_L(u - d)), toroidal
    u - d mod W, ghost C_L = 0 for u - d < 0"""
    cl, cr = transform(left, census, mode), transform(right, census, mode)
    n = 2 * (square_width // 2) + 1
    w = cl.shape[1]
    lo, hi, has = candidates(prior_right, num_shifts, radius)
    best = np.full(cl.shape, np.iinfo(np.int64).max, np.int64)
    web = np.zeros(cl.shape, np.int32)
    for d in range(num_shifts):
        m = has & (lo <= d) & (d <= hi)
        if not m.any():
            continue
        if mode == "toroidal":
            other = np.roll(cl, d, axis=1)                  # other(u) = C_L((u - d) mod W)
        else:
            other = np.zeros_like(cl)
            if d < w:
                other[:, d:] = cl[:, :w - d]
        total = _box(np.bitwise_count(cr ^ other).astype(np.int64), n, mode)
        upd = m & (total < best)
        best[upd] = total[upd]
        web[upd] = d + 1
    best[~has] = 0
    return best.astype(np.int32), web


def near_bruteforce(left, right, prior, num_shifts, square_width, census, radius, mode="toroidal"):
    """the left search pixel by pixel, tap by tap"""
    cl, cr = transform(left, census, mode), transform(right, census, mode)
    h, w = cl.shape
    half = square_width // 2

    def cost(x, y, d):
        if mode == "toroidal":
            return bin(int(cl[y % h, x % w]) ^ int(cr[y % h, (x + d) % w])).count("1")
        if not (0 <= x < w and 0 <= y < h):
            return 0
        return bin(int(cl[y, x]) ^ (int(cr[y, x + d]) if x + d < w else 0)).count("1")

    best = np.zeros((h, w), np.int32)
    web = np.zeros((h, w), np.int32)
    for y in range(h):
        for x in range(w):
            s = int(prior[y, x])
            if s == 0:
                continue
            b = None
            for d in range(num_shifts):
                if abs(d - (s - 1)) > radius:
                    continue
                a = sum(cost(x + tx, y + ty, d) for ty in range(-half, half + 1) for tx in range(-half, half + 1))
                if b is None or a < b:
                    b, best[y, x], web[y, x] = a, a, d + 1
    return best, web


def expected(left, right, prior, prior_right, num_shifts, square_width, census, radius, mode, max_diff):
    """the left maps, the right-reference maps and the checked map of one pair (sm_census_near_lr)"""
    best, web = near(left, right, prior, num_shifts, square_width, census, radius, mode)
    best_right, web_right = near_right(left, right, prior_right, num_shifts, square_width, census, radius, mode)
    checked, rejected = lr_check(web, web_right, max_diff, mode)
    return dict(best=best, web=web, best_right=best_right, web_right=web_right, checked=checked, rejected=rejected)
