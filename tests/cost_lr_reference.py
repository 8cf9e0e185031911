"""Definitions of the SAD / SSD cost mode's left-right consistency check in numpy (include/stereo_hip.h
sm_cost_lr).  Checker only: imported by tests/, never by the product package.

    (best_right, web_right) = mirror(cost_hot_path(mirror(R), mirror(L)))        mirror(a)(x) = a(W-1-x)

right_reference() computes that with the oracle; right_reference_bruteforce() restates the right-reference
match directly (right pixel u against left pixel u - d) so that the CPU suite can pin the identity.  The check
itself is tests/lr_reference.lr_check, unchanged."""
from __future__ import annotations

import numpy as np

from tests import oracle
from tests.lr_reference import lr_check, mirror

__all__ = ["right_reference", "right_reference_bruteforce", "expected", "lr_check", "mirror"]


def right_reference(left, right, num_shifts, square_width, mode="toroidal", cost="sad", banded=False):
    """-> (best_right, web_right) of one gray pair, by the oracle's cost mode on mirrored images"""
    hot = oracle.cost_hot_path_banded if banded else oracle.cost_hot_path
    best, web = hot(mirror(right), mirror(left), num_shifts, square_width, mode, cost)
    return mirror(best), mirror(web)


def _box(c, n, mode):
    """n x n window sums of a cost plane: toroidal wraps, ghost counts taps outside the image as 0"""
    half = n // 2
    h, w = c.shape
    if mode == "toroidal":
        p = c[np.arange(-half, h + half) % h][:, np.arange(-half, w + half) % w]
    else:
        p = np.pad(c, half)
    cs = np.zeros((p.shape[0] + 1, p.shape[1] + 1), np.int64)
    cs[1:, 1:] = p.cumsum(0).cumsum(1)
    return cs[n:, n:] - cs[:-n, n:] - cs[n:, :-n] + cs[:-n, :-n]


def right_reference_bruteforce(left, right, num_shifts, square_width, mode="toroidal", cost="sad"):
    """The right-reference cost match written out: for shift d, right pixel u costs |R(u) - L(u - d)| (or its
    square; toroidal: u - d mod W; ghost: L is 0 left of column 0), summed over the n x n window with the
    border's taps; the FIRST shift reaching the minimum wins (web = d + 1)."""
    L = np.asarray(left, np.int64)
    R = np.asarray(right, np.int64)
    h, w = L.shape
    n = 2 * (square_width // 2) + 1
    best = np.full((h, w), np.iinfo(np.int64).max, np.int64)
    web = np.zeros((h, w), np.int32)
    for d in range(num_shifts):
        if mode == "toroidal":
            shifted = np.roll(L, d, axis=1)               # shifted(u) = L((u - d) mod W)
        else:
            shifted = np.zeros_like(L)
            if d < w:
                shifted[:, d:] = L[:, :w - d]
        diff = R - shifted
        total = _box(diff * diff if cost == "ssd" else np.abs(diff), n, mode)
        upd = total < best
        best[upd] = total[upd]
        web[upd] = d + 1
    return best.astype(np.int32), web


def expected(left, right, num_shifts, square_width, mode, cost, max_diff, banded=False):
    """the left map / costs, the right-reference map / costs and the checked map of one gray pair"""
    hot = oracle.cost_hot_path_banded if banded else oracle.cost_hot_path
    best, web = hot(left, right, num_shifts, square_width, mode, cost)
    best_right, web_right = right_reference(left, right, num_shifts, square_width, mode, cost, banded)
    checked, rejected = lr_check(web, web_right, max_diff, mode)
    return dict(best=best, web=web, best_right=best_right, web_right=web_right, checked=checked, rejected=rejected)
