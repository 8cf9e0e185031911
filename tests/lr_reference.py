"""Definitions of the left-right consistency check in numpy (include/stereo_hip.h).
Checker only: imported by tests/, never by the product package.

    web_right = mirror(hot_path(mirror(eR), mirror(eL)))        mirror(a)(x) = a(W-1-x)

right_reference() computes that with the oracle; right_reference_bruteforce() restates the right-reference
match directly (right pixel u against left pixel u - d) so that the CPU suite can pin the identity."""
from __future__ import annotations

import numpy as np

from tests import oracle


def mirror(a):
    return np.ascontiguousarray(a[..., ::-1])


def right_reference(el, er, num_shifts, square_width, mode="toroidal", banded=False):
    """-> (best_right, web_right) of one pair of u8 edge images, by the oracle on mirrored images"""
    hot = oracle.hot_path_banded if banded else oracle.hot_path
    best, web = hot(mirror(er), mirror(el), num_shifts, square_width, mode)
    return mirror(best), mirror(web)


def right_reference_bruteforce(el, er, num_shifts, square_width, mode="toroidal"):
    """The right-reference match written out: for shift d, right pixel u matches iff eR(u) == eL(u - d)
    (toroidal: u - d mod W; ghost: 0 before column 0); window sums with the border's taps; a score only
    where the pixel itself matched; the last shift reaching the maximum wins."""
    el = np.asarray(el, np.int32)
    er = np.asarray(er, np.int32)
    h, w = el.shape
    half = square_width // 2
    best = np.zeros((h, w), np.int64)
    web = np.zeros((h, w), np.int32)
    for d in range(num_shifts):
        if mode == "toroidal":
            shifted = np.roll(el, d, axis=1)
        else:
            shifted = np.zeros_like(el)
            if d < w:
                shifted[:, d:] = el[:, :w - d]
        m = (er == shifted).astype(np.int64)
        total = np.zeros((h, w), np.int64)
        if mode == "toroidal":
            for ty in range(-half, half + 1):
                for tx in range(-half, half + 1):
                    total += np.roll(m, (-ty, -tx), axis=(0, 1))
        else:
            p = np.pad(m, half)
            for ty in range(2 * half + 1):
                for tx in range(2 * half + 1):
                    total += p[ty:ty + h, tx:tx + w]
        score = np.where(m == 1, total, 0)
        upd = score >= best
        best[upd] = score[upd]
        web[upd] = d + 1
    return best.astype(np.int32), web


def lr_check(web, web_right, max_diff, mode="toroidal"):
    """-> (checked map, rejected count) of one pair: left pixel x with s = web(x) matched right pixel
    u = x + s - 1 (toroidal: mod W; ghost: outside 0..W-1 = rejected) and is kept iff
    |web_right(u) - s| <= max_diff; rejected pixels become 0."""
    web = np.asarray(web, np.int64)
    web_right = np.asarray(web_right, np.int64)
    h, w = web.shape
    u = np.arange(w)[None, :] + web - 1
    if mode == "toroidal":
        valid = np.ones_like(u, bool)
        u = u % w
    else:
        valid = (u >= 0) & (u < w)
        u = np.clip(u, 0, w - 1)
    r = np.take_along_axis(web_right, u, axis=1)
    keep = valid & (np.abs(r - web) <= max_diff)
    return np.where(keep, web, 0).astype(np.int32), int((~keep).sum())
