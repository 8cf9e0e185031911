"""The subpixel refinement of the cost mode written out in numpy (include/stereo_hip.h sm_cost_refine, DESIGN.md
section 11).  Checker only: imported by tests/, never by the product package.  The window costs are summed here
with their own box sums (cumulative sums over a border-padded cost plane), independently of the oracle:

    C(d)(x, y) = sum over the n x n window of |L - R(. + d)| (SAD) or its square (SSD)
                 toroidal: everything wraps;  ghost: R = 0 past the right border, taps outside the image cost 0
    s = web(x, y);  sub = 0 if s is outside 1..D;  16 s if s == 1 or s == D;  else 16 s + q with
    a = C(s-2) - C(s-1), b = C(s) - C(s-1),
    SSD: q = floor((16 (a - b) + den) / (2 den)), den = a + b;  SAD: the same with den = max(a, b);
    q = 0 where den <= 0, else clamped to [-8, 8]."""
from __future__ import annotations

import numpy as np


def fit_q(a, b, cost):
    """q of the definition for rises a (left) and b (right) around the winner; works on arrays"""
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    den = a + b if cost == "ssd" else np.maximum(a, b)
    safe = np.where(den > 0, den, 1)
    q = (16 * (a - b) + safe) // (2 * safe)              # numpy // is floor division
    return np.where(den > 0, np.clip(q, -8, 8), 0)


def subpixel(c0, c1, c2, s, num_shifts, cost):
    """sub of the definition from the three costs C(s-2), C(s-1), C(s) (ignored where they do not exist)"""
    s = np.asarray(s, np.int64)
    q = fit_q(np.asarray(c0, np.int64) - c1, np.asarray(c2, np.int64) - c1, cost)
    inner = (s >= 2) & (s <= num_shifts - 1)
    valid = (s >= 1) & (s <= num_shifts)
    return np.where(valid, 16 * s + np.where(inner, q, 0), 0).astype(np.int16)


def _band_costs(left, right, d, n, mode, cost, y0, y1):
    """C(d) on rows y0 .. y1 - 1 of one pair"""
    h, w = left.shape
    half = n // 2
    ys = np.arange(y0 - half, y1 + half)
    if mode == "toroidal":
        rows, valid = ys % h, np.ones(len(ys), bool)
    else:
        valid = (ys >= 0) & (ys < h)
        rows = np.clip(ys, 0, h - 1)
    L = left[rows].astype(np.int64)
    Rr = right[rows].astype(np.int64)
    if mode == "toroidal":
        R = np.roll(Rr, -d, axis=1)
    else:
        R = np.zeros_like(Rr)
        if 0 <= d < w:
            R[:, :w - d] = Rr[:, d:]
    diff = L - R
    c = diff * diff if cost == "ssd" else np.abs(diff)
    c[~valid] = 0
    p = np.pad(c, ((0, 0), (half, half)), mode="wrap" if mode == "toroidal" else "constant")
    cs = np.zeros((p.shape[0] + 1, p.shape[1] + 1), np.int64)
    cs[1:, 1:] = p.cumsum(0).cumsum(1)
    return cs[n:, n:] - cs[:-n, n:] - cs[n:, :-n] + cs[:-n, :-n]


def refine(left, right, web, num_shifts, square_width, mode="toroidal", cost="sad", rows=None):
    """-> (sub int16 (h, w), costs int32 (3, h, w)) of one pair; rows=(y0, y1): only those rows of web's image
    (the result then has y1 - y0 rows)"""
    left = np.asarray(left, np.uint8)
    right = np.asarray(right, np.uint8)
    h, w = left.shape
    n = 2 * (square_width // 2) + 1
    y0, y1 = rows if rows is not None else (0, h)
    s = np.asarray(web, np.int64)[y0:y1]
    valid = (s >= 1) & (s <= num_shifts)
    costs = np.full((3,) + s.shape, -1, np.int64)
    for k in range(3):
        d = s - 2 + k                                      # shift indices s-2, s-1, s
        ok = valid & (d >= 0) & (d < num_shifts)
        for dv in np.unique(d[ok]):
            m = ok & (d == dv)
            costs[k][m] = _band_costs(left, right, int(dv), n, mode, cost, y0, y1)[m]
    sub = subpixel(costs[0], costs[1], costs[2], s, num_shifts, cost)
    return sub, costs.astype(np.int32)


def texture(w, h, seed, t, cosines=12):
    """A seeded smooth texture periodic in w, and its copy displaced by t pixels (R(u) = L(u - t), computed
    analytically), both rounded to uint8: the true disparity of every pixel is t"""
    rng = np.random.default_rng(seed)
    fx = rng.integers(1, max(2, w // 24), cosines)         # whole periods across the width
    fy = rng.uniform(0.5, 3.0, cosines) / h
    amp = rng.uniform(0.5, 1.0, cosines)
    ph = rng.uniform(0, 2 * np.pi, cosines)
    x = np.arange(w)[None, :, None]
    y = np.arange(h)[:, None, None]

    def img(shift):
        v = (amp * np.cos(2 * np.pi * (fx * (x - shift) / w + fy * y) + ph)).sum(-1)
        return v

    scale = 110.0 / amp.sum()
    left = np.clip(np.rint(128 + scale * img(0.0)), 0, 255).astype(np.uint8)
    right = np.clip(np.rint(128 + scale * img(t)), 0, 255).astype(np.uint8)
    return left, right
