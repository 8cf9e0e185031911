"""The definition of the guided weighted median (include/stereo_hip.h), in numpy.  Parity is unpinned:
the reference has no such stage, so this file is what sm_weighted_median is tested against.

Maps are [H][W] int32 (web) or int16 (sub); a pixel is valid iff its value != 0; a tap outside the image does not
exist; negative values are valid and order as signed integers.  The guide g is uint8 [H][W]; radius r is 1 .. 7;
weights holds 256 integers in 0 .. 65535 with weights[0] >= 1.

For pixel p the taps are the pixels q of the (2r+1) x (2r+1) window around p that lie in the image and have
in(q) != 0.  Tap q has the weight w_q = weights[|g(p) - g(q)|], and T is the sum of the w_q.  wmed(p) is the smallest
tap value v, in signed order, with 2 * sum{w_q : in(q) <= v} >= T: the lower weighted median.
    fill off:  out(p) = 0 where in(p) = 0; otherwise out(p) = wmed(p)
    fill on:   where in(p) = 0, out(p) = wmed(p) if T >= fill_min_weight, otherwise 0
filled = the number of pixels that were 0 and are no longer (0 with fill off).  Taps are read from the input.

    weighted_median(a, g, r, weights, fill, fill_min_weight)         vectorised: the window's taps stacked, sorted
                                                                     along the tap axis, the weights cumulated
    weighted_median_naive(a, g, r, weights, fill, fill_min_weight)   the same text, pixel by pixel
    totals(a, g, r, weights)                                         T of every pixel
each of the first two returns (filtered map, filled)."""
import numpy as np


def _check(a, g, radius, weights, fill, fill_min_weight):
    a, g, weights = np.asarray(a), np.asarray(g), np.asarray(weights)
    assert a.ndim == 2 and a.dtype in (np.int32, np.int16) and g.shape == a.shape and g.dtype == np.uint8
    assert 1 <= radius <= 7 and weights.shape == (256,) and weights.min() >= 0 and weights.max() <= 65535
    assert weights[0] >= 1 and (not fill or fill_min_weight >= 1)
    return a, g, weights.astype(np.int64)


def _stacked(a, g, radius, weights):
    """-> (values [taps][H][W] int64, weights [taps][H][W] int64: 0 for a tap that does not exist or is invalid)"""
    h, w = a.shape
    r, k = radius, 2 * radius + 1
    pa = np.zeros((h + 2 * r, w + 2 * r), np.int64)
    pa[r:r + h, r:r + w] = a
    pg = np.zeros((h + 2 * r, w + 2 * r), np.int64)
    pg[r:r + h, r:r + w] = g
    centre = g.astype(np.int64)
    vals = np.stack([pa[dy:dy + h, dx:dx + w] for dy in range(k) for dx in range(k)])
    gray = np.stack([pg[dy:dy + h, dx:dx + w] for dy in range(k) for dx in range(k)])
    wts = np.where(vals != 0, weights[np.abs(gray - centre[None])], 0)      # (a padded tap has the value 0)
    return vals, wts


def totals(a, g, radius, weights):
    a, g, weights = _check(a, g, radius, weights, False, 1)
    return _stacked(a, g, radius, weights)[1].sum(axis=0)


def weighted_median(a, g, radius, weights, fill=False, fill_min_weight=1):
    a, g, weights = _check(a, g, radius, weights, fill, fill_min_weight)
    vals, wts = _stacked(a, g, radius, weights)
    total = wts.sum(axis=0)
    order = np.argsort(vals, axis=0, kind="stable")
    vals, wts = np.take_along_axis(vals, order, axis=0), np.take_along_axis(wts, order, axis=0)
    # equal values are one step of the cumulated weight: a tap counts with every tap of its value, so the first tap
    # (in sorted order) that has a weight and reaches half of T is of the value looked for
    cum = np.cumsum(wts, axis=0)
    reached = (2 * cum >= total[None]) & (wts > 0)
    first = np.argmax(reached, axis=0)
    wmed = np.take_along_axis(vals, first[None], axis=0)[0]
    wmed = np.where(total > 0, wmed, 0)
    if fill:
        out = np.where(a != 0, wmed, np.where(total >= fill_min_weight, wmed, 0))
    else:
        out = np.where(a != 0, wmed, 0)
    return out.astype(a.dtype), int(((a == 0) & (out != 0)).sum())


def weighted_median_naive(a, g, radius, weights, fill=False, fill_min_weight=1):
    a, g, weights = _check(a, g, radius, weights, fill, fill_min_weight)
    h, w = a.shape
    out = np.zeros_like(a)
    filled = 0
    for y in range(h):
        for x in range(w):
            if a[y, x] == 0 and not fill:
                continue
            taps = [(int(a[yy, xx]), int(weights[abs(int(g[y, x]) - int(g[yy, xx]))]))
                    for yy in range(max(0, y - radius), min(h, y + radius + 1))
                    for xx in range(max(0, x - radius), min(w, x + radius + 1)) if a[yy, xx] != 0]
            total = sum(wq for _, wq in taps)
            if a[y, x] == 0 and total < fill_min_weight:
                continue
            for v in sorted({v for v, _ in taps}):
                if 2 * sum(wq for u, wq in taps if u <= v) >= total:
                    out[y, x] = v
                    break
            filled += int(a[y, x] == 0 and out[y, x] != 0)
    return out, filled
