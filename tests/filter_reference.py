"""The definition of the disparity post-filters (include/stereo_hip.h), in numpy.  Parity is unpinned:
the reference has no such stage, so this file is what sm_median_filter and sm_speckle_filter are tested against.

Maps are [H][W] int32 (web) or int16 (sub); a pixel is valid iff its value != 0; a tap outside the image does not
exist; negative values are valid and order as signed integers.

    median(a, k)                       vectorised: the k*k shifted copies sorted along a new axis
    median_naive(a, k)                 per pixel: the valid window values sorted, the lower median taken
    speckle(a, max_size, max_diff)     vectorised: min-label hooking with pointer jumping over the edge list
    speckle_naive(a, max_size, max_diff)   breadth-first flood fill, pixel by pixel
both speckle forms return (filtered map, number of valid pixels set to 0)."""
from collections import deque

import numpy as np


def median(a, k):
    a = np.asarray(a)
    assert a.ndim == 2 and k in (3, 5)
    h, w = a.shape
    r = k // 2
    big = np.iinfo(np.int64).max
    padded = np.zeros((h + 2 * r, w + 2 * r), np.int64)
    padded[r:r + h, r:r + w] = a
    taps = np.stack([padded[dy:dy + h, dx:dx + w] for dy in range(k) for dx in range(k)])
    valid = taps != 0
    m = valid.sum(axis=0)
    ordered = np.sort(np.where(valid, taps, big), axis=0)          # the valid values first, ascending
    pick = np.take_along_axis(ordered, (np.maximum(m, 1) - 1)[None] // 2, axis=0)[0]
    return np.where(a != 0, pick, 0).astype(a.dtype)


def median_naive(a, k):
    a = np.asarray(a)
    h, w = a.shape
    r = k // 2
    out = np.zeros_like(a)
    for y in range(h):
        for x in range(w):
            if a[y, x] == 0:
                continue
            v = sorted(int(a[yy, xx]) for yy in range(max(0, y - r), min(h, y + r + 1))
                       for xx in range(max(0, x - r), min(w, x + r + 1)) if a[yy, xx] != 0)
            out[y, x] = v[(len(v) - 1) // 2]
    return out


def component_roots(a, max_diff):
    """[H][W] int64: the least flat index of every valid pixel's component, -1 for invalid pixels"""
    a = np.asarray(a).astype(np.int64)
    h, w = a.shape
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    ok = a != 0
    joined_h = ok[:, 1:] & ok[:, :-1] & (np.abs(a[:, 1:] - a[:, :-1]) <= max_diff)
    joined_v = ok[1:] & ok[:-1] & (np.abs(a[1:] - a[:-1]) <= max_diff)
    ea = np.concatenate([idx[:, 1:][joined_h], idx[1:][joined_v]])
    eb = np.concatenate([idx[:, :-1][joined_h], idx[:-1][joined_v]])
    parent = np.arange(h * w, dtype=np.int64)
    while True:
        pa, pb = parent[ea], parent[eb]
        differ = pa != pb
        if not differ.any():
            break
        ea, eb, pa, pb = ea[differ], eb[differ], pa[differ], pb[differ]
        # every parent is a root here: hook the larger root of each edge below the smaller one ...
        np.minimum.at(parent, np.maximum(pa, pb), np.minimum(pa, pb))
        # ... and jump pointers until every parent is a root again
        while True:
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt
    roots = parent.reshape(h, w)
    return np.where(ok, roots, -1)


def speckle(a, max_size, max_diff):
    a = np.asarray(a)
    assert a.ndim == 2 and max_size >= 0 and max_diff >= 0
    roots = component_roots(a, max_diff)
    ok = roots >= 0
    sizes = np.bincount(roots[ok], minlength=a.size)
    keep = ok & (sizes[np.where(ok, roots, 0)] > max_size)
    return np.where(keep, a, 0).astype(a.dtype), int((ok & ~keep).sum())


def speckle_naive(a, max_size, max_diff):
    a = np.asarray(a)
    h, w = a.shape
    out = a.copy()
    seen = np.zeros((h, w), bool)
    removed = 0
    for y0 in range(h):
        for x0 in range(w):
            if seen[y0, x0] or a[y0, x0] == 0:
                continue
            seen[y0, x0] = True
            comp, todo = [], deque([(y0, x0)])
            while todo:
                y, x = todo.popleft()
                comp.append((y, x))
                for yy, xx in ((y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x)):
                    if 0 <= yy < h and 0 <= xx < w and not seen[yy, xx] and a[yy, xx] != 0 and \
                            abs(int(a[yy, xx]) - int(a[y, x])) <= max_diff:
                        seen[yy, xx] = True
                        todo.append((yy, xx))
            if len(comp) <= max_size:
                removed += len(comp)
                for y, x in comp:
                    out[y, x] = 0
    return out, removed


def components(a, max_diff):
    """(roots [H][W], {root: size}) for the assertions tests make about their own inputs"""
    roots = component_roots(a, max_diff)
    ids, counts = np.unique(roots[roots >= 0], return_counts=True)
    return roots, dict(zip(ids.tolist(), counts.tolist()))
