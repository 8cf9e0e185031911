"""The definition of occlusion-aware interpolation (include/stereo_hip.h), in numpy.  Parity is
unpinned: the reference has no such stage, so this file is what sm_occlusion_classify and sm_interpolate are tested
against.  (Hirschmueller, "Stereo Processing by Semiglobal Matching and Mutual Information", PAMI 2008: the
discontinuity-preserving interpolation of its post-processing section.)

Maps are [H][W] int32 (web) or int16 (sub); a pixel is valid iff its value != 0; negative values are valid and order
as signed integers.  web = 1 + shift: left pixel (x, y) with web = s matched right pixel u = x + s - 1, and
web_right(u, y) = s' means right pixel u matched left pixel u - (s' - 1).  A smaller value is farther away.

    classify(web, web_right, D, border)   u8 [H][W]: 0 valid, 1 occluded, 2 mismatched; vectorised over d
    classify_naive(...)                   per pixel, a loop over d
    interpolate(a, cls=None)              vectorised: eight "last valid value" propagations, a sort along a new axis
    interpolate_naive(a, cls=None)        per pixel: eight walks to the first valid pixel or the image edge
    filled(a, out)                        the number of pixels that were 0 and are not any more

classify: an invalid pixel (x, y) is mismatched iff some d in 0 .. D-1 has u = x + d inside the row (toroidal: u mod W;
ghost: u < W) and web_right(u, y) = d + 1, else occluded.
interpolate: a valid pixel is kept.  An invalid one looks along the eight directions for the first valid pixel of the
INPUT (no wrapping); with the m values found sorted c_0 <= ... <= c_{m-1}: 0 if m = 0; c_{min(1, m-1)} if the pixel is
occluded (cls = 1); else the lower median c_{(m-1)/2}.  cls is read where a = 0 only."""
import numpy as np

VALID, OCCLUDED, MISMATCHED = 0, 1, 2
DIRECTIONS = [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy]     # steps of the walk from the pixel


def _toroidal(border):
    assert border in ("toroidal", "ghost"), border
    return border == "toroidal"


def classify(web, web_right, d, border):
    web, r = np.asarray(web), np.asarray(web_right).astype(np.int64)
    assert web.ndim == 2 and web.shape == r.shape and d >= 1
    h, w = web.shape
    wrap = _toroidal(border)
    xs = np.arange(w)
    hit = np.zeros((h, w), bool)
    for k in range(d):
        if wrap:
            hit |= r[:, (xs + k) % w] == k + 1
        elif k < w:
            hit[:, :w - k] |= r[:, k:] == k + 1
    return np.where(web != 0, VALID, np.where(hit, MISMATCHED, OCCLUDED)).astype(np.uint8)


def classify_naive(web, web_right, d, border):
    web, r = np.asarray(web), np.asarray(web_right)
    h, w = web.shape
    wrap = _toroidal(border)
    out = np.zeros((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            if web[y, x] != 0:
                continue
            out[y, x] = OCCLUDED
            for k in range(d):
                u = x + k
                if u >= w:
                    if not wrap:
                        break
                    u %= w
                if int(r[y, u]) == k + 1:
                    out[y, x] = MISMATCHED
                    break
    return out


def _last_valid_along_rows(a):
    """[H][W]: for every pixel the value of the nearest valid pixel at or before it in its row, 0 if none"""
    h, w = a.shape
    idx = np.where(a != 0, np.arange(w)[None, :], -1)
    idx = np.maximum.accumulate(idx, axis=1)
    return np.where(idx >= 0, np.take_along_axis(a, np.maximum(idx, 0), axis=1), 0)


def _skew(a, sign):
    """rows shifted so that a diagonal becomes a column: row y moves right by y (sign +1) or by H-1-y (sign -1)"""
    h, w = a.shape
    out = np.zeros((h, w + h - 1), a.dtype)
    for y in range(h):
        o = y if sign > 0 else h - 1 - y
        out[y, o:o + w] = a[y]
    return out


def _unskew(s, sign, w):
    h = s.shape[0]
    return np.stack([s[y, (y if sign > 0 else h - 1 - y):(y if sign > 0 else h - 1 - y) + w] for y in range(h)])


def directional(a, dx, dy):
    """[H][W] int64: the first valid value met walking from each pixel in steps of (dx, dy), the pixel itself not
    counted; 0 if the walk reaches the image edge first"""
    a = np.asarray(a).astype(np.int64)
    h, w = a.shape
    if dy == 0:
        if dx < 0:                                          # the nearest valid pixel strictly to the left
            shifted = np.zeros_like(a)
            shifted[:, 1:] = _last_valid_along_rows(a)[:, :-1]
            return shifted
        return directional(a[:, ::-1], -1, 0)[:, ::-1]
    if dy > 0:                                              # look downwards: flip and look upwards
        return directional(a[::-1], dx, -1)[::-1]
    # dy < 0: the source lies above; along a column (dx = 0) or a diagonal made a column by skewing the rows.
    # dx < 0: the source is up-left, (x - k, y - k): constant x - y, a column once row y is moved LEFT by y, i.e.
    # right by H-1-y; dx > 0: constant x + y, a column once row y is moved right by y.
    if dx == 0:
        t = a.T
        shifted = np.zeros_like(t)
        shifted[:, 1:] = _last_valid_along_rows(t)[:, :-1]
        return shifted.T
    sign = -1 if dx < 0 else 1
    s = _skew(a, sign).T
    shifted = np.zeros_like(s)
    shifted[:, 1:] = _last_valid_along_rows(s)[:, :-1]
    return _unskew(shifted.T, sign, w)


def interpolate(a, cls=None):
    a = np.asarray(a)
    assert a.ndim == 2
    big = np.iinfo(np.int64).max
    cand = np.stack([directional(a, dx, dy) for dx, dy in DIRECTIONS])
    valid = cand != 0
    m = valid.sum(axis=0)
    ordered = np.sort(np.where(valid, cand, big), axis=0)          # the candidates first, ascending
    rank = (np.maximum(m, 1) - 1) // 2
    if cls is not None:
        cls = np.asarray(cls)
        assert cls.shape == a.shape
        rank = np.where(cls == OCCLUDED, np.minimum(1, np.maximum(m, 1) - 1), rank)
    pick = np.take_along_axis(ordered, rank[None], axis=0)[0]
    return np.where(a != 0, a, np.where(m > 0, pick, 0)).astype(a.dtype)


def candidates_naive(a, x, y):
    h, w = a.shape
    found = []
    for dx, dy in DIRECTIONS:
        xx, yy = x + dx, y + dy
        while 0 <= xx < w and 0 <= yy < h:
            if a[yy, xx] != 0:
                found.append(int(a[yy, xx]))
                break
            xx, yy = xx + dx, yy + dy
    return sorted(found)


def interpolate_naive(a, cls=None):
    a = np.asarray(a)
    h, w = a.shape
    out = a.copy()
    for y in range(h):
        for x in range(w):
            if a[y, x] != 0:
                continue
            c = candidates_naive(a, x, y)
            m = len(c)
            if m == 0:
                continue
            if cls is not None and cls[y, x] == OCCLUDED:
                out[y, x] = c[min(1, m - 1)]
            else:
                out[y, x] = c[(m - 1) // 2]
    return out


def candidate_count(a):
    """[H][W]: m, the number of directions in which a valid pixel is found (for the assertions tests make)"""
    return np.stack([directional(a, dx, dy) != 0 for dx, dy in DIRECTIONS]).sum(axis=0)


def filled(a, out):
    return int(((np.asarray(a) == 0) & (np.asarray(out) != 0)).sum())
