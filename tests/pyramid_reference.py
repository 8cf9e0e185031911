"""The definition of the half-resolution path (include/stereo_hip.h), in numpy.  Parity is unpinned: the
reference has no such stage, so this file is what sm_reduce_half and sm_upsample_double are tested against.

The fine size is W x H, the coarse size cw = (W + 1) >> 1, ch = (H + 1) >> 1.  Nothing wraps.

reduce (uint8 [H][W] -> uint8 [ch][cw]), exact integers, cx(u) = min(max(u, 0), W - 1) and cy likewise:
    "box":      dst(X, Y) = (sum{i, j in 0..1} src(cx(2X + i), cy(2Y + j)) + 2) >> 2
    "binomial": k = [1, 3, 3, 1]; dst(X, Y) = (sum{i, j in 0..3} k_i k_j src(cx(2X - 1 + i), cy(2Y - 1 + j)) + 32) >> 6

upsample (int32 or int16 [ch][cw] -> the same type [H][W]; a pixel is valid iff != 0), guides g uint8 [H][W] and gc
uint8 [ch][cw], weights 256 integers in 1 .. 65535:
    v(c) = clamp(2 in(c) - 1) to int32, or clamp(2 in(c) - 16) to int16
    fine pixel p = (x, y): home (X, Y) = (x >> 1, y >> 1), px = x & 1, py = y & 1
    taps: the coarse pixels c = (X + i, Y + j), i, j in -1 .. 1, that lie in the coarse image and have in(c) != 0
    w_c = weights[|g(p) - gc(c)|] * s(i, px) * s(j, py), s(i, 0) = 2, 4, 1 and s(i, 1) = 1, 4, 2 for i = -1, 0, 1
    T = sum of the w_c; wmed(p) = the smallest v(c), signed order, with 2 * sum{w_c' : v(c') <= v(c)} >= T
    fill off: out(p) = 0 where in(home) = 0, else wmed(p);  fill on: where in(home) = 0, wmed(p) if p has a tap, else 0

    half_shape(w, h)                                  (cw, ch)
    reduce_half(src, filter)                          vectorised: clamped index arrays
    reduce_half_naive(src, filter)                    the same text, pixel by pixel
    upsample_double(a, g, gc, weights, fill)          vectorised: the nine taps stacked, sorted, the weights cumulated
    upsample_double_naive(a, g, gc, weights, fill)    the same text, pixel by pixel"""
import numpy as np

S = np.array([[2, 4, 1], [1, 4, 2]], np.int64)        # s(i, px): S[px][i + 1]
K = np.array([1, 3, 3, 1], np.int64)
LIMITS = {np.dtype(np.int32): (-2**31, 2**31 - 1, 1), np.dtype(np.int16): (-2**15, 2**15 - 1, 16)}


def half_shape(w, h):
    return (w + 1) >> 1, (h + 1) >> 1


def _check_reduce(src, filter):
    src = np.asarray(src)
    assert src.ndim == 2 and src.dtype == np.uint8 and filter in ("box", "binomial")
    return src.astype(np.int64)


def reduce_half(src, filter):
    s = _check_reduce(src, filter)
    h, w = s.shape
    cw, ch = half_shape(w, h)
    xs, ys = 2 * np.arange(cw), 2 * np.arange(ch)
    acc = np.zeros((ch, cw), np.int64)
    if filter == "box":
        for j in range(2):
            for i in range(2):
                acc += s[np.clip(ys + j, 0, h - 1)][:, np.clip(xs + i, 0, w - 1)]
        return ((acc + 2) >> 2).astype(np.uint8)
    for j in range(4):
        for i in range(4):
            acc += K[i] * K[j] * s[np.clip(ys - 1 + j, 0, h - 1)][:, np.clip(xs - 1 + i, 0, w - 1)]
    return ((acc + 32) >> 6).astype(np.uint8)


def reduce_half_naive(src, filter):
    s = _check_reduce(src, filter)
    h, w = s.shape
    cw, ch = half_shape(w, h)
    cx, cy = (lambda u: min(max(u, 0), w - 1)), (lambda v: min(max(v, 0), h - 1))
    dst = np.zeros((ch, cw), np.uint8)
    for Y in range(ch):
        for X in range(cw):
            if filter == "box":
                dst[Y, X] = (sum(int(s[cy(2 * Y + j), cx(2 * X + i)]) for j in range(2) for i in range(2)) + 2) >> 2
            else:
                dst[Y, X] = (sum(int(K[i] * K[j] * s[cy(2 * Y - 1 + j), cx(2 * X - 1 + i)])
                                 for j in range(4) for i in range(4)) + 32) >> 6
    return dst


def _check_up(a, g, gc, weights):
    a, g, gc, weights = np.asarray(a), np.asarray(g), np.asarray(gc), np.asarray(weights)
    assert a.ndim == 2 and a.dtype in LIMITS and g.ndim == 2 and g.dtype == np.uint8 and gc.dtype == np.uint8
    assert gc.shape == a.shape and a.shape == half_shape(g.shape[1], g.shape[0])[::-1]
    assert weights.shape == (256,) and weights.min() >= 1 and weights.max() <= 65535
    return a, g, gc, weights.astype(np.int64)


def scale(a):
    """v(c) of every coarse pixel -> int64"""
    lo, hi, off = LIMITS[np.asarray(a).dtype]
    return np.clip(2 * np.asarray(a).astype(np.int64) - off, lo, hi)


def upsample_double(a, g, gc, weights, fill=False):
    a, g, gc, weights = _check_up(a, g, gc, weights)
    h, w = g.shape
    ch, cw = a.shape
    pa = np.zeros((ch + 2, cw + 2), np.int64)
    pa[1:-1, 1:-1] = a
    pv = np.zeros((ch + 2, cw + 2), np.int64)
    pv[1:-1, 1:-1] = scale(a)
    pg = np.zeros((ch + 2, cw + 2), np.int64)
    pg[1:-1, 1:-1] = gc
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    X, Y, px, py = xs >> 1, ys >> 1, xs & 1, ys & 1
    fine = g.astype(np.int64)
    vals, wts = [], []
    for j in (-1, 0, 1):
        for i in (-1, 0, 1):
            raw = pa[Y + 1 + j, X + 1 + i]                            # (a padded tap has the value 0)
            wq = weights[np.abs(fine - pg[Y + 1 + j, X + 1 + i])] * S[px, i + 1] * S[py, j + 1]
            vals.append(pv[Y + 1 + j, X + 1 + i])
            wts.append(np.where(raw != 0, wq, 0))
    vals, wts = np.stack(vals), np.stack(wts)
    total = wts.sum(axis=0)
    order = np.argsort(vals, axis=0, kind="stable")
    vals, wts = np.take_along_axis(vals, order, axis=0), np.take_along_axis(wts, order, axis=0)
    # equal values are one step of the cumulated weight: the first tap (in sorted order) that has a weight and reaches
    # half of T is of the value looked for
    reached = (2 * np.cumsum(wts, axis=0) >= total[None]) & (wts > 0)
    wmed = np.take_along_axis(vals, np.argmax(reached, axis=0)[None], axis=0)[0]
    wmed = np.where(total > 0, wmed, 0)
    home = pa[Y + 1, X + 1]
    return np.where((home != 0) | bool(fill), wmed, 0).astype(a.dtype)


def upsample_double_naive(a, g, gc, weights, fill=False):
    a, g, gc, weights = _check_up(a, g, gc, weights)
    h, w = g.shape
    ch, cw = a.shape
    v = scale(a)
    out = np.zeros((h, w), a.dtype)
    for y in range(h):
        for x in range(w):
            X, Y, px, py = x >> 1, y >> 1, x & 1, y & 1
            if a[Y, X] == 0 and not fill:
                continue
            taps = [(int(v[Y + j, X + i]), int(weights[abs(int(g[y, x]) - int(gc[Y + j, X + i]))] * S[px][i + 1] * S[py][j + 1]))
                    for j in (-1, 0, 1) for i in (-1, 0, 1)
                    if 0 <= X + i < cw and 0 <= Y + j < ch and a[Y + j, X + i] != 0]
            total = sum(wq for _, wq in taps)
            for val in sorted({val for val, _ in taps}):
                if 2 * sum(wq for u, wq in taps if u <= val) >= total:
                    out[y, x] = val
                    break
    return out
