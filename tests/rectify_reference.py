"""Stereo rectification, the definition (include/stereo_hip.h "rectification"): the remap of a
raw image through a fixed-point map (sm_rectify), the map of a calibration (sm_rectify_map_build) and the masking of a
disparity map by a validity image (sm_valid_mask).  Vectorised numpy, exact: the remap is integer arithmetic, the map
builder IEEE double with every operation rounded on its own (numpy rounds each ufunc separately), so the GPU is held
to both bit for bit.  tests/test_rectify_cpu.py pins the remap to per-pixel Python loops that share nothing with it.

A map is [H][W][2]: int32 (ABS32: the source position times 32) or int16 (REL16: that minus 32 * the destination
position); the dtype says which."""
import numpy as np

FRAC_BITS = 5
ONE = 1 << FRAC_BITS                     # 32: one source pixel
ABS32, REL16 = 0, 1                      # SM_RMAP_ABS32 / SM_RMAP_REL16
BILINEAR, NEAREST = 0, 1                 # SM_INTERP_BILINEAR / SM_INTERP_NEAREST
FORMATS = {"abs32": ABS32, "rel16": REL16}
INTERPS = {"bilinear": BILINEAR, "nearest": NEAREST}
INT32_MIN, INT32_MAX = -2**31, 2**31 - 1

# the fields of sm_rectify_calib, in its order (R row-major; new_*: the projection of the rectified image)
CALIB_FIELDS = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "R", "new_fx", "new_fy", "new_cx", "new_cy")


def calibration(fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0, R=None, new_fx=None, new_fy=None, new_cx=None,
                new_cy=None):
    """dict of CALIB_FIELDS; the new projection defaults to the camera matrix, R to the identity"""
    R = np.eye(3) if R is None else np.asarray(R, np.float64).reshape(3, 3)
    return dict(fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy), k1=float(k1), k2=float(k2), p1=float(p1),
                p2=float(p2), k3=float(k3), R=R, new_fx=float(fx if new_fx is None else new_fx),
                new_fy=float(fy if new_fy is None else new_fy), new_cx=float(cx if new_cx is None else new_cx),
                new_cy=float(cy if new_cy is None else new_cy))


def positions(m):
    """a map of either format -> (mx, my), int64 [H][W]: the source position of every destination pixel, times 32"""
    m = np.asarray(m)
    assert m.ndim == 3 and m.shape[2] == 2 and m.dtype in (np.int32, np.int16), (m.shape, m.dtype)
    mx, my = m[..., 0].astype(np.int64), m[..., 1].astype(np.int64)
    if m.dtype == np.int16:
        h, w = m.shape[:2]
        mx = mx + ONE * np.arange(w, dtype=np.int64)[None, :]
        my = my + ONE * np.arange(h, dtype=np.int64)[:, None]
    return mx, my


def abs_map(mx, my):
    return np.stack([mx, my], axis=-1).astype(np.int32)


def rel_map(mx, my):
    """REL16 map of the positions; ValueError where a displacement leaves int16 (sm_rectify_map_build refuses)"""
    mx, my = np.asarray(mx, np.int64), np.asarray(my, np.int64)
    h, w = mx.shape
    dx = mx - ONE * np.arange(w, dtype=np.int64)[None, :]
    dy = my - ONE * np.arange(h, dtype=np.int64)[:, None]
    d = np.stack([dx, dy], axis=-1)
    if d.min() < -32768 or d.max() > 32767:
        raise ValueError(f"displacements {int(d.min())} .. {int(d.max())} thirty-seconds of a pixel do not fit int16: "
                         "use the abs32 format")
    return d.astype(np.int16)


def identity_map(w, h, fmt="abs32"):
    mx = np.broadcast_to(ONE * np.arange(w, dtype=np.int64)[None, :], (h, w))
    my = np.broadcast_to(ONE * np.arange(h, dtype=np.int64)[:, None], (h, w))
    return abs_map(mx, my) if FORMATS[fmt] == ABS32 else rel_map(mx, my)


def _inside(src, xs, ys):
    sh, sw = src.shape
    return (xs >= 0) & (xs < sw) & (ys >= 0) & (ys < sh)


def _tap(src, xs, ys, border):
    """src(xs, ys) where inside, else border -> int64"""
    sh, sw = src.shape
    inside = _inside(src, xs, ys)
    v = src[np.clip(ys, 0, sh - 1), np.clip(xs, 0, sw - 1)].astype(np.int64)
    return np.where(inside, v, border)


def remap(src, m, interp="bilinear", border=0):
    """src [src_h][src_w] u8, m a map of W x H -> (out [H][W] u8, valid [H][W] u8)"""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 2 and 0 <= border <= 255
    mx, my = positions(m)
    if INTERPS[interp] == NEAREST:
        xs, ys = (mx + 16) >> FRAC_BITS, (my + 16) >> FRAC_BITS
        return _tap(src, xs, ys, border).astype(np.uint8), _inside(src, xs, ys).astype(np.uint8)
    x0, y0 = mx >> FRAC_BITS, my >> FRAC_BITS                    # arithmetic shifts: floor
    fx, fy = mx & (ONE - 1), my & (ONE - 1)
    acc = np.full(mx.shape, 512, np.int64)
    valid = np.ones(mx.shape, bool)
    for i, j, wgt in ((0, 0, (ONE - fx) * (ONE - fy)), (1, 0, fx * (ONE - fy)), (0, 1, (ONE - fx) * fy), (1, 1, fx * fy)):
        acc += wgt * _tap(src, x0 + i, y0 + j, border)
        valid &= (wgt == 0) | _inside(src, x0 + i, y0 + j)
    return (acc >> 10).astype(np.uint8), valid.astype(np.uint8)


def rectify(raw_left, raw_right, map_left, map_right, interp="bilinear", border=0):
    """what one sm_rectify call writes for batches [pairs][src_h][src_w] -> (left, right, valid_left, valid_right)"""
    outs = []
    for raw, m in ((raw_left, map_left), (raw_right, map_right)):
        res = [remap(a, m, interp, border) for a in raw]
        outs.append((np.stack([r[0] for r in res]), np.stack([r[1] for r in res])))
    return outs[0][0], outs[1][0], outs[0][1], outs[1][1]


def build_positions(c, w, h):
    """(mx, my) int64 of a calibration.  THE parenthesisation: the kernel is written from these lines."""
    R = np.asarray(c["R"], np.float64).reshape(3, 3)
    x = np.broadcast_to(np.arange(w, dtype=np.float64)[None, :], (h, w))
    y = np.broadcast_to(np.arange(h, dtype=np.float64)[:, None], (h, w))
    k1, k2, k3, p1, p2 = (np.float64(c[k]) for k in ("k1", "k2", "k3", "p1", "p2"))
    with np.errstate(all="ignore"):
        xn = (x - c["new_cx"]) / c["new_fx"]
        yn = (y - c["new_cy"]) / c["new_fy"]
        X = (R[0, 0] * xn + R[1, 0] * yn) + R[2, 0]                # R transposed, sums left to right
        Y = (R[0, 1] * xn + R[1, 1] * yn) + R[2, 1]
        Z = (R[0, 2] * xn + R[1, 2] * yn) + R[2, 2]
        a = X / Z
        b = Y / Z
        r2 = a * a + b * b
        rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        ad = a * rad + (((2.0 * p1) * a) * b + p2 * (r2 + (2.0 * a) * a))
        bd = b * rad + (p1 * (r2 + (2.0 * b) * b) + ((2.0 * p2) * a) * b)
        u = c["fx"] * ad + c["cx"]
        v = c["fy"] * bd + c["cy"]
        tx = np.floor(u * 32.0 + 0.5)
        ty = np.floor(v * 32.0 + 0.5)
        bad = ~(np.isfinite(u) & np.isfinite(v))                   # Z = 0: far outside, both coordinates
        tx = np.where(bad, float(INT32_MIN), np.clip(tx, float(INT32_MIN), float(INT32_MAX)))
        ty = np.where(bad, float(INT32_MIN), np.clip(ty, float(INT32_MIN), float(INT32_MAX)))
    return tx.astype(np.int64), ty.astype(np.int64)


def build_map(c, w, h, fmt="rel16"):
    """the map sm_rectify_map_build writes; ValueError where it refuses (REL16 and a displacement outside int16)"""
    mx, my = build_positions(c, w, h)
    return abs_map(mx, my) if FORMATS[fmt] == ABS32 else rel_map(mx, my)


def valid_mask(m, valid):
    """a disparity map (int32 web or int16 sub) with 0 where valid = 0"""
    m = np.asarray(m)
    return np.where(np.asarray(valid) != 0, m, 0).astype(m.dtype)
