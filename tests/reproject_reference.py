"""The definition of the reprojection stage (include/stereo_hip.h "reprojection"), vectorised in numpy: what
sm_reproject, sm_point_cloud and sm_reproject_q are held to, bit for bit.

Every operation is an IEEE double +, * or / rounded on its own, in the order written here, followed by one double ->
float32 conversion; numpy rounds all of them correctly (round to nearest even), and evaluates an expression one
operation at a time, so the parentheses below ARE the definition."""
import numpy as np

I32, I16 = 0, 1                     # SM_MAP_I32, SM_MAP_I16
TILE = 1024                         # pixels per tile of sm_point_cloud's workspace (the header's formula)


def workspace_bytes(w, h, max_pairs):
    """what sm_plan_reserve_cloud adds to sm_plan_workspace_bytes"""
    return 4 * max_pairs * ((w * h + TILE - 1) // TILE)


def disparity(m):
    """the exact double disparity of an int32 (web) or int16 (sub, 1/16 shift) map"""
    m = np.asarray(m)
    if m.dtype == np.int32:
        return m.astype(np.float64) - 1.0
    if m.dtype == np.int16:
        return m.astype(np.float64) / 16.0 - 1.0
    raise ValueError(f"a map is int32 or int16, not {m.dtype}")


def check_q(q):
    q = np.asarray(q, dtype=np.float64).reshape(16)
    if not np.isfinite(q).all():
        raise ValueError("q: every entry must be finite")
    return q


def check_z(z_range):
    lo, hi = (-np.inf, np.inf) if z_range is None else z_range
    lo, hi = np.float32(lo), np.float32(hi)
    if np.isnan(lo) or np.isnan(hi) or lo > hi:
        raise ValueError("z_range: a NaN bound, or z_min > z_max")
    return lo, hi


def project(m, q, z_range=None):
    """map [..., H, W] -> (Xf, Yf, Zf) float32 and the kept mask"""
    q = check_q(q)
    lo, hi = check_z(z_range)
    m = np.asarray(m)
    h, w = m.shape[-2:]
    d = disparity(m)
    x = np.broadcast_to(np.arange(w, dtype=np.float64)[None, :], (h, w))
    y = np.broadcast_to(np.arange(h, dtype=np.float64)[:, None], (h, w))
    with np.errstate(all="ignore"):
        r = [((q[4 * i] * x + q[4 * i + 1] * y) + q[4 * i + 2] * d) + q[4 * i + 3] for i in range(4)]
        xf, yf, zf = ((r[i] / r[3]).astype(np.float32) for i in range(3))
        kept = (m != 0) & np.isfinite(xf) & np.isfinite(yf) & np.isfinite(zf) & (lo <= zf) & (zf <= hi)
    return xf, yf, zf, kept


def reproject(m, q, missing=0.0, z_range=None):
    """-> depth [..., H, W], xyz [..., H, W, 3] (float32, `missing` where not kept), kept pixels per pair"""
    xf, yf, zf, kept = project(m, q, z_range)
    miss = np.float32(missing)
    depth = np.where(kept, zf, miss).astype(np.float32)
    xyz = np.where(kept[..., None], np.stack([xf, yf, zf], axis=-1), miss).astype(np.float32)
    return depth, xyz, kept.reshape(kept.shape[:-2] + (-1,)).sum(axis=-1).astype(np.int32)


def point_cloud(m, q, gray=None, z_range=None):
    """one map [H, W] -> records [count, 4] float32 (X, Y, Z, I) in raster order, and index [count] int32 (y W + x)"""
    m = np.asarray(m)
    assert m.ndim == 2
    xf, yf, zf, kept = project(m, q, z_range)
    idx = np.flatnonzero(kept.reshape(-1))                   # ascending: y outer, x inner
    inten = np.zeros(len(idx), np.float32) if gray is None else np.asarray(gray).reshape(-1)[idx].astype(np.float32)
    pts = np.stack([xf.reshape(-1)[idx], yf.reshape(-1)[idx], zf.reshape(-1)[idx], inten], axis=-1).astype(np.float32)
    return pts.reshape(-1, 4), idx.astype(np.int32)


def reprojection_matrix(first, second, baseline):
    """sm_reproject_q: first / second are dicts with new_fx, new_fy, new_cx, new_cy -> 16 doubles, row-major"""
    f, fy = np.float64(first["new_fx"]), np.float64(first["new_fy"])
    c1x, c1y, c2x = np.float64(first["new_cx"]), np.float64(first["new_cy"]), np.float64(second["new_cx"])
    t = np.float64(baseline)
    if not np.isfinite(t) or t == 0.0:
        raise ValueError("baseline: zero or not finite")
    if not (np.isfinite(f) and f > 0 and np.isfinite(fy) and fy > 0):
        raise ValueError("new_fx / new_fy: not positive and finite")
    r = f / fy
    q = np.zeros(16)
    q[0] = 1.0
    q[3] = -c1x
    q[5] = r
    q[7] = -(c1y * r)
    q[11] = f
    q[14] = 1.0 / t
    q[15] = -((c2x - c1x) / t)
    return q
