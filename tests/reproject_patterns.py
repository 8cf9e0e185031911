"""Sizes, maps and matrices for the reprojection tests (tests/test_reproject_cpu.py, tests/test_reproject_gpu.py).

The dense kernel gives a lane four consecutive pixels where W % 4 == 0 and the pointers allow it, one otherwise, 256
lanes a workgroup, at most 1024 workgroups a pair; the cloud works in tiles of 1024 pixels (four waves, four pixels a
lane) whose counts one workgroup of 256 lanes scans.  The sizes sit on and around those edges.  No pattern leads to
a float32 subnormal: finite non-zero results stay inside float32's normal range (the CPU test checks every pattern)."""
import numpy as np

from tests import reproject_reference as ref

TILE = ref.TILE
SCAN_LANES = 256
SMALL_SIZES = [(1, 1), (3, 3), (4, 4), (37, 5), (63, 5), (64, 9), (66, 7), (130, 33), (256, 9), (1024, 3)]
# W * H = TILE - 1, TILE, TILE + 1, and just over two tiles
TILE_SIZES = [(33, 31), (32, 32), (41, 25), (683, 3)]
# more tiles (257) than k_cloud_scan's workgroup has lanes: its loop runs twice (263168 pixels)
SCAN_LOOP_SIZE = (1028, 256)
SIZES = SMALL_SIZES + TILE_SIZES
assert [w * h for w, h in TILE_SIZES] == [TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
assert SCAN_LANES * TILE < SCAN_LOOP_SIZE[0] * SCAN_LOOP_SIZE[1] < 1000000

VALIDITY = ["all_valid", "all_zero", "first_only", "last_only", "checkerboard", "random_1", "random_50", "random_99"]
PATTERNS = VALIDITY + ["extremes"]
DTYPES = {ref.I32: np.int32, ref.I16: np.int16}
Z_GATES = [None, (2.0, 40.0)]
MISSING = [0.0, -1.0, float("inf"), float("nan")]


def values(pairs, w, h, dtype, seed):
    """plausible non-zero map values: web = 1 + shift in 1 .. 64, sub = 16 * (1 + shift) with sixteenths"""
    rng = np.random.default_rng(seed)
    if dtype == np.int32:
        return rng.integers(1, 65, (pairs, h, w)).astype(np.int32)
    return rng.integers(16, 1040, (pairs, h, w)).astype(np.int16)


def make_map(pattern, pairs, w, h, dtype, seed=0):
    """[pairs][H][W] of `dtype` with the validity of `pattern` (0 = invalid)"""
    v = values(pairs, w, h, dtype, seed)
    rng = np.random.default_rng(seed + 1000)
    if pattern == "all_valid":
        return v
    if pattern == "all_zero":
        return np.zeros_like(v)
    if pattern in ("first_only", "last_only"):
        m = np.zeros_like(v)
        i = 0 if pattern == "first_only" else w * h - 1
        m.reshape(pairs, -1)[:, i] = v.reshape(pairs, -1)[:, i]
        return m
    if pattern == "checkerboard":
        on = (np.arange(h)[:, None] + np.arange(w)[None, :]) % 2 == 0
        return np.where(on[None], v, 0).astype(dtype)
    if pattern.startswith("random_"):
        share = int(pattern.split("_")[1]) / 100.0
        return np.where(rng.random((pairs, h, w)) < share, v, 0).astype(dtype)
    if pattern == "extremes":
        info = np.iinfo(dtype)
        pool = np.array([info.min, info.max, -1, 1, 0, info.min + 1, info.max - 1, 2, 17, -16], dtype=dtype)
        return pool[rng.integers(0, len(pool), (pairs, h, w))]
    raise ValueError(pattern)


def rig(w, h, offset=3.5, baseline=0.12):
    """two calibrations (the rectified projections are what counts) and a baseline"""
    first = dict(new_fx=700.25, new_fy=701.5, new_cx=w / 2 - 0.25, new_cy=h / 2 + 0.125)       # (exact in binary: c2x - c1x IS the offset)
    second = dict(first, new_cx=first["new_cx"] + offset)
    return first, second, baseline


def matrices(w, h):
    """name -> 16 doubles"""
    rng = np.random.default_rng(w * 131 + h)
    dense = rng.uniform(0.5, 2.0, 16) * rng.choice([-1.0, 1.0], 16)
    crossing = ref.reprojection_matrix(*rig(w, h)).copy()
    crossing[12:] = [1.0, 0.0, 0.0, -float(w // 2)]           # Wh = x - W / 2: exactly 0 down one column
    return {
        "rig": ref.reprojection_matrix(*rig(w, h)),             # Z = f t / (d - 3.5): Wh = 0 where a sub map says 3.5
        "wh_crossing": crossing,
        "dense": dense,                                         # every entry non-zero
        "negative_z": ref.reprojection_matrix(*rig(w, h, offset=20.5)),   # Z < 0 for d < 20.5
    }


# ---------------------------------------------------------------------------
# the mutation audit's cases (profiles/mutants/README.md, third audit: J1, J2, J3, J5)
# ---------------------------------------------------------------------------

EDGE_W, EDGE_H = 8, 3                 # W % 4 == 0: four pixels a lane; EDGE_W - 1 columns of the same maps: one
EDGE_GATE = (2.0, 40.0)               # (Z_GATES' bounds)
FUSED_A = 1.0 + 2.0 ** -52            # 3 a = 3 + 1.5 ulp: a tie, rounded up to 3 + 2^-50 when the product is rounded
FUSED_B = -(2.0 - 2.0 ** -24 + 3 * 2.0 ** -52)


def edge_matrices():
    """name -> 16 doubles.  Wh = 1 in all three, Y = y and Z = d (the disparity itself), so that Z sits exactly on a
    gate's bounds where the map says so:
      z_is_d       X = x;
      x_overflows  X = 1e300 x: no float32 from column 1 on, while Y and Z stay finite;
      fused_tie    X = (a x + b y): at (x, y) = (3, 1) the double sum is 1 + 2^-24 + 2^-52, above the middle of the
                   float32 pair 1 and 1 + 2^-23, when a x is rounded on its own; formed with one rounding
                   (fused multiply-add) it is the middle itself, 1 + 2^-24, which goes to 1 (ties to even)."""
    base = np.zeros(16)
    base[0] = base[5] = base[10] = base[15] = 1.0
    over = base.copy()
    over[0] = 1e300
    fused = base.copy()
    fused[0], fused[1] = FUSED_A, FUSED_B
    return {"z_is_d": base, "x_overflows": over, "fused_tie": fused}


def edge_map(pairs, w, h, dtype):
    """every pixel valid, the even disparities 0, 2, 4, .. in raster order (every other pair: in reverse): d = 2 and
    d = 40, EDGE_GATE's bounds, occur in every pair of 21 pixels or more"""
    assert h * w >= 21
    d = (2 * np.arange(h * w)) % 64
    d = np.stack([d[::-1] if p % 2 else d for p in range(pairs)]).reshape(pairs, h, w)
    return (d + 1).astype(np.int32) if dtype == np.int32 else (16 * (d + 1)).astype(np.int16)


MISTAKES = ("z_min excluded", "z_max excluded", "X not tested", "row 0 fused")


def _fused_row0(q, x, y, d):
    """((fma(q0, x, q1 y) then fma(q2, d, .)) + q3 with each fused multiply-add rounded once (exact rationals,
    converted to the nearest double)"""
    from fractions import Fraction as Fr
    out = np.empty(x.shape)
    for i in np.ndindex(x.shape):
        inner = float(Fr(float(q[0])) * Fr(float(x[i])) + Fr(float(q[1] * y[i])))
        out[i] = float(Fr(float(q[2])) * Fr(float(d[i])) + Fr(inner)) + q[3]
    return out


def project_with(m, q, z_range, mistake):
    """ref.project with one mistake of MISTAKES made -> (Xf, Yf, Zf, kept)"""
    assert mistake in MISTAKES
    q = ref.check_q(q)
    lo, hi = ref.check_z(z_range)
    m = np.asarray(m)
    h, w = m.shape[-2:]
    d = ref.disparity(m)
    x = np.broadcast_to(np.arange(w, dtype=np.float64)[None, :], d.shape)
    y = np.broadcast_to(np.arange(h, dtype=np.float64)[:, None], d.shape)
    with np.errstate(all="ignore"):
        r = [((q[4 * i] * x + q[4 * i + 1] * y) + q[4 * i + 2] * d) + q[4 * i + 3] for i in range(4)]
        if mistake == "row 0 fused":
            r[0] = _fused_row0(q, x, y, d)
        xf, yf, zf = ((r[i] / r[3]).astype(np.float32) for i in range(3))
        above = lo < zf if mistake == "z_min excluded" else lo <= zf
        below = zf < hi if mistake == "z_max excluded" else zf <= hi
        finite = np.isfinite(yf) & np.isfinite(zf) & (True if mistake == "X not tested" else np.isfinite(xf))
        kept = (m != 0) & finite & above & below
    return xf, yf, zf, kept


def gray(pairs, w, h, seed):
    return np.random.default_rng(seed + 77).integers(0, 256, (pairs, h, w), dtype=np.uint8)
