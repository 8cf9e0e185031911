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


def gray(pairs, w, h, seed):
    return np.random.default_rng(seed + 77).integers(0, 256, (pairs, h, w), dtype=np.uint8)
