"""Inputs for the weighted-median tests (test_wmedian_cpu.py, test_wmedian_gpu.py): the named cases the GPU runs, each
made from a seed, with its expected result from the definition (tests/wmedian_reference.py), computed once; the
definition with one mistake applied (mutant), by which the CPU test shows that the cases can tell; and a model of the
kernel's bisection with a replaceable midpoint."""
import functools

import numpy as np

from tests import wmedian_reference as wr

TILE_W, TILE_H = 64, 16            # the kernel's tile (sm_filter.hip: FLT_TW, FLT_TH)
# widths and heights on and around every tile edge (64, 128; 16, 32), 1 and 2, and one smaller than every window
SIZES = [(1, 1), (1, 40), (70, 1), (2, 2), (15, 9), (63, 15), (64, 16), (65, 17), (127, 31), (128, 32), (129, 33), (66, 2),
         (3, 70), (200, 50)]
ALL_RADII = [(65, 17), (129, 33), (15, 9)]          # the sizes that also run radii 2, 4, 5 and 6
I32_MIN, I32_MAX = -2**31, 2**31 - 1


def guide_weights(sigma, peak=1024):
    """pipeline.guide_weights, repeated: the CPU tests need no library to make their inputs"""
    return np.maximum(1, np.rint(peak * np.exp(-np.arange(256) / sigma))).astype(np.uint16)


def table(name):
    d = np.arange(256)
    if name == "gw8":
        return guide_weights(8)
    if name == "gw32":
        return guide_weights(32)
    if name == "ones":
        return np.ones(256, np.uint16)
    if name == "max":
        return np.full(256, 65535, np.uint16)
    if name == "nonmono":                          # up and down, with zeros away from 0 (only weights[0] must be >= 1)
        return np.where(d % 5 == 3, 0, 1 + (d * 37 % 101) * 50).astype(np.uint16)
    raise KeyError(name)


def random_map(w, h, dtype, seed, invalid, hi, negative):
    rng = np.random.default_rng(seed)
    a = rng.integers(1, hi + 1, (h, w))
    if negative:
        a = np.where(rng.random((h, w)) < 0.4, -a, a)
    a[rng.random((h, w)) < invalid] = 0
    return a.astype(dtype)


def random_guide(w, h, seed):
    """blocks of a few gray levels (two of them 4 apart) with noise of +-3: differences from 0 to 230"""
    rng = np.random.default_rng(seed + 7777)
    levels = np.array([20, 60, 64, 130, 250])
    coarse = levels[rng.integers(0, len(levels), ((h + 3) // 4, (w + 4) // 5))]
    g = np.kron(coarse, np.ones((4, 5), np.int64))[:h, :w] + rng.integers(-3, 4, (h, w))
    return np.clip(g, 0, 255).astype(np.uint8)


def _random_cases():
    cases, i = [], 0
    for dtype in ("int32", "int16"):
        for w, h in SIZES:
            for radius in [1, 3, 7] + ([2, 4, 5, 6] if (w, h) in ALL_RADII else []):
                pairs, maxp = ((2, 2), (1, 3))[i % 2]                  # a full and a partial batch
                cases.append(dict(name=f"random {dtype} {w}x{h} r{radius}", kind="random", dtype=dtype, w=w, h=h,
                                  radius=radius, pairs=pairs, max_pairs=maxp, invalid=(0.0, 0.3, 0.7, 0.95)[(i // 2) % 4],
                                  fill=("off", "one", "median")[i % 3], table=("gw8", "gw32", "ones", "nonmono")[(i // 3) % 4],
                                  hi=(6, 2000)[(i // 4) % 2], negative=i % 5 < 2, seed=1000 + i))
                i += 1
    return cases


def _special_cases():
    cases = []
    # the largest sum: every weight 65535, radius 7, every pixel valid (T = 225 * 65535 inside)
    for dtype, (w, h) in (("int32", (65, 17)), ("int16", (129, 33))):
        cases.append(dict(name=f"max sum {dtype}", kind="random", dtype=dtype, w=w, h=h, radius=7, pairs=1, max_pairs=1,
                          invalid=0.0, fill="off", table="max", hi=2000, negative=True, seed=5))
    # the ends of the types mixed in one window, in the register path (radius 2) and the LDS path (radius 5)
    for dtype in ("int32", "int16"):
        for radius in (2, 5):
            for tab in ("ones", "gw32"):
                cases.append(dict(name=f"extremes {dtype} r{radius} {tab}", kind="extremes", dtype=dtype, w=70, h=20,
                                  radius=radius, pairs=1, max_pairs=1, fill="one", table=tab, seed=11 + radius))
    # the guide decides at tile borders: its step lies on x = 64 (pair 0) and on y = 16 (pair 1), the map's 4 beside
    for dtype in ("int32", "int16"):
        for radius in (3, 7):
            cases.append(dict(name=f"guide step {dtype} r{radius}", kind="step", dtype=dtype, w=130, h=35, radius=radius,
                              pairs=2, max_pairs=2, fill=("off", "median")[radius == 7], table="gw8", seed=radius))
    return cases


CASES = _random_cases() + _special_cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def step_scene(w, h, edge, offset, seed, along="x", invalid=0.0, near=40, far=24, dtype=np.int32):
    """A gray step at `edge` with noise of +-3 and a disparity step `offset` pixels further: the pixels in between
    are fattened (they carry the near side's value `near` on the far side of the image edge) -> (map, guide, fattened)"""
    rng = np.random.default_rng(seed)
    pos = np.arange(w)[None, :] if along == "x" else np.arange(h)[:, None]
    pos = np.broadcast_to(pos, (h, w))
    g = np.clip(np.where(pos < edge, 60, 180) + rng.integers(-3, 4, (h, w)), 0, 255).astype(np.uint8)
    a = np.where(pos < edge + offset, near, far)
    a = np.where(rng.random((h, w)) < invalid, 0, a).astype(dtype)
    return a, g, (pos >= edge) & (pos < edge + offset)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> (maps [pairs][H][W], guides [pairs][H][W] uint8, weights [256] uint16, fill, fill_min_weight)"""
    c = BY_NAME[name]
    dtype, w, h, pairs = np.dtype(c["dtype"]), c["w"], c["h"], c["pairs"]
    weights = table(c["table"])
    if c["kind"] == "random":
        maps = np.stack([random_map(w, h, dtype, c["seed"] + 50 * q, c["invalid"], c["hi"], c["negative"]) for q in range(pairs)])
        guides = np.stack([random_guide(w, h, c["seed"] + 50 * q) for q in range(pairs)])
    elif c["kind"] == "extremes":
        rng = np.random.default_rng(c["seed"])
        top = I32_MAX if dtype == np.int32 else 32767
        maps = rng.choice(np.array([-top, -1, 1, top, 0], np.int64), (pairs, h, w), p=[0.23, 0.23, 0.23, 0.23, 0.08]).astype(dtype)
        guides = np.stack([random_guide(w, h, c["seed"] + q) for q in range(pairs)])
    else:
        scenes = [step_scene(w, h, (TILE_W, TILE_H)[q], 4, c["seed"] + q, "xy"[q], 0.2, dtype=dtype) for q in range(pairs)]
        maps, guides = np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes])
    fmw = 1
    if c["fill"] == "median":                       # the lower median of T over pair 0's invalid pixels: a T that occurs
        t = np.sort(wr.totals(maps[0], guides[0], c["radius"], weights)[maps[0] == 0])
        fmw = max(1, int(t[(len(t) - 1) // 2])) if len(t) else 1
    for m in (maps, guides, weights):
        m.setflags(write=False)
    return maps, guides, weights, c["fill"] != "off", fmw


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> (maps [pairs][H][W], filled [pairs]) of the definition; computed once, shared, read-only"""
    maps, guides, weights, fill, fmw = inputs(name)
    res = [wr.weighted_median(m, g, BY_NAME[name]["radius"], weights, fill, fmw) for m, g in zip(maps, guides)]
    out, filled = np.stack([r[0] for r in res]), np.array([r[1] for r in res], np.int32)
    out.setflags(write=False)
    filled.setflags(write=False)
    return out, filled


# ---------------------------------------------------------------------------
# the definition with one mistake
# ---------------------------------------------------------------------------

MISTAKES = ["upper median", "weight from g(q) alone", "radius - 1", "invalid taps counted", "invalid centre is a tap",
            "fill threshold >"]


def mutant(a, g, radius, weights, fill, fill_min_weight, mistake):
    """wr.weighted_median with `mistake` (one of MISTAKES, or None) -> the filtered map"""
    assert mistake is None or mistake in MISTAKES
    a, g, weights = np.asarray(a), np.asarray(g), np.asarray(weights).astype(np.int64)
    h, w = a.shape
    r = radius - 1 if mistake == "radius - 1" else radius
    k = 2 * r + 1
    pa = np.zeros((h + 2 * r, w + 2 * r), np.int64)
    pa[r:r + h, r:r + w] = a
    pg = np.zeros((h + 2 * r, w + 2 * r), np.int64)
    pg[r:r + h, r:r + w] = g
    inside = np.zeros((h + 2 * r, w + 2 * r), bool)
    inside[r:r + h, r:r + w] = True
    win = [(dy, dx) for dy in range(k) for dx in range(k)]
    vals = np.stack([pa[dy:dy + h, dx:dx + w] for dy, dx in win])
    gray = np.stack([pg[dy:dy + h, dx:dx + w] for dy, dx in win])
    exists = np.stack([inside[dy:dy + h, dx:dx + w] for dy, dx in win])
    tap = exists & (vals != 0)
    if mistake == "invalid taps counted":
        tap = exists
    if mistake == "invalid centre is a tap":
        tap[r * k + r] = True
    wts = weights[gray] if mistake == "weight from g(q) alone" else weights[np.abs(gray - g.astype(np.int64)[None])]
    wts = np.where(tap, wts, 0)
    total = wts.sum(axis=0)
    order = np.argsort(vals, axis=0, kind="stable")
    vals, wts = np.take_along_axis(vals, order, axis=0), np.take_along_axis(wts, order, axis=0)
    cum = np.cumsum(wts, axis=0)
    if mistake == "upper median":
        # (the value at which the cumulated weight EXCEEDS half: equal values are one step, so the step's end counts)
        last = np.concatenate([vals[1:] != vals[:-1], np.ones((1,) + vals.shape[1:], bool)])
        full = np.where(last, cum, 0)
        for j in range(len(vals) - 2, -1, -1):                      # the cumulated weight at the end of each value's run
            full[j] = np.where(last[j], full[j], full[j + 1])
        reached = (2 * full > total[None]) & (wts > 0)
    else:
        reached = (2 * cum >= total[None]) & (wts > 0)
    wmed = np.take_along_axis(vals, np.argmax(reached, axis=0)[None], axis=0)[0]
    wmed = np.where(reached.any(axis=0), wmed, 0)
    enough = total > fill_min_weight if mistake == "fill threshold >" else total >= fill_min_weight
    return np.where(a != 0, wmed, np.where(enough, wmed, 0) if fill else 0).astype(a.dtype)


# ---------------------------------------------------------------------------
# the kernel's bisection, with the midpoint to be chosen
# ---------------------------------------------------------------------------

def wrap32(v):
    return (v + 2**31) % 2**32 - 2**31


def mid_unsigned(lo, hi):
    """what k_wmedian computes: lo + (unsigned difference >> 1)"""
    return wrap32(lo + (((hi - lo) % 2**32) >> 1))


def mid_int32_difference(lo, hi):
    """lo + (hi - lo) / 2 in int32: the difference wraps where hi - lo >= 2^31"""
    d = wrap32(hi - lo)
    return wrap32(lo + (abs(d) // 2) * (1 if d >= 0 else -1))


def mid_int32_sum(lo, hi):
    """(lo + hi) / 2 in int32: the sum wraps where both are large and of one sign"""
    s = wrap32(lo + hi)
    return (abs(s) // 2) * (1 if s >= 0 else -1)


def bisect(values, wts, midpoint, max_steps=80):
    """the smallest x in min .. max of `values` with 2 * cum(<= x) >= T, found as k_wmedian finds it (the taps given
    are the valid ones); gives up after max_steps (a wrong midpoint need not terminate)"""
    total, lo, hi = sum(wts), min(values), max(values)
    for _ in range(max_steps):
        if lo >= hi:
            break
        mid = midpoint(lo, hi)
        if 2 * sum(wq for v, wq in zip(values, wts) if v <= mid) >= total:
            hi = mid
        else:
            lo = wrap32(mid + 1)
    return lo


def window(a, g, radius, weights, x, y):
    """the valid taps of pixel (x, y) -> (values, weights), python ints"""
    h, w = a.shape
    taps = [(int(a[yy, xx]), int(weights[abs(int(g[y, x]) - int(g[yy, xx]))]))
            for yy in range(max(0, y - radius), min(h, y + radius + 1))
            for xx in range(max(0, x - radius), min(w, x + radius + 1)) if a[yy, xx] != 0]
    return [t[0] for t in taps], [t[1] for t in taps]
