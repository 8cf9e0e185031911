"""Inputs for the smoother's tests (test_wls_cpu.py, test_wls_gpu.py): the named cases the GPU runs, each made from a
seed, with its expected result from the definition (tests/wls_reference.py), computed once; the scene that shows what
the stage is for; and the definition with one mistake applied (mutant), by which the CPU test shows that the cases see
single roundings."""
import functools

import numpy as np

from tests import wls_reference as wr

CHUNK = 16                         # columns of a row-kernel chunk (sm_wls.hip: WLS_C); 64 rows or columns make a wave
# single-element lines; a partial last wave of rows (65, 67, 70) or columns (65, 70, 130, 257); a partial last chunk
# (17, 33, 65 ...); exactly one chunk (16), two (32), one wave of rows (64) and of columns (64)
SIZES = [(1, 1), (1, 5), (5, 1), (2, 2), (16, 64), (17, 65), (33, 70), (80, 33), (130, 67), (257, 3), (32, 2), (64, 5)]
I32_MIN, I32_MAX = -2**31, 2**31 - 1
TYPES = [("int32", "int32"), ("int16", "int16"), ("int32", "int16"), ("int16", "int32")]


def guide_weights(sigma, peak=1024):
    """pipeline.guide_weights, repeated: the CPU tests need no library to make their inputs"""
    return np.maximum(1, np.rint(peak * np.exp(-np.arange(256) / sigma))).astype(np.uint16)


def table(name):
    d = np.arange(256)
    if name == "gw8":
        return guide_weights(8)
    if name == "gw32":
        return guide_weights(32)
    if name == "zero":
        return np.zeros(256, np.uint16)
    if name == "holes":                            # isolated zeros, weights[0] among them, in a table that goes up and down
        return np.where(d % 5 == 0, 0, 200 + (d * 37 % 101) * 9).astype(np.uint16)
    if name == "max":
        return np.full(256, 65535, np.uint16)
    raise KeyError(name)


def random_map(w, h, dtype, seed, invalid, negative):
    """values of a few dozen pixels' disparity: 1 .. 128 shifts (int32) or 16 .. 2048 sixteenths (int16), some negative"""
    rng = np.random.default_rng(seed)
    a = rng.integers(1, 129, (h, w)) if np.dtype(dtype) == np.int32 else rng.integers(16, 2049, (h, w))
    if negative:
        a = np.where(rng.random((h, w)) < 0.3, -a, a)
    a[rng.random((h, w)) < invalid] = 0
    return a.astype(dtype)


def random_guide(w, h, seed):
    """blocks of a few gray levels (two of them 4 apart) with noise of +-3: differences from 0 to 230"""
    rng = np.random.default_rng(seed + 4242)
    levels = np.array([20, 60, 64, 130, 250])
    coarse = levels[rng.integers(0, len(levels), ((h + 3) // 4, (w + 4) // 5))]
    g = np.kron(coarse, np.ones((4, 5), np.int64))[:h, :w] + rng.integers(-3, 4, (h, w))
    return np.clip(g, 0, 255).astype(np.uint8)


def random_conf(w, h, seed):
    """every byte value, zeros among them"""
    rng = np.random.default_rng(seed + 99)
    c = rng.integers(0, 256, (h, w))
    c[rng.random((h, w)) < 0.1] = 0
    return c.astype(np.uint8)


def _cases():
    cases, i = [], 0
    for w, h in SIZES:
        for _ in range(2):
            tin, tout = TYPES[i % 4]
            pairs = (1, 3, 2)[i % 3]
            cases.append(dict(name=f"random {w}x{h} {tin}->{tout} T{1 + i % 4}", kind="random", w=w, h=h, tin=tin, tout=tout,
                              pairs=pairs, max_pairs=3, conf=i % 3 != 1, T=1 + i % 4, lam=(1 / 16, 0.5, 4.0)[(i // 2) % 3],
                              table=("gw8", "gw32", "holes")[(i // 4) % 3], invalid=(0.3, 0.0, 0.6)[(i // 3) % 3],
                              negative=i % 5 == 2, flags=wr.NO_FILL if i % 4 == 3 else 0, seed=3000 + i))
            i += 1
    base = dict(kind="special", pairs=2, max_pairs=3, conf=True, T=2, lam=0.5, table="gw8", invalid=0.3, negative=False,
                flags=0, tin="int16", tout="int16")
    cases.append(dict(base, name="eight passes", w=33, h=70, T=8, lam=2.0, tin="int32", seed=1))
    cases.append(dict(base, name="lambda zero", w=17, h=65, lam=0.0, tout="int32", seed=2))
    cases.append(dict(base, name="zero table", w=17, h=65, table="zero", tin="int32", tout="int32", seed=3))
    cases.append(dict(base, name="largest links", w=33, h=70, table="max", lam=float(2**20), T=1, seed=4))
    cases.append(dict(base, name="invalid rows and columns", kind="bands", w=33, h=70, T=3, seed=5))
    cases.append(dict(base, name="invalid rows and columns, no fill", kind="bands", w=33, h=70, T=3, flags=wr.NO_FILL,
                      conf=False, tin="int32", seed=6))
    for tin, tout in TYPES:
        # (weak links, at most 0.1: a pixel keeps most of its own value, so the results stay near the ends)
        cases.append(dict(base, name=f"extremes {tin}->{tout}", kind="extremes", w=80, h=33, tin=tin, tout=tout, lam=2.0**-12,
                          seed=7))
    return cases


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> (maps [pairs][H][W], guides u8 [pairs][H][W], conf u8 [pairs][H][W] or None, weights [256] uint16)"""
    c = BY_NAME[name]
    dtype, w, h, pairs = np.dtype(c["tin"]), c["w"], c["h"], c["pairs"]
    seeds = [c["seed"] + 50 * q for q in range(pairs)]
    guides = np.stack([random_guide(w, h, s) for s in seeds])
    conf = np.stack([random_conf(w, h, s) for s in seeds]) if c["conf"] else None
    if c["kind"] == "extremes":
        rng = np.random.default_rng(c["seed"])
        lo, hi = (I32_MIN, I32_MAX) if dtype == np.int32 else (-32768, 32767)
        maps = rng.choice(np.array([lo, lo + 1, -1, 1, hi - 1, hi, 0], np.int64), (pairs, h, w),
                          p=[0.1, 0.1, 0.1, 0.1, 0.1, 0.4, 0.1]).astype(dtype)
    else:
        maps = np.stack([random_map(w, h, dtype, s, c["invalid"], c["negative"]) for s in seeds])
    if c["kind"] == "bands":                       # whole rows and columns without a valid pixel, at both ends and inside
        maps = maps.copy()
        maps[:, [0, 1, 20, 21, 22, h - 1], :] = 0
        maps[:, :, [0, 7, 8, 15, 16, w - 2, w - 1]] = 0
    weights = table(c["table"])
    for m in (maps, guides, conf, weights):
        if m is not None:
            m.setflags(write=False)
    return maps, guides, conf, weights


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> (out [pairs][H][W] of the case's output type, raw [pairs][H][W] float64, filled [pairs] int32) of the
    definition; computed once, shared, read-only"""
    c = BY_NAME[name]
    maps, guides, conf, weights = inputs(name)
    res = [wr.wls_filter(maps[q], guides[q], weights, c["lam"], c["T"], None if conf is None else conf[q], c["flags"],
                         c["tout"]) for q in range(c["pairs"])]
    out = (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.array([r[2] for r in res], np.int32))
    for m in out:
        m.setflags(write=False)
    return out


# ---------------------------------------------------------------------------
# what the stage is for: one scene
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def scene(w=80, h=33, edge=40, seed=1):
    """A gray step at x = edge (60 | 180, noise of +-3) over a disparity step (16 x 21 | 16 x 41 sixteenths, noise of +-12):
    30 % holes, 5 % outliers (uniform in 16 x 2 .. 16 x 99, confidence 0 .. 19), the rest with confidence 200
    -> (map int16, guide, conf, truth float64, outlier mask)"""
    rng = np.random.default_rng(seed)
    left = np.broadcast_to(np.arange(w)[None, :] < edge, (h, w))
    guide = np.clip(np.where(left, 60, 180) + rng.integers(-3, 4, (h, w)), 0, 255).astype(np.uint8)
    truth = np.where(left, 16.0 * 21, 16.0 * 41)
    a = truth.astype(np.int64) + rng.integers(-12, 13, (h, w))
    conf = np.full((h, w), 200, np.int64)
    r = rng.random((h, w))
    outlier = (r >= 0.30) & (r < 0.35)
    a = np.where(outlier, rng.integers(16 * 2, 16 * 99 + 1, (h, w)), a)
    conf = np.where(outlier, rng.integers(0, 20, (h, w)), conf)
    a = np.where(r < 0.30, 0, a)
    res = (a.astype(np.int16), guide, conf.astype(np.uint8), truth, outlier)
    for m in res:
        m.setflags(write=False)
    return res


# ---------------------------------------------------------------------------
# the definition with one mistake
# ---------------------------------------------------------------------------

MISTAKES = ["links shifted by one", "lambdas reversed", "columns first", "confidence kept at invalid pixels",
            "division by den", "b summed from the right"]


def _solve(planes, links, mistake):
    m, n = planes[0].shape
    if n == 1:
        return [p.copy() for p in planes]
    if mistake == "links shifted by one":
        links = np.concatenate([links[:, 1:], links[:, -1:]], axis=1)
    zero = np.zeros((m, 1))
    lp, ln = np.concatenate([zero, links], axis=1), np.concatenate([links, zero], axis=1)
    a, k = -lp, -ln
    b = 1.0 + (lp + ln) if mistake == "b summed from the right" else (1.0 + lp) + ln
    cp, fp = np.empty((m, n)), [np.empty((m, n)) for _ in planes]
    for i in range(n):
        den = b[:, i] if i == 0 else b[:, i] - cp[:, i - 1] * a[:, i]
        inv = 1.0 / den
        cp[:, i] = k[:, i] * inv
        for f, p in zip(fp, planes):
            t = p[:, i] if i == 0 else p[:, i] - f[:, i - 1] * a[:, i]
            f[:, i] = t / den if mistake == "division by den" else t * inv
    out = [np.empty((m, n)) for _ in planes]
    for u, f in zip(out, fp):
        u[:, n - 1] = f[:, n - 1]
        for i in range(n - 2, -1, -1):
            u[:, i] = f[:, i] - cp[:, i] * u[:, i + 1]
    return out


def mutant(a, guide, weights, lam, iterations, conf, flags, mistake):
    """wr.wls_filter with `mistake` (one of MISTAKES, or None) -> raw"""
    assert mistake is None or mistake in MISTAKES
    a = np.asarray(a)
    N, M = wr.start_planes(a, conf)
    if mistake == "confidence kept at invalid pixels":
        M = np.full(a.shape, 255.0) if conf is None else np.asarray(conf).astype(np.float64)
    g = np.asarray(guide).astype(np.int64)
    wd = np.asarray(weights).astype(np.float64)
    wrow, wcol = wd[np.abs(g[:, :-1] - g[:, 1:])], wd[np.abs(g[:-1, :] - g[1:, :])].T
    lams = wr.lambdas(lam, iterations)
    for lam_t in (lams[::-1] if mistake == "lambdas reversed" else lams):
        for sweep in ("cr" if mistake == "columns first" else "rc"):
            if sweep == "r":
                N, M = _solve([N, M], lam_t * wrow, mistake)
            else:
                N, M = (p.T for p in _solve([np.ascontiguousarray(N.T), np.ascontiguousarray(M.T)], lam_t * wcol, mistake))
    return wr.finish(a, np.ascontiguousarray(N), np.ascontiguousarray(M), flags, a.dtype)[1]
