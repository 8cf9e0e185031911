"""Inputs for the tests of the half-resolution path (test_pyramid_cpu.py, test_pyramid_gpu.py): the named cases the GPU
runs, each made from a seed, with its expected result from the definition (tests/pyramid_reference.py), computed once;
and the definition with one mistake applied (reduce_mutant, upsample_mutant), by which the CPU test shows that the
cases can tell."""
import functools
import itertools

import numpy as np

from tests import pyramid_reference as pr
from tests.wmedian_patterns import guide_weights, random_guide, random_map

MAX_PAIRS = 3                       # of every plan the GPU cases run on
I32_MIN, I32_MAX = -2**31, 2**31 - 1

# ---------------------------------------------------------------------------
# reduce: a lane owns four coarse pixels (eight or ten source columns), a workgroup 256 x 4 coarse pixels
# ---------------------------------------------------------------------------
REDUCE_W = [1, 2, 3, 7, 8, 9, 63, 64, 65, 255, 257]
REDUCE_H = [1, 2, 3, 16, 17]
FILTERS = ["box", "binomial"]
CONTENTS = ["random", "all 255", "checkerboard", "random 2", "ramp", "random 3"]      # 2 * MAX_PAIRS images
# (first image, images) of the calls made on every size: 2 * max_pairs, one, and a partial batch
REDUCE_CALLS = [(0, 6), (1, 1), (2, 3)]
REDUCE_CASES = [dict(name=f"reduce {w}x{h}", w=w, h=h) for w in REDUCE_W for h in REDUCE_H]


@functools.lru_cache(maxsize=None)
def reduce_images(w, h):
    """-> uint8 [6][h][w], in the order of CONTENTS; read-only"""
    rng = np.random.default_rng(100 * w + h)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    imgs = np.stack([rng.integers(0, 256, (h, w)), np.full((h, w), 255), ((xx + yy) & 1) * 255,
                     rng.integers(0, 256, (h, w)), (xx * 7 + yy * 3) & 255, rng.integers(250, 256, (h, w))]).astype(np.uint8)
    imgs.setflags(write=False)
    return imgs


@functools.lru_cache(maxsize=None)
def reduce_expected(w, h, filter):
    out = np.stack([pr.reduce_half(img, filter) for img in reduce_images(w, h)])
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------
# upsample: a 64 x 16 fine tile over 32 x 8 coarse pixels and the ring around them
# ---------------------------------------------------------------------------
UP_W = [1, 2, 3, 63, 64, 65, 127, 129]
UP_H = [1, 2, 15, 16, 17, 33]
TABLES = ["ones", "max", "gw8"]


def table(name):
    return {"ones": np.ones(256, np.uint16), "max": np.full(256, 65535, np.uint16), "gw8": guide_weights(8)}[name]


def _up_cases():
    cases = []
    for dtype in ("int32", "int16"):
        for i, (w, h) in enumerate(itertools.product(UP_W, UP_H)):
            cases.append(dict(name=f"up {dtype} {w}x{h}", kind="random", dtype=dtype, w=w, h=h, invalid=(0.0, 0.3, 1.0)[i % 3],
                              fill=bool((i // 3) % 2), table=TABLES[(i // 6) % 3], pairs=(3, 1, 2)[(i // 2) % 3],
                              hi=(6, 2000)[(i // 4) % 2], negative=i % 5 < 2, reduced_guide=i % 2 == 0, seed=3000 + i))
        # the largest sum: every weight 65535 and every tap valid (T = 49 * 65535 inside)
        cases.append(dict(name=f"up max sum {dtype}", kind="random", dtype=dtype, w=65, h=17, invalid=0.0, fill=False,
                          table="max", pairs=1, hi=2000, negative=True, reduced_guide=True, seed=5))
        # the ends of the types (and the int16 input 8, which becomes 0) mixed in one neighbourhood
        for fill in (False, True):
            for tab in ("ones", "gw8"):
                cases.append(dict(name=f"up extremes {dtype} {tab} fill={int(fill)}", kind="extremes", dtype=dtype, w=70, h=20,
                                  fill=fill, table=tab, pairs=2, reduced_guide=fill, seed=17 + fill))
    return cases


UP_CASES = _up_cases()
UP_BY_NAME = {c["name"]: c for c in UP_CASES}
assert len(UP_BY_NAME) == len(UP_CASES)
EXTREMES = {"int32": [I32_MIN, I32_MIN + 1, -2**30 - 1, -1, 1, 2**30, I32_MAX - 1, I32_MAX],
            "int16": [-32768, -32767, -16377, -1, 1, 8, 9, 16391, 16392, 32767]}


@functools.lru_cache(maxsize=None)
def up_inputs(name):
    """-> (maps [pairs][ch][cw], guides [pairs][H][W] uint8, coarse guides [pairs][ch][cw] uint8, weights [256] uint16, fill)"""
    c = UP_BY_NAME[name]
    dtype, w, h, pairs = np.dtype(c["dtype"]), c["w"], c["h"], c["pairs"]
    cw, ch = pr.half_shape(w, h)
    if c["kind"] == "random":
        maps = np.stack([random_map(cw, ch, dtype, c["seed"] + 50 * q, c["invalid"], c["hi"], c["negative"]) for q in range(pairs)])
    else:
        rng = np.random.default_rng(c["seed"])
        vals = np.array(EXTREMES[c["dtype"]] + [0], np.int64)
        p = [0.9 / (len(vals) - 1)] * (len(vals) - 1) + [0.1]
        maps = rng.choice(vals, (pairs, ch, cw), p=p).astype(dtype)
    guides = np.stack([random_guide(w, h, c["seed"] + 50 * q) for q in range(pairs)])
    if c["reduced_guide"]:
        coarse = np.stack([pr.reduce_half(g, "binomial") for g in guides])
    else:
        coarse = np.stack([random_guide(cw, ch, c["seed"] + 50 * q + 9) for q in range(pairs)])
    weights = table(c["table"])
    for m in (maps, guides, coarse, weights):
        m.setflags(write=False)
    return maps, guides, coarse, weights, c["fill"]


@functools.lru_cache(maxsize=None)
def up_expected(name):
    maps, guides, coarse, weights, fill = up_inputs(name)
    out = np.stack([pr.upsample_double(m, g, gc, weights, fill) for m, g, gc in zip(maps, guides, coarse)])
    out.setflags(write=False)
    return out


def step_scene(w=82, h=34, edge=41, near=20, far=8, seed=1):
    """A gray step of 60 levels at the odd column `edge` with noise of +-3, and a disparity step of even shifts at the
    same column -> (fine truth: int32 web map [h][w], guide uint8 [h][w], coarse map: the truth sampled at (2X, 2Y),
    on the coarse scale (web = 1 + shift / 2))"""
    assert edge % 2 == 1 and near % 2 == 0 and far % 2 == 0
    rng = np.random.default_rng(seed)
    xx = np.broadcast_to(np.arange(w)[None, :], (h, w))
    g = np.clip(np.where(xx < edge, 90, 150) + rng.integers(-3, 4, (h, w)), 0, 255).astype(np.uint8)
    shift = np.where(xx < edge, near, far)
    truth = (1 + shift).astype(np.int32)
    coarse = (1 + shift[::2, ::2] // 2).astype(np.int32)
    return truth, g, coarse


# ---------------------------------------------------------------------------
# the definition with one mistake
# ---------------------------------------------------------------------------
REDUCE_MISTAKES = ["clamp at 255", "box rounds + 1", "binomial window offset by one"]
UP_MISTAKES = ["> for >= in the rank", "spatial table of the other parity", "home (x + 1) >> 1", "invalid taps counted",
               "scale 2 v"]


def reduce_mutant(src, filter, mistake):
    """pr.reduce_half with `mistake` (one of REDUCE_MISTAKES, or None)"""
    assert mistake is None or mistake in REDUCE_MISTAKES
    s = np.asarray(src).astype(np.int64)
    h, w = s.shape
    cw, ch = pr.half_shape(w, h)
    xs, ys = 2 * np.arange(cw), 2 * np.arange(ch)
    right = min(255, w - 1) if mistake == "clamp at 255" else w - 1
    acc = np.zeros((ch, cw), np.int64)
    if filter == "box":
        for j in range(2):
            for i in range(2):
                acc += s[np.clip(ys + j, 0, h - 1)][:, np.clip(xs + i, 0, right)]
        return ((acc + (1 if mistake == "box rounds + 1" else 2)) >> 2).astype(np.uint8)
    first = 0 if mistake == "binomial window offset by one" else -1
    for j in range(4):
        for i in range(4):
            acc += pr.K[i] * pr.K[j] * s[np.clip(ys - 1 + j, 0, h - 1)][:, np.clip(xs + first + i, 0, right)]
    return ((acc + 32) >> 6).astype(np.uint8)


def upsample_mutant(a, g, gc, weights, fill, mistake):
    """pr.upsample_double with `mistake` (one of UP_MISTAKES, or None)"""
    assert mistake is None or mistake in UP_MISTAKES
    a, g, gc, weights = np.asarray(a), np.asarray(g), np.asarray(gc), np.asarray(weights).astype(np.int64)
    h, w = g.shape
    ch, cw = a.shape
    lo, hi, off = pr.LIMITS[a.dtype]
    pad = 2                                                           # (the wrong home reaches one further)
    pa = np.zeros((ch + 2 * pad, cw + 2 * pad), np.int64)
    pa[pad:-pad, pad:-pad] = a
    pg = np.zeros_like(pa)
    pg[pad:-pad, pad:-pad] = gc
    inside = np.zeros(pa.shape, bool)
    inside[pad:-pad, pad:-pad] = True
    pv = np.clip(2 * pa - (0 if mistake == "scale 2 v" else off), lo, hi)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    px, py = xs & 1, ys & 1
    X, Y = ((xs + 1) >> 1, (ys + 1) >> 1) if mistake == "home (x + 1) >> 1" else (xs >> 1, ys >> 1)
    sx, sy = (1 - px, 1 - py) if mistake == "spatial table of the other parity" else (px, py)
    fine = g.astype(np.int64)
    vals, wts = [], []
    for j in (-1, 0, 1):
        for i in (-1, 0, 1):
            at = (Y + pad + j, X + pad + i)
            tap = inside[at] if mistake == "invalid taps counted" else inside[at] & (pa[at] != 0)
            vals.append(pv[at])
            wts.append(np.where(tap, weights[np.abs(fine - pg[at])] * pr.S[sx, i + 1] * pr.S[sy, j + 1], 0))
    vals, wts = np.stack(vals), np.stack(wts)
    total = wts.sum(axis=0)
    order = np.argsort(vals, axis=0, kind="stable")
    vals, wts = np.take_along_axis(vals, order, axis=0), np.take_along_axis(wts, order, axis=0)
    cum = np.cumsum(wts, axis=0)
    if mistake == "> for >= in the rank":
        # (the value at which the cumulated weight EXCEEDS half: equal values are one step, so the step's end counts)
        last = np.concatenate([vals[1:] != vals[:-1], np.ones((1,) + vals.shape[1:], bool)])
        full = np.where(last, cum, 0)
        for t in range(len(vals) - 2, -1, -1):
            full[t] = np.where(last[t], full[t], full[t + 1])
        reached = (2 * full > total[None]) & (wts > 0)
    else:
        reached = (2 * cum >= total[None]) & (wts > 0)
    wmed = np.take_along_axis(vals, np.argmax(reached, axis=0)[None], axis=0)[0]
    wmed = np.where(reached.any(axis=0), wmed, 0)
    home = pa[Y + pad, X + pad]
    return np.where((home != 0) | bool(fill), wmed, 0).astype(a.dtype)
