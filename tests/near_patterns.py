"""Inputs for the guided re-search tests (test_near_cpu.py, test_near_gpu.py): the named cases the GPU runs, each made
from a seed, with its expected result from the definition (tests/near_reference.py), computed once; and the
definition with one mistake applied (the "mutants"), which the CPU test shows the cases can tell from the definition.

The kernel works on tiles of 64 x 16 pixels with a halo of the window, and keeps the wanted shifts of a tile in a mask
of 32-bit words: the sizes sit around the tile and its halo (1, 2, 3, 63, 64, 65, 127, 129 columns; 1, 2, 15, 16, 17,
33 rows), the shift counts on every edge of a mask word (1, 4, 31, 33, 64, 130, 512).  The factors are spread over
the cases rather than multiplied out."""
from __future__ import annotations

import functools
import itertools

import numpy as np

from tests import census_extreme_patterns as xp
from tests import near_reference as nr
from tests.census_reference import mirror, transform
from tests.cost_lr_reference import _box

I32_MIN, I32_MAX = -2**31, 2**31 - 1
WIDTHS = [1, 2, 3, 63, 64, 65, 127, 129]
HEIGHTS = [1, 2, 15, 16, 17, 33]
WINDOWS = [1, 3, 5, 9, 25]
SHIFTS = [1, 4, 31, 33, 64, 130, 512]
CENSUS = [3, 5, 7]
RADII = [1, 2, 4]
MODES = ["toroidal", "ghost"]
PRIORS = ["const", "surfaces", "noise", "zeros30", "zeros100", "extremes", "border"]
MAX_PAIRS = 3


def _cases():
    cases = []
    sizes = list(itertools.product(WIDTHS, HEIGHTS))
    for k in range(2 * len(sizes)):
        w, h = sizes[k % len(sizes)]
        m = k // len(sizes)
        # (a plan takes square_width <= min(W, H): an even one equal to W gives a window n = W + 1 wider than the image)
        cases.append(dict(name=f"grid {k}", kind="random", w=w, h=h, mode=MODES[(m + k) % 2], sw=min(WINDOWS[k % 5], w, h),
                          d=SHIFTS[(k + 2 * m) % 7], census=CENSUS[(k + m) % 3], radius=RADII[(k // 3 + m) % 3],
                          pairs=(3, 1, 2)[(k // 2) % 3], prior=PRIORS[(k + 3 * m) % 7], levels=(256, 4)[(k // 5) % 2],
                          max_diff=k % 2, seed=7000 + k))
    # a tile that wants more than 32 distinct shifts, of every mask word, at every census width
    for i, (mode, census) in enumerate(itertools.product(MODES, CENSUS)):
        cases.append(dict(name=f"noise {mode} c={census}", kind="random", w=129, h=33, mode=mode, sw=(5, 9, 3)[i % 3],
                          d=(512, 130, 64)[i % 3], census=census, radius=RADII[i % 3], pairs=1, prior="noise", levels=256,
                          max_diff=1, seed=7200 + i))
    # the widest window (a halo of 12 on every side of the tile) at the narrow census widths, more than one tile
    for i, (mode, census) in enumerate(itertools.product(MODES, (3, 5))):
        cases.append(dict(name=f"window 25 {mode} c={census}", kind="random", w=(65, 129)[i % 2], h=33, mode=mode, sw=25,
                          d=(33, 64)[i // 2], census=census, radius=RADII[(i + 1) % 3], pairs=(2, 1)[i % 2],
                          prior=("surfaces", "border", "zeros30", "extremes")[i], levels=256, max_diff=1, seed=7250 + i))
    # a plan with D <= radius + 1: any prior in 1 .. D gives census_wta's result
    cases.append(dict(name="few shifts", kind="random", w=65, h=17, mode="ghost", sw=5, d=3, census=5, radius=2, pairs=2,
                      prior="noise1", levels=256, max_diff=0, seed=7300))
    # a constant gray pair: every cost ties at 0, web = 1 + max(0, s - 1 - r)
    for i, mode in enumerate(MODES):
        cases.append(dict(name=f"all tie {mode}", kind="gray", w=70, h=20, mode=mode, sw=9, d=40, census=7, radius=(2, 4)[i],
                          pairs=1, prior="noise", levels=1, max_diff=0, seed=7310 + i))
    # A = 30000 at the last shift of every pixel (census_extreme_patterns.anti: n = 25, c = 7), the only candidate where
    # the prior is D + r: the key's top field and the u16 sums
    cases.append(dict(name="maximum cost", kind="anti", w=98, h=28, mode="toroidal", sw=25, d=8, census=7, radius=1, pairs=1,
                      prior="last", levels=256, max_diff=0, seed=7320))
    return cases


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def make_prior(kind, w, h, d, radius, rng):
    """one int32 prior map"""
    yy, xx = np.mgrid[0:h, 0:w]
    surfaces = rng.integers(1, d + 1, (h // 11 + 1, w // 24 + 1))[yy // 11, xx // 24]      # 2 - 4 per 64 x 16 tile
    if kind == "const":
        p = np.full((h, w), rng.integers(1, d + 1))
    elif kind == "surfaces":
        p = surfaces
    elif kind == "noise":
        p = rng.integers(0, d + 1, (h, w))
    elif kind == "noise1":
        p = rng.integers(1, d + 1, (h, w))
    elif kind == "zeros30":
        p = np.where(rng.random((h, w)) < 0.3, 0, surfaces)
    elif kind == "zeros100":
        p = np.zeros((h, w))
    elif kind == "extremes":
        vals = np.array([I32_MIN, I32_MAX, -radius, 1 - radius, d + radius, d + radius + 1, 0, 1, d, -1, I32_MIN + 1,
                         I32_MAX - 1], np.int64)
        p = rng.choice(vals, (h, w))
    elif kind == "border":
        # the largest shifts: x + d runs across the right border (and u - d across the left one in the right pass)
        p = rng.integers(max(1, d - 2), d + 1, (h // 5 + 1, w // 7 + 1))[yy // 5, xx // 7]
    elif kind == "last":
        p = rng.integers(d - 1, d + radius + 1, (h, w))     # d + radius: K is the last shift alone
    else:
        raise ValueError(kind)
    return np.asarray(p, np.int64).astype(np.int32)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> (left, right uint8 [pairs][H][W], prior, prior_right int32 [pairs][H][W])"""
    c = BY_NAME[name]
    w, h, pairs = c["w"], c["h"], c["pairs"]
    rng = np.random.default_rng(c["seed"])
    if c["kind"] == "anti":
        l, r = xp.anti(w, h, c["d"] - 1)
        left, right = l[None].copy(), r[None].copy()
    elif c["kind"] == "gray":
        # (ghost: gray 0, the value the halo reads, so that the descriptors at the border are 0 as well)
        left = np.full((pairs, h, w), 97 if c["mode"] == "toroidal" else 0, np.uint8)
        right = left.copy()
    else:
        left = rng.integers(0, c["levels"], (pairs, h, w)).astype(np.uint8) * (256 // c["levels"] - (c["levels"] < 256))
        right = rng.integers(0, c["levels"], (pairs, h, w)).astype(np.uint8) * (256 // c["levels"] - (c["levels"] < 256))
    prior = np.stack([make_prior(c["prior"], w, h, c["d"], c["radius"], rng) for _ in range(pairs)])
    prior_right = np.stack([make_prior(c["prior"], w, h, c["d"], c["radius"], rng) for _ in range(pairs)])
    for a in (left, right, prior, prior_right):
        a.setflags(write=False)
    return left, right, prior, prior_right


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> per pair, near_reference.expected of the case (computed once, shared, read-only)"""
    c = BY_NAME[name]
    left, right, prior, prior_right = inputs(name)
    out = []
    for q in range(c["pairs"]):
        e = nr.expected(left[q], right[q], prior[q], prior_right[q], c["d"], c["sw"], c["census"], c["radius"], c["mode"],
                        c["max_diff"])
        for v in e.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(e)
    return out


def stacked(name, key):
    return np.stack([e[key] for e in expected(name)])


# ---------------------------------------------------------------------------
# the definition with one mistake
# ---------------------------------------------------------------------------

LEFT_MUTANTS = ("last_wins", "web_for_shift", "no_clip_hi", "no_clip_lo", "sentinel_best", "ghost_past_border_free",
                "neighbour_d")
MUTANTS = LEFT_MUTANTS + ("mirror_plus",)


def _costs(cl, cr, d, mode, free_past_border=False):
    """Hamming costs of any integer shift d (the no_clip mutants leave 0 .. D - 1)"""
    h, w = cl.shape
    x = np.arange(w) + d
    if mode == "toroidal":
        return np.bitwise_count(cl ^ cr[:, x % w]).astype(np.int64)
    inside = (x >= 0) & (x < w)
    other = np.where(inside[None, :], cr[:, np.clip(x, 0, w - 1)], np.uint64(0))
    c = np.bitwise_count(cl ^ other).astype(np.int64)
    if free_past_border:
        c[:, x >= w] = 0
    return c


def mutant_near(left, right, prior, num_shifts, square_width, census, radius, mode, kind):
    """-> (best, web) of the left search with the mistake `kind` of LEFT_MUTANTS"""
    assert kind in LEFT_MUTANTS
    cl, cr = transform(left, census, mode), transform(right, census, mode)
    n = 2 * (square_width // 2) + 1
    s = np.asarray(prior).astype(np.int64)
    centre = s if kind == "web_for_shift" else s - 1
    lo, hi = centre - radius, centre + radius
    if kind != "no_clip_lo":
        lo = np.maximum(0, lo)
    if kind != "no_clip_hi":
        hi = np.minimum(num_shifts - 1, hi)
    has = (s != 0) & (s >= 1 - radius) & (s <= num_shifts + radius) & (lo <= hi)
    best = np.full(cl.shape, np.iinfo(np.int64).max, np.int64)
    web = np.zeros(cl.shape, np.int32)
    if kind == "neighbour_d":
        # candidate k of every pixel is prior - 1 + k: the cost plane of candidate k takes EVERY pixel's own shift
        for k in range(-radius, radius + 1):
            dk = s - 1 + k
            ok = has & (dk >= lo) & (dk <= hi)
            plane = np.zeros(cl.shape, np.int64)
            for d in np.unique(dk[ok]):
                m = ok & (dk == d)
                plane[m] = _costs(cl, cr, int(d), mode)[m]
            total = _box(plane, n, mode)
            upd = ok & (total < best)
            best[upd] = total[upd]
            web[upd] = (dk + 1)[upd]
    else:
        for d in range(-2 * radius - 1, num_shifts + 2 * radius + 2):
            m = has & (lo <= d) & (d <= hi)
            if not m.any():
                continue
            total = _box(_costs(cl, cr, d, mode, kind == "ghost_past_border_free"), n, mode)
            upd = m & ((total <= best) if kind == "last_wins" else (total < best))
            best[upd] = total[upd]
            web[upd] = d + 1
    best[~has] = 0xffff if kind == "sentinel_best" else 0
    return best.astype(np.int32), web


def mutant_near_right(left, right, prior_right, num_shifts, square_width, census, radius, mode):
    """the right search written out with u + d where the definition has u - d ("mirror_plus")"""
    cl, cr = transform(left, census, mode), transform(right, census, mode)
    n = 2 * (square_width // 2) + 1
    lo, hi, has = nr.candidates(prior_right, num_shifts, radius)
    best = np.full(cl.shape, np.iinfo(np.int64).max, np.int64)
    web = np.zeros(cl.shape, np.int32)
    for d in range(num_shifts):
        m = has & (lo <= d) & (d <= hi)
        if not m.any():
            continue
        total = _box(_costs(cr, cl, d, mode), n, mode)
        upd = m & (total < best)
        best[upd] = total[upd]
        web[upd] = d + 1
    best[~has] = 0
    return best.astype(np.int32), web


# the named case on which each mutant must differ from the definition (tests/test_near_cpu.py)
MUTANT_CASE = {"last_wins": "all tie toroidal", "web_for_shift": "maximum cost", "no_clip_hi": "grid 35",
               "no_clip_lo": "grid 89", "sentinel_best": "grid 47", "ghost_past_border_free": "grid 94",
               "neighbour_d": "noise toroidal c=7", "mirror_plus": "noise ghost c=7"}


# ---------------------------------------------------------------------------
# the scene the feature is for ("what it is for")
# ---------------------------------------------------------------------------

def step_scene(seed, w=96, h=40):
    """-> (left, right, truth web map, half-path prior): shift 9 left of column 48 and 21 from it on, the nearer
    surface painted last; the prior is the even shift below the truth, all the half path can say"""
    rng = np.random.default_rng(seed)
    left = rng.integers(0, 256, (h, w)).astype(np.uint8)
    right = rng.integers(0, 256, (h, w)).astype(np.uint8)
    shift = np.where(np.arange(w) < w // 2, 9, 21)
    for d in (9, 21):                                       # the nearer surface (the larger shift) last
        for x in np.flatnonzero(shift == d):
            if x + d < w:
                right[:, x + d] = left[:, x]
    truth = np.broadcast_to(1 + shift, (h, w)).astype(np.int32)
    prior = np.broadcast_to(2 * (1 + shift // 2) - 1, (h, w)).astype(np.int32)
    return left, right, truth, prior


__all__ = ["CASES", "BY_NAME", "inputs", "expected", "stacked", "MUTANTS", "LEFT_MUTANTS", "MUTANT_CASE", "mutant_near",
           "mutant_near_right", "step_scene", "make_prior", "mirror"]
