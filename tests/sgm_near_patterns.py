"""Inputs for the banded SGM tests (test_sgm_near_cpu.py, test_sgm_near_gpu.py): the named cases the GPU runs, each made
from a seed, with its expected result from the definition (tests/sgm_near_reference.py), computed once; and the
definition with one mistake applied (the "mutants"), which the CPU test shows the cases can tell from the definition.

The data term works on tiles of 64 x 16 pixels with a halo of the window and keeps the wanted shifts of a tile in a
mask of 32-bit words; a path kernel gives a line to 16 lanes, 16 lines to a workgroup, and loads 12 steps ahead.  The
sizes sit around the tile, the workgroup's lines and the prefetch depth (1, 2, 12, 13, 15, 16, 17, 63, 64, 65 columns and
rows, and 129 x 5), the shift counts on every edge of a mask word (1, 4, 31, 33, 64, 130, 512).  The factors are
spread over the cases rather than multiplied out."""
from __future__ import annotations

import functools
import itertools

import numpy as np

from tests import census_extreme_patterns as xp
from tests import sgm_near_reference as sn
from tests.census_reference import mirror, transform
from tests.cost_lr_reference import _box
from tests.near_patterns import I32_MAX, I32_MIN, _costs
from tests.sgm_reference import DIRS

SIZES = [1, 2, 15, 16, 17, 63, 64, 65]
WINDOWS = [1, 3, 9, 25]
SHIFTS = [1, 4, 31, 33, 64, 130, 512]
CENSUS = [3, 5, 7]
RADII = [1, 2, 3, 4]
MODES = ["toroidal", "ghost"]
PRIORS = ["const", "jumps", "noise", "zeros30", "zeros100", "zero_ends", "extremes", "clipped"]
PENALTIES = [(10, 120), (7, 7), (0, 50), (300, 4000), (0, 0), (32767, 32767)]
MAX_PAIRS = 3


def _cases():
    cases = []
    sizes = list(itertools.product(SIZES, SIZES)) + [(129, 5), (13, 12), (12, 13), (13, 13), (5, 129)]
    for k, (w, h) in enumerate(sizes):
        p1, p2 = PENALTIES[k % 6]
        # (a plan takes square_width <= min(W, H): an even one equal to W gives a window n = W + 1 wider than the image)
        cases.append(dict(name=f"grid {k}", kind="random", w=w, h=h, mode=MODES[(k + k // 8) % 2],
                          sw=min(WINDOWS[k % 4], w, h), d=SHIFTS[(k + k // 7) % 7], census=CENSUS[(k + k // 3) % 3],
                          radius=RADII[(k + k // 4) % 4], pairs=(3, 1, 2)[(k // 2) % 3], prior=PRIORS[(k + k // 8) % 8],
                          paths=(8, 4)[(k // 3) % 2], p1=p1, p2=p2, levels=(256, 4)[(k // 5) % 2], max_diff=k % 2,
                          seed=9000 + k))
    # neighbour jumps of exactly 2r - 1 .. 2r + 2 at every radius, both borders, on more than one tile and workgroup
    for i, (mode, radius) in enumerate(itertools.product(MODES, RADII)):
        cases.append(dict(name=f"jumps {mode} r={radius}", kind="random", w=(65, 33)[i % 2], h=(17, 35)[i % 2], mode=mode,
                          sw=(3, 5)[i % 2], d=(64, 40)[i % 2], census=CENSUS[i % 3], radius=radius, pairs=1, prior="jumps",
                          paths=8, p1=(10, 0)[i // 4], p2=120, levels=256, max_diff=1, seed=9200 + i))
    # a tile that wants more than 32 distinct shifts, of every mask word, at every census width
    for i, (mode, census) in enumerate(itertools.product(MODES, CENSUS)):
        cases.append(dict(name=f"noise {mode} c={census}", kind="random", w=129, h=33, mode=mode, sw=(5, 9, 3)[i % 3],
                          d=(512, 130, 64)[i % 3], census=census, radius=(1, 2, 4)[i % 3], pairs=1, prior="noise",
                          paths=(8, 4)[i % 2], p1=20, p2=200, levels=256, max_diff=1, seed=9300 + i))
    # the widest window (a halo of 12 on every side of the tile), more than one tile
    for i, mode in enumerate(MODES):
        cases.append(dict(name=f"window 25 {mode}", kind="random", w=(65, 129)[i], h=33, mode=mode, sw=25, d=(33, 64)[i],
                          census=(3, 5)[i], radius=(2, 3)[i], pairs=(2, 1)[i], prior=("jumps", "zeros30")[i], paths=8,
                          p1=300, p2=4000, levels=256, max_diff=1, seed=9350 + i))
    # K(p) = 0 .. D - 1 at every pixel: sm_sgm_wta's maps
    cases.append(dict(name="whole range const", kind="random", w=70, h=20, mode="toroidal", sw=5, d=9, census=7, radius=4,
                      pairs=1, prior="centre", paths=8, p1=40, p2=300, levels=256, max_diff=1, seed=9400))
    cases.append(dict(name="whole range noise", kind="random", w=65, h=17, mode="ghost", sw=3, d=3, census=5, radius=2,
                      pairs=2, prior="noise1", paths=4, p1=15, p2=90, levels=256, max_diff=0, seed=9401))
    # a constant gray pair: the data term is 0 everywhere, the maps are those of the penalties between the noise bands
    for i, mode in enumerate(MODES):
        cases.append(dict(name=f"all tie {mode}", kind="gray", w=70, h=20, mode=mode, sw=9, d=40, census=7,
                          radius=(2, 4)[i], pairs=1, prior="noise", paths=8, p1=10, p2=120, levels=1, max_diff=0,
                          seed=9410 + i))
    # A = 30000 at the last shift of every pixel (census_extreme_patterns.anti: n = 25, c = 7); a lattice of pixels whose
    # band is that shift alone among neighbours whose bands lie 0 .. r: every direction jumps, L_r = 30000 + 32767 and
    # S = 8 * 62767 there, the bound of the u16 and of the key
    cases.append(dict(name="maximum cost", kind="anti", w=98, h=28, mode="toroidal", sw=25, d=32, census=7, radius=1,
                      pairs=1, prior="lattice", paths=8, p1=32767, p2=32767, levels=256, max_diff=0, seed=9420))
    return cases


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def make_prior(kind, w, h, d, radius, rng):
    """one int32 prior map"""
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "const":
        p = np.full((h, w), rng.integers(1, d + 1))
    elif kind == "centre":
        p = np.full((h, w), radius + 1)
    elif kind == "jumps":
        # blocks of 3 x 2 pixels; every other block column (row) is raised by a jump of 2r - 1 .. 2r + 2 or 0, so that
        # horizontal and vertical neighbours differ by exactly each of them, diagonal ones by their sums as well
        jumps = np.array([0, 2 * radius - 1, 2 * radius, 2 * radius + 1, 2 * radius + 2])
        jx = rng.choice(jumps, w // 3 + 1) * (np.arange(w // 3 + 1) % 2)
        jy = rng.choice(jumps, h // 2 + 1) * (np.arange(h // 2 + 1) % 2)
        p = np.clip(rng.integers(1, max(2, d - 4 * radius - 3)) + jx[xx // 3] + jy[yy // 2], 1, d)
    elif kind == "noise":
        p = rng.integers(0, d + 1, (h, w))
    elif kind == "noise1":
        p = rng.integers(1, d + 1, (h, w))
    elif kind == "zeros30":
        surfaces = rng.integers(1, d + 1, (h // 11 + 1, w // 24 + 1))[yy // 11, xx // 24]
        p = np.where(rng.random((h, w)) < 0.3, 0, surfaces)
    elif kind == "zeros100":
        p = np.zeros((h, w))
    elif kind == "zero_ends":
        # no band at the first and the last pixel of rows, columns and diagonals, and along a whole row and column
        p = rng.integers(1, d + 1, (h // 4 + 1, w // 5 + 1))[yy // 4, xx // 5]
        p[[0, -1], :] = 0
        p[:, [0, -1]] = 0
        p[h // 2, :] = 0
        p[:, w // 3] = 0
    elif kind == "extremes":
        vals = np.array([I32_MIN, I32_MAX, -radius, 1 - radius, d + radius, d + radius + 1, 0, 1, d, -1, I32_MIN + 1,
                         I32_MAX - 1], np.int64)
        p = rng.choice(vals, (h, w))
    elif kind == "clipped":
        # bands clipped at 0 and at D - 1, down to one shift
        vals = np.concatenate([np.arange(1 - radius, 3), np.arange(d - 1, d + radius + 1)])
        p = rng.choice(vals, (h // 2 + 1, w // 3 + 1))[yy // 2, xx // 3]
    elif kind == "lattice":
        p = np.where((xx % 3 == 1) & (yy % 3 == 1), d + radius, 1)
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
        scale = 256 // c["levels"] - (c["levels"] < 256)
        left = rng.integers(0, c["levels"], (pairs, h, w)).astype(np.uint8) * scale
        right = rng.integers(0, c["levels"], (pairs, h, w)).astype(np.uint8) * scale
    prior = np.stack([make_prior(c["prior"], w, h, c["d"], c["radius"], rng) for _ in range(pairs)])
    prior_right = np.stack([make_prior(c["prior"], w, h, c["d"], c["radius"], rng) for _ in range(pairs)])
    for a in (left, right, prior, prior_right):
        a.setflags(write=False)
    return left, right, prior, prior_right


def args(c):
    """the definition's arguments behind the images and priors"""
    return c["d"], c["sw"], c["census"], c["p1"], c["p2"], c["paths"], c["radius"], c["mode"]


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> per pair, sgm_near_reference.expected of the case (computed once, shared, read-only)"""
    c = BY_NAME[name]
    left, right, prior, prior_right = inputs(name)
    out = []
    for q in range(c["pairs"]):
        e = sn.expected(left[q], right[q], prior[q], prior_right[q], *args(c), c["max_diff"])
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

LEFT_MUTANTS = ("missing_zero", "no_restart", "no_delta", "m_clipped", "last_wins", "sub_across_end", "wrap",
                "no_clip_lo", "no_clip_hi")
MUTANTS = LEFT_MUTANTS + ("prior_not_mirrored",)
BIG = sn.BIG


def _mutant_path(a, ink, base, clipped, dx, dy, p1, p2, kind):
    """sgm_near_reference.path with the mistake `kind`.  base: the shift of every pixel's first slot (prior - 1 - r);
    clipped: the pixel's band has slots outside 0 .. D - 1"""
    h, w, D = a.shape
    has = ink.any(axis=-1)
    L = np.full(a.shape, BIG, np.int64)
    dd = np.arange(D)

    def step(av, inkv, lq, ok, bp, bq, clq, ins=True):
        if kind == "no_restart":
            ok = ok | (ins & (lq < BIG).any(axis=1))       # (lq is the last band met along the path)
        m = lq.min(axis=1, keepdims=True)
        if kind == "m_clipped":
            m = np.where((clq & ok)[:, None], np.minimum(m, 0), m)
        if kind == "no_delta":
            idx = dd[None, :] - (bp - bq)[:, None]          # slot k of p reads slot k of q
            lq = np.where((idx >= 0) & (idx < D), np.take_along_axis(lq, np.clip(idx, 0, D - 1), 1), BIG)
        lo = np.full_like(lq, BIG)
        hi = np.full_like(lq, BIG)
        lo[:, 1:] = lq[:, :-1]
        hi[:, :-1] = lq[:, 1:]
        if kind == "missing_zero":
            lq, lo, hi = (np.where(v >= BIG, 0, v) for v in (lq, lo, hi))
        t = np.minimum(np.minimum(lq, np.minimum(lo, hi) + p1), m + p2) - m
        out = np.where(inkv, np.where(ok[:, None], av + t, av), BIG)
        if kind == "no_restart":                            # a pixel without a band hands its predecessor's L on
            out = np.where(inkv.any(axis=1)[:, None], out, lq)
        return out

    def first(av, inkv):
        return np.where(inkv, av, BIG)
    if dy != 0:
        xq = np.arange(w) - dx
        inside = (xq >= 0) & (xq < w)
        xc = xq % w if kind == "wrap" else np.clip(xq, 0, w - 1)
        if kind == "wrap":
            inside = np.ones(w, bool)
        for y in (range(h) if dy > 0 else range(h - 1, -1, -1)):
            yq = y - dy
            if 0 <= yq < h:
                L[y] = step(a[y], ink[y], L[yq][xc], inside & has[yq][xc], base[y], base[yq][xc], clipped[yq][xc],
                            inside)
            elif kind == "wrap":
                yw = yq % h
                L[y] = step(a[y], ink[y], first(a[yw][xc], ink[yw][xc]), has[yw][xc], base[y], base[yw][xc],
                            clipped[yw][xc])
            else:
                L[y] = first(a[y], ink[y])
    else:
        for x in (range(w) if dx > 0 else range(w - 1, -1, -1)):
            xq = x - dx
            if 0 <= xq < w:
                L[:, x] = step(a[:, x], ink[:, x], L[:, xq], has[:, xq], base[:, x], base[:, xq], clipped[:, xq])
            elif kind == "wrap":
                xw = xq % w
                L[:, x] = step(a[:, x], ink[:, x], first(a[:, xw], ink[:, xw]), has[:, xw], base[:, x], base[:, xw],
                               clipped[:, xw])
            else:
                L[:, x] = first(a[:, x], ink[:, x])
    return np.where(ink, np.where(L >= BIG, 0, L), 0)


def mutant_sgm_near(left, right, prior, num_shifts, square_width, census, p1, p2, paths, radius, mode, kind):
    """-> (best, web, sub) of the left pass with the mistake `kind` of LEFT_MUTANTS.  The volumes run over the shifts
    -r .. D - 1 + r (index d + r), so that the bands of the no_clip mutants fit."""
    assert kind in LEFT_MUTANTS
    cl, cr = transform(left, census, mode), transform(right, census, mode)
    n = 2 * (square_width // 2) + 1
    D, r = num_shifts, radius
    s = np.asarray(prior).astype(np.int64)
    lo, hi = s - 1 - r, s - 1 + r
    has = (s != 0) & (s >= 1 - r) & (s <= D + r)
    clipped = has & ((lo < 0) | (hi > D - 1))
    base = np.where(has, lo, 0)
    if kind != "no_clip_lo":
        lo = np.maximum(0, lo)
    if kind != "no_clip_hi":
        hi = np.minimum(D - 1, hi)
    dvals = np.arange(-r, D + r)
    ink = has[..., None] & (lo[..., None] <= dvals) & (dvals <= hi[..., None])
    a = np.zeros(ink.shape, np.int64)
    for k, d in enumerate(dvals):
        m = ink[..., k]
        if m.any():
            a[..., k][m] = _box(_costs(cl, cr, int(d), mode), n, mode)[m]
    S = sum(_mutant_path(a, ink, base, clipped, dx, dy, p1, p2, kind) for dx, dy in DIRS[paths])
    if kind == "last_wins":
        E = S.shape[-1]
        k = E - 1 - np.argmin(np.where(ink, S, BIG)[..., ::-1], axis=-1)
    else:
        k = np.argmin(np.where(ink, S, BIG), axis=-1)
    E = S.shape[-1]

    def at(j):
        return np.take_along_axis(S, np.clip(j, 0, E - 1)[..., None], -1)[..., 0]

    def inside(j):
        if kind == "sub_across_end":                        # sm_sgm_wta's rule: 1 < web < D, whatever the band
            return (j - r >= 0) & (j - r < D)
        return (j >= 0) & (j < E) & np.take_along_axis(ink, np.clip(j, 0, E - 1)[..., None], -1)[..., 0]
    any_ = ink.any(axis=-1)
    best = at(k)
    web = k - r + 1
    aa, bb = at(k - 1) - best, at(k + 1) - best
    den = aa + bb
    ok = any_ & inside(k - 1) & inside(k + 1) & (den > 0)
    q = np.zeros_like(best)
    q[ok] = np.floor_divide(16 * (aa[ok] - bb[ok]) + den[ok], 2 * den[ok])
    sub = 16 * web + np.clip(q, -8, 8)
    return (np.where(any_, best, 0).astype(np.int32), np.where(any_, web, 0).astype(np.int32),
            np.where(any_, sub, 0).astype(np.int16))


def mutant_sgm_near_right(left, right, prior_right, num_shifts, square_width, census, p1, p2, paths, radius, mode):
    """the right pass around the prior as it lies, not mirrored ("prior_not_mirrored")"""
    best, web, _ = sn.sgm_near(mirror(right), mirror(left), np.asarray(prior_right), num_shifts, square_width, census,
                               p1, p2, paths, radius, mode)
    return mirror(best), mirror(web)


# the named case on which each mutant must differ from the definition (tests/test_sgm_near_cpu.py)
MUTANT_CASE = {"missing_zero": "jumps toroidal r=1", "no_restart": "grid 3", "no_delta": "jumps ghost r=2",
               "m_clipped": "grid 7", "last_wins": "all tie toroidal", "sub_across_end": "grid 7",
               "wrap": "grid 3", "no_clip_lo": "grid 7", "no_clip_hi": "grid 7", "prior_not_mirrored": "grid 9"}


# ---------------------------------------------------------------------------
# the scene the feature is for ("what it is for")
# ---------------------------------------------------------------------------

def band_scene(seed, w=96, h=40):
    """-> (left, right, truth web map, half-path prior, region): near_patterns.step_scene's depth step (shift 9 left of
    column 48, 21 from it on, the nearer surface painted last) with a textureless band, rows 14 .. 25, across it: the
    left image is one gray there, and so is what the right image shows of it.  The prior is the even shift below the
    truth; region is the band's pixels whose match lies inside the right image."""
    rng = np.random.default_rng(seed)
    left = rng.integers(0, 256, (h, w)).astype(np.uint8)
    right = rng.integers(0, 256, (h, w)).astype(np.uint8)
    left[14:26, :] = 128
    shift = np.where(np.arange(w) < w // 2, 9, 21)
    for d in (9, 21):                                       # the nearer surface (the larger shift) last
        for x in np.flatnonzero(shift == d):
            if x + d < w:
                right[:, x + d] = left[:, x]
    truth = np.broadcast_to(1 + shift, (h, w)).astype(np.int32)
    prior = np.broadcast_to(2 * (1 + shift // 2) - 1, (h, w)).astype(np.int32)
    region = np.zeros((h, w), bool)
    region[14:26, :] = (np.arange(w) + shift < w)[None, :]
    return left, right, truth, prior, region


__all__ = ["CASES", "BY_NAME", "inputs", "expected", "stacked", "args", "MUTANTS", "LEFT_MUTANTS", "MUTANT_CASE",
           "mutant_sgm_near", "mutant_sgm_near_right", "band_scene", "make_prior", "mirror", "MAX_PAIRS"]
