"""Gray images whose edge decisions sit next to a tie, and the exact arithmetic that says where the ties are.
Checker only: imported by tests/, never by the product package.

An edge decision of src/stereo.c:16-70 compares the means of two three-pixel sides of a 3 x 3 neighbourhood,

    |ma - mb| > clamp(T * (ma + mb) / 2, 0, 1),     m = (p0/256 + p1/256 + p2/256) / 3.0   (doubles),

so for in-image pixels it depends only on the two integer side sums (Sa, Sb) in [0, 765].  The edge kernels of
csrc/sm_edges.hip decide it with an f32 prefilter,

    F = fma(Sa + Sb, -(float)(T / 2), |Sa - Sb|)     (one rounding to f32),

and ask the per-threshold tables only where |F| <= 2^-12 (SM_EDGE_MARGIN).  This module

  * computes that band exactly (band_pairs): integer / Fraction arithmetic, no float64 step that can round twice;
  * restates the double decision in numpy (decision_table, find_all_edges), from src/stereo.c, not from
    oracle/stereo_oracle.c;
  * builds 3 x 3 blocks in which one orientation has a chosen (Sa, Sb) and the other three are clearly not edges,
    so that the chosen pair decides the centre pixel (block), places them on a lattice of spacing 3 (build_image)
    and reports which targets and which kernel positions the images reach (coverage).

Orientations, in the kernels' order (v[row][col], row 0 = y - 1, col 0 = x - 1):
    0 left | right            1 top | bottom            2 up-left | down-right            3 down-left | up-right
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

MARGIN = Fraction(1, 4096)                      # SM_EDGE_MARGIN, 2^-12
HALO = 32768                                    # ghost halo 128.0 in units of 1/256
SUMS = 766                                      # in-image side sums 0 .. 765

# the six pixels of each orientation's two sides, as (row, col) of the 3 x 3 neighbourhood
SIDES = (
    (((0, 0), (1, 0), (2, 0)), ((0, 2), (1, 2), (2, 2))),
    (((0, 0), (0, 1), (0, 2)), ((2, 0), (2, 1), (2, 2))),
    (((0, 0), (0, 1), (1, 0)), ((1, 2), (2, 1), (2, 2))),
    (((2, 0), (2, 1), (1, 0)), ((0, 1), (0, 2), (1, 2))),
)
ORIENTATION_NAMES = ("left|right", "top|bottom", "upleft|downright", "downleft|upright")
NEIGHBOURS = tuple((r, c) for r in range(3) for c in range(3) if (r, c) != (1, 1))

# the thresholds the GPU tests run (test_edge_ties_gpu.py).  The last three are the thresholds of the form 2d/k
# (k <= 1530) with the most pairs whose f32 sign alone is wrong, found by tie_richest_thresholds() and written
# here as literals; test_edge_ties_cpu.py checks that they still are.
NAMED_THRESHOLDS = (0.0, 1e-9, 0.02, 0.05, 0.075, 0.1, 0.15, 0.25, 1.0 / 3.0, 0.5, 2.0 / 3.0, 0.75, 1.0)
TIE_RICHEST = (0.4, 0.2857142857142857, 0.2222222222222222)
GPU_THRESHOLDS = NAMED_THRESHOLDS + TIE_RICHEST


# ---------------------------------------------------------------------------
# exact arithmetic of the f32 prefilter
# ---------------------------------------------------------------------------

def f32_half_threshold(t):
    """(float)(T * 0.5) as the host computes it (edge_neg_t: T * 0.5 is exact in double, one rounding to f32)"""
    return float(np.float32(float(t) * 0.5))


def round_f32(x: Fraction) -> Fraction:
    """x rounded to the nearest f32 (ties to even), exactly; no overflow handling (|x| < 2^11 here)"""
    if x == 0:
        return Fraction(0)
    sign = -1 if x < 0 else 1
    x = abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()       # 2^e <= x < 2^(e+2)
    if Fraction(2) ** e > x:
        e -= 1
    if Fraction(2) ** (e + 1) <= x:
        e += 1
    ulp = Fraction(2) ** (max(e, -126) - 23)                            # denormals below 2^-126
    q, r = divmod(x, ulp)
    if r * 2 > ulp or (r * 2 == ulp and q % 2 == 1):
        q += 1
    return sign * q * ulp


def prefilter_exact(sa, sb, t) -> Fraction:
    """F of the kernels for one pair, exactly: the fma's single rounding of |sa - sb| - (sa + sb) * (float)(T/2)"""
    return round_f32(abs(int(sa) - int(sb)) - (int(sa) + int(sb)) * Fraction(f32_half_threshold(t)))


def _grid():
    sa, sb = np.meshgrid(np.arange(SUMS, dtype=np.int64), np.arange(SUMS, dtype=np.int64), indexing="ij")
    return sa, sb


def band_pairs(t):
    """-> (band, wrong): the in-image pairs (sa, sb) with |F| <= 2^-12, and those of them where the f32 sign alone
    (edge iff F > 0) disagrees with the double decision, as sorted lists of tuples.  F == 0 counts as "no edge":
    at T = 1 the exact ties have F == 0 and the double decision says edge for about a third of them.

    Exactness: with Tf = (float)(T/2) (24-bit mantissa) and s = sa + sb < 2^11, s * Tf has at most 35 significant
    bits and is exact in float64; G = |d| - s * Tf then rounds once, |G| < 2^10, so |G - X| <= 2^-43 where X is the
    exact value the fma rounds.  Every pair with |G| <= 2^-11 is settled with Fraction arithmetic (round_f32 of X);
    every other pair has |X| > 2^-11 - 2^-43, so |F| > 2^-12 and sign(F) = sign(X) = sign(G)."""
    sa, sb = _grid()
    tf = f32_half_threshold(t)
    g = np.abs(sa - sb).astype(np.float64) - (sa + sb).astype(np.float64) * tf
    dec = decision_table(t).astype(bool)
    cand = np.abs(g) <= 2.0 ** -11
    band, wrong = [], []
    for a, b in zip(*np.nonzero(cand)):
        f = prefilter_exact(a, b, t)
        if abs(f) <= MARGIN:
            band.append((int(a), int(b)))
            if (f > 0) != dec[a, b]:
                wrong.append((int(a), int(b)))
    # outside the candidates the sign of G is the sign of F: a wrong sign there would break the kernels' margin
    outside_wrong = ~cand & ((g > 0) != dec)
    if outside_wrong.any():
        a, b = np.argwhere(outside_wrong)[0]
        raise AssertionError(f"T={t!r}: pair ({a}, {b}) outside the band has the wrong f32 sign")
    return band, wrong


def outside_band_sign_errors(t):
    """pairs with |F| > 2^-12 whose f32 sign disagrees with the double decision (the margin argument: none)"""
    try:
        band_pairs(t)
    except AssertionError as e:
        return [str(e)]
    return []


def break_points(t):
    """per sa, the pairs on each side of every switch of the double decision along sb (the table's lo / hi):
    a sorted list of (sa, sb)"""
    dec = decision_table(t).astype(np.int8)
    out = set()
    for a in range(SUMS):
        for b in np.nonzero(np.diff(dec[a]))[0]:
            out.add((a, int(b)))
            out.add((a, int(b) + 1))
    return sorted(out)


def exact_ties(p, q):
    """pairs (sa, sb) != (0, 0) with |sa - sb| / (sa + sb) = p / q exactly (p / q reduced): sa + sb = m q,
    |sa - sb| = m p, sa = m (q + p) / 2 an integer <= 765 -- two pairs per such m"""
    return sum(2 for m in range(1, 2 * 765 // (q + p) + 1) if (m * (q + p)) % 2 == 0 and m * (q + p) // 2 <= 765)


def tie_richest_thresholds(count, kmax=1530):
    """thresholds T = 2d/k (k <= kmax, 0 < T <= 1, d/k reduced) with the most exact ties |sa - sb| = (T/2)(sa + sb)
    among in-image pairs, richest first (then smallest k): [(T, ties)]"""
    from math import gcd
    out = []
    for k in range(1, kmax + 1):
        for d in range(1, k // 2 + 1):
            if gcd(d, k) == 1:
                n = exact_ties(d, k)
                if n:
                    out.append((-n, k, 2.0 * d / k))
    out.sort()
    return [(t, -n) for n, _, t in out[:count]]


def most_wrong_thresholds(count, pool=40):
    """of the `pool` tie-richest thresholds, the `count` with the most pairs whose f32 sign alone is wrong (then
    the largest band): [(T, wrong, band)]"""
    scored = []
    for t, _ in tie_richest_thresholds(pool):
        band, wrong = band_pairs(t)
        scored.append((-len(wrong), -len(band), t))
    scored.sort()
    return [(t, -w, -b) for w, b, t in scored[:count]]


def worst_rounding_thresholds(count, samples=200000, seed=5):
    """thresholds in (0, 1] whose (float)(T/2) is furthest from T/2 relative to one f32 ulp: a log-uniform sample
    scored by |Tf - T/2| / ulp(Tf) (at most 1/2), best first"""
    rng = np.random.default_rng(seed)
    t = np.concatenate([rng.random(samples), 10.0 ** rng.uniform(-9, 0, samples)])
    h = t * 0.5
    hf = h.astype(np.float32).astype(np.float64)
    ulp = np.spacing(np.abs(h).astype(np.float32)).astype(np.float64)
    score = np.abs(hf - h) / ulp
    order = np.argsort(-score, kind="stable")
    return [float(v) for v in t[order[:count]]]


# ---------------------------------------------------------------------------
# the double decision, restated from src/stereo.c:16-70
# ---------------------------------------------------------------------------

def _decide_means(avg_left, avg_right, t):
    overall = (avg_left + avg_right) / 2.0
    limit = np.clip(float(t) * overall, 0.0, 1.0)
    return np.abs(avg_left - avg_right) > limit


def decision_table(t):
    """766 x 766 u8: the double decision for in-image side sums (sa, sb), evaluated as the C source does --
    brightness k / 256.0, three brightnesses added and divided by 3.0 (a sum of three k/256 is exact, so the side
    mean is (S / 256.0) / 3.0)"""
    s = np.arange(SUMS, dtype=np.float64) / 256.0
    avg = s / 3.0
    return _decide_means(avg[:, None], avg[None, :], t).astype(np.uint8)


def find_all_edges(gray, t, mode="toroidal"):
    """u8 {0, 1} edge image of a u8 gray image, src/stereo.c:16-80 (toroidal) or src/stereo-ghost.c (the 128.0
    halo), in numpy doubles"""
    g = np.asarray(gray, np.float64) / 256.0
    h, w = g.shape
    if mode == "toroidal":
        p = np.pad(g, 1, mode="wrap")
    else:
        p = np.pad(g, 1, mode="constant", constant_values=128.0)

    def px(r, c):
        return p[r:r + h, c:c + w]
    out = np.zeros((h, w), bool)
    for side_a, side_b in SIDES:
        a = (px(*side_a[0]) + px(*side_a[1]) + px(*side_a[2])) / 3.0
        b = (px(*side_b[0]) + px(*side_b[1]) + px(*side_b[2])) / 3.0
        out |= _decide_means(a, b, t)
    return out.astype(np.uint8)


def side_sums(block):
    """(sa[4], sb[4]) integer side sums of a 3 x 3 block"""
    b = np.asarray(block, np.int64)
    return ([int(sum(b[r, c] for r, c in sa)) for sa, _ in SIDES],
            [int(sum(b[r, c] for r, c in sb)) for _, sb in SIDES])


# ---------------------------------------------------------------------------
# blocks: one orientation at (sa, sb), the other three clearly not edges
# ---------------------------------------------------------------------------

def tiny_threshold(t):
    """no non-edge pair can be outside the band: 1530 * (float)(T/2) <= 2^-12 (T = 0, T = 1e-9, ...)"""
    return 1530 * Fraction(f32_half_threshold(t)) <= MARGIN


def _others_ok(blocks, o, t, dec, tf):
    """vectorised over candidate blocks (N x 3 x 3 int): the three other orientations decide 0 and, unless the
    threshold is tiny, are outside the band (F < -margin, with float64 slack far above its 2^-43 error)"""
    ok = np.ones(len(blocks), bool)
    tiny = tiny_threshold(t)
    for k, (sa, sb) in enumerate(SIDES):
        if k == o:
            continue
        a = sum(blocks[:, r, c] for r, c in sa)
        b = sum(blocks[:, r, c] for r, c in sb)
        if tiny:
            ok &= a == b
        else:
            g = np.abs(a - b) - (a + b) * tf
            ok &= (dec[a, b] == 0) & (g < -2.0 ** -11)
    return ok


def _fill_side(rng, total, n):
    """n random triples in [0, 255] summing to `total` (N x 3), or fewer where rejection thins them"""
    lo = max(0, total - 510)
    hi = min(255, total)
    a0 = rng.integers(lo, hi + 1, n)
    rest = total - a0
    lo1 = np.maximum(0, rest - 255)
    hi1 = np.minimum(255, rest)
    a1 = lo1 + (rng.random(n) * (hi1 - lo1 + 1)).astype(np.int64)
    a2 = rest - a1
    perm = rng.permuted(np.stack([a0, a1, a2], 1), axis=1)
    return perm


def _tie_blocks(o, sa, sb, free=255, step=1):
    """every block of the exact-tie family of orientation o (0 or 2) at (sa, sb): the other three orientations
    have A == B.  Left | right: with d = sa - sb, left column (b2 + d, b1 - d, b0 + d) against right column
    (b0, b1, b2), middle column (f, ., f).  Up-left | down-right: v22 = v00 + d, v20 = v02 = f, v12 - v21 =
    v10 - v01.  -> N x 3 x 3 int64 (N may be 0)"""
    d = sa - sb
    x, y = np.meshgrid(np.arange(0, 256, step), np.arange(0, 256, step), indexing="ij")
    x, y = x.ravel(), y.ravel()
    v = np.zeros((x.size, 3, 3), np.int64)
    if o == 0:
        b0, b1 = x, y
        b2 = sb - b0 - b1
        v[:, 0, 2], v[:, 1, 2], v[:, 2, 2] = b0, b1, b2
        v[:, 0, 0], v[:, 1, 0], v[:, 2, 0] = b2 + d, b1 - d, b0 + d
        v[:, 0, 1] = v[:, 2, 1] = free
    else:
        v00, v01 = x, y
        v10 = sa - v00 - v01
        e = v10 - v01
        v[:, 0, 0], v[:, 0, 1], v[:, 1, 0] = v00, v01, v10
        v[:, 2, 2] = v00 + d
        v[:, 1, 2] = (2 * sb - sa - v00 + e) // 2
        v[:, 2, 1] = (2 * sb - sa - v00 - e) // 2
        v[:, 0, 2] = v[:, 2, 0] = free
    ok = ((v >= 0) & (v <= 255)).all(axis=(1, 2))
    return v[ok]


def _transform(blk, o):
    """a block built for orientation o & 2 (0 or 2) turned into one for o: top | bottom is the transpose of left |
    right, down-left | up-right the vertical mirror of up-left | down-right (the other orientations map onto each
    other, sides at most swapped, and the decision is symmetric in its sides)"""
    if o == 1:
        return blk.transpose(0, 2, 1) if blk.ndim == 3 else blk.T
    if o == 3:
        return blk[..., ::-1, :]
    return blk


def block(o, sa, sb, t, tries=(1024, 16384, 131072), seed=0):
    """a 3 x 3 u8 block whose orientation o has side sums (sa, sb) and whose other orientations decide 0 -- outside
    the band (F < -2^-12) unless the threshold is tiny (tiny_threshold), where they tie exactly -- or None if none
    was found.  The centre is 0 (unused by its own decision).  Deterministic: the exact-tie family first, then a
    seeded random search over all eight neighbours."""
    if not (0 <= sa < SUMS and 0 <= sb < SUMS):
        return None
    dec = decision_table_cached(t)
    tf = f32_half_threshold(t)
    base = o & 2
    side_a, side_b = SIDES[o]
    free = [p for p in NEIGHBOURS if p not in side_a and p not in side_b]
    rng = np.random.default_rng([seed, o, sa, sb])

    def ties(step):
        v = _tie_blocks(base, sa, sb, step=step)
        if len(v):
            v = _transform(v, o)
            ok = _others_ok(v, o, t, dec, tf)
            if ok.any():
                # of the valid ones, the block whose tied sums are largest (furthest outside the band)
                return v[np.argmax(ok * (1 + v.sum(axis=(1, 2))))].astype(np.uint8)
        return None

    def search(n):
        if tiny_threshold(t):
            return None
        cand = np.zeros((n, 3, 3), np.int64)
        ta, tb = _fill_side(rng, sa, n), _fill_side(rng, sb, n)
        for i, (r, c) in enumerate(side_a):
            cand[:, r, c] = ta[:, i]
        for i, (r, c) in enumerate(side_b):
            cand[:, r, c] = tb[:, i]
        for r, c in free:
            cand[:, r, c] = np.where(rng.random(n) < 0.5, 255, rng.integers(0, 256, n))
        ok = _others_ok(cand, o, t, dec, tf)
        return cand[np.argmax(ok)].astype(np.uint8) if ok.any() else None

    # a coarse grid of the tie family, a small random search, then all of the family and larger searches
    for step in (lambda: ties(5), lambda: search(tries[0]), lambda: ties(1),
                 *(lambda n=n: search(n) for n in tries[1:])):
        b = step()
        if b is not None:
            return b
    return None


_dec_cache: dict = {}
_band_cache: dict = {}


def band_pairs_cached(t):
    key = float(t)
    if key not in _band_cache:
        _band_cache[key] = band_pairs(key)
    return _band_cache[key]


def decision_table_cached(t):
    key = float(t)
    if key not in _dec_cache:
        _dec_cache[key] = decision_table(key)
    return _dec_cache[key]


_block_cache: dict = {}


def targets(t):
    """(band, wrong, blocks, unrealised) of a threshold: blocks maps every (o, sa, sb) of the band, o = 0..3, to its
    3 x 3 block; unrealised lists the targets block() found none for (reported, never dropped silently)"""
    key = float(t)
    if key not in _block_cache:
        band, wrong = band_pairs_cached(key)
        blocks, unrealised = {}, []
        for o in range(4):
            for sa, sb in band:
                b = block(o, sa, sb, key)
                if b is None:
                    unrealised.append((o, sa, sb))
                else:
                    blocks[(o, sa, sb)] = b
        _block_cache[key] = (band, wrong, blocks, unrealised)
    return _block_cache[key]


# ---------------------------------------------------------------------------
# images: blocks on a lattice of spacing 3
# ---------------------------------------------------------------------------

def lattice_offsets(n, mode):
    """per axis of length n: lattice offsets whose centres, together, reach every position a block fits at --
    toroidal: every position (blocks wrap round the edge), ghost: 1 .. n - 2 (no halo in a block)"""
    if n < 3:
        return []
    if mode == "ghost":
        return [o for o in (1, 2, 3) if o <= n - 2]
    offs, seen = [], set()
    for o in (0, 1, 2, n - 1, n - 2):
        c = lattice_centres(n, o % n, mode)
        if not set(c) <= seen:
            offs.append(o % n)
            seen |= set(c)
    return offs


def lattice_centres(n, off, mode):
    """block centres along one axis for one offset: ghost off, off + 3, ... <= n - 2; toroidal (off + 3i) mod n for
    i < n // 3 (a run of 3 * (n // 3) <= n cells, so no two blocks overlap, and one may straddle the edge)"""
    if mode == "ghost":
        return list(range(off, n - 1, 3))
    return [(off + 3 * i) % n for i in range(n // 3)]


def build_image(w, h, mode, off_x, off_y, blocks, fill_seed):
    """one h x w u8 image: `blocks` (N x 3 x 3, used in order, at most one per lattice point) on the lattice of
    offsets (off_x, off_y), row-major; pixels no block covers are seeded random.  -> (image, centres (K x 2, x y))"""
    img = np.random.default_rng(fill_seed).integers(0, 256, (h, w)).astype(np.uint8)
    xs, ys = lattice_centres(w, off_x, mode), lattice_centres(h, off_y, mode)
    cy, cx = np.meshgrid(np.array(ys, np.int64), np.array(xs, np.int64), indexing="ij")
    cx, cy = cx.ravel(), cy.ravel()
    k = min(len(cx), len(blocks))
    cx, cy = cx[:k], cy[:k]
    d = np.array([-1, 0, 1])
    rows = (cy[:, None] + d) % h
    cols = (cx[:, None] + d) % w
    img[rows[:, :, None], cols[:, None, :]] = blocks[:k]
    return img, np.stack([cx, cy], 1)


def batch(w, h, mode, t, variants=2):
    """the images of one geometry at one threshold: per variant and lattice offset pair, a left and a right image
    (different blocks).  The band targets are laid out in a cycle, each image continuing where the last one
    stopped (and each variant a prime step further), so that every target lands on many positions.
    -> (left, right): pairs x h x w u8 arrays"""
    _, _, blocks, _ = targets(t)
    keys = sorted(blocks)
    arr = np.stack([blocks[k] for k in keys]) if keys else np.zeros((0, 3, 3), np.uint8)
    lefts, rights = [], []
    pos = 0
    for variant in range(variants):
        for oy in lattice_offsets(h, mode) or [0]:
            for ox in lattice_offsets(w, mode) or [0]:
                imgs = []
                for side in range(2):
                    n = len(lattice_centres(w, ox, mode)) * len(lattice_centres(h, oy, mode))
                    idx = (pos + np.arange(n)) % max(1, len(arr))
                    seed = [int(1e6 * t) % 1000003, w, h, ox, oy, variant, side]
                    img, cs = build_image(w, h, mode, ox, oy, arr[idx] if len(arr) else arr, seed)
                    pos += n + 37
                    imgs.append(img)
                lefts.append(imgs[0])
                rights.append(imgs[1])
    return np.stack(lefts), np.stack(rights)


# ---------------------------------------------------------------------------
# coverage: which targets decide a centre, and at which kernel positions
# ---------------------------------------------------------------------------

def orientation_sums(img, mode):
    """(A, B): 4 x h x w integer side sums per pixel (wrapped, or with the ghost halo 32768)"""
    g = np.asarray(img, np.int64)
    h, w = g.shape
    p = np.pad(g, 1, mode="wrap") if mode == "toroidal" else np.pad(g, 1, constant_values=HALO)
    A = np.stack([sum(p[r:r + h, c:c + w] for r, c in sa) for sa, _ in SIDES])
    B = np.stack([sum(p[r:r + h, c:c + w] for r, c in sb) for _, sb in SIDES])
    return A, B


def deciding_centres(img, mode, t):
    """pixels decided by one near-tie pair: (x, y, o, sa, sb) where orientation o's pair is in the band and the
    other three decide 0 outside the band (or tie exactly, at a tiny threshold).  Ghost: interior pixels only."""
    band, _ = band_pairs_cached(t)
    in_band = np.zeros((SUMS, SUMS), bool)
    for a, b in band:
        in_band[a, b] = True
    dec = decision_table_cached(t)
    tf = f32_half_threshold(t)
    tiny = tiny_threshold(t)
    A, B = orientation_sums(img, mode)
    h, w = A.shape[1:]
    ok_px = np.ones((h, w), bool)
    if mode == "ghost":
        ok_px[:] = False
        ok_px[1:-1, 1:-1] = True
    Ac, Bc = np.minimum(A, SUMS - 1), np.minimum(B, SUMS - 1)
    if tiny:
        quiet = A == B
    else:
        quiet = (dec[Ac, Bc] == 0) & (np.abs(A - B) - (A + B) * tf < -2.0 ** -11)
    out = []
    for o in range(4):
        others = np.ones((h, w), bool)
        for k in range(4):
            if k != o:
                others &= quiet[k]
        sel = ok_px & others & in_band[Ac[o], Bc[o]] & (A[o] < SUMS) & (B[o] < SUMS)
        y, x = np.nonzero(sel)
        out.append(np.stack([x, y, np.full_like(x, o), A[o, y, x], B[o, y, x]], 1))
    return np.concatenate(out) if out else np.zeros((0, 5), np.int64)


def edge_words_r(w, d, sw, pad_l=32):
    """the host's g.edge_words_r (csrc/sm_match.hip, tiled kernels): ext words the right image's edges fill"""
    return (pad_l + w + sw // 2 + d - 2) // 32 + 1


def edges4_stacked(w, d, sw, pad_l=32):
    """sm_find_edges' choice of block shape for k_edges_ext4 (the rule restated in edges4_read_columns of
    test_hip_gpu.py, on the edge words the launch covers): stacked when side by side rounds a row up by > 3 %"""
    lanes = edge_words_r(w, d, sw, pad_l) * 8
    return (lanes + 255) // 256 * 256 > lanes + lanes // 32


def position_classes(x, y, w, h, mode, kernel, half, pad_l=32, stacked=False, rows4=4):
    """the kernel positions pixel (x, y) stands at.  kernel: "ext4" (k_edges_ext4) or "ext" (k_edges_ext)"""
    xe, ye = x + pad_l, y + half
    out = set()
    if kernel == "ext4":
        out.add(f"quad{xe % 4}")
        out.add(f"row{ye % rows4}")
        if xe % 256 < 4:
            out.add("lane0")
        if xe % 256 >= 252:
            out.add("lane63")
        if stacked:
            if (ye // rows4) % 4 in (1, 2, 3) and ye % rows4 == 0 or (ye // rows4) % 4 in (0, 1, 2) and ye % rows4 == rows4 - 1:
                out.add("wave_seam")
        elif xe >= 1024 and xe % 1024 < 4 or xe % 1024 >= 1020 and xe // 1024 < (w + pad_l) // 1024:
            out.add("workgroup_seam")
        if mode == "ghost":
            x0 = xe // 256 * 256 - pad_l
            y0 = (ye // rows4) * rows4 - half
            inside = x0 >= 1 and x0 + 256 <= w - 1 and y0 >= 1 and y0 + rows4 - 1 <= h - 2
            out.add("interior_wave" if inside else "sel_wave")
    else:
        out.add(f"bit{xe % 2}")
        if xe % 64 == 0:
            out.add("lane0")
        if xe % 64 == 63:
            out.add("lane63")
        if ye % 32 in (0, 31):
            out.add("strip_edge")
        if xe >= 256 and xe % 256 in (0, 255):
            out.add("workgroup_seam")
    if mode == "ghost":
        if x in (1, w - 2) or y in (1, h - 2):
            out.add("next_to_border")
    else:
        if x in (0, w - 1):
            out.add("wrap_x")
        if y in (0, h - 1):
            out.add("wrap_y")
    return out


def coverage(lefts, rights, mode, t, kernel, half, pad_l=32, stacked=False):
    """-> (targets, positions, where): the (o, sa, sb) that decide some centre of the batch, the position classes
    of all deciding centres, and for each target one (image, side, x, y) it decides (for failure reports)"""
    where, pixels = {}, set()
    h, w = lefts.shape[1:]
    for i in range(len(lefts)):
        for side, img in ((0, lefts[i]), (1, rights[i])):
            c = deciding_centres(img, mode, t)
            first = np.unique(c[:, 2:], axis=0, return_index=True)[1]
            for x, y, o, a, b in c[first].tolist():
                where.setdefault((o, a, b), (i, side, x, y))
            pixels |= set(map(tuple, np.unique(c[:, :2], axis=0).tolist()))
    pos = set()
    for x, y in pixels:
        pos |= position_classes(x, y, w, h, mode, kernel, half, pad_l, stacked)
    return set(where), pos, where


def reachable_classes(w, h, mode, kernel, half, pad_l=32, stacked=False):
    """the position classes any block centre of the geometry can stand at (what coverage must reach)"""
    out = set()
    xs = sorted({c for o in lattice_offsets(w, mode) for c in lattice_centres(w, o, mode)})
    ys = sorted({c for o in lattice_offsets(h, mode) for c in lattice_centres(h, o, mode)})
    for y in ys:
        for x in xs:
            out |= position_classes(x, y, w, h, mode, kernel, half, pad_l, stacked)
    return out


# ---------------------------------------------------------------------------
# the geometries of test_edge_ties_gpu.py: (name, w, h, D, square_width, kernel, shape, options, unaligned)
#   kernel "ext4" (k_edges_ext4; shape "stacked" / "side" as sm_find_edges picks it) or "ext" (k_edges_ext)
# ---------------------------------------------------------------------------
GEOMETRIES = (
    ("ext4_260_stacked", 260, 37, 16, 5, "ext4", "stacked", None, False),      # one ext row: 80 lanes
    ("ext4_252_stacked", 252, 21, 16, 5, "ext4", "stacked", None, False),
    ("ext4_960_side", 960, 18, 30, 5, "ext4", "side", None, False),            # 256 lanes: one workgroup
    ("ext4_1992_side", 1992, 13, 16, 5, "ext4", "side", None, False),          # 512 lanes: seam at xe = 1024
    ("ext4_1028_stacked", 1028, 9, 16, 5, "ext4", "stacked", None, False),
    ("ext4_8_narrow", 8, 10, 64, 5, "ext4", "stacked", None, False),           # w < pad_l: pos_mod fallback
    ("ext4_4x1", 4, 1, 16, 1, "ext4", "stacked", None, False),
    ("ext4_4x3", 4, 3, 16, 3, "ext4", "stacked", None, False),
    ("ext4_8x2", 8, 2, 16, 1, "ext4", "stacked", None, False),
    ("ext4_8x3", 8, 3, 16, 3, "ext4", "stacked", None, False),
    ("ext_258", 258, 35, 16, 5, "ext", None, None, False),                     # w % 4 != 0
    ("ext_option_260", 260, 37, 16, 5, "ext", None, {"edge_kernel": 1}, False),
    ("ext_unaligned_256", 256, 34, 16, 5, "ext", None, None, True),            # base pointer not 4-byte aligned
)
