"""Inputs for the post-filter tests (test_filter_cpu.py, test_filter_gpu.py): random maps with a chosen share of
invalid pixels, and component shapes that stress a tiled connected-component labelling.  Each structured pattern is
(map, max_size, max_diff); informative() asserts, from the definition alone, that the speckle filter both removes and
keeps a component of it and that a kept component spans more than one tile, so that neither an all-zero nor an
identity output can pass."""
import numpy as np

from tests import filter_reference as fr

TILE_W, TILE_H = 64, 16            # the kernels' tile (sm_filter.hip: FLT_TW, FLT_TH)


def random_map(w, h, dtype, seed, invalid=0.3, lo=1, hi=6, negative=False):
    rng = np.random.default_rng(seed)
    a = rng.integers(lo, hi + 1, (h, w))
    if negative:
        a = np.where(rng.random((h, w)) < 0.4, -a, a)
    a[rng.random((h, w)) < invalid] = 0
    return a.astype(dtype)


def whole(w, h, dtype):
    """one component over the whole map, but for a few 3 x 3 holes with a lone pixel of another value inside"""
    a = np.full((h, w), 7, dtype)
    for y, x in ((1, 1), (h // 2, w // 2), (h - 2, w - 2), (TILE_H, TILE_W), (h // 3, 2 * w // 3)):
        y, x = min(max(y, 1), h - 2), min(max(x, 1), w - 2)
        a[y - 1:y + 2, x - 1:x + 2] = 0
        a[y, x] = 9
    return a, 5, 0


def serpentine(w, h, dtype):
    """a one-pixel path: every even row, joined at alternating ends; lone pixels of a far value in the odd rows"""
    a = np.zeros((h, w), dtype)
    a[0::2] = 7
    for y in range(1, h - 1, 2):
        a[y, 5:w - 5:5] = 1000
        a[y, w - 1 if (y // 2) % 2 == 0 else 0] = 7
    return a, 3, 1


def spiral(w, h, dtype):
    """a rectangular spiral, one pixel wide with one-pixel gaps: ring i (inset 2 i) is cut open on its top row next to
    the bridge that leads down to ring i + 1; plus lone pixels far in value in the outermost gap"""
    a = np.zeros((h, w), dtype)
    i = 0
    while w - 4 * i >= 8 and h - 4 * i >= 8:
        o, x1, y1 = 2 * i, w - 1 - 2 * i, h - 1 - 2 * i
        a[o, o:x1 + 1] = 5
        a[y1, o:x1 + 1] = 5
        a[o:y1 + 1, o] = 5
        a[o:y1 + 1, x1] = 5
        if w - 4 * (i + 1) >= 8 and h - 4 * (i + 1) >= 8:
            a[o + 1, o + 2] = 5                 # bridge to the next ring's corner
            a[o, o + 3] = 0                     # ... and the cut beside it
        i += 1
    a[1, 12:w - 12:7] = 300
    return a, 4, 0


def checkerboard(w, h, dtype):
    """valid / invalid alternating (every valid pixel a component of its own) beside a solid band"""
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.where((xx + yy) % 2 == 0, 3, 0)
    a[:, 3 * w // 4:] = 3
    a[:, 3 * w // 4 - 1] = 0
    return a.astype(dtype), 1, 0


def rings(w, h, dtype, max_diff=2):
    """solid concentric rings, three pixels thick, whose values step by max_diff (joined) and max_diff + 1 (not) in
    turn, from the centre outwards: pairs of rings form the components"""
    yy, xx = np.mgrid[0:h, 0:w]
    inset = np.minimum(np.minimum(xx, w - 1 - xx), np.minimum(yy, h - 1 - yy)) // 3
    n = int(inset.max()) + 1
    steps = np.array([max_diff if j % 2 == 0 else max_diff + 1 for j in range(n)])
    values = 10 + np.concatenate([[0], np.cumsum(steps)[:-1]])
    a = values[inset]
    # the innermost components are the small ones
    roots, sizes = fr.components(a, max_diff)
    by_size = sorted(sizes.values())
    return a.astype(dtype), by_size[len(by_size) // 2], max_diff


def exact_sizes(w, h, dtype, max_size=40):
    """components of exactly max_size and max_size + 1 pixels, as lines and as blocks, laid across tile corners"""
    a = np.zeros((h, w), dtype)
    y, x = TILE_H - 2, TILE_W - 20
    a[y, x:x + max_size] = 4                                        # a line of max_size across a vertical border
    a[y + 3, x:x + max_size + 1] = 4                                # ... of max_size + 1
    a[y + 6:y + 6 + max_size // 8, x + 10:x + 18] = 6              # a block of max_size across a tile corner
    a[y + 6 + max_size // 8 + 2:y + 8 + 2 * (max_size // 8), x + 10:x + 18] = 6
    a[y + 8 + 2 * (max_size // 8), x + 10] = 6                      # ... of max_size + 1
    a[2:2 + max_size, 3] = 9                                         # a column of max_size across horizontal borders
    a[2:3 + max_size, 7] = 9                                         # ... of max_size + 1
    return a, max_size, 0


PATTERNS = {"whole": whole, "serpentine": serpentine, "spiral": spiral, "checkerboard": checkerboard, "rings": rings,
            "exact_sizes": exact_sizes}


def informative(a, max_size, max_diff):
    """assert on the definition: something is removed, something is kept, and a kept component spans tiles"""
    roots, sizes = fr.components(a, max_diff)
    assert any(s <= max_size for s in sizes.values()), "nothing to remove"
    assert any(s > max_size for s in sizes.values()), "nothing to keep"
    h, w = a.shape
    yy, xx = np.mgrid[0:h, 0:w]
    tiles_x = (w + TILE_W - 1) // TILE_W
    ntiles = tiles_x * ((h + TILE_H - 1) // TILE_H)
    tile = (yy // TILE_H) * tiles_x + xx // TILE_W
    ok = roots >= 0
    pairs = np.unique(roots[ok] * ntiles + tile[ok])               # the (component, tile) pairs that occur
    ids, tiles = np.unique(pairs // ntiles, return_counts=True)
    assert any(t > 1 and sizes[int(r)] > max_size for r, t in zip(ids, tiles)), "no kept component spans two tiles"
    return sizes
