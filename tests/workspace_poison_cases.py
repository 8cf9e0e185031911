"""Cases of the workspace poison tests (test_workspace_poison_gpu.py) and of the CPU test that they are informative
(test_workspace_poison_cpu.py): the poison words, the shapes, the inputs and -- computed once per process and never
changed -- the expected results, every one from the CPU definitions (tests/oracle.py and the *_reference modules).

The shapes are the smallest at which the tiling of a workspace can still go wrong: 129 x 33 is one pixel past two
64-pixel tiles / chunks and one row past two 16-row tiles; 66 x 2 has a ragged second tile and fewer rows than any tile
(its only window is 1: a window must fit the image).  max_pairs is 3, so that a batch of one pair has the slots of two
unused pairs behind it."""
import functools

import numpy as np

from stereomatching_amd.synth import make_pair
from tests import census_reference as cr
from tests import cost_lr_reference as clr
from tests import filter_patterns as fp
from tests import filter_reference as fr
from tests import interp_patterns as ip
from tests import interp_reference as ir
from tests import lr_reference as lr
from tests import oracle
from tests import reproject_patterns as pp
from tests import reproject_reference as rref
from tests import sgm_reference as sr

# in this order: a harsher word never runs once a milder one has shown a difference
WORDS = (
    0x00000001,     # first: as an int32 an in-range index on every shape here, and non-zero in every 32-bit word
    0x00000000,     # what fresh device memory very often holds: the state the other modules test by accident
    0x7FFF7FFF,     # the largest positive 16-bit cost in both halves: only a forgotten MINIMUM initialisation sees it
    0x80008000,     # the invalid-shift bias of the census fields, and negative as an int16
    0xA5A5A5A5,
    0xFFFFFFFF,     # -1: the "invalid" label and the missing cost
)
MAXP = 3
THR = 0.15
MODES = ("toroidal", "ghost")
# mode -> (W, H, D, window): D in {16, 48}, window 3 or 5 (1 where the image has two rows)
IMAGE_CASES = {"toroidal": ((129, 33, 16, 3), (66, 2, 48, 1)), "ghost": ((129, 33, 48, 5), (66, 2, 16, 1))}
MAP_SIZES = ((129, 33), (66, 2))
# the interpolation joins segments of 64 rows by carries: one more size, with three segments (the others have one)
INTERP_SIZES = MAP_SIZES + ((40, 130),)
INTERP_INVALID = (0.97, 0.6, 0.995)     # pair 0 (the batch of one): whole 64-pixel chunks and segments without a valid pixel
SPECKLE = (4, 1)                        # (max_size, max_diff)
CLOUD_BIG = (640, 420)                  # 263 tiles of 1024 pixels: k_cloud_scan takes a second turn of its 256 lanes
Z_GATES = pp.Z_GATES

# the interleaving test: one plan, two settings of every stage that has a parameter
INTERLEAVE = dict(size=(129, 33, 16, 3), mode="toroidal", max_pairs=2, census=(7, 5), sgm=((8, 10, 120), (4, 3, 40)),
                  speckle=((4, 1), (2, 2)), z_gates=Z_GATES, thresholds=(0.15, 0.3), cost="sad", max_diff=1)


@functools.lru_cache(maxsize=None)
def images(w, h, d, pairs=MAXP, seed=0):
    """-> (left, right) uint8 [pairs][H][W]: scenes, different content per pair"""
    imgs = [make_pair(w, h, d, seed=1000 * seed + 17 * w + d + q, kind="scene") for q in range(pairs)]
    left, right = np.stack([a for a, _ in imgs]), np.stack([b for _, b in imgs])
    left.setflags(write=False)
    right.setflags(write=False)
    return left, right


def _stack(rows):
    """list of dicts of arrays -> dict of stacked, read-only arrays"""
    res = {k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0]}
    for v in res.values():
        v.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def edge_expected(mode, w, h, d, sw, max_diff, thr=THR, pairs=MAXP, seed=0):
    left, right = images(w, h, d, pairs, seed)
    rows = []
    for q in range(pairs):
        el, er = oracle.find_all_edges(left[q], thr, mode), oracle.find_all_edges(right[q], thr, mode)
        best, web = oracle.hot_path(el, er, d, sw, mode)
        best_r, web_r = lr.right_reference(el, er, d, sw, mode)
        checked, rejected = lr.lr_check(web, web_r, max_diff, mode)
        rows.append(dict(best=best, web=web, best_right=best_r, web_right=web_r, checked=checked, rejected=rejected))
    return _stack(rows)


@functools.lru_cache(maxsize=None)
def cost_expected(mode, w, h, d, sw, cost, max_diff, pairs=MAXP, seed=0):
    left, right = images(w, h, d, pairs, seed)
    rows = []
    for q in range(pairs):
        best, web = oracle.cost_hot_path(left[q], right[q], d, sw, mode, cost)
        best_r, web_r = clr.right_reference(left[q], right[q], d, sw, mode, cost)
        checked, rejected = lr.lr_check(web, web_r, max_diff, mode)
        rows.append(dict(best=best, web=web, best_right=best_r, web_right=web_r, checked=checked, rejected=rejected))
    return _stack(rows)


@functools.lru_cache(maxsize=None)
def census_expected(mode, w, h, d, sw, census, max_diff, pairs=MAXP, seed=0):
    left, right = images(w, h, d, pairs, seed)
    rows = []
    for q in range(pairs):
        e = cr.expected(left[q], right[q], d, sw, census, mode, max_diff)
        e["sub"], e["costs"] = cr.refine(left[q], right[q], e["web"], d, sw, census, mode)
        rows.append(e)
    return _stack(rows)


@functools.lru_cache(maxsize=None)
def sgm_expected(mode, w, h, d, sw, census, p1, p2, paths, max_diff, pairs=MAXP, seed=0):
    left, right = images(w, h, d, pairs, seed)
    return _stack([sr.expected(left[q], right[q], d, sw, census, p1, p2, paths, mode, max_diff) for q in range(pairs)])


@functools.lru_cache(maxsize=None)
def speckle_case(w, h, dtype, max_size=SPECKLE[0], max_diff=SPECKLE[1], pairs=MAXP):
    """-> (maps, kept maps, removed counts)"""
    maps = np.stack([fp.random_map(w, h, dtype, 7 * w + q, (0.3, 0.45, 0.2)[q % 3], 1, 5, negative=True)
                     for q in range(pairs)])
    want = [fr.speckle(m, max_size, max_diff) for m in maps]
    return maps, np.stack([x[0] for x in want]), np.array([x[1] for x in want], np.int32)


@functools.lru_cache(maxsize=None)
def interp_case(w, h, dtype, pairs=MAXP):
    """-> (maps, classes, interpolated maps, filled counts)"""
    maps = np.stack([ip.random_map(w, h, dtype, 5 * h + q, INTERP_INVALID[q % 3], 1, 900, negative=True)
                     for q in range(pairs)])
    cls = np.stack([ip.random_class(w, h, 3 * w + q) for q in range(pairs)])
    want = np.stack([ir.interpolate(maps[q], cls[q]) for q in range(pairs)])
    return maps, cls, want, np.array([ir.filled(maps[q], want[q]) for q in range(pairs)], np.int32)


@functools.lru_cache(maxsize=None)
def cloud_case(w, h, dtype, gate_index, with_gray, pattern="random_50", pairs=MAXP):
    """-> (maps, gray or None, q, per pair (records [count][4] float32, index [count] int32))"""
    maps = pp.make_map(pattern, pairs, w, h, dtype, seed=w + h)
    g = pp.gray(pairs, w, h, w) if with_gray else None
    q = pp.matrices(w, h)["rig"]
    wants = tuple(rref.point_cloud(maps[p], q, None if g is None else g[p], Z_GATES[gate_index]) for p in range(pairs))
    return maps, g, q, wants


@functools.lru_cache(maxsize=None)
def cloud_big_case():
    """-> (all-kept map, none-kept map, q, the all-kept map's (records, index)): int32, no gate"""
    w, h = CLOUD_BIG
    full = pp.make_map("all_valid", 1, w, h, np.int32, seed=5)[0]
    none = pp.make_map("all_zero", 1, w, h, np.int32, seed=5)[0]
    q = pp.matrices(w, h)["rig"]
    return full, none, q, rref.point_cloud(full, q, None, None)
