"""The cross-based matcher at the shapes its own module does not ask for (tests/cross_patterns.py SMALL, MANY_TILES,
MANY_SHIFTS; profiles/mutants/README.md, fourth audit): images narrower than a tile, than 8 columns and than an arm, one
column, fewer than 32 rows, a second tile of one column, more than 8 tiles a pair, and shifts above 255.  Every map of
sm_cross_wta, sm_cross_wta_right and sm_cross_lr is compared with tests/cross_reference.py by exact equality, in both
border modes; tests/test_cross_cpu.py holds what the expected maps must contain for the cases to mean anything."""
import functools

import numpy as np
import pytest
import torch

from tests import cross_patterns as cp
from tests import cross_reference as x

pytestmark = pytest.mark.gpu
MODES = ["toroidal", "ghost"]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def expected_maps(kind, w, h, d, census, tau, arm, mode, md, pairs):
    """-> (left, right, maps): (pairs, h, w) each, from the CPU definition alone"""
    if kind == "shifts":
        left, right = (a[None] for a in cp.many_shifts_pair(d))
    elif kind == "tall":
        left, right = (a[None] for a in cp.anti(w, h, 0))
    else:
        left, right = cp.related_pairs(w, h, pairs, 1000 * w + 10 * h + census)
    rows = [x.expected(left[q], right[q], d, census, tau, arm, mode, md) for q in range(pairs)]
    return left, right, {k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0]}


def every_map_is_exact(hip, kind, w, h, d, census, tau, arm, mode, md, pairs, max_pairs):
    left, right, e = expected_maps(kind, w, h, d, census, tau, arm, mode, md, pairs)
    plan = hip.StereoPlan(w, h, d, 1, mode, max_pairs=max_pairs)
    try:
        gl, gr = dev(left), dev(right)
        web, best, sub = plan.cross_wta(gl, gr, census, tau, arm, want_sub=True)
        web_right, best_right = plan.cross_wta_right(gl, gr, census, tau, arm)
        res = plan.cross_lr(gl, gr, census, tau, arm, max_diff=md, want_right=True, want_best=True, want_sub=True)
        torch.cuda.synchronize()
        tag = (kind, w, h, d, census, tau, arm, mode)
        assert np.array_equal(host(web), e["web"]), tag
        assert np.array_equal(host(best), e["best"]), tag
        assert np.array_equal(host(sub), e["sub"]), tag
        assert np.array_equal(host(web_right), e["web_right"]), tag
        assert np.array_equal(host(best_right), e["best_right"]), tag
        assert np.array_equal(host(res.web), e["checked"]), tag
        assert np.array_equal(host(res.web_right), e["web_right"]), tag
        assert np.array_equal(host(res.best), e["best"]), tag
        assert host(res.rejected).tolist() == e["rejected"].tolist(), tag
        assert np.array_equal(host(res.sub), e["sub_checked"]), tag
    finally:
        plan.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("census", [3, 7])
@pytest.mark.parametrize("w,h,d,arm", cp.SMALL, ids=[f"{c[0]}x{c[1]}" for c in cp.SMALL])
def test_small_images(hip, w, h, d, arm, census, mode):
    """(what each size is there for: tests/cross_patterns.py SMALL) two pairs on a plan of three, arms of every length"""
    for tau in cp.SMALL_TAUS:
        every_map_is_exact(hip, "small", w, h, d, census, tau, arm, mode, (w + tau) % 2, 2, 3)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("census", [3, 7])
def test_many_tiles(hip, census, mode):
    """6 x 3 tiles a pair: more than 8 and no multiple of 8; an odd D whose second turn ends on a lone shift"""
    w, h, d, arm, tau = cp.MANY_TILES
    every_map_is_exact(hip, "tiles", w, h, d, census, tau, arm, mode, 1, 2, 3)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("census", [3, 7])
@pytest.mark.parametrize("d", sorted(cp.MANY_SHIFTS))
def test_many_shifts(hip, d, census, mode):
    """answers above 256 in every map, D itself among them: the whole of the key's shift field"""
    every_map_is_exact(hip, "shifts", cp.MANY_SHIFTS_W, cp.MANY_SHIFTS_H, d, census, cp.MANY_SHIFTS_TAU,
                       cp.MANY_SHIFTS_ARM, mode, 1, 1, 1)


@pytest.mark.parametrize("mode", MODES)
def test_column_sums_past_16_bits(hip, mode):
    """anti(98, 77, 0), census 7, arm 15, no threshold: a tile's column sums reach 89280, so the halves of Q wrap (the
    extremes of tests/test_cross_gpu.py have 42 rows and stay below 2^16: tests/cross_patterns.py TALL_H), and the second
    shift of the pair wins at every pixel, so a carry or a borrow between the halves shows in `best`"""
    every_map_is_exact(hip, "tall", cp.TALL_W, cp.TALL_H, cp.TALL_D, 7, 255, 15, mode, 0, 1, 1)
