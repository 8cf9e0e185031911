"""The census and SGM kernels at the extremes of their arithmetic (tests/census_extreme_patterns.py): window costs of
exactly 30000 in the packed u16 fields and the keys A << 16 | d of k_census_wta, in the first and the last lane of a
launch and, with the 0x8000 bias on top, in the first shift past the range; exact ties at a high cost between shifts
49 apart, across launches; all-tie maps at 26250; L_r = 62767 and S = 502136 in k_sgm_path's keys S << 8 | d, with a
padded shift range whose entries must lose.  Every expected value comes from the numpy definitions
(tests/census_reference.py, tests/sgm_reference.py), none from the HIP path, and every comparison is exact;
tests/test_census_extremes_cpu.py pins that the inputs reach the bounds."""
import numpy as np
import pytest
import torch

from tests import census_extreme_patterns as cx
from tests import census_reference as cr
from tests.test_census_gpu import dev, host
from tests.test_sgm_gpu import check_all

pytestmark = pytest.mark.gpu
MODES = ["toroidal", "ghost"]
# 98 x 28: the lattice closes across the wrap, W % 4 != 0 (scalar stores); 196 x 28: W % 4 == 0 (int4 stores);
# 100 x 30: the seam breaks the lattice
SHAPES = [(98, 28), (196, 28), (100, 30)]
SHIFTS = [1, 8, 9, 128, 129, 256, 257, 512]


def shifts_of_the_maximum(d, w):
    """k = 0 / D - 1: the full cost in the first / last lane of a launch; k = D mod W: in the first shift past the range"""
    return sorted({0, d - 1, d % w})


def refine_webs(k, d, h, w):
    """a map that puts s - 2, s - 1 and s on the shift k of the full cost (s = k + 2, k + 1, k, clipped to 1 .. D),
    mixed pixel by pixel"""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.clip(k + (xx + 2 * yy) % 3, 1, d).astype(np.int32)


def check_census(plan, left, right, d, sw, census, mode, tag, k=None, md=1):
    """census_wta, census_wta_right, census_lr with every map, and census_refine with its costs -- on the kernel's own
    map and, given k, on a map laid around shift k -- of one gray pair against the definition; returns the definition's
    maps"""
    h, w = left.shape
    gl, gr = dev(left[None]), dev(right[None])
    e = cr.expected(left, right, d, sw, census, mode, md)
    web, best = plan.census_wta(gl, gr, census)
    web_right, best_right = plan.census_wta_right(gl, gr, census)
    res = plan.census_lr(gl, gr, census, max_diff=md, want_right=True, want_best=True)
    maps = [e["web"]] + ([refine_webs(k, d, h, w)] if k is not None else [])
    refined = [plan.census_refine(gl, gr, dev(m[None]), census, want_costs=True) for m in maps]
    own_sub, own_costs = plan.census_refine(gl, gr, web, census, want_costs=True)
    torch.cuda.synchronize()
    assert np.array_equal(host(web)[0], e["web"]), tag
    assert np.array_equal(host(best)[0], e["best"]), tag
    assert np.array_equal(host(web_right)[0], e["web_right"]), tag
    assert np.array_equal(host(best_right)[0], e["best_right"]), tag
    assert np.array_equal(host(res.web)[0], e["checked"]), tag
    assert np.array_equal(host(res.web_right)[0], e["web_right"]), tag
    assert np.array_equal(host(res.best)[0], e["best"]), tag
    assert int(res.rejected[0]) == e["rejected"], tag
    for m, (sub, costs) in zip(maps, refined):
        want_sub, want_costs = cr.refine(left, right, m, d, sw, census, mode)
        assert np.array_equal(host(costs)[0], want_costs), tag
        assert np.array_equal(host(sub)[0], want_sub), tag
    # the kernel's own map: the one just shown to be the definition's
    want_sub, want_costs = cr.refine(left, right, e["web"], d, sw, census, mode)
    assert np.array_equal(host(own_costs)[0], want_costs) and np.array_equal(host(own_sub)[0], want_sub), tag
    assert np.array_equal(want_costs[1], e["best"]), tag
    return e


# ---------------------------------------------------------------------------
# census
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("d", SHIFTS)
def test_census_full_cost_at_every_shift_count(hip, mode, w, h, d):
    """anti, c = 7, n = 25: A = 30000 (98 x 28 and 196 x 28, toroidal) in the first lane, in the last lane and just
    past the range of the last launch, for one launch (D <= 128) and for two to four"""
    plan = hip.StereoPlan(w, h, d, 25, mode)
    try:
        for k in shifts_of_the_maximum(d, w):
            left, right = cx.anti(w, h, k)
            e = check_census(plan, left, right, d, 25, 7, mode, (mode, w, h, d, k), k=k)
            if mode == "toroidal" and w % 49 == 0 and k < d:
                # the input is on the bound: shift k costs 30000 at every pixel (so best is 30000 where D = 1)
                assert (cr.window_costs(left, right, k, 25, 7, mode) == 30000).all()
                assert d > 1 or (e["best"] == 30000).all()
    finally:
        plan.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("census,sw", [(3, 1), (3, 9), (3, 25), (5, 1), (5, 9), (5, 25), (7, 1), (7, 9)])
def test_census_full_cost_at_every_width_and_window(hip, mode, census, sw):
    """the other census widths and windows (A = (c^2 - 1) n^2 at shift k), thinned: one launch and several, every
    shape, each place of the maximum"""
    for w, h, d, k in ((98, 28, 129, 128), (196, 28, 257, 257 % 196), (100, 30, 9, 0), (98, 28, 512, 512 % 98),
                       (196, 28, 128, 127), (98, 28, 8, 8)):
        plan = hip.StereoPlan(w, h, d, sw, mode)
        try:
            left, right = cx.anti(w, h, k)
            check_census(plan, left, right, d, sw, census, mode, (mode, census, sw, w, h, d, k), k=k)
        finally:
            plan.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d", [1, 130, 300, 512])
@pytest.mark.parametrize("sw", [1, 25])
def test_census_all_tie_at_a_high_cost(hip, mode, d, sw):
    """rows_anti at 56 x 49: every shift of every pixel costs the same (26250 for c = 7, n = 25), within a launch and
    across launches: the first shift wins everywhere"""
    w, h = 56, 49
    left, right = cx.rows_anti(w, h)
    n = cx.window(sw)
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        for census in (7, 5) if d == 300 else (7,):
            check_census(plan, left, right, d, sw, census, mode, (mode, d, sw, census))
            if mode != "toroidal":
                continue
            const = (census * census - census) * n * n
            assert const == 26250 or (census, n) != (7, 25)
            gl, gr = dev(left[None]), dev(right[None])
            web, best = plan.census_wta(gl, gr, census)
            web_right, best_right = plan.census_wta_right(gl, gr, census)
            assert (host(web) == 1).all() and (host(best) == const).all()
            assert (host(web_right) == 1).all() and (host(best_right) == const).all()
    finally:
        plan.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("w,h", [(98, 28), (196, 28), (100, 30)])
def test_census_cheap_shifts_past_a_full_cost(hip, mode, w, h):
    """comb: the only shift of the range (D = 1) costs 30000 while the lane's other shifts cost next to nothing: their
    biased fields must lose all the same; and with the cheap shifts inside the range (D = 2, 8, 130)"""
    left, right = cx.comb(w, h)
    for d in (1, 2, 8, 130):
        plan = hip.StereoPlan(w, h, d, 25, mode)
        try:
            e = check_census(plan, left, right, d, 25, 7, mode, (mode, w, h, d), k=1)
            if d == 1 and mode == "toroidal" and w % 98 == 0:
                assert (e["best"] == 30000).all()
        finally:
            plan.close()


@pytest.mark.parametrize("census", [3, 5, 7])
@pytest.mark.parametrize("mode", MODES)
def test_census_degenerate_levels(hip, census, mode):
    """all 0, all 255 and 0 / 255 images: equal values and the ghost halo against the strict `<`, through
    census_transform (bit-exact) and census_lr"""
    for w, h, d, sw in ((67, 19, 20, 5), (64, 16, 9, 3)):
        plan = hip.StereoPlan(w, h, d, sw, mode, max_pairs=1)
        try:
            for name in cx.LEVEL_PATTERNS:
                left, right = cx.level_pair(name, w, h)
                got = host(plan.census_transform(dev(np.stack([left, right])), census)).view(np.uint64)
                assert np.array_equal(got[0], cr.transform(left, census, mode)), (name, w, h)
                assert np.array_equal(got[1], cr.transform(right, census, mode)), (name, w, h)
                check_census(plan, left, right, d, sw, census, mode, (name, mode, census, w, h), md=0)
        finally:
            plan.close()


# ---------------------------------------------------------------------------
# SGM
# ---------------------------------------------------------------------------

PENALTIES = [(32767, 32767), (0, 32767), (0, 0)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d", [64, 128, 200, 256])
@pytest.mark.parametrize("p1,p2", PENALTIES)
def test_sgm_at_its_u16_and_key_bounds(hip, mode, d, p1, p2):
    """anti(98, 28, k), n = 25, c = 7, 8 paths: L_r up to 62767 and S up to 502136 (toroidal, P2 = 32767), with 1, 2 and
    4 shifts per lane and, for D = 200, a padded range whose entries d >= D must lose"""
    w, h = 98, 28
    plan = hip.StereoPlan(w, h, d, 25, mode)
    try:
        for k in (5, 0, d - 1):
            left, right = cx.anti(w, h, k)
            check_all(plan, left[None], right[None], d, 25, 7, p1, p2, 8, mode, 1, 1, (mode, d, p1, p2, k))
    finally:
        plan.close()


@pytest.mark.parametrize("mode", MODES)
def test_sgm_full_cost_at_the_only_shift(hip, mode):
    """anti(98, 28, 0), D = 1: the one shift costs 30000 at every pixel (toroidal), so best = paths * 30000 and the data
    term's u16 store shows in a map.  With more shifts a cheaper one wins and the full cost reaches no map: a data term
    saturated at 0x7000 passed every other case here (profiles/mutants/README.md, census_c)"""
    w, h = 98, 28
    left, right = cx.anti(w, h, 0)
    plan = hip.StereoPlan(w, h, 1, 25, mode)
    try:
        for paths in (8, 4):
            check_all(plan, left[None], right[None], 1, 25, 7, 32767, 32767, paths, mode, 1, 0, (mode, paths))
        if mode == "toroidal":
            web, best, _ = plan.sgm_wta(dev(left[None]), dev(right[None]), 7, 32767, 32767, 4, want_sub=True)
            assert (host(web) == 1).all() and (host(best) == 4 * 30000).all()
    finally:
        plan.close()


@pytest.mark.parametrize("mode", MODES)
def test_sgm_bounds_with_four_paths_and_in_a_batch(hip, mode):
    """4 paths on the padded range; a batch of two pairs with distinct k, so that the volumes are reused between
    pairs at full range"""
    w, h = 98, 28
    plan = hip.StereoPlan(w, h, 200, 25, mode)
    try:
        for p1, p2 in PENALTIES[:2]:
            left, right = cx.anti(w, h, 5)
            check_all(plan, left[None], right[None], 200, 25, 7, p1, p2, 4, mode, 1, 0, (mode, 200, p1, p2, 4))
    finally:
        plan.close()
    plan = hip.StereoPlan(w, h, 256, 25, mode, max_pairs=2)
    try:
        pairs = [cx.anti(w, h, 5), cx.anti(w, h, 255)]
        left, right = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        check_all(plan, left, right, 256, 25, 7, 32767, 32767, 8, mode, 2, 1, (mode, "batch"))
        # the same volumes, now at the low end, then at the bound again
        check_all(plan, left[::-1].copy(), right[::-1].copy(), 256, 25, 7, 0, 32767, 8, mode, 2, 1, (mode, "batch 2"))
    finally:
        plan.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("p1,p2", PENALTIES)
def test_sgm_all_tie_at_a_high_cost(hip, mode, p1, p2):
    """rows_anti, D = 256: S is constant over d at every pixel, so web is 1, sub is 16 and (toroidal) best is
    paths * 26250"""
    w, h, d = 56, 49, 256
    left, right = cx.rows_anti(w, h)
    plan = hip.StereoPlan(w, h, d, 25, mode)
    try:
        for paths in (8, 4):
            check_all(plan, left[None], right[None], d, 25, 7, p1, p2, paths, mode, 1, 0, (mode, p1, p2, paths))
            if mode != "toroidal":
                continue
            web, best, sub = plan.sgm_wta(dev(left[None]), dev(right[None]), 7, p1, p2, paths, want_sub=True)
            assert (host(web) == 1).all() and (host(sub) == 16).all() and (host(best) == paths * 26250).all()
            web_right, best_right = plan.sgm_wta_right(dev(left[None]), dev(right[None]), 7, p1, p2, paths)
            assert (host(web_right) == 1).all() and (host(best_right) == paths * 26250).all()
    finally:
        plan.close()


@pytest.mark.parametrize("mode", MODES)
def test_sgm_low_end(hip, mode):
    """anti with n = 1, c = 3: A <= 8, with ties everywhere"""
    w, h = 98, 28
    for d, k, p1, p2, paths in ((64, 3, 0, 0, 8), (64, 63, 1, 2, 4), (100, 0, 32767, 32767, 8), (256, 9, 0, 32767, 8)):
        left, right = cx.anti(w, h, k)
        plan = hip.StereoPlan(w, h, d, 1, mode)
        try:
            check_all(plan, left[None], right[None], d, 1, 3, p1, p2, paths, mode, 1, 1, (mode, d, k, p1, p2, paths))
        finally:
            plan.close()
