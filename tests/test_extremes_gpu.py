"""Every match and cost kernel at the extremes of its arithmetic (tests/extreme_patterns.py): full windows, lone
matches, all-tie maps, row and column bands that flip a whole window row in one slide, black against white.

The patterns of one geometry are the pairs of one batch -- one plan, one launch -- and every map is compared with
the CPU oracle (tests/oracle.py; lr_reference.py for the right-reference mode), failures reported by pattern name
and plan description.  The sweeps over random edges at density 0.5 (tests/test_hip_gpu.py) keep every winning
count near n^2 / 2 and almost never tie; these reach the top planes of k_match_bs's counts and its "no shift
matched" marker, the largest shift index of the popcount kernels' keys, every lane-merge tie, and the largest SAD /
SSD sums on both sides of the matrix-core kernel's position 256.  test_extreme_patterns_cpu.py proves the inputs
reach those extremes."""
import numpy as np
import pytest
import torch

from tests import extreme_patterns as xp
from tests import lr_reference as lr
from tests import oracle
from tests.test_hip_gpu import BUILT_BS, NO_CAP2, ONE_WAVE, TWO_WAVES, poisoned
from tests.test_lr_gpu import KERNEL_CHOICES

pytestmark = pytest.mark.gpu
MODES = ["toroidal", "ghost"]
W = 150

_oracle_cache = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def _cached(key, compute):
    if key not in _oracle_cache:
        _oracle_cache[key] = compute()
    return _oracle_cache[key]


def edge_case(w, h, sw, d, mode, names=xp.EDGE_PATTERNS, right=False):
    """-> (names, eL, eR, oracle best, oracle web) of a batch of edge patterns, the oracle cached per pattern"""
    n = xp.window(sw)
    names, le, re = xp.edge_batch(w, h, n, d, names)

    def one(i):
        if right:
            return lr.right_reference(le[i], re[i], d, sw, mode)
        return oracle.hot_path(le[i], re[i], d, sw, mode)
    res = [_cached(("edge", right, p, w, h, sw, d, mode), lambda i=i: one(i)) for i, p in enumerate(names)]
    return names, le, re, np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def gray_case(w, h, sw, d, mode, cost):
    names, left, right = xp.gray_batch(w, h)
    res = [_cached(("gray", p, w, h, sw, d, mode, cost),
                   lambda i=i: oracle.cost_hot_path(left[i], right[i], d, sw, mode, cost))
           for i, p in enumerate(names)]
    return names, left, right, np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def differences(names, got, want, what):
    """one line per pattern whose map differs: name, map, pixels that differ, the first of them"""
    out = []
    for i, p in enumerate(names):
        bad = np.argwhere(got[i] != want[i])
        if len(bad):
            y, x = bad[0]
            out.append(f"{p}: {what} differs at {len(bad)} px, first (y={y}, x={x}): {got[i][y, x]} != {want[i][y, x]}")
    return out


def match_batch(hip, le, re, d, sw, mode, options=None, web_dtype=torch.int32):
    h, w = le.shape[-2:]
    plan = hip.StereoPlan(w, h, d, sw, mode, max_pairs=len(le), options=options)
    plan.load_edges(dev(le), dev(re))
    web, best = plan.match_wta(len(le), want_best=True, web=poisoned(len(le), h, w, web_dtype),
                               best=poisoned(len(le), h, w), web_dtype=web_dtype)
    torch.cuda.synchronize()
    desc = plan.describe()
    plan.close()
    return host(best), host(web.to(torch.int32)), desc


def check_match(hip, sw, d, mode, h, options=None, names=xp.EDGE_PATTERNS):
    names, le, re, ob, ow = edge_case(W, h, sw, d, mode, names)
    if tuple(names) == xp.EDGE_PATTERNS:        # the batch reaches what it is meant to (see the module docstring)
        assert xp.coverage_gaps(ob, xp.window(sw), mode) == [], (sw, d, mode)
    best, web, desc = match_batch(hip, le, re, d, sw, mode, options)
    bad = differences(names, web, ow, "web") + differences(names, best, ob, "best")
    assert not bad, "\n".join([desc, *bad])
    return desc


# ---------------------------------------------------------------------------
# k_match_bs: every built instantiation
# ---------------------------------------------------------------------------

SHAPES = {"one_wave": ONE_WAVE, "one_wave_uncapped": dict(ONE_WAVE, **NO_CAP2), "two_waves": TWO_WAVES}
# (lane merge, shift-lanes per word, D short of filling them by, image height above the window)
MERGES = {"dpp_2": (1, 2, 0, 10), "dpp_2_ragged": (1, 2, 3, 13), "lds_4": (2, 4, 0, 13), "lds_8_ragged": (2, 8, 3, 10)}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("merge", list(MERGES))
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("n,ds", BUILT_BS)
def test_every_built_kernel_at_the_extremes(hip, n, ds, shape, merge, mode):
    """window x shifts per lane x {one wave, one wave uncapped, two-wave workgroups} x {lanes merged by DPP (2 per
    word), through LDS (4 and 8 per word)} x {D fills the lanes, D = that - 3} x border, tiles of 4 rows, heights
    whose last tile is whole and ragged: the top planes of the count, the marker, every lane-merge tie"""
    lane_merge, nl, short, dh = MERGES[merge]
    opts = dict(SHAPES[shape], shifts_per_lane=ds, tile_h=4, lane_merge=lane_merge)
    desc = check_match(hip, n, nl * ds - short, mode, n + dh, opts)
    duo = shape == "two_waves"
    assert f"lanes of {ds})" in desc and f"x{8 if duo else 4} px" in desc, desc
    assert ("two-wave workgroups" in desc) == duo, desc
    if shape == "one_wave_uncapped":
        assert "2 waves/SIMD variant" not in desc, desc
    assert ("lanes merged through LDS" in desc) == (lane_merge == 2), desc
    if lane_merge == 2:
        assert f"{nl} shift-lanes of {ds})" in desc, desc


# ---------------------------------------------------------------------------
# the popcount kernels A / B / C and the generic kernel
# ---------------------------------------------------------------------------

LARGE_D = xp.TIE_PATTERNS + ("true_shift_last", "lone_match")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sw", [5, 11, 15, 21, 25])
def test_popcount_kernels_at_the_extremes(hip, sw, mode):
    """kernel_family = 1: every pattern at D = 64; at D = 1024 (the largest tiled D: shift index 1023 in the
    A << 10 | d key) the all-tie and full-window patterns, a unique match at d = 1023 and the lone matches"""
    for d, names in ((64, xp.EDGE_PATTERNS), (1024, LARGE_D)):
        desc = check_match(hip, sw, d, mode, sw + 10, dict(kernel_family=1), names)
        assert "tiled kernel" in desc, desc


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sw,d,names", [(27, 64, xp.EDGE_PATTERNS), (5, 1100, LARGE_D)])
def test_generic_kernel_at_the_extremes(hip, sw, d, names, mode):
    desc = check_match(hip, sw, d, mode, sw + 12, None, names)
    assert "generic kernel" in desc, desc


# ---------------------------------------------------------------------------
# narrow maps
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d,dtype", [(255, torch.uint8), (256, torch.uint16), (300, torch.uint16)])
def test_narrow_maps_of_all_tie_patterns(hip, d, dtype, mode):
    """every pixel of an all-tie map stores D (255: the largest byte), on the plan's own kernel, the bit-sliced
    kernel's narrow stores and the staging map of a popcount plan; equal to the int32 map and the oracle"""
    sw, h = 9, 21
    names, le, re, ob, ow = edge_case(W, h, sw, d, mode, xp.TIE_PATTERNS + ("true_shift_last",))
    for opts in (None, dict(shifts_per_lane=16), dict(kernel_family=1)):
        best32, web32, desc = match_batch(hip, le, re, d, sw, mode, opts)
        bestn, webn, _ = match_batch(hip, le, re, d, sw, mode, opts, web_dtype=dtype)
        if opts and "shifts_per_lane" in opts:
            assert "bit-sliced" in desc, desc
        bad = (differences(names, web32, ow, "web") + differences(names, webn, ow, f"{dtype} web") +
               differences(names, best32, ob, "best") + differences(names, bestn, ob, f"best beside {dtype}"))
        assert not bad, "\n".join([desc, *bad])


# ---------------------------------------------------------------------------
# right-reference mode
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sw,d", [(9, 64), (5, 30), (21, 32)])
@pytest.mark.parametrize("opts", KERNEL_CHOICES, ids=lambda o: "default" if o is None else
                         "-".join(f"{k}{v}" for k, v in o.items()))
def test_right_reference_mode_at_the_extremes(hip, opts, sw, d, mode):
    """sm_match_wta_right over the mirrored images carries the extremes unchanged, on every kernel choice"""
    h = sw + 11
    names, le, re, ob, ow = edge_case(W, h, sw, d, mode, right=True)
    assert xp.coverage_gaps(ob, sw, mode) == [], (sw, d, mode)
    plan = hip.StereoPlan(W, h, d, sw, mode, max_pairs=len(names), options=opts)
    plan.load_edges(dev(le), dev(re))
    web_right, best_right = plan.match_wta_right(len(names))
    torch.cuda.synchronize()
    bad = (differences(names, host(web_right), ow, "web_right") +
           differences(names, host(best_right), ob, "best_right"))
    assert not bad, "\n".join([plan.describe(), *bad])
    plan.close()


# ---------------------------------------------------------------------------
# cost mode (parity unpinned: the build's own CPU definition is the oracle)
# ---------------------------------------------------------------------------

def cost_batch(hip, left, right, d, sw, mode, cost, options=None):
    h, w = left.shape[-2:]
    plan = hip.StereoPlan(w, h, d, sw, mode, max_pairs=len(left), options=options)
    web, best = plan.cost_wta(dev(left), dev(right), cost, web=poisoned(len(left), h, w),
                              best=poisoned(len(left), h, w))
    torch.cuda.synchronize()
    plan.close()
    return host(best), host(web)


def check_cost(hip, sw, d, mode, cost, option_sets):
    names, left, right, ob, ow = gray_case(W, sw + 10, sw, d, mode, cost)
    bad = []
    for opts in option_sets:
        best, web = cost_batch(hip, left, right, d, sw, mode, cost, opts)
        bad += [f"{opts}: {b}" for b in differences(names, web, ow, "web") + differences(names, best, ob, "best")]
    assert not bad, "\n".join([f"{cost} {mode} n={sw} D={d}", *bad])
    return names, ob


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d", [1, 31, 32, 33, 64, 65, 224, 225, 255, 256])
@pytest.mark.parametrize("sw", [3, 5, 7, 9, 11])
def test_ssd_kernels_at_the_extremes(hip, sw, d, mode):
    """k_ssd_mfma<N, NB> (the plan's choice; NB = 1 .. 9, so that bands cross position 256 from D = 225 on; in ghost
    mode k_cost_strip behind it) and the general masked kernel (cost_kernel = 1) on the whole image: the largest sums
    N^2 x 65025 and every shift tying, where the first must win -- across the split of positions 0 .. 255 and 256 .."""
    sets = [None, dict(cost_kernel=1)]
    names, ob = check_cost(hip, sw, d, mode, "ssd", sets)
    if mode == "toroidal":
        assert (ob[names.index("black_white")] == sw * sw * 65025).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sw", [3, 5, 7, 9, 11, 13, 15, 17, 19, 21])
def test_sad_kernels_at_the_extremes(hip, sw, mode):
    """the quad-SAD / prefix-chain kernels in workgroups of 1, 2 and 4 waves (in ghost mode k_cost_strip behind them)
    and the general masked kernel (cost_kernel = 1) on the whole image, at 1, 33 and the most shifts they are built
    for (240 from 17 x 17 on: the 8-bit shift field of the split keys; 500 below)"""
    sets = [dict(cost_kernel=0, cost_workgroup_waves=wv) for wv in (1, 2, 4)] + [dict(cost_kernel=1)]
    for d in (1, 33, 240 if sw > 15 else 500):
        names, ob = check_cost(hip, sw, d, mode, "sad", sets)
        if mode == "toroidal":
            assert (ob[names.index("black_white")] == sw * sw * 255).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sw", [3, 5, 7, 9, 11, 13, 15])
def test_sad_full_cost_beside_a_free_shift_below_zero(hip, sw, mode):
    """k_sad_pc's lanes start their first quad up to three positions below shift 0, and only the constant those sums
    start at (BIG) keeps them from winning: it must exceed every real sum, by one at least, because the earlier
    position wins a tie.  That decides a pixel only where every real shift costs BIG more than a position below 0
    does -- nowhere in the other patterns (the mutation audit's S1 and S3 passed them all;
    test_a_free_shift_below_zero_tells_a_poison_constant_that_is_too_small is the CPU proof).  Here the right image is
    columns of 0 and 255 and the left one the same a column on: the shift -1 would cost 0, and with D = 1 the one real
    shift costs 255 at every tap, n^2 255 in all.  32 columns (even, so that the stripes meet across the wrap) by n + 2
    rows are one tile of every kernel; three of a lane group's four column residues have a position below 0."""
    w, h = xp.FREE_SHIFT_SHAPE[0], sw + xp.FREE_SHIFT_SHAPE[1]
    left, right = xp.gray_pattern(xp.FREE_SHIFT_BELOW_ZERO, w, h)
    ob, ow = oracle.cost_hot_path(left, right, 1, sw, mode, "sad")
    assert (ow == 1).all()
    if mode == "toroidal":
        assert (ob == sw * sw * 255).all()
    sets = [dict(cost_kernel=0, cost_workgroup_waves=wv) for wv in (1, 2, 4)] + [dict(cost_kernel=1)]
    bad = []
    for opts in sets:
        best, web = cost_batch(hip, left[None], right[None], 1, sw, mode, "sad", opts)
        bad += [f"{opts}: {b}" for b in differences(["stripes"], web, ow[None], "web") +
                differences(["stripes"], best, ob[None], "best")]
    assert not bad, "\n".join([f"sad {mode} n={sw} D=1", *bad])
