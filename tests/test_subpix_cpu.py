"""Subpixel refinement of the cost mode (sm_cost_refine): the definition pinned on hand-made
cost triples, its facts on maps of the oracle's cost mode, its accuracy on displaced textures, and the C entry's
argument checks before any device use.  No GPU needed."""
import numpy as np
import pytest

from tests import extreme_patterns as ep
from tests import oracle
from tests import subpix_reference as sr


@pytest.mark.parametrize("cost", ["sad", "ssd"])
def test_equal_rises_give_zero(cost):
    for a in (1, 2, 7, 1000, 625 * 65025):
        assert sr.fit_q(a, a, cost) == 0


@pytest.mark.parametrize("cost", ["sad", "ssd"])
def test_flat_right_side_gives_plus_eight(cost):
    for a in (1, 5, 123456, 625 * 65025):
        assert sr.fit_q(a, 0, cost) == 8
        assert sr.fit_q(0, a, cost) == -8


def test_negative_numerators_round_by_floor():
    # SSD a=1, b=2: (16 * -1 + 3) / 6 = -13 / 6 = -2.17 -> -3 (C truncation would give -2)
    assert sr.fit_q(1, 2, "ssd") == -3
    # SAD a=1, b=2: (-16 + 2) / 4 = -3.5 -> -4
    assert sr.fit_q(1, 2, "sad") == -4
    # SSD a=2, b=1: (16 + 3) / 6 = 3.17 -> 3;  SAD: (16 + 2) / 4 = 4.5 -> 4
    assert sr.fit_q(2, 1, "ssd") == 3
    assert sr.fit_q(2, 1, "sad") == 4
    # the two are mirror images up to the floor: q(a, b) + q(b, a) is 0 or -1
    rng = np.random.default_rng(3)
    a, b = rng.integers(1, 10**6, 1000), rng.integers(0, 10**6, 1000)
    for cost in ("sad", "ssd"):
        s = sr.fit_q(a, b, cost) + sr.fit_q(b, a, cost)
        assert set(np.unique(s)) <= {-1, 0}


def test_caller_made_rises_are_clamped_or_zero():
    assert sr.fit_q(-5, -5, "ssd") == 0 and sr.fit_q(-5, -5, "sad") == 0       # den <= 0
    assert sr.fit_q(3, -3, "ssd") == 0                                          # den = 0
    assert sr.fit_q(10, -9, "ssd") == 8                                         # 309 / 2 -> clamp
    assert sr.fit_q(-9, 10, "ssd") == -8
    assert sr.fit_q(-100, 1, "sad") == -8                                       # m = 1 -> clamp


@pytest.mark.parametrize("cost", ["sad", "ssd"])
def test_shift_range_ends_and_invalid_values(cost):
    D = 8
    s = np.array([1, D, 0, -3, D + 1, 4])
    c0, c1, c2 = np.array([5] * 6), np.array([1] * 6), np.array([1] * 6)       # would give +8 inside
    sub = sr.subpixel(c0, c1, c2, s, D, cost)
    assert sub.dtype == np.int16
    assert list(sub) == [16, 16 * D, 0, 0, 0, 16 * 4 + 8]
    assert list(sr.subpixel([9], [1], [9], [1], 1, cost)) == [16]             # D = 1: both ends at once
    assert np.iinfo(np.int16).max >= 16 * 512 + 8


@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
def test_refine_marks_missing_costs(mode):
    rng = np.random.default_rng(5)
    left, right = rng.integers(0, 256, (2, 9, 14), dtype=np.uint8)
    D = 6
    web = np.array([[0, -3, 1, D, D + 1, 3, 2] * 2] * 9, np.int32)
    sub, costs = sr.refine(left, right, web, D, 5, mode, "sad")
    assert (costs[:, web == 0] == -1).all() and (costs[:, web == D + 1] == -1).all()
    assert (costs[0, web == 1] == -1).all() and (costs[1:, web == 1] >= 0).all()
    assert (costs[2, web == D] == -1).all() and (costs[:2, web == D] >= 0).all()
    assert (sub[web == 0] == 0).all() and (sub[web == 1] == 16).all() and (sub[web == D] == 16 * D).all()


@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
@pytest.mark.parametrize("cost", ["sad", "ssd"])
def test_costs_equal_the_brute_force_window_sums(mode, cost):
    rng = np.random.default_rng(11)
    for w, h, D, sw in ((13, 7, 5, 9), (20, 11, 9, 5), (6, 5, 4, 7), (24, 9, 3, 1)):
        left, right = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
        web = rng.integers(1, D + 1, (h, w)).astype(np.int32)
        _, costs = sr.refine(left, right, web, D, sw, mode, cost)
        for d in range(D):
            diff = left.astype(np.int64) - ep._shifted_right(right.astype(np.int64), d, mode)
            plane = ep._window_sums(diff * diff if cost == "ssd" else np.abs(diff), sw, mode)
            for k in range(3):
                m = web - 2 + k == d
                assert np.array_equal(costs[k][m], plane[m])


@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
@pytest.mark.parametrize("cost", ["sad", "ssd"])
def test_cost_wta_maps_give_positive_rises(mode, cost):
    """first wins: a >= 1, b >= 0 on every map of the cost mode, so |q| <= 8 without the clamp"""
    rng = np.random.default_rng(17)
    for seed, (w, h, D, sw) in enumerate(((40, 24, 16, 5), (33, 20, 30, 9), (64, 16, 64, 3))):
        left, right = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
        if seed == 1:
            left //= 64                                     # few gray levels: many ties
            right //= 64
        best, web = oracle.cost_hot_path(left, right, D, sw, mode, cost)
        _, costs = sr.refine(left, right, web, D, sw, mode, cost)
        assert np.array_equal(costs[1], best)
        inner = (web >= 2) & (web <= D - 1)
        a = costs[0].astype(np.int64) - costs[1]
        b = costs[2].astype(np.int64) - costs[1]
        assert (a[inner] >= 1).all() and (b[inner] >= 0).all()
        den = a + b if cost == "ssd" else np.maximum(a, b)
        q = (16 * (a - b) + den) // (2 * np.where(den > 0, den, 1))
        assert (np.abs(q[inner]) <= 8).all()


def accuracy(cost, t, seeds=(0, 1, 2), refine=sr.refine):
    """-> (mean |sub / 16 - 1 - t|, mean |web - 1 - t|) over the seeds: 256 x 64, D = 32, 9 x 9, toroidal"""
    es, ei = [], []
    for seed in seeds:
        left, right = sr.texture(256, 64, seed, t)
        _, web = oracle.cost_hot_path(left, right, 32, 9, "toroidal", cost)
        sub, _ = refine(left, right, web, 32, 9, "toroidal", cost)
        es.append(np.abs(sub / 16.0 - 1 - t).mean())
        ei.append(np.abs(web - 1.0 - t).mean())
    return float(np.mean(es)), float(np.mean(ei))


ACCURACY_T = [10, 10.25, 10.5, 10.75, 10.125]


@pytest.mark.parametrize("cost", ["sad", "ssd"])
@pytest.mark.parametrize("t", ACCURACY_T)
def test_accuracy_on_displaced_textures(cost, t):
    """the fit recovers a known displacement: within 0.15 px everywhere, and below half the whole-pixel error
    wherever the displacement is fractional (measured: 0.013 .. 0.036 px)"""
    sub_err, int_err = accuracy(cost, t)
    assert sub_err <= 0.15
    if t != int(t):
        assert sub_err < 0.5 * int_err


def test_argument_validation_precedes_device_use():
    from stereomatching_amd import capi
    lib = capi.lib
    assert lib.sm_cost_refine(None, None, None, 1, 1, None, None, None, None) == capi.SM_ERR_ARG
    assert b"sm_cost_refine: plan is NULL" in lib.sm_last_error()
    assert capi.lib.sm_cost_refine.argtypes is not None and len(capi.lib.sm_cost_refine.argtypes) == 9
    assert "sm_cost_refine" in capi.declared_symbols()
