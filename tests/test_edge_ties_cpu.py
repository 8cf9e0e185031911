"""CPU proofs behind test_edge_ties_gpu.py (tests/edge_tie_patterns.py): the margin argument of csrc/sm_edges.hip's
f32 prefilter, the numpy restatement of the double decision against the oracle and against digests of the compiled
reference, and that the near-tie images reach every band pair in every orientation and every kernel position they
are meant to."""
import json
import sys

import numpy as np
import pytest

from tests import edge_tie_patterns as et
from tests import oracle
from tests.conftest import GOLDEN_DIR, sha256_of

sys.path.insert(0, str(GOLDEN_DIR))
import make_golden  # noqa: E402

MODES = ["toroidal", "ghost"]


def margin_thresholds():
    """>= 500 thresholds: the named ones, the tie-richest 2d/k (k <= 1530), the worst-rounding (float)(T/2) and
    random ones -- deterministic"""
    rng = np.random.default_rng(2024)
    ts = [*et.GPU_THRESHOLDS, 1e-12, 0.999999, 1.0 - 2.0 ** -40]
    ts += [t for t, _ in et.tie_richest_thresholds(200)]
    ts += et.worst_rounding_thresholds(150)
    ts += rng.random(100).tolist() + (10.0 ** rng.uniform(-9, 0, 50)).tolist()
    return sorted(set(ts))


def test_margin_argument_holds_for_500_thresholds():
    """no pair outside the band |F| <= 2^-12 has an f32 sign that disagrees with the double decision"""
    ts = margin_thresholds()
    assert len(ts) >= 500
    bad = [e for t in ts for e in et.outside_band_sign_errors(t)]
    assert not bad, bad[:5]


def test_band_counts_of_the_issue():
    """the exact calculator against a count made by hand: (band, f32-wrong) pairs"""
    want = {0.15: (35, 10), 1.0 / 3.0: (219, 74), 2.0 / 3.0: (765, 252), 1.0: (511, 172)}
    for t, (nb, nw) in want.items():
        band, wrong = et.band_pairs(t)
        assert (len(band), len(wrong)) == (nb, nw), t
        assert set(wrong) <= set(band)


def test_band_agrees_with_single_pair_arithmetic():
    """band_pairs' vectorised screen against prefilter_exact, pair by pair, around every band pair"""
    for t in (0.15, 2.0 / 3.0, 0.4, 1e-9):
        band = set(et.band_pairs(t)[0])
        for a, b in list(band)[:60]:
            for da in (-1, 0, 1):
                for db in (-1, 0, 1):
                    p = (a + da, b + db)
                    if 0 <= p[0] < et.SUMS and 0 <= p[1] < et.SUMS:
                        assert (abs(et.prefilter_exact(*p, t)) <= et.MARGIN) == (p in band), (t, p)


def test_round_f32_is_ieee_round_to_nearest_even():
    from fractions import Fraction
    rng = np.random.default_rng(3)
    for v in rng.uniform(-1000, 1000, 2000).tolist() + [2.0 ** -12 + 2.0 ** -36, 1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24]:
        assert et.round_f32(Fraction(v)) == Fraction(float(np.float32(v))), v


def test_tie_richest_literals_are_the_richest():
    """the thresholds the GPU tests add are those (outside the named ones) with the most f32-wrong pairs"""
    named = set(et.NAMED_THRESHOLDS)
    top = [t for t, _, _ in et.most_wrong_thresholds(12) if t not in named]
    assert tuple(top[:len(et.TIE_RICHEST)]) == et.TIE_RICHEST, top


@pytest.mark.parametrize("t", et.GPU_THRESHOLDS)
def test_restatement_equals_oracle_table(t):
    assert np.array_equal(et.decision_table(t), oracle.edge_table(t)), t
    # the break points: pairs on both sides of every switch along sb, and the table's threshold form
    dec = et.decision_table(t)
    for a, b in et.break_points(t)[::7]:
        assert oracle.edge_decision(a, b, t) == dec[a, b], (t, a, b)
    for a in range(0, et.SUMS, 5):
        row = dec[a].astype(np.int8)
        assert np.count_nonzero(np.diff(row)) <= 2, (t, a)


@pytest.mark.parametrize("t", et.GPU_THRESHOLDS)
def test_every_band_pair_decides_a_centre_in_every_orientation(t):
    band, wrong, blocks, unrealised = et.targets(t)
    assert not unrealised, (t, unrealised[:10])
    want = {(o, a, b) for o in range(4) for a, b in band}
    assert set(blocks) == want
    for key, blk in list(blocks.items())[::max(1, len(blocks) // 200)]:
        sa, sb = et.side_sums(blk)
        assert (sa[key[0]], sb[key[0]]) == key[1:], (t, key)
    for mode in MODES:
        name, w, h, d, sw, kernel, shape, _, _ = et.GEOMETRIES[0]
        lefts, rights = et.batch(w, h, mode, t)
        got, _, _ = et.coverage(lefts, rights, mode, t, kernel, sw // 2, stacked=shape == "stacked")
        missing = want - got
        assert not missing, (t, mode, sorted(missing)[:10])
        assert {(o, a, b) for o in range(4) for a, b in wrong} <= got


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geom", et.GEOMETRIES, ids=[g[0] for g in et.GEOMETRIES])
def test_position_coverage_is_complete(geom, mode):
    name, w, h, d, sw, kernel, shape, _, _ = geom
    stacked = shape == "stacked"
    if kernel == "ext4":
        assert et.edges4_stacked(w, d, sw) == stacked, name
    need = et.reachable_classes(w, h, mode, kernel, sw // 2, stacked=stacked)
    for t in (2.0 / 3.0,):          # the threshold with the most targets: each lands on the fewest positions
        lefts, rights = et.batch(w, h, mode, t)
        _, got, _ = et.coverage(lefts, rights, mode, t, kernel, sw // 2, stacked=stacked)
        assert need <= got, (name, mode, t, sorted(need - got))
    # what each kernel's shape must offer somewhere in the matrix
    if w >= 252 and h >= 9:
        base = {"lane0", "lane63"} | ({f"quad{q}" for q in range(4)} if kernel == "ext4" else set())
        assert base <= need, (name, sorted(base - need))
        if kernel == "ext4":
            assert {f"row{r}" for r in range(4)} <= need
            assert ("wave_seam" if stacked else "interior_wave" if mode == "ghost" else "row0") in need
        assert ({"next_to_border", "sel_wave"} & need) if mode == "ghost" else {"wrap_x", "wrap_y"} <= need
    if name == "ext4_1992_side":
        assert "workgroup_seam" in need
        if mode == "ghost":
            assert {"interior_wave", "sel_wave"} <= need


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("t", [0.0, 1e-9, 0.15, 1.0 / 3.0, 2.0 / 3.0, 1.0, et.TIE_RICHEST[0]])
def test_oracle_equals_restatement_on_the_images(mode, t):
    for geom in (et.GEOMETRIES[0], et.GEOMETRIES[8], et.GEOMETRIES[10]):
        w, h = geom[1], geom[2]
        lefts, rights = et.batch(w, h, mode, t)
        for img in (*lefts[:6], *rights[:6]):
            assert np.array_equal(oracle.find_all_edges(img, t, mode), et.find_all_edges(img, t, mode)), (geom[0], t)


@pytest.mark.parametrize("mode,w,h,t", make_golden.EDGE_TIE_PINNED)
def test_restatement_equals_the_compiled_reference(mode, w, h, t):
    """near-tie images pinned to the reference itself (tests/golden/make_golden.py --pinned)"""
    rec = json.loads((GOLDEN_DIR / "ref_pinned_cases.json").read_text())[make_golden.edge_tie_key(mode, w, h, t)]
    left, right = make_golden.edge_tie_images(mode, w, h, t)
    for k, img in (("edges-1", left), ("edges-2", right)):
        got = et.find_all_edges(img, t, mode)
        r = rec["arrays"][k]
        assert list(got.shape) == r["shape"] and sha256_of(got.astype(r["dtype"])) == r["sha256"], (mode, t, k)
    # and the images are near-tie images: pairs of the band decide centres
    assert len(et.deciding_centres(left, mode, t)) > 50
