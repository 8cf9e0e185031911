"""The steady-state row step of k_match_bs -- S += (entering row) - (leaving row) through the signed carry-save
network of csrc/sm_bs_network.h -- against the CPU oracle, bit for bit, at the smallest shapes at which the row step
can still go wrong.

Every window x shifts per lane the bit-sliced family instantiates, both borders, one-wave and two-wave workgroups,
D in {16, 64, 128} (and 8 where 8 or 4 shifts per lane apply), image widths 64 and 70 (not a multiple of 32), heights
N + 1 (warm-up and ONE steady row) and 2 * tile_h + 3 (the seam between the two waves of a workgroup and a tile
boundary are crossed).  The inputs of one geometry are the pairs of one batch: random edges at densities 0.5 and 0.02,
two equal images (every shift ties, the sums stay 0) and two complementary ones (every tap differs: with the toroidal
border the sums stay N^2) -- the last two pin both ends of the sum planes.  The oracle's maps are computed once per
(input, geometry) and shared by the kernels that must reproduce them."""
import numpy as np
import pytest
import torch

from tests import oracle
from tests.test_hip_gpu import BUILT_BS, ONE_WAVE, TWO_WAVES, poisoned

INPUTS = ("random_0.5", "random_0.02", "equal", "complementary")
WIDTHS = (64, 70)

_oracle_cache = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def edges(kind, w, h, seed):
    rng = np.random.default_rng(seed)
    if kind.startswith("random_"):
        dens = float(kind.split("_")[1])
        return (rng.random((h, w)) < dens).astype(np.uint8), (rng.random((h, w)) < dens).astype(np.uint8)
    if kind == "equal":
        return np.ones((h, w), np.uint8), np.ones((h, w), np.uint8)
    return np.ones((h, w), np.uint8), np.zeros((h, w), np.uint8)


def batch(w, h, d, n, mode):
    """-> (eL, eR, oracle best, oracle web), one pair per input kind; the oracle cached"""
    key = (w, h, d, n, mode)
    if key not in _oracle_cache:
        pairs = [edges(kind, w, h, seed=1000 * n + 10 * h + i) for i, kind in enumerate(INPUTS)]
        res = [oracle.hot_path(le, re, d, n, mode) for le, re in pairs]
        _oracle_cache[key] = (np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]),
                              np.stack([r[0] for r in res]), np.stack([r[1] for r in res]))
    return _oracle_cache[key]


def shift_counts(ds):
    return (16, 64, 128) if ds == 16 else (8, 16, 64, 128)


def test_the_pinning_inputs_pin_the_planes():
    """no GPU: with equal images every window sum is 0 (best = all taps), with complementary ones and the toroidal
    border it is N^2 at every shift, so nothing matches at the centre and the maps hold the "no match" values"""
    n, d, w, h = 9, 16, 64, 11
    _, _, ob, ow = batch(w, h, d, n, "toroidal")
    assert (ob[INPUTS.index("equal")] == n * n).all() and (ow[INPUTS.index("equal")] == d).all()
    assert (ob[INPUTS.index("complementary")] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
@pytest.mark.parametrize("shape", ["one_wave", "two_waves"])
@pytest.mark.parametrize("n,ds", BUILT_BS)
def test_row_step_matches_oracle(hip, n, ds, shape, mode):
    tile_h = max(4, n // 2)
    opts = dict(ONE_WAVE if shape == "one_wave" else TWO_WAVES, shifts_per_lane=ds, tile_h=tile_h)
    bad = []
    for d in shift_counts(ds):
        for w in WIDTHS:
            for h in (n + 1, 2 * tile_h + 3):
                le, re, ob, ow = batch(w, h, d, n, mode)
                plan = hip.StereoPlan(w, h, d, n, mode, max_pairs=len(INPUTS), options=opts)
                plan.load_edges(dev(le), dev(re))
                web, best = plan.match_wta(len(INPUTS), want_best=True, web=poisoned(len(INPUTS), h, w),
                                           best=poisoned(len(INPUTS), h, w))
                torch.cuda.synchronize()
                desc = plan.describe()
                plan.close()
                assert f"lanes of {ds})" in desc, desc
                assert ("two-wave workgroups" in desc) == (shape == "two_waves"), desc
                web, best = web.cpu().numpy(), best.cpu().numpy()
                for i, kind in enumerate(INPUTS):
                    for what, got, want in (("web", web[i], ow[i]), ("best", best[i], ob[i])):
                        diff = np.argwhere(got != want)
                        if len(diff):
                            y, x = diff[0]
                            bad.append(f"D={d} {w}x{h} {kind}: {what} differs at {len(diff)} px, first (y={y}, x={x}): "
                                       f"{got[y, x]} != {want[y, x]}  [{desc}]")
    assert not bad, "\n".join(bad[:20])
