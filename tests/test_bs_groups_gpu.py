"""The grouped inputs of k_match_bs's row network (csrc/sm_bs_network.h: of every three window columns of a row the
network takes two mismatch bits and the parity LX ^ RX of the three) against the CPU oracle, bit for bit, at the
smallest shapes at which the grouping can go wrong:

  * 320 x 40, 128 shifts, 9 x 9 toroidal, two-wave workgroups of 2 x 8 rows: two tile columns (256 + 64 pixels), RX
    values reused by all four groups of four shifts of a lane, a workgroup whose second wave has no rows left;
  * 96 x 24 at 16 and 64 shifts with 3 x 3, 5 x 5, 7 x 7 and 11 x 11 (N mod 3 = 0, 2, 1, 2: no, two, one, two single
    columns beside the groups), 16 and 8 shifts per lane, one- and two-wave workgroups.  (The kernel groups where that
    saves operations: 7 x 7 and 11 x 11 here.  3 x 3 and 5 x 5, one group per row side, keep the per-bit inputs and
    are the same cases run through the other path of the same code.)
  * one ghost case, 96 x 24 with 9 x 9: the ghost kernels keep their per-column inputs, so the maps must equal the
    oracle AND, bit for bit, what the library computed before the grouping (tests/golden/bs_groups/ghost_parent.npz,
    recorded on an MI355X from the parent commit's build with record_ghost_fixture() below).

The pairs of one batch: random edge maps at densities 0.5 and 0.1, and from tests/extreme_patterns.py the all-ones and
all-zero images, ones against zeros (every tap differs), row bands, column bands and the column checkerboard.  The
oracle's maps are computed once per geometry."""
import numpy as np
import pytest
import torch

from tests import oracle
from tests.conftest import GOLDEN_DIR
from tests.extreme_patterns import edge_pattern, gray_pattern
from tests.test_hip_gpu import ONE_WAVE, TWO_WAVES, poisoned

INPUTS = ("random_0.5", "random_0.1", "all_match_1", "all_match_0", "no_centre_match", "row_bands", "col_bands",
          "checkerboard")
GHOST_FIXTURE = GOLDEN_DIR / "bs_groups" / "ghost_parent.npz"
GHOST_CASE = dict(w=96, h=24, d=64, n=9)

_cache = {}


def edges(kind, w, h, n, d):
    if kind.startswith("random_"):
        rng = np.random.default_rng([w, h, n, d, INPUTS.index(kind)])
        dens = float(kind.split("_")[1])
        return (rng.random((h, w)) < dens).astype(np.uint8), (rng.random((h, w)) < dens).astype(np.uint8)
    if kind == "checkerboard":
        cols = gray_pattern("checker_2", w, h)[0] // 255        # columns 0 1 0 1 ...
        rows = (np.arange(h) & 1).astype(np.uint8)[:, None]
        return (cols ^ rows).astype(np.uint8), cols.astype(np.uint8)
    return edge_pattern(kind, w, h, n, d)


def batch(w, h, d, n, mode):
    """-> (eL, eR, oracle best, oracle web), one pair per input kind; computed once"""
    key = (w, h, d, n, mode)
    if key not in _cache:
        pairs = [edges(kind, w, h, n, d) for kind in INPUTS]
        res = [oracle.hot_path(le, re, d, n, mode) for le, re in pairs]
        _cache[key] = (np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]),
                       np.stack([r[0] for r in res]), np.stack([r[1] for r in res]))
    return _cache[key]


def run(hip, w, h, d, n, mode, opts):
    """-> (web, best, description) of one match launch over the batch"""
    le, re, _, _ = batch(w, h, d, n, mode)
    plan = hip.StereoPlan(w, h, d, n, mode, max_pairs=len(INPUTS), options=opts)
    plan.load_edges(torch.from_numpy(le).cuda(), torch.from_numpy(re).cuda())
    web, best = plan.match_wta(len(INPUTS), want_best=True, web=poisoned(len(INPUTS), h, w),
                               best=poisoned(len(INPUTS), h, w))
    torch.cuda.synchronize()
    desc = plan.describe()
    plan.close()
    return web.cpu().numpy(), best.cpu().numpy(), desc


def differences(got_web, got_best, want_web, want_best, desc):
    bad = []
    for i, kind in enumerate(INPUTS):
        for what, got, want in (("web", got_web[i], want_web[i]), ("best", got_best[i], want_best[i])):
            diff = np.argwhere(got != want)
            if len(diff):
                y, x = diff[0]
                bad.append(f"{kind}: {what} differs at {len(diff)} px, first (y={y}, x={x}): {got[y, x]} != {want[y, x]}"
                           f"  [{desc}]")
    return bad


def test_the_inputs_reach_both_parities_of_a_group():
    """no GPU: in the random pairs every group of three columns of a window row meets 0, 1, 2 and 3 mismatches (both
    parities, with the carry set and clear), and the uniform pairs hold every group at 0 and at 3"""
    w, h, d, n = 96, 24, 16, 9
    le, re, _, _ = batch(w, h, d, n, "toroidal")
    x = (le[0] ^ np.roll(re[0], -3, axis=1)).astype(np.int64)
    per_group = x + np.roll(x, -1, axis=1) + np.roll(x, -2, axis=1)
    assert set(np.unique(per_group)) == {0, 1, 2, 3}
    assert not (le[2] ^ re[2]).any() and not (le[3] ^ re[3]).any() and (le[4] ^ re[4]).all()


@pytest.mark.gpu
def test_two_tile_columns_two_waves_all_shift_groups(hip):
    w, h, d, n = 320, 40, 128, 9
    _, _, ob, ow = batch(w, h, d, n, "toroidal")
    web, best, desc = run(hip, w, h, d, n, "toroidal", dict(TWO_WAVES, shifts_per_lane=16, tile_h=8))
    assert "lanes of 16)" in desc and "two-wave workgroups" in desc, desc
    bad = differences(web, best, ow, ob, desc)
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["one_wave", "two_waves"])
@pytest.mark.parametrize("ds", [16, 8])
@pytest.mark.parametrize("d", [16, 64])
@pytest.mark.parametrize("n", [3, 5, 7, 11])
def test_groups_and_single_columns(hip, n, d, ds, shape):
    w, h = 96, 24
    _, _, ob, ow = batch(w, h, d, n, "toroidal")
    opts = dict(ONE_WAVE if shape == "one_wave" else TWO_WAVES, shifts_per_lane=ds, tile_h=6)
    web, best, desc = run(hip, w, h, d, n, "toroidal", opts)
    assert f"lanes of {ds})" in desc, desc
    assert ("two-wave workgroups" in desc) == (shape == "two_waves"), desc
    bad = differences(web, best, ow, ob, desc)
    assert not bad, "\n".join(bad)


def ghost_maps(hip):
    c = GHOST_CASE
    return run(hip, c["w"], c["h"], c["d"], c["n"], "ghost", dict(TWO_WAVES, shifts_per_lane=16, tile_h=6))


def record_ghost_fixture(hip, path=GHOST_FIXTURE):
    """writes the fixture of test_ghost_equals_oracle_and_parent: run with the PARENT's library loaded"""
    c = GHOST_CASE
    le, re, _, _ = batch(c["w"], c["h"], c["d"], c["n"], "ghost")
    web, best, desc = ghost_maps(hip)
    path.parent.mkdir(exist_ok=True)
    np.savez_compressed(path, left=le, right=re, web=web, best=best)
    return desc


@pytest.mark.gpu
def test_ghost_equals_oracle_and_parent(hip):
    c = GHOST_CASE
    le, re, ob, ow = batch(c["w"], c["h"], c["d"], c["n"], "ghost")
    z = np.load(GHOST_FIXTURE)
    assert np.array_equal(z["left"], le) and np.array_equal(z["right"], re), "the fixture was recorded from other inputs"
    web, best, desc = ghost_maps(hip)
    assert "lanes of 16)" in desc and "two-wave workgroups" in desc, desc
    bad = differences(web, best, ow, ob, desc)
    assert not bad, "\n".join(bad)
    assert web.dtype == z["web"].dtype and best.dtype == z["best"].dtype
    assert web.tobytes() == z["web"].tobytes() and best.tobytes() == z["best"].tobytes(), "ghost maps moved"
