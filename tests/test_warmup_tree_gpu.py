"""The shared warm-up of the bit-sliced match kernel's two-wave workgroups (csrc/sm_match_bs_kernel.h, WT): each wave
counts its half of the shared window rows in one carry-save counter per shift, the waves swap the partial sums on
TB planes and add them to totals of SB planes.

Every two-wave build whose waves share at least two rows (5 x 5 and up; the largest windows keep the row-by-row
warm-up and go through the same checks) is run at 16, 8 and 4 shifts per lane on both borders, forced through
sm_plan_options onto the smallest tiles -- two to four rows per wave, one tile across an image 69 .. 85 pixels wide --
with the images of tests/warmup_patterns.py as the pairs of one batch: no mismatch, ONE mismatching tap at every
position of the shared rows of either half, all taps but the centre mismatching, and i.i.d. images.  Each case
runs two plans:

  * D = twice the lane's shifts on an image one row ABOVE a multiple of the workgroup's height, where the last
    workgroup's wave 1 has no output row and must still stand behind both barriers of the exchange;
  * D three short of that (the last lane's shifts end early: the kernels built for any D) on an image one row
    BELOW a multiple.

web AND best must equal tests/oracle.py's hot_path exactly: best shows a wrong sum where web can hide it."""
import numpy as np
import pytest
import torch

from stereomatching_amd import pipeline
from tests import oracle
from tests.warmup_patterns import warmup_batch

pytestmark = pytest.mark.gpu

KERNEL_BS = 4           # sm_geometry.kernel of the bit-sliced family
# windows of the two-wave builds by shifts per lane (csrc/sm_match_bs_duo.hip, _duo8.hip, _ds4.hip), HALF >= 2
WINDOWS = {16: (5, 7, 9, 11), 8: (5, 7, 9, 11, 13, 15, 17, 19, 21), 4: (5, 7, 9, 11, 13, 15, 17, 19, 21)}
CASES = [(ds, n, border) for ds in (16, 8, 4) for n in WINDOWS[ds] for border in ("toroidal", "ghost")]


def rows_per_wave(n):
    return 2 + (n // 2) % 3         # 2, 3 or 4


def heights(n):
    """one row above and one row below a multiple of the workgroup's 2 * rows_per_wave rows, both at least the
    window and a workgroup tall"""
    wg = 2 * rows_per_wave(n)
    k = (n + wg) // wg + 1
    return k * wg + 1, (k + 1) * wg - 1


def run_plan(w, h, D, n, border, options):
    names, le, re_ = warmup_batch(w, h, n, D)
    pairs = len(names)
    plan = pipeline.StereoPlan(w, h, D, n, border, max_pairs=pairs, options=options)
    try:
        g = plan.geometry()
        assert g["kernel"] == KERNEL_BS, plan.describe()
        assert g["shifts_per_lane"] == options["shifts_per_lane"], plan.describe()
        assert g["waves_per_workgroup"] == 2, plan.describe()
        assert g["tile_h"] == 2 * options["tile_h"], plan.describe()
        assert g["tiles_y"] >= 2 and h % g["tile_h"], plan.describe()
        plan.load_edges(torch.from_numpy(le).cuda(), torch.from_numpy(re_).cuda())
        web, best = plan.match_wta(pairs, want_best=True)
        torch.cuda.synchronize()
        web, best = web.cpu().numpy(), best.cpu().numpy()
    finally:
        plan.close()
    return g, names, le, re_, web, best


@pytest.mark.parametrize("ds,n,border", CASES, ids=[f"ds{ds}-{n}x{n}-{b}" for ds, n, b in CASES])
def test_shared_warmup_matches_the_oracle(ds, n, border):
    w = 64 + n
    th = rows_per_wave(n)
    h_above, h_below = heights(n)
    for h, D in ((h_above, 2 * ds), (h_below, 2 * ds - 3)):
        g, names, le, re_, web, best = run_plan(w, h, D, n, border,
                                                dict(shifts_per_lane=ds, workgroup_waves=2, tile_h=th))
        wg = g["tile_h"]
        if h == h_above:
            # the last workgroup has one row: its wave 1 has none
            assert h % wg == 1 and h % wg <= th
        else:
            assert h % wg == wg - 1
        for q, name in enumerate(names):
            want_best, want_web = oracle.hot_path(le[q], re_[q], D, n, border)
            if name.startswith("one_tap") and border == "toroidal":
                # the pattern does what it is named after: one mismatch at every shift around each point
                assert (want_best == n * n - 1).sum() == (n * n - 1) * int(le[q].sum()), name
            if name.startswith("all_but_centre") and border == "toroidal":
                assert (want_best == 1).sum() == int((1 - le[q]).sum()) and (want_best > 1).sum() == 0, name
            where = f"{n}x{n} {border} ds {ds} D {D} h {h}, {name}"
            assert np.array_equal(best[q], want_best), \
                f"{where}: best differs at {np.argwhere(best[q] != want_best)[:5]}: " \
                f"{best[q][best[q] != want_best][:5]} for {want_best[best[q] != want_best][:5]}"
            assert np.array_equal(web[q], want_web), f"{where}: web differs at {np.argwhere(web[q] != want_web)[:5]}"
