"""The bit-sliced match kernel's staging (RowStager, csrc/sm_match_bs_kernel.h) at the corners of its chunked loop.

A workgroup of T threads stages `rows` rows of lw words of the left and rw words of the right packed image; thread t
takes elements t, t + T, ... of each image's rows, CH_L / CH_R of them per chunk with all loads in flight, chunk after
chunk, and in the last chunk a thread without an element repeats element 0.  The shapes below put the element count of
an image below T, at a multiple of T x CH, one above a multiple and well between two, on one- and two-wave workgroups,
at 4, 8 and 16 shifts per lane, with a last tile that is rounded up in both directions, on both borders.

Staging is isolated: random {0,1} edge images go in through sm_load_edges (no threshold arithmetic), sm_match_wta
returns web and best, and both must equal tests/oracle.py's hot_path on the same edge images, exactly.  A word staged
to the wrong place, from the wrong place or not at all changes the window sums of the pixels over it."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from stereomatching_amd import pipeline
from tests import oracle

pytestmark = pytest.mark.gpu

KERNEL_BS = 4           # sm_geometry.kernel of the bit-sliced family
_HEADER = Path(pipeline.__file__).resolve().parent / "csrc" / "sm_match_bs_kernel.h"


def chunk_sizes():
    """(CH_L, CH_R): loads a thread has in flight per chunk, as the kernel header defines them"""
    text = _HEADER.read_text()
    return tuple(int(re.search(rf"^#define {name}\s+(\d+)", text, re.M).group(1))
                 for name in ("SM_STAGE_CH_L", "SM_STAGE_CH_R"))


def staged(geom):
    """(T, rows, lw, rw) of a bit-sliced plan: threads of a workgroup, staged rows and words per staged row of the
    left / right image (match_row_layout and match_configure of csrc/sm_plan_model.h)"""
    nl, ds, waves = geom["shift_lanes"], geom["shifts_per_lane"], geom["waves_per_workgroup"]
    runs = 64 // nl
    assert geom["tile_w"] == 32 * runs
    # (sm_geometry.tile_h is the workgroup's rows: both waves' of a two-wave workgroup)
    return 64 * waves, geom["tile_h"] + geom["window"] - 1, runs + 2, runs + (nl * ds + 31) // 32 + 4


# name: (w, h, D, window, border, pairs, options (tile_h: rows per WAVE), conditions on (T, rows, lw, rw, CH_L, CH_R, geometry))
CASES = {
    # 4 rows of 6 + 10 words: both images have fewer words than the 64 threads
    "fewer_than_threads": (70, 5, 64, 3, "toroidal", 1, dict(shifts_per_lane=4, workgroup_waves=1, tile_h=2),
                           lambda T, rows, lw, rw, cl, cr, g: rows * lw < T and rows * rw < T),
    # 32 shifts, 9 x 9 on a 37-row image, two pairs: 28 rows of 34 + 37 words, both images between two multiples
    # of T x CH
    "between_multiples": (90, 37, 32, 9, "ghost", 2, dict(shifts_per_lane=16, workgroup_waves=2, tile_h=10),
                          lambda T, rows, lw, rw, cl, cr, g: rows * lw % (T * cl) > 1 and rows * rw % (T * cr) > 1),
    # 256 rows of 10 words: whole chunks of the left image exactly -- no chunk may follow the last
    "multiple_of_chunk": (37, 300, 32, 9, "toroidal", 1, dict(shifts_per_lane=4, workgroup_waves=1, tile_h=248),
                          lambda T, rows, lw, rw, cl, cr, g: rows * lw % (T * cl) == 0 and rows * lw > T * cl),
    # 197 rows of 13 words: ONE word of the right image above whole chunks -- a last chunk in which one thread
    # has one element
    "one_above_multiple": (37, 200, 32, 9, "toroidal", 1, dict(shifts_per_lane=4, workgroup_waves=1, tile_h=189),
                           lambda T, rows, lw, rw, cl, cr, g: rows * rw % (T * cr) == 1 and rows * rw > T * cr),
    # ... and of the left image, whose rows have an even number of words in this layout, two: 77 rows of 10
    "two_above_multiple": (37, 100, 32, 9, "ghost", 1, dict(shifts_per_lane=4, workgroup_waves=1, tile_h=69),
                           lambda T, rows, lw, rw, cl, cr, g: rows * lw % (T * cl) == 2 and rows * lw > T * cl),
    # 21 x 21 on a 64-thread workgroup: 32 rows of 10 + 14 words, two chunks of each image
    "window21_one_wave": (100, 50, 64, 21, "ghost", 1, dict(shifts_per_lane=8, workgroup_waves=1, tile_h=12),
                          lambda T, rows, lw, rw, cl, cr, g: T == 64 and rows * lw > T * cl and rows * rw > T * cr),
    # the flagship's layout (128 shifts, 9 x 9, two waves, 10 + 16 words) on a taller tile: 68 rows, two chunks of
    # each; two tiles across (the second starts at word 8 of a row) and a last tile of 10 of 60 rows
    "two_waves_two_chunks": (260, 70, 128, 9, "toroidal", 2, dict(shifts_per_lane=16, workgroup_waves=2, tile_h=30),
                             lambda T, rows, lw, rw, cl, cr, g: T == 128 and rows * lw > T * cl and rows * rw > T * cr
                             and g["tiles_x"] == 2 and g["tiles_y"] == 2),
    # 8 shifts per lane on two waves, one partial chunk of each image
    "eight_shifts_two_waves": (130, 45, 64, 7, "ghost", 1, dict(shifts_per_lane=8, workgroup_waves=2, tile_h=8),
                               lambda T, rows, lw, rw, cl, cr, g: T == 128 and T < rows * lw < T * cl),
}


def edge_images(pairs, h, w, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((pairs, h, w)) < 0.3).astype(np.uint8), (rng.random((pairs, h, w)) < 0.3).astype(np.uint8)


@pytest.mark.parametrize("name", list(CASES))
def test_staged_tiles_match_the_oracle(name):
    w, h, D, n, border, pairs, options, holds = CASES[name]
    le, re_ = edge_images(pairs, h, w, seed=len(name) + w)
    plan = pipeline.StereoPlan(w, h, D, n, border, max_pairs=pairs, options=options)
    try:
        g = plan.geometry()
        assert g["kernel"] == KERNEL_BS, plan.describe()
        assert g["shifts_per_lane"] == options["shifts_per_lane"], plan.describe()
        assert g["waves_per_workgroup"] == options["workgroup_waves"], plan.describe()
        assert g["tile_h"] == options["workgroup_waves"] * options["tile_h"], plan.describe()
        # a rounded-up last tile in both directions
        assert w % 32 and h % g["tile_h"], plan.describe()
        T, rows, lw, rw = staged(g)
        cl, cr = chunk_sizes()
        print(f"{name}: T {T}, {rows} rows of {lw} + {rw} words = {rows * lw} + {rows * rw}; chunks of {T * cl} + {T * cr}")
        assert holds(T, rows, lw, rw, cl, cr, g), (plan.describe(), T, rows, lw, rw, cl, cr)
        plan.load_edges(torch.from_numpy(le).cuda(), torch.from_numpy(re_).cuda())
        web, best = plan.match_wta(pairs, want_best=True)
        torch.cuda.synchronize()
        web, best = web.cpu().numpy(), best.cpu().numpy()
    finally:
        plan.close()
    for q in range(pairs):
        want_best, want_web = oracle.hot_path(le[q], re_[q], D, n, border)
        assert np.array_equal(web[q], want_web), f"{name}: web of pair {q} differs at {np.argwhere(web[q] != want_web)[:5]}"
        assert np.array_equal(best[q], want_best), f"{name}: best of pair {q} differs at {np.argwhere(best[q] != want_best)[:5]}"
