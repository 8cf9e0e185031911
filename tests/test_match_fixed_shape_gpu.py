"""The two forms of the bit-sliced match kernel's output path (csrc/sm_match_bs_kernel.h: `fixed`, FX).

A workgroup of a two-wave build of 16 shifts per lane with the full shift range takes the FIXED-SHAPE form -- lanes
merged through LDS, 8 lanes per word, int32 maps stored 16 bytes at a time, nothing asked about the image's size --
when its tile lies wholly inside the image and the launch is such a one; every other workgroup and every other
launch takes the generic form.  The shapes below are two whole tiles and a partial one wide and one whole workgroup
tile and a partial one (or more) high, so ONE launch holds workgroups of both forms, and the generic-only launches
(narrow maps, D short of the lanes' shifts, D = 64 merged with DPP, the 13 x 13 and 15 x 15 builds of 8 shifts per
lane) run on the same shapes.  Rows per wave of 5, 6 and 7 leave a last merge batch of 1, 2 and 3 rows, in the
interior tiles (fixed form) and the right-border tiles (generic form) alike.  All five windows whose builds carry the
fixed form (3 x 3 ... 11 x 11) have a case with both forms in one launch.

Every case runs a batch of two pairs -- i.i.d. edges, and both images 0, where every shift ties and the last must
win -- and a batch of one pair in which no shift ever matches (web = D, best = 0, in interior and border tiles).
web, and best where it is asked for, must equal tests/oracle.py's hot_path exactly."""
import numpy as np
import pytest
import torch

from stereomatching_amd import pipeline
from tests import oracle
from tests.extreme_patterns import edge_pattern

pytestmark = pytest.mark.gpu

KERNEL_BS = 4           # sm_geometry.kernel of the bit-sliced family

I32, U16, U8 = torch.int32, torch.uint16, torch.uint8
# (w, h, D, window, border, web type, best wanted, shifts per lane, rows per wave, workgroups in the fixed form)
CASES = {
    # the flagship's layout and tile: 256 x 32 pixels per workgroup
    "fixed-9-toroidal-544x40-best": (544, 40, 128, 9, "toroidal", I32, True, 16, 16, True),
    "fixed-9-ghost-800x72": (800, 72, 128, 9, "ghost", I32, False, 16, 16, True),
    # last merge batch of 1, 2, 3 rows
    "fixed-5-toroidal-last1-best": (544, 23, 128, 5, "toroidal", I32, True, 16, 5, True),
    "fixed-9-ghost-last2-best": (544, 29, 128, 9, "ghost", I32, True, 16, 6, True),
    "fixed-5-ghost-last3": (544, 37, 128, 5, "ghost", I32, False, 16, 7, True),
    # the other windows whose builds carry the fixed form: 3 x 3, 7 x 7 and 11 x 11 (the build with the fewest registers
    # to spare), each with a short last batch
    "fixed-11-ghost-last3-best": (544, 37, 128, 11, "ghost", I32, True, 16, 7, True),
    "fixed-11-toroidal-last1": (800, 23, 128, 11, "toroidal", I32, False, 16, 5, True),
    "fixed-7-toroidal-last2-best": (544, 29, 128, 7, "toroidal", I32, True, 16, 6, True),
    "fixed-3-ghost-last2": (544, 29, 128, 3, "ghost", I32, False, 16, 6, True),
    # narrow maps: no workgroup may take the fixed form, whose stores are int32
    "generic-9-toroidal-u16-best": (544, 40, 128, 9, "toroidal", U16, True, 16, 16, False),
    "generic-5-ghost-u8-last1": (544, 23, 128, 5, "ghost", U8, False, 16, 5, False),
    # D = 100: 8 lanes per word merged through LDS, the last lane's shifts end early
    "generic-9-toroidal-d100-last2-best": (544, 29, 100, 9, "toroidal", I32, True, 16, 6, False),
    "generic-9-ghost-d100-u16-last3": (544, 37, 100, 9, "ghost", U16, False, 16, 7, False),
    "generic-5-toroidal-d100-last1": (544, 23, 100, 5, "toroidal", I32, False, 16, 5, False),
    # D = 64: 4 lanes per word, merged per row with DPP (512 pixels per tile)
    "generic-5-ghost-d64-best": (1056, 40, 64, 5, "ghost", I32, True, 16, 16, False),
    # 13 x 13 (shared warm-up rows in one counter) and 15 x 15 (row by row): 8 shifts per lane, 128 pixels per tile
    "generic-13-toroidal-best": (300, 20, 128, 13, "toroidal", I32, True, 8, 3, False),
    "generic-15-ghost-best": (300, 20, 128, 15, "ghost", I32, True, 8, 3, False),
}


def batches(w, h, n, D, seed):
    """-> [(names, eL stack, eR stack)]: a batch of two pairs and a batch of one"""
    rng = np.random.default_rng([seed, w, h, n, D])
    rnd = ((rng.random((h, w)) < 0.3).astype(np.uint8), (rng.random((h, w)) < 0.3).astype(np.uint8))
    tie = edge_pattern("all_match_0", w, h, n, D)
    none = edge_pattern("no_centre_match", w, h, n, D)
    return [(("random", "all_tie"), np.stack([rnd[0], tie[0]]), np.stack([rnd[1], tie[1]])),
            (("no_shift_matched",), none[0][None].copy(), none[1][None].copy())]


@pytest.mark.parametrize("name", list(CASES))
def test_both_output_forms_match_the_oracle(name):
    w, h, D, n, border, web_dtype, want_best, ds, th, has_fixed = CASES[name]
    options = dict(shifts_per_lane=ds, workgroup_waves=2, tile_h=th)
    for names, le, re_ in batches(w, h, n, D, seed=len(name)):
        pairs = len(names)
        plan = pipeline.StereoPlan(w, h, D, n, border, max_pairs=pairs, options=options)
        try:
            g = plan.geometry()
            assert g["kernel"] == KERNEL_BS, plan.describe()
            assert g["shifts_per_lane"] == ds and g["waves_per_workgroup"] == 2, plan.describe()
            assert g["tile_h"] == 2 * th, plan.describe()
            # whole tiles and a partial one in both directions: the launch cannot miss either form
            assert g["tiles_x"] >= 3 and g["tiles_y"] >= 2, plan.describe()
            assert w % g["tile_w"] and h % g["tile_h"], plan.describe()
            assert w >= 2 * g["tile_w"] and h >= g["tile_h"], plan.describe()
            if has_fixed:
                # what the kernel asks of a launch before it looks at the tile
                assert ds == 16 and g["shift_lanes"] == 8 and D == 128 and g["lane_merge_lds"], plan.describe()
                assert web_dtype == I32 and w % 4 == 0, plan.describe()
            plan.load_edges(torch.from_numpy(le).cuda(), torch.from_numpy(re_).cuda())
            web, best = plan.match_wta(pairs, want_best=want_best, web_dtype=web_dtype)
            torch.cuda.synchronize()
            assert web.dtype == web_dtype
            web = web.to(torch.int32).cpu().numpy()
            best = best.cpu().numpy() if want_best else None
        finally:
            plan.close()
        for q, pattern in enumerate(names):
            want_b, want_w = oracle.hot_path(le[q], re_[q], D, n, border)
            where = f"{name}, {pattern}"
            if pattern == "all_tie":
                assert (want_w == D).all() and (want_b > 0).all(), where
            if pattern == "no_shift_matched":
                assert (want_w == D).all() and (want_b == 0).all(), where
            assert np.array_equal(web[q], want_w), \
                f"{where}: web differs at {np.argwhere(web[q] != want_w)[:5]}"
            if want_best:
                assert np.array_equal(best[q], want_b), \
                    f"{where}: best differs at {np.argwhere(best[q] != want_b)[:5]}: " \
                    f"{best[q][best[q] != want_b][:5]} for {want_b[best[q] != want_b][:5]}"
