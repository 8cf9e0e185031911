"""Loops that every other test leaves after one turn, at the smallest sizes that take them further.

  - k_itp_rowscan scans a row's chunk carries 64 chunks a turn, left to right and back, a carry going from turn to turn:
    widths of 65 and 129 chunks, and the transposed shape for the 129 segment carries of a column.
  - k_reproject, k_lr_check and the other kernels that stride over a map with at most 1024 workgroups: sizes that want
    more, on the one-pixel and on the four-pixel path.
  - k_lr_zero_counts and k_step3_init launch a workgroup per 64 pairs: batches of 65 and 130 pairs through every call that
    zeroes or initialises a per-pair value, each count buffer holding something else before the call.

Every expected value comes from the CPU definitions (tests/*_reference.py, tests/oracle.py), none from the HIP path, and
every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

from stereomatching_amd import capi
from stereomatching_amd.capi import lib
from tests import cost_lr_reference as clr
from tests import filter_reference as fr
from tests import interp_reference as ir
from tests import lr_reference as lr
from tests import oracle
from tests import reproject_patterns as pp
from tests import reproject_reference as ref
from tests import wmedian_reference as wr
from tests.test_reproject_gpu import check_cloud, check_dense
from tests.test_write_bounds_gpu import P, stream

pytestmark = pytest.mark.gpu
DTYPES = [np.int32, np.int16]
TYPE = {np.int32: capi.SM_MAP_I32, np.int16: capi.SM_MAP_I16}
CW = 64                     # pixels of a row chunk (a lane of k_itp_rowscan), rows of a column segment
TURN = 64 * CW              # columns that one turn of the row scan covers
STRIDE_BLOCKS = 1024        # workgroups per pair above which the striding kernels go round again
COUNT_FILL = 0x5A5A5A5A     # what a count buffer holds before the call


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------------------
# a. the row scan's second and third turn
# ---------------------------------------------------------------------------

def scan_rows(w, dtype, seed=0):
    """[2][3][w]: six rows whose valid pixels force the left and the right candidate of the others across the borders
    between the scan's turns.  Every valid pixel holds a value of its own (a permutation of 1 .. 3 w, which an int16
    holds at these widths), so that the definition's output says where each filled pixel got its value from."""
    chunks = (w + CW - 1) // CW
    assert chunks > 64 and 3 * w <= 32767
    rng = np.random.default_rng(seed + w)
    valid = np.zeros((2, 3, w), bool)
    valid[0, 0, 5] = True                                       # the only valid pixel in chunk 0
    valid[0, 1, w - 1 - (w - 1) % CW // 2] = True               # ... in the last chunk
    valid[0, 2, TURN + (min(w, TURN + CW) - TURN) // 2] = True  # ... in chunk 64
    #     [1, 0]: all pixels invalid
    near, over = TURN - CW + 9, TURN + min(2, w - 1 - TURN)      # valid pixels only in chunks 63 and 64
    valid[1, 1, near] = valid[1, 1, over] = True
    valid[1, 2] = rng.random(w) < 0.01                          # a random row with 99 % invalid pixels
    ids = np.stack([rng.permutation(3 * w).reshape(3, w) + 1 for _ in range(2)])
    if ids[1, 1, over] > ids[1, 1, near]:                       # the pixels between the two take the lower value where
        ids[1, 1, [near, over]] = ids[1, 1, [over, near]]       # they have no third candidate: the one from chunk 64
    return np.where(valid, ids, 0).astype(dtype)


def scan_classes(w, seed=0):
    """a class map with both kinds of invalid pixel (1: the second lowest candidate; else the lower median)"""
    return (np.random.default_rng(seed + 3 * w).random((2, 3, w)) < 0.5).astype(np.uint8)


def widest_horizontal_reach(a, want):
    """(columns, turns crossed to the right, to the left): over the filled pixels of one map [H][W] whose value stands
    in their own row of the input -- every input value is unique, so that is where it came from -- the largest
    distance in columns, and whether some value crossed a border between two turns of the row scan in each direction"""
    pos = {int(v): (y, x) for (y, x), v in np.ndenumerate(a) if v}
    assert len(pos) == int((a != 0).sum()), "the input values are not unique"
    far, right, left = 0, False, False
    for y, x in np.argwhere((a == 0) & (want != 0)):
        sy, sx = pos[int(want[y, x])]
        if sy != y:
            continue
        far = max(far, abs(int(sx) - int(x)))
        right |= sx // TURN < x // TURN
        left |= sx // TURN > x // TURN
    return far, right, left


@pytest.fixture(scope="module")
def scan_cases():
    """(w, dtype, with class map) -> (maps, cls or None, expected maps), computed once by the definition"""
    cases = {}
    for w in (TURN + 1, 8200):
        for dtype in DTYPES:
            a = scan_rows(w, dtype)
            for with_cls in (False, True):
                cls = scan_classes(w) if with_cls else None
                want = np.stack([ir.interpolate(a[q], None if cls is None else cls[q]) for q in range(2)])
                cases[w, dtype, with_cls] = (a, cls, want)
    return cases


@pytest.mark.parametrize("with_cls", [False, True], ids=["median", "classes"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["i32", "i16"])
@pytest.mark.parametrize("w", [TURN + 1, 8200])
def test_row_scan_carries_cross_its_turns(hip, scan_cases, w, dtype, with_cls):
    """W = 4097 is 65 chunks (a second turn with one chunk in it), W = 8200 is 129 (three turns).  The assertions on the
    definition come first: in each map some filled pixel takes its value from its own row across a border between two
    turns of the scan, over the two maps in both directions, and at W = 8200 in each map from more than 4096 columns
    away (no two pixels of a row of 4097 are further apart than 4096: there one map has that pair), so neither the
    input nor an all-zero map can pass."""
    a, cls, want = scan_cases[w, dtype, with_cls]
    reach = [widest_horizontal_reach(a[q], want[q]) for q in range(2)]
    for q, (far, right, left) in enumerate(reach):
        assert right or left, (w, q, far)
        assert far > TURN or w == TURN + 1, (w, q, far)
        assert not np.array_equal(want[q], a[q]) and want[q].any()
    assert any(r for _, r, _ in reach) and any(l for _, _, l in reach) and max(f for f, _, _ in reach) >= TURN
    plan = hip.StereoPlan(w, 3, 4, 1, "ghost", max_pairs=2)
    try:
        got, filled = plan.interpolate(dev(a), None if cls is None else dev(cls), want_filled=True)
        got, filled = host(got), host(filled)
        for q in range(2):
            assert np.array_equal(got[q], want[q]), (w, q, np.argwhere(got[q] != want[q])[:4].tolist())
            assert int(filled[q]) == ir.filled(a[q], want[q]), (w, q)
    finally:
        plan.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=["i32", "i16"])
def test_column_carries_over_129_segments(hip, scan_cases, dtype):
    """The transposed shape, 3 x 8200: the same valid pixels now send their values down and up the columns, through the
    carries of 129 segments of 64 rows.  The definition treats rows and columns alike (its eight directions and the
    order statistics of the candidates are unchanged by exchanging x and y), so what it gives for the transposed map is
    the transpose of what it gives for the map; the first assertion pins that on a small map."""
    rng = np.random.default_rng(5)
    small = np.where(rng.random((9, 40)) < 0.2, rng.integers(1, 90, (9, 40)), 0).astype(dtype)
    small_cls = (rng.random((9, 40)) < 0.5).astype(np.uint8)
    assert np.array_equal(ir.interpolate(small.T, small_cls.T), ir.interpolate(small, small_cls).T)
    assert np.array_equal(ir.interpolate(small.T), ir.interpolate(small).T)
    h = 8200
    plan = hip.StereoPlan(3, h, 4, 1, "ghost", max_pairs=2)
    try:
        for with_cls in (False, True):
            a, cls, want = scan_cases[h, dtype, with_cls]
            at, wt = np.ascontiguousarray(a.transpose(0, 2, 1)), want.transpose(0, 2, 1)
            ct = None if cls is None else dev(cls.transpose(0, 2, 1))
            got, filled = plan.interpolate(dev(at), ct, want_filled=True)
            got, filled = host(got), host(filled)
            for q in range(2):
                assert np.array_equal(got[q], wt[q]), (with_cls, q, np.argwhere(got[q] != wt[q])[:4].tolist())
                assert int(filled[q]) == ir.filled(at[q], wt[q]), (with_cls, q)
    finally:
        plan.close()


# ---------------------------------------------------------------------------
# b. reprojection at sizes whose workgroups stride
# ---------------------------------------------------------------------------

# (w, h, pixels a lane): 1029 x 256 is odd, so a lane takes one pixel: 1029 workgroups wanted, 1024 launched;
# 1028 x 1024 takes the four-pixel path: 263168 lanes, 1028 workgroups wanted
STRIDING_SIZES = [(1029, 256, 1), (1028, 1024, 4)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["i32", "i16"])
@pytest.mark.parametrize("w,h,v", STRIDING_SIZES)
def test_reproject_with_more_lanes_than_one_round_of_workgroups(hip, w, h, v, dtype):
    assert (w % 4 == 0) == (v == 4) and (w * h // v + 255) // 256 > STRIDE_BLOCKS
    plan = hip.StereoPlan(w, h, 4, 1, "ghost", max_pairs=1)
    try:
        q = pp.matrices(w, h)["rig"]
        for k, pattern in enumerate(("random_50", "last_only")):
            m = pp.make_map(pattern, 1, w, h, dtype, seed=k)
            gate = pp.Z_GATES[1 - k]                            # (the lone last pixel lies outside the gate)
            check_dense(plan, m, q, -1.0, gate, (True, True), True, (w, h, pattern, "dense"))
            counts = check_cloud(plan, m, q, pp.gray(1, w, h, k), gate, w * h, True, (w, h, pattern, "cloud"))
            assert min(counts) > 0
    finally:
        plan.close()


# ---------------------------------------------------------------------------
# c. the one-pixel path of the consistency check, striding
# ---------------------------------------------------------------------------

def lr_maps(w, h, d, seed):
    """a left map and a right-reference map that agree for about half of the pixels"""
    rng = np.random.default_rng(seed)
    web = rng.integers(1, d + 1, (h, w)).astype(np.int32)
    right = rng.integers(1, d + 1, (h, w)).astype(np.int32)
    agree = rng.random((h, w)) < 0.5
    ys, xs = np.nonzero(agree)
    u = xs + web[ys, xs] - 1
    inside = u < w
    right[ys[inside], u[inside]] = web[ys[inside], xs[inside]]
    return web, right


@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
def test_lr_check_one_pixel_path_strides(hip, mode):
    w, h, d = 1029, 256, 16
    assert w % 4 and (w * h + 255) // 256 > STRIDE_BLOCKS
    plan = hip.StereoPlan(w, h, d, 1, mode, max_pairs=1)
    try:
        for max_diff in (0, 1):
            web, right = lr_maps(w, h, d, seed=max_diff)
            want, rejected = lr.lr_check(web, right, max_diff, mode)
            assert w * h // 8 < rejected < w * h * 7 // 8
            got, n = plan.lr_check(dev(web), dev(right), max_diff)
            assert np.array_equal(host(got)[0], want), (mode, max_diff)
            assert int(n[0]) == rejected, (mode, max_diff)
    finally:
        plan.close()


@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
def test_mirrored_lr_check_one_pixel_path_strides(hip, mode):
    """the cost mode's checked entry: its right-reference pass leaves the map in mirrored order, and at a width that is
    no multiple of 4 the check reads it, and writes the natural-order map, a pixel a lane"""
    w, h, d, sw = 1029, 256, 6, 3
    rng = np.random.default_rng(12)
    left = rng.integers(0, 256, (h, w), dtype=np.uint8)
    right = np.roll(left, 2, axis=1)                                             # web = 3 where the rows match
    right[::3] = rng.integers(0, 256, right[::3].shape, dtype=np.uint8)          # rows that do not match
    e = clr.expected(left, right, d, sw, mode, "sad", 0)
    assert 1000 < e["rejected"] < w * h - 1000 and (e["checked"] == 3).sum() > w * h // 2
    plan = hip.StereoPlan(w, h, d, sw, mode, max_pairs=1)
    try:
        res = plan.cost_lr(dev(left), dev(right), "sad", max_diff=0, want_right=True, want_best=True)
        assert np.array_equal(host(res.web)[0], e["checked"]), plan.describe()
        assert np.array_equal(host(res.web_right)[0], e["web_right"]), plan.describe()
        assert np.array_equal(host(res.best)[0], e["best"]), plan.describe()
        assert int(res.rejected[0]) == e["rejected"]
    finally:
        plan.close()


# ---------------------------------------------------------------------------
# d. batches of more than 64 pairs: the second and third workgroup of k_lr_zero_counts and k_step3_init
# ---------------------------------------------------------------------------

BW, BH, BD, MAX_PAIRS = 17, 5, 6, 130


def counts_buffer(n):
    return torch.full((n,), COUNT_FILL, dtype=torch.int32, device="cuda")


@pytest.fixture(scope="module")
def batch():
    """130 small maps of each kind, every pair different: disparity maps with holes (int32 and int16), right-reference
    maps, guides, and hole-free maps of another value range per pair for the contours"""
    rng = np.random.default_rng(130)
    n, shape = MAX_PAIRS, (MAX_PAIRS, BH, BW)
    web = np.where(rng.random(shape) < 0.35, 0, rng.integers(1, BD + 1, shape)).astype(np.int32)
    sub = np.where(web == 0, 0, 16 * web + rng.integers(-8, 9, shape)).astype(np.int16)
    right = rng.integers(1, BD + 1, shape).astype(np.int32)
    guide = rng.integers(0, 256, shape, dtype=np.uint8)
    contour = (rng.integers(0, 40, shape) + 3 * np.arange(n)[:, None, None] - 100).astype(np.int32)
    contour[:, 0, 0] = contour[:, 0, 1] + 30                     # (no pair is constant: the contour interval is not 0)
    return dict(web=web, sub=sub, right=right, guide=guide, contour=contour)


@pytest.fixture(scope="module")
def big_batch_plan(hip):
    plan = hip.StereoPlan(BW, BH, BD, 1, "ghost", max_pairs=MAX_PAIRS)
    yield plan
    plan.close()


@pytest.mark.parametrize("pairs", [65, 130])
def test_counts_of_every_pair_in_batches_over_64(hip, big_batch_plan, batch, pairs):
    """each call on `pairs` maps at once; every pair's maps and count against the definition applied to that pair alone"""
    plan, h = big_batch_plan, big_batch_plan._h
    web, sub, right, guide = (batch[k][:pairs] for k in ("web", "sub", "right", "guide"))
    weights = hip.guide_weights(12.0)
    q = pp.matrices(BW, BH)["rig"]

    # lr_check with a rejected count
    d_web, d_right, d_guide = dev(web), dev(right), dev(guide)      # (named: a temporary would be freed before the launch)
    out, n = torch.empty_like(d_web), counts_buffer(pairs)
    capi.check(lib.sm_lr_check(h, P(d_web), P(d_right), 1, pairs, P(out), P(n), stream()))
    want = [lr.lr_check(web[p], right[p], 1, "ghost") for p in range(pairs)]
    assert np.array_equal(host(out), np.stack([m for m, _ in want])), "lr_check maps"
    assert host(n).tolist() == [c for _, c in want], "lr_check rejected"

    for name, maps in (("web", web), ("sub", sub)):
        dtype = maps.dtype.type
        d_in = dev(maps)
        # speckle_filter with the removed count
        out, n = torch.empty_like(d_in), counts_buffer(pairs)
        capi.check(lib.sm_speckle_filter(h, P(d_in), TYPE[dtype], 2, 1, pairs, P(out), P(n), stream()))
        want = [fr.speckle(maps[p], 2, 1) for p in range(pairs)]
        assert np.array_equal(host(out), np.stack([m for m, _ in want])), (name, "speckle maps")
        assert host(n).tolist() == [int(c) for _, c in want], (name, "speckle removed")
        # interpolate with the filled count
        out, n = torch.empty_like(d_in), counts_buffer(pairs)
        capi.check(lib.sm_interpolate(h, P(d_in), TYPE[dtype], P(None), pairs, P(out), P(n), stream()))
        want = [ir.interpolate(maps[p]) for p in range(pairs)]
        assert np.array_equal(host(out), np.stack(want)), (name, "interpolate maps")
        assert host(n).tolist() == [ir.filled(maps[p], want[p]) for p in range(pairs)], (name, "interpolate filled")
        # weighted_median, filling, with the filled count
        out, n = torch.empty_like(d_in), counts_buffer(pairs)
        capi.check(lib.sm_weighted_median(h, P(d_in), TYPE[dtype], P(d_guide), 2, capi.w256(weights), capi.SM_WMED_FILL,
                                          1, pairs, P(out), P(n), stream()))
        want = [wr.weighted_median(maps[p], guide[p], 2, weights, True, 1) for p in range(pairs)]
        assert np.array_equal(host(out), np.stack([m for m, _ in want])), (name, "weighted_median maps")
        assert host(n).tolist() == [c for _, c in want], (name, "weighted_median filled")
        # reproject with the kept count
        depth = torch.empty((pairs, BH, BW), dtype=torch.float32, device="cuda")
        xyz = torch.empty((pairs, BH, BW, 3), dtype=torch.float32, device="cuda")
        n = counts_buffer(pairs)
        capi.check(lib.sm_reproject(h, P(d_in), TYPE[dtype], capi.q16(q), -30.0, 60.0, -1.0, pairs, P(depth), P(xyz), P(n),
                                    stream()))
        for p in range(pairs):
            want_d, want_x, want_n = ref.reproject(maps[p:p + 1], q, -1.0, (-30.0, 60.0))
            assert np.array_equal(host(depth)[p].view(np.uint32), want_d[0].view(np.uint32)), (name, "depth", p)
            assert np.array_equal(host(xyz)[p].view(np.uint32), want_x[0].view(np.uint32)), (name, "xyz", p)
            assert int(n[p]) == int(want_n[0]), (name, "reproject count", p)
    assert COUNT_FILL not in host(n).tolist()


@pytest.mark.parametrize("pairs", [65, 130])
def test_min_max_and_step3_of_every_pair_in_batches_over_64(hip, big_batch_plan, batch, pairs):
    plan, h = big_batch_plan, big_batch_plan._h
    times, lines = 3, 7
    # image_min_max: every pair has a range of its own
    image = batch["contour"][:pairs]
    mm = torch.full((pairs, 2), COUNT_FILL, dtype=torch.int32, device="cuda")
    d_image = dev(image)
    capi.check(lib.sm_min_max(h, P(d_image), pairs, P(mm), stream()))
    want_mm = [[int(image[p].min()), int(image[p].max())] for p in range(pairs)]
    assert host(mm).tolist() == want_mm
    assert len({tuple(v) for v in want_mm}) == pairs
    # step3 on maps with holes (the fill leaves none at 17 x 5 after three passes, or the definition says which stay)
    for maps in (batch["web"][:pairs] * 9 + np.where(batch["web"][:pairs] != 0, np.arange(pairs)[:, None, None], 0), image):
        maps = maps.astype(np.int32)
        d_web = dev(maps).clone()
        tmp, which = torch.empty_like(d_web), C.c_int(0)
        mm = torch.full((pairs, 2), COUNT_FILL, dtype=torch.int32, device="cuda")
        out = torch.empty((pairs, BH, BW), dtype=torch.uint8, device="cuda")
        capi.check(lib.sm_step3(h, P(d_web), P(tmp), times, lines, pairs, P(mm), P(out), C.byref(which), stream()))
        capi.check(lib.sm_plan_status(h, stream()))
        filled = host(tmp if which.value else d_web)
        for p in range(pairs):
            want = oracle.fill_web_holes(maps[p], times)
            assert np.array_equal(filled[p], want), ("step3 filled", p)
            assert host(mm)[p].tolist() == [int(want.min()), int(want.max())], ("step3 minmax", p)
            assert np.array_equal(host(out)[p], oracle.draw_contour_map(want, lines)), ("step3 contour", p)
