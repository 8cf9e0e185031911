"""Step 3 on maps WITH holes on the GPU: sm_fill_web_holes (k_count_zeros, k_fill_holes_step),
sm_min_max (k_minmax_zero), sm_draw_contour_map (k_contour) and sm_step3 (its fused route for maps
without a 0, its staged route for maps with one), against

  - what the reference's own step-3 functions made of the maps of tests/step3_patterns.py
    (tests/golden/step3/, pinned to the restatement by tests/test_step3_cpu.py), and
  - elsewhere the restatement (oracle.fill_web_holes / oracle.draw_contour_map) and exact integer
    values: lone minima, maxima and zeros at the positions where a reduction's indexing can go
    wrong, at sizes from one workgroup to past the grid's 1024-workgroup cap.

Every assertion names its case and pair."""
import ctypes as C

import numpy as np
import pytest
import torch

from stereomatching_amd.synth import CONFIGS, make_pair
from tests import oracle
from tests import step3_patterns as sp
from tests.conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

STEP3_DIR = GOLDEN_DIR / "step3"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def fixture(name):
    z = np.load(STEP3_DIR / f"{name}.npz")
    return {k: z[k] for k in z.files}


def expect(web, times, lines):
    """(filled, contour or None where the interval is 0) of one map by the restatement"""
    filled = oracle.fill_web_holes(web, times)
    try:
        return filled, oracle.draw_contour_map(filled, lines)
    except ZeroDivisionError:
        return filled, None


def offset(web, k):
    """the map with every non-zero value moved k away from 0 (toward 0 where that would leave
    |v| < 2^29): the same holes, other values, another min / max per pair"""
    s = np.sign(web)
    big = np.abs(web.astype(np.int64)) + k >= sp.LIMIT
    return np.where(web == 0, 0, np.where(big, web - s * k, web + s * k)).astype(np.int32)


def zero_div(hip, fn, *args):
    with pytest.raises(hip.capi.StereoHipError) as e:
        fn(*args)
    assert e.value.code == hip.capi.SM_ERR_ZERO_DIV


def check_staged_and_fused(hip, plan, webs, wants, times, lines, what):
    """plan.fill_web_holes + image_min_max + draw_contour_map, and plan.step3, on a stack of maps:
    each pair against its (filled, contour) -- a contour of None means a zero interval; any one of
    them makes the whole call report SM_ERR_ZERO_DIV"""
    d = dev(np.stack(webs))
    traps = any(c is None for _, c in wants)
    filled = plan.fill_web_holes(d, times)
    mm = host(plan.image_min_max(filled))
    got = host(filled)
    for j, (f, _) in enumerate(wants):
        assert np.array_equal(got[j], f), (what, "fill_web_holes", "pair", j)
        assert mm[j].tolist() == [int(f.min()), int(f.max())], (what, "image_min_max", "pair", j)
    if traps:
        zero_div(hip, plan.draw_contour_map, filled, lines)
        zero_div(hip, plan.step3, d, times, lines)
        return
    out = host(plan.draw_contour_map(filled, lines))
    filled3, out3, mm3 = plan.step3(d, times, lines)
    filled3, out3, mm3 = host(filled3), host(out3), host(mm3)
    for j, (f, c) in enumerate(wants):
        assert np.array_equal(out[j], c), (what, "draw_contour_map", "pair", j)
        assert np.array_equal(filled3[j], f), (what, "step3 filled", "pair", j)
        assert np.array_equal(out3[j], c), (what, "step3 contour", "pair", j)
        assert mm3[j].tolist() == [int(f.min()), int(f.max())], (what, "step3 minmax", "pair", j)


# ---------------------------------------------------------------------------
# 1, 2: every reference fixture, alone and stacked (later pairs' bases off 16 bytes)
# ---------------------------------------------------------------------------

def test_fixture_shapes_cover_every_pair_stride():
    # n % 4 = 1, 2, 3: pair k > 0 of a stack starts 4 * k * n bytes in, not 16-byte aligned, and
    # k_minmax_zero reads it with its scalar loop
    assert {(w * h) % 4 for _, w, h, *_ in sp.CASES.values()} == {0, 1, 2, 3}


@pytest.mark.parametrize("name", sorted(sp.CASES))
def test_reference_fixture_alone_and_stacked(hip, name):
    z = fixture(name)
    web = z["web"]
    times, lines = z["params"].tolist()
    h, w = web.shape
    want = (z["filled_tor"], None if int(z["rc_tor"]) == -8 else z["contour_tor"])
    plan = hip.StereoPlan(w, h, 30, 5, max_pairs=4)
    check_staged_and_fused(hip, plan, [web], [want], times, lines, (name, "alone"))
    # four pairs: the fixture, two offset copies, and one without holes (the fused route's
    # speculation must see the others' zeros)
    webs = [web, offset(web, 1), np.where(web == 0, 1, web).astype(np.int32), offset(web, 3)]
    wants = [want] + [expect(x, times, lines) for x in webs[1:]]
    check_staged_and_fused(hip, plan, webs, wants, times, lines, (name, "stacked"))
    # a zero interval leaves the plan usable
    ok = np.arange(1, w * h + 1, dtype=np.int32).reshape(h, w)
    f, out, _ = plan.step3(dev(ok[None]), times, 10)
    assert np.array_equal(host(f)[0], ok) and np.array_equal(host(out)[0], oracle.draw_contour_map(ok, 10)), name
    plan.close()


# ---------------------------------------------------------------------------
# 3: the reductions over several workgroups
# ---------------------------------------------------------------------------

# (w, h): workgroups of k_minmax_zero = min(1024, ceil(n / 65536))
REDUCTION_SHAPES = {
    "1 block, n = 65535":        (255, 257),
    "2 blocks, n = 65750":       (263, 250),
    "16 blocks, odd n":          (1031, 1001),
    "4K, 127 blocks":            (3840, 2160),
    "past the 1024-block cap":   (8256, 8160),
}


def reduction_positions(n):
    """(label, pair, flat index) of the single special pixel: the first element, the last 16-byte
    quad, the scalar tail, the last workgroup's range (in its last grid-stride round), and in the
    last pair only (based 4 n bytes in: scalar loop unless n % 4 == 0)"""
    blocks = min(1024, -(-n // 65536))
    stride = blocks * 256
    nq = n // 4
    first_tid = (blocks - 1) * 256 + 255               # the last thread of the last workgroup

    def last_round(tid, count):
        return tid + (count - 1 - tid) // stride * stride

    quad_elem = 4 * last_round(first_tid, nq) + 1
    pos = [("first element", 0, 0), ("last quad", 0, 4 * nq - 1), ("last workgroup, quads", 0, quad_elem)]
    if n % 4:
        pos.append(("scalar tail", 0, n - 1))
        pos.append(("last pair, last workgroup, scalar loop", 1, last_round(first_tid, n)))
    else:
        pos.append(("last pair, last workgroup, quads", 1, quad_elem))
    pos.append(("last pair, last element", 1, n - 1))
    return pos


def lone_hole_fill(base, pair, e, times):
    """the value the restatement gives a lone 0 at flat index e of one pair: run on the rows around
    it (flat neighbours lie within one row of it; a crop that ends at a real border ends there)"""
    _, h, w = base.shape
    y = e // w
    y0, y1 = max(0, y - 2), min(h, y + 3)
    crop = host(base[pair, y0:y1]).copy()
    crop.reshape(-1)[e - y0 * w] = 0
    return int(oracle.fill_web_holes(crop, times).reshape(-1)[e - y0 * w])


def contour_of(filled, lines):
    """draw_contour_map of each pair, in torch integer ops (no project kernel)"""
    flat = filled.view(filled.shape[0], -1).to(torch.int64)
    lo = flat.min(1).values[:, None]
    hi = flat.max(1).values[:, None]
    interval = (hi - lo) // lines
    assert bool((interval > 0).all())
    return (((flat - lo) % interval) == 0).to(torch.uint8).view(filled.shape)


@pytest.mark.parametrize("shape", list(REDUCTION_SHAPES))
def test_lone_minimum_maximum_and_zero_over_many_workgroups(hip, shape):
    w, h = REDUCTION_SHAPES[shape]
    n = w * h
    times, lines = 2, 10
    plan = hip.StereoPlan(w, h, 16, 5, max_pairs=2)
    idx = torch.arange(2 * n, device="cuda", dtype=torch.int64)
    base = ((idx * 2654435761) % 1000 + 100).to(torch.int32).view(2, h, w)       # values 100..1099
    base[1] += 7
    flat = base.view(2, -1)
    lo = [int(flat[j].min()) for j in range(2)]
    hi = [int(flat[j].max()) for j in range(2)]

    # no zero: fused route; hole filling is the identity
    f, out, mm = plan.step3(base, times, lines)
    assert torch.equal(f, base) and torch.equal(out, contour_of(base, lines)), (shape, "no zero")
    assert host(mm).tolist() == [[lo[0], hi[0]], [lo[1], hi[1]]], (shape, "no zero")
    assert torch.equal(plan.fill_web_holes(base, times), base), (shape, "no zero")

    for label, pair, e in reduction_positions(n):
        what = (shape, label, "pair", pair, "index", e)
        keep = int(flat[pair, e])
        for value in (7, 5000):                      # the only minimum, the only maximum
            flat[pair, e] = value
            want = [[lo[0], hi[0]], [lo[1], hi[1]]]
            want[pair] = [min(value, lo[pair]), max(value, hi[pair])]
            assert host(plan.image_min_max(base)).tolist() == want, (*what, value)
            flat[pair, e] = keep
        # the only zero: found by k_count_zeros and by k_minmax_zero's flag (else step3 would take
        # its fused route and leave it unfilled), filled as the restatement fills it
        filled_value = lone_hole_fill(base, pair, e, times)
        flat[pair, e] = 0
        expected = base.clone()
        expected.view(2, -1)[pair, e] = filled_value
        mm0 = host(plan.image_min_max(base))
        assert mm0[pair].tolist() == [0, hi[pair]], what
        assert torch.equal(plan.fill_web_holes(base, times), expected), (*what, "fill_web_holes")
        f, out, mm = plan.step3(base, times, lines)
        assert torch.equal(f, expected), (*what, "step3 filled")
        assert torch.equal(out, contour_of(expected, lines)), (*what, "step3 contour")
        want = [[lo[0], hi[0]], [lo[1], hi[1]]]
        want[pair] = [min(filled_value, lo[pair]), hi[pair]]
        assert host(mm).tolist() == want, (*what, "step3 minmax")
        flat[pair, e] = keep
    plan.close()


@pytest.mark.parametrize("w,h", sp.NO_POSITIVE_SHAPES)
def test_minimum_and_maximum_of_maps_without_a_positive_value(hip, w, h):
    """Every other map of this module holds a value >= 0 in every pair, so a running maximum started at 0 instead of
    INT_MIN reported the right number (the mutation audit's Z4; the CPU proof is in tests/test_step3_cpu.py).  Here every
    value is negative: the maximum is -11, and the contour interval follows from it (98, not 100).  37 x 5 ends in
    k_minmax_zero's scalar tail and bases its second pair off 16 bytes (scalar loop); 64 x 4 is 16-byte loads alone.
    No map has a zero, so filling is the identity on both routes."""
    webs = [sp.no_positive(w, h, seed=w), sp.no_positive(w, h, seed=w + 1) - 5]
    wants = [expect(x, 2, 10) for x in webs]
    assert all(int(f.max()) < 0 and c is not None for f, c in wants)
    plan = hip.StereoPlan(w, h, 16, 1, max_pairs=2)         # (step 3 reads W, H and max_pairs of the plan only)
    check_staged_and_fused(hip, plan, webs, wants, 2, 10, ("no positive value", w, h))
    plan.close()


# ---------------------------------------------------------------------------
# 4: sm_step3's routes and flags
# ---------------------------------------------------------------------------

def raw_fill(hip, plan, web, times, step3_lines=None):
    """sm_fill_web_holes / sm_step3 through the C ABI -> (web buffer, tmp buffer, result_in_tmp)"""
    lib = hip.capi.lib
    web = web.clone()
    tmp = torch.zeros_like(web)
    which = C.c_int(-1)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    if step3_lines is None:
        rc = lib.sm_fill_web_holes(plan._h, ptr(web), ptr(tmp), times, web.shape[0], C.byref(which), stream)
    else:
        mm = torch.empty((web.shape[0], 2), dtype=torch.int32, device="cuda")
        out = torch.empty(web.shape, dtype=torch.uint8, device="cuda")
        rc = lib.sm_step3(plan._h, ptr(web), ptr(tmp), times, step3_lines, web.shape[0], ptr(mm), ptr(out),
                          C.byref(which), stream)
    hip.capi.check(rc)
    torch.cuda.synchronize()
    return web, tmp, which.value


def test_holes_in_one_pair_of_a_batch(hip):
    web, _, _ = sp.case("mixed_t2")
    h, w = web.shape
    full = np.where(web == 0, 3, web).astype(np.int32)
    plan = hip.StereoPlan(w, h, 30, 5, max_pairs=3)
    for holed in range(3):
        webs = [offset(full, k) for k in range(3)]
        webs[holed] = offset(web, holed)
        for times in (1, 2, 3):
            check_staged_and_fused(hip, plan, webs, [expect(x, times, 10) for x in webs], times, 10,
                                   ("holes in pair", holed, "times", times))
    plan.close()


def test_holes_with_times_zero_are_left_as_they_are(hip):
    web, _, _ = sp.case("mixed_t0")
    h, w = web.shape
    plan = hip.StereoPlan(w, h, 30, 5, max_pairs=2)
    webs = [web, offset(web, 2)]
    check_staged_and_fused(hip, plan, webs, [(x, oracle.draw_contour_map(x, 10)) for x in webs], 0, 10, "times 0")
    plan.close()


def test_zero_interval_after_filling_only(hip):
    z = fixture("zero_after_fill_t2")
    web = z["web"]
    times, lines = z["params"].tolist()
    h, w = web.shape
    assert int(z["rc_tor"]) == -8
    plan = hip.StereoPlan(w, h, 30, 5, max_pairs=2)
    out = host(plan.draw_contour_map(dev(web[None]), lines))[0]        # unfilled: interval 2
    assert np.array_equal(out, oracle.draw_contour_map(web, lines))
    zero_div(hip, plan.step3, dev(web[None]), times, lines)
    zero_div(hip, plan.step3, dev(np.stack([np.where(web == 0, 9, web), web]).astype(np.int32)), times, lines)
    # the plan succeeds on the next call
    other, _, _ = sp.case("mixed_t2")
    other = np.ascontiguousarray(np.resize(other, web.shape), np.int32)
    other[0] = other[-1] = 4
    want_f, want_c = expect(other, times, lines)
    f, c, mm = plan.step3(dev(other[None]), times, lines)
    assert np.array_equal(host(f)[0], want_f) and np.array_equal(host(c)[0], want_c)
    assert host(mm)[0].tolist() == [int(want_f.min()), int(want_f.max())]
    plan.close()


@pytest.mark.parametrize("name", ["big_block_t32", "persisting_t101", "lr_scene_t3"])
def test_zeros_left_after_filling(hip, name):
    z = fixture(name)
    web, (times, lines) = z["web"], z["params"].tolist()
    assert (z["filled_tor"] == 0).any()
    h, w = web.shape
    plan = hip.StereoPlan(w, h, 30, 5, max_pairs=2)
    f, c, mm = plan.step3(dev(np.stack([web, web])), times, lines)
    for j in range(2):
        assert np.array_equal(host(f)[j], z["filled_tor"]), (name, "pair", j)
        assert np.array_equal(host(c)[j], z["contour_tor"]), (name, "pair", j)
        assert host(mm)[j].tolist() == [int(z["filled_tor"].min()), int(z["filled_tor"].max())], (name, j)
    plan.close()


@pytest.mark.parametrize("route", ["sm_fill_web_holes", "sm_step3"])
def test_result_buffer_for_odd_and_even_times(hip, route):
    """the reference returns its own `web` for every `times` (its SWAP swaps nothing): result_in_tmp
    is 0, d_web holds the filled map, and the Python wrapper hands back that buffer"""
    web, _, _ = sp.case("mixed_t2")
    h, w = web.shape
    plan = hip.StereoPlan(w, h, 30, 5, max_pairs=2)
    d = dev(np.stack([web, offset(web, 5)]))
    for times in (0, 1, 2, 3, 4, 101):
        wants = [oracle.fill_web_holes(x, times) for x in host(d)]
        got_web, _, which = raw_fill(hip, plan, d, times, 10 if route == "sm_step3" else None)
        assert which == 0, (route, times)
        for j in range(2):
            assert np.array_equal(host(got_web)[j], wants[j]), (route, times, "pair", j)
        py = plan.fill_web_holes(d, times) if route == "sm_fill_web_holes" else plan.step3(d, times, 10)[0]
        for j in range(2):
            assert np.array_equal(host(py)[j], wants[j]), (route, times, "wrapper", "pair", j)
        if times:
            assert not np.array_equal(wants[0], web), times          # the buffers differ: the pick matters
    plan.close()


# ---------------------------------------------------------------------------
# 5: holes in the first and last rows (restatement only: the reference reads outside its array)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(37, 23), (64, 48), (41, 29)])
@pytest.mark.parametrize("times", [1, 2, 32])
def test_border_row_holes(hip, w, h, times):
    web = sp.border_holes(w, h, w + h)
    plan = hip.StereoPlan(w, h, 30, 5, max_pairs=2)
    webs = [web, offset(web, 2)]
    check_staged_and_fused(hip, plan, webs, [expect(x, times, 10) for x in webs], times, 10,
                           ("border rows", w, h, times))
    plan.close()


# ---------------------------------------------------------------------------
# 6: full size, left-right checked
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", ["C3", "C5"])
@pytest.mark.parametrize("max_diff", [0, 2])
def test_full_size_checked_map_through_step3(hip, cfg, max_diff):
    w, h, d, sw, mode = CONFIGS[cfg]
    times, lines = 32, 10
    left, right = make_pair(w, h, d, seed=5)
    plan = hip.StereoPlan(w, h, d, sw, mode)
    res = plan.algorithm(dev(left), dev(right), hip.AlgorithmParams(0.15, sw, times, lines), lr_max_diff=max_diff)
    web1 = host(res["web-1"])[0]
    assert (web1 == 0).any() and int(res["lr_rejected"][0]) == int((web1 == 0).sum()), (cfg, max_diff)
    want_f, want_c = expect(web1, times, lines)
    assert want_c is not None
    assert np.array_equal(host(res["web-2"])[0], want_f), (cfg, max_diff, "web-2")
    assert np.array_equal(host(res["output-0"])[0], want_c), (cfg, max_diff, "output-0")
    f, c, mm = plan.step3(res["web-1"], times, lines)
    assert np.array_equal(host(f)[0], want_f) and np.array_equal(host(c)[0], want_c), (cfg, max_diff, "step3")
    assert host(mm)[0].tolist() == [int(want_f.min()), int(want_f.max())], (cfg, max_diff)
    # holes of our own in columns 0 and w - 1 below row 0 and above row h - 1
    holed = web1.copy()
    holed[1:h - 1:3, 0] = 0
    holed[2:h - 1:5, w - 1] = 0
    holed[h // 2, w - 1] = holed[h // 2 + 1, 0] = 0
    want_f, want_c = expect(holed, times, lines)
    f, c, mm = plan.step3(dev(holed[None]), times, lines)
    assert np.array_equal(host(f)[0], want_f), (cfg, max_diff, "edge columns, filled")
    assert np.array_equal(host(c)[0], want_c), (cfg, max_diff, "edge columns, contour")
    assert host(mm)[0].tolist() == [int(want_f.min()), int(want_f.max())], (cfg, max_diff)
    plan.close()
