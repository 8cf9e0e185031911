"""SGM's left-right check from one aggregated volume on the GPU: sm_sgm_wta_both and sm_sgm_lr_single against the numpy
definition (tests/sgm_single_reference.py).  Every map is compared exactly; every expected value comes from the CPU
definitions, none from the HIP path."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from stereomatching_amd import capi
from stereomatching_amd.capi import lib
from tests import census_extreme_patterns as cx
from tests import sgm_single_patterns as sp
from tests import sgm_single_reference as ss
from tests.guarded import guarded_input
from tests.test_sgm_single_cpu import periodic_pair
from tests.test_write_bounds_gpu import P, Plan, expect, out, report, stream, twice

pytestmark = pytest.mark.gpu
MODES = ["toroidal", "ghost"]
# the right pixels a wave of k_sgm_both owns, per shift a lane holds: SGB_XK of stereomatching_amd/csrc/sm_sgm_both.hip
# (SGB_X = SGB_XK * K: 256 up to 64 shifts, 512 up to 128, 1024 up to 256)
XK = 256
X = XK                                     # at D = 64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def batch(w, h, pairs, seed, levels=256):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, levels, (pairs, h, w)).astype(np.uint8),
            rng.integers(0, levels, (pairs, h, w)).astype(np.uint8))


def check_both(plan, left, right, d, sw, census, p1, p2, paths, mode, tag, mds=(0, 1), left_too=True):
    """sgm_wta_both (every map) and sgm_lr_single (every map, per max_diff) against the definition, pair by pair; the
    left maps against sgm_wta's on the same plan as well"""
    pairs = left.shape[0]
    gl, gr = dev(left), dev(right)
    web, best, sub, web_right, best_right = plan.sgm_wta_both(gl, gr, census, p1, p2, paths, want_sub=True)
    res = {md: plan.sgm_lr_single(gl, gr, census, p1, p2, paths, max_diff=md, want_right=True, want_best=True,
                                  want_sub=True) for md in mds}
    if left_too:
        w0, b0, s0 = plan.sgm_wta(gl, gr, census, p1, p2, paths, want_sub=True)
        assert torch.equal(web, w0) and torch.equal(best, b0) and torch.equal(sub, s0), tag
    torch.cuda.synchronize()
    for q in range(pairs):
        e = ss.expected(left[q], right[q], d, sw, census, p1, p2, paths, mode, mds)
        t = tag + (q,)
        for name, got in (("web", web), ("best", best), ("sub", sub), ("web_right", web_right),
                          ("best_right", best_right)):
            assert np.array_equal(host(got)[q], e[name]), t + (name,)
        for md in mds:
            r = res[md]
            assert np.array_equal(host(r.web)[q], e[md]["checked"]), t + (md,)
            assert np.array_equal(host(r.web_right)[q], e["web_right"]), t + (md,)
            assert np.array_equal(host(r.best)[q], e["best"]), t + (md,)
            assert np.array_equal(host(r.sub)[q], e[md]["sub_checked"]), t + (md,)
            assert int(r.rejected[q]) == e[md]["rejected"], t + (md,)
    return web, web_right


def test_the_segment_length_named_here_is_the_kernels():
    src = (Path(__file__).resolve().parent.parent / "stereomatching_amd" / "csrc" / "sm_sgm_both.hip").read_text()
    assert int(re.search(r"^#define SGB_XK (\d+)", src, re.M).group(1)) == XK
    assert "#define SGB_X (SGB_XK * K)" in src


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d", [1, 2, 63, 64, 65, 128, 130, 200, 256])
def test_shift_counts_and_padding(hip, mode, d):
    """1, 2 and 4 shifts a lane on both sides of each boundary.  The entries d >= D of the volume hold 4 or 8 times
    0x3fffffff wrapped to -4 or -8, which would win every arg-min if read; the volume's earlier contents (two poisons)
    change nothing"""
    w, h, sw = 47, 5, 3
    paths, census = (8, 7) if d % 2 else (4, 5)
    left, right = batch(w, h, 1, 300 + d, levels=(256, 5)[d % 2])
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        plan.reserve_sgm()
        seen = []
        for word in (0x00000000, 0xFFFFFFFF):
            plan._poison_workspace(word)
            web, web_right = check_both(plan, left, right, d, sw, census, 12, 90, paths, mode, (mode, d, word),
                                        mds=(1,), left_too=word == 0)
            seen.append((host(web), host(web_right)))
        assert np.array_equal(seen[0][0], seen[1][0]) and np.array_equal(seen[0][1], seen[1][1])
    finally:
        plan.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("w", [X - 1, X, X + 1, 2 * X + 3])
def test_segment_boundaries(hip, mode, w):
    """D = 64.  Pair 0: right = left rolled by 63, so the right pixel at a segment's first column wins at d = 63 with a
    column that only the warm-up reads; pair 1: right = left, so the one at its last column wins at d = 0; pair 2: noise"""
    h, d = 3, 64
    rng = np.random.default_rng(w)
    a = rng.integers(0, 256, (h, w)).astype(np.uint8)
    n_l, n_r = batch(w, h, 1, w + 1, levels=7)
    left, right = np.stack([a, a, n_l[0]]), np.stack([np.roll(a, 63, axis=1), a, n_r[0]])
    plan = hip.StereoPlan(w, h, d, 1, mode, max_pairs=3)
    try:
        web, web_right = check_both(plan, left, right, d, 1, 7, 10, 120, 4, mode, (mode, w), mds=(0,))
        wr = host(web_right)
        for u in range(X, w, X):
            # (ghost: the rolled pair is no exact match where the roll wraps or the halo differs: the definition decides)
            assert mode == "ghost" or (wr[0, :, u] == 64).all(), u
            assert (wr[1, :, u - 1] == 1).all(), u
    finally:
        plan.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d", [128, 200])
def test_segment_boundaries_of_longer_lanes(hip, mode, d):
    """2 and 4 shifts a lane (segments of 2 X and 4 X pixels): one pixel past the first segment, the same three pairs"""
    k = (d + 63) // 64 if d <= 128 else 4
    w, h = k * X + 1, 2
    a = np.random.default_rng(d).integers(0, 256, (h, w)).astype(np.uint8)
    n_l, n_r = batch(w, h, 1, d + 1, levels=7)
    left, right = np.stack([a, a, n_l[0]]), np.stack([np.roll(a, d - 1, axis=1), a, n_r[0]])
    plan = hip.StereoPlan(w, h, d, 1, mode, max_pairs=3)
    try:
        _, web_right = check_both(plan, left, right, d, 1, 7, 10, 120, 4, mode, (mode, d), mds=(0,))
        wr = host(web_right)
        assert mode == "ghost" or (wr[0, :, k * X] == d).all()
        assert (wr[1, :, k * X - 1] == 1).all()
    finally:
        plan.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("w,h,d", [(20, 5, 65), (29, 7, 63)])
def test_width_below_shift_count(hip, mode, w, h, d):
    """the toroidal walk wraps more than once; in ghost mode most candidates are dropped"""
    left, right = batch(w, h, 1, w + d, levels=9)
    plan = hip.StereoPlan(w, h, d, 3, mode)
    try:
        _, web_right = check_both(plan, left, right, d, 3, 7, 12, 90, 8, mode, (mode, w, h, d))
        if mode == "ghost":
            assert (host(web_right)[0] <= np.arange(w)[None, :] + 1).all()
    finally:
        plan.close()


@pytest.mark.parametrize("census", [3, 5, 7])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("paths", [4, 8])
def test_borders_paths_and_census_widths(hip, census, mode, paths):
    w, h, d, sw = 33, 17, 12, 3
    left, right = batch(w, h, 1, 10 * census + paths, levels=(256, 6)[census == 5])
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        check_both(plan, left, right, d, sw, census, 12, 90, paths, mode, (census, mode, paths))
    finally:
        plan.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("w,h,d,sw", [(41, 13, 7, 1), (30, 11, 70, 3), (29, 21, 40, 9), (45, 27, 24, 25)])
def test_windows_and_batches(hip, mode, w, h, d, sw):
    """windows 1, 3, 9 and 25; a full batch (2 of 2) and a partial one (1 of 3)"""
    p1, p2 = (8 * (sw // 2 + 1), 100 * (sw // 2 + 1))
    for pairs, maxp in ((2, 2), (1, 3)):
        left, right = batch(w, h, pairs, w + d + pairs, levels=(256, 4)[pairs % 2])
        plan = hip.StereoPlan(w, h, d, sw, mode, max_pairs=maxp)
        try:
            check_both(plan, left, right, d, sw, 7, p1, p2, 8, mode, (mode, w, h, d, sw, pairs, maxp), mds=(d % 2,))
        finally:
            plan.close()


@pytest.mark.parametrize("mode", MODES)
def test_at_the_key_bound(hip, mode):
    """anti(98, 28, k), n = 25, c = 7, 8 paths, P1 = P2 = 32767: S up to 8 * 62767 = 502136 < 2^19 (toroidal), on a
    padded range (D = 200: four shifts a lane); both entries"""
    w, h, d = 98, 28, 200
    plan = hip.StereoPlan(w, h, d, 25, mode)
    try:
        for k in (5, d - 1):
            left, right = cx.anti(w, h, k)
            check_both(plan, left[None], right[None], d, 25, 7, 32767, 32767, 8, mode, (mode, k), mds=(1,))
    finally:
        plan.close()


@pytest.mark.parametrize("mode", MODES)
def test_all_tie_and_periodic_tie_maps(hip, mode):
    """rows_anti, toroidal: S is one constant over d and over the pixels of a row, so every candidate of every right pixel
    ties and web = web_right = 1 (ghost: the border breaks the ties, the definition decides); the periodic pair (L = R,
    period 8, W = 64, D = 20) ties d with d + 8 exactly and gives web_right = 1"""
    w, h, d = 56, 49, 256
    left, right = cx.rows_anti(w, h)
    plan = hip.StereoPlan(w, h, d, 25, mode)
    try:
        web, web_right = check_both(plan, left[None], right[None], d, 25, 7, 0, 32767, 8, mode, (mode, "all-tie"), mds=(0,))
        assert mode == "ghost" or ((host(web) == 1).all() and (host(web_right) == 1).all())
    finally:
        plan.close()
    left, right = periodic_pair()
    plan = hip.StereoPlan(left.shape[1], left.shape[0], 20, 1, mode)
    try:
        _, web_right = check_both(plan, left[None], right[None], 20, 1, 7, 10, 120, 8, mode, (mode, "periodic"))
        if mode == "toroidal":
            assert (host(web_right) == 1).all()
    finally:
        plan.close()


@pytest.mark.parametrize("name", sp.CASES)
def test_named_cases_are_exact(hip, name):
    """the cases of tests/sgm_single_patterns.py: each tells one mistake of the definition from the definition
    (test_sgm_single_cpu.py shows which), so an exact pass rules that mistake out in the kernel"""
    c = sp.inputs(name)
    h, w = c["left"].shape
    plan = hip.StereoPlan(w, h, c["d"], c["sw"], c["mode"])
    try:
        # (copies: the cases' arrays are read-only)
        check_both(plan, np.array(c["left"][None]), np.array(c["right"][None]), c["d"], c["sw"], c["census"], c["p1"],
                   c["p2"], c["paths"], c["mode"], (name,))
    finally:
        plan.close()


@pytest.mark.parametrize("mode", MODES)
def test_check_with_and_without_the_optional_maps(hip, mode):
    w, h, d, sw = 50, 14, 30, 5
    left, right = batch(w, h, 2, 8, levels=16)
    plan = hip.StereoPlan(w, h, d, sw, mode, max_pairs=2)
    try:
        gl, gr = dev(left), dev(right)
        for md in (0, 1):
            e = [ss.expected(left[q], right[q], d, sw, 5, 20, 200, 8, mode, (md,)) for q in range(2)]
            checked = np.stack([x[md]["checked"] for x in e])
            assert (checked == 0).any() and (checked != 0).any()
            for want_right, want_best, want_sub in ((False, False, False), (True, False, False), (False, True, True),
                                                    (False, False, True)):
                r = plan.sgm_lr_single(gl, gr, 5, 20, 200, 8, max_diff=md, want_right=want_right, want_best=want_best,
                                       want_sub=want_sub)
                t = (mode, md, want_right, want_best, want_sub)
                assert np.array_equal(host(r.web), checked), t
                assert host(r.rejected).tolist() == [x[md]["rejected"] for x in e], t
                assert (r.web_right is None) == (not want_right) and (r.best is None) == (not want_best)
                if want_right:
                    assert np.array_equal(host(r.web_right), np.stack([x["web_right"] for x in e])), t
                if want_best:
                    assert np.array_equal(host(r.best), np.stack([x["best"] for x in e])), t
                if want_sub:
                    assert np.array_equal(host(r.sub), np.stack([x[md]["sub_checked"] for x in e])), t
        web, best, sub, web_right, best_right = plan.sgm_wta_both(gl, gr, 5, 20, 200, 8, want_best=False,
                                                                  want_best_right=False)
        assert best is None and sub is None and best_right is None
        assert np.array_equal(host(web), np.stack([x["web"] for x in e]))
        assert np.array_equal(host(web_right), np.stack([x["web_right"] for x in e]))
    finally:
        plan.close()


# ---------------------------------------------------------------------------
# write bounds (tests/guarded.py)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_single_volume_entries_write_their_maps_and_nothing_else(mode):
    bad = []
    for idx, (w, h, d, sw, census, paths) in enumerate([(33, 17, 45, 3, 7, 8), (64, 12, 130, 1, 3, 4),
                                                        (10, 9, 24, 9, 5, 8)]):
        pairs, maxp = (2, 3) if idx % 2 == 0 else (1, 2)
        plan = Plan(w, h, d, sw, mode, maxp)
        tag = f"{mode} c={census} W={w} H={h} D={d} S={sw} paths={paths} pairs={pairs}/{maxp}"
        left, right = batch(w, h, pairs, idx + 70)
        p1, p2 = 9, 99
        want = [ss.expected(left[q], right[q], d, sw, census, p1, p2, paths, mode, (1,)) for q in range(pairs)]
        Wt = lambda k: np.stack([x[k] for x in want])         # noqa: E731
        Wc = lambda k: np.stack([x[1][k] for x in want])      # noqa: E731
        shp, s = (pairs, h, w), stream()
        gl, gr = guarded_input(left, "cuda", idx % 2, "left"), guarded_input(right, "cuda", 0, "right")
        for off in (0, 4):
            t = f"{tag} sm_sgm_wta_both offset {off}"
            ow, ob = out(shp, torch.int32, off, maxp, "web"), out(shp, torch.int32, 4 - off, maxp, "best")
            osb = out(shp, torch.int16, 2, maxp, "sub")
            owr, obr = out(shp, torch.int32, off, maxp, "web_right"), out(shp, torch.int32, 4 - off, maxp, "best_right")
            bad += twice(t, lambda r: lib.sm_sgm_wta_both(plan.h, P(gl.t), P(gr.t), census, p1, p2, paths, pairs, P(ow.t),
                                                          P(ob.t), P(osb.t), P(owr.t), P(obr.t), s),
                         [ow, ob, osb, owr, obr], [gl, gr])
            bad += expect(t, ow, Wt("web")) + expect(t, ob, Wt("best")) + expect(t, osb, Wt("sub"))
            bad += expect(t, owr, Wt("web_right")) + expect(t, obr, Wt("best_right"))
            t = f"{tag} sm_sgm_wta_both (web and web_right only) offset {off}"
            ow, owr = out(shp, torch.int32, off, maxp, "web"), out(shp, torch.int32, 4 - off, maxp, "web_right")
            bad += twice(t, lambda r: lib.sm_sgm_wta_both(plan.h, P(gl.t), P(gr.t), census, p1, p2, paths, pairs, P(ow.t),
                                                          None, None, P(owr.t), None, s), [ow, owr], [gl, gr])
            bad += expect(t, ow, Wt("web")) + expect(t, owr, Wt("web_right"))
            t = f"{tag} sm_sgm_lr_single offset {off}"
            ow, ob, owr = (out(shp, torch.int32, o, maxp, n) for o, n in ((off, "web"), (4 - off, "best"),
                                                                          (off, "web_right")))
            orj = out((pairs,), torch.int32, off, maxp, "rejected")
            osb = out(shp, torch.int16, 2, maxp, "sub")
            bad += twice(t, lambda r: lib.sm_sgm_lr_single(plan.h, P(gl.t), P(gr.t), census, p1, p2, paths, pairs, 1,
                                                           P(ow.t), P(ob.t), P(owr.t), P(orj.t), P(osb.t), s),
                         [ow, ob, owr, orj, osb], [gl, gr])
            bad += expect(t, ow, Wc("checked")) + expect(t, ob, Wt("best")) + expect(t, owr, Wt("web_right"))
            bad += expect(t, orj, Wc("rejected")) + expect(t, osb, Wc("sub_checked"))
            t = f"{tag} sm_sgm_lr_single (web only) offset {off}"
            ow = out(shp, torch.int32, off, maxp, "web")
            bad += twice(t, lambda r: lib.sm_sgm_lr_single(plan.h, P(gl.t), P(gr.t), census, p1, p2, paths, pairs, 1,
                                                           P(ow.t), None, None, None, None, s), [ow], [gl, gr])
            bad += expect(t, ow, Wc("checked"))
        plan.close()
    report(bad)


# ---------------------------------------------------------------------------
# arguments, workspace, capture
# ---------------------------------------------------------------------------

def test_argument_checks_on_a_plan(hip):
    w, h, d = 64, 32, 16
    plan = hip.StereoPlan(w, h, d, 5, "toroidal", max_pairs=2)
    base = plan.workspace_bytes()
    m = [torch.zeros((2, h, w), dtype=torch.int32, device="cuda") for _ in range(4)]
    p = [C.c_void_p(t.data_ptr()) for t in m]
    g = torch.zeros((4, h, w), dtype=torch.uint8, device="cuda")
    gp = C.c_void_p(g.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    inside = C.c_void_p(m[0].data_ptr() + 4)

    def refused(rc, text):
        assert rc == capi.SM_ERR_ARG and text in lib.sm_last_error(), lib.sm_last_error()
    both, single = lib.sm_sgm_wta_both, lib.sm_sgm_lr_single
    refused(both(plan._h, None, gp, 7, 10, 120, 8, 1, p[0], None, None, p[1], None, st),
            b"sm_sgm_wta_both: input image pointer is NULL")
    refused(both(plan._h, gp, gp, 7, 10, 120, 8, 1, None, None, None, p[1], None, st), b"sm_sgm_wta_both: d_web is NULL")
    refused(both(plan._h, gp, gp, 7, 10, 120, 8, 1, p[0], None, None, None, None, st),
            b"sm_sgm_wta_both: d_web_right is NULL")
    refused(both(plan._h, gp, gp, 7, 10, 120, 8, 3, p[0], None, None, p[1], None, st),
            b"sm_sgm_wta_both: pairs 3 outside 1..2")
    refused(both(plan._h, gp, gp, 7, 10, 120, 8, 0, p[0], None, None, p[1], None, st), b"sm_sgm_wta_both: pairs 0 outside")
    refused(both(plan._h, gp, gp, 6, 10, 120, 8, 1, p[0], None, None, p[1], None, st),
            b"sm_sgm_wta_both: census_width 6 is not 3, 5 or 7")
    refused(both(plan._h, gp, gp, 7, 10, 120, 6, 1, p[0], None, None, p[1], None, st), b"sm_sgm_wta_both: paths 6 is not")
    refused(both(plan._h, gp, gp, 7, 130, 120, 8, 1, p[0], None, None, p[1], None, st), b"sm_sgm_wta_both: penalties")
    for args in ((p[0], inside, None, p[1], None), (p[0], None, None, inside, None), (p[0], p[2], None, p[1], inside),
                 (p[0], p[2], None, p[1], p[2]), (p[0], p[2], inside, p[1], None),
                 (p[0], p[2], C.c_void_p(m[1].data_ptr() + 2), p[1], p[3]),
                 (p[0], p[2], C.c_void_p(m[3].data_ptr() + 2), p[1], p[3])):
        refused(both(plan._h, gp, gp, 7, 10, 120, 8, 1, *args, st), b"sm_sgm_wta_both: result maps overlap")
    refused(single(plan._h, gp, None, 3, 10, 120, 8, 1, 0, p[0], None, None, None, None, st),
            b"sm_sgm_lr_single: input image pointer is NULL")
    refused(single(plan._h, gp, gp, 3, 10, 120, 8, 1, 0, None, None, None, None, None, st),
            b"sm_sgm_lr_single: d_web is NULL")
    refused(single(plan._h, gp, gp, 3, 10, 120, 8, 3, -2, p[0], None, None, None, None, st),
            b"sm_sgm_lr_single: max_diff -2 is negative")          # before pairs: sm_sgm_lr's order
    refused(single(plan._h, gp, gp, 3, 10, 120, 8, 3, 0, p[0], None, None, None, None, st),
            b"sm_sgm_lr_single: pairs 3 outside")
    refused(single(plan._h, gp, gp, 4, 10, 120, 8, 1, 0, p[0], None, None, None, None, st),
            b"sm_sgm_lr_single: census_width 4 is not")
    refused(single(plan._h, gp, gp, 3, 10, 120, 5, 1, 0, p[0], None, None, None, None, st),
            b"sm_sgm_lr_single: paths 5 is not 4 or 8")
    refused(single(plan._h, gp, gp, 3, 10, 9, 8, 1, 0, p[0], None, None, None, None, st),
            b"sm_sgm_lr_single: penalties p1 10, p2 9 break")
    refused(single(plan._h, gp, gp, 3, 10, 120, 8, 1, 0, p[0], p[0], None, None, None, st),
            b"sm_sgm_lr_single: result maps overlap")
    refused(single(plan._h, gp, gp, 3, 10, 120, 8, 1, 0, p[0], None, inside, None, None, st),
            b"sm_sgm_lr_single: result maps overlap")
    refused(single(plan._h, gp, gp, 3, 10, 120, 8, 1, 0, p[0], None, p[1], None, C.c_void_p(m[1].data_ptr()), st),
            b"sm_sgm_lr_single: result maps overlap")
    refused(single(plan._h, gp, gp, 3, 10, 120, 8, 2, 0, p[0], p[1], None, inside, None, st),
            b"sm_sgm_lr_single: d_rejected overlaps a map")
    refused(single(plan._h, gp, gp, 3, 10, 120, 8, 1, 0, p[0], None, None, p[2], C.c_void_p(m[2].data_ptr()), st),
            b"sm_sgm_lr_single: d_rejected overlaps a map")
    assert plan.workspace_bytes() == base
    plan.close()
    for pw, ph, pd, psw, text in ((64, 32, 16, 27, b"(got 27x27, 16)"), (64, 32, 257, 5, b"(got 5x5, 257)")):
        plan = hip.StereoPlan(pw, ph, pd, psw, "toroidal")
        base = plan.workspace_bytes()
        q = [torch.zeros((1, ph, pw), dtype=torch.int32, device="cuda") for _ in range(2)]
        gq = torch.zeros((1, ph, pw), dtype=torch.uint8, device="cuda")
        qp, qr, gqp = C.c_void_p(q[0].data_ptr()), C.c_void_p(q[1].data_ptr()), C.c_void_p(gq.data_ptr())
        for name, call in ((b"sm_sgm_wta_both", lambda: both(plan._h, gqp, gqp, 7, 1, 2, 8, 1, qp, None, None, qr, None, st)),
                           (b"sm_sgm_lr_single", lambda: single(plan._h, gqp, gqp, 5, 1, 2, 8, 1, 0, qp, None, None, None,
                                                                None, st))):
            refused(call(), name + b": built for windows up to 25x25 and at most 256 shifts")
            assert text in lib.sm_last_error()
        assert plan.workspace_bytes() == base
        plan.close()


def test_workspace_is_the_sgm_workspace_and_allocated_by_the_first_call(hip):
    w, h, d, sw, mp = 120, 40, 100, 3, 2
    left, right = batch(w, h, 1, 3, levels=32)
    gl, gr = dev(left), dev(right)
    desc = 2 * mp * w * h * 8
    mapb = mp * w * h * 4
    vol = 6 * w * h * 128                                  # 100 shifts padded to 128
    e = ss.expected(left[0], right[0], d, sw, 5, 10, 120, 4, "toroidal", (0,))
    for first in ("both", "single"):
        plan = hip.StereoPlan(w, h, d, sw, "toroidal", max_pairs=mp)
        try:
            base = plan.workspace_bytes()
            if first == "both":
                got = plan.sgm_wta_both(gl, gr, 5, 10, 120, 4, want_best=False)[3]
                want = e["web_right"]
            else:
                got = plan.sgm_lr_single(gl, gr, 5, 10, 120, 4).web
                want = e[0]["checked"]
            torch.cuda.synchronize()
            assert plan.workspace_bytes() == base + desc + mapb + vol       # what reserve_sgm allocates: nothing new
            assert np.array_equal(host(got)[0], want)
            plan.sgm_lr_single(gl, gr, 5, 10, 120, 4, want_right=True, want_best=True, want_sub=True)
            plan.sgm_wta(gl, gr, 5, 10, 120, 4)
            plan.reserve_sgm()
            assert plan.workspace_bytes() == base + desc + mapb + vol
        finally:
            plan.close()


@pytest.mark.parametrize("mode,census,paths", [("ghost", 7, 8), ("toroidal", 5, 4)])
def test_captured_into_a_graph(hip, mode, census, paths):
    from stereomatching_amd import pipeline
    w, h, d, sw = 90, 30, 40, 3
    left, right = batch(w, h, 3, 60, levels=24)
    left_in = torch.zeros((1, h, w), dtype=torch.uint8, device="cuda")
    right_in = torch.zeros_like(left_in)
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        base = plan.workspace_bytes()
        web, wr, best, br, cweb, cright = (torch.zeros((1, h, w), dtype=torch.int32, device="cuda") for _ in range(6))
        sub = torch.zeros((1, h, w), dtype=torch.int16, device="cuda")
        rej = torch.zeros(1, dtype=torch.int32, device="cuda")
        for call in (lambda: plan.sgm_lr_single(left_in, right_in, census, 10, 120, paths, web=cweb),
                     lambda: plan.sgm_wta_both(left_in, right_in, census, 10, 120, paths, want_best=False,
                                               want_best_right=False, web=web, web_right=wr)):
            with pytest.raises(capi.StereoHipError, match="sm_plan_reserve_sgm"):
                with torch.cuda.graph(torch.cuda.CUDAGraph(), capture_error_mode="thread_local"):
                    call()
        assert plan.workspace_bytes() == base
        plan.reserve_sgm()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            pipeline.check(lib.sm_sgm_wta_both(plan._h, P(left_in), P(right_in), census, 10, 120, paths, 1, P(web),
                                               P(best), P(sub), P(wr), P(br), plan._stream()))
            pipeline.check(lib.sm_sgm_lr_single(plan._h, P(left_in), P(right_in), census, 10, 120, paths, 1, 1, P(cweb),
                                                None, P(cright), P(rej), None, plan._stream()))
        for rep in (1, 2, 0):
            left_in.copy_(dev(left[rep:rep + 1]))
            right_in.copy_(dev(right[rep:rep + 1]))
            for t in (web, wr, best, br, cweb, cright, sub):
                t.zero_()
            rej.fill_(12345)
            g.replay()
            torch.cuda.synchronize()
            e = ss.expected(left[rep], right[rep], d, sw, census, 10, 120, paths, mode, (1,))
            for name, got in (("web", web), ("best", best), ("sub", sub), ("web_right", wr), ("best_right", br),
                              ("web_right", cright)):
                assert np.array_equal(host(got)[0], e[name]), (rep, name)
            assert np.array_equal(host(cweb)[0], e[1]["checked"]), rep
            assert int(rej[0]) == e[1]["rejected"], rep
    finally:
        plan.close()
