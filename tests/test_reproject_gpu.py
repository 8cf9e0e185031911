"""Reprojection on the GPU: sm_reproject, sm_point_cloud and sm_plan_reserve_cloud against the numpy definition
(tests/reproject_reference.py).  Every expected value comes from the CPU definition, none from the HIP path; every
comparison is on the bits of the floats (a NaN `missing` is checked with isnan).  The sizes (tests/reproject_patterns.py)
sit on and around the dense kernel's four-pixel lanes and 256-lane workgroups and the cloud's tiles of 1024 pixels; one
size has more tiles than the scan's workgroup has lanes."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from stereomatching_amd import capi
from stereomatching_amd.capi import lib
from stereomatching_amd.synth import make_pair
from tests import cost_lr_reference as clr
from tests import filter_reference as fr
from tests import interp_reference as ir
from tests import rectify_patterns as rp
from tests import rectify_reference as rr
from tests import reproject_patterns as pp
from tests import reproject_reference as ref
from tests.guarded import POISON, guarded_input
from tests.test_write_bounds_gpu import P, Plan, expect, out, report, stream, twice

pytestmark = pytest.mark.gpu
TORCH = {np.int32: torch.int32, np.int16: torch.int16}
TYPE = {np.int32: capi.SM_MAP_I32, np.int16: capi.SM_MAP_I16}
DTYPES = [np.int32, np.int16]
BATCHES = ((2, 2), (1, 3))                                      # (pairs, max_pairs): a full and a partial batch
OUTPUTS = ((True, False), (False, True), (True, True))          # (depth, xyz)
INF = math.inf
FILL = 0x55555555                                               # what a cloud buffer holds before the call


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def plan_for(hip, w, h, max_pairs=1, d=4, mode="ghost"):
    """the stage reads W, H and max_pairs of the plan only; the window (1) fits every image"""
    return hip.StereoPlan(w, h, d, 1, mode, max_pairs=max_pairs)


def same_floats(got, want, missing, tag):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, (tag, got.dtype, got.shape, want.shape)
    if isinstance(missing, float) and math.isnan(missing):
        gone = np.isnan(want)
        assert np.isnan(got[gone]).all(), (tag, "missing is not NaN everywhere")
        got, want = got[~gone], want[~gone]
    bad = np.flatnonzero(bits(got).reshape(-1) != bits(want).reshape(-1))
    assert not len(bad), (tag, len(bad), int(bad[0]), got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


def check_dense(plan, m, q, missing, gate, outputs, want_count, tag):
    want_d, want_x, want_n = ref.reproject(m, q, missing, gate)
    res = plan.reproject(dev(m), q, want_depth=outputs[0], want_xyz=outputs[1], missing=missing, z_range=gate,
                         want_count=want_count)
    res = list(res) if isinstance(res, tuple) else [res]
    assert len(res) == outputs[0] + outputs[1] + want_count, tag
    if outputs[0]:
        same_floats(host(res.pop(0)), want_d, missing, tag + ("depth",))
    if outputs[1]:
        same_floats(host(res.pop(0)), want_x, missing, tag + ("xyz",))
    if want_count:
        n = host(res.pop(0))
        assert n.dtype == np.int32 and np.array_equal(n, want_n), (tag, n, want_n)


def check_cloud(plan, m, q, g, gate, capacity, want_index, tag):
    """capacity: an int, or "count" / "count-1" (of the fullest pair)"""
    pairs, h, w = m.shape
    wants = [ref.point_cloud(m[p], q, None if g is None else g[p], gate) for p in range(pairs)]
    counts = [len(i) for _, i in wants]
    cap = max(0, max(counts) - (capacity == "count-1")) if isinstance(capacity, str) else capacity
    pts = torch.full((pairs, cap, 4), FILL, dtype=torch.int32, device="cuda").view(torch.float32)
    res = plan.point_cloud(dev(m), q, None if g is None else dev(g), z_range=gate, want_index=want_index, points=pts)
    assert len(res) == (3 if want_index else 2) and res[0] is pts
    n = host(res[1])
    assert n.dtype == np.int32 and n.tolist() == counts, (tag, n.tolist(), counts)
    got = host(pts)
    for p in range(pairs):
        k = min(counts[p], cap)
        assert np.array_equal(bits(got[p, :k]), bits(wants[p][0][:k])), (tag, p, "records")
        assert (bits(got[p, k:]) == FILL).all(), (tag, p, "slots from count on were written")
        if want_index:
            assert np.array_equal(host(res[2])[p, :k], wants[p][1][:k]), (tag, p, "index")
    return counts


# ---------------------------------------------------------------------------
# dense
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_reproject_at_every_size(hip, dtype):
    i = 0
    for (w, h) in pp.SIZES:
        qs = pp.matrices(w, h)
        for pairs, maxp in BATCHES:
            plan = plan_for(hip, w, h, maxp)
            try:
                for outputs in OUTPUTS:
                    for want_count in (False, True):
                        name = list(qs)[i % len(qs)]
                        pattern = pp.PATTERNS[i % len(pp.PATTERNS)]
                        missing, gate = pp.MISSING[i % 4], pp.Z_GATES[(i // 4) % 2]
                        m = pp.make_map(pattern, pairs, w, h, dtype, seed=i)
                        check_dense(plan, m, qs[name], missing, gate, outputs, want_count,
                                    (w, h, pairs, maxp, name, pattern, missing, gate))
                        i += 1
            finally:
                plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", [(66, 7), (64, 9)])
def test_reproject_every_pattern_matrix_missing_and_gate(hip, dtype, size):
    w, h = size
    plan = plan_for(hip, w, h, 2)
    try:
        for name, q in pp.matrices(w, h).items():
            for k, pattern in enumerate(pp.PATTERNS):
                m = pp.make_map(pattern, 2, w, h, dtype, seed=k)
                for missing in pp.MISSING:
                    for gate in pp.Z_GATES:
                        check_dense(plan, m, q, missing, gate, (True, True), True, (w, h, name, pattern, missing, gate))
    finally:
        plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_gate_bounds_an_x_that_is_no_float_and_the_rounding_of_a_row(hip, dtype):
    """What the mutation audit's J1, J2, J3 and J5 changed decides a pixel only here (tests/reproject_patterns.py
    edge_matrices; the CPU proof is test_the_edge_cases_tell_each_mistake_and_the_older_inputs_do_not): Z = d exactly, so
    the pixels with d = 2 and d = 40 sit ON the gate's bounds and must be kept; X = 1e300 x is no float32 from column 1
    on while Y and Z are finite, so isfinite(X) alone drops the pixel; and at (3, 1) of `fused_tie` X rounds to
    1 + 2^-23 only if a x is rounded before b y is added.  8 x 3 is the smallest map with (3, 1) in a lane of four
    pixels (V = 4) and with both bounds in every pair (the even disparities 0 .. 46); 7 x 3 (0 .. 40) takes the
    one-pixel lanes.  Dense maps, counts and the cloud, both gates."""
    for w in (pp.EDGE_W, pp.EDGE_W - 1):
        m = pp.edge_map(2, w, pp.EDGE_H, dtype)
        plan = plan_for(hip, w, pp.EDGE_H, 2)
        try:
            for name, q in pp.edge_matrices().items():
                for gate in (None, pp.EDGE_GATE):
                    check_dense(plan, m, q, -1.0, gate, (True, True), True, (w, name, gate))
                    check_cloud(plan, m, q, None, gate, w * pp.EDGE_H, True, (w, name, gate))
        finally:
            plan.close()


def test_caller_buffers_and_larger_batches(hip):
    w, h = 64, 9
    plan = plan_for(hip, w, h, 3)
    try:
        q = pp.matrices(w, h)["rig"]
        m = pp.make_map("random_50", 2, w, h, np.int16, 4)
        depth = torch.full((3, h, w), 7.0, device="cuda")
        xyz = torch.full((3, h, w, 3), 7.0, device="cuda")
        d, x = plan.reproject(dev(m), q, missing=-1.0, depth=depth, xyz=xyz)
        assert d is depth and x is xyz
        want_d, want_x, _ = ref.reproject(m, q, -1.0)
        same_floats(host(depth)[:2], want_d, -1.0, "depth")
        same_floats(host(xyz)[:2], want_x, -1.0, "xyz")
        assert (host(depth)[2] == 7.0).all() and (host(xyz)[2] == 7.0).all()     # the unused pair slot
        with pytest.raises(ValueError):
            plan.reproject(dev(m), q, depth=torch.zeros((2, h, w + 1), device="cuda"))
        with pytest.raises(ValueError):
            plan.reproject(dev(m.astype(np.int64)), q)
        with pytest.raises(ValueError):
            plan.reproject(dev(m), list(q)[:15])
        with pytest.raises(capi.StereoHipError, match="sm_reproject: d_depth and d_xyz are both NULL"):
            plan.reproject(dev(m), q, want_depth=False)
    finally:
        plan.close()


# ---------------------------------------------------------------------------
# cloud
# ---------------------------------------------------------------------------

CAPACITIES = ("all", "count", "count-1", 1, 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_point_cloud_at_every_size(hip, dtype):
    i = 0
    for (w, h) in pp.SIZES:
        qs = pp.matrices(w, h)
        for pairs, maxp in BATCHES:
            plan = plan_for(hip, w, h, maxp)
            try:
                for capacity in CAPACITIES:
                    name = list(qs)[i % len(qs)]
                    pattern = pp.PATTERNS[(i // 2) % len(pp.PATTERNS)]
                    gate = pp.Z_GATES[(i // 3) % 2]
                    m = pp.make_map(pattern, pairs, w, h, dtype, seed=i)
                    g = pp.gray(pairs, w, h, i) if i % 2 == 0 else None
                    check_cloud(plan, m, qs[name], g, gate, w * h if capacity == "all" else capacity, i % 3 != 0,
                                (w, h, pairs, maxp, name, pattern, gate, capacity))
                    i += 1
            finally:
                plan.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", [(41, 25), (683, 3)])
def test_point_cloud_every_pattern_and_capacity(hip, dtype, size):
    w, h = size
    plan = plan_for(hip, w, h, 2)
    try:
        qs = pp.matrices(w, h)
        for k, pattern in enumerate(pp.PATTERNS):
            m = pp.make_map(pattern, 2, w, h, dtype, seed=k)
            g = pp.gray(2, w, h, k)
            for j, capacity in enumerate(CAPACITIES):
                name = list(qs)[(k + j) % len(qs)]
                check_cloud(plan, m, qs[name], g if j % 2 == 0 else None, pp.Z_GATES[(k + j) % 2],
                            w * h if capacity == "all" else capacity, j % 2 == 1, (w, h, name, pattern, capacity))
    finally:
        plan.close()


def test_more_tiles_than_the_scan_has_lanes(hip):
    """263168 pixels = 257 tiles: k_cloud_scan's loop runs twice and carries the first turn's sum.  (The dense kernel
    takes its four-pixel path here: 65792 lanes in 257 workgroups, below the 1024 at which they begin to stride;
    tests/test_second_turns_gpu.py has the sizes at which they do.)"""
    w, h = pp.SCAN_LOOP_SIZE
    plan = plan_for(hip, w, h, 2)
    try:
        q = pp.matrices(w, h)["rig"]
        for k, (dtype, pattern) in enumerate(((np.int32, "random_50"), (np.int16, "random_99"), (np.int32, "last_only"))):
            m = pp.make_map(pattern, 2, w, h, dtype, seed=k)
            check_dense(plan, m, q, 0.0, pp.Z_GATES[k % 2], (True, True), True, (w, h, pattern, "dense"))
            counts = check_cloud(plan, m, q, pp.gray(2, w, h, k), pp.Z_GATES[k % 2], w * h, True, (w, h, pattern, "cloud"))
            check_cloud(plan, m, q, None, pp.Z_GATES[k % 2], "count-1", False, (w, h, pattern, "count-1"))
            assert min(counts) > 0
    finally:
        plan.close()


def test_default_capacity_and_count_only_call(hip):
    w, h = 37, 5
    plan = plan_for(hip, w, h, 1)
    try:
        q = pp.matrices(w, h)["rig"]
        m = pp.make_map("checkerboard", 1, w, h, np.int32, 2)
        pts, n, idx = plan.point_cloud(dev(m), q, want_index=True)
        want_p, want_i = ref.point_cloud(m[0], q)
        assert pts.shape == (1, w * h, 4) and idx.shape == (1, w * h) and int(n[0]) == len(want_i)
        assert np.array_equal(bits(host(pts)[0, :len(want_i)]), bits(want_p))
        assert np.array_equal(host(idx)[0, :len(want_i)], want_i)
        pts, n = plan.point_cloud(dev(m), q, capacity=0)
        assert pts.shape == (1, 0, 4) and int(n[0]) == len(want_i)
    finally:
        plan.close()


# ---------------------------------------------------------------------------
# every output is written where the definition says, and nothing else is
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_reprojection_writes_its_outputs_and_nothing_else(dtype):
    bad = []
    nq = 0
    for (w, h) in ((37, 5), (64, 9), (41, 25), (1024, 3)):
        qs = pp.matrices(w, h)
        for pairs, maxp in BATCHES:
            plan = Plan(w, h, 4, 1, "ghost", maxp)
            try:
                for off in (0, 4):                               # 256-byte aligned, and one element off it
                    name = list(qs)[nq % len(qs)]
                    q = capi.q16(qs[name])
                    gate = pp.Z_GATES[nq % 2]
                    lo, hi = (-INF, INF) if gate is None else gate
                    nq += 1
                    m = pp.make_map("random_50", pairs, w, h, dtype, seed=nq)
                    g = pp.gray(pairs, w, h, nq)
                    gm = guarded_input(m, "cuda", offset=off if dtype is np.int32 else off // 2, name="map")
                    gg = guarded_input(g, "cuda", offset=1 + nq % 3, name="gray")
                    tag = f"{w}x{h} {pairs}/{maxp} off {off} {name}"
                    # dense: depth, xyz and the count
                    depth = out((pairs, h, w), torch.int32, off, maxp, "depth")
                    xyz = out((pairs, h, w, 3), torch.int32, off, maxp, "xyz")
                    count = out((pairs,), torch.int32, off, maxp, "count")
                    bad += twice(tag + " dense", lambda run: lib.sm_reproject(
                        plan.h, P(gm.t), TYPE[dtype], q, lo, hi, -1.0, pairs, P(depth.t), P(xyz.t), P(count.t), stream()),
                        [depth, xyz, count], [gm])
                    want_d, want_x, want_n = ref.reproject(m, qs[name], -1.0, gate)
                    bad += expect(tag, depth, want_d.view(np.int32)) + expect(tag, xyz, want_x.view(np.int32))
                    bad += expect(tag, count, want_n)
                    # cloud: a capacity above every count, so that slots stay untouched
                    wants = [ref.point_cloud(m[p], qs[name], g[p], gate) for p in range(pairs)]
                    cap = max(len(i) for _, i in wants) + 5
                    pts = out((pairs, cap, 4), torch.int32, off, maxp, "points")
                    idx = out((pairs, cap), torch.int32, off, maxp, "index")
                    cnt = out((pairs,), torch.int32, 0, maxp, "count")
                    kept_poison = []

                    def cloud(run):
                        rc = lib.sm_point_cloud(plan.h, P(gm.t), TYPE[dtype], q, lo, hi, P(gg.t), pairs, cap, P(pts.t),
                                                P(idx.t), P(cnt.t), stream())
                        torch.cuda.synchronize()
                        for p in range(pairs):
                            k = len(wants[p][1])
                            ok = (pts.t[p, k:].view(torch.uint8) == POISON[run]).all() and \
                                 (idx.t[p, k:].view(torch.uint8) == POISON[run]).all()
                            kept_poison.append(bool(ok))
                        return rc
                    bad += twice(tag + " cloud", cloud, [pts, idx, cnt], [gm, gg], partial=[pts, idx])
                    if not all(kept_poison):
                        bad.append(f"{tag}: slots count <= k < capacity lost their poison")
                    for p in range(pairs):
                        k = len(wants[p][1])
                        if not np.array_equal(pts.value()[p, :k], wants[p][0].view(np.int32)):
                            bad.append(f"{tag}: records of pair {p} differ from the definition")
                        if not np.array_equal(idx.value()[p, :k], wants[p][1]):
                            bad.append(f"{tag}: indices of pair {p} differ from the definition")
                    bad += expect(tag, cnt, [len(i) for _, i in wants])
            finally:
                plan.close()
    report(bad)


# ---------------------------------------------------------------------------
# workspace, capture, determinism, refusals that need a plan
# ---------------------------------------------------------------------------

def test_workspace_is_reserved_lazily_and_by_the_formula(hip):
    w, h, maxp = 130, 33, 3
    plan = plan_for(hip, w, h, maxp)
    try:
        base, describe, geometry = plan.workspace_bytes(), plan.describe(), plan.geometry()
        q = pp.matrices(w, h)["rig"]
        m = dev(pp.make_map("random_50", 2, w, h, np.int32, 1))
        plan.reproject(m, q, want_xyz=True, want_count=True)
        torch.cuda.synchronize()
        assert (plan.workspace_bytes(), plan.describe(), plan.geometry()) == (base, describe, geometry)
        need = ref.workspace_bytes(w, h, maxp)
        assert need == 4 * maxp * 5
        plan.reserve_cloud()
        plan.reserve_cloud()                                    # idempotent
        assert plan.workspace_bytes() == base + need
        plan.point_cloud(m, q)
        assert (plan.workspace_bytes(), plan.describe(), plan.geometry()) == (base + need, describe, geometry)
    finally:
        plan.close()
    plan = plan_for(hip, w, h, maxp)
    try:
        plan.point_cloud(m, q)                                  # the first call reserves
        assert plan.workspace_bytes() == base + need
    finally:
        plan.close()


def test_refusals_that_need_a_plan(hip):
    w, h = 16, 4
    plan = plan_for(hip, w, h, 2)
    try:
        q = capi.q16(pp.matrices(w, h)["rig"])
        buf = torch.zeros(4096, dtype=torch.int32, device="cuda")
        a = buf.data_ptr()
        vp = C.c_void_p
        base = plan.workspace_bytes()

        def refused(rc, text):
            assert rc == capi.SM_ERR_ARG and text in lib.sm_last_error(), lib.sm_last_error()
        for pairs in (0, 3, -1):
            refused(lib.sm_reproject(plan._h, vp(a), 0, q, -INF, INF, 0.0, pairs, vp(a + 4096), None, None, None),
                    b"sm_reproject: pairs %d outside 1..2" % pairs)
            refused(lib.sm_point_cloud(plan._h, vp(a), 0, q, -INF, INF, None, pairs, 4, vp(a + 4096), None, vp(a + 8192), None),
                    b"sm_point_cloud: pairs %d outside 1..2" % pairs)
        n = w * h * 4                                           # bytes of one int32 map
        refused(lib.sm_reproject(plan._h, vp(a), 0, q, -INF, INF, 0.0, 1, vp(a + n - 4), None, None, None),
                b"sm_reproject: an output overlaps an input")
        refused(lib.sm_reproject(plan._h, vp(a + 4096), 1, q, -INF, INF, 0.0, 2, vp(a + 4096 + n - 4), None, None, None),
                b"sm_reproject: an output overlaps an input")
        refused(lib.sm_reproject(plan._h, vp(a), 0, q, -INF, INF, 0.0, 1, vp(a + 4096), vp(a + 4096 + n - 4), None, None),
                b"sm_reproject: outputs overlap")
        refused(lib.sm_reproject(plan._h, vp(a), 0, q, -INF, INF, 0.0, 1, None, vp(a + 4096), vp(a + 4096 + 3 * n - 4), None),
                b"sm_reproject: outputs overlap")
        refused(lib.sm_point_cloud(plan._h, vp(a), 0, q, -INF, INF, None, 1, 8, vp(a + n - 16), None, vp(a + 8192), None),
                b"sm_point_cloud: an output overlaps an input")
        refused(lib.sm_point_cloud(plan._h, vp(a), 0, q, -INF, INF, vp(a + 4096), 1, 8, vp(a + 8192), vp(a + 4096 + w * h - 4),
                                   vp(a + 12288), None), b"sm_point_cloud: an output overlaps an input")
        refused(lib.sm_point_cloud(plan._h, vp(a), 0, q, -INF, INF, None, 1, 8, vp(a + 4096), vp(a + 4096 + 8 * 16 - 4),
                                   vp(a + 8192), None), b"sm_point_cloud: outputs overlap")
        refused(lib.sm_point_cloud(plan._h, vp(a), 0, q, -INF, INF, None, 2, 8, vp(a + 4096), None, vp(a + 4096 + 2 * 8 * 16 - 4),
                                   None), b"sm_point_cloud: outputs overlap")
        torch.cuda.synchronize()
        assert plan.workspace_bytes() == base and not buf.any()
    finally:
        plan.close()


def test_capture_refusal_and_replays(hip):
    w, h = 130, 33
    plan = plan_for(hip, w, h, 2)
    try:
        qs = pp.matrices(w, h)
        q, q2 = capi.q16(qs["rig"]), capi.q16(qs["dense"])
        base = plan.workspace_bytes()
        cap = w * h
        m = torch.zeros((2, h, w), dtype=torch.int16, device="cuda")
        g = dev(pp.gray(2, w, h, 1))
        depth = torch.zeros((2, h, w), device="cuda")
        xyz = torch.zeros((2, h, w, 3), device="cuda")
        n_dense = torch.zeros(2, dtype=torch.int32, device="cuda")
        pts = torch.zeros((2, cap, 4), device="cuda")
        idx = torch.zeros((2, cap), dtype=torch.int32, device="cuda")
        n_cloud = torch.zeros(2, dtype=torch.int32, device="cuda")

        def dense():
            return lib.sm_reproject(plan._h, P(m), capi.SM_MAP_I16, q, 2.0, 40.0, INF, 2, P(depth), P(xyz), P(n_dense),
                                    plan._stream())

        def cloud():
            return lib.sm_point_cloud(plan._h, P(m), capi.SM_MAP_I16, q, 2.0, 40.0, P(g), 2, cap, P(pts), P(idx), P(n_cloud),
                                      plan._stream())
        g0 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g0, capture_error_mode="thread_local"):
            assert cloud() == capi.SM_ERR_ARG
            message = lib.sm_last_error().decode()
            capi.check(dense())                                  # the capture goes on
        assert "sm_point_cloud" in message and "sm_plan_reserve_cloud" in message
        assert plan.workspace_bytes() == base
        first = pp.make_map("random_50", 2, w, h, np.int16, 9)
        m.copy_(dev(first))
        g0.replay()
        torch.cuda.synchronize()
        same_floats(host(depth), ref.reproject(first, qs["rig"], INF, (2.0, 40.0))[0], INF, "first capture")
        plan.reserve_cloud()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            capi.check(dense())
            capi.check(cloud())
        other = dev(pp.make_map("all_valid", 1, w, h, np.int32, 3))
        for rep in range(3):
            fresh = pp.make_map(("random_1", "checkerboard", "random_99")[rep], 2, w, h, np.int16, 20 + rep)
            m.copy_(dev(fresh))
            pts.view(torch.int32).fill_(FILL)
            idx.fill_(-1)
            n_dense.fill_(12345)
            n_cloud.fill_(54321)
            graph.replay()
            torch.cuda.synchronize()
            want_d, want_x, want_n = ref.reproject(fresh, qs["rig"], INF, (2.0, 40.0))
            same_floats(host(depth), want_d, INF, rep)
            same_floats(host(xyz), want_x, INF, rep)
            assert host(n_dense).tolist() == want_n.tolist() == host(n_cloud).tolist(), rep
            for p in range(2):
                want_p, want_i = ref.point_cloud(fresh[p], qs["rig"], host(g)[p], (2.0, 40.0))
                k = len(want_i)
                assert np.array_equal(bits(host(pts)[p, :k]), bits(want_p)) and (bits(host(pts)[p, k:]) == FILL).all(), rep
                assert np.array_equal(host(idx)[p, :k], want_i) and (host(idx)[p, k:] == -1).all(), rep
            # an eager call with other arguments between the replays (it shares the workspace, not the captured arguments)
            plan.point_cloud(other, q2, capacity=7, want_index=True)
            plan.reproject(other, q2, want_xyz=True, missing=1.0)
    finally:
        plan.close()


def test_fifty_launches_give_identical_bytes(hip):
    w, h = 256, 9
    plan = plan_for(hip, w, h, 2)
    try:
        q = pp.matrices(w, h)["dense"]
        m = dev(pp.make_map("random_50", 2, w, h, np.int32, 6))
        g = dev(pp.gray(2, w, h, 6))
        first = None
        for _ in range(50):
            depth, xyz, n = plan.reproject(m, q, want_xyz=True, want_count=True, missing=INF)
            pts = torch.full((2, w * h, 4), FILL, dtype=torch.int32, device="cuda").view(torch.float32)
            _, n2, idx = plan.point_cloud(m, q, g, want_index=True, points=pts)
            now = [t.clone() for t in (depth.view(torch.int32), xyz.view(torch.int32), n, pts.view(torch.int32), n2)]
            now.append(torch.stack([idx[p, :int(n2[p])].sum() for p in range(2)]))
            if first is None:
                first = now
            assert all(torch.equal(a, b) for a, b in zip(first, now))
    finally:
        plan.close()


# ---------------------------------------------------------------------------
# the whole chain: raw cameras -> rectify -> match + check -> mask -> speckle -> interpolate -> reproject
# ---------------------------------------------------------------------------

def moved(img, dx, dy, border):
    """out(x + dx, y + dy) = img(x, y), `border` where nothing lands"""
    h, w = img.shape
    res = np.full((h, w), border, np.uint8)
    ys, xs = np.arange(h), np.arange(w)
    ys, xs = ys[(ys + dy >= 0) & (ys + dy < h)], xs[(xs + dx >= 0) & (xs + dx < w)]
    res[np.ix_(ys + dy, xs + dx)] = img[np.ix_(ys, xs)]
    return res


@pytest.mark.parametrize("mode", ["toroidal", "ghost"])
def test_raw_scene_through_the_chain_to_depth_and_a_cloud(hip, mode):
    w, h, d, sw = 160, 64, 24, 5
    left, right = make_pair(w, h, d, seed=11)
    raw_l, raw_r = moved(left, 2, 3, 255), moved(right, -1, -2, 0)
    ml = rp.translation_map(w, h, 2, 3, "rel16")
    mx, my = rr.positions(rp.translation_map(w, h, -1, -2, "abs32"))
    mr = rr.rel_map(mx + (np.arange(h)[:, None] % 3) * 8, my)
    rl, rright, vl, vr = rr.rectify(raw_l[None], raw_r[None], ml, mr, "bilinear", 0)
    e = clr.expected(rl[0], rright[0], d, sw, mode, "sad", 1)
    masked = rr.valid_mask(e["checked"], vl[0] & vr[0])
    speckled, _ = fr.speckle(masked, 20, 1)
    cls = ir.classify(speckled, e["web_right"], d, mode)
    filled = ir.interpolate(speckled, cls)
    first, second, t = pp.rig(w, h, offset=-0.5)
    want_q = ref.reprojection_matrix(first, second, t)
    gate = (0.5, 150.0)
    want_d, want_x, want_n = ref.reproject(filled[None], want_q, np.nan, gate)
    want_p, want_i = ref.point_cloud(filled, want_q, rl[0], gate)
    assert 0 < int(want_n[0]) < w * h
    plan = hip.StereoPlan(w, h, d, sw, mode)
    try:
        q = hip.reprojection_matrix(dict(first, fx=1.0, fy=1.0, cx=0.0, cy=0.0), dict(second, fx=1.0, fy=1.0, cx=0.0, cy=0.0), t)
        assert np.array_equal(np.array(q).view(np.uint64), want_q.view(np.uint64))
        gl, gr, gvl, gvr = plan.rectify(dev(raw_l), dev(raw_r), dev(ml), dev(mr), "bilinear", 0, want_valid=True)
        res = plan.cost_lr(gl, gr, "sad", max_diff=1, want_right=True)
        got = plan.valid_mask(res.web, gvl & gvr)
        got = plan.speckle_filter(got, 20, 1, out=got)
        got = plan.interpolate(got, plan.occlusion_classify(got, res.web_right))
        assert np.array_equal(host(got)[0], filled)
        depth, xyz, n = plan.reproject(got, q, want_xyz=True, missing=float("nan"), z_range=gate, want_count=True)
        same_floats(host(depth), want_d, math.nan, "depth")
        same_floats(host(xyz), want_x, math.nan, "xyz")
        assert host(n).tolist() == want_n.tolist()
        pts, n2, idx = plan.point_cloud(got, q, gray=gl, z_range=gate, want_index=True)
        k = int(n2[0])
        assert k == len(want_i) and np.array_equal(bits(host(pts)[0, :k]), bits(want_p))
        assert np.array_equal(host(idx)[0, :k], want_i)
    finally:
        plan.close()
