"""The edge kernels on near-tie side sums (tests/edge_tie_patterns.py): every pair of the f32 prefilter's band, in
every orientation, decides a centre pixel, and the centres reach every quad position, lane 0 and 63 of a wave,
every row of a strip, the seams between waves and workgroups, ghost SEL and interior waves and the toroidal wrap.

Per geometry one plan runs every threshold in sequence (and returns to the first: the tables are rebuilt and the
cache keyed by threshold must follow), each as one batched launch of all the geometry's image pairs.  The u8 edge
images must equal the oracle's bit for bit, and the packed image the match consumes is checked through match_wta's
web and best against the oracle's hot path on the oracle's edges.  test_edge_ties_cpu.py proves what the images
reach."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import edge_tie_patterns as et
from tests import oracle

pytestmark = pytest.mark.gpu
MODES = ["toroidal", "ghost"]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def explain(img, mode, t, x, y, kernel, half, stacked, desc):
    """what a wrong pixel stands for: its deciding near-tie pair (or its four side-sum pairs) and position classes"""
    h, w = img.shape
    A, B = et.orientation_sums(img, mode)
    hit = [(o, a, b) for xx, yy, o, a, b in et.deciding_centres(img, mode, t).tolist() if (xx, yy) == (x, y)]
    what = (f"near-tie {et.ORIENTATION_NAMES[hit[0][0]]} (Sa, Sb) = {hit[0][1:]}" if hit else
            "sums " + ", ".join(f"{et.ORIENTATION_NAMES[o]} {(int(A[o, y, x]), int(B[o, y, x]))}" for o in range(4)))
    cls = sorted(et.position_classes(x, y, w, h, mode, kernel, half, 32, stacked))
    return f"T={t!r} pixel ({x}, {y}): {what}; positions {cls}; {desc}"


def find_edges(plan, left, right, t, unaligned):
    if not unaligned:
        return plan.find_all_edges(dev(left), dev(right), t)
    # inputs one and three bytes past a 4-byte boundary: sm_find_edges must leave k_edges_ext4 to k_edges_ext
    from stereomatching_amd.capi import check, lib
    n = left.size
    raw_l = torch.empty(n + 8, dtype=torch.uint8, device="cuda")
    raw_r = torch.empty(n + 8, dtype=torch.uint8, device="cuda")
    l_un = raw_l[1:1 + n].view(left.shape)
    r_un = raw_r[3:3 + n].view(right.shape)
    l_un.copy_(dev(left))
    r_un.copy_(dev(right))
    assert l_un.data_ptr() % 4 and r_un.data_ptr() % 4
    el = torch.empty(left.shape, dtype=torch.uint8, device="cuda")
    er = torch.empty(right.shape, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(lib.sm_find_edges(plan._h, C.c_void_p(l_un.data_ptr()), C.c_void_p(r_un.data_ptr()), float(t),
                            left.shape[0], C.c_void_p(el.data_ptr()), C.c_void_p(er.data_ptr()), st))
    return el, er


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,w,h,d,sw,kernel,shape,options,unaligned", et.GEOMETRIES,
                         ids=[g[0] for g in et.GEOMETRIES])
def test_edge_kernels_on_near_ties(hip, mode, name, w, h, d, sw, kernel, shape, options, unaligned):
    half = sw // 2
    batches = {t: et.batch(w, h, mode, t) for t in et.GPU_THRESHOLDS}
    pairs = max(len(b[0]) for b in batches.values())
    plan = hip.StereoPlan(w, h, d, sw, mode, max_pairs=pairs, options=options)
    g = plan.geometry()
    desc = f"{name} {mode}: {plan.describe()}"
    assert g["pad_l"] == 32, desc                        # the tiled match kernels' padding (position classes)
    assert g["edge_rows_per_wave"] == (4 if w % 4 == 0 else 32), desc
    stacked = shape == "stacked"
    if kernel == "ext4":
        assert w % 4 == 0 and not unaligned and not options
        assert et.edges4_stacked(w, d, sw) == stacked, (desc, "the host takes the other block shape")
    else:
        assert w % 4 or unaligned or (options or {}).get("edge_kernel") == 1
    for t in (*et.GPU_THRESHOLDS, et.GPU_THRESHOLDS[0]):
        left, right = batches[t]
        n = len(left)
        el, er = find_edges(plan, left, right, t, unaligned)
        web, best = plan.match_wta(n)
        el, er, web, best = host(el), host(er), host(web), host(best)
        for i in range(n):
            oel = oracle.find_all_edges(left[i], t, mode)
            oer = oracle.find_all_edges(right[i], t, mode)
            for side, got, want, img in ((0, el[i], oel, left[i]), (1, er[i], oer, right[i])):
                if not np.array_equal(got, want):
                    y, x = np.argwhere(got != want)[0]
                    pytest.fail(f"edges of image {i} side {side} differ at {int((got != want).sum())} pixels; first: "
                                + explain(img, mode, t, int(x), int(y), kernel, half, stacked, desc))
            ob, ow = oracle.hot_path(oel, oer, d, sw, mode)
            if not (np.array_equal(web[i], ow) and np.array_equal(best[i], ob)):
                y, x = np.argwhere((web[i] != ow) | (best[i] != ob))[0]
                pytest.fail(f"packed edges of pair {i}: web / best differ from the oracle's at ({x}, {y}); "
                            f"T={t!r}; {desc}")
    plan.close()
