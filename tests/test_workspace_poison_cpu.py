"""The poison words and the cases of test_workspace_poison_gpu.py are informative: from the CPU definitions alone.

A stage whose expected output were all zero, or its own input, would pass whatever the workspace held; two settings of
the interleaving test with the same expected result could not show stale state."""
import numpy as np
import pytest

from tests import filter_reference as fr
from tests import interp_patterns as ip
from tests import interp_reference as ir
from tests import reproject_reference as rref
from tests import workspace_poison_cases as wc


def test_the_words_are_the_listed_ones_in_their_order():
    assert wc.WORDS == (0x00000001, 0x00000000, 0x7FFF7FFF, 0x80008000, 0xA5A5A5A5, 0xFFFFFFFF)
    # the first word is an in-range int32 index on every shape: pixels, tiles, lines, chunks, shifts
    sizes = [(w, h) for cases in wc.IMAGE_CASES.values() for w, h, _, _ in cases] + list(wc.INTERP_SIZES) + [wc.CLOUD_BIG]
    assert all(w * h > 1 and w + h - 1 > 1 for w, h in sizes)
    assert all(d > 1 for cases in wc.IMAGE_CASES.values() for _, _, d, _ in cases)
    assert (wc.CLOUD_BIG[0] * wc.CLOUD_BIG[1] + 1023) // 1024 > 256     # more tiles than k_cloud_scan has lanes
    assert set(wc.IMAGE_CASES) == set(wc.MODES)
    assert {d for cases in wc.IMAGE_CASES.values() for _, _, d, _ in cases} == {16, 48}
    assert any(h > 2 * ip.SEG_H for _, h in wc.INTERP_SIZES) and any(w > 2 * ip.CHUNK_W for w, _ in wc.INTERP_SIZES)


def informative(name, out, *inputs):
    out = np.asarray(out)
    assert out.any(), f"{name}: all zero"
    for i in inputs:
        assert out.shape != np.asarray(i).shape or not np.array_equal(out, i), f"{name}: equals its input"


def differ_per_pair(name, a):
    assert all(not np.array_equal(a[0], a[q]) for q in range(1, len(a))), f"{name}: the same for two pairs"


@pytest.mark.parametrize("mode", wc.MODES)
def test_image_stage_results_are_neither_zero_nor_their_input(mode):
    for w, h, d, sw in wc.IMAGE_CASES[mode]:
        left, right = wc.images(w, h, d)
        differ_per_pair("left", left)
        tag = f"{mode} {w}x{h} D={d} S={sw}"
        todo = [("edge", wc.edge_expected(mode, w, h, d, sw, 1))]
        todo += [(c, wc.cost_expected(mode, w, h, d, sw, c, 1)) for c in ("sad", "ssd")]
        todo += [(f"census {c}", wc.census_expected(mode, w, h, d, sw, c, 1)) for c in (5, 7)]
        todo += [(f"sgm {p}", wc.sgm_expected(mode, w, h, d, sw, c, p1, p2, p, 1)) for p, c, p1, p2 in ((8, 7, 10, 120), (4, 5, 3, 40))]
        for name, e in todo:
            # (ghost border, two rows: every pixel touches the halo and is an edge whatever the image holds, so the edge
            # matcher's maps are the same for every pair there; they are still neither zero nor constant)
            same_edges = name == "edge" and mode == "ghost" and h == 2
            for k in ("web", "web_right", "checked"):
                informative(f"{tag} {name} {k}", e[k], left, right)
                if not same_edges:
                    differ_per_pair(f"{tag} {name} {k}", e[k])
            if same_edges:
                assert len(np.unique(e["web"])) > 2, (tag, name)
                continue
            # the check rejects some pixels and keeps some: a count that is neither 0 nor all
            assert all(0 < int(n) < w * h for n in e["rejected"]), (tag, name, e["rejected"])
            assert len({int(v) for v in np.unique(e["web"])}) > 2, (tag, name)
            if "sub" in e:
                informative(f"{tag} {name} sub", e["sub"])


@pytest.mark.parametrize("dtype", [np.int32, np.int16])
def test_map_stage_results_are_neither_zero_nor_their_input(dtype):
    for w, h in wc.MAP_SIZES:
        src, kept, removed = wc.speckle_case(w, h, dtype)
        informative(f"speckle {w}x{h}", kept, src)
        assert all(0 < int(n) < int((m != 0).sum()) for n, m in zip(removed, src))
        for gi in (0, 1):
            m, g, q, wants = wc.cloud_case(w, h, dtype, gi, True)
            counts = [len(i) for _, i in wants]
            assert all(3 < n < w * h for n in counts), (w, h, gi, counts)      # (a capacity of count - 3 is positive)
            assert len(set(counts)) > 1
        assert [len(i) for _, i in wc.cloud_case(w, h, dtype, 0, True)[3]] != [len(i) for _, i in wc.cloud_case(w, h, dtype, 1, True)[3]]
    for w, h in wc.INTERP_SIZES:
        src, cls, want, filled = wc.interp_case(w, h, dtype)
        informative(f"interpolate {w}x{h}", want, src)
        assert all(int(n) > 0 for n in filled)
        plain = np.stack([ir.interpolate(m) for m in src])
        assert not np.array_equal(plain, want)                    # the classes change the result
        # pair 0 (the batch of one) has row chunks and, where the map has several, line segments without a valid pixel
        a = src[0]
        chunks = [a[y, c:c + ip.CHUNK_W] for y in range(h) for c in range(0, w, ip.CHUNK_W)]
        assert any(not c.any() for c in chunks) and any(c.any() for c in chunks)
        if h > ip.SEG_H:
            segs = [a[s:s + ip.SEG_H, x] for x in range(w) for s in range(0, h, ip.SEG_H)]
            assert any(not s.any() for s in segs) and any(s.any() for s in segs)


def test_the_large_cloud_maps_keep_every_pixel_and_none():
    w, h = wc.CLOUD_BIG
    full, none, q, (records, index) = wc.cloud_big_case()
    assert len(index) == w * h and np.array_equal(index, np.arange(w * h))
    assert len(rref.point_cloud(none, q, None, None)[1]) == 0
    assert rref.reproject(full[None], q)[2].tolist() == [w * h] and rref.reproject(none[None], q)[2].tolist() == [0]


def test_the_two_settings_of_every_interleaved_stage_differ():
    c = wc.INTERLEAVE
    w, h, d, sw = c["size"]
    mode, mp, md = c["mode"], c["max_pairs"], c["max_diff"]
    cen = [wc.census_expected(mode, w, h, d, sw, cw, md, pairs=mp)["checked"] for cw in c["census"]]
    assert not np.array_equal(*cen)
    sgm = [wc.sgm_expected(mode, w, h, d, sw, 7, p1, p2, paths, md, pairs=mp)["checked"] for paths, p1, p2 in c["sgm"]]
    assert not np.array_equal(*sgm)
    smap = wc.speckle_case(w, h, np.int32, pairs=mp)[0]
    spk = [np.stack([fr.speckle(m, *s)[0] for m in smap]) for s in c["speckle"]]
    assert not np.array_equal(*spk) and all(s.any() for s in spk)
    clouds = [[len(i) for _, i in wc.cloud_case(w, h, np.int32, gi, True, pairs=mp)[3]] for gi in (0, 1)]
    assert clouds[0] != clouds[1] and all(n > 0 for n in clouds[0] + clouds[1])
    runs = [wc.edge_expected(mode, w, h, d, sw, md, thr=t, pairs=mp)["web"] for t in c["thresholds"]]
    assert not np.array_equal(*runs)
    # and the stages that share the mirrored-order map leave different maps in it
    edge = wc.edge_expected(mode, w, h, d, sw, md, pairs=mp)["web_right"]
    cost = wc.cost_expected(mode, w, h, d, sw, c["cost"], md, pairs=mp)["web_right"]
    cen_r = wc.census_expected(mode, w, h, d, sw, 7, md, pairs=mp)["web_right"]
    assert not np.array_equal(edge, cost) and not np.array_equal(cost, cen_r) and not np.array_equal(edge, cen_r)
