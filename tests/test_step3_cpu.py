"""Step 3 on maps WITH holes, on the CPU: the restatement (oracle.fill_web_holes /
oracle.draw_contour_map) against what the reference's own functions made of every map of
tests/step3_patterns.py (tests/golden/step3/, written by tests/golden/make_golden.py --step3 from
both src/stereo.c and src/stereo-ghost.c), and the generators against what they are named for.

The reference's SWAP (src/util.h:27-32) is a no-op (its local `tmp` shadows the buffer of that
name), so each of its `times` sweeps reads the unfilled map: times >= 1 fills once."""
import numpy as np
import pytest

from tests import oracle
from tests import step3_patterns as sp
from tests.conftest import GOLDEN_DIR

STEP3_DIR = GOLDEN_DIR / "step3"
SOURCES = {"stereo": "tor", "stereo-ghost": "gh"}       # reference source file -> fixture key suffix


def fixture(name):
    z = np.load(STEP3_DIR / f"{name}.npz")
    return {k: z[k] for k in z.files}


def one_sweep(web):
    """the reference's step 3 written out in numpy, for times >= 1: every 0 pixel becomes
    trunc((r + u + l + d) / 4) of the UNFILLED map, neighbours at flat offsets +-1 / +-w"""
    flat = web.astype(np.int64).ravel()
    n, w = flat.size, web.shape[1]
    p = np.flatnonzero(flat == 0)
    nb = lambda q: np.where((q >= 0) & (q < n), flat[np.clip(q, 0, n - 1)], 0)
    s = nb(p + 1) + nb(p + w) + nb(p - 1) + nb(p - w)
    out = flat.copy()
    out[p] = np.trunc(s / 4).astype(np.int64)           # |s| < 2^31: exact in a double
    return out.reshape(web.shape).astype(np.int32)


def test_every_case_has_a_fixture():
    assert sorted(p.stem for p in STEP3_DIR.glob("*.npz")) == sorted(sp.CASES)


@pytest.mark.parametrize("name", sorted(sp.CASES))
def test_fixture_input_is_the_generator(name):
    z = fixture(name)
    web, times, lines = sp.case(name)
    assert np.array_equal(z["web"], web) and z["web"].dtype == np.int32, name
    assert z["params"].tolist() == [times, lines], name


@pytest.mark.parametrize("source", sorted(SOURCES))
@pytest.mark.parametrize("name", sorted(sp.CASES))
def test_restatement_equals_the_reference(name, source):
    z = fixture(name)
    sfx = SOURCES[source]
    times, lines = z["params"].tolist()
    filled = oracle.fill_web_holes(z["web"], times)
    assert np.array_equal(filled, z[f"filled_{sfx}"]), (name, source, "filled")
    if int(z[f"rc_{sfx}"]) == -8:                       # the reference trapped on the zero interval
        with pytest.raises(ZeroDivisionError):
            oracle.draw_contour_map(filled, lines)
    else:
        assert int(z[f"rc_{sfx}"]) == 0, (name, source)
        assert np.array_equal(oracle.draw_contour_map(filled, lines), z[f"contour_{sfx}"]), (name, source, "contour")
    # and the rule written out in numpy, independently of the restatement
    want = one_sweep(z["web"]) if times >= 1 else z["web"]
    assert np.array_equal(z[f"filled_{sfx}"], want), (name, source, "numpy")


def test_reference_fills_once_whatever_times_is():
    """the fixtures of one map at several `times`: every times >= 1 gives the same map, times 0 the input"""
    groups = {}
    for name, (fn, w, h, seed, times, _) in sp.CASES.items():
        groups.setdefault((fn.__name__, w, h, seed), []).append((times, name))
    multi = 0
    for key, members in groups.items():
        filled = {t: fixture(n)["filled_tor"] for t, n in members}
        web = fixture(members[0][1])["web"]
        ones = [f for t, f in filled.items() if t >= 1]
        assert all(np.array_equal(f, ones[0]) for f in ones), key
        if 0 in filled:
            assert np.array_equal(filled[0], web), key
        if len({t % 2 for t in filled if t >= 1}) == 2:
            multi += 1
            assert not np.array_equal(ones[0], web), key      # holes were filled
    assert multi >= 4


def test_generators_reach_what_they_are_named_for():
    shapes, times_seen, trapped = set(), set(), []
    for name in sp.CASES:
        z = fixture(name)
        web, (times, lines) = z["web"], z["params"].tolist()
        h, w = web.shape
        assert (web[0] != 0).all() and (web[-1] != 0).all(), (name, "border rows stay hole-free")
        assert (np.abs(web.astype(np.int64)) < sp.LIMIT).all(), name
        assert (web == 0).any(), name
        shapes.add((w * h) % 4)
        times_seen.add(times)
        if int(z["rc_tor"]) == -8:
            trapped.append(name)
        assert int(z["rc_tor"]) == int(z["rc_gh"]) and np.array_equal(z["filled_tor"], z["filled_gh"]), name
    assert shapes == {0, 1, 2, 3}
    assert {0, 1, 2, 3, 32, 101} <= times_seen
    assert {"zero_after_fill_t2", "zero_unfilled_t0", "zero_lines_t2"} <= set(trapped)

    # holes at x = 0 and x = w - 1 whose flat neighbour across the row end (x - 1 / x + 1) is a
    # pixel of the previous / next row with a value that decides the result: a fill that wrapped
    # within the row would differ there
    z = fixture("edge_columns_t2")
    web, filled = z["web"], z["filled_tor"]
    h, w = web.shape
    wrapped = web.copy()
    for y, x in np.argwhere(web == 0):
        r = web[y, (x + 1) % w]
        l = web[y, (x - 1) % w]
        u = web[y + 1, x] if y + 1 < h else 0
        d = web[y - 1, x] if y > 0 else 0
        wrapped[y, x] = int((int(r) + int(u) + int(l) + int(d)) / 4)
    for x in (0, w - 1):
        assert (web[1:h - 1, x] == 0).any()
        assert (wrapped[:, x] != filled[:, x]).any(), x

    # persisting holes: 0 after filling, with neighbours that are not all 0 (|sum| < 4)
    for name in ("persisting_t2", "big_block_t32", "lr_scene_t32"):
        z = fixture(name)
        assert (z["filled_tor"] == 0).any(), name
    z = fixture("persisting_t2")
    web = z["web"].astype(np.int64)
    pad = np.pad(web.ravel(), z["web"].shape[1])
    w = z["web"].shape[1]
    stay = [p for p in np.flatnonzero((web.ravel() == 0) & (z["filled_tor"].ravel() == 0))
            if 0 < pad[p + w + 1] + pad[p + w - 1] + pad[p] + pad[p + 2 * w] < 4]
    assert stay

    # holes whose neighbours sum to a negative value that is not a multiple of 4: trunc(s / 4)
    # (C's /) and s >> 2 differ there
    differ = 0
    for name in ("negative_t2", "negative_t3", "extreme_t2"):
        z = fixture(name)
        web = z["web"]
        floor = web.astype(np.int64).ravel().copy()
        flat = web.astype(np.int64).ravel()
        n, w = flat.size, web.shape[1]
        for p in np.flatnonzero(flat == 0):
            s = sum(flat[q] for q in (p + 1, p + w, p - 1, p - w) if 0 <= q < n)
            floor[p] = s >> 2
        differ += int((floor != z["filled_tor"].ravel()).sum())
    assert differ > 20

    # the zero interval appears only after filling: the unfilled map's interval is not 0
    z = fixture("zero_after_fill_t2")
    web, lines = z["web"], int(z["params"][1])
    assert (int(web.max()) - int(web.min())) // lines > 0
    assert int(z["filled_tor"].max()) == int(z["filled_tor"].min())

    # a real left-right-checked map: many holes, spread over the image
    web = fixture("lr_scene_t32")["web"]
    assert 0.05 < (web == 0).mean() < 0.6 and (web[1:-1, 0] == 0).any() and (web[1:-1, -1] == 0).any()


def test_a_map_without_a_positive_value_tells_a_maximum_that_starts_at_zero():
    """(the mutation audit's Z4: k_minmax_zero with its running maximum started at 0 passed tests/test_step3_gpu.py)"""
    mistake = sp.MISTAKES[0]
    for w, h in sp.NO_POSITIVE_SHAPES:
        web = sp.no_positive(w, h, seed=w)
        assert (web < 0).all()
        assert sp.min_max_with(web, mistake) != (int(web.min()), int(web.max()))
        # and the contour depends on it: the interval (max - min) / lines differs
        lo, hi = int(web.min()), int(web.max())
        assert (hi - lo) // 10 != (0 - lo) // 10, (w, h)
    # every map the GPU module gave the reductions before holds a value >= 0 in every pair: a fixture's own map and
    # filled map, their offset copies (the sign is kept, zeros stay) and the hole-free copy; 100 .. 5000 elsewhere
    for name in sp.CASES:
        z = fixture(name)
        for m in (z["web"], z["filled_tor"]):
            assert int(m.max()) >= 0, name
            assert sp.min_max_with(m, mistake) == (int(m.min()), int(m.max())), name
            assert (m > 0).any() or (m == 0).any(), name


@pytest.mark.skipif(not (oracle.step3_ref_available() and oracle.step3_ref_available(asan=True)),
                    reason="oracle/_ref/step3-ref* not built: the reference's sources are not on this machine "
                           "(the fixtures pin it instead)")
def test_reference_drivers_still_make_the_fixtures():
    """the compiled reference's own step 3, re-run on every generator (both source files, and the
    AddressSanitizer / UBSan build: clean), reproduces the stored fixtures"""
    import sys
    sys.path.insert(0, str(GOLDEN_DIR))
    import make_golden
    for name in sp.CASES:
        web, times, lines = sp.case(name)
        got = make_golden.step3_reference(web, times, lines)
        z = fixture(name)
        assert sorted(got) == sorted(z), name
        for k, v in got.items():
            assert np.array_equal(np.asarray(v), z[k]), (name, k)


@pytest.mark.skipif(not oracle.step3_ref_available(asan=True),
                    reason="oracle/_ref/step3-ref*-asan not built: the reference's sources are not on this machine")
@pytest.mark.parametrize("source", sorted(SOURCES))
def test_sanitizer_driver_sees_border_row_holes(source):
    """a hole in row 0 or row h - 1 makes the reference read outside the map: the sanitizer build
    must say so (which is why those rows are pinned to the restatement only)"""
    web, times, lines = sp.case("mixed_t2")
    assert oracle.run_step3_reference(web, times, lines, source, asan=True)["returncode"] == 0
    for y, x in ((0, 5), (web.shape[0] - 1, 7), (0, 0), (web.shape[0] - 1, web.shape[1] - 1)):
        holed = web.copy()
        holed[y, x] = 0
        r = oracle.run_step3_reference(holed, times, lines, source, asan=True)
        assert r["returncode"] != 0 and "heap-buffer-overflow" in r["stderr"], (source, y, x)
