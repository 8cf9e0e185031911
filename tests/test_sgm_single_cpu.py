"""SGM's left-right check from one aggregated volume, CPU side: the C ABI declares, binds and exports the two entries and
refuses bad arguments before it touches a device; the vectorised numpy definition (tests/sgm_single_reference.py) agrees
with a loop over (u, d); the identities the GPU tests lean on hold."""
import ctypes as C

import numpy as np
import pytest

from tests import sgm_reference as sr
from tests import sgm_single_patterns as sp
from tests import sgm_single_reference as ss

NEW = ("sm_sgm_wta_both", "sm_sgm_lr_single")
MODES = ["toroidal", "ghost"]


def pair(w, h, seed, levels=256):
    rng = np.random.default_rng(seed)
    return rng.integers(0, levels, (h, w)).astype(np.uint8), rng.integers(0, levels, (h, w)).astype(np.uint8)


def periodic_pair(w=64, h=6, period=8, seed=5):
    """L = R, periodic in x: S(x, d) = S(x, d + period) exactly (toroidal, period | W)"""
    tile = np.random.default_rng(seed).integers(0, 256, (h, period)).astype(np.uint8)
    img = np.tile(tile, (1, w // period))
    return img, img.copy()


def test_new_symbols_are_declared_bound_and_exported():
    from stereomatching_amd import capi
    syms = capi.declared_symbols()
    for s in NEW:
        assert s in syms and s in capi._SIGNATURES and hasattr(capi.lib, s), s


def test_argument_checks_precede_device_use():
    """the checks that need no plan, on a NULL plan, in sm_sgm_wta's and sm_sgm_lr's order"""
    from stereomatching_amd import capi
    lib = capi.lib
    px = C.c_void_p(16)           # never dereferenced: every call below is refused first

    def refused(rc, text):
        assert rc == capi.SM_ERR_ARG
        assert text in lib.sm_last_error(), lib.sm_last_error()

    both = lambda **k: lib.sm_sgm_wta_both(None, k.get("l", px), px, k.get("c", 7), k.get("p1", 10), k.get("p2", 120),    # noqa: E731
                                           k.get("paths", 8), 1, k.get("web", px), None, None, k.get("wr", px), None, None)
    refused(both(), b"sm_sgm_wta_both: plan is NULL")
    refused(both(l=None, web=None), b"sm_sgm_wta_both: input image pointer is NULL")
    refused(both(web=None, wr=None), b"sm_sgm_wta_both: d_web is NULL")
    refused(both(wr=None, c=9), b"sm_sgm_wta_both: d_web_right is NULL")
    refused(both(c=9, paths=5), b"sm_sgm_wta_both: census_width 9 is not 3, 5 or 7")
    refused(both(paths=6, p1=-1), b"sm_sgm_wta_both: paths 6 is not 4 or 8")
    refused(both(p1=11, p2=10), b"sm_sgm_wta_both: penalties p1 11, p2 10 break 0 <= p1 <= p2 <= 32767")
    single = lambda **k: lib.sm_sgm_lr_single(None, k.get("l", px), px, k.get("c", 7), k.get("p1", 10), k.get("p2", 120),  # noqa: E731
                                              k.get("paths", 8), 1, k.get("md", 0), k.get("web", px), None, None, None,
                                              None, None)
    refused(single(), b"sm_sgm_lr_single: plan is NULL")
    refused(single(l=None, web=None), b"sm_sgm_lr_single: input image pointer is NULL")
    refused(single(web=None, md=-1), b"sm_sgm_lr_single: d_web is NULL")
    refused(single(md=-1, c=4), b"sm_sgm_lr_single: max_diff -1 is negative")
    refused(single(c=4, paths=3), b"sm_sgm_lr_single: census_width 4 is not 3, 5 or 7")
    refused(single(paths=3, p2=32768), b"sm_sgm_lr_single: paths 3 is not 4 or 8")
    refused(single(p2=32768), b"sm_sgm_lr_single: penalties p1 10, p2 32768 break")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("w,h,d,n", [(13, 5, 7, 1), (11, 4, 1, 3), (6, 5, 17, 3), (9, 3, 9, 1), (5, 4, 12, 1)])
def test_vectorised_right_map_against_the_loop(mode, w, h, d, n):
    """both borders, D = 1, D > W (the toroidal walk wraps more than once; ghost drops most candidates), n = 1 and 3"""
    left, right = pair(w, h, w + d, levels=5)
    s = sr.aggregate(sr.data_term(left, right, d, n, 5, mode), 3, 40, 8)
    best, web = ss.right_from_volume(s, mode)
    bb, bw = ss.right_from_volume_bruteforce(s, mode)
    assert np.array_equal(best, bb) and np.array_equal(web, bw)
    assert web.min() >= 1 and web.max() <= d
    if mode == "ghost":
        assert (web <= np.arange(w)[None, :] + 1).all()          # d <= u


def test_ties_in_a_random_volume_go_to_the_least_shift():
    s = np.random.default_rng(1).integers(0, 3, (4, 9, 6)).astype(np.int32)
    for mode in MODES:
        a, b = ss.right_from_volume(s, mode), ss.right_from_volume_bruteforce(s, mode)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("w,h,d,n,c", [(41, 13, 7, 1, 7), (33, 17, 12, 3, 5), (29, 11, 40, 5, 3), (20, 9, 1, 3, 7)])
def test_zero_penalties_give_the_census_right_reference(w, h, d, n, c):
    """toroidal, P1 = P2 = 0: S = paths * A, and the box window around left x at shift d holds the same pixel pairs as
    the window around right x + d, so the diagonal arg-min is the right-reference arg-min"""
    left, right = pair(w, h, w * d, levels=(256, 6)[c == 5])
    for paths in (4, 8):
        e = ss.both(left, right, d, n, c, 0, 0, paths, "toroidal")
        best_right, web_right = sr.right_reference(left, right, d, n, c, 0, 0, paths, "toroidal")
        assert np.array_equal(e[4], web_right) and np.array_equal(e[3], best_right)


@pytest.mark.parametrize("mode", MODES)
def test_a_constant_pair_gives_one_everywhere(mode):
    z = np.full((7, 19), 131, np.uint8)
    best, web, sub, best_right, web_right = ss.both(z, z, 9, 3, 5, 10, 120, 8, mode)
    assert (web == 1).all() and (web_right == 1).all() and (best == 0).all() and (best_right == 0).all()
    assert (sub == 16).all()


def test_a_periodic_pair_ties_and_the_least_shift_wins():
    left, right = periodic_pair()
    d = 20
    s = sr.aggregate(sr.data_term(left, right, d, 1, 7, "toroidal"), 10, 120, 8)
    assert np.array_equal(s[:, :, 0], s[:, :, 8]) and np.array_equal(s[:, :, 0], s[:, :, 16])     # exact ties
    best_right, web_right = ss.right_from_volume(s, "toroidal")
    assert (web_right == 1).all() and (best_right == 0).all()


@pytest.mark.parametrize("mode", MODES)
def test_left_maps_are_sgm_and_the_check_is_lr_check(mode):
    w, h, d, n, c = 23, 9, 10, 3, 7
    left, right = pair(w, h, 77, levels=8)
    e = ss.expected(left, right, d, n, c, 12, 90, 8, mode, max_diffs=(0, 1))
    best, web, sub = sr.sgm(left, right, d, n, c, 12, 90, 8, mode)
    assert np.array_equal(e["web"], web) and np.array_equal(e["best"], best) and np.array_equal(e["sub"], sub)
    for md in (0, 1):
        checked, rejected = sr.lr_check(web, e["web_right"], md, mode)
        assert np.array_equal(e[md]["checked"], checked) and e[md]["rejected"] == rejected
        assert ((e[md]["sub_checked"] == 0) == (checked == 0)).all()
    assert e[0]["rejected"] >= e[1]["rejected"] > 0


# ---------------------------------------------------------------------------
# what the named cases of the GPU test can tell (tests/sgm_single_patterns.py)
# ---------------------------------------------------------------------------

def test_every_mistake_has_a_case_and_every_case_is_the_definition():
    assert set(sp.MUTANT_CASE) == set(sp.MUTANTS) and set(sp.MUTANT_CASE.values()) <= set(sp.CASES)
    for name in sp.CASES:
        c, e = sp.inputs(name), sp.expected(name)
        want = ss.both(c["left"], c["right"], c["d"], c["sw"], c["census"], c["p1"], c["p2"], c["paths"], c["mode"])
        for k, v in zip(("best", "web", "sub", "best_right", "web_right"), want):
            assert np.array_equal(e[k], v), (name, k)


# the maps a mistake has to change on its case, and the ones it must leave alone
TELLS = {"last_wins": {"web_right"}, "ghost_wraps": {"best_right", "web_right"}, "toroidal_clips": {"best_right", "web_right"},
         "padding_joins": {"best", "web", "best_right", "web_right"}, "den_above_one": {"sub"}}


@pytest.mark.parametrize("mutant", sp.MUTANTS)
def test_the_named_case_tells_the_mistake_from_the_definition(mutant):
    name = sp.MUTANT_CASE[mutant]
    e, g = sp.expected(name), sp.mutant_maps(name, mutant)
    changed = {k for k in e if not np.array_equal(e[k], g[k])}
    assert changed == TELLS[mutant], (mutant, name, changed)


def test_what_the_named_cases_are_made_of():
    # the periodic pair ties three candidates of every right pixel; the padded case has one padded entry, in lane 63
    s = sp.volume("periodic toroidal")
    assert np.array_equal(s[:, :, 0], s[:, :, 8]) and np.array_equal(s[:, :, 0], s[:, :, 16])
    assert sp.inputs("padded 63")["d"] == 63
    for name in ("narrow toroidal", "narrow ghost"):
        assert sp.inputs(name)["d"] > 3 * sp.inputs(name)["left"].shape[1]
    # den = 1 comes as (S(d - 1), S(d + 1)) - best = (1, 0) only -- (0, 1) would make d - 1 the winner -- and gives q = 8
    e, s = sp.expected("den one"), sp.volume("den one").astype(np.int64)
    d = e["web"].astype(np.int64) - 1
    inner = (e["web"] > 1) & (e["web"] < s.shape[-1])
    lo = np.take_along_axis(s, np.clip(d - 1, 0, None)[..., None], -1)[..., 0] - e["best"]
    hi = np.take_along_axis(s, np.clip(d + 1, None, s.shape[-1] - 1)[..., None], -1)[..., 0] - e["best"]
    one = inner & (lo + hi == 1)
    assert one.sum() >= 2 and (lo[one] == 1).all() and (e["sub"][one] == 16 * e["web"][one] + 8).all()
