"""Left-right consistency check on the GPU at the shapes where the right-reference mode's own index arithmetic can go
wrong (sm_lr.hip): every width from 1 to 97 around the multiples of 32 (below 32 every word of
k_mirror_ext's output takes the bit-by-bit path and the toroidal halo wraps the row more than once), every kernel
family the plan can choose (bit-sliced with 4, 8 and 16 shifts per lane, popcount kernels A / B / C, the generic
kernel) and their 16-, 32- and 64-lane shift merges, and a seeded random sweep of sm_run_lr batches on plans with room
for more pairs than they are given, whose mirrored workspace is reused across calls.

Every expected value comes from the oracle (tests/oracle.py) and tests/lr_reference.py; none from the HIP path.  Each
test loops over its geometries, one plan each, and reports every map that differs, not just the first."""
import numpy as np
import pytest
import torch

from stereomatching_amd.synth import make_pair
from tests import lr_reference as lr
from tests import oracle
from tests.test_extremes_gpu import differences
from tests.test_hip_gpu import BUILT_BS, poisoned
from tests.test_lr_gpu import KERNEL_CHOICES, expected_lr

pytestmark = pytest.mark.gpu
MODES = ["toroidal", "ghost"]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def rand_edges(pairs, w, h, seed, density):
    rng = np.random.default_rng(seed)
    return ((rng.random((pairs, h, w)) < density).astype(np.uint8),
            (rng.random((pairs, h, w)) < density).astype(np.uint8))


def gray_pairs(pairs, w, h, d, seed):
    """pairs of different content: scenes whose right image is the left one moved (mostly consistent: both outcomes
    of the check occur) and white noise (nearly every pixel an edge)"""
    imgs = [make_pair(w, h, d, seed=seed + q, kind="noise" if q % 2 else "scene") for q in range(pairs)]
    return np.stack([a for a, _ in imgs]), np.stack([b for _, b in imgs])


def compare(tag, what, got, want):
    """differences() of one map kind over the pairs of a batch, labelled with the geometry"""
    return differences([f"{tag} pair {q}" for q in range(len(want))], got, np.stack(want), what)


def check_run_lr(plan, tag, left, right, d, sw, mode, max_diff, want_right=True, want_best=True, expect=None):
    """sm_run_lr on len(left) pairs against the definition -> list of differences.  expect: the expected_lr() dicts of
    these pairs, when already known"""
    pairs = len(left)
    want = expect or [expected_lr(left[q], right[q], d, sw, mode, max_diff) for q in range(pairs)]
    h, w = left.shape[-2:]
    res = plan.run_lr(dev(left), dev(right), 0.15, max_diff=max_diff, want_right=want_right, want_best=want_best,
                      web=poisoned(pairs, h, w), web_right=poisoned(pairs, h, w) if want_right else None,
                      best=poisoned(pairs, h, w) if want_best else None)
    bad = compare(f"{tag} run_lr", "web", host(res.web), [x["checked"] for x in want])
    got_rej, want_rej = host(res.rejected).tolist(), [x["rejected"] for x in want]
    if got_rej != want_rej:
        bad.append(f"{tag} run_lr rejected {got_rej} != {want_rej}")
    if want_right:
        bad += compare(f"{tag} run_lr", "web_right", host(res.web_right), [x["web_right"] for x in want])
    if want_best:
        bad += compare(f"{tag} run_lr", "best", host(res.best), [x["best"] for x in want])
    return bad, want


def check_right_reference(plan, tag, pairs, want_web, want_best):
    """sm_match_wta_right on the edges the plan holds -> list of differences"""
    h, w = want_web[0].shape
    web_right, best_right = plan.match_wta_right(pairs, web_right=poisoned(pairs, h, w),
                                                 best_right=poisoned(pairs, h, w))
    return (compare(f"{tag} match_wta_right", "web_right", host(web_right), want_web) +
            compare(f"{tag} match_wta_right", "best_right", host(best_right), want_best))


def check_geometry(hip, w, h, d, sw, mode, max_diff, options=None, pairs=2, seed=0):
    """One plan: sm_run_lr on gray pairs (edges by the edge kernels), sm_match_wta_right on the edges it left loaded,
    then sm_load_edges of other edge images (every packed word written) and sm_match_wta_right again, the workspace of
    the first call reused -> (plan description, list of differences)"""
    tag = f"{mode} W={w} H={h} D={d} S={sw} {options or ''}".rstrip()
    plan = hip.StereoPlan(w, h, d, sw, mode, max_pairs=pairs, options=options)
    desc = plan.describe()
    left, right = gray_pairs(pairs, w, h, d, seed)
    bad, want = check_run_lr(plan, tag, left, right, d, sw, mode, max_diff)
    bad += check_right_reference(plan, tag, pairs, [x["web_right"] for x in want], [x["best_right"] for x in want])
    el, er = rand_edges(pairs, w, h, seed + 1, 0.5 if seed % 2 else 0.2)
    plan.load_edges(dev(el), dev(er))
    ref = [lr.right_reference(el[q], er[q], d, sw, mode) for q in range(pairs)]
    bad += check_right_reference(plan, f"{tag} loaded", pairs, [r[1] for r in ref], [r[0] for r in ref])
    plan.close()
    return desc, [f"{b}   [{desc}]" for b in bad]


# ---------------------------------------------------------------------------
# 1. every width around the multiples of 32
# ---------------------------------------------------------------------------

WIDTHS = [1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 23, 29, 31, 32, 33, 36, 40, 47, 63, 64, 65, 95, 96, 97]
# (height, window): rows from one (below every tile height) to 26; windows of one pixel (S = 0 and 1), even ones
# (rounded up), and the whole image where the width allows (the window is clamped to min(W, H) below)
HEIGHT_WINDOWS = [(1, 0), (1, 1), (2, 2), (3, 3), (4, 1), (7, 5), (9, 9), (13, 7), (19, 19), (26, 25)]


def width_geometries(w):
    out = []
    for d in sorted({1, w - 1, w, w + 1, 3 * w}):
        if d < 1:
            continue
        for h, sw in HEIGHT_WINDOWS:
            out.append((h, d, min(sw, w, h)))
    return sorted(set(out))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("w", WIDTHS)
def test_right_reference_at_every_width(hip, w, mode):
    """web_right, best_right, the checked map and the rejected counts at D in {1, W - 1, W, W + 1, 3W}, on heights of
    1 to 26 rows with windows up to min(W, H); two pairs of different content per plan"""
    bad = []
    for i, (h, d, sw) in enumerate(width_geometries(w)):
        bad += check_geometry(hip, w, h, d, sw, mode, max_diff=(0, 1, 3)[i % 3], seed=w * 100 + i)[1]
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------
# 2. every kernel family in right-reference mode
# ---------------------------------------------------------------------------

def run_family(hip, mode, cases, must_say):
    """cases: (w, h, d, sw, options); every plan's description must contain must_say(case)"""
    bad = []
    for i, (w, h, d, sw, opts) in enumerate(cases):
        desc, b = check_geometry(hip, w, h, d, sw, mode, max_diff=(0, 1, 2, 10**6)[i % 4], options=opts,
                                 seed=7000 + i)
        for text in must_say(w, h, d, sw, opts):
            if text not in desc:
                b.append(f"W={w} H={h} D={d} S={sw} {opts}: plan is not the one named ('{text}' missing): {desc}")
        bad += b
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ds", [16, 8, 4])
def test_bit_sliced_kernels_in_right_reference_mode(hip, ds, mode):
    """k_match_bs with 4, 8 and 16 shifts per lane at every window it is built for, on widths below, at and above
    one word (the image as narrow as the window), D a part of one lane, a few lanes, up to 32 lanes"""
    cases = []
    for n, built in BUILT_BS:
        if built != ds:
            continue
        for j, w in enumerate((n, 31, 33, 70)):
            for d in (ds - 1, 3 * w if 3 * w <= 32 * ds else 32 * ds, 32 * ds - 3 * j):
                cases.append((w, n + j % 3, d, n, dict(shifts_per_lane=ds, tile_h=4 if j % 2 else 0)))
    run_family(hip, mode, cases, lambda w, h, d, sw, o: ("bit-sliced kernel", f"shift-lanes of {ds})"))


POPCOUNT = {"A": (0, 1, 3, 5, 8, 9), "B": (11, 13, 15), "C": (16, 17, 21, 25)}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("family", list(POPCOUNT))
def test_popcount_kernels_in_right_reference_mode(hip, family, mode):
    """kernel_family = 1: kernel A (windows up to 9), B (11 - 15), C (17 - 25; 16 rounds up to 17), on widths below,
    at and above one word, one shift to more than three times the width"""
    cases = []
    for sw in POPCOUNT[family]:
        for j, w in enumerate((max(sw, 1), 17, 31, 32, 33, 64, 97)):
            if w < sw:
                continue
            for d in (1, 16, 17, 3 * w):
                cases.append((w, max(sw, 1) + j % 4, d, sw, dict(kernel_family=1)))
    run_family(hip, mode, cases, lambda w, h, d, sw, o: (f"tiled kernel {family}",))


@pytest.mark.parametrize("mode", MODES)
def test_generic_kernel_in_right_reference_mode(hip, mode):
    """windows 27 and 31 (too large for the tiled kernels) and D = 1100, 1500 (past the popcount key's shift field)
    on small images: the generic kernel's own pad_l and row extents"""
    cases = []
    for sw in (27, 31):
        for w in (sw, 32, 33, 40, 64):
            for d in (1, 30, w, 3 * w):
                cases.append((w, sw + (w % 3), d, sw, None))
    for d in (1100, 1500):
        for w, h, sw in ((1, 3, 1), (5, 4, 3), (17, 9, 9), (31, 6, 5), (32, 5, 0), (33, 12, 11), (64, 7, 3),
                         (65, 26, 25), (97, 3, 3)):
            cases.append((w, h, d, sw, None))
    run_family(hip, mode, cases, lambda w, h, d, sw, o: ("generic kernel",))


MANY_SHIFTS = [129, 200, 256, 257, 300, 512, 600, 1000]
BS16 = {n for n, ds in BUILT_BS if ds == 16}
BS8 = {n for n, ds in BUILT_BS if ds == 8}


def shift_lanes(d, per_lane=16):
    nl = 1
    while nl * per_lane < d:
        nl *= 2
    return nl


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("opts", [None, dict(kernel_family=1)], ids=["default", "popcount"])
def test_many_shift_lanes_in_right_reference_mode(hip, opts, mode):
    """D from 129 to 1000: 16, 32 and 64 shift lanes merged per pixel run (popcount kernel A with 64 lanes at D = 600
    and 1000), on the plan's own kernel (bit-sliced up to D = 512) and the popcount kernels"""
    cases = [(w, h, d, sw, opts) for d in MANY_SHIFTS
             for w, h, sw in ((9, 5, 3), (31, 4, 1), (33, 9, 9), (96, 3, 3), (47, 13, 13), (64, 22, 21))]
    lanes = set()

    def must_say(w, h, d, sw, o):
        n = sw | 1
        # the plan's own choice: the bit-sliced kernel where its default build for the window (16 shifts per lane up
        # to 11 x 11, 8 up to 21 x 21) covers D in at most 32 lanes
        bs = 16 if n in BS16 else 8 if n in BS8 else 0
        if o is None and bs and shift_lanes(d, bs) <= 32:
            return ("bit-sliced kernel",)
        lanes.add((n <= 9, shift_lanes(d)))
        return (f"tiled kernel {'A' if n <= 9 else 'B' if n <= 16 else 'C'}", f"x {shift_lanes(d)} shift-lanes of 16)")
    run_family(hip, mode, cases, must_say)
    # every merge width on the popcount kernels, 64 lanes on kernel A among them (the default plans reach them too)
    assert {nl for _, nl in lanes} == {16, 32, 64} and (True, 64) in lanes, lanes


# ---------------------------------------------------------------------------
# 3. seeded random sweep of sm_run_lr
# ---------------------------------------------------------------------------

SWEEP_SHIFTS = [1, 2, 7, 16, 17, 30, 33, 64, 100, 128, 129, 200, 255, 257, 300, 512, 600, 1000, 1100]
ORACLE_BUDGET = 2.5e7       # W x H x D x (5 + n) of one oracle call: about 0.1 s


def _random_lr_cases(count, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        w = int(rng.integers(1, 331)); h = int(rng.integers(1, 201))
        if rng.random() < 0.2 and min(w, h) >= 27:
            sw = int(rng.integers(27, min(33, w, h) + 1))
        else:
            sw = int(rng.integers(0, min(26, w, h) + 1))
        d = int(rng.choice(SWEEP_SHIFTS))
        # the oracle's work bounds the image: rows go first, then columns (never below the window)
        while w * h * d * (5 + sw) > ORACLE_BUDGET and h > max(sw, 1):
            h = max(sw, 1, h // 2)
        while w * h * d * (5 + sw) > ORACLE_BUDGET and w > max(sw, 1):
            w = max(sw, 1, w // 2)
        mode = "ghost" if rng.integers(0, 2) else "toroidal"
        pairs = int(rng.integers(1, 4))
        max_pairs = pairs + int(rng.integers(1, 3))
        opts = KERNEL_CHOICES[int(rng.integers(0, len(KERNEL_CHOICES)))]
        max_diff = int(rng.choice([0, 1, 3, 10**6]))
        want_right, want_best = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        out.append((w, h, d, sw, mode, pairs, max_pairs, opts, max_diff, want_right, want_best))
    return out


@pytest.mark.parametrize("w,h,d,sw,mode,pairs,max_pairs,opts,max_diff,want_right,want_best",
                         _random_lr_cases(60, seed=1013))
def test_run_lr_random_geometries(hip, w, h, d, sw, mode, pairs, max_pairs, opts, max_diff, want_right, want_best):
    """a batch of 1 - 3 pairs of different content on a plan with room for more; then the same plan with fewer pairs
    (other content in the first slot), and after sm_load_edges of other edge images: the right-reference map, the
    left map and sm_lr_check on them -- the mirrored workspace of the first call reused throughout"""
    tag = f"{mode} W={w} H={h} D={d} S={sw} pairs={pairs}/{max_pairs} max_diff={max_diff}"
    seed = w * 1009 + h * 31 + d
    plan = hip.StereoPlan(w, h, d, sw, mode, max_pairs=max_pairs, options=opts)
    desc = plan.describe()
    left, right = gray_pairs(pairs, w, h, d, seed)
    bad, want = check_run_lr(plan, tag, left, right, d, sw, mode, max_diff, want_right, want_best)
    # fewer pairs, in reverse order: with more than one pair, slot 0 holds other content than in the first call
    fewer = max(1, pairs - 1)
    order = list(range(pairs))[::-1][:fewer]
    b2, _ = check_run_lr(plan, f"{tag} again with {fewer}", left[order], right[order], d, sw, mode, max_diff,
                         want_right=True, want_best=not want_best, expect=[want[q] for q in order])
    bad += b2
    # other edge images, as many pairs as the plan holds
    el, er = rand_edges(max_pairs, w, h, seed + 5, (0.05, 0.3, 0.5, 0.9)[seed % 4])
    plan.load_edges(dev(el), dev(er))
    ref = [lr.right_reference(el[q], er[q], d, sw, mode) for q in range(max_pairs)]
    bad += check_right_reference(plan, f"{tag} loaded", max_pairs, [r[1] for r in ref], [r[0] for r in ref])
    web, _ = plan.match_wta(max_pairs, want_best=False)
    web_right, _ = plan.match_wta_right(max_pairs, want_best=False)
    out, rejected = plan.lr_check(web, web_right, max_diff)
    left_maps = [oracle.hot_path(el[q], er[q], d, sw, mode)[1] for q in range(max_pairs)]
    checked = [lr.lr_check(left_maps[q], ref[q][1], max_diff, mode) for q in range(max_pairs)]
    bad += compare(f"{tag} loaded", "web", host(web), left_maps)
    bad += compare(f"{tag} loaded", "lr_check", host(out), [c[0] for c in checked])
    if host(rejected).tolist() != [c[1] for c in checked]:
        bad.append(f"{tag} loaded lr_check rejected {host(rejected).tolist()} != {[c[1] for c in checked]}")
    plan.close()
    assert not bad, "\n".join([desc, *bad])
