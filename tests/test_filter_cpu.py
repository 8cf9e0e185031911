"""The definition of the post-filters (tests/filter_reference.py): its vectorised form against the naive one (a
per-pixel window sort; a breadth-first flood fill), and the identities the definition implies.  No GPU."""
import numpy as np
import pytest

from tests import filter_patterns as fp
from tests import filter_reference as fr

DTYPES = [np.int32, np.int16]
SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (2, 7), (7, 2), (13, 11), (40, 23)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [3, 5])
def test_median_forms_agree(dtype, k):
    for i, (w, h) in enumerate(SHAPES):
        for invalid, neg in ((0.0, False), (0.3, True), (0.8, False), (1.0, False)):
            a = fp.random_map(w, h, dtype, 100 * i + k, invalid, 1, (5, 3000)[i % 2], neg)
            assert np.array_equal(fr.median(a, k), fr.median_naive(a, k)), (w, h, invalid)
    info = np.iinfo(dtype)
    rng = np.random.default_rng(k)
    a = rng.choice(np.array([info.min, info.max, 0, -1, 1], dtype), (17, 19))
    assert np.array_equal(fr.median(a, k), fr.median_naive(a, k))
    for name, make in fp.PATTERNS.items():
        a = make(70, 37, dtype)[0]
        got = fr.median(a, k)
        assert np.array_equal(got, fr.median_naive(a, k)), name
        assert got.dtype == a.dtype and ((got == 0) == (a == 0)).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_median_identities(dtype):
    for k in (3, 5):
        c = np.full((9, 14), -37, dtype)
        assert np.array_equal(fr.median(c, k), c)                  # a constant valid map is itself
        z = np.zeros((6, 5), dtype)
        assert np.array_equal(fr.median(z, k), z)                  # all invalid
        one = z.copy()
        one[3, 2] = 11
        assert np.array_equal(fr.median(one, k), one)              # a lone valid pixel is its own median
    # the LOWER median of an even count: 1, 2, 3, 4 -> 2; and no wrapping at the borders
    a = np.zeros((3, 3), dtype)
    a[1, 1], a[0, 0], a[0, 1], a[2, 2] = 4, 1, 2, 3
    assert fr.median(a, 3)[1, 1] == 2
    b = np.zeros((4, 6), dtype)
    b[0, 0], b[0, 5], b[3, 0] = 5, 1, 1
    assert fr.median(b, 3)[0, 0] == 5 and fr.median(b, 5)[0, 0] == 5


@pytest.mark.parametrize("dtype", DTYPES)
def test_speckle_forms_agree(dtype):
    for i, (w, h) in enumerate(SHAPES):
        for invalid, neg, max_size, max_diff in ((0.0, False, 3, 0), (0.3, True, 4, 1), (0.6, False, 1, 2),
                                                 (1.0, False, 2, 0), (0.2, False, 0, 0)):
            a = fp.random_map(w, h, dtype, 7 * i + max_size, invalid, 1, 4, neg)
            got, want = fr.speckle(a, max_size, max_diff), fr.speckle_naive(a, max_size, max_diff)
            assert np.array_equal(got[0], want[0]) and got[1] == want[1], (w, h, invalid)
            assert got[0].dtype == a.dtype
    for name, make in fp.PATTERNS.items():
        a, max_size, max_diff = make(150, 70, dtype)
        fp.informative(a, max_size, max_diff)
        got, want = fr.speckle(a, max_size, max_diff), fr.speckle_naive(a, max_size, max_diff)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1], name
    info = np.iinfo(dtype)
    a = np.random.default_rng(1).choice(np.array([info.min, info.max, 0, -1, 1], dtype), (17, 19))
    for max_diff in (0, 2, 2**31 - 1):
        got, want = fr.speckle(a, 2, max_diff), fr.speckle_naive(a, 2, max_diff)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1], max_diff


@pytest.mark.parametrize("dtype", DTYPES)
def test_speckle_identities(dtype):
    a = fp.random_map(45, 31, dtype, 5, 0.35, 1, 5, negative=True)
    out, removed = fr.speckle(a, 0, 1)
    assert np.array_equal(out, a) and removed == 0                   # max_size 0 keeps everything
    for max_size in (a.size, a.size + 7):
        out, removed = fr.speckle(a, max_size, 1)
        assert not out.any() and removed == int((a != 0).sum())     # max_size >= W * H gives all 0
    # max_diff >= the value range: the components are those of the validity mask
    mask = (a != 0).astype(dtype)
    wide, _ = fr.speckle(a, 6, 10)
    of_mask, _ = fr.speckle(mask, 6, 0)
    assert np.array_equal(wide != 0, of_mask != 0)
    for max_size, max_diff in ((3, 0), (6, 1), (20, 2)):
        once, removed = fr.speckle(a, max_size, max_diff)
        assert removed == int((once != a).sum())                     # removed = the changed pixels
        twice, again = fr.speckle(once, max_size, max_diff)
        assert np.array_equal(twice, once) and again == 0            # idempotent
    c = np.full((8, 9), 3, dtype)                                    # all equal: one component of 72
    assert np.array_equal(fr.speckle(c, 71, 0)[0], c) and not fr.speckle(c, 72, 0)[0].any()
    z = np.zeros((4, 4), dtype)
    out, removed = fr.speckle(z, 3, 1)
    assert np.array_equal(out, z) and removed == 0                   # all invalid


def test_patterns_say_what_they_claim():
    a, max_size, _ = fp.exact_sizes(200, 120, np.int32)
    sizes = sorted(fr.components(a, 0)[1].values())
    assert sizes == [max_size] * 3 + [max_size + 1] * 3
    a, _, max_diff = fp.rings(150, 70, np.int32)
    assert len(fr.components(a, max_diff)[1]) > 3 and len(fr.components(a, max_diff + 1)[1]) == 1
    a, _, _ = fp.serpentine(150, 71, np.int32)
    sizes = fr.components(a, 1)[1]
    assert max(sizes.values()) == int((a == 7).sum())                # the path is one component
    a, _, _ = fp.spiral(150, 70, np.int32)
    sizes = fr.components(a, 0)[1]
    assert max(sizes.values()) == int((a == 5).sum())
    a, _, _ = fp.whole(150, 70, np.int32)
    assert max(fr.components(a, 0)[1].values()) == 150 * 70 - 5 * 9
