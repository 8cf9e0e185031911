"""Inputs for the interpolation tests (test_interp_cpu.py, test_interp_gpu.py): random maps with a chosen share of
invalid pixels, holes that cross every border of the sweeps' pieces, and a hand-built scene with a true occlusion
band.  Each structured pattern comes with informative(), which asserts from the definition alone that the input has
holes, that they are filled, and that the two rank rules disagree somewhere, so that neither an identity nor a
one-rule output can pass."""
import numpy as np

from tests import interp_reference as ir

SEG_H, CHUNK_W = 64, 64            # the kernels' pieces (sm_interp.hip: ITP_SEG rows of a line, ITP_CW pixels of a row)
# on and around one and two pieces, both ways (test_interp_gpu.py adds the post-filters' sizes)
SIZES = [(63, 63), (64, 64), (65, 65), (127, 129), (129, 127), (128, 128), (1, 130), (130, 1), (2, 65), (65, 2),
         (200, 70), (70, 200)]


def random_map(w, h, dtype, seed, invalid=0.3, lo=1, hi=6, negative=False):
    rng = np.random.default_rng(seed)
    a = rng.integers(lo, hi + 1, (h, w))
    if negative:
        a = np.where(rng.random((h, w)) < 0.4, -a, a)
    a[rng.random((h, w)) < invalid] = 0
    return a.astype(dtype)


def random_class(w, h, seed, ones=False):
    if ones:
        return np.ones((h, w), np.uint8)
    return np.random.default_rng(seed).integers(0, 3, (h, w)).astype(np.uint8)


def _texture(w, h, dtype, seed=0):
    """every pixel valid, values that differ between neighbours in every direction"""
    yy, xx = np.mgrid[0:h, 0:w]
    return (1 + (3 * xx + 7 * yy + (xx * yy) % 5 + seed) % 23).astype(dtype)


def band_v(w, h, dtype):
    """valid everywhere but a full-height band a quarter of the width wide"""
    a = _texture(w, h, dtype)
    a[:, w // 3:w // 3 + max(1, w // 4)] = 0
    return a


def band_h(w, h, dtype):
    a = _texture(w, h, dtype)
    a[h // 4:h // 4 + max(1, h // 3), :] = 0
    return a


def band_diag(w, h, dtype):
    """a diagonal band, a sixth of the width wide"""
    a = _texture(w, h, dtype)
    yy, xx = np.mgrid[0:h, 0:w]
    a[((xx - yy) % w) < max(1, w // 6)] = 0
    return a


def checkerboard(w, h, dtype):
    a = _texture(w, h, dtype)
    yy, xx = np.mgrid[0:h, 0:w]
    a[(xx + yy) % 2 == 1] = 0
    return a


def frame(w, h, dtype):
    """only the border pixels are valid"""
    a = _texture(w, h, dtype)
    a[1:-1, 1:-1] = 0
    return a


def anti_frame(w, h, dtype):
    """only the centre pixel is valid"""
    a = np.zeros((h, w), dtype)
    a[h // 2, w // 2] = 5
    return a


def lone(w, h, dtype):
    """a single valid pixel in one corner"""
    a = np.zeros((h, w), dtype)
    a[0, 0] = 7
    return a


PATTERNS = {"band_v": band_v, "band_h": band_h, "band_diag": band_diag, "checkerboard": checkerboard, "frame": frame,
            "anti_frame": anti_frame, "lone": lone}
# where the two rank rules agree everywhere: a single source, or holes that never see more than four candidates (no
# diagonal of a checkerboard hole ever meets a valid pixel; the rules agree for m = 1, 3, 4)
RULES_AGREE = {"anti_frame", "lone", "checkerboard"}


def informative(name, a):
    """assert on the definition: there are holes, holes are filled, holes span pieces of the sweeps where the map is
    large enough, and (but for RULES_AGREE) the occluded rule and the median rule differ somewhere"""
    h, w = a.shape
    holes = a == 0
    assert holes.any() and (~holes).any(), name
    med = ir.interpolate(a)
    assert ir.filled(a, med) > 0, name
    if name not in RULES_AGREE:
        occ = ir.interpolate(a, np.ones((h, w), np.uint8))
        assert (occ != med).any(), f"{name}: the two rank rules agree everywhere"
    if h > SEG_H:
        rows = np.flatnonzero(holes.any(axis=1))
        assert rows.min() // SEG_H != rows.max() // SEG_H, f"{name}: holes in one segment only"
    if w > CHUNK_W:
        cols = np.flatnonzero(holes.any(axis=0))
        assert cols.min() // CHUNK_W != cols.max() // CHUNK_W, f"{name}: holes in one chunk only"
    return med


def occlusion_scene(w=96, h=40, d=32, bg=3, fg=20, border="ghost"):
    """A hand-built checked map: background web = bg, a foreground rectangle web = fg, the right-reference map that is
    consistent with both, the occlusion band beside the rectangle set to 0, and a few isolated 0s inside both surfaces.
    -> dict(web, web_right, band (bool mask), isolated (list of (y, x)), rect (x0, x1, y0, y1)).

    Where the band lies: left pixel x with web = s is seen at right pixel u = x + s - 1.  The rectangle covers left
    columns x0 .. x1-1, so right columns x0 + fg - 1 .. x1 + fg - 2.  A background pixel x is hidden in the right
    view iff x + bg - 1 falls into that range and x is not itself foreground: x0 + fg - bg <= x < x1 + fg - bg, minus
    [x0, x1): for a rectangle wider than fg - bg that is x1 <= x < x1 + fg - bg, the band to the RIGHT of the
    rectangle, fg - bg pixels wide."""
    assert fg > bg >= 1 and fg <= d
    x0, x1, y0, y1 = w // 4, w // 4 + 30, h // 4, 3 * h // 4
    assert x1 - x0 > fg - bg and x1 + fg - 1 < w - 8, "the scene does not fit"
    web = np.full((h, w), bg, np.int32)
    web[y0:y1, x0:x1] = fg
    # the right view: right pixel u shows the nearest surface that projects onto it
    web_right = np.zeros((h, w), np.int32)
    for y in range(h):
        for x in range(w):                                   # background first, foreground over it
            u = x + web[y, x] - 1
            if web[y, x] == bg and u < w:
                web_right[y, u] = bg
        for x in range(w):
            u = x + web[y, x] - 1
            if web[y, x] == fg and u < w:
                web_right[y, u] = fg
    # derive the band from the two maps, not from the formula: a left pixel whose right pixel shows another surface
    band = np.zeros((h, w), bool)
    for y in range(h):
        for x in range(w):
            u = x + web[y, x] - 1
            if u < w and web_right[y, u] != web[y, x]:
                band[y, x] = True
    assert band[y0:y1, x1:x1 + fg - bg].all() and band.sum() == (y1 - y0) * (fg - bg), "the band is not where derived"
    web[band] = 0
    isolated = [(y0 + 3, x0 + 5), (y0 + 7, x0 + 17), (2, 10), (h - 3, w // 2), (y0 + 5, 4)]
    for y, x in isolated:
        assert web[y, x] != 0 and not band[max(0, y - 1):y + 2, max(0, x - 1):x + 2].any()
        web[y, x] = 0
    return dict(web=web, web_right=web_right, band=band, isolated=isolated, rect=(x0, x1, y0, y1), d=d, border=border,
                bg=bg, fg=fg)
