"""The rectification stage on the CPU: tests/rectify_reference.py (the definition the GPU is held to) against per-pixel
Python loops that share nothing with it, its identities, its meaning on a scene in front of the oracle's SAD matcher,
and the argument refusals of the C ABI that need no device."""
import ctypes as C
import math

import numpy as np
import pytest

from stereomatching_amd.synth import make_pair
from tests import rectify_patterns as rp
from tests import rectify_reference as rr

FMTS = ["abs32", "rel16"]
INTERPS = ["bilinear", "nearest"]


# ---------------------------------------------------------------------------
# the loops: Python integers, one pixel at a time
# ---------------------------------------------------------------------------

def loop_positions(m):
    h, w = len(m), len(m[0])
    rel = m.dtype == np.int16
    return [[(int(m[y][x][0]) + (32 * x if rel else 0), int(m[y][x][1]) + (32 * y if rel else 0)) for x in range(w)]
            for y in range(h)]


def loop_remap(src, m, interp, border):
    sh, sw = src.shape
    pos = loop_positions(m)
    h, w = len(pos), len(pos[0])
    out, valid = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)

    def tap(x, y):
        return (int(src[y][x]), True) if 0 <= x < sw and 0 <= y < sh else (border, False)
    for y in range(h):
        for x in range(w):
            mx, my = pos[y][x]
            if interp == "nearest":
                v, ok = tap((mx + 16) // 32, (my + 16) // 32)
                out[y][x], valid[y][x] = v, ok
                continue
            x0, y0 = mx // 32, my // 32                       # Python's // floors
            fx, fy = mx - 32 * x0, my - 32 * y0
            total, ok = 512, True
            for dx, dy, wgt in ((0, 0, (32 - fx) * (32 - fy)), (1, 0, fx * (32 - fy)), (0, 1, (32 - fx) * fy),
                                (1, 1, fx * fy)):
                v, inside = tap(x0 + dx, y0 + dy)
                total += wgt * v
                ok = ok and (inside or wgt == 0)
            out[y][x], valid[y][x] = total // 1024, ok
    return out, valid


def check_against_loop(src, m, tag):
    for interp in INTERPS:
        for border in (0, 255, 97):
            got, gv = rr.remap(src, m, interp, border)
            want, wv = loop_remap(src, m, interp, border)
            assert got.dtype == np.uint8 and gv.dtype == np.uint8
            assert np.array_equal(got, want), (tag, interp, border, np.argwhere(got != want)[:4].tolist())
            assert np.array_equal(gv, wv), (tag, interp, border, np.argwhere(gv != wv)[:4].tolist())


@pytest.mark.parametrize("fmt", FMTS)
def test_definition_against_per_pixel_loops(fmt):
    # (W, H) of the destination, (src_w, src_h): equal, larger, smaller, 1 x 1, one pixel wide
    shapes = [((9, 7), (9, 7)), ((5, 6), (11, 9)), ((12, 10), (4, 3)), ((1, 1), (1, 1)), ((1, 9), (1, 5)), ((7, 1), (6, 1)),
              ((6, 4), (1, 1)), ((1, 1), (8, 8))]
    for i, ((w, h), (sw, sh)) in enumerate(shapes):
        src = rp.image(sw, sh, i)
        check_against_loop(src, rp.random_map(w, h, sw, sh, 10 + i, fmt), ("random", w, h, sw, sh))
        check_against_loop(src, rp.outside_map(w, h, sw, sh, 0, fmt), ("left of the source", w, h))
        check_against_loop(src, rp.outside_map(w, h, sw, sh, 1, fmt), ("right of the source", w, h))
        # negative coordinates with every fraction: >> must floor (-1/32 is in the pixel -1, not 0)
        mx = np.arange(-70, -70 + w * h).reshape(h, w)
        check_against_loop(src, rp.as_format(mx, mx[::-1, ::-1] + 3, fmt), ("negative", w, h))
    if fmt == "abs32":
        src = rp.image(6, 5, 99)
        for which in (2, 3, 4):
            check_against_loop(src, rp.outside_map(7, 5, 6, 5, which), ("int32 extremes", which))


def test_maps_wholly_outside_give_the_border_and_no_validity():
    src = rp.image(8, 6, 1)
    for which in range(4):
        for interp in INTERPS:
            out, valid = rr.remap(src, rp.outside_map(5, 4, 8, 6, which), interp, 77)
            assert (out == 77).all() and not valid.any(), (which, interp)


# ---------------------------------------------------------------------------
# identities
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("interp", INTERPS)
def test_identity_map_returns_the_input_and_is_valid_everywhere(fmt, interp):
    for w, h in ((1, 1), (1, 6), (13, 8), (64, 3)):
        src = rp.image(w, h, w + h)
        out, valid = rr.remap(src, rr.identity_map(w, h, fmt), interp, 200)
        assert np.array_equal(out, src) and valid.all()


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("interp", INTERPS)
def test_integer_translation_shifts_the_image(fmt, interp):
    w, h = 17, 11
    src = rp.image(w, h, 4)
    for tx, ty in ((3, 0), (0, -2), (-4, 5), (20, 0)):
        out, valid = rr.remap(src, rp.translation_map(w, h, tx, ty, fmt), interp, 9)
        want, wv = np.full((h, w), 9, np.uint8), np.zeros((h, w), np.uint8)
        for y in range(h):
            for x in range(w):
                if 0 <= x + tx < w and 0 <= y + ty < h:
                    want[y, x], wv[y, x] = src[y + ty, x + tx], 1
        assert np.array_equal(out, want) and np.array_equal(valid, wv), (tx, ty)


def test_half_pixel_map_averages_horizontal_neighbours():
    w, h = 12, 5
    src = rp.image(w, h, 6)
    out, valid = rr.remap(src, rp.translation_map(w, h, 0, 0, fx=16, fy=0), "bilinear", 0)
    a, b = src[:, :-1].astype(int), src[:, 1:].astype(int)
    assert np.array_equal(out[:, :-1], (a + b + 1) >> 1)
    assert np.array_equal(out[:, -1], (src[:, -1].astype(int) + 0 + 1) >> 1)     # the border is the right neighbour there
    assert valid[:, :-1].all() and not valid[:, -1].any()                     # fy = 0: the row below does not count
    assert valid[-1, :-1].all()


def test_rel16_and_abs32_maps_of_the_same_positions_agree():
    w, h, sw, sh = 21, 13, 30, 9
    src = rp.image(sw, sh, 3)
    rel = rp.random_map(w, h, sw, sh, 5, "rel16")
    mx, my = rr.positions(rel)
    ab = rr.abs_map(mx, my)
    assert ab.dtype == np.int32 and rel.dtype == np.int16 and np.array_equal(rr.rel_map(*rr.positions(ab)), rel)
    for interp in INTERPS:
        a, b = rr.remap(src, rel, interp, 50), rr.remap(src, ab, interp, 50)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_valid_mask_zeroes_where_invalid():
    rng = np.random.default_rng(1)
    valid = (rng.random((6, 9)) < 0.6).astype(np.uint8)
    for dtype in (np.int32, np.int16):
        m = rng.integers(-50, 50, (6, 9)).astype(dtype)
        got = rr.valid_mask(m, valid)
        assert got.dtype == dtype
        for y in range(6):
            for x in range(9):
                assert got[y, x] == (m[y, x] if valid[y, x] else 0)


# ---------------------------------------------------------------------------
# the map of a calibration
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,cx,cy,f", [(3840, 2160, 1919.37, 1080.61, 3500.123), (1920, 1080, 957.3, 541.9, 1100.7),
                                         (37, 19, 17.77, 9.21, 31.3)])
def test_identity_calibration_builds_the_identity_map(w, h, cx, cy, f):
    c = rr.calibration(f, 1.003 * f, cx, cy)
    for fmt in FMTS:
        assert np.array_equal(rr.build_map(c, w, h, fmt), rr.identity_map(w, h, fmt)), fmt


def loop_build(c, x, y):
    """one pixel of build_positions in Python floats (IEEE doubles, one rounding per operation)"""
    R = [[float(v) for v in row] for row in np.asarray(c["R"])]
    xn, yn = (float(x) - c["new_cx"]) / c["new_fx"], (float(y) - c["new_cy"]) / c["new_fy"]
    X = (R[0][0] * xn + R[1][0] * yn) + R[2][0]
    Y = (R[0][1] * xn + R[1][1] * yn) + R[2][1]
    Z = (R[0][2] * xn + R[1][2] * yn) + R[2][2]
    if Z == 0.0:
        return rr.INT32_MIN, rr.INT32_MIN
    a, b = X / Z, Y / Z
    r2 = a * a + b * b
    rad = 1.0 + r2 * (c["k1"] + r2 * (c["k2"] + r2 * c["k3"]))
    ad = a * rad + (((2.0 * c["p1"]) * a) * b + c["p2"] * (r2 + (2.0 * a) * a))
    bd = b * rad + (c["p1"] * (r2 + (2.0 * b) * b) + ((2.0 * c["p2"]) * a) * b)
    u, v = c["fx"] * ad + c["cx"], c["fy"] * bd + c["cy"]
    if not (math.isfinite(u) and math.isfinite(v)):
        return rr.INT32_MIN, rr.INT32_MIN
    sat = lambda t: int(min(max(math.floor(t * 32.0 + 0.5), rr.INT32_MIN), rr.INT32_MAX))
    return sat(u), sat(v)


def test_map_builder_against_a_per_pixel_loop():
    w, h = 41, 23
    cases = dict(rp.calibrations(w, h), z_crossing=rp.z_crossing_calibration(w, h))
    for name, c in cases.items():
        mx, my = rr.build_positions(c, w, h)
        for y in range(h):
            for x in range(w):
                assert (int(mx[y, x]), int(my[y, x])) == loop_build(c, x, y), (name, x, y)
    mx, my = rr.build_positions(cases["z_crossing"], w, h)
    assert (mx[:, w // 2] == rr.INT32_MIN).all() and (my[:, w // 2] == rr.INT32_MIN).all()
    # distortion and rotation do move pixels, in the direction they should: barrel (k1 < 0) reads nearer the centre
    ident = rr.build_positions(cases["identity"], w, h)[0]
    barrel = rr.build_positions(cases["barrel"], w, h)[0]
    assert barrel[0, 0] > ident[0, 0] and barrel[0, -1] < ident[0, -1]


def test_rel16_is_refused_where_a_displacement_leaves_int16():
    w, h = 64, 8
    for c in (rp.far_calibration(w, h), rp.z_crossing_calibration(w, h)):
        assert rr.build_map(c, w, h, "abs32").dtype == np.int32
        with pytest.raises(ValueError, match="abs32"):
            rr.build_map(c, w, h, "rel16")
    with pytest.raises(ValueError, match="int16"):
        rr.rel_map(np.full((2, 2), 32768), np.zeros((2, 2), np.int64))
    assert rr.rel_map(np.array([[32767, -32768 + 32]]), np.zeros((1, 2), np.int64)).tolist() == [[[32767, 0], [-32768, 0]]]


def test_the_refusal_edges_are_what_they_say_and_tell_a_flag_that_looks_at_one_axis():
    """(the mutation audit's R7: the cases of test_map_build_where_z_crosses_zero_and_the_rel16_refusal overflow along x
    or along both axes, so a builder whose flag looks at dx alone passed them)"""
    w, h = rp.EDGE_W, rp.EDGE_H
    edges = rp.refusal_edges()
    assert len(edges) == 12
    for name, (c, fits) in edges.items():
        axis, d = name[1], int(name.split()[1])
        mx, my = rr.build_positions(c, w, h)
        dx, dy = mx - rr.ONE * np.arange(w)[None, :], my - rr.ONE * np.arange(h)[:, None]
        moved, still = (dx, dy) if axis == "x" else (dy, dx)
        assert (moved == d).all() and (still == 0).all(), name        # exactly d along one axis, 0 along the other
        assert rp.rel16_refused(mx, my) == (not fits), name
        if fits:
            assert rr.build_map(c, w, h, "rel16").dtype == np.int16
        else:
            with pytest.raises(ValueError, match="abs32"):
                rr.build_map(c, w, h, "rel16")
        # the flag that looks at the other axis alone lets this map through; the one that looks at this axis does not
        this, other = rp.OVERFLOW_MISTAKES[axis == "y"], rp.OVERFLOW_MISTAKES[axis == "x"]
        assert rp.rel16_refused(mx, my, this) == (not fits) and not rp.rel16_refused(mx, my, other), name
    # the cases the GPU module had before cannot tell "dx only": both are refused with it as without it
    for c in (rp.far_calibration(320, 48), rp.z_crossing_calibration(320, 48)):
        mx, my = rr.build_positions(c, 320, 48)
        assert rp.rel16_refused(mx, my) and rp.rel16_refused(mx, my, "overflow looks at dx only")


def test_smooth_calibration_fits_rel16_at_4k():
    """the claim behind the REL16 format: a 4K camera with k1 = -0.12 and a 0.02 rad rotation stays inside int16"""
    for side in (0, 1):
        m = rr.build_map(rp.smooth_calibration(3840, 2160, side), 3840, 2160, "rel16")
        assert np.abs(m.astype(np.int64)).max() > 1000                  # and it is no identity


# ---------------------------------------------------------------------------
# the stage in front of a matcher
# ---------------------------------------------------------------------------

def moved(img, dx, dy, border):
    """out(x + dx, y + dy) = img(x, y), `border` where nothing lands"""
    h, w = img.shape
    out = np.full((h, w), border, np.uint8)
    ys, xs = np.arange(h), np.arange(w)
    ys, xs = ys[(ys + dy >= 0) & (ys + dy < h)], xs[(xs + dx >= 0) & (xs + dx < w)]
    out[np.ix_(ys + dy, xs + dx)] = img[np.ix_(ys, xs)]
    return out


@pytest.mark.parametrize("mode", ["ghost", "toroidal"])
def test_rectified_scene_matches_like_the_original(mode):
    from tests import oracle
    w, h, d, sw = 96, 40, 16, 5
    half = sw // 2
    left, right = make_pair(w, h, d, seed=5)
    raw_left, raw_right = moved(left, 2, 3, 255), moved(right, -1, -2, 0)     # left down 3 / right 2, right up 2 / left 1
    ml, mr = rp.translation_map(w, h, 2, 3, "rel16"), rp.translation_map(w, h, -1, -2, "abs32")
    rl, vl = rr.remap(raw_left, ml, "bilinear", 13)
    rright, vr = rr.remap(raw_right, mr, "bilinear", 13)
    assert vl[:h - 3, :w - 2].all() and not vl[h - 3:].any() and not vl[:, w - 2:].any()
    assert vr[2:, 1:].all() and not vr[:2].any() and not vr[:, :1].any()
    assert np.array_equal(rl[vl == 1], left[vl == 1]) and np.array_equal(rright[vr == 1], right[vr == 1])
    assert (rl[vl == 0] == 13).all() and (rright[vr == 0] == 13).all()
    # pixels whose windows, over every shift, lie inside the valid region of both images
    both = (vl & vr).astype(bool)
    inside = np.zeros((h, w), bool)
    for y in range(half, h - half):
        for x in range(half, w - (d - 1) - half):
            inside[y, x] = both[y - half:y + half + 1, x - half:x + d + half].all()
    assert inside.sum() > 1000
    _, web = oracle.cost_hot_path(left, right, d, sw, mode, "sad")
    _, web_rect = oracle.cost_hot_path(rl, rright, d, sw, mode, "sad")
    _, web_raw = oracle.cost_hot_path(raw_left, raw_right, d, sw, mode, "sad")
    assert np.array_equal(web_rect[inside], web[inside])
    # a stage that did nothing would leave the raw pair, whose rows do not correspond
    assert (web_raw[inside] != web[inside]).mean() > 0.2


# ---------------------------------------------------------------------------
# the C ABI: refusals that precede any device use
# ---------------------------------------------------------------------------

def test_argument_refusals_precede_device_use():
    from stereomatching_amd import capi
    lib = capi.lib
    assert C.sizeof(capi.RectifyCalib) == 8 + 8 * 22
    buf = [(C.c_ubyte * 64)() for _ in range(8)]
    p = [C.c_void_p(C.addressof(b)) for b in buf]
    A, B, R = capi.SM_RMAP_ABS32, capi.SM_INTERP_BILINEAR, capi.SM_RMAP_REL16

    def refused(rc, text):
        assert rc == capi.SM_ERR_ARG and text in lib.sm_last_error(), lib.sm_last_error()
    refused(lib.sm_rectify(None, p[0], p[1], 4, 4, p[2], p[3], A, B, 0, 1, p[4], p[5], None, None, None),
            b"sm_rectify: plan is NULL")
    refused(lib.sm_rectify(None, p[0], p[1], 4, 4, p[2], p[3], 2, B, 0, 1, p[4], p[5], None, None, None),
            b"sm_rectify: map_format 2")
    refused(lib.sm_rectify(None, p[0], p[1], 4, 4, p[2], p[3], R, -1, 0, 1, p[4], p[5], None, None, None),
            b"sm_rectify: interp -1")
    refused(lib.sm_rectify(None, p[0], p[1], 4, 4, p[2], p[3], A, 2, 0, 1, p[4], p[5], None, None, None),
            b"sm_rectify: interp 2")
    refused(lib.sm_rectify(None, p[0], p[1], 4, 4, p[2], p[3], A, B, 256, 1, p[4], p[5], None, None, None),
            b"sm_rectify: border 256")
    refused(lib.sm_rectify(None, p[0], p[1], 4, 4, p[2], p[3], A, B, -1, 1, p[4], p[5], None, None, None),
            b"sm_rectify: border -1")
    refused(lib.sm_rectify(None, p[0], p[1], 0, 4, p[2], p[3], A, B, 0, 1, p[4], p[5], None, None, None),
            b"sm_rectify: source size 0x4")
    refused(lib.sm_rectify(None, None, p[1], 4, 4, p[2], p[3], A, B, 0, 1, p[4], p[5], None, None, None),
            b"sm_rectify: input image pointer is NULL")
    refused(lib.sm_rectify(None, p[0], p[1], 4, 4, p[2], None, A, B, 0, 1, p[4], p[5], None, None, None),
            b"sm_rectify: a map pointer is NULL")
    refused(lib.sm_rectify(None, p[0], p[1], 4, 4, p[2], p[3], A, B, 0, 1, p[4], None, None, None, None),
            b"sm_rectify: output image pointer is NULL")
    # overlapping pointers: an output that is an input, two outputs that are one
    refused(lib.sm_rectify(None, p[0], p[1], 4, 4, p[2], p[3], A, B, 0, 1, p[0], p[5], None, None, None),
            b"sm_rectify: an output overlaps an input")
    refused(lib.sm_rectify(None, p[0], p[1], 4, 4, p[2], p[3], A, B, 0, 1, p[4], p[5], p[6], p[3], None),
            b"sm_rectify: an output overlaps an input")
    refused(lib.sm_rectify(None, p[0], p[1], 4, 4, p[2], p[2], A, B, 0, 1, p[4], p[4], None, None, None),
            b"sm_rectify: outputs overlap")
    refused(lib.sm_rectify(None, p[0], p[1], 4, 4, p[2], p[3], A, B, 0, 1, p[4], p[5], p[6], p[6], None),
            b"sm_rectify: outputs overlap")
    calib = capi.RectifyCalib.make(100.0, 100.0, 32.0, 24.0)
    refused(lib.sm_rectify_map_build(None, C.byref(calib), A, p[0], None), b"sm_rectify_map_build: plan is NULL")
    refused(lib.sm_valid_mask(None, p[0], capi.SM_MAP_I32, p[1], 1, None), b"sm_valid_mask: plan is NULL")
    refused(lib.sm_valid_mask(None, p[0], 2, p[1], 1, None), b"sm_valid_mask: map_type 2")
    refused(lib.sm_valid_mask(None, None, capi.SM_MAP_I16, p[1], 1, None), b"sm_valid_mask: a map pointer is NULL")
    refused(lib.sm_valid_mask(None, p[0], capi.SM_MAP_I16, None, 1, None), b"sm_valid_mask: d_valid is NULL")
    refused(lib.sm_valid_mask(None, p[0], capi.SM_MAP_I16, p[0], 1, None), b"sm_valid_mask: d_valid overlaps the map")
    assert all(bytes(b) == bytes(64) for b in buf)


def test_calibration_struct_mirrors_the_header():
    """the ctypes mirror of sm_rectify_calib has the header's fields in the header's order, and the reference's"""
    import re
    from stereomatching_amd import capi
    text = re.sub(r"/\*.*?\*/", "", capi.HEADER.read_text(), flags=re.S)
    body = re.search(r"typedef struct sm_rectify_calib \{(.*?)\} sm_rectify_calib;", text, re.S).group(1)
    fields = []
    for decl in re.findall(r"(?:int|double)\s+([^;]+);", body):
        fields += [re.sub(r"\[.*", "", f.strip()) for f in decl.split(",")]
    assert fields == [n for n, _ in capi.RectifyCalib._fields_]
    assert tuple(fields[2:]) == rr.CALIB_FIELDS
    c = capi.RectifyCalib.make(**{k: v for k, v in rp.smooth_calibration(64, 48).items()})
    assert c.struct_size == C.sizeof(capi.RectifyCalib) and c.reserved == 0
    assert [[c.R[i][j] for j in range(3)] for i in range(3)] == rp.smooth_calibration(64, 48)["R"].tolist()
    for name, value in (("SM_RMAP_FRAC_BITS", rr.FRAC_BITS), ("SM_RMAP_ABS32", rr.ABS32), ("SM_RMAP_REL16", rr.REL16),
                        ("SM_INTERP_BILINEAR", rr.BILINEAR), ("SM_INTERP_NEAREST", rr.NEAREST)):
        assert re.search(rf"#define {name} {value}\b", text) and getattr(capi, name) == value
