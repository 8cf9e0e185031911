"""Maps, images and calibrations shared by the CPU and GPU tests of the rectification stage (tests/rectify_reference.py
is the definition).  Everything is generated from a seed."""
import numpy as np

from tests import rectify_reference as rr

# the remap kernel gives a lane four consecutive pixels where W % 4 == 0 and one otherwise, 256 lanes a workgroup:
# widths of every residue mod 4, below 4, and on either side of 1024 = 4 * 256
SIZES = [(1, 1), (1, 7), (2, 3), (3, 5), (4, 4), (5, 2), (6, 9), (7, 1), (8, 33), (1023, 3), (1024, 2), (1025, 2),
         (1028, 5), (254, 17), (257, 9)]


def image(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def images(pairs, w, h, seed):
    return np.stack([image(w, h, seed + q) for q in range(pairs)])


def as_format(mx, my, fmt):
    return rr.abs_map(mx, my) if fmt == "abs32" else rr.rel_map(mx, my)


def random_map(w, h, src_w, src_h, seed, fmt="abs32", margin=3):
    """every pixel somewhere else: positions uniform over the source and `margin` pixels around it (REL16: as far as
    int16 reaches), every fraction"""
    rng = np.random.default_rng(seed)
    lo_x, hi_x = -margin * 32, (src_w + margin) * 32
    lo_y, hi_y = -margin * 32, (src_h + margin) * 32
    mx = rng.integers(lo_x, hi_x, (h, w))
    my = rng.integers(lo_y, hi_y, (h, w))
    if fmt == "rel16":
        x, y = 32 * np.arange(w)[None, :], 32 * np.arange(h)[:, None]
        mx, my = x + np.clip(mx - x, -32768, 32767), y + np.clip(my - y, -32768, 32767)
    return as_format(mx, my, fmt)


def permutation_map(w, h, seed, fmt="abs32"):
    """destination pixel i reads source pixel perm(i) of an image of the same size, with a fraction: the locality worst
    case (abs32 only beyond +-1023 pixels)"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(w * h).reshape(h, w)
    mx = 32 * (perm % w) + rng.integers(0, 32, (h, w))
    my = 32 * (perm // w) + rng.integers(0, 32, (h, w))
    return as_format(mx, my, fmt)


def translation_map(w, h, tx, ty, fmt="abs32", fx=0, fy=0):
    """destination (x, y) reads source (x + tx + fx/32, y + ty + fy/32)"""
    mx = np.broadcast_to(32 * (np.arange(w)[None, :] + tx) + fx, (h, w))
    my = np.broadcast_to(32 * (np.arange(h)[:, None] + ty) + fy, (h, w))
    return as_format(mx, my, fmt)


def outside_map(w, h, src_w, src_h, which, fmt="abs32"):
    """every entry outside the source: 0 left / above by two pixels, 1 right / below, 2 (abs32) INT32_MIN, 3 INT32_MAX,
    4 a mixture of both extremes and positions just inside and outside each edge"""
    if which == 0:
        mx, my = np.full((h, w), -64), np.full((h, w), -64)
    elif which == 1:
        mx, my = np.full((h, w), 32 * src_w + 40), np.full((h, w), 32 * src_h + 40)
    elif which == 2:
        mx, my = np.full((h, w), rr.INT32_MIN), np.full((h, w), rr.INT32_MIN)
    elif which == 3:
        mx, my = np.full((h, w), rr.INT32_MAX), np.full((h, w), rr.INT32_MAX)
    else:
        rng = np.random.default_rng(w * 131 + h)
        choices_x = np.array([rr.INT32_MIN, rr.INT32_MAX, -33, -32, -31, -17, -16, -1, 0, 1, 32 * src_w - 48,
                              32 * src_w - 33, 32 * src_w - 32, 32 * src_w - 17, 32 * src_w - 16, 32 * src_w - 1,
                              32 * src_w, rr.INT32_MAX - 15, rr.INT32_MAX - 16, rr.INT32_MIN + 31])
        choices_y = np.where(np.abs(choices_x) > 2**30, choices_x, choices_x - 32 * src_w + 32 * src_h)
        mx, my = rng.choice(choices_x, (h, w)), rng.choice(choices_y, (h, w))
    return as_format(mx, my, fmt)


def rotation(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    if axis == 0:
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    if axis == 1:
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def smooth_calibration(w, h, side=0):
    """a real-looking camera: focal length about the image width, barrel distortion k1 = -0.12, a little tangential
    distortion and a rectifying rotation of 0.02 rad (the other way for the right camera)"""
    sign = -1.0 if side else 1.0
    R = rotation(2, sign * 0.02) @ rotation(1, sign * 0.01) @ rotation(0, -sign * 0.005)
    return rr.calibration(0.9 * w, 0.9 * w, 0.5 * w - 3.25 * sign, 0.5 * h + 1.5, k1=-0.12, k2=0.03, p1=4e-4 * sign,
                          p2=-3e-4, k3=-0.004, R=R, new_fx=0.88 * w, new_fy=0.88 * w, new_cx=0.5 * w, new_cy=0.5 * h)


def calibrations(w, h):
    """name -> calibration: what sm_rectify_map_build is compared on"""
    f, cx, cy = 0.8 * w, 0.5 * w - 0.3, 0.5 * h + 0.7
    base = dict(fx=f, fy=1.01 * f, cx=cx, cy=cy)
    return {
        "identity": rr.calibration(**base),
        "barrel": rr.calibration(**base, k1=-0.35, k2=0.12, k3=-0.02),
        "pincushion": rr.calibration(**base, k1=0.4, k2=0.25, k3=0.08),
        "tangential": rr.calibration(**base, p1=0.01, p2=-0.007),
        "rotate_x": rr.calibration(**base, R=rotation(0, 0.03)),
        "rotate_y": rr.calibration(**base, R=rotation(1, -0.04)),
        "rotate_z": rr.calibration(**base, R=rotation(2, 0.05)),
        "new_projection": rr.calibration(**base, k1=-0.1, new_fx=0.6 * f, new_fy=0.7 * f, new_cx=cx + 5.5,
                                         new_cy=cy - 2.25),
        "smooth_left": smooth_calibration(w, h, 0),
        "smooth_right": smooth_calibration(w, h, 1),
    }


def z_crossing_calibration(w, h):
    """a rotation of 90 degrees about y and a principal point on a pixel: Z = 0 exactly on the column x = new_cx, small
    and of either sign beside it"""
    R = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])
    return rr.calibration(0.8 * w, 0.8 * w, w // 2, h // 2, k1=-0.05, R=R, new_cx=float(w // 2), new_cy=float(h // 2))


def far_calibration(w, h):
    """finite everywhere, but a new projection that moves pixels by more than 1023: REL16 must be refused"""
    return rr.calibration(float(w), float(w), 0.5 * w, 0.5 * h, new_cx=0.5 * w - 1100.0)


# ---------------------------------------------------------------------------
# the REL16 refusal, one axis at a time (the mutation audit, profiles/mutants/README.md: R7)
# ---------------------------------------------------------------------------
EDGE_W, EDGE_H = 8, 3               # focal length 8: every quotient and product below is exact in binary


def shift_calibration(w, h, sx, sy):
    """an undistorted, unrotated camera whose new projection moves every pixel by exactly (sx, sy) source pixels
    (multiples of 1/32 at a focal length that is a power of two): the displacement is (32 sx, 32 sy) everywhere"""
    return rr.calibration(float(w), float(w), 0.5 * w, 0.5 * h, new_cx=0.5 * w - sx, new_cy=0.5 * h - sy)


def refusal_edges(w=EDGE_W, h=EDGE_H):
    """name -> (calibration, fits REL16): a displacement on either side of each end of int16, along ONE axis with the
    other at 0, and one of 1100 pixels either way along y (far_calibration, which moves along x, turned by a quarter)"""
    out = {}
    for axis in "xy":
        for d, fits in ((32767, True), (32768, False), (-32768, True), (-32769, False), (35200, False), (-35200, False)):
            s = d / 32.0
            out[f"d{axis} {d}"] = (shift_calibration(w, h, s if axis == "x" else 0.0, s if axis == "y" else 0.0), fits)
    return out


OVERFLOW_MISTAKES = ["overflow looks at dx only", "overflow looks at dy only"]


def rel16_refused(mx, my, mistake=None):
    """does rr.rel_map refuse these positions?  With `mistake` (one of OVERFLOW_MISTAKES): would a builder that makes
    it refuse them"""
    assert mistake is None or mistake in OVERFLOW_MISTAKES
    mx, my = np.asarray(mx, np.int64), np.asarray(my, np.int64)
    h, w = mx.shape
    dx = mx - rr.ONE * np.arange(w, dtype=np.int64)[None, :]
    dy = my - rr.ONE * np.arange(h, dtype=np.int64)[:, None]
    seen = {None: (dx, dy), "overflow looks at dx only": (dx,), "overflow looks at dy only": (dy,)}[mistake]
    return any(d.min() < -32768 or d.max() > 32767 for d in seen)
