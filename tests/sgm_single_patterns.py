"""Named cases for SGM's left-right check from one aggregated volume (test_sgm_single_cpu.py, test_sgm_single_gpu.py),
each with the one mistake of the definition (tests/sgm_single_reference.py) that it is there to tell apart: MUTANT_CASE
names, for every mistake of MUTANTS, a case whose expected maps differ from the mistaken ones (pinned by
test_sgm_single_cpu.py), so that an exact pass of the GPU test on that case rules the mistake out in the kernel.

The mistakes are those a kernel of this shape can make: the tie rule of the diagonal arg-min, its candidate set at
either border, the padded entries of the volume (a lane holds 1, 2 or 4 shifts and the range is padded to 64, 128 or 256;
the path kernel leaves `paths` times 0x3fffffff there, wrapped to -4 or -8) and the subpixel fit's guard."""
from __future__ import annotations

import functools

import numpy as np

from tests import sgm_reference as sr
from tests import sgm_single_reference as ss

__all__ = ["CASES", "MUTANTS", "MUTANT_CASE", "inputs", "volume", "expected", "mutant_maps"]


def _noise(w, h, seed, levels):
    rng = np.random.default_rng(seed)
    return rng.integers(0, levels, (h, w)).astype(np.uint8), rng.integers(0, levels, (h, w)).astype(np.uint8)


def _periodic(w=64, h=6, period=8, seed=5):
    tile = np.random.default_rng(seed).integers(0, 256, (h, period)).astype(np.uint8)
    img = np.tile(tile, (1, w // period))
    return img, img.copy()


# name: (make(), D, window, census, P1, P2, paths, border)
_SPEC = {
    # L = R, periodic: S(x, d) = S(x, d + 8) exactly, every right pixel ties its candidates 0, 8, 16
    "periodic toroidal": (_periodic, 20, 1, 7, 10, 120, 8, "toroidal"),
    # more shifts than columns: the toroidal walk wraps more than once, the ghost one drops most candidates
    "narrow toroidal": (lambda: _noise(20, 5, 85, 9), 65, 3, 7, 12, 90, 8, "toroidal"),
    "narrow ghost": (lambda: _noise(20, 5, 85, 9), 65, 3, 7, 12, 90, 8, "ghost"),
    # one shift short of a full lane row: lane 63 holds the only padded entry
    "padded 63": (lambda: _noise(47, 5, 363, 256), 63, 3, 7, 12, 90, 8, "toroidal"),
    # few grey levels, a 1 x 1 window, small penalties: S differs by 1 between neighbouring shifts at many pixels
    "den one": (lambda: _noise(37, 6, 11, 3), 9, 1, 3, 1, 2, 4, "ghost"),
}
CASES = list(_SPEC)


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> dict(left, right [H][W] uint8, d, sw, census, p1, p2, paths, mode)"""
    make, d, sw, census, p1, p2, paths, mode = _SPEC[name]
    left, right = make()
    return dict(left=_frozen(left), right=_frozen(right), d=d, sw=sw, census=census, p1=p1, p2=p2, paths=paths, mode=mode)


@functools.lru_cache(maxsize=None)
def volume(name):
    c = inputs(name)
    return _frozen(sr.aggregate(sr.data_term(c["left"], c["right"], c["d"], c["sw"], c["census"], c["mode"]),
                                c["p1"], c["p2"], c["paths"]))


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> dict(best, web, sub, best_right, web_right): the definition's maps of the case, read-only"""
    s = volume(name)
    keys = ("best", "web", "sub", "best_right", "web_right")
    return {k: _frozen(v) for k, v in zip(keys, (*sr.winner(s), *ss.right_from_volume(s, inputs(name)["mode"])))}


MUTANTS = ("last_wins", "ghost_wraps", "toroidal_clips", "padding_joins", "den_above_one")
MUTANT_CASE = {"last_wins": "periodic toroidal", "ghost_wraps": "narrow ghost", "toroidal_clips": "narrow toroidal",
               "padding_joins": "padded 63", "den_above_one": "den one"}


def mutant_maps(name, kind):
    """-> dict like expected(name), with the mistake `kind` of MUTANTS made"""
    assert kind in MUTANTS
    c, s = inputs(name), volume(name)
    mode = c["mode"]
    h, w, D = s.shape
    best, web, sub = sr.winner(s)
    best_right, web_right = ss.right_from_volume(s, mode)
    if kind == "last_wins":
        # the greatest d reaching the minimum: the arg-min of the reversed candidates
        u = np.arange(w)
        cand = np.full((h, w, D), ss.NONE, np.int64)
        for d in range(D):
            if mode == "toroidal":
                cand[:, :, d] = s[:, (u - d) % w, d]
            elif d < w:
                cand[:, d:, d] = s[:, :w - d, d]
        k = D - 1 - np.argmin(cand[..., ::-1], axis=-1)
        web_right = (k + 1).astype(np.int32)
    elif kind == "ghost_wraps":
        best_right, web_right = ss.right_from_volume(s, "toroidal")
    elif kind == "toroidal_clips":
        best_right, web_right = ss.right_from_volume(s, "ghost")
    elif kind == "padding_joins":
        Dp = 64 if D <= 64 else 128 if D <= 128 else 256
        pad = np.full((h, w, Dp - D), -c["paths"], np.int32)
        sp = np.concatenate([s, pad], -1)
        best, web, _ = sr.winner(sp)
        best_right, web_right = ss.right_from_volume(sp, mode)
    elif kind == "den_above_one":
        d = web.astype(np.int64) - 1
        inner = (web > 1) & (web < D)
        a = np.take_along_axis(s, np.clip(d - 1, 0, D - 1)[..., None], -1)[..., 0].astype(np.int64) - best
        b = np.take_along_axis(s, np.clip(d + 1, 0, D - 1)[..., None], -1)[..., 0].astype(np.int64) - best
        sub = np.where(inner & (a + b == 1), 16 * web, sub).astype(np.int16)
    return dict(best=best, web=web, sub=sub, best_right=best_right, web_right=web_right)
