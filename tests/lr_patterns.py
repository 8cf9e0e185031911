"""Maps for the left-right check whose differences do not fit 32 bits (tests/test_lr_cpu.py, tests/test_lr_gpu.py).

sm_lr_check accepts every int32 in both maps, so web_right(u) - web(x) ranges over -(2^32 - 1) .. 2^32 - 1 and its
magnitude is compared as a 64-bit number.  A check that subtracts in 32 bits (the mutation audit's L2,
profiles/mutants/README.md) agrees with the definition unless the true difference is 2^32 - max_diff or more away
from 0 -- or, with a max_diff of 2^31 or so, lands on the far side of 2^31.  Checker only."""
import numpy as np

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
WIDE_H = 2
# (max_diff, mode): a small bound (toroidal only: in ghost mode a partner inside the row needs |s| <= W, so the
# difference stays within 2^31 + W of 0) and the largest bound there is
WIDE_CHECKS = ((2, "toroidal"), (INT_MAX, "toroidal"), (INT_MAX, "ghost"))


def wide_difference_maps(w):
    """-> (web, web_right) [WIDE_H][w], w >= 7.  Row 0 holds pairs of values about 2^32 apart (the true difference
    is +-(2^32 - 2) or +-(2^32 - 1): rejected at every max_diff, modulo 2^32 it is +-2 or +-1), row 1 small shifts
    whose partner inside the row is INT_MIN or INT_MAX (|difference| just above 2^31: rejected even at max_diff =
    INT_MAX, modulo 2^32 just below it), among ordinary consistent pixels."""
    assert w >= 7
    web = np.ones((WIDE_H, w), np.int64)                  # s = 1: u = x, consistent with a right map of 1s
    right = np.ones((WIDE_H, w), np.int64)

    def plant(y, x, s, r):
        web[y, x] = s
        right[y, (x + s - 1) % w] = r
    # partners u = (x + s - 1) mod w must be distinct columns: those of s = 1 pixels next to them stay consistent or not
    # by the definition, which both the oracle and the kernel apply
    plant(0, 0, INT_MIN + 1, INT_MAX)                     # diff = 2^32 - 2
    plant(0, 1, INT_MAX, INT_MIN)                         # diff = -(2^32 - 1)
    plant(0, 2, INT_MIN, INT_MAX)                         # diff = 2^32 - 1
    plant(1, 0, 3, INT_MIN)                               # u = 2: diff = -2^31 - 3
    plant(1, 3, -2, INT_MAX)                              # u = 0: diff = 2^31 + 1
    plant(1, 5, 2, INT_MIN)                               # u = 6: diff = -2^31 - 2
    return web.astype(np.int32), right.astype(np.int32)


MISTAKES = ("difference modulo 2^32",)


def lr_check_with(web, web_right, max_diff, mode, mistake):
    """lr.lr_check with the mistake made: the difference as a 32-bit number, its magnitude unsigned"""
    assert mistake in MISTAKES
    web = np.asarray(web, np.int64)
    web_right = np.asarray(web_right, np.int64)
    h, w = web.shape
    u = np.arange(w)[None, :] + web - 1
    valid = np.ones_like(u, bool) if mode == "toroidal" else (u >= 0) & (u < w)
    u = u % w if mode == "toroidal" else np.clip(u, 0, w - 1)
    du = (np.take_along_axis(web_right, u, axis=1) - web) % 2 ** 32
    mag = np.where(du >= 2 ** 31, 2 ** 32 - du, du)
    keep = valid & (mag <= max_diff)
    return np.where(keep, web, 0).astype(np.int32), int((~keep).sum())
