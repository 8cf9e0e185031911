"""Host-side mirror of the reference's pipeline interface over the C ABI.

The reference has no library API: `algorithm(first, second, width, height,
AlgorithmParams)` (/root/reference/src/stereo.cu:289-347) calls its stage
kernels in order.  `StereoPlan` exposes the same stages under the same names
and argument meaning, each one a thin call into libstereo_hip.so.  torch is
plumbing only: it owns the device buffers and the stream the launches go to.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import capi
from .capi import BORDERS, check, lib

# defaults of /root/reference/src/stereo.c:6-10
NUM_SHIFTS = 30
DEFAULT_THRESHOLD = 0.15
DEFAULT_SQUARE_WIDTH = 21
DEFAULT_TIMES = 32
DEFAULT_LINES = 10


@dataclass
class AlgorithmParams:
    """src/stereo.c:280-285"""
    threshold: float = DEFAULT_THRESHOLD
    square_width: int = DEFAULT_SQUARE_WIDTH
    times: int = DEFAULT_TIMES
    lines_to_draw: int = DEFAULT_LINES


class LRResult(NamedTuple):
    """StereoPlan.run_lr / cost_lr: the checked map (0 = rejected), rejected pixels per pair, and the optional maps"""
    web: torch.Tensor
    rejected: torch.Tensor
    web_right: Optional[torch.Tensor]
    best: Optional[torch.Tensor]


class SGMLRResult(NamedTuple):
    """StereoPlan.sgm_lr: LRResult's maps and the left pass's subpixel map (0 where rejected)"""
    web: torch.Tensor
    rejected: torch.Tensor
    web_right: Optional[torch.Tensor]
    best: Optional[torch.Tensor]
    sub: Optional[torch.Tensor]


WEB_TYPES = {torch.int32: capi.SM_WEB_I32, torch.uint16: capi.SM_WEB_U16, torch.uint8: capi.SM_WEB_U8}
MAP_TYPES = {torch.int32: capi.SM_MAP_I32, torch.int16: capi.SM_MAP_I16}
REDUCE_FILTERS = {"box": capi.SM_REDUCE_BOX, "binomial": capi.SM_REDUCE_BINOMIAL}


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def reprojection_matrix(first_calib, second_calib, baseline):
    """The 4 x 4 matrix Q of a rectified rig (sm_reproject_q; host only) -> 16 floats, row-major: [X Y Z Wh]' =
    Q [x y d 1]' with Z = f t / (d - (c2x - c1x)) in the baseline's unit.  *_calib: a capi.RectifyCalib or a dict of
    RectifyCalib.make's arguments (the rectified projection new_fx, new_fy, new_cx, new_cy is what counts)."""
    calibs = [c if isinstance(c, capi.RectifyCalib) else capi.RectifyCalib.make(**c) for c in (first_calib, second_calib)]
    q = capi.Q16()
    check(lib.sm_reproject_q(C.byref(calibs[0]), C.byref(calibs[1]), float(baseline), q))
    return list(q)


def guide_weights(sigma, peak=1024):
    """A weight table for StereoPlan.weighted_median -> 256 uint16: max(1, round(peak * exp(-delta / sigma))) for a
    gray difference delta = 0 .. 255 (numpy's exp and round-half-even; no C counterpart: the table is the interface)"""
    return np.maximum(1, np.rint(peak * np.exp(-np.arange(256) / sigma))).astype(np.uint16)


class StereoPlan:
    """Geometry + device workspace for one image size / shift count / window."""

    def __init__(self, width: int, height: int, num_shifts: int = NUM_SHIFTS,
                 square_width: int = DEFAULT_SQUARE_WIDTH, border: str | int = "toroidal",
                 max_pairs: int = 1, device: int = 0, options: dict | None = None):
        """options: fields of sm_plan_options (kernel variant / tiling chosen explicitly:
        tuning, A/B measurements, tests); None = the plan's own choices"""
        self.width, self.height = int(width), int(height)
        self.num_shifts, self.square_width = int(num_shifts), int(square_width)
        self.border = BORDERS[border] if isinstance(border, str) else int(border)
        self.max_pairs, self.device = int(max_pairs), int(device)
        self._h = C.c_void_p(0)
        opts = capi.PlanOptions.make(**options) if options else None
        check(lib.sm_plan_create_ex(self.device, self.width, self.height, self.num_shifts,
                                    self.square_width, self.border, self.max_pairs,
                                    C.byref(opts) if opts is not None else None, C.byref(self._h)))
        self._dev = torch.device("cuda", self.device)
        self._pipelined = 0
        self._side = None           # where result maps of calls that take the lanes are allocated (_lane_out)

    def close(self):
        if self._h:
            lib.sm_plan_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- helpers -----------------------------------------------------------
    def describe(self) -> str:
        return lib.sm_plan_describe(self._h).decode()

    def geometry(self) -> dict:
        """The kernel variant and tiling the plan selected (sm_plan_geometry)."""
        g = capi.Geometry()
        check(lib.sm_plan_geometry_sized(self._h, C.byref(g), C.sizeof(g)))
        return {n: getattr(g, n) for n, _ in capi.Geometry._fields_}

    def valu_model(self, pairs: int = 1, want_best: bool = False):
        """VALU wave-instructions of one match launch from the analytic model of
        valu_model.py; None where no coefficients exist for this kernel variant."""
        from . import valu_model
        return valu_model.match_launch(self.geometry(), self.width, self.height, self.num_shifts,
                                       self.border, pairs, want_best)

    def workspace_bytes(self) -> int:
        return int(lib.sm_plan_workspace_bytes(self._h))

    def set_pipelined(self, enabled: bool = True):
        """Let consecutive run() calls overlap (two internal lanes: edges of call i+1 beside
        the match of call i, the head of match i+1 in the tail of match i; give consecutive
        calls their own result maps).  With True the inputs given to run() must be complete in
        memory at call time; with 2 they may still be in flight on the current stream.  Inside
        a stream capture, run() on a pipelined plan needs web= (and best=) maps of your own."""
        check(lib.sm_plan_set_pipelined(self._h, int(enabled)))
        self._pipelined = 2 if enabled == 2 else int(bool(enabled))

    def prepare_threshold(self, threshold: float = DEFAULT_THRESHOLD):
        """Threshold-only set-up of find_all_edges (it does this itself on first use)."""
        check(lib.sm_plan_prepare_threshold(self._h, float(threshold), self._stream()))

    def reserve_narrow(self):
        """The int32 staging map that uint8 / uint16 results of the fallback kernels go through, allocated now
        (a no-op for plans whose kernel stores narrow maps itself): keeps the allocation out of timed paths and
        out of stream captures."""
        check(lib.sm_plan_reserve_narrow(self._h))
        self._narrow_ready = True

    def reserve_lr(self):
        """The workspace of the left-right consistency check (mirrored packed images, one mirrored-order map per
        pair), allocated now: keeps the allocation out of timed paths and out of stream captures."""
        check(lib.sm_plan_reserve_lr(self._h))

    def reserve_cost_lr(self):
        """The workspace of the cost mode's consistency check (mirrored gray images, and the mirrored-order map if
        reserve_lr has not allocated it), allocated now: keeps the allocation out of timed paths and out of stream
        captures."""
        check(lib.sm_plan_reserve_cost_lr(self._h))

    def time_kernels(self, capacity: int, every: int = 1):
        """Bracket every `every`-th of the coming match launches (at most `capacity` of
        them) with HIP events on the launch stream."""
        check(lib.sm_plan_time_stride(self._h, int(every)))
        check(lib.sm_plan_time_kernels(self._h, int(capacity)))

    def kernel_ms(self):
        """(mean ms, launches) of the match launches recorded since time_kernels()."""
        ms, n = C.c_double(0), C.c_int(0)
        check(lib.sm_plan_kernel_ms(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self._dev).cuda_stream)

    def _images(self, t: torch.Tensor, dtype, name: str):
        if t.device != self._dev or t.dtype != dtype or not t.is_contiguous():
            raise ValueError(f"{name}: need a contiguous {dtype} tensor on {self._dev}, "
                             f"got {t.dtype} on {t.device}")
        if t.dim() == 2:
            t = t.unsqueeze(0)
        if t.dim() != 3 or t.shape[1] != self.height or t.shape[2] != self.width:
            raise ValueError(f"{name}: shape {tuple(t.shape)} is not (pairs, {self.height}, {self.width})")
        return t

    def _out(self, t, pairs, name, dtype=torch.int32):
        """A caller-supplied result buffer gets the same checks as an input (a wrong
        buffer would otherwise become an out-of-bounds device write)."""
        if t is None:
            return self._new(pairs, dtype)
        t = self._images(t, dtype, name)
        if t.shape[0] < pairs:
            raise ValueError(f"{name}: room for {t.shape[0]} maps, {pairs} pairs requested")
        return t

    def _new(self, pairs, dtype):
        return torch.empty((pairs, self.height, self.width), dtype=dtype, device=self._dev)

    def _lane_out(self, t, pairs, name, dtype=torch.int32):
        """_out() for a call that may run on the plan's lanes (run_after, run on a pipelined plan).  Such a call is
        not ordered behind work already queued on the current stream, so a map from that stream's pool could be a
        block freed while a consumer of an earlier map is still pending there, and the lane would overwrite it
        first.  Maps of our own come from a private stream's pool instead, marked used by the current stream: the
        allocator hands the block out again only once the current stream's work at the time of the free is done.
        (Inside a capture there are none: _refuse_unowned_maps.)"""
        if t is not None:
            return self._out(t, pairs, name, dtype)
        if self._side is None:
            self._side = torch.cuda.Stream(self._dev)
        user = torch.cuda.current_stream(self._dev)
        with torch.cuda.stream(self._side):
            t = self._new(pairs, dtype)
        t.record_stream(user)
        return t

    def _refuse_unowned_maps(self, name, launch):
        """A call that takes the lanes inside a stream capture, without a map of the caller's for `name`: the lanes
        fork from the capturing stream where the PREVIOUS call ended, so nothing captured between two calls orders the
        second one, and a block freed in the capture could be handed to it while a consumer of the block is pending.
        `launch` makes the call with a NULL web map, which the library refuses before anything is captured -- after
        what cannot be captured at all (its message names the remedy, and is the one raised).  Always raises."""
        rc = launch()
        if rc != capi.SM_OK and "d_web is NULL" not in lib.sm_last_error().decode(errors="replace"):
            check(rc)
        raise ValueError(f"{name}=None inside a stream capture: a call that takes the plan's lanes cannot be ordered "
                         f"behind the consumers of a map allocated there -- pass {name}= a map of your own")

    # ---- step 1 ------------------------------------------------------------
    def find_all_edges(self, left, right, threshold=DEFAULT_THRESHOLD, want_edges=True):
        """find_all_edges x2 (src/stereo.cu:27-92,:312-313).  uint8 gray in; fills the
        plan's packed edge workspace; returns the u8 {0,1} edge images if wanted."""
        left = self._images(left, torch.uint8, "left")
        right = self._images(right, torch.uint8, "right")
        pairs = left.shape[0]
        el = self._new(pairs, torch.uint8) if want_edges else None
        er = self._new(pairs, torch.uint8) if want_edges else None
        check(lib.sm_find_edges(self._h, _ptr(left), _ptr(right), float(threshold), pairs,
                                _ptr(el), _ptr(er), self._stream()))
        return (el, er) if want_edges else None

    def load_edges(self, left_edges, right_edges):
        """Start from u8 {0,1} edge images (the arguments of fillup_matches)."""
        le = self._images(left_edges, torch.uint8, "left_edges")
        re = self._images(right_edges, torch.uint8, "right_edges")
        check(lib.sm_load_edges(self._h, _ptr(le), _ptr(re), le.shape[0], self._stream()))
        return le.shape[0]

    # ---- step 2: the hot path ----------------------------------------------
    def match_wta(self, pairs=1, want_best=True, web=None, best=None, web_dtype=torch.int32):
        """fillup_matches + fillup_scores + find_highest_scoring_shifts
        (src/stereo.cu:127-225) in one launch -> (web, best).  web_dtype torch.uint16 /
        torch.uint8 asks for the narrow map (sm_match_wta_typed); int32 is the reference's."""
        web = self._out(web, pairs, "web", web_dtype)
        best = self._out(best, pairs, "best") if want_best else None
        check(lib.sm_match_wta_typed(self._h, pairs, _ptr(web), WEB_TYPES[web_dtype],
                                     _ptr(best if want_best else None), self._stream()))
        return web, (best if want_best else None)

    def run(self, left, right, threshold=DEFAULT_THRESHOLD, want_best=False, web=None, best=None,
            web_dtype=torch.int32):
        """steps 1+2: uint8 pairs in, web (and optionally best) out."""
        left = self._images(left, torch.uint8, "left")
        right = self._images(right, torch.uint8, "right")
        pairs = left.shape[0]
        if self._pipelined and (web is None or (want_best and best is None)) and \
                torch.cuda.is_current_stream_capturing():
            self._refuse_unowned_maps("web" if web is None else "best", lambda: lib.sm_run_typed(
                self._h, _ptr(left), _ptr(right), float(threshold), pairs, _ptr(None), WEB_TYPES[web_dtype], _ptr(None),
                self._stream()))
        out = self._lane_out if self._pipelined else self._out
        web = out(web, pairs, "web", web_dtype)
        best = out(best, pairs, "best") if want_best else None
        if web_dtype != torch.int32 and not getattr(self, "_narrow_ready", False) and \
                not torch.cuda.is_current_stream_capturing():
            self.reserve_narrow()       # (inside a capture the library says what to call first)
        check(lib.sm_run_typed(self._h, _ptr(left), _ptr(right), float(threshold), pairs, _ptr(web),
                               WEB_TYPES[web_dtype], _ptr(best if want_best else None), self._stream()))
        return web, (best if want_best else None)

    def run_after(self, left, right, threshold=DEFAULT_THRESHOLD, inputs_ready=None, want_best=False, web=None,
                  best=None, web_dtype=torch.int32):
        """run() whose only input dependency is `inputs_ready`: consecutive calls may overlap, and on launches that
        cannot fill the chip twice over the plan lets them (sm_run_after).

        inputs_ready is a torch.cuda.Event recorded behind whatever produces `left` and `right`, or None: the images
        are complete in memory NOW.  None does not mean "queued on the current stream": the call is not ordered
        behind that stream's earlier work (that order would also put it behind the previous call, and take away
        the overlap this call exists for).  Inputs still in flight need an event here, or a plan run with
        set_pipelined(2) instead.  Inside a stream capture pass web= (and best=) maps of your own."""
        left = self._images(left, torch.uint8, "left")
        right = self._images(right, torch.uint8, "right")
        pairs = left.shape[0]
        ev = C.c_void_p(inputs_ready.cuda_event) if inputs_ready is not None else C.c_void_p(0)
        if (web is None or (want_best and best is None)) and torch.cuda.is_current_stream_capturing():
            self._refuse_unowned_maps("web" if web is None else "best", lambda: lib.sm_run_after(
                self._h, _ptr(left), _ptr(right), float(threshold), pairs, _ptr(None), WEB_TYPES[web_dtype], _ptr(None),
                self._stream(), ev))
        web = self._lane_out(web, pairs, "web", web_dtype)
        best = self._lane_out(best, pairs, "best") if want_best else None
        if web_dtype != torch.int32 and not getattr(self, "_narrow_ready", False) and \
                not torch.cuda.is_current_stream_capturing():
            self.reserve_narrow()
        check(lib.sm_run_after(self._h, _ptr(left), _ptr(right), float(threshold), pairs, _ptr(web),
                               WEB_TYPES[web_dtype], _ptr(best if want_best else None), self._stream(), ev))
        return web, (best if want_best else None)

    # ---- left-right consistency check ------------------------------------------
    def match_wta_right(self, pairs=1, want_best=True, web_right=None, best_right=None):
        """The right-reference map of the loaded edges (sm_match_wta_right) -> (web_right, best_right):
        web_right(u, y) = s' means right pixel u matched left pixel u - (s' - 1)."""
        web_right = self._out(web_right, pairs, "web_right")
        best_right = self._out(best_right, pairs, "best_right") if want_best else None
        check(lib.sm_match_wta_right(self._h, pairs, _ptr(web_right), _ptr(best_right), self._stream()))
        return web_right, best_right

    def lr_check(self, web, web_right, max_diff=0, out=None):
        """Left-right consistency check (sm_lr_check) -> (checked web, rejected pixels per pair): a left pixel
        whose right-reference map does not point back to it within max_diff becomes 0.  out=web checks in place."""
        web = self._images(web, torch.int32, "web")
        web_right = self._images(web_right, torch.int32, "web_right")
        pairs = web.shape[0]
        if web_right.shape[0] != pairs:
            raise ValueError(f"web_right: {web_right.shape[0]} maps for {pairs} pairs")
        out = self._out(out, pairs, "out")
        rejected = torch.empty(pairs, dtype=torch.int32, device=self._dev)
        check(lib.sm_lr_check(self._h, _ptr(web), _ptr(web_right), int(max_diff), pairs, _ptr(out), _ptr(rejected),
                              self._stream()))
        return out, rejected

    def run_lr(self, left, right, threshold=DEFAULT_THRESHOLD, max_diff=0, want_right=False, want_best=False,
               web=None, web_right=None, best=None) -> LRResult:
        """Edges, left match, right match and check in one call (sm_run_lr) -> LRResult(web, rejected, web_right,
        best); web is the checked map (0 = rejected)."""
        left = self._images(left, torch.uint8, "left")
        right = self._images(right, torch.uint8, "right")
        pairs = left.shape[0]
        web = self._out(web, pairs, "web")
        web_right = self._out(web_right, pairs, "web_right") if want_right else None
        best = self._out(best, pairs, "best") if want_best else None
        rejected = torch.empty(pairs, dtype=torch.int32, device=self._dev)
        check(lib.sm_run_lr(self._h, _ptr(left), _ptr(right), float(threshold), pairs, int(max_diff), _ptr(web),
                            _ptr(best), _ptr(web_right), _ptr(rejected), self._stream()))
        return LRResult(web, rejected, web_right, best)

    # ---- the cost modes' left, right and checked calls -------------------------
    def _pair(self, left, right):
        left = self._images(left, torch.uint8, "left")
        right = self._images(right, torch.uint8, "right")
        if right.shape[0] != left.shape[0]:
            raise ValueError(f"right: {right.shape[0]} images for {left.shape[0]} pairs")
        return left, right, left.shape[0]

    def _prior(self, prior, pairs, name):
        prior = self._images(prior, torch.int32, name)
        if prior.shape[0] != pairs:
            raise ValueError(f"{name}: {prior.shape[0]} maps for {pairs} pairs")
        return prior

    def _match_one(self, fn, mode, left, right, side, want_best, web, best, priors=(), want_sub=None, sub=None):
        """One direction of a cost mode -> (web, best), with sub behind them where the mode has one (want_sub is not
        None).  fn is the C function; mode(pairs, *prior pointers) gives its arguments from behind the images to before
        the maps (evaluated last, as the call is made); side is "" or "_right", the suffix of the maps' names; priors
        is (map, name) for every prior map the mode takes."""
        left, right, pairs = self._pair(left, right)
        priors = [_ptr(self._prior(p, pairs, name)) for p, name in priors]
        maps = [self._out(web, pairs, "web" + side), self._out(best, pairs, "best" + side) if want_best else None]
        if want_sub is not None:
            maps.append(self._out(sub, pairs, "sub", torch.int16) if want_sub else None)
        check(fn(self._h, _ptr(left), _ptr(right), *mode(pairs, *priors), *map(_ptr, maps), self._stream()))
        return tuple(maps)

    def _match_lr(self, fn, mode, left, right, max_diff, want_right, want_best, web, web_right, best, priors=(),
                  want_sub=None, sub=None):
        """Both directions of a cost mode and the check -> (web, rejected, web_right, best), with sub behind them where
        the mode has one: the fields of LRResult / SGMLRResult.  fn, mode, priors: as _match_one's."""
        left, right, pairs = self._pair(left, right)
        priors = [_ptr(self._prior(p, pairs, name)) for p, name in priors]
        web = self._out(web, pairs, "web")
        web_right = self._out(web_right, pairs, "web_right") if want_right else None
        best = self._out(best, pairs, "best") if want_best else None
        subs = [] if want_sub is None else [self._out(sub, pairs, "sub", torch.int16) if want_sub else None]
        rejected = torch.empty(pairs, dtype=torch.int32, device=self._dev)
        check(fn(self._h, _ptr(left), _ptr(right), *mode(pairs, *priors), int(max_diff), _ptr(web), _ptr(best),
                 _ptr(web_right), _ptr(rejected), *map(_ptr, subs), self._stream()))
        return (web, rejected, web_right, best, *subs)

    def cost_wta(self, left, right, cost="sad", want_best=True, web=None, best=None):
        """SAD / SSD cost mode on the uint8 images (parity unpinned: the reference has no
        such mode) -> (web, best): arg-min over the shifts, first shift wins."""
        left = self._images(left, torch.uint8, "left")
        right = self._images(right, torch.uint8, "right")
        pairs = left.shape[0]
        if web is None:
            web = self._new(pairs, torch.int32)
        if best is None and want_best:
            best = self._new(pairs, torch.int32)
        check(lib.sm_cost_wta(self._h, _ptr(left), _ptr(right), {"sad": 1, "ssd": 2}[cost], pairs,
                              _ptr(web), _ptr(best), self._stream()))
        return web, best

    def cost_wta_right(self, left, right, cost="sad", want_best=True, web_right=None, best_right=None):
        """The cost mode's right-reference map (sm_cost_wta_right) -> (web_right, best_right): web_right(u, y) = s'
        means right pixel u matched left pixel u - (s' - 1), best_right its window cost."""
        return self._match_one(lib.sm_cost_wta_right, lambda pairs: ({"sad": 1, "ssd": 2}[cost], pairs), left, right,
                               "_right", want_best, web_right, best_right)

    def cost_lr(self, left, right, cost="sad", max_diff=0, want_right=False, want_best=False, web=None,
                web_right=None, best=None) -> LRResult:
        """Left cost WTA, right cost WTA and check in one call (sm_cost_lr) -> LRResult(web, rejected, web_right,
        best); web is the checked map (0 = rejected), best the left window costs as cost_wta gives them."""
        return LRResult(*self._match_lr(lib.sm_cost_lr, lambda pairs: ({"sad": 1, "ssd": 2}[cost], pairs), left, right,
                                        max_diff, want_right, want_best, web, web_right, best))

    def cost_refine(self, left, right, web, cost="sad", want_costs=False, out=None):
        """Subpixel refinement of a cost_wta map (sm_cost_refine) -> (sub, costs): sub is int16 in 1/16 of a shift
        (SSD: parabola, SAD: equiangular fit over C(s-2), C(s-1), C(s); 0 where web is outside 1..D), costs the
        three window costs as (pairs, 3, H, W) int32 with -1 where a shift has none, if wanted."""
        left = self._images(left, torch.uint8, "left")
        right = self._images(right, torch.uint8, "right")
        web = self._images(web, torch.int32, "web")
        pairs = left.shape[0]
        if right.shape[0] != pairs or web.shape[0] != pairs:
            raise ValueError(f"right / web: {right.shape[0]} / {web.shape[0]} maps for {pairs} pairs")
        out = self._out(out, pairs, "out", torch.int16)
        costs = None
        if want_costs:
            costs = torch.empty((pairs, 3, self.height, self.width), dtype=torch.int32, device=self._dev)
        check(lib.sm_cost_refine(self._h, _ptr(left), _ptr(right), {"sad": 1, "ssd": 2}[cost], pairs, _ptr(web),
                                 _ptr(out), _ptr(costs), self._stream()))
        return out, costs

    # ---- census cost mode ----------------------------------------------------
    def reserve_census(self):
        """The census mode's workspace (the descriptors of max_pairs pairs, and the mirrored-order map if the plan has
        none yet), allocated now: keeps the allocation out of timed paths and out of stream captures."""
        check(lib.sm_plan_reserve_census(self._h))

    def census_transform(self, images, census=7, out=None):
        """Census descriptors of uint8 gray images (sm_census_transform) -> int64 tensor of their bits, same shape:
        bit k = the k-th neighbour of the census x census window (row-major, centre skipped) is darker than the pixel."""
        images = self._images(images, torch.uint8, "images")
        n = images.shape[0]
        if out is None:
            out = self._new(n, torch.int64)
        else:
            out = self._images(out, torch.int64, "out")
            if out.shape[0] < n:
                raise ValueError(f"out: room for {out.shape[0]} images, {n} given")
        check(lib.sm_census_transform(self._h, _ptr(images), int(census), n, _ptr(out), self._stream()))
        return out

    def census_wta(self, left, right, census=7, want_best=True, web=None, best=None):
        """Census cost mode (parity unpinned) -> (web, best): Hamming cost of census descriptors, n x n box sum,
        arg-min over the shifts, first shift wins."""
        return self._match_one(lib.sm_census_wta, lambda pairs: (int(census), pairs), left, right, "", want_best, web,
                               best)

    def census_wta_right(self, left, right, census=7, want_best=True, web_right=None, best_right=None):
        """The census mode's right-reference map (sm_census_wta_right) -> (web_right, best_right): web_right(u, y) = s'
        means right pixel u matched left pixel u - (s' - 1)."""
        return self._match_one(lib.sm_census_wta_right, lambda pairs: (int(census), pairs), left, right, "_right",
                               want_best, web_right, best_right)

    def census_lr(self, left, right, census=7, max_diff=0, want_right=False, want_best=False, web=None,
                  web_right=None, best=None) -> LRResult:
        """Left and right census arg-min and the check in one call (sm_census_lr) -> LRResult(web, rejected, web_right,
        best); web is the checked map (0 = rejected), best the left window costs as census_wta gives them."""
        return LRResult(*self._match_lr(lib.sm_census_lr, lambda pairs: (int(census), pairs), left, right, max_diff,
                                        want_right, want_best, web, web_right, best))

    def census_refine(self, left, right, web, census=7, want_costs=False, out=None):
        """Subpixel refinement of a census map (sm_census_refine) -> (sub, costs): sub int16 in 1/16 of a shift by the
        equiangular fit over C(s-2), C(s-1), C(s) (0 where web is outside 1..D), costs (pairs, 3, H, W) int32 with -1
        where a shift has none, if wanted."""
        left, right, pairs = self._pair(left, right)
        web = self._images(web, torch.int32, "web")
        if web.shape[0] != pairs:
            raise ValueError(f"web: {web.shape[0]} maps for {pairs} pairs")
        out = self._out(out, pairs, "out", torch.int16)
        costs = None
        if want_costs:
            costs = torch.empty((pairs, 3, self.height, self.width), dtype=torch.int32, device=self._dev)
        check(lib.sm_census_refine(self._h, _ptr(left), _ptr(right), int(census), pairs, _ptr(web), _ptr(out),
                                   _ptr(costs), self._stream()))
        return out, costs

    def census_wta_near(self, left, right, prior, census=7, radius=1, want_best=True, web=None, best=None):
        """Guided census re-search (sm_census_wta_near) -> (web, best): census_wta's arg-min over the shifts within
        `radius` (1..4) of the int32 web map `prior` (1 + shift, 0 invalid) only -- the upsampled map of the
        half-resolution path; web = best = 0 where the prior leaves no shift."""
        return self._match_one(lib.sm_census_wta_near, lambda pairs, p: (int(census), pairs, p, int(radius)), left, right,
                               "", want_best, web, best, priors=((prior, "prior"),))

    def census_wta_near_right(self, left, right, prior_right, census=7, radius=1, want_best=True, web_right=None,
                              best_right=None):
        """The right-reference re-search (sm_census_wta_near_right) -> (web_right, best_right), around a
        right-reference prior map."""
        return self._match_one(lib.sm_census_wta_near_right, lambda pairs, p: (int(census), pairs, p, int(radius)), left,
                               right, "_right", want_best, web_right, best_right, priors=((prior_right, "prior_right"),))

    def census_near_lr(self, left, right, prior, prior_right, census=7, radius=1, max_diff=0, want_right=False,
                       want_best=False, web=None, web_right=None, best=None) -> LRResult:
        """Both re-searches and the check in one call (sm_census_near_lr) -> LRResult(web, rejected, web_right, best),
        shaped like census_lr's."""
        return LRResult(*self._match_lr(
            lib.sm_census_near_lr, lambda pairs, p, q: (int(census), pairs, p, q, int(radius)), left, right, max_diff,
            want_right, want_best, web, web_right, best, priors=((prior, "prior"), (prior_right, "prior_right"))))

    # ---- semi-global matching over the census data term ------------------------
    def reserve_sgm(self):
        """The SGM workspace (the census workspace, and the data-term and aggregate volumes of one pair), allocated now:
        keeps the allocation out of timed paths and out of stream captures."""
        check(lib.sm_plan_reserve_sgm(self._h))

    def sgm_wta(self, left, right, census=7, p1=10, p2=120, paths=8, want_best=True, want_sub=False, web=None,
                best=None, sub=None):
        """Semi-global matching over the census cost (sm_sgm_wta, parity unpinned) -> (web, best, sub): the census
        window cost aggregated along `paths` (4 or 8) image lines with penalty p1 for a one-shift step and p2 for a
        larger jump, arg-min over the shifts (first shift wins), best = the minimum aggregate, sub int16 in 1/16 of a
        shift (parabola fit on the aggregates).  Outputs not wanted are None.  The default penalties suit a 1 x 1
        window (the pixelwise census cost, at most 48); window costs grow with n^2, so scale p1 and p2 with it."""
        return self._match_one(lib.sm_sgm_wta, lambda pairs: (int(census), int(p1), int(p2), int(paths), pairs), left,
                               right, "", want_best, web, best, want_sub=want_sub, sub=sub)

    def sgm_wta_right(self, left, right, census=7, p1=10, p2=120, paths=8, want_best=True, web_right=None,
                      best_right=None):
        """The SGM right-reference map (sm_sgm_wta_right) -> (web_right, best_right): web_right(u, y) = s' means right
        pixel u matched left pixel u - (s' - 1)."""
        return self._match_one(lib.sm_sgm_wta_right, lambda pairs: (int(census), int(p1), int(p2), int(paths), pairs),
                               left, right, "_right", want_best, web_right, best_right)

    def sgm_lr(self, left, right, census=7, p1=10, p2=120, paths=8, max_diff=0, want_right=False, want_best=False,
               want_sub=False, web=None, web_right=None, best=None, sub=None) -> SGMLRResult:
        """Left and right SGM and the check in one call (sm_sgm_lr) -> SGMLRResult(web, rejected, web_right, best,
        sub); web is the checked map (0 = rejected), best the left minima, sub the left subpixel map with 0 where
        rejected."""
        return SGMLRResult(*self._match_lr(
            lib.sm_sgm_lr, lambda pairs: (int(census), int(p1), int(p2), int(paths), pairs), left, right, max_diff,
            want_right, want_best, web, web_right, best, want_sub=want_sub, sub=sub))

    def sgm_wta_both(self, left, right, census=7, p1=10, p2=120, paths=8, want_best=True, want_sub=False,
                     want_best_right=True, web=None, best=None, sub=None, web_right=None, best_right=None):
        """sgm_wta's maps and a right-reference map read off the same aggregate (sm_sgm_wta_both) -> (web, best, sub,
        web_right, best_right): web_right(u, y) = 1 + the least d minimising S(y, u - d, d) over the left pixels that
        the border mode gives right pixel u (toroidal: all, modulo the width; ghost: d <= u).  One aggregation instead
        of sgm_wta + sgm_wta_right's two; the right map is not sgm_wta_right's.  Outputs not wanted are None."""
        left, right, pairs = self._pair(left, right)
        web = self._out(web, pairs, "web")
        best = self._out(best, pairs, "best") if want_best else None
        sub = self._out(sub, pairs, "sub", torch.int16) if want_sub else None
        web_right = self._out(web_right, pairs, "web_right")
        best_right = self._out(best_right, pairs, "best_right") if want_best_right else None
        check(lib.sm_sgm_wta_both(self._h, _ptr(left), _ptr(right), int(census), int(p1), int(p2), int(paths), pairs,
                                  _ptr(web), _ptr(best), _ptr(sub), _ptr(web_right), _ptr(best_right), self._stream()))
        return web, best, sub, web_right, best_right

    def sgm_lr_single(self, left, right, census=7, p1=10, p2=120, paths=8, max_diff=0, want_right=False,
                      want_best=False, want_sub=False, web=None, web_right=None, best=None, sub=None) -> SGMLRResult:
        """sgm_lr with sgm_wta_both's right map (sm_sgm_lr_single) -> SGMLRResult, shaped like sgm_lr's: one
        aggregation and the check, about half of sgm_lr's time."""
        return SGMLRResult(*self._match_lr(
            lib.sm_sgm_lr_single, lambda pairs: (int(census), int(p1), int(p2), int(paths), pairs), left, right, max_diff,
            want_right, want_best, web, web_right, best, want_sub=want_sub, sub=sub))

    # ---- cross-based adaptive support over the census cost ---------------------
    def reserve_cross(self):
        """The cross-based mode's workspace (the census workspace, and the packed arms of both images of max_pairs
        pairs), allocated now: keeps the allocation out of timed paths and out of stream captures."""
        check(lib.sm_plan_reserve_cross(self._h))

    def cross_arms(self, images, tau=20, arm=10, want_support=False, out=None):
        """The support arms of uint8 gray images (sm_cross_arms) -> (arms, support): arms uint16 l | r << 4 | u << 8 |
        d << 12, how far the pixel's support reaches left, right, up and down (at most `arm` pixels, never past a
        pixel that differs from it by more than tau, never outside the image); support int32, the number of pixels of
        the support, or None."""
        images = self._images(images, torch.uint8, "images")
        n = images.shape[0]
        if out is None:
            out = self._new(n, torch.uint16)
        else:
            out = self._images(out, torch.uint16, "out")
            if out.shape[0] < n:
                raise ValueError(f"out: room for {out.shape[0]} images, {n} given")
        support = self._new(n, torch.int32) if want_support else None
        check(lib.sm_cross_arms(self._h, _ptr(images), int(tau), int(arm), n, _ptr(out), _ptr(support), self._stream()))
        return out, support

    def cross_wta(self, left, right, census=7, tau=20, arm=10, want_best=True, want_sub=False, web=None, best=None,
                  sub=None):
        """Cross-based matcher (sm_cross_wta, parity unpinned) -> (web, best, sub): the census Hamming cost summed over
        each left pixel's own support (cross_arms of the left image; the plan's window plays no part), arg-min over
        the shifts, first shift wins; best = the minimum sum, sub int16 in 1/16 of a shift (equiangular fit).  Outputs
        not wanted are None."""
        return self._match_one(lib.sm_cross_wta, lambda pairs: (int(census), int(tau), int(arm), pairs), left, right, "",
                               want_best, web, best, want_sub=want_sub, sub=sub)

    def cross_wta_right(self, left, right, census=7, tau=20, arm=10, want_best=True, web_right=None, best_right=None):
        """The cross-based right-reference map (sm_cross_wta_right) -> (web_right, best_right), over the supports of
        the right image: web_right(u, y) = s' means right pixel u matched left pixel u - (s' - 1)."""
        return self._match_one(lib.sm_cross_wta_right, lambda pairs: (int(census), int(tau), int(arm), pairs), left,
                               right, "_right", want_best, web_right, best_right)

    def cross_lr(self, left, right, census=7, tau=20, arm=10, max_diff=0, want_right=False, want_best=False,
                 want_sub=False, web=None, web_right=None, best=None, sub=None) -> SGMLRResult:
        """Both cross-based passes and the check in one call (sm_cross_lr) -> SGMLRResult(web, rejected, web_right,
        best, sub); web is the checked map (0 = rejected), best the left minima, sub the left subpixel map with 0 where
        rejected."""
        return SGMLRResult(*self._match_lr(
            lib.sm_cross_lr, lambda pairs: (int(census), int(tau), int(arm), pairs), left, right, max_diff, want_right,
            want_best, web, web_right, best, want_sub=want_sub, sub=sub))

    # ---- banded SGM: aggregation within +-radius of a prior map -----------------
    def reserve_sgm_near(self):
        """The banded SGM workspace (the census workspace, and one pair's banded volumes, 96 bytes a pixel), allocated
        now: keeps the allocation out of timed paths and out of stream captures."""
        check(lib.sm_plan_reserve_sgm_near(self._h))

    def sgm_wta_near(self, left, right, prior, census=7, p1=10, p2=120, paths=8, radius=1, want_best=True,
                     want_sub=False, web=None, best=None, sub=None):
        """SGM within `radius` (1..4) of the int32 web map `prior` (sm_sgm_wta_near, parity unpinned) -> (web, best,
        sub): census_wta_near's candidates aggregated along `paths` lines with sgm_wta's penalties; a pixel whose
        prior leaves no shift breaks the paths through it and gets web = best = sub = 0."""
        return self._match_one(lib.sm_sgm_wta_near,
                               lambda pairs, p: (int(census), int(p1), int(p2), int(paths), pairs, p, int(radius)), left,
                               right, "", want_best, web, best, priors=((prior, "prior"),), want_sub=want_sub, sub=sub)

    def sgm_wta_near_right(self, left, right, prior_right, census=7, p1=10, p2=120, paths=8, radius=1, want_best=True,
                           web_right=None, best_right=None):
        """The right-reference banded SGM (sm_sgm_wta_near_right) -> (web_right, best_right), around a right-reference
        prior map."""
        return self._match_one(lib.sm_sgm_wta_near_right,
                               lambda pairs, p: (int(census), int(p1), int(p2), int(paths), pairs, p, int(radius)), left,
                               right, "_right", want_best, web_right, best_right, priors=((prior_right, "prior_right"),))

    def sgm_near_lr(self, left, right, prior, prior_right, census=7, p1=10, p2=120, paths=8, radius=1, max_diff=0,
                    want_right=False, want_best=False, want_sub=False, web=None, web_right=None, best=None,
                    sub=None) -> SGMLRResult:
        """Both banded passes and the check in one call (sm_sgm_near_lr) -> SGMLRResult(web, rejected, web_right, best,
        sub), shaped like sgm_lr's."""
        return SGMLRResult(*self._match_lr(
            lib.sm_sgm_near_lr,
            lambda pairs, p, q: (int(census), int(p1), int(p2), int(paths), pairs, p, q, int(radius)), left, right,
            max_diff, want_right, want_best, web, web_right, best,
            priors=((prior, "prior"), (prior_right, "prior_right")), want_sub=want_sub, sub=sub))

    # ---- match uniqueness: runner-up, ratio filter, confidence ---------------------
    def census_second(self, left, right, web, census=7, want_best=True, web2=None, best2=None):
        """The runner-up of the census search (sm_census_second) -> (web2, best2): census_wta's arg-min over the shifts
        further than 1 from the shift of the int32 map `web` (1 + shift; 0 and anything outside 1..D: over all shifts);
        web2 = 0 and best2 = -1 where no shift is left.  `web` may be census_wta's own map, a checked map, a re-search
        map."""
        left, right, pairs = self._pair(left, right)
        web = self._prior(web, pairs, "web")
        web2 = self._out(web2, pairs, "web2")
        best2 = self._out(best2, pairs, "best2") if want_best else None
        check(lib.sm_census_second(self._h, _ptr(left), _ptr(right), int(census), pairs, _ptr(web), _ptr(web2),
                                   _ptr(best2), self._stream()))
        return web2, best2

    def sgm_wta2(self, left, right, census=7, p1=10, p2=120, paths=8, want_best=True, want_sub=False, want_best2=True,
                 web=None, best=None, sub=None, web2=None, best2=None):
        """sgm_wta with the runner-up of the aggregate beside it (sm_sgm_wta2) -> (web, best, sub, web2, best2): the
        first three exactly as sgm_wta gives them, web2 / best2 the arg-min of S over the shifts further than 1 from
        the winner's (web2 = 0, best2 = -1 where there is none).  Outputs not wanted are None."""
        left, right, pairs = self._pair(left, right)
        web = self._out(web, pairs, "web")
        best = self._out(best, pairs, "best") if want_best else None
        sub = self._out(sub, pairs, "sub", torch.int16) if want_sub else None
        web2 = self._out(web2, pairs, "web2")
        best2 = self._out(best2, pairs, "best2") if want_best2 else None
        check(lib.sm_sgm_wta2(self._h, _ptr(left), _ptr(right), int(census), int(p1), int(p2), int(paths), pairs,
                              _ptr(web), _ptr(best), _ptr(sub), _ptr(web2), _ptr(best2), self._stream()))
        return web, best, sub, web2, best2

    def _unique_maps(self, web, best, best2):
        web = self._images(web, torch.int32, "web")
        pairs = web.shape[0]
        return web, self._prior(best, pairs, "best"), self._prior(best2, pairs, "best2"), pairs

    def uniqueness_filter(self, web, best, best2, ratio, out=None, want_rejected=False):
        """The uniqueness test (sm_uniqueness_filter) -> the filtered map, or (map, rejected pixels per pair) with
        want_rejected: a valid pixel stays iff it has no rival (best2 < 0) or best2 * (100 - ratio) >= best * 100,
        ratio in 0..100 (OpenCV's uniquenessRatio).  out=web filters in place; sub_mask lets a sub map follow."""
        web, best, best2, pairs = self._unique_maps(web, best, best2)
        out = self._out(out, pairs, "out")
        rejected = torch.empty(pairs, dtype=torch.int32, device=self._dev) if want_rejected else None
        check(lib.sm_uniqueness_filter(self._h, _ptr(web), _ptr(best), _ptr(best2), int(ratio), pairs, _ptr(out),
                                       _ptr(rejected), self._stream()))
        return (out, rejected) if want_rejected else out

    def confidence(self, web, best, best2, out=None):
        """Per-pixel confidence (sm_confidence) -> uint8 map: 0 where web = 0, 255 where there is no rival, 0 where
        best2 <= best, else min(255, 255 * (best2 - best) // best2)."""
        web, best, best2, pairs = self._unique_maps(web, best, best2)
        out = self._out(out, pairs, "out", torch.uint8)
        check(lib.sm_confidence(self._h, _ptr(web), _ptr(best), _ptr(best2), pairs, _ptr(out), self._stream()))
        return out

    # ---- disparity post-filters (between the check and step 3) ------------------
    def reserve_filter(self):
        """The speckle filter's workspace (a label and a component size per pixel of max_pairs maps), allocated now:
        keeps the allocation out of timed paths and out of stream captures."""
        check(lib.sm_plan_reserve_filter(self._h))

    def _filter_map(self, t, name):
        if t.dtype not in MAP_TYPES:
            raise ValueError(f"{name}: need an int32 (web) or int16 (sub) map, got {t.dtype}")
        return self._images(t, t.dtype, name)

    def median_filter(self, map, k=3, out=None):
        """Validity-aware k x k median (sm_median_filter) of an int32 web map or an int16 sub map -> the filtered map:
        0 stays 0, a valid pixel becomes the lower median of the valid values of its window that lie in the image."""
        map = self._filter_map(map, "map")
        pairs = map.shape[0]
        out = self._out(out, pairs, "out", map.dtype)
        check(lib.sm_median_filter(self._h, _ptr(map), MAP_TYPES[map.dtype], int(k), pairs, _ptr(out), self._stream()))
        return out

    def speckle_filter(self, map, max_size, max_diff, out=None, want_removed=False):
        """Speckle removal (sm_speckle_filter) of an int32 or int16 map -> the filtered map, or (map, removed pixels
        per pair) with want_removed: valid pixels whose 4-connected component (neighbours joined where their values
        differ by at most max_diff) has at most max_size pixels become 0.  out=map filters in place."""
        map = self._filter_map(map, "map")
        pairs = map.shape[0]
        out = self._out(out, pairs, "out", map.dtype)
        removed = torch.empty(pairs, dtype=torch.int32, device=self._dev) if want_removed else None
        check(lib.sm_speckle_filter(self._h, _ptr(map), MAP_TYPES[map.dtype], int(max_size), int(max_diff), pairs,
                                    _ptr(out), _ptr(removed), self._stream()))
        return (out, removed) if want_removed else out

    def sub_mask(self, web, sub):
        """sub = 0 where web = 0, in place (sm_sub_mask) -> sub: lets a subpixel map follow a web map that
        speckle_filter has thinned."""
        web = self._images(web, torch.int32, "web")
        sub = self._images(sub, torch.int16, "sub")
        if sub.shape[0] != web.shape[0]:
            raise ValueError(f"sub: {sub.shape[0]} maps for {web.shape[0]} pairs")
        check(lib.sm_sub_mask(self._h, _ptr(web), _ptr(sub), web.shape[0], self._stream()))
        return sub

    # ---- guided weighted median (between the speckle filter and the interpolation) ---
    def weighted_median(self, map, guide, radius, weights, fill=False, fill_min_weight=1, out=None, want_filled=False):
        """Guided weighted median (sm_weighted_median) of an int32 web map or an int16 sub map -> the filtered map, or
        (map, filled pixels per pair) with want_filled.  guide: uint8 images of the map's shape (the rectified left
        image); weights: 256 integers, the weight of a tap by the gray difference between it and the centre in the
        guide (guide_weights).  A valid pixel becomes the lower weighted median of the valid pixels of its
        (2 radius + 1)^2 window; 0 stays 0 unless fill is set and the window's weights sum to fill_min_weight or more."""
        map = self._filter_map(map, "map")
        pairs = map.shape[0]
        guide = self._images(guide, torch.uint8, "guide")
        if guide.shape[0] != pairs:
            raise ValueError(f"guide: {guide.shape[0]} images for {pairs} pairs")
        out = self._out(out, pairs, "out", map.dtype)
        filled = torch.empty(pairs, dtype=torch.int32, device=self._dev) if want_filled else None
        check(lib.sm_weighted_median(self._h, _ptr(map), MAP_TYPES[map.dtype], _ptr(guide), int(radius), capi.w256(weights),
                                     capi.SM_WMED_FILL if fill else 0, int(fill_min_weight), pairs, _ptr(out), _ptr(filled),
                                     self._stream()))
        return (out, filled) if want_filled else out

    # ---- edge-aware smoother (after the speckle filter; its output is dense) --------
    def reserve_wls(self):
        """The smoother's workspace (three double planes per pixel of max_pairs maps), allocated now: keeps the
        allocation out of timed paths and out of stream captures."""
        check(lib.sm_plan_reserve_wls(self._h))

    def wls_filter(self, map, guide, weights, lam, iterations=3, conf=None, fill=True, out=None, out_dtype=None,
                   want_raw=False, want_filled=False):
        """Confidence-weighted edge-aware smoother (sm_wls_filter) of an int32 web map or an int16 sub map -> the
        smoothed map of out_dtype (default: the map's), then the raw quotient (float64, sixteenths of a pixel) with
        want_raw, then the filled pixels per pair with want_filled.  guide: uint8 images of the map's shape; weights: 256
        integers, the smoothness weight of two neighbours by their gray difference in the guide (guide_weights; lam
        multiplies the entries as they are, so pass lam / peak with it); conf: uint8 confidence map (confidence()) or
        None for 255 everywhere.  fill=False leaves invalid pixels 0.  out=map smooths in place (same dtype)."""
        map = self._filter_map(map, "map")
        pairs = map.shape[0]
        guide = self._images(guide, torch.uint8, "guide")
        if guide.shape[0] != pairs:
            raise ValueError(f"guide: {guide.shape[0]} images for {pairs} pairs")
        if conf is not None:
            conf = self._images(conf, torch.uint8, "conf")
            if conf.shape[0] != pairs:
                raise ValueError(f"conf: {conf.shape[0]} maps for {pairs} pairs")
        out_dtype = out_dtype or (out.dtype if out is not None else map.dtype)
        if out_dtype not in MAP_TYPES:
            raise ValueError(f"out_dtype: need int32 or int16, got {out_dtype}")
        out = self._out(out, pairs, "out", out_dtype)
        raw = torch.empty((pairs, self.height, self.width), dtype=torch.float64, device=self._dev) if want_raw else None
        filled = torch.empty(pairs, dtype=torch.int32, device=self._dev) if want_filled else None
        check(lib.sm_wls_filter(self._h, _ptr(map), MAP_TYPES[map.dtype], _ptr(conf), _ptr(guide), capi.w256(weights),
                                float(lam), int(iterations), 0 if fill else capi.SM_WLS_NO_FILL, pairs, _ptr(out),
                                MAP_TYPES[out_dtype], _ptr(raw), _ptr(filled), self._stream()))
        res = (out,) + ((raw,) if want_raw else ()) + ((filled,) if want_filled else ())
        return res if len(res) > 1 else out

    # ---- half-resolution path (reduce -> a matcher on a plan of half_shape() -> upsample) ---
    def half_shape(self):
        """(cw, ch) = ((W + 1) >> 1, (H + 1) >> 1): the size reduce_half writes and upsample_double reads; the coarse
        matcher runs on a second plan, StereoPlan(cw, ch, num_shifts // 2, ...), that the caller makes"""
        return (self.width + 1) >> 1, (self.height + 1) >> 1

    def _coarse(self, t, dtype, name):
        cw, ch = self.half_shape()
        if t.device != self._dev or t.dtype != dtype or not t.is_contiguous():
            raise ValueError(f"{name}: need a contiguous {dtype} tensor on {self._dev}, got {t.dtype} on {t.device}")
        if t.dim() == 2:
            t = t.unsqueeze(0)
        if t.dim() != 3 or t.shape[1] != ch or t.shape[2] != cw:
            raise ValueError(f"{name}: shape {tuple(t.shape)} is not (pairs, {ch}, {cw})")
        return t

    def reduce_half(self, images, filter="binomial", out=None):
        """Images of the plan's size reduced by two in each direction (sm_reduce_half) -> uint8 (images, ch, cw).
        images: uint8 (n, H, W), n up to 2 * max_pairs (both sides of a batch in one call); filter: "binomial"
        ([1, 3, 3, 1] in each direction) or "box" (the 2 x 2 mean), both centred on the 2 x 2 block and rounded."""
        if filter not in REDUCE_FILTERS:
            raise ValueError(f"filter: {filter!r} is not one of {sorted(REDUCE_FILTERS)}")
        images = self._images(images, torch.uint8, "images")
        n = images.shape[0]
        if out is None:
            cw, ch = self.half_shape()
            out = torch.empty((n, ch, cw), dtype=torch.uint8, device=self._dev)
        else:
            out = self._coarse(out, torch.uint8, "out")
            if out.shape[0] < n:
                raise ValueError(f"out: room for {out.shape[0]} images, {n} given")
        check(lib.sm_reduce_half(self._h, _ptr(images), REDUCE_FILTERS[filter], n, _ptr(out), self._stream()))
        return out

    def upsample_double(self, map, guide, guide_coarse, weights, fill=False, out=None):
        """A map of half_shape() brought to the plan's size along the edges of the guide (sm_upsample_double) -> the fine
        map, of the coarse map's type (int32 web: 2 v - 1; int16 sub: 2 v - 16).  guide: uint8 images of the plan's
        size; guide_coarse: the same reduced (reduce_half); weights: 256 integers >= 1 (guide_weights).  A fine pixel
        becomes the lower weighted median of the valid coarse pixels among its home and the eight around it; where
        the home is invalid it stays 0 unless fill is set."""
        if map.dtype not in MAP_TYPES:
            raise ValueError(f"map: need an int32 (web) or int16 (sub) map, got {map.dtype}")
        map = self._coarse(map, map.dtype, "map")
        pairs = map.shape[0]
        guide = self._images(guide, torch.uint8, "guide")
        guide_coarse = self._coarse(guide_coarse, torch.uint8, "guide_coarse")
        if guide.shape[0] != pairs or guide_coarse.shape[0] != pairs:
            raise ValueError(f"guide, guide_coarse: {guide.shape[0]} and {guide_coarse.shape[0]} images for {pairs} pairs")
        out = self._out(out, pairs, "out", map.dtype)
        check(lib.sm_upsample_double(self._h, _ptr(map), MAP_TYPES[map.dtype], _ptr(guide), _ptr(guide_coarse),
                                     capi.w256(weights), capi.SM_UP_FILL if fill else 0, pairs, _ptr(out), self._stream()))
        return out

    # ---- occlusion-aware interpolation (between the post-filters and step 3) -----
    def reserve_interp(self):
        """The interpolation's workspace (six directional maps and the carries of their sweeps for max_pairs maps),
        allocated now: keeps the allocation out of timed paths and out of stream captures."""
        check(lib.sm_plan_reserve_interp(self._h))

    def occlusion_classify(self, web, web_right, out=None):
        """Class of every pixel of a checked web map (sm_occlusion_classify) -> uint8 tensor: 0 valid, 1 occluded, 2
        mismatched (the pixel's line of sight meets the right-reference map web_right of the check)."""
        web = self._images(web, torch.int32, "web")
        web_right = self._images(web_right, torch.int32, "web_right")
        pairs = web.shape[0]
        if web_right.shape[0] != pairs:
            raise ValueError(f"web_right: {web_right.shape[0]} maps for {pairs} pairs")
        out = self._out(out, pairs, "out", torch.uint8)
        check(lib.sm_occlusion_classify(self._h, _ptr(web), _ptr(web_right), pairs, _ptr(out), self._stream()))
        return out

    def interpolate(self, maps, cls=None, want_filled=False, out=None):
        """Discontinuity-preserving fill (sm_interpolate) of the 0s of an int32 web map or an int16 sub map -> the
        filled map, or (map, filled pixels per pair) with want_filled: an invalid pixel takes the second lowest of the
        first valid values met along the eight directions where cls is 1 (occluded), else their lower median."""
        maps = self._filter_map(maps, "maps")
        pairs = maps.shape[0]
        if cls is not None:
            cls = self._images(cls, torch.uint8, "cls")
            if cls.shape[0] != pairs:
                raise ValueError(f"cls: {cls.shape[0]} maps for {pairs} pairs")
        out = self._out(out, pairs, "out", maps.dtype)
        filled = torch.empty(pairs, dtype=torch.int32, device=self._dev) if want_filled else None
        check(lib.sm_interpolate(self._h, _ptr(maps), MAP_TYPES[maps.dtype], _ptr(cls), pairs, _ptr(out), _ptr(filled),
                                 self._stream()))
        return (out, filled) if want_filled else out

    # ---- rectification (in front of the matchers) --------------------------------
    def _rectify_map(self, t, name):
        """-> (map, format): [H][W][2] int32 (abs32) or int16 (rel16), contiguous, on the plan's device"""
        fmts = {torch.int32: capi.SM_RMAP_ABS32, torch.int16: capi.SM_RMAP_REL16}
        if t.dtype not in fmts:
            raise ValueError(f"{name}: need an int32 (abs32) or int16 (rel16) map, got {t.dtype}")
        if t.device != self._dev or not t.is_contiguous():
            raise ValueError(f"{name}: need a contiguous tensor on {self._dev}, got one on {t.device}")
        if tuple(t.shape) != (self.height, self.width, 2):
            raise ValueError(f"{name}: shape {tuple(t.shape)} is not ({self.height}, {self.width}, 2)")
        return t, fmts[t.dtype]

    def rectify_map(self, calibration, fmt="rel16", out=None):
        """The W x H map of one side's calibration (sm_rectify_map_build) -> device tensor [H][W][2], int16 for
        fmt="rel16" (refused where a displacement exceeds 1023 pixels: use "abs32"), int32 for "abs32".
        calibration: a capi.RectifyCalib or a dict of RectifyCalib.make's arguments.  Synchronises; not capturable."""
        if fmt not in capi.RMAP_FORMATS:
            raise ValueError(f"fmt: {fmt!r} is not one of {sorted(capi.RMAP_FORMATS)}")
        calib = calibration if isinstance(calibration, capi.RectifyCalib) else capi.RectifyCalib.make(**calibration)
        dtype = torch.int16 if fmt == "rel16" else torch.int32
        if out is None:
            out = torch.empty((self.height, self.width, 2), dtype=dtype, device=self._dev)
        out, _ = self._rectify_map(out, "out")
        if out.dtype != dtype:
            raise ValueError(f"out: {out.dtype} is not the {dtype} of a {fmt} map")
        check(lib.sm_rectify_map_build(self._h, C.byref(calib), capi.RMAP_FORMATS[fmt], _ptr(out), self._stream()))
        return out

    def rectify(self, raw_left, raw_right, map_left, map_right, interp="bilinear", border=0, want_valid=False,
                left=None, right=None):
        """Rectified images of raw pairs (sm_rectify) -> (left, right), or (left, right, valid_left, valid_right) with
        want_valid.  raw_*: uint8 [pairs][src_h][src_w] (or one [src_h][src_w] image) of any size; map_*: one map per
        side (rectify_map, or any [H][W][2] int32 / int16 tensor), both of one format; a tap outside the raw image
        reads `border`; valid_* is 1 where every tap that counts lay inside."""
        if interp not in capi.INTERPS:
            raise ValueError(f"interp: {interp!r} is not one of {sorted(capi.INTERPS)}")
        raws = []
        for t, name in ((raw_left, "raw_left"), (raw_right, "raw_right")):
            if t.device != self._dev or t.dtype != torch.uint8 or not t.is_contiguous():
                raise ValueError(f"{name}: need a contiguous {torch.uint8} tensor on {self._dev}, "
                                 f"got {t.dtype} on {t.device}")
            t = t.unsqueeze(0) if t.dim() == 2 else t
            if t.dim() != 3 or t.shape[1] < 1 or t.shape[2] < 1:
                raise ValueError(f"{name}: shape {tuple(t.shape)} is not (pairs, src_h, src_w)")
            raws.append(t)
        if raws[0].shape != raws[1].shape:
            raise ValueError(f"raw_right: shape {tuple(raws[1].shape)} is not raw_left's {tuple(raws[0].shape)}")
        pairs, src_h, src_w = raws[0].shape
        map_left, fmt = self._rectify_map(map_left, "map_left")
        map_right, fmt_r = self._rectify_map(map_right, "map_right")
        if fmt != fmt_r:
            raise ValueError(f"map_right: {map_right.dtype} is not map_left's {map_left.dtype}")
        left = self._out(left, pairs, "left", torch.uint8)
        right = self._out(right, pairs, "right", torch.uint8)
        vl = self._new(pairs, torch.uint8) if want_valid else None
        vr = self._new(pairs, torch.uint8) if want_valid else None
        check(lib.sm_rectify(self._h, _ptr(raws[0]), _ptr(raws[1]), src_w, src_h, _ptr(map_left), _ptr(map_right), fmt,
                             capi.INTERPS[interp], int(border), pairs, _ptr(left), _ptr(right), _ptr(vl), _ptr(vr),
                             self._stream()))
        return (left, right, vl, vr) if want_valid else (left, right)

    def valid_mask(self, map, valid):
        """map = 0 where valid = 0, in place (sm_valid_mask) -> map: an int32 web map or an int16 sub map follows the
        validity image rectify returns."""
        map = self._filter_map(map, "map")
        valid = self._images(valid, torch.uint8, "valid")
        if valid.shape[0] != map.shape[0]:
            raise ValueError(f"valid: {valid.shape[0]} images for {map.shape[0]} maps")
        check(lib.sm_valid_mask(self._h, _ptr(map), MAP_TYPES[map.dtype], _ptr(valid), map.shape[0], self._stream()))
        return map

    # ---- reprojection (behind the filters and the interpolation) -----------------
    def reserve_cloud(self):
        """point_cloud's workspace (one count per tile of 1024 pixels of max_pairs maps), allocated now: keeps the
        allocation out of timed paths and out of stream captures."""
        check(lib.sm_plan_reserve_cloud(self._h))

    @staticmethod
    def _z_range(z_range):
        lo, hi = (float("-inf"), float("inf")) if z_range is None else z_range
        return float(lo), float(hi)

    def _float_out(self, t, shape, name):
        """a caller's float32 result buffer (checked like an input), or a new one"""
        if t is None:
            return torch.empty(shape, dtype=torch.float32, device=self._dev)
        if t.device != self._dev or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{name}: need a contiguous {torch.float32} tensor on {self._dev}, got {t.dtype} on {t.device}")
        if t.dim() != len(shape) or t.shape[0] < shape[0] or tuple(t.shape[1:]) != tuple(shape[1:]):
            raise ValueError(f"{name}: shape {tuple(t.shape)} is not {tuple(shape)} (or more pairs)")
        return t

    def reproject(self, map, q, want_depth=True, want_xyz=False, missing=0.0, z_range=None, want_count=False,
                  depth=None, xyz=None):
        """Metric depth and / or 3-D points of an int32 web map or an int16 sub map (sm_reproject) through the 4 x 4
        matrix q (reprojection_matrix, or any 16 finite numbers) -> those asked for of (depth [pairs][H][W], xyz
        [pairs][H][W][3], kept pixels per pair), one tensor or a tuple in that order.  A pixel that is 0, whose point
        is not finite or whose Z lies outside z_range = (z_min, z_max), both inclusive, receives `missing`.  depth= /
        xyz= are result buffers of the caller's (and ask for that output)."""
        map = self._filter_map(map, "map")
        pairs = map.shape[0]
        want_depth, want_xyz = want_depth or depth is not None, want_xyz or xyz is not None
        depth = self._float_out(depth, (pairs, self.height, self.width), "depth") if want_depth else None
        xyz = self._float_out(xyz, (pairs, self.height, self.width, 3), "xyz") if want_xyz else None
        count = torch.empty(pairs, dtype=torch.int32, device=self._dev) if want_count else None
        lo, hi = self._z_range(z_range)
        check(lib.sm_reproject(self._h, _ptr(map), MAP_TYPES[map.dtype], capi.q16(q), lo, hi, float(missing), pairs,
                               _ptr(depth), _ptr(xyz), _ptr(count), self._stream()))
        res = tuple(t for t in (depth, xyz, count) if t is not None)
        return res[0] if len(res) == 1 else res

    def point_cloud(self, map, q, gray=None, capacity=None, z_range=None, want_index=False, points=None):
        """The kept pixels of a disparity map as a compacted cloud (sm_point_cloud) -> (points, counts) or (points,
        counts, index): points [pairs][capacity][4] float32 records (X, Y, Z, I) in raster order, I the value of the
        uint8 image `gray` at the pixel (0 without one); counts [pairs] int32, the kept pixels of each pair, ALSO where
        that exceeds capacity (records beyond it are dropped; slots from count on are not written); index
        [pairs][capacity] int32, y W + x of each record.  capacity defaults to W H; points= is a buffer of the caller's
        (its second dimension is then the capacity)."""
        map = self._filter_map(map, "map")
        pairs = map.shape[0]
        if gray is not None:
            gray = self._images(gray, torch.uint8, "gray")
            if gray.shape[0] != pairs:
                raise ValueError(f"gray: {gray.shape[0]} images for {pairs} maps")
        if points is not None:
            if points.dim() != 3 or points.shape[2] != 4 or (capacity is not None and points.shape[1] != int(capacity)):
                raise ValueError(f"points: shape {tuple(points.shape)} is not (pairs, capacity, 4)")
            capacity = points.shape[1]
        capacity = self.width * self.height if capacity is None else int(capacity)
        points = self._float_out(points, (pairs, capacity, 4), "points")
        index = torch.empty((pairs, capacity), dtype=torch.int32, device=self._dev) if want_index else None
        counts = torch.empty(pairs, dtype=torch.int32, device=self._dev)
        lo, hi = self._z_range(z_range)
        check(lib.sm_point_cloud(self._h, _ptr(map), MAP_TYPES[map.dtype], capi.q16(q), lo, hi, _ptr(gray), pairs, capacity,
                                 _ptr(points) if capacity else C.c_void_p(0), _ptr(index) if capacity else C.c_void_p(0),
                                 _ptr(counts), self._stream()))
        return (points, counts, index) if want_index else (points, counts)

    def debug_planes(self, pair: int, shift: int):
        """matches-i, score_all-i, scores-i of the reference's debug build."""
        m = torch.empty((self.height, self.width), dtype=torch.uint8, device=self._dev)
        sa = torch.empty((self.height, self.width), dtype=torch.int32, device=self._dev)
        sc = torch.empty_like(sa)
        check(lib.sm_debug_planes(self._h, pair, shift, _ptr(m), _ptr(sa), _ptr(sc), self._stream()))
        return m, sa, sc

    def _poison_workspace(self, word: int):
        """Tests only (sm_debug_poison_workspace): every allocated workspace that is not zero-filled on allocation,
        filled with the 32-bit `word`; synchronises the device.  Not inside a stream capture."""
        check(lib.sm_debug_poison_workspace(self._h, int(word) & 0xFFFFFFFF))

    # ---- step 3 ------------------------------------------------------------
    def fill_web_holes(self, web, times=DEFAULT_TIMES):
        """src/stereo.cu:235-256; returns the buffer the reference would return."""
        web = self._images(web, torch.int32, "web").clone()
        tmp = torch.empty_like(web)
        which = C.c_int(0)
        check(lib.sm_fill_web_holes(self._h, _ptr(web), _ptr(tmp), int(times), web.shape[0],
                                    C.byref(which), self._stream()))
        return tmp if which.value else web

    def image_min_max(self, image):
        image = self._images(image, torch.int32, "image")
        mm = torch.empty((image.shape[0], 2), dtype=torch.int32, device=self._dev)
        check(lib.sm_min_max(self._h, _ptr(image), image.shape[0], _ptr(mm), self._stream()))
        return mm

    def draw_contour_map(self, web, num_lines=DEFAULT_LINES):
        """src/stereo.cu:261-285.  Raises StereoHipError(SM_ERR_ZERO_DIV) where the
        reference would divide by zero."""
        web = self._images(web, torch.int32, "web")
        mm = self.image_min_max(web)
        out = self._new(web.shape[0], torch.uint8)
        check(lib.sm_draw_contour_map(self._h, _ptr(web), _ptr(mm), int(num_lines), web.shape[0],
                                      _ptr(out), self._stream()))
        check(lib.sm_plan_status(self._h, self._stream()))
        return out

    def step3(self, web, times=DEFAULT_TIMES, num_lines=DEFAULT_LINES):
        """fill_web_holes + min/max + draw_contour_map with a single synchronisation
        (sm_step3) -> (hole-filled web, contour image, minmax)."""
        web = self._images(web, torch.int32, "web").clone()
        tmp = torch.empty_like(web)
        pairs = web.shape[0]
        mm = torch.empty((pairs, 2), dtype=torch.int32, device=self._dev)
        out = self._new(pairs, torch.uint8)
        which = C.c_int(0)
        check(lib.sm_step3(self._h, _ptr(web), _ptr(tmp), int(times), int(num_lines), pairs, _ptr(mm),
                           _ptr(out), C.byref(which), self._stream()))
        return (tmp if which.value else web), out, mm

    # ---- the whole of algorithm() --------------------------------------------
    def algorithm(self, first, second, params: AlgorithmParams = AlgorithmParams(), step3=True,
                  lr_max_diff: int | None = None):
        """Stage order of src/stereo.cu:289-347; returns the images the reference dumps
        (minus the per-shift planes: see debug_planes).  lr_max_diff not None: web-1 is the
        left-right checked map (0 where rejected: step 3 fills those pixels), and the result
        adds the right-reference map ("web_right-1") and the rejected pixels per pair
        ("lr_rejected")."""
        if params.square_width != self.square_width:
            raise ValueError("params.square_width differs from the plan's")
        el, er = self.find_all_edges(first, second, params.threshold)
        web1, best = self.match_wta(el.shape[0], want_best=True)
        res = {"edges-1": el, "edges-2": er, "score_best-0": best, "web-1": web1}
        if lr_max_diff is not None:
            web_right, _ = self.match_wta_right(el.shape[0], want_best=False)
            web1, rejected = self.lr_check(web1, web_right, lr_max_diff, out=web1)
            res.update({"web-1": web1, "web_right-1": web_right, "lr_rejected": rejected})
        if step3:
            web2 = self.fill_web_holes(web1, params.times)
            res["web-2"] = web2
            res["output-0"] = self.draw_contour_map(web2, params.lines_to_draw)
        return res


__all__ = ["AlgorithmParams", "LRResult", "StereoPlan", "capi"]
