"""ctypes binding of include/stereo_hip.h (libstereo_hip.so).

This is the only way the Python host side reaches the kernels, and it is the
same C ABI a C caller links against.  There is no fallback: if the library is
missing or does not export a declared symbol, importing fails loudly.
"""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

PKG = Path(__file__).resolve().parent
import os as _os
# diagnostics only (tools/wave_timeline.py loads an instrumented build of the same sources)
LIB_PATH = Path(_os.environ["SM_HIP_LIB"]) if _os.environ.get("SM_HIP_LIB") else PKG / "libstereo_hip.so"
HEADER = PKG.parent / "include" / "stereo_hip.h"

SM_OK, SM_ERR_ARG, SM_ERR_HIP, SM_ERR_NOMEM, SM_ERR_ZERO_DIV = range(5)
SM_TOROIDAL, SM_GHOST = 0, 1
SM_WEB_I32, SM_WEB_U16, SM_WEB_U8 = 0, 1, 2
SM_MAP_I32, SM_MAP_I16 = 0, 1
SM_WMED_FILL = 1
SM_WLS_NO_FILL = 1
SM_REDUCE_BOX, SM_REDUCE_BINOMIAL = 0, 1
SM_UP_FILL = 1
SM_CLASS_VALID, SM_CLASS_OCCLUDED, SM_CLASS_MISMATCHED = 0, 1, 2
SM_RMAP_FRAC_BITS = 5
SM_RMAP_ABS32, SM_RMAP_REL16 = 0, 1
SM_INTERP_BILINEAR, SM_INTERP_NEAREST = 0, 1
RMAP_FORMATS = {"abs32": SM_RMAP_ABS32, "rel16": SM_RMAP_REL16}
INTERPS = {"bilinear": SM_INTERP_BILINEAR, "nearest": SM_INTERP_NEAREST}
BORDERS = {"toroidal": SM_TOROIDAL, "ghost": SM_GHOST}


class StereoHipError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"[sm error {code}] {message}")
        self.code = code
        self.message = message


def declared_symbols() -> list[str]:
    """Every function include/stereo_hip.h declares."""
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(sm_[a-z0-9_]+)\s*\(", text)))


_vp, _int, _sz, _dbl, _flt = C.c_void_p, C.c_int, C.c_size_t, C.c_double, C.c_float
_intp = C.POINTER(C.c_int)
_dblp = C.POINTER(C.c_double)      # a reprojection matrix: an instance of Q16 (or None)
Q16 = C.c_double * 16
_u16p = C.POINTER(C.c_uint16)      # a weight table of the weighted median: an instance of W256 (or None)
W256 = C.c_uint16 * 256

class Geometry(C.Structure):
    """sm_geometry of include/stereo_hip.h"""
    _fields_ = [(n, C.c_int) for n in (
        "kernel", "window", "shifts_per_lane", "shift_lanes", "threads", "tile_w", "tile_h",
        "tiles_x", "tiles_y", "ext_words", "ext_rows", "pad_l", "lds_bytes", "two_wave_variant",
        "edge_rows_per_wave", "waves_per_workgroup", "lane_merge_lds")]


class PlanOptions(C.Structure):
    """sm_plan_options of include/stereo_hip.h (every field 0 = the plan's own choice).  cost_pixels_per_lane
    and the four priority_* fields have no effect; they are kept for the struct layout."""
    _fields_ = [("struct_size", C.c_int), ("kernel_family", C.c_int), ("tile_h", C.c_int),
                ("shifts_per_lane", C.c_int), ("workgroup_waves", C.c_int), ("no_two_wave_cap", C.c_int),
                ("priority_pattern", C.c_uint), ("edge_kernel", C.c_int), ("timing_by_records", C.c_int),
                ("cost_pixels_per_lane", C.c_int), ("cost_tile_h", C.c_int), ("cost_kernel", C.c_int),
                ("priority_class", C.c_int), ("priority_on_change", C.c_int), ("lane_merge", C.c_int),
                ("no_four_shift_lanes", C.c_int), ("priority_unit_log2", C.c_int), ("cost_workgroup_waves", C.c_int)]

    @classmethod
    def make(cls, **kw):
        o = cls(**kw)
        o.struct_size = C.sizeof(cls)
        return o


class RectifyCalib(C.Structure):
    """sm_rectify_calib of include/stereo_hip.h: one side's camera matrix, distortion (k1, k2, p1, p2, k3), rectifying
    rotation R (row-major) and the projection of the rectified image"""
    _fields_ = [("struct_size", C.c_int), ("reserved", C.c_int)] + \
               [(n, C.c_double) for n in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")] + \
               [("R", C.c_double * 3 * 3)] + [(n, C.c_double) for n in ("new_fx", "new_fy", "new_cx", "new_cy")]

    @classmethod
    def make(cls, fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0, R=None, new_fx=None, new_fy=None,
             new_cx=None, new_cy=None):
        """R: None (identity) or 3 x 3 numbers; the new projection defaults to the camera matrix"""
        o = cls(fx=fx, fy=fy, cx=cx, cy=cy, k1=k1, k2=k2, p1=p1, p2=p2, k3=k3,
                new_fx=fx if new_fx is None else new_fx, new_fy=fy if new_fy is None else new_fy,
                new_cx=cx if new_cx is None else new_cx, new_cy=cy if new_cy is None else new_cy)
        rows = ((1, 0, 0), (0, 1, 0), (0, 0, 1)) if R is None else R
        for i in range(3):
            for j in range(3):
                o.R[i][j] = float(rows[i][j])
        o.struct_size = C.sizeof(cls)
        return o


_SIGNATURES = {
    "sm_last_error": (C.c_char_p, []),
    "sm_device_count": (_int, [_intp]),
    "sm_malloc": (_int, [_int, _sz, C.POINTER(_vp)]),
    "sm_free": (_int, [_int, _vp]),
    "sm_memcpy_h2d": (_int, [_int, _vp, _vp, _sz]),
    "sm_memcpy_d2h": (_int, [_int, _vp, _vp, _sz]),
    "sm_stream_sync": (_int, [_int, _vp]),
    "sm_host_alloc": (_int, [_sz, C.POINTER(_vp)]),
    "sm_host_free": (_int, [_vp]),
    "sm_memcpy_h2d_async": (_int, [_int, _vp, _vp, _sz, _vp]),
    "sm_memcpy_d2h_async": (_int, [_int, _vp, _vp, _sz, _vp]),
    "sm_stream_create": (_int, [_int, C.POINTER(_vp)]),
    "sm_stream_destroy": (_int, [_int, _vp]),
    "sm_event_create": (_int, [_int, C.POINTER(_vp)]),
    "sm_event_destroy": (_int, [_int, _vp]),
    "sm_event_record": (_int, [_int, _vp, _vp]),
    "sm_stream_wait_event": (_int, [_int, _vp, _vp]),
    "sm_event_sync": (_int, [_int, _vp]),
    "sm_comm_set_rccl_library": (_int, [C.c_char_p]),
    "sm_comm_create": (_int, [_intp, _int, C.POINTER(_vp)]),
    "sm_comm_destroy": (None, [_vp]),
    "sm_comm_size": (_int, [_vp]),
    "sm_broadcast": (_int, [_vp, C.POINTER(_vp), _sz, C.POINTER(_vp)]),
    "sm_gather_maps": (_int, [_vp, C.POINTER(_vp), C.POINTER(_sz), _vp, C.POINTER(_vp)]),
    "sm_plan_create": (_int, [_int, _int, _int, _int, _int, _int, _int, C.POINTER(_vp)]),
    "sm_plan_create_ex": (_int, [_int, _int, _int, _int, _int, _int, _int, C.POINTER(PlanOptions), C.POINTER(_vp)]),
    "sm_plan_destroy": (None, [_vp]),
    "sm_plan_describe": (C.c_char_p, [_vp]),
    "sm_plan_workspace_bytes": (_sz, [_vp]),
    "sm_plan_reserve_narrow": (_int, [_vp]),
    "sm_plan_geometry": (_int, [_vp, C.POINTER(Geometry)]),
    "sm_plan_geometry_sized": (_int, [_vp, C.POINTER(Geometry), _sz]),
    "sm_find_edges": (_int, [_vp, _vp, _vp, _dbl, _int, _vp, _vp, _vp]),
    "sm_load_edges": (_int, [_vp, _vp, _vp, _int, _vp]),
    "sm_match_wta": (_int, [_vp, _int, _vp, _vp, _vp]),
    "sm_match_wta_typed": (_int, [_vp, _int, _vp, _int, _vp, _vp]),
    "sm_run_typed": (_int, [_vp, _vp, _vp, _dbl, _int, _vp, _int, _vp, _vp]),
    "sm_run_after": (_int, [_vp, _vp, _vp, _dbl, _int, _vp, _int, _vp, _vp, _vp]),
    "sm_plan_set_pipelined": (_int, [_vp, _int]),
    "sm_plan_prepare_threshold": (_int, [_vp, C.c_double, _vp]),
    "sm_plan_time_kernels": (_int, [_vp, _int]),
    "sm_plan_time_stride": (_int, [_vp, _int]),
    "sm_plan_kernel_ms": (_int, [_vp, C.POINTER(C.c_double), _intp]),
    "sm_run": (_int, [_vp, _vp, _vp, _dbl, _int, _vp, _vp, _vp]),
    "sm_cost_wta": (_int, [_vp, _vp, _vp, _int, _int, _vp, _vp, _vp]),
    "sm_debug_planes": (_int, [_vp, _int, _int, _vp, _vp, _vp, _vp]),
    "sm_debug_edge_table": (_int, [_int, _dbl, _vp, _vp]),
    "sm_debug_edge_table_fast": (_int, [_vp, _dbl, _vp, _intp, _vp]),
    "sm_debug_poison_workspace": (_int, [_vp, C.c_uint32]),
    "sm_fill_web_holes": (_int, [_vp, _vp, _vp, _int, _int, _intp, _vp]),
    "sm_min_max": (_int, [_vp, _vp, _int, _vp, _vp]),
    "sm_draw_contour_map": (_int, [_vp, _vp, _vp, _int, _int, _vp, _vp]),
    "sm_plan_status": (_int, [_vp, _vp]),
    "sm_step3": (_int, [_vp, _vp, _vp, _int, _int, _int, _vp, _vp, _intp, _vp]),
    "sm_match_wta_right": (_int, [_vp, _int, _vp, _vp, _vp]),
    "sm_lr_check": (_int, [_vp, _vp, _vp, _int, _int, _vp, _vp, _vp]),
    "sm_run_lr": (_int, [_vp, _vp, _vp, _dbl, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    "sm_plan_reserve_lr": (_int, [_vp]),
    "sm_cost_refine": (_int, [_vp, _vp, _vp, _int, _int, _vp, _vp, _vp, _vp]),
    "sm_cost_wta_right": (_int, [_vp, _vp, _vp, _int, _int, _vp, _vp, _vp]),
    "sm_cost_lr": (_int, [_vp, _vp, _vp, _int, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    "sm_plan_reserve_cost_lr": (_int, [_vp]),
    "sm_census_transform": (_int, [_vp, _vp, _int, _int, _vp, _vp]),
    "sm_census_wta": (_int, [_vp, _vp, _vp, _int, _int, _vp, _vp, _vp]),
    "sm_census_wta_right": (_int, [_vp, _vp, _vp, _int, _int, _vp, _vp, _vp]),
    "sm_census_lr": (_int, [_vp, _vp, _vp, _int, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    "sm_census_refine": (_int, [_vp, _vp, _vp, _int, _int, _vp, _vp, _vp, _vp]),
    "sm_plan_reserve_census": (_int, [_vp]),
    "sm_census_wta_near": (_int, [_vp, _vp, _vp, _int, _int, _vp, _int, _vp, _vp, _vp]),
    "sm_census_wta_near_right": (_int, [_vp, _vp, _vp, _int, _int, _vp, _int, _vp, _vp, _vp]),
    "sm_census_near_lr": (_int, [_vp, _vp, _vp, _int, _int, _vp, _vp, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    "sm_sgm_wta": (_int, [_vp, _vp, _vp, _int, _int, _int, _int, _int, _vp, _vp, _vp, _vp]),
    "sm_sgm_wta_right": (_int, [_vp, _vp, _vp, _int, _int, _int, _int, _int, _vp, _vp, _vp]),
    "sm_sgm_lr": (_int, [_vp, _vp, _vp, _int, _int, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sm_plan_reserve_sgm": (_int, [_vp]),
    "sm_sgm_wta_both": (_int, [_vp, _vp, _vp, _int, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sm_sgm_lr_single": (_int, [_vp, _vp, _vp, _int, _int, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sm_sgm_wta_near": (_int, [_vp, _vp, _vp, _int, _int, _int, _int, _int, _vp, _int, _vp, _vp, _vp, _vp]),
    "sm_sgm_wta_near_right": (_int, [_vp, _vp, _vp, _int, _int, _int, _int, _int, _vp, _int, _vp, _vp, _vp]),
    "sm_sgm_near_lr": (_int, [_vp, _vp, _vp, _int, _int, _int, _int, _int, _vp, _vp, _int, _int, _vp, _vp, _vp, _vp,
                              _vp, _vp]),
    "sm_plan_reserve_sgm_near": (_int, [_vp]),
    "sm_census_second": (_int, [_vp, _vp, _vp, _int, _int, _vp, _vp, _vp, _vp]),
    "sm_sgm_wta2": (_int, [_vp, _vp, _vp, _int, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sm_uniqueness_filter": (_int, [_vp, _vp, _vp, _vp, _int, _int, _vp, _vp, _vp]),
    "sm_confidence": (_int, [_vp, _vp, _vp, _vp, _int, _vp, _vp]),
    "sm_median_filter": (_int, [_vp, _vp, _int, _int, _int, _vp, _vp]),
    "sm_speckle_filter": (_int, [_vp, _vp, _int, _int, _int, _int, _vp, _vp, _vp]),
    "sm_sub_mask": (_int, [_vp, _vp, _vp, _int, _vp]),
    "sm_plan_reserve_filter": (_int, [_vp]),
    "sm_weighted_median": (_int, [_vp, _vp, _int, _vp, _int, _u16p, _int, _int, _int, _vp, _vp, _vp]),
    "sm_wls_filter": (_int, [_vp, _vp, _int, _vp, _vp, _u16p, _dbl, _int, _int, _int, _vp, _int, _vp, _vp, _vp]),
    "sm_plan_reserve_wls": (_int, [_vp]),
    "sm_cross_arms": (_int, [_vp, _vp, _int, _int, _int, _vp, _vp, _vp]),
    "sm_cross_wta": (_int, [_vp, _vp, _vp, _int, _int, _int, _int, _vp, _vp, _vp, _vp]),
    "sm_cross_wta_right": (_int, [_vp, _vp, _vp, _int, _int, _int, _int, _vp, _vp, _vp]),
    "sm_cross_lr": (_int, [_vp, _vp, _vp, _int, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sm_plan_reserve_cross": (_int, [_vp]),
    "sm_reduce_half": (_int, [_vp, _vp, _int, _int, _vp, _vp]),
    "sm_upsample_double": (_int, [_vp, _vp, _int, _vp, _vp, _u16p, _int, _int, _vp, _vp]),
    "sm_occlusion_classify": (_int, [_vp, _vp, _vp, _int, _vp, _vp]),
    "sm_interpolate": (_int, [_vp, _vp, _int, _vp, _int, _vp, _vp, _vp]),
    "sm_plan_reserve_interp": (_int, [_vp]),
    "sm_rectify": (_int, [_vp, _vp, _vp, _int, _int, _vp, _vp, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    "sm_rectify_map_build": (_int, [_vp, C.POINTER(RectifyCalib), _int, _vp, _vp]),
    "sm_valid_mask": (_int, [_vp, _vp, _int, _vp, _int, _vp]),
    "sm_reproject": (_int, [_vp, _vp, _int, _dblp, _flt, _flt, _flt, _int, _vp, _vp, _vp, _vp]),
    "sm_point_cloud": (_int, [_vp, _vp, _int, _dblp, _flt, _flt, _vp, _int, _int, _vp, _vp, _vp, _vp]),
    "sm_plan_reserve_cloud": (_int, [_vp]),
    "sm_reproject_q": (_int, [C.POINTER(RectifyCalib), C.POINTER(RectifyCalib), _dbl, _dblp]),
}


def q16(q) -> "Q16":
    """A reprojection matrix as the c_double * 16 the C ABI takes: 16 numbers, or 4 rows of 4 (lists, numpy, torch)"""
    if isinstance(q, Q16):
        return q
    q = q.tolist() if hasattr(q, "tolist") else list(q)
    flat = [v for row in q for v in (row.tolist() if hasattr(row, "tolist") else row)] if len(q) == 4 else q
    if len(flat) != 16:
        raise ValueError(f"q: need 16 numbers (or 4 rows of 4), got {len(flat)}")
    return Q16(*(float(v) for v in flat))


def w256(weights) -> "W256":
    """A weight table as the c_uint16 * 256 the C ABI takes: 256 integers in 0 .. 65535 (a list, numpy, torch)"""
    if isinstance(weights, W256):
        return weights
    flat = weights.tolist() if hasattr(weights, "tolist") else list(weights)
    if len(flat) != 256 or any(isinstance(v, (list, tuple)) for v in flat):
        raise ValueError(f"weights: need 256 numbers, got {len(flat)}")
    if any(int(v) != v or not 0 <= v <= 65535 for v in flat):
        raise ValueError("weights: need integers in 0 .. 65535")
    return W256(*(int(v) for v in flat))


def _load() -> C.CDLL:
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension has not been built. Run "
            "`python -m stereomatching_amd.build` (needs hipcc; cross-compiles for gfx950 "
            "without a GPU). There is no CPU fallback.")
    lib = C.CDLL(str(LIB_PATH))
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    if missing:
        raise ImportError(f"{LIB_PATH} does not export {missing} declared in {HEADER}")
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def check(rc: int) -> None:
    if rc != SM_OK:
        raise StereoHipError(rc, lib.sm_last_error().decode(errors="replace"))
