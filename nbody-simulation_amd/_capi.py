"""ctypes binding of include/nbody_hip.h (libnbody_hip.so).  Plain pointers and sizes only.

Loading never touches the GPU; `load()` raises if the library has not been built.  Nothing here falls back to
a CPU implementation: compute calls need a context, and `create_context` raises NBodyError when no gfx950
device is present (NBODY_ERR_NO_DEVICE).
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libnbody_hip.so")
LAB_LIB_PATH = os.path.join(_HERE, "lib", "libnbody_hip_lab.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "nbody_hip.h")

ABI_VERSION = 3   # NBODY_ABI_VERSION of include/nbody_hip.h (tests/test_capi_host.py checks the two agree)
DELTAS_TRACERS, DELTAS_KEY = 1, 2   # NBODY_DELTAS_* of include/nbody_ensemble.h: the flags of nbody_deltas_<handle>
SUMMARY_TRACERS = 1                 # NBODY_SUMMARY_TRACERS: the flag of nbody_summary_<handle>
# nbody_world_summary of include/nbody_ensemble.h: 17 fields of 8 bytes, no padding
SUMMARY_DTYPE = np.dtype([(name, np.int64) for name in ("rows", "counted", "in_bounds", "sep_rows")] +
                         [(name, np.float64) for name in ("mass", "min_x", "min_y", "max_x", "max_y", "max_speed2", "sum_wx", "sum_wy",
                                                          "sum_wvx", "sum_wvy", "sum_wv2", "sep_max2", "sep_sum2")])
ENCOUNTERS_TRACERS = 1              # NBODY_ENCOUNTERS_TRACERS: the flag of nbody_encounters_<handle>
# nbody_world_encounters of include/nbody_ensemble.h: 12 fields of 8 bytes, no padding
ENCOUNTERS_DTYPE = np.dtype([(name, np.int64) for name in ("rows", "sources", "live_pairs", "skipped_pairs", "close_pairs", "close_rows",
                                                           "isolated_rows", "min_row", "min_source")] +
                            [("min_d2", np.float64), ("max_nn_row", np.int64), ("max_nn_d2", np.float64)])
WATCH_TRACERS, WATCH_RESUME = 1, 2   # NBODY_WATCH_*: the flags of nbody_watch_<handle>
WATCH_NEVER = 0xffffffff             # NBODY_WATCH_NEVER: a sample number that did not occur
# nbody_world_watch of include/nbody_ensemble.h: 13 fields of 8 bytes, no padding
WATCH_DTYPE = np.dtype([(name, np.int64) for name in ("rows", "sources", "samples", "min_row", "min_source", "min_sample")] +
                       [("min_d2", np.float64)] +
                       [(name, np.int64) for name in ("close_rows", "close_row_samples", "first_close_sample", "out_rows",
                                                      "first_out_sample", "isolated_rows")])
WATCH_ROWS = ("min_d2", "min_index", "min_sample", "first_close", "close_samples", "first_out")   # nbody_watch_rows_*, in order
OK, ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_DEGENERATE, ERR_NOMEM = 0, -1, -2, -3, -4, -5
ARITH_AUTO, ARITH_FAST, ARITH_EXACT = 0, 1, 2
ORDER_AS_WRITTEN, ORDER_CONSISTENT = 0, 1
TREE_BVH, TREE_QUAD = 0, 1
EXCHANGE_RCCL, EXCHANGE_PEER = 0, 1


class NBodyError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"nbody_hip error {code}: {msg}")
        self.code = code


class Counting(C.Structure):
    """`struct Counting` (main.rs:74-79)."""
    _fields_ = [("build_bvh", C.c_double), ("sum_gravity", C.c_double), ("post_calculations", C.c_double)]


class Params(C.Structure):
    _fields_ = [("theta", C.c_float), ("clamp", C.c_float), ("leaf_size", C.c_int32), ("order", C.c_int32),
                ("arith", C.c_int32), ("quad_root_x", C.c_float), ("quad_root_y", C.c_float),
                ("quad_root_h", C.c_float)]


class WatchRows(C.Structure):
    """`nbody_watch_rows_f32` / `_f64`: six pointers, the first to the handle's precision; each may be NULL."""
    _fields_ = [(name, C.c_void_p) for name in ("min_d2", "min_index", "min_sample", "first_close", "close_samples", "first_out")]


class TreeView(C.Structure):
    _fields_ = [("n_nodes", C.c_int64), ("kind", C.c_int32), ("max_depth", C.c_int32)]


_lib = None
_vp, _i64, _i32, _f32, _f64, _sz = C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_double, C.c_size_t

_SIGS = {
    "nbody_abi_version": (C.c_int, []),
    "nbody_create": (C.c_int, [C.POINTER(_vp), _i32]),
    "nbody_create_multi": (C.c_int, [C.POINTER(_vp), _i32, _vp]),
    "nbody_create_multi_ex": (C.c_int, [C.POINTER(_vp), _i32, _vp, _i32, _i32]),
    "nbody_multi_info": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_i64)]),
    "nbody_multi_comm_count": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "nbody_get_stream": (_vp, [_vp]),
    "nbody_direct_prep_dev": (C.c_int, [_vp, _i64, _vp, _vp, _f32, _i64, _i64, _f32, _i32, _vp, _sz]),
    "nbody_direct_run_dev": (C.c_int, [_vp, _i64, _vp, _vp, _f32, _i64, _i64, _vp, _vp, _vp, _f32, _f32, _i32, _i64, _i64, _vp, _sz, _vp]),
    "nbody_destroy": (None, [_vp]),
    "nbody_last_error": (C.c_char_p, [_vp]),
    "nbody_default_params": (C.c_int, [C.POINTER(Params)]),
    "nbody_set_params": (C.c_int, [_vp, C.POINTER(Params)]),
    "nbody_get_params": (C.c_int, [_vp, C.POINTER(Params)]),
    "nbody_upload_f32": (C.c_int, [_vp, _i64, _vp, _vp, _vp]),
    "nbody_upload_f64": (C.c_int, [_vp, _i64, _vp, _vp, _vp]),
    "nbody_download_f32": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "nbody_download_f64": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "nbody_num_particles": (_i64, [_vp]),
    "nbody_update_direct_f32": (C.c_int, [_vp, _f32, _i32, C.POINTER(Counting)]),
    "nbody_update_direct_f64": (C.c_int, [_vp, _f64, _i32, C.POINTER(Counting)]),
    "nbody_update_tree_f32": (C.c_int, [_vp, _i32, _f32, _i32, C.POINTER(Counting)]),
    "nbody_update_tree_f64": (C.c_int, [_vp, _i32, _f64, _i32, C.POINTER(Counting)]),
    "nbody_update_tree_async_f32": (C.c_int, [_vp, _i32, _f32, _i32]),
    "nbody_wait": (C.c_int, [_vp]),
    "nbody_update_tree_shard_f32": (C.c_int, [_vp, _i32, _f32, _i64, _i64, C.POINTER(Counting)]),
    "nbody_update_tree_shard_f64": (C.c_int, [_vp, _i32, _f64, _i64, _i64, C.POINTER(Counting)]),
    "nbody_export_slice_dev": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _vp]),
    "nbody_import_rows_dev": (C.c_int, [_vp, _i64, _vp, _vp, _vp]),
    "nbody_accel_direct_f32": (C.c_int, [_vp, _vp]),
    "nbody_accel_direct_f64": (C.c_int, [_vp, _vp]),
    "nbody_accel_direct_at_f32": (C.c_int, [_vp, _i64, _vp, _vp]),
    "nbody_accel_direct_at_f64": (C.c_int, [_vp, _i64, _vp, _vp]),
    "nbody_tracers_upload_f32": (C.c_int, [_vp, _i64, _vp, _vp]),
    "nbody_tracers_upload_f64": (C.c_int, [_vp, _i64, _vp, _vp]),
    "nbody_tracers_download_f32": (C.c_int, [_vp, _vp, _vp]),
    "nbody_tracers_download_f64": (C.c_int, [_vp, _vp, _vp]),
    "nbody_num_tracers": (_i64, [_vp]),
    "nbody_ensemble_create": (C.c_int, [C.POINTER(_vp), _i32]),
    "nbody_ensemble_destroy": (None, [_vp]),
    "nbody_ensemble_last_error": (C.c_char_p, [_vp]),
    "nbody_ensemble_set_params": (C.c_int, [_vp, C.POINTER(Params)]),
    "nbody_ensemble_get_params": (C.c_int, [_vp, C.POINTER(Params)]),
    "nbody_ensemble_upload_f32": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _vp]),
    "nbody_ensemble_download_f32": (C.c_int, [_vp, _vp, _vp]),
    "nbody_ensemble_num_worlds": (_i64, [_vp]),
    "nbody_ensemble_num_bodies": (_i64, [_vp]),
    "nbody_ensemble_update_f32": (C.c_int, [_vp, _f32, _i32, C.POINTER(Counting)]),
    "nbody_ensemble_accel_f32": (C.c_int, [_vp, _vp]),
    "nbody_ensemble64_create": (C.c_int, [C.POINTER(_vp), _i32]),
    "nbody_ensemble64_destroy": (None, [_vp]),
    "nbody_ensemble64_last_error": (C.c_char_p, [_vp]),
    "nbody_ensemble64_set_params": (C.c_int, [_vp, C.POINTER(Params)]),
    "nbody_ensemble64_get_params": (C.c_int, [_vp, C.POINTER(Params)]),
    "nbody_ensemble64_upload": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _vp]),
    "nbody_ensemble64_download": (C.c_int, [_vp, _vp, _vp]),
    "nbody_ensemble64_num_worlds": (_i64, [_vp]),
    "nbody_ensemble64_num_bodies": (_i64, [_vp]),
    "nbody_ensemble64_update": (C.c_int, [_vp, _f64, _i32, C.POINTER(Counting)]),
    "nbody_ensemble64_accel": (C.c_int, [_vp, _vp]),
    "nbody_ragged_create": (C.c_int, [C.POINTER(_vp), _i32]),
    "nbody_ragged_destroy": (None, [_vp]),
    "nbody_ragged_last_error": (C.c_char_p, [_vp]),
    "nbody_ragged_set_params": (C.c_int, [_vp, C.POINTER(Params)]),
    "nbody_ragged_get_params": (C.c_int, [_vp, C.POINTER(Params)]),
    "nbody_ragged_upload_f32": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp]),
    "nbody_ragged_download_f32": (C.c_int, [_vp, _vp, _vp]),
    "nbody_ragged_num_worlds": (_i64, [_vp]),
    "nbody_ragged_num_rows": (_i64, [_vp]),
    "nbody_ragged_sizes": (C.c_int, [_vp, _vp]),
    "nbody_ragged_update_f32": (C.c_int, [_vp, _f32, _i32, C.POINTER(Counting)]),
    "nbody_ragged_accel_f32": (C.c_int, [_vp, _vp]),
    "nbody_ragged_plan": (C.c_int, [_i64, _vp, _vp, _vp, C.POINTER(_i32), _vp, _vp]),
    "nbody_ragged64_create": (C.c_int, [C.POINTER(_vp), _i32]),
    "nbody_ragged64_destroy": (None, [_vp]),
    "nbody_ragged64_last_error": (C.c_char_p, [_vp]),
    "nbody_ragged64_set_params": (C.c_int, [_vp, C.POINTER(Params)]),
    "nbody_ragged64_get_params": (C.c_int, [_vp, C.POINTER(Params)]),
    "nbody_ragged64_upload": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp]),
    "nbody_ragged64_download": (C.c_int, [_vp, _vp, _vp]),
    "nbody_ragged64_num_worlds": (_i64, [_vp]),
    "nbody_ragged64_num_rows": (_i64, [_vp]),
    "nbody_ragged64_sizes": (C.c_int, [_vp, _vp]),
    "nbody_ragged64_update": (C.c_int, [_vp, _f64, _i32, C.POINTER(Counting)]),
    "nbody_ragged64_accel": (C.c_int, [_vp, _vp]),
    "nbody_ragged64_plan": (C.c_int, [_i64, _vp, _vp, _vp, C.POINTER(_i32), _vp, _vp]),
    "nbody_restricted_create": (C.c_int, [C.POINTER(_vp), _i32]),
    "nbody_restricted_destroy": (None, [_vp]),
    "nbody_restricted_last_error": (C.c_char_p, [_vp]),
    "nbody_restricted_set_params": (C.c_int, [_vp, C.POINTER(Params)]),
    "nbody_restricted_get_params": (C.c_int, [_vp, C.POINTER(Params)]),
    "nbody_restricted_upload_f32": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _vp]),
    "nbody_restricted_download_f32": (C.c_int, [_vp, _vp, _vp]),
    "nbody_restricted_tracers_upload_f32": (C.c_int, [_vp, _i64, _i64, _vp, _vp]),
    "nbody_restricted_tracers_download_f32": (C.c_int, [_vp, _vp, _vp]),
    "nbody_restricted_num_worlds": (_i64, [_vp]),
    "nbody_restricted_num_bodies": (_i64, [_vp]),
    "nbody_restricted_num_tracers": (_i64, [_vp]),
    "nbody_restricted_update_f32": (C.c_int, [_vp, _f32, _i32, C.POINTER(Counting)]),
    "nbody_restricted_accel_f32": (C.c_int, [_vp, _vp]),
    "nbody_restricted_tracers_accel_f32": (C.c_int, [_vp, _vp]),
    "nbody_restricted64_create": (C.c_int, [C.POINTER(_vp), _i32]),
    "nbody_restricted64_destroy": (None, [_vp]),
    "nbody_restricted64_last_error": (C.c_char_p, [_vp]),
    "nbody_restricted64_set_params": (C.c_int, [_vp, C.POINTER(Params)]),
    "nbody_restricted64_get_params": (C.c_int, [_vp, C.POINTER(Params)]),
    "nbody_restricted64_upload": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _vp]),
    "nbody_restricted64_download": (C.c_int, [_vp, _vp, _vp]),
    "nbody_restricted64_tracers_upload": (C.c_int, [_vp, _i64, _i64, _vp, _vp]),
    "nbody_restricted64_tracers_download": (C.c_int, [_vp, _vp, _vp]),
    "nbody_restricted64_num_worlds": (_i64, [_vp]),
    "nbody_restricted64_num_bodies": (_i64, [_vp]),
    "nbody_restricted64_num_tracers": (_i64, [_vp]),
    "nbody_restricted64_update": (C.c_int, [_vp, _f64, _i32, C.POINTER(Counting)]),
    "nbody_restricted64_accel": (C.c_int, [_vp, _vp]),
    "nbody_restricted64_tracers_accel": (C.c_int, [_vp, _vp]),
    "nbody_rr_create": (C.c_int, [C.POINTER(_vp), _i32]),
    "nbody_rr_destroy": (None, [_vp]),
    "nbody_rr_last_error": (C.c_char_p, [_vp]),
    "nbody_rr_set_params": (C.c_int, [_vp, C.POINTER(Params)]),
    "nbody_rr_get_params": (C.c_int, [_vp, C.POINTER(Params)]),
    "nbody_rr_upload_f32": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp]),
    "nbody_rr_download_f32": (C.c_int, [_vp, _vp, _vp]),
    "nbody_rr_tracers_upload_f32": (C.c_int, [_vp, _i64, _vp, _vp, _vp]),
    "nbody_rr_tracers_download_f32": (C.c_int, [_vp, _vp, _vp]),
    "nbody_rr_num_worlds": (_i64, [_vp]),
    "nbody_rr_num_rows": (_i64, [_vp]),
    "nbody_rr_num_tracer_rows": (_i64, [_vp]),
    "nbody_rr_sizes": (C.c_int, [_vp, _vp, _vp]),
    "nbody_rr_update_f32": (C.c_int, [_vp, _f32, _i32, C.POINTER(Counting)]),
    "nbody_rr_accel_f32": (C.c_int, [_vp, _vp]),
    "nbody_rr_tracers_accel_f32": (C.c_int, [_vp, _vp]),
    "nbody_rr_plan": (C.c_int, [_i64, _vp, _vp, _vp, _vp, C.POINTER(_i32), _vp, _vp]),
    "nbody_rr64_create": (C.c_int, [C.POINTER(_vp), _i32]),
    "nbody_rr64_destroy": (None, [_vp]),
    "nbody_rr64_last_error": (C.c_char_p, [_vp]),
    "nbody_rr64_set_params": (C.c_int, [_vp, C.POINTER(Params)]),
    "nbody_rr64_get_params": (C.c_int, [_vp, C.POINTER(Params)]),
    "nbody_rr64_upload": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp]),
    "nbody_rr64_download": (C.c_int, [_vp, _vp, _vp]),
    "nbody_rr64_tracers_upload": (C.c_int, [_vp, _i64, _vp, _vp, _vp]),
    "nbody_rr64_tracers_download": (C.c_int, [_vp, _vp, _vp]),
    "nbody_rr64_num_worlds": (_i64, [_vp]),
    "nbody_rr64_num_rows": (_i64, [_vp]),
    "nbody_rr64_num_tracer_rows": (_i64, [_vp]),
    "nbody_rr64_sizes": (C.c_int, [_vp, _vp, _vp]),
    "nbody_rr64_update": (C.c_int, [_vp, _f64, _i32, C.POINTER(Counting)]),
    "nbody_rr64_accel": (C.c_int, [_vp, _vp]),
    "nbody_rr64_tracers_accel": (C.c_int, [_vp, _vp]),
    "nbody_rr64_plan": (C.c_int, [_i64, _vp, _vp, _vp, _vp, C.POINTER(_i32), _vp, _vp]),
    "nbody_frames_ensemble": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp]),
    "nbody_frames_ensemble64": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp]),
    "nbody_frames_ragged": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp]),
    "nbody_frames_ragged64": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp]),
    "nbody_frames_restricted": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_int, _vp]),
    "nbody_frames_restricted64": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_int, _vp]),
    "nbody_frames_rr": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_int, _vp]),
    "nbody_frames_rr64": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_int, _vp]),
    **{"nbody_deltas_" + h: (C.c_int, [_vp, C.c_uint32, _vp, _sz, C.POINTER(_sz), _vp, C.POINTER(C.c_uint64)])
       for h in ("ensemble", "ensemble64", "ragged", "ragged64", "restricted", "restricted64", "rr", "rr64")},
    "nbody_deltas_bound": (_sz, [_i64, _vp, C.c_int]),
    # nbody_sweep_<handle>: delta[n_worlds] in the handle's precision, clamp[n_worlds] float on all eight, steps[n_worlds] int32
    **{"nbody_sweep_" + h: (C.c_int, [_vp, C.POINTER(_f64 if h.endswith("64") else _f32), C.POINTER(_f32), C.POINTER(C.c_int32), _i32,
                                      C.POINTER(Counting)])
       for h in ("ensemble", "ensemble64", "ragged", "ragged64", "restricted", "restricted64", "rr", "rr64")},
    # nbody_summary_<handle>: flags, height, ref int32[n_worlds] or NULL, out nbody_world_summary[n_worlds] (SUMMARY_DTYPE)
    **{"nbody_summary_" + h: (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), _vp])
       for h in ("ensemble", "ensemble64", "ragged", "ragged64", "restricted", "restricted64", "rr", "rr64")},
    "nbody_summary_of_f32": (C.c_int, [_i64, _vp, _vp, _vp, _vp, _vp, C.c_uint32, _vp]),
    "nbody_summary_of_f64": (C.c_int, [_i64, _vp, _vp, _vp, _vp, _vp, C.c_uint32, _vp]),
    # nbody_encounters_<handle>: flags, limit2 float32[n_worlds] or NULL, out nbody_world_encounters[n_worlds] (ENCOUNTERS_DTYPE),
    # nn_index int32[rows], nn_d2 [rows] of the handle's dtype, close uint32[rows], each or NULL
    **{"nbody_encounters_" + h: (C.c_int, [_vp, C.c_uint32, C.POINTER(_f32), _vp, _vp, _vp, _vp])
       for h in ("ensemble", "ensemble64", "ragged", "ragged64", "restricted", "restricted64", "rr", "rr64")},
    "nbody_encounters_of_f32": (C.c_int, [_i64, _vp, _i64, _vp, _i32, _f32, _vp, _vp, _vp, _vp]),
    "nbody_encounters_of_f64": (C.c_int, [_i64, _vp, _i64, _vp, _i32, _f64, _vp, _vp, _vp, _vp]),
    # nbody_watch_<handle>: flags, delta in the handle's precision, n_steps, stride, limit2 float32[n_worlds] or NULL, height,
    # out nbody_world_watch[n_worlds] (WATCH_DTYPE), rows nbody_watch_rows_* (WatchRows) or NULL, counter
    **{"nbody_watch_" + h: (C.c_int, [_vp, C.c_uint32, _f64 if h.endswith("64") else _f32, _i32, _i32, C.POINTER(_f32), C.c_uint32, _vp,
                                      C.POINTER(WatchRows), C.POINTER(Counting)])
       for h in ("ensemble", "ensemble64", "ragged", "ragged64", "restricted", "restricted64", "rr", "rr64")},
    # nbody_wsweep_<handle>: flags, then a sweep's delta, clamp, steps, n_steps, then stride int32[n_worlds] or NULL, limit2
    # float32[n_worlds] or NULL, and a watch's height, out, rows, counter
    **{"nbody_wsweep_" + h: (C.c_int, [_vp, C.c_uint32, C.POINTER(_f64 if h.endswith("64") else _f32), C.POINTER(_f32), C.POINTER(C.c_int32),
                                       _i32, C.POINTER(C.c_int32), C.POINTER(_f32), C.c_uint32, _vp, C.POINTER(WatchRows),
                                       C.POINTER(Counting)])
       for h in ("ensemble", "ensemble64", "ragged", "ragged64", "restricted", "restricted64", "rr", "rr64")},
    "nbody_wsweep_plan": (C.c_int, [_i64, C.POINTER(C.c_int32), _i32, C.POINTER(C.c_int32), C.c_uint32, _vp, _vp]),
    # nbody_resident_<handle>: a sweep's arguments, on the four handles without tracers
    **{"nbody_resident_" + h: (C.c_int, [_vp, C.POINTER(_f64 if h.endswith("64") else _f32), C.POINTER(_f32), C.POINTER(C.c_int32), _i32,
                                         C.POINTER(Counting)])
       for h in ("ensemble", "ensemble64", "ragged", "ragged64")},
    "nbody_resident_plan": (C.c_int, [_i64, C.POINTER(_i64), C.POINTER(C.c_int32), _i32, _i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "nbody_accel_tree_f32": (C.c_int, [_vp, _i32, _i64, _vp, _vp]),
    "nbody_accel_tree_f64": (C.c_int, [_vp, _i32, _i64, _vp, _vp]),
    "nbody_tree_info": (C.c_int, [_vp, C.POINTER(TreeView)]),
    "nbody_walk_tree_f32": (C.c_int, [_vp, _i32, _i64] + [_vp] * 7 + [_i64, _vp, _vp]),
    "nbody_walk_tree_f64": (C.c_int, [_vp, _i32, _i64] + [_vp] * 7 + [_i64, _vp, _vp]),
    "nbody_tree_validate": (C.c_int, [_i32, _i64] + [_vp] * 4 + [_i64, _vp, C.c_char_p, _sz]),
    "nbody_tree_export_f32": (C.c_int, [_vp] + [_vp] * 7),
    "nbody_tree_export_f64": (C.c_int, [_vp] + [_vp] * 7),
    "nbody_host_tree_build_f32": (C.c_int, [_i32, _i64, _vp, _vp, C.POINTER(Params), C.POINTER(_vp)]),
    "nbody_host_tree_build_f64": (C.c_int, [_i32, _i64, _vp, _vp, C.POINTER(Params), C.POINTER(_vp)]),
    "nbody_host_tree_free": (None, [_vp]),
    "nbody_host_tree_info": (C.c_int, [_vp, C.POINTER(TreeView)]),
    "nbody_host_tree_export_f32": (C.c_int, [_vp] + [_vp] * 7),
    "nbody_host_tree_export_f64": (C.c_int, [_vp] + [_vp] * 7),
    "nbody_tree_walk_stats": (C.c_int, [_vp, _i32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "nbody_get_counting": (C.c_int, [_vp, C.POINTER(Counting)]),
    "nbody_direct_workspace_bytes": (_sz, [_i64, _i64]),
    "nbody_direct_step_dev": (C.c_int, [_vp, _i64, _vp, _vp, _f32, _i64, _i64, _vp, _vp, _vp, _f32, _f32, _i32, _vp, _sz, _vp]),
    "nbody_direct_workspace_peek": (C.c_int, [_vp, _vp, C.POINTER(C.c_int32 * 4)]),
    "nbody_weights_to_mass_dev": (C.c_int, [_vp, _i64, _vp, _vp]),
    "nbody_snapshot_begin": (C.c_int, [_vp]),
    "nbody_snapshot_pending": (C.c_int, [_vp]),
    "nbody_snapshot_end_f32": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_uint64)]),
    "nbody_snapshot_end_f64": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_uint64)]),
    "nbody_snapshot_num_tracers": (_i64, [_vp]),
    "nbody_snapshot_tracers_f32": (C.c_int, [_vp, _vp, _vp]),
    "nbody_snapshot_tracers_f64": (C.c_int, [_vp, _vp, _vp]),
    "nbody_delta_begin": (C.c_int, [_vp]),
    "nbody_delta_pending": (C.c_int, [_vp]),
    "nbody_delta_end": (C.c_int, [_vp, _vp, _sz, C.POINTER(_sz), C.POINTER(C.c_uint64)]),
    "nbody_delta_reset": (C.c_int, [_vp]),
    "nbody_delta_bound": (_sz, [_i64, C.c_int]),
    "nbody_tracers_delta_begin": (C.c_int, [_vp]),
    "nbody_tracers_delta_pending": (C.c_int, [_vp]),
    "nbody_tracers_delta_end": (C.c_int, [_vp, _vp, _sz, C.POINTER(_sz), C.POINTER(C.c_uint64)]),
    "nbody_tracers_delta_reset": (C.c_int, [_vp]),
    "nbody_delta_decoder_create": (_vp, []),
    "nbody_delta_decoder_destroy": (None, [_vp]),
    "nbody_delta_decoder_apply": (C.c_int, [_vp, _vp, _sz]),
    "nbody_delta_decoder_set_max_bodies": (C.c_int, [_vp, _i64]),
    "nbody_delta_decoder_error": (C.c_char_p, [_vp]),
    "nbody_delta_decoder_count": (_i64, [_vp]),
    "nbody_delta_decoder_is_f64": (C.c_int, [_vp]),
    "nbody_delta_decoder_step": (C.c_uint64, [_vp]),
    "nbody_delta_decoder_positions_f32": (C.c_int, [_vp, _vp]),
    "nbody_delta_decoder_positions_f64": (C.c_int, [_vp, _vp]),
    "nbody_render_rgba": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp]),
    "nbody_render_rgba_tracers": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp]),
    "nbody_render_rgba_dev": (C.c_int, [_vp, C.c_int64, C.c_int, _vp, _vp, _vp, C.c_uint32, C.c_uint32, _vp, _vp]),
    "nbody_selftest_exact_sum": (C.c_int, [_vp, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int64)]),
    "nbody_selftest_exact_sum_f64": (C.c_int, [_vp, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "nbody_selftest_exact_sum_f64_segmented": (C.c_int, [_vp, C.c_int64, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "nbody_selftest_div_pair": (C.c_int, [C.c_int, _vp, _vp, _vp, C.c_int64, _vp, _vp]),
    "nbody_selftest_exact_sum_chunked": (C.c_int, [_vp, C.c_int64, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int64)]),
    "nbody_selftest_walk_estimate": (C.c_int, [_i32, _vp, _i64, _vp, _i64, _i32, _i32] + [_i32] * 8 + [_vp] * 6 + [_i64, _vp]),
    "nbody_selftest_nearfar": (C.c_int, [_i32, _vp, _vp, _i64, _f32, _f32, _i32, _i32, _i32] + [_vp] * 6),
    "nbody_bvh_build_restarts": (C.c_int, [_vp]),
    "nbody_last_build_on_device": (C.c_int, [_vp]),
    "nbody_timer_create": (C.c_int, [C.POINTER(_vp)]),
    "nbody_timer_destroy": (None, [_vp]),
    "nbody_timer_read": (C.c_int, [_vp, _i32, C.POINTER(_f64), C.POINTER(_i64)]),
    "nbody_set_timer": (C.c_int, [_vp, _vp]),
}


def declared_symbols() -> list:
    """Every function include/nbody_hip.h declares (parsed from the header text and that of the headers it includes from its
    own directory: nbody_ensemble.h)."""
    with open(HEADER_PATH) as f:
        txt = f.read()
    for inc in re.findall(r'^#include "([\w.]+)"', txt, flags=re.M):
        with open(os.path.join(os.path.dirname(HEADER_PATH), inc)) as f:
            txt += f.read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", txt)))


def _share_hip_runtime_with_torch():
    """PyTorch-ROCm wheels bundle their own libamdhip64 and load it by absolute path.  Two HIP runtimes in one
    process do not coexist (whichever comes second sees no GPU), so when PyTorch is installed its copy is loaded
    first and libnbody_hip's DT_NEEDED libamdhip64 resolves to it by SONAME.  Without PyTorch the system ROCm
    runtime is used, as for any C/Rust host."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except Exception:
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    for d in spec.submodule_search_locations:
        cand = os.path.join(d, "lib", "libamdhip64.so")
        if os.path.exists(cand):
            try:
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
            except OSError:
                pass
            return


_libs = {}
_active = "lab" if os.environ.get("NBODY_HIP_LIBRARY", "") == "lab" else "product"   # tools/ run with NBODY_HIP_LIBRARY=lab


def _load(which: str) -> C.CDLL:
    if which not in _libs:
        path = LAB_LIB_PATH if which == "lab" else LIB_PATH
        if not os.path.exists(path):
            raise NBodyError(ERR_NO_DEVICE, f"{path} is not built (run __graft_entry__.build() or "
                                            f"`make -C nbody-simulation_amd/csrc`); there is no CPU fallback")
        _share_hip_runtime_with_torch()
        lib = C.CDLL(path)
        lib.nbody_abi_version.restype = C.c_int
        lib.nbody_abi_version.argtypes = []
        have = lib.nbody_abi_version()
        if have != ABI_VERSION:  # before anything else is bound: a stale library would fail with an obscure AttributeError
            raise NBodyError(ERR_INVALID, f"{path} has ABI version {have}, this binding was written against {ABI_VERSION}: "
                                          f"rebuild it (`make -C nbody-simulation_amd/csrc`)")
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _libs[which] = lib
    return _libs[which]


def load() -> C.CDLL:
    """The library every call of this module goes to: libnbody_hip.so — or, inside `with laboratory():` (or with
    NBODY_HIP_LIBRARY=lab in the environment when this module is imported), libnbody_hip_lab.so."""
    global _lib
    _lib = _load(_active)
    return _lib


class laboratory:
    """`with laboratory():` — this module's calls go to libnbody_hip_lab.so (csrc/env.h: the build that honours the laboratory
    switches NBODY_DIRECT_ASM, NBODY_WALK_TILE_*, NBODY_BVH_BLIND_LEVELS, ... and contains the retired kernel variants) until the
    block ends.  Contexts made inside must be closed inside.  The product library never reads those switches."""

    def __enter__(self):
        global _active
        self.prev = _active
        _active = "lab"
        load()
        return self

    def __exit__(self, *exc):
        global _active
        _active = self.prev
        return False


def _err(ctx, code):
    msg = load().nbody_last_error(ctx)
    return NBodyError(code, msg.decode() if msg else "")


def check(ctx, code):
    if code != OK:
        raise _err(ctx, code)


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def default_params() -> Params:
    p = Params()
    check(None, load().nbody_default_params(C.byref(p)))
    return p


class Timer:
    """HIP-event timer for the dominant kernel (nbody_timer_*)."""

    def __init__(self):
        self.h = _vp()
        check(None, load().nbody_timer_create(C.byref(self.h)))

    def read(self, reset=True):
        ms, cnt = _f64(0), _i64(0)
        check(None, load().nbody_timer_read(self.h, 1 if reset else 0, C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value

    def close(self):
        if self.h:
            load().nbody_timer_destroy(self.h)
            self.h = None

    __del__ = close


def selftest_exact_sum(x, tile=4096, seq_run=64):
    """CPU emulation of the device build's exact sequential-sum scan -> (sum as np.float32, restarts)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    out, st = C.c_float(0), _i64(0)
    check(None, load().nbody_selftest_exact_sum(_ptr(x) if x.size else None, x.size, int(tile), int(seq_run),
                                                C.byref(out), C.byref(st)))
    return np.float32(out.value), st.value


def selftest_exact_sum_f64(x, tile=4096, seq_run=16):
    """CPU emulation of the f64 device build's exact sequential-sum scan -> (sum as np.float64, restarts)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out, st = C.c_double(0), _i64(0)
    check(None, load().nbody_selftest_exact_sum_f64(_ptr(x) if x.size else None, x.size, int(tile), int(seq_run),
                                                    C.byref(out), C.byref(st)))
    return np.float64(out.value), st.value


def selftest_exact_sum_f64_segmented(x, seg=8192):
    """CPU emulation of the segmented f64 fold (runs per segment, predicted binades) -> (sum, runs applied)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out, used = C.c_double(0), _i64(0)
    check(None, load().nbody_selftest_exact_sum_f64_segmented(_ptr(x) if x.size else None, x.size, int(seg), C.byref(out), C.byref(used)))
    return np.float64(out.value), used.value


def selftest_div_pair(nx, ny, den, device=0):
    """csrc/div_pair.h on the device: (nx / den, ny / den) as the exact kernels compute them."""
    nx, ny, den = (np.ascontiguousarray(a, np.float32) for a in (nx, ny, den))
    assert nx.shape == ny.shape == den.shape and nx.ndim == 1
    qx, qy = np.empty_like(nx), np.empty_like(nx)
    if nx.size:
        check(None, load().nbody_selftest_div_pair(int(device), _ptr(nx), _ptr(ny), _ptr(den), nx.size, _ptr(qx), _ptr(qy)))
    return qx, qy


def selftest_walk_estimate(hist, ids, shift=0, route=2, nodes=1, node_count=1, fallback=0, bad_index=0, long_nodes=0, level_end=0,
                           node_cap=1, keep_scratch=False, clear_words=128, device=0):
    """The one-pass walk's preparation alone on the device (nbody_selftest_walk_estimate) -> dict of off, info, verdict, pack,
    flags, clear, extra, grid_waves, kept."""
    hist = np.ascontiguousarray(hist, np.uint32)
    ids = np.ascontiguousarray(ids, np.uint32)
    assert hist.ndim == 1 and ids.ndim == 1
    off = np.empty(ids.size, np.uint32)
    info, verdict = np.zeros(8, np.int32), np.zeros(2, np.int32)
    pack, flags = np.zeros(2 + 128 + 8, np.int32), np.zeros(128, np.int32)
    clear, used = np.zeros(int(clear_words), np.int32), np.zeros(4, np.int64)
    check(None, load().nbody_selftest_walk_estimate(int(device), _ptr(hist), hist.size, _ptr(ids), ids.size, int(shift), int(route), int(nodes),
                                                    int(node_count), int(fallback), int(bad_index), int(long_nodes), int(level_end),
                                                    int(node_cap), 1 if keep_scratch else 0, _ptr(off), _ptr(info), _ptr(verdict), _ptr(pack),
                                                    _ptr(flags), _ptr(clear), int(clear_words), _ptr(used)))
    return dict(off=off, info=info, verdict=verdict, pack=pack, flags=flags, clear=clear, extra=int(used[0]), grid_waves=int(used[1]),
                kept=bool(used[2]))


def selftest_nearfar(pos, mass=None, heavy_base=0.0, clamp=0.001, use_hazard=False, couples=True, with_minv=False, device=0):
    """The near/far split of a direct step alone on the device (nbody_selftest_nearfar) -> dict of flags (hazard, fallback,
    n_near, state), is_near, scan, near_list (the n_near entries written), far (the raw far copy: 2 * 16 * ceil(n / 16) floats in
    couples, or (n, 2) without) and minv (16 * ceil(n / 16) floats, or None)."""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 2)
    n = pos.shape[0]
    if mass is not None:
        mass = np.ascontiguousarray(mass, np.float32)
        assert mass.shape == (n,)
    padded = (n + 15) // 16 * 16
    flags = np.zeros(4, np.int32)
    is_near, scan, near_list = (np.empty(n, np.uint32) for _ in range(3))
    far = np.empty(2 * padded if couples else 2 * n, np.float32)
    minv = np.empty(padded, np.float32) if with_minv else None
    check(None, load().nbody_selftest_nearfar(int(device), _ptr(pos), _ptr(mass), n, float(heavy_base), float(clamp), 1 if use_hazard else 0,
                                              1 if couples else 0, 1 if with_minv else 0, _ptr(flags), _ptr(is_near), _ptr(scan),
                                              _ptr(near_list), _ptr(far), _ptr(minv)))
    n_near = min(max(int(flags[2]), 0), n)
    return dict(flags=tuple(int(f) for f in flags), is_near=is_near, scan=scan, near_list=near_list[:n_near].copy(),
                far=far if couples else far.reshape(n, 2), minv=minv)


def selftest_exact_sum_chunked(x, chunk=2048):
    """CPU emulation of the chunked exact sum (predicted binades, runs with bounds) -> (sum, chunks taken whole)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    out, used = C.c_float(0), _i64(0)
    check(None, load().nbody_selftest_exact_sum_chunked(_ptr(x) if x.size else None, x.size, int(chunk), C.byref(out), C.byref(used)))
    return np.float32(out.value), used.value


class DeltaDecoder:
    """Receiving side of the delta snapshots (host only): apply every stream since the key frame, in order."""

    def __init__(self):
        self.lib = load()
        self.h = self.lib.nbody_delta_decoder_create()
        if not self.h:
            raise MemoryError("nbody_delta_decoder_create")

    def close(self):
        if getattr(self, "h", None):
            self.lib.nbody_delta_decoder_destroy(self.h)
            self.h = None

    __del__ = close

    def set_max_bodies(self, n: int):
        """Refuse streams whose header claims more than n bodies (the stream is untrusted input)."""
        rc = self.lib.nbody_delta_decoder_set_max_bodies(self.h, int(n))
        if rc != 0:
            raise NBodyError(rc, "delta decoder: set_max_bodies")

    def apply(self, stream: bytes):
        buf = np.frombuffer(bytes(stream), np.uint8)
        rc = self.lib.nbody_delta_decoder_apply(self.h, buf.ctypes.data_as(C.c_void_p) if buf.size else None, buf.size)
        if rc != 0:
            raise NBodyError(rc, self.lib.nbody_delta_decoder_error(self.h).decode())

    @property
    def n(self) -> int:
        return int(self.lib.nbody_delta_decoder_count(self.h))

    @property
    def step(self) -> int:
        return int(self.lib.nbody_delta_decoder_step(self.h))

    @property
    def dtype(self):
        return np.float64 if self.lib.nbody_delta_decoder_is_f64(self.h) else np.float32

    def positions(self):
        """Positions of the last applied snapshot, (n, 2), in upload (id) order."""
        n, dt = self.n, self.dtype
        if n < 0:
            raise NBodyError(ERR_INVALID, "no key frame applied yet")
        out = np.zeros((n, 2), dt)
        f = self.lib.nbody_delta_decoder_positions_f64 if dt == np.float64 else self.lib.nbody_delta_decoder_positions_f32
        rc = f(self.h, _ptr(out))
        if rc != 0:
            raise NBodyError(rc, "delta decoder: positions")
        return out


def host_tree(kind, pos, weight=None, params: "Params | None" = None):
    """Build the linearised tree on the host with the product builder (no device needed).
    -> dict(geom, mass, is_leaf, first, count, skip, order, kind, max_depth, overflow)."""
    lib = load()
    pos = np.asarray(pos)
    dt = np.float64 if pos.dtype == np.float64 else np.float32
    pos = np.ascontiguousarray(pos, dtype=dt).reshape(-1, 2)
    n = pos.shape[0]
    w = None if weight is None else np.ascontiguousarray(weight, dtype=np.uint32)
    h = _vp()
    f = lib.nbody_host_tree_build_f64 if dt == np.float64 else lib.nbody_host_tree_build_f32
    rc = f(int(kind), n, _ptr(pos), _ptr(w), C.byref(params) if params is not None else None, C.byref(h))
    if rc not in (OK, ERR_DEGENERATE):
        raise _err(None, rc)
    try:
        v = TreeView()
        check(None, lib.nbody_host_tree_info(h, C.byref(v)))
        m = v.n_nodes
        out = dict(geom=np.zeros((m, 6 if v.kind == TREE_BVH else 5), dt), mass=np.zeros(m, np.uint32),
                   is_leaf=np.zeros(m, np.int32), first=np.zeros(m, np.int64), count=np.zeros(m, np.int64),
                   skip=np.zeros(m, np.int64), order=np.zeros(n, np.uint32))
        fe = lib.nbody_host_tree_export_f64 if dt == np.float64 else lib.nbody_host_tree_export_f32
        check(None, fe(h, _ptr(out["geom"]), _ptr(out["mass"]), _ptr(out["is_leaf"]), _ptr(out["first"]),
                       _ptr(out["count"]), _ptr(out["skip"]), _ptr(out["order"])))
        out.update(kind=v.kind, max_depth=v.max_depth, overflow=(rc == ERR_DEGENERATE))
        return out
    finally:
        lib.nbody_host_tree_free(h)


def _tree_arrays(tree, dt):
    return dict(geom=np.ascontiguousarray(tree["geom"], dtype=dt), mass=np.ascontiguousarray(tree["mass"], dtype=np.uint32),
                is_leaf=np.ascontiguousarray(tree["is_leaf"], dtype=np.int32), first=np.ascontiguousarray(tree["first"], dtype=np.int64),
                count=np.ascontiguousarray(tree["count"], dtype=np.int64), skip=np.ascontiguousarray(tree["skip"], dtype=np.int64),
                order=np.ascontiguousarray(tree["order"], dtype=np.uint32))


def tree_validate(tree, n_particles=None):
    """The shape check nbody_walk_tree_* applies to a caller's tree, on the host alone -> (ok, reason)."""
    lib = load()
    a = _tree_arrays(tree, np.float32)
    n = a["order"].shape[0] if n_particles is None else int(n_particles)
    buf = C.create_string_buffer(256)
    rc = lib.nbody_tree_validate(int(tree["kind"]), a["skip"].shape[0], _ptr(a["is_leaf"]), _ptr(a["first"]), _ptr(a["count"]),
                                 _ptr(a["skip"]), n, _ptr(a["order"]), buf, 256)
    return rc == OK, buf.value.decode()


class Context:
    """Owner of one nbody_ctx (one GPU)."""

    def __init__(self, device: int = 0):
        self.lib = load()
        self.h = _vp()
        rc = self.lib.nbody_create(C.byref(self.h), int(device))
        if rc != OK:
            self.h = None
            raise _err(None, rc)
        self.dtype = None
        self.n = 0

    @property
    def stream(self) -> int:
        """The hipStream_t the context enqueues its steps on, as an integer (torch.cuda.ExternalStream takes it)."""
        return int(self.lib.nbody_get_stream(self.h) or 0)

    def multi_info(self):
        """-> (devices, exchange or -1, chunks per direct step, bodies per target block)."""
        g, x, c, b = C.c_int(0), C.c_int(0), C.c_int(0), _i64(0)
        check(self.h, self.lib.nbody_multi_info(self.h, C.byref(g), C.byref(x), C.byref(c), C.byref(b)))
        return g.value, x.value, c.value, b.value

    def comm_count(self) -> int:
        """Ranks of the context's RCCL communicator as ncclCommCount reports them (0: none)."""
        k = C.c_int(0)
        check(self.h, self.lib.nbody_multi_comm_count(self.h, C.byref(k)))
        return k.value

    def close(self):
        if getattr(self, "h", None):
            self.lib.nbody_destroy(self.h)
            self.h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- params
    def get_params(self) -> Params:
        p = Params()
        check(self.h, self.lib.nbody_get_params(self.h, C.byref(p)))
        return p

    def set_params(self, **kw):
        p = self.get_params()
        for k, v in kw.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
        check(self.h, self.lib.nbody_set_params(self.h, C.byref(p)))

    def set_timer(self, timer: "Timer | None"):
        check(self.h, self.lib.nbody_set_timer(self.h, timer.h if timer else None))

    # ---- state
    def upload(self, pos, vel, weight=None):
        pos = np.asarray(pos)
        dt = np.float64 if pos.dtype == np.float64 else np.float32
        pos = np.ascontiguousarray(pos, dtype=dt).reshape(-1, 2)
        vel = np.ascontiguousarray(vel, dtype=dt).reshape(-1, 2)
        n = pos.shape[0]
        if vel.shape[0] != n:
            raise ValueError("pos/vel length mismatch")
        w = None if weight is None else np.ascontiguousarray(weight, dtype=np.uint32)
        if w is not None and w.shape[0] != n:
            raise ValueError("weight length mismatch")
        f = self.lib.nbody_upload_f64 if dt == np.float64 else self.lib.nbody_upload_f32
        check(self.h, f(self.h, n, _ptr(pos), _ptr(vel), _ptr(w)))
        self.dtype, self.n = dt, n

    def download(self):
        """-> (pos[n,2], vel[n,2], weight[n], ids[n]) in the current row order."""
        dt, n = self.dtype, self.n
        pos = np.zeros((n, 2), dt)
        vel = np.zeros((n, 2), dt)
        w = np.zeros(n, np.uint32)
        ids = np.zeros(n, np.uint32)
        f = self.lib.nbody_download_f64 if dt == np.float64 else self.lib.nbody_download_f32
        check(self.h, f(self.h, _ptr(pos), _ptr(vel), _ptr(w), _ptr(ids)))
        return pos, vel, w, ids

    def upload_tracers(self, pos, vel):
        """Massless tracers (m, 2) that every update_direct / update_tree step advances with the bodies, on the device
        (nbody_tracers_upload_*): cast to the context's dtype; replaces any earlier set, m == 0 removes them."""
        if self.dtype is None:
            raise NBodyError(ERR_INVALID, "upload_tracers: tracers need particles uploaded first")
        pos = np.ascontiguousarray(pos, dtype=self.dtype).reshape(-1, 2)
        vel = np.ascontiguousarray(vel, dtype=self.dtype).reshape(-1, 2)
        if vel.shape[0] != pos.shape[0]:
            raise ValueError("pos/vel length mismatch")
        f = self.lib.nbody_tracers_upload_f64 if self.dtype == np.float64 else self.lib.nbody_tracers_upload_f32
        check(self.h, f(self.h, pos.shape[0], _ptr(pos), _ptr(vel)))

    def download_tracers(self):
        """-> (pos[m,2], vel[m,2]) of the tracers, in upload order."""
        m, dt = self.n_tracers, self.dtype
        pos, vel = np.zeros((m, 2), dt), np.zeros((m, 2), dt)
        f = self.lib.nbody_tracers_download_f64 if dt == np.float64 else self.lib.nbody_tracers_download_f32
        check(self.h, f(self.h, _ptr(pos), _ptr(vel)))
        return pos, vel

    @property
    def n_tracers(self) -> int:
        return int(self.lib.nbody_num_tracers(self.h))

    # ---- steps
    def update_direct(self, delta, n_steps=1, counter: Counting | None = None):
        f = self.lib.nbody_update_direct_f64 if self.dtype == np.float64 else self.lib.nbody_update_direct_f32
        check(self.h, f(self.h, float(delta), int(n_steps), C.byref(counter) if counter is not None else None))

    def update_tree(self, kind, delta, n_steps=1, counter: Counting | None = None):
        f = self.lib.nbody_update_tree_f64 if self.dtype == np.float64 else self.lib.nbody_update_tree_f32
        check(self.h, f(self.h, int(kind), float(delta), int(n_steps),
                        C.byref(counter) if counter is not None else None))

    def update_tree_async(self, kind, delta, n_steps=1):
        """f32 only: returns once the steps are enqueued; `wait()` (or any call that reads the rows) completes them."""
        check(self.h, self.lib.nbody_update_tree_async_f32(self.h, int(kind), float(delta), int(n_steps)))

    def wait(self):
        check(self.h, self.lib.nbody_wait(self.h))

    def update_tree_shard(self, kind, delta, begin, count, counter: Counting | None = None):
        f = self.lib.nbody_update_tree_shard_f64 if self.dtype == np.float64 else self.lib.nbody_update_tree_shard_f32
        check(self.h, f(self.h, int(kind), float(delta), int(begin), int(count),
                        C.byref(counter) if counter is not None else None))

    def export_slice_dev(self, begin, count, rows_ptr, pos_ptr, vel_ptr):
        check(self.h, self.lib.nbody_export_slice_dev(self.h, int(begin), int(count), _vp(rows_ptr), _vp(pos_ptr), _vp(vel_ptr)))

    def import_rows_dev(self, n_rows, rows_ptr, pos_ptr, vel_ptr):
        check(self.h, self.lib.nbody_import_rows_dev(self.h, int(n_rows), _vp(rows_ptr), _vp(pos_ptr), _vp(vel_ptr)))

    def accel_direct(self, targets=None):
        """The direct sum at the bodies, in row order — or, with an (m, 2) array `targets` (cast to the context's dtype), at
        those points (nbody_accel_direct_at_*: no mass, no self term; a target's result depends on its position alone)."""
        if targets is not None:
            dt = np.float64 if self.dtype == np.float64 else np.float32
            f = self.lib.nbody_accel_direct_at_f64 if dt == np.float64 else self.lib.nbody_accel_direct_at_f32
            tg = np.ascontiguousarray(targets, dtype=dt).reshape(-1, 2)
            acc = np.zeros_like(tg)
            check(self.h, f(self.h, tg.shape[0], _ptr(tg), _ptr(acc)))
            return acc
        if self.dtype == np.float64:
            acc = np.zeros((self.n, 2), np.float64)
            check(self.h, self.lib.nbody_accel_direct_f64(self.h, _ptr(acc)))
        else:
            acc = np.zeros((self.n, 2), np.float32)
            check(self.h, self.lib.nbody_accel_direct_f32(self.h, _ptr(acc)))
        return acc

    def accel_tree(self, kind, targets=None):
        dt = self.dtype
        f = self.lib.nbody_accel_tree_f64 if dt == np.float64 else self.lib.nbody_accel_tree_f32
        if targets is None:
            acc = np.zeros((self.n, 2), dt)
            check(self.h, f(self.h, int(kind), 0, None, _ptr(acc)))
            return acc
        tg = np.ascontiguousarray(targets, dtype=dt).reshape(-1, 2)
        acc = np.zeros_like(tg)
        check(self.h, f(self.h, int(kind), tg.shape[0], _ptr(tg), _ptr(acc)))
        return acc

    def walk_tree(self, tree, targets=None):
        """The force map alone over a caller's linearised tree (nbody_walk_tree_*): `tree` is a dict in tree_export()'s /
        host_tree()'s layout (geom, mass, is_leaf, first, count, skip, order, kind) over the uploaded particles.
        targets None: the particles themselves, in the row order after the call (BVH: tree order; quad: unchanged)."""
        dt = self.dtype
        f = self.lib.nbody_walk_tree_f64 if dt == np.float64 else self.lib.nbody_walk_tree_f32
        a = _tree_arrays(tree, dt)
        if targets is None:
            tg, nt = None, 0
            acc = np.zeros((self.n, 2), dt)
        else:
            tg = np.ascontiguousarray(targets, dtype=dt).reshape(-1, 2)
            nt = tg.shape[0]
            acc = np.zeros_like(tg)
        check(self.h, f(self.h, int(tree["kind"]), a["geom"].shape[0], _ptr(a["geom"]), _ptr(a["mass"]), _ptr(a["is_leaf"]),
                        _ptr(a["first"]), _ptr(a["count"]), _ptr(a["skip"]), _ptr(a["order"]), nt, _ptr(tg), _ptr(acc)))
        return acc

    def snapshot_begin(self):
        """Start the asynchronous hand-off of the current rows (main.rs:136-139); steps may follow at once."""
        check(self.h, self.lib.nbody_snapshot_begin(self.h))

    def snapshot_pending(self) -> bool:
        return bool(self.lib.nbody_snapshot_pending(self.h))

    def snapshot_end(self):
        """-> (position, velocity, weight, ids, steps done when the snapshot was taken)."""
        n, dt = self.n, self.dtype
        pos, vel = np.zeros((n, 2), dt), np.zeros((n, 2), dt)
        w, ids = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        step = C.c_uint64(0)
        f = self.lib.nbody_snapshot_end_f64 if dt == np.float64 else self.lib.nbody_snapshot_end_f32
        check(self.h, f(self.h, _ptr(pos), _ptr(vel), _ptr(w), _ptr(ids), C.byref(step)))
        return pos, vel, w, ids, step.value

    def snapshot_tracers(self):
        """-> (position[m,2], velocity[m,2]) of the tracers the context held at snapshot_begin, in upload order; the snapshot
        stays pending (snapshot_end takes the bodies)."""
        m = int(self.lib.nbody_snapshot_num_tracers(self.h))
        if m < 0:
            raise _err(self.h, m)
        dt = self.dtype
        pos, vel = np.zeros((m, 2), dt), np.zeros((m, 2), dt)
        f = self.lib.nbody_snapshot_tracers_f64 if dt == np.float64 else self.lib.nbody_snapshot_tracers_f32
        check(self.h, f(self.h, _ptr(pos), _ptr(vel)))
        return pos, vel

    def delta_begin(self):
        """Encode the positions (id order) against the previous delta snapshot and start the stream's hand-off."""
        check(self.h, self.lib.nbody_delta_begin(self.h))

    def delta_pending(self) -> bool:
        return bool(self.lib.nbody_delta_pending(self.h))

    def delta_end(self, cap=None):
        """-> (the stream as bytes, steps done when it was taken)."""
        if cap is None:
            cap = int(self.lib.nbody_delta_bound(self.n, 1 if self.dtype == np.float64 else 0))
        buf = np.zeros(max(int(cap), 1), np.uint8)
        size, step = _sz(0), C.c_uint64(0)
        check(self.h, self.lib.nbody_delta_end(self.h, _ptr(buf), int(cap), C.byref(size), C.byref(step)))
        return buf[:size.value].tobytes(), step.value

    def delta_reset(self):
        check(self.h, self.lib.nbody_delta_reset(self.h))

    def tracers_delta_begin(self):
        """delta_begin for the tracers' positions (upload order): a sequence of streams of its own, beside the bodies'."""
        check(self.h, self.lib.nbody_tracers_delta_begin(self.h))

    def tracers_delta_pending(self) -> bool:
        return self.lib.nbody_tracers_delta_pending(self.h) == 1

    def tracers_delta_end(self, cap=None):
        """-> (the tracers' stream as bytes, steps done when it was taken); a second DeltaDecoder decodes the sequence."""
        if cap is None:   # sized for the tracers the context holds now; pass `cap` if they were replaced since the begin
            cap = int(self.lib.nbody_delta_bound(self.n_tracers, 1 if self.dtype == np.float64 else 0))
        buf = np.zeros(max(int(cap), 1), np.uint8)
        size, step = _sz(0), C.c_uint64(0)
        check(self.h, self.lib.nbody_tracers_delta_end(self.h, _ptr(buf), int(cap), C.byref(size), C.byref(step)))
        return buf[:size.value].tobytes(), step.value

    def tracers_delta_reset(self):
        check(self.h, self.lib.nbody_tracers_delta_reset(self.h))

    def render(self, height=100_000, render_px=1250, tracers=False):
        """The reference's draw() of the current rows -> uint8 array (render_px, render_px, 4), RGBA.  tracers=True: of the
        rows followed by the tracers as rows of weight 1 (nbody_render_rgba_tracers)."""
        out = np.zeros((render_px, render_px, 4), np.uint8)
        f = self.lib.nbody_render_rgba_tracers if tracers else self.lib.nbody_render_rgba
        check(self.h, f(self.h, int(height), int(render_px), _ptr(out)))
        return out

    def last_build_on_device(self) -> bool:
        return bool(self.lib.nbody_last_build_on_device(self.h))

    def bvh_build_restarts(self) -> int:
        return int(self.lib.nbody_bvh_build_restarts(self.h))

    def tree_info(self) -> TreeView:
        v = TreeView()
        check(self.h, self.lib.nbody_tree_info(self.h, C.byref(v)))
        return v

    def tree_export(self):
        """-> dict(geom, mass, is_leaf, first, count, skip, order) of the last build."""
        v = self.tree_info()
        m, dt = v.n_nodes, self.dtype
        geom = np.zeros((m, 6 if v.kind == TREE_BVH else 5), dt)
        out = dict(geom=geom, mass=np.zeros(m, np.uint32), is_leaf=np.zeros(m, np.int32),
                   first=np.zeros(m, np.int64), count=np.zeros(m, np.int64), skip=np.zeros(m, np.int64),
                   order=np.zeros(self.n, np.uint32))
        f = self.lib.nbody_tree_export_f64 if dt == np.float64 else self.lib.nbody_tree_export_f32
        check(self.h, f(self.h, _ptr(out["geom"]), _ptr(out["mass"]), _ptr(out["is_leaf"]), _ptr(out["first"]),
                        _ptr(out["count"]), _ptr(out["skip"]), _ptr(out["order"])))
        out["kind"], out["max_depth"] = v.kind, v.max_depth
        return out

    def walk_stats(self, enable=True):
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        check(self.h, self.lib.nbody_tree_walk_stats(self.h, 1 if enable else 0, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def counting(self) -> Counting:
        c = Counting()
        check(self.h, self.lib.nbody_get_counting(self.h, C.byref(c)))
        return c


class MultiContext(Context):
    """Several GPUs of one node behind one handle (nbody_create_multi): the same calls as Context; the library shards
    every update over the devices and does the exchange itself (RCCL all-gather, or peer copies)."""

    def __init__(self, devices, exchange: int | None = None, chunks: int = 0):
        self.lib = load()
        self.h = _vp()
        ids = (C.c_int * len(devices))(*[int(d) for d in devices])
        if exchange is None:
            rc = self.lib.nbody_create_multi(C.byref(self.h), len(devices), ids)
        else:
            rc = self.lib.nbody_create_multi_ex(C.byref(self.h), len(devices), ids, int(exchange), int(chunks))
        if rc != OK:
            self.h = None
            raise _err(None, rc)
        self.dtype = None
        self.n = 0

    def update_direct(self, delta, n_steps=1, counter: Counting | None = None):
        """Multi-device direct steps are f32 only: after an f64 upload this fails, as it always has."""
        check(self.h, self.lib.nbody_update_direct_f32(self.h, float(delta), int(n_steps),
                                                       C.byref(counter) if counter is not None else None))

    def upload_tracers(self, pos, vel):
        raise NBodyError(ERR_INVALID, "upload_tracers: tracers are not available on a multi-device context")

    def download_tracers(self):
        raise NBodyError(ERR_INVALID, "download_tracers: tracers are not available on a multi-device context")


class _EnsembleHandleBase:
    """Owner of one ensemble handle of the C API (one GPU): many worlds of one size, world-major arrays of `_dtype`, every step
    of all of them one launch.  The C calls are `_prefix` + name, the typed ones with `_suffix`.  Arrays come in contiguous and
    checked (ensemble.py does that); this class only passes them on."""
    _prefix = _suffix = _dtype = None

    def _call(self, name, *args):
        return getattr(self.lib, self._prefix + name)(self.h, *args)

    def __init__(self, device: int = 0):
        self.lib = load()
        self.h = _vp()
        rc = getattr(self.lib, self._prefix + "_create")(C.byref(self.h), int(device))
        if rc != OK:
            self.h = None
            raise self._err(rc)

    def _err(self, code):
        msg = self._call("_last_error")
        return NBodyError(code, msg.decode() if msg else "")

    def _check(self, code):
        if code != OK:
            raise self._err(code)

    def close(self):
        if getattr(self, "h", None):
            self._call("_destroy")
            self.h = None

    __del__ = close

    def get_params(self) -> Params:
        p = Params()
        self._check(self._call("_get_params", C.byref(p)))
        return p

    def set_params(self, **kw):
        p = self.get_params()
        for k, v in kw.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
        self._check(self._call("_set_params", C.byref(p)))

    @property
    def shape(self):
        """(worlds, bodies per world) of the current upload; (0, 0) before one."""
        return int(self._call("_num_worlds")), int(self._call("_num_bodies"))

    def upload(self, n_worlds, n_bodies, pos, vel, weight):
        self._check(self._call("_upload" + self._suffix, int(n_worlds), int(n_bodies), _ptr(pos), _ptr(vel), _ptr(weight)))

    def download(self):
        b, n = self.shape
        pos, vel = np.zeros((b, n, 2), self._dtype), np.zeros((b, n, 2), self._dtype)
        self._check(self._call("_download" + self._suffix, _ptr(pos), _ptr(vel)))
        return pos, vel

    def update(self, delta, n_steps=1, counter: "Counting | None" = None):
        self._check(self._call("_update" + self._suffix, float(delta), int(n_steps),
                               C.byref(counter) if counter is not None else None))

    def accel(self):
        b, n = self.shape
        acc = np.zeros((b, n, 2), self._dtype)
        self._check(self._call("_accel" + self._suffix, _ptr(acc)))
        return acc

    def sweep(self, delta, clamp, steps, n_steps, counter: "Counting | None" = None):
        """nbody_sweep_<handle>: delta [worlds] of the handle's dtype, clamp float32[worlds] or None, steps int32[worlds] or None,
        all contiguous (ensemble.py's `sweep` checks and casts them)."""
        def typed(a, ctype):
            return None if a is None else a.ctypes.data_as(C.POINTER(ctype))
        name = "nbody_sweep_" + self._prefix[len("nbody_"):]
        real = C.c_double if self._dtype == np.float64 else C.c_float
        self._check(getattr(self.lib, name)(self.h, typed(delta, real), typed(clamp, C.c_float), typed(steps, C.c_int32), int(n_steps),
                                            C.byref(counter) if counter is not None else None))

    def resident(self, delta, clamp, steps, n_steps, counter: "Counting | None" = None):
        """nbody_resident_<handle> (the four handles without tracers): `sweep`'s arguments, `sweep`'s rows afterwards."""
        def typed(a, ctype):
            return None if a is None else a.ctypes.data_as(C.POINTER(ctype))
        name = "nbody_resident_" + self._prefix[len("nbody_"):]
        if name not in _SIGS:   # the handles with tracers inherit this method, and the library has no such call for them
            raise NBodyError(ERR_INVALID, f"{name}: resident runs are not offered on a handle with tracers (sweep is the call)")
        real = C.c_double if self._dtype == np.float64 else C.c_float
        self._check(getattr(self.lib, name)(self.h, typed(delta, real), typed(clamp, C.c_float), typed(steps, C.c_int32), int(n_steps),
                                            C.byref(counter) if counter is not None else None))

    _frames_tracers = False   # the handle's nbody_frames_* call takes with_tracers

    def frames(self, height, render_px, tracers=False):
        """nbody_frames_<handle>: every world's draw() raster of the current rows -> uint8 (worlds, render_px, render_px, 4).
        Arguments the C call cannot take as uint32 go to it as 0, which it refuses."""
        height, render_px = (v if 0 <= v < 1 << 32 else 0 for v in (int(height), int(render_px)))
        worlds = self.shape[0]
        # more than 2^26 pixels: the library refuses before it writes, so the output is not sized for them
        out = np.zeros((worlds, render_px, render_px, 4) if worlds * render_px * render_px <= 1 << 26 else (1, 1, 1, 4), np.uint8)
        name = "nbody_frames_" + self._prefix[len("nbody_"):]
        args = (height, render_px, 1 if tracers else 0) if self._frames_tracers else (height, render_px)
        self._check(getattr(self.lib, name)(self.h, *args, _ptr(out)))
        return out

    def summary(self, height, ref, tracers=False):
        """nbody_summary_<handle>: one record per world of the current rows (tracers=True: of the tracers' segments) ->
        SUMMARY_DTYPE[worlds].  ref: int32[worlds], contiguous, or None (ensemble.py's `summary` checks and casts it)."""
        out = np.zeros(self.shape[0], SUMMARY_DTYPE)
        name = "nbody_summary_" + self._prefix[len("nbody_"):]
        self._check(getattr(self.lib, name)(self.h, SUMMARY_TRACERS if tracers else 0, int(height),
                                            None if ref is None else ref.ctypes.data_as(C.POINTER(C.c_int32)), _ptr(out)))
        return out

    def encounters(self, limit2, tracers=False, rows=True):
        """nbody_encounters_<handle>: per target its nearest source and its clamped pairs, per world one record, of the current
        rows (tracers=True: the tracers against the bodies) -> (ENCOUNTERS_DTYPE[worlds], nn_index int32[targets], nn_d2
        [targets] of the handle's dtype, close uint32[targets]), the three per-target arrays flat in the download's order, or None
        with rows=False.  limit2: float32[worlds], contiguous, or None (ensemble.py's `encounters` checks and casts it)."""
        out = np.zeros(self.shape[0], ENCOUNTERS_DTYPE)
        total = int(self._delta_rows(tracers).sum()) if rows else 0
        index, d2, close = (np.zeros(total, t) for t in (np.int32, self._dtype, np.uint32)) if rows else (None, None, None)
        name = "nbody_encounters_" + self._prefix[len("nbody_"):]
        self._check(getattr(self.lib, name)(self.h, ENCOUNTERS_TRACERS if tracers else 0,
                                            None if limit2 is None else limit2.ctypes.data_as(C.POINTER(C.c_float)), _ptr(out),
                                            _ptr(index), _ptr(d2), _ptr(close)))
        return out, index, d2, close

    def watch(self, delta, n_steps, stride, limit2, height, tracers=False, resume=False, rows=True, counter: "Counting | None" = None):
        """nbody_watch_<handle>: update(delta, n_steps) with every world sampled before, between and after the steps (every
        `stride`-th sample; resume=True: not sample 0) -> (WATCH_DTYPE[worlds], dict of the six per-target arrays of WATCH_ROWS,
        flat in the download's order — min_d2 of the handle's dtype, min_index int32, the rest uint32 — or None with rows=False).
        limit2: float32[worlds], contiguous, or None (ensemble.py's `watch` checks and casts the arguments)."""
        out = np.zeros(self.shape[0], WATCH_DTYPE)
        arrays, block = None, None
        if rows:
            total = int(self._delta_rows(tracers).sum())
            arrays = {name: np.zeros(total, self._dtype if name == "min_d2" else np.int32 if name == "min_index" else np.uint32)
                      for name in WATCH_ROWS}
            block = WatchRows(*[a.ctypes.data for a in arrays.values()])
        name = "nbody_watch_" + self._prefix[len("nbody_"):]
        self._check(getattr(self.lib, name)(self.h, (WATCH_TRACERS if tracers else 0) | (WATCH_RESUME if resume else 0), float(delta),
                                            int(n_steps), int(stride), None if limit2 is None else limit2.ctypes.data_as(C.POINTER(C.c_float)),
                                            int(height), _ptr(out), C.byref(block) if block is not None else None,
                                            C.byref(counter) if counter is not None else None))
        return out, arrays

    def watch_sweep(self, delta, clamp, steps, n_steps, stride, limit2, height, tracers=False, resume=False, rows=True,
                    counter: "Counting | None" = None):
        """nbody_wsweep_<handle>: sweep(delta, clamp, steps, n_steps) with world k sampled at every s <= steps[k] with s %
        stride[k] == 0 (resume=True: not s = 0) -> what `watch` returns.  delta [worlds] of the handle's dtype; clamp, limit2
        float32[worlds] or None; steps, stride int32[worlds] or None; all contiguous (ensemble.py's `watch_sweep` checks and
        casts them)."""
        def typed(a, ctype):
            return None if a is None else a.ctypes.data_as(C.POINTER(ctype))
        out = np.zeros(self.shape[0], WATCH_DTYPE)
        arrays, block = None, None
        if rows:
            total = int(self._delta_rows(tracers).sum())
            arrays = {name: np.zeros(total, self._dtype if name == "min_d2" else np.int32 if name == "min_index" else np.uint32)
                      for name in WATCH_ROWS}
            block = WatchRows(*[a.ctypes.data for a in arrays.values()])
        name = "nbody_wsweep_" + self._prefix[len("nbody_"):]
        real = C.c_double if self._dtype == np.float64 else C.c_float
        self._check(getattr(self.lib, name)(self.h, (WATCH_TRACERS if tracers else 0) | (WATCH_RESUME if resume else 0), typed(delta, real),
                                            typed(clamp, C.c_float), typed(steps, C.c_int32), int(n_steps), typed(stride, C.c_int32),
                                            typed(limit2, C.c_float), int(height), _ptr(out), C.byref(block) if block is not None else None,
                                            C.byref(counter) if counter is not None else None))
        return out, arrays

    def _delta_rows(self, tracers):
        """The rows of every segment a deltas(), encounters() or watch() call addresses, int64[worlds]."""
        b, n = self.shape
        return np.full(b, getattr(self, "n_tracers", 0) if tracers else n, np.int64)

    def deltas(self, tracers=False, key=False, cap=None):
        """nbody_deltas_<handle>: one NBD1 stream per world of the current positions (tracers=True: of the tracers' sequence;
        key=True: key frames) -> (buffer uint8[bytes], offsets uint64[worlds + 1], step): world k's stream is
        buffer[offsets[k]:offsets[k + 1]].  The buffer is sized by nbody_deltas_bound unless `cap` says otherwise; a call the
        library refuses for a small `cap` raises with the bytes it needs in the error's `needed`."""
        rows = self._delta_rows(tracers)
        if cap is None:
            cap = int(self.lib.nbody_deltas_bound(int(rows.shape[0]), _ptr(rows), 1 if self._dtype == np.float64 else 0))
        cap = int(cap)
        buf = np.zeros(max(cap, 1), np.uint8)
        offsets = np.zeros(rows.shape[0] + 1, np.uint64)
        size, step = _sz(0), C.c_uint64(0)
        name = "nbody_deltas_" + self._prefix[len("nbody_"):]
        flags = (DELTAS_TRACERS if tracers else 0) | (DELTAS_KEY if key else 0)
        rc = getattr(self.lib, name)(self.h, flags, _ptr(buf) if cap else None, cap, C.byref(size), _ptr(offsets), C.byref(step))
        if rc != OK:
            err = self._err(rc)
            err.needed = size.value
            raise err
        return buf[:size.value], offsets, step.value


class EnsembleHandle(_EnsembleHandleBase):
    """nbody_ensemble_*: float32 worlds."""
    _prefix, _suffix, _dtype = "nbody_ensemble", "_f32", np.float32


class Ensemble64Handle(_EnsembleHandleBase):
    """nbody_ensemble64_*: float64 worlds, the sibling of EnsembleHandle."""
    _prefix, _suffix, _dtype = "nbody_ensemble64", "", np.float64


class RaggedHandle(_EnsembleHandleBase):
    """nbody_ragged_*: float32 worlds of different sizes, their rows one after another in world order."""
    _prefix, _suffix, _dtype = "nbody_ragged", "_f32", np.float32

    @property
    def shape(self):
        """(worlds, rows of all worlds together) of the current upload; (0, 0) before one."""
        return int(self._call("_num_worlds")), int(self._call("_num_rows"))

    @property
    def sizes(self):
        """The bodies of every world, int64[worlds]."""
        out = np.zeros(self.shape[0], np.int64)
        self._check(self._call("_sizes", _ptr(out)))
        return out

    def upload(self, sizes, pos, vel, weight):
        """sizes int64[worlds]; pos, vel [rows, 2]; weight uint32[rows] or None."""
        sizes = np.ascontiguousarray(sizes, dtype=np.int64)
        self._check(self._call("_upload" + self._suffix, int(sizes.shape[0]), _ptr(sizes), _ptr(pos), _ptr(vel), _ptr(weight)))

    def download(self):
        rows = self.shape[1]
        pos, vel = np.zeros((rows, 2), self._dtype), np.zeros((rows, 2), self._dtype)
        self._check(self._call("_download" + self._suffix, _ptr(pos), _ptr(vel)))
        return pos, vel

    def accel(self):
        acc = np.zeros((self.shape[1], 2), self._dtype)
        self._check(self._call("_accel" + self._suffix, _ptr(acc)))
        return acc

    def _delta_rows(self, tracers):
        sizes = self.sizes   # (a handle with tracers: the sizes and the counts)
        bodies, counts = sizes if isinstance(sizes, tuple) else (sizes, np.zeros_like(sizes))
        return np.ascontiguousarray(counts if tracers else bodies, dtype=np.int64)


class Ragged64Handle(RaggedHandle):
    """nbody_ragged64_*: float64 worlds of different sizes, the sibling of RaggedHandle."""
    _prefix, _suffix, _dtype = "nbody_ragged64", "", np.float64


class _TracerCalls:
    """The tracer calls of a restricted handle, beside the bodies' calls of the ensemble handle it is mixed into: m tracers per
    world in arrays of the handle's `_dtype`, the typed C calls with its `_suffix`."""
    _frames_tracers = True

    @property
    def n_tracers(self):
        """Tracers per world; 0 without any."""
        return int(self._call("_num_tracers"))

    def upload_tracers(self, n_worlds, n_tracers, pos, vel):
        """pos, vel [n_worlds, n_tracers, 2] of the handle's dtype, contiguous; n_tracers == 0 removes the tracers."""
        self._check(self._call("_tracers_upload" + self._suffix, int(n_worlds), int(n_tracers), _ptr(pos), _ptr(vel)))

    def download_tracers(self):
        b, m = self.shape[0], self.n_tracers
        pos, vel = np.zeros((b, m, 2), self._dtype), np.zeros((b, m, 2), self._dtype)
        self._check(self._call("_tracers_download" + self._suffix, _ptr(pos), _ptr(vel)))
        return pos, vel

    def tracers_accel(self):
        acc = np.zeros((self.shape[0], self.n_tracers, 2), self._dtype)
        self._check(self._call("_tracers_accel" + self._suffix, _ptr(acc)))
        return acc


class RestrictedHandle(_TracerCalls, EnsembleHandle):
    """nbody_restricted_*: float32 worlds of one size with m tracers each; the bodies' calls are EnsembleHandle's."""
    _prefix = "nbody_restricted"


class Restricted64Handle(_TracerCalls, Ensemble64Handle):
    """nbody_restricted64_*: float64 worlds of one size with m tracers each, the sibling of RestrictedHandle; the bodies' calls
    are Ensemble64Handle's."""
    _prefix = "nbody_restricted64"


class RRHandle(RaggedHandle):
    """nbody_rr_*: float32 worlds of different sizes, each with tracers of its own; the bodies' calls are RaggedHandle's.  The
    tracer rows of all worlds come one after another in world order, as the body rows do."""
    _prefix = "nbody_rr"
    _frames_tracers = True

    @property
    def n_tracer_rows(self):
        """The tracers of all worlds together; 0 without any."""
        return int(self._call("_num_tracer_rows"))

    @property
    def sizes(self):
        """(the bodies of every world, the tracers of every world), int64[worlds] each."""
        b = self.shape[0]
        bodies, tracers = np.zeros(b, np.int64), np.zeros(b, np.int64)
        self._check(self._call("_sizes", _ptr(bodies), _ptr(tracers)))
        return bodies, tracers

    def upload_tracers(self, counts, pos, vel):
        """counts int64[worlds]; pos, vel [tracer rows, 2] of the handle's dtype, contiguous (None where every count is 0: no
        tracers)."""
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        self._check(self._call("_tracers_upload" + self._suffix, int(counts.shape[0]), _ptr(counts), _ptr(pos), _ptr(vel)))

    def download_tracers(self):
        rows = self.n_tracer_rows
        pos, vel = np.zeros((rows, 2), self._dtype), np.zeros((rows, 2), self._dtype)
        self._check(self._call("_tracers_download" + self._suffix, _ptr(pos), _ptr(vel)))
        return pos, vel

    def tracers_accel(self):
        acc = np.zeros((self.n_tracer_rows, 2), self._dtype)
        self._check(self._call("_tracers_accel" + self._suffix, _ptr(acc)))
        return acc


class RR64Handle(RRHandle):
    """nbody_rr64_*: float64 worlds of different sizes, each with tracers of its own, the sibling of RRHandle."""
    _prefix, _suffix, _dtype = "nbody_rr64", "", np.float64


RAGGED_MAX_LAUNCHES = 6
RR_MAX_LAUNCHES = 12


def ragged_plan(sizes, f64=False):
    """nbody_ragged_plan (f64: nbody_ragged64_plan) of these sizes (pure host code) -> (launch_of_world int32[worlds],
    first_block_of_world int64[worlds], lds_bytes int32[launches], blocks int64[launches]); NBodyError(ERR_INVALID) for sizes
    outside the limits."""
    lib = load()
    prefix = "nbody_ragged64" if f64 else "nbody_ragged"
    sizes = np.ascontiguousarray(sizes, dtype=np.int64)
    b = int(sizes.shape[0])
    launch, first = np.zeros(b, np.int32), np.zeros(b, np.int64)
    lds, blocks = np.zeros(RAGGED_MAX_LAUNCHES, np.int32), np.zeros(RAGGED_MAX_LAUNCHES, np.int64)
    n = _i32(0)
    rc = getattr(lib, prefix + "_plan")(b, _ptr(sizes), _ptr(launch), _ptr(first), C.byref(n), _ptr(lds), _ptr(blocks))
    if rc != OK:
        msg = getattr(lib, prefix + "_last_error")(None)
        raise NBodyError(rc, msg.decode() if msg else "")
    return launch, first, lds[:n.value].copy(), blocks[:n.value].copy()


RESIDENT_MAX_BODIES, RESIDENT_STEPS_PER_LAUNCH = 256, 1024   # NBODY_RESIDENT_* of include/nbody_ensemble.h


def resident_plan(sizes, steps, n_steps, is_f64):
    """nbody_resident_plan (pure host code): sizes int64[n_worlds], steps int32[n_worlds] or None, contiguous -> (n_launches,
    lds_bytes) of nbody_resident_<handle> with these arguments; ValueError where the library refuses them."""
    lib = load()
    launches, lds = C.c_int32(-1), C.c_int32(-1)
    rc = lib.nbody_resident_plan(int(sizes.shape[0]), sizes.ctypes.data_as(C.POINTER(_i64)),
                                 None if steps is None else steps.ctypes.data_as(C.POINTER(C.c_int32)), int(n_steps), 1 if is_f64 else 0,
                                 C.byref(launches), C.byref(lds))
    if rc != OK:
        raise ValueError(f"resident_plan: refused ({sizes.shape[0]} worlds, n_steps = {n_steps}): a world of more than "
                         f"{RESIDENT_MAX_BODIES} bodies (or none), or a steps[k] outside 0 .. n_steps")
    return int(launches.value), int(lds.value)


def wsweep_plan(n_worlds, steps, n_steps, stride, resume=False):
    """nbody_wsweep_plan (pure host code): steps, stride int32[n_worlds], contiguous, or None -> (samples_of_world
    int64[n_worlds], n_sampling_launches); ValueError where the library refuses."""
    def typed(a):
        return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    lib = load()
    samples = np.zeros(max(int(n_worlds), 0), np.int64)
    launches = C.c_int64(0)
    rc = lib.nbody_wsweep_plan(int(n_worlds), typed(steps), int(n_steps), typed(stride), WATCH_RESUME if resume else 0, _ptr(samples),
                               C.byref(launches))
    if rc != 0:
        raise ValueError(f"wsweep_plan: refused (n_worlds = {n_worlds}, n_steps = {n_steps}): a steps[k] outside 0 .. n_steps or a stride[k] < 1")
    return samples, int(launches.value)


def rr_plan(sizes, tracer_counts, f64=False):
    """nbody_rr_plan (f64: nbody_rr64_plan) of these sizes and tracer counts (pure host code): the TRACERS' launches of a ragged
    restricted ensemble ->
    (launch_of_world int32[worlds], first_block_of_world int64[worlds], both -1 for a world without tracers, lds_bytes
    int32[launches], blocks int64[launches]); NBodyError(ERR_INVALID) for sizes or counts outside the limits."""
    lib = load()
    prefix = "nbody_rr64" if f64 else "nbody_rr"
    sizes = np.ascontiguousarray(sizes, dtype=np.int64)
    counts = np.ascontiguousarray(tracer_counts, dtype=np.int64)
    b = int(sizes.shape[0])
    if counts.shape != sizes.shape:
        raise ValueError(f"rr_plan: {counts.shape[0]} tracer counts beside {b} sizes")
    launch, first = np.zeros(b, np.int32), np.zeros(b, np.int64)
    lds, blocks = np.zeros(RAGGED_MAX_LAUNCHES, np.int32), np.zeros(RAGGED_MAX_LAUNCHES, np.int64)
    n = _i32(0)
    rc = getattr(lib, prefix + "_plan")(b, _ptr(sizes), _ptr(counts), _ptr(launch), _ptr(first), C.byref(n), _ptr(lds), _ptr(blocks))
    if rc != OK:
        msg = getattr(lib, prefix + "_last_error")(None)
        raise NBodyError(rc, msg.decode() if msg else "")
    return launch, first, lds[:n.value].copy(), blocks[:n.value].copy()


def mass_hint(weight) -> float:
    """The `uniform_mass` argument of the direct step for these weights (include/nbody_hip.h): > 0 all equal,
    < 0 all equal to its magnitude but for at most n/256 bodies, 0 neither."""
    w = np.asarray(weight)
    if w.size == 0:
        return 0.0
    vals, counts = np.unique(w, return_counts=True)
    base = vals[np.argmax(counts)]
    odd = int(w.size - counts.max())
    if base <= 0:
        return 0.0
    if odd == 0:
        return float(base)
    return -float(base) if odd <= w.size // 256 else 0.0


# ---- device-pointer level (raw addresses; used with torch tensors by sharding.py / bench.py)
def direct_workspace_bytes(n_sources: int, n_targets: int) -> int:
    return int(load().nbody_direct_workspace_bytes(int(n_sources), int(n_targets)))


def direct_step_dev(stream, n_sources, pos_all, mass_all, target_begin, n_targets, vel, pos_out, acc_out, delta,
                    clamp, arith, workspace, workspace_bytes, timer: Timer | None = None, uniform_mass: float = 0.0):
    rc = load().nbody_direct_step_dev(_vp(stream), int(n_sources), _vp(pos_all), _vp(mass_all), float(uniform_mass),
                                      int(target_begin),
                                      int(n_targets), _vp(vel) if vel else None, _vp(pos_out) if pos_out else None,
                                      _vp(acc_out) if acc_out else None, float(delta), float(clamp), int(arith),
                                      _vp(workspace), int(workspace_bytes), timer.h if timer else None)
    check(None, rc)


def direct_prep_dev(stream, n_sources, pos_all, mass_all, n_targets_total, n_targets_max, clamp, arith, workspace,
                    workspace_bytes, uniform_mass: float = 0.0):
    """One preparation per step over all positions (hazard scan, near/far split); direct_run_dev per target block."""
    check(None, load().nbody_direct_prep_dev(_vp(stream), int(n_sources), _vp(pos_all), _vp(mass_all), float(uniform_mass),
                                             int(n_targets_total), int(n_targets_max), float(clamp), int(arith),
                                             _vp(workspace), int(workspace_bytes)))


def direct_run_dev(stream, n_sources, pos_all, mass_all, target_begin, n_targets, vel, pos_out, acc_out, delta, clamp,
                   arith, n_targets_total, n_targets_max, workspace, workspace_bytes, timer: Timer | None = None,
                   uniform_mass: float = 0.0):
    rc = load().nbody_direct_run_dev(_vp(stream), int(n_sources), _vp(pos_all), _vp(mass_all), float(uniform_mass),
                                     int(target_begin), int(n_targets), _vp(vel) if vel else None,
                                     _vp(pos_out) if pos_out else None, _vp(acc_out) if acc_out else None, float(delta),
                                     float(clamp), int(arith), int(n_targets_total), int(n_targets_max), _vp(workspace),
                                     int(workspace_bytes), timer.h if timer else None)
    check(None, rc)


def direct_workspace_peek(stream, workspace):
    """-> (hazard, fallback, n_near, state) of the last direct_step_dev on that workspace."""
    out = (C.c_int32 * 4)()
    check(None, load().nbody_direct_workspace_peek(_vp(stream), _vp(workspace), C.byref(out)))
    return tuple(out)


def weights_to_mass_dev(stream, n, weight_u32, mass_f32):
    check(None, load().nbody_weights_to_mass_dev(_vp(stream), int(n), _vp(weight_u32), _vp(mass_f32)))
