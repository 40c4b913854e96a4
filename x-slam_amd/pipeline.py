"""ctypes binding of the host orchestrator's C ABI (include/xslam_amd_pipeline.h,
libxslam_host.so built from x-slam_amd/host/).  The orchestrator itself is C++
(KinectFusionReconstruction, mirroring the reference class); this module only lets Python
callers — bench.py and the parity tests — drive it.  No CPU fallback: a missing library is an
ImportError."""
import collections
import ctypes as C
import os

import numpy as np

from . import capi  # loads libxslam_hip.so first (libxslam_host.so links against it)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libxslam_host.so")
if not os.path.exists(LIB_PATH):
    raise ImportError(f"{LIB_PATH} not found: run __graft_entry__.build() (make -C x-slam_amd/host). There is no CPU fallback.")
_lib = C.CDLL(LIB_PATH)

_vp, _sz = C.c_void_p, C.c_size_t
_f32p, _f64p, _i32p = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int)
COLLECTIVE_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_void_p, C.c_long)  # (user, op, dev_ptr, count)


class AlignSearchOpts(C.Structure):
    """xs_align_search_opts (include/xslam_amd_pipeline.h)"""
    _fields_ = [("struct_bytes", C.c_uint), ("candidates", C.c_int), ("keep", C.c_int), ("rounds", C.c_int), ("stride", C.c_int), ("iterations", C.c_int),
                ("min_weight", C.c_int), ("user_n", C.c_int), ("box_t", C.c_double), ("refine_t", C.c_double), ("refine_r", C.c_double),
                ("damping", C.c_double), ("max_residual", C.c_double), ("user_T16xN", C.POINTER(C.c_double))]


# what the three diff calls share behind T16: min_weight, lo, hi, cell, min_size, capacity, two record buffers with their counts, counts3, two dense masks
_DIFF_TAIL = [C.c_int, C.c_float, C.c_float, C.c_int, C.c_ulonglong, C.c_int, C.POINTER(C.c_uint64), _i32p, C.POINTER(C.c_uint64), _i32p,
              C.POINTER(C.c_ulonglong), C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]

# what the four render calls share behind their source: views, c2v, complex_poses, intr4, rows, cols, opts, five outputs, on_device
_RENDER_TAIL = [C.c_int, _f32p, C.c_int, _f32p, C.c_int, C.c_int, C.POINTER(capi.RenderOpts), _vp, _vp, _vp, _vp, _vp, C.c_int]

# what the five sample calls share behind their source: min_weight, five outputs, on_device
_SAMPLE_TAIL = [C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int]
_SAMPLE_POINTS = [C.c_longlong, _vp, _f64p]   # n, points, T16

# what the three register calls share behind their source: n, points, on_device, T16xN, N, iterations, damping, min_weight, max_residual, T16_out, report7, history
_REGISTER_TAIL = [C.c_longlong, _vp, C.c_int, _f64p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_float, _f64p, _f64p, _f64p]

class RegisterSearchOpts(C.Structure):
    """xs_register_search_opts (include/xslam_amd_pipeline.h): xs_align_search_opts' fields"""
    _fields_ = AlignSearchOpts._fields_


# what the three point-score calls share behind their source: n, points, on_device, P, T16xP, stride, min_weight, max_residual, out2xP
_POINT_SCORE_TAIL = [C.c_longlong, _vp, C.c_int, C.c_int, _f64p, C.c_int, C.c_int, C.c_float, _f64p]
# and the three global registrations: n, points, on_device, opts, T16_out, report12
_REGISTER_GLOBAL_TAIL = [C.c_longlong, _vp, C.c_int, C.POINTER(RegisterSearchOpts), _f64p, _f64p]

_SIGS = {
    "xs_kf_register_search_defaults": (None, [_vp, C.POINTER(RegisterSearchOpts)]),
    "xs_kf_score_point_transforms": (C.c_int, [_vp] + _POINT_SCORE_TAIL),
    "xs_kf_score_point_transforms_map": (C.c_int, [_vp, _vp] + _POINT_SCORE_TAIL),
    "xs_kf_score_point_transforms_checkpoint": (C.c_int, [_vp, C.c_char_p] + _POINT_SCORE_TAIL),
    "xs_kf_register_points_global": (C.c_int, [_vp] + _REGISTER_GLOBAL_TAIL),
    "xs_kf_register_points_global_map": (C.c_int, [_vp, _vp] + _REGISTER_GLOBAL_TAIL),
    "xs_kf_register_points_global_checkpoint": (C.c_int, [_vp, C.c_char_p] + _REGISTER_GLOBAL_TAIL),
    "xs_host_points_centroid": (C.c_int, [_f32p, C.c_longlong, C.c_int, _f64p]),
    "xs_kf_register_points": (C.c_int, [_vp] + _REGISTER_TAIL),
    "xs_kf_register_map": (C.c_int, [_vp, _vp] + _REGISTER_TAIL),
    "xs_kf_register_checkpoint": (C.c_int, [_vp, C.c_char_p] + _REGISTER_TAIL),
    "xs_host_register_step": (C.c_int, [_f64p, C.c_double, _f64p]),
    "xs_kf_fuse_points": (C.c_int, [_vp, C.c_longlong, _vp, C.c_int, _f64p, _f32p, C.c_float, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_ulonglong)]),
    "xs_kf_release_fuse_scratch": (None, [_vp]),
    "xs_kf_sample_points": (C.c_int, [_vp] + _SAMPLE_POINTS + _SAMPLE_TAIL),
    "xs_kf_sample_volume": (C.c_int, [_vp, _vp, _vp, _vp, _sz, _i32p, C.c_float, C.c_float] + _SAMPLE_POINTS + _SAMPLE_TAIL),
    "xs_kf_sample_map": (C.c_int, [_vp, _vp] + _SAMPLE_POINTS + _SAMPLE_TAIL),
    "xs_kf_sample_checkpoint": (C.c_int, [_vp, C.c_char_p] + _SAMPLE_POINTS + _SAMPLE_TAIL),
    "xs_kf_frame_residuals": (C.c_int, [_vp, _vp, _sz, _f32p, C.c_int, _f32p, C.c_int, C.c_int] + _SAMPLE_TAIL),
    "xs_host_sample_compose": (C.c_int, [_f64p, _f64p, _f64p]),
    "xs_kf_render_views": (C.c_int, [_vp] + _RENDER_TAIL),
    "xs_kf_render_volume": (C.c_int, [_vp, _vp, _vp, _sz, _i32p, C.c_float, C.c_float] + _RENDER_TAIL),
    "xs_kf_render_map": (C.c_int, [_vp, _vp] + _RENDER_TAIL),
    "xs_kf_render_checkpoint": (C.c_int, [_vp, C.c_char_p] + _RENDER_TAIL),
    "xs_kf_create_sharded": (_vp, [C.c_char_p, C.c_int, C.c_int, COLLECTIVE_CB, _vp]),
    "xs_kf_shard_planes": (None, [_vp, _i32p, _i32p]),
    "xs_host_double_complex_table": (C.c_int, [C.c_int, C.c_long, _f32p, _f32p, _f32p]),
    "xs_host_complex_table": (C.c_int, [C.c_int, C.c_long, _f32p, _f32p, _f32p]),
    "xs_flat_yaml_get": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]),
    "xs_kf_set_stream": (None, [_vp]),
    "xs_kf_create": (_vp, [C.c_char_p]),
    "xs_kf_destroy": (None, [_vp]),
    "xs_kf_set_gt_poses": (None, [_vp, C.c_int, _f32p]),
    "xs_kf_process_frame": (C.c_int, [_vp, _vp, _sz]),
    "xs_kf_process_frame_host": (C.c_int, [_vp, _vp]),
    "xs_kf_ingest_buffer": (_vp, [_vp]),
    "xs_kf_get_camera2volume": (None, [_vp, _f32p]),
    "xs_kf_gauss_newton_terms": (C.c_int, [_vp, _vp, _sz, _f32p, _f64p]),
    "xs_kf_relocalize": (C.c_int, [_vp, _vp, _sz, _f32p, C.c_int, C.c_float, _f64p]),
    "xs_kf_relocalize_batch": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), _sz, _f32p, C.c_int, C.c_float, _f64p, _i32p]),
    "xs_kf_pose_hessian_terms": (C.c_int, [_vp, _vp, _sz, _f32p, _f64p]),
    "xs_kf_relocalize_newton": (C.c_int, [_vp, _vp, _sz, _f32p, C.c_int, C.c_float, _f64p, _i32p]),
    "xs_kf_relocalize_newton_batch": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), _sz, _f32p, C.c_int, C.c_float, _f64p, _i32p, _i32p]),
    "xs_host_newton_seeded_poses": (C.c_int, [_f32p, _f32p, _f32p]),
    "xs_host_newton_step": (C.c_int, [_f64p, C.c_double, _f32p]),
    "xs_kf_score_poses": (C.c_int, [_vp, _vp, _sz, C.c_int, _f32p, _f64p]),
    "xs_kf_relocalize_global": (C.c_int, [_vp, _vp, _sz, C.c_int, _f32p, C.c_int, C.c_int, C.c_float, _f32p, _f64p]),
    "xs_kf_score_views": (C.c_int, [_vp, C.c_int, _f32p, C.POINTER(capi.ViewOpts), C.c_int, C.POINTER(C.c_uint)]),
    "xs_kf_next_best_view": (C.c_int, [_vp, C.c_int, _f32p, C.POINTER(capi.ViewOpts), C.c_int, C.c_uint, C.POINTER(C.c_uint)]),
    "xs_kf_clearance_field": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint16)]),
    "xs_kf_reachable": (C.c_int, [_vp, _f32p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, _f32p, C.POINTER(C.c_ubyte), C.POINTER(C.c_uint16)]),
    "xs_kf_next_reachable_view": (C.c_int, [_vp, C.c_int, _f32p, C.POINTER(capi.ViewOpts), C.c_int, C.c_uint, C.POINTER(C.c_uint), C.c_float, C.c_int,
                                            C.c_int, C.POINTER(C.c_ubyte)]),
    "xs_kf_travel": (C.c_int, [_vp, _f32p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _f32p, C.POINTER(C.c_ubyte), C.POINTER(C.c_uint16),
                               C.POINTER(C.c_uint16)]),
    "xs_kf_path_to": (C.c_int, [_vp, _f32p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_float, _f32p, C.c_int, _i32p, _f32p, _i32p]),
    "xs_kf_next_view_by_travel": (C.c_int, [_vp, C.c_int, _f32p, C.POINTER(capi.ViewOpts), C.c_int, C.c_uint, C.POINTER(C.c_uint), C.c_float, C.c_int,
                                            C.c_int, C.c_float, C.c_float, C.POINTER(C.c_uint16)]),
    "xs_kf_frontiers": (C.c_int, [_vp, C.c_int, C.c_ulonglong, C.c_int, C.c_int, C.POINTER(C.c_uint64), _i32p]),
    "xs_kf_propose_views": (C.c_int, [_vp, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulonglong, C.c_int, C.c_float, C.c_int, C.c_int, _f32p, _i32p,
                                      _i32p]),
    "xs_kf_relocalization_index_voxels": (C.c_longlong, [_vp]),
    "xs_kf_export_point_cloud": (C.c_longlong, [_vp, C.c_int, _f32p, _f32p]),
    "xs_kf_export_ply": (C.c_longlong, [_vp, C.c_int, C.c_char_p]),
    "xs_kf_export_mesh": (C.c_longlong, [_vp, C.c_int, C.c_longlong, C.c_longlong, _f32p, _f32p, _f32p, C.POINTER(C.c_uint64), _i32p,
                                         C.POINTER(C.c_longlong), _i32p]),
    "xs_kf_export_mesh_ply": (C.c_longlong, [_vp, C.c_char_p]),
    "xs_kf_synchronize": (None, [_vp]),
    "xs_kf_frame_id": (C.c_int, [_vp]),
    "xs_kf_num_poses": (C.c_int, [_vp]),
    "xs_kf_get_world2camera": (None, [_vp, C.c_int, _f32p]),
    "xs_kf_tranc_dist": (C.c_float, [_vp]),
    "xs_kf_last_updated_voxels": (C.c_longlong, [_vp]),
    "xs_kf_last_raycast_hits": (C.c_longlong, [_vp]),
    "xs_kf_icp_log": (C.c_int, [_vp, _f64p, C.c_int]),
    "xs_kf_download_volume": (C.c_int, [_vp, _f32p, _i32p, _f32p]),
    "xs_kf_download_map": (C.c_int, [_vp, C.c_int, C.c_int, _f32p]),
    "xs_kf_volume_ptr": (_vp, [_vp, C.c_int, C.POINTER(_sz)]),
    "xs_kf_set_profiling": (None, [_vp, C.c_int]),
    "xs_kf_stage_times": (None, [_vp, _f64p, C.POINTER(C.c_longlong)]),
    "xs_kf_reset_stage_times": (None, [_vp]),
    "xs_kf_icp_iteration_times": (None, [_vp, _f64p, C.POINTER(C.c_longlong)]),
    "xs_kf_tail_host_times": (None, [_vp, _f64p, C.POINTER(C.c_longlong)]),
    "xs_kf_set_gn_post_pose": (None, [_vp, C.c_int]),
    "xs_kf_gn_poll_times": (None, [_vp, _f64p, C.POINTER(C.c_longlong), C.c_int]),
    "xs_kf_gn_times": (None, [_vp, _f64p, C.POINTER(C.c_longlong), _f64p, C.POINTER(C.c_longlong), C.c_int]),
    "xs_kf_debug_set_icp_sequence": (None, [_vp, C.c_ulonglong]),
    "xs_kf_debug_fail_icp_iteration": (None, [_vp, C.c_int]),
    "xs_kf_debug_post_delay": (None, [_vp, C.c_int, C.c_int]),
    "xs_kf_composite_bytes": (C.c_longlong, [_vp]),
    "xs_kf_rebuild_sign_map": (None, [_vp]),
    "xs_kf_hint_next_frame": (None, [_vp, _vp, _sz]),
    "xs_kf_list_cover_counts": (None, [_vp, C.POINTER(C.c_longlong)]),
    "xs_kf_cumulative_counters": (None, [_vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "xs_kf_volume_generation": (C.c_longlong, [_vp]),
    "xs_kf_save_checkpoint": (C.c_int, [_vp, C.c_char_p]),
    "xs_kf_load_checkpoint": (C.c_int, [_vp, C.c_char_p]),
    "xs_kf_save_tsdf_volume": (C.c_int, [_vp, C.c_char_p]),
    "xs_kf_save_checkpoint_sparse": (C.c_int, [_vp, C.c_char_p, C.POINTER(C.c_ulonglong)]),
    "xs_kf_checkpoint_staging_words": (C.c_longlong, [_vp, C.c_ulonglong]),
    "xs_host_checkpoint_info": (C.c_int, [C.c_char_p, _f64p]),
    "xs_kf_reintegrate": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), _sz, _f32p, _f32p, _i32p, _i32p, C.POINTER(C.c_ulonglong)]),
    "xs_kf_merge_volume": (C.c_int, [_vp, _vp, _vp, _vp, _sz, _i32p, C.c_float, C.c_float, _f64p, C.c_int, C.POINTER(C.c_ulonglong)]),
    "xs_kf_merge_map": (C.c_int, [_vp, _vp, _f64p, C.c_int, C.POINTER(C.c_ulonglong)]),
    "xs_kf_merge_checkpoint": (C.c_int, [_vp, C.c_char_p, _f64p, C.c_int, C.POINTER(C.c_ulonglong)]),
    "xs_kf_diff_volume": (C.c_int, [_vp, _vp, _vp, _sz, _i32p, C.c_float, C.c_float, _f64p] + _DIFF_TAIL),
    "xs_kf_diff_map": (C.c_int, [_vp, _vp, _f64p] + _DIFF_TAIL),
    "xs_kf_diff_checkpoint": (C.c_int, [_vp, C.c_char_p, _f64p] + _DIFF_TAIL),
    "xs_host_merge_affine": (C.c_int, [_f64p, C.c_double, C.c_double, _f32p]),
    "xs_host_map_transform": (C.c_int, [_f64p, _f64p, _f64p]),
    "xs_host_merge_tile_box": (C.c_int, [_f32p, _i32p, _i32p, _i32p, _i32p]),
    "xs_kf_align_map": (C.c_int, [_vp, _vp, _f64p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_float, _f64p, _f64p, _f64p]),
    "xs_kf_align_checkpoint": (C.c_int, [_vp, C.c_char_p, _f64p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_float, _f64p, _f64p, _f64p]),
    "xs_host_align_seeded_maps": (C.c_int, [_f64p, C.c_double, C.c_double, _f32p]),
    "xs_host_align_step": (C.c_int, [_f64p, C.c_double, _f64p]),
    "xs_kf_align_search_defaults": (None, [_vp, C.POINTER(AlignSearchOpts)]),
    "xs_kf_score_transforms": (C.c_int, [_vp, _vp, C.c_int, _f64p, C.c_int, C.c_int, C.c_float, _f64p]),
    "xs_kf_score_transforms_checkpoint": (C.c_int, [_vp, C.c_char_p, C.c_int, _f64p, C.c_int, C.c_int, C.c_float, _f64p]),
    "xs_kf_align_map_global": (C.c_int, [_vp, _vp, C.POINTER(AlignSearchOpts), _f64p, _f64p]),
    "xs_kf_align_checkpoint_global": (C.c_int, [_vp, C.c_char_p, C.POINTER(AlignSearchOpts), _f64p, _f64p]),
    "xs_host_align_search_free": (C.c_int, [C.c_int, _f64p, _f64p, C.c_double, _f64p]),
    "xs_host_align_search_around": (C.c_int, [_f64p, _f64p, C.c_double, C.c_double, C.c_int, _f64p]),
    "xs_host_align_search_rank": (C.c_int, [_f64p, C.c_int, C.c_int, _i32p]),
    "xs_host_band_centroid": (C.c_int, [C.POINTER(C.c_uint64), C.c_longlong, C.c_double, _f64p]),
    "xs_refshape_create": (_vp, [C.c_char_p]),
    "xs_refshape_destroy": (None, [_vp]),
    "xs_refshape_process_frame_host": (C.c_int, [_vp, _vp]),
    "xs_refshape_process_frame": (C.c_int, [_vp, _vp, _sz]),
    "xs_refshape_frame_id": (C.c_int, [_vp]),
    "xs_refshape_get_world2camera": (None, [_vp, C.c_int, _f32p]),
    "xs_refshape_download_volume": (C.c_int, [_vp, _f32p, _i32p, _f32p]),
    "xs_refshape_download_map": (C.c_int, [_vp, C.c_int, C.c_int, _f32p]),
    "xs_refshape_icp_log": (C.c_int, [_vp, _f64p, C.c_int]),
    "xs_refshape_hessian": (C.c_int, [_vp, _sz, C.c_int, C.c_int, _f32p, _i32p, C.c_float, _f32p, _f32p, C.c_float, _vp, C.c_int, _f32p, _f32p]),
    "xs_refshape_loss": (C.c_int, [_vp, _sz, C.c_int, C.c_int, _f32p, _i32p, C.c_float, _f32p, _f32p, C.c_float, _vp, C.c_int, _f32p, _f32p]),
}
for _n, (_r, _a) in _SIGS.items():
    _f = getattr(_lib, _n)
    _f.restype, _f.argtypes = _r, _a

STAGES = ("surface", "icp", "scale", "integrate", "raycast", "resize")
MAPS = {"depths_curr": 0, "vmaps_curr": 1, "nmaps_curr": 2, "vmaps_g_prev": 3, "nmaps_g_prev": 4}


def yaml_text(params: dict) -> str:
    """Flat YAML in the reference's format (ICL_traj2.yaml) from a dict of its keys."""
    out = []
    for k, v in params.items():
        if isinstance(v, bool):
            v = "true" if v else "false"
        elif isinstance(v, float):
            v = repr(float(np.float32(v))) if abs(v) < 1e-3 and v != 0 else repr(v)
        out.append(f"{k}: {v}")
    return "\n".join(out) + "\n"


HDC_OPS = {"add": 0, "sub": 1, "mul": 2, "div": 3, "sqrt": 4, "abs": 5, "exp": 6, "log": 7, "sin": 8, "cos": 9, "pow": 10, "f1": 11,
           "conj": 12, "norm": 13, "cmp": 14}


def host_double_complex(op, a, b=None):
    """Elementwise host DoubleComplex op over [n, 4] float32 arrays (CPU; no GPU involved)."""
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 4)
    b = a if b is None else np.ascontiguousarray(b, dtype=np.float32).reshape(-1, 4)
    out = np.empty_like(a)
    rc = _lib.xs_host_double_complex_table(HDC_OPS[op], a.shape[0], a.ctypes.data_as(_f32p), b.ctypes.data_as(_f32p), out.ctypes.data_as(_f32p))
    if rc != 0:
        raise ValueError("bad op")
    return out


def host_complex(op_code, a, b=None):
    """Elementwise complex<float> op of csrc/xs_complex.h compiled for the host, over [n, 2] float32 arrays (CPU)."""
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 2)
    b = a if b is None else np.ascontiguousarray(b, dtype=np.float32).reshape(-1, 2)
    out = np.empty_like(a)
    rc = _lib.xs_host_complex_table(int(op_code), a.shape[0], a.ctypes.data_as(_f32p), b.ctypes.data_as(_f32p), out.ctypes.data_as(_f32p))
    if rc != 0:
        raise ValueError("bad op")
    return out


def host_newton_seeded_poses(c2v):
    """The 21 dual-complex seeded poses of a Newton pass for camera2volume c2v [4, 4, 2]: (R [21, 3, 3, 4], t [21, 3, 4]) float32, pair
    (a, b), a <= b, row-major (CPU; no GPU involved)."""
    m = np.ascontiguousarray(c2v, dtype=np.float32).reshape(32)
    R, t = np.zeros((21, 3, 3, 4), np.float32), np.zeros((21, 3, 4), np.float32)
    _lib.xs_host_newton_seeded_poses(m.ctypes.data_as(_f32p), R.ctypes.data_as(_f32p), t.ctypes.data_as(_f32p))
    return R, t


def host_newton_step(s29, damping, c2v):
    """One Newton step on the 29 scaled sums of pose_hessian: (taken, c2v [4, 4, 2]); not taken (c2v unchanged) when count < 6 or
    H + damping diag(H) is not positive definite (CPU)."""
    s = np.ascontiguousarray(s29, dtype=np.float64).reshape(29)
    m = np.ascontiguousarray(c2v, dtype=np.float32).reshape(32).copy()
    rc = _lib.xs_host_newton_step(s.ctypes.data_as(_f64p), float(damping), m.ctypes.data_as(_f32p))
    return rc == 0, m.reshape(4, 4, 2)


def _real44(m):
    """A real 4 x 4 float64 from a 4 x 4 (real) or 4 x 4 x 2 (re, im: the real parts) pose."""
    a = np.asarray(m, dtype=np.float64)
    if a.shape == (4, 4, 2):
        a = a[..., 0]
    return np.ascontiguousarray(a.reshape(4, 4))


def merge_affine(T, dst_voxel_size, src_voxel_size):
    """xform12 of capi.tsdf_merge (float32 [12]: 3 x 3 row-major, then 3 offsets) from T (real 4 x 4: a point of the destination map's volume
    frame, in metres, to the source map's) and the two voxel sizes: float64 throughout, one rounding at the end (CPU).  ValueError for an
    input that is not finite or a voxel size that is not positive."""
    t = _real44(T)
    out = np.zeros(12, np.float32)
    if _lib.xs_host_merge_affine(t.ctypes.data_as(_f64p), float(dst_voxel_size), float(src_voxel_size), out.ctypes.data_as(_f32p)) != 0:
        raise ValueError("merge_affine: an input is not finite, or a voxel size is not positive")
    return out


def map_transform(c2v_this, c2v_other):
    """T = c2v_other c2v_this^-1 (real 4 x 4 float64) from the real parts of two camera-to-volume poses of one camera frame: the frame's pose in
    this map and, by relocalize_global there, in the other map give the T that merge_map takes (CPU)."""
    a, b = _real44(c2v_this), _real44(c2v_other)
    out = np.zeros((4, 4), np.float64)
    _lib.xs_host_map_transform(a.ctypes.data_as(_f64p), b.ctypes.data_as(_f64p), out.ctypes.data_as(_f64p))
    return out


def align_seeded_maps(T, vs_this, vs_other):
    """The six complex-seeded index maps of one alignment pass (float32 [6, 12, 2]: xform12's entries as (re, im)) from T (real 4 x 4, as
    merge_affine takes it): T_k = (I + i h G_k) T through merge_affine's formula, three translations then three rotations.  The real parts
    are merge_affine's bit for bit (CPU).  ValueError: merge_affine's refusals."""
    t = _real44(T)
    out = np.zeros((6, 12, 2), np.float32)
    if _lib.xs_host_align_seeded_maps(t.ctypes.data_as(_f64p), float(vs_this), float(vs_other), out.ctypes.data_as(_f32p)) != 0:
        raise ValueError("align_seeded_maps: an input is not finite, or a voxel size is not positive")
    return out


def align_step(s29, damping, T):
    """One damped Gauss-Newton step on the 29 scaled sums of an alignment pass: (taken, T [4, 4] float64) with T <- exp(delta) T; not taken
    (T unchanged) when count < 6 or A + damping diag(A) is not positive definite (CPU)."""
    s = np.ascontiguousarray(s29, dtype=np.float64).reshape(29)
    t = _real44(T).copy()
    rc = _lib.xs_host_align_step(s.ctypes.data_as(_f64p), float(damping), t.ctypes.data_as(_f64p))
    return rc == 0, t


def register_step(s29, damping, T):
    """One damped Gauss-Newton step on the 29 sums of capi.register_terms as they stand (no scaling): (taken, T [4, 4] float64) with
    T <- exp(delta) T, delta = (translation, rotation); not taken (T unchanged) when count < 6 or A + damping diag(A) is not positive
    definite (CPU)."""
    s = np.ascontiguousarray(s29, dtype=np.float64).reshape(29)
    t = _real44(T).copy()
    rc = _lib.xs_host_register_step(s.ctypes.data_as(_f64p), float(damping), t.ctypes.data_as(_f64p))
    return rc == 0, t


def transform_candidates_free(n, centroid_this, centroid_other, box_t):
    """n transforms [n, 4, 4] float64 that cover SO(3) with no guess (xs_host_align_search_free, CPU): candidate i's rotation is Shoemake's
    uniform-quaternion map at the Halton point (i + 1; bases 2, 3, 5), its translation takes this map's centroid onto the other's, plus
    box_t (2 halton(i + 1; 7, 11, 13) - 1) metres.  ValueError: n < 1, an input that is not finite, a negative box."""
    a, b = (np.ascontiguousarray(c, np.float64).reshape(3) for c in (centroid_this, centroid_other))
    out = np.zeros((max(int(n), 0), 4, 4), np.float64)
    if _lib.xs_host_align_search_free(int(n), a.ctypes.data_as(_f64p), b.ctypes.data_as(_f64p), float(box_t), out.ctypes.data_as(_f64p)) != 0:
        raise ValueError("transform_candidates_free: n < 1, an input that is not finite or a negative box")
    return out


def transform_candidates_around(T, pivot, box_t, box_r, n):
    """n transforms [n, 4, 4] float64 about T (xs_host_align_search_around, CPU): entry 0 is T itself; entry i >= 1 turns T by
    exp(box_r u[3:6]) about the image of `pivot` under T and shifts it by box_t u[0:3], u = 2 halton(i; 2, 3, 5, 7, 11, 13) - 1.
    ValueError: n < 1, an input that is not finite, a negative box."""
    t, p = _real44(T), np.ascontiguousarray(pivot, np.float64).reshape(3)
    out = np.zeros((max(int(n), 0), 4, 4), np.float64)
    if _lib.xs_host_align_search_around(t.ctypes.data_as(_f64p), p.ctypes.data_as(_f64p), float(box_t), float(box_r), int(n), out.ctypes.data_as(_f64p)) != 0:
        raise ValueError("transform_candidates_around: n < 1, an input that is not finite or a negative box")
    return out


def transform_rank(out2xP, keep):
    """The min(keep, P) indices of out2xP [P, 2] ({sum r^2, count}) with the highest S = count - sum r^2, best first, ties to the lower
    index (xs_host_align_search_rank, CPU)."""
    o = np.ascontiguousarray(out2xP, np.float64).reshape(-1, 2)
    idx = np.zeros(max(min(int(keep), o.shape[0]), 1), np.int32)
    n = _lib.xs_host_align_search_rank(o.ctypes.data_as(_f64p), o.shape[0], int(keep), idx.ctypes.data_as(_i32p))
    return idx[:n].copy()


def band_centroid(keys, voxel_size):
    """The centroid [3] (metres) of the voxel centres of packed band keys (x | y << 21 | z << 42): exact integer sums, then (sum / count + 0.5)
    voxel_size (xs_host_band_centroid, CPU).  ValueError for no key."""
    k = np.ascontiguousarray(keys).view(np.uint64).reshape(-1)
    out = np.zeros(3, np.float64)
    if _lib.xs_host_band_centroid(k.ctypes.data_as(C.POINTER(C.c_uint64)), k.size, float(voxel_size), out.ctypes.data_as(_f64p)) != 0:
        raise ValueError("band_centroid: no key")
    return out


def points_centroid(points, stride=1):
    """The centroid [3] float64 of every stride-th point of a host cloud [N, 3] float32: each axis added in double in index order, divided by
    the count (xs_host_points_centroid, CPU): the cloud centroid register_points_global matches to the map's.  ValueError for no point or
    stride < 1."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    out = np.zeros(3, np.float64)
    if _lib.xs_host_points_centroid(p.ctypes.data_as(_f32p), p.shape[0], int(stride), out.ctypes.data_as(_f64p)) != 0:
        raise ValueError("points_centroid: no point, or stride < 1")
    return out


def merge_tile_box(xform12, lo, hi, src_res):
    """The merge kernel's cull box (CPU): (lo [3], hi [3]) inclusive source voxel indices that contain every source voxel a destination voxel
    of the tile lo .. hi (inclusive) reads, or None when no voxel of the tile falls inside the source."""
    m = np.ascontiguousarray(xform12, np.float32).reshape(12)
    l, h, s = (np.ascontiguousarray(a, np.int32).reshape(3) for a in (lo, hi, src_res))
    box = np.zeros(6, np.int32)
    rc = _lib.xs_host_merge_tile_box(m.ctypes.data_as(_f32p), l.ctypes.data_as(_i32p), h.ctypes.data_as(_i32p), s.ctypes.data_as(_i32p), box.ctypes.data_as(_i32p))
    return (box[:3].copy(), box[3:].copy()) if rc == 1 else None


CHECKPOINT_ERRORS = ("ok", "magic", "geometry", "brick_edge", "reserved", "brick_grid", "poses", "class_byte", "payload_words", "length")


def checkpoint_info(path):
    """What a checkpoint file of either format holds (CPU; no payload is read): a dict with version (2: dense XSTSDF2, 3: brick-sparse XSTSDF3),
    valid (the format's full validation: header fields, every class byte, the sum of the words per class, the exact file length), error (one of
    CHECKPOINT_ERRORS), res, voxel_size, tranc_dist, frame_id, n_poses, planes (zs0, zs1), shard (rank, count), file_bytes, payload_words and,
    for version 3, brick_edge, brick_grid, bricks and classes (bricks per class 0 .. 7).  ValueError for a file that is neither."""
    o = np.zeros(32, np.float64)
    if _lib.xs_host_checkpoint_info(str(path).encode(), o.ctypes.data_as(_f64p)) != 0:
        raise ValueError(f"checkpoint_info: {path} is not a checkpoint file")
    i = lambda k: int(o[k])
    info = dict(version=i(0), valid=bool(o[1]), error=CHECKPOINT_ERRORS[i(28)], res=(i(2), i(3), i(4)), voxel_size=float(np.float32(o[5])),
                tranc_dist=float(np.float32(o[6])), frame_id=i(7), n_poses=i(8), planes=(i(9), i(10)), shard=(i(11), i(12)), file_bytes=i(27),
                payload_words=i(26))
    if info["version"] == 3:
        info.update(brick_edge=i(13), brick_grid=(i(14), i(15), i(16)), bricks=i(17), classes=[i(18 + c) for c in range(8)])
    return info


def _halton(i, base):
    """The radical inverse of the integer i >= 1 in `base` (float64)."""
    f, r = 1.0, 0.0
    while i > 0:
        f /= base
        r += f * (i % base)
        i //= base
    return r


def _se3_exp(xi):
    """The exponential of the real twist (v, omega) as a 4 x 4 matrix, float64."""
    v, w = np.asarray(xi[:3], np.float64), np.asarray(xi[3:], np.float64)
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        R, V = np.eye(3) + K, np.eye(3) + K
    else:
        R = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K
        V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * K + (th - np.sin(th)) / th ** 3 * K @ K
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, V @ v
    return T


POSE_CANDIDATE_PRIMES = (2, 3, 5, 7, 11, 13)


def pose_candidates(center_c2v, box_t, box_r, n):
    """n camera2volume hypotheses [n, 4, 4, 2] float32 (zero imaginary parts) around center_c2v ([4, 4, 2] or real [4, 4]) for
    KinectFusion.relocalize_global: candidate i = center @ se3Exp(twist_i), a camera-frame move by the twist
    (u[:3] * box_t metres, u[3:] * box_r radians) with u_j = 2 halton(i + 1, prime_j) - 1 in (-1, 1), primes 2, 3, 5, 7, 11, 13 — a
    low-discrepancy cover of the box, the same for every call (CPU, numpy)."""
    c = np.asarray(center_c2v, np.float64)
    c = c[..., 0] if c.ndim == 3 else c
    assert c.shape == (4, 4)
    out = np.zeros((int(n), 4, 4, 2), np.float32)
    for i in range(int(n)):
        u = np.array([2.0 * _halton(i + 1, b) - 1.0 for b in POSE_CANDIDATE_PRIMES])
        out[i, ..., 0] = c @ _se3_exp(np.concatenate([u[:3] * float(box_t), u[3:] * float(box_r)]))
    return out


def flat_yaml_get(text, key):
    buf = C.create_string_buffer(1024)
    n = _lib.xs_flat_yaml_get(text.encode(), key.encode(), buf, 1024)
    return None if n < 0 else buf.value.decode()


def set_stream(stream):
    _lib.xs_kf_set_stream(None if stream is None else (stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)))


class Mesh(collections.namedtuple("Mesh", "vertices vertex_im normals triangles edge_keys")):
    """A triangle mesh of the TSDF (KinectFusion.export_mesh): numpy arrays, vertices in ascending edge key."""


class MapDiff(collections.namedtuple("MapDiff", "counts only_this only_other masks")):
    """What differs between two maps (KinectFusion.diff_map): counts, a dict of compared, only_this and only_other voxels; only_this and
    only_other, the clusters of each class as structured arrays of KinectFusion.FRONTIER_DTYPE; masks, the pair (only_this, only_other) of
    uint8 [Z, Y, X] or None."""


class RenderedViews(collections.namedtuple("RenderedViews", "depth depth_u16 normal shade counts")):
    """What KinectFusion.render_views returns for P views of rows x cols pixels: depth float32 [P, rows, cols] (metres along the camera's z, 0 without
    a hit), depth_u16 uint16 [P, rows, cols] (millimetres, what process_frame and relocalize take), normal float32 [P, 3, rows, cols] (volume
    frame, pointing into free space, NaN without one), shade uint8 [P, rows, cols] (headlight shading, 0 without a normal) and counts uint32
    [P, 4] = {hit, backface, rejected, none} rays.  An output that was not asked for is None."""


class MapSamples(collections.namedtuple("MapSamples", "status value dvalue gradient counts")):
    """What KinectFusion.sample returns for N points: status uint8 [N] (capi.SAMPLE_OUTSIDE 0, SAMPLE_UNSEEN 1, SAMPLE_OK 2), value float32 [N] (the
    trilinear TSDF in units of the truncation distance, NaN where the status is not OK), dvalue float32 [N] (the grad volume interpolated the
    same way), gradient float32 [N, 3] (value per metre, NaN where one of its six samples is refused) and counts uint64 [4] = {outside, unseen, ok,
    no_depth} (int64 as a torch tensor).  An output that was not asked for is None."""


class FrameResiduals(collections.namedtuple("FrameResiduals", "status value dvalue gradient counts")):
    """What KinectFusion.frame_residuals returns: MapSamples' fields as images, status and the floats [rows, cols], gradient [3, rows, cols]; a pixel
    without a usable depth has status capi.SAMPLE_NO_DEPTH (3)."""


def sample_compose(T_a2v, T_p2a):
    """T = T_a2v T_p2a (real 4 x 4, float64) for KinectFusion.sample: the points are in a frame P whose pose in frame A is T_p2a, and T_a2v takes A to
    the volume (CPU)."""
    a, b, out = _real44(T_a2v), _real44(T_p2a), np.zeros(16, np.float64)
    if _lib.xs_host_sample_compose(a.ctypes.data_as(_f64p), b.ctypes.data_as(_f64p), out.ctypes.data_as(_f64p)) != 0:
        raise ValueError("sample_compose: two 4 x 4 matrices are needed")
    return out.reshape(4, 4)


def save_view_pgm(path, shade):
    """One rendered image (uint8 [rows, cols], e.g. RenderedViews.shade[p]) as a binary P5 file."""
    a = shade.cpu().numpy() if hasattr(shade, "cpu") else np.asarray(shade)
    if a.ndim != 2 or a.dtype != np.uint8:
        raise ValueError("save_view_pgm: a uint8 image [rows, cols] is needed")
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (a.shape[1], a.shape[0]))
        f.write(np.ascontiguousarray(a).tobytes())


class KinectFusion:
    """Handle to a C++ KinectFusionReconstruction."""

    def __init__(self, params, gt_poses=None):
        text = params if isinstance(params, str) else yaml_text(params)
        self.cfg = {}
        for line in text.splitlines():
            if ":" in line:
                k, v = line.split(":", 1)
                self.cfg[k.strip()] = v.split("#")[0].strip()
        self.h = _lib.xs_kf_create(text.encode())
        if not self.h:
            raise ValueError("xs_kf_create failed (missing config key, or a retired one set?)")
        self.res = [int(self.cfg[f"tsdf_size_{a}"]) for a in "xyz"]
        self.width, self.height = int(self.cfg["depth_width"]), int(self.cfg["depth_height"])
        if gt_poses is not None:
            g = np.ascontiguousarray(gt_poses, dtype=np.float32).reshape(-1, 32)
            _lib.xs_kf_set_gt_poses(self.h, g.shape[0], g.ctypes.data_as(_f32p))

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.xs_kf_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def process_frame(self, depth_dev, step_bytes=None):
        """depth_dev: torch int16/uint16 CUDA tensor [H, W] (u16 millimetres) or a raw device address."""
        ptr = depth_dev if isinstance(depth_dev, int) else depth_dev.data_ptr()
        step = step_bytes if step_bytes is not None else self.width * 2
        return _lib.xs_kf_process_frame(self.h, ptr, step)

    def hint_next_frame(self, depth_dev, step_bytes=None):
        """The device depth image the NEXT process_frame call will be given (unchanged until then): its maps are built
        during this frame's ICP loop.  Call before process_frame of the current frame."""
        _lib.xs_kf_hint_next_frame(self.h, depth_dev.data_ptr(), step_bytes or self.width * 2)

    def process_frame_host(self, depth_u16):
        """Host frame [H, W] u16: staged through pinned memory and copied asynchronously on the second stream
        (an array returned by ingest_buffer() is used in place)."""
        d = np.ascontiguousarray(depth_u16, dtype=np.uint16)
        return _lib.xs_kf_process_frame_host(self.h, d.ctypes.data)

    def ingest_buffer(self):
        """The next host-pinned staging buffer as a [H, W] uint16 array: fill it, then process_frame_host(it)."""
        ptr = _lib.xs_kf_ingest_buffer(self.h)
        n = self.width * self.height
        return np.ctypeslib.as_array((C.c_uint16 * n).from_address(ptr)).reshape(self.height, self.width)

    def camera2volume(self):
        out = np.zeros(32, np.float32)
        _lib.xs_kf_get_camera2volume(self.h, out.ctypes.data_as(_f32p))
        return out.reshape(4, 4, 2)

    def gauss_newton_terms(self, depth_dev, c2v):
        """29 doubles: J^T J upper triangle (21), J^T r (6), sum r^2, count, for the residual of the depth frame
        against the map at camera2volume c2v [4, 4, 2]."""
        m = np.ascontiguousarray(c2v, dtype=np.float32).reshape(32)
        out = np.zeros(29, np.float64)
        ok = _lib.xs_kf_gauss_newton_terms(self.h, depth_dev.data_ptr(), self.width * 2, m.ctypes.data_as(_f32p), out.ctypes.data_as(_f64p))
        return out if ok == 1 else None

    def pose_hessian_terms(self, depth_dev, c2v):
        """29 doubles: H upper triangle (21), g (6), sum r^2, count — the exact Hessian and the gradient of L = sum r^2 in the twist of
        c2v <- se3Exp(theta) c2v, from one launch over the map's band index."""
        m = np.ascontiguousarray(c2v, dtype=np.float32).reshape(32)
        out = np.zeros(29, np.float64)
        ok = _lib.xs_kf_pose_hessian_terms(self.h, depth_dev.data_ptr(), self.width * 2, m.ctypes.data_as(_f32p), out.ctypes.data_as(_f64p))
        return out if ok == 1 else None

    def pose_hessian(self, depth_dev, c2v):
        """(H [6, 6] symmetric, g [6], sum r^2, count) of pose_hessian_terms."""
        s = self.pose_hessian_terms(depth_dev, c2v)
        if s is None:
            return None
        H = np.zeros((6, 6))
        H[np.triu_indices(6)] = s[:21]
        H = H + np.triu(H, 1).T
        return H, s[21:27].copy(), float(s[27]), int(s[28])

    def relocalize(self, depth_dev, c2v, iterations=5, damping=1e-3, method="gauss_newton"):
        """Refinement of camera2volume against the map: (ok, refined c2v [4, 4, 2], loss history).  method "gauss_newton" (first-order
        seeds) or "newton" (the exact Hessian; the return then gains the number of iterations that fell back to Gauss-Newton)."""
        m = np.ascontiguousarray(c2v, dtype=np.float32).reshape(32).copy()
        hist = np.zeros(iterations + 1, np.float64)
        if method == "newton":
            fb = C.c_int(0)
            ok = _lib.xs_kf_relocalize_newton(self.h, depth_dev.data_ptr(), self.width * 2, m.ctypes.data_as(_f32p), iterations, damping,
                                              hist.ctypes.data_as(_f64p), C.cast(C.byref(fb), _i32p))
            return ok == 1, m.reshape(4, 4, 2), hist, int(fb.value)
        if method != "gauss_newton":
            raise ValueError(f"relocalize: unknown method {method!r}")
        ok = _lib.xs_kf_relocalize(self.h, depth_dev.data_ptr(), self.width * 2, m.ctypes.data_as(_f32p), iterations, damping,
                                   hist.ctypes.data_as(_f64p))
        return ok == 1, m.reshape(4, 4, 2), hist

    def relocalize_batch(self, depths, c2vs, iterations=5, damping=1e-3, method="gauss_newton"):
        """relocalize for F depth frames at once over the map's band index: (ok [F] bool, refined c2v [F, 4, 4, 2], loss histories
        [F, iterations + 1]; with method "newton" also the fallback counts [F]).  Frame f's results equal
        relocalize(depths[f], c2vs[f], ..., method=method) bit for bit."""
        F = len(depths)
        m = np.ascontiguousarray(c2vs, dtype=np.float32).reshape(F * 32).copy()
        hist = np.zeros((F, iterations + 1), np.float64)
        ok = np.zeros(F, np.int32)
        P = (_vp * max(F, 1))(*[d if isinstance(d, int) else d.data_ptr() for d in depths])
        if method == "newton":
            fb = np.zeros(max(F, 1), np.int32)
            n = _lib.xs_kf_relocalize_newton_batch(self.h, F, P, self.width * 2, m.ctypes.data_as(_f32p), iterations, damping,
                                                   hist.ctypes.data_as(_f64p), ok.ctypes.data_as(_i32p), fb.ctypes.data_as(_i32p))
            if n < 0:
                raise ValueError("xs_kf_relocalize_newton_batch: bad arguments")
            return ok == 1, m.reshape(F, 4, 4, 2), hist, fb[:F]
        if method != "gauss_newton":
            raise ValueError(f"relocalize_batch: unknown method {method!r}")
        n = _lib.xs_kf_relocalize_batch(self.h, F, P, self.width * 2, m.ctypes.data_as(_f32p), iterations, damping, hist.ctypes.data_as(_f64p),
                                        ok.ctypes.data_as(_i32p))
        if n < 0:
            raise ValueError("xs_kf_relocalize_batch: bad arguments")
        return ok == 1, m.reshape(F, 4, 4, 2), hist

    def score_poses(self, depth_dev, c2vs):
        """The alignment loss of one depth frame at P camera2volume hypotheses c2vs [P, 4, 4, 2] in one pass over the map's band index per
        4096 poses: (sum loss [P], count [P]) float64 — per pose what xs_compute_local_tsdf_loss gives on the dense map."""
        m = np.ascontiguousarray(c2vs, dtype=np.float32).reshape(-1)
        P = m.size // 32
        assert m.size == 32 * P
        out = np.zeros((max(P, 1), 2), np.float64)
        rc = _lib.xs_kf_score_poses(self.h, depth_dev.data_ptr(), self.width * 2, P, m.ctypes.data_as(_f32p), out.ctypes.data_as(_f64p))
        if rc != 1:
            raise ValueError("xs_kf_score_poses: bad arguments" if rc < 0 else "xs_kf_score_poses: no volume")
        return out[:P, 0].copy(), out[:P, 1].copy()

    def relocalize_global(self, depth_dev, candidates, keep=8, iterations=10, damping=1e-3):
        """Global relocalisation from pose hypotheses candidates [P, 4, 4, 2] (pose_candidates makes them): score all, refine the `keep`
        with the highest S = count - sum loss by Gauss-Newton, return the refined pose with the highest S: (ok, c2v [4, 4, 2], report).
        Not ok (none of the kept converged): c2v is candidates[0] and the report's index is -1."""
        m = np.ascontiguousarray(candidates, dtype=np.float32).reshape(-1)
        P = m.size // 32
        assert m.size == 32 * P and P > 0
        best = m[:32].copy()
        rep = np.zeros(8, np.float64)
        rc = _lib.xs_kf_relocalize_global(self.h, depth_dev.data_ptr(), self.width * 2, P, m.ctypes.data_as(_f32p), int(keep), int(iterations),
                                          float(damping), best.ctypes.data_as(_f32p), rep.ctypes.data_as(_f64p))
        if rc < 0:
            raise ValueError("xs_kf_relocalize_global: bad arguments")
        report = dict(index=int(rep[0]), S_before=float(rep[1]), S_after=float(rep[2]), sum_loss_after=float(rep[3]), count_after=float(rep[4]),
                      refined_ok=int(rep[5]), index_voxels=int(rep[6]))
        return rc == 1, best.reshape(4, 4, 2), report

    @staticmethod
    def _view_call(name, rc, bad):
        if rc == -2:
            raise capi.XsError(f"{name}: not available in shard mode (occlusion along a ray is not additive over z-slabs)")
        if rc == bad:
            raise ValueError(f"{name}: bad arguments or options")

    def score_views(self, c2vs, rays=(80, 60), t_near=0.2, t_far=5.0, step=None, min_weight=1):
        """What the camera would see from P hypothetical camera2volume poses c2vs [P, 4, 4, 2] (real parts; pose_candidates makes them), one
        launch over the volume's two-bit observation grid per 4096 poses: uint32 [P, 4] = {unknown, free, hits, frontier} samples per pose
        along rays[0] x rays[1] rays, depths t_near .. t_far in increments of `step` (None: a voxel).  XsError in shard mode."""
        m = np.ascontiguousarray(c2vs, dtype=np.float32).reshape(-1)
        P = m.size // 32
        assert m.size == 32 * P
        out = np.zeros((max(P, 1), 4), np.uint32)
        opts = capi.view_opts(rays, t_near, t_far, step)
        rc = _lib.xs_kf_score_views(self.h, P, m.ctypes.data_as(_f32p), C.byref(opts), int(min_weight), out.ctypes.data_as(C.POINTER(C.c_uint)))
        self._view_call("xs_kf_score_views", rc, -1)
        if rc != 1:
            raise ValueError("xs_kf_score_views: no volume")
        return out[:P].copy()

    def next_best_view(self, candidates, min_hits=None, rays=(80, 60), t_near=0.2, t_far=5.0, step=None, min_weight=1):
        """The candidate ([P, 4, 4, 2]) that sees the most unknown space among those with at least min_hits rays ending on a known surface
        (None: a quarter of the rays): (index, counts uint32 [P, 4] as score_views returns them); index -1 when no candidate qualifies.
        XsError in shard mode."""
        m = np.ascontiguousarray(candidates, dtype=np.float32).reshape(-1)
        P = m.size // 32
        assert m.size == 32 * P
        if min_hits is None:
            min_hits = int(rays[0]) * int(rays[1]) // 4
        out = np.zeros((max(P, 1), 4), np.uint32)
        opts = capi.view_opts(rays, t_near, t_far, step)
        rc = _lib.xs_kf_next_best_view(self.h, P, m.ctypes.data_as(_f32p), C.byref(opts), int(min_weight), int(min_hits),
                                       out.ctypes.data_as(C.POINTER(C.c_uint)))
        self._view_call("xs_kf_next_best_view", rc, -3)
        return int(rc), out[:P].copy()

    def clearance_field(self, max_radius_vox=8, unknown_blocks=True, min_weight=1):
        """How far the nearest obstacle is: uint16 [Z, Y, X] = min(d^2, R^2) in voxels, R = max_radius_vox (1 .. 255), to the nearest OCCUPIED
        voxel — with unknown_blocks also the nearest UNKNOWN voxel or position outside the volume — of the observation grid at min_weight.
        XsError in shard mode."""
        out = np.zeros((self.res[2], self.res[1], self.res[0]), np.uint16)
        rc = _lib.xs_kf_clearance_field(self.h, int(max_radius_vox), int(bool(unknown_blocks)), int(min_weight), out.ctypes.data_as(C.POINTER(C.c_uint16)))
        self._reach_call("xs_kf_clearance_field", rc, -1)
        if rc != 1:
            raise ValueError("xs_kf_clearance_field: no volume")
        return out

    @staticmethod
    def _reach_call(name, rc, bad):
        if rc == -2:
            raise capi.XsError(f"{name}: not available in shard mode (distance and connectivity are not additive over z-slabs)")
        if rc == bad:
            raise ValueError(f"{name}: bad arguments or options")

    def reachable(self, c2vs, radius_m, start=None, snap_vox=4, unknown_blocks=True, min_weight=1):
        """Which of the P camera2volume poses c2vs [P, 4, 4, 2] a body of radius_m can get to from `start` ([4, 4, 2]; None: the current
        camera2volume) through known free space: (reachable bool [P], clear2 uint16 [P] — the clearance field at each pose's centre voxel,
        squared voxels, capped at the R the radius needs).  The start is snapped to the nearest passable voxel within snap_vox voxels; the
        candidates are not snapped.  XsError in shard mode."""
        m = np.ascontiguousarray(c2vs, dtype=np.float32).reshape(-1)
        P = m.size // 32
        assert m.size == 32 * P
        flags, clear2 = np.zeros(max(P, 1), np.uint8), np.zeros(max(P, 1), np.uint16)
        s = None if start is None else np.ascontiguousarray(start, dtype=np.float32).reshape(32)
        rc = _lib.xs_kf_reachable(self.h, None if s is None else s.ctypes.data_as(_f32p), float(radius_m), int(snap_vox), int(bool(unknown_blocks)),
                                  int(min_weight), P, m.ctypes.data_as(_f32p), flags.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                  clear2.ctypes.data_as(C.POINTER(C.c_uint16)))
        self._reach_call("xs_kf_reachable", rc, -1)
        if rc != 1:
            raise ValueError("xs_kf_reachable: no volume")
        return flags[:P].astype(bool), clear2[:P].copy()

    def next_reachable_view(self, candidates, radius_m, min_hits=None, rays=(80, 60), t_near=0.2, t_far=5.0, step=None, min_weight=1, snap_vox=4,
                            unknown_blocks=True):
        """next_best_view among the candidates a body of radius_m can get to from the current camera through known free space: (index, counts
        uint32 [P, 4], reachable bool [P]); index -1 when no reachable candidate qualifies.  XsError in shard mode."""
        m = np.ascontiguousarray(candidates, dtype=np.float32).reshape(-1)
        P = m.size // 32
        assert m.size == 32 * P
        if min_hits is None:
            min_hits = int(rays[0]) * int(rays[1]) // 4
        out, flags = np.zeros((max(P, 1), 4), np.uint32), np.zeros(max(P, 1), np.uint8)
        opts = capi.view_opts(rays, t_near, t_far, step)
        rc = _lib.xs_kf_next_reachable_view(self.h, P, m.ctypes.data_as(_f32p), C.byref(opts), int(min_weight), int(min_hits),
                                            out.ctypes.data_as(C.POINTER(C.c_uint)), float(radius_m), int(snap_vox), int(bool(unknown_blocks)),
                                            flags.ctypes.data_as(C.POINTER(C.c_ubyte)))
        self._reach_call("xs_kf_next_reachable_view", rc, -3)
        return int(rc), out[:P].copy(), flags[:P].astype(bool)

    def _travel_m(self, units):
        """uint16 travel costs (thirds of a voxel edge) as float64 metres, inf for 65535."""
        vs = float(np.float32(float(self.cfg["tsdf_voxel_size"])))
        u = np.asarray(units, np.uint16)
        return np.where(u == capi.TRAVEL_NONE, np.inf, u.astype(np.float64) * vs / 3.0)

    def travel(self, c2vs, radius_m, start=None, snap_vox=4, unknown_blocks=True, min_weight=1, max_travel_m=None):
        """reachable() plus how far each pose is: (reachable bool [P], clear2 uint16 [P], travel_m float64 [P]) — the length in metres of the
        shortest path of 26-neighbour moves that cuts no corner (the <3, 4, 5> chamfer metric) from the snapped start to each pose's centre
        voxel through the reached voxels, inf where unreachable or beyond max_travel_m (None: no limit but 65534 thirds of a voxel).
        XsError in shard mode."""
        m = np.ascontiguousarray(c2vs, dtype=np.float32).reshape(-1)
        P = m.size // 32
        assert m.size == 32 * P
        flags, clear2, cost = np.zeros(max(P, 1), np.uint8), np.zeros(max(P, 1), np.uint16), np.zeros(max(P, 1), np.uint16)
        s = None if start is None else np.ascontiguousarray(start, dtype=np.float32).reshape(32)
        rc = _lib.xs_kf_travel(self.h, None if s is None else s.ctypes.data_as(_f32p), float(radius_m), int(snap_vox), int(bool(unknown_blocks)),
                               int(min_weight), 0.0 if max_travel_m is None else float(max_travel_m), P, m.ctypes.data_as(_f32p),
                               flags.ctypes.data_as(C.POINTER(C.c_ubyte)), clear2.ctypes.data_as(C.POINTER(C.c_uint16)),
                               cost.ctypes.data_as(C.POINTER(C.c_uint16)))
        self._reach_call("xs_kf_travel", rc, -1)
        if rc != 1:
            raise ValueError("xs_kf_travel: no volume")
        return flags[:P].astype(bool), clear2[:P].copy(), self._travel_m(cost[:P])

    def path_to(self, c2v, radius_m, start=None, snap_vox=4, unknown_blocks=True, min_weight=1, max_travel_m=None, capacity=1024):
        """The shortest collision-free path from the snapped start to the centre voxel of pose c2v ([4, 4, 2]), start first and target last:
        (points float32 [n, 3] — the voxel centres in volume coordinates, metres —, voxels int32 [n, 3]), or None when the target is not
        reached (or beyond max_travel_m).  A path longer than `capacity` voxels is fetched by one more call.  XsError in shard mode."""
        t = np.ascontiguousarray(c2v, dtype=np.float32).reshape(32)
        s = None if start is None else np.ascontiguousarray(start, dtype=np.float32).reshape(32)
        capacity = max(int(capacity), 1)
        for _ in range(2):
            voxels, points, needed = np.zeros((capacity, 3), np.int32), np.zeros((capacity, 3), np.float32), C.c_int(0)
            rc = _lib.xs_kf_path_to(self.h, None if s is None else s.ctypes.data_as(_f32p), float(radius_m), int(snap_vox), int(bool(unknown_blocks)),
                                    int(min_weight), 0.0 if max_travel_m is None else float(max_travel_m), t.ctypes.data_as(_f32p), capacity,
                                    voxels.ctypes.data_as(_i32p), points.ctypes.data_as(_f32p), C.byref(needed))
            if rc != -4:
                break
            capacity = int(needed.value)
        self._reach_call("xs_kf_path_to", rc, -1)
        if rc < 0:
            raise capi.XsError(f"xs_kf_path_to: {rc}")
        return None if rc == 0 else (points[:rc].copy(), voxels[:rc].copy())

    def next_view_by_travel(self, candidates, radius_m, bias_m=0.5, min_hits=None, rays=(80, 60), t_near=0.2, t_far=5.0, step=None, min_weight=1,
                            snap_vox=4, unknown_blocks=True, max_travel_m=None):
        """Weighs what a view sees against how far away it is: among the candidates a body of radius_m can get to from the current camera
        (within max_travel_m) with at least min_hits rays on a known surface, the one with the largest unknown / (travel + bias), bias_m
        being the fixed cost of taking any view at all: (index, counts uint32 [P, 4], travel_m float64 [P]); index -1 when no candidate
        qualifies.  XsError in shard mode."""
        m = np.ascontiguousarray(candidates, dtype=np.float32).reshape(-1)
        P = m.size // 32
        assert m.size == 32 * P
        if min_hits is None:
            min_hits = int(rays[0]) * int(rays[1]) // 4
        out, cost = np.zeros((max(P, 1), 4), np.uint32), np.zeros(max(P, 1), np.uint16)
        opts = capi.view_opts(rays, t_near, t_far, step)
        rc = _lib.xs_kf_next_view_by_travel(self.h, P, m.ctypes.data_as(_f32p), C.byref(opts), int(min_weight), int(min_hits),
                                            out.ctypes.data_as(C.POINTER(C.c_uint)), float(radius_m), int(snap_vox), int(bool(unknown_blocks)),
                                            0.0 if max_travel_m is None else float(max_travel_m), float(bias_m), cost.ctypes.data_as(C.POINTER(C.c_uint16)))
        self._reach_call("xs_kf_next_view_by_travel", rc, -3)
        return int(rc), out[:P].copy(), self._travel_m(cost[:P])

    FRONTIER_DTYPE = np.dtype([("label", np.uint32), ("count", np.uint64), ("sum", np.uint64, 3), ("centroid", np.float32, 3), ("min", np.int32, 3),
                               ("max", np.int32, 3)])

    @staticmethod
    def _frontier_call(name, rc):
        if rc == -2:
            raise capi.XsError(f"{name}: not available in shard mode (neither connectivity nor a cluster is additive over z-slabs)")
        if rc == -1:
            raise ValueError(f"{name}: bad arguments or options")

    def frontiers(self, cell_vox=32, min_size=8, min_weight=1):
        """Where known free space borders the unknown, grouped: the clusters of the frontier voxels (FREE with an UNKNOWN face neighbour in the
        observation grid at min_weight; 26-adjacency within cells of cell_vox voxels, 0: the whole volume, otherwise a multiple of 8) that
        have at least min_size voxels, in ascending label order.  A structured array with fields label (the lowest linear voxel index
        (z Y + y) X + x of the cluster), count, sum (of x, y, z), centroid (float32 metres in volume coordinates: (sum / count + 0.5) voxels)
        and the bounding box min / max (x, y, z voxels, inclusive).  XsError in shard mode."""
        capacity, n = 1024, C.c_int(0)
        for _ in range(2):
            rec = np.zeros((max(capacity, 1), capi.FRONTIER_RECORD_WORDS), np.uint64)
            rc = _lib.xs_kf_frontiers(self.h, int(cell_vox), int(min_size), int(min_weight), capacity, rec.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n))
            if rc != -4:
                break
            capacity = int(n.value)
        self._frontier_call("xs_kf_frontiers", rc)
        if rc != 1:
            raise ValueError("xs_kf_frontiers: no volume" if rc == 0 else f"xs_kf_frontiers: {rc}")
        return self._cluster_records(rec[:n.value])

    def _cluster_records(self, rec):
        """Records of 8 uint64 in the frontier's format [n, 8] as a structured array of FRONTIER_DTYPE: label, count, sum, the centroid in
        metres and the bounding box."""
        out = np.zeros(len(rec), self.FRONTIER_DTYPE)
        out["label"], out["count"], out["sum"] = rec[:, 0], rec[:, 1], rec[:, 2:5]
        vs = np.float32(float(self.cfg["tsdf_voxel_size"]))
        q = (rec[:, 2:5].astype(np.float64) / np.maximum(rec[:, 1:2], 1).astype(np.float64)).astype(np.float32)
        out["centroid"] = (q + np.float32(0.5)) * vs
        for name, col in (("min", 5), ("max", 6)):
            out[name] = np.stack([(rec[:, col] >> np.uint64(s)) & np.uint64(0xFFFF) for s in (0, 16, 32)], axis=1).astype(np.int32)
        return out

    def propose_views(self, radius_m, views_per_cluster=6, standoff_m=1.0, cell_vox=32, min_size=8, snap_vox=4, start_snap_vox=4, unknown_blocks=True,
                      min_weight=1):
        """Candidate views from the map alone: for every cluster frontiers(cell_vox, min_size, min_weight) returns, views_per_cluster
        standpoints at standoff_m around its centroid (Halton directions), each snapped to the nearest voxel within snap_vox that a body of
        radius_m reaches from the current camera (its start snapped within start_snap_vox, as reachable() does), duplicates and
        standpoints with no such voxel dropped: (c2vs float32 [P, 4, 4, 2] — at the voxel's centre, looking at the centroid —, cluster index
        int32 [P] into that list).  reachable() and travel() call every proposed pose reachable.  XsError in shard mode."""
        capacity, n = 1024, C.c_int(0)
        for _ in range(2):
            m, idx = np.zeros((max(capacity, 1), 4, 4, 2), np.float32), np.zeros(max(capacity, 1), np.int32)
            rc = _lib.xs_kf_propose_views(self.h, float(radius_m), int(start_snap_vox), int(bool(unknown_blocks)), int(min_weight), int(cell_vox), int(min_size),
                                          int(views_per_cluster), float(standoff_m), int(snap_vox), capacity, m.ctypes.data_as(_f32p), idx.ctypes.data_as(_i32p),
                                          C.byref(n))
            if rc != -4:
                break
            capacity = int(n.value)
        self._frontier_call("xs_kf_propose_views", rc)
        if rc != 1:
            raise ValueError("xs_kf_propose_views: no volume" if rc == 0 else f"xs_kf_propose_views: {rc}")
        return m[:n.value].copy(), idx[:n.value].copy()

    def explore_step(self, radius_m, views_per_cluster=6, standoff_m=1.0, cell_vox=32, min_size=8, snap_vox=4, unknown_blocks=True, min_weight=1, bias_m=0.5,
                     min_hits=None, rays=(80, 60), t_near=0.2, t_far=5.0, step=None, max_travel_m=None):
        """Where should the camera go next, and which way?  propose_views, then next_view_by_travel over the proposed poses, then path_to the
        chosen one (the start is snapped within snap_vox in all three).  A dict with index (into propose_views' list for the same arguments),
        pose [4, 4, 2], cluster, counts uint32 [4] = {unknown, free, hits, frontier}, travel_m and path (path_to's (points, voxels)); None
        when no view is proposed or none qualifies.  XsError in shard mode."""
        cands, cluster = self.propose_views(radius_m, views_per_cluster, standoff_m, cell_vox, min_size, snap_vox, snap_vox, unknown_blocks, min_weight)
        if len(cands) == 0:
            return None
        pick, counts, travel_m = self.next_view_by_travel(cands, radius_m, bias_m=bias_m, min_hits=min_hits, rays=rays, t_near=t_near, t_far=t_far, step=step,
                                                          min_weight=min_weight, snap_vox=snap_vox, unknown_blocks=unknown_blocks, max_travel_m=max_travel_m)
        if pick < 0:
            return None
        path = self.path_to(cands[pick], radius_m, snap_vox=snap_vox, unknown_blocks=unknown_blocks, min_weight=min_weight, max_travel_m=max_travel_m)
        return dict(index=pick, pose=cands[pick].copy(), cluster=int(cluster[pick]), counts=counts[pick].copy(), travel_m=float(travel_m[pick]), path=path)

    def relocalization_index_voxels(self):
        """Band voxels in the relocalisation index as last built by relocalize_batch (0 before the first)."""
        return int(_lib.xs_kf_relocalization_index_voxels(self.h))

    def export_point_cloud(self, max_buffer=1000000):
        """ExportPointCloud: (points [n, 3], normals [n, 3]) float32 on the host."""
        p = np.zeros((max_buffer, 3), np.float32)
        nr = np.zeros((max_buffer, 3), np.float32)
        n = _lib.xs_kf_export_point_cloud(self.h, max_buffer, p.ctypes.data_as(_f32p), nr.ctypes.data_as(_f32p))
        return p[:n], nr[:n]

    def export_ply(self, filename, max_buffer=1000000):
        return _lib.xs_kf_export_ply(self.h, max_buffer, str(filename).encode())

    def export_mesh(self, min_weight=1):
        """ExportMesh: the marching-cubes mesh on the host, a Mesh of vertices [V, 3] f32, vertex_im [V, 3] f32 (raw Im, divide by
        csfd_seed_h; None without a CSFD seed), normals [V, 3] f32, triangles [T, 3] i32 and edge_keys [V] u64."""
        nt, has_im = C.c_longlong(0), C.c_int(0)
        nv = _lib.xs_kf_export_mesh(self.h, min_weight, 0, 0, None, None, None, None, None, C.byref(nt), C.byref(has_im))
        while True:   # (the volume does not change between the calls: one retry)
            cap_v, cap_t = nv, nt.value
            v, n, im = (np.zeros((cap_v, 3), np.float32) for _ in range(3))
            k = np.zeros(cap_v, np.uint64)
            t = np.zeros((cap_t, 3), np.int32)
            nv = _lib.xs_kf_export_mesh(self.h, min_weight, cap_v, cap_t, v.ctypes.data_as(_f32p), n.ctypes.data_as(_f32p), im.ctypes.data_as(_f32p),
                                        k.ctypes.data_as(C.POINTER(C.c_uint64)), t.ctypes.data_as(_i32p), C.byref(nt), C.byref(has_im))
            if nv <= cap_v and nt.value <= cap_t:
                return Mesh(v[:nv], im[:nv] if has_im.value else None, n[:nv], t[:nt.value], k[:nv])

    def export_mesh_ply(self, filename):
        """Binary little-endian PLY of export_mesh (with dx dy dz = vertex_im while a CSFD seed is active); the vertex count, -1 on failure."""
        return _lib.xs_kf_export_mesh_ply(self.h, str(filename).encode())

    def synchronize(self):
        _lib.xs_kf_synchronize(self.h)

    @property
    def frame_id(self):
        return _lib.xs_kf_frame_id(self.h)

    def num_poses(self):
        return _lib.xs_kf_num_poses(self.h)

    def world2camera(self, idx=-1):
        out = np.zeros(32, np.float32)
        _lib.xs_kf_get_world2camera(self.h, idx, out.ctypes.data_as(_f32p))
        return out.reshape(4, 4, 2)

    def tranc_dist(self):
        return _lib.xs_kf_tranc_dist(self.h)

    def last_U(self):
        return _lib.xs_kf_last_updated_voxels(self.h)

    def last_hits(self):
        return _lib.xs_kf_last_raycast_hits(self.h)

    def icp_log(self):
        n = _lib.xs_kf_icp_log(self.h, None, 0)
        out = np.zeros(n, np.float64)
        if n:
            _lib.xs_kf_icp_log(self.h, out.ctypes.data_as(_f64p), n)
        return out.reshape(-1, 55)

    def volume(self):
        n = self.res[0] * self.res[1] * self.res[2]
        v, w, g = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.float32)
        _lib.xs_kf_download_volume(self.h, v.ctypes.data_as(_f32p), w.ctypes.data_as(_i32p), g.ctypes.data_as(_f32p))
        return v, w, g

    def map(self, which, level):
        rows, cols = self.height >> level, self.width >> level
        planes = 1 if which == "depths_curr" else 3
        out = np.zeros((planes * rows, cols, 2), np.float32)
        rc = _lib.xs_kf_download_map(self.h, MAPS[which], level, out.ctypes.data_as(_f32p))
        assert rc == 0
        return out

    def volume_ptr(self, which):
        step = _sz(0)
        p = _lib.xs_kf_volume_ptr(self.h, {"value": 0, "weight": 1, "grad": 2}[which], C.byref(step))
        return p, step.value

    def set_profiling(self, level=2):
        """0 off, 1 integrate-kernel events + counters only, 2 (True) every stage."""
        _lib.xs_kf_set_profiling(self.h, 2 if level is True else int(level))

    def stage_times(self):
        ms = np.zeros(6, np.float64)
        calls = (C.c_longlong * 6)()
        _lib.xs_kf_stage_times(self.h, ms.ctypes.data_as(_f64p), calls)
        return {s: (float(ms[i]), int(calls[i])) for i, s in enumerate(STAGES)}

    def cumulative_counters(self):
        u, h = C.c_longlong(0), C.c_longlong(0)
        _lib.xs_kf_cumulative_counters(self.h, C.byref(u), C.byref(h))
        return u.value, h.value

    def reset_stage_times(self):
        _lib.xs_kf_reset_stage_times(self.h)

    def icp_iteration_times(self):
        """{slot: (microseconds summed, iterations)} of the ICP loop's host-side iteration period since the last reset; slots 0..2 = pyramid
        level, 3 = the first iteration of each frame (which also waits for the previous frame's tail)."""
        us = np.zeros(4, np.float64)
        calls = (C.c_longlong * 4)()
        _lib.xs_kf_icp_iteration_times(self.h, us.ctypes.data_as(_f64p), calls)
        return {lv: (float(us[lv]), int(calls[lv])) for lv in range(4)}

    def tail_host_times(self):
        """Mean host microseconds per frame of the tail's four host stretches since the last reset (xs_kf_tail_host_times)."""
        us = np.zeros(4, np.float64)
        n = C.c_longlong(0)
        _lib.xs_kf_tail_host_times(self.h, us.ctypes.data_as(_f64p), C.byref(n))
        k = max(int(n.value), 1)
        return {"frames": int(n.value), "sums_seen_to_integrate_entered": round(float(us[0]) / k, 2), "entered_to_launch_call": round(float(us[1]) / k, 2),
                "integrate_launch_call": round(float(us[2]) / k, 2), "launch_returned_to_raycast_launched": round(float(us[3]) / k, 2)}

    def gn_poll_times(self, reset=False):
        """Mean microseconds a Gauss-Newton kernel that was enqueued ahead waited for its poses (the device's own clock), and how many such passes."""
        pu, n = C.c_double(0), C.c_longlong(0)
        _lib.xs_kf_gn_poll_times(self.h, C.byref(pu), C.byref(n), int(reset))
        return {"passes": int(n.value), "wait_us": pu.value / max(n.value, 1)}

    def set_gn_post_pose(self, on):
        _lib.xs_kf_set_gn_post_pose(self.h, int(bool(on)))

    def gn_times(self, reset=False):
        """Gauss-Newton passes run by relocalize since the last reset: mean wall clock per pass and (profiling on) mean kernel duration, microseconds."""
        pu, km = C.c_double(0), C.c_double(0)
        n, kc = C.c_longlong(0), C.c_longlong(0)
        _lib.xs_kf_gn_times(self.h, C.byref(pu), C.byref(n), C.byref(km), C.byref(kc), int(reset))
        return {"passes": int(n.value), "pass_us": pu.value / max(n.value, 1), "kernel_calls": int(kc.value), "kernel_us": 1e3 * km.value / max(kc.value, 1)}

    def debug_set_icp_sequence(self, v):
        _lib.xs_kf_debug_set_icp_sequence(self.h, int(v))

    def debug_fail_icp_iteration(self, n):
        _lib.xs_kf_debug_fail_icp_iteration(self.h, int(n))

    def debug_post_delay(self, min_us, max_us):
        """Test aid: a random host sleep of [min_us, max_us] microseconds in front of every ICP pose post."""
        _lib.xs_kf_debug_post_delay(self.h, int(min_us), int(max_us))

    def composite_bytes(self):
        """Shard mode: bytes this rank received through the raycast composite's collectives so far (see xs_kf_composite_bytes)."""
        return int(_lib.xs_kf_composite_bytes(self.h))

    def list_cover_counts(self):
        """Frames whose list / box classes decided ahead held for the final pose: {"neither": n, "list_only": n, "both": n}."""
        c = (C.c_longlong * 4)()
        _lib.xs_kf_list_cover_counts(self.h, c)
        return {"neither": int(c[0]), "list_only": int(c[1]), "both": int(c[3])}

    def rebuild_sign_map(self):
        """After writing the value array through volume_ptr: the ray march's sign map is rebuilt from the volume."""
        _lib.xs_kf_rebuild_sign_map(self.h)

    def volume_generation(self):
        """The version of the volume's contents: moves with every write of the volume, stays under calls that only read the map."""
        return int(_lib.xs_kf_volume_generation(self.h))

    def save_checkpoint(self, path, sparse=False):
        """The volume and the pose record to a file.  sparse=False: the dense XSTSDF2 dump, 12 bytes per voxel.  sparse=True: the brick-sparse
        XSTSDF3 (lossless; classified and compacted on the GPU, streamed through one pinned staging buffer), and the save's statistics as a dict:
        bricks, classes (bricks per class 0 .. 7), payload_words, file_bytes, chunks.  load_checkpoint and every *_checkpoint method take
        either file.  A rank of a sharded run saves its own planes in either format."""
        if not sparse:
            _lib.xs_kf_save_checkpoint(self.h, path.encode())
            return None
        s = (C.c_ulonglong * 12)()
        if _lib.xs_kf_save_checkpoint_sparse(self.h, path.encode(), s) != 0:
            raise OSError(f"save_checkpoint: cannot write {path}")
        return dict(bricks=int(s[0]), classes=[int(s[1 + c]) for c in range(8)], payload_words=int(s[9]), file_bytes=int(s[10]), chunks=int(s[11]))

    def checkpoint_staging_words(self, words=0):
        """The staging buffer of sparse saves and loads in 32-bit words (default 16 Mi = 64 MiB): set when words >= 1536, returned either way."""
        n = int(_lib.xs_kf_checkpoint_staging_words(self.h, int(words)))
        if n < 0:
            raise ValueError("checkpoint_staging_words: at least 1536 words (one brick at its largest)")
        return n

    def load_checkpoint(self, path):
        """Restores the volume, the pose record and the frame number from a checkpoint of either format (the magic decides), written by an
        instance of the same geometry (and, in shard mode, the same rank).  False, with the state unchanged, for any other file."""
        return _lib.xs_kf_load_checkpoint(self.h, path.encode()) == 0

    def save_tsdf_volume(self, path):
        _lib.xs_kf_save_tsdf_volume(self.h, path.encode())

    @staticmethod
    def _map_call(name, rc, bad, zero_ok=False):
        """The return code of a call that takes a second map: XsError in shard mode, ValueError on bad arguments (`bad` names the call's own) and,
        unless zero_ok (the align calls: no result), without a volume."""
        if rc == -2:
            raise capi.XsError(f"{name}: not available in shard mode")
        if rc == -1:
            raise ValueError(f"{name}: bad arguments ({bad}, the volume itself as source, a bad file or another truncation distance)")
        if rc != 1 and not (zero_ok and rc == 0):
            raise ValueError(f"{name}: no volume" if rc == 0 else f"{name}: {rc}")

    def _merge_call(self, name, source, T, min_weight):
        t = _real44(np.eye(4) if T is None else T)
        n = C.c_ulonglong(0)
        self._map_call(name, getattr(_lib, name)(self.h, source, t.ctypes.data_as(_f64p), int(min_weight), C.byref(n)), "T not finite, min_weight < 1")
        return int(n.value)

    def merge_map(self, other, T=None, min_weight=1):
        """Merges the map of `other` (another KinectFusion of this process; only read) into this one: its volume is resampled into this map's
        voxel grid under T (real 4 x 4: a point of THIS map's volume frame, in metres, to the other map's; None: the identity) and averaged in by
        weight as a new observation is, where all the corners it is interpolated from carry min_weight.  Resolutions and voxel sizes may
        differ, the truncation distances may not.  Everything derived from the volume follows; poses and the frame number do not change.
        Returns the number of voxels written.  XsError in shard mode, ValueError on bad arguments (the state is unchanged)."""
        return self._merge_call("xs_kf_merge_map", other.h, T, min_weight)

    def merge_checkpoint(self, path, T=None, min_weight=1):
        """merge_map with the other map read from a checkpoint file of a whole volume (save_checkpoint, dense or sparse: either format is accepted); the file is validated before anything
        is touched and a bad one raises ValueError with the state unchanged."""
        return self._merge_call("xs_kf_merge_checkpoint", path.encode(), T, min_weight)

    def _reintegrate_call(self, depths, c2v_olds, c2v_news, modes, frames):
        n = len(depths)
        if n < 1 or len(modes) != n:
            raise ValueError("reintegrate: at least one frame, one mode per frame")
        P = (_vp * n)(*[d if isinstance(d, int) else d.data_ptr() for d in depths])

        def poses(c):
            if c is None:
                return None, None
            a = np.ascontiguousarray(c, dtype=np.float32).reshape(-1)
            if a.size != 32 * n:
                raise ValueError("reintegrate: one camera2volume [4, 4, 2] per frame")
            return a, a.ctypes.data_as(_f32p)

        olds, po = poses(c2v_olds)
        news, pn = poses(c2v_news)
        mode = np.ascontiguousarray(modes, np.int32)
        idx = None if frames is None else np.ascontiguousarray([-1 if f is None else int(f) for f in frames], np.int32)
        if idx is not None and idx.size != n:
            raise ValueError("reintegrate: one frame index (or None) per frame")
        counts = (C.c_ulonglong * 4)()
        rc = _lib.xs_kf_reintegrate(self.h, n, P, self.width * 2, po, pn, mode.ctypes.data_as(_i32p), None if idx is None else idx.ctypes.data_as(_i32p), counts)
        if rc == -2:
            raise capi.XsError("reintegrate: not available in shard mode")
        if rc != 1:
            raise ValueError("reintegrate: no volume" if rc == 0 else "reintegrate: bad arguments (a pose that is not finite, a frame index past the record)")
        return dict(removed=int(counts[0]), added=int(counts[1]), emptied=int(counts[2]), orphaned=int(counts[3]))

    def deintegrate(self, depth_dev, c2v):
        """Takes the depth frame (torch CUDA tensor [H, W], u16 millimetres) fused at camera2volume c2v [4, 4, 2] out of the volume again: every
        voxel the frame wrote loses that observation from its running mean and one unit of weight; a voxel it alone had written is empty
        again.  Exact up to rounding while no weight had reached max_integration_weight (include/xslam_amd.h: what removal cannot undo).
        Everything derived from the volume follows, as after merge_map; poses and the frame number do not change.  Returns the counts
        dict(removed, added, emptied, orphaned) in voxels; orphaned: the frame would have written there but nothing was left to take.
        XsError in shard mode, ValueError on bad arguments (the state is unchanged)."""
        return self._reintegrate_call([depth_dev], [c2v], None, [1], None)

    def reintegrate(self, depth_dev, c2v_old, c2v_new, frame=None):
        """deintegrate at c2v_old and fuse the same frame again at c2v_new, in one pass over the volume.  frame: the index of that frame in the
        pose record (world2camera(frame)), which then receives the pose that gives c2v_new.  Returns the counts."""
        return self._reintegrate_call([depth_dev], [c2v_old], [c2v_new], [3], None if frame is None else [frame])

    def reintegrate_batch(self, depths, c2v_olds, c2v_news, frames=None):
        """reintegrate for several frames: the observations are applied in list order, up to eight per pass over the volume, and the derived
        state is rebuilt once.  The volume equals the one the single calls in the same order leave, bit for bit.  Returns the summed counts."""
        return self._reintegrate_call(list(depths), c2v_olds, c2v_news, [3] * len(depths), frames)

    def refine_frame(self, depth_dev, c2v, iterations=5, damping=1e-3, frame=None):
        """Refines the pose of a frame that is already fused: takes it out at c2v, runs relocalize against the map without it starting at c2v —
        a map that still holds the frame pulls the refinement towards where the frame already is — and puts it back at the refined pose, or at
        c2v again if the refinement failed.  Returns (ok, refined c2v [4, 4, 2], loss history, counts of both edits summed)."""
        c2v = np.ascontiguousarray(c2v, dtype=np.float32).reshape(4, 4, 2)
        out = self.deintegrate(depth_dev, c2v)
        ok, refined, hist = self.relocalize(depth_dev, c2v, iterations=iterations, damping=damping)
        ok = bool(ok) and bool(np.isfinite(refined).all())
        back = self._reintegrate_call([depth_dev], None, [refined if ok else c2v], [2], None if frame is None or not ok else [frame])
        return ok, (refined if ok else c2v), hist, {k: out[k] + back[k] for k in out}

    def _render_call(self, name, source, c2vs, intr, size, t_near, t_far, step, min_weight, outputs, cull, device):
        m = np.ascontiguousarray(c2vs, dtype=np.float32)
        if m.ndim == 2 or (m.ndim == 3 and m.shape[-1] == 2):
            m = m[None]
        if m.shape[1:] not in ((4, 4), (4, 4, 2)) or m.shape[0] < 1:
            raise ValueError(f"{name}: c2vs must be [P, 4, 4] or [P, 4, 4, 2]")
        P, is_complex = m.shape[0], int(m.ndim == 4)
        m = m.reshape(-1)
        k = None if intr is None else np.ascontiguousarray(intr, dtype=np.float32).reshape(4)
        rows, cols = (self.height, self.width) if size is None else (int(size[0]), int(size[1]))
        wanted = set(outputs)
        if not wanted or not wanted <= {"depth", "depth_u16", "normal", "shade", "counts"}:
            raise ValueError(f"{name}: outputs must name some of depth, depth_u16, normal, shade, counts")
        shapes = dict(depth=((P, rows, cols), np.float32), depth_u16=((P, rows, cols), np.uint16), normal=((P, 3, rows, cols), np.float32),
                      shade=((P, rows, cols), np.uint8), counts=((P, 4), np.uint32))
        out, ptr = {}, {}
        if device:
            import torch
            dt = {np.float32: torch.float32, np.uint16: getattr(torch, "uint16", torch.int16), np.uint8: torch.uint8, np.uint32: torch.int32}
            for n in wanted:
                out[n] = torch.empty(shapes[n][0], dtype=dt[shapes[n][1]], device="cuda")
                ptr[n] = out[n].data_ptr()
        else:
            for n in wanted:
                out[n] = np.zeros(*shapes[n])
                ptr[n] = out[n].ctypes.data
        opts = capi.render_opts(t_near, t_far, step, min_weight, cull)
        rc = getattr(_lib, name)(self.h, *source, P, m.ctypes.data_as(_f32p), is_complex, None if k is None else k.ctypes.data_as(_f32p), rows, cols,
                                 C.byref(opts), ptr.get("depth"), ptr.get("depth_u16"), ptr.get("normal"), ptr.get("shade"), ptr.get("counts"), int(bool(device)))
        self._map_call(name, rc, "poses, intrinsics or size out of range or not finite, t_far <= t_near, more than 4096 samples, a map that cannot be rendered")
        return RenderedViews(*(out.get(n) for n in RenderedViews._fields))

    def render_views(self, c2vs, intr=None, size=None, t_near=0.2, t_far=5.0, step=None, min_weight=1, outputs=("depth", "normal", "shade"), cull=True,
                     device=False):
        """Views of the map from P poses the caller picks, c2vs [P, 4, 4] or [P, 4, 4, 2] camera-to-volume (real parts; camera2volume() gives one),
        64 views per launch: a RenderedViews of the `outputs` asked for (depth, depth_u16, normal, shade, counts), numpy arrays, or torch tensors
        on the GPU with device=True.  intr (fx, fy, cx, cy) and size (rows, cols) default to the configuration's camera; depths t_near .. t_far
        along the camera's z in increments of `step` (None: a voxel); a voxel with a weight below min_weight is unseen.  cull=False reads every
        sample instead of consulting the brick mask: the same bits, slower.  depth_u16 is what a depth sensor at that pose would deliver, so it
        can stand in for a frame: relocalize(views.depth_u16[p], c2v) with device=True.  counts says how the rays ended; a crossing whose two
        trilinear values do not bracket zero is rejected, which a step of two or three voxels makes rarer than a step of one (DESIGN.md section
        4.28).  XsError in shard mode, ValueError on bad arguments."""
        return self._render_call("xs_kf_render_views", (), c2vs, intr, size, t_near, t_far, step, min_weight, outputs, cull, device)

    def render_map(self, other, c2vs, **kw):
        """render_views of the map of `other` (another KinectFusion of this process, which is only read); the poses are in ITS volume frame, the
        default camera is this instance's."""
        kw = {**dict(intr=None, size=None, t_near=0.2, t_far=5.0, step=None, min_weight=1, outputs=("depth", "normal", "shade"), cull=True, device=False), **kw}
        return self._render_call("xs_kf_render_map", (other.h,), c2vs, **kw)

    def render_checkpoint(self, path, c2vs, **kw):
        """render_views of the map in a checkpoint file of a whole volume (save_checkpoint, dense or sparse), validated as merge_checkpoint does."""
        kw = {**dict(intr=None, size=None, t_near=0.2, t_far=5.0, step=None, min_weight=1, outputs=("depth", "normal", "shade"), cull=True, device=False), **kw}
        return self._render_call("xs_kf_render_checkpoint", (path.encode(),), c2vs, **kw)

    _SAMPLE_OUTPUTS = ("status", "value", "dvalue", "gradient", "counts")

    @classmethod
    def _sample_buffers(cls, name, outputs, shapes, device):
        """The output buffers of a sample call: (dict of arrays or tensors, dict of their addresses)."""
        wanted = set(outputs)
        if not wanted or not wanted <= set(cls._SAMPLE_OUTPUTS):
            raise ValueError(f"{name}: outputs must name some of status, value, dvalue, gradient, counts")
        dtypes = dict(status=np.uint8, value=np.float32, dvalue=np.float32, gradient=np.float32, counts=np.uint64)
        out, ptr = {}, {}
        for n in wanted:
            if device:
                import torch
                dt = {np.uint8: torch.uint8, np.float32: torch.float32, np.uint64: torch.int64}[dtypes[n]]
                out[n] = torch.empty(shapes[n], dtype=dt, device="cuda")
                ptr[n] = out[n].data_ptr()
            else:
                out[n] = np.zeros(shapes[n], dtypes[n])
                ptr[n] = out[n].ctypes.data
        return out, ptr

    def _sample_call(self, name, source, points, T, min_weight, outputs, device):
        if hasattr(points, "data_ptr"):   # a torch tensor on the GPU
            if not points.is_cuda or not points.is_contiguous() or points.dim() != 2 or points.shape[1] != 3 or points.element_size() != 4 or not points.is_floating_point():
                raise ValueError(f"{name}: a torch points tensor must be contiguous float32 [N, 3] on the GPU")
            n, pp, on_device, keep = int(points.shape[0]), points.data_ptr(), 1, points
        else:
            keep = np.ascontiguousarray(points, dtype=np.float32)
            if keep.ndim != 2 or keep.shape[1] != 3:
                raise ValueError(f"{name}: points must be [N, 3]")
            n, pp, on_device = keep.shape[0], keep.ctypes.data, 0
        if n < 1:
            raise ValueError(f"{name}: at least one point is needed")
        t = None if T is None else _real44(T)
        out, ptr = self._sample_buffers(name, outputs, dict(status=(n,), value=(n,), dvalue=(n,), gradient=(n, 3), counts=(4,)), device)
        rc = getattr(_lib, name)(self.h, *source, n, pp, None if t is None else t.ctypes.data_as(_f64p), int(min_weight), ptr.get("status"), ptr.get("value"),
                                 ptr.get("dvalue"), ptr.get("gradient"), ptr.get("counts"), on_device | (2 if device else 0))
        self._map_call(name, rc, "more than 2^30 points, T not finite, dvalue of a map without a grad array")
        return MapSamples(*(out.get(f) for f in MapSamples._fields))

    def sample(self, points, T=None, min_weight=1, outputs=("status", "value", "gradient"), device=False):
        """The map asked at N points: what is the signed distance here, which way does it grow, has this place been seen.  points [N, 3] in metres,
        a numpy array or a contiguous float32 torch tensor on the GPU, in a frame that T (real 4 x 4; None: they are in the volume frame already
        and their bits are used as they are) takes to the volume frame.  Returns a MapSamples of the `outputs` asked for (status, value, dvalue,
        gradient, counts): numpy arrays, or torch tensors on the GPU with device=True.  value is the trilinear interpolation of the stored TSDF
        (the render's F, bit for bit), which is normalised by the truncation distance: value * tranc_dist() is the signed distance in metres
        near the surface, positive in free space, and the field is TRUNCATED: farther than tranc_dist() from the surface it is +-1 and says
        only which side the point is on, or the point is UNSEEN.  gradient is the central difference over one voxel, in value per metre: it
        points into free space with a length of about 1 / tranc_dist() near the surface.  dvalue is the same interpolation of the run's
        derivative volume (the CSFD seed's).  A voxel with a weight below min_weight is unseen.  XsError in shard mode, ValueError on bad
        arguments."""
        return self._sample_call("xs_kf_sample_points", (), points, T, min_weight, outputs, device)

    def sample_map(self, other, points, T=None, min_weight=1, outputs=("status", "value", "gradient"), device=False):
        """sample of the map of `other` (another KinectFusion of this process, which is only read); T takes the points to ITS volume frame."""
        return self._sample_call("xs_kf_sample_map", (other.h,), points, T, min_weight, outputs, device)

    def sample_checkpoint(self, path, points, T=None, min_weight=1, outputs=("status", "value", "gradient"), device=False):
        """sample of the map in a checkpoint file of a whole volume (save_checkpoint, dense or sparse), validated as merge_checkpoint does."""
        return self._sample_call("xs_kf_sample_checkpoint", (path.encode(),), points, T, min_weight, outputs, device)

    def frame_residuals(self, depth, c2v, min_weight=1, outputs=("status", "value"), device=False, intr=None):
        """A depth frame judged against the map before it is fused: every pixel's point (depth [rows, cols] u16 millimetres, a numpy array or a torch
        tensor on the GPU; unprojected with intr, None: the configuration's, and placed by the camera2volume c2v [4, 4] or [4, 4, 2]) sampled in
        the map.  Returns a FrameResiduals of images: value is the pixel's signed residual in units of the truncation distance (0 on the
        surface the map holds; large where an object moved or the pose is off), status says why a pixel has none."""
        m = np.ascontiguousarray(c2v, dtype=np.float32)
        if m.shape not in ((4, 4), (4, 4, 2)):
            raise ValueError("frame_residuals: c2v must be [4, 4] or [4, 4, 2]")
        if hasattr(depth, "data_ptr"):
            if not depth.is_cuda or depth.dim() != 2 or depth.element_size() != 2 or depth.stride(1) != 1:
                raise ValueError("frame_residuals: a torch depth image must be 16-bit [rows, cols] on the GPU")
            rows, cols, dp, step, on_device, keep = int(depth.shape[0]), int(depth.shape[1]), depth.data_ptr(), depth.stride(0) * 2, 1, depth
        else:
            keep = np.ascontiguousarray(depth, dtype=np.uint16)
            if keep.ndim != 2:
                raise ValueError("frame_residuals: depth must be [rows, cols]")
            rows, cols, dp, step, on_device = keep.shape[0], keep.shape[1], keep.ctypes.data, keep.shape[1] * 2, 0
        k = None if intr is None else np.ascontiguousarray(intr, dtype=np.float32).reshape(4)
        name = "xs_kf_frame_residuals"
        shape = (rows, cols)
        out, ptr = self._sample_buffers(name, outputs, dict(status=shape, value=shape, dvalue=shape, gradient=(3,) + shape, counts=(4,)), device)
        rc = _lib.xs_kf_frame_residuals(self.h, dp, step, m.reshape(-1).ctypes.data_as(_f32p), int(m.ndim == 3), None if k is None else k.ctypes.data_as(_f32p), rows, cols,
                                        int(min_weight), ptr.get("status"), ptr.get("value"), ptr.get("dvalue"), ptr.get("gradient"), ptr.get("counts"),
                                        on_device | (2 if device else 0))
        self._map_call(name, rc, "an empty or oversized image, a pose or intrinsics that are not finite")
        return FrameResiduals(*(out.get(f) for f in FrameResiduals._fields))

    def surface_error(self, points, T=None, min_weight=1):
        """How far a set of surface points (a ground-truth scan, another sensor's cloud) lies from the surface the map holds: a dict of the counts
        outside, unseen and ok, and over the OK points mean_abs, rms and max_abs of d = value * tranc_dist() in metres (NaN without an OK point).
        Float64 host arithmetic on sample's value output.  The field is truncated: a point farther than tranc_dist() from the surface
        contributes tranc_dist()."""
        s = self.sample(points, T=T, min_weight=min_weight, outputs=("status", "value", "counts"))
        d = s.value[s.status == capi.SAMPLE_OK].astype(np.float64) * float(self.tranc_dist())
        stats = dict(mean_abs=float(np.abs(d).mean()), rms=float(np.sqrt((d * d).mean())), max_abs=float(np.abs(d).max())) if d.size else \
            dict(mean_abs=float("nan"), rms=float("nan"), max_abs=float("nan"))
        return dict(outside=int(s.counts[0]), unseen=int(s.counts[1]), ok=int(s.counts[2]), **stats)

    def _diff_call(self, name, source, T, min_weight, lo, hi, cell_vox, min_size, masks, capacity):
        t = _real44(np.eye(4) if T is None else T)
        u64p = C.POINTER(C.c_uint64)
        dense = [np.zeros((self.res[2], self.res[1], self.res[0]), np.uint8) for _ in range(2)] if masks else None
        dp = [d.ctypes.data_as(C.POINTER(C.c_ubyte)) for d in dense] if masks else [None, None]
        counts, n_this, n_other = np.zeros(3, np.uint64), C.c_int(0), C.c_int(0)
        for _ in range(2):   # (the second with room for the counts the first returned)
            recs = [np.zeros((max(capacity, 1), capi.FRONTIER_RECORD_WORDS), np.uint64) for _ in range(2)]
            rc = getattr(_lib, name)(self.h, *source, t.ctypes.data_as(_f64p), int(min_weight), float(lo), float(hi), int(cell_vox), int(min_size), capacity,
                                     recs[0].ctypes.data_as(u64p), C.byref(n_this), recs[1].ctypes.data_as(u64p), C.byref(n_other),
                                     counts.ctypes.data_as(C.POINTER(C.c_ulonglong)), dp[0], dp[1])
            if rc != -4:
                break
            capacity = max(int(n_this.value), int(n_other.value))
        self._map_call(name, rc, "T, lo or hi not finite, lo > hi, min_weight < 1, a bad cell")
        return MapDiff(dict(compared=int(counts[0]), only_this=int(counts[1]), only_other=int(counts[2])), self._cluster_records(recs[0][:n_this.value]),
                       self._cluster_records(recs[1][:n_other.value]), tuple(dense) if masks else None)

    def diff_map(self, other, T=None, min_weight=1, lo=0.0, hi=0.5, cell_vox=0, min_size=8, masks=False, capacity=1024):
        """What differs between this map and the map of `other` (another KinectFusion of this process), with nothing averaged: THIS map is
        self, the OTHER map is `other` resampled into this map's voxel grid under T as merge_map does it (real 4 x 4: a point of this map's
        volume frame, in metres, to the other map's; None: the identity).  A voxel is compared where both maps carry min_weight; it is
        only_this where this map's value is below lo and the other's at least hi (matter here, firmly free there) and only_other the other
        way round.  With `other` the earlier map, only_this is what appeared and only_other what went away.  Returns a MapDiff: counts (a
        dict of compared, only_this and only_other voxels), only_this and only_other (the clusters of each class with at least min_size voxels,
        26-adjacency within cells of cell_vox voxels, 0: the whole volume, as frontiers() returns them) and masks (the pair of uint8 [Z, Y, X],
        with masks=True).  capacity: the first guess at the number of clusters per class; a longer list is fetched by a second run.  Nothing
        of either map is modified.  XsError in shard mode, ValueError on bad arguments.
        Intended use: kf.diff_map(other, kf.align_map_global(other)[1])."""
        return self._diff_call("xs_kf_diff_map", (other.h,), T, min_weight, lo, hi, cell_vox, min_size, masks, int(capacity))

    def diff_checkpoint(self, path, T=None, min_weight=1, lo=0.0, hi=0.5, cell_vox=0, min_size=8, masks=False, capacity=1024):
        """diff_map with the other map read from a checkpoint file of a whole volume (save_checkpoint, dense or sparse: either format is accepted), validated as merge_checkpoint does: with
        yesterday's checkpoint as the other map, only_this is what appeared since and only_other what went away.
        Intended use: kf.diff_checkpoint(path, kf.align_checkpoint_global(path)[1])."""
        return self._diff_call("xs_kf_diff_checkpoint", (path.encode(),), T, min_weight, lo, hi, cell_vox, min_size, masks, int(capacity))

    def _align_call(self, name, source, T0, iterations, damping, min_weight, max_residual):
        t = np.asarray(np.eye(4) if T0 is None else T0, dtype=np.float64)
        t = np.ascontiguousarray(t.reshape(-1, 4, 4))
        iterations = int(iterations)
        out, report, hist = np.zeros((4, 4), np.float64), np.zeros(8, np.float64), np.zeros(max(iterations, 0) + 1, np.float64)
        rc = getattr(_lib, name)(self.h, source, t.ctypes.data_as(_f64p), t.shape[0], iterations, float(damping), int(min_weight), float(max_residual),
                                 out.ctypes.data_as(_f64p), report.ctypes.data_as(_f64p), hist.ctypes.data_as(_f64p))
        self._map_call(name, rc, "T not finite, iterations < 0, min_weight < 1, max_residual or damping out of range", zero_ok=True)
        rep = {"start": int(report[0]), "count": int(report[1]), "sum_r2": float(report[2]), "loss": float(report[3]), "passes": int(report[4]),
               "ended_ok": int(report[5]), "band_voxels": int(report[6])}
        return rc == 1, (out if rc == 1 else t[0].copy()), rep, (hist.copy() if rc == 1 else hist[:0].copy())

    def align_map(self, other, T0=None, iterations=10, damping=1e-3, min_weight=1, max_residual=1.0):
        """Registers the map of `other` (another KinectFusion of this process) to this one, volume to volume, before a merge: damped Gauss-Newton
        over this map's band voxels on "the other map resampled under T minus this map", at the sample positions merge_map(other, T) will use.
        T0: a starting guess as merge_map takes T (None: the identity), or a stack [N, 4, 4] of them, refined together; the best by
        S = count - sum r^2 wins.  Returns (ok, T [4, 4] float64, report dict, loss history [iterations + 1]); ok False (T = the first start) when
        no start kept six voxels on every pass and a positive definite system.  Nothing is modified.  XsError in shard mode, ValueError on bad arguments.
        Intended use: kf.merge_map(other, kf.align_map(other, T_guess)[1])."""
        return self._align_call("xs_kf_align_map", other.h, T0, iterations, damping, min_weight, max_residual)

    def align_checkpoint(self, path, T0=None, iterations=10, damping=1e-3, min_weight=1, max_residual=1.0):
        """align_map with the other map read from a checkpoint file of a whole volume (save_checkpoint, dense or sparse: either format is accepted), validated as merge_checkpoint does.
        Intended use: kf.merge_checkpoint(path, kf.align_checkpoint(path, T_guess)[1])."""
        return self._align_call("xs_kf_align_checkpoint", path.encode(), T0, iterations, damping, min_weight, max_residual)

    @staticmethod
    def _points_arg(name, points):
        """(n, address, on_device, the array to keep alive) of a cloud: a numpy array [N, 3] or a contiguous float32 torch tensor on the GPU."""
        if hasattr(points, "data_ptr"):   # a torch tensor on the GPU
            if not points.is_cuda or not points.is_contiguous() or points.dim() != 2 or points.shape[1] != 3 or points.element_size() != 4 or not points.is_floating_point():
                raise ValueError(f"{name}: a torch points tensor must be contiguous float32 [N, 3] on the GPU")
            n, pp, on_device, keep = int(points.shape[0]), points.data_ptr(), 1, points
        else:
            keep = np.ascontiguousarray(points, dtype=np.float32)
            if keep.ndim != 2 or keep.shape[1] != 3:
                raise ValueError(f"{name}: points must be [N, 3]")
            n, pp, on_device = keep.shape[0], keep.ctypes.data, 0
        if n < 1:
            raise ValueError(f"{name}: at least one point is needed")
        return n, pp, on_device, keep

    def _register_call(self, name, source, points, T0, iterations, damping, min_weight, max_residual):
        n, pp, on_device, keep = self._points_arg(name, points)
        t = np.asarray(np.eye(4) if T0 is None else T0, dtype=np.float64)
        t = np.ascontiguousarray(t.reshape(-1, 4, 4))
        iterations = int(iterations)
        out, report, hist = np.zeros((4, 4), np.float64), np.zeros(7, np.float64), np.zeros(max(iterations, 0) + 1, np.float64)
        rc = getattr(_lib, name)(self.h, *source, n, pp, on_device, t.ctypes.data_as(_f64p), t.shape[0], iterations, float(damping), int(min_weight),
                                 float(max_residual), out.ctypes.data_as(_f64p), report.ctypes.data_as(_f64p), hist.ctypes.data_as(_f64p))
        self._map_call(name, rc, "more than 2^30 points, T not finite, iterations < 0, min_weight < 1, max_residual or damping out of range", zero_ok=True)
        rep = {"start": int(report[0]), "count": int(report[1]), "sum_r2": float(report[2]), "loss": float(report[3]), "passes": int(report[4]),
               "ended_ok": int(report[5]), "points": int(report[6]), "loss_history": hist.copy() if rc == 1 else hist[:0].copy()}
        return rc == 1, (out if rc == 1 else t[0].copy()), rep

    def register_points(self, points, T0=None, iterations=10, damping=1e-3, min_weight=1, max_residual=0.9):
        """Registers a point cloud (a lidar sweep, another sensor's points, a ground-truth scan, an exported cloud of an earlier session) to this
        map: damped Gauss-Newton on "the map's value at T p" over the points, whose Jacobian is the map's gradient there, one launch per pass
        for all starts.  points [N, 3] in metres, a numpy array or a contiguous float32 torch tensor on the GPU.  T0: a starting guess (real
        4 x 4: a point of the cloud's frame to the volume frame; None: the identity), or a stack [N, 4, 4] of them, refined together; the
        best by S = count - sum r^2 among the starts that kept six points on every pass wins (align_map's rule; iterations=0 ranks the starts
        without stepping).  A point takes part where the map holds a value and a gradient at T p with min_weight and |value| <= max_residual.
        The default max_residual is 0.9 rather than align_map's 1.0: a sample of exactly +-1 is the truncated field, which has gradient 0 and
        carries no information about T, so such points only dilute the loss.  Returns (ok, T [4, 4] float64, report dict: start, count,
        sum_r2, loss, passes, ended_ok, points, loss_history [iterations + 1]); ok False (T = the first start) when no start ended ok.
        Nothing is modified.  XsError in shard mode, ValueError on bad arguments.
        Intended use: kf.surface_error(scan, kf.register_points(scan, T_guess)[1])."""
        return self._register_call("xs_kf_register_points", (), points, T0, iterations, damping, min_weight, max_residual)

    def register_map_points(self, other, points, T0=None, iterations=10, damping=1e-3, min_weight=1, max_residual=0.9):
        """register_points against the map of `other` (another KinectFusion of this process, which is only read); T takes the points to ITS volume frame."""
        return self._register_call("xs_kf_register_map", (other.h,), points, T0, iterations, damping, min_weight, max_residual)

    def register_checkpoint_points(self, path, points, T0=None, iterations=10, damping=1e-3, min_weight=1, max_residual=0.9):
        """register_points against the map in a checkpoint file of a whole volume (save_checkpoint, dense or sparse), validated as merge_checkpoint does."""
        return self._register_call("xs_kf_register_checkpoint", (path.encode(),), points, T0, iterations, damping, min_weight, max_residual)

    _FUSE_COUNTS = ("used", "dropped", "visits", "outside", "written")

    def fuse_points(self, points, T=None, origin=(0.0, 0.0, 0.0), min_range=0.2, max_range=5.0, carve=False, weight=1):
        """Fuses a point cloud (a lidar sweep, another sensor's points, a ground-truth scan, an earlier session's cloud) into the map.  points [N, 3]
        in metres, a numpy array or a contiguous float32 torch tensor on the GPU, and origin, the sensor's position, both in a frame that T (real
        4 x 4, as register_points returns it; None: the volume frame, the bits as they are) takes to the volume frame.  Each point's ray from the
        origin is walked in half-voxel steps through the truncation band around the point (carve=True: from the sensor on, which turns the
        unknown space the ray crosses into free space for the planning calls, at the cost of a walk as long as the ray); a voxel the sweep
        touches receives one observation of `weight`, the mean over the rays through it of the signed distance to the point ALONG THE RAY,
        averaged in as a depth frame's is.  Rays shorter than min_range or longer than max_range are dropped.  Integer atomics only: the
        result does not depend on the order of the points, and two calls on equal maps give equal bytes.  Returns a dict of used and dropped
        points, visits (voxel additions), outside (ray samples that left the volume) and written voxels.  Everything derived from the map
        follows; poses and the frame number stay.  XsError in shard mode, ValueError on bad arguments.
        Intended use: kf.fuse_points(sweep, kf.register_points(sweep, T_guess)[1], origin=sensor_position)."""
        name = "xs_kf_fuse_points"
        n, pp, on_device, keep = self._points_arg(name, points)
        t = None if T is None else _real44(T)
        o = np.ascontiguousarray(origin, dtype=np.float32).reshape(-1)
        if o.size != 3:
            raise ValueError(f"{name}: origin must have three entries")
        counts = (C.c_ulonglong * 5)()
        rc = _lib.xs_kf_fuse_points(self.h, n, pp, on_device, None if t is None else t.ctypes.data_as(_f64p), o.ctypes.data_as(_f32p), float(min_range),
                                    float(max_range), int(bool(carve)), int(weight), counts)
        self._map_call(name, rc, "T, origin or a range not finite, min_range <= 0, max_range < min_range or too long, weight outside 1 .. max_integration_weight")
        return {k: int(counts[i]) for i, k in enumerate(self._FUSE_COUNTS)}

    def _score_points_call(self, name, source, points, Ts, stride, min_weight, max_residual):
        n, pp, on_device, keep = self._points_arg(name, points)
        t = np.ascontiguousarray(np.asarray(Ts, dtype=np.float64).reshape(-1, 4, 4))
        out = np.zeros((t.shape[0], 2), np.float64)
        rc = getattr(_lib, name)(self.h, *source, n, pp, on_device, t.shape[0], t.ctypes.data_as(_f64p), int(stride), int(min_weight), float(max_residual),
                                 out.ctypes.data_as(_f64p))
        self._map_call(name, rc, "more than 2^30 points, " + self._BAD_SEARCH)
        return out

    def score_point_transforms(self, points, Ts, stride=1, min_weight=1, max_residual=0.9):
        """{sum r^2, count} [P, 2] float64 of "this map's value at T p" over every stride-th point of a cloud (as register_points takes it), for
        each T of Ts [P, 4, 4] (cloud frame to volume frame), in one launch per 4096 transforms: register_points' residual without its
        gradient, so a point counts wherever the map holds a value with min_weight and |value| <= max_residual.  S = count - sum r^2 ranks the
        transforms.  Nothing is modified.  XsError in shard mode, ValueError on bad arguments."""
        return self._score_points_call("xs_kf_score_point_transforms", (), points, Ts, stride, min_weight, max_residual)

    def score_map_point_transforms(self, other, points, Ts, stride=1, min_weight=1, max_residual=0.9):
        """score_point_transforms against the map of `other` (another KinectFusion of this process, which is only read)."""
        return self._score_points_call("xs_kf_score_point_transforms_map", (other.h,), points, Ts, stride, min_weight, max_residual)

    def score_checkpoint_point_transforms(self, path, points, Ts, stride=1, min_weight=1, max_residual=0.9):
        """score_point_transforms against the map in a checkpoint file of a whole volume (either format), validated as merge_checkpoint does."""
        return self._score_points_call("xs_kf_score_point_transforms_checkpoint", (path.encode(),), points, Ts, stride, min_weight, max_residual)

    def _register_global_call(self, name, source, points, candidates, keep, rounds, stride, box_t, refine_t, refine_r, iterations, damping, min_weight, max_residual, Ts):
        n, pp, on_device, alive = self._points_arg(name, points)
        o = RegisterSearchOpts()
        _lib.xs_kf_register_search_defaults(self.h, C.byref(o))
        o.candidates, o.keep, o.rounds, o.stride, o.iterations, o.min_weight = int(candidates), int(keep), int(rounds), int(stride), int(iterations), int(min_weight)
        if box_t is not None:
            o.box_t = float(box_t)
        if refine_t is not None:
            o.refine_t = float(refine_t)
        o.refine_r, o.damping, o.max_residual = float(refine_r), float(damping), float(max_residual)
        user = None
        if Ts is not None:
            user = np.ascontiguousarray(np.asarray(Ts, dtype=np.float64).reshape(-1, 4, 4))
            o.user_n, o.user_T16xN = user.shape[0], user.ctypes.data_as(_f64p)
        out, report = np.eye(4, dtype=np.float64), np.zeros(12, np.float64)
        rc = getattr(_lib, name)(self.h, *source, n, pp, on_device, C.byref(o), out.ctypes.data_as(_f64p), report.ctypes.data_as(_f64p))
        self._map_call(name, rc, "more than 2^30 points or more than 2^24 scored ones (raise the stride), " + self._BAD_SEARCH, zero_ok=True)
        rep = {"rank": int(report[0]), "S_before": float(report[1]), "count": int(report[2]), "sum_r2": float(report[3]), "loss": float(report[4]),
               "score_launches": int(report[5]), "passes": int(report[6]), "ended_ok": int(report[7]), "points": int(report[8]),
               "scored_points": int(report[9]), "centroid_distance": float(report[10])}
        return rc == 1, out, rep

    def register_points_global(self, points, candidates=2048, keep=8, rounds=2, stride=4, box_t=None, refine_t=None, refine_r=0.25, iterations=10, damping=1e-3,
                               min_weight=1, max_residual=0.9, Ts=None):
        """register_points with no starting guess: a lidar sweep taken somewhere in the mapped room, yesterday's exported cloud in another frame,
        a ground-truth scan.  `candidates` transforms that cover all rotations (transform_candidates_free; translations take the centroid of
        the scored points onto the map's band centroid, jittered by box_t metres) are scored over every stride-th point
        (score_point_transforms), the `keep` best by S = count - sum r^2 are refined over `rounds` rounds of candidates about each
        (transform_candidates_around about the cloud's centroid: boxes refine_t metres and refine_r radians, halved per round), and the kept
        transforms start register_points' loop over ALL the points.  box_t, refine_t None: the map's truncation distance.  Ts [N, 4, 4]:
        candidates of the caller's that replace the free ones.  Returns (ok, T [4, 4] float64, report dict: rank, S_before, count, sum_r2,
        loss, score_launches, passes, ended_ok, points, scored_points, centroid_distance); ok False (T = the identity) when no start ended ok
        or the map has no band voxel.  The score cannot tell a scene from its image under one of its own symmetries: a symmetric scene has
        several equally good answers and any of them may be returned.  A cloud that covers only part of the map has its centroid elsewhere:
        widen box_t.  Nothing is modified.  XsError in shard mode, ValueError on bad arguments.
        Intended use: kf.fuse_points(sweep, kf.register_points_global(sweep)[1], origin=sensor_position)."""
        return self._register_global_call("xs_kf_register_points_global", (), points, candidates, keep, rounds, stride, box_t, refine_t, refine_r, iterations, damping,
                                          min_weight, max_residual, Ts)

    def register_map_points_global(self, other, points, candidates=2048, keep=8, rounds=2, stride=4, box_t=None, refine_t=None, refine_r=0.25, iterations=10,
                                   damping=1e-3, min_weight=1, max_residual=0.9, Ts=None):
        """register_points_global against the map of `other` (another KinectFusion of this process, which is only read); T takes the points to ITS volume frame."""
        return self._register_global_call("xs_kf_register_points_global_map", (other.h,), points, candidates, keep, rounds, stride, box_t, refine_t, refine_r,
                                          iterations, damping, min_weight, max_residual, Ts)

    def register_checkpoint_points_global(self, path, points, candidates=2048, keep=8, rounds=2, stride=4, box_t=None, refine_t=None, refine_r=0.25, iterations=10,
                                          damping=1e-3, min_weight=1, max_residual=0.9, Ts=None):
        """register_points_global against the map in a checkpoint file of a whole volume (save_checkpoint, dense or sparse), validated as merge_checkpoint does."""
        return self._register_global_call("xs_kf_register_points_global_checkpoint", (path.encode(),), points, candidates, keep, rounds, stride, box_t, refine_t,
                                          refine_r, iterations, damping, min_weight, max_residual, Ts)

    def register_and_fuse(self, points, T0=None, origin=(0.0, 0.0, 0.0), iterations=10, damping=1e-3, min_weight=1, max_residual=0.9, min_range=0.2, max_range=5.0,
                          carve=False, weight=1, global_search=False):
        """register_points followed, when it succeeded, by fuse_points at the winning transform: (ok, T, register report, fuse counts or None).
        Nothing is fused when no start ended ok.  global_search=True: the registration is register_points_global at its defaults (with these
        iterations, damping, min_weight and max_residual) and T0 is not used; the report is that call's."""
        if global_search:
            ok, T, rep = self.register_points_global(points, iterations=iterations, damping=damping, min_weight=min_weight, max_residual=max_residual)
            fused = self.fuse_points(points, T, origin, min_range, max_range, carve, weight) if ok else None
            return ok, T, rep, fused
        ok, T, rep = self.register_points(points, T0, iterations, damping, min_weight, max_residual)
        fused = self.fuse_points(points, T, origin, min_range, max_range, carve, weight) if ok else None
        return ok, T, rep, fused

    def release_fuse_scratch(self):
        """Frees fuse_points' accumulator (8 bytes per voxel); the next fuse_points allocates it again."""
        _lib.xs_kf_release_fuse_scratch(self.h)

    _BAD_SEARCH = "T not finite, a count, stride, box, min_weight, max_residual or damping out of range"

    def _score_transforms_call(self, name, source, Ts, stride, min_weight, max_residual):
        t = np.ascontiguousarray(np.asarray(Ts, dtype=np.float64).reshape(-1, 4, 4))
        out = np.zeros((t.shape[0], 2), np.float64)
        rc = getattr(_lib, name)(self.h, source, t.shape[0], t.ctypes.data_as(_f64p), int(stride), int(min_weight), float(max_residual), out.ctypes.data_as(_f64p))
        self._map_call(name, rc, self._BAD_SEARCH)
        return out

    def score_transforms(self, other, Ts, stride=1, min_weight=1, max_residual=1.0):
        """{sum r^2, count} [P, 2] float64 of "the map of `other` resampled under T minus this map" over every stride-th voxel of this map's
        band, for each T of Ts [P, 4, 4] (as merge_map takes T), in one launch per 4096 transforms: the residual and the gates of align_map,
        without derivatives.  S = count - sum r^2 ranks the transforms.  Nothing is modified.  XsError in shard mode, ValueError on bad arguments."""
        return self._score_transforms_call("xs_kf_score_transforms", other.h, Ts, stride, min_weight, max_residual)

    def score_transforms_checkpoint(self, path, Ts, stride=1, min_weight=1, max_residual=1.0):
        """score_transforms with the other map read from a checkpoint file of a whole volume (either format is accepted), validated as merge_checkpoint does."""
        return self._score_transforms_call("xs_kf_score_transforms_checkpoint", path.encode(), Ts, stride, min_weight, max_residual)

    def _align_global_call(self, name, source, candidates, keep, rounds, stride, box_t, refine_t, refine_r, iterations, damping, min_weight, max_residual, Ts):
        o = AlignSearchOpts()
        _lib.xs_kf_align_search_defaults(self.h, C.byref(o))
        o.candidates, o.keep, o.rounds, o.stride, o.iterations, o.min_weight = int(candidates), int(keep), int(rounds), int(stride), int(iterations), int(min_weight)
        if box_t is not None:
            o.box_t = float(box_t)
        if refine_t is not None:
            o.refine_t = float(refine_t)
        o.refine_r, o.damping, o.max_residual = float(refine_r), float(damping), float(max_residual)
        user = None
        if Ts is not None:
            user = np.ascontiguousarray(np.asarray(Ts, dtype=np.float64).reshape(-1, 4, 4))
            o.user_n, o.user_T16xN = user.shape[0], user.ctypes.data_as(_f64p)
        out, report = np.eye(4, dtype=np.float64), np.zeros(12, np.float64)
        rc = getattr(_lib, name)(self.h, source, C.byref(o), out.ctypes.data_as(_f64p), report.ctypes.data_as(_f64p))
        self._map_call(name, rc, self._BAD_SEARCH, zero_ok=True)
        rep = {"rank": int(report[0]), "S_before": float(report[1]), "count": int(report[2]), "sum_r2": float(report[3]), "loss": float(report[4]),
               "score_launches": int(report[5]), "passes": int(report[6]), "ended_ok": int(report[7]), "band_voxels": int(report[8]),
               "scored_entries": int(report[9]), "centroid_distance": float(report[10])}
        return rc == 1, out, rep

    def align_map_global(self, other, candidates=2048, keep=8, rounds=2, stride=4, box_t=None, refine_t=None, refine_r=0.25, iterations=10, damping=1e-3,
                         min_weight=1, max_residual=1.0, Ts=None):
        """align_map with no starting guess: `candidates` transforms that cover all rotations (transform_candidates_free; translations from the
        two maps' band centroids, jittered by box_t metres) are scored over every stride-th band voxel (score_transforms), the `keep` best by
        S = count - sum r^2 are refined over `rounds` rounds of candidates about each (transform_candidates_around: boxes refine_t metres and
        refine_r radians, halved per round), and the kept transforms start align_map's loop.  box_t, refine_t None: this map's truncation
        distance.  Ts [N, 4, 4]: candidates of the caller's that replace the free ones.  Returns (ok, T [4, 4] float64, report dict); ok False
        (T = the identity) when no start ended ok.  The score cannot tell a scene from its image under one of its own symmetries: a symmetric
        scene has several equally good answers and any of them may be returned.  Nothing is modified.  XsError in shard mode, ValueError on
        bad arguments.  Intended use: kf.merge_map(other, kf.align_map_global(other)[1])."""
        return self._align_global_call("xs_kf_align_map_global", other.h, candidates, keep, rounds, stride, box_t, refine_t, refine_r, iterations, damping,
                                       min_weight, max_residual, Ts)

    def align_checkpoint_global(self, path, candidates=2048, keep=8, rounds=2, stride=4, box_t=None, refine_t=None, refine_r=0.25, iterations=10, damping=1e-3,
                                min_weight=1, max_residual=1.0, Ts=None):
        """align_map_global with the other map read from a checkpoint file of a whole volume (save_checkpoint, dense or sparse: either format is accepted), validated as merge_checkpoint
        does.  Intended use: kf.merge_checkpoint(path, kf.align_checkpoint_global(path)[1])."""
        return self._align_global_call("xs_kf_align_checkpoint_global", path.encode(), candidates, keep, rounds, stride, box_t, refine_t, refine_r, iterations,
                                       damping, min_weight, max_residual, Ts)


class ReferenceCallShape:
    """Handle to a C++ ReferenceCallShape (x-slam_amd/host/reference_shape.hpp): the reference's own per-frame call
    sequence over the reference-signature launchers alone, a stream drain where the reference drains the device."""

    def __init__(self, params):
        text = params if isinstance(params, str) else yaml_text(params)
        cfg = {}
        for line in text.splitlines():
            if ":" in line:
                k, v = line.split(":", 1)
                cfg[k.strip()] = v.split("#")[0].strip()
        self.h = _lib.xs_refshape_create(text.encode())
        if not self.h:
            raise ValueError("xs_refshape_create failed (missing config key?)")
        self.res = [int(cfg[f"tsdf_size_{a}"]) for a in "xyz"]
        self.width, self.height = int(cfg["depth_width"]), int(cfg["depth_height"])

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.xs_refshape_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def process_frame(self, depth_dev, step_bytes=None):
        ptr = depth_dev if isinstance(depth_dev, int) else depth_dev.data_ptr()
        return _lib.xs_refshape_process_frame(self.h, ptr, step_bytes if step_bytes is not None else self.width * 2)

    def process_frame_host(self, depth_u16):
        d = np.ascontiguousarray(depth_u16, dtype=np.uint16)
        return _lib.xs_refshape_process_frame_host(self.h, d.ctypes.data)

    @property
    def frame_id(self):
        return _lib.xs_refshape_frame_id(self.h)

    def world2camera(self, idx=-1):
        out = np.zeros(32, np.float32)
        _lib.xs_refshape_get_world2camera(self.h, idx, out.ctypes.data_as(_f32p))
        return out.reshape(4, 4, 2)

    def volume(self):
        n = self.res[0] * self.res[1] * self.res[2]
        v, w, g = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.float32)
        _lib.xs_refshape_download_volume(self.h, v.ctypes.data_as(_f32p), w.ctypes.data_as(_i32p), g.ctypes.data_as(_f32p))
        return v, w, g

    def map(self, which, level):
        rows, cols = self.height >> level, self.width >> level
        planes = 1 if which == "depths_curr" else 3
        out = np.zeros((planes * rows, cols, 2), np.float32)
        assert _lib.xs_refshape_download_map(self.h, MAPS[which], level, out.ctypes.data_as(_f32p)) == 0
        return out

    def icp_log(self):
        n = _lib.xs_refshape_icp_log(self.h, None, 0)
        out = np.zeros(n, np.float64)
        if n:
            _lib.xs_refshape_icp_log(self.h, out.ctypes.data_as(_f64p), n)
        return out.reshape(-1, 54)


def reference_tsdf_hessian(depth_dev, rows, cols, intr4, res, voxel_size, R_dual, t_dual, tranc_dist, gt_dev, with_volumes=False):
    """ComputeLocalTsdf_hessian through its TsdfFusion.h:48-53 signature (xs_launchers.hpp): float4 {loss, gradient, second
    derivative, count} and, with_volumes, the per-voxel (real, grad, hessian, count) volumes."""
    k = np.ascontiguousarray(intr4, np.float32)
    r3 = np.ascontiguousarray(res, np.int32)
    R = np.ascontiguousarray(R_dual, np.float32).reshape(36)
    t = np.ascontiguousarray(t_dual, np.float32).reshape(12)
    n = int(r3[0]) * int(r3[1]) * int(r3[2])
    out = np.zeros(4, np.float32)
    vols = np.zeros(4 * n if with_volumes else 1, np.float32)
    rc = _lib.xs_refshape_hessian(depth_dev.data_ptr(), cols * 2, rows, cols, k.ctypes.data_as(_f32p), r3.ctypes.data_as(_i32p), voxel_size,
                                  R.ctypes.data_as(_f32p), t.ctypes.data_as(_f32p), tranc_dist, gt_dev.data_ptr(), int(with_volumes),
                                  out.ctypes.data_as(_f32p), vols.ctypes.data_as(_f32p) if with_volumes else None)
    assert rc == 0
    if not with_volumes:
        return out
    return out, (vols[:n], vols[n:2 * n], vols[2 * n:3 * n], vols[3 * n:].view(np.int32))


def reference_tsdf_loss(depth_dev, rows, cols, intr4, res, voxel_size, R9, t3, tranc_dist, gt_dev, with_volumes=False):
    """ComputeLocalTsdf_loss through its TsdfFusion.h:55-60 signature: float2 {loss, count} (+ the (real, count) volumes)."""
    k = np.ascontiguousarray(intr4, np.float32)
    r3 = np.ascontiguousarray(res, np.int32)
    R = np.ascontiguousarray(R9, np.float32).reshape(9)
    t = np.ascontiguousarray(t3, np.float32).reshape(3)
    n = int(r3[0]) * int(r3[1]) * int(r3[2])
    out = np.zeros(2, np.float32)
    vols = np.zeros(2 * n if with_volumes else 1, np.float32)
    rc = _lib.xs_refshape_loss(depth_dev.data_ptr(), cols * 2, rows, cols, k.ctypes.data_as(_f32p), r3.ctypes.data_as(_i32p), voxel_size,
                               R.ctypes.data_as(_f32p), t.ctypes.data_as(_f32p), tranc_dist, gt_dev.data_ptr(), int(with_volumes),
                               out.ctypes.data_as(_f32p), vols.ctypes.data_as(_f32p) if with_volumes else None)
    assert rc == 0
    if not with_volumes:
        return out
    return out, (vols[:n], vols[n:].view(np.int32))
