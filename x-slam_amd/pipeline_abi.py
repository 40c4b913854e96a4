"""The host library as ctypes sees it: libxslam_host.so loaded once (one CDLL object for every binding module), the pointer types, the
option structs, the argument table _SIGS of include/xslam_amd_pipeline.h and its binding, STAGES and MAPS.  No CPU fallback."""
import ctypes as C
import os

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
_MERGE_TAIL = [_f64p, C.c_int, C.POINTER(C.c_ulonglong)]   # T16, min_weight, voxels written
_ALIGN_TAIL = [_f64p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_float, _f64p, _f64p, _f64p]   # the register calls' tail without the cloud
_SCORE_TAIL = [C.c_int, _f64p, C.c_int, C.c_int, C.c_float, _f64p]   # P, T16xP, stride, min_weight, max_residual, out2xP
_ALIGN_GLOBAL_TAIL = [C.POINTER(AlignSearchOpts), _f64p, _f64p]   # opts, T16_out, report12

# Where a map comes from, stated once: call family -> (the C entry points that take it from this instance, None where there is no such
# call, from another instance, from a checkpoint file: behind the handle nothing, the other's handle, the path) and the arguments after that.
_MAP_SOURCES = {
    "merge": ((None, "xs_kf_merge_map", "xs_kf_merge_checkpoint"), _MERGE_TAIL),
    "diff": ((None, "xs_kf_diff_map", "xs_kf_diff_checkpoint"), [_f64p] + _DIFF_TAIL),
    "align": ((None, "xs_kf_align_map", "xs_kf_align_checkpoint"), _ALIGN_TAIL),
    "align_global": ((None, "xs_kf_align_map_global", "xs_kf_align_checkpoint_global"), _ALIGN_GLOBAL_TAIL),
    "score_transforms": ((None, "xs_kf_score_transforms", "xs_kf_score_transforms_checkpoint"), _SCORE_TAIL),
    "render": (("xs_kf_render_views", "xs_kf_render_map", "xs_kf_render_checkpoint"), _RENDER_TAIL),
    "sample": (("xs_kf_sample_points", "xs_kf_sample_map", "xs_kf_sample_checkpoint"), _SAMPLE_POINTS + _SAMPLE_TAIL),
    "register": (("xs_kf_register_points", "xs_kf_register_map", "xs_kf_register_checkpoint"), _REGISTER_TAIL),
    "score_points": (("xs_kf_score_point_transforms", "xs_kf_score_point_transforms_map", "xs_kf_score_point_transforms_checkpoint"), _POINT_SCORE_TAIL),
    "register_global": (("xs_kf_register_points_global", "xs_kf_register_points_global_map", "xs_kf_register_points_global_checkpoint"), _REGISTER_GLOBAL_TAIL),
}

_SIGS = {
    "xs_kf_register_search_defaults": (None, [_vp, C.POINTER(RegisterSearchOpts)]),
    "xs_host_points_centroid": (C.c_int, [_f32p, C.c_longlong, C.c_int, _f64p]),
    "xs_host_register_step": (C.c_int, [_f64p, C.c_double, _f64p]),
    "xs_kf_fuse_points": (C.c_int, [_vp, C.c_longlong, _vp, C.c_int, _f64p, _f32p, C.c_float, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_ulonglong)]),
    "xs_kf_release_fuse_scratch": (None, [_vp]),
    "xs_kf_sample_volume": (C.c_int, [_vp, _vp, _vp, _vp, _sz, _i32p, C.c_float, C.c_float] + _SAMPLE_POINTS + _SAMPLE_TAIL),
    "xs_kf_frame_residuals": (C.c_int, [_vp, _vp, _sz, _f32p, C.c_int, _f32p, C.c_int, C.c_int] + _SAMPLE_TAIL),
    "xs_host_sample_compose": (C.c_int, [_f64p, _f64p, _f64p]),
    "xs_kf_render_volume": (C.c_int, [_vp, _vp, _vp, _sz, _i32p, C.c_float, C.c_float] + _RENDER_TAIL),
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
    "xs_kf_merge_volume": (C.c_int, [_vp, _vp, _vp, _vp, _sz, _i32p, C.c_float, C.c_float] + _MERGE_TAIL),
    "xs_kf_diff_volume": (C.c_int, [_vp, _vp, _vp, _sz, _i32p, C.c_float, C.c_float, _f64p] + _DIFF_TAIL),
    "xs_host_merge_affine": (C.c_int, [_f64p, C.c_double, C.c_double, _f32p]),
    "xs_host_map_transform": (C.c_int, [_f64p, _f64p, _f64p]),
    "xs_host_merge_tile_box": (C.c_int, [_f32p, _i32p, _i32p, _i32p, _i32p]),
    "xs_host_align_seeded_maps": (C.c_int, [_f64p, C.c_double, C.c_double, _f32p]),
    "xs_host_align_step": (C.c_int, [_f64p, C.c_double, _f64p]),
    "xs_kf_align_search_defaults": (None, [_vp, C.POINTER(AlignSearchOpts)]),
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
for _names, _tail in _MAP_SOURCES.values():
    _SIGS.update({_n: (C.c_int, [_vp] + _lead + _tail) for _n, _lead in zip(_names, ([], [_vp], [C.c_char_p])) if _n})
for _n, (_r, _a) in _SIGS.items():
    _f = getattr(_lib, _n)
    _f.restype, _f.argtypes = _r, _a

STAGES = ("surface", "icp", "scale", "integrate", "raycast", "resize")
MAPS = {"depths_curr": 0, "vmaps_curr": 1, "nmaps_curr": 2, "vmaps_g_prev": 3, "nmaps_g_prev": 4}
