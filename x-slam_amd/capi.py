"""ctypes binding of the C ABI in include/xslam_amd.h (libxslam_hip.so, built in-tree by
x-slam_amd/csrc/Makefile).  This is the only compute path: if the library is missing the
import fails loudly — there is no CPU fallback.

Device memory, streams and collectives come from PyTorch-ROCm (plumbing); every argument
crossing this boundary is a raw device pointer, a pitch in bytes or a small host array.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libxslam_hip.so")

_vp = C.c_void_p
_sz = C.c_size_t
_f32p = C.POINTER(C.c_float)
_i32p = C.POINTER(C.c_int)
_f64p = C.POINTER(C.c_double)


class XsError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
            "or make -C x-slam_amd/csrc).  There is no CPU fallback.")
    return C.CDLL(LIB_PATH)


_lib = _load()

class IntegrateOpts(C.Structure):
    """xs_integrate_opts (include/xslam_amd.h): what an integrate / classify call takes besides its arguments proper."""
    _fields_ = [("struct_bytes", C.c_uint), ("flags", C.c_uint), ("depth_tiles", C.c_void_p), ("signmap", C.c_void_p),
                ("start_event", C.c_void_p), ("stop_event", C.c_void_p)]


class RaycastOpts(C.Structure):
    """xs_raycast_opts (include/xslam_amd.h)."""
    _fields_ = [("struct_bytes", C.c_uint), ("signmap_shift", C.c_int), ("signmap", C.c_void_p), ("signmap_tranc_dist", C.c_float),
                ("pyr_vmap1", C.c_void_p), ("pyr_nmap1", C.c_void_p), ("pyr_step1", C.c_size_t), ("pyr_vmap2", C.c_void_p), ("pyr_nmap2", C.c_void_p),
                ("pyr_step2", C.c_size_t), ("completion_event", C.c_void_p), ("steps_dev", C.c_void_p), ("pyramid_built", C.c_int)]


class MeshOpts(C.Structure):
    """xs_mesh_opts (include/xslam_amd.h)."""
    _fields_ = [("struct_bytes", C.c_uint), ("zs0", C.c_int), ("zs1", C.c_int), ("z0", C.c_int), ("z1", C.c_int), ("min_weight", C.c_int),
                ("want_normals", C.c_int), ("signmap", C.c_void_p), ("signmap_shift", C.c_int)]


class BandIndex(C.Structure):
    """xs_band_index (include/xslam_amd.h): the band voxels of a slab in the Gauss-Newton walk's order."""
    _fields_ = [("keys", C.c_void_p), ("values", C.c_void_p), ("capacity", C.c_longlong), ("segs", C.c_void_p), ("count", C.c_longlong),
                ("nblocks", C.c_int), ("res", C.c_int * 3), ("z0", C.c_int), ("z1", C.c_int)]


class ReintegrateOp(C.Structure):
    """xs_reintegrate_op (include/xslam_amd.h): one signed observation of tsdf_reintegrate."""
    _fields_ = [("sign", C.c_int), ("depth_scaled", C.c_void_p), ("Rv2c18", C.c_float * 18), ("tv2c6", C.c_float * 6)]


class ViewOpts(C.Structure):
    """xs_view_opts (include/xslam_amd.h)."""
    _fields_ = [("struct_bytes", C.c_uint), ("rays_x", C.c_int), ("rays_y", C.c_int), ("t_near", C.c_float), ("t_far", C.c_float), ("step", C.c_float)]


class RenderOpts(C.Structure):
    """xs_render_opts (include/xslam_amd.h)."""
    _fields_ = [("struct_bytes", C.c_uint), ("t_near", C.c_float), ("t_far", C.c_float), ("step", C.c_float), ("min_weight", C.c_int), ("cull", C.c_int),
                ("shade_mode", C.c_int)]


class SampleOpts(C.Structure):
    """xs_sample_opts (include/xslam_amd.h)."""
    _fields_ = [("struct_bytes", C.c_uint), ("min_weight", C.c_int)]


class FuseOpts(C.Structure):
    """xs_fuse_opts (include/xslam_amd.h)."""
    _fields_ = [("struct_bytes", C.c_uint), ("min_range", C.c_float), ("max_range", C.c_float), ("carve", C.c_int)]


_SIGS = {
    "xs_tsdf_sample_points": (C.c_int, [C.c_longlong, _vp, _f32p, _vp, _vp, _vp, _sz, _i32p, C.c_float, C.POINTER(SampleOpts), _vp, _vp, _vp, _vp, _vp, _vp]),
    "xs_tsdf_sample_depth": (C.c_int, [_vp, _sz, C.c_int, C.c_int, _f32p, _f32p, _f32p, _vp, _vp, _vp, _sz, _i32p, C.c_float, C.POINTER(SampleOpts), _vp, _vp, _vp,
                                       _vp, _vp, _vp]),
    "xs_render_workspace_bytes": (_sz, [_i32p]),
    "xs_render_mask_build": (C.c_int, [_vp, _vp, _sz, _i32p, C.c_int, _vp, _vp]),
    "xs_render_views": (C.c_int, [C.c_int, _f32p, _f32p, _f32p, C.c_int, C.c_int, _vp, _vp, _sz, _i32p, C.c_float, C.POINTER(RenderOpts), _vp, _vp, _vp, _vp,
                                  _vp, _vp, _vp]),
    "xs_view_grid_bytes": (_sz, [_i32p]),
    "xs_view_grid_build": (C.c_int, [_vp, _vp, _sz, _i32p, C.c_int, _vp, _vp]),
    "xs_view_grid_expand": (C.c_int, [_vp, _i32p, _vp, _vp]),
    "xs_score_views": (C.c_int, [C.c_int, _f32p, _f32p, _f32p, C.c_int, C.c_int, _i32p, C.c_float, _vp, C.POINTER(ViewOpts), _vp, _vp]),
    "xs_clearance_bytes": (_sz, [_i32p]),
    "xs_clearance_workspace_bytes": (_sz, [_i32p]),
    "xs_clearance_build": (C.c_int, [_vp, _i32p, C.c_int, C.c_int, _vp, _vp, _vp]),
    "xs_reach_bytes": (_sz, [_i32p]),
    "xs_reach_passable": (C.c_int, [_vp, _vp, _i32p, C.c_int, _vp, _vp]),
    "xs_reach_flood": (C.c_int, [_vp, _vp, _i32p, C.c_int, _i32p, C.c_int, _vp, _i32p, _vp]),
    "xs_reach_expand": (C.c_int, [_vp, _i32p, C.c_int, _vp, _vp]),
    "xs_reach_query": (C.c_int, [C.c_int, _vp, _i32p, C.c_float, _vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp]),
    "xs_travel_bytes": (_sz, [_i32p]),
    "xs_travel_workspace_bytes": (_sz, []),
    "xs_travel_build": (C.c_int, [_vp, _i32p, _i32p, C.c_int, C.c_int, _vp, _vp, _i32p, _vp]),
    "xs_travel_query": (C.c_int, [C.c_int, _vp, _i32p, _vp, _vp, _vp]),
    "xs_travel_path": (C.c_int, [C.c_int, _vp, _i32p, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    "xs_frontier_mask_bytes": (_sz, [_i32p]),
    "xs_frontier_label_bytes": (_sz, [_i32p]),
    "xs_frontier_workspace_bytes": (_sz, [_i32p, C.c_int]),
    "xs_frontier_mask": (C.c_int, [_vp, _i32p, _vp, _vp]),
    "xs_frontier_label": (C.c_int, [_vp, _i32p, C.c_int, _vp, _vp, _i32p, _vp]),
    "xs_frontier_clusters": (C.c_int, [_vp, _vp, _i32p, C.c_int, _vp, _vp, C.POINTER(C.c_uint), _vp, _vp]),
    "xs_frontier_expand": (C.c_int, [_vp, _i32p, _vp, _vp]),
    "xs_integrate_scaled_ex2": (C.c_int, [_vp, _sz, C.c_int, C.c_int, _f32p, C.c_int, _i32p, C.c_float, _f32p, _f32p, C.c_float, _vp, _vp, _vp,
                                         _sz, C.c_float, C.c_int, C.c_int, _vp, _vp, _vp, C.POINTER(IntegrateOpts), _vp]),
    "xs_integrate_classify_ex": (C.c_int, [C.c_int, C.c_int, _f32p, _i32p, C.c_float, _f32p, _f32p, C.c_float, C.c_int, C.c_int, _vp, _vp,
                                           C.c_float, C.POINTER(IntegrateOpts), _vp]),
    "xs_raycast_ex": (C.c_int, [_f32p, _f32p, _f32p, _f32p, _f32p, C.c_float, _i32p, C.c_float, _vp, _vp, _sz, _vp, _vp, _sz,
                                C.c_int, C.c_int, _vp, _vp, C.POINTER(RaycastOpts), _vp]),
    "xs_raycast_slab_ex": (C.c_int, [_f32p, _f32p, _f32p, _f32p, _f32p, C.c_float, _i32p, C.c_float, _vp, _vp, _sz, C.c_int, C.c_int,
                                     C.c_int, C.c_int, _vp, _vp, _sz, C.c_int, C.c_int, _vp, C.POINTER(RaycastOpts), _vp]),
    "xs_resize_pyramid_ex": (C.c_int, [_vp, _vp, _sz, C.c_int, C.c_int, _vp, _vp, _sz, _vp, _vp, _sz, _vp, _vp]),
    "xs_last_error": (C.c_char_p, []),
    "xs_abi_version": (C.c_int, []),
    "xs_init_volume": (C.c_int, [_vp, _vp, _vp, _sz, _i32p, C.c_int, C.c_int, _vp]),
    "xs_scale_depth": (C.c_int, [_vp, _sz, C.c_int, C.c_int, _vp, _sz, _vp]),
    "xs_integrate_tsdf_volume": (C.c_int, [_vp, _sz, C.c_int, C.c_int, _f32p, C.c_int, _i32p, C.c_float, _f32p, _f32p, C.c_float,
                                           _vp, _vp, _vp, _sz, _vp, _sz, C.c_float, C.c_int, C.c_int, _vp, _vp]),
    "xs_integrate_scaled": (C.c_int, [_vp, _sz, C.c_int, C.c_int, _f32p, C.c_int, _i32p, C.c_float, _f32p, _f32p, C.c_float,
                                      _vp, _vp, _vp, _sz, C.c_float, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "xs_integrate_scaled_ex": (C.c_int, [_vp, _sz, C.c_int, C.c_int, _f32p, C.c_int, _i32p, C.c_float, _f32p, _f32p, C.c_float, _vp, _vp, _vp,
                                        _sz, C.c_float, C.c_int, C.c_int, _vp, _vp, _vp, C.c_uint, _vp]),
    "xs_integrate_workspace_clear": (C.c_int, [_vp, _vp]),
    "xs_integrate_fold_counts": (C.c_int, [_vp, _vp, _vp]),
    "xs_integrate_classify": (C.c_int, [C.c_int, C.c_int, _f32p, _i32p, C.c_float, _f32p, _f32p, C.c_float, C.c_int, C.c_int, _vp, _vp,
                                        C.c_float, C.c_uint, _vp]),
    "xs_integrate_list_covers": (C.c_int, [C.c_int, C.c_int, _f32p, _i32p, C.c_float, _f32p, _f32p, C.c_float, _f32p, _f32p]),
    "xs_integrate_workspace_bytes": (_sz, [_i32p, C.c_int]),
    "xs_scale_depth_max": (C.c_int, [_vp, _sz, C.c_int, C.c_int, _vp, _sz, _vp, _vp]),
    "xs_scale_depth_tiles": (C.c_int, [_vp, _sz, C.c_int, C.c_int, _vp, _sz, _vp, _vp, _vp]),
    "xs_depth_tiles": (C.c_int, [_vp, _sz, C.c_int, C.c_int, _vp, _vp]),
    "xs_depth_tiles_bytes": (_sz, [C.c_int, C.c_int]),
    "xs_tsdf_reduce_workspace_bytes": (_sz, []),
    "xs_tsdf_band_segs_bytes": (_sz, [_i32p, C.c_int, C.c_int]),
    "xs_tsdf_band_build": (C.c_int, [_vp, _i32p, C.c_int, C.c_int, C.POINTER(BandIndex), _vp]),
    "xs_tsdf_band_workspace_bytes": (_sz, [C.c_int]),
    "xs_tsdf_gauss_newton_terms_band": (C.c_int, [C.c_int, C.POINTER(_vp), _sz, C.c_int, C.c_int, _f32p, C.c_float, _f32p, _f32p, C.c_float,
                                                  C.POINTER(BandIndex), _vp, _vp, _vp]),
    "xs_tsdf_pose_hessian_workspace_bytes": (_sz, [C.c_int]),
    "xs_tsdf_pose_hessian_band": (C.c_int, [C.c_int, C.POINTER(_vp), _sz, C.c_int, C.c_int, _f32p, C.c_float, _f32p, _f32p, C.c_float,
                                            C.POINTER(BandIndex), _vp, _vp, _vp]),
    "xs_tsdf_score_poses_workspace_bytes": (_sz, [C.c_int]),
    "xs_tsdf_score_poses_band": (C.c_int, [C.c_int, _vp, _sz, C.c_int, C.c_int, _f32p, C.c_float, _f32p, _f32p, C.c_float, C.POINTER(BandIndex), _vp,
                                           _vp, _vp]),
    "xs_tsdf_reduce_workspace_init": (C.c_int, [_vp, _vp]),
    "xs_compute_local_tsdf_hessian": (C.c_int, [_vp, _sz, C.c_int, C.c_int, _f32p, _i32p, C.c_float, _f32p, _f32p, C.c_float, _vp,
                                                _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    "xs_compute_local_tsdf_loss": (C.c_int, [_vp, _sz, C.c_int, C.c_int, _f32p, _i32p, C.c_float, _f32p, _f32p, C.c_float, _vp,
                                             _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    "xs_bilateral_filter": (C.c_int, [_vp, _sz, C.c_int, C.c_int, _vp, _sz, _vp]),
    "xs_pyr_down": (C.c_int, [_vp, _sz, C.c_int, C.c_int, _vp, _sz, _vp]),
    "xs_create_vmap": (C.c_int, [_f32p, _vp, _sz, C.c_int, C.c_int, _vp, _sz, _vp]),
    "xs_create_nmap": (C.c_int, [_vp, _vp, _sz, C.c_int, C.c_int, _vp]),
    "xs_create_vnmaps": (C.c_int, [C.c_int, _f32p, C.POINTER(_vp), C.POINTER(_sz), C.c_int, C.c_int, C.POINTER(_vp), C.POINTER(_vp),
                                   C.POINTER(_sz), _vp]),
    "xs_create_vnmaps_real": (C.c_int, [C.c_int, _f32p, C.POINTER(_vp), C.POINTER(_sz), C.c_int, C.c_int, C.POINTER(_vp), C.POINTER(_vp),
                                        C.POINTER(_sz), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_sz), _vp]),
    "xs_resize_vmap": (C.c_int, [_vp, _sz, C.c_int, C.c_int, _vp, _sz, _vp]),
    "xs_resize_nmap": (C.c_int, [_vp, _sz, C.c_int, C.c_int, _vp, _sz, _vp]),
    "xs_raycast": (C.c_int, [_f32p, _f32p, _f32p, _f32p, _f32p, C.c_float, _i32p, C.c_float, _vp, _vp, _sz, _vp, _vp, _sz,
                             C.c_int, C.c_int, _vp, _vp, _vp]),
    "xs_raycast_slab": (C.c_int, [_f32p, _f32p, _f32p, _f32p, _f32p, C.c_float, _i32p, C.c_float, _vp, _vp, _sz, C.c_int, C.c_int,
                                  C.c_int, C.c_int, _vp, _vp, _sz, C.c_int, C.c_int, _vp, _vp]),
    "xs_raycast_compose_mask": (C.c_int, [_vp, _vp, _vp, _vp, _sz, C.c_int, C.c_int, _vp]),
    "xs_raycast_compose_finish": (C.c_int, [_vp, _vp, _vp, _sz, C.c_int, C.c_int, _vp, _vp]),
    "xs_raycast_compose_entry_bytes": (_sz, []),
    "xs_raycast_compose_pack": (C.c_int, [_vp, _vp, _vp, _vp, _sz, C.c_int, C.c_int, _vp, _vp, _vp]),
    "xs_raycast_compose_scatter": (C.c_int, [_vp, C.c_long, _vp, _vp, _sz, C.c_int, C.c_int, _vp]),
    "xs_resize_pyramid": (C.c_int, [_vp, _vp, _sz, C.c_int, C.c_int, _vp, _vp, _sz, _vp, _vp, _sz, _vp]),
    "xs_tsdf_gauss_newton_terms": (C.c_int, [_vp, _sz, C.c_int, C.c_int, _f32p, _i32p, C.c_float, _f32p, _f32p, C.c_float, _vp, C.c_int,
                                             C.c_int, _vp, _vp, _vp]),
    "xs_tsdf_gauss_newton_terms_ex": (C.c_int, [_vp, _sz, C.c_int, C.c_int, _f32p, _i32p, C.c_float, _f32p, _f32p, C.c_float, _vp, C.c_int,
                                                C.c_int, _vp, _vp, _vp, _vp]),
    "xs_gn_publish_bytes": (_sz, []),
    "xs_gn_mailbox_bytes": (_sz, []),
    "xs_gn_post_poses": (None, [_vp, _f32p, _f32p, C.c_uint, C.c_int]),
    "xs_gn_publish_sums": (C.c_int, [_vp, C.c_int, _vp, C.c_ulonglong, _vp]),
    "xs_extract_workspace_bytes": (_sz, [_i32p]),
    "xs_extract_points": (C.c_int, [_vp, _sz, _i32p, C.c_float, C.c_int, C.c_int, C.c_int, _vp, _sz, _vp, C.POINTER(_sz), C.POINTER(_sz), _vp]),
    "xs_extract_normals": (C.c_int, [_vp, _sz, _i32p, C.c_float, C.c_int, C.c_int, _vp, _sz, _vp, _vp]),
    "xs_tsdf_merge_workspace_bytes": (_sz, [_i32p, _i32p]),
    "xs_tsdf_diff_workspace_bytes": (_sz, [_i32p, _i32p]),
    "xs_tsdf_diff": (C.c_int, [_vp, _vp, _sz, _i32p, _vp, _vp, _sz, _i32p, _f32p, C.c_int, C.c_float, C.c_float, C.c_uint, _vp, _vp, _vp, _vp, _vp]),
    "xs_tsdf_pack_bricks": (_sz, [_i32p, C.c_int]),
    "xs_tsdf_pack_workspace_bytes": (_sz, [_i32p, C.c_int]),
    "xs_tsdf_pack_classify": (C.c_int, [_vp, _vp, _vp, _sz, _i32p, C.c_int, _vp, _vp, _vp, _vp]),
    "xs_tsdf_pack_offsets": (C.c_int, [_vp, _sz, _vp, _vp, _vp]),
    "xs_tsdf_pack_gather": (C.c_int, [_vp, _vp, _vp, _sz, _i32p, C.c_int, _vp, _vp, _sz, _sz, _vp, _vp]),
    "xs_tsdf_unpack": (C.c_int, [_vp, _vp, _vp, _sz, _i32p, C.c_int, _vp, _vp, _sz, _sz, _vp, _vp]),
    "xs_tsdf_merge": (C.c_int, [_vp, _vp, _vp, _sz, _i32p, C.c_int, C.c_int, _vp, _vp, _vp, _sz, _i32p, _f32p, C.c_int, C.c_int, C.c_uint, _vp, _vp, _vp]),
    "xs_tsdf_reintegrate": (C.c_int, [C.c_int, C.POINTER(ReintegrateOp), _sz, C.c_int, C.c_int, _f32p, C.c_int, _i32p, C.c_float, C.c_float, C.c_float, _vp, _vp, _vp,
                                      _sz, C.c_int, C.c_int, _vp, C.c_uint, _vp]),
    "xs_tsdf_align_workspace_bytes": (_sz, [C.c_int]),
    "xs_tsdf_align_terms": (C.c_int, [C.c_int, C.POINTER(BandIndex), _vp, _vp, _sz, _i32p, _f32p, C.c_int, C.c_float, _vp, _vp, _vp]),
    "xs_tsdf_score_transforms_workspace_bytes": (_sz, [C.c_int]),
    "xs_tsdf_score_transforms": (C.c_int, [C.c_int, C.POINTER(BandIndex), C.c_int, _vp, _vp, _sz, _i32p, _f32p, C.c_int, C.c_float, _vp, _vp, _vp]),
    "xs_tsdf_fuse_accumulator_bytes": (_sz, [_i32p]),
    "xs_tsdf_fuse_points_accumulate": (C.c_int, [C.c_longlong, _vp, _f32p, _f32p, _i32p, C.c_float, C.c_float, C.POINTER(FuseOpts), _vp, _vp, _vp]),
    "xs_tsdf_fuse_points_fold": (C.c_int, [_vp, _vp, _vp, _sz, _i32p, C.c_int, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp]),
    "xs_tsdf_register_workspace_bytes": (_sz, [C.c_int]),
    "xs_tsdf_register_terms": (C.c_int, [C.c_int, C.c_longlong, _vp, _f32p, _vp, _vp, _sz, _i32p, C.c_float, C.c_int, C.c_float, _vp, _vp, _vp]),
    "xs_tsdf_score_points_workspace_bytes": (_sz, [C.c_int]),
    "xs_tsdf_score_points": (C.c_int, [C.c_int, C.c_longlong, C.c_int, _vp, _f32p, _vp, _vp, _sz, _i32p, C.c_float, C.c_int, C.c_float, _vp, _vp, _vp]),
    "xs_mesh_workspace_bytes": (_sz, [_i32p, C.POINTER(MeshOpts)]),
    "xs_extract_mesh": (C.c_int, [_vp, _vp, _vp, _sz, _i32p, C.c_float, C.POINTER(MeshOpts), _vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp,
                                  C.POINTER(_sz), C.POINTER(_sz), _vp]),
    "xs_mesh_case_table": (C.c_int, [C.c_int, C.c_void_p]),
    "xs_icp_wait_pairs": (C.c_int, [_vp, C.c_ulonglong, _vp, C.c_longlong]),
    "xs_icp_workspace_bytes": (_sz, []),
    "xs_icp_workspace_init": (C.c_int, [_vp, _vp]),
    "xs_icp_accumulate": (C.c_int, [_f32p, _f32p, _vp, _vp, _f32p, _f32p, _f32p, _vp, _vp, _sz, C.c_int, C.c_int, C.c_float,
                                    C.c_float, C.c_int, C.c_int, _vp, _vp, _vp, C.c_ulonglong, _vp]),
    "xs_icp_pose_state_bytes": (_sz, []),
    "xs_icp_mailbox_bytes": (_sz, []),
    "xs_icp_mailbox_alloc": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    "xs_icp_mailbox_free": (C.c_int, [_vp, C.c_int]),
    "xs_icp_accumulate_posted": (C.c_int, [_vp, C.c_uint, _vp, _vp, _f32p, _f32p, _f32p, _vp, _vp, _sz, C.c_int, C.c_int, C.c_float,
                                           C.c_float, C.c_int, C.c_int, _vp, _vp, _vp, C.c_ulonglong, _vp]),
    "xs_icp_post_pose": (None, [_vp, _f32p, _f32p, C.c_uint, C.c_int]),
    "xs_icp_accumulate_real": (C.c_int, [_f32p, _f32p, _vp, _vp, _vp, _vp, _sz, _f32p, _f32p, _f32p, _vp, _vp, _sz, C.c_int, C.c_int, C.c_float,
                                         C.c_float, C.c_int, C.c_int, _vp, _vp, _vp, C.c_ulonglong, _vp]),
    "xs_icp_accumulate_posted_real": (C.c_int, [_vp, C.c_uint, _vp, _vp, _vp, _vp, _sz, _f32p, _f32p, _f32p, _vp, _vp, _sz, C.c_int, C.c_int,
                                                C.c_float, C.c_float, C.c_int, C.c_int, _vp, _vp, _vp, C.c_ulonglong, _vp]),
    "xs_icp_records_bytes": (_sz, []),
    "xs_icp_records_count": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "xs_icp_accumulate_records": (C.c_int, [_f32p, _f32p, _vp, C.c_uint, _vp, _vp, _f32p, _f32p, _f32p, _vp, _vp, _sz, C.c_int, C.c_int, C.c_float,
                                            C.c_float, C.c_int, C.c_int, _vp, C.c_ulonglong, _vp]),
    "xs_icp_sum_records": (C.c_int, [_vp, C.c_int, C.c_ulonglong, _f64p, C.c_longlong]),
    "xs_icp_gate_selftest": (C.c_int, [_vp, C.c_int, C.c_float, C.c_int, _vp, _vp]),
    "xs_icp_iterate": (C.c_int, [_f32p, _f32p, _vp, _vp, _f32p, _f32p, _f32p, _vp, _vp, _sz, C.c_int, C.c_int, C.c_float,
                                 C.c_float, _vp, _vp, _vp, _vp, _vp, _vp, C.c_ulonglong, _vp]),
    "xs_estimate_combined": (C.c_int, [_f32p, _f32p, _vp, _vp, _f32p, _f32p, _f32p, _vp, _vp, _sz, C.c_int, C.c_int, C.c_float,
                                       C.c_float, _vp, _vp, _f64p, _f64p, C.POINTER(C.c_longlong), _vp]),
    "xs_icp_unpack": (None, [_f64p, _f64p, _f64p]),
    "xs_csfd_array_op": (C.c_int, [C.c_int, C.c_int, _vp, _vp, _vp, C.c_long, _vp]),
    "xs_dcsfd_f1": (C.c_int, [_vp, _vp, _vp, C.c_long, _vp]),
    "xs_complex_table": (C.c_int, [C.c_int, C.c_int, _vp, _vp, _vp, C.c_long, _vp]),
    "xs_const_div_prepare": (C.c_uint, [C.c_float]),
    "xs_raycast_signmap_shift": (C.c_int, [_f32p, C.c_float, C.c_float]),
    "xs_signmap_bytes": (C.c_size_t, [_i32p, C.c_int]),
    "xs_signmap_reset": (C.c_int, [_vp, _i32p, C.c_int, C.c_float, _vp]),
    "xs_signmap_rebuild": (C.c_int, [_vp, _i32p, C.c_int, C.c_float, _vp, C.c_size_t, _vp]),
    "xs_signmap_rebuild_slab": (C.c_int, [_vp, _i32p, C.c_int, C.c_float, _vp, C.c_size_t, C.c_int, C.c_int, _vp]),
    "xs_const_div_state": (C.c_uint, [C.c_float]),
    "xs_const_div_enable": (C.c_int, [C.c_int]),
}


def _bind():
    for name, (res, args) in _SIGS.items():
        f = getattr(_lib, name)
        f.restype = res
        f.argtypes = args


_bind()


def const_div_prepare(c):
    """xs_const_div_prepare: the exhaustive device check that lets the kernels divide by the constant c with the short form."""
    return int(_lib.xs_const_div_prepare(float(c)))


def const_div_state(c):
    return int(_lib.xs_const_div_state(float(c)))


def const_div_enable(on):
    return int(_lib.xs_const_div_enable(int(bool(on))))


_prepared = set()


def _prep(*consts):
    """The wrappers below prepare the constants their kernels divide by, as the C++ orchestrator does in AllocateBuffers."""
    for c in consts:
        c = float(np.float32(c))
        if c not in _prepared:
            _prepared.add(c)
            _lib.xs_const_div_prepare(c)


def check(rc):
    if rc != 0:
        raise XsError(f"hip error {rc}: {_lib.xs_last_error().decode()}")


def _fa(x, n):
    a = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    assert a.size == n, (a.size, n)
    return a


def _ia(x, n):
    a = np.ascontiguousarray(x, dtype=np.int32).reshape(-1)
    assert a.size == n
    return a


def _ptr(t):
    """Device address of a torch tensor (or None / int passthrough)."""
    if t is None:
        return None
    if isinstance(t, int):
        return t
    return t.data_ptr()


def _stream(stream):
    if stream is None:
        return None
    return stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)


def abi_version():
    return _lib.xs_abi_version()


def init_volume(value, weight, grad, step_bytes, res, z0=0, z1=None, stream=None):
    r = _ia(res, 3)
    z1 = int(r[2]) if z1 is None else z1
    check(_lib.xs_init_volume(_ptr(value), _ptr(weight), _ptr(grad), step_bytes, r.ctypes.data_as(_i32p), z0, z1, _stream(stream)))


def scale_depth(depth, depth_step, rows, cols, scaled, scaled_step, stream=None):
    check(_lib.xs_scale_depth(_ptr(depth), depth_step, rows, cols, _ptr(scaled), scaled_step, _stream(stream)))


def integrate_tsdf_volume(depth, depth_step, rows, cols, intr, max_weight, res, voxel_size, Rv2c, tv2c, tranc_dist, value, weight,
                          grad, vol_step, depth_scaled, scaled_step, threshold=0.0, z0=0, z1=None, updated=None, stream=None):
    r = _ia(res, 3)
    k, R, t = _fa(intr, 4), _fa(Rv2c, 18), _fa(tv2c, 6)
    z1 = int(r[2]) if z1 is None else z1
    check(_lib.xs_integrate_tsdf_volume(_ptr(depth), depth_step, rows, cols, k.ctypes.data_as(_f32p), max_weight,
                                        r.ctypes.data_as(_i32p), voxel_size, R.ctypes.data_as(_f32p), t.ctypes.data_as(_f32p),
                                        tranc_dist, _ptr(value), _ptr(weight), _ptr(grad), vol_step, _ptr(depth_scaled), scaled_step,
                                        threshold, z0, z1, _ptr(updated), _stream(stream)))


def scale_depth_max(depth, depth_step, rows, cols, scaled, scaled_step, max_dev, stream=None):
    check(_lib.xs_scale_depth_max(_ptr(depth), depth_step, rows, cols, _ptr(scaled), scaled_step, _ptr(max_dev), _stream(stream)))


def depth_tiles_bytes(rows, cols):
    return _lib.xs_depth_tiles_bytes(rows, cols)


def scale_depth_tiles(depth, depth_step, rows, cols, scaled, scaled_step, max_dev, tiles, stream=None):
    """scale_depth_max + the per-tile depth range table {lo, hi} per 8 x 8 pixels (depth_tiles_bytes(rows, cols) bytes)."""
    check(_lib.xs_scale_depth_tiles(_ptr(depth), depth_step, rows, cols, _ptr(scaled), scaled_step, _ptr(max_dev), _ptr(tiles), _stream(stream)))


def depth_tiles(scaled, scaled_step, rows, cols, tiles, stream=None):
    check(_lib.xs_depth_tiles(_ptr(scaled), scaled_step, rows, cols, _ptr(tiles), _stream(stream)))


def integrate_scaled(depth_scaled, scaled_step, rows, cols, intr, max_weight, res, voxel_size, Rv2c, tv2c, tranc_dist, value, weight,
                     grad, vol_step, threshold=0.0, z0=0, z1=None, updated=None, depth_max=None, workspace=None, stream=None):
    r = _ia(res, 3)
    k, R, t = _fa(intr, 4), _fa(Rv2c, 18), _fa(tv2c, 6)
    z1 = int(r[2]) if z1 is None else z1
    check(_lib.xs_integrate_scaled(_ptr(depth_scaled), scaled_step, rows, cols, k.ctypes.data_as(_f32p), max_weight,
                                   r.ctypes.data_as(_i32p), voxel_size, R.ctypes.data_as(_f32p), t.ctypes.data_as(_f32p), tranc_dist,
                                   _ptr(value), _ptr(weight), _ptr(grad), vol_step, threshold, z0, z1, _ptr(updated), _ptr(depth_max),
                                   _ptr(workspace), _stream(stream)))


def integrate_scaled_ex(depth_scaled, scaled_step, rows, cols, intr, max_weight, res, voxel_size, Rv2c, tv2c, tranc_dist, value, weight,
                        grad, vol_step, flags, threshold=0.0, z0=0, z1=None, updated=None, depth_max=None, workspace=None, stream=None, **opts):
    """xs_integrate_scaled_ex2 with its options as keyword arguments (integrate_opts' fields: depth_tiles, signmap, start_event, stop_event)
    and the flags positional, as the tests write it."""
    return integrate_scaled_ex2(depth_scaled, scaled_step, rows, cols, intr, max_weight, res, voxel_size, Rv2c, tv2c, tranc_dist, value, weight, grad, vol_step,
                                integrate_opts(flags=flags, **opts), threshold=threshold, z0=z0, z1=z1, updated=updated, depth_max=depth_max,
                                workspace=workspace, stream=stream)


def integrate_opts(flags=0, depth_tiles=None, signmap=None, start_event=None, stop_event=None):
    """An xs_integrate_opts for integrate_scaled_ex2 / integrate_classify_ex (tensors or raw addresses for the pointers)."""
    o = IntegrateOpts()
    o.struct_bytes = C.sizeof(IntegrateOpts)
    o.flags = flags
    o.depth_tiles, o.signmap = _ptr(depth_tiles), _ptr(signmap)
    o.start_event = start_event.value if hasattr(start_event, "value") else start_event
    o.stop_event = stop_event.value if hasattr(stop_event, "value") else stop_event
    return o


def integrate_scaled_ex2(depth_scaled, scaled_step, rows, cols, intr, max_weight, res, voxel_size, Rv2c, tv2c, tranc_dist, value, weight,
                         grad, vol_step, opts, threshold=0.0, z0=0, z1=None, updated=None, depth_max=None, workspace=None, stream=None):
    """xs_integrate_scaled_ex2: everything the call needs in its arguments (opts: integrate_opts(...)); reads no per-thread state."""
    r = _ia(res, 3)
    k, R, t = _fa(intr, 4), _fa(Rv2c, 18), _fa(tv2c, 6)
    z1 = int(r[2]) if z1 is None else z1
    check(_lib.xs_integrate_scaled_ex2(_ptr(depth_scaled), scaled_step, rows, cols, k.ctypes.data_as(_f32p), max_weight,
                                       r.ctypes.data_as(_i32p), voxel_size, R.ctypes.data_as(_f32p), t.ctypes.data_as(_f32p), tranc_dist,
                                       _ptr(value), _ptr(weight), _ptr(grad), vol_step, threshold, z0, z1, _ptr(updated), _ptr(depth_max),
                                       _ptr(workspace), C.byref(opts), _stream(stream)))


def integrate_classify_ex(rows, cols, intr, res, voxel_size, Rv2c, tv2c, tranc_dist, workspace, opts, slack_scale=2.0, z0=0, z1=None,
                          depth_max=None, stream=None):
    r = _ia(res, 3)
    k, R, t = _fa(intr, 4), _fa(Rv2c, 18), _fa(tv2c, 6)
    check(_lib.xs_integrate_classify_ex(rows, cols, k.ctypes.data_as(_f32p), r.ctypes.data_as(_i32p), voxel_size, R.ctypes.data_as(_f32p),
                                        t.ctypes.data_as(_f32p), tranc_dist, z0, int(r[2]) if z1 is None else z1, _ptr(depth_max), _ptr(workspace),
                                        slack_scale, C.byref(opts), _stream(stream)))


def integrate_classify(rows, cols, intr, res, voxel_size, Rv2c, tv2c, tranc_dist, workspace, slack_scale=2.0, flags=0, z0=0, z1=None,
                       depth_max=None, stream=None, **opts):
    """The brick classification of an integrate call on its own, for a pose near the final one (xs_integrate_classify_ex; options — depth_tiles,
    stop_event — as keyword arguments)."""
    return integrate_classify_ex(rows, cols, intr, res, voxel_size, Rv2c, tv2c, tranc_dist, workspace, integrate_opts(flags=flags, **opts), slack_scale=slack_scale,
                                 z0=z0, z1=z1, depth_max=depth_max, stream=stream)


def integrate_list_covers(rows, cols, intr, res, voxel_size, Rv2c_list, tv2c_list, slack_scale, Rv2c, tv2c):
    r = _ia(res, 3)
    k = _fa(intr, 4)
    a, b, c, d = _fa(Rv2c_list, 18), _fa(tv2c_list, 6), _fa(Rv2c, 18), _fa(tv2c, 6)
    P = lambda x: x.ctypes.data_as(_f32p)
    return int(_lib.xs_integrate_list_covers(rows, cols, P(k), r.ctypes.data_as(_i32p), voxel_size, P(a), P(b), slack_scale, P(c), P(d)))


def integrate_workspace_clear(workspace, stream=None):
    check(_lib.xs_integrate_workspace_clear(_ptr(workspace), _stream(stream)))


def integrate_fold_counts(workspace, updated, stream=None):
    check(_lib.xs_integrate_fold_counts(_ptr(workspace), _ptr(updated), _stream(stream)))


def integrate_workspace_bytes(res, nz=None):
    r = _ia(res, 3)
    return _lib.xs_integrate_workspace_bytes(r.ctypes.data_as(_i32p), int(r[2]) if nz is None else nz)


def integrate_listed(workspace):
    """(bricks with planes to walk, other bricks) of the list the last classification left in an integrate workspace (a torch uint8
    tensor): the two runs of the list (front / back of its region) — read back from the header, for tests and probes."""
    import torch
    pair = workspace[:8].view(torch.int32).cpu().numpy()
    return int(pair[0]), int(pair[1])


def integrate_list_layout(res, nz=None):
    """Byte offsets inside an integrate workspace: (list region, entries it holds, class words, second list region)."""
    r = _ia(res, 3)
    nz = int(r[2]) if nz is None else nz
    cap = -(-int(r[0]) // 32) * -(-int(r[1]) // 8) * -(-nz // 2)
    first = 256 + 8192 * 4     # the header and the update counts' room (a word per workgroup of the brick kernel) lie in front
    list_bytes = (first + cap * 4 + 255) // 256 * 256
    class_bytes = (cap * 16 + 255) // 256 * 256
    return first, cap, list_bytes, list_bytes + class_bytes + (1 << 20)


def tsdf_reduce_workspace_init(workspace, stream=None):
    """Zero the residual kernels' workspace ticket (once after allocation; torch.zeros does the same)."""
    check(_lib.xs_tsdf_reduce_workspace_init(_ptr(workspace), _stream(stream)))


def tsdf_reduce_workspace_bytes():
    return _lib.xs_tsdf_reduce_workspace_bytes()


def compute_local_tsdf_hessian(depth_scaled, scaled_step, rows, cols, intr, res, voxel_size, Rv2c, tv2c, tranc_dist, gt, workspace, out4,
                               volumes=None, z0=0, z1=None, stream=None):
    r = _ia(res, 3)
    k, R, t = _fa(intr, 4), _fa(Rv2c, 36), _fa(tv2c, 12)
    z1 = int(r[2]) if z1 is None else z1
    vols = [_ptr(v) for v in volumes] if volumes else [None] * 4
    check(_lib.xs_compute_local_tsdf_hessian(_ptr(depth_scaled), scaled_step, rows, cols, k.ctypes.data_as(_f32p), r.ctypes.data_as(_i32p),
                                             voxel_size, R.ctypes.data_as(_f32p), t.ctypes.data_as(_f32p), tranc_dist, _ptr(gt), vols[0],
                                             vols[1], vols[2], vols[3], z0, z1, _ptr(workspace), _ptr(out4), _stream(stream)))


def compute_local_tsdf_loss(depth_scaled, scaled_step, rows, cols, intr, res, voxel_size, Rv2c, tv2c, tranc_dist, gt, workspace, out2,
                            volumes=None, z0=0, z1=None, stream=None):
    r = _ia(res, 3)
    k, R, t = _fa(intr, 4), _fa(Rv2c, 9), _fa(tv2c, 3)
    z1 = int(r[2]) if z1 is None else z1
    vols = [_ptr(v) for v in volumes] if volumes else [None] * 2
    check(_lib.xs_compute_local_tsdf_loss(_ptr(depth_scaled), scaled_step, rows, cols, k.ctypes.data_as(_f32p), r.ctypes.data_as(_i32p),
                                          voxel_size, R.ctypes.data_as(_f32p), t.ctypes.data_as(_f32p), tranc_dist, _ptr(gt), vols[0],
                                          vols[1], z0, z1, _ptr(workspace), _ptr(out2), _stream(stream)))


def bilateral_filter(src, src_step, rows, cols, dst, dst_step, stream=None):
    check(_lib.xs_bilateral_filter(_ptr(src), src_step, rows, cols, _ptr(dst), dst_step, _stream(stream)))


def pyr_down(src, src_step, src_rows, src_cols, dst, dst_step, stream=None):
    check(_lib.xs_pyr_down(_ptr(src), src_step, src_rows, src_cols, _ptr(dst), dst_step, _stream(stream)))


def create_vmap(intr, depth, depth_step, rows, cols, vmap, vmap_step, stream=None):
    k = _fa(intr, 4)
    check(_lib.xs_create_vmap(k.ctypes.data_as(_f32p), _ptr(depth), depth_step, rows, cols, _ptr(vmap), vmap_step, _stream(stream)))


def create_vnmaps(intrs, depths, depth_steps, rows0, cols0, vmaps, nmaps, map_steps, stream=None, vreal=None, nreal=None, real_steps=None):
    """Vertex + normal maps of all pyramid levels in one launch.  intrs: per-level [fx, fy, cx, cy].  vreal / nreal / real_steps:
    optionally the real parts again as float planes (xs_create_vnmaps_real)."""
    n = len(depths)
    k = np.ascontiguousarray(intrs, dtype=np.float32).reshape(-1)
    assert k.size == 4 * n
    P = lambda ts: (_vp * n)(*[_ptr(t) for t in ts])
    S = lambda xs: (_sz * n)(*[int(x) for x in xs])
    if vreal is None:
        check(_lib.xs_create_vnmaps(n, k.ctypes.data_as(_f32p), P(depths), S(depth_steps), rows0, cols0, P(vmaps), P(nmaps), S(map_steps),
                                    _stream(stream)))
    else:
        check(_lib.xs_create_vnmaps_real(n, k.ctypes.data_as(_f32p), P(depths), S(depth_steps), rows0, cols0, P(vmaps), P(nmaps), S(map_steps),
                                         P(vreal), P(nreal), S(real_steps), _stream(stream)))


def tsdf_gauss_newton_terms(depth_scaled, scaled_step, rows, cols, intr, res, voxel_size, Rv2c6, tv2c6, tranc_dist, gt, workspace, out29,
                            z0=0, z1=None, stream=None):
    r = _ia(res, 3)
    k, R, t = _fa(intr, 4), _fa(Rv2c6, 108), _fa(tv2c6, 36)
    z1 = int(r[2]) if z1 is None else z1
    check(_lib.xs_tsdf_gauss_newton_terms(_ptr(depth_scaled), scaled_step, rows, cols, k.ctypes.data_as(_f32p), r.ctypes.data_as(_i32p),
                                          voxel_size, R.ctypes.data_as(_f32p), t.ctypes.data_as(_f32p), tranc_dist, _ptr(gt), z0, z1,
                                          _ptr(workspace), _ptr(out29), _stream(stream)))


BAND_OVER_CAPACITY = -3   # XS_BAND_OVER_CAPACITY
BAND_MAX_FRAMES = 32      # XS_BAND_MAX_FRAMES


def tsdf_band_segs_bytes(res, z0=0, z1=None):
    r = _ia(res, 3)
    return int(_lib.xs_tsdf_band_segs_bytes(r.ctypes.data_as(_i32p), z0, int(r[2]) if z1 is None else z1))


def tsdf_band_build_raw(gt, res, z0, z1, keys, values, capacity, segs, stream=None):
    """xs_tsdf_band_build on caller-provided buffers: (status 0 or BAND_OVER_CAPACITY, the BandIndex)."""
    r = _ia(res, 3)
    idx = BandIndex()
    idx.keys, idx.values, idx.capacity, idx.segs = _ptr(keys), _ptr(values), int(capacity), _ptr(segs)
    rc = _lib.xs_tsdf_band_build(_ptr(gt), r.ctypes.data_as(_i32p), z0, z1, C.byref(idx), _stream(stream))
    if rc != BAND_OVER_CAPACITY:
        check(rc)
    return rc, idx


def tsdf_band_build(gt, res, z0=0, z1=None, stream=None):
    """The band index of the slab [z0, z1) of the dense map gt (pointing at plane z0): count, then fill.  Returns the BandIndex with its
    device buffers attached (.keys_t int64, .values_t float32, .segs_t int64 torch tensors), which keep them alive."""
    import torch
    r = _ia(res, 3)
    z1 = int(r[2]) if z1 is None else z1
    segs = torch.empty(max(tsdf_band_segs_bytes(r, z0, z1) // 8, 1), dtype=torch.int64, device=gt.device)
    rc, idx = tsdf_band_build_raw(gt, r, z0, z1, None, None, 0, segs, stream)
    n = int(idx.count)
    keys = torch.empty(max(n, 1), dtype=torch.int64, device=gt.device)
    values = torch.empty(max(n, 1), dtype=torch.float32, device=gt.device)
    rc, idx = tsdf_band_build_raw(gt, r, z0, z1, keys, values, n, segs, stream)
    assert rc == 0 and idx.count == n
    idx.keys_t, idx.values_t, idx.segs_t = keys, values, segs
    return idx


def tsdf_band_workspace_bytes(frames):
    return int(_lib.xs_tsdf_band_workspace_bytes(int(frames)))


def tsdf_gauss_newton_terms_band(depths_scaled, scaled_step, rows, cols, intr, voxel_size, Rv2c6xF, tv2c6xF, tranc_dist, index, workspace, out29xF,
                                 stream=None):
    """xs_tsdf_gauss_newton_terms_band: F = len(depths_scaled) frames over a built index; Rv2c6xF [F, 6, 3, 3, 2], tv2c6xF [F, 6, 3, 2];
    frame f's 29 sums land at out29xF[29 f : 29 f + 29] (float64 device tensor)."""
    F = len(depths_scaled)
    k, R, t = _fa(intr, 4), _fa(Rv2c6xF, 108 * F), _fa(tv2c6xF, 36 * F)
    P = (_vp * max(F, 1))(*[_ptr(d) for d in depths_scaled])
    check(_lib.xs_tsdf_gauss_newton_terms_band(F, P, scaled_step, rows, cols, k.ctypes.data_as(_f32p), voxel_size, R.ctypes.data_as(_f32p),
                                               t.ctypes.data_as(_f32p), tranc_dist, C.byref(index), _ptr(workspace), _ptr(out29xF), _stream(stream)))


def tsdf_pose_hessian_workspace_bytes(frames):
    return int(_lib.xs_tsdf_pose_hessian_workspace_bytes(int(frames)))


def tsdf_pose_hessian_band(depths_scaled, scaled_step, rows, cols, intr, voxel_size, Rv2c21xF, tv2c21xF, tranc_dist, index, workspace, out29xF,
                           stream=None):
    """xs_tsdf_pose_hessian_band: F = len(depths_scaled) frames over a built index; Rv2c21xF [F, 21, 3, 3, 4], tv2c21xF [F, 21, 3, 4] (the
    dual-complex poses of the generator pairs a <= b); frame f's 29 raw sums land at out29xF[29 f : 29 f + 29] (float64 device tensor)."""
    F = len(depths_scaled)
    k, R, t = _fa(intr, 4), _fa(Rv2c21xF, 21 * 36 * F), _fa(tv2c21xF, 21 * 12 * F)
    P = (_vp * max(F, 1))(*[_ptr(d) for d in depths_scaled])
    check(_lib.xs_tsdf_pose_hessian_band(F, P, scaled_step, rows, cols, k.ctypes.data_as(_f32p), voxel_size, R.ctypes.data_as(_f32p),
                                         t.ctypes.data_as(_f32p), tranc_dist, C.byref(index), _ptr(workspace), _ptr(out29xF), _stream(stream)))


SCORE_MAX_POSES = 4096   # XS_SCORE_MAX_POSES


def tsdf_score_poses_workspace_bytes(poses):
    return int(_lib.xs_tsdf_score_poses_workspace_bytes(int(poses)))


def tsdf_score_poses_band(depth_scaled, scaled_step, rows, cols, intr, voxel_size, Rv2cxP, tv2cxP, tranc_dist, index, workspace, out2xP, stream=None):
    """xs_tsdf_score_poses_band: one depth frame at P real poses over a built index; Rv2cxP [P, 3, 3], tv2cxP [P, 3]; pose p's {sum loss,
    count} land at out2xP[2 p : 2 p + 2] (float64 device tensor)."""
    R = np.ascontiguousarray(Rv2cxP, dtype=np.float32).reshape(-1)
    P = R.size // 9
    k, R, t = _fa(intr, 4), _fa(R, 9 * P), _fa(tv2cxP, 3 * P)
    check(_lib.xs_tsdf_score_poses_band(P, _ptr(depth_scaled), scaled_step, rows, cols, k.ctypes.data_as(_f32p), voxel_size, R.ctypes.data_as(_f32p),
                                        t.ctypes.data_as(_f32p), tranc_dist, C.byref(index), _ptr(workspace), _ptr(out2xP), _stream(stream)))


VIEW_MAX_POSES = 4096   # XS_VIEW_MAX_POSES
VIEW_UNKNOWN, VIEW_FREE, VIEW_OCCUPIED = 0, 1, 2


def view_opts(rays=(0, 0), t_near=0.0, t_far=0.0, step=None):
    """An xs_view_opts; zeros (step None) are the library's defaults: 80 x 60 rays, depths 0.2 .. 5.0, a voxel per step."""
    o = ViewOpts()
    o.struct_bytes = C.sizeof(ViewOpts)
    o.rays_x, o.rays_y = int(rays[0]), int(rays[1])
    o.t_near, o.t_far, o.step = float(t_near), float(t_far), 0.0 if step is None else float(step)
    return o


def view_grid_bytes(res):
    """xs_view_grid_bytes (host only): the observation grid's buffer for a resolution, 0 for an invalid one."""
    r = np.ascontiguousarray(res, dtype=np.int32).reshape(-1)
    assert r.size == 3
    return int(_lib.xs_view_grid_bytes(r.ctypes.data_as(_i32p)))


def view_grid_build(value, weight, vol_step, res, grid, min_weight=1, stream=None):
    """xs_view_grid_build: the two-bit observation grid of the whole volume into `grid` (view_grid_bytes(res) bytes of device memory)."""
    r = _ia(res, 3)
    check(_lib.xs_view_grid_build(_ptr(value), _ptr(weight), vol_step, r.ctypes.data_as(_i32p), int(min_weight), _ptr(grid), _stream(stream)))


def view_grid_expand(grid, res, states, stream=None):
    """xs_view_grid_expand: one byte per voxel into `states` (X * Y * Z uint8 on the device, index (z * Y + y) * X + x)."""
    r = _ia(res, 3)
    check(_lib.xs_view_grid_expand(_ptr(grid), r.ctypes.data_as(_i32p), _ptr(states), _stream(stream)))


def score_views(Rc2vxP, tc2vxP, intr, rows, cols, res, voxel_size, grid, out4xP, opts=None, stream=None):
    """xs_score_views: P real camera-to-volume poses Rc2vxP [P, 3, 3], tc2vxP [P, 3] against a built grid in one launch; pose p's
    {unknown, free, hits, frontier} land at out4xP[4 p : 4 p + 4] (uint32 device tensor of 4 P words).  opts: view_opts(...) or None."""
    R = np.ascontiguousarray(Rc2vxP, dtype=np.float32).reshape(-1)
    P = R.size // 9
    k, R, t, r = _fa(intr, 4), _fa(R, 9 * P), _fa(tc2vxP, 3 * P), _ia(res, 3)
    check(_lib.xs_score_views(P, R.ctypes.data_as(_f32p), t.ctypes.data_as(_f32p), k.ctypes.data_as(_f32p), rows, cols, r.ctypes.data_as(_i32p),
                              voxel_size, _ptr(grid), C.byref(opts) if opts is not None else None, _ptr(out4xP), _stream(stream)))


RENDER_MAX_VIEWS = 64   # XS_RENDER_MAX_VIEWS
RENDER_HEADER_BYTES, RENDER_STAGING_BYTES = 256, 64 * 12 * 4   # the workspace in front of the mask words (host/render_host.hpp)


def render_opts(t_near=0.0, t_far=0.0, step=None, min_weight=1, cull=True, shade_mode=0):
    """An xs_render_opts; zeros (step None) are the library's defaults: depths 0.2 .. 5.0, a voxel per step."""
    o = RenderOpts()
    o.struct_bytes = C.sizeof(RenderOpts)
    o.t_near, o.t_far, o.step = float(t_near), float(t_far), 0.0 if step is None else float(step)
    o.min_weight, o.cull, o.shade_mode = int(min_weight), int(bool(cull)), int(shade_mode)
    return o


def render_workspace_bytes(res):
    """xs_render_workspace_bytes (host only): header, pose staging area and brick mask for a resolution; 0 for an unusable one."""
    return int(_lib.xs_render_workspace_bytes(_res3(res).ctypes.data_as(_i32p)))


def render_mask_build(value, weight, vol_step, res, workspace, min_weight=1, stream=None):
    """xs_render_mask_build: one bit per brick of 8 x 8 x 8 voxels (any value < 0 with weight >= min_weight) into the workspace, and its header."""
    r = _ia(res, 3)
    check(_lib.xs_render_mask_build(_ptr(value), _ptr(weight), vol_step, r.ctypes.data_as(_i32p), int(min_weight), _ptr(workspace), _stream(stream)))


def render_views(Rc2vxP, tc2vxP, intr, rows, cols, value, weight, vol_step, res, voxel_size, workspace, opts=None, depth=None, depth_u16=None, normal=None,
                 shade=None, counts=None, views=None, stream=None):
    """xs_render_views: P real camera-to-volume poses Rc2vxP [P, 3, 3], tc2vxP [P, 3] render rows x cols images of the volume in one launch into
    the device tensors that are given: depth float32 [P, rows, cols], depth_u16 uint16 [P, rows, cols], normal float32 [P, 3, rows, cols], shade
    uint8 [P, rows, cols], counts uint32 [P, 4] = {hit, backface, rejected, none}.  opts: render_opts(...) or None.  A None among the host
    arrays goes through as a null pointer (`views` then says how many were meant).  Waits for the stream once when opts.cull is set."""
    def fp(x):
        if x is None:
            return None, None
        a = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        return a, a.ctypes.data_as(_f32p)
    R, Rp = fp(Rc2vxP)
    t, tp = fp(tc2vxP)
    k, kp = fp(intr)
    r = None if res is None else _ia(res, 3)
    P = int(views) if views is not None else R.size // 9
    check(_lib.xs_render_views(P, Rp, tp, kp, int(rows), int(cols), _ptr(value), _ptr(weight), vol_step, None if r is None else r.ctypes.data_as(_i32p),
                               voxel_size, C.byref(opts) if opts is not None else None, _ptr(workspace), _ptr(depth), _ptr(depth_u16), _ptr(normal),
                               _ptr(shade), _ptr(counts), _stream(stream)))


SAMPLE_OUTSIDE, SAMPLE_UNSEEN, SAMPLE_OK, SAMPLE_NO_DEPTH = 0, 1, 2, 3   # the status byte of the sample calls, and the index into their counts
SAMPLE_MAX_POINTS = 1 << 30


def sample_opts(min_weight=1):
    """An xs_sample_opts."""
    o = SampleOpts()
    o.struct_bytes = C.sizeof(SampleOpts)
    o.min_weight = int(min_weight)
    return o


def _f32_or_null(x):
    if x is None:
        return None, None
    a = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    return a, a.ctypes.data_as(_f32p)


def sample_points(n, points, value, weight, vol_step, res, voxel_size, xform12=None, grad=None, opts=None, status=None, value_out=None, dvalue=None,
                  gradient=None, counts=None, stream=None):
    """xs_tsdf_sample_points: n points (device float32 [n, 3], metres; xform12 = row-major R then t takes them to the volume frame, None: as they
    are) sampled in the volume in one launch into the device tensors that are given: status uint8 [n] (SAMPLE_*), value_out float32 [n], dvalue
    float32 [n] (the grad array interpolated alike), gradient float32 [n, 3] (value per metre), counts uint64 [4] = {outside, unseen, ok,
    no_depth}.  opts: sample_opts(...) or None.  A None among the host arrays goes through as a null pointer."""
    m, mp = _f32_or_null(xform12)
    r = None if res is None else _ia(res, 3)
    check(_lib.xs_tsdf_sample_points(int(n), _ptr(points), mp, _ptr(value), _ptr(weight), _ptr(grad), vol_step, None if r is None else r.ctypes.data_as(_i32p),
                                     voxel_size, C.byref(opts) if opts is not None else None, _ptr(status), _ptr(value_out), _ptr(dvalue), _ptr(gradient),
                                     _ptr(counts), _stream(stream)))


def sample_depth(depth, depth_step, rows, cols, intr, Rc2v, tc2v, value, weight, vol_step, res, voxel_size, grad=None, opts=None, status=None, value_out=None,
                 dvalue=None, gradient=None, counts=None, stream=None):
    """xs_tsdf_sample_depth: sample_points at the points of a depth image's pixels (device u16 millimetres, depth_step bytes per row) seen from the
    real camera-to-volume pose Rc2v [3, 3], tc2v [3] with intrinsics intr (fx, fy, cx, cy): status and the floats are images [rows, cols], gradient
    [3, rows, cols]; a pixel with a depth outside 200 .. 5000 is SAMPLE_NO_DEPTH."""
    k, kp = _f32_or_null(intr)
    R, Rp = _f32_or_null(Rc2v)
    t, tp = _f32_or_null(tc2v)
    r = None if res is None else _ia(res, 3)
    check(_lib.xs_tsdf_sample_depth(_ptr(depth), depth_step, int(rows), int(cols), kp, Rp, tp, _ptr(value), _ptr(weight), _ptr(grad), vol_step,
                                    None if r is None else r.ctypes.data_as(_i32p), voxel_size, C.byref(opts) if opts is not None else None, _ptr(status),
                                    _ptr(value_out), _ptr(dvalue), _ptr(gradient), _ptr(counts), _stream(stream)))


CLEARANCE_MAX_RADIUS, REACH_MAX_SEEDS, REACH_MAX_SNAP = 255, 64, 16   # XS_CLEARANCE_MAX_RADIUS, XS_REACH_MAX_SEEDS, XS_REACH_MAX_SNAP


def _res3(res):
    r = np.ascontiguousarray(res, dtype=np.int32).reshape(-1)
    assert r.size == 3
    return r


def clearance_bytes(res):
    """xs_clearance_bytes (host only): the clearance field, 2 bytes per voxel; 0 for an invalid resolution."""
    return int(_lib.xs_clearance_bytes(_res3(res).ctypes.data_as(_i32p)))


def clearance_workspace_bytes(res):
    """xs_clearance_workspace_bytes (host only): the intermediates of xs_clearance_build; 0 for an invalid resolution."""
    return int(_lib.xs_clearance_workspace_bytes(_res3(res).ctypes.data_as(_i32p)))


def reach_bytes(res):
    """xs_reach_bytes (host only): the reached and passable words of a resolution; 0 for an invalid one."""
    return int(_lib.xs_reach_bytes(_res3(res).ctypes.data_as(_i32p)))


def clearance_build(grid, res, max_radius, unknown_blocks, workspace, field, stream=None):
    """xs_clearance_build: field[(z Y + y) X + x] (uint16 device tensor) = min(d^2, R^2) to the nearest obstacle of a built observation grid."""
    r = _res3(res)
    check(_lib.xs_clearance_build(_ptr(grid), r.ctypes.data_as(_i32p), int(max_radius), int(unknown_blocks), _ptr(workspace), _ptr(field), _stream(stream)))


def reach_passable(grid, field, res, r2, reach, stream=None):
    """xs_reach_passable: the passable words (FREE and field >= r2) of `reach` alone."""
    r = _res3(res)
    check(_lib.xs_reach_passable(_ptr(grid), _ptr(field), r.ctypes.data_as(_i32p), int(r2), _ptr(reach), _stream(stream)))


def reach_flood(grid, field, res, r2, seeds, reach, stream=None):
    """xs_reach_flood: the passable voxels 6-connected to one of `seeds` ([N, 3] integer voxels (x, y, z), N = 1 .. 64) into the reached
    words of `reach`.  Synchronises the stream.  Returns the number of rounds."""
    r = _res3(res)
    s = np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1)
    assert s.size % 3 == 0
    rounds = C.c_int(-1)
    check(_lib.xs_reach_flood(_ptr(grid), _ptr(field), r.ctypes.data_as(_i32p), int(r2), s.ctypes.data_as(_i32p), s.size // 3, _ptr(reach),
                              C.byref(rounds), _stream(stream)))
    return int(rounds.value)


def reach_expand(reach, res, out, passable=False, stream=None):
    """xs_reach_expand: one byte (0 or 1) per voxel into `out` from the reached words, or the passable ones."""
    r = _res3(res)
    check(_lib.xs_reach_expand(_ptr(reach), r.ctypes.data_as(_i32p), int(bool(passable)), _ptr(out), _stream(stream)))


def reach_query(n, points, res, voxel_size, reach, field, reachable, clear2, snap=0, over_passable=False, voxel=None, stream=None):
    """xs_reach_query: n points (float32 device tensor of 3 n metres in volume coordinates) -> reachable (uint8) and clear2 (uint16); voxel
    (optional int32 device tensor of 3 n) receives the answering voxels."""
    r = _res3(res)
    check(_lib.xs_reach_query(int(n), _ptr(points), r.ctypes.data_as(_i32p), float(voxel_size), _ptr(reach), int(bool(over_passable)), _ptr(field),
                              int(snap), _ptr(reachable), _ptr(clear2), _ptr(voxel), _stream(stream)))


TRAVEL_NONE, TRAVEL_MAX, TRAVEL_MAX_TARGETS = 65535, 65534, 64   # XS_TRAVEL_NONE, XS_TRAVEL_MAX, XS_TRAVEL_MAX_TARGETS


def travel_bytes(res):
    """xs_travel_bytes (host only): the travel field, 2 bytes per voxel; 0 for an invalid resolution."""
    return int(_lib.xs_travel_bytes(_res3(res).ctypes.data_as(_i32p)))


def travel_workspace_bytes():
    """xs_travel_workspace_bytes (host only): the control words of xs_travel_build."""
    return int(_lib.xs_travel_workspace_bytes())


def travel_build(reach, res, seeds, limit, travel, workspace, stream=None):
    """xs_travel_build: travel[(z Y + y) X + x] (uint16 device tensor) = the least <3, 4, 5> chamfer cost without corner cutting from one of
    `seeds` ([N, 3] integer voxels, N = 1 .. 64) over the reached words of a flooded `reach`, 65535 beyond `limit` (0 .. 65534) or where
    not reached.  Synchronises the stream.  Returns the number of rounds."""
    r = _res3(res)
    s = np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1)
    assert s.size % 3 == 0
    rounds = C.c_int(0)
    check(_lib.xs_travel_build(_ptr(reach), r.ctypes.data_as(_i32p), s.ctypes.data_as(_i32p), s.size // 3, int(limit), _ptr(travel), _ptr(workspace),
                               C.byref(rounds), _stream(stream)))
    return int(rounds.value)


def travel_query(n, voxels, res, travel, out, stream=None):
    """xs_travel_query: n integer voxels (int32 device tensor of 3 n) -> out (uint16): travel[v], 65535 outside the volume."""
    r = _res3(res)
    check(_lib.xs_travel_query(int(n), _ptr(voxels), r.ctypes.data_as(_i32p), _ptr(travel), _ptr(out), _stream(stream)))


def travel_path(n, targets, res, reach, travel, limit, capacity, path, lengths, stream=None):
    """xs_travel_path: n targets (1 .. 64; int32 device tensor of 3 n) -> path (int32, n x capacity x 3: the voxels from the target down to
    the seed, slots beyond a path's length untouched) and lengths (int32 [n], the full lengths)."""
    r = _res3(res)
    check(_lib.xs_travel_path(int(n), _ptr(targets), r.ctypes.data_as(_i32p), _ptr(reach), _ptr(travel), int(limit), int(capacity), _ptr(path),
                              _ptr(lengths), _stream(stream)))


FRONTIER_NONE, FRONTIER_RECORD_WORDS = 0xFFFFFFFF, 8   # XS_FRONTIER_NONE, XS_FRONTIER_RECORD_WORDS


def frontier_mask_bytes(res):
    """xs_frontier_mask_bytes (host only): the frontier mask, 8 bytes per brick of 4 x 4 x 4 voxels; 0 for an invalid resolution."""
    return int(_lib.xs_frontier_mask_bytes(_res3(res).ctypes.data_as(_i32p)))


def frontier_label_bytes(res):
    """xs_frontier_label_bytes (host only): the labels, 4 bytes per voxel; 0 for an invalid resolution."""
    return int(_lib.xs_frontier_label_bytes(_res3(res).ctypes.data_as(_i32p)))


def frontier_workspace_bytes(res, capacity=0):
    """xs_frontier_workspace_bytes (host only): the control words of xs_frontier_label plus what xs_frontier_clusters needs for `capacity`
    records; 0 for an invalid resolution or a negative capacity."""
    return int(_lib.xs_frontier_workspace_bytes(_res3(res).ctypes.data_as(_i32p), int(capacity)))


def frontier_mask(grid, res, mask, stream=None):
    """xs_frontier_mask: one 64-bit word per brick into `mask`: the FREE voxels of a built observation grid with an UNKNOWN face neighbour."""
    r = _res3(res)
    check(_lib.xs_frontier_mask(_ptr(grid), r.ctypes.data_as(_i32p), _ptr(mask), _stream(stream)))


def frontier_label(mask, res, cell, labels, workspace, stream=None):
    """xs_frontier_label: labels[(z Y + y) X + x] (uint32 device tensor) = the lowest linear index of the voxel's cluster (26-adjacency within
    cells of `cell` voxels; 0: the whole volume), 0xFFFFFFFF off the frontier.  Synchronises the stream.  Returns the number of rounds."""
    r = _res3(res)
    rounds = C.c_int(0)
    check(_lib.xs_frontier_label(_ptr(mask), r.ctypes.data_as(_i32p), int(cell), _ptr(labels), _ptr(workspace), C.byref(rounds), _stream(stream)))
    return int(rounds.value)


def frontier_clusters(mask, labels, res, capacity, records, count, workspace, stream=None):
    """xs_frontier_clusters: one record of 8 uint64 {label, count, sum x, sum y, sum z, packed min, packed max, 0} per cluster in ascending label
    order into `records` (capacity x 8) when the number of clusters is <= capacity; `count` (uint32 device tensor of one word) always receives
    that number, which is also returned.  Synchronises the stream."""
    r = _res3(res)
    n = C.c_uint(0)
    check(_lib.xs_frontier_clusters(_ptr(mask), _ptr(labels), r.ctypes.data_as(_i32p), int(capacity), _ptr(records), _ptr(count), C.byref(n), _ptr(workspace),
                                    _stream(stream)))
    return int(n.value)


def frontier_expand(mask, res, out, stream=None):
    """xs_frontier_expand: one byte (0 or 1) per voxel into `out` from the frontier mask."""
    r = _res3(res)
    check(_lib.xs_frontier_expand(_ptr(mask), r.ctypes.data_as(_i32p), _ptr(out), _stream(stream)))



class GnOpts(C.Structure):
    """xs_gn_opts (include/xslam_amd.h)"""
    _fields_ = [("struct_bytes", C.c_uint), ("mailbox_seq", C.c_uint), ("pose_mailbox", C.c_void_p), ("publish_host", C.c_void_p),
                ("publish_seq", C.c_ulonglong)]


def tsdf_gauss_newton_terms_ex(depth_scaled, scaled_step, rows, cols, intr, res, voxel_size, Rv2c6, tv2c6, tranc_dist, gt, workspace, out29,
                               z0=0, z1=None, stream=None, pose_mailbox=None, mailbox_seq=0, publish_host=None, publish_seq=0):
    """xs_tsdf_gauss_newton_terms_ex: the pass with the loop protocol's options.  Rv2c6 / tv2c6 None: the launch takes its six poses from
    `pose_mailbox` (gn_post_poses); publish_host: a pinned host tensor of gn_publish_bytes() bytes the last workgroup writes."""
    r = _ia(res, 3)
    k = _fa(intr, 4)
    z1 = int(r[2]) if z1 is None else z1
    o = GnOpts()
    o.struct_bytes = C.sizeof(GnOpts)
    o.mailbox_seq, o.pose_mailbox, o.publish_host, o.publish_seq = mailbox_seq, _ptr(pose_mailbox), _ptr(publish_host), publish_seq
    if Rv2c6 is None:
        pR = pt = None
    else:
        R, t = _fa(Rv2c6, 108), _fa(tv2c6, 36)
        pR, pt = R.ctypes.data_as(_f32p), t.ctypes.data_as(_f32p)
    check(_lib.xs_tsdf_gauss_newton_terms_ex(_ptr(depth_scaled), scaled_step, rows, cols, k.ctypes.data_as(_f32p), r.ctypes.data_as(_i32p),
                                             voxel_size, pR, pt, tranc_dist, _ptr(gt), z0, z1, _ptr(workspace), _ptr(out29), C.byref(o),
                                             _stream(stream)))


def gn_publish_bytes():
    return int(_lib.xs_gn_publish_bytes())


def gn_post_poses(mailbox, Rv2c6, tv2c6, mailbox_seq, cmd=0):
    """Host side of the six-pose mailbox (an icp_mailbox_alloc address): cmd 0 = run with these poses, 1 = leave."""
    if Rv2c6 is None:
        _lib.xs_gn_post_poses(_ptr(mailbox), None, None, mailbox_seq, cmd)
    else:
        R, t = _fa(Rv2c6, 108), _fa(tv2c6, 36)
        _lib.xs_gn_post_poses(_ptr(mailbox), R.ctypes.data_as(_f32p), t.ctypes.data_as(_f32p), mailbox_seq, cmd)


def extract_workspace_bytes(res):
    r = _ia(res, 3)
    return _lib.xs_extract_workspace_bytes(r.ctypes.data_as(_i32p))


def extract_points(value, vol_step, res, voxel_size, points, capacity, workspace, zs0=0, z0=0, z1=None, stream=None):
    """extractPoints: fills points[capacity, 3] (CUDA float32); returns (stored, found).  Synchronises."""
    r = _ia(res, 3)
    z1 = int(r[2]) - 1 if z1 is None else z1
    cnt, found = _sz(0), _sz(0)
    check(_lib.xs_extract_points(_ptr(value), vol_step, r.ctypes.data_as(_i32p), voxel_size, zs0, z0, z1, _ptr(points), capacity,
                                 _ptr(workspace), C.byref(cnt), C.byref(found), _stream(stream)))
    return int(cnt.value), int(found.value)


def extract_normals(value, vol_step, res, voxel_size, points, n, normals, zs0=0, zs1=None, stream=None):
    r = _ia(res, 3)
    zs1 = int(r[2]) if zs1 is None else zs1
    check(_lib.xs_extract_normals(_ptr(value), vol_step, r.ctypes.data_as(_i32p), voxel_size, zs0, zs1, _ptr(points), n, _ptr(normals),
                                  _stream(stream)))


MERGE_NO_CULL = 1   # XS_MERGE_NO_CULL


def tsdf_merge_workspace_bytes(dst_res, src_res):
    """xs_tsdf_merge_workspace_bytes (host only): a header and one bit per brick of 4 x 4 x 4 source voxels; 0 for an unusable resolution."""
    return int(_lib.xs_tsdf_merge_workspace_bytes(_res3(dst_res).ctypes.data_as(_i32p), _res3(src_res).ctypes.data_as(_i32p)))


def tsdf_merge(value, weight, grad, step, res, src_value, src_weight, src_grad, src_step, src_res, xform12, min_weight=1, max_weight=100, flags=0,
               z0=0, z1=None, written=None, workspace=None, stream=None):
    """xs_tsdf_merge: resamples the source volume into planes [z0, z1) of the destination's voxel grid under xform12 (destination voxel
    indices -> continuous source voxel indices, 3 x 3 row-major then 3 offsets) and averages the two by weight.  Arrays are device tensors
    or addresses of plane 0; `written` (uint64 / int64 device word, optional) is incremented by the number of voxels written; `workspace`:
    tsdf_merge_workspace_bytes(res, src_res) bytes (None only with MERGE_NO_CULL).  No synchronisation."""
    r, s = _ia(res, 3), _ia(src_res, 3)
    m = _fa(xform12, 12)
    z1 = int(r[2]) if z1 is None else z1
    check(_lib.xs_tsdf_merge(_ptr(value), _ptr(weight), _ptr(grad), step, r.ctypes.data_as(_i32p), z0, z1, _ptr(src_value), _ptr(src_weight), _ptr(src_grad),
                             src_step, s.ctypes.data_as(_i32p), m.ctypes.data_as(_f32p), int(min_weight), int(max_weight), int(flags), _ptr(written),
                             _ptr(workspace), _stream(stream)))


REINTEGRATE_MAX_OPS = 8      # XS_REINTEGRATE_MAX_OPS
REINTEGRATE_NO_CULL = 1      # XS_REINTEGRATE_NO_CULL


def tsdf_reintegrate(ops, scaled_step, rows, cols, intr, max_weight, res, voxel_size, tranc_dist, value, weight, grad, vol_step, counts, threshold=0.0,
                     z0=0, z1=None, flags=0, stream=None):
    """xs_tsdf_reintegrate: applies the observations `ops` = [(sign, depth_scaled, Rv2c, tv2c), ...] (at most REINTEGRATE_MAX_OPS; sign -1 takes the
    observation out of the running mean, +1 puts it in; depth_scaled: a device tensor or address, the image scale_depth gives, shared pitch
    scaled_step) to planes [z0, z1) in one pass, in list order per voxel.  value / weight / grad: device tensors or addresses of the first stored
    plane z0, as integrate_scaled takes them; counts (uint64 / int64 device tensor of 4 words) is incremented by {removed, added, emptied,
    orphaned}.  The table travels in the kernel's arguments.  No synchronisation."""
    r = _ia(res, 3)
    k = _fa(intr, 4)
    table = (ReintegrateOp * max(len(ops), 1))()
    for o, (sign, depth, R, t) in zip(table, ops):
        o.sign, o.depth_scaled = int(sign), _ptr(depth)
        o.Rv2c18[:] = _fa(R, 18).tolist()
        o.tv2c6[:] = _fa(t, 6).tolist()
    z1 = int(r[2]) if z1 is None else z1
    check(_lib.xs_tsdf_reintegrate(len(ops), table, scaled_step, rows, cols, k.ctypes.data_as(_f32p), int(max_weight), r.ctypes.data_as(_i32p), voxel_size,
                                   tranc_dist, threshold, _ptr(value), _ptr(weight), _ptr(grad), vol_step, z0, z1, _ptr(counts), int(flags), _stream(stream)))


def tsdf_pack_bricks(res, planes=None):
    """xs_tsdf_pack_bricks (host only): the bricks of 8 x 8 x 8 voxels of `planes` stored planes (None: res[2]); 0 for what the pack calls refuse."""
    r = _ia(res, 3)
    return int(_lib.xs_tsdf_pack_bricks(r.ctypes.data_as(_i32p), int(r[2]) if planes is None else int(planes)))


def tsdf_pack_workspace_bytes(res, planes=None):
    """xs_tsdf_pack_workspace_bytes (host only): the workspace of tsdf_pack_classify and tsdf_pack_offsets; 0 as tsdf_pack_bricks."""
    r = _ia(res, 3)
    return int(_lib.xs_tsdf_pack_workspace_bytes(r.ctypes.data_as(_i32p), int(r[2]) if planes is None else int(planes)))


def tsdf_pack_classify(value, weight, grad, step, res, cls, offsets, workspace, planes=None, stream=None):
    """xs_tsdf_pack_classify: cls [nbricks] uint8 (bit 0 / 1 / 2: the value / weight / grad words of the brick are not all equal to the word at
    its first voxel) and offsets [nbricks + 1] uint64 (the exclusive sum of the words per brick: 1 or 512 per array) of the volume given at its
    first stored plane.  Arrays are device tensors or addresses.  No synchronisation."""
    r = _ia(res, 3)
    check(_lib.xs_tsdf_pack_classify(_ptr(value), _ptr(weight), _ptr(grad), step, r.ctypes.data_as(_i32p), int(r[2]) if planes is None else int(planes),
                                     _ptr(cls), _ptr(offsets), _ptr(workspace), _stream(stream)))


def tsdf_pack_offsets(cls, nbricks, offsets, workspace, stream=None):
    """xs_tsdf_pack_offsets: the offsets alone from class bytes on the device.  No synchronisation."""
    check(_lib.xs_tsdf_pack_offsets(_ptr(cls), int(nbricks), _ptr(offsets), _ptr(workspace), _stream(stream)))


def tsdf_pack_gather(value, weight, grad, step, res, cls, offsets, brick0, brick1, payload, planes=None, stream=None):
    """xs_tsdf_pack_gather: the payload words of bricks [brick0, brick1) to payload[0 ..] (uint32 / int32 device words).  No synchronisation."""
    r = _ia(res, 3)
    check(_lib.xs_tsdf_pack_gather(_ptr(value), _ptr(weight), _ptr(grad), step, r.ctypes.data_as(_i32p), int(r[2]) if planes is None else int(planes),
                                   _ptr(cls), _ptr(offsets), int(brick0), int(brick1), _ptr(payload), _stream(stream)))


def tsdf_unpack(value, weight, grad, step, res, cls, offsets, brick0, brick1, payload, planes=None, stream=None):
    """xs_tsdf_unpack: the inverse of tsdf_pack_gather: writes every in-volume voxel of bricks [brick0, brick1) and nothing else.  No synchronisation."""
    r = _ia(res, 3)
    check(_lib.xs_tsdf_unpack(_ptr(value), _ptr(weight), _ptr(grad), step, r.ctypes.data_as(_i32p), int(r[2]) if planes is None else int(planes),
                              _ptr(cls), _ptr(offsets), int(brick0), int(brick1), _ptr(payload), _stream(stream)))


DIFF_NO_CULL = 1   # XS_DIFF_NO_CULL


def tsdf_diff_workspace_bytes(res, src_res):
    """xs_tsdf_diff_workspace_bytes (host only): tsdf_merge's workspace for this source; 0 for an unusable resolution or a destination that
    has no frontier mask."""
    return int(_lib.xs_tsdf_diff_workspace_bytes(_res3(res).ctypes.data_as(_i32p), _res3(src_res).ctypes.data_as(_i32p)))


def tsdf_diff(value, weight, step, res, src_value, src_weight, src_step, src_res, xform12, only_this, only_other, counts, min_weight=1, lo=0.0, hi=0.5,
              flags=0, workspace=None, stream=None):
    """xs_tsdf_diff: compares this volume (value, weight) with the source volume resampled under xform12 as tsdf_merge samples it, where both
    carry min_weight: only_this gets the voxels with value < lo here and >= hi there, only_other the reverse, one 64-bit word per brick in
    the frontier mask's layout (frontier_mask_bytes(res) bytes each, every word written); counts (uint64 / int64 device tensor of 3 words) is
    incremented by {compared, only_this, only_other}.  Arrays are device tensors or addresses of plane 0; `workspace`:
    tsdf_diff_workspace_bytes(res, src_res) bytes (None only with DIFF_NO_CULL).  Nothing of either volume is written.  No synchronisation."""
    r, s = _ia(res, 3), _ia(src_res, 3)
    m = _fa(xform12, 12)
    check(_lib.xs_tsdf_diff(_ptr(value), _ptr(weight), step, r.ctypes.data_as(_i32p), _ptr(src_value), _ptr(src_weight), src_step, s.ctypes.data_as(_i32p),
                            m.ctypes.data_as(_f32p), int(min_weight), float(lo), float(hi), int(flags), _ptr(only_this), _ptr(only_other), _ptr(counts),
                            _ptr(workspace), _stream(stream)))


def merge_affine(T, dst_voxel_size, src_voxel_size):
    """xs_host_merge_affine of libxslam_host.so (CPU): xform12 of tsdf_merge from a real 4 x 4 transform and the two voxel sizes."""
    from . import pipeline
    return pipeline.merge_affine(T, dst_voxel_size, src_voxel_size)


def map_transform(c2v_this, c2v_other):
    """xs_host_map_transform of libxslam_host.so (CPU): c2v_other c2v_this^-1 from the real parts."""
    from . import pipeline
    return pipeline.map_transform(c2v_this, c2v_other)


ALIGN_MAX_TRANSFORMS = 32   # XS_ALIGN_MAX_TRANSFORMS


def tsdf_align_workspace_bytes(transforms):
    """xs_tsdf_align_workspace_bytes (host only): tickets, maps and records for up to `transforms` transforms; 0 outside 1 .. 32."""
    return int(_lib.xs_tsdf_align_workspace_bytes(int(transforms)))


def tsdf_align_terms(index, src_value, src_weight, src_step, src_res, maps, min_weight, max_residual, workspace, out29xN, stream=None):
    """xs_tsdf_align_terms: the 29 raw Gauss-Newton sums of N transforms over a built band index of THIS map against the value and weight
    arrays of the other map (device tensors or addresses of plane 0); maps [N, 6, 12, 2] float32 (align_seeded_maps per transform);
    transform n's sums land at out29xN[29 n : 29 n + 29] (float64 device tensor).  No synchronisation."""
    m = np.ascontiguousarray(maps, dtype=np.float32).reshape(-1)
    assert m.size % 144 == 0, m.size
    s = _ia(src_res, 3)
    check(_lib.xs_tsdf_align_terms(m.size // 144, C.byref(index), _ptr(src_value), _ptr(src_weight), src_step, s.ctypes.data_as(_i32p), m.ctypes.data_as(_f32p),
                                   int(min_weight), float(max_residual), _ptr(workspace), _ptr(out29xN), _stream(stream)))


REGISTER_MAX_TRANSFORMS = 32   # XS_REGISTER_MAX_TRANSFORMS


def register_workspace_bytes(transforms):
    """xs_tsdf_register_workspace_bytes (host only): tickets and records for up to `transforms` transforms; 0 outside 1 .. 32.  Zero its first 256
    bytes once (tsdf_reduce_workspace_init)."""
    return int(_lib.xs_tsdf_register_workspace_bytes(int(transforms)))


def register_terms(n, points, xforms, value, weight, vol_step, res, voxel_size, min_weight, max_residual, workspace, out29xN, transforms=None, stream=None):
    """xs_tsdf_register_terms: the 29 Gauss-Newton sums {J^T J upper triangle, J^T r, sum r^2, count} of N transforms xforms [N, 12] float32
    (row-major R, then t: cloud frame to volume frame) over n points (device float32 [n, 3], metres) against a volume (device tensors or
    addresses of plane 0) in one launch; transform m's sums land at out29xN[29 m : 29 m + 29] (float64 device tensor).  transforms: N, where it
    is not to be taken from xforms.  A None among the arrays goes through as a null pointer.  No synchronisation."""
    m = None if xforms is None else np.ascontiguousarray(xforms, dtype=np.float32).reshape(-1)
    if transforms is None:
        assert m is not None and m.size % 12 == 0
        transforms = m.size // 12
    r = None if res is None else _ia(res, 3)
    check(_lib.xs_tsdf_register_terms(int(transforms), int(n), _ptr(points), None if m is None else m.ctypes.data_as(_f32p), _ptr(value), _ptr(weight), vol_step,
                                      None if r is None else r.ctypes.data_as(_i32p), float(voxel_size), int(min_weight), float(max_residual), _ptr(workspace),
                                      _ptr(out29xN), _stream(stream)))


REGISTER_SCORE_MAX_TRANSFORMS = 4096   # XS_REGISTER_SCORE_MAX_TRANSFORMS


def tsdf_score_points_workspace_bytes(transforms):
    """xs_tsdf_score_points_workspace_bytes (host only): tickets, transforms and records for up to `transforms` transforms; 0 outside 1 .. 4096.
    Zero its first 256 bytes once (tsdf_reduce_workspace_init)."""
    return int(_lib.xs_tsdf_score_points_workspace_bytes(int(transforms)))


def tsdf_score_points(n, points, xforms, value, weight, vol_step, res, voxel_size, min_weight, max_residual, workspace, out2xP, stride=1, transforms=None, stream=None):
    """xs_tsdf_score_points: {sum r^2, count} of P transforms xforms [P, 12] float32 (row-major R, then t: cloud frame to volume frame) over every
    stride-th of n points (device float32 [n, 3], metres) against a volume (device tensors or addresses of plane 0) in one launch; transform
    p's pair lands at out2xP[2 p : 2 p + 2] (float64 device tensor).  transforms: P, where it is not to be taken from xforms.  A None among the
    arrays goes through as a null pointer.  No synchronisation."""
    m = None if xforms is None else np.ascontiguousarray(xforms, dtype=np.float32).reshape(-1)
    if transforms is None:
        assert m is not None and m.size % 12 == 0
        transforms = m.size // 12
    r = None if res is None else _ia(res, 3)
    check(_lib.xs_tsdf_score_points(int(transforms), int(n), int(stride), _ptr(points), None if m is None else m.ctypes.data_as(_f32p), _ptr(value), _ptr(weight),
                                    vol_step, None if r is None else r.ctypes.data_as(_i32p), float(voxel_size), int(min_weight), float(max_residual),
                                    _ptr(workspace), _ptr(out2xP), _stream(stream)))


FUSE_MAX_POINTS, FUSE_MAX_HALF_STEPS = (1 << 24) - 1, 256   # XS_FUSE_MAX_POINTS, XS_FUSE_MAX_HALF_STEPS


def fuse_opts(min_range=0.2, max_range=5.0, carve=False):
    """An xs_fuse_opts."""
    o = FuseOpts()
    o.struct_bytes = C.sizeof(FuseOpts)
    o.min_range, o.max_range, o.carve = float(min_range), float(max_range), int(bool(carve))
    return o


def fuse_accumulator_bytes(res):
    """xs_tsdf_fuse_accumulator_bytes (host only): 8 bytes per voxel; 0 for a null or unusable resolution."""
    r = None if res is None else _ia(res, 3)
    return int(_lib.xs_tsdf_fuse_accumulator_bytes(None if r is None else r.ctypes.data_as(_i32p)))


def fuse_points_accumulate(n, points, origin, res, voxel_size, tranc_dist, opts, accumulator, counts, xform12=None, stream=None):
    """xs_tsdf_fuse_points_accumulate: the rays from `origin` [3] (the points' frame) to n points (device float32 [n, 3], metres; xform12 = row-major R
    then t takes both to the volume frame, None: as they are) walked in half-voxel steps; every voxel a ray enters has (1 << 40) | q added to its
    word of `accumulator` (device uint64, fuse_accumulator_bytes(res) bytes, zeroed once) by an integer atomic.  counts (device uint64 [4]) is
    INCREMENTED by {points used, points dropped, visits, samples outside}.  opts: fuse_opts(...).  A None goes through as a null pointer."""
    m, mp = _f32_or_null(xform12)
    o, op = _f32_or_null(origin)
    r = None if res is None else _ia(res, 3)
    check(_lib.xs_tsdf_fuse_points_accumulate(int(n), _ptr(points), mp, op, None if r is None else r.ctypes.data_as(_i32p), float(voxel_size), float(tranc_dist),
                                              C.byref(opts) if opts is not None else None, _ptr(accumulator), _ptr(counts), _stream(stream)))


def fuse_points_fold(value, weight, grad, step, res, accumulator, obs_weight=1, max_weight=100, z0=0, z1=None, written=None, stream=None):
    """xs_tsdf_fuse_points_fold: every voxel of planes [z0, z1) whose accumulator word has a count receives its mean observation with weight
    obs_weight by the merge's running mean (grad scaled by wp / (wp + ws)), and the word is cleared.  Arrays are device tensors or addresses of
    plane 0; `written` (uint64 / int64 device word, optional) is incremented by the voxels written.  No synchronisation."""
    r = None if res is None else _ia(res, 3)
    if z1 is None:
        z1 = 0 if r is None else int(r[2])
    check(_lib.xs_tsdf_fuse_points_fold(_ptr(value), _ptr(weight), _ptr(grad), step, None if r is None else r.ctypes.data_as(_i32p), int(z0), int(z1),
                                        _ptr(accumulator), int(obs_weight), int(max_weight), _ptr(written), _stream(stream)))


ALIGN_SCORE_MAX_TRANSFORMS = 4096   # XS_ALIGN_SCORE_MAX_TRANSFORMS


def tsdf_score_transforms_workspace_bytes(transforms):
    """xs_tsdf_score_transforms_workspace_bytes (host only): tickets, maps and records for up to `transforms` transforms; 0 outside 1 .. 4096."""
    return int(_lib.xs_tsdf_score_transforms_workspace_bytes(int(transforms)))


def tsdf_score_transforms(index, stride, src_value, src_weight, src_step, src_res, xforms, min_weight, max_residual, workspace, out2xP, stream=None):
    """xs_tsdf_score_transforms: {sum r^2, count} of P real index maps xforms [P, 12] float32 (merge_affine per transform) over every stride-th
    entry of a built band index of THIS map against the value and weight arrays of the other map (device tensors or addresses of plane 0);
    transform p's pair lands at out2xP[2 p : 2 p + 2] (float64 device tensor).  No synchronisation."""
    m = np.ascontiguousarray(xforms, dtype=np.float32).reshape(-1)
    assert m.size % 12 == 0, m.size
    s = _ia(src_res, 3)
    check(_lib.xs_tsdf_score_transforms(m.size // 12, C.byref(index), int(stride), _ptr(src_value), _ptr(src_weight), src_step, s.ctypes.data_as(_i32p),
                                        m.ctypes.data_as(_f32p), int(min_weight), float(max_residual), _ptr(workspace), _ptr(out2xP), _stream(stream)))


def align_seeded_maps(T, vs_this, vs_other):
    """xs_host_align_seeded_maps of libxslam_host.so (CPU): the six seeded maps [6, 12, 2] of tsdf_align_terms for one transform."""
    from . import pipeline
    return pipeline.align_seeded_maps(T, vs_this, vs_other)


MESH_OVER_CAPACITY = -2   # XS_MESH_OVER_CAPACITY


def mesh_opts(z0=0, z1=None, res=None, zs0=0, zs1=0, min_weight=1, want_normals=True, signmap=None, signmap_shift=3):
    o = MeshOpts()
    o.struct_bytes = C.sizeof(MeshOpts)
    o.zs0, o.zs1, o.z0 = zs0, zs1, z0
    o.z1 = int(res[2]) - 1 if z1 is None else z1
    o.min_weight, o.want_normals = min_weight, int(bool(want_normals))
    o.signmap, o.signmap_shift = _ptr(signmap), signmap_shift if signmap is not None else 0
    return o


def mesh_workspace_bytes(res, opts=None):
    r = _ia(res, 3)
    return _lib.xs_mesh_workspace_bytes(r.ctypes.data_as(_i32p), C.byref(opts) if opts is not None else None)


def mesh_case_table(cube_case):
    """xs_mesh_case_table (host only): the case's triangles as a list of edge triples."""
    out = (C.c_byte * 16)()
    check(_lib.xs_mesh_case_table(int(cube_case), out))
    e = [v for v in out if v >= 0]
    return [tuple(e[i:i + 3]) for i in range(0, len(e), 3)]


def extract_mesh_raw(value, weight, grad, vol_step, res, voxel_size, opts, vertices, vertex_im, normals, keys, vcap, triangles, tcap,
                     workspace, stream=None):
    """xs_extract_mesh on caller-provided buffers: returns (status, vertices found, triangles found) — status 0 or MESH_OVER_CAPACITY."""
    r = _ia(res, 3)
    nv, nt = _sz(0), _sz(0)
    rc = _lib.xs_extract_mesh(_ptr(value), _ptr(weight), _ptr(grad), vol_step, r.ctypes.data_as(_i32p), voxel_size, C.byref(opts),
                              _ptr(vertices), _ptr(vertex_im), _ptr(normals), _ptr(keys), vcap, _ptr(triangles), tcap, _ptr(workspace),
                              C.byref(nv), C.byref(nt), _stream(stream))
    if rc != MESH_OVER_CAPACITY:
        check(rc)
    return rc, int(nv.value), int(nt.value)


def extract_mesh(value, weight, grad, vol_step, res, voxel_size, z0=0, z1=None, zs0=0, zs1=0, min_weight=1, want_normals=True,
                 signmap=None, signmap_shift=3, stream=None):
    """Marching-cubes mesh of the TSDF (xs_extract_mesh, count then fill): a dict of CUDA tensors vertices [V, 3] f32, vertex_im [V, 3]
    f32 (None without grad), normals [V, 3] f32 (None unless want_normals), triangles [T, 3] i32, edge_keys [V] u64.  Synchronises."""
    import torch
    dev = value.device
    opts = mesh_opts(z0, z1, res, zs0, zs1, min_weight, want_normals, signmap, signmap_shift)
    ws = torch.empty(max(1, mesh_workspace_bytes(res, opts)), dtype=torch.uint8, device=dev)
    args = (value, weight, grad, vol_step, res, voxel_size, opts)
    rc, nv, nt = extract_mesh_raw(*args, None, None, None, None, 0, None, 0, ws, stream)
    f = lambda n: torch.empty((n, 3), dtype=torch.float32, device=dev)
    out = {"vertices": f(nv), "vertex_im": f(nv) if grad is not None else None, "normals": f(nv) if want_normals else None,
           "triangles": torch.empty((nt, 3), dtype=torch.int32, device=dev), "edge_keys": torch.empty(nv, dtype=torch.uint64, device=dev)}
    if rc == MESH_OVER_CAPACITY:
        rc, nv2, nt2 = extract_mesh_raw(*args, out["vertices"], out["vertex_im"], out["normals"], out["edge_keys"], nv, out["triangles"], nt,
                                        ws, stream)
        assert rc == 0 and (nv2, nt2) == (nv, nt), (rc, nv2, nt2, nv, nt)
    return out


def resize_pyramid(vmap0, nmap0, in_step, rows0, cols0, vmap1, nmap1, mid_step, vmap2, nmap2, out_step, stream=None):
    check(_lib.xs_resize_pyramid(_ptr(vmap0), _ptr(nmap0), in_step, rows0, cols0, _ptr(vmap1), _ptr(nmap1), mid_step, _ptr(vmap2), _ptr(nmap2),
                                 out_step, _stream(stream)))


def create_nmap(vmap, nmap, map_step, rows, cols, stream=None):
    check(_lib.xs_create_nmap(_ptr(vmap), _ptr(nmap), map_step, rows, cols, _stream(stream)))


def resize_vmap(src, src_step, src_rows, src_cols, dst, dst_step, stream=None):
    check(_lib.xs_resize_vmap(_ptr(src), src_step, src_rows, src_cols, _ptr(dst), dst_step, _stream(stream)))


def resize_nmap(src, src_step, src_rows, src_cols, dst, dst_step, stream=None):
    check(_lib.xs_resize_nmap(_ptr(src), src_step, src_rows, src_cols, _ptr(dst), dst_step, _stream(stream)))


def raycast(intr, Rc2v, tc2v, Rv2w, tv2w, tranc_dist, res, voxel_size, value, grad, vol_step, vmap, nmap, map_step, rows, cols,
            hits=None, workspace=None, stream=None, **opts):
    """xs_raycast; with options (signmap, signmap_shift, signmap_tranc_dist, pyramid, completion_event, steps) xs_raycast_ex — returns the options
    struct then (its pyramid_built field says whether the call built the pyramid)."""
    if opts:
        o = _ray_opts(opts)
        raycast_ex(intr, Rc2v, tc2v, Rv2w, tv2w, tranc_dist, res, voxel_size, value, grad, vol_step, vmap, nmap, map_step, rows, cols, o, hits=hits,
                   workspace=workspace, stream=stream)
        return o
    r = _ia(res, 3)
    _prep(voxel_size)
    k, a, b, c, d = _fa(intr, 4), _fa(Rc2v, 18), _fa(tc2v, 6), _fa(Rv2w, 18), _fa(tv2w, 6)
    P = lambda x: x.ctypes.data_as(_f32p)
    check(_lib.xs_raycast(P(k), P(a), P(b), P(c), P(d), tranc_dist, r.ctypes.data_as(_i32p), voxel_size, _ptr(value), _ptr(grad),
                          vol_step, _ptr(vmap), _ptr(nmap), map_step, rows, cols, _ptr(hits), _ptr(workspace), _stream(stream)))


def _ray_opts(kw):
    """raycast_opts from the keyword options of raycast / raycast_slab (whose own tranc_dist argument is the march's)."""
    kw = dict(kw)
    if "signmap_shift" in kw:
        kw["shift"] = kw.pop("signmap_shift")
    if "signmap_tranc_dist" in kw:
        kw["tranc_dist"] = kw.pop("signmap_tranc_dist")
    return raycast_opts(**kw)


def raycast_opts(signmap=None, shift=3, tranc_dist=0.0, pyramid=None, completion_event=None, steps=None):
    """An xs_raycast_opts; pyramid = (vmap1, nmap1, step1, vmap2, nmap2, step2) or None."""
    o = RaycastOpts()
    o.struct_bytes = C.sizeof(RaycastOpts)
    o.signmap, o.signmap_shift, o.signmap_tranc_dist = _ptr(signmap), shift, tranc_dist
    if pyramid is not None:
        o.pyr_vmap1, o.pyr_nmap1, o.pyr_step1, o.pyr_vmap2, o.pyr_nmap2, o.pyr_step2 = (_ptr(pyramid[0]), _ptr(pyramid[1]), pyramid[2],
                                                                                       _ptr(pyramid[3]), _ptr(pyramid[4]), pyramid[5])
    o.completion_event = completion_event.value if hasattr(completion_event, "value") else completion_event
    o.steps_dev = _ptr(steps)
    return o


def raycast_ex(intr, Rc2v, tc2v, Rv2w, tv2w, tranc_dist, res, voxel_size, value, grad, vol_step, vmap, nmap, map_step, rows, cols, opts,
               hits=None, workspace=None, stream=None):
    """xs_raycast_ex: xs_raycast with its options as an argument (opts: raycast_opts(...); opts.pyramid_built is set by the call)."""
    _prep(voxel_size)
    r = _ia(res, 3)
    k = _fa(intr, 4)
    a, b, c, d = _fa(Rc2v, 18), _fa(tc2v, 6), _fa(Rv2w, 18), _fa(tv2w, 6)
    P = lambda x: x.ctypes.data_as(_f32p)
    check(_lib.xs_raycast_ex(P(k), P(a), P(b), P(c), P(d), tranc_dist, r.ctypes.data_as(_i32p), voxel_size, _ptr(value), _ptr(grad), vol_step,
                             _ptr(vmap), _ptr(nmap), map_step, rows, cols, _ptr(hits), _ptr(workspace), C.byref(opts), _stream(stream)))


def raycast_signmap_shift(intr, voxel_size, tranc_dist):
    """xs_raycast_signmap_shift: the finest sign map the march can use for this configuration (log2 of the brick edge in voxels), 0 if none."""
    return int(_lib.xs_raycast_signmap_shift(_fa(intr, 4).ctypes.data_as(_f32p), voxel_size, tranc_dist))


def signmap_bytes(res, shift=3):
    """xs_signmap_bytes: device bytes of a sign map (one byte per brick of 2^shift voxels a side, twice, + the march's time table)."""
    return int(_lib.xs_signmap_bytes(_ia(res, 3).ctypes.data_as(_i32p), shift))


def signmap_reset(signmap, res, shift, tranc_dist, stream=None):
    check(_lib.xs_signmap_reset(_ptr(signmap), _ia(res, 3).ctypes.data_as(_i32p), shift, tranc_dist, _stream(stream)))


def signmap_rebuild(signmap, res, shift, tranc_dist, value, vol_step, stream=None):
    check(_lib.xs_signmap_rebuild(_ptr(signmap), _ia(res, 3).ctypes.data_as(_i32p), shift, tranc_dist, _ptr(value), vol_step, _stream(stream)))


def raycast_slab(intr, Rc2v, tc2v, Rv2w, tv2w, tranc_dist, res, voxel_size, value, grad, vol_step, zs0, zs1, z0, z1, vmap, nmap,
                 map_step, rows, cols, keys, stream=None, **opts):
    """xs_raycast_slab; with options (signmap, signmap_shift, signmap_tranc_dist) xs_raycast_slab_ex."""
    r = _ia(res, 3)
    _prep(voxel_size)
    k, a, b, c, d = _fa(intr, 4), _fa(Rc2v, 18), _fa(tc2v, 6), _fa(Rv2w, 18), _fa(tv2w, 6)
    P = lambda x: x.ctypes.data_as(_f32p)
    if opts:
        o = _ray_opts(opts)
        check(_lib.xs_raycast_slab_ex(P(k), P(a), P(b), P(c), P(d), tranc_dist, r.ctypes.data_as(_i32p), voxel_size, _ptr(value), _ptr(grad),
                                      vol_step, zs0, zs1, z0, z1, _ptr(vmap), _ptr(nmap), map_step, rows, cols, _ptr(keys), C.byref(o), _stream(stream)))
        return o
    check(_lib.xs_raycast_slab(P(k), P(a), P(b), P(c), P(d), tranc_dist, r.ctypes.data_as(_i32p), voxel_size, _ptr(value), _ptr(grad),
                               vol_step, zs0, zs1, z0, z1, _ptr(vmap), _ptr(nmap), map_step, rows, cols, _ptr(keys), _stream(stream)))


def raycast_compose_mask(own_keys, min_keys, vmap, nmap, map_step, rows, cols, stream=None):
    check(_lib.xs_raycast_compose_mask(_ptr(own_keys), _ptr(min_keys), _ptr(vmap), _ptr(nmap), map_step, rows, cols, _stream(stream)))


def raycast_compose_finish(min_keys, vmap, nmap, map_step, rows, cols, hits=None, stream=None):
    check(_lib.xs_raycast_compose_finish(_ptr(min_keys), _ptr(vmap), _ptr(nmap), map_step, rows, cols, _ptr(hits), _stream(stream)))


def raycast_compose_entry_bytes():
    return _lib.xs_raycast_compose_entry_bytes()


def raycast_compose_pack(own_keys, min_keys, vmap, nmap, map_step, rows, cols, entries, count, stream=None):
    """The pixels this rank owns with a vertex, packed (52-byte entries); *count (int32, zeroed by the caller) advances by their number."""
    check(_lib.xs_raycast_compose_pack(_ptr(own_keys), _ptr(min_keys), _ptr(vmap), _ptr(nmap), map_step, rows, cols, _ptr(entries), _ptr(count), _stream(stream)))


def raycast_compose_scatter(entries, n, vmap, nmap, map_step, rows, cols, stream=None):
    check(_lib.xs_raycast_compose_scatter(_ptr(entries), int(n), _ptr(vmap), _ptr(nmap), map_step, rows, cols, _stream(stream)))


def icp_workspace_bytes():
    return _lib.xs_icp_workspace_bytes()


def icp_workspace_init(workspace, stream=None):
    check(_lib.xs_icp_workspace_init(_ptr(workspace), _stream(stream)))


ICP_PUBLISH_PAIRS = 1      # XS_ICP_PUBLISH_PAIRS: pass as done_flag; `sums` is then ICP_PAIRS_BYTES of host-coherent pinned memory (icp_wait_pairs)
ICP_PAIRS_BYTES = 55 * 16


def icp_accumulate(Rcurr, tcurr, vmap_curr, nmap_curr, Rprev_inv, tprev, intr, vmap_g_prev, nmap_g_prev, map_step, rows, cols,
                   distThres, angleThres, workspace, sums, y0=0, y1=None, stream=None, done_flag=None, done_seq=0):
    a, b, c, d, k = _fa(Rcurr, 18), _fa(tcurr, 6), _fa(Rprev_inv, 18), _fa(tprev, 6), _fa(intr, 4)
    P = lambda x: x.ctypes.data_as(_f32p)
    y1 = rows if y1 is None else y1
    check(_lib.xs_icp_accumulate(P(a), P(b), _ptr(vmap_curr), _ptr(nmap_curr), P(c), P(d), P(k), _ptr(vmap_g_prev), _ptr(nmap_g_prev),
                                 map_step, rows, cols, distThres, angleThres, y0, y1, _ptr(workspace), _ptr(sums), _ptr(done_flag), done_seq,
                                 _stream(stream)))


def icp_wait_pairs(pairs, seq, max_spins=2_000_000_000):
    """(rc, sums[55]): spins until all 55 pairs of the pinned buffer carry seq; rc 1 = the launch gave up, 2 = nothing came."""
    out = np.zeros(55, np.float64)
    rc = _lib.xs_icp_wait_pairs(_ptr(pairs), seq, out.ctypes.data, max_spins)
    return rc, out


def icp_accumulate_real(Rcurr, tcurr, vmap_curr_real, nmap_curr_real, real_step, Rprev_inv, tprev, intr, vmap_g_prev, nmap_g_prev, map_step, rows,
                        cols, distThres, angleThres, workspace, sums, y0=0, y1=None, stream=None, vmap_curr=None, nmap_curr=None):
    """icp_accumulate reading the current-frame maps' real parts from float planes (create_vnmaps(..., vreal=, nreal=))."""
    a, b, c, d, k = _fa(Rcurr, 18), _fa(tcurr, 6), _fa(Rprev_inv, 18), _fa(tprev, 6), _fa(intr, 4)
    P = lambda x: x.ctypes.data_as(_f32p)
    y1 = rows if y1 is None else y1
    check(_lib.xs_icp_accumulate_real(P(a), P(b), _ptr(vmap_curr), _ptr(nmap_curr), _ptr(vmap_curr_real), _ptr(nmap_curr_real), real_step, P(c), P(d),
                                      P(k), _ptr(vmap_g_prev), _ptr(nmap_g_prev), map_step, rows, cols, distThres, angleThres, y0, y1,
                                      _ptr(workspace), _ptr(sums), None, 0, _stream(stream)))


def icp_accumulate_posted_real(mailbox, mailbox_seq, vmap_curr_real, nmap_curr_real, real_step, Rprev_inv, tprev, intr, vmap_g_prev, nmap_g_prev,
                               map_step, rows, cols, distThres, angleThres, workspace, sums, y0=0, y1=None, stream=None, done_flag=None, done_seq=0):
    c, d, k = _fa(Rprev_inv, 18), _fa(tprev, 6), _fa(intr, 4)
    P = lambda x: x.ctypes.data_as(_f32p)
    check(_lib.xs_icp_accumulate_posted_real(_ptr(mailbox), mailbox_seq, None, None, _ptr(vmap_curr_real), _ptr(nmap_curr_real), real_step, P(c), P(d),
                                             P(k), _ptr(vmap_g_prev), _ptr(nmap_g_prev), map_step, rows, cols, distThres, angleThres, y0,
                                             rows if y1 is None else y1, _ptr(workspace), _ptr(sums), _ptr(done_flag), done_seq, _stream(stream)))


def icp_iterate(Rcurr, tcurr, vmap_curr, nmap_curr, Rprev_inv, tprev, intr, vmap_g_prev, nmap_g_prev, map_step, rows, cols,
                distThres, angleThres, workspace, sums, pose_state, stream=None):
    """One ICP iteration with the pose update on the device (xs_icp_iterate).  Rcurr / tcurr None:
    continue from the pose the previous launch left in pose_state (a 128-byte device tensor)."""
    c, d, k = _fa(Rprev_inv, 18), _fa(tprev, 6), _fa(intr, 4)
    P = lambda x: x.ctypes.data_as(_f32p)
    if Rcurr is None:
        pa = pb = None
    else:
        a, b = _fa(Rcurr, 18), _fa(tcurr, 6)
        pa, pb = P(a), P(b)
    check(_lib.xs_icp_iterate(pa, pb, _ptr(vmap_curr), _ptr(nmap_curr), P(c), P(d), P(k), _ptr(vmap_g_prev), _ptr(nmap_g_prev),
                              map_step, rows, cols, distThres, angleThres, _ptr(workspace), _ptr(sums), None, _ptr(pose_state), None, None, 0,
                              _stream(stream)))


def icp_accumulate_posted(mailbox, mailbox_seq, vmap_curr, nmap_curr, Rprev_inv, tprev, intr, vmap_g_prev, nmap_g_prev, map_step, rows,
                          cols, distThres, angleThres, workspace, sums, y0=0, y1=None, stream=None, done_flag=None, done_seq=0):
    """Enqueue an ICP reduction whose pose arrives later through `mailbox` (a 128-byte tensor in pinned
    host memory, see icp_post_pose).  The launch polls until the sequence number shows up — post it, or
    the launch gives up after about a second."""
    c, d, k = _fa(Rprev_inv, 18), _fa(tprev, 6), _fa(intr, 4)
    P = lambda x: x.ctypes.data_as(_f32p)
    check(_lib.xs_icp_accumulate_posted(_ptr(mailbox), mailbox_seq, _ptr(vmap_curr), _ptr(nmap_curr), P(c), P(d), P(k), _ptr(vmap_g_prev),
                                        _ptr(nmap_g_prev), map_step, rows, cols, distThres, angleThres, y0, rows if y1 is None else y1,
                                        _ptr(workspace), _ptr(sums), _ptr(done_flag), done_seq, _stream(stream)))


def icp_post_pose(mailbox, Rcurr, tcurr, mailbox_seq, cmd=0):
    """Host side of the pose mailbox: cmd 0 = run with this pose, 1 = abandon the launch."""
    P = lambda x: x.ctypes.data_as(_f32p)
    if Rcurr is None:
        _lib.xs_icp_post_pose(_ptr(mailbox), None, None, mailbox_seq, cmd)
    else:
        a, b = _fa(Rcurr, 18), _fa(tcurr, 6)
        _lib.xs_icp_post_pose(_ptr(mailbox), P(a), P(b), mailbox_seq, cmd)


def icp_records_bytes():
    return int(_lib.xs_icp_records_bytes())


def icp_records_count(cols, y0, y1):
    return int(_lib.xs_icp_records_count(cols, y0, y1))


def icp_accumulate_records(Rcurr, tcurr, vmap_curr, nmap_curr, Rprev_inv, tprev, intr, vmap_g_prev, nmap_g_prev, map_step, rows, cols, distThres,
                           angleThres, records, seq, y0=0, y1=None, mailbox=None, mailbox_seq=0, stream=None):
    """estimateCombined with the final addition on the host: enqueue the launch; every workgroup writes its record into `records`
    (a pinned host tensor of icp_records_bytes() bytes).  Rcurr / tcurr None: the pose is posted through `mailbox`."""
    c, d, k = _fa(Rprev_inv, 18), _fa(tprev, 6), _fa(intr, 4)
    P = lambda x: x.ctypes.data_as(_f32p)
    a, b = (None, None) if Rcurr is None else (P(_fa(Rcurr, 18)), P(_fa(tcurr, 6)))
    check(_lib.xs_icp_accumulate_records(a, b, _ptr(mailbox), mailbox_seq, _ptr(vmap_curr), _ptr(nmap_curr), P(c), P(d), P(k), _ptr(vmap_g_prev),
                                         _ptr(nmap_g_prev), map_step, rows, cols, distThres, angleThres, y0, rows if y1 is None else y1,
                                         _ptr(records), seq, _stream(stream)))


def icp_sum_records(records, count, seq, max_spins=2000000000):
    """Host: wait for the `count` records of launch `seq` and add them in index order.  (status, sums[55])."""
    out = np.zeros(55, np.float64)
    rc = _lib.xs_icp_sum_records(_ptr(records), count, seq, out.ctypes.data_as(_f64p), max_spins)
    return rc, out


def icp_gate_selftest(z, thres, or_equal, stream=None):
    """Gate shortcut of the ICP search against the full complex square root on the complex64 tensor `z` (device).
    Returns (disagreements, values that needed the square root)."""
    import torch
    zz = torch.view_as_real(z.contiguous()).contiguous()
    counts = torch.zeros(2, dtype=torch.int32, device=z.device)
    check(_lib.xs_icp_gate_selftest(_ptr(zz), z.numel(), float(thres), int(bool(or_equal)), _ptr(counts), _stream(stream)))
    torch.cuda.synchronize()
    c = counts.cpu().numpy().astype(np.int64)
    return int(c[0]), int(c[1])


def icp_mailbox_bytes():
    return int(_lib.xs_icp_mailbox_bytes())


def icp_mailbox_alloc():
    """(address, in_device_memory) of a zeroed pose mailbox; release with icp_mailbox_free."""
    p, dev = C.c_void_p(), C.c_int(0)
    check(_lib.xs_icp_mailbox_alloc(C.byref(p), C.byref(dev)))
    return p.value, dev.value


def icp_mailbox_free(address, in_device_memory):
    check(_lib.xs_icp_mailbox_free(address, in_device_memory))


def estimate_combined(Rcurr, tcurr, vmap_curr, nmap_curr, Rprev_inv, tprev, intr, vmap_g_prev, nmap_g_prev, map_step, rows, cols,
                      distThres, angleThres, workspace, sums, stream=None):
    """Returns (A[72], b[12], inliers) on the host after synchronising, like estimateCombined."""
    a, b, c, d, k = _fa(Rcurr, 18), _fa(tcurr, 6), _fa(Rprev_inv, 18), _fa(tprev, 6), _fa(intr, 4)
    P = lambda x: x.ctypes.data_as(_f32p)
    A = np.zeros(72, np.float64)
    bb = np.zeros(12, np.float64)
    inl = C.c_longlong(0)
    check(_lib.xs_estimate_combined(P(a), P(b), _ptr(vmap_curr), _ptr(nmap_curr), P(c), P(d), P(k), _ptr(vmap_g_prev), _ptr(nmap_g_prev),
                                    map_step, rows, cols, distThres, angleThres, _ptr(workspace), _ptr(sums), A.ctypes.data_as(_f64p),
                                    bb.ctypes.data_as(_f64p), C.byref(inl), _stream(stream)))
    return A, bb, inl.value


def icp_unpack(sums54):
    s = np.ascontiguousarray(sums54, dtype=np.float64)
    A = np.zeros(72, np.float64)
    b = np.zeros(12, np.float64)
    _lib.xs_icp_unpack(s.ctypes.data_as(_f64p), A.ctypes.data_as(_f64p), b.ctypes.data_as(_f64p))
    return A, b


CSFD_OPS = {"mul": 0, "div": 1, "exp": 2, "sin": 3, "pow": 4}


def csfd_array_op(name, variant, a, b, out, n, stream=None):
    check(_lib.xs_csfd_array_op(CSFD_OPS[name], 1 if variant == "our" else 0, _ptr(a), _ptr(b), _ptr(out), n, _stream(stream)))


def dcsfd_f1(x, y, out, n, stream=None):
    check(_lib.xs_dcsfd_f1(_ptr(x), _ptr(y), _ptr(out), n, _stream(stream)))


def complex_table(dual, op, a, b, out, n, stream=None):
    check(_lib.xs_complex_table(1 if dual else 0, op, _ptr(a), _ptr(b), _ptr(out), n, _stream(stream)))
