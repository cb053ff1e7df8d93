"""ctypes binding of libnerf_hip.so (include/nerf_hip.h).

The library is the product: if it is missing or does not export a declared symbol this module
raises -- there is no CPU or eager-PyTorch fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NERF_HIP_LIB", os.path.join(_HERE, "libnerf_hip.so"))  # override: diagnostic builds only

NERF_HIP_ABI_VERSION = 7
SAVE_FOR_BACKWARD = 1 << 0
FORCE_TILE_KERNEL = 1 << 1
BF16_MLP = 1 << 2
WEIGHTS_UNCHANGED = 1 << 3
SPLIT_MLP = 1 << 4
CORRECTED = 1 << 5
STATUS_RESAMPLE_INDEX = 1 << 0
STATUS_PREP_TIMEOUT = 1 << 1
SIMPLIFY_TABLE_FULL = 1 << 0
EDGES_TABLE_FULL = 1 << 0
TSDF_CARVE = 1 << 0
MAX_QUANTILES = 4  # NERF_HIP_MAX_QUANTILES: quantiles of one nerf_hip_forward_quantiles call (they travel in the kernels' arguments)
VOLUME_MAX_STEPS = 65536  # NERF_HIP_VOLUME_MAX_STEPS: the cap on the samples of one ray of nerf_hip_volume_render
VOLUME_GRAD_SHIFT = 40  # NERF_HIP_VOLUME_GRAD_SHIFT: nerf_hip_volume_render_backward's accumulators count units of 2^-40
TSDF_VIEWS_PER_LAUNCH = 32  # NERF_HIP_TSDF_VIEWS_PER_LAUNCH: views whose cameras travel in one launch's kernel arguments

_p = C.c_void_p
_PROTOS = {
    "nerf_hip_abi_version": (C.c_int, []),
    "nerf_hip_last_error": (C.c_char_p, []),
    "nerf_hip_ws_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "nerf_hip_ws_offset": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_size_t)]),
    "nerf_hip_forward": (C.c_int, [_p, _p, _p, _p, _p, _p, C.c_int, C.c_int, C.c_int, C.c_float, _p, _p, _p, C.c_size_t, C.c_int, _p]),
    "nerf_hip_forward_maps": (C.c_int, [_p, _p, _p, _p, _p, _p, C.c_int, C.c_int, C.c_int, C.c_float, _p, _p, _p, _p, C.c_size_t, C.c_int,
                                        _p]),
    "nerf_hip_forward_quantiles": (C.c_int, [_p, _p, _p, _p, _p, _p, C.c_int, C.c_int, C.c_int, C.c_float, _p, _p, _p, _p, C.c_size_t, C.c_int,
                                             _p, _p, C.c_int, _p]),
    "nerf_hip_forward_maps_train": (C.c_int, [_p, _p, _p, _p, _p, _p, C.c_int, C.c_int, C.c_int, C.c_float, _p, _p, _p, _p, C.c_size_t,
                                              C.c_int, _p]),
    "nerf_hip_backward": (C.c_int, [_p, _p, _p, _p, C.c_int, C.c_int, C.c_int, C.c_float, _p, _p, C.c_size_t, C.c_int, _p]),
    "nerf_hip_backward_overlap": (C.c_int, [_p, _p, _p, _p, C.c_int, C.c_int, C.c_int, C.c_float, _p, _p, C.c_size_t, C.c_int, _p, _p]),
    "nerf_hip_backward_maps": (C.c_int, [_p, _p, _p, _p, _p, C.c_int, C.c_int, C.c_int, C.c_float, _p, _p, C.c_size_t, C.c_int, _p, _p]),
    "nerf_hip_ray_loss": (C.c_int, [_p, _p, _p, C.c_int, _p, _p, _p, _p]),
    "nerf_hip_train_step": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, C.c_int, C.c_int, C.c_int, C.c_float, _p, _p, _p, _p, _p, C.c_size_t, C.c_int, _p, _p]),
    "nerf_hip_read_status": (C.c_int, [_p, C.c_size_t, C.POINTER(C.c_uint32), _p]),
    "nerf_hip_read_status_sticky": (C.c_int, [_p, C.c_size_t, C.POINTER(C.c_uint32), C.c_int, _p]),
    "nerf_hip_profile_begin": (C.c_int, [C.c_int]),
    "nerf_hip_profile_end": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_int]),
    "nerf_hip_adam_step": (C.c_int, [_p, _p, _p, _p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, _p]),
    "nerf_hip_gather_rays": (C.c_int, [_p, _p, _p, C.c_int, C.c_int, C.c_int, _p, _p, _p, _p, _p, _p]),
    "nerf_hip_rays": (C.c_int, [_p, _p, _p, _p, C.c_int, C.c_int, _p, _p, _p, _p]),
    "nerf_hip_field": (C.c_int, [_p, _p, _p, _p, _p, _p, C.c_int, C.c_int, _p, _p, _p, _p, _p, C.c_size_t, _p]),
    "nerf_hip_field_bf16": (C.c_int, [_p, _p, _p, _p, _p, _p, C.c_int, C.c_int, _p, _p, _p, C.c_size_t, _p]),
    "nerf_hip_coarse_composite": (C.c_int, [_p, _p, _p, _p, C.c_float, C.c_int, C.c_int, C.c_int, _p, _p, _p, _p, _p]),
    "nerf_hip_coarse_composite_backward": (C.c_int, [_p, _p, _p, _p, C.c_float, C.c_int, C.c_int, C.c_int, _p, _p, _p, _p, _p]),
    "nerf_hip_merge_composite": (C.c_int, [_p, _p, _p, _p, _p, _p, C.c_int, C.c_int, C.c_int, C.c_float, _p, _p, _p, _p]),
    "nerf_hip_coarse_composite_maps": (C.c_int, [_p, _p, _p, _p, C.c_float, C.c_int, C.c_int, C.c_int, _p, _p, _p, _p, _p, _p]),
    "nerf_hip_coarse_composite_backward_maps": (C.c_int, [_p, _p, _p, _p, C.c_float, C.c_int, C.c_int, C.c_int, _p, _p, _p, _p, _p, _p]),
    "nerf_hip_merge_composite_train": (C.c_int, [_p, _p, _p, _p, _p, _p, C.c_int, C.c_int, C.c_int, C.c_float, _p, _p, _p, _p, C.c_int, _p,
                                                 _p]),
    "nerf_hip_coarse_composite_quantiles": (C.c_int, [_p, _p, _p, _p, C.c_float, C.c_int, C.c_int, C.c_int, _p, _p, _p, _p, _p, _p, _p, C.c_int,
                                                      _p]),
    "nerf_hip_merge_composite_quantiles": (C.c_int, [_p, _p, _p, _p, _p, _p, C.c_int, C.c_int, C.c_int, C.c_float, _p, _p, _p, _p, C.c_int, _p,
                                                     _p, _p, C.c_int, _p]),
    "nerf_hip_merge_composite_backward": (C.c_int, [_p, _p, _p, _p, C.c_int, C.c_int, C.c_int, C.c_float, _p, _p, _p, _p, _p, _p]),
    "nerf_hip_forward_distortion_train": (C.c_int, [_p, _p, _p, _p, _p, _p, C.c_int, C.c_int, C.c_int, C.c_float, _p, _p, _p, _p, C.c_size_t,
                                                    C.c_int, _p, _p]),
    "nerf_hip_backward_distortion": (C.c_int, [_p, _p, _p, _p, _p, C.c_int, C.c_int, C.c_int, C.c_float, _p, _p, C.c_size_t, C.c_int, _p, _p,
                                               _p]),
    "nerf_hip_coarse_composite_distortion": (C.c_int, [_p, _p, _p, _p, C.c_float, C.c_int, C.c_int, C.c_int, _p, _p, _p, _p, _p, _p, _p]),
    "nerf_hip_merge_composite_distortion": (C.c_int, [_p, _p, _p, _p, _p, _p, C.c_int, C.c_int, C.c_int, C.c_float, _p, _p, _p, _p, C.c_int, _p,
                                                      _p, _p, _p]),
    "nerf_hip_coarse_composite_backward_distortion": (C.c_int, [_p, _p, _p, _p, C.c_float, C.c_int, C.c_int, C.c_int, _p, _p, _p, _p, _p, _p,
                                                                _p]),
    "nerf_hip_merge_composite_backward_distortion": (C.c_int, [_p, _p, _p, _p, C.c_int, C.c_int, C.c_int, C.c_float, _p, _p, _p, _p, _p, _p, _p,
                                                               _p]),
    "nerf_hip_normals_ws_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "nerf_hip_normals_ws_offset": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_size_t)]),
    "nerf_hip_forward_normals": (C.c_int, [_p, _p, _p, _p, _p, _p, C.c_int, C.c_int, C.c_int, C.c_float, _p, _p, _p, _p, C.c_size_t, C.c_int,
                                           _p, C.c_int, _p, _p, C.c_size_t]),
    "nerf_hip_normal_composite": (C.c_int, [_p, _p, C.c_int, C.c_int, _p, C.c_int, _p]),
    "nerf_hip_query_ws_bytes": (C.c_int, [C.c_int, C.POINTER(C.c_size_t)]),
    "nerf_hip_query": (C.c_int, [_p, _p, _p, C.c_int, _p, _p, _p, C.c_size_t, _p]),
    "nerf_hip_density_grid": (C.c_int, [_p, _p, _p, C.c_int, C.c_int, C.c_int, _p, _p, C.c_size_t, _p]),
    "nerf_hip_query_grad_ws_bytes": (C.c_int, [C.c_int, C.POINTER(C.c_size_t)]),
    "nerf_hip_query_grad": (C.c_int, [_p, _p, _p, C.c_int, _p, _p, _p, _p, _p, _p, C.c_size_t, _p]),
    "nerf_hip_metrics_ws_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "nerf_hip_image_metrics": (C.c_int, [_p, _p, C.c_int, C.c_int, C.c_int, _p, _p, _p, C.c_size_t, _p]),
    "nerf_hip_mesh_ws_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "nerf_hip_mesh_count": (C.c_int, [_p, C.c_int, C.c_int, C.c_int, C.c_float, _p, C.c_size_t, _p, _p]),
    "nerf_hip_mesh_emit": (C.c_int, [_p, C.c_int, C.c_int, C.c_int, _p, _p, C.c_float, _p, C.c_size_t, _p, _p, _p, C.c_int64,
                                     C.c_int64, _p]),
    "nerf_hip_band_ws_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "nerf_hip_band_begin": (C.c_int, [_p, _p, _p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _p, _p, C.c_size_t, _p, _p]),
    "nerf_hip_band_grow": (C.c_int, [_p, _p, _p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int64, _p, _p, C.c_size_t, _p, _p]),
    "nerf_hip_mesh_cc_ws_bytes": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_size_t)]),
    "nerf_hip_mesh_cc_round": (C.c_int, [_p, C.c_int64, C.c_int64, C.c_int, _p, C.c_size_t, _p, _p]),
    "nerf_hip_mesh_cc_ids": (C.c_int, [_p, C.c_int64, C.c_int64, _p, C.c_size_t, _p, _p, _p, _p]),
    "nerf_hip_mesh_cc_stats": (C.c_int, [_p, _p, _p, C.c_int64, C.c_int64, _p, _p, _p, _p, C.c_int64, _p]),
    "nerf_hip_mesh_cc_compact": (C.c_int, [_p, _p, _p, _p, C.c_int64, C.c_int64, _p, _p, _p, C.c_int64, _p, C.c_size_t, _p, _p, _p, _p,
                                           C.c_int64, C.c_int64, _p, _p]),
    "nerf_hip_mesh_simplify_ws_bytes": (C.c_int, [C.c_int64, C.c_int64, _p, C.POINTER(C.c_size_t)]),
    "nerf_hip_mesh_simplify_count": (C.c_int, [_p, _p, _p, C.c_int64, C.c_int64, _p, _p, _p, _p, C.c_size_t, _p, _p]),
    "nerf_hip_mesh_simplify_emit": (C.c_int, [_p, C.c_int64, C.c_int64, _p, _p, _p, _p, C.c_size_t, _p, _p, _p, C.c_int64, C.c_int64, _p]),
    "nerf_hip_mesh_edges_ws_bytes": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_size_t)]),
    "nerf_hip_mesh_edges_build": (C.c_int, [_p, C.c_int64, C.c_int64, _p, C.c_size_t, _p, _p, _p, _p]),
    "nerf_hip_mesh_smooth_step": (C.c_int, [_p, _p, C.c_int64, C.c_int64, _p, C.c_float, C.c_double, _p, _p, C.c_size_t, C.c_int64, _p]),
    "nerf_hip_mesh_vertex_normals": (C.c_int, [_p, _p, C.c_int64, C.c_int64, _p, C.c_float, _p, C.c_size_t, _p, C.c_int64, _p]),
    "nerf_hip_mesh_measure": (C.c_int, [_p, _p, C.c_int64, C.c_int64, _p, C.c_float, _p, _p]),
    "nerf_hip_mesh_sample_ws_bytes": (C.c_int, [C.c_int64, C.POINTER(C.c_size_t)]),
    "nerf_hip_mesh_sample": (C.c_int, [_p, _p, C.c_int64, C.c_int64, _p, C.c_float, C.c_int64, C.c_uint32, _p, C.c_size_t, _p, _p, C.c_int64,
                                       _p, _p]),
    "nerf_hip_points_nearest_ws_bytes": (C.c_int, [C.c_int64, C.c_int64, _p, C.POINTER(C.c_size_t)]),
    "nerf_hip_points_grid_build": (C.c_int, [_p, C.c_int64, _p, C.c_float, _p, _p, C.c_size_t, _p, _p]),
    "nerf_hip_points_nearest": (C.c_int, [_p, C.c_int64, C.c_int64, _p, C.c_float, _p, _p, C.c_size_t, C.c_int, _p, _p, C.c_int64, _p]),
    "nerf_hip_distance_stats": (C.c_int, [_p, C.c_int64, C.c_double, _p, C.c_int, _p, _p]),
    "nerf_hip_mesh_raycast_ws_bytes": (C.c_int, [C.c_int64, C.c_int64, _p, C.POINTER(C.c_size_t)]),
    "nerf_hip_mesh_raycast_grid_count": (C.c_int, [_p, _p, C.c_int64, C.c_int64, _p, C.c_float, _p, _p, _p]),
    "nerf_hip_mesh_raycast_grid_fill": (C.c_int, [_p, _p, C.c_int64, C.c_int64, _p, C.c_float, _p, C.c_int64, _p, C.c_size_t, _p]),
    "nerf_hip_mesh_raycast": (C.c_int, [_p, _p, C.c_int64, C.c_int64, _p, C.c_float, _p, C.c_int64, _p, C.c_size_t, _p, _p, _p, C.c_int64,
                                        C.c_double, C.c_double, C.c_int, _p, _p, _p, _p, _p, C.c_int64, _p]),
    "nerf_hip_mesh_face_rays": (C.c_int, [_p, _p, C.c_int64, C.c_int64, _p, _p, C.c_int, C.c_int, _p, _p, _p, C.c_int64, _p]),
    "nerf_hip_mesh_select_faces_ws_bytes": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_size_t)]),
    "nerf_hip_mesh_select_faces_count": (C.c_int, [_p, C.c_int64, C.c_int64, _p, _p, C.c_size_t, _p, _p]),
    "nerf_hip_mesh_select_faces_emit": (C.c_int, [_p, _p, _p, _p, C.c_int64, C.c_int64, _p, _p, C.c_size_t, _p, _p, _p, _p, C.c_int64, C.c_int64,
                                                  _p]),
    "nerf_hip_tsdf_integrate": (C.c_int, [_p, _p, C.c_int, C.c_int, C.c_int, _p, _p, _p, _p, C.c_int, C.c_int, C.c_int, _p, _p, C.c_double,
                                          C.c_float, C.c_int, _p]),
    "nerf_hip_tsdf_integrate_color": (C.c_int, [_p, _p, _p, C.c_int, C.c_int, C.c_int, _p, _p, _p, _p, _p, C.c_int, C.c_int, C.c_int, _p, _p,
                                                C.c_double, C.c_float, C.c_int, _p]),
    "nerf_hip_tsdf_sample_color": (C.c_int, [_p, C.c_int, C.c_int, C.c_int, _p, _p, _p, C.c_int64, _p, _p, _p]),
    "nerf_hip_mesh_count_masked": (C.c_int, [_p, _p, C.c_int, C.c_int, C.c_int, C.c_float, _p, C.c_size_t, _p, _p]),
    "nerf_hip_mesh_emit_masked": (C.c_int, [_p, _p, C.c_int, C.c_int, C.c_int, _p, _p, C.c_float, _p, C.c_size_t, _p, _p, _p, C.c_int64,
                                            C.c_int64, _p]),
    "nerf_hip_mesh_atlas_dims": (C.c_int, [C.c_int64, C.c_int, _p]),
    "nerf_hip_mesh_atlas_texels": (C.c_int, [_p, _p, _p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, _p, _p, _p, _p]),
    "nerf_hip_mesh_texture_sample": (C.c_int, [_p, C.c_int64, C.c_int, _p, _p, C.c_int64, _p, _p, _p, _p]),
    "nerf_hip_volume_sh_table": (C.c_int, [_p, _p]),
    "nerf_hip_volume_ws_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "nerf_hip_volume_active_count": (C.c_int, [_p, C.c_int, C.c_int, C.c_int, _p, C.c_size_t, _p, _p]),
    "nerf_hip_volume_active_emit": (C.c_int, [_p, C.c_int, C.c_int, C.c_int, _p, C.c_size_t, _p, C.c_int64, _p]),
    "nerf_hip_volume_points": (C.c_int, [_p, C.c_int64, C.c_int, C.c_int, C.c_int, _p, _p, _p, _p]),
    "nerf_hip_volume_sh_accumulate": (C.c_int, [_p, C.c_int, C.c_int, C.c_int, C.c_int, _p, C.c_int64, _p, C.c_int, _p]),
    "nerf_hip_volume_blocks": (C.c_int, [_p, C.c_int, C.c_int, C.c_int, C.c_int, _p, _p]),
    "nerf_hip_volume_sample": (C.c_int, [_p, _p, C.c_int, C.c_int, C.c_int, C.c_int, _p, _p, _p, _p, C.c_int64, _p, _p, _p]),
    "nerf_hip_volume_render": (C.c_int, [_p, _p, _p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _p, _p, _p, _p, _p, _p, C.c_int64,
                                         C.c_float, C.c_float, _p, _p, _p, _p, _p]),
    "nerf_hip_volume_render_backward": (C.c_int, [_p, _p, _p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _p, _p, _p, _p, _p, _p, C.c_int64,
                                                  C.c_float, C.c_float, _p, _p, _p, _p, _p, _p]),
    "nerf_hip_volume_adam_step": (C.c_int, [_p, _p, C.c_int, C.c_int, C.c_int, C.c_int, _p, C.c_int64, _p, _p, _p, _p, C.c_double, C.c_int64,
                                            C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _p]),
    "nerf_hip_volume_member_mask": (C.c_int, [_p, C.c_int64, C.c_int, C.c_int, C.c_int, _p, _p]),
    "nerf_hip_volume_tv_backward": (C.c_int, [_p, _p, C.c_int, C.c_int, C.c_int, C.c_int, _p, C.c_int64, _p, C.c_double, C.c_double,
                                              C.c_double, _p, _p, _p]),
    "nerf_hip_volume_upsample": (C.c_int, [_p, _p, C.c_int, C.c_int, C.c_int, C.c_int, _p, _p, _p]),
    "nerf_hip_volume_prune": (C.c_int, [_p, _p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _p]),
    "nerf_hip_volume_compact_slots": (C.c_int, [_p, C.c_int64, C.c_int, C.c_int, C.c_int, _p, _p]),
    "nerf_hip_volume_compact_pack": (C.c_int, [_p, _p, C.c_int, C.c_int, C.c_int, C.c_int, _p, C.c_int64, C.c_int, _p, _p, _p]),
    "nerf_hip_volume_compact_unpack": (C.c_int, [_p, _p, C.c_int, _p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, _p, _p, _p]),
    "nerf_hip_volume_compact_sample": (C.c_int, [_p, _p, _p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _p, _p, _p, _p, C.c_int64,
                                                 _p, _p, _p]),
    "nerf_hip_volume_compact_render": (C.c_int, [_p, _p, _p, C.c_int64, C.c_int, _p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _p, _p, _p,
                                                 _p, _p, _p, C.c_int64, C.c_float, C.c_float, _p, _p, _p, _p, _p]),
    "nerf_hip_volume_compact_render_backward": (C.c_int, [_p, _p, _p, C.c_int64, _p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _p, _p, _p,
                                                          _p, _p, _p, C.c_int64, C.c_float, C.c_float, _p, _p, _p, _p, _p, _p]),
    "nerf_hip_volume_compact_adam_step": (C.c_int, [_p, _p, C.c_int64, C.c_int, _p, _p, _p, _p, C.c_double, C.c_int64, C.c_double, C.c_double,
                                                    C.c_double, C.c_double, C.c_double, _p]),
    "nerf_hip_volume_compact_tv_backward": (C.c_int, [_p, _p, _p, _p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                                      C.c_double, _p, _p, _p]),
    "nerf_hip_volume_compact_importance": (C.c_int, [_p, _p, C.c_int64, _p, C.c_int, C.c_int, C.c_int, C.c_int, _p, _p, _p, _p, _p, _p,
                                                     C.c_int64, C.c_float, C.c_float, _p, _p, _p]),
    "nerf_hip_volume_vq_assign": (C.c_int, [_p, C.c_int64, _p, C.c_int64, C.c_int, _p, _p, _p]),
    "nerf_hip_volume_vq_accumulate": (C.c_int, [_p, C.c_int64, C.c_int, _p, C.c_int64, _p, C.c_int64, _p, _p, _p]),
    "nerf_hip_volume_vq_update": (C.c_int, [_p, C.c_int64, C.c_int, _p, _p, _p]),
    "nerf_hip_volume_vq_decode": (C.c_int, [_p, _p, C.c_int64, _p, C.c_int64, _p, C.c_int64, _p, C.c_int64, C.c_int, _p, _p]),
    "nerf_hip_volume_vq_expand": (C.c_int, [_p, _p, C.c_int64, _p, C.c_int64, _p, C.c_int64, _p, C.c_int64, C.c_int, _p, _p, _p]),
    "nerf_hip_volume_vq_grad_reduce": (C.c_int, [_p, C.c_int64, C.c_int, _p, _p, C.c_int64, C.c_int64, _p, _p]),
    "nerf_hip_volume_vq_adam_step": (C.c_int, [_p, C.c_int64, _p, _p, C.c_int64, _p, C.c_int64, C.c_int, _p, _p, _p, _p, _p, C.c_double,
                                               C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _p]),
}
EXPORTS = tuple(_PROTOS)

_lib = None


class NerfHipError(RuntimeError):
    pass


def lib() -> C.CDLL:
    """Loads libnerf_hip.so once.  Raises if it is absent (run ``python -c 'import __graft_entry__ as g; g.build()'``)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NerfHipError(f"{LIB_PATH} not found: build it with `make -C {os.path.join(_HERE, 'csrc')}`; "
                               "this package has no fallback path")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _PROTOS.items():
            fn = getattr(L, name)  # AttributeError if the symbol is missing
            fn.restype = res
            fn.argtypes = args
        if L.nerf_hip_abi_version() != NERF_HIP_ABI_VERSION:
            raise NerfHipError("libnerf_hip.so ABI version mismatch; rebuild")
        _lib = L
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise NerfHipError(f"libnerf_hip error {rc}: {lib().nerf_hip_last_error().decode()}")


def ws_bytes(B: int, Nc: int, Nf: int, flags: int) -> int:
    n = C.c_size_t(0)
    check(lib().nerf_hip_ws_bytes(B, Nc, Nf, flags, C.byref(n)))
    return int(n.value)


def normals_ws_bytes(B: int, Nc: int, Nf: int) -> int:
    """Bytes of the side workspace of nerf_hip_forward_normals for these sizes."""
    n = C.c_size_t(0)
    check(lib().nerf_hip_normals_ws_bytes(B, Nc, Nf, C.byref(n)))
    return int(n.value)


def normals_ws_view(nws, B, Nc, Nf, name, shape, dtype=None):
    """A typed view of a named buffer of nerf_hip_forward_normals's side workspace (tests / debugging), as ws_view."""
    import torch

    off = C.c_size_t(0)
    check(lib().nerf_hip_normals_ws_offset(B, Nc, Nf, name.encode(), C.byref(off)))
    dtype = dtype or torch.float32
    n = 1
    for d in shape:
        n *= d
    nbytes = n * torch.empty((), dtype=dtype).element_size()
    return nws[off.value: off.value + nbytes].view(dtype).view(*shape)


def query_ws_bytes(with_rgb: bool) -> int:
    """Workspace bytes of nerf_hip_query / nerf_hip_density_grid (independent of the number of points)."""
    n = C.c_size_t(0)
    check(lib().nerf_hip_query_ws_bytes(1 if with_rgb else 0, C.byref(n)))
    return int(n.value)


def query_grad_ws_bytes(with_rgb: bool) -> int:
    """Workspace bytes of nerf_hip_query_grad (independent of the number of points)."""
    n = C.c_size_t(0)
    check(lib().nerf_hip_query_grad_ws_bytes(1 if with_rgb else 0, C.byref(n)))
    return int(n.value)


def mesh_ws_bytes(nx: int, ny: int, nz: int) -> int:
    """Workspace bytes of nerf_hip_mesh_count / nerf_hip_mesh_emit over an nx x ny x nz grid."""
    n = C.c_size_t(0)
    check(lib().nerf_hip_mesh_ws_bytes(int(nx), int(ny), int(nz), C.byref(n)))
    return int(n.value)


def band_ws_bytes(nx: int, ny: int, nz: int, block: int) -> int:
    """Workspace bytes of nerf_hip_band_begin / nerf_hip_band_grow over an nx x ny x nz grid in blocks of ``block`` points."""
    n = C.c_size_t(0)
    check(lib().nerf_hip_band_ws_bytes(int(nx), int(ny), int(nz), int(block), C.byref(n)))
    return int(n.value)


def mesh_cc_ws_bytes(V: int, F: int) -> int:
    """Workspace bytes of the nerf_hip_mesh_cc_* calls on a mesh of V vertices and F faces."""
    n = C.c_size_t(0)
    check(lib().nerf_hip_mesh_cc_ws_bytes(int(V), int(F), C.byref(n)))
    return int(n.value)


def i32_array(values) -> "C.Array":
    return (C.c_int * len(values))(*[int(v) for v in values])


def mesh_simplify_ws_bytes(V: int, F: int, dims) -> int:
    """Workspace bytes of nerf_hip_mesh_simplify_count / _emit on a mesh of V vertices and F faces over a cluster lattice of dims cells."""
    n = C.c_size_t(0)
    check(lib().nerf_hip_mesh_simplify_ws_bytes(int(V), int(F), i32_array(dims), C.byref(n)))
    return int(n.value)


def mesh_edges_ws_bytes(V: int, F: int) -> int:
    """Workspace bytes of nerf_hip_mesh_edges_build / nerf_hip_mesh_smooth_step / nerf_hip_mesh_vertex_normals on V vertices and F faces."""
    n = C.c_size_t(0)
    check(lib().nerf_hip_mesh_edges_ws_bytes(int(V), int(F), C.byref(n)))
    return int(n.value)


def mesh_sample_ws_bytes(F: int) -> int:
    """Workspace bytes of nerf_hip_mesh_sample on a mesh of F faces."""
    n = C.c_size_t(0)
    check(lib().nerf_hip_mesh_sample_ws_bytes(int(F), C.byref(n)))
    return int(n.value)


def mesh_raycast_ws_bytes(F: int, cap_entries: int, dims) -> int:
    """Workspace bytes of nerf_hip_mesh_raycast_grid_fill / nerf_hip_mesh_raycast for F faces, cap_entries grid entries and a grid of dims cells."""
    n = C.c_size_t(0)
    check(lib().nerf_hip_mesh_raycast_ws_bytes(int(F), int(cap_entries), i32_array(dims), C.byref(n)))
    return int(n.value)


def mesh_select_faces_ws_bytes(V: int, F: int) -> int:
    """Workspace bytes of nerf_hip_mesh_select_faces_count / _emit on a mesh of V vertices and F faces."""
    n = C.c_size_t(0)
    check(lib().nerf_hip_mesh_select_faces_ws_bytes(int(V), int(F), C.byref(n)))
    return int(n.value)


def mesh_atlas_dims(F: int, n: int) -> tuple:
    """Rule TA's sizes (c, Sx, Sy, W, H) of the atlas of F faces with charts of n texels (nerf_hip_mesh_atlas_dims; host only)."""
    out = (C.c_int * 5)()
    check(lib().nerf_hip_mesh_atlas_dims(int(F), int(n), out))
    return tuple(int(x) for x in out)


def volume_ws_bytes(nx: int, ny: int, nz: int) -> int:
    """Workspace bytes of nerf_hip_volume_active_count / _emit over an nx x ny x nz lattice."""
    n = C.c_size_t(0)
    check(lib().nerf_hip_volume_ws_bytes(int(nx), int(ny), int(nz), C.byref(n)))
    return int(n.value)


def volume_sh_table():
    """Rule VS's tables (nerf_hip_volume_sh_table; host only) -> (dirs [12][3], b [12][9]) as nested tuples of floats that are exact fp32."""
    d, b = (C.c_float * 36)(), (C.c_float * 108)()
    check(lib().nerf_hip_volume_sh_table(d, b))
    return (tuple(tuple(d[k * 3: k * 3 + 3]) for k in range(12)), tuple(tuple(b[k * 9: k * 9 + 9]) for k in range(12)))


def points_nearest_ws_bytes(M: int, N: int, dims) -> int:
    """Workspace bytes of nerf_hip_points_grid_build (N = 0) / nerf_hip_points_nearest for M reference points, N queries and a grid of dims cells."""
    n = C.c_size_t(0)
    check(lib().nerf_hip_points_nearest_ws_bytes(int(M), int(N), i32_array(dims), C.byref(n)))
    return int(n.value)


def metrics_ws_bytes(n: int, H: int, W: int) -> int:
    """Workspace bytes of nerf_hip_image_metrics for n views of H x W."""
    k = C.c_size_t(0)
    check(lib().nerf_hip_metrics_ws_bytes(int(n), int(H), int(W), C.byref(k)))
    return int(k.value)


KERNEL_NAMES = ("pack_weights", "rays", "field_fwd_coarse", "coarse_composite", "field_fwd_fine", "merge_composite",
                "bwd_merge", "bwd_field_fine", "bwd_coarse", "bwd_field_coarse", "bwd_dw", "render_pair")


def profile_begin(max_launches: int) -> None:
    check(lib().nerf_hip_profile_begin(max_launches))


def profile_end() -> dict:
    """-> {kernel name: (total ms, launches)}"""
    n = len(KERNEL_NAMES)
    ms = (C.c_double * n)()
    cnt = (C.c_int * n)()
    check(lib().nerf_hip_profile_end(ms, cnt, n))
    return {KERNEL_NAMES[i]: (ms[i], cnt[i]) for i in range(n) if cnt[i]}


def ws_view(ws, B, Nc, Nf, flags, name, shape, dtype=None):
    """A typed view of a named workspace buffer (tests / debugging)."""
    import torch

    off = C.c_size_t(0)
    check(lib().nerf_hip_ws_offset(B, Nc, Nf, flags, name.encode(), C.byref(off)))
    dtype = dtype or torch.float32
    n = 1
    for d in shape:
        n *= d
    nbytes = n * torch.empty((), dtype=dtype).element_size()
    return ws[off.value: off.value + nbytes].view(dtype).view(*shape)


def ptr_array(tensors) -> "C.Array":
    """HOST array of device pointers (weights24 / dweights24)."""
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr


def f32_array(values) -> "C.Array":
    return (C.c_float * len(values))(*[float(v) for v in values])
