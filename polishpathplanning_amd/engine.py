"""ctypes binding of the gfx950 engine (libppp_hip.so, C ABI in include/ppp_hip.h).

This module is plumbing only: every number comes from the HIP kernels.  There is no
CPU fallback -- if the shared library is missing or no MI355X is visible, construction
raises.  The oracle under oracle/ is never imported from here.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libppp_hip.so")

PAIR_KD, PAIR_BRUTE = 0, 1
WALK_SECTPATH, WALK_CENTER_INT, WALK_SDIR_INT, WALK_V1_CONTACT, WALK_V1_SLICING = range(5)
STAGE_WP_XYZ, STAGE_WP_NN, STAGE_WP_NORMAL, STAGE_WP_PRESMOOTH, STAGE_WP_SMOOTHED = range(5)

OK, ERR_ARG, ERR_HIP, ERR_NO_DEVICE, ERR_SLICE, ERR_CAPACITY, ERR_DOMAIN, ERR_UNSUPPORTED, ERR_IO = 0, -1, -2, -3, -4, -5, -6, -7, -8


class PPPError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("ppp error %d: %s" % (code, msg))
        self.code = code


class Config(C.Structure):
    pass  # fields assigned after Params


class Params(C.Structure):
    _fields_ = [
        ("tool_radius", C.c_double),
        ("path_resolution", C.c_double),
        ("rpy_resolution", C.c_double),
        ("ee_length", C.c_float),
        ("change_range", C.c_int),
        ("pairing", C.c_int),
        ("walk", C.c_int),
        ("trim", C.c_double),
        ("drop_ends", C.c_int),
        ("smooth", C.c_int),
        ("handeye", C.c_float * 6),
        ("normal_radius", C.c_float),
        ("smooth_max_sweeps", C.c_int),
        ("alignment", C.c_int),
        ("dynamic_adjustment", C.c_int),
        ("depth", C.c_double),
        ("adjust_threshold", C.c_double),
        ("toolthickness", C.c_double),
        ("curvature_k", C.c_int),
        ("slice_begin", C.c_int),
        ("slice_end", C.c_int),
        ("range_margin", C.c_float),
    ]


Config._fields_ = [
    ("params", Params),
    ("path_file", C.c_char * 512),
    ("depth", C.c_double),
    ("adjust_threshold", C.c_double),
    ("toolthickness", C.c_double),
    ("smooth_cloud", C.c_int),
    ("remove_outlier", C.c_int),
    ("alignment", C.c_int),
    ("dynamic_adjustment", C.c_int),
]

EXPORTS = [
    "ppp_default_params", "ppp_create", "ppp_destroy", "ppp_last_error", "ppp_version", "ppp_set_params",
    "ppp_set_cloud", "ppp_set_cloud_device", "ppp_num_points", "ppp_gen_path_async", "ppp_get_path_async", "ppp_run_async",
    "ppp_sync", "ppp_failed_slice", "ppp_num_slices", "ppp_num_waypoints", "ppp_get_waypoints",
    "ppp_get_waypoints_device", "ppp_copy_waypoints_to_device", "ppp_get_tail_index", "ppp_minmax", "ppp_get_slice_positions",
    "ppp_get_slice_indices", "ppp_get_nodes", "ppp_get_boundary", "ppp_get_coverage", "ppp_get_path_coverage", "ppp_get_path_contacts", "ppp_get_path_removal", "ppp_get_path_dwell", "ppp_get_path_feed", "ppp_default_feed_params", "ppp_write_feed_file", "ppp_default_deviation_params", "ppp_get_deviation", "ppp_default_registration_params", "ppp_get_registration_terms", "ppp_register", "ppp_default_trimmed_registration_params", "ppp_register_trimmed", "ppp_default_robust_registration_params", "ppp_get_robust_registration_terms", "ppp_register_robust", "ppp_transform_cloud", "ppp_get_cloud_moments", "ppp_cloud_frame_from_moments", "ppp_registration_starts", "ppp_default_global_registration_params", "ppp_register_global", "ppp_get_contact_field", "ppp_get_regions", "ppp_range_owned", "ppp_get_contact_field_tile", "ppp_get_regions_tile", "ppp_merge_region_tiles", "ppp_get_deviation_tile", "ppp_merge_deviation_tiles", "ppp_get_registration_terms_tile", "ppp_merge_registration_terms", "ppp_registration_step", "ppp_register_tiles", "ppp_trim_select", "ppp_trim_rank", "ppp_register_trimmed_tiles", "ppp_robust_sigma", "ppp_robust_weight", "ppp_register_robust_tiles", "ppp_principal_curvatures_at", "ppp_eval_spline", "ppp_ranged_x_index", "ppp_insert_point",
    "ppp_normals_at", "ppp_estimate_normals", "ppp_area2cloud", "ppp_nearest", "ppp_get_stage", "ppp_smooth_sweeps", "ppp_enable_timing",
    "ppp_get_kernel_times", "ppp_load_pcd", "ppp_save_pcd", "ppp_free", "ppp_default_config", "ppp_read_config",
    "ppp_write_path_file", "ppp_run_batch_async", "ppp_sync_batch", "ppp_get_stream", "ppp_gather_waypoints", "ppp_get_cloud", "ppp_remove_outlier", "ppp_voxel_down", "ppp_smooth_mls", "ppp_trans2center", "ppp_get_waypoint_counts", "ppp_copy_stage_to_device", "ppp_finish_path_async",
    "ppp_save_pcd_rgb", "ppp_range_interval", "ppp_set_cloud_part", "ppp_spline_create", "ppp_spline_restart", "ppp_spline_eval", "ppp_spline_range", "ppp_spline_destroy",
    "ppp_set_fast_path", "ppp_get_fast_path", "ppp_set_plan_reuse", "ppp_set_cloud_pcd", "ppp_pcd_probe", "ppp_set_cloud_device_async",
    "ppp_default_mesh_params", "ppp_set_cloud_mesh", "ppp_set_cloud_stl", "ppp_load_stl", "ppp_save_stl",
    "ppp_default_trimesh_params", "ppp_trimesh_create", "ppp_trimesh_create_stl", "ppp_trimesh_destroy", "ppp_trimesh_nearest", "ppp_get_mesh_deviation",
    "ppp_trimesh_topology", "ppp_trimesh_get_topology", "ppp_trimesh_signed_nearest", "ppp_get_mesh_signed_deviation",
    "ppp_get_mesh_registration_terms", "ppp_register_mesh", "ppp_get_mesh_robust_registration_terms", "ppp_register_mesh_robust",
    "ppp_default_mesh_trimmed_registration_params", "ppp_get_mesh_trimmed_registration_terms", "ppp_register_mesh_trimmed",
    "ppp_trimesh_get_moments", "ppp_mesh_frame_from_moments", "ppp_register_mesh_global",
    "ppp_get_mesh_deviation_tile", "ppp_get_mesh_signed_deviation_tile", "ppp_merge_mesh_deviation_tiles", "ppp_merge_mesh_signed_deviation_tiles",
    "ppp_get_mesh_registration_terms_tile", "ppp_register_mesh_tiles",
    "ppp_set_side_by_side", "ppp_get_binning_form", "ppp_get_launch_priorities", "ppp_queue_create", "ppp_queue_destroy", "ppp_queue_submit", "ppp_queue_wait", "ppp_queue_lanes", "ppp_queue_lane", "ppp_queue_last_error",
]


def build(force=False):
    """Compile the HIP engine for gfx950 (hipcc cross-compiles without a GPU)."""
    src_dir = os.path.join(_HERE, "csrc")
    newest = max(os.path.getmtime(os.path.join(src_dir, f)) for f in os.listdir(src_dir))
    newest = max(newest, os.path.getmtime(os.path.join(_HERE, "..", "include", "ppp_hip.h")))
    if force or not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < newest:
        subprocess.check_call(["make", "-j4", "-C", src_dir], stdout=subprocess.DEVNULL)  # the engine and the window kernels build side by side
    return LIB_PATH


_lib = None


def lib():
    """Loads libppp_hip.so (never builds implicitly: a missing library is an error)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PPPError(ERR_NO_DEVICE, "libppp_hip.so is missing: run __graft_entry__.build() (no CPU fallback exists)")
        L = C.CDLL(LIB_PATH)
        vp, sz = C.c_void_p, C.c_size_t
        fp, dp, ip = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int)
        szp = C.POINTER(C.c_size_t)
        L.ppp_default_params.argtypes = [C.POINTER(Params)]
        L.ppp_default_params.restype = None
        L.ppp_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.ppp_destroy.argtypes = [vp]
        L.ppp_last_error.argtypes = [vp]
        L.ppp_last_error.restype = C.c_char_p
        L.ppp_version.restype = C.c_char_p
        L.ppp_set_params.argtypes = [vp, C.POINTER(Params)]
        L.ppp_set_cloud.argtypes = [vp, vp, sz, sz, fp]
        L.ppp_set_cloud_device.argtypes = [vp, vp, sz, sz, fp]
        L.ppp_set_cloud_device_async.argtypes = [vp, vp, sz, sz, fp]
        L.ppp_set_side_by_side.argtypes = [vp, C.c_int]
        L.ppp_get_binning_form.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.ppp_get_launch_priorities.argtypes = [vp] + [C.POINTER(C.c_int)] * 3
        L.ppp_queue_create.argtypes = [C.c_int, C.c_int, C.POINTER(Params), C.POINTER(vp)]
        L.ppp_queue_destroy.argtypes = [vp]; L.ppp_queue_destroy.restype = None
        L.ppp_queue_submit.argtypes = [vp, vp, sz, sz, fp, C.POINTER(C.c_longlong)]
        L.ppp_queue_wait.argtypes = [vp, C.c_longlong, szp, C.POINTER(vp)]
        L.ppp_queue_lanes.argtypes = [vp]
        L.ppp_queue_lane.argtypes = [vp, C.c_int]; L.ppp_queue_lane.restype = vp
        L.ppp_queue_last_error.argtypes = [vp]; L.ppp_queue_last_error.restype = C.c_char_p
        L.ppp_num_points.argtypes = [vp, szp]
        L.ppp_range_interval.argtypes = [C.POINTER(Params), C.c_float, C.c_float, fp, fp, ip]
        L.ppp_set_cloud_part.argtypes = [vp, vp, sz, sz, fp, ip, fp, fp, sz, C.c_float, C.c_float]
        L.ppp_gen_path_async.argtypes = [vp]
        L.ppp_get_path_async.argtypes = [vp]
        L.ppp_run_async.argtypes = [vp]
        L.ppp_sync.argtypes = [vp]
        L.ppp_failed_slice.argtypes = [vp]
        L.ppp_num_slices.argtypes = [vp, ip]
        L.ppp_num_waypoints.argtypes = [vp, szp]
        L.ppp_get_waypoints.argtypes = [vp, fp, sz, szp]
        L.ppp_get_waypoints_device.argtypes = [vp, C.POINTER(vp), szp]
        L.ppp_copy_waypoints_to_device.argtypes = [vp, vp, sz, szp]
        L.ppp_get_tail_index.argtypes = [vp, ip, sz, szp]
        L.ppp_get_waypoint_counts.argtypes = [vp, ip, sz, szp]
        L.ppp_run_batch_async.argtypes = [C.POINTER(vp), sz, vp, szp, szp]
        L.ppp_sync_batch.argtypes = [C.POINTER(vp), sz, szp]
        L.ppp_get_stream.argtypes = [vp, C.POINTER(vp)]
        L.ppp_gather_waypoints.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, szp, vp]
        L.ppp_get_cloud.argtypes = [vp, fp, sz, szp]
        L.ppp_remove_outlier.argtypes = [vp, C.c_int, C.c_double, szp, C.POINTER(C.c_double)]
        L.ppp_voxel_down.argtypes = [vp, C.c_float, C.c_float, C.c_float, szp, C.POINTER(C.c_int)]
        L.ppp_smooth_mls.argtypes = [vp, C.c_double, C.c_int, szp]
        L.ppp_trans2center.argtypes = [vp, fp, fp, fp]
        L.ppp_copy_stage_to_device.argtypes = [vp, C.c_int, vp, sz, szp]
        L.ppp_finish_path_async.argtypes = [vp, vp, sz, ip, sz]
        L.ppp_minmax.argtypes = [vp, fp, fp]
        L.ppp_get_slice_positions.argtypes = [vp, fp, sz, szp]
        L.ppp_get_slice_indices.argtypes = [vp, C.c_int, ip, sz, szp]
        L.ppp_get_nodes.argtypes = [vp, C.c_int, dp, dp, dp, sz, szp]
        L.ppp_get_boundary.argtypes = [vp, C.c_int, dp, dp, dp, sz, szp, C.POINTER(C.c_int)]
        L.ppp_get_coverage.argtypes = [vp, C.POINTER(C.c_ubyte), sz, szp, szp]
        L.ppp_get_path_coverage.argtypes = [vp, C.POINTER(C.c_ubyte), sz, szp, szp]
        L.ppp_get_path_contacts.argtypes = [vp, C.POINTER(C.c_uint), ip, ip, sz, C.POINTER(ContactStats)]
        L.ppp_get_path_removal.argtypes = [vp, C.c_int, C.POINTER(C.c_double), sz, C.POINTER(RemovalStats)]
        L.ppp_get_path_dwell.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.c_int, C.c_double, C.c_double, C.POINTER(DwellRow), sz,
                                         C.POINTER(C.c_double), sz, C.POINTER(DwellStats)]
        L.ppp_get_path_feed.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.c_int, C.c_double, C.c_double, C.POINTER(FeedParams),
                                        C.POINTER(FeedRow), sz, C.POINTER(FeedStats)]
        L.ppp_default_feed_params.argtypes = [C.POINTER(FeedParams)]
        L.ppp_default_feed_params.restype = None
        L.ppp_write_feed_file.argtypes = [C.c_char_p, fp, C.POINTER(FeedRow), sz]
        L.ppp_default_deviation_params.argtypes = [C.POINTER(DeviationParams)]
        L.ppp_default_deviation_params.restype = None
        L.ppp_get_deviation.argtypes = [vp, vp, C.POINTER(DeviationParams), dp, dp, ip, C.POINTER(C.c_ubyte), dp, sz, C.POINTER(DeviationStats)]
        L.ppp_default_registration_params.argtypes = [C.POINTER(RegistrationParams)]
        L.ppp_default_registration_params.restype = None
        L.ppp_get_registration_terms.argtypes = [vp, vp, C.POINTER(RegistrationParams), dp, C.POINTER(RegistrationRow), C.POINTER(RegistrationStats)]
        L.ppp_register.argtypes = [vp, vp, C.POINTER(RegistrationParams), dp, C.POINTER(RegistrationRow), sz, C.POINTER(RegistrationStats)]
        L.ppp_get_registration_terms_tile.argtypes = [vp, vp, C.POINTER(RegistrationParams), dp, C.POINTER(RegistrationRow), C.POINTER(RegistrationPart)]
        L.ppp_merge_registration_terms.argtypes = [C.POINTER(RegistrationRow), C.POINTER(RegistrationPart), sz, dp, C.POINTER(RegistrationRow),
                                                   C.POINTER(RegistrationPart)]
        L.ppp_registration_step.argtypes = [C.POINTER(RegistrationRow), C.POINTER(RegistrationPart), C.c_double, dp, dp, ip, dp]
        L.ppp_register_tiles.argtypes = [C.POINTER(vp), C.POINTER(vp), sz, C.POINTER(RegistrationParams), dp, C.POINTER(RegistrationRow), sz,
                                         C.POINTER(RegisterTilesStats)]
        L.ppp_default_trimmed_registration_params.argtypes = [C.POINTER(TrimmedRegistrationParams)]
        L.ppp_default_trimmed_registration_params.restype = None
        L.ppp_register_trimmed.argtypes = [vp, vp, C.POINTER(TrimmedRegistrationParams), dp, C.POINTER(TrimmedRegistrationRow), sz, C.POINTER(C.c_ubyte), fp,
                                           sz, C.POINTER(RegistrationStats)]
        L.ppp_default_robust_registration_params.argtypes = [C.POINTER(RobustRegistrationParams)]
        L.ppp_default_robust_registration_params.restype = None
        L.ppp_get_robust_registration_terms.argtypes = [vp, vp, C.POINTER(RobustRegistrationParams), dp, C.POINTER(RobustRegistrationRow), C.POINTER(C.c_ubyte),
                                                        fp, dp, sz, C.POINTER(RegistrationStats)]
        L.ppp_register_robust.argtypes = [vp, vp, C.POINTER(RobustRegistrationParams), dp, C.POINTER(RobustRegistrationRow), sz, C.POINTER(C.c_ubyte), fp, dp,
                                          sz, C.POINTER(RegistrationStats)]
        L.ppp_get_mesh_robust_registration_terms.argtypes = L.ppp_get_robust_registration_terms.argtypes
        L.ppp_register_mesh_robust.argtypes = L.ppp_register_robust.argtypes
        L.ppp_default_mesh_trimmed_registration_params.argtypes = [C.POINTER(MeshTrimmedRegistrationParams)]
        L.ppp_default_mesh_trimmed_registration_params.restype = None
        L.ppp_get_mesh_trimmed_registration_terms.argtypes = [vp, vp, C.POINTER(MeshTrimmedRegistrationParams), dp, C.POINTER(MeshTrimmedRegistrationRow),
                                                              C.POINTER(C.c_ubyte), fp, sz, C.POINTER(RegistrationStats)]
        L.ppp_register_mesh_trimmed.argtypes = [vp, vp, C.POINTER(MeshTrimmedRegistrationParams), dp, C.POINTER(MeshTrimmedRegistrationRow), sz,
                                                C.POINTER(C.c_ubyte), fp, sz, C.POINTER(RegistrationStats)]
        L.ppp_trim_select.argtypes = [C.POINTER(C.c_uint), sz, sz, C.POINTER(C.c_uint), C.POINTER(sz)]
        L.ppp_trim_rank.argtypes = [C.c_double, sz]
        L.ppp_trim_rank.restype = sz
        L.ppp_register_trimmed_tiles.argtypes = [C.POINTER(vp), C.POINTER(vp), sz, C.POINTER(TrimmedRegistrationParams), dp, C.POINTER(TrimmedRegistrationRow),
                                                 sz, C.POINTER(C.POINTER(C.c_ubyte)), C.POINTER(fp), C.POINTER(C.POINTER(C.c_ubyte)), sz,
                                                 C.POINTER(RegisterTilesStats)]
        L.ppp_robust_sigma.argtypes = [C.c_uint, C.c_int, C.c_double]
        L.ppp_robust_sigma.restype = C.c_double
        L.ppp_robust_weight.argtypes = [C.c_double, C.c_double, C.c_double]
        L.ppp_robust_weight.restype = C.c_double
        L.ppp_register_robust_tiles.argtypes = [C.POINTER(vp), C.POINTER(vp), sz, C.POINTER(RobustRegistrationParams), dp, C.POINTER(RobustRegistrationRow),
                                                sz, C.POINTER(C.POINTER(C.c_ubyte)), C.POINTER(fp), C.POINTER(dp), C.POINTER(C.POINTER(C.c_ubyte)), sz,
                                                C.POINTER(RegisterTilesStats)]
        L.ppp_transform_cloud.argtypes = [vp, dp]
        L.ppp_get_cloud_moments.argtypes = [vp, C.POINTER(CloudFrame)]
        L.ppp_cloud_frame_from_moments.argtypes = [C.POINTER(C.c_longlong), C.c_int, dp, C.c_double, C.POINTER(CloudFrame)]
        L.ppp_registration_starts.argtypes = [C.POINTER(CloudFrame), C.POINTER(CloudFrame), C.c_int, dp]
        L.ppp_default_global_registration_params.argtypes = [C.POINTER(GlobalRegistrationParams)]
        L.ppp_default_global_registration_params.restype = None
        L.ppp_register_global.argtypes = [vp, vp, C.POINTER(GlobalRegistrationParams), C.POINTER(RegistrationCandidate), sz, C.POINTER(RegistrationRow), sz,
                                          C.POINTER(GlobalRegistrationStats)]
        L.ppp_get_contact_field.argtypes = [vp, fp, fp, sz, C.c_float, C.POINTER(ContactFieldStats)]
        L.ppp_get_regions.argtypes = [vp, C.c_int, C.POINTER(C.c_ubyte), C.c_float, C.c_float, ip, sz, C.POINTER(Region), sz,
                                      C.POINTER(RegionStats)]
        L.ppp_range_owned.argtypes = [C.POINTER(Params), C.c_float, C.c_float, fp, fp]
        L.ppp_get_contact_field_tile.argtypes = [vp, fp, fp, C.POINTER(C.c_ubyte), sz, C.c_float, C.c_float, C.POINTER(ContactFieldTileStats)]
        L.ppp_get_regions_tile.argtypes = [vp, C.c_int, C.POINTER(C.c_ubyte), C.c_float, C.c_float, ip, sz, C.POINTER(RegionPart), sz,
                                           C.POINTER(RegionHalo), sz, C.POINTER(RegionTileStats)]
        L.ppp_merge_region_tiles.argtypes = [sz, C.POINTER(ip), C.POINTER(C.POINTER(RegionPart)), C.POINTER(C.POINTER(RegionHalo)),
                                             C.POINTER(RegionTileStats), ip, sz, C.POINTER(Region), sz, C.POINTER(RegionStats)]
        ubp = C.POINTER(C.c_ubyte)
        L.ppp_get_deviation_tile.argtypes = [vp, vp, C.POINTER(DeviationParams), C.c_float, dp, dp, ip, ubp, dp, ubp, sz,
                                             C.POINTER(DeviationTileStats)]
        L.ppp_merge_deviation_tiles.argtypes = [sz, C.POINTER(DeviationTileStats), C.POINTER(dp), C.POINTER(ubp), C.POINTER(dp), C.POINTER(ubp),
                                                C.POINTER(DeviationStats)]
        L.ppp_principal_curvatures_at.argtypes = [vp, fp, sz, fp]
        L.ppp_eval_spline.argtypes = [vp, C.c_int, dp, sz, dp]
        L.ppp_ranged_x_index.argtypes = [vp, C.c_int, ip, sz, szp]
        L.ppp_insert_point.argtypes = [vp, ip, sz, C.c_float, dp, dp, dp, sz, szp]
        L.ppp_normals_at.argtypes = [vp, ip, sz, fp]
        L.ppp_estimate_normals.argtypes = [vp, fp]
        L.ppp_area2cloud.argtypes = [vp, dp, sz, C.c_int, fp]
        L.ppp_nearest.argtypes = [vp, fp, sz, ip]
        L.ppp_get_stage.argtypes = [vp, C.c_int, vp, sz, szp]
        L.ppp_smooth_sweeps.argtypes = [vp, ip]
        L.ppp_enable_timing.argtypes = [vp, C.c_int]
        L.ppp_get_kernel_times.argtypes = [vp, C.c_char_p, fp, ip, sz, szp]
        L.ppp_load_pcd.argtypes = [C.c_char_p, C.POINTER(fp), szp, fp]
        L.ppp_save_pcd.argtypes = [C.c_char_p, fp, sz, sz, fp, C.c_int]
        L.ppp_free.argtypes = [vp]
        L.ppp_free.restype = None
        L.ppp_default_config.argtypes = [C.POINTER(Config)]
        L.ppp_default_config.restype = None
        L.ppp_read_config.argtypes = [C.c_char_p, C.POINTER(Config)]
        L.ppp_write_path_file.argtypes = [C.c_char_p, fp, sz]
        L.ppp_spline_create.argtypes = [C.c_int, sz, dp, dp, dp, C.POINTER(vp)]
        L.ppp_spline_restart.argtypes = [vp, sz, dp, dp, dp]
        L.ppp_spline_eval.argtypes = [vp, dp, sz, dp]
        L.ppp_spline_range.argtypes = [vp, dp, dp, szp]
        L.ppp_spline_destroy.argtypes = [vp]
        L.ppp_set_fast_path.argtypes = [vp, C.c_int]
        L.ppp_set_plan_reuse.argtypes = [vp, C.c_int]
        L.ppp_set_cloud_pcd.argtypes = [vp, C.c_char_p, C.POINTER(C.c_size_t), C.POINTER(C.c_float)]
        L.ppp_pcd_probe.argtypes = [C.c_char_p, C.c_void_p]
        L.ppp_get_fast_path.argtypes = [vp, ip]
        L.ppp_default_mesh_params.argtypes = [C.POINTER(MeshParams)]
        L.ppp_default_mesh_params.restype = None
        L.ppp_set_cloud_mesh.argtypes = [vp, fp, sz, ip, sz, C.POINTER(MeshParams), fp, ip, sz, C.POINTER(MeshStats)]
        L.ppp_set_cloud_stl.argtypes = [vp, C.c_char_p, C.POINTER(MeshParams), fp, C.POINTER(MeshStats)]
        ubp = C.POINTER(C.c_ubyte)
        L.ppp_default_trimesh_params.argtypes = [C.POINTER(TriMeshParams)]
        L.ppp_default_trimesh_params.restype = None
        L.ppp_trimesh_create.argtypes = [vp, fp, sz, ip, sz, C.POINTER(TriMeshParams), fp, C.POINTER(vp), C.POINTER(TriMeshStats)]
        L.ppp_trimesh_create_stl.argtypes = [vp, C.c_char_p, C.POINTER(TriMeshParams), fp, C.POINTER(vp), C.POINTER(TriMeshStats)]
        L.ppp_trimesh_destroy.argtypes = [vp]
        L.ppp_trimesh_destroy.restype = None
        L.ppp_trimesh_nearest.argtypes = [vp, fp, sz, C.c_float, dp, dp, dp, ip, ubp, ubp]
        L.ppp_get_mesh_deviation.argtypes = [vp, vp, C.POINTER(DeviationParams), dp, dp, dp, ip, ubp, ubp, dp, sz, C.POINTER(MeshDeviationStats)]
        L.ppp_trimesh_topology.argtypes = [vp, C.POINTER(TriMeshTopologyStats)]
        L.ppp_trimesh_get_topology.argtypes = [vp, ip, ip, ubp, ubp, dp, dp, sz, C.POINTER(TriMeshTopologyStats)]
        L.ppp_trimesh_signed_nearest.argtypes = [vp, fp, sz, C.c_float, dp, dp, ubp, ubp, dp, dp, dp, ip, ubp, ubp]
        L.ppp_get_mesh_signed_deviation.argtypes = [vp, vp, C.POINTER(DeviationParams), dp, dp, dp, ip, ubp, ubp, ubp, ubp, dp, sz,
                                                    C.POINTER(MeshSignedDeviationStats)]
        L.ppp_get_mesh_registration_terms.argtypes = [vp, vp, C.POINTER(RegistrationParams), dp, C.POINTER(RegistrationRow), C.POINTER(RegistrationStats)]
        L.ppp_register_mesh.argtypes = [vp, vp, C.POINTER(RegistrationParams), dp, C.POINTER(RegistrationRow), sz, C.POINTER(RegistrationStats)]
        L.ppp_trimesh_get_moments.argtypes = [vp, C.POINTER(CloudFrame)]
        L.ppp_mesh_frame_from_moments.argtypes = [C.POINTER(C.c_longlong), C.c_int, dp, C.c_double, C.POINTER(CloudFrame)]
        L.ppp_register_mesh_global.argtypes = [vp, vp, C.POINTER(GlobalRegistrationParams), C.POINTER(RegistrationCandidate), sz, C.POINTER(RegistrationRow), sz,
                                               C.POINTER(GlobalRegistrationStats)]
        L.ppp_get_mesh_deviation_tile.argtypes = [vp, vp, C.POINTER(DeviationParams), dp, dp, dp, ip, ubp, ubp, dp, ubp, sz, C.POINTER(MeshDeviationTileStats)]
        L.ppp_get_mesh_signed_deviation_tile.argtypes = [vp, vp, C.POINTER(DeviationParams), dp, dp, dp, ip, ubp, ubp, ubp, ubp, dp, ubp, sz,
                                                         C.POINTER(MeshSignedDeviationTileStats)]
        L.ppp_merge_mesh_deviation_tiles.argtypes = [sz, C.POINTER(MeshDeviationTileStats), C.POINTER(dp), C.POINTER(ubp), C.POINTER(dp), C.POINTER(ubp),
                                                     C.POINTER(MeshDeviationStats)]
        L.ppp_merge_mesh_signed_deviation_tiles.argtypes = [sz, C.POINTER(MeshSignedDeviationTileStats), C.POINTER(dp), C.POINTER(ubp), C.POINTER(dp),
                                                            C.POINTER(ubp), C.POINTER(MeshSignedDeviationStats)]
        L.ppp_get_mesh_registration_terms_tile.argtypes = [vp, vp, C.POINTER(RegistrationParams), dp, C.POINTER(RegistrationRow), C.POINTER(RegistrationPart)]
        L.ppp_register_mesh_tiles.argtypes = [C.POINTER(vp), C.POINTER(vp), sz, C.POINTER(RegistrationParams), dp, C.POINTER(RegistrationRow), sz,
                                              C.POINTER(RegisterTilesStats)]
        L.ppp_load_stl.argtypes = [C.c_char_p, C.POINTER(fp), szp]
        L.ppp_save_stl.argtypes = [C.c_char_p, fp, sz, C.c_int]
        _lib = L
    return _lib


def default_params(**kw):
    p = Params()
    lib().ppp_default_params(C.byref(p))
    for k, v in kw.items():
        if k == "handeye":
            for j, x in enumerate(v):
                p.handeye[j] = x
        else:
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
    return p


def _f(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


# ---- host-side file formats (no GPU needed) ----
def load_pcd(path):
    """pcl::io::loadPCDFile: returns (xyz float32 [n,3], viewpoint float32 [7])."""
    L = lib()
    p = C.POINTER(C.c_float)()
    n = C.c_size_t()
    vp = np.zeros(7, np.float32)
    rc = L.ppp_load_pcd(path.encode(), C.byref(p), C.byref(n), _f(vp))
    if rc:
        raise PPPError(rc, "cannot read PCD %s" % path)
    xyz = np.ctypeslib.as_array(p, shape=(max(n.value, 1) * 3,))[: n.value * 3].reshape(-1, 3).copy()
    L.ppp_free(p)
    return xyz, vp


MESH_ALL, MESH_FRONT = 0, 1  # PPP_MESH_*


class MeshParams(C.Structure):  # ppp_mesh_params
    _fields_ = [("pitch", C.c_float), ("facing", C.c_int)]


class MeshStats(C.Structure):  # ppp_mesh_stats
    _fields_ = [("triangles", C.c_size_t), ("sampled", C.c_size_t), ("degenerate", C.c_size_t), ("culled", C.c_size_t),
                ("rows", C.c_size_t), ("samples", C.c_size_t)]


def _mesh_stats(st):
    return {k: int(getattr(st, k)) for k, _ in MeshStats._fields_}


TRIMESH_WINDING, TRIMESH_VIEWPOINT = 0, 1  # PPP_TRIMESH_*
REGION_FACE, REGION_EDGE, REGION_VERTEX, REGION_NONE = 0, 1, 2, 255  # the region map of the exact search
EDGE_BORDER, EDGE_MANIFOLD, EDGE_INCONSISTENT, EDGE_NONMANIFOLD = 0, 1, 2, 3  # PPP_EDGE_*
VERTEX_BORDER, VERTEX_IRREGULAR = 1, 2  # PPP_VERTEX_*
MESH_SIGN_BORDER, MESH_SIGN_IRREGULAR, MESH_SIGN_FALLBACK = 1, 2, 4  # PPP_MESH_SIGN_*
FEATURE_FACE, FEATURE_NONE = 6, 255  # the feature map of the signed search: 0 .. 2 a corner, 3 .. 5 a half-edge


class TriMeshParams(C.Structure):  # ppp_trimesh_params
    _fields_ = [("cell", C.c_float), ("orient", C.c_int)]


class TriMeshStats(C.Structure):  # ppp_trimesh_stats
    _fields_ = [("triangles", C.c_size_t), ("indexed", C.c_size_t), ("degenerate", C.c_size_t), ("cells", C.c_size_t * 3),
                ("pairs", C.c_size_t), ("max_per_cell", C.c_size_t), ("cell", C.c_float), ("mn", C.c_float * 3), ("mx", C.c_float * 3)]


class TriMeshTopologyStats(C.Structure):  # ppp_trimesh_topology_stats
    _fields_ = [(k, C.c_size_t) for k in ("vertices", "edges", "border_edges", "manifold_edges", "inconsistent_edges", "nonmanifold_edges",
                                          "border_vertices", "irregular_vertices")] + [("closed", C.c_int)]


def _trimesh_stats(st):
    out = {k: int(getattr(st, k)) for k in ("triangles", "indexed", "degenerate", "pairs", "max_per_cell")}
    out["cells"] = tuple(int(v) for v in st.cells)
    out["cell"] = float(st.cell)
    out["mn"] = np.array(st.mn[:], np.float32)
    out["mx"] = np.array(st.mx[:], np.float32)
    return out


class TriMesh:
    """A resident triangle mesh with its grid (ppp_trimesh): made by Engine.trimesh() / Engine.trimesh_stl(), independent of the
    engine afterwards.  stats: triangles, indexed, degenerate, cells, pairs, max_per_cell, cell, mn, mx."""

    def __init__(self, handle, stats):
        self.L = lib()
        self.m = handle
        self.stats = stats

    def nearest(self, xyz, max_dist=float("inf")):
        """(distance float64[n], closest float64[n, 3], deviation float64[n], tri_index int32[n], region uint8[n], status uint8[n])
        of n points in RESIDENT units against the mesh (ppp_trimesh_nearest): the closest point on the nearest triangle, its
        distance, the component of the offset along that facet's normal, the region of the triangle it lies in (REGION_FACE,
        REGION_EDGE, REGION_VERTEX) and DEV_MATCHED / DEV_TOO_FAR / DEV_DROPPED.  NaN, -1 and REGION_NONE where not matched."""
        q = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n = q.shape[0]
        dist, dev = np.zeros(max(n, 1), np.float64), np.zeros(max(n, 1), np.float64)
        close = np.zeros((max(n, 1), 3), np.float64)
        tri = np.zeros(max(n, 1), np.int32)
        region, status = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
        ub = C.POINTER(C.c_ubyte)
        rc = self.L.ppp_trimesh_nearest(self.m, _f(q), n, float(max_dist), _d(dist), _d(close), _d(dev), _i(tri), region.ctypes.data_as(ub),
                                        status.ctypes.data_as(ub))
        if rc:
            raise PPPError(rc, "ppp_trimesh_nearest failed")
        return dist[:n], close[:n], dev[:n], tri[:n], region[:n], status[:n]

    def topology(self, maps=True):
        """(stats dict, arrays dict) of the mesh's welded topology (ppp_trimesh_topology / ppp_trimesh_get_topology), built on
        the first call.  stats: vertices, edges, border_edges, manifold_edges, inconsistent_edges, nonmanifold_edges,
        border_vertices, irregular_vertices, closed.  arrays, per triangle and corner of the caller's list: vertex_id int32[nt, 3],
        edge_id int32[nt, 3] (corner indices 3 f + k), edge_class uint8[nt, 3] (EDGE_*), vertex_bits uint8[nt, 3] (VERTEX_*),
        vertex_normal and edge_normal float64[nt, 3, 3] (the pseudonormals, not normalised); -1, 255 and NaN for a degenerate
        triangle.  maps=False: the stats and None."""
        st = TriMeshTopologyStats()
        ub = C.POINTER(C.c_ubyte)
        arrays = None
        if not maps:
            rc = self.L.ppp_trimesh_topology(self.m, C.byref(st))
        else:
            nt = self.stats["triangles"]
            arrays = dict(vertex_id=np.zeros((nt, 3), np.int32), edge_id=np.zeros((nt, 3), np.int32), edge_class=np.zeros((nt, 3), np.uint8),
                          vertex_bits=np.zeros((nt, 3), np.uint8), vertex_normal=np.zeros((nt, 3, 3), np.float64), edge_normal=np.zeros((nt, 3, 3), np.float64))
            rc = self.L.ppp_trimesh_get_topology(self.m, _i(arrays["vertex_id"]), _i(arrays["edge_id"]), arrays["edge_class"].ctypes.data_as(ub),
                                                 arrays["vertex_bits"].ctypes.data_as(ub), _d(arrays["vertex_normal"]), _d(arrays["edge_normal"]), nt, C.byref(st))
        if rc:
            raise PPPError(rc, "ppp_trimesh_topology failed")
        return {k: int(getattr(st, k)) for k, _ in TriMeshTopologyStats._fields_}, arrays

    def signed_nearest(self, xyz, max_dist=float("inf")):
        """(signed_distance float64[n], pseudonormal float64[n, 3], feature uint8[n], flags uint8[n]) and then nearest()'s six maps,
        bit for bit (ppp_trimesh_signed_nearest): the distance with the sign of the offset's product with the angle-weighted
        pseudonormal of the feature the closest point lies on (a corner 0 .. 2, a half-edge 3 .. 5, FEATURE_FACE), and
        MESH_SIGN_BORDER / MESH_SIGN_IRREGULAR / MESH_SIGN_FALLBACK.  Negative means inside only where topology()'s closed is 1.
        NaN, FEATURE_NONE and 0 where not matched."""
        q = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n = q.shape[0]
        n1 = max(n, 1)
        sd, dist, dev = (np.zeros(n1, np.float64) for _ in range(3))
        pn, close = np.zeros((n1, 3), np.float64), np.zeros((n1, 3), np.float64)
        tri = np.zeros(n1, np.int32)
        feature, flags, region, status = (np.zeros(n1, np.uint8) for _ in range(4))
        ub = C.POINTER(C.c_ubyte)
        rc = self.L.ppp_trimesh_signed_nearest(self.m, _f(q), n, float(max_dist), _d(sd), _d(pn), feature.ctypes.data_as(ub), flags.ctypes.data_as(ub),
                                               _d(dist), _d(close), _d(dev), _i(tri), region.ctypes.data_as(ub), status.ctypes.data_as(ub))
        if rc:
            raise PPPError(rc, "ppp_trimesh_signed_nearest failed")
        return sd[:n], pn[:n], feature[:n], flags[:n], dist[:n], close[:n], dev[:n], tri[:n], region[:n], status[:n]

    def moments(self):
        """ppp_trimesh_get_moments: the frame dict of the mesh's SURFACE (cloud_moments()'s keys): count is the indexed triangles,
        words[0] the area in the fixed point 2^ms and the other nine words the area moments, so mesh_frame_from_moments(), not
        cloud_frame_from_moments(), is what turns these words into the frame"""
        f = CloudFrame()
        rc = self.L.ppp_trimesh_get_moments(self.m, C.byref(f))
        if rc:
            raise PPPError(rc, "ppp_trimesh_get_moments failed")
        return _cloud_frame(f)

    def close(self):
        if self.m:
            self.L.ppp_trimesh_destroy(self.m)
            self.m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def load_stl(path):
    """ppp_load_stl: the triangles of a binary or ASCII STL file as a soup, float32 [n_tris, 3, 3] (triangle, vertex, xyz)."""
    L = lib()
    p = C.POINTER(C.c_float)()
    n = C.c_size_t()
    rc = L.ppp_load_stl(path.encode(), C.byref(p), C.byref(n))
    if rc:
        raise PPPError(rc, "cannot read STL %s" % path)
    v = np.ctypeslib.as_array(p, shape=(max(n.value, 1) * 9,))[: n.value * 9].reshape(-1, 3, 3).copy()
    L.ppp_free(p)
    return v


def save_stl(path, verts9, binary=True):
    """ppp_save_stl: a soup (anything that reshapes to n_tris x 9 floats) as a binary or ASCII STL file."""
    v = np.ascontiguousarray(verts9, np.float32).reshape(-1, 9)
    rc = lib().ppp_save_stl(path.encode(), _f(v), v.shape[0], 1 if binary else 0)
    if rc:
        raise PPPError(rc, "cannot write STL %s" % path)


class PlannerQueue:
    """ppp_queue_*: workpieces in, lists out, `lanes` engine handles (default 2) behind it taking turns -- the passes of neighbouring
    workpieces overlap on the device.  submit(dptr, n) takes a cloud that is already in device memory (untouched until wait() of its
    ticket has returned) and returns a ticket; wait(ticket) returns (W, device pointer of the W x 6 list) -- valid until `lanes` more
    workpieces have been submitted -- or raises what that workpiece ended with."""

    def __init__(self, device=0, lanes=0, **params):
        self.L = lib()
        p = Params()
        self.L.ppp_default_params(C.byref(p))
        for k, v in params.items():
            if k == "handeye":
                for j, x in enumerate(v):
                    p.handeye[j] = x
            else:
                setattr(p, k, v)
        q = C.c_void_p()
        rc = self.L.ppp_queue_create(device, lanes, C.byref(p), C.byref(q))
        if rc:
            raise PPPError(rc, "ppp_queue_create failed")
        self.q = q
        self.lanes = self.L.ppp_queue_lanes(q)

    def _chk(self, rc):
        if rc:
            raise PPPError(rc, self.L.ppp_queue_last_error(self.q).decode())

    def submit(self, dptr, n, stride_bytes=12, viewpoint=None):
        t = C.c_longlong()
        vp = None if viewpoint is None else _f(np.ascontiguousarray(viewpoint, np.float32))
        self._chk(self.L.ppp_queue_submit(self.q, C.c_void_p(dptr), n, stride_bytes, vp, C.byref(t)))
        return t.value

    def wait(self, ticket):
        W = C.c_size_t()
        d = C.c_void_p()
        self._chk(self.L.ppp_queue_wait(self.q, ticket, C.byref(W), C.byref(d)))
        return W.value, d.value

    def close(self):
        if self.q:
            self.L.ppp_queue_destroy(self.q)
            self.q = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


CONTACT_BINS = 64  # PPP_CONTACT_BINS


class ContactStats(C.Structure):
    """ppp_contact_stats"""
    _fields_ = [("n", C.c_size_t), ("covered", C.c_size_t), ("multi_slice", C.c_size_t), ("max_count", C.c_uint),
                ("total", C.c_ulonglong), ("hist", C.c_size_t * CONTACT_BINS)]


REMOVAL_FLAT, REMOVAL_PARABOLIC, REMOVAL_HERTZ = range(3)  # PPP_REMOVAL_*


class RemovalStats(C.Structure):
    """ppp_removal_stats"""
    _fields_ = [("n", C.c_size_t), ("touched", C.c_size_t), ("min_removal", C.c_double), ("max_removal", C.c_double),
                ("sum", C.c_double), ("sum_sq", C.c_double), ("path_length", C.c_double), ("hist", C.c_size_t * CONTACT_BINS)]


class DwellRow(C.Structure):
    """ppp_dwell_row"""
    _fields_ = [("slice", C.c_int), ("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("r", C.c_float), ("ds", C.c_double),
                ("dwell", C.c_double)]


class DwellStats(C.Structure):
    """ppp_dwell_stats"""
    _fields_ = [("n", C.c_size_t), ("touched", C.c_size_t), ("rows", C.c_size_t), ("at_min", C.c_size_t), ("at_max", C.c_size_t),
                ("iterations", C.c_int), ("level", C.c_double), ("residual_before", C.c_double), ("residual_after", C.c_double),
                ("min_dwell", C.c_double), ("max_dwell", C.c_double), ("path_length", C.c_double), ("time_factor", C.c_double)]


FEED_TILE = 256  # FEED_TILE (csrc/ppp_feed.h): waypoints of a k_feed_env workgroup
FEED_LIMIT_DWELL, FEED_LIMIT_FEED_MAX, FEED_LIMIT_END, FEED_LIMIT_ACCEL = range(4)   # ppp_feed_row.limit


class FeedParams(C.Structure):
    """ppp_feed_params"""
    _fields_ = [("feed", C.c_double), ("feed_max", C.c_double), ("accel", C.c_double), ("end_feed", C.c_double),
                ("link_feed", C.c_double)]


class FeedRow(C.Structure):
    """ppp_feed_row"""
    _fields_ = [("slice", C.c_int), ("limit", C.c_int), ("dwell", C.c_double), ("s", C.c_double), ("feed", C.c_double),
                ("t", C.c_double)]


class FeedStats(C.Structure):
    """ppp_feed_stats"""
    _fields_ = [("W", C.c_size_t), ("slices", C.c_size_t), ("by_dwell", C.c_size_t), ("by_feed_max", C.c_size_t),
                ("by_end", C.c_size_t), ("by_accel", C.c_size_t), ("min_feed", C.c_double), ("max_feed", C.c_double),
                ("path_length", C.c_double), ("link_length", C.c_double), ("duration", C.c_double),
                ("duration_links", C.c_double), ("duration_nominal", C.c_double)]


DEV_MATCHED, DEV_TOO_FAR, DEV_NO_NORMAL, DEV_DROPPED = range(4)  # PPP_DEV_*


class DeviationParams(C.Structure):
    """ppp_deviation_params"""
    _fields_ = [("max_dist", C.c_float), ("smooth_radius", C.c_float), ("allowance", C.c_double), ("gain", C.c_double)]


class DeviationStats(C.Structure):
    """ppp_deviation_stats"""
    _fields_ = [("n", C.c_size_t), ("matched", C.c_size_t), ("too_far", C.c_size_t), ("no_normal", C.c_size_t), ("dropped", C.c_size_t),
                ("proud", C.c_size_t), ("below", C.c_size_t), ("min_dev", C.c_double), ("max_dev", C.c_double), ("mean_dev", C.c_double),
                ("rms_dev", C.c_double), ("max_dist2", C.c_float), ("target_sum", C.c_double), ("hist", C.c_size_t * CONTACT_BINS)]


class DeviationTileStats(C.Structure):
    """ppp_deviation_tile_stats"""
    _fields_ = [("n", C.c_size_t), ("owned", C.c_size_t), ("evaluated", C.c_size_t), ("matched", C.c_size_t), ("too_far", C.c_size_t),
                ("no_normal", C.c_size_t), ("proud", C.c_size_t), ("below", C.c_size_t), ("min_dev", C.c_double), ("max_dev", C.c_double),
                ("fix_sum", C.c_longlong), ("max_dist2", C.c_float), ("own_lo", C.c_float), ("own_hi", C.c_float), ("sum_parts", C.c_int)]


def _deviation_stats(st):
    stats = {k: getattr(st, k) for k, _ in DeviationStats._fields_ if k != "hist"}
    stats["hist"] = np.array(st.hist[:], np.int64)
    return stats


class MeshDeviationStats(C.Structure):
    """ppp_mesh_deviation_stats"""
    _fields_ = [("dev", DeviationStats), ("on_face", C.c_size_t), ("on_edge", C.c_size_t), ("on_vertex", C.c_size_t), ("max_distance", C.c_double)]


class MeshSignedDeviationStats(C.Structure):
    """ppp_mesh_signed_deviation_stats"""
    _fields_ = [("mesh", MeshDeviationStats), ("on_border", C.c_size_t), ("irregular", C.c_size_t), ("fallback", C.c_size_t), ("negative", C.c_size_t),
                ("positive", C.c_size_t)]


class MeshDeviationTileStats(C.Structure):
    """ppp_mesh_deviation_tile_stats"""
    _fields_ = [("dev", DeviationTileStats), ("on_face", C.c_size_t), ("on_edge", C.c_size_t), ("on_vertex", C.c_size_t), ("max_distance", C.c_double)]


class MeshSignedDeviationTileStats(C.Structure):
    """ppp_mesh_signed_deviation_tile_stats"""
    _fields_ = [("mesh", MeshDeviationTileStats), ("on_border", C.c_size_t), ("irregular", C.c_size_t), ("fallback", C.c_size_t), ("negative", C.c_size_t),
                ("positive", C.c_size_t)]


_MESH_TILE_FIELDS = ("on_face", "on_edge", "on_vertex", "max_distance")
_MESH_SIGNED_TILE_FIELDS = ("on_border", "irregular", "fallback", "negative", "positive")


def _mesh_tile_part(st, signed_st=None):
    """a MeshDeviationTileStats (and the signed struct around it) as one flat dict: deviation_tile()'s part, the counts by region
    and max_distance, and the signed call's five counts"""
    part = {k: getattr(st.dev, k) for k, _ in DeviationTileStats._fields_}
    part.update({k: getattr(st, k) for k in _MESH_TILE_FIELDS})
    if signed_st is not None:
        part.update({k: getattr(signed_st, k) for k in _MESH_SIGNED_TILE_FIELDS})
    return part


def _merge_mesh_tiles(tiles, signed):
    L = lib()
    T = len(tiles)
    ub, dpp = C.POINTER(C.c_ubyte), C.POINTER(C.c_double)
    # (signed_distance | deviation, smoothed, distance, tri_index, region, [feature, flags,] status, target, owned, part)
    keep = [(np.ascontiguousarray(t[1], np.float64), np.ascontiguousarray(t[-4], np.uint8), np.ascontiguousarray(t[-3], np.float64),
             np.ascontiguousarray(t[-2], np.uint8)) for t in tiles]
    vv = (dpp * max(T, 1))(*[_d(k[0]) for k in keep])
    ss = (ub * max(T, 1))(*[k[1].ctypes.data_as(ub) for k in keep])
    tt = (dpp * max(T, 1))(*[_d(k[2]) for k in keep])
    oo = (ub * max(T, 1))(*[k[3].ctypes.data_as(ub) for k in keep])
    parts = ((MeshSignedDeviationTileStats if signed else MeshDeviationTileStats) * max(T, 1))()
    for i, t in enumerate(tiles):
        part = t[-1]
        mesh = parts[i].mesh if signed else parts[i]
        for f, _ in DeviationTileStats._fields_:
            setattr(mesh.dev, f, part[f])
        for f in _MESH_TILE_FIELDS:
            setattr(mesh, f, part[f])
        if signed:
            for f in _MESH_SIGNED_TILE_FIELDS:
                setattr(parts[i], f, part[f])
        if any(len(a) != part["n"] for a in keep[i]):
            raise PPPError(ERR_ARG, "merge of mesh deviation tiles: tile %d's maps do not hold n entries" % i)
    st = MeshSignedDeviationStats() if signed else MeshDeviationStats()
    call = L.ppp_merge_mesh_signed_deviation_tiles if signed else L.ppp_merge_mesh_deviation_tiles
    rc = call(T, parts, vv, ss, tt, oo, C.byref(st))
    if rc:
        raise PPPError(rc, "merge of mesh deviation tiles: a point owned twice, a part that is not its maps', or tiles that do not belong together")
    mesh = st.mesh if signed else st
    stats = _deviation_stats(mesh.dev)
    stats.update(on_face=int(mesh.on_face), on_edge=int(mesh.on_edge), on_vertex=int(mesh.on_vertex), max_distance=float(mesh.max_distance))
    if signed:
        stats.update({k: int(getattr(st, k)) for k in _MESH_SIGNED_TILE_FIELDS})
    return stats, st


def merge_mesh_deviation_tiles(tiles):
    """Engine.mesh_deviation()'s stats dict of the whole cloud, bit for bit, from the tiles of ranges that tile the walk
    (ppp_merge_mesh_deviation_tiles: host only).  tiles = a sequence of Engine.mesh_deviation_tile() results.  deviation()'s
    fields merge as merge_deviation_tiles() merges them, the counts by region add, max_distance is the maximum (NaN when nothing
    matched)"""
    return _merge_mesh_tiles(tiles, False)[0]


def merge_mesh_signed_deviation_tiles(tiles):
    """Engine.mesh_signed_deviation()'s stats dict of the whole cloud, bit for bit, from a sequence of
    Engine.mesh_signed_deviation_tile() results (ppp_merge_mesh_signed_deviation_tiles: host only)"""
    return _merge_mesh_tiles(tiles, True)[0]


def merge_deviation_tiles(tiles):
    """ppp_deviation_stats of the whole cloud, as Engine.deviation()'s dict and bit for bit, from the tiles of ranges that tile the
    walk (ppp_merge_deviation_tiles: host only).  tiles = a sequence of Engine.deviation_tile() results (deviation, smoothed,
    ref_index, status, target, owned, part).  The counts, the integer sum and the extrema merge from the parts; hist, rms_dev and
    target_sum are computed here from the union of the owned entries of smoothed, status and target, in the whole-cloud call's
    fixed order."""
    L = lib()
    T = len(tiles)
    ub = C.POINTER(C.c_ubyte)
    keep = [(np.ascontiguousarray(t[1], np.float64), np.ascontiguousarray(t[3], np.uint8), np.ascontiguousarray(t[4], np.float64),
             np.ascontiguousarray(t[5], np.uint8)) for t in tiles]
    dpp = C.POINTER(C.c_double)
    vv = (dpp * T)(*[_d(k[0]) for k in keep])
    ss = (ub * T)(*[k[1].ctypes.data_as(ub) for k in keep])
    tt = (dpp * T)(*[_d(k[2]) for k in keep])
    oo = (ub * T)(*[k[3].ctypes.data_as(ub) for k in keep])
    parts = (DeviationTileStats * T)()
    for i, t in enumerate(tiles):
        for f, _ in DeviationTileStats._fields_:
            setattr(parts[i], f, t[6][f])
        if any(len(a) != t[6]["n"] for a in keep[i]):
            raise PPPError(ERR_ARG, "ppp_merge_deviation_tiles: tile %d's maps do not hold n entries" % i)
    st = DeviationStats()
    rc = L.ppp_merge_deviation_tiles(T, parts, vv, ss, tt, oo, C.byref(st))
    if rc:
        raise PPPError(rc, "ppp_merge_deviation_tiles: a point owned twice, a part that is not its maps', or tiles that do not belong together")
    return _deviation_stats(st)


class RegistrationParams(C.Structure):
    """ppp_registration_params"""
    _fields_ = [("max_dist", C.c_float), ("iterations", C.c_int), ("min_step", C.c_double), ("lock_eps", C.c_double)]


class RegistrationRow(C.Structure):
    """ppp_registration_row"""
    _fields_ = [("T", C.c_double * 12), ("pairs", C.c_size_t), ("A", C.c_longlong * 21), ("b", C.c_longlong * 6), ("E", C.c_longlong),
                ("locked", C.c_int), ("step2", C.c_double)]


class RegistrationStats(C.Structure):
    """ppp_registration_stats"""
    _fields_ = [("n", C.c_size_t), ("indexed", C.c_size_t), ("steps", C.c_int), ("converged", C.c_int), ("locked", C.c_int),
                ("shift", C.c_int), ("centre", C.c_double * 3), ("length", C.c_double), ("T", C.c_double * 12),
                ("pairs_before", C.c_size_t), ("pairs_after", C.c_size_t), ("rms_before", C.c_double), ("rms_after", C.c_double)]


class RegistrationPart(C.Structure):
    """ppp_registration_part"""
    _fields_ = [("owned", C.c_size_t), ("evaluated", C.c_size_t), ("own_lo", C.c_float), ("own_hi", C.c_float), ("n", C.c_size_t),
                ("shift", C.c_int), ("centre", C.c_double * 3), ("length", C.c_double)]


class RegisterTilesStats(C.Structure):
    """ppp_register_tiles_stats"""
    _fields_ = [("reg", RegistrationStats), ("failed_tile", C.c_int)]


STEP_TAKEN, STEP_FEW_PAIRS, STEP_STATIONARY, STEP_ALL_LOCKED = range(4)  # PPP_STEP_*


class TrimmedRegistrationParams(C.Structure):
    """ppp_trimmed_registration_params"""
    _fields_ = [("icp", RegistrationParams), ("keep", C.c_double)]


class TrimmedRegistrationRow(C.Structure):
    """ppp_trimmed_registration_row"""
    _fields_ = [("row", RegistrationRow), ("paired", C.c_size_t), ("trim_d2", C.c_float)]


TRIM_KEPT, TRIM_TRIMMED, TRIM_UNPAIRED, TRIM_DROPPED = range(4)  # PPP_TRIM_*


def _trimmed_registration_row(r):
    """a TrimmedRegistrationRow as a dict: _registration_row's fields (pairs = kept) with paired and trim_d2 (a Python float of
    the float32; trim_bits its bit pattern)"""
    out = _registration_row(r.row)
    out["paired"] = int(r.paired)
    out["trim_d2"] = float(r.trim_d2)
    out["trim_bits"] = int(np.array([r.trim_d2], np.float32).view(np.uint32)[0])
    return out


class MeshTrimmedRegistrationParams(C.Structure):
    """ppp_mesh_trimmed_registration_params"""
    _fields_ = [("trim", TrimmedRegistrationParams), ("border", C.c_int)]


class MeshTrimmedRegistrationRow(C.Structure):
    """ppp_mesh_trimmed_registration_row"""
    _fields_ = [("trim", TrimmedRegistrationRow), ("on_border", C.c_size_t)]


MESH_BORDER_PAIR, MESH_BORDER_REJECT = range(2)  # PPP_MESH_BORDER_*
MESH_TRIM_BORDER = 4                             # PPP_MESH_TRIM_BORDER, beside TRIM_KEPT .. TRIM_DROPPED


def _mesh_trimmed_registration_row(r):
    """a MeshTrimmedRegistrationRow as a dict: _trimmed_registration_row's fields with on_border"""
    out = _trimmed_registration_row(r.trim)
    out["on_border"] = int(r.on_border)
    return out


class RobustRegistrationParams(C.Structure):
    """ppp_robust_registration_params"""
    _fields_ = [("icp", RegistrationParams), ("tune", C.c_double), ("sigma_min", C.c_double)]


class RobustRegistrationRow(C.Structure):
    """ppp_robust_registration_row"""
    _fields_ = [("row", RegistrationRow), ("used", C.c_size_t), ("weight_sum", C.c_longlong), ("median_abs", C.c_float), ("sigma", C.c_double)]


ROBUST_USED, ROBUST_REJECTED, ROBUST_UNPAIRED, ROBUST_DROPPED = range(4)  # PPP_ROBUST_*


def _robust_registration_row(r):
    """a RobustRegistrationRow as a dict: _registration_row's fields (pairs = paired, A / b / E weighted) with used, weight_sum,
    median_abs (a Python float of the float32; median_bits its bit pattern) and sigma"""
    out = _registration_row(r.row)
    out["used"] = int(r.used)
    out["weight_sum"] = int(r.weight_sum)
    out["median_abs"] = float(r.median_abs)
    out["median_bits"] = int(np.array([r.median_abs], np.float32).view(np.uint32)[0])
    out["sigma"] = float(r.sigma)
    return out


def _registration_row(r):
    """a RegistrationRow as a dict: T float64[3, 4], pairs, A int64[21], b int64[6], E, locked, step2"""
    return dict(T=np.array(r.T[:], np.float64).reshape(3, 4), pairs=int(r.pairs), A=np.array(r.A[:], np.int64), b=np.array(r.b[:], np.int64),
                E=int(r.E), locked=int(r.locked), step2=float(r.step2))


def _registration_stats(st):
    out = {k: getattr(st, k) for k, _ in RegistrationStats._fields_}
    out["centre"] = np.array(st.centre[:], np.float64)
    out["T"] = np.array(st.T[:], np.float64).reshape(3, 4)
    return out


def _registration_part(p):
    """a RegistrationPart as a dict: owned, evaluated, own_lo, own_hi, n, shift, centre float64[3], length"""
    out = {k: getattr(p, k) for k, _ in RegistrationPart._fields_}
    out["centre"] = np.array(p.centre[:], np.float64)
    return out


def _row_struct(row, into=None):
    r = RegistrationRow() if into is None else into
    r.T[:] = [float(v) for v in np.asarray(row["T"], np.float64).reshape(12)]
    r.pairs = int(row["pairs"])
    r.A[:] = [int(v) for v in row["A"]]
    r.b[:] = [int(v) for v in row["b"]]
    r.E = int(row["E"])
    r.locked = int(row.get("locked", 63))
    r.step2 = float(row.get("step2", float("nan")))
    return r


def _part_struct(part, into=None):
    p = RegistrationPart() if into is None else into
    for k in ("owned", "evaluated", "own_lo", "own_hi", "n", "shift", "length"):
        setattr(p, k, part[k])
    p.centre[:] = [float(v) for v in part["centre"]]
    return p


def merge_registration_terms(tiles, T=None):
    """(row, part) of the whole cloud from the tiles of ranges that tile the walk (ppp_merge_registration_terms: host only).
    tiles = a sequence of Engine.registration_terms_tile() results (row, part).  The 29 words and pairs add as signed 64-bit
    integers, owned and evaluated add; row["T"] = T (3 x 4, None: the identity).  The row is Engine.registration_terms()'s on
    whole-cloud engines, bit for bit.  PPPError(ERR_ARG): no tile, parts that disagree on n, shift, centre or length, owned
    intervals that overlap"""
    k = len(tiles)
    rows, parts = (RegistrationRow * max(k, 1))(), (RegistrationPart * max(k, 1))()
    for i, (row, part) in enumerate(tiles):
        _row_struct(row, rows[i])
        _part_struct(part, parts[i])
    out, opart = RegistrationRow(), RegistrationPart()
    t = _t12(T)
    rc = lib().ppp_merge_registration_terms(rows, parts, k, None if t is None else _d(t), C.byref(out), C.byref(opart))
    if rc:
        raise PPPError(rc, "ppp_merge_registration_terms: no tile, tiles that do not belong together, or owned intervals that overlap")
    return _registration_row(out), _registration_part(opart)


def registration_step(row, part, lock_eps=1e-9, T=None):
    """(code, T' float64[3, 4], locked, step2): the step ppp_register takes from the evaluation `row` (ppp_registration_step: host
    only); part gives centre and length, T (None: row["T"]) the transform the row was taken at.  code STEP_TAKEN, or -- with T'
    = T, locked 63 and step2 NaN -- STEP_FEW_PAIRS, STEP_STATIONARY or STEP_ALL_LOCKED"""
    r, p = _row_struct(row), _part_struct(part)
    t = _t12(T)
    out = np.zeros(12, np.float64)
    locked, step2 = C.c_int(), C.c_double()
    rc = lib().ppp_registration_step(C.byref(r), C.byref(p), float(lock_eps), None if t is None else _d(t), _d(out), C.byref(locked), C.byref(step2))
    if rc < 0:
        raise PPPError(rc, "ppp_registration_step: bad arguments")
    return rc, out.reshape(3, 4), int(locked.value), float(step2.value)


def register_tiles(engines, refs, max_dist=2.0, iterations=30, min_step=1e-6, lock_eps=1e-9, T0=None):
    """(T float64[3, 4], rows, stats) as Engine.register() gives them, bit for bit, for a scan held as slice-range engines
    (ppp_register_tiles): engines[i] holds the scan with range i, refs[i] is its reference engine (one whole-cloud engine may
    stand in every slot; refs may also be that one engine).  Every evaluation is a host round trip: the tiles' words come back,
    the host merges, solves and steps.  A tile's error is raised with its index in the message"""
    engines = list(engines)
    refs = [refs] * len(engines) if isinstance(refs, Engine) else list(refs)
    if len(refs) != len(engines):
        raise PPPError(ERR_ARG, "register_tiles: one reference per tile")
    k = len(engines)
    hs = (C.c_void_p * max(k, 1))(*[e.h for e in engines])
    rs = (C.c_void_p * max(k, 1))(*[e.h for e in refs])
    rp = RegistrationParams(float(max_dist), int(iterations), float(min_step), float(lock_eps))
    cap = max(int(iterations), 0) + 1
    rows = (RegistrationRow * cap)()
    st = RegisterTilesStats()
    t = _t12(T0)
    rc = lib().ppp_register_tiles(hs, rs, k, C.byref(rp), None if t is None else _d(t), rows, cap, C.byref(st))
    if rc:
        at = st.failed_tile if st.failed_tile >= 0 else 0
        text = engines[at].L.ppp_last_error(engines[at].h).decode() if k else "no tile"
        raise PPPError(rc, "tile %d: %s" % (st.failed_tile, text))
    stats = _registration_stats(st.reg)
    return stats["T"].copy(), [_registration_row(rows[i]) for i in range(min(cap, st.reg.steps + 1))], stats


def register_mesh_tiles(engines, meshes, max_dist=2.0, iterations=30, min_step=1e-6, lock_eps=1e-9, T0=None):
    """(T float64[3, 4], rows, stats) as Engine.register_mesh() gives them, bit for bit, for a scan held as slice-range engines
    (ppp_register_mesh_tiles): engines[i] holds the scan with range i, meshes[i] is the TriMesh on its device (one TriMesh may
    stand in every slot when all engines share a device; meshes may also be that one TriMesh).  The mesh is whole, so no range
    condition exists and no call is refused for one.  Every evaluation is a host round trip: the tiles' words come back, the host
    merges, solves and steps.  A tile's error is raised with its index in the message"""
    engines = list(engines)
    meshes = [meshes] * len(engines) if isinstance(meshes, TriMesh) else list(meshes)
    if len(meshes) != len(engines):
        raise PPPError(ERR_ARG, "register_mesh_tiles: one mesh per tile")
    k = len(engines)
    hs = (C.c_void_p * max(k, 1))(*[e.h for e in engines])
    ms = (C.c_void_p * max(k, 1))(*[None if m is None else m.m for m in meshes])
    rp = RegistrationParams(float(max_dist), int(iterations), float(min_step), float(lock_eps))
    cap = max(int(iterations), 0) + 1
    rows = (RegistrationRow * cap)()
    st = RegisterTilesStats()
    t = _t12(T0)
    rc = lib().ppp_register_mesh_tiles(hs, ms, k, C.byref(rp), None if t is None else _d(t), rows, cap, C.byref(st))
    if rc:
        at = st.failed_tile if st.failed_tile >= 0 else 0
        text = engines[at].L.ppp_last_error(engines[at].h).decode() if k else "no tile"
        raise PPPError(rc, "tile %d: %s" % (st.failed_tile, text))
    stats = _registration_stats(st.reg)
    return stats["T"].copy(), [_registration_row(rows[i]) for i in range(min(cap, st.reg.steps + 1))], stats


def trim_select(hist, rank):
    """(bin, rank_in_bin): the bin of the histogram `hist` (counts, uint32) that holds the rank-th smallest entry, 1-based -- the
    first bin whose running count reaches rank -- and the rank inside it (ppp_trim_select: host only, the device's rule).
    rank 0 or a rank above the total finds nothing: (0, 0)"""
    h = np.ascontiguousarray(hist, np.uint32)
    b, r = C.c_uint(), C.c_size_t()
    rc = lib().ppp_trim_select(h.ctypes.data_as(C.POINTER(C.c_uint)), len(h), int(rank), C.byref(b), C.byref(r))
    if rc:
        raise PPPError(rc, "ppp_trim_select: bad arguments")
    return int(b.value), int(r.value)


def trim_rank(keep, paired):
    """k of the trimmed cut (ppp_trim_rank: host only): ceil(keep * paired) in double, clamped to [1, paired]; 0 without a pair"""
    return int(lib().ppp_trim_rank(float(keep), int(paired)))


def register_trimmed_tiles(engines, refs, keep=0.8, max_dist=2.0, iterations=30, min_step=1e-6, lock_eps=1e-9, T0=None, maps=True):
    """(T float64[3, 4], rows, statuses, d2s, owneds, stats): Engine.register_trimmed()'s T, rows and stats, bit for bit, for a scan
    held as slice-range engines (ppp_register_trimmed_tiles); engines and refs as register_tiles() takes them.  statuses[i],
    d2s[i] and owneds[i] are tile i's maps of the last evaluation by cloud index: an indexed point the tile owns has owned 1 and
    register_trimmed()'s status and d2, every other entry owned 0, TRIM_DROPPED and NaN; merge_trimmed_maps() makes the whole
    cloud's of them.  An evaluation is four host round trips: three histogram merges and the sums.  maps=False returns None
    for the three lists.  A tile's error is raised with its index in the message"""
    engines = list(engines)
    refs = [refs] * len(engines) if isinstance(refs, Engine) else list(refs)
    if len(refs) != len(engines):
        raise PPPError(ERR_ARG, "register_trimmed_tiles: one reference per tile")
    k = len(engines)
    hs = (C.c_void_p * max(k, 1))(*[e.h for e in engines])
    rs = (C.c_void_p * max(k, 1))(*[e.h for e in refs])
    tp = TrimmedRegistrationParams(RegistrationParams(float(max_dist), int(iterations), float(min_step), float(lock_eps)), float(keep))
    cap = max(int(iterations), 0) + 1
    rows = (TrimmedRegistrationRow * cap)()
    st = RegisterTilesStats()
    t = _t12(T0)
    statuses = d2s = owneds = sp = dp = op = None
    n = 0
    if maps and k:
        nn = C.c_size_t()
        engines[0]._chk(lib().ppp_num_points(engines[0].h, C.byref(nn)))
        n = nn.value
        ub, fp = C.POINTER(C.c_ubyte), C.POINTER(C.c_float)
        statuses = [np.zeros(max(n, 1), np.uint8) for _ in range(k)]
        d2s = [np.zeros(max(n, 1), np.float32) for _ in range(k)]
        owneds = [np.zeros(max(n, 1), np.uint8) for _ in range(k)]
        sp = (ub * k)(*[a.ctypes.data_as(ub) for a in statuses])
        dp = (fp * k)(*[a.ctypes.data_as(fp) for a in d2s])
        op = (ub * k)(*[a.ctypes.data_as(ub) for a in owneds])
    rc = lib().ppp_register_trimmed_tiles(hs, rs, k, C.byref(tp), None if t is None else _d(t), rows, cap, sp, dp, op, n, C.byref(st))
    if rc:
        at = st.failed_tile if st.failed_tile >= 0 else 0
        text = engines[at].L.ppp_last_error(engines[at].h).decode() if k else "no tile"
        raise PPPError(rc, "tile %d: %s" % (st.failed_tile, text))
    stats = _registration_stats(st.reg)
    if statuses is not None:
        statuses, d2s, owneds = [a[:n] for a in statuses], [a[:n] for a in d2s], [a[:n] for a in owneds]
    return (stats["T"].copy(), [_trimmed_registration_row(rows[i]) for i in range(min(cap, st.reg.steps + 1))], statuses, d2s, owneds, stats)


def merge_trimmed_maps(statuses, d2s, owneds):
    """(status uint8[n], d2 float32[n]) of the whole cloud from register_trimmed_tiles()' per-tile maps (numpy only): every point
    takes the entries of the one tile that owns it; a point nobody owns is not finite: TRIM_DROPPED and NaN.
    PPPError(ERR_ARG): no tile, maps of different lengths, a point two tiles own"""
    if not len(statuses) or not (len(statuses) == len(d2s) == len(owneds)):
        raise PPPError(ERR_ARG, "merge_trimmed_maps: no tile, or lists of different lengths")
    n = len(statuses[0])
    status = np.full(n, TRIM_DROPPED, np.uint8)
    d2 = np.full(n, np.nan, np.float32)
    seen = np.zeros(n, bool)
    for s, d, o in zip(statuses, d2s, owneds):
        if not (len(s) == len(d) == len(o) == n):
            raise PPPError(ERR_ARG, "merge_trimmed_maps: maps of different lengths")
        mine = np.asarray(o) != 0
        if np.any(seen & mine):
            raise PPPError(ERR_ARG, "merge_trimmed_maps: a point two tiles own")
        seen |= mine
        status[mine] = np.asarray(s, np.uint8)[mine]
        d2[mine] = np.asarray(d, np.float32)[mine]
    return status, d2


def robust_sigma(median_bits, none, sigma_min):
    """sigma of a robust evaluation from the bits of its median |r| (ppp_robust_sigma: host only, the routine the kernels compile):
    max(1.4826 * float32(median_bits), sigma_min); none (no pair): the quiet NaN"""
    return float(lib().ppp_robust_sigma(int(median_bits) & 0xffffffff, 1 if none else 0, float(sigma_min)))


def robust_weight(r, cs, tune):
    """Tukey's biweight of the residual r at the cut cs = tune * sigma (ppp_robust_weight: host only, the routine the kernels
    compile): tune = inf: 1; cs = 0: 1 where r = 0, else 0; otherwise (1 - (r / cs)^2)^2 inside the cut and 0 from it on"""
    return float(lib().ppp_robust_weight(float(r), float(cs), float(tune)))


def register_robust_tiles(engines, refs, tune=4.685, sigma_min=1e-4, max_dist=2.0, iterations=30, min_step=1e-6, lock_eps=1e-9, T0=None, maps=True):
    """(T float64[3, 4], rows, statuses, weights, residuals, owneds, stats): Engine.register_robust()'s T, rows and stats, bit for
    bit, for a scan held as slice-range engines (ppp_register_robust_tiles); engines and refs as register_tiles() takes them.
    statuses[i], weights[i], residuals[i] and owneds[i] are tile i's maps of the last evaluation by cloud index: an indexed point
    the tile owns has owned 1 and register_robust()'s status, weight and residual, every other entry owned 0, ROBUST_DROPPED and
    NaN; merge_robust_maps() makes the whole cloud's of them.  The median is taken on the tiles' merged histograms, never on a
    tile's own: an evaluation is four host round trips, three histogram merges and the sums.  maps=False returns None for the
    four lists.  A tile's error is raised with its index in the message"""
    engines = list(engines)
    refs = [refs] * len(engines) if isinstance(refs, Engine) else list(refs)
    if len(refs) != len(engines):
        raise PPPError(ERR_ARG, "register_robust_tiles: one reference per tile")
    k = len(engines)
    hs = (C.c_void_p * max(k, 1))(*[e.h for e in engines])
    rs = (C.c_void_p * max(k, 1))(*[e.h for e in refs])
    bp = RobustRegistrationParams(RegistrationParams(float(max_dist), int(iterations), float(min_step), float(lock_eps)), float(tune), float(sigma_min))
    cap = max(int(iterations), 0) + 1
    rows = (RobustRegistrationRow * cap)()
    st = RegisterTilesStats()
    t = _t12(T0)
    statuses = weights = residuals = owneds = sp = wp = rp = op = None
    n = 0
    if maps and k:
        nn = C.c_size_t()
        engines[0]._chk(lib().ppp_num_points(engines[0].h, C.byref(nn)))
        n = nn.value
        ub, fp, dp = C.POINTER(C.c_ubyte), C.POINTER(C.c_float), C.POINTER(C.c_double)
        statuses = [np.zeros(max(n, 1), np.uint8) for _ in range(k)]
        weights = [np.zeros(max(n, 1), np.float32) for _ in range(k)]
        residuals = [np.zeros(max(n, 1), np.float64) for _ in range(k)]
        owneds = [np.zeros(max(n, 1), np.uint8) for _ in range(k)]
        sp = (ub * k)(*[a.ctypes.data_as(ub) for a in statuses])
        wp = (fp * k)(*[a.ctypes.data_as(fp) for a in weights])
        rp = (dp * k)(*[a.ctypes.data_as(dp) for a in residuals])
        op = (ub * k)(*[a.ctypes.data_as(ub) for a in owneds])
    rc = lib().ppp_register_robust_tiles(hs, rs, k, C.byref(bp), None if t is None else _d(t), rows, cap, sp, wp, rp, op, n, C.byref(st))
    if rc:
        at = st.failed_tile if st.failed_tile >= 0 else 0
        text = engines[at].L.ppp_last_error(engines[at].h).decode() if k else "no tile"
        raise PPPError(rc, "tile %d: %s" % (st.failed_tile, text))
    stats = _registration_stats(st.reg)
    if statuses is not None:
        statuses, weights, residuals, owneds = ([a[:n] for a in m] for m in (statuses, weights, residuals, owneds))
    return (stats["T"].copy(), [_robust_registration_row(rows[i]) for i in range(min(cap, st.reg.steps + 1))], statuses, weights, residuals, owneds,
            stats)


def merge_robust_maps(statuses, weights, residuals, owneds):
    """(status uint8[n], weight float32[n], residual float64[n]) of the whole cloud from register_robust_tiles()' per-tile maps
    (numpy only): every point takes the entries of the one tile that owns it; a point nobody owns is not finite: ROBUST_DROPPED
    and NaN.  PPPError(ERR_ARG): no tile, maps of different lengths, a point two tiles own"""
    if not len(statuses) or not (len(statuses) == len(weights) == len(residuals) == len(owneds)):
        raise PPPError(ERR_ARG, "merge_robust_maps: no tile, or lists of different lengths")
    n = len(statuses[0])
    status = np.full(n, ROBUST_DROPPED, np.uint8)
    weight = np.full(n, np.nan, np.float32)
    residual = np.full(n, np.nan, np.float64)
    seen = np.zeros(n, bool)
    for s, w, r, o in zip(statuses, weights, residuals, owneds):
        if not (len(s) == len(w) == len(r) == len(o) == n):
            raise PPPError(ERR_ARG, "merge_robust_maps: maps of different lengths")
        mine = np.asarray(o) != 0
        if np.any(seen & mine):
            raise PPPError(ERR_ARG, "merge_robust_maps: a point two tiles own")
        seen |= mine
        status[mine] = np.asarray(s, np.uint8)[mine]
        weight[mine] = np.asarray(w, np.float32)[mine]
        residual[mine] = np.asarray(r, np.float64)[mine]
    return status, weight, residual


class CloudFrame(C.Structure):
    """ppp_cloud_frame"""
    _fields_ = [("count", C.c_size_t), ("ms", C.c_int), ("c", C.c_double * 3), ("L", C.c_double), ("words", C.c_longlong * 10),
                ("mean", C.c_double * 3), ("axes", C.c_double * 9), ("eigenvalues", C.c_double * 3)]


class GlobalRegistrationParams(C.Structure):
    """ppp_global_registration_params"""
    _fields_ = [("candidates", C.c_int), ("stride", C.c_int), ("coarse", RegistrationParams), ("fine", RegistrationParams)]


class RegistrationCandidate(C.Structure):
    """ppp_registration_candidate"""
    _fields_ = [("index", C.c_int), ("T0", C.c_double * 12), ("T", C.c_double * 12), ("steps", C.c_int), ("converged", C.c_int),
                ("locked", C.c_int), ("pairs0", C.c_size_t), ("pairs", C.c_size_t), ("E0", C.c_longlong), ("E", C.c_longlong),
                ("cost", C.c_longlong)]


class GlobalRegistrationStats(C.Structure):
    """ppp_global_registration_stats"""
    _fields_ = [("fine", RegistrationStats), ("scan", CloudFrame), ("ref", CloudFrame), ("queries", C.c_size_t), ("shift", C.c_int),
                ("candidates", C.c_int), ("winner", C.c_int), ("winner_cost", C.c_longlong), ("second_cost", C.c_longlong)]


def _cloud_frame(f):
    """a CloudFrame as a dict: count, ms, c float64[3], L, words int64[10], mean float64[3], axes float64[3, 3] (column k is
    axis k), eigenvalues float64[3]"""
    return dict(count=int(f.count), ms=int(f.ms), c=np.array(f.c[:], np.float64), L=float(f.L), words=np.array(f.words[:], np.int64),
                mean=np.array(f.mean[:], np.float64), axes=np.array(f.axes[:], np.float64).reshape(3, 3),
                eigenvalues=np.array(f.eigenvalues[:], np.float64))


def _frame_struct(frame):
    f = CloudFrame()
    f.count, f.ms, f.L = int(frame["count"]), int(frame["ms"]), float(frame["L"])
    f.c[:] = [float(v) for v in frame["c"]]
    f.words[:] = [int(v) for v in frame["words"]]
    f.mean[:] = [float(v) for v in frame["mean"]]
    f.axes[:] = [float(v) for v in np.asarray(frame["axes"], np.float64).reshape(9)]
    f.eigenvalues[:] = [float(v) for v in frame["eigenvalues"]]
    return f


def _registration_candidate(c):
    return dict(index=int(c.index), T0=np.array(c.T0[:], np.float64).reshape(3, 4), T=np.array(c.T[:], np.float64).reshape(3, 4),
                steps=int(c.steps), converged=int(c.converged), locked=int(c.locked), pairs0=int(c.pairs0), pairs=int(c.pairs),
                E0=int(c.E0), E=int(c.E), cost=int(c.cost))


def cloud_frame_from_moments(words, ms, c, L):
    """ppp_cloud_frame_from_moments (host only, no device): the frame dict of the ten integer words, their fixed point 2^ms, the
    box centre c and the length L"""
    w = (C.c_longlong * 10)(*[int(v) for v in words])
    cc = (C.c_double * 3)(*[float(v) for v in c])
    f = CloudFrame()
    rc = lib().ppp_cloud_frame_from_moments(w, int(ms), cc, float(L), C.byref(f))
    if rc:
        raise PPPError(rc, "ppp_cloud_frame_from_moments: bad arguments")
    return _cloud_frame(f)


def mesh_frame_from_moments(words, ms, c, L):
    """ppp_mesh_frame_from_moments (host only, no device): the frame dict of the ten area words of TriMesh.moments(), their
    fixed point 2^ms, the box centre c and the length L; count is 0: the words do not hold it"""
    w = (C.c_longlong * 10)(*[int(v) for v in words])
    cc = (C.c_double * 3)(*[float(v) for v in c])
    f = CloudFrame()
    rc = lib().ppp_mesh_frame_from_moments(w, int(ms), cc, float(L), C.byref(f))
    if rc:
        raise PPPError(rc, "ppp_mesh_frame_from_moments: bad arguments")
    return _cloud_frame(f)


def registration_starts(scan_frame, ref_frame, candidates=24):
    """ppp_registration_starts (host only, no device): float64[candidates, 3, 4], the rigid motions the two frame dicts imply,
    in the header's fixed order; candidates is 4 or 24"""
    out = np.zeros((max(int(candidates), 0), 3, 4), np.float64)
    a, b = _frame_struct(scan_frame), _frame_struct(ref_frame)
    rc = lib().ppp_registration_starts(C.byref(a), C.byref(b), int(candidates), out.ctypes.data_as(C.POINTER(C.c_double)))
    if rc:
        raise PPPError(rc, "ppp_registration_starts: bad arguments")
    return out


def _t12(T):
    """a 3 x 4 (or 4 x 4: its first three rows) transform as 12 doubles for the library; None stays None: the identity"""
    if T is None:
        return None
    return np.ascontiguousarray(np.asarray(T, np.float64).reshape(-1)[:12])


class ContactFieldStats(C.Structure):
    """ppp_contact_field_stats"""
    _fields_ = [("n", C.c_size_t), ("valid", C.c_size_t), ("narrow", C.c_size_t), ("min_abs_r", C.c_float), ("max_abs_r", C.c_float),
                ("sum_abs_r", C.c_double), ("hist", C.c_size_t * CONTACT_BINS)]


REGIONS_UNCOVERED, REGIONS_OVERLAP, REGIONS_NARROW, REGIONS_MASK = range(4)  # PPP_REGIONS_*


class Region(C.Structure):
    """ppp_region"""
    _fields_ = [("label", C.c_int), ("count", C.c_uint), ("mn", C.c_float * 3), ("mx", C.c_float * 3), ("centroid", C.c_double * 3)]


class RegionStats(C.Structure):
    """ppp_region_stats"""
    _fields_ = [("n", C.c_size_t), ("selected", C.c_size_t), ("regions", C.c_size_t), ("singletons", C.c_size_t), ("largest", C.c_size_t)]


REGION_DTYPE = np.dtype([("label", np.int32), ("count", np.uint32), ("mn", np.float32, 3), ("mx", np.float32, 3),
                         ("centroid", np.float64, 3)], align=True)


class ContactFieldTileStats(C.Structure):
    """ppp_contact_field_tile_stats"""
    _fields_ = ContactFieldStats._fields_ + [("owned", C.c_size_t), ("evaluated", C.c_size_t), ("own_lo", C.c_float), ("own_hi", C.c_float)]


class RegionHalo(C.Structure):
    """ppp_region_halo"""
    _fields_ = [("cloud_index", C.c_int), ("label", C.c_int)]


class RegionPart(C.Structure):
    """ppp_region_part"""
    _fields_ = [("label", C.c_int), ("count", C.c_uint), ("mn", C.c_float * 3), ("mx", C.c_float * 3), ("fsum", C.c_longlong * 3)]


class RegionTileStats(C.Structure):
    """ppp_region_tile_stats"""
    _fields_ = [("n", C.c_size_t), ("selected", C.c_size_t), ("parts", C.c_size_t), ("halo_points", C.c_size_t),
                ("max_abs_coord", C.c_double), ("own_lo", C.c_float), ("own_hi", C.c_float)]


REGION_PART_DTYPE = np.dtype([("label", np.int32), ("count", np.uint32), ("mn", np.float32, 3), ("mx", np.float32, 3),
                              ("fsum", np.int64, 3)], align=True)
REGION_HALO_DTYPE = np.dtype([("cloud_index", np.int32), ("label", np.int32)], align=True)
_TILE_STATS = ("n", "selected", "parts", "halo_points", "max_abs_coord", "own_lo", "own_hi")


def merge_region_tiles(tiles, labels=True):
    """(labels int32[n] | None, regions, stats dict) of the whole cloud from the tiles of ranges that tile the walk
    (ppp_merge_region_tiles: host only).  tiles = a sequence of Engine.regions_tile() results (labels, parts, halos, stats).
    The same bits as Engine.regions() on a whole-cloud handle with that mask or threshold and link radius."""
    L = lib()
    T = len(tiles)
    keep = [(np.ascontiguousarray(t[0], np.int32), np.ascontiguousarray(t[1], REGION_PART_DTYPE),
             np.ascontiguousarray(t[2], REGION_HALO_DTYPE)) for t in tiles]
    ip = C.POINTER(C.c_int)
    lp = (ip * T)(*[_i(k[0]) for k in keep])
    pp = (C.POINTER(RegionPart) * T)(*[k[1].ctypes.data_as(C.POINTER(RegionPart)) for k in keep])
    hp = (C.POINTER(RegionHalo) * T)(*[k[2].ctypes.data_as(C.POINTER(RegionHalo)) for k in keep])
    sts = (RegionTileStats * T)()
    for i, t in enumerate(tiles):
        for f in _TILE_STATS:
            setattr(sts[i], f, t[3][f])
    st = RegionStats()

    def chk(rc):
        if rc:
            raise PPPError(rc, "ppp_merge_region_tiles: a point owned twice, a halo point nobody owns, or tiles that do not belong together")

    chk(L.ppp_merge_region_tiles(T, lp, pp, hp, sts, None, 0, None, 0, C.byref(st)))
    lab = np.empty(max(st.n, 1), np.int32) if labels else None
    rows = np.zeros(max(st.regions, 1), REGION_DTYPE)
    chk(L.ppp_merge_region_tiles(T, lp, pp, hp, sts, None if lab is None else _i(lab), st.n if labels else 0,
                                 rows.ctypes.data_as(C.POINTER(Region)), st.regions, C.byref(st)))
    stats = dict(n=st.n, selected=st.selected, regions=st.regions, singletons=st.singletons, largest=st.largest)
    return (lab[:st.n] if labels else None), rows[:st.regions], stats


class PcdLayout(C.Structure):
    _fields_ = [("data_kind", C.c_int), ("points", C.c_size_t), ("record_bytes", C.c_size_t), ("x_offset", C.c_int), ("y_offset", C.c_int),
                ("z_offset", C.c_int), ("xyz_float32", C.c_int), ("data_offset", C.c_longlong), ("viewpoint", C.c_float * 7)]


def pcd_probe(path):
    """The header of a PCD file: ppp_pcd_layout (data_kind 0 ascii / 1 binary / 2 binary_compressed, points, record layout)."""
    lay = PcdLayout()
    rc = lib().ppp_pcd_probe(path.encode(), C.byref(lay))
    if rc:
        raise PPPError(rc, "cannot read PCD %s" % path)
    return lay


def save_pcd(path, xyz, viewpoint=None, binary=True):
    xyz = np.ascontiguousarray(xyz, np.float32)
    vp = None if viewpoint is None else _f(np.ascontiguousarray(viewpoint, np.float32))
    mode = 2 if binary == "compressed" else (1 if binary else 0)
    rc = lib().ppp_save_pcd(path.encode(), _f(xyz), xyz.shape[0], xyz.shape[1], vp, mode)
    if rc:
        raise PPPError(rc, "cannot write PCD %s" % path)


def read_config(path):
    c = Config()
    lib().ppp_default_config(C.byref(c))
    rc = lib().ppp_read_config(path.encode(), C.byref(c))
    return rc, c


def write_path_file(path, wp6):
    wp6 = np.ascontiguousarray(wp6, np.float32)
    rc = lib().ppp_write_path_file(path.encode(), _f(wp6), wp6.shape[0])
    if rc:
        raise PPPError(rc, "cannot write %s" % path)


def write_feed_file(path, wp6, rows):
    """pathFile's six columns, then t and feed of path_feed()'s rows (ppp_write_feed_file)"""
    wp6 = np.ascontiguousarray(wp6, np.float32)
    rows = np.ascontiguousarray(rows, np.dtype(FeedRow))
    if wp6.ndim != 2 or wp6.shape[1] != 6 or rows.shape != (wp6.shape[0],):
        raise ValueError("wp6 must be W x 6 and rows hold one row per waypoint")
    rc = lib().ppp_write_feed_file(path.encode(), _f(wp6), rows.ctypes.data_as(C.POINTER(FeedRow)), wp6.shape[0])
    if rc:
        raise PPPError(rc, "cannot write %s" % path)


def _d(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _i(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def run_batch_async(engines, dst_ptr=None, offsets=None, caps=None):
    """GenPath + getPath of several handles of one GPU as ONE hipGraph with a branch per handle (BASELINE config 3).
    With dst_ptr every list is also copied to dst_ptr + 24 * offsets[i] bytes (at most caps[i] rows)."""
    L = lib()
    n = len(engines)
    hs = (C.c_void_p * n)(*[e.h for e in engines])
    if dst_ptr is None:
        rc = L.ppp_run_batch_async(hs, n, None, None, None)
    else:
        off = (C.c_size_t * n)(*[int(x) for x in offsets])
        cap = (C.c_size_t * n)(*[int(x) for x in caps])
        rc = L.ppp_run_batch_async(hs, n, C.c_void_p(dst_ptr), off, cap)
    if rc:
        raise PPPError(rc, L.ppp_last_error(engines[0].h).decode())


def sync_batch(engines):
    L = lib()
    n = len(engines)
    hs = (C.c_void_p * n)(*[e.h for e in engines])
    bad = C.c_size_t(0)
    rc = L.ppp_sync_batch(hs, n, C.byref(bad))
    if rc:
        raise PPPError(rc, "handle %d of the batch: %s" % (bad.value, L.ppp_last_error(engines[bad.value].h).decode()))


class Spline:
    """class Spline of the reference (include/Spline.h:7-51) on caller-supplied knots: two Steffen interpolants y -> x, y -> z
    evaluated on the device in double (ppp_spline_create / _restart / _eval)."""

    def __init__(self, y, x, z, device=0):
        self.L = lib()
        self.h = C.c_void_p()
        y, x, z = (np.ascontiguousarray(a, np.float64) for a in (y, x, z))
        rc = self.L.ppp_spline_create(int(device), len(y), _d(y), _d(x), _d(z), C.byref(self.h))
        if rc:
            self.h = None
            raise PPPError(rc, "ppp_spline_create (GSL_EINVAL: fewer than 3 knots or y not strictly increasing)" if rc == ERR_ARG else "ppp_spline_create")

    def restart(self, y, x, z):
        y, x, z = (np.ascontiguousarray(a, np.float64) for a in (y, x, z))
        rc = self.L.ppp_spline_restart(self.h, len(y), _d(y), _d(x), _d(z))
        if rc:
            raise PPPError(rc, "ppp_spline_restart")

    def point(self, y):
        """(rc, [k, 3]): Spline::point for every y; rc = ERR_DOMAIN when a y lies outside [miny, bigy] (NaN rows)."""
        y = np.ascontiguousarray(np.atleast_1d(y), np.float64)
        out = np.empty((len(y), 3))
        rc = self.L.ppp_spline_eval(self.h, _d(y), len(y), _d(out))
        if rc and rc != ERR_DOMAIN:
            raise PPPError(rc, "ppp_spline_eval")
        return rc, out

    def range(self):
        a, b, n = C.c_double(), C.c_double(), C.c_size_t()
        self.L.ppp_spline_range(self.h, C.byref(a), C.byref(b), C.byref(n))
        return a.value, b.value, n.value

    def close(self):
        if self.h:
            self.L.ppp_spline_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    """One planner handle on one MI355X (one HIP stream, one resident cloud)."""

    def __init__(self, device=0, params=None, fast_path=True, **kw):
        self.L = lib()
        self.h = C.c_void_p()
        rc = self.L.ppp_create(int(device), C.byref(self.h))
        if rc:
            self.h = None
            raise PPPError(rc, "ppp_create failed (no gfx950 device? there is no CPU fallback)")
        self.params = params if params is not None else default_params(**kw)
        self._chk(self.L.ppp_set_params(self.h, C.byref(self.params)))
        if not fast_path:
            self.set_fast_path(False)

    def set_fast_path(self, on=True):
        """ppp_set_fast_path: False keeps this handle on the slab-index launch sequence (the window path is the default where it applies)."""
        self._chk(self.L.ppp_set_fast_path(self.h, 1 if on else 0))

    def set_plan_reuse(self, on=True):
        """ppp_set_plan_reuse: False makes every new cloud take its own window census (the default lets a cloud of the same size and
        parameters inherit the capacities of the handle's earlier plan and skip that launch)."""
        self._chk(self.L.ppp_set_plan_reuse(self.h, 1 if on else 0))

    def set_side_by_side(self, handles):
        """ppp_set_side_by_side: how many handles the caller runs side by side on this device (from two on: narrower slice workgroups where
        the windows are small, room for the neighbouring passes' launches; from three on a large cloud's binning launch narrows too)."""
        self._chk(self.L.ppp_set_side_by_side(self.h, int(handles)))

    def binning_form(self):
        """ppp_get_binning_form: (threads of a workgroup, points per thread) of the window path's binning launch under the current plan;
        (0, 0) on the slab-index path."""
        t, p = C.c_int(), C.c_int()
        self._chk(self.L.ppp_get_binning_form(self.h, C.byref(t), C.byref(p)))
        return t.value, p.value

    def launch_priorities(self):
        """ppp_get_launch_priorities: the wave priorities (binning, per-slice, finish) the current plan launches the window pass with;
        all 0 for a pass alone and on the slab-index path."""
        v = [C.c_int() for _ in range(3)]
        self._chk(self.L.ppp_get_launch_priorities(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def fast_path(self):
        """True when the current plan runs the window path (three launches), False for the slab-index path."""
        a = C.c_int()
        self._chk(self.L.ppp_get_fast_path(self.h, C.byref(a)))
        return bool(a.value)

    def _chk(self, rc):
        if rc:
            raise PPPError(rc, self.L.ppp_last_error(self.h).decode())

    def close(self):
        if self.h:
            self.L.ppp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, **kw):
        for k, v in kw.items():
            if k == "handeye":
                for j, x in enumerate(v):
                    self.params.handeye[j] = x
            else:
                setattr(self.params, k, v)
        self._chk(self.L.ppp_set_params(self.h, C.byref(self.params)))

    # -- cloud (constructor of the reference classes) --
    def set_cloud(self, xyz, viewpoint=None):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        assert xyz.ndim == 2 and xyz.shape[1] >= 3
        vp = None if viewpoint is None else _f(np.ascontiguousarray(viewpoint, np.float32))
        self._chk(self.L.ppp_set_cloud(self.h, xyz.ctypes.data, xyz.shape[0], xyz.shape[1] * 4, vp))
        self.n = xyz.shape[0]

    def set_cloud_pcd(self, path):
        """The constructors' loadPCDFile + scale loop in one call: the file goes straight to HBM.  Returns (n, viewpoint[7])."""
        n = C.c_size_t()
        vp = np.zeros(7, np.float32)
        self._chk(self.L.ppp_set_cloud_pcd(self.h, path.encode(), C.byref(n), _f(vp)))
        self.n = n.value
        return n.value, vp

    def _mesh_params(self, pitch, facing):
        mp = MeshParams()
        self.L.ppp_default_mesh_params(C.byref(mp))
        mp.pitch, mp.facing = float(pitch), int(facing)
        return mp

    def set_cloud_mesh(self, verts, tris=None, pitch=0.5, facing=MESH_ALL, viewpoint=None, tri_index=False):
        """ppp_set_cloud_mesh: the surface of a triangle mesh, sampled on the device at about 1 / pitch^2 (resident units), becomes the
        resident cloud.  verts [n_verts, 3] in the file's units, tris [n_tris, 3] indices or None for a soup (three vertices per
        triangle).  Returns the stats as a dict, with "tri_index" (the triangle of every sample) in it when asked.  A refused call
        fills "stats" of the PPPError it raises."""
        verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
        n_tris = verts.shape[0] // 3 if tris is None else None
        ti = None
        if tris is not None:
            ti = np.ascontiguousarray(tris, np.int32).reshape(-1, 3)
            n_tris = ti.shape[0]
        vp = None if viewpoint is None else _f(np.ascontiguousarray(viewpoint, np.float32))
        mp, st = self._mesh_params(pitch, facing), MeshStats()
        args = (self.h, _f(verts), verts.shape[0], None if ti is None else _i(ti), n_tris, C.byref(mp), vp)
        try:
            self._chk(self.L.ppp_set_cloud_mesh(*args, None, 0, C.byref(st)))
        except PPPError as e:
            e.stats = _mesh_stats(st)
            raise
        out = _mesh_stats(st)
        self.n = out["samples"]
        if tri_index:  # (the count is known only now: a second sampling, the same bits)
            idx = np.empty(max(self.n, 1), np.int32)
            self._chk(self.L.ppp_set_cloud_mesh(*args, _i(idx), self.n, C.byref(st)))
            out["tri_index"] = idx[:self.n]
        return out

    def set_cloud_stl(self, path, pitch=0.5, facing=MESH_ALL, viewpoint=None):
        """ppp_set_cloud_stl: set_cloud_mesh of the soup of an STL file.  Returns the stats as a dict."""
        vp = None if viewpoint is None else _f(np.ascontiguousarray(viewpoint, np.float32))
        mp, st = self._mesh_params(pitch, facing), MeshStats()
        self._chk(self.L.ppp_set_cloud_stl(self.h, path.encode(), C.byref(mp), vp, C.byref(st)))
        out = _mesh_stats(st)
        self.n = out["samples"]
        return out

    def _trimesh(self, call, *args, cell=0.0, orient=TRIMESH_WINDING, viewpoint=None):
        vp = None if viewpoint is None else _f(np.ascontiguousarray(viewpoint, np.float32))
        tp, st, m = TriMeshParams(), TriMeshStats(), C.c_void_p()
        self.L.ppp_default_trimesh_params(C.byref(tp))
        tp.cell, tp.orient = float(cell), int(orient)
        try:
            self._chk(call(self.h, *args, C.byref(tp), vp, C.byref(m), C.byref(st)))
        except PPPError as e:
            e.stats = _trimesh_stats(st)
            e.handle = m.value
            raise
        return TriMesh(m, _trimesh_stats(st))

    def trimesh(self, verts, tris=None, cell=0.0, orient=TRIMESH_WINDING, viewpoint=None):
        """ppp_trimesh_create: a TriMesh of verts [n_verts, 3] in the file's units (they go through this engine's conversion, the
        x1000 under change_range) and tris [n_tris, 3] indices, or None for a soup.  cell 0 chooses the grid's cell; the answers do
        not depend on it.  orient TRIMESH_VIEWPOINT turns every facet normal to the viewpoint's side (resident units, None =
        origin).  The mesh lives on this engine's device and needs the engine no longer.  A refused call fills "stats" of the
        PPPError it raises."""
        verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
        ti = None if tris is None else np.ascontiguousarray(tris, np.int32).reshape(-1, 3)
        n_tris = verts.shape[0] // 3 if ti is None else ti.shape[0]
        return self._trimesh(self.L.ppp_trimesh_create, _f(verts), verts.shape[0], None if ti is None else _i(ti), n_tris, cell=cell, orient=orient,
                             viewpoint=viewpoint)

    def trimesh_stl(self, path, cell=0.0, orient=TRIMESH_WINDING, viewpoint=None):
        """ppp_trimesh_create_stl: trimesh() of the soup of an STL file."""
        return self._trimesh(self.L.ppp_trimesh_create_stl, path.encode(), cell=cell, orient=orient, viewpoint=viewpoint)

    def mesh_deviation(self, mesh, max_dist=float("inf"), smooth_radius=0.0, allowance=0.0, gain=1.0, maps=True):
        """(deviation float64[n], smoothed float64[n], distance float64[n], tri_index int32[n], region uint8[n], status uint8[n],
        target float64[n], stats dict) of this engine's cloud, the scan, against the TriMesh `mesh` (ppp_get_mesh_deviation): per
        scan point the closest point on the nearest triangle within max_dist mm, its distance, and the offset's component along
        that facet's own normal; then deviation()'s smoothing, target and statistics, unchanged.  stats: deviation()'s fields
        (no_normal is 0, max_dist2 the float of the largest squared distance) and on_face, on_edge, on_vertex, max_distance.
        maps=False returns seven Nones and stats"""
        dp = DeviationParams(float(max_dist), float(smooth_radius), float(allowance), float(gain))
        st = MeshDeviationStats()
        dev = sm = dist = idx = region = status = target = None
        m = mesh.m if mesh is not None else None
        if not maps:
            self._chk(self.L.ppp_get_mesh_deviation(self.h, m, C.byref(dp), None, None, None, None, None, None, None, 0, C.byref(st)))
        else:
            nn = C.c_size_t()
            self._chk(self.L.ppp_num_points(self.h, C.byref(nn)))
            n = nn.value
            dev, sm, dist, target = (np.zeros(max(n, 1), np.float64) for _ in range(4))
            idx = np.zeros(max(n, 1), np.int32)
            region, status = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
            ub = C.POINTER(C.c_ubyte)
            self._chk(self.L.ppp_get_mesh_deviation(self.h, m, C.byref(dp), _d(dev), _d(sm), _d(dist), _i(idx), region.ctypes.data_as(ub),
                                                    status.ctypes.data_as(ub), _d(target), n, C.byref(st)))
            dev, sm, dist, idx, region, status, target = dev[:n], sm[:n], dist[:n], idx[:n], region[:n], status[:n], target[:n]
        stats = _deviation_stats(st.dev)
        stats.update(on_face=int(st.on_face), on_edge=int(st.on_edge), on_vertex=int(st.on_vertex), max_distance=float(st.max_distance))
        return dev, sm, dist, idx, region, status, target, stats

    def mesh_signed_deviation(self, mesh, max_dist=float("inf"), smooth_radius=0.0, allowance=0.0, gain=1.0, maps=True):
        """(signed_distance float64[n], smoothed float64[n], distance float64[n], tri_index int32[n], region uint8[n], feature
        uint8[n], flags uint8[n], status uint8[n], target float64[n], stats dict): mesh_deviation() with the signed distance of
        TriMesh.signed_nearest() in the deviation's place (ppp_get_mesh_signed_deviation): smoothed, target and the statistics are
        computed from it.  stats: mesh_deviation()'s fields and on_border, irregular, fallback, negative, positive.  maps=False
        returns nine Nones and stats"""
        dp = DeviationParams(float(max_dist), float(smooth_radius), float(allowance), float(gain))
        st = MeshSignedDeviationStats()
        sd = sm = dist = idx = region = feature = flags = status = target = None
        m = mesh.m if mesh is not None else None
        if not maps:
            self._chk(self.L.ppp_get_mesh_signed_deviation(self.h, m, C.byref(dp), None, None, None, None, None, None, None, None, None, 0, C.byref(st)))
        else:
            nn = C.c_size_t()
            self._chk(self.L.ppp_num_points(self.h, C.byref(nn)))
            n = nn.value
            n1 = max(n, 1)
            sd, sm, dist, target = (np.zeros(n1, np.float64) for _ in range(4))
            idx = np.zeros(n1, np.int32)
            region, feature, flags, status = (np.zeros(n1, np.uint8) for _ in range(4))
            ub = C.POINTER(C.c_ubyte)
            self._chk(self.L.ppp_get_mesh_signed_deviation(self.h, m, C.byref(dp), _d(sd), _d(sm), _d(dist), _i(idx), region.ctypes.data_as(ub),
                                                           feature.ctypes.data_as(ub), flags.ctypes.data_as(ub), status.ctypes.data_as(ub), _d(target), n,
                                                           C.byref(st)))
            sd, sm, dist, idx, region, feature, flags, status, target = (a[:n] for a in (sd, sm, dist, idx, region, feature, flags, status, target))
        stats = _deviation_stats(st.mesh.dev)
        stats.update(on_face=int(st.mesh.on_face), on_edge=int(st.mesh.on_edge), on_vertex=int(st.mesh.on_vertex), max_distance=float(st.mesh.max_distance),
                     on_border=int(st.on_border), irregular=int(st.irregular), fallback=int(st.fallback), negative=int(st.negative), positive=int(st.positive))
        return sd, sm, dist, idx, region, feature, flags, status, target, stats

    def mesh_registration_terms(self, mesh, T=None, max_dist=2.0, lock_eps=1e-9):
        """(row, stats) of one evaluation of the point-to-plane terms of this engine's cloud, the scan, moved by T (3 x 4, None:
        the identity), against the TriMesh `mesh` (ppp_get_mesh_registration_terms): the partner of a moved point is the closest
        point on its nearest triangle within max_dist mm, the normal that facet's own.  row and stats as registration_terms()
        gives them; no step is taken"""
        rp = RegistrationParams(float(max_dist), 1, 0.0, float(lock_eps))
        row, st = RegistrationRow(), RegistrationStats()
        t = _t12(T)
        m = mesh.m if mesh is not None else None
        self._chk(self.L.ppp_get_mesh_registration_terms(self.h, m, C.byref(rp), None if t is None else _d(t), C.byref(row), C.byref(st)))
        return _registration_row(row), _registration_stats(st)

    def register_mesh(self, mesh, T0=None, rows=True, max_dist=2.0, iterations=30, min_step=1e-6, lock_eps=1e-9):
        """(T float64[3, 4], rows, stats): point-to-plane ICP of this engine's cloud, the scan, to the triangles of the TriMesh
        `mesh` themselves (ppp_register_mesh), started at T0 (None: the identity): register()'s loop with the exact closest point
        and the facet's own normal in the place of a sample and its estimated normal, so that neither a pitch nor a smeared crease
        enters the fit.  T, rows and stats as register() gives them; rows=False asks for none, an integer caps their number.
        Neither the cloud nor the mesh is changed"""
        rp = RegistrationParams(float(max_dist), int(iterations), float(min_step), float(lock_eps))
        cap = max(int(iterations), 0) + 1 if rows is True else (0 if rows is False else int(rows))
        out = (RegistrationRow * max(cap, 1))()
        st = RegistrationStats()
        t = _t12(T0)
        m = mesh.m if mesh is not None else None
        self._chk(self.L.ppp_register_mesh(self.h, m, C.byref(rp), None if t is None else _d(t), out if cap else None, cap, C.byref(st)))
        stats = _registration_stats(st)
        return stats["T"].copy(), [_registration_row(out[k]) for k in range(min(cap, st.steps + 1))], stats

    def mesh_deviation_tile(self, mesh, max_dist=float("inf"), smooth_radius=0.0, allowance=0.0, gain=1.0, maps=True):
        """(deviation, smoothed, distance, tri_index, region, status, target, owned uint8[n], part dict): mesh_deviation() for the
        points this engine OWNS -- a slice-range engine of the scan, or a whole-cloud one, which owns every indexed point -- against
        the TriMesh `mesh` on this engine's device (ppp_get_mesh_deviation_tile).  The maps go by cloud index; an owned point's
        entries are mesh_deviation()'s bits on a whole-cloud engine, every other point has DEV_DROPPED, -1, 255, NaN, 0 and owned
        0.  The mesh is whole, so there is no halo: only this engine's range_margin must cover smooth_radius.  part:
        deviation_tile()'s fields and on_face, on_edge, on_vertex, max_distance -- what merge_mesh_deviation_tiles() takes.
        maps=False returns eight Nones and part"""
        dp = DeviationParams(float(max_dist), float(smooth_radius), float(allowance), float(gain))
        st = MeshDeviationTileStats()
        dev = sm = dist = idx = region = status = target = owned = None
        m = mesh.m if mesh is not None else None
        if not maps:
            self._chk(self.L.ppp_get_mesh_deviation_tile(self.h, m, C.byref(dp), None, None, None, None, None, None, None, None, 0, C.byref(st)))
        else:
            nn = C.c_size_t()
            self._chk(self.L.ppp_num_points(self.h, C.byref(nn)))
            n = nn.value
            n1 = max(n, 1)
            dev, sm, dist, target = (np.zeros(n1, np.float64) for _ in range(4))
            idx = np.zeros(n1, np.int32)
            region, status, owned = (np.zeros(n1, np.uint8) for _ in range(3))
            ub = C.POINTER(C.c_ubyte)
            self._chk(self.L.ppp_get_mesh_deviation_tile(self.h, m, C.byref(dp), _d(dev), _d(sm), _d(dist), _i(idx), region.ctypes.data_as(ub),
                                                         status.ctypes.data_as(ub), _d(target), owned.ctypes.data_as(ub), n, C.byref(st)))
            dev, sm, dist, idx, region, status, target, owned = (a[:n] for a in (dev, sm, dist, idx, region, status, target, owned))
        return dev, sm, dist, idx, region, status, target, owned, _mesh_tile_part(st)

    def mesh_signed_deviation_tile(self, mesh, max_dist=float("inf"), smooth_radius=0.0, allowance=0.0, gain=1.0, maps=True):
        """(signed_distance, smoothed, distance, tri_index, region, feature, flags, status, target, owned uint8[n], part dict):
        mesh_signed_deviation() for the points this engine OWNS (ppp_get_mesh_signed_deviation_tile); mesh_deviation_tile()'s
        rules, with feature 255 and flags 0 for a point that is not owned.  part: mesh_deviation_tile()'s fields and on_border,
        irregular, fallback, negative, positive -- what merge_mesh_signed_deviation_tiles() takes.  maps=False returns ten Nones
        and part"""
        dp = DeviationParams(float(max_dist), float(smooth_radius), float(allowance), float(gain))
        st = MeshSignedDeviationTileStats()
        sd = sm = dist = idx = region = feature = flags = status = target = owned = None
        m = mesh.m if mesh is not None else None
        if not maps:
            self._chk(self.L.ppp_get_mesh_signed_deviation_tile(self.h, m, C.byref(dp), None, None, None, None, None, None, None, None, None, None, 0,
                                                                C.byref(st)))
        else:
            nn = C.c_size_t()
            self._chk(self.L.ppp_num_points(self.h, C.byref(nn)))
            n = nn.value
            n1 = max(n, 1)
            sd, sm, dist, target = (np.zeros(n1, np.float64) for _ in range(4))
            idx = np.zeros(n1, np.int32)
            region, feature, flags, status, owned = (np.zeros(n1, np.uint8) for _ in range(5))
            ub = C.POINTER(C.c_ubyte)
            self._chk(self.L.ppp_get_mesh_signed_deviation_tile(self.h, m, C.byref(dp), _d(sd), _d(sm), _d(dist), _i(idx), region.ctypes.data_as(ub),
                                                                feature.ctypes.data_as(ub), flags.ctypes.data_as(ub), status.ctypes.data_as(ub), _d(target),
                                                                owned.ctypes.data_as(ub), n, C.byref(st)))
            sd, sm, dist, idx, region, feature, flags, status, target, owned = (a[:n] for a in (sd, sm, dist, idx, region, feature, flags, status, target,
                                                                                                owned))
        return sd, sm, dist, idx, region, feature, flags, status, target, owned, _mesh_tile_part(st.mesh, st)

    def mesh_registration_terms_tile(self, mesh, T=None, max_dist=2.0, lock_eps=1e-9):
        """(row, part): mesh_registration_terms() over the points this engine OWNS -- a slice-range engine of the scan, or a
        whole-cloud one -- against the TriMesh `mesh` on this engine's device (ppp_get_mesh_registration_terms_tile).  row as
        mesh_registration_terms() gives it; part = dict(owned, evaluated, own_lo, own_hi, n, shift, centre, length), the frame
        from the mesh's box and the shift from the whole scan: what merge_registration_terms() and registration_step() take,
        unchanged.  The mesh is whole: no range condition, never ERR_CAPACITY"""
        rp = RegistrationParams(float(max_dist), 1, 0.0, float(lock_eps))
        row, part = RegistrationRow(), RegistrationPart()
        t = _t12(T)
        m = mesh.m if mesh is not None else None
        self._chk(self.L.ppp_get_mesh_registration_terms_tile(self.h, m, C.byref(rp), None if t is None else _d(t), C.byref(row), C.byref(part)))
        return _registration_row(row), _registration_part(part)

    def range_interval(self, min_x, max_x):
        """(lo, hi, S): the planner-unit x interval this handle's slice range indexes for a cloud with these x bounds."""
        lo, hi, S = C.c_float(), C.c_float(), C.c_int()
        self._chk(self.L.ppp_range_interval(C.byref(self.params), float(min_x), float(max_x), C.byref(lo), C.byref(hi), C.byref(S)))
        return lo.value, hi.value, S.value

    def range_owned(self, min_x, max_x):
        """(own_lo, own_hi): this handle's range owns the indexed points with own_lo <= x < own_hi (planner units) of a cloud
        with these x bounds: the cuts half way between neighbouring slices (ppp_range_owned)."""
        lo, hi = C.c_float(), C.c_float()
        self._chk(self.L.ppp_range_owned(C.byref(self.params), float(min_x), float(max_x), C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def set_cloud_part(self, xyz, cloud_index, mn, mx, n_valid_total, part_lo, part_hi, viewpoint=None):
        """ppp_set_cloud_part: only this handle's part of the cloud + the whole cloud's bounds / count (planner units)."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        vp = None if viewpoint is None else _f(np.ascontiguousarray(viewpoint, np.float32))
        idx = None if cloud_index is None else _i(np.ascontiguousarray(cloud_index, np.int32))
        mn = np.ascontiguousarray(mn, np.float32); mx = np.ascontiguousarray(mx, np.float32)
        self._keep = (xyz, cloud_index)
        self._chk(self.L.ppp_set_cloud_part(self.h, xyz.ctypes.data, xyz.shape[0], xyz.shape[1] * 4, vp, idx, _f(mn), _f(mx),
                                            int(n_valid_total), float(part_lo), float(part_hi)))
        self.n = xyz.shape[0]

    def set_cloud_device_async(self, dptr, n, stride_bytes, viewpoint=None):
        """ppp_set_cloud_device_async: no wait for the conversion pass where the handle's plan allows; the buffer must stay untouched
        until a call that waits (sync, any getter) has returned."""
        vp = None if viewpoint is None else _f(np.ascontiguousarray(viewpoint, np.float32))
        self._chk(self.L.ppp_set_cloud_device_async(self.h, C.c_void_p(dptr), n, stride_bytes, vp))
        self.n = n

    def set_cloud_device(self, dptr, n, stride_bytes, viewpoint=None):
        vp = None if viewpoint is None else _f(np.ascontiguousarray(viewpoint, np.float32))
        self._chk(self.L.ppp_set_cloud_device(self.h, C.c_void_p(dptr), n, stride_bytes, vp))
        self.n = n

    # -- hot path --
    def gen_path_async(self):
        self._chk(self.L.ppp_gen_path_async(self.h))

    def get_path_async(self):
        self._chk(self.L.ppp_get_path_async(self.h))

    def run_async(self):
        """GenPath() + getPath() as one enqueue (captured hipGraph)."""
        self._chk(self.L.ppp_run_async(self.h))

    def sync(self):
        self._chk(self.L.ppp_sync(self.h))

    def gen_path(self):
        """GenPath(): returns S."""
        self.gen_path_async()
        self.sync()
        return self.num_slices()

    def get_path(self):
        """getPath(): returns W."""
        self.get_path_async()
        self.sync()
        return self.num_waypoints()

    def failed_slice(self):
        return self.L.ppp_failed_slice(self.h)

    # -- results --
    def num_slices(self):
        s = C.c_int()
        self._chk(self.L.ppp_num_slices(self.h, C.byref(s)))
        return s.value

    def num_waypoints(self):
        w = C.c_size_t()
        self._chk(self.L.ppp_num_waypoints(self.h, C.byref(w)))
        return w.value

    def waypoints(self):
        W = self.num_waypoints()
        out = np.empty((W, 6), np.float32)
        w = C.c_size_t()
        self._chk(self.L.ppp_get_waypoints(self.h, _f(out), W, C.byref(w)))
        return out

    def waypoints_device(self):
        p = C.c_void_p()
        w = C.c_size_t()
        self._chk(self.L.ppp_get_waypoints_device(self.h, C.byref(p), C.byref(w)))
        return p.value, w.value

    def copy_waypoints_to_device(self, dptr, cap):
        w = C.c_size_t()
        self._chk(self.L.ppp_copy_waypoints_to_device(self.h, C.c_void_p(dptr), cap, C.byref(w)))
        return w.value

    def cloud(self):
        """The resident cloud (scaled, preprocessed) as float32 [n, 3] in index order."""
        n = C.c_size_t()
        self._chk(self.L.ppp_get_cloud(self.h, None, 0, C.byref(n)))
        out = np.empty((max(n.value, 1), 3), np.float32)
        self._chk(self.L.ppp_get_cloud(self.h, _f(out), n.value, C.byref(n)))
        return out[:n.value]

    def remove_outlier(self, mean_k=50, stddev_mul=1.0):
        """SectPath::remove_outlier (pcl::StatisticalOutlierRemoval) on the resident cloud; returns (new size, threshold)."""
        n = C.c_size_t()
        thr = C.c_double()
        self._chk(self.L.ppp_remove_outlier(self.h, int(mean_k), float(stddev_mul), C.byref(n), C.byref(thr)))
        return n.value, thr.value

    def voxel_down(self, lx, ly, lz):
        """path_generater::voxel_down (pcl::VoxelGrid) on the resident cloud; returns (new size, overflow flag)."""
        n = C.c_size_t()
        ov = C.c_int()
        self._chk(self.L.ppp_voxel_down(self.h, float(lx), float(ly), float(lz), C.byref(n), C.byref(ov)))
        return n.value, bool(ov.value)

    def smooth_mls(self, radius=15.0, order=3):
        """SectPath::smooth (pcl::MovingLeastSquares) on the resident cloud; returns the new size."""
        n = C.c_size_t()
        self._chk(self.L.ppp_smooth_mls(self.h, float(radius), int(order), C.byref(n)))
        return n.value

    def trans2center(self):
        """SectPath::trans2center on the resident cloud; returns (TransAlign 4x4, centroid, accumulated covariance 3x3)."""
        T = np.zeros(16, np.float32); c = np.zeros(3, np.float32); cov = np.zeros(9, np.float32)
        self._chk(self.L.ppp_trans2center(self.h, _f(T), _f(c), _f(cov)))
        return T.reshape(4, 4), c, cov.reshape(3, 3)

    def gather_waypoints(self, comm_ptr, rank, nranks, root, counts, recv_ptr):
        """ppp_gather_waypoints: the finished lists of all ranks to `root` over RCCL (comm_ptr = ncclComm_t)."""
        c = (C.c_size_t * nranks)(*[int(x) for x in counts])
        self._chk(self.L.ppp_gather_waypoints(self.h, C.c_void_p(comm_ptr), rank, nranks, root, c, C.c_void_p(recv_ptr)))

    def stream_ptr(self):
        """hipStream_t of this handle as an integer (torch.cuda.ExternalStream(ptr) orders framework work behind it)."""
        p = C.c_void_p()
        self._chk(self.L.ppp_get_stream(self.h, C.byref(p)))
        return p.value

    def waypoint_counts(self):
        """Waypoints per kept slice in list order (zero outside this handle's slice range)."""
        n = C.c_size_t()
        self._chk(self.L.ppp_get_waypoint_counts(self.h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.int32)
        self._chk(self.L.ppp_get_waypoint_counts(self.h, _i(out), n.value, C.byref(n)))
        return out[:n.value]

    def copy_stage_to_device(self, stage, dptr, cap):
        """D2D copy of the pre-smoothing (or smoothed) W x 6 list into a caller-owned device buffer; returns W."""
        w = C.c_size_t()
        self._chk(self.L.ppp_copy_stage_to_device(self.h, stage, C.c_void_p(dptr), cap, C.byref(w)))
        return w.value

    def finish_path_async(self, dptr, W, counts):
        """postion_smooth + reduceRPY + TransFlangeposition over a gathered pre-smoothing list in device memory
        (SURVEY.md 8e case ii: the blocks of the slice-range handles, concatenated in slice order)."""
        counts = np.ascontiguousarray(counts, np.int32)
        self._chk(self.L.ppp_finish_path_async(self.h, C.c_void_p(dptr), int(W), _i(counts), counts.size))

    def tail_index(self):
        n = C.c_size_t()
        self._chk(self.L.ppp_get_tail_index(self.h, None, 0, C.byref(n)))
        out = np.empty(max(n.value, 1), np.int32)
        self._chk(self.L.ppp_get_tail_index(self.h, _i(out), n.value, C.byref(n)))
        return out[:n.value]

    def minmax(self):
        mn = np.empty(3, np.float32)
        mx = np.empty(3, np.float32)
        self._chk(self.L.ppp_minmax(self.h, _f(mn), _f(mx)))
        return mn, mx

    def slice_positions(self):
        S = C.c_size_t()
        self._chk(self.L.ppp_get_slice_positions(self.h, None, 0, C.byref(S)))
        px = np.empty(max(S.value, 1), np.float32)
        self._chk(self.L.ppp_get_slice_positions(self.h, _f(px), S.value, C.byref(S)))
        return px[:S.value]

    def slice_indices(self, s):
        cap = 4096
        while True:
            out = np.empty(cap, np.int32)
            n = C.c_size_t()
            self._chk(self.L.ppp_get_slice_indices(self.h, int(s), _i(out), cap, C.byref(n)))
            if n.value <= cap:
                return out[:n.value].copy()
            cap = n.value

    def ranged_x_index(self, position):
        cap = 4096
        while True:
            out = np.empty(cap, np.int32)
            n = C.c_size_t()
            self._chk(self.L.ppp_ranged_x_index(self.h, int(position), _i(out), cap, C.byref(n)))
            if n.value <= cap:
                return out[:n.value].copy()
            cap = n.value

    def nodes(self, s):
        m = C.c_size_t()
        self._chk(self.L.ppp_get_nodes(self.h, int(s), None, None, None, 0, C.byref(m)))
        k = max(m.value, 1)
        y = np.empty(k); x = np.empty(k); z = np.empty(k)
        self._chk(self.L.ppp_get_nodes(self.h, int(s), _d(y), _d(x), _d(z), m.value, C.byref(m)))
        return y[:m.value], x[:m.value], z[:m.value]

    def boundary(self, s):
        """(y, x, z, step): knots of the boundary spline slice s was adjusted against (empty: none) and the slice's step in its chain"""
        m = C.c_size_t(); step = C.c_int()
        self._chk(self.L.ppp_get_boundary(self.h, int(s), None, None, None, 0, C.byref(m), C.byref(step)))
        k = max(m.value, 1)
        y = np.empty(k); x = np.empty(k); z = np.empty(k)
        self._chk(self.L.ppp_get_boundary(self.h, int(s), _d(y), _d(x), _d(z), m.value, C.byref(m), C.byref(step)))
        return y[:m.value], x[:m.value], z[:m.value], step.value

    def coverage(self, flags=True):
        """(flags uint8[n], covered) of the last pass: path_generater::get_coverage (PPP_WALK_V1_CONTACT with the dynamic
        adjustment only); flags=False asks for the count alone and returns (None, covered)"""
        n = C.c_size_t(); cov = C.c_size_t()
        if not flags:
            self._chk(self.L.ppp_get_coverage(self.h, None, 0, C.byref(n), C.byref(cov)))
            return None, cov.value
        self._chk(self.L.ppp_get_coverage(self.h, None, 0, C.byref(n), C.byref(cov)))
        out = np.zeros(max(n.value, 1), np.uint8)
        self._chk(self.L.ppp_get_coverage(self.h, out.ctypes.data_as(C.POINTER(C.c_ubyte)), n.value, C.byref(n), C.byref(cov)))
        return out[:n.value], cov.value

    def path_coverage(self, flags=True):
        """(flags uint8[n], covered) of the last pass's final paths: the contact model of get_coverage applied to every slice's
        final knots, for every walk (ppp_get_path_coverage); flags=False asks for the count alone and returns (None, covered)"""
        n = C.c_size_t(); cov = C.c_size_t()
        self._chk(self.L.ppp_get_path_coverage(self.h, None, 0, C.byref(n), C.byref(cov)))
        if not flags:
            return None, cov.value
        out = np.zeros(max(n.value, 1), np.uint8)
        self._chk(self.L.ppp_get_path_coverage(self.h, out.ctypes.data_as(C.POINTER(C.c_ubyte)), n.value, C.byref(n), C.byref(cov)))
        return out[:n.value], cov.value

    def path_contacts(self, maps=True):
        """(counts uint32[n], first int32[n], last int32[n], stats dict) of the last pass's final paths: how many contact balls of
        path_coverage hold each cloud point and the first / last slice with one of them (-1: none; ppp_get_path_contacts).
        stats: n, covered, multi_slice (last > first), max_count, total (the sum of the counts), hist (CONTACT_BINS counts, the
        last bin holding the counts >= CONTACT_BINS - 1).  maps=False returns (None, None, None, stats)"""
        st = ContactStats()
        self._chk(self.L.ppp_get_path_contacts(self.h, None, None, None, 0, C.byref(st)))
        n = st.n
        if maps:
            counts = np.zeros(max(n, 1), np.uint32)
            first = np.zeros(max(n, 1), np.int32)
            last = np.zeros(max(n, 1), np.int32)
            ip = C.POINTER(C.c_int)
            self._chk(self.L.ppp_get_path_contacts(self.h, counts.ctypes.data_as(C.POINTER(C.c_uint)), first.ctypes.data_as(ip),
                                                   last.ctypes.data_as(ip), n, C.byref(st)))
            counts, first, last = counts[:n], first[:n], last[:n]
        else:
            counts = first = last = None
        stats = dict(n=st.n, covered=st.covered, multi_slice=st.multi_slice, max_count=st.max_count, total=st.total,
                     hist=np.array(st.hist[:], np.int64))
        return counts, first, last, stats

    def path_removal(self, profile=REMOVAL_HERTZ, maps=True):
        """(removal float64[n], stats dict) of the last pass's final paths: the balls of path_contacts(), each weighted by the
        path length its sample stands for and by the point's place inside it -- REMOVAL_FLAT 1, REMOVAL_PARABOLIC 1 - u,
        REMOVAL_HERTZ sqrt(1 - u) with u = d2 / r2 -- in millimetres of weighted tool travel (ppp_get_path_removal).  stats: n,
        touched, min_removal, max_removal, sum, sum_sq, path_length, hist (CONTACT_BINS counts of removal / max_removal), and
        mean = sum / touched, cv = the standard deviation over the touched points / mean (NaN when nothing is touched).
        maps=False returns (None, stats)"""
        st = RemovalStats()
        self._chk(self.L.ppp_get_path_removal(self.h, int(profile), None, 0, C.byref(st)))
        n = st.n
        removal = None
        if maps:
            removal = np.zeros(max(n, 1), np.float64)
            self._chk(self.L.ppp_get_path_removal(self.h, int(profile), removal.ctypes.data_as(C.POINTER(C.c_double)), n, C.byref(st)))
            removal = removal[:n]
        mean = st.sum / st.touched if st.touched else float("nan")
        cv = float(np.sqrt(max(0.0, st.sum_sq / st.touched - mean * mean))) / mean if st.touched and mean > 0 else float("nan")
        stats = dict(n=st.n, touched=st.touched, min_removal=st.min_removal, max_removal=st.max_removal, sum=st.sum, sum_sq=st.sum_sq,
                     path_length=st.path_length, hist=np.array(st.hist[:], np.int64), mean=mean, cv=cv)
        return removal, stats

    def path_dwell(self, profile=REMOVAL_HERTZ, target=None, iterations=8, dwell_min=0.25, dwell_max=4.0, maps=True):
        """(rows, removal float64[n], stats dict): a dwell factor per sample of the last pass's final paths that steers the
        predicted removal of path_removal(profile) towards target (float64[n] by cloud index; None: uniform, same total), after
        `iterations` rounds of the multiplicative update with the factors kept in [dwell_min, dwell_max] (ppp_get_path_dwell).
        rows: a structured array (slice, x, y, z, r, ds, dwell) in (slice, sample) order; removal: the map the factors predict;
        stats: n, touched, rows, at_min, at_max, iterations, level, residual_before, residual_after, min_dwell, max_dwell,
        path_length, time_factor.  maps=False returns (None, None, stats)"""
        tg = None
        if target is not None:
            tg = np.ascontiguousarray(target, np.float64)
            if tg.shape != (self.n,):
                raise ValueError("target must hold one value per cloud point")
        tp = tg.ctypes.data_as(C.POINTER(C.c_double)) if tg is not None else None
        args = (int(profile), tp, int(iterations), float(dwell_min), float(dwell_max))
        st = DwellStats()
        rows = removal = None
        if not maps:
            self._chk(self.L.ppp_get_path_dwell(self.h, *args, None, 0, None, 0, C.byref(st)))
        else:
            # the sizes first: without a target the result is kept and the second call launches nothing; with one both compute
            self._chk(self.L.ppp_get_path_dwell(self.h, *args, None, 0, None, 0, C.byref(st)))
            nrow, n = st.rows, st.n
            rows = np.zeros(max(nrow, 1), np.dtype(DwellRow))
            removal = np.zeros(max(n, 1), np.float64)
            self._chk(self.L.ppp_get_path_dwell(self.h, *args, rows.ctypes.data_as(C.POINTER(DwellRow)), nrow,
                                                removal.ctypes.data_as(C.POINTER(C.c_double)), n, C.byref(st)))
            rows, removal = rows[:st.rows], removal[:st.n]
        stats = {k: getattr(st, k) for k, _ in DwellStats._fields_}
        return rows, removal, stats

    def path_feed(self, profile=REMOVAL_HERTZ, target=None, iterations=8, dwell_min=0.25, dwell_max=4.0, feed=20.0, feed_max=30.0,
                  accel=100.0, end_feed=0.0, link_feed=100.0, maps=True):
        """(rows, stats dict): a timed feed schedule for the WayPointsList of the last pass (ppp_get_path_feed; needs
        get_path()).  The first five arguments are path_dwell()'s; feed, feed_max, end_feed (< 0: none) and link_feed in mm/s,
        accel in mm/s^2 (inf: no limit).  rows: a structured array (slice, limit, dwell, s, feed, t), one per row of
        waypoints(); stats: W, slices, by_dwell, by_feed_max, by_end, by_accel, min_feed, max_feed, path_length, link_length,
        duration, duration_links, duration_nominal.  maps=False returns (None, stats)"""
        tg = None
        if target is not None:
            tg = np.ascontiguousarray(target, np.float64)
            if tg.shape != (self.n,):
                raise ValueError("target must hold one value per cloud point")
        tp = tg.ctypes.data_as(C.POINTER(C.c_double)) if tg is not None else None
        fp = FeedParams(float(feed), float(feed_max), float(accel), float(end_feed), float(link_feed))
        args = (int(profile), tp, int(iterations), float(dwell_min), float(dwell_max), C.byref(fp))
        st = FeedStats()
        rows = None
        if not maps:
            self._chk(self.L.ppp_get_path_feed(self.h, *args, None, 0, C.byref(st)))
        else:
            # with a target every call computes again: one call sized by the list, which the call cannot outgrow
            W = self.num_waypoints()
            rows = np.zeros(max(W, 1), np.dtype(FeedRow))
            self._chk(self.L.ppp_get_path_feed(self.h, *args, rows.ctypes.data_as(C.POINTER(FeedRow)), W, C.byref(st)))
            rows = rows[:min(W, st.W)]
        stats = {k: getattr(st, k) for k, _ in FeedStats._fields_}
        return rows, stats

    def deviation(self, ref, max_dist=float("inf"), smooth_radius=0.0, allowance=0.0, gain=1.0, maps=True):
        """(deviation float64[n], smoothed float64[n], ref_index int32[n], status uint8[n], target float64[n], stats dict) of this
        engine's cloud, the scan, against the cloud of the engine `ref` (ppp_get_deviation): per scan point the signed distance
        to the reference surface along the normal of its nearest reference point within max_dist mm (positive: on the
        viewpoint's side, material to take off), that distance averaged over the matched scan points within smooth_radius mm
        (0: none), and target = gain * max(smoothed - allowance, 0), which path_dwell() and path_feed() take as it is.  status:
        DEV_MATCHED, DEV_TOO_FAR, DEV_NO_NORMAL, DEV_DROPPED; the maps are NaN (ref_index -1, target 0) where it is not
        DEV_MATCHED.  Needs clouds, not a pass; the two clouds are taken as registered in one frame.  stats: n, matched, too_far,
        no_normal, dropped, proud, below, min_dev, max_dev, mean_dev, rms_dev, max_dist2, target_sum, hist (CONTACT_BINS counts
        over [-span, span]).  maps=False returns five Nones and stats"""
        dp = DeviationParams(float(max_dist), float(smooth_radius), float(allowance), float(gain))
        st = DeviationStats()
        dev = sm = idx = status = target = None
        if not maps:
            self._chk(self.L.ppp_get_deviation(self.h, ref.h, C.byref(dp), None, None, None, None, None, 0, C.byref(st)))
        else:
            # every call computes again: one call sized by the resident cloud (preprocessing may have changed its size)
            nn = C.c_size_t()
            self._chk(self.L.ppp_num_points(self.h, C.byref(nn)))
            n = nn.value
            dev, sm, target = (np.zeros(max(n, 1), np.float64) for _ in range(3))
            idx = np.zeros(max(n, 1), np.int32)
            status = np.zeros(max(n, 1), np.uint8)
            self._chk(self.L.ppp_get_deviation(self.h, ref.h, C.byref(dp), _d(dev), _d(sm), _i(idx), status.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                               _d(target), n, C.byref(st)))
            dev, sm, idx, status, target = dev[:n], sm[:n], idx[:n], status[:n], target[:n]
        return dev, sm, idx, status, target, _deviation_stats(st)

    def deviation_tile(self, ref, halo, max_dist=2.0, smooth_radius=0.0, allowance=0.0, gain=1.0, maps=True):
        """(deviation, smoothed, ref_index, status, target, owned uint8[n], part dict) of the points this engine OWNS -- a
        slice-range engine of the scan, or a whole-cloud one, which owns every indexed point -- against the cloud of the engine
        `ref`, whole or a slice range of the reference (ppp_get_deviation_tile).  The maps go by cloud index; an owned point's
        entries are deviation()'s bits on whole-cloud engines, every other point has DEV_DROPPED, -1, NaN, 0 and owned 0.  halo
        (mm) >= max_dist + smooth_radius, max_dist finite; `ref` must index the owned interval widened by halo and its
        normal_radius, this engine's range_margin must cover smooth_radius.  part: n, owned, evaluated, matched, too_far,
        no_normal, proud, below, min_dev, max_dev, fix_sum, max_dist2, own_lo, own_hi, sum_parts -- what merge_deviation_tiles()
        takes.  maps=False returns six Nones and part"""
        dp = DeviationParams(float(max_dist), float(smooth_radius), float(allowance), float(gain))
        st = DeviationTileStats()
        dev = sm = idx = status = target = owned = None
        ub = C.POINTER(C.c_ubyte)
        if not maps:
            self._chk(self.L.ppp_get_deviation_tile(self.h, ref.h, C.byref(dp), float(halo), None, None, None, None, None, None, 0, C.byref(st)))
        else:
            nn = C.c_size_t()
            self._chk(self.L.ppp_num_points(self.h, C.byref(nn)))
            n = nn.value
            dev, sm, target = (np.zeros(max(n, 1), np.float64) for _ in range(3))
            idx = np.zeros(max(n, 1), np.int32)
            status, owned = (np.zeros(max(n, 1), np.uint8) for _ in range(2))
            self._chk(self.L.ppp_get_deviation_tile(self.h, ref.h, C.byref(dp), float(halo), _d(dev), _d(sm), _i(idx), status.ctypes.data_as(ub),
                                                    _d(target), owned.ctypes.data_as(ub), n, C.byref(st)))
            dev, sm, idx, status, target, owned = dev[:n], sm[:n], idx[:n], status[:n], target[:n], owned[:n]
        return dev, sm, idx, status, target, owned, {k: getattr(st, k) for k, _ in DeviationTileStats._fields_}

    def registration_terms(self, ref, T=None, max_dist=2.0, lock_eps=1e-9):
        """(row, stats) of one evaluation of the point-to-plane terms of this engine's cloud, the scan, moved by T (3 x 4, None:
        the identity), against the cloud of the engine `ref` (ppp_get_registration_terms): row = dict(T, pairs, A int64[21] the
        upper triangle of J^T J, b int64[6], E, locked 63, step2 NaN) in fixed point 2^stats["shift"]; no step is taken"""
        rp = RegistrationParams(float(max_dist), 1, 0.0, float(lock_eps))
        row, st = RegistrationRow(), RegistrationStats()
        t = _t12(T)
        self._chk(self.L.ppp_get_registration_terms(self.h, ref.h, C.byref(rp), None if t is None else _d(t), C.byref(row), C.byref(st)))
        return _registration_row(row), _registration_stats(st)

    def registration_terms_tile(self, ref, T=None, max_dist=2.0, lock_eps=1e-9):
        """(row, part): registration_terms() over the points this engine OWNS -- a slice-range engine of the scan, or a whole-cloud
        one, which owns every indexed point -- against the cloud of the engine `ref`, whole or a slice range of the reference
        (ppp_get_registration_terms_tile).  row as registration_terms() gives it; part = dict(owned, evaluated, own_lo, own_hi, n,
        shift, centre, length), the frame and the shift being the whole clouds': what merge_registration_terms() and
        registration_step() take.  A slice-range `ref` must index max_dist + its normal_radius around every moved query:
        PPPError(ERR_CAPACITY) otherwise"""
        rp = RegistrationParams(float(max_dist), 1, 0.0, float(lock_eps))
        row, part = RegistrationRow(), RegistrationPart()
        t = _t12(T)
        self._chk(self.L.ppp_get_registration_terms_tile(self.h, ref.h, C.byref(rp), None if t is None else _d(t), C.byref(row), C.byref(part)))
        return _registration_row(row), _registration_part(part)

    def register(self, ref, max_dist=2.0, iterations=30, min_step=1e-6, lock_eps=1e-9, T0=None):
        """(T float64[3, 4], rows, stats): point-to-plane ICP of this engine's cloud, the scan, to the cloud of the engine `ref`
        (ppp_register), started at T0 (None: the identity; ICP needs a start within the basin of the answer).  T carries a scan
        point into the reference's frame: transform_cloud(T) applies it.  rows[k] is the evaluation at T_k, k = 0 .. steps (dicts
        as registration_terms gives them; the last has locked 63 and step2 NaN); stats: n, indexed, steps, converged, locked,
        shift, centre, length, T, pairs_before / _after, rms_before / _after.  Neither cloud is changed"""
        rp = RegistrationParams(float(max_dist), int(iterations), float(min_step), float(lock_eps))
        cap = max(int(iterations), 0) + 1
        rows = (RegistrationRow * cap)()
        st = RegistrationStats()
        t = _t12(T0)
        self._chk(self.L.ppp_register(self.h, ref.h, C.byref(rp), None if t is None else _d(t), rows, cap, C.byref(st)))
        stats = _registration_stats(st)
        return stats["T"].copy(), [_registration_row(rows[k]) for k in range(min(cap, st.steps + 1))], stats

    def register_trimmed(self, ref, keep=0.8, max_dist=2.0, iterations=30, min_step=1e-6, lock_eps=1e-9, T0=None, maps=True):
        """(T float64[3, 4], rows, status uint8[n], d2 float32[n], stats): trimmed point-to-plane ICP (ppp_register_trimmed):
        register()'s loop in which only the share `keep` of an evaluation's pairs with the smallest pair distance enters its
        sums, so that what the scan shows and the reference does not (a clamp, a burr, an overhang) does not pull the fit.
        rows[k]: register()'s row over the kept pairs (pairs = kept) with paired, trim_d2 (the largest kept d2; NaN without a
        pair) and trim_bits; status / d2 describe the last evaluation by cloud index: TRIM_KEPT, TRIM_TRIMMED, TRIM_UNPAIRED,
        TRIM_DROPPED and the pair's float d2 (NaN without one); stats as register()'s over the kept pairs.  keep = 1 is
        register() bit for bit.  maps=False returns None for the two maps"""
        tp = TrimmedRegistrationParams(RegistrationParams(float(max_dist), int(iterations), float(min_step), float(lock_eps)), float(keep))
        cap = max(int(iterations), 0) + 1
        rows = (TrimmedRegistrationRow * cap)()
        st = RegistrationStats()
        t = _t12(T0)
        status = d2 = None
        n = 0
        if maps:
            nn = C.c_size_t()
            self._chk(self.L.ppp_num_points(self.h, C.byref(nn)))
            n = nn.value
            status = np.zeros(max(n, 1), np.uint8)
            d2 = np.zeros(max(n, 1), np.float32)
        self._chk(self.L.ppp_register_trimmed(self.h, ref.h, C.byref(tp), None if t is None else _d(t), rows, cap,
                                              None if status is None else status.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                              None if d2 is None else d2.ctypes.data_as(C.POINTER(C.c_float)), n, C.byref(st)))
        stats = _registration_stats(st)
        if maps:
            status, d2 = status[:n], d2[:n]
        return stats["T"].copy(), [_trimmed_registration_row(rows[k]) for k in range(min(cap, st.steps + 1))], status, d2, stats

    def _robust_maps(self, maps):
        """(n, status, weight, residual) to hand to the robust calls: arrays of the cloud's size, or 0 and three Nones"""
        if not maps:
            return 0, None, None, None
        nn = C.c_size_t()
        self._chk(self.L.ppp_num_points(self.h, C.byref(nn)))
        n = nn.value
        return n, np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float64)

    def _robust_terms(self, call, against, T, tune, sigma_min, max_dist, lock_eps, maps):
        """one evaluation by `call` (ppp_get_robust_registration_terms or its mesh form) against the handle `against`"""
        bp = RobustRegistrationParams(RegistrationParams(float(max_dist), 1, 0.0, float(lock_eps)), float(tune), float(sigma_min))
        row, st = RobustRegistrationRow(), RegistrationStats()
        t = _t12(T)
        n, status, weight, residual = self._robust_maps(maps)
        self._chk(call(self.h, against, C.byref(bp), None if t is None else _d(t), C.byref(row),
                       None if status is None else status.ctypes.data_as(C.POINTER(C.c_ubyte)),
                       None if weight is None else weight.ctypes.data_as(C.POINTER(C.c_float)),
                       None if residual is None else _d(residual), n, C.byref(st)))
        if maps:
            status, weight, residual = status[:n], weight[:n], residual[:n]
        return _robust_registration_row(row), status, weight, residual, _registration_stats(st)

    def _robust_loop(self, call, against, tune, sigma_min, max_dist, iterations, min_step, lock_eps, T0, maps):
        """the loop by `call` (ppp_register_robust or its mesh form) against the handle `against`"""
        bp = RobustRegistrationParams(RegistrationParams(float(max_dist), int(iterations), float(min_step), float(lock_eps)), float(tune), float(sigma_min))
        cap = max(int(iterations), 0) + 1
        rows = (RobustRegistrationRow * cap)()
        st = RegistrationStats()
        t = _t12(T0)
        n, status, weight, residual = self._robust_maps(maps)
        self._chk(call(self.h, against, C.byref(bp), None if t is None else _d(t), rows, cap,
                       None if status is None else status.ctypes.data_as(C.POINTER(C.c_ubyte)),
                       None if weight is None else weight.ctypes.data_as(C.POINTER(C.c_float)),
                       None if residual is None else _d(residual), n, C.byref(st)))
        stats = _registration_stats(st)
        if maps:
            status, weight, residual = status[:n], weight[:n], residual[:n]
        return stats["T"].copy(), [_robust_registration_row(rows[k]) for k in range(min(cap, st.steps + 1))], status, weight, residual, stats

    def robust_registration_terms(self, ref, T=None, tune=4.685, sigma_min=1e-4, max_dist=2.0, lock_eps=1e-9, maps=True):
        """(row, status uint8[n], weight float32[n], residual float64[n], stats) of one evaluation of register_robust()'s weighted
        terms at T (3 x 4, None: the identity) against the cloud of the engine `ref` (ppp_get_robust_registration_terms): no step
        is taken; row and the maps as register_robust() gives them.  maps=False returns None for the three maps"""
        return self._robust_terms(self.L.ppp_get_robust_registration_terms, ref.h, T, tune, sigma_min, max_dist, lock_eps, maps)

    def register_robust(self, ref, tune=4.685, sigma_min=1e-4, max_dist=2.0, iterations=30, min_step=1e-6, lock_eps=1e-9, T0=None, maps=True):
        """(T float64[3, 4], rows, status uint8[n], weight float32[n], residual float64[n], stats): robust point-to-plane ICP
        (ppp_register_robust): register()'s loop in which every pair enters the sums with Tukey's biweight of its point-to-plane
        residual r, the scale sigma = max(1.4826 median|r|, sigma_min) taken anew at every evaluation and the weight cut at
        tune * sigma -- no share of the scan has to be chosen, as register_trimmed()'s keep must be.  rows[k]: register()'s row
        with the weighted A / b / E (pairs = the pairs found) and used (pairs with a weight above 0), weight_sum, median_abs,
        median_bits and sigma; the maps describe the last evaluation by cloud index: ROBUST_USED, ROBUST_REJECTED,
        ROBUST_UNPAIRED, ROBUST_DROPPED, the weight and the residual (NaN without a pair); stats as register()'s with the
        weighted rms.  tune = inf is register() bit for bit.  It needs the median residual to lie on the part that shows the
        reference: with a third of the scan off it does not recover the motion (register_trimmed with a known keep does).
        maps=False returns None for the three maps"""
        return self._robust_loop(self.L.ppp_register_robust, ref.h, tune, sigma_min, max_dist, iterations, min_step, lock_eps, T0, maps)

    def mesh_robust_registration_terms(self, mesh, T=None, tune=4.685, sigma_min=1e-4, max_dist=2.0, lock_eps=1e-9, maps=True):
        """robust_registration_terms() against the triangles of the TriMesh `mesh` (ppp_get_mesh_robust_registration_terms): one
        evaluation of register_mesh_robust()'s weighted terms at T, no step; the same five results"""
        m = mesh.m if mesh is not None else None
        return self._robust_terms(self.L.ppp_get_mesh_robust_registration_terms, m, T, tune, sigma_min, max_dist, lock_eps, maps)

    def register_mesh_robust(self, mesh, tune=4.685, sigma_min=1e-4, max_dist=2.0, iterations=30, min_step=1e-6, lock_eps=1e-9, T0=None, maps=True):
        """(T, rows, status, weight, residual, stats) as register_robust() gives them, against the triangles of the TriMesh `mesh`
        themselves (ppp_register_mesh_robust): register_mesh()'s pairs -- the moved point in double, the exact closest point of its
        nearest triangle, that facet's own normal -- under register_robust()'s weights, for a scan that shows a clamp or a strip of
        the table within max_dist of the part.  tune = inf is register_mesh() bit for bit.  A mesh of either orientation gives the
        same rows; the residual map is signed by the facets' winding.  Neither the cloud nor the mesh is changed"""
        m = mesh.m if mesh is not None else None
        return self._robust_loop(self.L.ppp_register_mesh_robust, m, tune, sigma_min, max_dist, iterations, min_step, lock_eps, T0, maps)

    def _mesh_trimmed(self, call, loop, mesh, T, keep, border, max_dist, iterations, min_step, lock_eps, maps):
        """the evaluation (loop False) or the loop by `call` against the TriMesh `mesh`"""
        mp = MeshTrimmedRegistrationParams(TrimmedRegistrationParams(RegistrationParams(float(max_dist), int(iterations), float(min_step), float(lock_eps)),
                                                                     float(keep)), int(border))
        cap = max(int(iterations), 0) + 1 if loop else 1
        rows = (MeshTrimmedRegistrationRow * cap)()
        st = RegistrationStats()
        t = _t12(T)
        status = d2 = None
        n = 0
        if maps:
            nn = C.c_size_t()
            self._chk(self.L.ppp_num_points(self.h, C.byref(nn)))
            n = nn.value
            status = np.zeros(max(n, 1), np.uint8)
            d2 = np.zeros(max(n, 1), np.float32)
        args = [self.h, mesh.m if mesh is not None else None, C.byref(mp), None if t is None else _d(t), rows] + ([cap] if loop else [])
        self._chk(call(*args, None if status is None else status.ctypes.data_as(C.POINTER(C.c_ubyte)),
                       None if d2 is None else d2.ctypes.data_as(C.POINTER(C.c_float)), n, C.byref(st)))
        if maps:
            status, d2 = status[:n], d2[:n]
        return [_mesh_trimmed_registration_row(rows[k]) for k in range(min(cap, st.steps + 1))], status, d2, _registration_stats(st)

    def mesh_trimmed_registration_terms(self, mesh, T=None, keep=0.8, border=MESH_BORDER_PAIR, max_dist=2.0, lock_eps=1e-9, maps=True):
        """(row, status uint8[n], d2 float32[n], stats) of one evaluation of register_mesh_trimmed()'s terms at T (3 x 4, None: the
        identity) against the triangles of the TriMesh `mesh` (ppp_get_mesh_trimmed_registration_terms): no step is taken; row
        and the maps as register_mesh_trimmed() gives them.  maps=False returns None for the two maps"""
        rows, status, d2, stats = self._mesh_trimmed(self.L.ppp_get_mesh_trimmed_registration_terms, False, mesh, T, keep, border, max_dist, 1, 0.0,
                                                     lock_eps, maps)
        return rows[0], status, d2, stats

    def register_mesh_trimmed(self, mesh, keep=0.8, border=MESH_BORDER_PAIR, max_dist=2.0, iterations=30, min_step=1e-6, lock_eps=1e-9, T0=None,
                              maps=True):
        """(T float64[3, 4], rows, status uint8[n], d2 float32[n], stats): trimmed point-to-plane ICP against the triangles of the
        TriMesh `mesh` themselves (ppp_register_mesh_trimmed): register_mesh()'s candidates -- the moved point in double, the exact
        closest point of its nearest triangle, that facet's own normal -- of which only the share `keep` with the smallest
        distance enters an evaluation's sums: the tool for a scan more contaminated than register_mesh_robust()'s median bears.
        border = MESH_BORDER_REJECT drops, before the cut, every candidate whose closest point lies on a border edge or a border
        vertex of the mesh's welded topology (built where it is missing): the scan's overhang beyond an open mesh.  rows[k]:
        register_trimmed()'s row (pairs = kept, paired, trim_d2, trim_bits) with on_border; status / d2 describe the last
        evaluation by cloud index: TRIM_KEPT, TRIM_TRIMMED, TRIM_UNPAIRED, TRIM_DROPPED, MESH_TRIM_BORDER and the key's float
        (NaN without a pair).  keep = 1 with MESH_BORDER_PAIR is register_mesh() bit for bit.  maps=False returns None for the
        two maps.  The cloud is not changed"""
        rows, status, d2, stats = self._mesh_trimmed(self.L.ppp_register_mesh_trimmed, True, mesh, T0, keep, border, max_dist, iterations, min_step,
                                                     lock_eps, maps)
        return stats["T"].copy(), rows, status, d2, stats

    register_trimmed_tiles = staticmethod(register_trimmed_tiles)   # Engine.register_trimmed_tiles(engines, refs, ...): the module's function
    register_robust_tiles = staticmethod(register_robust_tiles)     # Engine.register_robust_tiles(engines, refs, ...) likewise

    def cloud_moments(self):
        """ppp_get_cloud_moments: the frame dict of the resident cloud (count, ms, c, L, the ten integer words, mean, axes with
        column k the k-th principal axis, eigenvalues in mm^2, descending)"""
        f = CloudFrame()
        self._chk(self.L.ppp_get_cloud_moments(self.h, C.byref(f)))
        return _cloud_frame(f)

    def register_global(self, ref, candidates=24, stride=16, coarse=None, fine=None):
        """(T float64[3, 4], cands, rows, stats): ppp_register_global of this engine's cloud, the scan, to the cloud of the engine
        `ref`, from the two clouds alone: the starts their principal frames imply, a coarse chain from each side by side on every
        stride-th point, the fine chain from the cheapest.  coarse / fine: dicts of register()'s parameters over the defaults
        (10, 8, 1e-3, 1e-9) and (2, 30, 1e-6, 1e-9).  cands: one dict per start (index, T0, T, steps, converged, locked, pairs0,
        pairs, E0, E, cost); rows: the fine chain's; stats: fine (register()'s stats), scan / ref (frame dicts), queries, shift,
        candidates, winner, winner_cost, second_cost"""
        return self._register_global(self.L.ppp_register_global, ref.h, candidates, stride, coarse, fine)

    def register_mesh_global(self, mesh, candidates=24, stride=16, coarse=None, fine=None):
        """(T, cands, rows, stats) as register_global() gives them: ppp_register_mesh_global of this engine's cloud, the scan, to
        the triangles of the TriMesh `mesh` themselves, from the scan and the mesh alone: stats["ref"] is the mesh's area frame
        (TriMesh.moments()), every coarse chain is register_mesh() with `coarse` on every stride-th point, the fine chain is
        register_mesh() with `fine` from the cheapest start's end"""
        m = getattr(mesh, "m", mesh)
        return self._register_global(self.L.ppp_register_mesh_global, m, candidates, stride, coarse, fine)

    def _register_global(self, call, against, candidates, stride, coarse, fine):
        gp = GlobalRegistrationParams()
        self.L.ppp_default_global_registration_params(C.byref(gp))
        gp.candidates, gp.stride = int(candidates), int(stride)
        for part, kw in ((gp.coarse, coarse), (gp.fine, fine)):
            for k, v in (kw or {}).items():
                if k not in ("max_dist", "iterations", "min_step", "lock_eps"):
                    raise TypeError("unknown registration parameter %r" % k)
                setattr(part, k, int(v) if k == "iterations" else float(v))
        ncand = max(gp.candidates, 1)
        cap = max(gp.fine.iterations, 0) + 1
        cands = (RegistrationCandidate * ncand)()
        rows = (RegistrationRow * cap)()
        st = GlobalRegistrationStats()
        self._chk(call(self.h, against, C.byref(gp), cands, ncand, rows, cap, C.byref(st)))
        stats = dict(fine=_registration_stats(st.fine), scan=_cloud_frame(st.scan), ref=_cloud_frame(st.ref), queries=int(st.queries),
                     shift=int(st.shift), candidates=int(st.candidates), winner=int(st.winner), winner_cost=int(st.winner_cost),
                     second_cost=int(st.second_cost))
        return (stats["fine"]["T"].copy(), [_registration_candidate(cands[k]) for k in range(min(ncand, st.candidates))],
                [_registration_row(rows[k]) for k in range(min(cap, st.fine.steps + 1))], stats)

    def transform_cloud(self, T):
        """ppp_transform_cloud: the resident cloud moved by T (3 x 4 in double, rounded to float; pcl::transformPointCloud's
        arithmetic).  Plan, index and stored results are withdrawn, as after any change of the cloud"""
        t = _t12(T)
        self._chk(self.L.ppp_transform_cloud(self.h, None if t is None else _d(t)))

    def contact_field(self, maps=True, min_width=0.0):
        """(curv5 float32[n, 5], half_width float32[n], stats dict) of the resident cloud: compute_transform + Area2Cloud at every
        cloud point (ppp_get_contact_field) -- pcx pcy pcz pc1 pc2 and the half width r of the contact ellipse, NaN where the
        model gives none.  Needs no pass.  stats: n, valid, narrow (valid points with 2|r| < min_width), min_abs_r, max_abs_r,
        sum_abs_r, mean_abs_r, hist (CONTACT_BINS counts of |r| / tool_radius).  maps=False returns (None, None, stats)"""
        st = ContactFieldStats()
        self._chk(self.L.ppp_get_contact_field(self.h, None, None, 0, float(min_width), C.byref(st)))
        n = st.n
        if maps:
            curv = np.empty((max(n, 1), 5), np.float32)
            hw = np.empty(max(n, 1), np.float32)
            self._chk(self.L.ppp_get_contact_field(self.h, _f(curv), _f(hw), n, float(min_width), C.byref(st)))
            curv, hw = curv[:n], hw[:n]
        else:
            curv = hw = None
        stats = dict(n=st.n, valid=st.valid, narrow=st.narrow, min_abs_r=st.min_abs_r, max_abs_r=st.max_abs_r, sum_abs_r=st.sum_abs_r,
                     mean_abs_r=(st.sum_abs_r / st.valid if st.valid else float("nan")), hist=np.array(st.hist[:], np.int64))
        return curv, hw, stats

    def contact_field_tile(self, maps=True, halo=0.0, min_width=0.0):
        """(curv5 float32[n, 5], half_width float32[n], owned uint8[n], stats dict): contact_field() for the points this handle's
        slice range owns and a halo of `halo` mm around them (ppp_get_contact_field_tile).  owned: 1 = owned, 2 = evaluated
        halo point, 0 = not evaluated (NaN rows).  stats cover the owned points: contact_field()'s, then owned, evaluated,
        own_lo, own_hi.  maps=False returns (None, None, None, stats)"""
        st = ContactFieldTileStats()
        args = (float(halo), float(min_width), C.byref(st))
        self._chk(self.L.ppp_get_contact_field_tile(self.h, None, None, None, 0, *args))
        n = st.n
        if maps:
            curv = np.empty((max(n, 1), 5), np.float32)
            hw = np.empty(max(n, 1), np.float32)
            own = np.empty(max(n, 1), np.uint8)
            self._chk(self.L.ppp_get_contact_field_tile(self.h, _f(curv), _f(hw), own.ctypes.data_as(C.POINTER(C.c_ubyte)), n, *args))
            curv, hw, own = curv[:n], hw[:n], own[:n]
        else:
            curv = hw = own = None
        stats = dict(n=st.n, valid=st.valid, narrow=st.narrow, min_abs_r=st.min_abs_r, max_abs_r=st.max_abs_r, sum_abs_r=st.sum_abs_r,
                     hist=np.array(st.hist[:], np.int64), owned=st.owned, evaluated=st.evaluated, own_lo=st.own_lo, own_hi=st.own_hi)
        return curv, hw, own, stats

    def regions_tile(self, source=REGIONS_MASK, mask=None, threshold=0.0, link_radius=0.0):
        """(labels int32[n], parts, halos, stats dict): the regions of this handle's tile (ppp_get_regions_tile), what
        merge_region_tiles() takes.  source: REGIONS_MASK (mask: one byte per point of the WHOLE cloud) or REGIONS_NARROW.
        labels = the tile-local label of an owned selected point, -1 otherwise; parts (REGION_PART_DTYPE) = the tile components
        with an owned point; halos (REGION_HALO_DTYPE) = their selected halo points; stats: n, selected, parts, halo_points,
        max_abs_coord, own_lo, own_hi"""
        st = RegionTileStats()
        mp = None
        if mask is not None:
            mask = np.ascontiguousarray(mask, np.uint8)
            if mask.ndim != 1 or mask.size != getattr(self, "n", mask.size):
                raise ValueError("mask must hold one byte per cloud point")
            mp = mask.ctypes.data_as(C.POINTER(C.c_ubyte))
        args = (int(source), mp, float(threshold), float(link_radius))
        self._chk(self.L.ppp_get_regions_tile(self.h, *args, None, 0, None, 0, None, 0, C.byref(st)))      # the sizes
        lab = np.empty(max(st.n, 1), np.int32)
        parts = np.zeros(max(st.parts, 1), REGION_PART_DTYPE)
        halos = np.zeros(max(st.halo_points, 1), REGION_HALO_DTYPE)
        # (answered from the result the first call left; a mask's is computed again)
        self._chk(self.L.ppp_get_regions_tile(self.h, *args, _i(lab), st.n, parts.ctypes.data_as(C.POINTER(RegionPart)), st.parts,
                                              halos.ctypes.data_as(C.POINTER(RegionHalo)), st.halo_points, C.byref(st)))
        stats = {f: getattr(st, f) for f in _TILE_STATS}
        return lab[:st.n], parts[:st.parts], halos[:st.halo_points], stats

    def regions(self, source=REGIONS_UNCOVERED, mask=None, threshold=0.0, link_radius=0.0, labels=True):
        """(labels int32[n] | None, regions, stats dict): the connected regions of the points `source` selects, two selected
        points being linked when they are within link_radius (<= 0: the handle's normal_radius) of each other (ppp_get_regions).
        source: REGIONS_UNCOVERED (points path_coverage() does not flag), REGIONS_OVERLAP (last > first in path_contacts()),
        REGIONS_NARROW (valid points of contact_field() with 2|r| < threshold) or REGIONS_MASK (mask: n bytes, non-zero =
        selected).  labels[i] = the label of point i's region (its smallest cloud index), -1 where i is not selected; regions =
        a structured array (REGION_DTYPE: label, count, mn, mx, centroid) in ascending label; stats: n, selected, regions,
        singletons, largest.  labels=False returns None for the labels"""
        st = RegionStats()
        mp = None
        if mask is not None:
            mask = np.ascontiguousarray(mask, np.uint8)
            if mask.ndim != 1 or mask.size != getattr(self, "n", mask.size):
                raise ValueError("mask must hold one byte per cloud point")
            mp = mask.ctypes.data_as(C.POINTER(C.c_ubyte))
        args = (int(source), mp, float(threshold), float(link_radius))
        self._chk(self.L.ppp_get_regions(self.h, *args, None, 0, None, 0, C.byref(st)))      # the sizes
        lab = np.empty(max(st.n, 1), np.int32) if labels else None
        rows = np.zeros(max(st.regions, 1), REGION_DTYPE)
        if labels or st.regions:  # (answered from the result the first call left; a mask's is computed again)
            self._chk(self.L.ppp_get_regions(self.h, *args, None if lab is None else _i(lab), st.n if labels else 0,
                                             rows.ctypes.data_as(C.POINTER(Region)), st.regions, C.byref(st)))
        stats = dict(n=st.n, selected=st.selected, regions=st.regions, singletons=st.singletons, largest=st.largest)
        return (lab[:st.n] if labels else None), rows[:st.regions], stats

    def principal_curvatures_at(self, q):
        """compute_transform's principal curvatures for query points [k, 3] (float32, mm): [k, 5] = pcx pcy pcz pc1 pc2."""
        q = np.ascontiguousarray(q, np.float32).reshape(-1, 3)
        out = np.empty((len(q), 5), np.float32)
        self._chk(self.L.ppp_principal_curvatures_at(self.h, _f(q), len(q), _f(out)))
        return out

    def eval_spline(self, s, y):
        y = np.ascontiguousarray(y, np.float64)
        out = np.empty((len(y), 3))
        rc = self.L.ppp_eval_spline(self.h, int(s), _d(y), len(y), _d(out))
        if rc and rc != ERR_DOMAIN:
            self._chk(rc)
        return rc, out

    def insert_point(self, indices, plane_x):
        indices = np.ascontiguousarray(indices, np.int32)
        cap = max(len(indices), 1)
        y = np.empty(cap); x = np.empty(cap); z = np.empty(cap)
        m = C.c_size_t()
        rc = self.L.ppp_insert_point(self.h, _i(indices), len(indices), float(plane_x), _d(y), _d(x), _d(z), cap, C.byref(m))
        if rc == ERR_SLICE:
            return rc, None, None, None
        self._chk(rc)
        return m.value, y[:m.value], x[:m.value], z[:m.value]

    def normals_at(self, idx):
        idx = np.ascontiguousarray(idx, np.int32)
        out = np.empty((len(idx), 4), np.float32)
        self._chk(self.L.ppp_normals_at(self.h, _i(idx), len(idx), _f(out)))
        return out

    def estimate_normals(self):
        """estimate_normal() over the whole cloud: [n, 4] = nx ny nz curvature."""
        out = np.empty((self.n, 4), np.float32)
        self._chk(self.L.ppp_estimate_normals(self.h, _f(out)))
        return out

    def area2cloud(self, pts, key):
        """Area2Cloud of the dynamic adjustment for points [k, 3] (float64, mm)."""
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        out = np.empty((len(pts), 3), np.float32)
        self._chk(self.L.ppp_area2cloud(self.h, _d(pts), len(pts), int(key), _f(out)))
        return out

    def nearest(self, q):
        q = np.ascontiguousarray(q, np.float32).reshape(-1, 3)
        out = np.empty(len(q), np.int32)
        self._chk(self.L.ppp_nearest(self.h, _f(q), len(q), _i(out)))
        return out

    def stage(self, stage):
        cnt = C.c_size_t()
        self._chk(self.L.ppp_get_stage(self.h, stage, None, 0, C.byref(cnt)))
        W = cnt.value
        shape, dt = {STAGE_WP_XYZ: ((W, 3), np.float32), STAGE_WP_NN: ((W,), np.int32),
                     STAGE_WP_NORMAL: ((W, 4), np.float32), STAGE_WP_PRESMOOTH: ((W, 6), np.float32),
                     STAGE_WP_SMOOTHED: ((W, 6), np.float32)}[stage]
        out = np.empty(shape, dt)
        if W:
            self._chk(self.L.ppp_get_stage(self.h, stage, out.ctypes.data, out.nbytes, C.byref(cnt)))
        return out

    def smooth_sweeps(self):
        s = C.c_int()
        self._chk(self.L.ppp_smooth_sweeps(self.h, C.byref(s)))
        return s.value

    # -- measurement --
    def enable_timing(self, on=True):
        self._chk(self.L.ppp_enable_timing(self.h, 1 if on else 0))

    def kernel_times(self, with_launches=False):
        """{kernel: ms summed over its launches since the last call} (and {kernel: launches})."""
        cap = 64
        names = C.create_string_buffer(48 * cap)
        ms = np.zeros(cap, np.float32)
        cnt = np.zeros(cap, np.int32)
        n = C.c_size_t()
        self._chk(self.L.ppp_get_kernel_times(self.h, names, _f(ms), _i(cnt), cap, C.byref(n)))
        out, launches = {}, {}
        for k in range(n.value):
            nm = names.raw[48 * k:48 * k + 48].split(b"\0", 1)[0].decode()
            out[nm] = float(ms[k])
            launches[nm] = int(cnt[k])
        return (out, launches) if with_launches else out
