"""Loader of the HIP C-ABI library (putslam_amd/libputslam_hip.so).

The library is the product: there is no Python or CPU fallback.  If the shared
object is missing the import fails loudly and tells the caller how to build it.
"""
import ctypes as C
import os

from ._abi import (PsDMatch, PsExclusionRule, PsFrameSet, PsFrameSetF32, PsHostPairResults, PsLoopBatch, PsLoopBatchF32, PsLoopResults, PsMapBatch,
                   PsMapBatchF32, PsMapStore, PsMapStoreF32, PsMapViewOut, PsMapViewOutF32, PsMapViewRequest, PsPairResults, PsPoseSetOut,
                   PsPoseSetOutF32, PsPoseSetRequest, PsRansacConfig, PsRansacParams, PsRansacStats, PsImageSet, PsKltParams, PsDetectParams, PsOrbParams, PsOrbDetectParams,
                   PsDepthSet, PsFrameGeometry, PsFrameRowsOut, PsFrontEndParams, PsPointSets, PsTrackedCarry, PsTrackedRows, PsTrackVoParams,
                   PsTrackVoIn, PsTrackVoOut, PsTrackCandidates, PsTrackCloseParams, PsTrackCloseOut, PsSensorModel, PsUncertaintyOut,
                   PsMeasurementEdgesOut, PsPatchParams, PsPatchModel)

# Hardware queues: the library's launch chains (batch queue, pipelined stream) want one each, the HIP runtime reads
# GPU_MAX_HW_QUEUES once, at its first call.  The library sets its default (16) from a constructor when it is loaded -- too late
# in a Python process whose torch has already initialised HIP, so the default is also set here, at import (csrc/ps_env.cpp).
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

_HERE = os.path.dirname(os.path.abspath(__file__))
# PUTSLAM_HIP_LIB: A/B hook of the profiling scripts (another build of the same library, e.g. a kernel variant)
LIB_PATH = os.environ.get("PUTSLAM_HIP_LIB") or os.path.join(_HERE, "libputslam_hip.so")

# every symbol include/putslam_hip.h declares
EXPORTED = [
    "ps_context_create", "ps_context_destroy", "ps_context_set_stream", "ps_context_synchronize",
    "ps_context_stream", "ps_context_device",
    "ps_context_set_option", "ps_context_get_option",
    "ps_last_error", "ps_abi_version", "ps_device_arch",
    "ps_match_hamming256", "ps_ransac_rigid3d", "ps_umeyama_f32", "ps_kabsch_f64",
    "ps_keypoints2Dto3D", "ps_depth_view_bytes", "ps_points3Dto2D", "ps_vo_pairs_device", "ps_dbscan_thin", "ps_dbscan_thin_device", "ps_debug_dbscan_bound",
    "ps_batch_queue_create", "ps_batch_queue_destroy", "ps_batch_queue_submit", "ps_batch_queue_wait", "ps_batch_queue_query",
    "ps_batch_queue_wait_on_stream", "ps_batch_queue_synchronize", "ps_batch_queue_chains", "ps_batch_queue_context",
    "ps_batch_queue_last_split", "ps_pack_records_device", "ps_match_xyz", "ps_predicted_level", "ps_remove_image_distortion",
    "ps_vo_stream_create", "ps_vo_stream_destroy", "ps_vo_stream_reset", "ps_vo_stream_push",
    "ps_vo_stream_set_result_mode", "ps_vo_stream_set_frame_layout", "ps_vo_stream_packed_stride", "ps_vo_stream_push_many_packed", "ps_vo_stream_configure_async", "ps_vo_stream_push_async", "ps_vo_stream_push_many", "ps_vo_stream_flush",
    "ps_vo_stream_pop_many", "ps_vo_stream_pop", "ps_vo_stream_pending", "ps_vo_stream_graph_launches", "ps_host_alloc", "ps_host_free",
    "ps_algorithmic_bytes", "ps_kernel_names", "ps_last_kernel_times_ms", "ps_kernel_time_totals",
    "ps_context_enable_timing",
    "ps_debug_ransac_counts", "ps_debug_limits", "ps_debug_keys_clean", "ps_debug_fastdiv", "ps_debug_mathcheck", "ps_debug_score_stats", "ps_debug_score_stats_ex", "ps_debug_stage_survivors", "ps_debug_stage_order", "ps_debug_stamps",
    "ps_abi_sizeof_dmatch", "ps_abi_sizeof_params", "ps_abi_sizeof_config", "ps_abi_sizeof_stats",
    "ps_abi_sizeof_frameset", "ps_abi_sizeof_results", "ps_abi_sizeof_host_results",
    "ps_map_sphere_bound", "ps_match_xyz_device", "ps_map_pairs_device", "ps_abi_sizeof_map_batch",
    "ps_abi_sizeof_exclusion_rule", "ps_sqrt_bound_f64", "ps_exclusion_rule_new_map_features", "ps_exclusion_rule_merge_tracked",
    "ps_exclusion_rule_too_close", "ps_exclude", "ps_exclude_device",
    "ps_level_thresholds", "ps_view_angles", "ps_map_views_device", "ps_frame_levels_device",
    "ps_abi_sizeof_map_store", "ps_abi_sizeof_map_view_request", "ps_abi_sizeof_map_view_out",
    "ps_pose_sets_device", "ps_loop_pairs_device",
    "ps_abi_sizeof_pose_set_request", "ps_abi_sizeof_pose_set_out", "ps_abi_sizeof_loop_batch", "ps_abi_sizeof_loop_results",    "ps_match_l2_f32", "ps_match_l2_device", "ps_vo_pairs_l2_device", "ps_abi_sizeof_frameset_f32", "ps_debug_l2_band",
    "ps_debug_l2_stats", "ps_match_xyz_l2_f32", "ps_match_xyz_l2_device", "ps_map_pairs_l2_device", "ps_abi_sizeof_map_batch_f32",
    "ps_map_views_l2_device", "ps_pose_sets_l2_device", "ps_loop_pairs_l2_device",
    "ps_abi_sizeof_map_store_f32", "ps_abi_sizeof_map_view_out_f32", "ps_abi_sizeof_pose_set_out_f32", "ps_abi_sizeof_loop_batch_f32",
    "ps_klt_pyramids_create", "ps_klt_pyramids_destroy", "ps_klt_pyramids_num_levels", "ps_klt_pyramids_build_device",
    "ps_klt_track_device", "ps_klt_select_device", "ps_calc_optical_flow_pyr_lk", "ps_perform_tracking", "ps_debug_klt_level",
    "ps_abi_sizeof_klt_params", "ps_abi_sizeof_image_set",
    "ps_fast_detector_create", "ps_fast_detector_destroy", "ps_detect_features_device", "ps_detect_features", "ps_debug_fast_maps", "ps_debug_fast_passes",
    "ps_abi_sizeof_detect_params",
    "ps_orb_pattern_default", "ps_orb_pyramids_create", "ps_orb_pyramids_destroy", "ps_orb_pyramids_level", "ps_orb_pyramids_build_device",
    "ps_describe_features_device", "ps_describe_features", "ps_debug_orb_level", "ps_debug_orb_passes", "ps_abi_sizeof_orb_params",
    "ps_orb_detector_create", "ps_orb_detector_destroy", "ps_orb_detector_level", "ps_orb_detect_quotas", "ps_orb_detect_frames",
    "ps_detect_features_orb", "ps_debug_orb_detect_level", "ps_debug_orb_detect_passes", "ps_abi_sizeof_orb_detect_params",
    "ps_gather_keypoints", "ps_assemble_frames", "ps_front_end_create", "ps_front_end_destroy", "ps_front_end_frames", "ps_front_end_frame",
    "ps_abi_sizeof_depth_set", "ps_abi_sizeof_frame_geometry", "ps_abi_sizeof_frame_rows_out", "ps_abi_sizeof_front_end_params",
    "ps_ransac_match_lists", "ps_assemble_tracked", "ps_track_vo_pairs", "ps_track_vo_pair",
    "ps_abi_sizeof_point_sets", "ps_abi_sizeof_tracked_carry", "ps_abi_sizeof_tracked_rows", "ps_abi_sizeof_track_vo_params",
    "ps_abi_sizeof_track_vo_in", "ps_abi_sizeof_track_vo_out",
    "ps_track_candidates", "ps_track_close_create", "ps_track_close_destroy", "ps_track_close_pairs",
    "ps_track_close_pair", "ps_debug_track_close_passes",
    "ps_abi_sizeof_track_candidates", "ps_abi_sizeof_track_close_params", "ps_abi_sizeof_track_close_out",
    "ps_sensor_model_default", "ps_debug_gradient_tie_table", "ps_feature_uncertainty", "ps_measurement_edges", "ps_compute_normals",
    "ps_compute_rgb_gradients", "ps_information_matrices",
    "ps_abi_sizeof_sensor_model", "ps_abi_sizeof_uncertainty_out", "ps_abi_sizeof_measurement_edges_out",
    "ps_patch_models", "ps_patch_align", "ps_compute_patch", "ps_compute_patch_gradient", "ps_optimize_location", "ps_optimize_locations",
    "ps_abi_sizeof_patch_params", "ps_abi_sizeof_patch_model",
]

# ps_abi_sizeof_<name>: the ctypes mirror (_abi.py) of every struct that crosses the C ABI
ABI_STRUCTS = dict(dmatch=PsDMatch, params=PsRansacParams, config=PsRansacConfig, stats=PsRansacStats, frameset=PsFrameSet,
                   results=PsPairResults, host_results=PsHostPairResults, map_batch=PsMapBatch, exclusion_rule=PsExclusionRule,
                   map_store=PsMapStore, map_view_request=PsMapViewRequest, map_view_out=PsMapViewOut,
                   pose_set_request=PsPoseSetRequest, pose_set_out=PsPoseSetOut, loop_batch=PsLoopBatch, loop_results=PsLoopResults)
# ... and of the float-descriptor matcher's frame set (a table of its own: ABI_STRUCTS is the ABI-2 set the layout tests count)
ABI_STRUCTS_F32 = dict(frameset_f32=PsFrameSetF32)
# ... and of the resident store with float rows (ps_map_views_l2_device / ps_pose_sets_l2_device / ps_loop_pairs_l2_device)
ABI_STRUCTS_STORE_F32 = dict(map_store_f32=PsMapStoreF32, map_view_out_f32=PsMapViewOutF32, pose_set_out_f32=PsPoseSetOutF32,
                             loop_batch_f32=PsLoopBatchF32)
# ... and of the Lucas-Kanade tracker (ps_klt_* / ps_perform_tracking)
ABI_STRUCTS_KLT = dict(klt_params=PsKltParams, image_set=PsImageSet)
# ... and of the FAST detector (ps_fast_detector_* / ps_detect_features)
ABI_STRUCTS_DETECT = dict(detect_params=PsDetectParams)
ABI_STRUCTS_ORB = dict(orb_params=PsOrbParams)
ABI_STRUCTS_ORB_DETECT = dict(orb_detect_params=PsOrbDetectParams)
# ... and of frame assembly and the front end (ps_gather_keypoints / ps_assemble_frames / ps_front_end_*)
ABI_STRUCTS_FRAME_ASSEMBLY = dict(depth_set=PsDepthSet, frame_geometry=PsFrameGeometry, frame_rows_out=PsFrameRowsOut,
                                  front_end_params=PsFrontEndParams)
# ... and of the tracking VO step (ps_ransac_match_lists / ps_assemble_tracked / ps_track_vo_pairs)
ABI_STRUCTS_TRACK_VO = dict(point_sets=PsPointSets, tracked_carry=PsTrackedCarry, tracked_rows=PsTrackedRows,
                            track_vo_params=PsTrackVoParams, track_vo_in=PsTrackVoIn, track_vo_out=PsTrackVoOut)
# ... and of its second half (ps_track_candidates / ps_track_close_pairs)
ABI_STRUCTS_TRACK_CLOSE = dict(track_candidates=PsTrackCandidates, track_close_params=PsTrackCloseParams, track_close_out=PsTrackCloseOut)
# ... and of the measurement uncertainty (ps_feature_uncertainty / ps_measurement_edges)
ABI_STRUCTS_UNCERTAINTY = dict(sensor_model=PsSensorModel, uncertainty_out=PsUncertaintyOut, measurement_edges_out=PsMeasurementEdgesOut)
# ... and of the matching on patches (ps_patch_models / ps_patch_align)
ABI_STRUCTS_PATCHES = dict(patch_params=PsPatchParams, patch_model=PsPatchModel)

_lib = None
_by_path = {}


class HipLibraryMissing(RuntimeError):
    pass


def _try_build():
    """The .so is a build artefact (git-ignored): if it is absent but hipcc is here, compile it in-tree (_build.py)."""
    from . import _build
    if not (os.path.exists(_build.HIPCC) and os.path.exists(os.path.join(_build.CSRC, _build.DEVICE_TU))):
        return
    import subprocess
    try:
        _build.build_hip()
    except (OSError, subprocess.CalledProcessError):
        pass


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        _try_build()
    if not os.path.exists(LIB_PATH):
        raise HipLibraryMissing(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    _lib = load_path(LIB_PATH)
    return _lib


def load_path(path):
    """Binds ONE build of the library (profiling hook: several builds side by side in one process for A/B timing on the
    same box, clock state and data -- profiles/scripts/ab_libs.py; entry points a build lacks are left unbound)."""
    path = os.path.abspath(path)
    if path in _by_path:
        return _by_path[path]
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7.  Loading it first lets
    # the dynamic linker satisfy our DT_NEEDED libamdhip64.so.7 with the copy torch uses, so torch tensors,
    # torch streams and our kernels share one runtime (two runtimes in one process cannot both see the GPU).
    # Consumers that do not use torch (the C++ drop-in) link /opt/rocm's runtime as usual.
    if os.environ.get("PUTSLAM_HIP_NO_TORCH", "0") != "1":
        try:
            import torch  # noqa: F401
        except Exception:  # torch absent: stand-alone use
            pass
    real = C.CDLL(path)

    class _Tolerant:
        """argtypes / restype assignments on symbols an older build does not export are dropped."""
        class _Missing:
            pass

        def __getattr__(self, name):
            try:
                return getattr(real, name)
            except AttributeError:
                if path == os.path.abspath(os.path.join(_HERE, "libputslam_hip.so")):   # the product itself: every symbol must be there
                    raise
                return _Tolerant._Missing()

    L = _Tolerant()
    vp, i32, sz = C.c_void_p, C.c_int, C.c_size_t
    L.ps_context_create.argtypes = [i32, C.POINTER(vp)]
    L.ps_context_destroy.argtypes = [vp]
    L.ps_context_destroy.restype = None
    L.ps_context_set_stream.argtypes = [vp, vp]
    L.ps_context_synchronize.argtypes = [vp]
    L.ps_context_stream.argtypes = [vp]
    L.ps_context_stream.restype = vp
    L.ps_context_device.argtypes = [vp]
    L.ps_context_set_option.argtypes = [vp, C.c_char_p, i32]
    L.ps_context_get_option.argtypes = [vp, C.c_char_p]
    L.ps_debug_score_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.ps_debug_score_stats_ex.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.ps_debug_stage_survivors.argtypes = [vp, i32, vp]
    L.ps_debug_stage_order.argtypes = [vp, i32, i32, vp, vp]
    L.ps_debug_stamps.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.ps_last_error.argtypes = [vp]
    L.ps_last_error.restype = C.c_char_p
    L.ps_device_arch.argtypes = [vp]
    L.ps_device_arch.restype = C.c_char_p
    L.ps_match_hamming256.argtypes = [vp, vp, i32, sz, vp, i32, sz, vp, C.POINTER(i32)]
    L.ps_ransac_rigid3d.argtypes = [vp, C.POINTER(PsRansacParams), C.POINTER(PsRansacConfig), vp, vp, i32, vp, i32,
                                    vp, i32, vp, vp, C.POINTER(i32), vp, vp]
    L.ps_debug_ransac_counts.argtypes = [vp, C.POINTER(PsRansacParams), C.POINTER(PsRansacConfig), vp, vp, i32, vp,
                                         i32, vp, i32, vp, C.POINTER(i32)]
    L.ps_debug_keys_clean.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.ps_debug_limits.argtypes = [vp, i32, C.c_double, i32, i32, vp]
    L.ps_debug_fastdiv.argtypes = [vp, C.c_uint64, i32, i32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.ps_debug_mathcheck.argtypes = [vp, i32, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.ps_umeyama_f32.argtypes = [vp, vp, vp, i32, i32, vp, vp]
    L.ps_kabsch_f64.argtypes = [vp, vp, vp, i32, i32, vp]
    L.ps_keypoints2Dto3D.argtypes = [vp, vp, i32, vp, i32, i32, sz, vp, C.c_double, vp]
    L.ps_depth_view_bytes.argtypes = [i32, i32, sz]
    L.ps_depth_view_bytes.restype = sz
    L.ps_points3Dto2D.argtypes = [vp, vp, i32, vp, vp]
    L.ps_dbscan_thin.argtypes = [vp, vp, sz, vp, sz, i32, C.c_double, i32, i32, vp, C.POINTER(i32)]
    L.ps_dbscan_thin_device.argtypes = [vp, vp, vp, vp, i32, i32, C.c_double, i32, i32, vp, vp]
    L.ps_debug_dbscan_bound.argtypes = [C.c_double]
    L.ps_debug_dbscan_bound.restype = C.c_double
    L.ps_match_xyz.argtypes = [vp, vp, vp, sz, vp, i32, vp, vp, sz, vp, i32, C.c_double, C.c_double, vp, i32,
                               C.POINTER(i32)]
    L.ps_predicted_level.argtypes = [i32, C.c_double, C.c_double]
    L.ps_remove_image_distortion.argtypes = [vp, vp, i32, vp, vp, vp]
    L.ps_vo_stream_create.argtypes = [vp, i32, C.POINTER(vp)]
    L.ps_vo_stream_destroy.argtypes = [vp]
    L.ps_vo_stream_destroy.restype = None
    L.ps_vo_stream_reset.argtypes = [vp]
    L.ps_vo_stream_push.argtypes = [vp, C.POINTER(PsRansacParams), C.POINTER(PsRansacConfig), vp, vp, sz, vp, i32, vp,
                                    C.POINTER(i32), vp, vp, vp]
    L.ps_vo_stream_configure_async.argtypes = [vp, C.POINTER(PsRansacParams), C.POINTER(PsRansacConfig), vp, i32, i32]
    L.ps_vo_stream_set_result_mode.argtypes = [vp, i32]
    L.ps_vo_stream_push_async.argtypes = [vp, vp, sz, vp, i32]
    L.ps_vo_stream_push_many.argtypes = [vp, vp, vp, vp, i32]
    L.ps_vo_stream_set_frame_layout.argtypes = [vp, i32]
    L.ps_vo_stream_packed_stride.argtypes = [vp]
    L.ps_vo_stream_packed_stride.restype = sz
    L.ps_vo_stream_push_many_packed.argtypes = [vp, vp, sz, vp, i32]
    L.ps_vo_stream_flush.argtypes = [vp]
    L.ps_vo_stream_pop_many.argtypes = [vp, i32, C.POINTER(PsHostPairResults)]
    L.ps_vo_stream_pop.argtypes = [vp, i32, vp, C.POINTER(i32), vp, vp, vp]
    L.ps_vo_stream_pending.argtypes = [vp]
    L.ps_vo_stream_graph_launches.argtypes = [vp]
    L.ps_vo_stream_graph_launches.restype = C.c_longlong
    L.ps_host_alloc.argtypes = [sz]
    L.ps_host_alloc.restype = vp
    L.ps_host_free.argtypes = [vp]
    L.ps_host_free.restype = None
    L.ps_vo_pairs_device.argtypes = [vp, C.POINTER(PsRansacParams), C.POINTER(PsRansacConfig), vp,
                                     C.POINTER(PsFrameSet), vp, i32, C.POINTER(PsPairResults)]
    L.ps_map_sphere_bound.argtypes = [C.c_double]
    L.ps_map_sphere_bound.restype = C.c_float
    L.ps_match_xyz_device.argtypes = [vp, C.POINTER(PsMapBatch), vp, vp]
    L.ps_map_pairs_device.argtypes = [vp, C.POINTER(PsRansacParams), C.POINTER(PsRansacConfig), vp, C.POINTER(PsMapBatch),
                                      C.POINTER(PsPairResults)]
    L.ps_sqrt_bound_f64.argtypes = [C.c_double]
    L.ps_sqrt_bound_f64.restype = C.c_double
    L.ps_exclusion_rule_new_map_features.argtypes = [C.c_double, C.c_double, i32, C.POINTER(PsExclusionRule)]
    L.ps_exclusion_rule_merge_tracked.argtypes = [C.c_double, C.POINTER(PsExclusionRule)]
    L.ps_exclusion_rule_too_close.argtypes = [C.c_double, C.c_double, C.POINTER(PsExclusionRule)]
    L.ps_exclude.argtypes = [vp, C.POINTER(PsExclusionRule), vp, vp, i32, vp, vp, i32, vp, C.POINTER(i32)]
    L.ps_exclude_device.argtypes = [vp, C.POINTER(PsExclusionRule), vp, vp, vp, i32, vp, vp, vp, i32, i32, vp, vp]
    L.ps_level_thresholds.argtypes = [C.POINTER(C.c_double)]
    L.ps_view_angles.argtypes = [vp, vp, i32, vp]
    L.ps_map_views_device.argtypes = [vp, C.POINTER(PsMapStore), C.POINTER(PsMapViewRequest), C.POINTER(PsMapViewOut)]
    L.ps_frame_levels_device.argtypes = [vp, C.POINTER(PsFrameSet), vp, vp, vp]
    L.ps_pose_sets_device.argtypes = [vp, C.POINTER(PsMapStore), C.POINTER(PsPoseSetRequest), C.POINTER(PsPoseSetOut)]
    L.ps_loop_pairs_device.argtypes = [vp, C.POINTER(PsRansacParams), C.POINTER(PsRansacConfig), vp, C.POINTER(PsLoopBatch),
                                       C.POINTER(PsLoopResults)]
    L.ps_match_l2_f32.argtypes = [vp, vp, i32, sz, vp, i32, sz, i32, vp, C.POINTER(i32)]
    L.ps_debug_l2_band.argtypes = [vp, vp, i32, sz, vp, i32, sz, i32, vp, vp]
    L.ps_debug_l2_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.ps_match_l2_device.argtypes = [vp, C.POINTER(PsFrameSetF32), vp, i32, vp, vp]
    L.ps_vo_pairs_l2_device.argtypes = [vp, C.POINTER(PsRansacParams), C.POINTER(PsRansacConfig), vp, C.POINTER(PsFrameSetF32), vp, i32,
                                        C.POINTER(PsPairResults)]
    L.ps_match_xyz_l2_f32.argtypes = [vp, vp, vp, sz, vp, i32, vp, vp, sz, vp, i32, i32, C.c_double, C.c_double, vp, i32, C.POINTER(i32)]
    L.ps_match_xyz_l2_device.argtypes = [vp, C.POINTER(PsMapBatchF32), vp, vp]
    L.ps_map_pairs_l2_device.argtypes = [vp, C.POINTER(PsRansacParams), C.POINTER(PsRansacConfig), vp, C.POINTER(PsMapBatchF32),
                                         C.POINTER(PsPairResults)]
    L.ps_abi_sizeof_map_batch_f32.restype = sz   # (ABI_STRUCTS_F32 stays the float matcher's one struct)
    L.ps_map_views_l2_device.argtypes = [vp, C.POINTER(PsMapStoreF32), C.POINTER(PsMapViewRequest), C.POINTER(PsMapViewOutF32)]
    L.ps_pose_sets_l2_device.argtypes = [vp, C.POINTER(PsMapStoreF32), C.POINTER(PsPoseSetRequest), C.POINTER(PsPoseSetOutF32)]
    L.ps_loop_pairs_l2_device.argtypes = [vp, C.POINTER(PsRansacParams), C.POINTER(PsRansacConfig), vp, C.POINTER(PsLoopBatchF32),
                                          C.POINTER(PsLoopResults)]
    L.ps_batch_queue_create.argtypes = [vp, i32, C.POINTER(vp)]
    L.ps_batch_queue_destroy.argtypes = [vp]
    L.ps_batch_queue_destroy.restype = None
    L.ps_batch_queue_submit.argtypes = [vp, C.POINTER(PsRansacParams), C.POINTER(PsRansacConfig), vp, C.POINTER(PsFrameSet), vp, i32,
                                        C.POINTER(PsPairResults), C.POINTER(C.c_int64)]
    L.ps_batch_queue_wait.argtypes = [vp, C.c_int64]
    L.ps_batch_queue_query.argtypes = [vp, C.c_int64]
    L.ps_batch_queue_wait_on_stream.argtypes = [vp, C.c_int64, vp]
    L.ps_batch_queue_synchronize.argtypes = [vp]
    L.ps_batch_queue_chains.argtypes = [vp]
    L.ps_batch_queue_context.argtypes = [vp, i32]
    L.ps_batch_queue_context.restype = vp
    L.ps_batch_queue_last_split.argtypes = [vp, vp]
    L.ps_pack_records_device.argtypes = [vp, vp, vp, vp, i32, i32, vp]
    L.ps_algorithmic_bytes.argtypes = [i32, i32, i32, i32]
    L.ps_algorithmic_bytes.restype = C.c_uint64
    L.ps_kernel_names.restype = C.POINTER(C.c_char)
    L.ps_last_kernel_times_ms.argtypes = [vp, vp]
    L.ps_kernel_time_totals.argtypes = [vp, vp, vp]
    L.ps_context_enable_timing.argtypes = [vp, i32]
    L.ps_klt_pyramids_create.argtypes = [vp, i32, i32, i32, i32, i32, i32, C.POINTER(vp)]
    L.ps_klt_pyramids_destroy.argtypes = [vp]
    L.ps_klt_pyramids_destroy.restype = None
    L.ps_klt_pyramids_num_levels.argtypes = [vp]
    L.ps_klt_pyramids_build_device.argtypes = [vp, vp, C.POINTER(PsImageSet), i32]
    L.ps_klt_track_device.argtypes = [vp, vp, C.POINTER(PsKltParams), vp, vp, vp, i32, i32, vp, vp, vp]
    L.ps_klt_select_device.argtypes = [vp, vp, vp, vp, vp, i32, i32, C.c_double, C.c_double, vp, vp, vp, vp]
    L.ps_calc_optical_flow_pyr_lk.argtypes = [vp, vp, vp, i32, i32, i32, sz, vp, vp, i32, vp, vp, C.POINTER(PsKltParams)]
    L.ps_perform_tracking.argtypes = [vp, vp, vp, i32, i32, i32, sz, vp, vp, i32, C.POINTER(PsKltParams), C.c_double, C.c_double,
                                      vp, vp, vp, C.POINTER(i32), vp, vp]
    L.ps_debug_klt_level.argtypes = [vp, vp, i32, i32, vp, vp, vp]
    L.ps_fast_detector_create.argtypes = [vp, i32, i32, i32, i32, C.POINTER(vp)]
    L.ps_fast_detector_destroy.argtypes = [vp]
    L.ps_fast_detector_destroy.restype = None
    L.ps_detect_features_device.argtypes = [vp, vp, C.POINTER(PsImageSet), C.POINTER(PsDetectParams), i32, vp, vp, vp]
    L.ps_detect_features.argtypes = [vp, vp, i32, i32, i32, sz, C.POINTER(PsDetectParams), vp, vp, i32, C.POINTER(i32)]
    L.ps_debug_fast_maps.argtypes = [vp, vp, i32, vp, vp, vp]
    L.ps_debug_fast_passes.argtypes = [vp, vp, C.POINTER(PsImageSet), C.POINTER(PsDetectParams), i32, vp, vp, vp, i32]
    L.ps_orb_pattern_default.argtypes = [vp]
    L.ps_orb_pyramids_create.argtypes = [vp, i32, i32, i32, C.POINTER(PsOrbParams), vp, i32, C.POINTER(vp)]
    L.ps_orb_pyramids_destroy.argtypes = [vp]
    L.ps_orb_pyramids_destroy.restype = None
    L.ps_orb_pyramids_level.argtypes = [vp, i32, vp, C.POINTER(C.c_float)]
    L.ps_orb_pyramids_build_device.argtypes = [vp, vp, C.POINTER(PsImageSet), i32]
    L.ps_describe_features_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp]
    L.ps_describe_features.argtypes = [vp, vp, i32, i32, i32, sz, C.POINTER(PsOrbParams), vp, vp, vp, vp, i32, vp, vp, C.POINTER(i32)]
    L.ps_debug_orb_level.argtypes = [vp, vp, i32, i32, vp, vp]
    L.ps_debug_orb_passes.argtypes = [vp, vp, C.POINTER(PsImageSet), i32, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, i32]
    L.ps_orb_detector_create.argtypes = [vp, i32, i32, i32, C.POINTER(PsOrbDetectParams), i32, C.POINTER(vp)]
    L.ps_orb_detector_destroy.argtypes = [vp]
    L.ps_orb_detector_destroy.restype = None
    L.ps_orb_detector_level.argtypes = [vp, i32, vp, C.POINTER(C.c_float)]
    L.ps_orb_detect_quotas.argtypes = [C.POINTER(PsOrbDetectParams), vp]
    L.ps_orb_detect_frames.argtypes = [vp, vp, C.POINTER(PsImageSet), C.POINTER(PsOrbDetectParams), i32, vp, vp, vp, vp, vp]
    L.ps_detect_features_orb.argtypes = [vp, vp, i32, i32, i32, sz, C.POINTER(PsOrbDetectParams), vp, vp, vp, vp, i32, C.POINTER(i32)]
    L.ps_debug_orb_detect_level.argtypes = [vp, vp, i32, i32, vp, vp, C.POINTER(i32), vp, vp, vp, vp, i32]
    L.ps_debug_orb_detect_passes.argtypes = [vp, vp, C.POINTER(PsImageSet), C.POINTER(PsOrbDetectParams), i32, vp, vp, vp, vp, vp, i32]
    L.ps_gather_keypoints.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.ps_assemble_frames.argtypes = [vp, C.POINTER(PsFrameGeometry), C.POINTER(PsDepthSet), i32, vp, vp, vp, i32, i32, C.POINTER(PsFrameRowsOut)]
    L.ps_front_end_create.argtypes = [vp, i32, i32, i32, C.POINTER(PsFrontEndParams), vp, i32, C.POINTER(vp)]
    L.ps_front_end_destroy.argtypes = [vp]
    L.ps_front_end_destroy.restype = None
    L.ps_front_end_frames.argtypes = [vp, vp, C.POINTER(PsImageSet), C.POINTER(PsDepthSet), C.POINTER(PsFrameGeometry), i32, vp,
                                      C.POINTER(PsFrameRowsOut)]
    L.ps_front_end_frame.argtypes = [vp, vp, vp, i32, i32, i32, sz, sz, C.POINTER(PsFrontEndParams), vp, C.POINTER(PsFrameGeometry), vp,
                                     C.POINTER(PsFrameRowsOut), i32, C.POINTER(i32)]
    L.ps_ransac_match_lists.argtypes = [vp, C.POINTER(PsRansacParams), C.POINTER(PsRansacConfig), vp, C.POINTER(PsPointSets),
                                        C.POINTER(PsPointSets), vp, vp, vp, i32, i32, C.POINTER(PsPairResults)]
    L.ps_assemble_tracked.argtypes = [vp, C.POINTER(PsFrameGeometry), C.POINTER(PsDepthSet), vp, vp, vp, vp, i32, i32, C.POINTER(PsTrackedCarry),
                                      C.POINTER(PsTrackedRows)]
    L.ps_track_vo_pairs.argtypes = [vp, vp, C.POINTER(PsKltParams), C.POINTER(PsTrackVoParams), C.POINTER(PsRansacParams),
                                    C.POINTER(PsRansacConfig), C.POINTER(PsFrameGeometry), C.POINTER(PsDepthSet), C.POINTER(PsTrackVoIn), i32, i32,
                                    C.POINTER(PsTrackVoOut)]
    L.ps_track_vo_pair.argtypes = [vp, vp, vp, vp, i32, i32, i32, sz, sz, C.POINTER(PsKltParams), C.POINTER(PsTrackVoParams),
                                   C.POINTER(PsRansacParams), C.POINTER(PsRansacConfig), C.POINTER(PsFrameGeometry), C.POINTER(PsTrackVoIn), i32,
                                   C.POINTER(PsTrackVoOut), C.POINTER(i32)]
    L.ps_track_candidates.argtypes = [vp, vp, C.POINTER(PsImageSet), C.POINTER(PsDepthSet), C.POINTER(PsFrameGeometry), i32,
                                      C.POINTER(PsFrameRowsOut)]
    L.ps_track_close_create.argtypes = [vp, i32, i32, C.POINTER(vp)]
    L.ps_track_close_destroy.argtypes = [vp]
    L.ps_track_close_destroy.restype = None
    L.ps_track_close_pairs.argtypes = [vp, vp, vp, vp, C.POINTER(PsTrackCloseParams), C.POINTER(PsTrackedRows), C.POINTER(PsTrackCandidates),
                                       vp, i32, i32, i32, C.POINTER(PsTrackCloseOut)]
    L.ps_debug_track_close_passes.argtypes = L.ps_track_close_pairs.argtypes + [i32]
    L.ps_track_close_pair.argtypes = [vp, vp, vp, i32, i32, i32, sz, sz, C.POINTER(PsFrontEndParams), vp, C.POINTER(PsFrameGeometry),
                                      C.POINTER(PsTrackCloseParams), C.POINTER(PsTrackedRows), i32, vp, C.POINTER(PsTrackedRows), vp, i32,
                                      C.POINTER(i32), C.POINTER(i32)]
    L.ps_sensor_model_default.argtypes = [C.POINTER(PsSensorModel)]
    L.ps_debug_gradient_tie_table.argtypes = [i32, vp]
    L.ps_feature_uncertainty.argtypes = [vp, C.POINTER(PsFrameGeometry), C.POINTER(PsSensorModel), i32, C.POINTER(PsImageSet),
                                         C.POINTER(PsDepthSet), vp, vp, vp, vp, i32, i32, C.POINTER(PsUncertaintyOut)]
    L.ps_measurement_edges.argtypes = [vp, C.POINTER(PsFrameGeometry), C.POINTER(PsSensorModel), i32, C.POINTER(PsImageSet),
                                       C.POINTER(PsDepthSet), vp, C.POINTER(PsMapBatch), C.POINTER(PsPairResults), vp,
                                       C.POINTER(PsMeasurementEdgesOut)]
    L.ps_compute_normals.argtypes = [vp, C.POINTER(PsFrameGeometry), vp, i32, i32, sz, vp, i32, vp]
    L.ps_compute_rgb_gradients.argtypes = [vp, C.POINTER(PsFrameGeometry), vp, i32, sz, vp, i32, i32, sz, vp, i32, vp]
    L.ps_information_matrices.argtypes = [vp, C.POINTER(PsFrameGeometry), C.POINTER(PsSensorModel), i32, vp, i32, sz, vp, i32, i32, sz,
                                          vp, vp, i32, vp]
    L.ps_patch_models.argtypes = [vp, C.POINTER(PsImageSet), vp, vp, vp, i32, i32, C.POINTER(PsPatchParams), C.POINTER(PsPatchModel), vp]
    L.ps_patch_align.argtypes = [vp, C.POINTER(PsImageSet), vp, vp, vp, vp, i32, i32, C.POINTER(PsPatchParams), C.POINTER(PsPatchModel), vp, vp]
    L.ps_compute_patch.argtypes = [vp, vp, i32, i32, i32, sz, vp, i32, C.POINTER(PsPatchParams), vp, vp]
    L.ps_compute_patch_gradient.argtypes = [vp, vp, i32, i32, i32, sz, vp, i32, C.POINTER(PsPatchParams), vp, vp, vp, vp]
    L.ps_optimize_location.argtypes = [vp, vp, vp, vp, i32, i32, i32, sz, vp, i32, vp, vp, vp, C.POINTER(PsPatchParams), vp, vp]
    L.ps_optimize_locations.argtypes = [vp, vp, vp, i32, i32, i32, sz, vp, vp, i32, C.POINTER(PsPatchParams), vp, vp]
    for n in (list(ABI_STRUCTS) + list(ABI_STRUCTS_F32) + list(ABI_STRUCTS_STORE_F32) + list(ABI_STRUCTS_KLT) + list(ABI_STRUCTS_DETECT)
              + list(ABI_STRUCTS_ORB) + list(ABI_STRUCTS_ORB_DETECT) + list(ABI_STRUCTS_FRAME_ASSEMBLY) + list(ABI_STRUCTS_TRACK_VO)
              + list(ABI_STRUCTS_TRACK_CLOSE) + list(ABI_STRUCTS_UNCERTAINTY) + list(ABI_STRUCTS_PATCHES)):
        getattr(L, "ps_abi_sizeof_" + n).restype = sz
    _by_path[path] = real
    return real


def struct_sizes():
    return {n: C.sizeof(t) for n, t in ABI_STRUCTS.items()}


def struct_sizes_f32():
    return {n: C.sizeof(t) for n, t in ABI_STRUCTS_F32.items()}


def struct_sizes_store_f32():
    return {n: C.sizeof(t) for n, t in ABI_STRUCTS_STORE_F32.items()}


def struct_sizes_klt():
    return {n: C.sizeof(t) for n, t in ABI_STRUCTS_KLT.items()}


def struct_sizes_detect():
    return {n: C.sizeof(t) for n, t in ABI_STRUCTS_DETECT.items()}


def struct_sizes_orb():
    return {n: C.sizeof(t) for n, t in ABI_STRUCTS_ORB.items()}


def struct_sizes_orb_detect():
    return {n: C.sizeof(t) for n, t in ABI_STRUCTS_ORB_DETECT.items()}


def struct_sizes_frame_assembly():
    return {n: C.sizeof(t) for n, t in ABI_STRUCTS_FRAME_ASSEMBLY.items()}


def struct_sizes_track_vo():
    return {n: C.sizeof(t) for n, t in ABI_STRUCTS_TRACK_VO.items()}


def struct_sizes_track_close():
    return {n: C.sizeof(t) for n, t in ABI_STRUCTS_TRACK_CLOSE.items()}


def struct_sizes_uncertainty():
    return {n: C.sizeof(t) for n, t in ABI_STRUCTS_UNCERTAINTY.items()}


def struct_sizes_patches():
    return {n: C.sizeof(t) for n, t in ABI_STRUCTS_PATCHES.items()}
