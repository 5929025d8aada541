"""stereo-visual-slam_amd -- MI355X (gfx950) build of the stereo-VO hot path of shangzhouye/stereo-visual-slam.

This Python layer is plumbing: a ctypes binding of the C-ABI in include/vslam_hip.h (libvslam_hip.so, hand-written
HIP kernels) whose method names mirror the reference's C++ surface (visual_odometry.hpp, optimization.hpp) so that
the parity tests read like calls into the reference.  There is NO CPU fallback: if libvslam_hip.so is missing or no
GPU is visible, every compute call raises.

Import name: `stereo_visual_slam_amd` (the repo-root shim maps it to this hyphenated directory).
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libvslam_hip.so")

VSLAM_OK, VSLAM_ERR_ARG, VSLAM_ERR_HIP, VSLAM_ERR_CAPACITY, VSLAM_ERR_NO_DEVICE = 0, -1, -2, -3, -4
MAX_KF = 12
MAX_ROWS = 4096

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                           ("octave", "<i4"), ("class_id", "<i4")])
DMATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])


class Params(C.Structure):
    _fields_ = [("img_w", C.c_int32), ("img_h", C.c_int32), ("max_batch", C.c_int32), ("orb_nfeatures", C.c_int32),
                ("anms_num", C.c_int32), ("fast_threshold", C.c_int32), ("kp_capacity", C.c_int32),
                ("cam", C.c_double * 5), ("depth_min", C.c_double), ("depth_max", C.c_double),
                ("depth_reliable", C.c_double), ("match_ratio", C.c_double), ("match_gap_thr", C.c_double),
                ("huber_delta", C.c_double), ("pnp_reproj_thr", C.c_double), ("stereo_row_tol", C.c_double),
                ("struct_size", C.c_int32), ("abi_version", C.c_int32)]


class SgbmParams(C.Structure):
    """vslam_sgbm_params: the cv::StereoSGBM::create arguments a caller may set (minDisparity 0, MODE_SGBM)"""
    _fields_ = [("num_disparities", C.c_int32), ("block_size", C.c_int32), ("P1", C.c_int32), ("P2", C.c_int32),
                ("disp12_max_diff", C.c_int32), ("pre_filter_cap", C.c_int32), ("uniqueness_ratio", C.c_int32),
                ("speckle_window_size", C.c_int32), ("speckle_range", C.c_int32), ("struct_size", C.c_int32)]

    def as_tuple(self):
        return tuple(getattr(self, f) for f, _ in self._fields_[:9])


class RectifyCam(C.Structure):
    """vslam_rectify_cam: one camera of a raw stereo rig -- K (fx fy cx cy, raw), D (k1 k2 p1 p2 k3 k4 k5 k6), R (rectifying rotation,
    row-major), P (fx' fy' cx' cy', rectified)"""
    _fields_ = [("K", C.c_double * 4), ("D", C.c_double * 8), ("R", C.c_double * 9), ("P", C.c_double * 4)]


class RectifyParams(C.Structure):
    """vslam_rectify_params: the raw image size and the two cameras (0 = left, 1 = right)"""
    _fields_ = [("src_w", C.c_int32), ("src_h", C.c_int32), ("cam", RectifyCam * 2), ("struct_size", C.c_int32)]


ABI_VERSION = 5  # VSLAM_ABI_VERSION of include/vslam_hip.h this binding was written against


class LmStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("total_trials", C.c_int32), ("chi2_init", C.c_double),
                ("chi2_final", C.c_double), ("lambda_final", C.c_double), ("chi2_iter", C.c_double * 32),
                ("lambda_iter", C.c_double * 32), ("trials_iter", C.c_int32 * 32)]

    def as_dict(self):
        n = min(self.iterations, 32)
        return dict(iterations=self.iterations, total_trials=self.total_trials, chi2_init=self.chi2_init,
                    chi2_final=self.chi2_final, lambda_final=self.lambda_final, chi2_iter=list(self.chi2_iter)[:n],
                    lambda_iter=list(self.lambda_iter)[:n], trials_iter=list(self.trials_iter)[:n])


class BaBatch(C.Structure):
    _fields_ = [("n_windows", C.c_int32), ("n_kf", C.c_int32), ("d_lm_off", C.c_void_p), ("d_edge_off", C.c_void_p),
                ("d_T_c_w", C.c_void_p), ("d_xyz", C.c_void_p), ("d_reliable", C.c_void_p), ("d_lm_inlier", C.c_void_p),
                ("d_kf_idx", C.c_void_p), ("d_lm_idx", C.c_void_p), ("d_uv", C.c_void_p), ("d_chi2", C.c_void_p),
                ("d_stats", C.c_void_p), ("total_lm", C.c_int32), ("total_edge", C.c_int32), ("K4", C.c_void_p), ("d_n_kf", C.c_void_p)]


class TracksIn(C.Structure):
    """vslam_tracks_in: the front end's per-frame results (device pointers) that vslam_build_windows_dev turns into BA windows"""
    _fields_ = [("n_frames", C.c_int32), ("kp_capacity", C.c_int32), ("lr_capacity", C.c_int32), ("match_capacity", C.c_int32),
                ("pnp_capacity", C.c_int32), ("d_kps", C.c_void_p), ("d_lr", C.c_void_p), ("d_nlr", C.c_void_p), ("d_xyz", C.c_void_p),
                ("d_valid", C.c_void_p), ("d_reliable", C.c_void_p), ("d_f2f", C.c_void_p), ("d_nf2f", C.c_void_p),
                ("d_pose_inlier", C.c_void_p), ("d_T_rel", C.c_void_p), ("d_nkps", C.c_void_p),
                # ABI rev 5: a chunk of a longer sequence -- absolute poses, carry across the chunk boundaries (all optional)
                ("d_T_abs", C.c_void_p), ("d_carry_in", C.c_void_p), ("d_carry_out", C.c_void_p), ("carry_out_frame", C.c_int32)]


class VoxelStats(C.Structure):
    """struct vslam_voxel_stats: the counters of a voxel map (status bit 0: table full, bit 1: a voxel count reached 2^24)"""
    _fields_ = [("n_occupied", C.c_uint64), ("n_points", C.c_uint64), ("n_dropped_range", C.c_uint64), ("n_dropped_full", C.c_uint64),
                ("status", C.c_uint32), ("struct_size", C.c_int32)]

    def as_dict(self):
        return {f: int(getattr(self, f)) for f, _ in self._fields_[:5]}


# vslam_voxel (32 bytes) and the form VoxelMap.extract() returns it in: the map id in front, sorted by (map, ix, iy, iz)
VOXEL_DTYPE = np.dtype([("ix", "<i4"), ("iy", "<i4"), ("iz", "<i4"), ("count", "<u4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4")])
VOXEL_MAP_DTYPE = np.dtype([("map", "<i4")] + VOXEL_DTYPE.descr)
VOXEL_MAX_MAP = 1022


class TsdfStats(C.Structure):
    """struct vslam_tsdf_stats: the counters of a surface map (status bit 0: pool full, bit 1: a weight reached 2^20, bit 2: a frame skipped for its pose,
    bit 3: a re-integration met a sum below what it was to take out)"""
    _fields_ = [("n_blocks", C.c_uint64), ("n_samples", C.c_uint64), ("n_dropped_range", C.c_uint64), ("n_dropped_full", C.c_uint64),
                ("n_frames_skipped", C.c_uint64), ("n_pairs_visited", C.c_uint64), ("n_pairs_kept", C.c_uint64), ("status", C.c_uint32), ("struct_size", C.c_int32)]

    def as_dict(self):
        return {f: int(getattr(self, f)) for f, _ in self._fields_[:8]}


# vslam_surfel (48 bytes) and the form TsdfMap.extract() returns it in: the map id in front, sorted by (map, ix, iy, iz, axis)
SURFEL_DTYPE = np.dtype([("ix", "<i4"), ("iy", "<i4"), ("iz", "<i4"), ("axis", "<u4"), ("weight", "<u4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4"),
                         ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("intensity", "<f4")])
SURFEL_MAP_DTYPE = np.dtype([("map", "<i4")] + SURFEL_DTYPE.descr)


class TsdfRenderParams(C.Structure):
    """struct vslam_tsdf_render_params: the camera, image size, depth range, step (in voxels) and weight gate of one vslam_tsdf_render_dev call"""
    _fields_ = [("struct_size", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("z_min", C.c_double), ("z_max", C.c_double), ("march", C.c_double), ("min_weight", C.c_int32), ("reserved", C.c_int32)]


class TsdfDistanceParams(C.Structure):
    """struct vslam_tsdf_distance_params: the maps covered, the weight gate, the radius in voxels and the size of the layer's table of one
    vslam_tsdf_distance_dev call"""
    _fields_ = [("struct_size", C.c_int32), ("map_id", C.c_int32), ("min_weight", C.c_int32), ("radius_voxels", C.c_int32),
                ("log2_layer_blocks", C.c_int32), ("reserved", C.c_int32)]


class PlaceStats(C.Structure):
    """struct vslam_place_stats: entries held, capacity, rows per entry, geometry flag and the adds refused for lack of room"""
    _fields_ = [("n_entries", C.c_int32), ("capacity", C.c_int32), ("rows_per_entry", C.c_int32), ("with_geometry", C.c_int32),
                ("n_refused", C.c_uint64), ("struct_size", C.c_int32)]

    def as_dict(self):
        return {f: int(getattr(self, f)) for f, _ in self._fields_[:5]}


# the rows KeyframePipeline.loop_closures returns: one per (query entry, candidate)
LOOP_EDGE_DTYPE = np.dtype([("entry_q", "<i4"), ("entry_c", "<i4"), ("seq", "<i4"), ("frame_q", "<i4"), ("frame_c", "<i4"), ("score", "<i4"),
                            ("n_matches", "<i4"), ("n_inliers", "<i4"), ("accepted", "?"), ("T_q_c", "<f8", (7,))])


class PoseGraphBatch(C.Structure):
    """vslam_pose_graph: a batch of independent pose graphs laid back to back (device pointers); struct_size is filled in by VO.pose_graph_dev"""
    _fields_ = [("struct_size", C.c_int32), ("n_graphs", C.c_int32), ("total_nodes", C.c_int32), ("total_edges", C.c_int32),
                ("d_node_off", C.c_void_p), ("d_edge_off", C.c_void_p), ("d_T", C.c_void_p), ("d_fixed", C.c_void_p), ("d_edge_i", C.c_void_p),
                ("d_edge_j", C.c_void_p), ("d_edge_Z", C.c_void_p), ("d_edge_w", C.c_void_p), ("d_edge_active", C.c_void_p), ("d_edge_chi2", C.c_void_p)]


class PoseGraphParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("max_iters", C.c_int32), ("pcg_max_iters", C.c_int32), ("reserved", C.c_int32),
                ("pcg_tol", C.c_double), ("step_tol", C.c_double), ("lambda_init", C.c_double)]


# vslam_pose_graph_stats, one per graph
POSE_GRAPH_STATS_DTYPE = np.dtype([("chi2_init", "<f8"), ("chi2_final", "<f8"), ("lambda", "<f8"), ("lm_iters", "<i4"), ("pcg_iters", "<i4"),
                                   ("n_free", "<i4"), ("status", "<i4")])
PG_BAD_INDEX, PG_NONFINITE, PG_PCG_CAP, PG_LAMBDA, PG_SINGULAR = 1, 2, 4, 8, 16


class FullBABatch(C.Structure):
    """vslam_full_ba: a batch of independent full bundle adjustment problems laid back to back (device pointers, the camera by value); struct_size is
    filled in by VO.full_ba_dev"""
    _fields_ = [("struct_size", C.c_int32), ("n_problems", C.c_int32), ("total_kfs", C.c_int32), ("total_lms", C.c_int32), ("total_obs", C.c_int32),
                ("total_edges", C.c_int32), ("d_kf_off", C.c_void_p), ("d_lm_off", C.c_void_p), ("d_obs_off", C.c_void_p), ("d_edge_off", C.c_void_p),
                ("d_T", C.c_void_p), ("d_fixed", C.c_void_p), ("d_xyz", C.c_void_p), ("d_obs_kf", C.c_void_p), ("d_obs_lm", C.c_void_p),
                ("d_obs_uv", C.c_void_p), ("d_obs_disp", C.c_void_p), ("d_obs_active", C.c_void_p), ("d_obs_chi2", C.c_void_p), ("d_edge_i", C.c_void_p),
                ("d_edge_j", C.c_void_p), ("d_edge_Z", C.c_void_p), ("d_edge_w", C.c_void_p), ("d_edge_active", C.c_void_p), ("K4", C.c_double * 4),
                ("bf", C.c_double), ("huber_delta", C.c_double)]


class FullBAParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("max_iters", C.c_int32), ("pcg_max_iters", C.c_int32), ("reserved", C.c_int32),
                ("pcg_tol", C.c_double), ("step_tol", C.c_double), ("lambda_init", C.c_double)]


# vslam_full_ba_stats, one per problem
FULL_BA_STATS_DTYPE = np.dtype([("chi2_init", "<f8"), ("chi2_final", "<f8"), ("lambda", "<f8"), ("lm_iters", "<i4"), ("pcg_iters", "<i4"), ("n_free", "<i4"),
                                ("n_obs_dropped", "<i4"), ("status", "<i4"), ("reserved", "<i4")])
FBA_BAD_INDEX, FBA_NONFINITE, FBA_PCG_CAP, FBA_LAMBDA, FBA_SINGULAR, FBA_DROPPED = 1, 2, 4, 8, 16, 32


class ProjectMatchBatch(C.Structure):
    """vslam_project_match: a batch of match-by-projection items laid back to back (device pointers; K4 a HOST pointer or None); struct_size is filled in
    by VO.project_match_dev"""
    _fields_ = [("struct_size", C.c_int32), ("n_items", C.c_int32), ("n_landmarks", C.c_int32), ("B", C.c_int32), ("kp_capacity", C.c_int32),
                ("n_src_rows", C.c_int32), ("d_lm_off", C.c_void_p), ("d_item_img", C.c_void_p), ("d_item_T", C.c_void_p), ("d_lm_xyz", C.c_void_p),
                ("d_lm_desc_row", C.c_void_p), ("d_src_desc", C.c_void_p), ("d_kps", C.c_void_p), ("d_desc", C.c_void_p), ("desc_stride_bytes", C.c_size_t),
                ("d_n", C.c_void_p), ("K4", C.POINTER(C.c_double)), ("d_match", C.c_void_p), ("d_dist", C.c_void_p), ("d_n_cand", C.c_void_p),
                ("d_status", C.c_void_p)]


class ProjectMatchParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("radius_px", C.c_float), ("tau", C.c_int32), ("ratio_pct", C.c_int32), ("z_min", C.c_double),
                ("z_max", C.c_double)]


PM_MATCHED, PM_BEHIND, PM_OUTSIDE, PM_NO_CANDIDATE, PM_TOO_FAR, PM_AMBIGUOUS, PM_CONTESTED, PM_INVALID = range(8)
PROJECT_MATCH_MAX_KP = 4096


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("total_ms", C.c_double), ("launches", C.c_int32), ("calls", C.c_int32)]


class StageInterval(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("t0_ms", C.c_double), ("t1_ms", C.c_double)]


class VslamError(RuntimeError):
    pass


class Ptr:
    """pointer parameter of the C-ABI: None, an int (a device address, e.g. torch.Tensor.data_ptr()), a numpy array (its data),
    or a ctypes object (byref, array, c_void_p)"""

    @classmethod
    def from_param(cls, a):
        if a is None or isinstance(a, int):
            return C.c_void_p(a)
        if isinstance(a, np.ndarray):
            return C.c_void_p(a.ctypes.data)
        return a


# restype and argtypes of every symbol include/vslam_hip.h declares, in its order (tests/test_abi.py checks them against the prototypes)
P, I, D, Z = Ptr, C.c_int, C.c_double, C.c_size_t
SIGNATURES = {
    "vslam_default_params": (None, [P]),
    "vslam_create": (I, [C.POINTER(Params), I, P, C.POINTER(C.c_void_p)]),
    "vslam_destroy": (None, [P]),
    "vslam_last_error": (C.c_char_p, []), "vslam_version": (C.c_char_p, []), "vslam_abi_version": (I, []), "vslam_sync": (I, [P]),
    "vslam_device_bytes": (Z, [P]), "vslam_kernel_names": (C.c_char_p, []),
    "vslam_default_rectify_params": (None, [P]),
    "vslam_rectify_params_check": (I, [P, I, I]),
    "vslam_rectify_build_maps": (I, [P, I, I, I, P, P]),
    "vslam_rectify_set": (I, [P, P]),
    "vslam_rectify_set_maps": (I, [P, I, P, P, I, I]),
    "vslam_rectify": (I, [P, I, P, I, P, I]),
    "vslam_rectify_dev": (I, [P, P, P, Z, I, I, P, P, Z, I]),
    "vslam_feature_detection": (I, [P, P, I, I, I, P, P, I, P]),
    "vslam_orb_detect": (I, [P, P, I, I, I, P, I, P]),
    "vslam_anms": (I, [P, P, I, I, P]),
    "vslam_orb_compute": (I, [P, P, I, I, I, P, I, P, P]),
    "vslam_feature_detection_dev": (I, [P, P, Z, I, I, P, P, P]),
    "vslam_feature_matching": (I, [P, P, I, P, I, D, I, P, P]),
    "vslam_feature_matching_dev": (I, [P, P, Z, P, P, Z, P, P, I, I, I, P, I, P]),
    "vslam_feature_matching_subset_dev": (I, [P, P, Z, P, P, P, I, P, Z, P, P, I, I, I, P, I, P]),
    "vslam_feature_matching_pairs_dev": (I, [P, P, Z, P, P, P, I, P, I, P, Z, P, P, I, I, I, P, I, P]),
    "vslam_disparity_map": (I, [P, P, P, I, I, I, P, P, P]),
    "vslam_disparity_map_dev": (I, [P, P, P, Z, I, I, I, I, P, P, P]),
    "vslam_default_sgbm_params": (None, [P]),
    "vslam_sgbm_params_check": (I, [P, I, I]),
    "vslam_disparity_map_ex": (I, [P, P, P, I, I, I, P, P, P, P]),
    "vslam_disparity_map_ex_dev": (I, [P, P, P, Z, I, I, I, I, P, P, P, P]),
    "vslam_find_3d_disparity": (I, [P, P, I, P, I, I, I, P, P, P, P, P]),
    "vslam_triangulate": (I, [P, P, P, I, P, P, P, P, P]),
    "vslam_find_3d_disparity_dev": (I, [P, P, P, I, I, P, I, I, P, P, P, P]),
    "vslam_triangulate_dev": (I, [P, P, P, P, I, I, P, P, P, P]),
    "vslam_gather_matched_uv_dev": (I, [P, P, P, I, P, P, I, I, P, P]),
    "vslam_pnp_motion_only": (I, [P, P, P, I, P, I, P, P, P]),
    "vslam_pnp_motion_only_dev": (I, [P, P, P, P, I, I, P, I, P, P]),
    "vslam_pnp_ransac": (I, [P, P, P, I, P, I, D, D, I, P, P, P]),
    "vslam_pnp_ransac_models": (I, [P, P, P, I, P, I, D, D, I, P, P, P, P, P]),
    "vslam_pnp_ransac_dev": (I, [P, P, P, P, I, I, P, I, D, D, P, P, P]),
    "vslam_check_motion": (I, [I, P, D]),
    "vslam_local_ba": (I, [P, I, P, I, P, I, P, P, P, P, P, I, I, I, P, P, P, P]),
    "vslam_pose_only_window": (I, [P, I, P, I, P, I, P, P, P, P, P, I, I, P, P, P, P]),
    "vslam_ba_batch_dev": (I, [P, P, I, I, I, I, I]),
    "vslam_set_window_ids": (I, [P, P, I]),
    "vslam_ba_chain_dev": (I, [P, P, P, P, I, P]),
    "vslam_build_windows_dev": (I, [P, P, I, I, I, P, P]),
    "vslam_build_windows_kf_dev": (I, [P, P, I, I, D, I, I, P, P, P, P]),
    "vslam_build_windows_gated_dev": (I, [P, P, I, I, D, P, I, I, P, P, P, P, P]),
    "vslam_set_segments": (I, [P, I, P]),
    "vslam_chain_poses_dev": (I, [P, I, P, P]),
    "vslam_build_map_pnp_inputs_dev": (I, [P, P, P, P, P, P, P, P, I, P]),
    "vslam_build_windows_map_dev": (I, [P, P, P, P, I, I, D, I, I, P, P, P, P]),
    "vslam_gate_states_dev": (I, [P, I, P, I, P, P]),
    "vslam_build_map_pnp_inputs_gated_dev": (I, [P, P, P, P, P, P, P, P, P, I, P]),
    "vslam_build_map_pnp_inputs_requery_dev": (I, [P, P, P, P, P, P, Z, P, P, P, P, P, P, P, P, I, P]),
    "vslam_build_windows_map_gated_dev": (I, [P, P, P, P, P, I, I, D, I, I, P, P, P, P]),
    "vslam_frame_pairs_dev": (I, [P, I, P, P, P]),
    "vslam_gate_states_pairs_dev": (I, [P, I, P, P, P, P]),
    "vslam_build_map_pnp_inputs_recover_dev": (I, [P, P, P, P, P, P, P, Z, P, P, P, P, P, P, P, P, I, P, P, P]),
    "vslam_build_windows_map_recover_dev": (I, [P, P, P, P, P, P, I, I, D, I, I, P, P, P, P]),
    "vslam_ba_status_dev": (I, [P, I, P]), "vslam_ba_schedule_passes_dev": (I, [P, I, P]), "vslam_ba_deferred_dev": (I, [P, I, P]),
    "vslam_edge_jacobians": (I, [P, I, P, P, P, P, P, P, P, P, P]),
    "vslam_set_tuning": (I, [P, C.c_char_p, I]), "vslam_sgbm_status_dev": (I, [P, P]), "vslam_orb_status_dev": (I, [P, I, P]), "vslam_orb_anms_path_dev": (I, [P, I, P]),
    "vslam_orb_level": (I, [P, I, I, I, P, I, I, P, P]),
    "vslam_build_pnp_inputs_dev": (I, [P, P, P, I, P, P, I, P, P, P, I, I, P, P, P, P, I]),
    "vslam_profile_enable": (I, [P, I]), "vslam_profile_read": (I, [P, P, I, P]), "vslam_profile_intervals": (I, [P, P, I, P]),
    "vslam_hbm_copy_probe": (I, [P, Z, I, P]), "vslam_hbm_copy_probe_variants": (I, []), "vslam_hbm_copy_probe_variant": (I, [P, Z, I, I, P, P]),
    "vslam_voxel_create": (I, [P, D, I, C.POINTER(C.c_void_p)]), "vslam_voxel_destroy": (None, [P]), "vslam_voxel_clear": (I, [P]),
    "vslam_voxel_stats": (I, [P, C.POINTER(VoxelStats)]),
    "vslam_reproject_dev": (I, [P, P, I, I, I, P, D, D, I, P, P]),
    "vslam_voxel_insert_points_dev": (I, [P, P, P, P, P, Z, I]),
    "vslam_voxel_fuse_disparity_dev": (I, [P, P, P, P, Z, I, I, I, I, P, P, D, D, I]),
    "vslam_voxel_extract_dev": (I, [P, P, I, I, P, P, Z, P]),
    "vslam_tsdf_create": (I, [P, D, I, I, C.POINTER(C.c_void_p)]), "vslam_tsdf_destroy": (None, [P]), "vslam_tsdf_clear": (I, [P]),
    "vslam_tsdf_stats": (I, [P, C.POINTER(TsdfStats)]),
    "vslam_tsdf_integrate_dev": (I, [P, P, P, P, Z, I, I, I, I, P, P, D, D, I]),
    "vslam_tsdf_reach_dev": (I, [P, P, P]),
    "vslam_tsdf_reintegrate_dev": (I, [P, P, P, P, Z, I, I, I, I, P, P, P, P, D, D, I]),
    "vslam_tsdf_extract_dev": (I, [P, P, I, I, P, P, Z, P]),
    "vslam_tsdf_blocks_dev": (I, [P, P, I, P, P, Z, P]),
    "vslam_tsdf_mesh_dev": (I, [P, P, I, I, P, P, Z, P, Z, P]),
    "vslam_tsdf_load_blocks_dev": (I, [P, P, P, P, Z]),
    "vslam_tsdf_render_dev": (I, [P, P, C.POINTER(TsdfRenderParams), I, P, P, P, P, P]),
    "vslam_tsdf_distance_dev": (I, [P, P, C.POINTER(TsdfDistanceParams), P]),
    "vslam_tsdf_distance_blocks_dev": (I, [P, P, I, P, P, Z, P]),
    "vslam_tsdf_distance_query_dev": (I, [P, P, P, P, Z, P, P]),
    "vslam_place_create": (I, [P, I, I, I, C.POINTER(C.c_void_p)]), "vslam_place_destroy": (None, [P]), "vslam_place_clear": (I, [P]),
    "vslam_place_stats": (I, [P, C.POINTER(PlaceStats)]),
    "vslam_place_read_entry": (I, [P, I, P, P, P, P, P, P]),
    "vslam_place_read_meta": (I, [P, I, I, P, P, P]),
    "vslam_place_add_dev": (I, [P, P, P, Z, P, P, P, P, P, P, P, I, I, P]),
    "vslam_place_score_dev": (I, [P, P, I, I, I, I, P, I]),
    "vslam_place_select_dev": (I, [P, P, I, I, P, I, I, I, P, P]),
    "vslam_place_verify_dev": (I, [P, P, I, I, P, I, I, I, P, P, P]),
    "vslam_pose_graph_default_params": (None, [C.POINTER(PoseGraphParams)]),
    "vslam_pose_graph_dev": (I, [P, C.POINTER(PoseGraphBatch), C.POINTER(PoseGraphParams), P, P]),
    "vslam_pose_graph_status_dev": (I, [P, I, P]),
    "vslam_full_ba_default_params": (None, [C.POINTER(FullBAParams)]),
    "vslam_full_ba_dev": (I, [P, C.POINTER(FullBABatch), C.POINTER(FullBAParams), P, P, P]),
    "vslam_full_ba_status_dev": (I, [P, I, P]),
    "vslam_project_match_default_params": (None, [C.POINTER(ProjectMatchParams)]),
    "vslam_project_match_dev": (I, [P, C.POINTER(ProjectMatchBatch), C.POINTER(ProjectMatchParams)]),
    "vslam_dev_alloc": (I, [P, Z]), "vslam_dev_free": (I, [P]), "vslam_dev_upload": (I, [P, P, P, Z]), "vslam_dev_download": (I, [P, P, P, Z]),
    "vslam_dev_memset": (I, [P, P, I, Z]),
}
ABI_SYMBOLS = list(SIGNATURES)
del P, I, D, Z


def build(force=False):
    """compile libvslam_hip.so for gfx950 (hipcc cross-compiles without a GPU)"""
    csrc = os.path.join(_HERE, "csrc")
    cmd = ["make", "-C", csrc, "-j8", "-s"]
    if force:
        subprocess.check_call(["make", "-C", csrc, "clean", "-s"])
    subprocess.check_call(cmd)
    return _SO


_lib = None


def load_library():
    """load libvslam_hip.so; raises (loudly) when it has not been built"""
    global _lib
    if _lib is not None:
        return _lib
    try:
        # torch bundles its own libamdhip64 (same SONAME).  Import it first so that this library binds to the HIP runtime
        # torch already loaded: two HIP runtimes in one process cannot both own the GPU.
        import torch  # noqa: F401
    except Exception:
        pass
    if not os.path.exists(_SO):
        raise VslamError("libvslam_hip.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                         "(there is no CPU fallback for the HIP path)")
    lib = C.CDLL(_SO)
    if not hasattr(lib, "vslam_abi_version") or lib.vslam_abi_version() != ABI_VERSION:
        raise VslamError("libvslam_hip.so was built from a different ABI revision than this binding (%s vs %d): rebuild it"
                         % (lib.vslam_abi_version() if hasattr(lib, "vslam_abi_version") else "pre-3", ABI_VERSION))
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def default_params(**kw):
    p = Params()
    load_library().vslam_default_params(C.byref(p))
    for k, v in kw.items():
        if k == "cam":
            for i in range(5):
                p.cam[i] = float(v[i])
        else:
            setattr(p, k, v)
    return p


def default_sgbm_params(**kw):
    """the reference's StereoSGBM set (96, 9, 648, 2592, 1, 63, 10, 100, 32), fields overridden by keyword"""
    p = SgbmParams()
    load_library().vslam_default_sgbm_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _sgbm_params(sgbm):
    """None (the reference's set), an SgbmParams, a dict of fields, or a tuple (num_disparities, block_size[, P1, P2, ...]) in field
    order; a tuple without P1 / P2 gets OpenCV's recommended 8 / 32 * block_size^2"""
    if sgbm is None or isinstance(sgbm, SgbmParams):
        return sgbm
    if isinstance(sgbm, dict):
        return default_sgbm_params(**sgbm)
    vals = [int(v) for v in sgbm]
    names = [f for f, _ in SgbmParams._fields_[:9]]
    assert 2 <= len(vals) <= 9 and len(vals) != 3, "SGBM set: (num_disparities, block_size[, P1, P2, ...])"
    if len(vals) == 2:
        vals += [8 * vals[1] ** 2, 32 * vals[1] ** 2]
    return default_sgbm_params(**dict(zip(names, vals)))


def sgbm_params_check(p, w, h):
    """vslam_sgbm_params_check: is the set admissible for w x h images?  Host arithmetic, needs no GPU.  Raises VslamError naming the field."""
    lib = load_library()
    p = _sgbm_params(p)
    if p is None:
        p = default_sgbm_params()
    rc = lib.vslam_sgbm_params_check(C.byref(p), w, h)
    if rc != VSLAM_OK:
        raise VslamError("vslam_sgbm_params_check failed (%d): %s" % (rc, lib.vslam_last_error().decode()))
    return True


def default_rectify_params(src_w=None, src_h=None, cams=None):
    """the identity rig at the KITTI camera and 1241 x 376 (its map is the identity), fields overridden: src_w / src_h, and cams = two dicts
    with any of K (4), D (up to 8), R (3 x 3 or 9) and P (4)"""
    p = RectifyParams()
    load_library().vslam_default_rectify_params(C.byref(p))
    if src_w is not None:
        p.src_w = int(src_w)
    if src_h is not None:
        p.src_h = int(src_h)
    for s, cam in enumerate(cams or ()):
        for name, vals in cam.items():
            arr = getattr(p.cam[s], name)
            vals = np.asarray(vals, np.float64).ravel()
            assert len(vals) <= len(arr), (name, len(vals))
            for i in range(len(arr)):
                arr[i] = float(vals[i]) if i < len(vals) else 0.0
    return p


def rectify_params_check(p, w, h):
    """vslam_rectify_params_check: is the rig admissible for w x h rectified images?  Host arithmetic, needs no GPU.  Raises VslamError naming the field."""
    lib = load_library()
    rc = lib.vslam_rectify_params_check(C.byref(p), w, h)
    if rc != VSLAM_OK:
        raise VslamError("vslam_rectify_params_check failed (%d): %s" % (rc, lib.vslam_last_error().decode()))
    return True


def rectify_build_maps(p, cam, w, h):
    """vslam_rectify_build_maps: (xy (h, w, 2) int16, frac (h, w) uint16) of camera `cam` for w x h rectified images.  Host arithmetic, needs no GPU."""
    lib = load_library()
    xy = np.zeros((max(h, 0), max(w, 0), 2), np.int16); frac = np.zeros((max(h, 0), max(w, 0)), np.uint16)
    rc = lib.vslam_rectify_build_maps(C.byref(p), cam, w, h, xy, frac)
    if rc != VSLAM_OK:
        raise VslamError("vslam_rectify_build_maps failed (%d): %s" % (rc, lib.vslam_last_error().decode()))
    return xy, frac


def default_pose_graph_params(**kw):
    """vslam_pose_graph_default_params (max_iters 50, pcg_max_iters 4000, pcg_tol 1e-10, step_tol 1e-9, lambda_init 1e-4), fields overridden by keyword"""
    p = PoseGraphParams()
    load_library().vslam_pose_graph_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_full_ba_params(**kw):
    """vslam_full_ba_default_params (max_iters 50, pcg_max_iters 4000, pcg_tol 1e-10, step_tol 1e-9, lambda_init 1e-4), fields overridden by keyword"""
    p = FullBAParams()
    load_library().vslam_full_ba_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_project_match_params(**kw):
    """vslam_project_match_default_params (radius_px 15, tau 50, ratio_pct 80, z_min 0.1, z_max 1e4), fields overridden by keyword"""
    p = ProjectMatchParams()
    load_library().vslam_project_match_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _desc(d):
    d = np.ascontiguousarray(d, np.uint8)
    if d.size == 0:
        d = d.reshape(0, 32)
    assert d.ndim == 2 and d.shape[1] == 32, d.shape
    return d


class VO:
    """Device context + the reference's VO / optimisation method names over the C-ABI.

    Host-buffer methods take and return numpy arrays (one call per reference method); `*_dev` methods take raw
    device pointers (ints, e.g. torch.Tensor.data_ptr()) and run batched + asynchronously on the context stream.
    """

    def __init__(self, params=None, device=0, stream=None, **kw):
        self.lib = load_library()
        self.params = params if params is not None else default_params(**kw)
        self._owned = []   # the VoxelMaps, TsdfMaps and PlaceDBs created on this context and not yet closed, in creation order
        h = C.c_void_p()
        rc = self.lib.vslam_create(C.byref(self.params), device, stream or None, C.byref(h))
        if rc != VSLAM_OK:
            raise VslamError("vslam_create failed (%d): %s" % (rc, self.lib.vslam_last_error().decode()))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            for obj in list(self._owned):   # (they belong to the context and go first)
                obj.close()
            self.lib.vslam_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != VSLAM_OK:
            raise VslamError("%s failed (%d): %s" % (what, rc, self.lib.vslam_last_error().decode()))

    def sync(self):
        self._chk(self.lib.vslam_sync(self.h), "vslam_sync")

    @property
    def device_bytes(self):
        return self.lib.vslam_device_bytes(self.h)

    # ------------------------------------------------------------ VO::feature_detection (visual_odometry.cpp:70-94)
    def _img(self, img):
        img = np.ascontiguousarray(img, np.uint8)
        assert img.ndim == 2
        return img

    def feature_detection(self, img):
        img = self._img(img)
        cap = self.params.kp_capacity
        kps = np.zeros(cap, KEYPOINT_DTYPE); desc = np.zeros((cap, 32), np.uint8); n = C.c_int()
        self._chk(self.lib.vslam_feature_detection(self.h, img, img.shape[1], img.shape[0], img.strides[0], kps, desc, cap, C.byref(n)), "vslam_feature_detection")
        return kps[:n.value].copy(), desc[:n.value].copy()

    def orb_detect(self, img):
        img = self._img(img)
        cap = self.params.kp_capacity
        kps = np.zeros(cap, KEYPOINT_DTYPE); n = C.c_int()
        self._chk(self.lib.vslam_orb_detect(self.h, img, img.shape[1], img.shape[0], img.strides[0], kps, cap, C.byref(n)), "vslam_orb_detect")
        return kps[:n.value].copy()

    def adaptive_non_maximal_suppresion(self, kps, num=500):
        kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE).copy()
        buf = np.zeros(max(len(kps), 1), KEYPOINT_DTYPE); buf[:len(kps)] = kps
        n = C.c_int()
        self._chk(self.lib.vslam_anms(self.h, buf, len(kps), num, C.byref(n)), "vslam_anms")
        return buf[:n.value].copy()

    def orb_compute(self, img, kps):
        img = self._img(img)
        kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE).copy()
        buf = np.zeros(max(len(kps), 1), KEYPOINT_DTYPE); buf[:len(kps)] = kps
        desc = np.zeros((max(len(kps), 1), 32), np.uint8); n = C.c_int()
        self._chk(self.lib.vslam_orb_compute(self.h, img, img.shape[1], img.shape[0], img.strides[0], buf, len(kps), desc, C.byref(n)), "vslam_orb_compute")
        return buf[:n.value].copy(), desc[:n.value].copy()

    def feature_detection_dev(self, d_imgs, img_bytes, pitch, B, d_kps, d_desc, d_count):
        self._chk(self.lib.vslam_feature_detection_dev(self.h, d_imgs, img_bytes, pitch, B, d_kps, d_desc, d_count), "vslam_feature_detection_dev")

    def orb_level(self, item, level, blurred):
        """one level of the (blurred) pyramid of image `item` of the most recent ORB launch (diagnostic)"""
        w, h = C.c_int(0), C.c_int(0)
        buf = np.zeros((self.params.img_h, (self.params.img_w + 63) & ~63), np.uint8)
        self._chk(self.lib.vslam_orb_level(self.h, item, level, bool(blurred), buf, buf.strides[0], buf.shape[0], C.byref(w), C.byref(h)), "vslam_orb_level")
        return buf[:h.value, :w.value].copy()

    def orb_status(self, B):
        st = np.zeros(B, np.int32)
        self._chk(self.lib.vslam_orb_status_dev(self.h, B, st), "vslam_orb_status_dev")
        return st

    def orb_anms_path(self, B):
        """per image of the last ANMS launch: 0 = no ANMS, 1 = capped radius walk accepted, 2 = its check failed and the stopped walks were finished,
        3 = uncapped walk (set_tuning(anms_cap=0))"""
        st = np.zeros(B, np.int32)
        self._chk(self.lib.vslam_orb_anms_path_dev(self.h, B, st), "vslam_orb_anms_path_dev")
        return st

    # ------------------------------------------------------------ VO::feature_matching (visual_odometry.cpp:219-251)
    def feature_matching(self, descriptors_1, descriptors_2, frame_gap=1.0, gate=True):
        q, t = _desc(descriptors_1), _desc(descriptors_2)
        out = np.zeros(max(len(q), 1), DMATCH_DTYPE); n = C.c_int()
        self._chk(self.lib.vslam_feature_matching(self.h, q, len(q), t, len(t), frame_gap, gate, out, C.byref(n)), "vslam_feature_matching")
        return out[:n.value].copy()

    def feature_matching_subset_dev(self, d_q, q_stride, d_nq, d_qsel, d_nqsel, sel_cap, d_t, t_stride, d_nt, d_gap, gate, B, max_rows, d_out, out_cap, d_nout):
        """feature_matching_dev on the query rows d_qsel[b][0 .. d_nqsel[b]) (ascending) of every item; queryIdx = the original row.  Semantics in include/vslam_hip.h."""
        self._chk(self.lib.vslam_feature_matching_subset_dev(self.h, d_q, q_stride, d_nq, d_qsel, d_nqsel, sel_cap, d_t, t_stride, d_nt, d_gap, gate, B, max_rows,
                                                             d_out, out_cap, d_nout), "vslam_feature_matching_subset_dev")

    def feature_matching_pairs_dev(self, d_q, q_stride, d_nq, d_qsel, d_nqsel, sel_cap, d_qitem, n_qitems, d_t, t_stride, d_nt, d_gap, gate, B, max_rows, d_out,
                                   out_cap, d_nout):
        """feature_matching_subset_dev with item b's query side taken from block d_qitem[b] of n_qitems (< 0: no match for the item).  include/vslam_hip.h."""
        self._chk(self.lib.vslam_feature_matching_pairs_dev(self.h, d_q, q_stride, d_nq, d_qsel, d_nqsel, sel_cap, d_qitem, n_qitems, d_t, t_stride, d_nt, d_gap,
                                                            gate, B, max_rows, d_out, out_cap, d_nout), "vslam_feature_matching_pairs_dev")

    def feature_matching_dev(self, d_q, q_stride, d_nq, d_t, t_stride, d_nt, d_gap, gate, B, max_rows, d_out, out_cap, d_nout):
        self._chk(self.lib.vslam_feature_matching_dev(self.h, d_q, q_stride, d_nq, d_t, t_stride, d_nt, d_gap, gate, B, max_rows, d_out, out_cap,
                                                      d_nout), "vslam_feature_matching_dev")

    # ------------------------------------------------------------ VO::disparity_map (StereoSGBM + convertTo 1/16)
    def disparity_map(self, left, right, return_i16=False, sgbm=None):
        """visual_odometry.cpp:159-174.  Returns the f32 disparity map (invalid = -1); with return_i16 also the CV_16S
        map after median/speckle filtering and the raw SGBM output before them.  sgbm: the StereoSGBM set (an SgbmParams, a dict of
        its fields or a tuple in field order); None = the reference's."""
        left = np.ascontiguousarray(left, np.uint8); right = np.ascontiguousarray(right, np.uint8)
        assert left.ndim == 2 and left.shape == right.shape
        h, w = left.shape
        out = np.zeros((h, w), np.float32)
        i16 = np.zeros((h, w), np.int16) if return_i16 else None
        raw = np.zeros((h, w), np.int16) if return_i16 else None
        if sgbm is None:
            self._chk(self.lib.vslam_disparity_map(self.h, left, right, w, h, w, out, i16, raw), "vslam_disparity_map")
        else:
            self._chk(self.lib.vslam_disparity_map_ex(self.h, left, right, w, h, w, C.byref(_sgbm_params(sgbm)), out, i16, raw), "vslam_disparity_map_ex")
        return (out, i16, raw) if return_i16 else out

    def disparity_map_dev(self, d_left, d_right, img_stride_bytes, pitch, w, h, B, d_disp, d_i16=None, d_raw=None, sgbm=None):
        if sgbm is None:
            self._chk(self.lib.vslam_disparity_map_dev(self.h, d_left, d_right, img_stride_bytes, pitch, w, h, B, d_disp, d_i16, d_raw), "vslam_disparity_map_dev")
        else:
            self._chk(self.lib.vslam_disparity_map_ex_dev(self.h, d_left, d_right, img_stride_bytes, pitch, w, h, B, C.byref(_sgbm_params(sgbm)), d_disp, d_i16, d_raw),
                      "vslam_disparity_map_ex_dev")

    # ------------------------------------------------------------ rectification: raw pairs -> rectified pairs (no counterpart in the reference)
    def rectify_set(self, params):
        """check the rig, build both maps for the context's image size and upload them (vslam_rectify_set)"""
        self._chk(self.lib.vslam_rectify_set(self.h, C.byref(params)), "vslam_rectify_set")

    def rectify_set_maps(self, cam, xy, frac, src_w, src_h):
        """a caller's own maps for camera `cam`: xy (img_h, img_w, 2) int16, frac (img_h, img_w) uint16, for src_w x src_h raw images"""
        xy = np.ascontiguousarray(xy, np.int16); frac = np.ascontiguousarray(frac, np.uint16)
        assert xy.shape == (self.params.img_h, self.params.img_w, 2) and frac.shape == xy.shape[:2], (xy.shape, frac.shape)
        self._chk(self.lib.vslam_rectify_set_maps(self.h, cam, xy, frac, src_w, src_h), "vslam_rectify_set_maps")

    def rectify(self, img, cam):
        """one raw image of camera `cam` -> the rectified img_h x img_w image (host buffers; the batched call's kernel)"""
        img = self._img(img)
        out = np.zeros((self.params.img_h, self.params.img_w), np.uint8)
        self._chk(self.lib.vslam_rectify(self.h, cam, img, img.strides[0], out, out.strides[0]), "vslam_rectify")
        return out

    def rectify_dev(self, d_src_left, d_src_right, src_img_bytes, src_pitch, B, d_dst_left, d_dst_right, dst_img_bytes, dst_pitch):
        """B raw pairs -> B rectified pairs, device-resident, asynchronous; a side whose two pointers are None is skipped (include/vslam_hip.h)"""
        self._chk(self.lib.vslam_rectify_dev(self.h, d_src_left, d_src_right, src_img_bytes, src_pitch, B, d_dst_left, d_dst_right, dst_img_bytes, dst_pitch),
                  "vslam_rectify_dev")

    def set_tuning(self, **kw):
        """kernel-choice overrides of this context, e.g. set_tuning(sgbm_fwd_min=1, sgbm_fw_rows=32); -1 = library default"""
        for k, v in kw.items():
            self._chk(self.lib.vslam_set_tuning(self.h, k.encode(), v), "vslam_set_tuning")

    def sgbm_status(self):
        """status word of the most recent disparity_map_dev launch (synchronises): 0, or raises VslamError"""
        st = C.c_int32(0)
        self._chk(self.lib.vslam_sgbm_status_dev(self.h, C.byref(st)), "vslam_sgbm_status_dev")
        return st.value

    # ------------------------------------------------------------ Frame::find_3d / VO::set_ref_3d_position
    def find_3d_disparity(self, kps, disparity, T_c_w):
        kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE); disparity = np.ascontiguousarray(disparity, np.float32)
        T = np.ascontiguousarray(T_c_w, np.float64); n = len(kps)
        xyz = np.zeros((max(n, 1), 3), np.float32); valid = np.zeros(max(n, 1), np.uint8); rel = np.zeros(max(n, 1), np.uint8)
        self._chk(self.lib.vslam_find_3d_disparity(self.h, kps, n, disparity, disparity.shape[1], disparity.shape[0],
                                                   disparity.shape[1], T, xyz, valid, rel, None), "vslam_find_3d_disparity")
        return xyz[:n], valid[:n], rel[:n]

    def find_3d_disparity_dev(self, d_kps, d_n, kp_capacity, B, d_disp, w, h, d_T, d_xyz, d_valid, d_rel):
        self._chk(self.lib.vslam_find_3d_disparity_dev(self.h, d_kps, d_n, kp_capacity, B, d_disp, w, h, d_T, d_xyz, d_valid, d_rel),
                  "vslam_find_3d_disparity_dev")

    def triangulate(self, uvL, uvR, T_c_w):
        uvL = np.ascontiguousarray(uvL, np.float32).reshape(-1, 2); uvR = np.ascontiguousarray(uvR, np.float32).reshape(-1, 2)
        T = np.ascontiguousarray(T_c_w, np.float64); n = len(uvL)
        xyz = np.zeros((max(n, 1), 3), np.float32); valid = np.zeros(max(n, 1), np.uint8); rel = np.zeros(max(n, 1), np.uint8)
        self._chk(self.lib.vslam_triangulate(self.h, uvL, uvR, n, T, xyz, valid, rel, None), "vslam_triangulate")
        return xyz[:n], valid[:n], rel[:n]

    def triangulate_dev(self, d_uvL, d_uvR, d_n, capacity, B, d_T, d_xyz, d_valid, d_rel):
        self._chk(self.lib.vslam_triangulate_dev(self.h, d_uvL, d_uvR, d_n, capacity, B, d_T, d_xyz, d_valid, d_rel), "vslam_triangulate_dev")

    def gather_matched_uv_dev(self, d_kpsQ, d_kpsT, kp_cap, d_matches, d_nmatch, match_cap, B, d_uvQ, d_uvT):
        self._chk(self.lib.vslam_gather_matched_uv_dev(self.h, d_kpsQ, d_kpsT, kp_cap, d_matches, d_nmatch, match_cap, B, d_uvQ, d_uvT),
                  "vslam_gather_matched_uv_dev")

    # ------------------------------------------------------------ VO::motion_estimation (north_star motion-only stage)
    def motion_estimation_ransac(self, xyz_w, uv, T_init=None, max_iters=100, reproj_err=4.0, confidence=0.99, lm_iters=0):
        """VO::motion_estimation's pose stage (cv::solvePnPRansac(..., false, 100, 4.0, 0.99), visual_odometry.cpp:277): EPnP per
        5-point hypothesis, no pose guess is consumed (T_init only pre-fills the output, which stays untouched on failure).
        lm_iters = 0: the best RANSAC model itself (OpenCV 3.2.0, the reference's pinned version); > 0: refined on the inliers (3.4.2+).
        Returns (T, inlier mask, n_inliers, iterations evaluated); n_inliers == 0 means no model was found."""
        xyz = np.ascontiguousarray(xyz_w, np.float32).reshape(-1, 3); uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        T = np.array([0, 0, 0, 1, 0, 0, 0], np.float64) if T_init is None else np.ascontiguousarray(T_init, np.float64).copy(); n = len(xyz)
        inl = np.zeros(max(n, 1), np.uint8); ni = C.c_int(); it = C.c_int()
        self._chk(self.lib.vslam_pnp_ransac(self.h, xyz, uv, n, T, max_iters, reproj_err, confidence,
                                            lm_iters, inl, C.byref(ni), C.byref(it)), "vslam_pnp_ransac")
        return T, inl[:n], ni.value, it.value

    def motion_estimation_ransac_models(self, xyz_w, uv, max_iters=100, reproj_err=4.0, confidence=0.99, lm_iters=0):
        """diagnostic form: (T, mask, n_inliers, iterations, models (max_iters, 12) [R | t], counts (max_iters,))"""
        xyz = np.ascontiguousarray(xyz_w, np.float32).reshape(-1, 3); uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        T = np.array([0, 0, 0, 1, 0, 0, 0], np.float64); n = len(xyz)
        inl = np.zeros(max(n, 1), np.uint8); ni = C.c_int(); it = C.c_int()
        models = np.zeros((max_iters, 12)); counts = np.zeros(max_iters, np.int32)
        self._chk(self.lib.vslam_pnp_ransac_models(self.h, xyz, uv, n, T, max_iters, reproj_err, confidence,
                                                   lm_iters, inl, C.byref(ni), C.byref(it), models, counts), "vslam_pnp_ransac_models")
        return T, inl[:n], ni.value, it.value, models, counts

    def motion_estimation(self, xyz_w, uv, T_guess, iters=10):
        xyz = np.ascontiguousarray(xyz_w, np.float32).reshape(-1, 3); uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        T = np.ascontiguousarray(T_guess, np.float64).copy(); n = len(xyz)
        inl = np.zeros(max(n, 1), np.uint8); ni = C.c_int(); st = LmStats()
        self._chk(self.lib.vslam_pnp_motion_only(self.h, xyz, uv, n, T, iters, inl, C.byref(ni), C.byref(st)), "vslam_pnp_motion_only")
        return T, inl[:n], ni.value, st.as_dict()

    def motion_estimation_dev(self, d_xyz, d_uv, d_n, capacity, B, d_T, iters, d_inlier, d_ninl):
        self._chk(self.lib.vslam_pnp_motion_only_dev(self.h, d_xyz, d_uv, d_n, capacity, B, d_T, iters, d_inlier, d_ninl), "vslam_pnp_motion_only_dev")

    def pnp_ransac_dev(self, d_xyz, d_uv, d_n, capacity, B, d_T, max_iters=100, reproj_err=4.0, confidence=0.99, d_inlier=None, d_ninl=None, d_iters=None):
        """cv::solvePnPRansac(..., 100, 4.0, 0.99) of VO::motion_estimation (visual_odometry.cpp:277) for B device-resident problems"""
        self._chk(self.lib.vslam_pnp_ransac_dev(self.h, d_xyz, d_uv, d_n, capacity, B, d_T, max_iters, reproj_err, confidence, d_inlier, d_ninl,
                                                d_iters), "vslam_pnp_ransac_dev")

    def check_motion_estimation(self, num_inliers, T_c_l, frame_gap):
        T = np.ascontiguousarray(T_c_l, np.float64)
        return bool(self.lib.vslam_check_motion(num_inliers, T, frame_gap))

    # ------------------------------------------------------------ optimize_map / optimize_pose_only (optimization.cpp)
    def _window(self, fn, name, T, xyz, kf_idx, lm_idx, uv, flag_lm, iters, update_poses, update_lms, lm_inlier, with_lms, K=None):
        T = np.ascontiguousarray(T, np.float64).reshape(-1, 7).copy()
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3).copy()
        kf_idx = np.ascontiguousarray(kf_idx, np.int32); lm_idx = np.ascontiguousarray(lm_idx, np.int32)
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        fl = None if flag_lm is None else np.ascontiguousarray(flag_lm, np.int32)
        K4 = None if K is None else np.ascontiguousarray(K, np.float64).reshape(4)  # {fx, fy, cx, cy}; None = context intrinsics
        inl = np.ones(len(xyz), np.uint8) if lm_inlier is None else np.ascontiguousarray(lm_inlier, np.uint8).copy()
        chi2 = np.zeros(len(kf_idx)); thr = C.c_double(); st = LmStats()
        flags = (update_poses, update_lms) if with_lms else (update_poses,)
        self._chk(fn(self.h, len(T), T, len(xyz), xyz, len(kf_idx), kf_idx, lm_idx, uv, K4, fl, iters, *flags, inl, chi2, C.byref(thr), C.byref(st)), name)
        return dict(T=T, xyz=xyz, chi2=chi2, threshold=thr.value, lm_inlier=inl, stats=st.as_dict())

    def optimize_map(self, T, xyz, kf_idx, lm_idx, uv, if_update_map=True, if_update_landmark=False, num_ite=10, flag_lm=None,
                     lm_inlier=None, K=None):
        return self._window(self.lib.vslam_local_ba, "vslam_local_ba", T, xyz, kf_idx, lm_idx, uv, flag_lm, num_ite, if_update_map,
                            if_update_landmark, lm_inlier, True, K)

    def optimize_pose_only(self, T, xyz, kf_idx, lm_idx, uv, if_update_map=True, num_ite=10, flag_lm=None, lm_inlier=None, K=None):
        return self._window(self.lib.vslam_pose_only_window, "vslam_pose_only_window", T, xyz, kf_idx, lm_idx, uv, flag_lm, num_ite,
                            if_update_map, False, lm_inlier, False, K)

    def ba_batch_dev(self, batch, schedule=1, mode=0, iters=10, update_poses=1, update_lms=0):
        self._chk(self.lib.vslam_ba_batch_dev(self.h, C.byref(batch), schedule, mode, iters, update_poses, update_lms), "vslam_ba_batch_dev")

    def set_window_ids(self, d_lm_id, capacity=0):
        """context state: while set, every build_windows*_dev entry also writes each landmark's identity (creating frame x kp_capacity + creating
        keypoint) to d_lm_id (capacity int32, device).  None clears it.  Semantics in include/vslam_hip.h."""
        if d_lm_id is None:
            self._chk(self.lib.vslam_set_window_ids(self.h, None, 0), "vslam_set_window_ids")
            return
        self._chk(self.lib.vslam_set_window_ids(self.h, d_lm_id, capacity), "vslam_set_window_ids")

    def ba_chain_dev(self, batch, d_lm_id, d_kf_frame=None, min_kf=None, d_ran=None):
        """the BA schedule with the windows of every sequence run in order, each from the poses and is_inlier flags the previous one left; the
        sequences of the segment table side by side.  d_kf_frame None: sliding windows; min_kf None: batch.n_kf.  Semantics in include/vslam_hip.h."""
        self._chk(self.lib.vslam_ba_chain_dev(self.h, C.byref(batch), d_lm_id, d_kf_frame, batch.n_kf if min_kf is None else int(min_kf), d_ran),
                  "vslam_ba_chain_dev")

    def build_windows_dev(self, tracks, n_kf, lm_capacity, edge_capacity, batch, d_status):
        """optimize_map's graph build on the device (optimization.cpp:127-214 + visual_odometry.cpp:363-424) for a batch of consecutive
        keyframes; fills the device arrays of `batch` (a BaBatch) and its scalar members"""
        self._chk(self.lib.vslam_build_windows_dev(self.h, C.byref(tracks), n_kf, lm_capacity, edge_capacity, C.byref(batch), d_status),
                  "vslam_build_windows_dev")

    def build_windows_kf_dev(self, tracks, n_kf, policy, near_dist, lm_capacity, edge_capacity, batch, d_kf_frame, d_evicted, d_status):
        """build_windows_dev with a keyframe policy: 0 the sliding window, 1 the reference's culling (Map::remove_keyframe, map.cpp:48-130, on the
        chained poses).  d_kf_frame (n_frames x n_kf int32): the window's frames ascending, -1 unused; d_evicted (n_frames int32): the frame evicted
        at step b, -1 none.  Semantics in include/vslam_hip.h."""
        self._chk(self.lib.vslam_build_windows_kf_dev(self.h, C.byref(tracks), n_kf, policy, near_dist, lm_capacity, edge_capacity, C.byref(batch),
                                                      d_kf_frame, d_evicted, d_status), "vslam_build_windows_kf_dev")

    def build_windows_gated_dev(self, tracks, n_kf, policy, near_dist, d_num_inliers, lm_capacity, edge_capacity, batch, d_kf_frame, d_evicted,
                                d_frame_state, d_status):
        """build_windows_kf_dev with insert_key_frame's keyframe gate (visual_odometry.cpp:353): d_num_inliers (n_frames - 1 int32, item i = frame
        i + 1) and the relative poses decide each frame's state (d_frame_state, n_frames int32: 2 keyframe, 1 tracked, 0 rejected); only keyframes
        create landmarks, record observations and enter the sets (policy 0 oldest evicted, 1 the reference's culling); a non-keyframe step's window
        is empty.  Semantics in include/vslam_hip.h."""
        self._chk(self.lib.vslam_build_windows_gated_dev(self.h, C.byref(tracks), n_kf, policy, near_dist, d_num_inliers, lm_capacity, edge_capacity,
                                                         C.byref(batch), d_kf_frame, d_evicted, d_frame_state, d_status), "vslam_build_windows_gated_dev")

    def set_segments(self, first):
        """declare every following batch of the consecutive-frame entries as independent sequences laid back to back: first = [0, ..., n_frames],
        strictly ascending, segment k = frames [first[k], first[k + 1]) (the rules: include/vslam_hip.h).  None or an empty list clears the table."""
        if first is None or len(first) == 0:
            self._chk(self.lib.vslam_set_segments(self.h, 0, None), "vslam_set_segments")
            return
        first = np.ascontiguousarray(first, np.int32)
        assert first.ndim == 1 and first.size >= 2, first.shape
        self._chk(self.lib.vslam_set_segments(self.h, int(first.size) - 1, first), "vslam_set_segments")

    def chain_poses_dev(self, n_frames, d_T_rel, d_T_c_w):
        """G_0 = identity, G_f = T_rel[f - 1] o G_{f - 1} (n_frames x 7 float64): the window builders' chain"""
        self._chk(self.lib.vslam_chain_poses_dev(self.h, n_frames, d_T_rel, d_T_c_w), "vslam_chain_poses_dev")

    def build_map_pnp_inputs_dev(self, tracks, d_T_c_w, d_input_of_match_prev, d_xyz_w, d_uv, d_n, d_input_of_match, out_capacity, d_status):
        """one refinement pass's pose inputs against the map (VO::motion_estimation, visual_odometry.cpp:260-277): every match out of a feature of frame
        i at its landmark's position in the world of d_T_c_w, links from d_input_of_match_prev (None: pass 0).  Semantics in include/vslam_hip.h."""
        self._chk(self.lib.vslam_build_map_pnp_inputs_dev(self.h, C.byref(tracks), d_T_c_w, d_input_of_match_prev, d_xyz_w, d_uv, d_n, d_input_of_match,
                                                          out_capacity, d_status), "vslam_build_map_pnp_inputs_dev")

    def build_windows_map_dev(self, tracks, d_T_c_w, d_input_of_match, n_kf, policy, near_dist, lm_capacity, edge_capacity, batch, d_kf_frame, d_evicted,
                              d_status):
        """build_windows_kf_dev on the caller's poses and the links of a refinement pass (d_input_of_match None: pass 0).  Semantics in include/vslam_hip.h."""
        self._chk(self.lib.vslam_build_windows_map_dev(self.h, C.byref(tracks), d_T_c_w, d_input_of_match, n_kf, policy, near_dist, lm_capacity,
                                                       edge_capacity, C.byref(batch), d_kf_frame, d_evicted, d_status), "vslam_build_windows_map_dev")

    def gate_states_dev(self, n_frames, d_T, absolute, d_num_inliers, d_frame_state):
        """insert_key_frame's gate per frame (n_frames int32: 2 keyframe, 1 tracked, 0 rejected) from the inlier counts (item i = frame i + 1) and d_T:
        absolute 0 -- the relative poses T_rel (the gated builder's states); 1 -- absolute poses G, T_c_l = G_f o G_{f-1}^-1.  Semantics in include/vslam_hip.h."""
        self._chk(self.lib.vslam_gate_states_dev(self.h, n_frames, d_T, absolute, d_num_inliers, d_frame_state), "vslam_gate_states_dev")

    def build_map_pnp_inputs_gated_dev(self, tracks, d_T_c_w, d_input_of_match_prev, d_frame_state, d_xyz_w, d_uv, d_n, d_input_of_match, out_capacity,
                                       d_status):
        """build_map_pnp_inputs_dev with the gated walk on the previous pass's frame states.  Semantics in include/vslam_hip.h."""
        self._chk(self.lib.vslam_build_map_pnp_inputs_gated_dev(self.h, C.byref(tracks), d_T_c_w, d_input_of_match_prev, d_frame_state, d_xyz_w, d_uv, d_n,
                                                                d_input_of_match, out_capacity, d_status), "vslam_build_map_pnp_inputs_gated_dev")

    def build_map_pnp_inputs_requery_dev(self, tracks, d_T_c_w, d_input_of_match_prev, d_frame_state, d_desc, desc_stride, d_feat, d_nfeat, d_f2f_out,
                                         d_nf2f_out, d_xyz_w, d_uv, d_n, d_input_of_match, out_capacity, d_status):
        """build_map_pnp_inputs_gated_dev with every pair re-matched on the features of its first frame (the reference's query set) between the walk and the
        emit: writes the feature lists, the new frame-to-frame table and the inputs on that table.  Semantics in include/vslam_hip.h."""
        self._chk(self.lib.vslam_build_map_pnp_inputs_requery_dev(self.h, C.byref(tracks), d_T_c_w, d_input_of_match_prev, d_frame_state, d_desc, desc_stride,
                                                                  d_feat, d_nfeat, d_f2f_out, d_nf2f_out, d_xyz_w, d_uv, d_n, d_input_of_match, out_capacity,
                                                                  d_status), "vslam_build_map_pnp_inputs_requery_dev")

    def build_windows_map_gated_dev(self, tracks, d_T_c_w, d_input_of_match, d_frame_state, n_kf, policy, near_dist, lm_capacity, edge_capacity, batch,
                                    d_kf_frame, d_evicted, d_status):
        """build_windows_map_dev with the frame states as an input: the gated windows (empty at a non-keyframe).  Semantics in include/vslam_hip.h."""
        self._chk(self.lib.vslam_build_windows_map_gated_dev(self.h, C.byref(tracks), d_T_c_w, d_input_of_match, d_frame_state, n_kf, policy, near_dist,
                                                             lm_capacity, edge_capacity, C.byref(batch), d_kf_frame, d_evicted, d_status),
                  "vslam_build_windows_map_gated_dev")

    def frame_pairs_dev(self, n_frames, d_frame_state, d_pred, d_gap):
        """every frame's last accepted predecessor (-1: frame 0, or Lost) and the gap to it, from the frame states.  Semantics in include/vslam_hip.h."""
        self._chk(self.lib.vslam_frame_pairs_dev(self.h, n_frames, d_frame_state, d_pred, d_gap), "vslam_frame_pairs_dev")

    def gate_states_pairs_dev(self, n_frames, d_T_c_w, d_pred, d_num_inliers, d_frame_state):
        """gate_states_dev(absolute=1) against the pairing d_pred at the pairs' real gaps, then the Lost scan (state 3).  Semantics in include/vslam_hip.h."""
        self._chk(self.lib.vslam_gate_states_pairs_dev(self.h, n_frames, d_T_c_w, d_pred, d_num_inliers, d_frame_state), "vslam_gate_states_pairs_dev")

    def build_map_pnp_inputs_recover_dev(self, tracks, d_T_c_w, d_input_of_match_prev, d_pred_prev, d_frame_state, d_desc, desc_stride, d_feat, d_nfeat,
                                         d_f2f_out, d_nf2f_out, d_xyz_w, d_uv, d_n, d_input_of_match, out_capacity, d_pred, d_gap, d_status):
        """build_map_pnp_inputs_requery_dev with every frame re-matched from its last accepted predecessor (the reference's failure handling): also
        writes the pairing d_pred / d_gap.  Semantics in include/vslam_hip.h."""
        self._chk(self.lib.vslam_build_map_pnp_inputs_recover_dev(self.h, C.byref(tracks), d_T_c_w, d_input_of_match_prev, d_pred_prev, d_frame_state, d_desc,
                                                                  desc_stride, d_feat, d_nfeat, d_f2f_out, d_nf2f_out, d_xyz_w, d_uv, d_n, d_input_of_match,
                                                                  out_capacity, d_pred, d_gap, d_status), "vslam_build_map_pnp_inputs_recover_dev")

    def build_windows_map_recover_dev(self, tracks, d_T_c_w, d_input_of_match, d_pred, d_frame_state, n_kf, policy, near_dist, lm_capacity, edge_capacity,
                                      batch, d_kf_frame, d_evicted, d_status):
        """build_windows_map_gated_dev on a table built on the pairing d_pred: rejected and Lost frames are dropped.  Semantics in include/vslam_hip.h."""
        self._chk(self.lib.vslam_build_windows_map_recover_dev(self.h, C.byref(tracks), d_T_c_w, d_input_of_match, d_pred, d_frame_state, n_kf, policy,
                                                               near_dist, lm_capacity, edge_capacity, C.byref(batch), d_kf_frame, d_evicted, d_status),
                  "vslam_build_windows_map_recover_dev")

    def build_pnp_inputs_dev(self, d_f2f, d_nf2f, match_cap, d_lr, d_nlr, lr_cap, d_xyz_lr, d_valid_lr, d_kps_cur, kp_cap, B, d_kp2lr,
                             d_xyz_out, d_uv_out, d_nout, out_cap):
        self._chk(self.lib.vslam_build_pnp_inputs_dev(self.h, d_f2f, d_nf2f, match_cap, d_lr, d_nlr, lr_cap, d_xyz_lr, d_valid_lr, d_kps_cur, kp_cap, B,
                                                      d_kp2lr, d_xyz_out, d_uv_out, d_nout, out_cap), "vslam_build_pnp_inputs_dev")

    # ------------------------------------------------------------ dense map: disparities fused into a voxel grid (no counterpart in the reference)
    def voxel_map(self, voxel_size=0.2, log2_capacity=22):
        """an empty VoxelMap of this context: 2^log2_capacity slots of 32 bytes for voxels of voxel_size metres"""
        return VoxelMap(self, voxel_size, log2_capacity)

    def reproject_dev(self, d_disp, w, h, B, d_T, z_min, z_max, step, d_xyz, d_valid):
        """every step-th pixel of B disparity maps through Frame::find_3d at the items' poses: B x ceil(h / step) x ceil(w / step) points and
        their depth-gate flags (z_min < Z < z_max).  Semantics in include/vslam_hip.h."""
        self._chk(self.lib.vslam_reproject_dev(self.h, d_disp, w, h, B, d_T, z_min, z_max, step, d_xyz, d_valid), "vslam_reproject_dev")

    def voxel_insert_points_dev(self, vm, d_xyz, d_valid, d_intensity, n, map_id=0):
        """n f32 points (d_valid / d_intensity uint8 or None) into map map_id of the VoxelMap vm"""
        self._chk(self.lib.vslam_voxel_insert_points_dev(self.h, vm.h, d_xyz, d_valid, d_intensity, n, map_id), "vslam_voxel_insert_points_dev")

    def voxel_fuse_disparity_dev(self, vm, d_disp, d_gray, img_bytes, pitch, w, h, B, d_T, d_map_id, z_min, z_max, step=1):
        """reproject_dev + voxel_insert_points_dev in one pass: item b's valid points into map d_map_id[b] (< 0: skipped), intensity from d_gray (None: 0)"""
        self._chk(self.lib.vslam_voxel_fuse_disparity_dev(self.h, vm.h, d_disp, d_gray, img_bytes, pitch, w, h, B, d_T, d_map_id, z_min, z_max, step),
                  "vslam_voxel_fuse_disparity_dev")

    # ------------------------------------------------------------ surface map: disparities fused into a TSDF (no counterpart in the reference)
    def tsdf_map(self, voxel_size=0.2, trunc_voxels=4, log2_blocks=16):
        """an empty TsdfMap of this context: 2^log2_blocks blocks of 8 x 8 x 8 voxels of voxel_size metres (8 KiB each), truncation trunc_voxels voxels"""
        return TsdfMap(self, voxel_size, trunc_voxels, log2_blocks)

    def tsdf_integrate_dev(self, tm, d_disp, d_gray, img_bytes, pitch, w, h, B, d_T, d_map_id, z_min, z_max, step=1):
        """allocation and integration of B frames into the TsdfMap tm: item b into map d_map_id[b] (< 0: skipped), intensity from d_gray (None: 0)"""
        self._chk(self.lib.vslam_tsdf_integrate_dev(self.h, tm.h, d_disp, d_gray, img_bytes, pitch, w, h, B, d_T, d_map_id, z_min, z_max, step),
                  "vslam_tsdf_integrate_dev")

    def tsdf_render_dev(self, tm, params, V, d_T, d_map_id, d_depth, d_attr=None, d_counts=None):
        """V views of the TsdfMap tm ray-cast by the RENDER rule of include/vslam_hip.h: params a TsdfRenderParams (struct_size is set here), d_depth
        V x h x w f32, d_attr V x h x w x 4 f32 of (nx, ny, nz, intensity) or None, d_counts two uint64 (rays that hit, samples evaluated) or None"""
        params.struct_size = C.sizeof(TsdfRenderParams)
        self._chk(self.lib.vslam_tsdf_render_dev(self.h, tm.h, C.byref(params), V, d_T, d_map_id, d_depth, d_attr, d_counts), "vslam_tsdf_render_dev")

    def voxel_extract_dev(self, vm, map_id, min_count, d_out, d_map_out, capacity, d_n_out):
        """the occupied voxels with count >= min_count of map map_id (-1: all) into d_out (capacity x 32 bytes) / d_map_out; d_n_out (uint64): the full count"""
        self._chk(self.lib.vslam_voxel_extract_dev(self.h, vm.h, map_id, min_count, d_out, d_map_out, capacity, d_n_out), "vslam_voxel_extract_dev")

    # ------------------------------------------------------------ loop closure: place database, score, candidates, verified edges (no counterpart in the reference)
    def place_db(self, rows=None, capacity=4096, with_geometry=True):
        """an empty PlaceDB of this context: `capacity` entries of `rows` descriptor rows (None: the context's anms_num)"""
        return PlaceDB(self, int(self.params.anms_num if rows is None else rows), capacity, with_geometry)

    def place_add_dev(self, db, d_desc, desc_stride, d_n, d_add, d_seq, d_frame, d_kps, d_xyz, d_valid, kp_capacity, B):
        """append the items of a batch whose d_add is non-zero (None: all); returns the id of the first entry added.  Semantics in include/vslam_hip.h."""
        first = C.c_int(-1)
        self._chk(self.lib.vslam_place_add_dev(self.h, db.h, d_desc, desc_stride, d_n, d_add, d_seq, d_frame, d_kps, d_xyz, d_valid, kp_capacity, B,
                                               C.byref(first)), "vslam_place_add_dev")
        return first.value

    def place_score_dev(self, db, q0, nq, tau, min_gap, d_score, ld):
        """the nq x n_entries place-score table (int32, row stride ld) of query entries [q0, q0 + nq): -1 where the pair is not eligible"""
        self._chk(self.lib.vslam_place_score_dev(self.h, db.h, q0, nq, tau, min_gap, d_score, ld), "vslam_place_score_dev")

    def place_select_dev(self, db, q0, nq, d_score, ld, K, min_score, d_cand, d_cand_score):
        """per query the K best eligible entries that reach min_score (descending score, ties to the smaller id; -1 / 0 unused)"""
        self._chk(self.lib.vslam_place_select_dev(self.h, db.h, q0, nq, d_score, ld, K, min_score, d_cand, d_cand_score), "vslam_place_select_dev")

    def place_verify_dev(self, db, q0, nq, d_cand, K, rank, min_inliers, d_T_q_c, d_n_matches, d_n_inliers):
        """matcher + gather + RANSAC pose of every query's rank-`rank` candidate: relative pose, match and inlier counts"""
        self._chk(self.lib.vslam_place_verify_dev(self.h, db.h, q0, nq, d_cand, K, rank, min_inliers, d_T_q_c, d_n_matches, d_n_inliers),
                  "vslam_place_verify_dev")

    # ------------------------------------------------------------ pose-graph optimisation (no counterpart in the reference)
    def pose_graph_dev(self, graph, params=None, d_T_out=None, d_stats=None):
        """vslam_pose_graph_dev on a PoseGraphBatch of device pointers: the optimised poses into d_T_out (total_nodes x 7 doubles; may be graph.d_T), the
        per-graph vslam_pose_graph_stats into d_stats (or None).  Asynchronous.  Semantics in include/vslam_hip.h."""
        graph.struct_size = C.sizeof(PoseGraphBatch)
        self._chk(self.lib.vslam_pose_graph_dev(self.h, C.byref(graph), None if params is None else C.byref(params), d_T_out, d_stats), "vslam_pose_graph_dev")

    def pose_graph_status(self, n_graphs):
        """the status words (PG_* bits) of the graphs of the most recent pose_graph_dev call; synchronises"""
        st = np.zeros(n_graphs, np.int32)
        self._chk(self.lib.vslam_pose_graph_status_dev(self.h, n_graphs, st), "vslam_pose_graph_status_dev")
        return st

    def optimize_pose_graph(self, T, node_off, edges, fixed=None, active=None, params=None, **kw):
        """A batch of pose graphs from numpy arrays: T (total_nodes, 7) poses T_c_w, node_off (G + 1), edges = dict(off (G + 1), i, j (graph-local
        node ids), Z (E, 7), w (E, 6)); fixed (total_nodes) and active (E) optional byte masks; params a PoseGraphParams, or its fields by keyword.
        Uploads, runs, downloads.  Returns dict(T (total_nodes, 7), stats (G records of POSE_GRAPH_STATS_DTYPE), edge_chi2 (E))."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        T = np.ascontiguousarray(T, np.float64).reshape(-1, 7)
        node_off = np.ascontiguousarray(node_off, np.int32); edge_off = np.ascontiguousarray(edges["off"], np.int32)
        ei = np.ascontiguousarray(edges["i"], np.int32); ej = np.ascontiguousarray(edges["j"], np.int32)
        Z = np.ascontiguousarray(edges["Z"], np.float64).reshape(-1, 7); w = np.ascontiguousarray(edges["w"], np.float64).reshape(-1, 6)
        G, N, E = len(node_off) - 1, len(T), len(ei)
        assert G >= 0 and len(edge_off) == G + 1 and len(ej) == E and len(Z) == E and len(w) == E
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        t = dict(node_off=up(node_off), edge_off=up(edge_off), T=up(T), ei=up(ei), ej=up(ej), Z=up(Z), w=up(w),
                 out=torch.zeros((N, 7), dtype=torch.float64, device=dev), chi2=torch.zeros(E, dtype=torch.float64, device=dev),
                 stats=torch.zeros(max(G, 1) * POSE_GRAPH_STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev))
        if fixed is not None:
            t["fixed"] = up(np.ascontiguousarray(fixed, np.uint8)); assert len(t["fixed"]) == N
        if active is not None:
            t["active"] = up(np.ascontiguousarray(active, np.uint8)); assert len(t["active"]) == E
        ptr = lambda k: t[k].data_ptr() if k in t and t[k].numel() else None
        g = PoseGraphBatch(n_graphs=G, total_nodes=N, total_edges=E, d_node_off=t["node_off"].data_ptr(), d_edge_off=t["edge_off"].data_ptr(), d_T=ptr("T"),
                      d_fixed=ptr("fixed"), d_edge_i=ptr("ei"), d_edge_j=ptr("ej"), d_edge_Z=ptr("Z"), d_edge_w=ptr("w"), d_edge_active=ptr("active"),
                      d_edge_chi2=ptr("chi2"))
        if params is None and kw:
            params = default_pose_graph_params(**kw)
        torch.cuda.synchronize()   # (the uploads are done before the context stream reads them)
        self.pose_graph_dev(g, params, ptr("out"), t["stats"].data_ptr())
        self.sync()
        stats = t["stats"].cpu().numpy().view(POSE_GRAPH_STATS_DTYPE)[:G].copy()
        return dict(T=t["out"].cpu().numpy(), stats=stats, edge_chi2=t["chi2"].cpu().numpy())

    # ------------------------------------------------------------ full bundle adjustment (no counterpart in the reference)
    def full_ba_dev(self, ba, params=None, d_T_out=None, d_xyz_out=None, d_stats=None):
        """vslam_full_ba_dev on a FullBABatch of device pointers: the optimised poses into d_T_out (total_kfs x 7 doubles; may be ba.d_T), the points into
        d_xyz_out (total_lms x 3 doubles; may be ba.d_xyz), the per-problem vslam_full_ba_stats into d_stats (or None).  Asynchronous.  Semantics in
        include/vslam_hip.h."""
        ba.struct_size = C.sizeof(FullBABatch)
        self._chk(self.lib.vslam_full_ba_dev(self.h, C.byref(ba), None if params is None else C.byref(params), d_T_out, d_xyz_out, d_stats), "vslam_full_ba_dev")

    def full_ba_status(self, n_problems):
        """the status words (FBA_* bits) of the problems of the most recent full_ba_dev call; synchronises"""
        st = np.zeros(n_problems, np.int32)
        self._chk(self.lib.vslam_full_ba_status_dev(self.h, n_problems, st), "vslam_full_ba_status_dev")
        return st

    def full_ba(self, T, xyz, offsets, obs, edges=None, fixed=None, K4=None, bf=None, huber_delta=0.0, params=None, **kw):
        """A batch of full bundle adjustment problems from numpy arrays: T (total_kfs, 7) poses T_c_w, xyz (total_lms, 3), offsets = dict(kf, lm, obs,
        edge: G + 1 each), obs = dict(kf, lm (problem-local ids, sorted by landmark inside a problem), uv (O, 2), disp (O) or None, active (O) or
        None), edges = dict(i, j, Z (E, 7), w (E, 6), active or None) or None; fixed (total_kfs) optional; K4 = (fx, fy, cx, cy) and bf default to
        the context's camera; params a FullBAParams, or its fields by keyword.  Uploads, runs, downloads.  Returns dict(T, xyz, stats (G records
        of FULL_BA_STATS_DTYPE), obs_chi2 (O))."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        T = np.ascontiguousarray(T, np.float64).reshape(-1, 7); xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        off = {k: np.ascontiguousarray(offsets[k], np.int32) for k in ("kf", "lm", "obs", "edge")}
        G = len(off["kf"]) - 1
        assert G >= 0 and all(len(v) == G + 1 for v in off.values())
        okf = np.ascontiguousarray(obs["kf"], np.int32); olm = np.ascontiguousarray(obs["lm"], np.int32)
        uv = np.ascontiguousarray(obs["uv"], np.float32).reshape(-1, 2)
        N, M, O = len(T), len(xyz), len(okf)
        assert len(olm) == O and len(uv) == O
        e = edges if edges is not None else dict(i=np.zeros(0, np.int32), j=np.zeros(0, np.int32), Z=np.zeros((0, 7)), w=np.zeros((0, 6)))
        ei = np.ascontiguousarray(e["i"], np.int32); ej = np.ascontiguousarray(e["j"], np.int32)
        Z = np.ascontiguousarray(e["Z"], np.float64).reshape(-1, 7); w = np.ascontiguousarray(e["w"], np.float64).reshape(-1, 6)
        E = len(ei)
        assert len(ej) == E and len(Z) == E and len(w) == E
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        t = dict(kf_off=up(off["kf"]), lm_off=up(off["lm"]), obs_off=up(off["obs"]), edge_off=up(off["edge"]), T=up(T), xyz=up(xyz), okf=up(okf), olm=up(olm),
                 uv=up(uv), ei=up(ei), ej=up(ej), Z=up(Z), w=up(w), T_out=torch.zeros((N, 7), dtype=torch.float64, device=dev),
                 xyz_out=torch.zeros((M, 3), dtype=torch.float64, device=dev), chi2=torch.zeros(O, dtype=torch.float64, device=dev),
                 stats=torch.zeros(max(G, 1) * FULL_BA_STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev))
        for key, src, n, dt in (("disp", obs.get("disp"), O, np.float32), ("oact", obs.get("active"), O, np.uint8), ("eact", e.get("active"), E, np.uint8),
                                ("fixed", fixed, N, np.uint8)):
            if src is not None:
                t[key] = up(np.ascontiguousarray(src, dt)); assert len(t[key]) == n, key
        ptr = lambda k: t[k].data_ptr() if k in t and t[k].numel() else None
        cam = list(self.params.cam)
        K4 = cam[:4] if K4 is None else [float(v) for v in K4]
        ba = FullBABatch(n_problems=G, total_kfs=N, total_lms=M, total_obs=O, total_edges=E, d_kf_off=t["kf_off"].data_ptr(), d_lm_off=t["lm_off"].data_ptr(),
                         d_obs_off=t["obs_off"].data_ptr(), d_edge_off=t["edge_off"].data_ptr(), d_T=ptr("T"), d_fixed=ptr("fixed"), d_xyz=ptr("xyz"),
                         d_obs_kf=ptr("okf"), d_obs_lm=ptr("olm"), d_obs_uv=ptr("uv"), d_obs_disp=ptr("disp"), d_obs_active=ptr("oact"), d_obs_chi2=ptr("chi2"),
                         d_edge_i=ptr("ei"), d_edge_j=ptr("ej"), d_edge_Z=ptr("Z"), d_edge_w=ptr("w"), d_edge_active=ptr("eact"),
                         K4=(C.c_double * 4)(*K4), bf=float(cam[0] * cam[4] if bf is None else bf), huber_delta=float(huber_delta))
        if params is None and kw:
            params = default_full_ba_params(**kw)
        torch.cuda.synchronize()   # (the uploads are done before the context stream reads them)
        self.full_ba_dev(ba, params, ptr("T_out"), ptr("xyz_out"), t["stats"].data_ptr())
        self.sync()
        stats = t["stats"].cpu().numpy().view(FULL_BA_STATS_DTYPE)[:G].copy()
        return dict(T=t["T_out"].cpu().numpy(), xyz=t["xyz_out"].cpu().numpy(), stats=stats, obs_chi2=t["chi2"].cpu().numpy())

    # ------------------------------------------------------------ match by projection (re-observed and fused landmarks)
    def project_match_dev(self, batch, params=None, n_cand=True, fill=None):
        """vslam_project_match_dev on a ProjectMatchBatch of device pointers (inputs; K4 None = the context's camera, else four numbers).  The outputs are
        allocated here on the current device, sentinel-free, and returned as torch tensors: dict(match int32, dist int32, status uint8, n_cand int32 or
        None), n_landmarks each; pointers already set in the batch's output fields are used instead and come back as None.  params a
        ProjectMatchParams or None for the defaults; fill = a value the allocated outputs hold before the call (what no item writes keeps it).
        Asynchronous on the context stream.  Semantics in include/vslam_hip.h."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        L = max(int(batch.n_landmarks), 0)
        out = {}
        for field, key, dt in (("d_match", "match", torch.int32), ("d_dist", "dist", torch.int32), ("d_status", "status", torch.uint8), ("d_n_cand", "n_cand", torch.int32)):
            out[key] = None
            if getattr(batch, field) is None and (key != "n_cand" or n_cand):
                out[key] = (torch.empty(max(L, 1), dtype=dt, device=dev) if fill is None else torch.full((max(L, 1),), fill, dtype=dt, device=dev))[:L]
                setattr(batch, field, out[key].data_ptr())
        batch.struct_size = C.sizeof(ProjectMatchBatch)
        if any(v is not None for v in out.values()):
            torch.cuda.current_stream().synchronize()   # (the allocations exist before the context stream writes them)
        self._chk(self.lib.vslam_project_match_dev(self.h, C.byref(batch), None if params is None else C.byref(params)), "vslam_project_match_dev")
        return out

    def project_match(self, lm_off, item_img, item_T, lm_xyz, lm_desc_row, src_desc, kps, desc, n, K4=None, params=None, fill=None, **kw):
        """Match by projection from numpy arrays: lm_off (n_items + 1), item_img (n_items), item_T (n_items, 7), lm_xyz (L, 3), lm_desc_row (L), src_desc
        (rows, 32) uint8 or None for desc itself, kps (B, kp_capacity) KEYPOINT_DTYPE, desc (B, kp_capacity, 32) uint8, n (B).  params a
        ProjectMatchParams, or its fields by keyword.  Uploads, runs, downloads: dict(match, dist, n_cand, status) numpy arrays."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE); desc = np.ascontiguousarray(desc, np.uint8)
        B, cap = kps.shape
        assert desc.shape == (B, cap, 32)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        pad = lambda t: t if t.numel() else torch.zeros(16, dtype=t.dtype, device=dev)
        t = dict(off=up(np.asarray(lm_off, np.int32)), img=up(np.asarray(item_img, np.int32)), T=up(np.asarray(item_T, np.float64).reshape(-1, 7)),
                 xyz=pad(up(np.asarray(lm_xyz, np.float64).reshape(-1, 3))), row=pad(up(np.asarray(lm_desc_row, np.int32))), kps=up(kps.view(np.uint8)), desc=up(desc),
                 n=up(np.asarray(n, np.int32)))
        t["src"] = t["desc"] if src_desc is None else pad(up(np.ascontiguousarray(src_desc, np.uint8).reshape(-1, 32)))
        L = len(np.asarray(lm_desc_row))
        rows = B * cap if src_desc is None else len(np.asarray(src_desc).reshape(-1, 32))
        k4 = None if K4 is None else (C.c_double * 4)(*[float(v) for v in K4])
        batch = ProjectMatchBatch(n_items=len(t["img"]), n_landmarks=L, B=B, kp_capacity=cap, n_src_rows=rows, d_lm_off=t["off"].data_ptr(),
                                  d_item_img=t["img"].data_ptr(), d_item_T=t["T"].data_ptr(), d_lm_xyz=t["xyz"].data_ptr(), d_lm_desc_row=t["row"].data_ptr(),
                                  d_src_desc=t["src"].data_ptr(), d_kps=t["kps"].data_ptr(), d_desc=t["desc"].data_ptr(), desc_stride_bytes=0, d_n=t["n"].data_ptr(),
                                  K4=None if k4 is None else C.cast(k4, C.POINTER(C.c_double)))
        if params is None and kw:
            params = default_project_match_params(**kw)
        torch.cuda.synchronize()   # (the uploads are done before the context stream reads them)
        out = self.project_match_dev(batch, params, fill=fill)
        self.sync()
        return {k: v.cpu().numpy() for k, v in out.items()}

    def profile_enable(self, on=True):
        self._chk(self.lib.vslam_profile_enable(self.h, on), "vslam_profile_enable")

    def profile_read(self):
        """{kernel family: (total_ms, launches, calls)} since the last read; synchronises the stream"""
        buf = (KernelTime * 32)(); n = C.c_int()
        self._chk(self.lib.vslam_profile_read(self.h, buf, 32, C.byref(n)), "vslam_profile_read")
        return {buf[i].name.decode(): (buf[i].total_ms, buf[i].launches, buf[i].calls) for i in range(n.value)}

    def profile_intervals(self, cap=4096):
        """[(kernel family, t0_ms, t1_ms)] of the brackets recorded since the last read, on the device's time axis (comparable across the contexts of one device)"""
        buf = (StageInterval * cap)(); n = C.c_int()
        self._chk(self.lib.vslam_profile_intervals(self.h, buf, cap, C.byref(n)), "vslam_profile_intervals")
        return [(buf[i].name.decode(), buf[i].t0_ms, buf[i].t1_ms) for i in range(n.value)]

    def hbm_copy_probe(self, nbytes=1 << 30, reps=5):
        """GB/s (read + write) of a float4 streaming copy on this GPU, timed on the context stream"""
        g = C.c_double()
        self._chk(self.lib.vslam_hbm_copy_probe(self.h, nbytes, reps, C.byref(g)), "vslam_hbm_copy_probe")
        return g.value

    def hbm_copy_probe_best(self, nbytes=1 << 30, reps=5):
        """every shape of the streaming copy (csrc/geom_kernels.hip): {"gbs": best GB/s, "variant": its description, "all": {name: GB/s}}"""
        res = {}
        for v in range(self.lib.vslam_hbm_copy_probe_variants()):
            g = C.c_double(); name = C.create_string_buffer(64)
            self._chk(self.lib.vslam_hbm_copy_probe_variant(self.h, nbytes, reps, v, C.byref(g), name), "vslam_hbm_copy_probe_variant")
            res[name.value.decode()] = round(g.value, 1)
        best = max(res, key=res.get)
        return {"gbs": res[best], "variant": best, "bytes": int(nbytes), "all": res}

    def ba_status(self, n_windows):
        st = np.zeros(n_windows, np.int32)
        self._chk(self.lib.vslam_ba_status_dev(self.h, n_windows, st), "vslam_ba_status_dev")
        return st

    def edge_jacobians(self, xyz_w, uv, T_c_w, K=None):
        """residual / Jacobians of EdgeProjection and PoseOnlyEdgeProjection (optimization.cpp:41-101) as the LM kernels' device functions evaluate
        them: {err (n, 2), J_pose (n, 2, 6), J_point (n, 2, 3), chi2 (n), huber_w (n)} for n world points seen through one pose"""
        xyz = np.ascontiguousarray(xyz_w, np.float32); z = np.ascontiguousarray(uv, np.float32); T = np.ascontiguousarray(T_c_w, np.float64)
        n = len(xyz)
        out = dict(err=np.zeros((n, 2)), J_pose=np.zeros((n, 2, 6)), J_point=np.zeros((n, 2, 3)), chi2=np.zeros(n), huber_w=np.zeros(n))
        K4 = None if K is None else np.ascontiguousarray(K, np.float64)
        self._chk(self.lib.vslam_edge_jacobians(self.h, n, xyz, z, T, K4, out["err"], out["J_pose"], out["J_point"], out["chi2"], out["huber_w"]),
                  "vslam_edge_jacobians")
        return out

    def ba_deferred(self, n_windows):
        """per window of the last BA launch: 0 = ba_resident_kernel ran it, 1 = lm_window_kernel did"""
        st = np.zeros(n_windows, np.int32)
        self._chk(self.lib.vslam_ba_deferred_dev(self.h, n_windows, st), "vslam_ba_deferred_dev")
        return st

    def ba_schedule_passes(self, n_windows):
        """optimize_map passes the last schedule executed per window (3, or 1 / 2 when a pass flagged nothing new and was continued instead of repeated)"""
        st = np.zeros(n_windows, np.int32)
        self._chk(self.lib.vslam_ba_schedule_passes_dev(self.h, n_windows, st), "vslam_ba_schedule_passes_dev")
        return st


class _Owned:
    """What VoxelMap, TsdfMap and PlaceDB share: an object that a VO creates, owns and closes with itself.  A subclass names its four entry points
    in _CREATE, _DESTROY, _CLEAR and _STATS, its stats struct in _STATS_T, and hands _create() the arguments of its create call."""

    def _create(self, vo, *args):
        self.vo = vo
        h = C.c_void_p()
        vo._chk(getattr(vo.lib, self._CREATE)(vo.h, *args, C.byref(h)), self._CREATE)
        self.h = h
        vo._owned.append(self)

    def close(self):
        if getattr(self, "h", None):
            getattr(self.vo.lib, self._DESTROY)(self.h)
            self.h = None
            self.vo._owned.remove(self)

    def clear(self):
        """empty again, counters zeroed; the two maps clear asynchronously on the context stream"""
        self.vo._chk(getattr(self.vo.lib, self._CLEAR)(self.h), self._CLEAR)

    def stats(self):
        """the fields of the object's stats struct as a dict (see the class); the two maps synchronise"""
        st = self._STATS_T(); st.struct_size = C.sizeof(self._STATS_T)
        self.vo._chk(getattr(self.vo.lib, self._STATS)(self.h, C.byref(st)), self._STATS)
        return st.as_dict()


def _read_lists(vo, call, lists, capacities=None):
    """Reads back the counted, capacity-limited lists a device entry writes.  lists: per list its parallel arrays as (torch dtype, row shape, fill);
    call(*args) runs the entry with, per list, its arrays' device pointers and its capacity, then the pointer to one uint64 count per list -- the
    order the extract, blocks and mesh entries take them in.  capacities None: a first pass without arrays (null pointers, capacity 0) counts.
    Returns (per list its arrays as numpy, cut to min(count, capacity) rows; the full counts)."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    d_n = torch.zeros(len(lists), dtype=torch.int64, device=dev)

    def run(bufs, caps):
        args = []
        for arrays, cap in zip(bufs, caps):
            args += [None if a is None else a.data_ptr() for a in arrays] + [cap]
        torch.cuda.synchronize(dev)   # (the buffers are ready before the context stream writes them)
        call(*args, d_n.data_ptr())
        vo.sync()
        return [int(c) for c in d_n.cpu().tolist()]

    if capacities is None:
        capacities = [max(c, 1) for c in run([[None] * len(arrays) for arrays in lists], [0] * len(lists))]
    bufs = [[torch.full((cap,) + tuple(shape), fill, dtype=dtype, device=dev) for dtype, shape, fill in arrays] for arrays, cap in zip(lists, capacities)]
    counts = run(bufs, capacities)
    return [[a[:min(n, cap)].cpu().numpy() for a in arrays] for arrays, n, cap in zip(bufs, counts, capacities)], counts


def _rows_with_map(rows, maps, row_dtype, out_dtype, order=None):
    """device rows (n, itemsize) uint8 of row_dtype and their map ids as one out_dtype array (`map` in front), sorted by the fields `order` (last
    is the primary key, as np.lexsort takes them) when given"""
    v = rows.reshape(-1).view(row_dtype)
    out = np.zeros(len(v), out_dtype)
    out["map"] = maps
    for f in row_dtype.names:
        out[f] = v[f]
    return out[np.lexsort(tuple(out[f] for f in order))] if order else out


class VoxelMap(_Owned):
    """A sparse voxel grid in a device hash table (include/vslam_hip.h "dense map"): per voxel a point count, the sums of the points' sub-voxel
    offsets and of their intensities, all integers, so the table does not depend on the order its points arrived in.  Filled through
    VO.voxel_insert_points_dev / VO.voxel_fuse_disparity_dev (or KeyframePipeline.dense_map); belongs to the VO it was created on.
    stats(): {n_occupied, n_points, n_dropped_range, n_dropped_full, status}."""
    _CREATE, _DESTROY, _CLEAR, _STATS, _STATS_T = "vslam_voxel_create", "vslam_voxel_destroy", "vslam_voxel_clear", "vslam_voxel_stats", VoxelStats

    def __init__(self, vo, voxel_size=0.2, log2_capacity=22):
        self.voxel_size, self.log2_capacity = float(voxel_size), int(log2_capacity)
        self._create(vo, voxel_size, log2_capacity)

    def extract(self, map_id=-1, min_count=1, capacity=None, sort=True):
        """the voxels with count >= min_count of map map_id (-1: every map) as a VOXEL_MAP_DTYPE array sorted by (map, ix, iy, iz) -- the canonical
        form for comparisons.  capacity: rows of the device buffer (None: the occupied slots); the call returns at most that many, in the table's
        order when the count exceeds it (self.last_count holds the full count)."""
        import torch
        vo = self.vo
        if capacity is None:
            capacity = max(self.stats()["n_occupied"], 1)
        ((rows, maps),), (self.last_count,) = _read_lists(vo, lambda *out: vo.voxel_extract_dev(self, map_id, min_count, *out),
                                                          [[(torch.uint8, (32,), 0), (torch.int32, (), 0)]], [capacity])
        return _rows_with_map(rows, maps, VOXEL_DTYPE, VOXEL_MAP_DTYPE, ("iz", "iy", "ix", "map") if sort else None)


def canonical_mesh(vertices, triangles):
    """the canonical form of a mesh for comparisons: vertices sorted by (map, ix, iy, iz, axis), triangle indices remapped (an index outside the vertex
    array stays as it is), every triangle's corner order kept, triangle rows sorted lexicographically"""
    order = np.lexsort((vertices["axis"], vertices["iz"], vertices["iy"], vertices["ix"], vertices["map"]))
    rank = np.empty(len(order), np.int32)
    rank[order] = np.arange(len(order), dtype=np.int32)
    tris = np.asarray(triangles, np.int32).reshape(-1, 3)
    inside = (tris >= 0) & (tris < len(order))
    tris = np.where(inside, rank[np.where(inside, tris, 0)] if len(order) else tris, tris).astype(np.int32)
    tris = tris[np.lexsort((tris[:, 2], tris[:, 1], tris[:, 0]))]
    return vertices[order], tris


class TsdfMap(_Owned):
    """A truncated signed distance field over 8 x 8 x 8 voxel blocks in a device pool (include/vslam_hip.h "surface map"): per voxel the integer sums
    of the quantised distance to the surface, of the views that saw it and of their intensities.  Views that look through a voxel carve it.  Filled
    through integrate_dev (or KeyframePipeline.surface_map) or load_blocks; extract() reads the surface as surfels, mesh() as indexed triangles over
    the same surfels; belongs to the VO it was created on.
    stats(): {n_blocks, n_samples, n_dropped_range, n_dropped_full, n_frames_skipped, n_pairs_visited, n_pairs_kept, status}."""
    _CREATE, _DESTROY, _CLEAR, _STATS, _STATS_T = "vslam_tsdf_create", "vslam_tsdf_destroy", "vslam_tsdf_clear", "vslam_tsdf_stats", TsdfStats

    def __init__(self, vo, voxel_size=0.2, trunc_voxels=4, log2_blocks=16):
        self.voxel_size, self.trunc_voxels, self.log2_blocks = float(voxel_size), int(trunc_voxels), int(log2_blocks)
        self._create(vo, voxel_size, trunc_voxels, log2_blocks)

    def integrate_dev(self, d_disp, d_gray, img_bytes, pitch, w, h, B, d_T, d_map_id, z_min, z_max, step=1):
        """VO.tsdf_integrate_dev into this map"""
        self.vo.tsdf_integrate_dev(self, d_disp, d_gray, img_bytes, pitch, w, h, B, d_T, d_map_id, z_min, z_max, step)

    def reach_dev(self, d_out):
        """the number of blocks claimed so far into the device uint32 at d_out, asynchronously on the context stream: after an integrate call, the
        reach of that call's frames (include/vslam_hip.h "RE-INTEGRATION")"""
        self.vo._chk(self.vo.lib.vslam_tsdf_reach_dev(self.vo.h, self.h, d_out), "vslam_tsdf_reach_dev")

    def reach(self):
        """reach_dev() read back: an int; synchronises"""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        d = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        self.reach_dev(d.data_ptr())
        self.vo.sync()
        return int(d.cpu()[0]) & 0xFFFFFFFF

    def reintegrate_dev(self, d_disp, d_gray, img_bytes, pitch, w, h, B, d_T_old, d_T_new, d_map_id, d_reach, z_min, z_max, step=1):
        """vslam_tsdf_reintegrate_dev on this map: B frames taken out at d_T_old within their d_reach and put in at d_T_new (a pose that is not
        finite switches its side off); asynchronous on the context stream"""
        self.vo._chk(self.vo.lib.vslam_tsdf_reintegrate_dev(self.vo.h, self.h, d_disp, d_gray, img_bytes, pitch, w, h, B, d_T_old, d_T_new, d_map_id, d_reach,
                                                            z_min, z_max, step), "vslam_tsdf_reintegrate_dev")

    def reintegrate(self, disp, gray, T_old, T_new, map_id, reach, z_min, z_max, step=1):
        """reintegrate_dev on host or torch arrays, for callers who keep disparities across steps: disp (B, h, w) float32, gray (B, h, pitch >= w) uint8
        or None, T_old / T_new (B, 7) (None: all NaN, that side switched off), map_id (B,) or one id, reach (B,) or one value -- what reach() gave
        after the call that integrated the frame.  The disparity, image, gates and old pose must be the ones the frame went in with.  Synchronises;
        returns the reach of this call's new sides."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())

        def put(a, dtype, shape=None):
            if isinstance(a, torch.Tensor):
                a = a.to(device=dev, dtype=dtype)
                return (a.expand(shape) if shape is not None else a).contiguous()
            a = np.asarray(a)
            return torch.from_numpy(np.array(np.broadcast_to(a, shape) if shape is not None else a)).to(device=dev, dtype=dtype)   # (a copy: the caller's array may be read-only)

        d_disp = put(disp, torch.float32)
        assert d_disp.dim() == 3, "disp: (B, h, w)"
        B, h, w = (int(v) for v in d_disp.shape)
        d_gray = None if gray is None else put(gray, torch.uint8)
        assert d_gray is None or (d_gray.dim() == 3 and d_gray.shape[0] == B and d_gray.shape[1] == h and d_gray.shape[2] >= w), "gray: (B, h, pitch >= w)"
        pitch = 0 if d_gray is None else int(d_gray.shape[2])
        nan = np.full((B, 7), np.nan)
        d_old = put(nan if T_old is None else T_old, torch.float64, (B, 7))
        d_new = put(nan if T_new is None else T_new, torch.float64, (B, 7))
        d_ids = put(map_id, torch.int32, (B,))
        r = reach.detach().cpu().numpy() if isinstance(reach, torch.Tensor) else np.asarray(reach)
        r = np.clip(np.broadcast_to(r.astype(np.int64), (B,)), 0, 0xFFFFFFFF).astype(np.uint32)   # (B numbers: the host is the simplest place to make them uint32)
        d_reach = torch.from_numpy(r.view(np.int32).copy()).to(dev)
        torch.cuda.synchronize(dev)   # (the buffers are ready before the context stream reads them)
        self.reintegrate_dev(d_disp.data_ptr(), None if d_gray is None else d_gray.data_ptr(), h * pitch, pitch, w, h, B, d_old.data_ptr(), d_new.data_ptr(),
                             d_ids.data_ptr(), d_reach.data_ptr(), float(z_min), float(z_max), int(step))
        return self.reach()

    def extract(self, map_id=-1, min_weight=1, capacity=None, sort=True):
        """the zero-crossing voxel edges of map map_id (-1: every map) between voxels of weight >= min_weight, as a SURFEL_MAP_DTYPE array sorted
        by (map, ix, iy, iz, axis) -- the canonical form for comparisons.  capacity: rows of the device buffer (None: counted by a first pass);
        the call returns at most that many (self.last_count holds the full count)."""
        import torch
        vo = self.vo
        call = lambda *out: vo._chk(vo.lib.vslam_tsdf_extract_dev(vo.h, self.h, map_id, min_weight, *out), "vslam_tsdf_extract_dev")
        ((rows, maps),), (self.last_count,) = _read_lists(vo, call, [[(torch.uint8, (48,), 0), (torch.int32, (), 0)]], None if capacity is None else [capacity])
        return _rows_with_map(rows, maps, SURFEL_DTYPE, SURFEL_MAP_DTYPE, ("axis", "iz", "iy", "ix", "map") if sort else None)

    def blocks(self, map_id=-1):
        """the claimed blocks of map map_id (-1: every map), raw: (ids (n, 4) int32 of (map, bx, by, bz), voxels (n, 512, 4) uint32 of (W, Sq, Wc, I)
        with voxel (ix, iy, iz) at (iz & 7) << 6 | (iy & 7) << 3 | (ix & 7)), sorted by (map, bx, by, bz)"""
        import torch
        vo = self.vo
        call = lambda *out: vo._chk(vo.lib.vslam_tsdf_blocks_dev(vo.h, self.h, map_id, *out), "vslam_tsdf_blocks_dev")
        ((ids, vox),), _ = _read_lists(vo, call, [[(torch.int32, (4,), 0), (torch.uint8, (8192,), 0)]], [max(self.stats()["n_blocks"], 1)])
        vox = vox.view(np.uint32).reshape(len(ids), 512, 4)
        order = np.lexsort((ids[:, 3], ids[:, 2], ids[:, 1], ids[:, 0]))
        return ids[order], vox[order]

    def load_blocks(self, ids, voxels):
        """the inverse of blocks(): every listed block (ids (n, 4) of (map, bx, by, bz), voxels (n, 512, 4) uint32) is claimed if it is absent and its
        voxels are replaced.  An id out of range counts in stats()["n_dropped_range"], a block that finds no slot in n_dropped_full; the ids of
        one call must be distinct."""
        import torch
        vo = self.vo
        ids = np.array(ids, np.int32).reshape(-1, 4)                  # (copies: the caller's arrays may be read-only)
        voxels = np.array(voxels, np.uint32).reshape(-1, 512, 4)
        assert len(ids) == len(voxels), (ids.shape, voxels.shape)
        if not len(ids):
            return
        dev = torch.device("cuda", torch.cuda.current_device())
        d_ids = torch.from_numpy(ids).to(dev)
        d_vox = torch.from_numpy(voxels.view(np.int32)).to(dev)
        torch.cuda.synchronize(dev)
        vo._chk(vo.lib.vslam_tsdf_load_blocks_dev(vo.h, self.h, d_ids.data_ptr(), d_vox.data_ptr(), len(ids)), "vslam_tsdf_load_blocks_dev")
        vo.sync()

    def mesh(self, map_id=-1, min_weight=1, sort=True):
        """the triangle mesh of map map_id (-1: every map) over voxels of weight >= min_weight (include/vslam_hip.h "MESH"): (vertices, triangles) --
        the surfels of extract() with the same arguments as a SURFEL_MAP_DTYPE array, and (n, 3) int32 indices into it, counter-clockwise seen from
        free space.  sort: the canonical form -- vertices sorted by (map, ix, iy, iz, axis), the indices remapped, every triangle's corner order kept
        as emitted, the rows sorted lexicographically; otherwise the device's order.  A first call counts, as extract() does; self.last_counts
        holds the device's two counts."""
        import torch
        vo = self.vo
        call = lambda *out: vo._chk(vo.lib.vslam_tsdf_mesh_dev(vo.h, self.h, map_id, min_weight, *out), "vslam_tsdf_mesh_dev")
        ((rows, maps), (tris,)), counts = _read_lists(vo, call, [[(torch.uint8, (48,), 0), (torch.int32, (), 0)], [(torch.int32, (3,), -1)]])
        self.last_counts = tuple(counts)
        verts = _rows_with_map(rows, maps, SURFEL_DTYPE, SURFEL_MAP_DTYPE)
        if not sort:
            return verts, tris
        return canonical_mesh(verts, tris)

    def render(self, T_c_w, map_id=0, K4=None, size=None, z_min=None, z_max=None, march=0.5, min_weight=1, attrs=True):
        """what cameras at the poses T_c_w (V, 7) see of the map (include/vslam_hip.h "RENDER"): dict(depth (V, h, w) f32 -- the camera's z of the
        surface, 0 where the ray misses --, normal (V, h, w, 3) f32 in the world frame pointing into free space, intensity (V, h, w) f32,
        counts = (rays that hit, samples evaluated)); normal and intensity are None with attrs=False.  map_id: one id for every view or one
        per view (outside 0 .. 1022: all misses).  K4 = (fx, fy, cx, cy), size = (w, h) and the depth range default to the context's camera, image
        size and depth_min .. depth_reliable; march: the step between samples in voxels, in [1/8, 1]; min_weight as in extract()."""
        import torch
        vo = self.vo
        p = vo.params
        T = np.ascontiguousarray(T_c_w, np.float64).reshape(-1, 7)
        V = len(T)
        ids = np.array(np.broadcast_to(np.asarray(map_id, np.int32), (V,)))                 # (a copy: the caller's array may be read-only)
        fx, fy, cx, cy = (float(v) for v in (p.cam[:4] if K4 is None else K4))
        w, h = (int(p.img_w), int(p.img_h)) if size is None else (int(size[0]), int(size[1]))
        rp = TsdfRenderParams(w=w, h=h, fx=fx, fy=fy, cx=cx, cy=cy, z_min=float(p.depth_min if z_min is None else z_min),
                              z_max=float(p.depth_reliable if z_max is None else z_max), march=float(march), min_weight=int(min_weight))
        dev = torch.device("cuda", torch.cuda.current_device())
        d_T = torch.from_numpy(T).to(dev)
        d_ids = torch.from_numpy(ids).to(dev)
        d_depth = torch.zeros((V, max(h, 0), max(w, 0)), dtype=torch.float32, device=dev)
        d_attr = torch.zeros((V, max(h, 0), max(w, 0), 4), dtype=torch.float32, device=dev) if attrs else None
        d_counts = torch.zeros(2, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)   # (the buffers are ready before the context stream writes them)
        vo.tsdf_render_dev(self, rp, V, d_T.data_ptr(), d_ids.data_ptr(), d_depth.data_ptr(), d_attr.data_ptr() if attrs else None, d_counts.data_ptr())
        vo.sync()
        attr = d_attr.cpu().numpy() if attrs else None
        return dict(depth=d_depth.cpu().numpy(), normal=attr[..., :3] if attrs else None, intensity=attr[..., 3] if attrs else None,
                    counts=tuple(int(c) for c in d_counts.cpu().tolist()))

    def distance(self, map_id=-1, min_weight=1, radius=8, log2_layer_blocks=None):
        """builds the map's clearance layer (include/vslam_hip.h "DISTANCE") over map map_id (-1: every map) with radius `radius` voxels in [1, 16] and
        reads it back: dict(ids (n, 4) int32 of (map, bx, by, bz), cells (n, 512) uint16 cell words -- bits 0-11 the squared distance to the nearest
        site in voxel units (0xFFF: FAR), bits 12-13 the class (0 UNKNOWN, 1 FREE, 2 OCCUPIED) -- in blocks()' voxel order, counts = (sites, layer
        blocks, layer blocks the pool does not hold)), sorted by (map, bx, by, bz).  log2_layer_blocks: the size of the layer's table (None: the
        map's log2_blocks); a layer that does not fit is void (stats()["status"] bit 4, no blocks).  The layer stays in the handle for
        distance_query() until the map changes."""
        import torch
        vo = self.vo
        dp = TsdfDistanceParams(struct_size=C.sizeof(TsdfDistanceParams), map_id=int(map_id), min_weight=int(min_weight), radius_voxels=int(radius),
                                log2_layer_blocks=int(self.log2_blocks if log2_layer_blocks is None else log2_layer_blocks))
        dev = torch.device("cuda", torch.cuda.current_device())
        d_counts = torch.zeros(3, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)   # (the buffer is ready before the context stream writes it)
        vo._chk(vo.lib.vslam_tsdf_distance_dev(vo.h, self.h, C.byref(dp), d_counts.data_ptr()), "vslam_tsdf_distance_dev")
        vo.sync()
        counts = tuple(int(c) for c in d_counts.cpu().tolist())
        call = lambda *out: vo._chk(vo.lib.vslam_tsdf_distance_blocks_dev(vo.h, self.h, map_id, *out), "vslam_tsdf_distance_blocks_dev")
        ((ids, cells),), (self.last_count,) = _read_lists(vo, call, [[(torch.int32, (4,), 0), (torch.uint8, (1024,), 0)]], [max(counts[1], 1)])
        cells = cells.view(np.uint16).reshape(len(ids), 512)
        order = np.lexsort((ids[:, 3], ids[:, 2], ids[:, 1], ids[:, 0]))
        return dict(ids=ids[order], cells=cells[order], counts=counts)

    def distance_query(self, xyz, map_id=0):
        """the clearance of world points against the layer distance() built: xyz (N, 3) float64, map_id one id or (N,) -> (dist (N,) float32 in
        metres -- negative inside occupied space, +-inf beyond the radius --, cls (N,) uint8: 0 UNKNOWN, 1 FREE, 2 OCCUPIED, 3 INVALID).  The
        nearest voxel answers: no interpolation."""
        import torch
        vo = self.vo
        xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        N = len(xyz)
        ids = np.array(np.broadcast_to(np.asarray(map_id, np.int32), (N,)))                 # (a copy: the caller's array may be read-only)
        dev = torch.device("cuda", torch.cuda.current_device())
        d_xyz = torch.from_numpy(xyz).to(dev)
        d_ids = torch.from_numpy(ids).to(dev)
        d_dist = torch.zeros(max(N, 1), dtype=torch.float32, device=dev)
        d_cls = torch.zeros(max(N, 1), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)   # (the buffers are ready before the context stream writes them)
        vo._chk(vo.lib.vslam_tsdf_distance_query_dev(vo.h, self.h, d_xyz.data_ptr(), d_ids.data_ptr(), N, d_dist.data_ptr(), d_cls.data_ptr()),
                "vslam_tsdf_distance_query_dev")
        vo.sync()
        return d_dist[:N].cpu().numpy(), d_cls[:N].cpu().numpy()


class PlaceDB(_Owned):
    """A database of keyframe descriptor blocks that outlives the steps (include/vslam_hip.h "place database"): entries are appended by
    VO.place_add_dev, scored against each other by brute force on the matrix cores (VO.place_score_dev), and the best candidates verified with the
    matcher and the RANSAC pose stage (VO.place_verify_dev).  KeyframePipeline.loop_closures drives all of it; belongs to the VO it was created on.
    stats(): {n_entries, capacity, rows_per_entry, with_geometry, n_refused}; clear() forgets every entry and zeroes the refusal counter."""
    _CREATE, _DESTROY, _CLEAR, _STATS, _STATS_T = "vslam_place_create", "vslam_place_destroy", "vslam_place_clear", "vslam_place_stats", PlaceStats

    def __init__(self, vo, rows, capacity=4096, with_geometry=True):
        self.rows, self.capacity, self.with_geometry = int(rows), int(capacity), bool(with_geometry)
        self._create(vo, self.rows, self.capacity, int(self.with_geometry))

    def __len__(self):
        return self.stats()["n_entries"]

    def meta(self, first=0, count=None):
        """(n, seq, frame) int32 arrays of entries [first, first + count) (count None: to the last entry); synchronises"""
        count = len(self) - first if count is None else count
        n = np.zeros(count, np.int32); seq = np.zeros(count, np.int32); frame = np.zeros(count, np.int32)
        self.vo._chk(self.vo.lib.vslam_place_read_meta(self.h, first, count, n, seq, frame), "vslam_place_read_meta")
        return n, seq, frame

    def entry(self, e):
        """entry e as the database holds it: dict(n, seq, frame, desc (n, 32)) and, with geometry, xy (n, 2), xyz (n, 3), valid (n,), qsel (ascending
        rows that own a valid point); synchronises"""
        R = self.rows
        meta = np.zeros(4, np.int32); desc = np.zeros((R, 32), np.uint8)
        g = self.with_geometry
        xy = np.zeros((R, 2), np.float32) if g else None; xyz = np.zeros((R, 3), np.float32) if g else None
        valid = np.zeros(R, np.uint8) if g else None; qsel = np.zeros(R, np.int32) if g else None
        self.vo._chk(self.vo.lib.vslam_place_read_entry(self.h, e, meta, desc, xy, xyz, valid, qsel), "vslam_place_read_entry")
        n = int(meta[0])
        out = dict(n=n, seq=int(meta[1]), frame=int(meta[2]), desc=desc[:n], desc_tail=desc[n:])
        if g:
            out.update(xy=xy[:n], xyz=xyz[:n], valid=valid[:n], qsel=qsel[:int(meta[3])])
        return out

    def score(self, q0, nq, tau, min_gap):
        """the (nq, n_entries) int32 score table of query entries [q0, q0 + nq) as a torch tensor on the device (asynchronous on the context stream)"""
        import torch
        n = len(self)
        d_score = torch.empty((nq, max(n, 1)), dtype=torch.int32, device=torch.device("cuda", torch.cuda.current_device()))
        torch.cuda.synchronize()   # (the buffer is ready before the context stream writes it)
        self.vo.place_score_dev(self, q0, nq, tau, min_gap, d_score.data_ptr(), d_score.shape[1])
        return d_score

    def select(self, q0, d_score, K, min_score):
        """(candidates, scores), each (nq, K) int32 on the device, of a table score() returned"""
        import torch
        nq = d_score.shape[0]
        d_cand = torch.empty((nq, K), dtype=torch.int32, device=d_score.device); d_cs = torch.empty_like(d_cand)
        torch.cuda.synchronize()
        self.vo.place_select_dev(self, q0, nq, d_score.data_ptr(), d_score.shape[1], K, min_score, d_cand.data_ptr(), d_cs.data_ptr())
        return d_cand, d_cs

    def verify(self, q0, d_cand, rank, min_inliers=10):
        """(T_q_c (nq, 7) float64, n_matches, n_inliers (nq,) int32), on the device, of every query's rank-`rank` candidate"""
        import torch
        nq, K = d_cand.shape
        d_T = torch.empty((nq, 7), dtype=torch.float64, device=d_cand.device)
        d_nm = torch.empty(nq, dtype=torch.int32, device=d_cand.device); d_ni = torch.empty_like(d_nm)
        torch.cuda.synchronize()
        self.vo.place_verify_dev(self, q0, nq, d_cand.data_ptr(), K, rank, min_inliers, d_T.data_ptr(), d_nm.data_ptr(), d_ni.data_ptr())
        return d_T, d_nm, d_ni
