"""ctypes binding of the C-ABI in include/fpc.h (libfpc.so, built in-tree by
`__graft_entry__.build()` / `make -C feature-point-cnn_amd/csrc`).

There is no fallback: if the shared library is missing or cannot be loaded this
module raises, and so does every entry point of the package.
"""
import ctypes
import os
import subprocess

# PyTorch bundles its own HIP runtime (torch/lib/libamdhip64.so, soname libamdhip64.so.7).
# Import it BEFORE libfpc.so is mapped so that the loader resolves libfpc's
# libamdhip64.so.7 dependency to that already-loaded copy: two HIP runtimes in one
# process do not share a device.  (A C/C++ host links the system ROCm instead.)
import torch  # noqa: F401

_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FPC_LIB_PATH") or os.path.join(_DIR, "lib", "libfpc.so")   # FPC_LIB_PATH: A/B builds
CSRC = os.path.join(_DIR, "csrc")

# every symbol include/fpc.h declares (tests/test_abi.py checks the header against this list)
SYMBOLS = [
    "fpc_abi_version", "fpc_build_flags", "fpc_strerror", "fpc_last_hip_error", "fpc_default_config", "fpc_create",
    "fpc_destroy", "fpc_load_weights", "fpc_packed_size", "fpc_packed_device_ptr",
    "fpc_export_packed", "fpc_import_packed", "fpc_import_packed_device", "fpc_mark_weights_loaded", "fpc_set_stream", "fpc_upload_stream",
    "fpc_get_stream", "fpc_sync", "fpc_forward", "fpc_detect", "fpc_get_points", "fpc_results",
    "fpc_get_counts", "fpc_get_keypoints", "fpc_set_timing", "fpc_get_timings", "fpc_match", "fpc_first_within",
    "fpc_detect_u8", "fpc_u8_staging", "fpc_homography_adaptation", "fpc_detect_u8_resized",
    "fpc_sample_descriptors", "fpc_plan_hash", "fpc_broadcast_weights", "fpc_read_activation",
    "fpc_pack_layout_revision", "fpc_tile_choice", "fpc_check_guards", "fpc_stream_report", "fpc_output_range",
    "fpc_match_frames", "fpc_first_within_frames",
    "fpc_default_ransac_params", "fpc_ransac_homography", "fpc_homography_frames",
    "fpc_bank_create", "fpc_bank_destroy", "fpc_bank_get", "fpc_bank_store", "fpc_bank_store_rows", "fpc_bank_clear",
    "fpc_match_bank", "fpc_homography_bank", "fpc_bank_create_ex", "fpc_bank_format",
    "fpc_match_frames_guided", "fpc_match_bank_guided",
    "fpc_cell_order", "fpc_match_frames_guided_cells", "fpc_match_bank_guided_cells",
    "fpc_bank_topk_reserve", "fpc_match_bank_topk", "fpc_homography_bank_topk",
    "fpc_ransac_fundamental", "fpc_fundamental_frames", "fpc_fundamental_bank",
    "fpc_match_frames_guided_epipolar", "fpc_match_bank_guided_epipolar",
    "fpc_match_frames_guided_epipolar_cells", "fpc_match_bank_guided_epipolar_cells",
    "fpc_default_pose_params", "fpc_pose_fundamental", "fpc_pose_frames", "fpc_pose_bank",
    "fpc_default_pose_homography_params", "fpc_pose_homography", "fpc_pose_homography_frames", "fpc_pose_homography_bank",
    "fpc_default_pnp_params", "fpc_pnp_reserve", "fpc_bank_landmarks_reserve", "fpc_bank_store_landmarks",
    "fpc_bank_landmarks_get", "fpc_ransac_pnp", "fpc_pnp_frames", "fpc_pnp_bank",
    "fpc_ransac_p3p", "fpc_p3p_frames", "fpc_p3p_bank",
    "fpc_default_essential_params", "fpc_ransac_essential", "fpc_essential_frames", "fpc_essential_bank",
    "fpc_match_frames_guided_pose", "fpc_match_bank_guided_pose",
    "fpc_default_landmark_params", "fpc_landmarks_pairs", "fpc_landmarks_frames", "fpc_landmarks_bank",
    "fpc_default_sim3_params", "fpc_ransac_sim3", "fpc_sim3_frames", "fpc_sim3_bank",
    "fpc_default_refine_params", "fpc_refine_pose", "fpc_refine_pose_frames", "fpc_refine_pose_bank",
    "fpc_pnp_topk_reserve", "fpc_pnp_bank_topk", "fpc_p3p_bank_topk", "fpc_fundamental_bank_topk",
    "fpc_essential_bank_topk",
    "fpc_default_window_params", "fpc_window_reserve", "fpc_refine_window", "fpc_refine_window_frames",
    "fpc_refine_window_bank",
    "fpc_default_graph_params", "fpc_graph_reserve", "fpc_graph_get", "fpc_graph_clear", "fpc_graph_set_nodes",
    "fpc_graph_add_edges", "fpc_graph_optimise", "fpc_graph_apply_scale",
]

ABI_VERSION = 4
PACK_LAYOUT_REVISION = 4      # include/fpc.h FPC_PACK_LAYOUT_REVISION

# fpc_config.plan_flags (include/fpc.h, FPC_PLAN_*)
PLAN_FLAGS = {
    "no_fused_blocks": 1 << 0, "no_winograd": 1 << 1, "no_winograd_detector": 1 << 2, "no_winograd_layer_in1": 1 << 3,
    "no_xcd_order": 1 << 4, "no_fused_stem_pool": 1 << 5, "split_heads": 1 << 6, "nms_in_line": 1 << 7,
    "no_persistent_grid": 1 << 8, "layer1_tile_8x16": 1 << 9, "winograd_gen1": 1 << 10, "no_latency_tiles": 1 << 11,
    "nms_one_workgroup": 1 << 12, "no_fused_softmax": 1 << 13, "winograd_gen2": 1 << 14, "guard_zones": 1 << 15, "detector_gen1": 1 << 16, "heads_in_line": 1 << 17, "w36_one_wave": 1 << 18, "convt_phases": 1 << 19, "stem_round3": 1 << 20, "conv_round1": 1 << 21,
    "tiles_round5": 1 << 22,
}


class FpcConfig(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int), ("height", ctypes.c_int), ("width", ctypes.c_int),
                ("max_batch", ctypes.c_int), ("cell", ctypes.c_int), ("nms_dist", ctypes.c_int),
                ("conf_thresh", ctypes.c_float), ("border_remove", ctypes.c_int),
                ("descriptor_enabled", ctypes.c_int), ("max_keypoints", ctypes.c_int),
                ("in_channels", ctypes.c_int), ("dtype", ctypes.c_int), ("arch", ctypes.c_int),
                ("num_streams", ctypes.c_int), ("plan_flags", ctypes.c_uint), ("nms_round_launches", ctypes.c_int),
                ("min_sub_batch", ctypes.c_int)]


class FpcTensor(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("data", ctypes.c_void_p), ("ndim", ctypes.c_int),
                ("shape", ctypes.c_int64 * 4)]


class FpcDeviceResults(ctypes.Structure):
    _fields_ = [("count", ctypes.c_void_p), ("n_candidates", ctypes.c_void_p), ("xy", ctypes.c_void_p),
                ("conf", ctypes.c_void_p), ("desc", ctypes.c_void_p), ("capacity", ctypes.c_int),
                ("desc_dim", ctypes.c_int)]


class FpcStreamReport(ctypes.Structure):
    _fields_ = [("n_streams", ctypes.c_int), ("slot", ctypes.c_int * 16), ("queue", ctypes.c_int * 16),
                ("probing", ctypes.c_int), ("hw_queues_found", ctypes.c_int), ("process_probe_rounds", ctypes.c_int),
                ("process_probe_launches", ctypes.c_int), ("process_inconclusive_rounds", ctypes.c_int),
                ("process_probe_ms", ctypes.c_float), ("create_probe_rounds", ctypes.c_int),
                ("create_placement_ms", ctypes.c_float), ("process_registered_streams", ctypes.c_int)]


class FpcRansacParams(ctypes.Structure):
    """fpc_ransac_params (include/fpc.h)."""
    _fields_ = [("iterations", ctypes.c_int), ("reproj_threshold", ctypes.c_float), ("seed", ctypes.c_uint32),
                ("refits", ctypes.c_int), ("min_inliers", ctypes.c_int)]


class FpcEssentialParams(ctypes.Structure):
    """fpc_essential_params (include/fpc.h): the fields of fpc_ransac_params, then the two cameras."""
    _fields_ = FpcRansacParams._fields_ + [
        ("q_fx", ctypes.c_float), ("q_fy", ctypes.c_float), ("q_cx", ctypes.c_float), ("q_cy", ctypes.c_float),
        ("t_fx", ctypes.c_float), ("t_fy", ctypes.c_float), ("t_cx", ctypes.c_float), ("t_cy", ctypes.c_float)]


class FpcPoseParams(ctypes.Structure):
    """fpc_pose_params (include/fpc.h)."""
    _fields_ = [("q_fx", ctypes.c_float), ("q_fy", ctypes.c_float), ("q_cx", ctypes.c_float), ("q_cy", ctypes.c_float),
                ("t_fx", ctypes.c_float), ("t_fy", ctypes.c_float), ("t_cx", ctypes.c_float), ("t_cy", ctypes.c_float),
                ("reproj_threshold", ctypes.c_float), ("min_front", ctypes.c_int)]


class FpcPoseHomographyParams(ctypes.Structure):
    """fpc_pose_homography_params (include/fpc.h)."""
    _fields_ = [("q_fx", ctypes.c_float), ("q_fy", ctypes.c_float), ("q_cx", ctypes.c_float), ("q_cy", ctypes.c_float),
                ("t_fx", ctypes.c_float), ("t_fy", ctypes.c_float), ("t_cx", ctypes.c_float), ("t_cy", ctypes.c_float),
                ("reproj_threshold", ctypes.c_float), ("min_front", ctypes.c_int), ("min_baseline", ctypes.c_float),
                ("which", ctypes.c_int)]


class FpcPnpParams(ctypes.Structure):
    """fpc_pnp_params (include/fpc.h)."""
    _fields_ = [("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("iterations", ctypes.c_int), ("reproj_threshold", ctypes.c_float), ("seed", ctypes.c_uint32),
                ("refits", ctypes.c_int), ("min_inliers", ctypes.c_int)]


class FpcLandmarkParams(ctypes.Structure):
    """fpc_landmark_params (include/fpc.h)."""
    _fields_ = [("q_fx", ctypes.c_float), ("q_fy", ctypes.c_float), ("q_cx", ctypes.c_float), ("q_cy", ctypes.c_float),
                ("t_fx", ctypes.c_float), ("t_fy", ctypes.c_float), ("t_cx", ctypes.c_float), ("t_cy", ctypes.c_float),
                ("reproj_threshold", ctypes.c_float), ("min_parallax_deg", ctypes.c_float)]


class FpcRefineParams(ctypes.Structure):
    """fpc_refine_params (include/fpc.h)."""
    _fields_ = [("q_fx", ctypes.c_float), ("q_fy", ctypes.c_float), ("q_cx", ctypes.c_float), ("q_cy", ctypes.c_float),
                ("t_fx", ctypes.c_float), ("t_fy", ctypes.c_float), ("t_cx", ctypes.c_float), ("t_cy", ctypes.c_float),
                ("reproj_threshold", ctypes.c_float), ("min_parallax_deg", ctypes.c_float), ("iterations", ctypes.c_int),
                ("lambda0", ctypes.c_float), ("min_front", ctypes.c_int)]


class FpcWindowParams(ctypes.Structure):
    """fpc_window_params (include/fpc.h)."""
    _fields_ = [("q_fx", ctypes.c_float), ("q_fy", ctypes.c_float), ("q_cx", ctypes.c_float), ("q_cy", ctypes.c_float),
                ("t_fx", ctypes.c_float), ("t_fy", ctypes.c_float), ("t_cx", ctypes.c_float), ("t_cy", ctypes.c_float),
                ("reproj_threshold", ctypes.c_float), ("iterations", ctypes.c_int), ("lambda0", ctypes.c_float),
                ("min_obs", ctypes.c_int)]


WINDOW_MAX_FRAMES = 16        # include/fpc.h FPC_WINDOW_MAX_FRAMES


class FpcGraphParams(ctypes.Structure):
    """fpc_graph_params (include/fpc.h)."""
    _fields_ = [("iterations", ctypes.c_int), ("lambda0", ctypes.c_float), ("cg_iterations", ctypes.c_int),
                ("cg_tol", ctypes.c_float), ("trans_unit", ctypes.c_float)]


class FpcGraphView(ctypes.Structure):
    """fpc_graph_view (include/fpc.h)."""
    _fields_ = [("nodes", ctypes.c_int), ("edges", ctypes.c_int), ("node_s", ctypes.c_void_p), ("node_R", ctypes.c_void_p),
                ("node_t", ctypes.c_void_p), ("edge_from", ctypes.c_void_p), ("edge_to", ctypes.c_void_p),
                ("edge_s", ctypes.c_void_p), ("edge_R", ctypes.c_void_p), ("edge_t", ctypes.c_void_p),
                ("edge_w", ctypes.c_void_p), ("count", ctypes.c_void_p), ("bytes", ctypes.c_size_t)]


GRAPH_MAX_EDGES = 16384       # include/fpc.h FPC_GRAPH_MAX_EDGES
GRAPH_INIT_TO = 1             # include/fpc.h FPC_GRAPH_INIT_TO


class FpcSim3Params(ctypes.Structure):
    """fpc_sim3_params (include/fpc.h)."""
    _fields_ = [("q_fx", ctypes.c_float), ("q_fy", ctypes.c_float), ("q_cx", ctypes.c_float), ("q_cy", ctypes.c_float),
                ("t_fx", ctypes.c_float), ("t_fy", ctypes.c_float), ("t_cx", ctypes.c_float), ("t_cy", ctypes.c_float),
                ("iterations", ctypes.c_int), ("reproj_threshold", ctypes.c_float), ("seed", ctypes.c_uint32),
                ("refits", ctypes.c_int), ("min_inliers", ctypes.c_int), ("fix_scale", ctypes.c_int)]


BANK_MAX_SLOTS = 1024        # include/fpc.h FPC_BANK_MAX_SLOTS
BANK_TOPK_MAX = 16            # include/fpc.h FPC_BANK_TOPK_MAX


class FpcBankView(ctypes.Structure):
    """fpc_bank_view (include/fpc.h)."""
    _fields_ = [("desc", ctypes.c_void_p), ("xy", ctypes.c_void_p), ("count", ctypes.c_void_p), ("slots", ctypes.c_int),
                ("rows", ctypes.c_int), ("desc_dim", ctypes.c_int), ("chunk", ctypes.c_int), ("bytes", ctypes.c_size_t)]


class FpcError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        l = load()
        msg = l.fpc_strerror(code).decode()
        detail = l.fpc_last_hip_error().decode()
        super().__init__("%s: %s (%d)%s" % (where, msg, code, " -- " + detail if detail else ""))


_lib = None


def build(force=False):
    """Compile libfpc.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    args = ["make", "-s", "-C", CSRC]
    if force:
        args.append("-B")
    subprocess.check_call(args)
    return LIB_PATH


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libfpc.so is not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `make -C feature-point-cnn_amd/csrc`; there is no CPU fallback" % LIB_PATH)
    l = ctypes.CDLL(LIB_PATH)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    l.fpc_abi_version.restype = ci
    l.fpc_build_flags.restype = ctypes.c_char_p
    l.fpc_strerror.restype = ctypes.c_char_p
    l.fpc_strerror.argtypes = [ci]
    l.fpc_last_hip_error.restype = ctypes.c_char_p
    l.fpc_default_config.argtypes = [ctypes.POINTER(FpcConfig)]
    l.fpc_create.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(FpcConfig)]
    l.fpc_destroy.argtypes = [vp]
    l.fpc_destroy.restype = None
    l.fpc_load_weights.argtypes = [vp, ctypes.POINTER(FpcTensor), ci]
    l.fpc_packed_size.argtypes = [vp]
    l.fpc_packed_size.restype = ctypes.c_size_t
    l.fpc_packed_device_ptr.argtypes = [vp]
    l.fpc_packed_device_ptr.restype = vp
    l.fpc_export_packed.argtypes = [vp, vp, ctypes.c_size_t]
    l.fpc_import_packed.argtypes = [vp, vp, ctypes.c_size_t]
    l.fpc_import_packed_device.argtypes = [vp, vp, ctypes.c_size_t]
    l.fpc_mark_weights_loaded.argtypes = [vp]
    l.fpc_set_stream.argtypes = [vp, vp]
    l.fpc_upload_stream.argtypes = [vp]
    l.fpc_upload_stream.restype = vp
    l.fpc_get_stream.argtypes = [vp]
    l.fpc_get_stream.restype = vp
    l.fpc_sync.argtypes = [vp]
    l.fpc_forward.argtypes = [vp, vp, ci, vp, vp, vp]
    l.fpc_detect.argtypes = [vp, vp, ci]
    l.fpc_get_points.argtypes = [vp, vp, vp, ci]
    l.fpc_detect_u8.argtypes = [vp, vp, ci, ci]
    l.fpc_u8_staging.argtypes = [vp]
    l.fpc_detect_u8_resized.argtypes = [vp, vp, ci, ci, ci, ci]
    l.fpc_homography_adaptation.argtypes = [vp, vp, ci, vp, vp, ci, ci, ci, vp]
    l.fpc_u8_staging.restype = vp
    l.fpc_results.argtypes = [vp, ctypes.POINTER(FpcDeviceResults)]
    l.fpc_get_counts.argtypes = [vp, ci, vp, vp]
    l.fpc_get_keypoints.argtypes = [vp, ci, ci, vp, vp, vp]
    l.fpc_output_range.argtypes = [vp, ci, vp, vp, vp]
    l.fpc_match.argtypes = [vp, vp, ci, vp, ci, ci, ctypes.c_float, vp, vp]
    l.fpc_first_within.argtypes = [vp, vp, ci, vp, ci, ctypes.c_float, vp]
    l.fpc_match_frames.argtypes = [vp, ci, ci, vp, vp, ci, ctypes.c_float, ctypes.c_float, vp, vp]
    l.fpc_first_within_frames.argtypes = [vp, ci, vp, vp, ctypes.c_float, vp]
    rp = ctypes.POINTER(FpcRansacParams)
    l.fpc_default_ransac_params.argtypes = [rp]
    l.fpc_ransac_homography.argtypes = [vp, ci, vp, vp, vp, ci, rp, vp, vp, vp]
    l.fpc_homography_frames.argtypes = [vp, ci, ci, vp, vp, vp, rp, vp, vp, vp]
    l.fpc_bank_create.argtypes = [vp, ci, ci]
    l.fpc_bank_create_ex.argtypes = [vp, ci, ci, ci]
    l.fpc_bank_format.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(vp)]
    l.fpc_bank_destroy.argtypes = [vp]
    l.fpc_bank_get.argtypes = [vp, ctypes.POINTER(FpcBankView)]
    l.fpc_bank_store.argtypes = [vp, ci, ci]
    l.fpc_bank_store_rows.argtypes = [vp, ci, vp, vp, vp]
    l.fpc_bank_clear.argtypes = [vp, ci]
    l.fpc_match_bank.argtypes = [vp, ci, ci, ctypes.c_float, ctypes.c_float, ci, vp, vp, vp, vp]
    l.fpc_homography_bank.argtypes = [vp, ci, vp, vp, rp, vp, vp, vp]
    l.fpc_ransac_fundamental.argtypes = [vp, ci, vp, vp, vp, ci, rp, vp, vp, vp]
    l.fpc_fundamental_frames.argtypes = [vp, ci, ci, vp, vp, vp, rp, vp, vp, vp]
    l.fpc_fundamental_bank.argtypes = [vp, ci, vp, vp, rp, vp, vp, vp]
    pp = ctypes.POINTER(FpcPoseParams)
    l.fpc_default_pose_params.argtypes = [pp]
    # the fundamental twins' arguments with (F_dev, params) where their params stand and five outputs for their three
    l.fpc_pose_fundamental.argtypes = [vp, ci, vp, vp, vp, ci, vp, pp, vp, vp, vp, vp, vp]
    l.fpc_pose_frames.argtypes = [vp, ci, ci, vp, vp, vp, vp, pp, vp, vp, vp, vp, vp]
    l.fpc_pose_bank.argtypes = [vp, ci, vp, vp, vp, pp, vp, vp, vp, vp, vp]
    hp = ctypes.POINTER(FpcPoseHomographyParams)
    l.fpc_default_pose_homography_params.argtypes = [hp]
    # the homography twins' arguments with (H_dev, params) where their params stand and eight outputs for their three
    l.fpc_pose_homography.argtypes = [vp, ci, vp, vp, vp, ci, vp, hp] + [vp] * 8
    l.fpc_pose_homography_frames.argtypes = [vp, ci, ci, vp, vp, vp, vp, hp] + [vp] * 8
    l.fpc_pose_homography_bank.argtypes = [vp, ci, vp, vp, vp, hp] + [vp] * 8
    np_ = ctypes.POINTER(FpcPnpParams)
    l.fpc_default_pnp_params.argtypes = [np_]
    l.fpc_pnp_reserve.argtypes = [vp, ctypes.POINTER(ctypes.c_size_t)]
    l.fpc_bank_landmarks_reserve.argtypes = [vp, ctypes.POINTER(ctypes.c_size_t)]
    l.fpc_bank_store_landmarks.argtypes = [vp, ci, vp, vp]
    l.fpc_bank_landmarks_get.argtypes = [vp, ctypes.POINTER(vp)]
    l.fpc_ransac_pnp.argtypes = [vp, ci, vp, vp, vp, ci, np_, vp, vp, vp, vp]
    l.fpc_pnp_frames.argtypes = [vp, ci, vp, vp, vp, vp, np_, vp, vp, vp, vp]
    l.fpc_pnp_bank.argtypes = [vp, ci, vp, vp, np_, vp, vp, vp, vp]
    l.fpc_ransac_p3p.argtypes = l.fpc_ransac_pnp.argtypes
    l.fpc_p3p_frames.argtypes = l.fpc_pnp_frames.argtypes
    l.fpc_p3p_bank.argtypes = l.fpc_pnp_bank.argtypes
    ep = ctypes.POINTER(FpcEssentialParams)
    l.fpc_default_essential_params.argtypes = [ep]
    # the fundamental twins' arguments with fpc_essential_params and E_dev behind F_dev
    l.fpc_ransac_essential.argtypes = [vp, ci, vp, vp, vp, ci, ep, vp, vp, vp, vp]
    l.fpc_essential_frames.argtypes = [vp, ci, ci, vp, vp, vp, ep, vp, vp, vp, vp]
    l.fpc_essential_bank.argtypes = [vp, ci, vp, vp, ep, vp, vp, vp, vp]
    l.fpc_match_frames_guided.argtypes = [vp, ci, ci, vp, vp, vp, vp, ctypes.c_float, ci, ctypes.c_float, ctypes.c_float,
                                          vp, vp]
    l.fpc_match_bank_guided.argtypes = [vp, ci, vp, vp, ctypes.c_float, ci, ctypes.c_float, ctypes.c_float, vp, vp]
    l.fpc_cell_order.argtypes = [vp, vp, vp, ci, ci, vp]
    l.fpc_match_frames_guided_cells.argtypes = [vp, ci, ci, vp, vp, vp, vp, ctypes.c_float, ci, ctypes.c_float,
                                                ctypes.c_float, vp, vp, vp]
    l.fpc_match_bank_guided_cells.argtypes = [vp, ci, vp, vp, ctypes.c_float, ci, ctypes.c_float, ctypes.c_float, vp, vp,
                                              vp]
    l.fpc_match_frames_guided_epipolar.argtypes = list(l.fpc_match_frames_guided.argtypes)      # F_dev where H_dev stands
    l.fpc_match_bank_guided_epipolar.argtypes = list(l.fpc_match_bank_guided.argtypes)
    l.fpc_match_frames_guided_epipolar_cells.argtypes = list(l.fpc_match_frames_guided_cells.argtypes)   # likewise
    l.fpc_match_bank_guided_epipolar_cells.argtypes = list(l.fpc_match_bank_guided_cells.argtypes)
    cf = ctypes.c_float
    l.fpc_match_frames_guided_pose.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, cf, cf, cf, cf, cf, ci, cf, cf, vp, vp]
    l.fpc_match_bank_guided_pose.argtypes = [vp, ci, vp, vp, vp, cf, cf, cf, cf, cf, ci, cf, cf, vp, vp]
    lp = ctypes.POINTER(FpcLandmarkParams)
    l.fpc_default_landmark_params.argtypes = [lp]
    # a pair source, then (R_dev, t_dev, params, xyz_dev, kind_dev, counts_dev)
    l.fpc_landmarks_pairs.argtypes = [vp, ci, vp, vp, vp, vp, vp, ci, vp, vp, lp, vp, vp, vp]
    l.fpc_landmarks_frames.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp, lp, vp, vp, vp]
    l.fpc_landmarks_bank.argtypes = [vp, ci, vp, vp, vp, vp, lp, vp, vp, vp]
    sp = ctypes.POINTER(FpcSim3Params)
    l.fpc_default_sim3_params.argtypes = [sp]
    l.fpc_ransac_sim3.argtypes = [vp, ci, vp, vp, vp, ci, sp, vp, vp, vp, vp, vp]
    l.fpc_sim3_frames.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, sp, vp, vp, vp, vp, vp]
    l.fpc_sim3_bank.argtypes = [vp, ci, vp, vp, vp, vp, sp, vp, vp, vp, vp, vp]
    fp = ctypes.POINTER(FpcRefineParams)
    l.fpc_default_refine_params.argtypes = [fp]
    # the pose twins' arguments with (R_in_dev, t_in_dev) where their F_dev stands and six outputs for their five
    l.fpc_refine_pose.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp, fp] + [vp] * 6
    l.fpc_refine_pose_frames.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, fp] + [vp] * 6
    l.fpc_refine_pose_bank.argtypes = [vp, ci, vp, vp, vp, vp, fp] + [vp] * 6
    wp = ctypes.POINTER(FpcWindowParams)
    l.fpc_default_window_params.argtypes = [wp]
    l.fpc_window_reserve.argtypes = [vp, ctypes.POINTER(ctypes.c_size_t)]
    # an observation source and the key, then (R_in_dev, t_in_dev, params) and the seven outputs
    l.fpc_refine_window.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, wp] + [vp] * 7
    l.fpc_refine_window_frames.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp, wp] + [vp] * 7
    l.fpc_refine_window_bank.argtypes = [vp, ci, vp, vp, vp, vp, vp, wp] + [vp] * 7
    gp = ctypes.POINTER(FpcGraphParams)
    l.fpc_default_graph_params.argtypes = [gp]
    l.fpc_graph_reserve.argtypes = [vp, ci, ci, ctypes.POINTER(ctypes.c_size_t)]
    l.fpc_graph_get.argtypes = [vp, ctypes.POINTER(FpcGraphView)]
    l.fpc_graph_clear.argtypes = [vp]
    l.fpc_graph_set_nodes.argtypes = [vp, ci, ci, vp, vp, vp]
    # (n, from_dev, to_dev, s_dev, R_dev, t_dev, ninliers_dev, min_inliers, flags)
    l.fpc_graph_add_edges.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, ci, ctypes.c_uint]
    l.fpc_graph_optimise.argtypes = [vp, vp, gp, vp]
    l.fpc_graph_apply_scale.argtypes = [vp]
    l.fpc_bank_topk_reserve.argtypes =[vp, ci, ctypes.POINTER(ctypes.c_size_t)]
    l.fpc_match_bank_topk.argtypes = [vp, ci, ci, ci, ctypes.c_float, ctypes.c_float, ci, vp, vp, vp, vp, vp]
    l.fpc_homography_bank_topk.argtypes = [vp, ci, ci, vp, vp, rp, vp, vp, vp, vp, vp]
    # the homography call's arguments with the model's parameters and outputs, and the picked model(s) behind best_dev
    l.fpc_pnp_topk_reserve.argtypes = [vp, ctypes.POINTER(ctypes.c_size_t)]
    l.fpc_pnp_bank_topk.argtypes = [vp, ci, ci, vp, vp, np_] + [vp] * 8
    l.fpc_p3p_bank_topk.argtypes = l.fpc_pnp_bank_topk.argtypes
    l.fpc_fundamental_bank_topk.argtypes = [vp, ci, ci, vp, vp, rp] + [vp] * 6
    l.fpc_essential_bank_topk.argtypes = [vp, ci, ci, vp, vp, ep] + [vp] * 7
    l.fpc_sample_descriptors.argtypes = [vp, vp, vp, ci, vp]
    l.fpc_read_activation.argtypes = [vp, ctypes.c_char_p, ci, ci, vp, ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ci)]
    l.fpc_plan_hash.argtypes = [vp]
    l.fpc_plan_hash.restype = ctypes.c_uint64
    l.fpc_broadcast_weights.argtypes = [vp, vp, ci]
    l.fpc_pack_layout_revision.restype = ci
    l.fpc_tile_choice.argtypes = [ci, ci, ci, ci, ctypes.c_uint]
    l.fpc_check_guards.argtypes = [vp, ctypes.POINTER(ctypes.c_longlong)]
    l.fpc_stream_report.argtypes = [vp, ctypes.POINTER(FpcStreamReport)]
    l.fpc_set_timing.argtypes = [vp, ci]
    l.fpc_get_timings.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_char_p),
                                  ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double),
                                  ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    for s in SYMBOLS:
        getattr(l, s)  # AttributeError if the library lacks a declared symbol
    if l.fpc_abi_version() != ABI_VERSION:
        raise ImportError("libfpc.so has ABI version %d, this binding is for %d: rebuild (make -C %s)"
                          % (l.fpc_abi_version(), ABI_VERSION, CSRC))
    if l.fpc_pack_layout_revision() != PACK_LAYOUT_REVISION:
        raise ImportError("libfpc.so packs fragment-layout revision %d, this binding expects %d: rebuild (make -C %s)"
                          % (l.fpc_pack_layout_revision(), PACK_LAYOUT_REVISION, CSRC))
    _lib = l
    return l


def check(code, where):
    if code < 0:
        raise FpcError(code, where)
    return code
