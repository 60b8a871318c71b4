"""ctypes binding of include/hafgrasp.h (libhafgrasp.so).  No torch types cross this boundary: plain pointers and
sizes only.  The library is gfx950-only and has no CPU fallback; loading works anywhere, haf_create needs the GPU."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HAF_LIB", os.path.join(HERE, "libhafgrasp.so"))   # HAF_LIB: A/B another build of the same ABI
# the TESTING build (-DHAF_TESTING): same kernels, plus the haf_test_* hooks and the environment switches that scale the
# guard bands.  Only tests/ load it (testlib(), Engine(..., testing=True)); the product library has neither.
TESTLIB_PATH = os.environ.get("HAF_TESTLIB", os.path.join(HERE, "libhafgrasp_testing.so"))   # HAF_TESTLIB: likewise (tools/ablate_h.sh)

HAF_OK, HAF_E_ARG, HAF_E_IO, HAF_E_DEVICE, HAF_E_CAPACITY, HAF_E_BUDGET, HAF_E_INTERNAL = 0, -1, -2, -3, -4, -5, -6
FLAG_KEEP_DEBUG, FLAG_PROFILE, FLAG_FP32_MFMA, FLAG_SPLIT_F16, FLAG_PROBABILITY, FLAG_FULL_RANK = 1, 2, 4, 8, 16, 32
DBG_HEIGHTS, DBG_INTEGRAL, DBG_MASK, DBG_LABELS, DBG_DECISION, DBG_TRANSFORM, DBG_SCREEN_MARGIN, DBG_PROBABILITY, DBG_GRASPSGRID, DBG_ROI = range(10)
SHARD_ROLLS, SHARD_CLOUDS = 0, 1
FRAME_DEPTH_U16, FRAME_DEPTH_F32, FRAME_XYZ_F32 = 0, 1, 2
MAP_NO_CELL = -32768                 # HAF_MAP_NO_CELL: a grasp-map pixel no roll has a cell for
MAX_LABELS = 4096                    # HAF_MAX_LABELS: instance labels of one haf_grasp_map_labels call
STAGES = ["upload", "bin", "integral", "mask", "features", "svm", "refine", "recheck", "vote", "download"]


class Config(C.Structure):
    _fields_ = [("feature_file", C.c_char_p), ("range_file", C.c_char_p), ("model_file", C.c_char_p),
                ("nr_features_without_shaf", C.c_int32), ("grid_h", C.c_int32), ("grid_w", C.c_int32),
                ("n_rolls", C.c_int32), ("roll_step_deg", C.c_int32), ("z_shift", C.c_float),
                ("graspval_top", C.c_int32), ("device", C.c_int32), ("max_clouds", C.c_int32),
                ("max_points", C.c_int64), ("flags", C.c_uint32), ("graspval_th", C.c_int32),
                ("max_rolls_per_call", C.c_int32)]


class GraspInput(C.Structure):
    _fields_ = [("grasp_area_center", C.c_double * 3), ("grasp_area_length_x", C.c_float),
                ("grasp_area_length_y", C.c_float), ("approach_vector", C.c_double * 3),
                ("max_calculation_time", C.c_double), ("show_only_best_grasp", C.c_int32),
                ("threshold_grasp_evaluation", C.c_int32), ("gripper_opening_width", C.c_int32)]


class GraspOutput(C.Structure):
    _fields_ = [("eval", C.c_int32), ("grasp_point1", C.c_double * 3), ("grasp_point2", C.c_double * 3),
                ("averaged_grasp_point", C.c_double * 3), ("approach_vector", C.c_double * 3), ("roll", C.c_float),
                ("best_row", C.c_int32), ("best_col", C.c_int32), ("best_roll", C.c_int32), ("best_vote", C.c_int32),
                ("rolls_done", C.c_int32), ("n_evals", C.c_int64), ("n_rechecked", C.c_int64)]


class RollRecord(C.Structure):
    _fields_ = [("vote", C.c_int32), ("row", C.c_int16), ("col", C.c_int16), ("h_locmax", C.c_float),
                ("n_evals", C.c_int32)]


class TopParams(C.Structure):
    """haf_top_params: ranked top-K candidates of the last scored batch (haf_top_grasps)"""
    _fields_ = [("k", C.c_int32), ("min_vote", C.c_int32), ("cell_radius", C.c_int32), ("roll_window", C.c_int32),
                ("min_dist_m", C.c_double)]


class GraspCandidate(C.Structure):
    _fields_ = [("grasp", GraspOutput), ("run_length", C.c_int32), ("h_locmax", C.c_float)]


class Cloud(C.Structure):
    _fields_ = [("xyz", C.c_void_p), ("n_points", C.c_size_t), ("stride_floats", C.c_size_t), ("on_device", C.c_int32)]


class Frame(C.Structure):
    """haf_frame: a depth image with its camera's intrinsics, or an organised sensor-frame cloud, plus the sensor-to-base transform"""
    _fields_ = [("data", C.c_void_p), ("kind", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("on_device", C.c_int32),
                ("row_stride_bytes", C.c_size_t), ("point_stride_bytes", C.c_size_t),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("depth_scale", C.c_float),
                ("min_depth", C.c_float), ("max_depth", C.c_float), ("sensor_to_base", C.c_float * 12)]


class DepthFilter(C.Structure):
    """haf_depth_filter: the parameters of haf_filter_depth"""
    _fields_ = [("radius", C.c_int32), ("min_support", C.c_int32), ("tol_abs", C.c_float), ("tol_rel", C.c_float), ("min_valid", C.c_int32)]


class SegmentParams(C.Structure):
    """haf_segment_params: the parameters of haf_segment_frame"""
    _fields_ = [("plane", C.c_float * 4), ("min_height", C.c_float), ("max_height", C.c_float), ("max_gap", C.c_float),
                ("min_pixels", C.c_int32), ("max_labels", C.c_int32)]


class SegmentInfo(C.Structure):
    """haf_segment_info: pixel count, anchor and inclusive bounding box of one label"""
    _fields_ = [(f, C.c_int32) for f in ("n_pixels", "anchor_u", "anchor_v", "u_min", "v_min", "u_max", "v_max")]


SEGMENT_INFO_DTYPE = np.dtype([(f, np.int32) for f in ("n_pixels", "anchor_u", "anchor_v", "u_min", "v_min", "u_max", "v_max")])
assert SEGMENT_INFO_DTYPE.itemsize == C.sizeof(SegmentInfo) == 28


class CellSegmentParams(C.Structure):
    """haf_cell_segment_params: the parameters of haf_segment_cells"""
    _fields_ = [("plane", C.c_float * 4), ("min_height", C.c_float), ("max_height", C.c_float), ("cell", C.c_float), ("x0", C.c_float),
                ("y0", C.c_float), ("nx", C.c_int32), ("ny", C.c_int32), ("connectivity", C.c_int32), ("max_step", C.c_float),
                ("min_points", C.c_int32), ("max_labels", C.c_int32)]


class CellSegmentInfo(C.Structure):
    """haf_cell_segment_info: point and cell counts, anchor cell, inclusive cell box and largest top of one label"""
    _fields_ = [(f, C.c_int32) for f in ("n_points", "n_cells", "anchor_ix", "anchor_iy", "ix_min", "iy_min", "ix_max", "iy_max")] + \
               [("top", C.c_float)]


CELL_SEGMENT_INFO_DTYPE = np.dtype([(f, np.int32) for f in ("n_points", "n_cells", "anchor_ix", "anchor_iy", "ix_min", "iy_min", "ix_max",
                                                             "iy_max")] + [("top", np.float32)])
assert CELL_SEGMENT_INFO_DTYPE.itemsize == C.sizeof(CellSegmentInfo) == 36
MAX_CELLS = 1 << 22


class PlaneParams(C.Structure):
    """haf_plane_params: the parameters of haf_fit_plane"""
    _fields_ = [("tol", C.c_float), ("min_area2", C.c_float), ("up", C.c_float * 3), ("max_tilt", C.c_float), ("n_hyp", C.c_int32),
                ("min_inliers", C.c_int32), ("seed", C.c_uint32)]


class PlaneResult(C.Structure):
    """haf_plane_result: the fitted plane, what it was fitted on and the integers behind it"""
    _fields_ = [("plane", C.c_float * 4), ("found", C.c_int32), ("winner", C.c_int32), ("n_inliers", C.c_int32), ("reserved", C.c_int32),
                ("rms", C.c_double), ("stats", C.c_int64 * 4), ("moments", C.c_int64 * 10)]


MAX_PLANE_HYP = 1024


class Gripper(C.Structure):
    """haf_gripper: one parallel-jaw gripper of haf_check_grasps, metres; the library's defaults are nominal figures, no real gripper's"""
    _fields_ = [("opening", C.c_float), ("finger_thickness", C.c_float), ("finger_breadth", C.c_float), ("tip_depth", C.c_float),
                ("finger_length", C.c_float), ("palm_width", C.c_float), ("palm_breadth", C.c_float), ("palm_height", C.c_float),
                ("max_hits", C.c_int32), ("min_between", C.c_int32)]


class GraspClearance(C.Structure):
    """haf_grasp_clearance: a grasp's integer row and what clearance_finish derives from it"""
    _fields_ = [("free", C.c_int32), ("n_near", C.c_int32), ("n_finger", C.c_int32 * 2), ("n_palm", C.c_int32), ("n_between", C.c_int32),
                ("s_min", C.c_int32), ("s_max", C.c_int32), ("u_max", C.c_int32), ("reserved", C.c_int32), ("width_m", C.c_double),
                ("offset_m", C.c_double), ("top_m", C.c_double)]


CLEARANCE_DTYPE = np.dtype([("free", np.int32), ("n_near", np.int32), ("n_finger", np.int32, 2), ("n_palm", np.int32), ("n_between", np.int32),
                            ("s_min", np.int32), ("s_max", np.int32), ("u_max", np.int32), ("reserved", np.int32), ("width_m", np.float64),
                            ("offset_m", np.float64), ("top_m", np.float64)])
assert CLEARANCE_DTYPE.itemsize == C.sizeof(GraspClearance) == 64
MAX_CHECK_GRASPS = 4096              # HAF_MAX_CHECK_GRASPS: grasps of one haf_check_grasps call


class OpeningParams(C.Structure):
    """haf_opening_params: the openings and the sideways shift haf_fit_openings searches, metres, and when a placement is free"""
    _fields_ = [("min_opening", C.c_float), ("max_opening", C.c_float), ("max_shift", C.c_float), ("max_hits", C.c_int32),
                ("min_between", C.c_int32)]


class GraspOpening(C.Structure):
    """haf_grasp_opening: a grasp's placement, the counts there and what opening_finish derives from them"""
    _fields_ = [("found", C.c_int32), ("j", C.c_int32), ("c", C.c_int32), ("sym_j", C.c_int32), ("n_between", C.c_int32),
                ("n_finger", C.c_int32 * 2), ("n_palm", C.c_int32), ("n_finger_slab", C.c_int32), ("n_palm_slab", C.c_int32),
                ("opening_m", C.c_double), ("shift_m", C.c_double), ("sym_opening_m", C.c_double)]


class OpeningInfo(C.Structure):
    """haf_opening_info: the integers of one haf_fit_openings call"""
    _fields_ = [("shift", C.c_int32), ("half_bins", C.c_int32), ("tb", C.c_int32), ("pb", C.c_int32), ("j_min", C.c_int32),
                ("j_max", C.c_int32), ("c_max", C.c_int32), ("reserved", C.c_int32), ("bin_m", C.c_double)]


OPENING_DTYPE = np.dtype([("found", np.int32), ("j", np.int32), ("c", np.int32), ("sym_j", np.int32), ("n_between", np.int32),
                          ("n_finger", np.int32, 2), ("n_palm", np.int32), ("n_finger_slab", np.int32), ("n_palm_slab", np.int32),
                          ("opening_m", np.float64), ("shift_m", np.float64), ("sym_opening_m", np.float64)])
assert OPENING_DTYPE.itemsize == C.sizeof(GraspOpening) == 64
OPEN_BINS = 128                      # HAF_OPEN_BINS: words of one histogram of haf_fit_openings


class SpaceParams(C.Structure):
    """haf_space_params: the lattice step of haf_check_space, the projection's near plane and tolerances, and when a grasp is clear; the
    library's defaults are nominal figures"""
    _fields_ = [("sample_step", C.c_float), ("near_m", C.c_float), ("tol_abs", C.c_float), ("tol_rel", C.c_float), ("max_hit", C.c_int32),
                ("max_unknown", C.c_int32), ("min_between_hit", C.c_int32)]


class GraspSpace(C.Structure):
    """haf_grasp_space: a grasp's counts n[region][state] and what space_finish derives from them"""
    _fields_ = [("clear", C.c_int32), ("n", (C.c_int32 * 4) * 4), ("reserved", C.c_int32 * 3)]


class SpaceInfo(C.Structure):
    """haf_space_info: the lattice of one haf_check_space call"""
    _fields_ = [("step", C.c_int32), ("n", (C.c_int32 * 3) * 4), ("n_samples", C.c_int32), ("reserved", C.c_int32 * 2)]


SPACE_DTYPE = np.dtype([("clear", np.int32), ("n", np.int32, (4, 4)), ("reserved", np.int32, 3)])
assert SPACE_DTYPE.itemsize == C.sizeof(GraspSpace) == 80 and C.sizeof(SpaceInfo) == 64
MAX_SPACE_VIEWS = 8                  # HAF_MAX_SPACE_VIEWS: depth views of one haf_check_space call
MAX_SPACE_SAMPLES = 65536            # HAF_MAX_SPACE_SAMPLES: lattice points of one grasp
MAX_SPACE_STATES = 1 << 22           # bytes of `states` haf_check_space offers
SPACE_BETWEEN, SPACE_FINGER0, SPACE_FINGER1, SPACE_PALM = range(4)         # HAF_SPACE_*: the regions, the first index of n
SPACE_UNSEEN, SPACE_HIDDEN, SPACE_FREE, SPACE_HIT = range(4)               # ... the states and their ranks, the second


class Roi(C.Structure):
    """haf_roi: the pixel mask of one request of haf_score_frames_roi, of one view of haf_score_views_roi"""
    _fields_ = [("mask", C.c_void_p), ("row_stride_bytes", C.c_size_t), ("on_device", C.c_int32)]


class LabelImage(C.Structure):
    """haf_label_image: an instance-label image that goes with a Frame of the same width x height (0 background, 1..n_labels instances)"""
    _fields_ = [("data", C.c_void_p), ("elem_bytes", C.c_int32), ("on_device", C.c_int32), ("row_stride_bytes", C.c_size_t)]


class Camera(C.Structure):
    """haf_camera: the rectified pinhole camera a label image belongs to, and the transform from the base frame into its frame"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("base_to_camera", C.c_float * 12)]


class TransferParams(C.Structure):
    """haf_transfer_params: the parameters of haf_transfer_labels"""
    _fields_ = [("near_m", C.c_float), ("tol_abs", C.c_float), ("tol_rel", C.c_float), ("splat", C.c_int32)]


class LabelPick(C.Structure):
    """haf_label_pick: the best pixel of one label and its grasp-map values"""
    _fields_ = [("found", C.c_int32), ("u", C.c_int32), ("v", C.c_int32), ("vote", C.c_int32), ("roll", C.c_int32), ("cell", C.c_int32),
                ("n_pixels", C.c_int32)]


LABEL_PICK_DTYPE = np.dtype([(f, np.int32) for f in ("found", "u", "v", "vote", "roll", "cell", "n_pixels")])
assert LABEL_PICK_DTYPE.itemsize == C.sizeof(LabelPick) == 28

SHAPE_DIRS = 12                      # HAF_SHAPE_DIRS: directions of haf_measure_labels' fan, 15 degrees apart
SHAPE_COS = (8192, 7913, 7094, 5793, 4096, 2120, 0, -2120, -4096, -5793, -7094, -7913)      # HAF_SHAPE_COS
SHAPE_SIN = (0, 2120, 4096, 5793, 7094, 7913, 8192, 7913, 7094, 5793, 4096, 2120)           # HAF_SHAPE_SIN
SHAPE_NN = tuple(c * c + s_ * s_ for c, s_ in zip(SHAPE_COS, SHAPE_SIN))                    # HAF_SHAPE_NN


class LabelShape(C.Structure):
    """haf_label_shape: the integers of one label's points in the base frame and the box derived from them"""
    _fields_ = [("sum", C.c_int64 * 3), ("found", C.c_int32), ("n_pixels", C.c_int32), ("n_points", C.c_int32), ("narrow_dir", C.c_int32),
                ("q_min", C.c_int32 * 3), ("q_max", C.c_int32 * 3), ("t_min", C.c_int32 * SHAPE_DIRS), ("t_max", C.c_int32 * SHAPE_DIRS),
                ("h_max", C.c_float), ("centroid", C.c_float * 3), ("box_min", C.c_float * 3), ("box_max", C.c_float * 3),
                ("width", C.c_float * SHAPE_DIRS), ("narrow_width", C.c_float), ("long_width", C.c_float), ("yaw", C.c_float),
                ("diameter", C.c_float), ("height", C.c_float), ("reserved", C.c_int32)]


LABEL_SHAPE_DTYPE = np.dtype([("sum", np.int64, 3), ("found", np.int32), ("n_pixels", np.int32), ("n_points", np.int32), ("narrow_dir", np.int32),
                              ("q_min", np.int32, 3), ("q_max", np.int32, 3), ("t_min", np.int32, SHAPE_DIRS), ("t_max", np.int32, SHAPE_DIRS),
                              ("h_max", np.float32), ("centroid", np.float32, 3), ("box_min", np.float32, 3), ("box_max", np.float32, 3),
                              ("width", np.float32, SHAPE_DIRS), ("narrow_width", np.float32), ("long_width", np.float32), ("yaw", np.float32),
                              ("diameter", np.float32), ("height", np.float32), ("reserved", np.int32)])
assert LABEL_SHAPE_DTYPE.itemsize == C.sizeof(LabelShape) == 272

ATTR_RECORD_DTYPE = np.dtype([("feature", np.float32), ("pad", np.float32), ("q4", np.float64), ("scaled", np.float64)])
assert ATTR_RECORD_DTYPE.itemsize == 24

ROLL_RECORD_DTYPE = np.dtype([("vote", np.int32), ("row", np.int16), ("col", np.int16), ("h_locmax", np.float32),
                              ("n_evals", np.int32)])
assert ROLL_RECORD_DTYPE.itemsize == C.sizeof(RollRecord) == 16

_lib = None
_testlib = None


class HafError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("hafgrasp error %d: %s" % (code, msg))
        self.code = code


def _bind(path, testing):
    if not os.path.exists(path):
        raise RuntimeError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950); "
                           "there is no CPU fallback" % path)
    L = C.CDLL(path)
    E = C.c_void_p
    L.haf_abi_version.restype = C.c_int
    L.haf_config_default.argtypes = [C.POINTER(Config)]
    L.haf_grasp_input_default.argtypes = [C.POINTER(GraspInput)]
    L.haf_create.argtypes = [C.POINTER(Config), C.POINTER(E)]
    L.haf_destroy.argtypes = [E]
    L.haf_last_error.restype = C.c_char_p
    L.haf_last_error.argtypes = [E]
    L.haf_score.argtypes = [E, C.POINTER(Cloud), C.POINTER(GraspInput), C.POINTER(GraspOutput)]
    L.haf_score_batch.argtypes = [E, C.c_int32, C.POINTER(Cloud), C.POINTER(GraspInput), C.POINTER(GraspOutput)]
    L.haf_score_rolls.argtypes = [E, C.c_int32, C.POINTER(Cloud), C.POINTER(GraspInput), C.c_int32, C.c_int32,
                                  C.c_void_p]
    L.haf_finalize.argtypes = [E, C.POINTER(GraspInput), C.c_void_p, C.POINTER(GraspOutput)]
    L.haf_roll_pose.argtypes = [E, C.POINTER(GraspInput), C.c_void_p, C.c_int32, C.POINTER(GraspOutput),
                                C.POINTER(C.c_int32)]
    L.haf_get_roll_grid.argtypes = [E, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.haf_debug_fetch.argtypes = [E, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t]
    L.haf_debug_fetch_attr.argtypes = [E, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.POINTER(C.c_int32)]
    L.haf_top_params_default.argtypes = [E, C.POINTER(TopParams)]
    L.haf_top_params_default.restype = None
    L.haf_top_grasps.argtypes = [E, C.POINTER(TopParams), C.c_void_p, C.c_void_p]
    L.haf_set_stream.argtypes = [E, C.c_void_p]
    L.haf_get_stream.restype = C.c_void_p
    L.haf_get_stream.argtypes = [E]
    L.haf_get_stage_ms.argtypes = [E, C.POINTER(C.c_float)]
    L.haf_model_info.argtypes = [E, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.haf_last_counts.argtypes = [E, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.haf_last_tiers.argtypes = [E] + [C.POINTER(C.c_int64)] * 4
    L.haf_last_prestage.argtypes = [E, C.POINTER(C.c_int64)]
    L.haf_multi_plan.argtypes = [C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                 C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.haf_last_strict_host.argtypes = [E, C.POINTER(C.c_int64)]
    L.haf_last_exact_tiers.argtypes = [E, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.haf_screen_form.argtypes = [E, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.haf_screen_low_rank.argtypes = [E, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.haf_register_host_cloud.argtypes = [E, C.c_void_p, C.c_size_t]
    L.haf_unregister_host_cloud.argtypes = [E, C.c_void_p]
    L.haf_pcd_load.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_size_t), C.c_char_p,
                               C.c_size_t]
    L.haf_free.argtypes = [C.c_void_p]
    L.haf_frame_default.argtypes = [C.POINTER(Frame)]
    L.haf_frame_default.restype = None
    L.haf_frame_points.argtypes = [C.POINTER(Frame), C.c_void_p]
    L.haf_score_frames.argtypes = [E, C.c_int32, C.POINTER(Frame), C.POINTER(GraspInput), C.POINTER(GraspOutput)]
    L.haf_debug_fetch_points.argtypes = [E, C.c_int32, C.c_void_p, C.c_size_t]
    L.haf_view_points.argtypes = [C.POINTER(Frame), C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.haf_score_views.argtypes = [E, C.c_int32, C.POINTER(C.c_int32), C.POINTER(Frame), C.POINTER(GraspInput), C.POINTER(GraspOutput),
                                  C.POINTER(C.c_int64)]
    L.haf_pgm16_load.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_uint16)), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_char_p,
                                 C.c_size_t]
    L.haf_point_cells.argtypes = [C.POINTER(Config), C.POINTER(GraspInput), C.c_int32, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    L.haf_grasp_map_ref.argtypes = [C.POINTER(Config), C.POINTER(GraspInput), C.c_int32, C.c_int32, C.c_void_p, C.POINTER(Frame), C.c_void_p,
                                    C.c_void_p, C.c_void_p]
    L.haf_grasp_map.argtypes = [E, C.c_int32, C.POINTER(Frame), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    L.haf_cell_pose.argtypes = [E, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(GraspCandidate)]
    L.haf_grasp_map_best.argtypes = [E, C.c_int32, C.POINTER(Frame), C.c_void_p, C.c_size_t, C.c_int32, C.POINTER(GraspCandidate),
                                     C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.haf_label_best_ref.argtypes = [C.POINTER(Config), C.POINTER(GraspInput), C.c_int32, C.c_int32, C.c_void_p, C.POINTER(Frame),
                                     C.POINTER(LabelImage), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    L.haf_grasp_map_labels.argtypes = [E, C.c_int32, C.POINTER(Frame), C.POINTER(LabelImage), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.POINTER(C.c_int32)]
    L.haf_score_objects.argtypes = [E, C.POINTER(Frame), C.POINTER(LabelImage), C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(GraspInput),
                                    C.c_int32, C.POINTER(GraspOutput), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    L.haf_roi_cells.argtypes = [C.POINTER(Config), C.POINTER(GraspInput), C.c_int32, C.POINTER(Frame), C.c_void_p, C.c_size_t, C.c_void_p,
                                C.c_void_p]
    L.haf_score_frames_roi.argtypes = [E, C.c_int32, C.POINTER(Frame), C.POINTER(Roi), C.POINTER(GraspInput), C.POINTER(GraspOutput)]
    L.haf_score_views_roi.argtypes = [E, C.c_int32, C.POINTER(C.c_int32), C.POINTER(Frame), C.POINTER(Roi), C.POINTER(GraspInput),
                                      C.POINTER(GraspOutput), C.POINTER(C.c_int64)]
    L.haf_roi_cells_views.argtypes = [C.POINTER(Config), C.POINTER(GraspInput), C.c_int32, C.POINTER(Frame), C.POINTER(Roi), C.c_int32,
                                      C.c_void_p, C.c_void_p]
    L.haf_depth_filter_default.argtypes = [C.POINTER(DepthFilter)]
    L.haf_depth_filter_default.restype = None
    L.haf_filter_depth_ref.argtypes = [C.POINTER(Frame), C.c_int32, C.POINTER(DepthFilter), C.c_void_p, C.c_size_t, C.POINTER(C.c_int64)]
    L.haf_filter_depth.argtypes = [E, C.POINTER(Frame), C.c_int32, C.POINTER(DepthFilter), C.c_void_p, C.c_size_t, C.c_int32, C.POINTER(Frame),
                                   C.POINTER(C.c_int64)]
    L.haf_segment_default.argtypes = [C.POINTER(SegmentParams)]
    L.haf_segment_default.restype = None
    L.haf_segment_ref.argtypes = [C.POINTER(Frame), C.POINTER(SegmentParams), C.c_void_p, C.c_int32, C.c_size_t, C.c_void_p,
                                  C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.haf_segment_frame.argtypes = [E, C.POINTER(Frame), C.POINTER(SegmentParams), C.c_void_p, C.c_int32, C.c_size_t, C.c_int32,
                                    C.POINTER(LabelImage), C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.haf_cell_segment_default.argtypes = [C.POINTER(CellSegmentParams)]
    L.haf_cell_segment_default.restype = None
    L.haf_segment_cells_ref.argtypes = [C.POINTER(Frame), C.POINTER(CellSegmentParams), C.c_void_p, C.c_int32, C.c_size_t, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.haf_segment_cells.argtypes = [E, C.POINTER(Frame), C.POINTER(CellSegmentParams), C.c_void_p, C.c_int32, C.c_size_t, C.c_int32,
                                    C.POINTER(LabelImage), C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.haf_plane_default.argtypes = [C.POINTER(PlaneParams)]
    L.haf_plane_default.restype = None
    L.haf_fit_plane_ref.argtypes = [C.POINTER(Frame), C.POINTER(Roi), C.POINTER(PlaneParams), C.POINTER(PlaneResult), C.c_void_p, C.c_void_p]
    L.haf_fit_plane.argtypes = [E, C.POINTER(Frame), C.POINTER(Roi), C.POINTER(PlaneParams), C.POINTER(PlaneResult), C.c_void_p, C.c_void_p]
    L.haf_gripper_default.argtypes = [C.POINTER(Gripper)]
    L.haf_gripper_default.restype = None
    L.haf_check_grasps_ref.argtypes = [C.POINTER(Frame), C.POINTER(Roi), C.POINTER(Gripper), C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p,
                                       C.c_void_p, C.POINTER(C.c_int32)]
    L.haf_check_grasps.argtypes = [E, C.POINTER(Frame), C.POINTER(Roi), C.POINTER(Gripper), C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p,
                                   C.c_void_p, C.POINTER(C.c_int32)]
    L.haf_opening_default.argtypes = [C.POINTER(OpeningParams)]
    L.haf_opening_default.restype = None
    L.haf_fit_openings_ref.argtypes = [C.POINTER(Frame), C.POINTER(Roi), C.POINTER(Gripper), C.POINTER(OpeningParams), C.c_int32, C.c_void_p,
                                       C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(OpeningInfo), C.c_void_p]
    L.haf_fit_openings.argtypes = [E, C.POINTER(Frame), C.POINTER(Roi), C.POINTER(Gripper), C.POINTER(OpeningParams), C.c_int32, C.c_void_p,
                                   C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(OpeningInfo), C.c_void_p]
    L.haf_apply_opening.argtypes = [C.POINTER(GraspOutput), C.POINTER(GraspOpening), C.POINTER(GraspOutput)]
    L.haf_space_default.argtypes = [C.POINTER(SpaceParams)]
    L.haf_space_default.restype = None
    L.haf_check_space_ref.argtypes = [C.POINTER(Frame), C.c_int32, C.POINTER(Gripper), C.POINTER(SpaceParams), C.c_int32, C.c_void_p, C.c_size_t,
                                      C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(SpaceInfo), C.c_void_p]
    L.haf_check_space.argtypes = [E, C.POINTER(Frame), C.c_int32, C.POINTER(Gripper), C.POINTER(SpaceParams), C.c_int32, C.c_void_p, C.c_size_t,
                                  C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(SpaceInfo), C.c_void_p]
    L.haf_measure_labels_ref.argtypes = [C.POINTER(Frame), C.POINTER(LabelImage), C.c_int32, C.c_void_p, C.c_void_p]
    L.haf_measure_labels.argtypes = [E, C.POINTER(Frame), C.POINTER(LabelImage), C.c_int32, C.c_void_p, C.c_void_p]
    L.haf_object_input.argtypes = [C.POINTER(Config), C.POINTER(GraspInput), C.c_void_p, C.c_int32, C.POINTER(GraspInput), C.POINTER(C.c_int32)]
    L.haf_transfer_default.argtypes = [C.POINTER(TransferParams)]
    L.haf_transfer_default.restype = None
    L.haf_invert_pose.argtypes = [C.c_void_p, C.c_void_p]
    L.haf_transfer_labels_ref.argtypes = [C.POINTER(Frame), C.POINTER(Camera), C.POINTER(LabelImage), C.c_int32, C.POINTER(TransferParams),
                                          C.c_void_p, C.c_int32, C.c_size_t, C.c_void_p, C.POINTER(C.c_int64)]
    L.haf_transfer_labels.argtypes = [E, C.POINTER(Frame), C.POINTER(Camera), C.POINTER(LabelImage), C.c_int32, C.POINTER(TransferParams),
                                      C.c_void_p, C.c_int32, C.c_size_t, C.c_int32, C.POINTER(LabelImage), C.c_void_p, C.POINTER(C.c_int64)]
    # several GPUs in one process (csrc/multi.cpp)
    L.haf_create_multi.argtypes = [C.POINTER(Config), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.POINTER(E)]
    L.haf_destroy_multi.argtypes = [E]
    L.haf_multi_last_error.restype = C.c_char_p
    L.haf_multi_last_error.argtypes = [E]
    L.haf_score_sharded.argtypes = [E, C.POINTER(Cloud), C.POINTER(GraspInput), C.POINTER(GraspOutput)]
    L.haf_score_batch_sharded.argtypes = [E, C.c_int32, C.POINTER(Cloud), C.POINTER(GraspInput), C.POINTER(GraspOutput),
                                          C.POINTER(C.c_int32)]
    L.haf_multi_info.argtypes = [E, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.haf_multi_engine.restype = C.c_void_p
    L.haf_multi_engine.argtypes = [E, C.c_int32]
    L.haf_multi_last_records.argtypes = [E, C.c_int32, C.c_void_p]
    L.haf_multi_last_timing.argtypes = [E, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p]
    if testing:
        L.haf_test_decq_host.restype = C.c_double
        L.haf_test_decq_host.argtypes = [C.c_double, C.c_int]
        L.haf_test_scale_host.restype = C.c_double
        L.haf_test_scale_host.argtypes = [C.c_double] * 5
        L.haf_test_sigma_upper.restype = C.c_double
        L.haf_test_sigma_upper.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.haf_test_table_digest.argtypes = [E, C.c_char_p, C.c_int]
        L.haf_test_host_table_digest.argtypes = [C.POINTER(Config), C.c_double, C.c_double, C.c_char_p, C.c_int, C.c_char_p, C.c_int]
        L.haf_test_decq4_scr.restype = C.c_double
        L.haf_test_decq4_scr.argtypes = [C.c_float]
        L.haf_test_decq4_scr_n.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.haf_test_host_slot_table.argtypes = [C.POINTER(Config), C.c_double, C.c_double, C.c_int] + [C.c_void_p] * 8 + \
            [C.POINTER(C.c_int), C.c_char_p, C.c_int]
        L.haf_test_feature_thresholds.argtypes = [C.c_void_p]
        L.haf_test_feature_form.argtypes = [E, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.haf_test_screen_finish.argtypes = [E, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.haf_test_split3.restype = C.c_double
        L.haf_test_split3.argtypes = [C.c_double, C.c_void_p]
        L.haf_test_decq_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.haf_test_mfma_accum.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.haf_test_mfma_rate.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.haf_test_mfma_model.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.haf_test_scale_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p,
                                            C.c_int]
        L.haf_test_feature_table.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int]
        L.haf_test_range_table.argtypes = [C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                           C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.haf_test_model.argtypes = [C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int),
                                     C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]
        L.haf_test_model_kernel.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.haf_test_roll_geo.argtypes = [C.POINTER(Config), C.POINTER(GraspInput), C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p]
        L.haf_test_finalize.argtypes = [C.POINTER(Config), C.POINTER(GraspInput), C.c_void_p, C.POINTER(GraspOutput)]
        L.haf_test_roll_pose.argtypes = [C.POINTER(Config), C.POINTER(GraspInput), C.c_void_p, C.c_int,
                                         C.POINTER(GraspOutput), C.POINTER(C.c_int32)]
        L.haf_test_mfma_kappa.argtypes = [E, C.c_void_p, C.c_void_p]
        L.haf_test_f16_mfma.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.haf_test_screen_state.argtypes = [E, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double)]
        L.haf_test_set_screen_inactive.argtypes = [E]
        L.haf_test_check_canaries.argtypes = [C.c_char_p, C.c_int]
        L.haf_test_canary_buffers.argtypes = []
        L.haf_test_poke_flag0_list.argtypes = [E, C.c_int, C.c_int, C.c_int]
        L.haf_test_overflow_stats.argtypes = [E, C.c_void_p]
        L.haf_test_fetch_list.argtypes = [E, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.haf_test_snapshot_screen.argtypes = [E, C.c_int]
        L.haf_test_prestage_forms.argtypes = [E, C.c_void_p]
        L.haf_test_fetch_snapshot.argtypes = [E, C.c_int, C.c_longlong, C.c_void_p, C.c_longlong, C.POINTER(C.c_longlong)]
        L.haf_test_sweep_form.argtypes = [E, C.c_int, C.c_void_p]
        L.haf_test_fetch_sweep.argtypes = [E, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_longlong, C.POINTER(C.c_longlong)]
        L.haf_test_host_sweep_tables.argtypes = [C.POINTER(Config), C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_longlong,
                                                 C.POINTER(C.c_longlong), C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
        L.haf_test_host_screen_finish.argtypes = [C.POINTER(Config), C.c_double, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                  C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
        L.haf_test_lr_finish_band.argtypes = [C.POINTER(Config), C.c_double, C.c_double, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_char_p, C.c_int]
        L.haf_test_tier_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]
        L.haf_test_revote.argtypes = [E, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.haf_test_last_batch.argtypes = [E, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.haf_test_top_merge.argtypes = [C.POINTER(Config), C.POINTER(GraspInput), C.c_int] + [C.c_void_p] * 5 + \
            [C.c_int, C.c_int, C.c_double, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    return L


def lib():
    """Loads libhafgrasp.so (the product).  Raises if it has not been built: nothing here falls back to anything else."""
    global _lib
    if _lib is None:
        _lib = _bind(LIB_PATH, testing=False)
    return _lib


def multi_plan(devices, shard_mode, n_rolls):
    """haf_multi_plan: the partition haf_create_multi would build for `devices` (no device is touched).  Raises HafError like
    MultiEngine would.  -> dict(rank_of, slot_of, roll_first, roll_count, n_ranks)"""
    L = lib()
    n = len(devices)
    dev = (C.c_int32 * max(1, n))(*devices)
    rk, sl, rf, rc_ = [(C.c_int32 * max(1, n))() for _ in range(4)]
    nr = C.c_int32()
    rc = L.haf_multi_plan(dev, n, shard_mode, n_rolls, rk, sl, rf, rc_, C.byref(nr))
    if rc != 0:
        raise HafError(rc, L.haf_multi_last_error(None).decode())
    return dict(rank_of=list(rk)[:n], slot_of=list(sl)[:n], roll_first=list(rf)[:n], roll_count=list(rc_)[:n], n_ranks=nr.value)


def testlib():
    """Loads libhafgrasp_testing.so: the same kernels with the haf_test_* hooks and the guard-band environment switches."""
    global _testlib
    if _testlib is None:
        _testlib = _bind(TESTLIB_PATH, testing=True)
    return _testlib


def check_canaries():
    """Testing build: the guard zones in front of and behind EVERY device buffer of every engine of this process (csrc/engine_state.h:
    DevBuf).  -> (number of damaged buffers, report naming them by the source line that allocated them, buffers registered)"""
    L = testlib()
    msg = C.create_string_buffer(4096)
    bad = L.haf_test_check_canaries(msg, 4096)
    return bad, msg.value.decode(errors="replace"), L.haf_test_canary_buffers()


def default_config(**kw):
    cfg = Config()
    lib().haf_config_default(C.byref(cfg))
    for k, v in kw.items():
        if k in ("feature_file", "range_file", "model_file") and isinstance(v, str):
            v = v.encode()
        setattr(cfg, k, v)
    return cfg


def default_input(**kw):
    gi = GraspInput()
    lib().haf_grasp_input_default(C.byref(gi))
    for k, v in kw.items():
        if k in ("grasp_area_center", "approach_vector"):
            v = (C.c_double * 3)(*v)
        setattr(gi, k, v)
    return gi


def output_to_dict(o):
    return dict(eval=o.eval, grasp_point1=tuple(o.grasp_point1), grasp_point2=tuple(o.grasp_point2),
                averaged_grasp_point=tuple(o.averaged_grasp_point), approach_vector=tuple(o.approach_vector),
                roll=o.roll, best_row=o.best_row, best_col=o.best_col, best_roll=o.best_roll, best_vote=o.best_vote,
                rolls_done=o.rolls_done, n_evals=o.n_evals, n_rechecked=o.n_rechecked)


def top_params(engine_handle=None, **kw):
    """haf_top_params_default (min_vote from the engine's graspval_th; haf_config_default's without an engine) with kw overrides"""
    p = TopParams()
    lib().haf_top_params_default(engine_handle, C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError("unknown haf_top_params field %r" % k)
        setattr(p, k, v)
    return p


def candidate_to_dict(c):
    d = output_to_dict(c.grasp)
    d.update(run_length=c.run_length, h_locmax=c.h_locmax)
    return d


def load_pcd(path):
    """PCD file -> float32 [N, 3] through the library's own reader (haf_pcd_load)."""
    p = C.POINTER(C.c_float)()
    n = C.c_size_t()
    err = C.create_string_buffer(256)
    rc = lib().haf_pcd_load(path.encode(), C.byref(p), C.byref(n), err, 256)
    if rc != HAF_OK:
        raise HafError(rc, err.value.decode())
    try:
        return np.ctypeslib.as_array(p, shape=(n.value, 3)).copy()
    finally:
        lib().haf_free(p)


def load_pgm16(path):
    """16-bit binary PGM -> uint16 [height, width] through the library's own reader (haf_pgm16_load)."""
    p = C.POINTER(C.c_uint16)()
    w, h = C.c_int32(), C.c_int32()
    err = C.create_string_buffer(256)
    rc = lib().haf_pgm16_load(path.encode(), C.byref(p), C.byref(w), C.byref(h), err, 256)
    if rc != HAF_OK:
        raise HafError(rc, err.value.decode())
    try:
        return np.ctypeslib.as_array(p, shape=(h.value, w.value)).copy()
    finally:
        lib().haf_free(p)


def default_frame(**kw):
    f = Frame()
    lib().haf_frame_default(C.byref(f))
    for k, v in kw.items():
        if not hasattr(f, k):
            raise TypeError("unknown haf_frame field %r" % k)
        if k == "sensor_to_base":
            v = (C.c_float * 12)(*np.asarray(v, dtype=np.float32).reshape(-1)[:12])
        setattr(f, k, v)
    return f


def _frame_of(kind, data, width, height, on_device, row_stride_bytes, point_stride_bytes, keep, **kw):
    f = default_frame(data=data, kind=kind, width=width, height=height, on_device=on_device, row_stride_bytes=row_stride_bytes,
                      point_stride_bytes=point_stride_bytes, **kw)
    f._keep = keep                  # the array must outlive the frame
    return f


def depth_frame(array, fx, fy, cx, cy, depth_scale=None, min_depth=0.0, max_depth=0.0, sensor_to_base=None, width=None, height=None,
                row_stride_bytes=None, dtype=None):
    """haf_frame of a depth image: a numpy uint16 / float32 [height, width] array (host; its last axis contiguous, rows may be padded:
    a view into a wider array), or a device pointer (int) with width, height and dtype given.  depth_scale defaults to 0.001 for uint16
    and 1 for float32; sensor_to_base is a 3x4 or 4x4 matrix (default: identity)."""
    if isinstance(array, np.ndarray):
        assert array.ndim == 2 and array.dtype in (np.uint16, np.float32) and array.strides[1] == array.itemsize
        dt, on_dev, ptr = array.dtype, 0, array.ctypes.data
        height, width = array.shape
        row_stride_bytes = array.strides[0] if height > 1 else (row_stride_bytes or width * array.itemsize)
    else:
        dt, on_dev, ptr = np.dtype(dtype), 1, int(array)
        assert dt in (np.uint16, np.float32) and width and height
        row_stride_bytes = row_stride_bytes or width * dt.itemsize
    kind = FRAME_DEPTH_U16 if dt == np.uint16 else FRAME_DEPTH_F32
    if depth_scale is None:
        depth_scale = 0.001 if kind == FRAME_DEPTH_U16 else 1.0
    kw = dict(fx=fx, fy=fy, cx=cx, cy=cy, depth_scale=depth_scale, min_depth=min_depth, max_depth=max_depth)
    if sensor_to_base is not None:
        kw["sensor_to_base"] = sensor_to_base
    return _frame_of(kind, ptr, width, height, on_dev, row_stride_bytes, 0, array, **kw)


def xyz_frame(array, sensor_to_base=None, width=None, height=None, row_stride_bytes=None, point_stride_bytes=None):
    """haf_frame of an organised sensor-frame cloud: numpy float32 [height, width, >= 3] (host) or a device pointer with width, height
    and the strides given."""
    if isinstance(array, np.ndarray):
        assert array.ndim == 3 and array.dtype == np.float32 and array.shape[2] >= 3 and array.strides[2] == 4
        height, width = array.shape[:2]
        on_dev, ptr = 0, array.ctypes.data
        point_stride_bytes = array.strides[1] if width > 1 else (point_stride_bytes or array.shape[2] * 4)
        row_stride_bytes = array.strides[0] if height > 1 else (row_stride_bytes or width * point_stride_bytes)
    else:
        on_dev, ptr = 1, int(array)
        point_stride_bytes = point_stride_bytes or 12
        row_stride_bytes = row_stride_bytes or width * point_stride_bytes
    kw = {} if sensor_to_base is None else dict(sensor_to_base=sensor_to_base)
    return _frame_of(FRAME_XYZ_F32, ptr, width, height, on_dev, row_stride_bytes, point_stride_bytes, array, **kw)


def cloud_frame(xyz):
    """an unorganised base-frame cloud (float32 [N, >= 3], host) as a haf_frame: N x 1 points of HAF_FRAME_XYZ_F32 under the identity pose,
    what haf_segment_cells, haf_measure_labels and haf_score_objects take for a cloud; its label image is [1, N]"""
    xyz = np.asarray(xyz)
    assert xyz.ndim == 2 and xyz.dtype == np.float32 and xyz.shape[1] >= 3 and xyz.strides[1] == 4
    return xyz_frame(xyz.reshape(1, xyz.shape[0], xyz.shape[1]), point_stride_bytes=xyz.strides[0])


def frame_points(frame):
    """haf_frame_points: the host definition of record -> float32 [height * width, 3]"""
    out = np.empty((max(0, frame.width) * max(0, frame.height), 3), np.float32)
    rc = lib().haf_frame_points(C.byref(frame), out.ctypes.data)
    if rc != HAF_OK:
        raise HafError(rc, "haf_frame_points refused the frame")
    return out


MAX_VIEWS = 16
MAX_STACK = 8                        # HAF_MAX_STACK: exposures of one haf_filter_depth call


def depth_filter(**kw):
    """haf_depth_filter with the library's defaults (radius 2, min_support 6, tol_abs 0.004, tol_rel 0.01, min_valid 1) and `kw` over them"""
    p = DepthFilter()
    lib().haf_depth_filter_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError("unknown haf_depth_filter field %r" % k)
        setattr(p, k, v)
    return p


def _filter_image(frame, out):
    """the host output image of a filter call for exposures like `frame`: `out` (uint16 / float32 [height, width], rows may be padded) or a
    new packed one -> (array, pointer, row stride)"""
    dt = np.uint16 if frame.kind == FRAME_DEPTH_U16 else np.float32
    if out is None or out is True:
        out = np.empty((max(0, frame.height), max(0, frame.width)), dt)
    assert out.ndim == 2 and out.dtype == dt and out.shape == (frame.height, frame.width) and out.strides[1] == out.itemsize
    return out, out.ctypes.data, out.strides[0] if frame.height > 1 else frame.width * out.itemsize


def filter_depth_ref(frames, params=None, out=None):
    """haf_filter_depth_ref: the host definition of record of the depth filter on `frames` (1..8 host Frames, exposures of one depth
    camera) -> (image: uint16 / float32 [height, width], stats: [pixels, valid after the temporal stage, kept]).  out: the array to
    write into (rows may be padded: a view into a wider array)."""
    L, n = lib(), len(frames)
    arr = (Frame * max(1, n))(*frames)
    p = params if params is not None else depth_filter()
    img, ptr, stride = _filter_image(arr[0], out)
    stats = (C.c_int64 * 3)()
    rc = L.haf_filter_depth_ref(arr, n, C.byref(p), ptr, stride, stats)
    if rc != HAF_OK:
        raise HafError(rc, "haf_filter_depth_ref refused its arguments")
    return img, [int(x) for x in stats]


def segment_params(**kw):
    """haf_segment_params with the library's defaults (plane (0, 0, 1, 0), min_height 0.01, max_height 0 = none, max_gap 0.02, min_pixels
    50, max_labels 255) and `kw` over them; plane: four floats"""
    p = SegmentParams()
    lib().haf_segment_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError("unknown haf_segment_params field %r" % k)
        if k == "plane":
            v = (C.c_float * 4)(*np.asarray(v, dtype=np.float32).reshape(-1)[:4])
        setattr(p, k, v)
    return p


def _label_out(frame, dtype, out):
    """the host label image of a segment call for `frame`: `out` (uint8 / uint16 [height, width], rows may be padded) or a new packed one
    -> (array, pointer, element size, row stride)"""
    dt = np.dtype(dtype)
    assert dt in (np.uint8, np.uint16)
    if out is None:
        out = np.empty((max(0, frame.height), max(0, frame.width)), dt)
    assert out.ndim == 2 and out.dtype == dt and out.shape == (frame.height, frame.width) and out.strides[1] == out.itemsize
    return out, out.ctypes.data, dt.itemsize, out.strides[0] if frame.height > 1 else frame.width * dt.itemsize


def _label_target(frame, dtype, device_out, host_out, got):
    """where a label-writing engine call for `frame` writes, from the arguments of Engine.segment: -> (labels pointer, element size, row
    stride, out_on_device, what the method returns as its labels): device_out=True the engine's own image, device_out a pointer or
    (pointer, row_stride_bytes) the caller's -- both returned as `got`, the LabelImage the call fills -- else the host array of _label_out"""
    if device_out is True:
        return None, np.dtype(dtype).itemsize, 0, 1, got
    if device_out is not False and device_out is not None:
        ptr, stride = device_out if isinstance(device_out, tuple) else (device_out, 0)
        elem = np.dtype(dtype).itemsize
        return int(ptr), elem, stride or frame.width * elem, 1, got
    img, ptr, elem, stride = _label_out(frame, dtype, host_out)
    return ptr, elem, stride, 0, img


def segment_ref(frame, params=None, dtype=np.uint8, out=None):
    """haf_segment_ref: the host definition of record of the tabletop segmentation of a host Frame -> (labels: uint8 / uint16 [height,
    width], infos: SEGMENT_INFO_DTYPE [n_labels], stats: [pixels, foreground, components, components that pass the size rule]).
    out: the array to write into (rows may be padded: a view into a wider array)."""
    p = params if params is not None else segment_params()
    img, ptr, elem, stride = _label_out(frame, dtype, out)
    info = np.zeros(max(1, p.max_labels), SEGMENT_INFO_DTYPE)
    n, stats = C.c_int32(-1), (C.c_int64 * 4)()
    rc = lib().haf_segment_ref(C.byref(frame), C.byref(p), ptr, elem, stride, info.ctypes.data, C.byref(n), stats)
    if rc != HAF_OK:
        raise HafError(rc, "haf_segment_ref refused its arguments")
    return img, info[:n.value].copy(), [int(x) for x in stats]


def cell_segment_params(**kw):
    """haf_cell_segment_params with the library's defaults (plane (0, 0, 1, 0), min_height 0.01, max_height 0 = none, cell 0.01, origin
    (-5.12, -5.12), 1024 x 1024 cells, connectivity 8, max_step 0 = none, min_points 50, max_labels 255) and `kw` over them"""
    p = CellSegmentParams()
    lib().haf_cell_segment_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError("unknown haf_cell_segment_params field %r" % k)
        if k == "plane":
            v = (C.c_float * 4)(*np.asarray(v, dtype=np.float32).reshape(-1)[:4])
        setattr(p, k, v)
    return p


def segment_cells_ref(frame, params=None, dtype=np.uint8, out=None, cell_labels=False):
    """haf_segment_cells_ref: the host definition of record of the top-down cell clustering of a host Frame of any shape -> (labels: uint8
    / uint16 [height, width], infos: CELL_SEGMENT_INFO_DTYPE [n_labels], stats: [pixels, foreground, foreground outside the grid,
    occupied cells, components, components that pass the size rule]) and, with cell_labels=True, the uint16 [ny, nx] label grid as a
    fourth entry.  out: the array to write into (rows may be padded: a view into a wider array)."""
    p = params if params is not None else cell_segment_params()
    img, ptr, elem, stride = _label_out(frame, dtype, out)
    info = np.zeros(max(1, p.max_labels), CELL_SEGMENT_INFO_DTYPE)
    grid = np.zeros((max(0, p.ny), max(0, p.nx)), np.uint16) if cell_labels else None
    n, stats = C.c_int32(-1), (C.c_int64 * 6)()
    rc = lib().haf_segment_cells_ref(C.byref(frame), C.byref(p), ptr, elem, stride, grid.ctypes.data if cell_labels else None, info.ctypes.data,
                                     C.byref(n), stats)
    if rc != HAF_OK:
        raise HafError(rc, "haf_segment_cells_ref refused its arguments")
    res = (img, info[:n.value].copy(), [int(x) for x in stats])
    return res + (grid,) if cell_labels else res


def plane_params(**kw):
    """haf_plane_params with the library's defaults (tol 0.005, min_area2 1e-6, up (0, 0, 0) = no tilt test, max_tilt 0, n_hyp 256,
    min_inliers 100, seed 1) and `kw` over them; up: three floats"""
    p = PlaneParams()
    lib().haf_plane_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError("unknown haf_plane_params field %r" % k)
        if k == "up":
            v = (C.c_float * 3)(*np.asarray(v, dtype=np.float32).reshape(-1)[:3])
        setattr(p, k, v)
    return p


def _plane_mask(frame, mask):
    """None, a host mask (uint8 [height, width], rows may be padded) or a device mask ((device_ptr, row_stride_bytes)) -> (Roi or None, keep-alive)"""
    if mask is None:
        return None, None
    if isinstance(mask, tuple):
        return Roi(int(mask[0]), int(mask[1]), 1), None
    keep, ptr, stride = _host_mask(mask, frame)
    return Roi(ptr, stride, 0), keep


def _plane_result(res, n_hyp, counts, hyps, debug):
    out = dict(plane=np.array(list(res.plane), np.float32), found=bool(res.found), winner=int(res.winner), n_inliers=int(res.n_inliers),
               rms=float(res.rms), stats=[int(x) for x in res.stats])
    if debug:
        out.update(moments=[int(x) for x in res.moments], counts=counts[:n_hyp].copy(), hyps=hyps[:n_hyp].copy())
    return out


def fit_plane_ref(frame, params=None, mask=None, debug=False):
    """haf_fit_plane_ref: the host definition of record of the dominant plane of a host Frame -> dict(plane: float32 [4], assignable to
    segment_params(plane=...); found, winner, n_inliers, rms, stats: [pixels, usable, hypotheses that are not void, best count]).
    mask: uint8 [height, width], a non-zero byte admits the pixel.  debug=True adds moments (ten ints), counts (int32 [n_hyp]) and hyps
    (float32 [n_hyp, 4]: the un-normalised n and d of every hypothesis)."""
    p = params if params is not None else plane_params()
    roi, keep = _plane_mask(frame, mask)
    res, counts, hyps = PlaneResult(), np.zeros(MAX_PLANE_HYP, np.int32), np.zeros((MAX_PLANE_HYP, 4), np.float32)
    rc = lib().haf_fit_plane_ref(C.byref(frame), C.byref(roi) if roi is not None else None, C.byref(p), C.byref(res),
                                 counts.ctypes.data if debug else None, hyps.ctypes.data if debug else None)
    if rc != HAF_OK:
        raise HafError(rc, "haf_fit_plane_ref refused its arguments")
    return _plane_result(res, p.n_hyp, counts, hyps, debug)


def gripper(**kw):
    """haf_gripper with the library's defaults (opening 0.08, finger_thickness 0.01, finger_breadth 0.02, tip_depth 0.03, finger_length
    0.06, palm 0.12 x 0.04 x 0.04, max_hits 0, min_between 1 -- nominal figures, no real gripper's) and `kw` over them"""
    g = Gripper()
    lib().haf_gripper_default(C.byref(g))
    for k, v in kw.items():
        if not hasattr(g, k):
            raise TypeError("unknown haf_gripper field %r" % k)
        setattr(g, k, v)
    return g


def _grasp_array(grasps):
    """a list of the dicts top_grasps / best_per_label / score give (the four pose fields are read), or a ctypes array of GraspOutput or
    GraspCandidate -> (ctypes array, count, stride in bytes)"""
    if isinstance(grasps, C.Array):
        return grasps, len(grasps), C.sizeof(grasps._type_)
    arr = (GraspOutput * max(1, len(grasps)))()
    for o, g in zip(arr, grasps):
        for f in ("grasp_point1", "grasp_point2", "averaged_grasp_point", "approach_vector"):
            setattr(o, f, (C.c_double * 3)(*[float(x) for x in g[f]]))
    return arr, len(grasps), C.sizeof(GraspOutput)


def _check_grasps(call, frame, grasps, grip, mask):
    g = grip if grip is not None else gripper()
    roi, keep = _plane_mask(frame, mask)
    arr, n, stride = _grasp_array(grasps)
    out, order, nf = np.zeros(max(1, n), CLEARANCE_DTYPE), np.zeros(max(1, n), np.int32), C.c_int32(0)
    rc = call(C.byref(frame), C.byref(roi) if roi is not None else None, C.byref(g), n, arr, stride, out.ctypes.data, order.ctypes.data, C.byref(nf))
    return rc, out[:n], order[:nf.value].copy()


def check_grasps_ref(frame, grasps, gripper=None, mask=None):
    """haf_check_grasps_ref: the host definition of record of the gripper's clearance at every grasp against the points of a host Frame
    -> (CLEARANCE_DTYPE [n_grasps], order: the indices of the free grasps in input order).  grasps: a list of grasp dicts or a ctypes
    array of GraspOutput / GraspCandidate; gripper: gripper(...), default the library's nominal one; mask: uint8 [height, width], a
    non-zero byte admits the pixel."""
    rc, out, order = _check_grasps(lib().haf_check_grasps_ref, frame, grasps, gripper, mask)
    if rc != HAF_OK:
        raise HafError(rc, "haf_check_grasps_ref refused its arguments")
    return out, order


def opening_params(**kw):
    """haf_opening_params with the library's defaults (min_opening 0.01, max_opening 0.08, max_shift 0, max_hits 0, min_between 1) and
    `kw` over them"""
    p = OpeningParams()
    lib().haf_opening_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError("unknown haf_opening_params field %r" % k)
        setattr(p, k, v)
    return p


def _fit_openings(call, frame, grasps, grip, params, mask, hist):
    g = grip if grip is not None else gripper()
    p = params if params is not None else opening_params()
    roi, keep = _plane_mask(frame, mask)
    arr, n, stride = _grasp_array(grasps)
    out, order, nf, info = np.zeros(max(1, n), OPENING_DTYPE), np.zeros(max(1, n), np.int32), C.c_int32(0), OpeningInfo()
    words = np.zeros((max(1, n), 2, OPEN_BINS), np.uint32) if hist else None
    rc = call(C.byref(frame), C.byref(roi) if roi is not None else None, C.byref(g), C.byref(p), n, arr, stride, out.ctypes.data,
              order.ctypes.data, C.byref(nf), C.byref(info), words.ctypes.data if hist else None)
    facts = {f: getattr(info, f) for f, _ in OpeningInfo._fields_ if f != "reserved"}
    return rc, (out[:n], order[:nf.value].copy(), facts) + ((words[:n], ) if hist else ())


def fit_openings_ref(frame, grasps, gripper=None, params=None, mask=None, hist=False):
    """haf_fit_openings_ref: the host definition of record of the smallest free opening at every grasp against the points of a host
    Frame -> (OPENING_DTYPE [n_grasps], order: the indices of the found grasps in input order, info: dict of haf_opening_info's fields)
    and, with hist=True, the histograms uint32 [n_grasps, 2, 128] as a fourth entry.  grasps, gripper and mask as check_grasps_ref's
    (the gripper's opening is not read); params: opening_params(...), default the library's."""
    rc, res = _fit_openings(lib().haf_fit_openings_ref, frame, grasps, gripper, params, mask, hist)
    if rc != HAF_OK:
        raise HafError(rc, "haf_fit_openings_ref refused its arguments")
    return res


def apply_opening(grasp, opening):
    """haf_apply_opening: a grasp dict and its OPENING_DTYPE record (found == 1) -> the dict with averaged_grasp_point moved by shift_m
    along the closing axis and the grasp points at -+ opening_m / 2 about it; every other entry is the input's"""
    arr, _, _ = _grasp_array([grasp])
    rec = GraspOpening.from_buffer_copy(np.asarray(opening, OPENING_DTYPE).tobytes())
    out = GraspOutput()
    rc = lib().haf_apply_opening(C.byref(arr[0]), C.byref(rec), C.byref(out))
    if rc != HAF_OK:
        raise HafError(rc, "haf_apply_opening: a void grasp, or an opening that was not found")
    return dict(grasp, grasp_point1=tuple(out.grasp_point1), grasp_point2=tuple(out.grasp_point2),
                averaged_grasp_point=tuple(out.averaged_grasp_point))


def space_params(**kw):
    """haf_space_params with the library's defaults (sample_step 0.004, near_m 0.05, tol_abs 0.004, tol_rel 0.002, max_hit 0, max_unknown
    0, min_between_hit 1 -- nominal figures) and `kw` over them"""
    p = SpaceParams()
    lib().haf_space_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError("unknown haf_space_params field %r" % k)
        setattr(p, k, v)
    return p


def _check_space(call, views, grasps, grip, params, states):
    g = grip if grip is not None else gripper()
    p = params if params is not None else space_params()
    views = list(views) if isinstance(views, (list, tuple)) else [views]
    arr, n, stride = _grasp_array(grasps)
    frames = (Frame * max(1, len(views)))(*views)
    out, order, nc, info = np.zeros(max(1, n), SPACE_DTYPE), np.zeros(max(1, n), np.int32), C.c_int32(0), SpaceInfo()
    # (N is the call's to say: what is offered always fits min(n * MAX_SPACE_SAMPLES, MAX_SPACE_STATES) bytes)
    st = np.zeros(min(max(1, n) * MAX_SPACE_SAMPLES, MAX_SPACE_STATES), np.uint8) if states else None
    rc = call(frames, len(views), C.byref(g), C.byref(p), n, arr, stride, out.ctypes.data, order.ctypes.data, C.byref(nc), C.byref(info),
              st.ctypes.data if states else None)
    facts = dict(step=info.step, n=[list(r) for r in info.n], n_samples=info.n_samples)
    res = (out[:n], order[:nc.value].copy(), facts)
    if states and rc == HAF_OK:
        res += (st[:n * info.n_samples].reshape(n, info.n_samples).copy(), )
    return rc, res


def check_space_ref(views, grasps, gripper=None, params=None, states=False):
    """haf_check_space_ref: the host definition of record of what 1..8 host depth Frames have seen of the gripper's volume at every grasp
    -> (SPACE_DTYPE [n_grasps], order: the indices of the clear grasps in input order, info: dict(step, n [4][3], n_samples)) and, with
    states=True, every sample's final rank uint8 [n_grasps, n_samples] as a fourth entry.  views: a Frame or a list of them; grasps and
    gripper as check_grasps_ref's; params: space_params(...), default the library's."""
    rc, res = _check_space(lib().haf_check_space_ref, views, grasps, gripper, params, states)
    if rc != HAF_OK:
        raise HafError(rc, "haf_check_space_ref refused its arguments")
    return res


def _shape_plane(plane):
    """None or four floats -> (pointer or None, keep-alive)"""
    if plane is None:
        return None, None
    keep = np.ascontiguousarray(np.asarray(plane, dtype=np.float32).reshape(-1)[:4])
    assert keep.size == 4
    return keep.ctypes.data, keep


def measure_labels_ref(frame, labels, n_labels=None, plane=None):
    """haf_measure_labels_ref: the host definition of record of every label's box in the base frame.  frame: a host Frame; labels: a host
    uint8 / uint16 [height, width] array (label_image()); plane: None or the four floats of a segment_params plane, for the heights
    -> LABEL_SHAPE_DTYPE [n_labels] (label l is entry l - 1)."""
    img, n_labels = label_image(labels, frame, n_labels)
    ptr, keep = _shape_plane(plane)
    shapes = np.zeros(max(1, n_labels), LABEL_SHAPE_DTYPE)
    rc = lib().haf_measure_labels_ref(C.byref(frame), C.byref(img), n_labels, ptr, shapes.ctypes.data)
    if rc != HAF_OK:
        raise HafError(rc, "haf_measure_labels_ref refused its arguments")
    return shapes[:n_labels]


def camera(width, height, fx, fy, cx, cy, base_to_camera=None, sensor_to_base=None):
    """haf_camera: the camera a label image belongs to.  base_to_camera: a 3x4 or 4x4 matrix, base frame -> the camera's frame (default:
    identity); or sensor_to_base, the camera's pose as a Frame carries it, which invert_pose() turns into it."""
    if sensor_to_base is not None:
        assert base_to_camera is None
        base_to_camera = invert_pose(sensor_to_base)
    m = np.eye(4, dtype=np.float32)[:3] if base_to_camera is None else np.asarray(base_to_camera, dtype=np.float32).reshape(-1)[:12]
    return Camera(width, height, fx, fy, cx, cy, (C.c_float * 12)(*np.asarray(m, dtype=np.float32).reshape(-1)))


def transfer_params(**kw):
    """haf_transfer_params with the library's defaults (near_m 0.05, tol_abs 0.01, tol_rel 0.01, splat 1) and `kw` over them"""
    p = TransferParams()
    lib().haf_transfer_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError("unknown haf_transfer_params field %r" % k)
        setattr(p, k, v)
    return p


def invert_pose(pose):
    """haf_invert_pose: the inverse of a 3x4 (or the first three rows of a 4x4) affine, in double, rounded once -> float32 [3, 4]"""
    m = np.ascontiguousarray(np.asarray(pose, dtype=np.float32).reshape(-1)[:12])
    assert m.size == 12
    out = np.zeros(12, np.float32)
    rc = lib().haf_invert_pose(m.ctypes.data, out.ctypes.data)
    if rc != HAF_OK:
        raise HafError(rc, "haf_invert_pose refused the pose (an entry that is not finite, or a singular matrix)")
    return out.reshape(3, 4)


def transfer_labels_ref(depth, cam, cam_labels, n_labels=None, params=None, dtype=np.uint8, out=None, zbuffer=False):
    """haf_transfer_labels_ref: the host definition of record of a camera's label image carried over to a depth frame.  depth: a host
    Frame of any kind; cam: a Camera; cam_labels: a host uint8 / uint16 [cam.height, cam.width] array (label_image()) -> (labels:
    uint8 / uint16 [height, width] on the depth frame, stats: [pixels, in front of the camera, projecting, visible, labelled]);
    zbuffer=True appends the int32 [cam.height, cam.width] z-buffer.  out: the array to write into (rows may be padded)."""
    img, n_labels = label_image(cam_labels, cam, n_labels)
    p = params if params is not None else transfer_params()
    lab, ptr, elem, stride = _label_out(depth, dtype, out)
    z = np.zeros((max(0, cam.height), max(0, cam.width)), np.int32) if zbuffer else None
    stats = (C.c_int64 * 5)()
    rc = lib().haf_transfer_labels_ref(C.byref(depth), C.byref(cam), C.byref(img), n_labels, C.byref(p), ptr, elem, stride,
                                       z.ctypes.data if zbuffer else None, stats)
    if rc != HAF_OK:
        raise HafError(rc, "haf_transfer_labels_ref refused its arguments")
    res = (lab, [int(x) for x in stats])
    return res + (z,) if zbuffer else res


def shape_to_dict(shape):
    """one entry of a LABEL_SHAPE_DTYPE array -> dict of plain Python values (lists for the arrays)"""
    return {k: (shape[k].tolist() if np.ndim(shape[k]) else shape[k].item()) for k in LABEL_SHAPE_DTYPE.names if k != "reserved"}


def object_input(cfg, base, shape, margin_cells=4):
    """haf_object_input: the GraspInput `base` re-centred on the box of `shape` (one entry of a LABEL_SHAPE_DTYPE array) with a square
    grasp area that covers the object and margin_cells more cells under every roll -> (GraspInput, fits); fits is False when the area
    had to be cut to the engine's grid (Config `cfg`)."""
    one = np.zeros(1, LABEL_SHAPE_DTYPE)
    one[0] = shape
    out, fits = GraspInput(), C.c_int32(-1)
    rc = lib().haf_object_input(C.byref(cfg), C.byref(base), one.ctypes.data, margin_cells, C.byref(out), C.byref(fits))
    if rc != HAF_OK:
        raise HafError(rc, "haf_object_input refused its arguments")
    return out, bool(fits.value)


def view_points(frames):
    """haf_view_points: the host definition of record of a request's fused cloud -- the valid points of `frames` (host Frames), frame
    after frame in pixel order -> float32 [n_valid, 3]"""
    L, n = lib(), len(frames)
    arr = (Frame * max(1, n))(*frames)
    cnt = C.c_size_t()
    rc = L.haf_view_points(arr, n, None, 0, C.byref(cnt))
    if rc == HAF_OK:
        out = np.empty((cnt.value, 3), np.float32)
        rc = L.haf_view_points(arr, n, out.ctypes.data, cnt.value, C.byref(cnt))
    if rc != HAF_OK:
        raise HafError(rc, (L.haf_last_error(None) or b"").decode())
    return out


def point_cells(cfg, grasp_input, roll, xyz):
    """haf_point_cells: the cell row * grid_w + col of every point of float32 [N, >= 3] `xyz` under roll `roll` (global index) of
    `grasp_input` on the grids of Config `cfg`, or -1 -> int32 [N].  Host definition of record: no device, no engine."""
    a = np.ascontiguousarray(xyz, dtype=np.float32)
    assert a.ndim == 2 and a.shape[1] >= 3
    out = np.empty(a.shape[0], np.int32)
    rc = lib().haf_point_cells(C.byref(cfg), C.byref(grasp_input), roll, a.ctypes.data, a.shape[0], a.shape[1], out.ctypes.data)
    if rc != HAF_OK:
        raise HafError(rc, "haf_point_cells refused its arguments")
    return out


def grasp_map_ref(cfg, grasp_input, roll_first, eval_grids, frame, want=("vote", "roll", "cell")):
    """haf_grasp_map_ref: the host definition of record of a grasp map.  eval_grids: float32 [roll_count, grid_h, grid_w] as
    Engine.roll_grid returns them for the rolls roll_first .. of one request; frame: a host Frame
    -> dict(vote int16 [height, width], roll int16, cell int32), only the images named in `want`."""
    g = np.ascontiguousarray(eval_grids, dtype=np.float32).reshape(-1, cfg.grid_h, cfg.grid_w)
    shape = (max(0, frame.height), max(0, frame.width))
    out = {k: np.empty(shape, np.int32 if k == "cell" else np.int16) for k in want}
    ptr = lambda k: out[k].ctypes.data if k in out else None
    rc = lib().haf_grasp_map_ref(C.byref(cfg), C.byref(grasp_input), roll_first, g.shape[0], g.ctypes.data if g.size else None, C.byref(frame),
                                 ptr("vote"), ptr("roll"), ptr("cell"))
    if rc != HAF_OK:
        raise HafError(rc, "haf_grasp_map_ref refused its arguments")
    return out


def _host_mask(mask, frame):
    """uint8 [height, width] with contiguous rows (they may be padded: a view into a wider array) -> (array to keep, pointer, row stride)"""
    keep = np.asarray(mask)
    assert keep.dtype == np.uint8 and keep.shape == (frame.height, frame.width) and (keep.shape[1] == 1 or keep.strides[1] == 1)
    if keep.shape[0] > 1 and keep.strides[0] < keep.shape[1]:
        keep = np.ascontiguousarray(keep)
    return keep, keep.ctypes.data, (keep.strides[0] if keep.shape[0] > 1 else keep.shape[1])


def label_image(labels, frame, n_labels=None):
    """-> (LabelImage, n_labels) for `labels`: a numpy uint8 / uint16 [height, width] array (host; rows may be padded: a view into a
    wider array; n_labels defaults to the image's maximum, at least 1), a device tensor of such a shape (anything with data_ptr(), element_size() and
    stride(): a torch tensor, possibly a view), (device_ptr, elem_bytes, row_stride_bytes), or a LabelImage as it is (what
    Engine.segment(..., device_out=True) returns); n_labels must be given for device images."""
    if isinstance(labels, LabelImage):
        img, keep = labels, getattr(labels, "_keep", None)
    elif isinstance(labels, tuple):
        ptr, eb, stride = (int(x) for x in labels)
        img, keep = LabelImage(ptr, eb, 1, stride), None
    elif hasattr(labels, "data_ptr"):
        assert tuple(labels.shape) == (frame.height, frame.width) and (frame.width == 1 or labels.stride(1) == 1)
        eb = labels.element_size()
        img, keep = LabelImage(labels.data_ptr(), eb, 1, labels.stride(0) * eb if frame.height > 1 else frame.width * eb), labels
    else:
        keep = np.asarray(labels)
        assert keep.dtype in (np.uint8, np.uint16) and keep.shape == (frame.height, frame.width)
        if (keep.shape[1] > 1 and keep.strides[1] != keep.itemsize) or (keep.shape[0] > 1 and keep.strides[0] < keep.shape[1] * keep.itemsize):
            keep = np.ascontiguousarray(keep)
        if n_labels is None:
            n_labels = max(1, int(keep.max()) if keep.size else 0)      # (an image without any object: one label, not found)
        img = LabelImage(keep.ctypes.data, keep.itemsize, 0, keep.strides[0] if keep.shape[0] > 1 else keep.shape[1] * keep.itemsize)
    if n_labels is None:
        raise TypeError("n_labels must be given for a device-resident label image")
    img._keep = keep
    return img, int(n_labels)


def _label_result(picks, order, n_found, poses=None):
    out = dict(picks=picks, order=[int(x) for x in order[:n_found]])
    if poses is not None:
        out["poses"] = [candidate_to_dict(poses[k]) if picks["found"][k] else None for k in range(len(picks))]
    return out


def label_best_ref(cfg, grasp_input, roll_first, eval_grids, frame, labels, n_labels=None, min_vote=1):
    """haf_label_best_ref: the host definition of record of the best pixel per instance label.  eval_grids and frame as grasp_map_ref
    takes them; labels: a host uint8 / uint16 [height, width] array -> dict(picks: LABEL_PICK_DTYPE [n_labels] (label l is entry
    l - 1), order: the found labels, best pick first)"""
    g = np.ascontiguousarray(eval_grids, dtype=np.float32).reshape(-1, cfg.grid_h, cfg.grid_w)
    img, n_labels = label_image(labels, frame, n_labels)
    picks = np.zeros(max(1, n_labels), LABEL_PICK_DTYPE)
    order = np.zeros(max(1, n_labels), np.int32)
    nf = C.c_int32(0)
    rc = lib().haf_label_best_ref(C.byref(cfg), C.byref(grasp_input), roll_first, g.shape[0], g.ctypes.data if g.size else None, C.byref(frame),
                                  C.byref(img), n_labels, min_vote, picks.ctypes.data, order.ctypes.data, C.byref(nf))
    if rc != HAF_OK:
        raise HafError(rc, "haf_label_best_ref refused its arguments")
    return _label_result(picks[:n_labels], order, nf.value)


def roi_cells(cfg, grasp_input, roll, frame, mask, want=("roi", "eval")):
    """haf_roi_cells: the host definition of record of haf_score_frames_roi's cell sets for roll `roll` (global index) -- roi: the cells
    of the masked pixels' points, eval: their dilation by the vote's 29-tap footprint (before the test of the search area)
    -> dict of uint8 [grid_h, grid_w], only the grids named in `want`.  frame: a host Frame; mask: uint8 [height, width]."""
    keep, ptr, stride = _host_mask(mask, frame)
    out = {k: np.empty((cfg.grid_h, cfg.grid_w), np.uint8) for k in want}
    p = lambda k: out[k].ctypes.data if k in out else None
    rc = lib().haf_roi_cells(C.byref(cfg), C.byref(grasp_input), roll, C.byref(frame), ptr, stride, p("roi"), p("eval"))
    if rc != HAF_OK:
        raise HafError(rc, "haf_roi_cells refused its arguments")
    return out


def _rois(frames, masks):
    """per frame a host mask (uint8 [height, width]), a device mask ((device_ptr, row_stride_bytes)) or None -> (Roi array, keep-alive)"""
    rois = (Roi * max(1, len(frames)))()
    keep = []
    for k, m in enumerate(masks):
        if m is None:
            rois[k] = Roi(None, 0, 0)
        elif isinstance(m, tuple):
            rois[k] = Roi(int(m[0]), int(m[1]), 1)
        else:
            kk, ptr, stride = _host_mask(m, frames[k])
            keep.append(kk)
            rois[k] = Roi(ptr, stride, 0)
    return rois, keep


def roi_cells_views(cfg, grasp_input, roll, frames, masks, want=("roi", "eval")):
    """haf_roi_cells_views: the host definition of record of haf_score_views_roi's cell sets for roll `roll` (global index) -- roi: the
    union over the views of the cells of their masked pixels' points, eval: its dilation by the vote's footprint -> dict of uint8
    [grid_h, grid_w], only the grids named in `want`.  frames: host Frames; masks: per frame uint8 [height, width] or None."""
    frames = list(frames)
    if len(masks) != len(frames):
        raise HafError(HAF_E_ARG, "roi_cells_views: one mask (or None) per frame")
    arr = (Frame * max(1, len(frames)))(*frames)
    rois, keep = _rois(frames, masks)
    out = {k: np.empty((cfg.grid_h, cfg.grid_w), np.uint8) for k in want}
    p = lambda k: out[k].ctypes.data if k in out else None
    rc = lib().haf_roi_cells_views(C.byref(cfg), C.byref(grasp_input), roll, arr, rois, len(frames), p("roi"), p("eval"))
    if rc != HAF_OK:
        raise HafError(rc, "haf_roi_cells_views refused its arguments")
    return out


class Engine:
    """Owns one haf_engine handle (one GPU)."""

    def __init__(self, feature_file, range_file, model_file, testing=False, **cfg):
        self._L = testlib() if testing else lib()
        self.cfg = default_config(feature_file=feature_file, range_file=range_file, model_file=model_file, **cfg)
        self._h = C.c_void_p()
        rc = self._L.haf_create(C.byref(self.cfg), C.byref(self._h))
        if rc != HAF_OK:
            raise HafError(rc, (self._L.haf_last_error(None) or b"").decode())

    def close(self):
        if getattr(self, "_h", None):
            self._L.haf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != HAF_OK:
            raise HafError(rc, (self._L.haf_last_error(self._h) or b"").decode())

    def register_host(self, arr):
        """haf_register_host_cloud: page-locks the numpy array's buffer; clouds passed as views into it then go with on_device = 2
        (DMA straight from the caller's memory).  The array must outlive the registration."""
        assert isinstance(arr, np.ndarray) and arr.flags["C_CONTIGUOUS"]
        self._check(self._L.haf_register_host_cloud(self._h, C.c_void_p(arr.ctypes.data), arr.nbytes))
        if not hasattr(self, "_regs"):
            self._regs = []
        self._regs.append((arr.ctypes.data, arr.nbytes, arr))

    def unregister_host(self, arr):
        self._check(self._L.haf_unregister_host_cloud(self._h, C.c_void_p(arr.ctypes.data)))
        self._regs = [r for r in getattr(self, "_regs", []) if r[0] != arr.ctypes.data]

    def _cloud(self, xyz):
        """numpy float32 [N, >=3] (host; inside a register_host buffer: page-locked, on_device = 2) or (device_ptr, n_points,
        stride_floats) tuple (HBM resident)."""
        if isinstance(xyz, tuple):
            ptr, n, stride = xyz
            return Cloud(C.c_void_p(ptr), n, stride, 1), None
        a = np.ascontiguousarray(xyz, dtype=np.float32)
        assert a.ndim == 2 and a.shape[1] >= 3
        where = 0
        if a.shape[1] == 3:
            for base, nbytes, _ in getattr(self, "_regs", []):
                if base <= a.ctypes.data and a.ctypes.data + a.nbytes <= base + nbytes:
                    where = 2
        return Cloud(a.ctypes.data_as(C.c_void_p), a.shape[0], a.shape[1], where), a

    def model_info(self):
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._L.haf_model_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(n_sv=a.value, dim=b.value, n_features=c.value)

    def last_counts(self):
        a, r, b, c = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._L.haf_last_tiers(self._h, C.byref(a), C.byref(r), C.byref(b), C.byref(c)))
        return dict(n_evals=a.value, n_refined=r.value, n_rechecked=b.value, n_strict=c.value)

    def fetch_list(self, which, cap=1 << 22):
        """Testing build: a device list of the last request as it lies in memory (0 evaluation cells, 1 exact tiers' input, 2 exact-integer
        tier's hand-over, 3 strict tier's, 4 screening pass's)."""
        buf = np.empty(cap, dtype=np.int32)
        n = C.c_int()
        self._check(self._L.haf_test_fetch_list(self._h, which, buf.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
        return buf[:min(n.value, cap)].copy()

    BIN_FORMS = ("k_bin", "k_bin_lds", "k_bin_tiles", "k_small_pre<true>", "k_bin_lds+k_small_pre<false>")
    INTEGRAL_FORMS = ("k_integral_small", "k_integral_band", "k_small_pre")

    def prestage_forms(self):
        """Testing build (haf_test_prestage_forms): which pre-stage kernels served the last request -- bin (index into BIN_FORMS),
        integral (index into INTEGRAL_FORMS), bucket_refused (the bucket-sorted binning path was refused because the grid's bucket count
        exceeds its LDS histogram) and n_inexact_grids."""
        out = (C.c_int * 4)()
        self._check(self._L.haf_test_prestage_forms(self._h, out))
        return dict(bin=out[0], integral=out[1], bucket_refused=bool(out[2]), n_inexact_grids=out[3])

    FEATURE_FORMS = ("k_features_small", "k_features<16>", "k_features<8>", "k_features_serial", "k_features_serial<lr>")

    def feature_form(self, per_roll=False):
        """Testing build (haf_test_feature_form): which feature kernel served the last request's screening pass (index into FEATURE_FORMS;
        -1: none ran) and which ScreenParams set it read -> dict(kernel, params: index into SCREEN_PARAMS, cr_poly).  per_roll: also
        flags and iiabs, what the pre-stages left per (cloud, roll) for the low-rank form: the flags word (bit 1: the grid holds a
        negative height) and the sum of |height| in units of 2^-20 m."""
        form, n = (C.c_int * 3)(), C.c_int()
        self._check(self._L.haf_test_feature_form(self._h, form, None, None, 0, C.byref(n)))
        out = dict(kernel=form[0], params=form[1], cr_poly=bool(form[2]))
        if per_roll:
            flags, iiabs = np.zeros(max(1, n.value), np.int32), np.zeros(max(1, n.value), np.uint64)
            self._check(self._L.haf_test_feature_form(self._h, form, flags.ctypes.data_as(C.c_void_p), iiabs.ctypes.data_as(C.c_void_p),
                                                      len(flags), C.byref(n)))
            out.update(flags=flags[:n.value], iiabs=iiabs[:n.value])
        return out

    SCREEN_PARAMS = ("screen", "screen_cr", "screen_lrp")

    def screen_finish(self, sums):
        """Testing build (haf_test_screen_finish): screen_finish on the host with the constants the last screening feature pass was launched
        with, for sums [n, 5] = su2, sd2, sx2, cr, ub (fp64) -> (band [n, 8] fp32, a_x [n] fp32)."""
        sums = np.ascontiguousarray(sums, np.float64)
        assert sums.ndim == 2 and sums.shape[1] == 5
        band, nax = np.zeros((len(sums), 8), np.float32), np.zeros(len(sums), np.float32)
        self._check(self._L.haf_test_screen_finish(self._h, sums.ctypes.data_as(C.c_void_p), len(sums), band.ctypes.data_as(C.c_void_p),
                                                   nax.ctypes.data_as(C.c_void_p)))
        return band, nax

    def snapshot_screen(self, on=True):
        """Testing build: from now on every request keeps a copy of what its screening feature pass wrote (fetch_snapshot)."""
        self._check(self._L.haf_test_snapshot_screen(self._h, 1 if on else 0))

    def fetch_snapshot(self, which, offset=0, nbytes=None):
        """Testing build: bytes of the last request's snapshot as uint8 -- which = 0 the fp16 operand images (20 KiB per tile of 32
        evaluations), 1 the 8 band floats per evaluation (the raw sums in the low-rank form), 2 a_x."""
        avail = C.c_longlong()
        self._check(self._L.haf_test_fetch_snapshot(self._h, which, 0, None, 0, C.byref(avail)))
        if nbytes is None:
            nbytes = avail.value - offset
        buf = np.empty(max(0, nbytes), dtype=np.uint8)
        if nbytes > 0:
            self._check(self._L.haf_test_fetch_snapshot(self._h, which, offset, buf.ctypes.data_as(C.c_void_p), nbytes, C.byref(avail)))
        return buf

    SWEEP_PARTS = ("dec", "margin", "words", "list", "counters", "part", "in_X", "in_gband", "in_ax", "labels", "raw", "Y")
    _SWEEP_DTYPES = (np.float32, np.float32, np.uint64, np.int32, np.int32, np.float32, np.uint8, np.float32, np.float32, np.int8, np.float32, np.uint8)

    def sweep_form(self, slot=0):
        """Testing build (haf_test_sweep_form): which sweep launch `slot` (0 the first pass, 1 tier 0b) of the last request was, as its
        launcher reported it -> dict(variant: SCREEN_* of the kernel, -1 when there was no such launch; lr, part, fused, gather, list:
        bool; compaction: 0 one workgroup, 1 two launches; blocks; cap: the evaluation slots the launch covered)."""
        out = (C.c_longlong * 9)()
        self._check(self._L.haf_test_sweep_form(self._h, slot, out))
        return dict(variant=int(out[0]), lr=bool(out[1]), part=bool(out[2]), fused=bool(out[3]), gather=bool(out[4]), list=bool(out[5]),
                    compaction=int(out[6]), blocks=int(out[7]), cap=int(out[8]))

    def fetch_sweep(self, what, slot=0):
        """Testing build (haf_test_fetch_sweep; snapshot_screen must be on): what sweep launch `slot` of the last request left, copied
        right behind the launch -- `what` one of SWEEP_PARTS: dec and margin [cap] fp32, the flag words uint64, the output list int32
        [flag0_cap], the counters int32 as they stood behind the launch, part (PART form: float32 [16, blocks * 256, 4]) and, for tier
        0b's list-image form, its list-indexed operand images (uint8), bands and a_x; labels: the label grids int8 (every cell of the
        engine's grids); raw: the raw sums a low-rank sweep read; Y: the 6-step images k_project wrote (uint8, two-launch form)."""
        which = self.SWEEP_PARTS.index(what)
        avail = C.c_longlong()
        self._check(self._L.haf_test_fetch_sweep(self._h, slot, which, 0, None, 0, C.byref(avail)))
        buf = np.empty(max(0, avail.value), dtype=np.uint8)
        if avail.value > 0:
            self._check(self._L.haf_test_fetch_sweep(self._h, slot, which, 0, buf.ctypes.data_as(C.c_void_p), avail.value, C.byref(avail)))
        return buf.view(self._SWEEP_DTYPES[which])

    def revote(self, labels=None, gridf=None, heights=None, roi_words=None):
        """Testing build (haf_test_revote): replaces the last scored batch's B x R grids by `labels` (int8 [B, R, H, W]; a plain engine)
        or `gridf` (float32; an engine with FLAG_PROBABILITY), optionally its height grids (float32 [B, R, H, W]) and ROI cell sets
        (uint64 [B, R, H, (W + 63) // 64]; needs an earlier score_frames_roi), and runs the request path's vote launchers on them
        -> the roll records [B, R].  roll_grid, top_grasps, grasp_map, best_in_mask and cell_pose then describe the re-voted grids."""
        H, W = self.cfg.grid_h, self.cfg.grid_w
        if (labels is None) == (gridf is None):
            raise HafError(HAF_E_ARG, "revote: exactly one of labels and gridf")
        # the hook reads B x R grids of the LAST BATCH from every pointer it is given: the arrays must have exactly that shape
        b, r = C.c_int(), C.c_int()
        self._check(self._L.haf_test_last_batch(self._h, C.byref(b), C.byref(r)))
        B, R = b.value, r.value
        if B < 1 or R < 1:                                   # no scored batch: the hook refuses before it reads anything
            B, R = np.shape(labels if labels is not None else gridf)[:2]
        for a in (labels, gridf, heights):
            if a is not None and np.shape(a) != (B, R, H, W):
                raise HafError(HAF_E_ARG, "revote: an array of shape %r, the last batch is %r" % (np.shape(a), (B, R, H, W)))
        if roi_words is not None and np.shape(roi_words) != (B, R, H, (W + 63) // 64):
            raise HafError(HAF_E_ARG, "revote: roi_words of shape %r, the last batch needs %r" % (np.shape(roi_words), (B, R, H, (W + 63) // 64)))
        keep = []

        def ptr(a, dt, shape):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt)
            assert a.shape == shape, (a.shape, shape)
            keep.append(a)
            return a.ctypes.data
        rec = np.zeros((B, R), dtype=ROLL_RECORD_DTYPE)
        self._check(self._L.haf_test_revote(self._h, ptr(labels, np.int8, (B, R, H, W)), ptr(gridf, np.float32, (B, R, H, W)),
                                            ptr(heights, np.float32, (B, R, H, W)), ptr(roi_words, np.uint64, (B, R, H, (W + 63) // 64)),
                                            rec.ctypes.data))
        return rec

    def overflow_stats(self):
        """Testing build: how often this engine's requests met a list smaller than what it had to hold."""
        out = (C.c_longlong * 2)()
        self._check(self._L.haf_test_overflow_stats(self._h, out))
        return dict(screening_list_overflows=int(out[0]), extra_windows=int(out[1]))

    def last_exact_tiers(self):
        a, b = C.c_int64(), C.c_int64()
        self._check(self._L.haf_last_exact_tiers(self._h, C.byref(a), C.byref(b)))
        return dict(n_integer=a.value, n_fp64=b.value)

    def last_strict_host(self):
        a = C.c_int64()
        self._check(self._L.haf_last_strict_host(self._h, C.byref(a)))
        return a.value

    def last_prestage(self):
        a = C.c_int64()
        self._check(self._L.haf_last_prestage(self._h, C.byref(a)))
        return dict(n_inexact_grids=a.value)

    def score(self, xyz, grasp_input):
        return self.score_batch([xyz], [grasp_input])[0]

    def score_batch(self, clouds, inputs):
        n = len(clouds)
        keep = []
        arr = (Cloud * n)()
        for i, c in enumerate(clouds):
            arr[i], k = self._cloud(c)
            keep.append(k)
        gi = (GraspInput * n)(*inputs)
        out = (GraspOutput * n)()
        self._check(self._L.haf_score_batch(self._h, n, arr, gi, out))
        self._last_points = [int(c.n_points) for c in arr]
        return [output_to_dict(o) for o in out]

    def score_frames(self, frames, inputs):
        """haf_score_frames: one Frame (depth_frame / xyz_frame) and one GraspInput per request of the batch"""
        n = len(frames)
        arr = (Frame * n)(*frames)
        gi = (GraspInput * n)(*inputs)
        out = (GraspOutput * n)()
        self._check(self._L.haf_score_frames(self._h, n, arr, gi, out))
        self._last_points = [f.width * f.height for f in frames]
        return [output_to_dict(o) for o in out]

    def score_frames_roi(self, frames, masks, inputs):
        """haf_score_frames_roi: score_frames with, per request, a pixel mask over its frame -- only the cells near the cells of the
        masked pixels are evaluated.  masks[b]: uint8 [height, width] (host; rows may be padded), or (device_ptr, row_stride_bytes)."""
        n = len(frames)
        arr = (Frame * max(1, n))(*frames)
        rois = (Roi * max(1, n))()
        keep = []
        for b, m in enumerate(masks):
            if isinstance(m, tuple):
                rois[b] = Roi(int(m[0]), int(m[1]), 1)
            else:
                k, ptr, stride = _host_mask(m, frames[b])
                keep.append(k)
                rois[b] = Roi(ptr, stride, 0)
        gi = (GraspInput * max(1, n))(*inputs)
        out = (GraspOutput * max(1, n))()
        self._check(self._L.haf_score_frames_roi(self._h, n, arr, rois, gi, out))
        self._last_points = [f.width * f.height for f in frames]
        return [output_to_dict(o) for o in out[:n]]

    def score_views(self, view_sets, inputs):
        """haf_score_views: per request a list of Frames (its views, fused on the device into one cloud of their valid points) and one
        GraspInput -> (outputs, valid points per request)"""
        n = len(view_sets)
        flat = [f for vs in view_sets for f in vs]
        arr = (Frame * max(1, len(flat)))(*flat)
        per = (C.c_int32 * max(1, n))(*[len(vs) for vs in view_sets])
        gi = (GraspInput * max(1, n))(*inputs)
        out = (GraspOutput * max(1, n))()
        cnt = (C.c_int64 * max(1, n))()
        self._check(self._L.haf_score_views(self._h, n, per, arr, gi, out, cnt))
        counts = [int(c) for c in cnt[:n]]
        self._last_points = [max(0, c) for c in counts]
        return [output_to_dict(o) for o in out[:n]], counts

    def score_views_roi(self, view_sets, mask_sets, inputs):
        """haf_score_views_roi: score_views with a pixel mask per view -- mask_sets[b][v] goes with view_sets[b][v]: uint8 [height, width]
        (host; rows may be padded), (device_ptr, row_stride_bytes), or None for a view that contributes its points and selects nothing
        -> (outputs, valid points per request)"""
        n = len(view_sets)
        flat = [f for vs in view_sets for f in vs]
        masks = [m for ms in mask_sets for m in ms]
        if [len(ms) for ms in mask_sets] != [len(vs) for vs in view_sets]:
            raise HafError(HAF_E_ARG, "score_views_roi: one mask (or None) per view")
        arr = (Frame * max(1, len(flat)))(*flat)
        rois, keep = _rois(flat, masks)
        per = (C.c_int32 * max(1, n))(*[len(vs) for vs in view_sets])
        gi = (GraspInput * max(1, n))(*inputs)
        out = (GraspOutput * max(1, n))()
        cnt = (C.c_int64 * max(1, n))()
        self._check(self._L.haf_score_views_roi(self._h, n, per, arr, rois, gi, out, cnt))
        counts = [int(c) for c in cnt[:n]]
        self._last_points = [max(0, c) for c in counts]
        return [output_to_dict(o) for o in out[:n]], counts

    def fetch_points(self, cloud, n_points=None):
        """debug_points under the name of the C function: after score_views the request's fused cloud, its valid points in the order
        the device compacted them (unspecified; sort the rows to compare)"""
        return self.debug_points(cloud, n_points)

    def debug_points(self, cloud, n_points=None):
        """haf_debug_fetch_points: cloud `cloud` of the last batch as the kernels read it -> float32 [n_points, 3] (KEEP_DEBUG).
        n_points defaults to the cloud's size in the last score_frames / score_batch call made through this object."""
        if n_points is None:
            n_points = getattr(self, "_last_points", [])[cloud]
        out = np.empty((n_points, 3), np.float32)
        self._check(self._L.haf_debug_fetch_points(self._h, cloud, out.ctypes.data, n_points))
        return out

    def score_rolls(self, clouds, inputs, roll_first, roll_count):
        n = len(clouds)
        keep = []
        arr = (Cloud * n)()
        for i, c in enumerate(clouds):
            arr[i], k = self._cloud(c)
            keep.append(k)
        gi = (GraspInput * n)(*inputs)
        rec = np.zeros((n, roll_count), dtype=ROLL_RECORD_DTYPE)
        self._check(self._L.haf_score_rolls(self._h, n, arr, gi, roll_first, roll_count, rec.ctypes.data))
        return rec

    def finalize(self, grasp_input, records):
        rec = np.ascontiguousarray(records, dtype=ROLL_RECORD_DTYPE)
        assert rec.shape == (self.cfg.n_rolls,)
        out = GraspOutput()
        self._check(self._L.haf_finalize(self._h, C.byref(grasp_input), rec.ctypes.data, C.byref(out)))
        return output_to_dict(out)

    def roll_pose(self, grasp_input, records, roll):
        """One roll's own hypothesis (server.cpp:962-969): (output dict, published flag)."""
        rec = np.ascontiguousarray(records, dtype=ROLL_RECORD_DTYPE)
        assert rec.shape == (self.cfg.n_rolls,)
        out, pub = GraspOutput(), C.c_int32()
        self._check(self._L.haf_roll_pose(self._h, C.byref(grasp_input), rec.ctypes.data, roll, C.byref(out), C.byref(pub)))
        return output_to_dict(out), bool(pub.value)

    def top_grasps(self, **params):
        """haf_top_grasps: ranked, suppressed candidates of the last scored batch -> one list of candidate dicts per cloud
        (output_to_dict fields + run_length, h_locmax).  params: k, min_vote, cell_radius, roll_window, min_dist_m."""
        p = top_params(self._h, **params)
        cap = max(1, self.cfg.max_clouds)
        out = (GraspCandidate * (cap * min(1024, max(1, p.k))))()
        n = (C.c_int32 * cap)(*([-1] * cap))          # the call fills one entry per cloud of the last batch
        self._check(self._L.haf_top_grasps(self._h, C.byref(p), out, n))
        return [[candidate_to_dict(out[b * p.k + i]) for i in range(n[b])] for b in range(cap) if n[b] >= 0]

    def grasp_map(self, request, frame, want=("vote", "roll", "cell"), device_out=None):
        """haf_grasp_map: the last batch's votes in the pixels of `frame` (a Frame, host or device-resident, scored or not)
        -> dict(vote int16 [height, width], roll int16 (global roll index, -1 without a cell), cell int32 (row * grid_w + col, or -1)),
        only the images named in `want`; a pixel without a cell has vote MAP_NO_CELL.  device_out: dict name -> device pointer of a
        packed width * height image; the images are then written there and None is returned."""
        if device_out is not None:
            self._check(self._L.haf_grasp_map(self._h, request, C.byref(frame), device_out.get("vote"), device_out.get("roll"),
                                              device_out.get("cell"), 1))
            return None
        shape = (max(0, frame.height), max(0, frame.width))
        out = {k: np.empty(shape, np.int32 if k == "cell" else np.int16) for k in want}
        ptr = lambda k: out[k].ctypes.data if k in out else None
        self._check(self._L.haf_grasp_map(self._h, request, C.byref(frame), ptr("vote"), ptr("roll"), ptr("cell"), 0))
        return out

    def filter_depth(self, frames, params=None, device_out=None, host_out=None):
        """haf_filter_depth: 1..8 exposures of one depth camera (Frames, host or device-resident) -> (frame, stats): one conditioned depth
        image as a Frame of the exposures' kind and parameters, ready for score_frames, score_views, their _roi forms and the grasp maps,
        and [pixels, valid after the temporal stage, kept].  Without an output argument the frame is the engine's own device image, valid
        until the next filter_depth or close().  device_out: a device pointer, or (pointer, row_stride_bytes), of the caller's image (as
        grasp_map's: written there; the caller keeps it alive).  host_out: True for a new numpy image, or the array to write into (rows
        may be padded); the frame then keeps it alive and frame.image is the array."""
        n = len(frames)
        arr = (Frame * max(1, n))(*frames)
        p = params if params is not None else depth_filter()
        got, stats = Frame(), (C.c_int64 * 3)()
        keep = None
        if host_out is not None and host_out is not False:
            keep, ptr, stride = _filter_image(arr[0], host_out)
            rc = self._L.haf_filter_depth(self._h, arr, n, C.byref(p), ptr, stride, 0, C.byref(got), stats)
        elif device_out is not None:
            ptr, stride = device_out if isinstance(device_out, tuple) else (device_out, 0)
            stride = stride or arr[0].width * (2 if arr[0].kind == FRAME_DEPTH_U16 else 4)
            rc = self._L.haf_filter_depth(self._h, arr, n, C.byref(p), int(ptr), stride, 1, C.byref(got), stats)
        else:
            rc = self._L.haf_filter_depth(self._h, arr, n, C.byref(p), None, 0, 1, C.byref(got), stats)
        self._check(rc)
        got._keep = keep
        got.image = keep
        return got, [int(x) for x in stats]

    def segment(self, frame, params=None, dtype=np.uint8, device_out=False, host_out=None):
        """haf_segment_frame: a Frame (any kind, host or device-resident) -> (labels, infos, stats) as segment_ref gives them, computed on
        the device.  labels is a new uint8 / uint16 [height, width] array (host_out: the array to write into, rows may be padded).
        device_out=True: the engine's own packed device image, returned as a LabelImage (valid until the next segment, segment_cells or close(), across
        scoring and map calls; as uint8 its data is also a device mask for score_frames_roi); device_out=(pointer, row_stride_bytes) or a
        pointer: the caller's device image, likewise described by the LabelImage returned."""
        p = params if params is not None else segment_params()
        info = np.zeros(max(1, p.max_labels), SEGMENT_INFO_DTYPE)
        n, stats, got = C.c_int32(-1), (C.c_int64 * 4)(), LabelImage()
        ptr, elem, stride, on_device, img = _label_target(frame, dtype, device_out, host_out, got)
        self._check(self._L.haf_segment_frame(self._h, C.byref(frame), C.byref(p), ptr, elem, stride, on_device, C.byref(got), info.ctypes.data,
                                              C.byref(n), stats))
        return img, info[:n.value].copy(), [int(x) for x in stats]

    def segment_cells(self, frame, params=None, dtype=np.uint8, device_out=False, host_out=None, cell_labels=False):
        """haf_segment_cells: a Frame of any kind and shape (host or device-resident) -> what segment_cells_ref gives, computed on the
        device.  The outputs are segment()'s: a new host array (host_out: the array to write into), device_out=True for the engine's own
        packed device image -- the same image segment(..., device_out=True) uses -- or device_out=(pointer, row_stride_bytes) for the
        caller's.  cell_labels=True appends the uint16 [ny, nx] label grid."""
        p = params if params is not None else cell_segment_params()
        info = np.zeros(max(1, p.max_labels), CELL_SEGMENT_INFO_DTYPE)
        grid = np.zeros((max(0, p.ny), max(0, p.nx)), np.uint16) if cell_labels else None
        gptr = grid.ctypes.data if cell_labels else None
        n, stats, got = C.c_int32(-1), (C.c_int64 * 6)(), LabelImage()
        ptr, elem, stride, on_device, img = _label_target(frame, dtype, device_out, host_out, got)
        self._check(self._L.haf_segment_cells(self._h, C.byref(frame), C.byref(p), ptr, elem, stride, on_device, C.byref(got), gptr,
                                              info.ctypes.data, C.byref(n), stats))
        res = (img, info[:n.value].copy(), [int(x) for x in stats])
        return res + (grid,) if cell_labels else res

    def fit_plane(self, frame, params=None, mask=None, debug=False):
        """haf_fit_plane: a Frame (any kind, host or device-resident) -> the dict fit_plane_ref gives, computed on the device.  mask: a host
        uint8 [height, width] array or (device_ptr, row_stride_bytes)."""
        p = params if params is not None else plane_params()
        roi, keep = _plane_mask(frame, mask)
        res, counts, hyps = PlaneResult(), np.zeros(MAX_PLANE_HYP, np.int32), np.zeros((MAX_PLANE_HYP, 4), np.float32)
        self._check(self._L.haf_fit_plane(self._h, C.byref(frame), C.byref(roi) if roi is not None else None, C.byref(p), C.byref(res),
                                          counts.ctypes.data if debug else None, hyps.ctypes.data if debug else None))
        return _plane_result(res, p.n_hyp, counts, hyps, debug)

    def check_grasps(self, frame, grasps, gripper=None, mask=None):
        """haf_check_grasps: a Frame (any kind, host or device-resident) and grasps -> what check_grasps_ref gives, computed on the
        device.  mask: a host uint8 [height, width] array or (device_ptr, row_stride_bytes)."""
        rc, out, order = _check_grasps(lambda *a: self._L.haf_check_grasps(self._h, *a), frame, grasps, gripper, mask)
        self._check(rc)
        return out, order

    def fit_openings(self, frame, grasps, gripper=None, params=None, mask=None, hist=False):
        """haf_fit_openings: a Frame (any kind, host or device-resident) and grasps -> what fit_openings_ref gives, computed on the
        device.  mask: a host uint8 [height, width] array or (device_ptr, row_stride_bytes); hist=True copies the histograms back."""
        rc, res = _fit_openings(lambda *a: self._L.haf_fit_openings(self._h, *a), frame, grasps, gripper, params, mask, hist)
        self._check(rc)
        return res

    def check_space(self, views, grasps, gripper=None, params=None, states=False):
        """haf_check_space: 1..8 depth Frames (each host or device-resident) and grasps -> what check_space_ref gives, computed on the
        device: (SPACE_DTYPE rows, order, info[, states])."""
        rc, res = _check_space(lambda *a: self._L.haf_check_space(self._h, *a), views, grasps, gripper, params, states)
        self._check(rc)
        return res

    def measure_labels(self, frame, labels, n_labels=None, plane=None):
        """haf_measure_labels: a Frame (any kind, host or device-resident) and its label image (label_image(): a numpy uint8 / uint16
        array, a device tensor, a device pointer tuple, or the LabelImage segment(..., device_out=True) returned) -> the array
        measure_labels_ref gives, computed on the device in one pass.  plane: None or four floats, for the heights."""
        img, n_labels = label_image(labels, frame, n_labels)
        ptr, keep = _shape_plane(plane)
        shapes = np.zeros(max(1, n_labels), LABEL_SHAPE_DTYPE)
        self._check(self._L.haf_measure_labels(self._h, C.byref(frame), C.byref(img), n_labels, ptr, shapes.ctypes.data))
        return shapes[:n_labels]

    def transfer_labels(self, depth, cam, cam_labels, n_labels=None, params=None, dtype=np.uint8, device_out=False, host_out=None,
                        zbuffer=False):
        """haf_transfer_labels: a depth Frame (any kind, host or device-resident), a Camera and its label image (label_image(): a numpy
        uint8 / uint16 [cam.height, cam.width] array, a device tensor, a device pointer tuple or a LabelImage) -> (labels, stats) as
        transfer_labels_ref gives them, computed on the device; zbuffer=True appends the int32 [cam.height, cam.width] z-buffer.  The
        outputs are segment()'s: a new host array (host_out: the array to write into), device_out=True for the engine's own packed
        device image -- the same image segment(..., device_out=True) uses -- or device_out=(pointer, row_stride_bytes) for the caller's."""
        img, n_labels = label_image(cam_labels, cam, n_labels)
        p = params if params is not None else transfer_params()
        z = np.zeros((max(0, cam.height), max(0, cam.width)), np.int32) if zbuffer else None
        zptr = z.ctypes.data if zbuffer else None
        stats, got = (C.c_int64 * 5)(), LabelImage()
        ptr, elem, stride, on_device, lab = _label_target(depth, dtype, device_out, host_out, got)
        self._check(self._L.haf_transfer_labels(self._h, C.byref(depth), C.byref(cam), C.byref(img), n_labels, C.byref(p), ptr, elem, stride,
                                                on_device, C.byref(got), zptr, stats))
        res = (lab, [int(x) for x in stats])
        return res + (z,) if zbuffer else res

    def cell_pose(self, request, roll, row, col):
        """haf_cell_pose: the pose of cell (row, col) of roll `roll` (global index) of request `request` of the last batch -> candidate dict"""
        c = GraspCandidate()
        self._check(self._L.haf_cell_pose(self._h, request, roll, row, col, C.byref(c)))
        return candidate_to_dict(c)

    def best_in_mask(self, request, frame, mask=None, min_vote=1):
        """haf_grasp_map_best: the best pixel of grasp_map(request, frame) among those `mask` (uint8 [height, width], None: all) selects
        and whose vote is >= min_vote -- vote descending, roll, v, u ascending -> (candidate dict, u, v), or None when none qualifies"""
        ptr, stride, keep = None, 0, None
        if mask is not None:
            keep, ptr, stride = _host_mask(mask, frame)
        c, u, v, found = GraspCandidate(), C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
        self._check(self._L.haf_grasp_map_best(self._h, request, C.byref(frame), ptr, stride, min_vote, C.byref(c), C.byref(u), C.byref(v),
                                               C.byref(found)))
        return (candidate_to_dict(c), u.value, v.value) if found.value else None

    def best_per_label(self, request, frame, labels, n_labels=None, min_vote=1):
        """haf_grasp_map_labels: the best pixel of grasp_map(request, frame) for every instance of a label image (label_image(): a numpy
        uint8 / uint16 array, a device tensor or a device pointer tuple) in one device pass -> dict(picks: LABEL_PICK_DTYPE [n_labels]
        (label l is entry l - 1), poses: per label the candidate dict of cell_pose at its pick or None, order: the found labels, best
        pick first)"""
        img, n_labels = label_image(labels, frame, n_labels)
        picks = np.zeros(max(1, n_labels), LABEL_PICK_DTYPE)
        order = np.zeros(max(1, n_labels), np.int32)
        poses = (GraspCandidate * max(1, n_labels))()
        nf = C.c_int32(0)
        self._check(self._L.haf_grasp_map_labels(self._h, request, C.byref(frame), C.byref(img), n_labels, min_vote, picks.ctypes.data, poses,
                                                 order.ctypes.data, C.byref(nf)))
        return _label_result(picks[:n_labels], order, nf.value, poses)

    def score_objects(self, frame, labels, n_labels, object_labels, inputs, min_vote=1):
        """haf_score_objects: every listed object of a label image (label_image(): a numpy uint8 / uint16 array, a device tensor, a device
        pointer tuple or the LabelImage segment(..., device_out=True) returned) as an ROI request of its own on ONE frame -- request b is
        inputs[b] under the mask `labels == object_labels[b]` -- and each object's pick from its own request, in one call
        -> (outputs: a dict per object, picks: LABEL_PICK_DTYPE [n_objects], poses: per object the candidate dict of its pick or None,
        order: the indices b of the found objects, best pick first).  Afterwards the last batch is those n_objects ROI requests."""
        img, n_labels = label_image(labels, frame, n_labels)
        n = len(object_labels)
        ol = (C.c_int32 * max(1, n))(*[int(l) for l in object_labels])
        gi = (GraspInput * max(1, n))(*inputs)
        out = (GraspOutput * max(1, n))()
        picks = np.zeros(max(1, n), LABEL_PICK_DTYPE)
        order = np.zeros(max(1, n), np.int32)
        poses = (GraspCandidate * max(1, n))()
        nf = C.c_int32(0)
        self._check(self._L.haf_score_objects(self._h, C.byref(frame), C.byref(img), n_labels, n, ol, gi, min_vote, out, picks.ctypes.data, poses,
                                              order.ctypes.data, C.byref(nf)))
        self._last_points = [frame.width * frame.height] * n
        res = _label_result(picks[:n], order, nf.value, poses)
        return [output_to_dict(o) for o in out[:n]], res["picks"], res["poses"], res["order"]

    def debug_attr(self, cloud, roll):
        """Attribute records of the masked cells of (cloud, roll): cells [n, 2], records [n, 324], computed [n]."""
        n = C.c_int32()
        self._check(self._L.haf_debug_fetch_attr(self._h, cloud, roll, 0, None, None, None, C.byref(n)))
        cells = np.zeros((n.value, 2), np.int32)
        attr = np.zeros((n.value, 324), ATTR_RECORD_DTYPE)
        comp = np.zeros(n.value, np.uint8)
        if n.value:
            self._check(self._L.haf_debug_fetch_attr(self._h, cloud, roll, n.value, cells.ctypes.data, attr.ctypes.data,
                                                     comp.ctypes.data, C.byref(n)))
        return cells, attr, comp.astype(bool)

    def roll_grid(self, cloud, roll):
        H, W = self.cfg.grid_h, self.cfg.grid_w
        ev = np.zeros((H, W), np.float32)
        mask = np.zeros((H, W), np.uint8)
        self._check(self._L.haf_get_roll_grid(self._h, cloud, roll, ev.ctypes.data, mask.ctypes.data))
        return ev, mask

    def debug(self, what, cloud, roll):
        H, W = self.cfg.grid_h, self.cfg.grid_w
        shape, dt = {DBG_HEIGHTS: ((H, W), np.float32), DBG_INTEGRAL: ((H + 1, W + 1), np.float32),
                     DBG_MASK: ((H, W), np.uint8), DBG_LABELS: ((H, W), np.int8), DBG_DECISION: ((H, W), np.float64),
                     DBG_TRANSFORM: ((4, 4), np.float32), DBG_SCREEN_MARGIN: ((H, W), np.float32),
                     DBG_PROBABILITY: ((H, W, 2), np.float64), DBG_GRASPSGRID: ((H, W), np.float32), DBG_ROI: ((H, W), np.uint8)}[what]
        a = np.zeros(shape, dt)
        self._check(self._L.haf_debug_fetch(self._h, what, cloud, roll, a.ctypes.data, a.nbytes))
        return a

    SCREEN_FORMS = ("plain", "sumsq", "centred-remainder/exp", "centred-remainder/poly")

    def screen_form(self):
        """haf_screen_form: the form of the screening kernel that serves the model, or "off" (three-pass kernel for everything)."""
        f, a = C.c_int32(), C.c_int32()
        self._check(self._L.haf_screen_form(self._h, C.byref(f), C.byref(a)))
        return self.SCREEN_FORMS[f.value] if a.value else "off"

    def screen_state(self):
        """TESTING build: which form of the screening pass serves the model (0 plain, 1 sumsq, 2 centred-remainder with exp, 3 with the
        polynomial), whether the pass is on, and the undecided share of every form on the calibration scene (-1: not tried)."""
        v, a, sh = C.c_int(), C.c_int(), (C.c_double * 4)()
        self._check(self._L.haf_test_screen_state(self._h, C.byref(v), C.byref(a), sh))
        return dict(variant=v.value & 15, tier0b=bool(v.value & 16), tier1_skipped=bool(v.value & 32), low_rank=bool(v.value & 64), active=bool(a.value),
                    shares=list(sh))

    def screen_low_rank(self):
        """haf_screen_low_rank: (tables available, rank of the HAF attributes' span, the last request's screening pass ran in the low-rank form)."""
        a, r, u = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._L.haf_screen_low_rank(self._h, C.byref(a), C.byref(r), C.byref(u)))
        return dict(available=bool(a.value), rank=r.value, last_used=bool(u.value))

    def set_screen_inactive(self):
        """TESTING build: switches the screening pass off as the adaptive rule does after a request every form failed on."""
        self._check(self._L.haf_test_set_screen_inactive(self._h))

    def set_stream(self, hip_stream_ptr):
        """haf_set_stream: every later call enqueues all its work on this hipStream_t (an int: torch's stream.cuda_stream; 0 or None is
        HIP's default stream, torch.cuda.default_stream()).  The caller keeps the stream alive while it is current; the handle
        get_stream() gave before the first switch is the engine's own stream and switches back to it."""
        self._check(self._L.haf_set_stream(self._h, C.c_void_p(hip_stream_ptr or None)))

    def get_stream(self):
        """haf_get_stream: the current stream's handle as an int (0: HIP's default stream)"""
        return int(self._L.haf_get_stream(self._h) or 0)

    def stage_ms(self):
        ms = (C.c_float * len(STAGES))()
        self._check(self._L.haf_get_stage_ms(self._h, ms))
        return dict(zip(STAGES, list(ms)))


class MultiEngine:
    """Owns one haf_multi handle: several GPUs of one node in this process, RCCL collectives behind the C-ABI."""

    def __init__(self, feature_file, range_file, model_file, devices, shard_mode=SHARD_ROLLS, **cfg):
        self._L = lib()
        self.cfg = default_config(feature_file=feature_file, range_file=range_file, model_file=model_file, **cfg)
        self.devices = list(devices)
        dev = (C.c_int32 * len(self.devices))(*self.devices)
        self._h = C.c_void_p()
        rc = self._L.haf_create_multi(C.byref(self.cfg), dev, len(self.devices), shard_mode, C.byref(self._h))
        if rc != HAF_OK:
            raise HafError(rc, (self._L.haf_multi_last_error(None) or b"").decode())

    def close(self):
        if getattr(self, "_h", None):
            self._L.haf_destroy_multi(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != HAF_OK:
            raise HafError(rc, (self._L.haf_multi_last_error(self._h) or b"").decode())

    def info(self):
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._L.haf_multi_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(n_shards=a.value, n_ranks=b.value, rccl_version=c.value)

    def score_sharded(self, xyz, grasp_input):
        cl, keep = Engine._cloud(self, xyz)
        out = GraspOutput()
        self._check(self._L.haf_score_sharded(self._h, C.byref(cl), C.byref(grasp_input), C.byref(out)))
        return output_to_dict(out)

    def score_batch_sharded(self, clouds, inputs):
        n = len(clouds)
        keep = []
        arr = (Cloud * n)()
        for i, c in enumerate(clouds):
            arr[i], k = Engine._cloud(self, c)
            keep.append(k)
        gi = (GraspInput * n)(*inputs)
        out = (GraspOutput * n)()
        best = C.c_int32(-1)
        self._check(self._L.haf_score_batch_sharded(self._h, n, arr, gi, out, C.byref(best)))
        return [output_to_dict(o) for o in out], best.value

    def last_timing(self):
        """haf_multi_last_timing: host wall-clock of the last sharded call's parts."""
        n = self.info()["n_shards"]
        tot, bc, co, sh = C.c_float(), C.c_float(), C.c_float(), (C.c_float * n)()
        self._check(self._L.haf_multi_last_timing(self._h, C.byref(tot), C.byref(bc), C.byref(co), sh))
        return dict(total_ms=tot.value, bcast_us=bc.value, collective_us=co.value, shard_ms=list(sh))

    def last_records(self, rank):
        rec = np.zeros(self.cfg.n_rolls, dtype=ROLL_RECORD_DTYPE)
        self._check(self._L.haf_multi_last_records(self._h, rank, rec.ctypes.data))
        return rec

    def shard_stage_ms(self, shard):
        e = self._L.haf_multi_engine(self._h, shard)
        ms = (C.c_float * len(STAGES))()
        if self._L.haf_get_stage_ms(C.c_void_p(e), ms) != HAF_OK:
            return None
        return dict(zip(STAGES, list(ms)))
