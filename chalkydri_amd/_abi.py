"""ctypes mirror of include/chalkydri_hip.h and csrc/synth.h (POD structs only)."""
import ctypes as C

CK_OK = 0
CK_EINVAL, CK_ENOMEM, CK_EDEVICE, CK_ENODEVICE, CK_ECAPACITY, CK_EUNSUPPORTED = -1, -2, -3, -4, -5, -6
CK_MAX_FAMILIES = 4
CK_INVALID_LABEL = 0xFFFFFFFF


class ImageU8(C.Structure):
    _fields_ = [("buf", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32)]


class Family(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("nbits", C.c_uint32), ("ncodes", C.c_uint32),
                ("codes", C.POINTER(C.c_uint64)), ("bit_x", C.POINTER(C.c_uint32)),
                ("bit_y", C.POINTER(C.c_uint32)), ("width_at_border", C.c_int32),
                ("total_width", C.c_int32), ("reversed_border", C.c_int32), ("min_hamming", C.c_uint32),
                ("n_upstream", C.c_uint32)]


class Config(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("max_batch", C.c_int32), ("device", C.c_int32),
                ("quad_decimate", C.c_int32), ("min_white_black_diff", C.c_int32),
                ("min_component_px", C.c_int32), ("min_cluster_pixels", C.c_int32),
                ("max_nmaxima", C.c_int32), ("cos_critical_rad", C.c_double),
                ("max_line_fit_mse", C.c_double), ("refine_edges", C.c_int32),
                ("decode_sharpening", C.c_double), ("max_hamming", C.c_int32), ("n_families", C.c_int32),
                ("families", C.POINTER(Family) * CK_MAX_FAMILIES), ("max_points_per_frame", C.c_int32),
                ("max_clusters_per_frame", C.c_int32), ("max_quads_per_frame", C.c_int32)]


class Detection(C.Structure):
    _fields_ = [("id", C.c_int32), ("hamming", C.c_int32), ("family", C.c_int32),
                ("decision_margin", C.c_float), ("c", C.c_double * 2), ("p", (C.c_double * 2) * 4)]


class ClusterPoint(C.Structure):
    _fields_ = [("x", C.c_uint16), ("y", C.c_uint16), ("gx", C.c_int8), ("gy", C.c_int8), ("pad", C.c_uint16)]


class Cluster(C.Structure):
    _fields_ = [("rep0", C.c_uint32), ("rep1", C.c_uint32), ("start", C.c_uint32), ("count", C.c_uint32)]


class Quad(C.Structure):
    _fields_ = [("p", (C.c_double * 2) * 4), ("reversed_border", C.c_int32), ("rep0", C.c_uint32),
                ("rep1", C.c_uint32)]


class StageMs(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("h2d", "threshold", "segment", "clusters", "quads", "decode", "d2h", "total")]


class Iso3(C.Structure):
    _fields_ = [("t", C.c_double * 3), ("q", C.c_double * 4)]


class SqpnpParams(C.Structure):
    _fields_ = [("max_iter", C.c_int32), ("tol_sq", C.c_double)]


class SqpnpProblem(C.Structure):
    _fields_ = [("n_tags", C.c_int32), ("n_bearings", C.c_int32), ("tag_offset", C.c_int32),
                ("bearing_offset", C.c_int32), ("robot_to_cam", Iso3), ("gyro", C.c_double),
                ("sign_change_error", C.c_double)]


class SqpnpResult(C.Structure):
    _fields_ = [("valid", C.c_int32), ("pad", C.c_int32), ("rot", C.c_double * 9), ("pos", C.c_double * 3),
                ("std_devs", C.c_double * 3), ("yaw", C.c_double), ("energy", C.c_double)]


CK_RIG_MAX_CAMS = 8


class RigParams(C.Structure):
    _fields_ = [("sqpnp", SqpnpParams), ("sign_change_error", C.c_double), ("rig_id", C.c_uint8), ("pad", C.c_uint8 * 7)]


class RigResult(C.Structure):
    _fields_ = [("valid", C.c_int32), ("n_tags", C.c_int32), ("rot", C.c_double * 9), ("pos", C.c_double * 3),
                ("std_devs", C.c_double * 3), ("yaw", C.c_double), ("energy", C.c_double),
                ("cam_tags", C.c_int32 * CK_RIG_MAX_CAMS), ("cam_rms", C.c_double * CK_RIG_MAX_CAMS)]


CK_RIG_ROBUST_MAX_TAGS = 64
CK_RIG_ROBUST_CLEAN, CK_RIG_ROBUST_REJECTED, CK_RIG_ROBUST_MAXROUNDS, CK_RIG_ROBUST_NO_CONSENSUS = 0, 1, 2, 3


class RigRobustParams(C.Structure):
    _fields_ = [("rig", RigParams), ("gate_rad", C.c_double), ("mu_factor", C.c_double), ("max_rounds", C.c_int32),
                ("min_inlier_tags", C.c_int32)]


class RigRobustResult(C.Structure):
    _fields_ = [("fused", RigResult), ("status", C.c_int32), ("rounds", C.c_int32), ("n_rejected", C.c_int32), ("pad", C.c_int32),
                ("rejected", C.c_uint64 * CK_RIG_MAX_CAMS), ("worst_inlier_rad", C.c_double), ("best_rejected_rad", C.c_double)]


CK_RIG_REFINE_FREE, CK_RIG_REFINE_PLANAR = 0, 1
CK_RIG_REFINE_CONVERGED, CK_RIG_REFINE_MAXITERS, CK_RIG_REFINE_DEGENERATE, CK_RIG_REFINE_NO_START = 0, 1, 2, 3


class RigRefineParams(C.Structure):
    _fields_ = [("mode", C.c_int32), ("max_iters", C.c_int32), ("sigma_rad", C.c_double), ("gyro_sigma_rad", C.c_double), ("z", C.c_double)]


class RigRefined(C.Structure):
    _fields_ = [("status", C.c_int32), ("iters", C.c_int32), ("n_points", C.c_int32), ("dof", C.c_int32), ("rot", C.c_double * 9),
                ("pos", C.c_double * 3), ("cov", C.c_double * 36), ("std_devs", C.c_double * 3), ("cost0", C.c_double),
                ("cost", C.c_double), ("rms", C.c_double), ("chi2", C.c_double), ("moved_m", C.c_double), ("moved_rad", C.c_double),
                ("cam_rms", C.c_double * CK_RIG_MAX_CAMS)]


class OpenCV5(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")]


CK_CAMERA_OPENCV5, CK_CAMERA_EUCM, CK_CAMERA_UCM = 0, 1, 2


class Camera(C.Structure):
    """ck_camera_t: k = fx fy cx cy k1 k2 p1 p2 k3 (OPENCV5), fx fy cx cy alpha beta 0 0 0 (EUCM), fx fy cx cy alpha (UCM)."""
    _fields_ = [("model", C.c_int32), ("pad", C.c_int32), ("k", C.c_double * 9)]


# coloured game pieces: ck_blob_t.flags, then the per-frame status bits
CK_BLOB_MAX_CLASSES = 4
CK_BLOB_HAS_BEARING, CK_BLOB_HAS_GROUND, CK_BLOB_AT_BORDER = 1, 2, 4
CK_BLOB_TRUNCATED, CK_BLOB_OVERFLOW = 1, 2


class BlobClass(C.Structure):
    """ck_blob_class_t"""
    _fields_ = [(k, C.c_int32) for k in ("h_min", "h_max", "s_min", "s_max", "v_min", "v_max", "min_area", "max_area",
                                         "min_fill_permille", "min_aspect_permille", "max_aspect_permille", "pad")] + [("ground_z", C.c_double)]


class BlobParams(C.Structure):
    """ck_blob_params_t"""
    _fields_ = [(k, C.c_int32) for k in ("n_classes", "erode", "dilate", "max_targets", "max_components", "has_camera", "has_mount", "pad")] + [
        ("cls", BlobClass * CK_BLOB_MAX_CLASSES), ("cam", Camera), ("robot_to_cam", Iso3), ("max_range", C.c_double)]


class Blob(C.Structure):
    """ck_blob_t"""
    _fields_ = [(k, C.c_int32) for k in ("class_id", "flags", "area", "x0", "y0", "x1", "y1", "seed")] + [
        (k, C.c_int64) for k in ("sx", "sy", "sxx", "sxy", "syy")] + [
        ("cx", C.c_double), ("cy", C.c_double), ("major", C.c_double), ("minor", C.c_double), ("axis", C.c_double * 2),
        ("bearing", C.c_double * 3), ("ground", C.c_double * 2)]


assert C.sizeof(BlobClass) == 56 and C.sizeof(BlobParams) == 400 and C.sizeof(Blob) == 160

CK_SUBPIX_CONVERGED, CK_SUBPIX_MAXIT, CK_SUBPIX_FLAT, CK_SUBPIX_REJECTED = 0, 1, 2, 3


class SubpixParams(C.Structure):
    """ck_subpix_params_t"""
    _fields_ = [("half_win", C.c_int32), ("max_iters", C.c_int32), ("eps", C.c_double), ("det_min", C.c_double)]


class SubpixInfo(C.Structure):
    """ck_subpix_info_t"""
    _fields_ = [("status", C.c_int32), ("iters", C.c_int32), ("shift", C.c_double)]


class BoardDesc(C.Structure):
    """ck_board_t"""
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("first_id", C.c_int32), ("family", C.c_int32),
                ("tag_size", C.c_double), ("tag_spacing", C.c_double)]


class BoardParams(C.Structure):
    """ck_board_params_t"""
    _fields_ = [("seed_max_shift", C.c_double), ("max_shift", C.c_double), ("probe", C.c_double * 2), ("agree", C.c_double)]


assert C.sizeof(SubpixParams) == 24 and C.sizeof(SubpixInfo) == 16 and C.sizeof(BoardDesc) == 32 and C.sizeof(BoardParams) == 40


class TagPoseParams(C.Structure):
    _fields_ = [("cam", OpenCV5), ("tagsize", C.c_double * CK_MAX_FAMILIES), ("n_iters", C.c_int32), ("pad", C.c_int32)]


class TagPose(C.Structure):
    _fields_ = [("id", C.c_int32), ("family", C.c_int32), ("valid", C.c_int32), ("has_alt", C.c_int32),
                ("R", C.c_double * 9), ("t", C.c_double * 3), ("err", C.c_double), ("R_alt", C.c_double * 9),
                ("t_alt", C.c_double * 3), ("err_alt", C.c_double), ("H", C.c_double * 9)]


class JpegFrame(C.Structure):
    _fields_ = [("data", C.c_void_p), ("size", C.c_int64)]


class JpegInfo(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("width", "height", "n_components", "h_samp", "v_samp", "restart_interval", "has_dht",
                                         "pad")]


class RawFormat(C.Structure):
    _fields_ = [("fourcc", C.c_uint32), ("orientation", C.c_int32)]


class RawPlanes(C.Structure):   # ck_raw_planes_t
    _fields_ = [("sw", C.c_int32), ("sh", C.c_int32), ("cw", C.c_int32), ("ch", C.c_int32), ("offset", C.c_int64 * 3),
                ("row_stride", C.c_int32 * 3), ("step", C.c_int32 * 3), ("pad", C.c_int32 * 2), ("bytes", C.c_int64)]


class PreviewParams(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("width", "height", "quality", "restart_rows", "overlay", "pad")]


CK_EXPOSURE_GAMMAS, CK_EXPOSURE_BINS = 7, 192


class Rect(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("x0", "y0", "x1", "y1")]


class ExposureStats(C.Structure):
    _fields_ = [("luma", C.c_uint32 * 256), ("grad", (C.c_uint32 * CK_EXPOSURE_BINS) * CK_EXPOSURE_GAMMAS),
                ("n_luma", C.c_uint32), ("n_grad", C.c_uint32), ("pad", C.c_uint32 * 2)]


class ExposureParams(C.Structure):
    _fields_ = [("gamma", C.c_double * CK_EXPOSURE_GAMMAS), ("lambda_", C.c_double), ("delta", C.c_double), ("kp", C.c_double),
                ("e_min", C.c_double), ("e_max", C.c_double)]


CK_TRI_MAX_ROUNDS, CK_TRI_FLAT = 32, 1


class TriOtsuParams(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("max_iters", "min_delta", "keep_tbd", "channels")]


class TriOtsuInfo(C.Structure):
    _fields_ = [("n_rounds", C.c_int32), ("T", C.c_int32 * CK_TRI_MAX_ROUNDS), ("T_last", C.c_int32), ("lo_final", C.c_int32),
                ("hi_final", C.c_int32), ("n_black", C.c_uint32), ("n_white", C.c_uint32), ("n_other", C.c_uint32), ("flags", C.c_uint32)]


CK_CALIB_CONVERGED, CK_CALIB_STALLED, CK_CALIB_MAXIT, CK_CALIB_DEGENERATE = 0, 1, 2, 3
CK_CALIB_MAX_FRAMES, CK_CALIB_MAX_POINTS = 4096, 4096
CK_CALIB_FIX_DISTORTION, CK_CALIB_FIX_FOCAL = 0x1F0, 0x003


class CalibParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fixed_mask", C.c_uint32), ("max_iters", C.c_int32),
                ("min_points_per_frame", C.c_int32), ("min_frames", C.c_int32)]


class CalibProblem(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n_frames", "start_offset", "point_offset", "pose_offset")]


class CalibResult(C.Structure):
    _fields_ = [("cam", OpenCV5), ("status", C.c_int32), ("iters", C.c_int32), ("n_frames", C.c_int32), ("n_points", C.c_int32),
                ("rms", C.c_double), ("cost0", C.c_double), ("cost", C.c_double)]


CK_RIGCAL_MAX_STEPS = 4096


class RigcalParams(C.Structure):
    _fields_ = [("fixed_mask", C.c_uint64), ("max_iters", C.c_int32), ("min_steps", C.c_int32), ("min_cams_per_step", C.c_int32),
                ("pad", C.c_int32)]


class RigcalProblem(C.Structure):
    _fields_ = [("n_steps", C.c_int32), ("step_offset", C.c_int32)]


CK_FIELDCAL_MAX_TAGS, CK_FIELDCAL_MAX_STEPS, CK_FIELDCAL_FIX_ALL = 64, 4096, 63


class FieldcalParams(C.Structure):
    _fields_ = [("max_iters", C.c_int32), ("min_steps", C.c_int32), ("min_tags_per_step", C.c_int32), ("pad", C.c_int32)]


class FieldcalResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("iters", C.c_int32), ("n_steps", C.c_int32), ("n_steps_used", C.c_int32), ("n_points", C.c_int32),
                ("n_tags_solved", C.c_int32), ("rms", C.c_double), ("cost0", C.c_double), ("cost", C.c_double)]


class VisionMeasurement(C.Structure):
    _fields_ = [("pose_x", C.c_double), ("pose_y", C.c_double), ("pose_rot", C.c_double),
                ("std_x", C.c_double), ("std_y", C.c_double), ("std_rot", C.c_double), ("ts", C.c_uint64),
                ("camera_id", C.c_uint8), ("tag_count", C.c_uint8), ("reserved", C.c_uint8 * 6)]


class FieldTag(C.Structure):
    _fields_ = [("id", C.c_int32), ("pad", C.c_int32), ("pose", Iso3)]


class ProcessParams(C.Structure):
    _fields_ = [("cam", OpenCV5), ("robot_to_cam", Iso3), ("field", C.POINTER(FieldTag)),
                ("n_field", C.c_int32), ("camera_id", C.c_uint8), ("sign_change_error", C.c_double),
                ("sqpnp", SqpnpParams), ("allow_unverified_ids", C.c_int32)]


class SynthTag(C.Structure):
    _fields_ = [("family", C.c_int32), ("id", C.c_int32), ("H", C.c_double * 9),
                ("corners", (C.c_double * 2) * 4), ("center", C.c_double * 2)]


class SynthParams(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("width", "height", "n_tags", "min_side", "max_side", "max_tilt_t64",
                                         "noise_amp", "ramp_amp", "black", "white", "bg", "family_mode",
                                         "max_id")]


assert C.sizeof(VisionMeasurement) == 64  # crates/whacknet/src/lib.rs:92-95
assert C.sizeof(TagPoseParams) == 112 and C.sizeof(TagPose) == 296
assert C.sizeof(Camera) == 80
assert C.sizeof(JpegFrame) == 16 and C.sizeof(JpegInfo) == 32
assert C.sizeof(RawFormat) == 8 and C.sizeof(RawPlanes) == 80
assert C.sizeof(PreviewParams) == 24
assert C.sizeof(Rect) == 16 and C.sizeof(ExposureStats) == 6416 and C.sizeof(ExposureParams) == 96
assert C.sizeof(TriOtsuParams) == 16 and C.sizeof(TriOtsuInfo) == 160
assert C.sizeof(CalibParams) == 24 and C.sizeof(CalibProblem) == 16 and C.sizeof(CalibResult) == 112
assert C.sizeof(RigParams) == 32 and C.sizeof(RigResult) == 240
assert C.sizeof(RigRobustParams) == 56 and C.sizeof(RigRobustResult) == 336
assert C.sizeof(RigRefineParams) == 32 and C.sizeof(RigRefined) == 536


CK_CAMCAL_STARTS = 6


class CameraCalibResult(C.Structure):
    _fields_ = [("cam", Camera), ("status", C.c_int32), ("iters", C.c_int32), ("n_frames", C.c_int32), ("n_points", C.c_int32),
                ("rms", C.c_double), ("cost0", C.c_double), ("cost", C.c_double), ("start", C.c_int32), ("n_starts", C.c_int32)]


assert C.sizeof(CameraCalibResult) == 128


class RigcalResult(C.Structure):
    _fields_ = [("robot_to_cam", Iso3 * CK_RIG_MAX_CAMS), ("status", C.c_int32), ("iters", C.c_int32), ("n_steps", C.c_int32),
                ("n_steps_used", C.c_int32), ("n_points", C.c_int32), ("pad", C.c_int32), ("rms", C.c_double), ("cost0", C.c_double),
                ("cost", C.c_double), ("cam_points", C.c_int32 * CK_RIG_MAX_CAMS), ("cam_rms", C.c_double * CK_RIG_MAX_CAMS)]


assert C.sizeof(RigcalParams) == 24 and C.sizeof(RigcalProblem) == 8 and C.sizeof(RigcalResult) == 592
assert C.sizeof(FieldcalParams) == 16 and C.sizeof(FieldcalResult) == 48

# per-frame status bits (include/chalkydri_hip.h)
CK_FRAME_OK, CK_FRAME_POINTS_OVERFLOW, CK_FRAME_CLUSTERS_OVERFLOW, CK_FRAME_QUADS_OVERFLOW, CK_FRAME_DETS_OVERFLOW = 0, 1, 2, 4, 8
CK_FRAME_UNVERIFIED_ID = 16

# per-frame jpeg_status bits (ck_upload_jpeg / ck_jpeg_luma_batch)
CK_JPEG_OK, CK_JPEG_UNSUPPORTED, CK_JPEG_GEOMETRY, CK_JPEG_CORRUPT = 0, 1, 2, 4

# per-frame status bits of ck_preview_jpeg
CK_PREVIEW_OK, CK_PREVIEW_TRUNCATED = 0, 1

# ck_raw_format_t.orientation: the reference's VideoOrientation, by its serde names (chalkydri_core/src/config.rs:201-207)
CK_ORIENT_NONE, CK_ORIENT_CLOCKWISE, CK_ORIENT_ROTATE_180, CK_ORIENT_COUNTERCLOCKWISE = 0, 1, 2, 3
ORIENTATIONS = {"none": CK_ORIENT_NONE, "clockwise": CK_ORIENT_CLOCKWISE, "rotate-180": CK_ORIENT_ROTATE_180,
                "counterclockwise": CK_ORIENT_COUNTERCLOCKWISE}
# or-ed into ck_raw_format_t.orientation: the chroma planes behind the luma plane are part of every frame (PLANAR_FOURCCS only)
CK_RAW_PLANES = 0x100
PLANAR_FOURCCS = ("NV12", "NV21", "I420", "YV12")
# the fourccs of the raw entry points (ck_raw_layout answers CK_EUNSUPPORTED to every other one)
RAW_FOURCCS = ("GREY", "GRAY", "Y800", "NV12", "NV21", "I420", "YV12", "YUYV", "YUY2", "UYVY", "RGB3", "RGB ", "BGR3", "BGR ",
               "RGBA", "BGRA")
# the names the host layers accept for compressed frames (IngestRing, AprilTags): not raw formats, so not ck_raw_layout's business
JPEG_FOURCCS = ("MJPG", "JPEG")
