"""Host-side mirror of the reference's detector interface over the C ABI.

`AprilTagDetector` plays the role of `apriltag::Detector` as the reference uses it
(crates/apriltags/src/lib.rs:258-262 build, :301 detect, :306-314 id()/corners()), batched over frames.
`CatDetector` keeps the surface of crates/chalkydri-apriltags `Detector`
(src/lib.rs:158 new, :191 calc_otsu, :265 process_frame, :291 detect_corners, :319 thresh, :480 check_edges,
:501 connected_components).  Every call goes through libchalkydri_hip.so; nothing here computes on the CPU.
"""
import ctypes as C

import numpy as np

from . import _abi as A
from ._lib import check, default_config, lib

_P = C.POINTER


def _bind(L):
    if getattr(L, "_ck_bound", False):
        return L
    vp, i32, u32p = C.c_void_p, C.c_int32, _P(C.c_uint32)
    L.ck_last_error.restype = C.c_char_p
    L.ck_device_count.restype = C.c_int
    L.ck_create.argtypes = [_P(A.Config), _P(vp)]
    L.ck_destroy.argtypes = [vp]
    L.ck_destroy.restype = None
    L.ck_upload_frames.argtypes = [vp, _P(A.ImageU8), i32]
    L.ck_threshold_batch.argtypes = [vp, _P(A.ImageU8), i32, vp]
    L.ck_segment_batch.argtypes = [vp, _P(A.ImageU8), i32, vp, vp]
    L.ck_time_threshold_segment.argtypes = [vp, i32, i32, _P(C.c_float)]
    L.ck_detect_batch.argtypes = [vp, _P(A.ImageU8), i32, _P(A.Detection), i32, _P(i32), u32p]
    L.ck_detect_uploaded.argtypes = [vp, i32, _P(A.Detection), i32, _P(i32), u32p]
    L.ck_detect_batch_device.argtypes = [vp, vp, i32, i32, C.c_int64, _P(A.Detection), i32, _P(i32), u32p]
    L.ck_clusters_batch.argtypes = [vp, _P(A.ImageU8), i32, vp, i32, _P(i32), vp, i32, _P(i32)]
    L.ck_quads_batch.argtypes = [vp, _P(A.ImageU8), i32, _P(A.Quad), i32, _P(i32)]
    L.ck_decode_quads_batch.argtypes = [vp, _P(A.ImageU8), i32, _P(A.Quad), i32, _P(i32), _P(A.Detection), i32, _P(i32), u32p]
    L.ck_last_stage_ms.argtypes = [vp, _P(A.StageMs)]
    L.ck_selftest_fp64.argtypes = [vp, i32, vp, vp, i32, vp]
    L.ck_cat_calc_otsu.argtypes = [vp, vp, i32, i32, vp]
    L.ck_cat_thresh.argtypes = [vp, vp, i32, i32, vp]
    L.ck_cat_detect_corners.argtypes = [vp, vp, i32, i32, vp, i32, _P(i32)]
    L.ck_cat_check_edges.argtypes = [vp, vp, i32, i32, vp, i32, vp, i32, _P(i32)]
    L.ck_cat_connected_components.argtypes = [vp, vp, i32, i32, vp, vp]
    L.ck_cat_process_frame.argtypes = [vp, vp, C.c_size_t, i32, i32, vp, vp, i32, _P(i32), vp, i32, _P(i32)]
    L.ck_sqpnp_solve_batch.argtypes = [vp, _P(A.SqpnpParams), _P(A.SqpnpProblem), i32, _P(A.Iso3), i32, vp, i32,
                                       _P(A.SqpnpResult)]
    L.ck_sqpnp_create_solver_camera_transform.argtypes = [C.c_double] * 6 + [_P(A.Iso3)]
    L.ck_sqpnp_create_solver_camera_transform.restype = None
    L.ck_process_uploaded.argtypes = [vp, i32, _P(A.ProcessParams), vp, vp, _P(A.VisionMeasurement), _P(i32)]
    L.ck_process_batch_device.argtypes = [vp, vp, i32, i32, C.c_int64, _P(A.ProcessParams), vp, vp,
                                          _P(A.VisionMeasurement), _P(i32)]
    L.ck_unproject_opencv5.argtypes = [_P(A.OpenCV5), vp, i32, vp, vp]
    L.ck_ingest_create.argtypes = [vp, i32, _P(vp)]
    L.ck_ingest_destroy.argtypes = [vp]
    L.ck_ingest_destroy.restype = None
    L.ck_ingest_stride.argtypes = [vp]
    L.ck_ingest_stride.restype = i32
    L.ck_ingest_frame.argtypes = [vp, i32, i32]
    L.ck_ingest_frame.restype = vp
    L.ck_ingest_write.argtypes = [vp, i32, i32, _P(A.ImageU8), C.c_uint32]
    L.ck_ingest_submit.argtypes = [vp, i32, i32]
    L.ck_detect_ingested.argtypes = [vp, i32, i32, _P(A.Detection), i32, _P(i32), u32p]
    L.ck_process_ingested.argtypes = [vp, i32, i32, _P(A.ProcessParams), vp, vp, _P(A.VisionMeasurement), _P(i32)]
    L.ck_quad_sigma_kernel.argtypes = [C.c_float, vp, i32, _P(i32)]
    L.ck_set_quad_sigma.argtypes = [vp, C.c_float]
    L.ck_quad_image_batch.argtypes = [vp, _P(A.ImageU8), i32, vp]
    L.ck_estimate_tag_poses.argtypes = [vp, _P(A.TagPoseParams), vp, i32, vp]
    L.ck_last_tag_poses.argtypes = [vp, _P(A.TagPoseParams), vp, i32, vp]
    L.ck_jpeg_info.argtypes = [vp, C.c_int64, _P(A.JpegInfo)]
    L.ck_upload_jpeg.argtypes = [vp, _P(A.JpegFrame), i32, u32p]
    L.ck_jpeg_luma_batch.argtypes = [vp, _P(A.JpegFrame), i32, vp, u32p]
    L.ck_upload_jpeg_oriented.argtypes = [vp, _P(A.JpegFrame), i32, i32, u32p]
    L.ck_jpeg_luma_batch_oriented.argtypes = [vp, _P(A.JpegFrame), i32, i32, vp, u32p]
    L.ck_ingest_create_jpeg.argtypes = [vp, i32, i32, C.c_int64, _P(vp)]
    L.ck_ingest_write_jpeg.argtypes = [vp, i32, i32, vp, C.c_int64]
    L.ck_ingest_jpeg_status.argtypes = [vp, i32, i32, u32p]
    L.ck_upload_jpeg_color.argtypes = [vp, _P(A.JpegFrame), i32, i32, u32p]
    L.ck_ingest_create_jpeg_color.argtypes = [vp, i32, i32, C.c_int64, _P(vp)]
    rf = _P(A.RawFormat)
    L.ck_raw_layout.argtypes = [rf, i32, i32, _P(i32), _P(i32), _P(i32), _P(C.c_int64)]
    L.ck_upload_raw.argtypes = [vp, _P(A.ImageU8), i32, rf]
    L.ck_upload_raw_device.argtypes = [vp, vp, i32, i32, C.c_int64, rf]
    L.ck_raw_luma_batch.argtypes = [vp, _P(A.ImageU8), i32, rf, vp]
    L.ck_ingest_create_raw.argtypes = [vp, i32, rf, _P(vp)]
    L.ck_raw_plane_layout.argtypes = [rf, i32, i32, i32, _P(A.RawPlanes)]
    L.ck_raw_ycc_host.argtypes = [rf, _P(A.ImageU8), i32, i32, i32, vp]
    pv = _P(A.PreviewParams)
    L.ck_preview_params_default.argtypes = [pv]
    L.ck_preview_params_default.restype = None
    L.ck_preview_layout.argtypes = [pv, i32, i32, _P(i32), _P(i32), _P(C.c_int64)]
    L.ck_preview_jpeg.argtypes = [vp, pv, vp, i32, vp, C.c_int64, vp, vp]
    L.ck_preview_luma.argtypes = [vp, pv, vp, i32, vp]
    L.ck_preview_color_layout.argtypes = [pv, i32, i32, _P(i32), _P(i32), _P(C.c_int64)]
    L.ck_preview_jpeg_color.argtypes = [vp, pv, vp, i32, vp, C.c_int64, vp, vp]
    L.ck_preview_color.argtypes = [vp, pv, vp, i32, vp]
    L.ck_preview_jpeg_color_device.argtypes = [vp, pv, vp, i32, C.c_int64, rf, vp, i32, i32, vp, C.c_int64, vp, vp]
    L.ck_preview_color_device.argtypes = [vp, pv, vp, i32, C.c_int64, rf, vp, i32, i32, vp]
    L.ck_preview_jpeg_color_ingested.argtypes = [vp, i32, pv, vp, i32, vp, C.c_int64, vp, vp]
    L.ck_preview_color_ingested.argtypes = [vp, i32, pv, vp, i32, vp]
    ep, es = _P(A.ExposureParams), _P(A.ExposureStats)
    L.ck_exposure_params_default.argtypes = [ep]
    L.ck_exposure_params_default.restype = None
    L.ck_exposure_luts.argtypes = [ep, vp]
    L.ck_exposure_metric.argtypes = [ep, es, _P(C.c_double)]
    L.ck_exposure_recommend.argtypes = [ep, es, C.c_double, _P(C.c_double), _P(C.c_double)]
    L.ck_exposure_stats.argtypes = [vp, vp, i32, ep, vp, vp]
    L.ck_exposure_stats_ingested.argtypes = [vp, i32, vp, i32, ep, vp, vp]
    tp = _P(A.TriOtsuParams)
    L.ck_tri_otsu_params_default.argtypes = [tp]
    L.ck_tri_otsu_params_default.restype = None
    L.ck_tri_otsu_solve.argtypes = [tp, vp, _P(A.TriOtsuInfo), vp]
    L.ck_cat_tri_otsu_batch.argtypes = [vp, tp, vp, i32, i32, i32, vp, vp, vp]
    L.ck_cat_tri_otsu.argtypes = [vp, vp, i32, i32, vp]
    cp, cq, cr, cam = _P(A.CalibParams), _P(A.CalibProblem), _P(A.CalibResult), _P(A.OpenCV5)
    L.ck_calib_params_default.argtypes = [cp, i32, i32]
    L.ck_calib_params_default.restype = None
    L.ck_calib_check.argtypes = [cp, cq, i32, vp, vp, vp, i32, i32, i32]
    L.ck_calib_init.argtypes = [cp, cq, vp, vp, vp, i32, i32, i32, cam, vp, _P(i32)]
    L.ck_calib_jacobian.argtypes = [cam, vp, vp, vp, i32, C.c_uint32, vp, vp]
    L.ck_calib_refine_host.argtypes = [cp, cq, vp, vp, vp, i32, i32, i32, cam, vp, cr, vp]
    L.ck_calib_refine_batch.argtypes = [vp, cp, cq, i32, vp, vp, vp, i32, i32, i32, cam, vp, cr, vp]
    L.ck_calibrate_batch.argtypes = [vp, cp, cq, i32, vp, vp, vp, i32, i32, i32, cr, vp]
    rp, rr, sp = _P(A.RigParams), _P(A.RigResult), _P(A.SqpnpProblem)
    L.ck_rig_params_default.argtypes = [rp]
    L.ck_rig_params_default.restype = None
    L.ck_rig_solve_host.argtypes = [rp, i32, sp, i32, _P(A.Iso3), i32, vp, i32, vp, rr]
    L.ck_rig_solve_batch.argtypes = [vp, rp, i32, sp, i32, _P(A.Iso3), i32, vp, i32, vp, rr]
    L.ck_rig_process_last.argtypes = [_P(vp), i32, i32, rp, vp, vp, rr, _P(A.VisionMeasurement), _P(i32)]
    L.ck_rig_time_last.argtypes = [_P(vp), i32, i32, rp, vp, vp, i32, vp, vp]
    bp, br = _P(A.RigRobustParams), _P(A.RigRobustResult)
    L.ck_rig_robust_params_default.argtypes = [bp]
    L.ck_rig_robust_params_default.restype = None
    L.ck_rig_solve_robust_host.argtypes = [bp, i32, sp, i32, _P(A.Iso3), i32, vp, i32, vp, br]
    L.ck_rig_solve_robust_batch.argtypes = [vp, bp, i32, sp, i32, _P(A.Iso3), i32, vp, i32, vp, br]
    L.ck_rig_process_last_robust.argtypes = [_P(vp), i32, i32, bp, vp, vp, br, _P(A.VisionMeasurement), _P(i32)]
    fp, fr = _P(A.RigRefineParams), _P(A.RigRefined)
    L.ck_rig_refine_params_default.argtypes = [fp]
    L.ck_rig_refine_params_default.restype = None
    L.ck_rig_refine_host.argtypes = [fp, i32, sp, i32, _P(A.Iso3), i32, vp, i32, vp, vp, vp, fr]
    L.ck_rig_refine_batch.argtypes = [vp, fp, i32, sp, i32, _P(A.Iso3), i32, vp, i32, vp, vp, vp, fr]
    L.ck_rig_process_last_refined.argtypes = [_P(vp), i32, i32, bp, i32, fp, vp, vp, vp, fr, _P(A.VisionMeasurement), _P(i32)]
    L.ck_rig_refine_time.argtypes = [vp, fp, i32, sp, i32, _P(A.Iso3), i32, vp, i32, vp, i32, vp, vp]
    mp, mq, mr, iso = _P(A.RigcalParams), _P(A.RigcalProblem), _P(A.RigcalResult), _P(A.Iso3)
    L.ck_rigcal_params_default.argtypes = [mp]
    L.ck_rigcal_params_default.restype = None
    capture = [i32, sp, i32, iso, i32, vp, i32]
    L.ck_rigcal_check.argtypes = [mp] + capture + [mq, i32, vp, i32, iso]
    L.ck_rigcal_jacobian.argtypes = [iso, vp, vp, vp, i32, C.c_uint32, vp, vp]
    L.ck_rigcal_refine_host.argtypes = [mp] + capture + [mq, vp, i32, iso, vp, mr, vp]
    L.ck_rigcal_refine_batch.argtypes = [vp, mp] + capture + [mq, i32, vp, i32, iso, vp, mr, vp]
    L.ck_rig_calibrate_batch.argtypes = [vp, mp] + capture + [vp, mq, i32, vp, i32, iso, mr, vp]
    L.ck_last_pose_inputs.argtypes = [vp, i32, sp, iso, i32, vp, i32, _P(i32), _P(i32)]
    fp, fr = _P(A.FieldcalParams), _P(A.FieldcalResult)
    L.ck_fieldcal_params_default.argtypes = [fp]
    L.ck_fieldcal_params_default.restype = None
    fcap, flay = [i32, sp, i32, vp, i32, vp, i32], [iso, iso, i32, vp]               # ..., mounts, layout0, n_layout, fixed6
    fout = [fr, iso, vp, vp, vp]                                                     # results, layout_out, tag_sightings, tag_rms, poses_out
    L.ck_fieldcal_check.argtypes = [fp] + fcap + [mq, i32, vp, i32] + flay
    L.ck_fieldcal_jacobian.argtypes = [iso, vp, iso, vp, i32, C.c_uint32, vp, vp]
    L.ck_fieldcal_refine_host.argtypes = [fp] + fcap + [mq, vp, i32] + flay + [vp] + fout
    L.ck_fieldcal_refine_batch.argtypes = [vp, fp] + fcap + [mq, i32, vp, i32] + flay + [vp] + fout
    L.ck_field_calibrate_batch.argtypes = [vp, fp] + fcap + [vp, mq, i32, vp, i32] + flay + fout
    cm = _P(A.Camera)
    L.ck_camera_check.argtypes = [cm]
    L.ck_camera_unproject_host.argtypes = [cm, vp, i32, vp, vp]
    L.ck_camera_normalize_host.argtypes = [cm, vp, i32, vp, vp]
    L.ck_camera_project_host.argtypes = [cm, vp, i32, vp, vp]
    L.ck_camera_unproject.argtypes = [cm, vp, i32, vp, vp]
    L.ck_set_camera.argtypes = [vp, cm]
    ccr = _P(A.CameraCalibResult)
    L.ck_camera_calib_jacobian.argtypes = [i32, cm, vp, vp, vp, i32, C.c_uint32, vp, vp]
    L.ck_camera_calib_init.argtypes = [i32, cp, cq, vp, vp, vp, i32, i32, i32, i32, cm, vp, _P(i32)]
    L.ck_camera_calib_refine_host.argtypes = [i32, cp, cq, vp, vp, vp, i32, i32, i32, cm, vp, ccr, vp]
    L.ck_camera_calib_refine_batch.argtypes = [vp, i32, cp, cq, i32, vp, vp, vp, i32, i32, i32, cm, vp, ccr, vp]
    L.ck_camera_calibrate_batch.argtypes = [vp, i32, cp, cq, i32, vp, vp, vp, i32, i32, i32, ccr, vp]
    sx, sb, sq = _P(A.SubpixParams), _P(A.BoardDesc), _P(A.BoardParams)
    L.ck_subpix_params_default.argtypes = [sx]
    L.ck_subpix_params_default.restype = None
    L.ck_subpix_weights.argtypes = [sx, vp]
    L.ck_corner_subpix.argtypes = [vp, sx, vp, vp, i32, vp, vp]
    L.ck_corner_subpix_host.argtypes = [sx, _P(A.ImageU8), i32, vp, vp, i32, vp, vp]
    L.ck_set_corner_subpix.argtypes = [vp, sx]
    L.ck_board_params_default.argtypes = [sq]
    L.ck_board_params_default.restype = None
    L.ck_board_corners_last.argtypes = [vp, sb, sx, sq, vp, vp, vp]
    L.ck_board_corners_host.argtypes = [sb, sx, sq, _P(A.ImageU8), i32, vp, i32, vp, vp, vp, vp]
    bb, bo = _P(A.BlobParams), _P(A.Blob)
    L.ck_blob_params_default.argtypes = [bb]
    L.ck_blob_params_default.restype = None
    L.ck_blob_check.argtypes = [bb]
    L.ck_blob_rgb_hsv.argtypes = [vp, C.c_int64, vp]
    L.ck_blob_mask_host.argtypes = [bb, vp, i32, i32, i32, i32, i32, vp]
    L.ck_blobs_host.argtypes = [bb, vp, i32, i32, i32, vp, i32, vp, vp]
    L.ck_detect_blobs.argtypes = [vp, bb, vp, i32, vp, i32, vp, vp]
    L.ck_detect_blobs_device.argtypes = [vp, bb, vp, i32, C.c_int64, rf, vp, i32, i32, vp, i32, vp, vp]
    L.ck_detect_blobs_ingested.argtypes = [vp, i32, bb, vp, i32, vp, i32, vp, vp]
    L.ck_blob_rgb.argtypes = [vp, vp, i32, vp]
    L.ck_blob_rgb_device.argtypes = [vp, vp, i32, C.c_int64, rf, vp, i32, i32, vp]
    L.ck_blob_mask.argtypes = [vp, bb, vp, i32, i32, i32, vp]
    L.ck_blob_mask_device.argtypes = [vp, bb, vp, i32, C.c_int64, rf, vp, i32, i32, i32, i32, vp]
    L.ck_blob_time.argtypes = [vp, bb, vp, i32, C.c_int64, rf, i32, i32, i32, _P(C.c_float)]
    L._ck_bound = True
    return L


def device_count():
    return _bind(lib()).ck_device_count()


def _images(frames):
    """frames: uint8 array [n][h][stride>=w] (C-contiguous rows) -> (ImageU8 array, keepalive)."""
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    if frames.ndim == 2:
        frames = frames[None]
    n, h, w = frames.shape
    arr = (A.ImageU8 * n)()
    for i in range(n):
        arr[i].buf = frames[i].ctypes.data
        arr[i].width, arr[i].height, arr[i].stride = w, h, frames.strides[1]
    return arr, frames


class Detection:
    """Mirrors the accessors the reference uses on apriltag::Detection (crates/apriltags/src/lib.rs:306-314)."""
    __slots__ = ("_id", "_hamming", "_family", "_margin", "_c", "_p")

    def __init__(self, d):
        self._id, self._hamming, self._family, self._margin = d.id, d.hamming, d.family, d.decision_margin
        self._c = np.array([d.c[0], d.c[1]])
        self._p = np.array([[d.p[k][0], d.p[k][1]] for k in range(4)])

    def id(self):
        return self._id

    def hamming(self):
        return self._hamming

    def family(self):
        return self._family

    def decision_margin(self):
        return self._margin

    def center(self):
        return self._c

    def corners(self):
        return self._p

    def __repr__(self):
        return f"Detection(id={self._id}, hamming={self._hamming}, margin={self._margin:.1f})"


def tag_pose_params(fx, fy, cx, cy, tagsize=0.1651, distortion=None, n_iters=50):
    """ck_tag_pose_params_t for estimate_tag_poses / last_tag_poses.  tagsize: edge of the black square in metres, one value
    for every family or a sequence by family index; distortion: OpenCV-5 (k1, k2, p1, p2, k3), None = pinhole."""
    pp = A.TagPoseParams()
    lib().ck_tag_pose_params_default(C.byref(pp))
    k1, k2, p1, p2, k3 = (0.0,) * 5 if distortion is None else (float(v) for v in distortion)
    pp.cam = A.OpenCV5(float(fx), float(fy), float(cx), float(cy), k1, k2, p1, p2, k3)
    sizes = [tagsize] * A.CK_MAX_FAMILIES if np.ndim(tagsize) == 0 else list(tagsize)
    for i, v in enumerate(sizes[:A.CK_MAX_FAMILIES]):
        pp.tagsize[i] = float(v)
    pp.n_iters = int(n_iters)
    return pp


class TagPose:
    """One ck_tag_pose_t: the pose of a tag relative to the camera (tag -> camera; camera x right, y down, z forward), as
    AprilTag-3's estimate_tag_pose returns it, with the other local minimum kept beside it."""
    __slots__ = ("id", "family", "valid", "has_alt", "_R", "_t", "_err", "_R_alt", "_t_alt", "_err_alt", "_H")

    def __init__(self, r):
        self.id, self.family, self.valid, self.has_alt = r.id, r.family, bool(r.valid), bool(r.has_alt)
        self._R = np.array(r.R[:]).reshape(3, 3)
        self._t = np.array(r.t[:])
        self._err = r.err
        self._R_alt = np.array(r.R_alt[:]).reshape(3, 3)
        self._t_alt = np.array(r.t_alt[:])
        self._err_alt = r.err_alt
        self._H = np.array(r.H[:]).reshape(3, 3)

    def rotation(self):
        return self._R

    def translation(self):
        return self._t

    def error(self):
        return self._err

    def homography(self):
        return self._H

    def alternative(self):
        """(R, t, err) of the other local minimum, or None."""
        return (self._R_alt, self._t_alt, self._err_alt) if self.has_alt else None

    def ambiguity(self):
        """err / err_alt: near 1 when the two minima explain the corners equally well; 0 without an alternative."""
        return self._err / self._err_alt if self.has_alt and self._err_alt > 0 else 0.0

    def __repr__(self):
        return f"TagPose(id={self.id}, valid={self.valid}, t={np.round(self._t, 4).tolist()}, err={self._err:.3g})"


def _jpeg_frames(frames):
    """bytes-like JPEG frames -> (ck_jpeg_frame_t array, keepalive)."""
    keep = [np.frombuffer(bytes(f), np.uint8) for f in frames]
    arr = (A.JpegFrame * max(len(keep), 1))()
    for i, b in enumerate(keep):
        arr[i].data, arr[i].size = b.ctypes.data, b.size
    return arr, keep


def jpeg_info(data):
    """ck_jpeg_info: the header of one JPEG as a dict (width, height, n_components, h_samp, v_samp, restart_interval, has_dht).
    Raises ChalkydriError with CK_EUNSUPPORTED for a valid JPEG outside the supported subset, CK_EINVAL for anything else."""
    b = np.frombuffer(bytes(data), np.uint8)
    info = A.JpegInfo()
    check(_bind(lib()).ck_jpeg_info(b.ctypes.data if b.size else None, b.size, C.byref(info)), "ck_jpeg_info")
    return {k: getattr(info, k) for k, _ in A.JpegInfo._fields_ if k != "pad"}


def orientation_code(orientation):
    """'none' / 'clockwise' / 'rotate-180' / 'counterclockwise' (the reference's serde names) or 0..3 -> CK_ORIENT_*."""
    if isinstance(orientation, str):
        if orientation not in A.ORIENTATIONS:
            raise ValueError(f"orientation must be one of {sorted(A.ORIENTATIONS)}")
        return A.ORIENTATIONS[orientation]
    return int(orientation)


def raw_format(code, orientation="none", planes=False):
    """ck_raw_format_t from a fourcc string (or its u32) and an orientation.  planes: CK_RAW_PLANES, the chroma planes behind the
    luma plane of 'NV12' / 'NV21' / 'I420' / 'YV12' are part of every frame."""
    return A.RawFormat(fourcc(code) if isinstance(code, str) else int(code),
                       orientation_code(orientation) | (A.CK_RAW_PLANES if planes else 0))


def raw_layout(code, width, height, orientation="none", planes=False):
    """ck_raw_layout: (sw, sh, min_stride, min_bytes) of the source of an oriented width x height frame.  No device needed."""
    sw, sh, ms, mb = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    fmt = raw_format(code, orientation, planes)
    check(_bind(lib()).ck_raw_layout(C.byref(fmt), width, height, C.byref(sw), C.byref(sh), C.byref(ms), C.byref(mb)), "ck_raw_layout")
    return sw.value, sh.value, ms.value, mb.value


def raw_plane_layout(code, width, height, stride, orientation="none"):
    """ck_raw_plane_layout: where the samples of a planar frame (CK_RAW_PLANES) of row stride `stride` lie, as a dict of
    sw, sh, cw, ch, offset[3], row_stride[3], step[3] (Y, Cb, Cr) and bytes.  No device needed."""
    fmt, out = raw_format(code, orientation, True), A.RawPlanes()
    check(_bind(lib()).ck_raw_plane_layout(C.byref(fmt), width, height, int(stride), C.byref(out)), "ck_raw_plane_layout")
    return {"sw": out.sw, "sh": out.sh, "cw": out.cw, "ch": out.ch, "offset": tuple(out.offset), "row_stride": tuple(out.row_stride),
            "step": tuple(out.step), "bytes": out.bytes}


def _raw_rows(fmt, width, height):
    """(sw, sh, rows) of a format's source: rows = the rows of the row stride a frame holds, sh + ch with CK_RAW_PLANES."""
    sw, sh, _, _ = raw_layout(fmt.fourcc, width, height, fmt.orientation)
    return sw, sh, sh + ((sh + 1) // 2 if fmt.orientation & A.CK_RAW_PLANES else 0)


def raw_ycc_host(frames, code, width, height, orientation="none", planes=False):
    """ck_raw_ycc_host: [n][height][width][3] uint8, the (Y, Cb, Cr) triples of raw frames turned by `orientation`, computed on the
    host by the library's one-thread twin of preview_color at the identity size.  No device needed."""
    fmt = raw_format(code, orientation, planes)
    sw, sh, rows = _raw_rows(fmt, width, height)
    arr, keep = _raw_images(frames, sw, sh)
    for f in keep:
        if f.shape[0] < rows:
            raise ValueError(f"a raw frame needs {rows} rows")
    out = np.empty((len(keep), height, width, 3), np.uint8)
    buf = out if out.size else np.empty(1, np.uint8)
    check(_bind(lib()).ck_raw_ycc_host(C.byref(fmt), arr, len(keep), width, height, buf.ctypes.data), "ck_raw_ycc_host")
    return out


def _raw_images(frames, sw, sh):
    """Raw frames — one uint8 array [n][sh][stride] or a sequence of [sh][stride] arrays (stride in bytes, rows contiguous) ->
    (ImageU8 array declaring sw x sh, keepalive)."""
    if isinstance(frames, np.ndarray) and frames.ndim == 2:
        frames = [frames]
    keep = []
    for f in frames:
        f = np.asarray(f)
        if f.dtype != np.uint8 or f.ndim != 2 or f.strides[1] != 1:
            f = np.ascontiguousarray(f, dtype=np.uint8)
            if f.ndim != 2:
                raise ValueError("a raw frame is a 2-D uint8 array [rows][bytes]")
        keep.append(f)
    arr = (A.ImageU8 * max(len(keep), 1))()
    for i, f in enumerate(keep):
        arr[i].buf, arr[i].width, arr[i].height, arr[i].stride = f.ctypes.data, sw, sh, f.strides[0]
    return arr, keep


def _raw_detections(dets):
    """Detection objects, ck_detection_t arrays or an [n] ctypes array -> ctypes array (+ count)."""
    if isinstance(dets, C.Array):
        return dets, len(dets)
    arr = (A.Detection * max(len(dets), 1))()
    for i, d in enumerate(dets):
        if isinstance(d, A.Detection):
            arr[i] = d
            continue
        r = arr[i]
        r.id, r.hamming, r.family, r.decision_margin = d.id(), d.hamming(), d.family(), d.decision_margin()
        r.c[0], r.c[1] = d.center()
        for k in range(4):
            r.p[k][0], r.p[k][1] = d.corners()[k]
    return arr, len(dets)


def preview_params(width=640, height=480, quality=50, restart_rows=0, overlay=False):
    """ck_preview_params_t; the defaults are the reference's driver-station stream (640 x 480, quality 50)."""
    pp = A.PreviewParams()
    _bind(lib()).ck_preview_params_default(C.byref(pp))
    pp.width, pp.height, pp.quality, pp.restart_rows, pp.overlay = int(width), int(height), int(quality), int(restart_rows), int(bool(overlay))
    return pp


def preview_layout(params, width, height):
    """ck_preview_layout: (pw, ph, max_bytes) of a preview of a width x height handle.  No device needed."""
    pw, ph, mb = C.c_int32(), C.c_int32(), C.c_int64()
    check(_bind(lib()).ck_preview_layout(C.byref(params), width, height, C.byref(pw), C.byref(ph), C.byref(mb)), "ck_preview_layout")
    return pw.value, ph.value, mb.value


def preview_color_layout(params, width, height):
    """ck_preview_color_layout: (pw, ph, max_bytes) of a colour preview of a width x height handle.  No device needed."""
    pw, ph, mb = C.c_int32(), C.c_int32(), C.c_int64()
    check(_bind(lib()).ck_preview_color_layout(C.byref(params), width, height, C.byref(pw), C.byref(ph), C.byref(mb)), "ck_preview_color_layout")
    return pw.value, ph.value, mb.value


def mjpeg_part(jpeg):
    """One part of the reference's multipart stream (crates/chalkydri/src/cameras/mjpeg.rs:122-128): the boundary, the length and
    the content type in front of a complete JPEG."""
    jpeg = bytes(jpeg)
    return b"--frame\r\nContent-Length: " + str(len(jpeg)).encode("ascii") + b"\r\nContent-Type: image/jpeg\r\n\r\n" + jpeg


class MjpegStream:
    """The reference's rate limit in front of the framing (videorate max-rate 20, drop-only: mjpeg.rs:30-34): part(jpeg, now)
    gives the framed bytes, or None for a frame that comes sooner than 1 / max_rate seconds after the last one sent."""

    def __init__(self, max_rate=20.0):
        self.period, self._last = 1.0 / float(max_rate), None

    def part(self, jpeg, now):
        if self._last is not None and now - self._last < self.period:
            return None
        self._last = now
        return mjpeg_part(jpeg)


class AprilTagDetector:
    """One handle = one GPU + its stream; not thread-safe (mirrors `&mut self`)."""

    def __init__(self, width, height, max_batch=1, families=("tag36h11",), bits_corrected=3, device=0, quad_sigma=0.0,
                 corner_subpix=None, **cfg):
        self._L = _bind(lib())
        self.cfg = default_config(width, height, max_batch, families, max_hamming=bits_corrected, device=device,
                                  **cfg)
        self.width, self.height, self.max_batch = width, height, max_batch
        self.qw, self.qh = width // self.cfg.quad_decimate, height // self.cfg.quad_decimate
        h = C.c_void_p()
        check(self._L.ck_create(C.byref(self.cfg), C.byref(h)), "ck_create")
        self._h = h
        self.quad_sigma = 0.0
        self.camera = None
        self.corner_subpix_params = None
        if quad_sigma:
            self.set_quad_sigma(quad_sigma)
        if corner_subpix:
            self.set_corner_subpix(**({} if corner_subpix is True else dict(corner_subpix)))

    def set_quad_sigma(self, sigma):
        """AprilTag-3's quad_sigma: > 0 blurs, < 0 sharpens the image the quad stages run on; |sigma| < 0.5 is off.  May be
        changed between calls."""
        check(self._L.ck_set_quad_sigma(self._h, float(sigma)), "ck_set_quad_sigma")
        self.quad_sigma = float(sigma)

    def set_camera(self, cam):
        """The camera model the pose paths unproject with (an A.Camera: chalkydri_amd.camera.camera_from_calib): while one is set,
        process / tag-pose calls ignore their params' OpenCVModel5.  None restores it.  A refused camera leaves the setting as it was."""
        check(self._L.ck_set_camera(self._h, None if cam is None else C.byref(cam)), "ck_set_camera")
        self.camera = cam

    def set_corner_subpix(self, half_win=None, max_iters=None, eps=None, det_min=None, on=True):
        """Sub-pixel refinement of every final detection's corners inside the detect / process calls (ck_set_corner_subpix): a
        gradient-orthogonality iteration over a window of (2 half_win + 1)^2 taps on the full-resolution frame, which rewrites
        the corners and the centre, so everything downstream inherits them.  Off by default; on=False turns it off again.  A
        window wider than the blur of the lens helps, a narrower one can hurt: half_win is the caller's choice (default 5)."""
        from .subpix import subpix_params
        pp = subpix_params(half_win, max_iters, eps, det_min) if on else None
        check(self._L.ck_set_corner_subpix(self._h, None if pp is None else C.byref(pp)), "ck_set_corner_subpix")
        self.corner_subpix_params = pp

    def corner_subpix(self, frame, xy, params=None, return_info=False):
        """Refines points xy [n][2] (pixels, the detections' convention) of the staged frames on the device (ck_corner_subpix);
        frame: the staged frame of every point (an int for all of them, or [n]).  Returns [n][2], with return_info also the
        status, iteration count and shift of every point as a structured array."""
        from .subpix import INFO_DTYPE, subpix_params
        pp = params or self.corner_subpix_params or subpix_params()
        xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
        n = len(xy)
        fr = np.ascontiguousarray(np.broadcast_to(np.asarray(frame, np.int32), (n,)))
        out, info = np.empty((n, 2)), np.zeros(n, INFO_DTYPE)
        check(self._L.ck_corner_subpix(self._h, C.byref(pp), fr.ctypes.data, xy.ctypes.data, n, out.ctypes.data, info.ctypes.data),
              "ck_corner_subpix")
        return (out, info) if return_info else out

    def board_corners(self, board, params=None, board_params=None, family=0):
        """Recovers a tag board (a calibration.Board) in every frame of the last detect / process call from the tags that decoded
        (ck_board_corners_last): (uv [n][rows * cols][4][2], state [n][rows * cols]: 0 absent, 1 seed, 2 recovered)."""
        from .subpix import board_desc, board_params as default_bp, subpix_params
        pp = params or self.corner_subpix_params or subpix_params()
        bd, bp = board_desc(board, family), board_params or default_bp()
        nt, nb = board.rows * board.cols, self.max_batch
        uv, state = np.zeros((nb, nt, 4, 2)), np.zeros((nb, nt), np.uint8)
        counts = np.full(nb, -1, np.int32)  # the call writes one count per frame of the last call: the rest stay -1
        check(self._L.ck_board_corners_last(self._h, C.byref(bd), C.byref(pp), C.byref(bp), uv.ctypes.data, state.ctypes.data,
                                            counts.ctypes.data), "ck_board_corners_last")
        n = int((counts >= 0).sum())
        return uv[:n], state[:n]

    def close(self):
        if getattr(self, "_h", None):
            self._L.ck_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- staging ----------------------------------------------------------------------------------------
    def upload(self, frames):
        arr, keep = _images(frames)
        check(self._L.ck_upload_frames(self._h, arr, len(arr)), "ck_upload_frames")
        return len(arr)

    def upload_jpeg(self, frames, orientation="none", return_status=False, color=False):
        """Decodes the luma of baseline JPEG frames (bytes each) on the device into the staged frames, as `upload` stages raw
        luma: detect_batch(None, n) / the process and pose calls follow.  A frame that is unsupported, of another size or
        corrupt is staged as zeros; its CK_JPEG_* bits are in the status list (return_status=True).  With an `orientation` the
        frames are staged turned, the detector's width x height being the ORIENTED frame (the streams are height x width for
        the quarter turns), as upload_raw does it.  color=True (ck_upload_jpeg_color) stages the same luma and keeps the frames'
        chroma planes on the device: preview_jpeg_color / preview_color then work on them until frames are staged another way."""
        arr, keep = _jpeg_frames(frames)
        status = (C.c_uint32 * max(len(keep), 1))()
        o = orientation_code(orientation)
        if color:
            check(self._L.ck_upload_jpeg_color(self._h, arr, len(keep), o, status), "ck_upload_jpeg_color")
        else:
            check(self._L.ck_upload_jpeg_oriented(self._h, arr, len(keep), o, status), "ck_upload_jpeg_oriented")
        return (len(keep), list(status)[:len(keep)]) if return_status else len(keep)

    def decode_jpeg(self, frames, return_status=False, orientation="none"):
        """[n][height][width] uint8: the luma the device decodes from the JPEG frames (bit-identical to libjpeg's islow IDCT),
        turned by `orientation`."""
        arr, keep = _jpeg_frames(frames)
        out = np.empty((len(keep), self.height, self.width), np.uint8)
        status = (C.c_uint32 * max(len(keep), 1))()
        o = orientation_code(orientation)
        check(self._L.ck_jpeg_luma_batch_oriented(self._h, arr, len(keep), o, out.ctypes.data, status), "ck_jpeg_luma_batch_oriented")
        return (out, list(status)[:len(keep)]) if return_status else out

    def upload_raw(self, frames, code, orientation="none", planes=False):
        """Raw camera frames ([rows][bytes] each: 'YUYV', 'RGB3', 'BGRA', ... as ck_raw_layout lists them) are converted to luma
        and turned by `orientation` on the device into the staged frames; the detector's width x height is the ORIENTED frame.
        detect_batch(None, n=...) / the process and pose calls follow, as after `upload`.  planes=True ('NV12', 'NV21', 'I420',
        'YV12'): every frame carries its chroma planes ([sh + ch][bytes]), which the colour preview and the blob calls then read."""
        fmt = raw_format(code, orientation, planes)
        sw, sh, rows = _raw_rows(fmt, self.width, self.height)
        arr, keep = _raw_images(frames, sw, sh)
        for f in keep:
            if f.shape[0] < rows:
                raise ValueError(f"a raw frame needs {rows} rows")
        check(self._L.ck_upload_raw(self._h, arr, len(keep), C.byref(fmt)), "ck_upload_raw")
        return len(keep)

    def upload_raw_device(self, ptr, n, stride, frame_pitch, code, orientation="none", planes=False):
        """The same from device-resident frames (a torch tensor's data_ptr(), another decoder's output): no host copy.  The
        work that produced them must have completed (torch.cuda.synchronize / the producing stream)."""
        fmt = raw_format(code, orientation, planes)
        check(self._L.ck_upload_raw_device(self._h, C.c_void_p(ptr), n, stride, frame_pitch, C.byref(fmt)), "ck_upload_raw_device")
        return n

    def raw_luma(self, frames, code, orientation="none", planes=False):
        """[n][height][width] uint8: the oriented luma the device makes of the raw frames (and leaves staged)."""
        fmt = raw_format(code, orientation, planes)
        sw, sh, rows = _raw_rows(fmt, self.width, self.height)
        arr, keep = _raw_images(frames, sw, sh)
        for f in keep:
            if f.shape[0] < rows:
                raise ValueError(f"a raw frame needs {rows} rows")
        out = np.empty((len(keep), self.height, self.width), np.uint8)
        check(self._L.ck_raw_luma_batch(self._h, arr, len(keep), C.byref(fmt), out.ctypes.data), "ck_raw_luma_batch")
        return out

    # -- stages -------------------------------------------------------------------------------------------
    def threshold(self, frames=None, n=None):
        arr, keep, n = self._in(frames, n)
        out = np.empty((n, self.qh, self.qw), np.uint8)
        check(self._L.ck_threshold_batch(self._h, arr, n, out.ctypes.data), "ck_threshold_batch")
        return out

    def segment(self, frames=None, n=None, sizes=True):
        arr, keep, n = self._in(frames, n)
        labels = np.empty((n, self.qh, self.qw), np.uint32)
        sz = np.empty((n, self.qh, self.qw), np.uint32) if sizes else None
        check(self._L.ck_segment_batch(self._h, arr, n, labels.ctypes.data, sz.ctypes.data if sizes else None),
              "ck_segment_batch")
        return labels, sz

    def quad_image(self, frames=None, n=None):
        """[n][qh][qw]: the image the quad stages run on (decimated and / or filtered frame)."""
        arr, keep, n = self._in(frames, n)
        out = np.empty((n, self.qh, self.qw), np.uint8)
        check(self._L.ck_quad_image_batch(self._h, arr, n, out.ctypes.data), "ck_quad_image_batch")
        return out

    def time_threshold_segment(self, n, iters=10):
        ms = C.c_float(0)
        check(self._L.ck_time_threshold_segment(self._h, n, iters, C.byref(ms)), "ck_time_threshold_segment")
        return ms.value

    def clusters(self, frames=None, n=None, cluster_cap=None, point_cap=None):
        arr, keep, n = self._in(frames, n)
        ccap = cluster_cap or (self.qw * self.qh // 8 + 1024)
        pcap = point_cap or (2 * self.qw * self.qh)
        cl = np.zeros((n, ccap, 4), np.uint32)
        pts = np.zeros((n, pcap), np.dtype([("x", "<u2"), ("y", "<u2"), ("gx", "i1"), ("gy", "i1"), ("pad", "<u2")]))
        nc = (C.c_int32 * n)()
        npt = (C.c_int32 * n)()
        check(self._L.ck_clusters_batch(self._h, arr, n, cl.ctypes.data, ccap, nc, pts.ctypes.data, pcap, npt),
              "ck_clusters_batch")
        return [(cl[i, :nc[i]].copy(), pts[i, :npt[i]].copy()) for i in range(n)]

    def quads(self, frames=None, n=None, cap=1024):
        arr, keep, n = self._in(frames, n)
        q = (A.Quad * (n * cap))()
        nq = (C.c_int32 * n)()
        check(self._L.ck_quads_batch(self._h, arr, n, q, cap, nq), "ck_quads_batch")
        return [[q[i * cap + k] for k in range(nq[i])] for i in range(n)]

    def decode_quads(self, quads, frames=None, cap=64, return_status=False, raw=False):
        """The decode stage alone (ck_decode_quads_batch): quads is one list of ck_quad_t (_abi.Quad) per frame; frames None runs on
        the staged frames.  Returns what detect_batch returns; raw=True gives each frame's ck_detection_t records as bytes."""
        n = len(quads)
        arr = None if frames is None else _images(frames)
        if arr is not None and len(arr[0]) != n:
            raise ValueError("one list of quads per frame")
        stride = max([len(q) for q in quads] + [1])
        qa = (A.Quad * (max(n, 1) * stride))()
        nq = (C.c_int32 * max(n, 1))()
        for i, ql in enumerate(quads):
            nq[i] = len(ql)
            for k, q in enumerate(ql):
                qa[i * stride + k] = q
        dets = (A.Detection * (max(n, 1) * cap))()
        counts = (C.c_int32 * max(n, 1))()
        status = (C.c_uint32 * max(n, 1))()
        check(self._L.ck_decode_quads_batch(self._h, None if arr is None else arr[0], n, qa, stride, nq, dets, cap, counts, status),
              "ck_decode_quads_batch")
        if raw:
            sz = C.sizeof(A.Detection)
            out = [C.string_at(C.addressof(dets) + i * cap * sz, counts[i] * sz) for i in range(n)]
        else:
            out = [[Detection(dets[i * cap + k]) for k in range(counts[i])] for i in range(n)]
        return (out, list(status)[:n]) if return_status else out

    # -- the call the reference makes: detector.detect(&image) -----------------------------------------------
    def detect(self, frame, cap=64):
        return self.detect_batch(frame[None] if np.ndim(frame) == 2 else frame, cap)[0]

    def detect_batch(self, frames=None, cap=64, n=None, return_status=False):
        arr, keep, n = self._in(frames, n)
        dets = (A.Detection * (n * cap))()
        counts = (C.c_int32 * n)()
        status = (C.c_uint32 * n)()
        if arr is None:
            check(self._L.ck_detect_uploaded(self._h, n, dets, cap, counts, status), "ck_detect_uploaded")
        else:
            check(self._L.ck_detect_batch(self._h, arr, n, dets, cap, counts, status), "ck_detect_batch")
        out = [[Detection(dets[i * cap + k]) for k in range(counts[i])] for i in range(n)]
        return (out, list(status)) if return_status else out

    def detect_device(self, ptr, n, stride, frame_pitch, cap=64):
        dets = (A.Detection * (n * cap))()
        counts = (C.c_int32 * n)()
        status = (C.c_uint32 * n)()
        check(self._L.ck_detect_batch_device(self._h, C.c_void_p(ptr), n, stride, frame_pitch, dets, cap, counts,
                                             status), "ck_detect_batch_device")
        return [[Detection(dets[i * cap + k]) for k in range(counts[i])] for i in range(n)], list(status)

    # -- per-tag pose (AprilTag-3's estimate_tag_pose), on the GPU ---------------------------------------------------
    def estimate_tag_poses(self, dets, params, raw=False):
        """Poses of caller detections (Detection objects or ck_detection_t records): one TagPose per detection."""
        arr, n = _raw_detections(dets)
        out = (A.TagPose * max(n, 1))()
        check(self._L.ck_estimate_tag_poses(self._h, C.byref(params), arr, n, out), "ck_estimate_tag_poses")
        return out[:n] if raw else [TagPose(out[i]) for i in range(n)]

    def last_tag_poses(self, params, cap=64, raw=False):
        """Poses of the detections the last detect / process call of this handle produced (still on the device):
        a list per frame of that call, truncated to `cap` like the detections."""
        nb = self.max_batch
        out = (A.TagPose * (nb * cap))()
        counts = (C.c_int32 * nb)(*([-1] * nb))   # the call writes one count per frame of the last call: the rest stay -1
        check(self._L.ck_last_tag_poses(self._h, C.byref(params), out, cap, counts), "ck_last_tag_poses")
        n = sum(1 for c in counts if c >= 0)
        if raw:
            return [[out[i * cap + k] for k in range(counts[i])] for i in range(n)]
        return [[TagPose(out[i * cap + k]) for k in range(counts[i])] for i in range(n)]

    # -- JPEG preview of the staged frames, encoded on the GPU (the driver-station stream) ------------------------------
    def _preview_in(self, frames, n, width, height, quality, restart_rows, overlay, color=False):
        pp = preview_params(width, height, quality, restart_rows, overlay)
        pw, ph, max_bytes = (preview_color_layout if color else preview_layout)(pp, self.width, self.height)
        if frames is None:
            if n is None:
                raise ValueError("frames (indices into the staged frames) or n is required")
            return pp, pw, ph, max_bytes, None, int(n)
        idx = np.ascontiguousarray(frames, np.int32).reshape(-1)
        return pp, pw, ph, max_bytes, idx, idx.size

    def preview_jpeg(self, frames=None, n=None, width=640, height=480, quality=50, restart_rows=0, overlay=False, cap=None,
                     return_status=False):
        """Baseline JPEG files (bytes each) of staged frames, scaled to width x height (nearest neighbour; never enlarged) and
        encoded on the device exactly as libjpeg writes them.  frames: indices into the staged frames, or n for 0..n-1.
        overlay=True outlines the detections of the last detect / process call.  cap: bytes per file (default: the bound of
        ck_preview_layout); a file that does not fit comes back cut to cap with CK_PREVIEW_TRUNCATED in its status."""
        call = lambda pp, idx, n, out, c, sizes, status: self._L.ck_preview_jpeg(self._h, C.byref(pp), idx, n, out, c, sizes, status)
        return self._preview_files(call, "ck_preview_jpeg", False, frames, n, width, height, quality, restart_rows, overlay, cap, return_status)

    def _preview_files(self, call, name, color, frames, n, width, height, quality, restart_rows, overlay, cap, return_status):
        """The files of one of the preview entry points: call(pp, idx, n, out, cap, sizes, status) -> its return code."""
        pp, pw, ph, max_bytes, idx, n = self._preview_in(frames, n, width, height, quality, restart_rows, overlay, color)
        # without a cap the slots are sized for the pixels themselves (a file beyond that is noise at the highest qualities) and
        # the call is repeated with the bound of ck_preview_layout if a file did not fit; the buffer is kept between calls
        tries = [min(max_bytes, (3 if color else 1) * pw * ph + 1024), max_bytes] if cap is None else [int(cap)]
        for c in tries:
            need = max(n, 1) * max(c, 1)
            if getattr(self, "_pv_buf", None) is None or self._pv_buf.size < need:
                self._pv_buf = np.empty(need, np.uint8)
            out = self._pv_buf[:need].reshape(max(n, 1), max(c, 1))
            sizes = (C.c_int64 * max(n, 1))()
            status = (C.c_uint32 * max(n, 1))()
            check(call(pp, idx.ctypes.data if idx is not None else None, n, out.ctypes.data, c, sizes, status), name)
            if cap is not None or not any(status[:n]):
                break
        files = [out[i, :min(sizes[i], c)].tobytes() for i in range(n)]
        return (files, list(sizes)[:n], list(status)[:n]) if return_status else files

    def _preview_triples(self, call, name, frames, n, width, height, quality, restart_rows, overlay):
        """[n][ph][pw][3] uint8 of one of the ck_preview_color entry points: call(pp, idx, n, out) -> its return code."""
        pp, pw, ph, _, idx, n = self._preview_in(frames, n, width, height, quality, restart_rows, overlay, True)
        out = np.empty((n, ph, pw, 3), np.uint8)
        buf = out if n else np.empty(1, np.uint8)
        check(call(pp, idx.ctypes.data if idx is not None else None, n, buf.ctypes.data), name)
        return out

    # -- the same in colour, from the raw frames ---------------------------------------------------------------
    def preview_jpeg_color(self, frames=None, n=None, width=640, height=480, quality=50, restart_rows=0, overlay=False, cap=None,
                           return_status=False):
        """preview_jpeg in colour: three-component 4:4:4 files of the RAW frames the last upload_raw / raw_luma left on the
        device (a packed colour family: 'YUYV', 'UYVY', 'RGB3', 'BGR3', 'RGBA', 'BGRA'; or 'NV12', 'NV21', 'I420', 'YV12' uploaded
        with planes=True), or of the JPEG frames the last
        upload_jpeg(..., color=True) decoded, byte-equal to libjpeg's.  Valid until frames are staged another way."""
        call = lambda pp, idx, n, out, c, sizes, status: self._L.ck_preview_jpeg_color(self._h, C.byref(pp), idx, n, out, c, sizes, status)
        return self._preview_files(call, "ck_preview_jpeg_color", True, frames, n, width, height, quality, restart_rows, overlay, cap, return_status)

    def preview_color(self, frames=None, n=None, width=640, height=480, quality=50, restart_rows=0, overlay=False):
        """[n][ph][pw][3] uint8: the (Y, Cb, Cr) triples the colour encoder is given."""
        call = lambda pp, idx, n, out: self._L.ck_preview_color(self._h, C.byref(pp), idx, n, out)
        return self._preview_triples(call, "ck_preview_color", frames, n, width, height, quality, restart_rows, overlay)

    def preview_jpeg_color_device(self, ptr, n_frames, stride, frame_pitch, code, orientation="none", frames=None, n=None, width=640,
                                  height=480, quality=50, restart_rows=0, overlay=False, cap=None, return_status=False, planes=False):
        """preview_jpeg_color of n_frames raw frames in device memory (laid out as upload_raw_device takes them)."""
        fmt = raw_format(code, orientation, planes)
        call = lambda pp, idx, n, out, c, sizes, status: self._L.ck_preview_jpeg_color_device(
            self._h, C.byref(pp), C.c_void_p(ptr), stride, frame_pitch, C.byref(fmt), idx, n_frames, n, out, c, sizes, status)
        return self._preview_files(call, "ck_preview_jpeg_color_device", True, frames, n, width, height, quality, restart_rows, overlay, cap,
                                   return_status)

    def preview_color_device(self, ptr, n_frames, stride, frame_pitch, code, orientation="none", frames=None, n=None, width=640,
                             height=480, quality=50, restart_rows=0, overlay=False, planes=False):
        fmt = raw_format(code, orientation, planes)
        call = lambda pp, idx, n, out: self._L.ck_preview_color_device(self._h, C.byref(pp), C.c_void_p(ptr), stride, frame_pitch,
                                                                       C.byref(fmt), idx, n_frames, n, out)
        return self._preview_triples(call, "ck_preview_color_device", frames, n, width, height, quality, restart_rows, overlay)

    # -- coloured game pieces (chalkydri_amd/blobs.py has the parameters and the host twin) ------------------------
    def _frame_list(self, frames, n):
        if frames is None:
            if n is None:
                raise ValueError("frames (indices into the source's frames) or n is required")
            return None, None, int(n)
        idx = np.ascontiguousarray(frames, np.int32).reshape(-1)
        return idx, idx.ctypes.data, idx.size

    def _blob_records(self, call, name, params, frames, n, cap):
        """(records [n][n_classes][cap], counts [n][n_classes], status [n]) of one of the ck_detect_blobs entry points:
        call(pp, idx, n, out, cap, counts, status) -> its return code."""
        from .blobs import BLOB_DTYPE
        idx, ip, n = self._frame_list(frames, n)
        cap = params.max_targets if cap is None else int(cap)
        out = np.zeros((n, params.n_classes, cap), BLOB_DTYPE)
        counts, status = np.zeros((n, params.n_classes), np.int32), np.zeros(n, np.uint32)
        buf = out if out.size else np.zeros(1, BLOB_DTYPE)
        check(call(C.byref(params), ip, n, buf.ctypes.data, cap, counts.ctypes.data, status.ctypes.data), name)
        return out, counts, status

    def detect_blobs(self, params, frames=None, n=None, cap=None):
        """Coloured targets of the frames behind the staged ones (the RAW frames of the last upload_raw / raw_luma, or the JPEG
        frames of the last upload_jpeg(..., color=True)): blobs.blobs_host's triple, byte for byte, given blob_rgb's pixels.
        frames: indices (one may repeat), or n for 0..n-1.  cap: records per frame and class (None: params.max_targets)."""
        call = lambda pp, idx, n, out, cap, counts, status: self._L.ck_detect_blobs(self._h, pp, idx, n, out, cap, counts, status)
        return self._blob_records(call, "ck_detect_blobs", params, frames, n, cap)

    def detect_blobs_device(self, params, ptr, n_frames, stride, frame_pitch, code, orientation="none", frames=None, n=None, cap=None,
                            planes=False):
        """detect_blobs of n_frames raw frames in device memory (laid out as upload_raw_device takes them)."""
        fmt = raw_format(code, orientation, planes)
        call = lambda pp, idx, n, out, cap, counts, status: self._L.ck_detect_blobs_device(
            self._h, pp, C.c_void_p(ptr), stride, frame_pitch, C.byref(fmt), idx, n_frames, n, out, cap, counts, status)
        return self._blob_records(call, "ck_detect_blobs_device", params, frames, n_frames if n is None and frames is None else n, cap)

    def blob_rgb(self, frames=None, n=None, device=None):
        """[n][H][W][3] uint8: the RGB the classifier sees.  device: (ptr, n_frames, stride, frame_pitch, code, orientation[, planes])
        for raw frames in device memory instead of the frames behind the staged ones."""
        idx, ip, n = self._frame_list(frames, n)
        out = np.empty((n, self.height, self.width, 3), np.uint8)
        buf = out if n else np.empty(1, np.uint8)
        if device is None:
            check(self._L.ck_blob_rgb(self._h, ip, n, buf.ctypes.data), "ck_blob_rgb")
        else:
            ptr, n_frames, stride, pitch, code, orientation = device[:6]
            fmt = raw_format(code, orientation, *device[6:])
            check(self._L.ck_blob_rgb_device(self._h, C.c_void_p(ptr), stride, pitch, C.byref(fmt), ip, n_frames, n, buf.ctypes.data), "ck_blob_rgb_device")
        return out

    def blob_mask(self, params, cls=0, stage=1, frames=None, n=None, device=None):
        """[n][H][ceil(W/32)] uint32: class cls's packed plane after the threshold (stage 0) or the morphology (1);
        blobs.mask_host's bytes.  device: as blob_rgb's."""
        idx, ip, n = self._frame_list(frames, n)
        out = np.zeros((n, self.height, (self.width + 31) // 32), np.uint32)
        buf = out if n else np.zeros(1, np.uint32)
        if device is None:
            check(self._L.ck_blob_mask(self._h, C.byref(params), ip, n, int(cls), int(stage), buf.ctypes.data), "ck_blob_mask")
        else:
            ptr, n_frames, stride, pitch, code, orientation = device[:6]
            fmt = raw_format(code, orientation, *device[6:])
            check(self._L.ck_blob_mask_device(self._h, C.byref(params), C.c_void_p(ptr), stride, pitch, C.byref(fmt), ip, n_frames, n, int(cls),
                                              int(stage), buf.ctypes.data), "ck_blob_mask_device")
        return out

    def blob_time(self, params, ptr, n_frames, stride, frame_pitch, code, orientation="none", n=None, reps=10, planes=False):
        """ck_blob_time: mean milliseconds of the kernels of one detect_blobs_device call on frames 0..n-1."""
        fmt, ms = raw_format(code, orientation, planes), C.c_float()
        check(self._L.ck_blob_time(self._h, C.byref(params), C.c_void_p(ptr), stride, frame_pitch, C.byref(fmt), n_frames,
                                   n_frames if n is None else int(n), int(reps), C.byref(ms)), "ck_blob_time")
        return ms.value

    def preview_luma(self, frames=None, n=None, width=640, height=480, quality=50, restart_rows=0, overlay=False):
        """[n][ph][pw] uint8: the scaled (+ overlaid) pixels the encoder is given."""
        pp, pw, ph, _, idx, n = self._preview_in(frames, n, width, height, quality, restart_rows, overlay)
        out = np.empty((n, ph, pw), np.uint8)
        buf = out if n else np.empty(1, np.uint8)
        check(self._L.ck_preview_luma(self._h, C.byref(pp), idx.ctypes.data if idx is not None else None, n, buf.ctypes.data),
              "ck_preview_luma")
        return out

    # -- exposure metering of the staged frames, on the GPU (chalkydri_amd/exposure.py has the parameters and the controller) ----
    def exposure_stats(self, n=None, frames=None, roi=None, params=None):
        """One ck_exposure_stats_t per metered frame, as a structured numpy array (fields luma [256], grad [7][192], n_luma,
        n_grad): the luma histogram and, per gamma curve of `params` (ExposureParams; None: the defaults), the histogram of the
        Sobel gradient magnitude, over `roi`.  frames: indices into the staged frames, or n for 0..n-1.  roi: None (whole
        frames), one (x0, y0, x1, y1) for every frame, or one per frame; half-open, clamped to the frame."""
        from . import exposure as X
        return X.stats_call(self, None, n, frames, roi, params)

    def stage_ms(self):
        ms = A.StageMs()
        check(self._L.ck_last_stage_ms(self._h, C.byref(ms)), "ck_last_stage_ms")
        return {k: getattr(ms, k) for k, _ in A.StageMs._fields_}

    def fp64_probe(self, op, a, b=None):
        a = np.ascontiguousarray(a, np.float64)
        out = np.empty_like(a)
        bb = np.ascontiguousarray(b, np.float64) if b is not None else None
        check(self._L.ck_selftest_fp64(self._h, op, a.ctypes.data, bb.ctypes.data if bb is not None else None,
                                       a.size, out.ctypes.data), "ck_selftest_fp64")
        return out

    def _in(self, frames, n):
        if frames is None:
            if n is None:
                raise ValueError("n is required when running on uploaded frames")
            return None, None, n
        arr, keep = _images(frames)
        return arr, keep, len(arr)


def fourcc(code):
    """'GREY' -> the little-endian u32 the C ABI takes (crates/chalkydri/src/cameras/gst_to_cu.rs:171-179)."""
    b = code.encode("ascii")
    if len(b) != 4:
        raise ValueError("fourcc must be exactly 4 characters")
    return int.from_bytes(b, "little")


class IngestRing:
    """Pinned host slots + asynchronous upload in front of a detector (the pooled host buffers of the reference's camera
    layer, gst_to_cu.rs:49-72,131-188).  slot_view(s) is a writable numpy view [max_batch][h][stride] of pinned memory.
    With a fourcc the slots hold RAW frames of that format ([max_batch][sh][raw stride]; with planes=True the chroma planes too,
    [max_batch][sh + ch][raw stride]); submit converts and orients them on the device, and detect / process work as on a plain ring.  With fourcc "MJPG" (or "JPEG") the slots take one compressed
    frame per index (write(slot, index, data) with bytes, at most max_frame_bytes each; 0 = sw * sh); submit decodes and
    orients them on the ring's copy stream, and jpeg_status(slot, n) gives their CK_JPEG_* words; with color=True the slots also
    keep their frames' chroma planes (ck_ingest_create_jpeg_color), the source of preview_jpeg_color / preview_color."""

    def __init__(self, detector, n_slots=2, fourcc=None, orientation="none", max_frame_bytes=0, color=False, planes=False):
        self.det, self._L = detector, detector._L
        g = C.c_void_p()
        self._g = None
        self.code, self.rows = fourcc, detector.height
        self.jpeg = isinstance(fourcc, str) and fourcc in A.JPEG_FOURCCS
        if color and not self.jpeg:
            raise ValueError("color=True is an option of a JPEG ring: a raw ring keeps its raw frames anyway")
        if planes and (fourcc is None or self.jpeg):
            raise ValueError("planes=True is an option of a raw ring of a planar format")
        if fourcc is None:
            check(self._L.ck_ingest_create(detector._h, n_slots, C.byref(g)), "ck_ingest_create")
        elif self.jpeg:
            o = orientation_code(orientation)
            if color:
                check(self._L.ck_ingest_create_jpeg_color(detector._h, n_slots, o, int(max_frame_bytes), C.byref(g)), "ck_ingest_create_jpeg_color")
            else:
                check(self._L.ck_ingest_create_jpeg(detector._h, n_slots, o, int(max_frame_bytes), C.byref(g)), "ck_ingest_create_jpeg")
        else:
            fmt = raw_format(fourcc, orientation, planes)
            # (the layout first: an unknown fourcc or orientation is refused on the host, before the ring touches the device)
            self.sw, self.sh, self.min_stride, _ = raw_layout(fmt.fourcc, detector.width, detector.height, fmt.orientation)
            self.rows = _raw_rows(fmt, detector.width, detector.height)[2]   # sh, and the chroma rows behind them with planes
            check(self._L.ck_ingest_create_raw(detector._h, n_slots, C.byref(fmt), C.byref(g)), "ck_ingest_create_raw")
        self._g, self.n_slots = g, n_slots
        self.stride = self._L.ck_ingest_stride(g)

    def close(self):
        if self._g:
            self._L.ck_ingest_destroy(self._g)
            self._g = None

    def slot_view(self, slot):
        cfg = self.det.cfg
        ptr = self._L.ck_ingest_frame(self._g, slot, 0)
        pitch = self._L.ck_ingest_frame(self._g, slot, 1) - ptr if cfg.max_batch > 1 else self.stride * self.rows
        buf = (C.c_uint8 * (pitch * cfg.max_batch)).from_address(ptr)
        a = np.frombuffer(buf, np.uint8).reshape(cfg.max_batch, pitch)[:, :self.stride * self.rows]
        return a.reshape(cfg.max_batch, self.rows, self.stride)

    def write(self, slot, index, frame, code=None):
        """Stride-aware copy of one caller frame into the slot: a luma frame [h][>=w] on a plain ring, a raw frame
        [sh][>=min_stride bytes] of the ring's format family on a raw ring, the bytes of one JPEG on a JPEG ring."""
        if self.jpeg:
            b = np.frombuffer(bytes(frame), np.uint8)
            check(self._L.ck_ingest_write_jpeg(self._g, slot, index, b.ctypes.data if b.size else None, b.size), "ck_ingest_write_jpeg")
            return
        if self.code is None:
            arr, keep = _images(frame)
        else:
            arr, keep = _raw_images(frame, self.sw, self.sh)
        code = code or self.code or "GREY"
        check(self._L.ck_ingest_write(self._g, slot, index, arr, fourcc(code)), "ck_ingest_write")

    def submit(self, slot, n):
        check(self._L.ck_ingest_submit(self._g, slot, n), "ck_ingest_submit")

    def jpeg_status(self, slot, n):
        """The CK_JPEG_* words of the n frames the slot was submitted with (waits for the slot's decode)."""
        status = (C.c_uint32 * max(n, 1))()
        check(self._L.ck_ingest_jpeg_status(self._g, slot, n, status), "ck_ingest_jpeg_status")
        return list(status)[:n]

    def exposure_stats(self, slot, n=None, frames=None, roi=None, params=None):
        """AprilTagDetector.exposure_stats on the frames of a submitted slot (waits for its upload; the slot stays as it is)."""
        from . import exposure as X
        return X.stats_call(self.det, (self._g, slot), n, frames, roi, params)

    def preview_jpeg_color(self, slot, frames=None, n=None, width=640, height=480, quality=50, restart_rows=0, overlay=False, cap=None,
                           return_status=False):
        """AprilTagDetector.preview_jpeg_color on the raw frames of a submitted slot of a raw ring, or on the decoded frames of a
        slot of a JPEG ring made with color=True (waits for its upload; the slot stays as it is).  frames: indices below the count the slot was submitted with."""
        call = lambda pp, idx, n, out, c, sizes, status: self._L.ck_preview_jpeg_color_ingested(self._g, slot, C.byref(pp), idx, n, out, c,
                                                                                               sizes, status)
        return self.det._preview_files(call, "ck_preview_jpeg_color_ingested", True, frames, n, width, height, quality, restart_rows,
                                       overlay, cap, return_status)

    def preview_color(self, slot, frames=None, n=None, width=640, height=480, quality=50, restart_rows=0, overlay=False):
        call = lambda pp, idx, n, out: self._L.ck_preview_color_ingested(self._g, slot, C.byref(pp), idx, n, out)
        return self.det._preview_triples(call, "ck_preview_color_ingested", frames, n, width, height, quality, restart_rows, overlay)

    def detect_blobs(self, slot, params, frames=None, n=None, cap=None):
        """AprilTagDetector.detect_blobs on the raw frames of a submitted slot of a raw ring, or on the decoded frames of a slot of
        a JPEG ring made with color=True (waits for its upload; the slot stays as it is)."""
        call = lambda pp, idx, n, out, cap, counts, status: self._L.ck_detect_blobs_ingested(self._g, slot, pp, idx, n, out, cap, counts, status)
        return self.det._blob_records(call, "ck_detect_blobs_ingested", params, frames, n, cap)

    def detect(self, slot, n, cap=64):
        dets = (A.Detection * (cap * n))()
        counts = (C.c_int32 * n)()
        status = (C.c_uint32 * n)()
        check(self._L.ck_detect_ingested(self._g, slot, n, dets, cap, counts, status), "ck_detect_ingested")
        return [[Detection(dets[i * cap + k]) for k in range(min(counts[i], cap))] for i in range(n)], np.array(status[:])

    def process(self, slot, n, pp, gyro, has_gyro):
        out = (A.VisionMeasurement * n)()
        valid = (C.c_int32 * n)()
        g = np.ascontiguousarray(gyro, np.float64)
        hg = np.ascontiguousarray(has_gyro, np.uint8)
        if g.size != n or hg.size != n:
            raise ValueError("gyro / has_gyro must hold one entry per submitted frame")
        check(self._L.ck_process_ingested(self._g, slot, n, C.byref(pp), g.ctypes.data, hg.ctypes.data, out, valid), "ck_process_ingested")
        return out, np.array(valid[:])
