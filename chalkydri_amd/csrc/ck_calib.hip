// Camera calibration: the host half that drives the device.  Validates a call (ck_calib_check, before any device is
// touched), grows the workspace, writes every problem's start into its result record, copies the call's arrays over, runs k_calib on
// the handle's stream and brings results and poses back.
#include <string.h>

#include <vector>

#include "ck_calib.h"
#include "ck_calib_math.h"

static_assert(sizeof(ck_calib_params_t) == 24, "ck_calib_params_t layout");
static_assert(sizeof(ck_calib_problem_t) == 16, "ck_calib_problem_t layout");
static_assert(sizeof(ck_calib_result_t) == 112, "ck_calib_result_t layout");
static_assert(sizeof(ck_opencv5_t) == 9 * sizeof(double), "ck_opencv5_t is nine doubles");
static_assert(CKC_WS_COST < CKC_WS_STRIDE, "frame record layout");

static int refine_batch(ck_handle_t *h, const ck_calib_params_t *p, const ck_calib_problem_t *problems, int32_t n, const double *board_xy,
                        const double *image_uv, const int32_t *frame_start, int32_t n_points, int32_t n_starts, int32_t n_frames,
                        ck_calib_result_t *results, double *poses, std::vector<int32_t> &rec0) {
    int64_t n_rec = 0;
    for (int32_t i = 0; i < n; i++) {
        const ck_calib_problem_t &q = problems[i];
        const int32_t *fs = frame_start + q.start_offset;
        ck_calib_result_t &r = results[i];
        const ck_opencv5_t cam0 = r.cam;
        memset(&r, 0, sizeof r);
        r.cam = cam0;
        r.n_frames = q.n_frames; r.n_points = fs[q.n_frames] - fs[0];
        r.status = ck_calib_start_ok((const double *)&cam0, poses + 12 * (size_t)q.pose_offset, q.n_frames) ? -1 : CK_CALIB_DEGENERATE;
        rec0[i] = (int32_t)n_rec;
        n_rec += q.n_frames;
    }
    if (n_rec >= ((int64_t)1 << 31) / CKC_WS_STRIDE) return CK_ECAPACITY;
    CK_HIP(hipSetDevice(h->device));
    if (!ck_workspace(h->calib)) return CK_ENOMEM;
    ck_calib_ws &W = *h->calib;
    const size_t pt_bytes = sizeof(double) * 2 * (size_t)n_points, pose_bytes = sizeof(double) * 12 * (size_t)n_frames;
    int rc = ck_upload(W.d_prob, problems, sizeof(ck_calib_problem_t) * (size_t)n, h->stream);
    if (rc == CK_OK) rc = ck_upload(W.d_rec0, rec0.data(), sizeof(int32_t) * (size_t)n, h->stream);
    if (rc == CK_OK) rc = ck_upload(W.d_fs, frame_start, sizeof(int32_t) * (size_t)n_starts, h->stream);
    if (rc == CK_OK) rc = ck_upload(W.d_bxy, board_xy, pt_bytes, h->stream);
    if (rc == CK_OK) rc = ck_upload(W.d_uv, image_uv, pt_bytes, h->stream);
    if (rc == CK_OK) rc = W.d_rec.reserve(sizeof(double) * CKC_WS_STRIDE * (size_t)n_rec);
    if (rc == CK_OK) rc = ck_upload(W.d_poses, poses, pose_bytes, h->stream);
    if (rc == CK_OK) rc = ck_upload(W.d_res, results, sizeof(ck_calib_result_t) * (size_t)n, h->stream);
    if (rc != CK_OK) return rc;
    rc = ck_launch_calib(h->stream, *p, W.d_prob, W.d_rec0, n, W.d_fs, W.d_bxy, W.d_uv, W.d_rec, W.d_poses, W.d_res);
    if (rc != CK_OK) return rc;
    CK_HIP(hipMemcpyAsync(results, W.d_res, sizeof(ck_calib_result_t) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    CK_HIP(hipMemcpyAsync(poses, W.d_poses, pose_bytes, hipMemcpyDeviceToHost, h->stream));
    CK_HIP(hipStreamSynchronize(h->stream));
    return CK_OK;
}

extern "C" int ck_calib_refine_batch(ck_handle_t *h, const ck_calib_params_t *p, const ck_calib_problem_t *problems, int32_t n,
                                     const double *board_xy, const double *image_uv, const int32_t *frame_start, int32_t n_points,
                                     int32_t n_starts, int32_t n_frames, const ck_opencv5_t *cams0, const double *poses0,
                                     ck_calib_result_t *results, double *poses_out) {
    if (!h || !cams0 || !poses0 || !results || !poses_out) return CK_EINVAL;
    int rc = ck_calib_check(p, problems, n, board_xy, image_uv, frame_start, n_points, n_starts, n_frames);
    if (rc != CK_OK || n == 0) return rc;
    std::vector<int32_t> rec0;
    try {
        rec0.resize((size_t)n);
    } catch (...) {
        return CK_ENOMEM;
    }
    for (int32_t i = 0; i < n; i++) {
        results[i].cam = cams0[i];
        const size_t o = 12 * (size_t)problems[i].pose_offset;
        if (poses_out != poses0) memmove(poses_out + o, poses0 + o, sizeof(double) * 12 * (size_t)problems[i].n_frames);
    }
    return refine_batch(h, p, problems, n, board_xy, image_uv, frame_start, n_points, n_starts, n_frames, results, poses_out, rec0);
}

extern "C" int ck_calibrate_batch(ck_handle_t *h, const ck_calib_params_t *p, const ck_calib_problem_t *problems, int32_t n,
                                  const double *board_xy, const double *image_uv, const int32_t *frame_start, int32_t n_points,
                                  int32_t n_starts, int32_t n_frames, ck_calib_result_t *results, double *poses_out) {
    if (!h || !results || !poses_out) return CK_EINVAL;
    int rc = ck_calib_check(p, problems, n, board_xy, image_uv, frame_start, n_points, n_starts, n_frames);
    if (rc != CK_OK || n == 0) return rc;
    std::vector<int32_t> rec0;
    try {
        rec0.resize((size_t)n);
    } catch (...) {
        return CK_ENOMEM;
    }
    for (int32_t i = 0; i < n; i++) {
        int32_t st;
        rc = ck_calib_init(p, problems + i, board_xy, image_uv, frame_start, n_points, n_starts, n_frames, &results[i].cam, poses_out, &st);
        if (rc != CK_OK) return rc; // (a start without a solution is a zero camera: refine_batch marks it DEGENERATE)
    }
    return refine_batch(h, p, problems, n, board_xy, image_uv, frame_start, n_points, n_starts, n_frames, results, poses_out, rec0);
}
