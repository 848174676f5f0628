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

static_assert(sizeof(ck_camera_calib_result_t) == 128, "ck_camera_calib_result_t layout");

// model: CK_CAMERA_*; results[i].cam holds the start in the solver's nine slots (an EUCM / UCM problem its six parameters)
static int refine_batch(ck_handle_t *h, int model, const ck_calib_params_t *p, const ck_calib_problem_t *problems, int32_t n, const double *board_xy,
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
    rc = ck_launch_calib(h->stream, model, *p, W.d_prob, W.d_rec0, n, W.d_fs, W.d_bxy, W.d_uv, W.d_rec, W.d_poses, W.d_res);
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
    return refine_batch(h, CK_CAMERA_OPENCV5, p, problems, n, board_xy, image_uv, frame_start, n_points, n_starts, n_frames, results, poses_out, rec0);
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
    return refine_batch(h, CK_CAMERA_OPENCV5, p, problems, n, board_xy, image_uv, frame_start, n_points, n_starts, n_frames, results, poses_out, rec0);
}

// ---- any camera model ----------------------------------------------------------------------------------------
static bool camera_model_ok(int32_t m) { return m == CK_CAMERA_OPENCV5 || m == CK_CAMERA_EUCM || m == CK_CAMERA_UCM; }

extern "C" int ck_camera_calib_refine_batch(ck_handle_t *h, int32_t model, const ck_calib_params_t *p, const ck_calib_problem_t *problems,
                                            int32_t n, const double *board_xy, const double *image_uv, const int32_t *frame_start,
                                            int32_t n_points, int32_t n_starts, int32_t n_frames, const ck_camera_t *cams0,
                                            const double *poses0, ck_camera_calib_result_t *results, double *poses_out) {
    if (!h || !cams0 || !poses0 || !results || !poses_out || !camera_model_ok(model)) return CK_EINVAL;
    int rc = ck_calib_check(p, problems, n, board_xy, image_uv, frame_start, n_points, n_starts, n_frames);
    if (rc != CK_OK || n == 0) return rc;
    std::vector<int32_t> rec0;
    std::vector<ck_calib_result_t> res;
    try {
        rec0.resize((size_t)n);
        res.resize((size_t)n);
    } catch (...) {
        return CK_ENOMEM;
    }
    for (int32_t i = 0; i < n; i++) {
        ck_calib_start_from_camera(model, cams0 + i, &res[i].cam);
        const size_t o = 12 * (size_t)problems[i].pose_offset;
        if (poses_out != poses0) memmove(poses_out + o, poses0 + o, sizeof(double) * 12 * (size_t)problems[i].n_frames);
    }
    rc = refine_batch(h, model, p, problems, n, board_xy, image_uv, frame_start, n_points, n_starts, n_frames, res.data(), poses_out, rec0);
    if (rc != CK_OK) return rc;
    for (int32_t i = 0; i < n; i++) ck_calib_result_to_camera(model, &res[i], 0, 1, results + i);
    return CK_OK;
}

// Every problem S times, once per start: copy s of problem i shares the problem's points and keeps its poses in a pose array of its
// own, S times the caller's, at pose_offset + s * n_frames.  One launch solves them all; the host picks per problem.
extern "C" int ck_camera_calibrate_batch(ck_handle_t *h, int32_t model, const ck_calib_params_t *p, const ck_calib_problem_t *problems,
                                         int32_t n, const double *board_xy, const double *image_uv, const int32_t *frame_start,
                                         int32_t n_points, int32_t n_starts, int32_t n_frames, ck_camera_calib_result_t *results,
                                         double *poses_out) {
    if (!h || !results || !poses_out || !camera_model_ok(model)) return CK_EINVAL;
    int rc = ck_calib_check(p, problems, n, board_xy, image_uv, frame_start, n_points, n_starts, n_frames);
    if (rc != CK_OK || n == 0) return rc;
    const int S = model == CK_CAMERA_OPENCV5 ? 1 : CK_CAMCAL_STARTS;
    if ((int64_t)S * n_frames >= ((int64_t)1 << 31) || (int64_t)S * n >= ((int64_t)1 << 31)) return CK_ECAPACITY;
    std::vector<int32_t> rec0;
    std::vector<ck_calib_result_t> res;
    std::vector<ck_calib_problem_t> prob;
    std::vector<double> poses;
    try {
        rec0.resize((size_t)S * n);
        res.resize((size_t)S * n);
        prob.resize((size_t)S * n);
        poses.assign((size_t)12 * S * n_frames, 0.0);
    } catch (...) {
        return CK_ENOMEM;
    }
    for (int32_t i = 0; i < n; i++)
        for (int s = 0; s < S; s++) {
            ck_calib_problem_t &q = prob[(size_t)i * S + s];
            q = problems[i];
            q.pose_offset = problems[i].pose_offset + s * n_frames;
            ck_camera_t cam0;
            int32_t st;
            rc = ck_camera_calib_init(model, p, &q, board_xy, image_uv, frame_start, n_points, n_starts, S * n_frames, s, &cam0, poses.data(), &st);
            if (rc != CK_OK) return rc; // (a start without a solution is a zero camera: refine_batch marks it DEGENERATE)
            ck_calib_start_from_camera(model, &cam0, &res[(size_t)i * S + s].cam);
            if (st != CK_CALIB_CONVERGED) memset(&res[(size_t)i * S + s].cam, 0, sizeof(ck_opencv5_t));
        }
    rc = refine_batch(h, model, p, prob.data(), S * n, board_xy, image_uv, frame_start, n_points, n_starts, S * n_frames, res.data(), poses.data(), rec0);
    if (rc != CK_OK) return rc;
    for (int32_t i = 0; i < n; i++) {
        int best = -1;
        for (int s = 0; s < S; s++) {
            const ck_calib_result_t &r = res[(size_t)i * S + s];
            if (r.status == CK_CALIB_DEGENERATE || !(r.cost - r.cost == 0.0)) continue; // (not finite)
            if (best < 0 || r.cost < res[(size_t)i * S + best].cost) best = s;
        }
        const int take = best < 0 ? 0 : best;
        ck_calib_result_to_camera(model, &res[(size_t)i * S + take], take, S, results + i);
        memcpy(poses_out + 12 * (size_t)problems[i].pose_offset, poses.data() + 12 * (size_t)prob[(size_t)i * S + take].pose_offset,
               sizeof(double) * 12 * (size_t)problems[i].n_frames);
    }
    return CK_OK;
}
