// ck_rig_refine.hip — the entry points of the rig pose refinement: checks, the handle's workspace, uploads, the launch
// of k_rig_refine.hip.  What needs no device (the checks, the twin) is ck_rig_refine_host.c's.
#include <math.h>
#include <string.h>

#include <vector>

#include "ck_internal.h"
#include "ck_rig.h"
#include "ck_rig_refine.h"

namespace {

bool on_device(const void *p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeDevice;
}

// The stand-alone call up to, not including, the wait for the stream: checks, uploads, launch.  `keep` holds the pageable sources of the
// copies until the caller has waited.
struct staged_t {
    std::vector<ck_sqpnp_problem_t> rec;
    std::vector<double> cs;
    int32_t max_points = 0;
};
int refine_enqueue(ck_handle_t *h, const ck_rig_refine_params_t *params, int32_t n_cams, const ck_sqpnp_problem_t *problems, int32_t n,
                   const ck_iso3_t *tags, int32_t n_tags_total, const double *bearings, int32_t n_bearings_total, const double *gyro,
                   const ck_rig_result_t *start, const uint64_t *rejected, ck_rig_refined_t *out, staged_t &keep, ck_rig_refine_args &a) {
    if (!h || !params || !problems || !start || !out || n < 0 || n_cams < 1 || n_cams > CK_RIG_MAX_CAMS) return CK_EINVAL;
    if (n == 0) return ck_rig_refine_check(params, n_cams, problems, 0, tags, n_tags_total, bearings, n_bearings_total, gyro, start, out, nullptr);
    CK_HIP(hipSetDevice(h->device));
    // the records may lie on the device: the checks read a host copy
    keep.rec.resize((size_t)n_cams * (size_t)n);
    CK_HIP(hipMemcpy(keep.rec.data(), problems, sizeof(ck_sqpnp_problem_t) * keep.rec.size(), hipMemcpyDefault));
    int rc = ck_rig_refine_check(params, n_cams, keep.rec.data(), n, tags, n_tags_total, bearings, n_bearings_total, gyro, start, out, &keep.max_points);
    if (rc != CK_OK) return rc;
    ck_rig_refine_ws *ws = ck_workspace(h->rig_refine);
    if (!ws) return CK_ENOMEM;
    const int cap = keep.max_points > 0 ? keep.max_points : 1;
    const bool prior = params->gyro_sigma_rad > 0.0, dev_gyro = prior && on_device(gyro);
    if ((rc = ws->d_pts.reserve(sizeof(double) * CKF_PT * (size_t)n * (size_t)cap)) != CK_OK) return rc;
    if ((rc = ws->d_out.reserve(sizeof(ck_rig_refined_t) * (size_t)n)) != CK_OK) return rc;
    if ((rc = ws->d_gyro.reserve(sizeof(double) * 2 * (size_t)n)) != CK_OK) return rc;
    if ((rc = ws->d_start.reserve(sizeof(ck_rig_result_t) * (size_t)n)) != CK_OK) return rc;
    if ((rc = ws->d_rejected.reserve(sizeof(uint64_t) * CK_RIG_MAX_CAMS * (size_t)n)) != CK_OK) return rc;
    if ((rc = ws->d_prob.reserve(sizeof(ck_sqpnp_problem_t) * keep.rec.size())) != CK_OK) return rc;
    if ((rc = ws->d_tags.reserve(sizeof(ck_iso3_t) * (size_t)(n_tags_total ? n_tags_total : 1))) != CK_OK) return rc;
    if ((rc = ws->d_bearings.reserve(sizeof(double) * 3 * (size_t)(n_bearings_total ? n_bearings_total : 1))) != CK_OK) return rc;
    CK_HIP(hipMemcpyAsync(ws->d_prob, keep.rec.data(), sizeof(ck_sqpnp_problem_t) * keep.rec.size(), hipMemcpyHostToDevice, h->stream));
    if (n_tags_total) CK_HIP(hipMemcpyAsync(ws->d_tags, tags, sizeof(ck_iso3_t) * (size_t)n_tags_total, hipMemcpyDefault, h->stream));
    if (n_bearings_total) CK_HIP(hipMemcpyAsync(ws->d_bearings, bearings, sizeof(double) * 3 * (size_t)n_bearings_total, hipMemcpyDefault, h->stream));
    CK_HIP(hipMemcpyAsync(ws->d_start, start, sizeof(ck_rig_result_t) * (size_t)n, hipMemcpyDefault, h->stream));
    if (rejected) CK_HIP(hipMemcpyAsync(ws->d_rejected, rejected, sizeof(uint64_t) * CK_RIG_MAX_CAMS * (size_t)n, hipMemcpyDefault, h->stream));
    if (dev_gyro) {
        CK_HIP(hipMemcpyAsync(ws->d_gyro, gyro, sizeof(double) * (size_t)n, hipMemcpyDefault, h->stream));
    } else if (prior) { // the heading's cosine and sine as the twin takes them
        keep.cs.resize(2 * (size_t)n);
        for (int32_t s = 0; s < n; s++) { keep.cs[2 * (size_t)s] = cos(gyro[s]); keep.cs[2 * (size_t)s + 1] = sin(gyro[s]); }
        CK_HIP(hipMemcpyAsync(ws->d_gyro, keep.cs.data(), sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, h->stream));
    }
    memset(&a, 0, sizeof a);
    a.prm = *params;
    for (int c = 0; c < n_cams; c++) a.cam[c] = {ws->d_prob.p + (size_t)c * n, ws->d_tags, ws->d_bearings, 0, 0};
    a.n_cams = n_cams; a.n = n; a.max_points = cap;
    a.device_heading = dev_gyro ? 1 : 0;
    a.gyro = prior ? ws->d_gyro.p : nullptr;
    a.start = reinterpret_cast<const char *>(ws->d_start.p); a.start_stride = sizeof(ck_rig_result_t);
    a.rejected = rejected ? ws->d_rejected.p : nullptr; a.rejected_stride = CK_RIG_MAX_CAMS;
    a.pts = ws->d_pts; a.out = ws->d_out;
    return ck_launch_rig_refine(h->stream, a);
}

} // namespace

extern "C" int ck_rig_refine_batch(ck_handle_t *h, const ck_rig_refine_params_t *params, int32_t n_cams, const ck_sqpnp_problem_t *problems,
                                   int32_t n, const ck_iso3_t *tags, int32_t n_tags_total, const double *bearings, int32_t n_bearings_total,
                                   const double *gyro, const ck_rig_result_t *start, const uint64_t *rejected, ck_rig_refined_t *out) {
    staged_t keep;
    ck_rig_refine_args a;
    const int rc = refine_enqueue(h, params, n_cams, problems, n, tags, n_tags_total, bearings, n_bearings_total, gyro, start, rejected, out, keep, a);
    if (rc != CK_OK && !keep.rec.empty()) (void)hipStreamSynchronize(h->stream); // (copies from `keep` and the caller may be in flight)
    if (rc != CK_OK || n == 0) return rc;
    CK_HIP(hipMemcpyAsync(out, h->rig_refine->d_out, sizeof(ck_rig_refined_t) * (size_t)n, hipMemcpyDefault, h->stream));
    CK_HIP(hipStreamSynchronize(h->stream));
    return CK_OK;
}

namespace {

// What ck_rig_process_last_refined enqueues behind ck_rig_enqueue_last: the workspace, k_rig_refine over the records and buffers in
// place, the refined records and the measurements out
int refined_enqueue(ck_handle_t *const *handles, int32_t n_cams, int32_t n, const ck_rig_robust_params_t *rp,
                    const ck_rig_refine_params_t *refine_params, ck_rig_ws *rig, ck_rig_refined_t *out, ck_vision_measurement_t *meas) {
    ck_handle *h = handles[0];
    int rc;
    ck_rig_refine_ws *ws = ck_workspace(h->rig_refine);
    if (!ws) return CK_ENOMEM;
    int max_points = 0;
    for (int c = 0; c < n_cams; c++) max_points += 4 * handles[c]->ws.det_cap;
    if (max_points < 1) max_points = 1;
    if ((rc = ws->d_pts.reserve(sizeof(double) * CKF_PT * (size_t)n * (size_t)max_points)) != CK_OK) return rc;
    if ((rc = ws->d_out.reserve(sizeof(ck_rig_refined_t) * (size_t)n)) != CK_OK) return rc;
    ck_rig_refine_args a;
    memset(&a, 0, sizeof a);
    a.prm = *refine_params;
    for (int c = 0; c < n_cams; c++) {
        const ck_stage_ws &w = handles[c]->ws;
        a.cam[c] = {w.d_problems, w.d_pose_tags, w.d_bearings, w.det_cap, 0};
    }
    a.n_cams = n_cams; a.n = n; a.max_points = max_points;
    a.device_heading = 1;
    a.gyro = refine_params->gyro_sigma_rad > 0.0 ? rig->d_gyro.p : nullptr;
    if (rp) {
        a.start = reinterpret_cast<const char *>(rig->d_rres.p); a.start_stride = sizeof(ck_rig_robust_result_t);
        a.rejected = reinterpret_cast<const uint64_t *>(reinterpret_cast<const char *>(rig->d_rres.p) + offsetof(ck_rig_robust_result_t, rejected));
        a.rejected_stride = sizeof(ck_rig_robust_result_t) / sizeof(uint64_t);
    } else {
        a.start = reinterpret_cast<const char *>(rig->d_res.p); a.start_stride = sizeof(ck_rig_result_t);
    }
    a.pts = ws->d_pts; a.out = ws->d_out; a.meas = rig->d_meas;
    if ((rc = ck_launch_rig_refine(h->stream, a)) != CK_OK) return rc;
    CK_HIP(hipMemcpyAsync(out, ws->d_out, sizeof(ck_rig_refined_t) * (size_t)n, hipMemcpyDefault, h->stream));
    CK_HIP(hipMemcpyAsync(meas, rig->d_meas, sizeof(ck_vision_measurement_t) * (size_t)n, hipMemcpyDefault, h->stream));
    return CK_OK;
}

} // namespace

extern "C" int ck_rig_process_last_refined(ck_handle_t *const *handles, int32_t n_cams, int32_t n, const ck_rig_robust_params_t *robust_params,
                                           int32_t use_robust, const ck_rig_refine_params_t *refine_params, const double *gyro,
                                           const uint8_t *has_gyro, void *start_out, ck_rig_refined_t *out, ck_vision_measurement_t *meas,
                                           int32_t *valid) {
    if (!robust_params || !refine_params || !out) return CK_EINVAL;
    int rc = ck_rig_refine_params_check(refine_params);
    if (rc != CK_OK) return rc;
    const ck_rig_robust_params_t *rp = use_robust ? robust_params : nullptr;
    if ((rc = ck_rig_enqueue_last(handles, n_cams, n, &robust_params->rig, rp, gyro, has_gyro, start_out, meas, valid)) != CK_OK) return rc;
    ck_handle *h = handles[0];
    ck_rig_ws *rig = h->rig; // (ck_rig_enqueue_last made it)
    // From here on copies into the caller's start_out, meas and valid are in flight: no return without the wait for the stream.
    rc = refined_enqueue(handles, n_cams, n, rp, refine_params, rig, out, meas);
    if (hipStreamSynchronize(h->stream) != hipSuccess && rc == CK_OK) { (void)hipGetLastError(); rc = CK_EDEVICE; }
    return rc;
}

extern "C" int ck_rig_refine_time(ck_handle_t *h, const ck_rig_refine_params_t *params, int32_t n_cams, const ck_sqpnp_problem_t *problems,
                                  int32_t n, const ck_iso3_t *tags, int32_t n_tags_total, const double *bearings, int32_t n_bearings_total,
                                  const double *gyro, int32_t iters, float *ms_refine, float *ms_rig) {
    if (!h || iters < 1 || !ms_refine || !ms_rig || n < 1 || !gyro) return CK_EINVAL;
    ck_rig_params_t rig;
    ck_rig_params_default(&rig);
    std::vector<ck_rig_result_t> start((size_t)n);
    std::vector<ck_rig_refined_t> out((size_t)n);
    int rc = ck_rig_solve_batch(h, &rig, n_cams, problems, n, tags, n_tags_total, bearings, n_bearings_total, gyro, start.data());
    if (rc != CK_OK) return rc;
    staged_t keep;
    ck_rig_refine_args a;
    rc = refine_enqueue(h, params, n_cams, problems, n, tags, n_tags_total, bearings, n_bearings_total, gyro, start.data(), nullptr, out.data(), keep, a);
    if (rc != CK_OK) { (void)hipStreamSynchronize(h->stream); return rc; }
    CK_HIP(hipStreamSynchronize(h->stream));
    hipEvent_t e0, e1;
    CK_HIP_ALLOC(hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); (void)hipGetLastError(); return CK_ENOMEM; }
    for (int it = 0; it < iters && rc == CK_OK; it++) {
        float *dst[2] = {ms_refine + it, ms_rig + it};
        for (int which = 0; which < 2 && rc == CK_OK; which++) {
            if (hipEventRecord(e0, h->stream) != hipSuccess) { rc = CK_EDEVICE; break; }
            rc = which == 0 ? ck_launch_rig_refine(h->stream, a) : ck_rig_relaunch_batch(h, &rig, n_cams, n, keep.max_points);
            if (rc != CK_OK) break;
            if (hipEventRecord(e1, h->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
                hipEventElapsedTime(dst[which], e0, e1) != hipSuccess) rc = CK_EDEVICE;
        }
    }
    (void)hipStreamSynchronize(h->stream);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (rc == CK_EDEVICE) (void)hipGetLastError();
    return rc;
}
