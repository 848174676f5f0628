// Mount calibration: the host half that drives the device.  Validates a call (ck_rigcal_check, before any device is
// touched), decides per problem what ck_rigcal_host.c decides for the twin (used steps and views, gauge, connectivity), grows the workspace,
// copies the capture and the starts over, runs k_rigcal on the handle's stream and brings results, mounts and poses back.
#include <string.h>

#include <vector>

#include "ck_cal.h"
#include "ck_rigcal.h"
#include "ck_rigcal_math.h"

static_assert(sizeof(ck_rigcal_params_t) == 24, "ck_rigcal_params_t layout");
static_assert(sizeof(ck_rigcal_problem_t) == 8, "ck_rigcal_problem_t layout");
static_assert(sizeof(ck_rigcal_result_t) == 592, "ck_rigcal_result_t layout");
static_assert(sizeof(ck_rigcal_dev_problem) == 32, "ck_rigcal_dev_problem layout");
static_assert(CKA_B_WG + 6 <= CKA_B_STRIDE && CKA_S_COST < CKA_S_STRIDE, "record layouts");

extern "C" int ck_rigcal_refine_batch(ck_handle_t *h, const ck_rigcal_params_t *p, int32_t n_cams, const ck_sqpnp_problem_t *records,
                                      int32_t n_steps, const ck_iso3_t *tags, int32_t n_tags_total, const double *bearings,
                                      int32_t n_bearings_total, const ck_rigcal_problem_t *problems, int32_t n, const int32_t *step_index,
                                      int32_t n_index_total, const ck_iso3_t *mounts0, const double *poses0, ck_rigcal_result_t *results,
                                      double *poses_out) {
    if (!h || !poses0 || !results || !poses_out) return CK_EINVAL;
    int rc = ck_rigcal_check(p, n_cams, records, n_steps, tags, n_tags_total, bearings, n_bearings_total, problems, n, step_index,
                             n_index_total, mounts0);
    if (rc != CK_OK || n == 0) return rc;
    std::vector<int32_t> tab, index;
    std::vector<double> world, mounts, steps;
    std::vector<ck_rigcal_plan_t> plans;
    std::vector<ck_rigcal_dev_problem> dprob;
    size_t n_used = 0, n_views = 0, n_index = 0;
    try {
        tab.resize(CKR_TAB * (size_t)n_cams * (size_t)n_steps + 1);
        world.resize(12 * (size_t)n_tags_total + 1);
        plans.resize((size_t)n);
        dprob.resize((size_t)n);
        mounts.assign((size_t)12 * CK_RIG_MAX_CAMS * (size_t)n, 0.0);
        ck_rigcal_table(n_cams, records, n_steps, tags, n_tags_total, tab.data(), world.data());
        for (int32_t i = 0; i < n; i++) {
            const ck_rigcal_problem_t &q = problems[i];
            // (problems may share a run of step_index: every problem gets an index of its own)
            index.resize(n_index + cka_index_size((size_t)q.n_steps, (size_t)n_cams * (size_t)q.n_steps, (size_t)n_cams) + 1);
            ck_rigcal_plan(p, n_cams, tab.data(), n_steps, &q, step_index, poses0, index.data() + n_index, &plans[i]);
            ck_rigcal_result_start(&q, &plans[i], n_cams, mounts0, &results[i]);
            ck_cal_poses_start(&q, step_index, poses0, poses_out);
            for (int c = 0; c < n_cams; c++) ck_rigcal_mount_in(mounts0 + c, mounts.data() + 12 * ((size_t)CK_RIG_MAX_CAMS * i + c));
            ck_rigcal_dev_problem &d = dprob[i];
            d.index_off = (int64_t)n_index; d.step_off = (int32_t)n_used; d.view_off = (int32_t)n_views;
            d.n_used = d.n_views = 0;
            d.mask = plans[i].mask;
            if (plans[i].status == CK_CALIB_DEGENERATE) continue;
            d.n_used = plans[i].n_used; d.n_views = plans[i].n_views;
            n_index += cka_index_size((size_t)d.n_used, (size_t)d.n_views, (size_t)n_cams);
            n_used += (size_t)d.n_used; n_views += (size_t)d.n_views;
            if (n_used * (size_t)n_cams >= ((size_t)1 << 31) / CKA_B_STRIDE) return CK_ECAPACITY;
        }
        index.resize(n_index + 1);
        steps.assign((size_t)CKA_S_STRIDE * (n_used + 1), 0.0);
        for (int32_t i = 0; i < n; i++)
            ck_cal_steps_seed(steps.data() + (size_t)CKA_S_STRIDE * (size_t)dprob[i].step_off, index.data() + dprob[i].index_off, dprob[i].n_used, poses0);
    } catch (...) {
        return CK_ENOMEM;
    }
    CK_HIP(hipSetDevice(h->device));
    if (!ck_workspace(h->rigcal)) return CK_ENOMEM;
    ck_rigcal_ws &W = *h->rigcal;
    const size_t mount_bytes = sizeof(double) * mounts.size(), step_bytes = sizeof(double) * steps.size();
    const size_t res_bytes = sizeof(ck_rigcal_result_t) * (size_t)n;
    rc = ck_upload(W.d_prob, dprob.data(), sizeof(ck_rigcal_dev_problem) * (size_t)n, h->stream);
    if (rc == CK_OK) rc = ck_upload(W.d_tab, tab.data(), sizeof(int32_t) * CKR_TAB * (size_t)n_cams * (size_t)n_steps, h->stream, 4);
    if (rc == CK_OK) rc = ck_upload(W.d_index, index.data(), sizeof(int32_t) * index.size(), h->stream);
    if (rc == CK_OK) rc = ck_upload(W.d_world, world.data(), sizeof(double) * 12 * (size_t)n_tags_total, h->stream, 8);
    if (rc == CK_OK) rc = ck_upload(W.d_bear, bearings, sizeof(double) * 3 * (size_t)n_bearings_total, h->stream, 8);
    if (rc == CK_OK) rc = ck_upload(W.d_mounts, mounts.data(), mount_bytes, h->stream);
    if (rc == CK_OK) rc = ck_upload(W.d_steps, steps.data(), step_bytes, h->stream);
    if (rc == CK_OK) rc = W.d_views.reserve(sizeof(double) * CKA_B_STRIDE * (n_views + 1));
    if (rc == CK_OK) rc = ck_upload(W.d_res, results, res_bytes, h->stream);
    if (rc != CK_OK) return rc;
    rc = ck_launch_rigcal(h->stream, p->max_iters, n_cams, n_steps, W.d_prob, n, W.d_tab, W.d_index, W.d_world, W.d_bear, W.d_mounts, W.d_steps,
                          W.d_views, W.d_res);
    if (rc != CK_OK) return rc;
    CK_HIP(hipMemcpyAsync(results, W.d_res, res_bytes, hipMemcpyDeviceToHost, h->stream));
    CK_HIP(hipMemcpyAsync(mounts.data(), W.d_mounts, mount_bytes, hipMemcpyDeviceToHost, h->stream));
    CK_HIP(hipMemcpyAsync(steps.data(), W.d_steps, step_bytes, hipMemcpyDeviceToHost, h->stream));
    CK_HIP(hipStreamSynchronize(h->stream));
    for (int32_t i = 0; i < n; i++) {
        if (results[i].status == CK_CALIB_DEGENERATE) continue;
        ck_rigcal_result_finish(&plans[i], n_cams, mounts0, mounts.data() + (size_t)12 * CK_RIG_MAX_CAMS * i, &results[i]);
        ck_cal_poses_finish(&problems[i], step_index, index.data() + dprob[i].index_off, dprob[i].n_used,
                            steps.data() + (size_t)CKA_S_STRIDE * (size_t)dprob[i].step_off, poses_out);
    }
    return CK_OK;
}

int ck_cal_starts_solve(ck_handle_t *h, int32_t n_cams, const ck_sqpnp_problem_t *records, int32_t n_steps, const ck_iso3_t *tags,
                        int32_t n_tags_total, const double *bearings, int32_t n_bearings_total, const double *gyro,
                        const ck_rigcal_problem_t *problems, int32_t n, const int32_t *step_index, const ck_iso3_t *mounts, ck_cal_starts &s) {
    std::vector<ck_sqpnp_problem_t> rec;
    std::vector<ck_rig_result_t> rig;
    try {
        rec.assign(records, records + (size_t)n_cams * (size_t)n_steps);
        rig.resize((size_t)n_steps + 1);
        s.poses0.assign(12 * ((size_t)n_steps + 1), 0.0);
        s.prob.resize((size_t)n);
    } catch (...) {
        return CK_ENOMEM;
    }
    for (int c = 0; c < n_cams; c++)
        for (int32_t t = 0; t < n_steps; t++) rec[(size_t)c * n_steps + t].robot_to_cam = mounts[c];
    ck_rig_params_t rp;
    ck_rig_params_default(&rp);
    rp.sign_change_error = 0.0;
    const int rc = ck_rig_solve_batch(h, &rp, n_cams, rec.data(), n_steps, tags, n_tags_total, bearings, n_bearings_total, gyro, rig.data());
    if (rc != CK_OK) return rc;
    for (int32_t t = 0; t < n_steps; t++) { // world -> robot = (rot^T, -rot^T pos)
        const ck_rig_result_t &r = rig[t];
        double *P = s.poses0.data() + 12 * (size_t)t;
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) P[3 * i + j] = r.rot[3 * j + i];
            P[9 + i] = -(r.rot[i] * r.pos[0] + r.rot[3 + i] * r.pos[1] + r.rot[6 + i] * r.pos[2]);
        }
    }
    try {
        for (int32_t i = 0; i < n; i++) {
            s.prob[i].step_offset = (int32_t)s.index.size();
            for (int32_t j = 0; j < problems[i].n_steps; j++) {
                const int32_t t = step_index[problems[i].step_offset + j];
                if (!rig[t].valid) continue;
                s.index.push_back(t);
                s.where.push_back(problems[i].step_offset + j);
            }
            s.prob[i].n_steps = (int32_t)s.index.size() - s.prob[i].step_offset;
        }
        s.index.push_back(0);
        s.poses.assign(12 * (s.where.size() + 1), 0.0); // every problem has a run of its own here, also where the caller's problems share one
    } catch (...) {
        return CK_ENOMEM;
    }
    return CK_OK;
}

extern "C" int ck_rig_calibrate_batch(ck_handle_t *h, const ck_rigcal_params_t *p, int32_t n_cams, const ck_sqpnp_problem_t *records,
                                      int32_t n_steps, const ck_iso3_t *tags, int32_t n_tags_total, const double *bearings,
                                      int32_t n_bearings_total, const double *gyro, const ck_rigcal_problem_t *problems, int32_t n,
                                      const int32_t *step_index, int32_t n_index_total, const ck_iso3_t *mounts0, ck_rigcal_result_t *results,
                                      double *poses_out) {
    if (!h || !gyro || !results || !poses_out) return CK_EINVAL;
    int rc = ck_rigcal_check(p, n_cams, records, n_steps, tags, n_tags_total, bearings, n_bearings_total, problems, n, step_index,
                             n_index_total, mounts0);
    if (rc != CK_OK || n == 0) return rc;
    ck_cal_starts s;
    rc = ck_cal_starts_solve(h, n_cams, records, n_steps, tags, n_tags_total, bearings, n_bearings_total, gyro, problems, n, step_index, mounts0, s);
    if (rc != CK_OK) return rc;
    rc = ck_rigcal_refine_batch(h, p, n_cams, records, n_steps, tags, n_tags_total, bearings, n_bearings_total, s.prob.data(), n, s.index.data(),
                                s.n_index(), mounts0, s.poses0.data(), results, s.poses.data());
    if (rc != CK_OK) return rc;
    ck_cal_starts_finish(s, problems, n, results, poses_out);
    return CK_OK;
}

extern "C" int ck_last_pose_inputs(ck_handle_t *h, int32_t n, ck_sqpnp_problem_t *records_out, ck_iso3_t *tags_out, int32_t tag_cap,
                                   double *bearings_out, int32_t bearing_cap, int32_t *n_tags_out, int32_t *n_bearings_out) {
    if (!h || !records_out || !tags_out || !bearings_out || !n_tags_out || !n_bearings_out || n < 1 || tag_cap < 0 || bearing_cap < 0) return CK_EINVAL;
    if (h->n_last_pose != n || h->n_pose_inputs != n) return CK_EINVAL; // the test ck_rig_process_last makes
    const ck_stage_ws &w = h->ws;
    const size_t cap = (size_t)w.det_cap;
    std::vector<ck_iso3_t> tags;
    std::vector<double> bear;
    try {
        tags.resize((size_t)n * cap);
        bear.resize((size_t)n * cap * 12);
    } catch (...) {
        return CK_ENOMEM;
    }
    CK_HIP(hipSetDevice(h->device));
    CK_HIP(hipMemcpyAsync(records_out, w.d_problems, sizeof(ck_sqpnp_problem_t) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    CK_HIP(hipMemcpyAsync(tags.data(), w.d_pose_tags, sizeof(ck_iso3_t) * tags.size(), hipMemcpyDeviceToHost, h->stream));
    CK_HIP(hipMemcpyAsync(bear.data(), w.d_bearings, sizeof(double) * bear.size(), hipMemcpyDeviceToHost, h->stream));
    CK_HIP(hipStreamSynchronize(h->stream));
    // Step s owns tags [s * det_cap ..] and bearings [s * det_cap * 4 ..] of the workspace (its record's offsets say the same); the
    // outputs are packed in step order, and the records' offsets rewritten to match
    int64_t nt = 0;
    for (int32_t s = 0; s < n; s++) nt += records_out[s].n_tags > 0 && (size_t)records_out[s].n_tags <= cap ? records_out[s].n_tags : 0;
    *n_tags_out = (int32_t)nt; *n_bearings_out = (int32_t)(4 * nt);
    if (nt > tag_cap || 4 * nt > bearing_cap) return CK_ECAPACITY;
    nt = 0;
    for (int32_t s = 0; s < n; s++) {
        ck_sqpnp_problem_t &r = records_out[s];
        if (r.n_tags < 0 || (size_t)r.n_tags > cap) r.n_tags = 0;
        r.n_bearings = 4 * r.n_tags;
        memcpy(tags_out + nt, tags.data() + (size_t)s * cap, sizeof(ck_iso3_t) * (size_t)r.n_tags);
        memcpy(bearings_out + 12 * nt, bear.data() + (size_t)s * cap * 12, sizeof(double) * 12 * (size_t)r.n_tags);
        r.tag_offset = (int32_t)nt; r.bearing_offset = (int32_t)(4 * nt);
        nt += r.n_tags;
    }
    return CK_OK;
}
