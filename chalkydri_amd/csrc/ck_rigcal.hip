// Mount calibration: the host half that drives the device.  Validates a call (ck_rigcal_check, before any device is
// touched), decides per problem what ck_rigcal_host.c decides for the twin (used steps, gauge, connectivity), grows the workspace,
// copies the capture and the starts over, runs k_rigcal on the handle's stream and brings results, mounts and poses back.
#include <string.h>

#include <vector>

#include "ck_rigcal.h"
#include "ck_rigcal_math.h"

static_assert(sizeof(ck_rigcal_params_t) == 24, "ck_rigcal_params_t layout");
static_assert(sizeof(ck_rigcal_problem_t) == 8, "ck_rigcal_problem_t layout");
static_assert(sizeof(ck_rigcal_result_t) == 592, "ck_rigcal_result_t layout");
static_assert(sizeof(ck_rigcal_dev_problem) == 16, "ck_rigcal_dev_problem layout");
static_assert(CKR_V_WG + 6 <= CKR_V_STRIDE && CKR_S_COST < CKR_S_STRIDE, "record layouts");

extern "C" int ck_rigcal_refine_batch(ck_handle_t *h, const ck_rigcal_params_t *p, int32_t n_cams, const ck_sqpnp_problem_t *records,
                                      int32_t n_steps, const ck_iso3_t *tags, int32_t n_tags_total, const double *bearings,
                                      int32_t n_bearings_total, const ck_rigcal_problem_t *problems, int32_t n, const int32_t *step_index,
                                      int32_t n_index_total, const ck_iso3_t *mounts0, const double *poses0, ck_rigcal_result_t *results,
                                      double *poses_out) {
    if (!h || !poses0 || !results || !poses_out) return CK_EINVAL;
    int rc = ck_rigcal_check(p, n_cams, records, n_steps, tags, n_tags_total, bearings, n_bearings_total, problems, n, step_index,
                             n_index_total, mounts0);
    if (rc != CK_OK || n == 0) return rc;
    std::vector<int32_t> tab, used;
    std::vector<double> world, mounts, steps;
    std::vector<ck_rigcal_plan_t> plans;
    std::vector<ck_rigcal_dev_problem> dprob;
    size_t n_used = 0;
    try {
        tab.resize(CKR_TAB * (size_t)n_cams * (size_t)n_steps + 1);
        world.resize(12 * (size_t)n_tags_total + 1);
        used.resize((size_t)n_index_total + 1);
        plans.resize((size_t)n);
        dprob.resize((size_t)n);
        mounts.assign((size_t)12 * CK_RIG_MAX_CAMS * (size_t)n, 0.0);
        ck_rigcal_table(n_cams, records, n_steps, tags, n_tags_total, tab.data(), world.data());
        for (int32_t i = 0; i < n; i++) {
            const ck_rigcal_problem_t &q = problems[i];
            // (problems may share a run of step_index: every problem gets its own run of used steps)
            if (n_used + (size_t)q.n_steps + 1 > used.size()) used.resize(n_used + (size_t)q.n_steps + 1);
            ck_rigcal_plan(p, n_cams, tab.data(), n_steps, &q, step_index, poses0, used.data() + n_used, &plans[i]);
            ck_rigcal_result_start(&q, &plans[i], n_cams, mounts0, &results[i]);
            for (int32_t j = 0; j < q.n_steps; j++)
                memcpy(poses_out + 12 * ((size_t)q.step_offset + j), poses0 + 12 * (size_t)step_index[q.step_offset + j], sizeof(double) * 12);
            for (int c = 0; c < n_cams; c++) ck_rigcal_mount_in(mounts0 + c, mounts.data() + 12 * ((size_t)CK_RIG_MAX_CAMS * i + c));
            dprob[i].used_off = (int32_t)n_used;
            dprob[i].n_used = plans[i].status == CK_CALIB_DEGENERATE ? 0 : plans[i].n_used;
            dprob[i].mask = plans[i].mask;
            n_used += (size_t)dprob[i].n_used;
            if (n_used * (size_t)n_cams >= ((size_t)1 << 31) / CKR_V_STRIDE) return CK_ECAPACITY;
        }
        steps.assign((size_t)CKR_S_STRIDE * (n_used + 1), 0.0);
        for (int32_t i = 0; i < n; i++)
            for (int32_t u = 0; u < dprob[i].n_used; u++) {
                double *st = steps.data() + (size_t)CKR_S_STRIDE * ((size_t)dprob[i].used_off + u);
                memcpy(st + CKR_S_POSE, poses0 + 12 * (size_t)used[(size_t)dprob[i].used_off + u], sizeof(double) * 12);
                memcpy(st + CKR_S_CAND, st + CKR_S_POSE, sizeof(double) * 12);
            }
    } catch (...) {
        return CK_ENOMEM;
    }
    CK_HIP(hipSetDevice(h->device));
    if (!ck_workspace(h->rigcal)) return CK_ENOMEM;
    ck_rigcal_ws &W = *h->rigcal;
    const size_t tab_bytes = sizeof(int32_t) * CKR_TAB * (size_t)n_cams * (size_t)n_steps, used_bytes = sizeof(int32_t) * (n_used + 1);
    const size_t world_bytes = sizeof(double) * 12 * (size_t)n_tags_total, bear_bytes = sizeof(double) * 3 * (size_t)n_bearings_total;
    const size_t mount_bytes = sizeof(double) * mounts.size(), step_bytes = sizeof(double) * CKR_S_STRIDE * (n_used + 1);
    rc = W.d_prob.reserve(sizeof(ck_rigcal_dev_problem) * (size_t)n);
    if (rc == CK_OK) rc = W.d_tab.reserve(tab_bytes + 4);
    if (rc == CK_OK) rc = W.d_used.reserve(used_bytes);
    if (rc == CK_OK) rc = W.d_world.reserve(world_bytes + 8);
    if (rc == CK_OK) rc = W.d_bear.reserve(bear_bytes + 8);
    if (rc == CK_OK) rc = W.d_mounts.reserve(mount_bytes);
    if (rc == CK_OK) rc = W.d_steps.reserve(step_bytes);
    if (rc == CK_OK) rc = W.d_views.reserve(sizeof(double) * CKR_V_STRIDE * (n_used * (size_t)n_cams + 1));
    if (rc == CK_OK) rc = W.d_res.reserve(sizeof(ck_rigcal_result_t) * (size_t)n);
    if (rc != CK_OK) return rc;
    CK_HIP(hipMemcpyAsync(W.d_prob, dprob.data(), sizeof(ck_rigcal_dev_problem) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    if (tab_bytes) CK_HIP(hipMemcpyAsync(W.d_tab, tab.data(), tab_bytes, hipMemcpyHostToDevice, h->stream));
    CK_HIP(hipMemcpyAsync(W.d_used, used.data(), used_bytes, hipMemcpyHostToDevice, h->stream));
    if (world_bytes) CK_HIP(hipMemcpyAsync(W.d_world, world.data(), world_bytes, hipMemcpyHostToDevice, h->stream));
    if (bear_bytes) CK_HIP(hipMemcpyAsync(W.d_bear, bearings, bear_bytes, hipMemcpyHostToDevice, h->stream));
    CK_HIP(hipMemcpyAsync(W.d_mounts, mounts.data(), mount_bytes, hipMemcpyHostToDevice, h->stream));
    CK_HIP(hipMemcpyAsync(W.d_steps, steps.data(), step_bytes, hipMemcpyHostToDevice, h->stream));
    CK_HIP(hipMemcpyAsync(W.d_res, results, sizeof(ck_rigcal_result_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    rc = ck_launch_rigcal(h->stream, p->max_iters, n_cams, n_steps, W.d_prob, n, W.d_tab, W.d_used, W.d_world, W.d_bear, W.d_mounts, W.d_steps,
                          W.d_views, W.d_res);
    if (rc != CK_OK) return rc;
    CK_HIP(hipMemcpyAsync(results, W.d_res, sizeof(ck_rigcal_result_t) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    CK_HIP(hipMemcpyAsync(mounts.data(), W.d_mounts, mount_bytes, hipMemcpyDeviceToHost, h->stream));
    CK_HIP(hipMemcpyAsync(steps.data(), W.d_steps, step_bytes, hipMemcpyDeviceToHost, h->stream));
    CK_HIP(hipStreamSynchronize(h->stream));
    for (int32_t i = 0; i < n; i++) {
        if (results[i].status == CK_CALIB_DEGENERATE) continue;
        const ck_rigcal_problem_t &q = problems[i];
        ck_rigcal_result_finish(&plans[i], n_cams, mounts0, mounts.data() + (size_t)12 * CK_RIG_MAX_CAMS * i, &results[i]);
        for (int32_t u = 0, j = 0; u < dprob[i].n_used; u++) {
            const size_t at = (size_t)dprob[i].used_off + u;
            while (step_index[q.step_offset + j] != used[at]) j++;
            memcpy(poses_out + 12 * ((size_t)q.step_offset + j), steps.data() + (size_t)CKR_S_STRIDE * at + CKR_S_POSE, sizeof(double) * 12);
        }
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
    std::vector<ck_sqpnp_problem_t> rec;
    std::vector<ck_rig_result_t> rig;
    std::vector<ck_rigcal_problem_t> prob2;
    std::vector<int32_t> index2, where;
    std::vector<double> poses0, poses2;
    try {
        rec.assign(records, records + (size_t)n_cams * (size_t)n_steps);
        rig.resize((size_t)n_steps + 1);
        poses0.assign(12 * ((size_t)n_steps + 1), 0.0);
        prob2.resize((size_t)n);
    } catch (...) {
        return CK_ENOMEM;
    }
    // the starts: the rig solver with the start mounts and no gyro penalty over the whole capture, once
    for (int c = 0; c < n_cams; c++)
        for (int32_t s = 0; s < n_steps; s++) rec[(size_t)c * n_steps + s].robot_to_cam = mounts0[c];
    ck_rig_params_t rp;
    ck_rig_params_default(&rp);
    rp.sign_change_error = 0.0;
    rc = ck_rig_solve_batch(h, &rp, n_cams, rec.data(), n_steps, tags, n_tags_total, bearings, n_bearings_total, gyro, rig.data());
    if (rc != CK_OK) return rc;
    for (int32_t s = 0; s < n_steps; s++) { // world -> robot = (rot^T, -rot^T pos)
        const ck_rig_result_t &r = rig[s];
        double *P = poses0.data() + 12 * (size_t)s;
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) P[3 * i + j] = r.rot[3 * j + i];
            P[9 + i] = -(r.rot[i] * r.pos[0] + r.rot[3 + i] * r.pos[1] + r.rot[6 + i] * r.pos[2]);
        }
    }
    // a step without a start is left out of every problem
    try {
        for (int32_t i = 0; i < n; i++) {
            prob2[i].step_offset = (int32_t)index2.size();
            for (int32_t j = 0; j < problems[i].n_steps; j++) {
                const int32_t s = step_index[problems[i].step_offset + j];
                if (!rig[s].valid) continue;
                index2.push_back(s);
                where.push_back(problems[i].step_offset + j);
            }
            prob2[i].n_steps = (int32_t)index2.size() - prob2[i].step_offset;
        }
        index2.push_back(0);
        poses2.assign(12 * (where.size() + 1), 0.0); // every problem has a run of its own here, also where the caller's problems share one
    } catch (...) {
        return CK_ENOMEM;
    }
    rc = ck_rigcal_refine_batch(h, p, n_cams, records, n_steps, tags, n_tags_total, bearings, n_bearings_total, prob2.data(), n, index2.data(),
                                (int32_t)where.size(), mounts0, poses0.data(), results, poses2.data());
    if (rc != CK_OK) return rc;
    for (int32_t i = 0; i < n; i++) {
        results[i].n_steps = problems[i].n_steps;
        memset(poses_out + 12 * (size_t)problems[i].step_offset, 0, sizeof(double) * 12 * (size_t)problems[i].n_steps);
    }
    for (size_t k = 0; k < where.size(); k++) memcpy(poses_out + 12 * (size_t)where[k], poses2.data() + 12 * k, sizeof(double) * 12);
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
    // Step s owns tags [s * det_cap ..] and bearings [s * det_cap * 4 ..] of the workspace whichever piece of a split batch wrote its
    // record (the record's own offsets are relative to that piece): the outputs are packed in step order
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
