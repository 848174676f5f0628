// Field calibration: the host half that drives the device.  Validates a call (ck_fieldcal_check, before any device is
// touched), decides per problem what ck_fieldcal_host.c decides for the twin (used steps, tags, sightings, gauge, connectivity), grows
// the workspace, copies the tables, the bearings and the starts over, runs k_fieldcal on the handle's stream and brings results, tags
// and poses back.
#include <string.h>

#include <vector>

#include "ck_fieldcal.h"
#include "ck_fieldcal_math.h"
#include "ck_rigcal_c.h"

static_assert(sizeof(ck_fieldcal_params_t) == 16, "ck_fieldcal_params_t layout");
static_assert(sizeof(ck_fieldcal_result_t) == 48, "ck_fieldcal_result_t layout");
static_assert(sizeof(ck_fieldcal_dev_problem) == 56, "ck_fieldcal_dev_problem layout");
static_assert(CKF_I_COST < CKF_I_STRIDE && CKF_P_COSTA < CKF_P_STRIDE, "record layouts");

namespace {
struct plans_t { // the plans of a call, released with it
    std::vector<ck_fieldcal_plan_t> v;
    ~plans_t() { for (auto &p : v) ck_fieldcal_plan_free(&p); }
};
} // namespace

extern "C" int ck_fieldcal_refine_batch(ck_handle_t *h, const ck_fieldcal_params_t *p, int32_t n_cams, const ck_sqpnp_problem_t *records,
                                        int32_t n_steps, const int32_t *tag_index, int32_t n_tags_total, const double *bearings,
                                        int32_t n_bearings_total, const ck_rigcal_problem_t *problems, int32_t n, const int32_t *step_index,
                                        int32_t n_index_total, const ck_iso3_t *mounts, const ck_iso3_t *layout0, int32_t n_layout,
                                        const uint8_t *fixed6, const double *poses0, ck_fieldcal_result_t *results, ck_iso3_t *layout_out,
                                        int32_t *tag_sightings, double *tag_rms, double *poses_out) {
    if (!h || !poses0 || !results || !layout_out || !tag_sightings || !tag_rms || !poses_out) return CK_EINVAL;
    int rc = ck_fieldcal_check(p, n_cams, records, n_steps, tag_index, n_tags_total, bearings, n_bearings_total, problems, n, step_index,
                               n_index_total, mounts, layout0, n_layout, fixed6);
    if (rc != CK_OK || n == 0) return rc;
    plans_t plans;
    std::vector<ck_fieldcal_dev_problem> dprob;
    std::vector<int32_t> meta;
    std::vector<double> M, tags, rms, steps;
    size_t n_used = 0, n_pairs = 0, n_sights = 0, n_S = 0;
    try {
        plans.v.resize((size_t)n);
        for (auto &pl : plans.v) memset(&pl, 0, sizeof pl);
        dprob.resize((size_t)n);
        M.assign((size_t)12 * CK_RIG_MAX_CAMS, 0.0);
        tags.assign((size_t)12 * CK_FIELDCAL_MAX_TAGS * (size_t)n, 0.0);
        rms.assign((size_t)CK_FIELDCAL_MAX_TAGS * (size_t)n, 0.0);
        for (int c = 0; c < n_cams; c++) ck_rigcal_mount_in(mounts + c, M.data() + 12 * c);
        for (int32_t i = 0; i < n; i++) {
            const ck_rigcal_problem_t &q = problems[i];
            ck_fieldcal_plan_t &pl = plans.v[i];
            rc = ck_fieldcal_plan(p, n_cams, records, n_steps, tag_index, &q, step_index, n_layout, fixed6, poses0,
                                  tag_sightings + (size_t)n_layout * i, &pl);
            if (rc != CK_OK) return rc;
            ck_fieldcal_result_start(&q, &pl, layout0, n_layout, &results[i], layout_out + (size_t)n_layout * i, tag_rms + (size_t)n_layout * i);
            for (int32_t j = 0; j < q.n_steps; j++)
                memcpy(poses_out + 12 * ((size_t)q.step_offset + j), poses0 + 12 * (size_t)step_index[q.step_offset + j], sizeof(double) * 12);
            ck_fieldcal_dev_problem &d = dprob[i];
            d.meta_off = (int64_t)meta.size();
            d.step_off = (int64_t)n_used; d.pair_off = (int64_t)n_pairs; d.sight_off = (int64_t)n_sights; d.s_off = (int64_t)n_S;
            d.U = d.P = d.NS = d.T = 0;
            if (pl.status == CK_CALIB_DEGENERATE) continue;
            d.U = pl.n_used; d.P = pl.n_pairs; d.NS = pl.n_sights; d.T = pl.n_tags;
            meta.insert(meta.end(), pl.meta, pl.meta + pl.n_meta);
            const ckf_meta_t m = ckf_meta_at(pl.meta, (size_t)d.U, (size_t)d.P, (size_t)d.NS, (size_t)d.T);
            for (int k = 0; k < d.T; k++) ck_fieldcal_tag_in(layout0 + m.ltag[k], tags.data() + 12 * ((size_t)CK_FIELDCAL_MAX_TAGS * i + k));
            n_used += (size_t)d.U; n_pairs += (size_t)d.P; n_sights += (size_t)d.NS;
            n_S += CKF_LT(6 * (size_t)d.T, 0);
            if (n_sights >= ((size_t)1 << 31) / CKF_I_STRIDE || n_pairs >= ((size_t)1 << 31) / CKF_P_STRIDE || n_S >= ((size_t)1 << 31)) return CK_ECAPACITY;
        }
        meta.push_back(0);
        steps.assign((size_t)CKR_S_STRIDE * (n_used + 1), 0.0);
        for (int32_t i = 0; i < n; i++) {
            const ckf_meta_t m = ckf_meta_at(meta.data() + dprob[i].meta_off, (size_t)dprob[i].U, (size_t)dprob[i].P, (size_t)dprob[i].NS, (size_t)dprob[i].T);
            for (int32_t u = 0; u < dprob[i].U; u++) {
                double *st = steps.data() + (size_t)CKR_S_STRIDE * ((size_t)dprob[i].step_off + u);
                memcpy(st + CKR_S_POSE, poses0 + 12 * (size_t)m.used[u], sizeof(double) * 12);
                memcpy(st + CKR_S_CAND, st + CKR_S_POSE, sizeof(double) * 12);
            }
        }
    } catch (...) {
        return CK_ENOMEM;
    }
    CK_HIP(hipSetDevice(h->device));
    if (!ck_workspace(h->fieldcal)) return CK_ENOMEM;
    ck_fieldcal_ws &W = *h->fieldcal;
    const size_t prob_bytes = sizeof(ck_fieldcal_dev_problem) * (size_t)n, meta_bytes = sizeof(int32_t) * meta.size();
    const size_t bear_bytes = sizeof(double) * 3 * (size_t)n_bearings_total, mount_bytes = sizeof(double) * M.size();
    const size_t tag_bytes = sizeof(double) * tags.size(), rms_bytes = sizeof(double) * rms.size();
    const size_t step_bytes = sizeof(double) * steps.size(), res_bytes = sizeof(ck_fieldcal_result_t) * (size_t)n;
    rc = W.d_prob.reserve(prob_bytes);
    if (rc == CK_OK) rc = W.d_meta.reserve(meta_bytes);
    if (rc == CK_OK) rc = W.d_bear.reserve(bear_bytes + 8);
    if (rc == CK_OK) rc = W.d_mounts.reserve(mount_bytes);
    if (rc == CK_OK) rc = W.d_tags.reserve(tag_bytes);
    if (rc == CK_OK) rc = W.d_rms.reserve(rms_bytes);
    if (rc == CK_OK) rc = W.d_steps.reserve(step_bytes);
    if (rc == CK_OK) rc = W.d_pairs.reserve(sizeof(double) * CKF_P_STRIDE * (n_pairs + 1));
    if (rc == CK_OK) rc = W.d_sights.reserve(sizeof(double) * CKF_I_STRIDE * (n_sights + 1));
    if (rc == CK_OK) rc = W.d_S.reserve(sizeof(double) * (n_S + 1));
    if (rc == CK_OK) rc = W.d_res.reserve(res_bytes);
    if (rc != CK_OK) return rc;
    CK_HIP(hipMemcpyAsync(W.d_prob, dprob.data(), prob_bytes, hipMemcpyHostToDevice, h->stream));
    CK_HIP(hipMemcpyAsync(W.d_meta, meta.data(), meta_bytes, hipMemcpyHostToDevice, h->stream));
    if (bear_bytes) CK_HIP(hipMemcpyAsync(W.d_bear, bearings, bear_bytes, hipMemcpyHostToDevice, h->stream));
    CK_HIP(hipMemcpyAsync(W.d_mounts, M.data(), mount_bytes, hipMemcpyHostToDevice, h->stream));
    CK_HIP(hipMemcpyAsync(W.d_tags, tags.data(), tag_bytes, hipMemcpyHostToDevice, h->stream));
    CK_HIP(hipMemsetAsync(W.d_rms, 0, rms_bytes, h->stream));
    CK_HIP(hipMemcpyAsync(W.d_steps, steps.data(), step_bytes, hipMemcpyHostToDevice, h->stream));
    CK_HIP(hipMemcpyAsync(W.d_res, results, res_bytes, hipMemcpyHostToDevice, h->stream));
    rc = ck_launch_fieldcal(h->stream, p->max_iters, n_cams, W.d_prob, n, W.d_meta, W.d_bear, W.d_mounts, W.d_tags, W.d_rms, W.d_steps, W.d_pairs,
                            W.d_sights, W.d_S, W.d_res);
    if (rc != CK_OK) return rc;
    CK_HIP(hipMemcpyAsync(results, W.d_res, res_bytes, hipMemcpyDeviceToHost, h->stream));
    CK_HIP(hipMemcpyAsync(tags.data(), W.d_tags, tag_bytes, hipMemcpyDeviceToHost, h->stream));
    CK_HIP(hipMemcpyAsync(rms.data(), W.d_rms, rms_bytes, hipMemcpyDeviceToHost, h->stream));
    CK_HIP(hipMemcpyAsync(steps.data(), W.d_steps, step_bytes, hipMemcpyDeviceToHost, h->stream));
    CK_HIP(hipStreamSynchronize(h->stream));
    for (int32_t i = 0; i < n; i++) {
        if (results[i].status == CK_CALIB_DEGENERATE) continue;
        const ck_rigcal_problem_t &q = problems[i];
        const ckf_meta_t m = ckf_meta_at(plans.v[i].meta, (size_t)dprob[i].U, (size_t)dprob[i].P, (size_t)dprob[i].NS, (size_t)dprob[i].T);
        ck_fieldcal_result_finish(&plans.v[i], layout0, tags.data() + (size_t)12 * CK_FIELDCAL_MAX_TAGS * i, rms.data() + (size_t)CK_FIELDCAL_MAX_TAGS * i,
                                  layout_out + (size_t)n_layout * i, tag_rms + (size_t)n_layout * i);
        for (int32_t u = 0, j = 0; u < dprob[i].U; u++) {
            while (step_index[q.step_offset + j] != m.used[u]) j++;
            memcpy(poses_out + 12 * ((size_t)q.step_offset + j), steps.data() + (size_t)CKR_S_STRIDE * ((size_t)dprob[i].step_off + u) + CKR_S_POSE,
                   sizeof(double) * 12);
        }
    }
    return CK_OK;
}

extern "C" int ck_field_calibrate_batch(ck_handle_t *h, const ck_fieldcal_params_t *p, int32_t n_cams, const ck_sqpnp_problem_t *records,
                                        int32_t n_steps, const int32_t *tag_index, int32_t n_tags_total, const double *bearings,
                                        int32_t n_bearings_total, const double *gyro, const ck_rigcal_problem_t *problems, int32_t n,
                                        const int32_t *step_index, int32_t n_index_total, const ck_iso3_t *mounts, const ck_iso3_t *layout0,
                                        int32_t n_layout, const uint8_t *fixed6, ck_fieldcal_result_t *results, ck_iso3_t *layout_out,
                                        int32_t *tag_sightings, double *tag_rms, double *poses_out) {
    if (!h || !gyro || !results || !layout_out || !tag_sightings || !tag_rms || !poses_out) return CK_EINVAL;
    int rc = ck_fieldcal_check(p, n_cams, records, n_steps, tag_index, n_tags_total, bearings, n_bearings_total, problems, n, step_index,
                               n_index_total, mounts, layout0, n_layout, fixed6);
    if (rc != CK_OK || n == 0) return rc;
    std::vector<ck_sqpnp_problem_t> rec;
    std::vector<ck_iso3_t> tags;
    std::vector<ck_rig_result_t> rig;
    std::vector<ck_rigcal_problem_t> prob2;
    std::vector<int32_t> index2, where;
    std::vector<double> poses0, poses2;
    try {
        rec.assign(records, records + (size_t)n_cams * (size_t)n_steps);
        tags.resize((size_t)n_tags_total + 1);
        rig.resize((size_t)n_steps + 1);
        poses0.assign(12 * ((size_t)n_steps + 1), 0.0);
        prob2.resize((size_t)n);
    } catch (...) {
        return CK_ENOMEM;
    }
    // the starts: the rig solver with the tags at layout0, the given mounts and no gyro penalty over the whole capture, once
    for (int32_t t = 0; t < n_tags_total; t++) tags[t] = layout0[tag_index[t]];
    for (int c = 0; c < n_cams; c++)
        for (int32_t s = 0; s < n_steps; s++) rec[(size_t)c * n_steps + s].robot_to_cam = mounts[c];
    ck_rig_params_t rp;
    ck_rig_params_default(&rp);
    rp.sign_change_error = 0.0;
    rc = ck_rig_solve_batch(h, &rp, n_cams, rec.data(), n_steps, tags.data(), n_tags_total, bearings, n_bearings_total, gyro, rig.data());
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
    rc = ck_fieldcal_refine_batch(h, p, n_cams, records, n_steps, tag_index, n_tags_total, bearings, n_bearings_total, prob2.data(), n,
                                  index2.data(), (int32_t)where.size(), mounts, layout0, n_layout, fixed6, poses0.data(), results, layout_out,
                                  tag_sightings, tag_rms, poses2.data());
    if (rc != CK_OK) return rc;
    for (int32_t i = 0; i < n; i++) {
        results[i].n_steps = problems[i].n_steps;
        memset(poses_out + 12 * (size_t)problems[i].step_offset, 0, sizeof(double) * 12 * (size_t)problems[i].n_steps);
    }
    for (size_t k = 0; k < where.size(); k++) memcpy(poses_out + 12 * (size_t)where[k], poses2.data() + 12 * k, sizeof(double) * 12);
    return CK_OK;
}
