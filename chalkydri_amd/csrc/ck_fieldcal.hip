// Field calibration: the host half that drives the device.  Validates a call (ck_fieldcal_check, before any device is
// touched), decides per problem what ck_fieldcal_host.c decides for the twin (used steps, tags, sightings, gauge, connectivity), grows
// the workspace, copies the tables, the bearings and the starts over, runs k_fieldcal on the handle's stream and brings results, tags
// and poses back.
#include <string.h>

#include <vector>

#include "ck_cal.h"
#include "ck_fieldcal.h"
#include "ck_fieldcal_math.h"
#include "ck_rigcal_c.h"

static_assert(sizeof(ck_fieldcal_params_t) == 16, "ck_fieldcal_params_t layout");
static_assert(sizeof(ck_fieldcal_result_t) == 48, "ck_fieldcal_result_t layout");
static_assert(sizeof(ck_fieldcal_dev_problem) == 56, "ck_fieldcal_dev_problem layout");
static_assert(CKF_I_COST < CKF_I_STRIDE && CKA_B_WG + 6 <= CKA_B_STRIDE, "record layouts");

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
            ck_cal_poses_start(&q, step_index, poses0, poses_out);
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
            if (n_sights >= ((size_t)1 << 31) / CKF_I_STRIDE || n_pairs >= ((size_t)1 << 31) / CKA_B_STRIDE || n_S >= ((size_t)1 << 31)) return CK_ECAPACITY;
        }
        meta.push_back(0);
        steps.assign((size_t)CKA_S_STRIDE * (n_used + 1), 0.0);
        for (int32_t i = 0; i < n; i++) // (a problem's tables start with its used steps)
            ck_cal_steps_seed(steps.data() + (size_t)CKA_S_STRIDE * (size_t)dprob[i].step_off, meta.data() + dprob[i].meta_off, dprob[i].U, poses0);
    } catch (...) {
        return CK_ENOMEM;
    }
    CK_HIP(hipSetDevice(h->device));
    if (!ck_workspace(h->fieldcal)) return CK_ENOMEM;
    ck_fieldcal_ws &W = *h->fieldcal;
    const size_t tag_bytes = sizeof(double) * tags.size(), rms_bytes = sizeof(double) * rms.size();
    const size_t step_bytes = sizeof(double) * steps.size(), res_bytes = sizeof(ck_fieldcal_result_t) * (size_t)n;
    rc = ck_upload(W.d_prob, dprob.data(), sizeof(ck_fieldcal_dev_problem) * (size_t)n, h->stream);
    if (rc == CK_OK) rc = ck_upload(W.d_meta, meta.data(), sizeof(int32_t) * meta.size(), h->stream);
    if (rc == CK_OK) rc = ck_upload(W.d_bear, bearings, sizeof(double) * 3 * (size_t)n_bearings_total, h->stream, 8);
    if (rc == CK_OK) rc = ck_upload(W.d_mounts, M.data(), sizeof(double) * M.size(), h->stream);
    if (rc == CK_OK) rc = ck_upload(W.d_tags, tags.data(), tag_bytes, h->stream);
    if (rc == CK_OK) rc = W.d_rms.reserve(rms_bytes);
    if (rc == CK_OK) rc = ck_upload(W.d_steps, steps.data(), step_bytes, h->stream);
    if (rc == CK_OK) rc = W.d_pairs.reserve(sizeof(double) * CKA_B_STRIDE * (n_pairs + 1));
    if (rc == CK_OK) rc = W.d_sights.reserve(sizeof(double) * CKF_I_STRIDE * (n_sights + 1));
    if (rc == CK_OK) rc = W.d_S.reserve(sizeof(double) * (n_S + 1));
    if (rc == CK_OK) rc = ck_upload(W.d_res, results, res_bytes, h->stream);
    if (rc != CK_OK) return rc;
    CK_HIP(hipMemsetAsync(W.d_rms, 0, rms_bytes, h->stream));
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
        ck_fieldcal_result_finish(&plans.v[i], layout0, tags.data() + (size_t)12 * CK_FIELDCAL_MAX_TAGS * i, rms.data() + (size_t)CK_FIELDCAL_MAX_TAGS * i,
                                  layout_out + (size_t)n_layout * i, tag_rms + (size_t)n_layout * i);
        ck_cal_poses_finish(&problems[i], step_index, plans.v[i].meta, dprob[i].U, steps.data() + (size_t)CKA_S_STRIDE * (size_t)dprob[i].step_off, poses_out);
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
    std::vector<ck_iso3_t> tags; // the starts: the rig solver with the tags at layout0
    try {
        tags.resize((size_t)n_tags_total + 1);
    } catch (...) {
        return CK_ENOMEM;
    }
    for (int32_t t = 0; t < n_tags_total; t++) tags[t] = layout0[tag_index[t]];
    ck_cal_starts s;
    rc = ck_cal_starts_solve(h, n_cams, records, n_steps, tags.data(), n_tags_total, bearings, n_bearings_total, gyro, problems, n, step_index, mounts, s);
    if (rc != CK_OK) return rc;
    rc = ck_fieldcal_refine_batch(h, p, n_cams, records, n_steps, tag_index, n_tags_total, bearings, n_bearings_total, s.prob.data(), n,
                                  s.index.data(), s.n_index(), mounts, layout0, n_layout, fixed6, s.poses0.data(), results, layout_out,
                                  tag_sightings, tag_rms, s.poses.data());
    if (rc != CK_OK) return rc;
    ck_cal_starts_finish(s, problems, n, results, poses_out);
    return CK_OK;
}
