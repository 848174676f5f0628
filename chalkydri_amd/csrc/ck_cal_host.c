/* Mount and field calibration, the host code the two share: see ck_cal_c.h. */
#include "ck_cal_c.h"
#include "ck_cal_math.h"
#include <string.h>

int ck_cal_iso_finite(const ck_iso3_t *t) {
    for (int k = 0; k < 3; k++)
        if (!ckc_finite(t->t[k])) return 0;
    for (int k = 0; k < 4; k++)
        if (!ckc_finite(t->q[k])) return 0;
    return t->q[0] * t->q[0] + t->q[1] * t->q[1] + t->q[2] * t->q[2] + t->q[3] * t->q[3] > 0.0;
}

int ck_cal_find(int *parent, int i) {
    while (parent[i] != i) i = parent[i] = parent[parent[i]];
    return i;
}

int ck_cal_check(int32_t n_cams, const ck_sqpnp_problem_t *records, int32_t n_steps, const void *tags, int32_t n_tags_total,
                 const double *bearings, int32_t n_bearings_total, const ck_rigcal_problem_t *problems, int32_t n_problems,
                 const int32_t *step_index, int32_t n_index_total, const ck_iso3_t *mounts, int32_t max_iters, int32_t min_steps,
                 int32_t min_per_step) {
    if (!records || !problems || !step_index || !mounts) return CK_EINVAL;
    if ((!tags && n_tags_total != 0) || (!bearings && n_bearings_total != 0)) return CK_EINVAL;
    if (n_cams < 1 || n_cams > CK_RIG_MAX_CAMS) return CK_EINVAL;
    if (n_steps < 0 || n_tags_total < 0 || n_bearings_total < 0 || n_problems < 0 || n_index_total < 0) return CK_EINVAL;
    if (n_tags_total > 0x0FFFFFFF || (int64_t)n_cams * n_steps > 0x0FFFFFFF) return CK_EINVAL;
    const int64_t n_rec = (int64_t)n_cams * n_steps;
    for (int64_t i = 0; i < n_rec; i++) {
        const ck_sqpnp_problem_t *r = records + i;
        if (r->n_tags < 0 || r->n_bearings < 0 || r->tag_offset < 0 || r->bearing_offset < 0) return CK_EINVAL;
        if ((int64_t)r->tag_offset + r->n_tags > n_tags_total || (int64_t)r->bearing_offset + r->n_bearings > n_bearings_total) return CK_EINVAL;
        if ((int64_t)4 * r->n_tags != r->n_bearings) return CK_EINVAL;
    }
    for (int32_t i = 0; i < n_problems; i++) {
        const ck_rigcal_problem_t *q = problems + i;
        if (q->n_steps < 0 || q->step_offset < 0 || (int64_t)q->step_offset + q->n_steps > n_index_total) return CK_EINVAL;
        for (int32_t j = 0; j < q->n_steps; j++) {
            const int32_t s = step_index[q->step_offset + j];
            if (s < 0 || s >= n_steps || (j > 0 && s <= step_index[q->step_offset + j - 1])) return CK_EINVAL;
        }
    }
    if (max_iters < 1 || max_iters > 10000 || min_steps < 1 || min_per_step < 2) return CK_EINVAL;
    for (int64_t i = 0; i < n_rec; i++) {
        const ck_sqpnp_problem_t *r = records + i;
        for (int64_t j = 3 * (int64_t)r->bearing_offset; j < 3 * ((int64_t)r->bearing_offset + r->n_bearings); j++)
            if (!ckc_finite(bearings[j])) return CK_EINVAL;
    }
    for (int32_t c = 0; c < n_cams; c++)
        if (!ck_cal_iso_finite(mounts + c)) return CK_EINVAL;
    return CK_OK;
}

void ck_cal_poses_start(const ck_rigcal_problem_t *problem, const int32_t *step_index, const double *poses0, double *poses_out) {
    for (int32_t j = 0; j < problem->n_steps; j++)
        memcpy(poses_out + 12 * ((size_t)problem->step_offset + j), poses0 + 12 * (size_t)step_index[problem->step_offset + j], sizeof(double) * 12);
}

void ck_cal_steps_seed(double *steps, const int32_t *used, int32_t n_used, const double *poses0) {
    for (int32_t u = 0; u < n_used; u++) {
        double *st = steps + (size_t)CKA_S_STRIDE * u;
        memcpy(st + CKA_S_POSE, poses0 + 12 * (size_t)used[u], sizeof(double) * 12);
        memcpy(st + CKA_S_CAND, st + CKA_S_POSE, sizeof(double) * 12);
    }
}

void ck_cal_poses_finish(const ck_rigcal_problem_t *problem, const int32_t *step_index, const int32_t *used, int32_t n_used,
                         const double *steps, double *poses_out) {
    for (int32_t u = 0, j = 0; u < n_used; u++) {
        while (step_index[problem->step_offset + j] != used[u]) j++;
        memcpy(poses_out + 12 * ((size_t)problem->step_offset + j), steps + (size_t)CKA_S_STRIDE * u + CKA_S_POSE, sizeof(double) * 12);
    }
}
