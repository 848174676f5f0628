/* Rig pose refinement, the half that needs no device: the checks both entry points share and ck_rig_refine_host, the
 * one-thread twin of k_rig_refine.hip.  The solve is ck_rig_refine_math.h's, compiled into both; this file walks the points the way the
 * kernel's 64 lanes do, so that the two return the same bytes. */
#include "ck_rig_refine_c.h"
#include "ck_rig_refine_math.h"
#include <stdlib.h>
#include <string.h>

void ck_rig_refine_params_default(ck_rig_refine_params_t *p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->mode = CK_RIG_REFINE_FREE; p->max_iters = 10;
    p->sigma_rad = 1e-3; p->gyro_sigma_rad = 0.0; p->z = 0.0;
}

int ck_rig_refine_params_check(const ck_rig_refine_params_t *p) {
    if (!p) return CK_EINVAL;
    if (p->mode != CK_RIG_REFINE_FREE && p->mode != CK_RIG_REFINE_PLANAR) return CK_EINVAL;
    if (!ckc_finite(p->sigma_rad) || !ckc_finite(p->z) || !(p->sigma_rad > 0.0)) return CK_EINVAL;
    if (!ckc_finite(p->gyro_sigma_rad) || p->gyro_sigma_rad < 0.0) return CK_EINVAL;
    if (p->max_iters < 1 || p->max_iters > 100) return CK_EINVAL;
    return CK_OK;
}

int ck_rig_refine_check(const ck_rig_refine_params_t *params, int32_t n_cams, const ck_sqpnp_problem_t *problems, int32_t n, const void *tags,
                        int32_t n_tags_total, const void *bearings, int32_t n_bearings_total, const void *gyro, const void *start,
                        const void *out, int32_t *max_points) {
    ck_rig_params_t rig; /* (ck_rig_check only compares it with null) */
    if (!params || !problems || !start || !out) return CK_EINVAL;
    memset(&rig, 0, sizeof rig);
    int rc = ck_rig_check(&rig, n_cams, problems, n, tags, n_tags_total, bearings, n_bearings_total, problems, out, max_points);
    if (rc != CK_OK) return rc;
    if ((rc = ck_rig_refine_params_check(params)) != CK_OK) return rc;
    if (params->gyro_sigma_rad > 0.0 && !gyro) return CK_EINVAL;
    return CK_OK;
}

/* ---- the twin ---------------------------------------------------------------------------------------------------------------- */
/* the xor butterfly 32 .. 1 of the lanes' partial sums, as lane 0 sees it */
static void butterfly(double (*part)[CKF_NSUM], int n) {
    for (int m = CKF_LANES / 2; m >= 1; m >>= 1)
        for (int l = 0; l < m; l++)
            for (int j = 0; j < n; j++) part[l][j] = part[l][j] + part[l + m][j];
}

#define REC(cx, i, j) ((cx)->pts[(size_t)(j) * (cx)->stride + (size_t)(i)])
static void load_point(const ckf_ctx_t *cx, int i, double *X, double *v, double *M) {
    for (int k = 0; k < 3; k++) { X[k] = REC(cx, i, k); v[k] = REC(cx, i, 3 + k); }
    for (int k = 0; k < 12; k++) M[k] = REC(cx, i, 6 + k);
}

static inline void ckf_walk_jac(const ckf_ctx_t *cx, const int planar, const double *P, const double *xy, double *acc) {
    double (*part)[CKF_NSUM] = (double (*)[CKF_NSUM])cx->part;
    const int n = planar ? 9 : CKF_NSUM;
    for (int l = 0; l < CKF_LANES; l++) {
        for (int j = 0; j < n; j++) part[l][j] = 0.0;
        for (int i = l; i < cx->np; i += CKF_LANES) {
            double X[3], v[3], M[12];
            load_point(cx, i, X, v, M);
            ckf_point_sums(planar, M, P, xy, X, v, part[l]);
        }
    }
    butterfly(part, n);
    for (int j = 0; j < n; j++) acc[j] = part[0][j];
}

static inline void ckf_walk_cost(const ckf_ctx_t *cx, const double *P, double *cost, int *behind) {
    double (*part)[CKF_NSUM] = (double (*)[CKF_NSUM])cx->part;
    int bad = 0;
    for (int l = 0; l < CKF_LANES; l++) {
        double a = 0.0;
        for (int i = l; i < cx->np; i += CKF_LANES) {
            double X[3], v[3], M[12], e[3];
            load_point(cx, i, X, v, M);
            if (!(ckf_residual(M, P, X, v, e) > 0.0)) bad = 1;
            a = a + ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
        }
        part[l][0] = a;
    }
    butterfly(part, 1);
    *cost = part[0][0];
    *behind = bad;
}

static inline void ckf_walk_cams(const ckf_ctx_t *cx, const double *P, double *cam_cost) {
    double (*part)[CKF_NSUM] = (double (*)[CKF_NSUM])cx->part;
    for (int l = 0; l < CKF_LANES; l++) {
        for (int c = 0; c < CK_RIG_MAX_CAMS; c++) part[l][c] = 0.0;
        for (int i = l; i < cx->np; i += CKF_LANES) {
            double X[3], v[3], M[12], e[3];
            load_point(cx, i, X, v, M);
            ckf_residual(M, P, X, v, e);
            const int c = (int)REC(cx, i, 18);
            part[l][c] = part[l][c] + ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
        }
    }
    butterfly(part, CK_RIG_MAX_CAMS);
    for (int c = 0; c < CK_RIG_MAX_CAMS; c++) cam_cost[c] = part[0][c];
}

int ck_rig_refine_host(const ck_rig_refine_params_t *params, int32_t n_cams, const ck_sqpnp_problem_t *problems, int32_t n,
                       const ck_iso3_t *tags, int32_t n_tags_total, const double *bearings, int32_t n_bearings_total, const double *gyro,
                       const ck_rig_result_t *start, const uint64_t *rejected, ck_rig_refined_t *out) {
    int32_t max_points = 0;
    const int rc = ck_rig_refine_check(params, n_cams, problems, n, tags, n_tags_total, bearings, n_bearings_total, gyro, start, out, &max_points);
    if (rc != CK_OK) return rc;
    const size_t cap = max_points > 0 ? (size_t)max_points : 1;
    /* the call's own memory: the point records, then the walkers' partial sums (no state outlives or is shared between calls) */
    double *pts = (double *)malloc(sizeof(double) * (CKF_PT * cap + (size_t)CKF_LANES * CKF_NSUM));
    if (!pts) return CK_ENOMEM;
    double *part = pts + CKF_PT * cap;
    const int prior = params->gyro_sigma_rad > 0.0;
    for (int32_t s = 0; s < n; s++) {
        ck_rig_refined_t *r = out + s;
        memset(r, 0, sizeof *r);
        if (!start[s].valid) { r->status = CK_RIG_REFINE_NO_START; continue; }
        ckf_ctx_t cx = {pts, cap, 0, 0, part};
        int cam_np[CK_RIG_MAX_CAMS] = {0};
        for (int c = 0; c < n_cams; c++) {
            const ck_sqpnp_problem_t *p = &problems[(size_t)c * (size_t)n + (size_t)s];
            const uint64_t rej = rejected ? rejected[(size_t)s * CK_RIG_MAX_CAMS + c] : 0;
            const int kept = ckf_kept(p->n_tags, rej);
            for (int k = 0; k < 4 * kept; k++) {
                const int t = ckf_kept_tag(p->n_tags, rej, k >> 2);
                double rec[CKF_PT];
                ckf_point_record(tags[p->tag_offset + t].t, tags[p->tag_offset + t].q, k & 3, bearings + 3 * ((size_t)p->bearing_offset + 4 * (size_t)t + (k & 3)),
                                 p->robot_to_cam.t, p->robot_to_cam.q, rec);
                rec[18] = (double)c;
                for (int j = 0; j < CKF_PT; j++) pts[(size_t)j * cap + (size_t)cx.np] = rec[j];
                cx.np++;
            }
            cam_np[c] = 4 * kept;
        }
        const double cg = prior ? cos(gyro[s]) : 0.0, sg = prior ? sin(gyro[s]) : 0.0;
        if (params->mode == CK_RIG_REFINE_PLANAR)
            ckf_solve(&cx, 1, params->sigma_rad, params->gyro_sigma_rad, params->z, params->max_iters, prior, cg, sg, start[s].rot, start[s].pos, cam_np, r);
        else
            ckf_solve(&cx, 0, params->sigma_rad, params->gyro_sigma_rad, params->z, params->max_iters, prior, cg, sg, start[s].rot, start[s].pos, cam_np, r);
    }
    free(pts);
    return CK_OK;
}
