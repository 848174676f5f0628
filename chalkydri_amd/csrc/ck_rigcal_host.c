/* Mount calibration, the half that needs no device: the checks every entry point shares, what is decided about a
 * problem before it is solved (which steps count, the gauge, the co-visibility graph), the conversions at the ABI's boundary and
 * ck_rigcal_refine_host, the one-thread twin of k_rigcal.hip.  The arithmetic of the refinement is ck_rigcal_math.h's and ck_cal_math.h's,
 * compiled into both; this file walks views and points the way the kernel's lane groups do, so that the two return the same bytes.
 * What the field calibration does the same way on the host is ck_cal_host.c's. */
#include "ck_cal_c.h"
#include "ck_pose_math.h"
#include "ck_rigcal_c.h"
#include "ck_rigcal_math.h"
#include <stdlib.h>
#include <string.h>

void ck_rigcal_params_default(ck_rigcal_params_t *p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->max_iters = 100; p->min_steps = 3; p->min_cams_per_step = 2;
}

int ck_rigcal_check(const ck_rigcal_params_t *p, int32_t n_cams, const ck_sqpnp_problem_t *records, int32_t n_steps, const ck_iso3_t *tags,
                    int32_t n_tags_total, const double *bearings, int32_t n_bearings_total, const ck_rigcal_problem_t *problems,
                    int32_t n_problems, const int32_t *step_index, int32_t n_index_total, const ck_iso3_t *mounts0) {
    if (!p) return CK_EINVAL;
    const int rc = ck_cal_check(n_cams, records, n_steps, tags, n_tags_total, bearings, n_bearings_total, problems, n_problems, step_index,
                                n_index_total, mounts0, p->max_iters, p->min_steps, p->min_cams_per_step);
    if (rc != CK_OK) return rc;
    for (int64_t i = 0; i < (int64_t)n_cams * n_steps; i++)
        for (int32_t t = 0; t < records[i].n_tags; t++)
            if (!ck_cal_iso_finite(tags + records[i].tag_offset + t)) return CK_EINVAL;
    int gauge = 0;
    for (int32_t c = 0; c < n_cams && !gauge; c++) {
        if (((p->fixed_mask >> (6 * c)) & 63u) != 63u) continue;
        for (int32_t s = 0; s < n_steps && !gauge; s++) gauge = records[(size_t)c * (size_t)n_steps + (size_t)s].n_tags > 0;
    }
    if (!gauge) return CK_EINVAL;
    for (int32_t i = 0; i < n_problems; i++)
        if (problems[i].n_steps > CK_RIGCAL_MAX_STEPS) return CK_ECAPACITY;
    return CK_OK;
}

/* ---- what both solvers share ------------------------------------------------------------------------------------------------- */
/* (w, x, y, z) of a rotation matrix by the largest of the four squared components, w >= 0 */
void ck_rigcal_mat_to_quat(const double R[9], double q[4]) {
    const double K[4] = {1 + R[0] + R[4] + R[8], 1 + R[0] - R[4] - R[8], 1 - R[0] + R[4] - R[8], 1 - R[0] - R[4] + R[8]};
    int k = 0;
    for (int i = 1; i < 4; i++)
        if (K[i] > K[k]) k = i;
    const double s = 2 * sqrt(K[k]);
    if (k == 0) { q[0] = s / 4; q[1] = (R[7] - R[5]) / s; q[2] = (R[2] - R[6]) / s; q[3] = (R[3] - R[1]) / s; }
    else if (k == 1) { q[0] = (R[7] - R[5]) / s; q[1] = s / 4; q[2] = (R[1] + R[3]) / s; q[3] = (R[2] + R[6]) / s; }
    else if (k == 2) { q[0] = (R[2] - R[6]) / s; q[1] = (R[1] + R[3]) / s; q[2] = s / 4; q[3] = (R[5] + R[7]) / s; }
    else { q[0] = (R[3] - R[1]) / s; q[1] = (R[2] + R[6]) / s; q[2] = (R[5] + R[7]) / s; q[3] = s / 4; }
    const double n = (q[0] < 0 ? -1.0 : 1.0) * sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; i++) q[i] /= n;
}

void ck_rigcal_mount_in(const ck_iso3_t *iso, double *M) {
    quat_to_mat(iso->q, M);
    ckp_camera_origin(M, iso->t, M + 9);
}

void ck_rigcal_table(int32_t n_cams, const ck_sqpnp_problem_t *records, int32_t n_steps, const ck_iso3_t *tags, int32_t n_tags_total,
                     int32_t *tab, double *world) {
    for (int32_t t = 0; t < n_tags_total; t++) {
        double R[9];
        quat_to_mat(tags[t].q, R);
        for (int j = 0; j < 4; j++) ckp_tag_corner(R, tags[t].t, j, world + ((size_t)4 * t + j) * 3);
    }
    for (int64_t i = 0; i < (int64_t)n_cams * n_steps; i++) {
        tab[CKR_TAB * i] = 4 * records[i].tag_offset;
        tab[CKR_TAB * i + 1] = records[i].bearing_offset;
        tab[CKR_TAB * i + 2] = records[i].n_bearings;
    }
}

void ck_rigcal_plan(const ck_rigcal_params_t *p, int32_t n_cams, const int32_t *tab, int32_t n_steps, const ck_rigcal_problem_t *problem,
                    const int32_t *step_index, const double *poses0, int32_t *index, ck_rigcal_plan_t *plan) {
    int parent[CK_RIG_MAX_CAMS], anchored[CK_RIG_MAX_CAMS];
    memset(plan, 0, sizeof *plan);
    plan->status = -1;
    for (int c = 0; c < n_cams; c++) parent[c] = c;
    for (int32_t j = 0; j < problem->n_steps; j++) {
        const int32_t s = step_index[problem->step_offset + j];
        int seen = 0, first = -1;
        for (int c = 0; c < n_cams; c++) seen += CKR_NPTS(tab, n_steps, c, s) > 0;
        if (seen < p->min_cams_per_step) continue;
        index[plan->n_used++] = s; /* (the index starts with the used steps, whatever their number) */
        plan->n_views += seen;
        for (int c = 0; c < n_cams; c++) {
            const int32_t k = CKR_NPTS(tab, n_steps, c, s);
            if (k <= 0) continue;
            plan->cam_points[c] += k;
            plan->n_points += k;
            if (first < 0) first = c;
            else parent[ck_cal_find(parent, c)] = ck_cal_find(parent, first);
        }
        for (int i = 0; i < 12; i++)
            if (!ckc_finite(poses0[12 * (size_t)s + i])) plan->status = CK_CALIB_DEGENERATE;
    }
    /* the views, step by step in camera order */
    const cka_index_t x = cka_index_at(index, (size_t)plan->n_used, (size_t)plan->n_views);
    int32_t *first = (int32_t *)x.first, *col = (int32_t *)x.col, *step = (int32_t *)x.step, *colmap = (int32_t *)x.colmap, nv = 0;
    for (int32_t u = 0; u < plan->n_used; u++) {
        first[u] = nv;
        for (int c = 0; c < n_cams; c++) {
            const int on = CKR_NPTS(tab, n_steps, c, x.used[u]) > 0;
            colmap[(size_t)c * plan->n_used + u] = on ? nv : -1;
            if (on) { col[nv] = c; step[nv] = u; nv++; }
        }
    }
    first[plan->n_used] = nv;
    plan->mask = p->fixed_mask;
    for (int c = 0; c < n_cams; c++)
        if (plan->cam_points[c] == 0) plan->mask |= CK_RIGCAL_FIX_CAMERA(c);
    if (plan->n_used < p->min_steps) plan->status = CK_CALIB_DEGENERATE;
    /* every camera that moves hangs on one that does not */
    for (int c = 0; c < n_cams; c++) anchored[c] = 0;
    for (int c = 0; c < n_cams; c++)
        if (plan->cam_points[c] > 0 && ((p->fixed_mask >> (6 * c)) & 63u) == 63u) anchored[ck_cal_find(parent, c)] = 1;
    for (int c = 0; c < n_cams; c++)
        if (plan->cam_points[c] > 0 && ((p->fixed_mask >> (6 * c)) & 63u) != 63u && !anchored[ck_cal_find(parent, c)]) plan->status = CK_CALIB_DEGENERATE;
}

void ck_rigcal_result_start(const ck_rigcal_problem_t *problem, const ck_rigcal_plan_t *plan, int32_t n_cams, const ck_iso3_t *mounts0,
                            ck_rigcal_result_t *res) {
    memset(res, 0, sizeof *res);
    for (int c = 0; c < n_cams; c++) res->robot_to_cam[c] = mounts0[c];
    res->status = plan->status;
    res->n_steps = problem->n_steps; res->n_steps_used = plan->n_used; res->n_points = plan->n_points;
    for (int c = 0; c < n_cams; c++) res->cam_points[c] = plan->cam_points[c];
}

void ck_rigcal_result_finish(const ck_rigcal_plan_t *plan, int32_t n_cams, const ck_iso3_t *mounts0, const double *M, ck_rigcal_result_t *res) {
    for (int c = 0; c < n_cams; c++) {
        const unsigned m6 = (unsigned)((plan->mask >> (6 * c)) & 63u);
        const double *Mc = M + 12 * c;
        ck_iso3_t *o = res->robot_to_cam + c;
        *o = mounts0[c];
        if (m6 == 63u) continue;
        if ((m6 & 7u) != 7u) ck_rigcal_mat_to_quat(Mc, o->q);
        for (int i = 0; i < 3; i++) o->t[i] = -(Mc[3 * i] * Mc[9] + Mc[3 * i + 1] * Mc[10] + Mc[3 * i + 2] * Mc[11]);
    }
}

int ck_rigcal_jacobian(const ck_iso3_t *mount, const double *pose, const double *world_xyz, const double *bearings, int32_t n,
                       uint32_t fixed6, double *r_out, double *J_out) {
    if (!mount || !pose || !world_xyz || !bearings || !r_out || !J_out || n < 0) return CK_EINVAL;
    double M[12];
    ck_rigcal_mount_in(mount, M);
    for (int32_t i = 0; i < n; i++) ckr_jacobian(M, pose, world_xyz + 3 * (size_t)i, bearings + 3 * (size_t)i, fixed6 & 63u, r_out + 3 * (size_t)i, J_out + 3 * CKA_NJ * (size_t)i);
    return CK_OK;
}

/* ---- the twin ---------------------------------------------------------------------------------------------------------------- */
typedef struct {
    cka_index_t x;
    const int32_t *tab;
    const double *world, *bear;
    int n, U, P;
    double *st, *vw;
    double part[CKR_GROUP][CKA_NACC];
} twin_t;

/* the xor butterfly 8, 4, 2, 1 of a group's partial sums, as its lane 0 sees it */
static void butterfly(double (*part)[CKA_NACC], int n) {
    for (int m = CKR_GROUP / 2; m >= 1; m >>= 1)
        for (int l = 0; l < m; l++)
            for (int j = 0; j < n; j++) part[l][j] = part[l][j] + part[l + m][j];
}

/* the candidate's cost: per view by lanes and butterfly, per step the views in camera order, then the steps in order */
static double twin_cost(twin_t *T, const double *Mc) {
    for (int u = 0; u < T->U; u++) {
        double *st = T->st + (size_t)CKA_S_STRIDE * u, cs = 0.0;
        for (int v = T->x.first[u]; v < T->x.first[u + 1]; v++) {
            const int c = T->x.col[v];
            const int32_t *tb = T->tab + ((size_t)c * T->n + T->x.used[u]) * CKR_TAB;
            for (int l = 0; l < CKR_GROUP; l++) {
                double a = 0.0, e[3];
                for (int i = l; i < tb[2]; i += CKR_GROUP) {
                    ckr_residual(Mc + 12 * c, st + CKA_S_CAND, T->world + 3 * ((size_t)tb[0] + i), T->bear + 3 * ((size_t)tb[1] + i), e);
                    a = a + ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
                }
                T->part[l][0] = a;
            }
            butterfly(T->part, 1);
            T->vw[(size_t)CKA_B_STRIDE * v + CKA_B_COST] = T->part[0][0];
            cs = cs + T->part[0][0];
        }
        st[CKA_S_COST] = cs;
    }
    double t = 0.0;
    for (int u = 0; u < T->U; u++) t = t + T->st[(size_t)CKA_S_STRIDE * u + CKA_S_COST];
    return t;
}

static void twin_jacobian(twin_t *T, const double *M, const int32_t *mask6) {
    for (int v = 0; v < T->P; v++) {
        const int c = T->x.col[v];
        const int32_t *tb = T->tab + ((size_t)c * T->n + T->x.used[T->x.step[v]]) * CKR_TAB;
        const double *st = T->st + (size_t)CKA_S_STRIDE * T->x.step[v];
        for (int l = 0; l < CKR_GROUP; l++) {
            double e[3], J[3 * CKA_NJ];
            for (int j = 0; j < CKA_NACC; j++) T->part[l][j] = 0.0;
            for (int i = l; i < tb[2]; i += CKR_GROUP) {
                ckr_jacobian(M + 12 * c, st + CKA_S_POSE, T->world + 3 * ((size_t)tb[0] + i), T->bear + 3 * ((size_t)tb[1] + i), (unsigned)mask6[c], e, J);
                ckr_accumulate_rows(T->part[l], T->part[l] + CKA_NH, e, J, 0, CKA_NJ);
            }
        }
        butterfly(T->part, CKA_NACC);
        memcpy(T->vw + (size_t)CKA_B_STRIDE * v + CKA_B_H, T->part[0], sizeof(double) * CKA_NACC);
    }
}

static void accept_costs(twin_t *T) {
    for (int v = 0; v < T->P; v++) T->vw[(size_t)CKA_B_STRIDE * v + CKA_B_COSTA] = T->vw[(size_t)CKA_B_STRIDE * v + CKA_B_COST];
}

int ck_rigcal_refine_host(const ck_rigcal_params_t *p, int32_t n_cams, const ck_sqpnp_problem_t *records, int32_t n_steps,
                          const ck_iso3_t *tags, int32_t n_tags_total, const double *bearings, int32_t n_bearings_total,
                          const ck_rigcal_problem_t *problem, const int32_t *step_index, int32_t n_index_total, const ck_iso3_t *mounts0,
                          const double *poses0, ck_rigcal_result_t *res, double *poses_out) {
    if (!poses0 || !res || !poses_out) return CK_EINVAL;
    const int rc = ck_rigcal_check(p, n_cams, records, n_steps, tags, n_tags_total, bearings, n_bearings_total, problem, 1, step_index,
                                   n_index_total, mounts0);
    if (rc != CK_OK) return rc;
    const int N = 6 * n_cams;
    ck_rigcal_plan_t plan;
    int32_t *tab = (int32_t *)malloc(sizeof(int32_t) * CKR_TAB * ((size_t)n_cams * n_steps + 1));
    double *world = (double *)malloc(sizeof(double) * 12 * ((size_t)n_tags_total + 1));
    int32_t *index = (int32_t *)malloc(sizeof(int32_t) * (cka_index_size((size_t)problem->n_steps, (size_t)n_cams * (size_t)problem->n_steps, (size_t)n_cams) + 1));
    twin_t *T = (twin_t *)calloc(1, sizeof(twin_t));
    double *S = (double *)malloc(sizeof(double) * ((size_t)N * N + (size_t)N + CKA_HK * CK_RIG_MAX_CAMS));
    int ret = CK_ENOMEM;
    if (!tab || !world || !index || !T || !S) goto done;
    ck_rigcal_table(n_cams, records, n_steps, tags, n_tags_total, tab, world);
    ck_rigcal_plan(p, n_cams, tab, n_steps, problem, step_index, poses0, index, &plan);
    ck_rigcal_result_start(problem, &plan, n_cams, mounts0, res);
    ck_cal_poses_start(problem, step_index, poses0, poses_out);
    ret = CK_OK;
    if (plan.status == CK_CALIB_DEGENERATE) goto done;
    T->x = cka_index_at(index, (size_t)plan.n_used, (size_t)plan.n_views);
    T->tab = tab; T->world = world; T->bear = bearings;
    T->n = n_steps; T->U = plan.n_used; T->P = plan.n_views;
    T->st = (double *)calloc((size_t)CKA_S_STRIDE * (size_t)T->U, sizeof(double));
    T->vw = (double *)calloc((size_t)CKA_B_STRIDE * (size_t)T->P, sizeof(double));
    if (!T->st || !T->vw) { ret = CK_ENOMEM; goto done; }
    {
        double M[12 * CK_RIG_MAX_CAMS], Mc[12 * CK_RIG_MAX_CAMS];
        double *dk = S + (size_t)N * N, *Hc = dk + N;
        int32_t mask6[CK_RIG_MAX_CAMS];
        for (int c = 0; c < n_cams; c++) {
            ck_rigcal_mount_in(mounts0 + c, M + 12 * c);
            mask6[c] = (int32_t)((plan.mask >> (6 * c)) & 63u);
        }
        memcpy(Mc, M, sizeof M);
        ck_cal_steps_seed(T->st, T->x.used, T->U, poses0);
        const double cost0 = twin_cost(T, Mc);
        accept_costs(T);
        res->status = CK_CALIB_DEGENERATE;
        if (!ckc_finite(cost0)) goto done;
        ckc_lm_t lm;
        ckc_lm_start(&lm, cost0, CKR_COST_FLOOR);
        while (lm.status < 0) {
            if (lm.need_jac) {
                twin_jacobian(T, M, mask6);
                for (int j = 0; j < CKA_HK * n_cams; j++) Hc[j] = cka_col_sum(T->vw, T->x.colmap + (size_t)(j / CKA_HK) * T->U, T->U, j % CKA_HK);
            }
            int solved = 1;
            for (int u = 0; u < T->U; u++)
                if (!cka_step_schur(T->st + (size_t)CKA_S_STRIDE * u, T->vw + (size_t)CKA_B_STRIDE * T->x.first[u], T->x.first[u + 1] - T->x.first[u], lm.lambda))
                    solved = 0;
            for (int r = 0; r < N; r++) {
                for (int k = 0; k <= r; k++) S[r * N + k] = cka_reduced_entry(T->vw, T->x.colmap, mask6, Hc, T->U, NULL, T->U, lm.lambda, r, k);
                dk[r] = cka_reduced_rhs(T->vw, T->x.colmap, mask6, Hc, T->U, r);
            }
            if (!ckc_chol_n(S, N)) solved = 0;
            ckc_fwd_n(S, N, dk, 1);
            ckc_bwd_n(S, N, dk);
            double pred = cka_reduced_pred(mask6, Hc, N, lm.lambda, dk), cost_new = 0.0;
            if (solved) {
                for (int c = 0; c < n_cams; c++) ckc_rigid_step(M + 12 * c, dk + 6 * c, (unsigned)mask6[c], Mc + 12 * c);
                for (int u = 0; u < T->U; u++)
                    cka_step_step(T->st + (size_t)CKA_S_STRIDE * u, T->vw + (size_t)CKA_B_STRIDE * T->x.first[u], T->x.col + T->x.first[u],
                                  T->x.first[u + 1] - T->x.first[u], dk, lm.lambda);
                for (int u = 0; u < T->U; u++) pred = pred + T->st[(size_t)CKA_S_STRIDE * u + CKA_S_PRED];
                cost_new = twin_cost(T, Mc);
            }
            if (ckc_lm_decide(&lm, solved, pred, cost_new, p->max_iters, CKR_COST_FLOOR)) {
                memcpy(M, Mc, sizeof M);
                for (int u = 0; u < T->U; u++)
                    memcpy(T->st + (size_t)CKA_S_STRIDE * u + CKA_S_POSE, T->st + (size_t)CKA_S_STRIDE * u + CKA_S_CAND, sizeof(double) * 12);
                accept_costs(T);
            }
        }
        ck_cal_poses_finish(problem, step_index, T->x.used, T->U, T->st, poses_out);
        ck_rigcal_result_finish(&plan, n_cams, mounts0, M, res);
        res->status = lm.status; res->iters = lm.iters;
        res->cost0 = cost0; res->cost = lm.cost;
        res->rms = sqrt(lm.cost / (double)res->n_points);
        for (int c = 0; c < n_cams; c++)
            if (plan.cam_points[c] > 0) res->cam_rms[c] = cka_col_rms(T->vw, T->x.colmap + (size_t)c * T->U, T->U, plan.cam_points[c]);
    }
done:
    if (T) { free(T->st); free(T->vw); }
    free(tab); free(world); free(index); free(T); free(S);
    return ret;
}
