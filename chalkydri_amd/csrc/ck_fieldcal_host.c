/* Field calibration, the half that needs no device: the checks every entry point shares, what is decided about a
 * problem before it is solved (which steps count, the tags with sightings, the sightings in the order they are summed in, the gauge,
 * the co-visibility graph), the conversions at the ABI's boundary and ck_fieldcal_refine_host, the one-thread twin of k_fieldcal.hip.
 * The arithmetic is ck_fieldcal_math.h's and ck_cal_math.h's, compiled into both; this file walks sightings, pairs and steps the way the
 * kernel's lanes and threads do, and factors the reduced system in the order the kernel's rows do, so that the two return the same
 * bytes.  What the mount calibration does the same way on the host is ck_cal_host.c's. */
#include "ck_cal_c.h"
#include "ck_fieldcal_c.h"
#include "ck_fieldcal_math.h"
#include "ck_pose_math.h"
#include "ck_rigcal_c.h"
#include <stdlib.h>
#include <string.h>

void ck_fieldcal_params_default(ck_fieldcal_params_t *p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->max_iters = 100; p->min_steps = 3; p->min_tags_per_step = 2;
}

int ck_fieldcal_check(const ck_fieldcal_params_t *p, int32_t n_cams, const ck_sqpnp_problem_t *records, int32_t n_steps,
                      const int32_t *tag_index, int32_t n_tags_total, const double *bearings, int32_t n_bearings_total,
                      const ck_rigcal_problem_t *problems, int32_t n_problems, const int32_t *step_index, int32_t n_index_total,
                      const ck_iso3_t *mounts, const ck_iso3_t *layout0, int32_t n_layout, const uint8_t *fixed6) {
    if (!p || !layout0 || !fixed6 || n_layout < 1 || n_layout > 0x0FFFFFFF) return CK_EINVAL;
    int rc = ck_cal_check(n_cams, records, n_steps, tag_index, n_tags_total, bearings, n_bearings_total, problems, n_problems, step_index,
                          n_index_total, mounts, p->max_iters, p->min_steps, p->min_tags_per_step);
    if (rc != CK_OK) return rc;
    const int64_t n_rec = (int64_t)n_cams * n_steps;
    for (int32_t t = 0; t < n_tags_total; t++)
        if (tag_index[t] < 0 || tag_index[t] >= n_layout) return CK_EINVAL;
    for (int32_t k = 0; k < n_layout; k++)
        if (fixed6[k] > CK_FIELDCAL_FIX_ALL || !ck_cal_iso_finite(layout0 + k)) return CK_EINVAL;
    int gauge = 0;
    for (int64_t i = 0; i < n_rec; i++) {
        const int32_t *ti = tag_index + records[i].tag_offset;
        for (int32_t a = 0; a < records[i].n_tags; a++) {
            for (int32_t b = 0; b < a; b++)
                if (ti[a] == ti[b]) return CK_EINVAL;
            gauge |= fixed6[ti[a]] == CK_FIELDCAL_FIX_ALL;
        }
    }
    if (!gauge) return CK_EINVAL;
    for (int32_t i = 0; i < n_problems; i++)
        if (problems[i].n_steps > CK_FIELDCAL_MAX_STEPS) return CK_ECAPACITY;
    int32_t *stamp = (int32_t *)calloc((size_t)n_layout, sizeof(int32_t));
    if (!stamp) return CK_ENOMEM;
    for (int32_t i = 0; i < n_problems && rc == CK_OK; i++) {
        int32_t seen = 0;
        for (int32_t j = 0; j < problems[i].n_steps; j++) {
            const int32_t s = step_index[problems[i].step_offset + j];
            for (int32_t c = 0; c < n_cams; c++) {
                const ck_sqpnp_problem_t *r = records + (size_t)c * (size_t)n_steps + (size_t)s;
                for (int32_t t = 0; t < r->n_tags; t++) {
                    const int32_t k = tag_index[r->tag_offset + t];
                    if (stamp[k] != i + 1) { stamp[k] = i + 1; seen++; }
                }
            }
        }
        if (seen > CK_FIELDCAL_MAX_TAGS) rc = CK_ECAPACITY;
    }
    free(stamp);
    return rc;
}

/* ---- what both solvers share ------------------------------------------------------------------------------------------------- */
void ck_fieldcal_tag_in(const ck_iso3_t *iso, double *T) {
    quat_to_mat(iso->q, T);
    for (int i = 0; i < 3; i++) T[9 + i] = iso->t[i];
}

void ck_fieldcal_plan_free(ck_fieldcal_plan_t *plan) {
    if (plan) { free(plan->meta); plan->meta = NULL; }
}

int ck_fieldcal_plan(const ck_fieldcal_params_t *p, int32_t n_cams, const ck_sqpnp_problem_t *records, int32_t n_steps,
                     const int32_t *tag_index, const ck_rigcal_problem_t *problem, const int32_t *step_index, int32_t n_layout,
                     const uint8_t *fixed6, const double *poses0, int32_t *tag_sightings, ck_fieldcal_plan_t *plan) {
    memset(plan, 0, sizeof *plan);
    plan->status = -1;
    memset(tag_sightings, 0, sizeof(int32_t) * (size_t)n_layout);
    int32_t *stamp = (int32_t *)calloc((size_t)n_layout, sizeof(int32_t));
    int32_t *loc = (int32_t *)malloc(sizeof(int32_t) * (size_t)n_layout);
    int32_t *used = (int32_t *)malloc(sizeof(int32_t) * ((size_t)problem->n_steps + 1));
    int32_t *key = NULL, *kbo = NULL;
    int ret = CK_ENOMEM;
    if (!stamp || !loc || !used) goto done;
    size_t U = 0, P = 0, NS = 0, T = 0;
    int32_t most = 0;
    for (int32_t j = 0; j < problem->n_steps; j++) {
        const int32_t s = step_index[problem->step_offset + j];
        int32_t distinct = 0, sights = 0;
        for (int32_t c = 0; c < n_cams; c++) {
            const ck_sqpnp_problem_t *r = records + (size_t)c * (size_t)n_steps + (size_t)s;
            for (int32_t t = 0; t < r->n_tags; t++) {
                const int32_t k = tag_index[r->tag_offset + t];
                if (stamp[k] != j + 1) { stamp[k] = j + 1; distinct++; }
            }
            sights += r->n_tags;
        }
        if (distinct < p->min_tags_per_step) continue;
        used[U++] = s;
        P += (size_t)distinct; NS += (size_t)sights;
        if (sights > most) most = sights;
        for (int32_t c = 0; c < n_cams; c++) {
            const ck_sqpnp_problem_t *r = records + (size_t)c * (size_t)n_steps + (size_t)s;
            for (int32_t t = 0; t < r->n_tags; t++) tag_sightings[tag_index[r->tag_offset + t]]++;
        }
        for (int i = 0; i < 12; i++)
            if (!ckc_finite(poses0[12 * (size_t)s + i])) plan->status = CK_CALIB_DEGENERATE;
    }
    for (int32_t k = 0; k < n_layout; k++) loc[k] = tag_sightings[k] > 0 ? (int32_t)T++ : -1;
    if (T > CK_FIELDCAL_MAX_TAGS) { ret = CK_ECAPACITY; goto done; }
    if ((int32_t)U < p->min_steps) plan->status = CK_CALIB_DEGENERATE;
    plan->n_used = (int32_t)U; plan->n_pairs = (int32_t)P; plan->n_sights = (int32_t)NS; plan->n_tags = (int32_t)T;
    plan->n_points = (int32_t)(4 * NS);
    plan->n_meta = ckf_meta_size(U, P, NS, T);
    plan->meta = (int32_t *)malloc(sizeof(int32_t) * (plan->n_meta + 1));
    key = (int32_t *)malloc(sizeof(int32_t) * ((size_t)most + 1));
    kbo = (int32_t *)malloc(sizeof(int32_t) * ((size_t)most + 1));
    if (!plan->meta || !key || !kbo) goto done;
    {
        const ckf_meta_t m = ckf_meta_at(plan->meta, U, P, NS, T);
        int32_t *m_used = (int32_t *)m.ix.used, *step_pair = (int32_t *)m.ix.first, *pair_tag = (int32_t *)m.ix.col;
        int32_t *pair_step = (int32_t *)m.ix.step, *pair_sight = (int32_t *)m.pair_sight, *sight_pair = (int32_t *)m.sight_pair;
        int32_t *sight_cam = (int32_t *)m.sight_cam, *sight_bear = (int32_t *)m.sight_bear, *pairmap = (int32_t *)m.ix.colmap;
        int32_t *ltag = (int32_t *)m.ltag, *tag_ns = (int32_t *)m.tag_ns, *mask6 = (int32_t *)m.mask6;
        int parent[CK_FIELDCAL_MAX_TAGS], anchored[CK_FIELDCAL_MAX_TAGS];
        for (size_t i = 0; i < T * U; i++) pairmap[i] = -1;
        for (int32_t k = 0; k < n_layout; k++)
            if (loc[k] >= 0) { ltag[loc[k]] = k; tag_ns[loc[k]] = tag_sightings[k]; mask6[loc[k]] = fixed6[k] & 63; }
        for (size_t k = 0; k < T; k++) { parent[k] = (int)k; anchored[k] = 0; }
        int32_t np = 0, ns = 0;
        for (size_t u = 0; u < U; u++) {
            const int32_t s = used[u];
            m_used[u] = s;
            step_pair[u] = np;
            /* the step's sightings, by tag and then camera */
            int32_t n = 0;
            for (int32_t c = 0; c < n_cams; c++) {
                const ck_sqpnp_problem_t *r = records + (size_t)c * (size_t)n_steps + (size_t)s;
                for (int32_t t = 0; t < r->n_tags; t++) {
                    const int32_t kk = loc[tag_index[r->tag_offset + t]] * CK_RIG_MAX_CAMS + c, bo = r->bearing_offset + 4 * t;
                    int32_t i = n++;
                    for (; i > 0 && key[i - 1] > kk; i--) { key[i] = key[i - 1]; kbo[i] = kbo[i - 1]; }
                    key[i] = kk; kbo[i] = bo;
                }
            }
            for (int32_t i = 0; i < n; i++) {
                const int32_t k = key[i] / CK_RIG_MAX_CAMS;
                if (i == 0 || key[i - 1] / CK_RIG_MAX_CAMS != k) {
                    pair_tag[np] = k; pair_step[np] = (int32_t)u; pair_sight[np] = ns;
                    pairmap[(size_t)k * U + u] = np;
                    parent[ck_cal_find(parent, k)] = ck_cal_find(parent, key[0] / CK_RIG_MAX_CAMS);
                    np++;
                }
                sight_pair[ns] = np - 1; sight_cam[ns] = key[i] % CK_RIG_MAX_CAMS; sight_bear[ns] = kbo[i];
                ns++;
            }
        }
        step_pair[U] = np;
        pair_sight[P] = ns;
        /* every tag that moves hangs on one that does not */
        for (size_t k = 0; k < T; k++)
            if (mask6[k] == 63) anchored[ck_cal_find(parent, (int)k)] = 1;
        for (size_t k = 0; k < T; k++) {
            if (mask6[k] == 63) continue;
            plan->n_solved++;
            if (!anchored[ck_cal_find(parent, (int)k)]) plan->status = CK_CALIB_DEGENERATE;
        }
    }
    ret = CK_OK;
done:
    free(stamp); free(loc); free(used); free(key); free(kbo);
    if (ret != CK_OK) ck_fieldcal_plan_free(plan);
    return ret;
}

void ck_fieldcal_result_start(const ck_rigcal_problem_t *problem, const ck_fieldcal_plan_t *plan, const ck_iso3_t *layout0, int32_t n_layout,
                              ck_fieldcal_result_t *res, ck_iso3_t *layout_out, double *tag_rms) {
    memset(res, 0, sizeof *res);
    res->status = plan->status;
    res->n_steps = problem->n_steps; res->n_steps_used = plan->n_used; res->n_points = plan->n_points;
    res->n_tags_solved = plan->n_solved;
    for (int32_t k = 0; k < n_layout; k++) { layout_out[k] = layout0[k]; tag_rms[k] = 0.0; }
}

void ck_fieldcal_result_finish(const ck_fieldcal_plan_t *plan, const ck_iso3_t *layout0, const double *T, const double *rms,
                               ck_iso3_t *layout_out, double *tag_rms) {
    const ckf_meta_t m = ckf_meta_at(plan->meta, (size_t)plan->n_used, (size_t)plan->n_pairs, (size_t)plan->n_sights, (size_t)plan->n_tags);
    for (int32_t k = 0; k < plan->n_tags; k++) {
        const int32_t li = m.ltag[k];
        const unsigned m6 = (unsigned)m.mask6[k];
        ck_iso3_t *o = layout_out + li;
        *o = layout0[li];
        tag_rms[li] = rms[k];
        if (m6 == 63u) continue;
        if ((m6 & 7u) != 7u) ck_rigcal_mat_to_quat(T + 12 * (size_t)k, o->q);
        for (int i = 0; i < 3; i++)
            if (!((m6 >> (3 + i)) & 1u)) o->t[i] = T[12 * (size_t)k + 9 + i];
    }
}

int ck_fieldcal_jacobian(const ck_iso3_t *mount, const double *pose, const ck_iso3_t *tag, const double *bearings, int32_t n,
                         uint32_t fixed6, double *r_out, double *J_out) {
    if (!mount || !pose || !tag || !bearings || !r_out || !J_out || n < 0 || n > 4) return CK_EINVAL;
    double M[12], T[12];
    ck_rigcal_mount_in(mount, M);
    ck_fieldcal_tag_in(tag, T);
    for (int32_t i = 0; i < n; i++) ckf_jacobian(M, pose, T, i, bearings + 3 * (size_t)i, fixed6 & 63u, r_out + 3 * (size_t)i, J_out + 3 * CKA_NJ * (size_t)i);
    return CK_OK;
}

/* ---- the twin ---------------------------------------------------------------------------------------------------------------- */
typedef struct {
    ckf_meta_t m;
    int U, P, NS, T;
    const double *bear, *M;
    double *st, *pr, *si;
} twin_t;

/* the candidate's cost: per sighting by lanes and the butterfly 2, 1 as its lane 0 sees it, per step its pairs, then the steps in order */
static double twin_cost(twin_t *W, const double *Tc) {
    for (int g = 0; g < W->NS; g++) {
        const int pi = W->m.sight_pair[g];
        const double *T = Tc + 12 * (size_t)W->m.ix.col[pi], *P = W->st + (size_t)CKA_S_STRIDE * W->m.ix.step[pi] + CKA_S_CAND;
        double a[CKF_GROUP];
        for (int l = 0; l < CKF_GROUP; l++) {
            double e[3];
            ckf_residual(W->M + 12 * W->m.sight_cam[g], P, T, l, W->bear + 3 * ((size_t)W->m.sight_bear[g] + l), e);
            a[l] = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
        }
        W->si[(size_t)CKF_I_STRIDE * g + CKF_I_COST] = (a[0] + a[2]) + (a[1] + a[3]);
    }
    double t = 0.0;
    for (int u = 0; u < W->U; u++) {
        const int p0 = W->m.ix.first[u];
        double *st = W->st + (size_t)CKA_S_STRIDE * u;
        ckf_step_cost(st, W->pr + (size_t)CKA_B_STRIDE * p0, W->si + (size_t)CKF_I_STRIDE * W->m.pair_sight[p0], W->m.pair_sight + p0,
                      W->m.ix.first[u + 1] - p0);
        t = t + st[CKA_S_COST];
    }
    return t;
}

static void twin_jacobian(twin_t *W, const double *Tm) {
    for (int g = 0; g < W->NS; g++) {
        const int pi = W->m.sight_pair[g], k = W->m.ix.col[pi];
        const double *P = W->st + (size_t)CKA_S_STRIDE * W->m.ix.step[pi] + CKA_S_POSE;
        double part[CKF_GROUP][CKA_NACC];
        for (int l = 0; l < CKF_GROUP; l++) {
            double e[3], J[3 * CKA_NJ];
            for (int j = 0; j < CKA_NACC; j++) part[l][j] = 0.0;
            ckf_jacobian(W->M + 12 * W->m.sight_cam[g], P, Tm + 12 * (size_t)k, l, W->bear + 3 * ((size_t)W->m.sight_bear[g] + l),
                         (unsigned)W->m.mask6[k], e, J);
            ckr_accumulate_rows(part[l], part[l] + CKA_NH, e, J, 0, CKA_NJ);
        }
        for (int j = 0; j < CKA_NACC; j++) W->si[(size_t)CKF_I_STRIDE * g + CKF_I_H + j] = (part[0][j] + part[2][j]) + (part[1][j] + part[3][j]);
    }
    for (int pi = 0; pi < W->P; pi++)
        ckf_pair_sum(W->pr + (size_t)CKA_B_STRIDE * pi, W->si + (size_t)CKF_I_STRIDE * W->m.pair_sight[pi], W->m.pair_sight[pi + 1] - W->m.pair_sight[pi]);
}

static void accept_costs(twin_t *W) {
    for (int pi = 0; pi < W->P; pi++) W->pr[(size_t)CKA_B_STRIDE * pi + CKA_B_COSTA] = W->pr[(size_t)CKA_B_STRIDE * pi + CKA_B_COST];
}

/* The reduced system S (packed lower triangle, CKF_LT) d = rhs, in place in dk.  Left-looking column Cholesky: entry (i, j) subtracts
 * L[i][c] L[j][c] for c = 0 .. j - 1 in increasing c and is divided by the pivot's root; the first pivot that is not positive ends it
 * (0).  Forward substitution subtracts L[i][c] y[c] in increasing c, backward substitution L[c][i] x[c] in DEcreasing c from N - 1:
 * the order in which the kernel's column sweeps reach a row. */
static int reduced_solve(double *S, int N, double *dk) {
    for (int j = 0; j < N; j++) {
        double t = S[CKF_LT(j, j)];
        for (int c = 0; c < j; c++) t = t - S[CKF_LT(j, c)] * S[CKF_LT(j, c)];
        if (!(t > 0.0)) return 0;
        const double d = sqrt(t);
        S[CKF_LT(j, j)] = d;
        for (int i = j + 1; i < N; i++) {
            double w = S[CKF_LT(i, j)];
            for (int c = 0; c < j; c++) w = w - S[CKF_LT(i, c)] * S[CKF_LT(j, c)];
            S[CKF_LT(i, j)] = w / d;
        }
    }
    for (int i = 0; i < N; i++) {
        double t = dk[i];
        for (int c = 0; c < i; c++) t = t - S[CKF_LT(i, c)] * dk[c];
        dk[i] = t / S[CKF_LT(i, i)];
    }
    for (int i = N - 1; i >= 0; i--) {
        double t = dk[i];
        for (int c = N - 1; c > i; c--) t = t - S[CKF_LT(c, i)] * dk[c];
        dk[i] = t / S[CKF_LT(i, i)];
    }
    return 1;
}

int ck_fieldcal_refine_host(const ck_fieldcal_params_t *p, int32_t n_cams, const ck_sqpnp_problem_t *records, int32_t n_steps,
                            const int32_t *tag_index, int32_t n_tags_total, const double *bearings, int32_t n_bearings_total,
                            const ck_rigcal_problem_t *problem, const int32_t *step_index, int32_t n_index_total, const ck_iso3_t *mounts,
                            const ck_iso3_t *layout0, int32_t n_layout, const uint8_t *fixed6, const double *poses0,
                            ck_fieldcal_result_t *res, ck_iso3_t *layout_out, int32_t *tag_sightings, double *tag_rms, double *poses_out) {
    if (!poses0 || !res || !layout_out || !tag_sightings || !tag_rms || !poses_out) return CK_EINVAL;
    const int rc = ck_fieldcal_check(p, n_cams, records, n_steps, tag_index, n_tags_total, bearings, n_bearings_total, problem, 1, step_index,
                                     n_index_total, mounts, layout0, n_layout, fixed6);
    if (rc != CK_OK) return rc;
    ck_fieldcal_plan_t plan;
    int ret = ck_fieldcal_plan(p, n_cams, records, n_steps, tag_index, problem, step_index, n_layout, fixed6, poses0, tag_sightings, &plan);
    if (ret != CK_OK) return ret;
    ck_fieldcal_result_start(problem, &plan, layout0, n_layout, res, layout_out, tag_rms);
    ck_cal_poses_start(problem, step_index, poses0, poses_out);
    if (plan.status == CK_CALIB_DEGENERATE) { ck_fieldcal_plan_free(&plan); return CK_OK; }
    twin_t W;
    memset(&W, 0, sizeof W);
    W.U = plan.n_used; W.P = plan.n_pairs; W.NS = plan.n_sights; W.T = plan.n_tags;
    W.m = ckf_meta_at(plan.meta, (size_t)W.U, (size_t)W.P, (size_t)W.NS, (size_t)W.T);
    W.bear = bearings;
    const int N = 6 * W.T;
    double M[12 * CK_RIG_MAX_CAMS];
    double *Tm = (double *)calloc((size_t)24 * (size_t)W.T + (size_t)CKA_HK * W.T + 2 * (size_t)N + CKF_LT(N, 0) + 1, sizeof(double));
    W.st = (double *)calloc((size_t)CKA_S_STRIDE * (size_t)W.U + 1, sizeof(double));
    W.pr = (double *)calloc((size_t)CKA_B_STRIDE * (size_t)W.P + 1, sizeof(double));
    W.si = (double *)calloc((size_t)CKF_I_STRIDE * (size_t)W.NS + 1, sizeof(double));
    int32_t *shared = (int32_t *)malloc(sizeof(int32_t) * ((size_t)W.U + 1));
    ret = CK_ENOMEM;
    if (!Tm || !W.st || !W.pr || !W.si || !shared) goto done;
    ret = CK_OK;
    {
        double *Tc = Tm + 12 * (size_t)W.T, *Hk = Tc + 12 * (size_t)W.T, *dk = Hk + (size_t)CKA_HK * W.T, *rms = dk + N, *S = rms + N;
        for (int c = 0; c < n_cams; c++) ck_rigcal_mount_in(mounts + c, M + 12 * c);
        W.M = M;
        for (int k = 0; k < W.T; k++) ck_fieldcal_tag_in(layout0 + W.m.ltag[k], Tm + 12 * (size_t)k);
        memcpy(Tc, Tm, sizeof(double) * 12 * (size_t)W.T);
        ck_cal_steps_seed(W.st, W.m.ix.used, W.U, poses0);
        const double cost0 = twin_cost(&W, Tc);
        accept_costs(&W);
        res->status = CK_CALIB_DEGENERATE;
        if (!ckc_finite(cost0)) goto done;
        ckc_lm_t lm;
        ckc_lm_start(&lm, cost0, CKR_COST_FLOOR);
        while (lm.status < 0) {
            if (lm.need_jac) {
                twin_jacobian(&W, Tm);
                for (int k = 0; k < W.T; k++)
                    for (int j = 0; j < CKA_HK; j++) Hk[CKA_HK * k + j] = cka_col_sum(W.pr, W.m.ix.colmap + (size_t)k * W.U, W.U, j);
            }
            int solved = 1;
            for (int u = 0; u < W.U; u++)
                if (!cka_step_schur(W.st + (size_t)CKA_S_STRIDE * u, W.pr + (size_t)CKA_B_STRIDE * W.m.ix.first[u],
                                    W.m.ix.first[u + 1] - W.m.ix.first[u], lm.lambda))
                    solved = 0;
            for (int tr = 0; tr < W.T; tr++)
                for (int tk = 0; tk <= tr; tk++) { /* the steps that see both tags, once for the block's entries */
                    int ns = 0;
                    for (int u = 0; u < W.U; u++)
                        if (W.m.ix.colmap[(size_t)tr * W.U + u] >= 0 && W.m.ix.colmap[(size_t)tk * W.U + u] >= 0) shared[ns++] = u;
                    for (int r = 6 * tr; r < 6 * tr + 6; r++)
                        for (int k = 6 * tk; k < 6 * tk + 6 && k <= r; k++)
                            S[CKF_LT(r, k)] = cka_reduced_entry(W.pr, W.m.ix.colmap, W.m.mask6, Hk, W.U, shared, ns, lm.lambda, r, k);
                }
            for (int r = 0; r < N; r++) dk[r] = cka_reduced_rhs(W.pr, W.m.ix.colmap, W.m.mask6, Hk, W.U, r);
            double pred = 0.0, cost_new = 0.0;
            if (!reduced_solve(S, N, dk)) solved = 0;
            if (solved) {
                pred = cka_reduced_pred(W.m.mask6, Hk, N, lm.lambda, dk);
                for (int k = 0; k < W.T; k++) ckc_rigid_step(Tm + 12 * (size_t)k, dk + 6 * k, (unsigned)W.m.mask6[k], Tc + 12 * (size_t)k);
                for (int u = 0; u < W.U; u++)
                    cka_step_step(W.st + (size_t)CKA_S_STRIDE * u, W.pr + (size_t)CKA_B_STRIDE * W.m.ix.first[u], W.m.ix.col + W.m.ix.first[u],
                                  W.m.ix.first[u + 1] - W.m.ix.first[u], dk, lm.lambda);
                for (int u = 0; u < W.U; u++) pred = pred + W.st[(size_t)CKA_S_STRIDE * u + CKA_S_PRED];
                cost_new = twin_cost(&W, Tc);
            }
            if (ckc_lm_decide(&lm, solved, pred, cost_new, p->max_iters, CKR_COST_FLOOR)) {
                memcpy(Tm, Tc, sizeof(double) * 12 * (size_t)W.T);
                for (int u = 0; u < W.U; u++)
                    memcpy(W.st + (size_t)CKA_S_STRIDE * u + CKA_S_POSE, W.st + (size_t)CKA_S_STRIDE * u + CKA_S_CAND, sizeof(double) * 12);
                accept_costs(&W);
            }
        }
        ck_cal_poses_finish(problem, step_index, W.m.ix.used, W.U, W.st, poses_out);
        for (int k = 0; k < W.T; k++) rms[k] = cka_col_rms(W.pr, W.m.ix.colmap + (size_t)k * W.U, W.U, 4 * W.m.tag_ns[k]);
        ck_fieldcal_result_finish(&plan, layout0, Tm, rms, layout_out, tag_rms);
        res->status = lm.status; res->iters = lm.iters;
        res->cost0 = cost0; res->cost = lm.cost;
        res->rms = sqrt(lm.cost / (double)res->n_points);
    }
done:
    free(Tm); free(W.st); free(W.pr); free(W.si); free(shared);
    ck_fieldcal_plan_free(&plan);
    return ret;
}
