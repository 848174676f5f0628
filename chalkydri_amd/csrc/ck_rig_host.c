/* ck_rig_host.c — the rig solver on the host, one thread, plain C: the specification of k_rig and k_rig_robust (k_rigpnp.hip) and what
 * the CPU suite tests the arithmetic with.  DESIGN.md §4k has the formulas.  What one lane computes alone is ck_pose_math.h's, the text
 * the kernels compile: the 3x3 algebra up to the nearest rotation, a point's world position, ray and residual, the translation of an r,
 * the GNC weight, the standard deviations, the yaw pivot.  What the kernels spread over lanes is spelled out here a second time, in the
 * order of the device code: the sums over cameras in index order and points in index order (rig_system), the 9x9 Jacobi (jacobi9), the
 * 15x15 elimination of the SQP step (lu_solve15, optimization), the choice among the candidates.  So the two agree to round-off of the
 * transcendental functions alone.  No device, no HIP header. */
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "ck_pose_math.h"
#include "ck_rig_c.h"

/* cyclic Jacobi of a symmetric 9x9 (destroyed), row-major; the columns of V are the eigenvectors.  Stop rule, sweep order and
 * rotation formulas are jacobi3's (ck_pose_math.h) and jacobi9_wave's (ck_sqpnp_dev.h). */
static void jacobi9(double *A, double *V, double *w) {
    const int n = 9;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) V[i * n + j] = (i == j);
    double tot = 0;
    for (int i = 0; i < n * n; i++) tot += A[i] * A[i];
    const double stop = 1e-32 * tot;
    for (int sweep = 0; sweep < 64; sweep++) {
        double off = 0;
        for (int i = 0; i < n; i++)
            for (int j = i + 1; j < n; j++) off += A[i * n + j] * A[i * n + j];
        if (off <= stop) break;
        for (int p = 0; p < n; p++)
            for (int q = p + 1; q < n; q++) {
                double apq = A[p * n + q];
                if (fabs(apq) < 1e-300) continue;
                double app = A[p * n + p], aqq = A[q * n + q];
                double theta = (aqq - app) / (2.0 * apq);
                double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; k++) { double akp = A[k * n + p], akq = A[k * n + q]; A[k * n + p] = c * akp - s * akq; A[k * n + q] = s * akp + c * akq; }
                for (int k = 0; k < n; k++) { double apk = A[p * n + k], aqk = A[q * n + k]; A[p * n + k] = c * apk - s * aqk; A[q * n + k] = s * apk + c * aqk; }
                for (int k = 0; k < n; k++) { double vkp = V[k * n + p], vkq = V[k * n + q]; V[k * n + p] = c * vkp - s * vkq; V[k * n + q] = s * vkp + c * vkq; }
            }
    }
    for (int i = 0; i < n; i++) w[i] = A[i * n + i];
}

/* 15x15 LU with partial pivoting (first maximum of a column); 0 when a pivot is exactly zero */
static int lu_solve15(double *A, double *b) {
    const int n = 15;
    for (int col = 0; col < n; col++) {
        int piv = col;
        double best = fabs(A[col * n + col]);
        for (int r = col + 1; r < n; r++)
            if (fabs(A[r * n + col]) > best) { best = fabs(A[r * n + col]); piv = r; }
        if (best == 0.0) return 0;
        if (piv != col) {
            for (int k = 0; k < n; k++) { double t = A[col * n + k]; A[col * n + k] = A[piv * n + k]; A[piv * n + k] = t; }
            double t = b[col]; b[col] = b[piv]; b[piv] = t;
        }
        for (int r = col + 1; r < n; r++) {
            double f = A[r * n + col] / A[col * n + col];
            if (f == 0.0) continue;
            for (int k = col; k < n; k++) A[r * n + k] -= f * A[col * n + k];
            b[r] -= f * b[col];
        }
    }
    for (int r = n - 1; r >= 0; r--) {
        double s = b[r];
        for (int k = r + 1; k < n; k++) s -= A[r * n + k] * b[k];
        b[r] = s / A[r * n + r];
    }
    return 1;
}

/* SQP refinement of one start: the KKT step [[Omega, J^T], [J, 0]] [d; lambda] = [-(Omega r - g); -h].  Returns r^T Omega r. */
static double optimization(int max_iter, double tol_sq, double r[9], const double omega[81], const double g[9]) {
    for (int it = 0; it < max_iter; it++) {
        const double *c1 = r, *c2 = r + 3, *c3 = r + 6;
        double h[6], J[54], lhs[225], rhs[15];
        h[0] = c1[0] * c1[0] + c1[1] * c1[1] + c1[2] * c1[2] - 1.0;
        h[1] = c2[0] * c2[0] + c2[1] * c2[1] + c2[2] * c2[2] - 1.0;
        h[2] = c3[0] * c3[0] + c3[1] * c3[1] + c3[2] * c3[2] - 1.0;
        h[3] = c1[0] * c2[0] + c1[1] * c2[1] + c1[2] * c2[2];
        h[4] = c1[0] * c3[0] + c1[1] * c3[1] + c1[2] * c3[2];
        h[5] = c2[0] * c3[0] + c2[1] * c3[1] + c2[2] * c3[2];
        memset(J, 0, sizeof J);
        for (int k = 0; k < 3; k++) {
            J[0 * 9 + k] = 2.0 * c1[k]; J[1 * 9 + 3 + k] = 2.0 * c2[k]; J[2 * 9 + 6 + k] = 2.0 * c3[k];
            J[3 * 9 + k] = c2[k]; J[3 * 9 + 3 + k] = c1[k];
            J[4 * 9 + k] = c3[k]; J[4 * 9 + 6 + k] = c1[k];
            J[5 * 9 + 3 + k] = c3[k]; J[5 * 9 + 6 + k] = c2[k];
        }
        memset(lhs, 0, sizeof lhs);
        for (int i = 0; i < 9; i++)
            for (int j = 0; j < 9; j++) lhs[i * 15 + j] = omega[i * 9 + j];
        for (int i = 0; i < 6; i++)
            for (int j = 0; j < 9; j++) { lhs[j * 15 + 9 + i] = J[i * 9 + j]; lhs[(9 + i) * 15 + j] = J[i * 9 + j]; }
        for (int i = 0; i < 9; i++) {
            double s = 0;
            for (int j = 0; j < 9; j++) s += omega[i * 9 + j] * r[j];
            rhs[i] = -(s - g[i]);
        }
        for (int i = 0; i < 6; i++) rhs[9 + i] = -h[i];
        if (!lu_solve15(lhs, rhs)) break;
        double n2 = 0;
        for (int k = 0; k < 9; k++) { r[k] += rhs[k]; n2 += rhs[k] * rhs[k]; }
        if (n2 < tol_sq) break;
    }
    double e = 0;
    for (int i = 0; i < 9; i++) {
        double s = 0;
        for (int j = 0; j < 9; j++) s += omega[i * 9 + j] * r[j];
        e += r[i] * s;
    }
    return e;
}
/* E(r) = r^T Omega r - 2 g^T r + c, from r^T Omega r */
static double full_energy(double rOr, const double r[9], const double g[9], double c) {
    double gr = 0;
    for (int k = 0; k < 9; k++) gr += g[k] * r[k];
    return (rOr - 2.0 * gr) + c;
}

/* ck_rig_c.h */
int ck_rig_check(const ck_rig_params_t *params, int32_t n_cams, const ck_sqpnp_problem_t *problems, int32_t n, const void *tags,
                 int32_t n_tags_total, const void *bearings, int32_t n_bearings_total, const void *gyro, const void *out,
                 int32_t *max_points) {
    if (!params || !problems || !gyro || !out || n < 0 || n_cams < 1 || n_cams > CK_RIG_MAX_CAMS || n_tags_total < 0 ||
        n_bearings_total < 0 || (n_tags_total > 0 && !tags) || (n_bearings_total > 0 && !bearings)) return CK_EINVAL;
    int32_t most = 0;
    for (int s = 0; s < n; s++) {
        int64_t pts = 0;
        for (int c = 0; c < n_cams; c++) {
            const ck_sqpnp_problem_t *p = &problems[(size_t)c * (size_t)n + (size_t)s];
            if (p->n_tags < 0 || p->n_bearings < 0 || p->tag_offset < 0 || p->bearing_offset < 0 ||
                (int64_t)p->tag_offset + p->n_tags > n_tags_total || (int64_t)p->bearing_offset + p->n_bearings > n_bearings_total ||
                (int64_t)4 * p->n_tags != p->n_bearings) return CK_EINVAL;
            pts += p->n_bearings;
        }
        if (pts > 0x3FFFFFFF) return CK_EINVAL;
        if (pts > most) most = (int32_t)pts;
    }
    if (max_points) *max_points = most;
    return CK_OK;
}

/* One step's cameras and points.  A tag weight array `w` (one per tag, the tags numbered camera-major, then by the record's index;
 * null: every tag counts once) runs through the pieces below: the plain solve is the pieces with w = null, the robust solve
 *  the same pieces with the weights of its rounds.  A point of weight 0 is skipped, a weight of 1 multiplies exactly. */
typedef struct {
    int n_cams, N;
    double A[CK_RIG_MAX_CAMS][9], b[CK_RIG_MAX_CAMS][3], o[CK_RIG_MAX_CAMS][3];
    int base[CK_RIG_MAX_CAMS + 1];
    const ck_iso3_t *tg[CK_RIG_MAX_CAMS];
    double *world, *dir;
    int *cam_of;
} rig_step_t;
typedef struct {
    double centroid[3], Qrr[81], Qrt[27], qt[3], QttInv[9], omega[81], g[9], cc, S[9];
} rig_sys_t;

static double tag_weight(const double *w, int point) { return w ? w[point >> 2] : 1.0; }

static void rig_prepare(rig_step_t *st, int n_cams, const ck_sqpnp_problem_t *problems, int n, int step, const ck_iso3_t *tags,
                        const double *bearings, double *world, double *dir, int *cam_of) {
    st->n_cams = n_cams; st->world = world; st->dir = dir; st->cam_of = cam_of;
    st->base[0] = 0;
    for (int c = 0; c < n_cams; c++) {
        const ck_sqpnp_problem_t *p = &problems[(size_t)c * (size_t)n + (size_t)step];
        quat_to_mat(p->robot_to_cam.q, st->A[c]);
        for (int k = 0; k < 3; k++) st->b[c][k] = p->robot_to_cam.t[k];
        ckp_camera_origin(st->A[c], st->b[c], st->o[c]);
        st->base[c + 1] = st->base[c] + 4 * p->n_tags;
        st->tg[c] = tags + p->tag_offset;
    }
    st->N = st->base[n_cams];
    for (int c = 0; c < n_cams; c++) {
        const ck_sqpnp_problem_t *p = &problems[(size_t)c * (size_t)n + (size_t)step];
        const ck_iso3_t *tg = st->tg[c];
        const double *v = bearings + (size_t)3 * (size_t)p->bearing_offset;
        for (int j = 0; j < 4 * p->n_tags; j++) {
            const int i = st->base[c] + j, t = j >> 2;
            double R[9];
            quat_to_mat(tg[t].q, R);
            ckp_tag_corner(R, tg[t].t, j & 3, world + i * 3);
            ckp_ray(st->A[c], v + 3 * j, dir + i * 3);
            cam_of[i] = c;
        }
    }
}

/* the accumulated entries, centred on the (weighted) centroid, and Omega, g, c */
static void rig_system(const rig_step_t *st, const double *w, rig_sys_t *y) {
    const int N = st->N;
    const double *world = st->world, *dir = st->dir;
    for (int k = 0; k < 3; k++) {
        double s = 0, sw = 0;
        for (int i = 0; i < N; i++) {
            const double wi = tag_weight(w, i);
            if (wi == 0.0) continue;
            s += wi * world[i * 3 + k];
            sw += wi;
        }
        y->centroid[k] = s / sw;
    }
    double *Qrr = y->Qrr, *Qrt = y->Qrt, Qtt[9], qr[9], *qt = y->qt, q0 = 0, *S = y->S;
    memset(Qrr, 0, sizeof y->Qrr); memset(Qrt, 0, sizeof y->Qrt); memset(Qtt, 0, sizeof Qtt); memset(qr, 0, sizeof qr); memset(qt, 0, sizeof y->qt);
    memset(S, 0, sizeof y->S);
    for (int k = 0; k < N; k++) {
        const double wk = tag_weight(w, k);
        if (wk == 0.0) continue;
        const double *u = dir + 3 * k, *oc = st->o[st->cam_of[k]];
        const double X[3] = {world[k * 3] - y->centroid[0], world[k * 3 + 1] - y->centroid[1], world[k * 3 + 2] - y->centroid[2]};
        const double sq = u[0] * u[0] + u[1] * u[1] + u[2] * u[2], inv = 1.0 / sq;
        double P[9], Mo[3];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) P[i * 3 + j] = (i == j ? 1.0 : 0.0) - (u[i] * u[j]) * inv;
        for (int i = 0; i < 3; i++) Mo[i] = P[i * 3] * oc[0] + P[i * 3 + 1] * oc[1] + P[i * 3 + 2] * oc[2];
        for (int i = 0; i < 9; i++) Qtt[i] += wk * P[i];
        for (int a = 0; a < 3; a++) {
            for (int i = 0; i < 3; i++) {
                for (int j = 0; j < 3; j++) Qrt[(3 * a + i) * 3 + j] += wk * (P[i * 3 + j] * X[a]);
                qr[3 * a + i] += wk * (X[a] * Mo[i]);
            }
            for (int bb = 0; bb < 3; bb++)
                for (int i = 0; i < 3; i++)
                    for (int j = 0; j < 3; j++) Qrr[(3 * a + i) * 9 + 3 * bb + j] += wk * ((P[i * 3 + j] * X[a]) * X[bb]);
        }
        for (int i = 0; i < 3; i++) qt[i] += wk * Mo[i];
        q0 += wk * (oc[0] * Mo[0] + oc[1] * Mo[1] + oc[2] * Mo[2]);
        for (int i = 0; i < 3; i++)
            for (int j = i; j < 3; j++) S[i * 3 + j] += wk * (X[i] * X[j]); /* scatter of the centred points (upper triangle) */
    }
    double *QttInv = y->QttInv, *omega = y->omega, *g = y->g;
    if (!mat3_try_inverse(Qtt, QttInv)) memset(QttInv, 0, sizeof y->QttInv);
    for (int i = 0; i < 9; i++) {
        const double t0 = Qrt[i * 3] * QttInv[0] + Qrt[i * 3 + 1] * QttInv[3] + Qrt[i * 3 + 2] * QttInv[6];
        const double t1 = Qrt[i * 3] * QttInv[1] + Qrt[i * 3 + 1] * QttInv[4] + Qrt[i * 3 + 2] * QttInv[7];
        const double t2 = Qrt[i * 3] * QttInv[2] + Qrt[i * 3 + 1] * QttInv[5] + Qrt[i * 3 + 2] * QttInv[8];
        for (int j = 0; j < 9; j++) omega[i * 9 + j] = Qrr[i * 9 + j] - (t0 * Qrt[j * 3] + t1 * Qrt[j * 3 + 1] + t2 * Qrt[j * 3 + 2]);
        g[i] = qr[i] - (t0 * qt[0] + t1 * qt[1] + t2 * qt[2]);
    }
    {
        double ww[3];
        mat3_vec(QttInv, qt, ww);
        y->cc = q0 - (qt[0] * ww[0] + qt[1] * ww[1] + qt[2] * ww[2]);
    }
}

/* the six starts, refined, and their order by penalised energy */
static void rig_starts(const ck_rig_params_t *prm, rig_sys_t *y, double gyro, double candR[6][9], double candE[6], int order[6]) {
    const double *omega = y->omega, *g = y->g, *Qrr = y->Qrr;
    double *S = y->S;
    double Aw[81], V[81], ev[9];
    memcpy(Aw, omega, sizeof Aw);
    {   /* Coplanar points (one tag; tags on one wall) with normal n: R n is free, Omega has the exact null space {vec(a n^T)} and its
         * "three smallest eigenvectors" would be an arbitrary basis of it that says nothing about the pose.  The eigenvectors are then
         * taken on the complement: mu * sum_k v_k v_k^T, v_k = vec(e_k n^T), mu = trace(Q_rr) >= every eigenvalue of Omega, moves
         * that space to the top of the spectrum.  The refinement keeps Omega itself. */
        double Sw[9], Sv[9], sw[3];
        S[3] = S[1]; S[6] = S[2]; S[7] = S[5];
        memcpy(Sw, S, sizeof Sw);
        jacobi3(Sw, Sv, sw);
        int k = 0;
        double wmin = sw[0], wmax = sw[0];
        if (sw[1] < wmin) { wmin = sw[1]; k = 1; }
        if (sw[2] < wmin) { wmin = sw[2]; k = 2; }
        if (sw[1] > wmax) wmax = sw[1];
        if (sw[2] > wmax) wmax = sw[2];
        if (wmin <= CK_RIG_PLANAR_EPS * wmax) {
            const double nrm[3] = {Sv[k], Sv[3 + k], Sv[6 + k]};
            double mu = 0;
            for (int i = 0; i < 9; i++) mu += Qrr[i * 9 + i];
            for (int i = 0; i < 9; i++)
                for (int j = 0; j < 9; j++)
                    if (i % 3 == j % 3) Aw[i * 9 + j] += mu * (nrm[i / 3] * nrm[j / 3]);
        }
    }
    jacobi9(Aw, V, ev);
    int idx[9] = {0, 1, 2, 3, 4, 5, 6, 7, 8};
    for (int i = 1; i < 9; i++) { /* stable ascending order of the eigenvalues */
        int v = idx[i], j = i - 1;
        while (j >= 0 && ev[idx[j]] > ev[v]) { idx[j + 1] = idx[j]; j--; }
        idx[j + 1] = v;
    }
    const double gc = cos(gyro), gs = sin(gyro);
    for (int q = 0; q < 6; q++) {
        const int t = q >> 1;
        const double sign = (q & 1) ? 1.0 : -1.0;
        double guess[9], *r = candR[q];
        for (int k = 0; k < 9; k++) guess[k] = V[k * 9 + idx[t]] * sign;
        nearest_so3(guess, r);
        double energy = full_energy(optimization(prm->sqpnp.max_iter, prm->sqpnp.tol_sq, r, omega, g), r, g, y->cc);
        double dot = r[0] * gc + r[3] * gs; /* the robot's forward axis in the world is row 0 of R */
        double ae = 1.0 - dot;
        if (ae < 0.0) ae = 0.0;
        candE[q] = energy + prm->sign_change_error * ae;
    }
    for (int i = 0; i < 6; i++) order[i] = i;
    for (int i = 1; i < 6; i++) { /* stable sort by penalised energy */
        int v = order[i], j = i - 1;
        while (j >= 0 && candE[order[j]] > candE[v]) { order[j + 1] = order[j]; j--; }
        order[j + 1] = v;
    }
}

/* R (row-major) of r (column-major) and the t that goes with it */
static void rig_translation(const rig_sys_t *y, const double r[9], double Rm[9], double t[3]) {
    ckp_translation(y->Qrt, y->qt, y->QttInv, y->centroid, r, Rm, t);
}

/* the cheapest candidate with every point (of a weight other than 0) in front of its own camera */
static int rig_pick(const rig_step_t *st, const rig_sys_t *y, const double *w, double candR[6][9], const double candE[6], const int order[6],
                    double bestRm[9], double bestT[3]) {
    int found = 0;
    double best_score = DBL_MAX;
    for (int oi = 0; oi < 6; oi++) {
        double Rm[9], t[3];
        rig_translation(y, candR[order[oi]], Rm, t);
        int behind = 0;
        for (int i = 0; i < st->N; i++) {
            if (tag_weight(w, i) == 0.0) continue;
            const int c = st->cam_of[i];
            double pr[3];
            mat3_vec(Rm, st->world + 3 * i, pr);
            for (int k = 0; k < 3; k++) pr[k] += t[k];
            if (!((st->A[c][6] * pr[0] + st->A[c][7] * pr[1] + st->A[c][8] * pr[2]) + st->b[c][2] > 0.0)) behind = 1;
        }
        if (behind) continue;
        if (candE[order[oi]] < best_score) {
            best_score = candE[order[oi]];
            memcpy(bestRm, Rm, sizeof Rm);
            memcpy(bestT, t, sizeof t);
            found = 1;
        }
    }
    return found;
}

/* the record of the chosen candidate; bestR = polar(bestRm) comes back too */
static void rig_finish(const rig_step_t *st, const double *w, const double bestRm[9], const double bestT[3], double gyro, double bestR[9],
                       ck_rig_result_t *out) {
    /* The pose that is returned: R^ = polar(R), the rotation next to the refinement's last iterate (which meets the constraints to
     * round-off only), and t.  Per camera: its tags and the RMS point-to-ray distance of its own points at that pose.  The squared
     * distances, summed per camera and then over the cameras, are E again, without the cancellation of the quadratic form (terms
     * of the size of |o|^2 * points against a sum of noise^2) and, taken ON the constraint manifold, without the first-order
     * sensitivity to how far off it the iterate ended: that sum is the energy the record and the standard deviations carry. */
    const double *world = st->world, *dir = st->dir;
    int total_tags = 0;
    double best_energy = 0, tc[3] = {0, 0, 0}; /* tc: sum of the tag centres, cameras and tags in index order */
    polar_rotation(bestRm, bestR);
    for (int c = 0; c < st->n_cams; c++) {
        int cnt = 0;
        for (int i = st->base[c]; i < st->base[c + 1]; i += 4)
            if (tag_weight(w, i) != 0.0) {
                cnt += 4;
                for (int k = 0; k < 3; k++) tc[k] += st->tg[c][(i - st->base[c]) >> 2].t[k];
            }
        out->cam_tags[c] = cnt / 4;
        total_tags += cnt / 4;
        if (!cnt) continue;
        double s = 0;
        for (int i = st->base[c]; i < st->base[c + 1]; i++) {
            if (tag_weight(w, i) == 0.0) continue;
            double ud, dd;
            s += ckp_ray_residual(bestR, bestT, world + 3 * i, dir + 3 * i, st->o[c], &ud, &dd);
        }
        out->cam_rms[c] = sqrt((s > 0.0 ? s : 0.0) / (double)cnt);
        best_energy += s;
    }
    const double distance = sqrt(bestT[0] * bestT[0] + bestT[1] * bestT[1] + bestT[2] * bestT[2]);
    ckp_std_devs(best_energy > 0.0 ? best_energy : 0.0, total_tags, distance, out->std_devs); /* a round-off negative energy counts as 0 */
    /* world <- robot: rot = polar(R)^T, pos = -rot t; then the yaw pivot about the mean tag centre */
    double robot_rot[9], robot_pos[3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) robot_rot[i * 3 + j] = bestR[j * 3 + i];
    for (int k = 0; k < 3; k++) robot_pos[k] = -(robot_rot[k * 3] * bestT[0] + robot_rot[k * 3 + 1] * bestT[1] + robot_rot[k * 3 + 2] * bestT[2]);
    for (int k = 0; k < 3; k++) tc[k] /= (double)total_tags;
    ckp_yaw_pivot(robot_rot, robot_pos, tc, gyro, out->rot, out->pos, &out->yaw);
    out->energy = best_energy;
    out->n_tags = total_tags;
    out->valid = 1;
}

static void solve_step(const ck_rig_params_t *prm, int n_cams, const ck_sqpnp_problem_t *problems, int n, int step, const ck_iso3_t *tags,
                       const double *bearings, double gyro, double *world, double *dir, int *cam_of, ck_rig_result_t *out) {
    rig_step_t st;
    rig_sys_t y;
    double candR[6][9], candE[6], bestRm[9], bestT[3], bestR[9];
    int order[6];
    memset(out, 0, sizeof *out);
    rig_prepare(&st, n_cams, problems, n, step, tags, bearings, world, dir, cam_of);
    if (st.N < 3) return;
    rig_system(&st, NULL, &y);
    rig_starts(prm, &y, gyro, candR, candE, order);
    if (!rig_pick(&st, &y, NULL, candR, candE, order, bestRm, bestT)) return;
    rig_finish(&st, NULL, bestRm, bestT, gyro, bestR, out);
}

/* ---- the robust solve (chalkydri_hip.h has the arithmetic) ---- */
/* rho of every tag at (R row-major, t): the mean over its corners of the squared sine of the angle between the ray and the point */
static void rig_tag_rho(const rig_step_t *st, const double R[9], const double t[3], double *rho) {
    for (int j = 0; j < st->N / 4; j++) {
        double s = 0;
        for (int i = 4 * j; i < 4 * j + 4; i++) {
            double ud, dd;
            const double pp = ckp_ray_residual(R, t, st->world + 3 * i, st->dir + 3 * i, st->o[st->cam_of[i]], &ud, &dd);
            s += (ud > 0.0 && dd > 0.0) ? pp / dd : 1.0;
        }
        rho[j] = s * 0.25;
    }
}

#define ROBUST_TAGS (CK_RIG_MAX_CAMS * CK_RIG_ROBUST_MAX_TAGS)
static void solve_step_robust(const ck_rig_robust_params_t *rp, int n_cams, const ck_sqpnp_problem_t *problems, int n, int step,
                              const ck_iso3_t *tags, const double *bearings, double gyro, double *world, double *dir, int *cam_of,
                              ck_rig_robust_result_t *out) {
    const ck_rig_params_t *prm = &rp->rig;
    rig_step_t st;
    rig_sys_t y;
    double candR[6][9], candE[6], bestRm[9], bestT[3], bestR[9], Rm[9], t[3], r[9];
    double rho[ROBUST_TAGS], w[ROBUST_TAGS];
    int order[6];
    memset(out, 0, sizeof *out);
    rig_prepare(&st, n_cams, problems, n, step, tags, bearings, world, dir, cam_of);
    if (st.N < 3) return;
    const int nt = st.N / 4;
    const double c = rp->gate_rad, c2 = c * c;
    rig_system(&st, NULL, &y);
    rig_starts(prm, &y, gyro, candR, candE, order);
    int found = rig_pick(&st, &y, NULL, candR, candE, order, bestRm, bestT);
    if (found) {
        for (int cc = 0; cc < 3; cc++)
            for (int rr = 0; rr < 3; rr++) r[cc * 3 + rr] = bestRm[rr * 3 + cc];
        memcpy(Rm, bestRm, sizeof Rm); memcpy(t, bestT, sizeof t);
    } else { /* the cheapest candidate stands in */
        memcpy(r, candR[order[0]], sizeof r);
        rig_translation(&y, r, Rm, t);
    }
    rig_tag_rho(&st, Rm, t, rho);
    double rho_max = rho[0];
    for (int j = 1; j < nt; j++)
        if (rho[j] > rho_max) rho_max = rho[j];
    const double *wf = NULL; /* the weights of the final solve: null when no round ran */
    if (!(rho_max <= c2)) {
        double mu = c2 / (2.0 * rho_max - c2);
        int maxed = 0;
        for (int j = 0; j < nt; j++) w[j] = 1.0;
        for (;;) {
            int binary = 1, same = 1, alive = 0;
            for (int j = 0; j < nt; j++) {
                const double wn = gnc_weight(rho[j], mu, c, c2);
                if (wn != 0.0 && wn != 1.0) binary = 0;
                if (wn != w[j]) same = 0;
                if (wn > 0.0) alive = 1;
                w[j] = wn;
            }
            if ((binary && same) || !alive) break;
            if (out->rounds == rp->max_rounds) { maxed = 1; break; }
            rig_system(&st, w, &y);
            double start[9];
            nearest_so3(r, start);
            memcpy(r, start, sizeof r);
            (void)optimization(prm->sqpnp.max_iter, prm->sqpnp.tol_sq, r, y.omega, y.g);
            rig_translation(&y, r, Rm, t);
            rig_tag_rho(&st, Rm, t, rho);
            mu *= rp->mu_factor;
            out->rounds++;
        }
        int n_in = 0;
        for (int j = 0; j < nt; j++) {
            w[j] = (maxed ? w[j] >= 0.5 : w[j] == 1.0) ? 1.0 : 0.0;
            n_in += w[j] != 0.0;
        }
        for (int cc = 0; cc < n_cams; cc++)
            for (int i = st.base[cc]; i < st.base[cc + 1]; i += 4)
                if (w[i >> 2] == 0.0) out->rejected[cc] |= (uint64_t)1 << ((i - st.base[cc]) >> 2);
        out->n_rejected = nt - n_in;
        out->status = maxed ? CK_RIG_ROBUST_MAXROUNDS : (out->n_rejected ? CK_RIG_ROBUST_REJECTED : CK_RIG_ROBUST_CLEAN);
        if (n_in < rp->min_inlier_tags) { out->status = CK_RIG_ROBUST_NO_CONSENSUS; return; }
        wf = w;
        rig_system(&st, w, &y);
        rig_starts(prm, &y, gyro, candR, candE, order);
        found = rig_pick(&st, &y, w, candR, candE, order, bestRm, bestT);
    } else if (nt < rp->min_inlier_tags) { out->status = CK_RIG_ROBUST_NO_CONSENSUS; return; }
    if (!found) return;
    rig_finish(&st, wf, bestRm, bestT, gyro, bestR, &out->fused);
    rig_tag_rho(&st, bestR, bestT, rho);
    double worst = 0.0, best = DBL_MAX;
    for (int j = 0; j < nt; j++) {
        if (!wf || wf[j] != 0.0) { if (rho[j] > worst) worst = rho[j]; }
        else if (rho[j] < best) best = rho[j];
    }
    out->worst_inlier_rad = sqrt(worst);
    out->best_rejected_rad = out->n_rejected ? sqrt(best) : 0.0;
}

void ck_rig_params_default(ck_rig_params_t *p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->sqpnp.max_iter = 15;
    p->sqpnp.tol_sq = 1e-16;
    p->sign_change_error = 600.0;
    p->rig_id = 255;
}

int ck_rig_solve_host(const ck_rig_params_t *params, int32_t n_cams, const ck_sqpnp_problem_t *problems, int32_t n, const ck_iso3_t *tags,
                      int32_t n_tags_total, const double *bearings, int32_t n_bearings_total, const double *gyro, ck_rig_result_t *out) {
    int32_t max_points = 0;
    const int rc = ck_rig_check(params, n_cams, problems, n, tags, n_tags_total, bearings, n_bearings_total, gyro, out, &max_points);
    if (rc != CK_OK) return rc;
    const size_t cap = max_points > 0 ? (size_t)max_points : 1;
    double *world = (double *)malloc(sizeof(double) * 6 * cap);
    int *cam_of = (int *)malloc(sizeof(int) * cap);
    if (!world || !cam_of) { free(world); free(cam_of); return CK_ENOMEM; }
    for (int s = 0; s < n; s++) solve_step(params, n_cams, problems, n, s, tags, bearings, gyro[s], world, world + 3 * cap, cam_of, &out[s]);
    free(world); free(cam_of);
    return CK_OK;
}

void ck_rig_robust_params_default(ck_rig_robust_params_t *p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    ck_rig_params_default(&p->rig);
    p->gate_rad = 0.01;
    p->mu_factor = 1.4;
    p->max_rounds = 64;
    p->min_inlier_tags = 1;
}

int ck_rig_robust_check(const ck_rig_robust_params_t *params, int32_t n_cams, const ck_sqpnp_problem_t *problems, int32_t n) {
    if (!params) return CK_EINVAL;
    if (!isfinite(params->gate_rad) || !(params->gate_rad > 0.0) || !isfinite(params->mu_factor) || !(params->mu_factor > 1.0) ||
        params->max_rounds < 1 || params->min_inlier_tags < 1) return CK_EINVAL;
    if (problems)
        for (size_t i = 0; i < (size_t)n_cams * (size_t)n; i++)
            if (problems[i].n_tags > CK_RIG_ROBUST_MAX_TAGS) return CK_EINVAL;
    return CK_OK;
}

int ck_rig_solve_robust_host(const ck_rig_robust_params_t *params, int32_t n_cams, const ck_sqpnp_problem_t *problems, int32_t n,
                             const ck_iso3_t *tags, int32_t n_tags_total, const double *bearings, int32_t n_bearings_total,
                             const double *gyro, ck_rig_robust_result_t *out) {
    int32_t max_points = 0;
    if (!params) return CK_EINVAL;
    int rc = ck_rig_check(&params->rig, n_cams, problems, n, tags, n_tags_total, bearings, n_bearings_total, gyro, out, &max_points);
    if (rc != CK_OK) return rc;
    if ((rc = ck_rig_robust_check(params, n_cams, problems, n)) != CK_OK) return rc;
    const size_t cap = max_points > 0 ? (size_t)max_points : 1;
    double *world = (double *)malloc(sizeof(double) * 6 * cap);
    int *cam_of = (int *)malloc(sizeof(int) * cap);
    if (!world || !cam_of) { free(world); free(cam_of); return CK_ENOMEM; }
    for (int s = 0; s < n; s++)
        solve_step_robust(params, n_cams, problems, n, s, tags, bearings, gyro[s], world, world + 3 * cap, cam_of, &out[s]);
    free(world); free(cam_of);
    return CK_OK;
}
