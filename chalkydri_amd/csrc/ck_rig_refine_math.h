// ck_rig_refine_math.h — the refinement of one instant's robot pose and its covariance: the whole solve, written once
// and compiled twice, as C into the host twin (ck_rig_refine_host.c) and as device code into k_rig_refine.hip, -ffp-contract=off on both
// sides.  Only + - * / sqrt on doubles, every expression evaluated as written, so the two return the same bytes.  The residual and the
// pose's Jacobian columns are cka_point's (ck_cal_math.h), the damping and the stop rules ckc_lm_*, the small solves ckc_chol / ckc_fwd /
// ckc_bwd, the pose update ckc_rigid_step (ck_calib_math.h).  What differs between the two sides is only who walks the points: the three
// walkers ckf_walk_* are declared here and defined by the file that includes this one.
//
// A pose P is 12 doubles, world -> robot: p_robot = R X + t, R row-major then t.  A mount M is 12 doubles, A row-major then o: p_cam =
// A (p_robot - o).  A POINT RECORD is CKF_PT doubles: world point X [3], bearing v [3], mount [12], camera number; record j of point i
// lies at pts[j * stride + i].  The used points of an instant are numbered camera-major, then by the tag's index in the camera's
// record, then by corner, the deleted tags left out: a deleted tag leaves no trace in the numbering.
// SUMMATION ORDER (part of the contract): lane l of 64 adds the points l, l + 64, ... in index order into its own sums, every sum from
// zero; the 64 partial sums are combined by the xor butterfly 32, 16, 8, 4, 2, 1 (a + b is commutative, so every lane ends with lane
// 0's value); the prior's terms are added to the combined sums last.  A point's share of an entry of J^T J is ((J0a J0b + J1a J1b) +
// J2a J2b) over its three residual rows, of J^T e likewise, of the cost ((e0 e0 + e1 e1) + e2 e2).
#ifndef CK_RIG_REFINE_MATH_H
#define CK_RIG_REFINE_MATH_H

#include "ck_pose_math.h"
#include "ck_rig_refine_c.h"
#include "ck_rigcal_math.h"

#define CKF_LANES 64
#define CKF_NSUM 27               /* free mode: the upper triangle of the 6 x 6 J^T J row by row (21), then J^T e (6); planar: 6 + 3 */

// What a walker needs of one instant
typedef struct ckf_ctx {
    const double *pts; // the point records
    size_t stride;     // doubles between the records' entries
    int np;            // used points
    int lane;          // the kernel's lane (the twin walks all 64 itself)
    double *part;      // the twin's scratch for the lanes' partial sums, [CKF_LANES][CKF_NSUM], its call's own; the kernel has none
} ckf_ctx_t;

// The three sums over the used points, each lane's share and the butterfly: n = 9 (planar) or 27 sums of the normal equations at P;
// the cost at P and whether any point lies at or behind its camera; the cost at P per camera.  xy = the planar position (planar only).
CKC_FN void ckf_walk_jac(const ckf_ctx_t *cx, const int planar, const double *P, const double *xy, double *acc);
CKC_FN void ckf_walk_cost(const ckf_ctx_t *cx, const double *P, double *cost, int *behind);
CKC_FN void ckf_walk_cams(const ckf_ctx_t *cx, const double *P, double *cam_cost);

// The tags a camera's record of nt tags keeps under the mask rej (bit t deletes tag t < 64; a tag from 64 on is always kept): how many,
// and the r-th of them
CKC_FN uint64_t ckf_keep_mask(int nt, uint64_t rej) { return ~rej & (nt >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << nt) - 1)); }
CKC_FN int ckf_kept(int nt, uint64_t rej) {
    uint64_t m = ckf_keep_mask(nt, rej);
    int k = nt > 64 ? nt - 64 : 0;
    while (m) { m &= m - 1; k++; }
    return k;
}
CKC_FN int ckf_kept_tag(int nt, uint64_t rej, int r) {
    if (rej == 0) return r;
    uint64_t m = ckf_keep_mask(nt, rej);
    int t = 0;
    while (m) {
        if (m & 1) { if (r == 0) return t; r--; }
        m >>= 1; t++;
    }
    return 64 + r;
}

// One point's record but for its camera number: corner 0..3 of the tag (t, q) seen along v by the camera mounted by robot_to_cam (bt, bq)
CKC_FN void ckf_point_record(const double *t, const double *q, const int corner, const double *v, const double *bt, const double *bq, double *rec) {
    double R[9], A[9];
    quat_to_mat(q, R);
    quat_to_mat(bq, A);
    const double y = (corner == 1 || corner == 2) ? CORNER_DISTANCE : -CORNER_DISTANCE, z = corner >= 2 ? CORNER_DISTANCE : -CORNER_DISTANCE;
    CKC_UNROLL
    for (int k = 0; k < 3; k++) {
        rec[k] = (R[3 * k + 1] * y + R[3 * k + 2] * z) + t[k];
        rec[3 + k] = v[k];
        rec[6 + 9 + k] = -((A[k] * bt[0] + A[3 + k] * bt[1]) + A[6 + k] * bt[2]);
    }
    CKC_UNROLL
    for (int k = 0; k < 9; k++) rec[6 + k] = A[k];
}

// The residual of one point and v.p (<= 0: the point lies at or behind the camera's plane)
CKC_FN double ckf_residual(const double *M, const double *P, const double *X, const double *v, double *e) {
    const double q0 = (P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[9]) - M[9];
    const double q1 = (P[3] * X[0] + P[4] * X[1] + P[5] * X[2] + P[10]) - M[10];
    const double q2 = (P[6] * X[0] + P[7] * X[1] + P[8] * X[2] + P[11]) - M[11];
    const double p0 = M[0] * q0 + M[1] * q1 + M[2] * q2, p1 = M[3] * q0 + M[4] * q1 + M[5] * q2, p2 = M[6] * q0 + M[7] * q1 + M[8] * q2;
    const double vp = v[0] * p0 + v[1] * p1 + v[2] * p2;
    const double f = vp / (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const double s = sqrt(p0 * p0 + p1 * p1 + p2 * p2);
    e[0] = (p0 - v[0] * f) / s; e[1] = (p1 - v[1] * f) / s; e[2] = (p2 - v[2] * f) / s;
    return vp;
}

// acc += one point's share of the normal equations.  Free: the six columns are cka_point's 6..11 (rotation increment about world axes:
// R <- R C(dw); translation).  Planar: the three columns (x, y, theta) of world <- robot = (Rz(theta), (x, y, z)) are those six times
// the chain-rule matrix: dw = (0, 0, -dtheta), dt = -R (dx, dy, 0) + dtheta (p_x R's column 1 - p_y R's column 0).
CKC_FN void ckf_point_sums(const int planar, const double *M, const double *P, const double *xy, const double *X, const double *v, double *acc) {
    double e[3], q[3], GA[9], GR[9], J[3 * CKA_NJ], Jm[18];
    cka_point(M, P, X, v, e, q, GA, GR, J);
    const int n = planar ? 3 : 6;
    if (planar) {
        const double k0 = P[1] * xy[0] - P[0] * xy[1], k1 = P[4] * xy[0] - P[3] * xy[1], k2 = P[7] * xy[0] - P[6] * xy[1];
        CKC_UNROLL
        for (int i = 0; i < 3; i++) {
            const double *Ji = J + CKA_NJ * i;
            Jm[3 * i] = -((Ji[9] * P[0] + Ji[10] * P[3]) + Ji[11] * P[6]);
            Jm[3 * i + 1] = -((Ji[9] * P[1] + Ji[10] * P[4]) + Ji[11] * P[7]);
            Jm[3 * i + 2] = ((Ji[9] * k0 + Ji[10] * k1) + Ji[11] * k2) - Ji[8];
        }
    } else {
        CKC_UNROLL
        for (int i = 0; i < 3; i++) {
            CKC_UNROLL
            for (int a = 0; a < 6; a++) Jm[6 * i + a] = J[CKA_NJ * i + 6 + a];
        }
    }
    int k = 0;
    CKC_UNROLL
    for (int a = 0; a < n; a++) {
        CKC_UNROLL
        for (int b = a; b < n; b++) {
            acc[k] = acc[k] + ((Jm[a] * Jm[b] + Jm[n + a] * Jm[n + b]) + Jm[2 * n + a] * Jm[2 * n + b]);
            k++;
        }
    }
    CKC_UNROLL
    for (int a = 0; a < n; a++) {
        acc[k] = acc[k] + ((Jm[a] * e[0] + Jm[n + a] * e[1]) + Jm[2 * n + a] * e[2]);
        k++;
    }
}

// The planar state S = (cos theta, sin theta, x, y) of world <- robot, its pose, its step by (dx, dy, dtheta): theta moves by the 2-d
// Cayley map ((1 - a^2) / (1 + a^2), 2 a / (1 + a^2)), a = dtheta / 2, a rotation for every dtheta
CKC_FN void ckf_planar_pose(const double *S, double z, double *P) {
    P[0] = S[0]; P[1] = S[1]; P[2] = 0.0;
    P[3] = -S[1]; P[4] = S[0]; P[5] = 0.0;
    P[6] = 0.0; P[7] = 0.0; P[8] = 1.0;
    P[9] = -(S[0] * S[2] + S[1] * S[3]);
    P[10] = -(S[0] * S[3] - S[1] * S[2]);
    P[11] = -z;
}
CKC_FN void ckf_planar_step(const double *S, const double *d, double *Sc) {
    const double a = 0.5 * d[2], den = 1.0 + a * a, cd = (1.0 - a * a) / den, sd = (2.0 * a) / den;
    Sc[0] = S[0] * cd - S[1] * sd;
    Sc[1] = S[1] * cd + S[0] * sd;
    Sc[2] = S[2] + d[0];
    Sc[3] = S[3] + d[1];
}

// The heading prior at P: the residual (R_wr[1][0] cg - R_wr[0][0] sg) / gs = (P[1] cg - P[0] sg) / gs and its row over the unknowns
CKC_FN double ckf_prior(const int planar, const double *P, double cg, double sg, double gs, double *jp) {
    if (planar) {
        jp[0] = 0.0; jp[1] = 0.0; jp[2] = (P[0] * cg + P[1] * sg) / gs;
    } else {
        jp[0] = (P[2] * cg) / gs; jp[1] = (P[2] * sg) / gs; jp[2] = -((P[0] * cg + P[1] * sg) / gs);
        jp[3] = 0.0; jp[4] = 0.0; jp[5] = 0.0;
    }
    return (P[1] * cg - P[0] * sg) / gs;
}

// The normal equations of the solve from the points' sums: A (lower triangle of n x n, row-major) = s2 acc + jp jp^T, g = s2 acc + jp rp
CKC_FN void ckf_normal(const int planar, const double *acc, double s2, int prior, const double *jp, double rp, double *A, double *g) {
    const int n = planar ? 3 : 6;
    int k = 0;
    CKC_UNROLL
    for (int a = 0; a < n; a++) {
        CKC_UNROLL
        for (int b = a; b < n; b++) {
            A[b * n + a] = s2 * acc[k];
            if (b > a) A[a * n + b] = 0.0;
            k++;
        }
    }
    CKC_UNROLL
    for (int a = 0; a < n; a++) {
        g[a] = s2 * acc[k];
        k++;
    }
    if (prior) {
        CKC_UNROLL
        for (int a = 0; a < n; a++) {
            CKC_UNROLL
            for (int b = 0; b <= a; b++) A[a * n + b] = A[a * n + b] + jp[a] * jp[b];
            g[a] = g[a] + jp[a] * rp;
        }
    }
}

// One instant.  planar is a constant where this is called.  sigma, gs, z, max_iters: the parameters; prior: gs > 0, with (cg, sg) the
// heading's cosine and sine; rot0 / pos0: the start record's pose (world <- robot); cam_np: the used points of every camera.  r is
// zero on entry; on return it is the instant's record.
CKC_FN void ckf_solve(const ckf_ctx_t *cx, const int planar, double sigma, double gs, double z, int max_iters, int prior, double cg,
                      double sg, const double *rot0, const double *pos0, const int *cam_np, ck_rig_refined_t *r) {
    const int n = planar ? 3 : 6;
    double Pa[12], Pc[12], Sa[4], Sc[4], acc[CKF_NSUM], A[36], L[36], g[6], d[6], D[6], jp[6];
    r->status = CK_RIG_REFINE_DEGENERATE;
    r->n_points = cx->np;
    CKC_UNROLL
    for (int i = 0; i < 9; i++) r->rot[i] = rot0[i];
    CKC_UNROLL
    for (int i = 0; i < 3; i++) r->pos[i] = pos0[i];
    CKC_UNROLL
    for (int i = 0; i < 4; i++) { Sa[i] = 0.0; Sc[i] = 0.0; }
    CKC_UNROLL
    for (int i = 0; i < 6; i++) jp[i] = 0.0;
    if (cx->np < 1) return;
    if (planar) {
        const double nn = sqrt(rot0[0] * rot0[0] + rot0[3] * rot0[3]);
        if (!(nn > 0.0)) return;
        Sa[0] = rot0[0] / nn; Sa[1] = rot0[3] / nn; Sa[2] = pos0[0]; Sa[3] = pos0[1];
        ckf_planar_pose(Sa, z, Pa);
    } else {
        CKC_UNROLL
        for (int i = 0; i < 3; i++) {
            CKC_UNROLL
            for (int j = 0; j < 3; j++) Pa[3 * i + j] = rot0[3 * j + i];
        }
        CKC_UNROLL
        for (int i = 0; i < 3; i++) Pa[9 + i] = -((Pa[3 * i] * pos0[0] + Pa[3 * i + 1] * pos0[1]) + Pa[3 * i + 2] * pos0[2]);
    }
    const double s2 = prior ? 1.0 / (sigma * sigma) : 1.0;
    double cpts = 0.0, rp = 0.0;
    int behind = 0;
    ckf_walk_cost(cx, Pa, &cpts, &behind);
    if (prior) rp = ckf_prior(planar, Pa, cg, sg, gs, jp);
    r->cost0 = cpts;
    const double c0 = s2 * cpts + rp * rp;
    if (!ckc_finite(c0)) return;
    ckc_lm_t lm;
    ckc_lm_start(&lm, c0, CKR_COST_FLOOR);
    while (lm.status < 0) {
        if (lm.need_jac) {
            ckf_walk_jac(cx, planar, Pa, Sa + 2, acc);
            if (prior) rp = ckf_prior(planar, Pa, cg, sg, gs, jp);
            ckf_normal(planar, acc, s2, prior, jp, rp, A, g);
            CKC_UNROLL
            for (int i = 0; i < n; i++) D[i] = A[i * n + i];
        }
        CKC_UNROLL
        for (int i = 0; i < n * n; i++) L[i] = A[i];
        CKC_UNROLL
        for (int i = 0; i < n; i++) {
            L[i * n + i] = L[i * n + i] + lm.lambda * ckc_scale(D[i]);
            d[i] = -g[i];
        }
        int solved = ckc_chol(L, n);
        ckc_fwd(L, n, d, 1);
        ckc_bwd(L, n, d);
        double pred = 0.0, cnew = 0.0, cpts_new = 0.0;
        CKC_UNROLL
        for (int i = 0; i < n; i++) pred = pred + d[i] * ((lm.lambda * ckc_scale(D[i])) * d[i] - g[i]);
        // A relative rule asked of the step before it is paid for: the model itself promises no more than 1e-18 of the cost (the
        // predicted decrease is formed from the step and the gradient, so it resolves what a difference of two costs cannot).  Without
        // it a solve at its minimum, where round-off decides the sign of a decrease, spends a dozen iterations raising the damping to
        // 1e30 before it may say so.
        if (solved && pred <= 1e-18 * lm.cost) {
            lm.status = 0;
            lm.need_jac = 0; // (the sums are the accepted pose's)
            break;
        }
        if (solved) {
            if (planar) {
                ckf_planar_step(Sa, d, Sc);
                ckf_planar_pose(Sc, z, Pc);
            } else {
                ckc_rigid_step(Pa, d, 0u, Pc);
            }
            ckf_walk_cost(cx, Pc, &cpts_new, &behind);
            double rpn = 0.0, jn[6];
            if (prior) rpn = ckf_prior(planar, Pc, cg, sg, gs, jn);
            cnew = s2 * cpts_new + rpn * rpn;
            if (behind) solved = 0; // refused like a cost increase
        }
        if (ckc_lm_decide(&lm, solved, pred, cnew, max_iters, CKR_COST_FLOOR)) {
            CKC_UNROLL
            for (int i = 0; i < 12; i++) Pa[i] = Pc[i];
            CKC_UNROLL
            for (int i = 0; i < 4; i++) Sa[i] = Sc[i];
            cpts = cpts_new;
        }
    }
    // the covariance at the accepted pose: the undamped normal matrix (its sums are the last pass's unless a step was accepted since)
    if (lm.need_jac) {
        ckf_walk_jac(cx, planar, Pa, Sa + 2, acc);
        if (prior) rp = ckf_prior(planar, Pa, cg, sg, gs, jp);
        ckf_normal(planar, acc, s2, prior, jp, rp, A, g);
    }
    if (!ckc_chol(A, n)) return;
    if (prior) rp = ckf_prior(planar, Pa, cg, sg, gs, jp);
    double rot[9], pos[3], B[36];
    CKC_UNROLL
    for (int i = 0; i < 3; i++) {
        CKC_UNROLL
        for (int j = 0; j < 3; j++) rot[3 * i + j] = Pa[3 * j + i];
        pos[i] = -((Pa[i] * Pa[9] + Pa[3 + i] * Pa[10]) + Pa[6 + i] * Pa[11]);
    }
    if (planar) { pos[0] = Sa[2]; pos[1] = Sa[3]; pos[2] = z; }
    // B = L^-1 T^T, cov = scale B^T B: T maps the solve's increments to the world-axes tangent of world <- robot.  Free: dp = p x dw - R^T
    // dt, dwr = -dw, rows (dp, dwr), columns (dw, dt).  Planar: (x, y, theta) are the tangent's x, y, wz themselves.
    CKC_UNROLL
    for (int i = 0; i < 36; i++) B[i] = 0.0;
    if (planar) {
        B[0] = 1.0; B[4] = 1.0; B[8] = 1.0;
    } else {
        B[0 * 6 + 1] = pos[2]; B[0 * 6 + 2] = -pos[1];   // column i of T^T = row i of T; B[k * 6 + i] = T[i][k]
        B[1 * 6 + 0] = -pos[2]; B[1 * 6 + 2] = pos[0];
        B[2 * 6 + 0] = pos[1]; B[2 * 6 + 1] = -pos[0];
        CKC_UNROLL
        for (int i = 0; i < 3; i++) {
            CKC_UNROLL
            for (int j = 0; j < 3; j++) B[(3 + j) * 6 + i] = -Pa[3 * j + i];
            B[i * 6 + 3 + i] = -1.0;
        }
    }
    CKC_UNROLL
    for (int i = 0; i < n; i++) ckc_fwd(A, n, B + i, n);
    const double scale = prior ? 1.0 : sigma * sigma;
    CKC_UNROLL
    for (int i = 0; i < n; i++) {
        CKC_UNROLL
        for (int j = i; j < n; j++) {
            double t = 0.0;
            CKC_UNROLL
            for (int k = 0; k < n; k++) t = t + B[k * n + i] * B[k * n + j];
            t = scale * t;
            const int a = planar ? (i == 2 ? 5 : i) : i, b = planar ? (j == 2 ? 5 : j) : j;
            r->cov[a * 6 + b] = t;
            r->cov[b * 6 + a] = t;
        }
    }
    r->std_devs[0] = sqrt(r->cov[0]); r->std_devs[1] = sqrt(r->cov[7]); r->std_devs[2] = sqrt(r->cov[35]);
    double m2 = 0.0, a2 = 0.0;
    CKC_UNROLL
    for (int i = 0; i < 3; i++) m2 = m2 + (pos[i] - pos0[i]) * (pos[i] - pos0[i]);
    CKC_UNROLL
    for (int i = 0; i < 9; i++) a2 = a2 + (rot[i] - rot0[i]) * (rot[i] - rot0[i]);
    r->moved_m = sqrt(m2);
    r->moved_rad = sqrt(a2 / 2.0);
    CKC_UNROLL
    for (int i = 0; i < 9; i++) r->rot[i] = rot[i];
    CKC_UNROLL
    for (int i = 0; i < 3; i++) r->pos[i] = pos[i];
    r->status = lm.status == 2 ? CK_RIG_REFINE_MAXITERS : CK_RIG_REFINE_CONVERGED;
    r->iters = lm.iters;
    r->cost = cpts;
    r->rms = sqrt(cpts / (double)cx->np);
    r->dof = 2 * cx->np + (prior ? 1 : 0) - n;
    r->chi2 = r->dof > 0 ? (cpts / (sigma * sigma) + rp * rp) / (double)r->dof : 0.0;
    double cc[CK_RIG_MAX_CAMS];
    ckf_walk_cams(cx, Pa, cc);
    CKC_UNROLL
    for (int c = 0; c < CK_RIG_MAX_CAMS; c++) r->cam_rms[c] = cam_np[c] > 0 ? sqrt(cc[c] / (double)cam_np[c]) : 0.0;
}

#endif
