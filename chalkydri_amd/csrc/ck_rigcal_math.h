// ck_rigcal_math.h — the mount calibration's own arithmetic: its residual, the camera's columns of the Jacobian and
// the points' sums.  Everything else of the solver is ck_cal_math.h's, shared with the field calibration (§4m): there a COLUMN is a
// camera's mount and a BLOCK is a VIEW, one (used step, camera) that has points.  Compiled as C into the host twin
// (ck_rigcal_host.c) and as device code into k_rigcal.hip, -ffp-contract=off on both sides, so the two produce the same bytes.
//
// A pose is 12 doubles, R row-major then t: p_robot = R X + t.  A mount is 12 doubles, A row-major then o: p_cam = A (p_robot - o).
// A view's Jacobian has 12 columns: the camera's rotation increment about robot x y z (0..2), the camera's position o (3..5), the
// step's rotation increment (6..8), the step's translation (9..11).
// SUMMATION ORDER (part of the contract): lane l of a group of 16 adds the points l, l + 16, ... of its view in index order into its
// own sums, starting from zero; the 16 partial sums are combined by the xor butterfly 8, 4, 2, 1; then ck_cal_math.h's order: the
// views of a step in camera order, the steps in step order, a camera without a point in a step skipped.
#ifndef CK_RIGCAL_MATH_H
#define CK_RIGCAL_MATH_H

#include "ck_cal_math.h"

#define CKR_GROUP 16              /* lanes per view */
// The view table of a capture, three int32 per (camera, step) record c * n + s: first world point, first bearing, points
#define CKR_TAB 3
#define CKR_NPTS(tab, n, c, s) ((tab)[((size_t)(c) * (size_t)(n) + (size_t)(s)) * CKR_TAB + 2])

// residual of one point: world point X seen along v by the camera mounted by M at the step with pose P
CKC_FN void ckr_residual(const double *M, const double *P, const double *X, const double *v, double *e) {
    const double q0 = (P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[9]) - M[9];
    const double q1 = (P[3] * X[0] + P[4] * X[1] + P[5] * X[2] + P[10]) - M[10];
    const double q2 = (P[6] * X[0] + P[7] * X[1] + P[8] * X[2] + P[11]) - M[11];
    const double p0 = M[0] * q0 + M[1] * q1 + M[2] * q2, p1 = M[3] * q0 + M[4] * q1 + M[5] * q2, p2 = M[6] * q0 + M[7] * q1 + M[8] * q2;
    const double f = (v[0] * p0 + v[1] * p1 + v[2] * p2) / (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const double s = sqrt(p0 * p0 + p1 * p1 + p2 * p2);
    e[0] = (p0 - v[0] * f) / s; e[1] = (p1 - v[1] * f) / s; e[2] = (p2 - v[2] * f) / s;
}

// residual and the three Jacobian rows J[3][12] at zero increments; the camera's frozen columns (bits 0..5 of mask6) are zero
CKC_FN void ckr_jacobian(const double *M, const double *P, const double *X, const double *v, unsigned mask6, double *e, double *J) {
    double q[3], GA[9], GR[9];
    cka_point(M, P, X, v, e, q, GA, GR, J);
    // A C(dw) q = A (q + dw x q): the columns of d(dw x q) / d(dw) are (0, -q2, q1), (q2, 0, -q0), (-q1, q0, 0)
    CKC_UNROLL
    for (int i = 0; i < 3; i++) {
        double *Ji = J + CKA_NJ * i;
        Ji[0] = GA[3 * i + 2] * q[1] - GA[3 * i + 1] * q[2];
        Ji[1] = GA[3 * i] * q[2] - GA[3 * i + 2] * q[0];
        Ji[2] = GA[3 * i + 1] * q[0] - GA[3 * i] * q[1];
        Ji[3] = -GA[3 * i]; Ji[4] = -GA[3 * i + 1]; Ji[5] = -GA[3 * i + 2];
    }
    cka_freeze_columns(J, mask6);
}

// tri += the rows a0 .. a1 - 1 of one point's share of the triangle (from row a0's diagonal on) and, when g is not null, g += J^T e.
// The kernel forms the sums in two passes over the points so that a lane's partial sums stay in registers; each entry is the same sum.
CKC_FN void ckr_accumulate_rows(double *tri, double *g, const double *e, const double *J, const int a0, const int a1) {
    int n = 0;
    CKC_UNROLL
    for (int a = a0; a < a1; a++) {
        CKC_UNROLL
        for (int b = a; b < CKA_NJ; b++) {
            tri[n] = tri[n] + ((J[a] * J[b] + J[CKA_NJ + a] * J[CKA_NJ + b]) + J[2 * CKA_NJ + a] * J[2 * CKA_NJ + b]);
            n++;
        }
    }
    if (g) {
        CKC_UNROLL
        for (int a = 0; a < CKA_NJ; a++) g[a] = g[a] + ((J[a] * e[0] + J[CKA_NJ + a] * e[1]) + J[2 * CKA_NJ + a] * e[2]);
    }
}

// The cost below which a solve is done (ckc_lm_start / ckc_lm_decide).  §4j's is 1e-20 px^2; this cost is in rad^2, and 1e-20 rad^2
// over the thousands of points of a capture is an rms of 1e-12 rad, which ends a noise-free solve one step before the mounts reach
// round-off.  CKR_COST_FLOOR is below what double precision leaves of an exact capture's cost (1e-32 per point), so such a solve ends
// by the relative rule or STALLED.
#define CKR_COST_FLOOR 1e-40

#endif
