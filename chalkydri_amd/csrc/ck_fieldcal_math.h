// ck_fieldcal_math.h — the field calibration's own arithmetic: its residual, the tag's columns of the Jacobian and the
// sums of a pair's sightings.  Everything else of the solver is ck_cal_math.h's, shared with the mount calibration (§4l): there a
// COLUMN is a tag's pose and a BLOCK is a PAIR.  From ck_rigcal_math.h: ckr_residual, ckr_accumulate_rows, CKR_COST_FLOOR.  Compiled
// as C into the host twin (ck_fieldcal_host.c) and as device code into k_fieldcal.hip, both with -ffp-contract=off, so the two
// produce the same bytes.
//
// A pose is 12 doubles, R row-major then t: p_robot = R X + t.  A mount is 12 doubles (A, o): p_cam = A (p_robot - o).  A tag is 12
// doubles, Q row-major then c: X = Q x + c for a corner x in the tag's own frame.  A SIGHTING is one (used step, camera, tag) of 4
// points; a PAIR is one (used step, tag), the sightings of it in camera order.  A point's Jacobian has 12 columns: the tag's rotation
// increment about its own axes (0..2), the tag's position in world axes (3..5), the step's rotation increment (6..8) and the step's
// translation (9..11).
// SUMMATION ORDER (part of the contract): lane l of a group of 4 has corner l of its sighting; the 4 values are combined by the xor
// butterfly 2, 1; the sightings of a pair are added in camera order, each sum starting from zero; then ck_cal_math.h's order: the pairs
// of a step in tag order, the steps in step order, a tag that a step does not see skipped.  Every entry of the reduced system is one
// such sum over the steps; its factorisation and the two substitutions subtract their products in a fixed order per entry
// (ck_fieldcal_host.c: reduced_solve), which does not depend on how many threads share the work.
#ifndef CK_FIELDCAL_MATH_H
#define CK_FIELDCAL_MATH_H

#include "ck_rigcal_math.h"

#define CKF_GROUP 4                      /* lanes per sighting = corners of a tag */
#define CKF_S (0.1651 / 2.0)             /* corner_points_from_center: half the tag's side */
#define CKF_LT(i, j) (((size_t)(i) * ((size_t)(i) + 1)) / 2 + (size_t)(j)) /* entry (i, j), j <= i, of a packed lower triangle */

// The record of a sighting (doubles)
enum {
    CKF_I_H = 0,                  // [78] upper triangle of J^T J of its 4 points, row by row
    CKF_I_G = CKF_I_H + CKA_NH,   // [12] J^T e
    CKF_I_COST = CKF_I_G + CKA_NJ, // [1] the candidate's squared residuals
    CKF_I_STRIDE = 92
};

// The integer tables of one problem, laid out one after the other from `base`: the arrowhead index (columns = tags, blocks = pairs)
// and on top of it the sightings; U used steps, P pairs, NS sightings, T tags
typedef struct ckf_meta {
    cka_index_t ix;
    const int32_t *pair_sight; // [P + 1] first sighting of every pair
    const int32_t *sight_pair; // [NS]
    const int32_t *sight_cam;  // [NS]
    const int32_t *sight_bear; // [NS]    first of its 4 bearings
    const int32_t *ltag;       // [T]     the tag's entry of the layout
    const int32_t *tag_ns;     // [T]     its sightings
    const int32_t *mask6;      // [T]     its frozen increments
} ckf_meta_t;
CKA_HD size_t ckf_meta_size(size_t U, size_t P, size_t NS, size_t T) { return cka_index_size(U, P, T) + P + 1 + 3 * NS + 3 * T; }
CKA_HD ckf_meta_t ckf_meta_at(const int32_t *base, size_t U, size_t P, size_t NS, size_t T) {
    ckf_meta_t m;
    m.ix = cka_index_at(base, U, P);
    m.pair_sight = base + cka_index_size(U, P, T); m.sight_pair = m.pair_sight + P + 1; m.sight_cam = m.sight_pair + NS;
    m.sight_bear = m.sight_cam + NS; m.ltag = m.sight_bear + NS; m.tag_ns = m.ltag + T; m.mask6 = m.tag_ns + T;
    return m;
}

// corner j of a tag in its own frame, and in the world under the tag pose T
CKC_FN void ckf_corner(int j, double *x) {
    x[0] = 0.0;
    x[1] = (j == 0 || j == 3) ? -CKF_S : CKF_S;
    x[2] = j < 2 ? -CKF_S : CKF_S;
}
CKC_FN void ckf_world(const double *T, const double *x, double *X) {
    CKC_UNROLL
    for (int k = 0; k < 3; k++) X[k] = (T[3 * k] * x[0] + T[3 * k + 1] * x[1] + T[3 * k + 2] * x[2]) + T[9 + k];
}

// residual of corner j of the tag T seen along v by the camera mounted by M at the step with pose P
CKC_FN void ckf_residual(const double *M, const double *P, const double *T, int j, const double *v, double *e) {
    double x[3], X[3];
    ckf_corner(j, x);
    ckf_world(T, x, X);
    ckr_residual(M, P, X, v, e);
}

// residual and the three Jacobian rows J[3][12] at zero increments; the tag's frozen columns (bits 0..5 of mask6) are zero
CKC_FN void ckf_jacobian(const double *M, const double *P, const double *T, int j, const double *v, unsigned mask6, double *e, double *J) {
    double x[3], X[3], q[3], GA[9], GR[9], GQ[9];
    ckf_corner(j, x);
    ckf_world(T, x, X);
    cka_point(M, P, X, v, e, q, GA, GR, J);
    // GR = de / dX = de / dc;  GQ = GR Q
    CKC_UNROLL
    for (int i = 0; i < 3; i++) {
        CKC_UNROLL
        for (int k = 0; k < 3; k++) GQ[3 * i + k] = GR[3 * i] * T[k] + GR[3 * i + 1] * T[3 + k] + GR[3 * i + 2] * T[6 + k];
    }
    // Q C(dw) x = Q (x + dw x x): the columns of d(dw x x) / d(dw) are (0, -x2, x1), (x2, 0, -x0), (-x1, x0, 0)
    CKC_UNROLL
    for (int i = 0; i < 3; i++) {
        double *Ji = J + CKA_NJ * i;
        Ji[0] = GQ[3 * i + 2] * x[1] - GQ[3 * i + 1] * x[2];
        Ji[1] = GQ[3 * i] * x[2] - GQ[3 * i + 2] * x[0];
        Ji[2] = GQ[3 * i + 1] * x[0] - GQ[3 * i] * x[1];
        Ji[3] = GR[3 * i]; Ji[4] = GR[3 * i + 1]; Ji[5] = GR[3 * i + 2];
    }
    cka_freeze_columns(J, mask6);
}

// A pair's normal equations: its n sightings' records (consecutive, in camera order) added from zero
CKC_FN void ckf_pair_sum(double *pr, const double *sights, int n) {
    for (int j = 0; j < CKA_NH + CKA_NJ; j++) {
        double t = 0.0;
        for (int i = 0; i < n; i++) t = t + sights[(size_t)CKF_I_STRIDE * i + CKF_I_H + j];
        pr[CKA_B_H + j] = t;
    }
}

// A used step's candidate cost: per pair its n sightings in camera order, then the step's np pairs (consecutive records, in tag order)
CKC_FN void ckf_step_cost(double *st, double *pairs, const double *sights, const int32_t *pair_sight, int np) {
    double cs = 0.0;
    for (int k = 0; k < np; k++) {
        double t = 0.0;
        for (int i = pair_sight[k]; i < pair_sight[k + 1]; i++) t = t + sights[(size_t)CKF_I_STRIDE * (i - pair_sight[0]) + CKF_I_COST];
        pairs[(size_t)CKA_B_STRIDE * k + CKA_B_COST] = t;
        cs = cs + t;
    }
    st[CKA_S_COST] = cs;
}

#endif
