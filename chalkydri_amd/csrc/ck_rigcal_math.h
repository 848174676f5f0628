// ck_rigcal_math.h — the arithmetic of the mount calibration, written once and compiled twice: as C into the host
// twin (ck_rigcal_host.c) and as device code into k_rigcal.hip.  Only + - * / sqrt on doubles, every expression evaluated as written
// (-ffp-contract=off on both sides), so the two produce the same bytes.  The helpers of ck_calib_math.h that fit are used as they
// are: ckc_finite, ckc_scale, ckc_chol / ckc_fwd / ckc_bwd on the 6 x 6 blocks, the damping and stop rules (ckc_lm_t).
//
// A pose is 12 doubles, R row-major then t: p_robot = R X + t.  A mount is 12 doubles, A row-major then o: p_cam = A (p_robot - o).
// A VIEW is one (used step, camera) pair; its Jacobian has 12 columns: the camera's rotation increment about robot x y z (0..2), the
// camera's position o (3..5), the step's rotation increment (6..8), the step's translation (9..11).
// SUMMATION ORDER (part of the contract): lane l of a group of 16 adds the points l, l + 16, ... of its view in index order into its
// own sums, starting from zero; the 16 partial sums are combined by the xor butterfly 8, 4, 2, 1; the views of a step are added in
// camera order, the steps in step order.  A camera that has no point in a step has no view there and is skipped, not added as zero.
#ifndef CK_RIGCAL_MATH_H
#define CK_RIGCAL_MATH_H

#include <stdint.h>

#include "ck_calib_math.h"

#define CKR_NJ 12                 /* columns of one point's Jacobian */
#define CKR_NH 78                 /* upper triangle of NJ x NJ */
#define CKR_TRI(a, b) ((a) * CKR_NJ - ((a) * ((a) - 1)) / 2 + ((b) - (a))) /* a <= b */
#define CKR_GROUP 16              /* lanes per view */

// The record of a view (doubles)
enum {
    CKR_V_H = 0,                  // [78] upper triangle of J^T J, row by row
    CKR_V_G = CKR_V_H + CKR_NH,   // [12] J^T e
    CKR_V_COST = CKR_V_G + CKR_NJ, // [1] the candidate's squared residuals of this view
    CKR_V_COSTA = CKR_V_COST + 1, // [1] the same at the accepted parameters
    CKR_V_W = CKR_V_COSTA + 1,    // [6][6] L^-1 B^T: rows = the step's increments, columns = the camera's
    CKR_V_WG = CKR_V_W + 36,      // [6]  W^T wg
    CKR_V_STRIDE = 136
};
// The record of a used step (doubles)
enum {
    CKR_S_POSE = 0,               // [12] accepted
    CKR_S_CAND = 12,              // [12] candidate
    CKR_S_L = 24,                 // [36] Cholesky factor of A_s + lambda D_s, lower triangle of a 6 x 6
    CKR_S_WG = 60,                // [6]  L^-1 g_s
    CKR_S_D = 66,                 // [6]  diagonal of A_s
    CKR_S_G = 72,                 // [6]  g_s
    CKR_S_PRED = 78,              // [1]  the step's share of the predicted decrease
    CKR_S_COST = 79,              // [1]  the candidate's squared residuals of this step
    CKR_S_STRIDE = 80
};
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
    double q[3], p[3];
    CKC_UNROLL
    for (int i = 0; i < 3; i++) q[i] = (P[3 * i] * X[0] + P[3 * i + 1] * X[1] + P[3 * i + 2] * X[2] + P[9 + i]) - M[9 + i];
    CKC_UNROLL
    for (int i = 0; i < 3; i++) p[i] = M[3 * i] * q[0] + M[3 * i + 1] * q[1] + M[3 * i + 2] * q[2];
    const double vv = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    const double f = (v[0] * p[0] + v[1] * p[1] + v[2] * p[2]) / vv;
    const double pp = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
    const double s = sqrt(pp);
    CKC_UNROLL
    for (int i = 0; i < 3; i++) e[i] = (p[i] - v[i] * f) / s;
    // G = de / dp = (I - v v^T / v.v) / |p| - e p^T / p.p;  GA = G A;  GR = GA R
    double G[9], GA[9], GR[9];
    CKC_UNROLL
    for (int i = 0; i < 3; i++) {
        CKC_UNROLL
        for (int j = 0; j < 3; j++) G[3 * i + j] = ((i == j ? 1.0 : 0.0) - (v[i] * v[j]) / vv) / s - (e[i] * p[j]) / pp;
    }
    CKC_UNROLL
    for (int i = 0; i < 3; i++) {
        CKC_UNROLL
        for (int j = 0; j < 3; j++) GA[3 * i + j] = G[3 * i] * M[j] + G[3 * i + 1] * M[3 + j] + G[3 * i + 2] * M[6 + j];
    }
    CKC_UNROLL
    for (int i = 0; i < 3; i++) {
        CKC_UNROLL
        for (int j = 0; j < 3; j++) GR[3 * i + j] = GA[3 * i] * P[j] + GA[3 * i + 1] * P[3 + j] + GA[3 * i + 2] * P[6 + j];
    }
    // A C(dw) q = A (q + dw x q): the columns of d(dw x q) / d(dw) are (0, -q2, q1), (q2, 0, -q0), (-q1, q0, 0); the same with R and X
    CKC_UNROLL
    for (int i = 0; i < 3; i++) {
        double *Ji = J + CKR_NJ * i;
        Ji[0] = GA[3 * i + 2] * q[1] - GA[3 * i + 1] * q[2];
        Ji[1] = GA[3 * i] * q[2] - GA[3 * i + 2] * q[0];
        Ji[2] = GA[3 * i + 1] * q[0] - GA[3 * i] * q[1];
        Ji[3] = -GA[3 * i]; Ji[4] = -GA[3 * i + 1]; Ji[5] = -GA[3 * i + 2];
        Ji[6] = GR[3 * i + 2] * X[1] - GR[3 * i + 1] * X[2];
        Ji[7] = GR[3 * i] * X[2] - GR[3 * i + 2] * X[0];
        Ji[8] = GR[3 * i + 1] * X[0] - GR[3 * i] * X[1];
        Ji[9] = GA[3 * i]; Ji[10] = GA[3 * i + 1]; Ji[11] = GA[3 * i + 2];
        CKC_UNROLL
        for (int a = 0; a < 6; a++)
            if ((mask6 >> a) & 1u) Ji[a] = 0.0;
    }
}

// tri += the rows a0 .. a1 - 1 of one point's share of the triangle (from row a0's diagonal on) and, when g is not null, g += J^T e.
// The kernel forms the sums in two passes over the points so that a lane's partial sums stay in registers; each entry is the same sum.
CKC_FN void ckr_accumulate_rows(double *tri, double *g, const double *e, const double *J, const int a0, const int a1) {
    int n = 0;
    CKC_UNROLL
    for (int a = a0; a < a1; a++) {
        CKC_UNROLL
        for (int b = a; b < CKR_NJ; b++) {
            tri[n] = tri[n] + ((J[a] * J[b] + J[CKR_NJ + a] * J[CKR_NJ + b]) + J[2 * CKR_NJ + a] * J[2 * CKR_NJ + b]);
            n++;
        }
    }
    if (g) {
        CKC_UNROLL
        for (int a = 0; a < CKR_NJ; a++) g[a] = g[a] + ((J[a] * e[0] + J[CKR_NJ + a] * e[1]) + J[2 * CKR_NJ + a] * e[2]);
    }
}

// One used step's part of the Schur complement at damping lambda.  st = the step's record, views = the records of its n_cams views,
// tab / n / s = the capture's view table, its step count and the step's number in it.  A_s and g_s are the views' step blocks added
// in camera order; L = chol(A_s + lambda D_s), wg = L^-1 g_s, and per view W = L^-1 B^T, W^T wg.  0 when the factorisation fails.
CKC_FN int ckr_step_schur(double *st, double *views, int n_cams, const int32_t *tab, int n, int s, double lambda) {
    double L[36], wg[6];
    CKC_UNROLL
    for (int i = 0; i < 36; i++) L[i] = 0.0;
    CKC_UNROLL
    for (int i = 0; i < 6; i++) wg[i] = 0.0;
    for (int c = 0; c < n_cams; c++) {
        if (CKR_NPTS(tab, n, c, s) <= 0) continue;
        const double *V = views + (size_t)CKR_V_STRIDE * c;
        CKC_UNROLL
        for (int i = 0; i < 6; i++) {
            CKC_UNROLL
            for (int j = 0; j <= i; j++) L[i * 6 + j] = L[i * 6 + j] + V[CKR_V_H + CKR_TRI(6 + j, 6 + i)];
            wg[i] = wg[i] + V[CKR_V_G + 6 + i];
        }
    }
    CKC_UNROLL
    for (int i = 0; i < 6; i++) {
        st[CKR_S_D + i] = L[i * 6 + i];
        st[CKR_S_G + i] = wg[i];
        L[i * 6 + i] = L[i * 6 + i] + lambda * ckc_scale(L[i * 6 + i]);
    }
    const int ok = ckc_chol(L, 6);
    ckc_fwd(L, 6, wg, 1);
    CKC_UNROLL
    for (int i = 0; i < 36; i++) st[CKR_S_L + i] = L[i];
    CKC_UNROLL
    for (int i = 0; i < 6; i++) st[CKR_S_WG + i] = wg[i];
    for (int c = 0; c < n_cams; c++) {
        if (CKR_NPTS(tab, n, c, s) <= 0) continue;
        double *V = views + (size_t)CKR_V_STRIDE * c;
        double W[36];
        CKC_UNROLL
        for (int i = 0; i < 6; i++) {
            CKC_UNROLL
            for (int a = 0; a < 6; a++) W[i * 6 + a] = V[CKR_V_H + CKR_TRI(a, 6 + i)];
        }
        CKC_UNROLL
        for (int a = 0; a < 6; a++) ckc_fwd(L, 6, W + a, 6);
        CKC_UNROLL
        for (int i = 0; i < 36; i++) V[CKR_V_W + i] = W[i];
        CKC_UNROLL
        for (int a = 0; a < 6; a++) {
            double t = 0.0;
            CKC_UNROLL
            for (int i = 0; i < 6; i++) t = t + W[i * 6 + a] * wg[i];
            V[CKR_V_WG + a] = t;
        }
    }
    return ok;
}

// Entry j of camera c's own sums over the used steps, in step order: j < 21 the upper triangle of its 6 x 6 block row by row, then
// J^T e (6).  views = the problem's view records [n_used][n_cams], used = its used steps' numbers.
CKC_FN double ckr_cam_sum(const double *views, int n_used, int n_cams, const int32_t *tab, int n, const int32_t *used, int c, int j) {
    int off = CKR_V_G + (j - 21);
    if (j < 21) {
        int a = 0, k = j;
        while (k >= 6 - a) { k -= 6 - a; a++; }
        off = CKR_V_H + CKR_TRI(a, a + k);
    }
    double t = 0.0;
    for (int u = 0; u < n_used; u++)
        if (CKR_NPTS(tab, n, c, used[u]) > 0) t = t + views[(size_t)CKR_V_STRIDE * ((size_t)u * n_cams + c) + off];
    return t;
}
// What the elimination of the steps takes from entry (r, k), r <= k, of the reduced system (r = 6 c + a), over the steps where
// both cameras have a view, in step order; with k < 0 the entry r of the right-hand side, sum of W^T wg.
CKC_FN double ckr_schur_sum(const double *views, int n_used, int n_cams, const int32_t *tab, int n, const int32_t *used, int r, int k) {
    const int c = r / 6, a = r % 6;
    double t = 0.0;
    if (k < 0) {
        for (int u = 0; u < n_used; u++)
            if (CKR_NPTS(tab, n, c, used[u]) > 0) t = t + views[(size_t)CKR_V_STRIDE * ((size_t)u * n_cams + c) + CKR_V_WG + a];
        return t;
    }
    const int c2 = k / 6, b = k % 6;
    for (int u = 0; u < n_used; u++) {
        if (CKR_NPTS(tab, n, c, used[u]) <= 0 || CKR_NPTS(tab, n, c2, used[u]) <= 0) continue;
        const double *W1 = views + (size_t)CKR_V_STRIDE * ((size_t)u * n_cams + c) + CKR_V_W + a;
        const double *W2 = views + (size_t)CKR_V_STRIDE * ((size_t)u * n_cams + c2) + CKR_V_W + b;
        double w = 0.0;
        CKC_UNROLL
        for (int i = 0; i < 6; i++) w = w + W1[6 * i] * W2[6 * i];
        t = t + w;
    }
    return t;
}

// The reduced system of N = 6 n_cams unknowns: S (N x N, lower triangle used) = C + lambda D - E, rhs = E_g - g; a frozen unknown
// (bit of mask) gets the row of the identity.  Hc = the cameras' own sums [n_cams][27], E = the upper triangle of ckr_schur_sum row
// by row [N (N + 1) / 2], Eg [N].  dk = the step, *pred its share of the predicted decrease.  0 when the factorisation fails.
CKC_FN int ckr_reduced_solve(const double *Hc, const double *E, const double *Eg, int N, double lambda, uint64_t mask, double *S, double *dk,
                             double *pred) {
    int n = 0;
    for (int r = 0; r < N; r++)
        for (int k = r; k < N; k++) {
            double t = 0.0;
            if (r / 6 == k / 6) {
                const int a = r % 6, b = k % 6;
                t = Hc[27 * (r / 6) + (a * 6 - (a * (a - 1)) / 2 + (b - a))];
                if (r == k) t = t + lambda * ckc_scale(t);
            }
            t = t - E[n];
            n++;
            if (((mask >> r) & 1u) || ((mask >> k) & 1u)) t = r == k ? 1.0 : 0.0;
            S[k * N + r] = t;
        }
    for (int r = 0; r < N; r++) dk[r] = ((mask >> r) & 1u) ? 0.0 : Eg[r] - Hc[27 * (r / 6) + 21 + r % 6];
    int ok = 1;
    for (int j = 0; j < N; j++) {
        double t = S[j * N + j];
        for (int c = 0; c < j; c++) t = t - S[j * N + c] * S[j * N + c];
        if (!(t > 0.0)) ok = 0;
        const double d = sqrt(t);
        S[j * N + j] = d;
        for (int i = j + 1; i < N; i++) {
            double w = S[i * N + j];
            for (int c = 0; c < j; c++) w = w - S[i * N + c] * S[j * N + c];
            S[i * N + j] = w / d;
        }
    }
    for (int i = 0; i < N; i++) {
        double t = dk[i];
        for (int c = 0; c < i; c++) t = t - S[i * N + c] * dk[c];
        dk[i] = t / S[i * N + i];
    }
    for (int ii = 0; ii < N; ii++) {
        const int i = N - 1 - ii;
        double t = dk[i];
        for (int c = i + 1; c < N; c++) t = t - S[c * N + i] * dk[c];
        dk[i] = t / S[i * N + i];
    }
    double p = 0.0;
    for (int r = 0; r < N; r++) {
        if ((mask >> r) & 1u) dk[r] = 0.0;
        const int a = r % 6;
        p = p + dk[r] * ((lambda * ckc_scale(Hc[27 * (r / 6) + (a * 6 - (a * (a - 1)) / 2)])) * dk[r] - Hc[27 * (r / 6) + 21 + a]);
    }
    *pred = p;
    return ok;
}

// C(d), the Cayley map of ck_calib_math.h: ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a), a = d / 2
CKC_FN void ckr_cayley(const double *d, double *Cm) {
    const double a0 = 0.5 * d[0], a1 = 0.5 * d[1], a2 = 0.5 * d[2];
    const double nn = a0 * a0 + a1 * a1 + a2 * a2, den = 1.0 + nn, e = 1.0 - nn;
    Cm[0] = (e + (2.0 * a0) * a0) / den; Cm[1] = ((2.0 * a0) * a1 - 2.0 * a2) / den; Cm[2] = ((2.0 * a0) * a2 + 2.0 * a1) / den;
    Cm[3] = ((2.0 * a1) * a0 + 2.0 * a2) / den; Cm[4] = (e + (2.0 * a1) * a1) / den; Cm[5] = ((2.0 * a1) * a2 - 2.0 * a0) / den;
    Cm[6] = ((2.0 * a2) * a0 - 2.0 * a1) / den; Cm[7] = ((2.0 * a2) * a1 + 2.0 * a0) / den; Cm[8] = (e + (2.0 * a2) * a2) / den;
}

// One step's increment given the cameras': d_s = -L^-T (wg + sum_c W_c dk_c), cameras in order; the candidate pose R C(d_w), t + d_t;
// the step's share of the predicted decrease.
CKC_FN void ckr_step_step(double *st, const double *views, int n_cams, const int32_t *tab, int n, int s, const double *dk, double lambda) {
    double d[6], L[36], Cm[9];
    CKC_UNROLL
    for (int i = 0; i < 6; i++) d[i] = st[CKR_S_WG + i];
    for (int c = 0; c < n_cams; c++) {
        if (CKR_NPTS(tab, n, c, s) <= 0) continue;
        const double *W = views + (size_t)CKR_V_STRIDE * c + CKR_V_W;
        CKC_UNROLL
        for (int i = 0; i < 6; i++) {
            CKC_UNROLL
            for (int a = 0; a < 6; a++) d[i] = d[i] + W[i * 6 + a] * dk[6 * c + a];
        }
    }
    CKC_UNROLL
    for (int i = 0; i < 6; i++) d[i] = -d[i];
    CKC_UNROLL
    for (int i = 0; i < 36; i++) L[i] = st[CKR_S_L + i];
    ckc_bwd(L, 6, d);
    double p = 0.0;
    CKC_UNROLL
    for (int i = 0; i < 6; i++) p = p + d[i] * ((lambda * ckc_scale(st[CKR_S_D + i])) * d[i] - st[CKR_S_G + i]);
    st[CKR_S_PRED] = p;
    ckr_cayley(d, Cm);
    CKC_UNROLL
    for (int i = 0; i < 3; i++) {
        const double r0 = st[CKR_S_POSE + 3 * i], r1 = st[CKR_S_POSE + 3 * i + 1], r2 = st[CKR_S_POSE + 3 * i + 2];
        CKC_UNROLL
        for (int j = 0; j < 3; j++) st[CKR_S_CAND + 3 * i + j] = (r0 * Cm[j] + r1 * Cm[3 + j]) + r2 * Cm[6 + j];
        st[CKR_S_CAND + 9 + i] = st[CKR_S_POSE + 9 + i] + d[3 + i];
    }
}

// One camera's candidate mount: A C(d_w), o + d_o.  A rotation whose three increments are frozen and a frozen component of o are
// copied, so they come back bit for bit.
CKC_FN void ckr_mount_step(const double *M, const double *dk, unsigned mask6, double *Mc) {
    double Cm[9];
    ckr_cayley(dk, Cm);
    CKC_UNROLL
    for (int i = 0; i < 3; i++) {
        const double r0 = M[3 * i], r1 = M[3 * i + 1], r2 = M[3 * i + 2];
        CKC_UNROLL
        for (int j = 0; j < 3; j++) Mc[3 * i + j] = (mask6 & 7u) == 7u ? M[3 * i + j] : (r0 * Cm[j] + r1 * Cm[3 + j]) + r2 * Cm[6 + j];
        Mc[9 + i] = ((mask6 >> (3 + i)) & 1u) ? M[9 + i] : M[9 + i] + dk[3 + i];
    }
}

// Nielsen's damping and the stop rules: ckc_lm_start / ckc_lm_decide of ck_calib_math.h with one number changed, the cost below which
// a solve is done.  There it is 1e-20 px^2; this cost is in rad^2, and 1e-20 rad^2 over the thousands of points of a capture is an rms
// of 1e-12 rad, which ends a noise-free solve one step before the mounts reach round-off.  CKR_COST_FLOOR is below what double
// precision leaves of an exact capture's cost (1e-32 per point), so such a solve ends by the relative rule or STALLED.
#define CKR_COST_FLOOR 1e-40
CKC_FN void ckr_lm_start(ckc_lm_t *s, double cost0) {
    s->lambda = 1e-3; s->nu = 2.0; s->cost = cost0;
    s->iters = 0; s->need_jac = 1;
    s->status = cost0 < CKR_COST_FLOOR ? 0 : -1;
}
CKC_FN int ckr_lm_decide(ckc_lm_t *s, int solved, double pred, double cost_new, int max_iters) {
    int accept = 0;
    double rho = 0.0;
    s->iters = s->iters + 1;
    if (solved && pred > 0.0 && ckc_finite(cost_new)) {
        rho = (s->cost - cost_new) / pred;
        accept = rho > 0.0;
    }
    if (accept) {
        const double dec = s->cost - cost_new, t = 2.0 * rho - 1.0, m = 1.0 - (t * t) * t;
        const int done = dec <= 1e-14 * s->cost || cost_new < CKR_COST_FLOOR;
        s->lambda = s->lambda * (m < 1.0 / 3.0 ? 1.0 / 3.0 : m);
        s->nu = 2.0;
        s->cost = cost_new;
        s->need_jac = 1;
        if (done) s->status = 0;
    } else {
        s->lambda = s->lambda * s->nu;
        s->nu = 2.0 * s->nu;
        s->need_jac = 0;
        if (s->lambda > 1e30) s->status = 1;
    }
    if (s->status < 0 && s->iters >= max_iters) s->status = 2;
    return accept;
}

#endif
