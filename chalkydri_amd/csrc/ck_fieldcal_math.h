// ck_fieldcal_math.h — the arithmetic of the field calibration, written once and compiled twice: as C into the host
// twin (ck_fieldcal_host.c) and as device code into k_fieldcal.hip, both with -ffp-contract=off, so the two produce the same bytes.
// What fits of ck_rigcal_math.h / ck_calib_math.h is used as it is: ckr_residual, ckr_accumulate_rows, ckr_cayley, the step record
// (CKR_S_*), ckr_lm_start / ckr_lm_decide with CKR_COST_FLOOR, ckc_chol / ckc_fwd / ckc_bwd on the 6 x 6 step blocks, ckc_scale.
//
// A pose is 12 doubles, R row-major then t: p_robot = R X + t.  A mount is 12 doubles (A, o): p_cam = A (p_robot - o).  A tag is 12
// doubles, Q row-major then c: X = Q x + c for a corner x in the tag's own frame.  A SIGHTING is one (used step, camera, tag) of 4
// points; a PAIR is one (used step, tag), the sightings of it in camera order.  A point's Jacobian has 12 columns: the tag's rotation
// increment about its own axes (0..2), the tag's position in world axes (3..5), the step's rotation increment (6..8) and the step's
// translation (9..11).
// SUMMATION ORDER (part of the contract): lane l of a group of 4 has corner l of its sighting; the 4 values are combined by the xor
// butterfly 2, 1; the sightings of a pair are added in camera order, the pairs of a step in tag order, the steps in step order, each
// sum starting from zero.  A tag that a step does not see has no pair there and is skipped, not added as zero.  Every entry of the
// reduced system is one such sum over the steps; its factorisation and the two substitutions subtract their products in a fixed order
// per entry (ck_fieldcal_host.c: reduced_solve), which does not depend on how many threads share the work.
#ifndef CK_FIELDCAL_MATH_H
#define CK_FIELDCAL_MATH_H

#include "ck_rigcal_math.h"

#define CKF_GROUP 4                      /* lanes per sighting = corners of a tag */
#define CKF_S (0.1651 / 2.0)             /* corner_points_from_center: half the tag's side */
#define CKF_LT(i, j) (((size_t)(i) * ((size_t)(i) + 1)) / 2 + (size_t)(j)) /* entry (i, j), j <= i, of a packed lower triangle */

// The record of a sighting (doubles)
enum {
    CKF_I_H = 0,                  // [78] upper triangle of J^T J of its 4 points, row by row
    CKF_I_G = CKF_I_H + CKR_NH,   // [12] J^T e
    CKF_I_COST = CKF_I_G + CKR_NJ, // [1] the candidate's squared residuals
    CKF_I_STRIDE = 92
};
// The record of a pair (doubles)
enum {
    CKF_P_H = 0,                  // [78] its sightings' sums
    CKF_P_G = CKF_P_H + CKR_NH,   // [12]
    CKF_P_W = CKF_P_G + CKR_NJ,   // [6][6] L^-1 B^T: rows = the step's increments, columns = the tag's
    CKF_P_WG = CKF_P_W + 36,      // [6]  W^T wg
    CKF_P_COST = CKF_P_WG + 6,    // [1]  the candidate's squared residuals of the pair
    CKF_P_COSTA = CKF_P_COST + 1, // [1]  the same at the accepted parameters
    CKF_P_STRIDE = 136
};

// (the driver reads the tables on the host too)
#ifdef __HIPCC__
#define CKF_HD static __host__ __device__ __forceinline__
#else
#define CKF_HD static inline
#endif

// The integer tables of one problem, laid out one after the other from `base`; U used steps, P pairs, NS sightings, T tags
typedef struct ckf_meta {
    const int32_t *used;       // [U]     the used steps' numbers in the capture
    const int32_t *step_pair;  // [U + 1] first pair of every used step
    const int32_t *pair_tag;   // [P]     the pair's tag, 0 .. T - 1
    const int32_t *pair_step;  // [P]     the pair's used step, 0 .. U - 1
    const int32_t *pair_sight; // [P + 1] first sighting of every pair
    const int32_t *sight_pair; // [NS]
    const int32_t *sight_cam;  // [NS]
    const int32_t *sight_bear; // [NS]    first of its 4 bearings
    const int32_t *pairmap;    // [T][U]  the pair of (tag, used step), -1: not seen
    const int32_t *ltag;       // [T]     the tag's entry of the layout
    const int32_t *tag_ns;     // [T]     its sightings
    const int32_t *mask6;      // [T]     its frozen increments
} ckf_meta_t;
CKF_HD size_t ckf_meta_size(size_t U, size_t P, size_t NS, size_t T) { return 2 * U + 1 + 3 * P + 1 + 3 * NS + T * U + 3 * T; }
CKF_HD ckf_meta_t ckf_meta_at(const int32_t *base, size_t U, size_t P, size_t NS, size_t T) {
    ckf_meta_t m;
    m.used = base; m.step_pair = m.used + U; m.pair_tag = m.step_pair + U + 1; m.pair_step = m.pair_tag + P;
    m.pair_sight = m.pair_step + P; m.sight_pair = m.pair_sight + P + 1; m.sight_cam = m.sight_pair + NS;
    m.sight_bear = m.sight_cam + NS; m.pairmap = m.sight_bear + NS; m.ltag = m.pairmap + T * U; m.tag_ns = m.ltag + T;
    m.mask6 = m.tag_ns + T;
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
    double x[3], X[3], q[3], p[3];
    ckf_corner(j, x);
    ckf_world(T, x, X);
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
    // G = de / dp as in ckr_jacobian;  GA = G A = de / dt;  GR = GA R = de / dX = de / dc;  GQ = GR Q
    double G[9], GA[9], GR[9], GQ[9];
    CKC_UNROLL
    for (int i = 0; i < 3; i++) {
        CKC_UNROLL
        for (int k = 0; k < 3; k++) G[3 * i + k] = ((i == k ? 1.0 : 0.0) - (v[i] * v[k]) / vv) / s - (e[i] * p[k]) / pp;
    }
    CKC_UNROLL
    for (int i = 0; i < 3; i++) {
        CKC_UNROLL
        for (int k = 0; k < 3; k++) GA[3 * i + k] = G[3 * i] * M[k] + G[3 * i + 1] * M[3 + k] + G[3 * i + 2] * M[6 + k];
    }
    CKC_UNROLL
    for (int i = 0; i < 3; i++) {
        CKC_UNROLL
        for (int k = 0; k < 3; k++) GR[3 * i + k] = GA[3 * i] * P[k] + GA[3 * i + 1] * P[3 + k] + GA[3 * i + 2] * P[6 + k];
    }
    CKC_UNROLL
    for (int i = 0; i < 3; i++) {
        CKC_UNROLL
        for (int k = 0; k < 3; k++) GQ[3 * i + k] = GR[3 * i] * T[k] + GR[3 * i + 1] * T[3 + k] + GR[3 * i + 2] * T[6 + k];
    }
    // Q C(dw) x = Q (x + dw x x) and R C(dw) X = R (X + dw x X): the columns of d(dw x y) / d(dw) are (0, -y2, y1), (y2, 0, -y0), (-y1, y0, 0)
    CKC_UNROLL
    for (int i = 0; i < 3; i++) {
        double *Ji = J + CKR_NJ * i;
        Ji[0] = GQ[3 * i + 2] * x[1] - GQ[3 * i + 1] * x[2];
        Ji[1] = GQ[3 * i] * x[2] - GQ[3 * i + 2] * x[0];
        Ji[2] = GQ[3 * i + 1] * x[0] - GQ[3 * i] * x[1];
        Ji[3] = GR[3 * i]; Ji[4] = GR[3 * i + 1]; Ji[5] = GR[3 * i + 2];
        Ji[6] = GR[3 * i + 2] * X[1] - GR[3 * i + 1] * X[2];
        Ji[7] = GR[3 * i] * X[2] - GR[3 * i + 2] * X[0];
        Ji[8] = GR[3 * i + 1] * X[0] - GR[3 * i] * X[1];
        Ji[9] = GA[3 * i]; Ji[10] = GA[3 * i + 1]; Ji[11] = GA[3 * i + 2];
        CKC_UNROLL
        for (int a = 0; a < 6; a++)
            if ((mask6 >> a) & 1u) Ji[a] = 0.0;
    }
}

// A pair's normal equations: its n sightings' records (consecutive, in camera order) added from zero
CKC_FN void ckf_pair_sum(double *pr, const double *sights, int n) {
    for (int j = 0; j < CKR_NH + CKR_NJ; j++) {
        double t = 0.0;
        for (int i = 0; i < n; i++) t = t + sights[(size_t)CKF_I_STRIDE * i + CKF_I_H + j];
        pr[CKF_P_H + j] = t;
    }
}

// A used step's candidate cost: per pair its n sightings in camera order, then the step's np pairs (consecutive records, in tag order)
CKC_FN void ckf_step_cost(double *st, double *pairs, const double *sights, const int32_t *pair_sight, int np) {
    double cs = 0.0;
    for (int k = 0; k < np; k++) {
        double t = 0.0;
        for (int i = pair_sight[k]; i < pair_sight[k + 1]; i++) t = t + sights[(size_t)CKF_I_STRIDE * (i - pair_sight[0]) + CKF_I_COST];
        pairs[(size_t)CKF_P_STRIDE * k + CKF_P_COST] = t;
        cs = cs + t;
    }
    st[CKR_S_COST] = cs;
}

// One used step's part of the Schur complement at damping lambda: A_s and g_s are its np pairs' step blocks added in tag order,
// L = chol(A_s + lambda D_s), wg = L^-1 g_s, and per pair W = L^-1 B^T and W^T wg.  0 when the factorisation fails.
CKC_FN int ckf_step_schur(double *st, double *pairs, int np, double lambda) {
    double L[36], wg[6];
    CKC_UNROLL
    for (int i = 0; i < 36; i++) L[i] = 0.0;
    CKC_UNROLL
    for (int i = 0; i < 6; i++) wg[i] = 0.0;
    for (int k = 0; k < np; k++) {
        const double *V = pairs + (size_t)CKF_P_STRIDE * k;
        CKC_UNROLL
        for (int i = 0; i < 6; i++) {
            CKC_UNROLL
            for (int j = 0; j <= i; j++) L[i * 6 + j] = L[i * 6 + j] + V[CKF_P_H + CKR_TRI(6 + j, 6 + i)];
            wg[i] = wg[i] + V[CKF_P_G + 6 + i];
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
    for (int k = 0; k < np; k++) {
        double *V = pairs + (size_t)CKF_P_STRIDE * k;
        double W[36];
        CKC_UNROLL
        for (int i = 0; i < 6; i++) {
            CKC_UNROLL
            for (int a = 0; a < 6; a++) W[i * 6 + a] = V[CKF_P_H + CKR_TRI(a, 6 + i)];
        }
        CKC_UNROLL
        for (int a = 0; a < 6; a++) ckc_fwd(L, 6, W + a, 6);
        CKC_UNROLL
        for (int i = 0; i < 36; i++) V[CKF_P_W + i] = W[i];
        CKC_UNROLL
        for (int a = 0; a < 6; a++) {
            double t = 0.0;
            CKC_UNROLL
            for (int i = 0; i < 6; i++) t = t + W[i * 6 + a] * wg[i];
            V[CKF_P_WG + a] = t;
        }
    }
    return ok;
}

// Entry j of tag k's own sums over the used steps that see it, in step order: j < 21 the upper triangle of its 6 x 6 block row by
// row, then J^T e (6).  map = the tag's row of pairmap.
CKC_FN double ckf_tag_sum(const double *pairs, const int32_t *map, int U, int j) {
    int off = CKF_P_G + (j - 21);
    if (j < 21) {
        int a = 0, k = j;
        while (k >= 6 - a) { k -= 6 - a; a++; }
        off = CKF_P_H + CKR_TRI(a, a + k);
    }
    double t = 0.0;
    for (int u = 0; u < U; u++)
        if (map[u] >= 0) t = t + pairs[(size_t)CKF_P_STRIDE * map[u] + off];
    return t;
}
#define CKF_HK 27
#define CKF_HK_DIAG(a) ((a) * 6 - ((a) * ((a) - 1)) / 2)

// Entry (r, k), k <= r, of the reduced system of N = 6 T unknowns at damping lambda: [same tag](the tag's own sum + lambda D) minus
// what the elimination of the steps takes, the sum of W_r . W_k over the used steps that see both tags, in step order; a frozen
// unknown has the row and column of the identity.  Hk = the tags' own sums [T][27].  The steps walked are list[0 .. n - 1], increasing
// (the twin hands over the steps that see both tags, found once per pair of tags), or with list = null all of 0 .. n - 1 (the kernel):
// a step that does not see both adds nothing either way, so the sum is the same.
CKC_FN double ckf_reduced_entry(const double *pairs, const int32_t *pairmap, const int32_t *mask6, const double *Hk, int U, const int32_t *list,
                                int n, double lambda, int r, int k) {
    const int tr = r / 6, a = r % 6, tk = k / 6, b = k % 6;
    if (((mask6[tr] >> a) & 1) || ((mask6[tk] >> b) & 1)) return r == k ? 1.0 : 0.0;
    const int32_t *mr = pairmap + (size_t)tr * U, *mk = pairmap + (size_t)tk * U;
    double E = 0.0;
    for (int i = 0; i < n; i++) {
        const int u = list ? list[i] : i;
        if (mr[u] < 0 || mk[u] < 0) continue;
        const double *W1 = pairs + (size_t)CKF_P_STRIDE * mr[u] + CKF_P_W + a, *W2 = pairs + (size_t)CKF_P_STRIDE * mk[u] + CKF_P_W + b;
        double w = 0.0;
        CKC_UNROLL
        for (int j = 0; j < 6; j++) w = w + W1[6 * j] * W2[6 * j];
        E = E + w;
    }
    double t = 0.0;
    if (tr == tk) {
        t = Hk[CKF_HK * tr + CKF_HK_DIAG(b) + (a - b)];
        if (r == k) t = t + lambda * ckc_scale(t);
    }
    return t - E;
}
// Entry r of its right-hand side: the sum of W^T wg over the steps that see the tag, minus the tag's own J^T e; 0 when frozen
CKC_FN double ckf_reduced_rhs(const double *pairs, const int32_t *pairmap, const int32_t *mask6, const double *Hk, int U, int r) {
    const int tr = r / 6, a = r % 6;
    if ((mask6[tr] >> a) & 1) return 0.0;
    const int32_t *mr = pairmap + (size_t)tr * U;
    double t = 0.0;
    for (int u = 0; u < U; u++)
        if (mr[u] >= 0) t = t + pairs[(size_t)CKF_P_STRIDE * mr[u] + CKF_P_WG + a];
    return t - Hk[CKF_HK * tr + 21 + a];
}
// The tags' share of the predicted decrease, and the frozen increments set to exactly zero
CKC_FN double ckf_reduced_pred(const int32_t *mask6, const double *Hk, int N, double lambda, double *dk) {
    double p = 0.0;
    for (int r = 0; r < N; r++) {
        const int a = r % 6;
        if ((mask6[r / 6] >> a) & 1) dk[r] = 0.0;
        p = p + dk[r] * ((lambda * ckc_scale(Hk[CKF_HK * (r / 6) + CKF_HK_DIAG(a)])) * dk[r] - Hk[CKF_HK * (r / 6) + 21 + a]);
    }
    return p;
}

// One step's increment given the tags': d_s = -L^-T (wg + sum_k W_k dk_k), its np pairs in tag order; the candidate pose R C(d_w),
// t + d_t; the step's share of the predicted decrease.
CKC_FN void ckf_step_step(double *st, const double *pairs, const int32_t *pair_tag, int np, const double *dk, double lambda) {
    double d[6], L[36], Cm[9];
    CKC_UNROLL
    for (int i = 0; i < 6; i++) d[i] = st[CKR_S_WG + i];
    for (int k = 0; k < np; k++) {
        const double *W = pairs + (size_t)CKF_P_STRIDE * k + CKF_P_W;
        const double *dt = dk + 6 * pair_tag[k];
        CKC_UNROLL
        for (int i = 0; i < 6; i++) {
            CKC_UNROLL
            for (int a = 0; a < 6; a++) d[i] = d[i] + W[i * 6 + a] * dt[a];
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

// One tag's candidate pose: Q C(d_w), c + d_c.  A rotation whose three increments are frozen and a frozen component of c are copied,
// so they come back bit for bit.
CKC_FN void ckf_tag_step(const double *T, const double *dk, unsigned mask6, double *Tc) {
    double Cm[9];
    ckr_cayley(dk, Cm);
    CKC_UNROLL
    for (int i = 0; i < 3; i++) {
        const double r0 = T[3 * i], r1 = T[3 * i + 1], r2 = T[3 * i + 2];
        CKC_UNROLL
        for (int j = 0; j < 3; j++) Tc[3 * i + j] = (mask6 & 7u) == 7u ? T[3 * i + j] : (r0 * Cm[j] + r1 * Cm[3 + j]) + r2 * Cm[6 + j];
        Tc[9 + i] = ((mask6 >> (3 + i)) & 1u) ? T[9 + i] : T[9 + i] + dk[3 + i];
    }
}

// A tag's rms at the accepted parameters: its pairs' costs over the used steps in step order, over 4 points per sighting
CKC_FN double ckf_tag_rms(const double *pairs, const int32_t *map, int U, int n_sightings) {
    double t = 0.0;
    for (int u = 0; u < U; u++)
        if (map[u] >= 0) t = t + pairs[(size_t)CKF_P_STRIDE * map[u] + CKF_P_COSTA];
    return sqrt(t / (double)(4 * n_sightings));
}

#endif
