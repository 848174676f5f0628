// ck_cal_math.h — what the mount calibration and the field calibration (§4m) share of their arithmetic: one solver with
// two residuals.  Both minimise bearing residuals over a few 6-vector COLUMNS that every step sees (camera mounts there, tag poses
// here) and one robot pose per used STEP; a BLOCK is one (used step, column) that has points: a view of §4l, a pair of §4m.  The steps
// are eliminated (6 x 6 each) and the columns' reduced system is solved; the normal equations are an arrowhead.  Written once and
// compiled four times: as C into the two host twins and as device code into the two kernels, -ffp-contract=off everywhere, so all
// return the same bytes.  From ck_calib_math.h: ckc_finite, ckc_scale, ckc_chol / ckc_fwd / ckc_bwd, ckc_rigid_step, ckc_lm_t.
//
// A point's Jacobian has 12 columns: the column's six increments (0..5, each solver's own) and the step's (6..11: rotation increment
// about robot axes, translation).  SUMMATION ORDER (part of the contract): the blocks of a step are added in column order, the steps
// in step order, every sum from zero; a column that a step has no block for is skipped, not added as zero.
#ifndef CK_CAL_MATH_H
#define CK_CAL_MATH_H

#include <stddef.h>
#include <stdint.h>

#include "ck_calib_math.h"

#define CKA_NJ 12                 /* columns of one point's Jacobian */
#define CKA_NH 78                 /* upper triangle of NJ x NJ */
#define CKA_NACC (CKA_NH + CKA_NJ)
#define CKA_TRI(a, b) ((a) * CKA_NJ - ((a) * ((a) - 1)) / 2 + ((b) - (a))) /* a <= b */
#define CKA_HK 27                 /* a column's own sums: the upper triangle of its 6 x 6 block row by row (21), then J^T e (6) */
#define CKA_HK_DIAG(a) ((a) * 6 - ((a) * ((a) - 1)) / 2)

// The record of a block (doubles); a device workspace layout, nothing outside the solvers reads it
enum {
    CKA_B_H = 0,                  // [78] upper triangle of J^T J of its points, row by row
    CKA_B_G = CKA_B_H + CKA_NH,   // [12] J^T e
    CKA_B_COST = CKA_B_G + CKA_NJ, // [1] the candidate's squared residuals of this block
    CKA_B_COSTA = CKA_B_COST + 1, // [1] the same at the accepted parameters
    CKA_B_W = CKA_B_COSTA + 1,    // [6][6] L^-1 B^T: rows = the step's increments, columns = the column's
    CKA_B_WG = CKA_B_W + 36,      // [6]  W^T wg
    CKA_B_STRIDE = 136
};
// The record of a used step (doubles)
enum {
    CKA_S_POSE = 0,               // [12] accepted
    CKA_S_CAND = 12,              // [12] candidate
    CKA_S_L = 24,                 // [36] Cholesky factor of A_s + lambda D_s, lower triangle of a 6 x 6
    CKA_S_WG = 60,                // [6]  L^-1 g_s
    CKA_S_D = 66,                 // [6]  diagonal of A_s
    CKA_S_G = 72,                 // [6]  g_s
    CKA_S_PRED = 78,              // [1]  the step's share of the predicted decrease
    CKA_S_COST = 79,              // [1]  the candidate's squared residuals of this step
    CKA_S_STRIDE = 80
};

// (the drivers read the tables on the host too)
#ifdef __HIPCC__
#define CKA_HD static __host__ __device__ __forceinline__
#else
#define CKA_HD static inline
#endif

// The arrowhead index of one problem, int32 tables laid out one after the other from `base`: U used steps, P blocks (step by step,
// in column order within a step), NC columns.  Both planners fill it; both kernels and both twins read it.
typedef struct cka_index {
    const int32_t *used;   // [U]      the used steps' numbers in the capture
    const int32_t *first;  // [U + 1]  first block of every used step
    const int32_t *col;    // [P]      the block's column, 0 .. NC - 1
    const int32_t *step;   // [P]      the block's used step, 0 .. U - 1
    const int32_t *colmap; // [NC][U]  the block of (column, used step), -1: none
} cka_index_t;
CKA_HD size_t cka_index_size(size_t U, size_t P, size_t NC) { return 2 * U + 1 + 2 * P + NC * U; }
CKA_HD cka_index_t cka_index_at(const int32_t *base, size_t U, size_t P) {
    cka_index_t x;
    x.used = base; x.first = x.used + U; x.col = x.first + U + 1; x.step = x.col + P; x.colmap = x.step + P;
    return x;
}

// The shared part of a point's residual and Jacobian: world point X seen along v by the camera mounted by M (A row-major, o: p_cam =
// A (p_robot - o)) at the step with pose P (p_robot = R X + t).  e[3] the residual, q = p_robot - o, GA = de / dt, GR = GA R = de / dX,
// and the step's columns 6..11 of the rows J[3][12]; the caller adds its columns 0..5 (cka_freeze_columns after them).  The nine
// arrays are distinct: where a twin's compiler keeps this function out of line, it need not reload an input after every store.
CKC_FN void cka_point(const double *__restrict__ M, const double *__restrict__ P, const double *__restrict__ X, const double *__restrict__ v, double *__restrict__ e,
                    double *__restrict__ q, double *__restrict__ GA, double *__restrict__ GR, double *__restrict__ J) {
    double p[3], G[9];
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
    // G = de / dp = (I - v v^T / v.v) / |p| - e p^T / p.p
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
    // R C(dw) X = R (X + dw x X): the columns of d(dw x y) / d(dw) are (0, -y2, y1), (y2, 0, -y0), (-y1, y0, 0)
    CKC_UNROLL
    for (int i = 0; i < 3; i++) {
        double *Ji = J + CKA_NJ * i;
        Ji[6] = GR[3 * i + 2] * X[1] - GR[3 * i + 1] * X[2];
        Ji[7] = GR[3 * i] * X[2] - GR[3 * i + 2] * X[0];
        Ji[8] = GR[3 * i + 1] * X[0] - GR[3 * i] * X[1];
        Ji[9] = GA[3 * i]; Ji[10] = GA[3 * i + 1]; Ji[11] = GA[3 * i + 2];
    }
}
// the column's frozen increments (bits 0..5 of mask6): their Jacobian columns are zero
CKC_FN void cka_freeze_columns(double *J, unsigned mask6) {
    CKC_UNROLL
    for (int i = 0; i < 3; i++) {
        CKC_UNROLL
        for (int a = 0; a < 6; a++)
            if ((mask6 >> a) & 1u) J[CKA_NJ * i + a] = 0.0;
    }
}

// One used step's part of the Schur complement at damping lambda.  st = the step's record, blocks = the records of its nb blocks
// (consecutive, in column order).  A_s and g_s are the blocks' step parts added in that order; L = chol(A_s + lambda D_s), wg = L^-1
// g_s, and per block W = L^-1 B^T and W^T wg.  0 when the factorisation fails.
CKC_FN int cka_step_schur(double *st, double *blocks, int nb, double lambda) {
    double L[36], wg[6];
    CKC_UNROLL
    for (int i = 0; i < 36; i++) L[i] = 0.0;
    CKC_UNROLL
    for (int i = 0; i < 6; i++) wg[i] = 0.0;
    for (int k = 0; k < nb; k++) {
        const double *V = blocks + (size_t)CKA_B_STRIDE * k;
        CKC_UNROLL
        for (int i = 0; i < 6; i++) {
            CKC_UNROLL
            for (int j = 0; j <= i; j++) L[i * 6 + j] = L[i * 6 + j] + V[CKA_B_H + CKA_TRI(6 + j, 6 + i)];
            wg[i] = wg[i] + V[CKA_B_G + 6 + i];
        }
    }
    CKC_UNROLL
    for (int i = 0; i < 6; i++) {
        st[CKA_S_D + i] = L[i * 6 + i];
        st[CKA_S_G + i] = wg[i];
        L[i * 6 + i] = L[i * 6 + i] + lambda * ckc_scale(L[i * 6 + i]);
    }
    const int ok = ckc_chol(L, 6);
    ckc_fwd(L, 6, wg, 1);
    CKC_UNROLL
    for (int i = 0; i < 36; i++) st[CKA_S_L + i] = L[i];
    CKC_UNROLL
    for (int i = 0; i < 6; i++) st[CKA_S_WG + i] = wg[i];
    for (int k = 0; k < nb; k++) {
        double *V = blocks + (size_t)CKA_B_STRIDE * k;
        double W[36];
        CKC_UNROLL
        for (int i = 0; i < 6; i++) {
            CKC_UNROLL
            for (int a = 0; a < 6; a++) W[i * 6 + a] = V[CKA_B_H + CKA_TRI(a, 6 + i)];
        }
        CKC_UNROLL
        for (int a = 0; a < 6; a++) ckc_fwd(L, 6, W + a, 6);
        CKC_UNROLL
        for (int i = 0; i < 36; i++) V[CKA_B_W + i] = W[i];
        CKC_UNROLL
        for (int a = 0; a < 6; a++) {
            double t = 0.0;
            CKC_UNROLL
            for (int i = 0; i < 6; i++) t = t + W[i * 6 + a] * wg[i];
            V[CKA_B_WG + a] = t;
        }
    }
    return ok;
}

// One step's increment given the columns': d_s = -L^-T (wg + sum_k W_k dk_col[k]), its nb blocks in order (col = their columns); the
// candidate pose R C(d_w), t + d_t; the step's share of the predicted decrease.
CKC_FN void cka_step_step(double *st, const double *blocks, const int32_t *col, int nb, const double *dk, double lambda) {
    double d[6], L[36];
    CKC_UNROLL
    for (int i = 0; i < 6; i++) d[i] = st[CKA_S_WG + i];
    for (int k = 0; k < nb; k++) {
        const double *W = blocks + (size_t)CKA_B_STRIDE * k + CKA_B_W;
        const double *dc = dk + 6 * col[k];
        CKC_UNROLL
        for (int i = 0; i < 6; i++) {
            CKC_UNROLL
            for (int a = 0; a < 6; a++) d[i] = d[i] + W[i * 6 + a] * dc[a];
        }
    }
    CKC_UNROLL
    for (int i = 0; i < 6; i++) d[i] = -d[i];
    CKC_UNROLL
    for (int i = 0; i < 36; i++) L[i] = st[CKA_S_L + i];
    ckc_bwd(L, 6, d);
    double p = 0.0;
    CKC_UNROLL
    for (int i = 0; i < 6; i++) p = p + d[i] * ((lambda * ckc_scale(st[CKA_S_D + i])) * d[i] - st[CKA_S_G + i]);
    st[CKA_S_PRED] = p;
    ckc_rigid_step(st + CKA_S_POSE, d, 0u, st + CKA_S_CAND);
}

// Entry j < CKA_HK of a column's own sums over the used steps that have a block of it, in step order.  map = its row of colmap.
CKC_FN double cka_col_sum(const double *blocks, const int32_t *map, int U, int j) {
    int off = CKA_B_G + (j - 21);
    if (j < 21) {
        int a = 0, k = j;
        while (k >= 6 - a) { k -= 6 - a; a++; }
        off = CKA_B_H + CKA_TRI(a, a + k);
    }
    double t = 0.0;
    for (int u = 0; u < U; u++)
        if (map[u] >= 0) t = t + blocks[(size_t)CKA_B_STRIDE * map[u] + off];
    return t;
}
// A column's rms at the accepted parameters: its blocks' costs over the used steps in step order, over its n_points points
CKC_FN double cka_col_rms(const double *blocks, const int32_t *map, int U, int n_points) {
    double t = 0.0;
    for (int u = 0; u < U; u++)
        if (map[u] >= 0) t = t + blocks[(size_t)CKA_B_STRIDE * map[u] + CKA_B_COSTA];
    return sqrt(t / (double)n_points);
}

// Entry (r, k), k <= r, of the reduced system of N = 6 NC unknowns at damping lambda: [same column](the column's own sum + lambda D)
// minus what the elimination of the steps takes, the sum of W_r . W_k over the used steps that have both columns, in step order; a
// frozen unknown (mask6 = the columns' masks) has the row and column of the identity.  Hk = the columns' own sums [NC][CKA_HK].  The
// steps walked are list[0 .. n - 1], increasing (a twin may hand over the steps that have both columns, found once per pair of
// columns), or with list = null all of 0 .. n - 1: a step that does not have both adds nothing either way, so the sum is the same.
CKC_FN double cka_reduced_entry(const double *blocks, const int32_t *colmap, const int32_t *mask6, const double *Hk, int U, const int32_t *list,
                                int n, double lambda, int r, int k) {
    const int tr = r / 6, a = r % 6, tk = k / 6, b = k % 6;
    if (((mask6[tr] >> a) & 1) || ((mask6[tk] >> b) & 1)) return r == k ? 1.0 : 0.0;
    const int32_t *mr = colmap + (size_t)tr * U, *mk = colmap + (size_t)tk * U;
    double E = 0.0;
    for (int i = 0; i < n; i++) {
        const int u = list ? list[i] : i;
        if (mr[u] < 0 || mk[u] < 0) continue;
        const double *W1 = blocks + (size_t)CKA_B_STRIDE * mr[u] + CKA_B_W + a, *W2 = blocks + (size_t)CKA_B_STRIDE * mk[u] + CKA_B_W + b;
        double w = 0.0;
        CKC_UNROLL
        for (int j = 0; j < 6; j++) w = w + W1[6 * j] * W2[6 * j];
        E = E + w;
    }
    double t = 0.0;
    if (tr == tk) {
        t = Hk[CKA_HK * tr + CKA_HK_DIAG(b) + (a - b)];
        if (r == k) t = t + lambda * ckc_scale(t);
    }
    return t - E;
}
// Entry r of its right-hand side: the sum of W^T wg over the steps that have the column, minus the column's own J^T e; 0 when frozen
CKC_FN double cka_reduced_rhs(const double *blocks, const int32_t *colmap, const int32_t *mask6, const double *Hk, int U, int r) {
    const int tr = r / 6, a = r % 6;
    if ((mask6[tr] >> a) & 1) return 0.0;
    const int32_t *mr = colmap + (size_t)tr * U;
    double t = 0.0;
    for (int u = 0; u < U; u++)
        if (mr[u] >= 0) t = t + blocks[(size_t)CKA_B_STRIDE * mr[u] + CKA_B_WG + a];
    return t - Hk[CKA_HK * tr + 21 + a];
}
// The columns' share of the predicted decrease, and the frozen increments set to exactly zero
CKC_FN double cka_reduced_pred(const int32_t *mask6, const double *Hk, int N, double lambda, double *dk) {
    double p = 0.0;
    for (int r = 0; r < N; r++) {
        const int a = r % 6;
        if ((mask6[r / 6] >> a) & 1) dk[r] = 0.0;
        p = p + dk[r] * ((lambda * ckc_scale(Hk[CKA_HK * (r / 6) + CKA_HK_DIAG(a)])) * dk[r] - Hk[CKA_HK * (r / 6) + 21 + a]);
    }
    return p;
}
// The row r of entry e = r (r + 1) / 2 + k, k <= r, of a lower triangle stored row by row (how the kernels' threads share the entries)
CKC_FN int cka_lt_row(int e) {
    int r = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
    while ((r * (r + 1)) / 2 > e) r--;
    while (((r + 1) * (r + 2)) / 2 <= e) r++;
    return r;
}
// The two reduced solves stay apart on purpose.  §4l's (at most 48 unknowns, one thread, dense in LDS) is ckc_chol_n / ckc_fwd_n / ckc_bwd_n,
// whose backward substitution subtracts its products in increasing c; §4m's (up to 384 unknowns, the whole workgroup) sweeps the
// columns in parallel, which reaches a row's products in decreasing c.  One order for both would change one solver's bytes.

#endif
