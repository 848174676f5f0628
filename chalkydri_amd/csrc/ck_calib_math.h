// ck_calib_math.h — the arithmetic of the intrinsic calibration, written once and compiled twice: as C into the host
// twin (ck_calib_host.c) and as device code into k_calib.hip.  Only + - * / sqrt on doubles, every expression evaluated as written
// (-ffp-contract=off on both sides), so the two produce the same bytes.  What differs between the two sides is only who walks the
// observations and the frames; the order in which sums are formed is fixed here and in the two walkers (see ckc_accumulate).
//
// Parameters: k[9] = fx fy cx cy k1 k2 p1 p2 k3 (ck_opencv5_t's order); a pose is 12 doubles, R row-major then t.
// Normal equations of one frame, 135 doubles: the upper triangle of the 15 x 15 matrix J^T J over the columns (9 intrinsics, 3
// rotation, 3 translation) row by row (120), then J^T r (15).  Every local array is indexed by constants once the loops are
// unrolled: a runtime-indexed local array would live in scratch memory on the device.
#ifndef CK_CALIB_MATH_H
#define CK_CALIB_MATH_H

#include <math.h>

#if defined(__HIPCC__)
#define CKC_FN static __device__ __forceinline__
#define CKC_HOST_FN static __host__ __device__ __forceinline__ /* what the launching host code asks too */
#define CKC_UNROLL _Pragma("unroll")
#else
#define CKC_FN static inline
#define CKC_HOST_FN static inline
#define CKC_UNROLL
#endif

#define CKC_NK 9                  /* intrinsics */
#define CKC_NP 6                  /* pose increments: rotation, translation */
#define CKC_NJ (CKC_NK + CKC_NP)  /* columns of one observation's Jacobian */
#define CKC_NH 120                /* upper triangle of NJ x NJ */
#define CKC_NACC (CKC_NH + CKC_NJ)
#define CKC_TRI(a, b) ((a) * CKC_NJ - ((a) * ((a) - 1)) / 2 + ((b) - (a))) /* a <= b */

// The per-frame record both walkers keep (doubles): the frame's normal equations, the factor of its damped pose block, what the
// Schur complement takes from it, its accepted and its candidate pose, its share of the predicted decrease and its cost.
enum {
    CKC_WS_H = 0,                       // [135] normal equations (ckc_accumulate's layout)
    CKC_WS_L = CKC_WS_H + CKC_NACC,     // [36]  Cholesky factor of A_f + lambda D_f, lower triangle of a 6 x 6
    CKC_WS_W = CKC_WS_L + 36,           // [6][9] L^-1 B_f^T
    CKC_WS_WG = CKC_WS_W + 54,          // [6]   L^-1 g_f
    CKC_WS_E = CKC_WS_WG + 6,           // [54]  W^T W (upper triangle of 9 x 9, row by row: 45), W^T wg (9)
    CKC_WS_POSE = CKC_WS_E + 54,        // [12]
    CKC_WS_CAND = CKC_WS_POSE + 12,     // [12]
    CKC_WS_PRED = CKC_WS_CAND + 12,     // [1]   sum over the frame's six increments of d (lambda D d - g)
    CKC_WS_COST = CKC_WS_PRED + 1,      // [1]   the candidate's squared residuals of this frame
    CKC_WS_STRIDE = 312
};

CKC_FN int ckc_finite(double x) { return x - x == 0.0; }

// residual of one observation: board point (X, Y, 0) under pose P seen at (u, v)
CKC_FN void ckc_residual(const double *k, const double *P, double X, double Y, double u, double v, double *r) {
    const double Px = P[0] * X + P[1] * Y + P[9], Py = P[3] * X + P[4] * Y + P[10], Pz = P[6] * X + P[7] * Y + P[11];
    const double x = Px / Pz, y = Py / Pz;
    const double r2 = x * x + y * y;
    const double rad = 1.0 + r2 * (k[4] + r2 * (k[5] + r2 * k[8]));
    const double xy2 = (2.0 * x) * y;
    const double xd = x * rad + k[6] * xy2 + k[7] * (r2 + (2.0 * x) * x);
    const double yd = y * rad + k[6] * (r2 + (2.0 * y) * y) + k[7] * xy2;
    r[0] = k[0] * xd + k[2] - u;
    r[1] = k[1] * yd + k[3] - v;
}

// residual and the two Jacobian rows at a zero pose increment; the columns of frozen intrinsics (bits of fixed_mask) are zero
CKC_FN void ckc_jacobian(const double *k, const double *P, double X, double Y, double u, double v, unsigned fixed_mask, double *r,
                         double *Ju, double *Jv) {
    const double Px = P[0] * X + P[1] * Y + P[9], Py = P[3] * X + P[4] * Y + P[10], Pz = P[6] * X + P[7] * Y + P[11];
    const double x = Px / Pz, y = Py / Pz, iz = 1.0 / Pz;
    const double r2 = x * x + y * y;
    const double rad = 1.0 + r2 * (k[4] + r2 * (k[5] + r2 * k[8]));
    const double xy2 = (2.0 * x) * y;
    const double ax = r2 + (2.0 * x) * x, ay = r2 + (2.0 * y) * y;
    const double xd = x * rad + k[6] * xy2 + k[7] * ax;
    const double yd = y * rad + k[6] * ay + k[7] * xy2;
    r[0] = k[0] * xd + k[2] - u;
    r[1] = k[1] * yd + k[3] - v;
    const double r4 = r2 * r2, r6 = r4 * r2;
    Ju[0] = xd; Ju[1] = 0.0; Ju[2] = 1.0; Ju[3] = 0.0;
    Ju[4] = k[0] * (x * r2); Ju[5] = k[0] * (x * r4); Ju[6] = k[0] * xy2; Ju[7] = k[0] * ax; Ju[8] = k[0] * (x * r6);
    Jv[0] = 0.0; Jv[1] = yd; Jv[2] = 0.0; Jv[3] = 1.0;
    Jv[4] = k[1] * (y * r2); Jv[5] = k[1] * (y * r4); Jv[6] = k[1] * ay; Jv[7] = k[1] * xy2; Jv[8] = k[1] * (y * r6);
    CKC_UNROLL
    for (int i = 0; i < CKC_NK; i++)
        if ((fixed_mask >> i) & 1u) { Ju[i] = 0.0; Jv[i] = 0.0; }
    // d(xd, yd) / d(x, y)
    const double dr = k[4] + r2 * (2.0 * k[5] + (3.0 * k[8]) * r2);
    const double xdx = rad + ((2.0 * x) * x) * dr + (2.0 * k[6]) * y + (6.0 * k[7]) * x;
    const double xdy = xy2 * dr + (2.0 * k[6]) * x + (2.0 * k[7]) * y;
    const double ydy = rad + ((2.0 * y) * y) * dr + (6.0 * k[6]) * y + (2.0 * k[7]) * x;
    // d(u, v) / d(camera point)
    double du[3], dv[3];
    du[0] = k[0] * (xdx * iz); du[1] = k[0] * (xdy * iz); du[2] = -(k[0] * ((xdx * x + xdy * y) * iz));
    dv[0] = k[1] * (xdy * iz); dv[1] = k[1] * (ydy * iz); dv[2] = -(k[1] * ((xdy * x + ydy * y) * iz));
    // d(camera point) / d(rotation increment) = -R [X]x: columns Y c2, -X c2, X c1 - Y c0 of R's columns c0 c1 c2
    CKC_UNROLL
    for (int i = 0; i < 3; i++) {
        Ju[12 + i] = du[i];
        Jv[12 + i] = dv[i];
    }
    double w0[3], w1[3], w2[3];
    CKC_UNROLL
    for (int i = 0; i < 3; i++) {
        w0[i] = Y * P[3 * i + 2];
        w1[i] = -(X * P[3 * i + 2]);
        w2[i] = X * P[3 * i + 1] - Y * P[3 * i];
    }
    Ju[9] = du[0] * w0[0] + du[1] * w0[1] + du[2] * w0[2];
    Ju[10] = du[0] * w1[0] + du[1] * w1[1] + du[2] * w1[2];
    Ju[11] = du[0] * w2[0] + du[1] * w2[1] + du[2] * w2[2];
    Jv[9] = dv[0] * w0[0] + dv[1] * w0[1] + dv[2] * w0[2];
    Jv[10] = dv[0] * w1[0] + dv[1] * w1[1] + dv[2] * w1[2];
    Jv[11] = dv[0] * w2[0] + dv[1] * w2[1] + dv[2] * w2[2];
}

// The six pose columns of an observation's Jacobian from d(u, v) / d(camera point), as ckc_jacobian forms them (its text is left as it
// is: the OpenCVModel5 kernel's code must not move)
CKC_FN void ckc_pose_columns(const double *P, double X, double Y, const double *du, const double *dv, double *Ju, double *Jv) {
    CKC_UNROLL
    for (int i = 0; i < 3; i++) {
        Ju[12 + i] = du[i];
        Jv[12 + i] = dv[i];
    }
    double w0[3], w1[3], w2[3];
    CKC_UNROLL
    for (int i = 0; i < 3; i++) {
        w0[i] = Y * P[3 * i + 2];
        w1[i] = -(X * P[3 * i + 2]);
        w2[i] = X * P[3 * i + 1] - Y * P[3 * i];
    }
    Ju[9] = du[0] * w0[0] + du[1] * w0[1] + du[2] * w0[2];
    Ju[10] = du[0] * w1[0] + du[1] * w1[1] + du[2] * w1[2];
    Ju[11] = du[0] * w2[0] + du[1] * w2[1] + du[2] * w2[2];
    Jv[9] = dv[0] * w0[0] + dv[1] * w0[1] + dv[2] * w0[2];
    Jv[10] = dv[0] * w1[0] + dv[1] * w1[1] + dv[2] * w1[2];
    Jv[11] = dv[0] * w2[0] + dv[1] * w2[1] + dv[2] * w2[2];
}

// ---- EUCM / UCM ----------------------------------------------------------------------------------------------
// k[9] = fx fy cx cy alpha beta 0 0 0 in the same nine slots, so the 9-column layout, the Schur complement, the Cayley update and
// the LM rules are shared.  The slots a model does not have are frozen whatever the caller's mask says: 6..8 for EUCM, and 5 (at
// 1.0, which the start holds) for UCM; the reduced system gives frozen columns the row of the identity.
#define CKC_MODEL_OPENCV5 0
#define CKC_MODEL_EUCM 1
#define CKC_MODEL_UCM 2
CKC_HOST_FN unsigned ckc_model_mask(int model) { return model == CKC_MODEL_OPENCV5 ? 0u : (model == CKC_MODEL_UCM ? 0x1E0u : 0x1C0u); }
CKC_FN double ckc_nan(void) { return __builtin_nan(""); }

// The projection rule: den > 0 and Pz > -w d; parameters outside the model (alpha outside [0, 1], beta <= 0) are never valid.  An
// observation that is not valid makes the cost NaN, and ckc_lm_decide rejects the step: a candidate is rejected, never clamped.
CKC_FN int ckc_eucm_valid(const double *k, double den, double d, double Pz) {
    const double alpha = k[4], beta = k[5];
    const double w = alpha > 0.5 ? (1.0 - alpha) / alpha : alpha / (1.0 - alpha);
    return (alpha >= 0.0) & (alpha <= 1.0) & (beta > 0.0) & (den > 0.0) & (Pz > -w * d);
}

CKC_FN void ckc_residual_eucm(const double *k, const double *P, double X, double Y, double u, double v, double *r) {
    const double Px = P[0] * X + P[1] * Y + P[9], Py = P[3] * X + P[4] * Y + P[10], Pz = P[6] * X + P[7] * Y + P[11];
    const double d = sqrt(k[5] * (Px * Px + Py * Py) + Pz * Pz);
    const double den = k[4] * d + (1.0 - k[4]) * Pz;
    const int valid = ckc_eucm_valid(k, den, d, Pz); // (selects, not branches: nothing here may end up in scratch memory)
    r[0] = valid ? k[0] * (Px / den) + k[2] - u : ckc_nan();
    r[1] = valid ? k[1] * (Py / den) + k[3] - v : ckc_nan();
}

// columns fx fy cx cy alpha beta (slots 6..8 zero), then the six pose columns, analytically.  An invalid observation: r NaN; its J is
// what the formulas give and never used (the solver differentiates at accepted parameters only, where the cost is finite)
CKC_FN void ckc_jacobian_eucm(const double *k, const double *P, double X, double Y, double u, double v, unsigned fixed_mask, double *r,
                              double *Ju, double *Jv) {
    const double Px = P[0] * X + P[1] * Y + P[9], Py = P[3] * X + P[4] * Y + P[10], Pz = P[6] * X + P[7] * Y + P[11];
    const double rho2 = Px * Px + Py * Py;
    const double d = sqrt(k[5] * rho2 + Pz * Pz);
    const double den = k[4] * d + (1.0 - k[4]) * Pz;
    const int valid = ckc_eucm_valid(k, den, d, Pz);
    const double xn = Px / den, yn = Py / den, id = 1.0 / den;
    r[0] = valid ? k[0] * xn + k[2] - u : ckc_nan();
    r[1] = valid ? k[1] * yn + k[3] - v : ckc_nan();
    // d(den) / d(alpha, beta), d(xn, yn) / d(den) = -(xn, yn) / den
    const double da = d - Pz, db = (k[4] * rho2) / (2.0 * d);
    const double xq = xn * id, yq = yn * id;
    Ju[0] = xn; Ju[1] = 0.0; Ju[2] = 1.0; Ju[3] = 0.0;
    Ju[4] = -(k[0] * (xq * da)); Ju[5] = -(k[0] * (xq * db)); Ju[6] = 0.0; Ju[7] = 0.0; Ju[8] = 0.0;
    Jv[0] = 0.0; Jv[1] = yn; Jv[2] = 0.0; Jv[3] = 1.0;
    Jv[4] = -(k[1] * (yq * da)); Jv[5] = -(k[1] * (yq * db)); Jv[6] = 0.0; Jv[7] = 0.0; Jv[8] = 0.0;
    CKC_UNROLL
    for (int i = 0; i < CKC_NK; i++)
        if ((fixed_mask >> i) & 1u) { Ju[i] = 0.0; Jv[i] = 0.0; }
    // d(den) / d(camera point), then d(u, v) / d(camera point)
    const double ab = k[4] * k[5];
    const double dx = (ab * Px) / d, dy = (ab * Py) / d, dz = (k[4] * Pz) / d + (1.0 - k[4]);
    double du[3], dv[3];
    du[0] = k[0] * (id - xq * dx); du[1] = -(k[0] * (xq * dy)); du[2] = -(k[0] * (xq * dz));
    dv[0] = -(k[1] * (yq * dx)); dv[1] = k[1] * (id - yq * dy); dv[2] = -(k[1] * (yq * dz));
    ckc_pose_columns(P, X, Y, du, dv, Ju, Jv);
}

// the two by model: a constant where the kernel calls them (its template argument), a variable in the host twin
CKC_FN void ckc_residual_of(const int model, const double *k, const double *P, double X, double Y, double u, double v, double *r) {
    if (model == CKC_MODEL_OPENCV5) ckc_residual(k, P, X, Y, u, v, r);
    else ckc_residual_eucm(k, P, X, Y, u, v, r);
}
CKC_FN void ckc_jacobian_of(const int model, const double *k, const double *P, double X, double Y, double u, double v, unsigned fixed_mask,
                            double *r, double *Ju, double *Jv) {
    if (model == CKC_MODEL_OPENCV5) ckc_jacobian(k, P, X, Y, u, v, fixed_mask, r, Ju, Jv);
    else ckc_jacobian_eucm(k, P, X, Y, u, v, fixed_mask, r, Ju, Jv);
}

// acc += one observation's share of the normal equations.  SUMMATION ORDER (part of the contract): lane l of a wave of 64 adds the
// observations l, l + 64, ... of its frame in index order into its own acc, starting from zero; the 64 partial sums are combined
// by the xor butterfly 32, 16, 8, 4, 2, 1 (a + b is commutative, so every lane ends with lane 0's value); frames are added into
// the problem's sums in frame order.
// The rows a0 .. a1 - 1 of the triangle (tri = their entries, from row a0's diagonal on) and, when g is not null, J^T r: the kernel
// forms the sums in two passes over the observations so that a lane's partial sums stay in registers; each entry is the same sum.
CKC_FN void ckc_accumulate_rows(double *tri, double *g, const double *r, const double *Ju, const double *Jv, const int a0, const int a1) {
    int n = 0;
    CKC_UNROLL
    for (int a = a0; a < a1; a++) {
        CKC_UNROLL
        for (int b = a; b < CKC_NJ; b++) {
            tri[n] = tri[n] + (Ju[a] * Ju[b] + Jv[a] * Jv[b]);
            n++;
        }
    }
    if (g) {
        CKC_UNROLL
        for (int a = 0; a < CKC_NJ; a++) g[a] = g[a] + (Ju[a] * r[0] + Jv[a] * r[1]);
    }
}
CKC_FN void ckc_accumulate(double *acc, const double *r, const double *Ju, const double *Jv) {
    ckc_accumulate_rows(acc, acc + CKC_NH, r, Ju, Jv, 0, CKC_NJ);
}

// Marquardt scaling: the diagonal of J^T J, floored
CKC_FN double ckc_scale(double d) { return d < 1e-30 ? 1e-30 : d; }

// Three dense helpers, one text in two forms: ckc_chol / ckc_fwd / ckc_bwd for an n that is a constant where they are called (6, 9:
// every loop unrolled, the matrices in registers) and ckc_chol_n / ckc_fwd_n / ckc_bwd_n for an n known only at run time (plain loops:
// there is nothing to unroll, and asking for it only earns a warning).  The operations and their order are the same.
//   chol  in-place Cholesky of the lower triangle of the n x n row-major M; 0 when a pivot is not positive (the factor is garbage then)
//   fwd   y = L^-1 b, products subtracted in increasing c; b and the result have stride `st`
//   bwd   x = L^-T y, products subtracted in increasing c
#define CKC_DENSE(SUFFIX, LOOP)                                                      \
    CKC_FN int ckc_chol##SUFFIX(double *M, const int n) {                            \
        int ok = 1;                                                                  \
        LOOP for (int j = 0; j < n; j++) {                                           \
            double s = M[j * n + j];                                                 \
            LOOP for (int c = 0; c < j; c++) s = s - M[j * n + c] * M[j * n + c];    \
            if (!(s > 0.0)) ok = 0;                                                  \
            const double d = sqrt(s);                                                \
            M[j * n + j] = d;                                                        \
            LOOP for (int i = j + 1; i < n; i++) {                                   \
                double t = M[i * n + j];                                             \
                LOOP for (int c = 0; c < j; c++) t = t - M[i * n + c] * M[j * n + c]; \
                M[i * n + j] = t / d;                                                \
            }                                                                        \
        }                                                                            \
        return ok;                                                                   \
    }                                                                                \
    CKC_FN void ckc_fwd##SUFFIX(const double *L, const int n, double *b, const int st) { \
        LOOP for (int i = 0; i < n; i++) {                                           \
            double t = b[i * st];                                                    \
            LOOP for (int c = 0; c < i; c++) t = t - L[i * n + c] * b[c * st];       \
            b[i * st] = t / L[i * n + i];                                            \
        }                                                                            \
    }                                                                                \
    CKC_FN void ckc_bwd##SUFFIX(const double *L, const int n, double *b) {           \
        LOOP for (int ii = 0; ii < n; ii++) {                                        \
            const int i = n - 1 - ii;                                                \
            double t = b[i];                                                         \
            LOOP for (int c = i + 1; c < n; c++) t = t - L[c * n + i] * b[c];        \
            b[i] = t / L[i * n + i];                                                 \
        }                                                                            \
    }
CKC_DENSE(, CKC_UNROLL)
CKC_DENSE(_n, )

// One frame's part of the Schur complement at damping lambda: factor A_f + lambda D_f, W = L^-1 B_f^T, wg = L^-1 g_f,
// E = (W^T W, W^T wg).  `f` is the frame's record; 0 when the factorisation fails.
CKC_FN int ckc_frame_schur(double *f, double lambda) {
    double L[36], W[54], wg[6];
    CKC_UNROLL
    for (int i = 0; i < 6; i++) {
        CKC_UNROLL
        for (int j = 0; j < 6; j++) L[i * 6 + j] = 0.0;
    }
    CKC_UNROLL
    for (int i = 0; i < 6; i++) {
        CKC_UNROLL
        for (int j = 0; j <= i; j++) L[i * 6 + j] = f[CKC_WS_H + CKC_TRI(9 + j, 9 + i)];
        L[i * 6 + i] = L[i * 6 + i] + lambda * ckc_scale(L[i * 6 + i]);
        wg[i] = f[CKC_WS_H + CKC_NH + 9 + i];
        CKC_UNROLL
        for (int a = 0; a < 9; a++) W[i * 9 + a] = f[CKC_WS_H + CKC_TRI(a, 9 + i)];
    }
    const int ok = ckc_chol(L, 6);
    ckc_fwd(L, 6, wg, 1);
    CKC_UNROLL
    for (int a = 0; a < 9; a++) ckc_fwd(L, 6, W + a, 9);
    CKC_UNROLL
    for (int i = 0; i < 36; i++) f[CKC_WS_L + i] = L[i];
    CKC_UNROLL
    for (int i = 0; i < 54; i++) f[CKC_WS_W + i] = W[i];
    CKC_UNROLL
    for (int i = 0; i < 6; i++) f[CKC_WS_WG + i] = wg[i];
    int n = 0;
    CKC_UNROLL
    for (int a = 0; a < 9; a++) {
        CKC_UNROLL
        for (int b = a; b < 9; b++) {
            double s = 0.0;
            CKC_UNROLL
            for (int i = 0; i < 6; i++) s = s + W[i * 9 + a] * W[i * 9 + b];
            f[CKC_WS_E + n] = s;
            n++;
        }
    }
    CKC_UNROLL
    for (int a = 0; a < 9; a++) {
        double s = 0.0;
        CKC_UNROLL
        for (int i = 0; i < 6; i++) s = s + W[i * 9 + a] * wg[i];
        f[CKC_WS_E + 45 + a] = s;
    }
    return ok;
}

// The reduced system: S = C + lambda D_k - sum E, rhs = -g_k + sum W^T wg; frozen intrinsics get the row of the identity.
// Hs = the problem's summed normal equations (135), Es = the summed E (54), S = 81 doubles of work space.  dk = the intrinsics'
// step, *pred = its share of the predicted decrease.  0 when the factorisation fails.
CKC_FN int ckc_reduced_solve(const double *Hs, const double *Es, double lambda, unsigned fixed_mask, double *S, double *dk, double *pred) {
    int n = 0;
    for (int a = 0; a < 9; a++)
        for (int b = a; b < 9; b++) {
            double s = Hs[CKC_TRI(a, b)];
            if (a == b) s = s + lambda * ckc_scale(s);
            s = s - Es[n];
            n++;
            if (((fixed_mask >> a) & 1u) || ((fixed_mask >> b) & 1u)) s = a == b ? 1.0 : 0.0;
            S[b * 9 + a] = s;
        }
    for (int a = 0; a < 9; a++) dk[a] = ((fixed_mask >> a) & 1u) ? 0.0 : Es[45 + a] - Hs[CKC_NH + a];
    const int ok = ckc_chol(S, 9);
    ckc_fwd(S, 9, dk, 1);
    ckc_bwd(S, 9, dk);
    double p = 0.0;
    for (int a = 0; a < 9; a++) {
        if ((fixed_mask >> a) & 1u) dk[a] = 0.0;
        p = p + dk[a] * ((lambda * ckc_scale(Hs[CKC_TRI(a, a)])) * dk[a] - Hs[CKC_NH + a]);
    }
    *pred = p;
    return ok;
}

// The Cayley map C(d) = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a), a = d / 2: a rotation for every d, the identity at d = 0
CKC_FN void ckc_cayley(const double *d, double *Cm) {
    const double a0 = 0.5 * d[0], a1 = 0.5 * d[1], a2 = 0.5 * d[2];
    const double nn = a0 * a0 + a1 * a1 + a2 * a2, den = 1.0 + nn, e = 1.0 - nn;
    Cm[0] = (e + (2.0 * a0) * a0) / den; Cm[1] = ((2.0 * a0) * a1 - 2.0 * a2) / den; Cm[2] = ((2.0 * a0) * a2 + 2.0 * a1) / den;
    Cm[3] = ((2.0 * a1) * a0 + 2.0 * a2) / den; Cm[4] = (e + (2.0 * a1) * a1) / den; Cm[5] = ((2.0 * a1) * a2 - 2.0 * a0) / den;
    Cm[6] = ((2.0 * a2) * a0 - 2.0 * a1) / den; Cm[7] = ((2.0 * a2) * a1 + 2.0 * a0) / den; Cm[8] = (e + (2.0 * a2) * a2) / den;
}
// The update of a rigid transform P = (R row-major, t) by the increment d = (d_w, d_t): Pc = (R C(d_w), t + d_t).  mask6 freezes
// increments: a rotation whose three increments (bits 0..2) are all frozen and a frozen component of t (bits 3..5) are copied, so
// they come back bit for bit.
CKC_FN void ckc_rigid_step(const double *P, const double *d, unsigned mask6, double *Pc) {
    double Cm[9];
    ckc_cayley(d, Cm);
    CKC_UNROLL
    for (int i = 0; i < 3; i++) {
        const double r0 = P[3 * i], r1 = P[3 * i + 1], r2 = P[3 * i + 2];
        CKC_UNROLL
        for (int j = 0; j < 3; j++) Pc[3 * i + j] = (mask6 & 7u) == 7u ? P[3 * i + j] : (r0 * Cm[j] + r1 * Cm[3 + j]) + r2 * Cm[6 + j];
        Pc[9 + i] = ((mask6 >> (3 + i)) & 1u) ? P[9 + i] : P[9 + i] + d[3 + i];
    }
}

// One frame's step given the intrinsics' step: d_f = -L^-T (wg + W dk); the candidate pose (ckc_rigid_step); the frame's share of
// the predicted decrease.
CKC_FN void ckc_frame_step(double *f, const double *dk, double lambda) {
    double d[6];
    CKC_UNROLL
    for (int i = 0; i < 6; i++) {
        double s = f[CKC_WS_WG + i];
        CKC_UNROLL
        for (int a = 0; a < 9; a++) s = s + f[CKC_WS_W + i * 9 + a] * dk[a];
        d[i] = -s;
    }
    double L[36];
    CKC_UNROLL
    for (int i = 0; i < 36; i++) L[i] = f[CKC_WS_L + i];
    ckc_bwd(L, 6, d);
    double p = 0.0;
    CKC_UNROLL
    for (int i = 0; i < 6; i++)
        p = p + d[i] * ((lambda * ckc_scale(f[CKC_WS_H + CKC_TRI(9 + i, 9 + i)])) * d[i] - f[CKC_WS_H + CKC_NH + 9 + i]);
    f[CKC_WS_PRED] = p;
    ckc_rigid_step(f + CKC_WS_POSE, d, 0u, f + CKC_WS_CAND);
}

// Nielsen's damping and the stop rules.  `cost_floor` is the cost below which a solve is done, in the units of the caller's cost: 1e-20
// px^2 here (CKC_COST_FLOOR), CKR_COST_FLOOR for the two solvers of ck_cal_math.h.  The scalar state of one solve:
typedef struct ckc_lm {
    double lambda, nu, cost;
    int iters, status, need_jac; // status -1 while running
} ckc_lm_t;
#define CKC_COST_FLOOR 1e-20
CKC_FN void ckc_lm_start(ckc_lm_t *s, double cost0, double cost_floor) {
    s->lambda = 1e-3; s->nu = 2.0; s->cost = cost0;
    s->iters = 0; s->need_jac = 1;
    s->status = cost0 < cost_floor ? 0 : -1;
}
// One outer iteration ends: solved = the factorisations went through, pred / cost_new as computed.  1: the candidate is accepted.
CKC_FN int ckc_lm_decide(ckc_lm_t *s, int solved, double pred, double cost_new, int max_iters, double cost_floor) {
    int accept = 0;
    double rho = 0.0;
    s->iters = s->iters + 1;
    if (solved && pred > 0.0 && ckc_finite(cost_new)) {
        rho = (s->cost - cost_new) / pred;
        accept = rho > 0.0;
    }
    if (accept) {
        const double dec = s->cost - cost_new, t = 2.0 * rho - 1.0, m = 1.0 - (t * t) * t;
        const int done = dec <= 1e-14 * s->cost || cost_new < cost_floor;
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
