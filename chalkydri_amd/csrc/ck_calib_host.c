// Camera calibration, the half that needs no device: the checks every entry point shares, the start of a problem
// (homographies, focal lengths, poses) and ck_calib_refine_host, the one-thread twin of k_calib.hip.  The arithmetic of the refinement
// is ck_calib_math.h's, compiled into both; this file walks the observations the way the kernel's lanes do (ckc_accumulate), so
// that the two return the same bytes.
#include "chalkydri_hip.h"
#include "ck_calib_math.h"
#include <stdlib.h>
#include <string.h>

void ck_calib_params_default(ck_calib_params_t *p, int32_t width, int32_t height) {
    if (!p) return;
    p->width = width; p->height = height;
    p->fixed_mask = 0; p->max_iters = 100;
    p->min_points_per_frame = 24; p->min_frames = 3;
}

int ck_calib_check(const ck_calib_params_t *p, const ck_calib_problem_t *problems, int32_t n_problems, const double *board_xy,
                   const double *image_uv, const int32_t *frame_start, int32_t n_points_total, int32_t n_starts_total,
                   int32_t n_frames_total) {
    if (!p || !problems || !board_xy || !image_uv || !frame_start) return CK_EINVAL;
    if (n_problems < 0 || n_points_total < 0 || n_starts_total < 0 || n_frames_total < 0) return CK_EINVAL;
    if (p->width < 16 || p->height < 16 || p->max_iters < 1 || p->max_iters > 10000) return CK_EINVAL;
    if (p->min_points_per_frame < 4 || p->min_frames < 1) return CK_EINVAL;
    for (int32_t i = 0; i < n_problems; i++) {
        const ck_calib_problem_t *q = problems + i;
        if (q->n_frames < p->min_frames) return CK_EINVAL;
        if (q->n_frames > CK_CALIB_MAX_FRAMES) return CK_ECAPACITY;
        if (q->start_offset < 0 || q->point_offset < 0 || q->pose_offset < 0) return CK_EINVAL;
        if ((int64_t)q->start_offset + q->n_frames + 1 > n_starts_total || (int64_t)q->pose_offset + q->n_frames > n_frames_total) return CK_EINVAL;
        const int32_t *fs = frame_start + q->start_offset;
        if (fs[0] < 0 || (int64_t)q->point_offset + fs[q->n_frames] > n_points_total) return CK_EINVAL;
        for (int32_t f = 0; f < q->n_frames; f++) {
            if (fs[f + 1] < fs[f]) return CK_EINVAL;
            const int32_t n = fs[f + 1] - fs[f];
            if (n > CK_CALIB_MAX_POINTS) return CK_ECAPACITY;
            if (n < p->min_points_per_frame) return CK_EINVAL;
        }
        if ((int64_t)q->point_offset + fs[q->n_frames] > n_points_total) return CK_EINVAL;
        for (int64_t j = 2 * ((int64_t)q->point_offset + fs[0]); j < 2 * ((int64_t)q->point_offset + fs[q->n_frames]); j++)
            if (!ckc_finite(board_xy[j]) || !ckc_finite(image_uv[j])) return CK_EINVAL;
    }
    return CK_OK;
}

// ---- the start ---------------------------------------------------------------------------------------------------------------
// a = A^-1 b by Gaussian elimination with partial pivoting, in place; 0 when a pivot vanishes against the matrix' largest entry
static int gauss(double *A, double *b, int n) {
    double big = 0.0;
    for (int i = 0; i < n * n; i++) big = fabs(A[i]) > big ? fabs(A[i]) : big;
    if (!(big > 0.0) || !ckc_finite(big)) return 0;
    for (int c = 0; c < n; c++) {
        int piv = c;
        for (int r = c + 1; r < n; r++)
            if (fabs(A[r * n + c]) > fabs(A[piv * n + c])) piv = r;
        if (!(fabs(A[piv * n + c]) > 1e-13 * big)) return 0;
        if (piv != c) {
            for (int j = 0; j < n; j++) { const double t = A[c * n + j]; A[c * n + j] = A[piv * n + j]; A[piv * n + j] = t; }
            const double t = b[c]; b[c] = b[piv]; b[piv] = t;
        }
        for (int r = c + 1; r < n; r++) {
            const double m = A[r * n + c] / A[c * n + c];
            for (int j = c; j < n; j++) A[r * n + j] -= m * A[c * n + j];
            b[r] -= m * b[c];
        }
    }
    for (int r = n - 1; r >= 0; r--) {
        double t = b[r];
        for (int j = r + 1; j < n; j++) t -= A[r * n + j] * b[j];
        b[r] = t / A[r * n + r];
    }
    return 1;
}

// Hartley's normalisation of n points: x' = s (x - mx), y' = s (y - my) with mean distance sqrt(2) from the origin
static int hartley(const double *xy, int n, double *mx, double *my, double *s) {
    double sx = 0.0, sy = 0.0, sd = 0.0;
    for (int i = 0; i < n; i++) { sx += xy[2 * i]; sy += xy[2 * i + 1]; }
    *mx = sx / n; *my = sy / n;
    for (int i = 0; i < n; i++) sd += sqrt((xy[2 * i] - *mx) * (xy[2 * i] - *mx) + (xy[2 * i + 1] - *my) * (xy[2 * i + 1] - *my));
    if (!(sd > 0.0)) return 0;
    *s = sqrt(2.0) * n / sd;
    return ckc_finite(*s);
}

// board -> image homography of one frame, H[8] = 1 in the normalised frames, then taken back to metres and pixels
static int homography(const double *bxy, const double *uv, int n, double *H) {
    double bx, by, bs, ux, uy, us, A[64], b[8];
    if (!hartley(bxy, n, &bx, &by, &bs) || !hartley(uv, n, &ux, &uy, &us)) return 0;
    memset(A, 0, sizeof A);
    memset(b, 0, sizeof b);
    for (int i = 0; i < n; i++) {
        const double x = bs * (bxy[2 * i] - bx), y = bs * (bxy[2 * i + 1] - by), u = us * (uv[2 * i] - ux), v = us * (uv[2 * i + 1] - uy);
        const double r1[8] = {x, y, 1.0, 0.0, 0.0, 0.0, -u * x, -u * y}, r2[8] = {0.0, 0.0, 0.0, x, y, 1.0, -v * x, -v * y};
        for (int a = 0; a < 8; a++) {
            for (int c = 0; c < 8; c++) A[a * 8 + c] += r1[a] * r1[c] + r2[a] * r2[c];
            b[a] += r1[a] * u + r2[a] * v;
        }
    }
    if (!gauss(A, b, 8)) return 0;
    // H = Tu^-1 Hn Tb with Tb = [bs 0 -bs bx; 0 bs -bs by; 0 0 1], Tu^-1 = [1/us 0 ux; 0 1/us uy; 0 0 1]
    const double Hn[9] = {b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], 1.0};
    double M[9];
    for (int r = 0; r < 3; r++) {
        M[3 * r] = Hn[3 * r] * bs; M[3 * r + 1] = Hn[3 * r + 1] * bs;
        M[3 * r + 2] = Hn[3 * r + 2] - bs * (Hn[3 * r] * bx + Hn[3 * r + 1] * by);
    }
    for (int c = 0; c < 3; c++) {
        H[c] = M[c] / us + ux * M[6 + c];
        H[3 + c] = M[3 + c] / us + uy * M[6 + c];
        H[6 + c] = M[6 + c];
    }
    for (int i = 0; i < 9; i++)
        if (!ckc_finite(H[i])) return 0;
    return 1;
}

// The start of one checked problem: k4 = fx fy cx cy and the poses (zero when there is none: *status_out DEGENERATE).  given_f <= 0:
// the focal lengths come from the homographies (ck_calib_init's start); given_f > 0: fx = fy = given_f, the homographies give the poses.
static int start_of(const ck_calib_params_t *p, const ck_calib_problem_t *q, const double *board_xy, const double *image_uv,
                    const int32_t *frame_start, double given_f, double *k4, double *poses0, int32_t *status_out) {
    const int F = q->n_frames;
    const int32_t *fs = frame_start + q->start_offset;
    double *poses = poses0 + 12 * (size_t)q->pose_offset;
    memset(k4, 0, sizeof(double) * 4);
    memset(poses, 0, sizeof(double) * 12 * (size_t)F);
    *status_out = CK_CALIB_DEGENERATE;
    double *H = (double *)malloc(sizeof(double) * 9 * (size_t)F);
    if (!H) return CK_ENOMEM;
    const double cx = 0.5 * (p->width - 1), cy = 0.5 * (p->height - 1);
    double N[4] = {0, 0, 0, 0}, nb[2] = {0, 0};
    int ok = 1;
    for (int f = 0; f < F && ok; f++) {
        double *Hf = H + 9 * f;
        const size_t o = (size_t)q->point_offset + (size_t)fs[f];
        ok = homography(board_xy + 2 * o, image_uv + 2 * o, fs[f + 1] - fs[f], Hf);
        if (!ok) break;
        for (int c = 0; c < 3; c++) { Hf[c] -= cx * Hf[6 + c]; Hf[3 + c] -= cy * Hf[6 + c]; } // the principal point becomes the origin
        const double e[2][3] = {{Hf[0] * Hf[1], Hf[3] * Hf[4], Hf[6] * Hf[7]},
                                {Hf[0] * Hf[0] - Hf[1] * Hf[1], Hf[3] * Hf[3] - Hf[4] * Hf[4], Hf[6] * Hf[6] - Hf[7] * Hf[7]}};
        for (int k = 0; k < 2; k++) {
            N[0] += e[k][0] * e[k][0]; N[1] += e[k][0] * e[k][1]; N[3] += e[k][1] * e[k][1];
            nb[0] -= e[k][0] * e[k][2]; nb[1] -= e[k][1] * e[k][2];
        }
    }
    N[2] = N[1];
    double fx = 0.0, fy = 0.0;
    // Singular in the sense that matters: frames that are all (nearly) parallel to the image plane make every equation a multiple
    // of (1, -1, 0), and nothing separates the focal length from the distance.  sin^2 of the angle between the system's two columns
    // is at most 1.7e-5 for such captures of the reference's cameras and at least 1.2e-3 for captures tilted as DESIGN.md §4j says
    if (ok) ok = N[0] * N[3] - N[1] * N[1] > 1e-4 * (N[0] * N[3]); // (the capture's geometry: it holds for a given focal length too)
    if (given_f > 0.0) {
        fx = given_f; fy = given_f;
    } else {
        if (ok) ok = gauss(N, nb, 2);
        if (ok) ok = nb[0] > 0.0 && nb[1] > 0.0 && ckc_finite(nb[0]) && ckc_finite(nb[1]);
        if (ok) {
            fx = 1.0 / sqrt(nb[0]); fy = 1.0 / sqrt(nb[1]);
            ok = ckc_finite(fx) && ckc_finite(fy);
        }
    }
    for (int f = 0; f < F && ok; f++) {
        const double *Hf = H + 9 * f;
        double m[3][3]; // columns of K^-1 H
        for (int c = 0; c < 3; c++) { m[c][0] = Hf[c] / fx; m[c][1] = Hf[3 + c] / fy; m[c][2] = Hf[6 + c]; }
        const double n1 = sqrt(m[0][0] * m[0][0] + m[0][1] * m[0][1] + m[0][2] * m[0][2]);
        const double n2 = sqrt(m[1][0] * m[1][0] + m[1][1] * m[1][1] + m[1][2] * m[1][2]);
        double lam = 2.0 / (n1 + n2);
        if (lam * m[2][2] < 0.0) lam = -lam;
        double r1[3], r2[3], r3[3], d = 0.0, nn;
        for (int i = 0; i < 3; i++) r1[i] = lam * m[0][i];
        nn = sqrt(r1[0] * r1[0] + r1[1] * r1[1] + r1[2] * r1[2]);
        for (int i = 0; i < 3; i++) r1[i] /= nn;
        for (int i = 0; i < 3; i++) { r2[i] = lam * m[1][i]; d += r1[i] * r2[i]; }
        for (int i = 0; i < 3; i++) r2[i] -= d * r1[i];
        nn = sqrt(r2[0] * r2[0] + r2[1] * r2[1] + r2[2] * r2[2]);
        for (int i = 0; i < 3; i++) r2[i] /= nn;
        r3[0] = r1[1] * r2[2] - r1[2] * r2[1]; r3[1] = r1[2] * r2[0] - r1[0] * r2[2]; r3[2] = r1[0] * r2[1] - r1[1] * r2[0];
        double *P = poses + 12 * f;
        for (int i = 0; i < 3; i++) { P[3 * i] = r1[i]; P[3 * i + 1] = r2[i]; P[3 * i + 2] = r3[i]; P[9 + i] = lam * m[2][i]; }
        for (int i = 0; i < 12; i++) ok = ok && ckc_finite(P[i]);
        ok = ok && P[11] > 0.0;
    }
    free(H);
    if (!ok) {
        memset(poses, 0, sizeof(double) * 12 * (size_t)F);
        return CK_OK;
    }
    k4[0] = fx; k4[1] = fy; k4[2] = cx; k4[3] = cy;
    *status_out = CK_CALIB_CONVERGED;
    return CK_OK;
}

int ck_calib_init(const ck_calib_params_t *p, const ck_calib_problem_t *q, const double *board_xy, const double *image_uv,
                  const int32_t *frame_start, int32_t n_points_total, int32_t n_starts_total, int32_t n_frames_total,
                  ck_opencv5_t *cam0_out, double *poses0, int32_t *status_out) {
    if (!cam0_out || !poses0 || !status_out) return CK_EINVAL;
    const int rc = ck_calib_check(p, q, 1, board_xy, image_uv, frame_start, n_points_total, n_starts_total, n_frames_total);
    if (rc != CK_OK) return rc;
    memset(cam0_out, 0, sizeof *cam0_out);
    return start_of(p, q, board_xy, image_uv, frame_start, 0.0, (double *)cam0_out, poses0, status_out);
}

static int model_ok(int32_t model) { return model == CK_CAMERA_OPENCV5 || model == CK_CAMERA_EUCM || model == CK_CAMERA_UCM; }

// Start `start_index` of a problem.  OPENCV5 has one: ck_calib_init's.  EUCM / UCM have CK_CAMCAL_STARTS: 0 =
// ck_calib_init's focal lengths, 1..5 = fx = fy = {0.3, 0.45, 0.65, 1.0, 1.5} max(width, height); each with the principal point at
// the image centre, alpha = 0.5, beta = 1 and the poses from the frames' homographies and that K.
int ck_camera_calib_init(int32_t model, const ck_calib_params_t *p, const ck_calib_problem_t *q, const double *board_xy,
                         const double *image_uv, const int32_t *frame_start, int32_t n_points_total, int32_t n_starts_total,
                         int32_t n_frames_total, int32_t start_index, ck_camera_t *cam0_out, double *poses0, int32_t *status_out) {
    static const double ladder[CK_CAMCAL_STARTS] = {0.0, 0.3, 0.45, 0.65, 1.0, 1.5};
    if (!cam0_out || !poses0 || !status_out) return CK_EINVAL;
    if (!model_ok(model) || start_index < 0 || start_index >= (model == CK_CAMERA_OPENCV5 ? 1 : CK_CAMCAL_STARTS)) return CK_EINVAL;
    const int rc = ck_calib_check(p, q, 1, board_xy, image_uv, frame_start, n_points_total, n_starts_total, n_frames_total);
    if (rc != CK_OK) return rc;
    memset(cam0_out, 0, sizeof *cam0_out);
    cam0_out->model = model;
    const double f = ladder[start_index] * (double)(p->width > p->height ? p->width : p->height);
    const int rs = start_of(p, q, board_xy, image_uv, frame_start, f, cam0_out->k, poses0, status_out);
    if (rs == CK_OK && *status_out == CK_CALIB_CONVERGED && model != CK_CAMERA_OPENCV5) { cam0_out->k[4] = 0.5; cam0_out->k[5] = 1.0; }
    return rs;
}

// ---- the refinement ----------------------------------------------------------------------------------------------------------
int ck_calib_start_ok(const double *cam0, const double *poses, int n_frames); // (ck_calib.h: the device half asks here too)
int ck_calib_start_ok(const double *cam0, const double *poses, int n_frames) {
    for (int i = 0; i < 9; i++)
        if (!ckc_finite(cam0[i])) return 0;
    if (!(cam0[0] > 0.0) || !(cam0[1] > 0.0)) return 0;
    for (int i = 0; i < 12 * n_frames; i++)
        if (!ckc_finite(poses[i])) return 0;
    return 1;
}

int ck_calib_jacobian(const ck_opencv5_t *cam, const double *pose, const double *board_xy, const double *image_uv, int32_t n,
                      uint32_t fixed_mask, double *r_out, double *J_out) {
    if (!cam || !pose || !board_xy || !image_uv || !r_out || !J_out || n < 0) return CK_EINVAL;
    for (int32_t i = 0; i < n; i++)
        ckc_jacobian((const double *)cam, pose, board_xy[2 * i], board_xy[2 * i + 1], image_uv[2 * i], image_uv[2 * i + 1], fixed_mask,
                     r_out + 2 * i, J_out + 2 * CKC_NJ * (size_t)i, J_out + 2 * CKC_NJ * (size_t)i + CKC_NJ);
    return CK_OK;
}

int ck_camera_calib_jacobian(int32_t model, const ck_camera_t *cam, const double *pose, const double *board_xy, const double *image_uv,
                             int32_t n, uint32_t fixed_mask, double *r_out, double *J_out) {
    if (!cam || !pose || !board_xy || !image_uv || !r_out || !J_out || n < 0 || !model_ok(model)) return CK_EINVAL;
    double k[9];
    memcpy(k, cam->k, sizeof k);
    if (model == CK_CAMERA_UCM) k[5] = 1.0;
    for (int32_t i = 0; i < n; i++)
        ckc_jacobian_of(model, k, pose, board_xy[2 * i], board_xy[2 * i + 1], image_uv[2 * i], image_uv[2 * i + 1],
                        fixed_mask | ckc_model_mask(model), r_out + 2 * i, J_out + 2 * CKC_NJ * (size_t)i, J_out + 2 * CKC_NJ * (size_t)i + CKC_NJ);
    return CK_OK;
}

// the xor butterfly 32, 16, ..., 1 of 64 lanes' partial sums, as lane 0 sees it
static void butterfly(double (*part)[CKC_NACC], int n) {
    for (int m = 32; m >= 1; m >>= 1)
        for (int l = 0; l < m; l++)
            for (int j = 0; j < n; j++) part[l][j] = part[l][j] + part[l + m][j];
}

typedef struct {
    const double *bxy, *uv;
    const int32_t *fs;
    int F, model;
    double *ws;
    double (*part)[CKC_NACC];
} twin_t;

// the candidate's cost: per frame by lanes and butterfly into the frame's record, then the frames in order
static double twin_cost(const twin_t *T, const double *k) {
    for (int f = 0; f < T->F; f++) {
        double *wf = T->ws + (size_t)CKC_WS_STRIDE * f;
        for (int l = 0; l < 64; l++) {
            double c = 0.0, r[2];
            for (int i = T->fs[f] + l; i < T->fs[f + 1]; i += 64) {
                ckc_residual_of(T->model, k, wf + CKC_WS_CAND, T->bxy[2 * i], T->bxy[2 * i + 1], T->uv[2 * i], T->uv[2 * i + 1], r);
                c = c + (r[0] * r[0] + r[1] * r[1]);
            }
            T->part[l][0] = c;
        }
        butterfly(T->part, 1);
        wf[CKC_WS_COST] = T->part[0][0];
    }
    double c = 0.0;
    for (int f = 0; f < T->F; f++) c = c + T->ws[(size_t)CKC_WS_STRIDE * f + CKC_WS_COST];
    return c;
}

// The refinement of one checked problem of any model; an EUCM / UCM problem keeps its parameters in the nine slots of res->cam
static int refine_host(int model, const ck_calib_params_t *p, const ck_calib_problem_t *q, const double *board_xy, const double *image_uv,
                       const int32_t *frame_start, const ck_opencv5_t *cam0, const double *poses0, ck_calib_result_t *res, double *poses_out) {
    const int F = q->n_frames;
    const unsigned fixed_mask = p->fixed_mask | ckc_model_mask(model);
    twin_t T;
    T.fs = frame_start + q->start_offset; T.F = F; T.model = model;
    T.bxy = board_xy + 2 * (size_t)q->point_offset; T.uv = image_uv + 2 * (size_t)q->point_offset;
    const double *pin = poses0 + 12 * (size_t)q->pose_offset;
    double *pout = poses_out + 12 * (size_t)q->pose_offset;
    memset(res, 0, sizeof *res);
    res->cam = *cam0;
    res->n_frames = F; res->n_points = T.fs[F] - T.fs[0];
    res->status = CK_CALIB_DEGENERATE;
    if (pout != pin) memmove(pout, pin, sizeof(double) * 12 * (size_t)F);
    if (!ck_calib_start_ok((const double *)cam0, pin, F)) return CK_OK;
    T.ws = (double *)calloc((size_t)CKC_WS_STRIDE * (size_t)F, sizeof(double));
    T.part = (double (*)[CKC_NACC])malloc(sizeof(double) * 64 * CKC_NACC);
    if (!T.ws || !T.part) { free(T.ws); free(T.part); return CK_ENOMEM; }
    double k[9], kc[9], Hs[CKC_NACC], Es[54], S[81], dk[9];
    memcpy(k, cam0, sizeof k);
    memcpy(kc, k, sizeof k);
    for (int f = 0; f < F; f++) {
        memcpy(T.ws + (size_t)CKC_WS_STRIDE * f + CKC_WS_POSE, pout + 12 * f, sizeof(double) * 12);
        memcpy(T.ws + (size_t)CKC_WS_STRIDE * f + CKC_WS_CAND, pout + 12 * f, sizeof(double) * 12);
    }
    const double cost0 = twin_cost(&T, kc);
    if (ckc_finite(cost0)) {
        ckc_lm_t lm;
        ckc_lm_start(&lm, cost0, CKC_COST_FLOOR);
        while (lm.status < 0) {
            if (lm.need_jac) {
                for (int f = 0; f < F; f++) {
                    double *wf = T.ws + (size_t)CKC_WS_STRIDE * f;
                    for (int l = 0; l < 64; l++) {
                        double r[2], Ju[CKC_NJ], Jv[CKC_NJ];
                        for (int j = 0; j < CKC_NACC; j++) T.part[l][j] = 0.0;
                        for (int i = T.fs[f] + l; i < T.fs[f + 1]; i += 64) {
                            ckc_jacobian_of(model, k, wf + CKC_WS_POSE, T.bxy[2 * i], T.bxy[2 * i + 1], T.uv[2 * i], T.uv[2 * i + 1], fixed_mask, r, Ju, Jv);
                            ckc_accumulate(T.part[l], r, Ju, Jv);
                        }
                    }
                    butterfly(T.part, CKC_NACC);
                    memcpy(wf + CKC_WS_H, T.part[0], sizeof(double) * CKC_NACC);
                }
                for (int j = 0; j < CKC_NACC; j++) {
                    double s = 0.0;
                    for (int f = 0; f < F; f++) s = s + T.ws[(size_t)CKC_WS_STRIDE * f + CKC_WS_H + j];
                    Hs[j] = s;
                }
            }
            int solved = 1;
            for (int f = 0; f < F; f++)
                if (!ckc_frame_schur(T.ws + (size_t)CKC_WS_STRIDE * f, lm.lambda)) solved = 0;
            for (int j = 0; j < 54; j++) {
                double s = 0.0;
                for (int f = 0; f < F; f++) s = s + T.ws[(size_t)CKC_WS_STRIDE * f + CKC_WS_E + j];
                Es[j] = s;
            }
            double pred = 0.0, cost_new = 0.0;
            if (!ckc_reduced_solve(Hs, Es, lm.lambda, fixed_mask, S, dk, &pred)) solved = 0;
            if (solved) {
                for (int i = 0; i < 9; i++) kc[i] = ((fixed_mask >> i) & 1u) ? k[i] : k[i] + dk[i];
                for (int f = 0; f < F; f++) ckc_frame_step(T.ws + (size_t)CKC_WS_STRIDE * f, dk, lm.lambda);
                for (int f = 0; f < F; f++) pred = pred + T.ws[(size_t)CKC_WS_STRIDE * f + CKC_WS_PRED];
                cost_new = twin_cost(&T, kc);
            }
            if (ckc_lm_decide(&lm, solved, pred, cost_new, p->max_iters, CKC_COST_FLOOR)) {
                memcpy(k, kc, sizeof k);
                for (int f = 0; f < F; f++)
                    memcpy(T.ws + (size_t)CKC_WS_STRIDE * f + CKC_WS_POSE, T.ws + (size_t)CKC_WS_STRIDE * f + CKC_WS_CAND, sizeof(double) * 12);
            }
        }
        memcpy(&res->cam, k, sizeof k);
        for (int f = 0; f < F; f++) memcpy(pout + 12 * f, T.ws + (size_t)CKC_WS_STRIDE * f + CKC_WS_POSE, sizeof(double) * 12);
        res->status = lm.status; res->iters = lm.iters;
        res->cost0 = cost0; res->cost = lm.cost;
        res->rms = sqrt(lm.cost / (double)res->n_points);
    }
    free(T.ws);
    free(T.part);
    return CK_OK;
}

int ck_calib_refine_host(const ck_calib_params_t *p, const ck_calib_problem_t *q, const double *board_xy, const double *image_uv,
                         const int32_t *frame_start, int32_t n_points_total, int32_t n_starts_total, int32_t n_frames_total,
                         const ck_opencv5_t *cam0, const double *poses0, ck_calib_result_t *res, double *poses_out) {
    if (!cam0 || !poses0 || !res || !poses_out) return CK_EINVAL;
    const int rc = ck_calib_check(p, q, 1, board_xy, image_uv, frame_start, n_points_total, n_starts_total, n_frames_total);
    if (rc != CK_OK) return rc;
    return refine_host(CK_CAMERA_OPENCV5, p, q, board_xy, image_uv, frame_start, cam0, poses0, res, poses_out);
}

// ck_calib_result_t (the solver's record, any model in its nine slots) -> ck_camera_calib_result_t; ck_calib.hip converts here too
void ck_calib_result_to_camera(int model, const ck_calib_result_t *r, int start, int n_starts, ck_camera_calib_result_t *o);
void ck_calib_result_to_camera(int model, const ck_calib_result_t *r, int start, int n_starts, ck_camera_calib_result_t *o) {
    memset(o, 0, sizeof *o);
    o->cam.model = model;
    memcpy(o->cam.k, &r->cam, sizeof o->cam.k);
    o->status = r->status; o->iters = r->iters; o->n_frames = r->n_frames; o->n_points = r->n_points;
    o->rms = r->rms; o->cost0 = r->cost0; o->cost = r->cost;
    o->start = start; o->n_starts = n_starts;
}
// the start a caller hands over, in the solver's nine slots: UCM's slot 5 is 1.0 whatever it holds
void ck_calib_start_from_camera(int model, const ck_camera_t *cam, ck_opencv5_t *k0);
void ck_calib_start_from_camera(int model, const ck_camera_t *cam, ck_opencv5_t *k0) {
    memcpy(k0, cam->k, sizeof *k0);
    if (model == CK_CAMERA_UCM) ((double *)k0)[5] = 1.0;
}

int ck_camera_calib_refine_host(int32_t model, const ck_calib_params_t *p, const ck_calib_problem_t *q, const double *board_xy,
                                const double *image_uv, const int32_t *frame_start, int32_t n_points_total, int32_t n_starts_total,
                                int32_t n_frames_total, const ck_camera_t *cam0, const double *poses0, ck_camera_calib_result_t *res,
                                double *poses_out) {
    if (!cam0 || !poses0 || !res || !poses_out || !model_ok(model)) return CK_EINVAL;
    const int rc = ck_calib_check(p, q, 1, board_xy, image_uv, frame_start, n_points_total, n_starts_total, n_frames_total);
    if (rc != CK_OK) return rc;
    ck_opencv5_t k0;
    ck_calib_result_t r;
    ck_calib_start_from_camera(model, cam0, &k0);
    const int rr = refine_host(model, p, q, board_xy, image_uv, frame_start, &k0, poses0, &r, poses_out);
    if (rr == CK_OK) ck_calib_result_to_camera(model, &r, 0, 1, res);
    return rr;
}
