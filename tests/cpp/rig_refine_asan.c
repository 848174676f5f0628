/* The host twin of the rig pose refinement (ck_rig_refine_host) under AddressSanitizer + UBSan, on the CPU: a stand-alone
 * program of the twin's C files over the shapes at which its walkers' loops end differently (0, 1, 4, 16, 17 tags; 8 cameras of one
 * tag; one camera of 64 tags; a camera without tags between two that have some), in both modes, with and without the heading prior and
 * the rejection masks, and the refusals.  Run by tests/test_rig_refine_host.py.  Prints "ok" and returns 0. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "chalkydri_hip.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
#define HALF (0.1651 / 2.0)

static unsigned g_seed = 12345u;
static double noise(void) { g_seed = g_seed * 1664525u + 1013904223u; return ((double)(g_seed >> 8) / 16777216.0 - 0.5) * 1e-3; }

static void mat_to_quat(const double R[9], double q[4]) {
    const double K[4] = {1 + R[0] + R[4] + R[8], 1 + R[0] - R[4] - R[8], 1 - R[0] + R[4] - R[8], 1 - R[0] - R[4] + R[8]};
    int k = 0;
    for (int i = 1; i < 4; i++) if (K[i] > K[k]) k = i;
    const double s = 2 * sqrt(K[k]);
    if (k == 0) { q[0] = s / 4; q[1] = (R[7] - R[5]) / s; q[2] = (R[2] - R[6]) / s; q[3] = (R[3] - R[1]) / s; }
    else if (k == 1) { q[0] = (R[7] - R[5]) / s; q[1] = s / 4; q[2] = (R[1] + R[3]) / s; q[3] = (R[2] + R[6]) / s; }
    else if (k == 2) { q[0] = (R[2] - R[6]) / s; q[1] = (R[1] + R[3]) / s; q[2] = s / 4; q[3] = (R[5] + R[7]) / s; }
    else { q[0] = (R[3] - R[1]) / s; q[1] = (R[2] + R[6]) / s; q[2] = (R[5] + R[7]) / s; q[3] = s / 4; }
}
static void mul(const double *A, const double *B, double *C) {
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

/* one instant: camera c (looking along the robot's x turned by c * 45 degrees, 0.5 m up) sees counts[c] tags, 3 .. 6 m away, facing it */
typedef struct { ck_sqpnp_problem_t rec[CK_RIG_MAX_CAMS]; ck_iso3_t *tags; double *bear; int nt; double gyro; } instant_t;
static int make_instant(int n_cams, const int *counts, instant_t *I) {
    const double yaw = 0.1, px = 2.0, py = 0.3;
    const double Rwr[9] = {cos(yaw), -sin(yaw), 0, sin(yaw), cos(yaw), 0, 0, 0, 1};
    const double front[9] = {0, -1, 0, 0, 0, -1, 1, 0, 0}, tagc[9] = {0, 1, 0, 0, 0, -1, -1, 0, 0};
    int total = 0;
    for (int c = 0; c < n_cams; c++) total += counts[c];
    I->tags = (ck_iso3_t *)calloc((size_t)total + 1, sizeof(ck_iso3_t));
    I->bear = (double *)calloc(12 * (size_t)total + 3, sizeof(double));
    if (!I->tags || !I->bear) return 0;
    I->nt = total; I->gyro = yaw + 0.004;
    int at = 0;
    for (int c = 0; c < n_cams; c++) {
        const double a = -0.785398163 * c, Rz[9] = {cos(a), -sin(a), 0, sin(a), cos(a), 0, 0, 0, 1}, o[3] = {0.1 * c, 0.05 * c, 0.5};
        double A[9], At[9], Rcw[9], Rt[9];
        mul(front, Rz, A);                                      /* robot -> camera */
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) At[3 * i + j] = A[3 * j + i];
        ck_sqpnp_problem_t *p = &I->rec[c];
        memset(p, 0, sizeof *p);
        p->n_tags = counts[c]; p->n_bearings = 4 * counts[c]; p->tag_offset = at; p->bearing_offset = 4 * at;
        mat_to_quat(A, p->robot_to_cam.q);
        for (int i = 0; i < 3; i++) p->robot_to_cam.t[i] = -(A[3 * i] * o[0] + A[3 * i + 1] * o[1] + A[3 * i + 2] * o[2]);
        mul(Rwr, At, Rcw);                                      /* camera -> world (rotation) */
        mul(Rcw, tagc, Rt);                                     /* tag -> world */
        for (int t = 0; t < counts[c]; t++, at++) {
            const double pc[3] = {-1.5 + 0.4 * (t % 8), -0.6 + 0.25 * ((t / 8) % 8), 3.0 + 0.37 * (t % 9)};
            double pr[3];
            for (int i = 0; i < 3; i++) pr[i] = At[3 * i] * pc[0] + At[3 * i + 1] * pc[1] + At[3 * i + 2] * pc[2] + o[i];
            ck_iso3_t *g = &I->tags[at];
            g->t[0] = Rwr[0] * pr[0] + Rwr[1] * pr[1] + px; g->t[1] = Rwr[3] * pr[0] + Rwr[4] * pr[1] + py; g->t[2] = pr[2];
            mat_to_quat(Rt, g->q);
            for (int j = 0; j < 4; j++) {
                const double y = (j == 1 || j == 2) ? HALF : -HALF, z = j >= 2 ? HALF : -HALF;
                double v[3], nn = 0;
                for (int i = 0; i < 3; i++) { v[i] = pc[i] + tagc[3 * i + 1] * y + tagc[3 * i + 2] * z; nn += v[i] * v[i]; }
                for (int i = 0; i < 3; i++) I->bear[3 * (4 * at + j) + i] = v[i] / sqrt(nn) + noise();
            }
        }
    }
    return 1;
}

static int run_shape(int n_cams, const int *counts, int expect_start) {
    instant_t I;
    CHECK(make_instant(n_cams, counts, &I));
    ck_rig_params_t rp;
    ck_rig_params_default(&rp);
    ck_rig_result_t start;
    CHECK(ck_rig_solve_host(&rp, n_cams, I.rec, 1, I.tags, I.nt, I.bear, 4 * I.nt, &I.gyro, &start) == CK_OK);
    CHECK(start.valid == expect_start);
    for (int mode = 0; mode < 2; mode++)
        for (int prior = 0; prior < 2; prior++)
            for (int masked = 0; masked < 2; masked++) {
                ck_rig_refine_params_t fp;
                ck_rig_refine_params_default(&fp);
                fp.mode = mode; fp.gyro_sigma_rad = prior ? 0.01 : 0.0; fp.sigma_rad = 3e-4; fp.max_iters = 30;
                uint64_t rej[CK_RIG_MAX_CAMS] = {0};
                if (masked) for (int c = 0; c < n_cams; c++) if (counts[c] > 1) rej[c] = (uint64_t)1 << (counts[c] > 64 ? 63 : counts[c] - 1);
                ck_rig_refined_t out;
                CHECK(ck_rig_refine_host(&fp, n_cams, I.rec, 1, I.tags, I.nt, I.bear, 4 * I.nt, prior ? &I.gyro : NULL, &start, masked ? rej : NULL, &out) == CK_OK);
                if (!expect_start) { CHECK(out.status == CK_RIG_REFINE_NO_START && out.n_points == 0 && out.cov[0] == 0.0); continue; }
                int used = 0;
                for (int c = 0; c < n_cams; c++) used += 4 * (counts[c] - (masked && counts[c] > 1));
                CHECK(out.n_points == used);
                CHECK(out.status == CK_RIG_REFINE_CONVERGED || out.status == CK_RIG_REFINE_MAXITERS || out.status == CK_RIG_REFINE_DEGENERATE);
                for (int i = 0; i < 36; i++) CHECK(out.cov[i] - out.cov[i] == 0.0);
                /* (the heading prior may buy its agreement with a larger bearing cost) */
                if (out.status != CK_RIG_REFINE_DEGENERATE && !((prior || out.cost <= out.cost0) && out.rms < 2e-3))
                    printf("mode %d prior %d masked %d: status %d iters %d cost0 %g cost %g rms %g\n", mode, prior, masked, out.status, out.iters, out.cost0, out.cost, out.rms);
                if (out.status != CK_RIG_REFINE_DEGENERATE) CHECK((prior || out.cost <= out.cost0) && out.rms < 2e-3);
            }
    free(I.tags); free(I.bear);
    return 0;
}

int main(void) {
    setvbuf(stdout, NULL, _IONBF, 0);
    static const int shapes[][CK_RIG_MAX_CAMS + 1] = {
        {1, 0}, {1, 1}, {1, 4}, {1, 16}, {1, 17}, {8, 1, 1, 1, 1, 1, 1, 1, 1}, {1, 64}, {3, 2, 0, 3}, {2, 65, 2}};
    for (size_t k = 0; k < sizeof shapes / sizeof shapes[0]; k++) {
        int any = 0;
        for (int c = 0; c < shapes[k][0]; c++) any |= shapes[k][1 + c] > 0;
        if (run_shape(shapes[k][0], shapes[k] + 1, any)) { printf("shape %zu\n", k); return 1; }
    }
    /* the refusals leave the output alone */
    instant_t I;
    const int one[1] = {2};
    CHECK(make_instant(1, one, &I));
    ck_rig_result_t start;
    memset(&start, 0, sizeof start);
    ck_rig_refined_t out, keep;
    memset(&out, 0x5A, sizeof out);
    keep = out;
    ck_rig_refine_params_t fp;
    ck_rig_refine_params_default(&fp);
    CHECK(fp.mode == CK_RIG_REFINE_FREE && fp.max_iters == 10 && fp.sigma_rad == 1e-3 && fp.gyro_sigma_rad == 0.0 && fp.z == 0.0);
    CHECK(ck_rig_refine_host(NULL, 1, I.rec, 1, I.tags, I.nt, I.bear, 4 * I.nt, NULL, &start, NULL, &out) == CK_EINVAL);
    fp.max_iters = 101;
    CHECK(ck_rig_refine_host(&fp, 1, I.rec, 1, I.tags, I.nt, I.bear, 4 * I.nt, NULL, &start, NULL, &out) == CK_EINVAL);
    fp.max_iters = 10; fp.gyro_sigma_rad = 0.01;
    CHECK(ck_rig_refine_host(&fp, 1, I.rec, 1, I.tags, I.nt, I.bear, 4 * I.nt, NULL, &start, NULL, &out) == CK_EINVAL);
    CHECK(memcmp(&out, &keep, sizeof out) == 0);
    free(I.tags); free(I.bear);
    printf("ok\n");
    return 0;
}
