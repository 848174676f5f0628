// ck_blob_math.h — the arithmetic of the coloured-piece detector, written once and compiled twice, as ck_camera_math.h
// is: as C into the host twin (ck_blobs_host.c) and as device code into the kernels (k_blobs.hip).  The classifier is integer
// arithmetic; the derived doubles use only + - * / sqrt, every expression evaluated as written (-ffp-contract=off on both sides), so
// the two sides produce the same bytes.  THE OPERATION ORDER IS PART OF THE CONTRACT.
#ifndef CK_BLOB_MATH_H
#define CK_BLOB_MATH_H

#include <stdint.h>

#include "chalkydri_hip.h"
#include "ck_camera_math.h"
#include "ck_pose_math.h"

#define CKB_FN CKM_FN

// libjpeg's ycc_rgb_convert (jdcolor.c) in 16-bit fixed point; the shifts are arithmetic
CKB_FN int ckb_clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
CKB_FN void ckb_ycc_rgb(int y, int cb, int cr, int *r, int *g, int *b) {
    const int u = cb - 128, v = cr - 128;
    *r = ckb_clamp8(y + ((91881 * v + 32768) >> 16));
    *g = ckb_clamp8(y + ((-22554 * u - 46802 * v + 32768) >> 16));
    *b = ckb_clamp8(y + ((116130 * u + 32768) >> 16));
}

// What the classifier compares: V, d = V - min, and the hue as the fraction num / den before its floor, H = floor(num / den) mod 180
// with num = 2 hn + d in [d, 361 d) and den = 2 d (d = 0: 0 / 1).  Ties for the maximum go to R, then G, then B.
CKB_FN void ckb_hsv_terms(int r, int g, int b, int *V, int *d, int *num, int *den) {
    const int mx = r > g ? (r > b ? r : b) : (g > b ? g : b), mn = r < g ? (r < b ? r : b) : (g < b ? g : b);
    const int dd = mx - mn;
    int hn = 0;
    if (dd != 0) {
        if (mx == r) hn = 30 * (g - b) + (g < b ? 180 * dd : 0);
        else if (mx == g) hn = 30 * (b - r) + 60 * dd;
        else hn = 30 * (r - g) + 120 * dd;
    }
    *V = mx; *d = dd;
    *num = dd ? 2 * hn + dd : 0;
    *den = dd ? 2 * dd : 1;
}
// H >= k and H <= k for 0 <= k <= 179, by cross-multiplication: floor(num / den) reaches 180 exactly when num >= 180 den, and 180 is
// hue 0 (the mod 180 of the definition)
CKB_FN int ckb_h_ge(int num, int den, int k) { return num >= 180 * den ? k <= 0 : num >= k * den; }
CKB_FN int ckb_h_le(int num, int den, int k) { return num >= 180 * den ? 1 : num < (k + 1) * den; }
// S = V ? floor(255 d / V) : 0 against its bounds, the same way
CKB_FN int ckb_s_in(int V, int d, int lo, int hi) { return V == 0 ? lo <= 0 : (255 * d >= lo * V && 255 * d < (hi + 1) * V); }

CKB_FN int ckb_class_pass(const ck_blob_class_t *c, int r, int g, int b) {
    int V, d, num, den;
    ckb_hsv_terms(r, g, b, &V, &d, &num, &den);
    if (V < c->v_min || V > c->v_max) return 0;
    if (!ckb_s_in(V, d, c->s_min, c->s_max)) return 0;
    const int ge = ckb_h_ge(num, den, c->h_min), le = ckb_h_le(num, den, c->h_max);
    return c->h_min > c->h_max ? (ge || le) : (ge && le); // h_min > h_max: red wraps, [h_min, 179] or [0, h_max]
}

// the only place that divides: the tuning helper ck_blob_rgb_hsv
CKB_FN void ckb_hsv(int r, int g, int b, int *h, int *s, int *v) {
    int V, d, num, den;
    ckb_hsv_terms(r, g, b, &V, &d, &num, &den);
    *v = V;
    *s = V ? (255 * d) / V : 0;
    *h = (num / den) % 180;
}

// 3x3 square on the packed rows: bit x & 31 of word x >> 5.  l, m, r: a word's left neighbour, itself, its right neighbour
// (0 outside the row).  The three pixels x - 1, x, x + 1 of every bit of m, joined by AND or by OR.
CKB_FN uint32_t ckb_row3(uint32_t l, uint32_t m, uint32_t r, int dilate) {
    const uint32_t a = (m << 1) | (l >> 31), b = (m >> 1) | (r << 31);
    return dilate ? (a | m | b) : (a & m & b);
}

// One component's sums (k_blobs.hip accumulates them with integer atomics, the twin in a loop)
typedef struct ckb_comp {
    int32_t area, seed, x0, y0, x1, y1;
    int64_t sx, sy, sxx, sxy, syy;
} ckb_comp;

// the filter, all in integers
CKB_FN int ckb_filter(const ck_blob_class_t *c, const ckb_comp *k) {
    const int64_t N = k->area, bw = k->x1 - k->x0 + 1, bh = k->y1 - k->y0 + 1;
    if (N < c->min_area) return 0;
    if (c->max_area != 0 && N > c->max_area) return 0;
    if (1000 * N < (int64_t)c->min_fill_permille * bw * bh) return 0;
    if ((int64_t)c->min_aspect_permille * bh > 1000 * bw) return 0;
    if (c->max_aspect_permille != 0 && 1000 * bw > (int64_t)c->max_aspect_permille * bh) return 0;
    return 1;
}
// the order of the records: area descending, then seed ascending
CKB_FN int ckb_before(int32_t area_a, int32_t seed_a, int32_t area_b, int32_t seed_b) {
    return area_a > area_b || (area_a == area_b && seed_a < seed_b);
}

// What a call's geometry comes to, computed once on the host by both sides: the camera (UCM's k[5] already 1.0) and the mount as the
// ray origin -R^T t and R^T itself (robot_to_cam is cam from robot).
typedef struct ckb_geo {
    int32_t has_camera, model, has_mount, pad;
    double k[9];
    double Rt[9]; // R^T, row-major: robot from camera
    double o[3];  // camera centre in the robot frame
    double max_range;
} ckb_geo;

CKB_FN void ckb_geo_make(const ck_blob_params_t *pp, const ck_camera_t *cam, ckb_geo *g) {
    g->has_camera = cam != 0; g->model = cam ? cam->model : 0; g->pad = 0;
    g->has_mount = cam != 0 && pp->has_mount != 0;
    for (int i = 0; i < 9; i++) g->k[i] = 0.0;
    if (cam) ckm_effective(cam->model, cam->k, g->k);
    double R[9];
    quat_to_mat(pp->robot_to_cam.q, R);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) g->Rt[i * 3 + j] = g->has_mount ? R[j * 3 + i] : 0.0;
    for (int i = 0; i < 3; i++) {
        const double *t = pp->robot_to_cam.t;
        g->o[i] = g->has_mount ? -(g->Rt[i * 3] * t[0] + g->Rt[i * 3 + 1] * t[1] + g->Rt[i * 3 + 2] * t[2]) : 0.0;
    }
    g->max_range = pp->max_range;
}

CKB_FN int ckb_unproject(const ckb_geo *g, double u, double v, double *b) {
    return g->model == CK_CAMERA_OPENCV5 ? ckm_opencv5_unproject(g->k, u, v, b) : ckm_eucm_unproject(g->k, u, v, b);
}

// the record of one component that passed the filter
CKB_FN void ckb_record(const ckb_comp *k, int class_id, double ground_z, int W, int H, const ckb_geo *g, ck_blob_t *o) {
    o->class_id = class_id;
    o->flags = 0;
    o->area = k->area; o->x0 = k->x0; o->y0 = k->y0; o->x1 = k->x1; o->y1 = k->y1; o->seed = k->seed;
    o->sx = k->sx; o->sy = k->sy; o->sxx = k->sxx; o->sxy = k->sxy; o->syy = k->syy;
    if (k->x0 == 0 || k->y0 == 0 || k->x1 == W - 1 || k->y1 == H - 1) o->flags |= CK_BLOB_AT_BORDER;
    const double N = (double)k->area;
    const double mx = (double)k->sx / N, my = (double)k->sy / N;
    o->cx = mx + 0.5; o->cy = my + 0.5;
    // covariance of the pixel centres, its eigenvalues from the closed 2x2 form
    const double a = (double)k->sxx / N - mx * mx, b = (double)k->sxy / N - mx * my, c = (double)k->syy / N - my * my;
    const double tr = a + c, df = a - c;
    const double rt = sqrt(df * df + 4.0 * (b * b));
    double l1 = (tr + rt) / 2.0, l2 = (tr - rt) / 2.0;
    if (!(l1 > 0.0)) l1 = 0.0;
    if (!(l2 > 0.0)) l2 = 0.0;
    o->major = sqrt(l1); o->minor = sqrt(l2);
    double ax = 1.0, ay = 0.0;
    if (rt > 0.0) { // the eigenvector of the larger eigenvalue, from the better-conditioned row
        double vx, vy;
        if (a >= c) { vx = (df + rt) / 2.0; vy = b; } else { vx = b; vy = (rt - df) / 2.0; }
        const double nrm = sqrt(vx * vx + vy * vy);
        ax = vx / nrm; ay = vy / nrm;
        if (ax < 0.0 || (ax == 0.0 && ay < 0.0)) { ax = -ax; ay = -ay; }
    }
    o->axis[0] = ax; o->axis[1] = ay;
    o->bearing[0] = 0.0; o->bearing[1] = 0.0; o->bearing[2] = 0.0;
    o->ground[0] = 0.0; o->ground[1] = 0.0;
    if (!g->has_camera) return;
    double bb[3];
    if (ckb_unproject(g, o->cx, o->cy, bb)) {
        o->bearing[0] = bb[0]; o->bearing[1] = bb[1]; o->bearing[2] = bb[2];
        o->flags |= CK_BLOB_HAS_BEARING;
    }
    if (!g->has_mount) return;
    // the ray through the bottom centre of the box against the plane z = ground_z of the robot frame
    if (!ckb_unproject(g, (double)(k->x0 + k->x1 + 1) / 2.0, (double)(k->y1 + 1), bb)) return;
    const double dx = g->Rt[0] * bb[0] + g->Rt[1] * bb[1] + g->Rt[2] * bb[2];
    const double dy = g->Rt[3] * bb[0] + g->Rt[4] * bb[1] + g->Rt[5] * bb[2];
    const double dz = g->Rt[6] * bb[0] + g->Rt[7] * bb[1] + g->Rt[8] * bb[2];
    if (!(dz < 0.0) || !(g->o[2] > ground_z)) return;
    const double s = (ground_z - g->o[2]) / dz; // the range: the length of the unit ray down to the plane
    if (!(s <= g->max_range)) return;
    o->ground[0] = g->o[0] + s * dx; o->ground[1] = g->o[1] + s * dy;
    o->flags |= CK_BLOB_HAS_GROUND;
}

#endif
