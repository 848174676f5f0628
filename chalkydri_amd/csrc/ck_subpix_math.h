// ck_subpix_math.h — the arithmetic of the sub-pixel corner refinement and of the board recovery, written once and
// compiled twice, as ck_camera_math.h is: as C into the host twins (ck_subpix_host.c) and as device code into the kernels
// (ck_subpix.hip).  Only + - * / sqrt on doubles, every expression evaluated as written (-ffp-contract=off on both sides), so the two
// produce the same bytes.  THE OPERATION ORDER IS PART OF THE CONTRACT.
//
// One thing differs between the two sides and is therefore not in this file: how the five sums of a window are formed from the
// partial sums of 64 lanes.  The including file defines cks_window_sums() after the include — the kernel with one lane of a wave per
// partial sum and a butterfly over the lanes, the twin with a loop over the lanes and the same tree (cks_tree_sum) — and everything
// below it, from the step to the board rounds, is this text on both sides.
#ifndef CK_SUBPIX_MATH_H
#define CK_SUBPIX_MATH_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "chalkydri_hip.h"

#if defined(__HIPCC__)
#define CKS_FN static __device__ __forceinline__
#else
#define CKS_FN static inline
#endif

#define CKS_LANES 64
#define CKS_MAX_HALF 7
#define CKS_MAX_TAPS ((2 * CKS_MAX_HALF + 1) * (2 * CKS_MAX_HALF + 1))
#define CKS_MAX_TAGS 64 /* tags of a board */

// one frame of 8-bit pixels, wherever it lies
typedef struct cks_image {
    const uint8_t *p;
    int stride, w, h;
} cks_image;

CKS_FN int cks_finite(double x) { return x - x == 0.0; }
CKS_FN double cks_abs(double x) { return x < 0.0 ? -x : x; }

// floor(v) and v - floor(v) of a sampling coordinate, v kept within 32 pixels of the frame first (NaN becomes the lower end): an
// estimate that ran away samples the clamped frame edge, where a window is flat, and the conversion to int is always defined
CKS_FN int cks_base(double v, int size, double *frac) {
    const double lo = -32.0, hi = (double)size + 32.0;
    if (!(v >= lo)) v = lo;
    if (v > hi) v = hi;
    int i = (int)v;
    if ((double)i > v) i--;
    *frac = v - (double)i;
    return i;
}
CKS_FN double cks_pix(const cks_image *im, int x, int y) {
    x = x < 0 ? 0 : (x > im->w - 1 ? im->w - 1 : x);
    y = y < 0 ? 0 : (y > im->h - 1 ? im->h - 1 : y);
    return (double)im->p[(size_t)y * (size_t)im->stride + (size_t)x];
}
// bilinear sample whose upper left pixel is (x, y)
CKS_FN double cks_sample(const cks_image *im, int x, int y, double fx, double ux, double fy, double uy) {
    const double top = cks_pix(im, x, y) * ux + cks_pix(im, x + 1, y) * fx;
    const double bot = cks_pix(im, x, y + 1) * ux + cks_pix(im, x + 1, y + 1) * fx;
    return top * uy + bot * fy;
}

// The projective map of the tag square S_i = (-1,1), (1,1), (1,-1), (-1,-1) onto the points (x_i, y_i), row-major, up to scale:
// Heckbert's unit-square mapping composed with (u, v) = ((X + 1) / 2, (1 - Y) / 2), which sends S_i to the unit square's
// (0,0), (1,0), (1,1), (0,1).  0 when the points do not define one (den == 0, or anything non-finite).  The per-tag pose's routine
// (k_tagpose.hip calls this text).
CKS_FN int cks_square_homography(const double x[4], const double y[4], double G[9]) {
    const double sx = x[0] - x[1] + x[2] - x[3], sy = y[0] - y[1] + y[2] - y[3];
    const double dx1 = x[1] - x[2], dx2 = x[3] - x[2], dy1 = y[1] - y[2], dy2 = y[3] - y[2];
    const double den = dx1 * dy2 - dx2 * dy1;
    if (den == 0.0) return 0;
    const double g = (sx * dy2 - dx2 * sy) / den, hh = (dx1 * sy - sx * dy1) / den;
    const double a = x[1] - x[0] + g * x[1], b = x[3] - x[0] + hh * x[3], c = x[0];
    const double d = y[1] - y[0] + g * y[1], e = y[3] - y[0] + hh * y[3], f = y[0];
    G[0] = 0.5 * a; G[1] = -0.5 * b; G[2] = 0.5 * (a + b) + c;
    G[3] = 0.5 * d; G[4] = -0.5 * e; G[5] = 0.5 * (d + e) + f;
    G[6] = 0.5 * g; G[7] = -0.5 * hh; G[8] = 0.5 * (g + hh) + 1.0;
    int ok = 1;
    for (int i = 0; i < 9; i++) ok = ok && cks_finite(G[i]);
    return ok;
}
// the image of the tag-square point (X, Y) under G; 0 when it is not finite
CKS_FN int cks_map(const double G[9], double X, double Y, double *u, double *v) {
    const double d = G[6] * X + G[7] * Y + G[8];
    *u = (G[0] * X + G[1] * Y + G[2]) / d;
    *v = (G[3] * X + G[4] * Y + G[5]) / d;
    return cks_finite(*u) && cks_finite(*v);
}

#ifndef CKS_HOMOGRAPHY_ONLY /* k_tagpose.hip takes the homography alone */

// Lane t's share of the window sums at the estimate (x, y): taps t, t + 64, ... in increasing order, tap k = iy * (2w + 1) + ix.
// s = {a, b, c, b1, b2}
CKS_FN void cks_lane_sums(const cks_image *im, double x, double y, int w, const double *wts, int t, double s[5]) {
    double fx, fy;
    const int ix0 = cks_base(x - 0.5, im->w, &fx), iy0 = cks_base(y - 0.5, im->h, &fy);
    const double ux = 1.0 - fx, uy = 1.0 - fy;
    const int side = 2 * w + 1, taps = side * side;
    double a = 0.0, b = 0.0, c = 0.0, b1 = 0.0, b2 = 0.0;
    for (int k = t; k < taps; k += CKS_LANES) {
        const int iy = k / side, ix = k - iy * side;
        const int X = ix0 + ix - w, Y = iy0 + iy - w;
        const double gx = (cks_sample(im, X + 1, Y, fx, ux, fy, uy) - cks_sample(im, X - 1, Y, fx, ux, fy, uy)) * 0.5;
        const double gy = (cks_sample(im, X, Y + 1, fx, ux, fy, uy) - cks_sample(im, X, Y - 1, fx, ux, fy, uy)) * 0.5;
        const double px = (double)(ix - w), py = (double)(iy - w);
        const double m = wts[k];
        const double mgx = m * gx, mgy = m * gy;
        const double gxx = mgx * gx, gxy = mgx * gy, gyy = mgy * gy;
        a = a + gxx;
        b = b + gxy;
        c = c + gyy;
        b1 = b1 + (gxx * px + gxy * py);
        b2 = b2 + (gxy * px + gyy * py);
    }
    s[0] = a; s[1] = b; s[2] = c; s[3] = b1; s[4] = b2;
}

// the fixed pairwise tree over 64 partial sums, in place: v[t] += v[t + s] for t < s, s = 32, 16, ..., 1.  (The kernel's butterfly
// v += v[lane ^ s] forms the same sums in lane 0, and, addition being commutative, the same bits in every lane.)
CKS_FN double cks_tree_sum(double *v) {
    for (int s = CKS_LANES / 2; s >= 1; s >>= 1)
        for (int t = 0; t < s; t++) v[t] = v[t] + v[t + s];
    return v[0];
}

// defined by the including file: the five window sums at (x, y), the same in every lane that calls it
CKS_FN void cks_window_sums(const cks_image *im, double x, double y, int w, const double *wts, double S[5]);

// One point.  FLAT and REJECTED return the input's bytes.
CKS_FN void cks_refine(const cks_image *im, const ck_subpix_params_t *pp, const double *wts, double x0, double y0, double *ox, double *oy,
                       int32_t *status_o, int32_t *iters_o, double *shift_o) {
    const int w = pp->half_win;
    const double eps2 = pp->eps * pp->eps, wd = (double)w;
    double x = x0, y = y0;
    int status = CK_SUBPIX_MAXIT, it = 0;
    while (it < pp->max_iters) {
        double S[5];
        cks_window_sums(im, x, y, w, wts, S);
        const double a = S[0], b = S[1], c = S[2], b1 = S[3], b2 = S[4];
        const double det = a * c - b * b;
        if (cks_abs(det) <= pp->det_min) { status = CK_SUBPIX_FLAT; break; }
        const double dx = (c * b1 - b * b2) / det, dy = (a * b2 - b * b1) / det;
        x = x + dx; y = y + dy;
        it++;
        if (dx * dx + dy * dy <= eps2) { status = CK_SUBPIX_CONVERGED; break; }
    }
    const double mx = x - x0, my = y - y0;
    if (status != CK_SUBPIX_FLAT && (!(cks_abs(mx) <= wd) || !(cks_abs(my) <= wd))) status = CK_SUBPIX_REJECTED; // (a NaN is rejected too)
    const int keep = status == CK_SUBPIX_FLAT || status == CK_SUBPIX_REJECTED;
    *ox = keep ? x0 : x;
    *oy = keep ? y0 : y;
    *status_o = status;
    *iters_o = it;
    *shift_o = keep ? 0.0 : sqrt(mx * mx + my * my);
}

// ---- board recovery ---------------------------------------------------------------------------------------------------------------
// A board tag's corner k lies at the tag's centre + (tag_size / 2) * S_k.  Seen from a neighbour tag whose centre is (dc, dr) grid
// steps away, in that neighbour's tag-square coordinates (its own corners are S_k): S_k + 2 (1 + tag_spacing) (dc, dr).
CKS_FN void cks_corner_from_neighbour(const ck_board_t *b, int dc, int dr, int k, double *X, double *Y) {
    const double step = 2.0 * (1.0 + b->tag_spacing);
    const double sx = (k == 1 || k == 2) ? 1.0 : -1.0, sy = (k == 0 || k == 1) ? 1.0 : -1.0;
    *X = sx + step * (double)dc;
    *Y = sy + step * (double)dr;
}
// a prediction within half_win + 2 pixels of the frame edge (or not finite) is not tried
CKS_FN int cks_near_edge(const cks_image *im, int w, double x, double y) {
    const double m = (double)(w + 2);
    return !(x >= m && x <= (double)im->w - m && y >= m && y <= (double)im->h - m);
}
// One corner of a candidate tag from its prediction (px, py): the refined point, and whether it converged within max_shift and a
// second refinement started `probe` away from it came back to within `agree` of it
CKS_FN int cks_board_corner(const cks_image *im, const ck_subpix_params_t *pp, const ck_board_params_t *bp, const double *wts, double px,
                            double py, double *rx, double *ry) {
    int32_t st, it;
    double sh, qx, qy;
    cks_refine(im, pp, wts, px, py, rx, ry, &st, &it, &sh);
    if (st != CK_SUBPIX_CONVERGED || !(sh <= bp->max_shift)) return 0;
    cks_refine(im, pp, wts, *rx + bp->probe[0], *ry + bp->probe[1], &qx, &qy, &st, &it, &sh);
    const double ex = qx - *rx, ey = qy - *ry;
    return ex * ex + ey * ey <= bp->agree * bp->agree;
}
// One corner of a seed: the refined point (the input for FLAT and REJECTED), and whether it moved at most seed_max_shift
CKS_FN int cks_seed_corner(const cks_image *im, const ck_subpix_params_t *pp, const ck_board_params_t *bp, const double *wts, double px,
                           double py, double *rx, double *ry) {
    int32_t st, it;
    double sh;
    cks_refine(im, pp, wts, px, py, rx, ry, &st, &it, &sh);
    return sh <= bp->seed_max_shift;
}
// a detection that may seed the board: its tag's index on the board, or -1
CKS_FN int cks_seed_index(const ck_board_t *b, const ck_detection_t *d) {
    if (d->family != b->family || d->hamming != 0) return -1;
    const int64_t k = (int64_t)d->id - (int64_t)b->first_id;
    return (k >= 0 && k < (int64_t)b->rows * b->cols) ? (int)k : -1;
}
// The first known 4-neighbour of tag t (row-major) in the order left, right, up, down: its index, or -1
CKS_FN int cks_first_neighbour(const ck_board_t *b, const uint8_t *state, int t, int *dc, int *dr) {
    const int r = t / b->cols, c = t - r * b->cols;
    if (c > 0 && state[t - 1]) { *dc = 1; *dr = 0; return t - 1; }
    if (c + 1 < b->cols && state[t + 1]) { *dc = -1; *dr = 0; return t + 1; }
    if (r > 0 && state[t - b->cols]) { *dc = 0; *dr = 1; return t - b->cols; }
    if (r + 1 < b->rows && state[t + b->cols]) { *dc = 0; *dr = -1; return t + b->cols; }
    return -1;
}

#endif /* CKS_HOMOGRAPHY_ONLY */

#endif
