// Sub-pixel corners, the half that needs no device: the parameter checks every entry point shares, the weight table,
// and the one-thread twins of k_subpix and k_board.  The arithmetic is ck_subpix_math.h's, the same text the kernels compile; the
// window sums walk the kernels' lanes one after the other and add them up in the kernels' tree, so the bytes are theirs.
#include <string.h>

#include "ck_subpix_math.h"

// lane by lane, then the tree: what a wave does at once
static inline void cks_window_sums(const cks_image *im, double x, double y, int w, const double *wts, double S[5]) {
    double part[5][CKS_LANES];
    for (int t = 0; t < CKS_LANES; t++) {
        double s[5];
        cks_lane_sums(im, x, y, w, wts, t, s);
        for (int q = 0; q < 5; q++) part[q][t] = s[q];
    }
    for (int q = 0; q < 5; q++) S[q] = cks_tree_sum(part[q]);
}

void ck_subpix_params_default(ck_subpix_params_t *pp) {
    if (!pp) return;
    pp->half_win = 5;
    pp->max_iters = 30;
    pp->eps = 1e-3;
    // the determinant of a window with one edge in it is zero, and a c - b b leaves a rounding residue of up to 2^-52 a c:
    // 1.4e-3 for the largest window at full contrast (a, c <= 153 * 127.5^2).  One order above that; a corner of a single grey
    // level is at 0.1 and more
    pp->det_min = 1e-2;
}

int ck_subpix_params_check(const ck_subpix_params_t *pp) {
    if (!pp) return CK_EINVAL;
    if (pp->half_win < 2 || pp->half_win > CKS_MAX_HALF || pp->max_iters < 1 || pp->max_iters > 1000) return CK_EINVAL;
    if (!cks_finite(pp->eps) || !(pp->eps >= 0.0) || !cks_finite(pp->det_min) || !(pp->det_min >= 0.0)) return CK_EINVAL;
    return CK_OK;
}

int ck_subpix_weights(const ck_subpix_params_t *pp, double *w_out) {
    const int rc = ck_subpix_params_check(pp);
    if (rc != CK_OK) return rc;
    if (!w_out) return CK_EINVAL;
    const int w = pp->half_win, side = 2 * w + 1;
    double e[2 * CKS_MAX_HALF + 1];
    for (int i = 0; i < side; i++) {
        const double d = (double)(i - w) / (double)w;
        e[i] = exp(-(d * d));
    }
    for (int iy = 0; iy < side; iy++)
        for (int ix = 0; ix < side; ix++) w_out[iy * side + ix] = e[ix] * e[iy];
    return CK_OK;
}

// a point the refinement takes: finite and inside the closed frame
int ck_subpix_point_ok(double x, double y, int width, int height) {
    return cks_finite(x) && cks_finite(y) && x >= 0.0 && x <= (double)width && y >= 0.0 && y <= (double)height;
}

static int images_ok(const ck_image_u8_t *imgs, int32_t n) {
    if (n < 0 || (n > 0 && !imgs)) return 0;
    for (int32_t i = 0; i < n; i++)
        if (!imgs[i].buf || imgs[i].width < 1 || imgs[i].height < 1 || imgs[i].stride < imgs[i].width || imgs[i].width != imgs[0].width ||
            imgs[i].height != imgs[0].height)
            return 0;
    return 1;
}
static cks_image image_of(const ck_image_u8_t *im) {
    cks_image r;
    r.p = im->buf; r.stride = im->stride; r.w = im->width; r.h = im->height;
    return r;
}

int ck_corner_subpix_host(const ck_subpix_params_t *pp, const ck_image_u8_t *imgs, int32_t n_imgs, const int32_t *frame, const double *xy_in,
                          int32_t n, double *xy_out, ck_subpix_info_t *info) {
    int rc = ck_subpix_params_check(pp);
    if (rc != CK_OK) return rc;
    if (n < 0 || !images_ok(imgs, n_imgs)) return CK_EINVAL;
    if (n == 0) return CK_OK;
    if (!xy_in || !xy_out || n_imgs < 1) return CK_EINVAL;
    for (int32_t i = 0; i < n; i++) {
        const int f = frame ? frame[i] : 0;
        if (f < 0 || f >= n_imgs || !ck_subpix_point_ok(xy_in[2 * (size_t)i], xy_in[2 * (size_t)i + 1], imgs[0].width, imgs[0].height)) return CK_EINVAL;
    }
    double wts[CKS_MAX_TAPS];
    rc = ck_subpix_weights(pp, wts);
    if (rc != CK_OK) return rc;
    for (int32_t i = 0; i < n; i++) {
        const cks_image im = image_of(&imgs[frame ? frame[i] : 0]);
        int32_t st, it;
        double sh, ox, oy;
        cks_refine(&im, pp, wts, xy_in[2 * (size_t)i], xy_in[2 * (size_t)i + 1], &ox, &oy, &st, &it, &sh);
        xy_out[2 * (size_t)i] = ox; xy_out[2 * (size_t)i + 1] = oy;
        if (info) { info[i].status = st; info[i].iters = it; info[i].shift = sh; }
    }
    return CK_OK;
}

void ck_board_params_default(ck_board_params_t *bp) {
    if (!bp) return;
    bp->seed_max_shift = 2.0;
    bp->max_shift = 2.5;
    bp->probe[0] = 0.7; bp->probe[1] = -0.6;
    bp->agree = 0.05;
}

// n_families < 0: the caller has no handle to hold the family against
int ck_board_check(const ck_board_t *b, const ck_board_params_t *bp, int n_families) {
    if (!b || !bp) return CK_EINVAL;
    if (b->rows < 1 || b->cols < 1 || (int64_t)b->rows * b->cols > CKS_MAX_TAGS) return CK_EINVAL;
    if (b->family < 0 || b->family >= CK_MAX_FAMILIES || (n_families >= 0 && b->family >= n_families)) return CK_EINVAL;
    if (!cks_finite(b->tag_size) || !(b->tag_size > 0.0) || !cks_finite(b->tag_spacing) || !(b->tag_spacing >= 0.0)) return CK_EINVAL;
    const double v[5] = {bp->seed_max_shift, bp->max_shift, bp->agree, bp->probe[0], bp->probe[1]};
    for (int i = 0; i < 5; i++)
        if (!cks_finite(v[i]) || (i < 3 && !(v[i] >= 0.0))) return CK_EINVAL;
    return CK_OK;
}

int ck_board_corners_host(const ck_board_t *board, const ck_subpix_params_t *pp, const ck_board_params_t *bp, const ck_image_u8_t *imgs,
                          int32_t n, const ck_detection_t *dets, int32_t cap_per_frame, const int32_t *counts, double *uv_out,
                          uint8_t *tag_state, int32_t *n_tags) {
    int rc = ck_subpix_params_check(pp);
    if (rc == CK_OK) rc = ck_board_check(board, bp, -1);
    if (rc != CK_OK) return rc;
    if (n < 0 || cap_per_frame < 1 || !images_ok(imgs, n)) return CK_EINVAL;
    if (n == 0) return CK_OK;
    if (!dets || !counts || !uv_out || !tag_state || !n_tags) return CK_EINVAL;
    for (int32_t f = 0; f < n; f++)
        if (counts[f] < 0 || counts[f] > cap_per_frame) return CK_EINVAL;
    double wts[CKS_MAX_TAPS];
    rc = ck_subpix_weights(pp, wts);
    if (rc != CK_OK) return rc;
    const int nt = board->rows * board->cols, w = pp->half_win;
    for (int32_t f = 0; f < n; f++) {
        const cks_image im = image_of(&imgs[f]);
        double *uv = uv_out + (size_t)f * nt * 8;
        uint8_t *state = tag_state + (size_t)f * nt;
        uint8_t seen[CKS_MAX_TAGS], next[CKS_MAX_TAGS];
        memset(uv, 0, sizeof(double) * 8 * (size_t)nt);
        memset(state, 0, (size_t)nt);
        memset(seen, 0, sizeof seen);
        int known = 0;
        for (int32_t i = 0; i < counts[f]; i++) {
            const ck_detection_t *d = dets + (size_t)f * cap_per_frame + i;
            const int t = cks_seed_index(board, d);
            if (t < 0 || seen[t]) continue;
            seen[t] = 1;
            double r[8];
            int ok = 1;
            for (int k = 0; k < 4; k++) ok &= cks_seed_corner(&im, pp, bp, wts, d->p[k][0], d->p[k][1], &r[2 * k], &r[2 * k + 1]);
            if (!ok) continue;
            memcpy(uv + 8 * (size_t)t, r, sizeof r);
            state[t] = 1;
            known++;
        }
        for (int round = 0; round < board->rows + board->cols; round++) {
            int added = 0;
            memcpy(next, state, (size_t)nt);
            for (int t = 0; t < nt; t++) {
                if (state[t]) continue;
                int dc, dr;
                const int nb = cks_first_neighbour(board, state, t, &dc, &dr);
                if (nb < 0) continue;
                double x[4], y[4], G[9], r[8];
                for (int k = 0; k < 4; k++) { x[k] = uv[8 * (size_t)nb + 2 * k]; y[k] = uv[8 * (size_t)nb + 2 * k + 1]; }
                if (!cks_square_homography(x, y, G)) continue;
                int ok = 1;
                double px[4], py[4];
                for (int k = 0; k < 4; k++) {
                    double X, Y;
                    cks_corner_from_neighbour(board, dc, dr, k, &X, &Y);
                    ok = ok && cks_map(G, X, Y, &px[k], &py[k]) && !cks_near_edge(&im, w, px[k], py[k]);
                }
                if (!ok) continue;
                for (int k = 0; k < 4; k++) ok &= cks_board_corner(&im, pp, bp, wts, px[k], py[k], &r[2 * k], &r[2 * k + 1]);
                if (!ok) continue;
                memcpy(uv + 8 * (size_t)t, r, sizeof r);
                next[t] = 2;
                added++;
            }
            memcpy(state, next, (size_t)nt);
            known += added;
            if (!added) break;
        }
        n_tags[f] = known;
    }
    return CK_OK;
}
