// Coloured game pieces, the half that needs no device: the parameter check every entry point shares, the tuning helper
// and the one-thread twin of the kernels.  The classifier, the filter, the order and the derived doubles are ck_blob_math.h's, the
// same text the kernels compile; the morphology and the labelling are written per pixel here, as plainly as the definition reads,
// where the kernels work on packed words and runs.
#include <stdlib.h>
#include <string.h>

#include "chalkydri_hip.h"
#include "ck_blob_math.h"

void ck_blob_params_default(ck_blob_params_t *pp) {
    if (!pp) return;
    memset(pp, 0, sizeof *pp);
    pp->n_classes = 1;
    pp->max_targets = 16;
    pp->max_components = 4096;
    pp->max_range = 20.0;
    for (int c = 0; c < CK_BLOB_MAX_CLASSES; c++) {
        ck_blob_class_t *k = &pp->cls[c];
        k->h_max = 179; k->s_min = 64; k->s_max = 255; k->v_min = 64; k->v_max = 255;
        k->min_area = 16;
    }
    pp->robot_to_cam.q[0] = 1.0;
}

int ck_blob_check(const ck_blob_params_t *pp) {
    if (!pp) return CK_EINVAL;
    if (pp->n_classes < 1 || pp->n_classes > CK_BLOB_MAX_CLASSES) return CK_EINVAL;
    if (pp->erode < 0 || pp->erode > 4 || pp->dilate < 0 || pp->dilate > 4) return CK_EINVAL;
    if (pp->max_targets < 0) return CK_EINVAL;
    if (pp->max_components < 1) return CK_EINVAL;
    for (int c = 0; c < pp->n_classes; c++) {
        const ck_blob_class_t *k = &pp->cls[c];
        if (k->h_min < 0 || k->h_min > 179 || k->h_max < 0 || k->h_max > 179) return CK_EINVAL;
        if (k->s_min < 0 || k->s_min > 255 || k->s_max < 0 || k->s_max > 255) return CK_EINVAL;
        if (k->v_min < 0 || k->v_min > 255 || k->v_max < 0 || k->v_max > 255) return CK_EINVAL;
        if (k->min_area < 0 || k->max_area < 0) return CK_EINVAL;
        if (k->min_fill_permille < 0 || k->min_aspect_permille < 0 || k->max_aspect_permille < 0) return CK_EINVAL;
        if (!ckm_finite(k->ground_z)) return CK_EINVAL;
    }
    if (pp->has_camera && ck_camera_check(&pp->cam) != CK_OK) return CK_EINVAL;
    if (pp->has_mount) {
        const double *t = pp->robot_to_cam.t, *q = pp->robot_to_cam.q;
        for (int i = 0; i < 3; i++)
            if (!ckm_finite(t[i])) return CK_EINVAL;
        for (int i = 0; i < 4; i++)
            if (!ckm_finite(q[i])) return CK_EINVAL;
        if (!(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] > 0.0)) return CK_EINVAL;
    }
    if (!ckm_finite(pp->max_range) || pp->max_range < 0.0) return CK_EINVAL;
    return CK_OK;
}

int ck_blob_rgb_hsv(const uint8_t *rgb, int64_t n, uint8_t *hsv_out) {
    if (!rgb || !hsv_out || n < 0) return CK_EINVAL;
    for (int64_t i = 0; i < n; i++) {
        int h, s, v;
        ckb_hsv(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], &h, &s, &v);
        hsv_out[3 * i] = (uint8_t)h; hsv_out[3 * i + 1] = (uint8_t)s; hsv_out[3 * i + 2] = (uint8_t)v;
    }
    return CK_OK;
}

static int geometry_ok(const ck_blob_params_t *pp, const uint8_t *rgb, int32_t W, int32_t H, int32_t n) {
    if (ck_blob_check(pp) != CK_OK || !rgb || W < 1 || H < 1 || n < 0) return 0;
    return (int64_t)W * H < ((int64_t)1 << 31);
}

// class c's plane of one frame, one byte per pixel, at `stage`; tmp: another W H bytes
static void plane_of(const ck_blob_params_t *pp, const uint8_t *rgb, int W, int H, int c, int stage, uint8_t *m, uint8_t *tmp) {
    for (size_t i = 0; i < (size_t)W * H; i++) m[i] = (uint8_t)ckb_class_pass(&pp->cls[c], rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]);
    if (stage == 0) return;
    for (int it = 0; it < pp->erode + pp->dilate; it++) {
        const int dil = it >= pp->erode;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                int v = dil ? 0 : 1;
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++) {
                        const int xx = x + dx, yy = y + dy;
                        const int s = xx >= 0 && xx < W && yy >= 0 && yy < H ? m[(size_t)yy * W + xx] : 0; // outside: background
                        if (dil) v |= s; else v &= s;
                    }
                tmp[(size_t)y * W + x] = (uint8_t)v;
            }
        memcpy(m, tmp, (size_t)W * H);
    }
}

int ck_blob_mask_host(const ck_blob_params_t *pp, const uint8_t *rgb, int32_t W, int32_t H, int32_t n, int32_t cls, int32_t stage,
                      uint32_t *bits_out) {
    if (!geometry_ok(pp, rgb, W, H, n) || !bits_out || cls < 0 || cls >= pp->n_classes || stage < 0 || stage > 1) return CK_EINVAL;
    if (n == 0) return CK_OK;
    const size_t np = (size_t)W * H;
    const int ww = (W + 31) / 32;
    uint8_t *m = (uint8_t *)malloc(2 * np);
    if (!m) return CK_ENOMEM;
    memset(bits_out, 0, sizeof(uint32_t) * (size_t)ww * H * n);
    for (int f = 0; f < n; f++) {
        plane_of(pp, rgb + 3 * np * f, W, H, cls, stage, m, m + np);
        uint32_t *o = bits_out + (size_t)ww * H * f;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++)
                if (m[(size_t)y * W + x]) o[(size_t)y * ww + (x >> 5)] |= 1u << (x & 31);
    }
    free(m);
    return CK_OK;
}

static int32_t find_root(int32_t *p, int32_t i) {
    while (p[i] != i) { p[i] = p[p[i]]; i = p[i]; }
    return i;
}
static void unite(int32_t *p, int32_t a, int32_t b) { // the smaller index stays the root: a component's root is its seed
    a = find_root(p, a); b = find_root(p, b);
    if (a < b) p[b] = a; else p[a] = b;
}

static int by_rank(const void *pa, const void *pb) {
    const ckb_comp *a = (const ckb_comp *)pa, *b = (const ckb_comp *)pb;
    return ckb_before(a->area, a->seed, b->area, b->seed) ? -1 : 1; // (seeds are unique: no two compare equal)
}

int ck_blobs_host(const ck_blob_params_t *pp, const uint8_t *rgb, int32_t W, int32_t H, int32_t n, ck_blob_t *out, int32_t cap,
                  int32_t *counts, uint32_t *status) {
    if (!geometry_ok(pp, rgb, W, H, n) || !out || !counts || cap < 0) return CK_EINVAL;
    if (n == 0) return CK_OK;
    const size_t np = (size_t)W * H;
    const int nc = pp->n_classes;
    uint8_t *m = (uint8_t *)malloc(2 * np);
    int32_t *par = (int32_t *)malloc(sizeof(int32_t) * np), *slot = (int32_t *)malloc(sizeof(int32_t) * np);
    ckb_comp *comps = (ckb_comp *)malloc(sizeof(ckb_comp) * (size_t)pp->max_components);
    if (!m || !par || !slot || !comps) { free(m); free(par); free(slot); free(comps); return CK_ENOMEM; }
    ckb_geo geo;
    ckb_geo_make(pp, pp->has_camera ? &pp->cam : 0, &geo);
    memset(out, 0, sizeof(ck_blob_t) * (size_t)n * nc * cap);
    for (int f = 0; f < n; f++) {
        uint32_t st = 0;
        for (int c = 0; c < nc; c++) {
            const ck_blob_class_t *K = &pp->cls[c];
            plane_of(pp, rgb + 3 * np * f, W, H, c, 1, m, m + np);
            // 8-connected components: the four neighbours that come earlier in raster order
            for (int y = 0; y < H; y++)
                for (int x = 0; x < W; x++) {
                    const int32_t i = (int32_t)((size_t)y * W + x);
                    if (!m[i]) continue;
                    par[i] = i;
                    if (x > 0 && m[i - 1]) unite(par, i, i - 1);
                    if (y > 0) {
                        if (x > 0 && m[i - W - 1]) unite(par, i, i - W - 1);
                        if (m[i - W]) unite(par, i, i - W);
                        if (x < W - 1 && m[i - W + 1]) unite(par, i, i - W + 1);
                    }
                }
            // area first: only the roots of min_area pixels and more take one of the max_components slots
            for (size_t i = 0; i < np; i++)
                if (m[i]) { par[i] = find_root(par, (int32_t)i); slot[i] = 0; }
            for (size_t i = 0; i < np; i++)
                if (m[i]) slot[par[i]]++;
            int64_t ncomp = 0;
            for (size_t i = 0; i < np; i++) {
                if (!m[i] || par[i] != (int32_t)i) continue;
                const int32_t area = slot[i];
                slot[i] = -1;
                if (area < K->min_area) continue;
                if (ncomp < pp->max_components) {
                    ckb_comp *k = &comps[ncomp];
                    memset(k, 0, sizeof *k);
                    k->area = area; k->seed = (int32_t)i;
                    k->x0 = W; k->y0 = H; k->x1 = -1; k->y1 = -1;
                    slot[i] = (int32_t)ncomp;
                }
                ncomp++;
            }
            int32_t *cnt = &counts[(size_t)f * nc + c];
            *cnt = 0;
            if (ncomp > pp->max_components) { st |= CK_BLOB_OVERFLOW; continue; }
            for (int y = 0; y < H; y++)
                for (int x = 0; x < W; x++) {
                    const size_t i = (size_t)y * W + x;
                    if (!m[i] || slot[par[i]] < 0) continue;
                    ckb_comp *k = &comps[slot[par[i]]];
                    if (x < k->x0) k->x0 = x;
                    if (x > k->x1) k->x1 = x;
                    if (y < k->y0) k->y0 = y;
                    if (y > k->y1) k->y1 = y;
                    k->sx += x; k->sy += y; k->sxx += (int64_t)x * x; k->sxy += (int64_t)x * y; k->syy += (int64_t)y * y;
                }
            int np_pass = 0;
            for (int64_t j = 0; j < ncomp; j++)
                if (ckb_filter(K, &comps[j])) comps[np_pass++] = comps[j];
            qsort(comps, (size_t)np_pass, sizeof(ckb_comp), by_rank);
            *cnt = np_pass;
            int nw = np_pass < pp->max_targets ? np_pass : pp->max_targets;
            if (cap < nw) nw = cap;
            if (nw < np_pass) st |= CK_BLOB_TRUNCATED;
            for (int j = 0; j < nw; j++) ckb_record(&comps[j], c, K->ground_z, W, H, &geo, &out[((size_t)f * nc + c) * cap + j]);
        }
        if (status) status[f] = st;
    }
    free(m); free(par); free(slot); free(comps);
    return CK_OK;
}
