// Iterative tri-class Otsu threshold, the host half that needs no device: parameter checks and the solve of one
// 256-bin histogram into the per-frame record and the class table.  Integer statistics throughout; the one floating-point
// expression, v(t), is two double multiplications and one division evaluated exactly as written (tests/np_tri_otsu.py restates it,
// k_tri_solve of k_tri_otsu.hip produces the same bytes on the device).
#include "chalkydri_hip.h"
#include <string.h>

void ck_tri_otsu_params_default(ck_tri_otsu_params_t *p) {
    if (!p) return;
    p->max_iters = 8; p->min_delta = 1;
    p->keep_tbd = 1; p->channels = 3;
}

int ck_tri_otsu_params_ok(const ck_tri_otsu_params_t *p); // (ck_tri_otsu.h: the device half asks here too, one place)
int ck_tri_otsu_params_ok(const ck_tri_otsu_params_t *p) {
    if (!p) return 0;
    if (p->max_iters < 1 || p->max_iters > CK_TRI_MAX_ROUNDS) return 0;
    if (p->min_delta < 1 || p->min_delta > 255) return 0;
    if (p->keep_tbd != 0 && p->keep_tbd != 1) return 0;
    return p->channels == 1 || p->channels == 3;
}

int ck_tri_otsu_solve(const ck_tri_otsu_params_t *p, const uint32_t *hist, ck_tri_otsu_info_t *info, uint8_t *lut) {
    if (!ck_tri_otsu_params_ok(p) || !hist || !info || !lut) return CK_EINVAL;
    memset(info, 0, sizeof *info);
    for (int k = 0; k < CK_TRI_MAX_ROUNDS; k++) info->T[k] = -1;
    int lo = 0, hi = 255, T_last = -1, rounds = 0;
    for (int k = 1;; k++) {
        int64_t N = 0, S = 0;
        int occupied = 0;
        for (int g = lo; g <= hi; g++)
            if (hist[g]) { N += hist[g]; S += (int64_t)g * hist[g]; occupied++; }
        if (occupied < 2) break; // no threshold from this round
        int64_t n = 0, s = 0, n_T = 0, s_T = 0;
        double best = -1.0;
        int T = -1;
        for (int t = lo; t < hi; t++) {
            n += hist[t]; s += (int64_t)t * hist[t];
            if (n > 0 && N - n > 0) {
                const double d = (double)(int64_t)((uint64_t)S * (uint64_t)n - (uint64_t)N * (uint64_t)s); // (two's complement: defined for every input)
                const double v = (d * d) / ((double)n * (double)(N - n));
                if (v > best) { best = v; T = t; n_T = n; s_T = s; }
            }
        }
        const int lo2 = (int)((s_T + n_T - 1) / n_T), hi2 = (int)((S - s_T) / (N - n_T)); // ceil of the lower mean, floor of the upper
        const int repeat = k >= 2 && (T > T_last ? T - T_last : T_last - T) < p->min_delta;
        info->T[k - 1] = T;
        T_last = T; rounds = k;
        if (repeat || k == p->max_iters) { lo = lo2; hi = hi2; break; }
        if (lo2 > hi2) break;
        lo = lo2; hi = hi2;
    }
    info->n_rounds = rounds; info->T_last = T_last;
    info->lo_final = lo; info->hi_final = hi;
    if (rounds == 0) info->flags |= CK_TRI_FLAT;
    for (int g = 0; g < 256; g++) {
        uint8_t c;
        if (rounds == 0) c = g < 128 ? 0 : 1;
        else if (g < lo) c = 0;
        else if (g > hi) c = 1;
        else c = p->keep_tbd ? 2 : (g <= T_last ? 0 : 1);
        lut[g] = c;
        if (c == 0) info->n_black += hist[g];
        else if (c == 1) info->n_white += hist[g];
        else info->n_other += hist[g];
    }
    return CK_OK;
}
