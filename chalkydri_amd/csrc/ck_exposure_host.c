// Exposure metering, the host half that needs no device: parameter checks, the gamma tables the kernel is handed,
// the gradient-information metric of a frame's histograms and the exposure recommended from it.  Plain double arithmetic, libm
// pow / log / exp, evaluated exactly as written (tests/np_exposure.py restates it).
#include "chalkydri_hip.h"
#include <math.h>
#include <string.h>

void ck_exposure_params_default(ck_exposure_params_t *p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    const double g[CK_EXPOSURE_GAMMAS] = {1.0 / 1.9, 1.0 / 1.5, 1.0 / 1.2, 1.0, 1.2, 1.5, 1.9};
    memcpy(p->gamma, g, sizeof g);
    p->lambda = 1000.0; p->delta = 0.06;
    p->kp = 1.0;
    p->e_min = 1e-6; p->e_max = 1e6;
}

static int positive(double v) { return isfinite(v) && v > 0.0; }

static int params_ok(const ck_exposure_params_t *p) {
    if (!p) return 0;
    for (int k = 0; k < CK_EXPOSURE_GAMMAS; k++) {
        if (!positive(p->gamma[k])) return 0;
        if (k && !(p->gamma[k] > p->gamma[k - 1])) return 0;
    }
    if (!positive(p->lambda) || !positive(p->kp) || !positive(p->e_min) || !positive(p->e_max)) return 0;
    if (!isfinite(p->delta) || p->delta < 0.0 || p->delta >= 1.0) return 0;
    return p->e_min <= p->e_max;
}

int ck_exposure_luts(const ck_exposure_params_t *p, uint8_t *lut) {
    if (!params_ok(p) || !lut) return CK_EINVAL;
    for (int k = 0; k < CK_EXPOSURE_GAMMAS; k++) {
        uint8_t *t = lut + 256 * k;
        for (int v = 0; v < 256; v++) {
            if (p->gamma[k] == 1.0 || v == 0 || v == 255) { t[v] = (uint8_t)v; continue; }
            double r = floor(255.0 * pow((double)v / 255.0, p->gamma[k]) + 0.5);
            t[v] = (uint8_t)(r < 0.0 ? 0.0 : (r > 255.0 ? 255.0 : r));
        }
    }
    return CK_OK;
}

int ck_exposure_metric(const ck_exposure_params_t *p, const ck_exposure_stats_t *s, double *m) {
    if (!params_ok(p) || !s || !m) return CK_EINVAL;
    double W[CK_EXPOSURE_BINS];
    const double norm = log(p->lambda * (1.0 - p->delta) + 1.0);
    for (int b = 0; b < CK_EXPOSURE_BINS; b++) {
        const double x = (double)b / 180.0;
        W[b] = x >= p->delta ? log(p->lambda * (x - p->delta) + 1.0) / norm : 0.0;
    }
    for (int k = 0; k < CK_EXPOSURE_GAMMAS; k++) {
        double acc = 0.0;
        for (int b = 0; b < CK_EXPOSURE_BINS; b++) acc += (double)s->grad[k][b] * W[b];
        m[k] = s->n_grad ? acc / (double)s->n_grad : 0.0;
    }
    return CK_OK;
}

int ck_exposure_recommend(const ck_exposure_params_t *p, const ck_exposure_stats_t *s, double exposure, double *next, double *gamma_hat) {
    double m[CK_EXPOSURE_GAMMAS];
    if (!next || !positive(exposure)) return CK_EINVAL;
    const int rc = ck_exposure_metric(p, s, m);
    if (rc != CK_OK) return rc;
    int best = 0, flat = 1;
    for (int k = 1; k < CK_EXPOSURE_GAMMAS; k++) {
        if (m[k] > m[best]) best = k;
        if (m[k] != m[0]) flat = 0;
    }
    double g = p->gamma[best];
    if (flat) g = 1.0;
    else if (best > 0 && best < CK_EXPOSURE_GAMMAS - 1) {
        const double x0 = log(p->gamma[best - 1]), x1 = log(p->gamma[best]), x2 = log(p->gamma[best + 1]);
        const double y0 = m[best - 1], y1 = m[best], y2 = m[best + 1];
        const double d1 = (y1 - y0) / (x1 - x0), d2 = (y2 - y1) / (x2 - x1);
        const double dd = (d2 - d1) / (x2 - x0); // second divided difference: the parabola's leading coefficient
        if (dd != 0.0) {
            const double xv = 0.5 * (x0 + x1) - d1 / (2.0 * dd);
            g = exp(xv);
            if (!(g >= p->gamma[best - 1])) g = p->gamma[best - 1];
            if (g > p->gamma[best + 1]) g = p->gamma[best + 1];
        }
    }
    double e = exposure * pow(g, -p->kp);
    if (!(e >= p->e_min)) e = p->e_min;
    if (e > p->e_max) e = p->e_max;
    *next = e;
    if (gamma_hat) *gamma_hat = g;
    return CK_OK;
}
