// Iterative tri-class Otsu threshold: what ck_tri_otsu.hip (host) and k_tri_otsu.hip (kernels) share.
#ifndef CK_TRI_OTSU_H
#define CK_TRI_OTSU_H

#include "ck_grow.h"

// Workspace, allocated by the first tri-class call and grown on demand (ck_create allocates none of it)
struct ck_tri_otsu_ws {
    ck_dev_buf<uint32_t> d_hist;           // [n][256] the counters k_tri_hist adds into
    ck_dev_buf<uint8_t> d_lut;             // [n][256] class of every gray level
    ck_dev_buf<ck_tri_otsu_info_t> d_info; // [n] the records
    ck_dev_buf<uint8_t> d_px;              // staging of a caller's host pixels (arrays on the handle's device are used in place)
    ck_dev_buf<uint8_t> d_cls;             // ... and of the classes on their way to a host array
};

extern "C" int ck_tri_otsu_params_ok(const ck_tri_otsu_params_t *p); // ck_tri_otsu_host.c: the one range check

// k_tri_otsu.hip: histogram, solve and look-up of n dense frames of `npix` pixels with p.channels bytes each, on `stream`.
// d_hist is zeroed here; every array is the device's.
int ck_launch_tri_otsu(hipStream_t stream, const ck_tri_otsu_params_t &p, const uint8_t *d_px, int n, size_t npix, uint8_t *d_classes,
                       uint32_t *d_hist, uint8_t *d_lut, ck_tri_otsu_info_t *d_info);

#endif
