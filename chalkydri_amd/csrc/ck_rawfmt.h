// Raw camera formats -> oriented luma: what the host half (ck_rawfmt.hip, ck_ingest.hip) hands k_rawfmt.hip.
#ifndef CK_RAWFMT_H
#define CK_RAWFMT_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ck_grow.h"

// 16-bit fixed-point weights of L(R,G,B) (libjpeg's jccolor.c grey conversion); they sum to 65536
#define CK_LUMA_R 19595u
#define CK_LUMA_G 38470u
#define CK_LUMA_B 7471u

// A fourcc as the kernel sees it: bytes per pixel + where the luma comes from.  Two fourccs with equal classes are one family.
struct ck_raw_class {
    int bpp;         // 1: a leading luma plane, 2: packed 4:2:2, 3 / 4: packed colour
    uint32_t k[3];   // bpp 3 / 4: weight of byte 0, 1, 2 of a pixel.  bpp 2: v_perm_b32 selector that picks the four luma bytes of
                     // two dwords in order, the one that picks them reversed, the luma's byte offset in a pixel.  bpp 1: k[0] = the
                     // layout of the chroma planes behind the luma (CKP_*, ck_raw_planes.h) of a format with CK_RAW_PLANES, else 0
};
static inline bool ck_raw_same_family(const ck_raw_class &a, const ck_raw_class &b) {
    return a.bpp == b.bpp && a.k[0] == b.k[0] && a.k[1] == b.k[1] && a.k[2] == b.k[2];
}
// CK_OK / CK_EUNSUPPORTED (a fourcc outside the table of §4d).  k[0] of NV12 / NV21 / I420 / YV12 names the layout: ck_raw_geometry
// keeps it for a format with CK_RAW_PLANES and clears it otherwise (without the flag the luma-first fourccs are one family).
int ck_raw_classify(uint32_t fourcc, ck_raw_class *out);

// The source of an oriented w x h frame of format `fmt`: its class, its size, the bytes a row holds at least, and the layout every
// staging of such frames uses (the host entry points' and a raw ingest ring's): rows at the minimum stride rounded up to 16.
// CK_EINVAL (null fmt, w or h < 1, orientation out of range) / CK_EUNSUPPORTED (fourcc; CK_RAW_PLANES with a fourcc that has no
// chroma planes), in ck_raw_layout's order.  This is the one place that splits ck_raw_format_t::orientation into the turn
// (CK_ORIENT_*: what kernels and switches take) and the flag: planes = the layout (CKP_*), 0 without the flag; ch = the chroma
// rows behind the sh luma rows of a frame (0 without the flag), which pitch16 counts.
struct ck_raw_geom { ck_raw_class cls; int sw, sh, min_stride, stride16; size_t pitch16; int turn, planes, ch; };
int ck_raw_geometry(const ck_raw_format_t *fmt, int w, int h, ck_raw_geom *out);
// a caller's row stride and frame pitch against the geometry: at least the minimum, even where two half-stride planes follow,
// and a frame of stride * (sh + ch) bytes inside the pitch (planes 3 and 4: CKP_I420 and CKP_YV12 of ck_raw_planes.h)
static inline bool ck_raw_stride_ok(const ck_raw_geom &L, int64_t stride) {
    return stride >= L.min_stride && !((L.planes == 3 || L.planes == 4) && (stride & 1));
}
static inline bool ck_raw_pitch_ok(const ck_raw_geom &L, int64_t stride, int64_t pitch) {
    return ck_raw_stride_ok(L, stride) && pitch >= stride * (L.sh + L.ch);
}

// The source side of one conversion: n frames of sw x sh pixels in device memory, row y of frame f at p + f * pitch + y * stride
struct ck_raw_src { const uint8_t *p; int stride; size_t pitch; int sw, sh; };

struct ck_handle;
// k_rawfmt.hip: converts + orients n frames into dst (the handle's staged layout: rows of h->frame_stride, frames of h->frame_pitch)
int ck_launch_rawfmt(ck_handle *h, hipStream_t st, const ck_raw_src &src, const ck_raw_class &cls, int orientation, uint8_t *dst, int n);

// Staging of the host-frame entry points (ck_handle::raw): allocated by the first raw call, grown on demand (ck_rawfmt.hip)
struct ck_raw_ws {
    ck_pinned_buf<uint8_t> h_stage; // pinned host: [n][sh][stride16] raw rows
    ck_dev_buf<uint8_t> d_stage;    // its device copy; it ends with the last row's last byte the kernel may read
};

#endif
