// ck_raw_planes.h — the plane map of the planar 4:2:0 raw formats (NV12, NV21, I420, YV12 with CK_RAW_PLANES: DESIGN.md §4s), written
// once and compiled into everything that places a sample of such a frame: ck_raw_plane_layout and ck_raw_ycc_host, the host copy
// loops of ck_upload_raw and ck_ingest_write, the source the kernels read through (ck_pv_source.h: Planar) and the stand-alone
// check (tests/cpp/raw_planes_check.cpp).  Pure C, integers only, as ck_blob_math.h and ck_camera_math.h are.
//
// The layout is V4L2's single-buffer one.  With cw = ceil(sw / 2), ch = ceil(sh / 2) and a row stride `stride` >= 2 cw: sh luma rows
// of `stride` bytes; then NV12 / NV21: ch rows of `stride` bytes, pair i of a row at bytes 2i, 2i + 1, (Cb, Cr) / (Cr, Cb); I420 /
// YV12 (stride even): ch rows of stride / 2 bytes of Cb / Cr, then as many of Cr / Cb.  A frame extends stride * (sh + ch) bytes.
// The triple of source pixel (u, v) is (Y[v][u], Cb[v >> 1][u >> 1], Cr[v >> 1][u >> 1]): the bytes unchanged, chroma replicated.
#ifndef CK_RAW_PLANES_H
#define CK_RAW_PLANES_H

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define CKRP_FN static __device__ __host__ __forceinline__
#else
#define CKRP_FN static inline
#endif

// the four layouts (ck_raw_class::k[0] of a format with CK_RAW_PLANES; 0 = no chroma planes)
enum { CKP_NONE = 0, CKP_NV12 = 1, CKP_NV21 = 2, CKP_I420 = 3, CKP_YV12 = 4 };

// component c (0 Y, 1 Cb, 2 Cr) of source pixel (u, v) is the byte at off + (v >> rs) * row_stride + (u >> cs) * step of the frame
typedef struct ckp_plane { int64_t off; int32_t row_stride, step, cs, rs; } ckp_plane;
typedef struct ckp_map {
    ckp_plane c[3];
    int32_t sw, sh, cw, ch;
    int64_t bytes; // stride * (sh + ch): what a frame extends
} ckp_map;

CKRP_FN int32_t ckp_min_stride(int32_t sw) { return 2 * ((sw + 1) / 2); }

// 0, or -1 for a stride the layout cannot have (below 2 cw; odd with two half-stride planes)
CKRP_FN int ckp_map_make(int kind, int32_t sw, int32_t sh, int32_t stride, ckp_map *m) {
    const int32_t cw = (sw + 1) / 2, ch = (sh + 1) / 2;
    const int split = kind == CKP_I420 || kind == CKP_YV12;
    if (stride < 2 * cw || (split && (stride & 1))) return -1;
    const int64_t base = (int64_t)stride * sh;
    m->sw = sw; m->sh = sh; m->cw = cw; m->ch = ch;
    m->bytes = (int64_t)stride * (sh + ch);
    m->c[0].off = 0; m->c[0].row_stride = stride; m->c[0].step = 1; m->c[0].cs = 0; m->c[0].rs = 0;
    for (int c = 1; c < 3; c++) {
        // the component that comes first in memory: Cb of NV12 and I420, Cr of NV21 and YV12
        const int first = (c == 1) == (kind == CKP_NV12 || kind == CKP_I420);
        m->c[c].cs = 1; m->c[c].rs = 1;
        if (split) {
            m->c[c].row_stride = stride / 2; m->c[c].step = 1;
            m->c[c].off = base + (first ? 0 : (int64_t)(stride / 2) * ch);
        } else {
            m->c[c].row_stride = stride; m->c[c].step = 2;
            m->c[c].off = base + (first ? 0 : 1);
        }
    }
    return 0;
}

CKRP_FN int64_t ckp_at(const ckp_map *m, int c, int32_t u, int32_t v) {
    const ckp_plane *p = &m->c[c];
    return p->off + (int64_t)(v >> p->rs) * p->row_stride + (int64_t)(u >> p->cs) * p->step;
}

// one past the last byte of a frame that holds a sample: what a reader may touch, and what a copy has to bring
CKRP_FN int64_t ckp_extent(const ckp_map *m) {
    int64_t e = 0;
    for (int c = 0; c < 3; c++) {
        const int64_t a = ckp_at(m, c, m->sw - 1, m->sh - 1) + 1;
        if (a > e) e = a;
    }
    return e;
}

// the source pixel (u, v) behind pixel (ox, oy) of the frame turned by `turn` (CK_ORIENT_* 0..3): the index maps of §4d
CKRP_FN void ckp_source_xy(int turn, int32_t sw, int32_t sh, int32_t ox, int32_t oy, int32_t *u, int32_t *v) {
    switch (turn) {
    case 1: *u = oy; *v = sh - 1 - ox; return;          // clockwise: S[sh-1-ox][oy]
    case 2: *u = sw - 1 - ox; *v = sh - 1 - oy; return; // rotate-180: S[sh-1-oy][sw-1-ox]
    case 3: *u = sw - 1 - oy; *v = ox; return;          // counterclockwise: S[ox][sw-1-oy]
    }
    *u = ox; *v = oy;
}

CKRP_FN void ckp_triple(const ckp_map *m, const uint8_t *frame, int32_t u, int32_t v, uint8_t *ycc) {
    for (int c = 0; c < 3; c++) ycc[c] = frame[ckp_at(m, c, u, v)];
}


// A frame of row stride sstride into one of row stride dstride (both valid for the layout): equal strides are one copy of the
// frame's extent; otherwise every plane row moves the bytes it holds (sw of luma, 2 cw of an interleaved chroma row, cw of a split
// one) and nothing of the rows' padding.  Reads nothing at or beyond sstride * (sh + ch), writes nothing at or beyond dstride * (sh + ch).
static inline void ckp_copy(int kind, int32_t sw, int32_t sh, const uint8_t *src, int32_t sstride, uint8_t *dst, int32_t dstride) {
    ckp_map s, d;
    if (ckp_map_make(kind, sw, sh, sstride, &s) != 0 || ckp_map_make(kind, sw, sh, dstride, &d) != 0) return;
    if (sstride == dstride) { memcpy(dst, src, (size_t)ckp_extent(&s)); return; }
    for (int32_t y = 0; y < sh; y++) memcpy(dst + (size_t)y * dstride, src + (size_t)y * sstride, (size_t)sw);
    if (s.c[1].step == 2) { // one interleaved plane: the lower of the two offsets is the row's first byte
        const int64_t so = s.c[1].off < s.c[2].off ? s.c[1].off : s.c[2].off, dn = d.c[1].off < d.c[2].off ? d.c[1].off : d.c[2].off;
        for (int32_t y = 0; y < s.ch; y++) memcpy(dst + dn + (size_t)y * dstride, src + so + (size_t)y * sstride, (size_t)(2 * s.cw));
        return;
    }
    for (int c = 1; c < 3; c++)
        for (int32_t y = 0; y < s.ch; y++)
            memcpy(dst + d.c[c].off + (size_t)y * d.c[c].row_stride, src + s.c[c].off + (size_t)y * s.c[c].row_stride, (size_t)s.cw);
}

#endif
