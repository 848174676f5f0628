// The device side of a colour source: what k_jpegenc.hip (the colour preview) and k_blobs.hip (the coloured-piece
// detector, §4r) both read the ORIENTED pixels of a raw or a decoded frame through.  One copy of the orientation maps.
#ifndef CK_PV_SOURCE_H
#define CK_PV_SOURCE_H

#include "ck_preview.h"

namespace {

// ---- colour (§4g): component `comp` of pixel (ox, oy) of the ORIENTED frame, from the raw source --------------------------------
// The address of a pixel's bytes separates into a term of ox and a term of oy under all four index maps of §4d (none: S[oy][ox],
// clockwise: S[sh-1-ox][oy], rotate-180: S[sh-1-oy][sw-1-ox], counterclockwise: S[ox][sw-1-oy]), so a block computes eight of each.
// Every read lies inside [row, row + min_stride) of a source row 0 .. sh-1: ox < W and oy < H bound the row and the pixel, and the
// pair of a 4:2:2 pixel u ends at byte 4 (u >> 1) + 3 < 4 ceil(sw / 2).
struct CLane { int comp, off, w0, w1, w2, bias, ovl; }; // a lane's component and its constants out of ck_pv_csrc
__device__ __forceinline__ CLane clane(const ck_pv_csrc &s, int comp) {
    const auto pick = [&](int a, int b, int c) { return comp == 0 ? a : (comp == 1 ? b : c); };
    return {comp, pick(s.off[0], s.off[1], s.off[2]), pick(s.wgt[0][0], s.wgt[1][0], s.wgt[2][0]), pick(s.wgt[0][1], s.wgt[1][1], s.wgt[2][1]),
            pick(s.wgt[0][2], s.wgt[1][2], s.wgt[2][2]), pick(s.bias[0], s.bias[1], s.bias[2]), pick(s.ovl[0], s.ovl[1], s.ovl[2])};
}
template <bool YUV>
__device__ __forceinline__ int c_pixel_off(const ck_pv_csrc &s, const CLane &L, int u) { // pixel u of a source row
    if (YUV) return (L.comp ? (u >> 1) << 2 : u << 1) + L.off;
    return u * s.bpp;
}
template <bool YUV>
__device__ __forceinline__ int c_term_x(const ck_pv_csrc &s, const CLane &L, int ox) {
    switch (s.orientation) {
    case CK_ORIENT_CLOCKWISE: return (s.sh - 1 - ox) * s.stride;
    case CK_ORIENT_COUNTERCLOCKWISE: return ox * s.stride;
    case CK_ORIENT_ROTATE_180: return c_pixel_off<YUV>(s, L, s.sw - 1 - ox);
    }
    return c_pixel_off<YUV>(s, L, ox);
}
template <bool YUV>
__device__ __forceinline__ int c_term_y(const ck_pv_csrc &s, const CLane &L, int oy) {
    switch (s.orientation) {
    case CK_ORIENT_CLOCKWISE: return c_pixel_off<YUV>(s, L, oy);
    case CK_ORIENT_COUNTERCLOCKWISE: return c_pixel_off<YUV>(s, L, s.sw - 1 - oy);
    case CK_ORIENT_ROTATE_180: return (s.sh - 1 - oy) * s.stride;
    }
    return oy * s.stride;
}
// the component at byte offset `at` of the frame `p`; then the overlay (bit = the preview pixel's index in the mask)
template <bool YUV>
__device__ __forceinline__ int c_pixel(const uint8_t *p, int at, const CLane &L, const uint32_t *mask, int bit) {
    int v = YUV ? (int)p[at] : (L.w0 * (int)p[at] + L.w1 * (int)p[at + 1] + L.w2 * (int)p[at + 2] + L.bias) >> 16;
    if (mask && ((mask[bit >> 5] >> (bit & 31)) & 1u)) v = L.ovl;
    return v;
}

// The source kinds of the colour front end (pv_triples, pv_fdct_color below: one body, one kernel per kind).  A kind gives a lane its constants (lane), the two terms of a pixel's place (term_x of
// the oriented column, term_y of the oriented row; their sum is the place), a frame (frame) and the lane's component of the pixel at
// a place of a frame, overlaid (pixel).  Raw<YUV>: the packed 4:2:2 and packed colour families above, the place a byte offset.
template <bool YUV>
struct Raw {
    ck_pv_csrc s;
    using Lane = CLane;
    using Frame = const uint8_t *;
    __device__ __forceinline__ Lane lane(int comp) const { return clane(s, comp); }
    __device__ __forceinline__ int term_x(const Lane &L, int ox) const { return c_term_x<YUV>(s, L, ox); }
    __device__ __forceinline__ int term_y(const Lane &L, int oy) const { return c_term_y<YUV>(s, L, oy); }
    __device__ __forceinline__ Frame frame(int f) const { return s.p + (size_t)f * s.pitch; }
    __device__ __forceinline__ int pixel(Frame p, int at, const Lane &L, const uint32_t *mask, int bit) const { return c_pixel<YUV>(p, at, L, mask, bit); }
};

// Decoded: the frames of a JPEG decode in the colour form (§4i).  The place is a pair of coordinates x | y << 16: for Y those of the
// ORIENTED pixel in the staged (or the slot's) luma, for Cb and Cr those of the SOURCE pixel the index maps of §4d name, whose value
// is libjpeg's fancy upsampling of the component's cw x ch plane: at most two rows j, jn and two columns i, in of it, each inside
// [0, ch) and [0, cw) because 0 <= x < sw <= hs cw and 0 <= y < sh <= vs ch and the neighbours are clamped.
struct Decoded {
    ck_pv_jsrc s;
    struct Lane { int comp, ovl; };
    struct Frame { const uint8_t *luma, *plane; int cw, ch, h2, v2; }; // plane == nullptr: grey or failed, Cb = Cr = 128
    __device__ __forceinline__ Lane lane(int comp) const { return {comp, comp == 0 ? s.ovl[0] : (comp == 1 ? s.ovl[1] : s.ovl[2])}; }
    __device__ __forceinline__ int term_x(const Lane &L, int ox) const {
        if (L.comp == 0) return ox;
        switch (s.orientation) {
        case CK_ORIENT_CLOCKWISE: return (s.sh - 1 - ox) << 16;
        case CK_ORIENT_COUNTERCLOCKWISE: return ox << 16;
        case CK_ORIENT_ROTATE_180: return s.sw - 1 - ox;
        }
        return ox;
    }
    __device__ __forceinline__ int term_y(const Lane &L, int oy) const {
        if (L.comp == 0) return oy << 16;
        switch (s.orientation) {
        case CK_ORIENT_CLOCKWISE: return oy;
        case CK_ORIENT_COUNTERCLOCKWISE: return s.sw - 1 - oy;
        case CK_ORIENT_ROTATE_180: return (s.sh - 1 - oy) << 16;
        }
        return oy << 16;
    }
    __device__ __forceinline__ Frame frame(int f) const {
        const ck_jpeg_desc &d = s.descs[f];
        Frame F = {s.luma + (size_t)f * s.lpitch, nullptr, 0, 0, 0, 0};
        if (s.status[f] == 0 && d.bpm > 1) {
            const int hs = (int)d.hs, vs = (int)(d.nyb / d.hs);
            F.cw = (s.sw + hs - 1) / hs; F.ch = (s.sh + vs - 1) / vs; F.h2 = hs == 2; F.v2 = vs == 2;
            F.plane = s.planes + d.plane_off;
        }
        return F;
    }
    __device__ __forceinline__ int pixel(const Frame &F, int at, const Lane &L, const uint32_t *mask, int bit) const {
        const int x = at & 0xFFFF, y = at >> 16;
        int v;
        if (L.comp == 0) {
            v = F.luma[(size_t)y * s.lstride + x];
        } else if (!F.plane) {
            v = 128;
        } else {
            const uint8_t *P = F.plane + (L.comp == 2 ? (size_t)F.cw * F.ch : 0);
            const int i = F.h2 ? x >> 1 : x, j = F.v2 ? y >> 1 : y;
            const uint8_t *r0 = P + (size_t)j * F.cw;
            if (!F.h2 && !F.v2) {
                v = r0[i];
            } else {
                const int in = (x & 1) ? min(i + 1, F.cw - 1) : max(i - 1, 0), jn = (y & 1) ? min(j + 1, F.ch - 1) : max(j - 1, 0);
                const uint8_t *r1 = P + (size_t)jn * F.cw;
                if (!F.v2) v = (3 * r0[i] + r0[in] + ((x & 1) ? 2 : 1)) >> 2;
                else if (!F.h2) v = (3 * r0[i] + r1[i] + ((y & 1) ? 2 : 1)) >> 2;
                else v = (3 * (3 * r0[i] + r1[i]) + 3 * r0[in] + r1[in] + ((x & 1) ? 7 : 8)) >> 4;
            }
        }
        if (mask && ((mask[bit >> 5] >> (bit & 31)) & 1u)) v = L.ovl;
        return v;
    }
};

// Planar: the 4:2:0 raw formats with CK_RAW_PLANES (§4s).  The place is a byte offset into the frame, as Raw's is: component c of
// source pixel (u, v) lies at off + (v >> rs) * rstride + (u >> cs) * step, a term of u plus a term of v, so under all four index
// maps it is a term of the oriented column plus a term of the oriented row (the plane's offset rides on the row's).  Lanes differ
// in these five constants, never in control flow.  Every read lies inside the plane's own rows: u < sw and v < sh bound
// (u >> cs) * step + step - 1 by the bytes a row of the plane holds and v >> rs by its rows (ck_raw_planes.h).
struct Planar {
    ck_pv_psrc s;
    struct Lane { int comp, off, rstride, step, cs, rs, ovl; };
    using Frame = const uint8_t *;
    __device__ __forceinline__ Lane lane(int comp) const {
        const auto pick = [&](const int (&a)[3]) { return comp == 0 ? a[0] : (comp == 1 ? a[1] : a[2]); };
        return {comp, pick(s.off), pick(s.rstride), pick(s.step), pick(s.cs), pick(s.rs), pick(s.ovl)};
    }
    __device__ __forceinline__ int col(const Lane &L, int u) const { return (u >> L.cs) * L.step; }
    __device__ __forceinline__ int row(const Lane &L, int v) const { return (v >> L.rs) * L.rstride; }
    __device__ __forceinline__ int term_x(const Lane &L, int ox) const {
        switch (s.orientation) {
        case CK_ORIENT_CLOCKWISE: return row(L, s.sh - 1 - ox);
        case CK_ORIENT_COUNTERCLOCKWISE: return row(L, ox);
        case CK_ORIENT_ROTATE_180: return col(L, s.sw - 1 - ox);
        }
        return col(L, ox);
    }
    __device__ __forceinline__ int term_y(const Lane &L, int oy) const {
        switch (s.orientation) {
        case CK_ORIENT_CLOCKWISE: return L.off + col(L, oy);
        case CK_ORIENT_COUNTERCLOCKWISE: return L.off + col(L, s.sw - 1 - oy);
        case CK_ORIENT_ROTATE_180: return L.off + row(L, s.sh - 1 - oy);
        }
        return L.off + row(L, oy);
    }
    __device__ __forceinline__ Frame frame(int f) const { return s.p + (size_t)f * s.pitch; }
    __device__ __forceinline__ int pixel(Frame p, int at, const Lane &L, const uint32_t *mask, int bit) const {
        int v = p[at];
        if (mask && ((mask[bit >> 5] >> (bit & 31)) & 1u)) v = L.ovl;
        return v;
    }
};

} // namespace

#endif
