// JPEG preview of the staged frames and its colour form from the raw frames (§4g): what ck_preview.hip (host) and
// k_jpegenc.hip (kernels) share.
#ifndef CK_PREVIEW_H
#define CK_PREVIEW_H

#include "ck_grow.h"
#include "ck_jpeg.h"

#define CK_PV_BLOCK_BYTES 264 /* a baseline block before stuffing: 68 symbols of at most 31 bits */
#define CK_PV_CHUNK 64        /* bytes of the bit buffer one lane of the stuffing passes owns */
#define CK_PV_HDR_MAX 640     /* the three-component header is 623 bytes, 629 with DRI; the grey one 330 / 336 */

// geometry of one call, the same for all its frames
struct ck_pv_geom {
    int W, H, pw, ph;      // frame, preview
    int nc;                // components: 1 (grey) or 3 (Y Cb Cr, 4:4:4: the blocks of an MCU follow each other)
    int bw, bh, nblk;      // MCUs across and down; 8 x 8 blocks of the preview (nc * bw * bh, in scan order)
    int R, nint;           // blocks per restart interval (nblk when there is none; a multiple of nc), intervals per frame
    int overlay;
    int mask_words;        // 32-bit words of a frame's overlay mask: ceil(pw * ph / 32)
    int bit_words;         // 32-bit words of a frame's bit buffer (a multiple of 4)
    int chunk_cap;         // chunks of CK_PV_CHUNK bytes a frame's bit buffer holds at most
    int hdr_len;
};

struct ck_pv_tables {
    uint16_t qdiv[2][64];           // divisor of coefficient k (natural order): 8 * quantisation value; [0] Y, [1] Cb and Cr
    uint8_t hdr[CK_PV_HDR_MAX];     // the file's header, SOI .. SOS
};

// Workspace, allocated by the first preview call and grown on demand (ck_create allocates none of it)
struct ck_preview_ws {
    ck_dev_buf<int32_t> d_frames;    // [n] staged-frame index of every entry
    ck_dev_buf<uint32_t> d_mask;     // [n][mask_words] overlay bit image
    ck_dev_buf<int16_t> d_coef;      // [n][nblk][64] quantised coefficients, zig-zag order
    ck_dev_buf<int16_t> d_dc;        // [n][nblk] quantised DC
    ck_dev_buf<uint32_t> d_len;      // [n][nblk] AC bits of a block, then the block's first bit inside its interval
    ck_dev_buf<uint32_t> d_istart;   // [n][nint + 1] bytes per interval, then the interval's first byte in the frame's bit buffer
    ck_dev_buf<uint32_t> d_bits;     // [n][bit_words] the entropy-coded bits before stuffing, MSB first in every word
    ck_dev_buf<uint32_t> d_cpre;     // [n][chunk_cap] 0xFF bytes in front of every chunk
    ck_dev_buf<int64_t> d_sizes;     // [3][n] file size | offset of the file in the output | status
    ck_dev_buf<uint8_t> d_out;       // compact output staging of a call with a host `out`; ck_preview_luma's pixels
    ck_pinned_buf<int64_t> h_sizes;  // pinned mirror of d_sizes
    ck_pinned_buf<uint8_t> h_out;    // pinned staging of the files
};

// The source of a colour preview (§4g): n_frames raw frames of a packed colour family in device memory, as ck_raw_src lays them
// out, and what turns a pixel's bytes into component c of (Y, Cb, Cr).  Packed 4:2:2 (bpp 2): the one byte at off[c] inside the
// pixel's 2 bytes (c = 0) or its pair's 4 bytes.  Packed colour (bpp 3 / 4): (sum_k wgt[c][k] * byte k + bias[c]) >> 16, libjpeg's
// rgb_ycc_convert.  ovl: the overlay's triple, RGB (0, 255, 0) through the same formulas.
struct ck_pv_csrc {
    const uint8_t *p; int stride; size_t pitch;
    int sw, sh, orientation, bpp;
    int off[3];
    int wgt[3][3], bias[3];
    int ovl[3];
};

// The third source kind (§4i): the frames of a JPEG decode in the colour form.  Y from the oriented luma, Cb and Cr from the
// unoriented planes through the inverse index map and libjpeg's fancy upsampling.  ovl as above.
struct ck_pv_jsrc {
    const uint8_t *luma; int lstride; size_t lpitch;
    const ck_jpeg_desc *descs; const uint32_t *status; const uint8_t *planes;
    int sw, sh, orientation;
    int ovl[3];
};
// The planar 4:2:0 raw formats with CK_RAW_PLANES (§4s): component c of source pixel (u, v) of a frame is the byte at
// off[c] + (v >> rs[c]) * rstride[c] + (u >> cs[c]) * step[c] (ck_raw_planes.h's map at the source's stride, in 32 bits).  ovl as above.
struct ck_pv_psrc {
    const uint8_t *p; size_t pitch;
    int sw, sh, orientation;
    int off[3], rstride[3], step[3], cs[3], rs[3];
    int ovl[3];
};
// the source of a colour call: one of the three
struct ck_pv_src { const ck_pv_csrc *raw; const ck_pv_jsrc *jpeg; const ck_pv_psrc *planar; };
// ... and the storage behind it, whichever it is
struct ck_pv_any { ck_pv_csrc cs; ck_pv_jsrc js; ck_pv_psrc ps; };

// k_jpegenc.hip: the stages, enqueued on the handle's stream, in two halves.  d_out == nullptr: scale .. stuffing scan, after which
// d_sizes holds every file's size, its offset in the output (i * cap for a caller's device buffer, one file behind the other with
// `compact`) and its status.  d_out != nullptr: the files themselves, file i at d_out + offset, never more than cap bytes each.
// cs: the source of a colour call (g.nc = 3), nullptr for the staged luma (g.nc = 1).
int ck_launch_preview_encode(ck_handle *h, const ck_pv_geom &g, const ck_pv_tables &t, const ck_pv_src *cs, int n, uint8_t *d_out,
                             int64_t cap, bool compact);
int ck_launch_preview_mask(ck_handle *h, const ck_pv_geom &g, int n);
int ck_launch_preview_luma(ck_handle *h, const ck_pv_geom &g, int n, uint8_t *d_out);
int ck_launch_preview_color(ck_handle *h, const ck_pv_geom &g, const ck_pv_src &src, int n, uint8_t *d_out); // [n][ph][pw][3]

// ck_preview.hip: the one path of the colour entry points (the ring's are in ck_ingest.hip, where the ring is defined) on n_frames
// raw frames of format *fmt at p, or (jpeg != nullptr, the rest unused) on the frames of a JPEG decode in the colour form.
// files: the JPEG files (ck_preview_jpeg_color*), else the triples (ck_preview_color*).
struct ck_pv_color_src { const uint8_t *p; int stride; int64_t pitch; int n_frames; const ck_raw_format_t *fmt; const ck_jpeg_color_src *jpeg; };
int ck_preview_color_run(ck_handle *h, const ck_preview_params_t *pp, const ck_pv_color_src &src, const int32_t *frames, int32_t n,
                         uint8_t *out, bool files, int64_t cap_per_frame, int64_t *sizes, uint32_t *status);

// the same source as the kernels take it (identity: a packed colour family's own R, G, B instead of its Y Cb Cr: §4r), checked;
// *n_avail: the frames an index may name.  ck_pv_staged_source: the colour source behind the staged frames (CK_EINVAL: none).
int ck_pv_source(ck_handle *h, const ck_pv_color_src &src, bool identity, ck_pv_any *store, ck_pv_src *any, int *n_avail);
int ck_pv_staged_source(ck_handle *h, ck_pv_color_src *src, ck_jpeg_color_src *js);

#endif
