// JPEG preview of the staged frames: what ck_preview.hip (host) and k_jpegenc.hip (kernels) share.
#ifndef CK_PREVIEW_H
#define CK_PREVIEW_H

#include "ck_internal.h"

#define CK_PV_BLOCK_BYTES 264 /* a baseline block before stuffing: 68 symbols of at most 31 bits */
#define CK_PV_CHUNK 64        /* bytes of the bit buffer one lane of the stuffing passes owns */
#define CK_PV_HDR_MAX 336

// geometry of one call, the same for all its frames
struct ck_pv_geom {
    int W, H, pw, ph;      // frame, preview
    int bw, bh, nblk;      // 8 x 8 blocks of the preview
    int R, nint;           // blocks per restart interval (nblk when there is none), intervals per frame
    int overlay;
    int mask_words;        // 32-bit words of a frame's overlay mask: ceil(pw * ph / 32)
    int bit_words;         // 32-bit words of a frame's bit buffer (a multiple of 4)
    int chunk_cap;         // chunks of CK_PV_CHUNK bytes a frame's bit buffer holds at most
    int hdr_len;
};

struct ck_pv_tables {
    uint16_t qdiv[64];              // divisor of coefficient k (natural order): 8 * quantisation value
    uint8_t hdr[CK_PV_HDR_MAX];     // the file's header, SOI .. SOS
};

// Workspace, allocated by the first preview call and grown on demand (ck_create allocates none of it)
struct ck_preview_ws {
    int32_t *d_frames; size_t frames_cap;   // [n] staged-frame index of every entry
    uint32_t *d_mask; size_t mask_cap;      // [n][mask_words] overlay bit image
    int16_t *d_coef; size_t coef_cap;       // [n][nblk][64] quantised coefficients, zig-zag order
    int16_t *d_dc; size_t dc_cap;           // [n][nblk] quantised DC
    uint32_t *d_len; size_t len_cap;        // [n][nblk] AC bits of a block, then the block's first bit inside its interval
    uint32_t *d_istart; size_t istart_cap;  // [n][nint + 1] bytes per interval, then the interval's first byte in the frame's bit buffer
    uint32_t *d_bits; size_t bits_cap;      // [n][bit_words] the entropy-coded bits before stuffing, MSB first in every word
    uint32_t *d_cpre; size_t cpre_cap;      // [n][chunk_cap] 0xFF bytes in front of every chunk
    int64_t *d_sizes; size_t sizes_cap;     // [3][n] file size | offset of the file in the output | status
    uint8_t *d_out; size_t out_cap;         // compact output staging of a call with a host `out`; ck_preview_luma's pixels
    int64_t *h_sizes; size_t h_sizes_cap;   // pinned mirror of d_sizes
    uint8_t *h_out; size_t h_out_cap;       // pinned staging of the files
};

// k_jpegenc.hip: the stages, enqueued on the handle's stream, in two halves.  d_out == nullptr: scale .. stuffing scan, after which
// d_sizes holds every file's size, its offset in the output (i * cap for a caller's device buffer, one file behind the other with
// `compact`) and its status.  d_out != nullptr: the files themselves, file i at d_out + offset, never more than cap bytes each.
int ck_launch_preview_encode(ck_handle *h, const ck_pv_geom &g, const ck_pv_tables &t, int n, uint8_t *d_out, int64_t cap, bool compact);
int ck_launch_preview_mask(ck_handle *h, const ck_pv_geom &g, int n);
int ck_launch_preview_luma(ck_handle *h, const ck_pv_geom &g, int n, uint8_t *d_out);
void ck_preview_free(ck_handle *h);

#endif
