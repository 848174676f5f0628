// Baseline JPEG luma decode: what the host parse (ck_jpeg.hip) hands the device kernels (k_jpeg.hip).  DESIGN.md §4c.
#ifndef CK_JPEG_H
#define CK_JPEG_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ck_grow.h"

constexpr int CK_JPEG_SUB_BITS = 512;       // bits of scan one lane decodes speculatively (a subsequence)
constexpr int CK_JPEG_FRAME_THREADS = 1024; // workgroup of k_jpeg_frame (one per frame)

// One subsequence: a piece of at most CK_JPEG_SUB_BITS bits of one restart interval.  A decoder state packs
// (bit position << 16) | (block slot in the MCU << 8) | (zig-zag index: 0 = the DC comes next).
struct ck_jpeg_sub {
    uint32_t start, end;  // bit range in the frame's unstuffed scan: the lane decodes every code that starts in it
    uint32_t interval;    // restart interval it belongs to
    uint32_t first;       // 1: the interval's first piece (its entry state is exact: slot 0, DC)
    uint64_t entry;       // the state the last decode of the piece started from
    uint64_t exit[2];     // the state it ended in (double-buffered across the synchronisation rounds)
    uint32_t nb;          // blocks completed inside the piece (ending inside the interval)
    uint32_t blk0;        // index in the interval of the block in progress at entry
};
static_assert(sizeof(ck_jpeg_sub) == 48, "subsequence record");

// Canonical decode table of one DHT, libjpeg's layout: a 9-bit lookahead for the short codes, maxcode / valoff for the rest.
struct ck_jpeg_huff {
    uint16_t look[512];   // (length << 8) | symbol of the code the 9 bits start with; 0 = a longer code or none
    int32_t maxcode[18];  // largest code of each length 1..16 (-1: none)
    int32_t valoff[18];   // index into vals of the code c of length l = c + valoff[l]
    uint8_t vals[256];
};
static_assert(sizeof(ck_jpeg_huff) % 16 == 0, "tables are copied as 16-byte units");

// One frame of a call.  Offsets are into the call's device buffers.
struct ck_jpeg_desc {
    uint64_t raw_off;      // scan payload (the bytes after the SOS header up to the end of the frame) in the payload area; its
                           // unstuffed copy lands at the same offset in d_compact.  16-byte aligned
    uint64_t int_off;      // first entry of the frame's interval starts in d_int ([nint + 1] byte offsets in the compact stream)
    uint64_t sub_off;      // first record of the frame's subsequences in d_sub
    uint32_t raw_len;      // payload bytes (its region is raw_len + 4 rounded up to 16)
    uint32_t status;       // CK_JPEG_* bits found by the host (non-zero: the frame is staged as zeros)
    uint32_t sub_cap;      // subsequence records the frame may use
    uint32_t nint;         // restart intervals (1 without DRI)
    uint32_t restart;      // MCUs per interval (= nmcu without DRI)
    uint32_t nmcu;         // MCUs of the scan
    uint32_t mcux;         // MCUs per row
    uint32_t bpm;          // blocks per MCU
    uint32_t nyb;          // Y blocks per MCU (1 for grey)
    uint32_t hs;           // Y blocks per MCU along x
    uint32_t yblk_stride;  // Y blocks per row of the frame (mcux * hs)
    uint32_t yblk_rows;    // Y block rows of the frame
    uint32_t qt;           // index of Y's quantisation table in the quant area
    uint16_t dc[3], ac[3]; // indices of the scan components' tables in the table area (unused entries 0)
    // the colour form (ck_upload_jpeg_color, ck_ingest_create_jpeg_color); unused and 0 otherwise
    uint32_t qtc[2];       // indices of Cb's and Cr's quantisation tables
    uint32_t pad;
    uint64_t plane_off;    // the frame's chroma planes in d_planes: Cb [ch][cw], then Cr, cw x ch = ceil(sw / hs) x ceil(sh / vs).  16-byte aligned
};

// Device workspace of a JPEG decode in flight: the handle's (ck_handle::jpeg, grown on demand) and one per slot of a JPEG ingest
// ring (sized once by ck_ingest_create_jpeg), ck_jpeg.hip.
struct ck_jpeg_ws {
    ck_pinned_buf<uint8_t> h_stage;  // pinned host staging: descriptors | Huffman tables | quant tables | payloads
    ck_dev_buf<uint8_t> d_in;        // its device copy
    ck_dev_buf<uint8_t> d_compact;   // unstuffed scans, at the payloads' offsets
    ck_dev_buf<uint32_t> d_int;      // interval starts
    ck_dev_buf<ck_jpeg_sub> d_sub;   // subsequence records
    ck_dev_buf<int16_t> d_coef;      // Y coefficients [frame][block][64], natural order; the colour form: Y | Cb | Cr, nmcu * (nyb + 2) blocks
    ck_dev_buf<uint8_t> d_planes;    // the colour form: the unoriented chroma planes of every frame, at ck_jpeg_desc::plane_off
    ck_dev_buf<uint32_t> d_status;   // [max_batch] final per-frame status
    ck_pinned_buf<uint32_t> h_status; // pinned [max_batch]
};

// k_jpeg.hip: the per-frame decode and the IDCT of n described frames on stream s, with workspace J, into the frames `dst`
// (statuses in J.d_status).  The streams are sw x sh; dst holds them turned by `orientation` (CK_ORIENT_*).
int ck_launch_jpeg(const ck_jpeg_ws &J, hipStream_t s, int n, const ck_jpeg_desc *d_desc, const ck_jpeg_huff *d_huff, const int32_t *d_qt,
                   const uint8_t *d_raw, size_t coef_frame_blocks, const ck_dev_image &dst, int sw, int sh, int orientation, bool color);

// What the colour preview reads of a decode in the colour form (k_jpegenc.hip: the third source kind): the oriented luma `img` of
// n_frames frames, their descriptors and statuses and the chroma planes, all on the device, for sw x sh streams turned by `orientation`
struct ck_jpeg_color_src {
    ck_dev_image img;
    const ck_jpeg_desc *descs;
    const uint32_t *status;
    const uint8_t *planes;
    int n_frames, sw, sh, orientation;
};
// the handle's, while the frames of the last ck_upload_jpeg_color still are its staged frames (CK_EINVAL otherwise)
int ck_jpeg_color_source(ck_handle *h, ck_jpeg_color_src *out);

// The JPEG half of an ingest ring (ck_ingest_create_jpeg; ck_jpeg.hip): per slot one workspace sized once for max_batch frames of
// at most max_frame_bytes, the parsed headers of the frames written since the slot's last submit, and which indices they are.
struct ck_jpeg_slots;
// color: the slots also keep their frames' chroma planes (ck_ingest_create_jpeg_color)
int ck_jpeg_slots_create(ck_handle *h, int n_slots, int orientation, int64_t max_frame_bytes, bool color, ck_jpeg_slots **out);
void ck_jpeg_slots_free(ck_jpeg_slots *q);
// parse + copy of the scan into the slot's pinned staging (the caller has made sure no earlier submit still reads it)
int ck_jpeg_slots_write(ck_jpeg_slots *q, int slot, int index, const uint8_t *data, int64_t size);
// descriptors + merged tables of frames [0, n), then copy, decode, IDCT and the status copy enqueued on s; no synchronisation
int ck_jpeg_slots_submit(ck_jpeg_slots *q, int slot, int n, hipStream_t s, const ck_dev_image &dst);
// the colour source of a slot whose luma frames are `img` (n_frames of them); false: not a colour ring
bool ck_jpeg_slots_color_source(const ck_jpeg_slots *q, int slot, const ck_dev_image &img, int n_frames, ck_jpeg_color_src *out);
const uint32_t *ck_jpeg_slots_status(const ck_jpeg_slots *q, int slot); // pinned [max_batch]: valid once the submit's work is done

#endif
