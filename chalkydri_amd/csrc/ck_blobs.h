// Coloured game pieces: what ck_blobs.hip (host) and k_blobs.hip (kernels) share.
#ifndef CK_BLOBS_H
#define CK_BLOBS_H

#include "ck_grow.h"
#include "ck_preview.h"
#include "ck_blob_math.h" // (after the runtime's header: its functions are __device__ here)

// geometry of one call, the same for all its frames
struct ck_blob_geom {
    int W, H;
    int ww;     // 32-bit words of a row of a plane: ceil(W / 32)
    int nc;     // classes
    int maxc;   // component slots per plane
    int cap;    // records per plane in the output
};

// Workspace, allocated by the first blob call and grown on demand (ck_create allocates none of it).  A plane = one class of one frame.
struct ck_blob_ws {
    ck_dev_buf<int32_t> d_frames;    // [n] source-frame index of every entry
    ck_dev_buf<uint8_t> d_rgb;       // [n][H][W][3]: ck_blob_rgb's pixels (the stage entry point only)
    ck_dev_buf<uint32_t> d_bits;     // [2][n][nc][H][ww] the planes, and the other side of the morphology's ping-pong
    ck_dev_buf<uint32_t> d_parent;   // [n][nc][H][32 ww] union-find over the runs: an entry per pixel, used at the first pixel of every run of a word
    ck_dev_buf<uint32_t> d_area;     // [n][nc][H][32 ww] at a root: its area, then its slot | 2^31 (or ~0: none)
    ck_dev_buf<uint32_t> d_nslot;    // [n][nc] roots of min_area pixels and more
    ck_dev_buf<ckb_comp> d_comps;    // [n][nc][maxc]
    ck_dev_buf<uint32_t> d_list;     // [n][nc][maxc] slots that pass the filter
    ck_dev_buf<ck_blob_t> d_out;     // [n][nc][cap]
    ck_dev_buf<int32_t> d_counts;    // [n][nc]
    ck_dev_buf<uint32_t> d_status;   // [n]
    hipEvent_t ev[2] = {nullptr, nullptr}; // ck_blob_time's
    ~ck_blob_ws() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// k_blobs.hip, everything enqueued on the handle's stream.  P.d_frames holds the n indices.
int ck_launch_blob_rgb(ck_handle *h, const ck_blob_geom &g, const ck_pv_src &src, int n, uint8_t *d_out);
// threshold of all classes into side 0 of d_bits, then (stage 1) the morphology; *side: where the final planes lie
int ck_launch_blob_mask(ck_handle *h, const ck_blob_geom &g, const ck_blob_params_t &pp, const ck_pv_src &src, int n, int stage, int *side);
// labelling, statistics and records of the planes at `side`: d_out, d_counts, d_status
int ck_launch_blob_components(ck_handle *h, const ck_blob_geom &g, const ck_blob_params_t &pp, const ckb_geo &geo, int n, int side);

// ck_blobs.hip: the one path of the detect entry points on a colour source (the ring's is in ck_ingest.hip, where the ring is defined)
int ck_blobs_run(ck_handle *h, const ck_blob_params_t *pp, const ck_pv_color_src &src, const int32_t *frames, int32_t n, ck_blob_t *out,
                 int32_t cap, int32_t *counts, uint32_t *status);

#endif
