// Internal declarations shared by the HIP translation units of libchalkydri_hip.so.
#ifndef CK_INTERNAL_H
#define CK_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "chalkydri_hip.h"

// ---- label word format (segment stage output; DESIGN.md §Data layout) --------------------------------
// 16 bits per pixel, TILE-LOCAL (the consumer knows the pixel's 32 x 128 tile from its coordinates):
// bit  15     CK_LBL_BORDER: the tile-local component touches its tile's outer ring, so it may continue in a neighbouring tile;
//             bits 0..8 are its tile-local id, SLOT = tile index * CK_RING_CAP + id in the frame's tables:
//             groot[slot] = pixel index of the frame-level root, gsize[slot] = the component's pixel count (exact while below
//             min_component_px) — two independent reads
// bit  14     CK_LBL_SMALL : tile-interior component with fewer than min_component_px pixels (final)
// bits 0..11  (neither BORDER nor all ones) tile pixel (row << 7 | column) of the component's root inside the pixel's own tile:
//             its pixel index in the frame is (tile_y0 + row) * width + tile_x0 + column
// 0xFFFF      pixel thresholded to 127 (no component)
// (Round 3: the words were 32 bits with frame-level indices — 4 of the stage's 6 bytes per pixel of HBM traffic.)
typedef uint16_t ck_label_t;
#define CK_LBL_BORDER 0x8000u
#define CK_LBL_SMALL 0x4000u
#define CK_LBL_LOCAL_MASK 0x0FFFu
#define CK_LBL_ID_MASK 0x01FFu
#define CK_LBL_NONE 0xFFFFu
#define CK_LBL_INVALID 0xFFFFFFFFu /* "no component" in CANONICAL label arrays (32-bit pixel indices: the C ABI's label output) */

// CCL tile geometry (one workgroup per tile)
#define CK_TW 128
#define CK_TH 32
#define CK_RING_CAP (2 * (CK_TW + CK_TH)) /* ring-touching roots a tile can have: one per ring pixel at most */

// frame-level resolution of a label word at pixel (x, y): the root's pixel index for an interior component, CK_LBL_INVALID for none;
// a ring-touching component (CK_LBL_BORDER) is resolved by the caller through the slot tables (ck_label_slot).
// Both are a term of the pixel's CCL tile + a term of the label word: k_emit2's group staging forms the tile terms once for four
// pixels of one tile (ck_emit_stage.h: ck_es_slot_base, ck_es_root_base; tests/cpp/emit_stage_check.cpp holds the two texts together)
__host__ __device__ inline uint32_t ck_label_slot(uint32_t l, int x, int y, int ccl_tiles_x) {
    return (uint32_t)((y / CK_TH) * ccl_tiles_x + x / CK_TW) * (uint32_t)CK_RING_CAP + (l & CK_LBL_ID_MASK);
}
__host__ __device__ inline uint32_t ck_label_interior_root(uint32_t l, int x, int y, int w) {
    return (uint32_t)((y & ~(CK_TH - 1)) + (int)((l >> 7) & (CK_TH - 1))) * (uint32_t)w + (uint32_t)((x & ~(CK_TW - 1)) + (int)(l & (CK_TW - 1)));
}

struct ck_border_root {
    uint32_t root; // pixel index of a tile-local root whose component touches the tile ring
    uint32_t size; // its tile-local pixel count
};

struct ck_dev_family {
    uint32_t nbits, ncodes, n_upstream;
    int32_t width_at_border, total_width, reversed_border;
    const uint64_t *codes; // device
    uint32_t bit_x[64], bit_y[64];
};

// One boundary point while it waits to be grouped (k_clusters.hip)
// size classes of the quad fit (k_quads.hip), by list index: 0: 257..512 points per cluster, 1: 1025..2048, 2: <= 4096, 3: <= 8192,
// 4: <= 16384, 5: the rest (up to 3 * (2w + 2h): only frames with more than 2730 pixels of half-perimeter can have such clusters),
// 6: 513..1024, 7: <= 256 (the two youngest classes took the free indices: a cluster's cost is mostly per cluster, not per
// point, so the small ones run on small workgroups, many per CU)
constexpr int CK_FIT_CLASSES = 8;
constexpr int CK_FIT_LISTS = 9;    // work lists: one per size class + (index 8) every cluster of the batch, which the tail kernel of the split fit walks
// The split quad fit (k_quads.hip: k_seq -> k_chunk -> k_tail) passes a cluster's sorted, de-duplicated points on as an
// EXTENDED sequence: its last CK_EXT_PRE points, the points, its first CK_EXT_POST points again — so that the windowed line-fit
// error, its smoothing and the maxima test of every point read neighbours at plain offsets and a kernel can stream over all
// clusters of a frame without knowing where one ends.  A cluster's place in the frame's sequence is handed out when it gets there
// (a per-frame counter); it needs its point count after duplicate removal + CK_EXT_HALO positions.
constexpr int CK_EXT_PRE = 25, CK_EXT_POST = 24, CK_EXT_HALO = CK_EXT_PRE + CK_EXT_POST;
constexpr int CK_SPAN = 960;       // positions one k_chunk workgroup decides (15 words of 64), CK_SPAN / 2 = most maxima it can find
constexpr int CK_HUGE_CAP = 65536, CK_HUGE_WGS = 256; // largest class: points per cluster (3 * 4 * 4095 < 65536), workgroups in its grid
constexpr int CK_FIT_PARALLEL_MAX_FRAMES = 16; // calls with at most this many frames (twice as many at quad_decimate >= 2) run the classes side by side
constexpr int CK_FIT_SIDE_STREAMS = 2;         // ... on the handle's stream and this many more (a process has few hardware queues)
constexpr int CK_LSCRATCH_PER_WG = 16384, CK_LSCRATCH_WGS = 1024; // large class: points per cluster, workgroups in its grid (at most)

#include "ck_point.h" // ck_packed_point: a boundary point inside the pipeline, 32 bits
// One (tile, cluster) run of boundary points in the temp array
struct ck_run {
    uint32_t slot;      // hash-table slot of the cluster
    uint32_t base;      // unused (the run's place inside the cluster is handed out by k_scatter)
    uint32_t tmp_start; // where the run starts in the frame's temp array
    uint32_t count;
};

// Workspace of the irregular stages, sized for cfg.max_batch frames
struct ck_stage_ws {
    int ht_size;               // hash-table slots per frame (power of two)
    int point_cap, cluster_cap, quad_cap, det_cap;
    int max_cluster_points;
    unsigned long long *d_ht_keys; // [n][ht_size]  (rep0<<32 | rep1), 0 = empty
    unsigned long long *d_ht_count; // [n][ht_size] points of the cluster: logical count << 32 | physical count (one add carries both)
    uint32_t *d_ht_off;        // [n][ht_size] start of the cluster in d_points (k_scatter advances it as it fills), or 0xFFFFFFFF
    ck_packed_point *d_tmp;    // [n][ext_cap] (point_cap used) points in emission order (runs)
    ck_packed_point *d_points; // [n][ext_cap] (point_cap used) points grouped by cluster
    // split quad fit: extended point sequences and what k_chunk leaves for k_tail.  d_tmp and d_points are dead by then and carry
    // the two largest arrays (same frame pitch, so a frame's bytes never overlap another frame's)
    int ext_cap;               // positions per frame: point_cap + CK_EXT_HALO * cluster_cap (+ ck_ext_room()), rounded up to a multiple of CK_SPAN; the frame pitch of d_tmp / d_points
    uint32_t *d_ext_xy;        // = d_tmp: [n][ext_cap] x << 13 | y (half-pixel) | window half-width << 26
    uint16_t *d_ext_w;         // [n][ext_cap] gradient weight
    double *d_maxval;          // = d_points: [n][ext_cap / CK_SPAN][CK_SPAN / 2] smoothed errors at the maxima of a span, in position order
    uint16_t *d_maxpos;        // same shape: the maximum's position inside its span
    unsigned long long *d_maxmask; // [n][ext_cap / 64] bit = position is a maximum
    uint16_t *d_maxpre;        // [n][ext_cap / 64] maxima of the span before this word
    long long *d_blk;          // [n][ext_cap / 32][6] moment sums (Mx, My, Mxx, Mxy, Myy, W) from the first position of the block's span (CK_SPAN positions) through the block's last
    uint32_t *d_cstate;        // [n][cluster_cap][2] points left after duplicate removal | reversed border << 31 (0: rejected before the fit), first position of the cluster's extended sequence
    ck_run *d_runs;            // [n][run_cap]
    int run_cap;
    unsigned long long *d_lscratch; // [CK_LSCRATCH_WGS][CK_LSCRATCH_PER_WG]: sort scratch / maxima list of the large fit class, per workgroup
    unsigned long long *d_hscratch; // [CK_HUGE_WGS][2][hcap]: keys + sort scratch / maxima list of the largest class (null when no cluster can be that large)
    int hcap;                       // points per cluster that buffer is laid out for: max_cluster_points rounded up to 1024 (<= CK_HUGE_CAP)
    ck_cluster_t *d_clusters;  // [n][cluster_cap]
    uint32_t *d_counters;      // [n][8]: 0 tmp points, 1 clusters, 2 kept points, 3 quads, 4 detections, 5 status
    ck_quad_t *d_quads;        // [n][quad_cap]
    ck_detection_t *d_dets;    // [n][det_cap]
    uint16_t *d_wimg;          // [n][qh][qw] gradient-magnitude weight of every pixel (isqrt(gx^2+gy^2)+1; 1 on the frame ring)
    void *d_fit_scratch;       // work lists of the quad-fit classes + decode candidates
    size_t fit_scratch_bytes;
    // pose stage (glue + SQPnP), sized for max_batch frames and det_cap tags per frame
    ck_field_tag_t *d_field; int field_cap;
    double *d_gyro; uint8_t *d_has_gyro;
    ck_sqpnp_problem_t *d_problems;
    ck_iso3_t *d_pose_tags;    // [n][det_cap]
    double *d_bearings;        // [n][det_cap][4][3]
    double *d_world;           // [n][det_cap][4][3]
    ck_sqpnp_result_t *d_results;
    ck_vision_measurement_t *d_meas;
    int32_t *d_valid;
};
#define CK_CNT_TMP 0
#define CK_CNT_CLUSTERS 1 /* written by k_scan; until then k_emit2's running count of emitted points, twins counted twice */
#define CK_CNT_POINTS 2
#define CK_CNT_QUADS 3
#define CK_CNT_DETS 4
#define CK_CNT_STATUS 5
#define CK_CNT_RUNS 6
#define CK_CNT_EXT 7 /* split quad fit: positions of the frame's extended sequences handed out so far */
#define CK_CNT_STRIDE 8

struct ck_handle {
    ck_config_t cfg;
    int device;
    hipStream_t stream;   // every stage of a call runs here (ck_stages.hip: run_pipeline), but for the quad fit's side lanes below
    hipEvent_t ev[16];
    // a call with a few frames runs the size classes of the quad fit side by side (k_quads.hip): each class is then a handful of
    // workgroups whose time is one cluster's dependency chain, and five chains in a row were a quarter of a one-frame call
    hipStream_t fit_stream[CK_FIT_SIDE_STREAMS];
    hipEvent_t ev_fit_fork, ev_fit_join[CK_FIT_SIDE_STREAMS];
    int w, h;            // full-resolution frame
    int qw, qh;          // geometry of the image the quad stages run on (w/decimate)
    int tiles_x, tiles_y;
    size_t npix;         // qw*qh
    // device buffers, sized for cfg.max_batch frames
    uint8_t *d_frames;   // staged input frames, pitch = frame_stride
    int frame_stride;
    size_t frame_pitch;
    uint8_t *d_qframes;  // the quad image Q when it is a buffer of its own (ck_quad_separate): decimated and/or filtered copy, rows
                         // padded to 16 bytes; at quad_decimate 1 allocated by the first ck_set_quad_sigma that turns the filter on
    // quad_sigma (k_prefilter.hip): qf_ksz <= 1 = no filter (the default: nothing about the path changes)
    float quad_sigma;
    int qf_ksz;          // taps of the Gaussian, odd, <= 33
    uint8_t qf_k[33];    // its u8 weights (ck_quad_sigma_kernel)
    uint8_t *d_thresh;   // [n][qh][qw]
    ck_label_t *d_labels; // [n][qh][qw] label words
    uint32_t *d_groot;   // [n][broot_cap] slot table: frame-level root (pixel index) of every ring-touching tile-local component
    uint32_t *d_gsize;   // [n][broot_cap] slot table: its pixel count (exact while below min_component_px)
    uint32_t *d_gscratch; // [n][2][broot_cap] parents and sizes of k_fmerge's global-memory path
    uint32_t *d_xband;    // [n][2][broot_cap] a frame joined in bands of tile rows: every slot's root within its band, the band roots' parents (k_fseam)
    ck_border_root *d_broots; // [n][2][broot_cap]: per tile a slice of CK_RING_CAP entries (k_tile), then the same entries packed (k_fmerge)
    uint32_t *d_tile_count;   // [n][tiles]: entries used in every tile's slice
    int broot_cap;            // tiles * CK_RING_CAP
    // ids of the ring-touching roots along the tile boundaries (k_tile writes them, k_fmerge joins across them), per frame:
    // HT[tiles_y][qw] top rows | HB[tiles_y][qw] bottom rows | VL[tiles_x][qh] left columns | VR[tiles_x][qh] right columns;
    // an entry = index into the frame's d_broots list | colour << 15 (1 = white), 0xFFFF = no colour
    uint16_t *d_ring;         // [n][ring_len]
    size_t ring_len;
    // later stages
    ck_stage_ws ws;      // workspace of clusters / quads / decode
    int pts_distinct;    // what ck_launch_clusters says of the points it left in ws.d_points: 1 = no coordinate twice in a cluster (k_emit2
                         // merged the diagonal twins, the only points that share one), so the quad fit's front half searches for none
    ck_stage_ms_t last_ms;
    ck_dev_family *d_fams;
    uint64_t *d_fam_codes; // every family's code table, one after the other (ck_dev_family::codes point into it)
    int n_staged;        // frames currently staged in d_frames (assigned through ck_set_staged only)
    // the raw frames the staged ones were converted from, while they still lie in raw->d_stage (ck_upload_raw, ck_raw_luma_batch):
    // what ck_preview_jpeg_color reads.  n_raw_staged = -1: the frames were staged another way since
    int n_raw_staged;
    ck_raw_format_t raw_staged_fmt;
    // the frames the last ck_upload_jpeg_color staged, while their chroma planes still lie in jpeg->d_planes: the other source of
    // ck_preview_jpeg_color.  -1: the frames were staged another way since
    int n_jpeg_color, jpeg_color_orientation;
    int n_last_pose;     // records the last ck_process_* call left in ws.d_meas (what ck_gather_poses may send); -1: none yet
    int n_pose_inputs;   // frames whose glue records (ws.d_problems, d_pose_tags, d_bearings) and detection counts the last ck_process_* call
                         // left in ws (what ck_rig_process_last reads in place); -1: none yet, or a later pipeline call rewrote the workspace
    int n_last_dets;     // frames whose detections the last ck_detect_* / ck_process_* call left in ws (what ck_last_tag_poses reads);
                         // -1: none yet, or a later call (ck_clusters_batch, ck_quads_batch, ck_decode_quads_batch, a failed pipeline) rewrote the workspace
    // per-tag pose (k_tagpose.hip): allocated by the first ck_estimate_tag_poses / ck_last_tag_poses, max_batch * det_cap entries
    ck_detection_t *d_tp_dets; // caller detections staged for ck_estimate_tag_poses
    ck_tag_pose_t *d_tp_out;   // pose records
    int32_t *d_tp_counts;      // [max_batch] per-frame counts of ck_last_tag_poses
    // baseline JPEG decode (ck_jpeg.hip, k_jpeg.hip): allocated by the first ck_upload_jpeg / ck_jpeg_luma_batch, grown on demand
    struct ck_jpeg_ws *jpeg;
    // raw camera formats (ck_rawfmt.hip, k_rawfmt.hip): staging of the host-frame entry points, allocated by the first raw call
    struct ck_raw_ws *raw;
    // JPEG preview of the staged frames (ck_preview.hip, k_jpegenc.hip): allocated by the first preview call, grown on demand
    struct ck_preview_ws *preview;
    // exposure metering of the staged frames (ck_exposure.hip, k_exposure.hip): allocated by the first exposure call, grown on demand
    struct ck_exposure_ws *exposure;
    // iterative tri-class Otsu threshold (ck_tri_otsu.hip, k_tri_otsu.hip): allocated by the first tri-class call, grown on demand
    struct ck_tri_otsu_ws *tri_otsu;
    // camera calibration (ck_calib.hip, k_calib.hip): allocated by the first calibration call, grown on demand
    struct ck_calib_ws *calib;
    // camera rig (k_rigpnp.hip): allocated by the first rig call, grown on demand
    struct ck_rig_ws *rig;
    // mount calibration (ck_rigcal.hip, k_rigcal.hip): allocated by the first mount calibration call, grown on demand
    struct ck_rigcal_ws *rigcal;
    // field calibration (ck_fieldcal.hip, k_fieldcal.hip): allocated by the first field calibration call, grown on demand
    struct ck_fieldcal_ws *fieldcal;
    // rig pose refinement (ck_rig_refine.hip, k_rig_refine.hip): allocated by the first refinement call, grown on demand
    struct ck_rig_refine_ws *rig_refine;
    // coloured game pieces (ck_blobs.hip, k_blobs.hip): allocated by the first blob call, grown on demand
    struct ck_blob_ws *blobs;
    bool fmerge_lds_allowed; // k_fmerge's dynamic LDS limit has been raised on this handle's device
    // ck_set_camera: while has_camera, the glue and the per-tag pose unproject with `camera` (UCM's k[5] already 1.0) instead of their
    // params' OpenCVModel5; 0 (the default): nothing about those paths changes
    int has_camera;
    ck_camera_t camera;
    // ck_set_corner_subpix: while has_subpix, the detections a pipeline call leaves in ws.d_dets get their corners refined on the frame
    // the call was given (ck_subpix.hip: k_subpix_dets, launched by run_pipeline); 0 (the default): no launch is added
    int has_subpix;
    ck_subpix_params_t subpix;
    // sub-pixel corners (ck_subpix.hip): the weight tables and the staging of its calls, allocated by the first of them
    struct ck_subpix_ws *subpix_ws;
    // the full-resolution frames of the call that left n_last_dets detections (what ck_board_corners_last reads): the staged frames,
    // an ingest slot, or the caller's device memory, which has to be there still
    const uint8_t *last_img_p;
    int last_img_stride;
    size_t last_img_pitch;
};

// the camera a pose kernel takes: the handle's setting, or the params' OpenCVModel5 in ck_camera_t's clothes
static inline ck_camera_t ck_kernel_camera(const ck_handle *h, const ck_opencv5_t &c) {
    if (h->has_camera) return h->camera;
    ck_camera_t cam;
    cam.model = CK_CAMERA_OPENCV5; cam.pad = 0;
    cam.k[0] = c.fx; cam.k[1] = c.fy; cam.k[2] = c.cx; cam.k[3] = c.cy; cam.k[4] = c.k1; cam.k[5] = c.k2; cam.k[6] = c.p1; cam.k[7] = c.p2; cam.k[8] = c.k3;
    return cam;
}

extern thread_local char ck_err_text[512];
// The one path of a failed runtime call (ck_api.hip): writes ck_err_text, clears the runtime's per-thread error (the next launch
// check must not meet it) and gives the code: CK_ENOMEM for an allocation that failed for lack of memory, CK_EDEVICE otherwise.
int ck_hip_failed(hipError_t e, const char *call, const char *file, int line, bool alloc);
#define CK_HIP_(call, alloc)                                                              \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) return ck_hip_failed(e_, #call, __FILE__, __LINE__, alloc); \
    } while (0)
#define CK_HIP(call) CK_HIP_(call, false)
#define CK_HIP_ALLOC(call) CK_HIP_(call, true)

// The diagnostic knobs (ck_knob(CK_KNOB_...): values only the diagnostics library takes from the environment) have one table: ck_knobs.h.
#include "ck_knobs.h"

// The quad stages run on a buffer of their own (d_qframes) when the frame is decimated or filtered; otherwise on the frame itself.
static inline bool ck_quad_separate(const ck_handle *h) { return h->cfg.quad_decimate > 1 || h->qf_ksz > 1; }
// Edge refinement and decode read the quad image instead of the frame: at quad_decimate 1 with the filter on (upstream blurs the
// caller's image in place there, so its later stages see the filtered pixels).  The one routing predicate.
static inline bool ck_refine_reads_quad(const ck_handle *h) { return h->cfg.quad_decimate == 1 && h->qf_ksz > 1; }
// n frames of 8-bit pixels on the device: row i of frame f starts at p + f * pitch + i * stride
struct ck_dev_image { const uint8_t *p; int stride; size_t pitch; };
static inline ck_dev_image ck_staged_image(const ck_handle *h) { return {h->d_frames, h->frame_stride, h->frame_pitch}; }
// d_qframes as an image (rows padded to 16 bytes), whether or not the quad stages use it at the moment: the one place its pitch is
static inline ck_dev_image ck_qframes_image(const ck_handle *h) {
    const int stride = (h->qw + 15) / 16 * 16;
    return {h->d_qframes, stride, (size_t)stride * h->qh};
}
// the image the quad stages (threshold .. quad fit) read, and the one edge refinement and decode read, for the input image `in`
static inline ck_dev_image ck_quad_image(const ck_handle *h, const ck_dev_image &in) { return ck_quad_separate(h) ? ck_qframes_image(h) : in; }
static inline ck_dev_image ck_refine_image(const ck_handle *h, const ck_dev_image &in) { return ck_refine_reads_quad(h) ? ck_qframes_image(h) : in; }

// Frames arrive turned by the camera's mounting (CK_ORIENT_*): the handle's w x h is the ORIENTED frame, its source is h x w for
// the quarter turns.  The one range check and the one source geometry of the JPEG and raw-format paths.
static inline bool ck_orientation_ok(int o) { return o >= CK_ORIENT_NONE && o <= CK_ORIENT_COUNTERCLOCKWISE; }
static inline void ck_source_size(int w, int h, int orientation, int *sw, int *sh) {
    const bool quarter = orientation == CK_ORIENT_CLOCKWISE || orientation == CK_ORIENT_COUNTERCLOCKWISE;
    *sw = quarter ? h : w;
    *sh = quarter ? w : h;
}
// The one place n_staged is assigned: frames staged any other way than from the raw staging take its colour twin with them
static inline void ck_set_staged(ck_handle *h, int n) {
    h->n_staged = n;
    h->n_raw_staged = -1;
    h->n_jpeg_color = -1;
}
// a caller's list of n frame indices (null: 0 .. n - 1): every entry is one of the n_avail frames at hand
static inline bool ck_frame_list_ok(const int32_t *frames, int n, int n_avail) {
    for (int i = 0; i < n; i++) {
        const int f = frames ? frames[i] : i;
        if (f < 0 || f >= n_avail) return false;
    }
    return true;
}

// Device allocation of the handle's buffers.  CK_POISON=1 (tests) fills every buffer with 0xA5 bytes, so that a kernel which
// reads an entry nobody wrote in this call — what an undersized capacity once made of the cluster and run tables — meets the
// same garbage on every run instead of whatever the allocator happens to hand back.  CK_POISON=2 also lists the buffers.
// CK_POISON=3 gives every buffer a virtual-address range of its own, mapped so that the buffer ENDS at the end of the mapping
// and the next granule is reserved but unmapped: an access past a buffer's end is a GPU memory fault at once, wherever the
// allocator would have put its neighbours (guard pages; hipMemAddressReserve / hipMemCreate / hipMemMap).
struct ck_guarded_alloc { void *va; size_t va_bytes; hipMemGenericAllocationHandle_t mem; size_t map_bytes; };
hipError_t ck_guarded_malloc(void **p, size_t bytes); // ck_api.hip
bool ck_guarded_free(void *p);                        // true when p was a guarded allocation (and is released now)
template <typename T>
static inline hipError_t ck_malloc_dev_at(T **p, size_t bytes, const char *what, int line) {
    const char *pe = getenv("CK_POISON"); // (read per allocation: a test sets it for the handles it creates)
    const int poison = pe ? atoi(pe) : 0;
    hipError_t e = (poison >= 3 && bytes && bytes < ((size_t)1 << 30)) ? ck_guarded_malloc( // (buffers of a gigabyte and more keep the plain allocator)
                   reinterpret_cast<void **>(p), bytes) : hipMalloc(reinterpret_cast<void **>(p), bytes);
    if (e == hipSuccess && poison && bytes) {
        e = hipMemset(*p, 0xA5, bytes);
        if (e == hipSuccess) e = hipDeviceSynchronize(); // (the fill is asynchronous, and the handle's streams do not wait for the null stream)
    }
    if (poison >= 2) fprintf(stderr, "ck_alloc %p..%p %zu %s:%d\n", (void *)*p, (void *)((char *)*p + bytes), bytes, what, line);
    return e;
}
#define ck_malloc_dev(p, bytes) ck_malloc_dev_at(p, bytes, #p, __LINE__)
static inline hipError_t ck_free_dev(const void *p) {
    if (p && ck_guarded_free(const_cast<void *>(p))) return hipSuccess;
    return hipFree(const_cast<void *>(p));
}
// a temporary of one call (plain hipMalloc: not handle workspace)
template <typename T>
struct DevBuf {
    T *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(size_t n) { return hipMalloc(&p, sizeof(T) * (n ? n : 1)) == hipSuccess ? CK_OK : CK_ENOMEM; }
};

// ---- stage launchers (k_*.hip) ------------------------------------------------------------------------
// threshold + tile-local CCL + cross-tile merge + border-root flatten, on frames [0,n) of `frames`
int ck_launch_threshold_segment(ck_handle *h, const ck_dev_image &img, int n, bool precomputed = false);
// canonical labels (min pixel index, flags stripped) and exact sizes — parity/test path, not the hot path
int ck_launch_canonical_labels(ck_handle *h, int n, uint32_t *d_labels_out, uint32_t *d_sizes_out);
int ck_launch_decimate(ck_handle *h, const ck_dev_image &img, int n);
// quad_sigma filter (+ decimation at quad_decimate 2) of frames [0,n) into d_qframes (k_prefilter.hip)
int ck_launch_prefilter(ck_handle *h, const ck_dev_image &img, int n);
// The handle's device buffers, all of them described once by the table in ck_stages.hip: capacities + every buffer ck_create
// allocates; one buffer that is allocated on first use (`member` = the address of its pointer in the handle; a no-op once it
// exists); all of them released
int ck_bufs_create(ck_handle *h);
int ck_buf_alloc(ck_handle *h, const void *member);
void ck_bufs_free(ck_handle *h);
// the staged luma of frames [0, n) into a packed host buffer [n][h][w], enqueued on the handle's stream (ck_api.hip)
int ck_read_staged_luma(ck_handle *h, int n, uint8_t *luma_out);
int ck_stage_device_frames(ck_handle *h, const uint8_t *d_frames, int n, int stride, int64_t frame_pitch, ck_dev_image *use);
int ck_run_threshold_segment(ck_handle *h, const ck_dev_image &img, int n);
// Q of n frames into d_qframes when the quad image is a buffer of its own (decimation and / or quad_sigma); nothing otherwise
int ck_make_quad_image(ck_handle *h, const ck_dev_image &img, int n);
// gradient clusters from thresh/labels/csize of frames [0,n)
int ck_launch_clusters(ck_handle *h, int n);
// quad fit (+ edge refinement) of every cluster; qframes = image the clusters came from, frames = full resolution
int ck_launch_fit_quads(ck_handle *h, const ck_dev_image &qimg, const ck_dev_image &img, int n);
// k_chunk.hip, the one unit whose device code differs in the diagnostics library (ck_knobs.h): the split fit's middle kernel
// k_chunk over the n frames' positions on the handle's stream, `wgs` workgroups over the batch at most (never fewer than 8 a frame, never more
// than a frame has spans).  *fit_stop is the quad fit's stop_after: at 3 and below nothing is launched; a k_chunk that the
// diagnostics library cuts short (CK_CHUNK_STOP_AFTER) lowers it to 4, where k_tail ends every cluster before it reads k_chunk's lists
void ck_launch_chunk(ck_handle *h, int n, int wgs, int *fit_stop);
// diagnostics library: the n frames' position counters start at CK_EXT_BASE, on the handle's stream.  Product: nothing
void ck_launch_ext_base(ck_handle *h, int n);
// positions a frame's extended sequences are longer by for CK_EXT_BASE: 2 * CK_SPAN in the diagnostics library, 0 in the product
int ck_ext_room();
int ck_launch_decode(ck_handle *h, const ck_dev_image &img, int n);
// whole pipeline on device-resident frames (16-byte aligned rows): detections to the host / pose records
int ck_detect_frames(ck_handle *h, const ck_dev_image &img, int n, ck_detection_t *dets, int cap, int32_t *counts, uint32_t *status);
int ck_process_frames(ck_handle *h, const ck_dev_image &img, int n, const ck_process_params_t *pp, const double *gyro,
                      const uint8_t *has_gyro, ck_vision_measurement_t *out, int32_t *valid);
// glue + SQPnP + measurement on the detections left on the device by the last pipeline run
int ck_launch_sqpnp_last(ck_handle *h, int n, const ck_sqpnp_params_t *prm, hipStream_t stream); // k_sqpnp.hip
int ck_run_pose(ck_handle *h, int n, const ck_process_params_t *pp, const double *gyro, const uint8_t *has_gyro,
                ck_vision_measurement_t *out, int32_t *valid, bool upload_field = true, bool sync = true);

// Layout of the fit scratch (ck_stage_ws::d_fit_scratch): [CK_FIT_LISTS][list_cap] work-list entries, 16 list counts,
// 16 dequeue heads, then (256-byte aligned) the decode candidates' per-frame counts and the candidates themselves.
struct ck_fit_layout {
    int list_cap;
    uint32_t *lists, *list_counts, *heads, *cand_count;
    ck_detection_t *cands;
};
static inline ck_fit_layout ck_fit_scratch_layout(const ck_stage_ws &ws, int max_batch) {
    ck_fit_layout L;
    L.list_cap = ws.cluster_cap * max_batch;
    L.lists = reinterpret_cast<uint32_t *>(ws.d_fit_scratch);
    L.list_counts = L.lists + (size_t)CK_FIT_LISTS * L.list_cap;
    L.heads = L.list_counts + 16;
    const size_t list_bytes = ((size_t)CK_FIT_LISTS * L.list_cap + 32) * sizeof(uint32_t);
    uint8_t *base = reinterpret_cast<uint8_t *>(ws.d_fit_scratch) + ((list_bytes + 255) / 256) * 256;
    L.cand_count = reinterpret_cast<uint32_t *>(base);
    L.cands = reinterpret_cast<ck_detection_t *>(base + (((size_t)max_batch * 4 + 255) / 256) * 256);
    return L;
}

#ifdef __HIPCC__
// Wave-wide inclusive sums on the DPP path (no LDS crossbar, no lane-index arithmetic): four row_shr steps inside each
// row of 16 lanes, then row_bcast:15 into rows 1 and 3 and row_bcast:31 into rows 2 and 3.  Lanes without a source add 0.
template <int CTRL, int ROWS>
__device__ __forceinline__ uint32_t dpp0(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWS, 0xF, true); }
template <int CTRL, int ROWS>
__device__ __forceinline__ unsigned long long dpp0_64(unsigned long long v) {
    return ((unsigned long long)dpp0<CTRL, ROWS>((uint32_t)(v >> 32)) << 32) | dpp0<CTRL, ROWS>((uint32_t)v);
}
__device__ __forceinline__ uint32_t wave_scan_u32(uint32_t x) {
    x += dpp0<0x111, 0xF>(x); x += dpp0<0x112, 0xF>(x); x += dpp0<0x114, 0xF>(x); x += dpp0<0x118, 0xF>(x);
    x += dpp0<0x142, 0xA>(x); x += dpp0<0x143, 0xC>(x);
    return x;
}
// the same inside every row of 16 lanes on its own (the first four steps): sixteen values and fewer, one per lane of a row
__device__ __forceinline__ uint32_t row_scan_u32(uint32_t x) {
    x += dpp0<0x111, 0xF>(x); x += dpp0<0x112, 0xF>(x); x += dpp0<0x114, 0xF>(x); x += dpp0<0x118, 0xF>(x);
    return x;
}
__device__ __forceinline__ unsigned long long wave_scan_u64(unsigned long long x) {
    x += dpp0_64<0x111, 0xF>(x); x += dpp0_64<0x112, 0xF>(x); x += dpp0_64<0x114, 0xF>(x); x += dpp0_64<0x118, 0xF>(x);
    x += dpp0_64<0x142, 0xA>(x); x += dpp0_64<0x143, 0xC>(x);
    return x;
}

__device__ __forceinline__ int wave_min_i32(int x) { // same DPP ladder with min; lanes without a source keep their own value
    x = min(x, __builtin_amdgcn_update_dpp(x, x, 0x111, 0xF, 0xF, false));
    x = min(x, __builtin_amdgcn_update_dpp(x, x, 0x112, 0xF, 0xF, false));
    x = min(x, __builtin_amdgcn_update_dpp(x, x, 0x114, 0xF, 0xF, false));
    x = min(x, __builtin_amdgcn_update_dpp(x, x, 0x118, 0xF, 0xF, false));
    x = min(x, __builtin_amdgcn_update_dpp(x, x, 0x142, 0xA, 0xF, false));
    x = min(x, __builtin_amdgcn_update_dpp(x, x, 0x143, 0xC, 0xF, false));
    return __builtin_amdgcn_readlane(x, 63);
}

// Moves inside every group of four lanes (DPP quad_perm: lane i of a group reads lane A, B, C or D of its own group for i = 0..3).
// Every lane has a source; call them where all lanes are active.
template <int A, int B, int C, int D>
__device__ __forceinline__ uint32_t quad_perm_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, A | (B << 2) | (C << 4) | (D << 6), 0xF, 0xF, true);
}
template <int A, int B, int C, int D>
__device__ __forceinline__ unsigned long long quad_perm_u64(unsigned long long v) {
    return ((unsigned long long)quad_perm_u32<A, B, C, D>((uint32_t)(v >> 32)) << 32) | quad_perm_u32<A, B, C, D>((uint32_t)v);
}
template <int A, int B, int C, int D>
__device__ __forceinline__ double quad_perm_f64(double v) {
    return __longlong_as_double((long long)quad_perm_u64<A, B, C, D>((unsigned long long)__double_as_longlong(v)));
}
// sums over every group of four lanes, in all four of them
__device__ __forceinline__ uint32_t quad_sum_u32(uint32_t x) { x += quad_perm_u32<2, 3, 0, 1>(x); return x + quad_perm_u32<1, 0, 3, 2>(x); }
__device__ __forceinline__ unsigned long long quad_sum_u64(unsigned long long x) { x += quad_perm_u64<2, 3, 0, 1>(x); return x + quad_perm_u64<1, 0, 3, 2>(x); }

// The wave's smallest pair (key, tag) in lexicographic order, for every lane: wave_min_i32's ladder on three words.  Lanes without a
// source meet their own pair.
template <int CTRL, int ROWS>
__device__ __forceinline__ void argmin_step(unsigned long long &key, int &tag) {
    const uint32_t lo = (uint32_t)key, hi = (uint32_t)(key >> 32);
    const uint32_t olo = (uint32_t)__builtin_amdgcn_update_dpp((int)lo, (int)lo, CTRL, ROWS, 0xF, false);
    const uint32_t ohi = (uint32_t)__builtin_amdgcn_update_dpp((int)hi, (int)hi, CTRL, ROWS, 0xF, false);
    const int otag = __builtin_amdgcn_update_dpp(tag, tag, CTRL, ROWS, 0xF, false);
    const unsigned long long okey = ((unsigned long long)ohi << 32) | olo;
    if (okey < key || (okey == key && otag < tag)) { key = okey; tag = otag; }
}
__device__ __forceinline__ void wave_argmin_u64_i32(unsigned long long &key, int &tag) {
    argmin_step<0x111, 0xF>(key, tag); argmin_step<0x112, 0xF>(key, tag); argmin_step<0x114, 0xF>(key, tag); argmin_step<0x118, 0xF>(key, tag);
    argmin_step<0x142, 0xA>(key, tag); argmin_step<0x143, 0xC>(key, tag);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)key, 63), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(key >> 32), 63);
    key = ((unsigned long long)hi << 32) | lo;
    tag = __builtin_amdgcn_readlane(tag, 63);
}

// The wave's largest key, for every lane, on the same ladder (two words per step, no LDS).
template <int CTRL, int ROWS>
__device__ __forceinline__ unsigned long long max_step_u64(unsigned long long key) {
    const uint32_t lo = (uint32_t)key, hi = (uint32_t)(key >> 32);
    const uint32_t olo = (uint32_t)__builtin_amdgcn_update_dpp((int)lo, (int)lo, CTRL, ROWS, 0xF, false);
    const uint32_t ohi = (uint32_t)__builtin_amdgcn_update_dpp((int)hi, (int)hi, CTRL, ROWS, 0xF, false);
    const unsigned long long okey = ((unsigned long long)ohi << 32) | olo;
    return okey > key ? okey : key;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long key) {
    key = max_step_u64<0x111, 0xF>(key); key = max_step_u64<0x112, 0xF>(key); key = max_step_u64<0x114, 0xF>(key); key = max_step_u64<0x118, 0xF>(key);
    key = max_step_u64<0x142, 0xA>(key); key = max_step_u64<0x143, 0xC>(key);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)key, 63), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(key >> 32), 63);
    return ((unsigned long long)hi << 32) | lo;
}

// CAT's gray level of an RGB pixel (utils.rs:33-46): trunc(fma(r, 0.33f, fma(g, 0.33f, b * 0.33f))) in f32, saturating.  The one
// map of k_cat.hip and k_tri_otsu.hip.
__device__ __forceinline__ uint8_t ck_cat_grayscale(uint8_t r, uint8_t g, uint8_t b) {
    float v = __fmaf_rn((float)r, 0.33f, __fmaf_rn((float)g, 0.33f, (float)b * 0.33f));
    if (!(v > 0.0f)) return 0;
    if (v >= 255.0f) return 255;
    return (uint8_t)v;
}

#endif // __HIPCC__

#endif
