/*
 * chalkydri_hip.h — C ABI of the MI355X-native AprilTag detect + SQPnP pose hot path.
 *
 * This is the drop-in boundary.  Every entry point is plain C: pointers, sizes and
 * POD structs, no C++/torch types.  Reference citations are relative to /root/reference.
 *
 * What each group replaces in the reference:
 *   ck_image_u8_t ............ the hand-built apriltag `image_u8_t {buf,width,height,stride}` that
 *                              `image_from_cuimage` hands to the C detector  (crates/apriltags/src/lib.rs:197-213)
 *   ck_create/ck_destroy ..... `DetectorBuilder::default().add_family_bits(family,bits).build()` and Drop
 *                              (crates/apriltags/src/lib.rs:258-262,279-282)
 *   ck_detect_batch* ......... `self.detector.detect(&image)` → Vec<Detection> with id()/corners()
 *                              (crates/apriltags/src/lib.rs:301-314), batched over frames
 *   ck_threshold/segment ..... the stages `north_star` scores against the HBM roofline
 *   ck_cat_* ................. chalkydri-apriltags "CAT" `Detector::{calc_otsu,thresh,process_frame,
 *                              detect_corners,check_edges,connected_components}`
 *                              (crates/chalkydri-apriltags/src/lib.rs:191,265,291,319,480,501)
 *   ck_sqpnp_* ............... `SqPnP::{new,max_iter,tolerance,solve_robot_pose,
 *                              create_solver_camera_transform}` (crates/chalkydri_sqpnp/src/lib.rs:201-222,297-377,430-461)
 *   ck_unproject_* ........... `cam_model.unproject(corners)` for OpenCVModel5 (crates/apriltags/src/lib.rs:316-322)
 *   ck_process_batch ......... `AprilTags::process` glue: filter → unproject → solve → VisionMeasurement
 *                              (crates/apriltags/src/lib.rs:293-379; wire struct crates/whacknet/src/lib.rs:43-66)
 *
 * Error convention: every function returning int returns CK_OK (0) or a negative CK_E* code; nothing
 * throws or aborts across the ABI.  Per-frame capacity overflows are reported in status words, not as
 * failures.  A handle is bound to one HIP device and is NOT thread-safe (mirrors `&mut self`).
 */
#ifndef CHALKYDRI_HIP_H
#define CHALKYDRI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CK_ABI_VERSION 3 /* 3: ck_gather_poses takes (n_valid, rows) — a changed prototype is a new version, like a changed struct */

/* ---- status codes ------------------------------------------------------------------------- */
enum {
    CK_OK = 0,
    CK_EINVAL = -1,      /* bad argument (null pointer, size mismatch, unsupported geometry) */
    CK_ENOMEM = -2,      /* host or device allocation failed */
    CK_EDEVICE = -3,     /* HIP runtime error; ck_last_error() has the text */
    CK_ENODEVICE = -4,   /* no HIP device visible: the product path has NO CPU fallback */
    CK_ECAPACITY = -5,   /* batch larger than the handle was created for */
    CK_EUNSUPPORTED = -6 /* valid request this build does not implement */
};

/* per-frame status bits (ck_detect_batch `status[]`) */
enum {
    CK_FRAME_OK = 0,
    CK_FRAME_POINTS_OVERFLOW = 1,   /* boundary-point buffer full: clusters may be missing */
    CK_FRAME_CLUSTERS_OVERFLOW = 2, /* cluster table full.  Also: more than 512 distinct pairs of neighbouring components inside one
                                       64 x 16-pixel tile of the quad image (the stage's per-tile table); the pairs beyond the 512
                                       lose their points.  Reachable only with min_component_px of 1 or 2 (a one-pixel checkerboard
                                       at min_component_px = 1 does it; at the default of 25 a tile has no room for that many
                                       components); the frame's batch neighbours and later calls are not affected */
    CK_FRAME_QUADS_OVERFLOW = 4,    /* more candidate quads than capacity */
    CK_FRAME_DETS_OVERFLOW = 8,     /* more detections than `cap_per_frame` */
    CK_FRAME_UNVERIFIED_ID = 16     /* a detection's id is >= its family's n_upstream (see ck_family_t) */
};

/* ---- images --------------------------------------------------------------------------------- */
/* Layout-identical to apriltag's image_u8_t (crates/apriltags/src/lib.rs:204-209). stride >= width. */
typedef struct ck_image_u8 {
    uint8_t *buf;
    int32_t width;
    int32_t height;
    int32_t stride;
} ck_image_u8_t;

/* ---- tag families (runtime data; AprilTag-3 layout convention) -------------------------------- */
typedef struct ck_family {
    char name[32];
    uint32_t nbits;           /* 36 for tag36h11, 16 for tag16h5 */
    uint32_t ncodes;
    const uint64_t *codes;    /* bit (nbits-1-i) of a code is the cell at (bit_x[i], bit_y[i]) */
    const uint32_t *bit_x;    /* cell coordinates, origin = outer corner of the black border */
    const uint32_t *bit_y;
    int32_t width_at_border;  /* 8 for tag36h11, 6 for tag16h5 */
    int32_t total_width;      /* 10 / 8 (adds the white quiet ring) */
    int32_t reversed_border;  /* 0 for both classic families */
    uint32_t min_hamming;     /* 11 / 5 */
    uint32_t n_upstream;      /* IDs 0..n_upstream-1 are known to equal the upstream AprilTag table of this name.  A caller
                               * that passes upstream's own table sets n_upstream = ncodes.  Detections with a larger id
                               * raise CK_FRAME_UNVERIFIED_ID and are ignored by the pose glue unless
                               * ck_process_params_t.allow_unverified_ids is set.  0 (a zero-initialised table, or one
                               * built against ABI version 1, which had no such field) means ncodes: the caller vouches
                               * for its table; a value above ncodes is refused by ck_create (CK_EINVAL). */
} ck_family_t;
/* What ck_create accepts as a family (CK_EINVAL otherwise): codes, bit_x and bit_y not NULL; 1 <= nbits <= 64;
 * 1 <= ncodes < 2^20; every code < 2^nbits; 1 <= width_at_border <= total_width <= 16; every bit cell inside the grid,
 * min_coord <= bit_x[i], bit_y[i] < min_coord + total_width with min_coord = (width_at_border - total_width) / 2 (C division,
 * AprilTag-3's; bit_x and bit_y are read as int32 there, so cells outside the border are negative); n_upstream <= ncodes.
 * The bit layout must follow AprilTag-3's convention for rotations to decode: bits nbits/4 apart are one quarter turn of the
 * tag apart (the centre cell last when nbits % 4 == 1), as in the built-in tables. */

/* Built-in tables.  "tag16h5": all 30 upstream codes (n_upstream = 30).  "tag36h11": upstream layout, 587 codes of which
 * IDs 0..38 are upstream codes (n_upstream = 39: every tag of the reference's field.json, IDs 1..32) and IDs 39..586 are a
 * stand-in lexicode from tools/gen_family36.c that keeps the codebook search at its real size — NOT upstream IDs; an
 * integrator who needs them passes upstream's tag36h11.c table through ck_config_t.families.
 * Returns NULL for unknown names. */
const ck_family_t *ck_family_builtin(const char *name);

/* ---- detector configuration -------------------------------------------------------------------- */
#define CK_MAX_FAMILIES 4
/* max_quads_per_frame x n_families may not exceed this (ck_create: CK_EINVAL): the de-duplication ranks a frame's decode
 * candidates, one per quad and family, in 4 bytes of workgroup memory each, and 64 KiB is what a launch gets without asking */
#define CK_MAX_FRAME_CANDIDATES 16384

typedef struct ck_config {
    int32_t width, height;        /* frame geometry, fixed per handle (cf. Detector::new(width,height,..)) */
    int32_t max_batch;            /* frames per ck_detect_batch call the workspace is sized for.  Every stage keeps worst-case capacity
                                   * resident, about 86 bytes per pixel of quad-stage image and frame at the default capacities
                                   * (1280 x 800: 88 MB per frame of max_batch; max_points_per_frame / max_clusters_per_frame
                                   * shrink it); ck_create fails with CK_ENOMEM when the device has no room */
    int32_t device;               /* HIP device ordinal */
    /* AprilTag-3 detector defaults the reference inherits unchanged */
    int32_t quad_decimate;        /* 1 (full resolution) or 2 (AT3 default) */
    int32_t min_white_black_diff; /* 5 */
    int32_t min_component_px;     /* 25: components smaller than this emit no boundary points (>= 1) */
    int32_t min_cluster_pixels;   /* 24: smallest cluster handed to the quad fitter */
    int32_t max_nmaxima;          /* 10 */
    double cos_critical_rad;      /* cos(10 deg) */
    double max_line_fit_mse;      /* 10.0 */
    int32_t refine_edges;         /* 1 */
    double decode_sharpening;     /* 0.25 */
    int32_t max_hamming;          /* bits_corrected: 3 with a config, 1 without (lib.rs:230,280) */
    int32_t n_families;
    const ck_family_t *families[CK_MAX_FAMILIES];
    /* capacities of the irregular stages (0 = derive from geometry: 4 points per pixel — the most a frame can produce,
     * one per forward neighbour —, one cluster per 32 pixels, 1024 quads) */
    int32_t max_points_per_frame;
    int32_t max_clusters_per_frame;
    int32_t max_quads_per_frame;
} ck_config_t;

void ck_config_default(ck_config_t *cfg, int32_t width, int32_t height, int32_t max_batch);

/* One decoded tag.  Corner order = apriltag's: bottom-left, bottom-right, top-right, top-left in the
 * tag's own frame, which is what corner_points_from_center assumes (chalkydri_sqpnp/src/lib.rs:383-388). */
typedef struct ck_detection {
    int32_t id;
    int32_t hamming;
    int32_t family;          /* index into ck_config_t.families */
    float decision_margin;
    double c[2];             /* centre, pixels */
    double p[4][2];          /* corners, pixels */
} ck_detection_t;

typedef struct ck_handle ck_handle_t;

int ck_abi_version(void);
const char *ck_strerror(int code);
const char *ck_last_error(void); /* text of the most recent CK_EDEVICE on this thread */
int ck_device_count(void);       /* 0 when no HIP device is visible */

/* Frame geometry accepted by ck_create: any width and height of 16..4095 pixels (at least 8 after quad_decimate) — what an
 * image_u8_t can describe within the 13-bit half-pixel coordinates of the boundary points; quad_decimate 1 or 2
 * (CK_EUNSUPPORTED otherwise); min_component_px >= 1; 1..CK_MAX_FAMILIES families, each valid as ck_family_t's
 * rules say; max_quads_per_frame (1024 when 0) x n_families <= CK_MAX_FRAME_CANDIDATES.
 * CK_EINVAL for everything else.  Arguments are validated before a device is looked for (CK_ENODEVICE). */
int ck_create(const ck_config_t *cfg, ck_handle_t **out);
void ck_destroy(ck_handle_t *h);

/* ---- full pipeline ------------------------------------------------------------------------------ */
/* Host frames in, host detections out (H2D copy inside).  dets is [n][cap_per_frame]; counts[n] gets the
 * number written per frame (sorted by id, then hamming, then margin desc); status[n] may be NULL. */
int ck_detect_batch(ck_handle_t *h, const ck_image_u8_t *imgs, int32_t n, ck_detection_t *dets,
                    int32_t cap_per_frame, int32_t *counts, uint32_t *status);

/* Frames already resident in HBM: d_frames is a device pointer to n frames of height rows, row pitch
 * `stride` bytes, frame pitch `frame_pitch` bytes.  Results land in host arrays as above. */
int ck_detect_batch_device(ck_handle_t *h, const uint8_t *d_frames, int32_t n, int32_t stride,
                           int64_t frame_pitch, ck_detection_t *dets, int32_t cap_per_frame,
                           int32_t *counts, uint32_t *status);

/* Device-resident staging owned by the handle (used by benchmarks / streaming callers). */
int ck_upload_frames(ck_handle_t *h, const ck_image_u8_t *imgs, int32_t n);
int ck_detect_uploaded(ck_handle_t *h, int32_t n, ck_detection_t *dets, int32_t cap_per_frame,
                       int32_t *counts, uint32_t *status);

/* ---- stage entry points (parity tests + roofline measurement) ------------------------------------ */
/* thresh_out: [n][height][width] bytes in {0,127,255}.  Runs on frames staged by ck_upload_frames when
 * imgs == NULL. */
int ck_threshold_batch(ck_handle_t *h, const ck_image_u8_t *imgs, int32_t n, uint8_t *thresh_out);
/* labels_out: [n][height][width] u32, canonical label = smallest pixel index (y*width+x) of the
 * component, 0xFFFFFFFF for 127-pixels.  sizes_out (optional): component size at every pixel. */
int ck_segment_batch(ck_handle_t *h, const ck_image_u8_t *imgs, int32_t n, uint32_t *labels_out,
                     uint32_t *sizes_out);
/* Times only the threshold+segment kernels on the already-uploaded frames: runs them `iters` times on the
 * handle's stream between HIP events and returns the mean milliseconds per pass in *ms_out. */
int ck_time_threshold_segment(ck_handle_t *h, int32_t n, int32_t iters, float *ms_out);

/* ---- quad_sigma: Gaussian blur / sharpen of the quad image (AprilTag-3's detector field quad_sigma) -------------------------
 * sigma > 0 blurs the image the quad stages run on (the decimated frame D, or the frame itself at quad_decimate 1) with a
 * Gaussian of ksz taps, sigma < 0 sharpens it (clamp(2 D - blur, 0, 255)); |sigma| < 0.5 (ksz <= 1) is no filter at all, the
 * default.  Threshold, segmentation, clusters and the quad fit's gradient weights read the filtered image Q; edge refinement and
 * decode read the unfiltered frame at quad_decimate 2 and Q at quad_decimate 1 (upstream filters the caller's image in place
 * there; the library reproduces that result without writing to the caller's frame).  DESIGN.md §quad_sigma has the exact rule.
 * While the filter is on, ck_last_stage_ms().threshold and ck_time_threshold_segment include it, as they include decimation. */
/* The u8 weights of a sigma: pure host arithmetic, no device needed.  *ksz_out = taps (1: no filter, k_out untouched);
 * k_out[0..ksz) = the weights.  CK_EINVAL for NaN / inf, a null ksz_out, or (filter on) a null k_out or cap < ksz (*ksz_out is
 * set then); CK_EUNSUPPORTED for |sigma| > 8 (ksz > 33). */
int ck_quad_sigma_kernel(float sigma, uint8_t *k_out, int32_t cap, int32_t *ksz_out);
/* Sets the handle's quad_sigma; may be called at any time between calls (a batch already enqueued keeps the value it was
 * enqueued with).  At quad_decimate 1 the first value that turns the filter on allocates the quad-image buffer (one byte per
 * pixel per max_batch frame): CK_ENOMEM when that fails.  Errors as ck_quad_sigma_kernel; the handle keeps its value then. */
int ck_set_quad_sigma(ck_handle_t *h, float sigma);
/* out: [n][height / quad_decimate][width / quad_decimate] — the image the quad stages run on (Q; D when the filter is off).
 * Runs on frames staged by ck_upload_frames when imgs == NULL. */
int ck_quad_image_batch(ck_handle_t *h, const ck_image_u8_t *imgs, int32_t n, uint8_t *out);

/* Boundary points grouped in clusters.  A point packs x,y in half-pixel units and the gradient sign. */
typedef struct ck_cluster_point {
    uint16_t x, y;  /* half-pixel coordinates 2*px+dx, 2*py+dy */
    int8_t gx, gy;  /* sign of the black→white step along x / y, in {-1,0,1} */
    uint16_t pad;
} ck_cluster_point_t;
typedef struct ck_cluster {
    uint32_t rep0, rep1;  /* canonical labels of the two components, rep0 < rep1 */
    uint32_t start, count; /* range in the frame's point array */
} ck_cluster_t;
/* Emits clusters sorted by (rep0,rep1) and points sorted by emission order inside each cluster. */
int ck_clusters_batch(ck_handle_t *h, const ck_image_u8_t *imgs, int32_t n, ck_cluster_t *clusters,
                      int32_t cluster_cap, int32_t *n_clusters, ck_cluster_point_t *points,
                      int32_t point_cap, int32_t *n_points);

typedef struct ck_quad {
    double p[4][2];          /* corners in pixels, winding as fitted */
    int32_t reversed_border;
    uint32_t rep0, rep1;     /* cluster the quad came from */
} ck_quad_t;
/* Candidate quads after fit (+ edge refinement when enabled), sorted by (rep0,rep1). */
int ck_quads_batch(ck_handle_t *h, const ck_image_u8_t *imgs, int32_t n, ck_quad_t *quads,
                   int32_t quad_cap, int32_t *n_quads);
/* The decode stage alone, on the caller's quads: quads is [n][quad_stride], frame i decodes its first n_quads[i] entries
 * (p and reversed_border are read; rep0 / rep1 are not).  It reads the image ck_detect_*'s decode reads on this handle — the
 * frame, at either quad_decimate; the filtered frame while quad_sigma is on at quad_decimate 1 — and returns what ck_detect_*
 * returns: dets [n][cap_per_frame], counts[n], status[n] (may be NULL) with the decode stage's bits only
 * (CK_FRAME_DETS_OVERFLOW, CK_FRAME_UNVERIFIED_ID).  Runs on frames staged by ck_upload_frames when imgs == NULL.
 * CK_EINVAL for null pointers, negative counts, cap_per_frame < 1, an n_quads[i] above quad_stride or above the handle's
 * max_quads_per_frame (1024 by default), and n above what is staged; CK_ECAPACITY for more host frames than max_batch (as
 * ck_upload_frames).  A quad that decodes but whose centre or a corner is not finite (three collinear corners put a tag corner at
 * infinity) leaves no detection. */
int ck_decode_quads_batch(ck_handle_t *h, const ck_image_u8_t *imgs, int32_t n, const ck_quad_t *quads,
                          int32_t quad_stride, const int32_t *n_quads, ck_detection_t *dets,
                          int32_t cap_per_frame, int32_t *counts, uint32_t *status);

/* per-stage timings of the last ck_detect_* call, milliseconds (HIP events on the handle's stream) */
typedef struct ck_stage_ms {
    float h2d, threshold, segment, clusters, quads, decode, d2h, total;
} ck_stage_ms_t;
int ck_last_stage_ms(ck_handle_t *h, ck_stage_ms_t *out);

/* ---- CAT: chalkydri-apriltags experimental detector front-end --------------------------------------- */
/* Classes are the reference's `Color` enum: 0 Black, 1 White, 2 Other (src/utils.rs:1-6). */
/* calc_otsu on an RGB8 frame [h][w][3] (lib.rs:191-259). classes_out: [h][w]. */
int ck_cat_calc_otsu(ck_handle_t *h, const uint8_t *rgb, int32_t width, int32_t height,
                     uint8_t *classes_out);
/* thresh(): fixed <60 / >160 split (lib.rs:319-334). */
int ck_cat_thresh(ck_handle_t *h, const uint8_t *rgb, int32_t width, int32_t height,
                  uint8_t *classes_out);
/* detect_corners over a class map (lib.rs:291-309,345-400); points in the reference's x-major order. */
int ck_cat_detect_corners(ck_handle_t *h, const uint8_t *classes, int32_t width, int32_t height,
                          uint32_t *points_xy, int32_t cap, int32_t *n_points);
/* check_edges (lib.rs:409-499): lines (x1,y1,x2,y2) in the reference's push order. */
int ck_cat_check_edges(ck_handle_t *h, const uint8_t *classes, int32_t width, int32_t height,
                       const uint32_t *points_xy, int32_t n_points, uint32_t *lines_xyxy, int32_t cap,
                       int32_t *n_lines);
/* connected_components (lib.rs:501-549): canonical root (min index) and component size per pixel;
 * pixels of class Other and never-visited pixels are their own singleton sets, as in UnionFind::new. */
int ck_cat_connected_components(ck_handle_t *h, const uint8_t *classes, int32_t width, int32_t height,
                                uint32_t *roots_out, uint32_t *sizes_out);
/* process_frame = calc_otsu → detect_corners → check_edges (lib.rs:265-287). Returns CK_EINVAL when
 * rgb_len != width*height*3 (the reference asserts). */
int ck_cat_process_frame(ck_handle_t *h, const uint8_t *rgb, size_t rgb_len, int32_t width,
                         int32_t height, uint8_t *classes_out, uint32_t *points_xy, int32_t point_cap,
                         int32_t *n_points, uint32_t *lines_xyxy, int32_t line_cap, int32_t *n_lines);

/* ---- CAT: iterative tri-class Otsu threshold, batched -------------------------------------------------------------------
 * The threshold the CAT design document asks for (book/src/maintenance/apriltags.md:33), after Cai, Yang, Cao, Xia and Xu,
 * "A new iterative triclass thresholding technique in image segmentation" (IEEE TIP 2014), restated in integers; DESIGN.md §4h is
 * the contract.  Per frame: hist[g] counts the pixels of gray level g = grayscale(r, g, b) (utils.rs:33-46; a 1-channel pixel v is
 * grayscale(v, v, v)).  The state is an inclusive interval [lo, hi] = [0, 255] of levels still to be determined.  Round k:
 *   1. N = sum hist[g], S = sum g hist[g] over [lo, hi] (int64); fewer than two occupied levels there: stop, no threshold
 *   2. T_k = the smallest t in lo..hi-1 with the strictly greatest v(t) = (d d) / ((double)n (double)(N - n)), d = (double)(S n - N s),
 *      n = sum_{g<=t} hist[g], s = sum_{g<=t} g hist[g] inside the interval, among the t with n > 0 and N - n > 0; two
 *      multiplications and one division in double, in that order, not contracted; S n - N s in 64-bit two's complement
 *   3. lo' = ceil(s / n), hi' = floor((S - s) / (N - n)) at t = T_k: levels below the lower class mean are Black, above the upper White
 *   4. k >= 2 and |T_k - T_{k-1}| < min_delta: adopt [lo', hi'] and stop; k == max_iters: adopt and stop; lo' > hi': stop without
 *      adopting; otherwise adopt and go on
 * lut[g]: Black below lo_final, White above hi_final; inside the final interval Other (keep_tbd = 1) or Black up to T_last and White
 * above it (keep_tbd = 0).  A frame with fewer than two occupied levels has no threshold: lut[g] = g < 128 ? Black : White for both
 * values of keep_tbd, n_rounds 0, T_last -1, the interval [0, 255], CK_TRI_FLAT set. */
#define CK_TRI_MAX_ROUNDS 32
#define CK_TRI_FLAT 1 /* ck_tri_otsu_info_t.flags: fewer than two occupied gray levels */
typedef struct ck_tri_otsu_params {
    int32_t max_iters; /* 1..32, default 8 */
    int32_t min_delta; /* 1..255, default 1: stop when T repeats */
    int32_t keep_tbd;  /* 0 / 1, default 1 */
    int32_t channels;  /* 1 or 3, default 3 */
} ck_tri_otsu_params_t;
typedef struct ck_tri_otsu_info {
    int32_t n_rounds;                     /* rounds that produced a threshold */
    int32_t T[CK_TRI_MAX_ROUNDS];         /* T_1 .. T_n_rounds, -1 past the end */
    int32_t T_last, lo_final, hi_final;
    uint32_t n_black, n_white, n_other;   /* sum of hist[g] over the levels of each class */
    uint32_t flags;
} ck_tri_otsu_info_t;
void ck_tri_otsu_params_default(ck_tri_otsu_params_t *p);
/* Host arithmetic, no device needed: the record and the table lut[256] of one histogram hist[256].  CK_EINVAL: a null pointer, a
 * parameter out of range. */
int ck_tri_otsu_solve(const ck_tri_otsu_params_t *p, const uint32_t *hist, ck_tri_otsu_info_t *info, uint8_t *lut);
/* n dense frames px [n][height][width][channels] -> classes_out [n][height][width] on the handle's stream: a histogram pass, one
 * wave per frame that produces exactly the bytes of ck_tri_otsu_solve, and a look-up pass.  info_out [n] and hist_out [n][256] may
 * be NULL.  Every pointer may be a host or a device pointer; arrays on the handle's device are used in place.  n is not bound to
 * max_batch and the geometry not to the handle's; the staged frames and the detection workspace stay as they are.  Returns when the
 * outputs are complete.  CK_EINVAL: a null h, p, px or classes_out, n < 0, width or height < 1, width * height >= 2^31, a parameter
 * out of range.  CK_ENOMEM: the workspace (allocated by the first call, grown on demand; ck_create allocates none of it) could not
 * grow. */
int ck_cat_tri_otsu_batch(ck_handle_t *h, const ck_tri_otsu_params_t *p, const uint8_t *px, int32_t n, int32_t width, int32_t height,
                          uint8_t *classes_out, ck_tri_otsu_info_t *info_out, uint32_t *hist_out);
/* One RGB8 frame with the default parameters: drops into the place of ck_cat_calc_otsu. */
int ck_cat_tri_otsu(ck_handle_t *h, const uint8_t *rgb, int32_t width, int32_t height, uint8_t *classes_out);

/* ---- SQPnP ------------------------------------------------------------------------------------------ */
/* Isometry = translation + unit quaternion (w,x,y,z), matching nalgebra's Isometry3<f64> content. */
typedef struct ck_iso3 {
    double t[3];
    double q[4]; /* w, x, y, z */
} ck_iso3_t;

typedef struct ck_sqpnp_params {
    int32_t max_iter;  /* 15  (lib.rs:203) */
    double tol_sq;     /* 1e-16 (lib.rs:204); SqPnP::tolerance(t) sets t*t (lib.rs:219-222) */
} ck_sqpnp_params_t;

/* One solve_robot_pose problem (lib.rs:297-304). tags[] / bearings[] live in caller-provided arrays. */
typedef struct ck_sqpnp_problem {
    int32_t n_tags;            /* points_isometry.len() */
    int32_t n_bearings;        /* points_2d.len(); must equal 4*n_tags for a solve (lib.rs:255) */
    int32_t tag_offset;        /* first tag of this problem in the tags[] array */
    int32_t bearing_offset;    /* first bearing in the bearings[] array (3 doubles each) */
    ck_iso3_t robot_to_cam;
    double gyro;
    double sign_change_error;  /* 600.0 at the reference call site (apriltags/src/lib.rs:6,337) */
} ck_sqpnp_problem_t;

typedef struct ck_sqpnp_result {
    int32_t valid;         /* 0 = the reference would return None */
    int32_t pad;
    double rot[9];         /* pivoted robot rotation, row-major 3x3 */
    double pos[3];         /* pivoted robot position */
    double std_devs[3];
    double yaw;            /* euler_angles().2 of rot — what the caller publishes (apriltags/src/lib.rs:343) */
    double energy;         /* pure geometric energy r^T Omega r of the chosen candidate */
} ck_sqpnp_result_t;

void ck_sqpnp_params_default(ck_sqpnp_params_t *p);
int ck_sqpnp_solve_batch(ck_handle_t *h, const ck_sqpnp_params_t *params,
                         const ck_sqpnp_problem_t *problems, int32_t n, const ck_iso3_t *tags,
                         int32_t n_tags_total, const double *bearings, int32_t n_bearings_total,
                         ck_sqpnp_result_t *out);
/* SqPnP::create_solver_camera_transform (lib.rs:430-461); pure host arithmetic, no device needed. */
void ck_sqpnp_create_solver_camera_transform(double fwd_m, double left_m, double up_m, double roll_deg,
                                             double pitch_deg, double yaw_deg, ck_iso3_t *out);

/* ---- glue: AprilTags::process ------------------------------------------------------------------------ */
typedef struct ck_opencv5 {
    double fx, fy, cx, cy, k1, k2, p1, p2, k3;
} ck_opencv5_t;

/* The 64-byte record whacknet puts on the wire (crates/whacknet/src/lib.rs:43-66). */
typedef struct ck_vision_measurement {
    double pose_x, pose_y, pose_rot;
    double std_x, std_y, std_rot;
    uint64_t ts;
    uint8_t camera_id;
    uint8_t tag_count;
    uint8_t reserved[6];
} ck_vision_measurement_t;

typedef struct ck_field_tag {
    int32_t id;
    int32_t pad;
    ck_iso3_t pose;
} ck_field_tag_t;

typedef struct ck_process_params {
    ck_opencv5_t cam;
    ck_iso3_t robot_to_cam;
    const ck_field_tag_t *field;   /* known field tags (field.json) */
    int32_t n_field;
    uint8_t camera_id;
    double sign_change_error;
    ck_sqpnp_params_t sqpnp;
    int32_t allow_unverified_ids;  /* 0 (default): detections with id >= their family's n_upstream never reach the solver */
} ck_process_params_t;

/* detect → known-tag filter → unproject → solve_robot_pose → measurement, per frame.
 * gyro[n]: heading per frame; has_gyro[n] == 0 reproduces the "no gyro, no solve" gate (lib.rs:330).
 * out[i].tag_count = number of ALL detections in the frame (lib.rs:354); frames without a pose get a
 * zeroed record with tag_count 0 (lib.rs:365-376). */
int ck_process_batch_device(ck_handle_t *h, const uint8_t *d_frames, int32_t n, int32_t stride,
                            int64_t frame_pitch, const ck_process_params_t *pp, const double *gyro,
                            const uint8_t *has_gyro, ck_vision_measurement_t *out, int32_t *valid);
int ck_process_uploaded(ck_handle_t *h, int32_t n, const ck_process_params_t *pp, const double *gyro,
                        const uint8_t *has_gyro, ck_vision_measurement_t *out, int32_t *valid);

/* ---- ingest ring: pinned host slots + asynchronous upload ---------------------------------------------------------------
 * What the reference's camera layer hands the detector is a pooled host buffer per frame {buf,width,height,stride} in one
 * of the 8-bit-luma formats (crates/chalkydri/src/cameras/gst_to_cu.rs:49-72,131-188; fourcc GREY/GRAY/Y800, or the Y
 * plane that leads NV12/NV21/I420/YV12).  A ring owns `n_slots` pinned host buffers and as many device buffers of
 * max_batch frames each: the caller writes frames into a slot, submits it (one asynchronous copy on the ring's copy
 * stream) and processes it; submitting slot k+1 before processing slot k overlaps the upload with the compute. */
typedef struct ck_ingest ck_ingest_t;
int ck_ingest_create(ck_handle_t *h, int32_t n_slots, ck_ingest_t **out);
void ck_ingest_destroy(ck_ingest_t *ing);
int32_t ck_ingest_stride(const ck_ingest_t *ing);                                  /* row stride of a slot frame, bytes */
uint8_t *ck_ingest_frame(ck_ingest_t *ing, int32_t slot, int32_t index);           /* pinned host memory of one frame */
/* stride-aware copy of a caller frame into the slot; fourcc as four ASCII bytes, little-endian ("GREY" = 0x59455247) */
int ck_ingest_write(ck_ingest_t *ing, int32_t slot, int32_t index, const ck_image_u8_t *img, uint32_t fourcc);
int ck_ingest_submit(ck_ingest_t *ing, int32_t slot, int32_t n);
/* n = frames the output (and gyro) arrays hold; CK_EINVAL unless it is the count the slot was submitted with */
int ck_detect_ingested(ck_ingest_t *ing, int32_t slot, int32_t n, ck_detection_t *dets, int32_t cap_per_frame,
                       int32_t *counts, uint32_t *status);
int ck_process_ingested(ck_ingest_t *ing, int32_t slot, int32_t n, const ck_process_params_t *pp, const double *gyro,
                        const uint8_t *has_gyro, ck_vision_measurement_t *out, int32_t *valid);

/* ---- per-tag pose: AprilTag-3's estimate_tag_pose ----------------------------------------------------------------------
 * The pose of each single tag relative to the camera: homography -> orthogonal iteration (Lu, Hager & Mjolsness) -> second
 * local minimum (Schweighofer & Pinz) -> the lower object-space error first.  One fp64 lane per detection on the handle's
 * stream; nothing is computed on the host.  DESIGN.md §Per-tag pose has the exact contract.  Tag frame: object corners
 * s*(-1,1,0), s*(1,1,0), s*(1,-1,0), s*(-1,-1,0) in ck_detection_t's corner order, s = tagsize / 2. */
typedef struct ck_tag_pose_params {
    ck_opencv5_t cam;                  /* fx, fy, cx, cy, k1, k2, p1, p2, k3; all-zero distortion = AprilTag-3's pinhole */
    double tagsize[CK_MAX_FAMILIES];   /* edge of the black square in metres, by ck_detection_t.family */
    int32_t n_iters;                   /* orthogonal-iteration steps per minimum: 50, as estimate_tag_pose */
    int32_t pad;
} ck_tag_pose_params_t;

typedef struct ck_tag_pose {
    int32_t id, family;                /* copied from the detection */
    int32_t valid;                     /* 0: no pose (degenerate input); every other field but id / family is then 0 */
    int32_t has_alt;                   /* a second local minimum was found */
    double R[9];                       /* tag -> camera, row-major; camera x right, y down, z forward */
    double t[3];                       /* tag centre in camera coordinates, metres */
    double err;                        /* object-space error of (R, t) */
    double R_alt[9], t_alt[3];         /* the other minimum (zero when has_alt == 0) */
    double err_alt;                    /* +inf when has_alt == 0 */
    double H[9];                       /* pixel homography, tag square (the object corners / s) -> image, H[8] = 1 */
} ck_tag_pose_t;

/* n_iters 50, every tagsize 0.1651 (the reference's TAG_SIZE, chalkydri_sqpnp/src/lib.rs:38), cam all zero */
void ck_tag_pose_params_default(ck_tag_pose_params_t *pp);
/* Poses of caller detections: out[i] for dets[i].  dets and out may be host or device pointers (hipMemcpyDefault, as
 * ck_process_* accepts).  CK_EINVAL: a null pointer, n < 0, fx / fy not finite or <= 0, cx / cy / a distortion coefficient
 * not finite, a tagsize of one of the handle's families not finite or <= 0, n_iters outside 1..1000.
 * CK_ECAPACITY: n > max_batch * 256 (the per-frame detection capacity).  The first call that needs them allocates the
 * device buffers of the pose records (CK_ENOMEM when that fails); ck_create allocates nothing for them. */
int ck_estimate_tag_poses(ck_handle_t *h, const ck_tag_pose_params_t *pp, const ck_detection_t *dets, int32_t n,
                          ck_tag_pose_t *out);
/* Poses of the detections the handle's last ck_detect_batch / ck_detect_batch_device / ck_detect_uploaded /
 * ck_detect_ingested / ck_process_* call produced.  Those detections are still on the device, so only the pose records cross
 * the bus.  out is [n][cap_per_frame] and counts[n] gets min(detections, cap_per_frame), the truncation ck_detect_* applies,
 * with n = the frames of that call; the entries of a frame past its count are zero records.  out and counts may be host or
 * device pointers.  Errors as ck_estimate_tag_poses, and CK_EINVAL for cap_per_frame < 1 or when the detection workspace
 * holds no such call's result: no detect / process call since ck_create, a failed one, or a later call that rewrote the
 * workspace: ck_clusters_batch, ck_quads_batch and ck_decode_quads_batch.  ck_upload_frames, ck_upload_raw, ck_upload_raw_device, ck_raw_luma_batch, ck_threshold_batch, ck_segment_batch,
 * ck_quad_image_batch, ck_time_threshold_segment, ck_set_quad_sigma, ck_sqpnp_solve_batch, ck_gather_poses, ck_preview_jpeg,
 * ck_preview_luma, the ck_preview_*color* calls, ck_exposure_stats, ck_exposure_stats_ingested, ck_corner_subpix, ck_set_corner_subpix,
 * ck_board_corners_last, the ck_cat_*
 * calls (ck_cat_tri_otsu and ck_cat_tri_otsu_batch among them) and the ck_ingest_write / ck_ingest_submit calls leave it as it is. */
int ck_last_tag_poses(ck_handle_t *h, const ck_tag_pose_params_t *pp, ck_tag_pose_t *out, int32_t cap_per_frame,
                      int32_t *counts);

/* ---- baseline JPEG (MJPEG) luma decode on the device ---------------------------------------------------------------------
 * What the reference's camera layer would hand a `jpegdec` element (crates/chalkydri/src/cameras/pipeline.rs:43-44,123-124):
 * one complete JPEG per frame.  The library decodes its luma on the device into the handle's staged frames, bit-identical to
 * libjpeg's integer ("islow") IDCT — what a grayscale decode by libjpeg returns.  Supported: SOF0, and SOF1 at 8-bit precision,
 * Huffman coded, one interleaved scan; 1 component, or 3 with Y first; Y sampling 1x1, 2x1, 1x2 or 2x2 with chroma at 1x1; DRI
 * present or absent; 8- or 16-bit DQT; no DHT = the standard tables of ITU-T T.81 Annex K.3 (the UVC / AVI1 MJPEG convention).
 * DESIGN.md §4c has the stages.  Workspace (allocated by the first JPEG call, grown on demand; ck_create allocates none of it):
 * per frame of a call, the compressed bytes three times (pinned host staging, its device copy, the device's unstuffed copy),
 * a 48-byte record per 512 bits of scan plus one per restart interval, 4 bytes per restart interval, and the Y coefficients at
 * 2 bytes per pixel of the frame rounded up to whole 16 x 16 MCUs (2.0 MB for 1280 x 800). */
typedef struct ck_jpeg_frame {
    const uint8_t *data;     /* one complete JPEG (SOI..EOI) in host memory */
    int64_t size;
} ck_jpeg_frame_t;
typedef struct ck_jpeg_info {
    int32_t width, height, n_components;   /* 1 (grey) or 3 (Y first) */
    int32_t h_samp, v_samp;                /* Y's sampling factors = Hmax, Vmax in {1,2} */
    int32_t restart_interval;              /* MCUs, 0 = none */
    int32_t has_dht;                       /* 0: stream relies on the standard tables (UVC/AVI1 MJPEG convention) */
    int32_t pad;
} ck_jpeg_info_t;
/* per-frame jpeg_status bits */
enum {
    CK_JPEG_OK = 0,
    CK_JPEG_UNSUPPORTED = 1, /* a valid JPEG outside the supported subset (what ck_jpeg_info answers with CK_EUNSUPPORTED) */
    CK_JPEG_GEOMETRY = 2,    /* not the handle's width x height */
    CK_JPEG_CORRUPT = 4      /* invalid Huffman code, AC run past coefficient 63, an interval that ends before its MCUs do,
                              * a restart marker missing / out of sequence / in excess, or a header ck_jpeg_info refuses */
};
/* Parses markers up to SOS on the host (no device needed).  CK_OK, CK_EUNSUPPORTED (valid JPEG outside the supported subset:
 * progressive, lossless, arithmetic coding, 12-bit, more than one scan, other sampling factors, a scan without Y),
 * CK_EINVAL (null pointer, size < 4, not a JPEG, a truncated or inconsistent header). */
int ck_jpeg_info(const uint8_t *data, int64_t size, ck_jpeg_info_t *out);
/* Decodes the luma of n frames on the device into the handle's staged frames: after it, ck_detect_uploaded, ck_process_uploaded,
 * ck_time_threshold_segment and ck_last_tag_poses work exactly as after ck_upload_frames.  A frame that is unsupported, has the
 * wrong geometry or is corrupt is staged as all zeros and flagged in jpeg_status[n] (may be NULL); the call still returns CK_OK.
 * CK_EINVAL: null handle or frames, n < 0, a frame with a null data pointer or size < 4.  CK_ECAPACITY: n > max_batch.
 * CK_ENOMEM: the workspace could not grow.  Trailing bytes after the last MCU and after EOI are ignored. */
int ck_upload_jpeg(ck_handle_t *h, const ck_jpeg_frame_t *frames, int32_t n, uint32_t *jpeg_status);
/* The same, then copies the decoded luma out: luma_out is [n][height][width]. */
int ck_jpeg_luma_batch(ck_handle_t *h, const ck_jpeg_frame_t *frames, int32_t n, uint8_t *luma_out, uint32_t *jpeg_status);
/* JPEG frames turned by the camera's mounting (the reference's jpegdec -> videoflip, crates/chalkydri/src/cameras/pipeline.rs:123-162).
 * orientation is a CK_ORIENT_* value (below) and the handle's width x height the ORIENTED frame W x H, as for the raw formats: the
 * streams must be sw x sh as ck_raw_layout({GREY, orientation}, W, H) gives it (W x H for none and rotate-180, H x W for the
 * quarter turns), and with S the luma ck_upload_jpeg would stage for a stream, the staged frame is orient(S, orientation) by the four
 * formulas of the raw formats' contract below.  The IDCT kernel writes the turned blocks itself: no second pass over the frame.
 * CK_ORIENT_NONE is ck_upload_jpeg / ck_jpeg_luma_batch byte for byte.  A stream that is not sw x sh is CK_JPEG_GEOMETRY and staged
 * as zeros; the other status bits and the errors are ck_upload_jpeg's, and CK_EINVAL also for an orientation outside 0..3.
 * DESIGN.md §4c, "JPEG frames: orientation and the ring". */
int ck_upload_jpeg_oriented(ck_handle_t *h, const ck_jpeg_frame_t *frames, int32_t n, int32_t orientation, uint32_t *jpeg_status);
int ck_jpeg_luma_batch_oriented(ck_handle_t *h, const ck_jpeg_frame_t *frames, int32_t n, int32_t orientation, uint8_t *luma_out,
                                uint32_t *jpeg_status);
/* An ingest ring whose slots take JPEG frames: the asynchronous form of ck_upload_jpeg_oriented.  ck_ingest_create_jpeg allocates,
 * once, for every slot: the pinned staging and its device copy (max_batch regions of max_frame_bytes + the tables), the unstuffed
 * copy, the decode workspace at its worst case for sw x sh streams of max_frame_bytes (one 48-byte record per 512 bits of scan and
 * per 8 x 8 pixels, the Y coefficients) and the slot's device frames; ck_ingest_destroy releases them.  max_frame_bytes bounds one
 * frame's size; 0 = sw * sh, which no camera's JPEG of that size exceeds in practice — a caller that knows its camera's largest
 * frame saves memory by saying so.  CK_EINVAL: a null handle / out, n_slots outside 1..8, an orientation outside 0..3, a negative
 * max_frame_bytes.  CK_ENOMEM as ck_ingest_create.
 * ck_ingest_write_jpeg parses the header on the host and copies the scan into the slot's pinned staging; the caller's buffer is free
 * when it returns.  A stream that is unsupported, corrupt in its header or of the wrong geometry is not an error of the call: CK_OK,
 * and the frame comes out as zeros with its CK_JPEG_* bit, exactly as through ck_upload_jpeg.  CK_ECAPACITY: size > max_frame_bytes.
 * CK_EINVAL: a null pointer, size < 4, a slot or index out of range, a ring that is not a JPEG ring.
 * ck_ingest_submit(ing, slot, n) on a JPEG ring: CK_EINVAL unless every index in [0, n) has been written since the slot's last
 * submit; it merges the frames' tables, enqueues the copies, the decode and the oriented IDCT on the ring's copy stream into the
 * slot's device frames and records the slot's event, without allocating and without waiting for the device.  ck_detect_ingested /
 * ck_process_ingested then work as on every ring.  ck_ingest_jpeg_status waits for the slot's decode and gives the n status words
 * (n = the count the slot was submitted with, CK_EINVAL otherwise).
 * On a JPEG ring ck_ingest_write returns CK_EUNSUPPORTED, ck_ingest_frame NULL and ck_ingest_stride 0.
 * On EVERY kind of ring a slot must not be written again before the call that processes it (ck_detect_ingested,
 * ck_process_ingested) has returned: until then its staging may still be feeding the copy. */
int ck_ingest_create_jpeg(ck_handle_t *h, int32_t n_slots, int32_t orientation, int64_t max_frame_bytes, ck_ingest_t **out);
int ck_ingest_write_jpeg(ck_ingest_t *ing, int32_t slot, int32_t index, const uint8_t *data, int64_t size);
int ck_ingest_jpeg_status(ck_ingest_t *ing, int32_t slot, int32_t n, uint32_t *jpeg_status);
/* The colour form of the JPEG decode: the source of the colour preview for MJPEG cameras.  DESIGN.md §4i is the contract.
 * ck_upload_jpeg_color stages the luma exactly as ck_upload_jpeg_oriented does (the same bytes, the same statuses, the same errors)
 * and also keeps the Cb and Cr planes of the n frames on the device: per component the cw x ch plane, cw = ceil(sw / hs),
 * ch = ceil(sh / vs) for Y sampling hs x vs, from jpeg_idct_islow with the component's own quantisation table.  The planes are the
 * handle's colour source (ck_preview_jpeg_color, ck_preview_color) until any other call stages frames, the rule of the raw staging.
 * The frame of triples C (sh x sw) those calls orient, scale and encode: Y = the luma; Cb, Cr = libjpeg's fancy upsampling of the
 * plane P, in integers, with i = x >> 1, j = y >> 1:
 *   1x1  P[y][x]
 *   2x1  x even: x == 0 ? P[y][0] : (3 P[y][i] + P[y][i-1] + 1) >> 2;  x odd: x == 2cw-1 ? P[y][cw-1] : (3 P[y][i] + P[y][i+1] + 2) >> 2
 *   1x2  y even: (3 P[j][x] + P[max(j-1,0)][x] + 1) >> 2;              y odd: (3 P[j][x] + P[min(j+1,ch-1)][x] + 2) >> 2
 *   2x2  T[k] = 3 P[j][k] + P[jn][k], jn = max(j-1,0) for y even, min(j+1,ch-1) for y odd;
 *        x even: x == 0 ? (4 T[0] + 8) >> 4 : (3 T[i] + T[i-1] + 8) >> 4;  x odd: x == 2cw-1 ? (4 T[cw-1] + 7) >> 4 : (3 T[i] + T[i+1] + 7) >> 4
 * what libjpeg(-turbo) decodes to YCbCr.  A one-component stream has Cb = Cr = 128; a frame with a non-zero CK_JPEG_* status is
 * (0, 128, 128) everywhere.  Workspace beyond ck_upload_jpeg's (grown on demand; ck_create allocates none of it): 256 bytes of
 * chroma coefficients per MCU and 2 cw ch bytes of planes per frame.
 * ck_ingest_create_jpeg_color is ck_ingest_create_jpeg whose slots also keep their frames' chroma planes (sized once, for 1x1
 * sampling) until the slot is submitted again: the source of ck_preview_jpeg_color_ingested / ck_preview_color_ingested.  Writing,
 * submitting, the status and the detect / process calls are those of every JPEG ring. */
int ck_upload_jpeg_color(ck_handle_t *h, const ck_jpeg_frame_t *frames, int32_t n, int32_t orientation, uint32_t *jpeg_status);
int ck_ingest_create_jpeg_color(ck_handle_t *h, int32_t n_slots, int32_t orientation, int64_t max_frame_bytes, ck_ingest_t **out);

/* ---- raw camera formats and orientation on the device -------------------------------------------------------------------
 * What the reference does between the camera and AprilTags::process with `videoconvert` + a GRAY8 caps filter and `videoflip`
 * (crates/chalkydri/src/cameras/pipeline.rs:96-137): raw frames in one of the formats of its buffer layer
 * (crates/chalkydri/src/cameras/gst_to_cu.rs:152-188) become 8-bit luma, turned by the camera's mounting, on the device, straight
 * into the staged frames.  DESIGN.md §4d is the contract.  fourcc (four ASCII bytes, little-endian), minimum row stride, luma of
 * pixel x of a row r[]:
 *   GREY GRAY Y800 NV12 NV21 I420 YV12   sw             r[x]  (only the leading plane is read; with CK_RAW_PLANES below the
 *                                                             chroma planes of the last four are part of the frame)
 *   YUYV YUY2                            4*ceil(sw/2)   r[2x]
 *   UYVY                                 4*ceil(sw/2)   r[2x+1]
 *   RGB3 "RGB "  /  BGR3 "BGR "          3*sw           L(r[3x], r[3x+1], r[3x+2])  /  L(r[3x+2], r[3x+1], r[3x])
 *   RGBA  /  BGRA                        4*sw           L(r[4x], r[4x+1], r[4x+2])  /  L(r[4x+2], r[4x+1], r[4x]), alpha ignored
 * L(R,G,B) = (19595 R + 38470 G + 7471 B + 32768) >> 16: the JFIF luma in libjpeg's fixed point, the Y that ck_upload_jpeg
 * reproduces.  The Y byte of the YUV formats is copied as it is.  Any stride at or above the minimum, any base alignment; bytes
 * of a row beyond the minimum and the planes behind a luma plane are never read.
 * The handle's width x height is the ORIENTED frame W x H; the source is sw x sh = W x H (none, rotate-180) or H x W (the
 * quarter turns).  With S the source's luma: none out[y][x] = S[y][x]; clockwise out[y][x] = S[sh-1-x][y]; rotate-180
 * out[y][x] = S[sh-1-y][sw-1-x]; counterclockwise out[y][x] = S[x][sw-1-y]. */
enum {
    CK_ORIENT_NONE = 0,            /* the reference's VideoOrientation discriminants (chalkydri_core/src/config.rs:201-207) */
    CK_ORIENT_CLOCKWISE = 1,
    CK_ORIENT_ROTATE_180 = 2,
    CK_ORIENT_COUNTERCLOCKWISE = 3
};
/* Or-ed into ck_raw_format_t.orientation: the chroma planes behind the luma plane are part of every frame.  Only
 * NV12, NV21, I420 and YV12 take it (CK_EUNSUPPORTED with any other fourcc of the table), and with it they are four families.
 * The layout is V4L2's single-buffer one; with cw = ceil(sw / 2), ch = ceil(sh / 2) and a row stride `stride`:
 *   all four     luma row y at y * stride; min_stride = 2 cw; a frame extends stride * (sh + ch) bytes
 *   NV12 / NV21  one interleaved plane at stride * sh, ch rows of `stride` bytes, pair i of a row at bytes 2i, 2i + 1:
 *                (Cb, Cr) / (Cr, Cb)
 *   I420 / YV12  stride even (CK_EINVAL otherwise); Cb / Cr at stride * sh, ch rows of stride / 2 bytes; then Cr / Cb at
 *                stride * sh + (stride / 2) * ch
 * The triple of source pixel (x, y) is Y = luma[y][x], Cb = Cb[y >> 1][x >> 1], Cr = Cr[y >> 1][x >> 1]: the bytes unchanged,
 * chroma replicated, the rule of the 4:2:2 families.  Bytes of a row beyond what the plane holds (sw of luma, 2 cw of an
 * interleaved chroma row, cw of a split one) are never read.  What the flag switches on: ck_upload_raw / ck_raw_luma_batch copy
 * all planes (every image's buf spans stride * (sh + ch) bytes) and the colour and blob calls then work from the staging; the
 * *_device forms need frame_pitch >= stride * (sh + ch); a ring of ck_ingest_create_raw holds whole frames (ck_ingest_frame
 * points at sh + ch rows of ck_ingest_stride, ck_ingest_write copies all planes and takes the ring's own fourcc only).  The
 * staged luma and everything computed from it are those of the same call without the flag. */
#define CK_RAW_PLANES 0x100
/* orientation: CK_ORIENT_* in bits 0..1, optionally | CK_RAW_PLANES */
typedef struct ck_raw_format {
    uint32_t fourcc;
    int32_t orientation;
} ck_raw_format_t;
/* Host only (no device needed): the source geometry of an oriented width x height frame.  min_bytes = sh * min_stride; with
 * CK_RAW_PLANES min_stride = 2 cw and min_bytes = (sh + ch) * min_stride.
 * CK_EINVAL: a null pointer, width or height < 1, an orientation with a bit outside 0x103; CK_EUNSUPPORTED: a fourcc outside the
 * table, then CK_RAW_PLANES with a fourcc that has no chroma planes.  Every raw entry point validates its format through this. */
int ck_raw_layout(const ck_raw_format_t *fmt, int32_t width, int32_t height, int32_t *sw, int32_t *sh, int32_t *min_stride,
                  int64_t *min_bytes);
/* Host frames (width / height = sw / sh, stride in bytes) -> one pinned staging buffer -> one asynchronous copy -> the convert
 * kernel on the handle's stream -> the staged frames: after it ck_detect_uploaded, ck_process_uploaded,
 * ck_time_threshold_segment and ck_last_tag_poses work exactly as after ck_upload_frames.  Returns when the frames are staged.
 * Errors of ck_raw_layout, and CK_EINVAL: null handle / imgs / buffer, n < 0, a geometry that is not the one ck_raw_layout gives
 * for the handle, a stride below the minimum.  CK_ECAPACITY: n > max_batch.  CK_ENOMEM: the staging memory (pinned host + device,
 * n * sh rows of the minimum stride rounded up to 16; allocated by the first raw call, grown on demand; ck_create allocates none
 * of it) could not grow. */
int ck_upload_raw(ck_handle_t *h, const ck_image_u8_t *imgs, int32_t n, const ck_raw_format_t *fmt);
/* The same from device-resident frames (row y of frame f at d_raw + f * frame_pitch + y * stride), no host copy and no staging.
 * The caller's work on d_raw must have completed; the source may be reused when the call returns.  CK_EINVAL also for
 * frame_pitch < stride * sh (with CK_RAW_PLANES: stride * (sh + ch); the luma is staged, the planes are only validated). */
int ck_upload_raw_device(ck_handle_t *h, const uint8_t *d_raw, int32_t n, int32_t stride, int64_t frame_pitch,
                         const ck_raw_format_t *fmt);
/* As ck_upload_raw, then copies the oriented luma out: luma_out is [n][height][width]. */
int ck_raw_luma_batch(ck_handle_t *h, const ck_image_u8_t *imgs, int32_t n, const ck_raw_format_t *fmt, uint8_t *luma_out);
/* An ingest ring whose pinned slots hold RAW frames: ck_ingest_stride is the slot's raw row stride, ck_ingest_frame the raw
 * frame; ck_ingest_write takes exactly the fourccs of the ring's family (CK_EUNSUPPORTED otherwise) and sw x sh frames and copies
 * min_stride bytes per row; ck_ingest_submit enqueues the copy and the conversion on the ring's copy stream, so the slot's device
 * frames are oriented luma and ck_detect_ingested / ck_process_ingested work as on a ring of ck_ingest_create. */
int ck_ingest_create_raw(ck_handle_t *h, int32_t n_slots, const ck_raw_format_t *fmt, ck_ingest_t **out);
/* Host only: where the samples of a frame with CK_RAW_PLANES lie, for the source of an oriented width x height frame at row stride
 * `stride`.  Component c (0 Y, 1 Cb, 2 Cr) of source pixel (x, y) is the byte at offset[c] + (y >> (c ? 1 : 0)) * row_stride[c] +
 * (x >> (c ? 1 : 0)) * step[c].  Errors of ck_raw_layout; CK_EUNSUPPORTED without the flag; CK_EINVAL for a null out, a stride
 * below 2 cw, or an odd stride with I420 / YV12. */
typedef struct ck_raw_planes {
    int32_t sw, sh, cw, ch;
    int64_t offset[3];      /* byte of the first Y, Cb, Cr sample from the frame's start */
    int32_t row_stride[3];  /* bytes between rows of that component */
    int32_t step[3];        /* bytes between samples of a row: 1,2,2 for NV12/NV21; 1,1,1 for I420/YV12 */
    int32_t pad[2];
    int64_t bytes;          /* stride * (sh + ch) */
} ck_raw_planes_t;
int ck_raw_plane_layout(const ck_raw_format_t *fmt, int32_t width, int32_t height, int32_t stride, ck_raw_planes_t *out);
/* Host only: the triples (Y, Cb, Cr) of n frames turned by the format's orientation, ycc_out [n][H][W][3]: the one-thread C twin of
 * ck_preview_color at width = W, height = H, overlay = 0, for every colour source a raw format can name (the packed families by
 * the formulas of the colour preview below, the planar ones with CK_RAW_PLANES).  imgs as ck_upload_raw takes them.  Errors of
 * ck_raw_layout; CK_EUNSUPPORTED: a luma-first fourcc without the flag; CK_EINVAL: null imgs / buffer / ycc_out, n < 0, an image
 * that is not sw x sh or whose stride the format cannot have. */
int ck_raw_ycc_host(const ck_raw_format_t *fmt, const ck_image_u8_t *imgs, int32_t n, int32_t W, int32_t H, uint8_t *ycc_out);

/* ---- JPEG preview of the staged frames, encoded on the device -------------------------------------------------------------
 * The way back of the camera layer: what the reference's driver-station stream does with videoconvertscale (nearest neighbour,
 * 640 x 480) and turbojpeg::compress(quality 50) (crates/chalkydri/src/cameras/mjpeg.rs:30-51,108-128), on the staged frames
 * (whatever staged them: ck_upload_frames, ck_upload_jpeg, ck_upload_raw*), so that only compressed bytes cross the bus.
 * DESIGN.md §4e is the contract.  Per frame F (W x H, the handle's geometry):
 *   scale    P[y][x] = F[(2y+1) H / (2 ph)][(2x+1) W / (2 pw)] in integers (pw = W, ph = H is the identity);
 *   overlay  (overlay = 1) the outlines of the detections the handle's last ck_detect_* / ck_process_* call left on the device
 *            for frame index frames[i] of that call: corner (px, py) -> pixel ((int)floor(px * pw / W), (int)floor(py * ph / H))
 *            in double, clamped to the preview; edges corner k -> (k+1) mod 4 by the integer Bresenham line of §4e; every line
 *            pixel of the frame forms a mask first, then P = P < 128 ? 255 : 0 where the mask is set;
 *   encode   a 1-component baseline JPEG exactly as libjpeg writes it (jpeg_fdct_islow, jpeg_set_quality(quality, baseline),
 *            Annex-K luminance Huffman tables, JFIF 1.01 header, DRI = restart_rows * ceil(pw / 8) when restart_rows > 0):
 *            the file equals libjpeg(-turbo)'s byte for byte.
 * width / height: 0 = W / H; larger than W / H is clipped to it (the library never enlarges); below 8 or negative is CK_EINVAL. */
typedef struct ck_preview_params {
    int32_t width, height;   /* preview size */
    int32_t quality;         /* 1..100 */
    int32_t restart_rows;    /* block rows per restart interval, 0 = no restart markers */
    int32_t overlay;         /* 0 / 1 */
    int32_t pad;
} ck_preview_params_t;
/* per-frame preview status bits */
enum {
    CK_PREVIEW_OK = 0,
    CK_PREVIEW_TRUNCATED = 1 /* the file did not fit cap_per_frame: sizes[i] is the size it needs */
};
/* 640 x 480, quality 50, no restart markers, no overlay: the reference's stream (mjpeg.rs:41-49,116) */
void ck_preview_params_default(ck_preview_params_t *pp);
/* Host only (no device needed): validates pp against a W x H handle geometry and resolves the preview size; max_bytes = an
 * upper bound of a file's size (a baseline block is at most 264 bytes before byte stuffing).  pw, ph, max_bytes may be NULL.
 * CK_EINVAL: a null pp, W or H < 1, width or height negative or (after resolving) below 8, quality outside 1..100,
 * restart_rows < 0 or restart_rows * ceil(pw / 8) > 65535.  Every preview entry point validates through this. */
int ck_preview_layout(const ck_preview_params_t *pp, int32_t W, int32_t H, int32_t *pw, int32_t *ph, int64_t *max_bytes);
/* Encodes n staged frames.  frames: n indices into the staged frames of the last upload (NULL = 0..n-1; an index may repeat).
 * out: [n][cap_per_frame], a host or a device pointer; sizes[n]: the size of every file; status[n] (may be NULL): CK_PREVIEW_*.
 * A file that does not fit cap_per_frame writes nothing past its slot, reports the size it needs and CK_PREVIEW_TRUNCATED; the
 * call still returns CK_OK.  Only the sizes and the bytes used are copied to a host `out`.  Runs on the handle's stream after
 * whatever was enqueued, returns when the files are complete, and leaves the staged frames and the detection workspace as they
 * are.  CK_EINVAL: a null handle / pp / out / sizes, n < 0, cap_per_frame < 1, an index outside the staged frames, what
 * ck_preview_layout refuses, and with overlay = 1: no valid detection result on the handle (ck_last_tag_poses' rule) or an
 * index that call did not cover.  CK_ECAPACITY: n > max_batch.  CK_ENOMEM: the workspace (allocated by the first preview call,
 * grown on demand; ck_create allocates none of it: per frame of a call 128 bytes of coefficients + 272 bytes of bit buffer per
 * 8 x 8 block of the preview, pw * ph / 8 bytes of mask, and the output staging) could not grow. */
int ck_preview_jpeg(ck_handle_t *h, const ck_preview_params_t *pp, const int32_t *frames, int32_t n, uint8_t *out,
                    int64_t cap_per_frame, int64_t *sizes, uint32_t *status);
/* The scaled (+ overlaid) pixels the encoder is given, out [n][ph][pw] (host or device pointer): for tests and for callers with
 * an encoder of their own.  quality and restart_rows are validated and otherwise unused.  Errors as ck_preview_jpeg. */
int ck_preview_luma(ck_handle_t *h, const ck_preview_params_t *pp, const int32_t *frames, int32_t n, uint8_t *out);

/* ---- the preview in colour, from the raw camera frames ---------------------------------------------------------------------
 * The reference's stream is a colour picture (videoconvertscale to RGB, turbojpeg::compress(.., PixelFormat::RGB, 50,
 * Subsamp::None): mjpeg.rs:41-49,108-118); the staged frames are luma, so the colour form reads the RAW frames they were made
 * from, while those are still on the device.  DESIGN.md §4g is the contract.  Sources: the packed colour families of
 * ck_raw_layout (YUYV / YUY2, UYVY, RGB3 / "RGB ", BGR3 / "BGR ", RGBA, BGRA) and NV12 / NV21 / I420 / YV12 with CK_RAW_PLANES
 * (their triple is stated there); a luma-first family (GREY .. YV12) without the flag is CK_EUNSUPPORTED: its chroma does not
 * reach the device, and ck_preview_jpeg serves it.  Per entry, with S the sh x sw source:
 *   orient   O[y][x] = the triple (Y, Cb, Cr) of the source pixel the index maps of ck_raw_format_t name.  RGB families: libjpeg's
 *            rgb_ycc_convert on R, G, B (alpha ignored), in 32-bit signed arithmetic:
 *              Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16          (the staged luma)
 *              Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
 *              Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16
 *            4:2:2 families: the bytes unchanged, Y = the pixel's luma byte, (Cb, Cr) = the U, V bytes of its pair x >> 1;
 *   scale    as ck_preview_jpeg, on O;
 *   overlay  the mask of ck_preview_jpeg; where it is set the triple of RGB (0, 255, 0): (150, 44, 21);
 *   encode   a three-component 4:4:4 interleaved baseline JPEG exactly as libjpeg writes it from YCbCr input: table 0 and the
 *            luminance Huffman tables for Y, the chrominance tables for Cb and Cr, DRI = restart_rows * ceil(pw / 8) MCUs.
 *            Pillow's save(quality, subsampling=0) of the RGB picture gives the same bytes.
 * out, cap_per_frame, sizes, status, CK_PREVIEW_TRUNCATED, the errors and the on-demand workspace (three times the blocks) are
 * ck_preview_jpeg's; `frames` indexes the RAW frames at hand.  No call touches the staged luma, the detection workspace or a ring
 * slot. */
/* ck_preview_layout with the colour file's upper bound.  Host only. */
int ck_preview_color_layout(const ck_preview_params_t *pp, int32_t W, int32_t H, int32_t *pw, int32_t *ph, int64_t *max_bytes);
/* From the raw frames the handle's last ck_upload_raw / ck_raw_luma_batch left in its raw staging, or from the frames of the last
 * ck_upload_jpeg_color (O = orient(C, orientation) of its triples C; `frames` indexes them).  Valid only while they are the
 * handle's staged frames: after any call that stages frames another way (ck_upload_frames, ck_upload_jpeg, ck_upload_jpeg_oriented,
 * ck_jpeg_luma_batch*, ck_upload_raw_device, the *_batch calls given images, the *_device calls) CK_EINVAL.  CK_EUNSUPPORTED: that
 * upload was of a luma-first family without CK_RAW_PLANES. */
int ck_preview_jpeg_color(ck_handle_t *h, const ck_preview_params_t *pp, const int32_t *frames, int32_t n, uint8_t *out,
                          int64_t cap_per_frame, int64_t *sizes, uint32_t *status);
/* From n_frames raw frames in the caller's device memory, laid out as ck_upload_raw_device takes them: any stride >= min_stride,
 * frame_pitch >= stride * sh (stride * (sh + ch) with CK_RAW_PLANES), any base alignment.  The work that produced them must have completed.  CK_EINVAL also for a null
 * d_raw / fmt, n_frames < 0, a stride or pitch below the minimum, an orientation out of range; CK_EUNSUPPORTED: the fourcc. */
int ck_preview_jpeg_color_device(ck_handle_t *h, const ck_preview_params_t *pp, const uint8_t *d_raw, int32_t stride,
                                 int64_t frame_pitch, const ck_raw_format_t *fmt, const int32_t *frames, int32_t n_frames, int32_t n,
                                 uint8_t *out, int64_t cap_per_frame, int64_t *sizes, uint32_t *status);
/* From the raw twin of a submitted slot of a ck_ingest_create_raw ring, or from the frames and chroma planes of a submitted slot of a
 * ck_ingest_create_jpeg_color ring (indices below the count the slot was submitted with; they are kept until the slot is submitted
 * again).  Waits for the slot like ck_exposure_stats_ingested and leaves it as it is.
 * CK_EUNSUPPORTED: a ring of ck_ingest_create or ck_ingest_create_jpeg. */
int ck_preview_jpeg_color_ingested(ck_ingest_t *ing, int32_t slot, const ck_preview_params_t *pp, const int32_t *frames, int32_t n,
                                   uint8_t *out, int64_t cap_per_frame, int64_t *sizes, uint32_t *status);
/* The triples (Y, Cb, Cr) the encoder is given, out [n][ph][pw][3] (host or device pointer), in the same three forms: for tests
 * and for callers with an encoder of their own.  quality and restart_rows are validated and otherwise unused. */
int ck_preview_color(ck_handle_t *h, const ck_preview_params_t *pp, const int32_t *frames, int32_t n, uint8_t *out);
int ck_preview_color_device(ck_handle_t *h, const ck_preview_params_t *pp, const uint8_t *d_raw, int32_t stride, int64_t frame_pitch,
                            const ck_raw_format_t *fmt, const int32_t *frames, int32_t n_frames, int32_t n, uint8_t *out);
int ck_preview_color_ingested(ck_ingest_t *ing, int32_t slot, const ck_preview_params_t *pp, const int32_t *frames, int32_t n,
                              uint8_t *out);

/* ---- exposure metering of the staged frames on the device ---------------------------------------------------------------
 * The camera-side loop the reference leaves open (Camera.auto_exposure / manual_exposure, crates/chalkydri_core/src/config.rs:64-65;
 * the commented-out V4L2 controls of crates/chalkydri/src/cameras/pipeline.rs:237-245; the stub crate crates/aaec): gradient-based
 * metering with a gamma sweep, after Shim, Lee and Kweon (2014).  The device re-renders every staged frame under CK_EXPOSURE_GAMMAS
 * gamma curves and histograms the Sobel gradient magnitude of each; the host turns the histograms into the gamma that carries the
 * most gradient information and scales the caller's exposure by it.  Everything the device produces is an integer.  DESIGN.md §4f
 * is the contract.  Per selected frame F (W x H) and rectangle R (clamped to the frame; NULL = the frame; empty = all-zero stats):
 *   luma[v]      pixels of R with F = v; n_luma = |R|
 *   I_k          lut[k][F], lut = ck_exposure_luts(p)
 *   Gx, Gy       the 3 x 3 Sobel pair on I_k (weights 1 2 1, not normalised): |Gx|, |Gy| <= 1020
 *   bin          floor(sqrt(Gx^2 + Gy^2)) >> 3, 0..180, the floor exact
 *   grad[k][bin] pixels of R intersected with [1, W-1) x [1, H-1): neighbours outside R are read; n_grad = that area */
#define CK_EXPOSURE_GAMMAS 7
#define CK_EXPOSURE_BINS 192 /* bins 0..180 are reachable */
typedef struct ck_rect {
    int32_t x0, y0, x1, y1;  /* half-open: x0 <= x < x1, y0 <= y < y1 */
} ck_rect_t;
typedef struct ck_exposure_stats {
    uint32_t luma[256];
    uint32_t grad[CK_EXPOSURE_GAMMAS][CK_EXPOSURE_BINS];
    uint32_t n_luma, n_grad;
    uint32_t pad[2];
} ck_exposure_stats_t;
typedef struct ck_exposure_params {
    double gamma[CK_EXPOSURE_GAMMAS]; /* strictly increasing, all > 0; default 1/1.9, 1/1.5, 1/1.2, 1, 1.2, 1.5, 1.9 */
    double lambda, delta;             /* the metric's weight W(m); default 1000, 0.06 */
    double kp;                        /* gain of the recommendation; default 1 */
    double e_min, e_max;              /* clamp of the recommendation; default 1e-6, 1e6 */
} ck_exposure_params_t;
/* Host arithmetic, no device needed.  CK_EINVAL from all of them: a null pointer, a parameter that is not finite, a gamma, lambda,
 * kp, e_min or e_max <= 0, gammas not strictly increasing, delta outside [0, 1), e_min > e_max.
 *   ck_exposure_luts       lut[k][v] = floor(255 (v / 255)^gamma[k] + 0.5), lut[k][0] = 0, lut[k][255] = 255, identity at gamma 1
 *   ck_exposure_metric     m[k] = (1 / n_grad) sum_b grad[k][b] W(b / 180) in ascending b, W(x) = log(lambda (x - delta) + 1) /
 *                          log(lambda (1 - delta) + 1) for x >= delta, else 0; n_grad = 0 gives 0
 *   ck_exposure_recommend  k* = first index of the largest m; gamma_hat = gamma[k*] at an end index, else the vertex of the parabola
 *                          through (ln gamma[j], m[j]), j = k*-1..k*+1, clamped to [gamma[k*-1], gamma[k*+1]] (gamma[k*] when the
 *                          second difference is zero); all m equal gives 1.  next = clamp(exposure gamma_hat^-kp, e_min, e_max):
 *                          a best gamma below 1 means the frame wants brightening.  exposure must be finite and > 0; its unit is
 *                          the caller's.  gamma_hat may be NULL. */
void ck_exposure_params_default(ck_exposure_params_t *p);
int ck_exposure_luts(const ck_exposure_params_t *p, uint8_t *lut);
int ck_exposure_metric(const ck_exposure_params_t *p, const ck_exposure_stats_t *s, double *m);
int ck_exposure_recommend(const ck_exposure_params_t *p, const ck_exposure_stats_t *s, double exposure, double *next,
                          double *gamma_hat);
/* Meters n staged frames (whatever staged them) in one pass on the handle's stream.  frames: n indices into the staged frames
 * (NULL = 0..n-1; an index may repeat); roi: n rectangles or NULL; out: n records in host memory.  Returns when they are complete
 * and leaves the staged frames and every detector buffer as they are.  CK_EINVAL: a null handle / p / out, n < 0, an index
 * outside the staged frames, params the host functions refuse.  CK_ECAPACITY: n > max_batch.  CK_ENOMEM: the workspace (n records
 * and the tables on the device, n records of pinned host memory; allocated by the first call, grown on demand; ck_create allocates
 * none of it) could not grow. */
int ck_exposure_stats(ck_handle_t *h, const int32_t *frames, int32_t n, const ck_exposure_params_t *p, const ck_rect_t *roi,
                      ck_exposure_stats_t *out);
/* The same on the frames of a submitted slot of an ingest ring of any kind (indices below the count the slot was submitted with);
 * waits for the slot's upload like ck_detect_ingested, and leaves the slot as it is: ck_detect_ingested may follow. */
int ck_exposure_stats_ingested(ck_ingest_t *ing, int32_t slot, const int32_t *frames, int32_t n, const ck_exposure_params_t *p,
                               const ck_rect_t *roi, ck_exposure_stats_t *out);

/* ---- camera calibration: intrinsics from board points, batched Levenberg-Marquardt ---------------------------------------
 * What the reference's configurator computes with `Calibrator::calibrate` (crates/configurator/src/calibration.rs:110-143): the
 * nine OpenCVModel5 parameters of a camera and one board pose per frame from point correspondences of a planar board.  The solver
 * takes correspondences, not frames; one problem calibrates one camera, and a batch of problems (leave-frames-out subsets of one
 * capture, say) is solved in one call, one workgroup per problem.  DESIGN.md §4j is the contract: the forward model is the one
 * ck_unproject_opencv5 inverts, poses are kept as rotation matrices and updated through the Cayley map, and the whole solve uses
 * only + - * / sqrt on doubles in a fixed order, so ck_calib_refine_host and ck_calib_refine_batch return the same bytes.
 * Shared arrays of a call: board_xy [n_points_total][2] (metres, board plane, Z = 0), image_uv [n_points_total][2] (pixels),
 * frame_start [n_starts_total] and the pose arrays [n_frames_total][12] (R row-major board -> camera, then t).  Frame f of a problem
 * owns the points point_offset + frame_start[start_offset + f] .. point_offset + frame_start[start_offset + f + 1] and the pose
 * pose_offset + f. */
enum {
    CK_CALIB_CONVERGED = 0,  /* an accepted step lowered the cost by at most 1e-14 of it, or the cost fell below 1e-20 */
    CK_CALIB_STALLED = 1,    /* the damping passed 1e30 without an acceptable step: the numerical floor of this start */
    CK_CALIB_MAXIT = 2,      /* max_iters outer iterations (accepted or rejected) */
    CK_CALIB_DEGENERATE = 3  /* no start (ck_calib_init) or a start that cannot be evaluated; the other fields: see ck_calib_result_t */
};
#define CK_CALIB_MAX_FRAMES 4096 /* per problem */
#define CK_CALIB_MAX_POINTS 4096 /* per frame */
typedef struct ck_calib_params {
    int32_t width, height;         /* of the image, >= 16: the start's principal point is ((w-1)/2, (h-1)/2) */
    uint32_t fixed_mask;           /* bit i freezes parameter i of ck_opencv5_t's order (fx fy cx cy k1 k2 p1 p2 k3) at its start */
    int32_t max_iters;             /* 1..10000, default 100 */
    int32_t min_points_per_frame;  /* >= 4, default 24 (the reference's MIN_CORNERS) */
    int32_t min_frames;            /* >= 1, default 3 */
} ck_calib_params_t;
typedef struct ck_calib_problem {
    int32_t n_frames;
    int32_t start_offset;          /* first of this problem's n_frames + 1 entries of frame_start[], non-decreasing */
    int32_t point_offset;          /* added to those entries: index into board_xy / image_uv */
    int32_t pose_offset;           /* first of this problem's poses in the pose arrays */
} ck_calib_problem_t;
#define CK_CALIB_FIX_DISTORTION 0x1F0u /* fixed_mask: k1 k2 p1 p2 k3 */
#define CK_CALIB_FIX_FOCAL 0x003u      /* fixed_mask: fx fy */
typedef struct ck_calib_result {
    ck_opencv5_t cam;              /* the best accepted parameters */
    int32_t status;                /* CK_CALIB_* */
    int32_t iters;                 /* outer iterations, accepted or rejected */
    int32_t n_frames, n_points;
    double rms;                    /* sqrt(cost / n_points), pixels */
    double cost0, cost;            /* sum of squared pixel residuals at the start and at cam; DEGENERATE: cam = the start, the
                                    * poses the start's, rms = cost0 = cost = 0, iters = 0 */
} ck_calib_result_t;
void ck_calib_params_default(ck_calib_params_t *p, int32_t width, int32_t height);
/* What every calibration entry point refuses, in this order, before it touches a device.  CK_EINVAL: a null pointer; n_problems
 * < 0; width or height < 16; max_iters outside 1..10000; min_points_per_frame < 4; min_frames < 1; a problem with fewer than
 * min_frames frames, offsets outside the arrays, a frame_start run that decreases or leaves the arrays, a frame with fewer than
 * min_points_per_frame points; a coordinate that is not finite.  CK_ECAPACITY: a problem with more than CK_CALIB_MAX_FRAMES frames
 * or a frame with more than CK_CALIB_MAX_POINTS points.  Host only. */
int ck_calib_check(const ck_calib_params_t *p, const ck_calib_problem_t *problems, int32_t n_problems, const double *board_xy,
                   const double *image_uv, const int32_t *frame_start, int32_t n_points_total, int32_t n_starts_total,
                   int32_t n_frames_total);
/* The start of one problem, on the host (no device needed): per frame a homography by the normalised DLT (h33 = 1, 8 x 8 normal
 * equations, Gaussian elimination with partial pivoting), the principal point at the image centre, 1 / fx^2 and 1 / fy^2 by least
 * squares over two orthogonality equations per frame, zero distortion, and per frame the pose from K^-1 H.  poses0 [n_frames_total][12], written at the problem's pose_offset.  *status_out = CK_CALIB_CONVERGED (a start exists) or
 * CK_CALIB_DEGENERATE (singular systems, a focal length that is not positive: frames that are all parallel to the image plane, which
 * leave the focal equations' two columns within sin^2 = 1e-4 of parallel, collinear points;
 * cam0_out and the problem's poses are zero then).  Errors: ck_calib_check's. */
int ck_calib_init(const ck_calib_params_t *p, const ck_calib_problem_t *problem, const double *board_xy, const double *image_uv,
                  const int32_t *frame_start, int32_t n_points_total, int32_t n_starts_total, int32_t n_frames_total,
                  ck_opencv5_t *cam0_out, double *poses0, int32_t *status_out);
/* The solver's residuals and analytic Jacobian of n observations of one frame, on the host: r_out [n][2] = projection - image_uv,
 * J_out [n][2][15] = d r / d (fx fy cx cy k1 k2 p1 p2 k3, rotation increment [3], translation increment [3]) at a zero pose
 * increment, where the increment (w, t) moves the pose to (R C(w), t + dt) with the Cayley map C; columns of frozen intrinsics are
 * zero.  pose: 12 doubles.  CK_EINVAL: a null pointer, n < 0. */
int ck_calib_jacobian(const ck_opencv5_t *cam, const double *pose, const double *board_xy, const double *image_uv, int32_t n,
                      uint32_t fixed_mask, double *r_out, double *J_out);
/* Levenberg-Marquardt over 9 + 6 n_frames parameters from a start, on the host, one thread: the bitwise specification of the
 * device solver.  poses0 and poses_out [n_frames_total][12] (read and written at the problem's pose_offset; they
 * may be the same array).  A start that is not finite, has fx or fy <= 0 or whose cost is not finite: CK_OK with status DEGENERATE.
 * Errors: ck_calib_check's, CK_ENOMEM. */
int ck_calib_refine_host(const ck_calib_params_t *p, const ck_calib_problem_t *problem, const double *board_xy, const double *image_uv,
                         const int32_t *frame_start, int32_t n_points_total, int32_t n_starts_total, int32_t n_frames_total,
                         const ck_opencv5_t *cam0, const double *poses0, ck_calib_result_t *result, double *poses_out);
/* The same for n_problems problems on the handle's stream, one workgroup of 256 threads per problem with the whole iteration
 * inside the kernel; every byte of results and of the problems' poses equals ck_calib_refine_host's.  cams0 [n_problems].  All
 * arrays are host arrays.  Returns when the outputs are complete.  The workspace (the inputs, 312 doubles per frame of the call
 * and the results on the device; allocated by the first call, grown on demand; ck_create allocates none of it) is not bound to the
 * handle's geometry or max_batch, and the staged frames and the detection workspace stay as they are.  Errors: ck_calib_check's
 * (the handle among the null pointers), CK_ENOMEM. */
int ck_calib_refine_batch(ck_handle_t *h, const ck_calib_params_t *p, const ck_calib_problem_t *problems, int32_t n_problems,
                          const double *board_xy, const double *image_uv, const int32_t *frame_start, int32_t n_points_total,
                          int32_t n_starts_total, int32_t n_frames_total, const ck_opencv5_t *cams0, const double *poses0,
                          ck_calib_result_t *results, double *poses_out);
/* ck_calib_init per problem, then ck_calib_refine_batch: what Calibrator::calibrate does in one call.  A problem without a start
 * comes back DEGENERATE and does not disturb its neighbours. */
int ck_calibrate_batch(ck_handle_t *h, const ck_calib_params_t *p, const ck_calib_problem_t *problems, int32_t n_problems,
                       const double *board_xy, const double *image_uv, const int32_t *frame_start, int32_t n_points_total,
                       int32_t n_starts_total, int32_t n_frames_total, ck_calib_result_t *results, double *poses_out);

/* ---- camera rig: one robot pose from all the cameras of a robot ------------------------------------------
 * SQPnP over rays with different origins.  The unknown is world -> robot (R, t): p_robot = R X + t; camera c is mounted by its
 * robot_to_cam (A_c, b_c): p_cam = A_c p_robot + b_c.  A bearing v of camera c is the ray with direction u = A_c^T v through
 * o_c = -A_c^T b_c, and the cost is sum_i (R X_i + t - o_i)^T (I - u_i u_i^T / u_i^T u_i) (R X_i + t - o_i) over the four corners
 * of every tag of every camera: E(r) = r^T Omega r - 2 g^T r + c in r = vec(R) (column-major), minimised from SQPnP's six starts
 * (for coplanar points, one tag or one wall, the three smallest eigenvectors outside Omega's exact null space {vec(a n^T)}).
 * The candidate energy adds sign_change_error * max(0, 1 - (R00 cos gyro + R01 sin gyro)); the cheapest candidate with every point
 * in front of its own camera wins.  One step = one instant: camera c's record of step s is problems[c * n + s], of which n_tags,
 * n_bearings (= 4 * n_tags), the offsets and robot_to_cam are read.  A camera without tags at a step is skipped; a step without
 * any tag has valid = 0 and an all-zero record.
 * Beside ck_sqpnp_solve_batch: a rig of ONE camera returns its pose (1e-9) when the points are not coplanar.  Coplanar points (one
 * tag; tags on one wall) are where the two differ on purpose: the per-camera solver's starts are then an arbitrary basis of a null
 * space and its pose can be the other minimum of the planar ambiguity, this one takes its starts outside that space.  The switch is a
 * threshold (smallest / largest eigenvalue of the points' scatter <= 1e-12): points a hair off a plane take SQPnP's own starts.
 * std_devs takes the distance of the world origin from the ROBOT, the per-camera solver from the camera. */
#define CK_RIG_MAX_CAMS 8
typedef struct ck_rig_params {
    ck_sqpnp_params_t sqpnp;       /* max_iter 15, tol_sq 1e-16 */
    double sign_change_error;      /* 600.0 */
    uint8_t rig_id;                /* camera_id of the fused measurement; default 255 */
    uint8_t pad[7];
} ck_rig_params_t;
typedef struct ck_rig_result {
    int32_t valid;                 /* 0: no pose; every other field is 0 then */
    int32_t n_tags;                /* over all cameras */
    double rot[9];                 /* pivoted robot rotation (world <- robot), row-major */
    double pos[3];                 /* pivoted robot position */
    double std_devs[3];            /* compute_std_devs of (E, |t|, n_tags) */
    double yaw;
    double energy;                 /* E at the returned pose, without the gyro penalty: the sum of the squared point-to-ray distances */
    int32_t cam_tags[CK_RIG_MAX_CAMS]; /* tags camera c contributed */
    double cam_rms[CK_RIG_MAX_CAMS];   /* sqrt(mean point-to-ray distance^2) of camera c's own points at the solution, metres */
} ck_rig_result_t;
void ck_rig_params_default(ck_rig_params_t *p);
/* On the host, one thread, no device needed: the specification of the device solver (same summation and rotation order).
 * CK_EINVAL: a null pointer (tags / bearings may be null when their total is 0), n < 0, n_cams outside 1..CK_RIG_MAX_CAMS, a
 * record with a negative count or offset, offsets outside the arrays, 4 * n_tags != n_bearings.  CK_ENOMEM. */
int ck_rig_solve_host(const ck_rig_params_t *params, int32_t n_cams, const ck_sqpnp_problem_t *problems, int32_t n,
                      const ck_iso3_t *tags, int32_t n_tags_total, const double *bearings, int32_t n_bearings_total,
                      const double *gyro, ck_rig_result_t *out);
/* The same on the handle's stream, one workgroup per step.  Every pointer may be a host or a device pointer.  Returns when out is
 * complete.  The workspace (inputs, results and 7 doubles per point of the call; allocated by the first call, grown on demand;
 * ck_create allocates none of it) leaves the staged frames and the detection workspace as they are.  Errors: ck_rig_solve_host's
 * (the handle among the null pointers), CK_ENOMEM. */
int ck_rig_solve_batch(ck_handle_t *h, const ck_rig_params_t *params, int32_t n_cams, const ck_sqpnp_problem_t *problems, int32_t n,
                       const ck_iso3_t *tags, int32_t n_tags_total, const double *bearings, int32_t n_bearings_total,
                       const double *gyro, ck_rig_result_t *out);
/* Fuses what the last ck_process_* call of each handle left on the device: frame s of every handle is step s.  The kernel reads
 * the other handles' buffers in place, on handles[0]'s stream after an event on each of the others'.  Only out[n] (may be null)
 * and meas[n], valid[n] come back; gyro, has_gyro, out, meas and valid may be host or device pointers.  meas[s].camera_id =
 * rig_id, tag_count = the cameras' detection counts summed, saturated at 255; a step without a pose (no known tag in any camera,
 * has_gyro[s] == 0, no candidate in front of the cameras) has valid 0 and the zeroed record with camera_id alone.  CK_EINVAL: a
 * null pointer, n_cams outside 1..CK_RIG_MAX_CAMS, n < 1, handles on different devices, a handle whose last pipeline call was not
 * a ck_process_* call of exactly n frames.  (The records are the library's own, written by that call: ck_rig_solve_host's checks of
 * counts and offsets apply to the stand-alone calls only.)  CK_ENOMEM: the point scratch is sized for what the handles can hold,
 * n * sum(4 * their detection capacity) * 56 bytes, not for what they saw. */
int ck_rig_process_last(ck_handle_t *const *handles, int32_t n_cams, int32_t n, const ck_rig_params_t *params, const double *gyro,
                        const uint8_t *has_gyro, ck_rig_result_t *out, ck_vision_measurement_t *meas, int32_t *valid);
/* Measurement aid (tools/bench_rig.py): after the calls ck_rig_process_last needs, runs `iters` times on handles[0]'s stream, between two
 * hipEvents each, (a) everything ck_rig_process_last enqueues (gyro in, k_rig, records out; written to ms_rig[iters]) and (b) k_sqpnp
 * once per handle on the problems of its last ck_process_* call, back to back (ms_sqpnp[iters]): the solves the per-camera path pays.
 * Errors as ck_rig_process_last, and CK_EINVAL for iters < 1 or a null array. */
int ck_rig_time_last(ck_handle_t *const *handles, int32_t n_cams, int32_t n, const ck_rig_params_t *params, const double *gyro,
                     const uint8_t *has_gyro, int32_t iters, float *ms_rig, float *ms_sqpnp);

/* ---- robust camera rig: the rig solve that drops a wrong tag ---------------------------------------------------
 * Graduated non-convexity with a truncated-least-squares cost (GNC-TLS; Yang, Antonante, Tzoumas, Carlone, RA-L 2020) around the rig
 * solve above.  The unit of rejection is the TAG (its four corners together): a wrong id, a wrong rotation of the corners and a tag
 * that was moved all corrupt a whole tag.  The tags of an instant are numbered camera-major, then by the tag index of the record.
 *   round 0   the plain solve on all tags (when no candidate passes the cheirality test, the cheapest candidate stands in for
 *             what follows).  At the refinement's rotation R and its t, a point of camera c has d = R X + t - o_c and
 *             e^2 = |d - u (u.d)/(u.u)|^2 / |d|^2 (rad^2; e^2 = 1 when u.d <= 0 or d = 0); rho_j = the mean of tag j's four e^2.
 *   gate      max_j rho_j <= gate_rad^2: every tag is an inlier, `fused` is the plain solve's record byte for byte, status CLEAN.
 *   GNC       otherwise mu = c^2 / (2 rho_max - c^2), c = gate_rad, and per round: w_j = 1 for rho_j <= mu/(mu+1) c^2, 0 for
 *             rho_j >= (mu+1)/mu c^2, c/sqrt(rho_j) sqrt(mu(mu+1)) - mu between; when every w_j is 0 or 1 and so it was, with the
 *             same values, the round before (round 0: all 1), the loop ends; after max_rounds rounds it ends with w_j >= 0.5 as the
 *             inliers (status MAXROUNDS); else the weighted system (every point's contribution times its tag's weight, centred
 *             on the weighted centroid, points of weight 0 skipped) is solved by ONE refinement from the nearest rotation of the
 *             previous round's r, the rho_j are taken at it, mu *= mu_factor.
 *   final     fewer than min_inlier_tags inliers: no pose (status NO_CONSENSUS, `fused` zero).  Otherwise `fused` is the plain
 *             solve on the inlier tags alone: what ck_rig_solve_batch returns for the input with the rejected tags deleted.
 * A camera's record of one step holds at most CK_RIG_ROBUST_MAX_TAGS tags: more is CK_EINVAL in the stand-alone calls; in
 * ck_rig_process_last_robust such a step takes the PLAIN solve (status CLEAN, rounds 0, rejected 0), whatever its residuals. */
#define CK_RIG_ROBUST_MAX_TAGS 64
#define CK_RIG_ROBUST_CLEAN 0        /* no tag dropped (no GNC round ran, or every tag came back in) */
#define CK_RIG_ROBUST_REJECTED 1     /* >= 1 tag dropped */
#define CK_RIG_ROBUST_MAXROUNDS 2    /* max_rounds rounds ran without the weights settling; the inliers are w >= 0.5 */
#define CK_RIG_ROBUST_NO_CONSENSUS 3 /* fewer than min_inlier_tags inliers: no pose */
typedef struct ck_rig_robust_params {
    ck_rig_params_t rig;
    double gate_rad;                      /* 0.01 */
    double mu_factor;                     /* 1.4 */
    int32_t max_rounds;                   /* 64 */
    int32_t min_inlier_tags;              /* 1 */
} ck_rig_robust_params_t;
typedef struct ck_rig_robust_result {
    ck_rig_result_t fused;                /* of the inliers */
    int32_t status;                       /* CK_RIG_ROBUST_* */
    int32_t rounds;                       /* GNC solves that ran */
    int32_t n_rejected;
    int32_t pad;
    uint64_t rejected[CK_RIG_MAX_CAMS];   /* bit t: tag t of camera c's record at this step was dropped */
    double worst_inlier_rad;              /* sqrt(rho) of the worst kept tag at the returned pose (polar(R), t), before the yaw pivot;
                                             0 without a pose */
    double best_rejected_rad;             /* sqrt(rho) of the best dropped tag there; 0 when none */
} ck_rig_robust_result_t;
void ck_rig_robust_params_default(ck_rig_robust_params_t *p);
/* The twins of ck_rig_solve_host / ck_rig_solve_batch / ck_rig_process_last: same arguments (params->rig is theirs), same errors,
 * and CK_EINVAL for gate_rad not finite or <= 0, mu_factor <= 1 (or not finite), max_rounds < 1, min_inlier_tags < 1 and, in the two
 * stand-alone calls, a record of more than CK_RIG_ROBUST_MAX_TAGS tags.  A step without a pose has an all-zero `fused`; a step
 * without tags (or, in ck_rig_process_last_robust, without a gyro heading) an all-zero record.  meas and valid are those of
 * `fused`; tag_count still counts all detections. */
int ck_rig_solve_robust_host(const ck_rig_robust_params_t *params, int32_t n_cams, const ck_sqpnp_problem_t *problems, int32_t n,
                             const ck_iso3_t *tags, int32_t n_tags_total, const double *bearings, int32_t n_bearings_total,
                             const double *gyro, ck_rig_robust_result_t *out);
int ck_rig_solve_robust_batch(ck_handle_t *h, const ck_rig_robust_params_t *params, int32_t n_cams, const ck_sqpnp_problem_t *problems,
                              int32_t n, const ck_iso3_t *tags, int32_t n_tags_total, const double *bearings, int32_t n_bearings_total,
                              const double *gyro, ck_rig_robust_result_t *out);
int ck_rig_process_last_robust(ck_handle_t *const *handles, int32_t n_cams, int32_t n, const ck_rig_robust_params_t *params,
                               const double *gyro, const uint8_t *has_gyro, ck_rig_robust_result_t *out, ck_vision_measurement_t *meas,
                               int32_t *valid);

/* ---- rig pose refinement: the maximum-likelihood pose of an instant and its covariance -----------------------------
 * Levenberg-Marquardt on the angular residual of §4l, e = (p - v (v.p)/(v.v)) / |p| with p = A_c (R X + t - o_c), over every corner of
 * every tag of the instant that `rejected` does not delete, from the fused record's pose (ck_rig_result_t: rot / pos, world <- robot,
 * inverted to world -> robot).  One unknown pose per instant:
 *   CK_RIG_REFINE_FREE    six increments (rotation about world axes, translation), as the calibrators step a pose
 *   CK_RIG_REFINE_PLANAR  world <- robot = (Rz(theta), (x, y, params.z)): three unknowns.  The start is projected: z = params.z,
 *                         (cos theta, sin theta) = (rot[0], rot[3]) normalised (a zero norm: DEGENERATE)
 * gyro_sigma_rad > 0 adds the heading as a measurement: one residual (R_wr[1][0] cos g - R_wr[0][0] sin g) / gyro_sigma_rad (sin(yaw - g)
 * of a level robot); the bearing residuals then count 1 / sigma_rad^2, so both are in units of their standard deviation.  Without the
 * prior sigma_rad only scales the covariance.  A candidate that puts a used point at or behind its camera is refused like a cost
 * increase.  cov = the inverse of the normal matrix at the accepted pose in radians and metres (sigma_rad^2 (J^T J)^-1 with the prior's
 * row scaled by sigma_rad / gyro_sigma_rad), in the world-axes tangent of the world <- robot pose (R_wr <- Exp(dw) R_wr, p <- p + dp),
 * ordered (x, y, z, wx, wy, wz), row-major; in planar mode the rows and columns of z, wx and wy are zero.
 * Status: CONVERGED (an accepted step's relative decrease fell below 1e-14, a step's predicted decrease below 1e-18 of the cost, the
 * cost below 1e-40 rad^2, or no damping up to 1e30 found a decrease: a minimum to round-off), MAXITERS (max_iters iterations ran
 * without a stop rule's confirmation: the record is complete, the pose the best accepted one and cov its covariance, as usable as a
 * CONVERGED one; do not gate on the difference.  On weakly determined scenes, coplanar tags with six unknowns, the damping needs more
 * than ten iterations to come down: at the default 10, 1412 of 2000 noisy draws of three tags on one wall end MAXITERS, within 5e-6 of
 * their own standard deviations of the 30-iteration pose), DEGENERATE (no usable point, a non-finite cost, a normal matrix that does not factor, the
 * planar projection of a vertical x axis: the pose is the start's, cov and std_devs are 0, and so is everything after them but
 * cost0), NO_START (start.valid == 0: all other fields are 0). */
#define CK_RIG_REFINE_FREE 0
#define CK_RIG_REFINE_PLANAR 1
#define CK_RIG_REFINE_CONVERGED 0
#define CK_RIG_REFINE_MAXITERS 1
#define CK_RIG_REFINE_DEGENERATE 2
#define CK_RIG_REFINE_NO_START 3
typedef struct ck_rig_refine_params {
    int32_t mode;                  /* CK_RIG_REFINE_FREE */
    int32_t max_iters;             /* 10; 1..100: a bound on the time of an instant, not a quality gate (see MAXITERS) */
    double sigma_rad;              /* 1e-3: the standard deviation of a bearing, per component */
    double gyro_sigma_rad;         /* 0: no heading prior */
    double z;                      /* 0: the robot origin's height in planar mode */
} ck_rig_refine_params_t;
typedef struct ck_rig_refined {
    int32_t status;                /* CK_RIG_REFINE_* */
    int32_t iters;
    int32_t n_points;              /* corners used */
    int32_t dof;                   /* 2 per corner (the residual's rank), 1 for the prior, minus the unknowns */
    double rot[9];                 /* world <- robot, row-major */
    double pos[3];
    double cov[36];
    double std_devs[3];            /* sqrt of cov's x, y, wz diagonal */
    double cost0, cost;            /* sum of the squared bearing residuals at the start and at the result, rad^2 (without the prior) */
    double rms;                    /* sqrt(cost / n_points) */
    double chi2;                   /* (cost / sigma_rad^2 + prior^2) / dof, 0 when dof < 1: near 1 when sigma_rad is the noise */
    double moved_m;                /* |pos - start.pos| */
    double moved_rad;              /* |rot - start.rot|_F / sqrt(2) = 2 sin(angle / 2) */
    double cam_rms[CK_RIG_MAX_CAMS]; /* of camera c's used corners at the result, rad */
} ck_rig_refined_t;
void ck_rig_refine_params_default(ck_rig_refine_params_t *p);
/* On the host, one thread, no device: the specification of the kernel (same summation order, same bytes).  Reentrant: every call works in
 * memory of its own, so several threads may call it at once.  The first eight arguments
 * after params are ck_rig_solve_host's; gyro [n] may be null when gyro_sigma_rad == 0; start [n] are the fused records; rejected
 * [n][CK_RIG_MAX_CAMS] (may be null) is ck_rig_robust_result_t's mask: bit t of [s][c] deletes tag t (< 64) of camera c's record at
 * instant s.  CK_EINVAL, checked in this order and before anything is written: a null params, problems, start or out; ck_rig_solve_host's
 * checks of counts and records; a mode outside the two; sigma_rad or z not finite, sigma_rad <= 0; gyro_sigma_rad < 0 or not finite;
 * max_iters outside 1..100; gyro_sigma_rad > 0 with a null gyro.  CK_ENOMEM. */
int ck_rig_refine_host(const ck_rig_refine_params_t *params, int32_t n_cams, const ck_sqpnp_problem_t *problems, int32_t n,
                       const ck_iso3_t *tags, int32_t n_tags_total, const double *bearings, int32_t n_bearings_total, const double *gyro,
                       const ck_rig_result_t *start, const uint64_t *rejected, ck_rig_refined_t *out);
/* The same on the handle's stream, one 64-lane wave per instant.  Every pointer may be a host or a device pointer.  Returns when out
 * is complete; the twin's bytes when gyro is a host pointer or null (the heading's sine and cosine are then taken on the host, as
 * the twin takes them; a device gyro takes them on the device).  The workspace is allocated by the first call and grown on demand.
 * Errors: ck_rig_refine_host's (the handle among the null pointers). */
int ck_rig_refine_batch(ck_handle_t *h, const ck_rig_refine_params_t *params, int32_t n_cams, const ck_sqpnp_problem_t *problems, int32_t n,
                        const ck_iso3_t *tags, int32_t n_tags_total, const double *bearings, int32_t n_bearings_total, const double *gyro,
                        const ck_rig_result_t *start, const uint64_t *rejected, ck_rig_refined_t *out);
/* ck_rig_process_last (use_robust == 0: robust_params->rig is read) or ck_rig_process_last_robust, then the refinement of every
 * instant on the same stream, reading the fused records (and the robust solve's masks) and the handles' buffers in place.  start_out
 * [n] (may be null) is what the unrefined call returns in `out`, byte for byte; out [n] the refined records.  meas[s] carries the
 * refined x, y, yaw and std_devs; camera_id and tag_count are the fused measurement's; an instant whose refinement is DEGENERATE or
 * NO_START publishes the fused measurement unchanged.  With gyro_sigma_rad > 0 the heading's sine and cosine are taken on the device:
 * out equals ck_rig_refine_batch on ck_last_pose_inputs' arrays to a tolerance, not byte for byte: 1e-9 (m, rad) on the pose and 1e-6
 * relative on std_devs are what the tests hold it to; measured on an MI355X on the rendered two-camera scene the two were identical
 * (DESIGN.md §4o).  Without the prior the bytes are equal.  Errors: the
 * unrefined call's, ck_rig_refine_host's parameter checks, a null refine_params or out. */
int ck_rig_process_last_refined(ck_handle_t *const *handles, int32_t n_cams, int32_t n, const ck_rig_robust_params_t *robust_params,
                                int32_t use_robust, const ck_rig_refine_params_t *refine_params, const double *gyro, const uint8_t *has_gyro,
                                void *start_out /* ck_rig_result_t [n], with use_robust ck_rig_robust_result_t [n] */, ck_rig_refined_t *out,
                                ck_vision_measurement_t *meas, int32_t *valid);
/* Measurement aid (tools/bench_rig_refine.py): after ck_rig_refine_batch's checks and uploads, runs `iters` times on the handle's
 * stream, between two hipEvents each, k_rig_refine (ms_refine[iters]) and k_rig on the same inputs (ms_rig[iters]).  gyro [n] is the host's. */
int ck_rig_refine_time(ck_handle_t *h, const ck_rig_refine_params_t *params, int32_t n_cams, const ck_sqpnp_problem_t *problems, int32_t n,
                       const ck_iso3_t *tags, int32_t n_tags_total, const double *bearings, int32_t n_bearings_total, const double *gyro,
                       int32_t iters, float *ms_refine, float *ms_rig);

/* ---- camera mounts: the robot_to_cam of a rig's cameras from a capture, batched Levenberg-Marquardt ------
 * The capture is what ck_rig_solve_batch takes: n_steps instants of n_cams cameras, camera c's record of step s at
 * records[c * n_steps + s] (n_tags, n_bearings = 4 * n_tags and the offsets are read; the records' own robot_to_cam is ignored), and
 * the start mounts mounts0[n_cams].  Unknowns: one world -> robot pose per step and the mount of every camera, kept as (A_c, o_c)
 * with p_cam = A_c (p_robot - o_c); robot_to_cam (A_c, b_c = -A_c o_c) is converted at the boundary.  Residual of a corner with
 * bearing v: p = A_c (R_s X + t_s - o_c), e = (p - v (v.p) / (v.v)) / |p|: the point-to-ray distance over the range, radians.
 * fixed_mask: bit 6 c + i freezes increment i of camera c; i = 0..2 the rotation about robot x, y, z, i = 3..5 o_c x, y, z.  A
 * camera with all six bits set comes back bit for bit, so does the quaternion of one with bits 0..2 set.  At least one camera that
 * has observations must have all six bits set (the gauge).  A problem is a run of step_index[] (step numbers of the capture,
 * strictly increasing), so leave-out subsets share one copy of the observations.  A step is used when at least min_cams_per_step
 * cameras have a tag in it; the others are counted in n_steps - n_steps_used and their poses come back as given.  DEGENERATE
 * (CK_CALIB_DEGENERATE; the statuses are ck_calib_status', except that the cost below which a solve is CONVERGED at once is 1e-40:
 * the cost is in rad^2, and 1e-20 would end a noise-free solve at 1e-10 from the truth): fewer than min_steps used steps, a camera with free increments that
 * no chain of shared used steps connects to a fully frozen camera, a start that is not finite.  Mounts and poses are the starts then.
 * ck_rigcal_refine_host is the specification: ck_rigcal_refine_batch returns its bytes. */
#define CK_RIGCAL_MAX_STEPS 4096 /* per problem */
#define CK_RIGCAL_FIX_CAMERA(c) ((uint64_t)0x3F << (6 * (c)))
#define CK_RIGCAL_FIX_POSITION(c) ((uint64_t)0x38 << (6 * (c)))
typedef struct ck_rigcal_params {
    uint64_t fixed_mask;
    int32_t max_iters;             /* 100; 1..10000 */
    int32_t min_steps;             /* 3 */
    int32_t min_cams_per_step;     /* 2 */
    int32_t pad;
} ck_rigcal_params_t;
typedef struct ck_rigcal_problem {
    int32_t n_steps;               /* entries of step_index[] */
    int32_t step_offset;           /* the first of them */
} ck_rigcal_problem_t;
typedef struct ck_rigcal_result {
    ck_iso3_t robot_to_cam[CK_RIG_MAX_CAMS];
    int32_t status;                /* CK_CALIB_* */
    int32_t iters;
    int32_t n_steps, n_steps_used;
    int32_t n_points;              /* of the used steps */
    int32_t pad;
    double rms;                    /* sqrt(cost / n_points), radians */
    double cost0, cost;
    int32_t cam_points[CK_RIG_MAX_CAMS];
    double cam_rms[CK_RIG_MAX_CAMS]; /* of camera c's own points at the solution */
} ck_rigcal_result_t;
void ck_rigcal_params_default(ck_rigcal_params_t *p);
/* What every entry point refuses, in this order, before it touches a device.  CK_EINVAL: a null pointer (tags / bearings may be
 * null when their total is 0); n_cams outside 1..CK_RIG_MAX_CAMS; a negative count or offset, or one outside its array;
 * 4 * n_tags != n_bearings in a record; a problem's step indices out of range or not increasing; max_iters outside 1..10000;
 * min_steps < 1; min_cams_per_step < 2; a tag, bearing or mount that is not finite; no camera with observations that has all six
 * bits of fixed_mask.  CK_ECAPACITY: a problem of more than CK_RIGCAL_MAX_STEPS steps.  Host only. */
int ck_rigcal_check(const ck_rigcal_params_t *p, int32_t n_cams, const ck_sqpnp_problem_t *records, int32_t n_steps, const ck_iso3_t *tags,
                    int32_t n_tags_total, const double *bearings, int32_t n_bearings_total, const ck_rigcal_problem_t *problems,
                    int32_t n_problems, const int32_t *step_index, int32_t n_index_total, const ck_iso3_t *mounts0);
/* Residuals r_out [n][3] and analytic Jacobian J_out [n][3][12] of n points of one view: world_xyz [n][3] seen along bearings [n][3]
 * by the camera mounted by `mount` at the step with pose [12] (R row-major, t).  Columns: the camera's six increments, the step's
 * six (rotation, translation); the camera's frozen columns (bits 0..5 of fixed6) are zero.  Host only. */
int ck_rigcal_jacobian(const ck_iso3_t *mount, const double *pose, const double *world_xyz, const double *bearings, int32_t n,
                       uint32_t fixed6, double *r_out, double *J_out);
/* One problem on the host, one thread, no device.  poses0 [n_steps][12]: the start pose of every step of the capture;
 * poses_out [n_index_total][12]: entry step_offset + j is the pose of the problem's j-th step; it must not overlap poses0 (the two are
 * indexed differently).  Errors: ck_rigcal_check's, CK_ENOMEM. */
int ck_rigcal_refine_host(const ck_rigcal_params_t *p, int32_t n_cams, const ck_sqpnp_problem_t *records, int32_t n_steps,
                          const ck_iso3_t *tags, int32_t n_tags_total, const double *bearings, int32_t n_bearings_total,
                          const ck_rigcal_problem_t *problem, const int32_t *step_index, int32_t n_index_total, const ck_iso3_t *mounts0,
                          const double *poses0, ck_rigcal_result_t *result, double *poses_out);
/* n_problems problems on the handle's stream, one persistent workgroup each, the whole iteration inside the kernel; every byte of
 * results and poses_out equals ck_rigcal_refine_host's.  All arrays are the host's.  Problems may share a run of step_index[]; they then
 * share its entries of poses_out, which hold the poses of the last of them.  The workspace (allocated by the first call,
 * grown on demand; ck_create allocates none of it) leaves the staged frames and the detection workspace as they are.  Errors:
 * ck_rigcal_check's (the handle among the null pointers), CK_ECAPACITY when the records of the call pass 2^31 doubles, CK_ENOMEM. */
int ck_rigcal_refine_batch(ck_handle_t *h, const ck_rigcal_params_t *p, int32_t n_cams, const ck_sqpnp_problem_t *records, int32_t n_steps,
                           const ck_iso3_t *tags, int32_t n_tags_total, const double *bearings, int32_t n_bearings_total,
                           const ck_rigcal_problem_t *problems, int32_t n_problems, const int32_t *step_index, int32_t n_index_total,
                           const ck_iso3_t *mounts0, const double *poses0, ck_rigcal_result_t *results, double *poses_out);

/* The starts from ck_rig_solve_batch with mounts0 and sign_change_error = 0 over the whole capture, once (gyro [n_steps]: the heading
 * of every step, which that solver pivots towards), then ck_rigcal_refine_batch.  A step that solver has no pose for is left out of
 * every problem (it is not counted in n_steps_used, and its pose in poses_out is zero).  The rig solver's device and host results
 * agree to round-off (4e-16), not byte for byte, so this entry point equals the twin from the same starts to a tolerance (DESIGN.md
 * §4l); the byte contract is ck_rigcal_refine_batch's.  Errors: ck_rigcal_check's, ck_rig_solve_batch's. */
int ck_rig_calibrate_batch(ck_handle_t *h, const ck_rigcal_params_t *p, int32_t n_cams, const ck_sqpnp_problem_t *records, int32_t n_steps,
                           const ck_iso3_t *tags, int32_t n_tags_total, const double *bearings, int32_t n_bearings_total, const double *gyro,
                           const ck_rigcal_problem_t *problems, int32_t n_problems, const int32_t *step_index, int32_t n_index_total,
                           const ck_iso3_t *mounts0, ck_rigcal_result_t *results, double *poses_out);
/* Copies to the host what the last ck_process_* call of exactly n frames left on the device for the pose solvers: records_out [n]
 * (n_tags, n_bearings, robot_to_cam, gyro, sign_change_error as that call wrote them; the offsets relative to tags_out and
 * bearings_out, packed in frame order), the known tags' field poses and the four
 * corner bearings of each.  *n_tags_out and *n_bearings_out are the totals, also when they do not fit.  Waits for the handle's
 * stream.  CK_EINVAL: a null pointer, n < 1, a negative capacity, a handle whose last pipeline call was not a ck_process_* call of
 * exactly n frames (the test ck_rig_process_last makes).  CK_ECAPACITY: tag_cap or bearing_cap (in tags, in bearings of 3 doubles)
 * is too small; only records_out and the totals are written then.  CK_ENOMEM. */
int ck_last_pose_inputs(ck_handle_t *h, int32_t n, ck_sqpnp_problem_t *records_out, ck_iso3_t *tags_out, int32_t tag_cap,
                        double *bearings_out, int32_t bearing_cap, int32_t *n_tags_out, int32_t *n_bearings_out);

/* ---- field layout: the tag poses of field.json from a capture, batched Levenberg-Marquardt ----------------
 * The capture is what ck_rig_solve_batch takes (records[c * n_steps + s]: n_tags, n_bearings = 4 * n_tags and the offsets are read,
 * the records' robot_to_cam is ignored in favour of mounts[n_cams], which stay fixed), but in place of the tags' poses there is
 * tag_index[n_tags_total]: for every observed tag its entry of layout0[n_layout].  The same tag in two cameras of a step is normal;
 * twice in one view it is refused.  Unknowns: one world <- tag pose (Q_k, c_k) per tag and one world -> robot pose per used step.  A
 * corner x of a tag (corner_points_from_center: (0, -S, -S), (0, S, -S), (0, S, S), (0, -S, S), S = 0.08255) is X = Q_k x + c_k, and
 * its residual is §4l's: p = A_c (R_s X + t_s - o_c), e = (p - v (v.p) / (v.v)) / |p|, radians.  Increments: Q_k <- Q_k C(dw) about
 * the tag's own axes, c_k <- c_k + dc in world axes.  fixed6[n_layout]: bits 0..2 of a tag's byte freeze its rotation, bits 3..5 c_k
 * x, y, z; a wholly frozen tag (63) comes back bit for bit, so do the quaternion of a tag with bits 0..2 set and every frozen
 * component of c_k.  At least one tag with sightings must be wholly frozen (the gauge).  A tag without a sighting in the used steps
 * of a problem is returned as given with tag_sightings = 0.  Problems are runs of step_index[] as in §4l (ck_rigcal_problem_t).  A
 * step is used when at least min_tags_per_step distinct tags are seen in it, over all cameras.  DEGENERATE (the statuses and the
 * solver are §4l's): fewer than min_steps used steps, a start pose that is not finite, a tag with a free increment that no chain
 * of shared used steps joins to a wholly frozen tag.  Layout and poses are the starts then.
 * ck_fieldcal_refine_host is the specification: ck_fieldcal_refine_batch returns its bytes. */
#define CK_FIELDCAL_MAX_TAGS 64    /* tags of the layout with sightings in one problem */
#define CK_FIELDCAL_MAX_STEPS 4096 /* per problem */
#define CK_FIELDCAL_FIX_ALL 63
typedef struct ck_fieldcal_params {
    int32_t max_iters;             /* 100; 1..10000 */
    int32_t min_steps;             /* 3 */
    int32_t min_tags_per_step;     /* 2 */
    int32_t pad;
} ck_fieldcal_params_t;
typedef struct ck_fieldcal_result {
    int32_t status;                /* CK_CALIB_* */
    int32_t iters;
    int32_t n_steps, n_steps_used;
    int32_t n_points;              /* of the used steps */
    int32_t n_tags_solved;         /* tags with sightings and a free increment */
    double rms;                    /* sqrt(cost / n_points), radians */
    double cost0, cost;
} ck_fieldcal_result_t;
void ck_fieldcal_params_default(ck_fieldcal_params_t *p);
/* What every entry point refuses, in this order, before it touches a device.  CK_EINVAL: (1) a null pointer (tag_index / bearings may
 * be null when their total is 0); (2) n_cams outside 1..CK_RIG_MAX_CAMS, n_layout < 1, a negative count; (3) a record's count or offset
 * negative or outside its array; (4) 4 * n_tags != n_bearings in a record; (5) a tag_index outside 0..n_layout - 1; (6) a problem's run
 * outside step_index[], its step numbers out of range or not increasing; (7) max_iters outside 1..10000, min_steps < 1,
 * min_tags_per_step < 2, a fixed6 byte above 63; (8) a bearing, mount or layout pose that is not finite (a zero quaternion counts);
 * (9) the same tag twice in one view; (10) no wholly frozen tag with a sighting.  CK_ECAPACITY: (11) a problem of more than
 * CK_FIELDCAL_MAX_STEPS steps, or whose steps see more than CK_FIELDCAL_MAX_TAGS different tags.  Host only. */
int ck_fieldcal_check(const ck_fieldcal_params_t *p, int32_t n_cams, const ck_sqpnp_problem_t *records, int32_t n_steps,
                      const int32_t *tag_index, int32_t n_tags_total, const double *bearings, int32_t n_bearings_total,
                      const ck_rigcal_problem_t *problems, int32_t n_problems, const int32_t *step_index, int32_t n_index_total,
                      const ck_iso3_t *mounts, const ck_iso3_t *layout0, int32_t n_layout, const uint8_t *fixed6);
/* Residuals r_out [n][3] and analytic Jacobian J_out [n][3][12] of the first n <= 4 corners of one sighting: the tag at `tag` seen
 * along bearings [n][3] by the camera mounted by `mount` at the step with pose [12] (R row-major, t).  Columns: the tag's rotation
 * about its own axes (0..2), the tag's position (3..5), the step's rotation and translation (6..11); the tag's frozen columns (bits
 * 0..5 of fixed6) are zero.  Host only. */
int ck_fieldcal_jacobian(const ck_iso3_t *mount, const double *pose, const ck_iso3_t *tag, const double *bearings, int32_t n,
                         uint32_t fixed6, double *r_out, double *J_out);
/* One problem on the host, one thread, no device.  poses0 [n_steps][12]: the start pose of every step of the capture.  Outputs:
 * layout_out [n_layout], tag_sightings [n_layout], tag_rms [n_layout] (the rms of the tag's own points at the solution, radians; 0
 * without sightings) and poses_out [n_index_total][12] as in ck_rigcal_refine_host.  Errors: ck_fieldcal_check's, CK_ENOMEM. */
int ck_fieldcal_refine_host(const ck_fieldcal_params_t *p, int32_t n_cams, const ck_sqpnp_problem_t *records, int32_t n_steps,
                            const int32_t *tag_index, int32_t n_tags_total, const double *bearings, int32_t n_bearings_total,
                            const ck_rigcal_problem_t *problem, const int32_t *step_index, int32_t n_index_total, const ck_iso3_t *mounts,
                            const ck_iso3_t *layout0, int32_t n_layout, const uint8_t *fixed6, const double *poses0,
                            ck_fieldcal_result_t *result, ck_iso3_t *layout_out, int32_t *tag_sightings, double *tag_rms, double *poses_out);
/* n_problems problems on the handle's stream, one persistent workgroup each, the whole iteration inside the kernel; every byte of
 * results, layout_out [n_problems][n_layout], tag_sightings and tag_rms (the same shape) and poses_out equals
 * ck_fieldcal_refine_host's.  All arrays are the host's.  The workspace (allocated by the first call, grown on demand; ck_create
 * allocates none of it) leaves the staged frames and the detection workspace as they are.  Errors: ck_fieldcal_check's (the handle
 * among the null pointers), CK_ECAPACITY when the records of the call pass 2^31 doubles, CK_ENOMEM. */
int ck_fieldcal_refine_batch(ck_handle_t *h, const ck_fieldcal_params_t *p, int32_t n_cams, const ck_sqpnp_problem_t *records,
                             int32_t n_steps, const int32_t *tag_index, int32_t n_tags_total, const double *bearings,
                             int32_t n_bearings_total, const ck_rigcal_problem_t *problems, int32_t n_problems, const int32_t *step_index,
                             int32_t n_index_total, const ck_iso3_t *mounts, const ck_iso3_t *layout0, int32_t n_layout,
                             const uint8_t *fixed6, const double *poses0, ck_fieldcal_result_t *results, ck_iso3_t *layout_out,
                             int32_t *tag_sightings, double *tag_rms, double *poses_out);
/* The starts from ck_rig_solve_batch with the tags at layout0, the given mounts and sign_change_error = 0 over the whole capture, once
 * (gyro [n_steps]), then ck_fieldcal_refine_batch.  A step that solver has no pose for is left out of every problem (its pose in
 * poses_out is zero).  As with ck_rig_calibrate_batch this entry equals the twin from the host rig solver's starts to a tolerance
 * (DESIGN.md §4m), not byte for byte.  Errors: ck_fieldcal_check's, ck_rig_solve_batch's. */
int ck_field_calibrate_batch(ck_handle_t *h, const ck_fieldcal_params_t *p, int32_t n_cams, const ck_sqpnp_problem_t *records,
                             int32_t n_steps, const int32_t *tag_index, int32_t n_tags_total, const double *bearings,
                             int32_t n_bearings_total, const double *gyro, const ck_rigcal_problem_t *problems, int32_t n_problems,
                             const int32_t *step_index, int32_t n_index_total, const ck_iso3_t *mounts, const ck_iso3_t *layout0,
                             int32_t n_layout, const uint8_t *fixed6, ck_fieldcal_result_t *results, ck_iso3_t *layout_out,
                             int32_t *tag_sightings, double *tag_rms, double *poses_out);

/* ---- multi-GPU: the final pose gather ----------------------------------------------------------------------------------
 * Frames shard over GPUs without any data-path collective (one handle, one process or host thread per GPU).  The only
 * exchange is the gather of the 64-byte records (the wire struct of crates/whacknet/src/lib.rs:43-66): ONE ncclAllGather
 * (RCCL over xGMI) of n x 64 bytes per batch, on the communicator's own stream beside the handle's next batch.  The host distributes the 128-byte id that rank 0
 * obtains from ck_comm_unique_id over whatever channel it has (the reference has UDP; the Python mirror uses
 * torch.distributed's store).  librccl is opened on first use: CK_EUNSUPPORTED when it cannot be loaded. */
#define CK_COMM_ID_BYTES 128
#define CK_BACKEND_HIP 1
typedef struct ck_comm ck_comm_t;
int ck_backend(const ck_handle_t *h);                      /* CK_BACKEND_HIP: the library has no CPU backend */
int ck_comm_unique_id(uint8_t *id_out);                    /* rank 0: id_out[CK_COMM_ID_BYTES] */
int ck_comm_create(ck_handle_t *h, const uint8_t *id, int32_t world, int32_t rank, ck_comm_t **out); /* collective: every rank calls it */
void ck_comm_destroy(ck_comm_t *comm);
/* Gathers the records the handle's last ck_process_* call produced (they are still on the device) from every rank into
 * out[world*rows] in rank order.  n_valid = the frames of that call (CK_EINVAL when it is not: the send buffer is the handle's
 * own, so a wrong count would ship stale records); rows = the common row count of the collective, the same on every rank,
 * n_valid <= rows <= max_batch: the library pads a ragged last shard with empty records (all zero, tag_count = 0 — what a
 * frame without a pose publishes anyway: crates/apriltags/src/lib.rs:365-376).  `out` may be a host or a device pointer.
 * sync = 0 only enqueues: the handle's stream copies the records aside (the next ck_process_* call may follow at once) and the
 * collective runs on the communicator's stream; `out` is complete after ck_comm_sync (or a later call with sync = 1) — NOT after
 * a synchronisation of the handle alone.  A rank whose n_valid fails the local check still takes part with `rows` empty records
 * and then returns CK_EINVAL, so its peers complete; after any other error of a collective destroy the communicator on every rank.
 * Destroy a communicator before the handle it was made for. */
int ck_gather_poses(ck_handle_t *h, ck_comm_t *comm, int32_t n_valid, int32_t rows, ck_vision_measurement_t *out, int32_t sync);
int ck_comm_sync(ck_comm_t *comm);
const char *ck_comm_library(const ck_comm_t *comm);      /* path of the librccl the communicator's calls resolved to */

/* OpenCVModel5 unprojection of pixel points to bearings (x,y,1)/norm; ok[i]=0 when it does not converge. */
int ck_unproject_opencv5(const ck_opencv5_t *cam, const double *px, int32_t n, double *bearings,
                         uint8_t *ok);

/* ---- camera models: OpenCVModel5, EUCM, UCM ----------------------------------------------------------------
 * The Enhanced Unified Camera Model (Khomutenko, Garcia & Martinet 2016) for lenses whose image corners are 70 degrees and
 * more off axis; UCM is its special case beta = 1, the pinhole alpha = 0.  Projection and closed-form unprojection use only
 * + - * / sqrt on doubles (csrc/ck_camera_math.h, compiled into the host functions and into the kernels), so the host
 * functions return the bytes of the device path. */
enum { CK_CAMERA_OPENCV5 = 0, CK_CAMERA_EUCM = 1, CK_CAMERA_UCM = 2 };
typedef struct ck_camera {
    int32_t model;
    int32_t pad;
    double k[9]; /* OPENCV5: fx fy cx cy k1 k2 p1 p2 k3 (ck_opencv5_t's order)
                  * EUCM:    fx fy cx cy alpha beta, k[6..8] = 0
                  * UCM:     fx fy cx cy alpha; k[5] is read as 1.0 whatever it holds, k[6..8] = 0 */
} ck_camera_t;

/* CK_EINVAL, in this order: a null pointer; an unknown model; a parameter that is not finite; fx or fy <= 0; for EUCM / UCM
 * alpha outside [0, 1], beta <= 0, a non-zero k[6..8].  UCM's k[5] is never looked at.  Host arithmetic, no device needed. */
int ck_camera_check(const ck_camera_t *cam);
/* Pixels px[n][2] -> unit bearings[n][3]; ok[i] = 0: OPENCV5 did not converge, EUCM / UCM the pixel lies outside the model's
 * valid disc (alpha > 0.5: r2 >= 1 / (beta (2 alpha - 1))) or the bearing is not finite.  Pure C, no device needed.  For
 * OPENCV5 the same 50-step fixed-point iteration as the device path.  Errors: ck_camera_check's, a null array, n < 0. */
int ck_camera_unproject_host(const ck_camera_t *cam, const double *px, int32_t n, double *bearings, uint8_t *ok);
/* Camera points xyz[n][3] -> pixels px[n][2].  ok[i] = 0 (and the pixel (0, 0)): the point does not project (OPENCV5: Z <= 0;
 * EUCM / UCM: den <= 0 or Z <= -w d, w = alpha > 0.5 ? (1 - alpha) / alpha : alpha / (1 - alpha)) or the pixel is not finite. */
int ck_camera_project_host(const ck_camera_t *cam, const double *xyz, int32_t n, double *px, uint8_t *ok);
/* The normalised points (x, y) = (mx / kz, my / kz) of pixels, what the per-tag pose works on: ok[i] additionally needs
 * kz > 0 (a pixel more than 90 degrees off axis has a bearing but no normalised point).  OPENCV5: the undistorted point. */
int ck_camera_normalize_host(const ck_camera_t *cam, const double *px, int32_t n, double *xy, uint8_t *ok);
/* The device counterpart of ck_unproject_opencv5, one thread per point: the bytes of ck_camera_unproject_host for every
 * model and, for OPENCV5, of ck_unproject_opencv5.  CK_ENODEVICE without a device (after the argument checks). */
int ck_camera_unproject(const ck_camera_t *cam, const double *px, int32_t n, double *bearings, uint8_t *ok);
/* ---- intrinsic calibration of any camera model ---------------------------------------------------------------
 * The five calibration entry points again, taking the model (CK_CAMERA_*) and ck_camera_t; the arrays, the problem records, the
 * params, the checks and the LM rules are ck_calib_*'s.  EUCM / UCM keep fx fy cx cy alpha beta in the first six of the solver's
 * nine parameter slots: fixed_mask bits 0..5 freeze them, slots 6..8 are always frozen, and UCM also freezes slot 5 at 1.0.  An
 * observation that does not project (ck_camera_project_host's rule) and a candidate with alpha outside [0, 1] or beta <= 0 make the
 * cost NaN: the step is rejected, never clamped; a start like that is DEGENERATE.  With model == CK_CAMERA_OPENCV5 every call
 * returns what its ck_calib_* counterpart returns, byte for byte.  CK_EINVAL also for an unknown model. */
#define CK_CAMCAL_STARTS 6
typedef struct ck_camera_calib_result {
    ck_camera_t cam;               /* the best accepted parameters (UCM: k[5] = 1.0) */
    int32_t status, iters, n_frames, n_points;
    double rms, cost0, cost;       /* as ck_calib_result_t */
    int32_t start, n_starts;       /* ck_camera_calibrate_batch: the start this result came from, of how many; otherwise 0 of 1 */
} ck_camera_calib_result_t;
/* J_out [n][2][15]: columns fx fy cx cy alpha beta 0 0 0, then the six pose columns (OPENCV5: ck_calib_jacobian's). */
int ck_camera_calib_jacobian(int32_t model, const ck_camera_t *cam, const double *pose, const double *board_xy, const double *image_uv,
                             int32_t n, uint32_t fixed_mask, double *r_out, double *J_out);
/* Start `start_index` of a problem, on the host.  OPENCV5 has one start, ck_calib_init's.  EUCM / UCM have CK_CAMCAL_STARTS,
 * because the pinhole start alone is not usable on wide lenses: 0 = ck_calib_init's focal lengths, 1..5 = fx = fy = {0.3, 0.45,
 * 0.65, 1.0, 1.5} * max(width, height); every one with the principal point at the image centre, alpha = 0.5, beta = 1, and each
 * frame's pose from its DLT homography and that K.  *status_out as ck_calib_init.  CK_EINVAL also for a start_index outside the
 * model's starts. */
int ck_camera_calib_init(int32_t model, const ck_calib_params_t *p, const ck_calib_problem_t *problem, const double *board_xy,
                         const double *image_uv, const int32_t *frame_start, int32_t n_points_total, int32_t n_starts_total,
                         int32_t n_frames_total, int32_t start_index, ck_camera_t *cam0_out, double *poses0, int32_t *status_out);
/* One problem from one start on the host, one thread: the bitwise specification of ck_camera_calib_refine_batch. */
int ck_camera_calib_refine_host(int32_t model, const ck_calib_params_t *p, const ck_calib_problem_t *problem, const double *board_xy,
                                const double *image_uv, const int32_t *frame_start, int32_t n_points_total, int32_t n_starts_total,
                                int32_t n_frames_total, const ck_camera_t *cam0, const double *poses0, ck_camera_calib_result_t *result,
                                double *poses_out);
/* n_problems problems, each from its start cams0[i], one workgroup of 256 threads per problem: ck_camera_calib_refine_host's bytes. */
int ck_camera_calib_refine_batch(ck_handle_t *h, int32_t model, const ck_calib_params_t *p, const ck_calib_problem_t *problems,
                                 int32_t n_problems, const double *board_xy, const double *image_uv, const int32_t *frame_start,
                                 int32_t n_points_total, int32_t n_starts_total, int32_t n_frames_total, const ck_camera_t *cams0,
                                 const double *poses0, ck_camera_calib_result_t *results, double *poses_out);
/* Every problem from every start of its model (ck_camera_calib_init), all of them in one launch; per problem the result with the
 * lowest finite final cost (ties: the lowest start), its poses in poses_out, `start` and `n_starts` in the record.  A problem
 * none of whose starts can be evaluated is DEGENERATE (start 0's record) and does not disturb its neighbours.  CK_ECAPACITY
 * also when n_starts x n_frames_total passes 2^31. */
int ck_camera_calibrate_batch(ck_handle_t *h, int32_t model, const ck_calib_params_t *p, const ck_calib_problem_t *problems,
                              int32_t n_problems, const double *board_xy, const double *image_uv, const int32_t *frame_start,
                              int32_t n_points_total, int32_t n_starts_total, int32_t n_frames_total,
                              ck_camera_calib_result_t *results, double *poses_out);

/* A handle setting, like ck_set_quad_sigma.  While a camera is set, ck_process_batch_device, ck_process_uploaded,
 * ck_process_ingested, ck_estimate_tag_poses and ck_last_tag_poses use it instead of their params' `cam` field, which is then
 * ignored (and not checked).  NULL restores the params' field.  A refused camera (ck_camera_check) leaves the previous
 * setting in place.  What reads the glue's bearings in place (ck_rig_process_last*, ck_last_pose_inputs) inherits the model. */
int ck_set_camera(ck_handle_t *h, const ck_camera_t *cam);

/* ---- sub-pixel corners: gradient-orthogonality refinement and board recovery -------------------------------
 * The refinement looks at the pixels around a corner again (Förstner & Gülch 1987; OpenCV's cornerSubPix, ArUco's
 * CORNER_REFINE_SUBPIX): at a corner or an X-saddle every image gradient in the neighbourhood is orthogonal to the vector from the
 * corner to its pixel, so the corner q solves (sum m g g^T) q = sum m g g^T p over a window of (2 half_win + 1)^2 taps p, weighted
 * by a Gaussian m, and the window is moved to q until the step falls below eps.  Coordinates are the library's: pixel (i, j) covers
 * [i, i+1) x [j, j+1) (ck_detection_t.p).  Sampling is bilinear on the 8-bit frame, clamped to the frame edge.  Only + - * / and
 * one sqrt on doubles in a summation order DESIGN.md states (csrc/ck_subpix_math.h, compiled into the host twins and into the
 * kernels), so the host twins return the bytes of the device path. */
enum { CK_SUBPIX_CONVERGED = 0, CK_SUBPIX_MAXIT = 1, CK_SUBPIX_FLAT = 2, CK_SUBPIX_REJECTED = 3 };
typedef struct ck_subpix_params {
    int32_t half_win;  /* w, 2..7: the window is (2w + 1)^2 taps; default 5 */
    int32_t max_iters; /* 1..1000, default 30 */
    double eps;        /* stop when the step is at most this long, pixels; >= 0, default 1e-3 */
    double det_min;    /* |det| <= det_min: the window has no corner (FLAT); >= 0, default 1e-2 */
} ck_subpix_params_t;
typedef struct ck_subpix_info {
    int32_t status;    /* CK_SUBPIX_*.  FLAT: a window's determinant was at most det_min.  REJECTED: the point ended more than
                        * half_win from its start on either axis (or not finite).  Both return the input, bit for bit */
    int32_t iters;     /* steps taken */
    double shift;      /* |out - in|, pixels; 0 for FLAT and REJECTED */
} ck_subpix_info_t;
void ck_subpix_params_default(ck_subpix_params_t *pp);
/* The (2w + 1)^2 weights exp(-(dx / w)^2) * exp(-(dy / w)^2), row-major: pure host arithmetic, no device needed.  The one table
 * the kernels and the twins both read.  CK_EINVAL: a null pointer, a parameter out of range. */
int ck_subpix_weights(const ck_subpix_params_t *pp, double *w_out);
/* Refines n points xy_in [n][2] of the staged frames (ck_upload_frames and its kin): point i lies in frame frame[i] (NULL: every
 * point in frame 0).  xy_out [n][2] and info [n] (may be NULL) come back; frame, xy_in, xy_out and info may be host or device
 * pointers.  One 64-lane wave per point on the handle's stream; the detection workspace stays as it is.  n = 0 is a no-op.
 * CK_EINVAL: a null pointer, n < 0, a parameter out of range, a frame index outside the staged frames, a point that is not finite
 * or outside [0, width] x [0, height]. */
int ck_corner_subpix(ck_handle_t *h, const ck_subpix_params_t *pp, const int32_t *frame, const double *xy_in, int32_t n,
                     double *xy_out, ck_subpix_info_t *info);
/* The one-thread C twin on host images (all of one size): the bytes of ck_corner_subpix.  No device needed. */
int ck_corner_subpix_host(const ck_subpix_params_t *pp, const ck_image_u8_t *imgs, int32_t n_imgs, const int32_t *frame,
                          const double *xy_in, int32_t n, double *xy_out, ck_subpix_info_t *info);
/* A handle setting, like ck_set_quad_sigma and ck_set_camera; NULL = off, the default.  While it is on, every ck_detect_* and
 * ck_process_* call refines the four corners of every final detection on the device, after the de-duplication, on the
 * full-resolution unfiltered frame the call was given (staged, caller device memory, an ingest slot), rewrites `p` and recomputes `c`
 * as the image of the tag centre under the homography of the four new corners.  A detection none of whose corners moved keeps its
 * bytes.  What reads the detections afterwards (the glue's bearings, ck_last_tag_poses, ck_last_pose_inputs, the rig calls, the
 * preview overlay) inherits the refined corners.  While it is off no launch is added.  CK_EINVAL: a parameter out of range (the
 * previous setting stays). */
int ck_set_corner_subpix(ck_handle_t *h, const ck_subpix_params_t *pp);

/* Board recovery: from the few tags of a tag grid that decoded to all of them.  ck_board_t is the Board of
 * chalkydri_amd/calibration.py: rows x cols tags of edge tag_size, tag_spacing times that between neighbours, ids row-major from
 * first_id; rows * cols <= 64.  A seed is a detection of family `family` with an id on the board and hamming 0, the first per id;
 * its corners are refined and it is kept when none moved more than seed_max_shift.  Then rounds: every absent tag with a known
 * 4-neighbour (the first in the order left, right, up, down, among the tags known when the round began) maps its four corners
 * through that neighbour's homography, skips the round when a prediction lies within half_win + 2 pixels of the frame edge,
 * refines them, and is accepted when all four converge, none moved more than max_shift, and a second refinement started `probe`
 * away from each result ends within `agree` of it — which keeps flat and occluded spots out.  Rounds go on until one adds no tag, at
 * most rows + cols of them. */
typedef struct ck_board {
    int32_t rows, cols, first_id, family;
    double tag_size, tag_spacing;
} ck_board_t;
typedef struct ck_board_params {
    double seed_max_shift; /* 2.0 px */
    double max_shift;      /* 2.5 px */
    double probe[2];       /* (+0.7, -0.6) px */
    double agree;          /* 0.05 px */
} ck_board_params_t;
void ck_board_params_default(ck_board_params_t *bp);
/* On the detections the handle's last ck_detect_* / ck_process_* call left on the device (ck_last_tag_poses' validity rule) and the
 * frames of that call.  uv_out [n][rows * cols][4][2] (zeros for absent tags), tag_state [n][rows * cols] (0 absent, 1 seed,
 * 2 recovered) and n_tags [n] come back, n = the frames of that call; host or device pointers.  One workgroup per frame.
 * CK_EINVAL: a null pointer, a board with rows or cols < 1, rows * cols > 64, a family the handle does not have, tag_size <= 0,
 * tag_spacing < 0 or not finite, a parameter out of range, no such call's result in the workspace. */
int ck_board_corners_last(ck_handle_t *h, const ck_board_t *board, const ck_subpix_params_t *pp, const ck_board_params_t *bp,
                          double *uv_out, uint8_t *tag_state, int32_t *n_tags);
/* The one-thread C twin: dets [n][cap_per_frame] with counts [n], as ck_detect_* returns them, and the n images they came from. */
int ck_board_corners_host(const ck_board_t *board, const ck_subpix_params_t *pp, const ck_board_params_t *bp, const ck_image_u8_t *imgs,
                          int32_t n, const ck_detection_t *dets, int32_t cap_per_frame, const int32_t *counts, double *uv_out,
                          uint8_t *tag_state, int32_t *n_tags);

/* ---- coloured game pieces: HSV mask, connected components, targets ----------------------------------------------
 * The second consumer of a camera's frames (the reference's `ml` slot, config.rs:88-102): objects of one saturated colour, found in
 * the colour information that is on the device already — the sources of the colour preview (§4g, §4i).  All integer arithmetic.
 *
 * Pixels.  O[y][x] is the oriented full-resolution triple of ck_preview_color (width = W, height = H, overlay = 0).  The packed
 * colour families (RGB3 BGR3 RGBA BGRA) give the classifier their own R, G, B bytes; the 4:2:2 families and the JPEG colour form
 * give it libjpeg's ycc_rgb_convert of the triple, clamped to 0..255 (arithmetic shifts):
 *   R = Y + ((91881 (Cr-128) + 32768) >> 16),  G = Y + ((-22554 (Cb-128) - 46802 (Cr-128) + 32768) >> 16),
 *   B = Y + ((116130 (Cb-128) + 32768) >> 16).
 * HSV, 8 bits, OpenCV's ranges.  V = max, m = min, d = V - m; S = V ? floor(255 d / V) : 0; H = 0 when d = 0, else with ties for
 * the maximum going to R, then G, then B: hn = 30 (G-B) + (G < B ? 180 d : 0) | 30 (B-R) + 60 d | 30 (R-G) + 120 d and
 * H = floor((2 hn + d) / (2 d)) mod 180.  The kernels compare by cross-multiplication and never divide.
 * Class c holds a pixel when s_min <= S <= s_max, v_min <= V <= v_max and H in [h_min, h_max], or, when h_min > h_max (red wraps),
 * in [h_min, 179] or [0, h_max].  Every class is a bit plane of its own: 32-bit words, bit x & 31 of word x >> 5 of row y, rows
 * of ceil(W / 32) words, the bits at x >= W zero.
 * Morphology: `erode` then `dilate` iterations of the 3x3 square, outside the frame background for both.
 * Components: 8-connected.  Per component the area N, the inclusive box x0 y0 x1 y1, seed = the smallest y W + x, and the sums
 * sx sy sxx sxy syy of its pixels' coordinates.  Filter, with bw = x1-x0+1 and bh = y1-y0+1: min_area <= N; N <= max_area (0: no
 * upper bound); 1000 N >= min_fill_permille bw bh; min_aspect_permille bh <= 1000 bw <= max_aspect_permille bh (0: no upper bound).
 * Order: area descending, then seed ascending.  counts[frame][class] is the number that pass; min(count, max_targets, cap) records
 * are written (the rest of `out` is zero) and CK_BLOB_TRUNCATED is set in the frame's status when that is fewer.
 * Capacity: at most max_components components of area >= min_area per frame and class.  More set CK_BLOB_OVERFLOW in the frame's
 * status and make that class's count 0: no targets rather than an arbitrary subset. */
#define CK_BLOB_MAX_CLASSES 4
enum { CK_BLOB_HAS_BEARING = 1, CK_BLOB_HAS_GROUND = 2, CK_BLOB_AT_BORDER = 4 }; /* ck_blob_t.flags */
enum { CK_BLOB_TRUNCATED = 1, CK_BLOB_OVERFLOW = 2 };                             /* status[frame] */
typedef struct ck_blob_class {
    int32_t h_min, h_max;          /* 0..179 each; h_min > h_max wraps through 0 */
    int32_t s_min, s_max;          /* 0..255 */
    int32_t v_min, v_max;          /* 0..255 */
    int32_t min_area, max_area;    /* pixels, >= 0; max_area 0: no upper bound */
    int32_t min_fill_permille;     /* >= 0: area against the box */
    int32_t min_aspect_permille;   /* >= 0: box width against box height */
    int32_t max_aspect_permille;   /* >= 0; 0: no upper bound */
    int32_t pad;
    double ground_z;               /* the plane the piece's lowest point rests on, robot frame, metres */
} ck_blob_class_t;
typedef struct ck_blob_params {
    int32_t n_classes;             /* 1..CK_BLOB_MAX_CLASSES */
    int32_t erode, dilate;         /* 0..4 iterations each */
    int32_t max_targets;           /* >= 0: records written per frame and class, at most */
    int32_t max_components;        /* >= 1, default 4096 */
    int32_t has_camera;            /* cam is valid (a camera set with ck_set_camera comes first) */
    int32_t has_mount;             /* robot_to_cam is valid */
    int32_t pad;
    ck_blob_class_t cls[CK_BLOB_MAX_CLASSES];
    ck_camera_t cam;
    ck_iso3_t robot_to_cam;        /* the solver's convention: cam from robot */
    double max_range;              /* metres along the ray; beyond it there is no ground point */
} ck_blob_params_t;
/* One target.  Doubles in the library's pixel convention, pixel i covers [i, i+1). */
typedef struct ck_blob {
    int32_t class_id, flags;       /* CK_BLOB_HAS_BEARING | CK_BLOB_HAS_GROUND | CK_BLOB_AT_BORDER (the box touches the frame edge) */
    int32_t area;
    int32_t x0, y0, x1, y1;        /* inclusive */
    int32_t seed;                  /* the smallest y W + x */
    int64_t sx, sy, sxx, sxy, syy;
    double cx, cy;                 /* sx / N + 0.5, sy / N + 0.5 */
    double major, minor;           /* square roots of the eigenvalues of the covariance of the pixel centres */
    double axis[2];                /* unit major axis, first non-zero component positive; (1, 0) when isotropic */
    double bearing[3];             /* unit ray of (cx, cy) through the camera model; zeros without CK_BLOB_HAS_BEARING */
    double ground[2];              /* robot-frame (x, y) where the ray through the box's bottom centre ((x0+x1+1)/2, y1+1) meets
                                    * z = ground_z: valid with CK_BLOB_HAS_GROUND, that is with a mount, a ray that goes down, a
                                    * camera above the plane and a range <= max_range; zeros otherwise */
} ck_blob_t;
/* One class, and in every class slot: any hue (0..179), s and v 64..255, min_area 16, no other filter, ground_z 0.  No morphology,
 * max_targets 16, max_components 4096, no camera, no mount (the identity), max_range 20. */
void ck_blob_params_default(ck_blob_params_t *pp);
/* CK_EINVAL, in this order: a null pointer; n_classes outside 1..4; erode or dilate outside 0..4; max_targets < 0;
 * max_components < 1; then per class in turn: a hue bound outside 0..179, an s or v bound outside 0..255, a negative area or
 * permille value, a ground_z that is not finite; then, with has_camera, a camera ck_camera_check refuses; then, with has_mount, a
 * mount that is not finite or whose quaternion is zero; max_range not finite or negative.  Host arithmetic, no device needed. */
int ck_blob_check(const ck_blob_params_t *pp);
/* rgb [n][3] -> hsv [n][3] by the definition above: for tuning UIs and tests.  Host arithmetic. */
int ck_blob_rgb_hsv(const uint8_t *rgb, int64_t n, uint8_t *hsv_out);
/* The host twin, pure C, one thread: rgb [n][H][W][3] is what ck_blob_rgb returns.  stage 0: class `cls`'s plane after the
 * threshold, 1: after the morphology; bits_out [n][H][ceil(W/32)].  ck_blobs_host: out [n][n_classes][cap], counts
 * [n][n_classes], status [n] (may be NULL); the camera is params.cam when has_camera.  CK_EINVAL: ck_blob_check's, a null
 * pointer, W or H < 1, W H >= 2^31, n < 0, cap < 0, a class or stage out of range. */
int ck_blob_mask_host(const ck_blob_params_t *pp, const uint8_t *rgb, int32_t W, int32_t H, int32_t n, int32_t cls, int32_t stage,
                      uint32_t *bits_out);
int ck_blobs_host(const ck_blob_params_t *pp, const uint8_t *rgb, int32_t W, int32_t H, int32_t n, ck_blob_t *out, int32_t cap,
                  int32_t *counts, uint32_t *status);
/* On the device, from the three sources of the colour preview with its validity rules and errors (ck_preview_color,
 * ck_preview_color_device, ck_preview_color_ingested): the frames behind the staged ones, raw frames in the caller's device
 * memory, a submitted slot of a raw or JPEG-colour ring.  frames [n]: indices into the source's frames (NULL: 0 .. n-1; an index may
 * repeat).  out, counts and status (may be NULL) are host or device pointers.  The camera of the bearings is the handle's
 * (ck_set_camera) if one is set, else params.cam when has_camera.  For any source the call returns the bytes of ck_blobs_host
 * given ck_blob_rgb's pixels (and that camera).  Everything runs on the handle's stream in a workspace of its own, allocated by
 * the first call and grown on demand: the staged frames, the detection workspace and the ring slots stay as they are.
 * CK_EINVAL also for cap < 0; CK_ECAPACITY for n > max_batch. */
int ck_detect_blobs(ck_handle_t *h, const ck_blob_params_t *pp, const int32_t *frames, int32_t n, ck_blob_t *out, int32_t cap,
                    int32_t *counts, uint32_t *status);
int ck_detect_blobs_device(ck_handle_t *h, const ck_blob_params_t *pp, const uint8_t *d_raw, int32_t stride, int64_t frame_pitch,
                           const ck_raw_format_t *fmt, const int32_t *frames, int32_t n_frames, int32_t n, ck_blob_t *out,
                           int32_t cap, int32_t *counts, uint32_t *status);
int ck_detect_blobs_ingested(ck_ingest_t *ing, int32_t slot, const ck_blob_params_t *pp, const int32_t *frames, int32_t n,
                             ck_blob_t *out, int32_t cap, int32_t *counts, uint32_t *status);
/* The stages, for parity: the RGB the classifier sees, rgb_out [n][H][W][3], and one class's plane at a stage, bits_out
 * [n][H][ceil(W/32)]; host or device pointers. */
int ck_blob_rgb(ck_handle_t *h, const int32_t *frames, int32_t n, uint8_t *rgb_out);
int ck_blob_rgb_device(ck_handle_t *h, const uint8_t *d_raw, int32_t stride, int64_t frame_pitch, const ck_raw_format_t *fmt,
                       const int32_t *frames, int32_t n_frames, int32_t n, uint8_t *rgb_out);
int ck_blob_mask(ck_handle_t *h, const ck_blob_params_t *pp, const int32_t *frames, int32_t n, int32_t cls, int32_t stage,
                 uint32_t *bits_out);
int ck_blob_mask_device(ck_handle_t *h, const ck_blob_params_t *pp, const uint8_t *d_raw, int32_t stride, int64_t frame_pitch,
                        const ck_raw_format_t *fmt, const int32_t *frames, int32_t n_frames, int32_t n, int32_t cls, int32_t stage,
                        uint32_t *bits_out);
/* The kernels of ck_detect_blobs_device alone, `reps` times between two events on the handle's stream: *ms_out is the mean of one
 * pass in milliseconds.  Nothing is copied out. */
int ck_blob_time(ck_handle_t *h, const ck_blob_params_t *pp, const uint8_t *d_raw, int32_t stride, int64_t frame_pitch,
                 const ck_raw_format_t *fmt, int32_t n_frames, int32_t n, int32_t reps, float *ms_out);

/* fp64 conformance probe used by the parity tests: out[i] = op(a[i], b[i]) computed on the device with
 * the same flags as the kernels. op: 0 add, 1 mul, 2 div, 3 sqrt(a), 4 a*b+c style unfused (a*b)+a. */
int ck_selftest_fp64(ck_handle_t *h, int32_t op, const double *a, const double *b, int32_t n,
                     double *out);

#ifdef __cplusplus
}
#endif
#endif /* CHALKYDRI_HIP_H */
