// chalkydri.hpp — C++17 host layer over the C ABI of libchalkydri_hip.so (include/chalkydri_hip.h).
//
// The reference's host side is Rust; this image has no Rust toolchain, so the host side above the C ABI is written in
// C++ and mirrors the reference's public surface for the hot path: same type and method names, argument meaning and
// error behaviour, so that a test written against the Rust crates reads the same here.  (INTEGRATION.md holds the
// Rust `extern "C"` shim a maintainer would drop into the reference itself.)
//
//   chalkydri::apriltags::{Detector, UnionFind}   crates/chalkydri-apriltags/src/lib.rs:42-113,142-181,191,265,291,319,480,501,663
//   chalkydri::sqpnp::SqPnP                       crates/chalkydri_sqpnp/src/lib.rs:183-222,297-304,430-437
//   chalkydri::AprilTags (+ Detection)            crates/apriltags/src/lib.rs:166-183,217-379 and the `apriltag` crate calls at :301-314
//   chalkydri::whacknet::VisionMeasurement        crates/whacknet/src/lib.rs:19-66 (64-byte wire record)
//
// Error behaviour: where the Rust code panics (`assert_eq!`, `unwrap`, `expect`) these wrappers throw
// chalkydri::Panic; where it returns `None`/skips, they return std::nullopt.  There is no CPU fallback: without a HIP
// device every constructor throws (CK_ENODEVICE).
#ifndef CHALKYDRI_HPP
#define CHALKYDRI_HPP

#include <arpa/inet.h>
#include <netinet/in.h>
#include <sys/socket.h>
#include <unistd.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "chalkydri_hip.h"

namespace chalkydri {

// A Rust panic on this path (failed assertion, unwrap on an error).  `code` is the C ABI status when there is one.
struct Panic : std::runtime_error {
    int code;
    explicit Panic(const std::string &what, int code_ = 0) : std::runtime_error(what), code(code_) {}
};
inline void check(int rc, const char *what) {
    if (rc != CK_OK) throw Panic(std::string(what) + ": " + ck_strerror(rc), rc);
}

// RAII handle: one handle = one GPU + its stream; not thread-safe, like `&mut self`.
class Handle {
  public:
    Handle(int width, int height, int max_batch, const std::vector<std::string> &families, int bits_corrected, int quad_decimate, int device) {
        ck_config_default(&cfg_, width, height, max_batch);
        cfg_.device = device;
        cfg_.quad_decimate = quad_decimate;
        cfg_.max_hamming = bits_corrected;
        cfg_.n_families = (int)families.size();
        for (size_t i = 0; i < families.size(); i++) {
            cfg_.families[i] = ck_family_builtin(families[i].c_str());
            if (!cfg_.families[i]) throw Panic("unknown tag family " + families[i]); // DetectorBuilder::add_family_bits on a bad name
        }
        check(ck_create(&cfg_, &h_), "ck_create");
    }
    ~Handle() { ck_destroy(h_); }
    Handle(const Handle &) = delete;
    Handle &operator=(const Handle &) = delete;
    ck_handle_t *get() const { return h_; }
    const ck_config_t &config() const { return cfg_; }
    // AprilTag-3's quad_sigma (chalkydri_hip.h: ck_set_quad_sigma): > 0 blurs, < 0 sharpens the quad image; may change between calls
    void set_quad_sigma(float sigma) { check(ck_set_quad_sigma(h_, sigma), "ck_set_quad_sigma"); }
    // the camera model the pose paths unproject with (chalkydri_hip.h: ck_set_camera; chalkydri::Camera::raw): while one is set, the
    // process and tag-pose calls ignore their params' OpenCVModel5.  nullptr restores it; a refused camera leaves the setting as it was
    void set_camera(const ck_camera_t *cam) { check(ck_set_camera(h_, cam), "ck_set_camera"); }
    // sub-pixel refinement of every final detection's corners inside the detect / process calls (chalkydri_hip.h:
    // ck_set_corner_subpix); nullptr = off, the default.  A refused parameter set leaves the setting as it was
    void set_corner_subpix(const ck_subpix_params_t *pp) { check(ck_set_corner_subpix(h_, pp), "ck_set_corner_subpix"); }
    // Raw camera frames (chalkydri_hip.h: ck_upload_raw) converted to luma and turned by fmt.orientation on the device, into the
    // staged frames; the handle's width x height is the ORIENTED frame, imgs carry the source's sw x sh (ck_raw_layout)
    void upload_raw(const std::vector<ck_image_u8_t> &imgs, const ck_raw_format_t &fmt) {
        check(ck_upload_raw(h_, imgs.data(), (int32_t)imgs.size(), &fmt), "ck_upload_raw");
    }
    void upload_raw_device(const uint8_t *d_raw, int n, int stride, int64_t frame_pitch, const ck_raw_format_t &fmt) {
        check(ck_upload_raw_device(h_, d_raw, n, stride, frame_pitch, &fmt), "ck_upload_raw_device");
    }
    // the same, and the oriented luma [n][height][width] back on the host
    std::vector<uint8_t> raw_luma(const std::vector<ck_image_u8_t> &imgs, const ck_raw_format_t &fmt) {
        std::vector<uint8_t> out(imgs.size() * (size_t)cfg_.width * (size_t)cfg_.height);
        check(ck_raw_luma_batch(h_, imgs.data(), (int32_t)imgs.size(), &fmt, out.data()), "ck_raw_luma_batch");
        return out;
    }
    // JPEG frames (chalkydri_hip.h: ck_upload_jpeg_oriented) decoded and turned by `orientation` (CK_ORIENT_*) on the device into
    // the staged frames; returns the per-frame CK_JPEG_* statuses.  The streams are sw x sh of the ORIENTED width x height.
    std::vector<uint32_t> upload_jpeg(const std::vector<std::vector<uint8_t>> &jpegs, int32_t orientation = CK_ORIENT_NONE) {
        std::vector<ck_jpeg_frame_t> f;
        for (const auto &j : jpegs) f.push_back({j.data(), (int64_t)j.size()});
        std::vector<uint32_t> st(f.size());
        check(ck_upload_jpeg_oriented(h_, f.data(), (int32_t)f.size(), orientation, st.data()), "ck_upload_jpeg_oriented");
        return st;
    }
    // the same luma, and the frames' chroma planes kept on the device (ck_upload_jpeg_color): preview_jpeg_color then encodes the
    // colour preview of these frames, until frames are staged another way
    std::vector<uint32_t> upload_jpeg_color(const std::vector<std::vector<uint8_t>> &jpegs, int32_t orientation = CK_ORIENT_NONE) {
        std::vector<ck_jpeg_frame_t> f;
        for (const auto &j : jpegs) f.push_back({j.data(), (int64_t)j.size()});
        std::vector<uint32_t> st(f.size());
        check(ck_upload_jpeg_color(h_, f.data(), (int32_t)f.size(), orientation, st.data()), "ck_upload_jpeg_color");
        return st;
    }
    // Coloured game pieces (chalkydri_hip.h: ck_detect_blobs) of the frames behind the staged ones: out [n][n_classes][cap] records
    // (the unwritten ones zero), counts [n][n_classes], status [n]; frames: indices into those frames, one may repeat
    struct BlobResult { std::vector<ck_blob_t> records; std::vector<int32_t> counts; std::vector<uint32_t> status; int32_t cap = 0; };
    BlobResult detect_blobs(const ck_blob_params_t &pp, const std::vector<int32_t> &frames, int32_t cap = -1) {
        BlobResult r;
        r.cap = cap < 0 ? pp.max_targets : cap;
        const size_t planes = frames.size() * (size_t)(pp.n_classes > 0 ? pp.n_classes : 1);
        r.records.assign(planes * (size_t)r.cap + 1, ck_blob_t{});
        r.counts.assign(planes + 1, 0);
        r.status.assign(frames.size() + 1, 0);
        check(ck_detect_blobs(h_, &pp, frames.data(), (int32_t)frames.size(), r.records.data(), r.cap, r.counts.data(), r.status.data()),
              "ck_detect_blobs");
        r.records.resize(planes * (size_t)r.cap); r.counts.resize(planes); r.status.resize(frames.size());
        return r;
    }

  private:
    ck_config_t cfg_{};
    ck_handle_t *h_ = nullptr;
};

// ---- coloured game pieces (chalkydri_hip.h: ck_detect_blobs) ----------------------------------------------------
// ck_blob_params_t with its defaults; class(i) is the i-th colour, add_class() appends one with the default bounds
struct BlobParams {
    ck_blob_params_t p;
    BlobParams() { ck_blob_params_default(&p); }
    ck_blob_class_t &cls(int i) { return p.cls[i]; }
    ck_blob_class_t &add_class() {
        if (p.n_classes >= CK_BLOB_MAX_CLASSES) throw Panic("at most CK_BLOB_MAX_CLASSES colour classes", CK_EINVAL);
        return p.cls[p.n_classes++];
    }
    BlobParams &hsv(int i, int h_min, int h_max, int s_min, int s_max, int v_min, int v_max) {
        ck_blob_class_t &c = p.cls[i];
        c.h_min = h_min; c.h_max = h_max; c.s_min = s_min; c.s_max = s_max; c.v_min = v_min; c.v_max = v_max;
        return *this;
    }
    BlobParams &camera(const ck_camera_t &cam) { p.cam = cam; p.has_camera = 1; return *this; }
    BlobParams &mount(const ck_iso3_t &robot_to_cam) { p.robot_to_cam = robot_to_cam; p.has_mount = 1; return *this; }
    void check_ok() const { check(ck_blob_check(&p), "ck_blob_check"); }
};
inline Handle::BlobResult detect_blobs(Handle &h, const BlobParams &pp, const std::vector<int32_t> &frames, int32_t cap = -1) {
    return h.detect_blobs(pp.p, frames, cap);
}

// ck_raw_format_t from a fourcc ("YUYV", "RGB3", "BGR ", ...) and the reference's VideoOrientation serde name
// (crates/chalkydri_core/src/config.rs:201-207): "none", "clockwise", "rotate-180", "counterclockwise"
inline int32_t orientation_code(const std::string &orientation) {
    if (orientation == "none") return CK_ORIENT_NONE;
    if (orientation == "clockwise") return CK_ORIENT_CLOCKWISE;
    if (orientation == "rotate-180") return CK_ORIENT_ROTATE_180;
    if (orientation == "counterclockwise") return CK_ORIENT_COUNTERCLOCKWISE;
    throw Panic("unknown orientation " + orientation, CK_EINVAL);
}
// planes: CK_RAW_PLANES, the chroma planes behind the luma plane of "NV12" / "NV21" / "I420" / "YV12" are part of every frame
inline ck_raw_format_t raw_format(const std::string &fourcc, const std::string &orientation = "none", bool planes = false) {
    if (fourcc.size() != 4) throw Panic("a fourcc has exactly 4 characters: " + fourcc, CK_EINVAL);
    ck_raw_format_t f{};
    for (int i = 0; i < 4; i++) f.fourcc |= (uint32_t)(uint8_t)fourcc[i] << (8 * i);
    f.orientation = orientation_code(orientation) | (planes ? CK_RAW_PLANES : 0);
    return f;
}
// the names the host layers take for a camera that delivers one JPEG per frame (not raw formats: ck_raw_layout refuses them)
inline bool is_jpeg_fourcc(const std::string &fourcc) { return fourcc == "MJPG" || fourcc == "JPEG"; }
struct RawLayout { int32_t sw = 0, sh = 0, min_stride = 0; int64_t min_bytes = 0; };
// source geometry of an oriented width x height frame (no device needed); throws for a fourcc outside the table
inline RawLayout raw_layout(const ck_raw_format_t &fmt, int width, int height) {
    RawLayout l;
    check(ck_raw_layout(&fmt, width, height, &l.sw, &l.sh, &l.min_stride, &l.min_bytes), "ck_raw_layout");
    return l;
}
// where the samples of a planar frame (a format with CK_RAW_PLANES) of row stride `stride` lie (no device needed)
inline ck_raw_planes_t raw_plane_layout(const ck_raw_format_t &fmt, int width, int height, int stride) {
    ck_raw_planes_t p{};
    check(ck_raw_plane_layout(&fmt, width, height, stride, &p), "ck_raw_plane_layout");
    return p;
}

// What the reference reads from an `apriltag::Detection` (crates/apriltags/src/lib.rs:306-314).
class Detection {
  public:
    explicit Detection(const ck_detection_t &d) : d_(d) {}
    size_t id() const { return (size_t)d_.id; }
    size_t hamming() const { return (size_t)d_.hamming; }
    float decision_margin() const { return d_.decision_margin; }
    std::array<double, 2> center() const { return {d_.c[0], d_.c[1]}; }
    std::array<std::array<double, 2>, 4> corners() const {
        return {{{d_.p[0][0], d_.p[0][1]}, {d_.p[1][0], d_.p[1][1]}, {d_.p[2][0], d_.p[2][1]}, {d_.p[3][0], d_.p[3][1]}}};
    }
    const ck_detection_t &raw() const { return d_; }

  private:
    ck_detection_t d_;
};

// ---- per-tag pose (chalkydri_hip.h: ck_estimate_tag_poses / ck_last_tag_poses), AprilTag-3's estimate_tag_pose ----------
// What `apriltag::TagParams {tagsize, fx, fy, cx, cy}` carries; the OpenCV-5 distortion stays zero (pinhole) unless set.
inline ck_tag_pose_params_t tag_pose_params(double fx, double fy, double cx, double cy, double tagsize = 0.1651, int n_iters = 50) {
    ck_tag_pose_params_t pp;
    ck_tag_pose_params_default(&pp);
    pp.cam.fx = fx; pp.cam.fy = fy; pp.cam.cx = cx; pp.cam.cy = cy;
    for (double &s : pp.tagsize) s = tagsize;
    pp.n_iters = n_iters;
    return pp;
}

// One pose record: tag -> camera (camera x right, y down, z forward), the lower-error minimum first.
class TagPose {
  public:
    explicit TagPose(const ck_tag_pose_t &r) : r_(r) {}
    bool valid() const { return r_.valid != 0; }
    std::array<double, 9> rotation() const { std::array<double, 9> a; std::copy(r_.R, r_.R + 9, a.begin()); return a; }
    std::array<double, 3> translation() const { return {r_.t[0], r_.t[1], r_.t[2]}; }
    double error() const { return r_.err; }
    bool has_alternative() const { return r_.has_alt != 0; }
    std::array<double, 9> alternative_rotation() const { std::array<double, 9> a; std::copy(r_.R_alt, r_.R_alt + 9, a.begin()); return a; }
    std::array<double, 3> alternative_translation() const { return {r_.t_alt[0], r_.t_alt[1], r_.t_alt[2]}; }
    double alternative_error() const { return r_.err_alt; }
    // err / err_alt: near 1 when both minima explain the corners equally well (an ambiguous view); 0 without an alternative
    double ambiguity() const { return r_.has_alt && r_.err_alt > 0 ? r_.err / r_.err_alt : 0.0; }
    const ck_tag_pose_t &raw() const { return r_; }

  private:
    ck_tag_pose_t r_;
};

inline std::vector<TagPose> estimate_tag_poses(Handle &h, const ck_tag_pose_params_t &pp, const std::vector<Detection> &dets) {
    std::vector<ck_detection_t> in;
    for (const Detection &d : dets) in.push_back(d.raw());
    std::vector<ck_tag_pose_t> out(in.size() ? in.size() : 1);
    check(ck_estimate_tag_poses(h.get(), &pp, in.data(), (int32_t)in.size(), out.data()), "ck_estimate_tag_poses");
    std::vector<TagPose> r;
    for (size_t i = 0; i < in.size(); i++) r.emplace_back(out[i]);
    return r;
}

// Poses of the detections the handle's last detect / process call produced, per frame of that call.
inline std::vector<std::vector<TagPose>> last_tag_poses(Handle &h, const ck_tag_pose_params_t &pp, int cap_per_frame = 64) {
    const int nb = h.config().max_batch;
    std::vector<ck_tag_pose_t> out((size_t)nb * cap_per_frame);
    std::vector<int32_t> counts((size_t)nb, -1); // one count per frame of the last call is written: the rest stay -1
    check(ck_last_tag_poses(h.get(), &pp, out.data(), cap_per_frame, counts.data()), "ck_last_tag_poses");
    std::vector<std::vector<TagPose>> r;
    for (int f = 0; f < nb && counts[f] >= 0; f++) {
        r.emplace_back();
        for (int k = 0; k < counts[f]; k++) r.back().emplace_back(out[(size_t)f * cap_per_frame + k]);
    }
    return r;
}

// ---- baseline JPEG (MJPEG) luma decode on the device (chalkydri_hip.h: ck_jpeg_info / ck_upload_jpeg / ck_jpeg_luma_batch) ----
// The frames an `image/jpeg` appsink hands over (crates/chalkydri/src/cameras/pipeline.rs:43-44,123-124), decoded to the luma
// the detector stages, bit-identical to libjpeg's islow IDCT.  Statuses are the CK_JPEG_* bits per frame.
inline std::optional<ck_jpeg_info_t> jpeg_info(const std::vector<uint8_t> &jpeg) {
    ck_jpeg_info_t info{};
    if (ck_jpeg_info(jpeg.data(), (int64_t)jpeg.size(), &info) != CK_OK) return std::nullopt;
    return info;
}
inline std::vector<ck_jpeg_frame_t> jpeg_frames(const std::vector<std::vector<uint8_t>> &jpegs) {
    std::vector<ck_jpeg_frame_t> f;
    for (const auto &j : jpegs) f.push_back({j.data(), (int64_t)j.size()});
    return f;
}
// Stages the decoded luma (ck_detect_uploaded / ck_process_uploaded follow); returns the per-frame statuses.
inline std::vector<uint32_t> upload_jpeg(Handle &h, const std::vector<std::vector<uint8_t>> &jpegs) {
    std::vector<ck_jpeg_frame_t> f = jpeg_frames(jpegs);
    std::vector<uint32_t> st(f.size());
    check(ck_upload_jpeg(h.get(), f.data(), (int32_t)f.size(), st.data()), "ck_upload_jpeg");
    return st;
}
// The same, and the luma itself: [n][height][width].
inline std::vector<uint8_t> decode_jpeg(Handle &h, const std::vector<std::vector<uint8_t>> &jpegs, std::vector<uint32_t> *status = nullptr) {
    std::vector<ck_jpeg_frame_t> f = jpeg_frames(jpegs);
    std::vector<uint8_t> out((size_t)f.size() * h.config().width * h.config().height);
    std::vector<uint32_t> st(f.size());
    check(ck_jpeg_luma_batch(h.get(), f.data(), (int32_t)f.size(), out.data(), st.data()), "ck_jpeg_luma_batch");
    if (status) *status = st;
    return out;
}
// ... turned by `orientation` (CK_ORIENT_*; the handle's geometry is the oriented frame): [n][height][width]
inline std::vector<uint8_t> decode_jpeg(Handle &h, const std::vector<std::vector<uint8_t>> &jpegs, int32_t orientation, std::vector<uint32_t> *status = nullptr) {
    std::vector<ck_jpeg_frame_t> f = jpeg_frames(jpegs);
    std::vector<uint8_t> out((size_t)f.size() * h.config().width * h.config().height);
    std::vector<uint32_t> st(f.size());
    check(ck_jpeg_luma_batch_oriented(h.get(), f.data(), (int32_t)f.size(), orientation, out.data(), st.data()), "ck_jpeg_luma_batch_oriented");
    if (status) *status = st;
    return out;
}

// ---- JPEG preview of the staged frames, encoded on the device (chalkydri_hip.h: ck_preview_jpeg / ck_preview_luma) -------------
// The reference's driver-station stream (crates/chalkydri/src/cameras/mjpeg.rs): scale to 640 x 480, JPEG at quality 50, multipart
// framing.  frames: indices into the staged frames; the files equal libjpeg's byte for byte.
inline ck_preview_params_t preview_params(int width = 640, int height = 480, int quality = 50, int restart_rows = 0, bool overlay = false) {
    ck_preview_params_t pp;
    ck_preview_params_default(&pp);
    pp.width = width; pp.height = height; pp.quality = quality; pp.restart_rows = restart_rows; pp.overlay = overlay ? 1 : 0;
    return pp;
}
// The files of one of the preview entry points: `encode(out, cap, sizes)` is the call, `bound` its layout's upper bound.
template <typename Encode>
inline std::vector<std::vector<uint8_t>> preview_files(size_t n, int64_t first_cap, int64_t bound, Encode encode) {
    // slots sized for the pixels themselves first (a file beyond that is noise at the highest qualities); the bound if one did not fit
    int64_t cap = std::min<int64_t>(bound, first_cap);
    std::vector<uint8_t> out;
    std::vector<int64_t> sizes(n);
    for (;;) {
        out.resize(n * (size_t)cap);
        encode(out.data(), cap, sizes.data());
        bool fits = true;
        for (size_t i = 0; i < n; i++) fits = fits && sizes[i] <= cap;
        if (fits || cap == bound) break;
        cap = bound;
    }
    std::vector<std::vector<uint8_t>> files(n);
    for (size_t i = 0; i < n; i++) files[i].assign(out.begin() + i * (size_t)cap, out.begin() + i * (size_t)cap + (size_t)sizes[i]);
    return files;
}
inline std::vector<std::vector<uint8_t>> preview_jpeg(Handle &h, const std::vector<int32_t> &frames, const ck_preview_params_t &pp) {
    int64_t bound = 0;
    int32_t pw = 0, ph = 0;
    check(ck_preview_layout(&pp, h.config().width, h.config().height, &pw, &ph, &bound), "ck_preview_layout");
    return preview_files(frames.size(), (int64_t)pw * ph + 1024, bound, [&](uint8_t *out, int64_t cap, int64_t *sizes) {
        check(ck_preview_jpeg(h.get(), &pp, frames.data(), (int32_t)frames.size(), out, cap, sizes, nullptr), "ck_preview_jpeg");
    });
}
// The same in colour (chalkydri_hip.h: ck_preview_jpeg_color): three-component files of the raw frames the handle's last
// ck_upload_raw left on the device (a packed colour format); frames: indices into those.
inline std::vector<std::vector<uint8_t>> preview_jpeg_color(Handle &h, const std::vector<int32_t> &frames, const ck_preview_params_t &pp) {
    int64_t bound = 0;
    int32_t pw = 0, ph = 0;
    check(ck_preview_color_layout(&pp, h.config().width, h.config().height, &pw, &ph, &bound), "ck_preview_color_layout");
    return preview_files(frames.size(), 3 * (int64_t)pw * ph + 1024, bound, [&](uint8_t *out, int64_t cap, int64_t *sizes) {
        check(ck_preview_jpeg_color(h.get(), &pp, frames.data(), (int32_t)frames.size(), out, cap, sizes, nullptr), "ck_preview_jpeg_color");
    });
}
// The scaled (+ overlaid) pixels the encoder is given: [n][ph][pw]; pw / ph come back through the pointers.
inline std::vector<uint8_t> preview_luma(Handle &h, const std::vector<int32_t> &frames, const ck_preview_params_t &pp, int32_t *pw = nullptr,
                                         int32_t *ph = nullptr) {
    int32_t w = 0, hh = 0;
    check(ck_preview_layout(&pp, h.config().width, h.config().height, &w, &hh, nullptr), "ck_preview_layout");
    std::vector<uint8_t> out(frames.size() * (size_t)w * (size_t)hh);
    check(ck_preview_luma(h.get(), &pp, frames.data(), (int32_t)frames.size(), out.data()), "ck_preview_luma");
    if (pw) *pw = w;
    if (ph) *ph = hh;
    return out;
}
// One part of the multipart stream (mjpeg.rs:122-128): boundary, length and content type in front of a complete JPEG.
inline std::vector<uint8_t> mjpeg_part(const std::vector<uint8_t> &jpeg) {
    const std::string head = "--frame\r\nContent-Length: " + std::to_string(jpeg.size()) + "\r\nContent-Type: image/jpeg\r\n\r\n";
    std::vector<uint8_t> out(head.begin(), head.end());
    out.insert(out.end(), jpeg.begin(), jpeg.end());
    return out;
}

// ---- exposure metering of the staged frames on the device (chalkydri_hip.h: ck_exposure_stats / ck_exposure_recommend) ----------
// The loop the reference leaves open (Camera.auto_exposure, crates/chalkydri_core/src/config.rs:64-65; the V4L2 controls commented
// out in crates/chalkydri/src/cameras/pipeline.rs:237-245): the device histograms the gradients of every staged frame under seven
// gamma curves, the host turns them into the exposure to set next.  Driving the camera stays the caller's part.
inline ck_exposure_params_t exposure_params() {
    ck_exposure_params_t p;
    ck_exposure_params_default(&p);
    return p;
}
// One record per entry of `frames` (indices into the staged frames); roi: empty = whole frames, else one rectangle per entry.
inline std::vector<ck_exposure_stats_t> exposure_stats(Handle &h, const std::vector<int32_t> &frames, const ck_exposure_params_t &p,
                                                       const std::vector<ck_rect_t> &roi = {}) {
    if (!roi.empty() && roi.size() != frames.size()) throw Panic("exposure_stats: one rectangle per frame", CK_EINVAL);
    std::vector<ck_exposure_stats_t> out(frames.size() ? frames.size() : 1);
    check(ck_exposure_stats(h.get(), frames.data(), (int32_t)frames.size(), &p, roi.empty() ? nullptr : roi.data(), out.data()), "ck_exposure_stats");
    out.resize(frames.size());
    return out;
}
// Keeps one camera's exposure (in the caller's unit: a V4L2 exposure_time_absolute, milliseconds, a gain) and moves it by what
// every metered frame recommends.
class ExposureController {
  public:
    explicit ExposureController(double exposure0, const ck_exposure_params_t &p = exposure_params()) : p_(p), exposure_(exposure0) {
        uint8_t lut[CK_EXPOSURE_GAMMAS * 256];
        check(ck_exposure_luts(&p_, lut), "ck_exposure_luts"); // (refuses bad parameters here, not at the first frame)
        if (!(exposure0 > 0) || !std::isfinite(exposure0)) throw Panic("ExposureController: exposure must be positive", CK_EINVAL);
    }
    double update(const ck_exposure_stats_t &s) {
        double next = exposure_;
        check(ck_exposure_recommend(&p_, &s, exposure_, &next, &gamma_hat_), "ck_exposure_recommend");
        return exposure_ = next;
    }
    double exposure() const { return exposure_; }
    double gamma_hat() const { return gamma_hat_; } // of the last update: below 1 = the frame wanted brightening
    const ck_exposure_params_t &params() const { return p_; }
    // The rectangle to meter next: the bounding box of a frame's detections grown by `margin` pixels and clamped to the frame, or
    // the whole frame when there are none.
    static ck_rect_t roi_from_detections(const std::vector<Detection> &dets, int margin, int w, int h) {
        if (dets.empty()) return {0, 0, w, h};
        double x0 = 1e300, y0 = 1e300, x1 = -1e300, y1 = -1e300;
        for (const Detection &d : dets)
            for (const auto &c : d.corners()) {
                x0 = std::min(x0, c[0]); x1 = std::max(x1, c[0]);
                y0 = std::min(y0, c[1]); y1 = std::max(y1, c[1]);
            }
        const auto clampi = [](double v, int hi) { return (int32_t)std::min<double>(std::max<double>(v, 0), hi); };
        return {clampi(std::floor(x0) - margin, w), clampi(std::floor(y0) - margin, h), clampi(std::floor(x1) + 1 + margin, w),
                clampi(std::floor(y1) + 1 + margin, h)};
    }

  private:
    ck_exposure_params_t p_;
    double exposure_, gamma_hat_ = 1.0;
};

// ---- iterative tri-class Otsu threshold (chalkydri_hip.h: ck_tri_otsu_solve / ck_cat_tri_otsu_batch) -------------
inline ck_tri_otsu_params_t tri_otsu_params() {
    ck_tri_otsu_params_t p;
    ck_tri_otsu_params_default(&p);
    return p;
}
struct TriOtsu {
    ck_tri_otsu_info_t info;
    std::array<uint8_t, 256> lut; // Color of every gray level
};
// The record and the table of one 256-bin histogram, on the host (no device needed)
inline TriOtsu tri_otsu_solve(const std::array<uint32_t, 256> &hist, const ck_tri_otsu_params_t &p = tri_otsu_params()) {
    TriOtsu r;
    check(ck_tri_otsu_solve(&p, hist.data(), &r.info, r.lut.data()), "ck_tri_otsu_solve");
    return r;
}

namespace apriltags {

enum class Color : uint8_t { Black = 0, White = 1, Other = 2 }; // src/utils.rs:2-6

// src/utils.rs helpers (crate-private in the reference and, except grayscale, unused by its pipeline; kept under the same names).
namespace utils {
// utils.rs:33-46: trunc(fma(r, .33f, fma(g, .33f, b * .33f))), saturating cast
inline uint8_t grayscale(uint8_t r, uint8_t g, uint8_t b) {
    float v = std::fmaf((float)r, 0.33f, std::fmaf((float)g, 0.33f, (float)b * 0.33f));
    return v >= 255.0f ? 255 : (v <= 0.0f ? 0 : (uint8_t)v);
}
// utils.rs:51-72: FAST ring position 1..16 -> degrees
inline float fast_angle(uint8_t p) {
    if (p < 1 || p > 16) throw Panic("invalid FAST point", CK_EINVAL);
    return (float)(p - 1) * 22.5f;
}
enum class Orientation { Collinear, Clockwise, Counterclockwise }; // utils.rs:74-79
using Point = std::pair<size_t, size_t>;
// utils.rs:82-101
inline Orientation orientation(Point p, Point q, Point r) {
    int32_t v = ((int32_t)q.second - (int32_t)p.second) * ((int32_t)r.first - (int32_t)q.first) -
                ((int32_t)q.first - (int32_t)p.first) * ((int32_t)r.second - (int32_t)q.second);
    return v == 0 ? Orientation::Collinear : (v > 0 ? Orientation::Clockwise : Orientation::Counterclockwise);
}
// utils.rs:113-152: gift wrapping from the left-most point
struct PresentWrapper {
    static std::vector<Point> find_convex_hull(const std::vector<Point> &points) {
        if (points.empty()) throw Panic("index out of bounds: find_convex_hull of no points", CK_EINVAL);
        size_t l = 0, n = points.size();
        for (size_t i = 0; i < n; i++)
            if (points[i].first < points[l].first) l = i;
        std::vector<Point> hull;
        size_t p = l;
        while (p != l || hull.empty()) {
            hull.push_back(points[p]);
            size_t q = (p + 1) % n;
            for (size_t i = 0; i < n; i++)
                if (orientation(points[p], points[i], points[q]) == Orientation::Counterclockwise) q = i;
            p = q;
            if (hull.size() > n) break; // degenerate (collinear duplicate) input: stop where the walk starts repeating
        }
        return hull;
    }
};
} // namespace utils

// Result of Detector::connected_components (lib.rs:42-113).  The device returns the forest already flattened:
// find() is the canonical root (smallest index of the set), get_size() the size of the set.
class UnionFind {
  public:
    UnionFind(std::vector<uint32_t> roots, std::vector<uint32_t> sizes) : parent_(std::move(roots)), size_(std::move(sizes)) {}
    explicit UnionFind(size_t len) : parent_(len), size_(len, 1) { // UnionFind::new: singletons (lib.rs:49-65)
        for (size_t i = 0; i < len; i++) parent_[i] = (uint32_t)i;
    }
    size_t find(size_t id) { // lib.rs:67-76 (path compression)
        size_t r = id;
        while (parent_[r] != r) r = parent_[r];
        while (parent_[id] != r) { size_t n = parent_[id]; parent_[id] = (uint32_t)r; id = n; }
        return r;
    }
    void union_(size_t id1, size_t id2) { // lib.rs:78-94: by size, ties keep root1
        size_t r1 = find(id1), r2 = find(id2);
        if (r1 == r2) return;
        if (size_[r1] < size_[r2]) std::swap(r1, r2);
        parent_[r2] = (uint32_t)r1;
        size_[r1] += size_[r2];
    }
    size_t get_size(size_t id) const { // lib.rs:96-98: size stored at `id` (meaningful at roots, as in the reference)
        return size_[id];
    }
    size_t len() const { return parent_.size(); }

  private:
    std::vector<uint32_t> parent_, size_;
};

// chalkydri_apriltags::Detector — the experimental front-end ("CAT"), plus `detect`/`detect_batch` which the Rust shim adds
// because CAT itself exposes no IDs or corners.
class Detector {
  public:
    Detector(size_t width, size_t height, const std::vector<size_t> &valid_tags, int device = 0, int max_batch = 1)
        : width_(width), height_(height), valid_tags_(valid_tags), device_(device), max_batch_(max_batch),
          h_(std::make_shared<Handle>((int)width, (int)height, max_batch, std::vector<std::string>{"tag36h11"}, 3, 1, device)),
          buf_(width * height, (uint8_t)Color::Black) {} // alloc_zeroed: all Black (lib.rs:166-167)

    // Clone = a fresh detector of the same size with no valid tags (lib.rs:663-667)
    Detector clone() const { return Detector(width_, height_, {}, device_, max_batch_); }

    size_t width() const { return width_; }
    size_t height() const { return height_; }
    const std::vector<uint8_t> &buf() const { return buf_; }                             // Color per pixel
    const std::vector<std::pair<size_t, size_t>> &points() const { return points_; }      // (x, y), x-major order
    const std::vector<std::array<size_t, 4>> &lines() const { return lines_; }            // (x1, y1, x2, y2)

    // lib.rs:191-259.  `input` is RGB8 [h][w][3].
    void calc_otsu(std::vector<uint8_t> &input) {
        need_rgb(input.size());
        check(ck_cat_calc_otsu(h_->get(), input.data(), (int)width_, (int)height_, buf_.data()), "ck_cat_calc_otsu");
    }
    // The threshold the CAT design document asks for (book/src/maintenance/apriltags.md:33) in calc_otsu's place: iterative
    // tri-class Otsu of the frame's gray levels.  `input` is [h][w][p.channels]; returns the frame's record.
    ck_tri_otsu_info_t tri_otsu(const std::vector<uint8_t> &input, const ck_tri_otsu_params_t &p = tri_otsu_params()) {
        if (input.size() != width_ * height_ * (size_t)p.channels) throw Panic("input is not width*height*channels bytes", CK_EINVAL);
        ck_tri_otsu_info_t info;
        check(ck_cat_tri_otsu_batch(h_->get(), &p, input.data(), 1, (int)width_, (int)height_, buf_.data(), &info, nullptr), "ck_cat_tri_otsu_batch");
        return info;
    }
    // lib.rs:319-334
    void thresh(const std::vector<uint8_t> &input) {
        need_rgb(input.size());
        check(ck_cat_thresh(h_->get(), input.data(), (int)width_, (int)height_, buf_.data()), "ck_cat_thresh");
    }
    // lib.rs:265-287: panics unless input.len() == width*height*3
    void process_frame(const std::vector<uint8_t> &input) {
        if (input.size() != width_ * height_ * 3) throw Panic("assertion `left == right` failed: input.len() == width * height * 3", CK_EINVAL);
        std::vector<uint32_t> pts(2 * point_cap()), lines(4 * line_cap_);
        int32_t np = 0, nl = 0;
        check(ck_cat_process_frame(h_->get(), input.data(), input.size(), (int)width_, (int)height_, buf_.data(), pts.data(), (int)point_cap(), &np,
                                   lines.data(), (int)line_cap_, &nl),
              "ck_cat_process_frame");
        store_points(pts, np);
        store_lines(lines, nl);
    }
    // lib.rs:291-309
    void detect_corners() {
        std::vector<uint32_t> pts(2 * point_cap());
        int32_t np = 0;
        check(ck_cat_detect_corners(h_->get(), buf_.data(), (int)width_, (int)height_, pts.data(), (int)point_cap(), &np), "ck_cat_detect_corners");
        store_points(pts, np);
    }
    // lib.rs:480-499
    void check_edges() {
        std::vector<uint32_t> pts(2 * points_.size() + 2), lines(4 * line_cap_);
        for (size_t i = 0; i < points_.size(); i++) { pts[2 * i] = (uint32_t)points_[i].first; pts[2 * i + 1] = (uint32_t)points_[i].second; }
        int32_t nl = 0;
        check(ck_cat_check_edges(h_->get(), buf_.data(), (int)width_, (int)height_, pts.data(), (int)points_.size(), lines.data(), (int)line_cap_, &nl),
              "ck_cat_check_edges");
        store_lines(lines, nl);
    }
    // lib.rs:501-549
    UnionFind connected_components() const {
        std::vector<uint32_t> roots(width_ * height_), sizes(width_ * height_);
        check(ck_cat_connected_components(h_->get(), buf_.data(), (int)width_, (int)height_, roots.data(), sizes.data()), "ck_cat_connected_components");
        return UnionFind(std::move(roots), std::move(sizes));
    }
    // lib.rs:615-661 writes lines.png for debugging; here: the lines whose end points share a component, returned instead of drawn
    std::vector<std::array<size_t, 4>> draw() const {
        UnionFind uf = connected_components();
        std::vector<std::array<size_t, 4>> out;
        for (const auto &l : lines_)
            if (uf.find(l[1] * width_ + l[0]) == uf.find(l[3] * width_ + l[2])) out.push_back(l);
        return out;
    }

    // Added by the shim: the production detector on a mono8 frame (stride in bytes, >= width).
    std::vector<Detection> detect(const uint8_t *mono8, size_t stride) {
        ck_image_u8_t img{const_cast<uint8_t *>(mono8), (int32_t)width_, (int32_t)height_, (int32_t)stride};
        std::vector<ck_detection_t> dets(det_cap_);
        int32_t n = 0;
        uint32_t st = 0;
        check(ck_detect_batch(h_->get(), &img, 1, dets.data(), (int)det_cap_, &n, &st), "ck_detect_batch");
        std::vector<Detection> out;
        for (int i = 0; i < n && i < (int)det_cap_; i++) out.emplace_back(dets[i]);
        return out;
    }
    std::vector<std::vector<Detection>> detect_batch(const std::vector<ck_image_u8_t> &imgs) {
        if ((int)imgs.size() > max_batch_) throw Panic("detect_batch: more frames than max_batch", CK_EINVAL);
        std::vector<ck_detection_t> dets(det_cap_ * imgs.size());
        std::vector<int32_t> counts(imgs.size());
        std::vector<uint32_t> st(imgs.size());
        check(ck_detect_batch(h_->get(), imgs.data(), (int)imgs.size(), dets.data(), (int)det_cap_, counts.data(), st.data()), "ck_detect_batch");
        std::vector<std::vector<Detection>> out(imgs.size());
        for (size_t f = 0; f < imgs.size(); f++)
            for (int i = 0; i < counts[f] && i < (int)det_cap_; i++) out[f].emplace_back(dets[f * det_cap_ + i]);
        return out;
    }
    // The decode stage alone on the caller's quads (ck_decode_quads_batch), one list per frame; `status` gets the frames' words.
    // No images: the frames staged on the handle (imgs == NULL), one per list of quads.
    std::vector<std::vector<Detection>> decode_quads(const std::vector<ck_image_u8_t> &imgs, const std::vector<std::vector<ck_quad_t>> &quads,
                                                     std::vector<uint32_t> *status = nullptr) {
        if (!imgs.empty() && imgs.size() != quads.size()) throw Panic("decode_quads: one list of quads per frame", CK_EINVAL);
        const size_t n = quads.size();
        size_t stride = 1;
        for (const auto &q : quads) stride = std::max(stride, q.size());
        std::vector<ck_quad_t> flat(stride * quads.size());
        std::vector<int32_t> nq(quads.size()), counts(quads.size());
        for (size_t f = 0; f < quads.size(); f++) {
            nq[f] = (int32_t)quads[f].size();
            std::copy(quads[f].begin(), quads[f].end(), flat.begin() + f * stride);
        }
        std::vector<ck_detection_t> dets(det_cap_ * n);
        std::vector<uint32_t> st(n);
        check(ck_decode_quads_batch(h_->get(), imgs.empty() ? nullptr : imgs.data(), (int)n, flat.data(), (int)stride, nq.data(), dets.data(), (int)det_cap_,
                                    counts.data(), st.data()),
              "ck_decode_quads_batch");
        std::vector<std::vector<Detection>> out(n);
        for (size_t f = 0; f < n; f++)
            for (int i = 0; i < counts[f] && i < (int)det_cap_; i++) out[f].emplace_back(dets[f * det_cap_ + i]);
        if (status) *status = st;
        return out;
    }

  private:
    void need_rgb(size_t len) const {
        if (len != width_ * height_ * 3) throw Panic("input is not width*height*3 bytes", CK_EINVAL);
    }
    size_t point_cap() const { return width_ * height_; } // the reference's points buffer holds one entry per pixel (lib.rs:168-169)
    void store_points(const std::vector<uint32_t> &pts, int32_t n) {
        points_.clear();
        for (int32_t i = 0; i < n; i++) points_.emplace_back(pts[2 * i], pts[2 * i + 1]);
    }
    void store_lines(const std::vector<uint32_t> &l, int32_t n) {
        lines_.clear();
        for (int32_t i = 0; i < n && (size_t)i < line_cap_; i++) lines_.push_back({l[4 * i], l[4 * i + 1], l[4 * i + 2], l[4 * i + 3]});
    }
    size_t width_, height_;
    std::vector<size_t> valid_tags_; // stored, never read — as in the reference (lib.rs:145)
    int device_, max_batch_;
    std::shared_ptr<Handle> h_;
    std::vector<uint8_t> buf_;
    std::vector<std::pair<size_t, size_t>> points_;
    std::vector<std::array<size_t, 4>> lines_;
    size_t line_cap_ = 1 << 20, det_cap_ = 256;
};

} // namespace apriltags

namespace sqpnp {

using Vec3 = std::array<double, 3>;
using Rot3 = std::array<double, 9>; // row-major 3x3
struct Iso3 {                       // nalgebra Isometry3<f64>: translation + unit quaternion (w, x, y, z)
    Vec3 translation{0, 0, 0};
    std::array<double, 4> rotation{1, 0, 0, 0};
    ck_iso3_t raw() const {
        ck_iso3_t r;
        std::memcpy(r.t, translation.data(), sizeof r.t);
        std::memcpy(r.q, rotation.data(), sizeof r.q);
        return r;
    }
    static Iso3 from_raw(const ck_iso3_t &r) {
        Iso3 o;
        std::memcpy(o.translation.data(), r.t, sizeof r.t);
        std::memcpy(o.rotation.data(), r.q, sizeof r.q);
        return o;
    }
};

// chalkydri_sqpnp::SqPnP (lib.rs:183-222): builder-style `max_iter` / `tolerance`, `solve_robot_pose`,
// `create_solver_camera_transform`.  The solve runs on the device (one wave per problem).
class SqPnP {
  public:
    explicit SqPnP(int device = 0) : h_(std::make_shared<Handle>(64, 64, 1, std::vector<std::string>{"tag36h11"}, 3, 1, device)) {
        ck_sqpnp_params_default(&prm_); // max_iter 15, tol_sq 1e-16 (lib.rs:201-212)
    }
    SqPnP &max_iter(size_t n) { prm_.max_iter = (int32_t)n; return *this; }          // lib.rs:214-217
    SqPnP &tolerance(double tol) { prm_.tol_sq = tol * tol; return *this; }          // lib.rs:219-222

    // lib.rs:297-377.  Returns (pivoted rotation, pivoted position, std devs) or nullopt where the reference returns None.
    std::optional<std::tuple<Rot3, Vec3, Vec3>> solve_robot_pose(const std::vector<Iso3> &points_isometry, const std::vector<Vec3> &points_2d,
                                                                const Iso3 &robot_to_cam, double gyro, double sign_change_error) {
        std::vector<ck_iso3_t> tags;
        for (const auto &t : points_isometry) tags.push_back(t.raw());
        std::vector<double> b;
        for (const auto &v : points_2d) b.insert(b.end(), v.begin(), v.end());
        ck_sqpnp_problem_t pb{};
        pb.n_tags = (int32_t)tags.size(); pb.n_bearings = (int32_t)points_2d.size();
        pb.tag_offset = 0; pb.bearing_offset = 0;
        pb.robot_to_cam = robot_to_cam.raw(); pb.gyro = gyro; pb.sign_change_error = sign_change_error;
        ck_sqpnp_result_t res{};
        ck_iso3_t dummy_tag{};
        double dummy_b[3] = {0, 0, 1};
        check(ck_sqpnp_solve_batch(h_->get(), &prm_, &pb, 1, tags.empty() ? &dummy_tag : tags.data(), (int32_t)tags.size(),
                                   b.empty() ? dummy_b : b.data(), (int32_t)points_2d.size(), &res),
              "ck_sqpnp_solve_batch");
        if (!res.valid) return std::nullopt;
        Rot3 R; Vec3 p, s;
        std::memcpy(R.data(), res.rot, sizeof res.rot);
        std::memcpy(p.data(), res.pos, sizeof res.pos);
        std::memcpy(s.data(), res.std_devs, sizeof res.std_devs);
        last_yaw_ = res.yaw;
        return std::make_tuple(R, p, s);
    }
    // euler_angles().2 of the last returned rotation — what the caller publishes (crates/apriltags/src/lib.rs:343)
    double last_yaw() const { return last_yaw_; }

    // lib.rs:430-461
    static Iso3 create_solver_camera_transform(double fwd_m, double left_m, double up_m, double roll_deg, double pitch_deg, double yaw_deg) {
        ck_iso3_t o;
        ck_sqpnp_create_solver_camera_transform(fwd_m, left_m, up_m, roll_deg, pitch_deg, yaw_deg, &o);
        return Iso3::from_raw(o);
    }

  private:
    std::shared_ptr<Handle> h_;
    ck_sqpnp_params_t prm_{};
    double last_yaw_ = 0.0;
};

} // namespace sqpnp

namespace whacknet {
// crates/whacknet/src/lib.rs:19-66 — the 64-byte record sent as one datagram
using VisionMeasurement = ck_vision_measurement_t;
static_assert(sizeof(VisionMeasurement) == 64, "wire record is 64 bytes (crates/whacknet/src/lib.rs:92-95)");

// WhacknetClient (lib.rs:68-89): a UDP socket bound to 0.0.0.0:0 and connected to the roboRIO; send() puts the 64 raw
// bytes of one measurement on the wire as one datagram, so a consumer cannot tell which backend produced it.
class WhacknetClient {
  public:
    explicit WhacknetClient(const std::string &remote_ip = "10.45.33.2", uint16_t remote_port = 7001) { // REMOTE_ADDR, lib.rs:14
        fd_ = ::socket(AF_INET, SOCK_DGRAM, 0);
        if (fd_ < 0) throw Panic("whacknet: socket() failed");
        sockaddr_in local{};
        local.sin_family = AF_INET; local.sin_addr.s_addr = htonl(INADDR_ANY); local.sin_port = 0;            // BIND_ADDR, lib.rs:13
        sockaddr_in remote{};
        remote.sin_family = AF_INET; remote.sin_port = htons(remote_port);
        if (::bind(fd_, reinterpret_cast<sockaddr *>(&local), sizeof local) != 0 || ::inet_pton(AF_INET, remote_ip.c_str(), &remote.sin_addr) != 1 ||
            ::connect(fd_, reinterpret_cast<sockaddr *>(&remote), sizeof remote) != 0) {
            ::close(fd_);
            throw Panic("whacknet: bind/connect failed");
        }
    }
    ~WhacknetClient() { if (fd_ >= 0) ::close(fd_); }
    WhacknetClient(const WhacknetClient &) = delete;
    WhacknetClient &operator=(const WhacknetClient &) = delete;
    // lib.rs:83-89; false where the reference returns the io::Error
    bool send(const VisionMeasurement &m) const { return ::send(fd_, &m, sizeof m, 0) == (ssize_t)sizeof m; }

  private:
    int fd_ = -1;
};

// The gyro heading arrives as one little-endian f64 per datagram on port 7002 (lib.rs:112-130)
inline std::optional<double> decode_gyro(const uint8_t *buf, size_t len) {
    if (len < 8) return std::nullopt;
    uint64_t bits = 0;
    for (int i = 7; i >= 0; i--) bits = (bits << 8) | buf[i];
    double v;
    std::memcpy(&v, &bits, sizeof v);
    return v;
}

// Comm (lib.rs:99-185): the gyro listener and the measurement publisher, each on a thread of its own.  The listener binds
// 0.0.0.0:<gyro_port> (7002 in the reference) and stores every 8-byte datagram as the current heading; publish() queues a
// measurement for the sender thread, which puts it on the wire through a WhacknetClient.  gyro_angle() starts at 0.0 like
// the reference's `Some(0f64)`; dropping the Comm ends both threads (the reference's listener only notices on its next
// datagram; here the socket has a receive timeout so that the destructor returns).
class Comm {
  public:
    explicit Comm(uint16_t gyro_port = 7002, const std::string &remote_ip = "10.45.33.2", uint16_t remote_port = 7001)
        : client_(remote_ip, remote_port) {
        gyro_fd_ = ::socket(AF_INET, SOCK_DGRAM, 0);
        sockaddr_in local{};
        local.sin_family = AF_INET; local.sin_addr.s_addr = htonl(INADDR_ANY); local.sin_port = htons(gyro_port);
        if (gyro_fd_ < 0 || ::bind(gyro_fd_, reinterpret_cast<sockaddr *>(&local), sizeof local) != 0) {
            if (gyro_fd_ >= 0) ::close(gyro_fd_);
            throw Panic("whacknet: gyro socket bind failed"); // `.unwrap()` at lib.rs:113
        }
        socklen_t ll = sizeof local;
        ::getsockname(gyro_fd_, reinterpret_cast<sockaddr *>(&local), &ll);
        gyro_port_ = ntohs(local.sin_port);
        timeval tv{0, 100000};
        ::setsockopt(gyro_fd_, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof tv);
        listener_ = std::thread([this] {
            uint8_t buf[8];
            while (!stop_.load(std::memory_order_acquire)) {
                std::memset(buf, 0, sizeof buf);                                  // `buf = [0u8; 8]` per datagram (lib.rs:128)
                const ssize_t got = ::recv(gyro_fd_, buf, sizeof buf, 0);
                if (got < 0) continue;                                            // Err(_) => {} (lib.rs:125)
                uint64_t bits = 0;                                                // f64::from_le_bytes(buf): a short datagram leaves zero bytes
                for (int i = 7; i >= 0; i--) bits = (bits << 8) | buf[i];
                gyro_bits_.store(bits, std::memory_order_release);
            }
        });
        sender_ = std::thread([this] {
            std::unique_lock<std::mutex> lk(mu_);
            for (;;) {
                cv_.wait(lk, [this] { return !queue_.empty() || stop_.load(std::memory_order_acquire); });
                if (queue_.empty()) return;                                       // stopping and drained
                const VisionMeasurement m = queue_.front();
                queue_.pop_front();
                lk.unlock();
                client_.send(m);                                                  // `.ok()`: a failed send is dropped (lib.rs:142)
                lk.lock();
            }
        });
    }
    ~Comm() {
        stop_.store(true, std::memory_order_release);
        cv_.notify_all();
        if (sender_.joinable()) sender_.join();
        if (listener_.joinable()) listener_.join();
        ::close(gyro_fd_);
    }
    Comm(const Comm &) = delete;
    Comm &operator=(const Comm &) = delete;
    // lib.rs:154-172
    void publish(uint8_t cam_id, uint8_t tag_count, uint64_t ts, double x, double y, double rot, double std_x, double std_y, double std_rot) {
        VisionMeasurement m{};
        m.pose_x = x; m.pose_y = y; m.pose_rot = rot; m.std_x = std_x; m.std_y = std_y; m.std_rot = std_rot;
        m.ts = ts; m.camera_id = cam_id; m.tag_count = tag_count;
        publish(m);
    }
    void publish(const VisionMeasurement &m) {
        { std::lock_guard<std::mutex> lk(mu_); queue_.push_back(m); }
        cv_.notify_one();
    }
    // lib.rs:174-179: the last heading received (0.0 before the first datagram)
    std::optional<double> gyro_angle() const {
        const uint64_t bits = gyro_bits_.load(std::memory_order_acquire);
        double v;
        std::memcpy(&v, &bits, sizeof v);
        return v;
    }
    uint16_t gyro_port() const { return gyro_port_; } // the bound port (pass 0 to let the system pick one: tests)

  private:
    WhacknetClient client_;
    int gyro_fd_ = -1;
    uint16_t gyro_port_ = 0;
    std::atomic<uint64_t> gyro_bits_{0};
    std::atomic<bool> stop_{false};
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<VisionMeasurement> queue_;
    std::thread listener_, sender_;
};
} // namespace whacknet

// Pinned host slots + asynchronous upload (the pooled host buffers of the camera layer,
// crates/chalkydri/src/cameras/gst_to_cu.rs:49-72,131-188): write frames, submit the slot, process it; submitting slot
// k+1 before processing slot k overlaps its upload with the compute.
class IngestRing {
  public:
    IngestRing(const std::shared_ptr<Handle> &h, int n_slots = 2) : h_(h) { check(ck_ingest_create(h_->get(), n_slots, &g_), "ck_ingest_create"); }
    // slots of RAW frames: submit converts and orients them on the device (ck_ingest_create_raw)
    IngestRing(const std::shared_ptr<Handle> &h, int n_slots, const ck_raw_format_t &fmt) : h_(h) {
        check(ck_ingest_create_raw(h_->get(), n_slots, &fmt, &g_), "ck_ingest_create_raw");
    }
    // slots of JPEG frames, one compressed frame per index: submit decodes and orients them on the ring's copy stream
    // (ck_ingest_create_jpeg; max_frame_bytes 0 = sw * sh).  color: the slots also keep their frames' chroma planes
    // (ck_ingest_create_jpeg_color), the source of preview_jpeg_color
    struct Jpeg { int32_t orientation = CK_ORIENT_NONE; int64_t max_frame_bytes = 0; bool color = false; };
    IngestRing(const std::shared_ptr<Handle> &h, int n_slots, const Jpeg &j) : h_(h) {
        if (j.color) check(ck_ingest_create_jpeg_color(h_->get(), n_slots, j.orientation, j.max_frame_bytes, &g_), "ck_ingest_create_jpeg_color");
        else check(ck_ingest_create_jpeg(h_->get(), n_slots, j.orientation, j.max_frame_bytes, &g_), "ck_ingest_create_jpeg");
    }
    void write_jpeg(int slot, int index, const uint8_t *data, size_t size) { check(ck_ingest_write_jpeg(g_, slot, index, data, (int64_t)size), "ck_ingest_write_jpeg"); }
    void write_jpeg(int slot, int index, const std::vector<uint8_t> &jpeg) { write_jpeg(slot, index, jpeg.data(), jpeg.size()); }
    // the CK_JPEG_* words of the n frames the slot was submitted with (waits for the slot's decode)
    std::vector<uint32_t> jpeg_status(int slot, int n) {
        std::vector<uint32_t> st((size_t)std::max(n, 1));
        check(ck_ingest_jpeg_status(g_, slot, n, st.data()), "ck_ingest_jpeg_status");
        st.resize((size_t)n);
        return st;
    }
    ~IngestRing() { ck_ingest_destroy(g_); }
    IngestRing(const IngestRing &) = delete;
    IngestRing &operator=(const IngestRing &) = delete;
    int stride() const { return ck_ingest_stride(g_); }
    uint8_t *frame(int slot, int index) { return ck_ingest_frame(g_, slot, index); }
    static uint32_t fourcc(const char (&c)[5]) { return (uint32_t)(uint8_t)c[0] | ((uint32_t)(uint8_t)c[1] << 8) | ((uint32_t)(uint8_t)c[2] << 16) | ((uint32_t)(uint8_t)c[3] << 24); }
    void write(int slot, int index, const ck_image_u8_t &img, uint32_t code) { check(ck_ingest_write(g_, slot, index, &img, code), "ck_ingest_write"); }
    void submit(int slot, int n) { check(ck_ingest_submit(g_, slot, n), "ck_ingest_submit"); }
    ck_ingest_t *get() const { return g_; }
    // the colour preview of a submitted slot of a raw ring, from the slot's raw frames, or of a JPEG ring made with color
    // (ck_preview_jpeg_color_ingested)
    std::vector<std::vector<uint8_t>> preview_jpeg_color(int slot, const std::vector<int32_t> &frames, const ck_preview_params_t &pp) {
        int64_t bound = 0;
        int32_t pw = 0, ph = 0;
        check(ck_preview_color_layout(&pp, h_->config().width, h_->config().height, &pw, &ph, &bound), "ck_preview_color_layout");
        return preview_files(frames.size(), 3 * (int64_t)pw * ph + 1024, bound, [&](uint8_t *out, int64_t cap, int64_t *sizes) {
            check(ck_preview_jpeg_color_ingested(g_, slot, &pp, frames.data(), (int32_t)frames.size(), out, cap, sizes, nullptr),
                  "ck_preview_jpeg_color_ingested");
        });
    }

  private:
    std::shared_ptr<Handle> h_;
    ck_ingest_t *g_ = nullptr;
};

// A camera model (chalkydri_hip.h: ck_camera_t): what the reference's `calib` blob deserialises into
// (camera_intrinsic_model::GenericModel, lib.rs:176,256), for the three models this library has.  The factories check their
// parameters (Panic for what ck_camera_check refuses); the pixel <-> bearing functions are host arithmetic with the device's bytes.
enum class CameraModel : int32_t { OpenCv5 = CK_CAMERA_OPENCV5, Eucm = CK_CAMERA_EUCM, Ucm = CK_CAMERA_UCM };
struct Camera {
    ck_camera_t raw{};
    static Camera of(CameraModel m, std::initializer_list<double> k) {
        Camera c;
        c.raw.model = (int32_t)m;
        int i = 0;
        for (double v : k) c.raw.k[i++] = v;
        if (m == CameraModel::Ucm) c.raw.k[5] = 1.0;
        check(ck_camera_check(&c.raw), "ck_camera_check");
        return c;
    }
    static Camera opencv5(const ck_opencv5_t &c) { return of(CameraModel::OpenCv5, {c.fx, c.fy, c.cx, c.cy, c.k1, c.k2, c.p1, c.p2, c.k3}); }
    static Camera eucm(double fx, double fy, double cx, double cy, double alpha, double beta) { return of(CameraModel::Eucm, {fx, fy, cx, cy, alpha, beta}); }
    static Camera ucm(double fx, double fy, double cx, double cy, double alpha) { return of(CameraModel::Ucm, {fx, fy, cx, cy, alpha}); }
    CameraModel model() const { return (CameraModel)raw.model; }
    // px as u0 v0 u1 v1 ... -> unit bearings x0 y0 z0 ...; ok[i] = 0: no bearing (outside the model's valid disc, not converged)
    std::vector<double> unproject(const std::vector<double> &px, std::vector<uint8_t> *ok = nullptr) const {
        std::vector<double> b(px.size() / 2 * 3);
        std::vector<uint8_t> o(px.size() / 2);
        check(ck_camera_unproject_host(&raw, px.data(), (int32_t)(px.size() / 2), b.data(), o.data()), "ck_camera_unproject_host");
        if (ok) *ok = o;
        return b;
    }
    // camera points x0 y0 z0 ... -> pixels u0 v0 ...; ok[i] = 0: the point does not project
    std::vector<double> project(const std::vector<double> &xyz, std::vector<uint8_t> *ok = nullptr) const {
        std::vector<double> px(xyz.size() / 3 * 2);
        std::vector<uint8_t> o(xyz.size() / 3);
        check(ck_camera_project_host(&raw, xyz.data(), (int32_t)(xyz.size() / 3), px.data(), o.data()), "ck_camera_project_host");
        if (ok) *ok = o;
        return px;
    }
};

// crates/apriltags/src/lib.rs:185-192
struct RobotToCamOffset { double roll = 0, pitch = 0, yaw = 0, x = 0, y = 0, z = 0; };

// The AprilTags sink task (crates/apriltags/src/lib.rs:166-183,217-379): built from the task's config values, `process`
// turns one frame (+ the gyro heading, if any) into the measurement `Comm::publish` would send.
class AprilTags {
  public:
    struct Config {
        size_t width = 1280, height = 800;
        std::string family = "tag36h11";       // lib.rs:229
        size_t bits_corrected = 3;              // lib.rs:230
        ck_opencv5_t calib{};                   // "calib" JSON -> OpenCVModel5 (lib.rs:232-238)
        std::optional<Camera> camera;           // ... or another model of the blob (EUCM, UCM): set on the handle, `calib` is then ignored
        RobotToCamOffset robot_to_cam{};        // "robot_to_cam" JSON (lib.rs:240-254)
        std::map<size_t, sqpnp::Iso3> layout;   // AprilTagFieldLayout::load (field_layout.rs:18-44)
        uint8_t cam_id = 0;                     // lib.rs:256
        int device = 0, max_batch = 1, quad_decimate = 1;
        float quad_sigma = 0.0f;                // AprilTag-3 detector field; 0 = no filter
        // the camera's raw format ("" = 8-bit luma, else a fourcc of ck_raw_layout's table) and mounting: `process` then takes the
        // frames as the camera hands them over; width / height / calib are those of the ORIENTED image.  "MJPG" / "JPEG": the camera
        // delivers one JPEG per frame, which `process_jpeg` takes
        std::string fourcc;
        std::string orientation = "none";
        // "NV12" / "NV21" / "I420" / "YV12" only: the frames carry their chroma planes behind the luma plane (CK_RAW_PLANES), so the
        // colour preview and the coloured-piece detector work from the frames `process` staged
        bool raw_planes = false;
    };
    explicit AprilTags(const Config &c)
        : cfg_(c), h_(std::make_shared<Handle>((int)c.width, (int)c.height, c.max_batch, std::vector<std::string>{c.family}, (int)c.bits_corrected,
                                               c.quad_decimate, c.device)) {
        for (const auto &kv : c.layout) {
            ck_field_tag_t t{};
            t.id = (int32_t)kv.first;
            t.pose = kv.second.raw();
            field_.push_back(t);
        }
        if (c.quad_sigma != 0.0f) h_->set_quad_sigma(c.quad_sigma);
        pp_.cam = c.calib;
        if (c.camera) h_->set_camera(&c.camera->raw);
        pp_.robot_to_cam = sqpnp::SqPnP::create_solver_camera_transform(c.robot_to_cam.x, c.robot_to_cam.y, c.robot_to_cam.z, c.robot_to_cam.roll,
                                                                        c.robot_to_cam.pitch, c.robot_to_cam.yaw).raw(); // lib.rs:247-254
        pp_.field = field_.data();
        pp_.n_field = (int32_t)field_.size();
        pp_.camera_id = c.cam_id;
        pp_.sign_change_error = 600.0; // SIGN_FLIP_CONST (lib.rs:6)
        ck_sqpnp_params_default(&pp_.sqpnp);
    }

    // lib.rs:293-379 for a batch of frames: measurement i is what `comm.publish` would send for frame i; valid[i] == false
    // reproduces the paths that publish nothing but the heartbeat (no detections, unknown tags only, no gyro, solver None).
    std::vector<std::pair<whacknet::VisionMeasurement, bool>> process(const std::vector<ck_image_u8_t> &imgs, const std::vector<std::optional<double>> &gyro) {
        const int n = (int)imgs.size();
        if (n > cfg_.max_batch || gyro.size() != imgs.size()) throw Panic("process: batch larger than max_batch or gyro size mismatch", CK_EINVAL);
        if (cfg_.fourcc.empty() && cfg_.orientation == "none") check(ck_upload_frames(h_->get(), imgs.data(), n), "ck_upload_frames");
        else h_->upload_raw(imgs, raw_format(cfg_.fourcc.empty() ? "GREY" : cfg_.fourcc, cfg_.orientation, cfg_.raw_planes));
        std::vector<double> g(n);
        std::vector<uint8_t> has(n);
        for (int i = 0; i < n; i++) { has[i] = gyro[i].has_value(); g[i] = gyro[i].value_or(0.0); }
        std::vector<whacknet::VisionMeasurement> out(n);
        std::vector<int32_t> valid(n);
        check(ck_process_uploaded(h_->get(), n, &pp_, g.data(), has.data(), out.data(), valid.data()), "ck_process_uploaded");
        std::vector<std::pair<whacknet::VisionMeasurement, bool>> r;
        for (int i = 0; i < n; i++) r.emplace_back(out[i], valid[i] != 0);
        return r;
    }
    // a camera that delivers MJPG (Config::fourcc "MJPG" / "JPEG"): one JPEG per frame, decoded and turned by Config::orientation on
    // the device; a frame the decoder refuses (CK_JPEG_* status) is a black frame: no detections, no pose
    std::vector<std::pair<whacknet::VisionMeasurement, bool>> process_jpeg(const std::vector<std::vector<uint8_t>> &jpegs, const std::vector<std::optional<double>> &gyro) {
        const int n = (int)jpegs.size();
        if (!is_jpeg_fourcc(cfg_.fourcc)) throw Panic("process_jpeg: the task's fourcc is not MJPG", CK_EINVAL);
        if (n > cfg_.max_batch || gyro.size() != jpegs.size()) throw Panic("process_jpeg: batch larger than max_batch or gyro size mismatch", CK_EINVAL);
        (void)h_->upload_jpeg(jpegs, orientation_code(cfg_.orientation));
        std::vector<double> g(n);
        std::vector<uint8_t> has(n);
        for (int i = 0; i < n; i++) { has[i] = gyro[i].has_value(); g[i] = gyro[i].value_or(0.0); }
        std::vector<whacknet::VisionMeasurement> out(n);
        std::vector<int32_t> valid(n);
        check(ck_process_uploaded(h_->get(), n, &pp_, g.data(), has.data(), out.data(), valid.data()), "ck_process_uploaded");
        std::vector<std::pair<whacknet::VisionMeasurement, bool>> r;
        for (int i = 0; i < n; i++) r.emplace_back(out[i], valid[i] != 0);
        return r;
    }
    // `ts` of a record is the processing latency in microseconds, clock.now() - tov (lib.rs:351,366): the device leaves it
    // zero, the host stamps it when the batch comes back.  tov_us[i] = time of validity of frame i on the same clock.
    static void stamp(std::vector<std::pair<whacknet::VisionMeasurement, bool>> &recs, const std::vector<uint64_t> &tov_us, uint64_t now_us) {
        for (size_t i = 0; i < recs.size() && i < tov_us.size(); i++) recs[i].first.ts = now_us - tov_us[i];
    }
    std::pair<whacknet::VisionMeasurement, bool> process(const ck_image_u8_t &img, std::optional<double> gyro) {
        return process(std::vector<ck_image_u8_t>{img}, std::vector<std::optional<double>>{gyro})[0];
    }
    const ck_process_params_t &params() const { return pp_; }
    const std::shared_ptr<Handle> &handle() const { return h_; }
    // the same for a batch that was written into an IngestRing slot and submitted
    std::vector<std::pair<whacknet::VisionMeasurement, bool>> process(IngestRing &ring, int slot, const std::vector<std::optional<double>> &gyro) {
        const int n = (int)gyro.size();
        std::vector<double> g(n);
        std::vector<uint8_t> has(n);
        for (int i = 0; i < n; i++) { has[i] = gyro[i].has_value(); g[i] = gyro[i].value_or(0.0); }
        std::vector<whacknet::VisionMeasurement> out(n);
        std::vector<int32_t> valid(n);
        check(ck_process_ingested(ring.get(), slot, n, &pp_, g.data(), has.data(), out.data(), valid.data()), "ck_process_ingested"); // CK_EINVAL unless n frames were submitted
        std::vector<std::pair<whacknet::VisionMeasurement, bool>> r;
        for (int i = 0; i < n; i++) r.emplace_back(out[i], valid[i] != 0);
        return r;
    }

  private:
    Config cfg_;
    std::shared_ptr<Handle> h_;
    std::vector<ck_field_tag_t> field_;
    ck_process_params_t pp_{};
};

// ---- camera rig (chalkydri_hip.h: ck_rig_*) ----------------------------------------------------------------------
// All the cameras of a robot fused into one robot pose.  One camera's view of a step: its known tags, the bearings of their
// corners (four per tag) and its mount.
struct RigView {
    std::vector<sqpnp::Iso3> tags;
    std::vector<sqpnp::Vec3> bearings;
    sqpnp::Iso3 robot_to_cam;
};
class RigSolver {
  public:
    RigSolver() { ck_rig_params_default(&prm_); }                                     // solve_host alone: no device
    explicit RigSolver(std::shared_ptr<Handle> h) : h_(std::move(h)) { ck_rig_params_default(&prm_); }
    RigSolver &max_iter(size_t n) { prm_.sqpnp.max_iter = (int32_t)n; return *this; }
    RigSolver &tolerance(double tol) { prm_.sqpnp.tol_sq = tol * tol; return *this; }
    RigSolver &rig_id(uint8_t id) { prm_.rig_id = id; return *this; }
    const ck_rig_params_t &params() const { return prm_; }
    // steps[s][c] = camera c at step s (every step with the same cameras); gyro[s] = the heading of step s.  On the device ...
    std::vector<ck_rig_result_t> solve_batch(const std::vector<std::vector<RigView>> &steps, const std::vector<double> &gyro) const {
        if (!h_) throw Panic("RigSolver::solve_batch needs a handle", CK_EINVAL);
        return solve(steps, gyro, false);
    }
    // ... and on the host, one thread
    std::vector<ck_rig_result_t> solve_host(const std::vector<std::vector<RigView>> &steps, const std::vector<double> &gyro) const {
        return solve(steps, gyro, true);
    }
    // The solve that drops a wrong tag (chalkydri_hip.h: ck_rig_solve_robust_*): GNC-TLS around the same solver, the
    // pose of the inliers in `fused`.  On the device, or with host = true on the host.  The robust parameters' own `rig` is ignored:
    // this solver's parameters take its place.
    static ck_rig_robust_params_t robust_defaults() { ck_rig_robust_params_t p; ck_rig_robust_params_default(&p); return p; }
    std::vector<ck_rig_robust_result_t> solve_robust(const std::vector<std::vector<RigView>> &steps, const std::vector<double> &gyro,
                                                     ck_rig_robust_params_t robust = robust_defaults(), bool host = false) const {
        if (!host && !h_) throw Panic("RigSolver::solve_robust needs a handle", CK_EINVAL);
        robust.rig = prm_;
        std::vector<ck_sqpnp_problem_t> probs;
        std::vector<ck_iso3_t> tags;
        std::vector<double> b;
        const int n = (int)steps.size(), n_cams = pack(steps, gyro, probs, tags, b);
        std::vector<ck_rig_robust_result_t> out((size_t)n + 1);
        const double g0 = 0.0;
        const int rc = host ? ck_rig_solve_robust_host(&robust, n_cams, probs.data(), n, tags.data(), (int32_t)tags.size(), b.data(),
                                                       (int32_t)(b.size() / 3), n ? gyro.data() : &g0, out.data())
                            : ck_rig_solve_robust_batch(h_->get(), &robust, n_cams, probs.data(), n, tags.data(), (int32_t)tags.size(), b.data(),
                                                        (int32_t)(b.size() / 3), n ? gyro.data() : &g0, out.data());
        check(rc, host ? "ck_rig_solve_robust_host" : "ck_rig_solve_robust_batch");
        out.resize((size_t)n);
        return out;
    }
    // The maximum-likelihood pose of every step and its covariance (chalkydri_hip.h: ck_rig_refine_*) from the fused
    // records `start` of the same steps; `rejected` (optional, [steps][CK_RIG_MAX_CAMS]) are a robust solve's masks.  gyro is read
    // when refine.gyro_sigma_rad > 0 and may be empty otherwise.  On the device, or with host = true on the host: the same bytes.
    // The host call keeps no state between or across calls: it may run on several threads at once.
    static ck_rig_refine_params_t refine_defaults() { ck_rig_refine_params_t p; ck_rig_refine_params_default(&p); return p; }
    std::vector<ck_rig_refined_t> refine(const std::vector<std::vector<RigView>> &steps, const std::vector<double> &gyro,
                                         const std::vector<ck_rig_result_t> &start, ck_rig_refine_params_t refine = refine_defaults(),
                                         bool host = false, const std::vector<uint64_t> *rejected = nullptr) const {
        if (!host && !h_) throw Panic("RigSolver::refine needs a handle", CK_EINVAL);
        std::vector<ck_sqpnp_problem_t> probs;
        std::vector<ck_iso3_t> tags;
        std::vector<double> b;
        const bool no_heading = gyro.empty() && !(refine.gyro_sigma_rad > 0.0);
        const int n = (int)steps.size(), n_cams = pack(steps, no_heading ? std::vector<double>(steps.size(), 0.0) : gyro, probs, tags, b);
        if (start.size() != steps.size() || (rejected && rejected->size() != steps.size() * CK_RIG_MAX_CAMS))
            throw Panic("RigSolver::refine: one start record (and one row of masks) per step", CK_EINVAL);
        std::vector<ck_rig_refined_t> out((size_t)n + 1);
        std::vector<ck_rig_result_t> st(start);
        st.resize((size_t)n + 1);
        const double g0 = 0.0;
        const uint64_t *rej = rejected && n ? rejected->data() : nullptr;
        const int rc = host ? ck_rig_refine_host(&refine, n_cams, probs.data(), n, tags.data(), (int32_t)tags.size(), b.data(), (int32_t)(b.size() / 3),
                                                 no_heading ? nullptr : n ? gyro.data() : &g0, st.data(), rej, out.data())
                            : ck_rig_refine_batch(h_->get(), &refine, n_cams, probs.data(), n, tags.data(), (int32_t)tags.size(), b.data(),
                                                  (int32_t)(b.size() / 3), no_heading ? nullptr : n ? gyro.data() : &g0, st.data(), rej, out.data());
        check(rc, host ? "ck_rig_refine_host" : "ck_rig_refine_batch");
        out.resize((size_t)n);
        return out;
    }

  private:
    // the records, tags and bearings of the steps as the C calls take them; returns the number of cameras
    static int pack(const std::vector<std::vector<RigView>> &steps, const std::vector<double> &gyro, std::vector<ck_sqpnp_problem_t> &probs,
                    std::vector<ck_iso3_t> &tags, std::vector<double> &b) {
        const int n = (int)steps.size(), n_cams = n ? (int)steps[0].size() : 1;
        if (gyro.size() != steps.size()) throw Panic("RigSolver: one gyro heading per step", CK_EINVAL);
        probs.assign((size_t)n_cams * n + 1, ck_sqpnp_problem_t{});
        for (int s = 0; s < n; s++) {
            if ((int)steps[s].size() != n_cams) throw Panic("RigSolver: every step needs the same cameras", CK_EINVAL);
            for (int c = 0; c < n_cams; c++) {
                const RigView &v = steps[s][c];
                ck_sqpnp_problem_t &p = probs[(size_t)c * n + s];
                p = ck_sqpnp_problem_t{};
                p.n_tags = (int32_t)v.tags.size(); p.n_bearings = (int32_t)v.bearings.size();
                p.tag_offset = (int32_t)tags.size(); p.bearing_offset = (int32_t)(b.size() / 3);
                p.robot_to_cam = v.robot_to_cam.raw();
                for (const auto &t : v.tags) tags.push_back(t.raw());
                for (const auto &x : v.bearings) b.insert(b.end(), x.begin(), x.end());
            }
        }
        return n_cams;
    }
    std::vector<ck_rig_result_t> solve(const std::vector<std::vector<RigView>> &steps, const std::vector<double> &gyro, bool host) const {
        std::vector<ck_sqpnp_problem_t> probs;
        std::vector<ck_iso3_t> tags;
        std::vector<double> b;
        const int n = (int)steps.size(), n_cams = pack(steps, gyro, probs, tags, b);
        std::vector<ck_rig_result_t> out((size_t)n + 1);
        const double g0 = 0.0;
        const int rc = host ? ck_rig_solve_host(&prm_, n_cams, probs.data(), n, tags.data(), (int32_t)tags.size(), b.data(), (int32_t)(b.size() / 3),
                                                n ? gyro.data() : &g0, out.data())
                            : ck_rig_solve_batch(h_->get(), &prm_, n_cams, probs.data(), n, tags.data(), (int32_t)tags.size(), b.data(),
                                                 (int32_t)(b.size() / 3), n ? gyro.data() : &g0, out.data());
        check(rc, host ? "ck_rig_solve_host" : "ck_rig_solve_batch");
        out.resize((size_t)n);
        return out;
    }
    std::shared_ptr<Handle> h_;
    ck_rig_params_t prm_{};
};
// After every task of `tasks` has processed the n frames of one instant each (AprilTags::process): the fused measurement of every
// step, read from what the tasks left on the device.  results (optional): the full records.
inline std::vector<std::pair<whacknet::VisionMeasurement, bool>> rig_process_last(const std::vector<AprilTags *> &tasks, const ck_rig_params_t &params,
                                                                                  const std::vector<std::optional<double>> &gyro,
                                                                                  std::vector<ck_rig_result_t> *results = nullptr) {
    const int n = (int)gyro.size();
    std::vector<ck_handle_t *> hs;
    for (const AprilTags *t : tasks) hs.push_back(t ? t->handle()->get() : nullptr);
    std::vector<double> g((size_t)n + 1);
    std::vector<uint8_t> has((size_t)n + 1);
    for (int i = 0; i < n; i++) { has[i] = gyro[i].has_value(); g[i] = gyro[i].value_or(0.0); }
    std::vector<ck_rig_result_t> res((size_t)n + 1);
    std::vector<whacknet::VisionMeasurement> out((size_t)n + 1);
    std::vector<int32_t> valid((size_t)n + 1);
    check(ck_rig_process_last(hs.data(), (int32_t)hs.size(), n, &params, g.data(), has.data(), res.data(), out.data(), valid.data()), "ck_rig_process_last");
    std::vector<std::pair<whacknet::VisionMeasurement, bool>> r;
    for (int i = 0; i < n; i++) r.emplace_back(out[i], valid[i] != 0);
    if (results) results->assign(res.begin(), res.begin() + n);
    return r;
}
// ... and with the solve that drops a wrong tag (ck_rig_process_last_robust): `robust.rig` is the rig's parameters
inline std::vector<std::pair<whacknet::VisionMeasurement, bool>> rig_process_last_robust(const std::vector<AprilTags *> &tasks,
                                                                                         const ck_rig_robust_params_t &robust,
                                                                                         const std::vector<std::optional<double>> &gyro,
                                                                                         std::vector<ck_rig_robust_result_t> *results = nullptr) {
    const int n = (int)gyro.size();
    std::vector<ck_handle_t *> hs;
    for (const AprilTags *t : tasks) hs.push_back(t ? t->handle()->get() : nullptr);
    std::vector<double> g((size_t)n + 1);
    std::vector<uint8_t> has((size_t)n + 1);
    for (int i = 0; i < n; i++) { has[i] = gyro[i].has_value(); g[i] = gyro[i].value_or(0.0); }
    std::vector<ck_rig_robust_result_t> res((size_t)n + 1);
    std::vector<whacknet::VisionMeasurement> out((size_t)n + 1);
    std::vector<int32_t> valid((size_t)n + 1);
    check(ck_rig_process_last_robust(hs.data(), (int32_t)hs.size(), n, &robust, g.data(), has.data(), res.data(), out.data(), valid.data()),
          "ck_rig_process_last_robust");
    std::vector<std::pair<whacknet::VisionMeasurement, bool>> r;
    for (int i = 0; i < n; i++) r.emplace_back(out[i], valid[i] != 0);
    if (results) results->assign(res.begin(), res.begin() + n);
    return r;
}
// ... and with the refinement behind either solve (ck_rig_process_last_refined): the measurements carry the refined x, y,
// yaw and the standard deviations of its covariance where the refinement has a pose.  use_robust false: `robust.rig` alone is read.
// refined (optional): the refinement's records; fused (optional): the robust solve's records (use_robust true only).
inline std::vector<std::pair<whacknet::VisionMeasurement, bool>> rig_process_last_refined(const std::vector<AprilTags *> &tasks,
                                                                                          const ck_rig_robust_params_t &robust, bool use_robust,
                                                                                          const ck_rig_refine_params_t &refine,
                                                                                          const std::vector<std::optional<double>> &gyro,
                                                                                          std::vector<ck_rig_refined_t> *refined = nullptr,
                                                                                          std::vector<ck_rig_robust_result_t> *fused = nullptr) {
    const int n = (int)gyro.size();
    std::vector<ck_handle_t *> hs;
    for (const AprilTags *t : tasks) hs.push_back(t ? t->handle()->get() : nullptr);
    std::vector<double> g((size_t)n + 1);
    std::vector<uint8_t> has((size_t)n + 1);
    for (int i = 0; i < n; i++) { has[i] = gyro[i].has_value(); g[i] = gyro[i].value_or(0.0); }
    std::vector<ck_rig_robust_result_t> res((size_t)n + 1);
    std::vector<ck_rig_refined_t> ref((size_t)n + 1);
    std::vector<whacknet::VisionMeasurement> out((size_t)n + 1);
    std::vector<int32_t> valid((size_t)n + 1);
    check(ck_rig_process_last_refined(hs.data(), (int32_t)hs.size(), n, &robust, use_robust ? 1 : 0, &refine, g.data(), has.data(),
                                      use_robust ? res.data() : nullptr, ref.data(), out.data(), valid.data()),
          "ck_rig_process_last_refined");
    std::vector<std::pair<whacknet::VisionMeasurement, bool>> r;
    for (int i = 0; i < n; i++) r.emplace_back(out[i], valid[i] != 0);
    if (refined) refined->assign(ref.begin(), ref.begin() + n);
    if (fused && use_robust) fused->assign(res.begin(), res.begin() + n);
    return r;
}

// ---- camera calibration (chalkydri_hip.h: ck_calib_*) ---------------------------------------------------------
// The reference configurator's `Calibrator` (crates/configurator/src/calibration.rs:30-143): process() collects frames of a tag
// board, calibrate() solves for the OpenCVModel5 of the camera.  Here the frames become point correspondences on the host and the
// solve runs on the device.
using OpenCv5 = ck_opencv5_t;

// A grid of tags on a plane, ids row-major from the board's origin (the aprilgrid convention); x along a row, y along a column
struct Board {
    int rows = 6, cols = 6;
    double tag_size = 0.088, tag_spacing = 0.3; // the defaults of the external crate's create_default_6x6_board(): measure the printed board
    int first_id = 0;
    double pitch() const { return tag_size * (1.0 + tag_spacing); }
    bool has(int id) const { return id >= first_id && id < first_id + rows * cols; }
    // board-plane coordinates of the tag's corners in ck_detection_t's corner order
    std::array<std::array<double, 2>, 4> tag_corners(int id) const {
        if (!has(id)) throw Panic("Board::tag_corners: no such tag", CK_EINVAL);
        const int k = id - first_id;
        const double s = tag_size / 2, cx = (k % cols) * pitch() + s, cy = (k / cols) * pitch() + s;
        return {{{cx - s, cy + s}, {cx + s, cy + s}, {cx + s, cy - s}, {cx - s, cy - s}}};
    }
};

// ---- sub-pixel corners (chalkydri_hip.h: ck_corner_subpix, ck_board_corners_last) -----------------------------
inline ck_subpix_params_t subpix_params(int half_win = 5) {
    ck_subpix_params_t pp;
    ck_subpix_params_default(&pp);
    pp.half_win = half_win;
    return pp;
}
// points xy (x0 y0 x1 y1 ...) of the staged frames, point i in frame frames[i] (empty: all in frame 0), refined on the device
inline std::vector<double> corner_subpix(Handle &h, const ck_subpix_params_t &pp, const std::vector<int32_t> &frames, const std::vector<double> &xy,
                                         std::vector<ck_subpix_info_t> *info = nullptr) {
    if (xy.size() % 2 || (!frames.empty() && frames.size() != xy.size() / 2)) throw Panic("corner_subpix: size mismatch", CK_EINVAL);
    const int32_t n = (int32_t)(xy.size() / 2);
    std::vector<double> out(xy.size());
    if (info) info->assign((size_t)n, ck_subpix_info_t{});
    check(ck_corner_subpix(h.get(), &pp, frames.empty() ? nullptr : frames.data(), xy.data(), n, out.data(), info ? info->data() : nullptr), "ck_corner_subpix");
    return out;
}
// the same on host images, one thread: the bytes of corner_subpix
inline std::vector<double> corner_subpix_host(const ck_subpix_params_t &pp, const std::vector<ck_image_u8_t> &imgs, const std::vector<int32_t> &frames,
                                              const std::vector<double> &xy, std::vector<ck_subpix_info_t> *info = nullptr) {
    if (xy.size() % 2 || (!frames.empty() && frames.size() != xy.size() / 2)) throw Panic("corner_subpix_host: size mismatch", CK_EINVAL);
    const int32_t n = (int32_t)(xy.size() / 2);
    std::vector<double> out(xy.size());
    if (info) info->assign((size_t)n, ck_subpix_info_t{});
    check(ck_corner_subpix_host(&pp, imgs.data(), (int32_t)imgs.size(), frames.empty() ? nullptr : frames.data(), xy.data(), n, out.data(),
                                info ? info->data() : nullptr), "ck_corner_subpix_host");
    return out;
}
// A board recovered from the tags that decoded, in the n_frames frames of the handle's last detect / process call
struct BoardCorners {
    int n_frames = 0, n_tags_per_frame = 0;
    std::vector<double> uv;       // [n_frames][rows * cols][4][2]
    std::vector<uint8_t> state;   // [n_frames][rows * cols]: 0 absent, 1 seed, 2 recovered
    std::vector<int32_t> n_tags;  // [n_frames]
};
inline ck_board_t board_desc(const Board &b, int family = 0) { return ck_board_t{b.rows, b.cols, b.first_id, family, b.tag_size, b.tag_spacing}; }
inline BoardCorners board_corners(Handle &h, const Board &board, const ck_subpix_params_t *pp = nullptr, const ck_board_params_t *bp = nullptr) {
    ck_subpix_params_t p = pp ? *pp : subpix_params();
    ck_board_params_t q;
    ck_board_params_default(&q);
    if (bp) q = *bp;
    const ck_board_t bd = board_desc(board);
    BoardCorners r;
    const int nb = h.config().max_batch;
    r.n_tags_per_frame = board.rows * board.cols;
    r.uv.assign((size_t)nb * r.n_tags_per_frame * 8, 0.0);
    r.state.assign((size_t)nb * r.n_tags_per_frame, 0);
    r.n_tags.assign((size_t)nb, -1); // the call writes one count per frame of the last call: the rest stay -1
    check(ck_board_corners_last(h.get(), &bd, &p, &q, r.uv.data(), r.state.data(), r.n_tags.data()), "ck_board_corners_last");
    while (r.n_frames < nb && r.n_tags[(size_t)r.n_frames] >= 0) r.n_frames++;
    r.uv.resize((size_t)r.n_frames * r.n_tags_per_frame * 8);
    r.state.resize((size_t)r.n_frames * r.n_tags_per_frame);
    r.n_tags.resize((size_t)r.n_frames);
    return r;
}

class Calibrator {
  public:
    static constexpr int MIN_CORNERS = 24; // calibration.rs:30
    struct Report {
        ck_calib_result_t result{};
        std::vector<std::array<double, 12>> poses; // board -> camera per kept frame: R row-major, t
    };
    // recover: process() recovers the whole board from the tags that decoded (board_corners), every seed and recovered tag's four
    // refined corners kept; false (the default) is the reference's path
    explicit Calibrator(std::shared_ptr<Handle> h, const Board &board = Board(), int min_corners = MIN_CORNERS, bool recover = false)
        : h_(std::move(h)), board_(board), min_corners_(min_corners), recover_(recover) {}

    // Detects the board in the frames and keeps each one with at least min_corners corners of the board's ids decoded without a
    // corrected bit; returns the number of frames kept so far, like the reference
    size_t process(const std::vector<ck_image_u8_t> &imgs) {
        const int n = (int)imgs.size(), cap = std::max(64, board_.rows * board_.cols);
        std::vector<ck_detection_t> dets((size_t)n * cap);
        std::vector<int32_t> counts(n);
        check(ck_detect_batch(h_->get(), imgs.data(), n, dets.data(), cap, counts.data(), nullptr), "ck_detect_batch");
        if (recover_) {
            const BoardCorners r = board_corners(*h_, board_);
            for (int i = 0; i < r.n_frames; i++) {
                std::vector<double> b, u;
                for (int t = 0; t < r.n_tags_per_frame; t++) {
                    if (!r.state[(size_t)i * r.n_tags_per_frame + t]) continue;
                    const auto c = board_.tag_corners(board_.first_id + t);
                    const double *q = &r.uv[((size_t)i * r.n_tags_per_frame + t) * 8];
                    for (int j = 0; j < 4; j++) { b.push_back(c[j][0]); b.push_back(c[j][1]); u.push_back(q[2 * j]); u.push_back(q[2 * j + 1]); }
                }
                if ((int)b.size() / 2 >= min_corners_) add_observations(b, u);
            }
            return starts_.size() - 1;
        }
        for (int i = 0; i < n; i++) {
            std::vector<double> b, u;
            std::vector<int> seen;
            for (int k = 0; k < counts[i]; k++) {
                const ck_detection_t &d = dets[(size_t)i * cap + k];
                if (!board_.has(d.id) || d.hamming != 0 || d.family != 0 || std::find(seen.begin(), seen.end(), d.id) != seen.end()) continue;
                seen.push_back(d.id);
                const auto c = board_.tag_corners(d.id);
                for (int j = 0; j < 4; j++) { b.push_back(c[j][0]); b.push_back(c[j][1]); u.push_back(d.p[j][0]); u.push_back(d.p[j][1]); }
            }
            if ((int)b.size() / 2 >= min_corners_) add_observations(b, u);
        }
        return starts_.size() - 1;
    }
    // one frame's correspondences from elsewhere: board_xy and image_uv as x0 y0 x1 y1 ...
    void add_observations(const std::vector<double> &board_xy, const std::vector<double> &image_uv) {
        if (board_xy.size() != image_uv.size() || board_xy.size() % 2) throw Panic("add_observations: size mismatch", CK_EINVAL);
        bxy_.insert(bxy_.end(), board_xy.begin(), board_xy.end());
        uv_.insert(uv_.end(), image_uv.begin(), image_uv.end());
        starts_.push_back((int32_t)(bxy_.size() / 2));
    }
    size_t frames() const { return starts_.size() - 1; }
    void clear() { bxy_.clear(); uv_.clear(); starts_.assign(1, 0); }

    // calibration.rs:110-143: the model, or nullopt when the solve neither converged nor stalled at a finite rms; the frames are
    // cleared either way, as the reference does.  fixed_mask: bits of ck_calib_params_t.fixed_mask.
    std::optional<OpenCv5> calibrate(uint32_t fixed_mask = 0, Report *report = nullptr) {
        ck_calib_params_t p;
        ck_calib_params_default(&p, h_->config().width, h_->config().height);
        p.fixed_mask = fixed_mask;
        p.min_points_per_frame = std::max(4, min_corners_);
        const int F = (int)frames();
        Report r;
        r.poses.resize(F);
        std::optional<OpenCv5> out;
        if (F >= p.min_frames) {
            const ck_calib_problem_t q{F, 0, 0, 0};
            check(ck_calibrate_batch(h_->get(), &p, &q, 1, bxy_.data(), uv_.data(), starts_.data(), starts_.back(), F + 1, F, &r.result,
                                     F ? r.poses[0].data() : nullptr), "ck_calibrate_batch");
            if ((r.result.status == CK_CALIB_CONVERGED || r.result.status == CK_CALIB_STALLED) && std::isfinite(r.result.rms)) out = r.result.cam;
        } else {
            r.result.status = CK_CALIB_DEGENERATE;
        }
        if (report) *report = r;
        clear();
        return out;
    }

    // The same for any camera model (ck_camera_calibrate_batch): an EUCM / UCM problem is solved from CK_CAMCAL_STARTS starts in one
    // launch and the lowest final cost kept (report->result.start).  fixed_mask bits 0..5: fx fy cx cy alpha beta.
    struct CameraReport {
        ck_camera_calib_result_t result{};
        std::vector<std::array<double, 12>> poses;
    };
    std::optional<Camera> calibrate(CameraModel model, uint32_t fixed_mask = 0, CameraReport *report = nullptr) {
        ck_calib_params_t p;
        ck_calib_params_default(&p, h_->config().width, h_->config().height);
        p.fixed_mask = fixed_mask;
        p.min_points_per_frame = std::max(4, min_corners_);
        const int F = (int)frames();
        CameraReport r;
        r.poses.resize(F);
        std::optional<Camera> out;
        if (F >= p.min_frames) {
            const ck_calib_problem_t q{F, 0, 0, 0};
            check(ck_camera_calibrate_batch(h_->get(), (int32_t)model, &p, &q, 1, bxy_.data(), uv_.data(), starts_.data(), starts_.back(), F + 1, F,
                                            &r.result, r.poses[0].data()), "ck_camera_calibrate_batch");
            if ((r.result.status == CK_CALIB_CONVERGED || r.result.status == CK_CALIB_STALLED) && std::isfinite(r.result.rms)) {
                out.emplace();
                out->raw = r.result.cam;
            }
        } else {
            r.result.status = CK_CALIB_DEGENERATE;
        }
        if (report) *report = r;
        clear();
        return out;
    }

  private:
    std::shared_ptr<Handle> h_;
    Board board_;
    int min_corners_;
    bool recover_ = false;
    std::vector<double> bxy_, uv_;
    std::vector<int32_t> starts_{0};
};

// Calibration of the camera mounts of a rig (chalkydri_hip.h: ck_rigcal_*): collects steps (instants in which the
// cameras saw field tags) and solves for the robot_to_cam of every camera that is not frozen and one robot pose per step.
class MountCalibrator {
  public:
    struct Report {
        ck_rigcal_result_t result{};
        std::vector<std::array<double, 12>> poses; // world -> robot per step: R row-major, t
    };
    // mounts0: the start robot_to_cam of every camera; fixed_mask: ck_rigcal_params_t.fixed_mask (camera 0 wholly: the gauge)
    MountCalibrator(std::shared_ptr<Handle> h, std::vector<ck_iso3_t> mounts0, uint64_t fixed_mask = CK_RIGCAL_FIX_CAMERA(0))
        : h_(std::move(h)), mounts0_(std::move(mounts0)), fixed_(fixed_mask) {
        if (mounts0_.empty() || mounts0_.size() > CK_RIG_MAX_CAMS) throw Panic("a rig has 1..8 cameras", CK_EINVAL);
    }
    // one step: per camera its known tags and the four corner bearings of each (x y z per corner); gyro = the heading of the step
    void add_step(const std::vector<std::vector<ck_iso3_t>> &tags, const std::vector<std::vector<double>> &bearings, double gyro) {
        if (tags.size() != mounts0_.size() || bearings.size() != mounts0_.size()) throw Panic("add_step: one entry per camera", CK_EINVAL);
        for (size_t c = 0; c < tags.size(); c++) {
            if (bearings[c].size() != 12 * tags[c].size()) throw Panic("add_step: four bearings per tag", CK_EINVAL);
            ck_sqpnp_problem_t r{};
            r.n_tags = (int32_t)tags[c].size(); r.n_bearings = 4 * r.n_tags;
            r.tag_offset = (int32_t)tags_.size(); r.bearing_offset = (int32_t)(bear_.size() / 3);
            r.robot_to_cam = mounts0_[c];
            tags_.insert(tags_.end(), tags[c].begin(), tags[c].end());
            bear_.insert(bear_.end(), bearings[c].begin(), bearings[c].end());
            steps_.push_back(r); // step-major here, camera-major in a call (records())
        }
        gyro_.push_back(gyro);
    }
    // the steps of the last ck_process_* call of n frames of every camera's handle (ck_last_pose_inputs), gyro[n] their headings
    void add_last(const std::vector<std::shared_ptr<Handle>> &cams, int n, const std::vector<double> &gyro) {
        if (cams.size() != mounts0_.size() || (int)gyro.size() != n) throw Panic("add_last: one handle per camera, one heading per frame", CK_EINVAL);
        std::vector<std::vector<ck_sqpnp_problem_t>> rec(cams.size(), std::vector<ck_sqpnp_problem_t>((size_t)n));
        std::vector<std::vector<ck_iso3_t>> tg(cams.size());
        std::vector<std::vector<double>> br(cams.size());
        for (size_t c = 0; c < cams.size(); c++) {
            int32_t nt = 0, nb = 0;
            ck_iso3_t none{};
            double nob = 0;
            int rc = ck_last_pose_inputs(cams[c]->get(), n, rec[c].data(), &none, 0, &nob, 0, &nt, &nb);
            if (rc != CK_OK && rc != CK_ECAPACITY) check(rc, "ck_last_pose_inputs");
            tg[c].resize((size_t)nt + 1); br[c].resize(3 * (size_t)nb + 3);
            check(ck_last_pose_inputs(cams[c]->get(), n, rec[c].data(), tg[c].data(), nt, br[c].data(), nb, &nt, &nb), "ck_last_pose_inputs");
        }
        for (int s = 0; s < n; s++) {
            std::vector<std::vector<ck_iso3_t>> t(cams.size());
            std::vector<std::vector<double>> b(cams.size());
            for (size_t c = 0; c < cams.size(); c++) {
                const ck_sqpnp_problem_t &r = rec[c][(size_t)s];
                t[c].assign(tg[c].begin() + r.tag_offset, tg[c].begin() + r.tag_offset + r.n_tags);
                b[c].assign(br[c].begin() + 3 * (size_t)r.bearing_offset, br[c].begin() + 3 * ((size_t)r.bearing_offset + r.n_bearings));
            }
            add_step(t, b, gyro[(size_t)s]);
        }
    }
    size_t steps() const { return gyro_.size(); }
    void clear() { steps_.clear(); tags_.clear(); bear_.clear(); gyro_.clear(); }

    // The mounts, or nullopt when the solve neither converged nor stalled at a finite rms.  Start poses from the rig solver on the
    // device (ck_rig_calibrate_batch).  The steps stay until clear().
    std::optional<std::vector<ck_iso3_t>> calibrate(Report *report = nullptr, int max_iters = 0) {
        return solve(nullptr, false, report, max_iters);
    }
    // the refinement alone from given start poses [steps][12]: on the device (ck_rigcal_refine_batch) or on the host, one thread,
    // no device (ck_rigcal_refine_host); the two return the same bytes
    std::optional<std::vector<ck_iso3_t>> refine(const std::vector<std::array<double, 12>> &poses0, bool host, Report *report = nullptr,
                                                  int max_iters = 0) {
        if (poses0.size() != steps()) throw Panic("refine: one start pose per step", CK_EINVAL);
        return solve(&poses0, host, report, max_iters);
    }

  private:
    std::optional<std::vector<ck_iso3_t>> solve(const std::vector<std::array<double, 12>> *poses0, bool host, Report *report, int max_iters) {
        const int n = (int)steps(), C = (int)mounts0_.size();
        ck_rigcal_params_t p;
        ck_rigcal_params_default(&p);
        p.fixed_mask = fixed_;
        if (max_iters > 0) p.max_iters = max_iters;
        Report r;
        r.poses.resize((size_t)n);
        std::optional<std::vector<ck_iso3_t>> out;
        if (n >= p.min_steps) {
            std::vector<ck_sqpnp_problem_t> rec((size_t)C * n);
            for (int s = 0; s < n; s++)
                for (int c = 0; c < C; c++) rec[(size_t)c * n + s] = steps_[(size_t)s * C + c];
            std::vector<int32_t> index((size_t)n);
            for (int s = 0; s < n; s++) index[(size_t)s] = s;
            const ck_rigcal_problem_t q{n, 0};
            const int32_t nt = (int32_t)tags_.size(), nb = (int32_t)(bear_.size() / 3);
            if (!poses0)
                check(ck_rig_calibrate_batch(h_->get(), &p, C, rec.data(), n, tags_.data(), nt, bear_.data(), nb, gyro_.data(), &q, 1, index.data(), n,
                                             mounts0_.data(), &r.result, r.poses[0].data()), "ck_rig_calibrate_batch");
            else if (host)
                check(ck_rigcal_refine_host(&p, C, rec.data(), n, tags_.data(), nt, bear_.data(), nb, &q, index.data(), n, mounts0_.data(),
                                            (*poses0)[0].data(), &r.result, r.poses[0].data()), "ck_rigcal_refine_host");
            else
                check(ck_rigcal_refine_batch(h_->get(), &p, C, rec.data(), n, tags_.data(), nt, bear_.data(), nb, &q, 1, index.data(), n, mounts0_.data(),
                                             (*poses0)[0].data(), &r.result, r.poses[0].data()), "ck_rigcal_refine_batch");
            if ((r.result.status == CK_CALIB_CONVERGED || r.result.status == CK_CALIB_STALLED) && std::isfinite(r.result.rms))
                out = std::vector<ck_iso3_t>(r.result.robot_to_cam, r.result.robot_to_cam + C);
        } else {
            r.result.status = CK_CALIB_DEGENERATE;
        }
        if (report) *report = r;
        return out;
    }
    std::shared_ptr<Handle> h_; // may be null for refine(..., host = true)
    std::vector<ck_iso3_t> mounts0_;
    uint64_t fixed_;
    std::vector<ck_sqpnp_problem_t> steps_;
    std::vector<ck_iso3_t> tags_;
    std::vector<double> bear_, gyro_;
};

// Calibration of the field's tag layout (chalkydri_hip.h: ck_fieldcal_*): collects steps (instants in which the cameras
// saw two or more field tags) and solves for the pose of every tag that is not frozen and one robot pose per step.  The mounts stay.
class FieldCalibrator {
  public:
    struct Report {
        ck_fieldcal_result_t result{};
        std::vector<ck_iso3_t> layout;             // per entry of the layout
        std::vector<int32_t> sightings;
        std::vector<double> tag_rms;
        std::vector<std::array<double, 12>> poses; // world -> robot per step: R row-major, t
    };
    // mounts: the robot_to_cam of every camera; layout: the nominal tag poses; fixed6: one mask per entry (one tag with sightings
    // must be CK_FIELDCAL_FIX_ALL: the gauge)
    FieldCalibrator(std::shared_ptr<Handle> h, std::vector<ck_iso3_t> mounts, std::vector<ck_iso3_t> layout, std::vector<uint8_t> fixed6)
        : h_(std::move(h)), mounts_(std::move(mounts)), layout_(std::move(layout)), fixed_(std::move(fixed6)) {
        if (mounts_.empty() || mounts_.size() > CK_RIG_MAX_CAMS) throw Panic("a rig has 1..8 cameras", CK_EINVAL);
        if (layout_.empty() || fixed_.size() != layout_.size()) throw Panic("one mask per entry of the layout", CK_EINVAL);
        for (size_t a = 0; a < layout_.size(); a++)
            for (size_t b = 0; b < a; b++)
                if (std::memcmp(&layout_[a], &layout_[b], sizeof(ck_iso3_t)) == 0) throw Panic("two entries of the layout have the same pose", CK_EINVAL);
    }
    // one step: per camera the entries of the layout it saw and the four corner bearings of each (x y z per corner); gyro = the heading
    void add_step(const std::vector<std::vector<int32_t>> &tags, const std::vector<std::vector<double>> &bearings, double gyro) {
        if (tags.size() != mounts_.size() || bearings.size() != mounts_.size()) throw Panic("add_step: one entry per camera", CK_EINVAL);
        for (size_t c = 0; c < tags.size(); c++) {
            if (bearings[c].size() != 12 * tags[c].size()) throw Panic("add_step: four bearings per tag", CK_EINVAL);
            ck_sqpnp_problem_t r{};
            r.n_tags = (int32_t)tags[c].size(); r.n_bearings = 4 * r.n_tags;
            r.tag_offset = (int32_t)index_.size(); r.bearing_offset = (int32_t)(bear_.size() / 3);
            r.robot_to_cam = mounts_[c];
            index_.insert(index_.end(), tags[c].begin(), tags[c].end());
            bear_.insert(bear_.end(), bearings[c].begin(), bearings[c].end());
            steps_.push_back(r); // step-major here, camera-major in a call
        }
        gyro_.push_back(gyro);
    }
    // the steps of the last ck_process_* call of n frames of every camera's handle (ck_last_pose_inputs), gyro[n] their headings.  That
    // call returns the tags' poses, not their ids: each is matched byte for byte against the layout, which must be the one the
    // handles solved with
    void add_last(const std::vector<std::shared_ptr<Handle>> &cams, int n, const std::vector<double> &gyro) {
        if (cams.size() != mounts_.size() || (int)gyro.size() != n) throw Panic("add_last: one handle per camera, one heading per frame", CK_EINVAL);
        std::vector<std::vector<ck_sqpnp_problem_t>> rec(cams.size(), std::vector<ck_sqpnp_problem_t>((size_t)n));
        std::vector<std::vector<ck_iso3_t>> tg(cams.size());
        std::vector<std::vector<double>> br(cams.size());
        for (size_t c = 0; c < cams.size(); c++) {
            int32_t nt = 0, nb = 0;
            ck_iso3_t none{};
            double nob = 0;
            int rc = ck_last_pose_inputs(cams[c]->get(), n, rec[c].data(), &none, 0, &nob, 0, &nt, &nb);
            if (rc != CK_OK && rc != CK_ECAPACITY) check(rc, "ck_last_pose_inputs");
            tg[c].resize((size_t)nt + 1); br[c].resize(3 * (size_t)nb + 3);
            check(ck_last_pose_inputs(cams[c]->get(), n, rec[c].data(), tg[c].data(), nt, br[c].data(), nb, &nt, &nb), "ck_last_pose_inputs");
        }
        for (int s = 0; s < n; s++) {
            std::vector<std::vector<int32_t>> t(cams.size());
            std::vector<std::vector<double>> b(cams.size());
            for (size_t c = 0; c < cams.size(); c++) {
                const ck_sqpnp_problem_t &r = rec[c][(size_t)s];
                for (int32_t k = 0; k < r.n_tags; k++) {
                    size_t at = 0;
                    while (at < layout_.size() && std::memcmp(&layout_[at], &tg[c][(size_t)r.tag_offset + k], sizeof(ck_iso3_t)) != 0) at++;
                    if (at == layout_.size()) throw Panic("add_last: a tag the handle solved with is not in the layout", CK_EINVAL);
                    t[c].push_back((int32_t)at);
                }
                b[c].assign(br[c].begin() + 3 * (size_t)r.bearing_offset, br[c].begin() + 3 * ((size_t)r.bearing_offset + r.n_bearings));
            }
            add_step(t, b, gyro[(size_t)s]);
        }
    }
    size_t steps() const { return gyro_.size(); }
    void clear() { steps_.clear(); index_.clear(); bear_.clear(); gyro_.clear(); }

    // The layout, or nullopt when the solve neither converged nor stalled at a finite rms.  Start poses from the rig solver on the
    // device with the nominal layout (ck_field_calibrate_batch).  The steps stay until clear().
    std::optional<std::vector<ck_iso3_t>> calibrate(Report *report = nullptr, int max_iters = 0) {
        return solve(nullptr, false, report, max_iters);
    }
    // the refinement alone from given start poses [steps][12]: on the device (ck_fieldcal_refine_batch) or on the host, one thread,
    // no device (ck_fieldcal_refine_host); the two return the same bytes
    std::optional<std::vector<ck_iso3_t>> refine(const std::vector<std::array<double, 12>> &poses0, bool host, Report *report = nullptr,
                                                  int max_iters = 0) {
        if (poses0.size() != steps()) throw Panic("refine: one start pose per step", CK_EINVAL);
        return solve(&poses0, host, report, max_iters);
    }

  private:
    std::optional<std::vector<ck_iso3_t>> solve(const std::vector<std::array<double, 12>> *poses0, bool host, Report *report, int max_iters) {
        const int n = (int)steps(), C = (int)mounts_.size(), L = (int)layout_.size();
        ck_fieldcal_params_t p;
        ck_fieldcal_params_default(&p);
        if (max_iters > 0) p.max_iters = max_iters;
        Report r;
        r.poses.resize((size_t)n);
        r.layout = layout_;
        r.sightings.assign((size_t)L, 0);
        r.tag_rms.assign((size_t)L, 0.0);
        std::optional<std::vector<ck_iso3_t>> out;
        if (n >= p.min_steps) {
            std::vector<ck_sqpnp_problem_t> rec((size_t)C * n);
            for (int s = 0; s < n; s++)
                for (int c = 0; c < C; c++) rec[(size_t)c * n + s] = steps_[(size_t)s * C + c];
            std::vector<int32_t> index((size_t)n);
            for (int s = 0; s < n; s++) index[(size_t)s] = s;
            const ck_rigcal_problem_t q{n, 0};
            const int32_t nt = (int32_t)index_.size(), nb = (int32_t)(bear_.size() / 3);
            if (!poses0)
                check(ck_field_calibrate_batch(h_->get(), &p, C, rec.data(), n, index_.data(), nt, bear_.data(), nb, gyro_.data(), &q, 1, index.data(),
                                               n, mounts_.data(), layout_.data(), L, fixed_.data(), &r.result, r.layout.data(), r.sightings.data(),
                                               r.tag_rms.data(), r.poses[0].data()), "ck_field_calibrate_batch");
            else if (host)
                check(ck_fieldcal_refine_host(&p, C, rec.data(), n, index_.data(), nt, bear_.data(), nb, &q, index.data(), n, mounts_.data(),
                                              layout_.data(), L, fixed_.data(), (*poses0)[0].data(), &r.result, r.layout.data(), r.sightings.data(),
                                              r.tag_rms.data(), r.poses[0].data()), "ck_fieldcal_refine_host");
            else
                check(ck_fieldcal_refine_batch(h_->get(), &p, C, rec.data(), n, index_.data(), nt, bear_.data(), nb, &q, 1, index.data(), n,
                                               mounts_.data(), layout_.data(), L, fixed_.data(), (*poses0)[0].data(), &r.result, r.layout.data(),
                                               r.sightings.data(), r.tag_rms.data(), r.poses[0].data()), "ck_fieldcal_refine_batch");
            if ((r.result.status == CK_CALIB_CONVERGED || r.result.status == CK_CALIB_STALLED) && std::isfinite(r.result.rms)) out = r.layout;
        } else {
            r.result.status = CK_CALIB_DEGENERATE;
        }
        if (report) *report = r;
        return out;
    }
    std::shared_ptr<Handle> h_; // may be null for refine(..., host = true)
    std::vector<ck_iso3_t> mounts_, layout_;
    std::vector<uint8_t> fixed_;
    std::vector<ck_sqpnp_problem_t> steps_;
    std::vector<int32_t> index_;
    std::vector<double> bear_, gyro_;
};

} // namespace chalkydri
#endif // CHALKYDRI_HPP
