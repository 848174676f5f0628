// Sub-pixel corners on the device: k_subpix refines caller points, k_subpix_dets the corners of a call's final
// detections (the detector setting), k_board recovers a tag board from its decoded tags.  One 64-lane wave per point in all three:
// lane t sums the window's taps t, t + 64, ... in increasing order, a butterfly over the lanes adds the 64 partial sums up in the tree
// of cks_tree_sum, and every lane then takes the same step.  Pixels are read straight from the frame (L1 / L2 hits after the first
// iteration: a window is at most 18 x 18 bytes); no LDS for the arithmetic, no scratch.  The arithmetic is ck_subpix_math.h's.
#include <vector>

#include "ck_internal.h"
#include "ck_subpix.h"
#include "ck_subpix_math.h"

static_assert(sizeof(ck_subpix_params_t) == 24, "ck_subpix_params_t layout");
static_assert(sizeof(ck_subpix_info_t) == 16, "ck_subpix_info_t layout");
static_assert(sizeof(ck_board_t) == 32, "ck_board_t layout");
static_assert(sizeof(ck_board_params_t) == 40, "ck_board_params_t layout");

// one partial sum per lane, then v += v[lane ^ s] for s = 32 .. 1: cks_tree_sum's sums, the same bits in every lane
CKS_FN void cks_window_sums(const cks_image *im, double x, double y, int w, const double *wts, double S[5]) {
    double s[5];
    cks_lane_sums(im, x, y, w, wts, (int)(threadIdx.x & (CKS_LANES - 1)), s);
#pragma unroll
    for (int q = 0; q < 5; q++) {
        double v = s[q];
#pragma unroll
        for (int m = CKS_LANES / 2; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, CKS_LANES);
        S[q] = v;
    }
}

namespace {

constexpr int SP_NT = 64;   // k_subpix: one wave, one point
constexpr int SPD_NT = 256; // k_subpix_dets, k_board: four waves, the four corners of a tag

struct SubpixArgs {
    ck_subpix_params_t pp;
    const uint8_t *frames; // frame f at frames + f * pitch
    int stride, w, h;
    size_t pitch;
    const double *wts;
};

__device__ inline cks_image frame_of(const SubpixArgs &a, int f) {
    cks_image im;
    im.p = a.frames + (size_t)f * a.pitch; im.stride = a.stride; im.w = a.w; im.h = a.h;
    return im;
}

__global__ __launch_bounds__(SP_NT) void k_subpix(SubpixArgs a, const int32_t *frame, const double *xy_in, int n, double *xy_out,
                                                  ck_subpix_info_t *info) {
    const int i = blockIdx.x;
    if (i >= n) return;
    const cks_image im = frame_of(a, frame ? frame[i] : 0);
    int32_t st, it;
    double sh, ox, oy;
    cks_refine(&im, &a.pp, a.wts, xy_in[2 * (size_t)i], xy_in[2 * (size_t)i + 1], &ox, &oy, &st, &it, &sh);
    if (threadIdx.x == 0) {
        xy_out[2 * (size_t)i] = ox; xy_out[2 * (size_t)i + 1] = oy;
        if (info) { info[i].status = st; info[i].iters = it; info[i].shift = sh; }
    }
}

// One workgroup per detection slot of a frame, wave k on corner k.  A detection none of whose corners moved is not written.
__global__ __launch_bounds__(SPD_NT) void k_subpix_dets(SubpixArgs a, ck_detection_t *dets, const uint32_t *counters, int det_cap) {
    const int f = blockIdx.y, slot = blockIdx.x;
    uint32_t nd = counters[(size_t)f * CK_CNT_STRIDE + CK_CNT_DETS];
    if (nd > (uint32_t)det_cap) nd = (uint32_t)det_cap;
    if ((uint32_t)slot >= nd) return;
    ck_detection_t *d = dets + (size_t)f * det_cap + slot;
    const cks_image im = frame_of(a, f);
    const int k = threadIdx.x >> 6;
    const double x0 = d->p[k][0], y0 = d->p[k][1];
    int32_t st, it;
    double sh, ox, oy;
    cks_refine(&im, &a.pp, a.wts, x0, y0, &ox, &oy, &st, &it, &sh);
    __shared__ double r[8];
    __shared__ int moved[4];
    if ((threadIdx.x & 63) == 0) {
        r[2 * k] = ox; r[2 * k + 1] = oy;
        moved[k] = (ox != x0 || oy != y0) ? 1 : 0; // (FLAT and REJECTED return the input's bytes)
    }
    __syncthreads();
    if (threadIdx.x != 0 || !(moved[0] | moved[1] | moved[2] | moved[3])) return;
    const double x[4] = {r[0], r[2], r[4], r[6]}, y[4] = {r[1], r[3], r[5], r[7]};
#pragma unroll
    for (int q = 0; q < 4; q++) { d->p[q][0] = x[q]; d->p[q][1] = y[q]; }
    double G[9], cx, cy;
    if (cks_square_homography(x, y, G) && cks_map(G, 0.0, 0.0, &cx, &cy)) { d->c[0] = cx; d->c[1] = cy; } // (no homography: the centre stays)
}

struct BoardArgs {
    SubpixArgs s;
    ck_board_t board;
    ck_board_params_t bp;
    const ck_detection_t *dets;
    const uint32_t *counters;
    int det_cap;
    double *uv_out;
    uint8_t *tag_state;
    int32_t *n_tags;
};

// One workgroup per frame.  Tags are taken one after the other, the four corners of a tag side by side (wave k on corner k); what a
// round reads (state, the known tags' corners) is not written during the round, so the result is ck_board_corners_host's.
__global__ __launch_bounds__(SPD_NT) void k_board(BoardArgs a) {
    __shared__ double uv[CKS_MAX_TAGS * 8];
    __shared__ double r[8];
    __shared__ uint8_t state[CKS_MAX_TAGS], next[CKS_MAX_TAGS], seen[CKS_MAX_TAGS];
    __shared__ int okk[4], added, known;
    const int f = blockIdx.x, tid = threadIdx.x, k = tid >> 6, lane0 = (tid & 63) == 0;
    const int nt = a.board.rows * a.board.cols, w = a.s.pp.half_win;
    const cks_image im = frame_of(a.s, f);
    for (int t = tid; t < CKS_MAX_TAGS; t += SPD_NT) { state[t] = 0; next[t] = 0; seen[t] = 0; }
    for (int t = tid; t < CKS_MAX_TAGS * 8; t += SPD_NT) uv[t] = 0.0;
    if (tid == 0) known = 0;
    uint32_t nd = a.counters[(size_t)f * CK_CNT_STRIDE + CK_CNT_DETS];
    if (nd > (uint32_t)a.det_cap) nd = (uint32_t)a.det_cap;
    // seeds
    for (uint32_t i = 0; i < nd; i++) {
        const ck_detection_t *d = a.dets + (size_t)f * a.det_cap + i;
        const int t = cks_seed_index(&a.board, d);
        __syncthreads(); // what the detection before this one wrote
        const bool go = t >= 0 && !seen[t];
        __syncthreads(); // everyone has looked before seen[t] changes
        if (!go) continue;
        if (tid == 0) seen[t] = 1;
        double rx, ry;
        const int ok1 = cks_seed_corner(&im, &a.s.pp, &a.bp, a.s.wts, d->p[k][0], d->p[k][1], &rx, &ry);
        if (lane0) { r[2 * k] = rx; r[2 * k + 1] = ry; okk[k] = ok1; }
        __syncthreads();
        if (okk[0] & okk[1] & okk[2] & okk[3]) {
            if (tid < 8) uv[8 * t + tid] = r[tid];
            if (tid == 0) { state[t] = 1; known = known + 1; }
        }
    }
    // rounds
    for (int round = 0; round < a.board.rows + a.board.cols; round++) {
        __syncthreads();
        for (int t = tid; t < nt; t += SPD_NT) next[t] = state[t];
        if (tid == 0) added = 0;
        __syncthreads();
        for (int t = 0; t < nt; t++) {
            if (state[t]) continue;
            int dc, dr;
            const int nb = cks_first_neighbour(&a.board, state, t, &dc, &dr);
            if (nb < 0) continue;
            double x[4], y[4], G[9];
#pragma unroll
            for (int q = 0; q < 4; q++) { x[q] = uv[8 * nb + 2 * q]; y[q] = uv[8 * nb + 2 * q + 1]; }
            if (!cks_square_homography(x, y, G)) continue;
            bool ok = true;
            double mx = 0.0, my = 0.0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                double X, Y, px, py;
                cks_corner_from_neighbour(&a.board, dc, dr, q, &X, &Y);
                ok = ok && cks_map(G, X, Y, &px, &py) && !cks_near_edge(&im, w, px, py);
                if (q == k) { mx = px; my = py; }
            }
            if (!ok) continue; // (the same for every thread: all of them computed it from the same numbers)
            double rx, ry;
            const int ok1 = cks_board_corner(&im, &a.s.pp, &a.bp, a.s.wts, mx, my, &rx, &ry);
            if (lane0) { r[2 * k] = rx; r[2 * k + 1] = ry; okk[k] = ok1; }
            __syncthreads();
            if (okk[0] & okk[1] & okk[2] & okk[3]) {
                if (tid < 8) uv[8 * t + tid] = r[tid];
                if (tid == 0) { next[t] = 2; added = added + 1; }
            }
            __syncthreads(); // before the next tag writes r and okk
        }
        __syncthreads();
        for (int t = tid; t < nt; t += SPD_NT) state[t] = next[t];
        const int got = added;
        if (tid == 0) known = known + got;
        if (!got) break;
    }
    __syncthreads();
    for (int t = tid; t < nt * 8; t += SPD_NT) a.uv_out[(size_t)f * nt * 8 + t] = uv[t];
    for (int t = tid; t < nt; t += SPD_NT) a.tag_state[(size_t)f * nt + t] = state[t];
    if (tid == 0) a.n_tags[f] = known;
}

// memory of the handle's device that a kernel may use as it is; anything else goes through a copy
bool on_device(const void *p, int device) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError(); // (pageable host memory is unknown to the runtime: an error here, not a failure of the call)
        return false;
    }
    return a.type == hipMemoryTypeDevice && a.device == device;
}

SubpixArgs make_args(const ck_handle *h, const ck_subpix_params_t &pp, const ck_dev_image &img, const double *d_wts) {
    SubpixArgs a;
    a.pp = pp; a.frames = img.p; a.stride = img.stride; a.pitch = img.pitch; a.w = h->w; a.h = h->h; a.wts = d_wts;
    return a;
}

} // namespace

int ck_launch_subpix_dets(ck_handle *h, const ck_dev_image &img, int n) {
    if (!h->has_subpix || n < 1) return CK_OK;
    const SubpixArgs a = make_args(h, h->subpix, img, h->subpix_ws->d_set_wts);
    hipLaunchKernelGGL(k_subpix_dets, dim3((unsigned)h->ws.det_cap, (unsigned)n), dim3(SPD_NT), 0, h->stream, a, h->ws.d_dets, h->ws.d_counters,
                       h->ws.det_cap);
    CK_HIP(hipGetLastError());
    return CK_OK;
}

extern "C" int ck_set_corner_subpix(ck_handle_t *h, const ck_subpix_params_t *pp) {
    if (!h) return CK_EINVAL;
    if (!pp) { h->has_subpix = 0; return CK_OK; }
    double wts[CKS_MAX_TAPS];
    const int rc = ck_subpix_weights(pp, wts);
    if (rc != CK_OK) return rc;
    CK_HIP(hipSetDevice(h->device));
    if (!ck_workspace(h->subpix_ws)) return CK_ENOMEM;
    const int rc2 = h->subpix_ws->d_set_wts.reserve(sizeof wts, true);
    if (rc2 != CK_OK) return rc2;
    CK_HIP(hipStreamSynchronize(h->stream)); // (nothing in flight reads the table being replaced)
    CK_HIP(hipMemcpy(h->subpix_ws->d_set_wts, wts, sizeof wts, hipMemcpyHostToDevice));
    h->subpix = *pp;
    h->has_subpix = 1;
    return CK_OK;
}

extern "C" int ck_corner_subpix(ck_handle_t *h, const ck_subpix_params_t *pp, const int32_t *frame, const double *xy_in, int32_t n,
                                double *xy_out, ck_subpix_info_t *info) {
    if (!h) return CK_EINVAL;
    double wts[CKS_MAX_TAPS];
    int rc = ck_subpix_weights(pp, wts);
    if (rc != CK_OK) return rc;
    if (n < 0) return CK_EINVAL;
    if (n == 0) return CK_OK;
    if (!xy_in || !xy_out || h->n_staged < 1) return CK_EINVAL;
    CK_HIP(hipSetDevice(h->device));
    // the points and their frames are checked on the host, wherever they lie
    std::vector<double> hxy((size_t)n * 2);
    std::vector<int32_t> hfr(frame ? (size_t)n : 0);
    CK_HIP(hipMemcpy(hxy.data(), xy_in, sizeof(double) * hxy.size(), hipMemcpyDefault));
    if (frame) CK_HIP(hipMemcpy(hfr.data(), frame, sizeof(int32_t) * hfr.size(), hipMemcpyDefault));
    for (int i = 0; i < n; i++) {
        const int f = frame ? hfr[(size_t)i] : 0;
        if (f < 0 || f >= h->n_staged || !ck_subpix_point_ok(hxy[2 * (size_t)i], hxy[2 * (size_t)i + 1], h->w, h->h)) return CK_EINVAL;
    }
    if (!ck_workspace(h->subpix_ws)) return CK_ENOMEM;
    ck_subpix_ws &W = *h->subpix_ws;
    const bool in_here = on_device(xy_in, h->device), fr_here = frame && on_device(frame, h->device);
    const bool out_here = on_device(xy_out, h->device), info_here = info && on_device(info, h->device);
    rc = W.d_wts.reserve(sizeof wts, true);
    if (rc == CK_OK && !in_here) rc = W.d_in.reserve(sizeof(double) * 2 * (size_t)n);
    if (rc == CK_OK && frame && !fr_here) rc = W.d_frame.reserve(sizeof(int32_t) * (size_t)n);
    if (rc == CK_OK && !out_here) rc = W.d_out.reserve(sizeof(double) * 2 * (size_t)n);
    if (rc == CK_OK && info && !info_here) rc = W.d_info.reserve(sizeof(ck_subpix_info_t) * (size_t)n);
    if (rc != CK_OK) return rc;
    // the copies below read wts, hxy and hfr while they are in flight: no return before the stream has drained
    auto enqueue = [&]() -> int {
        CK_HIP(hipMemcpyAsync(W.d_wts, wts, sizeof wts, hipMemcpyHostToDevice, h->stream));
        if (!in_here) CK_HIP(hipMemcpyAsync(W.d_in, hxy.data(), sizeof(double) * hxy.size(), hipMemcpyHostToDevice, h->stream));
        if (frame && !fr_here) CK_HIP(hipMemcpyAsync(W.d_frame, hfr.data(), sizeof(int32_t) * hfr.size(), hipMemcpyHostToDevice, h->stream));
        const double *d_in = in_here ? xy_in : W.d_in.p;
        const int32_t *d_frame = !frame ? nullptr : (fr_here ? frame : W.d_frame.p);
        double *d_out = out_here ? xy_out : W.d_out.p;
        ck_subpix_info_t *d_info = !info ? nullptr : (info_here ? info : W.d_info.p);
        const SubpixArgs a = make_args(h, *pp, ck_staged_image(h), W.d_wts);
        hipLaunchKernelGGL(k_subpix, dim3((unsigned)n), dim3(SP_NT), 0, h->stream, a, d_frame, d_in, (int)n, d_out, d_info);
        CK_HIP(hipGetLastError());
        if (!out_here) CK_HIP(hipMemcpyAsync(xy_out, d_out, sizeof(double) * 2 * (size_t)n, hipMemcpyDeviceToHost, h->stream));
        if (info && !info_here) CK_HIP(hipMemcpyAsync(info, d_info, sizeof(ck_subpix_info_t) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
        return CK_OK;
    };
    rc = enqueue();
    if (rc != CK_OK) { (void)hipStreamSynchronize(h->stream); return rc; }
    CK_HIP(hipStreamSynchronize(h->stream));
    return CK_OK;
}

extern "C" int ck_board_corners_last(ck_handle_t *h, const ck_board_t *board, const ck_subpix_params_t *pp, const ck_board_params_t *bp,
                                     double *uv_out, uint8_t *tag_state, int32_t *n_tags) {
    if (!h) return CK_EINVAL;
    double wts[CKS_MAX_TAPS];
    int rc = ck_subpix_weights(pp, wts);
    if (rc == CK_OK) rc = ck_board_check(board, bp, h->cfg.n_families);
    if (rc != CK_OK) return rc;
    if (!uv_out || !tag_state || !n_tags) return CK_EINVAL;
    if (h->n_last_dets < 1 || !h->last_img_p) return CK_EINVAL; // nothing detected since ck_create, or the workspace was rewritten since
    const int n = h->n_last_dets, nt = board->rows * board->cols;
    CK_HIP(hipSetDevice(h->device));
    if (!ck_workspace(h->subpix_ws)) return CK_ENOMEM;
    ck_subpix_ws &W = *h->subpix_ws;
    const bool uv_here = on_device(uv_out, h->device), st_here = on_device(tag_state, h->device), nt_here = on_device(n_tags, h->device);
    const size_t uv_bytes = sizeof(double) * 8 * (size_t)nt * (size_t)n, st_bytes = (size_t)nt * (size_t)n, nt_bytes = sizeof(int32_t) * (size_t)n;
    rc = W.d_wts.reserve(sizeof wts, true);
    if (rc == CK_OK && !uv_here) rc = W.d_out.reserve(uv_bytes);
    if (rc == CK_OK && !st_here) rc = W.d_state.reserve(st_bytes);
    if (rc == CK_OK && !nt_here) rc = W.d_ntags.reserve(nt_bytes);
    if (rc != CK_OK) return rc;
    auto enqueue = [&]() -> int { // (the copy reads wts while it is in flight)
        CK_HIP(hipMemcpyAsync(W.d_wts, wts, sizeof wts, hipMemcpyHostToDevice, h->stream));
        BoardArgs a;
        a.s = make_args(h, *pp, {h->last_img_p, h->last_img_stride, h->last_img_pitch}, W.d_wts);
        a.board = *board; a.bp = *bp; a.dets = h->ws.d_dets; a.counters = h->ws.d_counters; a.det_cap = h->ws.det_cap;
        a.uv_out = uv_here ? uv_out : W.d_out.p; a.tag_state = st_here ? tag_state : W.d_state.p; a.n_tags = nt_here ? n_tags : W.d_ntags.p;
        hipLaunchKernelGGL(k_board, dim3((unsigned)n), dim3(SPD_NT), 0, h->stream, a);
        CK_HIP(hipGetLastError());
        if (!uv_here) CK_HIP(hipMemcpyAsync(uv_out, a.uv_out, uv_bytes, hipMemcpyDeviceToHost, h->stream));
        if (!st_here) CK_HIP(hipMemcpyAsync(tag_state, a.tag_state, st_bytes, hipMemcpyDeviceToHost, h->stream));
        if (!nt_here) CK_HIP(hipMemcpyAsync(n_tags, a.n_tags, nt_bytes, hipMemcpyDeviceToHost, h->stream));
        return CK_OK;
    };
    rc = enqueue();
    if (rc != CK_OK) { (void)hipStreamSynchronize(h->stream); return rc; }
    CK_HIP(hipStreamSynchronize(h->stream));
    return CK_OK;
}
