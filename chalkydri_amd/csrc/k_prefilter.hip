// k_prefilter.hip — quad_sigma: Gaussian blur (sigma > 0) or unsharp mask (sigma < 0) of the quad image.
//
// One kernel reads the frames (decimating them on the way when quad_decimate = 2) and writes Q into d_qframes, rows padded to
// 16 bytes like every staged frame.  The contract restated from AprilTag-3's image_u8_gaussian_blur / convolve:
//   row pass    y[i] = (sum_j k[j] * x[i - h + j]) >> 8 for h <= i <= qw - h - 2, y[i] = x[i] elsewhere (truncated to u8)
//   column pass the same along every column of the row pass's result
//   sigma < 0   Q = clamp(2 D - B, 0, 255)
// A workgroup takes one frame and a TW x TH tile of output pixels.  The tile's input rows (TH + 2 HC of them) are loaded in
// 16-byte chunks into LDS (A); the row pass writes its bytes TRANSPOSED into LDS (BT: one row of bytes per column), so that the
// column pass is the row pass again.  Four taps per v_dot4_u32_u8: the weights are zero-padded to KP taps (a multiple of 4)
// around a fixed centre HC per size class, so a window always starts HC pixels before its output pixel, whatever ksz is.
#include "ck_internal.h"

namespace {

constexpr int TW = 256; // output columns of a tile (one wave of 64 lanes x 4 pixels)
constexpr int NT = 256;

template <int CLS> struct qf_class;
template <> struct qf_class<0> { static constexpr int HC = 2, KP = 8, TH = 32; };   // ksz <= 5
template <> struct qf_class<1> { static constexpr int HC = 4, KP = 12, TH = 32; };  // ksz <= 9
template <> struct qf_class<2> { static constexpr int HC = 8, KP = 20, TH = 64; };  // ksz <= 17
template <> struct qf_class<3> { static constexpr int HC = 16, KP = 36, TH = 64; }; // ksz <= 33

struct qf_weights { uint32_t k4[9]; }; // KP taps, four per dword (little-endian: tap 4m + b in byte b of k4[m])

__device__ __forceinline__ uint32_t bytes_at(const uint32_t *d, int e) { // the 4 bytes starting e bytes into d[0] (e compile-time)
    const int w = e >> 2, s = e & 3;
    return s == 0 ? d[w] : __builtin_amdgcn_alignbyte(d[w + 1], d[w], (uint32_t)s);
}
// 4x4 byte transpose: out[r].byte[c] = in[c].byte[r]
__device__ __forceinline__ void transpose4(const uint32_t in[4], uint32_t out[4]) {
    const uint32_t lo01 = __builtin_amdgcn_perm(in[1], in[0], 0x05010400u), hi01 = __builtin_amdgcn_perm(in[1], in[0], 0x07030602u);
    const uint32_t lo23 = __builtin_amdgcn_perm(in[3], in[2], 0x05010400u), hi23 = __builtin_amdgcn_perm(in[3], in[2], 0x07030602u);
    out[0] = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u); out[1] = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
    out[2] = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u); out[3] = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
}
// four outputs of one 1-D pass: window of output q starts S + q bytes into the dwords d[] (S compile-time); an output outside
// [lo, hi] keeps the byte `keep` gives it
template <int KP, int S>
__device__ __forceinline__ uint32_t pass4(const uint32_t *d, const qf_weights &k, int i0, int lo, int hi, uint32_t keep) {
    uint32_t out = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        uint32_t acc = 0;
#pragma unroll
        for (int m = 0; m < KP / 4; m++) acc = __builtin_amdgcn_udot4(bytes_at(d, S + q + 4 * m), k.k4[m], acc, false);
        const int i = i0 + q;
        const uint32_t v = (i >= lo && i <= hi) ? (acc >> 8) : ((keep >> (8 * q)) & 0xFFu);
        out |= v << (8 * q);
    }
    return out;
}

// grid: x = tile (tiles_x * tiles_y), y = frame.  src rows 16-byte aligned (stride, frame_pitch, base); dst rows qstride bytes.
template <int CLS, int F, bool SHARP>
__global__ __launch_bounds__(NT) void k_prefilter(const uint8_t *__restrict__ src, size_t frame_pitch, int stride, int qw, int qh, int tiles_x,
                                                  int h, qf_weights k, uint8_t *__restrict__ dst, int qstride, size_t qpitch) {
    using C = qf_class<CLS>;
    constexpr int HC = C::HC, KP = C::KP, TH = C::TH;
    constexpr int RA = TH + 2 * HC;                                 // input rows of the tile (rows of A and of the row pass)
    constexpr int AW = (TW + KP + 24 + 15) / 16 * 16;               // bytes per A row: input columns x0 - 16 .. x0 - 16 + AW - 1
    constexpr int AWD = AW / 4;
    constexpr int BSTR = (((TH + KP) / 4) | 1);                     // dwords per BT column (odd: conflict-free across columns)
    __shared__ __attribute__((aligned(16))) uint32_t A[RA * AWD];
    __shared__ uint32_t BT[TW * BSTR];                               // column c = 4 t + q at (q * 64 + t) * BSTR

    const int tile = blockIdx.x, fr = blockIdx.y;
    const int x0 = (tile % tiles_x) * TW, y0 = (tile / tiles_x) * TH;
    const uint8_t *s = src + (size_t)fr * frame_pitch;

    // ---- load: A[rr][c] = D[y0 - HC + rr][x0 - 16 + c], zero outside the image
    if (F == 1) {
        constexpr int CH = AW / 16;
        for (int it = threadIdx.x; it < RA * CH; it += NT) {
            const int rr = it / CH, kk = it - rr * CH;
            const int y = y0 - HC + rr, cq = x0 - 16 + 16 * kk;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (y >= 0 && y < qh && cq >= 0 && cq < qw) v = *reinterpret_cast<const uint4 *>(s + (size_t)y * stride + cq);
            *reinterpret_cast<uint4 *>(&A[rr * AWD + 4 * kk]) = v;
        }
    } else {
        constexpr int CH = AW / 8; // one 16-byte chunk of a source row = 8 quad pixels
        for (int it = threadIdx.x; it < RA * CH; it += NT) {
            const int rr = it / CH, kk = it - rr * CH;
            const int y = y0 - HC + rr, cq = x0 - 16 + 8 * kk;
            uint2 o = make_uint2(0, 0);
            if (y >= 0 && y < qh && cq >= 0 && cq < qw) {
                const uint4 v = *reinterpret_cast<const uint4 *>(s + (size_t)(2 * y) * stride + 2 * cq);
                o.x = __builtin_amdgcn_perm(v.y, v.x, 0x06040200u);
                o.y = __builtin_amdgcn_perm(v.w, v.z, 0x06040200u);
            }
            *reinterpret_cast<uint2 *>(&A[rr * AWD + 2 * kk]) = o;
        }
    }
    __syncthreads();

    // ---- row pass: a thread takes 4 rows x 4 columns (output columns x0 + 4t .. + 3), writes the block transposed into BT
    {
        constexpr int S = 16 - HC; // window of output column x0 + 4t starts at A byte 4t + 16 - HC
        constexpr int ND = KP / 4 + 2; // bytes (S & 3) + q + 4 m .. + 3, q <= 3, m < KP / 4: dwords 0 .. KP / 4 + 1
        const int lo = h, hi = qw - h - 2;
        for (int it = threadIdx.x; it < (RA / 4) * (TW / 4); it += NT) {
            const int rq = it / (TW / 4), t = it - rq * (TW / 4);
            uint32_t rows[4], cols[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const uint32_t *ar = &A[(4 * rq + r) * AWD + t + (S >> 2)];
                uint32_t d[ND];
#pragma unroll
                for (int m = 0; m < ND; m++) d[m] = ar[m];
                const uint32_t keep = A[(4 * rq + r) * AWD + t + 4]; // D at the four output columns
                rows[r] = pass4<KP, (S & 3)>(d, k, x0 + 4 * t, lo, hi, keep);
            }
            transpose4(rows, cols);
#pragma unroll
            for (int q = 0; q < 4; q++) BT[(q * (TW / 4) + t) * BSTR + rq] = cols[q];
        }
    }
    __syncthreads();

    // ---- column pass: a thread takes 4 output rows x 4 columns; transposed back, unsharp step, one dword store per row
    {
        // window of output row y0 + o starts at BT byte o (o a multiple of 4): bytes r + 4 m .. + 3, r <= 3, m < KP / 4.  Dwords
        // past the RA / 4 the row pass wrote meet zero weights only (the taps that matter end at row TH - 1 + 2 HC)
        constexpr int ND = KP / 4 + 1;
        const int lo = h, hi = qh - h - 2;
        for (int it = threadIdx.x; it < (TH / 4) * (TW / 4); it += NT) {
            const int og = it / (TW / 4), t = it - og * (TW / 4);
            const int c = x0 + 4 * t;
            if (c >= qstride || y0 + 4 * og >= qh) continue;
            uint32_t cols[4], rows[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t *bc = &BT[(q * (TW / 4) + t) * BSTR + og];
                uint32_t d[ND];
#pragma unroll
                for (int m = 0; m < ND; m++) d[m] = bc[m];
                const uint32_t keep = bytes_at(d, HC); // the row pass's bytes at the four output rows
                cols[q] = pass4<KP, 0>(d, k, y0 + 4 * og, lo, hi, keep);
            }
            transpose4(cols, rows);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int y = y0 + 4 * og + r;
                if (y >= qh) break;
                uint32_t v = rows[r];
                if (SHARP) {
                    const uint32_t dv = A[(4 * og + r + HC) * AWD + t + 4];
                    uint32_t o = 0;
#pragma unroll
                    for (int b = 0; b < 4; b++) {
                        const int x = 2 * (int)((dv >> (8 * b)) & 0xFFu) - (int)((v >> (8 * b)) & 0xFFu);
                        o |= (uint32_t)(x < 0 ? 0 : (x > 255 ? 255 : x)) << (8 * b);
                    }
                    v = o;
                }
                *reinterpret_cast<uint32_t *>(dst + (size_t)fr * qpitch + (size_t)y * qstride + c) = v;
            }
        }
    }
}

template <int CLS, int F>
void launch_cls(ck_handle *h, const ck_dev_image &img, int n, const qf_weights &k, bool sharp) {
    const int tiles_x = (h->qw + TW - 1) / TW, tiles_y = (h->qh + qf_class<CLS>::TH - 1) / qf_class<CLS>::TH;
    const ck_dev_image q = ck_qframes_image(h);
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)n);
    if (sharp)
        hipLaunchKernelGGL((k_prefilter<CLS, F, true>), grid, dim3(NT), 0, h->stream, img.p, img.pitch, img.stride, h->qw, h->qh, tiles_x,
                           h->qf_ksz / 2, k, h->d_qframes, q.stride, q.pitch);
    else
        hipLaunchKernelGGL((k_prefilter<CLS, F, false>), grid, dim3(NT), 0, h->stream, img.p, img.pitch, img.stride, h->qw, h->qh, tiles_x,
                           h->qf_ksz / 2, k, h->d_qframes, q.stride, q.pitch);
}

} // namespace

// Q of frames [0, n) into h->d_qframes with the handle's current weights (by value: a batch keeps the sigma it was enqueued with)
int ck_launch_prefilter(ck_handle *h, const ck_dev_image &img, int n) {
    const int ksz = h->qf_ksz, half = ksz / 2;
    if (ksz <= 1 || ksz > 33 || !h->d_qframes) return CK_EINVAL;
    if (n == 0) return CK_OK;
    const int cls = ksz <= 5 ? 0 : (ksz <= 9 ? 1 : (ksz <= 17 ? 2 : 3));
    static const int hcs[4] = {2, 4, 8, 16};
    // the ksz taps centred on tap hc of the class's zero-padded window
    uint8_t taps[36] = {0};
    for (int j = 0; j < ksz; j++) taps[hcs[cls] - half + j] = h->qf_k[j];
    qf_weights k;
    for (int m = 0; m < 9; m++)
        k.k4[m] = (uint32_t)taps[4 * m] | ((uint32_t)taps[4 * m + 1] << 8) | ((uint32_t)taps[4 * m + 2] << 16) | ((uint32_t)taps[4 * m + 3] << 24);
    const bool sharp = h->quad_sigma < 0;
    const bool dec = h->cfg.quad_decimate > 1;
    switch (cls) {
    case 0: dec ? launch_cls<0, 2>(h, img, n, k, sharp) : launch_cls<0, 1>(h, img, n, k, sharp); break;
    case 1: dec ? launch_cls<1, 2>(h, img, n, k, sharp) : launch_cls<1, 1>(h, img, n, k, sharp); break;
    case 2: dec ? launch_cls<2, 2>(h, img, n, k, sharp) : launch_cls<2, 1>(h, img, n, k, sharp); break;
    default: dec ? launch_cls<3, 2>(h, img, n, k, sharp) : launch_cls<3, 1>(h, img, n, k, sharp); break;
    }
    CK_HIP(hipGetLastError());
    return CK_OK;
}
