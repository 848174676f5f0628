// JPEG preview of the staged frames, the device half: nearest-neighbour scale + detection overlay + libjpeg's
// integer forward DCT and quantiser, Huffman coding with the Annex-K luminance tables, bit packing, byte stuffing and restart
// markers.  Every stage is data-parallel over the blocks (or the bytes) of all frames of a call; nothing comes back to the host
// between the stages.  The files equal libjpeg's byte for byte (tests/np_jpeg_enc.py restates it).
// The colour form (§4g) has a front end of its own, k_pv_fdct_color: it gathers from the RAW frames (orientation, packed 2 / 3 / 4
// byte pixels, libjpeg's colour conversion) one block per (MCU, component), and hands the same stages the interleaved block
// sequence Y Cb Cr Y Cb Cr ...: there NC = 3, a block's component is its index mod 3, its DC predecessor lies three blocks back
// and components 1 and 2 use the chrominance tables.  NC = 1 is the grey code as it was.  The front end is a template over the kind
// of source: the raw families, or the frames of a JPEG decode that kept its chroma planes (§4i).
#include "ck_jpeg_tables.h"
#include "ck_preview.h"
#include "ck_pv_source.h"

namespace {

constexpr int PV_NT = 256;

// zig-zag index -> natural index (ITU-T T.81 figure A.6)
__device__ constexpr uint8_t kZZ[64] = CK_JPEG_NATURAL_ORDER;

// the encoder's view of both tables: [symbol] = code | length << 16 (0 = the symbol has no code); DC at 0..15, AC at 16..271;
// the luminance pair (Annex K.3) first, the chrominance pair behind it
constexpr int PV_ENC_WORDS = 16 + 256;
struct HuffEnc { uint32_t e[2 * PV_ENC_WORDS]; };
constexpr HuffEnc make_enc() {
    HuffEnc t{};
    for (int set = 0; set < 2; set++)
        for (int cls = 0; cls < 2; cls++) {
            const ck_jpeg_std_huff &s = kStdHuff[cls][set];
            uint32_t code = 0;
            int p = 0;
            for (int l = 1; l <= 16; l++) {
                for (int k = 0; k < s.bits[l - 1]; k++, p++, code++) t.e[set * PV_ENC_WORDS + (cls ? 16 : 0) + s.vals[p]] = code | ((uint32_t)l << 16);
                code <<= 1;
            }
        }
    return t;
}
__device__ constexpr HuffEnc kEnc = make_enc();

// NC = 1: the luminance pair; NC = 3: both
template <int NC = 1>
__device__ __forceinline__ void load_enc(uint32_t *lds) {
    for (int i = threadIdx.x; i < (NC == 3 ? 2 : 1) * PV_ENC_WORDS; i += PV_NT) lds[i] = kEnc.e[i];
    __syncthreads();
}
// the tables of block b of the interleaved sequence
template <int NC>
__device__ __forceinline__ const uint32_t *enc_of(const uint32_t *lds, int b) { return NC == 3 && b % 3 ? lds + PV_ENC_WORDS : lds; }

// ---- overlay: the outline pixels of a frame's detections as a bit image ----------------------------------------------------
__device__ __forceinline__ int corner_px(double p, int pn, int fn) {
    double v = floor(p * (double)pn / (double)fn); // one multiplication, one division, floor (the build never contracts them)
    if (!(v >= 0.0)) v = 0.0;
    if (v > (double)(pn - 1)) v = (double)(pn - 1);
    return (int)v;
}

// one lane per (entry, detection, edge): integer Bresenham, both end points included, always walked from the end point that is
// smaller in (y, x) order, so that an edge and its reverse set the same pixels
__global__ __launch_bounds__(PV_NT) void k_pv_mask(ck_pv_geom g, int n, int det_cap, const int32_t *frames, const ck_detection_t *dets,
                                                   const uint32_t *counters, uint32_t *mask) {
    const long t = (long)blockIdx.x * PV_NT + threadIdx.x;
    if (t >= (long)n * det_cap * 4) return;
    const int e = (int)(t & 3), d = (int)((t >> 2) % det_cap), i = (int)((t >> 2) / det_cap);
    const int f = frames[i];
    uint32_t nd = counters[(size_t)f * CK_CNT_STRIDE + CK_CNT_DETS];
    if (nd > (uint32_t)det_cap) nd = (uint32_t)det_cap;
    if ((uint32_t)d >= nd) return;
    const ck_detection_t *D = &dets[(size_t)f * det_cap + d];
    int x0 = corner_px(D->p[e][0], g.pw, g.W), y0 = corner_px(D->p[e][1], g.ph, g.H);
    int x1 = corner_px(D->p[(e + 1) & 3][0], g.pw, g.W), y1 = corner_px(D->p[(e + 1) & 3][1], g.ph, g.H);
    if (y1 < y0 || (y1 == y0 && x1 < x0)) { int s = x0; x0 = x1; x1 = s; s = y0; y0 = y1; y1 = s; }
    const int dx = abs(x1 - x0), dy = -abs(y1 - y0), sx = x0 < x1 ? 1 : -1, sy = y0 < y1 ? 1 : -1;
    int err = dx + dy;
    uint32_t *m = mask + (size_t)i * g.mask_words;
    for (int step = 0; step <= dx - dy; step++) { // (a line has at most dx + |dy| + 1 pixels: the bound keeps the walk inside the preview)
        const int bit = y0 * g.pw + x0;
        atomicOr(&m[bit >> 5], 1u << (bit & 31));
        if (x0 == x1 && y0 == y1) break;
        const int e2 = 2 * err;
        if (e2 >= dy) { err += dy; x0 += sx; }
        if (e2 <= dx) { err += dx; y0 += sy; }
    }
}

// pixel (x, y) of the preview of one frame: the gather of the scale, then the overlay
struct PvSrc { const uint8_t *p; int stride; const uint32_t *mask; };
__device__ __forceinline__ int pv_pixel(const ck_pv_geom &g, const PvSrc &s, int x, int y, int sx, int sy) {
    int v = s.p[(size_t)sy * s.stride + sx];
    if (s.mask) {
        const int bit = y * g.pw + x;
        if ((s.mask[bit >> 5] >> (bit & 31)) & 1u) v = v < 128 ? 255 : 0;
    }
    return v;
}

__global__ __launch_bounds__(PV_NT) void k_pv_luma(ck_pv_geom g, int n, ck_dev_image img, const int32_t *frames, const uint32_t *mask, uint8_t *out) {
    const long t = (long)blockIdx.x * PV_NT + threadIdx.x;
    const long npx = (long)g.pw * g.ph;
    if (t >= npx * n) return;
    const int i = (int)(t / npx), r = (int)(t - i * npx), y = r / g.pw, x = r - y * g.pw;
    const PvSrc s = {img.p + (size_t)frames[i] * img.pitch, img.stride, g.overlay ? mask + (size_t)i * g.mask_words : nullptr};
    out[t] = (uint8_t)pv_pixel(g, s, x, y, ((2 * x + 1) * g.W) / (2 * g.pw), ((2 * y + 1) * g.H) / (2 * g.ph));
}

// the triples the encoder is given, [n][ph][pw][3]: one lane per byte
template <class SRC>
__device__ __forceinline__ void pv_triples(const ck_pv_geom &g, const SRC &s, int n, const int32_t *frames, const uint32_t *mask, uint8_t *out) {
    const long t = (long)blockIdx.x * PV_NT + threadIdx.x;
    const long npx = (long)g.pw * g.ph;
    if (t >= npx * n * 3) return;
    const long q = t / 3;
    const int i = (int)(q / npx), r = (int)(q - i * npx), y = r / g.pw, x = r - y * g.pw;
    const typename SRC::Lane L = s.lane((int)(t - q * 3));
    const int at = s.term_x(L, ((2 * x + 1) * g.W) / (2 * g.pw)) + s.term_y(L, ((2 * y + 1) * g.H) / (2 * g.ph));
    out[t] = (uint8_t)s.pixel(s.frame(frames[i]), at, L, g.overlay ? mask + (size_t)i * g.mask_words : nullptr, r);
}
template <bool YUV>
__global__ __launch_bounds__(PV_NT) void k_pv_color(ck_pv_geom g, ck_pv_csrc s, int n, const int32_t *frames, const uint32_t *mask, uint8_t *out) {
    pv_triples(g, Raw<YUV>{s}, n, frames, mask, out);
}
// ... from the planar 4:2:0 raw formats (§4s)
__global__ __launch_bounds__(PV_NT) void k_pv_ptriples(ck_pv_geom g, ck_pv_psrc s, int n, const int32_t *frames, const uint32_t *mask, uint8_t *out) {
    pv_triples(g, Planar{s}, n, frames, mask, out);
}
__global__ __launch_bounds__(PV_NT) void k_pv_jtriples(ck_pv_geom g, ck_pv_jsrc s, int n, const int32_t *frames, const uint32_t *mask, uint8_t *out) {
    pv_triples(g, Decoded{s}, n, frames, mask, out);
}

// ---- forward DCT: libjpeg's jpeg_fdct_islow ------------------------------------------------------------------------------------
// CONST_BITS 13, PASS1_BITS 2.  32-bit arithmetic is exact here (libjpeg's JLONG is not needed): samples are in [-128, 127], a
// 1-D pass amplifies by at most 8 (sum of |cos| times sqrt 2), so after the row pass (scaled by 4) |v| <= 4097; in the column pass
// the even part is at most 32776 * 4433 + 16388 * 15137 < 4.0e8 and the odd part at most 8194 * 25172 + 16388 * 20995 +
// 16388 * 16069 + 32776 * 9633 < 1.14e9, plus the rounding constant 2^14: below 2^31 = 2.147e9 with a factor 1.8 to spare.  The
// extreme blocks of the tests (all 0, all 255, checkerboards, single pixel) are the inputs that come closest.
template <bool FIRST>
__device__ __forceinline__ void fdct_1d(int &d0, int &d1, int &d2, int &d3, int &d4, int &d5, int &d6, int &d7) {
    constexpr int SH = FIRST ? 11 : 15, RND = 1 << (SH - 1);
    int tmp0 = d0 + d7, tmp7 = d0 - d7, tmp1 = d1 + d6, tmp6 = d1 - d6, tmp2 = d2 + d5, tmp5 = d2 - d5, tmp3 = d3 + d4, tmp4 = d3 - d4;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    if (FIRST) { d0 = (tmp10 + tmp11) * 4; d4 = (tmp10 - tmp11) * 4; }
    else { d0 = (tmp10 + tmp11 + 2) >> 2; d4 = (tmp10 - tmp11 + 2) >> 2; }
    int z1 = (tmp12 + tmp13) * 4433;
    d2 = (z1 + tmp13 * 6270 + RND) >> SH;
    d6 = (z1 + tmp12 * -15137 + RND) >> SH;
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * 9633;
    tmp4 *= 2446; tmp5 *= 16819; tmp6 *= 25172; tmp7 *= 12299;
    z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
    d7 = (tmp4 + z1 + z3 + RND) >> SH;
    d5 = (tmp5 + z2 + z4 + RND) >> SH;
    d3 = (tmp6 + z2 + z3 + RND) >> SH;
    d1 = (tmp7 + z1 + z4 + RND) >> SH;
}

__device__ __forceinline__ int category(int v) { return 32 - __clz(abs(v)); }

// What follows the row passes of block t, whose rows are in d[]: column pass, libjpeg's quantiser (sign-magnitude, (|c| + qval / 2)
// / qval with qval = 8 q: the exact integer quotient; the chrominance divisors where `chroma`), coefficients out in zig-zag order;
// the block's AC bit count under the tables `enc` and its DC beside them for the scan that places the blocks.
__device__ __forceinline__ void fdct_finish(int (&d)[64], const ck_pv_tables &tab, bool chroma, const uint32_t *enc, long t, int16_t *coef,
                                            int16_t *dc, uint32_t *len) {
#pragma unroll
    for (int c = 0; c < 8; c++) fdct_1d<false>(d[c], d[8 + c], d[16 + c], d[24 + c], d[32 + c], d[40 + c], d[48 + c], d[56 + c]);
#pragma unroll
    for (int k = 0; k < 64; k++) {
        const int q = chroma ? tab.qdiv[1][k] : tab.qdiv[0][k], a = (abs(d[k]) + (q >> 1)) / q;
        d[k] = d[k] < 0 ? -a : a;
    }
    // AC bits: (run, size) codes + value bits, ZRL for every 16 zeros in front of a coefficient, EOB after the last one
    uint32_t bits = 0;
    int run = 0;
    uint32_t zz[32];
#pragma unroll
    for (int k = 0; k < 64; k++) {
        const int v = d[kZZ[k]];
        if (k & 1) zz[k >> 1] |= (uint32_t)(uint16_t)v << 16; else zz[k >> 1] = (uint16_t)v;
        if (k == 0) continue;
        if (v == 0) { run++; continue; }
        bits += (uint32_t)(run >> 4) * (enc[16 + 0xF0] >> 16);
        const int sz = category(v);
        bits += (enc[16 + (((run & 15) << 4) | sz)] >> 16) + (uint32_t)sz;
        run = 0;
    }
    if (run) bits += enc[16] >> 16;
    uint4 *o = reinterpret_cast<uint4 *>(coef + (size_t)t * 64);
#pragma unroll
    for (int k = 0; k < 8; k++) o[k] = make_uint4(zz[4 * k], zz[4 * k + 1], zz[4 * k + 2], zz[4 * k + 3]);
    dc[t] = (int16_t)d[0];
    len[t] = bits;
}

// One 8 x 8 block per lane, the block in registers: gather (scale + overlay, right / bottom edge replicated), level shift, row
// pass, then fdct_finish.
__global__ __launch_bounds__(PV_NT) void k_pv_fdct(ck_pv_geom g, ck_pv_tables tab, int n, ck_dev_image img, const int32_t *frames,
                                                   const uint32_t *mask, int16_t *coef, int16_t *dc, uint32_t *len) {
    __shared__ uint32_t enc[PV_ENC_WORDS];
    load_enc(enc);
    const long t = (long)blockIdx.x * PV_NT + threadIdx.x;
    if (t >= (long)n * g.nblk) return;
    const int i = (int)(t / g.nblk), b = (int)(t - (long)i * g.nblk), by = b / g.bw, bx = b - by * g.bw;
    const PvSrc s = {img.p + (size_t)frames[i] * img.pitch, img.stride, g.overlay ? mask + (size_t)i * g.mask_words : nullptr};
    int px[8], sx[8];
#pragma unroll
    for (int c = 0; c < 8; c++) {
        px[c] = min(bx * 8 + c, g.pw - 1);
        sx[c] = ((2 * px[c] + 1) * g.W) / (2 * g.pw);
    }
    int d[64];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int py = min(by * 8 + r, g.ph - 1), sy = ((2 * py + 1) * g.H) / (2 * g.ph);
#pragma unroll
        for (int c = 0; c < 8; c++) d[r * 8 + c] = pv_pixel(g, s, px[c], py, sx[c], sy) - 128;
        fdct_1d<true>(d[r * 8], d[r * 8 + 1], d[r * 8 + 2], d[r * 8 + 3], d[r * 8 + 4], d[r * 8 + 5], d[r * 8 + 6], d[r * 8 + 7]);
    }
    fdct_finish(d, tab, false, enc, t, coef, dc, len);
}

// The colour front end (§4g): one block per lane again, the lane's block being component t % 3 of MCU t / 3 of the frame — so the
// coefficients come out in scan order.  The gather reads the raw frame through the orientation's index map and converts on the
// way: no colour image is materialised.
template <class SRC>
__device__ __forceinline__ void pv_fdct_color(const ck_pv_geom &g, const ck_pv_tables &tab, const SRC &s, int n, const int32_t *frames,
                                              const uint32_t *mask, int16_t *coef, int16_t *dc, uint32_t *len, uint32_t *enc) {
    load_enc<3>(enc);
    const long t = (long)blockIdx.x * PV_NT + threadIdx.x;
    if (t >= (long)n * g.nblk) return;
    const int i = (int)(t / g.nblk), b = (int)(t - (long)i * g.nblk), m = b / 3, by = m / g.bw, bx = m - by * g.bw;
    const typename SRC::Lane L = s.lane(b - 3 * m);
    const typename SRC::Frame P = s.frame(frames[i]);
    const uint32_t *M = g.overlay ? mask + (size_t)i * g.mask_words : nullptr;
    int px[8], tx[8];
#pragma unroll
    for (int c = 0; c < 8; c++) {
        px[c] = min(bx * 8 + c, g.pw - 1);
        tx[c] = s.term_x(L, ((2 * px[c] + 1) * g.W) / (2 * g.pw));
    }
    int d[64];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int py = min(by * 8 + r, g.ph - 1), ty = s.term_y(L, ((2 * py + 1) * g.H) / (2 * g.ph));
#pragma unroll
        for (int c = 0; c < 8; c++) d[r * 8 + c] = s.pixel(P, tx[c] + ty, L, M, py * g.pw + px[c]) - 128;
        fdct_1d<true>(d[r * 8], d[r * 8 + 1], d[r * 8 + 2], d[r * 8 + 3], d[r * 8 + 4], d[r * 8 + 5], d[r * 8 + 6], d[r * 8 + 7]);
    }
    fdct_finish(d, tab, L.comp != 0, enc_of<3>(enc, b), t, coef, dc, len);
}
template <bool YUV>
__global__ __launch_bounds__(PV_NT) void k_pv_fdct_color(ck_pv_geom g, ck_pv_tables tab, ck_pv_csrc s, int n, const int32_t *frames,
                                                         const uint32_t *mask, int16_t *coef, int16_t *dc, uint32_t *len) {
    __shared__ uint32_t enc[2 * PV_ENC_WORDS];
    pv_fdct_color(g, tab, Raw<YUV>{s}, n, frames, mask, coef, dc, len, enc);
}
// ... from the planar 4:2:0 raw formats (§4s)
__global__ __launch_bounds__(PV_NT) void k_pv_pfdct(ck_pv_geom g, ck_pv_tables tab, ck_pv_psrc s, int n, const int32_t *frames,
                                                    const uint32_t *mask, int16_t *coef, int16_t *dc, uint32_t *len) {
    __shared__ uint32_t enc[2 * PV_ENC_WORDS];
    pv_fdct_color(g, tab, Planar{s}, n, frames, mask, coef, dc, len, enc);
}
// ... and from the frames of a JPEG decode in the colour form (§4i)
__global__ __launch_bounds__(PV_NT) void k_pv_jfdct(ck_pv_geom g, ck_pv_tables tab, ck_pv_jsrc s, int n, const int32_t *frames,
                                                    const uint32_t *mask, int16_t *coef, int16_t *dc, uint32_t *len) {
    __shared__ uint32_t enc[2 * PV_ENC_WORDS];
    pv_fdct_color(g, tab, Decoded{s}, n, frames, mask, coef, dc, len, enc);
}

// ---- placement: where every block's bits start --------------------------------------------------------------------------------
// One wave per (entry, restart interval): the exclusive scan of the blocks' bit counts (DC difference from the previous block's
// DC — known, so nothing is sequential — plus the AC bits), four consecutive blocks per lane and step; then the interval's bytes.
// NC = 3: the previous block of the same component, NC blocks back (an interval starts on an MCU), and the component's tables.
template <int NC>
__global__ __launch_bounds__(PV_NT) void k_pv_scan(ck_pv_geom g, int n, const int16_t *dc, uint32_t *len, uint32_t *istart) {
    __shared__ uint32_t enc[(NC == 3 ? 2 : 1) * PV_ENC_WORDS];
    load_enc<NC>(enc);
    const int lane = threadIdx.x & 63;
    const long w = (long)blockIdx.x * (PV_NT / 64) + (threadIdx.x >> 6);
    if (w >= (long)n * g.nint) return;
    const int i = (int)(w / g.nint), j = (int)(w - (long)i * g.nint);
    const int b0 = j * g.R, b1 = min(g.nblk, b0 + g.R);
    const int16_t *D = dc + (size_t)i * g.nblk;
    uint32_t *L = len + (size_t)i * g.nblk;
    uint32_t carry = 0;
    for (int base = b0; base < b1; base += 256) {
        uint32_t v[4], s = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int b = base + lane * 4 + k;
            v[k] = 0;
            if (b < b1) {
                const int diff = (int)D[b] - (b - b0 < NC ? 0 : (int)D[b - NC]), sz = category(diff);
                v[k] = L[b] + (enc_of<NC>(enc, b)[sz] >> 16) + (uint32_t)sz;
            }
            s += v[k];
        }
        const uint32_t incl = wave_scan_u32(s);
        uint32_t at = incl - s + carry;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int b = base + lane * 4 + k;
            if (b < b1) L[b] = at;
            at += v[k];
        }
        carry += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
    if (lane == 0) istart[(size_t)i * (g.nint + 1) + j] = (carry + 7) >> 3;
}

// One wave per entry: the intervals' byte counts become their first byte in the frame's bit buffer; entry nint = all bytes.
__global__ __launch_bounds__(64) void k_pv_iscan(ck_pv_geom g, uint32_t *istart) {
    const int lane = threadIdx.x;
    uint32_t *I = istart + (size_t)blockIdx.x * (g.nint + 1);
    uint32_t carry = 0;
    for (int base = 0; base < g.nint; base += 64) {
        const int j = base + lane;
        const uint32_t v = j < g.nint ? I[j] : 0;
        const uint32_t incl = wave_scan_u32(v);
        if (j < g.nint) I[j] = incl - v + carry;
        carry += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
    if (lane == 0) I[g.nint] = carry;
}

// the part of every frame's bit buffer that will be written (whole chunks, and one more), zeroed: blocks OR their bits in
__global__ __launch_bounds__(PV_NT) void k_pv_zero(ck_pv_geom g, const uint32_t *istart, uint32_t *bitbuf) {
    const int i = blockIdx.y;
    const uint32_t total = istart[(size_t)i * (g.nint + 1) + g.nint];
    const uint32_t nq = min(((total + CK_PV_CHUNK - 1) / CK_PV_CHUNK + 1) * (CK_PV_CHUNK / 16), (uint32_t)g.bit_words / 4);
    uint4 *B = reinterpret_cast<uint4 *>(bitbuf + (size_t)i * g.bit_words);
    for (uint32_t q = blockIdx.x * PV_NT + threadIdx.x; q < nq; q += gridDim.x * PV_NT) B[q] = make_uint4(0, 0, 0, 0);
}

// MSB-first bit writer into 32-bit words that neighbouring blocks share: the first and the last word a block touches are OR-ed in,
// the words in between are its own
struct BitWriter {
    uint32_t *w;
    unsigned long long acc;
    int n;
    bool first;
    __device__ __forceinline__ void put(uint32_t code, int nbits) { // nbits <= 27
        acc = (acc << nbits) | code;
        n += nbits;
        if (n >= 32) {
            const uint32_t word = (uint32_t)(acc >> (n - 32));
            if (first) atomicOr(w, word); else *w = word;
            first = false;
            w++;
            n -= 32;
            acc &= (1ull << n) - 1;
        }
    }
    __device__ __forceinline__ void finish() {
        if (n > 0) atomicOr(w, (uint32_t)(acc << (32 - n)));
    }
};

// One block per lane: Huffman codes and value bits at the block's bit position; the last block of an interval pads the interval's
// last byte with 1-bits.
template <int NC>
__global__ __launch_bounds__(PV_NT) void k_pv_pack(ck_pv_geom g, int n, const int16_t *coef, const int16_t *dc, const uint32_t *len,
                                                   const uint32_t *istart, uint32_t *bitbuf) {
    __shared__ uint32_t enc_all[(NC == 3 ? 2 : 1) * PV_ENC_WORDS];
    load_enc<NC>(enc_all);
    const long t = (long)blockIdx.x * PV_NT + threadIdx.x;
    if (t >= (long)n * g.nblk) return;
    const int i = (int)(t / g.nblk), b = (int)(t - (long)i * g.nblk), j = b / g.R, b0 = j * g.R;
    const uint32_t *enc = enc_of<NC>(enc_all, b);
    const uint32_t pos = istart[(size_t)i * (g.nint + 1) + j] * 8u + len[t];
    BitWriter W = {bitbuf + (size_t)i * g.bit_words + (pos >> 5), 0ull, (int)(pos & 31), true};
    const uint4 *c4 = reinterpret_cast<const uint4 *>(coef + (size_t)t * 64);
    int run = 0;
    for (int q = 0; q < 8; q++) {
        const uint4 c = c4[q];
        const uint32_t cw[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
        for (int k = 0; k < 8; k++) {
            int v = (int)(int16_t)(cw[k >> 1] >> ((k & 1) * 16));
            const bool is_dc = q == 0 && k == 0;
            if (is_dc) v -= b - b0 < NC ? 0 : (int)dc[t - NC];
            else if (v == 0) { run++; continue; }
            for (; run > 15; run -= 16) W.put(enc[16 + 0xF0] & 0xFFFFu, (int)(enc[16 + 0xF0] >> 16));
            const int sz = category(v);
            const uint32_t e = is_dc ? enc[sz] : enc[16 + ((run << 4) | sz)];
            const uint32_t val = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << sz) - 1u);
            W.put(((e & 0xFFFFu) << sz) | val, (int)(e >> 16) + sz);
            run = 0;
        }
    }
    if (run) W.put(enc[16] & 0xFFFFu, (int)(enc[16] >> 16));
    if (b == min(g.nblk, b0 + g.R) - 1) {
        const int pad = (8 - (W.n & 7)) & 7;
        W.put((1u << pad) - 1u, pad);
    }
    W.finish();
}

// ---- byte stuffing -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t count_ff(uint32_t w) {
    return (uint32_t)((w >> 24) == 0xFFu) + (uint32_t)(((w >> 16) & 0xFFu) == 0xFFu) + (uint32_t)(((w >> 8) & 0xFFu) == 0xFFu) + (uint32_t)((w & 0xFFu) == 0xFFu);
}

// One workgroup per entry: the 0xFF bytes of every chunk of the bit buffer, their exclusive scan over the frame (wave DPP scan +
// one LDS exchange per 256 chunks), the file's size and status.  Bytes past the frame's last one were zeroed, so they count nothing.
__global__ __launch_bounds__(PV_NT) void k_pv_cscan(ck_pv_geom g, int n, int64_t cap, const uint32_t *istart, const uint32_t *bitbuf,
                                                    uint32_t *cpre, int64_t *sizes) {
    __shared__ uint32_t wsum[PV_NT / 64];
    const int i = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t total = istart[(size_t)i * (g.nint + 1) + g.nint];
    const uint32_t nch = (total + CK_PV_CHUNK - 1) / CK_PV_CHUNK;
    const uint4 *B = reinterpret_cast<const uint4 *>(bitbuf + (size_t)i * g.bit_words);
    uint32_t *C = cpre + (size_t)i * g.chunk_cap;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nch; base += PV_NT) {
        const uint32_t c = base + threadIdx.x;
        uint32_t v = 0;
        if (c < nch) {
#pragma unroll
            for (int q = 0; q < CK_PV_CHUNK / 16; q++) {
                const uint4 x = B[(size_t)c * (CK_PV_CHUNK / 16) + q];
                v += count_ff(x.x) + count_ff(x.y) + count_ff(x.z) + count_ff(x.w);
            }
        }
        const uint32_t incl = wave_scan_u32(v);
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < PV_NT / 64; k++) { before += k < wv ? wsum[k] : 0; all += wsum[k]; }
        if (c < nch) C[c] = carry + before + incl - v;
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int64_t size = (int64_t)g.hdr_len + total + carry + 2 * (g.nint - 1) + 2;
        sizes[i] = size;
        sizes[2 * (size_t)n + i] = size > cap ? CK_PREVIEW_TRUNCATED : CK_PREVIEW_OK;
    }
}

// One wave: where every file starts in the output: i * cap in a caller's device buffer, one after the other in the staging
__global__ __launch_bounds__(64) void k_pv_offsets(int n, int64_t cap, int compact, int64_t *sizes) {
    const int lane = threadIdx.x;
    unsigned long long carry = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const unsigned long long v = i < n ? (unsigned long long)min((long long)sizes[i], (long long)cap) : 0ull;
        const unsigned long long incl = wave_scan_u64(v);
        if (i < n) sizes[(size_t)n + i] = compact ? (int64_t)(carry + incl - v) : (int64_t)i * cap;
        carry += __shfl(incl, 63);
    }
}

// One chunk per lane and step: its bytes at their final places (header in front, a 0x00 behind every 0xFF, RSTm in front of
// every interval but the first), the header and EOI by the entry's first workgroup.  Nothing is written at or past `cap`.
__global__ __launch_bounds__(PV_NT) void k_pv_emit(ck_pv_geom g, ck_pv_tables tab, int n, int64_t cap, const uint32_t *istart,
                                                   const uint32_t *bitbuf, const uint32_t *cpre, const int64_t *sizes, uint8_t *out) {
    const int i = blockIdx.y;
    const uint32_t *I = istart + (size_t)i * (g.nint + 1);
    const uint32_t total = I[g.nint];
    const uint32_t nch = (total + CK_PV_CHUNK - 1) / CK_PV_CHUNK;
    const uint32_t *B = bitbuf + (size_t)i * g.bit_words;
    const uint32_t *C = cpre + (size_t)i * g.chunk_cap;
    uint8_t *O = out + sizes[(size_t)n + i];
    auto put = [&](int64_t at, uint32_t v) { if (at < cap) O[at] = (uint8_t)v; };
    if (blockIdx.x == 0) {
        for (int k = threadIdx.x; k < g.hdr_len; k += PV_NT) put(k, tab.hdr[k]);
        if (threadIdx.x == 0) { put(sizes[i] - 2, 0xFF); put(sizes[i] - 1, 0xD9); }
    }
    for (uint32_t c = blockIdx.x * PV_NT + threadIdx.x; c < nch; c += gridDim.x * PV_NT) {
        const uint32_t i0 = c * CK_PV_CHUNK, i1 = min(total, i0 + CK_PV_CHUNK);
        int lo = 0, hi = g.nint - 1; // the interval of the chunk's first byte: the last one that starts at or before it
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (I[mid] <= i0) lo = mid; else hi = mid - 1;
        }
        int j = lo;
        uint32_t next = I[j + 1];
        int64_t at = (int64_t)g.hdr_len + i0 + C[c] + 2 * (int64_t)j;
        if (i0 == I[j] && j > 0) { put(at - 2, 0xFF); put(at - 1, 0xD0 + ((j - 1) & 7)); }
        for (uint32_t k = i0; k < i1; k++) {
            if (k == next) { // (an interval holds at least one byte, so at most one starts here)
                j++;
                next = I[j + 1];
                put(at, 0xFF); put(at + 1, 0xD0 + ((j - 1) & 7));
                at += 2;
            }
            const uint32_t v = (B[k >> 2] >> (24 - 8 * (k & 3))) & 0xFFu;
            put(at++, v);
            if (v == 0xFFu) put(at++, 0);
        }
    }
}

unsigned blocks_for(long items) { return (unsigned)((items + PV_NT - 1) / PV_NT); }

} // namespace

int ck_launch_preview_mask(ck_handle *h, const ck_pv_geom &g, int n) {
    ck_preview_ws &P = *h->preview;
    if (!g.overlay) return CK_OK;
    CK_HIP(hipMemsetAsync(P.d_mask, 0, sizeof(uint32_t) * (size_t)g.mask_words * n, h->stream));
    hipLaunchKernelGGL(k_pv_mask, dim3(blocks_for((long)n * h->ws.det_cap * 4)), dim3(PV_NT), 0, h->stream, g, n, h->ws.det_cap,
                       P.d_frames, h->ws.d_dets, h->ws.d_counters, P.d_mask);
    CK_HIP(hipGetLastError());
    return CK_OK;
}

int ck_launch_preview_luma(ck_handle *h, const ck_pv_geom &g, int n, uint8_t *d_out) {
    ck_preview_ws &P = *h->preview;
    hipLaunchKernelGGL(k_pv_luma, dim3(blocks_for((long)n * g.pw * g.ph)), dim3(PV_NT), 0, h->stream, g, n, ck_staged_image(h),
                       P.d_frames, P.d_mask, d_out);
    CK_HIP(hipGetLastError());
    return CK_OK;
}

int ck_launch_preview_color(ck_handle *h, const ck_pv_geom &g, const ck_pv_src &src, int n, uint8_t *d_out) {
    ck_preview_ws &P = *h->preview;
    const dim3 grid(blocks_for((long)n * g.pw * g.ph * 3));
    if (src.jpeg) hipLaunchKernelGGL(k_pv_jtriples, grid, dim3(PV_NT), 0, h->stream, g, *src.jpeg, n, P.d_frames, P.d_mask, d_out);
    else if (src.planar) hipLaunchKernelGGL(k_pv_ptriples, grid, dim3(PV_NT), 0, h->stream, g, *src.planar, n, P.d_frames, P.d_mask, d_out);
    else if (src.raw->bpp == 2) hipLaunchKernelGGL(k_pv_color<true>, grid, dim3(PV_NT), 0, h->stream, g, *src.raw, n, P.d_frames, P.d_mask, d_out);
    else hipLaunchKernelGGL(k_pv_color<false>, grid, dim3(PV_NT), 0, h->stream, g, *src.raw, n, P.d_frames, P.d_mask, d_out);
    CK_HIP(hipGetLastError());
    return CK_OK;
}

namespace {

// front end (the staged luma, or the raw frames `cs` of a colour call) .. stuffing scan
template <int NC>
void launch_first_half(ck_handle *h, const ck_pv_geom &g, const ck_pv_tables &t, const ck_pv_src *cs, int n, int64_t cap, bool compact) {
    ck_preview_ws &P = *h->preview;
    hipStream_t st = h->stream;
    const unsigned nb = blocks_for((long)n * g.nblk);
    if constexpr (NC == 1) hipLaunchKernelGGL(k_pv_fdct, dim3(nb), dim3(PV_NT), 0, st, g, t, n, ck_staged_image(h), P.d_frames, P.d_mask, P.d_coef, P.d_dc, P.d_len);
    else if (cs->jpeg) hipLaunchKernelGGL(k_pv_jfdct, dim3(nb), dim3(PV_NT), 0, st, g, t, *cs->jpeg, n, P.d_frames, P.d_mask, P.d_coef, P.d_dc, P.d_len);
    else if (cs->planar) hipLaunchKernelGGL(k_pv_pfdct, dim3(nb), dim3(PV_NT), 0, st, g, t, *cs->planar, n, P.d_frames, P.d_mask, P.d_coef, P.d_dc, P.d_len);
    else if (cs->raw->bpp == 2) hipLaunchKernelGGL(k_pv_fdct_color<true>, dim3(nb), dim3(PV_NT), 0, st, g, t, *cs->raw, n, P.d_frames, P.d_mask, P.d_coef, P.d_dc, P.d_len);
    else hipLaunchKernelGGL(k_pv_fdct_color<false>, dim3(nb), dim3(PV_NT), 0, st, g, t, *cs->raw, n, P.d_frames, P.d_mask, P.d_coef, P.d_dc, P.d_len);
    hipLaunchKernelGGL(k_pv_scan<NC>, dim3((unsigned)(((long)n * g.nint + PV_NT / 64 - 1) / (PV_NT / 64))), dim3(PV_NT), 0, st, g, n, P.d_dc, P.d_len, P.d_istart);
    hipLaunchKernelGGL(k_pv_iscan, dim3((unsigned)n), dim3(64), 0, st, g, P.d_istart);
    const unsigned gz = (unsigned)min(64, (g.bit_words / 4 + PV_NT - 1) / PV_NT);
    hipLaunchKernelGGL(k_pv_zero, dim3(gz, (unsigned)n), dim3(PV_NT), 0, st, g, P.d_istart, P.d_bits);
    hipLaunchKernelGGL(k_pv_pack<NC>, dim3(nb), dim3(PV_NT), 0, st, g, n, P.d_coef, P.d_dc, P.d_len, P.d_istart, P.d_bits);
    hipLaunchKernelGGL(k_pv_cscan, dim3((unsigned)n), dim3(PV_NT), 0, st, g, n, cap, P.d_istart, P.d_bits, P.d_cpre, P.d_sizes);
    hipLaunchKernelGGL(k_pv_offsets, dim3(1), dim3(64), 0, st, n, cap, compact ? 1 : 0, P.d_sizes);
}

} // namespace

// scale .. stuffing scan: after it d_sizes holds every file's size, offset in the output and status
int ck_launch_preview_encode(ck_handle *h, const ck_pv_geom &g, const ck_pv_tables &t, const ck_pv_src *cs, int n, uint8_t *d_out,
                             int64_t cap, bool compact) {
    ck_preview_ws &P = *h->preview;
    if (!d_out) {
        if (cs) launch_first_half<3>(h, g, t, cs, n, cap, compact);
        else launch_first_half<1>(h, g, t, nullptr, n, cap, compact);
    } else {
        const unsigned ge = (unsigned)min(64, (g.chunk_cap + PV_NT - 1) / PV_NT);
        hipLaunchKernelGGL(k_pv_emit, dim3(ge, (unsigned)n), dim3(PV_NT), 0, h->stream, g, t, n, cap, P.d_istart, P.d_bits, P.d_cpre, P.d_sizes, d_out);
    }
    CK_HIP(hipGetLastError());
    return CK_OK;
}
