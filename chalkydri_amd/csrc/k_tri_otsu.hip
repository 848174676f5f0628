// k_tri_otsu.hip — iterative tri-class Otsu threshold of n dense frames: three kernels on one stream.
//
//   k_tri_hist      a streaming pass: every lane takes pieces of 16 pixels (16 * channels bytes, read as `channels` 16-byte loads; a
//                   frame is dense, so a piece may straddle rows), makes their CAT gray levels and adds them into its wave's own
//                   256-bin LDS histogram.  Inside a piece a run of equal levels is one add of the run's length, so a flat frame
//                   costs one LDS atomic per piece and wave instead of sixteen on one bin.  The workgroup folds its four
//                   sub-histograms and adds the occupied bins into the frame's 256 global counters.
//   k_tri_solve     one wave per frame, four bins per lane: the rounds of the contract in a uniform loop.  Prefix sums of n and s by
//                   the DPP wave scans of ck_internal.h, v(t) per lane in the fixed order (two fp64 multiplications, one division,
//                   no contraction), arg-max by a butterfly with "greater v, then smaller t".  ceil / floor of the class means are
//                   counted with the contract's own int64 comparisons (g n < s, g (N - n) <= S - s), so there is no 64-bit
//                   division.  Writes the table, the record and the class counts (from the histogram and the table).
//   k_tri_classify  the second streaming pass: gray level, then the frame's 256-byte table from LDS; 16 class bytes per lane in one
//                   16-byte store.
// The loads and stores carry no alignment assumption (k_rawfmt.hip's align-1 copies), so an odd frame size or base pointer costs
// cache-line straddles, not another path.  Only the ragged end of a frame — fewer than 16 pixels left — goes pixel by pixel: no
// lane reads or writes past the last pixel of its frame.
#include "ck_tri_otsu.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr int NT = 256, WAVES = NT / 64;

__device__ __forceinline__ u32x4 ld16(const uint8_t *p) {
    u32x4 v;
    __builtin_memcpy(&v, p, 16); // align 1: one global_load_dwordx4
    return v;
}
__device__ __forceinline__ void st16(uint8_t *p, const u32x4 v) { __builtin_memcpy(p, &v, 16); }

template <int N>
__device__ __forceinline__ uint32_t byte_of(const uint32_t (&d)[N], int i) { return (d[i >> 2] >> (8 * (i & 3))) & 0xFFu; }

template <int CH>
__device__ __forceinline__ uint32_t gray1(const uint8_t *p) {
    return CH == 1 ? ck_cat_grayscale(p[0], p[0], p[0]) : ck_cat_grayscale(p[0], p[1], p[2]);
}
// gray levels of the 16 pixels that start at p, pixel j in byte j of g
template <int CH>
__device__ __forceinline__ void gray16(const uint8_t *p, uint32_t (&g)[4]) {
    uint32_t d[4 * CH];
#pragma unroll
    for (int c = 0; c < CH; c++) {
        const u32x4 v = ld16(p + 16 * c);
        d[4 * c] = v.x; d[4 * c + 1] = v.y; d[4 * c + 2] = v.z; d[4 * c + 3] = v.w;
    }
    g[0] = g[1] = g[2] = g[3] = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const uint32_t r = byte_of(d, CH * j);
        const uint32_t v = CH == 1 ? ck_cat_grayscale(r, r, r) : ck_cat_grayscale(r, byte_of(d, CH * j + (CH - 1) / 2), byte_of(d, CH * j + CH - 1));
        g[j >> 2] |= v << (8 * (j & 3));
    }
}

// blockIdx.x = frame * bx + b: workgroup b of the frame's bx walks the pieces b * NT + tid, + bx * NT, ...
template <int CH>
__global__ __launch_bounds__(NT) void k_tri_hist(const uint8_t *__restrict__ px, const size_t npix, const unsigned bx, uint32_t *__restrict__ hist) {
    __shared__ uint32_t sub[WAVES][256];
    const unsigned f = blockIdx.x / bx, b = blockIdx.x - f * bx;
    const int tid = (int)threadIdx.x;
#pragma unroll
    for (int w = 0; w < WAVES; w++) sub[w][tid] = 0; // (NT == 256 bins)
    __syncthreads();
    uint32_t *my = sub[tid >> 6];
    const uint8_t *base = px + (size_t)f * npix * CH;
    const size_t pieces = (npix + 15) / 16;
    for (size_t i = (size_t)b * NT + tid; i < pieces; i += (size_t)bx * NT) {
        const size_t x0 = i * 16;
        if (x0 + 16 <= npix) {
            uint32_t g[4];
            gray16<CH>(base + x0 * CH, g);
            uint32_t prev = g[0] & 0xFFu, run = 1;
#pragma unroll
            for (int j = 1; j < 16; j++) {
                const uint32_t cur = byte_of(g, j);
                if (cur == prev) run++;
                else { atomicAdd(&my[prev], run); prev = cur; run = 1; }
            }
            atomicAdd(&my[prev], run);
        } else { // the ragged end of the frame: the pixels that exist
            for (size_t x = x0; x < npix; x++) atomicAdd(&my[gray1<CH>(base + x * CH)], 1u);
        }
    }
    __syncthreads();
    uint32_t t = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) t += sub[w][tid];
    if (t) atomicAdd(&hist[(size_t)f * 256 + tid], t);
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t x) { return (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_u32(x), 63); }
__device__ __forceinline__ long long last_lane_i64(unsigned long long x) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, 63), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), 63);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// one wave per frame; lane l owns the levels 4 l .. 4 l + 3
__global__ __launch_bounds__(64) void k_tri_solve(const uint32_t *__restrict__ hist, const ck_tri_otsu_params_t p, uint8_t *__restrict__ lut,
                                                  ck_tri_otsu_info_t *__restrict__ info) {
    const int lane = (int)threadIdx.x, g0 = 4 * lane;
    const size_t f = blockIdx.x;
    const u32x4 hv = reinterpret_cast<const u32x4 *>(hist + f * 256)[lane];
    const uint32_t c[4] = {hv.x, hv.y, hv.z, hv.w};
    int lo = 0, hi = 255, T_last = -1, rounds = 0, myT = -1;
    for (int k = 1;; k++) {
        uint32_t m[4], occupied = 0;
        unsigned long long n4 = 0, s4 = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int g = g0 + j;
            m[j] = (g >= lo && g <= hi) ? c[j] : 0u;
            n4 += m[j]; s4 += (unsigned long long)g * m[j];
            occupied += m[j] != 0u;
        }
        if (wave_sum_u32(occupied) < 2u) break; // no threshold from this round
        const unsigned long long ni = wave_scan_u64(n4), si = wave_scan_u64(s4);
        const long long N = last_lane_i64(ni), S = last_lane_i64(si);
        long long n = (long long)(ni - n4), s = (long long)(si - s4);
        // the lane's best t: levels below lo have n = 0 and levels from hi on have N - n = 0, so only lo .. hi-1 can qualify
        double best = -1.0;
        int bt = 256;
        long long bn = 0, bs = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            n += m[j]; s += (long long)(g0 + j) * m[j];
            if (n > 0 && N - n > 0) {
                const double d = (double)(long long)((unsigned long long)S * (unsigned long long)n - (unsigned long long)N * (unsigned long long)s);
                const double v = (d * d) / ((double)n * (double)(N - n));
                if (v > best) { best = v; bt = g0 + j; bn = n; bs = s; }
            }
        }
        double wv = best;
        int wt = bt;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { // greater v wins, then the smaller t: a total order, every lane ends with the winner
            const double ov = __shfl_xor(wv, off);
            const int ot = __shfl_xor(wt, off);
            if (ov > wv || (ov == wv && ot < wt)) { wv = ov; wt = ot; }
        }
        const int T = __builtin_amdgcn_readfirstlane(wt);
        const long long n_T = __shfl(bn, T >> 2), s_T = __shfl(bs, T >> 2); // (the winner is its lane's best)
        // lo' = ceil(s / n) = levels with g n < s;  hi' = floor((S - s) / (N - n)) = levels with g (N - n) <= S - s, less one
        uint32_t below = 0, upto = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            below += (long long)(g0 + j) * n_T < s_T;
            upto += (long long)(g0 + j) * (N - n_T) <= S - s_T;
        }
        const int lo2 = (int)wave_sum_u32(below), hi2 = (int)wave_sum_u32(upto) - 1;
        const int delta = T > T_last ? T - T_last : T_last - T;
        const bool repeat = k >= 2 && delta < p.min_delta;
        if (lane == k - 1) myT = T;
        T_last = T; rounds = k;
        if (repeat || k == p.max_iters) { lo = lo2; hi = hi2; break; }
        if (lo2 > hi2) break;
        lo = lo2; hi = hi2;
    }
    uint32_t word = 0, cnt[3] = {0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int g = g0 + j;
        uint32_t cls;
        if (rounds == 0) cls = g < 128 ? 0u : 1u;
        else if (g < lo) cls = 0u;
        else if (g > hi) cls = 1u;
        else cls = p.keep_tbd ? 2u : (g <= T_last ? 0u : 1u);
        word |= cls << (8 * j);
        cnt[0] += cls == 0u ? c[j] : 0u; cnt[1] += cls == 1u ? c[j] : 0u; cnt[2] += cls == 2u ? c[j] : 0u;
    }
    reinterpret_cast<uint32_t *>(lut + f * 256)[lane] = word;
    const uint32_t nb = wave_sum_u32(cnt[0]), nw = wave_sum_u32(cnt[1]), no = wave_sum_u32(cnt[2]);
    ck_tri_otsu_info_t *I = info + f;
    if (lane < CK_TRI_MAX_ROUNDS) I->T[lane] = myT;
    if (lane == 0) {
        I->n_rounds = rounds; I->T_last = T_last;
        I->lo_final = lo; I->hi_final = hi;
        I->n_black = nb; I->n_white = nw; I->n_other = no;
        I->flags = rounds == 0 ? (uint32_t)CK_TRI_FLAT : 0u;
    }
}

template <int CH>
__global__ __launch_bounds__(NT) void k_tri_classify(const uint8_t *__restrict__ px, const size_t npix, const unsigned bx,
                                                     const uint8_t *__restrict__ lut, uint8_t *__restrict__ classes) {
    __shared__ __attribute__((aligned(4))) uint8_t tab[256];
    const unsigned f = blockIdx.x / bx, b = blockIdx.x - f * bx;
    const int tid = (int)threadIdx.x;
    if (tid < 64) reinterpret_cast<uint32_t *>(tab)[tid] = reinterpret_cast<const uint32_t *>(lut + (size_t)f * 256)[tid];
    __syncthreads();
    const uint8_t *base = px + (size_t)f * npix * CH;
    uint8_t *out = classes + (size_t)f * npix;
    const size_t pieces = (npix + 15) / 16;
    for (size_t i = (size_t)b * NT + tid; i < pieces; i += (size_t)bx * NT) {
        const size_t x0 = i * 16;
        if (x0 + 16 <= npix) {
            uint32_t g[4], o[4] = {0, 0, 0, 0};
            gray16<CH>(base + x0 * CH, g);
#pragma unroll
            for (int j = 0; j < 16; j++) o[j >> 2] |= (uint32_t)tab[byte_of(g, j)] << (8 * (j & 3));
            st16(out + x0, u32x4{o[0], o[1], o[2], o[3]});
        } else {
            for (size_t x = x0; x < npix; x++) out[x] = tab[gray1<CH>(base + x * CH)];
        }
    }
}

// workgroups per frame: enough of them over the whole call to fill the chip, never more than the frame has blocks of pieces
unsigned groups_per_frame(size_t npix, int n, unsigned want_total) {
    const size_t blocks = ((npix + 15) / 16 + NT - 1) / NT;
    const size_t share = (want_total + (unsigned)n - 1) / (unsigned)n;
    return (unsigned)(blocks < share ? blocks : share);
}

template <int CH>
int launch(hipStream_t st, const ck_tri_otsu_params_t &p, const uint8_t *d_px, int n, size_t npix, uint8_t *d_classes, uint32_t *d_hist,
           uint8_t *d_lut, ck_tri_otsu_info_t *d_info) {
    // the histogram pass pays a fold and up to 256 global adds per workgroup, so it takes fewer, longer workgroups than the look-up
    const unsigned bh = groups_per_frame(npix, n, 2048), bc = groups_per_frame(npix, n, 16384);
    if ((size_t)bc * (size_t)n > 0x7FFFFFFFu) return CK_EINVAL;
    CK_HIP(hipMemsetAsync(d_hist, 0, sizeof(uint32_t) * 256 * (size_t)n, st));
    hipLaunchKernelGGL((k_tri_hist<CH>), dim3(bh * (unsigned)n), dim3(NT), 0, st, d_px, npix, bh, d_hist);
    hipLaunchKernelGGL(k_tri_solve, dim3((unsigned)n), dim3(64), 0, st, d_hist, p, d_lut, d_info);
    hipLaunchKernelGGL((k_tri_classify<CH>), dim3(bc * (unsigned)n), dim3(NT), 0, st, d_px, npix, bc, d_lut, d_classes);
    CK_HIP(hipGetLastError());
    return CK_OK;
}

} // namespace

int ck_launch_tri_otsu(hipStream_t stream, const ck_tri_otsu_params_t &p, const uint8_t *d_px, int n, size_t npix, uint8_t *d_classes,
                       uint32_t *d_hist, uint8_t *d_lut, ck_tri_otsu_info_t *d_info) {
    if (n <= 0) return CK_OK;
    return p.channels == 1 ? launch<1>(stream, p, d_px, n, npix, d_classes, d_hist, d_lut, d_info)
                           : launch<3>(stream, p, d_px, n, npix, d_classes, d_hist, d_lut, d_info);
}
