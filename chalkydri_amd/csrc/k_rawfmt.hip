// k_rawfmt.hip — raw camera formats to luma, turned by the camera's mounting, into the staged frames.
//
// A streaming kernel: every lane makes 16 luma bytes from 16 source pixels (16 * bpp bytes, read as bpp 16-byte loads along the
// source row) and every staged byte leaves in a 16-byte store along an output row.
//   k_raw_straight  none / rotate-180: lane = one 16-byte piece of an output row.  Rotate-180 reads the mirrored 16 pixels of the
//                   mirrored row and reverses the 16 bytes in registers (4:2:2: the reversed v_perm_b32 selector does it).
//   k_raw_quarter   the quarter turns: a workgroup owns 64 source columns x 64 output columns (= source rows).  Lanes read along
//                   source rows, scatter their 16 luma bytes into a 64 x 64 LDS tile transposed, and after the barrier read the
//                   tile along its rows as 16-byte pieces of output rows.  The tile is XOR-swizzled by 16-byte piece instead of
//                   padded (a padded pitch would take the 16-byte alignment from the ds_read_b128): piece p of tile row c lives at
//                   p ^ (c >> 4), so the four column groups of a wave's byte stores fall on four different bank quads and the
//                   wide reads stay one contiguous KiB per wave.
// The loads carry no alignment assumption (global memory takes unaligned dwordx4 on gfx9+; the compiler emits them for the
// align-1 copy below), so an odd base pointer or stride costs cache-line straddles, not another path.  Only the ragged end of a
// row — fewer than 16 pixels left — goes pixel by pixel, and that path reads exactly the bytes of the pixels that exist: no lane
// reads outside [row, row + bpp * sw) of a source row.
#include "ck_internal.h"
#include "ck_rawfmt.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct raw_args {
    const uint8_t *src; int sstride; size_t spitch; int sw, sh;
    uint8_t *dst; int dstride; size_t dpitch; int W, H; // the oriented frame
    uint32_t k0, k1, k2;                                 // ck_raw_class::k
};

__device__ __forceinline__ u32x4 ld16(const uint8_t *p) {
    u32x4 v;
    __builtin_memcpy(&v, p, 16); // align 1: one global_load_dwordx4
    return v;
}

__device__ __forceinline__ uint32_t luma_rgb(uint32_t b0, uint32_t b1, uint32_t b2, const raw_args &a) {
    return (__umul24(b0, a.k0) + __umul24(b1, a.k1) + __umul24(b2, a.k2) + 32768u) >> 16;
}

// luma of the one pixel at p
template <int BPP>
__device__ __forceinline__ uint32_t luma1(const uint8_t *p, const raw_args &a) {
    if (BPP == 1) return p[0];
    if (BPP == 2) return p[a.k2];
    return luma_rgb(p[0], p[1], p[2], a);
}

// byte `i` of the 12 / 16 dwords d[] of 16 packed pixels
template <int N>
__device__ __forceinline__ uint32_t byte_of(const uint32_t (&d)[N], int i) { return (d[i >> 2] >> (8 * (i & 3))) & 0xFFu; }

// luma of the 16 pixels that start at p, pixel j in byte j of the result.  REV (bpp 2 only): pixel j in byte 15 - j.
template <int BPP, bool REV>
__device__ __forceinline__ u32x4 luma16(const uint8_t *p, const raw_args &a) {
    if (BPP == 1) return ld16(p);
    if (BPP == 2) {
        const u32x4 lo = ld16(p), hi = ld16(p + 16);
        const uint32_t sel = REV ? a.k1 : a.k0;
        const uint32_t q0 = __builtin_amdgcn_perm(lo.y, lo.x, sel), q1 = __builtin_amdgcn_perm(lo.w, lo.z, sel);
        const uint32_t q2 = __builtin_amdgcn_perm(hi.y, hi.x, sel), q3 = __builtin_amdgcn_perm(hi.w, hi.z, sel);
        return REV ? u32x4{q3, q2, q1, q0} : u32x4{q0, q1, q2, q3};
    }
    uint32_t d[4 * BPP];
#pragma unroll
    for (int c = 0; c < BPP; c++) {
        const u32x4 v = ld16(p + 16 * c);
        d[4 * c] = v.x; d[4 * c + 1] = v.y; d[4 * c + 2] = v.z; d[4 * c + 3] = v.w;
    }
    uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; j++)
        o[j >> 2] |= luma_rgb(byte_of(d, BPP * j), byte_of(d, BPP * j + 1), byte_of(d, BPP * j + 2), a) << (8 * (j & 3));
    return u32x4{o[0], o[1], o[2], o[3]};
}

__device__ __forceinline__ u32x4 reverse16(const u32x4 v) {
    return u32x4{__builtin_bswap32(v.w), __builtin_bswap32(v.z), __builtin_bswap32(v.y), __builtin_bswap32(v.x)};
}

// none (FLIP = false): out[y][x] = S[y][x];  rotate-180: out[y][x] = S[sh-1-y][sw-1-x]
template <int BPP, bool FLIP>
__global__ __launch_bounds__(256) void k_raw_straight(const raw_args a, const int pieces) {
    const int idx = (int)(blockIdx.x * 256u + threadIdx.x);
    const int y = idx / pieces, x0 = 16 * (idx - y * pieces);
    if (y >= a.H) return;
    const uint8_t *row = a.src + (size_t)blockIdx.y * a.spitch + (size_t)(FLIP ? a.sh - 1 - y : y) * a.sstride;
    u32x4 o;
    if (x0 + 16 <= a.W) {
        const uint8_t *p = row + (size_t)(FLIP ? a.sw - 16 - x0 : x0) * BPP;
        if (BPP == 2) o = luma16<2, FLIP>(p, a);
        else { o = luma16<BPP, false>(p, a); if (FLIP) o = reverse16(o); }
    } else { // the ragged end of the row: the pixels that exist, zeros behind them
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 16; k++)
            if (x0 + k < a.W) w[k >> 2] |= luma1<BPP>(row + (size_t)(FLIP ? a.sw - 1 - x0 - k : x0 + k) * BPP, a) << (8 * (k & 3));
        o = u32x4{w[0], w[1], w[2], w[3]};
    }
    *reinterpret_cast<u32x4 *>(a.dst + (size_t)blockIdx.y * a.dpitch + (size_t)y * a.dstride + x0) = o;
}

// clockwise (CW): out[y][x] = S[sh-1-x][y];  counterclockwise: out[y][x] = S[x][sw-1-y].  W = sh, H = sw.
// Tile: output columns X0 .. X0+63 (i) x source columns C0 .. C0+63 (c); LDS byte (c, i) at c * 64 + (i ^ (c >> 4) * 16).
template <int BPP, bool CW>
__global__ __launch_bounds__(256) void k_raw_quarter(const raw_args a) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[64 * 64];
    const int X0 = (int)blockIdx.x * 64, C0 = (int)blockIdx.y * 64, tid = (int)threadIdx.x;
    {
        const int i = tid >> 2, cc = tid & 3, x = X0 + i, col = C0 + 16 * cc;
        if (x < a.W && col < a.sw) {
            const uint8_t *p = a.src + (size_t)blockIdx.z * a.spitch + (size_t)(CW ? a.sh - 1 - x : x) * a.sstride + (size_t)col * BPP;
            uint32_t w[4] = {0, 0, 0, 0};
            if (col + 16 <= a.sw) {
                const u32x4 v = luma16<BPP, false>(p, a);
                w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
            } else {
#pragma unroll
                for (int k = 0; k < 16; k++)
                    if (col + k < a.sw) w[k >> 2] |= luma1<BPP>(p + k * BPP, a) << (8 * (k & 3));
            }
            uint8_t *t = tile + (16 * cc) * 64 + (i ^ (cc << 4));
#pragma unroll
            for (int k = 0; k < 16; k++) t[k * 64] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
        }
    }
    __syncthreads();
    {
        const int c = tid >> 2, j = tid & 3, col = C0 + c, x = X0 + 16 * j;
        if (col < a.sw && x < a.W) { // (x + 15 may pass W: those bytes land in the staged row's padding)
            const u32x4 v = *reinterpret_cast<const u32x4 *>(tile + c * 64 + ((j ^ (c >> 4)) << 4));
            const int y = CW ? col : a.sw - 1 - col;
            *reinterpret_cast<u32x4 *>(a.dst + (size_t)blockIdx.z * a.dpitch + (size_t)y * a.dstride + x) = v;
        }
    }
}

template <int BPP>
int launch(hipStream_t st, const raw_args &a, int orientation, int n) {
    if (orientation == CK_ORIENT_NONE || orientation == CK_ORIENT_ROTATE_180) {
        const int pieces = a.dstride / 16;
        const dim3 grid((unsigned)(((size_t)pieces * a.H + 255) / 256), (unsigned)n);
        if (orientation == CK_ORIENT_NONE) hipLaunchKernelGGL((k_raw_straight<BPP, false>), grid, dim3(256), 0, st, a, pieces);
        else hipLaunchKernelGGL((k_raw_straight<BPP, true>), grid, dim3(256), 0, st, a, pieces);
    } else {
        const dim3 grid((unsigned)((a.W + 63) / 64), (unsigned)((a.sw + 63) / 64), (unsigned)n);
        if (orientation == CK_ORIENT_CLOCKWISE) hipLaunchKernelGGL((k_raw_quarter<BPP, true>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_raw_quarter<BPP, false>), grid, dim3(256), 0, st, a);
    }
    CK_HIP(hipGetLastError());
    return CK_OK;
}

} // namespace

int ck_launch_rawfmt(ck_handle *h, hipStream_t st, const ck_raw_src &src, const ck_raw_class &cls, int orientation, uint8_t *dst, int n) {
    if (n <= 0) return CK_OK;
    int sw, sh;
    ck_source_size(h->w, h->h, orientation, &sw, &sh);
    if (src.sw != sw || src.sh != sh || n > 65535) return CK_EINVAL;
    const raw_args a = {src.p, src.stride, src.pitch, src.sw, src.sh, dst, h->frame_stride, h->frame_pitch, h->w, h->h, cls.k[0], cls.k[1], cls.k[2]};
    switch (cls.bpp) {
    case 1: return launch<1>(st, a, orientation, n);
    case 2: return launch<2>(st, a, orientation, n);
    case 3: return launch<3>(st, a, orientation, n);
    case 4: return launch<4>(st, a, orientation, n);
    }
    return CK_EINVAL;
}
