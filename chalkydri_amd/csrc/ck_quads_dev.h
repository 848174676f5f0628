// ck_quads_dev.h — device helpers of the quad fit that k_quads.hip (k_fit, k_seq, k_tail) and k_chunk.hip (k_chunk) share: the moment
// sums of a point, their conversion to doubles, the smoothing kernel, the barrier and the wait that order LDS traffic and prefetches.
#ifndef CK_QUADS_DEV_H
#define CK_QUADS_DEV_H
#include "ck_internal.h"

namespace {

struct M6 { long long Mx, My, Mxx, Mxy, Myy, W; };
__device__ __forceinline__ M6 m6_add(M6 a, M6 b) { a.Mx += b.Mx; a.My += b.My; a.Mxx += b.Mxx; a.Mxy += b.Mxy; a.Myy += b.Myy; a.W += b.W; return a; }
__device__ __forceinline__ M6 m6_sub(M6 a, M6 b) { a.Mx -= b.Mx; a.My -= b.My; a.Mxx -= b.Mxx; a.Mxy -= b.Mxy; a.Myy -= b.Myy; a.W -= b.W; return a; }
__device__ __forceinline__ M6 m6_zero() { M6 z = {0, 0, 0, 0, 0, 0}; return z; }

__device__ __forceinline__ M6 moments_of(uint32_t xy, uint32_t Wt) {
    // W <= 362, X, Y <= 8192: the first-order products fit 32 bits, the second-order ones are one 32x32->64 multiply each
    const uint32_t X = (xy >> 13) + 1, Y = (xy & 0x1FFF) + 1;
    const uint32_t wx = Wt * X, wy = Wt * Y;
    M6 m;
    m.Mx = (long long)wx; m.My = (long long)wy;
    m.Mxx = (long long)((unsigned long long)wx * X); m.Mxy = (long long)((unsigned long long)wx * Y); m.Myy = (long long)((unsigned long long)wy * Y);
    m.W = (long long)Wt;
    return m;
}

// an integer below 2^52 as a double: its bits under the exponent of 2^52, less 2^52 (exact; the generic 64-bit conversion is two
// conversions and a scaling).  The moment sums of a window or a cluster side are such integers (<= 49 140 points x 362 x 8192^2 < 2^51).
__device__ __forceinline__ double f64_of_u52(unsigned long long x) {
    return __longlong_as_double((long long)(0x4330000000000000ull | x)) - 4503599627370496.0;
}

__device__ const double k_smooth[7] = {0.011108996538242306, 0.1353352832366127, 0.6065306597126334, 1.0,
                                       0.6065306597126334, 0.1353352832366127, 0.011108996538242306};

// s_waitcnt vmcnt(0) as an instruction the compiler's own wait insertion knows about (gfx9 encoding: vmcnt in bits 3:0 and 15:14,
// expcnt 6:4 and lgkmcnt 11:8 left at "do not wait"): placed BEFORE a prefetch is issued, so that what the iteration is about to use
// is known to be there and the compiler's later waits (which, inside loops, are for everything outstanding) find nothing to sit on
constexpr int WAIT_VMCNT0 = 0x0F70;
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__GFX9__)
#error "WAIT_VMCNT0 is the gfx9-family encoding of s_waitcnt (this library is written for gfx950): another target needs its own"
#endif
// Barriers that order LDS traffic only.  __syncthreads() carries a workgroup-scope fence, which the compiler turns into a wait for
// EVERY outstanding memory operation — a prefetch issued for the next cluster would be waited for at the first barrier behind it.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

} // namespace

#endif
