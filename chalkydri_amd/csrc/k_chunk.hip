// k_chunk.hip — the split quad fit's middle kernel (k_quads.hip has the fit's other kernels and its launch plan), in a unit of its
// own because it is the one place where the diagnostics library's device code differs from the product's (ck_knobs.h): there k_chunk
// takes a stop_after argument (CK_CHUNK_STOP_AFTER) and k_ext_base exists (CK_EXT_BASE).  Compiled twice, plain and with -DCK_DIAG;
// every other kernel of the diagnostics library is the product's own object file.
#include "ck_quads_dev.h"

namespace {

// Reciprocals of the window weights of k_chunk: a window holds at most 2 * 20 + 1 points of weight <= 362, so its weight sum is an
// integer below INV_N and 1.0 / W a table entry — the IEEE quotient, formed by the compiler: the same bits as the device's division
// (a dozen instructions around v_rcp_f64, 70 clocks of a SIMD per position by tools/probes/valu_rate_probe.hip) for one 8-byte load
// from a 116 KB table that lives in L2.  A position nobody wrote has a weight like any other (k_chunk gathers it from the weight image
// at whatever coordinates the position holds, or takes 1), so no window leaves the table; k_chunk clamps the index all the same.
constexpr int INV_N = 41 * 362 + 1;
struct InvTable {
    double v[INV_N];
    constexpr InvTable() : v() {
        v[0] = __builtin_huge_val(); // 1.0 / 0.0
        for (int n = 1; n < INV_N; n++) v[n] = 1.0 / (double)n;
    }
};
__device__ const InvTable g_inv_table{};

// ---- windowed line-fit error, smoothing and maxima of EVERY position of a frame's extended sequences --------
// One workgroup decides CK_SPAN = 960 consecutive positions (15 words of 64) from 1024 loaded ones; it knows nothing about clusters:
// a cluster's extended sequence carries its own neighbours (ck_internal.h), the window half-width travels in the point word, and
// what it finds is filed by POSITION — a bit per position, the smoothed errors of a span's maxima side by side in position
// order, the span's running moment sums at the end of every aligned block of 32 positions — so k_tail picks its cluster's share with a
// few popcounts and a target's prefix sum with one entry per span.  Positions
// nobody wrote (rejected clusters, the room duplicates left) compute garbage that nobody reads.  All sums are exact integers,
// the doubles are formed by the operations of k_fit's chunk loop in the same order: the same bits.
constexpr int KL = 1024, KOFF = 32;
static_assert(CK_SPAN == 960 && KOFF >= CK_EXT_PRE + 3 && KL - KOFF - CK_SPAN >= CK_EXT_POST + 4, "span geometry");
// (diagnostics, CK_CHUNK_STOP_AFTER: every span ends after step k, the next span's points and weights in hand as ever; the product
// kernel passes the constant 99 and holds none of it)
__device__ __forceinline__ void k_chunk_body(const ck_stage_ws &ws, int qw, int qh, const int stop_after) {
    __shared__ __attribute__((aligned(16))) unsigned long long sP64[3][KL]; // inclusive sums from the first loaded position: Mxx, Mxy, Myy
    __shared__ __attribute__((aligned(16))) uint32_t sP32[3][KL];           // Mx, My, W (a window's sums stay below 2^32: differences are exact)
    __shared__ uint8_t sKsz[KL];
    __shared__ __attribute__((aligned(16))) unsigned long long sScan64[3][4];
    __shared__ __attribute__((aligned(16))) uint32_t sScan32[3][4];
    __shared__ uint32_t sCnt[16];
    // the errors and their smoothed values take the place of two of the sums once every window has been formed (the four errors of a
    // thread wait in registers for the barrier in between): 38 KB instead of 46, four workgroups per CU instead of three
    double *sS = reinterpret_cast<double *>(&sP64[0][0]), *sErr = reinterpret_cast<double *>(&sP64[1][0]);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wvs = __builtin_amdgcn_readfirstlane(wv); // the wave's number where it decides what a whole wave does: a scalar, so no loop over lanes
    const int frame = blockIdx.y;
    const uint32_t *counters = ws.d_counters + (size_t)frame * CK_CNT_STRIDE;
    const uint32_t ext_total = min(counters[CK_CNT_EXT], (uint32_t)ws.ext_cap); // positions k_seq handed out
    const uint32_t *xy = ws.d_ext_xy + (size_t)frame * ws.ext_cap;
    uint16_t *w16 = ws.d_ext_w + (size_t)frame * ws.ext_cap;
    const uint16_t *wq = ws.d_wimg + (size_t)frame * qw * qh;
    double *mval = ws.d_maxval + (size_t)frame * (ws.ext_cap / 2);
    uint16_t *mpos = ws.d_maxpos + (size_t)frame * (ws.ext_cap / 2);
    unsigned long long *mmask = ws.d_maxmask + (size_t)frame * (ws.ext_cap / 64);
    uint16_t *mpre = ws.d_maxpre + (size_t)frame * (ws.ext_cap / 64);
    long long *blk = ws.d_blk + (size_t)frame * 6 * (ws.ext_cap / 32);
    // the gradient weight of every point: one gather from the weight image (k_fit's phase 3; a position nobody wrote gathers at
    // whatever 13-bit coordinates it holds, inside the image or refused), kept for k_tail in the sequence's weight array.  The
    // span after this one is fetched while this one is worked on: its points at the top, their weights once those have arrived
    auto load_xy = [&](uint32_t s) -> uint4 {
        const long long p0 = (long long)s * CK_SPAN - KOFF + 4 * tid;
        if ((unsigned long long)s * CK_SPAN < ext_total && p0 >= 0 && p0 + 4 <= (long long)ws.ext_cap) return *reinterpret_cast<const uint4 *>(xy + p0);
        return make_uint4(0, 0, 0, 0);
    };
    auto gather_w = [&](uint32_t v) -> uint32_t {
        const int x = (int)((v >> 13) & 0x1FFFu), y = (int)(v & 0x1FFFu);
        const int ix = (x + 1) >> 1, iy = (y + 1) >> 1;
        return (ix < qw && iy < qh) ? (uint32_t)wq[(size_t)iy * qw + ix] : 1u;
    };
    uint4 x4 = load_xy(blockIdx.x);
    uint32_t ww[4] = {gather_w(x4.x), gather_w(x4.y), gather_w(x4.z), gather_w(x4.w)};
    for (uint32_t s = blockIdx.x; (unsigned long long)s * CK_SPAN < ext_total; s += gridDim.x) {
        // 1. four consecutive positions per thread: moments, running sums, one scan over the workgroup
        __builtin_amdgcn_s_waitcnt(WAIT_VMCNT0); // vmcnt(0): this span's points and weights (asked for during the span before) are here
        const long long p0 = (long long)s * CK_SPAN - KOFF + 4 * tid;
        const uint32_t xw[4] = {x4.x, x4.y, x4.z, x4.w};
        if (tid >= KOFF / 4 && tid < (KOFF + CK_SPAN) / 4) // the positions this span decides: their weights stay for k_tail
            *reinterpret_cast<uint2 *>(w16 + p0) = make_uint2(ww[0] | (ww[1] << 16), ww[2] | (ww[3] << 16));
        unsigned long long l64[4][3];
        uint32_t l32[4][3];
        unsigned long long a64[3] = {0, 0, 0};
        uint32_t a32[3] = {0, 0, 0};
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const M6 m = moments_of(xw[e] & 0x3FFFFFFu, ww[e]);
            a64[0] += (unsigned long long)m.Mxx; a64[1] += (unsigned long long)m.Mxy; a64[2] += (unsigned long long)m.Myy;
            a32[0] += (uint32_t)m.Mx; a32[1] += (uint32_t)m.My; a32[2] += (uint32_t)m.W;
#pragma unroll
            for (int q = 0; q < 3; q++) { l64[e][q] = a64[q]; l32[e][q] = a32[q]; }
        }
        unsigned long long x64[3];
        uint32_t x32[3];
#pragma unroll
        for (int q = 0; q < 3; q++) { x64[q] = wave_scan_u64(a64[q]); x32[q] = wave_scan_u32(a32[q]); }
        lds_barrier(); // the previous span's readers are done with every array
        if (lane == 63)
#pragma unroll
            for (int q = 0; q < 3; q++) { sScan64[q][wv] = x64[q]; sScan32[q][wv] = x32[q]; }
        lds_barrier();
#pragma unroll
        for (int q = 0; q < 3; q++) {
            // the waves before this one: all totals in three wide reads, summed under the wave's own number (a scalar: no loop over
            // lanes that agree anyway, no read that waits for the one before)
            const ulonglong2 t01 = *reinterpret_cast<const ulonglong2 *>(&sScan64[q][0]);
            const unsigned long long t2 = sScan64[q][2];
            const uint4 u = *reinterpret_cast<const uint4 *>(&sScan32[q][0]);
            const unsigned long long b64 = (wvs > 0 ? t01.x : 0ull) + (wvs > 1 ? t01.y : 0ull) + (wvs > 2 ? t2 : 0ull);
            const uint32_t b32 = (wvs > 0 ? u.x : 0u) + (wvs > 1 ? u.y : 0u) + (wvs > 2 ? u.z : 0u);
            x64[q] += b64 - a64[q]; x32[q] += b32 - a32[q]; // exclusive of this thread's four
        }
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int j = 4 * tid + e;
#pragma unroll
            for (int q = 0; q < 3; q++) { sP64[q][j] = l64[e][q] + x64[q]; sP32[q][j] = l32[e][q] + x32[q]; }
            const uint32_t k = (xw[e] >> 26) & 31u;
            sKsz[j] = (uint8_t)(k > 20u ? 20u : k);
        }
        // the next span's points: asked for here, behind this span's own wait (the compiler's waits are for "everything outstanding":
        // at the top of the loop the request would be waited for at once); their weights once the errors are done
        const uint4 nx4 = load_xy(s + gridDim.x);
        lds_barrier();
        // 2. running moment sums at the ends of the span's 30 aligned blocks of 32 positions, from the span's first decided position
        // (Mx, My, Mxx, Mxy, Myy, W: the order of M6).  The first-order sums are widened from 32-bit differences, which are exact
        // whatever the span's positions hold, written in this call or not: a coordinate is 13 bits of the point word (+ 1: <= 8192)
        // and a weight comes from the weight image (<= 362; k_tail reads nine bits of it), so a span's worth is at most
        // 960 x 511 x 8192 < 2^32
        if (tid < 180 && stop_after >= 2) {
            const int b = tid / 6, q = tid - 6 * b;
            const int jh = KOFF + 32 * b + 31, jl = KOFF - 1;
            long long d;
            if (q == 0) d = (long long)(uint32_t)(sP32[0][jh] - sP32[0][jl]);
            else if (q == 1) d = (long long)(uint32_t)(sP32[1][jh] - sP32[1][jl]);
            else if (q == 5) d = (long long)(uint32_t)(sP32[2][jh] - sP32[2][jl]);
            else d = (long long)(sP64[q - 2][jh] - sP64[q - 2][jl]);
            blk[((size_t)s * (CK_SPAN / 32) + b) * 6 + q] = d;
        }
        if (stop_after <= 2) { // diagnostics: 1 ends the span behind the running sums, 2 behind the block sums
            x4 = nx4;
            ww[0] = gather_w(nx4.x); ww[1] = gather_w(nx4.y); ww[2] = gather_w(nx4.z); ww[3] = gather_w(nx4.w);
            continue;
        }
        // 3. windowed line-fit error of the positions whose smoothed value is needed (k_fit's chunk loop, same operations)
        // 1 / W first, for all four positions of the thread: four table reads under way together, one wait in front of the doubles.
        // Every position takes the same path — one outside [KOFF - 4, KOFF + CK_SPAN + 4) works on the nearest one inside, its
        // result is never read — and every index lies in the table: a weight is what gather_w gave, the weight image's (<= 362)
        // or 1, whatever the position holds, and sKsz is clamped to 20, so a window's weights sum to (2 * 20 + 1) * 362 at most.  The
        // clamp is for a reader of this code, not for a case
        static_assert(INV_N == (2 * 20 + 1) * 362 + 1 && KOFF - 4 - 20 - 1 >= 0 && KOFF + CK_SPAN + 3 + 20 < KL, "a window's weight sum and its ends");
        int jc[4], ksz4[4];
        double inv4[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            jc[r] = min(max(tid + 256 * r, KOFF - 4), KOFF + CK_SPAN + 3);
            ksz4[r] = (int)sKsz[jc[r]];
            const uint32_t mw = sP32[2][jc[r] + ksz4[r]] - sP32[2][jc[r] - ksz4[r] - 1];
            inv4[r] = g_inv_table.v[min(mw, (uint32_t)(INV_N - 1))];
        }
        double ev[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int ksz = ksz4[r], hi = jc[r] + ksz, lo = jc[r] - ksz - 1;
            const uint32_t mx = sP32[0][hi] - sP32[0][lo], my = sP32[1][hi] - sP32[1][lo];
            M6 m;
            m.Mxx = (long long)(sP64[0][hi] - sP64[0][lo]); m.Mxy = (long long)(sP64[1][hi] - sP64[1][lo]); m.Myy = (long long)(sP64[2][hi] - sP64[2][lo]);
            const double inv = inv4[r];
            const double Ex = (0.5 * (double)mx) * inv, Ey = (0.5 * (double)my) * inv;
            const double Cxx = (0.25 * f64_of_u52((unsigned long long)m.Mxx)) * inv - Ex * Ex;
            const double Cxy = (0.25 * f64_of_u52((unsigned long long)m.Mxy)) * inv - Ex * Ey;
            const double Cyy = (0.25 * f64_of_u52((unsigned long long)m.Myy)) * inv - Ey * Ey;
            const double d = Cxx - Cyy, q4 = 4.0 * Cxy;
            const double disc = sqrt(d * d + q4 * Cxy);
            ev[r] = (double)(2 * ksz + 1) * (0.5 * ((Cxx + Cyy) - disc));
        }
        lds_barrier(); // every window has been read: the sums may go
        // (all KL entries are written, the ones outside [KOFF - 4, KOFF + CK_SPAN + 4) with their nearest neighbour's value, which
        // nobody reads: under a condition the compiler moves the first position's table read and doubles in here, behind the barrier)
#pragma unroll
        for (int r = 0; r < 4; r++) sErr[tid + 256 * r] = ev[r];
        const uint32_t nww[4] = {gather_w(nx4.x), gather_w(nx4.y), gather_w(nx4.z), gather_w(nx4.w)};
        lds_barrier();
        auto next_span = [&]() {
            x4 = nx4;
#pragma unroll
            for (int e = 0; e < 4; e++) ww[e] = nww[e];
        };
        if (stop_after == 3) { next_span(); continue; } // diagnostics: behind the window errors
        // 4. smoothed errors (the oracle's one-value-at-a-time sum, in its order)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int j = tid + 256 * r;
            if (j >= KOFF - 1 && j < KOFF + CK_SPAN + 1) {
                double sm = 0.0;
#pragma unroll
                for (int q = 0; q < 7; q++) sm += sErr[j + q - 3] * k_smooth[q];
                sS[j] = sm;
            }
        }
        lds_barrier();
        if (stop_after == 4) { next_span(); continue; } // diagnostics: behind the smoothing
        // 5. maxima: one word of 64 positions per wave and round
        unsigned long long bal[4];
        double myv[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int j = KOFF + tid + 256 * r;
            bool ismax = false;
            myv[r] = 0.0;
            if (j < KOFF + CK_SPAN) {
                const double v = sS[j];
                myv[r] = v;
                ismax = v > sS[j + 1] && v > sS[j - 1];
            }
            bal[r] = __ballot(ismax);
            if (lane == 0) sCnt[4 * r + wvs] = (uint32_t)__popcll(bal[r]);
        }
        lds_barrier();
        // the maxima in the words before word k: the sixteen counts in the lanes of a row, summed there, lane k's sum less its own
        const uint32_t cnt = sCnt[lane & 15], cnt_excl = row_scan_u32(cnt) - cnt;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int k = 4 * r + wvs;
            if (k >= CK_SPAN / 64) continue;
            const uint32_t pre = (uint32_t)__builtin_amdgcn_readlane((int)cnt_excl, k);
            if (lane == 0) { mmask[(size_t)s * (CK_SPAN / 64) + k] = bal[r]; mpre[(size_t)s * (CK_SPAN / 64) + k] = (uint16_t)pre; }
            if ((bal[r] >> lane) & 1ull) {
                const uint32_t pos = pre + (uint32_t)__popcll(bal[r] & ((1ull << lane) - 1ull));
                mval[(size_t)s * (CK_SPAN / 2) + pos] = myv[r];
                mpos[(size_t)s * (CK_SPAN / 2) + pos] = (uint16_t)(tid + 256 * r);
            }
        }
        next_span();
    }
}

#ifdef CK_DIAG
__global__ __launch_bounds__(256) void k_chunk(ck_stage_ws ws, int qw, int qh, int stop_after) { k_chunk_body(ws, qw, qh, stop_after); }
#else
__global__ __launch_bounds__(256) void k_chunk(ck_stage_ws ws, int qw, int qh) { k_chunk_body(ws, qw, qh, 99); }
#endif

} // namespace

#ifdef CK_DIAG
// (diagnostics, CK_EXT_BASE: the first position k_seq hands out in every frame of the call — where a cluster lands on k_chunk's span grid)
__global__ void k_ext_base(uint32_t *counters, int n, uint32_t base) {
    const int f = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (f < n) counters[(size_t)f * CK_CNT_STRIDE + CK_CNT_EXT] = base;
}
#endif

int ck_ext_room() {
#ifdef CK_DIAG
    return 2 * CK_SPAN;
#else
    return 0;
#endif
}

void ck_launch_ext_base(ck_handle *h, int n) {
#ifdef CK_DIAG
    // read per call; clamped to the room stage_caps (ck_stages.hip) adds for it.  On the handle's stream: behind k_clear's zero and
    // before the first k_seq of any lane
    int ext_base = ck_knob(CK_KNOB_EXT_BASE);
    if (ext_base > 2 * CK_SPAN) ext_base = 2 * CK_SPAN;
    if (ext_base > 0) hipLaunchKernelGGL(k_ext_base, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->ws.d_counters, n, (uint32_t)ext_base);
#endif
}

void ck_launch_chunk(ck_handle *h, int n, int wgs, int *fit_stop) {
    const ck_stage_ws &ws = h->ws;
    // spans per frame and workgroups that share them: a batch gives every workgroup a few spans, a short call one each
    const unsigned spans = (unsigned)(ws.ext_cap / CK_SPAN);
    unsigned gx = (unsigned)((wgs + n - 1) / n);
    if (gx < 8) gx = 8;
    if (gx > spans) gx = spans;
    // (k_chunk's register count capped at 96 / 80: no difference — three workgroups per CU either way, its LDS decides)
#ifdef CK_DIAG
    // (read per call; tools/ablate_chunk.sh.  Cut short — 5 is the whole kernel — its lists are not there for k_tail, which then ends
    // every cluster before it reads them, as under CK_FIT_STOP_AFTER=4)
    const int chunk_stop = ck_knob(CK_KNOB_CHUNK_STOP_AFTER);
    if (*fit_stop > 3) hipLaunchKernelGGL(k_chunk, dim3(gx, (unsigned)n), dim3(256), 0, h->stream, ws, h->qw, h->qh, chunk_stop);
    if (chunk_stop <= 5 && *fit_stop > 4) *fit_stop = 4;
#else
    if (*fit_stop > 3) hipLaunchKernelGGL(k_chunk, dim3(gx, (unsigned)n), dim3(256), 0, h->stream, ws, h->qw, h->qh);
#endif
}
