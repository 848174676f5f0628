// k_exposure.hip — exposure metering of the staged frames: per selected frame the luma histogram of a rectangle
// and, for each of CK_EXPOSURE_GAMMAS gamma curves, the histogram of the Sobel gradient magnitude of the frame seen through that
// curve.  Integer arithmetic throughout; the curves are 256-byte tables made on the host.
//
// One 256-thread workgroup walks tiles of CK_EX_TW x CK_EX_TH pixels down a tile column of one frame.  A tile and its one-pixel
// halo are loaded into LDS once (16-byte loads; 16 bytes of halo on either side keep every load aligned).  A thread owns 4 pixels
// of 8 rows: per curve it slides down its strip, maps the 6 bytes of a row through the table in LDS, keeps the horizontal halves
// of the two Sobel kernels (smooth 1 2 1, difference -1 0 1) of the last three rows, and bins floor(sqrt(Gx^2 + Gy^2)) >> 3 of
// the 4 pixels of the middle row: 15 table look-ups per 4 pixels and curve instead of 36.  The histograms of the workgroup live in
// LDS (one copy: the LDS serves one wave instruction at a time, so copies per wave would only add to the flush) and go to the
// frame's record with one integer atomicAdd per non-zero bin when the column is done.  Integer adds commute: the record does not
// depend on scheduling.  Bin 0 of a curve, where most pixels of most frames fall, is counted in a register.
#include "ck_exposure.h"

namespace {

constexpr int TW = CK_EX_TW, TH = CK_EX_TH;
constexpr int HALO_B = 16;                    // bytes of halo on either side of a tile row: the loads stay 16-byte aligned
constexpr int LROW = TW + 2 * HALO_B;         // bytes of a tile row in LDS
constexpr int LROWS = TH + 2;
constexpr int CHUNKS = LROW / 16;
constexpr int RPT = TH / 8;                   // rows of a thread's strip
constexpr int NGRAD = CK_EXPOSURE_GAMMAS * CK_EXPOSURE_BINS;
constexpr int NHIST = NGRAD + 256;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// The luma counts of one dword (4 pixels of a row) per lane.  Where the whole wave counts one value (a flat region: all 256 pixels
// inside the rectangle and equal) one lane adds 256, instead of 256 adds to one address queueing in the LDS.
__device__ __forceinline__ void luma_add(uint32_t *hist, uint32_t d, bool rowin, int px0, int x0, int x1) {
    const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)d);
    const bool same = rowin && px0 >= x0 && px0 + 4 <= x1 && d == first;
    if (__ballot(same) == ~0ull && first == (first & 255u) * 0x01010101u) {
        if ((threadIdx.x & 63) == 0) atomicAdd(&hist[first & 255u], 256u);
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (rowin && px0 + j >= x0 && px0 + j < x1) atomicAdd(&hist[(d >> (8 * j)) & 255u], 1u);
}

// floor(sqrt(s)) for s < 2^24 (exact as a float): v_sqrt_f32 is within one ulp, so the truncated root is off by at most one
__device__ __forceinline__ uint32_t isqrt24(uint32_t s) {
    uint32_t r = (uint32_t)__builtin_amdgcn_sqrtf((float)s);
    if (r * r > s) r--;
    else if ((r + 1) * (r + 1) <= s) r++;
    return r;
}

__global__ __launch_bounds__(256) void k_exposure(const uint8_t *frames, int stride, size_t pitch, int w, int h, int tiles_y,
                                                  const uint8_t *lut, const ck_ex_job *jobs, ck_exposure_stats_t *stats) {
    __shared__ u32x4 s_tile4[LROWS * CHUNKS];
    __shared__ uint32_t s_lut32[CK_EXPOSURE_GAMMAS * 64];
    __shared__ uint32_t s_hist[NHIST]; // grad[k][bin], then luma[256]
    const uint32_t *s_tile = reinterpret_cast<const uint32_t *>(s_tile4);
    const uint8_t *s_lut = reinterpret_cast<const uint8_t *>(s_lut32);
    const int tid = threadIdx.x;
    const ck_ex_job job = jobs[blockIdx.z];
    const int x0 = job.x0, y0 = job.y0, x1 = job.x1, y1 = job.y1;
    const bool empty = x0 >= x1 || y0 >= y1;
    // the gradient's domain: the rectangle inside [1, w - 1) x [1, h - 1)
    const int gx0 = max(x0, 1), gy0 = max(y0, 1), gx1 = min(x1, w - 1), gy1 = min(y1, h - 1);
    uint32_t *rec = reinterpret_cast<uint32_t *>(stats + blockIdx.z);
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
        stats[blockIdx.z].n_luma = empty ? 0u : (uint32_t)(x1 - x0) * (uint32_t)(y1 - y0);
        stats[blockIdx.z].n_grad = (empty || gx0 >= gx1 || gy0 >= gy1) ? 0u : (uint32_t)(gx1 - gx0) * (uint32_t)(gy1 - gy0);
    }
    const int tx0 = blockIdx.x * TW;
    if (empty || tx0 >= x1 || tx0 + TW <= x0) return; // (the same for the whole workgroup)
    for (int i = tid; i < CK_EXPOSURE_GAMMAS * 64; i += 256) s_lut32[i] = reinterpret_cast<const uint32_t *>(lut)[i];
    for (int i = tid; i < NHIST; i += 256) s_hist[i] = 0;
    const uint8_t *frame = frames + (size_t)job.frame * pitch;
    const int cg = tid & 31, rg = tid >> 5;
    const int px0 = tx0 + 4 * cg;
    uint32_t gmask = 0; // bit j: pixel px0 + j lies in the gradient domain's columns
    for (int j = 0; j < 4; j++) gmask |= (uint32_t)(px0 + j >= gx0 && px0 + j < gx1) << j;

    for (int ty = blockIdx.y; ty < tiles_y; ty += gridDim.y) {
        const int ty0 = ty * TH;
        if (ty0 >= y1 || ty0 + TH <= y0) continue;
        __syncthreads(); // the last tile has been read (first round: the tables and the zeroed histograms are in place)
        for (int i = tid; i < LROWS * CHUNKS; i += 256) {
            const int row = i / CHUNKS, c = i - row * CHUNKS;
            const int gy = ty0 - 1 + row, gb = tx0 - HALO_B + 16 * c;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (gy >= 0 && gy < h && gb >= 0 && gb + 16 <= stride) v = *reinterpret_cast<const u32x4 *>(frame + (size_t)gy * stride + gb);
            s_tile4[i] = v;
        }
        __syncthreads();
        const int py0 = ty0 + rg * RPT; // first row of the strip; LDS row of frame row y: y - ty0 + 1
        // luma histogram of the strip
#pragma unroll
        for (int r = 0; r < RPT; r++) {
            const uint32_t d = s_tile[(rg * RPT + r + 1) * (LROW / 4) + HALO_B / 4 + cg];
            const bool rowin = py0 + r >= y0 && py0 + r < y1;
            luma_add(s_hist + NGRAD, d, rowin, px0, x0, x1);
        }
        // gradient histogram of every curve; bit 4 r + j of gbits: pixel j of the strip's row r lies in the gradient's domain
        uint32_t gbits = 0;
#pragma unroll
        for (int r = 0; r < RPT; r++) gbits |= ((py0 + r >= gy0 && py0 + r < gy1) ? gmask : 0u) << (4 * r);
#pragma unroll 1
        for (int k = 0; k < CK_EXPOSURE_GAMMAS; k++) {
            const uint8_t *t = s_lut + 256 * k;
            uint32_t *hist = s_hist + CK_EXPOSURE_BINS * k;
            int sa[4] = {}, da[4] = {}, sb[4] = {}, db[4] = {}; // smooth / difference halves of the two rows above the current one
            uint32_t vb = gbits;
            asm volatile("" : "+v"(vb)); // (kept in one register: 32 lane masks hoisted out of this loop would not fit the scalar file)
            uint32_t zeros = 0; // bin 0 (most pixels of most frames) is counted in a register and added once per curve
#pragma unroll
            for (int rr = 0; rr < RPT + 2; rr++) { // frame row py0 - 1 + rr
                const uint32_t *row = s_tile + (rg * RPT + rr) * (LROW / 4) + HALO_B / 4 + cg;
                const uint32_t dl = row[-1], dm = row[0], dr = row[1];
                int m[6];
                m[0] = t[dl >> 24];
                m[1] = t[dm & 255u]; m[2] = t[(dm >> 8) & 255u]; m[3] = t[(dm >> 16) & 255u]; m[4] = t[dm >> 24];
                m[5] = t[dr & 255u];
                int sc[4], dc[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    sc[j] = m[j] + 2 * m[j + 1] + m[j + 2];
                    dc[j] = m[j + 2] - m[j];
                }
                if (rr >= 2) {
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int gx = da[j] + 2 * db[j] + dc[j], gy = sc[j] - sa[j];
                        const uint32_t s = (uint32_t)(gx * gx + gy * gy);
                        const uint32_t bin = isqrt24(s) >> 3;
                        const bool v = (vb >> (4 * (rr - 2) + j)) & 1u;
                        zeros += v && !bin;
                        if (v && bin) atomicAdd(&hist[bin], 1u);
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; j++) { sa[j] = sb[j]; da[j] = db[j]; sb[j] = sc[j]; db[j] = dc[j]; }
            }
            if (zeros) atomicAdd(&hist[0], zeros);
        }
    }
    __syncthreads();
    for (int i = tid; i < NHIST; i += 256) {
        const uint32_t v = s_hist[i];
        if (v) atomicAdd(rec + (i < NGRAD ? 256 + i : i - NGRAD), v); // ck_exposure_stats_t: luma[256], then grad
    }
}

} // namespace

static_assert(sizeof(ck_exposure_stats_t) == 4 * (256 + CK_EXPOSURE_GAMMAS * CK_EXPOSURE_BINS + 4), "ck_exposure_stats_t layout");
static_assert(offsetof(ck_exposure_stats_t, grad) == 1024, "ck_exposure_stats_t layout");
static_assert(CK_EX_TW == 128 && CK_EX_TH % 8 == 0, "tile geometry");

int ck_launch_exposure(hipStream_t stream, const ck_dev_image &img, int w, int h, int n, const uint8_t *d_lut, const ck_ex_job *d_jobs,
                       ck_exposure_stats_t *d_stats) {
    if (n <= 0) return CK_OK;
    if (n > 65535 || img.stride % 16 || img.pitch % 16 || (uintptr_t)img.p % 16) return CK_EINVAL;
    CK_HIP(hipMemsetAsync(d_stats, 0, sizeof(ck_exposure_stats_t) * (size_t)n, stream));
    const int tiles_x = (w + TW - 1) / TW, tiles_y = (h + TH - 1) / TH;
    // a workgroup takes every split-th tile of its column: few flushes on a large batch, enough workgroups on a small one
    int split = (2048 + tiles_x * n - 1) / (tiles_x * n);
    split = split < 1 ? 1 : (split > tiles_y ? tiles_y : split);
    hipLaunchKernelGGL(k_exposure, dim3((unsigned)tiles_x, (unsigned)split, (unsigned)n), dim3(256), 0, stream, img.p, img.stride, img.pitch, w, h,
                       tiles_y, d_lut, d_jobs, d_stats);
    CK_HIP(hipGetLastError());
    return CK_OK;
}
