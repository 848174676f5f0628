// Baseline JPEG luma decode on the device: one workgroup per frame unstuffs the scan, cuts it into
// subsequences, decodes them speculatively until every piece starts from the state its predecessor ends in, redecodes them
// writing Y coefficients and turns the Y DC differences into values; then many lanes per 8x8 block run libjpeg's islow IDCT.
// Every read of the scan is bounded by the frame's own region, every coefficient write by its block's 64 entries.
#include "ck_internal.h"
#include "ck_jpeg.h"
#include "ck_jpeg_tables.h"

namespace {

constexpr int NT = CK_JPEG_FRAME_THREADS;
constexpr int NW = NT / 64;
constexpr uint32_t SUB = CK_JPEG_SUB_BITS;

__constant__ uint8_t k_natural[64] = CK_JPEG_NATURAL_ORDER;

struct FrameLds {
    ck_jpeg_huff tab[3][2]; // by scan component: DC, AC
    uint32_t wv[NW], wf[NW];
    uint32_t bcast, term, bad;
};

// ---- workgroup scans (all NT threads call them) --------------------------------------------------------------------------
__device__ uint32_t block_excl(FrameLds &L, uint32_t v, uint32_t &total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint32_t incl = wave_scan_u32(v);
    if (lane == 63) L.wv[wid] = incl;
    __syncthreads();
    uint32_t off = 0, tot = 0;
    for (int w = 0; w < NW; w++) {
        const uint32_t t = L.wv[w];
        off += w < wid ? t : 0;
        tot += t;
    }
    __syncthreads();
    total = tot;
    return off + incl - v;
}

// inclusive sum that restarts at every element with `flag`; `carry` is the running sum of the chunks before (uniform)
__device__ uint32_t block_seg_incl(FrameLds &L, uint32_t v, bool flag, uint32_t &carry) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t x = v, f = flag ? 1u : 0u;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d), g = __shfl_up(f, d);
        if (lane >= d) {
            if (!f) x += y;
            f |= g;
        }
    }
    if (lane == 63) { L.wv[wid] = x; L.wf[wid] = f; }
    __syncthreads();
    if (!f) {
        uint32_t c = 0;
        bool stop = false;
        for (int w = wid - 1; w >= 0 && !stop; w--) {
            c += L.wv[w];
            stop = L.wf[w] != 0;
        }
        x += c + (stop ? 0u : carry);
    }
    __syncthreads();
    if (threadIdx.x == NT - 1) L.bcast = x;
    __syncthreads();
    carry = L.bcast;
    return x;
}

// ---- bit reader over the frame's unstuffed scan (big-endian words; all ones past its end) ----------------------------------
struct BitReader {
    const uint32_t *w;
    uint32_t nw, wi, pos;
    uint64_t buf;
    int nb;
    uint4 q;      // the 16-byte group of words last loaded (one load per 128 bits: the serial walk is latency-bound)
    uint32_t qg;  // its index, UINT32_MAX: none
    __device__ uint32_t word(uint32_t i) {
        if (i >= nw) return 0xFFFFFFFFu;
        if ((i >> 2) != qg) { qg = i >> 2; q = reinterpret_cast<const uint4 *>(w)[qg]; } // inside the frame's 16-byte aligned region
        const uint32_t x = (i & 3) == 0 ? q.x : (i & 3) == 1 ? q.y : (i & 3) == 2 ? q.z : q.w;
        return __builtin_bswap32(x);
    }
    __device__ void refill() {
        while (nb <= 32) {
            buf |= (uint64_t)word(wi) << (32 - nb);
            wi++;
            nb += 32;
        }
    }
    __device__ void seek(uint32_t p) {
        pos = p; wi = p >> 5; buf = 0; nb = 0; qg = 0xFFFFFFFFu;
        refill();
        const int s = (int)(p & 31);
        buf <<= s; nb -= s;
        refill();
    }
    __device__ void skip(int n) { buf <<= n; nb -= n; pos += (uint32_t)n; }
    __device__ uint32_t get(int n) { // n <= 16, nb >= n
        const uint32_t v = n ? (uint32_t)(buf >> (64 - n)) : 0u;
        skip(n);
        return v;
    }
};

// libjpeg's jpeg_huff_decode: the 9-bit lookahead, then lengths 10..16; -1 = no code (16 one-bits never are one)
__device__ __forceinline__ int huff_sym(const ck_jpeg_huff &t, BitReader &br) {
    const uint32_t p = (uint32_t)(br.buf >> 48);
    const uint32_t lk = t.look[p >> 7];
    if (lk) {
        br.skip((int)(lk >> 8));
        return (int)(lk & 0xFF);
    }
    for (int l = 10; l <= 16; l++) {
        const int32_t code = (int32_t)(p >> (16 - l));
        if (code <= t.maxcode[l]) {
            const int32_t idx = code + t.valoff[l];
            if (idx < 0 || idx > 255) return -1;
            br.skip(l);
            return t.vals[idx];
        }
    }
    return -1;
}

__device__ __forceinline__ int extend(uint32_t v, int s) { return v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

__device__ __forceinline__ uint64_t pack_state(uint32_t pos, int slot, int zz) { return ((uint64_t)pos << 16) | ((uint32_t)slot << 8) | (uint32_t)zz; }

// Y block (in the frame's block grid) of block `b` of interval `k`; UINT32_MAX for a chroma block
__device__ __forceinline__ uint32_t y_block(const ck_jpeg_desc &d, uint32_t k, uint32_t b) {
    const uint32_t mcu = k * d.restart + b / d.bpm, sl = b % d.bpm;
    if (sl >= d.nyb) return 0xFFFFFFFFu;
    const uint32_t my = mcu / d.mcux, mx = mcu - my * d.mcux;
    return (my * (d.nyb / d.hs) + sl / d.hs) * d.yblk_stride + mx * d.hs + sl % d.hs;
}
// The colour form's store: the Y grid, then one Cb block per MCU in raster order over the MCUs, then the Cr blocks.  Block `b` of
// interval `k` for every slot; below nmcu * bpm while b is below the interval's block count
__device__ __forceinline__ uint32_t c_block(const ck_jpeg_desc &d, uint32_t mcu, uint32_t comp) { return d.nmcu * (d.nyb + comp - 1) + mcu; }
__device__ __forceinline__ uint32_t any_block(const ck_jpeg_desc &d, uint32_t k, uint32_t b) {
    const uint32_t sl = b % d.bpm;
    return sl < d.nyb ? y_block(d, k, b) : c_block(d, k * d.restart + b / d.bpm, sl - d.nyb + 1);
}

struct RunOut {
    uint32_t nb;  // blocks completed at or before the interval's end
    int32_t err;  // index (relative to the entry) of the block in which decoding failed, -1 if none
};

// Decodes every code that starts before `end` from the reader's state.  Without WRITE (speculative) an invalid code or a run
// past 63 is no failure: the decode goes on at a block start (one bit on for an invalid code), deterministically, so that a wrong
// trajectory can still merge with the true one; only the WRITE pass from synchronised entries decides corruption.  WRITE: coefficients of the Y blocks with an index below
// `expected` (blk0 = index of the block in progress at entry) go to coef; with COLOR those of the Cb and Cr blocks too.
template <bool WRITE, bool COLOR = false>
__device__ RunOut decode_run(const FrameLds &L, const ck_jpeg_desc &d, BitReader &br, uint32_t end, uint32_t lim, int &slot, int &zz,
                             int16_t *coef, uint32_t k, uint32_t blk0, uint32_t expected) {
    RunOut r{0u, -1};
    uint32_t yb = 0xFFFFFFFFu;
    if (WRITE && blk0 < expected) yb = COLOR ? any_block(d, k, blk0) : y_block(d, k, blk0);
    while (br.pos < end) {
        br.refill();
        const int comp = slot < (int)d.nyb ? 0 : slot - (int)d.nyb + 1;
        const int sym = huff_sym(L.tab[comp][zz ? 1 : 0], br);
        if (sym < 0) {
            if (!WRITE) { br.skip(1); zz = 0; continue; } // speculative: not corruption; resume one bit on at a block start
            r.err = (int32_t)r.nb;
            break;
        }
        if (zz == 0) {
            const int s = sym; // DC categories are <= 15 (ck_jpeg.hip refuses other tables)
            const int v = s ? extend(br.get(s), s) : 0;
            if (WRITE && yb != 0xFFFFFFFFu) coef[(size_t)yb * 64] = (int16_t)v;
            zz = 1;
        } else {
            const int rr = sym >> 4, s = sym & 15;
            if (s) {
                zz += rr;
                if (zz > 63) {
                    if (!WRITE) { zz = 0; continue; }
                    r.err = (int32_t)r.nb;
                    break;
                }
                const int v = extend(br.get(s), s);
                if (WRITE && yb != 0xFFFFFFFFu) coef[(size_t)yb * 64 + k_natural[zz]] = (int16_t)v;
                zz++;
            } else if (rr == 15) {
                if (zz + 15 > 63) {
                    if (!WRITE) { zz = 0; continue; }
                    r.err = (int32_t)r.nb;
                    break;
                }
                zz += 16;
            } else {
                zz = 64; // EOB (and, as libjpeg reads them, the EOB-run symbols of progressive scans)
            }
        }
        if (zz >= 64) {
            if (br.pos <= lim) r.nb++;
            zz = 0;
            slot = slot + 1 == (int)d.bpm ? 0 : slot + 1;
            if (WRITE) yb = blk0 + r.nb < expected ? (COLOR ? any_block(d, k, blk0 + r.nb) : y_block(d, k, blk0 + r.nb)) : 0xFFFFFFFFu;
        }
    }
    return r;
}

__device__ __forceinline__ uint32_t interval_blocks(const ck_jpeg_desc &d, uint32_t k) {
    const uint32_t left = d.nmcu - k * d.restart;
    return (left < d.restart ? left : d.restart) * d.bpm;
}

// A baseline block is at most 68 symbols (DC, 63 coefficients, 3 ZRL, EOB) of at most 16 + 15 bits: 264 bytes.  Bytes of an
// interval past 272 per block it needs are trailing bits whatever they hold, so the decode never looks at them: the work on a
// frame is linear in its pixels however much junk precedes its EOI.
constexpr uint32_t MAX_BLOCK_BYTES = 272;
__device__ __forceinline__ uint32_t interval_end_byte(const ck_jpeg_desc &d, const uint32_t *istart, uint32_t k) {
    const uint64_t cap = (uint64_t)istart[k] + (uint64_t)MAX_BLOCK_BYTES * interval_blocks(d, k);
    return (uint32_t)min((uint64_t)istart[k + 1], cap);
}

// Ends the frame (uniformly) when a stage flagged it; every thread reads the flag before any can set it again.
__device__ bool frame_failed(FrameLds &L, uint32_t *status, int f) {
    __syncthreads();
    const uint32_t bad = L.bad;
    __syncthreads();
    if (bad && threadIdx.x == 0) status[f] = bad;
    return bad != 0;
}

// COLOR (ck_upload_jpeg_color, a ring of ck_ingest_create_jpeg_color): the write pass keeps the Cb and Cr coefficients as well and
// their DC differences are summed like Y's.  Everything else, and all of the luma form, is the same code.
template <bool COLOR>
__global__ void __launch_bounds__(NT) k_jpeg_frame(const ck_jpeg_desc *__restrict__ descs, const ck_jpeg_huff *__restrict__ huff,
                                                   const uint8_t *__restrict__ raw_base, uint8_t *__restrict__ cmp_base,
                                                   uint32_t *__restrict__ int_base, ck_jpeg_sub *__restrict__ sub_base,
                                                   int16_t *__restrict__ coef_base, size_t coef_frame_blocks,
                                                   uint32_t *__restrict__ status) {
    __shared__ FrameLds L;
    const int f = blockIdx.x, tid = threadIdx.x;
    const ck_jpeg_desc &d = descs[f]; // (a private copy would live in scratch: the helpers take it by reference)
    if (d.status) {
        if (tid == 0) status[f] = d.status;
        return;
    }
    {
        const int ncomp = d.bpm == 1 ? 1 : 3;
        constexpr int Q = (int)(sizeof(ck_jpeg_huff) / 16);
        for (int i = tid; i < ncomp * 2 * Q; i += NT) {
            const int t = i / Q, q = i % Q, c = t >> 1;
            const uint4 *src = reinterpret_cast<const uint4 *>(&huff[(t & 1) ? d.ac[c] : d.dc[c]]);
            reinterpret_cast<uint4 *>(&L.tab[c][t & 1])[q] = src[q];
        }
    }
    if (tid == 0) L.bad = 0;
    __syncthreads();

    // ---- 1. unstuff: drop the 0x00 after 0xFF and fill bytes, cut at the first marker that is not RSTn, check the RSTs ----------
    const uint8_t *raw = raw_base + d.raw_off;
    uint8_t *cmp = cmp_base + d.raw_off;
    uint32_t *istart = int_base + d.int_off;
    const uint32_t len = d.raw_len;
    uint32_t out_base = 0, rst_base = 0;
    bool done = false;
    for (uint32_t c0 = 0; c0 < len && !done; c0 += NT * 4) {
        const uint32_t i0 = c0 + (uint32_t)tid * 4;
        // per byte j: kinds >> 2j = 0 drop, 1 emit, 2 RST, 3 terminating marker; vals >> 8j = the byte / the RST's number
        uint32_t kinds = 0, vals = 0;
        uint32_t my_term = 0xFFFFFFFFu;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t i = i0 + j;
            if (i >= len) continue;
            const uint32_t b = raw[i], p = i ? raw[i - 1] : 0u, nx = i + 1 < len ? raw[i + 1] : 0x100u;
            uint32_t kd = 0, v = 0;
            if (p == 0xFF && b != 0xFF) {
                if (b >= 0xD0 && b <= 0xD7) { kd = 2; v = b - 0xD0; }
                else if (b != 0) { kd = 3; if (my_term == 0xFFFFFFFFu) my_term = i; } // (b == 0: the stuffed zero)
            } else if (b == 0xFF) {
                if (nx == 0) { kd = 1; v = 0xFF; } // a data byte 0xFF; otherwise a fill byte or a marker's lead
            } else {
                kd = 1; v = b;
            }
            kinds |= kd << (2 * j);
            vals |= v << (8 * j);
        }
        if (tid == 0) L.term = 0xFFFFFFFFu;
        __syncthreads();
        if (my_term != 0xFFFFFFFFu) atomicMin(&L.term, my_term);
        __syncthreads();
        const uint32_t term = L.term;
        uint32_t e = 0, r = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (i0 + j >= term) kinds &= ~(3u << (2 * j));
            const uint32_t kd = (kinds >> (2 * j)) & 3;
            e += kd == 1;
            r += kd == 2;
        }
        uint32_t total;
        const uint32_t ex = block_excl(L, e | (r << 16), total);
        uint32_t o = out_base + (ex & 0xFFFFu), ri = rst_base + (ex >> 16);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t kd = (kinds >> (2 * j)) & 3, v = (vals >> (8 * j)) & 0xFF;
            if (kd == 1) cmp[o++] = (uint8_t)v;
            else if (kd == 2) {
                if (ri + 1 >= d.nint || v != (ri & 7)) atomicOr(&L.bad, (uint32_t)CK_JPEG_CORRUPT); // in excess / out of sequence
                else istart[ri + 1] = o;
                ri++;
            }
        }
        out_base += total & 0xFFFFu;
        rst_base += total >> 16;
        done = term != 0xFFFFFFFFu;
    }
    if (tid == 0) {
        istart[0] = 0;
        istart[d.nint] = out_base;
        for (uint32_t i = out_base; i < ((out_base + 3) & ~3u); i++) cmp[i] = 0xFF; // the last word reads as ones past the end
        if (rst_base != d.nint - 1) atomicOr(&L.bad, (uint32_t)CK_JPEG_CORRUPT);      // restart markers missing
    }
    if (frame_failed(L, status, f)) return;
    BitReader br;
    br.w = reinterpret_cast<const uint32_t *>(cmp);
    br.nw = (out_base + 3) >> 2;

    // ---- 2. subsequences: every interval in pieces of SUB bits (one piece at least) ------------------------------------------------
    ck_jpeg_sub *sub = sub_base + d.sub_off;
    uint32_t nsub = 0;
    for (uint32_t k0 = 0; k0 < d.nint; k0 += NT) {
        const uint32_t k = k0 + tid;
        uint32_t cnt = 0, b0 = 0, b1 = 0;
        if (k < d.nint) {
            b0 = istart[k]; b1 = interval_end_byte(d, istart, k);
            cnt = ((b1 - b0) * 8 + SUB - 1) / SUB;
            cnt = cnt ? cnt : 1;
        }
        uint32_t total;
        const uint32_t ex = block_excl(L, cnt, total);
        for (uint32_t j = 0; j < cnt; j++) {
            const uint32_t s = nsub + ex + j;
            if (s >= d.sub_cap) { atomicOr(&L.bad, (uint32_t)CK_JPEG_CORRUPT); break; }
            ck_jpeg_sub &rec = sub[s];
            const uint32_t st = b0 * 8 + j * SUB;
            rec.start = st;
            rec.end = min(st + SUB, b1 * 8);
            rec.interval = k;
            rec.first = j == 0;
            rec.entry = pack_state(st, 0, 0);
            rec.nb = 0;
        }
        nsub += total;
    }
    if (frame_failed(L, status, f)) return;

    // ---- 3. speculative decode: every piece from "slot 0, DC next" at its first bit ------------------------------------------------
    for (uint32_t s = tid; s < nsub; s += NT) {
        const uint32_t st = sub[s].start, en = sub[s].end, k = sub[s].interval;
        br.seek(st);
        int slot = 0, zz = 0;
        const RunOut r = decode_run<false>(L, d, br, en, interval_end_byte(d, istart, k) * 8, slot, zz, nullptr, k, 0, 0);
        sub[s].exit[0] = pack_state(br.pos, slot, zz);
        sub[s].nb = r.nb;
    }
    // ---- 4. synchronise: a piece whose predecessor now ends in another state than the one it started from decodes again
    // from that state.  A piece after an exact one is exact, so round t leaves pieces 0..t of every interval exact at the latest.
    // At most SYNC_ROUNDS rounds (each one decode per piece at most); then one lane per interval walks its pieces in order and
    // re-decodes those whose entry is still not their predecessor's exit.  Either way every piece is decoded O(1) times. ----------
    constexpr int SYNC_ROUNDS = 4;
    int cur = 0;
    bool converged = false;
    for (int round = 0; round < SYNC_ROUNDS && !converged; round++) {
        __syncthreads();
        int changed = 0;
        for (uint32_t s = tid; s < nsub; s += NT) {
            const uint64_t ex_cur = sub[s].exit[cur];
            if (!sub[s].first) {
                const uint64_t e = sub[s - 1].exit[cur];
                if (e != sub[s].entry) {
                    const uint32_t en = sub[s].end, k = sub[s].interval;
                    br.seek((uint32_t)(e >> 16));
                    int slot = (int)((e >> 8) & 0xFF), zz = (int)(e & 0xFF);
                    const RunOut r = decode_run<false>(L, d, br, en, interval_end_byte(d, istart, k) * 8, slot, zz, nullptr, k, 0, 0);
                    sub[s].entry = e;
                    sub[s].exit[cur ^ 1] = pack_state(br.pos, slot, zz);
                    sub[s].nb = r.nb;
                    changed = 1;
                    continue;
                }
            }
            sub[s].exit[cur ^ 1] = ex_cur;
        }
        cur ^= 1;
        converged = !__syncthreads_or(changed);
    }
    if (!converged) {
        __syncthreads();
        for (uint32_t s = tid; s < nsub; s += NT) {
            if (!sub[s].first) continue;
            uint64_t prev = sub[s].exit[cur];
            // blocks the exact chain has completed so far: once the interval has all it needs, the pieces after are trailing bits
            // (their block indices are past the interval's count, so nothing downstream reads their states)
            const uint32_t need = interval_blocks(d, sub[s].interval);
            uint32_t done_blocks = sub[s].nb;
            for (uint32_t j = s + 1; j < nsub && !sub[j].first && done_blocks < need; j++) {
                if (sub[j].entry != prev) {
                    const uint32_t en = sub[j].end, k = sub[j].interval;
                    br.seek((uint32_t)(prev >> 16));
                    int slot = (int)((prev >> 8) & 0xFF), zz = (int)(prev & 0xFF);
                    const RunOut r = decode_run<false>(L, d, br, en, interval_end_byte(d, istart, k) * 8, slot, zz, nullptr, k, 0, 0);
                    sub[j].entry = prev;
                    sub[j].exit[cur] = pack_state(br.pos, slot, zz);
                    sub[j].nb = r.nb;
                }
                prev = sub[j].exit[cur];
                done_blocks += sub[j].nb;
            }
        }
    }
    __syncthreads();

    // ---- 5. block index of every piece's entry (a sum of the blocks before it in its interval); intervals one block short -------
    {
        uint32_t carry = 0;
        for (uint32_t s0 = 0; s0 < nsub; s0 += NT) {
            const uint32_t s = s0 + tid;
            const bool valid = s < nsub;
            const uint32_t nb = valid ? sub[s].nb : 0u;
            const uint32_t incl = block_seg_incl(L, nb, valid && sub[s].first, carry);
            if (valid) {
                sub[s].blk0 = incl - nb;
                if ((s + 1 == nsub || sub[s + 1].first) && incl < interval_blocks(d, sub[s].interval))
                    atomicOr(&L.bad, (uint32_t)CK_JPEG_CORRUPT); // the interval ends before its MCUs do
            }
        }
    }
    // zero the frame's Y coefficients, with COLOR all its nmcu * bpm blocks (the decode writes the non-zero ones)
    int16_t *coef = coef_base + (size_t)f * coef_frame_blocks * 64;
    {
        const size_t n16 = (COLOR ? (size_t)d.nmcu * d.bpm : (size_t)d.yblk_stride * d.yblk_rows) * 64 * sizeof(int16_t) / 16;
        uint4 *z = reinterpret_cast<uint4 *>(coef);
        for (size_t i = tid; i < n16; i += NT) z[i] = make_uint4(0, 0, 0, 0);
    }
    if (frame_failed(L, status, f)) return;

    // ---- 6. the synchronised decode, writing Y coefficients (Y DC as differences) ---------------------------------------------------
    for (uint32_t s = tid; s < nsub; s += NT) {
        const uint64_t e = sub[s].entry;
        const uint32_t en = sub[s].end, k = sub[s].interval, blk0 = sub[s].blk0, expected = interval_blocks(d, k);
        br.seek((uint32_t)(e >> 16));
        int slot = (int)((e >> 8) & 0xFF), zz = (int)(e & 0xFF);
        const RunOut r = decode_run<true, COLOR>(L, d, br, en, interval_end_byte(d, istart, k) * 8, slot, zz, coef, k, blk0, expected);
        if (r.err >= 0 && blk0 + (uint32_t)r.err < expected) atomicOr(&L.bad, (uint32_t)CK_JPEG_CORRUPT);
    }
    if (frame_failed(L, status, f)) return;

    // ---- 7. DC prediction: a sum of the Y DC differences in decode order that restarts with every interval ---------------------
    {
        const uint32_t total = d.nmcu * d.nyb;
        uint32_t carry = 0;
        for (uint32_t t0 = 0; t0 < total; t0 += NT) {
            const uint32_t t = t0 + tid;
            const bool valid = t < total;
            uint32_t yb = 0, v = 0;
            bool flag = false;
            if (valid) {
                const uint32_t mcu = t / d.nyb, sl = t % d.nyb;
                flag = sl == 0 && mcu % d.restart == 0;
                yb = y_block(d, mcu / d.restart, (mcu % d.restart) * d.bpm + sl);
                v = (uint32_t)(int32_t)coef[(size_t)yb * 64];
            }
            const uint32_t incl = block_seg_incl(L, v, flag, carry);
            if (valid) coef[(size_t)yb * 64] = (int16_t)incl; // libjpeg keeps the sum in an int and stores it as a JCOEF
        }
    }
    if constexpr (COLOR) { // ... and one sum per chroma component over its block of every MCU
        for (uint32_t comp = 1; comp < d.bpm - d.nyb + 1; comp++) {
            uint32_t carry = 0;
            for (uint32_t t0 = 0; t0 < d.nmcu; t0 += NT) {
                const uint32_t t = t0 + tid;
                const bool valid = t < d.nmcu;
                const uint32_t cb = valid ? c_block(d, t, comp) : 0u;
                const uint32_t v = valid ? (uint32_t)(int32_t)coef[(size_t)cb * 64] : 0u;
                const uint32_t incl = block_seg_incl(L, v, valid && t % d.restart == 0, carry);
                if (valid) coef[(size_t)cb * 64] = (int16_t)incl;
            }
        }
    }
    if (tid == 0) status[f] = 0;
}

// ---- islow IDCT (libjpeg-turbo jidctint.c, jpeg_idct_islow), 8 lanes per block -----------------------------------------------
constexpr int IDCT_NT = 256, IDCT_BLOCKS = IDCT_NT / 8;

__device__ __forceinline__ void islow_1d(const int64_t in[8], int64_t out[8]) {
    int64_t z2 = in[2], z3 = in[6];
    int64_t z1 = (z2 + z3) * 4433;            // FIX_0_541196100
    int64_t tmp2 = z1 + z3 * -15137;          // FIX_1_847759065
    int64_t tmp3 = z1 + z2 * 6270;            // FIX_0_765366865
    z2 = in[0]; z3 = in[4];
    int64_t tmp0 = (z2 + z3) * 8192;          // LEFT_SHIFT(., CONST_BITS)
    int64_t tmp1 = (z2 - z3) * 8192;
    const int64_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    int64_t z4 = tmp1 + tmp3;
    const int64_t z5 = (z3 + z4) * 9633;      // FIX_1_175875602
    tmp0 *= 2446;                             // FIX_0_298631336
    tmp1 *= 16819;                            // FIX_2_053119869
    tmp2 *= 25172;                            // FIX_3_072711026
    tmp3 *= 12299;                            // FIX_1_501321110
    z1 *= -7373;                              // FIX_0_899976223
    z2 *= -20995;                             // FIX_2_562915447
    z3 *= -16069;                             // FIX_1_961570560
    z4 *= -3196;                              // FIX_0_390180644
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    out[0] = tmp10 + tmp3; out[7] = tmp10 - tmp3;
    out[1] = tmp11 + tmp2; out[6] = tmp11 - tmp2;
    out[2] = tmp12 + tmp1; out[5] = tmp12 - tmp1;
    out[3] = tmp13 + tmp0; out[4] = tmp13 - tmp0;
}

// libjpeg's post-IDCT range-limit table at a MASKED index (x & 1023): the output sample of a descaled value x
__device__ __forceinline__ uint8_t range_limit(int64_t x) {
    const int j = (int)x & 1023;
    return (uint8_t)(j < 128 ? j + 128 : j < 512 ? 255 : j < 896 ? 0 : j - 896);
}

// The staged frame is orient(S, O) of the decoded luma S (sw x sh): the contract of chalkydri_hip.h's raw formats, DESIGN.md §4c.
// The two passes run in libjpeg's order whatever O is; the turn happens on the eight finished bytes of a lane.  O = none is the
// kernel as it was before frames could be turned: row c of block (bx, by) goes to row by*8+c, column bx*8 with one 8-byte store.
// rotate-180: a lane reverses its bytes, and the block lands mirrored.  The quarter turns transpose the block's 8 x 8 bytes
// between its eight lanes through a padded LDS tile, so that every lane again owns one row of the TURNED block and stores it
// with one row-contiguous store (8 bytes when its first column is a multiple of 8 and the block does not hang over the frame,
// bytes otherwise).  Every store is to a pixel (x, y) with 0 <= x < the oriented width and 0 <= y < the oriented height.
template <int O>
__global__ void __launch_bounds__(IDCT_NT) k_jpeg_idct(const ck_jpeg_desc *__restrict__ descs, const int32_t *__restrict__ qts,
                                                       const int16_t *__restrict__ coef_base, size_t coef_frame_blocks,
                                                       const uint32_t *__restrict__ status, uint8_t *__restrict__ frames, int stride,
                                                       size_t pitch, int w, int h) { // w x h: the source S
    __shared__ int32_t ws[IDCT_BLOCKS][8][9];
    const int f = blockIdx.y, g = threadIdx.x >> 3, c = threadIdx.x & 7;
    const int bxn = (w + 7) / 8, byn = (h + 7) / 8;
    const int b = blockIdx.x * IDCT_BLOCKS + g;
    const bool live = b < bxn * byn;
    // consecutive blocks follow a row of the ORIENTED frame, so that the eight blocks of a wave store 64 contiguous bytes per row:
    // a source row for none and rotate-180, a source column for the quarter turns (a block's coefficients are one 128-byte line
    // wherever its neighbours lie, so the reads do not care)
    constexpr bool kQuarter = O == CK_ORIENT_CLOCKWISE || O == CK_ORIENT_COUNTERCLOCKWISE;
    const int by = !live ? 0 : kQuarter ? b % byn : b / bxn, bx = !live ? 0 : kQuarter ? b / byn : b % bxn;
    const bool ok = status[f] == 0;
    const ck_jpeg_desc &d = descs[f];
    if (live && ok) { // pass 1: column c
        const int16_t *cf = coef_base + ((size_t)f * coef_frame_blocks + (size_t)by * d.yblk_stride + bx) * 64;
        const int32_t *q = qts + (size_t)d.qt * 64;
        int64_t in[8], out[8];
        for (int r = 0; r < 8; r++) in[r] = (int64_t)((int32_t)cf[r * 8 + c] * q[r * 8 + c]); // DEQUANTIZE in int
        islow_1d(in, out);
        for (int r = 0; r < 8; r++) ws[g][r][c] = (int32_t)((out[r] + 1024) >> 11);      // DESCALE(., CONST_BITS - PASS1_BITS)
    }
    __syncthreads();
    if constexpr (O == CK_ORIENT_NONE) {
        if (!live) return;
        const int y = by * 8 + c;
        if (y >= h) return;
        uint8_t px[8];
        if (ok) { // pass 2: row c
            int64_t in[8], out[8];
            for (int k = 0; k < 8; k++) in[k] = ws[g][c][k];
            islow_1d(in, out);
            for (int k = 0; k < 8; k++) px[k] = range_limit((out[k] + (1 << 17)) >> 18); // DESCALE(., CONST_BITS + PASS1_BITS + 3)
        } else {
            for (int k = 0; k < 8; k++) px[k] = 0;
        }
        uint8_t *row = frames + (size_t)f * pitch + (size_t)y * stride + bx * 8;
        if (bx * 8 + 8 <= w) {
            uint64_t v = 0;
            for (int k = 0; k < 8; k++) v |= (uint64_t)px[k] << (8 * k);
            *reinterpret_cast<uint64_t *>(row) = v;
        } else {
            for (int k = 0; k < 8 && bx * 8 + k < w; k++) row[k] = px[k];
        }
    } else {
        // row c of the source block as two words, byte k of v = S[by*8+c][bx*8+k] (rows and columns past sw / sh are JPEG's padding
        // to whole MCUs: computed like the rest and cropped on the turned side)
        uint64_t v = 0;
        if (live && ok) { // pass 2: row c
            int64_t in[8], out[8];
            for (int k = 0; k < 8; k++) in[k] = ws[g][c][k];
            islow_1d(in, out);
            for (int k = 0; k < 8; k++) v |= (uint64_t)range_limit((out[k] + (1 << 17)) >> 18) << (8 * k);
        }
        int y, x0; // the lane's row of the turned block: out[y][x0 + j] = byte j of v, for the j with 0 <= x0 + j < W
        bool row_ok;
        if constexpr (O == CK_ORIENT_ROTATE_180) {
            v = __builtin_bswap64(v);
            y = h - 1 - (by * 8 + c);
            x0 = w - 8 - bx * 8;
            row_ok = live && y >= 0;
        } else {
            // 18 words per block: the eight rows of two words and a pad that spreads the blocks of a half-wave over the 32 banks
            // of ds_read_b32 (block g starts at bank 18 g mod 32: 0, 18, 4, 22 / 8, 26, 12, 30, each followed by its r*2 + {0, 1})
            __shared__ uint32_t tr[IDCT_BLOCKS][18];
            tr[g][c * 2] = (uint32_t)v;
            tr[g][c * 2 + 1] = (uint32_t)(v >> 32);
            __syncthreads();
            // lane c now takes source COLUMN c: byte r of t = S[by*8+r][bx*8+c]
            uint64_t t = 0;
            for (int r = 0; r < 8; r++) t |= (uint64_t)((tr[g][r * 2 + (c >> 2)] >> (8 * (c & 3))) & 0xFFu) << (8 * r);
            if constexpr (O == CK_ORIENT_CLOCKWISE) { // out[y][x] = S[sh-1-x][y]: row bx*8+c, columns sh-8-by*8 .., source rows descending
                v = __builtin_bswap64(t);
                y = bx * 8 + c;
                x0 = h - 8 - by * 8;
                row_ok = live && y < w;
            } else {                                  // out[y][x] = S[x][sw-1-y]: row sw-1-(bx*8+c), columns by*8 .., source rows ascending
                v = t;
                y = w - 1 - (bx * 8 + c);
                x0 = by * 8;
                row_ok = live && y >= 0;
            }
        }
        if (!row_ok) return;
        const int W = (O == CK_ORIENT_ROTATE_180) ? w : h; // the oriented width (its height bounds y above)
        uint8_t *row = frames + (size_t)f * pitch + (size_t)y * stride;
        if (x0 >= 0 && x0 + 8 <= W && (x0 & 7) == 0) {
            *reinterpret_cast<uint64_t *>(row + x0) = v;
        } else {
            for (int j = 0; j < 8; j++)
                if (x0 + j >= 0 && x0 + j < W) row[x0 + j] = (uint8_t)(v >> (8 * j));
        }
    }
}

// The chroma planes of the colour form: block m of component comp = 1, 2 is MCU m's, so the plane of a component is
// the MCU grid in blocks, cropped to cw x ch = ceil(sw / hs) x ceil(sh / vs) and never turned (the preview's sampler applies the
// index map).  The frames of a call differ in their sampling, so the grid covers the 1 x 1 case and a frame's own MCU count
// bounds its blocks.  Every store is to a pixel (x, y) of the frame's two planes with 0 <= x < cw and 0 <= y < ch.
__global__ void __launch_bounds__(IDCT_NT) k_jpeg_idct_chroma(const ck_jpeg_desc *__restrict__ descs, const int32_t *__restrict__ qts,
                                                              const int16_t *__restrict__ coef_base, size_t coef_frame_blocks,
                                                              const uint32_t *__restrict__ status, uint8_t *__restrict__ planes, int w, int h) {
    __shared__ int32_t ws[IDCT_BLOCKS][8][9];
    const int f = blockIdx.y, g = threadIdx.x >> 3, c = threadIdx.x & 7;
    const ck_jpeg_desc &d = descs[f];
    const bool ok = status[f] == 0 && d.bpm > 1;
    const uint32_t b = blockIdx.x * IDCT_BLOCKS + g;
    const bool live = ok && b < 2 * d.nmcu;
    const uint32_t comp = live && b >= d.nmcu ? 1u : 0u, m = live ? b - comp * d.nmcu : 0u;
    if (live) { // pass 1: column c
        const int16_t *cf = coef_base + ((size_t)f * coef_frame_blocks + c_block(d, m, comp + 1)) * 64;
        const int32_t *q = qts + (size_t)d.qtc[comp] * 64;
        int64_t in[8], out[8];
        for (int r = 0; r < 8; r++) in[r] = (int64_t)((int32_t)cf[r * 8 + c] * q[r * 8 + c]);
        islow_1d(in, out);
        for (int r = 0; r < 8; r++) ws[g][r][c] = (int32_t)((out[r] + 1024) >> 11);
    }
    __syncthreads();
    if (!live) return;
    const int vs = (int)(d.nyb / d.hs), cw = (w + (int)d.hs - 1) / (int)d.hs, ch = (h + vs - 1) / vs;
    const int by = (int)(m / d.mcux), bx = (int)(m - (uint32_t)by * d.mcux), y = by * 8 + c;
    if (y >= ch) return;
    int64_t in[8], out[8];
    for (int k = 0; k < 8; k++) in[k] = ws[g][c][k]; // pass 2: row c
    islow_1d(in, out);
    uint8_t *row = planes + d.plane_off + (size_t)comp * cw * ch + (size_t)y * cw + bx * 8;
    for (int k = 0; k < 8 && bx * 8 + k < cw; k++) row[k] = range_limit((out[k] + (1 << 17)) >> 18);
}

template <int O>
void launch_idct(hipStream_t s, int n, const ck_jpeg_desc *d_desc, const int32_t *d_qt, const ck_jpeg_ws &J, size_t coef_frame_blocks,
                 const ck_dev_image &dst, int sw, int sh) {
    const int nblk = ((sw + 7) / 8) * ((sh + 7) / 8);
    hipLaunchKernelGGL(k_jpeg_idct<O>, dim3((unsigned)((nblk + IDCT_BLOCKS - 1) / IDCT_BLOCKS), (unsigned)n), dim3(IDCT_NT), 0, s, d_desc, d_qt,
                       J.d_coef, coef_frame_blocks, J.d_status, const_cast<uint8_t *>(dst.p), dst.stride, dst.pitch, sw, sh);
}

} // namespace

int ck_launch_jpeg(const ck_jpeg_ws &J, hipStream_t s, int n, const ck_jpeg_desc *d_desc, const ck_jpeg_huff *d_huff, const int32_t *d_qt,
                   const uint8_t *d_raw, size_t coef_frame_blocks, const ck_dev_image &dst, int sw, int sh, int orientation, bool color) {
    if (color) {
        hipLaunchKernelGGL(k_jpeg_frame<true>, dim3((unsigned)n), dim3(NT), 0, s, d_desc, d_huff, d_raw, J.d_compact, J.d_int, J.d_sub, J.d_coef,
                           coef_frame_blocks, J.d_status);
        CK_HIP(hipGetLastError());
        const int nblk = 2 * ((sw + 7) / 8) * ((sh + 7) / 8); // two components at 1 x 1 sampling
        hipLaunchKernelGGL(k_jpeg_idct_chroma, dim3((unsigned)((nblk + IDCT_BLOCKS - 1) / IDCT_BLOCKS), (unsigned)n), dim3(IDCT_NT), 0, s, d_desc, d_qt,
                           J.d_coef, coef_frame_blocks, J.d_status, J.d_planes, sw, sh);
    } else {
        hipLaunchKernelGGL(k_jpeg_frame<false>, dim3((unsigned)n), dim3(NT), 0, s, d_desc, d_huff, d_raw, J.d_compact, J.d_int, J.d_sub, J.d_coef,
                           coef_frame_blocks, J.d_status);
    }
    CK_HIP(hipGetLastError());
    switch (orientation) {
    case CK_ORIENT_NONE: launch_idct<CK_ORIENT_NONE>(s, n, d_desc, d_qt, J, coef_frame_blocks, dst, sw, sh); break;
    case CK_ORIENT_CLOCKWISE: launch_idct<CK_ORIENT_CLOCKWISE>(s, n, d_desc, d_qt, J, coef_frame_blocks, dst, sw, sh); break;
    case CK_ORIENT_ROTATE_180: launch_idct<CK_ORIENT_ROTATE_180>(s, n, d_desc, d_qt, J, coef_frame_blocks, dst, sw, sh); break;
    case CK_ORIENT_COUNTERCLOCKWISE: launch_idct<CK_ORIENT_COUNTERCLOCKWISE>(s, n, d_desc, d_qt, J, coef_frame_blocks, dst, sw, sh); break;
    default: return CK_EINVAL;
    }
    CK_HIP(hipGetLastError());
    return CK_OK;
}
