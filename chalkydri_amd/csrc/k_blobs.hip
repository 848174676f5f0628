// Coloured game pieces, the device half: HSV classification of the oriented colour source into one bit plane per
// class, 3x3 morphology on the packed words, 8-connected components at run granularity, integer statistics, filter + rank + records.
// Every stage is data-parallel over the words of all planes of a call (a plane = one class of one frame); nothing comes back to the
// host between the stages.  The pixels are read through the colour preview's source accessors (ck_pv_source.h), the arithmetic is
// ck_blob_math.h's, which the host twin compiles too.
//
// Labelling.  The unit is a RUN: a maximal group of consecutive set bits inside one 32-bit word, named by the plane-local index
// y * 32 ww + x of its first pixel.  A word has at most 16 of them and finds them with ctz on registers.  Runs are joined by the
// lock-free union-find of Playne & Hawick (atomicMin on the larger root, retried until it sticks): with the word to the left when
// bit 0 and that word's bit 31 are set, and with every run of the row above that has a pixel in [s - 1, e + 1] (8-connectivity),
// which lies in at most three words.  The smaller index always stays the root, so a component's root is its seed.  No write is
// addressed by data: every index is that of a set bit inside the plane, so no mask can send a store out of bounds.
#include "ck_blobs.h"
#include "ck_pv_source.h"

namespace {

constexpr int BL_NT = 256;

struct Classes { ck_blob_class_t c[CK_BLOB_MAX_CLASSES]; };

template <bool YUV> __device__ constexpr bool is_ycc(const Raw<YUV> &) { return YUV; }
__device__ constexpr bool is_ycc(const Decoded &) { return true; }
__device__ constexpr bool is_ycc(const Planar &) { return true; }

// the RGB the classifier sees of oriented pixel (x, y) of frame F
template <class SRC>
__device__ __forceinline__ void blob_px(const SRC &s, const typename SRC::Frame &F, int x, int y, int *r, int *g, int *b) {
    int v[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const typename SRC::Lane L = s.lane(c);
        v[c] = s.pixel(F, s.term_x(L, x) + s.term_y(L, y), L, nullptr, 0);
    }
    if (is_ycc(s)) ckb_ycc_rgb(v[0], v[1], v[2], r, g, b);
    else { *r = v[0]; *g = v[1]; *b = v[2]; }
}

template <class SRC>
__device__ __forceinline__ void blob_rgb(const ck_blob_geom &g, const SRC &s, int n, const int32_t *frames, uint8_t *out) {
    const long t = (long)blockIdx.x * BL_NT + threadIdx.x;
    const long npx = (long)g.W * g.H;
    if (t >= npx * n) return;
    const int i = (int)(t / npx), q = (int)(t - i * npx), y = q / g.W, x = q - y * g.W;
    int r, gg, b;
    blob_px(s, s.frame(frames[i]), x, y, &r, &gg, &b);
    out[3 * t] = (uint8_t)r; out[3 * t + 1] = (uint8_t)gg; out[3 * t + 2] = (uint8_t)b;
}
template <bool YUV>
__global__ __launch_bounds__(BL_NT) void k_blob_rgb(ck_blob_geom g, ck_pv_csrc s, int n, const int32_t *frames, uint8_t *out) {
    blob_rgb(g, Raw<YUV>{s}, n, frames, out);
}
__global__ __launch_bounds__(BL_NT) void k_blob_prgb(ck_blob_geom g, ck_pv_psrc s, int n, const int32_t *frames, uint8_t *out) {
    blob_rgb(g, Planar{s}, n, frames, out);
}
__global__ __launch_bounds__(BL_NT) void k_blob_jrgb(ck_blob_geom g, ck_pv_jsrc s, int n, const int32_t *frames, uint8_t *out) {
    blob_rgb(g, Decoded{s}, n, frames, out);
}

// ---- threshold: a wave per row and up to MASK_CHUNKS groups of 64 of its pixels, a lane per pixel of a group; the wave's ballot
// is two words of every class's plane.  What depends on the row alone (the frame, the lanes' constants, the row's term of the
// address) is computed once per wave, and the groups are unrolled, so the loads of one overlap the arithmetic of another.
constexpr int MASK_CHUNKS = 4;
template <class SRC>
__device__ __forceinline__ void blob_mask(const ck_blob_geom &g, const SRC &s, const Classes &K, const int32_t *frames, uint32_t *bits) {
    const int y = blockIdx.y * 4 + threadIdx.y, i = blockIdx.z;
    if (y >= g.H) return; // (the whole wave)
    const typename SRC::Frame F = s.frame(frames[i]);
    const typename SRC::Lane L0 = s.lane(0), L1 = s.lane(1), L2 = s.lane(2);
    const int ty0 = s.term_y(L0, y), ty1 = s.term_y(L1, y), ty2 = s.term_y(L2, y);
#pragma unroll
    for (int k = 0; k < MASK_CHUNKS; k++) {
        const int xb = (blockIdx.x * MASK_CHUNKS + k) * 64;
        if (xb >= g.W) break; // (the whole wave)
        const int x = xb + threadIdx.x;
        const bool in = x < g.W;
        int r = 0, gg = 0, b = 0;
        if (in) {
            const int v0 = s.pixel(F, s.term_x(L0, x) + ty0, L0, nullptr, 0), v1 = s.pixel(F, s.term_x(L1, x) + ty1, L1, nullptr, 0),
                      v2 = s.pixel(F, s.term_x(L2, x) + ty2, L2, nullptr, 0);
            if (is_ycc(s)) ckb_ycc_rgb(v0, v1, v2, &r, &gg, &b);
            else { r = v0; gg = v1; b = v2; }
        }
#pragma unroll
        for (int c = 0; c < CK_BLOB_MAX_CLASSES; c++) {
            if (c >= g.nc) break;
            const unsigned long long m = __ballot(in && ckb_class_pass(&K.c[c], r, gg, b));
            if (threadIdx.x == 0) {
                uint32_t *row = bits + (((size_t)i * g.nc + c) * g.H + y) * g.ww;
                const int w0 = xb >> 5; // w0 < ww because xb < W
                row[w0] = (uint32_t)m;
                if (w0 + 1 < g.ww) row[w0 + 1] = (uint32_t)(m >> 32);
            }
        }
    }
}
template <bool YUV>
__global__ __launch_bounds__(BL_NT) void k_blob_mask(ck_blob_geom g, ck_pv_csrc s, Classes K, const int32_t *frames, uint32_t *bits) {
    blob_mask(g, Raw<YUV>{s}, K, frames, bits);
}
__global__ __launch_bounds__(BL_NT) void k_blob_pmask(ck_blob_geom g, ck_pv_psrc s, Classes K, const int32_t *frames, uint32_t *bits) {
    blob_mask(g, Planar{s}, K, frames, bits);
}
__global__ __launch_bounds__(BL_NT) void k_blob_jmask(ck_blob_geom g, ck_pv_jsrc s, Classes K, const int32_t *frames, uint32_t *bits) {
    blob_mask(g, Decoded{s}, K, frames, bits);
}

// a lane's word: plane p, row y, word wx of `total` = planes * H * ww
struct WordAt { int p, y, wx; bool ok; };
__device__ __forceinline__ WordAt word_at(const ck_blob_geom &g, long total) {
    const long t = (long)blockIdx.x * BL_NT + threadIdx.x;
    WordAt a = {0, 0, 0, t < total};
    if (a.ok) { a.wx = (int)(t % g.ww); const long q = t / g.ww; a.y = (int)(q % g.H); a.p = (int)(q / g.H); }
    return a;
}

// ---- morphology: one iteration of the 3x3 square, a lane per word; outside the frame is background ---------------------------
__global__ __launch_bounds__(BL_NT) void k_blob_morph(ck_blob_geom g, long total, int dilate, const uint32_t *in, uint32_t *out) {
    const WordAt a = word_at(g, total);
    if (!a.ok) return;
    const uint32_t *P = in + (size_t)a.p * g.H * g.ww;
    uint32_t acc = dilate ? 0u : ~0u;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
        const int yy = a.y + dy;
        uint32_t v = 0;
        if (yy >= 0 && yy < g.H) {
            const uint32_t *row = P + (size_t)yy * g.ww;
            v = ckb_row3(a.wx > 0 ? row[a.wx - 1] : 0u, row[a.wx], a.wx + 1 < g.ww ? row[a.wx + 1] : 0u, dilate);
        }
        acc = dilate ? (acc | v) : (acc & v);
    }
    if (a.wx == g.ww - 1 && (g.W & 31)) acc &= (1u << (g.W & 31)) - 1u; // the bits at x >= W stay 0
    out[((size_t)a.p * g.H + a.y) * g.ww + a.wx] = acc;
}

// ---- runs of a word ---------------------------------------------------------------------------------------------------------------
// the first bit of the run of w that holds bit b (which is set)
__device__ __forceinline__ int run_start(uint32_t w, int b) {
    const uint32_t z = ~w & ((1u << b) - 1u);
    return z ? 32 - __clz(z) : 0;
}
// the length of the run of w that starts at bit s
__device__ __forceinline__ int run_len(uint32_t w, int s) {
    const uint32_t nt = ~(w >> s);
    return nt ? __ffs(nt) - 1 : 32; // (w >> s shifts zeros in: nt is 0 only for s = 0 and a full word)
}
__device__ __forceinline__ uint32_t run_bits(int s, int len) { return len >= 32 ? ~0u : ((1u << len) - 1u) << s; }

__device__ __forceinline__ uint32_t uf_find(uint32_t *p, uint32_t i) {
    for (;;) {
        const uint32_t n = __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n == i) return i;
        i = n;
    }
}
__device__ __forceinline__ void uf_unite(uint32_t *p, uint32_t a, uint32_t b) {
    for (;;) {
        a = uf_find(p, a); b = uf_find(p, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; } // a: the larger root, which takes b as its parent
        const uint32_t old = atomicMin(p + a, b);
        if (old == a) return;
        a = old; // somebody else linked a in the meantime: join what it was linked to
    }
}

__global__ __launch_bounds__(BL_NT) void k_blob_init(ck_blob_geom g, long total, const uint32_t *bits, uint32_t *parent, uint32_t *area) {
    const WordAt a = word_at(g, total);
    if (!a.ok) return;
    const uint32_t w = bits[((size_t)a.p * g.H + a.y) * g.ww + a.wx];
    const size_t base = (size_t)a.p * g.H * g.ww * 32;
    const uint32_t at = (uint32_t)(a.y * g.ww + a.wx) * 32u;
    for (uint32_t m = w & ~(w << 1); m; m &= m - 1) { // the first bits of the runs
        const uint32_t i = at + (uint32_t)(__ffs(m) - 1);
        parent[base + i] = i;
        area[base + i] = 0;
    }
}

__global__ __launch_bounds__(BL_NT) void k_blob_merge(ck_blob_geom g, long total, const uint32_t *bits, uint32_t *parent) {
    const WordAt a = word_at(g, total);
    if (!a.ok) return;
    const uint32_t *row = bits + ((size_t)a.p * g.H + a.y) * g.ww;
    const uint32_t w = row[a.wx];
    if (!w) return;
    uint32_t *P = parent + (size_t)a.p * g.H * g.ww * 32;
    const uint32_t at = (uint32_t)(a.y * g.ww + a.wx) * 32u;
    if ((w & 1u) && a.wx > 0) {
        const uint32_t l = row[a.wx - 1];
        if (l >> 31) uf_unite(P, at, at - 32u + (uint32_t)run_start(l, 31));
    }
    if (a.y == 0) return;
    const uint32_t *up = row - g.ww;
    const uint32_t u0 = up[a.wx], ul = a.wx > 0 ? up[a.wx - 1] : 0u, ur = a.wx + 1 < g.ww ? up[a.wx + 1] : 0u;
    if (!(u0 | (ul >> 31) | (ur & 1u))) return;
    const uint32_t uat = at - (uint32_t)g.ww * 32u;
    for (uint32_t m = w; m;) {
        const int s = __ffs(m) - 1, len = run_len(w, s), e = s + len - 1;
        m &= ~run_bits(s, len);
        const uint32_t me = at + (uint32_t)s;
        if (s == 0 && (ul >> 31)) uf_unite(P, me, uat - 32u + (uint32_t)run_start(ul, 31));
        if (e == 31 && (ur & 1u)) uf_unite(P, me, uat + 32u);
        // the bits s - 1 .. e + 1 of the word above, run by run
        const int lo = s > 0 ? s - 1 : 0, hi = e < 31 ? e + 1 : 31;
        for (uint32_t q = u0 & run_bits(lo, hi - lo + 1); q;) {
            const int b = __ffs(q) - 1, rs = run_start(u0, b);
            q &= ~run_bits(rs, run_len(u0, rs));
            uf_unite(P, me, uat + (uint32_t)rs);
        }
    }
}

// every run's parent becomes its root, and the root's area grows by the run's length
__global__ __launch_bounds__(BL_NT) void k_blob_flatten(ck_blob_geom g, long total, const uint32_t *bits, uint32_t *parent, uint32_t *area) {
    const WordAt a = word_at(g, total);
    if (!a.ok) return;
    const uint32_t w = bits[((size_t)a.p * g.H + a.y) * g.ww + a.wx];
    const size_t base = (size_t)a.p * g.H * g.ww * 32;
    const uint32_t at = (uint32_t)(a.y * g.ww + a.wx) * 32u;
    for (uint32_t m = w; m;) {
        const int s = __ffs(m) - 1, len = run_len(w, s);
        m &= ~run_bits(s, len);
        const uint32_t r = uf_find(parent + base, at + (uint32_t)s);
        // (a root's own entry is never rewritten here, so the finds of other lanes still end at it)
        if (r != at + (uint32_t)s) __hip_atomic_store(parent + base + at + s, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        atomicAdd(area + base + r, (uint32_t)len);
    }
}

// the roots of min_area pixels and more take a slot each; area[root] becomes slot | 2^31, or ~0 for a root without one
__global__ __launch_bounds__(BL_NT) void k_blob_slots(ck_blob_geom g, long total, Classes K, const uint32_t *bits, const uint32_t *parent,
                                                      uint32_t *area, uint32_t *nslot, ckb_comp *comps) {
    const WordAt a = word_at(g, total);
    if (!a.ok) return;
    const uint32_t w = bits[((size_t)a.p * g.H + a.y) * g.ww + a.wx];
    const size_t base = (size_t)a.p * g.H * g.ww * 32;
    const uint32_t at = (uint32_t)(a.y * g.ww + a.wx) * 32u;
    const int c = a.p % g.nc;
    const int min_area = c == 0 ? K.c[0].min_area : (c == 1 ? K.c[1].min_area : (c == 2 ? K.c[2].min_area : K.c[3].min_area));
    for (uint32_t m = w & ~(w << 1); m; m &= m - 1) {
        const int s = __ffs(m) - 1;
        const uint32_t i = at + (uint32_t)s;
        if (parent[base + i] != i) continue;
        const uint32_t n = area[base + i];
        uint32_t tag = ~0u;
        if ((int)n >= min_area) {
            const uint32_t slot = atomicAdd(nslot + a.p, 1u);
            if (slot < (uint32_t)g.maxc) {
                ckb_comp k;
                k.area = (int32_t)n; k.seed = a.y * g.W + (a.wx * 32 + s);
                k.x0 = g.W; k.y0 = g.H; k.x1 = -1; k.y1 = -1;
                k.sx = 0; k.sy = 0; k.sxx = 0; k.sxy = 0; k.syy = 0;
                comps[(size_t)a.p * g.maxc + slot] = k;
                tag = slot | 0x80000000u;
            }
        }
        area[base + i] = tag;
    }
}

// The wide sums, a run at a time in closed form; integer atomics only, so the sums do not depend on the order.  The runs of a piece
// lie in neighbouring words, that is in neighbouring lanes: the lanes of a wave whose (first) run belongs to the same component add
// up across the wave first, and one lane issues the component's nine atomics for all of them.  After SUM_ROUNDS components a wave
// stops sorting itself out (a mask of specks has a component per lane) and the lanes left add for themselves, as every further run of
// a word does.
constexpr int SUM_ROUNDS = 4;
struct RunSums { int x0, x1, y0, y1; long long sx, sy, sxx, sxy, syy; };
__device__ __forceinline__ void sums_add(ckb_comp *k, const RunSums &v) {
    atomicMin(&k->x0, v.x0); atomicMax(&k->x1, v.x1);
    atomicMin(&k->y0, v.y0); atomicMax(&k->y1, v.y1);
    atomicAdd(reinterpret_cast<unsigned long long *>(&k->sx), (unsigned long long)v.sx);
    atomicAdd(reinterpret_cast<unsigned long long *>(&k->sy), (unsigned long long)v.sy);
    atomicAdd(reinterpret_cast<unsigned long long *>(&k->sxx), (unsigned long long)v.sxx);
    atomicAdd(reinterpret_cast<unsigned long long *>(&k->sxy), (unsigned long long)v.sxy);
    atomicAdd(reinterpret_cast<unsigned long long *>(&k->syy), (unsigned long long)v.syy);
}
template <class T, class Op>
__device__ __forceinline__ T wave_all(T v, Op op) { // every lane of the wave takes part
#pragma unroll
    for (int o = 32; o; o >>= 1) v = op(v, __shfl_xor(v, o));
    return v;
}
__global__ __launch_bounds__(BL_NT) void k_blob_sums(ck_blob_geom g, long total, const uint32_t *bits, const uint32_t *parent,
                                                     const uint32_t *area, ckb_comp *comps) {
    const WordAt a = word_at(g, total); // (no early return: the wave operations below need every lane)
    const uint32_t w = a.ok ? bits[((size_t)a.p * g.H + a.y) * g.ww + a.wx] : 0u;
    const size_t base = (size_t)a.p * g.H * g.ww * 32;
    const uint32_t at = (uint32_t)(a.y * g.ww + a.wx) * 32u;
    ckb_comp *mine = nullptr;
    RunSums v = {0x7FFFFFFF, -1, 0x7FFFFFFF, -1, 0, 0, 0, 0, 0};
    for (uint32_t m = w; m;) {
        const int s = __ffs(m) - 1, len = run_len(w, s);
        m &= ~run_bits(s, len);
        const uint32_t tag = area[base + parent[base + at + s]];
        if (tag == ~0u) continue;
        ckb_comp *k = comps + (size_t)a.p * g.maxc + (tag & 0x7FFFFFFFu);
        const long long xs = a.wx * 32 + s, xe = xs + len - 1, y = a.y, L = len;
        const long long sx = (xs + xe) * L / 2;                                               // sum of xs .. xe
        const long long sxx = (xe * (xe + 1) * (2 * xe + 1) - (xs - 1) * xs * (2 * xs - 1)) / 6; // sum of their squares
        const RunSums r = {(int)xs, (int)xe, (int)y, (int)y, sx, y * L, sxx, y * sx, y * y * L};
        if (!mine) { mine = k; v = r; }
        else sums_add(k, r);
    }
    const auto imin = [](int p, int q) { return p < q ? p : q; };
    const auto imax = [](int p, int q) { return p > q ? p : q; };
    const auto ladd = [](long long p, long long q) { return p + q; };
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(mine != nullptr);
    for (int round = 0; todo && round < SUM_ROUNDS; round++) { // (todo is the same in every lane: the loop is the whole wave's)
        const int leader = __ffsll((long long)todo) - 1;
        const unsigned long long key = __shfl((unsigned long long)(uintptr_t)mine, leader);
        const bool in = mine != nullptr && (unsigned long long)(uintptr_t)mine == key;
        RunSums t;
        t.x0 = wave_all(in ? v.x0 : 0x7FFFFFFF, imin); t.x1 = wave_all(in ? v.x1 : -1, imax);
        t.y0 = wave_all(in ? v.y0 : 0x7FFFFFFF, imin); t.y1 = wave_all(in ? v.y1 : -1, imax);
        t.sx = wave_all(in ? v.sx : 0ll, ladd); t.sy = wave_all(in ? v.sy : 0ll, ladd); t.sxx = wave_all(in ? v.sxx : 0ll, ladd);
        t.sxy = wave_all(in ? v.sxy : 0ll, ladd); t.syy = wave_all(in ? v.syy : 0ll, ladd);
        if (lane == leader) sums_add(mine, t);
        if (in) mine = nullptr;
        todo &= ~__ballot(in);
    }
    if (mine) sums_add(mine, v);
}

// ---- finalize: one workgroup per plane: capacity rule, filter, rank by (area, seed), records -------------------------------------
__global__ __launch_bounds__(BL_NT) void k_blob_final(ck_blob_geom g, Classes K, ckb_geo geo, int max_targets, const uint32_t *nslot,
                                                      const ckb_comp *comps, uint32_t *list, ck_blob_t *out, int32_t *counts, uint32_t *status) {
    __shared__ uint32_t n_pass;
    const int p = blockIdx.x, c = p % g.nc, f = p / g.nc;
    const uint32_t ns = nslot[p];
    if (ns > (uint32_t)g.maxc) { // no targets rather than an arbitrary subset
        if (threadIdx.x == 0) { counts[p] = 0; atomicOr(status + f, (uint32_t)CK_BLOB_OVERFLOW); }
        return;
    }
    ck_blob_class_t k;
    if (c == 0) k = K.c[0]; else if (c == 1) k = K.c[1]; else if (c == 2) k = K.c[2]; else k = K.c[3];
    if (threadIdx.x == 0) n_pass = 0;
    __syncthreads();
    const ckb_comp *C = comps + (size_t)p * g.maxc;
    uint32_t *Lst = list + (size_t)p * g.maxc;
    for (uint32_t j = threadIdx.x; j < ns; j += BL_NT) {
        const ckb_comp v = C[j];
        if (ckb_filter(&k, &v)) Lst[atomicAdd(&n_pass, 1u)] = j;
    }
    __syncthreads();
    const uint32_t np = n_pass;
    uint32_t nw = np < (uint32_t)max_targets ? np : (uint32_t)max_targets;
    if ((uint32_t)g.cap < nw) nw = (uint32_t)g.cap;
    if (threadIdx.x == 0) {
        counts[p] = (int32_t)np;
        if (nw < np) atomicOr(status + f, (uint32_t)CK_BLOB_TRUNCATED);
    }
    // seeds are unique, so the ranks are a permutation whatever order the list came in
    for (uint32_t a = threadIdx.x; a < np; a += BL_NT) {
        const ckb_comp v = C[Lst[a]];
        uint32_t rank = 0;
        for (uint32_t b = 0; b < np; b++) {
            const ckb_comp *o = C + Lst[b];
            rank += ckb_before(o->area, o->seed, v.area, v.seed) ? 1u : 0u;
        }
        if (rank < nw) ckb_record(&v, c, k.ground_z, g.W, g.H, &geo, out + (size_t)p * g.cap + rank);
    }
}

inline unsigned blocks_of(long total) { return (unsigned)((total + BL_NT - 1) / BL_NT); }

} // namespace

int ck_launch_blob_rgb(ck_handle *h, const ck_blob_geom &g, const ck_pv_src &src, int n, uint8_t *d_out) {
    ck_blob_ws &P = *h->blobs;
    const dim3 grid(blocks_of((long)g.W * g.H * n));
    if (src.jpeg) hipLaunchKernelGGL(k_blob_jrgb, grid, dim3(BL_NT), 0, h->stream, g, *src.jpeg, n, P.d_frames, d_out);
    else if (src.planar) hipLaunchKernelGGL(k_blob_prgb, grid, dim3(BL_NT), 0, h->stream, g, *src.planar, n, P.d_frames, d_out);
    else if (src.raw->bpp == 2) hipLaunchKernelGGL(k_blob_rgb<true>, grid, dim3(BL_NT), 0, h->stream, g, *src.raw, n, P.d_frames, d_out);
    else hipLaunchKernelGGL(k_blob_rgb<false>, grid, dim3(BL_NT), 0, h->stream, g, *src.raw, n, P.d_frames, d_out);
    CK_HIP(hipGetLastError());
    return CK_OK;
}

static Classes classes_of(const ck_blob_params_t &pp) {
    Classes K = {};
    for (int c = 0; c < pp.n_classes; c++) K.c[c] = pp.cls[c];
    return K;
}

int ck_launch_blob_mask(ck_handle *h, const ck_blob_geom &g, const ck_blob_params_t &pp, const ck_pv_src &src, int n, int stage, int *side) {
    ck_blob_ws &P = *h->blobs;
    const Classes K = classes_of(pp);
    const long total = (long)n * g.nc * g.H * g.ww;
    uint32_t *b[2] = {P.d_bits.p, P.d_bits.p + total};
    const dim3 grid((g.W + 64 * MASK_CHUNKS - 1) / (64 * MASK_CHUNKS), (g.H + 3) / 4, n), block(64, 4);
    if (src.jpeg) hipLaunchKernelGGL(k_blob_jmask, grid, block, 0, h->stream, g, *src.jpeg, K, P.d_frames, b[0]);
    else if (src.planar) hipLaunchKernelGGL(k_blob_pmask, grid, block, 0, h->stream, g, *src.planar, K, P.d_frames, b[0]);
    else if (src.raw->bpp == 2) hipLaunchKernelGGL(k_blob_mask<true>, grid, block, 0, h->stream, g, *src.raw, K, P.d_frames, b[0]);
    else hipLaunchKernelGGL(k_blob_mask<false>, grid, block, 0, h->stream, g, *src.raw, K, P.d_frames, b[0]);
    CK_HIP(hipGetLastError());
    int at = 0;
    for (int it = 0; stage == 1 && it < pp.erode + pp.dilate; it++, at ^= 1) {
        hipLaunchKernelGGL(k_blob_morph, dim3(blocks_of(total)), dim3(BL_NT), 0, h->stream, g, total, it >= pp.erode ? 1 : 0, b[at], b[at ^ 1]);
        CK_HIP(hipGetLastError());
    }
    *side = at;
    return CK_OK;
}

int ck_launch_blob_components(ck_handle *h, const ck_blob_geom &g, const ck_blob_params_t &pp, const ckb_geo &geo, int n, int side) {
    ck_blob_ws &P = *h->blobs;
    const Classes K = classes_of(pp);
    const int planes = n * g.nc;
    const long total = (long)planes * g.H * g.ww;
    const uint32_t *bits = P.d_bits.p + (side ? total : 0);
    const dim3 grid(blocks_of(total)), block(BL_NT);
    CK_HIP(hipMemsetAsync(P.d_nslot, 0, sizeof(uint32_t) * (size_t)planes, h->stream));
    CK_HIP(hipMemsetAsync(P.d_status, 0, sizeof(uint32_t) * (size_t)n, h->stream));
    if (g.cap) CK_HIP(hipMemsetAsync(P.d_out, 0, sizeof(ck_blob_t) * (size_t)planes * g.cap, h->stream));
    hipLaunchKernelGGL(k_blob_init, grid, block, 0, h->stream, g, total, bits, P.d_parent.p, P.d_area.p);
    hipLaunchKernelGGL(k_blob_merge, grid, block, 0, h->stream, g, total, bits, P.d_parent.p);
    hipLaunchKernelGGL(k_blob_flatten, grid, block, 0, h->stream, g, total, bits, P.d_parent.p, P.d_area.p);
    hipLaunchKernelGGL(k_blob_slots, grid, block, 0, h->stream, g, total, K, bits, P.d_parent.p, P.d_area.p, P.d_nslot.p, P.d_comps.p);
    hipLaunchKernelGGL(k_blob_sums, grid, block, 0, h->stream, g, total, bits, P.d_parent.p, P.d_area.p, P.d_comps.p);
    hipLaunchKernelGGL(k_blob_final, dim3(planes), block, 0, h->stream, g, K, geo, pp.max_targets, P.d_nslot.p, P.d_comps.p, P.d_list.p,
                       P.d_out.p, P.d_counts.p, P.d_status.p);
    CK_HIP(hipGetLastError());
    return CK_OK;
}
