// k_clusters.hip — gradient clusters: one point per 8-neighbour pair of opposite colour whose components both
// have >= min_component_px pixels, grouped by the unordered pair of component ids.
//
// Replaces the "gradient clusters" stage of the external AprilTag-3 detector (crates/apriltags/src/lib.rs:301);
// the hash-map-of-component-pairs formulation is the one CAT was converging on (stub `ClusterHash`, `u64hash_2`
// and the 0.2*w*h cluster map at crates/chalkydri-apriltags/src/lib.rs:115-124,551-557).
//
//   k_emit2    one workgroup per 16x64 pixel tile: resolves every pixel's component once into LDS (one extra
//              hop for ring-touching components, see ck_internal.h), aggregates the tile's points per cluster key
//              in an LDS hash table, then makes ONE global insert + one add per (tile, key), writes the tile's points to
//              the temp array as one contiguous run per key (4-byte packed points) and one run record per key.
//              The two points a straight edge emits at one half-pixel (diagonal twins) are stored as ONE word
//              (ck_point.h), so a cluster has a logical count (the oracle's) and a physical one (words stored).
//   k_scan     one workgroup per frame: prefix sums over the frame's hash table -> cluster table + point offsets
//              (clusters outside [min_cluster_pixels, max_cluster_points], by their logical count, are dropped here).
//   k_scatter  one wave per run: temp array -> points grouped by cluster.
#include "ck_internal.h"
#include "ck_emit_row.h"
#include "ck_emit_stage.h"

namespace {

constexpr int NT = 256;
constexpr int ETW = 64, ETH = 16;         // emit tile
constexpr int LW = ETW + 2, LH = ETH + 1; // staged region: one column each side, one row below
constexpr int LHT = 512;                  // LDS hash slots (= 2 * NT: the reservation pass gives every thread two)
constexpr uint32_t SKIP = 0xFFFFFFFFu;
constexpr unsigned SCATTER_WGS = 32;      // k_scatter<64>: workgroups per frame

__device__ __forceinline__ uint32_t key_hash(unsigned long long k) {
    uint32_t x = (uint32_t)((k >> 32) ^ k); // u64hash_2 of the reference's stub
    x *= 2654435761u;
    return x ^ (x >> 15);
}

struct EmitArgs {
    const uint8_t *thresh;
    const ck_label_t *labels;
    const uint32_t *groot, *gsize; // slot tables of the ring-touching components (k_ccl.hip: k_fmerge)
    size_t slots;
    int w, h, tiles_x, tiles_y, min_comp;
    int ccl_tiles_x; // tiles per row of the segmentation stage (the label words are local to its 32 x 128 tiles)
    int stop_after; // diagnostics (CK_EMIT_STOP_AFTER): 0 staging only, 1 +count, 2 +reserve; 99 = everything
    int twins;      // k_emit2 merges diagonal twin points (diagnostics: CK_EMIT_TWINS=0 emits every point on its own)
    int stage4;     // k_emit2 stages its tile in aligned groups of four pixels where the frame allows it (diagnostics: CK_EMIT_STAGE4=0 never)
    ck_stage_ws ws;
};

// A barrier that orders LDS traffic only: __syncthreads() carries a workgroup-scope fence, i.e. a wait for EVERY outstanding memory
// operation — the barrier before the point writes would wait for the acknowledgement of the cluster-count adds nobody reads.
// Nothing a workgroup of k_emit2 writes to global memory is read by it again.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---- k_emit2 (round 4): the same function as k_emit, re-cut around what the counters said about it ---------------------------------
// (k_emit is the round-1..3 kernel, since removed: git history holds it.)
// k_emit on the bench batch (rocprofv3 --pmc): 1 226 vector, 1 128 scalar and 171 LDS instructions per wave; by phase (stop-after knob)
// staging 0.5 ms · count pass 1.16 · reservation 0.44 · point writes 0.35.  Every pixel of the count pass re-read its centre and four
// neighbours (ten LDS reads: threshold byte and root each) before it probed.  Here a staged pixel is ONE word — the frame pixel of its
// component's root | a colour bit (the colour test and the gradient sign come from it: the threshold bytes are not staged) — and a
// thread reads the 5 x 3 words around its four pixels ONCE (15 LDS reads instead of 40) and works on them from registers; the staging
// loads are branch-free (clamped addresses, masked results).
// With frames dealt to XCDs (a frame's tiles and slot tables in one L2: -0.11 ms) and a thread remembering its last key's place (the
// pixel below often continues the same boundary: -0.05 ms) the clusters stage takes 3.35 ms against k_emit's 3.50 (same box).  What the
// count pass spends its 1.2 ms on, by ablation: the key probe (64-bit read, compare-and-swap on an empty slot, the divergent loop
// around them) 0.63 ms, the counting add 0.08, reads and arithmetic 0.45.
// The count pass's per-pixel predicates were 794 lane-mask instructions on the scalar unit, the fuller issue port of the kernel (1 242
// scalar against 1 389 vector instructions per wave); they are now bits of one vector register per pixel row that index a table of
// the row's leaders (ck_emit_row.h), and the probe-and-add block runs once per leader: 580 scalar + 1 300 vector instructions per
// wave, count pass 1.36 -> 0.85 ms, kernel 2.58 -> 2.25 ms.
// The point writes read ONE LDS word per point and make one test: pass 2 marks the run start of a key without a place in the frame's
// table (NO_RUN, bit 31), which puts its points past point_cap; the table of places (2 KB of LDS) is gone: write pass and run
// records 251 + 212 -> 235 vector + 145 scalar and 36 -> 18 LDS instructions (static), -0.15 ms.  When the frame's width is a multiple
// of four the tile is staged in aligned groups of four pixels (ck_emit_stage.h, k_emit2<true>): staging 292 + 292 -> 197 + 240
// (static, the two waves with a second round), -0.09 ms on top (by itself, on the earlier write pass, it was inside the noise).
// Tried on the way and measured slower (1280 x 800 x 256, clusters stage, same box; k_emit: 3.51-3.56 ms):
//  * the count and write passes as straight-line code over all 16 candidate slots of a thread (a slot without a point counts 0 into
//    a per-lane dummy entry) and the tile's points ordered in LDS and copied out in one piece: fewer scalar instructions, but 32 slot
//    reads / adds per thread instead of the 7 its 3.5 real keys need, and 2.6 x the bank conflicts: 4.19 ms;
//  * ring-touching components keyed by their SLOT (CCL tile, tile-local id) in the tile's table and resolved to the frame-level root
//    once per key in the reservation pass, instead of two gathers per staged pixel: staging 0.76 -> 0.49 ms, but a component that is
//    one piece in the frame is several pieces inside a 32 x 128 tile (the white giant component of dense noise above all), so every
//    black blob beside two of its pieces became two keys, two runs, two inserts: count pass 1.18 -> 1.75 ms, 4.05 ms in all.
constexpr uint32_t ID_WHITE = 0x40000000u, ID_VALUE = 0x3FFFFFFFu; // a staged pixel: frame pixel of its root (< 2^24) | colour
static_assert(ID_WHITE == CK_PT_TWIN_SIGN, "a twin's sign is its white neighbour's colour bit, taken as it stands");
constexpr int SR_PAD = ((LH * LW + NT - 1) / NT) * NT; // ids: every thread stores SPT of them unconditionally
static_assert(SKIP == CK_ER_SKIP && ID_WHITE == CK_ER_WHITE, "ck_emit_row.h speaks of the staged words of this kernel");
// the row table (ck_emit_row.h), generated at compile time; every workgroup copies its 4 KB into LDS (one 16-byte load per thread,
// after the staging loads: issued before them it holds four registers across the kernel's register peak): with it a workgroup holds
// 17 460 of the 20 480 bytes that eight of them leave each other
__device__ const ck_emit_row_table g_emit_rows = ck_make_emit_row_table();
static_assert(CK_ER_ROWS == 4 * NT, "one uint4 of the row table per thread");
static_assert(CK_ES_NT == NT && CK_ES_TW == ETW && CK_ES_TH == ETH && CK_ES_LW == LW && CK_ES_LH == LH && CK_ES_WORDS <= SR_PAD, "ck_emit_stage.h speaks of this kernel's tile");
static_assert(CK_ES_CCL_TW == CK_TW && CK_ES_CCL_TH == CK_TH && CK_ES_RING_CAP == CK_RING_CAP && CK_ES_LBL_BORDER == CK_LBL_BORDER && CK_ES_LBL_SMALL == CK_LBL_SMALL &&
              CK_ES_LBL_ID_MASK == CK_LBL_ID_MASK && CK_ES_SKIP == SKIP && CK_ES_WHITE == ID_WHITE, "... and of the label words of ck_internal.h");

// G4: the tile is staged in aligned groups of four pixels (ck_emit_stage.h; the width is a multiple of four and the buffers are
// aligned: ck_launch_clusters decides for the whole launch).  Without it: every pixel on its own, for any width.
template <bool G4>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_num_sgpr(80), amdgpu_waves_per_eu(8))) void k_emit2(EmitArgs a, int xcd_map, int n_frames) {
    __shared__ __attribute__((aligned(16))) uint32_t sRaw[SR_PAD + LHT * 2 + LHT];
    __shared__ uint32_t sTBase[LHT];
    __shared__ uint32_t sWave[NT / 64 + 1], sRunW[NT / 64 + 1];
    __shared__ __attribute__((aligned(16))) uint32_t sRow[CK_ER_ROWS];
    uint32_t *sR = sRaw;                                                             // [LH][LW] ids
    unsigned long long *sKey = reinterpret_cast<unsigned long long *>(sRaw + SR_PAD); // [LHT]
    uint32_t *sCnt = sRaw + SR_PAD + LHT * 2;                                         // [LHT]
    const int tid = threadIdx.x;
    const int tiles = a.tiles_x * a.tiles_y;
    int frame, tile;
    if (xcd_map) { // workgroups b and b + 8 share an XCD: a frame's tiles (and its slot tables) stay in one L2
        const int x = blockIdx.x & 7, j = blockIdx.x >> 3;
        frame = (j / tiles) * 8 + x; tile = j % tiles;
        if (frame >= n_frames) return;
    } else { frame = blockIdx.x / tiles; tile = blockIdx.x - frame * tiles; }
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int x0 = tx * ETW, y0 = ty * ETH;
    const int w = a.w, h = a.h;
    const size_t npix = (size_t)w * h;
    const uint8_t *T = a.thresh + (size_t)frame * npix;
    const ck_label_t *L = a.labels + (size_t)frame * npix;
    const uint32_t *GR = a.groot + (size_t)frame * a.slots, *GS = a.gsize + (size_t)frame * a.slots;
    const ck_stage_ws &ws = a.ws;
    unsigned long long *gkeys = ws.d_ht_keys + (size_t)frame * ws.ht_size;
    unsigned long long *gcount = ws.d_ht_count + (size_t)frame * ws.ht_size;
    uint32_t *counters = ws.d_counters + (size_t)frame * CK_CNT_STRIDE;
    ck_packed_point *tmp = ws.d_tmp + (size_t)frame * ws.ext_cap;
    ck_run *runs = ws.d_runs + (size_t)frame * ws.run_cap;

    for (int i = tid; i < LHT; i += NT) { sKey[i] = 0ull; sCnt[i] = 0; }
    if constexpr (G4) {
        // staging in groups (ck_emit_stage.h): one dword of threshold bytes and one 8-byte word of labels per four pixels, the tile
        // terms of slot and root once per group, one 16-byte LDS write.  Round 0: every thread one group of the tile's own pixels;
        // round 1: the bottom halo row and the two halo columns, 98 single pixels, the first two waves' — the other two skip it on
        // a scalar.  A wave has both rounds' loads in flight together, then both rounds' gathers.
        // (every address is a uniform base + a 32-bit byte offset, which the load takes as it is: a frame's labels and a frame's slot
        // tables are far below 4 GiB)
        auto at = [](const void *base, uint32_t bytes) { return reinterpret_cast<const char *>(base) + bytes; };
        auto gather = [&](uint32_t slot, uint32_t &hop, uint32_t &csz) {
            hop = *reinterpret_cast<const uint32_t *>(at(GR, slot * 4u)); csz = *reinterpret_cast<const uint32_t *>(at(GS, slot * 4u));
        };
        const bool round1 = __builtin_amdgcn_readfirstlane(tid >> 6) < CK_ES_ROUND1_WAVES;
        const ck_es_item it0 = ck_es_round0(tid, x0, y0, w, h);
        ck_es_item it1 = it0;
        uint32_t lab[4], tv[4], hop[4], csz[4], lab1 = 0u, tv1 = 0u, hop1 = 0u, csz1 = 0u;
        {
            const uint32_t p = (uint32_t)it0.cy * (uint32_t)w + (uint32_t)it0.cx; // (a multiple of four)
            const uint32_t t4 = *reinterpret_cast<const uint32_t *>(at(T, p));
            const uint2 l4 = *reinterpret_cast<const uint2 *>(at(L, p * (uint32_t)sizeof(ck_label_t)));
#pragma unroll
            for (int j = 0; j < 4; j++) {
                tv[j] = (t4 >> (8 * j)) & 0xFFu;
                const uint32_t l2 = j < 2 ? l4.x : l4.y;
                lab[j] = (j & 1) ? l2 >> 16 : l2 & 0xFFFFu;
            }
        }
        if (round1) {
            it1 = ck_es_round1(tid, x0, y0, w, h);
            const uint32_t p = (uint32_t)it1.cy * (uint32_t)w + (uint32_t)it1.cx;
            tv1 = T[p]; lab1 = L[p];
        }
        {
            const uint32_t slot_base = ck_es_slot_base(it0.cx, it0.cy, a.ccl_tiles_x);
#pragma unroll
            for (int j = 0; j < 4; j++) gather(ck_es_pixel_slot(lab[j], tv[j], it0.inb, slot_base), hop[j], csz[j]);
        }
        if (round1) gather(ck_es_pixel_slot(lab1, tv1, it1.inb && it1.keep, ck_es_slot_base(it1.cx, it1.cy, a.ccl_tiles_x)), hop1, csz1);
        {
            const uint32_t rb = ck_es_root_base(it0.cx, it0.cy, w);
            uint4 v;
            v.x = ck_es_pixel_word(lab[0], tv[0], it0.inb, hop[0], csz[0], rb, w, a.min_comp);
            v.y = ck_es_pixel_word(lab[1], tv[1], it0.inb, hop[1], csz[1], rb, w, a.min_comp);
            v.z = ck_es_pixel_word(lab[2], tv[2], it0.inb, hop[2], csz[2], rb, w, a.min_comp);
            v.w = ck_es_pixel_word(lab[3], tv[3], it0.inb, hop[3], csz[3], rb, w, a.min_comp);
            *reinterpret_cast<uint4 *>(sR + ck_es_item_word(it0)) = v;
        }
        if (round1 && it1.keep)
            sR[ck_es_item_word(it1)] = ck_es_pixel_word(lab1, tv1, it1.inb, hop1, csz1, ck_es_root_base(it1.cx, it1.cy, w), w, a.min_comp);
    } else
    {   // staging: every thread's pixels go through the (up to two) dependent loads side by side (addresses clamped into the frame,
        // results masked): a pixel becomes the frame pixel of its component's root | its colour, or SKIP
        constexpr int SPT = SR_PAD / NT;
        uint32_t lab[SPT], tv[SPT], slot[SPT], hop[SPT], csz[SPT];
        bool inb[SPT];
        int gxs[SPT], gys[SPT];
#pragma unroll
        for (int q = 0; q < SPT; q++) {
            const int i = tid + q * NT;
            const int ly = i / LW, lx = i - ly * LW;
            const int gy = y0 + ly, gx = x0 - 1 + lx;
            inb[q] = i < LH * LW && gy < h && gx >= 0 && gx < w;
            const int cy = min(gy, h - 1), cx = min(max(gx, 0), w - 1);
            const uint32_t p = (uint32_t)cy * (uint32_t)w + (uint32_t)cx;
            tv[q] = T[p]; lab[q] = L[p];
            gxs[q] = cx; gys[q] = cy;
        }
#pragma unroll
        for (int q = 0; q < SPT; q++) { // ring-touching components: the word holds a tile-local id; root and size come from the frame's tables
            // (a word with CK_LBL_SMALL: an interior component below min_component_px — or no component: CK_LBL_NONE has every bit set)
            const bool two = inb[q] && tv[q] != 127u && !(lab[q] & CK_LBL_SMALL) && (lab[q] & CK_LBL_BORDER);
            slot[q] = two ? ck_label_slot(lab[q], gxs[q], gys[q], a.ccl_tiles_x) : 0u; // (entry 0: a harmless read, unused)
            hop[q] = GR[slot[q]]; csz[q] = GS[slot[q]];
        }
#pragma unroll
        for (int q = 0; q < SPT; q++) {
            const bool brd = (lab[q] & CK_LBL_BORDER) != 0u;
            const bool none = !inb[q] || tv[q] == 127u || (lab[q] & CK_LBL_SMALL) || (brd && (int)csz[q] < a.min_comp);
            const uint32_t root = brd ? hop[q] : ck_label_interior_root(lab[q], gxs[q], gys[q], w);
            sR[tid + q * NT] = none ? SKIP : (root | (tv[q] == 255u ? ID_WHITE : 0u));
        }
    }
    reinterpret_cast<uint4 *>(sRow)[tid] = reinterpret_cast<const uint4 *>(g_emit_rows.e)[tid];
    lds_barrier();
    if (a.stop_after == 0) return;

    const int lx = (tid & 63) + 1; // staged column of this thread's pixels
    const int gx = x0 + (tid & 63);
    const int row0 = (tid >> 6) * 4;

    // pass 1: count points per key in the LDS table; the add's return value is the point's rank inside (tile, key), kept in
    // registers (sign << 31 | slot << 16 | rank) so that the write pass neither probes nor counts again.  The thread's 5 x 3 ids
    // are read once; the (up to four) points of a pixel often share their key — the three neighbours below are side by side, so
    // when they are white they are one component — and then make ONE add, the first point of the key doing it for the others.
    constexpr uint32_t NONE = 0xFFFFFFFFu, NO_RUN = 0x80000000u;
    uint32_t cand[16];
    {
        uint32_t R[5][3];
        unsigned long long last_key = 0ull; // the thread's last key and where it is: the pixel below often continues the same boundary
        uint32_t last_s = 0;
        // (a staged row is read one pixel row ahead of its first use, not all five at the start: nine words live instead of fifteen)
        auto stage_row = [&](int r) {
#pragma unroll
            for (int c = 0; c < 3; c++) R[r][c] = sR[G4 ? ck_es_word(row0 + r, lx - 1 + c) : (row0 + r) * LW + lx - 1 + c];
        };
        stage_row(0); stage_row(1);
        // The predicates of a pixel row (ck_emit_row.h) are bits of one vector register, never lane masks: the Boolean algebra the
        // compiler makes of `bool`s runs on the scalar unit, which was this kernel's fuller issue port.  The equalities inside a
        // staged row are formed once and serve the pixel row above (its partners') and the row itself (absorb / drop).
        uint32_t H[5];
        H[0] = ck_er_hword(R[0][0], R[0][1], R[0][2]);
        // (all ones where a sign bit says "outside": columns 1..w-2 emit, x-1 >= 1 may drop, x+1 <= w-2 may absorb)
        const uint32_t colskip = (uint32_t)(((gx - 1) | (w - 2 - gx)) >> 31);
        const uint32_t can = (a.twins ? 3u : 0u) & ~(((uint32_t)((gx - 2) >> 31) & CK_ER_CAN_DROP) | ((uint32_t)((w - 3 - gx) >> 31) & CK_ER_CAN_ABSORB));
        // one leader's probe and add: its place in the table << 16 | the rank of its first point, or NONE (no room in the table)
        auto count = [&](uint32_t r0, uint32_t r1, uint32_t mult) -> uint32_t {
            const uint32_t ra = r0 & ID_VALUE, rb = r1 & ID_VALUE; // (the roots without their colour bits: the cluster's key)
            const unsigned long long key = ra < rb ? ((unsigned long long)ra << 32) | rb : ((unsigned long long)rb << 32) | ra;
            uint32_t s = key_hash(key) & (LHT - 1);
            bool placed = false;
            if (key == last_key) { placed = true; s = last_s; } // (the probe is the expensive part of this pass: 0.6 of its 1.2 ms)
            else
            for (int probe = 0; probe < LHT; probe++) {
                // most points meet their key already in place: a plain read (lanes with one address are served together)
                // finds that out, and only a slot seen empty costs a compare-and-swap (same-address lanes one by one)
                __asm__ volatile("" ::: "memory");
                unsigned long long prev = sKey[s];
                if (prev == 0ull) prev = atomicCAS(&sKey[s], 0ull, key);
                if (prev == 0ull || prev == key) { placed = true; break; }
                s = (s + 1) & (LHT - 1);
            }
            if (!placed) { atomicOr(&counters[CK_CNT_STATUS], (uint32_t)CK_FRAME_CLUSTERS_OVERFLOW); return NONE; }
            last_key = key; last_s = s;
            // (one add carries both counts of the key: physical in the high half — what it was before is the point's rank —, logical
            // in the low half, which never carries: a tile has at most 5 120 points, twins counted twice)
            return (s << 16) | (atomicAdd(&sCnt[s], mult) >> 16);
        };
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
            const int gy = y0 + row0 + rr;
            if (rr < 3) stage_row(rr + 2);
            H[rr + 1] = ck_er_hword(R[rr + 1][0], R[rr + 1][1], R[rr + 1][2]);
            const uint32_t r0 = R[rr][1] | colskip | (uint32_t)(((gy - 1) | (h - 2 - gy)) >> 31); // SKIP where the pixel emits nothing
            const uint32_t r1v[4] = {R[rr][2], R[rr + 1][1], R[rr + 1][0], R[rr + 1][2]}; // (1,0) (0,1) (-1,1) (1,1)
            uint32_t absorb;
            const uint32_t idx = ck_er_index(H[rr], H[rr + 1], r0, R[rr][0], R[rr][1], R[rr][2], R[rr + 1][0], R[rr + 1][1], R[rr + 1][2], can, &absorb);
            const uint32_t e = sRow[idx];
            // Only the first point of a key probes and adds (LDS traffic is what this pass is bound by): the row's LEADERS, which the
            // entry lists with the number of points each stands for.  One block for all of them, in a loop: a wave goes round as
            // often as its lane with the most leaders has them, and a thread has about 3.5 keys in its four rows.  A leader's result
            // goes to the points that named it (c4); an absorbed twin is one more logical point of the (1,1) point's leader.
            const uint32_t lj[4] = {0u, (e >> 20) & 1u, (e >> 21) & 3u, (e >> 23) & 3u}; // the place of a point's leader in the list
            uint32_t c4[4] = {NONE, NONE, NONE, NONE};
            uint32_t le = e & CK_ER_LEADERS; // (a row of four leaders ends with the list)
            for (uint32_t j = 0; (le & 0x1Cu) != 0u; j++, le >>= 5) {
                const uint32_t sl = le & 3u;
                const uint32_t r1 = sl == 0u ? r1v[0] : (sl == 1u ? r1v[1] : (sl == 2u ? r1v[2] : r1v[3]));
                // (physical << 16 | logical: a twin is one word and two points)
                const uint32_t c = count(r0, r1, ((le >> 2) & 7u) * 0x10001u + (lj[3] == j ? absorb : 0u));
#pragma unroll
                for (int k = 0; k < 4; k++) c4[k] = lj[k] == j ? c : c4[k];
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t nth = k == 0 ? 0u : (k == 1 ? (e >> 25) & 1u : (k == 2 ? (e >> 26) & 3u : (e >> 28) & 3u));
                uint32_t c = c4[k];
                c = ((idx >> (9 - k)) & 1u) ? c : NONE; // (not a point, or dropped)
                const uint32_t sign = (r1v[k] & ID_WHITE) << 1; // gradient sign (bit 31): the neighbour is the white one
                // (the twin's sign: its neighbour (x, y+1) is the white one — ID_WHITE is CK_PT_TWIN_SIGN's bit)
                const uint32_t twin = k == 3 ? (0u - absorb) & (CK_PT_TWIN | (r1v[1] & ID_WHITE)) : 0u;
                cand[rr * 4 + k] = c != NONE ? ((c + nth) | sign | twin) : NONE;
                asm volatile("" : "+v"(cand[rr * 4 + k])); // (formed here: left to the compiler it sinks into pass 3, its five inputs kept alive instead)
            }
        }
    }
    lds_barrier();
    if (a.stop_after == 1) return;

    // pass 2: one reservation of temp space and of run records per tile (exclusive scans of the per-key counts / used entries),
    // and per (tile, key) one insert into the frame's table (waited for: it yields the slot) + one add to the cluster's point
    // count that nobody waits for.
    const unsigned long long k0 = sKey[2 * tid], k1 = sKey[2 * tid + 1];
    // (an entry's two counts, physical << 16 | logical, stay side by side through the scans: a tile's 1 024 pixels own at most four
    // points each and absorb at most one more, so neither sum comes near 2^16)
    const uint32_t b0 = k0 ? sCnt[2 * tid] : 0u, b1 = k1 ? sCnt[2 * tid + 1] : 0u;
    const uint32_t c0 = b0 >> 16, c1 = b1 >> 16;
    uint32_t found0 = SKIP, found1 = SKIP, ridx0, tb0, tb1; // (tb: where the key's run starts in the tile's piece of the temp array)
    {
        const uint32_t incl2 = wave_scan_u32(b0 + b1), incl = incl2 >> 16;
        const unsigned long long u0 = __ballot(k0 != 0ull), u1 = __ballot(k1 != 0ull);
        const unsigned long long below = (1ull << (tid & 63)) - 1ull;
        ridx0 = (uint32_t)(__popcll(u0 & below) + __popcll(u1 & below)); // rank of this thread's first used entry in its wave
        if ((tid & 63) == 63) sWave[tid >> 6] = incl2;
        if ((tid & 63) == 0) sRunW[tid >> 6] = (uint32_t)(__popcll(u0) + __popcll(u1));
        lds_barrier();
        uint32_t before = 0, total = 0, rbefore = 0, rtotal = 0;
#pragma unroll
        for (int wv = 0; wv < NT / 64; wv++) {
            uint32_t t = sWave[wv], r = sRunW[wv];
            if (wv < (tid >> 6)) { before += t; rbefore += r; }
            total += t; rtotal += r;
        }
        ridx0 += rbefore;
        before >>= 16;
        if (tid == 0) { // (entries NT / 64 of the two arrays are not among those the loop above reads)
            const uint32_t ptotal = total >> 16, ltotal = total & 0xFFFFu;
            // One add reserves the tile's words in the temp array (CK_CNT_TMP) and counts its points as the oracle counts them, in
            // the word beside it (CK_CNT_CLUSTERS, which is nobody's until k_scan writes it).  The frame's point buffer counts as
            // full when the points the frame HAS pass its capacity, stored twice or once.
            static_assert(CK_CNT_TMP == 0 && CK_CNT_CLUSTERS == 1 && CK_CNT_STRIDE % 2 == 0, "the two counters are one aligned 64-bit word");
            const unsigned long long was = total ? atomicAdd(reinterpret_cast<unsigned long long *>(counters), ((unsigned long long)ltotal << 32) | ptotal) : 0ull;
            sWave[NT / 64] = (uint32_t)was;
            sRunW[NT / 64] = rtotal ? atomicAdd(&counters[CK_CNT_RUNS], rtotal) : 0u;
            if ((uint32_t)(was >> 32) + ltotal > (uint32_t)ws.point_cap) atomicOr(&counters[CK_CNT_STATUS], (uint32_t)CK_FRAME_POINTS_OVERFLOW);
        }
        const uint32_t excl = before + incl - (c0 + c1);
        tb0 = excl; tb1 = excl + c0;
        {   // both first probes of the frame table in flight together; only a probe that met another key walks on
            const uint32_t hm = (uint32_t)(ws.ht_size - 1);
            const uint32_t g0 = key_hash(k0) & hm, g1 = key_hash(k1) & hm;
            const unsigned long long p0 = k0 ? atomicCAS(&gkeys[g0], 0ull, k0) : 0ull;
            const unsigned long long p1 = k1 ? atomicCAS(&gkeys[g1], 0ull, k1) : 0ull;
#pragma unroll
            for (int q = 0; q < 2; q++) {
                const unsigned long long key = q ? k1 : k0, pv = q ? p1 : p0;
                uint32_t found = SKIP;
                if (key != 0ull) {
                    uint32_t g = q ? g1 : g0;
                    if (pv == 0ull || pv == key) found = g;
                    else {
                        for (int probe = 1; probe < ws.ht_size; probe++) {
                            g = (g + 1) & hm;
                            unsigned long long prev = atomicCAS(&gkeys[g], 0ull, key);
                            if (prev == 0ull || prev == key) { found = g; break; }
                        }
                    }
                    if (found == SKIP) atomicOr(&counters[CK_CNT_STATUS], (uint32_t)CK_FRAME_CLUSTERS_OVERFLOW);
                }
                // (a key without a place — no room in the frame's table — has no run: the mark puts every point of it past point_cap
                // in pass 3, which so needs no test of its own for it; point_cap and a tile's base are far below 2^31)
                sTBase[2 * tid + q] = (q ? tb1 : tb0) | (found == SKIP ? NO_RUN : 0u);
                if (q) found1 = found; else found0 = found;
            }
        }
        // (result unused: nothing waits for these)
        if (found0 != SKIP) atomicAdd(&gcount[found0], ((unsigned long long)(b0 & 0xFFFFu) << 32) | c0);
        if (found1 != SKIP) atomicAdd(&gcount[found1], ((unsigned long long)(b1 & 0xFFFFu) << 32) | c1);
    }
    lds_barrier();
    if (a.stop_after == 2) return;

    // pass 3: write the points (one contiguous run per key in the frame's temp array)
    const uint32_t tile_base = sWave[NT / 64];
#pragma unroll
    for (int q = 0; q < 16; q++) {
        const uint32_t cd = cand[q];
        if (cd == NONE) continue;
        const int rr = q >> 2, k = q & 3;
        const int dxk = k == 1 ? 0 : (k == 2 ? -1 : 1), dyk = k == 0 ? 0 : 1;
        const uint32_t s = (cd >> 16) & 0x3FFu, lr = cd & 0xFFFFu;
        const uint32_t ti = tile_base + sTBase[s] + lr;
        if (ti >= (uint32_t)ws.point_cap) continue; // (pass 2 has set the status bit: fewer words than points; or NO_RUN: a key it dropped)
        const int gy = y0 + row0 + rr;
        const uint32_t twin = k == 3 ? cd & (CK_PT_TWIN | CK_PT_TWIN_SIGN) : 0u; // (only a (1,1) point absorbs)
        tmp[ti] = twin | ((uint32_t)(2 * gx + dxk) << 16) | ((uint32_t)(2 * gy + dyk) << 3) | ((uint32_t)k << 1) | (cd >> 31);
    }
    // run records (their place inside the cluster is decided by k_scatter)
    {
        uint32_t ri = sRunW[NT / 64] + ridx0;
#pragma unroll
        for (int q = 0; q < 2; q++) {
            if ((q ? k1 : k0) == 0ull) continue;
            const uint32_t found = q ? found1 : found0;
            // (a key the frame's table had no room for still owns its place in the run list: it gets an empty record — left
            // as it was, k_scatter would follow whatever an earlier call had written there)
            if (ri < (uint32_t)ws.run_cap) {
                ck_run r;
                r.slot = found != SKIP ? found : 0u; r.base = 0; r.tmp_start = tile_base + (q ? tb1 : tb0);
                r.count = found != SKIP ? (q ? c1 : c0) : 0u;
                runs[ri] = r;
            } else if (found != SKIP) atomicOr(&counters[CK_CNT_STATUS], (uint32_t)CK_FRAME_CLUSTERS_OVERFLOW);
            ri++;
        }
    }
}

// zeroes the frames' key and count tables (16 bytes per thread) and, with its first threads, three short arrays
__global__ __launch_bounds__(NT) void k_clear(uint4 *keys4, size_t nkeys4, uint4 *cnt4, size_t ncnt4, uint32_t *c0, uint32_t n0, uint32_t *c1,
                                              uint32_t n1, uint32_t *c2, uint32_t n2) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    const uint4 z = make_uint4(0, 0, 0, 0);
    if (i < nkeys4) keys4[i] = z;
    else if (i - nkeys4 < ncnt4) cnt4[i - nkeys4] = z;
    if (i < n0) c0[i] = 0;
    if (i < n1) c1[i] = 0;
    if (i < n2) c2[i] = 0;
}

// ---- per-frame scan of the hash table -------------------------------------------------------------------------
constexpr int SNT = 1024;
// One workgroup per frame; every wave owns a contiguous 1/16 of the table and walks it 64 slots at a time (coalesced
// reads, DPP wave scans, running offsets in registers): one pass for the wave totals, one to hand out the offsets.
// A cluster's LOGICAL count (twins counted twice: the oracle's) passes the size gates and, as a running sum, decides what the
// frame's point capacity has room for; its PHYSICAL count (words stored) makes the offsets and the cluster record.
__global__ __launch_bounds__(SNT) void k_scan(ck_stage_ws ws, int min_cluster, int max_cluster) {
    __shared__ uint32_t sPts[SNT / 64], sLog[SNT / 64], sCl[SNT / 64];
    const int frame = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const unsigned long long *gkeys = ws.d_ht_keys + (size_t)frame * ws.ht_size;
    const unsigned long long *gcount = ws.d_ht_count + (size_t)frame * ws.ht_size;
    uint32_t *goff = ws.d_ht_off + (size_t)frame * ws.ht_size;
    uint32_t *counters = ws.d_counters + (size_t)frame * CK_CNT_STRIDE;
    ck_cluster_t *clusters = ws.d_clusters + (size_t)frame * ws.cluster_cap;
    const int seg = ws.ht_size / (SNT / 64); // ht_size is a multiple of SNT, so seg is a multiple of 64
    const int base = wv * seg;
    uint32_t pts = 0, lpts = 0, cl = 0;
#pragma unroll 8
    for (int r = 0; r < seg; r += 64) { // (unrolled: eight loads in flight; as a plain loop every 64 slots cost a trip to memory)
        const unsigned long long c2 = gcount[base + r + lane];
        const uint32_t c = (uint32_t)c2, lc = (uint32_t)(c2 >> 32);
        bool ok = (int)lc >= min_cluster && (int)lc <= max_cluster;
        pts += ok ? c : 0u; lpts += ok ? lc : 0u; cl += ok ? 1u : 0u;
    }
    pts = (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_u32(pts), 63);
    lpts = (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_u32(lpts), 63);
    cl = (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_u32(cl), 63);
    if (lane == 0) { sPts[wv] = pts; sLog[wv] = lpts; sCl[wv] = cl; }
    __syncthreads();
    uint32_t po = 0, lo = 0, co = 0;
    for (int k = 0; k < wv; k++) { po += sPts[k]; lo += sLog[k]; co += sCl[k]; }
    // (the counts of four rounds are fetched together, then worked off in order; seg is a multiple of 64, not always of 256)
    for (int r4 = 0; r4 < seg; r4 += 256) {
        unsigned long long c4[4];
#pragma unroll
        for (int q = 0; q < 4; q++) c4[q] = r4 + 64 * q < seg ? gcount[base + r4 + 64 * q + lane] : 0ull;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int r = r4 + 64 * q;
        if (r >= seg) continue; // (uniform)
        const int e = base + r + lane;
        const uint32_t c = (uint32_t)c4[q], lc = (uint32_t)(c4[q] >> 32);
        const bool ok = (int)lc >= min_cluster && (int)lc <= max_cluster;
        const uint32_t ip = wave_scan_u32(ok ? c : 0u), il = wave_scan_u32(ok ? lc : 0u), ic = wave_scan_u32(ok ? 1u : 0u);
        uint32_t off = SKIP;
        if (ok) {
            const uint32_t my_po = po + ip - c, my_lo = lo + il - lc, my_co = co + ic - 1u;
            if (my_co < (uint32_t)ws.cluster_cap && my_lo + lc <= (uint32_t)ws.point_cap) { // (my_po + c <= my_lo + lc: the words fit too)
                off = my_po;
                unsigned long long key = gkeys[e];
                ck_cluster_t ck;
                ck.rep0 = (uint32_t)(key >> 32); ck.rep1 = (uint32_t)key; ck.start = my_po; ck.count = c;
                clusters[my_co] = ck;
            } else {
                // no room for the cluster's points (or for its record): it is dropped.  Its record must not stay what an earlier
                // call left there — the count of clusters below includes it — so it becomes an empty one, which k_classify skips
                if (my_co < (uint32_t)ws.cluster_cap) {
                    ck_cluster_t ck;
                    ck.rep0 = 0; ck.rep1 = 0; ck.start = 0; ck.count = 0;
                    clusters[my_co] = ck;
                }
                atomicOr(&counters[CK_CNT_STATUS], (uint32_t)CK_FRAME_CLUSTERS_OVERFLOW);
            }
        }
        goff[e] = off;
        po += (uint32_t)__builtin_amdgcn_readlane((int)ip, 63);
        lo += (uint32_t)__builtin_amdgcn_readlane((int)il, 63);
        co += (uint32_t)__builtin_amdgcn_readlane((int)ic, 63);
    }
    }
    if (tid == SNT - 1) {
        counters[CK_CNT_CLUSTERS] = min(co, (uint32_t)ws.cluster_cap);
        counters[CK_CNT_POINTS] = min(po, (uint32_t)ws.point_cap);
    }
}

// One wave per run: a (tile, cluster) run of the temp array goes to its place inside the cluster, coalesced on both sides.
// RPW: run records a wave takes per round — 64 for batches; a call with a few frames has too few runs to keep the chip busy
// that way (8 k runs = 128 waves), so it hands them out 8 at a time over eight times as many waves
template <int RPW>
__global__ __launch_bounds__(NT) void k_scatter(ck_stage_ws ws) {
    const int frame = blockIdx.y;
    const uint32_t *counters = ws.d_counters + (size_t)frame * CK_CNT_STRIDE;
    const uint32_t nruns = min(counters[CK_CNT_RUNS], (uint32_t)ws.run_cap);
    const uint32_t ntmp = min(counters[CK_CNT_TMP], (uint32_t)ws.point_cap);
    const ck_packed_point *tmp = ws.d_tmp + (size_t)frame * ws.ext_cap;
    const ck_run *runs = ws.d_runs + (size_t)frame * ws.run_cap;
    uint32_t *goff = ws.d_ht_off + (size_t)frame * ws.ht_size;
    ck_packed_point *pts = ws.d_points + (size_t)frame * ws.ext_cap;
    const int lane = threadIdx.x & 63;
    const uint32_t wave = blockIdx.x * (NT / 64) + (threadIdx.x >> 6), nwaves = gridDim.x * (NT / 64);
    // 64 runs per wave and round: every lane fetches one run record and its cluster offset (two dependent loads paid once
    // for 64 runs), then the wave copies the runs one after the other (runs of up to 64 points: 16 lanes each, four runs at a time)
    for (uint32_t r0 = wave * RPW; r0 < nruns; r0 += nwaves * RPW) {
        ck_run mine = {0, 0, 0, 0};
        uint32_t moff = SKIP;
        if (lane < RPW && r0 + lane < nruns) { mine = runs[r0 + lane]; moff = goff[mine.slot]; }
        if (moff == SKIP) mine.count = 0; // cluster dropped by k_scan (too small / too large / no room)
        // goff[slot] starts as the cluster's offset and serves as its fill cursor: the add returns where this run goes
        const uint32_t dst0 = mine.count ? atomicAdd(&goff[mine.slot], mine.count) : 0u;
        // short runs first, four per step
        const unsigned long long small = __ballot(mine.count > 0 && mine.count <= 64);
        unsigned long long todo = small;
        const int sub = lane >> 4, sl = lane & 15;
        while (todo) {
            // pick up to four set bits of `todo`; sub-group `sub` takes the sub-th of them
            unsigned long long t = todo;
            int pick = -1;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int bit = t ? __builtin_ctzll(t) : -1;
                if (q == sub) pick = bit;
                if (t) t &= t - 1;
            }
            todo = t;
            const int srcl = pick < 0 ? 0 : pick;
            const uint32_t cnt = (uint32_t)__shfl((int)mine.count, srcl, 64), ts = (uint32_t)__shfl((int)mine.tmp_start, srcl, 64),
                           ds = (uint32_t)__shfl((int)dst0, srcl, 64);
            ck_packed_point v[4];
            bool ok[4];
#pragma unroll
            for (int q = 0; q < 4; q++) { // all loads of the step are in flight before the first store
                const uint32_t j = (uint32_t)sl + 16u * q;
                ok[q] = pick >= 0 && j < cnt && ts + j < ntmp;
                v[q] = ok[q] ? tmp[ts + j] : 0u;
            }
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (ok[q]) pts[ds + (uint32_t)sl + 16u * q] = v[q];
        }
        unsigned long long big = __ballot(mine.count > 64);
        while (big) {
            const int srcl = __builtin_ctzll(big);
            big &= big - 1;
            const uint32_t cnt = (uint32_t)__builtin_amdgcn_readlane((int)mine.count, srcl), ts = (uint32_t)__builtin_amdgcn_readlane((int)mine.tmp_start, srcl),
                           ds = (uint32_t)__builtin_amdgcn_readlane((int)dst0, srcl);
            for (uint32_t j0 = 0; j0 < cnt; j0 += 256) {
                ck_packed_point v[4];
                bool ok[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const uint32_t j = j0 + (uint32_t)lane + 64u * q;
                    ok[q] = j < cnt && ts + j < ntmp;
                    v[q] = ok[q] ? tmp[ts + j] : 0u;
                }
#pragma unroll
                for (int q = 0; q < 4; q++)
                    if (ok[q]) pts[ds + j0 + (uint32_t)lane + 64u * q] = v[q];
            }
        }
    }
}

} // namespace

int ck_launch_clusters(ck_handle *h, int n) {
    ck_stage_ws &ws = h->ws;
    {   // one launch clears everything the rest of the call counts into: the frames' key / count tables and counters, the fit's
        // list counts and dequeue heads, the decode candidates' counts (five fills before; their launches were a twentieth of
        // a one-frame call)
        const ck_fit_layout fl = ck_fit_scratch_layout(ws, h->cfg.max_batch);
        const size_t nkeys4 = (size_t)ws.ht_size * n / 2, ncnt4 = (size_t)ws.ht_size * n / 2; // (8 bytes per slot each) ht_size is a multiple of 1024
        const size_t total4 = nkeys4 + ncnt4;
        hipLaunchKernelGGL(k_clear, dim3((unsigned)((total4 + NT - 1) / NT)), dim3(NT), 0, h->stream,
                           reinterpret_cast<uint4 *>(ws.d_ht_keys), nkeys4, reinterpret_cast<uint4 *>(ws.d_ht_count), ncnt4, ws.d_counters,
                           (uint32_t)(CK_CNT_STRIDE * n), fl.list_counts, 32u, fl.cand_count, (uint32_t)n);
    }
    EmitArgs a;
    a.thresh = h->d_thresh; a.labels = h->d_labels; a.groot = h->d_groot; a.gsize = h->d_gsize; a.slots = (size_t)h->broot_cap;
    a.w = h->qw; a.h = h->qh; a.tiles_x = (h->qw + ETW - 1) / ETW; a.tiles_y = (h->qh + ETH - 1) / ETH;
    a.min_comp = h->cfg.min_component_px; a.ws = ws; a.ccl_tiles_x = h->tiles_x;
    { static const int stop_after = ck_knob(CK_KNOB_EMIT_STOP_AFTER); a.stop_after = stop_after; }
    // (diagnostics: 0 = every point on its own, for A/B; 2 = twins merged, but the quad fit is not told and keeps its duplicate removal)
    { static const int twins = ck_knob(CK_KNOB_EMIT_TWINS); a.twins = twins; h->pts_distinct = twins == 1; }
    { static const int stage4 = ck_knob(CK_KNOB_EMIT_STAGE4); a.stage4 = stage4; } // (diagnostics: 0 = every pixel staged on its own, for A/B)
    const int xcd_map = n >= 16 ? 1 : 0; // frames dealt to XCDs: batches of 16 frames and more
    const unsigned grid = xcd_map ? (unsigned)(((n + 7) / 8) * 8 * a.tiles_x * a.tiles_y) : (unsigned)(a.tiles_x * a.tiles_y * n);
    // groups of four pixels: rows, frames and the buffers themselves start at multiples of four pixels
    const bool g4 = a.stage4 && ck_es_group_path(a.w) && ((uintptr_t)a.thresh & 3u) == 0 && ((uintptr_t)a.labels & 7u) == 0;
    if (g4) hipLaunchKernelGGL(k_emit2<true>, dim3(grid), dim3(NT), 0, h->stream, a, xcd_map, n);
    else hipLaunchKernelGGL(k_emit2<false>, dim3(grid), dim3(NT), 0, h->stream, a, xcd_map, n);
    int min_cluster = h->cfg.min_cluster_pixels < 24 ? 24 : h->cfg.min_cluster_pixels;
    hipLaunchKernelGGL(k_scan, dim3((unsigned)n), dim3(SNT), 0, h->stream, ws, min_cluster, ws.max_cluster_points);
    if (n <= 4) hipLaunchKernelGGL(k_scatter<8>, dim3(256u, (unsigned)n), dim3(NT), 0, h->stream, ws);
    else hipLaunchKernelGGL(k_scatter<64>, dim3(SCATTER_WGS, (unsigned)n), dim3(NT), 0, h->stream, ws);
    CK_HIP(hipGetLastError());
    return CK_OK;
}
