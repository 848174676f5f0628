// ck_emit_row.h — one pixel row of k_emit2's count pass (k_clusters.hip) as a word of predicate bits and a table indexed by it.
//
// A pixel (x, y) emits up to four points, one per forward neighbour k = 0..3 at (1,0) (0,1) (-1,1) (1,1).  What the count pass
// needs to know about them is a function of six staged words — A0 A1 A2 = (x-1..x+1, y), B0 B1 B2 = (x-1..x+1, y+1), each the
// frame pixel of a component's root | its colour, or SKIP — and of three thread constants: the pixel lies in the emitting
// columns and rows, its right neighbour does (it may ABSORB the twin that neighbour would emit), its left neighbour does (it
// may DROP its own (-1,1) point, which that neighbour absorbs).  ck_emit_row_direct() below is that function, written as the
// kernel had it; it is the specification.  The kernel does not evaluate it: it forms the predicates as bits of a 32-bit value
// in a vector register (ck_er_index: a compare into VCC and an add-with-carry per bit, no lane masks), and reads the points'
// leaders, places and counts from ck_emit_row_table, which is generated from ck_emit_row_classes() at compile time.
// tests/cpp/emit_row_check.cpp checks the table entry of every index six words can produce against the direct evaluation.
// Plain C++17: a host program includes this file without the HIP headers.
#ifndef CK_EMIT_ROW_H
#define CK_EMIT_ROW_H

#include <stdint.h>

#if defined(__HIPCC__)
#define CK_ER_HD __host__ __device__ __forceinline__
#else
#define CK_ER_HD inline
#endif

constexpr uint32_t CK_ER_SKIP = 0xFFFFFFFFu;  // a staged word without a component
constexpr uint32_t CK_ER_WHITE = 0x40000000u; // a staged word's colour bit; the root below it is < 2^24

// ---- the specification ---------------------------------------------------------------------------------------------------------------
struct ck_emit_row {
    bool ok[4];       // neighbour k makes a point (after a drop: ok[2] false)
    uint8_t lead[4];  // the first point with k's partner (its key's leader: the one that probes and adds)
    uint8_t nth[4];   // k's place among the points of its key
    uint8_t units[4]; // how many points leader k adds for (itself and its followers); an absorbed twin is NOT in here
    bool absorb;      // the (1,1) point stands for the twin of (x+1, y) as well: one word, one more logical point
    bool drop;        // the (-1,1) point is the twin (x-1, y) absorbs
};

// leaders, places and counts from the points that exist and the equalities of their partner words (eq[j][k], j < k)
CK_ER_HD constexpr void ck_emit_row_classes(ck_emit_row &r, const bool eq[4][4]) {
    for (int k = 0; k < 4; k++) {
        r.lead[k] = (uint8_t)k; r.nth[k] = 0; r.units[k] = 1;
        for (int j = k - 1; j >= 0; j--)
            if (r.ok[j] && r.ok[k] && eq[j][k]) { r.lead[k] = (uint8_t)j; r.nth[k]++; }
        for (int j = k + 1; j < 4; j++)
            if (r.ok[j] && r.ok[k] && eq[k][j]) r.units[k]++;
    }
}

// emits: (x, y) lies in columns 1..w-2 and rows 1..h-2; can_absorb: twins merge and x+1 <= w-2; can_drop: twins merge and x-1 >= 1
CK_ER_HD constexpr ck_emit_row ck_emit_row_direct(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t b0, uint32_t b1, uint32_t b2, bool emits,
                                                  bool can_absorb, bool can_drop) {
    ck_emit_row r{};
    const uint32_t r0 = emits ? a1 : CK_ER_SKIP;
    const uint32_t r1v[4] = {a2, b1, b0, b2};
    for (int k = 0; k < 4; k++) r.ok[k] = r0 != CK_ER_SKIP && r1v[k] != CK_ER_SKIP && ((r0 ^ r1v[k]) & CK_ER_WHITE) != 0u;
    // Twins.  When both diagonals of the 2 x 2 block at (x, y) join the same two components, the point (2x+1, 2y+1) is emitted
    // twice into one cluster: by (1,1) from (x, y) and by (-1,1) from (x+1, y).  The first ABSORBS the second (its word then
    // stands for both), the owner of the second DROPS it.  Absorb, at (x, y): the own k = 3 pair is a point; the twin's
    // owner (x+1, y) lies in the emitting columns (x+1 <= w-2; its row is this one); the twin's pair (x+1, y) / (x, y+1)
    // holds the same two staged words — which makes it a point as well: equal words are equal colours and neither is SKIP.
    // Drop, at (x, y): the mirror image — the own k = 2 pair is a point, (x-1, y) lies in the emitting columns (x-1 >= 1),
    // and its k = 3 pair (x-1, y) / (x, y+1) holds the same two words.  Both threads evaluate the same four staged words by
    // the same rule, also across an emit-tile boundary (the staged region carries a column either side and a row below,
    // and a staged word is a function of the frame alone), so one absorbs exactly when the other drops.  At the frame's
    // edges one copy does not exist (owner in column 0 or w-1; rows 0 and h-1 emit nothing for either) and nothing merges.
    r.absorb = can_absorb && r.ok[3] && ((r0 == a2 && b2 == b1) || (r0 == b1 && b2 == a2));
    r.drop = can_drop && r.ok[2] && ((r0 == a0 && b0 == b1) || (r0 == b1 && b0 == a0));
    r.ok[2] = r.ok[2] && !r.drop;
    bool eq[4][4] = {};
    for (int j = 0; j < 4; j++)
        for (int k = j + 1; k < 4; k++) eq[j][k] = r1v[j] == r1v[k];
    ck_emit_row_classes(r, eq);
    return r;
}

// ---- the row word ----------------------------------------------------------------------------------------------------------------------
// One predicate becomes the lowest bit of an accumulator that moves up by one: acc = 2 acc + p.  On the device that is a compare
// into VCC and an add-with-carry, two vector instructions and nothing on the scalar unit; written in C++ the compiler keeps
// predicates as 64-bit lane masks and combines them there.
CK_ER_HD uint32_t ck_er_push_eq(uint32_t acc, uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm("v_cmp_eq_u32_e32 vcc, %1, %2\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc" : "+v"(acc) : "v"(a), "v"(b) : "vcc");
    return acc;
#else
    return 2u * acc + (a == b ? 1u : 0u);
#endif
}
// (the first bit of an accumulator, and a predicate as a mask of all ones: neither needs a register set to zero first)
CK_ER_HD uint32_t ck_er_bit_eq(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t acc;
    asm("v_cmp_eq_u32_e32 vcc, %1, %2\n\tv_addc_co_u32_e64 %0, vcc, 0, 0, vcc" : "=v"(acc) : "v"(a), "v"(b) : "vcc");
    return acc;
#else
    return a == b ? 1u : 0u;
#endif
}
CK_ER_HD uint32_t ck_er_mask_eq(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t m;
    asm("v_cmp_eq_u32_e32 vcc, %1, %2\n\tv_cndmask_b32_e64 %0, 0, -1, vcc" : "=v"(m) : "v"(a), "v"(b) : "vcc");
    return m;
#else
    return a == b ? 0xFFFFFFFFu : 0u;
#endif
}
// a point: neither word is SKIP and the colours differ.  x = r0 ^ r1 has bit 31 set when exactly one is SKIP (the other's bit 31 is
// clear), is 0 when both are, and has the colours' difference in bit 30 otherwise: a point exactly when 2^30 <= x < 2^31.
CK_ER_HD uint32_t ck_er_push_ok(uint32_t acc, uint32_t r0, uint32_t r1) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t x = r0 ^ r1;
    asm("v_cmp_le_i32_e32 vcc, 0x40000000, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc" : "+v"(acc) : "v"(x) : "vcc");
    return acc;
#else
    return 2u * acc + ((int32_t)(r0 ^ r1) >= (int32_t)CK_ER_WHITE ? 1u : 0u);
#endif
}
// the equalities inside one staged row: e(0,2) << 2 | e(0,1) << 1 | e(1,2).  A thread forms them once per staged row: for the
// pixel row above they are the partners' equalities, for the row itself the centre's left / right tests of absorb and drop.
CK_ER_HD uint32_t ck_er_hword(uint32_t r0, uint32_t r1, uint32_t r2) {
    return ck_er_push_eq(ck_er_push_eq(ck_er_bit_eq(r0, r2), r0, r1), r1, r2);
}

// Index bits: 9..6 ok[0..3] (a dropped point's bit cleared), 5..3 eq(0,1) eq(0,2) eq(0,3), 2..0 eq(2,3) eq(1,2) eq(1,3) of the
// partners r1v = {A2, B1, B0, B2}; the equalities are those of the WORDS, whether the points exist or not.
constexpr int CK_ER_INDEX_BITS = 10, CK_ER_ROWS = 1 << CK_ER_INDEX_BITS;
constexpr uint32_t CK_ER_CAN_ABSORB = 1u, CK_ER_CAN_DROP = 2u; // the thread constants, in the places of ok[3] and ok[2] of `okw`

// ha, hb: ck_er_hword of the rows A and B; r0: A1, or SKIP where the pixel does not emit; can: CK_ER_CAN_*.  *absorb: 0 or 1.
CK_ER_HD uint32_t ck_er_index(uint32_t ha, uint32_t hb, uint32_t r0, uint32_t a0, uint32_t a1, uint32_t a2, uint32_t b0, uint32_t b1,
                              uint32_t b2, uint32_t can, uint32_t *absorb) {
    const uint32_t okw = ck_er_push_ok(ck_er_push_ok(ck_er_push_ok(ck_er_push_ok(0u, r0, a2), r0, b1), r0, b0), r0, b2);
    const uint32_t acc = ck_er_push_eq(ck_er_push_eq(ck_er_push_eq(okw, a2, b1), a2, b0), a2, b2);
    // bit 1: drop, bit 0: absorb.  Either both rows' horizontal equalities hold (A0 = A1 and B0 = B1; A1 = A2 and B1 = B2) or the
    // vertical and the far one do (A1 = B1 and A0 = B0; A1 = B1 and A2 = B2); gated by the own point and the thread's constants.
    const uint32_t far = ck_er_push_eq(ck_er_bit_eq(a0, b0), a2, b2);
    const uint32_t vert = ck_er_mask_eq(a1, b1);
    const uint32_t ad = ((ha & hb) | (far & vert)) & okw & can;
    *absorb = ad & 1u;
    return ((acc << 3) | hb) - ((ad & CK_ER_CAN_DROP) << 6); // (a drop: ok[2], which was set, cleared)
}

// ---- the table ---------------------------------------------------------------------------------------------------------------------------
// An entry lists the row's LEADERS in order of k, five bits each: bits 5j+1..5j the j-th leader's k, bits 5j+4..5j+2 its units
// (0: the row has no j-th leader, nor a later one); and for every point its leader's place in that list and its own place among its key's points: bit 20, bits
// 22..21, 24..23 for k = 1, 2, 3 (k = 0 can only be leader 0), and bit 25, bits 27..26, 29..28 likewise.
struct ck_emit_row_table { uint32_t e[CK_ER_ROWS]; };
constexpr uint32_t CK_ER_LEADERS = 0xFFFFFu; // the list of leaders inside an entry

CK_ER_HD constexpr uint32_t ck_emit_row_entry(uint32_t idx) {
    ck_emit_row r{};
    for (int k = 0; k < 4; k++) r.ok[k] = ((idx >> (9 - k)) & 1u) != 0u;
    bool eq[4][4] = {};
    eq[0][1] = (idx >> 5) & 1u; eq[0][2] = (idx >> 4) & 1u; eq[0][3] = (idx >> 3) & 1u;
    eq[2][3] = (idx >> 2) & 1u; eq[1][2] = (idx >> 1) & 1u; eq[1][3] = idx & 1u;
    ck_emit_row_classes(r, eq);
    uint32_t e = 0, n = 0, rank[4] = {0, 0, 0, 0};
    for (int k = 0; k < 4; k++)
        if (r.ok[k] && r.lead[k] == k) { e |= ((uint32_t)r.units[k] << 2 | (uint32_t)k) << (5 * n); rank[k] = n++; }
    const int rank_at[4] = {0, 20, 21, 23}, nth_at[4] = {0, 25, 26, 28};
    for (int k = 1; k < 4; k++)
        if (r.ok[k]) e |= rank[r.lead[k]] << rank_at[k] | (uint32_t)r.nth[k] << nth_at[k];
    return e;
}

CK_ER_HD constexpr ck_emit_row_table ck_make_emit_row_table() {
    ck_emit_row_table t{};
    for (uint32_t i = 0; i < (uint32_t)CK_ER_ROWS; i++) t.e[i] = ck_emit_row_entry(i);
    return t;
}

#endif
