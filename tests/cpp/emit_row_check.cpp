// emit_row_check.cpp — CPU check of chalkydri_amd/csrc/ck_emit_row.h: the row word and the row table k_emit2's count pass reads its
// leaders from, against the definition the kernel evaluated per pixel before the table existed (transcribed below from that kernel).
//
// Every combination of six staged words over an alphabet of SKIP and four roots of either colour, times the eight settings of the
// thread constants, is run through (a) the earlier kernel's text, (b) ck_emit_row_direct, the header's specification, and (c) the
// kernel's own path: ck_er_index -> table entry -> the walk over the entry's leaders exactly as k_emit2 does it.  All three must
// agree on which points exist, on each point's leader and place, on what every leader adds, and on absorb and drop.  Four roots
// per colour reach every index six words can reach: the index holds the four ok bits and the six equalities of the four partner
// words, and four words take at most four different values; the centre word enters only through its colour and SKIP.  An index is
// "missing" when six words produce it and the table's entry there is not what the definition says — which is what (c) tests for
// every index met; the number of different indices met is printed and must be the number a plain count of the consistent ones gives.
// Built with -fsanitize=address,undefined (Makefile: emit_row_check); no GPU, no library.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "ck_emit_row.h"

static constexpr ck_emit_row_table TABLE = ck_make_emit_row_table();   // as the kernel's translation unit holds it

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 10) { printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Old { bool ok[4], absorb, drop; uint32_t lead[4], nth[4], mult[4]; };

// k_emit2's count pass as it stood before ck_emit_row.h (names and expressions kept)
static Old old_row(const uint32_t R0[3], const uint32_t R1[3], bool emits, bool twins, bool right_emits, bool left_emits) {
    const uint32_t SKIP = 0xFFFFFFFFu, ID_WHITE = 0x40000000u;
    Old o;
    const uint32_t r0 = emits ? R0[1] : SKIP;
    const uint32_t r1v[4] = {R0[2], R1[1], R1[0], R1[2]}; // (1,0) (0,1) (-1,1) (1,1)
    bool ok[4];
    for (int k = 0; k < 4; k++) ok[k] = r0 != SKIP && r1v[k] != SKIP && ((r0 ^ r1v[k]) & ID_WHITE) != 0u;
    const bool absorb = twins && ok[3] && right_emits && ((r0 == r1v[0] && r1v[3] == r1v[1]) || (r0 == r1v[1] && r1v[3] == r1v[0]));
    const bool drop = twins && ok[2] && left_emits && ((r0 == R0[0] && r1v[2] == r1v[1]) || (r0 == r1v[1] && r1v[2] == R0[0]));
    ok[2] = ok[2] && !drop;
    const uint32_t unit = 0x10001u, unit3 = absorb ? 0x10002u : unit;
    for (int k = 0; k < 4; k++) {
        o.lead[k] = (uint32_t)k; o.nth[k] = 0; o.mult[k] = k == 3 ? unit3 : unit;
        for (int j = k - 1; j >= 0; j--) { const bool eq = ok[j] && r1v[j] == r1v[k]; o.lead[k] = eq ? (uint32_t)j : o.lead[k]; o.nth[k] += eq ? 1u : 0u; }
        for (int j = k + 1; j < 4; j++) o.mult[k] += (ok[j] && r1v[j] == r1v[k]) ? (j == 3 ? unit3 : unit) : 0u;
    }
    for (int k = 0; k < 4; k++) o.ok[k] = ok[k];
    o.absorb = absorb; o.drop = drop;
    return o;
}

// an index some six words can produce: the equalities are an equivalence of the four partners, and partners that are equal words
// are points together — unless the one that is not is k = 2, dropped
static bool consistent(uint32_t idx, bool *needs_drop) {
    bool ok[4], eq[4][4] = {};
    for (int k = 0; k < 4; k++) { ok[k] = (idx >> (9 - k)) & 1u; eq[k][k] = true; }
    eq[0][1] = (idx >> 5) & 1u; eq[0][2] = (idx >> 4) & 1u; eq[0][3] = (idx >> 3) & 1u;
    eq[2][3] = (idx >> 2) & 1u; eq[1][2] = (idx >> 1) & 1u; eq[1][3] = idx & 1u;
    for (int j = 0; j < 4; j++) for (int k = 0; k < j; k++) eq[j][k] = eq[k][j];
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) for (int k = 0; k < 4; k++)
        if (eq[i][j] && eq[j][k] && !eq[i][k]) return false;
    *needs_drop = false;
    for (int j = 0; j < 4; j++) for (int k = 0; k < 4; k++)
        if (eq[j][k] && ok[j] != ok[k]) {
            if ((j == 2 && !ok[2]) || (k == 2 && !ok[2])) *needs_drop = true; else return false;
        }
    return true;
}

int main() {
    const uint32_t W = CK_ER_WHITE, S = CK_ER_SKIP;
    const uint32_t alphabet[9] = {S, 11u, 500u, 70000u, 0xFFFFFEu, W | 11u, W | 500u, W | 70001u, W | 0xFFFFFFu};
    static bool seen[CK_ER_ROWS];
    static int leaders_hist[5];
    long rows = 0, absorbs = 0, drops = 0, both = 0;
    uint32_t w[6];
    for (int n = 0; n < 9 * 9 * 9 * 9 * 9 * 9; n++) {
        int m = n;
        for (int i = 0; i < 6; i++) { w[i] = alphabet[m % 9]; m /= 9; }
        const uint32_t a0 = w[0], a1 = w[1], a2 = w[2], b0 = w[3], b1 = w[4], b2 = w[5];
        const uint32_t ha = ck_er_hword(a0, a1, a2), hb = ck_er_hword(b0, b1, b2);
        CHECK(ha < 8u && hb < 8u, "hword %u %u", ha, hb);
        for (int f = 0; f < 8; f++) {
            const bool emits = f & 1, can_absorb = f & 2, can_drop = f & 4;
            const uint32_t R0[3] = {a0, a1, a2}, R1[3] = {b0, b1, b2};
            // (twins on with either neighbour emitting or not; twins off is both constants false)
            const Old o = old_row(R0, R1, emits, can_absorb || can_drop, can_absorb, can_drop);
            const ck_emit_row d = ck_emit_row_direct(a0, a1, a2, b0, b1, b2, emits, can_absorb, can_drop);
            uint32_t absorb = 7u;
            const uint32_t can = (can_absorb ? CK_ER_CAN_ABSORB : 0u) | (can_drop ? CK_ER_CAN_DROP : 0u);
            const uint32_t idx = ck_er_index(ha, hb, emits ? a1 : S, a0, a1, a2, b0, b1, b2, can, &absorb);
            CHECK(idx < (uint32_t)CK_ER_ROWS && absorb <= 1u, "index %u absorb %u", idx, absorb);
            if (idx >= (uint32_t)CK_ER_ROWS) continue;
            seen[idx] = true;
            rows++;
            // (b) the specification against the earlier kernel's text
            CHECK(d.absorb == o.absorb && d.drop == o.drop, "n %d f %d absorb %d/%d drop %d/%d", n, f, d.absorb, o.absorb, d.drop, o.drop);
            for (int k = 0; k < 4; k++) {
                CHECK(d.ok[k] == o.ok[k], "n %d f %d k %d ok", n, f, k);
                if (!o.ok[k]) continue;
                CHECK(d.lead[k] == o.lead[k] && d.nth[k] == o.nth[k], "n %d f %d k %d lead %d/%u nth %d/%u", n, f, k, d.lead[k], o.lead[k], d.nth[k], o.nth[k]);
                if (o.lead[k] == (uint32_t)k)
                    CHECK(d.units[k] * 0x10001u + ((d.absorb && d.lead[3] == k) ? 1u : 0u) == o.mult[k], "n %d f %d k %d units %d mult %x", n, f, k, d.units[k], o.mult[k]);
            }
            // (c) the kernel's path: the entry, walked as k_emit2 walks it
            const uint32_t e = TABLE.e[idx];
            const uint32_t lj[4] = {0u, (e >> 20) & 1u, (e >> 21) & 3u, (e >> 23) & 3u};
            const uint32_t nth[4] = {0u, (e >> 25) & 1u, (e >> 26) & 3u, (e >> 28) & 3u};
            uint32_t slot_of[4] = {9, 9, 9, 9}, mult_of[4] = {0, 0, 0, 0}, nlead = 0;
            uint32_t le = e & CK_ER_LEADERS;
            for (uint32_t j = 0; (le & 0x1Cu) != 0u; j++, le >>= 5) {
                CHECK(j < 4u, "n %d f %d: a fifth leader", n, f);
                if (j >= 4u) break;
                slot_of[j] = le & 3u;
                mult_of[j] = ((le >> 2) & 7u) * 0x10001u + (lj[3] == j ? absorb : 0u);
                nlead++;
            }
            CHECK(absorb == (o.absorb ? 1u : 0u), "n %d f %d absorb %u/%d", n, f, absorb, o.absorb);
            uint32_t want_leaders = 0;
            for (int k = 0; k < 4; k++) {
                const bool okk = (idx >> (9 - k)) & 1u;
                CHECK(okk == o.ok[k], "n %d f %d k %d ok bit of the index", n, f, k);
                if (!o.ok[k]) continue;
                CHECK(lj[k] < nlead && slot_of[lj[k]] == o.lead[k] && nth[k] == o.nth[k], "n %d f %d k %d idx %u entry %x: leader %u (slot %u) / %u, nth %u / %u",
                      n, f, k, idx, e, lj[k], lj[k] < 4 ? slot_of[lj[k]] : 99u, o.lead[k], nth[k], o.nth[k]);
                if (o.lead[k] == (uint32_t)k) {
                    want_leaders++;
                    CHECK(lj[k] < nlead && mult_of[lj[k]] == o.mult[k], "n %d f %d k %d idx %u entry %x: adds %x / %x", n, f, k, idx, e, lj[k] < 4 ? mult_of[lj[k]] : 0u, o.mult[k]);
                }
            }
            CHECK(nlead == want_leaders, "n %d f %d idx %u: %u leaders / %u", n, f, idx, nlead, want_leaders);
            for (uint32_t j = 1; j < nlead; j++) CHECK(slot_of[j] > slot_of[j - 1], "n %d f %d: leaders out of order", n, f);
            leaders_hist[want_leaders <= 4 ? want_leaders : 4]++;
            absorbs += o.absorb; drops += o.drop; both += o.absorb && o.drop;
        }
    }
    // the indices met are exactly the consistent ones (a count that knows nothing of staged words)
    int met = 0, want = 0;
    for (uint32_t i = 0; i < (uint32_t)CK_ER_ROWS; i++) {
        bool needs_drop = false;
        const bool c = consistent(i, &needs_drop);
        met += seen[i]; want += c && (!needs_drop || seen[i]);
        // (of the indices only a drop explains, those are met whose other bits the drop's own condition allows)
        CHECK(seen[i] ? c : (!c || needs_drop), "index %u: met %d, consistent %d (by a drop only: %d)", i, seen[i], c, needs_drop);
        CHECK(TABLE.e[i] == ck_emit_row_entry(i) && (TABLE.e[i] >> 30) == 0u, "entry %u", i);
    }
    for (int l = 0; l <= 4; l++) CHECK(leaders_hist[l] > 0, "no row of %d leaders", l);
    CHECK(absorbs > 0 && drops > 0 && both > 0, "absorb %ld drop %ld both %ld", absorbs, drops, both);
    if (fails) { printf("%d failures\n", fails); return 1; }
    printf("OK %ld rows, %d of %d indices met (= the consistent ones: %d), leaders 0..4: %d %d %d %d %d, absorb %ld drop %ld both %ld\n", rows, met,
           CK_ER_ROWS, want, leaders_hist[0], leaders_hist[1], leaders_hist[2], leaders_hist[3], leaders_hist[4], absorbs, drops, both);
    return 0;
}
