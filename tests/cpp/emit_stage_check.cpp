// emit_stage_check.cpp — CPU check of chalkydri_amd/csrc/ck_emit_stage.h: which thread of k_emit2 stages which cells of the 17 x 66
// region in which round when the tile is staged in aligned groups of four pixels, what it loads for them and where it writes them,
// against the per-pixel staging the kernel keeps for widths that are no multiple of four (transcribed below from that kernel).
//
// Every width 16, 20, ... 272 and every height 16..70 (one to five emit-tile columns and rows, the CCL-tile seams at x = 128 and
// 256 and at y = 32 and 64, ragged last groups and rows), every emit tile, every thread, both rounds:
//   1  every cell of the region is written exactly once, from the frame pixel the per-pixel staging reads for it, or masked where
//      that one masks it;
//   2  every load lies inside [0, w * h) of its frame, and a group's is aligned — 4 bytes for the threshold bytes, 8 for the label
//      words — given a 256-byte aligned buffer, for the first, an odd and the last frame of a batch;
//   3  the LDS words are distinct, below the kernel's SR_PAD, and a whole group's first word is a multiple of four;
//   4  the per-group tile terms and the per-pixel functions give, for each of the group's pixels, the words ck_label_slot and
//      ck_label_interior_root give at the pixel's own coordinates (label words: ring-touching ids 0 and 511, interior roots at the
//      CCL tile's four corners, SMALL, NONE; threshold bytes 0, 127, 255; sizes either side of min_component_px);
//   5  the count pass's read of (row0 + r, lx - 1 + c) lands on the word staging wrote for that cell;
//   6  widths that are no multiple of four take the per-pixel path.
// Built with -fsanitize=address,undefined (Makefile: emit_stage_check); no GPU, no library.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "ck_emit_stage.h"

static long fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 10) { printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// ---- the kernel's per-pixel text (k_clusters.hip, ck_internal.h; names and expressions kept) ---------------------------------------
static const int NT = 256, ETW = 64, ETH = 16, LW = ETW + 2, LH = ETH + 1;
static const int SR_PAD = ((LH * LW + NT - 1) / NT) * NT;
static const uint32_t SKIP = 0xFFFFFFFFu, ID_WHITE = 0x40000000u;
static const uint32_t CK_LBL_BORDER = 0x8000u, CK_LBL_SMALL = 0x4000u, CK_LBL_ID_MASK = 0x01FFu;
static const int CK_TW = 128, CK_TH = 32, CK_RING_CAP = 2 * (CK_TW + CK_TH);
static uint32_t ck_label_slot(uint32_t l, int x, int y, int ccl_tiles_x) {
    return (uint32_t)((y / CK_TH) * ccl_tiles_x + x / CK_TW) * (uint32_t)CK_RING_CAP + (l & CK_LBL_ID_MASK);
}
static uint32_t ck_label_interior_root(uint32_t l, int x, int y, int w) {
    return (uint32_t)((y & ~(CK_TH - 1)) + (int)((l >> 7) & (CK_TH - 1))) * (uint32_t)w + (uint32_t)((x & ~(CK_TW - 1)) + (int)(l & (CK_TW - 1)));
}
struct OldPixel { bool inb; int cx, cy; uint32_t p; };
static OldPixel old_pixel(int i, int x0, int y0, int w, int h) {
    OldPixel o;
    const int ly = i / LW, lx = i - ly * LW;
    const int gy = y0 + ly, gx = x0 - 1 + lx;
    o.inb = i < LH * LW && gy < h && gx >= 0 && gx < w;
    o.cy = gy < h - 1 ? gy : h - 1; o.cx = (gx > 0 ? gx : 0) < w - 1 ? (gx > 0 ? gx : 0) : w - 1;
    o.p = (uint32_t)o.cy * (uint32_t)w + (uint32_t)o.cx;
    return o;
}
static uint32_t old_slot(uint32_t lab, uint32_t tv, bool inb, int gxs, int gys, int ccl_tiles_x) {
    const bool two = inb && tv != 127u && !(lab & CK_LBL_SMALL) && (lab & CK_LBL_BORDER);
    return two ? ck_label_slot(lab, gxs, gys, ccl_tiles_x) : 0u;
}
static uint32_t old_word(uint32_t lab, uint32_t tv, bool inb, uint32_t hop, uint32_t csz, int gxs, int gys, int w, int min_comp) {
    const bool brd = (lab & CK_LBL_BORDER) != 0u;
    const bool none = !inb || tv == 127u || (lab & CK_LBL_SMALL) || (brd && (int)csz < min_comp);
    const uint32_t root = brd ? hop : ck_label_interior_root(lab, gxs, gys, w);
    return none ? SKIP : (root | (tv == 255u ? ID_WHITE : 0u));
}

static const uint32_t LABELS[] = {CK_LBL_BORDER | 0u, CK_LBL_BORDER | 511u, 0u, 127u, 31u << 7, (31u << 7) | 127u, CK_LBL_SMALL | (5u << 7) | 9u, 0xFFFFu};
static const uint32_t TVS[] = {0u, 127u, 255u};

struct Cell { int n; bool inb; uint32_t p; int word; };

static long groups_checked = 0, pixels_checked = 0;
static std::vector<uint8_t> g_seen;
static int g_seen_w = -1;

// nw: 4 a group (round 0), 1 a single pixel (round 1)
static void check_item(const ck_es_item &it, int nw, int x0, int y0, int w, int h, Cell cells[LH][LW], std::vector<int> &lds) {
    const long npix = (long)w * h;
    // 2: the load (also of a thread that stages nothing: it loads all the same)
    CHECK(it.cx >= 0 && it.cx <= w - nw && it.cy >= 0 && it.cy <= h - 1, "w %d h %d cx %d cy %d", w, h, it.cx, it.cy);
    const long p0 = (long)it.cy * w + it.cx;
    CHECK(p0 >= 0 && p0 + nw <= npix, "w %d h %d p0 %ld", w, h, p0);
    if (nw == 4)
        for (long frame : {0l, 1l, 2l, 254l, 255l}) {
            const long e = frame * npix + p0; // element offset from the 256-byte aligned buffer
            CHECK((it.cx & 3) == 0 && e % 4 == 0, "T: w %d h %d frame %ld", w, h, frame);
            CHECK((2 * e) % 8 == 0, "L: w %d h %d frame %ld", w, h, frame);
        }
    if (!it.keep) return;
    groups_checked++;
    // 3: the LDS words
    const int word = ck_es_item_word(it);
    if (nw == 4) CHECK((word & 3) == 0, "group word %d", word);
    for (int j = 0; j < nw; j++) {
        CHECK(word + j >= 0 && word + j < SR_PAD && word + j < CK_ES_WORDS, "word %d", word + j);
        if (word + j >= 0 && word + j < SR_PAD) lds[(size_t)(word + j)]++;
    }
    // 1: the cells, and 4: the tile terms
    const int ccl_tiles_x = (w + CK_TW - 1) / CK_TW;
    const uint32_t slot_base = ck_es_slot_base(it.cx, it.cy, ccl_tiles_x), root_base = ck_es_root_base(it.cx, it.cy, w);
    for (int j = 0; j < nw; j++) {
        const int ly = it.ly, lx = it.lx + j;
        CHECK(ly >= 0 && ly < LH && lx >= 0 && lx < LW, "cell %d %d", ly, lx);
        if (!(ly >= 0 && ly < LH && lx >= 0 && lx < LW)) continue;
        Cell &c = cells[ly][lx];
        c.n++; c.inb = it.inb; c.p = (uint32_t)p0 + (uint32_t)j;
        c.word = word + j;
        pixels_checked++;
        const OldPixel o = old_pixel(ly * LW + lx, x0, y0, w, h);
        if (!it.inb) continue;
        const int px = it.cx + j, py = it.cy; // the pixel's own coordinates: what the per-pixel staging hands to the two functions
        CHECK(o.cx == px && o.cy == py, "w %d h %d tile %d %d cell %d %d", w, h, x0, y0, ly, lx);
        // (a pixel inside the frame always lies in the same group, whatever the height and whichever tile stages it: once per width)
        if (g_seen_w != w) { g_seen_w = w; g_seen.assign((size_t)w * 70, 0); }
        if (g_seen[(size_t)py * w + px]) continue;
        g_seen[(size_t)py * w + px] = 1;
        for (uint32_t lab : LABELS)
            for (uint32_t tv : TVS)
                for (uint32_t csz : {3u, 40u}) {
                    const uint32_t hop = 0x123456u;
                    const uint32_t s_new = ck_es_pixel_slot(lab, tv, it.inb, slot_base), s_old = old_slot(lab, tv, o.inb, px, py, ccl_tiles_x);
                    CHECK(s_new == s_old, "slot: w %d h %d px %d py %d lab %x tv %u: %u != %u", w, h, px, py, lab, tv, s_new, s_old);
                    const uint32_t w_new = ck_es_pixel_word(lab, tv, it.inb, hop, csz, root_base, w, 25), w_old = old_word(lab, tv, o.inb, hop, csz, px, py, w, 25);
                    CHECK(w_new == w_old, "word: w %d h %d px %d py %d lab %x tv %u: %x != %x", w, h, px, py, lab, tv, w_new, w_old);
                }
        // (and with the tile term of the slot alone, for both ends of the id range)
        CHECK(slot_base + 511u == ck_label_slot(CK_LBL_BORDER | 511u, px, py, ccl_tiles_x) && slot_base == ck_label_slot(CK_LBL_BORDER, px, py, ccl_tiles_x), "slot base");
    }
}

static void check_tile(int x0, int y0, int w, int h) {
    static Cell cells[LH][LW];
    for (int ly = 0; ly < LH; ly++) for (int lx = 0; lx < LW; lx++) cells[ly][lx] = Cell{0, false, 0u, -1};
    std::vector<int> lds((size_t)SR_PAD, 0);
    for (int t = 0; t < NT; t++) {
        const ck_es_item it = ck_es_round0(t, x0, y0, w, h);
        CHECK(it.keep, "round 0 stages every group");
        check_item(it, 4, x0, y0, w, h, cells, lds);
    }
    int staged1 = 0;
    for (int t = 0; t < 64 * CK_ES_ROUND1_WAVES; t++) { // round 1: the first two waves
        const ck_es_item it = ck_es_round1(t, x0, y0, w, h);
        CHECK(it.keep == (t < CK_ES_ROUND1), "round 1: thread %d", t);
        staged1 += it.keep;
        check_item(it, 1, x0, y0, w, h, cells, lds);
    }
    CHECK(staged1 == 98 && CK_ES_ROUND1_WAVES == 2, "round 1 has %d items", staged1);
    for (size_t i = 0; i < lds.size(); i++) CHECK(lds[i] <= 1, "LDS word %zu written %d times", i, lds[i]);
    for (int ly = 0; ly < LH; ly++)
        for (int lx = 0; lx < LW; lx++) {
            const Cell &c = cells[ly][lx];
            const OldPixel o = old_pixel(ly * LW + lx, x0, y0, w, h);
            CHECK(c.n == 1, "w %d h %d tile %d %d cell %d %d written %d times", w, h, x0, y0, ly, lx, c.n);
            CHECK(c.inb == o.inb, "w %d h %d tile %d %d cell %d %d inb %d != %d", w, h, x0, y0, ly, lx, (int)c.inb, (int)o.inb);
            if (o.inb) CHECK(c.p == o.p, "w %d h %d tile %d %d cell %d %d pixel %u != %u", w, h, x0, y0, ly, lx, c.p, o.p);
            CHECK(c.word == ck_es_word(ly, lx), "cell %d %d at word %d", ly, lx, c.word);
        }
    // 5: the count pass: thread tid reads rows row0 .. row0 + 4, staged columns lx - 1 .. lx + 1
    for (int tid = 0; tid < NT; tid++) {
        const int lx = (tid & 63) + 1, row0 = (tid >> 6) * 4;
        for (int r = 0; r < 5; r++)
            for (int c = 0; c < 3; c++) {
                const int rd = ck_es_word(row0 + r, lx - 1 + c);
                CHECK(row0 + r < LH && rd == cells[row0 + r][lx - 1 + c].word && lds[(size_t)rd] == 1, "count pass: tid %d r %d c %d", tid, r, c);
            }
    }
}

int main() {
    static_assert(CK_ES_NT == NT && CK_ES_TW == ETW && CK_ES_TH == ETH && CK_ES_LW == LW && CK_ES_LH == LH, "the kernel's geometry");
    static_assert(CK_ES_WORDS <= SR_PAD, "the ids keep their LDS");
    static_assert(CK_ES_SKIP == SKIP && CK_ES_WHITE == ID_WHITE && CK_ES_CCL_TW == CK_TW && CK_ES_CCL_TH == CK_TH && CK_ES_RING_CAP == CK_RING_CAP, "");
    long tiles = 0;
    for (int w = 16; w <= 272; w++) {
        CHECK(ck_es_group_path(w) == (w % 4 == 0), "w %d", w); // 6
        if (w % 4 != 0) continue;
        for (int h = 16; h <= 70; h++)
            for (int ty = 0; ty < (h + ETH - 1) / ETH; ty++)
                for (int tx = 0; tx < (w + ETW - 1) / ETW; tx++) { check_tile(tx * ETW, ty * ETH, w, h); tiles++; }
    }
    for (int w : {0, 1, 2, 3, 5, 6, 7}) CHECK(!ck_es_group_path(w), "w %d", w);
    if (fails) { printf("FAILED: %ld checks\n", fails); return 1; }
    printf("OK %ld tiles, %ld items, %ld staged pixels\n", tiles, groups_checked, pixels_checked);
    return 0;
}
