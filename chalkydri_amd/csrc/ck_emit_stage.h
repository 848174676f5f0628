// ck_emit_stage.h — who stages what in k_emit2 (k_clusters.hip) when the tile is staged in aligned groups of four pixels.
//
// A workgroup of 256 threads stages the 17 x 66 region around its 64 x 16 emit tile at (x0, y0): staged column lx = 0..65 is frame
// column x0 - 1 + lx, staged row ly = 0..16 is frame row y0 + ly.  A staged cell is one word: the frame pixel of its component's
// root | a colour bit, or SKIP.  The per-pixel staging gives thread t the cells t + 256 q of the region and pays, for each of them, a
// division by 66, the clamps, two addresses, a byte load and a 16-bit load, and the tile terms of ck_label_slot and
// ck_label_interior_root (ck_internal.h).  Four pixels of one frame row that start at a multiple of four lie in one CCL tile
// (128 x 32) and in one emit tile; their threshold bytes are one dword and their label words one 8-byte word.  So, when the frame's
// width is a multiple of four (then every row starts at a multiple of four as well, and so does every frame of a batch):
//   round 0  every thread one group: t -> row t >> 4, group t & 15: the tile's own 64 x 16 pixels, no division;
//   round 1  the 98 cells left, one pixel per thread as the per-pixel staging does it, in waves 0 and 1: the bottom halo row's own
//            64 pixels (threads 0..63) and the 34 pixels of the two halo columns, rows 0..16 (threads 64..97).  A round costs a
//            wave its instructions whatever the number of lanes at work, and a workgroup's staging ends with its slowest wave: a
//            second round of groups in one wave (16 groups and 34 halo pixels are 50 items) made that wave as slow as all four were
//            before, and the kernel no faster; a pixel round is well under half a group round.
// A group's start is clamped to [0, w - 4] and its row to [0, h - 1]; a group is wholly inside the frame or wholly outside it
// (one bit masks it); a single pixel is clamped to [0, w - 1] x [0, h - 1]: no load touches an element outside [0, w * h) of its frame.
// LDS: staged cell (ly, lx) is word 68 ly + 3 + lx, so a group's four words (lx = 1 + 4 g) start at 68 ly + 4 + 4 g: one 16-byte
// aligned ds_write_b128.  17 rows of 68 words and the last row's right halo at word 1 156: below the 1 280 words the per-pixel
// layout takes.  The count pass reads through the same function (ck_es_word).
// This file is the one text of that index arithmetic; tests/cpp/emit_stage_check.cpp checks it exhaustively on the host.
// Plain C++17: a host program includes this file without the HIP headers.
#ifndef CK_EMIT_STAGE_H
#define CK_EMIT_STAGE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define CK_ES_HD __host__ __device__ __forceinline__
#else
#define CK_ES_HD inline
#endif

constexpr int CK_ES_NT = 256;                                    // threads of the workgroup
constexpr int CK_ES_TW = 64, CK_ES_TH = 16;                      // the emit tile
constexpr int CK_ES_LW = CK_ES_TW + 2, CK_ES_LH = CK_ES_TH + 1;  // the staged region
constexpr int CK_ES_STRIDE = 68, CK_ES_COL0 = 3;                 // LDS words per staged row, word of staged column 0
constexpr int CK_ES_WORDS = CK_ES_STRIDE * (CK_ES_LH - 1) + CK_ES_COL0 + CK_ES_LW; // one past the last word written
constexpr int CK_ES_ROUND1 = CK_ES_TW + 2 * CK_ES_LH;            // pixels of round 1 (threads 0..97)
constexpr int CK_ES_ROUND1_WAVES = (CK_ES_ROUND1 + 63) / 64;     // ... which are the first two waves
// the segmentation stage's tiles and label words (the kernel asserts these against ck_internal.h)
constexpr int CK_ES_CCL_TW = 128, CK_ES_CCL_TH = 32, CK_ES_RING_CAP = 2 * (CK_ES_CCL_TW + CK_ES_CCL_TH);
constexpr uint32_t CK_ES_LBL_BORDER = 0x8000u, CK_ES_LBL_SMALL = 0x4000u, CK_ES_LBL_ID_MASK = 0x01FFu;
constexpr uint32_t CK_ES_SKIP = 0xFFFFFFFFu, CK_ES_WHITE = 0x40000000u;

// the group path is taken for the whole launch or not at all
CK_ES_HD bool ck_es_group_path(int w) { return w >= 4 && (w & 3) == 0; }

// LDS word of staged cell (ly, lx)
CK_ES_HD int ck_es_word(int ly, int lx) { return ly * CK_ES_STRIDE + CK_ES_COL0 + lx; }

struct ck_es_item {
    int ly, lx; // staged cell: a group's first pixel, or the single pixel
    int cx, cy; // the load: frame column (a group's: a multiple of 4 in [0, w - 4]; a pixel's: in [0, w - 1]) and row (in [0, h - 1])
    bool keep;  // the item is staged (round 1, threads 98..127: not; they load like thread 97)
    bool inb;   // the group / the pixel lies inside the frame (else its cells are SKIP)
};

// round 0: thread t of all 256, one group
CK_ES_HD ck_es_item ck_es_round0(int t, int x0, int y0, int w, int h) {
    ck_es_item it;
    it.ly = t >> 4; it.lx = 1 + 4 * (t & 15); it.keep = true;
    const int gx = x0 - 1 + it.lx, gy = y0 + it.ly; // (gx >= 0: a tile's own pixels)
    it.inb = gx < w && gy < h;
    it.cx = gx > w - 4 ? w - 4 : gx;
    it.cy = gy > h - 1 ? h - 1 : gy;
    return it;
}

// round 1: thread t of the first two waves (t = 0..127), one pixel
CK_ES_HD ck_es_item ck_es_round1(int t, int x0, int y0, int w, int h) {
    ck_es_item it;
    const int j = t - CK_ES_TW < 2 * CK_ES_LH ? t - CK_ES_TW : 2 * CK_ES_LH - 1;
    const bool right = j >= CK_ES_LH;
    it.ly = t < CK_ES_TW ? CK_ES_LH - 1 : (right ? j - CK_ES_LH : j);
    it.lx = t < CK_ES_TW ? 1 + t : (right ? CK_ES_LW - 1 : 0);
    it.keep = t < CK_ES_ROUND1;
    const int gx = x0 - 1 + it.lx, gy = y0 + it.ly;
    it.inb = gx >= 0 && gx < w && gy < h;
    it.cx = gx < 0 ? 0 : (gx > w - 1 ? w - 1 : gx);
    it.cy = gy > h - 1 ? h - 1 : gy;
    return it;
}

// where an item's words go: a group's four from here on, a pixel's one
CK_ES_HD int ck_es_item_word(const ck_es_item &it) { return ck_es_word(it.ly, it.lx); }

// ---- what a group forms once for its four pixels: the tile terms of ck_label_slot and ck_label_interior_root -----------------------
CK_ES_HD uint32_t ck_es_slot_base(int cx, int cy, int ccl_tiles_x) {
    // (cx and cy are clamped into the frame: not negative, so the divisions are shifts)
    return (((uint32_t)cy / (uint32_t)CK_ES_CCL_TH) * (uint32_t)ccl_tiles_x + (uint32_t)cx / (uint32_t)CK_ES_CCL_TW) * (uint32_t)CK_ES_RING_CAP;
}
CK_ES_HD uint32_t ck_es_root_base(int cx, int cy, int w) { return (uint32_t)(cy & ~(CK_ES_CCL_TH - 1)) * (uint32_t)w + (uint32_t)(cx & ~(CK_ES_CCL_TW - 1)); }

// ---- what stays per pixel ----------------------------------------------------------------------------------------------------------
// the slot whose root and size the pixel gathers (entry 0, a harmless read, where it needs none)
CK_ES_HD uint32_t ck_es_pixel_slot(uint32_t lab, uint32_t tv, bool inb, uint32_t slot_base) {
    const bool two = inb && tv != 127u && !(lab & CK_ES_LBL_SMALL) && (lab & CK_ES_LBL_BORDER);
    return two ? slot_base + (lab & CK_ES_LBL_ID_MASK) : 0u;
}
// the staged word, from the label word, the threshold byte and the two gathered values
CK_ES_HD uint32_t ck_es_pixel_word(uint32_t lab, uint32_t tv, bool inb, uint32_t hop, uint32_t csz, uint32_t root_base, int w, int min_comp) {
    const bool brd = (lab & CK_ES_LBL_BORDER) != 0u;
    const bool none = !inb || tv == 127u || (lab & CK_ES_LBL_SMALL) || (brd && (int)csz < min_comp);
    const uint32_t root = brd ? hop : root_base + ((lab >> 7) & (uint32_t)(CK_ES_CCL_TH - 1)) * (uint32_t)w + (lab & (uint32_t)(CK_ES_CCL_TW - 1));
    return none ? CK_ES_SKIP : (root | (tv == 255u ? CK_ES_WHITE : 0u));
}

#endif
