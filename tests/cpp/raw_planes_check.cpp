// raw_planes_check.cpp — CPU check of chalkydri_amd/csrc/ck_raw_planes.h: the plane map, the plane copy of ck_upload_raw /
// ck_ingest_write and the triple of a pixel, for the four planar layouts x four turns x the shapes of tests/test_raw_planes_host.py at
// the minimum stride, minimum + 2 and minimum + 16.
//
// A frame is built here from three arrays Y[sh][sw], Cb[ch][cw], Cr[ch][cw] by the layout's own words, not through the
// header; the header's map must then find every sample, under every turn, and a copy into another stride must carry every sample and
// nothing else.  Every source buffer is malloc'ed to exactly stride * (sh + ch) bytes and every destination to exactly its own, so
// one byte read or written outside ends the program under AddressSanitizer; the destination starts as 0xEE and the bytes no plane
// holds must still be 0xEE afterwards.  Built with -fsanitize=address,undefined (Makefile: raw_planes_check); no GPU, no library.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ck_raw_planes.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 10) { printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint8_t y_of(int u, int v) { return (uint8_t)(u * 7 + v * 13 + 1); }
static uint8_t cb_of(int i, int j) { return (uint8_t)((i * 5 + j * 3) & 127); }        // 0..127
static uint8_t cr_of(int i, int j) { return (uint8_t)(128 + ((i * 11 + j * 17) & 127)); } // 128..255: a swapped order shows

// the frame by the words of the layout; `used` marks the bytes a plane holds
static void build(int kind, int sw, int sh, int stride, uint8_t *buf, uint8_t *used, uint8_t pad) {
    const int cw = (sw + 1) / 2, ch = (sh + 1) / 2;
    const size_t bytes = (size_t)stride * (sh + ch);
    memset(buf, pad, bytes);
    memset(used, 0, bytes);
    for (int v = 0; v < sh; v++)
        for (int u = 0; u < sw; u++) { buf[(size_t)v * stride + u] = y_of(u, v); used[(size_t)v * stride + u] = 1; }
    const size_t base = (size_t)stride * sh;
    for (int j = 0; j < ch; j++)
        for (int i = 0; i < cw; i++) {
            size_t b, r;
            if (kind == CKP_NV12 || kind == CKP_NV21) {
                b = base + (size_t)j * stride + 2 * i + (kind == CKP_NV21);
                r = base + (size_t)j * stride + 2 * i + (kind == CKP_NV12);
            } else {
                const size_t half = stride / 2, p0 = base + (size_t)j * half + i, p1 = base + half * ch + (size_t)j * half + i;
                b = kind == CKP_I420 ? p0 : p1;
                r = kind == CKP_I420 ? p1 : p0;
            }
            buf[b] = cb_of(i, j); buf[r] = cr_of(i, j); used[b] = used[r] = 1;
        }
}

static void check_triples(const ckp_map &m, const uint8_t *buf, int W, int H, int turn, const char *what) {
    for (int oy = 0; oy < H; oy++)
        for (int ox = 0; ox < W; ox++) {
            int32_t u, v;
            ckp_source_xy(turn, m.sw, m.sh, ox, oy, &u, &v);
            // the index maps of §4d, restated
            const int eu = turn == 0 ? ox : turn == 1 ? oy : turn == 2 ? m.sw - 1 - ox : m.sw - 1 - oy;
            const int ev = turn == 0 ? oy : turn == 1 ? m.sh - 1 - ox : turn == 2 ? m.sh - 1 - oy : ox;
            CHECK(u == eu && v == ev, "%s turn %d (%d,%d)", what, turn, ox, oy);
            uint8_t t[3];
            ckp_triple(&m, buf, u, v, t);
            CHECK(t[0] == y_of(eu, ev) && t[1] == cb_of(eu >> 1, ev >> 1) && t[2] == cr_of(eu >> 1, ev >> 1), "%s turn %d (%d,%d): %d %d %d", what, turn,
                  ox, oy, t[0], t[1], t[2]);
        }
}

int main() {
    static const int shapes[][2] = {{16, 16}, {17, 19}, {34, 18}, {641, 479}, {17, 4095}, {1, 1}, {2, 2}};
    static const int extra[] = {0, 2, 16};
    long maps = 0;
    for (const auto &wh : shapes)
        for (int kind = CKP_NV12; kind <= CKP_YV12; kind++)
            for (int turn = 0; turn < 4; turn++) {
                const int W = wh[0], H = wh[1], sw = (turn & 1) ? H : W, sh = (turn & 1) ? W : H;
                const int cw = (sw + 1) / 2, ch = (sh + 1) / 2, ms = ckp_min_stride(sw);
                CHECK(ms == 2 * cw, "min stride");
                ckp_map bad;
                CHECK(ckp_map_make(kind, sw, sh, ms - 1, &bad) != 0, "a stride below the minimum");
                if (kind >= CKP_I420) CHECK(ckp_map_make(kind, sw, sh, ms + 1, &bad) != 0, "an odd stride of a split layout");
                for (int e : extra) {
                    const int stride = ms + e;
                    const size_t bytes = (size_t)stride * (sh + ch);
                    uint8_t *src = (uint8_t *)malloc(bytes), *used = (uint8_t *)malloc(bytes);
                    build(kind, sw, sh, stride, src, used, 0x5A);
                    ckp_map m;
                    CHECK(ckp_map_make(kind, sw, sh, stride, &m) == 0, "map");
                    maps++;
                    CHECK(m.bytes == (int64_t)bytes && m.sw == sw && m.sh == sh && m.cw == cw && m.ch == ch, "sizes");
                    const bool nv = kind <= CKP_NV21, cb_first = kind == CKP_NV12 || kind == CKP_I420;
                    const int64_t base = (int64_t)stride * sh, second = nv ? base + 1 : base + (int64_t)(stride / 2) * ch;
                    CHECK(m.c[0].off == 0 && m.c[1].off == (cb_first ? base : second) && m.c[2].off == (cb_first ? second : base), "offsets");
                    CHECK(m.c[0].row_stride == stride && m.c[1].row_stride == (nv ? stride : stride / 2) && m.c[2].row_stride == m.c[1].row_stride, "row strides");
                    CHECK(m.c[0].step == 1 && m.c[1].step == (nv ? 2 : 1) && m.c[2].step == m.c[1].step, "steps");
                    // the extent ends with the last byte a plane holds
                    size_t last = 0;
                    for (size_t k = 0; k < bytes; k++) if (used[k]) last = k;
                    CHECK((size_t)ckp_extent(&m) == last + 1 && ckp_extent(&m) <= m.bytes, "extent %lld", (long long)ckp_extent(&m));
                    if ((long)W * H <= 641L * 479) check_triples(m, src, W, H, turn, "source");
                    else if (turn == 0) check_triples(m, src, W, H, turn, "source");
                    // the copy: into the 16-rounded staging stride, into the same stride, into the minimum
                    const int dstrides[3] = {(ms + 15) / 16 * 16, stride, ms};
                    for (int ds : dstrides) {
                        const size_t dbytes = (size_t)ds * (sh + ch);
                        uint8_t *dst = (uint8_t *)malloc(dbytes), *dused = (uint8_t *)malloc(dbytes), *want = (uint8_t *)malloc(dbytes);
                        memset(dst, 0xEE, dbytes);
                        ckp_copy(kind, sw, sh, src, stride, dst, ds);
                        build(kind, sw, sh, ds, want, dused, 0xEE);
                        size_t wrong = 0, touched = 0;
                        for (size_t k = 0; k < dbytes; k++) {
                            if (dused[k]) wrong += dst[k] != want[k];
                            else if (ds != stride) touched += dst[k] != 0xEE; // (equal strides copy the rows' padding with them)
                        }
                        CHECK(wrong == 0 && touched == 0, "copy %d -> %d: %zu wrong, %zu touched", stride, ds, wrong, touched);
                        free(dst); free(dused); free(want);
                    }
                    free(src); free(used);
                }
            }
    // the two worked examples of the contract: 17 x 19 turned clockwise, stride 24
    ckp_map m;
    CHECK(ckp_map_make(CKP_I420, 19, 17, 24, &m) == 0 && m.cw == 10 && m.ch == 9 && m.c[1].off == 408 && m.c[2].off == 516 && m.c[1].row_stride == 12 &&
          m.bytes == 624, "I420 example");
    CHECK(ckp_map_make(CKP_NV21, 19, 17, 24, &m) == 0 && m.c[1].off == 409 && m.c[2].off == 408 && m.c[1].row_stride == 24 && m.c[1].step == 2, "NV21 example");
    if (fails) { printf("raw_planes_check: %d failures\n", fails); return 1; }
    printf("raw_planes_check ok: %ld maps\n", maps);
    return 0;
}
