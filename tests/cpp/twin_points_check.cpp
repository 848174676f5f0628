// Host check of the packed boundary point's twin encoding (chalkydri_amd/csrc/ck_point.h), run by tests/test_twin_points_host.py.
// A twin is the point (2x+1, 2y+1) emitted twice into one cluster: by direction (1,1) from pixel (x, y) and by direction (-1,1)
// from pixel (x+1, y).  That happens on the four 2 x 2 blocks whose rows or columns are uniform and of opposite colour; each is
// tried at the smallest and at the largest coordinates the 13-bit fields hold: eight merged words.  For each, the two points the
// oracle's emit rule (oracle/detector.c: ora_clusters) makes of the block must come back from ck_unpack_point + ck_unpack_twin,
// ck_stage_point must carry their coordinates and the SUM of their gradients, and the word without the twin bits must unpack and
// stage as it always did.
#include <cstdio>
#include <cstdlib>

#include "ck_point.h"

struct Pt { int x, y, gx, gy; };

// the oracle's rule for the pair (x, y) -> (x + dx, y + dy) with threshold values v0, v1 (0 or 255)
static Pt oracle_point(int x, int y, int dx, int dy, int v0, int v1) {
    const int s = v1 - v0 > 0 ? 1 : -1;
    return Pt{2 * x + dx, 2 * y + dy, dx * s, dy * s};
}

static int fails = 0;
static void expect(bool ok, const char *what, int block, int x, int y) {
    if (!ok) { fails++; printf("FAIL %s (block %d at %d,%d)\n", what, block, x, y); }
}
static bool same(const ck_cluster_point_t &p, const Pt &q) { return p.x == q.x && p.y == q.y && p.gx == q.gx && p.gy == q.gy && p.pad == 0; }

int main() {
    // t[row][column] of the block at (x, y): uniform rows (a horizontal edge) and uniform columns (a vertical edge), either polarity
    static const int blocks[4][2][2] = {{{0, 0}, {255, 255}}, {{255, 255}, {0, 0}}, {{0, 255}, {0, 255}}, {{255, 0}, {255, 0}}};
    static const int at[2][2] = {{1, 1}, {4094, 4094}}; // 2x + 1 = 3 and 8189 < 2^13
    int seen_sums = 0;
    for (int b = 0; b < 4; b++)
        for (int q = 0; q < 2; q++) {
            const int x = at[q][0], y = at[q][1];
            const int (*t)[2] = blocks[b];
            const Pt first = oracle_point(x, y, 1, 1, t[0][0], t[1][1]);       // direction (1,1) from (x, y)
            const Pt second = oracle_point(x + 1, y, -1, 1, t[0][1], t[1][0]); // direction (-1,1) from (x+1, y)
            expect(first.x == second.x && first.y == second.y, "the two points share their coordinates", b, x, y);
            // the word as k_emit2 forms it: coordinates, direction 3, sign = the first pair's neighbour is white; twin bit; twin
            // sign = the second pair's neighbour (x, y+1) is white
            const ck_packed_point plain = ((uint32_t)(2 * x + 1) << 16) | ((uint32_t)(2 * y + 1) << 3) | (3u << 1) | (t[1][1] > t[0][0] ? 1u : 0u);
            const ck_packed_point v = plain | CK_PT_TWIN | (t[1][0] > t[0][1] ? CK_PT_TWIN_SIGN : 0u);
            expect(same(ck_unpack_point(v), first), "ck_unpack_point gives the first point", b, x, y);
            expect(same(ck_unpack_twin(v), second), "ck_unpack_twin gives the second point", b, x, y);
            expect(same(ck_unpack_point(plain), first), "the plain word unpacks as before", b, x, y);
            const unsigned long long s = ck_stage_point(v), sp = ck_stage_point(plain);
            const int sgx = (int)(signed char)((s >> 32) & 0xFF), sgy = (int)(signed char)((s >> 40) & 0xFF);
            expect((int)(s & 0xFFFF) == first.x && (int)((s >> 16) & 0xFFFF) == first.y && (s >> 48) == 0, "staged coordinates", b, x, y);
            expect(sgx == first.gx + second.gx && sgy == first.gy + second.gy, "staged gradient is the sum of the two", b, x, y);
            expect((int)(signed char)((sp >> 32) & 0xFF) == first.gx && (int)(signed char)((sp >> 40) & 0xFF) == first.gy &&
                   (sp & 0xFFFFFFFFull) == (s & 0xFFFFFFFFull), "the plain word stages as before", b, x, y);
            // the sums are (+-2, 0) for the vertical edges and (0, +-2) for the horizontal ones
            expect((abs(sgx) == 2 && sgy == 0) || (sgx == 0 && abs(sgy) == 2), "sum of a twin's gradients", b, x, y);
            seen_sums |= 1 << ((sgx == 2) ? 0 : (sgx == -2) ? 1 : (sgy == 2) ? 2 : 3);
        }
    expect(seen_sums == 15, "all four gradient sums occur", -1, 0, 0);
    if (fails) return 1;
    printf("OK 8 merged encodings\n");
    return 0;
}
