// The packed boundary point of the cluster and quad-fit stages (k_clusters.hip, k_quads.hip, ck_stages.hip).  Plain C++: a host
// program includes it without the HIP headers (tests/cpp/twin_points_check.cpp).
#ifndef CK_POINT_H
#define CK_POINT_H

#include <stdint.h>

#include "chalkydri_hip.h"

#if defined(__HIPCC__)
#define CK_PT_HD __host__ __device__
#else
#define CK_PT_HD
#endif

// A boundary point inside the pipeline, packed into 32 bits: [twin sign:1][twin:1][x:13][y:13][direction:2][sign:1] at bits 30, 29,
// 28..16, 15..3, 2..1, 0 (bit 31 unused).  x/y are half-pixel coordinates, direction = which of the four forward neighbours
// (1,0),(0,1),(-1,1),(1,1) the pair spans, sign = 1 when the gradient points along it.  k_emit2 writes the points of one
// (tile, cluster) run next to each other; k_scatter moves whole runs to their place inside the cluster; k_fit unpacks.
// A TWIN point (k_emit2) stands for two points of one cluster at the same (odd, odd) coordinates: its own, of direction (1,1) from
// pixel (x, y), and the one of direction (-1,1) from pixel (x+1, y), whose sign is the twin sign bit.  A cluster then has two
// counts: the LOGICAL one (a twin counts twice: what the size gates, the overflow bits and ck_clusters_batch go by) and the PHYSICAL
// one (words stored: offsets, ck_cluster_t::start / count on the device, the fit's classes).
typedef uint32_t ck_packed_point;
constexpr uint32_t CK_PT_TWIN = 1u << 29, CK_PT_TWIN_SIGN = 1u << 30;
CK_PT_HD inline ck_cluster_point_t ck_unpack_point(ck_packed_point v) {
    const int k = (int)(v >> 1) & 3, sgn = (v & 1u) ? 1 : -1;
    const int dx = k == 2 ? -1 : (k == 1 ? 0 : 1), dy = k == 0 ? 0 : 1;
    ck_cluster_point_t p;
    p.x = (uint16_t)((v >> 16) & 0x1FFFu); p.y = (uint16_t)((v >> 3) & 0x1FFFu);
    p.gx = (int8_t)(dx * sgn); p.gy = (int8_t)(dy * sgn); p.pad = 0;
    return p;
}
// the second point of a twin (only where v & CK_PT_TWIN): same coordinates, direction (-1,1), its own sign
CK_PT_HD inline ck_cluster_point_t ck_unpack_twin(ck_packed_point v) {
    const int sgn = (v & CK_PT_TWIN_SIGN) ? 1 : -1;
    ck_cluster_point_t p;
    p.x = (uint16_t)((v >> 16) & 0x1FFFu); p.y = (uint16_t)((v >> 3) & 0x1FFFu);
    p.gx = (int8_t)(-sgn); p.gy = (int8_t)sgn; p.pad = 0;
    return p;
}
// The same fields in one word, the staged form the quad fit's sort reads: x | y << 16 | (u8)gx << 32 | (u8)gy << 40.  A twin
// carries the SUM of its two gradients: the border-direction sum, the only reader of gx / gy, is linear in them.
CK_PT_HD inline __attribute__((always_inline)) unsigned long long ck_stage_point(ck_packed_point v) {
    const ck_cluster_point_t p = ck_unpack_point(v);
    const int tw = (int)(v >> 29) & 1, tsg = (int)((v >> 30) & 1) * 2 - 1;
    const int gx = p.gx - tw * tsg, gy = p.gy + tw * tsg;
    return (unsigned long long)p.x | ((unsigned long long)p.y << 16) | ((unsigned long long)(uint8_t)gx << 32) | ((unsigned long long)(uint8_t)gy << 40);
}

#endif
