// rf_iso.hpp -- marching tetrahedra on the Delaunay mesh, one tetrahedron or one crossed edge at a time
// (rf_isosurface.hip; DESIGN.md, "Isosurface of an interpolated field"), in double.
//
// A per-site value interpolated linearly over every tetrahedron is a continuous field; its level set cuts a
// tetrahedron in a triangle (one or three corners inside) or a quad (two), whose corners lie on the tetrahedron's edges
// between an inside and an outside corner.  The corner on edge (a,b), a < b the two site indices, has the key
// a * 2^32 + b: every tetrahedron around the edge derives the same key, so equal keys weld without a tolerance.
//
//   inside        value > level, strictly; NaN is outside.  A tetrahedron with a value that is not finite emits nothing.
//   case rule     (i,j,k,l) is an even permutation of the row positions (0,1,2,3).  One corner inside: i is that corner,
//                 three inside: i is the corner outside; (j,k,l) are the rest, in the even order that starts with the
//                 lowest.  Two inside: i < j are the corners inside and (k,l) the corners outside in the one order that
//                 makes the permutation even.  Corner (x,y) being the crossing of the edge between positions x and y:
//                     one inside     (ij, ik, il)
//                     three inside   (ij, il, ik)
//                     two inside     the quad q = (ik, il, jl, jk) as (q0,q1,q2) and (q0,q2,q3)
//                 which, for a tetrahedron with det = d_1 . (d_2 x d_3) > 0 (d_i = p_i - p_0), winds every triangle
//                 counter-clockwise seen from the outside corners: its normal points from value > level to the rest.
//   winding       det < 0 swaps the last two corners of every triangle; zero and NaN count as positive.  The sign is
//                 taken once per tetrahedron from the sites, never from the interpolated positions.
//   vertex        t = (level - v_a) / (v_b - v_a),  x = p_a + t (p_b - p_a), in this order of operations.  v_a == v_b,
//                 a site out of range or a result that is not finite: NaN forward, nothing backward.
//   backward      for an upstream g, D = v_b - v_a, e = p_b - p_a:
//                     grad p_a = (1 - t) g,  grad p_b = t g,
//                     grad v_a = ((g . e) (level - v_b)) / D^2,  grad v_b = -(((g . e) (level - v_a)) / D^2)
//                 all eight dropped together when one of them is not finite.
//
// __host__ __device__, no HIP types: tests/host_harness/iso_host.cpp compiles this file with g++ (no FMA contraction on
// either side).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RF_ISO_HD __host__ __device__ __forceinline__
#else
#define RF_ISO_HD inline
#endif

namespace rf {
namespace iso {

constexpr int64_t kNoKey = -1;   // the key of a corner that cannot be written

RF_ISO_HD bool finite(double x) { return fabs(x) < (double)INFINITY; }

// bit c: corner c is inside; 0 when a value is not finite
RF_ISO_HD uint32_t tet_mask(double v0, double v1, double v2, double v3, double level) {
    if (!(finite(v0) && finite(v1) && finite(v2) && finite(v3))) return 0u;
    return (v0 > level ? 1u : 0u) | (v1 > level ? 2u : 0u) | (v2 > level ? 4u : 0u) | (v3 > level ? 8u : 0u);
}

// the triangles of a mask: 0, 1 or 2
RF_ISO_HD uint32_t mask_triangles(uint32_t mask) {
    const uint32_t m = mask & 15u, bits = (m & 1u) + ((m >> 1) & 1u) + ((m >> 2) & 1u) + (m >> 3);
    return bits == 0u || bits == 4u ? 0u : (bits == 2u ? 2u : 1u);
}

constexpr uint64_t perm_byte(uint64_t i, uint64_t j, uint64_t k, uint64_t l) { return i | (j << 2) | (k << 4) | (l << 6); }

// (i,j,k,l) of the case rule, two bits each from the low end, for masks 1 .. 14
RF_ISO_HD uint32_t mask_perm(uint32_t mask) {
    constexpr uint64_t lo = (perm_byte(0, 1, 2, 3) << 8)        // 1: corner 0 inside
                            | (perm_byte(1, 0, 3, 2) << 16)     // 2: corner 1
                            | (perm_byte(0, 1, 2, 3) << 24)     // 3: corners 0, 1
                            | (perm_byte(2, 0, 1, 3) << 32)     // 4: corner 2
                            | (perm_byte(0, 2, 3, 1) << 40)     // 5: corners 0, 2
                            | (perm_byte(1, 2, 0, 3) << 48)     // 6: corners 1, 2
                            | (perm_byte(3, 0, 2, 1) << 56);    // 7: corner 3 outside
    constexpr uint64_t hi = perm_byte(3, 0, 2, 1)               // 8: corner 3 inside
                            | (perm_byte(0, 3, 1, 2) << 8)      // 9: corners 0, 3
                            | (perm_byte(1, 3, 2, 0) << 16)     // 10: corners 1, 3
                            | (perm_byte(2, 0, 1, 3) << 24)     // 11: corner 2 outside
                            | (perm_byte(2, 3, 0, 1) << 32)     // 12: corners 2, 3
                            | (perm_byte(1, 0, 3, 2) << 40)     // 13: corner 1 outside
                            | (perm_byte(0, 1, 2, 3) << 48);    // 14: corner 0 outside
    const uint32_t m = mask & 15u;
    return (uint32_t)(((m < 8u ? lo : hi) >> (8u * (m & 7u))) & 0xFFu);
}

// det = d_1 . (d_2 x d_3) < 0 of the four sites p[c][0..3): the winding is flipped
RF_ISO_HD bool tet_flipped(const double (*p)[3]) {
    const double d1x = p[1][0] - p[0][0], d1y = p[1][1] - p[0][1], d1z = p[1][2] - p[0][2];
    const double d2x = p[2][0] - p[0][0], d2y = p[2][1] - p[0][1], d2z = p[2][2] - p[0][2];
    const double d3x = p[3][0] - p[0][0], d3y = p[3][1] - p[0][1], d3z = p[3][2] - p[0][2];
    const double ax = d2y * d3z - d2z * d3y, ay = d2z * d3x - d2x * d3z, az = d2x * d3y - d2y * d3x;
    const double det = (d1x * ax + d1y * ay) + d1z * az;
    return det < 0.0;
}

// the key of the edge between sites x and y (both in [0, 2^31)): the lower one in the high word
RF_ISO_HD int64_t edge_key(int64_t x, int64_t y) {
    const int64_t a = x < y ? x : y, b = x < y ? y : x;
    return a * 4294967296ll + b;
}

RF_ISO_HD void key_sites(int64_t key, int64_t &a, int64_t &b) {
    a = key >> 32, b = key & 0xFFFFFFFFll;
}

// keys[3 * f + c]: corner c of triangle f of the tetrahedron of sites s[0..4) with that mask, in the final winding.
// Returns the number of triangles, mask_triangles(mask).
RF_ISO_HD uint32_t tet_keys(uint32_t mask, bool flipped, const int64_t *s, int64_t *keys) {
    const uint32_t n = mask_triangles(mask);
    if (n == 0u) return 0u;
    const uint32_t perm = mask_perm(mask);
    const int64_t si = s[perm & 3u], sj = s[(perm >> 2) & 3u], sk = s[(perm >> 4) & 3u], sl = s[(perm >> 6) & 3u];
    const uint32_t m = mask & 15u;
    int64_t q0, q1, q2, q3 = kNoKey;
    if (n == 2u) {
        q0 = edge_key(si, sk), q1 = edge_key(si, sl), q2 = edge_key(sj, sl), q3 = edge_key(sj, sk);
    } else if (m == 1u || m == 2u || m == 4u || m == 8u) {
        q0 = edge_key(si, sj), q1 = edge_key(si, sk), q2 = edge_key(si, sl);
    } else {
        q0 = edge_key(si, sj), q1 = edge_key(si, sl), q2 = edge_key(si, sk);
    }
    keys[0] = q0, keys[1] = flipped ? q2 : q1, keys[2] = flipped ? q1 : q2;
    if (n == 2u) keys[3] = q0, keys[4] = flipped ? q3 : q2, keys[5] = flipped ? q2 : q3;
    return n;
}

// s[0..4): the sites of a row of 32- or 64-bit indices; false if one of them is outside [0, num_points)
template <typename I>
RF_ISO_HD bool tet_sites(const I *row, uint32_t num_points, int64_t *s) {
    const int64_t n = (int64_t)num_points;
    bool ok = true;
    for (uint32_t c = 0; c < 4u; ++c) {
        s[c] = (int64_t)row[c];
        ok = ok && s[c] >= 0 && s[c] < n;
    }
    return ok;
}

// the mask of a tetrahedron whose sites are in range
RF_ISO_HD uint32_t sites_mask(const float *values, const int64_t *s, double level) {
    return tet_mask((double)values[s[0]], (double)values[s[1]], (double)values[s[2]], (double)values[s[3]], level);
}

RF_ISO_HD bool sites_flipped(const float *points, const int64_t *s) {
    double p[4][3];
    for (uint32_t c = 0; c < 4u; ++c)
        for (uint32_t d = 0; d < 3u; ++d) p[c][d] = (double)points[3 * (size_t)s[c] + d];
    return tet_flipped(p);
}

// The `count` triangles of a tetrahedron (what the counting pass said of it) at keys[3 * count]: tet_keys, or kNoKey
// throughout if the sites are out of range or the mask now gives another count.
RF_ISO_HD void tet_emit(const float *points, const float *values, bool in_range, const int64_t *s, double level,
                        uint32_t count, int64_t *keys) {
    int64_t k[6];
    uint32_t n = 0u;
    if (in_range) {
        const uint32_t mask = sites_mask(values, s, level);
        if (mask_triangles(mask) == count) n = tet_keys(mask, sites_flipped(points, s), s, k);
    }
    for (uint32_t i = 0; i < 3u * count; ++i) keys[i] = n == count ? k[i] : kNoKey;
}

// the operands of the vertex on edge (a,b); false if a site is out of range
struct Edge {
    double pa[3], e[3], va, vb;
};

RF_ISO_HD bool load_edge(const float *points, const float *values, uint32_t num_points, int64_t a, int64_t b, Edge &k) {
    const int64_t n = (int64_t)num_points;
    if (a < 0 || a >= n || b < 0 || b >= n) return false;
    for (uint32_t c = 0; c < 3u; ++c) {
        k.pa[c] = (double)points[3 * (size_t)a + c];
        k.e[c] = (double)points[3 * (size_t)b + c] - k.pa[c];
    }
    k.va = (double)values[a], k.vb = (double)values[b];
    return true;
}

// x[3] and t of the edge; false (nothing written) where v_a == v_b or a result is not finite
RF_ISO_HD bool edge_point(const Edge &k, double level, double *x, double &t) {
    const double D = k.vb - k.va;
    if (D == 0.0) return false;
    const double tt = (level - k.va) / D;
    const double x0 = k.pa[0] + tt * k.e[0], x1 = k.pa[1] + tt * k.e[1], x2 = k.pa[2] + tt * k.e[2];
    if (!(finite(tt) && finite(x0) && finite(x1) && finite(x2))) return false;
    x[0] = x0, x[1] = x1, x[2] = x2, t = tt;
    return true;
}

// vertex[3] and t of the edge sites[0] -> sites[1]; NaN where there is none
RF_ISO_HD void edge_vertex(const float *points, const float *values, uint32_t num_points, const int64_t *sites, double level,
                           double *vertex, double *t) {
    Edge k;
    vertex[0] = vertex[1] = vertex[2] = *t = (double)NAN;
    if (!load_edge(points, values, num_points, sites[0], sites[1], k)) return;
    double x[3], tt;
    if (!edge_point(k, level, x, tt)) return;
    vertex[0] = x[0], vertex[1] = x[1], vertex[2] = x[2], *t = tt;
}

// parts[2][4]: what the upstream g[3] of the edge's vertex gives (p_a, v_a) and (p_b, v_b); zeros where the vertex is
// NaN or one of the eight is not finite
RF_ISO_HD void edge_vertex_grad(const float *points, const float *values, uint32_t num_points, const int64_t *sites,
                                double level, const double *g, double *parts) {
    Edge k;
    for (uint32_t i = 0; i < 8u; ++i) parts[i] = 0.0;
    if (!load_edge(points, values, num_points, sites[0], sites[1], k)) return;
    double x[3], t;
    if (!edge_point(k, level, x, t)) return;
    const double D = k.vb - k.va, s = 1.0 - t;
    const double dot = (g[0] * k.e[0] + g[1] * k.e[1]) + g[2] * k.e[2];
    const double ga = (dot * (level - k.vb)) / (D * D), gb = -((dot * (level - k.va)) / (D * D));
    const double ax = s * g[0], ay = s * g[1], az = s * g[2], bx = t * g[0], by = t * g[1], bz = t * g[2];
    if (!(finite(ax) && finite(ay) && finite(az) && finite(ga) && finite(bx) && finite(by) && finite(bz) && finite(gb)))
        return;
    parts[0] = ax, parts[1] = ay, parts[2] = az, parts[3] = ga;
    parts[4] = bx, parts[5] = by, parts[6] = bz, parts[7] = gb;
}

}  // namespace iso
}  // namespace rf
