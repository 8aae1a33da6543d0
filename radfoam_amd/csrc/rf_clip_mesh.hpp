// rf_clip_mesh.hpp -- the corners of the Voronoi faces as named Voronoi vertices (rf_cell_mesh.hip), over the labelled
// clipping of rf_clip_area_grad.hpp, in double.
//
// The labelled clipping knows for every edge of a face's polygon which neighbour's plane it lies on.  Corner i of the
// polygon of face (a,b) is where the edge labelled label[i-1] (the one that arrives) meets the edge labelled label[i] (the
// one that leaves): the point equidistant from a, b and those two sites, the Voronoi vertex dual to the Delaunay
// tetrahedron of the four.  The four site indices in ascending order are the corner's key: every face around the vertex
// derives the same key from its own row, so equal keys weld the faces without a tolerance on positions.  A label of the
// square (none) gives the site kNoSite; it cannot occur on a bounded face.  A key with a repeated site (degenerate
// input) is kept as it is.
//
// The clipping here starts from the forward's square (rf::clip::half_side), not the backward's of
// rf_clip_area_grad.hpp, and the corner's position is p_a + to_space(...): the arithmetic of surface_emit_kernel, so a
// corner is bit for bit the triangle corner cell_surface writes.
//
// The vertex of a key is also a closed form of four rows of `points`, the circumcentre of the tetrahedron: with
// d_i = p_i - p_0 (i = 1..3; exact in double for fp32 inputs), M the matrix of rows d_i and r_i = |d_i|^2 / 2,
//     x = M^-1 r,  c = p_0 + x;      for an upstream g:  y = M^-T g,  grad p_i = y_i (d_i - x),  grad p_0 = g - sum_i grad p_i
// (M x = r differentiates to M dx = [ddelta_i . (d_i - x)]).  Both by Cramer's rule on the cross products of the d_i.
// det M == 0 exactly, a site out of range or a result that is not finite: NaN forward, nothing backward.  There is no
// other guard; a nearly flat tetrahedron gives large finite values.
//
// __host__ __device__, no HIP types: tests/host_harness/clip_mesh_host.cpp compiles this file with g++ (no FMA
// contraction on either side).
#pragma once

#include "rf_clip_area_grad.hpp"

namespace rf {
namespace clip {

constexpr uint32_t kNoSite = 0xFFFFFFFFu;
constexpr uint32_t kCellVertexCount = 3;   // the labelled polygon has another vertex count than cell_geometry's

// the cell whose row holds adjacency slot e: the last a with offsets[a] <= e (kNoSite if the offsets do not say)
RF_CLIP_HD uint32_t slot_owner(const uint32_t *offsets, uint32_t num_points, uint32_t num_edges, uint32_t e) {
    uint32_t lo = 0, hi = num_points + 1u;   // first index whose offset is > e
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (offsets[mid] > e) hi = mid;
        else lo = mid + 1u;
    }
    if (lo == 0 || lo > num_points) return kNoSite;
    const uint32_t a = lo - 1u;
    return (offsets[a] <= e && e < offsets[a + 1] && offsets[a + 1] <= num_edges) ? a : kNoSite;
}

RF_CLIP_HD void order2(uint32_t &lo, uint32_t &hi) {
    const uint32_t l = lo < hi ? lo : hi, h = lo < hi ? hi : lo;
    lo = l, hi = h;
}

RF_CLIP_HD void sort4(uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d) {
    order2(a, b), order2(c, d), order2(a, c), order2(b, d), order2(b, c);
}

// the site a label of row `row_adj` (adj + begin) names
template <typename L>
RF_CLIP_HD uint32_t label_site(const uint32_t *row_adj, L l) {
    return l == no_label<L>() ? kNoSite : row_adj[(uint32_t)l];
}

// The corners of the finished polygon (ps, pt, pl)[0..m) of face (a,b) in frame f: xyz[3 * i ..] = p_a + the vertex,
// sites[4 * i ..] its key.  row_adj: the row of a, every entry of which is < num_points (row_is_valid).
template <typename L>
RF_CLIP_HD void write_corners(const float *points, const uint32_t *row_adj, uint32_t a, uint32_t b, const Frame &f,
                              const double *ps, const double *pt, const L *pl, uint32_t stride, uint32_t m, double *xyz,
                              uint32_t *sites) {
    const double px = points[3 * (size_t)a], py = points[3 * (size_t)a + 1], pz = points[3 * (size_t)a + 2];
    uint32_t arrives = m ? label_site(row_adj, pl[(m - 1u) * stride]) : kNoSite;
    for (uint32_t i = 0; i < m; ++i) {
        double x, y, z;
        to_space(f, ps[i * stride], pt[i * stride], x, y, z);
        x += px, y += py, z += pz;
        xyz[3 * (size_t)i] = x, xyz[3 * (size_t)i + 1] = y, xyz[3 * (size_t)i + 2] = z;
        const uint32_t leaves = label_site(row_adj, pl[i * stride]);
        uint32_t k0 = a, k1 = b, k2 = arrives, k3 = leaves;
        sort4(k0, k1, k2, k3);
        sites[4 * (size_t)i] = k0, sites[4 * (size_t)i + 1] = k1, sites[4 * (size_t)i + 2] = k2, sites[4 * (size_t)i + 3] = k3;
        arrives = leaves;
    }
}

// corners that cannot be written: NaN and kNoSite, never stale
RF_CLIP_HD void void_corners(uint32_t count, double *xyz, uint32_t *sites) {
    for (uint32_t i = 0; i < count; ++i) {
        xyz[3 * (size_t)i] = xyz[3 * (size_t)i + 1] = xyz[3 * (size_t)i + 2] = (double)NAN;
        sites[4 * (size_t)i] = sites[4 * (size_t)i + 1] = sites[4 * (size_t)i + 2] = sites[4 * (size_t)i + 3] = kNoSite;
    }
}

// One face, serially: the counterpart of cell_serial (the host harness, and the kernel of last resort).  a owns slot.
// s, t and lab have 2 * cap entries.  Writes exactly `expect` corners, cell_geometry's face_vertices of the slot (the
// labelled step emits clip_step's vertices, so the counts agree); on a status other than kCellOk they are void.
RF_CLIP_HD uint32_t face_corners_serial(const float *points, uint32_t num_points, const uint32_t *adj,
                                        const uint32_t *offsets, uint32_t num_edges, uint32_t a, uint32_t slot, double R,
                                        double *s, double *t, uint32_t *lab, uint32_t cap, uint32_t expect, double *xyz,
                                        uint32_t *sites) {
    uint32_t status = kCellBadRow, m = 0, cur = 0;
    Frame frame;
    if (a < num_points) {
        const uint32_t begin = offsets[a], end = offsets[a + 1];
        if (row_is_valid(points, num_points, adj, num_edges, a, begin, end) && begin <= slot && slot < end) {
            status = kCellOk;
            if (!face_polygon_labelled(points, adj, a, begin, end, slot, R, s, t, lab, 1u, cap, frame, m, cur))
                status = kCellTooManyVertices;
            else if (m != expect)
                status = kCellVertexCount;
            if (status == kCellOk)
                write_corners(points, adj + begin, a, adj[slot], frame, s + cur * cap, t + cur * cap, lab + cur * cap, 1u,
                              m, xyz, sites);
        }
    }
    if (status != kCellOk) void_corners(expect, xyz, sites);
    return status;
}

// d_i = p_i - p_0 of the four sites of a key; false if one of them is out of range
RF_CLIP_HD bool key_edges(const float *points, uint32_t num_points, const int64_t *key, double *p0, double *d1, double *d2,
                          double *d3) {
    const int64_t i0 = key[0], i1 = key[1], i2 = key[2], i3 = key[3];
    const int64_t n = (int64_t)num_points;
    if (i0 < 0 || i0 >= n || i1 < 0 || i1 >= n || i2 < 0 || i2 >= n || i3 < 0 || i3 >= n) return false;
    for (uint32_t c = 0; c < 3u; ++c) {
        p0[c] = (double)points[3 * (size_t)i0 + c];
        d1[c] = (double)points[3 * (size_t)i1 + c] - p0[c];
        d2[c] = (double)points[3 * (size_t)i2 + c] - p0[c];
        d3[c] = (double)points[3 * (size_t)i3 + c] - p0[c];
    }
    return true;
}

// the three cross products of Cramer's rule and det M = d_1 . (d_2 x d_3)
struct TetCross {
    double ax, ay, az, bx, by, bz, cx, cy, cz, det;   // a = d_2 x d_3, b = d_3 x d_1, c = d_1 x d_2
};

RF_CLIP_HD TetCross tet_cross(double d1x, double d1y, double d1z, double d2x, double d2y, double d2z, double d3x,
                              double d3y, double d3z) {
    TetCross k;
    k.ax = d2y * d3z - d2z * d3y, k.ay = d2z * d3x - d2x * d3z, k.az = d2x * d3y - d2y * d3x;
    k.bx = d3y * d1z - d3z * d1y, k.by = d3z * d1x - d3x * d1z, k.bz = d3x * d1y - d3y * d1x;
    k.cx = d1y * d2z - d1z * d2y, k.cy = d1z * d2x - d1x * d2z, k.cz = d1x * d2y - d1y * d2x;
    k.det = (d1x * k.ax + d1y * k.ay) + d1z * k.az;
    return k;
}

// x = M^-1 r relative to p_0; false where det == 0 or x is not finite
RF_CLIP_HD bool tet_centre(const TetCross &k, double d1x, double d1y, double d1z, double d2x, double d2y, double d2z,
                           double d3x, double d3y, double d3z, double &x, double &y, double &z) {
    if (k.det == 0.0 || k.det != k.det) return false;
    const double r1 = 0.5 * ((d1x * d1x + d1y * d1y) + d1z * d1z), r2 = 0.5 * ((d2x * d2x + d2y * d2y) + d2z * d2z),
                 r3 = 0.5 * ((d3x * d3x + d3y * d3y) + d3z * d3z);
    x = ((r1 * k.ax + r2 * k.bx) + r3 * k.cx) / k.det;
    y = ((r1 * k.ay + r2 * k.by) + r3 * k.cy) / k.det;
    z = ((r1 * k.az + r2 * k.bz) + r3 * k.cz) / k.det;
    const double big = (double)INFINITY;
    return fabs(x) < big && fabs(y) < big && fabs(z) < big;
}

// vertex[3]: the circumcentre of the key's four sites, NaN where there is none
RF_CLIP_HD void key_vertex(const float *points, uint32_t num_points, const int64_t *key, double *vertex) {
    double p0[3], d1[3], d2[3], d3[3], x, y, z;
    vertex[0] = vertex[1] = vertex[2] = (double)NAN;
    if (!key_edges(points, num_points, key, p0, d1, d2, d3)) return;
    const TetCross k = tet_cross(d1[0], d1[1], d1[2], d2[0], d2[1], d2[2], d3[0], d3[1], d3[2]);
    if (!tet_centre(k, d1[0], d1[1], d1[2], d2[0], d2[1], d2[2], d3[0], d3[1], d3[2], x, y, z)) return;
    vertex[0] = p0[0] + x, vertex[1] = p0[1] + y, vertex[2] = p0[2] + z;
}

// grad[4][3]: what the upstream g[3] of the key's vertex gives its four sites, in the key's order; zeros where the
// vertex is NaN or a term is not finite
RF_CLIP_HD void key_vertex_grad(const float *points, uint32_t num_points, const int64_t *key, const double *g,
                                double *grad) {
    double p0[3], d1[3], d2[3], d3[3], x, y, z;
    for (uint32_t i = 0; i < 12u; ++i) grad[i] = 0.0;
    if (!key_edges(points, num_points, key, p0, d1, d2, d3)) return;
    const TetCross k = tet_cross(d1[0], d1[1], d1[2], d2[0], d2[1], d2[2], d3[0], d3[1], d3[2]);
    if (!tet_centre(k, d1[0], d1[1], d1[2], d2[0], d2[1], d2[2], d3[0], d3[1], d3[2], x, y, z)) return;
    const double gx = g[0], gy = g[1], gz = g[2];
    const double y1 = ((gx * k.ax + gy * k.ay) + gz * k.az) / k.det, y2 = ((gx * k.bx + gy * k.by) + gz * k.bz) / k.det,
                 y3 = ((gx * k.cx + gy * k.cy) + gz * k.cz) / k.det;
    const double g1x = y1 * (d1[0] - x), g1y = y1 * (d1[1] - y), g1z = y1 * (d1[2] - z);
    const double g2x = y2 * (d2[0] - x), g2y = y2 * (d2[1] - y), g2z = y2 * (d2[2] - z);
    const double g3x = y3 * (d3[0] - x), g3y = y3 * (d3[1] - y), g3z = y3 * (d3[2] - z);
    const double g0x = gx - ((g1x + g2x) + g3x), g0y = gy - ((g1y + g2y) + g3y), g0z = gz - ((g1z + g2z) + g3z);
    // finite, all twelve: a sum of magnitudes carries a NaN or an inf of any of them (an upstream's included)
    const double all = ((fabs(g0x) + fabs(g0y)) + (fabs(g0z) + fabs(g1x))) + ((fabs(g1y) + fabs(g1z)) + (fabs(g2x) + fabs(g2y))) +
                       ((fabs(g2z) + fabs(g3x)) + (fabs(g3y) + fabs(g3z)));
    if (!(all < (double)INFINITY)) return;
    grad[0] = g0x, grad[1] = g0y, grad[2] = g0z;
    grad[3] = g1x, grad[4] = g1y, grad[5] = g1z;
    grad[6] = g2x, grad[7] = g2y, grad[8] = g2z;
    grad[9] = g3x, grad[10] = g3y, grad[11] = g3z;
}

}  // namespace clip
}  // namespace rf
