// rf_clip_box_area_grad.hpp -- the backward of the face and wall areas of the Voronoi cells clipped to a box
// (rf_cell_box_area_grad.hip): the gradient of  L = sum_s g[s] face_area[s] + sum_{a,w} gw[a,w] wall_area[a,w]  with
// respect to the sites, in double ("Point gradients of the face and wall areas in a box").  The box is fixed.
//
// The polygons are the forward's: face i < degree of the plane list of rf_clip_box.hpp (the row in row order, then the
// six walls), the same R, the tie rule of clip_by_list_plane, the list order.  The clipping carries the labels of
// rf_clip_area_grad.hpp: one per vertex, the LIST index of the plane its outgoing edge lies on (a row index < degree: that
// neighbour's bisector; degree + w: wall w; none: the starting square).  clip_by_list_plane_labelled emits the vertices
// of clip_by_list_plane bit for bit.  The walls are in the list, so nothing of the square survives them and every edge of
// a finished polygon is a bounded segment: an edge still labelled none is skipped before any arithmetic, and the 8 R
// square of rf_clip_area_grad.hpp (which kept the three rows of a triangle from cutting an unbounded edge differently) is
// not needed -- here the three rows cut a Voronoi edge by the same six walls.
//
// Weights: g^[s] = g[s] where face_area[s] > 0 and 0 where it is exactly 0, gw^[a,w] likewise by wall_area[a,w] > 0, and
// G_ab = g^[a->b] + g^[b->a] (effective_weight of rf_clip_area_grad.hpp; a missing mate weighs 0).
//
// A flat face changes its area only through the in-plane motion of its edges, and every edge lies on a's own polytope:
//   * a Voronoi edge of F_ab labelled by a row site c is dual to the triangle (a,b,c) and carries the closed form of
//     rf_clip_area_grad.hpp,  l (lambda_b + lambda_c) y  with G_ab, G_ac, G_bc (edge_lambda), l and y the length and the
//     midpoint of the segment as the box clipped it: the displacement of a point of the edge is affine along it, so the
//     midpoint carries the integral, and the motion of an end point along the edge is of second order.  Counted once
//     (counts_here, by the forward's boxed areas), and shared among cocircular sites as there.
//   * a wall edge of F_ab labelled wall w is the trace of the bisector in the wall and bounds F_ab, W_aw and W_bw.  A
//     point of it moves by w with  n_w . w = 0  and  d_b . w = y . delta_a - (y - d_b) . delta_b =: beta.  With cos t =
//     n_w . d_b / |d_b| and sin t > 0 the in-plane outward conormals are  (n_w - cos t d^) / sin t  for F_ab and
//     +-(d^ - cos t n_w) / sin t  for W_aw / W_bw, so  w . nu  is  -cot t beta / |d_b|  and  +-beta / (|d_b| sin t):
//         grad p_a += (l y / |d_b|) [ -G_ab cot t + (gw^[a,w] - gw^[b,w]) / sin t ].
//     gw^[b,w] is read directly.  The edge is in exactly one lane, that of F_ab, and counts where the forward area of
//     that slot is > 0: a face the forward left with area exactly 0 is a point or a segment (cocircular sites, a
//     bisector in a wall), its trace in the wall has length 0 on either side of the kink, and what the degenerate polygon
//     shows as an edge is not one.  sin t == 0 cannot bound a polygon and is skipped.
//     A wall-labelled edge both of whose end points lie on a further row plane (kOnLine) is a Voronoi edge lying in the
//     wall.  The row's planes come first in the list, so exact arithmetic labels such an edge with the row plane; the
//     wall's label shows only where rounding let the wall cut a hair off (the unjittered grid in a box whose walls are
//     bisectors).  The areas have a kink there; the wall-labelled copy is skipped, so that the result does not depend on
//     which label the rounding chose, and the row-labelled copy keeps the Voronoi-edge treatment.
//   * an edge between two walls does not move; it never appears in a row face's polygon.  Zero length: nothing.
// An empty row and an empty cell (nonempty false) get a zero row.
//
// __host__ __device__ and free of HIP types: tests/host_harness/clip_box_area_grad_host.cpp compiles this file with g++
// (no FMA contraction on either side).
#pragma once

#include "rf_clip_area_grad.hpp"
#include "rf_clip_box.hpp"

namespace rf {
namespace clip {

// clip_by_list_plane with labels: the same tie rule, the same vertices
template <typename L>
RF_CLIP_HD bool clip_by_list_plane_labelled(const Frame &frame, double nx, double ny, double nz, bool earlier, double dx,
                                            double dy, double dz, double h, double *s, double *t, L *lab, uint32_t stride,
                                            uint32_t cap, uint32_t &m, uint32_t &cur, L label) {
    double A, B, C;
    plane_in_frame(frame, dx, dy, dz, h, A, B, C);
    if (A == 0.0 && B == 0.0 && C == 0.0 && nx * dx + ny * dy + nz * dz > 0.0) {
        if (earlier) m = 0;
        return true;
    }
    const uint32_t in = cur * cap * stride, out = (cur ^ 1u) * cap * stride;
    if (!clip_step_labelled(s + in, t + in, lab + in, s + out, t + out, lab + out, stride, cap, m, A, B, C, label))
        return false;
    cur ^= 1u;
    return true;
}

// face_polygon_box for a row face i < degree, with labels; lab has 2 * cap * stride entries like s and t
template <typename L>
RF_CLIP_HD bool face_polygon_box_labelled(const float *points, const uint32_t *adj, uint32_t a, uint32_t begin,
                                          uint32_t end, const Box &box, uint32_t i, double R, double *s, double *t, L *lab,
                                          uint32_t stride, uint32_t cap, Frame &frame, uint32_t &m, uint32_t &cur) {
    const uint32_t degree = end - begin, count = degree + kWalls;
    double nx, ny, nz, h;
    list_plane(points, adj, a, begin, degree, box, i, nx, ny, nz, h);
    frame = list_frame(false, nx, ny, nz, h);
    init_square(s, t, stride, R);
    init_square_labels(lab, stride);
    m = 4, cur = 0;
    for (uint32_t j = 0; j < count && m != 0; ++j) {
        if (j == i) continue;
        double dx, dy, dz, hj;
        list_plane(points, adj, a, begin, degree, box, j, dx, dy, dz, hj);
        if (!clip_by_list_plane_labelled(frame, nx, ny, nz, j < i, dx, dy, dz, hj, s, t, lab, stride, cap, m, cur, (L)j))
            return false;
    }
    return true;
}

// effective_weight for an upstream that may be null (zero)
RF_CLIP_HD double effective_weight_box(const uint32_t *adj, const uint32_t *offsets, uint32_t num_points,
                                       uint32_t num_edges, const double *face_area, const double *g, uint32_t a,
                                       uint32_t k) {
    return g == nullptr ? 0.0 : effective_weight(adj, offsets, num_points, num_edges, face_area, g, a, k);
}

// gw^ of (cell, wall): the upstream where that wall's own forward area is positive (false for NaN too); gw may be null
RF_CLIP_HD double wall_weight(const double *wall_area, const double *gw, uint32_t cell, uint32_t w) {
    const size_t at = kWalls * (size_t)cell + w;
    if (gw == nullptr || !(wall_area[at] > 0.0)) return 0.0;
    return gw[at];
}

// The bracket of a wall edge over |d_b|:  [ -G_ab cot t + (gwa - gwb) / sin t ] / |d_b|  for wall w and d_b = (bx,by,bz)
// of length lb; 0 where sin t == 0.  A choice among computed values, not among addresses.
RF_CLIP_HD double wall_edge_term(uint32_t w, double lb, double bx, double by, double bz, double gab, double gwa,
                                 double gwb) {
    const uint32_t k = w >> 1;
    const double along = k == 0u ? bx : k == 1u ? by : bz;
    const double xx = bx * bx, yy = by * by, zz = bz * bz;
    const double across2 = k == 0u ? yy + zz : k == 1u ? xx + zz : xx + yy;
    if (!(across2 > 0.0)) return 0.0;
    const double cs = ((w & 1u) != 0u ? along : -along) / lb, sn = sqrt(across2) / lb;
    return ((gwa - gwb) / sn - gab * (cs / sn)) / lb;
}

// add_polygon_terms of rf_clip_area_grad.hpp for a face of the boxed cell: the labels are list indices, an edge labelled
// degree + w is a wall edge, and no edge is unbounded.  gwa[6]: the cell's own masked wall weights; wall_area / gw: the
// arrays gw^[b,w] is read from.  Everything else as there (wsum, wn: free buffers of the polygon's stride).
template <typename Row, typename L>
RF_CLIP_HD void add_polygon_terms_box(const Row &row, uint32_t degree, uint32_t k, const Frame &f, double bx, double by,
                                      double bz, const double *ps, const double *pt, const L *pl, double *wsum, double *wn,
                                      uint32_t stride, uint32_t m, const uint32_t *adj, const uint32_t *offsets,
                                      uint32_t num_edges, const double *G, uint32_t b, const double *row_G,
                                      const double *row_area, const double *gwa, const double *wall_area, const double *gw,
                                      double &gx, double &gy, double &gz) {
    const double gab = row_G[k], area_b = row_area[k];
    double cx, cy, cz, h;
    for (uint32_t i = 0; i < m; ++i) {
        const uint32_t j = i + 1 < m ? i + 1 : 0u;
        const L l = pl[i * stride];
        const double s1 = ps[i * stride], t1 = pt[i * stride], s2 = ps[j * stride], t2 = pt[j * stride];
        double sum = 0.0, n = -1.0;
        if (l != no_label<L>() && (s1 != s2 || t1 != t2)) {   // not left of the square, not of zero length
            if ((uint32_t)l >= degree) {
                if (area_b > 0.0) {   // a wall edge is its face's alone: none where the forward clipped the face away
                    const uint32_t w = (uint32_t)l - degree;
                    sum = wall_edge_term(w, f.len, bx, by, bz, gab, gwa[w], wall_weight(wall_area, gw, b, w));
                    n = 0.0;
                }
            } else {
                double gbc = 0.0;
                n = listed_weight(adj, offsets, num_edges, G, b, row.site(l), gbc) ? 1.0 : 0.0;
                if (counts_here(area_b, row_area[l], k, l)) {
                    row.plane(l, cx, cy, cz, h);
                    sum = edge_lambda(f.len, bx, by, bz, cx, cy, cz, gab, row_G[l], gbc);   // with G_bc = 0 where n is 0
                }
            }
        }
        wsum[i * stride] = sum, wn[i * stride] = n;
    }
    for (uint32_t j = 0; j < degree; ++j) {   // further row sites cocircular around a Voronoi edge
        if (j == k) continue;
        double A, B, C;
        row.plane(j, cx, cy, cz, h);
        plane_in_frame(f, cx, cy, cz, h, A, B, C);
        int listed = -1;
        double gbc = 0.0;
        const bool on_0 = on_line(A, B, C, ps[0], pt[0]);
        bool on_c = on_0;
        for (uint32_t i = 0; i < m; ++i) {
            const bool on_n = i + 1 < m ? on_line(A, B, C, ps[(i + 1) * stride], pt[(i + 1) * stride]) : on_0;
            const bool both = on_c && on_n;
            on_c = on_n;
            if (!both) continue;
            const L l = pl[i * stride];
            const double n = wn[i * stride];
            if (n < 0.0 || l == (L)j) continue;
            if ((uint32_t)l >= degree) {   // a Voronoi edge lying in the wall: the wall-labelled copy carries nothing
                wn[i * stride] = -1.0;
                continue;
            }
            double lx, ly, lz, lh, A0, B0, C0;
            row.plane(l, lx, ly, lz, lh);
            plane_in_frame(f, lx, ly, lz, lh, A0, B0, C0);
            if (!(A * A0 + B * B0 > 0.0)) continue;   // from the other side: the second edge of a sliver
            if (listed < 0) listed = listed_weight(adj, offsets, num_edges, G, b, row.site(j), gbc) ? 1 : 0;
            if (listed == 0) continue;
            double sum = n > 0.0 ? wsum[i * stride] : 0.0;   // the first triangle that b lists replaces the stand-in
            if (counts_here(area_b, row_area[j], k, j))
                sum += edge_lambda(f.len, bx, by, bz, cx, cy, cz, gab, row_G[j], gbc);
            wsum[i * stride] = sum, wn[i * stride] = n + 1.0;
        }
    }
    for (uint32_t i = 0; i < m; ++i) {
        const double n = wn[i * stride];
        if (n < 0.0) continue;
        const uint32_t j = i + 1 < m ? i + 1 : 0u;
        const double s1 = ps[i * stride], t1 = pt[i * stride], s2 = ps[j * stride], t2 = pt[j * stride];
        const double ds = s2 - s1, dt = t2 - t1;
        const double len = sqrt(ds * ds + dt * dt);
        double x, y, z;
        to_space(f, 0.5 * (s1 + s2), 0.5 * (t1 + t2), x, y, z);
        const double w = len * wsum[i * stride] / fmax(n, 1.0);
        gx += w * x, gy += w * y, gz += w * z;
    }
}

// One whole row of the gradient, row face after row face (the host harness, and the kernel of last resort).  G[E] holds
// effective_weight of every slot (zeros for a null upstream); grad_wall_area may be null.  s, t and lab hold 2 * cap each.
// Writes grad_points[3 a ..] (NaN on a status other than kCellOk) and returns a kCell* status.
RF_CLIP_HD uint32_t cell_box_area_grad_serial(const float *points, uint32_t num_points, const uint32_t *adj,
                                              const uint32_t *offsets, uint32_t num_edges, uint32_t a, const Box &box,
                                              double R, double *s, double *t, uint32_t *lab, uint32_t cap,
                                              const uint8_t *nonempty, const double *face_area, const double *wall_area,
                                              const double *G, const double *grad_wall_area, double *grad_points) {
    const uint32_t begin = offsets[a], end = offsets[a + 1];
    uint32_t status = row_is_valid(points, num_points, adj, num_edges, a, begin, end) ? kCellOk : kCellBadRow;
    double gx = 0.0, gy = 0.0, gz = 0.0;
    if (status == kCellOk && begin < end && nonempty[a]) {
        double gwa[kWalls];
        for (uint32_t w = 0; w < kWalls; ++w) gwa[w] = wall_weight(wall_area, grad_wall_area, a, w);
        const RowFromArrays row = {points, adj + begin, a};
        for (uint32_t i = 0; i < end - begin; ++i) {
            Frame frame;
            uint32_t m, cur;
            if (!face_polygon_box_labelled(points, adj, a, begin, end, box, i, R, s, t, lab, 1u, cap, frame, m, cur)) {
                status = kCellTooManyVertices;
                break;
            }
            if (m == 0) continue;
            double bx, by, bz, h;
            neighbour(points, a, adj[begin + i], bx, by, bz, h);
            add_polygon_terms_box(row, end - begin, i, frame, bx, by, bz, s + cur * cap, t + cur * cap, lab + cur * cap,
                                  s + (cur ^ 1u) * cap, t + (cur ^ 1u) * cap, 1u, m, adj, offsets, num_edges, G,
                                  adj[begin + i], G + begin, face_area + begin, gwa, wall_area, grad_wall_area, gx, gy, gz);
        }
    }
    if (status != kCellOk) gx = gy = gz = (double)NAN;
    grad_points[3 * (size_t)a] = gx, grad_points[3 * (size_t)a + 1] = gy, grad_points[3 * (size_t)a + 2] = gz;
    return status;
}

}  // namespace clip
}  // namespace rf
