// rf_clip_area_grad.hpp -- the backward of the Voronoi face areas (rf_face_area_grad.hip) over the clipping core of
// rf_clip.hpp, in double: the gradient of  L = sum_slots g[s] face_area[s]  (finite areas only) with respect to the sites.
//
// Face {a,b} has two slots; its effective weight is G_ab = g^[a->b] + g^[b->a], g^ = g where that slot's own area is
// finite and 0 elsewhere (effective_weight below; what arrives for a slot of infinite area is never read).  A slot whose
// area is exactly zero has g^ = 0 as well: the forward clipped its polygon away (a face of two hull cells that lies
// wholly outside the forward's square, or a sliver of cospherical sites), its area is the constant 0 around there and
// the derivative of that is 0.
//
// A flat face changes its area only through the in-plane motion of its edges.  A finite Voronoi edge e (length l,
// midpoint y) is dual to a Delaunay triangle (a,b,c) and bounds exactly F_ab, F_ac and F_bc.  With d_b = p_b - p_a,
// d_c = p_c - p_a, e_bc = d_c - d_b the in-plane outward conormals of the three faces at e are the unit vectors of
//     nu_ab ~ d_c - (d_c . d_b / |d_b|^2) d_b,   nu_ac ~ d_b - (d_b . d_c / |d_c|^2) d_c,   nu_bc ~ -d_b + (d_b . e_bc / |e_bc|^2) e_bc,
// each of norm sqrt(det / |.|^2), det = |d_b x d_c|^2.  When the sites move by delta a point of the edge line stays
// equidistant from the three sites: its displacement w has  d_b . w = y . delta_a - (y - d_b) . delta_b  and the same
// with c (y relative to p_a).  Writing q = G_ab nu_ab + G_ac nu_ac + G_bc nu_bc = lambda_b d_b + lambda_c d_c, the
// triangle gives  dL = l w . q = l (lambda_b d_b . w + lambda_c d_c . w),  and the coefficient of delta_a is
//     l (lambda_b + lambda_c) y,   lambda_b + lambda_c = [ -G_ab (d_b . e_bc) / |d_b| + G_ac (d_c . e_bc) / |d_c| - G_bc |e_bc| ] / sqrt(det)
// (the 2x2 Gram system solved in closed form).  Row a forms that term alone: e is the edge of a's own polygon of F_ab
// that the plane of c cut, G_ab and G_ac are weights of a's own slots, and only G_bc is looked up, in row b.  The
// triangle turns up twice in row a (in F_ab as the edge labelled c, in F_ac as the edge labelled b) and counts once, in
// the lane of the face whose forward area is larger (counts_here): a sliver's degenerate polygon is never relied on.
// Where four sites are cocircular around an edge (the unjittered grid) the areas have a kink and the planes of two
// neighbours pass through the same edge line; add_polygon_terms then shares the edge among the triangles that the
// adjacency admits, the same in every row, so that the rows still add up to a gradient of one invariant function.
//
// To know which plane an edge lies on, the clipping carries one label per vertex: the row index of the plane its outgoing
// edge (to the next vertex) lies on, none for the square.  clip_step_labelled emits the vertices of clip_step bit for bit.
// An edge of the square, or one with an endpoint on it, is an unbounded Voronoi edge: all three of its faces are
// unbounded, their weights zero; it is skipped before any arithmetic.  A finite edge of an unbounded face counts.
// For that to hold in every row the backward clips from a square of half-side 8 R (area_grad_half_side), R the forward's:
// the three rows of a triangle see its edge from three frames whose centres lie up to a bounding-box diagonal (R / 4)
// apart and are turned against each other, so a point at max-norm distance 8 R in one frame is at least (8 R - R / 4) /
// sqrt(2) > R away in the others, and every face through it has area +inf in the forward, or 0 where it lies wholly
// outside its square: weight zero either way.  With the forward's own R an
// edge of a finite face of a far-reaching hull cell would be cut in one row and whole in another.
//
// The sum over a's own row is the exact gradient for a symmetric adjacency; a mate slot or a slot b->c that does not
// exist has weight 0.  __host__ __device__, no HIP types: tests/host_harness/clip_area_grad_host.cpp compiles this file
// with g++ (no FMA contraction on either side).
#pragma once

#include "rf_clip.hpp"

namespace rf {
namespace clip {

RF_CLIP_HD double area_grad_half_side(const float *bbox) {
    return 8.0 * half_side(bbox);
}

template <typename L>
RF_CLIP_HD L no_label() {
    return (L) ~(L)0;
}

RF_CLIP_HD bool area_has_weight(double area) {   // false for NaN too
    return area > 0.0 && area < (double)INFINITY;
}

// the weight of slot k of row a: g^[k] plus g^ of the mate slot (a in the row of b = adj[k]; the first if repeated)
RF_CLIP_HD double effective_weight(const uint32_t *adj, const uint32_t *offsets, uint32_t num_points, uint32_t num_edges,
                                   const double *face_area, const double *g, uint32_t a, uint32_t k) {
    double w = 0.0;
    if (area_has_weight(face_area[k])) w = g[k];
    const uint32_t b = adj[k];
    if (b >= num_points) return w;
    uint32_t rb = offsets[b], re = offsets[b + 1];
    if (re > num_edges) re = num_edges;
    for (; rb < re; ++rb)
        if (adj[rb] == a) {
            if (area_has_weight(face_area[rb])) w += g[rb];
            break;
        }
    return w;
}

template <typename L>
RF_CLIP_HD void init_square_labels(L *lab, uint32_t stride) {
    lab[0] = lab[stride] = lab[2 * stride] = lab[3 * stride] = no_label<L>();
}

// clip_step with labels: the same vertices by the same arithmetic.  A kept vertex keeps its label unless its edge leaves
// through the line without a crossing of its own (the vertex is exactly on the line): then, like a crossing on the way
// out, it starts the edge along the line and takes `label`.  A crossing on the way in continues the edge it cut.
template <typename L>
RF_CLIP_HD bool clip_step_labelled(const double *si, const double *ti, const L *li, double *so, double *to, L *lo,
                                   uint32_t stride, uint32_t cap, uint32_t &m, double A, double B, double C, L label) {
    uint32_t k = 0;
    if (m == 0) return true;
    const double s0 = si[0], t0 = ti[0], e0 = (A * s0 + B * t0) - C;
    double sc = s0, tc = t0, ec = e0;
    for (uint32_t i = 0; i < m; ++i) {
        double sn = s0, tn = t0, en = e0;
        if (i + 1 < m) {
            sn = si[(i + 1) * stride], tn = ti[(i + 1) * stride];
            en = (A * sn + B * tn) - C;
        }
        const L lc = li[i * stride];
        const bool in_c = ec <= 0.0, in_n = en <= 0.0;
        if (in_c) {
            if (k == cap) return false;
            so[k * stride] = sc, to[k * stride] = tc;
            lo[k * stride] = (!in_n && ec == 0.0) ? label : lc;
            ++k;
        }
        if (in_c != in_n && ec != 0.0 && en != 0.0) {
            if (k == cap) return false;
            const double w = ec / (ec - en);
            so[k * stride] = sc + w * (sn - sc), to[k * stride] = tc + w * (tn - tc);
            lo[k * stride] = in_c ? label : lc;
            ++k;
        }
        sc = sn, tc = tn, ec = en;
    }
    m = k;
    return true;
}

// face_polygon with labels (the row index f - begin of the plane); lab has 2 * cap * stride entries like s and t
template <typename L>
RF_CLIP_HD bool face_polygon_labelled(const float *points, const uint32_t *adj, uint32_t a, uint32_t begin, uint32_t end,
                                      uint32_t slot, double R, double *s, double *t, L *lab, uint32_t stride,
                                      uint32_t cap, Frame &frame, uint32_t &m, uint32_t &cur) {
    double dx, dy, dz, h;
    neighbour(points, a, adj[slot], dx, dy, dz, h);
    frame = make_frame(dx, dy, dz);
    init_square(s, t, stride, R);
    init_square_labels(lab, stride);
    m = 4, cur = 0;
    for (uint32_t f = begin; f < end && m != 0; ++f) {
        if (f == slot) continue;
        double A, B, C;
        neighbour(points, a, adj[f], dx, dy, dz, h);
        plane_in_frame(frame, dx, dy, dz, h, A, B, C);
        const uint32_t in = cur * cap * stride, out = (cur ^ 1u) * cap * stride;
        if (!clip_step_labelled(s + in, t + in, lab + in, s + out, t + out, lab + out, stride, cap, m, A, B, C,
                                (L)(f - begin)))
            return false;
        cur ^= 1u;
    }
    return true;
}

// does row b list site x?  g: the weight of that slot (the first if repeated)
RF_CLIP_HD bool listed_weight(const uint32_t *adj, const uint32_t *offsets, uint32_t num_edges, const double *G, uint32_t b,
                              uint32_t x, double &g) {
    uint32_t rb = offsets[b], re = offsets[b + 1];
    if (re > num_edges) re = num_edges;
    for (; rb < re; ++rb)
        if (adj[rb] == x) {
            g = G[rb];
            return true;
        }
    return false;
}

// a point of the face's plane on the line A s + B t = C, to the rounding of the three terms
constexpr double kOnLine = 1e-12;

RF_CLIP_HD bool on_line(double A, double B, double C, double s, double t) {
    const double as = A * s, bt = B * t;
    return fabs((as + bt) - C) <= kOnLine * (fabs(as) + fabs(bt) + fabs(C));
}

// Of the two lanes of row a that see the triangle (a,b,c), F_ab (row index k, forward area area_b) and F_ac (j, area_c),
// the one that counts it: the larger face, the lower index between equals (NaN compares as equal).
RF_CLIP_HD bool counts_here(double area_b, double area_c, uint32_t k, uint32_t j) {
    return area_b > area_c || (!(area_c > area_b) && k < j);
}

// lambda_b + lambda_c of the triangle (a,b,c); 0 for collinear sites
RF_CLIP_HD double edge_lambda(double lb, double bx, double by, double bz, double cx, double cy, double cz, double gab,
                              double gac, double gbc) {
    const double nx = by * cz - bz * cy, ny = bz * cx - bx * cz, nz = bx * cy - by * cx;   // d_b x d_c
    const double det = nx * nx + ny * ny + nz * nz;
    if (!(det > 0.0)) return 0.0;
    const double ex = cx - bx, ey = cy - by, ez = cz - bz;
    const double be = bx * ex + by * ey + bz * ez, ce = cx * ex + cy * ey + cz * ez;
    const double lc = sqrt(cx * cx + cy * cy + cz * cz), le = sqrt(ex * ex + ey * ey + ez * ez);
    return ((gac * (ce / lc) - gab * (be / lb)) - gbc * le) / sqrt(det);
}

// the row of a as the serial routine reads it, straight from the arrays
struct RowFromArrays {
    const float *points;
    const uint32_t *adj;   // of the row
    uint32_t a;
    RF_CLIP_HD uint32_t site(uint32_t j) const { return adj[j]; }
    RF_CLIP_HD void plane(uint32_t j, double &dx, double &dy, double &dz, double &h) const {
        neighbour(points, a, adj[j], dx, dy, dz, h);
    }
};

// The terms of grad p_a of the finished polygon (ps, pt, pl)[0..m) of F_ab (row index k, frame f, d_b = (bx,by,bz)),
// added to (gx, gy, gz).  The triangles of an edge are (a,b,x) over the row's sites x whose plane passes through both
// endpoints from the label's side and that b lists; there is one, the label itself, unless more than three sites are
// cocircular around the edge (kOnLine), where the rounding of the clipping decides which of their planes labels it.
// Those n triangles share the edge equally: every row of the four or more sites then finds the same triangles with the
// same shares from the adjacency alone, and the rows add up to the mean of the gradients of the triangulations that the
// adjacency admits.  Where b lists none of them (an asymmetric row) the label's triangle stands with G_bc = 0.
// First every edge takes its label's triangle, then one pass over the row's planes looks for further ones (per plane
// one residual per vertex; anything more only where two neighbouring vertices are on it), then the edges are summed.
// wsum and wn: free buffers of the polygon's stride for the sum of lambdas and the number of triangles per edge (-1:
// the edge is skipped).  row_G and row_area: the row's effective weights and forward areas.
template <typename Row, typename L>
RF_CLIP_HD void add_polygon_terms(const Row &row, uint32_t degree, uint32_t k, const Frame &f, double bx, double by,
                                  double bz, double R, const double *ps, const double *pt, const L *pl, double *wsum,
                                  double *wn, uint32_t stride, uint32_t m, const uint32_t *adj, const uint32_t *offsets,
                                  uint32_t num_edges, const double *G, uint32_t b, const double *row_G,
                                  const double *row_area, double &gx, double &gy, double &gz) {
    const double gab = row_G[k], area_b = row_area[k];
    double cx, cy, cz, h;
    for (uint32_t i = 0; i < m; ++i) {
        const uint32_t j = i + 1 < m ? i + 1 : 0u;
        const L l = pl[i * stride];
        const double s1 = ps[i * stride], t1 = pt[i * stride], s2 = ps[j * stride], t2 = pt[j * stride];
        double sum = 0.0, n = -1.0;
        // not made by the square, not an unbounded Voronoi edge, not of zero length
        if (l != no_label<L>() && fmax(fabs(s1), fabs(t1)) < R && fmax(fabs(s2), fabs(t2)) < R && (s1 != s2 || t1 != t2)) {
            double gbc = 0.0;
            n = listed_weight(adj, offsets, num_edges, G, b, row.site(l), gbc) ? 1.0 : 0.0;
            if (counts_here(area_b, row_area[l], k, l)) {
                row.plane(l, cx, cy, cz, h);
                sum = edge_lambda(f.len, bx, by, bz, cx, cy, cz, gab, row_G[l], gbc);   // with G_bc = 0 where n is 0
            }
        }
        wsum[i * stride] = sum, wn[i * stride] = n;
    }
    for (uint32_t j = 0; j < degree; ++j) {
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

// One whole row of the gradient, face after face: the counterpart of cell_serial (the host harness, and the kernel of
// last resort).  G[E] holds effective_weight of every slot.  s, t and lab have 2 * cap entries.  Writes
// grad_points[3 a ..] (NaN on a status other than kCellOk) and returns a kCell* status.
RF_CLIP_HD uint32_t face_area_grad_serial(const float *points, uint32_t num_points, const uint32_t *adj,
                                          const uint32_t *offsets, uint32_t num_edges, uint32_t a, double R, double *s,
                                          double *t, uint32_t *lab, uint32_t cap, const double *face_area, const double *G,
                                          double *grad_points) {
    const uint32_t begin = offsets[a], end = offsets[a + 1];
    uint32_t status = row_is_valid(points, num_points, adj, num_edges, a, begin, end) ? kCellOk : kCellBadRow;
    double gx = 0.0, gy = 0.0, gz = 0.0;
    for (uint32_t slot = begin; status == kCellOk && slot < end; ++slot) {
        Frame frame;
        uint32_t m, cur;
        if (!face_polygon_labelled(points, adj, a, begin, end, slot, R, s, t, lab, 1u, cap, frame, m, cur)) {
            status = kCellTooManyVertices;
            break;
        }
        const double *ps = s + cur * cap, *pt = t + cur * cap;
        const uint32_t *pl = lab + cur * cap;
        double bx, by, bz, h;
        neighbour(points, a, adj[slot], bx, by, bz, h);
        const RowFromArrays row = {points, adj + begin, a};
        add_polygon_terms(row, end - begin, slot - begin, frame, bx, by, bz, R, ps, pt, pl, s + (cur ^ 1u) * cap,
                          t + (cur ^ 1u) * cap, 1u, m, adj, offsets, num_edges, G, adj[slot], G + begin, face_area + begin, gx,
                          gy, gz);
    }
    if (status != kCellOk) gx = gy = gz = (double)NAN;
    grad_points[3 * (size_t)a] = gx, grad_points[3 * (size_t)a + 1] = gy, grad_points[3 * (size_t)a + 2] = gz;
    return status;
}

}  // namespace clip
}  // namespace rf
