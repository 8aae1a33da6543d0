// rf_clip_grad.hpp -- the backward of the Voronoi cell geometry (rf_cell_geometry_grad.hip) over the clipping core of
// rf_clip.hpp, in double: the gradient of  L = sum_a gV_a V_a + gC_a . c_a  with respect to the sites.
//
// When the sites move by delta, face (a,b) moves outward from a with normal speed
//     v_n(x) = [(x - p_a) . delta_a - (x - p_b) . delta_b] / |d|,   d = p_b - p_a,
// and the transport theorem gives dV_a = sum_b int_F v_n dA, d(V_a c_a) = sum_b int_F x v_n dA.  With the affine
//     phi_a(x) = gV_a + (gC_a / V_a) . (x - c_a)      (phi_a == 0 for an unbounded cell, whatever arrives for it)
// that is  dL = sum_a sum_b int_F phi_a v_n dA,  and collecting delta_a:
//     grad p_a = sum_{b in N(a)} (1 / |d|) int_{F_ab} (phi_a(x) - phi_b(x)) (x - p_a) dA.
// Row a reads per-cell data of its neighbours (gV, gC, V, c, bounded) and the moments of its own face polygons: a
// gather, nothing is scattered.  phi_a - phi_b = k0 + k . y in y = x - p_a, from c_a - p_a and c_b - p_a (never from
// absolute coordinates), and with y = y0 + s' u + t' v (y0 vertex 0 of the polygon, (s',t') relative to it)
//     int (k0 + k . y) y dA = y0 (w A + ku Ms + kv Mt) + u (w Ms + ku Mss + kv Mst) + v (w Mt + ku Mst + kv Mtt),
// w = k0 + k . y0, ku = k . u, kv = k . v, from the polygon's 2-D moments up to second order about vertex 0.
//
// An unbounded face (both of its cells are unbounded) contributes nothing and is skipped before any arithmetic; a
// bounded face of an unbounded row still carries the neighbour's term.  The sum over a's own row is the exact gradient
// when the adjacency is symmetric; a term of a site that lists a but is missing from a's row is dropped.
//
// __host__ __device__ and free of HIP types like rf_clip.hpp: tests/host_harness/clip_grad_host.cpp compiles this file
// with g++ (no FMA contraction on either side).
#pragma once

#include "rf_clip.hpp"

namespace rf {
namespace clip {

// 2-D moments of a polygon about its vertex 0: area, int s', int t', int s's', int s't', int t't'; (s0,t0) is vertex 0
struct Moments {
    double a, s, t, ss, st, tt, s0, t0;
    bool unbounded;   // a piece of the square survived (rf_clip.hpp)
};

// As a fan about vertex 0, like measure(): triangle (0, p, q) with cr = p x q has
//   int s' = cr (ps + qs) / 6,  int s's' = cr (ps^2 + qs^2 + ps qs) / 12,  int s't' = cr (2 ps pt + 2 qs qt + ps qt + qs pt) / 24.
RF_CLIP_HD Moments moments(const double *s, const double *t, uint32_t stride, uint32_t m, double R) {
    Moments o = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, false};
    if (m == 0) return o;
    const double s0 = s[0], t0 = t[0];
    double a2 = 0.0, ms = 0.0, mt = 0.0, mss = 0.0, mst = 0.0, mtt = 0.0;
    double ps = 0.0, pt = 0.0;   // previous vertex relative to vertex 0
    for (uint32_t i = 0; i < m; ++i) {
        const double si = s[i * stride], ti = t[i * stride];
        o.unbounded = o.unbounded || fmax(fabs(si), fabs(ti)) >= R;
        const double qs = si - s0, qt = ti - t0;
        if (i >= 2) {
            const double cr = ps * qt - pt * qs;
            a2 += cr;
            ms += cr * (ps + qs);
            mt += cr * (pt + qt);
            mss += cr * ((ps * ps + qs * qs) + ps * qs);
            mtt += cr * ((pt * pt + qt * qt) + pt * qt);
            mst += cr * (2.0 * (ps * pt + qs * qt) + (ps * qt + qs * pt));
        }
        ps = qs, pt = qt;
    }
    o.a = 0.5 * a2, o.s = ms / 6.0, o.t = mt / 6.0;
    o.ss = mss / 12.0, o.tt = mtt / 12.0, o.st = mst / 24.0;
    o.s0 = s0, o.t0 = t0;
    return o;
}

// what phi_q is made of, relative to the site p_a of the row being gathered: gV_q, gC_q / V_q, c_q - p_a; all zero
// for an unbounded cell (its upstream gradients are never read) and where an upstream array is absent
struct CellTerm {
    double gv, gx, gy, gz, cx, cy, cz;
};

RF_CLIP_HD CellTerm cell_term(const float *points, uint32_t a, uint32_t q, const double *volume, const double *centroid,
                              const uint8_t *bounded, const double *grad_volume, const double *grad_centroid) {
    CellTerm c = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (!bounded[q]) return c;
    if (grad_volume) c.gv = grad_volume[q];
    if (grad_centroid) {
        const double v = volume[q];
        c.gx = grad_centroid[3 * (size_t)q] / v, c.gy = grad_centroid[3 * (size_t)q + 1] / v;
        c.gz = grad_centroid[3 * (size_t)q + 2] / v;
    }
    c.cx = centroid[3 * (size_t)q] - (double)points[3 * (size_t)a];
    c.cy = centroid[3 * (size_t)q + 1] - (double)points[3 * (size_t)a + 1];
    c.cz = centroid[3 * (size_t)q + 2] - (double)points[3 * (size_t)a + 2];
    return c;
}

// face (a,b)'s term of grad p_a: (1 / |d|) int (phi_a - phi_b)(p_a + y) y dA, added to (gx, gy, gz)
RF_CLIP_HD void add_face_grad(const Frame &f, const Moments &mo, const CellTerm &ca, const CellTerm &cb, double &gx,
                              double &gy, double &gz) {
    if (mo.unbounded) return;
    const double kx = ca.gx - cb.gx, ky = ca.gy - cb.gy, kz = ca.gz - cb.gz;
    const double k0 = ((ca.gv - cb.gv) - (ca.gx * ca.cx + ca.gy * ca.cy + ca.gz * ca.cz)) +
                      (cb.gx * cb.cx + cb.gy * cb.cy + cb.gz * cb.cz);
    double x0, y0, z0;
    to_space(f, mo.s0, mo.t0, x0, y0, z0);
    const double w = k0 + (kx * x0 + ky * y0 + kz * z0);
    const double ku = kx * f.ux + ky * f.uy + kz * f.uz, kv = kx * f.vx + ky * f.vy + kz * f.vz;
    const double f0 = (w * mo.a + ku * mo.s) + kv * mo.t;
    const double fu = (w * mo.s + ku * mo.ss) + kv * mo.st;
    const double fv = (w * mo.t + ku * mo.st) + kv * mo.tt;
    gx += ((x0 * f0 + f.ux * fu) + f.vx * fv) / f.len;
    gy += ((y0 * f0 + f.uy * fu) + f.vy * fv) / f.len;
    gz += ((z0 * f0 + f.uz * fu) + f.vz * fv) / f.len;
}

// One whole row of the gradient, face after face: the counterpart of cell_serial (the host harness, and the kernel of
// last resort).  volume / centroid / bounded are the forward's outputs; grad_volume and grad_centroid may be null.
// Writes grad_points[3 a ..] (NaN on a status other than kCellOk) and returns a kCell* status.
RF_CLIP_HD uint32_t cell_grad_serial(const float *points, uint32_t num_points, const uint32_t *adj,
                                     const uint32_t *offsets, uint32_t num_edges, uint32_t a, double R, double *s,
                                     double *t, uint32_t cap, const double *volume, const double *centroid,
                                     const uint8_t *bounded, const double *grad_volume, const double *grad_centroid,
                                     double *grad_points) {
    const uint32_t begin = offsets[a], end = offsets[a + 1];
    uint32_t status = row_is_valid(points, num_points, adj, num_edges, a, begin, end) ? kCellOk : kCellBadRow;
    double gx = 0.0, gy = 0.0, gz = 0.0;
    if (status == kCellOk && begin < end) {
        const CellTerm ca = cell_term(points, a, a, volume, centroid, bounded, grad_volume, grad_centroid);
        for (uint32_t slot = begin; slot < end; ++slot) {
            Frame frame;
            uint32_t m, cur;
            if (!face_polygon(points, adj, a, begin, end, slot, R, s, t, 1u, cap, frame, m, cur)) {
                status = kCellTooManyVertices;
                break;
            }
            const Moments mo = moments(s + cur * cap, t + cur * cap, 1u, m, R);
            const CellTerm cb = cell_term(points, a, adj[slot], volume, centroid, bounded, grad_volume, grad_centroid);
            add_face_grad(frame, mo, ca, cb, gx, gy, gz);
        }
    }
    if (status != kCellOk) gx = gy = gz = (double)NAN;
    grad_points[3 * (size_t)a] = gx, grad_points[3 * (size_t)a + 1] = gy, grad_points[3 * (size_t)a + 2] = gz;
    return status;
}

}  // namespace clip
}  // namespace rf
