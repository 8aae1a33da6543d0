// rf_clip_box_moments_grad.hpp -- the backward of the second moments of the Voronoi cells clipped to a box
// (rf_cell_box_moments_grad.hip), fused with the backward of their volumes and centroids: the gradient of
//     L = sum_a <S(gQ_a), Q_a> + <S(gC_a), C_a> + gV_a V_a + gc_a . c_a     over the non-empty boxed cells
// with respect to the sites, the box fixed, in double ("Point gradients of the second moments in a box").
// Q_a and C_a are the site and central moment of rf_clip_box_moments.hpp, V_a and c_a the volume and centroid of
// rf_clip_box.hpp, S(g) the six-number convention of rf_clip_moments_grad.hpp.
//
// The walls do not move, so only the row's faces carry a boundary term, each by its part inside the box:
//     grad p_a = sum_{b in row(a)} (1 / |d|) int_{F_ab n box} (Psi_a(x) - Psi_b(x)) (x - p_a) dA  -  2 V_a G_a m_a,
// m_a = c_a - p_a, G_a = S(gQ_a).  In y = x - p_a a non-empty cell q of the row (a itself or a neighbour) is the quadratic
//     Psi_q(y) = y^T K_q y + l_q . y + k_q,   K_q = G_q + H_q,   l_q = -2 (G_q r_q + H_q e_q) + gc_q / V_q,
//     k_q = r_q^T G_q r_q + e_q^T H_q e_q + gV_q - (gc_q / V_q) . e_q,     r_q = p_q - p_a,  e_q = c_q - p_a
// (never from absolute coordinates): the moment_term of rf_clip_moments_grad.hpp plus the affine phi_q of
// rf_clip_grad.hpp, ten doubles, with `nonempty` in the place of `bounded`.  Psi_q == 0 for an empty cell, whatever
// arrives for it, and its NaN centroid is never read.  The face integral is add_face_moment_grad over moments3 as it is.
//
// The direct term -2 V_a G_a m_a is the site moment's alone: the central moment has none (c_a is the centroid of the
// clipped cell), nor have the volume and the centroid.  It is there whenever the cell is non-empty, also for an EMPTY ROW:
// that cell is the whole box wherever the site is, and grad p_a = -2 V_box G_a (centre - p_a).
//
// The polygon of face (a,b) is the forward's: face i < degree of the plane list of rf_clip_box.hpp (the row in row order,
// then the six walls), the same R, clip_by_list_plane with its tie rule, the list order.  A face with an empty cell on
// either side carries no term and is not clipped, and an empty cell's row is zero, for the reasons of
// rf_clip_box_grad.hpp.
//
// __host__ __device__ and free of HIP types: tests/host_harness/clip_box_moments_grad_host.cpp compiles this file with
// g++ (no FMA contraction on either side).
#pragma once

#include "rf_clip_box.hpp"
#include "rf_clip_grad.hpp"
#include "rf_clip_moments_grad.hpp"

namespace rf {
namespace clip {

// Psi_q in y = x - p_a: moment_term over `nonempty`, plus the linear and constant parts of the volume and centroid
// upstreams; any of the four arrays may be null.  All zero (`bounded` false) for an empty cell.
RF_CLIP_HD MomentTerm box_moment_term(const float *points, uint32_t a, uint32_t q, const double *volume,
                                      const double *centroid, const uint8_t *nonempty, const double *grad_site_moment,
                                      const double *grad_central_moment, const double *grad_volume,
                                      const double *grad_centroid) {
    MomentTerm c = moment_term(points, a, q, centroid, nonempty, grad_site_moment, grad_central_moment);
    if (!c.bounded) return c;
    if (grad_volume) c.k += grad_volume[q];
    if (grad_centroid) {
        const double v = volume[q];
        const double lx = grad_centroid[3 * (size_t)q] / v, ly = grad_centroid[3 * (size_t)q + 1] / v,
                     lz = grad_centroid[3 * (size_t)q + 2] / v;
        const double ex = centroid[3 * (size_t)q] - (double)points[3 * (size_t)a];
        const double ey = centroid[3 * (size_t)q + 1] - (double)points[3 * (size_t)a + 1];
        const double ez = centroid[3 * (size_t)q + 2] - (double)points[3 * (size_t)a + 2];
        c.lx += lx, c.ly += ly, c.lz += lz;
        c.k -= (lx * ex + ly * ey) + lz * ez;
    }
    return c;
}

// One whole row of the gradient, row face after row face, then the direct term (the host harness, and the kernel of
// last resort).  volume / centroid / nonempty are the outputs of cell_box_serial or cell_box_kernel; each of the four
// upstreams may be null.  Writes grad_points[3 a ..] (NaN on a status other than kCellOk) and returns a kCell* status;
// s and t hold 2 cap each.
RF_CLIP_HD uint32_t cell_box_moments_grad_serial(const float *points, uint32_t num_points, const uint32_t *adj,
                                                 const uint32_t *offsets, uint32_t num_edges, uint32_t a, const Box &box,
                                                 double R, double *s, double *t, uint32_t cap, const double *volume,
                                                 const double *centroid, const uint8_t *nonempty,
                                                 const double *grad_site_moment, const double *grad_central_moment,
                                                 const double *grad_volume, const double *grad_centroid,
                                                 double *grad_points) {
    const uint32_t begin = offsets[a], end = offsets[a + 1];
    uint32_t status = row_is_valid(points, num_points, adj, num_edges, a, begin, end) ? kCellOk : kCellBadRow;
    double gx = 0.0, gy = 0.0, gz = 0.0;
    if (status == kCellOk && nonempty[a]) {
        if (begin < end) {
            const MomentTerm ca = box_moment_term(points, a, a, volume, centroid, nonempty, grad_site_moment,
                                                  grad_central_moment, grad_volume, grad_centroid);
            for (uint32_t i = 0; i < end - begin; ++i) {
                if (!nonempty[adj[begin + i]]) continue;
                Frame frame;
                bool wall;
                double h;
                uint32_t m, cur;
                if (!face_polygon_box(points, adj, a, begin, end, box, i, R, s, t, 1u, cap, frame, wall, h, m, cur)) {
                    status = kCellTooManyVertices;
                    break;
                }
                const Moments3 m3 = moments3(s + cur * cap, t + cur * cap, 1u, m, R);
                const MomentTerm cb = box_moment_term(points, a, adj[begin + i], volume, centroid, nonempty,
                                                      grad_site_moment, grad_central_moment, grad_volume,
                                                      grad_centroid);
                add_face_moment_grad(frame, m3, ca, cb, gx, gy, gz);
            }
        }
        add_direct_moment_grad(points, a, volume, centroid, nonempty, grad_site_moment, gx, gy, gz);
    }
    if (status != kCellOk) gx = gy = gz = (double)NAN;
    grad_points[3 * (size_t)a] = gx, grad_points[3 * (size_t)a + 1] = gy, grad_points[3 * (size_t)a + 2] = gz;
    return status;
}

}  // namespace clip
}  // namespace rf
