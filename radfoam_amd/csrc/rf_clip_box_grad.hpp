// rf_clip_box_grad.hpp -- the backward of the Voronoi cells clipped to a box (rf_cell_box_grad.hip): the gradient of
// L = sum_a gV_a V_a + gC_a . c_a  over the non-empty boxed cells with respect to the sites, in double (DESIGN.md,
// "Point gradients of the cells in a box").
//
// The box is fixed: its walls have normal speed 0, so only the row's faces carry a term, and the transport theorem of
// rf_clip_grad.hpp holds with every face replaced by its part inside the box:
//     grad p_a = sum_{b in row(a)} (1 / |d|) int_{F_ab n box} (phi_a(x) - phi_b(x)) (x - p_a) dA,
//     phi_a(x) = gV_a + (gC_a / V_a) . (x - c_a)  where nonempty[a],  phi_a == 0 where not (whatever arrives for it).
// The polygon of face (a,b) is the forward's: face i < degree of the plane list of rf_clip_box.hpp (the row in row
// order, then the six walls), the same R, clip_by_list_plane with its tie rule, the list order.  The walls are clip
// planes only.  A face with an empty cell on either side carries no term and is not clipped: in exact arithmetic its part
// inside the box has area zero, or the empty cell is flat against a wall that coincides with the bisector, and the wall
// does not move (rf_clip_box.hpp keeps that face's area on the row's side; taken with phi == 0 beyond it, it would break
// sum V = V_box, which holds on both sides of the kink).  So an empty cell's row is zero.  Moments, the per-cell terms
// (`nonempty` in the place of `bounded`) and the single-face term are those of rf_clip_grad.hpp, V and c the forward's
// boxed values, entering relative to p_a.
//
// __host__ __device__ and free of HIP types: tests/host_harness/clip_box_grad_host.cpp compiles this file with g++ (no
// FMA contraction on either side).
#pragma once

#include "rf_clip_box.hpp"
#include "rf_clip_grad.hpp"

namespace rf {
namespace clip {

// One whole row of the gradient, row face after row face (the host harness, and the kernel of last resort).  volume /
// centroid / nonempty are the outputs of cell_box_serial or cell_box_kernel; grad_volume and grad_centroid may be null.
// Writes grad_points[3 a ..] (NaN on a status other than kCellOk) and returns a kCell* status; s and t hold 2 cap each.
RF_CLIP_HD uint32_t cell_box_grad_serial(const float *points, uint32_t num_points, const uint32_t *adj,
                                         const uint32_t *offsets, uint32_t num_edges, uint32_t a, const Box &box, double R,
                                         double *s, double *t, uint32_t cap, const double *volume, const double *centroid,
                                         const uint8_t *nonempty, const double *grad_volume, const double *grad_centroid,
                                         double *grad_points) {
    const uint32_t begin = offsets[a], end = offsets[a + 1];
    uint32_t status = row_is_valid(points, num_points, adj, num_edges, a, begin, end) ? kCellOk : kCellBadRow;
    double gx = 0.0, gy = 0.0, gz = 0.0;
    if (status == kCellOk && begin < end && nonempty[a]) {
        const CellTerm ca = cell_term(points, a, a, volume, centroid, nonempty, grad_volume, grad_centroid);
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
            const Moments mo = moments(s + cur * cap, t + cur * cap, 1u, m, R);
            const CellTerm cb = cell_term(points, a, adj[begin + i], volume, centroid, nonempty, grad_volume,
                                          grad_centroid);
            add_face_grad(frame, mo, ca, cb, gx, gy, gz);
        }
    }
    if (status != kCellOk) gx = gy = gz = (double)NAN;
    grad_points[3 * (size_t)a] = gx, grad_points[3 * (size_t)a + 1] = gy, grad_points[3 * (size_t)a + 2] = gz;
    return status;
}

}  // namespace clip
}  // namespace rf
