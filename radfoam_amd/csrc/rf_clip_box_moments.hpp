// rf_clip_box_moments.hpp -- the second moments of the Voronoi cells clipped to an axis-aligned box
// (rf_cell_box_moments.hip): the plane list, wall frames and tie rule of rf_clip_box.hpp, the polygon moments of
// rf_clip_grad.hpp and their lift into space of rf_clip_moments.hpp, in double ("Second moments of the cells
// clipped to a box").
//
// In y = x - p_a, every plane i of the list of cell_box(a) = cell(a) n box carries a face F_i (face_polygon_box: the
// square of half-side R = half_side_box(bbox, box) clipped by every other plane of the list, coincident planes by the tie
// rule), and F_i = int_{F_i} y y^T dA comes from rf::clip::moments through face_moment_entry.  div(y y_i y_j) = 5 y_i y_j,
// and y . n = h_i on face i, so
//     int_{cell_box(a)} y y^T dy = sum_i (h_i / 5) F_i,
// h_i the SIGNED height of plane i over the site: |d_b| / 2 for a row face (the weight |d_b| / 10 of add_face_moment), h_w
// for a wall, negative when the site is outside that wall.  The signed sum is the moment of cell(a) n box also for a site
// outside the box, exactly as the signed pyramid sum is its volume.
//
//   site_moment[a]     that sum as it is: xx, yy, zz, xy, xz, yz.  An exactly empty intersection leaves no polygon and
//                      gives exactly 0 in all six.
//   central_moment[a]  site_moment[a] - V_a m m^T, m = centroid[a] - p_a, with the volume and centroid rf_cell_box wrote;
//                      NaN in all six where nonempty[a] is false.
//   an empty row       the cell is the whole box, a closed form without clipping: with lo' = lo - p, hi' = hi - p and
//                      e = hi - lo, the diagonal is  ex ey ez / 3 ((hi'_k)^3 - (lo'_k)^3) / e_k  on axis k, formed as
//                      V / 3 (hi'_k^2 + hi'_k lo'_k + lo'_k^2), the same number without the cancellation; the off-diagonals
//                      are V m_i m_j with m = centre - p; the central moment is diag(V e_k^2 / 12), off-diagonals exactly 0.
//   a malformed row, a polygon beyond the capacity: the status says so and all twelve numbers are NaN.
//   a polygon that still reaches the square (Moments::unbounded) cannot occur once the walls have clipped it; if it does,
//   the cell is NaN rather than wrong.
//
// __host__ __device__ and free of HIP types like rf_clip.hpp: tests/host_harness/clip_box_moments_host.cpp compiles this
// file with g++ (no FMA contraction on either side).
#pragma once

#include "rf_clip_box.hpp"
#include "rf_clip_grad.hpp"
#include "rf_clip_moments.hpp"

namespace rf {
namespace clip {

// face i's signed pyramid over the site: (h_i / 5) F_i, added to the six sums.  A row face has h_i = f.len / 2.
RF_CLIP_HD void add_face_moment_box(MomentSums &q, const Frame &f, bool wall, double h, const Moments &mo) {
    if (mo.unbounded) {
        q.unbounded = true;
        return;
    }
    double x0, y0, z0;
    to_space(f, mo.s0, mo.t0, x0, y0, z0);
    const double w = wall ? h / 5.0 : f.len / 10.0;
    q.xx += w * face_moment_entry(mo, x0, x0, f.ux, f.ux, f.vx, f.vx);
    q.yy += w * face_moment_entry(mo, y0, y0, f.uy, f.uy, f.vy, f.vy);
    q.zz += w * face_moment_entry(mo, z0, z0, f.uz, f.uz, f.vz, f.vz);
    q.xy += w * face_moment_entry(mo, x0, y0, f.ux, f.uy, f.vx, f.vy);
    q.xz += w * face_moment_entry(mo, x0, z0, f.ux, f.uz, f.vx, f.vz);
    q.yz += w * face_moment_entry(mo, y0, z0, f.uy, f.uz, f.vy, f.vz);
}

// the cell of an empty row: the whole box, in closed form
RF_CLIP_HD void whole_box_moments(const float *points, uint32_t a, const Box &box, double *site_moment,
                                  double *central_moment) {
    const double px = (double)points[3 * (size_t)a], py = (double)points[3 * (size_t)a + 1],
                 pz = (double)points[3 * (size_t)a + 2];
    const double ex = box.hix - box.lox, ey = box.hiy - box.loy, ez = box.hiz - box.loz;
    const double v = ex * ey * ez;
    const double ax = box.lox - px, bx = box.hix - px, ay = box.loy - py, by = box.hiy - py, az = box.loz - pz,
                 bz = box.hiz - pz;
    const double mx = 0.5 * (box.lox + box.hix) - px, my = 0.5 * (box.loy + box.hiy) - py,
                 mz = 0.5 * (box.loz + box.hiz) - pz;
    double *site = site_moment + 6 * (size_t)a, *central = central_moment + 6 * (size_t)a;
    site[0] = v / 3.0 * ((bx * bx + ax * ax) + ax * bx);
    site[1] = v / 3.0 * ((by * by + ay * ay) + ay * by);
    site[2] = v / 3.0 * ((bz * bz + az * az) + az * bz);
    site[3] = v * (mx * my), site[4] = v * (mx * mz), site[5] = v * (my * mz);
    central[0] = v * (ex * ex) / 12.0, central[1] = v * (ey * ey) / 12.0, central[2] = v * (ez * ez) / 12.0;
    central[3] = central[4] = central[5] = 0.0;
}

// the twelve numbers of cell a from its six sums and what rf_cell_box wrote for it
RF_CLIP_HD void write_moments_box(const float *points, uint32_t a, const MomentSums &q, const double *volume,
                                  const double *centroid, const uint8_t *nonempty, double *site_moment,
                                  double *central_moment) {
    double *site = site_moment + 6 * (size_t)a, *central = central_moment + 6 * (size_t)a;
    if (q.unbounded) {
        for (uint32_t k = 0; k < 6u; ++k) site[k] = central[k] = (double)NAN;
        return;
    }
    site[0] = q.xx, site[1] = q.yy, site[2] = q.zz, site[3] = q.xy, site[4] = q.xz, site[5] = q.yz;
    if (!nonempty[a]) {
        for (uint32_t k = 0; k < 6u; ++k) central[k] = (double)NAN;
        return;
    }
    const double v = volume[a];
    const double mx = centroid[3 * (size_t)a] - (double)points[3 * (size_t)a];
    const double my = centroid[3 * (size_t)a + 1] - (double)points[3 * (size_t)a + 1];
    const double mz = centroid[3 * (size_t)a + 2] - (double)points[3 * (size_t)a + 2];
    central[0] = q.xx - v * (mx * mx), central[1] = q.yy - v * (my * my), central[2] = q.zz - v * (mz * mz);
    central[3] = q.xy - v * (mx * my), central[4] = q.xz - v * (mx * mz), central[5] = q.yz - v * (my * mz);
}

// One whole cell, face after face of its list: the counterpart of cell_box_serial / cell_moments_serial (the host
// harness, and the kernel of last resort).  volume / centroid / nonempty are what rf_cell_box wrote.  Writes
// site_moment[6 a ..] and central_moment[6 a ..] (NaN on a status other than kCellOk) and returns a kCell* status.
RF_CLIP_HD uint32_t cell_box_moments_serial(const float *points, uint32_t num_points, const uint32_t *adj,
                                            const uint32_t *offsets, uint32_t num_edges, uint32_t a, const Box &box,
                                            double R, double *s, double *t, uint32_t cap, const double *volume,
                                            const double *centroid, const uint8_t *nonempty, double *site_moment,
                                            double *central_moment) {
    const uint32_t begin = offsets[a], end = offsets[a + 1];
    uint32_t status = row_is_valid(points, num_points, adj, num_edges, a, begin, end) ? kCellOk : kCellBadRow;
    if (status == kCellOk && begin == end) {
        whole_box_moments(points, a, box, site_moment, central_moment);
        return status;
    }
    const uint32_t count = status == kCellOk ? end - begin + kWalls : 0u;
    MomentSums q = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, false};
    for (uint32_t i = 0; i < count && !q.unbounded; ++i) {
        Frame frame;
        bool wall;
        double h;
        uint32_t m, cur;
        if (!face_polygon_box(points, adj, a, begin, end, box, i, R, s, t, 1u, cap, frame, wall, h, m, cur)) {
            status = kCellTooManyVertices;
            break;
        }
        add_face_moment_box(q, frame, wall, h, moments(s + cur * cap, t + cur * cap, 1u, m, R));
    }
    if (status != kCellOk) q.unbounded = true;
    write_moments_box(points, a, q, volume, centroid, nonempty, site_moment, central_moment);
    return status;
}

}  // namespace clip
}  // namespace rf
