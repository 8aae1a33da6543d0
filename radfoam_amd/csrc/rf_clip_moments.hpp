// rf_clip_moments.hpp -- the second moments of the Voronoi cells (rf_cell_moments.hip) over the clipping core of
// rf_clip.hpp and the polygon moments of rf_clip_grad.hpp, in double ("Second moments of the cells").
//
// In y = x - p_a, face (a,b) lies in the plane at height |d_b| / 2 over the site, and the cell is the union of the
// pyramids over its faces with the apex at y = 0.  A point of the pyramid is lambda y with y on the face, lambda in [0,1],
// and dy = lambda^2 (|d_b| / 2) dlambda dA, so
//     int_pyramid y y^T dy = (|d_b| / 2) int_0^1 lambda^4 dlambda  int_F y y^T dA = (|d_b| / 10) F_ab.
// With y = y0 + s' u + t' v (y0 vertex 0 of the polygon, (s',t') relative to it) and the polygon's moments about vertex 0
//     F_ab = a y0 y0^T + s (y0 u^T + u y0^T) + t (y0 v^T + v y0^T) + ss u u^T + st (u v^T + v u^T) + tt v v^T.
// site_moment[a] = sum_b (|d_b| / 10) F_ab = int_cell y y^T dy, whose trace is the cell's centroidal-Voronoi energy;
// central_moment[a] = site_moment[a] - V_a m m^T with m = c_a - p_a is the moment about the centroid, V_a times the
// covariance of the uniform distribution on the cell.  Six numbers each: xx, yy, zz, xy, xz, yz.
//
// An unbounded cell (bounded[a] == 0, or no neighbours) has no moments: twelve NaN, and its faces are not clipped.  A face
// of zero area has zero moments and adds exactly 0.
//
// __host__ __device__ and free of HIP types like rf_clip.hpp: tests/host_harness/clip_moments_host.cpp compiles this file
// with g++ (no FMA contraction on either side).
#pragma once

#include "rf_clip.hpp"
#include "rf_clip_grad.hpp"

namespace rf {
namespace clip {

// what a cell accumulates over its faces: int y y^T dy as xx, yy, zz, xy, xz, yz
struct MomentSums {
    double xx, yy, zz, xy, xz, yz;
    bool unbounded;
};

// entry (i,j) of F_ab from the components i and j of y0 (pi, pj), u and v
RF_CLIP_HD double face_moment_entry(const Moments &mo, double pi, double pj, double ui, double uj, double vi,
                                    double vj) {
    return ((mo.a * (pi * pj) + mo.s * (pi * uj + ui * pj)) + mo.t * (pi * vj + vi * pj)) +
           ((mo.ss * (ui * uj) + mo.st * (ui * vj + vi * uj)) + mo.tt * (vi * vj));
}

// face (a,b)'s pyramid over the site: (|d_b| / 10) F_ab, added to the six sums
RF_CLIP_HD void add_face_moment(MomentSums &q, const Frame &f, const Moments &mo) {
    if (mo.unbounded) {
        q.unbounded = true;
        return;
    }
    double x0, y0, z0;
    to_space(f, mo.s0, mo.t0, x0, y0, z0);
    const double w = f.len / 10.0;
    q.xx += w * face_moment_entry(mo, x0, x0, f.ux, f.ux, f.vx, f.vx);
    q.yy += w * face_moment_entry(mo, y0, y0, f.uy, f.uy, f.vy, f.vy);
    q.zz += w * face_moment_entry(mo, z0, z0, f.uz, f.uz, f.vz, f.vz);
    q.xy += w * face_moment_entry(mo, x0, y0, f.ux, f.uy, f.vx, f.vy);
    q.xz += w * face_moment_entry(mo, x0, z0, f.ux, f.uz, f.vx, f.vz);
    q.yz += w * face_moment_entry(mo, y0, z0, f.uy, f.uz, f.vy, f.vz);
}

// the twelve numbers of cell a from its six sums and what rf_cell_geometry wrote for it (NaN for an unbounded cell)
RF_CLIP_HD void write_moments(const float *points, uint32_t a, const MomentSums &q, const double *volume,
                              const double *centroid, double *site_moment, double *central_moment) {
    double *site = site_moment + 6 * (size_t)a, *central = central_moment + 6 * (size_t)a;
    if (q.unbounded) {
        for (uint32_t k = 0; k < 6u; ++k) site[k] = central[k] = (double)NAN;
        return;
    }
    const double v = volume[a];
    const double mx = centroid[3 * (size_t)a] - (double)points[3 * (size_t)a];
    const double my = centroid[3 * (size_t)a + 1] - (double)points[3 * (size_t)a + 1];
    const double mz = centroid[3 * (size_t)a + 2] - (double)points[3 * (size_t)a + 2];
    site[0] = q.xx, site[1] = q.yy, site[2] = q.zz, site[3] = q.xy, site[4] = q.xz, site[5] = q.yz;
    central[0] = q.xx - v * (mx * mx), central[1] = q.yy - v * (my * my), central[2] = q.zz - v * (mz * mz);
    central[3] = q.xy - v * (mx * my), central[4] = q.xz - v * (mx * mz), central[5] = q.yz - v * (my * mz);
}

// One whole cell, face after face: the counterpart of cell_serial / cell_grad_serial (the host harness, and the kernel of
// last resort).  volume / centroid / bounded are what rf_cell_geometry wrote.  Writes site_moment[6 a ..] and
// central_moment[6 a ..] (NaN for an unbounded cell and on a status other than kCellOk) and returns a kCell* status.
RF_CLIP_HD uint32_t cell_moments_serial(const float *points, uint32_t num_points, const uint32_t *adj,
                                        const uint32_t *offsets, uint32_t num_edges, uint32_t a, double R, double *s,
                                        double *t, uint32_t cap, const double *volume, const double *centroid,
                                        const uint8_t *bounded, double *site_moment, double *central_moment) {
    const uint32_t begin = offsets[a], end = offsets[a + 1];
    uint32_t status = row_is_valid(points, num_points, adj, num_edges, a, begin, end) ? kCellOk : kCellBadRow;
    MomentSums q = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, begin == end || !bounded[a]};
    for (uint32_t slot = begin; status == kCellOk && !q.unbounded && slot < end; ++slot) {
        Frame frame;
        uint32_t m, cur;
        if (!face_polygon(points, adj, a, begin, end, slot, R, s, t, 1u, cap, frame, m, cur)) {
            status = kCellTooManyVertices;
            break;
        }
        add_face_moment(q, frame, moments(s + cur * cap, t + cur * cap, 1u, m, R));
    }
    if (status != kCellOk) q.unbounded = true;
    write_moments(points, a, q, volume, centroid, site_moment, central_moment);
    return status;
}

}  // namespace clip
}  // namespace rf
