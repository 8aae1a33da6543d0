// rf_cell_moments_grad.hip -- point gradients of the cells' second moments ("Point gradients of the second
// moments").  The mathematics and the per-face arithmetic: rf_clip_moments_grad.hpp, all in double.  The wave scheme, its
// LDS layout and the hand-off through redo[cell]: rf_cell_wave.hpp.
//
//   cell_moments_grad_kernel       the lane clips its face again, takes the polygon's moments up to third order, reads
//                                  its neighbour's twelve upstream numbers, centroid and bounded flag and forms its
//                                  3-vector; three wave sums, and lane 0 adds the direct term -2 V G m and writes the
//                                  row.  Rows of up to 64 faces.
//   cell_moments_grad_redo_kernel  the cells handed on, by rf::clip::cell_moments_grad_serial.
//
// Row a is a gather over a's own adjacency row: every output element is written exactly once by a plain store, there are
// no atomics, and the result is bit-reproducible.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/radfoam_hip_moments_grad.h"
#include "rf_cell_wave.hpp"
#include "rf_clip_moments_grad.hpp"

namespace rf {
namespace moments_grad {

__global__ __launch_bounds__(64) void cell_moments_grad_kernel(
    const float *__restrict__ points, uint32_t num_points, const uint32_t *__restrict__ adj,
    const uint32_t *__restrict__ offsets, uint32_t num_edges, const float *__restrict__ bbox,
    const double *__restrict__ volume, const double *__restrict__ centroid, const uint8_t *__restrict__ bounded,
    const double *__restrict__ grad_site_moment, const double *__restrict__ grad_central_moment,
    double *__restrict__ grad_points, uint8_t *__restrict__ redo) {
    __shared__ double s_plane[4][kWave];             // d_c (x, y, z), |d_c|^2 / 2 of the row
    __shared__ double s_s[2 * kLaneCap][kWave];      // polygons: buffer 0 at vertex rows [0, kLaneCap), buffer 1 after
    __shared__ double s_t[2 * kLaneCap][kWave];
    const uint32_t a = blockIdx.x, lane = threadIdx.x;
    const uint32_t begin = offsets[a], end = offsets[a + 1];
    if (begin > end || end > num_edges || end - begin > kWave) return hand_on(redo, a, lane);   // wave-uniform
    const uint32_t degree = end - begin;
    if (degree == 0) {   // no neighbours: nothing depends on this site through its own row
        if (lane == 0) {
            grad_points[3 * (size_t)a] = grad_points[3 * (size_t)a + 1] = grad_points[3 * (size_t)a + 2] = 0.0;
            keep(redo, a);
        }
        return;
    }
    const CellLane f = stage_row(points, num_points, adj, a, begin, degree, lane, s_plane);
    if (sync_any_bad(f.bad)) return hand_on(redo, a, lane);
    const double R = clip::half_side(bbox);
    bool overflow = false;
    double gx = 0.0, gy = 0.0, gz = 0.0;
    if (f.have) {
        const clip::Frame frame = clip::make_frame(f.dx, f.dy, f.dz);
        double *s = &s_s[0][lane], *t = &s_t[0][lane];
        const Clipped c = clip_by_row(frame, s_plane, degree, lane, R, s, t);
        overflow = c.overflow;
        if (!overflow) {
            const uint32_t at = c.cur * kLaneCap * kWave;
            const clip::Moments3 m3 = clip::moments3(s + at, t + at, kWave, c.m, R);
            if (!m3.m.unbounded) {   // q < num_points: no lane of this wave is bad
                const clip::MomentTerm ca = clip::moment_term(points, a, a, centroid, bounded, grad_site_moment,
                                                              grad_central_moment);
                const clip::MomentTerm cb = clip::moment_term(points, a, f.q, centroid, bounded, grad_site_moment,
                                                              grad_central_moment);
                clip::add_face_moment_grad(frame, m3, ca, cb, gx, gy, gz);
            }
        }
    }
    if (__any(overflow)) return hand_on(redo, a, lane);
    gx = wave_sum(gx), gy = wave_sum(gy), gz = wave_sum(gz);
    if (lane == 0) {
        clip::add_direct_moment_grad(points, a, volume, centroid, bounded, grad_site_moment, gx, gy, gz);
        grad_points[3 * (size_t)a] = gx, grad_points[3 * (size_t)a + 1] = gy, grad_points[3 * (size_t)a + 2] = gz;
        keep(redo, a);
    }
}

__global__ __launch_bounds__(64) void cell_moments_grad_redo_kernel(
    const float *__restrict__ points, uint32_t num_points, const uint32_t *__restrict__ adj,
    const uint32_t *__restrict__ offsets, uint32_t num_edges, const float *__restrict__ bbox,
    const double *__restrict__ volume, const double *__restrict__ centroid, const uint8_t *__restrict__ bounded,
    const double *__restrict__ grad_site_moment, const double *__restrict__ grad_central_moment,
    double *__restrict__ grad_points, const uint8_t *__restrict__ redo, uint8_t *__restrict__ cell_status) {
    __shared__ double s_s[2 * kWaveCap], s_t[2 * kWaveCap];
    unsigned long long todo = redo_todo(num_points, redo, cell_status);
    if (threadIdx.x != 0) return;
    const double R = clip::half_side(bbox);
    while (todo) {
        const uint32_t a = redo_next(todo);
        cell_status[a] = (uint8_t)clip::cell_moments_grad_serial(points, num_points, adj, offsets, num_edges, a, R, s_s,
                                                                 s_t, kWaveCap, volume, centroid, bounded,
                                                                 grad_site_moment, grad_central_moment, grad_points);
    }
}

}  // namespace moments_grad
}  // namespace rf

using namespace rf;

extern "C" {

size_t rf_cell_moments_grad_workspace_bytes(uint32_t num_points) { return redo_bytes(num_points); }

int rf_cell_moments_grad(const float *points, uint32_t num_points, const uint32_t *point_adjacency,
                         const uint32_t *point_adjacency_offsets, uint32_t num_edges, const float *bbox,
                         const double *volume, const double *centroid, const uint8_t *bounded,
                         const double *grad_site_moment, const double *grad_central_moment, double *grad_points,
                         uint8_t *cell_status, void *workspace, size_t workspace_bytes, void *stream) {
    g_err[0] = 0;
    if (num_points == 0) return RF_OK;
    if (!points || !point_adjacency_offsets || !bbox || !volume || !centroid || !bounded || !grad_points ||
        !cell_status || (num_edges && !point_adjacency))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_cell_moments_grad: null pointer");
    if (!workspace || workspace_bytes < rf_cell_moments_grad_workspace_bytes(num_points))
        return fail(RF_ERR_WORKSPACE, "rf_cell_moments_grad: workspace missing or too small");
    return launch_cell_waves("rf_cell_moments_grad", stream, num_points, workspace, cell_status,
                             moments_grad::cell_moments_grad_kernel, moments_grad::cell_moments_grad_redo_kernel, points,
                             num_points, point_adjacency, point_adjacency_offsets, num_edges, bbox, volume, centroid,
                             bounded, grad_site_moment, grad_central_moment, grad_points);
}

}  // extern "C"
