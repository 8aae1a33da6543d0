// rf_cell_moments.hip -- the second moments of the Voronoi cells: int y y^T dy about the site and about the centroid
// ("Second moments of the cells").  The mathematics and the per-face arithmetic: rf_clip_moments.hpp, all in
// double.  The wave scheme, its LDS layout and the hand-off through redo[cell]: rf_cell_wave.hpp.
//
//   cell_moments_kernel       the lane clips its face again (the forward keeps no moments: 48 B a face) and lifts the
//                             polygon's moments into its pyramid's six sums; six wave sums, and lane 0 forms the central
//                             moment and writes the twelve numbers.  An unbounded cell is NaN before anything is clipped.
//                             Rows of up to 64 faces.
//   cell_moments_redo_kernel  the cells handed on, by rf::clip::cell_moments_serial.
//
// Cell a is a gather over a's own adjacency row: every output element is written exactly once by a plain store, there are
// no atomics, and the result is bit-reproducible.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/radfoam_hip_moments.h"
#include "rf_cell_wave.hpp"
#include "rf_clip_moments.hpp"

namespace rf {
namespace cell_moments {

__global__ __launch_bounds__(64) void cell_moments_kernel(
    const float *__restrict__ points, uint32_t num_points, const uint32_t *__restrict__ adj,
    const uint32_t *__restrict__ offsets, uint32_t num_edges, const float *__restrict__ bbox,
    const double *__restrict__ volume, const double *__restrict__ centroid, const uint8_t *__restrict__ bounded,
    double *__restrict__ site_moment, double *__restrict__ central_moment, uint8_t *__restrict__ redo) {
    __shared__ double s_plane[4][kWave];             // d_c (x, y, z), |d_c|^2 / 2 of the row
    __shared__ double s_s[2 * kLaneCap][kWave];      // polygons: buffer 0 at vertex rows [0, kLaneCap), buffer 1 after
    __shared__ double s_t[2 * kLaneCap][kWave];
    const uint32_t a = blockIdx.x, lane = threadIdx.x;
    const uint32_t begin = offsets[a], end = offsets[a + 1];
    if (begin > end || end > num_edges || end - begin > kWave) return hand_on(redo, a, lane);   // wave-uniform
    const uint32_t degree = end - begin;
    const CellLane f = stage_row(points, num_points, adj, a, begin, degree, lane, s_plane);
    if (sync_any_bad(f.bad)) return hand_on(redo, a, lane);   // a malformed row says so in its status, bounded or not
    clip::MomentSums sums = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, degree == 0 || !bounded[a]};
    if (sums.unbounded) {   // wave-uniform: no moments, and nothing is clipped
        if (lane == 0) {
            clip::write_moments(points, a, sums, volume, centroid, site_moment, central_moment);
            keep(redo, a);
        }
        return;
    }
    const double R = clip::half_side(bbox);
    bool overflow = false;
    if (f.have) {
        const clip::Frame frame = clip::make_frame(f.dx, f.dy, f.dz);
        double *s = &s_s[0][lane], *t = &s_t[0][lane];
        const Clipped c = clip_by_row(frame, s_plane, degree, lane, R, s, t);
        overflow = c.overflow;
        if (!overflow) {
            const uint32_t at = c.cur * kLaneCap * kWave;
            clip::add_face_moment(sums, frame, clip::moments(s + at, t + at, kWave, c.m, R));
        }
    }
    if (__any(overflow)) return hand_on(redo, a, lane);
    sums.unbounded = __any(sums.unbounded);   // a face of a cell called bounded came out open: the geometry is not this row's
    sums.xx = wave_sum(sums.xx), sums.yy = wave_sum(sums.yy), sums.zz = wave_sum(sums.zz);
    sums.xy = wave_sum(sums.xy), sums.xz = wave_sum(sums.xz), sums.yz = wave_sum(sums.yz);
    if (lane == 0) {
        clip::write_moments(points, a, sums, volume, centroid, site_moment, central_moment);
        keep(redo, a);
    }
}

__global__ __launch_bounds__(64) void cell_moments_redo_kernel(
    const float *__restrict__ points, uint32_t num_points, const uint32_t *__restrict__ adj,
    const uint32_t *__restrict__ offsets, uint32_t num_edges, const float *__restrict__ bbox,
    const double *__restrict__ volume, const double *__restrict__ centroid, const uint8_t *__restrict__ bounded,
    double *__restrict__ site_moment, double *__restrict__ central_moment, const uint8_t *__restrict__ redo,
    uint8_t *__restrict__ cell_status) {
    __shared__ double s_s[2 * kWaveCap], s_t[2 * kWaveCap];
    unsigned long long todo = redo_todo(num_points, redo, cell_status);
    if (threadIdx.x != 0) return;
    const double R = clip::half_side(bbox);
    while (todo) {
        const uint32_t a = redo_next(todo);
        cell_status[a] = (uint8_t)clip::cell_moments_serial(points, num_points, adj, offsets, num_edges, a, R, s_s, s_t,
                                                            kWaveCap, volume, centroid, bounded, site_moment,
                                                            central_moment);
    }
}

}  // namespace cell_moments
}  // namespace rf

using namespace rf;

extern "C" {

size_t rf_cell_moments_workspace_bytes(uint32_t num_points) { return redo_bytes(num_points); }

int rf_cell_moments(const float *points, uint32_t num_points, const uint32_t *point_adjacency,
                    const uint32_t *point_adjacency_offsets, uint32_t num_edges, const float *bbox,
                    const double *volume, const double *centroid, const uint8_t *bounded, double *site_moment,
                    double *central_moment, uint8_t *cell_status, void *workspace, size_t workspace_bytes,
                    void *stream) {
    g_err[0] = 0;
    if (num_points == 0) return RF_OK;
    if (!points || !point_adjacency_offsets || !bbox || !volume || !centroid || !bounded || !site_moment ||
        !central_moment || !cell_status || (num_edges && !point_adjacency))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_cell_moments: null pointer");
    if (!workspace || workspace_bytes < rf_cell_moments_workspace_bytes(num_points))
        return fail(RF_ERR_WORKSPACE, "rf_cell_moments: workspace missing or too small");
    return launch_cell_waves("rf_cell_moments", stream, num_points, workspace, cell_status,
                             cell_moments::cell_moments_kernel, cell_moments::cell_moments_redo_kernel, points,
                             num_points, point_adjacency, point_adjacency_offsets, num_edges, bbox, volume, centroid,
                             bounded, site_moment, central_moment);
}

}  // extern "C"
