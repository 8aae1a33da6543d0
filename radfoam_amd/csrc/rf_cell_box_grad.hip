// rf_cell_box_grad.hip -- point gradients of the volumes and centroids of the Voronoi cells clipped to an axis-aligned
// box ("Point gradients of the cells in a box").  The mathematics: rf_clip_box_grad.hpp; the plane list and
// its tie rule: rf_clip_box.hpp; the moments and the per-face arithmetic: rf_clip_grad.hpp, all in double.  The wave
// scheme, its LDS layout and the hand-off through redo[cell]: rf_cell_wave.hpp.
//
//   cell_box_grad_kernel       one lane per ROW face; the six walls are staged behind the row by lanes 0..5.  The lane
//                              clips its face again by the whole list in list order, takes the polygon's moments, reads
//                              its neighbour's gV, gC, V, c and nonempty and forms its 3-vector; three wave sums, and
//                              lane 0 writes the row.  A face with an empty cell on either side is passed over.  The
//                              walls do not move: they are clip planes only and take no lanes, so rows of up to 64 faces
//                              (lists of up to 70 planes) stay here.
//   cell_box_grad_redo_kernel  the cells handed on, by rf::clip::cell_box_grad_serial.
//
// Row a is a gather over a's own adjacency row: every output element is written exactly once by a plain store, there are
// no atomics, and the result is bit-reproducible.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/radfoam_hip_box_grad.h"
#include "rf_cell_wave.hpp"
#include "rf_clip_box_grad.hpp"

namespace rf {
namespace cell_box_grad {

__global__ __launch_bounds__(64) void cell_box_grad_kernel(
    const float *__restrict__ points, uint32_t num_points, const uint32_t *__restrict__ adj,
    const uint32_t *__restrict__ offsets, uint32_t num_edges, const float *__restrict__ bbox, double lo_x, double lo_y,
    double lo_z, double hi_x, double hi_y, double hi_z, const double *__restrict__ volume,
    const double *__restrict__ centroid, const uint8_t *__restrict__ nonempty, const double *__restrict__ grad_volume,
    const double *__restrict__ grad_centroid, double *__restrict__ grad_points, uint8_t *__restrict__ redo) {
    __shared__ double s_plane[4][kWave + clip::kWalls];   // d (x, y, z), h of the list: the row, then the walls
    __shared__ double s_s[2 * kLaneCap][kWave];           // polygons: buffer 0 at vertex rows [0, kLaneCap), buffer 1 after
    __shared__ double s_t[2 * kLaneCap][kWave];
    const clip::Box box = {lo_x, lo_y, lo_z, hi_x, hi_y, hi_z};
    const uint32_t a = blockIdx.x, lane = threadIdx.x;
    const uint32_t begin = offsets[a], end = offsets[a + 1];
    if (begin > end || end > num_edges || end - begin > kWave) return hand_on(redo, a, lane);   // wave-uniform
    const uint32_t degree = end - begin, count = degree + clip::kWalls;
    if (degree == 0) {   // no neighbours: the cell is the whole box wherever the site is
        if (lane == 0) {
            grad_points[3 * (size_t)a] = grad_points[3 * (size_t)a + 1] = grad_points[3 * (size_t)a + 2] = 0.0;
            keep(redo, a);
        }
        return;
    }
    const CellLane f = load_neighbour(points, num_points, adj, a, begin, degree, lane);
    if (f.have) store_plane(s_plane, lane, f.dx, f.dy, f.dz, f.h);
    stage_walls(points, a, box, degree, lane, s_plane);
    if (sync_any_bad(f.bad)) return hand_on(redo, a, lane);
    const double R = clip::half_side_box(bbox, box);
    bool overflow = false;
    double gx = 0.0, gy = 0.0, gz = 0.0;
    if (f.have && nonempty[a] && nonempty[f.q]) {   // a face with an empty cell on either side carries no term
        const clip::Frame frame = clip::list_frame(false, f.dx, f.dy, f.dz, f.h);
        double *s = &s_s[0][lane], *t = &s_t[0][lane];
        clip::init_square(s, t, kWave, R);
        uint32_t m = 4, cur = 0;
        for (uint32_t j = 0; j < count && m != 0; ++j) {   // by the other planes of the list, in list order
            if (j == lane) continue;
            if (!clip::clip_by_list_plane(frame, f.dx, f.dy, f.dz, j < lane, s_plane[0][j], s_plane[1][j], s_plane[2][j],
                                          s_plane[3][j], s, t, kWave, kLaneCap, m, cur)) {
                overflow = true;
                break;
            }
        }
        if (!overflow) {   // q < num_points: no lane of this wave is bad
            const clip::Moments mo = clip::moments(s + cur * kLaneCap * kWave, t + cur * kLaneCap * kWave, kWave, m, R);
            const clip::CellTerm ca = clip::cell_term(points, a, a, volume, centroid, nonempty, grad_volume,
                                                      grad_centroid);
            const clip::CellTerm cb = clip::cell_term(points, a, f.q, volume, centroid, nonempty, grad_volume,
                                                      grad_centroid);
            clip::add_face_grad(frame, mo, ca, cb, gx, gy, gz);
        }
    }
    if (__any(overflow)) return hand_on(redo, a, lane);
    gx = wave_sum(gx), gy = wave_sum(gy), gz = wave_sum(gz);
    if (lane == 0) {
        grad_points[3 * (size_t)a] = gx, grad_points[3 * (size_t)a + 1] = gy, grad_points[3 * (size_t)a + 2] = gz;
        keep(redo, a);
    }
}

__global__ __launch_bounds__(64) void cell_box_grad_redo_kernel(
    const float *__restrict__ points, uint32_t num_points, const uint32_t *__restrict__ adj,
    const uint32_t *__restrict__ offsets, uint32_t num_edges, const float *__restrict__ bbox, double lo_x, double lo_y,
    double lo_z, double hi_x, double hi_y, double hi_z, const double *__restrict__ volume,
    const double *__restrict__ centroid, const uint8_t *__restrict__ nonempty, const double *__restrict__ grad_volume,
    const double *__restrict__ grad_centroid, double *__restrict__ grad_points, const uint8_t *__restrict__ redo,
    uint8_t *__restrict__ cell_status) {
    __shared__ double s_s[2 * kWaveCap], s_t[2 * kWaveCap];
    const clip::Box box = {lo_x, lo_y, lo_z, hi_x, hi_y, hi_z};
    unsigned long long todo = redo_todo(num_points, redo, cell_status);
    if (threadIdx.x != 0) return;
    const double R = clip::half_side_box(bbox, box);
    while (todo) {
        const uint32_t a = redo_next(todo);
        cell_status[a] = (uint8_t)clip::cell_box_grad_serial(points, num_points, adj, offsets, num_edges, a, box, R, s_s,
                                                             s_t, kWaveCap, volume, centroid, nonempty, grad_volume,
                                                             grad_centroid, grad_points);
    }
}

}  // namespace cell_box_grad
}  // namespace rf

using namespace rf;

extern "C" {

size_t rf_cell_box_grad_workspace_bytes(uint32_t num_points) { return redo_bytes(num_points); }

int rf_cell_box_grad(const float *points, uint32_t num_points, const uint32_t *point_adjacency,
                     const uint32_t *point_adjacency_offsets, uint32_t num_edges, const float *bbox, double lo_x,
                     double lo_y, double lo_z, double hi_x, double hi_y, double hi_z, const double *volume,
                     const double *centroid, const uint8_t *nonempty, const double *grad_volume,
                     const double *grad_centroid, double *grad_points, uint8_t *cell_status, void *workspace,
                     size_t workspace_bytes, void *stream) {
    g_err[0] = 0;
    if (num_points == 0) return RF_OK;
    if (!points || !point_adjacency_offsets || !bbox || !volume || !centroid || !nonempty || !grad_points ||
        !cell_status || (num_edges && !point_adjacency))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_cell_box_grad: null pointer");
    if (int rc = check_box("rf_cell_box_grad", lo_x, lo_y, lo_z, hi_x, hi_y, hi_z)) return rc;
    if (!workspace || workspace_bytes < rf_cell_box_grad_workspace_bytes(num_points))
        return fail(RF_ERR_WORKSPACE, "rf_cell_box_grad: workspace missing or too small");
    return launch_cell_waves("rf_cell_box_grad", stream, num_points, workspace, cell_status,
                             cell_box_grad::cell_box_grad_kernel, cell_box_grad::cell_box_grad_redo_kernel, points,
                             num_points, point_adjacency, point_adjacency_offsets, num_edges, bbox, lo_x, lo_y, lo_z,
                             hi_x, hi_y, hi_z, volume, centroid, nonempty, grad_volume, grad_centroid, grad_points);
}

}  // extern "C"
