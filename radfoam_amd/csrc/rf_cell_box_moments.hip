// rf_cell_box_moments.hip -- the second moments of the Voronoi cells clipped to an axis-aligned box: int y y^T dy about
// the site and about the centroid ("Second moments of the cells clipped to a box").  The definition, the signed
// pyramids and the closed form of the whole box: rf_clip_box_moments.hpp; the plane list, the wall frames and the tie rule
// of coincident planes: rf_clip_box.hpp, all in double.  The wave scheme, its LDS layout and the hand-off through
// redo[cell]: rf_cell_wave.hpp.
//
//   cell_box_moments_kernel       one lane per plane of the cell's list, as cell_box_kernel: the row's lanes first, then
//                                 six wall lanes.  The lane clips its face again (the forward keeps no moments), forms
//                                 the polygon's moments and weights them with the signed height of its plane; six wave
//                                 sums, and lane 0 forms the central moment and writes the twelve numbers.  Lists of up to
//                                 64 planes (rows of up to 58).
//   cell_box_moments_redo_kernel  the cells handed on, by rf::clip::cell_box_moments_serial.
//
// Cell a is a gather over a's own list: every output element is written exactly once by a plain store, there are no
// atomics, and the result is bit-reproducible.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/radfoam_hip_box_moments.h"
#include "rf_cell_wave.hpp"
#include "rf_clip_box_moments.hpp"

namespace rf {
namespace cell_box_moments {

__global__ __launch_bounds__(64) void cell_box_moments_kernel(
    const float *__restrict__ points, uint32_t num_points, const uint32_t *__restrict__ adj,
    const uint32_t *__restrict__ offsets, uint32_t num_edges, const float *__restrict__ bbox, double lo_x, double lo_y,
    double lo_z, double hi_x, double hi_y, double hi_z, const double *__restrict__ volume,
    const double *__restrict__ centroid, const uint8_t *__restrict__ nonempty, double *__restrict__ site_moment,
    double *__restrict__ central_moment, uint8_t *__restrict__ redo) {
    __shared__ double s_plane[4][kWave];             // d (x, y, z), h of the list
    __shared__ double s_s[2 * kLaneCap][kWave];      // polygons: buffer 0 at vertex rows [0, kLaneCap), buffer 1 after
    __shared__ double s_t[2 * kLaneCap][kWave];
    const clip::Box box = {lo_x, lo_y, lo_z, hi_x, hi_y, hi_z};
    const uint32_t a = blockIdx.x, lane = threadIdx.x;
    const uint32_t begin = offsets[a], end = offsets[a + 1];
    if (begin > end || end > num_edges || end - begin > kWave - clip::kWalls)   // wave-uniform
        return hand_on(redo, a, lane);
    const uint32_t degree = end - begin, count = degree + clip::kWalls;
    if (degree == 0) {   // no neighbours: the whole box, in closed form
        if (lane == 0) {
            clip::whole_box_moments(points, a, box, site_moment, central_moment);
            keep(redo, a);
        }
        return;
    }
    // the staging with the walls as lanes, spelled out as in cell_box_kernel.  The load and the bad test are
    // load_neighbour's of rf_cell_wave.hpp, line for line: keep the two in step.
    const bool row = lane < degree, wall = !row && lane < count;
    uint32_t q = row ? adj[begin + lane] : 0u;
    bool bad = row && (q >= num_points || q == a);
    if (!row || bad) q = a;
    double dx, dy, dz, h;
    clip::neighbour(points, a, q, dx, dy, dz, h);
    bad = bad || (row && !(h > 0.0));
    if (wall) clip::wall_plane(points, a, box, lane - degree, dx, dy, dz, h);   // a choice among values, not members
    s_plane[0][lane] = dx, s_plane[1][lane] = dy, s_plane[2][lane] = dz, s_plane[3][lane] = h;
    if (sync_any_bad(bad)) return hand_on(redo, a, lane);
    const double R = clip::half_side_box(bbox, box);
    bool overflow = false;
    clip::MomentSums sums = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, false};
    if (row || wall) {
        const clip::Frame frame = clip::list_frame(wall, dx, dy, dz, h);
        double *s = &s_s[0][lane], *t = &s_t[0][lane];
        clip::init_square(s, t, kWave, R);
        uint32_t m = 4, cur = 0;
        for (uint32_t j = 0; j < count && m != 0; ++j) {   // by the other planes of the list, in list order
            if (j == lane) continue;
            if (!clip::clip_by_list_plane(frame, dx, dy, dz, j < lane, s_plane[0][j], s_plane[1][j], s_plane[2][j],
                                          s_plane[3][j], s, t, kWave, kLaneCap, m, cur)) {
                overflow = true;
                break;
            }
        }
        if (!overflow)
            clip::add_face_moment_box(sums, frame, wall, h,
                                      clip::moments(s + cur * kLaneCap * kWave, t + cur * kLaneCap * kWave, kWave, m, R));
    }
    if (__any(overflow)) return hand_on(redo, a, lane);
    sums.unbounded = __any(sums.unbounded);   // cannot be: the walls are in the list; NaN rather than wrong
    sums.xx = wave_sum(sums.xx), sums.yy = wave_sum(sums.yy), sums.zz = wave_sum(sums.zz);
    sums.xy = wave_sum(sums.xy), sums.xz = wave_sum(sums.xz), sums.yz = wave_sum(sums.yz);
    if (lane == 0) {
        clip::write_moments_box(points, a, sums, volume, centroid, nonempty, site_moment, central_moment);
        keep(redo, a);
    }
}

__global__ __launch_bounds__(64) void cell_box_moments_redo_kernel(
    const float *__restrict__ points, uint32_t num_points, const uint32_t *__restrict__ adj,
    const uint32_t *__restrict__ offsets, uint32_t num_edges, const float *__restrict__ bbox, double lo_x, double lo_y,
    double lo_z, double hi_x, double hi_y, double hi_z, const double *__restrict__ volume,
    const double *__restrict__ centroid, const uint8_t *__restrict__ nonempty, double *__restrict__ site_moment,
    double *__restrict__ central_moment, const uint8_t *__restrict__ redo, uint8_t *__restrict__ cell_status) {
    __shared__ double s_s[2 * kWaveCap], s_t[2 * kWaveCap];
    const clip::Box box = {lo_x, lo_y, lo_z, hi_x, hi_y, hi_z};
    unsigned long long todo = redo_todo(num_points, redo, cell_status);
    if (threadIdx.x != 0) return;
    const double R = clip::half_side_box(bbox, box);
    while (todo) {
        const uint32_t a = redo_next(todo);
        cell_status[a] = (uint8_t)clip::cell_box_moments_serial(points, num_points, adj, offsets, num_edges, a, box, R, s_s,
                                                                s_t, kWaveCap, volume, centroid, nonempty, site_moment,
                                                                central_moment);
    }
}

}  // namespace cell_box_moments
}  // namespace rf

using namespace rf;

extern "C" {

size_t rf_cell_box_moments_workspace_bytes(uint32_t num_points) { return redo_bytes(num_points); }

int rf_cell_box_moments(const float *points, uint32_t num_points, const uint32_t *point_adjacency,
                        const uint32_t *point_adjacency_offsets, uint32_t num_edges, const float *bbox, double lo_x,
                        double lo_y, double lo_z, double hi_x, double hi_y, double hi_z, const double *volume,
                        const double *centroid, const uint8_t *nonempty, double *site_moment, double *central_moment,
                        uint8_t *cell_status, void *workspace, size_t workspace_bytes, void *stream) {
    g_err[0] = 0;
    if (num_points == 0) return RF_OK;
    if (!points || !point_adjacency_offsets || !bbox || !volume || !centroid || !nonempty || !site_moment ||
        !central_moment || !cell_status || (num_edges && !point_adjacency))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_cell_box_moments: null pointer");
    if (int rc = check_box("rf_cell_box_moments", lo_x, lo_y, lo_z, hi_x, hi_y, hi_z)) return rc;
    if (!workspace || workspace_bytes < rf_cell_box_moments_workspace_bytes(num_points))
        return fail(RF_ERR_WORKSPACE, "rf_cell_box_moments: workspace missing or too small");
    return launch_cell_waves("rf_cell_box_moments", stream, num_points, workspace, cell_status,
                             cell_box_moments::cell_box_moments_kernel, cell_box_moments::cell_box_moments_redo_kernel,
                             points, num_points, point_adjacency, point_adjacency_offsets, num_edges, bbox, lo_x, lo_y,
                             lo_z, hi_x, hi_y, hi_z, volume, centroid, nonempty, site_moment, central_moment);
}

}  // extern "C"
