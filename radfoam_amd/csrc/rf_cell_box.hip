// rf_cell_box.hip -- Voronoi cells clipped to an axis-aligned box: volume, centroid, the part of every face inside the
// box and the part of every wall that bounds the cell ("Cells clipped to a box").  The definition, the plane
// list, the wall frames and the tie rule of coincident planes: rf_clip_box.hpp, all in double.  The wave scheme, its LDS
// layout and the hand-off through redo[cell]: rf_cell_wave.hpp.
//
//   cell_box_kernel       one lane per face of the cell's list: the row's lanes first, then six wall lanes; each lane
//                         clips its face's square by the other planes in list order.  Volume and first moments are wave
//                         reductions.  Lists of up to 64 planes (rows of up to 58).
//   cell_box_redo_kernel  the cells handed on, by rf::clip::cell_box_serial.
//
// Every output element is written exactly once, by plain stores; no atomics: the result is bit-reproducible.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/radfoam_hip_box.h"
#include "rf_cell_wave.hpp"

namespace rf {
namespace cell_box {

__global__ __launch_bounds__(64) void cell_box_kernel(
    const float *__restrict__ points, uint32_t num_points, const uint32_t *__restrict__ adj,
    const uint32_t *__restrict__ offsets, uint32_t num_edges, const float *__restrict__ bbox, double lo_x, double lo_y,
    double lo_z, double hi_x, double hi_y, double hi_z,
    double *__restrict__ volume, double *__restrict__ centroid, uint8_t *__restrict__ nonempty,
    double *__restrict__ face_area, uint32_t *__restrict__ face_vertices, double *__restrict__ wall_area,
    uint32_t *__restrict__ wall_vertices, uint8_t *__restrict__ redo) {
    __shared__ double s_plane[4][kWave];             // d (x, y, z), h of the list
    __shared__ double s_s[2 * kLaneCap][kWave];      // polygons: buffer 0 at vertex rows [0, kLaneCap), buffer 1 after
    __shared__ double s_t[2 * kLaneCap][kWave];
    const clip::Box box = {lo_x, lo_y, lo_z, hi_x, hi_y, hi_z};
    const uint32_t a = blockIdx.x, lane = threadIdx.x;
    const uint32_t begin = offsets[a], end = offsets[a + 1];
    if (begin > end || end > num_edges || end - begin > kWave - clip::kWalls)   // wave-uniform
        return hand_on(redo, a, lane);
    const uint32_t degree = end - begin, count = degree + clip::kWalls;
    if (degree == 0) {   // no neighbours: the whole box
        if (lane == 0) {
            clip::whole_box(box, a, volume, centroid, nonempty, wall_area, wall_vertices);
            keep(redo, a);
        }
        return;
    }
    // the staging with the walls as lanes, spelled out: through a shared helper the wall test moves in the kernel's code.
    // The load and the bad test are load_neighbour's of rf_cell_wave.hpp, line for line: keep the two in step.
    const bool row = lane < degree, wall = !row && lane < count;
    uint32_t q = row ? adj[begin + lane] : 0u;
    bool bad = row && (q >= num_points || q == a);
    if (!row || bad) q = a;
    double dx, dy, dz, h;
    clip::neighbour(points, a, q, dx, dy, dz, h);
    bad = bad || (row && !(h > 0.0));
    if (wall) clip::wall_plane(points, a, box, lane - degree, dx, dy, dz, h);
    s_plane[0][lane] = dx, s_plane[1][lane] = dy, s_plane[2][lane] = dz, s_plane[3][lane] = h;
    if (sync_any_bad(bad)) return hand_on(redo, a, lane);
    const double R = clip::half_side_box(bbox, box);
    bool overflow = false;
    double area = 0.0;
    clip::CellSums sums = {0.0, 0.0, 0.0, 0.0, false};
    uint32_t m = 0;
    if (row || wall) {
        const clip::Frame frame = clip::list_frame(wall, dx, dy, dz, h);
        double *s = &s_s[0][lane], *t = &s_t[0][lane];
        clip::init_square(s, t, kWave, R);
        m = 4;
        uint32_t cur = 0;
        for (uint32_t j = 0; j < count && m != 0; ++j) {   // by the other planes of the list, in list order
            if (j == lane) continue;
            if (!clip::clip_by_list_plane(frame, dx, dy, dz, j < lane, s_plane[0][j], s_plane[1][j], s_plane[2][j],
                                          s_plane[3][j], s, t, kWave, kLaneCap, m, cur)) {
                overflow = true;
                break;
            }
        }
        if (!overflow) {
            double cs, ct;
            bool square;   // cannot be: the walls are in the list
            clip::measure(s + cur * kLaneCap * kWave, t + cur * kLaneCap * kWave, kWave, m, R, area, cs, ct, square);
            clip::add_face_box(sums, frame, wall, h, area, cs, ct);
        }
    }
    if (__any(overflow)) return hand_on(redo, a, lane);
    if (row) {
        face_area[begin + lane] = area;
        face_vertices[begin + lane] = m;
    } else if (wall) {
        wall_area[clip::kWalls * (size_t)a + (lane - degree)] = area;
        wall_vertices[clip::kWalls * (size_t)a + (lane - degree)] = m;
    }
    sums.volume = wave_sum(sums.volume);
    sums.mx = wave_sum(sums.mx), sums.my = wave_sum(sums.my), sums.mz = wave_sum(sums.mz);
    if (lane == 0) {
        clip::write_cell_box(points, a, sums, volume, centroid, nonempty);
        keep(redo, a);
    }
}

__global__ __launch_bounds__(64) void cell_box_redo_kernel(
    const float *__restrict__ points, uint32_t num_points, const uint32_t *__restrict__ adj,
    const uint32_t *__restrict__ offsets, uint32_t num_edges, const float *__restrict__ bbox, double lo_x, double lo_y,
    double lo_z, double hi_x, double hi_y, double hi_z,
    double *__restrict__ volume, double *__restrict__ centroid, uint8_t *__restrict__ nonempty,
    double *__restrict__ face_area, uint32_t *__restrict__ face_vertices, double *__restrict__ wall_area,
    uint32_t *__restrict__ wall_vertices, const uint8_t *__restrict__ redo, uint8_t *__restrict__ cell_status) {
    __shared__ double s_s[2 * kWaveCap], s_t[2 * kWaveCap];
    const clip::Box box = {lo_x, lo_y, lo_z, hi_x, hi_y, hi_z};
    unsigned long long todo = redo_todo(num_points, redo, cell_status);
    if (threadIdx.x != 0) return;
    const double R = clip::half_side_box(bbox, box);
    while (todo) {
        const uint32_t a = redo_next(todo);
        cell_status[a] = (uint8_t)clip::cell_box_serial(points, num_points, adj, offsets, num_edges, a, box, R, s_s, s_t,
                                                        kWaveCap, volume, centroid, nonempty, face_area, face_vertices,
                                                        wall_area, wall_vertices);
    }
}

}  // namespace cell_box
}  // namespace rf

using namespace rf;

extern "C" {

size_t rf_cell_box_workspace_bytes(uint32_t num_points) { return redo_bytes(num_points); }

int rf_cell_box(const float *points, uint32_t num_points, const uint32_t *point_adjacency,
                const uint32_t *point_adjacency_offsets, uint32_t num_edges, const float *bbox, double lo_x, double lo_y,
                double lo_z, double hi_x, double hi_y, double hi_z, double *volume, double *centroid, uint8_t *nonempty,
                double *face_area, uint32_t *face_vertices, double *wall_area, uint32_t *wall_vertices,
                uint8_t *cell_status, void *workspace, size_t workspace_bytes, void *stream) {
    g_err[0] = 0;
    if (num_points == 0) return RF_OK;
    if (!points || !point_adjacency_offsets || !bbox || !volume || !centroid || !nonempty || !wall_area ||
        !wall_vertices || !cell_status || (num_edges && (!point_adjacency || !face_area || !face_vertices)))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_cell_box: null pointer");
    if (int rc = check_box("rf_cell_box", lo_x, lo_y, lo_z, hi_x, hi_y, hi_z)) return rc;
    if (!workspace || workspace_bytes < rf_cell_box_workspace_bytes(num_points))
        return fail(RF_ERR_WORKSPACE, "rf_cell_box: workspace missing or too small");
    return launch_cell_waves("rf_cell_box", stream, num_points, workspace, cell_status, cell_box::cell_box_kernel,
                             cell_box::cell_box_redo_kernel, points, num_points, point_adjacency,
                             point_adjacency_offsets, num_edges, bbox, lo_x, lo_y, lo_z, hi_x, hi_y, hi_z, volume,
                             centroid, nonempty, face_area, face_vertices, wall_area, wall_vertices);
}

}  // extern "C"
