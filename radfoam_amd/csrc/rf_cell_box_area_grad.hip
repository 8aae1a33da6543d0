// rf_cell_box_area_grad.hip -- point gradients of the face and wall areas of the Voronoi cells clipped to an axis-aligned
// box ("Point gradients of the face and wall areas in a box").  The mathematics, the labelled list-plane step
// and the two edge terms: rf_clip_box_area_grad.hpp; the plane list and its tie rule: rf_clip_box.hpp; the effective
// weight, the row search and the Voronoi-edge term: rf_clip_area_grad.hpp, all in double.  The wave scheme, its LDS layout
// and the hand-off through redo[cell]: rf_cell_wave.hpp.
//
//   box_face_weight_kernel         the pre-pass, one wave per cell and one lane per slot: the effective weight G of every
//                                  slot (its own upstream plus its mate's, found by a search of the neighbour's row, each
//                                  masked by its own boxed face_area; zero for a null upstream) into an f64[E] workspace
//                                  array, by plain stores.
//   cell_box_area_grad_kernel      one lane per ROW face, as face_area_grad_kernel and cell_box_grad_kernel: beside the
//                                  list's planes (the six walls behind the row by lanes 0..5), the row's sites and weights
//                                  and the cell's six wall weights are staged in LDS, and each lane's polygon has one byte
//                                  of label per vertex beside it.  The lane clips its face again by the whole list with
//                                  labels (its own loop: the labelled step) and sums its edges' terms; three wave sums,
//                                  and lane 0 writes the row.  Rows of up to 64 faces (lists of up to 70 planes).
//   cell_box_area_grad_redo_kernel the cells handed on, by rf::clip::cell_box_area_grad_serial.
//
// Row a is a gather over a's own adjacency row, one look-up per Voronoi edge in a neighbour's row and one read of the
// neighbour's wall weight per wall edge: every output element is written exactly once by a plain store, there are no
// atomics, and the result is bit-reproducible.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/radfoam_hip_box_area_grad.h"
#include "rf_cell_wave.hpp"
#include "rf_clip_box_area_grad.hpp"

namespace rf {
namespace cell_box_area_grad {

constexpr uint32_t kWeightWaves = 4;
constexpr uint32_t kList = kWave + clip::kWalls;

__global__ __launch_bounds__(kWave *kWeightWaves) void box_face_weight_kernel(
    uint32_t num_points, const uint32_t *__restrict__ adj, const uint32_t *__restrict__ offsets, uint32_t num_edges,
    const double *__restrict__ face_area, const double *__restrict__ grad_face_area, double *__restrict__ weight) {
    const uint32_t a = blockIdx.x * kWeightWaves + threadIdx.x / kWave, lane = threadIdx.x % kWave;
    if (a >= num_points) return;
    const uint32_t begin = offsets[a], end = offsets[a + 1];
    if (begin > end || end > num_edges) return;   // a malformed row: the main kernels report it
    for (uint32_t k = begin + lane; k < end; k += kWave)
        weight[k] = clip::effective_weight_box(adj, offsets, num_points, num_edges, face_area, grad_face_area, a, k);
}

__global__ __launch_bounds__(64) void cell_box_area_grad_kernel(
    const float *__restrict__ points, uint32_t num_points, const uint32_t *__restrict__ adj,
    const uint32_t *__restrict__ offsets, uint32_t num_edges, const float *__restrict__ bbox, double lo_x, double lo_y,
    double lo_z, double hi_x, double hi_y, double hi_z, const uint8_t *__restrict__ nonempty,
    const double *__restrict__ face_area, const double *__restrict__ wall_area, const double *__restrict__ weight,
    const double *__restrict__ grad_wall_area, double *__restrict__ grad_points, uint8_t *__restrict__ redo) {
    __shared__ double s_plane[4][kList];             // d (x, y, z), h of the list: the row, then the walls
    __shared__ double s_g[kWave];                    // the row's effective weights
    __shared__ double s_gw[clip::kWalls];            // the cell's masked wall weights
    __shared__ uint32_t s_q[kWave];                  // the row's sites
    __shared__ double s_s[2 * kLaneCap][kWave];      // polygons: buffer 0 at vertex rows [0, kLaneCap), buffer 1 after
    __shared__ double s_t[2 * kLaneCap][kWave];
    __shared__ uint8_t s_l[2 * kLaneCap][kWave];     // labels, beside the vertices
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
    if (lane < clip::kWalls) s_gw[lane] = clip::wall_weight(wall_area, grad_wall_area, a, lane);
    s_q[lane] = f.q;
    s_g[lane] = f.have ? weight[begin + lane] : 0.0;
    if (sync_any_bad(f.bad)) return hand_on(redo, a, lane);
    const double R = clip::half_side_box(bbox, box);
    bool overflow = false;
    double gx = 0.0, gy = 0.0, gz = 0.0;
    if (f.have && nonempty[a]) {   // an empty cell stays empty around here: a zero row
        const clip::Frame frame = clip::list_frame(false, f.dx, f.dy, f.dz, f.h);
        double *s = &s_s[0][lane], *t = &s_t[0][lane];
        uint8_t *l = &s_l[0][lane];
        clip::init_square(s, t, kWave, R);
        clip::init_square_labels(l, kWave);
        uint32_t m = 4, cur = 0;
        for (uint32_t j = 0; j < count && m != 0; ++j) {
            if (j == lane) continue;
            if (!clip::clip_by_list_plane_labelled(frame, f.dx, f.dy, f.dz, j < lane, s_plane[0][j], s_plane[1][j],
                                                   s_plane[2][j], s_plane[3][j], s, t, l, kWave, kLaneCap, m, cur,
                                                   (uint8_t)j)) {
                overflow = true;
                break;
            }
        }
        if (!overflow && m != 0) {   // q < num_points: no lane of this wave is bad
            const uint32_t at = cur * kLaneCap * kWave, free_at = (cur ^ 1u) * kLaneCap * kWave;
            const RowFromLds<kList> row = {&s_plane[0][0], s_q};
            clip::add_polygon_terms_box(row, degree, lane, frame, f.dx, f.dy, f.dz, s + at, t + at, l + at, s + free_at,
                                        t + free_at, kWave, m, adj, offsets, num_edges, weight, f.q, s_g,
                                        face_area + begin, s_gw, wall_area, grad_wall_area, gx, gy, gz);
        }
    }
    if (__any(overflow)) return hand_on(redo, a, lane);
    gx = wave_sum(gx), gy = wave_sum(gy), gz = wave_sum(gz);
    if (lane == 0) {
        grad_points[3 * (size_t)a] = gx, grad_points[3 * (size_t)a + 1] = gy, grad_points[3 * (size_t)a + 2] = gz;
        keep(redo, a);
    }
}

__global__ __launch_bounds__(64) void cell_box_area_grad_redo_kernel(
    const float *__restrict__ points, uint32_t num_points, const uint32_t *__restrict__ adj,
    const uint32_t *__restrict__ offsets, uint32_t num_edges, const float *__restrict__ bbox, double lo_x, double lo_y,
    double lo_z, double hi_x, double hi_y, double hi_z, const uint8_t *__restrict__ nonempty,
    const double *__restrict__ face_area, const double *__restrict__ wall_area, const double *__restrict__ weight,
    const double *__restrict__ grad_wall_area, double *__restrict__ grad_points, const uint8_t *__restrict__ redo,
    uint8_t *__restrict__ cell_status) {
    __shared__ double s_s[2 * kWaveCap], s_t[2 * kWaveCap];
    __shared__ uint32_t s_l[2 * kWaveCap];
    const clip::Box box = {lo_x, lo_y, lo_z, hi_x, hi_y, hi_z};
    unsigned long long todo = redo_todo(num_points, redo, cell_status);
    if (threadIdx.x != 0) return;
    const double R = clip::half_side_box(bbox, box);
    while (todo) {
        const uint32_t a = redo_next(todo);
        cell_status[a] = (uint8_t)clip::cell_box_area_grad_serial(points, num_points, adj, offsets, num_edges, a, box, R,
                                                                  s_s, s_t, s_l, kWaveCap, nonempty, face_area, wall_area,
                                                                  weight, grad_wall_area, grad_points);
    }
}

}  // namespace cell_box_area_grad
}  // namespace rf

using namespace rf;

extern "C" {

size_t rf_cell_box_area_grad_workspace_bytes(uint32_t num_points, uint32_t num_edges) {
    return redo_bytes(num_points) + sizeof(double) * (size_t)num_edges;
}

int rf_cell_box_area_grad(const float *points, uint32_t num_points, const uint32_t *point_adjacency,
                          const uint32_t *point_adjacency_offsets, uint32_t num_edges, const float *bbox, double lo_x,
                          double lo_y, double lo_z, double hi_x, double hi_y, double hi_z, const double *volume,
                          const double *centroid, const uint8_t *nonempty, const double *face_area,
                          const double *wall_area, const double *grad_face_area, const double *grad_wall_area,
                          double *grad_points, uint8_t *cell_status, void *workspace, size_t workspace_bytes,
                          void *stream) {
    g_err[0] = 0;
    if (num_points == 0) return RF_OK;
    if (!points || !point_adjacency_offsets || !bbox || !volume || !centroid || !nonempty || !wall_area || !grad_points ||
        !cell_status || (num_edges && (!point_adjacency || !face_area)))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_cell_box_area_grad: null pointer");
    if (int rc = check_box("rf_cell_box_area_grad", lo_x, lo_y, lo_z, hi_x, hi_y, hi_z)) return rc;
    if (!workspace || workspace_bytes < rf_cell_box_area_grad_workspace_bytes(num_points, num_edges))
        return fail(RF_ERR_WORKSPACE, "rf_cell_box_area_grad: workspace missing or too small");
    double *weight = reinterpret_cast<double *>(static_cast<uint8_t *>(workspace) + redo_bytes(num_points));
    if (num_edges)
        hipLaunchKernelGGL(cell_box_area_grad::box_face_weight_kernel,
                           dim3((num_points + cell_box_area_grad::kWeightWaves - 1u) / cell_box_area_grad::kWeightWaves),
                           dim3(kWave * cell_box_area_grad::kWeightWaves), 0, static_cast<hipStream_t>(stream),
                           num_points, point_adjacency, point_adjacency_offsets, num_edges, face_area, grad_face_area,
                           weight);
    return launch_cell_waves("rf_cell_box_area_grad", stream, num_points, workspace, cell_status,
                             cell_box_area_grad::cell_box_area_grad_kernel,
                             cell_box_area_grad::cell_box_area_grad_redo_kernel, points, num_points, point_adjacency,
                             point_adjacency_offsets, num_edges, bbox, lo_x, lo_y, lo_z, hi_x, hi_y, hi_z, nonempty,
                             face_area, wall_area, weight, grad_wall_area, grad_points);
}

}  // extern "C"
