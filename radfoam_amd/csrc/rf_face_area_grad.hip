// rf_face_area_grad.hip -- point gradients of the Voronoi face areas ("Point gradients of the face areas").
// The mathematics, the labelled clipping and the per-edge arithmetic: rf_clip_area_grad.hpp, all in double.  The wave
// scheme, its LDS layout and the hand-off through redo[cell]: rf_cell_wave.hpp.
//
//   face_weight_kernel          the pre-pass, one wave per cell and one lane per slot: the effective weight G of every
//                               slot (its own upstream plus its mate's, found by a search of the neighbour's row, each
//                               masked by its own face_area) into an f64[E] workspace array, by plain stores.
//   face_area_grad_kernel       beside the planes, the row's neighbour indices and weights are staged in LDS, and each
//                               lane's polygon has its labels beside it in the same layout.  The lane clips its face
//                               again with labels (its own loop: the labelled step) and sums its edges' terms: per edge
//                               a search of the row of b for G_bc of its label, then one pass over the staged planes for
//                               further sites cocircular around an edge (none, off degenerate clouds), the sums per edge
//                               kept in the polygon buffer the clipping left free; a triangle counts in the lane of its
//                               larger face.  Three wave sums, and lane 0 writes the row.  Rows of up to 64 faces.
//   face_area_grad_redo_kernel  the cells handed on, by rf::clip::face_area_grad_serial.
//
// Row a is a gather over a's own adjacency row and one look-up per edge in a neighbour's: every output element is
// written exactly once by a plain store, there are no atomics, and the result is bit-reproducible.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/radfoam_hip_face_area_grad.h"
#include "rf_cell_wave.hpp"
#include "rf_clip_area_grad.hpp"

namespace rf {
namespace face_area_grad {

constexpr uint32_t kWeightWaves = 4;

__global__ __launch_bounds__(kWave *kWeightWaves) void face_weight_kernel(
    uint32_t num_points, const uint32_t *__restrict__ adj, const uint32_t *__restrict__ offsets, uint32_t num_edges,
    const double *__restrict__ face_area, const double *__restrict__ grad_face_area, double *__restrict__ weight) {
    const uint32_t a = blockIdx.x * kWeightWaves + threadIdx.x / kWave, lane = threadIdx.x % kWave;
    if (a >= num_points) return;
    const uint32_t begin = offsets[a], end = offsets[a + 1];
    if (begin > end || end > num_edges) return;   // a malformed row: the main kernels report it
    for (uint32_t k = begin + lane; k < end; k += kWave)
        weight[k] = clip::effective_weight(adj, offsets, num_points, num_edges, face_area, grad_face_area, a, k);
}

__global__ __launch_bounds__(64) void face_area_grad_kernel(
    const float *__restrict__ points, uint32_t num_points, const uint32_t *__restrict__ adj,
    const uint32_t *__restrict__ offsets, uint32_t num_edges, const float *__restrict__ bbox,
    const double *__restrict__ face_area, const double *__restrict__ weight, double *__restrict__ grad_points,
    uint8_t *__restrict__ redo) {
    __shared__ double s_plane[4][kWave];             // d_c (x, y, z), |d_c|^2 / 2 of the row
    __shared__ double s_g[kWave];                    // the row's effective weights
    __shared__ uint32_t s_q[kWave];                  // the row's sites
    __shared__ double s_s[2 * kLaneCap][kWave];      // polygons: buffer 0 at vertex rows [0, kLaneCap), buffer 1 after
    __shared__ double s_t[2 * kLaneCap][kWave];
    __shared__ uint8_t s_l[2 * kLaneCap][kWave];     // labels, beside the vertices
    const uint32_t a = blockIdx.x, lane = threadIdx.x;
    const uint32_t begin = offsets[a], end = offsets[a + 1];
    if (begin > end || end > num_edges || end - begin > kWave) return hand_on(redo, a, lane);   // wave-uniform
    const uint32_t degree = end - begin;
    if (degree == 0) {   // no neighbours: no face of this site's own row
        if (lane == 0) {
            grad_points[3 * (size_t)a] = grad_points[3 * (size_t)a + 1] = grad_points[3 * (size_t)a + 2] = 0.0;
            keep(redo, a);
        }
        return;
    }
    // the staging of stage_row, spelled out: through the helper this kernel's code comes out in another order.  The load
    // and the bad test are load_neighbour's of rf_cell_wave.hpp, line for line: keep the two in step.
    const bool have = lane < degree;
    uint32_t q = have ? adj[begin + lane] : 0u;
    bool bad = have && (q >= num_points || q == a);
    if (!have || bad) q = a;
    double dx, dy, dz, h;
    clip::neighbour(points, a, q, dx, dy, dz, h);
    bad = bad || (have && !(h > 0.0));
    s_plane[0][lane] = dx, s_plane[1][lane] = dy, s_plane[2][lane] = dz, s_plane[3][lane] = h;
    s_q[lane] = q;
    s_g[lane] = have ? weight[begin + lane] : 0.0;
    if (sync_any_bad(bad)) return hand_on(redo, a, lane);
    const double R = clip::area_grad_half_side(bbox);
    bool overflow = false;
    double gx = 0.0, gy = 0.0, gz = 0.0;
    if (have) {
        const clip::Frame frame = clip::make_frame(dx, dy, dz);
        double *s = &s_s[0][lane], *t = &s_t[0][lane];
        uint8_t *l = &s_l[0][lane];
        clip::init_square(s, t, kWave, R);
        clip::init_square_labels(l, kWave);
        uint32_t m = 4, cur = 0;
        for (uint32_t j = 0; j < degree && m != 0; ++j) {
            if (j == lane) continue;
            double A, B, C;
            clip::plane_in_frame(frame, s_plane[0][j], s_plane[1][j], s_plane[2][j], s_plane[3][j], A, B, C);
            const uint32_t in = cur * kLaneCap * kWave, out = (cur ^ 1u) * kLaneCap * kWave;
            if (!clip::clip_step_labelled(s + in, t + in, l + in, s + out, t + out, l + out, kWave, kLaneCap, m, A, B, C,
                                          (uint8_t)j)) {
                overflow = true;
                break;
            }
            cur ^= 1u;
        }
        if (!overflow && m != 0) {   // q < num_points: no lane of this wave is bad
            const uint32_t at = cur * kLaneCap * kWave, free_at = (cur ^ 1u) * kLaneCap * kWave;
            const RowFromLds<kWave> row = {&s_plane[0][0], s_q};
            clip::add_polygon_terms(row, degree, lane, frame, dx, dy, dz, R, s + at, t + at, l + at, s + free_at,
                                    t + free_at, kWave, m, adj, offsets, num_edges, weight, q, s_g, face_area + begin, gx,
                                    gy, gz);
        }
    }
    if (__any(overflow)) return hand_on(redo, a, lane);
    gx = wave_sum(gx), gy = wave_sum(gy), gz = wave_sum(gz);
    if (lane == 0) {
        grad_points[3 * (size_t)a] = gx, grad_points[3 * (size_t)a + 1] = gy, grad_points[3 * (size_t)a + 2] = gz;
        keep(redo, a);
    }
}

__global__ __launch_bounds__(64) void face_area_grad_redo_kernel(
    const float *__restrict__ points, uint32_t num_points, const uint32_t *__restrict__ adj,
    const uint32_t *__restrict__ offsets, uint32_t num_edges, const float *__restrict__ bbox,
    const double *__restrict__ face_area, const double *__restrict__ weight, double *__restrict__ grad_points,
    const uint8_t *__restrict__ redo, uint8_t *__restrict__ cell_status) {
    __shared__ double s_s[2 * kWaveCap], s_t[2 * kWaveCap];
    __shared__ uint32_t s_l[2 * kWaveCap];
    unsigned long long todo = redo_todo(num_points, redo, cell_status);
    if (threadIdx.x != 0) return;
    const double R = clip::area_grad_half_side(bbox);
    while (todo) {
        const uint32_t a = redo_next(todo);
        cell_status[a] = (uint8_t)clip::face_area_grad_serial(points, num_points, adj, offsets, num_edges, a, R, s_s, s_t,
                                                              s_l, kWaveCap, face_area, weight, grad_points);
    }
}

}  // namespace face_area_grad
}  // namespace rf

using namespace rf;

extern "C" {

size_t rf_face_area_grad_workspace_bytes(uint32_t num_points, uint32_t num_edges) {
    return redo_bytes(num_points) + sizeof(double) * (size_t)num_edges;
}

int rf_face_area_grad(const float *points, uint32_t num_points, const uint32_t *point_adjacency,
                      const uint32_t *point_adjacency_offsets, uint32_t num_edges, const float *bbox,
                      const double *face_area, const double *grad_face_area, double *grad_points, uint8_t *cell_status,
                      void *workspace, size_t workspace_bytes, void *stream) {
    g_err[0] = 0;
    if (num_points == 0) return RF_OK;
    if (!points || !point_adjacency_offsets || !bbox || !grad_points || !cell_status ||
        (num_edges && (!point_adjacency || !face_area || !grad_face_area)))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_face_area_grad: null pointer");
    if (!workspace || workspace_bytes < rf_face_area_grad_workspace_bytes(num_points, num_edges))
        return fail(RF_ERR_WORKSPACE, "rf_face_area_grad: workspace missing or too small");
    double *weight = reinterpret_cast<double *>(static_cast<uint8_t *>(workspace) + redo_bytes(num_points));
    if (num_edges)
        hipLaunchKernelGGL(face_area_grad::face_weight_kernel,
                           dim3((num_points + face_area_grad::kWeightWaves - 1u) / face_area_grad::kWeightWaves),
                           dim3(kWave * face_area_grad::kWeightWaves), 0, static_cast<hipStream_t>(stream), num_points,
                           point_adjacency, point_adjacency_offsets, num_edges, face_area, grad_face_area, weight);
    return launch_cell_waves("rf_face_area_grad", stream, num_points, workspace, cell_status,
                             face_area_grad::face_area_grad_kernel, face_area_grad::face_area_grad_redo_kernel, points,
                             num_points, point_adjacency, point_adjacency_offsets, num_edges, bbox, face_area,
                             weight, grad_points);
}

}  // extern "C"
