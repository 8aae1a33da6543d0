// rf_cell_box_area_grad.hip -- point gradients of the face and wall areas of the Voronoi cells clipped to an axis-aligned
// box ("Point gradients of the face and wall areas in a box").  The mathematics, the labelled list-plane step
// and the two edge terms: rf_clip_box_area_grad.hpp; the plane list and its tie rule: rf_clip_box.hpp; the effective
// weight, the row search and the Voronoi-edge term: rf_clip_area_grad.hpp, all in double.
//
//   box_face_weight_kernel         the pre-pass, one wave per cell and one lane per slot: the effective weight G of every
//                                  slot (its own upstream plus its mate's, found by a search of the neighbour's row, each
//                                  masked by its own boxed face_area; zero for a null upstream) into an f64[E] workspace
//                                  array, by plain stores.
//   cell_box_area_grad_kernel      one wave per cell, one lane per ROW face, the layout of face_area_grad_kernel and
//                                  cell_box_grad_kernel: the list's planes (the row's by their lanes, the six walls behind
//                                  them by lanes 0..5), the row's sites and weights and the cell's six wall weights staged
//                                  in LDS, each lane's polygon in its vertex-major LDS slot with one byte of label per
//                                  vertex beside it (no per-lane arrays).  The lane clips its face again by the whole list
//                                  with labels and sums its edges' terms; three __shfl_xor reductions, and lane 0 writes
//                                  the row.  The walls are clip planes only and take no lanes, so rows of up to 64 faces
//                                  (lists of up to 70 planes) stay here.  Longer rows and polygons of more than kLaneCap
//                                  vertices are handed on, unwritten, through redo[cell].
//   cell_box_area_grad_redo_kernel one wave per 64 cells: the cells handed on are walked by lane 0, face after face
//                                  (rf::clip::cell_box_area_grad_serial, what the host harness runs), with kWaveCap
//                                  vertices.
//
// Row a is a gather over a's own adjacency row, one look-up per Voronoi edge in a neighbour's row and one read of the
// neighbour's wall weight per wall edge: every output element is written exactly once by a plain store, there are no
// atomics, and the result is bit-reproducible.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/radfoam_hip_box_area_grad.h"
#include "rf_clip_box_area_grad.hpp"
#include "rf_host.hpp"

namespace rf {
namespace cell_box_area_grad {

constexpr uint32_t kWave = 64;
constexpr uint32_t kLaneCap = 16;    // as cell_box_kernel: 32 KiB of polygons per wave
constexpr uint32_t kWaveCap = 256;   // as cell_box_redo_kernel
constexpr uint32_t kWeightWaves = 4;
constexpr uint32_t kList = kWave + clip::kWalls;

// the row of a as the wave staged it in LDS: planes[4][kList] (the row's part of the list) and the sites
struct RowFromLds {
    const double *planes;
    const uint32_t *sites;
    __device__ __forceinline__ uint32_t site(uint32_t j) const { return sites[j]; }
    __device__ __forceinline__ void plane(uint32_t j, double &dx, double &dy, double &dz, double &h) const {
        dx = planes[j], dy = planes[kList + j], dz = planes[2 * kList + j], h = planes[3 * kList + j];
    }
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

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
    if (begin > end || end > num_edges || end - begin > kWave) {   // wave-uniform
        if (lane == 0) redo[a] = 1;
        return;
    }
    const uint32_t degree = end - begin, count = degree + clip::kWalls;
    if (degree == 0) {   // no neighbours: the cell is the whole box wherever the site is
        if (lane == 0) {
            grad_points[3 * (size_t)a] = grad_points[3 * (size_t)a + 1] = grad_points[3 * (size_t)a + 2] = 0.0;
            redo[a] = 0;
        }
        return;
    }
    const bool have = lane < degree;
    uint32_t q = have ? adj[begin + lane] : 0u;
    bool bad = have && (q >= num_points || q == a);
    if (!have || bad) q = a;
    double dx, dy, dz, h;
    clip::neighbour(points, a, q, dx, dy, dz, h);
    bad = bad || (have && !(h > 0.0));
    if (have) s_plane[0][lane] = dx, s_plane[1][lane] = dy, s_plane[2][lane] = dz, s_plane[3][lane] = h;
    if (lane < clip::kWalls) {
        double wx, wy, wz, wh;
        clip::wall_plane(points, a, box, lane, wx, wy, wz, wh);
        s_plane[0][degree + lane] = wx, s_plane[1][degree + lane] = wy, s_plane[2][degree + lane] = wz;
        s_plane[3][degree + lane] = wh;
        s_gw[lane] = clip::wall_weight(wall_area, grad_wall_area, a, lane);
    }
    s_q[lane] = q;
    s_g[lane] = have ? weight[begin + lane] : 0.0;
    __syncthreads();
    if (__any(bad)) {
        if (lane == 0) redo[a] = 1;
        return;
    }
    const double R = clip::half_side_box(bbox, box);
    bool overflow = false;
    double gx = 0.0, gy = 0.0, gz = 0.0;
    if (have && nonempty[a]) {   // an empty cell stays empty around here: a zero row
        const clip::Frame frame = clip::list_frame(false, dx, dy, dz, h);
        double *s = &s_s[0][lane], *t = &s_t[0][lane];
        uint8_t *l = &s_l[0][lane];
        clip::init_square(s, t, kWave, R);
        clip::init_square_labels(l, kWave);
        uint32_t m = 4, cur = 0;
        for (uint32_t j = 0; j < count && m != 0; ++j) {
            if (j == lane) continue;
            if (!clip::clip_by_list_plane_labelled(frame, dx, dy, dz, j < lane, s_plane[0][j], s_plane[1][j], s_plane[2][j],
                                                   s_plane[3][j], s, t, l, kWave, kLaneCap, m, cur, (uint8_t)j)) {
                overflow = true;
                break;
            }
        }
        if (!overflow && m != 0) {   // q < num_points: no lane of this wave is bad
            const uint32_t at = cur * kLaneCap * kWave, free_at = (cur ^ 1u) * kLaneCap * kWave;
            const RowFromLds row = {&s_plane[0][0], s_q};
            clip::add_polygon_terms_box(row, degree, lane, frame, dx, dy, dz, s + at, t + at, l + at, s + free_at,
                                        t + free_at, kWave, m, adj, offsets, num_edges, weight, q, s_g, face_area + begin,
                                        s_gw, wall_area, grad_wall_area, gx, gy, gz);
        }
    }
    if (__any(overflow)) {
        if (lane == 0) redo[a] = 1;
        return;
    }
    gx = wave_sum(gx), gy = wave_sum(gy), gz = wave_sum(gz);
    if (lane == 0) {
        grad_points[3 * (size_t)a] = gx, grad_points[3 * (size_t)a + 1] = gy, grad_points[3 * (size_t)a + 2] = gz;
        redo[a] = 0;
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
    const uint32_t cell = blockIdx.x * kWave + threadIdx.x;
    const bool mine = cell < num_points && redo[cell] != 0;
    if (cell < num_points && !mine) cell_status[cell] = (uint8_t)clip::kCellOk;
    unsigned long long todo = __ballot(mine);
    if (threadIdx.x != 0) return;
    const double R = clip::half_side_box(bbox, box);
    while (todo) {
        const uint32_t a = blockIdx.x * kWave + (uint32_t)__builtin_ctzll(todo);
        todo &= todo - 1ull;
        cell_status[a] = (uint8_t)clip::cell_box_area_grad_serial(points, num_points, adj, offsets, num_edges, a, box, R,
                                                                  s_s, s_t, s_l, kWaveCap, nonempty, face_area, wall_area,
                                                                  weight, grad_wall_area, grad_points);
    }
}

}  // namespace cell_box_area_grad
}  // namespace rf

using namespace rf;

static size_t redo_bytes(uint32_t num_points) {
    return ((size_t)num_points + 255u) & ~(size_t)255u;
}

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
    if (!(lo_x < hi_x && lo_y < hi_y && lo_z < hi_z) || !(hi_x - lo_x < __builtin_inf()) ||
        !(hi_y - lo_y < __builtin_inf()) || !(hi_z - lo_z < __builtin_inf()))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_cell_box_area_grad: the box must be finite with lo < hi");
    if (!workspace || workspace_bytes < rf_cell_box_area_grad_workspace_bytes(num_points, num_edges))
        return fail(RF_ERR_WORKSPACE, "rf_cell_box_area_grad: workspace missing or too small");
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t *redo = static_cast<uint8_t *>(workspace);
    double *weight = reinterpret_cast<double *>(redo + redo_bytes(num_points));
    if (num_edges)
        hipLaunchKernelGGL(cell_box_area_grad::box_face_weight_kernel,
                           dim3((num_points + cell_box_area_grad::kWeightWaves - 1u) / cell_box_area_grad::kWeightWaves),
                           dim3(cell_box_area_grad::kWave * cell_box_area_grad::kWeightWaves), 0, s, num_points,
                           point_adjacency, point_adjacency_offsets, num_edges, face_area, grad_face_area, weight);
    hipLaunchKernelGGL(cell_box_area_grad::cell_box_area_grad_kernel, dim3(num_points), dim3(cell_box_area_grad::kWave),
                       0, s, points, num_points, point_adjacency, point_adjacency_offsets, num_edges, bbox, lo_x, lo_y,
                       lo_z, hi_x, hi_y, hi_z, nonempty, face_area, wall_area, weight, grad_wall_area, grad_points, redo);
    hipLaunchKernelGGL(cell_box_area_grad::cell_box_area_grad_redo_kernel,
                       dim3((num_points + cell_box_area_grad::kWave - 1u) / cell_box_area_grad::kWave),
                       dim3(cell_box_area_grad::kWave), 0, s, points, num_points, point_adjacency,
                       point_adjacency_offsets, num_edges, bbox, lo_x, lo_y, lo_z, hi_x, hi_y, hi_z, nonempty, face_area,
                       wall_area, weight, grad_wall_area, grad_points, redo, cell_status);
    return check_launch("rf_cell_box_area_grad");
}

}  // extern "C"
