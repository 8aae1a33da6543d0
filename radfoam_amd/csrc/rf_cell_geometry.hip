// rf_cell_geometry.hip -- what a Voronoi cell IS: volume, centroid, boundedness, face areas, and the faces between
// selected and unselected cells as triangles ("Cell geometry").  Clipping core: rf_clip.hpp, all in double.
//
//   cell_geometry_kernel       one wave per cell, one lane per face.  The row's planes {d_c, |d_c|^2/2} are staged once
//                              in LDS; each lane clips its face's square by the other planes, its polygon in an LDS slot
//                              (vertex-major, lanes side by side: lanes at the same vertex index hit different banks).
//                              Volume and centroid are wave reductions.  Takes rows of up to 64 faces whose polygons stay
//                              within kLaneCap vertices; anything else it hands on, untouched, through redo[cell].
//   cell_geometry_redo_kernel  one wave per 64 cells: a lane per cell reads redo[cell]; the cells handed on are walked one
//                              after the other, face by face, by lane 0 (rf::clip::cell_serial, what the host harness
//                              runs) with room for kWaveCap vertices: slow, and rare -- rows longer than 64, faces like
//                              the 48-gon of the tests.  Beyond that the cell's status says so and the caller raises.
//   surface_count_kernel       lane per adjacency slot: triangles of the face if it separates inside from outside.
//   surface_emit_kernel        wave per listed slot: lane 0 clips the face, the wave writes its triangle fan.
//
// Every output element is written exactly once, by plain stores; no atomics.  An adjacency row is taken as given.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/radfoam_hip_geometry.h"
#include "rf_clip.hpp"
#include "rf_host.hpp"

namespace rf {

constexpr uint32_t kWave = 64;
constexpr uint32_t kLaneCap = 16;    // polygon vertices per lane: 2 buffers * 2 coordinates * 16 * 64 lanes * 8 B = 32 KiB
constexpr uint32_t kWaveCap = 256;   // polygon vertices of the serial path: 8 KiB

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(64) void cell_geometry_kernel(
    const float *__restrict__ points, uint32_t num_points, const uint32_t *__restrict__ adj,
    const uint32_t *__restrict__ offsets, uint32_t num_edges, const float *__restrict__ bbox,
    double *__restrict__ volume, double *__restrict__ centroid, uint8_t *__restrict__ bounded,
    double *__restrict__ face_area, uint32_t *__restrict__ face_vertices, uint8_t *__restrict__ redo) {
    __shared__ double s_plane[4][kWave];             // d_c (x, y, z), |d_c|^2 / 2 of the row
    __shared__ double s_s[2 * kLaneCap][kWave];      // polygons: buffer 0 at vertex rows [0, kLaneCap), buffer 1 after
    __shared__ double s_t[2 * kLaneCap][kWave];
    const uint32_t a = blockIdx.x, lane = threadIdx.x;
    const uint32_t begin = offsets[a], end = offsets[a + 1];
    if (begin > end || end > num_edges || end - begin > kWave) {   // wave-uniform
        if (lane == 0) redo[a] = 1;
        return;
    }
    const uint32_t degree = end - begin;
    if (degree == 0) {   // no neighbours: the whole space
        if (lane == 0) {
            volume[a] = __builtin_inf();
            centroid[3 * (size_t)a] = centroid[3 * (size_t)a + 1] = centroid[3 * (size_t)a + 2] = __builtin_nan("");
            bounded[a] = 0;
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
    s_plane[0][lane] = dx, s_plane[1][lane] = dy, s_plane[2][lane] = dz, s_plane[3][lane] = h;
    __syncthreads();
    if (__any(bad)) {
        if (lane == 0) redo[a] = 1;
        return;
    }
    const double R = clip::half_side(bbox);
    bool overflow = false, unbounded = false;
    double area = 0.0, vol = 0.0, mx = 0.0, my = 0.0, mz = 0.0;
    uint32_t m = 0;
    if (have) {
        const clip::Frame frame = clip::make_frame(dx, dy, dz);
        double *s = &s_s[0][lane], *t = &s_t[0][lane];
        clip::init_square(s, t, kWave, R);
        m = 4;
        uint32_t cur = 0;
        for (uint32_t j = 0; j < degree && m != 0; ++j) {
            if (j == lane) continue;
            double A, B, C;
            clip::plane_in_frame(frame, s_plane[0][j], s_plane[1][j], s_plane[2][j], s_plane[3][j], A, B, C);
            const uint32_t in = cur * kLaneCap * kWave, out = (cur ^ 1u) * kLaneCap * kWave;
            if (!clip::clip_step(s + in, t + in, s + out, t + out, kWave, kLaneCap, m, A, B, C)) {
                overflow = true;
                break;
            }
            cur ^= 1u;
        }
        if (!overflow) {
            double cs, ct;
            clip::measure(s + cur * kLaneCap * kWave, t + cur * kLaneCap * kWave, kWave, m, R, area, cs, ct, unbounded);
            clip::CellSums sums = {0.0, 0.0, 0.0, 0.0, false};
            clip::add_face(sums, frame, area, cs, ct, unbounded);
            vol = sums.volume, mx = sums.mx, my = sums.my, mz = sums.mz;
        }
    }
    if (__any(overflow)) {
        if (lane == 0) redo[a] = 1;
        return;
    }
    if (have) {
        face_area[begin + lane] = unbounded ? __builtin_inf() : area;
        face_vertices[begin + lane] = m;
    }
    const bool open = __any(unbounded);
    vol = wave_sum(vol), mx = wave_sum(mx), my = wave_sum(my), mz = wave_sum(mz);
    if (lane == 0) {
        const float *p = points + 3 * (size_t)a;
        volume[a] = open ? __builtin_inf() : vol;
        centroid[3 * (size_t)a] = open ? __builtin_nan("") : (double)p[0] + mx / vol;
        centroid[3 * (size_t)a + 1] = open ? __builtin_nan("") : (double)p[1] + my / vol;
        centroid[3 * (size_t)a + 2] = open ? __builtin_nan("") : (double)p[2] + mz / vol;
        bounded[a] = open ? 0 : 1;
        redo[a] = 0;
    }
}

__global__ __launch_bounds__(64) void cell_geometry_redo_kernel(
    const float *__restrict__ points, uint32_t num_points, const uint32_t *__restrict__ adj,
    const uint32_t *__restrict__ offsets, uint32_t num_edges, const float *__restrict__ bbox,
    double *__restrict__ volume, double *__restrict__ centroid, uint8_t *__restrict__ bounded,
    double *__restrict__ face_area, uint32_t *__restrict__ face_vertices, const uint8_t *__restrict__ redo,
    uint8_t *__restrict__ cell_status) {
    __shared__ double s_s[2 * kWaveCap], s_t[2 * kWaveCap];
    const uint32_t cell = blockIdx.x * kWave + threadIdx.x;
    const bool mine = cell < num_points && redo[cell] != 0;
    if (cell < num_points && !mine) cell_status[cell] = (uint8_t)clip::kCellOk;
    unsigned long long todo = __ballot(mine);
    if (threadIdx.x != 0) return;
    const double R = clip::half_side(bbox);
    while (todo) {
        const uint32_t a = blockIdx.x * kWave + (uint32_t)__builtin_ctzll(todo);
        todo &= todo - 1ull;
        cell_status[a] = (uint8_t)clip::cell_serial(points, num_points, adj, offsets, num_edges, a, R, s_s, s_t, kWaveCap,
                                                    volume, centroid, bounded, face_area, face_vertices);
    }
}

// the cell whose row holds adjacency slot e: the last a with offsets[a] <= e (kNoCell if the offsets do not say)
constexpr uint32_t kNoCell = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t owner_of_slot(const uint32_t *__restrict__ offsets, uint32_t num_points,
                                                  uint32_t num_edges, uint32_t e) {
    uint32_t lo = 0, hi = num_points + 1u;   // first index whose offset is > e
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (offsets[mid] > e) hi = mid;
        else lo = mid + 1u;
    }
    if (lo == 0 || lo > num_points) return kNoCell;
    const uint32_t a = lo - 1u;
    return (offsets[a] <= e && e < offsets[a + 1] && offsets[a + 1] <= num_edges) ? a : kNoCell;
}

__global__ __launch_bounds__(256) void surface_count_kernel(uint32_t num_points, const uint32_t *__restrict__ adj,
                                                            const uint32_t *__restrict__ offsets, uint32_t num_edges,
                                                            const uint8_t *__restrict__ inside,
                                                            const uint32_t *__restrict__ face_vertices,
                                                            int32_t *__restrict__ triangle_count) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= num_edges) return;
    int32_t count = 0;
    const uint32_t b = adj[e];
    if (b < num_points && !inside[b]) {
        const uint32_t a = owner_of_slot(offsets, num_points, num_edges, e);
        const uint32_t nv = face_vertices[e];
        if (a != kNoCell && inside[a] && nv >= 3u && nv <= kWaveCap) count = (int32_t)(nv - 2u);
    }
    triangle_count[e] = count;
}

__global__ __launch_bounds__(64) void surface_emit_kernel(
    const float *__restrict__ points, uint32_t num_points, const uint32_t *__restrict__ adj,
    const uint32_t *__restrict__ offsets, uint32_t num_edges, const float *__restrict__ bbox,
    const uint32_t *__restrict__ face_vertices, const int64_t *__restrict__ slots,
    const int64_t *__restrict__ triangle_begin, double *__restrict__ triangles, int64_t *__restrict__ triangle_slot) {
    __shared__ double s_s[2 * kWaveCap], s_t[2 * kWaveCap];
    __shared__ clip::Frame s_frame;
    __shared__ uint32_t s_m, s_cur;
    const uint32_t lane = threadIdx.x;
    const int64_t slot64 = slots[blockIdx.x];
    const uint32_t e = (uint32_t)slot64;
    const uint32_t nv = (slot64 >= 0 && slot64 < (int64_t)num_edges) ? face_vertices[e] : 0u;
    if (nv < 3u || nv > kWaveCap) return;   // nothing was counted for such a slot
    const uint32_t count = nv - 2u;
    const uint32_t a = owner_of_slot(offsets, num_points, num_edges, e);
    if (lane == 0) {
        uint32_t m = 0, cur = 0;
        clip::Frame frame = {};
        if (a != kNoCell && clip::row_is_valid(points, num_points, adj, num_edges, a, offsets[a], offsets[a + 1])) {
            if (!clip::face_polygon(points, adj, a, offsets[a], offsets[a + 1], e, clip::half_side(bbox), s_s, s_t, 1u,
                                    kWaveCap, frame, m, cur))
                m = 0;
        }
        s_frame = frame, s_m = m, s_cur = cur;
    }
    __syncthreads();
    const uint32_t m = s_m;
    const double *s = s_s + s_cur * kWaveCap, *t = s_t + s_cur * kWaveCap;
    const int64_t first = triangle_begin[blockIdx.x];
    double px = 0.0, py = 0.0, pz = 0.0;
    if (a != kNoCell) px = points[3 * (size_t)a], py = points[3 * (size_t)a + 1], pz = points[3 * (size_t)a + 2];
    for (uint32_t k = lane; k < count; k += kWave) {
        double *out = triangles + 9 * (size_t)(first + k);
#pragma unroll
        for (uint32_t c = 0; c < 3u; ++c) {
            // the same clipping as rf_cell_geometry, so m == nv; were it not, the missing corners are NaN, never stale
            const uint32_t v = c == 0u ? 0u : k + c;
            double x = __builtin_nan(""), y = x, z = x;
            if (v < m) {
                clip::to_space(s_frame, s[v], t[v], x, y, z);
                x += px, y += py, z += pz;
            }
            out[3 * c] = x, out[3 * c + 1] = y, out[3 * c + 2] = z;
        }
        triangle_slot[first + k] = slot64;
    }
}

}  // namespace rf

using namespace rf;

extern "C" {

size_t rf_cell_geometry_workspace_bytes(uint32_t num_points) { return ((size_t)num_points + 255u) & ~(size_t)255u; }

int rf_cell_geometry(const float *points, uint32_t num_points, const uint32_t *point_adjacency,
                     const uint32_t *point_adjacency_offsets, uint32_t num_edges, const float *bbox, double *volume,
                     double *centroid, uint8_t *bounded, double *face_area, uint32_t *face_vertices,
                     uint8_t *cell_status, void *workspace, size_t workspace_bytes, void *stream) {
    g_err[0] = 0;
    if (num_points == 0) return RF_OK;
    if (!points || !point_adjacency_offsets || !bbox || !volume || !centroid || !bounded || !cell_status ||
        (num_edges && (!point_adjacency || !face_area || !face_vertices)))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_cell_geometry: null pointer");
    if (!workspace || workspace_bytes < rf_cell_geometry_workspace_bytes(num_points))
        return fail(RF_ERR_WORKSPACE, "rf_cell_geometry: workspace missing or too small");
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t *redo = static_cast<uint8_t *>(workspace);
    hipLaunchKernelGGL(cell_geometry_kernel, dim3(num_points), dim3(kWave), 0, s, points, num_points, point_adjacency,
                       point_adjacency_offsets, num_edges, bbox, volume, centroid, bounded, face_area, face_vertices,
                       redo);
    hipLaunchKernelGGL(cell_geometry_redo_kernel, dim3((num_points + kWave - 1u) / kWave), dim3(kWave), 0, s, points, num_points,
                       point_adjacency, point_adjacency_offsets, num_edges, bbox, volume, centroid, bounded, face_area,
                       face_vertices, redo, cell_status);
    return check_launch("rf_cell_geometry");
}

int rf_cell_surface_count(uint32_t num_points, const uint32_t *point_adjacency,
                          const uint32_t *point_adjacency_offsets, uint32_t num_edges, const uint8_t *inside,
                          const uint32_t *face_vertices, int32_t *triangle_count, void *stream) {
    g_err[0] = 0;
    if (num_edges == 0) return RF_OK;
    if (!point_adjacency || !point_adjacency_offsets || !inside || !face_vertices || !triangle_count)
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_cell_surface_count: null pointer");
    hipLaunchKernelGGL(surface_count_kernel, dim3((num_edges + 255u) / 256u), dim3(256), 0,
                       static_cast<hipStream_t>(stream), num_points, point_adjacency, point_adjacency_offsets, num_edges,
                       inside, face_vertices, triangle_count);
    return check_launch("rf_cell_surface_count");
}

int rf_cell_surface_emit(const float *points, uint32_t num_points, const uint32_t *point_adjacency,
                         const uint32_t *point_adjacency_offsets, uint32_t num_edges, const float *bbox,
                         const uint32_t *face_vertices, const int64_t *slots, const int64_t *triangle_begin,
                         uint32_t num_slots, double *triangles, int64_t *triangle_slot, void *stream) {
    g_err[0] = 0;
    if (num_slots == 0) return RF_OK;
    if (!points || !point_adjacency || !point_adjacency_offsets || !bbox || !face_vertices || !slots ||
        !triangle_begin || !triangles || !triangle_slot)
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_cell_surface_emit: null pointer");
    hipLaunchKernelGGL(surface_emit_kernel, dim3(num_slots), dim3(kWave), 0, static_cast<hipStream_t>(stream), points,
                       num_points, point_adjacency, point_adjacency_offsets, num_edges, bbox, face_vertices, slots,
                       triangle_begin, triangles, triangle_slot);
    return check_launch("rf_cell_surface_emit");
}

}  // extern "C"
