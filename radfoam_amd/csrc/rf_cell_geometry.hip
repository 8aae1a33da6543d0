// rf_cell_geometry.hip -- what a Voronoi cell IS: volume, centroid, boundedness, face areas, and the faces between
// selected and unselected cells as triangles ("Cell geometry").  Clipping core: rf_clip.hpp, all in double.
// The wave scheme, its LDS layout and the hand-off through redo[cell]: rf_cell_wave.hpp.
//
//   cell_geometry_kernel       the scheme's plain form: the face's area and vertex count per lane, volume and first
//                              moments as wave reductions.  Rows of up to 64 faces.
//   cell_geometry_redo_kernel  the cells handed on, by rf::clip::cell_serial: rows longer than 64, faces like the 48-gon
//                              of the tests.
//   surface_count_kernel       lane per adjacency slot: triangles of the face if it separates inside from outside.
//   surface_emit_kernel        wave per listed slot: lane 0 clips the face, the wave writes its triangle fan.
//
// Every output element is written exactly once, by plain stores; no atomics.  An adjacency row is taken as given.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/radfoam_hip_geometry.h"
#include "rf_cell_wave.hpp"

namespace rf {

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
    if (begin > end || end > num_edges || end - begin > kWave) return hand_on(redo, a, lane);   // wave-uniform
    const uint32_t degree = end - begin;
    if (degree == 0) {   // no neighbours: the whole space
        if (lane == 0) {
            volume[a] = __builtin_inf();
            centroid[3 * (size_t)a] = centroid[3 * (size_t)a + 1] = centroid[3 * (size_t)a + 2] = __builtin_nan("");
            bounded[a] = 0;
            keep(redo, a);
        }
        return;
    }
    const CellLane f = stage_row(points, num_points, adj, a, begin, degree, lane, s_plane);
    if (sync_any_bad(f.bad)) return hand_on(redo, a, lane);
    const double R = clip::half_side(bbox);
    bool overflow = false, unbounded = false;
    double area = 0.0, vol = 0.0, mx = 0.0, my = 0.0, mz = 0.0;
    uint32_t m = 0;
    if (f.have) {
        const clip::Frame frame = clip::make_frame(f.dx, f.dy, f.dz);
        double *s = &s_s[0][lane], *t = &s_t[0][lane];
        const Clipped c = clip_by_row(frame, s_plane, degree, lane, R, s, t);
        m = c.m, overflow = c.overflow;
        if (!overflow) {
            const uint32_t at = c.cur * kLaneCap * kWave;
            double cs, ct;
            clip::measure(s + at, t + at, kWave, m, R, area, cs, ct, unbounded);
            clip::CellSums sums = {0.0, 0.0, 0.0, 0.0, false};
            clip::add_face(sums, frame, area, cs, ct, unbounded);
            vol = sums.volume, mx = sums.mx, my = sums.my, mz = sums.mz;
        }
    }
    if (__any(overflow)) return hand_on(redo, a, lane);
    if (f.have) {
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
        keep(redo, a);
    }
}

__global__ __launch_bounds__(64) void cell_geometry_redo_kernel(
    const float *__restrict__ points, uint32_t num_points, const uint32_t *__restrict__ adj,
    const uint32_t *__restrict__ offsets, uint32_t num_edges, const float *__restrict__ bbox,
    double *__restrict__ volume, double *__restrict__ centroid, uint8_t *__restrict__ bounded,
    double *__restrict__ face_area, uint32_t *__restrict__ face_vertices, const uint8_t *__restrict__ redo,
    uint8_t *__restrict__ cell_status) {
    __shared__ double s_s[2 * kWaveCap], s_t[2 * kWaveCap];
    unsigned long long todo = redo_todo(num_points, redo, cell_status);
    if (threadIdx.x != 0) return;
    const double R = clip::half_side(bbox);
    while (todo) {
        const uint32_t a = redo_next(todo);
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

size_t rf_cell_geometry_workspace_bytes(uint32_t num_points) { return redo_bytes(num_points); }

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
    return launch_cell_waves("rf_cell_geometry", stream, num_points, workspace, cell_status, cell_geometry_kernel,
                             cell_geometry_redo_kernel, points, num_points, point_adjacency, point_adjacency_offsets,
                             num_edges, bbox, volume, centroid, bounded, face_area, face_vertices);
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
