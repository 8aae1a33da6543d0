// rf_cell_mesh.hip -- the faces between selected and unselected cells as a welded, differentiable mesh (DESIGN.md,
// "Welded surface mesh").  The keys, the serial face and the circumcentre arithmetic: rf_clip_mesh.hpp, all in double.
//
//   mesh_emit_kernel           one lane per listed face, 64 faces per wave (surface_emit_kernel clips on lane 0 while 63
//                              lanes wait).  The lane finds the slot's cell, checks its row and clips the face with
//                              labels straight from the arrays, its polygon and labels in its own column of LDS
//                              (vertex-major, the 64 lanes side by side, two buffers of kLaneCap vertices, uint16
//                              labels: 36 KiB per block).  It writes the face's corners and their keys.  Faces of more
//                              than kLaneCap vertices and rows of 65535 or more entries are handed on, unwritten,
//                              through redo[face].  No lane talks to another: there is no barrier and no cross-lane
//                              operation, a lane's early exit concerns it alone.
//   mesh_emit_redo_kernel      one wave per 64 faces: the faces handed on are walked by lane 0 one after the other
//                              (rf::clip::face_corners_serial, what the host harness runs) with kWaveCap vertices.
//   mesh_vertices_kernel       one lane per vertex: the circumcentre of the key's four sites.
//   mesh_vertices_grad_kernel  one lane per vertex: the four 3-vectors its upstream gives its sites, to f64[V,4,3].
//   mesh_site_sum_kernel       one lane per site: adds the site's run of those vectors (the incidences sorted by site,
//                              stably, by the caller) in double, in that order.
//
// Every output element is written exactly once by a plain store; there are no atomics; every index read from memory is
// range-checked before it is used.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/radfoam_hip_mesh.h"
#include "rf_cell_wave.hpp"
#include "rf_clip_mesh.hpp"

namespace rf {
namespace cell_mesh {

// kWave, kLaneCap, kWaveCap and the redo sweep: rf_cell_wave.hpp (here 32 KiB of polygons and 4 KiB of labels per wave)
constexpr uint32_t kLongRow = 0xFFFFu;   // a uint16 label cannot name this row index apart from "none"
constexpr uint32_t kFlat = 256;

// what face i asks for: its slot e, its cell a (kNoSite if the offsets do not place e), its vertex count and where its
// corners go.  false: nothing of it can be written.
__device__ __forceinline__ bool face_target(const uint32_t *__restrict__ offsets, uint32_t num_points,
                                            uint32_t num_edges, const uint32_t *__restrict__ face_vertices,
                                            const int64_t *__restrict__ slots, const int64_t *__restrict__ corner_begin,
                                            int64_t num_corners, uint32_t i, uint32_t &e, uint32_t &a, uint32_t &nv,
                                            int64_t &first) {
    const int64_t slot64 = slots[i];
    if (slot64 < 0 || slot64 >= (int64_t)num_edges) return false;
    e = (uint32_t)slot64;
    nv = face_vertices[e];
    first = corner_begin[i];
    if (nv < 3u || nv > kWaveCap || first < 0 || first > num_corners || (int64_t)nv > num_corners - first) return false;
    a = clip::slot_owner(offsets, num_points, num_edges, e);
    return true;
}

__global__ __launch_bounds__(64) void mesh_emit_kernel(
    const float *__restrict__ points, uint32_t num_points, const uint32_t *__restrict__ adj,
    const uint32_t *__restrict__ offsets, uint32_t num_edges, const float *__restrict__ bbox,
    const uint32_t *__restrict__ face_vertices, const int64_t *__restrict__ slots,
    const int64_t *__restrict__ corner_begin, uint32_t num_faces, int64_t num_corners, double *__restrict__ corner_xyz,
    uint32_t *__restrict__ corner_sites, uint8_t *__restrict__ redo) {
    __shared__ double s_s[2 * kLaneCap][kWave];      // polygons: buffer 0 at vertex rows [0, kLaneCap), buffer 1 after
    __shared__ double s_t[2 * kLaneCap][kWave];
    __shared__ uint16_t s_l[2 * kLaneCap][kWave];    // labels, beside the vertices
    const uint32_t lane = threadIdx.x, i = blockIdx.x * kWave + lane;
    if (i >= num_faces) return;
    uint32_t e = 0, a = clip::kNoSite, nv = 0;
    int64_t first = 0;
    bool done = false;
    if (face_target(offsets, num_points, num_edges, face_vertices, slots, corner_begin, num_corners, i, e, a, nv, first) &&
        a != clip::kNoSite && nv <= kLaneCap) {
        const uint32_t begin = offsets[a], end = offsets[a + 1];   // in order and within the list: slot_owner
        if (end - begin < kLongRow && clip::row_is_valid(points, num_points, adj, num_edges, a, begin, end)) {
            clip::Frame frame;
            uint32_t m = 0, cur = 0;
            if (clip::face_polygon_labelled(points, adj, a, begin, end, e, clip::half_side(bbox), &s_s[0][lane],
                                            &s_t[0][lane], &s_l[0][lane], kWave, kLaneCap, frame, m, cur) &&
                m == nv) {
                const uint32_t at = cur * kLaneCap;
                clip::write_corners(points, adj + begin, a, adj[e], frame, &s_s[at][lane], &s_t[at][lane],
                                    &s_l[at][lane], kWave, m, corner_xyz + 3 * (size_t)first,
                                    corner_sites + 4 * (size_t)first);
                done = true;
            }
        }
    }
    redo[i] = done ? 0 : 1;
}

__global__ __launch_bounds__(64) void mesh_emit_redo_kernel(
    const float *__restrict__ points, uint32_t num_points, const uint32_t *__restrict__ adj,
    const uint32_t *__restrict__ offsets, uint32_t num_edges, const float *__restrict__ bbox,
    const uint32_t *__restrict__ face_vertices, const int64_t *__restrict__ slots,
    const int64_t *__restrict__ corner_begin, uint32_t num_faces, int64_t num_corners, double *__restrict__ corner_xyz,
    uint32_t *__restrict__ corner_sites, const uint8_t *__restrict__ redo, uint8_t *__restrict__ face_status) {
    __shared__ double s_s[2 * kWaveCap], s_t[2 * kWaveCap];
    __shared__ uint32_t s_l[2 * kWaveCap];
    unsigned long long todo = redo_todo(num_faces, redo, face_status);
    if (threadIdx.x != 0) return;
    const double R = clip::half_side(bbox);
    while (todo) {
        const uint32_t i = redo_next(todo);
        uint32_t e = 0, a = clip::kNoSite, nv = 0;
        int64_t first = 0;
        uint32_t status = clip::kCellBadRow;
        if (face_target(offsets, num_points, num_edges, face_vertices, slots, corner_begin, num_corners, i, e, a, nv, first))
            status = clip::face_corners_serial(points, num_points, adj, offsets, num_edges, a, e, R, s_s, s_t, s_l, kWaveCap,
                                               nv, corner_xyz + 3 * (size_t)first, corner_sites + 4 * (size_t)first);
        face_status[i] = (uint8_t)status;
    }
}

__global__ __launch_bounds__(kFlat) void mesh_vertices_kernel(const float *__restrict__ points, uint32_t num_points,
                                                              const int64_t *__restrict__ vertex_sites,
                                                              uint32_t num_vertices, double *__restrict__ vertices) {
    const uint32_t v = blockIdx.x * kFlat + threadIdx.x;
    if (v >= num_vertices) return;
    clip::key_vertex(points, num_points, vertex_sites + 4 * (size_t)v, vertices + 3 * (size_t)v);
}

__global__ __launch_bounds__(kFlat) void mesh_vertices_grad_kernel(const float *__restrict__ points, uint32_t num_points,
                                                                   const int64_t *__restrict__ vertex_sites,
                                                                   uint32_t num_vertices,
                                                                   const double *__restrict__ grad_vertices,
                                                                   double *__restrict__ site_grad) {
    const uint32_t v = blockIdx.x * kFlat + threadIdx.x;
    if (v >= num_vertices) return;
    clip::key_vertex_grad(points, num_points, vertex_sites + 4 * (size_t)v, grad_vertices + 3 * (size_t)v,
                          site_grad + 12 * (size_t)v);
}

__global__ __launch_bounds__(kFlat) void mesh_site_sum_kernel(uint32_t num_points, uint32_t num_vertices,
                                                              const int64_t *__restrict__ incidence_order,
                                                              const int64_t *__restrict__ site_runs,
                                                              const double *__restrict__ site_grad,
                                                              double *__restrict__ grad_points) {
    const uint32_t a = blockIdx.x * kFlat + threadIdx.x;
    if (a >= num_points) return;
    const int64_t total = 4 * (int64_t)num_vertices;
    int64_t k = site_runs[a], end = site_runs[a + 1];
    if (k < 0) k = 0;
    if (end > total) end = total;
    double x = 0.0, y = 0.0, z = 0.0;
    for (; k < end; ++k) {
        const int64_t at = incidence_order[k];
        if (at < 0 || at >= total) continue;
        x += site_grad[3 * (size_t)at], y += site_grad[3 * (size_t)at + 1], z += site_grad[3 * (size_t)at + 2];
    }
    grad_points[3 * (size_t)a] = x, grad_points[3 * (size_t)a + 1] = y, grad_points[3 * (size_t)a + 2] = z;
}

}  // namespace cell_mesh
}  // namespace rf

using namespace rf;

extern "C" {

size_t rf_cell_mesh_emit_workspace_bytes(uint32_t num_faces) { return redo_bytes(num_faces); }

int rf_cell_mesh_emit(const float *points, uint32_t num_points, const uint32_t *point_adjacency,
                      const uint32_t *point_adjacency_offsets, uint32_t num_edges, const float *bbox,
                      const uint32_t *face_vertices, const int64_t *slots, const int64_t *corner_begin,
                      uint32_t num_faces, int64_t num_corners, double *corner_xyz, uint32_t *corner_sites,
                      uint8_t *face_status, void *workspace, size_t workspace_bytes, void *stream) {
    g_err[0] = 0;
    if (num_faces == 0) return RF_OK;
    if (!points || !point_adjacency || !point_adjacency_offsets || !bbox || !face_vertices || !slots || !corner_begin ||
        !face_status || num_corners < 0 || (num_corners && (!corner_xyz || !corner_sites)))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_cell_mesh_emit: null pointer");
    if (!workspace || workspace_bytes < rf_cell_mesh_emit_workspace_bytes(num_faces))
        return fail(RF_ERR_WORKSPACE, "rf_cell_mesh_emit: workspace missing or too small");
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t *redo = static_cast<uint8_t *>(workspace);
    const dim3 grid((num_faces + kWave - 1u) / kWave), block(kWave);
    hipLaunchKernelGGL(cell_mesh::mesh_emit_kernel, grid, block, 0, s, points, num_points, point_adjacency,
                       point_adjacency_offsets, num_edges, bbox, face_vertices, slots, corner_begin, num_faces, num_corners,
                       corner_xyz, corner_sites, redo);
    hipLaunchKernelGGL(cell_mesh::mesh_emit_redo_kernel, grid, block, 0, s, points, num_points, point_adjacency,
                       point_adjacency_offsets, num_edges, bbox, face_vertices, slots, corner_begin, num_faces, num_corners,
                       corner_xyz, corner_sites, redo, face_status);
    return check_launch("rf_cell_mesh_emit");
}

int rf_mesh_vertices(const float *points, uint32_t num_points, const int64_t *vertex_sites, uint32_t num_vertices,
                     double *vertices, void *stream) {
    g_err[0] = 0;
    if (num_vertices == 0) return RF_OK;
    if (!vertex_sites || !vertices || (num_points && !points))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_mesh_vertices: null pointer");
    hipLaunchKernelGGL(cell_mesh::mesh_vertices_kernel, dim3((num_vertices + cell_mesh::kFlat - 1u) / cell_mesh::kFlat),
                       dim3(cell_mesh::kFlat), 0, static_cast<hipStream_t>(stream), points, num_points, vertex_sites,
                       num_vertices, vertices);
    return check_launch("rf_mesh_vertices");
}

int rf_mesh_vertices_grad(const float *points, uint32_t num_points, const int64_t *vertex_sites, uint32_t num_vertices,
                          const double *grad_vertices, const int64_t *incidence_order, const int64_t *site_runs,
                          double *site_grad, double *grad_points, void *stream) {
    g_err[0] = 0;
    if (num_points == 0) return RF_OK;
    if (!points || !site_runs || !grad_points ||
        (num_vertices && (!vertex_sites || !grad_vertices || !incidence_order || !site_grad)))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_mesh_vertices_grad: null pointer");
    if (num_vertices > 0x3FFFFFFFu) return fail(RF_ERR_INVALID_ARGUMENT, "rf_mesh_vertices_grad: more than 2^30 vertices");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (num_vertices)
        hipLaunchKernelGGL(cell_mesh::mesh_vertices_grad_kernel,
                           dim3((num_vertices + cell_mesh::kFlat - 1u) / cell_mesh::kFlat), dim3(cell_mesh::kFlat), 0, s,
                           points, num_points, vertex_sites, num_vertices, grad_vertices, site_grad);
    hipLaunchKernelGGL(cell_mesh::mesh_site_sum_kernel, dim3((num_points + cell_mesh::kFlat - 1u) / cell_mesh::kFlat),
                       dim3(cell_mesh::kFlat), 0, s, num_points, num_vertices, incidence_order, site_runs, site_grad,
                       grad_points);
    return check_launch("rf_mesh_vertices_grad");
}

}  // extern "C"
