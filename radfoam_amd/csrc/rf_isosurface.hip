// rf_isosurface.hip -- marching tetrahedra on the Delaunay mesh ("Isosurface of an interpolated field").  The
// mask, the case rule, the winding, the keys, the vertex and its backward: rf_iso.hpp, all in double.
//
//   iso_count_kernel          one lane per tetrahedron: its row of indices in one 16-byte load (two for int64), the
//                             range check, four gathered values, the mask; writes the triangle count (0, 1 or 2) and,
//                             where an index is out of range, 1 to the flag word (a plain store of one value).
//   iso_emit_kernel           one lane per tetrahedron: those that count none leave at once; the rest gather their four
//                             sites for the sign of the determinant and write their triangles' three keys, in the final
//                             winding, and their own index, at the offset the scan of the counts gives them.
//   iso_vertices_kernel       one lane per welded edge: x and t.
//   iso_vertices_grad_kernel  one lane per welded edge: (grad p, grad v) for its two sites, to f64[V,2,4].
//   iso_site_sum_kernel       one lane per site: adds the site's run of those (the incidences sorted by site, stably, by
//                             the caller) in double, in that order.
//
// Streaming kernels without reuse: 256 lanes a block, a lane an item, nothing in LDS.  Every output element is written
// exactly once by a plain store; there are no atomics; every index read from memory is range-checked before it is used.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/radfoam_hip_isosurface.h"
#include "rf_host.hpp"
#include "rf_iso.hpp"

namespace rf {
namespace iso {

constexpr uint32_t kFlat = 256;

// the row of tetrahedron t, whole: tets is 16-byte aligned and a row is 16 or 32 bytes
__device__ __forceinline__ void load_row(const uint32_t *__restrict__ tets, uint32_t t, uint32_t *row) {
    const uint4 r = reinterpret_cast<const uint4 *>(tets)[t];
    row[0] = r.x, row[1] = r.y, row[2] = r.z, row[3] = r.w;
}

__device__ __forceinline__ void load_row(const int64_t *__restrict__ tets, uint32_t t, int64_t *row) {
    const longlong2 lo = reinterpret_cast<const longlong2 *>(tets)[2 * (size_t)t],
                    hi = reinterpret_cast<const longlong2 *>(tets)[2 * (size_t)t + 1];
    row[0] = lo.x, row[1] = lo.y, row[2] = hi.x, row[3] = hi.y;
}

template <typename I>
__global__ __launch_bounds__(kFlat) void iso_count_kernel(const I *__restrict__ tets, uint32_t num_tets,
                                                          const float *__restrict__ values, uint32_t num_points,
                                                          double level, uint8_t *__restrict__ counts,
                                                          uint32_t *__restrict__ bad) {
    const uint32_t t = blockIdx.x * kFlat + threadIdx.x;
    if (t >= num_tets) return;
    I row[4];
    int64_t s[4];
    load_row(tets, t, row);
    uint32_t n = 0u;
    if (tet_sites(row, num_points, s))
        n = mask_triangles(sites_mask(values, s, level));
    else
        *bad = 1u;
    counts[t] = (uint8_t)n;
}

template <typename I>
__global__ __launch_bounds__(kFlat) void iso_emit_kernel(const I *__restrict__ tets, uint32_t num_tets,
                                                         const float *__restrict__ points,
                                                         const float *__restrict__ values, uint32_t num_points,
                                                         double level, const uint8_t *__restrict__ counts,
                                                         const int64_t *__restrict__ ends, int64_t num_triangles,
                                                         int64_t *__restrict__ keys, int64_t *__restrict__ triangle_tet) {
    const uint32_t t = blockIdx.x * kFlat + threadIdx.x;
    if (t >= num_tets) return;
    const uint32_t count = counts[t];
    if (count == 0u || count > 2u) return;
    const int64_t first = ends[t] - (int64_t)count;
    if (first < 0 || first > num_triangles - (int64_t)count) return;
    I row[4];
    int64_t s[4], k[6];
    load_row(tets, t, row);
    tet_emit(points, values, tet_sites(row, num_points, s), s, level, count, k);
    for (uint32_t f = 0; f < count; ++f) {
        keys[3 * (size_t)(first + f)] = k[3 * f], keys[3 * (size_t)(first + f) + 1] = k[3 * f + 1];
        keys[3 * (size_t)(first + f) + 2] = k[3 * f + 2];
        triangle_tet[first + f] = (int64_t)t;
    }
}

__global__ __launch_bounds__(kFlat) void iso_vertices_kernel(const float *__restrict__ points,
                                                             const float *__restrict__ values, uint32_t num_points,
                                                             const int64_t *__restrict__ vertex_sites,
                                                             uint32_t num_vertices, double level,
                                                             double *__restrict__ vertices, double *__restrict__ vertex_t) {
    const uint32_t v = blockIdx.x * kFlat + threadIdx.x;
    if (v >= num_vertices) return;
    edge_vertex(points, values, num_points, vertex_sites + 2 * (size_t)v, level, vertices + 3 * (size_t)v, vertex_t + v);
}

__global__ __launch_bounds__(kFlat) void iso_vertices_grad_kernel(const float *__restrict__ points,
                                                                  const float *__restrict__ values, uint32_t num_points,
                                                                  const int64_t *__restrict__ vertex_sites,
                                                                  uint32_t num_vertices, double level,
                                                                  const double *__restrict__ grad_vertices,
                                                                  double *__restrict__ site_grad) {
    const uint32_t v = blockIdx.x * kFlat + threadIdx.x;
    if (v >= num_vertices) return;
    edge_vertex_grad(points, values, num_points, vertex_sites + 2 * (size_t)v, level, grad_vertices + 3 * (size_t)v,
                     site_grad + 8 * (size_t)v);
}

__global__ __launch_bounds__(kFlat) void iso_site_sum_kernel(uint32_t num_points, uint32_t num_vertices,
                                                             const int64_t *__restrict__ incidence_order,
                                                             const int64_t *__restrict__ site_runs,
                                                             const double *__restrict__ site_grad,
                                                             double *__restrict__ grad_points,
                                                             double *__restrict__ grad_values) {
    const uint32_t a = blockIdx.x * kFlat + threadIdx.x;
    if (a >= num_points) return;
    const int64_t total = 2 * (int64_t)num_vertices;
    int64_t k = site_runs[a], end = site_runs[a + 1];
    if (k < 0) k = 0;
    if (end > total) end = total;
    double x = 0.0, y = 0.0, z = 0.0, w = 0.0;
    for (; k < end; ++k) {
        const int64_t at = incidence_order[k];
        if (at < 0 || at >= total) continue;
        const double *part = site_grad + 4 * (size_t)at;
        x += part[0], y += part[1], z += part[2], w += part[3];
    }
    grad_points[3 * (size_t)a] = x, grad_points[3 * (size_t)a + 1] = y, grad_points[3 * (size_t)a + 2] = z;
    grad_values[a] = w;
}

inline dim3 flat_grid(uint32_t n) { return dim3((n + kFlat - 1u) / kFlat); }

// what every entry point asks of its tetrahedra; nullptr if they pass
inline const char *tets_fault(const void *tets, uint32_t index_bytes, uint32_t num_tets, uint32_t num_points) {
    if (index_bytes != 4u && index_bytes != 8u) return "index_bytes must be 4 or 8";
    if ((uintptr_t)tets % 16u) return "tets must be 16-byte aligned";
    if (num_tets > 0x40000000u) return "more than 2^30 tetrahedra";
    if (num_points >= 0x80000000u) return "2^31 points or more";
    return nullptr;
}

}  // namespace iso
}  // namespace rf

using namespace rf;

extern "C" {

int rf_isosurface_count(const void *tets, uint32_t index_bytes, uint32_t num_tets, const float *values,
                        uint32_t num_points, double level, uint8_t *counts, uint32_t *bad, void *stream) {
    g_err[0] = 0;
    if (num_tets == 0) return RF_OK;
    if (!tets || !counts || !bad || (num_points && !values))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_isosurface_count: null pointer");
    if (const char *why = iso::tets_fault(tets, index_bytes, num_tets, num_points))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_isosurface_count: %s", why);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (index_bytes == 4u)
        hipLaunchKernelGGL(iso::iso_count_kernel<uint32_t>, iso::flat_grid(num_tets), dim3(iso::kFlat), 0, s,
                           static_cast<const uint32_t *>(tets), num_tets, values, num_points, level, counts, bad);
    else
        hipLaunchKernelGGL(iso::iso_count_kernel<int64_t>, iso::flat_grid(num_tets), dim3(iso::kFlat), 0, s,
                           static_cast<const int64_t *>(tets), num_tets, values, num_points, level, counts, bad);
    return check_launch("rf_isosurface_count");
}

int rf_isosurface_emit(const void *tets, uint32_t index_bytes, uint32_t num_tets, const float *points, const float *values,
                       uint32_t num_points, double level, const uint8_t *counts, const int64_t *ends,
                       int64_t num_triangles, int64_t *keys, int64_t *triangle_tet, void *stream) {
    g_err[0] = 0;
    if (num_tets == 0 || num_triangles == 0) return RF_OK;
    if (!tets || !counts || !ends || !keys || !triangle_tet || num_triangles < 0 || (num_points && (!points || !values)))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_isosurface_emit: null pointer");
    if (const char *why = iso::tets_fault(tets, index_bytes, num_tets, num_points))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_isosurface_emit: %s", why);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (index_bytes == 4u)
        hipLaunchKernelGGL(iso::iso_emit_kernel<uint32_t>, iso::flat_grid(num_tets), dim3(iso::kFlat), 0, s,
                           static_cast<const uint32_t *>(tets), num_tets, points, values, num_points, level, counts, ends,
                           num_triangles, keys, triangle_tet);
    else
        hipLaunchKernelGGL(iso::iso_emit_kernel<int64_t>, iso::flat_grid(num_tets), dim3(iso::kFlat), 0, s,
                           static_cast<const int64_t *>(tets), num_tets, points, values, num_points, level, counts, ends,
                           num_triangles, keys, triangle_tet);
    return check_launch("rf_isosurface_emit");
}

int rf_isosurface_vertices(const float *points, const float *values, uint32_t num_points, const int64_t *vertex_sites,
                           uint32_t num_vertices, double level, double *vertices, double *vertex_t, void *stream) {
    g_err[0] = 0;
    if (num_vertices == 0) return RF_OK;
    if (!vertex_sites || !vertices || !vertex_t || (num_points && (!points || !values)))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_isosurface_vertices: null pointer");
    hipLaunchKernelGGL(iso::iso_vertices_kernel, iso::flat_grid(num_vertices), dim3(iso::kFlat), 0,
                       static_cast<hipStream_t>(stream), points, values, num_points, vertex_sites, num_vertices, level,
                       vertices, vertex_t);
    return check_launch("rf_isosurface_vertices");
}

int rf_isosurface_vertices_grad(const float *points, const float *values, uint32_t num_points, const int64_t *vertex_sites,
                                uint32_t num_vertices, double level, const double *grad_vertices,
                                const int64_t *incidence_order, const int64_t *site_runs, double *site_grad,
                                double *grad_points, double *grad_values, void *stream) {
    g_err[0] = 0;
    if (num_points == 0) return RF_OK;
    if (!points || !values || !site_runs || !grad_points || !grad_values ||
        (num_vertices && (!vertex_sites || !grad_vertices || !incidence_order || !site_grad)))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_isosurface_vertices_grad: null pointer");
    if (num_vertices > 0x40000000u)
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_isosurface_vertices_grad: more than 2^30 vertices");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (num_vertices)
        hipLaunchKernelGGL(iso::iso_vertices_grad_kernel, iso::flat_grid(num_vertices), dim3(iso::kFlat), 0, s, points,
                           values, num_points, vertex_sites, num_vertices, level, grad_vertices, site_grad);
    hipLaunchKernelGGL(iso::iso_site_sum_kernel, iso::flat_grid(num_points), dim3(iso::kFlat), 0, s, num_points,
                       num_vertices, incidence_order, site_runs, site_grad, grad_points, grad_values);
    return check_launch("rf_isosurface_vertices_grad");
}

}  // extern "C"
