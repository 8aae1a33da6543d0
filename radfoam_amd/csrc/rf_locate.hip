// rf_locate.hip -- point location and interpolation on the Delaunay mesh ("Point location and interpolation").
// The face signs, the step, the faults, the interpolation and its backward: rf_locate.hpp, shared with the host build of
// tests/host_harness; the exact predicate: rf_star.hpp, as the triangulation uses it.
//
//   locate_walk_kernel        one lane per query: walks from its start row across the face of the lowest negative sign
//                             until no sign is negative, the hull, a fault or max_hops.  A row of indices and a row of
//                             adjacency are one 16-byte load each (two for int64).  The fp64 filter of every predicate is
//                             inline; what it cannot sign goes to the 384-bit path, out of line.
//   interp_kernel             one lane per query: value, weights, gradient.
//   interp_grad_parts_kernel  one lane per query: the parts of its four corners, once, and the query's own gradient.
//   interp_site_sum_kernel    one lane per site: adds the site's run of the parts (the corners sorted by site, stably, by
//                             the caller) in double, in that order.
//
// 256 lanes a block, a lane an item, nothing in LDS.  tet, hops and every other output element are written by plain
// stores of their one lane; there are no atomics; every index read from memory is range-checked before it is used.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/radfoam_hip_locate.h"
#include "rf_host.hpp"

#define RF_STAR_FN __device__ __forceinline__
#define RF_STAR_NOINLINE __device__ __noinline__
#define RF_STAR_NOUNROLL _Pragma("nounroll")
#include "rf_locate.hpp"

namespace rf {
namespace locate {

constexpr uint32_t kFlat = 256;

template <typename I>
__global__ __launch_bounds__(kFlat) void locate_walk_kernel(const float *__restrict__ pts, uint32_t n,
                                                            const I *__restrict__ tets, const I *__restrict__ adjacency,
                                                            uint32_t num_tets, const float *__restrict__ queries,
                                                            const int64_t *__restrict__ start, uint32_t num_queries,
                                                            uint32_t max_hops, int64_t *__restrict__ tet_out,
                                                            int32_t *__restrict__ hops_out, uint32_t *__restrict__ flags) {
    const uint32_t k = blockIdx.x * kFlat + threadIdx.x;
    if (k >= num_queries) return;
    const float q[3] = {queries[3 * (size_t)k], queries[3 * (size_t)k + 1], queries[3 * (size_t)k + 2]};
    int64_t tet;
    int32_t hops;
    walk(pts, n, tets, adjacency, num_tets, q, start ? start[k] : 0, max_hops, tet, hops);
    if (tet < kOutside) flags[((-2 - tet) & 7) == (int64_t)kHopCap ? 1 : 0] = 1u;
    tet_out[k] = tet;
    hops_out[k] = hops;
}

template <typename I>
__global__ __launch_bounds__(kFlat) void interp_kernel(const float *__restrict__ pts, uint32_t n, const I *__restrict__ tets,
                                                       uint32_t num_tets, const float *__restrict__ values,
                                                       uint32_t channels, const float *__restrict__ queries,
                                                       const int64_t *__restrict__ tet, uint32_t num_queries,
                                                       double *__restrict__ value, double *__restrict__ weights,
                                                       double *__restrict__ gradient) {
    const uint32_t k = blockIdx.x * kFlat + threadIdx.x;
    if (k >= num_queries) return;
    const float q[3] = {queries[3 * (size_t)k], queries[3 * (size_t)k + 1], queries[3 * (size_t)k + 2]};
    int64_t s[4];
    const bool ok = located_sites(tets, num_tets, n, tet[k], s);
    interpolate(pts, s, ok, values, channels, q, value + (size_t)k * channels, weights + 4 * (size_t)k,
                gradient + 3 * (size_t)k * channels);
}

template <typename I>
__global__ __launch_bounds__(kFlat) void interp_grad_parts_kernel(const float *__restrict__ pts, uint32_t n,
                                                                  const I *__restrict__ tets, uint32_t num_tets,
                                                                  const float *__restrict__ values, uint32_t channels,
                                                                  const float *__restrict__ queries,
                                                                  const int64_t *__restrict__ tet, uint32_t num_queries,
                                                                  const double *__restrict__ grad_value,
                                                                  double *__restrict__ parts,
                                                                  double *__restrict__ grad_queries) {
    const uint32_t k = blockIdx.x * kFlat + threadIdx.x;
    if (k >= num_queries) return;
    const float q[3] = {queries[3 * (size_t)k], queries[3 * (size_t)k + 1], queries[3 * (size_t)k + 2]};
    int64_t s[4];
    const bool ok = located_sites(tets, num_tets, n, tet[k], s);
    interpolate_grad(pts, s, ok, values, channels, q, grad_value + (size_t)k * channels,
                     parts + 4 * (size_t)k * (3u + channels), grad_queries + 3 * (size_t)k);
}

__global__ __launch_bounds__(kFlat) void interp_site_sum_kernel(uint32_t num_points, uint32_t num_queries, uint32_t channels,
                                                                const int64_t *__restrict__ incidence_order,
                                                                const int64_t *__restrict__ site_runs,
                                                                const double *__restrict__ parts,
                                                                double *__restrict__ grad_points,
                                                                double *__restrict__ grad_values) {
    const uint32_t a = blockIdx.x * kFlat + threadIdx.x;
    if (a >= num_points) return;
    site_sum(incidence_order, site_runs, 4 * (int64_t)num_queries, parts, channels, a, grad_points, grad_values);
}

inline dim3 flat_grid(uint32_t n) { return dim3((n + kFlat - 1u) / kFlat); }

// what every entry point asks of its tables; nullptr if they pass
inline const char *tables_fault(const void *tets, const void *adjacency, uint32_t index_bytes, uint32_t num_tets,
                                uint32_t num_points, uint32_t num_queries) {
    if (index_bytes != 4u && index_bytes != 8u) return "index_bytes must be 4 or 8";
    if ((uintptr_t)tets % 16u || (uintptr_t)adjacency % 16u) return "tets and tet_adjacency must be 16-byte aligned";
    if (num_tets > kMaxTets) return "2^30 tetrahedra or more";
    if (num_points >= 0x80000000u) return "2^31 points or more";
    if (num_queries > 0x40000000u) return "more than 2^30 queries";
    return nullptr;
}

}  // namespace locate
}  // namespace rf

using namespace rf;

extern "C" {

int rf_locate_walk(const float *points, uint32_t num_points, const void *tets, const void *tet_adjacency,
                   uint32_t index_bytes, uint32_t num_tets, const float *queries, const int64_t *start,
                   uint32_t num_queries, uint32_t max_hops, int64_t *tet, int32_t *hops, uint32_t *flags, void *stream) {
    g_err[0] = 0;
    if (num_queries == 0) return RF_OK;
    if (!queries || !tet || !hops || !flags || (num_points && !points) || (num_tets && (!tets || !tet_adjacency)))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_locate_walk: null pointer");
    if (const char *why = locate::tables_fault(tets, tet_adjacency, index_bytes, num_tets, num_points, num_queries))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_locate_walk: %s", why);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (index_bytes == 4u)
        hipLaunchKernelGGL(locate::locate_walk_kernel<uint32_t>, locate::flat_grid(num_queries), dim3(locate::kFlat), 0, s,
                           points, num_points, static_cast<const uint32_t *>(tets),
                           static_cast<const uint32_t *>(tet_adjacency), num_tets, queries, start, num_queries, max_hops,
                           tet, hops, flags);
    else
        hipLaunchKernelGGL(locate::locate_walk_kernel<int64_t>, locate::flat_grid(num_queries), dim3(locate::kFlat), 0, s,
                           points, num_points, static_cast<const int64_t *>(tets),
                           static_cast<const int64_t *>(tet_adjacency), num_tets, queries, start, num_queries, max_hops,
                           tet, hops, flags);
    return check_launch("rf_locate_walk");
}

int rf_interpolate(const float *points, uint32_t num_points, const void *tets, uint32_t index_bytes, uint32_t num_tets,
                   const float *values, uint32_t channels, const float *queries, const int64_t *tet, uint32_t num_queries,
                   double *value, double *weights, double *gradient, void *stream) {
    g_err[0] = 0;
    if (num_queries == 0) return RF_OK;
    if (!queries || !tet || !value || !weights || !gradient || (num_points && (!points || !values)) || (num_tets && !tets))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_interpolate: null pointer");
    if (channels == 0 || channels > locate::kMaxChannels)
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_interpolate: channels must be in 1..8");
    if (const char *why = locate::tables_fault(tets, nullptr, index_bytes, num_tets, num_points, num_queries))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_interpolate: %s", why);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (index_bytes == 4u)
        hipLaunchKernelGGL(locate::interp_kernel<uint32_t>, locate::flat_grid(num_queries), dim3(locate::kFlat), 0, s, points,
                           num_points, static_cast<const uint32_t *>(tets), num_tets, values, channels, queries, tet,
                           num_queries, value, weights, gradient);
    else
        hipLaunchKernelGGL(locate::interp_kernel<int64_t>, locate::flat_grid(num_queries), dim3(locate::kFlat), 0, s, points,
                           num_points, static_cast<const int64_t *>(tets), num_tets, values, channels, queries, tet,
                           num_queries, value, weights, gradient);
    return check_launch("rf_interpolate");
}

int rf_interpolate_grad(const float *points, uint32_t num_points, const void *tets, uint32_t index_bytes, uint32_t num_tets,
                        const float *values, uint32_t channels, const float *queries, const int64_t *tet,
                        uint32_t num_queries, const double *grad_value, const int64_t *incidence_order,
                        const int64_t *site_runs, double *parts, double *grad_points, double *grad_values,
                        double *grad_queries, void *stream) {
    g_err[0] = 0;
    if (num_points == 0 && num_queries == 0) return RF_OK;
    if ((num_points && (!points || !values || !site_runs || !grad_points || !grad_values)) || (num_tets && !tets) ||
        (num_queries && (!queries || !tet || !grad_value || !incidence_order || !parts || !grad_queries)))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_interpolate_grad: null pointer");
    if (channels == 0 || channels > locate::kMaxChannels)
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_interpolate_grad: channels must be in 1..8");
    if (const char *why = locate::tables_fault(tets, nullptr, index_bytes, num_tets, num_points, num_queries))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_interpolate_grad: %s", why);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (num_queries) {
        if (index_bytes == 4u)
            hipLaunchKernelGGL(locate::interp_grad_parts_kernel<uint32_t>, locate::flat_grid(num_queries),
                               dim3(locate::kFlat), 0, s, points, num_points, static_cast<const uint32_t *>(tets), num_tets,
                               values, channels, queries, tet, num_queries, grad_value, parts, grad_queries);
        else
            hipLaunchKernelGGL(locate::interp_grad_parts_kernel<int64_t>, locate::flat_grid(num_queries),
                               dim3(locate::kFlat), 0, s, points, num_points, static_cast<const int64_t *>(tets), num_tets,
                               values, channels, queries, tet, num_queries, grad_value, parts, grad_queries);
    }
    if (num_points)
        hipLaunchKernelGGL(locate::interp_site_sum_kernel, locate::flat_grid(num_points), dim3(locate::kFlat), 0, s,
                           num_points, num_queries, channels, incidence_order, site_runs, parts, grad_points, grad_values);
    return check_launch("rf_interpolate_grad");
}

}  // extern "C"
