// rf_nearest.hip -- the Voronoi cell of any point by a greedy walk over the neighbour lists ("Cell location").
// The predicate, the key, the step, the seeds and the faults: rf_nearest.hpp, shared with the host build of
// tests/host_harness; the 384-bit integers of the exact path: rf_star.hpp, as the triangulation uses them.
//
//   locate_cells_kernel   one lane per query, 256 lanes a block.  Without given starts the block stages the coordinates of
//                         the S <= 1024 seed sites in LDS once (one barrier), and every lane scans them with the fp64
//                         filter for its start.  Then the walk: per step the row's bounds, then the row's entries and their
//                         points, kGather entries requested before the first is consumed.  What the filter cannot sign
//                         goes to the exact path, out of line.
//
// cell and hops are written once each by plain stores of their one lane; there are no atomics, no LDS beyond the seeds
// and no barrier after the staging one; every index read from memory is range-checked before it is used.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/radfoam_hip_nearest.h"
#include "rf_host.hpp"

#define RF_STAR_FN __device__ __forceinline__
#define RF_STAR_NOINLINE __device__ __noinline__
#define RF_STAR_NOUNROLL _Pragma("nounroll")
#define RF_NEAREST_UNROLL _Pragma("unroll")
#include "rf_nearest.hpp"

namespace rf {
namespace nearest {

constexpr uint32_t kFlat = 256;

template <typename Idx>
__global__ __launch_bounds__(kFlat) void locate_cells_kernel(const float *__restrict__ pts, uint32_t n,
                                                             const Idx *__restrict__ adj, const Idx *__restrict__ offsets,
                                                             uint32_t num_edges, const float *__restrict__ queries,
                                                             const int64_t *__restrict__ start, uint32_t num_seeds,
                                                             uint32_t num_queries, uint32_t max_hops,
                                                             int64_t *__restrict__ cell_out, int32_t *__restrict__ hops_out,
                                                             uint32_t *__restrict__ flags) {
    __shared__ float s_seeds[3 * kMaxSeeds];
    if (!start && num_seeds) {   // block-uniform; num_seeds <= min(n, kMaxSeeds): the entry point checks
        for (uint32_t i = threadIdx.x; i < num_seeds; i += kFlat) load_point(pts, seed_site(i, n, num_seeds), s_seeds + 3 * i);
        __syncthreads();
    }
    const uint32_t k = blockIdx.x * kFlat + threadIdx.x;
    if (k >= num_queries) return;
    const float q[3] = {queries[3 * (size_t)k], queries[3 * (size_t)k + 1], queries[3 * (size_t)k + 2]};
    int64_t cell;
    int32_t hops;
    locate_one(pts, n, adj, offsets, num_edges, s_seeds, num_seeds, q, start ? start + k : nullptr, max_hops, cell, hops);
    if (cell < kNoCell) flags[((-2 - cell) & 7) == (int64_t)kHopCap ? 1 : 0] = 1u;
    cell_out[k] = cell;
    hops_out[k] = hops;
}

}  // namespace nearest
}  // namespace rf

using namespace rf;

extern "C" {

int rf_locate_cells(const float *points, uint32_t num_points, const uint32_t *point_adjacency,
                    const uint32_t *point_adjacency_offsets, uint32_t num_edges, const float *queries, const int64_t *start,
                    uint32_t num_seeds, uint32_t num_queries, uint32_t max_hops, int64_t *cell, int32_t *hops,
                    uint32_t *flags, void *stream) {
    g_err[0] = 0;
    if (num_queries == 0) return RF_OK;
    if (!points || !point_adjacency_offsets || !queries || !cell || !hops || !flags || (num_edges && !point_adjacency))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_locate_cells: null pointer");
    if (num_points == 0 || num_points >= 0x80000000u)
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_locate_cells: num_points must be in [1, 2^31)");
    if (num_queries > 0x40000000u) return fail(RF_ERR_INVALID_ARGUMENT, "rf_locate_cells: more than 2^30 queries");
    if (num_seeds > nearest::kMaxSeeds || num_seeds > num_points)
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_locate_cells: num_seeds must be at most min(num_points, 1024)");
    hipLaunchKernelGGL(nearest::locate_cells_kernel<uint32_t>, dim3((num_queries + nearest::kFlat - 1u) / nearest::kFlat),
                       dim3(nearest::kFlat), 0, static_cast<hipStream_t>(stream), points, num_points, point_adjacency,
                       point_adjacency_offsets, num_edges, queries, start, num_seeds, num_queries, max_hops, cell, hops,
                       flags);
    return check_launch("rf_locate_cells");
}

}  // extern "C"
