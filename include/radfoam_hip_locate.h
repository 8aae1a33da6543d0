/*
 * radfoam_hip_locate.h -- C-ABI of point location and interpolation on the Delaunay mesh (libradfoam_hip.so,
 * rf_locate.hip).  Conventions of radfoam_hip_geometry.h: device pointers, `stream` a hipStream_t passed as void*, RF_OK
 * or a negative rf_status, nothing synchronises.
 *
 * The definitions (face signs, the step, the faults, the order of the interpolation's operations and its backward) are
 * those of csrc/rf_locate.hpp ("Point location and interpolation").  Every output element is written by plain
 * stores of one lane, there are no atomics, and the outputs are bit-reproducible.
 *
 * tets[T*4] and tet_adjacency[T*4]: rows of index_bytes = 4 (uint32, or int32: a negative index is out of range and
 * -1 is the hull word) or 8 (int64; the hull word is -1 or 0xFFFFFFFF) byte words, both of the same width, 16-byte
 * aligned.  num_points < 2^31, num_tets < 2^30, num_queries <= 2^30.
 */
#ifndef RADFOAM_HIP_LOCATE_H
#define RADFOAM_HIP_LOCATE_H

#include "radfoam_hip_geometry.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * tet[Q] (int64) and hops[Q] (int32) of queries[Q*3] (float): the walk from row start[q] (int64; NULL: row 0) over
 * tet_adjacency with exact face signs.  tet >= 0: the closed tetrahedron holds the query; -1: outside the hull, or a
 * coordinate that is not finite (0 hops); below -1: the fault code -2 - (kind + 8 * row), kind 0 a corner outside
 * [0, num_points), 1 an adjacency entry that is neither the hull word nor below 4T, 2 a flat row, 3 a start outside
 * [0, T), 4 a walk that would cross more than max_hops faces.  flags[2] (uint32, zeroed by the caller on the stream
 * beforehand): flags[0] becomes 1 with a fault of kind 0..3, flags[1] with one of kind 4 (plain stores of one value).
 */
int rf_locate_walk(const float *points, uint32_t num_points, const void *tets, const void *tet_adjacency,
                   uint32_t index_bytes, uint32_t num_tets, const float *queries, const int64_t *start,
                   uint32_t num_queries, uint32_t max_hops, int64_t *tet, int32_t *hops, uint32_t *flags, void *stream);

/*
 * value[Q*C], weights[Q*4], gradient[Q*C*3] (double) of the field values[N*C] (float), C = channels in 1..8, at the
 * queries, each in the tetrahedron tet[Q] (int64) names.  NaN in all three where tet is outside [0, T), a corner is out
 * of range, the determinant is zero or a result is not finite.
 */
int rf_interpolate(const float *points, uint32_t num_points, const void *tets, uint32_t index_bytes, uint32_t num_tets,
                   const float *values, uint32_t channels, const float *queries, const int64_t *tet, uint32_t num_queries,
                   double *value, double *weights, double *gradient, void *stream);

/*
 * The backward of value for the upstream grad_value[Q*C] (double): parts[Q*4*(3+C)] (double, scratch the caller owns)
 * takes (grad p, grad v[C]) of the four corners of every query (zeros where the forward is NaN or a term is not finite),
 * grad_queries[Q*3] the gradient of every query, and grad_points[N*3], grad_values[N*C] (double) the parts' sums per
 * site as a gather: incidence_order[4Q] (int64) lists the 4Q corners (4 q + corner) in ascending order of site, ties in
 * ascending order of corner entry (a stable sort; corners without a site sorted behind all sites), and site_runs[N+1]
 * (int64) where the run of every site starts in it.  One lane per site adds its run in that order.
 */
int rf_interpolate_grad(const float *points, uint32_t num_points, const void *tets, uint32_t index_bytes, uint32_t num_tets,
                        const float *values, uint32_t channels, const float *queries, const int64_t *tet,
                        uint32_t num_queries, const double *grad_value, const int64_t *incidence_order,
                        const int64_t *site_runs, double *parts, double *grad_points, double *grad_values,
                        double *grad_queries, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RADFOAM_HIP_LOCATE_H */
