/*
 * radfoam_hip_nearest.h -- C-ABI of cell location: the Voronoi cell (the nearest site) of any point, by a greedy walk over
 * the neighbour lists (libradfoam_hip.so, rf_nearest.hip).  Conventions of radfoam_hip_geometry.h: device pointers,
 * `stream` a hipStream_t passed as void*, RF_OK or a negative rf_status, nothing synchronises.
 *
 * The definitions (the exact closer predicate, the key, the step, the seeds, the faults) are those of
 * csrc/rf_nearest.hpp ("Cell location").  Every output element is written by plain stores of one lane, there
 * are no atomics, and the outputs are bit-reproducible.
 *
 * point_adjacency[E] and point_adjacency_offsets[N+1] as rf_cell_geometry takes them: 4-byte words (uint32, or int32: a
 * negative word is out of range), row i at point_adjacency[offsets[i] .. offsets[i+1]).  1 <= num_points < 2^31,
 * num_queries <= 2^30.
 */
#ifndef RADFOAM_HIP_NEAREST_H
#define RADFOAM_HIP_NEAREST_H

#include "radfoam_hip_geometry.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * cell[Q] (int64) and hops[Q] (int32) of queries[Q*3] (float): from site start[q] (int64), or with start NULL from the
 * nearest of num_seeds <= min(num_points, 1024) seed sites (seed i is site floor(i * num_points / num_seeds)), or with
 * num_seeds 0 from site 0, the walk steps to the entry of the site's row with the smallest key (exact squared distance,
 * index) for as long as that key is below the site's own.  cell >= 0: no entry of the cell's row is nearer to the query;
 * on the neighbour lists of a Delaunay triangulation of the points, no site is.  -1: a coordinate of the query is not
 * finite (0 hops).  Below -1: the fault code -2 - (kind + 8 * site), kind 0 a start outside [0, num_points), 1 a row whose
 * bounds run backwards or past num_edges, 2 a list entry outside [0, num_points), 3 a walk that would take more than
 * max_hops steps.  flags[2] (uint32, zeroed by the caller on the stream beforehand): flags[0] becomes 1 with a fault of
 * kind 0..2, flags[1] with one of kind 3 (plain stores of one value).
 */
int rf_locate_cells(const float *points, uint32_t num_points, const uint32_t *point_adjacency,
                    const uint32_t *point_adjacency_offsets, uint32_t num_edges, const float *queries, const int64_t *start,
                    uint32_t num_seeds, uint32_t num_queries, uint32_t max_hops, int64_t *cell, int32_t *hops,
                    uint32_t *flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RADFOAM_HIP_NEAREST_H */
