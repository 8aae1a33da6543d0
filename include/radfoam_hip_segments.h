/*
 * radfoam_hip_segments.h -- C-ABI of the walk export (libradfoam_hip.so, rf_segments.hip): the cells every ray
 * scans, in order, with the ray parameters at which it enters and leaves each.
 *
 * Conventions of radfoam_hip.h: every pointer is a DEVICE pointer, `stream` is a hipStream_t passed as void*, every
 * function returns RF_OK or a negative rf_status and leaves a message for rf_last_error.  Nothing synchronises.
 *
 * Both functions read the PREPARED workspace of rf_prepare_foam (any sh_degree / attr_type: the part of the layout
 * they read -- cell records, fp16 face blocks, links, padded offsets -- depends on num_points and
 * point_adjacency_size alone) and walk exactly as rf_trace_forward does with the same settings: the reference's scan
 * (every face divided, smallest rounded quotient, lowest index among equals), the same transmittance test, the same
 * step limit.  Only the density of a cell is read, never its colour row.
 *
 * The result is a ragged list in CSR form, filled in two passes with a prefix sum by the caller in between:
 *   1. rf_trace_segments_count: counts[r] = entries of ray r = min(num_intersections[r], settings->max_intersections)
 *   2. the caller forms offsets[0] = 0, offsets[r + 1] = offsets[r] + counts[r]  (int64) and allocates offsets[R] entries
 *   3. rf_trace_segments_fill: entry offsets[r] + k is step k of ray r
 *        cells    the cell scanned (entry 0: start_point_index[r])
 *        t_exit   where the walk leaves it; +inf when the cell has no exit (the walk ends there)
 *        t_enter  the t0 the compositing used: 0 for entry 0, then the running maximum of the earlier t_exit
 * A ray whose start_point_index is not below num_points has no entries and num_intersections 0.
 */
#ifndef RADFOAM_HIP_SEGMENTS_H
#define RADFOAM_HIP_SEGMENTS_H

#include "radfoam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* counts[num_rays] (uint32); num_intersections[num_rays] (uint32, optional): what rf_trace_forward reports */
int rf_trace_segments_count(const rf_trace_settings *settings, uint32_t num_points, uint32_t point_adjacency_size,
                            const void *workspace, uint32_t num_rays, const float *rays,
                            const uint32_t *start_point_index, uint32_t *counts, uint32_t *num_intersections,
                            void *stream);

/* offsets[num_rays + 1] (int64) as described above; cells / t_enter / t_exit hold offsets[num_rays] entries each.
 * A ray never writes outside offsets[r] .. offsets[r + 1]. */
int rf_trace_segments_fill(const rf_trace_settings *settings, uint32_t num_points, uint32_t point_adjacency_size,
                           const void *workspace, uint32_t num_rays, const float *rays,
                           const uint32_t *start_point_index, const int64_t *offsets, uint32_t *cells, float *t_enter,
                           float *t_exit, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RADFOAM_HIP_SEGMENTS_H */
