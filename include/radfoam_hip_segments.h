/*
 * radfoam_hip_segments.h -- C-ABI of the walk export (libradfoam_hip.so, rf_segments.hip): the cells every ray
 * scans, in order, with the ray parameters at which it enters and leaves each, and of its
 * gradient with respect to the points (rf_segments_grad.hip, section 4.9) and to the rays (rf_segments_rays_grad.hip,
 * section 4.10).
 *
 * Conventions of radfoam_hip.h: every pointer is a DEVICE pointer, `stream` is a hipStream_t passed as void*, every
 * function returns RF_OK or a negative rf_status and leaves a message for rf_last_error.  Nothing synchronises.
 *
 * The walk functions read the PREPARED workspace of rf_prepare_foam (any sh_degree / attr_type: the part of the layout
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

/* The cell behind every ray's last face: exit_cells[num_rays] (uint32).  One lane per ray scans
 * the cell of the ray's last entry again over the same prepared workspace, exactly as the walk did, and follows the
 * winner's link.  0xFFFFFFFF where the ray has no entries or the t_exit of its last entry is +inf.  offsets / cells /
 * t_exit are what rf_trace_segments_fill wrote for the same rays and workspace. */
int rf_trace_segments_exit_cells(uint32_t num_points, uint32_t point_adjacency_size, const void *workspace,
                                 uint32_t num_rays, const float *rays, const int64_t *offsets, const uint32_t *cells,
                                 const float *t_exit, uint32_t *exit_cells, void *stream);

/* Gradient of a loss with respect to the points through the stored t_enter / t_exit (rf_segments_grad.hip; DESIGN.md
 * section 4.9).  Face j lies between a = cells[j] and b = the next cell of the walk (cells[j + 1] inside the ray's
 * range, exit_cells[r] behind the ray's last entry, none where t_exit[j] is +inf or exit_cells[r] is 0xFFFFFFFF);
 * entry j HOLDS the running maximum iff t_exit[j] > t_enter[j];
 *     G_j = grad_t_exit[j] + [j holds] * (sum of grad_t_enter[m] over the ray's entries after j, up to and including
 *           the next holder)
 *     points_grad[a] += G_j dt/dp_a,  points_grad[b] += G_j dt/dp_b     (nothing where G_j == 0 exactly)
 * with the derivatives of the exact fp32 bisector of (p_a, p_b), as rf_trace_backward forms them.  One lane per entry:
 * entry_ray[num_entries] (int32) names the ray of every entry; num_entries = offsets[num_rays].  points_grad
 * [num_points][3] (fp32) is ACCUMULATED into with atomics: the caller zeroes it.  The rays' gradient is
 * rf_segments_rays_grad's. */
int rf_segments_points_grad(uint32_t num_points, const float *points, uint32_t num_rays, const float *rays,
                            const int64_t *offsets, int64_t num_entries, const int32_t *entry_ray,
                            const uint32_t *cells, const float *t_enter, const float *t_exit,
                            const uint32_t *exit_cells, const float *grad_t_enter, const float *grad_t_exit,
                            float *points_grad, void *stream);

/* Gradient of the same loss with respect to the RAYS (rf_segments_rays_grad.hip).  Arguments,
 * faces, holders and G_j as above; with n = p_b - p_a, m = (p_a + p_b) / 2, O / D the ray's origin / stored direction,
 * d = D / |D|, num = (m - O) . n and dp = n . d (the crossing is t = num / dp; the cell sequence is held fixed):
 *     ray_grad[r][0:3] += sum over the ray's entries of G_j * (-n / dp)
 *     ray_grad[r][3:6] += sum over the ray's entries of G_j * (-num / (dp^2 |D|)) * (n - dp d)
 * Nothing where G_j == 0 exactly or the face has no next cell; dp = 0 gives non-finite values in that ray's row only.
 * One lane per entry; a ray's contributions are summed in double within the wave and its row gets at most one atomic
 * update per wave the ray reaches into.  Entries whose entry_ray is out of range or does not match the offsets add
 * nothing.  ray_grad [num_rays][6] (fp32) is ACCUMULATED into: the caller zeroes it. */
int rf_segments_rays_grad(uint32_t num_points, const float *points, uint32_t num_rays, const float *rays,
                          const int64_t *offsets, int64_t num_entries, const int32_t *entry_ray, const uint32_t *cells,
                          const float *t_enter, const float *t_exit, const uint32_t *exit_cells,
                          const float *grad_t_enter, const float *grad_t_exit, float *ray_grad, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RADFOAM_HIP_SEGMENTS_H */
