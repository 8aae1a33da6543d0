/*
 * radfoam_hip_moments_grad.h -- C-ABI of the point gradients of the second moments of the Voronoi cells
 * (libradfoam_hip.so, rf_cell_moments_grad.hip).  Conventions of radfoam_hip_geometry_grad.h: device pointers, `stream`
 * a hipStream_t passed as void*, RF_OK or a negative rf_status, nothing synchronises.
 *
 * Six upstream numbers g = (xx, yy, zz, xy, xz, yz) stand for the symmetric matrix S(g) with the diagonal as it is and
 * half of each off-diagonal number on both sides, so that <S(g), Q> = sum_k g[k] Q[k] over the six stored numbers.  For
 * L = sum_a <grad_site_moment[a], site_moment[a]> + <grad_central_moment[a], central_moment[a]> over the bounded cells,
 *     grad_points[a] = sum_{b in row a} (1 / |p_b - p_a|) int_{F_ab} (Psi_a(x) - Psi_b(x)) (x - p_a) dA
 *                      - 2 volume[a] G_a (centroid[a] - p_a),
 *     Psi_a(x) = (x - p_a)^T G_a (x - p_a) + (x - centroid[a])^T H_a (x - centroid[a]),   Psi_a == 0 if !bounded[a]
 * with G_a = S(grad_site_moment[a]), H_a = S(grad_central_moment[a]); the last term only if bounded[a] (DESIGN.md,
 * "Point gradients of the second moments").  A gather over a's own row: exact for a symmetric adjacency; the term of a
 * site that lists a but is missing from a's row is dropped.
 */
#ifndef RADFOAM_HIP_MOMENTS_GRAD_H
#define RADFOAM_HIP_MOMENTS_GRAD_H

#include "radfoam_hip_geometry.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of device workspace rf_cell_moments_grad needs for num_points cells */
size_t rf_cell_moments_grad_workspace_bytes(uint32_t num_points);

/*
 * volume[N], centroid[N*3], bounded[N]: what rf_cell_geometry wrote for the same points, adjacency and bbox.
 * grad_site_moment[N*6] and grad_central_moment[N*6] (double) may each be NULL (zero); their entries for unbounded cells
 * are never read.  grad_points[N*3] (double) and cell_status[N] (an rf_cell_status; the row is NaN unless RF_CELL_OK)
 * are each written exactly once by plain stores: the output is bit-reproducible.
 */
int rf_cell_moments_grad(const float *points, uint32_t num_points, const uint32_t *point_adjacency,
                         const uint32_t *point_adjacency_offsets, uint32_t num_edges, const float *bbox,
                         const double *volume, const double *centroid, const uint8_t *bounded,
                         const double *grad_site_moment, const double *grad_central_moment, double *grad_points,
                         uint8_t *cell_status, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RADFOAM_HIP_MOMENTS_GRAD_H */
