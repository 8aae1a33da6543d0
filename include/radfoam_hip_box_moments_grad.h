/*
 * radfoam_hip_box_moments_grad.h -- C-ABI of the point gradients of the second moments of the Voronoi cells clipped to an
 * axis-aligned box, fused with those of their volumes and centroids (libradfoam_hip.so, rf_cell_box_moments_grad.hip).
 * Conventions of radfoam_hip_box_grad.h: device pointers, `stream` a hipStream_t passed as void*, RF_OK or a negative
 * rf_status, nullable upstreams, nothing synchronises.
 *
 * For L = sum_a <S(grad_site_moment[a]), site_moment[a]> + <S(grad_central_moment[a]), central_moment[a]>
 *           + grad_volume[a] * volume[a] + grad_centroid[a] . centroid[a]   over the non-empty cells of rf_cell_box,
 * each bracket the plain sum over the six stored numbers (xx, yy, zz, xy, xz, yz),
 *     grad_points[a] = sum_{b in row a} (1 / |p_b - p_a|) int_{F_ab n box} (Psi_a(x) - Psi_b(x)) (x - p_a) dA
 *                      - 2 volume[a] G_a (centroid[a] - p_a),
 *     Psi_a(x) = (x - p_a)^T G_a (x - p_a) + (x - c_a)^T H_a (x - c_a) + grad_volume[a]
 *                + (grad_centroid[a] / volume[a]) . (x - c_a),          Psi_a == 0 if !nonempty[a]
 * ("Point gradients of the second moments in a box").  The box is fixed: its walls carry no term and clip the
 * row's faces exactly as in rf_cell_box (the same plane list, half-side and tie rule).  A gather over a's own row: exact
 * for a symmetric adjacency; the term of a site that lists a but is missing from a's row is dropped.  The box and `bbox`
 * are those of rf_cell_box.
 */
#ifndef RADFOAM_HIP_BOX_MOMENTS_GRAD_H
#define RADFOAM_HIP_BOX_MOMENTS_GRAD_H

#include "radfoam_hip_box.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of device workspace rf_cell_box_moments_grad needs for num_points cells */
size_t rf_cell_box_moments_grad_workspace_bytes(uint32_t num_points);

/*
 * volume[N], centroid[N*3], nonempty[N]: what rf_cell_box wrote for the same points, adjacency, bbox and box.
 * grad_site_moment[N*6], grad_central_moment[N*6], grad_volume[N] and grad_centroid[N*3] (double) may each be NULL
 * (zero); their entries for empty cells, and the centroids of empty cells, are never read.  grad_points[N*3] (double) and
 * cell_status[N] (an rf_cell_status; the row is NaN unless RF_CELL_OK) are each written exactly once by plain stores: the
 * output is bit-reproducible.  An empty cell gets a zero row; a non-empty cell with an empty row is the whole box and
 * gets the direct term of its site moment alone.
 */
int rf_cell_box_moments_grad(const float *points, uint32_t num_points, const uint32_t *point_adjacency,
                             const uint32_t *point_adjacency_offsets, uint32_t num_edges, const float *bbox, double lo_x,
                             double lo_y, double lo_z, double hi_x, double hi_y, double hi_z, const double *volume,
                             const double *centroid, const uint8_t *nonempty, const double *grad_site_moment,
                             const double *grad_central_moment, const double *grad_volume, const double *grad_centroid,
                             double *grad_points, uint8_t *cell_status, void *workspace, size_t workspace_bytes,
                             void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RADFOAM_HIP_BOX_MOMENTS_GRAD_H */
