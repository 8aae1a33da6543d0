/*
 * radfoam_hip_box_grad.h -- C-ABI of the point gradients of the Voronoi cells clipped to an axis-aligned box
 * (libradfoam_hip.so, rf_cell_box_grad.hip).  Conventions of radfoam_hip_geometry.h: device pointers, `stream` a
 * hipStream_t passed as void*, RF_OK or a negative rf_status, nothing synchronises.
 *
 * For L = sum_a grad_volume[a] * volume[a] + grad_centroid[a] . centroid[a] over the non-empty cells of rf_cell_box,
 *     grad_points[a] = sum_{b in row a} (1 / |p_b - p_a|) int_{F_ab n box} (phi_a(x) - phi_b(x)) (x - p_a) dA,
 *     phi_a(x) = grad_volume[a] + (grad_centroid[a] / volume[a]) . (x - centroid[a]),   phi_a == 0 if !nonempty[a]
 * ("Point gradients of the cells in a box").  The box is fixed: its walls carry no term and clip the row's
 * faces exactly as in rf_cell_box (the same plane list, half-side and tie rule).  A gather over a's own row: exact for a
 * symmetric adjacency; the term of a site that lists a but is missing from a's row is dropped.  The box and `bbox` are
 * those of rf_cell_box.
 */
#ifndef RADFOAM_HIP_BOX_GRAD_H
#define RADFOAM_HIP_BOX_GRAD_H

#include "radfoam_hip_box.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of device workspace rf_cell_box_grad needs for num_points cells */
size_t rf_cell_box_grad_workspace_bytes(uint32_t num_points);

/*
 * volume[N], centroid[N*3], nonempty[N]: what rf_cell_box wrote for the same points, adjacency, bbox and box.
 * grad_volume[N] and grad_centroid[N*3] (double) may each be NULL (zero); their entries for empty cells, and the
 * centroids of empty cells, are never read.  grad_points[N*3] (double) and cell_status[N] (an rf_cell_status; the row is
 * NaN unless RF_CELL_OK) are each written exactly once by plain stores: the output is bit-reproducible.  A cell with an
 * empty row gets a zero row.
 */
int rf_cell_box_grad(const float *points, uint32_t num_points, const uint32_t *point_adjacency,
                     const uint32_t *point_adjacency_offsets, uint32_t num_edges, const float *bbox, double lo_x,
                     double lo_y, double lo_z, double hi_x, double hi_y, double hi_z, const double *volume,
                     const double *centroid, const uint8_t *nonempty, const double *grad_volume,
                     const double *grad_centroid, double *grad_points, uint8_t *cell_status, void *workspace,
                     size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RADFOAM_HIP_BOX_GRAD_H */
