/*
 * radfoam_hip_box_area_grad.h -- C-ABI of the point gradients of the face and wall areas of the Voronoi cells clipped to
 * an axis-aligned box (libradfoam_hip.so, rf_cell_box_area_grad.hip).  Conventions of radfoam_hip_geometry.h: device
 * pointers, `stream` a hipStream_t passed as void*, RF_OK or a negative rf_status, nothing synchronises.
 *
 * For L = sum_s grad_face_area[s] * face_area[s] + sum_{a,w} grad_wall_area[a,w] * wall_area[a,w] of rf_cell_box, each
 * upstream counted where that slot's or wall's own forward area is > 0, grad_points[a] sums over the edges of the row
 * faces of cell a inside the box: a Voronoi edge (a,b,c) adds  l (lambda_b + lambda_c) (y - p_a)  as in
 * radfoam_hip_face_area_grad.h with the segment as the box clipped it, and the trace of the bisector of (a,b) in wall w
 * adds  (l (y - p_a) / |d_b|) [ -G_ab cot t + (gw[a,w] - gw[b,w]) / sin t ],  cos t = n_w . d_b / |d_b|  (DESIGN.md,
 * "Point gradients of the face and wall areas in a box").  The box is fixed.  A gather over a's own row with look-ups in
 * the neighbours' rows: exact for a symmetric adjacency; a missing mate slot or slot b->c weighs 0.  The box and `bbox`
 * are those of rf_cell_box.
 */
#ifndef RADFOAM_HIP_BOX_AREA_GRAD_H
#define RADFOAM_HIP_BOX_AREA_GRAD_H

#include "radfoam_hip_box.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of device workspace rf_cell_box_area_grad needs for num_points cells and num_edges adjacency slots */
size_t rf_cell_box_area_grad_workspace_bytes(uint32_t num_points, uint32_t num_edges);

/*
 * volume[N], centroid[N*3], nonempty[N], face_area[E], wall_area[N*6]: what rf_cell_box wrote for the same points,
 * adjacency, bbox and box (volume and centroid are not read).  grad_face_area[E] and grad_wall_area[N*6] (double) may
 * each be NULL (zero); an entry whose own forward area is exactly 0 is never read.  grad_points[N*3] (double) and
 * cell_status[N] (an rf_cell_status; the row is NaN unless RF_CELL_OK) are each written exactly once by plain stores:
 * the output is bit-reproducible.  A cell with an empty row, and an empty cell, get a zero row.
 */
int rf_cell_box_area_grad(const float *points, uint32_t num_points, const uint32_t *point_adjacency,
                          const uint32_t *point_adjacency_offsets, uint32_t num_edges, const float *bbox, double lo_x,
                          double lo_y, double lo_z, double hi_x, double hi_y, double hi_z, const double *volume,
                          const double *centroid, const uint8_t *nonempty, const double *face_area,
                          const double *wall_area, const double *grad_face_area, const double *grad_wall_area,
                          double *grad_points, uint8_t *cell_status, void *workspace, size_t workspace_bytes,
                          void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RADFOAM_HIP_BOX_AREA_GRAD_H */
