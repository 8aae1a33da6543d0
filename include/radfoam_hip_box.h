/*
 * radfoam_hip_box.h -- C-ABI of the Voronoi cells clipped to an axis-aligned box (libradfoam_hip.so, rf_cell_box.hip).
 * Conventions of radfoam_hip_geometry.h: device pointers, `stream` a hipStream_t passed as void*, RF_OK or a negative
 * rf_status, nothing synchronises.
 *
 * cell_box(a) = cell(a) n box: the planes of a's adjacency row, in row order, followed by the six walls of the box in wall
 * order, wall 2k being x_k >= lo_k and wall 2k+1 x_k <= hi_k ("Cells clipped to a box").  Every cell is a
 * bounded polytope and every output is finite, except the centroid of an empty cell.  The box is six doubles passed BY
 * VALUE; it must be finite with lo < hi in every axis and need not contain the points.  `bbox` is min[3], max[3] of all
 * points as 6 floats on the device, as for rf_cell_geometry: the clipping square's half-side is 4 * |diagonal of the
 * bounding box of the points and the box together|.
 */
#ifndef RADFOAM_HIP_BOX_H
#define RADFOAM_HIP_BOX_H

#include "radfoam_hip_geometry.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of device workspace rf_cell_box needs for num_points cells */
size_t rf_cell_box_workspace_bytes(uint32_t num_points);

/*
 * volume[N] (the signed pyramid sum: >= 0 up to rounding), centroid[N*3] (NaN where volume <= 0), nonempty[N] (volume > 0),
 * face_area[E] and face_vertices[E] (the part of face (a,b) inside the box and its polygon's vertex count, aligned with
 * point_adjacency), wall_area[N*6] and wall_vertices[N*6] (the part of each wall that bounds the cell, in wall order);
 * cell_status[N] holds an rf_cell_status per cell, and the outputs of a cell whose status is not RF_CELL_OK are NaN / 0.
 * A cell with an empty row is the whole box.  Every element is written exactly once by a plain store: the output is
 * bit-reproducible.
 */
int rf_cell_box(const float *points, uint32_t num_points, const uint32_t *point_adjacency,
                const uint32_t *point_adjacency_offsets, uint32_t num_edges, const float *bbox, double lo_x, double lo_y,
                double lo_z, double hi_x, double hi_y, double hi_z, double *volume, double *centroid, uint8_t *nonempty,
                double *face_area, uint32_t *face_vertices, double *wall_area, uint32_t *wall_vertices,
                uint8_t *cell_status, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RADFOAM_HIP_BOX_H */
