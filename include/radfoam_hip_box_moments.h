/*
 * radfoam_hip_box_moments.h -- C-ABI of the second moments of the Voronoi cells clipped to an axis-aligned box
 * (libradfoam_hip.so, rf_cell_box_moments.hip).  Conventions of radfoam_hip_geometry.h: device pointers, `stream` a
 * hipStream_t passed as void*, RF_OK or a negative rf_status, nothing synchronises.
 *
 * cell_box(a) = cell(a) n box, its planes the list of radfoam_hip_box.h: a's adjacency row in row order, then the six
 * walls in wall order.  In y = x - p_a and in double,
 *     site_moment[a]    = int_{cell_box(a)} y y^T dy = sum over the list's planes i of (h_i / 5) int_{F_i} y y^T dA,
 *     central_moment[a] = site_moment[a] - volume[a] m m^T,   m = centroid[a] - p_a,
 * each as six numbers xx, yy, zz, xy, xz, yz ("Second moments of the cells clipped to a box").  h_i is the
 * signed height of plane i over the site, |p_b - p_a| / 2 for a row face and negative for a wall the site is outside of:
 * the signed sum is the moment of cell(a) n box also for a site outside the box.  The box is six doubles passed BY VALUE;
 * it must be finite with lo < hi in every axis and need not contain the points.  `bbox` is as for rf_cell_box.
 */
#ifndef RADFOAM_HIP_BOX_MOMENTS_H
#define RADFOAM_HIP_BOX_MOMENTS_H

#include "radfoam_hip_geometry.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of device workspace rf_cell_box_moments needs for num_points cells */
size_t rf_cell_box_moments_workspace_bytes(uint32_t num_points);

/*
 * volume[N], centroid[N*3], nonempty[N]: what rf_cell_box wrote for the same points, adjacency, bbox and box.
 * site_moment[N*6], central_moment[N*6] (double) and cell_status[N] (an rf_cell_status) are each written exactly once by
 * plain stores: the output is bit-reproducible.  Every cell has a finite site_moment, exactly 0 in all six where the
 * intersection is exactly empty; central_moment is NaN where nonempty[a] == 0.  A cell with an empty row is the whole box,
 * in closed form.  A cell whose status is not RF_CELL_OK (a malformed row, or a face of more than 256 vertices) gets
 * twelve NaN.
 */
int rf_cell_box_moments(const float *points, uint32_t num_points, const uint32_t *point_adjacency,
                        const uint32_t *point_adjacency_offsets, uint32_t num_edges, const float *bbox, double lo_x,
                        double lo_y, double lo_z, double hi_x, double hi_y, double hi_z, const double *volume,
                        const double *centroid, const uint8_t *nonempty, double *site_moment, double *central_moment,
                        uint8_t *cell_status, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RADFOAM_HIP_BOX_MOMENTS_H */
