/*
 * radfoam_hip_moments.h -- C-ABI of the second moments of the Voronoi cells (libradfoam_hip.so, rf_cell_moments.hip).
 * Conventions of radfoam_hip_geometry.h: device pointers, `stream` a hipStream_t passed as void*, RF_OK or a negative
 * rf_status, nothing synchronises.
 *
 * In y = x - p_a and in double,
 *     site_moment[a]    = int_{cell a} y y^T dy = sum_{b in row a} (|p_b - p_a| / 10) int_{F_ab} y y^T dA,
 *     central_moment[a] = site_moment[a] - volume[a] m m^T,   m = centroid[a] - p_a,
 * each as six numbers xx, yy, zz, xy, xz, yz ("Second moments of the cells").  The trace of site_moment is the
 * cell's centroidal-Voronoi energy int |x - p_a|^2 dx; central_moment / volume is the covariance of the uniform
 * distribution on the cell.  A gather over a's own row.
 */
#ifndef RADFOAM_HIP_MOMENTS_H
#define RADFOAM_HIP_MOMENTS_H

#include "radfoam_hip_geometry.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of device workspace rf_cell_moments needs for num_points cells */
size_t rf_cell_moments_workspace_bytes(uint32_t num_points);

/*
 * volume[N], centroid[N*3], bounded[N]: what rf_cell_geometry wrote for the same points, adjacency and bbox.
 * site_moment[N*6], central_moment[N*6] (double) and cell_status[N] (an rf_cell_status) are each written exactly once by
 * plain stores: the output is bit-reproducible.  A cell with bounded[a] == 0 or an empty row gets twelve NaN and none of
 * its faces is clipped; so does a cell whose status is not RF_CELL_OK (a malformed row, bounded or not, or a face of
 * more than 256 vertices).
 */
int rf_cell_moments(const float *points, uint32_t num_points, const uint32_t *point_adjacency,
                    const uint32_t *point_adjacency_offsets, uint32_t num_edges, const float *bbox,
                    const double *volume, const double *centroid, const uint8_t *bounded, double *site_moment,
                    double *central_moment, uint8_t *cell_status, void *workspace, size_t workspace_bytes,
                    void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RADFOAM_HIP_MOMENTS_H */
