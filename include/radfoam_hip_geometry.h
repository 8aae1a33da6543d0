/*
 * radfoam_hip_geometry.h -- C-ABI of the Voronoi cell geometry (libradfoam_hip.so, rf_cell_geometry.hip).
 *
 * Conventions of radfoam_hip.h: every pointer is a DEVICE pointer, `stream` is a hipStream_t passed as void*, every
 * function returns RF_OK or a negative rf_status and leaves a message for rf_last_error.  Nothing synchronises.
 *
 * Cell a is the intersection of the half-spaces of its adjacency row ("Cell geometry").  `bbox` is
 * min[3], max[3] of all points as 6 floats ON THE DEVICE: the clipping square's half-side is 4 * |bbox diagonal|.
 */
#ifndef RADFOAM_HIP_GEOMETRY_H
#define RADFOAM_HIP_GEOMETRY_H

#include "radfoam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* per-cell status written by rf_cell_geometry */
typedef enum rf_cell_status {
    RF_CELL_OK = 0,
    RF_CELL_TOO_MANY_VERTICES = 1, /* a face outgrew 256 vertices while it was clipped: outputs of the cell are NaN */
    RF_CELL_BAD_ROW = 2            /* offsets out of order, an index >= num_points, the site itself or a duplicate   */
} rf_cell_status;

/* bytes of device workspace rf_cell_geometry needs for num_points cells */
size_t rf_cell_geometry_workspace_bytes(uint32_t num_points);

/*
 * volume[N], centroid[N*3] (double), bounded[N] (0/1), face_area[E] (double) and face_vertices[E] (vertex count of the
 * face polygon), the last two aligned with point_adjacency; cell_status[N] holds an rf_cell_status per cell.
 * Unbounded cells: volume +inf, centroid NaN, bounded 0; unbounded faces: area +inf.  Every element is written once.
 */
int rf_cell_geometry(const float *points, uint32_t num_points, const uint32_t *point_adjacency,
                     const uint32_t *point_adjacency_offsets, uint32_t num_edges, const float *bbox, double *volume,
                     double *centroid, uint8_t *bounded, double *face_area, uint32_t *face_vertices,
                     uint8_t *cell_status, void *workspace, size_t workspace_bytes, void *stream);

/*
 * triangle_count[e] = face_vertices[e] - 2 for an adjacency slot e = (a -> b) with inside[a] && !inside[b], else 0.
 */
int rf_cell_surface_count(uint32_t num_points, const uint32_t *point_adjacency,
                          const uint32_t *point_adjacency_offsets, uint32_t num_edges, const uint8_t *inside,
                          const uint32_t *face_vertices, int32_t *triangle_count, void *stream);

/*
 * The faces of the num_slots adjacency slots listed in `slots` (ascending), each as a triangle fan wound so that the
 * normal points from a to b: triangles[(triangle_begin[i] + k) * 9 ..] for k < face_vertices[slots[i]] - 2, and
 * triangle_slot[...] = slots[i].  triangle_begin is the exclusive prefix sum of the counts of the listed slots.
 */
int rf_cell_surface_emit(const float *points, uint32_t num_points, const uint32_t *point_adjacency,
                         const uint32_t *point_adjacency_offsets, uint32_t num_edges, const float *bbox,
                         const uint32_t *face_vertices, const int64_t *slots, const int64_t *triangle_begin,
                         uint32_t num_slots, double *triangles, int64_t *triangle_slot, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RADFOAM_HIP_GEOMETRY_H */
