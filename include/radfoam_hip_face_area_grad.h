/*
 * radfoam_hip_face_area_grad.h -- C-ABI of the point gradients of the Voronoi face areas (libradfoam_hip.so,
 * rf_face_area_grad.hip).  Conventions of radfoam_hip_geometry.h: device pointers, `stream` a hipStream_t passed as
 * void*, RF_OK or a negative rf_status, nothing synchronises.
 *
 * For L = sum over the adjacency slots s of grad_face_area[s] * face_area[s], the slots of finite positive area only
 * (what arrives for a slot of area +inf, or of area exactly 0, is never read), face {a,b} has the effective weight
 * G_ab = g^[a->b] + g^[b->a] and every finite Voronoi edge e (length l, midpoint y) of row a, dual to the Delaunay
 * triangle (a,b,c), adds
 *     grad_points[a] += l (lambda_b + lambda_c) (y - p_a),
 *     lambda_b + lambda_c = [ -G_ab d_b.e_bc / |d_b| + G_ac d_c.e_bc / |d_c| - G_bc |e_bc| ] / |d_b x d_c|,
 * d_b = p_b - p_a, d_c = p_c - p_a, e_bc = d_c - d_b ("Point gradients of the face areas").  A gather over
 * a's own row plus one search of the row of b per face: exact for a symmetric adjacency; a mate slot or a slot b->c that
 * does not exist has weight 0.
 */
#ifndef RADFOAM_HIP_FACE_AREA_GRAD_H
#define RADFOAM_HIP_FACE_AREA_GRAD_H

#include "radfoam_hip_geometry.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of device workspace rf_face_area_grad needs: a byte per cell and the f64[E] effective weights */
size_t rf_face_area_grad_workspace_bytes(uint32_t num_points, uint32_t num_edges);

/*
 * face_area[E]: what rf_cell_geometry wrote for the same points, adjacency and bbox.  grad_face_area[E] (double) is
 * aligned with it.  grad_points[N*3] (double) and cell_status[N] (an rf_cell_status; the row is NaN unless RF_CELL_OK)
 * are each written exactly once by plain stores, and there are no atomics: the output is bit-reproducible.
 */
int rf_face_area_grad(const float *points, uint32_t num_points, const uint32_t *point_adjacency,
                      const uint32_t *point_adjacency_offsets, uint32_t num_edges, const float *bbox,
                      const double *face_area, const double *grad_face_area, double *grad_points, uint8_t *cell_status,
                      void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RADFOAM_HIP_FACE_AREA_GRAD_H */
