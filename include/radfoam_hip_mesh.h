/*
 * radfoam_hip_mesh.h -- C-ABI of the welded surface mesh of selected Voronoi cells (libradfoam_hip.so,
 * rf_cell_mesh.hip).  Conventions of radfoam_hip_geometry.h: device pointers, `stream` a hipStream_t passed as void*,
 * RF_OK or a negative rf_status, nothing synchronises.
 *
 * A corner of the polygon of face (a,b) lies where the planes of two further neighbours c_in and c_out of a's row meet
 * the face: it is the Voronoi vertex of the four sites, and the ascending 4-tuple (a, b, c_in, c_out) is its key.  Equal
 * keys are one vertex ("Welded surface mesh").  The caller welds; this interface emits the corners with
 * their keys, evaluates the vertex of a key as the circumcentre of its four sites, and runs the backward of that.
 * Every output element is written exactly once by a plain store, there are no atomics, and the outputs are
 * bit-reproducible.
 */
#ifndef RADFOAM_HIP_MESH_H
#define RADFOAM_HIP_MESH_H

#include "radfoam_hip_geometry.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a face_status beyond rf_cell_status: the labelled polygon has another vertex count than face_vertices says */
#define RF_FACE_VERTEX_COUNT 3

/* bytes of device workspace rf_cell_mesh_emit needs: a byte per face */
size_t rf_cell_mesh_emit_workspace_bytes(uint32_t num_faces);

/*
 * slots[F] (int64, ascending or not): adjacency slots a -> b whose polygon is wanted; face_vertices[E] what
 * rf_cell_geometry wrote for the same points, adjacency and bbox; corner_begin[F] (int64): where the
 * face_vertices[slots[i]] corners of face i start in corner_xyz[C*3] (double, absolute positions, the arithmetic of
 * rf_cell_surface_emit) and corner_sites[C*4] (uint32 keys, ascending; 0xFFFFFFFF for a corner of the clipping
 * square).  A face is skipped, with face_status[i] = RF_CELL_BAD_ROW, when its slot, its vertex count (< 3) or its
 * corner range [corner_begin[i], + face_vertices) is out of bounds; otherwise exactly its range is written, with NaN /
 * 0xFFFFFFFF when face_status[i] (an rf_cell_status or RF_FACE_VERTEX_COUNT) is not RF_CELL_OK.
 */
int rf_cell_mesh_emit(const float *points, uint32_t num_points, const uint32_t *point_adjacency,
                      const uint32_t *point_adjacency_offsets, uint32_t num_edges, const float *bbox,
                      const uint32_t *face_vertices, const int64_t *slots, const int64_t *corner_begin,
                      uint32_t num_faces, int64_t num_corners, double *corner_xyz, uint32_t *corner_sites,
                      uint8_t *face_status, void *workspace, size_t workspace_bytes, void *stream);

/*
 * vertices[V*3] (double): the circumcentre of points[vertex_sites[v][0..4)] (int64 [V*4]), taken relative to the first
 * site in double; NaN where a site is out of range, the four are exactly coplanar or the result is not finite.
 */
int rf_mesh_vertices(const float *points, uint32_t num_points, const int64_t *vertex_sites, uint32_t num_vertices,
                     double *vertices, void *stream);

/*
 * The backward of rf_mesh_vertices for the upstream grad_vertices[V*3] (double): site_grad[V*4*3] (double, scratch the
 * caller owns) takes the four 3-vectors of every vertex (zeros where the vertex is NaN or a term is not finite), and
 * grad_points[N*3] (double) their sum per site as a gather: incidence_order[4V] (int64) lists the 4V entries of
 * vertex_sites in ascending order of site, ties in ascending order of entry (a stable sort), and site_runs[N+1] (int64)
 * where the run of every site starts in it.  One lane per site adds its run in that order.
 */
int rf_mesh_vertices_grad(const float *points, uint32_t num_points, const int64_t *vertex_sites, uint32_t num_vertices,
                          const double *grad_vertices, const int64_t *incidence_order, const int64_t *site_runs,
                          double *site_grad, double *grad_points, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RADFOAM_HIP_MESH_H */
