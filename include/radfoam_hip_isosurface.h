/*
 * radfoam_hip_isosurface.h -- C-ABI of marching tetrahedra on the Delaunay mesh (libradfoam_hip.so, rf_isosurface.hip).
 * Conventions of radfoam_hip_geometry.h: device pointers, `stream` a hipStream_t passed as void*, RF_OK or a negative
 * rf_status, nothing synchronises.
 *
 * A site is inside where values[site] > level (strictly; NaN is outside); a tetrahedron with a value that is not finite
 * emits nothing, one with 1 or 3 corners inside a triangle, one with 2 a quad as two triangles.  A triangle corner lies
 * on a tetrahedron edge between an inside and an outside site a < b and is named by the key a * 2^32 + b; equal keys
 * are one vertex ("Isosurface of an interpolated field").  The caller scans the counts and welds the keys;
 * this interface counts, emits the keys in the final winding, evaluates the vertex of an edge and runs the backward of
 * that.  Every output element is written exactly once by a plain store, there are no atomics, and the outputs are
 * bit-reproducible.
 *
 * tets[T*4]: rows of index_bytes = 4 (uint32, or int32: a negative index is out of range) or 8 (int64) byte indices,
 * 16-byte aligned.  num_points < 2^31, num_tets <= 2^30.
 */
#ifndef RADFOAM_HIP_ISOSURFACE_H
#define RADFOAM_HIP_ISOSURFACE_H

#include "radfoam_hip_geometry.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * counts[T] (uint8): the triangles of every tetrahedron, 0, 1 or 2.  A tetrahedron with an index outside
 * [0, num_points) counts 0 and sets *bad (uint32, zeroed by the caller on the stream beforehand) to 1.
 */
int rf_isosurface_count(const void *tets, uint32_t index_bytes, uint32_t num_tets, const float *values,
                        uint32_t num_points, double level, uint8_t *counts, uint32_t *bad, void *stream);

/*
 * ends[T] (int64): the inclusive running sum of counts, so that tetrahedron t owns triangles
 * [ends[t] - counts[t], ends[t]).  keys[F*3] (int64): the three corner keys of every triangle, wound with the normal
 * from the inside to the outside sites; triangle_tet[F] (int64): its tetrahedron.  A tetrahedron whose range is not
 * within [0, num_triangles) is skipped; one whose count does not match its values any more gets -1 keys.
 */
int rf_isosurface_emit(const void *tets, uint32_t index_bytes, uint32_t num_tets, const float *points, const float *values,
                       uint32_t num_points, double level, const uint8_t *counts, const int64_t *ends,
                       int64_t num_triangles, int64_t *keys, int64_t *triangle_tet, void *stream);

/*
 * vertices[V*3] and vertex_t[V] (double) of the edges vertex_sites[V*2] (int64; a then b):
 * t = (level - v_a) / (v_b - v_a), x = p_a + t (p_b - p_a) in double; NaN where a site is out of range, v_a == v_b or
 * a result is not finite.
 */
int rf_isosurface_vertices(const float *points, const float *values, uint32_t num_points, const int64_t *vertex_sites,
                           uint32_t num_vertices, double level, double *vertices, double *vertex_t, void *stream);

/*
 * The backward of rf_isosurface_vertices for the upstream grad_vertices[V*3] (double): site_grad[V*2*4] (double,
 * scratch the caller owns) takes (grad p, grad v) of a and of b for every vertex (zeros where the vertex is NaN or a
 * term is not finite), and grad_points[N*3], grad_values[N] (double) their sums per site as a gather:
 * incidence_order[2V] (int64) lists the 2V entries of vertex_sites in ascending order of site, ties in ascending order
 * of entry (a stable sort), and site_runs[N+1] (int64) where the run of every site starts in it.  One lane per site adds
 * its run in that order.
 */
int rf_isosurface_vertices_grad(const float *points, const float *values, uint32_t num_points, const int64_t *vertex_sites,
                                uint32_t num_vertices, double level, const double *grad_vertices,
                                const int64_t *incidence_order, const int64_t *site_runs, double *site_grad,
                                double *grad_points, double *grad_values, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RADFOAM_HIP_ISOSURFACE_H */
