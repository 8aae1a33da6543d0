/*
 * radfoam_hip_tets.h -- C-ABI of the Delaunay tetrahedra read back off the neighbour lists (libradfoam_hip.so,
 * rf_tets.hip).  Conventions of radfoam_hip_geometry.h: device pointers, `stream` a hipStream_t passed as void*, RF_OK
 * or a negative rf_status, nothing synchronises.
 *
 * The star of a site in the Delaunay triangulation of the site and its Delaunay neighbours is its star in the full
 * triangulation ("Tetrahedra from the neighbour lists"), so every row of (adjacency, offsets) is inserted
 * into a fresh star with exact predicates and the tetrahedra are read off its link.  The caller scans the counts; this
 * interface counts, emits, matches every star's triangles against the emitted rows and pairs the faces.  Every output
 * element is written exactly once by a plain store, there are no atomics, and the outputs are bit-reproducible.
 *
 * adjacency[E] and offsets[N+1] are 32-bit words (uint32, or int32: a negative value is out of range).  N < 2^31,
 * E < 2^31, T <= 2^30.  code[N] (uint8) holds rf::tets::Code of csrc/rf_tets.hpp.
 */
#ifndef RADFOAM_HIP_TETS_H
#define RADFOAM_HIP_TETS_H

#include "radfoam_hip_geometry.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * One lane per site: checks the row, builds the star of a row of at most 63 neighbours and writes code[i] and the
 * site's finite triangles entries[i], those among them it owns (all link ids above its own) owned[i] and its hull
 * facets ghosts[i] (uint32 each; zero unless code[i] is 0).  A longer row only gets its class.
 */
int rf_tets_count(const float *points, uint32_t num_points, const uint32_t *adjacency, uint32_t num_edges,
                  const uint32_t *offsets, uint8_t *code, uint32_t *entries, uint32_t *owned, uint32_t *ghosts,
                  void *stream);

/* bytes of the workspace of the second (instance = 1: up to 249 neighbours) or third (2: up to 4095) star instance */
size_t rf_tets_large_workspace_bytes(uint32_t instance);

/*
 * The same for the rows rows[0 .. num_rows) (int64, ascending) with the larger instance, whose stars live in
 * `workspace`: a lane per row, a fixed number of lanes.  code[i] becomes 4 (instance 1) or 5 (instance 2), the class of
 * the next instance, or a failure.
 */
int rf_tets_count_large(uint32_t instance, const float *points, uint32_t num_points, const uint32_t *adjacency,
                        uint32_t num_edges, const uint32_t *offsets, const int64_t *rows, uint32_t num_rows, uint8_t *code,
                        uint32_t *entries, uint32_t *owned, uint32_t *ghosts, void *workspace, size_t workspace_bytes,
                        void *stream);

/*
 * owned_off[N+1], entries_off[N+1] (int64): the exclusive running sums of owned and entries.  Every site with code 0
 * rebuilds its star and writes its owned rows, canonical and in order, to tets[T*4] at owned_off[i] and every finite
 * triangle as its ascending triple to star_entries[F*3] at entries_off[i]; faults[i] (uint32) counts flat and repeated
 * rows, or is 0xFFFFFFFF where the star no longer matches its counts.  Sites of another code are left alone.
 */
int rf_tets_emit(const float *points, uint32_t num_points, const uint32_t *adjacency, uint32_t num_edges,
                 const uint32_t *offsets, const uint8_t *code, const int64_t *owned_off, const int64_t *entries_off,
                 int64_t num_tets, int64_t num_entries, uint32_t *tets, uint32_t *star_entries, uint32_t *faults,
                 void *stream);

/* ... and for the rows of a larger instance (code 4 or 5), as rf_tets_count_large */
int rf_tets_emit_large(uint32_t instance, const float *points, uint32_t num_points, const uint32_t *adjacency,
                       uint32_t num_edges, const uint32_t *offsets, const int64_t *rows, uint32_t num_rows,
                       const uint8_t *code, const int64_t *owned_off, const int64_t *entries_off, int64_t num_tets,
                       int64_t num_entries, uint32_t *tets, uint32_t *star_entries, uint32_t *faults, void *workspace,
                       size_t workspace_bytes, void *stream);

/*
 * One lane per site: looks every entry of the site up among the rows of its owner, ticks the site's corner of the row
 * found in ticks[T*4] (uint8, zeroed by the caller on the stream beforehand), and writes missing[i] (uint32: entries
 * without a row) and vert_to_tet[i] (the smallest row with the site; 0xFFFFFFFF if none).
 */
int rf_tets_match(uint32_t num_points, const uint32_t *star_entries, const int64_t *entries_off, int64_t num_entries,
                  const uint32_t *tets, const int64_t *owned_off, int64_t num_tets, uint8_t *ticks, uint32_t *missing,
                  uint32_t *vert_to_tet, void *stream);

/*
 * order[4T] (int64): the faces 4t + j (the face opposite corner j of row t) in ascending order of their sorted site
 * triples.  One lane per position: tet_adjacency[face] = the face it is paired with, 0xFFFFFFFF on the hull
 * (single[position] = 1); fault[position] = 1 where a face occurs more than twice.
 */
int rf_tets_pair_faces(const uint32_t *tets, int64_t num_tets, const int64_t *order, uint32_t *tet_adjacency,
                       uint8_t *single, uint8_t *fault, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RADFOAM_HIP_TETS_H */
