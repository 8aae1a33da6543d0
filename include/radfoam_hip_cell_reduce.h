/*
 * radfoam_hip_cell_reduce.h -- C-ABI of the sum per cell over an exported walk (libradfoam_hip.so, rf_cell_reduce.hip;
 * DESIGN.md section 4.15): for a per-entry quantity values [num_entries, num_channels] and the walk transposed (its
 * entries in a stable sort by cell),
 *     out[c, :] = sum of values[e, :] over the entries e of cell c,
 * which is also the gradient of the lookup table[cells] with respect to the table.
 *
 * Conventions of radfoam_hip.h: every pointer is a DEVICE pointer, `stream` is a hipStream_t passed as void*, every
 * function returns RF_OK or a negative rf_status and leaves a message for rf_last_error.  Nothing synchronises.
 *
 * The index is two arrays of num_entries int64 each, position by position of the sorted list:
 *     sorted_cells[k]  the cell of position k, non-decreasing in k
 *     entries[k]       the entry at position k; within a cell in ascending order
 * Work is dealt by POSITIONS, never by cells: one wave owns rf_reduce_entries_chunk() consecutive positions whatever
 * the cells' list lengths are.  Sums are formed in double and rounded to fp32 once.  Nothing is accumulated with
 * atomics: out is cleared once (cells without entries keep those exact zeros), then every element of a cell with
 * entries is written by exactly one lane, and two calls on the same inputs give the same bits.  A cell whose list
 * crosses from one chunk into the next has its per-chunk sums stored in double in the workspace and added in chunk
 * order by a second launch.
 *
 * A position whose sorted_cells lies outside 0 .. num_cells - 1 is skipped, and so is one whose entries lies outside
 * 0 .. num_entries - 1: an index that is no index of this list gives wrong numbers, never an access outside the arrays.
 */
#ifndef RADFOAM_HIP_CELL_REDUCE_H
#define RADFOAM_HIP_CELL_REDUCE_H

#include "radfoam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The number of consecutive sorted positions one wave owns (a compile-time constant of the library, a multiple of 64). */
uint32_t rf_reduce_entries_chunk(void);

/* Bytes of workspace rf_reduce_entries needs for num_entries positions and num_channels channels: two rows of doubles
 * per chunk.  0 for a negative num_entries. */
size_t rf_reduce_entries_workspace_bytes(int64_t num_entries, uint32_t num_channels);

/* out [num_cells * num_channels] (fp32): every element is written.  values holds num_entries * num_channels elements
 * (fp32, row-major), workspace at least rf_reduce_entries_workspace_bytes(num_entries, num_channels) bytes, 8-byte
 * aligned; its contents before and after the call mean nothing.  With num_entries == 0 only out is written. */
int rf_reduce_entries(int64_t num_cells, int64_t num_entries, const int64_t *sorted_cells, const int64_t *entries,
                      const float *values, uint32_t num_channels, float *out, void *workspace, size_t workspace_bytes,
                      void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RADFOAM_HIP_CELL_REDUCE_H */
