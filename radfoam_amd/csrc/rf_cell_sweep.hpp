// rf_cell_sweep.hpp -- what the two sums per cell over an exported walk state once: reduce_entries (rf_cell_reduce.hip,
// whose head describes the scheme) and the coefficient gradient of rf_sh_entries.hip.  On the
// host the chunk, the chunks of a list, the workspace of their partial sums, the checks, the launch sizes and the
// boundary launch; on the device cell_at and came_in (both parameter structs name num_cells, total, num_chunks and
// sorted_cells).  THE TWO PAIRS OF KERNELS ARE NOT HERE: every shared spelling of their bodies tried so far changes
// their code (DESIGN 4.16 lists them).  reduce_entries_kernel and reduce_entries_boundaries_kernel are the text;
// sh_entries_coeffs_kernel and sh_entries_coeffs_boundaries_kernel follow it line by line.
#pragma once

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include "rf_host.hpp"
#include "rf_ray_sweep.hpp"

#ifndef RF_CELL_REDUCE_CHUNK
#define RF_CELL_REDUCE_CHUNK 1024
#endif

namespace rf {

constexpr int kCellBlock = 256;
constexpr int kCellWaves = kCellBlock / 64;
constexpr int kCellChunk = RF_CELL_REDUCE_CHUNK;           // sorted positions per wave: 256 .. 2048 timed, DESIGN 4.15
static_assert(kCellChunk >= 64 && kCellChunk % 64 == 0, "a wave sweeps its chunk in whole steps of 64 positions");

// ---- host ----
inline int64_t cell_chunks(int64_t num_entries) { return (num_entries + kCellChunk - 1) / kCellChunk; }

// partial[num_chunks][2][num_channels] in double
inline size_t cell_workspace_bytes(int64_t num_entries, uint32_t num_channels) {
    if (num_entries <= 0) return 0;
    return (size_t)cell_chunks(num_entries) * 2 * (size_t)num_channels * sizeof(double);
}

// blocks of kCellWaves waves: one wave per chunk, and one lane per boundary between two chunks
inline int64_t cell_sweep_blocks(int64_t num_chunks) { return (num_chunks + kCellWaves - 1) / kCellWaves; }
inline int64_t cell_boundary_blocks(int64_t num_chunks) {
    const int64_t waves = (num_chunks - 1 + 63) / 64;
    return (waves + kCellWaves - 1) / kCellWaves;
}

// RF_OK, or the error of a workspace that is missing, too small or misaligned, or of a list too long for one launch
inline int cell_check(const char *what, int64_t num_entries, uint32_t num_channels, const void *workspace,
                      size_t workspace_bytes) {
    if (!workspace || workspace_bytes < cell_workspace_bytes(num_entries, num_channels))
        return fail(RF_ERR_WORKSPACE, "%s: workspace missing or too small", what);
    if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0)
        return fail(RF_ERR_WORKSPACE, "%s: the workspace must be 8-byte aligned", what);
    if (cell_sweep_blocks(cell_chunks(num_entries)) >= ((int64_t)1 << 31))
        return fail(RF_ERR_INVALID_ARGUMENT, "%s: too many entries for one launch", what);
    return RF_OK;
}

// the boundary pass behind the sweeps, where there is a boundary
template <class P>
int cell_launch_boundaries(const char *what, void (*kernel)(P), const P &p, hipStream_t stream) {
    if (p.num_chunks <= 1) return RF_OK;
    hipLaunchKernelGGL(kernel, dim3((uint32_t)cell_boundary_blocks(p.num_chunks)), dim3(kCellBlock), 0, stream, p);
    return check_launch(what);
}

// ---- device ----
// the cell of position k: -1 for a position outside the list or a cell outside 0 .. N-1
template <class P>
__device__ __forceinline__ int64_t cell_at(const P &p, int64_t k) {
    if (k < 0 || k >= p.total) return -1;
    const int64_t c = p.sorted_cells[k];
    return c < 0 || c >= p.num_cells ? -1 : c;
}

// chunk j holds a partial[j][0] of `cell`: the list came in from the chunk before
template <class P>
__device__ __forceinline__ bool came_in(const P &p, int64_t j, int64_t cell) {
    return j < p.num_chunks && cell_at(p, j * kCellChunk) == cell && cell_at(p, j * kCellChunk - 1) == cell;
}

}  // namespace rf
