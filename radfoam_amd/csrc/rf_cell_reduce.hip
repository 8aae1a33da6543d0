// rf_cell_reduce.hip -- the sum per cell of a per-entry quantity over an exported walk
// (include/radfoam_hip_cell_reduce.h).
//
//     out[c][:] = sum of values[e][:] over the entries e of cell c
//
// read through the walk transposed: position k of the list sorted by cell holds its cell sorted_cells[k] and its entry
// entries[k].  The list lengths of a camera frame are as skewed as they can be (every ray's first entry is the start
// cell), so WORK IS DEALT BY POSITIONS, never by cells: one wave owns kCellChunk consecutive positions and sweeps them
// 64 at a time, one lane per position.  It reads the cell and the entry coalesced and the entry's row of values by the
// entry.  A run of equal cells is summed by rf_ray_sweep.hpp's inclusive segmented scan in double; a run that goes on
// into the wave's next step hands its sums on in wave-uniform registers.
//
// NO ATOMICS, EVERY ELEMENT OF A CELL WITH ENTRIES WRITTEN ONCE.  The last lane of a run within the chunk holds the
// run's sum.  A cell whose list lies inside the chunk is rounded to fp32 there and stored.  A list that crosses a chunk
// boundary leaves its per-chunk sums in double in partial[chunk][0] (it came in from the chunk before) or
// partial[chunk][1] (it begins here and goes on).  reduce_entries_boundaries_kernel, one lane per chunk BOUNDARY, then
// finds the boundaries a list crosses; the lane of the boundary the list crosses first adds the partial sums in chunk
// order and stores the row.  A list of up to two chunks is finished by that lane alone; a longer one by the whole wave,
// which loads 64 chunks' sums coalesced and adds them one after the other.  The cells without entries are not visited:
// out is cleared once in front of the launches.
//
// Whether a list goes on is read from sorted_cells itself (the position in front of the chunk, the one behind it), so
// the two kernels agree on it by construction.  Every cell and entry is range-checked where it is read; what lies
// outside is skipped.  No lane returns before the last cross-lane operation of its wave (a wave without work returns
// whole, before the first).  No LDS.
//
// Channels go in groups of at most kCellGroup, one sweep per group, so that the carried sums stay in registers
// whatever C is.
//
// Compiled like the tracer (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/radfoam_hip_cell_reduce.h"
#include "rf_host.hpp"
#include "rf_ray_sweep.hpp"

#ifndef RF_CELL_REDUCE_CHUNK
#define RF_CELL_REDUCE_CHUNK 1024
#endif

namespace rf {

constexpr int kCellBlock = 256;
constexpr int kCellWaves = kCellBlock / 64;
constexpr int kCellChunk = RF_CELL_REDUCE_CHUNK;           // sorted positions per wave: 256 .. 2048 timed, DESIGN 4.15
constexpr int kCellGroup = 8;                              // channels per sweep: 8 timed against 4, DESIGN 4.15
static_assert(kCellChunk >= 64 && kCellChunk % 64 == 0, "a wave sweeps its chunk in whole steps of 64 positions");

struct CellReduceParams {
    int64_t num_cells, total, num_chunks;
    uint32_t num_channels;
    uint32_t first_channel;      // this launch sums channels first_channel .. first_channel + NCH - 1
    const int64_t *sorted_cells, *entries;   // [S]
    const float *values;         // [S][C]
    float *out;                  // [N][C]
    double *partial;             // [num_chunks][2][C]
};

// the cell of position k: -1 for a position outside the list or a cell outside 0 .. N-1
__device__ __forceinline__ int64_t cell_at(const CellReduceParams &p, int64_t k) {
    if (k < 0 || k >= p.total) return -1;
    const int64_t c = p.sorted_cells[k];
    return c < 0 || c >= p.num_cells ? -1 : c;
}

template <int NCH>
__global__ __launch_bounds__(kCellBlock) void reduce_entries_kernel(CellReduceParams p) {
    const int lane = (int)(threadIdx.x & 63u);
    const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t chunk = (int64_t)blockIdx.x * kCellWaves + wave_in_block;
    if (chunk >= p.num_chunks) return;
    const int64_t c0 = chunk * kCellChunk;
    const int64_t c1 = c0 + kCellChunk < p.total ? c0 + kCellChunk : p.total;
    const int64_t cell_before = cell_at(p, c0 - 1);                      // wave-uniform
    const uint64_t upto_me = ~(uint64_t)0 >> (63 - lane);
    const size_t C = p.num_channels;

    double carry[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) carry[c] = 0.0;
    bool carry_first = true;     // the run that reaches a step's first lane began at the chunk's first position
    for (int64_t base = c0; base < c1; base += 64) {
        const int64_t k = base + lane;
        const bool in = k < c1;
        const int64_t cell = in ? cell_at(p, k) : -1;
        const int64_t next = in ? cell_at(p, k + 1) : -1;
        const bool chunk_end = k + 1 == c1;
        const bool same_next = cell >= 0 && next == cell;
        const bool run_end = !same_next || chunk_end;                    // the last lane of its run within the chunk
        const uint64_t ends = __builtin_amdgcn_ballot_w64(run_end || lane == 63);
        const int begin = 63 - __builtin_clzll(((ends << 1) | 1u) & upto_me);   // the first lane of its run in this step
        const bool first_run = begin == 0 && carry_first;

        double v[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) v[c] = 0.0;
        if (cell >= 0) {
            const int64_t e = p.entries[k];
            if (e >= 0 && e < p.total) {
                const float *row = p.values + (size_t)e * C + p.first_channel;
#pragma unroll
                for (int c = 0; c < NCH; ++c) v[c] = (double)row[c];
            }
        }
        WaveLanes::scan(v, lane, begin);
        if (begin == 0) {                                                // what the run carried in: zeros for a new one
#pragma unroll
            for (int c = 0; c < NCH; ++c) v[c] = v[c] + carry[c];
        }

        if (cell >= 0 && run_end) {
            const bool from_before = first_run && cell_before == cell;
            const bool goes_on = chunk_end && same_next;
            if (from_before || goes_on) {
                double *row = p.partial + ((size_t)chunk * 2 + (from_before ? 0 : 1)) * C + p.first_channel;
#pragma unroll
                for (int c = 0; c < NCH; ++c) row[c] = v[c];
            } else {                                                     // the cell's whole list: round once
                float *row = p.out + (size_t)cell * C + p.first_channel;
#pragma unroll
                for (int c = 0; c < NCH; ++c) row[c] = (float)v[c];
            }
        }
        const bool onward = !run_end;                                    // read at lane 63: its run meets the next step
#pragma unroll
        for (int c = 0; c < NCH; ++c) carry[c] = WaveLanes::from_lane(onward ? v[c] : 0.0, 63);
        carry_first = (__builtin_amdgcn_ballot_w64(onward && first_run) >> 63) != 0;
    }
}

// chunk j holds a partial[j][0] of `cell`: the list came in from the chunk before
__device__ __forceinline__ bool came_in(const CellReduceParams &p, int64_t j, int64_t cell) {
    return j < p.num_chunks && cell_at(p, j * kCellChunk) == cell && cell_at(p, j * kCellChunk - 1) == cell;
}

__global__ __launch_bounds__(kCellBlock) void reduce_entries_boundaries_kernel(CellReduceParams p) {
    const int lane = (int)(threadIdx.x & 63u);
    const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t boundaries = p.num_chunks - 1;                         // boundary b lies between chunks b and b + 1
    const int64_t b0 = ((int64_t)blockIdx.x * kCellWaves + wave_in_block) * 64;
    if (b0 >= boundaries) return;
    const int64_t b = b0 + lane;
    const size_t C = p.num_channels;

    // the list that crosses boundary b, if one does, and whether it begins in chunk b: then this lane answers for it
    int64_t cell = -1;
    bool longer = false;
    if (b < boundaries) {
        const int64_t left = cell_at(p, (b + 1) * kCellChunk - 1);
        if (left >= 0 && cell_at(p, (b + 1) * kCellChunk) == left && !came_in(p, b, left)) {
            cell = left;
            longer = came_in(p, b + 2, left);
            if (!longer) {                                               // two chunks: this lane alone
                const double *first = p.partial + ((size_t)b * 2 + 1) * C;
                const double *second = p.partial + ((size_t)b + 1) * 2 * C;
                float *row = p.out + (size_t)cell * C;
                for (size_t c = 0; c < C; ++c) row[c] = (float)(first[c] + second[c]);
            }
        }
    }

    // three chunks and more: the wave, 64 chunks a step, added one after the other in chunk order
    uint64_t todo = __builtin_amdgcn_ballot_w64(longer);
    while (todo != 0) {                                                  // wave-uniform
        const int owner = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int64_t first_chunk = b0 + owner;
        const int64_t its_cell = WaveLanes::uniform(WaveLanes::from_lane(cell, owner));
        for (size_t c = 0; c < C; ++c) {
            double sum = p.partial[((size_t)first_chunk * 2 + 1) * C + c];
            for (int64_t j0 = first_chunk + 1;; j0 += 64) {
                const int64_t j = j0 + lane;
                const uint64_t others = ~__builtin_amdgcn_ballot_w64(came_in(p, j, its_cell));
                const int count = others != 0 ? __builtin_ctzll(others) : 64;    // the chunks in front of the first other
                const double mine = lane < count ? p.partial[(size_t)j * 2 * C + c] : 0.0;
                for (int i = 0; i < count; ++i)
                    sum = sum + __builtin_bit_cast(double, WaveLanes::read_lane(__builtin_bit_cast(int64_t, mine), i));
                if (count < 64) break;
            }
            if (lane == 0) p.out[(size_t)its_cell * C + c] = (float)sum;
        }
    }
}

}  // namespace rf

using namespace rf;

namespace {

int64_t cell_chunks(int64_t num_entries) { return (num_entries + kCellChunk - 1) / kCellChunk; }

template <int NCH>
void cell_launch(const CellReduceParams &p, hipStream_t stream) {
    const int64_t blocks = (p.num_chunks + kCellWaves - 1) / kCellWaves;
    hipLaunchKernelGGL(reduce_entries_kernel<NCH>, dim3((uint32_t)blocks), dim3(kCellBlock), 0, stream, p);
}

}  // namespace

extern "C" {

uint32_t rf_reduce_entries_chunk(void) { return (uint32_t)kCellChunk; }

size_t rf_reduce_entries_workspace_bytes(int64_t num_entries, uint32_t num_channels) {
    if (num_entries <= 0) return 0;
    return (size_t)cell_chunks(num_entries) * 2 * (size_t)num_channels * sizeof(double);
}

int rf_reduce_entries(int64_t num_cells, int64_t num_entries, const int64_t *sorted_cells, const int64_t *entries,
                      const float *values, uint32_t num_channels, float *out, void *workspace, size_t workspace_bytes,
                      void *stream) {
    const char *what = "rf_reduce_entries";
    g_err[0] = 0;
    if (num_entries < 0) return fail(RF_ERR_INVALID_ARGUMENT, "%s: negative entry count", what);
    if (num_cells < 0) return fail(RF_ERR_INVALID_ARGUMENT, "%s: negative cell count", what);
    if (num_channels == 0) return fail(RF_ERR_INVALID_ARGUMENT, "%s: no channels", what);
    if (num_cells == 0) return RF_OK;
    if (!out) return fail(RF_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(out, 0, (size_t)num_cells * num_channels * sizeof(float), s) != hipSuccess)
        return check_launch(what);
    if (num_entries == 0) return RF_OK;
    if (!sorted_cells || !entries || !values) return fail(RF_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    if (!workspace || workspace_bytes < rf_reduce_entries_workspace_bytes(num_entries, num_channels))
        return fail(RF_ERR_WORKSPACE, "%s: workspace missing or too small", what);
    if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0)
        return fail(RF_ERR_WORKSPACE, "%s: the workspace must be 8-byte aligned", what);
    CellReduceParams p{};
    p.num_cells = num_cells;
    p.total = num_entries;
    p.num_chunks = cell_chunks(num_entries);
    p.num_channels = num_channels;
    p.sorted_cells = sorted_cells;
    p.entries = entries;
    p.values = values;
    p.out = out;
    p.partial = static_cast<double *>(workspace);
    if ((p.num_chunks + kCellWaves - 1) / kCellWaves >= ((int64_t)1 << 31))
        return fail(RF_ERR_INVALID_ARGUMENT, "%s: too many entries for one launch", what);
    for (uint32_t first = 0; first < num_channels; first += kCellGroup) {
        p.first_channel = first;
        switch (num_channels - first < (uint32_t)kCellGroup ? num_channels - first : (uint32_t)kCellGroup) {
            case 1: cell_launch<1>(p, s); break;
            case 2: cell_launch<2>(p, s); break;
            case 3: cell_launch<3>(p, s); break;
            case 4: cell_launch<4>(p, s); break;
            case 5: cell_launch<5>(p, s); break;
            case 6: cell_launch<6>(p, s); break;
            case 7: cell_launch<7>(p, s); break;
            default: cell_launch<8>(p, s); break;
        }
        const int rc = check_launch(what);
        if (rc != RF_OK) return rc;
    }
    if (p.num_chunks > 1) {
        const int64_t waves = (p.num_chunks - 1 + 63) / 64;
        hipLaunchKernelGGL(reduce_entries_boundaries_kernel, dim3((uint32_t)((waves + kCellWaves - 1) / kCellWaves)),
                           dim3(kCellBlock), 0, s, p);
        return check_launch(what);
    }
    return RF_OK;
}

}  // extern "C"
