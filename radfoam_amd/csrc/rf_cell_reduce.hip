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
#include "rf_cell_sweep.hpp"

namespace rf {

constexpr int kCellGroup = 8;                              // channels per sweep: 8 timed against 4, DESIGN 4.15

struct CellReduceParams {
    int64_t num_cells, total, num_chunks;
    uint32_t num_channels;
    uint32_t first_channel;      // this launch sums channels first_channel .. first_channel + NCH - 1
    const int64_t *sorted_cells, *entries;   // [S]
    const float *values;         // [S][C]
    float *out;                  // [N][C]
    double *partial;             // [num_chunks][2][C]
};

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

template <int NCH>
void cell_launch(const CellReduceParams &p, hipStream_t stream) {
    hipLaunchKernelGGL(reduce_entries_kernel<NCH>, dim3((uint32_t)cell_sweep_blocks(p.num_chunks)), dim3(kCellBlock),
                       0, stream, p);
}

}  // namespace

extern "C" {

uint32_t rf_reduce_entries_chunk(void) { return (uint32_t)kCellChunk; }

size_t rf_reduce_entries_workspace_bytes(int64_t num_entries, uint32_t num_channels) {
    return cell_workspace_bytes(num_entries, num_channels);
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
    int rc = cell_check(what, num_entries, num_channels, workspace, workspace_bytes);
    if (rc != RF_OK) return rc;
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
        rc = check_launch(what);
        if (rc != RF_OK) return rc;
    }
    return cell_launch_boundaries(what, reduce_entries_boundaries_kernel, p, s);
}

}  // extern "C"
