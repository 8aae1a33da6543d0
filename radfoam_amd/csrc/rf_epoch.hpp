// The length of the image backward's next flush epoch (backward_replay_cached_kernel, rf_kernels.hip), as a pure
// function of what the block's waves reported between the two barriers of the flush that just ended.  Kept apart
// from the kernel so that it compiles for the host (tests/host_harness/epoch_host.cpp).
#pragma once
#include <cstdint>

// steps between two flushes while colour or point gradients arrive (wide rows resident), or the table is filling
#ifndef RF_CACHE_EPOCH
#define RF_CACHE_EPOCH 4
#endif
// steps between two flushes while only density sums trickle in; RF_CACHE_EPOCH_LONG == RF_CACHE_EPOCH: fixed epochs
#ifndef RF_CACHE_EPOCH_LONG
#define RF_CACHE_EPOCH_LONG 8
#endif
// a long epoch starts only with at most this many rows resident
#ifndef RF_CACHE_EPOCH_LONG_ROWS
#define RF_CACHE_EPOCH_LONG_ROWS 48
#endif

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RF_EPOCH_FN __host__ __device__ __forceinline__
#else
#define RF_EPOCH_FN inline
#endif

namespace rf {

// What the waves add to the block's epoch word (one LDS atomic per wave and flush; at most 15 waves): the rows a
// wave's threads keep resident in bits 0-15, and one count of waves each in bits 16-19 (the wave keeps a wide row),
// 20-23 (sections build: the wave added colour or point gradients in the epoch) and 24-27 (the wave has a live lane).
constexpr uint32_t kEpochWideBit = 1u << 16, kEpochLitBit = 1u << 20, kEpochAliveBit = 1u << 24;

RF_EPOCH_FN constexpr uint32_t epoch_word(uint32_t resident, bool any_wide) {
    return resident + (any_wide ? kEpochWideBit : 0u);
}
RF_EPOCH_FN constexpr uint32_t epoch_resident(uint32_t word) { return word & 0xffffu; }
RF_EPOCH_FN constexpr bool epoch_any_wide(uint32_t word) { return (word & (15u * kEpochWideBit)) != 0u; }
RF_EPOCH_FN constexpr bool epoch_lit(uint32_t word) { return (word & (15u * kEpochLitBit)) != 0u; }
RF_EPOCH_FN constexpr bool epoch_alive(uint32_t word) { return (word & (15u * kEpochAliveBit)) != 0u; }

RF_EPOCH_FN constexpr uint32_t epoch_steps(uint32_t resident, bool any_wide) {
    return (any_wide || resident > (uint32_t)RF_CACHE_EPOCH_LONG_ROWS) ? (uint32_t)RF_CACHE_EPOCH : (uint32_t)RF_CACHE_EPOCH_LONG;
}

}  // namespace rf
