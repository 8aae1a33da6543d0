// epoch_host.cpp -- TEST HARNESS, not product: a stand-alone program (its own main, no Python) around the host build of
// radfoam_amd/csrc/rf_epoch.hpp, the length of the image backward's flush epochs.  tests/test_epoch_host.py builds it
// with the shipped constants and with -DRF_CACHE_EPOCH=... -DRF_CACHE_EPOCH_LONG=... -DRF_CACHE_EPOCH_LONG_ROWS=...,
// plainly and with the host sanitizers:
//     g++ -O1 -g -std=c++17 -fsanitize=undefined,address -fno-sanitize-recover=all -o epoch_host tests/host_harness/epoch_host.cpp
//     ./epoch_host 256
// It prints the configured constants and, for every resident count 0..ROWS and both values of the wide bit, the length
// epoch_steps returns (for the test to judge on its own), checks the same properties itself and that the epoch word
// gives back what up to 15 waves added to it; exit status 1 on any miss.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../radfoam_amd/csrc/rf_epoch.hpp"

static_assert(rf::epoch_steps(0u, true) == (uint32_t)RF_CACHE_EPOCH, "usable in constant expressions");

int main(int argc, char **argv) {
    const uint32_t rows = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 256u;
    const uint32_t shorter = RF_CACHE_EPOCH, longer = RF_CACHE_EPOCH_LONG, limit = RF_CACHE_EPOCH_LONG_ROWS;
    std::printf("config %u %u %u %u\n", shorter, longer, limit, rows);
    int bad = 0;
    for (uint32_t wide = 0; wide < 2u; ++wide)
        for (uint32_t resident = 0; resident <= rows; ++resident) {
            const uint32_t steps = rf::epoch_steps(resident, wide != 0u);
            std::printf("steps %u %u %u\n", resident, wide, steps);
            if (steps != shorter && steps != longer) bad++;
            if ((wide != 0u || resident > limit) && steps != shorter) bad++;
            if (wide == 0u && resident <= limit && steps != longer) bad++;
        }
    // the word: `waves` waves, each keeping `per` rows; wave w keeps a wide row / was lit / has a live lane by the bits of
    // three masks.  Every field must come back whatever the others hold.
    for (uint32_t waves = 1; waves <= 15u; waves += 2u)
        for (uint32_t per = 0; per <= 64u; per += 16u)
            for (uint32_t mask = 0; mask < 8u; ++mask) {
                uint32_t word = 0u;
                for (uint32_t w = 0; w < waves; ++w) {
                    const bool last = w + 1u == waves;   // the flags of one wave only, or of all of them
                    const bool wide = (mask & 1u) && (last || (per & 16u));
                    const bool lit = (mask & 2u) && (last || (per & 32u));
                    const bool alive = (mask & 4u) && (last || (per & 16u));
                    word += rf::epoch_word(per, wide) + (lit ? rf::kEpochLitBit : 0u) + (alive ? rf::kEpochAliveBit : 0u);
                }
                if (rf::epoch_resident(word) != waves * per) bad++;
                if (rf::epoch_any_wide(word) != ((mask & 1u) != 0u)) bad++;
                if (rf::epoch_lit(word) != ((mask & 2u) != 0u)) bad++;
                if (rf::epoch_alive(word) != ((mask & 4u) != 0u)) bad++;
            }
    std::printf("bad %d\n", bad);
    return bad ? 1 : 0;
}
