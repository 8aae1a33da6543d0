// nearest_host.cpp -- TEST HARNESS, not product: compiles radfoam_amd/csrc/rf_nearest.hpp (over rf_star.hpp) for the host
// and runs the pass of radfoam_amd/nearest.py / rf_nearest.hip over it, a loop trip where the kernel has a lane: the seeds
// staged once, then every query's start and walk.  Only tests/ loads the library this builds;
// tests/host_harness/nearest_sanitize.cpp includes this file.
#include <cstdint>
#include <vector>

#define RF_STAR_FN static inline
#define RF_STAR_NOINLINE static __attribute__((noinline))
#define RF_STAR_NOUNROLL
static int64_t g_predicates = 0, g_exact = 0;
// counts the predicates and those the fp64 filter does not sign
#define RF_NEAREST_TRACE_CLOSER(decided) (++g_predicates, g_exact += !(decided))
#include "../../radfoam_amd/csrc/rf_nearest.hpp"

using namespace rf::nearest;

namespace {

template <typename I>
void locate_all(const float *pts, uint32_t n, const void *adj, const void *offsets, uint32_t ne, const float *queries,
                const int64_t *start, uint32_t num_seeds, uint32_t nq, uint32_t max_hops, int64_t *cell, int32_t *hops) {
    std::vector<float> staged(3 * (size_t)(start ? 0u : num_seeds) + 3);
    if (!start)
        for (uint32_t i = 0; i < num_seeds; ++i) load_point(pts, seed_site(i, n, num_seeds), staged.data() + 3 * (size_t)i);
    for (uint32_t k = 0; k < nq; ++k)
        locate_one(pts, n, static_cast<const I *>(adj), static_cast<const I *>(offsets), ne, staged.data(), num_seeds,
                   queries + 3 * (size_t)k, start ? start + k : nullptr, max_hops, cell[k], hops[k]);
}

}  // namespace

extern "C" {

// the cell of every query; num_seeds <= min(n, 1024) as the kernel; counters[0] = predicates evaluated, counters[1] =
// those that left the fp64 filter
void nearest_host_locate(const float *pts, uint32_t n, const void *adj, const void *offsets, uint32_t index_bytes, uint32_t ne,
                         const float *queries, const int64_t *start, uint32_t num_seeds, uint32_t nq, uint32_t max_hops,
                         int64_t *cell, int32_t *hops, int64_t *counters) {
    g_predicates = g_exact = 0;
    if (index_bytes == 4u)
        locate_all<uint32_t>(pts, n, adj, offsets, ne, queries, start, num_seeds, nq, max_hops, cell, hops);
    else
        locate_all<int64_t>(pts, n, adj, offsets, ne, queries, start, num_seeds, nq, max_hops, cell, hops);
    if (counters) counters[0] = g_predicates, counters[1] = g_exact;
}

// the exact path on its own: the sign of |a - q|^2 - |b - q|^2 of p = {a, b, q}
int nearest_host_exact_closer(const float *p) { return exact_closer(p); }

}  // extern "C"
