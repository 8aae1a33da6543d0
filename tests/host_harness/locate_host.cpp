// locate_host.cpp -- TEST HARNESS, not product: compiles radfoam_amd/csrc/rf_locate.hpp (over rf_star.hpp) for the host and
// runs the passes of radfoam_amd/locate.py / rf_locate.hip over it, a loop trip where the kernels have a lane: the walk,
// the interpolation, the backward's parts, the stable sort of the corners by site and the sums per site in that order.
// Only tests/ loads the library this builds; tests/host_harness/locate_sanitize.cpp includes this file.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#define RF_STAR_FN static inline
#define RF_STAR_NOINLINE static __attribute__((noinline))
#define RF_STAR_NOUNROLL
static int64_t g_predicates = 0, g_exact = 0;
static inline void locate_trace_face(const float *pi, const float *pa, const float *pb, const float *pc);
#define RF_LOCATE_TRACE_FACE(pi, pa, pb, pc) locate_trace_face(pi, pa, pb, pc)
#include "../../radfoam_amd/csrc/rf_locate.hpp"

using namespace rf::locate;

// counts the predicates and those the fp64 filter of star::orient_sign does not sign (the same filter, evaluated again)
static inline void locate_trace_face(const float *pi, const float *pa, const float *pb, const float *pc) {
    using namespace rf::star;
    const D3 A = diff(pa[0], pa[1], pa[2], pi[0], pi[1], pi[2]), B = diff(pb[0], pb[1], pb[2], pi[0], pi[1], pi[2]),
             C = diff(pc[0], pc[1], pc[2], pi[0], pi[1], pi[2]);
    double perm;
    const double d = det3(A, B, C, perm);
    ++g_predicates;
    g_exact += !(fabs(d) > kOrientBound * perm);
}

namespace {

// a table of 4- or 8-byte words in storage aligned as the kernels ask
template <typename I>
std::vector<Row32> aligned_copy(const void *table, size_t rows) {
    std::vector<Row32> out(rows * sizeof(I) / 4 + 1);
    if (rows) std::memcpy(out.data(), table, 4 * rows * sizeof(I));
    return out;
}

template <typename I>
void walk_all(const float *pts, uint32_t n, const void *tets, const void *adj, uint32_t nt, const float *queries,
              const int64_t *start, uint32_t nq, uint32_t max_hops, int64_t *tet, int32_t *hops) {
    const auto rows = aligned_copy<I>(tets, nt), links = aligned_copy<I>(adj, nt);
    const I *r = reinterpret_cast<const I *>(rows.data()), *l = reinterpret_cast<const I *>(links.data());
    for (uint32_t k = 0; k < nq; ++k) walk(pts, n, r, l, nt, queries + 3 * (size_t)k, start ? start[k] : 0, max_hops, tet[k], hops[k]);
}

template <typename I, typename V>
void interp_all(const float *pts, uint32_t n, const void *tets, uint32_t nt, const V *values, uint32_t c, const float *queries,
                const int64_t *tet, uint32_t nq, double *value, double *weights, double *gradient) {
    const auto rows = aligned_copy<I>(tets, nt);
    const I *r = reinterpret_cast<const I *>(rows.data());
    for (uint32_t k = 0; k < nq; ++k) {
        int64_t s[4];
        const bool ok = located_sites(r, nt, n, tet[k], s);
        interpolate(pts, s, ok, values, c, queries + 3 * (size_t)k, value + (size_t)k * c, weights + 4 * (size_t)k,
                    gradient + 3 * (size_t)k * c);
    }
}

template <typename I, typename V>
void grad_all(const float *pts, uint32_t n, const void *tets, uint32_t nt, const V *values, uint32_t c, const float *queries,
              const int64_t *tet, uint32_t nq, const double *grad_value, double *parts, double *grad_points,
              double *grad_values, double *grad_queries) {
    const auto rows = aligned_copy<I>(tets, nt);
    const I *r = reinterpret_cast<const I *>(rows.data());
    std::vector<int64_t> site(4 * (size_t)nq), order(4 * (size_t)nq), runs((size_t)n + 1);
    for (uint32_t k = 0; k < nq; ++k) {
        int64_t s[4];
        const bool ok = located_sites(r, nt, n, tet[k], s);
        interpolate_grad(pts, s, ok, values, c, queries + 3 * (size_t)k, grad_value + (size_t)k * c,
                         parts + 4 * (size_t)k * (3 + c), grad_queries + 3 * (size_t)k);
        for (int i = 0; i < 4; ++i) site[4 * (size_t)k + i] = ok ? s[i] : (int64_t)n;   // no site: behind all sites
    }
    for (size_t e = 0; e < order.size(); ++e) order[e] = (int64_t)e;
    std::stable_sort(order.begin(), order.end(), [&site](int64_t x, int64_t y) { return site[x] < site[y]; });
    size_t at = 0;
    for (uint32_t a = 0; a <= n; ++a) {
        while (at < order.size() && site[order[at]] < (int64_t)a) ++at;
        runs[a] = (int64_t)at;
    }
    for (uint32_t a = 0; a < n; ++a)
        site_sum(order.data(), runs.data(), 4 * (int64_t)nq, parts, c, a, grad_points, grad_values);
}

}  // namespace

extern "C" {

// the walk of every query; counters[0] = predicates evaluated, counters[1] = those that left the fp64 filter
void locate_host_walk(const float *pts, uint32_t n, const void *tets, const void *adj, uint32_t index_bytes, uint32_t nt,
                      const float *queries, const int64_t *start, uint32_t nq, uint32_t max_hops, int64_t *tet, int32_t *hops,
                      int64_t *counters) {
    g_predicates = g_exact = 0;
    if (index_bytes == 4u)
        walk_all<uint32_t>(pts, n, tets, adj, nt, queries, start, nq, max_hops, tet, hops);
    else
        walk_all<int64_t>(pts, n, tets, adj, nt, queries, start, nq, max_hops, tet, hops);
    if (counters) counters[0] = g_predicates, counters[1] = g_exact;
}

void locate_host_interpolate(const float *pts, uint32_t n, const void *tets, uint32_t index_bytes, uint32_t nt,
                             const void *values, uint32_t value_bytes, uint32_t c, const float *queries, const int64_t *tet,
                             uint32_t nq, double *value, double *weights, double *gradient) {
    const float *v32 = static_cast<const float *>(values);
    const double *v64 = static_cast<const double *>(values);
    if (index_bytes == 4u && value_bytes == 4u)
        interp_all<uint32_t>(pts, n, tets, nt, v32, c, queries, tet, nq, value, weights, gradient);
    else if (index_bytes == 4u)
        interp_all<uint32_t>(pts, n, tets, nt, v64, c, queries, tet, nq, value, weights, gradient);
    else if (value_bytes == 4u)
        interp_all<int64_t>(pts, n, tets, nt, v32, c, queries, tet, nq, value, weights, gradient);
    else
        interp_all<int64_t>(pts, n, tets, nt, v64, c, queries, tet, nq, value, weights, gradient);
}

// c <= 8, as the kernels
void locate_host_interpolate_grad(const float *pts, uint32_t n, const void *tets, uint32_t index_bytes, uint32_t nt,
                                  const void *values, uint32_t value_bytes, uint32_t c, const float *queries,
                                  const int64_t *tet, uint32_t nq, const double *grad_value, double *parts,
                                  double *grad_points, double *grad_values, double *grad_queries) {
    const float *v32 = static_cast<const float *>(values);
    const double *v64 = static_cast<const double *>(values);
    if (index_bytes == 4u && value_bytes == 4u)
        grad_all<uint32_t>(pts, n, tets, nt, v32, c, queries, tet, nq, grad_value, parts, grad_points, grad_values, grad_queries);
    else if (index_bytes == 4u)
        grad_all<uint32_t>(pts, n, tets, nt, v64, c, queries, tet, nq, grad_value, parts, grad_points, grad_values, grad_queries);
    else if (value_bytes == 4u)
        grad_all<int64_t>(pts, n, tets, nt, v32, c, queries, tet, nq, grad_value, parts, grad_points, grad_values, grad_queries);
    else
        grad_all<int64_t>(pts, n, tets, nt, v64, c, queries, tet, nq, grad_value, parts, grad_points, grad_values, grad_queries);
}

}  // extern "C"
