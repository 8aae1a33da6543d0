// rf_nearest.hpp -- the Voronoi cell of any point: the greedy walk over the neighbour lists that ends at the site nearest
// to a query (rf_nearest.hip; DESIGN.md, "Cell location").  Stated once for the kernel, the host build of
// tests/host_harness and the restatement of radfoam_amd/nearest.py, so that the three can be compared for equality.
//
//   lists         adj[E] and offsets[N + 1] as the cell-geometry operators take them (rf_cell_geometry.hip): row i is
//                 adj[offsets[i] .. offsets[i + 1]).  4-byte words (uint32, or int32: a negative word reads as 2^31 or
//                 more and is out of range) or int64.
//   closer        closer(a, b, q) is the exact sign of |p_a - q|^2 - |p_b - q|^2 for float32 inputs.  The filter is
//                 D(s) = (dx dx + dy dy) + dz dz in double with dx = (double)p_sx - (double)q_x, nothing fused; the sign is
//                 that of D_a - D_b when |D_a - D_b| > kCloserBound (D_a + D_b).  Below the bound the nine coordinates go
//                 to star::to_grid and the squares and sums to 384-bit integers, out of line (exact_closer).  The limit of
//                 to_grid applies and is the only one: a coordinate whose last bit lies more than 38 binary places below
//                 the last bit of the coarsest of the nine is snapped to their grid; the predicate is then exact for the
//                 snapped coordinates only.
//   key           sites are ordered by (exact squared distance to q, index), lexicographic: a strict total order.
//   step          at site s scan row s in list order and keep the entry with the smallest key (a candidate whose D is
//                 within the bound of the running best is compared to it exactly).  If that entry's key is below the key
//                 of s the walk goes there, otherwise s is the answer; an empty row answers s.  The key falls strictly at
//                 every step, so the walk ends on any input (for coordinates beyond to_grid's limit, where the predicates
//                 of different triples may disagree, the hop cap ends it).
//   hops          the steps taken.  A walk that would take more than max_hops steps is a fault; that count is the only
//                 bound of the loop besides the falling key.  A query with a coordinate that is not finite gets -1 and 0
//                 hops, no walk.
//   start         given, in [0, N); or the seed with the smallest key among S staged sites, seed i being site
//                 floor(i N / S) (S <= N, so the sites ascend with i and i stands for the index in the key); or site 0.
//   faults        every index read from memory is checked before it is used: a start outside [0,N), a row whose bounds
//                 run backwards or past E, a list entry outside [0,N), the hop cap.  The result of such a query is
//                 fault_code(kind, site) < -1, which names the kind and the site the walk stood at.
//   guaranteed    on any tables, a returned cell has no entry of its own row with a smaller key; on the neighbour lists
//                 of a Delaunay triangulation of the points it is a global nearest site (a site that is not nearest to q
//                 has a Delaunay neighbour strictly nearer), the nearest site where that is unique.
//
// The includer defines RF_STAR_FN / RF_STAR_NOINLINE / RF_STAR_NOUNROLL as rf_star.hpp asks; no HIP types.
#pragma once

#include <math.h>
#include <stdint.h>

#include "rf_star.hpp"

#ifndef RF_NEAREST_TRACE_CLOSER   // instrumentation hook of the host harness: (the filter signed the predicate)
#define RF_NEAREST_TRACE_CLOSER(decided) ((void)0)
#endif
#ifndef RF_NEAREST_UNROLL         // loop pragma for the short loops over one gather of a row
#define RF_NEAREST_UNROLL
#endif

namespace rf {
namespace nearest {

constexpr int64_t kNoCell = -1;
constexpr uint32_t kMaxSeeds = 1024;   // what the kernel stages: 12 KB of LDS
constexpr uint32_t kGather = 4;        // entries of a row whose points are requested before the first is consumed

enum Fault : uint32_t { kBadStart = 0, kBadRow = 1, kBadEntry = 2, kHopCap = 3 };

// what a faulted query gets in place of a cell: below -1; kind = (-2 - code) & 7, site = (-2 - code) >> 3
RF_STAR_FN int64_t fault_code(uint32_t kind, int64_t site) { return -2 - ((int64_t)kind + 8 * site); }

// The forward error of D, u = 2^-53 per rounding, first order.  dx is exact when the two floats lie within 29 binary
// places of each other (a 53-bit result holds both 24-bit mantissas) and rounds once otherwise: relative error u.  dx dx
// then carries 2 u from its factors and one rounding of its own: 3 u.  (dx dx + dy dy) rounds once: its terms are not
// negative, so the sum is within 4 u of itself; adding dz dz (3 u) rounds once more: D is within 5 u D of the exact
// squared distance.  The difference D_a - D_b rounds once, u |D_a - D_b| <= u (D_a + D_b): the computed difference is
// within 6 u (D_a + D_b) of the exact one, and has its sign whenever it exceeds that.  The right-hand side's own two
// roundings (the sum, the product) are inside the factor of two the constant leaves on the count of 6.  Nothing
// underflows or overflows: a difference of floats is a multiple of 2^-149 below 2^129, its square a double.
constexpr double kCloserBound = 1.5e-15;   // > 2 * 6 * 2^-53

RF_STAR_FN bool finite(float x) { return fabsf(x) < INFINITY; }

RF_STAR_FN bool query_finite(const float *q) { return finite(q[0]) && finite(q[1]) && finite(q[2]); }

RF_STAR_FN int64_t index_at(const uint32_t *table, size_t i) { return (int64_t)table[i]; }
RF_STAR_FN int64_t index_at(const int64_t *table, size_t i) { return table[i]; }

RF_STAR_FN void load_point(const float *pts, int64_t s, float *p) {
    p[0] = pts[3 * (size_t)s], p[1] = pts[3 * (size_t)s + 1], p[2] = pts[3 * (size_t)s + 2];
}

RF_STAR_FN double dist2(const float *p, const float *q) {
    const double dx = (double)p[0] - (double)q[0], dy = (double)p[1] - (double)q[1], dz = (double)p[2] - (double)q[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// sign of |a - q|^2 - |b - q|^2, exact.  p = {a, b, q} as 9 floats.  On the grid a coordinate has 62 bits, a difference
// 63, a square 126 and the six-term sum 129: far inside Big.
RF_STAR_NOINLINE int exact_closer(const float *p) {
    int64_t g[9];
    star::to_grid(p, 9, g);
    star::Big sum, t, x, y;
    star::big_set(&sum, 0);
    RF_STAR_NOUNROLL
    for (int k = 0; k < 6; ++k) {
        const int64_t d = g[k] - g[6 + k % 3];
        star::big_set(&x, d);
        star::big_set(&y, d);
        star::big_mul(&t, &x, &y);
        star::big_addsub(&sum, &sum, &t, k >= 3);
    }
    return star::big_sign(&sum);
}

// key(a) < key(b) for the sites (or seeds) a != b with the filter values da, db
RF_STAR_FN bool key_less(int64_t a, double da, const float *pa, int64_t b, double db, const float *pb, const float *q) {
    const bool decided = fabs(da - db) > kCloserBound * (da + db);
    RF_NEAREST_TRACE_CLOSER(decided);
    if (decided) return da < db;
    const float p[9] = {pa[0], pa[1], pa[2], pb[0], pb[1], pb[2], q[0], q[1], q[2]};
    const int s = exact_closer(p);
    return s < 0 || (s == 0 && a < b);
}

// seed i of S over n sites
RF_STAR_FN uint32_t seed_site(uint32_t i, uint32_t n, uint32_t num_seeds) {
    return (uint32_t)(((uint64_t)i * (uint64_t)n) / (uint64_t)num_seeds);
}

// the seed with the smallest key; staged[3 i ..] are the coordinates of seed_site(i), 1 <= num_seeds <= n
RF_STAR_FN uint32_t best_seed(const float *staged, uint32_t num_seeds, const float *q) {
    uint32_t best = 0;
    double dbest = dist2(staged, q);
    RF_STAR_NOUNROLL
    for (uint32_t i = 1; i < num_seeds; ++i) {
        const double d = dist2(staged + 3 * (size_t)i, q);
        if (key_less((int64_t)i, d, staged + 3 * (size_t)i, (int64_t)best, dbest, staged + 3 * (size_t)best, q)) {
            best = i;
            dbest = d;
        }
    }
    return best;
}

// The walk of one finite query: (cell or a fault code; steps taken).
template <typename I>
RF_STAR_FN void walk(const float *pts, uint32_t n, const I *adj, const I *offsets, uint32_t num_edges, const float *q,
                     int64_t start, uint32_t max_hops, int64_t &cell, int32_t &hops_out) {
    hops_out = 0;
    if (start < 0 || start >= (int64_t)n) {
        cell = fault_code(kBadStart, 0);
        return;
    }
    int64_t s = start;
    uint32_t hops = 0;
    float ps[3];
    load_point(pts, s, ps);
    double ds = dist2(ps, q);
    RF_STAR_NOUNROLL
    for (;;) {
        const int64_t begin = index_at(offsets, (size_t)s), end = index_at(offsets, (size_t)s + 1);
        if (begin < 0 || begin > end || end > (int64_t)num_edges) {
            cell = fault_code(kBadRow, s);
            break;
        }
        int64_t best = -1;
        double dbest = 0.0;
        float pb[3] = {0.0f, 0.0f, 0.0f};
        bool bad = false;
        RF_STAR_NOUNROLL
        for (int64_t j = begin; j < end; j += (int64_t)kGather) {
            const uint32_t count = end - j < (int64_t)kGather ? (uint32_t)(end - j) : kGather;
            int64_t e[kGather];
            float p[kGather][3];
            RF_NEAREST_UNROLL
            for (uint32_t c = 0; c < kGather; ++c) {
                e[c] = c < count ? index_at(adj, (size_t)j + c) : 0;
                bad |= e[c] < 0 || e[c] >= (int64_t)n;
            }
            if (bad) break;
            RF_NEAREST_UNROLL
            for (uint32_t c = 0; c < kGather; ++c) load_point(pts, e[c], p[c]);   // (a slot past the row reads site 0)
            RF_NEAREST_UNROLL
            for (uint32_t c = 0; c < kGather; ++c) {
                if (c >= count) continue;
                const double d = dist2(p[c], q);
                if (best < 0 || (e[c] != best && key_less(e[c], d, p[c], best, dbest, pb, q))) {
                    best = e[c], dbest = d;
                    pb[0] = p[c][0], pb[1] = p[c][1], pb[2] = p[c][2];
                }
            }
        }
        if (bad) {
            cell = fault_code(kBadEntry, s);
            break;
        }
        if (best < 0 || best == s || !key_less(best, dbest, pb, s, ds, ps, q)) {
            cell = s;
            break;
        }
        if (hops >= max_hops) {
            cell = fault_code(kHopCap, s);
            break;
        }
        s = best, ds = dbest;
        ps[0] = pb[0], ps[1] = pb[1], ps[2] = pb[2];
        ++hops;
    }
    hops_out = (int32_t)hops;
}

// One query from end to end: not finite, -1; else from its start, the best of the staged seeds, or site 0.
template <typename I>
RF_STAR_FN void locate_one(const float *pts, uint32_t n, const I *adj, const I *offsets, uint32_t num_edges,
                           const float *staged, uint32_t num_seeds, const float *q, const int64_t *start, uint32_t max_hops,
                           int64_t &cell, int32_t &hops) {
    cell = kNoCell, hops = 0;
    if (!query_finite(q)) return;
    const int64_t from = start ? *start : num_seeds ? (int64_t)seed_site(best_seed(staged, num_seeds, q), n, num_seeds) : 0;
    walk(pts, n, adj, offsets, num_edges, q, from, max_hops, cell, hops);
}

}  // namespace nearest
}  // namespace rf
