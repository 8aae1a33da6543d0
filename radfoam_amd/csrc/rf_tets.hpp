// rf_tets.hpp -- the Delaunay tetrahedra read back off the neighbour lists ("Tetrahedra from the neighbour
// lists").  Stated once, for the kernels of rf_tets.hip and for the host build of tests/host_harness/tets_host.cpp:
//
//   * the row check: what a row of (point_adjacency, point_adjacency_offsets) must be before anything is built from it;
//   * the star from a row: the Voronoi cell of a site is the intersection of the half-spaces of its Delaunay neighbours
//     alone, so the star of a in the triangulation of {a} u N(a) is its star in the full triangulation, hull facets
//     included.  A row is therefore inserted into a fresh star (rf_star.hpp: nearest first, exact predicates) with no
//     tree, no query and no certification; the row is accepted when every entry ends as a link vertex;
//   * the canonical row of a tetrahedron: its four sites ascending, the last two swapped where the exact sign of
//     det[p1 - p0; p2 - p0; p3 - p0] asks for it, so that the determinant is positive; a zero sign is a failure;
//   * the order of a star's rows: ascending by the sorted triple of link ids.  A site owns the tetrahedra in which it
//     is the smallest site, so "owner after owner, each owner's rows ascending" is the ascending lexicographic order
//     of the sorted site sets;
//   * the match: every finite link triangle of every star is looked up among its owner's rows and ticks the corner it
//     stands for.  A row whose four corners are ticked is confirmed by all four of its sites.
//
// The includer defines the qualifier macros of rf_star.hpp before including this file.
#pragma once

#include "rf_star.hpp"

namespace rf {
namespace tets {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kSmallRow = 63, kBigRow = 249, kHugeRow = 4095;   // neighbours the three star instances take

using SmallStar = star::Star<64, 124>;
using BigStar = star::Star<250, 496>;
using HugeStar = star::Star<4096, 8188, uint16_t, 1024>;

// what the count pass says about a row (one byte per site)
enum Code : uint8_t {
    kOk = 0,         // built by the small instance
    kNeedBig = 1,    // 64..249 neighbours, or the small instance ran out of room: the second instance
    kNeedHuge = 2,   // 250..4095 neighbours, or the second instance ran out of room: the third
    kOkBig = 4,      // built by the second instance
    kOkHuge = 5,     // built by the third
    // malformed lists (RuntimeError)
    kBadOffsets = 8, kBadIndex = 9, kSelf = 10, kTwice = 11, kTooLong = 12,
    // the lists are not those of a Delaunay triangulation of the points (TriangulationFailedError)
    kDegenerate = 16, kBroken = 17, kDuplicate = 18, kNotLink = 19,
};

// where row i lies in the adjacency, or kBadOffsets.  Offsets and indices arrive as 32-bit words: a negative int32 is
// a value above 2^31 and fails the comparisons like any other value out of range.
RF_STAR_FN uint8_t row_bounds(const uint32_t *off, uint32_t n, uint32_t num_edges, uint32_t i, uint32_t &first,
                              uint32_t &deg) {
    const uint32_t a = off[i], b = off[i + 1];
    first = 0;
    deg = 0;
    if (a > b || b > num_edges || (i == 0 && a != 0u) || (i + 1 == n && b != num_edges)) return kBadOffsets;
    first = a;
    deg = b - a;
    return kOk;
}

// the row itself: every index in range, none the site itself, none twice
RF_STAR_FN uint8_t row_check(const uint32_t *row, uint32_t deg, uint32_t n, uint32_t i) {
    if (deg > kHugeRow) return kTooLong;
    for (uint32_t k = 0; k < deg; ++k)
        if (row[k] >= n) return kBadIndex;
    for (uint32_t k = 0; k < deg; ++k)
        if (row[k] == i) return kSelf;
    for (uint32_t k = 1; k < deg; ++k) {
        const uint32_t g = row[k];
        bool twice = false;
        for (uint32_t m = 0; m < k; ++m) twice |= row[m] == g;
        if (twice) return kTwice;
    }
    return kOk;
}

// star::sort_seeds over buffers the caller owns (the large instances keep theirs in a workspace): nearest first, ties in
// the order of the row
RF_STAR_FN void sort_row(const float *pts, const float *p, const uint32_t *row, uint32_t deg, uint32_t *seeds, float *d2) {
    for (uint32_t k = 0; k < deg; ++k) {
        const uint32_t g = row[k];
        const float dx = pts[3 * (size_t)g] - p[0], dy = pts[3 * (size_t)g + 1] - p[1], dz = pts[3 * (size_t)g + 2] - p[2];
        const float d = dx * dx + dy * dy + dz * dz;
        uint32_t pos = k;
        while (pos > 0 && d2[pos - 1] > d) {
            d2[pos] = d2[pos - 1];
            seeds[pos] = seeds[pos - 1];
            --pos;
        }
        d2[pos] = d;
        seeds[pos] = g;
    }
}

// The star of site i from its (checked) row.  kOk, the class of the next instance when this one has no room, or why the
// row is not the site's Delaunay neighbourhood.  seeds / d2: room for deg entries.
template <typename S>
RF_STAR_FN uint8_t star_from_row(S &s, const float *pts, uint32_t i, const uint32_t *row, uint32_t deg, uint32_t *seeds,
                                 float *d2, uint8_t next_class) {
    if (deg > (uint32_t)S::kV - 1u) return next_class;
    sort_row(pts, pts + 3 * (size_t)i, row, deg, seeds, d2);
    star::star_reset(s, i, pts + 3 * (size_t)i);
    uint32_t inserted = 0;
    star::star_seed(s, pts, seeds, (int)deg, inserted);
    if (s.status == star::kOverflow) return next_class;
    if (s.status == star::kDegenerate) return kDegenerate;
    if (s.status == star::kDuplicate) return kDuplicate;
    if (s.status != star::kOk) return kBroken;
    // every entry of the row is a link vertex: the entries are distinct, so as many live slots as entries
    uint32_t live = 0;
    for (int k = 1; k < S::kV; ++k) live += s.v[k].use != 0;
    return live == deg ? kOk : kNotLink;
}

template <typename S>
RF_STAR_FN bool tri_finite(const S &s, int t) {
    return s.t[t].a != 0 && s.t[t].b != 0 && s.t[t].c != 0;
}

RF_STAR_FN void sort3(uint32_t *g) {
    uint32_t t;
    if (g[0] > g[1]) t = g[0], g[0] = g[1], g[1] = t;
    if (g[1] > g[2]) t = g[1], g[1] = g[2], g[2] = t;
    if (g[0] > g[1]) t = g[0], g[0] = g[1], g[1] = t;
}

// the three link ids of a finite triangle, ascending
template <typename S>
RF_STAR_FN void tri_sites(const S &s, int t, uint32_t *g) {
    g[0] = s.v[s.t[t].a].g;
    g[1] = s.v[s.t[t].b].g;
    g[2] = s.v[s.t[t].c].g;
    sort3(g);
}

RF_STAR_FN int triple_cmp(const uint32_t *x, const uint32_t *y) {
    if (x[0] != y[0]) return x[0] < y[0] ? -1 : 1;
    if (x[1] != y[1]) return x[1] < y[1] ? -1 : 1;
    if (x[2] != y[2]) return x[2] < y[2] ? -1 : 1;
    return 0;
}

// finite triangles, those the site owns (all three link ids above its own) and ghosts (hull facets at the site)
template <typename S>
RF_STAR_FN void star_counts(const S &s, uint32_t &entries, uint32_t &owned, uint32_t &ghosts) {
    entries = owned = ghosts = 0;
    for (int t = 0; t < s.nt; ++t) {
        if (!tri_finite(s, t)) {
            ++ghosts;
            continue;
        }
        ++entries;
        const uint32_t a = s.v[s.t[t].a].g, b = s.v[s.t[t].b].g, c = s.v[s.t[t].c].g;
        owned += a > s.self && b > s.self && c > s.self;
    }
}

// The canonical row from four ascending sites: the exact sign of det[p1 - p0; p2 - p0; p3 - p0]; negative swaps the
// last two.  Returns the sign before the swap: zero is a flat tetrahedron, which no triangulation returns.
RF_STAR_FN int canonical_row(const float *pts, uint32_t *row) {
    const int sign = star::orient_sign(pts + 3 * (size_t)row[0], pts + 3 * (size_t)row[1], pts + 3 * (size_t)row[2],
                                       pts + 3 * (size_t)row[3]);
    if (sign < 0) {
        const uint32_t t = row[2];
        row[2] = row[3];
        row[3] = t;
    }
    return sign;
}

// Writes what a star emits: its owned rows, canonical, in the order of a star's rows (tets_out: 4 words a row) and every
// finite triangle as its ascending triple (entries_out: 3 words an entry).  ord: room for S::kT indices.  Returns the
// number of faults -- a flat row, a row that occurs twice -- or kNone, with nothing written, when the star does not hold
// the counts the scan was made from.
template <typename S>
RF_STAR_FN uint32_t star_emit(const S &s, const float *pts, uint16_t *ord, uint32_t owned, uint32_t entries,
                              uint32_t *tets_out, uint32_t *entries_out) {
    uint32_t ne, no, ng;
    star_counts(s, ne, no, ng);
    if (ne != entries || no != owned) return kNone;
    uint32_t e = 0, o = 0;
    for (int t = 0; t < s.nt; ++t) {
        if (!tri_finite(s, t)) continue;
        uint32_t g[3];
        tri_sites(s, t, g);
        entries_out[3 * (size_t)e] = g[0], entries_out[3 * (size_t)e + 1] = g[1], entries_out[3 * (size_t)e + 2] = g[2];
        ++e;
        if (g[0] <= s.self) continue;
        // insertion into the order of the star's rows
        uint32_t pos = o++;
        while (pos > 0) {
            uint32_t h[3];
            tri_sites(s, ord[pos - 1], h);
            if (triple_cmp(h, g) <= 0) break;
            ord[pos] = ord[pos - 1];
            --pos;
        }
        ord[pos] = (uint16_t)t;
    }
    uint32_t faults = 0;
    uint32_t prev[3] = {kNone, kNone, kNone};
    for (uint32_t k = 0; k < o; ++k) {
        uint32_t row[4];
        tri_sites(s, ord[k], row + 1);
        row[0] = s.self;
        faults += k > 0 && triple_cmp(prev, row + 1) == 0;
        prev[0] = row[1], prev[1] = row[2], prev[2] = row[3];
        faults += canonical_row(pts, row) == 0;
        uint32_t *out = tets_out + 4 * (size_t)k;
        out[0] = row[0], out[1] = row[1], out[2] = row[2], out[3] = row[3];
    }
    return faults;
}

// The match of one site: each of its `count` entries (ascending triples) is a tetrahedron with the site; its owner is the
// smallest of the four, and the owner's rows [owned_off[o], owned_off[o + 1]) are searched for it.  A row found gets the
// site's corner ticked in `ticks` (4 bytes a row, zeroed beforehand; plain stores of 1).  first_tet: the smallest row
// found, kNone if none.  Returns the number of entries without a row.
RF_STAR_FN uint32_t match_site(uint32_t v, uint32_t n, const uint32_t *entries, uint32_t count, const int64_t *owned_off,
                               const uint32_t *tets, int64_t num_tets, uint8_t *ticks, uint32_t &first_tet) {
    uint32_t missing = 0;
    first_tet = kNone;
    for (uint32_t k = 0; k < count; ++k) {
        const uint32_t *g = entries + 3 * (size_t)k;
        uint32_t rest[3] = {g[0], g[1], g[2]};
        uint32_t owner = v;
        if (g[0] < v) {   // the owner is g[0]: v takes its place among the other three
            owner = g[0];
            rest[0] = v;
            sort3(rest);
        }
        bool found = false;
        if (owner < n) {
            int64_t lo = owned_off[owner], hi = owned_off[owner + 1];
            if (lo >= 0 && lo <= hi && hi <= num_tets) {
                while (lo < hi) {
                    const int64_t mid = lo + (hi - lo) / 2;
                    const uint32_t *row = tets + 4 * (size_t)mid;
                    const uint32_t key[3] = {row[1], row[2] < row[3] ? row[2] : row[3], row[2] < row[3] ? row[3] : row[2]};
                    const int c = triple_cmp(key, rest);
                    if (c == 0) {
                        for (int j = 0; j < 4; ++j)
                            if (row[j] == v) {
                                ticks[4 * (size_t)mid + j] = 1;
                                found = true;
                            }
                        first_tet = (uint32_t)mid < first_tet ? (uint32_t)mid : first_tet;
                        break;
                    }
                    if (c < 0) lo = mid + 1;
                    else hi = mid;
                }
            }
        }
        missing += !found;
    }
    return missing;
}

// The face opposite corner j of a row, as an ascending triple
RF_STAR_FN void row_face(const uint32_t *row, uint32_t j, uint32_t *g) {
    uint32_t m = 0;
    for (uint32_t c = 0; c < 4; ++c)
        if (c != j) g[m++] = row[c];
    sort3(g);
}

// One sorted face: order[0 .. 4T) lists the faces 4t + j in ascending order of their triples.  Position i pairs with its
// equal neighbour: adjacency[face] = the other face, kNone when it has none (a hull facet: *single = 1).  *fault = 1
// when the face is seen more than twice.
RF_STAR_FN void pair_face(const uint32_t *tets, int64_t num_faces, const int64_t *order, int64_t i, uint32_t *adjacency,
                          uint8_t *single, uint8_t *fault) {
    const int64_t f = order[i];
    single[i] = 0;
    fault[i] = 0;
    if (f < 0 || f >= num_faces) {
        fault[i] = 1;
        return;
    }
    uint32_t g[3], h[3];
    row_face(tets + 4 * (size_t)(f >> 2), (uint32_t)(f & 3), g);
    int64_t before = -1, after = -1;
    if (i > 0) {
        const int64_t b = order[i - 1];
        if (b >= 0 && b < num_faces) {
            row_face(tets + 4 * (size_t)(b >> 2), (uint32_t)(b & 3), h);
            if (triple_cmp(g, h) == 0) before = b;
        }
    }
    if (i + 1 < num_faces) {
        const int64_t a = order[i + 1];
        if (a >= 0 && a < num_faces) {
            row_face(tets + 4 * (size_t)(a >> 2), (uint32_t)(a & 3), h);
            if (triple_cmp(g, h) == 0) after = a;
        }
    }
    if (before >= 0 && after >= 0) fault[i] = 1;
    const int64_t mate = after >= 0 ? after : before;
    adjacency[f] = mate >= 0 ? (uint32_t)mate : kNone;
    single[i] = mate < 0;
}

}  // namespace tets
}  // namespace rf
