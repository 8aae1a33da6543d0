// tets_host.cpp -- TEST HARNESS, not product: compiles radfoam_amd/csrc/rf_tets.hpp (over rf_star.hpp) for the host and
// runs the passes of radfoam_amd/tets.py / rf_tets.hip over it, a loop trip where the kernels have a lane: count, the
// larger instances, the scans, emit, match, the face pairing.  Only tests/ loads the library this builds.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#define RF_STAR_FN static inline
#define RF_STAR_NOINLINE static __attribute__((noinline))
#define RF_STAR_NOUNROLL
#include "../../radfoam_amd/csrc/rf_tets.hpp"

using namespace rf::tets;

namespace {

template <typename S>
struct Slot {
    S star;
    uint32_t seeds[S::kV];
    float d2[S::kV];
    uint16_t ord[S::kT];
};

struct Result {
    std::vector<uint8_t> code;
    std::vector<uint32_t> entries, owned, ghosts, tets, vert_to_tet, adjacency;
    int64_t num_tets = 0, hull = 0;
} g;

template <typename S>
uint8_t count_row(Slot<S> &w, const float *pts, uint32_t n, const uint32_t *adj, uint32_t e, const uint32_t *off, uint32_t i,
                  uint8_t ok, uint8_t next) {
    uint32_t first, deg;
    uint8_t c = row_bounds(off, n, e, i, first, deg);
    if (c == kOk) c = row_check(adj + first, deg, n, i);
    if (c == kOk) c = star_from_row(w.star, pts, i, adj + first, deg, w.seeds, w.d2, next);
    g.entries[i] = g.owned[i] = g.ghosts[i] = 0;
    if (c == kOk) {
        star_counts(w.star, g.entries[i], g.owned[i], g.ghosts[i]);
        c = ok;
    }
    return c;
}

template <typename S>
uint32_t emit_row(Slot<S> &w, const float *pts, uint32_t n, const uint32_t *adj, uint32_t e, const uint32_t *off, uint32_t i,
                  uint32_t *tets_out, uint32_t *entries_out) {
    uint32_t first, deg;
    if (row_bounds(off, n, e, i, first, deg) != kOk) return kNone;
    if (star_from_row(w.star, pts, i, adj + first, deg, w.seeds, w.d2, kTooLong) != kOk) return kNone;
    return star_emit(w.star, pts, w.ord, g.owned[i], g.entries[i], tets_out, entries_out);
}

}  // namespace

extern "C" {

// 0: done; 1: malformed lists (info[2] = the first such row, info[3] = its code); 2: not a Delaunay triangulation.
// info[0] = T, info[1] = hull facets, info[4] = failed stars, info[5] = sites with a flat or repeated row, info[6] = sites
// with a triangle their owner does not hold, info[7] = corners unconfirmed, info[8] / info[9] = rows built by the second /
// third instance, info[10] = F, info[11] = faces seen more than twice, info[12] = unpaired faces
int tets_host_build(const float *pts, uint32_t n, const uint32_t *adj, uint32_t e, const uint32_t *off, int want_adjacency,
                    int64_t *info) {
    for (int k = 0; k < 13; ++k) info[k] = 0;
    g = Result();
    g.code.assign(n, 0);
    g.entries.assign(n, 0);
    g.owned.assign(n, 0);
    g.ghosts.assign(n, 0);
    auto small = std::make_unique<Slot<SmallStar>>();
    auto big = std::make_unique<Slot<BigStar>>();
    auto huge = std::make_unique<Slot<HugeStar>>();
    // count: the small instance, then the rows of the larger classes
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t first, deg;
        uint8_t c = row_bounds(off, n, e, i, first, deg);
        if (c == kOk) c = row_check(adj + first, deg, n, i);
        if (c == kOk) c = deg > kBigRow ? kNeedHuge : deg > kSmallRow ? kNeedBig : count_row(*small, pts, n, adj, e, off, i, kOk, kNeedBig);
        g.code[i] = c;
    }
    for (uint32_t i = 0; i < n; ++i)
        if (g.code[i] == kNeedBig) g.code[i] = count_row(*big, pts, n, adj, e, off, i, kOkBig, kNeedHuge);
    for (uint32_t i = 0; i < n; ++i)
        if (g.code[i] == kNeedHuge) g.code[i] = count_row(*huge, pts, n, adj, e, off, i, kOkHuge, kTooLong);
    int64_t failed = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t c = g.code[i];
        if (c >= 8 && c < 16) {
            info[2] = i;
            info[3] = c;
            return 1;
        }
        failed += c >= 16;
        info[8] += c == kOkBig;
        info[9] += c == kOkHuge;
    }
    info[4] = failed;
    if (failed) return 2;
    // the scans
    std::vector<int64_t> owned_off(n + 1, 0), entries_off(n + 1, 0);
    int64_t ghosts = 0;
    for (uint32_t i = 0; i < n; ++i) {
        owned_off[i + 1] = owned_off[i] + g.owned[i];
        entries_off[i + 1] = entries_off[i] + g.entries[i];
        ghosts += g.ghosts[i];
    }
    const int64_t nt = owned_off[n], nf = entries_off[n];
    info[0] = g.num_tets = nt;
    info[1] = g.hull = ghosts / 3;
    info[10] = nf;
    if (nf != 4 * nt || ghosts % 3) return 2;
    // emit
    g.tets.assign(4 * (size_t)nt + 4, kNone);
    std::vector<uint32_t> entries(3 * (size_t)nf + 3, kNone);
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t *to = g.tets.data() + 4 * (size_t)owned_off[i], *eo = entries.data() + 3 * (size_t)entries_off[i];
        const uint32_t faults = g.code[i] == kOk      ? emit_row(*small, pts, n, adj, e, off, i, to, eo)
                                : g.code[i] == kOkBig ? emit_row(*big, pts, n, adj, e, off, i, to, eo)
                                                      : emit_row(*huge, pts, n, adj, e, off, i, to, eo);
        info[5] += faults != 0;
    }
    // match
    std::vector<uint8_t> ticks(4 * (size_t)nt + 4, 0);
    g.vert_to_tet.assign(n, kNone);
    for (uint32_t v = 0; v < n; ++v)
        info[6] += match_site(v, n, entries.data() + 3 * (size_t)entries_off[v], g.entries[v], owned_off.data(), g.tets.data(),
                              nt, ticks.data(), g.vert_to_tet[v]) != 0;
    int64_t ticked = 0;
    for (int64_t k = 0; k < 4 * nt; ++k) ticked += ticks[k];
    info[7] = 4 * nt - ticked;
    if (info[5] || info[6] || info[7]) return 2;
    if (!want_adjacency) return 0;
    // the faces, sorted by their triples, paired
    const int64_t faces = 4 * nt;
    std::vector<int64_t> order(faces);
    for (int64_t f = 0; f < faces; ++f) order[f] = f;
    const uint32_t *tets = g.tets.data();
    std::stable_sort(order.begin(), order.end(), [tets](int64_t x, int64_t y) {
        uint32_t a[3], b[3];
        row_face(tets + 4 * (size_t)(x >> 2), (uint32_t)(x & 3), a);
        row_face(tets + 4 * (size_t)(y >> 2), (uint32_t)(y & 3), b);
        return triple_cmp(a, b) < 0;
    });
    g.adjacency.assign(faces + 4, kNone);
    std::vector<uint8_t> single(faces + 1), fault(faces + 1);
    for (int64_t i = 0; i < faces; ++i) {
        pair_face(tets, faces, order.data(), i, g.adjacency.data(), single.data(), fault.data());
        info[11] += fault[i];
        info[12] += single[i];
    }
    return info[11] || info[12] != info[1] ? 2 : 0;
}

void tets_host_fetch(uint32_t *tets, uint32_t *vert_to_tet, uint32_t *adjacency, uint32_t *owned, uint8_t *code) {
    const size_t nt = (size_t)g.num_tets;
    if (tets && nt) std::memcpy(tets, g.tets.data(), 16 * nt);
    if (vert_to_tet && !g.vert_to_tet.empty()) std::memcpy(vert_to_tet, g.vert_to_tet.data(), 4 * g.vert_to_tet.size());
    if (adjacency && nt && !g.adjacency.empty()) std::memcpy(adjacency, g.adjacency.data(), 16 * nt);
    if (owned && !g.owned.empty()) std::memcpy(owned, g.owned.data(), 4 * g.owned.size());
    if (code && !g.code.empty()) std::memcpy(code, g.code.data(), g.code.size());
}

}  // extern "C"
