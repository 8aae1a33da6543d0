// nearest_sanitize.cpp -- run by hand, not by the suite: the pass of nearest_host.cpp (csrc/rf_nearest.hpp over
// rf_star.hpp) as a stand-alone program for the sanitizers.
//
//   python -c "from tests.host_harness import nearest_host as H; H.write_cases('/tmp/nearest_cases.bin')"
//   g++ -O1 -g -std=c++20 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tests/host_harness/nearest_sanitize.cpp -o /tmp/nearest_sanitize && /tmp/nearest_sanitize /tmp/nearest_cases.bin
//
// C++20 because the tie queries take the 384-bit path, whose star::to_grid shifts negative mantissas left: defined since
// C++20 (and what every compiler here does under C++17, where the sanitizer reports it).
//
// The file holds a count and then, per case, {n, E, Q, has start, seeds, max_hops, expected fault kind or -1} (int64) and
// the arrays points f32[n,3], adjacency i64[E], offsets i64[n+1], queries f32[Q,3] and start i64[Q] where it has one: the
// 400-point cloud with all query kinds (seeded, from site 0, from given starts), the capped walk and the malformed lists
// of the tests.  Every case is walked with int64 and with 4-byte lists.
#include <cstdio>
#include <vector>

#include "nearest_host.cpp"

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t cases = 0;
    if (std::fread(&cases, 8, 1, f) != 1) return 2;
    int wrong = 0;
    for (int64_t c = 0; c < cases; ++c) {
        int64_t head[7];
        if (std::fread(head, 8, 7, f) != 7) return 2;
        const uint32_t n = (uint32_t)head[0], ne = (uint32_t)head[1], nq = (uint32_t)head[2];
        const uint32_t seeds = head[3] ? 0u : (uint32_t)(head[4] < head[0] ? head[4] : head[0]);
        std::vector<float> pts(3 * (size_t)n), q(3 * (size_t)nq);
        std::vector<int64_t> adj(ne), off((size_t)n + 1), start(head[3] ? nq : 0);
        if (std::fread(pts.data(), 4, pts.size(), f) != pts.size() || std::fread(adj.data(), 8, adj.size(), f) != adj.size() ||
            std::fread(off.data(), 8, off.size(), f) != off.size() || std::fread(q.data(), 4, q.size(), f) != q.size() ||
            std::fread(start.data(), 8, start.size(), f) != start.size())
            return 2;
        std::vector<uint32_t> adj32(adj.size()), off32(off.size());
        for (size_t k = 0; k < adj.size(); ++k) adj32[k] = (uint32_t)adj[k];
        for (size_t k = 0; k < off.size(); ++k) off32[k] = (uint32_t)off[k];
        std::vector<int64_t> cell(nq), cell32(nq);
        std::vector<int32_t> hops(nq), hops32(nq);
        int64_t counters[2];
        const int64_t *s = head[3] ? start.data() : nullptr;
        nearest_host_locate(pts.data(), n, adj.data(), off.data(), 8, ne, q.data(), s, seeds, nq, (uint32_t)head[5], cell.data(),
                            hops.data(), counters);
        nearest_host_locate(pts.data(), n, adj32.data(), off32.data(), 4, ne, q.data(), s, seeds, nq, (uint32_t)head[5],
                            cell32.data(), hops32.data(), nullptr);
        int64_t first = -1, found = 0, none = 0, most = 0;
        bool same = true;
        for (uint32_t k = 0; k < nq; ++k) {
            if (cell[k] < -1 && first < 0) first = (-2 - cell[k]) & 7;
            found += cell[k] >= 0, none += cell[k] == -1;
            most = hops[k] > most ? hops[k] : most;
            same &= cell[k] == cell32[k] && hops[k] == hops32[k];
        }
        std::printf("case %lld: %u queries over %u sites, %u seeds, max_hops %lld: %lld cells, %lld without, at most %lld hops, "
                    "first fault kind %lld (expected %lld), %lld of %lld predicates past the filter, 4-byte lists %s\n",
                    (long long)c, nq, n, seeds, (long long)head[5], (long long)found, (long long)none, (long long)most,
                    (long long)first, (long long)head[6], (long long)counters[1], (long long)counters[0],
                    same ? "equal" : "DIFFER");
        wrong += first != head[6] || !same;
    }
    std::fclose(f);
    std::printf(wrong ? "%d cases ended with another status\n" : "all cases as expected\n", wrong);
    return wrong ? 1 : 0;
}
