// locate_sanitize.cpp -- run by hand, not by the suite: the passes of locate_host.cpp (csrc/rf_locate.hpp over rf_star.hpp)
// as a stand-alone program for the sanitizers.
//
//   python -c "from tests.host_harness import locate_host as H; H.write_cases('/tmp/locate_cases.bin')"
//   g++ -O1 -g -std=c++20 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tests/host_harness/locate_sanitize.cpp -o /tmp/locate_sanitize && /tmp/locate_sanitize /tmp/locate_cases.bin
//
// C++20 because the queries on sites, edges and faces take the 384-bit path, whose star::to_grid shifts negative
// mantissas left: defined since C++20 (and what every compiler here does under C++17, where the sanitizer reports it).
//
// The file holds a count and then, per case, {n, T, Q, has start, max_hops, expected fault kind or -1} (int64) and the
// arrays points f32[n,3], tets i64[T,4], tet_adjacency i64[T,4], queries f32[Q,3] and start i64[Q] where it has one: the
// 400-point cloud with the boundary queries, the capped walk and the malformed tables of the tests.  Every case is walked
// with int64 and with 4-byte tables, interpolated (3 channels) and run backward.
#include <cstdio>
#include <vector>

#include "locate_host.cpp"

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t cases = 0;
    if (std::fread(&cases, 8, 1, f) != 1) return 2;
    int wrong = 0;
    for (int64_t c = 0; c < cases; ++c) {
        int64_t head[6];
        if (std::fread(head, 8, 6, f) != 6) return 2;
        const uint32_t n = (uint32_t)head[0], nt = (uint32_t)head[1], nq = (uint32_t)head[2];
        std::vector<float> pts(3 * (size_t)n), q(3 * (size_t)nq);
        std::vector<int64_t> rows(4 * (size_t)nt), adj(4 * (size_t)nt), start(head[3] ? nq : 0);
        if (std::fread(pts.data(), 4, pts.size(), f) != pts.size() || std::fread(rows.data(), 8, rows.size(), f) != rows.size() ||
            std::fread(adj.data(), 8, adj.size(), f) != adj.size() || std::fread(q.data(), 4, q.size(), f) != q.size() ||
            std::fread(start.data(), 8, start.size(), f) != start.size())
            return 2;
        std::vector<uint32_t> rows32(rows.size()), adj32(adj.size());
        for (size_t k = 0; k < rows.size(); ++k) rows32[k] = (uint32_t)rows[k], adj32[k] = (uint32_t)adj[k];
        std::vector<int64_t> tet(nq), tet32(nq);
        std::vector<int32_t> hops(nq), hops32(nq);
        int64_t counters[2];
        const int64_t *s = head[3] ? start.data() : nullptr;
        locate_host_walk(pts.data(), n, rows.data(), adj.data(), 8, nt, q.data(), s, nq, (uint32_t)head[4], tet.data(), hops.data(), counters);
        locate_host_walk(pts.data(), n, rows32.data(), adj32.data(), 4, nt, q.data(), s, nq, (uint32_t)head[4], tet32.data(), hops32.data(), nullptr);
        int64_t first = -1, found = 0, outside = 0;
        bool same = true;
        for (uint32_t k = 0; k < nq; ++k) {
            if (tet[k] < -1 && first < 0) first = (-2 - tet[k]) & 7;
            found += tet[k] >= 0, outside += tet[k] == -1;
            same &= tet[k] == tet32[k] && hops[k] == hops32[k];
        }
        // the interpolation and its backward over whatever the walk gave, fault codes included
        const uint32_t ch = 3;
        std::vector<float> values((size_t)n * ch);
        for (size_t k = 0; k < values.size(); ++k) values[k] = (float)(k % 17) - 8.0f;
        std::vector<double> value((size_t)nq * ch), weights(4 * (size_t)nq), gradient(3 * (size_t)nq * ch), up((size_t)nq * ch, 1.0),
            parts(4 * (size_t)nq * (3 + ch)), gp(3 * (size_t)n), gv((size_t)n * ch), gq(3 * (size_t)nq);
        locate_host_interpolate(pts.data(), n, rows.data(), 8, nt, values.data(), 4, ch, q.data(), tet.data(), nq, value.data(),
                                weights.data(), gradient.data());
        locate_host_interpolate_grad(pts.data(), n, rows32.data(), 4, nt, values.data(), 4, ch, q.data(), tet.data(), nq, up.data(),
                                     parts.data(), gp.data(), gv.data(), gq.data());
        std::printf("case %lld: %u queries over %u tetrahedra, max_hops %lld: %lld found, %lld outside, first fault kind %lld "
                    "(expected %lld), %lld of %lld predicates past the filter, 4-byte tables %s\n",
                    (long long)c, nq, nt, (long long)head[4], (long long)found, (long long)outside, (long long)first,
                    (long long)head[5], (long long)counters[1], (long long)counters[0], same ? "equal" : "DIFFER");
        wrong += first != head[5] || !same;
    }
    std::fclose(f);
    std::printf(wrong ? "%d cases ended with another status\n" : "all cases as expected\n", wrong);
    return wrong ? 1 : 0;
}
