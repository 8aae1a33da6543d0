// tets_sanitize.cpp -- run by hand, not by the suite: the passes of tets_host.cpp (csrc/rf_tets.hpp over rf_star.hpp) as
// a stand-alone program for the sanitizers.
//
//   python -c "from tests.host_harness import tets_host as H; H.write_cases('/tmp/tets_cases.bin')"
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tests/host_harness/tets_sanitize.cpp -o /tmp/tets_sanitize && /tmp/tets_sanitize /tmp/tets_cases.bin
//
// The file holds a count and then, per case, {n, e, expected status} and the arrays points f32[n,3], adjacency i32[e],
// offsets i32[n+1]: the 400-point cloud, the hub of 300 neighbours, and the malformed and stale rows of the tests.
#include <cstdio>
#include <vector>

#include "tets_host.cpp"

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t cases = 0;
    if (std::fread(&cases, 4, 1, f) != 1) return 2;
    int wrong = 0;
    for (uint32_t c = 0; c < cases; ++c) {
        uint32_t head[3];
        if (std::fread(head, 4, 3, f) != 3) return 2;
        const uint32_t n = head[0], e = head[1];
        std::vector<float> pts(3 * (size_t)n);
        std::vector<uint32_t> adj(e), off(n + 1);
        if (std::fread(pts.data(), 4, pts.size(), f) != pts.size() || std::fread(adj.data(), 4, e, f) != e ||
            std::fread(off.data(), 4, off.size(), f) != off.size())
            return 2;
        int64_t info[13];
        const int rc = tets_host_build(pts.data(), n, adj.data(), e, off.data(), 1, info);
        std::vector<uint32_t> tets(4 * (size_t)info[0] + 4), v2t(n), tadj(4 * (size_t)info[0] + 4), owned(n);
        std::vector<uint8_t> code(n);
        if (rc == 0) tets_host_fetch(tets.data(), v2t.data(), tadj.data(), owned.data(), code.data());
        std::printf("case %u: %u points, %u entries: status %d (expected %u), %lld tetrahedra, %lld hull facets, big %lld, huge %lld\n",
                    c, n, e, rc, head[2], (long long)info[0], (long long)info[1], (long long)info[8], (long long)info[9]);
        wrong += rc != (int)head[2];
    }
    std::fclose(f);
    std::printf(wrong ? "%d cases ended with another status\n" : "all cases as expected\n", wrong);
    return wrong ? 1 : 0;
}
