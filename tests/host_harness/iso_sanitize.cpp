// iso_sanitize.cpp -- TEST HARNESS, not product: a stand-alone program (its own main, no Python) that runs the
// per-tetrahedron and per-edge routines of radfoam_amd/csrc/rf_iso.hpp over fields written out as plain arrays, meant to
// be built with the host sanitizers and run once on the CPU:
//
//     python -c "from tests.host_harness import iso_host as h; h.write_arrays('masks', 'masks.bin'); h.write_arrays((400, 1), 'cloud.bin')"
//     g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//         -o iso_sanitize tests/host_harness/iso_sanitize.cpp
//     ./iso_sanitize masks.bin cloud.bin
//
// A file is: uint32 N, uint32 T, uint32 fields, float points[3N], int64 tets[4T], then per field double level and float
// values[N].  Every field is counted, emitted into arrays of exactly 3F keys and F tetrahedra, welded, and its vertices
// and their backward evaluated into arrays of exactly 3V, V and 8V doubles, so that a write past an end is a heap
// overflow the sanitizer sees; then once more with a value made NaN, one made infinite and an index out of range on
// either side, and with the vertices of a topology gone stale (two equal values, a site out of range).  Prints one line
// per field; exit status 0 unless a file cannot be read, a key is unwritten, a vertex of a fresh topology is not finite or
// a stale one's backward is.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../radfoam_amd/csrc/rf_iso.hpp"

namespace {

template <class T>
bool read_array(std::FILE *f, std::vector<T> &out, size_t count) {
    out.resize(count);
    return count == 0 || std::fread(out.data(), sizeof(T), count, f) == count;
}

struct Mesh {
    size_t triangles = 0, vertices = 0;
    int64_t first_bad = -1;
    double sum = 0.0;
    bool ok = true;
};

Mesh run_field(const std::vector<float> &points, const std::vector<int64_t> &tets, const std::vector<float> &values,
               double level) {
    using namespace rf::iso;
    const uint32_t n = (uint32_t)values.size(), nt = (uint32_t)(tets.size() / 4);
    Mesh m;
    std::vector<uint8_t> counts(nt);
    for (uint32_t t = 0; t < nt; ++t) {
        int64_t s[4];
        counts[t] = 0;
        if (tet_sites(tets.data() + 4 * (size_t)t, n, s))
            counts[t] = (uint8_t)mask_triangles(sites_mask(values.data(), s, level));
        else if (m.first_bad < 0)
            m.first_bad = t;
        m.triangles += counts[t];
    }
    std::vector<int64_t> keys(3 * m.triangles);
    size_t first = 0;
    for (uint32_t t = 0; t < nt; ++t) {
        if (!counts[t]) continue;
        int64_t s[4];
        const bool in_range = tet_sites(tets.data() + 4 * (size_t)t, n, s);
        tet_emit(points.data(), values.data(), in_range, s, level, counts[t], keys.data() + 3 * first);
        first += counts[t];
    }
    for (int64_t k : keys) m.ok = m.ok && k >= 0;
    std::vector<int64_t> uniq(keys);
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    m.vertices = uniq.size();
    std::vector<int64_t> sites(2 * m.vertices);
    for (size_t v = 0; v < m.vertices; ++v) key_sites(uniq[v], sites[2 * v], sites[2 * v + 1]);
    std::vector<double> x(3 * m.vertices), t(m.vertices), parts(8 * m.vertices), g(3 * m.vertices, 1.0);
    for (size_t v = 0; v < m.vertices; ++v) {
        edge_vertex(points.data(), values.data(), n, sites.data() + 2 * v, level, x.data() + 3 * v, t.data() + v);
        edge_vertex_grad(points.data(), values.data(), n, sites.data() + 2 * v, level, g.data() + 3 * v, parts.data() + 8 * v);
        for (int c = 0; c < 3; ++c) m.ok = m.ok && std::isfinite(x[3 * v + c]);
        m.ok = m.ok && t[v] >= 0.0 && t[v] <= 1.0;
        for (int c = 0; c < 8; ++c) m.ok = m.ok && std::isfinite(parts[8 * v + c]);
        m.sum += x[3 * v] + x[3 * v + 1] + x[3 * v + 2];
    }
    // the same topology gone stale: the first vertex's two values made equal, the last one's second site out of range
    if (m.vertices) {
        std::vector<float> stale(values);
        stale[sites[1]] = stale[sites[0]];
        std::vector<int64_t> moved(sites);
        moved[2 * m.vertices - 1] = (int64_t)n;
        for (size_t v = 0; v < m.vertices; ++v) {
            edge_vertex(points.data(), stale.data(), n, moved.data() + 2 * v, level, x.data() + 3 * v, t.data() + v);
            edge_vertex_grad(points.data(), stale.data(), n, moved.data() + 2 * v, level, g.data() + 3 * v, parts.data() + 8 * v);
            for (int c = 0; c < 8; ++c) m.ok = m.ok && std::isfinite(parts[8 * v + c]);
        }
        m.ok = m.ok && std::isnan(x[0]) && parts[0] == 0.0 && std::isnan(x[3 * m.vertices - 1]);
    }
    return m;
}

int run_file(const char *path) {
    std::FILE *f = std::fopen(path, "rb");
    if (!f) return std::fprintf(stderr, "%s: cannot open\n", path), 2;
    uint32_t head[3];
    if (std::fread(head, sizeof(uint32_t), 3, f) != 3) return std::fclose(f), std::fprintf(stderr, "%s: short\n", path), 2;
    const uint32_t n = head[0], nt = head[1], fields = head[2];
    std::vector<float> points;
    std::vector<int64_t> tets;
    if (!(read_array(f, points, 3 * (size_t)n) && read_array(f, tets, 4 * (size_t)nt)))
        return std::fclose(f), std::fprintf(stderr, "%s: short\n", path), 2;
    int rc = 0;
    for (uint32_t k = 0; k < fields; ++k) {
        double level;
        std::vector<float> values;
        if (std::fread(&level, sizeof(double), 1, f) != 1 || !read_array(f, values, n))
            return std::fclose(f), std::fprintf(stderr, "%s: short\n", path), 2;
        const Mesh plain = run_field(points, tets, values, level);
        std::vector<float> holed(values);
        std::vector<int64_t> broken(tets);
        if (n > 1) holed[0] = NAN, holed[n - 1] = INFINITY;
        if (nt > 1) broken[1] = -1, broken[4 * (size_t)nt - 1] = (int64_t)n;
        const Mesh other = run_field(points, broken, holed, level);
        if (!plain.ok || !other.ok || plain.first_bad != -1 || (nt > 1 && other.first_bad != 0)) rc = 1;
        std::printf("%s field %u: N = %u, T = %u, level %g: %zu triangles over %zu vertices, sum of coordinates %.17g; with a "
                    "NaN, an infinity and two indices out of range %zu over %zu%s\n",
                    path, k, n, nt, level, plain.triangles, plain.vertices, plain.sum, other.triangles, other.vertices,
                    rc ? "  FAILED" : "");
    }
    std::fclose(f);
    return rc;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) return std::fprintf(stderr, "usage: %s arrays.bin [...]\n", argv[0]), 2;
    int rc = 0;
    for (int i = 1; i < argc; ++i) {
        const int one = run_file(argv[i]);
        if (one > rc) rc = one;
    }
    return rc;
}
