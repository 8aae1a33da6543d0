// clip_box_area_grad_sanitize.cpp -- TEST HARNESS, not product: a stand-alone program (its own main, no Python) that runs
// rf::clip::cell_box_area_grad_serial of radfoam_amd/csrc/rf_clip_box_area_grad.hpp over clouds written out as plain arrays, meant
// to be built with the host sanitizers and run once on the CPU:
//
//     python -c "from tests.host_harness import clip_box_area_grad_host as h; h.write_arrays('hub65', 'hub65.bin')"
//     g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//         -o clip_box_area_grad_sanitize tests/host_harness/clip_box_area_grad_sanitize.cpp
//     ./clip_box_area_grad_sanitize hub65.bin ring17_cut.bin grid_bisectors.bin
//
// A file is: uint32 N, uint32 E, float points[3N], uint32 adj[E], uint32 offsets[N+1], float bbox[6], double box[6] (the
// format of clip_box_sanitize.cpp).  The forward runs once at capacity 256; then every row of the gradient is run with
// polygon and label buffers of exactly 2 * cap elements and arrays of exactly E, 6N and 3N elements, for cap = 256 and
// for the small capacities at which rows start to be refused (17, 16 and 4, the square itself), so that a write past a
// buffer's end is a heap overflow the sanitizer sees.  The upstreams are +-1 / V^(1/3) per slot and per wall (+-1 on a
// cell that is not non-empty) and NaN wherever the slot's or wall's own forward area is exactly 0, which nothing may
// read; the effective weights come from the pre-pass's routine.  Prints one line per file and capacity; exit status 0 unless a file cannot be read, the forward refuses
// a cell, a row that fits comes out non-finite, or a refused one finite.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../radfoam_amd/csrc/rf_clip_box_area_grad.hpp"

namespace {

template <class T>
bool read_array(std::FILE *f, std::vector<T> &out, size_t count) {
    out.resize(count);
    return count == 0 || std::fread(out.data(), sizeof(T), count, f) == count;
}

int run_file(const char *path) {
    std::FILE *f = std::fopen(path, "rb");
    if (!f) return std::fprintf(stderr, "%s: cannot open\n", path), 2;
    uint32_t head[2];
    if (std::fread(head, sizeof(uint32_t), 2, f) != 2) return std::fclose(f), std::fprintf(stderr, "%s: short\n", path), 2;
    const uint32_t n = head[0], e = head[1];
    std::vector<float> points, bbox;
    std::vector<uint32_t> adj, offsets;
    std::vector<double> six;
    const bool ok = read_array(f, points, 3 * (size_t)n) && read_array(f, adj, e) && read_array(f, offsets, (size_t)n + 1) &&
                    read_array(f, bbox, 6) && read_array(f, six, 6);
    std::fclose(f);
    if (!ok) return std::fprintf(stderr, "%s: short\n", path), 2;
    const rf::clip::Box box = {six[0], six[1], six[2], six[3], six[4], six[5]};
    const double R = rf::clip::half_side_box(bbox.data(), box);
    std::vector<double> volume(n), centroid(3 * (size_t)n), face_area(e), wall_area(6 * (size_t)n), g(e), gw(6 * (size_t)n),
        G(e);
    std::vector<uint8_t> nonempty(n);
    {
        std::vector<double> s(512), t(512);
        std::vector<uint32_t> face_vertices(e), wall_vertices(6 * (size_t)n);
        for (uint32_t a = 0; a < n; ++a)
            if (rf::clip::cell_box_serial(points.data(), n, adj.data(), offsets.data(), e, a, box, R, s.data(), t.data(),
                                          256u, volume.data(), centroid.data(), nonempty.data(), face_area.data(),
                                          face_vertices.data(), wall_area.data(), wall_vertices.data()) != rf::clip::kCellOk)
                return std::fprintf(stderr, "%s: the forward refuses cell %u\n", path, a), 1;
    }
    uint32_t solid = 0;
    for (uint32_t a = 0; a < n; ++a) {
        solid += nonempty[a];
        const double unit = nonempty[a] ? 1.0 / std::cbrt(volume[a]) : 1.0;   // a flat cell has areas and no size
        for (uint32_t k = offsets[a]; k < offsets[a + 1]; ++k)
            g[k] = !(face_area[k] > 0.0) ? (double)NAN : (k & 1u) ? -unit : unit;
        for (uint32_t w = 0; w < 6; ++w)
            gw[6 * (size_t)a + w] = !(wall_area[6 * (size_t)a + w] > 0.0) ? (double)NAN : (w & 1u) ? -0.5 * unit : unit;
    }
    for (uint32_t a = 0; a < n; ++a)
        for (uint32_t k = offsets[a]; k < offsets[a + 1]; ++k)
            G[k] = rf::clip::effective_weight_box(adj.data(), offsets.data(), n, e, face_area.data(), g.data(), a, k);
    int rc = 0;
    for (uint32_t cap : {256u, 17u, 16u, 4u}) {
        std::vector<double> s(2 * (size_t)cap), t(2 * (size_t)cap), grad(3 * (size_t)n);
        std::vector<uint32_t> lab(2 * (size_t)cap);
        uint32_t refused = 0;
        double sum = 0.0;
        for (uint32_t a = 0; a < n; ++a) {
            const uint32_t status = rf::clip::cell_box_area_grad_serial(
                points.data(), n, adj.data(), offsets.data(), e, a, box, R, s.data(), t.data(), lab.data(), cap,
                nonempty.data(), face_area.data(), wall_area.data(), G.data(), gw.data(), grad.data());
            const double *row = grad.data() + 3 * (size_t)a;
            const bool finite = std::isfinite(row[0]) && std::isfinite(row[1]) && std::isfinite(row[2]);
            if (status != rf::clip::kCellOk) {
                ++refused;
                if (finite) rc = 1;   // a refused row is NaN
            } else {
                if (!finite) rc = 1;
                sum += std::fabs(row[0]) + std::fabs(row[1]) + std::fabs(row[2]);
            }
        }
        std::printf("%s: N = %u (%u non-empty), E = %u, capacity %u: %u rows refused, sum |grad| of the others = %.17g\n",
                    path, n, solid, e, cap, refused, sum);
    }
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
