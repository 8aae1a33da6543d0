// clip_box_moments_sanitize.cpp -- TEST HARNESS, not product: a stand-alone program (its own main, no Python) that runs
// rf::clip::cell_box_moments_serial of radfoam_amd/csrc/rf_clip_box_moments.hpp over clouds written out as plain arrays,
// meant to be built with the host sanitizers and run once on the CPU:
//
//     python -c "from tests.host_harness import clip_box_host as h; h.write_arrays('hub59', 'hub59.bin')"
//     g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//         -o clip_box_moments_sanitize tests/host_harness/clip_box_moments_sanitize.cpp
//     ./clip_box_moments_sanitize hub59.bin ring17.bin grid_bisectors.bin
//
// A file is: uint32 N, uint32 E, float points[3N], uint32 adj[E], uint32 offsets[N+1], float bbox[6], double box[6]
// (clip_box_host.write_arrays).  The geometry the moments need is rf::clip::cell_box_serial's at capacity 256.  Every
// cell is then run with polygon buffers of exactly 2 * cap doubles and output arrays of exactly 6N elements, for cap =
// 256 and for the small capacities at which cells start to be refused (17, 16 and 4, the square itself), so that a write
// past a buffer's end is a heap overflow the sanitizer sees.  Prints one line per file and capacity; exit status 0 unless
// a file cannot be read, a cell that fits comes out with a non-finite site moment, or a refused one with a finite number.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../radfoam_amd/csrc/rf_clip_box_moments.hpp"

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
    std::vector<double> volume(n), centroid(3 * (size_t)n), face_area(e), wall_area(6 * (size_t)n);
    std::vector<uint8_t> nonempty(n);
    std::vector<uint32_t> face_vertices(e), wall_vertices(6 * (size_t)n);
    {
        std::vector<double> s(2 * 256), t(2 * 256);
        for (uint32_t a = 0; a < n; ++a)
            if (rf::clip::cell_box_serial(points.data(), n, adj.data(), offsets.data(), e, a, box, R, s.data(), t.data(), 256u,
                                          volume.data(), centroid.data(), nonempty.data(), face_area.data(),
                                          face_vertices.data(), wall_area.data(), wall_vertices.data()) != rf::clip::kCellOk)
                return std::fprintf(stderr, "%s: cell %u has no geometry\n", path, a), 2;
    }
    int rc = 0;
    for (uint32_t cap : {256u, 17u, 16u, 4u}) {
        std::vector<double> s(2 * (size_t)cap), t(2 * (size_t)cap), site(6 * (size_t)n), central(6 * (size_t)n);
        uint32_t refused = 0;
        double sum = 0.0;
        for (uint32_t a = 0; a < n; ++a) {
            const uint32_t status = rf::clip::cell_box_moments_serial(
                points.data(), n, adj.data(), offsets.data(), e, a, box, R, s.data(), t.data(), cap, volume.data(),
                centroid.data(), nonempty.data(), site.data(), central.data());
            bool finite = true, any_finite = false;
            for (uint32_t k = 0; k < 6; ++k) {
                finite = finite && std::isfinite(site[6 * (size_t)a + k]);
                any_finite = any_finite || std::isfinite(site[6 * (size_t)a + k]) || std::isfinite(central[6 * (size_t)a + k]);
                if (nonempty[a]) finite = finite && std::isfinite(central[6 * (size_t)a + k]);
            }
            if (status != rf::clip::kCellOk) {
                ++refused;
                if (any_finite) rc = 1;   // a refused cell is NaN in all twelve
            } else {
                if (!finite) rc = 1;
                sum += site[6 * (size_t)a] + site[6 * (size_t)a + 1] + site[6 * (size_t)a + 2];
            }
        }
        std::printf("%s: N = %u, E = %u, capacity %u: %u cells refused, sum of the others' tr site_moment = %.17g\n", path,
                    n, e, cap, refused, sum);
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
