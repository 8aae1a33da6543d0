// clip_moments_grad_sanitize.cpp -- TEST HARNESS, not product: a stand-alone program (its own main, no Python) that runs
// rf::clip::cell_moments_grad_serial of radfoam_amd/csrc/rf_clip_moments_grad.hpp over clouds written out as plain arrays,
// meant to be built with the host sanitizers and run once on the CPU:
//
//     python -c "from tests.host_harness import clip_moments_grad_host as h; h.write_arrays('hub65', 'hub65.bin')"
//     g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//         -o clip_moments_grad_sanitize tests/host_harness/clip_moments_grad_sanitize.cpp
//     ./clip_moments_grad_sanitize hub65.bin ring17.bin
//
// A file is: uint32 N, uint32 E, float points[3N], uint32 adj[E], uint32 offsets[N+1], float bbox[6], double volume[N],
// double centroid[3N], uint8 bounded[N], double grad_site_moment[6N], double grad_central_moment[6N].  Every row is run
// with polygon buffers of exactly 2 * cap doubles, for cap = 256 and for the small capacities at which rows start to be
// refused (17, 16 and 4, the square itself), so that a write past a buffer's end is a heap overflow the sanitizer sees.  Prints one line per
// file and capacity; exit status 0 unless a file cannot be read or a row that fits comes out non-finite.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../radfoam_amd/csrc/rf_clip_moments_grad.hpp"

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
    std::vector<double> volume, centroid, gq, gc;
    std::vector<uint8_t> bounded;
    const bool ok = read_array(f, points, 3 * (size_t)n) && read_array(f, adj, e) && read_array(f, offsets, (size_t)n + 1) &&
                    read_array(f, bbox, 6) && read_array(f, volume, n) && read_array(f, centroid, 3 * (size_t)n) &&
                    read_array(f, bounded, n) && read_array(f, gq, 6 * (size_t)n) && read_array(f, gc, 6 * (size_t)n);
    std::fclose(f);
    if (!ok) return std::fprintf(stderr, "%s: short\n", path), 2;
    const double R = rf::clip::half_side(bbox.data());
    int rc = 0;
    for (uint32_t cap : {256u, 17u, 16u, 4u}) {
        std::vector<double> s(2 * (size_t)cap), t(2 * (size_t)cap), grad(3 * (size_t)n);
        uint32_t refused = 0;
        double sum = 0.0;
        for (uint32_t a = 0; a < n; ++a) {
            const uint32_t status = rf::clip::cell_moments_grad_serial(
                points.data(), n, adj.data(), offsets.data(), e, a, R, s.data(), t.data(), cap, volume.data(),
                centroid.data(), bounded.data(), gq.data(), gc.data(), grad.data());
            const bool finite = std::isfinite(grad[3 * (size_t)a]) && std::isfinite(grad[3 * (size_t)a + 1]) &&
                                std::isfinite(grad[3 * (size_t)a + 2]);
            if (status != rf::clip::kCellOk) {
                ++refused;
                if (finite) rc = 1;   // a refused row is NaN
            } else {
                if (!finite) rc = 1;
                sum += std::fabs(grad[3 * (size_t)a]) + std::fabs(grad[3 * (size_t)a + 1]) + std::fabs(grad[3 * (size_t)a + 2]);
            }
        }
        // either upstream absent, at full capacity only
        if (cap == 256u)
            for (uint32_t a = 0; a < n; ++a) {
                rf::clip::cell_moments_grad_serial(points.data(), n, adj.data(), offsets.data(), e, a, R, s.data(), t.data(),
                                                   cap, volume.data(), centroid.data(), bounded.data(), gq.data(), nullptr,
                                                   grad.data());
                rf::clip::cell_moments_grad_serial(points.data(), n, adj.data(), offsets.data(), e, a, R, s.data(), t.data(),
                                                   cap, volume.data(), centroid.data(), bounded.data(), nullptr, gc.data(),
                                                   grad.data());
            }
        std::printf("%s: N = %u, E = %u, capacity %u: %u rows refused, sum |grad| of the others = %.17g\n", path, n, e, cap,
                    refused, sum);
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
