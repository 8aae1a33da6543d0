// clip_moments_host.cpp -- TEST HARNESS, not product: compiles radfoam_amd/csrc/rf_clip_moments.hpp (the per-face
// arithmetic and the serial row of rf_cell_moments.hip) for the host, so that the second moments of the cells can be checked
// against the exact reference without a GPU.  Only tests/ loads the library this builds.
#include <cstdint>
#include <vector>

#include "../../radfoam_amd/csrc/rf_clip_moments.hpp"

extern "C" {

// every cell through rf::clip::cell_moments_serial with polygons of at most `cap` vertices.  status[a] is the routine's
// return value; returns the number of cells whose status is not kCellOk.
int clip_moments_host_cell_moments(const float *points, uint32_t num_points, const uint32_t *adj,
                                   const uint32_t *offsets, uint32_t num_edges, const float *bbox, uint32_t cap,
                                   const double *volume, const double *centroid, const uint8_t *bounded,
                                   double *site_moment, double *central_moment, uint32_t *status) {
    const double R = rf::clip::half_side(bbox);
    std::vector<double> s(2 * (size_t)cap), t(2 * (size_t)cap);
    int bad = 0;
    for (uint32_t a = 0; a < num_points; ++a) {
        status[a] = rf::clip::cell_moments_serial(points, num_points, adj, offsets, num_edges, a, R, s.data(), t.data(),
                                                  cap, volume, centroid, bounded, site_moment, central_moment);
        bad += status[a] != rf::clip::kCellOk;
    }
    return bad;
}

}  // extern "C"
