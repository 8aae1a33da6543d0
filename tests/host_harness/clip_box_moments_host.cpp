// clip_box_moments_host.cpp -- TEST HARNESS, not product: compiles radfoam_amd/csrc/rf_clip_box_moments.hpp (the signed
// pyramids, the whole-box closed form and the serial cell of rf_cell_box_moments.hip) for the host, so that the second
// moments of the cells clipped to a box can be checked against the exact reference without a GPU.  Only tests/ loads the
// library this builds.
#include <cstdint>
#include <vector>

#include "../../radfoam_amd/csrc/rf_clip_box_moments.hpp"

extern "C" {

// every cell through rf::clip::cell_box_moments_serial with polygons of at most `cap` vertices; box: lo[3], hi[3];
// volume / centroid / nonempty: what the serial boxed cell wrote.  status[a] is the routine's return value; returns the
// number of cells whose status is not kCellOk.
int clip_box_moments_host_cell_box_moments(const float *points, uint32_t num_points, const uint32_t *adj,
                                           const uint32_t *offsets, uint32_t num_edges, const float *bbox,
                                           const double *box, uint32_t cap, const double *volume, const double *centroid,
                                           const uint8_t *nonempty, double *site_moment, double *central_moment,
                                           uint32_t *status) {
    const rf::clip::Box b = {box[0], box[1], box[2], box[3], box[4], box[5]};
    const double R = rf::clip::half_side_box(bbox, b);
    std::vector<double> s(2 * (size_t)cap), t(2 * (size_t)cap);
    int bad = 0;
    for (uint32_t a = 0; a < num_points; ++a) {
        status[a] = rf::clip::cell_box_moments_serial(points, num_points, adj, offsets, num_edges, a, b, R, s.data(),
                                                      t.data(), cap, volume, centroid, nonempty, site_moment,
                                                      central_moment);
        bad += status[a] != rf::clip::kCellOk;
    }
    return bad;
}

}  // extern "C"
