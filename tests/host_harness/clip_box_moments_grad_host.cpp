// clip_box_moments_grad_host.cpp -- TEST HARNESS, not product: compiles radfoam_amd/csrc/rf_clip_box_moments_grad.hpp
// (the serial row of rf_cell_box_moments_grad.hip, over the plane list of rf_clip_box.hpp and the per-face arithmetic of
// rf_clip_moments_grad.hpp) for the host, so that the point gradients of the boxed second moments can be checked against
// the exact reference without a GPU.  Only tests/ loads the library this builds.
#include <cstdint>
#include <vector>

#include "../../radfoam_amd/csrc/rf_clip_box_moments_grad.hpp"

extern "C" {

// every row through rf::clip::cell_box_moments_grad_serial with polygons of at most `cap` vertices; box: lo[3], hi[3];
// each of the four upstreams may be null.  status[a] is the routine's return value; returns the number of rows whose
// status is not kCellOk.
int clip_box_moments_grad_host_cell_box_moments_grad(const float *points, uint32_t num_points, const uint32_t *adj,
                                                     const uint32_t *offsets, uint32_t num_edges, const float *bbox,
                                                     const double *box, uint32_t cap, const double *volume,
                                                     const double *centroid, const uint8_t *nonempty,
                                                     const double *grad_site_moment, const double *grad_central_moment,
                                                     const double *grad_volume, const double *grad_centroid,
                                                     double *grad_points, uint32_t *status) {
    const rf::clip::Box b = {box[0], box[1], box[2], box[3], box[4], box[5]};
    const double R = rf::clip::half_side_box(bbox, b);
    std::vector<double> s(2 * (size_t)cap), t(2 * (size_t)cap);
    int bad = 0;
    for (uint32_t a = 0; a < num_points; ++a) {
        status[a] = rf::clip::cell_box_moments_grad_serial(points, num_points, adj, offsets, num_edges, a, b, R, s.data(),
                                                           t.data(), cap, volume, centroid, nonempty, grad_site_moment,
                                                           grad_central_moment, grad_volume, grad_centroid, grad_points);
        bad += status[a] != rf::clip::kCellOk;
    }
    return bad;
}

}  // extern "C"
