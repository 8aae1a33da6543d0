// clip_moments_grad_host.cpp -- TEST HARNESS, not product: compiles radfoam_amd/csrc/rf_clip_moments_grad.hpp (the
// per-face arithmetic and the serial row of rf_cell_moments_grad.hip) for the host, so that the point gradients of the
// second moments can be checked against the exact reference without a GPU.  Only tests/ loads the library this builds.
#include <cstdint>
#include <vector>

#include "../../radfoam_amd/csrc/rf_clip_moments_grad.hpp"

extern "C" {

// every row through rf::clip::cell_moments_grad_serial with polygons of at most `cap` vertices; either upstream may be
// null.  status[a] is the routine's return value; returns the number of rows whose status is not kCellOk.
int clip_moments_grad_host_cell_moments_grad(const float *points, uint32_t num_points, const uint32_t *adj,
                                             const uint32_t *offsets, uint32_t num_edges, const float *bbox,
                                             uint32_t cap, const double *volume, const double *centroid,
                                             const uint8_t *bounded, const double *grad_site_moment,
                                             const double *grad_central_moment, double *grad_points,
                                             uint32_t *status) {
    const double R = rf::clip::half_side(bbox);
    std::vector<double> s(2 * (size_t)cap), t(2 * (size_t)cap);
    int bad = 0;
    for (uint32_t a = 0; a < num_points; ++a) {
        status[a] = rf::clip::cell_moments_grad_serial(points, num_points, adj, offsets, num_edges, a, R, s.data(),
                                                       t.data(), cap, volume, centroid, bounded, grad_site_moment,
                                                       grad_central_moment, grad_points);
        bad += status[a] != rf::clip::kCellOk;
    }
    return bad;
}

// rf::clip::moments3 of the polygon (s, t)[0..m) as it stands: out = a, s, t, ss, st, tt, sss, sst, stt, ttt, all about
// vertex 0.  Returns whether a vertex reaches R.
int clip_moments_grad_host_moments3(const double *s, const double *t, uint32_t m, double R, double *out) {
    const rf::clip::Moments3 o = rf::clip::moments3(s, t, 1u, m, R);
    out[0] = o.m.a, out[1] = o.m.s, out[2] = o.m.t, out[3] = o.m.ss, out[4] = o.m.st, out[5] = o.m.tt;
    out[6] = o.sss, out[7] = o.sst, out[8] = o.stt, out[9] = o.ttt;
    return o.m.unbounded ? 1 : 0;
}

}  // extern "C"
