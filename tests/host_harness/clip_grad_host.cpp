// clip_grad_host.cpp -- TEST HARNESS, not product: compiles radfoam_amd/csrc/rf_clip_grad.hpp (the per-face arithmetic
// and the serial row of rf_cell_geometry_grad.hip) for the host, so that the point gradients of the cell geometry can be
// checked against the exact reference without a GPU.  Only tests/ loads the library this builds.
#include <cstdint>
#include <vector>

#include "../../radfoam_amd/csrc/rf_clip_grad.hpp"

extern "C" {

// every row through rf::clip::cell_grad_serial with polygons of at most `cap` vertices; grad_volume / grad_centroid may
// be null.  status[a] is the routine's return value; returns the number of rows whose status is not kCellOk.
int clip_grad_host_cell_geometry_grad(const float *points, uint32_t num_points, const uint32_t *adj,
                                      const uint32_t *offsets, uint32_t num_edges, const float *bbox, uint32_t cap,
                                      const double *volume, const double *centroid, const uint8_t *bounded,
                                      const double *grad_volume, const double *grad_centroid, double *grad_points,
                                      uint32_t *status) {
    const double R = rf::clip::half_side(bbox);
    std::vector<double> s(2 * (size_t)cap), t(2 * (size_t)cap);
    int bad = 0;
    for (uint32_t a = 0; a < num_points; ++a) {
        status[a] = rf::clip::cell_grad_serial(points, num_points, adj, offsets, num_edges, a, R, s.data(), t.data(), cap,
                                               volume, centroid, bounded, grad_volume, grad_centroid, grad_points);
        bad += status[a] != rf::clip::kCellOk;
    }
    return bad;
}

// the moments of one face (adjacency slot `slot` of cell a) in space, in y = x - p_a: out = A, m[3] = int y dA,
// S[6] = int y y^T dA as xx, xy, xz, yy, yz, zz.  Returns the vertex count, or -1 when the polygon outgrew cap.
int clip_grad_host_face_moments(const float *points, const uint32_t *adj, const uint32_t *offsets, const float *bbox,
                                uint32_t a, uint32_t slot, uint32_t cap, double *out) {
    using namespace rf::clip;
    const double R = half_side(bbox);
    std::vector<double> s(2 * (size_t)cap), t(2 * (size_t)cap);
    Frame f;
    uint32_t m, cur;
    if (!face_polygon(points, adj, a, offsets[a], offsets[a + 1], slot, R, s.data(), t.data(), 1u, cap, f, m, cur))
        return -1;
    const Moments mo = moments(s.data() + cur * cap, t.data() + cur * cap, 1u, m, R);
    double y[3];
    to_space(f, mo.s0, mo.t0, y[0], y[1], y[2]);
    const double u[3] = {f.ux, f.uy, f.uz}, v[3] = {f.vx, f.vy, f.vz};
    out[0] = mo.a;
    for (int i = 0; i < 3; ++i) out[1 + i] = mo.a * y[i] + mo.s * u[i] + mo.t * v[i];
    int k = 4;
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j)
            out[k++] = mo.a * y[i] * y[j] + mo.s * (y[i] * u[j] + u[i] * y[j]) + mo.t * (y[i] * v[j] + v[i] * y[j]) +
                       mo.ss * u[i] * u[j] + mo.st * (u[i] * v[j] + v[i] * u[j]) + mo.tt * v[i] * v[j];
    return (int)m;
}

}  // extern "C"
