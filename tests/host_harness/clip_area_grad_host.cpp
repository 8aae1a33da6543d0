// clip_area_grad_host.cpp -- TEST HARNESS, not product: compiles radfoam_amd/csrc/rf_clip_area_grad.hpp (the labelled
// clipping, the per-edge arithmetic and the serial row of rf_face_area_grad.hip) for the host, so that the point
// gradients of the face areas can be checked against the exact reference without a GPU.  Only tests/ loads the library
// this builds.
#include <cstdint>
#include <vector>

#include "../../radfoam_amd/csrc/rf_clip_area_grad.hpp"

extern "C" {

// the pre-pass (rf::clip::effective_weight of every slot into weight[E]) and every row through
// rf::clip::face_area_grad_serial with polygons of at most `cap` vertices.  status[a] is the routine's return value;
// returns the number of rows whose status is not kCellOk.
int clip_area_grad_host_face_area_grad(const float *points, uint32_t num_points, const uint32_t *adj,
                                       const uint32_t *offsets, uint32_t num_edges, const float *bbox, uint32_t cap,
                                       const double *face_area, const double *grad_face_area, double *weight,
                                       double *grad_points, uint32_t *status) {
    using namespace rf::clip;
    const double R = area_grad_half_side(bbox);
    for (uint32_t a = 0; a < num_points; ++a) {
        const uint32_t begin = offsets[a], end = offsets[a + 1];
        if (begin > end || end > num_edges) continue;
        for (uint32_t k = begin; k < end; ++k)
            weight[k] = effective_weight(adj, offsets, num_points, num_edges, face_area, grad_face_area, a, k);
    }
    std::vector<double> s(2 * (size_t)cap), t(2 * (size_t)cap);
    std::vector<uint32_t> lab(2 * (size_t)cap);
    int bad = 0;
    for (uint32_t a = 0; a < num_points; ++a) {
        status[a] = face_area_grad_serial(points, num_points, adj, offsets, num_edges, a, R, s.data(), t.data(),
                                          lab.data(), cap, face_area, weight, grad_points);
        bad += status[a] != kCellOk;
    }
    return bad;
}

// the labelled polygon of one face (adjacency slot `slot` of cell a): st[2 * i ..] the vertices in the face's own (s,t)
// coordinates, xyz[3 * i ..] the same relative to p_a, label[i] the row index of the plane the edge from vertex i to
// vertex i + 1 lies on (0xffffffff: the square), plain[2 * i ..] the vertices of rf::clip::face_polygon (unlabelled)
// and *plain_count their number.  Returns the vertex count, or -1 when either polygon outgrew cap.
int clip_area_grad_host_labelled_polygon(const float *points, const uint32_t *adj, const uint32_t *offsets,
                                         const float *bbox, uint32_t a, uint32_t slot, uint32_t cap, double *st,
                                         double *xyz, uint32_t *label, double *plain, uint32_t *plain_count) {
    using namespace rf::clip;
    const double R = area_grad_half_side(bbox);
    std::vector<double> s(2 * (size_t)cap), t(2 * (size_t)cap);
    std::vector<uint32_t> lab(2 * (size_t)cap);
    Frame frame;
    uint32_t m, cur;
    if (!face_polygon(points, adj, a, offsets[a], offsets[a + 1], slot, R, s.data(), t.data(), 1u, cap, frame, m, cur))
        return -1;
    *plain_count = m;
    for (uint32_t i = 0; i < m; ++i) plain[2 * i] = s[cur * cap + i], plain[2 * i + 1] = t[cur * cap + i];
    if (!face_polygon_labelled(points, adj, a, offsets[a], offsets[a + 1], slot, R, s.data(), t.data(), lab.data(), 1u,
                               cap, frame, m, cur))
        return -1;
    for (uint32_t i = 0; i < m; ++i) {
        st[2 * i] = s[cur * cap + i], st[2 * i + 1] = t[cur * cap + i];
        to_space(frame, st[2 * i], st[2 * i + 1], xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
        label[i] = lab[cur * cap + i];
    }
    return (int)m;
}

}  // extern "C"
