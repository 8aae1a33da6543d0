// clip_box_area_grad_host.cpp -- TEST HARNESS, not product: compiles radfoam_amd/csrc/rf_clip_box_area_grad.hpp (the
// pre-pass and the serial row of rf_cell_box_area_grad.hip, over the plane list of rf_clip_box.hpp and the edge arithmetic
// of rf_clip_area_grad.hpp) for the host, so that the point gradients of the boxed face and wall areas can be checked
// against the exact reference without a GPU.  Only tests/ loads the library this builds.
#include <cstdint>
#include <vector>

#include "../../radfoam_amd/csrc/rf_clip_box_area_grad.hpp"

extern "C" {

// The pre-pass (effective_weight_box of every slot of every well-formed row), then every row through
// rf::clip::cell_box_area_grad_serial with polygons of at most `cap` vertices; box: lo[3], hi[3]; grad_face_area /
// grad_wall_area may be null.  status[a] is the routine's return value; returns the number of rows not kCellOk.
int clip_box_area_grad_host_run(const float *points, uint32_t num_points, const uint32_t *adj, const uint32_t *offsets,
                                uint32_t num_edges, const float *bbox, const double *box, uint32_t cap,
                                const uint8_t *nonempty, const double *face_area, const double *wall_area,
                                const double *grad_face_area, const double *grad_wall_area, double *grad_points,
                                uint32_t *status) {
    const rf::clip::Box b = {box[0], box[1], box[2], box[3], box[4], box[5]};
    const double R = rf::clip::half_side_box(bbox, b);
    std::vector<double> s(2 * (size_t)cap), t(2 * (size_t)cap), G(num_edges, 0.0);
    std::vector<uint32_t> lab(2 * (size_t)cap);
    for (uint32_t a = 0; a < num_points; ++a) {
        const uint32_t begin = offsets[a], end = offsets[a + 1];
        if (begin > end || end > num_edges) continue;
        for (uint32_t k = begin; k < end; ++k)
            G[k] = rf::clip::effective_weight_box(adj, offsets, num_points, num_edges, face_area, grad_face_area, a, k);
    }
    int bad = 0;
    for (uint32_t a = 0; a < num_points; ++a) {
        status[a] = rf::clip::cell_box_area_grad_serial(points, num_points, adj, offsets, num_edges, a, b, R, s.data(),
                                                        t.data(), lab.data(), cap, nonempty, face_area, wall_area,
                                                        G.data(), grad_wall_area, grad_points);
        bad += status[a] != rf::clip::kCellOk;
    }
    return bad;
}

// The labelled polygon of row face i of cell a, as the serial row clips it: vertices in space relative to p_a (xyz[3 m])
// and labels (list indices, 0xffffffff for none).  Returns m, or -1 when it outgrew `cap`.
int clip_box_area_grad_host_polygon(const float *points, const uint32_t *adj, const uint32_t *offsets, const float *bbox,
                                    const double *box, uint32_t cap, uint32_t a, uint32_t i, double *xyz,
                                    uint32_t *labels) {
    const rf::clip::Box b = {box[0], box[1], box[2], box[3], box[4], box[5]};
    const double R = rf::clip::half_side_box(bbox, b);
    std::vector<double> s(2 * (size_t)cap), t(2 * (size_t)cap);
    std::vector<uint32_t> lab(2 * (size_t)cap);
    rf::clip::Frame frame;
    uint32_t m, cur;
    if (!rf::clip::face_polygon_box_labelled(points, adj, a, offsets[a], offsets[a + 1], b, i, R, s.data(), t.data(),
                                             lab.data(), 1u, cap, frame, m, cur))
        return -1;
    for (uint32_t v = 0; v < m; ++v) {
        rf::clip::to_space(frame, s[cur * cap + v], t[cur * cap + v], xyz[3 * v], xyz[3 * v + 1], xyz[3 * v + 2]);
        labels[v] = lab[cur * cap + v];
    }
    return (int)m;
}

// the unlabelled polygon of the same face in (s,t) against the labelled one: 1 when they are bit-identical
int clip_box_area_grad_host_same_vertices(const float *points, const uint32_t *adj, const uint32_t *offsets,
                                          const float *bbox, const double *box, uint32_t cap, uint32_t a, uint32_t i) {
    const rf::clip::Box b = {box[0], box[1], box[2], box[3], box[4], box[5]};
    const double R = rf::clip::half_side_box(bbox, b);
    std::vector<double> s(2 * (size_t)cap), t(2 * (size_t)cap), s2(2 * (size_t)cap), t2(2 * (size_t)cap);
    std::vector<uint32_t> lab(2 * (size_t)cap);
    rf::clip::Frame f1, f2;
    uint32_t m1, c1, m2, c2;
    bool wall;
    double h;
    const bool ok1 = rf::clip::face_polygon_box_labelled(points, adj, a, offsets[a], offsets[a + 1], b, i, R, s.data(),
                                                         t.data(), lab.data(), 1u, cap, f1, m1, c1);
    const bool ok2 = rf::clip::face_polygon_box(points, adj, a, offsets[a], offsets[a + 1], b, i, R, s2.data(), t2.data(),
                                                1u, cap, f2, wall, h, m2, c2);
    if (ok1 != ok2) return 0;
    if (!ok1) return 1;
    if (m1 != m2 || c1 != c2) return 0;
    for (uint32_t v = 0; v < m1; ++v)
        if (s[c1 * cap + v] != s2[c2 * cap + v] || t[c1 * cap + v] != t2[c2 * cap + v]) return 0;
    return 1;
}

}  // extern "C"
