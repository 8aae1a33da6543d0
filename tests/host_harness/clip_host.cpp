// clip_host.cpp -- TEST HARNESS, not product: compiles radfoam_amd/csrc/rf_clip.hpp (the clipping core the kernels of
// rf_cell_geometry.hip run) for the host, so that its numerics can be checked against Qhull without a GPU.  Only tests/
// loads the library this builds; nothing under radfoam_amd/ does.
#include <cstdint>
#include <vector>

#include "../../radfoam_amd/csrc/rf_clip.hpp"

extern "C" {

// every cell through rf::clip::cell_serial with polygons of at most `cap` vertices; status[a] is its return value.
// Returns the number of cells whose status is not kCellOk.
int clip_host_cell_geometry(const float *points, uint32_t num_points, const uint32_t *adj, const uint32_t *offsets,
                            uint32_t num_edges, const float *bbox, uint32_t cap, double *volume, double *centroid,
                            uint8_t *bounded, double *face_area, uint32_t *face_vertices, uint32_t *status) {
    const double R = rf::clip::half_side(bbox);
    std::vector<double> s(2 * (size_t)cap), t(2 * (size_t)cap);
    int bad = 0;
    for (uint32_t a = 0; a < num_points; ++a) {
        status[a] = rf::clip::cell_serial(points, num_points, adj, offsets, num_edges, a, R, s.data(), t.data(), cap,
                                          volume, centroid, bounded, face_area, face_vertices);
        bad += status[a] != rf::clip::kCellOk;
    }
    return bad;
}

// the polygon of one face (adjacency slot `slot` of cell a) in space, relative to nothing: absolute coordinates,
// xyz[3 * i ..]; returns the vertex count, or -1 when it outgrew cap
int clip_host_face_polygon(const float *points, const uint32_t *adj, const uint32_t *offsets, const float *bbox,
                           uint32_t a, uint32_t slot, uint32_t cap, double *xyz) {
    const double R = rf::clip::half_side(bbox);
    std::vector<double> s(2 * (size_t)cap), t(2 * (size_t)cap);
    rf::clip::Frame frame;
    uint32_t m, cur;
    if (!rf::clip::face_polygon(points, adj, a, offsets[a], offsets[a + 1], slot, R, s.data(), t.data(), 1u, cap, frame,
                                m, cur))
        return -1;
    for (uint32_t i = 0; i < m; ++i) {
        double x, y, z;
        rf::clip::to_space(frame, s[cur * cap + i], t[cur * cap + i], x, y, z);
        xyz[3 * i] = (double)points[3 * (size_t)a] + x;
        xyz[3 * i + 1] = (double)points[3 * (size_t)a + 1] + y;
        xyz[3 * i + 2] = (double)points[3 * (size_t)a + 2] + z;
    }
    return (int)m;
}

}  // extern "C"
