// clip_mesh_host.cpp -- TEST HARNESS, not product: compiles radfoam_amd/csrc/rf_clip_mesh.hpp (the corner keys, the serial
// face of rf_cell_mesh.hip and the circumcentre arithmetic) for the host, so that the welded mesh can be checked without
// a GPU.  Only tests/ loads the library this builds.
#include <cstdint>
#include <vector>

#include "../../radfoam_amd/csrc/rf_clip_mesh.hpp"

extern "C" {

// the vertex count of the labelled polygon of adjacency slot `slot` of cell a, from the forward's square; -1 past cap
int clip_mesh_host_face_count(const float *points, const uint32_t *adj, const uint32_t *offsets, const float *bbox,
                              uint32_t a, uint32_t slot, uint32_t cap) {
    using namespace rf::clip;
    std::vector<double> s(2 * (size_t)cap), t(2 * (size_t)cap);
    std::vector<uint32_t> lab(2 * (size_t)cap);
    Frame frame;
    uint32_t m, cur;
    if (!face_polygon_labelled(points, adj, a, offsets[a], offsets[a + 1], slot, half_side(bbox), s.data(), t.data(),
                               lab.data(), 1u, cap, frame, m, cur))
        return -1;
    return (int)m;
}

// rf::clip::face_corners_serial of that face: xyz[3 * expect], sites[4 * expect]; returns its status
int clip_mesh_host_face_corners(const float *points, uint32_t num_points, const uint32_t *adj, const uint32_t *offsets,
                                uint32_t num_edges, const float *bbox, uint32_t a, uint32_t slot, uint32_t cap,
                                uint32_t expect, double *xyz, uint32_t *sites) {
    using namespace rf::clip;
    std::vector<double> s(2 * (size_t)cap), t(2 * (size_t)cap);
    std::vector<uint32_t> lab(2 * (size_t)cap);
    return (int)face_corners_serial(points, num_points, adj, offsets, num_edges, a, slot, half_side(bbox), s.data(),
                                    t.data(), lab.data(), cap, expect, xyz, sites);
}

void clip_mesh_host_vertices(const float *points, uint32_t num_points, const int64_t *vertex_sites,
                             uint32_t num_vertices, double *vertices) {
    for (uint32_t v = 0; v < num_vertices; ++v)
        rf::clip::key_vertex(points, num_points, vertex_sites + 4 * (size_t)v, vertices + 3 * (size_t)v);
}

// site_grad[V][4][3]
void clip_mesh_host_vertices_grad(const float *points, uint32_t num_points, const int64_t *vertex_sites,
                                  uint32_t num_vertices, const double *grad_vertices, double *site_grad) {
    for (uint32_t v = 0; v < num_vertices; ++v)
        rf::clip::key_vertex_grad(points, num_points, vertex_sites + 4 * (size_t)v, grad_vertices + 3 * (size_t)v,
                                  site_grad + 12 * (size_t)v);
}

}  // extern "C"
