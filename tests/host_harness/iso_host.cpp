// iso_host.cpp -- TEST HARNESS, not product: compiles radfoam_amd/csrc/rf_iso.hpp (the mask, the case rule, the winding,
// the keys, the vertex on an edge and its backward, as rf_isosurface.hip runs them) for the host, so that marching
// tetrahedra can be checked without a GPU.  Only tests/ loads the library this builds.
#include <cstdint>

#include "../../radfoam_amd/csrc/rf_iso.hpp"

extern "C" {

// counts[T]: the triangles of every tetrahedron; returns the first tetrahedron with an index out of range, or -1
int64_t iso_host_count(const int64_t *tets, uint32_t num_tets, const float *values, uint32_t num_points, double level,
                       uint8_t *counts) {
    int64_t first_bad = -1;
    for (uint32_t t = 0; t < num_tets; ++t) {
        int64_t s[4];
        counts[t] = 0;
        if (rf::iso::tet_sites(tets + 4 * (size_t)t, num_points, s))
            counts[t] = (uint8_t)rf::iso::mask_triangles(rf::iso::sites_mask(values, s, level));
        else if (first_bad < 0)
            first_bad = (int64_t)t;
    }
    return first_bad;
}

// keys[F*3], triangle_tet[F] with F the sum of counts, tetrahedron after tetrahedron
void iso_host_emit(const int64_t *tets, uint32_t num_tets, const float *points, const float *values, uint32_t num_points,
                   double level, const uint8_t *counts, int64_t *keys, int64_t *triangle_tet) {
    size_t first = 0;
    for (uint32_t t = 0; t < num_tets; ++t) {
        const uint32_t count = counts[t];
        if (count == 0u || count > 2u) continue;
        int64_t s[4];
        const bool in_range = rf::iso::tet_sites(tets + 4 * (size_t)t, num_points, s);
        rf::iso::tet_emit(points, values, in_range, s, level, count, keys + 3 * first);
        for (uint32_t f = 0; f < count; ++f) triangle_tet[first + f] = (int64_t)t;
        first += count;
    }
}

void iso_host_vertices(const float *points, const float *values, uint32_t num_points, const int64_t *vertex_sites,
                       uint32_t num_vertices, double level, double *vertices, double *vertex_t) {
    for (uint32_t v = 0; v < num_vertices; ++v)
        rf::iso::edge_vertex(points, values, num_points, vertex_sites + 2 * (size_t)v, level, vertices + 3 * (size_t)v,
                             vertex_t + v);
}

// site_grad[V][2][4]
void iso_host_vertices_grad(const float *points, const float *values, uint32_t num_points, const int64_t *vertex_sites,
                            uint32_t num_vertices, double level, const double *grad_vertices, double *site_grad) {
    for (uint32_t v = 0; v < num_vertices; ++v)
        rf::iso::edge_vertex_grad(points, values, num_points, vertex_sites + 2 * (size_t)v, level,
                                  grad_vertices + 3 * (size_t)v, site_grad + 8 * (size_t)v);
}

}  // extern "C"
