// clip_box_host.cpp -- TEST HARNESS, not product: compiles radfoam_amd/csrc/rf_clip_box.hpp (the plane list, the wall
// frames, the tie rule and the serial cell of rf_cell_box.hip) for the host, so that the cells clipped to a box can be
// checked against the exact reference without a GPU.  Only tests/ loads the library this builds.
#include <cstdint>
#include <vector>

#include "../../radfoam_amd/csrc/rf_clip_box.hpp"

extern "C" {

// every cell through rf::clip::cell_box_serial with polygons of at most `cap` vertices; box: lo[3], hi[3].  status[a] is
// the routine's return value; returns the number of cells whose status is not kCellOk.
int clip_box_host_cell_box(const float *points, uint32_t num_points, const uint32_t *adj, const uint32_t *offsets,
                           uint32_t num_edges, const float *bbox, const double *box, uint32_t cap, double *volume,
                           double *centroid, uint8_t *nonempty, double *face_area, uint32_t *face_vertices,
                           double *wall_area, uint32_t *wall_vertices, uint32_t *status) {
    const rf::clip::Box b = {box[0], box[1], box[2], box[3], box[4], box[5]};
    const double R = rf::clip::half_side_box(bbox, b);
    std::vector<double> s(2 * (size_t)cap), t(2 * (size_t)cap);
    int bad = 0;
    for (uint32_t a = 0; a < num_points; ++a) {
        status[a] = rf::clip::cell_box_serial(points, num_points, adj, offsets, num_edges, a, b, R, s.data(), t.data(), cap,
                                              volume, centroid, nonempty, face_area, face_vertices, wall_area,
                                              wall_vertices);
        bad += status[a] != rf::clip::kCellOk;
    }
    return bad;
}

}  // extern "C"
