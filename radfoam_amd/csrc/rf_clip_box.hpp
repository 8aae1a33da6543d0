// rf_clip_box.hpp -- Voronoi cells clipped to an axis-aligned box (rf_cell_box.hip), on the clipping core of rf_clip.hpp
// and in double like it ("Cells clipped to a box").
//
// cell_box(a) = cell(a) n box.  Its planes are a LIST: the row's {d_c, |d_c|^2 / 2} in row order, then the six walls in
// wall order, wall 2k being x_k >= lo_k and wall 2k+1 x_k <= hi_k: a unit axis normal n_w and the SIGNED offset h_w =
// p_a,k - lo_k or hi_k - p_a,k, negative when the site is outside that wall.  Every plane of the list carries a face: the
// square of half-side R in that plane (centred on d_b / 2 for a row plane, on n_w h_w for a wall), clipped by every other
// plane of the list in list order.  R = 4 |diagonal of the bounding box of (all points u the box's corners)|, so the
// square covers the box's section with the plane, and once the walls have clipped a face nothing of the square is left:
// there is no unbounded outcome.  Pyramids over p_a have signed heights: area |d_b| / 6 for a row face, area h_w / 3 for a
// wall; their sum is the volume of cell_box(a) also for a site outside the box.
//
// Coincident planes: while face i is clipped, a plane j whose line in i's frame is exactly A == B == C == 0 and whose
// normal points the same way (d_i . d_j > 0) is the plane of face i itself.  The earlier of the two keeps the face: j < i
// empties face i, j > i is passed over (a row face wins over a wall).  With opposite normals both faces stay and their
// pyramids cancel: the cell is flat.  clip_step and the rest of rf_clip.hpp are used as they are.
//
// __host__ __device__ and free of HIP types, like rf_clip.hpp: tests/host_harness/clip_box_host.cpp compiles this file
// with g++.
#pragma once

#include "rf_clip.hpp"

namespace rf {
namespace clip {

struct Box {
    double lox, loy, loz, hix, hiy, hiz;
};

constexpr uint32_t kWalls = 6;

// R = 4 |diagonal| of the bounding box of the points (bbox: min[3], max[3]) and the box together
RF_CLIP_HD double half_side_box(const float *bbox, const Box &box) {
    const double ex = fmax((double)bbox[3], box.hix) - fmin((double)bbox[0], box.lox),
                 ey = fmax((double)bbox[4], box.hiy) - fmin((double)bbox[1], box.loy),
                 ez = fmax((double)bbox[5], box.hiz) - fmin((double)bbox[2], box.loz);
    return 4.0 * sqrt(ex * ex + ey * ey + ez * ez);
}

// wall w of the box relative to p_a: n . y <= h, n = -e_k (w = 2k) or +e_k (w = 2k + 1)
RF_CLIP_HD void wall_plane(const float *points, uint32_t a, const Box &box, uint32_t w, double &dx, double &dy,
                           double &dz, double &h) {
    // all six offsets as values and a choice among values: a choice among the box's members is a choice among
    // addresses to the compiler, which keeps the box in scratch on gfx950
    const double px = (double)points[3 * (size_t)a], py = (double)points[3 * (size_t)a + 1],
                 pz = (double)points[3 * (size_t)a + 2];
    const double h0 = px - box.lox, h1 = box.hix - px, h2 = py - box.loy, h3 = box.hiy - py, h4 = pz - box.loz,
                 h5 = box.hiz - pz;
    const uint32_t k = w >> 1;
    const double n = (w & 1u) != 0u ? 1.0 : -1.0;
    dx = k == 0u ? n : 0.0, dy = k == 1u ? n : 0.0, dz = k == 2u ? n : 0.0;
    h = w == 0u ? h0 : w == 1u ? h1 : w == 2u ? h2 : w == 3u ? h3 : w == 4u ? h4 : h5;
}

// plane `i` of the list of a valid row of `degree` entries starting at adjacency slot `begin`
RF_CLIP_HD void list_plane(const float *points, const uint32_t *adj, uint32_t a, uint32_t begin, uint32_t degree,
                           const Box &box, uint32_t i, double &dx, double &dy, double &dz, double &h) {
    if (i < degree) neighbour(points, a, adj[begin + i], dx, dy, dz, h);
    else wall_plane(points, a, box, i - degree, dx, dy, dz, h);
}

// the frame of a face of the list: a wall's is centred on n h and has len == 1
RF_CLIP_HD Frame list_frame(bool wall, double dx, double dy, double dz, double h) {
    Frame f = make_frame(dx, dy, dz);
    if (wall) f.cx = dx * h, f.cy = dy * h, f.cz = dz * h;
    return f;
}

// Face i (normal along (nx, ny, nz), frame `frame`) against plane j of the list, `earlier` saying j < i; the polygon is
// in buffer `cur` before and after.  This is where the tie rule lives.  false: more than cap vertices.
RF_CLIP_HD bool clip_by_list_plane(const Frame &frame, double nx, double ny, double nz, bool earlier, double dx, double dy,
                                   double dz, double h, double *s, double *t, uint32_t stride, uint32_t cap, uint32_t &m,
                                   uint32_t &cur) {
    double A, B, C;
    plane_in_frame(frame, dx, dy, dz, h, A, B, C);
    if (A == 0.0 && B == 0.0 && C == 0.0 && nx * dx + ny * dy + nz * dz > 0.0) {
        if (earlier) m = 0;
        return true;
    }
    const uint32_t in = cur * cap * stride, out = (cur ^ 1u) * cap * stride;
    if (!clip_step(s + in, t + in, s + out, t + out, stride, cap, m, A, B, C)) return false;
    cur ^= 1u;
    return true;
}

// face (area, 2-D centroid) -> its signed pyramid over p_a
RF_CLIP_HD void add_face_box(CellSums &c, const Frame &f, bool wall, double h, double area, double cs, double ct) {
    double x, y, z;
    to_space(f, cs, ct, x, y, z);
    const double v = wall ? area * h / 3.0 : area * f.len / 6.0;
    c.volume += v;
    c.mx += v * 0.75 * x, c.my += v * 0.75 * y, c.mz += v * 0.75 * z;
}

// The polygon of face `i` of the list (i < degree: adjacency slot begin + i; else wall i - degree) of a valid row,
// planes taken straight from the arrays.  The result is in buffer `cur`; `wall` and `h` are the face's own.
RF_CLIP_HD bool face_polygon_box(const float *points, const uint32_t *adj, uint32_t a, uint32_t begin, uint32_t end,
                                 const Box &box, uint32_t i, double R, double *s, double *t, uint32_t stride,
                                 uint32_t cap, Frame &frame, bool &wall, double &h, uint32_t &m, uint32_t &cur) {
    const uint32_t degree = end - begin, count = degree + kWalls;
    double nx, ny, nz;
    list_plane(points, adj, a, begin, degree, box, i, nx, ny, nz, h);
    wall = i >= degree;
    frame = list_frame(wall, nx, ny, nz, h);
    init_square(s, t, stride, R);
    m = 4, cur = 0;
    for (uint32_t j = 0; j < count && m != 0; ++j) {
        if (j == i) continue;
        double dx, dy, dz, hj;
        list_plane(points, adj, a, begin, degree, box, j, dx, dy, dz, hj);
        if (!clip_by_list_plane(frame, nx, ny, nz, j < i, dx, dy, dz, hj, s, t, stride, cap, m, cur)) return false;
    }
    return true;
}

// the cell of an empty row: the whole box
RF_CLIP_HD void whole_box(const Box &box, uint32_t a, double *volume, double *centroid, uint8_t *nonempty,
                          double *wall_area, uint32_t *wall_vertices) {
    const double ex = box.hix - box.lox, ey = box.hiy - box.loy, ez = box.hiz - box.loz;
    volume[a] = ex * ey * ez;
    centroid[3 * (size_t)a] = 0.5 * (box.lox + box.hix);
    centroid[3 * (size_t)a + 1] = 0.5 * (box.loy + box.hiy);
    centroid[3 * (size_t)a + 2] = 0.5 * (box.loz + box.hiz);
    nonempty[a] = 1;
    double *wa = wall_area + kWalls * (size_t)a;
    wa[0] = wa[1] = ey * ez, wa[2] = wa[3] = ex * ez, wa[4] = wa[5] = ex * ey;
    for (uint32_t w = 0; w < kWalls; ++w) wall_vertices[kWalls * (size_t)a + w] = 4u;
}

// what a cell's sums become: the signed volume as it is, the centroid where the volume is positive
RF_CLIP_HD void write_cell_box(const float *points, uint32_t a, const CellSums &sums, double *volume, double *centroid,
                               uint8_t *nonempty) {
    const bool ok = sums.volume > 0.0;
    const float *p = points + 3 * (size_t)a;
    volume[a] = sums.volume;
    centroid[3 * (size_t)a] = ok ? (double)p[0] + sums.mx / sums.volume : (double)NAN;
    centroid[3 * (size_t)a + 1] = ok ? (double)p[1] + sums.my / sums.volume : (double)NAN;
    centroid[3 * (size_t)a + 2] = ok ? (double)p[2] + sums.mz / sums.volume : (double)NAN;
    nonempty[a] = ok ? 1 : 0;
}

// One whole cell, face after face of its list (the host harness, and the kernel of last resort).  Writes face_area /
// face_vertices of the row, wall_area / wall_vertices [6] and the cell's volume, centroid[3], nonempty; returns a kCell*
// status (on a status other than kCellOk the outputs are NaN / 0 / false, still written).
RF_CLIP_HD uint32_t cell_box_serial(const float *points, uint32_t num_points, const uint32_t *adj, const uint32_t *offsets,
                                    uint32_t num_edges, uint32_t a, const Box &box, double R, double *s, double *t,
                                    uint32_t cap, double *volume, double *centroid, uint8_t *nonempty, double *face_area,
                                    uint32_t *face_vertices, double *wall_area, uint32_t *wall_vertices) {
    const uint32_t begin = offsets[a], end = offsets[a + 1];
    uint32_t status = row_is_valid(points, num_points, adj, num_edges, a, begin, end) ? kCellOk : kCellBadRow;
    if (status == kCellOk && begin == end) {
        whole_box(box, a, volume, centroid, nonempty, wall_area, wall_vertices);
        return status;
    }
    const uint32_t degree = status == kCellOk ? end - begin : 0u;
    CellSums sums = {0.0, 0.0, 0.0, 0.0, false};
    uint32_t i = 0;   // the first face of the list not written yet
    for (; status == kCellOk && i < degree + kWalls; ++i) {
        Frame frame;
        bool wall;
        double h;
        uint32_t m, cur;
        if (!face_polygon_box(points, adj, a, begin, end, box, i, R, s, t, 1u, cap, frame, wall, h, m, cur)) {
            status = kCellTooManyVertices;
            break;
        }
        double area, cs, ct;
        bool square;   // cannot be: the walls are in the list
        measure(s + cur * cap, t + cur * cap, 1u, m, R, area, cs, ct, square);
        add_face_box(sums, frame, wall, h, area, cs, ct);
        if (wall) wall_area[kWalls * (size_t)a + (i - degree)] = area, wall_vertices[kWalls * (size_t)a + (i - degree)] = m;
        else face_area[begin + i] = area, face_vertices[begin + i] = m;
    }
    if (status != kCellOk) {
        if (begin <= end && end <= num_edges) {
            const uint32_t rows = end - begin;
            for (uint32_t f = begin + (i < rows ? i : rows); f < end; ++f) face_area[f] = (double)NAN, face_vertices[f] = 0u;
            for (uint32_t w = i > rows ? i - rows : 0u; w < kWalls; ++w)
                wall_area[kWalls * (size_t)a + w] = (double)NAN, wall_vertices[kWalls * (size_t)a + w] = 0u;
        } else {
            for (uint32_t w = 0; w < kWalls; ++w)
                wall_area[kWalls * (size_t)a + w] = (double)NAN, wall_vertices[kWalls * (size_t)a + w] = 0u;
        }
        volume[a] = (double)NAN;
        centroid[3 * (size_t)a] = centroid[3 * (size_t)a + 1] = centroid[3 * (size_t)a + 2] = (double)NAN;
        nonempty[a] = 0;
        return status;
    }
    write_cell_box(points, a, sums, volume, centroid, nonempty);
    return status;
}

}  // namespace clip
}  // namespace rf
