// rf_clip.hpp -- the clipping core of the Voronoi cell geometry (rf_cell_geometry.hip), in double.
//
// Cell a is the intersection of the half-spaces of its adjacency row: { x : d_c . x <= |d_c|^2 / 2 }, d_c = p_c - p_a,
// in coordinates relative to p_a (the differences of fp32 inputs are exact in double).  Face (a,b) starts as a square of
// half-side R centred on d_b / 2 in the bisector plane of (a,b), in 2-D coordinates (s,t) on an orthonormal basis (u,v)
// of that plane with u x v = d_b / |d_b|, and is clipped by every other plane of the row (Sutherland-Hodgman against a
// half-plane  A s + B t <= C).  The square is counter-clockwise in (s,t), so every polygon here is wound with its normal
// from a to b.  An intersection along a square edge keeps that coordinate exactly R (s0 + w * (s1 - s0) with s0 == s1),
// so "some surviving vertex has max(|s|,|t|) >= R" says exactly that a piece of the square survived: the face is
// unbounded.
//
// Everything is __host__ __device__ and free of HIP types: tests/host_harness/clip_host.cpp compiles this file with g++
// and runs the same arithmetic on the CPU (no FMA contraction on either side).  A polygon lives in two caller-owned
// buffers per coordinate (ping-pong), vertex i of a buffer at [i * stride]: stride 1 on the host and in the wave-per-cell
// kernel's serial path, 64 in the lane-per-face kernel (vertex-major LDS, lanes side by side).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RF_CLIP_HD __host__ __device__ __forceinline__
#else
#define RF_CLIP_HD inline
#endif

namespace rf {
namespace clip {

enum : uint32_t {
    kCellOk = 0,
    kCellTooManyVertices = 1,   // a face outgrew the polygon capacity of the last resort
    kCellBadRow = 2             // offsets out of order / an index past N / the site itself or a duplicate of it in the row
};

// basis and centre of the bisector plane of (a,b); u x v = n = d / |d|
struct Frame {
    double ux, uy, uz, vx, vy, vz, cx, cy, cz, len;
};

RF_CLIP_HD Frame make_frame(double dx, double dy, double dz) {
    Frame f;
    f.len = sqrt(dx * dx + dy * dy + dz * dz);
    const double nx = dx / f.len, ny = dy / f.len, nz = dz / f.len;
    const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
    double ux, uy, uz;   // n x e, e the axis n leans on least
    if (ax <= ay && ax <= az) {
        ux = 0.0, uy = nz, uz = -ny;
    } else if (ay <= az) {
        ux = -nz, uy = 0.0, uz = nx;
    } else {
        ux = ny, uy = -nx, uz = 0.0;
    }
    const double ul = sqrt(ux * ux + uy * uy + uz * uz);
    f.ux = ux / ul, f.uy = uy / ul, f.uz = uz / ul;
    f.vx = ny * f.uz - nz * f.uy, f.vy = nz * f.ux - nx * f.uz, f.vz = nx * f.uy - ny * f.ux;   // n x u
    f.cx = 0.5 * dx, f.cy = 0.5 * dy, f.cz = 0.5 * dz;
    return f;
}

// the half-space of neighbour c (d_c, h_c = |d_c|^2 / 2) in the face's coordinates: A s + B t <= C
RF_CLIP_HD void plane_in_frame(const Frame &f, double dx, double dy, double dz, double h, double &A, double &B,
                               double &C) {
    A = dx * f.ux + dy * f.uy + dz * f.uz;
    B = dx * f.vx + dy * f.vy + dz * f.vz;
    C = h - (dx * f.cx + dy * f.cy + dz * f.cz);
}

RF_CLIP_HD void init_square(double *s, double *t, uint32_t stride, double R) {
    s[0] = -R, t[0] = -R;
    s[stride] = R, t[stride] = -R;
    s[2 * stride] = R, t[2 * stride] = R;
    s[3 * stride] = -R, t[3 * stride] = R;
}

// One Sutherland-Hodgman step: (si,ti)[0..m) clipped by A s + B t <= C into (so,to); m becomes the new count.
// false: the result needs more than cap vertices (m is then meaningless).  A vertex exactly on the line is inside and is
// not emitted a second time as the crossing of an edge it ends.
RF_CLIP_HD bool clip_step(const double *si, const double *ti, double *so, double *to, uint32_t stride, uint32_t cap,
                          uint32_t &m, double A, double B, double C) {
    uint32_t k = 0;
    if (m == 0) return true;
    const double s0 = si[0], t0 = ti[0], e0 = (A * s0 + B * t0) - C;
    double sc = s0, tc = t0, ec = e0;
    for (uint32_t i = 0; i < m; ++i) {
        double sn = s0, tn = t0, en = e0;
        if (i + 1 < m) {
            sn = si[(i + 1) * stride], tn = ti[(i + 1) * stride];
            en = (A * sn + B * tn) - C;
        }
        const bool in_c = ec <= 0.0, in_n = en <= 0.0;
        if (in_c) {
            if (k == cap) return false;
            so[k * stride] = sc, to[k * stride] = tc;
            ++k;
        }
        if (in_c != in_n && ec != 0.0 && en != 0.0) {
            if (k == cap) return false;
            const double w = ec / (ec - en);
            so[k * stride] = sc + w * (sn - sc), to[k * stride] = tc + w * (tn - tc);
            ++k;
        }
        sc = sn, tc = tn, ec = en;
    }
    m = k;
    return true;
}

// shoelace area (as a fan about vertex 0), area centroid in (s,t), and whether a piece of the square survived
RF_CLIP_HD void measure(const double *s, const double *t, uint32_t stride, uint32_t m, double R, double &area,
                        double &cs, double &ct, bool &unbounded) {
    area = 0.0, cs = 0.0, ct = 0.0, unbounded = false;
    if (m == 0) return;
    const double s0 = s[0], t0 = t[0];
    double a2 = 0.0, ms = 0.0, mt = 0.0;
    double ps = 0.0, pt = 0.0;   // previous vertex relative to vertex 0
    for (uint32_t i = 0; i < m; ++i) {
        const double si = s[i * stride], ti = t[i * stride];
        unbounded = unbounded || fmax(fabs(si), fabs(ti)) >= R;
        const double qs = si - s0, qt = ti - t0;
        if (i >= 2) {
            const double cr = ps * qt - pt * qs;
            a2 += cr;
            ms += cr * (ps + qs);
            mt += cr * (pt + qt);
        }
        ps = qs, pt = qt;
    }
    area = 0.5 * a2;
    if (a2 > 0.0) {
        cs = s0 + ms / (3.0 * a2);
        ct = t0 + mt / (3.0 * a2);
    }
}

RF_CLIP_HD void to_space(const Frame &f, double s, double t, double &x, double &y, double &z) {
    x = f.cx + s * f.ux + t * f.vx;
    y = f.cy + s * f.uy + t * f.vy;
    z = f.cz + s * f.uz + t * f.vz;
}

// what a cell accumulates over its faces
struct CellSums {
    double volume, mx, my, mz;   // sum V_b, sum V_b * 3/4 * c_b
    bool unbounded;
};

// face (area, 2-D centroid) -> its pyramid over p_a: V_b = area |d_b| / 6, centroid 3/4 of the way to the face's
RF_CLIP_HD void add_face(CellSums &c, const Frame &f, double area, double cs, double ct, bool unbounded) {
    if (unbounded) {
        c.unbounded = true;
        return;
    }
    double x, y, z;
    to_space(f, cs, ct, x, y, z);
    const double v = area * f.len / 6.0;
    c.volume += v;
    c.mx += v * 0.75 * x, c.my += v * 0.75 * y, c.mz += v * 0.75 * z;
}

RF_CLIP_HD double half_side(const float *bbox) {   // bbox: min[3], max[3] of all points; R = 4 |diagonal|
    const double ex = (double)bbox[3] - (double)bbox[0], ey = (double)bbox[4] - (double)bbox[1],
                 ez = (double)bbox[5] - (double)bbox[2];
    return 4.0 * sqrt(ex * ex + ey * ey + ez * ez);
}

RF_CLIP_HD void neighbour(const float *points, uint32_t a, uint32_t q, double &dx, double &dy, double &dz, double &h) {
    dx = (double)points[3 * (size_t)q] - (double)points[3 * (size_t)a];
    dy = (double)points[3 * (size_t)q + 1] - (double)points[3 * (size_t)a + 1];
    dz = (double)points[3 * (size_t)q + 2] - (double)points[3 * (size_t)a + 2];
    h = 0.5 * (dx * dx + dy * dy + dz * dz);
}

// a row the geometry is defined for: offsets in order and inside the list, every entry another, distinct site
RF_CLIP_HD bool row_is_valid(const float *points, uint32_t num_points, const uint32_t *adj, uint32_t num_edges,
                             uint32_t a, uint32_t begin, uint32_t end) {
    if (begin > end || end > num_edges) return false;
    for (uint32_t f = begin; f < end; ++f) {
        const uint32_t q = adj[f];
        if (q >= num_points || q == a) return false;
        double dx, dy, dz, h;
        neighbour(points, a, q, dx, dy, dz, h);
        if (!(h > 0.0)) return false;
    }
    return true;
}

// The polygon of face `slot` (begin <= slot < end) of a valid row, planes taken straight from the arrays.  The result is
// in buffer `cur` (0 or 1): s + cur * cap * stride.  false: more than cap vertices along the way.
RF_CLIP_HD bool face_polygon(const float *points, const uint32_t *adj, uint32_t a, uint32_t begin, uint32_t end,
                             uint32_t slot, double R, double *s, double *t, uint32_t stride, uint32_t cap, Frame &frame,
                             uint32_t &m, uint32_t &cur) {
    double dx, dy, dz, h;
    neighbour(points, a, adj[slot], dx, dy, dz, h);
    frame = make_frame(dx, dy, dz);
    init_square(s, t, stride, R);
    m = 4, cur = 0;
    for (uint32_t f = begin; f < end && m != 0; ++f) {
        if (f == slot) continue;
        double A, B, C;
        neighbour(points, a, adj[f], dx, dy, dz, h);
        plane_in_frame(frame, dx, dy, dz, h, A, B, C);
        const uint32_t in = cur * cap * stride, out = (cur ^ 1u) * cap * stride;
        if (!clip_step(s + in, t + in, s + out, t + out, stride, cap, m, A, B, C)) return false;
        cur ^= 1u;
    }
    return true;
}

// One whole cell, face after face (the host harness, and the kernel of last resort for rows and faces the lane-per-face
// kernel does not take).  Writes face_area / face_vertices of the row and the cell's volume, centroid[3], bounded;
// returns a kCell* status (on a status other than kCellOk the outputs are NaN / 0 / false, still written).
RF_CLIP_HD uint32_t cell_serial(const float *points, uint32_t num_points, const uint32_t *adj, const uint32_t *offsets,
                                uint32_t num_edges, uint32_t a, double R, double *s, double *t, uint32_t cap,
                                double *volume, double *centroid, uint8_t *bounded, double *face_area,
                                uint32_t *face_vertices) {
    const uint32_t begin = offsets[a], end = offsets[a + 1];
    uint32_t status = row_is_valid(points, num_points, adj, num_edges, a, begin, end) ? kCellOk : kCellBadRow;
    CellSums sums = {0.0, 0.0, 0.0, 0.0, begin == end};
    uint32_t slot = begin;   // the first face not written yet
    for (; status == kCellOk && slot < end; ++slot) {
        Frame frame;
        uint32_t m, cur;
        if (!face_polygon(points, adj, a, begin, end, slot, R, s, t, 1u, cap, frame, m, cur)) {
            status = kCellTooManyVertices;
            break;
        }
        double area, cs, ct;
        bool unbounded;
        measure(s + cur * cap, t + cur * cap, 1u, m, R, area, cs, ct, unbounded);
        add_face(sums, frame, area, cs, ct, unbounded);
        face_area[slot] = unbounded ? (double)INFINITY : area;
        face_vertices[slot] = m;
    }
    if (status != kCellOk) {
        if (begin <= end && end <= num_edges)
            for (; slot < end; ++slot) face_area[slot] = (double)NAN, face_vertices[slot] = 0u;
        volume[a] = (double)NAN;
        centroid[3 * (size_t)a] = centroid[3 * (size_t)a + 1] = centroid[3 * (size_t)a + 2] = (double)NAN;
        bounded[a] = 0;
        return status;
    }
    const bool ok = !sums.unbounded;
    volume[a] = ok ? sums.volume : (double)INFINITY;
    const float *p = points + 3 * (size_t)a;
    centroid[3 * (size_t)a] = ok ? (double)p[0] + sums.mx / sums.volume : (double)NAN;
    centroid[3 * (size_t)a + 1] = ok ? (double)p[1] + sums.my / sums.volume : (double)NAN;
    centroid[3 * (size_t)a + 2] = ok ? (double)p[2] + sums.mz / sums.volume : (double)NAN;
    bounded[a] = ok ? 1 : 0;
    return status;
}

}  // namespace clip
}  // namespace rf
