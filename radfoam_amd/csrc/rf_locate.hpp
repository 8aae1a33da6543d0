// rf_locate.hpp -- the Delaunay field at any point: the walk that finds the tetrahedron of a query, and the linear
// interpolation of per-site values inside it with its backward (rf_locate.hip; DESIGN.md, "Point location and
// interpolation").  Stated once for the kernels, the host build of tests/host_harness and the restatement of
// radfoam_amd/locate.py, so that the three can be compared for equality.
//
//   face sign     for a row (s0,s1,s2,s3) and a query q, sigma_j is the exact sign of the row's determinant
//                 det[p1 - p0; p2 - p0; p3 - p0] with corner j replaced by q.  One call of star::orient_sign(i, a, b, c)
//                 (the sign of det[a - i; b - i; c - i]) per face, the four points permuted evenly so that q comes first:
//                     sigma_0 = orient(q, p1, p2, p3)      sigma_1 = orient(q, p0, p3, p2)
//                     sigma_2 = orient(q, p0, p1, p3)      sigma_3 = orient(q, p1, p0, p2)
//                 Queries are float32 like the sites, so the predicate is as exact for them as for the triangulation:
//                 fp64 with a forward error bound, 384-bit integers below it.  Its documented limit applies to the
//                 queries too: a coordinate whose last bit lies more than 38 binary places below the last bit of the
//                 coarsest coordinate of the same predicate is snapped to that predicate's grid (star::to_grid).
//   step          at tetrahedron t take the lowest j with sigma_j < 0 and read tet_adjacency[t][j]: the hull word
//                 0xFFFFFFFF (-1 in int64 tables) ends the walk with -1, the query is outside the hull; anything else
//                 is 4 t' + j' and the walk goes to t' = entry >> 2.  With no negative sigma_j the closed tetrahedron t
//                 contains q and is the result; with all four zero the row is flat, a fault.  The four face determinants
//                 add up to the row's own, so four non-negative signs that are not all zero imply a positive row: a
//                 returned t >= 0 contains its query exactly, whatever the tables hold.  -1 is only right for
//                 conforming input (positive rows that triangulate a convex hull).
//   hops          the faces crossed.  A walk that would cross more than max_hops faces is a fault; that count is the
//                 only bound of the loop.  A query with a coordinate that is not finite gets -1 and 0 hops, no walk.
//   faults        every index read from memory is checked before it is used: a start outside [0,T), a corner outside
//                 [0,N), an adjacency entry that is neither the hull word nor below 4T, a flat row, the hop cap.  The
//                 result of such a query is fault_code(kind, t) < -1, which names the kind and the row.
//
//   interpolation all in double, nothing fused, in this order (differences of float32 are exact in double):
//                     d_i = p_si - p_s0 (i = 1..3),  x = q - p_s0
//                     n_1 = d_2 x d_3,  n_2 = d_3 x d_1,  n_3 = d_1 x d_2      (a x b)_x = a_y b_z - a_z b_y, cyclic
//                     det = (d_1x n_1x + d_1y n_1y) + d_1z n_1z
//                     w_i = ((n_ix x_x + n_iy x_y) + n_iz x_z) / det (i = 1..3),  w_0 = 1 - ((w_1 + w_2) + w_3)
//                     g_k = (((v_1 - v_0) n_1k + (v_2 - v_0) n_2k) + (v_3 - v_0) n_3k) / det
//                     value = v_0 + ((g_x x_x + g_y x_y) + g_z x_z)
//                 per channel.  Weights are not clamped.  tet outside [0,T), a corner out of range, det == 0 or a result
//                 that is not finite: NaN in all outputs of the query, nothing backward.
//   backward      for the upstream G_c of value_c:  h = sum_c G_c g_c (from 0.0, channels ascending),
//                     grad q = h,   grad p_si = -(w_i h),   grad v_si,c = G_c w_i
//                 the four corners' parts are f64[4][3 + C]; all dropped together when one term is not finite.
//
// The includer defines RF_STAR_FN / RF_STAR_NOINLINE / RF_STAR_NOUNROLL as rf_star.hpp asks; no HIP types.
#pragma once

#include <math.h>
#include <stdint.h>

#include "rf_star.hpp"

#ifndef RF_LOCATE_TRACE_FACE   // instrumentation hook of the host harness: the four points of every predicate
#define RF_LOCATE_TRACE_FACE(pi, pa, pb, pc) ((void)0)
#endif

namespace rf {
namespace locate {

constexpr uint32_t kHull = 0xFFFFFFFFu;
constexpr int64_t kOutside = -1;
constexpr uint32_t kMaxTets = 0x3FFFFFFFu;   // 4T stays below the hull word
constexpr uint32_t kMaxChannels = 8;          // the widest value table the kernels serve

enum Fault : uint32_t { kBadRow = 0, kBadAdjacency = 1, kFlatRow = 2, kBadStart = 3, kHopCap = 4 };

// what a faulted query gets in place of a tetrahedron: below -1; kind = (-2 - code) & 7, row = (-2 - code) >> 3
RF_STAR_FN int64_t fault_code(uint32_t kind, int64_t row) { return -2 - ((int64_t)kind + 8 * row); }

// The forward error of the spelled order, u = 2^-53 per rounding, first order.  The differences d_i and x are exact.
// Write |n|_i for n_i with its two products added in absolute value, A_i = sum_k |n|_ik |x_k| (the absolute terms of
// the numerator of w_i) and perm = sum_k |d_1k| |n|_1k (those of det).  A component of n_i carries 2 roundings relative
// to |n|_ik (a product, the difference), its product with x_k one more, the two sums of the dot product two more: the
// numerator is within 5 u A_i, det within 5 u perm; the quotient rounds once.  Since perm >= |det|,
//     |err w_i| <= (5 u A_i + 5 u |w_i| perm) / |det| + u |w_i| <= 7 u (A_i + |w_i| perm) / |det|      (i = 1..3)
//     |err w_0| <= sum_i |err w_i| + 3 u (1 + |w_1| + |w_2| + |w_3|)
// kWeightBound leaves a factor of two on the count of 7:  tol_i = kWeightBound (A_i + |w_i| perm) / |det|,
// tol_0 = tol_1 + tol_2 + tol_3 + kWeightBound (1 + |w_1| + |w_2| + |w_3|).  perm / |det| is what a sliver pays.
constexpr double kWeightBound = 2.0e-15;   // > 2 * 7 * 2^-53
// The value, for values of magnitude M at most (so |v_i - v_0| <= 2 M, rounded once for float64 values): a term of a
// numerator of g carries 4 roundings and the sums 2, the division by det 5 u perm / |det| and one more: g_k is within
// 2 M * 12 u (perm / |det|) sum_i |n|_ik / |det|; the dot product with x adds 3 u, the last sum one rounding of the
// result:  |err value| <= 2 M * 15 u (perm / |det|) (A_1 + A_2 + A_3) / |det| + u max(M, |value|).
// kValueBound leaves a factor of two:  tol = M (kValueBound (perm / |det|) (A_1 + A_2 + A_3) / |det| + 4 u).
constexpr double kValueBound = 8.0e-15;    // > 2 * 30 * 2^-53

RF_STAR_FN bool finite(double x) { return fabs(x) < (double)INFINITY; }

struct alignas(16) Row32 {
    uint32_t v[4];
};
struct alignas(16) Row64 {
    int64_t v[2];
};

// row t of a table of 4-byte words (uint32, or int32: a negative word reads as 2^31 or more) or of int64, whole: the
// table is 16-byte aligned, so this is one 16-byte load (two for int64)
RF_STAR_FN void load_row(const uint32_t *table, uint32_t t, int64_t *row) {
    const Row32 r = *reinterpret_cast<const Row32 *>(table + 4 * (size_t)t);
    row[0] = (int64_t)r.v[0], row[1] = (int64_t)r.v[1], row[2] = (int64_t)r.v[2], row[3] = (int64_t)r.v[3];
}

RF_STAR_FN void load_row(const int64_t *table, uint32_t t, int64_t *row) {
    const Row64 lo = *reinterpret_cast<const Row64 *>(table + 4 * (size_t)t),
                hi = *reinterpret_cast<const Row64 *>(table + 4 * (size_t)t + 2);
    row[0] = lo.v[0], row[1] = lo.v[1], row[2] = hi.v[0], row[3] = hi.v[1];
}

// an adjacency entry as read: the hull word of either width becomes kHull, everything else stays itself
RF_STAR_FN int64_t adjacency_entry(const uint32_t *, int64_t e) { return e; }
RF_STAR_FN int64_t adjacency_entry(const int64_t *, int64_t e) { return e == -1 ? (int64_t)kHull : e; }

RF_STAR_FN bool sites_in_range(const int64_t *s, uint32_t n) {
    return s[0] >= 0 && s[0] < (int64_t)n && s[1] >= 0 && s[1] < (int64_t)n && s[2] >= 0 && s[2] < (int64_t)n &&
           s[3] >= 0 && s[3] < (int64_t)n;
}

RF_STAR_FN void load_point(const float *pts, int64_t s, float *p) {
    p[0] = pts[3 * (size_t)s], p[1] = pts[3 * (size_t)s + 1], p[2] = pts[3 * (size_t)s + 2];
}

RF_STAR_FN int face_orient(const float *q, const float *a, const float *b, const float *c) {
    RF_LOCATE_TRACE_FACE(q, a, b, c);
    return star::orient_sign(q, a, b, c);
}

// the lowest j with sigma_j < 0; 4 when there is none (the closed tetrahedron holds q), 5 when all four are zero
RF_STAR_FN uint32_t exit_face(const float *p0, const float *p1, const float *p2, const float *p3, const float *q) {
    int s;
    bool positive = false;
    if ((s = face_orient(q, p1, p2, p3)) < 0) return 0u;
    positive |= s > 0;
    if ((s = face_orient(q, p0, p3, p2)) < 0) return 1u;
    positive |= s > 0;
    if ((s = face_orient(q, p0, p1, p3)) < 0) return 2u;
    positive |= s > 0;
    if ((s = face_orient(q, p1, p0, p2)) < 0) return 3u;
    positive |= s > 0;
    return positive ? 4u : 5u;
}

// The walk of one query: (tetrahedron, -1 or a fault code; faces crossed).  start < 0 or >= T is a fault.
template <typename I>
RF_STAR_FN void walk(const float *pts, uint32_t n, const I *tets, const I *adjacency, uint32_t num_tets, const float *q,
                     int64_t start, uint32_t max_hops, int64_t &tet, int32_t &hops_out) {
    hops_out = 0;
    if (!(finite((double)q[0]) && finite((double)q[1]) && finite((double)q[2]))) {
        tet = kOutside;
        return;
    }
    if (start < 0 || start >= (int64_t)num_tets) {
        tet = fault_code(kBadStart, 0);
        return;
    }
    uint32_t t = (uint32_t)start, hops = 0;
    RF_STAR_NOUNROLL
    for (;;) {
        int64_t s[4], e[4];
        load_row(tets, t, s);
        if (!sites_in_range(s, n)) {
            tet = fault_code(kBadRow, t);
            break;
        }
        float p0[3], p1[3], p2[3], p3[3];
        load_point(pts, s[0], p0), load_point(pts, s[1], p1), load_point(pts, s[2], p2), load_point(pts, s[3], p3);
        const uint32_t j = exit_face(p0, p1, p2, p3, q);
        if (j >= 4u) {
            tet = j == 4u ? (int64_t)t : fault_code(kFlatRow, t);
            break;
        }
        load_row(adjacency, t, e);
        const int64_t entry = adjacency_entry(adjacency, j == 0u ? e[0] : j == 1u ? e[1] : j == 2u ? e[2] : e[3]);
        if (entry == (int64_t)kHull) {
            tet = kOutside;
            break;
        }
        if (entry < 0 || entry >= 4 * (int64_t)num_tets) {
            tet = fault_code(kBadAdjacency, t);
            break;
        }
        if (hops >= max_hops) {
            tet = fault_code(kHopCap, t);
            break;
        }
        t = (uint32_t)(entry >> 2);
        ++hops;
    }
    hops_out = (int32_t)hops;
}

// ---- interpolation ------------------------------------------------------------------------------------------------------

struct Frame {
    double x[3], n1[3], n2[3], n3[3], det, w[4];
};

RF_STAR_FN void cross(const double *a, const double *b, double *r) {
    r[0] = a[1] * b[2] - a[2] * b[1], r[1] = a[2] * b[0] - a[0] * b[2], r[2] = a[0] * b[1] - a[1] * b[0];
}

RF_STAR_FN double dot(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// the frame of a query in the tetrahedron of the sites s (in range); false where det == 0 or a weight is not finite
RF_STAR_FN bool frame_of(const float *pts, const int64_t *s, const float *q, Frame &f) {
    float p0[3], p1[3], p2[3], p3[3];
    load_point(pts, s[0], p0), load_point(pts, s[1], p1), load_point(pts, s[2], p2), load_point(pts, s[3], p3);
    double d1[3], d2[3], d3[3];
    for (int k = 0; k < 3; ++k) {
        d1[k] = (double)p1[k] - (double)p0[k], d2[k] = (double)p2[k] - (double)p0[k];
        d3[k] = (double)p3[k] - (double)p0[k], f.x[k] = (double)q[k] - (double)p0[k];
    }
    cross(d2, d3, f.n1), cross(d3, d1, f.n2), cross(d1, d2, f.n3);
    f.det = dot(d1, f.n1);
    if (f.det == 0.0) return false;
    f.w[1] = dot(f.n1, f.x) / f.det, f.w[2] = dot(f.n2, f.x) / f.det, f.w[3] = dot(f.n3, f.x) / f.det;
    f.w[0] = 1.0 - ((f.w[1] + f.w[2]) + f.w[3]);
    return finite(f.w[0]) && finite(f.w[1]) && finite(f.w[2]) && finite(f.w[3]);
}

// g and value of channel c; false where one of them is not finite
template <typename V>
RF_STAR_FN bool channel_of(const Frame &f, const V *values, uint32_t channels, const int64_t *s, uint32_t c, double *g,
                           double &value) {
    const double v0 = (double)values[(size_t)s[0] * channels + c];
    const double e1 = (double)values[(size_t)s[1] * channels + c] - v0, e2 = (double)values[(size_t)s[2] * channels + c] - v0,
                 e3 = (double)values[(size_t)s[3] * channels + c] - v0;
    for (int k = 0; k < 3; ++k) g[k] = ((e1 * f.n1[k] + e2 * f.n2[k]) + e3 * f.n3[k]) / f.det;
    value = v0 + dot(g, f.x);
    return finite(g[0]) && finite(g[1]) && finite(g[2]) && finite(value);
}

// the sites of the tetrahedron a query was located in; false for tet outside [0,T) or a corner outside [0,N)
template <typename I>
RF_STAR_FN bool located_sites(const I *tets, uint32_t num_tets, uint32_t n, int64_t tet, int64_t *s) {
    if (tet < 0 || tet >= (int64_t)num_tets) return false;
    load_row(tets, (uint32_t)tet, s);
    return sites_in_range(s, n);
}

// value[C], weights[4], gradient[C][3] of one query
template <typename V>
RF_STAR_FN void interpolate(const float *pts, const int64_t *s, bool sites_ok, const V *values, uint32_t channels,
                            const float *q, double *value, double *weights, double *gradient) {
    Frame f;
    bool ok = sites_ok && frame_of(pts, s, q, f);
    if (ok) {
        RF_STAR_NOUNROLL
        for (uint32_t c = 0; c < channels; ++c) {
            double g[3], v;
            ok &= channel_of(f, values, channels, s, c, g, v);
            value[c] = v, gradient[3 * c] = g[0], gradient[3 * c + 1] = g[1], gradient[3 * c + 2] = g[2];
        }
        weights[0] = f.w[0], weights[1] = f.w[1], weights[2] = f.w[2], weights[3] = f.w[3];
    }
    if (!ok) {
        const double nan = (double)NAN;
        RF_STAR_NOUNROLL
        for (uint32_t c = 0; c < channels; ++c) value[c] = gradient[3 * c] = gradient[3 * c + 1] = gradient[3 * c + 2] = nan;
        weights[0] = weights[1] = weights[2] = weights[3] = nan;
    }
}

// parts[4][3 + C] and grad_q[3] of one query for the upstream grad_value[C]
template <typename V>
RF_STAR_FN void interpolate_grad(const float *pts, const int64_t *s, bool sites_ok, const V *values, uint32_t channels,
                                 const float *q, const double *grad_value, double *parts, double *grad_q) {
    const uint32_t width = 3u + channels;
    Frame f;
    bool ok = sites_ok && frame_of(pts, s, q, f);
    if (ok) {
        double h[3] = {0.0, 0.0, 0.0};
        RF_STAR_NOUNROLL
        for (uint32_t c = 0; c < channels; ++c) {
            double g[3], v;
            ok &= channel_of(f, values, channels, s, c, g, v);
            const double up = grad_value[c];
            h[0] = h[0] + up * g[0], h[1] = h[1] + up * g[1], h[2] = h[2] + up * g[2];
            for (uint32_t i = 0; i < 4u; ++i) {
                const double part = up * f.w[i];
                parts[i * width + 3u + c] = part;
                ok &= finite(part);
            }
        }
        for (uint32_t i = 0; i < 4u; ++i)
            for (uint32_t k = 0; k < 3u; ++k) {
                const double part = -(f.w[i] * h[k]);
                parts[i * width + k] = part;
                ok &= finite(part);
            }
        grad_q[0] = h[0], grad_q[1] = h[1], grad_q[2] = h[2];
    }
    if (!ok) {
        RF_STAR_NOUNROLL
        for (uint32_t e = 0; e < 4u * width; ++e) parts[e] = 0.0;
        grad_q[0] = grad_q[1] = grad_q[2] = 0.0;
    }
}

// what one site adds up: its run of the sorted incidences, each a row of `width` doubles of parts, ascending
RF_STAR_FN void site_sum(const int64_t *incidence_order, const int64_t *site_runs, int64_t total, const double *parts,
                         uint32_t channels, uint32_t site, double *grad_points, double *grad_values) {
    const uint32_t width = 3u + channels;
    int64_t k = site_runs[site], end = site_runs[site + 1];
    if (k < 0) k = 0;
    if (end > total) end = total;
    double acc[3 + kMaxChannels];
    for (uint32_t e = 0; e < 3u + kMaxChannels; ++e) acc[e] = 0.0;
    RF_STAR_NOUNROLL
    for (; k < end; ++k) {
        const int64_t at = incidence_order[k];
        if (at < 0 || at >= total) continue;
        const double *part = parts + (size_t)at * width;
        for (uint32_t e = 0; e < 3u + kMaxChannels; ++e)
            if (e < width) acc[e] += part[e];
    }
    grad_points[3 * (size_t)site] = acc[0], grad_points[3 * (size_t)site + 1] = acc[1], grad_points[3 * (size_t)site + 2] = acc[2];
    for (uint32_t c = 0; c < kMaxChannels; ++c)
        if (c < channels) grad_values[(size_t)site * channels + c] = acc[3 + c];
}

}  // namespace locate
}  // namespace rf
