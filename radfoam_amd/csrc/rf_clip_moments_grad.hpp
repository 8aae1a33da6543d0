// rf_clip_moments_grad.hpp -- the backward of the second moments of the Voronoi cells (rf_cell_moments_grad.hip) over the
// clipping core of rf_clip.hpp, in double: the gradient of  L = sum_a <G_a, Q_a> + <H_a, C_a>  with respect to the sites,
// Q_a = int (x - p_a)(x - p_a)^T dx the site moment and C_a = int (x - c_a)(x - c_a)^T dx the central moment of
// rf_clip_moments.hpp ("Point gradients of the second moments").
//
// Six upstream numbers g = (xx, yy, zz, xy, xz, yz) stand for the symmetric matrix S(g) with the diagonal as it is and
// HALF of each off-diagonal number on both sides, so that <S(g), Q> is the plain sum of g_k Q_k over the six stored
// numbers.  With G_a = S(grad_site_moment[a]), H_a = S(grad_central_moment[a]) and
//     Psi_a(x) = (x - p_a)^T G_a (x - p_a) + (x - c_a)^T H_a (x - c_a)     (Psi_a == 0 for an unbounded cell, whatever
//                                                                            arrives for it)
// L = sum_a int_a Psi_a dx, and the transport theorem of rf_clip_grad.hpp (face (a,b) moves outward from a with normal
// speed [(x - p_a) . delta_a - (x - p_b) . delta_b] / |d|) gives
//     grad p_a = sum_{b in N(a)} (1 / |d|) int_{F_ab} (Psi_a(x) - Psi_b(x)) (x - p_a) dA  -  2 V_a G_a m_a,
// m_a = c_a - p_a.  The last, direct term is the dependence of the integrand (x - p_a)(x - p_a)^T on p_a (for G = I the
// classical 2 V_a (p_a - c_a)); the central moment has none: d/dc int (x - c)^T H (x - c) dx = -2 H int (x - c) dx = 0 at
// the centroid, so the motion of c_a drops out to first order.
//
// In y = x - p_a a cell q of the row (a itself or a neighbour) is the quadratic
//     Psi_q(y) = y^T K_q y + l_q . y + k_q,   K_q = G_q + H_q,  l_q = -2 (G_q r_q + H_q e_q),
//     k_q = r_q^T G_q r_q + e_q^T H_q e_q,    r_q = p_q - p_a,  e_q = c_q - p_a
// (never from absolute coordinates), and with y = y0 + s' u + t' v (y0 vertex 0 of the polygon) the difference is
//     Psi_a - Psi_b = w + lu s' + lv t' + Kuu s'^2 + 2 Kuv s' t' + Kvv t'^2,
// w = y0^T K y0 + l . y0 + k, (lu, lv) = (2 K y0 + l) . (u, v), Kuu = u^T K u and so on, so that
//     int (Psi_a - Psi_b) y dA = y0 int f + u int f s' + v int f t'
// from the polygon's 2-D moments about vertex 0 up to THIRD order.
//
// An unbounded face contributes nothing and is skipped before any arithmetic; a bounded face of an unbounded row still
// carries the neighbour's term; a term of a site that lists a but is missing from a's row is dropped.
//
// __host__ __device__ and free of HIP types like rf_clip.hpp: tests/host_harness/clip_moments_grad_host.cpp compiles this
// file with g++ (no FMA contraction on either side).
#pragma once

#include "rf_clip.hpp"
#include "rf_clip_grad.hpp"
#include "rf_clip_moments.hpp"

namespace rf {
namespace clip {

// Moments plus the third-order sums about vertex 0: int s'^3, int s'^2 t', int s' t'^2, int t'^3
struct Moments3 {
    Moments m;
    double sss, sst, stt, ttt;
};

// One pass over the fan about vertex 0; the second-order sums are those of moments(), term for term.  Triangle (0, p, q)
// with cr = p x q and barycentric int l1^i l2^j dA = cr i! j! / (i + j + 2)! has
//   int s'^3    = cr (ps^3 + ps^2 qs + ps qs^2 + qs^3) / 20,
//   int s'^2 t' = cr (3 ps^2 pt + 3 qs^2 qt + ps^2 qt + qs^2 pt + 2 ps qs (pt + qt)) / 60,
// and the other two with s and t exchanged.
RF_CLIP_HD Moments3 moments3(const double *s, const double *t, uint32_t stride, uint32_t m, double R) {
    Moments3 o = {{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, false}, 0.0, 0.0, 0.0, 0.0};
    if (m == 0) return o;
    const double s0 = s[0], t0 = t[0];
    double a2 = 0.0, ms = 0.0, mt = 0.0, mss = 0.0, mst = 0.0, mtt = 0.0;
    double msss = 0.0, msst = 0.0, mstt = 0.0, mttt = 0.0;
    double ps = 0.0, pt = 0.0;   // previous vertex relative to vertex 0
    for (uint32_t i = 0; i < m; ++i) {
        const double si = s[i * stride], ti = t[i * stride];
        o.m.unbounded = o.m.unbounded || fmax(fabs(si), fabs(ti)) >= R;
        const double qs = si - s0, qt = ti - t0;
        if (i >= 2) {
            const double cr = ps * qt - pt * qs;
            const double pss = ps * ps, qss = qs * qs, psqs = ps * qs;
            const double ptt = pt * pt, qtt = qt * qt, ptqt = pt * qt;
            a2 += cr;
            ms += cr * (ps + qs);
            mt += cr * (pt + qt);
            mss += cr * ((pss + qss) + psqs);
            mtt += cr * ((ptt + qtt) + ptqt);
            mst += cr * (2.0 * (ps * pt + qs * qt) + (ps * qt + qs * pt));
            msss += cr * ((pss + qss) * (ps + qs));
            mttt += cr * ((ptt + qtt) * (pt + qt));
            msst += cr * ((3.0 * (pss * pt + qss * qt) + (pss * qt + qss * pt)) + 2.0 * (psqs * (pt + qt)));
            mstt += cr * ((3.0 * (ptt * ps + qtt * qs) + (ptt * qs + qtt * ps)) + 2.0 * (ptqt * (ps + qs)));
        }
        ps = qs, pt = qt;
    }
    o.m.a = 0.5 * a2, o.m.s = ms / 6.0, o.m.t = mt / 6.0;
    o.m.ss = mss / 12.0, o.m.tt = mtt / 12.0, o.m.st = mst / 24.0;
    o.m.s0 = s0, o.m.t0 = t0;
    o.sss = msss / 20.0, o.ttt = mttt / 20.0, o.sst = msst / 60.0, o.stt = mstt / 60.0;
    return o;
}

// a symmetric 3x3 matrix by its entries (xy is the entry itself, half the stored upstream number)
struct Sym3 {
    double xx, yy, zz, xy, xz, yz;
};

RF_CLIP_HD Sym3 sym_of_upstream(const double *g) {   // S(g); zero where the array is absent
    Sym3 m = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (g) m.xx = g[0], m.yy = g[1], m.zz = g[2], m.xy = 0.5 * g[3], m.xz = 0.5 * g[4], m.yz = 0.5 * g[5];
    return m;
}

RF_CLIP_HD void sym_apply(const Sym3 &m, double x, double y, double z, double &ox, double &oy, double &oz) {
    ox = (m.xx * x + m.xy * y) + m.xz * z;
    oy = (m.xy * x + m.yy * y) + m.yz * z;
    oz = (m.xz * x + m.yz * y) + m.zz * z;
}

RF_CLIP_HD double sym_form(const Sym3 &m, double ax, double ay, double az, double bx, double by, double bz) {   // a^T M b
    double x, y, z;
    sym_apply(m, bx, by, bz, x, y, z);
    return (ax * x + ay * y) + az * z;
}

// Psi_q in y = x - p_a: y^T K y + l . y + k; all zero for an unbounded cell (its upstream entries are never read)
struct MomentTerm {
    Sym3 K;
    double lx, ly, lz, k;
    bool bounded;
};

RF_CLIP_HD MomentTerm moment_term(const float *points, uint32_t a, uint32_t q, const double *centroid,
                                  const uint8_t *bounded, const double *grad_site_moment,
                                  const double *grad_central_moment) {
    MomentTerm c = {{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, 0.0, 0.0, 0.0, 0.0, false};
    if (!bounded[q]) return c;
    c.bounded = true;
    const Sym3 G = sym_of_upstream(grad_site_moment ? grad_site_moment + 6 * (size_t)q : nullptr);
    const Sym3 H = sym_of_upstream(grad_central_moment ? grad_central_moment + 6 * (size_t)q : nullptr);
    double rx, ry, rz, h;
    neighbour(points, a, q, rx, ry, rz, h);
    const double ex = centroid[3 * (size_t)q] - (double)points[3 * (size_t)a];
    const double ey = centroid[3 * (size_t)q + 1] - (double)points[3 * (size_t)a + 1];
    const double ez = centroid[3 * (size_t)q + 2] - (double)points[3 * (size_t)a + 2];
    double gx, gy, gz, hx, hy, hz;
    sym_apply(G, rx, ry, rz, gx, gy, gz);
    sym_apply(H, ex, ey, ez, hx, hy, hz);
    c.K.xx = G.xx + H.xx, c.K.yy = G.yy + H.yy, c.K.zz = G.zz + H.zz;
    c.K.xy = G.xy + H.xy, c.K.xz = G.xz + H.xz, c.K.yz = G.yz + H.yz;
    c.lx = -2.0 * (gx + hx), c.ly = -2.0 * (gy + hy), c.lz = -2.0 * (gz + hz);
    c.k = ((rx * gx + ry * gy) + rz * gz) + ((ex * hx + ey * hy) + ez * hz);
    return c;
}

// face (a,b)'s term of grad p_a: (1 / |d|) int (Psi_a - Psi_b)(p_a + y) y dA, added to (gx, gy, gz)
RF_CLIP_HD void add_face_moment_grad(const Frame &f, const Moments3 &m3, const MomentTerm &ca, const MomentTerm &cb,
                                     double &gx, double &gy, double &gz) {
    const Moments &mo = m3.m;
    if (mo.unbounded) return;
    const Sym3 K = {ca.K.xx - cb.K.xx, ca.K.yy - cb.K.yy, ca.K.zz - cb.K.zz,
                    ca.K.xy - cb.K.xy, ca.K.xz - cb.K.xz, ca.K.yz - cb.K.yz};
    const double lx = ca.lx - cb.lx, ly = ca.ly - cb.ly, lz = ca.lz - cb.lz, k0 = ca.k - cb.k;
    double x0, y0, z0, kx, ky, kz;
    to_space(f, mo.s0, mo.t0, x0, y0, z0);
    sym_apply(K, x0, y0, z0, kx, ky, kz);   // K y0
    const double w = (((kx * x0 + ky * y0) + kz * z0) + ((lx * x0 + ly * y0) + lz * z0)) + k0;
    const double px = 2.0 * kx + lx, py = 2.0 * ky + ly, pz = 2.0 * kz + lz;
    const double lu = (px * f.ux + py * f.uy) + pz * f.uz, lv = (px * f.vx + py * f.vy) + pz * f.vz;
    const double kuu = sym_form(K, f.ux, f.uy, f.uz, f.ux, f.uy, f.uz);
    const double kuv = 2.0 * sym_form(K, f.ux, f.uy, f.uz, f.vx, f.vy, f.vz);
    const double kvv = sym_form(K, f.vx, f.vy, f.vz, f.vx, f.vy, f.vz);
    const double f0 = ((w * mo.a + lu * mo.s) + lv * mo.t) + ((kuu * mo.ss + kuv * mo.st) + kvv * mo.tt);
    const double fu = ((w * mo.s + lu * mo.ss) + lv * mo.st) + ((kuu * m3.sss + kuv * m3.sst) + kvv * m3.stt);
    const double fv = ((w * mo.t + lu * mo.st) + lv * mo.tt) + ((kuu * m3.sst + kuv * m3.stt) + kvv * m3.ttt);
    gx += ((x0 * f0 + f.ux * fu) + f.vx * fv) / f.len;
    gy += ((y0 * f0 + f.uy * fu) + f.vy * fv) / f.len;
    gz += ((z0 * f0 + f.uz * fu) + f.vz * fv) / f.len;
}

// the direct term -2 V_a G_a m_a of a bounded cell, added to (gx, gy, gz); nothing for an unbounded one
RF_CLIP_HD void add_direct_moment_grad(const float *points, uint32_t a, const double *volume, const double *centroid,
                                       const uint8_t *bounded, const double *grad_site_moment, double &gx, double &gy,
                                       double &gz) {
    if (!bounded[a] || !grad_site_moment) return;
    const Sym3 G = sym_of_upstream(grad_site_moment + 6 * (size_t)a);
    const double mx = centroid[3 * (size_t)a] - (double)points[3 * (size_t)a];
    const double my = centroid[3 * (size_t)a + 1] - (double)points[3 * (size_t)a + 1];
    const double mz = centroid[3 * (size_t)a + 2] - (double)points[3 * (size_t)a + 2];
    double x, y, z;
    sym_apply(G, mx, my, mz, x, y, z);
    const double w = 2.0 * volume[a];
    gx -= w * x, gy -= w * y, gz -= w * z;
}

// One whole row of the gradient, face after face: the counterpart of cell_grad_serial (the host harness, and the kernel
// of last resort).  volume / centroid / bounded are what rf_cell_geometry wrote; either upstream may be null.  Writes
// grad_points[3 a ..] (zero for an empty row, NaN on a status other than kCellOk) and returns a kCell* status.
RF_CLIP_HD uint32_t cell_moments_grad_serial(const float *points, uint32_t num_points, const uint32_t *adj,
                                             const uint32_t *offsets, uint32_t num_edges, uint32_t a, double R, double *s,
                                             double *t, uint32_t cap, const double *volume, const double *centroid,
                                             const uint8_t *bounded, const double *grad_site_moment,
                                             const double *grad_central_moment, double *grad_points) {
    const uint32_t begin = offsets[a], end = offsets[a + 1];
    uint32_t status = row_is_valid(points, num_points, adj, num_edges, a, begin, end) ? kCellOk : kCellBadRow;
    double gx = 0.0, gy = 0.0, gz = 0.0;
    if (status == kCellOk && begin < end) {
        const MomentTerm ca = moment_term(points, a, a, centroid, bounded, grad_site_moment, grad_central_moment);
        for (uint32_t slot = begin; slot < end; ++slot) {
            Frame frame;
            uint32_t m, cur;
            if (!face_polygon(points, adj, a, begin, end, slot, R, s, t, 1u, cap, frame, m, cur)) {
                status = kCellTooManyVertices;
                break;
            }
            const Moments3 m3 = moments3(s + cur * cap, t + cur * cap, 1u, m, R);
            const MomentTerm cb = moment_term(points, a, adj[slot], centroid, bounded, grad_site_moment,
                                              grad_central_moment);
            add_face_moment_grad(frame, m3, ca, cb, gx, gy, gz);
        }
        add_direct_moment_grad(points, a, volume, centroid, bounded, grad_site_moment, gx, gy, gz);
    }
    if (status != kCellOk) gx = gy = gz = (double)NAN;
    grad_points[3 * (size_t)a] = gx, grad_points[3 * (size_t)a + 1] = gy, grad_points[3 * (size_t)a + 2] = gz;
    return status;
}

}  // namespace clip
}  // namespace rf
