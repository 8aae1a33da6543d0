// rf_segments_grad.hip -- the backward operator of the exported walk: dL/dt_enter[S], dL/dt_exit[S] -> points_grad[N][3]
// (include/radfoam_hip_segments.h).
//
// Entry j of ray r leaves cell a = cells[j] through the face it shares with b = next(j): cells[j + 1] inside the ray's
// range, exit_cells[r] for the ray's last entry, none when t_exit[j] is infinite (or exit_cells[r] is kNone).  The
// derivative of that crossing is the reference's cell_intersection_grad on the fp32 points (the formula of
// rf_math.hpp::bisector_grad, evaluated in double here: seg_bisector_grad; the fp16 face table the walk used is not
// differentiated), as in trace_backward.  t_enter[m] is the running maximum of the
// earlier t_exit, so its gradient belongs to the entry that holds that maximum: j is a holder iff t_exit[j] > t_enter[j],
// decided from the stored floats, and
//     G_j = grad_t_exit[j] + [j holds] * sum of grad_t_enter[m], m = j + 1 .. the next holder of the ray (included)
//     points_grad[a] += G_j dt/dp_a,   points_grad[b] += G_j dt/dp_b          (skipped when G_j == 0 exactly)
//
// ONE LANE PER ENTRY, not per ray: every [S] array is read coalesced, and the lane of entry k owns cell cells[k].  Cell
// cells[k] is the `a` of face k and the `b` of face k - 1, so the lane forms G_k and G_{k-1} (each a forward look over
// the following entries up to the next holder: one step almost always), the two derivatives with respect to its own
// site, and issues one 3-float atomic update.  The lane of a ray's last entry also issues the `b` part of its face to
// exit_cells[r], which has no lane.  Nothing is kept in per-lane arrays.
//
// Compiled like the tracer (-ffp-contract=off; every fused multiply-add spelled out).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/radfoam_hip_segments.h"
#include "rf_host.hpp"
#include "rf_math.hpp"
#include "rf_segments_face.hpp"

namespace rf {

constexpr int kSegGradBlock = 256;

struct SegGradParams {
    uint32_t num_points, num_rays;
    int64_t total;               // S
    const float *points;         // [N][3]
    const float *rays;           // [R][6]
    const int64_t *offsets;      // [R + 1]
    const int32_t *entry_ray;    // [S]
    const uint32_t *cells;       // [S]
    const float *t_enter, *t_exit;
    const uint32_t *exit_cells;  // [R]
    const float *g_enter, *g_exit;
    float *points_grad;          // [N][3], accumulated into
};

// gradient accumulation: hardware fp32 atomic add without return, as rf_kernels.hip issues it
__device__ __forceinline__ void seg_grad_add(float *dst, float v) { unsafeAtomicAdd(dst, v); }

// rf_math.hpp::bisector_grad -- d(t)/d(p) of the ray's crossing of the bisector of (p, q), the reference's
// cell_intersection_grad on the fp32 points -- with the fp32 values widened and every operation in double.  The
// formula divides by dp^2, dp = (q - p) . d, and on a face the ray nearly grazes dp is what is left of a cancellation:
// evaluated in fp32 it keeps a few digits, and since such faces have the largest derivatives by orders of magnitude
// they carry the rows they touch.  Measured on 3000 incoherent rays with random upstream gradients (|dt/dp| up to
// 5.8e9): the fp32 evaluation put the worst element of points_grad at 1.9 times the project's 1e-3 gradient bar
// against a float64 evaluation of the same definition.  No guard is added: dp = 0 still gives non-finite values.
__device__ __forceinline__ void seg_bisector_grad(double px, double py, double pz, double qx, double qy, double qz,
                                                  double ox, double oy, double oz, double dx, double dy, double dz,
                                                  double &gx, double &gy, double &gz) {
    const double fnx = qx - px, fny = qy - py, fnz = qz - pz;
    const double vx = (px + qx) / 2.0 - ox;
    const double vy = (py + qy) / 2.0 - oy;
    const double vz = (pz + qz) / 2.0 - oz;
    const double num = seg_dot3(vx, vy, vz, fnx, fny, fnz);
    const double dp = seg_dot3(fnx, fny, fnz, dx, dy, dz);
    const double den = dp * dp;
    gx = __builtin_fma(num, dx, dp * (ox - px)) / den;
    gy = __builtin_fma(num, dy, dp * (oy - py)) / den;
    gz = __builtin_fma(num, dz, dp * (oz - pz)) / den;
}

__global__ __launch_bounds__(kSegGradBlock) void segments_points_grad_kernel(SegGradParams p) {
    const int64_t k = (int64_t)blockIdx.x * kSegGradBlock + threadIdx.x;
    if (k >= p.total) return;
    const uint32_t ray = (uint32_t)p.entry_ray[k];
    if (ray >= p.num_rays) return;
    const int64_t lo = p.offsets[ray], hi = p.offsets[ray + 1];
    if (k < lo || k >= hi) return;                       // entry_ray does not match the offsets: not this ray's entry
    const uint32_t a = p.cells[k];
    if (a >= p.num_points) return;

    const bool first = k == lo, last = k + 1 == hi;
    const uint32_t b = last ? p.exit_cells[ray] : p.cells[k + 1];
    const uint32_t prev = first ? kNone : p.cells[k - 1];
    float Gk = b < p.num_points ? seg_face_total(p, k, hi) : 0.0f;
    float Gp = prev < p.num_points ? seg_face_total(p, k - 1, hi) : 0.0f;
    if (Gk == 0.0f && Gp == 0.0f) return;

    // everything below is double arithmetic on the fp32 inputs (see seg_bisector_grad)
    const float *rp = p.rays + (size_t)ray * 6;
    const double Ox = rp[0], Oy = rp[1], Oz = rp[2];
    double dx = rp[3], dy = rp[4], dz = rp[5];
    const double nrm = __builtin_sqrt(seg_dot3(dx, dy, dz, dx, dy, dz));
    dx = dx / nrm;
    dy = dy / nrm;
    dz = dz / nrm;

    const float *pa = p.points + (size_t)a * 3;
    const double ax = pa[0], ay = pa[1], az = pa[2];
    double sx = 0.0, sy = 0.0, sz = 0.0;                 // the update of cell a
    if (Gk != 0.0f) {
        const float *pb = p.points + (size_t)b * 3;
        const double bx = pb[0], by = pb[1], bz = pb[2];
        const double G = Gk;
        double gx, gy, gz;
        seg_bisector_grad(ax, ay, az, bx, by, bz, Ox, Oy, Oz, dx, dy, dz, gx, gy, gz);
        sx = G * gx;
        sy = G * gy;
        sz = G * gz;
        if (last) {                                      // the far side of a ray's last face has no lane of its own
            seg_bisector_grad(bx, by, bz, ax, ay, az, Ox, Oy, Oz, dx, dy, dz, gx, gy, gz);
            float *dst = p.points_grad + (size_t)b * 3;
            seg_grad_add(dst + 0, (float)(G * gx));
            seg_grad_add(dst + 1, (float)(G * gy));
            seg_grad_add(dst + 2, (float)(G * gz));
        }
    }
    if (Gp != 0.0f) {
        const float *pq = p.points + (size_t)prev * 3;
        const double G = Gp;
        double gx, gy, gz;
        seg_bisector_grad(ax, ay, az, pq[0], pq[1], pq[2], Ox, Oy, Oz, dx, dy, dz, gx, gy, gz);
        sx = __builtin_fma(G, gx, sx);
        sy = __builtin_fma(G, gy, sy);
        sz = __builtin_fma(G, gz, sz);
    }
    float *dst = p.points_grad + (size_t)a * 3;
    seg_grad_add(dst + 0, (float)sx);
    seg_grad_add(dst + 1, (float)sy);
    seg_grad_add(dst + 2, (float)sz);
}

}  // namespace rf

using namespace rf;

extern "C" {

int rf_segments_points_grad(uint32_t num_points, const float *points, uint32_t num_rays, const float *rays,
                            const int64_t *offsets, int64_t num_entries, const int32_t *entry_ray,
                            const uint32_t *cells, const float *t_enter, const float *t_exit,
                            const uint32_t *exit_cells, const float *grad_t_enter, const float *grad_t_exit,
                            float *points_grad, void *stream) {
    const char *what = "rf_segments_points_grad";
    g_err[0] = 0;
    if (num_entries < 0) return fail(RF_ERR_INVALID_ARGUMENT, "%s: negative entry count", what);
    if (num_entries == 0 || num_rays == 0 || num_points == 0) return RF_OK;
    if (!points || !rays || !offsets || !entry_ray || !cells || !t_enter || !t_exit || !exit_cells || !grad_t_enter ||
        !grad_t_exit || !points_grad)
        return fail(RF_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    const int64_t blocks = (num_entries + kSegGradBlock - 1) / kSegGradBlock;
    if (blocks > 0x7FFFFFFFll) return fail(RF_ERR_INVALID_ARGUMENT, "%s: too many entries for one launch", what);
    SegGradParams p{};
    p.num_points = num_points;
    p.num_rays = num_rays;
    p.total = num_entries;
    p.points = points;
    p.rays = rays;
    p.offsets = offsets;
    p.entry_ray = entry_ray;
    p.cells = cells;
    p.t_enter = t_enter;
    p.t_exit = t_exit;
    p.exit_cells = exit_cells;
    p.g_enter = grad_t_enter;
    p.g_exit = grad_t_exit;
    p.points_grad = points_grad;
    hipLaunchKernelGGL(segments_points_grad_kernel, dim3((uint32_t)blocks), dim3(kSegGradBlock), 0,
                       static_cast<hipStream_t>(stream), p);
    return check_launch(what);
}

}  // extern "C"
