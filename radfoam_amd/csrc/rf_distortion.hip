// rf_distortion.hip -- the distortion regulariser over an exported walk, and its gradients
// (include/radfoam_hip_distortion.h).
//
// Per ray r over its entries i, in order (the weights are rf_composite.hip's):
//     dt_i = 0 where t_exit[i] is infinite, else max(t_exit[i] - t_enter[i], 0),      x_i = sigma[i] dt_i
//     T_i = exp(-(sum of x_k, k < i)),      w_i = T_i (1 - exp(-x_i))
//     a_i, b_i = s_enter[i], s_exit[i] where given, else t_enter[i], t_exit[i]
//     m_i = (a_i + b_i) / 2,   d_i = max(b_i - a_i, 0);   both 0, selected, where t_exit[i] is infinite
//     out[r] = 2 sum_i w_i (m_i W<_i - M<_i) + (1/3) sum_i w_i^2 d_i,      W<_i = sum_{k<i} w_k, M<_i = sum_{k<i} w_k m_k
//
// The wave scheme -- one wave owns kDistRays consecutive rays and sweeps their entries 64 at a time, segmented scans in
// double, no atomics, no LDS, no lane returning before the wave's last cross-lane operation -- is rf_ray_sweep.hpp's.
//
// A sweep scans three times per step: x (for T and w), then w and w m together (W< and M< are the inclusive sums less
// the lane's own term), then the entry's share of out[r].  The sums over a ray's LATER entries, which only the
// gradients need, are the ray's totals less the inclusive sums, so the backward SWEEPS ITS RANGE TWICE: the first sweep,
// which is the forward's, leaves sum w, sum w m and out of ray r0 + i in lane i; the second forms the gradients.  out is
// homogeneous of degree 2 in w, so sum_k w_k (d out / d w_k) = 2 out[r], and the suffix sum in dL/dx is 2 out[r] less an
// inclusive prefix: no third sweep.  The forward stores from those lanes: lane i rounds ONCE to fp32 and writes out[r0 + i]
// (0 for a ray without entries).  Nothing is reconstructed from the fp32 output of the forward.
//
// Compiled like the tracer (-ffp-contract=off); exp and expm1 are the double ones.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/radfoam_hip_distortion.h"
#include "rf_host.hpp"
#include "rf_ray_sweep.hpp"

#ifndef RF_DISTORTION_RAYS_PER_WAVE
#define RF_DISTORTION_RAYS_PER_WAVE 8
#endif

namespace rf {

constexpr int kDistBlock = 256;
constexpr int kDistWaves = kDistBlock / 64;
constexpr int kDistRays = RF_DISTORTION_RAYS_PER_WAVE;     // rays per wave: 8 and 16 measured equal, 2, 4, 32 slower
using DistSweep = RaySweep<kDistRays, kDistWaves>;
using DistWave = DistSweep::Wave;
using DistStep = DistSweep::Step;

// ---- what an entry brings: zeros where the lane is not valid.  dt, sigma, x, infinite and moves are SweepEntry's,
// taken over from it in the one branch that also reads the interval; the members stand in this order because another
// one, a struct derived from SweepEntry too, changes the kernels' code ----
struct DistEntry {
    double dt, sigma, x;
    double m, d;       // midpoint and width in the measure of the distortion; 0, selected, where t_exit is infinite
    bool infinite, moves;
    bool widens;       // not infinite and b >= a: d passes its gradient on (the convention of moves)
};

__device__ __forceinline__ DistEntry dist_entry(const DistStep &s, const float *t_enter, const float *t_exit,
                                                const float *sigma, const float *s_enter, const float *s_exit) {
    DistEntry e{0.0, 0.0, 0.0, 0.0, 0.0, false, false, false};
    if (s.valid) {
        const SweepEntry in = sweep_entry_at(s.k, t_enter, t_exit, sigma);
        e.infinite = in.infinite;
        e.moves = in.moves;
        e.dt = in.dt;
        e.sigma = in.sigma;
        e.x = in.x;
        const float a = s_enter ? s_enter[s.k] : in.t0, b = s_exit ? s_exit[s.k] : in.t1;
        const double width = (double)b - (double)a;
        e.widens = !e.infinite && b >= a;
        e.m = e.infinite ? 0.0 : ((double)a + (double)b) * 0.5;
        e.d = e.infinite ? 0.0 : (width < 0.0 ? 0.0 : width);
    }
    return e;
}

// ---- the weights of a step and their running sums ----
struct DistCarry {
    double x, w, wm;   // of the ray that runs past the step before: sum x, sum w, sum w m so far
};

struct DistWeights {
    double through;    // T_i
    double alpha;      // 1 - exp(-x_i)
    double w;          // T_i alpha_i
    double before_w, before_wm;      // W<_i, M<_i
    double upto_w, upto_wm;          // the same with the entry's own term: the ray's sums up to and including i
};

__device__ __forceinline__ DistWeights dist_weights(const DistWave &wv, const DistStep &s, const DistEntry &e,
                                                    DistCarry &carry) {
    DistWeights o;
    const double sum_x = DistSweep::running(wv, s, e.x, carry.x);
    const SweepWeight t = sweep_weight(sum_x, e.x);
    o.through = t.through;
    o.alpha = t.alpha;
    o.w = t.weight;
    const double wm = o.w * e.m;
    double v[2] = {o.w, wm};
    DistSweep::scan(v, wv.lane, s.begin);
    o.upto_w = s.cont ? v[0] + carry.w : v[0];
    o.upto_wm = s.cont ? v[1] + carry.wm : v[1];
    o.before_w = o.upto_w - o.w;
    o.before_wm = o.upto_wm - wm;
    carry.x = DistSweep::carry(s, sum_x);
    carry.w = DistSweep::carry(s, o.upto_w);
    carry.wm = DistSweep::carry(s, o.upto_wm);
    return o;
}

struct DistParams {
    uint32_t num_rays;
    int64_t total;               // S
    const int64_t *offsets;      // [R + 1]
    const float *t_enter, *t_exit, *sigma;   // [S]
    const float *s_enter, *s_exit;           // [S], or both null: the distortion is measured in t
    float *out;                  // forward: [R]
    const float *grad_out;       // backward: [R]
    float *grad_sigma, *grad_t_enter, *grad_t_exit, *grad_s_enter, *grad_s_exit;   // backward: each may be null
};

// ---- the sweep both kernels begin with: lane i gets sum w, sum w m and out of ray r0 + i (zeros for a ray without
// entries and for the lanes from nrays on), from the lane of the ray's last entry ----
__device__ __forceinline__ void dist_totals(const DistWave &w, const DistParams &p, double &ray_w, double &ray_wm,
                                            double &ray_out) {
    ray_w = ray_wm = ray_out = 0.0;
    const int64_t next = DistSweep::from_lane(w.off, (w.lane + 1) & 63);
    const bool mine = w.lane < w.nrays && next > w.off;
    const int64_t my_last = next - 1;
    DistCarry carry{0.0, 0.0, 0.0};
    double carry_out = 0.0;
    for (int64_t base = w.first_base(); base < w.hi; base += 64) {
        const DistStep s = DistSweep::step(w, base);
        const DistEntry e = dist_entry(s, p.t_enter, p.t_exit, p.sigma, p.s_enter, p.s_exit);
        const DistWeights q = dist_weights(w, s, e, carry);
        // the entry's share: 2 w (m W< - M<) + w^2 d / 3
        const double share = 2.0 * q.w * (e.m * q.before_w - q.before_wm) + q.w * q.w * e.d / 3.0;
        const double sum_out = DistSweep::running(w, s, share, carry_out);
        carry_out = DistSweep::carry(s, sum_out);

        // the ray's totals to lane i: spelled out as in rf_composite.hip's first sweep, keep in step
        const bool here = mine && my_last >= base && my_last < base + 64;
        const int src = here ? (int)(my_last - base) : w.lane;
        const double end_w =DistSweep::from_lane(q.upto_w, src), end_wm = DistSweep::from_lane(q.upto_wm, src);
        const double end_out = DistSweep::from_lane(sum_out, src);
        if (here) {
            ray_w = end_w;
            ray_wm = end_wm;
            ray_out = end_out;
        }
    }
}

__global__ __launch_bounds__(kDistBlock) void ray_distortion_forward_kernel(DistParams p) {
    DistWave w;
    if (!w.init(p.num_rays, p.total, p.offsets)) return;
    double ray_w, ray_wm, ray_out;
    dist_totals(w, p, ray_w, ray_wm, ray_out);
    if (w.lane < w.nrays) p.out[w.r0 + w.lane] = (float)ray_out;         // the ray's sum is complete: round once
}

__global__ __launch_bounds__(kDistBlock) void ray_distortion_backward_kernel(DistParams p) {
    DistWave w;
    if (!w.init(p.num_rays, p.total, p.offsets)) return;
    const bool need_x = p.grad_sigma != nullptr || p.grad_t_enter != nullptr || p.grad_t_exit != nullptr;
    const bool own_measure = p.s_enter != nullptr;                       // the times get the part through w alone

    // ---- first sweep: the totals ----
    double ray_w, ray_wm, ray_out;
    dist_totals(w, p, ray_w, ray_wm, ray_out);

    // ---- second sweep: the gradients ----
    DistCarry carry{0.0, 0.0, 0.0};
    double carry_wg = 0.0;
    for (int64_t base = w.first_base(); base < w.hi; base += 64) {
        const DistStep s = DistSweep::step(w, base);
        const DistEntry e = dist_entry(s, p.t_enter, p.t_exit, p.sigma, p.s_enter, p.s_exit);
        const DistWeights q = dist_weights(w, s, e, carry);
        const double total_w = DistSweep::from_lane(ray_w, s.ray), total_wm = DistSweep::from_lane(ray_wm, s.ray);
        const double total_out = DistSweep::from_lane(ray_out, s.ray);
        const double after_w = total_w - q.upto_w, after_wm = total_wm - q.upto_wm;      // W>_i, M>_i
        const double g_ray = s.valid ? (double)p.grad_out[w.r0 + s.ray] : 0.0;

        // through m and d
        const double half_dm = q.w * (q.before_w - after_w);                               // 1/2 d out / d m_i
        const double dd = e.widens ? q.w * q.w / 3.0 : 0.0;                                // [b >= a] d out / d d_i
        const double g_b = e.infinite ? 0.0 : g_ray * (half_dm + dd);
        const double g_a = e.infinite ? 0.0 : g_ray * (half_dm - dd);
        if (s.valid && own_measure) {
            if (p.grad_s_enter) p.grad_s_enter[s.k] = (float)g_a;
            if (p.grad_s_exit) p.grad_s_exit[s.k] = (float)g_b;
        }
        if (!need_x) continue;                                                              // wave-uniform

        // through w: d out / d w_i, its inclusive prefix sum with w, and the suffix as 2 out[r] less that
        const double g_w = 2.0 * (e.m * q.before_w - q.before_wm) + 2.0 * (after_wm - e.m * after_w)
                           + 2.0 * q.w * e.d / 3.0;
        double swg[1] = {q.w * g_w};
        DistSweep::scan(swg, w.lane, s.begin);
        const double sum_wg = s.cont ? swg[0] + carry_wg : swg[0];
        carry_wg = DistSweep::carry(s, sum_wg);
        if (s.valid) {
            // T_i exp(-x_i) g_i - (the ray's later w g); exp(-x_i) = 1 - alpha_i
            const double dx = g_ray * (q.through * (1.0 - q.alpha) * g_w - (2.0 * total_out - sum_wg));
            const SweepGrad g = sweep_grad(e, dx);
            if (p.grad_sigma) p.grad_sigma[s.k] = (float)g.sigma;
            if (p.grad_t_exit) p.grad_t_exit[s.k] = (float)(own_measure ? g.exit : g.exit + g_b);
            if (p.grad_t_enter) p.grad_t_enter[s.k] = (float)(own_measure ? 0.0 - g.exit : g_a - g.exit);
        }
    }
}

}  // namespace rf

using namespace rf;

extern "C" {

uint32_t rf_distortion_rays_per_wave(void) { return (uint32_t)kDistRays; }

int rf_ray_distortion_forward(uint32_t num_rays, const int64_t *offsets, int64_t num_entries, const float *t_enter,
                              const float *t_exit, const float *sigma, const float *s_enter, const float *s_exit,
                              float *out, void *stream) {
    const char *what = "rf_ray_distortion_forward";
    g_err[0] = 0;
    if (num_entries < 0) return fail(RF_ERR_INVALID_ARGUMENT, "%s: negative entry count", what);
    if ((s_enter == nullptr) != (s_exit == nullptr))
        return fail(RF_ERR_INVALID_ARGUMENT, "%s: s_enter and s_exit are both given or both null", what);
    if (num_rays == 0) return RF_OK;
    if (!out) return fail(RF_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (num_entries == 0) {
        if (hipMemsetAsync(out, 0, (size_t)num_rays * sizeof(float), s) != hipSuccess) return check_launch(what);
        return RF_OK;
    }
    if (!offsets || !t_enter || !t_exit || !sigma) return fail(RF_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    DistParams p{};
    p.num_rays = num_rays;
    p.total = num_entries;
    p.offsets = offsets;
    p.t_enter = t_enter;
    p.t_exit = t_exit;
    p.sigma = sigma;
    p.s_enter = s_enter;
    p.s_exit = s_exit;
    p.out = out;
    hipLaunchKernelGGL(ray_distortion_forward_kernel, dim3((uint32_t)DistSweep::blocks(num_rays)), dim3(kDistBlock), 0,
                       s, p);
    return check_launch(what);
}

int rf_ray_distortion_backward(uint32_t num_rays, const int64_t *offsets, int64_t num_entries, const float *t_enter,
                               const float *t_exit, const float *sigma, const float *s_enter, const float *s_exit,
                               const float *grad_out, float *grad_sigma, float *grad_t_enter, float *grad_t_exit,
                               float *grad_s_enter, float *grad_s_exit, void *stream) {
    const char *what = "rf_ray_distortion_backward";
    g_err[0] = 0;
    if (num_entries < 0) return fail(RF_ERR_INVALID_ARGUMENT, "%s: negative entry count", what);
    if ((s_enter == nullptr) != (s_exit == nullptr))
        return fail(RF_ERR_INVALID_ARGUMENT, "%s: s_enter and s_exit are both given or both null", what);
    if (!s_enter && (grad_s_enter || grad_s_exit))
        return fail(RF_ERR_INVALID_ARGUMENT, "%s: grad_s_enter / grad_s_exit without s_enter / s_exit", what);
    if (num_rays == 0 || num_entries == 0) return RF_OK;
    if (!grad_sigma && !grad_t_enter && !grad_t_exit && !grad_s_enter && !grad_s_exit) return RF_OK;
    if (!offsets || !t_enter || !t_exit || !sigma || !grad_out)
        return fail(RF_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    DistParams p{};
    p.num_rays = num_rays;
    p.total = num_entries;
    p.offsets = offsets;
    p.t_enter = t_enter;
    p.t_exit = t_exit;
    p.sigma = sigma;
    p.s_enter = s_enter;
    p.s_exit = s_exit;
    p.grad_out = grad_out;
    p.grad_sigma = grad_sigma;
    p.grad_t_enter = grad_t_enter;
    p.grad_t_exit = grad_t_exit;
    p.grad_s_enter = grad_s_enter;
    p.grad_s_exit = grad_s_exit;
    hipLaunchKernelGGL(ray_distortion_backward_kernel, dim3((uint32_t)DistSweep::blocks(num_rays)), dim3(kDistBlock), 0,
                       static_cast<hipStream_t>(stream), p);
    return check_launch(what);
}

}  // extern "C"
