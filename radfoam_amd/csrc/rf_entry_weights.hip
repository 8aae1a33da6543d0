// rf_entry_weights.hip -- the compositing weight and the transmittance of every entry of an exported walk, and their
// gradients (include/radfoam_hip_entry_weights.h).
//
// Per ray r over its entries e, in order (the definitions of rf_composite.hip, word for word):
//     dt_e = 0 where t_exit[e] is infinite, else max(t_exit[e] - t_enter[e], 0),      x_e = sigma[e] dt_e
//     T_e = exp(-(sum of x_k over the ray's earlier entries)),      w_e = T_e (1 - exp(-x_e))
// rf_composite.hip forms w_e and T_e in registers and sums them away; here they are the output, one element per entry.
//
// The wave scheme -- one wave owns kWeightRays consecutive rays and sweeps their entries 64 at a time, one lane per
// entry, a segmented scan in double, no atomics, no LDS, no lane returning before the wave's last cross-lane
// operation -- is rf_ray_sweep.hpp's.  Forward: one sweep, one scan (x).  Backward: one launch; with
// u_e = g_w[e] w_e + g_T[e] T_e the gradient to x_e needs the sum of u over the ray's LATER entries, which is the
// ray's total minus an inclusive prefix, so the wave SWEEPS ITS RANGE TWICE: the first sweep leaves the total of ray
// r0 + i in lane i, the second forms the gradients.  Nothing is reconstructed from the fp32 outputs of the forward.
//
// Compiled like the tracer (-ffp-contract=off; every fused multiply-add spelled out); exp and expm1 are the double
// ones.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/radfoam_hip_entry_weights.h"
#include "rf_host.hpp"
#include "rf_ray_sweep.hpp"

#ifndef RF_ENTRY_WEIGHTS_RAYS_PER_WAVE
#define RF_ENTRY_WEIGHTS_RAYS_PER_WAVE 8
#endif

namespace rf {

constexpr int kWeightBlock = 256;
constexpr int kWeightWaves = kWeightBlock / 64;
constexpr int kWeightRays = RF_ENTRY_WEIGHTS_RAYS_PER_WAVE;    // rays per wave: rf_composite.hip's
using WeightSweep = RaySweep<kWeightRays, kWeightWaves>;
using WeightWave = WeightSweep::Wave;
using WeightStep = WeightSweep::Step;

// The running sums, T and w, and the ray's total of lane i below are spelled out as in rf_composite.hip: keep in step.

struct WeightForwardParams {
    uint32_t num_rays;
    int64_t total;               // S
    const int64_t *offsets;      // [R + 1]
    const float *t_enter, *t_exit, *sigma;   // [S]
    float *weights;              // [S]
    float *transmittance;        // [S], may be null
};

__global__ __launch_bounds__(kWeightBlock) void entry_weights_forward_kernel(WeightForwardParams p) {
    WeightWave w;
    if (!w.init(p.num_rays, p.total, p.offsets)) return;

    double carry_x = 0.0;
    for (int64_t base = w.first_base(); base < w.hi; base += 64) {
        const WeightStep s = WeightSweep::step(w, base);
        const SweepEntry e = sweep_entry(s, p.t_enter, p.t_exit, p.sigma);
        double sx[1] = {e.x};
        WeightSweep::scan(sx, w.lane, s.begin);
        const double sum_x = s.cont ? sx[0] + carry_x : sx[0];          // the ray's x up to and including this entry
        const double through = ::exp(-(sum_x - e.x));                    // T_e: exp(-0) = 1 at a ray's first entry
        const double weight = through * -::expm1(-e.x);
        if (s.valid) {                                                   // round once
            p.weights[s.k] = (float)weight;
            if (p.transmittance) p.transmittance[s.k] = (float)through;
        }
        carry_x = WeightSweep::carry(s, sum_x);
    }
}

struct WeightBackwardParams {
    uint32_t num_rays;
    int64_t total;
    const int64_t *offsets;
    const float *t_enter, *t_exit, *sigma;
    const float *grad_weights, *grad_transmittance;      // [S]; each may be null (zeros), not both
    float *grad_sigma, *grad_t_enter, *grad_t_exit;      // [S]; each may be null
};

// u_e = g_w[e] w_e + g_T[e] T_e (zero where the lane is not valid); g_w is handed back for the entry's own term
__device__ __forceinline__ double weight_u(const WeightBackwardParams &p, const WeightStep &s, double through,
                                           double weight, double &g_w) {
    g_w = 0.0;
    double u = 0.0;
    if (s.valid) {
        if (p.grad_weights) {
            g_w = (double)p.grad_weights[s.k];
            u = g_w * weight;
        }
        if (p.grad_transmittance) u = __builtin_fma((double)p.grad_transmittance[s.k], through, u);
    }
    return u;
}

__global__ __launch_bounds__(kWeightBlock) void entry_weights_backward_kernel(WeightBackwardParams p) {
    WeightWave w;
    if (!w.init(p.num_rays, p.total, p.offsets)) return;

    // ---- first sweep: lane i gets the sum of u over ray r0 + i, from the lane of the ray's last entry ----
    double ray_u = 0.0;
    {
        const int64_t next = WeightSweep::from_lane(w.off, (w.lane + 1) & 63);
        const bool mine = w.lane < w.nrays && next > w.off;
        const int64_t my_last = next - 1;
        double carry_x = 0.0, carry_u = 0.0;
        for (int64_t base = w.first_base(); base < w.hi; base += 64) {
            const WeightStep s = WeightSweep::step(w, base);
            const SweepEntry e = sweep_entry(s, p.t_enter, p.t_exit, p.sigma);
            double sx[1] = {e.x};
            WeightSweep::scan(sx, w.lane, s.begin);
            const double sum_x = s.cont ? sx[0] + carry_x : sx[0];
            const double through = ::exp(-(sum_x - e.x));
            const double weight = through * -::expm1(-e.x);
            double g_w;
            double su[1] = {weight_u(p, s, through, weight, g_w)};
            WeightSweep::scan(su, w.lane, s.begin);
            const double sum_u = s.cont ? su[0] + carry_u : su[0];

            const bool here = mine && my_last >= base && my_last < base + 64;
            const int src = here ? (int)(my_last - base) : w.lane;
            const double end_u = WeightSweep::from_lane(sum_u, src);
            if (here) ray_u = end_u;
            carry_x = WeightSweep::carry(s, sum_x);
            carry_u = WeightSweep::carry(s, sum_u);
        }
    }

    // ---- second sweep: the gradients ----
    double carry_x = 0.0, carry_u = 0.0;
    for (int64_t base = w.first_base(); base < w.hi; base += 64) {
        const WeightStep s = WeightSweep::step(w, base);
        const SweepEntry e = sweep_entry(s, p.t_enter, p.t_exit, p.sigma);
        double sx[1] = {e.x};
        WeightSweep::scan(sx, w.lane, s.begin);
        const double sum_x = s.cont ? sx[0] + carry_x : sx[0];
        const double through = ::exp(-(sum_x - e.x));            // T_e
        const double alpha = -::expm1(-e.x);
        const double weight = through * alpha;
        carry_x = WeightSweep::carry(s, sum_x);

        double g_w;
        double su[1] = {weight_u(p, s, through, weight, g_w)};
        WeightSweep::scan(su, w.lane, s.begin);
        const double sum_u = s.cont ? su[0] + carry_u : su[0];
        carry_u = WeightSweep::carry(s, sum_u);
        const double total_u = WeightSweep::from_lane(ray_u, s.ray);
        if (s.valid) {
            // g_w[e] T_e exp(-x_e) - (the ray's later u); exp(-x_e) = 1 - alpha_e
            const double dx = __builtin_fma(through * (1.0 - alpha), g_w, -(total_u - sum_u));
            const SweepGrad g = sweep_grad(e, dx);
            if (p.grad_sigma) p.grad_sigma[s.k] = (float)g.sigma;
            if (p.grad_t_exit) p.grad_t_exit[s.k] = (float)g.exit;
            if (p.grad_t_enter) p.grad_t_enter[s.k] = (float)(0.0 - g.exit);
        }
    }
}

}  // namespace rf

using namespace rf;

extern "C" {

uint32_t rf_entry_weights_rays_per_wave(void) { return (uint32_t)kWeightRays; }

int rf_entry_weights_forward(uint32_t num_rays, const int64_t *offsets, int64_t num_entries, const float *t_enter,
                             const float *t_exit, const float *sigma, float *weights, float *transmittance,
                             void *stream) {
    const char *what = "rf_entry_weights_forward";
    g_err[0] = 0;
    if (num_entries < 0) return fail(RF_ERR_INVALID_ARGUMENT, "%s: negative entry count", what);
    if (num_rays == 0 || num_entries == 0) return RF_OK;
    if (!offsets || !t_enter || !t_exit || !sigma || !weights)
        return fail(RF_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    WeightForwardParams p{};
    p.num_rays = num_rays;
    p.total = num_entries;
    p.offsets = offsets;
    p.t_enter = t_enter;
    p.t_exit = t_exit;
    p.sigma = sigma;
    p.weights = weights;
    p.transmittance = transmittance;
    hipLaunchKernelGGL(entry_weights_forward_kernel, dim3((uint32_t)WeightSweep::blocks(num_rays)), dim3(kWeightBlock),
                       0, static_cast<hipStream_t>(stream), p);
    return check_launch(what);
}

int rf_entry_weights_backward(uint32_t num_rays, const int64_t *offsets, int64_t num_entries, const float *t_enter,
                              const float *t_exit, const float *sigma, const float *grad_weights,
                              const float *grad_transmittance, float *grad_sigma, float *grad_t_enter,
                              float *grad_t_exit, void *stream) {
    const char *what = "rf_entry_weights_backward";
    g_err[0] = 0;
    if (num_entries < 0) return fail(RF_ERR_INVALID_ARGUMENT, "%s: negative entry count", what);
    if (num_rays == 0 || num_entries == 0) return RF_OK;
    if (!grad_sigma && !grad_t_enter && !grad_t_exit) return RF_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!grad_weights && !grad_transmittance) {                          // nothing came in: zeros go out
        float *outs[3] = {grad_sigma, grad_t_enter, grad_t_exit};
        for (float *out : outs)
            if (out && hipMemsetAsync(out, 0, (size_t)num_entries * sizeof(float), s) != hipSuccess)
                return check_launch(what);
        return RF_OK;
    }
    if (!offsets || !t_enter || !t_exit || !sigma) return fail(RF_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    WeightBackwardParams p{};
    p.num_rays = num_rays;
    p.total = num_entries;
    p.offsets = offsets;
    p.t_enter = t_enter;
    p.t_exit = t_exit;
    p.sigma = sigma;
    p.grad_weights = grad_weights;
    p.grad_transmittance = grad_transmittance;
    p.grad_sigma = grad_sigma;
    p.grad_t_enter = grad_t_enter;
    p.grad_t_exit = grad_t_exit;
    hipLaunchKernelGGL(entry_weights_backward_kernel, dim3((uint32_t)WeightSweep::blocks(num_rays)), dim3(kWeightBlock),
                       0, s, p);
    return check_launch(what);
}

}  // extern "C"
