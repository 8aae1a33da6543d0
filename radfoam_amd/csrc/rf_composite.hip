// rf_composite.hip -- compositing over an exported walk with per-entry inputs, and its gradients
// (include/radfoam_hip_composite.h).
//
// Per ray r over its entries e, in order (the compositing of radfoam.composite_segments, with the density and the
// values of every entry left to the caller):
//     dt_e = 0 where t_exit[e] is infinite, else max(t_exit[e] - t_enter[e], 0),      x_e = sigma[e] dt_e
//     T_e = exp(-(sum of x_k over the ray's earlier entries)),      w_e = T_e (1 - exp(-x_e))
//     out[r][c] = sum_e w_e values[e][c],      out[r][C] = 1 - exp(-(sum_e x_e))
//
// The wave scheme -- one wave owns kCompRays consecutive rays and sweeps their entries 64 at a time, segmented scans in
// double, no atomics, no LDS, no lane returning before the wave's last cross-lane operation -- is rf_ray_sweep.hpp's.
// Here the per-channel sums are segmented reductions by its scan: the last lane of a ray's run in the step holds the
// run's sums, adds what the ray carried in, and when the ray ends there rounds ONCE to fp32 and stores the row.
//
// Forward: channels go in groups of at most kCompGroup, one launch (one sweep) per group, so that the carried sums stay
// in registers whatever C is; the first group writes the opacity as well.  Backward: one launch whatever C is, since
// only two sums are scanned (x, and w q with q_e = sum_c grad_out[r][c] values[e][c]); the suffix sum it needs is a
// ray's total minus an inclusive prefix, so the wave SWEEPS ITS RANGE TWICE: the first sweep leaves the totals of ray
// r0 + i in lane i, the second forms the gradients.  Nothing is reconstructed from the fp32 output of the forward.
//
// Compiled like the tracer (-ffp-contract=off; every fused multiply-add spelled out); exp and expm1 are the double
// ones.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/radfoam_hip_composite.h"
#include "rf_host.hpp"
#include "rf_ray_sweep.hpp"

#ifndef RF_COMPOSITE_RAYS_PER_WAVE
#define RF_COMPOSITE_RAYS_PER_WAVE 8
#endif

namespace rf {

constexpr int kCompBlock = 256;
constexpr int kCompWaves = kCompBlock / 64;
constexpr int kCompRays = RF_COMPOSITE_RAYS_PER_WAVE;      // rays per wave: chosen with scripts/gpu_composite_time.py
constexpr int kCompGroup = 4;                              // channels per forward sweep
using CompSweep = RaySweep<kCompRays, kCompWaves>;
using CompWave = CompSweep::Wave;
using CompStep = CompSweep::Step;

// The running sums, T and w in the backward, and the ray's total of lane i are spelled out here and, in step with
// this text, in rf_entry_weights.hip and rf_distortion.hip: as calls of shared helpers they change the kernels' code.

struct CompForwardParams {
    uint32_t num_rays, num_channels;
    uint32_t first_channel;      // this launch composites channels first_channel .. first_channel + NCH - 1
    uint32_t write_alpha;        // and the opacity, column num_channels
    int64_t total;               // S
    const int64_t *offsets;      // [R + 1]
    const float *t_enter, *t_exit, *sigma;   // [S]
    const float *values;         // [S][C]
    float *out;                  // [R][C + 1]
};

template <int NCH>
__global__ __launch_bounds__(kCompBlock) void composite_forward_kernel(CompForwardParams p) {
    CompWave w;
    if (!w.init(p.num_rays, p.total, p.offsets)) return;
    const size_t pitch = (size_t)p.num_channels + 1;

    // rays without entries: lane i answers for ray r0 + i
    {
        const int64_t next = CompSweep::from_lane(w.off, (w.lane + 1) & 63);
        if (w.lane < w.nrays && next == w.off) {
            float *row = p.out + (size_t)(w.r0 + w.lane) * pitch;
#pragma unroll
            for (int c = 0; c < NCH; ++c) row[p.first_channel + c] = 0.0f;
            if (p.write_alpha) row[p.num_channels] = 0.0f;
        }
    }

    double carry_x = 0.0, carry[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) carry[c] = 0.0;
    for (int64_t base = w.first_base(); base < w.hi; base += 64) {
        const CompStep s = CompSweep::step(w, base);
        const SweepEntry e = sweep_entry(s, p.t_enter, p.t_exit, p.sigma);
        double v[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) v[c] = 0.0;
        if (s.valid) {
            const float *row = p.values + (size_t)s.k * p.num_channels + p.first_channel;
#pragma unroll
            for (int c = 0; c < NCH; ++c) v[c] = (double)row[c];
        }

        double sx[1] = {e.x};
        CompSweep::scan(sx, w.lane, s.begin);
        const double sum_x = s.cont ? sx[0] + carry_x : sx[0];          // the ray's x up to and including this entry
        const double weight = sweep_weight(sum_x, e.x).weight;
#pragma unroll
        for (int c = 0; c < NCH; ++c) v[c] = weight * v[c];
        CompSweep::scan(v, w.lane, s.begin);
#pragma unroll
        for (int c = 0; c < NCH; ++c) v[c] = s.cont ? v[c] + carry[c] : v[c];

        if (s.last && s.ends) {                                          // the ray's sums are complete: round once
            float *row = p.out + (size_t)(w.r0 + s.ray) * pitch;
#pragma unroll
            for (int c = 0; c < NCH; ++c) row[p.first_channel + c] = (float)v[c];
            if (p.write_alpha) row[p.num_channels] = (float)-::expm1(-sum_x);
        }
        carry_x = CompSweep::carry(s, sum_x);
#pragma unroll
        for (int c = 0; c < NCH; ++c) carry[c] = CompSweep::carry(s, v[c]);
    }
}

struct CompBackwardParams {
    uint32_t num_rays, num_channels;
    int64_t total;
    const int64_t *offsets;
    const float *t_enter, *t_exit, *sigma, *values;
    const float *grad_out;       // [R][C + 1]
    float *grad_sigma, *grad_values, *grad_t_enter, *grad_t_exit;   // each may be null
};

__global__ __launch_bounds__(kCompBlock) void composite_backward_kernel(CompBackwardParams p) {
    CompWave w;
    if (!w.init(p.num_rays, p.total, p.offsets)) return;
    const uint32_t C = p.num_channels;
    const size_t pitch = (size_t)C + 1;
    const bool need_x = p.grad_sigma != nullptr || p.grad_t_enter != nullptr || p.grad_t_exit != nullptr;

    // ---- first sweep: lane i gets sum x and sum w q of ray r0 + i, from the lane of the ray's last entry ----
    double ray_x = 0.0, ray_wq = 0.0;
    if (need_x) {
        const int64_t next = CompSweep::from_lane(w.off, (w.lane + 1) & 63);
        const bool mine = w.lane < w.nrays && next > w.off;
        const int64_t my_last = next - 1;
        double carry_x = 0.0, carry_wq = 0.0;
        for (int64_t base = w.first_base(); base < w.hi; base += 64) {
            const CompStep s = CompSweep::step(w, base);
            const SweepEntry e = sweep_entry(s, p.t_enter, p.t_exit, p.sigma);
            double q = 0.0;
            if (s.valid) {
                const float *g = p.grad_out + (size_t)(w.r0 + s.ray) * pitch;
                const float *row = p.values + (size_t)s.k * C;
                for (uint32_t c = 0; c < C; ++c) q = __builtin_fma((double)g[c], (double)row[c], q);
            }
            double sx[1] = {e.x};
            CompSweep::scan(sx, w.lane, s.begin);
            const double sum_x = s.cont ? sx[0] + carry_x : sx[0];
            const double weight = ::exp(-(sum_x - e.x)) * -::expm1(-e.x);
            double swq[1] = {weight * q};
            CompSweep::scan(swq, w.lane, s.begin);
            const double sum_wq = s.cont ? swq[0] + carry_wq : swq[0];

            const bool here = mine && my_last >= base && my_last < base + 64;
            const int src = here ? (int)(my_last - base) : w.lane;
            const double end_x = CompSweep::from_lane(sum_x, src), end_wq = CompSweep::from_lane(sum_wq, src);
            if (here) {
                ray_x = end_x;
                ray_wq = end_wq;
            }
            carry_x = CompSweep::carry(s, sum_x);
            carry_wq = CompSweep::carry(s, sum_wq);
        }
    }
    const double ray_keep = ::exp(-ray_x);                       // what the whole ray lets through

    // ---- second sweep: the gradients ----
    double carry_x = 0.0, carry_wq = 0.0;
    for (int64_t base = w.first_base(); base < w.hi; base += 64) {
        const CompStep s = CompSweep::step(w, base);
        const SweepEntry e = sweep_entry(s, p.t_enter, p.t_exit, p.sigma);
        double sx[1] = {e.x};
        CompSweep::scan(sx, w.lane, s.begin);
        const double sum_x = s.cont ? sx[0] + carry_x : sx[0];
        const double through = ::exp(-(sum_x - e.x));            // T_e
        const double alpha = -::expm1(-e.x);
        const double weight = through * alpha;
        carry_x = CompSweep::carry(s, sum_x);

        double q = 0.0;
        if (s.valid) {
            const float *g = p.grad_out + (size_t)(w.r0 + s.ray) * pitch;
            const float *row = p.values + (size_t)s.k * C;
            float *grow = p.grad_values ? p.grad_values + (size_t)s.k * C : nullptr;
            for (uint32_t c = 0; c < C; ++c) {
                const double gc = (double)g[c];
                if (need_x) q = __builtin_fma(gc, (double)row[c], q);
                if (grow) grow[c] = (float)(weight * gc);
            }
        }
        if (!need_x) continue;                                           // wave-uniform

        double swq[1] = {weight * q};
        CompSweep::scan(swq, w.lane, s.begin);
        const double sum_wq = s.cont ? swq[0] + carry_wq : swq[0];
        carry_wq = CompSweep::carry(s, sum_wq);
        const double keep = CompSweep::from_lane(ray_keep, s.ray);
        const double total_wq = CompSweep::from_lane(ray_wq, s.ray);
        if (s.valid) {
            const double g_alpha = (double)p.grad_out[(size_t)(w.r0 + s.ray) * pitch + C];
            // T_e exp(-x_e) q_e - (the ray's later w q) + G[r][C] exp(-sum x); exp(-x_e) = 1 - alpha_e
            const double dx = __builtin_fma(g_alpha, keep, __builtin_fma(through * (1.0 - alpha), q, -(total_wq - sum_wq)));
            const SweepGrad g = sweep_grad(e, dx);
            if (p.grad_sigma) p.grad_sigma[s.k] = (float)g.sigma;
            if (p.grad_t_exit) p.grad_t_exit[s.k] = (float)g.exit;
            if (p.grad_t_enter) p.grad_t_enter[s.k] = (float)(0.0 - g.exit);
        }
    }
}

}  // namespace rf

using namespace rf;

namespace {

template <int NCH>
void comp_launch_forward(const CompForwardParams &p, hipStream_t stream) {
    hipLaunchKernelGGL(composite_forward_kernel<NCH>, dim3((uint32_t)CompSweep::blocks(p.num_rays)), dim3(kCompBlock),
                       0, stream, p);
}

}  // namespace

extern "C" {

uint32_t rf_composite_rays_per_wave(void) { return (uint32_t)kCompRays; }

int rf_composite_entries_forward(uint32_t num_rays, const int64_t *offsets, int64_t num_entries, const float *t_enter,
                                 const float *t_exit, const float *sigma, const float *values, uint32_t num_channels,
                                 float *out, void *stream) {
    const char *what = "rf_composite_entries_forward";
    g_err[0] = 0;
    if (num_entries < 0) return fail(RF_ERR_INVALID_ARGUMENT, "%s: negative entry count", what);
    if (num_channels == 0) return fail(RF_ERR_INVALID_ARGUMENT, "%s: no channels", what);
    if (num_rays == 0) return RF_OK;
    if (!out) return fail(RF_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (num_entries == 0) {
        if (hipMemsetAsync(out, 0, (size_t)num_rays * ((size_t)num_channels + 1) * sizeof(float), s) != hipSuccess)
            return check_launch(what);
        return RF_OK;
    }
    if (!offsets || !t_enter || !t_exit || !sigma || !values)
        return fail(RF_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    CompForwardParams p{};
    p.num_rays = num_rays;
    p.num_channels = num_channels;
    p.total = num_entries;
    p.offsets = offsets;
    p.t_enter = t_enter;
    p.t_exit = t_exit;
    p.sigma = sigma;
    p.values = values;
    p.out = out;
    for (uint32_t first = 0; first < num_channels; first += kCompGroup) {
        p.first_channel = first;
        p.write_alpha = first == 0;
        switch (num_channels - first < (uint32_t)kCompGroup ? num_channels - first : (uint32_t)kCompGroup) {
            case 1: comp_launch_forward<1>(p, s); break;
            case 2: comp_launch_forward<2>(p, s); break;
            case 3: comp_launch_forward<3>(p, s); break;
            default: comp_launch_forward<4>(p, s); break;
        }
        const int rc = check_launch(what);
        if (rc != RF_OK) return rc;
    }
    return RF_OK;
}

int rf_composite_entries_backward(uint32_t num_rays, const int64_t *offsets, int64_t num_entries, const float *t_enter,
                                  const float *t_exit, const float *sigma, const float *values, uint32_t num_channels,
                                  const float *grad_out, float *grad_sigma, float *grad_values, float *grad_t_enter,
                                  float *grad_t_exit, void *stream) {
    const char *what = "rf_composite_entries_backward";
    g_err[0] = 0;
    if (num_entries < 0) return fail(RF_ERR_INVALID_ARGUMENT, "%s: negative entry count", what);
    if (num_channels == 0) return fail(RF_ERR_INVALID_ARGUMENT, "%s: no channels", what);
    if (num_rays == 0 || num_entries == 0) return RF_OK;
    if (!grad_sigma && !grad_values && !grad_t_enter && !grad_t_exit) return RF_OK;
    if (!offsets || !t_enter || !t_exit || !sigma || !values || !grad_out)
        return fail(RF_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    CompBackwardParams p{};
    p.num_rays = num_rays;
    p.num_channels = num_channels;
    p.total = num_entries;
    p.offsets = offsets;
    p.t_enter = t_enter;
    p.t_exit = t_exit;
    p.sigma = sigma;
    p.values = values;
    p.grad_out = grad_out;
    p.grad_sigma = grad_sigma;
    p.grad_values = grad_values;
    p.grad_t_enter = grad_t_enter;
    p.grad_t_exit = grad_t_exit;
    hipLaunchKernelGGL(composite_backward_kernel, dim3((uint32_t)CompSweep::blocks(num_rays)), dim3(kCompBlock), 0,
                       static_cast<hipStream_t>(stream), p);
    return check_launch(what);
}

}  // extern "C"
