// rf_quantiles.hip -- depth quantiles over an exported walk, and their gradients
// (include/radfoam_hip_quantiles.h).
//
// Per ray r over its entries i, in order (dt and x are rf_composite.hip's), for each of its Q levels L = levels[r, q]:
//     dt_i = 0 where t_exit[i] is infinite, else max(t_exit[i] - t_enter[i], 0),      x_i = sigma[i] dt_i
//     X_i = sum of x_k, k < i,      I_i = X_i + x_i
//     j = the first entry of the ray with I_j > L
//     depth[r, q] = t_enter[j] + (L - X_j) / sigma[j],      entries[r, q] = j;      -1 / -1 where there is no such j
//
// The wave scheme -- one wave owns kQuantRays consecutive rays and sweeps their entries 64 at a time, a segmented scan
// in double, no atomics, no LDS, no lane returning before the wave's last cross-lane operation -- is
// rf_ray_sweep.hpp's.
//
// One scan per step (x).  A lane's X is THE VERY BITS ITS PREDECESSOR HOLDS AS I: lane - 1's value, or at a run's head
// what the ray carried in (0 for a ray that begins there); it is not I - x.  Neighbouring lanes then partition the axis
// of L without gaps or overlaps.  The tree scan is not monotone to the last bit, so the crossing lane of (ray, q) is
// the LOWEST lane of the run whose I exceeds L, found by a ballot masked to the run, and a ray that continues past a
// step carries, next to its running sum, a wave-uniform bitmask of the quantiles it has crossed: hence kQuantMax.
// The crossing lane writes depth (rounded once to fp32) and entries; a pair never crossed gets -1 / -1 from the lane of
// the ray's last entry, or from lane i for a ray r0 + i without entries.  Every (ray, q) has exactly one writer.
//
// The backward sweeps once with the same scan (X_k is needed in double at crossing lanes) and reads the entries the
// forward wrote, range-checked before anything is gathered by them.  Nothing is reconstructed from the fp32 depth.
//
// Compiled like the tracer (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/radfoam_hip_quantiles.h"
#include "rf_host.hpp"
#include "rf_ray_sweep.hpp"

#ifndef RF_QUANTILES_RAYS_PER_WAVE
#define RF_QUANTILES_RAYS_PER_WAVE 8
#endif

namespace rf {

constexpr int kQuantBlock = 256;
constexpr int kQuantWaves = kQuantBlock / 64;
constexpr int kQuantRays = RF_QUANTILES_RAYS_PER_WAVE;     // rays per wave: 4, 8, 16 measured equal, 2 and 32 slower
constexpr int kQuantMax = 8;                               // quantiles per ray: one bit each in the carried mask
using QuantSweep = RaySweep<kQuantRays, kQuantWaves>;
using QuantWave = QuantSweep::Wave;
using QuantStep = QuantSweep::Step;
static_assert(kQuantMax >= 1 && kQuantMax <= 32, "the carried mask of crossed quantiles is one 32-bit register");

// ---- the sums of a step: upto = I_k, before = X_k as the bits the entry before holds as I ----
struct QuantSums {
    double upto, before;
};

__device__ __forceinline__ QuantSums quant_sums(const QuantWave &w, const QuantStep &s, const SweepEntry &e,
                                                double &carry_x) {
    QuantSums o;
    o.upto = QuantSweep::running(w, s, e.x, carry_x);
    const double below = QuantSweep::from_lane(o.upto, (w.lane - 1) & 63);
    o.before = w.lane > s.begin ? below : (s.cont ? carry_x : 0.0);
    carry_x = QuantSweep::carry(s, o.upto);
    return o;
}

struct QuantParams {
    uint32_t num_rays;
    uint32_t num_q;              // Q: 1 .. kQuantMax
    int64_t total;               // S
    const int64_t *offsets;      // [R + 1]
    const float *t_enter, *t_exit, *sigma;   // [S]
    const double *levels;        // [R, Q]
    float *depth;                // forward: [R, Q]
    int64_t *entries;            // forward: [R, Q], written; backward: read
    const float *grad_depth;     // backward: [R, Q]
    float *grad_sigma, *grad_t_enter, *grad_t_exit;   // backward: each may be null
};

__global__ __launch_bounds__(kQuantBlock) void ray_quantiles_forward_kernel(QuantParams p) {
    QuantWave w;
    if (!w.init(p.num_rays, p.total, p.offsets)) return;
    const int num_q = (int)p.num_q;
    const int64_t next = QuantSweep::from_lane(w.off, (w.lane + 1) & 63);
    const bool empty = w.lane < w.nrays && next <= w.off;               // lane i: ray r0 + i has no entries
    const uint64_t below_me = ((uint64_t)1 << w.lane) - 1;
    double carry_x = 0.0;
    uint32_t carry_done = 0;                                             // of the ray that runs past the step before
    for (int64_t base = w.first_base(); base < w.hi; base += 64) {
        const QuantStep s = QuantSweep::step(w, base);
        const SweepEntry e = sweep_entry(s, p.t_enter, p.t_exit, p.sigma);
        const uint32_t done_before = s.cont ? carry_done : 0u;
        const QuantSums sum = quant_sums(w, s, e, carry_x);
        const uint64_t my_run = (~(uint64_t)0 << s.begin) & below_me;    // the lanes of my run below me
        const int64_t row = (w.r0 + s.ray) * num_q;                      // valid: ray < nrays, so the row exists
        uint32_t done = done_before;
        for (int q = 0; q < num_q; ++q) {                                // wave-uniform trip count
            const double level = s.valid ? p.levels[row + q] : 0.0;
            const bool above = s.valid && sum.upto > level;
            const uint64_t ballot = __builtin_amdgcn_ballot_w64(above);
            const bool prior = ((done_before >> q) & 1u) != 0 || (ballot & my_run) != 0;
            if (above && !prior) {                                       // the lowest lane of the ray above the level
                p.depth[row + q] = (float)((double)e.t0 + (level - sum.before) / e.sigma);
                p.entries[row + q] = s.k;
            }
            if (above || prior) done |= 1u << q;
        }
        if (s.ends && s.last) {                                          // the ray's last entry: what it never crossed
            for (int q = 0; q < num_q; ++q) {
                if (((done >> q) & 1u) == 0) {
                    p.depth[row + q] = -1.0f;
                    p.entries[row + q] = -1;
                }
            }
        }
        carry_done = (uint32_t)__builtin_amdgcn_readlane((int)(s.last && !s.ends ? done : 0u), 63);
    }
    if (empty) {
        const int64_t row = (w.r0 + w.lane) * num_q;
        for (int q = 0; q < num_q; ++q) {
            p.depth[row + q] = -1.0f;
            p.entries[row + q] = -1;
        }
    }
}

__global__ __launch_bounds__(kQuantBlock) void ray_quantiles_backward_kernel(QuantParams p) {
    QuantWave w;
    if (!w.init(p.num_rays, p.total, p.offsets)) return;
    const int num_q = (int)p.num_q;
    double carry_x = 0.0;
    for (int64_t base = w.first_base(); base < w.hi; base += 64) {
        const QuantStep s = QuantSweep::step(w, base);
        const SweepEntry e = sweep_entry(s, p.t_enter, p.t_exit, p.sigma);
        const QuantSums sum = quant_sums(w, s, e, carry_x);
        if (s.valid) {                                                   // no cross-lane operation in here
            const int64_t row = (w.r0 + s.ray) * num_q;
            double later = 0.0;                      // sum of G_q / sigma[j_q] over the quantiles that cross behind it
            double own_sigma = 0.0, own_enter = 0.0;                     // the terms of the quantiles that cross in it
            for (int q = 0; q < num_q; ++q) {
                const int64_t j = p.entries[row + q];
                if (j < s.k || j >= p.total) continue;                   // -1, in front of the entry, or no index
                const double g = (double)p.grad_depth[row + q];
                if (j > s.k) {
                    later = later + g / (double)p.sigma[j];
                } else {
                    const double c = g / e.sigma;
                    own_sigma = own_sigma + c * (p.levels[row + q] - sum.before) / e.sigma;
                    own_enter = own_enter + g;
                }
            }
            const double through = e.moves ? e.sigma * later : 0.0;
            const double g_sigma = e.infinite ? 0.0 : (0.0 - e.dt * later) - own_sigma;
            const double g_enter = e.infinite ? 0.0 : through + own_enter;
            const double g_exit = 0.0 - through;
            if (p.grad_sigma) p.grad_sigma[s.k] = (float)g_sigma;
            if (p.grad_t_enter) p.grad_t_enter[s.k] = (float)g_enter;
            if (p.grad_t_exit) p.grad_t_exit[s.k] = (float)g_exit;
        }
    }
}

}  // namespace rf

using namespace rf;

extern "C" {

uint32_t rf_quantiles_rays_per_wave(void) { return (uint32_t)kQuantRays; }

uint32_t rf_quantiles_max(void) { return (uint32_t)kQuantMax; }

int rf_ray_quantiles_forward(uint32_t num_rays, const int64_t *offsets, int64_t num_entries, const float *t_enter,
                             const float *t_exit, const float *sigma, uint32_t num_quantiles, const double *levels,
                             float *depth, int64_t *entries, void *stream) {
    const char *what = "rf_ray_quantiles_forward";
    g_err[0] = 0;
    if (num_entries < 0) return fail(RF_ERR_INVALID_ARGUMENT, "%s: negative entry count", what);
    if (num_rays == 0) return RF_OK;
    if (num_quantiles < 1 || num_quantiles > (uint32_t)kQuantMax)
        return fail(RF_ERR_INVALID_ARGUMENT, "%s: the number of quantiles must be 1 .. rf_quantiles_max()", what);
    if (!offsets || !depth || !entries) return fail(RF_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    if (num_entries > 0 && (!t_enter || !t_exit || !sigma || !levels))
        return fail(RF_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    QuantParams p{};
    p.num_rays = num_rays;
    p.num_q = num_quantiles;
    p.total = num_entries;
    p.offsets = offsets;
    p.t_enter = t_enter;
    p.t_exit = t_exit;
    p.sigma = sigma;
    p.levels = levels;
    p.depth = depth;
    p.entries = entries;
    hipLaunchKernelGGL(ray_quantiles_forward_kernel, dim3((uint32_t)QuantSweep::blocks(num_rays)), dim3(kQuantBlock), 0,
                       static_cast<hipStream_t>(stream), p);
    return check_launch(what);
}

int rf_ray_quantiles_backward(uint32_t num_rays, const int64_t *offsets, int64_t num_entries, const float *t_enter,
                              const float *t_exit, const float *sigma, uint32_t num_quantiles, const double *levels,
                              const int64_t *entries, const float *grad_depth, float *grad_sigma, float *grad_t_enter,
                              float *grad_t_exit, void *stream) {
    const char *what = "rf_ray_quantiles_backward";
    g_err[0] = 0;
    if (num_entries < 0) return fail(RF_ERR_INVALID_ARGUMENT, "%s: negative entry count", what);
    if (num_rays == 0 || num_entries == 0) return RF_OK;
    if (!grad_sigma && !grad_t_enter && !grad_t_exit) return RF_OK;
    if (num_quantiles < 1 || num_quantiles > (uint32_t)kQuantMax)
        return fail(RF_ERR_INVALID_ARGUMENT, "%s: the number of quantiles must be 1 .. rf_quantiles_max()", what);
    if (!offsets || !t_enter || !t_exit || !sigma || !levels || !entries || !grad_depth)
        return fail(RF_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    QuantParams p{};
    p.num_rays = num_rays;
    p.num_q = num_quantiles;
    p.total = num_entries;
    p.offsets = offsets;
    p.t_enter = t_enter;
    p.t_exit = t_exit;
    p.sigma = sigma;
    p.levels = levels;
    p.entries = const_cast<int64_t *>(entries);
    p.grad_depth = grad_depth;
    p.grad_sigma = grad_sigma;
    p.grad_t_enter = grad_t_enter;
    p.grad_t_exit = grad_t_exit;
    hipLaunchKernelGGL(ray_quantiles_backward_kernel, dim3((uint32_t)QuantSweep::blocks(num_rays)), dim3(kQuantBlock),
                       0, static_cast<hipStream_t>(stream), p);
    return check_launch(what);
}

}  // extern "C"
