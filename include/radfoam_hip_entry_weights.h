/*
 * radfoam_hip_entry_weights.h -- C-ABI of the per-entry compositing weights over an exported walk (libradfoam_hip.so,
 * rf_entry_weights.hip): the weight and the transmittance of every entry of a ragged list in
 * CSR form (radfoam_hip_segments.h) for a per-entry sigma[S], and the gradients of that.
 *
 * Conventions of radfoam_hip.h: every pointer is a DEVICE pointer, `stream` is a hipStream_t passed as void*, every
 * function returns RF_OK or a negative rf_status and leaves a message for rf_last_error.  Nothing synchronises.
 *
 * Per ray r over its entries e = offsets[r] .. offsets[r + 1] - 1, in order (radfoam_hip_composite.h's definitions):
 *     dt_e = 0 where t_exit[e] is infinite, else max(t_exit[e] - t_enter[e], 0)
 *     x_e  = sigma[e] dt_e
 *     T_e  = exp(-(sum of x_k over the ray's entries before e))          transmittance[e]
 *     w_e  = T_e (1 - exp(-x_e))                                         weights[e]
 * T is exactly 1 at a ray's first entry and w is exactly 0 behind an infinite t_exit.  Everything is formed in double on
 * the widened fp32 inputs and rounded to fp32 once.  One wave owns rf_entry_weights_rays_per_wave() consecutive rays and
 * nothing is accumulated with atomics: every output element is written exactly once, and two calls on the same inputs
 * give the same bits.
 *
 * offsets [num_rays + 1] (int64) must not decrease; every offset is clamped to 0 .. num_entries before anything is read
 * or written by it, so a list that breaks this gives wrong numbers, never an access outside the arrays.  Of every
 * output, the elements of the entries offsets[0] .. offsets[num_rays] - 1 are written, each once: all of them for a list
 * with offsets[0] = 0 and offsets[num_rays] = num_entries.
 */
#ifndef RADFOAM_HIP_ENTRY_WEIGHTS_H
#define RADFOAM_HIP_ENTRY_WEIGHTS_H

#include "radfoam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The number of consecutive rays one wave owns (a compile-time constant of the library). */
uint32_t rf_entry_weights_rays_per_wave(void);

/* weights, transmittance [num_entries] (fp32) from t_enter / t_exit / sigma [num_entries]: one sweep.  weights is
 * required; transmittance may be NULL and is then neither formed for output nor written.  Rays without entries have
 * nothing to write. */
int rf_entry_weights_forward(uint32_t num_rays, const int64_t *offsets, int64_t num_entries, const float *t_enter,
                             const float *t_exit, const float *sigma, float *weights, float *transmittance,
                             void *stream);

/* For grad_weights g_w and grad_transmittance g_T [num_entries] (fp32) and u_e = g_w[e] w_e + g_T[e] T_e:
 *     dL/dx_e         = g_w[e] T_e exp(-x_e) - (sum of u_k over the ray's LATER entries)
 *     grad_sigma[e]   = dL/dx_e dt_e
 *     grad_t_exit[e]  = dL/dx_e sigma[e]  where t_exit[e] is finite and t_exit[e] >= t_enter[e], else 0
 *     grad_t_enter[e] = -grad_t_exit[e]
 * Entries with an infinite t_exit get exact zeros in all three.  Each of the two incoming gradients may be NULL: it
 * then counts as zeros and is not read; with both NULL the outputs that are given are filled with zeros.  Each of the
 * three outputs (fp32 [num_entries]) may be NULL: it is then neither computed nor written.  One launch. */
int rf_entry_weights_backward(uint32_t num_rays, const int64_t *offsets, int64_t num_entries, const float *t_enter,
                              const float *t_exit, const float *sigma, const float *grad_weights,
                              const float *grad_transmittance, float *grad_sigma, float *grad_t_enter,
                              float *grad_t_exit, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RADFOAM_HIP_ENTRY_WEIGHTS_H */
