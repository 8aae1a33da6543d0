/*
 * radfoam_hip_composite.h -- C-ABI of the compositing over an exported walk (libradfoam_hip.so, rf_composite.hip;
 * DESIGN.md section 4.11): per-entry sigma[S] and values[S][C] along the intervals of a ragged list in CSR form
 * (radfoam_hip_segments.h), and the gradients of that.
 *
 * Conventions of radfoam_hip.h: every pointer is a DEVICE pointer, `stream` is a hipStream_t passed as void*, every
 * function returns RF_OK or a negative rf_status and leaves a message for rf_last_error.  Nothing synchronises.
 *
 * Per ray r over its entries e = offsets[r] .. offsets[r + 1] - 1, in order:
 *     dt_e = 0 where t_exit[e] is infinite, else max(t_exit[e] - t_enter[e], 0)
 *     x_e  = sigma[e] dt_e
 *     T_e  = exp(-(sum of x_k over the ray's entries before e))
 *     w_e  = T_e (1 - exp(-x_e))
 *     out[r][c] = sum_e w_e values[e][c]   (c < C),      out[r][C] = 1 - exp(-(sum_e x_e))
 * A ray without entries gets a row of zeros.  Everything is formed in double on the widened fp32 inputs and rounded to
 * fp32 once.  One wave owns rf_composite_rays_per_wave() consecutive rays and nothing is accumulated with atomics: every
 * output element is written exactly once, and two calls on the same inputs give the same bits.
 *
 * offsets [num_rays + 1] (int64) must not decrease; every offset is clamped to 0 .. num_entries before anything is read
 * or written by it, so a list that breaks this gives wrong numbers, never an access outside the arrays.
 */
#ifndef RADFOAM_HIP_COMPOSITE_H
#define RADFOAM_HIP_COMPOSITE_H

#include "radfoam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The number of consecutive rays one wave owns (a compile-time constant of the library). */
uint32_t rf_composite_rays_per_wave(void);

/* out [num_rays][num_channels + 1] (fp32): every element is written.  t_enter / t_exit / sigma hold num_entries
 * elements, values [num_entries][num_channels] row-major; num_channels >= 1. */
int rf_composite_entries_forward(uint32_t num_rays, const int64_t *offsets, int64_t num_entries, const float *t_enter,
                                 const float *t_exit, const float *sigma, const float *values, uint32_t num_channels,
                                 float *out, void *stream);

/* For grad_out [num_rays][num_channels + 1] (fp32) and q_e = sum_c grad_out[r][c] values[e][c]:
 *     grad_values[e][c] = w_e grad_out[r][c]
 *     dL/dx_e = T_e exp(-x_e) q_e - (sum of w_k q_k over the ray's LATER entries) + grad_out[r][C] exp(-(sum_e x_e))
 *     grad_sigma[e]   = dL/dx_e dt_e
 *     grad_t_exit[e]  = dL/dx_e sigma[e]  where t_exit[e] is finite and t_exit[e] >= t_enter[e], else 0
 *     grad_t_enter[e] = -grad_t_exit[e]
 * Entries with an infinite t_exit get exact zeros in grad_sigma, grad_t_exit and grad_t_enter.  Each of the four
 * outputs (grad_sigma, grad_t_enter, grad_t_exit [num_entries], grad_values [num_entries][num_channels]; fp32) may be
 * NULL: it is then neither computed nor written.  Of an output that is given, the elements of the entries
 * offsets[0] .. offsets[num_rays] - 1 are written, each once: all of them for a list with offsets[0] = 0 and
 * offsets[num_rays] = num_entries. */
int rf_composite_entries_backward(uint32_t num_rays, const int64_t *offsets, int64_t num_entries, const float *t_enter,
                                  const float *t_exit, const float *sigma, const float *values, uint32_t num_channels,
                                  const float *grad_out, float *grad_sigma, float *grad_values, float *grad_t_enter,
                                  float *grad_t_exit, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RADFOAM_HIP_COMPOSITE_H */
