/*
 * radfoam_hip_distortion.h -- C-ABI of the distortion regulariser over an exported walk (libradfoam_hip.so,
 * rf_distortion.hip): one number per ray of a ragged list in CSR form (radfoam_hip_segments.h)
 * that measures how far the ray's compositing weights are spread in depth, and the gradients of that.
 *
 * Conventions of radfoam_hip.h: every pointer is a DEVICE pointer, `stream` is a hipStream_t passed as void*, every
 * function returns RF_OK or a negative rf_status and leaves a message for rf_last_error.  Nothing synchronises.
 *
 * Per ray r over its entries i = offsets[r] .. offsets[r + 1] - 1, in order (the weights are those of
 * radfoam_hip_composite.h):
 *     dt_i = 0 where t_exit[i] is infinite, else max(t_exit[i] - t_enter[i], 0)
 *     x_i  = sigma[i] dt_i,   T_i = exp(-(sum of x_k, k < i)),   w_i = T_i (1 - exp(-x_i))
 *     a_i, b_i = s_enter[i], s_exit[i] where the two are given, else t_enter[i], t_exit[i]
 *     m_i  = (a_i + b_i) / 2,   d_i = max(b_i - a_i, 0);   both 0, selected, where t_exit[i] is infinite
 *     W<_i = sum of w_k over k < i,   M<_i = sum of w_k m_k over k < i     (W>_i, M>_i: the same over k > i)
 *     out[r] = 2 sum_i w_i (m_i W<_i - M<_i) + (1/3) sum_i w_i^2 d_i
 * which is sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i wherever the midpoints of the entries that carry weight
 * do not decrease along the ray.  A ray without entries gets 0.  Everything is formed in double on the widened fp32
 * inputs and rounded to fp32 once.  One wave owns rf_distortion_rays_per_wave() consecutive rays and nothing is
 * accumulated with atomics: every output element is written exactly once, and two calls on the same inputs give the
 * same bits.
 *
 * offsets [num_rays + 1] (int64) must not decrease; every offset is clamped to 0 .. num_entries before anything is read
 * or written by it, so a list that breaks this gives wrong numbers, never an access outside the arrays.  s_enter and
 * s_exit are both given or both NULL.
 */
#ifndef RADFOAM_HIP_DISTORTION_H
#define RADFOAM_HIP_DISTORTION_H

#include "radfoam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The number of consecutive rays one wave owns (a compile-time constant of the library). */
uint32_t rf_distortion_rays_per_wave(void);

/* out [num_rays] (fp32): every element is written.  t_enter / t_exit / sigma, and s_enter / s_exit where given, hold
 * num_entries elements (fp32). */
int rf_ray_distortion_forward(uint32_t num_rays, const int64_t *offsets, int64_t num_entries, const float *t_enter,
                              const float *t_exit, const float *sigma, const float *s_enter, const float *s_exit,
                              float *out, void *stream);

/* For grad_out [num_rays] (fp32), G = grad_out[r]:
 *     g_i           = 2 (m_i W<_i - M<_i) + 2 (M>_i - m_i W>_i) + (2/3) w_i d_i           (d out / d w_i)
 *     d out / d m_i = 2 w_i (W<_i - W>_i),      d out / d d_i = w_i^2 / 3
 *     grad_b_i      = G (1/2 d out/d m_i + [b_i >= a_i] d out/d d_i)
 *     grad_a_i      = G (1/2 d out/d m_i - [b_i >= a_i] d out/d d_i)
 *     dL/dx_i       = G (T_i exp(-x_i) g_i - (sum of w_k g_k over k > i))      with sum_k w_k g_k = 2 out[r]
 *     grad_sigma[i] = dL/dx_i dt_i
 *     through w: grad_t_exit[i] = dL/dx_i sigma[i] where t_exit[i] is finite and >= t_enter[i], else 0;
 *                grad_t_enter[i] = -grad_t_exit[i]
 * With s_enter / s_exit given, grad_s_enter = grad_a, grad_s_exit = grad_b and the times get the part through w alone;
 * without them the times get the sum of both parts, and grad_s_enter / grad_s_exit must be NULL.  Entries with an
 * infinite t_exit get exact zeros in every gradient.  Each of the five outputs ([num_entries], fp32) may be NULL: it is
 * then neither computed nor written.  Of an output that is given, the elements of the entries offsets[0] ..
 * offsets[num_rays] - 1 are written, each once: all of them for a list with offsets[0] = 0 and offsets[num_rays] =
 * num_entries. */
int rf_ray_distortion_backward(uint32_t num_rays, const int64_t *offsets, int64_t num_entries, const float *t_enter,
                               const float *t_exit, const float *sigma, const float *s_enter, const float *s_exit,
                               const float *grad_out, float *grad_sigma, float *grad_t_enter, float *grad_t_exit,
                               float *grad_s_enter, float *grad_s_exit, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RADFOAM_HIP_DISTORTION_H */
