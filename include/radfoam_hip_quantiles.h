/*
 * radfoam_hip_quantiles.h -- C-ABI of the depth quantiles over an exported walk (libradfoam_hip.so, rf_quantiles.hip;
 * DESIGN.md section 4.14): for every ray of a ragged list in CSR form (radfoam_hip_segments.h) and each of its
 * num_quantiles levels, the depth at which the ray's transmittance falls through the level and the entry it does so in,
 * and the gradients of those depths.
 *
 * Conventions of radfoam_hip.h: every pointer is a DEVICE pointer, `stream` is a hipStream_t passed as void*, every
 * function returns RF_OK or a negative rf_status and leaves a message for rf_last_error.  Nothing synchronises.
 *
 * Per ray r over its entries i = offsets[r] .. offsets[r + 1] - 1, in order (dt and x are those of
 * radfoam_hip_composite.h):
 *     dt_i = 0 where t_exit[i] is infinite, else max(t_exit[i] - t_enter[i], 0)
 *     x_i  = sigma[i] dt_i,   X_i = sum of x_k over k < i,   I_i = X_i + x_i
 *     L    = levels[r * num_quantiles + q]: -log of the quantile, >= 0; +inf for a level that is never reached
 *     j    = the first entry of the ray with I_j > L
 *     depth[r, q]   = t_enter[j] + (L - X_j) / sigma[j]
 *     entries[r, q] = j, an index into the list
 * and depth = -1, entries = -1 where the ray has no such entry (a ray without entries included).  The levels come as
 * doubles and are compared as they are: the caller takes the logarithm.  Everything is formed in double on the widened
 * fp32 inputs and rounded to fp32 once.  X_i is, to the bit, the I of the entry before (0 at a ray's first), so
 * neighbouring entries partition the axis of L without gaps or overlaps; j is the LOWEST entry whose I exceeds L.
 * sigma >= 0 is a precondition; negative densities give unspecified values, never an access outside the arrays.
 *
 * One wave owns rf_quantiles_rays_per_wave() consecutive rays and nothing is accumulated with atomics: every output
 * element is written exactly once, and two calls on the same inputs give the same bits.  num_quantiles is 1 ..
 * rf_quantiles_max().
 *
 * offsets [num_rays + 1] (int64) must not decrease; every offset is clamped to 0 .. num_entries before anything is read
 * or written by it, so a list that breaks this gives wrong numbers, never an access outside the arrays.
 */
#ifndef RADFOAM_HIP_QUANTILES_H
#define RADFOAM_HIP_QUANTILES_H

#include "radfoam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The number of consecutive rays one wave owns (a compile-time constant of the library). */
uint32_t rf_quantiles_rays_per_wave(void);

/* The largest num_quantiles the kernels take (a compile-time constant of the library). */
uint32_t rf_quantiles_max(void);

/* depth [num_rays * num_quantiles] (fp32) and entries [num_rays * num_quantiles] (int64): every element is written.
 * t_enter / t_exit / sigma hold num_entries elements (fp32), levels num_rays * num_quantiles (double).  With
 * num_entries == 0 only offsets, depth and entries are read or written. */
int rf_ray_quantiles_forward(uint32_t num_rays, const int64_t *offsets, int64_t num_entries, const float *t_enter,
                             const float *t_exit, const float *sigma, uint32_t num_quantiles, const double *levels,
                             float *depth, int64_t *entries, void *stream);

/* For grad_depth [num_rays * num_quantiles] (fp32), G_q = grad_depth[r, q], and the entries the forward wrote, j_q =
 * entries[r, q] (a pair with j_q outside 0 .. num_entries - 1, -1 among them, contributes nothing), c_q = G_q /
 * sigma[j_q], pass_k = t_exit[k] finite and >= t_enter[k]:
 *     grad_sigma[k]   = -dt_k (sum of c_q over j_q > k) - (sum over j_q == k of c_q (L_q - X_k) / sigma[k])
 *     grad_t_enter[k] = [pass_k] sigma[k] (sum of c_q over j_q > k) + (sum of G_q over j_q == k)
 *     grad_t_exit[k]  = -[pass_k] sigma[k] (sum of c_q over j_q > k)
 * Entries with an infinite t_exit get exact zeros in every gradient.  Each of the three outputs ([num_entries], fp32)
 * may be NULL: it is then neither computed nor written.  Of an output that is given, the elements of the entries
 * offsets[0] .. offsets[num_rays] - 1 are written, each once: all of them for a list with offsets[0] = 0 and
 * offsets[num_rays] = num_entries. */
int rf_ray_quantiles_backward(uint32_t num_rays, const int64_t *offsets, int64_t num_entries, const float *t_enter,
                              const float *t_exit, const float *sigma, uint32_t num_quantiles, const double *levels,
                              const int64_t *entries, const float *grad_depth, float *grad_sigma, float *grad_t_enter,
                              float *grad_t_exit, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RADFOAM_HIP_QUANTILES_H */
