/*
 * radfoam_hip_sh_entries.h -- C-ABI of the tracer's colour per entry of an exported walk (libradfoam_hip.so,
 * rf_sh_entries.hip): for a per-cell table of spherical-harmonic coefficients
 * coeffs [num_cells, 3 K], K = (degree + 1)^2 (element i is channel i % 3 of basis function i / 3: the layout of the
 * tracer's attribute row without its density), and the ray directions [num_rays, 3],
 *     dhat = d / |d|,      rgb[e, c] = max(0.5 + sum_k Y_k(dhat_ray(e)) coeffs[cell(e), 3 k + c], 0)
 * with the basis, the order of operations and the roundings of the tracer's forward kernel, so that rgb is the colour
 * the tracer gives that cell on that ray bit for bit (without its density gate); and the gradients of rgb with respect
 * to coeffs and to the directions.  The gradient of the clamp is zero where rgb == 0.
 *
 * Conventions of radfoam_hip.h: every pointer is a DEVICE pointer, `stream` is a hipStream_t passed as void*, every
 * function returns RF_OK or a negative rf_status and leaves a message for rf_last_error.  Nothing synchronises.
 * Arguments are checked before the device is touched.  degree is 0 .. 3; fp32 throughout.
 *
 * The walk is given three ways, each to the kernel that reads it coalesced:
 *     cells[e]         int64 [num_entries]: the cell of every entry
 *     entry_rays[e]    int32 [num_entries]: the ray of every entry
 *     offsets[r]       int64 [num_rays + 1]: ray r owns the entries offsets[r] .. offsets[r + 1] - 1
 *     sorted_cells[k], entries[k]   int64 [num_entries]: the index of radfoam_hip_cell_reduce.h
 * Every index read from memory is range-checked where it is read: an entry whose cell lies outside 0 .. num_cells - 1
 * or whose ray lies outside 0 .. num_rays - 1 gets a colour of zeros and adds nothing to a gradient; positions whose
 * entry lies outside 0 .. num_entries - 1 are skipped; offsets are clamped to 0 .. num_entries and made
 * non-decreasing.  Wrong indices give wrong numbers, never an access outside the arrays.
 *
 * No atomics anywhere; every output element is written once (grad_coeffs after one clearing fill); two calls on the
 * same inputs give the same bits.
 */
#ifndef RADFOAM_HIP_SH_ENTRIES_H
#define RADFOAM_HIP_SH_ENTRIES_H

#include "radfoam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The number of basis functions one sweep of rf_sh_entries_backward_coeffs sums (a compile-time constant). */
uint32_t rf_sh_entries_group(void);

/* rgb [num_entries * 3]: every element is written.  Row c of coeffs begins at coeffs + c * coeff_pitch floats,
 * coeff_pitch >= 3 K; rows need only be 4-byte aligned.  directions need not be unit length. */
int rf_sh_entries_forward(uint32_t degree, int64_t num_cells, int64_t num_entries, uint32_t num_rays,
                          const int64_t *cells, const int32_t *entry_rays, const float *coeffs, uint32_t coeff_pitch,
                          const float *directions, float *rgb, void *stream);

/* Bytes of workspace rf_sh_entries_backward_coeffs needs: two rows of 3 K doubles per chunk of
 * rf_reduce_entries_chunk() positions.  0 for a negative num_entries or a degree above 3. */
size_t rf_sh_entries_workspace_bytes(int64_t num_entries, uint32_t degree);

/* grad_coeffs [num_cells * 3 K], packed: every element is written,
 *     grad_coeffs[n, 3 k + c] = sum over the entries e of cell n of Y_k(dhat_ray(e)) (rgb[e, c] > 0 ? grad_rgb[e, c] : 0),
 * each product rounded to fp32, summed in double over the cell's list, rounded once: the sum per cell of
 * rf_reduce_entries with the row formed in registers.  rgb is what rf_sh_entries_forward returned.  workspace at least
 * rf_sh_entries_workspace_bytes(num_entries, degree) bytes, 8-byte aligned. */
int rf_sh_entries_backward_coeffs(uint32_t degree, int64_t num_cells, int64_t num_entries, uint32_t num_rays,
                                  const int64_t *sorted_cells, const int64_t *entries, const int32_t *entry_rays,
                                  const float *directions, const float *rgb, const float *grad_rgb, float *grad_coeffs,
                                  void *workspace, size_t workspace_bytes, void *stream);

/* grad_directions [num_rays * 3]: every element is written; exact zeros for a ray without entries and for degree 0.
 * Per entry q_e = sum_c m[e, c] grad_rgb[e, c] sum_k grad Y_k(dhat) coeffs[cell, 3 k + c], summed per ray in double,
 * then through the normalisation: (q - dhat (dhat . q)) / |d|. */
int rf_sh_entries_backward_directions(uint32_t degree, int64_t num_cells, int64_t num_entries, uint32_t num_rays,
                                      const int64_t *offsets, const int64_t *cells, const float *coeffs,
                                      uint32_t coeff_pitch, const float *directions, const float *rgb,
                                      const float *grad_rgb, float *grad_directions, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RADFOAM_HIP_SH_ENTRIES_H */
