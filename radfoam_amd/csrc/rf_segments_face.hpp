// rf_segments_face.hpp -- what the two backward operators of the exported walk share (rf_segments_grad.hip,
// rf_segments_rays_grad.hip; DESIGN.md sections 4.9, 4.10).
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace rf {

__device__ __forceinline__ double seg_dot3(double ax, double ay, double az, double bx, double by, double bz) {
    return __builtin_fma(ax, bx, __builtin_fma(ay, by, az * bz));
}

// G of face j, the holder-aware total of section 4.9: grad_t_exit[j], and where j holds the running maximum
// (t_exit[j] > t_enter[j], from the stored floats) the grad_t_enter of the ray's later entries up to the next holder,
// included.  hi is the end of the ray's range.  0 for a face without a far side.  Params: t_enter, t_exit, g_enter,
// g_exit [S].
template <class Params>
__device__ __forceinline__ float seg_face_total(const Params &p, int64_t j, int64_t hi) {
    const float t1 = p.t_exit[j];
    if (t1 == __builtin_inff()) return 0.0f;
    float G = p.g_exit[j];
    if (t1 > p.t_enter[j]) {
        for (int64_t m = j + 1; m < hi; ++m) {
            G = G + p.g_enter[m];
            if (p.t_exit[m] > p.t_enter[m]) break;
        }
    }
    return G;
}

}  // namespace rf
