// rf_segments_rays_grad.hip -- the exported walk's backward operator with respect to the RAYS:
// dL/dt_enter[S], dL/dt_exit[S] -> ray_grad[R][6] (include/radfoam_hip_segments.h).
//
// Terms of rf_segments_grad.hip: face j of ray r lies between a = cells[j] and b = next(j), n = p_b - p_a,
// m = (p_a + p_b) / 2, O the ray's origin, D its stored direction, d = D / |D|, num = (m - O) . n, dp = n . d, and the
// crossing is t = num / dp.  With the cell sequence held fixed
//     dt/dO = -n / dp
//     dt/dD = -num / (dp^2 |D|) (n - dp d)          (dt/dd = -num n / dp^2 through (I - d d^T) / |D|: nothing along D)
//     ray_grad[r][0:3] = sum over the ray's entries of G_j dt/dO,   ray_grad[r][3:6] = sum of G_j dt/dD
// with G_j the holder-aware total of section 4.9 (rf_segments_face.hpp::seg_face_total).  Faces with
// G_j == 0 exactly, or without a next cell, add nothing; dp = 0 gives non-finite values in that ray's row.
//
// ONE LANE PER ENTRY, 256 per block, every [S] array read coalesced.  A lane forms its six contributions in double on
// the widened fp32 inputs (dp is what a cancellation leaves and the grazing faces carry the result: section 4.9).  The
// entries of a ray are consecutive, so the six sums of a ray are a SEGMENTED REDUCTION: the wave runs an inclusive
// segmented scan in double over its 64 lanes (six steps, distance 1 .. 32, rf_ray_sweep.hpp's exchange of a double:
// ds_bpermute on its two halves), and the last lane of every run rounds to fp32 once and issues the six atomics: at
// most one update of a ray's row per (wave, ray) pair, exactly one for a ray that fits in a wave.  A lane knows where
// its run begins in the wave from data it has anyway: max(offsets[ray], the wave's first entry) - the wave's first
// entry.
//
// NO LANE RETURNS before the last cross-lane operation.  Lanes past the end of the list, lanes whose entry_ray is out
// of range or does not match the offsets, faces without a next cell and faces with G == 0 all stay and carry zeros;
// loads and stores are predicated instead.  A lane whose entry_ray is bad does not know its run: it takes the run of
// the nearest sound lane below it when that run reaches over it (so that the partial sums passing through it stay
// whole), and is a run of its own otherwise; a run's atomics are issued by its last SOUND lane.
//
// Compiled like the tracer (-ffp-contract=off; every fused multiply-add spelled out).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/radfoam_hip_segments.h"
#include "rf_host.hpp"
#include "rf_math.hpp"
#include "rf_ray_sweep.hpp"
#include "rf_segments_face.hpp"
#include "rf_wave.hpp"

namespace rf {

constexpr int kSegRaysBlock = 256;

struct SegRaysParams {
    uint32_t num_points, num_rays;
    int64_t total;               // S
    const float *points;         // [N][3]
    const float *rays;           // [R][6]
    const int64_t *offsets;      // [R + 1]
    const int32_t *entry_ray;    // [S]
    const uint32_t *cells;       // [S]
    const float *t_enter, *t_exit;
    const uint32_t *exit_cells;  // [R]
    const float *g_enter, *g_exit;
    float *ray_grad;             // [R][6], accumulated into
};

__global__ __launch_bounds__(kSegRaysBlock) void segments_rays_grad_kernel(SegRaysParams p) {
    const int lane = (int)(threadIdx.x & 63u);
    const int64_t k = (int64_t)blockIdx.x * kSegRaysBlock + threadIdx.x;
    const int64_t wave_first = k - lane;

    // ---- this lane's entry: sound (its ray is known and owns it) or not; nothing leaves the kernel here ----
    uint32_t ray = 0;
    int64_t hi = 0;
    int begin = lane, end = lane;                        // the run of this lane within the wave, [begin, end]
    bool sound = false;
    if (k < p.total) {
        ray = (uint32_t)p.entry_ray[k];
        if (ray < p.num_rays) {
            const int64_t lo = p.offsets[ray];
            hi = p.offsets[ray + 1];
            if (hi > p.total) hi = p.total;              // nothing is read past the list, whatever the offsets say
            if (k >= lo && k < hi) {
                sound = true;
                begin = (int)((lo > wave_first ? lo : wave_first) - wave_first);
                end = (int)((hi < wave_first + 64 ? hi : wave_first + 64) - 1 - wave_first);
            }
        }
    }

    // ---- the six contributions, in double; zeros for everything that adds nothing ----
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0, v4 = 0.0, v5 = 0.0;
    if (sound) {
        const uint32_t a = p.cells[k];
        const uint32_t b = k + 1 == hi ? p.exit_cells[ray] : p.cells[k + 1];
        const float Gf = (a < p.num_points && b < p.num_points) ? seg_face_total(p, k, hi) : 0.0f;
        if (Gf != 0.0f) {
            const float *rp = p.rays + (size_t)ray * 6;
            const double Ox = rp[0], Oy = rp[1], Oz = rp[2];
            const double Dx = rp[3], Dy = rp[4], Dz = rp[5];
            const double nrm = __builtin_sqrt(seg_dot3(Dx, Dy, Dz, Dx, Dy, Dz));
            const double dx = Dx / nrm, dy = Dy / nrm, dz = Dz / nrm;
            const float *pa = p.points + (size_t)a * 3;
            const float *pb = p.points + (size_t)b * 3;
            const double ax = pa[0], ay = pa[1], az = pa[2];
            const double bx = pb[0], by = pb[1], bz = pb[2];
            const double nx = bx - ax, ny = by - ay, nz = bz - az;
            const double mx = (ax + bx) / 2.0 - Ox, my = (ay + by) / 2.0 - Oy, mz = (az + bz) / 2.0 - Oz;
            const double num = seg_dot3(mx, my, mz, nx, ny, nz);
            const double dp = seg_dot3(nx, ny, nz, dx, dy, dz);
            const double G = Gf;
            const double wo = -G / dp;                                   // G dt/dO = wo n
            const double wd = -(G * num) / ((dp * dp) * nrm);            // G dt/dD = wd (n - dp d)
            v0 = wo * nx;
            v1 = wo * ny;
            v2 = wo * nz;
            v3 = wd * __builtin_fma(-dp, dx, nx);
            v4 = wd * __builtin_fma(-dp, dy, ny);
            v5 = wd * __builtin_fma(-dp, dz, nz);
        }
    }

    // ---- every lane is here.  A lane that is not sound joins the run of the nearest sound lane below, if that run
    // reaches over it: the partial sums of the scan pass through it.  (Runs are disjoint intervals of lanes, so the
    // nearest sound lane below is the only candidate.) ----
    const uint64_t sound_mask = ballot(sound);
    const uint64_t below = sound_mask & ((1ull << lane) - 1ull);
    const int nearest = below ? 63 - __builtin_clzll(below) : lane;
    const int run_of_nearest = __builtin_amdgcn_ds_bpermute(nearest << 2, begin | (end << 8));
    if (!sound && below && (run_of_nearest >> 8) >= lane) begin = run_of_nearest & 0xFF;

    // ---- inclusive segmented scan: after the step of distance s a lane holds the sum over max(begin, lane - 2s + 1)
    // .. lane.  The source index wraps below lane 0; what comes from there is not added. ----
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int src = (lane - s) & 63;
        const double u0 = WaveLanes::from_lane(v0, src), u1 = WaveLanes::from_lane(v1, src);
        const double u2 = WaveLanes::from_lane(v2, src), u3 = WaveLanes::from_lane(v3, src);
        const double u4 = WaveLanes::from_lane(v4, src), u5 = WaveLanes::from_lane(v5, src);
        if (lane - s >= begin) {
            v0 = v0 + u0;
            v1 = v1 + u1;
            v2 = v2 + u2;
            v3 = v3 + u3;
            v4 = v4 + u4;
            v5 = v5 + u5;
        }
    }

    // ---- no cross-lane operation below.  The last sound lane of a run holds the run's sums ----
    if (!sound) return;
    const uint64_t above = end > lane ? (sound_mask >> (lane + 1)) & ((1ull << (end - lane)) - 1ull) : 0ull;
    if (above) return;
    if (v0 == 0.0 && v1 == 0.0 && v2 == 0.0 && v3 == 0.0 && v4 == 0.0 && v5 == 0.0) return;
    float *dst = p.ray_grad + (size_t)ray * 6;
    unsafeAtomicAdd(dst + 0, (float)v0);
    unsafeAtomicAdd(dst + 1, (float)v1);
    unsafeAtomicAdd(dst + 2, (float)v2);
    unsafeAtomicAdd(dst + 3, (float)v3);
    unsafeAtomicAdd(dst + 4, (float)v4);
    unsafeAtomicAdd(dst + 5, (float)v5);
}

}  // namespace rf

using namespace rf;

extern "C" {

int rf_segments_rays_grad(uint32_t num_points, const float *points, uint32_t num_rays, const float *rays,
                          const int64_t *offsets, int64_t num_entries, const int32_t *entry_ray, const uint32_t *cells,
                          const float *t_enter, const float *t_exit, const uint32_t *exit_cells,
                          const float *grad_t_enter, const float *grad_t_exit, float *ray_grad, void *stream) {
    const char *what = "rf_segments_rays_grad";
    g_err[0] = 0;
    if (num_entries < 0) return fail(RF_ERR_INVALID_ARGUMENT, "%s: negative entry count", what);
    if (num_entries == 0 || num_rays == 0 || num_points == 0) return RF_OK;
    if (!points || !rays || !offsets || !entry_ray || !cells || !t_enter || !t_exit || !exit_cells || !grad_t_enter ||
        !grad_t_exit || !ray_grad)
        return fail(RF_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    const int64_t blocks = (num_entries + kSegRaysBlock - 1) / kSegRaysBlock;
    if (blocks > 0x7FFFFFFFll) return fail(RF_ERR_INVALID_ARGUMENT, "%s: too many entries for one launch", what);
    SegRaysParams p{};
    p.num_points = num_points;
    p.num_rays = num_rays;
    p.total = num_entries;
    p.points = points;
    p.rays = rays;
    p.offsets = offsets;
    p.entry_ray = entry_ray;
    p.cells = cells;
    p.t_enter = t_enter;
    p.t_exit = t_exit;
    p.exit_cells = exit_cells;
    p.g_enter = grad_t_enter;
    p.g_exit = grad_t_exit;
    p.ray_grad = ray_grad;
    hipLaunchKernelGGL(segments_rays_grad_kernel, dim3((uint32_t)blocks), dim3(kSegRaysBlock), 0,
                       static_cast<hipStream_t>(stream), p);
    return check_launch(what);
}

}  // extern "C"
