// rf_segments.hip -- the walk of every ray as data: the cells it scans, in order, and the ray parameters at which it
// enters and leaves each (include/radfoam_hip_segments.h).
//
// One lane walks one ray over the PREPARED workspace of rf_prepare_foam (rf_foam.hpp: cell records {x, y, z, density},
// planar fp16 face blocks, links, padded offsets) -- the tables forward_kernel of rf_kernels.hip reads, and the same walk:
//   scan      the reference's, tracing_utils.cuh:43-67, evaluated the way the reference writes it: every face of the padded
//             list divided (IEEE), a running minimum of the rounded quotients with a strict '<' -- scan_faces_strict of
//             rf_kernels.hip and scan_cell_strict_padded of the CPU checker.  num = ((P + o/2) - O).o and dp = o.d in the
//             association of rf_math.hpp::dot3, o the fp16 offset of the table.  A padding entry never wins (see "the
//             face scan" in rf_kernels.hip); should one, its own link is followed, which is the link of the face it copies.
//   ending    no exit, transmittance T <= weight_threshold after a segment, or the step that overruns max_intersections
//             (counted, not scanned): forward_kernel's operations in forward_kernel's order.  T needs the density only
//             (alpha = 1 - exp(-s dt), T *= 1 - alpha); no colour row is read.
// The result is ragged, so the kernel is one template run twice: <FILL = false> counts the entries of every ray, the
// caller turns the counts into offsets (a prefix sum), <FILL = true> walks again and writes.  Every element of the
// outputs is written once, by plain stores; a ray never writes outside its own range of the offsets it is given.
//
// The translation unit is compiled like the tracer (-ffp-contract=off; every fused multiply-add spelled out), which is
// what makes the walk bit-identical to forward_kernel's.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/radfoam_hip_segments.h"
#include "rf_foam.hpp"
#include "rf_host.hpp"
#include "rf_math.hpp"
#include "rf_wave.hpp"

namespace rf {

constexpr int kSegBlock = 256;

struct SegParams {
    const float4 *cells;      // {x, y, z, density}
    const uint32_t *geo;      // face blocks, 6 dwords each: half x[4], y[4], z[4]
    const Link *link;
    const uint32_t *poff;
    rf_trace_settings settings;
    uint32_t num_points, num_rays;
    const float *rays;
    const uint32_t *start;
    uint32_t *counts;         // count pass
    uint32_t *nint;           // count pass, optional
    const int64_t *offsets;   // fill pass: [num_rays + 1]
    uint32_t *out_cells;
    float *t_enter, *t_exit;
};

// a face block arrives as one 16-byte and one 8-byte load; blocks are 8-byte aligned (24 bytes each)
struct __attribute__((aligned(8))) SegGeoXY {
    uint32_t x01, x23, y01, y23;
};
struct __attribute__((aligned(8))) SegGeoZ {
    uint32_t z01, z23;
};

struct SegExit {
    float t1;
    uint32_t k;   // winning entry, relative to the cell's first entry; kNone: no exit
};

// one face of the reference's loop: take it if dp > 0 and its rounded quotient is strictly smaller
__device__ __forceinline__ void seg_face(SegExit &r, uint32_t k, float ox, float oy, float oz, float Px, float Py, float Pz,
                                         float Ox, float Oy, float Oz, float dx, float dy, float dz) {
    const float dp = dot3(ox, oy, oz, dx, dy, dz);
    const float vx = fma_(ox, 0.5f, Px) - Ox;      // (P + o/2) - O; o/2 is exact, so P + o/2 is one rounding
    const float vy = fma_(oy, 0.5f, Py) - Oy;
    const float vz = fma_(oz, 0.5f, Pz) - Oz;
    const float t = dot3(vx, vy, vz, ox, oy, oz) / dp;
    const bool take = (dp > 0.0f) & (t < r.t1);
    r.t1 = take ? t : r.t1;
    r.k = take ? k : r.k;
}

// the dividing scan over the cnt (a multiple of 4) padded entries that start at dword `src`
__device__ __forceinline__ SegExit seg_scan(const uint32_t *src, uint32_t cnt, float Px, float Py, float Pz, float Ox,
                                            float Oy, float Oz, float dx, float dy, float dz) {
    SegExit r;
    r.t1 = __builtin_inff();
    r.k = kNone;
    for (uint32_t k = 0; k < cnt; k += 4) {
        const SegGeoXY A = *reinterpret_cast<const SegGeoXY *>(src);
        const SegGeoZ B = *reinterpret_cast<const SegGeoZ *>(src + 4);
        src += 6;
        seg_face(r, k + 0u, half_lo(A.x01), half_lo(A.y01), half_lo(B.z01), Px, Py, Pz, Ox, Oy, Oz, dx, dy, dz);
        seg_face(r, k + 1u, half_hi(A.x01), half_hi(A.y01), half_hi(B.z01), Px, Py, Pz, Ox, Oy, Oz, dx, dy, dz);
        seg_face(r, k + 2u, half_lo(A.x23), half_lo(A.y23), half_lo(B.z23), Px, Py, Pz, Ox, Oy, Oz, dx, dy, dz);
        seg_face(r, k + 3u, half_hi(A.x23), half_hi(A.y23), half_hi(B.z23), Px, Py, Pz, Ox, Oy, Oz, dx, dy, dz);
    }
    return r;
}

// Control flow as in forward_kernel: every lane keeps an `alive` flag and the wave iterates while any lane is alive (no
// per-lane break out of nested conditionals).
template <bool FILL>
__global__ __launch_bounds__(kSegBlock) void segments_kernel(SegParams p) {
    const uint32_t ray = blockIdx.x * (uint32_t)kSegBlock + threadIdx.x;
    const bool valid = ray < p.num_rays;
    bool alive = valid;

    float Ox = 0.0f, Oy = 0.0f, Oz = 0.0f, dx = 0.0f, dy = 0.0f, dz = 1.0f;
    uint32_t cur = 0;
    if (alive) {
        const float *rp = p.rays + (size_t)ray * 6;
        Ox = rp[0];
        Oy = rp[1];
        Oz = rp[2];
        dx = rp[3];
        dy = rp[4];
        dz = rp[5];
        const float nrm = sqrtf(dot3(dx, dy, dz, dx, dy, dz));
        dx = dx / nrm;
        dy = dy / nrm;
        dz = dz / nrm;
        cur = p.start[ray];
        if (cur >= p.num_points) alive = false;   // not a cell: no entries
    }

    int64_t base = 0, room = 0;
    if constexpr (FILL) {
        if (alive) {
            base = p.offsets[ray];
            room = p.offsets[ray + 1] - base;
        }
    }

    const float thr = p.settings.weight_threshold;
    const uint32_t max_steps = p.settings.max_intersections;
    float T = 1.0f, t0 = 0.0f;
    uint32_t n = 0, entries = 0;
    uint32_t nb = 0, cnt = 0;
    float4 head = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (alive) {
        nb = p.poff[cur];
        cnt = p.poff[cur + 1] - nb;
        head = p.cells[cur];
    }
    while (ballot(alive) != 0ull) {
        if (alive) {
            n++;
            if (n > max_steps) alive = false;
        }
        SegExit sr;
        sr.t1 = __builtin_inff();
        sr.k = kNone;
        if (alive) {
            sr = seg_scan(p.geo + (size_t)(nb >> 2) * 6u, cnt, head.x, head.y, head.z, Ox, Oy, Oz, dx, dy, dz);
            if constexpr (FILL) {
                if ((int64_t)entries < room) {
                    const int64_t e = base + (int64_t)entries;
                    p.out_cells[e] = cur;
                    p.t_enter[e] = t0;
                    p.t_exit[e] = sr.k == kNone ? __builtin_inff() : sr.t1;
                }
            }
            entries++;
            if (sr.k == kNone) alive = false;
        }
        const float dens = head.w;
        if (alive) {
            const Link link = p.link[nb + sr.k];
            cur = link.nbr;
            nb = link.first;
            cnt = link.count;
            head = p.cells[cur];
        }
        if (alive) {
            const float t1 = sr.t1;
            const bool segment = t1 > t0;
            // a segment through a cell of density exactly 0 changes nothing (alpha = 0): skipped, as forward_kernel does
            if (segment && dens != 0.0f) {
                const float dt = __builtin_fmaxf(t1 - t0, 0.0f);
                const float alpha = 1.0f - exp_(-dens * dt);
                T = T * (1.0f - alpha);
                if (!(T > thr)) alive = false;
            }
            t0 = segment ? t1 : t0;     // fmaxf(t0, t1): t0 is never NaN
        }
    }

    if constexpr (!FILL) {
        if (valid) {
            p.counts[ray] = entries;
            if (p.nint) p.nint[ray] = n;
        }
    }
}

static int launch_segments(bool fill, const char *what, const rf_trace_settings *settings, uint32_t num_points,
                           uint32_t adj_size, const void *workspace, uint32_t num_rays, const float *rays,
                           const uint32_t *start, SegParams p, void *stream) {
    g_err[0] = 0;
    if (!settings) return fail(RF_ERR_INVALID_ARGUMENT, "%s: settings null", what);
    if (num_rays == 0) return RF_OK;
    if (!rays || !start || (num_points && !workspace)) return fail(RF_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    // the tables the walk reads sit in front of everything that depends on the SH degree or the attribute type
    const FoamLayout L = foam_layout(num_points, adj_size, 0, 0);
    const char *ws = static_cast<const char *>(workspace);
    p.cells = reinterpret_cast<const float4 *>(ws + L.cells_off);
    p.geo = reinterpret_cast<const uint32_t *>(ws + L.geo_off);
    p.link = reinterpret_cast<const Link *>(ws + L.link_off);
    p.poff = reinterpret_cast<const uint32_t *>(ws + L.poff_off);
    p.settings = *settings;
    p.num_points = num_points;
    p.num_rays = num_rays;
    p.rays = rays;
    p.start = start;
    const dim3 grid((num_rays + (uint32_t)kSegBlock - 1u) / (uint32_t)kSegBlock), block(kSegBlock);
    if (fill)
        hipLaunchKernelGGL(segments_kernel<true>, grid, block, 0, static_cast<hipStream_t>(stream), p);
    else
        hipLaunchKernelGGL(segments_kernel<false>, grid, block, 0, static_cast<hipStream_t>(stream), p);
    return check_launch(what);
}

// The cell behind every ray's last face.  A ray that ends on the threshold or the step limit
// leaves its last entry with a finite t_exit, and the cell on the far side of that face is not in the list.  One lane
// per ray scans the last entry's cell again -- seg_scan over the same workspace, hence the winner the walk found -- and
// follows its link.  kNone where the ray has no entries or its last exit is infinite.
struct SegExitParams {
    const float4 *cells;
    const uint32_t *geo;
    const Link *link;
    const uint32_t *poff;
    uint32_t num_points, num_rays;
    const float *rays;
    const int64_t *offsets;
    const uint32_t *seg_cells;
    const float *t_exit;
    uint32_t *exit_cells;
};

__global__ __launch_bounds__(kSegBlock) void segments_exit_cells_kernel(SegExitParams p) {
    const uint32_t ray = blockIdx.x * (uint32_t)kSegBlock + threadIdx.x;
    if (ray >= p.num_rays) return;
    uint32_t out = kNone;
    const int64_t lo = p.offsets[ray], hi = p.offsets[ray + 1];
    if (hi > lo) {
        const uint32_t cur = p.seg_cells[hi - 1];
        if (p.t_exit[hi - 1] != __builtin_inff() && cur < p.num_points) {
            const float *rp = p.rays + (size_t)ray * 6;
            const float Ox = rp[0], Oy = rp[1], Oz = rp[2];
            float dx = rp[3], dy = rp[4], dz = rp[5];
            const float nrm = sqrtf(dot3(dx, dy, dz, dx, dy, dz));
            dx = dx / nrm;
            dy = dy / nrm;
            dz = dz / nrm;
            const uint32_t nb = p.poff[cur];
            const uint32_t cnt = p.poff[cur + 1] - nb;
            const float4 head = p.cells[cur];
            const SegExit sr = seg_scan(p.geo + (size_t)(nb >> 2) * 6u, cnt, head.x, head.y, head.z, Ox, Oy, Oz, dx, dy, dz);
            if (sr.k != kNone) out = p.link[nb + sr.k].nbr;
        }
    }
    p.exit_cells[ray] = out;
}

}  // namespace rf

using namespace rf;

extern "C" {

int rf_trace_segments_count(const rf_trace_settings *settings, uint32_t num_points, uint32_t point_adjacency_size,
                            const void *workspace, uint32_t num_rays, const float *rays,
                            const uint32_t *start_point_index, uint32_t *counts, uint32_t *num_intersections,
                            void *stream) {
    if (num_rays && !counts) return fail(RF_ERR_INVALID_ARGUMENT, "%s: null pointer", "rf_trace_segments_count");
    SegParams p{};
    p.counts = counts;
    p.nint = num_intersections;
    return launch_segments(false, "rf_trace_segments_count", settings, num_points, point_adjacency_size, workspace,
                           num_rays, rays, start_point_index, p, stream);
}

int rf_trace_segments_fill(const rf_trace_settings *settings, uint32_t num_points, uint32_t point_adjacency_size,
                           const void *workspace, uint32_t num_rays, const float *rays,
                           const uint32_t *start_point_index, const int64_t *offsets, uint32_t *cells, float *t_enter,
                           float *t_exit, void *stream) {
    // (cells / t_enter / t_exit may be null when the offsets say that no ray has an entry: nothing is written then)
    if (num_rays && !offsets) return fail(RF_ERR_INVALID_ARGUMENT, "%s: null pointer", "rf_trace_segments_fill");
    SegParams p{};
    p.offsets = offsets;
    p.out_cells = cells;
    p.t_enter = t_enter;
    p.t_exit = t_exit;
    return launch_segments(true, "rf_trace_segments_fill", settings, num_points, point_adjacency_size, workspace,
                           num_rays, rays, start_point_index, p, stream);
}

int rf_trace_segments_exit_cells(uint32_t num_points, uint32_t point_adjacency_size, const void *workspace,
                                 uint32_t num_rays, const float *rays, const int64_t *offsets, const uint32_t *cells,
                                 const float *t_exit, uint32_t *exit_cells, void *stream) {
    const char *what = "rf_trace_segments_exit_cells";
    g_err[0] = 0;
    if (num_rays == 0) return RF_OK;
    // (cells / t_exit may be null when the offsets say that no ray has an entry: nothing of them is read then)
    if (!rays || !offsets || !exit_cells || (num_points && !workspace))
        return fail(RF_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    const FoamLayout L = foam_layout(num_points, point_adjacency_size, 0, 0);
    const char *ws = static_cast<const char *>(workspace);
    SegExitParams p{};
    p.cells = reinterpret_cast<const float4 *>(ws + L.cells_off);
    p.geo = reinterpret_cast<const uint32_t *>(ws + L.geo_off);
    p.link = reinterpret_cast<const Link *>(ws + L.link_off);
    p.poff = reinterpret_cast<const uint32_t *>(ws + L.poff_off);
    p.num_points = num_points;
    p.num_rays = num_rays;
    p.rays = rays;
    p.offsets = offsets;
    p.seg_cells = cells;
    p.t_exit = t_exit;
    p.exit_cells = exit_cells;
    const dim3 grid((num_rays + (uint32_t)kSegBlock - 1u) / (uint32_t)kSegBlock), block(kSegBlock);
    hipLaunchKernelGGL(segments_exit_cells_kernel, grid, block, 0, static_cast<hipStream_t>(stream), p);
    return check_launch(what);
}

}  // extern "C"
