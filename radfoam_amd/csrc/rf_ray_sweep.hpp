// rf_ray_sweep.hpp -- the wave scheme of the kernels that go over an exported walk ray by ray (rf_composite.hip,
// rf_distortion.hip, rf_quantiles.hip, rf_entry_weights.hip) with what an entry contributes to
// them, and the lane exchange and the segmented scan for those without rays (rf_segments_rays_grad.hip, the cell sweeps).
//
// ONE WAVE OWNS kRays CONSECUTIVE RAYS and sweeps their contiguous range of entries 64 at a time, one lane per entry,
// from the 64-aligned entry at or below the range's first: every [S] array is read coalesced.  No ray is shared between
// waves, so nothing is accumulated with atomics and no output is zeroed first: every element is written once and the
// result is the same bits from call to call.  (rf_segments_rays_grad.hip deals entries to waves evenly instead and
// finishes a ray with atomics.)  The price is load imbalance when the rays' entry counts differ wildly.
//
// The wave keeps its kRays + 1 offsets in its first lanes (clamped to 0 .. S and made non-decreasing, so that nothing
// below can index outside the arrays whatever the list holds).  In a step a lane finds its ray by counting the offsets
// at or below its entry (they are wave-uniform: scalar reads of those lanes), and its run's first lane from
// max(offsets[ray], the step's first entry).  The sums over a ray's earlier entries are an INCLUSIVE SEGMENTED SCAN IN
// DOUBLE over the wave (six steps of distance 1 .. 32, ds_bpermute on the two halves of each double); a ray that
// continues past the step hands its running sums on in wave-uniform registers (carry).  A sum over a whole ray is a
// segmented reduction by the same scan: the last lane of a ray's run in the step holds the run's sum, adds what the ray
// carried in, and when the ray ends there the sum is complete.
//
// NO LANE RETURNS before the last cross-lane operation of its wave (a wave without rays returns whole, before the
// first).  Lanes outside the wave's range of entries stay, as runs of their own holding zeros; loads and stores are
// predicated.  No LDS.
//
// Everything here is inlined into the kernels that use it.  scripts/isa_same.py tells whether an edit changed their code.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace rf {

// 64-bit values across the lanes of a wave, and sums of doubles over runs of lanes
struct WaveLanes {
    // the value lane `src` (0 .. 63) holds, every lane of the wave taking part
    static __device__ __forceinline__ uint64_t bits_from_lane(uint64_t bits, int src) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)(uint32_t)bits);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)(uint32_t)(bits >> 32));
        return ((uint64_t)hi << 32) | (uint64_t)lo;
    }
    static __device__ __forceinline__ double from_lane(double x, int src) {
        return __builtin_bit_cast(double, bits_from_lane(__builtin_bit_cast(uint64_t, x), src));
    }
    static __device__ __forceinline__ int64_t from_lane(int64_t x, int src) {
        return (int64_t)bits_from_lane((uint64_t)x, src);
    }

    // the value of a lane known at compile time, as a scalar
    static __device__ __forceinline__ int64_t read_lane(int64_t x, int lane) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)x, lane);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)x >> 32), lane);
        return (int64_t)(((uint64_t)hi << 32) | (uint64_t)lo);
    }
    // the value of the first lane, as a scalar
    static __device__ __forceinline__ int64_t uniform(int64_t x) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uint64_t)x);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)x >> 32));
        return (int64_t)(((uint64_t)hi << 32) | (uint64_t)lo);
    }

    // inclusive segmented scan over the wave (begin: the first lane of the lane's run): after the step of distance s a
    // lane holds the sum over max(begin, lane - 2s + 1) .. lane.  The source index wraps below lane 0; what comes from
    // there is not added.
    template <int N>
    static __device__ __forceinline__ void scan(double (&v)[N], int lane, int begin) {
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int src = (lane - s) & 63;
            double u[N];
#pragma unroll
            for (int n = 0; n < N; ++n) u[n] = from_lane(v[n], src);
            if (lane - s >= begin) {
#pragma unroll
                for (int n = 0; n < N; ++n) v[n] = v[n] + u[n];
            }
        }
    }
};

// kRays rays per wave, kWaves waves per block: both fixed where a kernel file names its sweep
template <int kRays, int kWaves>
struct RaySweep : WaveLanes {
    static_assert(kRays >= 1 && kRays <= 63, "a wave keeps kRays + 1 offsets in its lanes");

    // blocks of kWaves waves for num_rays rays (host)
    static int64_t blocks(uint32_t num_rays) {
        const int64_t waves = ((int64_t)num_rays + kRays - 1) / kRays;
        return (waves + kWaves - 1) / kWaves;
    }

    // ---- the rays of a wave ----
    struct Wave {
        int lane;
        int64_t r0;        // its first ray
        int nrays;         // 1 .. kRays
        int64_t off;       // lane i: offsets[r0 + min(i, nrays)], clamped to 0 .. S, non-decreasing over the lanes
        int64_t lo, hi;    // its entries: off of lane 0 and of lane nrays

        // false for a wave without rays: the whole wave leaves, before any cross-lane operation
        __device__ __forceinline__ bool init(uint32_t num_rays, int64_t total, const int64_t *offsets) {
            lane = (int)(threadIdx.x & 63u);
            const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
            r0 = ((int64_t)blockIdx.x * kWaves + wave_in_block) * kRays;
            if (r0 >= (int64_t)num_rays) return false;
            const int64_t left = (int64_t)num_rays - r0;
            nrays = left < kRays ? (int)left : kRays;
            int64_t o = offsets[r0 + (lane < nrays ? lane : nrays)];
            o = o < 0 ? 0 : (o > total ? total : o);
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {             // running maximum: non-decreasing whatever the list holds
                const int64_t below = from_lane(o, (lane - s) & 63);
                if (lane >= s && below > o) o = below;
            }
            off = o;
            lo = uniform(o);
            hi = read_lane(o, 63);                         // the lanes from nrays on all hold the range's end
            return true;
        }

        // the first entry of the first step: the 64-aligned entry at or below lo
        __device__ __forceinline__ int64_t first_base() const { return lo & ~(int64_t)63; }
    };

    // ---- a lane's place in one step of 64 entries ----
    struct Step {
        int64_t k;         // its entry
        bool valid;        // within the wave's range
        int ray;           // its ray, counted from r0 (0 where not valid)
        int begin;         // first lane of its run in this step (itself where not valid)
        bool cont;         // its ray began before this step: the carried sums belong to it
        bool ends;         // its ray ends within this step
        bool last;         // it is the last lane of its run in this step
    };

    static __device__ __forceinline__ Step step(const Wave &w, int64_t base) {
        Step s;
        s.k = base + w.lane;
        s.valid = s.k >= w.lo && s.k < w.hi;
        int ray = 0;
#pragma unroll
        for (int i = 1; i <= kRays; ++i) ray += s.k >= read_lane(w.off, i) ? 1 : 0;
        s.ray = s.valid ? ray : 0;                         // valid: off[ray] <= k < off[ray + 1], ray < nrays
        const int64_t seg_lo = from_lane(w.off, s.ray);
        const int64_t seg_hi = from_lane(w.off, s.ray + 1);
        const int64_t step_end = base + 64;
        const int end = (int)((seg_hi < step_end ? seg_hi : step_end) - 1 - base);
        s.begin = s.valid ? (int)((seg_lo > base ? seg_lo : base) - base) : w.lane;
        s.cont = s.valid && seg_lo < base;
        s.ends = s.valid && seg_hi <= step_end;
        s.last = s.valid && w.lane == end;
        return s;
    }

    // what the ray that runs past the step's last lane hands on: every lane gets it (0 when no ray does)
    static __device__ __forceinline__ double carry(const Step &s, double sum) {
        return from_lane(s.last && !s.ends ? sum : 0.0, 63);
    }

    // the sum of v over the lane's ray up to and including its entry: the scan over its run in this step, and what the
    // ray carried in.  For helpers such as quant_sums and dist_weights only: called from a kernel's own body it changes
    // the kernel's code, so the kernels spell these three lines out, array, scan and cont, as they stand
    // here.
    static __device__ __forceinline__ double running(const Wave &w, const Step &s, double v, double carried) {
        double a[1] = {v};
        scan(a, w.lane, s.begin);
        return s.cont ? a[0] + carried : a[0];
    }
};

// ---- what an entry of the walk contributes: zeros where the lane is not valid.  THE ONE STATEMENT, for every
// operator over the walk, of
//     dt = 0 where t_exit is infinite, else max(t_exit - t_enter, 0),      x = sigma dt ----
struct SweepEntry {
    float t0, t1;      // t_enter and t_exit as read
    double dt, sigma, x;
    bool infinite;     // t_exit is infinite: every gradient of the entry is an exact zero
    bool moves;        // t_exit is finite and >= t_enter: the times get a gradient (torch's clamp_min convention)
};

// entry k, for a lane that may read it
__device__ __forceinline__ SweepEntry sweep_entry_at(int64_t k, const float *t_enter, const float *t_exit,
                                                     const float *sigma) {
    SweepEntry e;
    e.t0 = t_enter[k];
    e.t1 = t_exit[k];
    const double d = (double)e.t1 - (double)e.t0;
    e.infinite = __builtin_isinf(e.t1);
    e.moves = !e.infinite && e.t1 >= e.t0;
    e.dt = e.infinite ? 0.0 : (d < 0.0 ? 0.0 : d);
    e.sigma = (double)sigma[k];
    e.x = e.sigma * e.dt;
    return e;
}

// the entry of a step's lane
template <class Step>
__device__ __forceinline__ SweepEntry sweep_entry(const Step &s, const float *t_enter, const float *t_exit,
                                                  const float *sigma) {
    SweepEntry e{};
    if (s.valid) e = sweep_entry_at(s.k, t_enter, t_exit, sigma);
    return e;
}

// T = exp(-(the ray's earlier x)), alpha = 1 - exp(-x) and w = T alpha of an entry, from the ray's x up to and
// including it
struct SweepWeight {
    double through, alpha, weight;
};

__device__ __forceinline__ SweepWeight sweep_weight(double sum_x, double x) {
    SweepWeight o;
    o.through = ::exp(-(sum_x - x));                       // exp(-0) = 1 at a ray's first entry
    o.alpha = -::expm1(-x);
    o.weight = o.through * o.alpha;
    return o;
}

// dL/dx of an entry handed on to sigma and to t_exit; t_enter gets the negative of the latter.  Entry: SweepEntry, or
// an entry that states dt, sigma, infinite and moves as SweepEntry does.
struct SweepGrad {
    double sigma, exit;
};

template <class Entry>
__device__ __forceinline__ SweepGrad sweep_grad(const Entry &e, double dx) {
    return SweepGrad{e.infinite ? 0.0 : dx * e.dt, e.moves ? dx * e.sigma : 0.0};
}

}  // namespace rf
