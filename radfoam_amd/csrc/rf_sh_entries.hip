// rf_sh_entries.hip -- the tracer's colour per entry of an exported walk, and its gradients
// (include/radfoam_hip_sh_entries.h).
//
//     dhat = d / |d|,      rgb[e][c] = max(0.5 + sum_k Y_k(dhat_ray(e)) coeffs[cell(e)][3 k + c], 0)
//
// FORWARD: one lane per entry in entry order.  The colour is the tracer's bit for bit: the direction is normalised as
// the forward kernel of rf_kernels.hip normalises it (sqrtf of dot3, three IEEE divides), the basis is rf_math.hpp's
// sh_basis<DEG>, the chain is cell_rgb's -- acc[i % 3] = fma_(sh[i / 3], row[i], acc[i % 3]) from 0.5 in ascending i,
// then fmaxf(., 0) -- and the row is loaded as cell_rgb loads it, in vectors declared 4-byte aligned.  (cell_rgb reads
// whole vectors because the density follows the coefficients in the tracer's row; here the table may end with the
// row, so what is left of 3 K after the whole vectors is read element by element.)
//
// BACKWARD TO THE COEFFICIENTS: the sum per cell of rf_cell_reduce.hip with the row formed in registers: at sorted
// position k with entry e and ray r the row is Y_k'(dhat_r) (rgb[e][c] > 0 ? g[e][c] : 0), each product rounded to fp32
// (what the reference adds per entry), summed in double over the cell's run, rounded once.  The scheme is
// rf_cell_sweep.hpp's, which also holds what the two users state once: the chunk, the workspace, the checks, the launch
// sizes, cell_at and came_in.  The bodies of the two kernels below follow reduce_entries_kernel and
// reduce_entries_boundaries_kernel of rf_cell_reduce.hip line by line, but for where a lane's row and the first channel
// come from: an edit to either pair belongs in the other (DESIGN 4.16 lists the shared spellings that changed the
// kernels' code).  Channels go in groups of kShGroup whole basis functions, one sweep per group.
//
// BACKWARD TO THE DIRECTIONS: one lane per entry in entry order under rf_ray_sweep.hpp's RaySweep.  Per entry
// q_e = sum_c m g[e][c] sum_k grad Y_k(dhat) coeffs[cell][3 k + c], in double; the three components are summed per ray
// by the segmented scan with carries across the wave's steps; the lane that holds a ray's complete sum applies the
// Jacobian of the normalisation, (q - dhat (dhat . q)) / |d|, and stores the ray's row.
//
// No atomics, no LDS; every output element is written once; no lane returns before the last cross-lane operation of its
// wave.  Every index read from memory is range-checked where it is read.
//
// Compiled like the tracer (-ffp-contract=off; every fused multiply-add spelled out).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/radfoam_hip_sh_entries.h"
#include "rf_host.hpp"
#include "rf_cell_sweep.hpp"
#include "rf_math.hpp"

#ifndef RF_SH_ENTRIES_GROUP
#define RF_SH_ENTRIES_GROUP 8
#endif

namespace rf {

constexpr int kShBlock = 256;
constexpr int kShWaves = kShBlock / 64;
constexpr int kShGroup = RF_SH_ENTRIES_GROUP;              // basis functions per sweep: 8 of 1, 2, 4, 8 timed, DESIGN 4.16
constexpr int kShRays = 8;                                 // rays per wave of the direction gradient
static_assert(kShGroup == 1 || kShGroup == 2 || kShGroup == 4 || kShGroup == 8, "3, 6, 12 or 24 channels per sweep");
using ShSweep = RaySweep<kShRays, kShWaves>;

struct __attribute__((packed, aligned(4))) ShFloat4U {     // four floats at a 4-byte aligned address
    float x, y, z, w;
};

// a row of NC coefficients: whole vectors as cell_rgb loads them, then what is left
template <int NC>
__device__ __forceinline__ void load_row(const float *row, float (&c)[NC]) {
    constexpr int NV = NC / 4;
    const ShFloat4U *vec = reinterpret_cast<const ShFloat4U *>(row);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const ShFloat4U w = vec[i];
        c[4 * i + 0] = w.x;
        c[4 * i + 1] = w.y;
        c[4 * i + 2] = w.z;
        c[4 * i + 3] = w.w;
    }
#pragma unroll
    for (int i = 4 * NV; i < NC; ++i) c[i] = row[i];
}

// the basis of a ray as the tracer's forward kernel forms it from an unnormalised direction
template <int DEG>
__device__ __forceinline__ void ray_basis(const float *d, float (&sh)[sh_dim(DEG)]) {
    float dx = d[0], dy = d[1], dz = d[2];
    const float nrm = sqrtf(dot3(dx, dy, dz, dx, dy, dz));
    dx = dx / nrm;
    dy = dy / nrm;
    dz = dz / nrm;
    sh_basis<DEG>(dx, dy, dz, sh);
}

// ---------------------------------------------------------------------------------------------------------------
// forward

struct ShForwardParams {
    int64_t num_cells, total;
    uint32_t num_rays, pitch;
    const int64_t *cells;        // [S]
    const int32_t *entry_rays;   // [S]
    const float *coeffs;         // [N] rows of 3 K, pitch floats apart
    const float *directions;     // [R][3]
    float *rgb;                  // [S][3]
};

template <int DEG>
__global__ __launch_bounds__(kShBlock) void sh_entries_forward_kernel(ShForwardParams p) {
    constexpr int NC = 3 * sh_dim(DEG);
    const int64_t e = (int64_t)blockIdx.x * kShBlock + threadIdx.x;
    if (e >= p.total) return;
    const int64_t cell = p.cells[e];
    const int32_t ray = p.entry_rays[e];
    float r = 0.0f, g = 0.0f, b = 0.0f;
    if (cell >= 0 && cell < p.num_cells && ray >= 0 && (uint32_t)ray < p.num_rays) {
        float sh[sh_dim(DEG)];
        ray_basis<DEG>(p.directions + (size_t)ray * 3, sh);
        float c[NC];
        load_row<NC>(p.coeffs + (size_t)cell * p.pitch, c);
        float acc[3] = {0.5f, 0.5f, 0.5f};
#pragma unroll
        for (int i = 0; i < NC; ++i) acc[i % 3] = fma_(sh[i / 3], c[i], acc[i % 3]);
        r = __builtin_fmaxf(acc[0], 0.0f);
        g = __builtin_fmaxf(acc[1], 0.0f);
        b = __builtin_fmaxf(acc[2], 0.0f);
    }
    float *out = p.rgb + (size_t)e * 3;
    out[0] = r;
    out[1] = g;
    out[2] = b;
}

// ---------------------------------------------------------------------------------------------------------------
// backward to the coefficients: rf_cell_sweep.hpp's scheme; the bodies follow rf_cell_reduce.hip's (see the head)

struct ShCoeffParams {
    int64_t num_cells, total, num_chunks;
    uint32_t num_rays;
    uint32_t num_channels;       // 3 K
    const int64_t *sorted_cells, *entries;   // [S]
    const int32_t *entry_rays;   // [S]
    const float *directions;     // [R][3]
    const float *rgb, *grad_rgb; // [S][3]
    float *out;                  // [N][3 K]
    double *partial;             // [num_chunks][2][3 K]
};

// this launch sums basis functions FIRST .. FIRST + NB - 1: channels 3 FIRST .. 3 (FIRST + NB) - 1
template <int DEG, int FIRST, int NB>
__global__ __launch_bounds__(kCellBlock) void sh_entries_coeffs_kernel(ShCoeffParams p) {
    constexpr int NCH = 3 * NB;
    const int lane = (int)(threadIdx.x & 63u);
    const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t chunk = (int64_t)blockIdx.x * kCellWaves + wave_in_block;
    if (chunk >= p.num_chunks) return;
    const int64_t c0 = chunk * kCellChunk;
    const int64_t c1 = c0 + kCellChunk < p.total ? c0 + kCellChunk : p.total;
    const int64_t cell_before = cell_at(p, c0 - 1);                   // wave-uniform
    const uint64_t upto_me = ~(uint64_t)0 >> (63 - lane);
    const size_t C = p.num_channels;

    double carry[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) carry[c] = 0.0;
    bool carry_first = true;     // the run that reaches a step's first lane began at the chunk's first position
    for (int64_t base = c0; base < c1; base += 64) {
        const int64_t k = base + lane;
        const bool in = k < c1;
        const int64_t cell = in ? cell_at(p, k) : -1;
        const int64_t next = in ? cell_at(p, k + 1) : -1;
        const bool chunk_end = k + 1 == c1;
        const bool same_next = cell >= 0 && next == cell;
        const bool run_end = !same_next || chunk_end;                    // the last lane of its run within the chunk
        const uint64_t ends = __builtin_amdgcn_ballot_w64(run_end || lane == 63);
        const int begin = 63 - __builtin_clzll(((ends << 1) | 1u) & upto_me);   // the first lane of its run in this step
        const bool first_run = begin == 0 && carry_first;

        double v[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) v[c] = 0.0;
        if (cell >= 0) {
            const int64_t e = p.entries[k];
            if (e >= 0 && e < p.total) {
                const int32_t ray = p.entry_rays[e];
                if (ray >= 0 && (uint32_t)ray < p.num_rays) {
                    float sh[sh_dim(DEG)];
                    ray_basis<DEG>(p.directions + (size_t)ray * 3, sh);
                    const float *colour = p.rgb + (size_t)e * 3;
                    const float *grad = p.grad_rgb + (size_t)e * 3;
                    float mg[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) mg[c] = colour[c] > 0.0f ? grad[c] : 0.0f;
#pragma unroll
                    for (int c = 0; c < NCH; ++c) v[c] = (double)(sh[FIRST + c / 3] * mg[c % 3]);
                }
            }
        }
        WaveLanes::scan(v, lane, begin);
        if (begin == 0) {                                                // what the run carried in: zeros for a new one
#pragma unroll
            for (int c = 0; c < NCH; ++c) v[c] = v[c] + carry[c];
        }

        if (cell >= 0 && run_end) {
            const bool from_before = first_run && cell_before == cell;
            const bool goes_on = chunk_end && same_next;
            if (from_before || goes_on) {
                double *row = p.partial + ((size_t)chunk * 2 + (from_before ? 0 : 1)) * C + 3 * FIRST;
#pragma unroll
                for (int c = 0; c < NCH; ++c) row[c] = v[c];
            } else {                                                     // the cell's whole list: round once
                float *row = p.out + (size_t)cell * C + 3 * FIRST;
#pragma unroll
                for (int c = 0; c < NCH; ++c) row[c] = (float)v[c];
            }
        }
        const bool onward = !run_end;                                    // read at lane 63: its run meets the next step
#pragma unroll
        for (int c = 0; c < NCH; ++c) carry[c] = WaveLanes::from_lane(onward ? v[c] : 0.0, 63);
        carry_first = (__builtin_amdgcn_ballot_w64(onward && first_run) >> 63) != 0;
    }
}

__global__ __launch_bounds__(kCellBlock) void sh_entries_coeffs_boundaries_kernel(ShCoeffParams p) {
    const int lane = (int)(threadIdx.x & 63u);
    const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t boundaries = p.num_chunks - 1;                         // boundary b lies between chunks b and b + 1
    const int64_t b0 = ((int64_t)blockIdx.x * kCellWaves + wave_in_block) * 64;
    if (b0 >= boundaries) return;
    const int64_t b = b0 + lane;
    const size_t C = p.num_channels;

    // the list that crosses boundary b, if one does, and whether it begins in chunk b: then this lane answers for it
    int64_t cell = -1;
    bool longer = false;
    if (b < boundaries) {
        const int64_t left = cell_at(p, (b + 1) * kCellChunk - 1);
        if (left >= 0 && cell_at(p, (b + 1) * kCellChunk) == left && !came_in(p, b, left)) {
            cell = left;
            longer = came_in(p, b + 2, left);
            if (!longer) {                                               // two chunks: this lane alone
                const double *first = p.partial + ((size_t)b * 2 + 1) * C;
                const double *second = p.partial + ((size_t)b + 1) * 2 * C;
                float *row = p.out + (size_t)cell * C;
                for (size_t c = 0; c < C; ++c) row[c] = (float)(first[c] + second[c]);
            }
        }
    }

    // three chunks and more: the wave, 64 chunks a step, added one after the other in chunk order
    uint64_t todo = __builtin_amdgcn_ballot_w64(longer);
    while (todo != 0) {                                                  // wave-uniform
        const int owner = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int64_t first_chunk = b0 + owner;
        const int64_t its_cell = WaveLanes::uniform(WaveLanes::from_lane(cell, owner));
        for (size_t c = 0; c < C; ++c) {
            double sum = p.partial[((size_t)first_chunk * 2 + 1) * C + c];
            for (int64_t j0 = first_chunk + 1;; j0 += 64) {
                const int64_t j = j0 + lane;
                const uint64_t others = ~__builtin_amdgcn_ballot_w64(came_in(p, j, its_cell));
                const int count = others != 0 ? __builtin_ctzll(others) : 64;    // the chunks in front of the first other
                const double mine = lane < count ? p.partial[(size_t)j * 2 * C + c] : 0.0;
                for (int i = 0; i < count; ++i)
                    sum = sum + __builtin_bit_cast(double, WaveLanes::read_lane(__builtin_bit_cast(int64_t, mine), i));
                if (count < 64) break;
            }
            if (lane == 0) p.out[(size_t)its_cell * C + c] = (float)sum;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// backward to the directions

// q = sum_k a[k] grad Y_k at the unit vector (x, y, z): the polynomials of sh_basis as written, differentiated
template <int DEG>
__device__ __forceinline__ void sh_basis_grad_dot(double x, double y, double z, const double (&a)[sh_dim(DEG)],
                                                  double &qx, double &qy, double &qz) {
    constexpr double C1 = 0.4886025119029199;
    qx = 0.0;
    qy = 0.0;
    qz = 0.0;
    if constexpr (DEG > 0) {
        qy += -C1 * a[1];
        qz += C1 * a[2];
        qx += -C1 * a[3];
    }
    if constexpr (DEG > 1) {
        constexpr double A = 1.0925484305920792, B = 0.31539156525252005, C = 0.5462742152960396;
        qx += a[4] * (A * y);
        qy += a[4] * (A * x);
        qy += a[5] * (-A * z);
        qz += a[5] * (-A * y);
        qx += a[6] * (-2.0 * B * x);
        qy += a[6] * (-2.0 * B * y);
        qz += a[6] * (4.0 * B * z);
        qx += a[7] * (-A * z);
        qz += a[7] * (-A * x);
        qx += a[8] * (2.0 * C * x);
        qy += a[8] * (-2.0 * C * y);
    }
    if constexpr (DEG > 2) {
        constexpr double E = 0.5900435899266435, F = 2.890611442640554, H = 0.4570457994644658;
        constexpr double P = 0.3731763325901154, S = 1.445305721320277;
        const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        qx += a[9] * (-6.0 * E * xy);
        qy += a[9] * (-3.0 * E * (xx - yy));
        qx += a[10] * (F * yz);
        qy += a[10] * (F * xz);
        qz += a[10] * (F * xy);
        qx += a[11] * (2.0 * H * xy);
        qy += a[11] * (-H * (4.0 * zz - xx - 3.0 * yy));
        qz += a[11] * (-8.0 * H * yz);
        qx += a[12] * (-6.0 * P * xz);
        qy += a[12] * (-6.0 * P * yz);
        qz += a[12] * (P * (6.0 * zz - 3.0 * xx - 3.0 * yy));
        qx += a[13] * (-H * (4.0 * zz - 3.0 * xx - yy));
        qy += a[13] * (2.0 * H * xy);
        qz += a[13] * (-8.0 * H * xz);
        qx += a[14] * (2.0 * S * xz);
        qy += a[14] * (-2.0 * S * yz);
        qz += a[14] * (S * (xx - yy));
        qx += a[15] * (-3.0 * E * (xx - yy));
        qy += a[15] * (6.0 * E * xy);
    }
}

struct ShDirParams {
    int64_t num_cells, total;
    uint32_t num_rays, pitch;
    const int64_t *offsets;      // [R + 1]
    const int64_t *cells;        // [S]
    const float *coeffs;
    const float *directions;     // [R][3]
    const float *rgb, *grad_rgb; // [S][3]
    float *out;                  // [R][3]
};

template <int DEG>
__global__ __launch_bounds__(kShBlock) void sh_entries_directions_kernel(ShDirParams p) {
    constexpr int K = sh_dim(DEG);
    constexpr int NC = 3 * K;
    ShSweep::Wave w;
    if (!w.init(p.num_rays, p.total, p.offsets)) return;

    // rays without entries: lane i answers for ray r0 + i
    {
        const int64_t next = ShSweep::from_lane(w.off, (w.lane + 1) & 63);
        if (w.lane < w.nrays && next == w.off) {
            float *row = p.out + (size_t)(w.r0 + w.lane) * 3;
            row[0] = 0.0f;
            row[1] = 0.0f;
            row[2] = 0.0f;
        }
    }

    double carry[3] = {0.0, 0.0, 0.0};
    for (int64_t base = w.first_base(); base < w.hi; base += 64) {
        const ShSweep::Step s = ShSweep::step(w, base);
        double v[3] = {0.0, 0.0, 0.0};
        double x = 0.0, y = 0.0, z = 1.0, nrm = 1.0;
        if (s.valid) {
            const float *d = p.directions + (size_t)(w.r0 + s.ray) * 3;
            const double dx = (double)d[0], dy = (double)d[1], dz = (double)d[2];
            nrm = ::sqrt(dx * dx + dy * dy + dz * dz);
            x = dx / nrm;
            y = dy / nrm;
            z = dz / nrm;
            const int64_t cell = p.cells[s.k];
            if (cell >= 0 && cell < p.num_cells) {
                const float *colour = p.rgb + (size_t)s.k * 3;
                const float *grad = p.grad_rgb + (size_t)s.k * 3;
                double mg[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) mg[c] = colour[c] > 0.0f ? (double)grad[c] : 0.0;
                float row[NC];
                load_row<NC>(p.coeffs + (size_t)cell * p.pitch, row);
                double a[K];
#pragma unroll
                for (int k = 0; k < K; ++k)
                    a[k] = __builtin_fma(mg[0], (double)row[3 * k],
                                         __builtin_fma(mg[1], (double)row[3 * k + 1], mg[2] * (double)row[3 * k + 2]));
                sh_basis_grad_dot<DEG>(x, y, z, a, v[0], v[1], v[2]);
            }
        }
        ShSweep::scan(v, w.lane, s.begin);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = s.cont ? v[c] + carry[c] : v[c];

        if (s.last && s.ends) {                                          // the ray's sums are complete
            const double along = x * v[0] + y * v[1] + z * v[2];
            float *row = p.out + (size_t)(w.r0 + s.ray) * 3;
            row[0] = (float)((v[0] - x * along) / nrm);
            row[1] = (float)((v[1] - y * along) / nrm);
            row[2] = (float)((v[2] - z * along) / nrm);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) carry[c] = ShSweep::carry(s, v[c]);
    }
}

}  // namespace rf

using namespace rf;

namespace {

template <int DEG>
void sh_launch_forward(const ShForwardParams &p, hipStream_t stream) {
    const int64_t blocks = (p.total + kShBlock - 1) / kShBlock;
    hipLaunchKernelGGL(sh_entries_forward_kernel<DEG>, dim3((uint32_t)blocks), dim3(kShBlock), 0, stream, p);
}

// one sweep per group of kShGroup basis functions, the last group what is left
template <int DEG, int FIRST>
void sh_launch_coeffs(const ShCoeffParams &p, hipStream_t stream) {
    if constexpr (FIRST < sh_dim(DEG)) {
        constexpr int NB = sh_dim(DEG) - FIRST < kShGroup ? sh_dim(DEG) - FIRST : kShGroup;
        hipLaunchKernelGGL((sh_entries_coeffs_kernel<DEG, FIRST, NB>), dim3((uint32_t)cell_sweep_blocks(p.num_chunks)),
                           dim3(kCellBlock), 0, stream, p);
        sh_launch_coeffs<DEG, FIRST + NB>(p, stream);
    }
}

template <int DEG>
void sh_launch_directions(const ShDirParams &p, hipStream_t stream) {
    hipLaunchKernelGGL(sh_entries_directions_kernel<DEG>, dim3((uint32_t)ShSweep::blocks(p.num_rays)),
                       dim3(kShBlock), 0, stream, p);
}

}  // namespace

extern "C" {

uint32_t rf_sh_entries_group(void) { return (uint32_t)kShGroup; }

int rf_sh_entries_forward(uint32_t degree, int64_t num_cells, int64_t num_entries, uint32_t num_rays,
                          const int64_t *cells, const int32_t *entry_rays, const float *coeffs, uint32_t coeff_pitch,
                          const float *directions, float *rgb, void *stream) {
    const char *what = "rf_sh_entries_forward";
    g_err[0] = 0;
    if (degree > 3) return fail(RF_ERR_INVALID_ARGUMENT, "%s: the degree must be 0 .. 3", what);
    if (num_entries < 0) return fail(RF_ERR_INVALID_ARGUMENT, "%s: negative entry count", what);
    if (num_cells < 0) return fail(RF_ERR_INVALID_ARGUMENT, "%s: negative cell count", what);
    if (coeff_pitch < 3 * (degree + 1) * (degree + 1))
        return fail(RF_ERR_INVALID_ARGUMENT, "%s: the pitch is below the row's 3 K coefficients", what);
    if (num_entries == 0) return RF_OK;
    if (!rgb || !cells || !entry_rays) return fail(RF_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    if ((num_cells > 0 && !coeffs) || (num_rays > 0 && !directions))
        return fail(RF_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    if ((num_entries + kShBlock - 1) / kShBlock >= ((int64_t)1 << 31))
        return fail(RF_ERR_INVALID_ARGUMENT, "%s: too many entries for one launch", what);
    ShForwardParams p{};
    p.num_cells = num_cells;
    p.total = num_entries;
    p.num_rays = num_rays;
    p.pitch = coeff_pitch;
    p.cells = cells;
    p.entry_rays = entry_rays;
    p.coeffs = coeffs;
    p.directions = directions;
    p.rgb = rgb;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (degree) {
        case 0: sh_launch_forward<0>(p, s); break;
        case 1: sh_launch_forward<1>(p, s); break;
        case 2: sh_launch_forward<2>(p, s); break;
        default: sh_launch_forward<3>(p, s); break;
    }
    return check_launch(what);
}

size_t rf_sh_entries_workspace_bytes(int64_t num_entries, uint32_t degree) {
    if (degree > 3) return 0;
    return cell_workspace_bytes(num_entries, 3 * (degree + 1) * (degree + 1));
}

int rf_sh_entries_backward_coeffs(uint32_t degree, int64_t num_cells, int64_t num_entries, uint32_t num_rays,
                                  const int64_t *sorted_cells, const int64_t *entries, const int32_t *entry_rays,
                                  const float *directions, const float *rgb, const float *grad_rgb, float *grad_coeffs,
                                  void *workspace, size_t workspace_bytes, void *stream) {
    const char *what = "rf_sh_entries_backward_coeffs";
    g_err[0] = 0;
    if (degree > 3) return fail(RF_ERR_INVALID_ARGUMENT, "%s: the degree must be 0 .. 3", what);
    if (num_entries < 0) return fail(RF_ERR_INVALID_ARGUMENT, "%s: negative entry count", what);
    if (num_cells < 0) return fail(RF_ERR_INVALID_ARGUMENT, "%s: negative cell count", what);
    if (num_cells == 0) return RF_OK;
    if (!grad_coeffs) return fail(RF_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    const uint32_t channels = 3 * (degree + 1) * (degree + 1);
    if (num_entries > 0 && num_rays > 0) {
        if (!sorted_cells || !entries || !entry_rays || !directions || !rgb || !grad_rgb)
            return fail(RF_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
        const int rc = cell_check(what, num_entries, channels, workspace, workspace_bytes);
        if (rc != RF_OK) return rc;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(grad_coeffs, 0, (size_t)num_cells * channels * sizeof(float), s) != hipSuccess)
        return check_launch(what);
    if (num_entries == 0 || num_rays == 0) return RF_OK;
    ShCoeffParams p{};
    p.num_cells = num_cells;
    p.total = num_entries;
    p.num_chunks = cell_chunks(num_entries);
    p.num_rays = num_rays;
    p.num_channels = channels;
    p.sorted_cells = sorted_cells;
    p.entries = entries;
    p.entry_rays = entry_rays;
    p.directions = directions;
    p.rgb = rgb;
    p.grad_rgb = grad_rgb;
    p.out = grad_coeffs;
    p.partial = static_cast<double *>(workspace);
    switch (degree) {
        case 0: sh_launch_coeffs<0, 0>(p, s); break;
        case 1: sh_launch_coeffs<1, 0>(p, s); break;
        case 2: sh_launch_coeffs<2, 0>(p, s); break;
        default: sh_launch_coeffs<3, 0>(p, s); break;
    }
    const int rc = check_launch(what);
    if (rc != RF_OK) return rc;
    return cell_launch_boundaries(what, sh_entries_coeffs_boundaries_kernel, p, s);
}

int rf_sh_entries_backward_directions(uint32_t degree, int64_t num_cells, int64_t num_entries, uint32_t num_rays,
                                      const int64_t *offsets, const int64_t *cells, const float *coeffs,
                                      uint32_t coeff_pitch, const float *directions, const float *rgb,
                                      const float *grad_rgb, float *grad_directions, void *stream) {
    const char *what = "rf_sh_entries_backward_directions";
    g_err[0] = 0;
    if (degree > 3) return fail(RF_ERR_INVALID_ARGUMENT, "%s: the degree must be 0 .. 3", what);
    if (num_entries < 0) return fail(RF_ERR_INVALID_ARGUMENT, "%s: negative entry count", what);
    if (num_cells < 0) return fail(RF_ERR_INVALID_ARGUMENT, "%s: negative cell count", what);
    if (coeff_pitch < 3 * (degree + 1) * (degree + 1))
        return fail(RF_ERR_INVALID_ARGUMENT, "%s: the pitch is below the row's 3 K coefficients", what);
    if (num_rays == 0) return RF_OK;
    if (!grad_directions) return fail(RF_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (degree == 0 || num_entries == 0 || num_cells == 0) {             // a constant colour: no launch
        if (hipMemsetAsync(grad_directions, 0, (size_t)num_rays * 3 * sizeof(float), s) != hipSuccess)
            return check_launch(what);
        return RF_OK;
    }
    if (!offsets || !cells || !coeffs || !directions || !rgb || !grad_rgb)
        return fail(RF_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    ShDirParams p{};
    p.num_cells = num_cells;
    p.total = num_entries;
    p.num_rays = num_rays;
    p.pitch = coeff_pitch;
    p.offsets = offsets;
    p.cells = cells;
    p.coeffs = coeffs;
    p.directions = directions;
    p.rgb = rgb;
    p.grad_rgb = grad_rgb;
    p.out = grad_directions;
    switch (degree) {
        case 1: sh_launch_directions<1>(p, s); break;
        case 2: sh_launch_directions<2>(p, s); break;
        default: sh_launch_directions<3>(p, s); break;
    }
    return check_launch(what);
}

}  // extern "C"
