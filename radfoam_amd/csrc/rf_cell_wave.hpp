// rf_cell_wave.hpp -- the wave scheme of the kernels that go over the Voronoi cells one by one (rf_cell_geometry.hip,
// rf_cell_geometry_grad.hip, rf_cell_moments.hip, rf_cell_moments_grad.hip, rf_face_area_grad.hip, rf_cell_box.hip,
// rf_cell_box_grad.hip, rf_cell_box_moments.hip, rf_cell_box_moments_grad.hip, rf_cell_box_area_grad.hip; DESIGN.md, "Cell
// geometry"), and the host-side pieces their C entry points share.  rf_cell_mesh.hip takes the constants and the redo
// helpers.  For the .hip files only: the arithmetic is in the rf_clip*.hpp headers, which stay free of HIP types.
//
// ONE WAVE OWNS ONE CELL, ONE LANE ONE FACE.  The wave checks the cell's adjacency row, each lane loads its neighbour
// (load_neighbour) and the planes {d_c, |d_c|^2 / 2} are staged once in LDS, in one of three layouts: the row alone
// (stage_row); the row, then the six walls of a box as lanes of their own (cell_box_kernel, cell_box_moments_kernel); the
// row by its lanes and the walls behind it by lanes 0..5, taking no lanes (store_plane under `have`, then stage_walls:
// the three box gradients).  The wave meets at a barrier and a row with a bad entry is handed on (sync_any_bad).  Then
// each lane clips its face's square by the other planes, its polygon in an LDS slot of its own: vertex-major, the lanes
// side by side, so lanes at the same vertex index hit different banks, two buffers of kLaneCap vertices and no per-lane
// arrays.  The lane forms its operator's term of the face, the wave adds the terms up (wave_sum) and lane 0 writes the
// cell.  Every output element is written exactly once by a plain store; there are no atomics.
//
// WHAT DOES NOT FIT IS HANDED ON, untouched, through redo[cell] (hand_on; the lane that wrote a cell says so with keep):
// a malformed row, a row of more faces than the wave has lanes for, a polygon of more than kLaneCap vertices.  A second
// kernel, one wave per 64 cells, reads redo[] a lane per cell (redo_todo); the cells handed on are walked one after the
// other (redo_next), face by face, by lane 0 with the operator's rf::clip::*_serial (what the host harnesses run) and
// room for kWaveCap vertices: slow, and rare.  What that cannot do either is named in cell_status and the caller raises.
//
// Each kernel declares its own __shared__ arrays, since their order sets their offsets, and passes the plane array
// itself, whose stride the helpers take from its type.  Everything here is inlined into the kernels that use it, and the
// kernels' gfx950 code is what it was when each spelled the scheme out: scripts/isa_same.py tells whether an edit
// changed it.  That rule is why some pieces are NOT here but in every kernel, as the same few lines: the row check, the
// clip loop over a plane list with walls (clip::clip_by_list_plane) and the two labelled clip loops, the staging where
// the walls take lanes, and the staging of face_area_grad_kernel.  Shared forms of them compiled to other code.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "rf_clip_box.hpp"
#include "rf_host.hpp"

namespace rf {

constexpr uint32_t kWave = 64;
constexpr uint32_t kLaneCap = 16;    // polygon vertices per lane: 2 buffers * 2 coordinates * 16 * 64 lanes * 8 B = 32 KiB
constexpr uint32_t kWaveCap = 256;   // polygon vertices of the serial path: 2 buffers * 2 coordinates * 256 * 8 B = 8 KiB

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// ---- the hand-off ----
__device__ __forceinline__ void hand_on(uint8_t *redo, uint32_t a, uint32_t lane) {
    if (lane == 0) redo[a] = 1;
}
// by the lane that wrote cell a
__device__ __forceinline__ void keep(uint8_t *redo, uint32_t a) { redo[a] = 0; }

// ---- the row ----
// The check of row a is three lines in each kernel: begin > end || end > num_edges || end - begin > limit hands the cell
// on (wave-uniform), with limit = kWave, or kWave - kWalls where the walls take lanes.  Through a helper the compiler
// folds the three comparisons into one branch, which the kernels' code does not have.

// what a lane holds of its plane of the list
struct CellLane {
    bool have;   // a face of the row
    bool bad;    // the row's entry is out of range or the site itself, or its plane is not in front of the site
    uint32_t q;  // the neighbour; a itself where there is none
    double dx, dy, dz, h;
};

__device__ __forceinline__ CellLane load_neighbour(const float *points, uint32_t num_points, const uint32_t *adj,
                                                   uint32_t a, uint32_t begin, uint32_t degree, uint32_t lane) {
    CellLane f;
    f.have = lane < degree;
    f.q = f.have ? adj[begin + lane] : 0u;
    f.bad = f.have && (f.q >= num_points || f.q == a);
    if (!f.have || f.bad) f.q = a;
    clip::neighbour(points, a, f.q, f.dx, f.dy, f.dz, f.h);
    f.bad = f.bad || (f.have && !(f.h > 0.0));
    return f;
}

// plane[4][kStride]: d (x, y, z) and h of entry j
template <uint32_t kStride>
__device__ __forceinline__ void store_plane(double (&plane)[4][kStride], uint32_t j, double dx, double dy, double dz,
                                            double h) {
    plane[0][j] = dx, plane[1][j] = dy, plane[2][j] = dz, plane[3][j] = h;
}

// the row alone; every lane stores, a lane without a face the plane of a itself, which nothing reads
template <uint32_t kStride>
__device__ __forceinline__ CellLane stage_row(const float *points, uint32_t num_points, const uint32_t *adj, uint32_t a,
                                              uint32_t begin, uint32_t degree, uint32_t lane,
                                              double (&plane)[4][kStride]) {
    const CellLane f = load_neighbour(points, num_points, adj, a, begin, degree, lane);
    store_plane(plane, lane, f.dx, f.dy, f.dz, f.h);
    return f;
}

// the six walls behind a row that only the lanes with a face stored, by lanes 0..5: the walls take no lanes
__device__ __forceinline__ void stage_walls(const float *points, uint32_t a, const clip::Box &box, uint32_t degree,
                                            uint32_t lane, double (&plane)[4][kWave + clip::kWalls]) {
    if (lane < clip::kWalls) {
        double wx, wy, wz, wh;
        clip::wall_plane(points, a, box, lane, wx, wy, wz, wh);
        store_plane(plane, degree + lane, wx, wy, wz, wh);
    }
}

// after the staging: the barrier, then whether any lane's entry is bad (the cell is to be handed on)
__device__ __forceinline__ bool sync_any_bad(bool bad) {
    __syncthreads();
    return __any(bad);
}

// ---- one lane's clipping by the other planes of the row ----
// From the square of half-side R in the lane's LDS slot (s, t: stride kWave, two buffers of kLaneCap) to the polygon's m
// vertices in buffer cur.  overflow: more than kLaneCap vertices, the cell is to be handed on.
struct Clipped {
    uint32_t m, cur;
    bool overflow;
};
__device__ __forceinline__ Clipped clip_by_row(const clip::Frame &frame, const double (&plane)[4][kWave], uint32_t degree,
                                               uint32_t lane, double R, double *s, double *t) {
    clip::init_square(s, t, kWave, R);
    uint32_t m = 4, cur = 0;
    for (uint32_t j = 0; j < degree && m != 0; ++j) {
        if (j == lane) continue;
        double A, B, C;
        clip::plane_in_frame(frame, plane[0][j], plane[1][j], plane[2][j], plane[3][j], A, B, C);
        const uint32_t in = cur * kLaneCap * kWave, out = (cur ^ 1u) * kLaneCap * kWave;
        if (!clip::clip_step(s + in, t + in, s + out, t + out, kWave, kLaneCap, m, A, B, C)) return {m, cur, true};
        cur ^= 1u;
    }
    return {m, cur, false};
}

// the row of a as the wave staged it in LDS, for the edge terms of the area gradients: planes[4][kStride] and the sites
template <uint32_t kStride>
struct RowFromLds {
    const double *planes;
    const uint32_t *sites;
    __device__ __forceinline__ uint32_t site(uint32_t j) const { return sites[j]; }
    __device__ __forceinline__ void plane(uint32_t j, double &dx, double &dy, double &dz, double &h) const {
        dx = planes[j], dy = planes[kStride + j], dz = planes[2 * kStride + j], h = planes[3 * kStride + j];
    }
};

// ---- the redo kernel: one wave per 64 cells (or faces), a lane per cell ----
// Every lane: kCellOk into the status of a cell that was not handed on; returns the wave's cells that were, as a mask.
// Lane 0 then walks them alone: `if (threadIdx.x != 0) return;`, the clipping square's R, and
// `while (todo) { i = redo_next(todo); status[i] = <the operator's *_serial>(i); }`.
__device__ __forceinline__ unsigned long long redo_todo(uint32_t num, const uint8_t *redo, uint8_t *status) {
    const uint32_t cell = blockIdx.x * kWave + threadIdx.x;
    const bool mine = cell < num && redo[cell] != 0;
    if (cell < num && !mine) status[cell] = (uint8_t)clip::kCellOk;
    return __ballot(mine);
}
__device__ __forceinline__ uint32_t redo_next(unsigned long long &todo) {
    const uint32_t i = blockIdx.x * kWave + (uint32_t)__builtin_ctzll(todo);
    todo &= todo - 1ull;
    return i;
}

// ---- host ----
inline size_t redo_bytes(uint32_t num_points) { return ((size_t)num_points + 255u) & ~(size_t)255u; }

inline int check_box(const char *op, double lo_x, double lo_y, double lo_z, double hi_x, double hi_y, double hi_z) {
    if (!(lo_x < hi_x && lo_y < hi_y && lo_z < hi_z) || !(hi_x - lo_x < __builtin_inf()) ||
        !(hi_y - lo_y < __builtin_inf()) || !(hi_z - lo_z < __builtin_inf()))
        return fail(RF_ERR_INVALID_ARGUMENT, "%s: the box must be finite with lo < hi", op);
    return RF_OK;
}

// the wave kernel over the cells, then its redo kernel: `args` are the parameters the two have in common
template <class Main, class Redo, class... Args>
inline int launch_cell_waves(const char *op, void *stream, uint32_t num_points, void *workspace, uint8_t *cell_status,
                             Main main_kernel, Redo redo_kernel, Args... args) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t *redo = static_cast<uint8_t *>(workspace);
    hipLaunchKernelGGL(main_kernel, dim3(num_points), dim3(kWave), 0, s, args..., redo);
    hipLaunchKernelGGL(redo_kernel, dim3((num_points + kWave - 1u) / kWave), dim3(kWave), 0, s, args..., redo,
                       cell_status);
    return check_launch(op);
}

}  // namespace rf
