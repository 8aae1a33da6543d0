// rf_tets.hip -- the Delaunay tetrahedra from the neighbour lists ("Tetrahedra from the neighbour lists").  The
// row check, the star from a row, the canonical row, the order of a star's rows, the match and the face pairing:
// rf_tets.hpp, shared with the host build of tests/host_harness.
//
//   tets_count_kernel        one lane per site, a wave = 64 consecutive sites; the star is a private Star<64,124> (scratch),
//                            as in delaunay_star_kernel.  Checks the row, builds the star, writes the counts and a code byte;
//                            a row of more than 63 neighbours only writes its class.
//   tets_count_large_kernel  the rows of a larger class (listed ascending by the caller): Star<250,496> or
//                            Star<4096,8188,uint16_t,1024> in a workspace, a lane per row, a fixed number of lanes.  Rare;
//                            written for correctness.
//   tets_emit_kernel         rebuilds the star and writes the owned rows, canonical and in order, at the scan's offset and
//   tets_emit_large_kernel   every finite triangle as an ascending triple at the other scan's.
//   tets_match_kernel        one lane per site: every entry is binary-searched among its owner's rows; ticks the corner,
//                            keeps the smallest row (vert_to_tet) and counts the entries without a row.
//   tets_pair_faces_kernel   one lane per sorted face: pairs it with its equal neighbour.
//
// Every output element is written exactly once by a plain store (the ticks: plain stores of 1 into zeroed bytes, one
// store per byte when the lists are consistent); there are no atomics; every index read from memory is range-checked
// before it is used.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/radfoam_hip_tets.h"
#include "rf_host.hpp"

#define RF_STAR_FN __device__ __forceinline__
#define RF_STAR_NOINLINE __device__ __noinline__
#define RF_STAR_NOUNROLL _Pragma("nounroll")
#include "rf_tets.hpp"

namespace rf {
namespace tets {

constexpr uint32_t kFlat = 256;
constexpr uint32_t kBigSlots = 256, kHugeSlots = 16;   // stars of the larger instances at work at a time

// what a lane of a larger instance works in
template <typename S>
struct Slot {
    S star;
    uint32_t seeds[S::kV];
    float d2[S::kV];
    uint16_t ord[S::kT];
};

__global__ __launch_bounds__(64) void tets_count_kernel(const float *__restrict__ pts, uint32_t n,
                                                        const uint32_t *__restrict__ adj, uint32_t num_edges,
                                                        const uint32_t *__restrict__ off, uint8_t *__restrict__ code,
                                                        uint32_t *__restrict__ entries, uint32_t *__restrict__ owned,
                                                        uint32_t *__restrict__ ghosts) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    uint32_t first, deg, ne = 0, no = 0, ng = 0;
    uint8_t c = row_bounds(off, n, num_edges, i, first, deg);
    if (c == kOk) c = row_check(adj + first, deg, n, i);
    if (c == kOk) {
        if (deg > kBigRow) {
            c = kNeedHuge;
        } else if (deg > kSmallRow) {
            c = kNeedBig;
        } else {
            SmallStar s;
            uint32_t seeds[SmallStar::kV];
            float d2[SmallStar::kV];
            c = star_from_row(s, pts, i, adj + first, deg, seeds, d2, kNeedBig);
            if (c == kOk) star_counts(s, ne, no, ng);
        }
    }
    code[i] = c;
    entries[i] = ne;
    owned[i] = no;
    ghosts[i] = ng;
}

template <typename S>
__global__ __launch_bounds__(64) void tets_count_large_kernel(const float *__restrict__ pts, uint32_t n,
                                                              const uint32_t *__restrict__ adj, uint32_t num_edges,
                                                              const uint32_t *__restrict__ off,
                                                              const int64_t *__restrict__ rows, uint32_t num_rows,
                                                              uint32_t slots, uint8_t ok, uint8_t next,
                                                              uint8_t *__restrict__ code, uint32_t *__restrict__ entries,
                                                              uint32_t *__restrict__ owned, uint32_t *__restrict__ ghosts,
                                                              Slot<S> *__restrict__ ws) {
    const uint32_t lane = blockIdx.x * 64u + threadIdx.x;
    if (lane >= slots) return;
    Slot<S> &w = ws[lane];
    for (uint32_t r = lane; r < num_rows; r += slots) {
        const int64_t at = rows[r];
        if (at < 0 || at >= (int64_t)n) continue;
        const uint32_t i = (uint32_t)at;
        uint32_t first, deg, ne = 0, no = 0, ng = 0;
        uint8_t c = row_bounds(off, n, num_edges, i, first, deg);
        if (c == kOk) c = row_check(adj + first, deg, n, i);
        if (c == kOk) c = star_from_row(w.star, pts, i, adj + first, deg, w.seeds, w.d2, next);
        if (c == kOk) {
            star_counts(w.star, ne, no, ng);
            c = ok;
        }
        code[i] = c;
        entries[i] = ne;
        owned[i] = no;
        ghosts[i] = ng;
    }
}

// where site i writes, or false: its ranges of the two scans, checked against the totals and the instance's room
__device__ __forceinline__ bool emit_ranges(uint32_t i, const int64_t *__restrict__ owned_off,
                                            const int64_t *__restrict__ entries_off, int64_t num_tets, int64_t num_entries,
                                            int64_t room, int64_t &o0, int64_t &no, int64_t &e0, int64_t &ne) {
    o0 = owned_off[i];
    no = owned_off[i + 1] - o0;
    e0 = entries_off[i];
    ne = entries_off[i + 1] - e0;
    return o0 >= 0 && no >= 0 && no <= room && o0 <= num_tets - no && e0 >= 0 && ne >= 0 && ne <= room &&
           e0 <= num_entries - ne;
}

__global__ __launch_bounds__(64) void tets_emit_kernel(const float *__restrict__ pts, uint32_t n,
                                                       const uint32_t *__restrict__ adj, uint32_t num_edges,
                                                       const uint32_t *__restrict__ off, const uint8_t *__restrict__ code,
                                                       const int64_t *__restrict__ owned_off,
                                                       const int64_t *__restrict__ entries_off, int64_t num_tets,
                                                       int64_t num_entries, uint32_t *__restrict__ tets,
                                                       uint32_t *__restrict__ star_entries, uint32_t *__restrict__ faults) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n || code[i] != kOk) return;
    uint32_t first, deg, result = kNone;
    int64_t o0, no, e0, ne;
    uint8_t c = row_bounds(off, n, num_edges, i, first, deg);
    if (c == kOk) c = row_check(adj + first, deg, n, i);
    if (c == kOk && deg <= kSmallRow &&
        emit_ranges(i, owned_off, entries_off, num_tets, num_entries, SmallStar::kT, o0, no, e0, ne)) {
        SmallStar s;
        uint32_t seeds[SmallStar::kV];
        float d2[SmallStar::kV];
        uint16_t ord[SmallStar::kT];
        if (star_from_row(s, pts, i, adj + first, deg, seeds, d2, kNeedBig) == kOk)
            result = star_emit(s, pts, ord, (uint32_t)no, (uint32_t)ne, tets + 4 * (size_t)o0, star_entries + 3 * (size_t)e0);
    }
    faults[i] = result;
}

template <typename S>
__global__ __launch_bounds__(64) void tets_emit_large_kernel(const float *__restrict__ pts, uint32_t n,
                                                             const uint32_t *__restrict__ adj, uint32_t num_edges,
                                                             const uint32_t *__restrict__ off,
                                                             const int64_t *__restrict__ rows, uint32_t num_rows,
                                                             uint32_t slots, uint8_t ok, const uint8_t *__restrict__ code,
                                                             const int64_t *__restrict__ owned_off,
                                                             const int64_t *__restrict__ entries_off, int64_t num_tets,
                                                             int64_t num_entries, uint32_t *__restrict__ tets,
                                                             uint32_t *__restrict__ star_entries,
                                                             uint32_t *__restrict__ faults, Slot<S> *__restrict__ ws) {
    const uint32_t lane = blockIdx.x * 64u + threadIdx.x;
    if (lane >= slots) return;
    Slot<S> &w = ws[lane];
    for (uint32_t r = lane; r < num_rows; r += slots) {
        const int64_t at = rows[r];
        if (at < 0 || at >= (int64_t)n) continue;
        const uint32_t i = (uint32_t)at;
        if (code[i] != ok) continue;
        uint32_t first, deg, result = kNone;
        int64_t o0, no, e0, ne;
        uint8_t c = row_bounds(off, n, num_edges, i, first, deg);
        if (c == kOk) c = row_check(adj + first, deg, n, i);
        if (c == kOk && emit_ranges(i, owned_off, entries_off, num_tets, num_entries, S::kT, o0, no, e0, ne) &&
            star_from_row(w.star, pts, i, adj + first, deg, w.seeds, w.d2, kTooLong) == kOk)
            result = star_emit(w.star, pts, w.ord, (uint32_t)no, (uint32_t)ne, tets + 4 * (size_t)o0,
                               star_entries + 3 * (size_t)e0);
        faults[i] = result;
    }
}

__global__ __launch_bounds__(kFlat) void tets_match_kernel(uint32_t n, const uint32_t *__restrict__ star_entries,
                                                           const int64_t *__restrict__ entries_off, int64_t num_entries,
                                                           const uint32_t *__restrict__ tets,
                                                           const int64_t *__restrict__ owned_off, int64_t num_tets,
                                                           uint8_t *__restrict__ ticks, uint32_t *__restrict__ missing,
                                                           uint32_t *__restrict__ vert_to_tet) {
    const uint32_t v = blockIdx.x * kFlat + threadIdx.x;
    if (v >= n) return;
    const int64_t e0 = entries_off[v], ne = entries_off[v + 1] - e0;
    uint32_t lost = kNone, first = kNone;
    if (e0 >= 0 && ne >= 0 && ne <= (int64_t)HugeStar::kT && e0 <= num_entries - ne)
        lost = match_site(v, n, star_entries + 3 * (size_t)e0, (uint32_t)ne, owned_off, tets, num_tets, ticks, first);
    missing[v] = lost;
    vert_to_tet[v] = first;
}

__global__ __launch_bounds__(kFlat) void tets_pair_faces_kernel(const uint32_t *__restrict__ tets, int64_t num_faces,
                                                                const int64_t *__restrict__ order,
                                                                uint32_t *__restrict__ adjacency,
                                                                uint8_t *__restrict__ single, uint8_t *__restrict__ fault) {
    const int64_t i = (int64_t)blockIdx.x * kFlat + threadIdx.x;
    if (i >= num_faces) return;
    pair_face(tets, num_faces, order, i, adjacency, single, fault);
}

inline const char *lists_fault(uint32_t num_points, uint32_t num_edges) {
    if (num_points >= 0x80000000u) return "2^31 points or more";
    if (num_edges >= 0x80000000u) return "2^31 adjacency entries or more";
    return nullptr;
}

inline const char *totals_fault(int64_t num_tets, int64_t num_entries) {
    if (num_tets < 0 || num_tets > 0x40000000ll) return "more than 2^30 tetrahedra";
    if (num_entries < 0 || num_entries > 4 * 0x40000000ll) return "more than 2^32 star entries";
    return nullptr;
}

}  // namespace tets
}  // namespace rf

using namespace rf;

extern "C" {

int rf_tets_count(const float *points, uint32_t num_points, const uint32_t *adjacency, uint32_t num_edges,
                  const uint32_t *offsets, uint8_t *code, uint32_t *entries, uint32_t *owned, uint32_t *ghosts,
                  void *stream) {
    g_err[0] = 0;
    if (num_points == 0) return RF_OK;
    if (!points || !offsets || !code || !entries || !owned || !ghosts || (num_edges && !adjacency))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_tets_count: null pointer");
    if (const char *why = tets::lists_fault(num_points, num_edges))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_tets_count: %s", why);
    hipLaunchKernelGGL(tets::tets_count_kernel, dim3((num_points + 63u) / 64u), dim3(64), 0,
                       static_cast<hipStream_t>(stream), points, num_points, adjacency, num_edges, offsets, code, entries,
                       owned, ghosts);
    return check_launch("rf_tets_count");
}

size_t rf_tets_large_workspace_bytes(uint32_t instance) {
    if (instance == 1u) return sizeof(tets::Slot<tets::BigStar>) * tets::kBigSlots;
    if (instance == 2u) return sizeof(tets::Slot<tets::HugeStar>) * tets::kHugeSlots;
    return 0;
}

int rf_tets_count_large(uint32_t instance, const float *points, uint32_t num_points, const uint32_t *adjacency,
                        uint32_t num_edges, const uint32_t *offsets, const int64_t *rows, uint32_t num_rows, uint8_t *code,
                        uint32_t *entries, uint32_t *owned, uint32_t *ghosts, void *workspace, size_t workspace_bytes,
                        void *stream) {
    g_err[0] = 0;
    if (num_rows == 0) return RF_OK;
    if (!points || !offsets || !adjacency || !rows || !code || !entries || !owned || !ghosts || !workspace)
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_tets_count_large: null pointer");
    if (instance != 1u && instance != 2u) return fail(RF_ERR_INVALID_ARGUMENT, "rf_tets_count_large: instance must be 1 or 2");
    if (workspace_bytes < rf_tets_large_workspace_bytes(instance) || (uintptr_t)workspace % 16u)
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_tets_count_large: workspace too small or not 16-byte aligned");
    if (const char *why = tets::lists_fault(num_points, num_edges))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_tets_count_large: %s", why);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (instance == 1u)
        hipLaunchKernelGGL(tets::tets_count_large_kernel<tets::BigStar>, dim3((tets::kBigSlots + 63u) / 64u), dim3(64), 0, s,
                           points, num_points, adjacency, num_edges, offsets, rows, num_rows, tets::kBigSlots,
                           (uint8_t)tets::kOkBig, (uint8_t)tets::kNeedHuge, code, entries, owned, ghosts,
                           static_cast<tets::Slot<tets::BigStar> *>(workspace));
    else
        hipLaunchKernelGGL(tets::tets_count_large_kernel<tets::HugeStar>, dim3((tets::kHugeSlots + 63u) / 64u), dim3(64), 0,
                           s, points, num_points, adjacency, num_edges, offsets, rows, num_rows, tets::kHugeSlots,
                           (uint8_t)tets::kOkHuge, (uint8_t)tets::kTooLong, code, entries, owned, ghosts,
                           static_cast<tets::Slot<tets::HugeStar> *>(workspace));
    return check_launch("rf_tets_count_large");
}

int rf_tets_emit(const float *points, uint32_t num_points, const uint32_t *adjacency, uint32_t num_edges,
                 const uint32_t *offsets, const uint8_t *code, const int64_t *owned_off, const int64_t *entries_off,
                 int64_t num_tets, int64_t num_entries, uint32_t *tets_out, uint32_t *star_entries, uint32_t *faults,
                 void *stream) {
    g_err[0] = 0;
    if (num_points == 0) return RF_OK;
    if (!points || !offsets || !code || !owned_off || !entries_off || !faults || (num_edges && !adjacency) ||
        (num_tets && !tets_out) || (num_entries && !star_entries))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_tets_emit: null pointer");
    if (const char *why = tets::lists_fault(num_points, num_edges))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_tets_emit: %s", why);
    if (const char *why = tets::totals_fault(num_tets, num_entries))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_tets_emit: %s", why);
    hipLaunchKernelGGL(tets::tets_emit_kernel, dim3((num_points + 63u) / 64u), dim3(64), 0,
                       static_cast<hipStream_t>(stream), points, num_points, adjacency, num_edges, offsets, code,
                       owned_off, entries_off, num_tets, num_entries, tets_out, star_entries, faults);
    return check_launch("rf_tets_emit");
}

int rf_tets_emit_large(uint32_t instance, const float *points, uint32_t num_points, const uint32_t *adjacency,
                       uint32_t num_edges, const uint32_t *offsets, const int64_t *rows, uint32_t num_rows,
                       const uint8_t *code, const int64_t *owned_off, const int64_t *entries_off, int64_t num_tets,
                       int64_t num_entries, uint32_t *tets_out, uint32_t *star_entries, uint32_t *faults, void *workspace,
                       size_t workspace_bytes, void *stream) {
    g_err[0] = 0;
    if (num_rows == 0) return RF_OK;
    if (!points || !offsets || !adjacency || !rows || !code || !owned_off || !entries_off || !faults || !workspace ||
        (num_tets && !tets_out) || (num_entries && !star_entries))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_tets_emit_large: null pointer");
    if (instance != 1u && instance != 2u) return fail(RF_ERR_INVALID_ARGUMENT, "rf_tets_emit_large: instance must be 1 or 2");
    if (workspace_bytes < rf_tets_large_workspace_bytes(instance) || (uintptr_t)workspace % 16u)
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_tets_emit_large: workspace too small or not 16-byte aligned");
    if (const char *why = tets::lists_fault(num_points, num_edges))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_tets_emit_large: %s", why);
    if (const char *why = tets::totals_fault(num_tets, num_entries))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_tets_emit_large: %s", why);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (instance == 1u)
        hipLaunchKernelGGL(tets::tets_emit_large_kernel<tets::BigStar>, dim3((tets::kBigSlots + 63u) / 64u), dim3(64), 0, s,
                           points, num_points, adjacency, num_edges, offsets, rows, num_rows, tets::kBigSlots,
                           (uint8_t)tets::kOkBig, code, owned_off, entries_off, num_tets, num_entries, tets_out,
                           star_entries, faults, static_cast<tets::Slot<tets::BigStar> *>(workspace));
    else
        hipLaunchKernelGGL(tets::tets_emit_large_kernel<tets::HugeStar>, dim3((tets::kHugeSlots + 63u) / 64u), dim3(64), 0,
                           s, points, num_points, adjacency, num_edges, offsets, rows, num_rows, tets::kHugeSlots,
                           (uint8_t)tets::kOkHuge, code, owned_off, entries_off, num_tets, num_entries, tets_out,
                           star_entries, faults, static_cast<tets::Slot<tets::HugeStar> *>(workspace));
    return check_launch("rf_tets_emit_large");
}

int rf_tets_match(uint32_t num_points, const uint32_t *star_entries, const int64_t *entries_off, int64_t num_entries,
                  const uint32_t *tets_in, const int64_t *owned_off, int64_t num_tets, uint8_t *ticks, uint32_t *missing,
                  uint32_t *vert_to_tet, void *stream) {
    g_err[0] = 0;
    if (num_points == 0) return RF_OK;
    if (!entries_off || !owned_off || !missing || !vert_to_tet || (num_entries && !star_entries) ||
        (num_tets && (!tets_in || !ticks)))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_tets_match: null pointer");
    if (num_points >= 0x80000000u) return fail(RF_ERR_INVALID_ARGUMENT, "rf_tets_match: 2^31 points or more");
    if (const char *why = tets::totals_fault(num_tets, num_entries))
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_tets_match: %s", why);
    hipLaunchKernelGGL(tets::tets_match_kernel, dim3((num_points + tets::kFlat - 1u) / tets::kFlat), dim3(tets::kFlat), 0,
                       static_cast<hipStream_t>(stream), num_points, star_entries, entries_off, num_entries, tets_in,
                       owned_off, num_tets, ticks, missing, vert_to_tet);
    return check_launch("rf_tets_match");
}

int rf_tets_pair_faces(const uint32_t *tets_in, int64_t num_tets, const int64_t *order, uint32_t *tet_adjacency,
                       uint8_t *single, uint8_t *fault, void *stream) {
    g_err[0] = 0;
    if (num_tets == 0) return RF_OK;
    if (!tets_in || !order || !tet_adjacency || !single || !fault)
        return fail(RF_ERR_INVALID_ARGUMENT, "rf_tets_pair_faces: null pointer");
    if (num_tets < 0 || num_tets > 0x40000000ll) return fail(RF_ERR_INVALID_ARGUMENT, "rf_tets_pair_faces: more than 2^30 tetrahedra");
    const int64_t faces = 4 * num_tets;
    hipLaunchKernelGGL(tets::tets_pair_faces_kernel, dim3((uint32_t)((faces + tets::kFlat - 1) / tets::kFlat)),
                       dim3(tets::kFlat), 0, static_cast<hipStream_t>(stream), tets_in, faces, order, tet_adjacency, single,
                       fault);
    return check_launch("rf_tets_pair_faces");
}

}  // extern "C"
