// nb_assign.hpp -- the front end of a pass that starts from a caller's assignment of bodies to rows (nb_shape.hip;
// DESIGN.md 6n "The front end"): group_of[n] from the host, every value NB_FOF_NONE or a row < m.  Enqueued on the
// simulator's stream with no synchronisation, it leaves on the device
//   info        -- the values that are no row (their number, the smallest body index that has one), the members
//                  that do not count (body_ok) and the members that do;
//   row_start   -- [m + 1]: row r's list is the positions [row_start[r], row_start[r + 1]), row_start[m] = members;
//   the lists   -- the counted members sorted stably by row, so every row's list is in ascending body index: the
//                  body of a position (idx()), its row (rows()), and its position, mass and velocity gathered once
//                  (gpos, gvel).
// The key of a body is its row, or m for a body of no row, a body that does not count and a value that is no row;
// the sort is nb_analysis_sort.hpp's on as many 8-bit digits as m has, known on the host.  Integer work only.
#pragma once

#include <cstring>

#include "nb_analysis.hpp"
#include "nb_analysis_sort.hpp"
#include "nb_common.hpp"
#include "nb_sim.hpp"

namespace nb {

struct AssignInfo {
    uint32_t invalid;        // values that are neither NB_FOF_NONE nor < m
    uint32_t first_invalid;  // the smallest body index with one (NB_FOF_NONE: none)
    uint32_t nonfinite;      // members that do not count
    uint32_t members;        // members that do
};

// 8-bit digits of the largest key, m
inline uint32_t assign_passes(uint32_t m) {
    uint32_t passes = 1;
    while (passes < 4 && (m >> (8 * passes))) ++passes;
    return passes;
}

#ifdef __HIPCC__

struct AssignBufs {  // (all grow to the largest call so far)
    PinnedBuf<uint32_t> h_group_of;  // [n]
    DeviceBuf<uint32_t> group_of;    // [n]
    SortBufs<uint32_t> sort;         // the two sides of (row, body index), the histogram
    DeviceBuf<uint32_t> row_start;   // [m + 1]
    DeviceBuf<float4> gpos, gvel;    // [n]: x y z m and vx vy vz -, in list order
    DeviceBuf<AssignInfo> info;      // [1]
    PinnedBuf<AssignInfo> h_info;    // [1]
    uint32_t side = 0;               // of `sort`, where the last call's lists are
    const uint32_t *idx() const { return sort.idx[side]; }
    const uint32_t *rows() const { return sort.keys[side]; }

    template <class Reserve>
    int reserve(uint32_t n, uint32_t m, Reserve reserve) {
        if (int rc = reserve(h_group_of, (size_t)n)) return rc;
        if (int rc = reserve(group_of, (size_t)n)) return rc;
        if (int rc = sort.reserve(n, sort_shape(n), reserve)) return rc;
        if (int rc = reserve(row_start, (size_t)m + 1)) return rc;
        if (int rc = reserve(gpos, (size_t)n)) return rc;
        if (int rc = reserve(gvel, (size_t)n)) return rc;
        if (int rc = reserve(info, (size_t)1)) return rc;
        return reserve(h_info, (size_t)1);
    }
};

namespace {

__global__ __launch_bounds__(kBlock) void assign_key_kernel(const uint32_t *__restrict__ group_of,
                                                            const float4 *__restrict__ posm,
                                                            const float4 *__restrict__ vel, uint32_t n, uint32_t m,
                                                            AssignInfo *__restrict__ info,
                                                            uint32_t *__restrict__ keys) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t g = group_of[i];
    uint32_t key = m;
    if (g != NB_FOF_NONE) {
        if (g >= m) {
            atomicAdd(&info->invalid, 1u);
            atomicMin(&info->first_invalid, (uint32_t)i);
        } else if (!body_ok(posm[i], vel[i])) {
            atomicAdd(&info->nonfinite, 1u);
        } else {
            key = g;
        }
    }
    keys[i] = key;
}

// row_start[r] = the first position of the ascending keys[0 .. n) with a key >= r, for r = 0 .. m
__global__ __launch_bounds__(kBlock) void assign_rows_kernel(const uint32_t *__restrict__ keys, uint32_t n,
                                                             uint32_t m, uint32_t *__restrict__ row_start,
                                                             AssignInfo *__restrict__ info) {
    const size_t r = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (r > m) return;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < r) lo = mid + 1;
        else hi = mid;
    }
    row_start[r] = lo;
    if (r == m) info->members = lo;
}

__global__ __launch_bounds__(kBlock) void assign_gather_kernel(const uint32_t *__restrict__ row_start, uint32_t m,
                                                               const uint32_t *__restrict__ idx,
                                                               const float4 *__restrict__ posm,
                                                               const float4 *__restrict__ vel,
                                                               float4 *__restrict__ gpos, float4 *__restrict__ gvel) {
    const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= row_start[m]) return;
    const uint32_t body = idx[p];
    gpos[p] = posm[body];
    gvel[p] = vel[body];
}

// n > 0; b.reserve(n, m, ...) has succeeded.  With m == 0 only the values are checked: there is no list.
int assign_enqueue(hipStream_t stream, AssignBufs &b, const uint32_t *group_of, uint32_t n, uint32_t m,
                   const float4 *posm, const float4 *vel) {
    const uint32_t blocks = (n + kBlock - 1) / kBlock, passes = assign_passes(m);
    std::memcpy(b.h_group_of, group_of, sizeof(uint32_t) * n);
    NB_HIP_TRY(hipMemcpyAsync(b.group_of, b.h_group_of, sizeof(uint32_t) * n, hipMemcpyHostToDevice, stream));
    AssignInfo zero{};
    zero.first_invalid = NB_FOF_NONE;
    *static_cast<AssignInfo *>(b.h_info) = zero;
    NB_HIP_TRY(hipMemcpyAsync(b.info, b.h_info, sizeof(AssignInfo), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(assign_key_kernel, dim3(blocks), dim3(kBlock), 0, stream, (const uint32_t *)b.group_of, posm, vel,
                       n, m, (AssignInfo *)b.info, (uint32_t *)b.sort.keys[0]);
    NB_HIP_TRY(hipGetLastError());
    b.side = 0;
    if (m == 0) return NB_OK;
    if (int rc = enqueue_sort(stream, b.sort, n, sort_shape(n), passes, 0, nullptr)) return rc;
    b.side = passes & 1;
    hipLaunchKernelGGL(assign_rows_kernel, dim3(m / kBlock + 1), dim3(kBlock), 0, stream, b.rows(), n, m,
                       (uint32_t *)b.row_start, (AssignInfo *)b.info);
    NB_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(assign_gather_kernel, dim3(blocks), dim3(kBlock), 0, stream, (const uint32_t *)b.row_start, m,
                       b.idx(), posm, vel, (float4 *)b.gpos, (float4 *)b.gvel);
    NB_HIP_TRY(hipGetLastError());
    return NB_OK;
}

}  // namespace

#endif  // __HIPCC__

}  // namespace nb
