// nb_bound.hip -- nb_sim_bound: every friends-of-friends group of a simulator's current state unbound on the
// device (include/nbody.h "Bound groups"; no reference counterpart).
//
// The group finder's own kernels run first (fof_enqueue, nb_fof.hip): they leave group_of, the catalogue's label
// and count, row_start and the bodies sorted by row on the device.  Then, with no host round trip:
//   gather   -- one wave per chunk of a row's list: the members' position, mass and velocity copied into row
//               order (position p of the list), every member active, and the runs of the first moments;
//   update   -- one thread per row, after the gather (t = 0) and after every round: the round's verdict --
//               converged, dissolved, unconverged, or another round with M and V of the members that stayed, the
//               runs added in order.  A finished row raises its status word: every later block of it returns;
//   pairs    -- the hot path.  Block (x, y) = an i-tile of T members of a row against the y-th work item of the
//               row's j-range, whole segments of it (bound_seg_len: a function of the row's size alone).  The
//               j-tiles go through LDS, every lane reads the same j (a broadcast), the terms are binary32, runs
//               of 64 are folded into binary64, one partial per member and segment.  A removed member keeps its
//               place with mass 0: it adds +0 to a run, so the sums are those of the active set.  T = 64 (a
//               wave) for the small rows, 256 for the large: both make the same runs in the same order;
//   decide   -- one wave per chunk of a row's list: S_i = the partials in segment order, phi_i, k_i, e_i; a member
//               with e_i > 0 leaves (its mass in the gathered list becomes 0); the runs of the next moments;
//   sums     -- after round 1 over L (kinetic0, potential0) and at the end over B: runs of 64 by the butterfly,
//               the runs added in order by one thread per row; the minimum of phi and the smallest index there;
//   scatter  -- energy and bound_of from row order back to body order.
// All max_iter rounds are enqueued up front; the grids depend on n, the capacity and the tuning alone.  Integer
// atomics only (the count of removed members, the finished rows).
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "nb_analysis.hpp"
#include "nb_common.hpp"
#include "nb_fof.hpp"
#include "nb_psi.hpp"
#include "nb_sim.hpp"

namespace nb {

namespace {

constexpr uint32_t kThreads = kBlock;
constexpr uint32_t kListChunk = 1024;  // positions of a row's list per wave of gather, decide and sums
constexpr uint32_t kSegs = 8;          // at most this many segments of a row's j-range
constexpr uint32_t kSegMin = 1024;     // ... of at least this many positions (a multiple of 256)
constexpr uint32_t kSmallRow = kBlock; // "bound_tile" 0: rows of at most this many members take wave tiles
constexpr uint32_t kMomTerms = 4;      // m, m vx, m vy, m vz
constexpr uint32_t kSumTerms = 10;     // m, m x, m y, m z, m vx, m vy, m vz, m |x|^2, m k, m phi
constexpr uint64_t kPairsPerLaunch = 1ull << 35;  // as the diagnostics: no launch runs for long
constexpr uint32_t kLive = NB_BOUND_CONVERGED | NB_BOUND_UNCONVERGED;  // a row with a bound set

struct BoundInfo {
    unsigned long long pairs;  // pair terms of the finished rows
    uint32_t finished;         // rows with a status
    uint32_t pad;
};

// a row between the rounds
struct BoundRow {
    double mass, v[3];   // of the active set: the round to come
    double v_last[3];    // V of the last round that ran
    uint32_t active, removed, iterations, status;
};

// positions per segment of the j-range of a row of `count` members: the row's size decides, nothing else
__host__ __device__ inline uint32_t bound_seg_len(uint32_t count) {
    const uint32_t tiles = count / 256 + (count % 256 != 0), per = tiles / kSegs + (tiles % kSegs != 0);
    return per * 256 > kSegMin ? per * 256 : kSegMin;
}
__host__ __device__ inline uint32_t bound_segs(uint32_t count) {
    const uint32_t len = bound_seg_len(count);
    return count / len + (count % len != 0);
}

__device__ inline bool all_done(const FofInfo *info, const BoundInfo *bi) {
    return info->status || __atomic_load_n(&bi->finished, __ATOMIC_RELAXED) >= info->rows;
}

// ---- gather --------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void bound_gather_kernel(const FofInfo *__restrict__ info,
                                                             const float4 *__restrict__ posm,
                                                             const float4 *__restrict__ vel,
                                                             const uint32_t *__restrict__ i0p,
                                                             const uint32_t *__restrict__ i1p,
                                                             const uint32_t *__restrict__ row_start,
                                                             float4 *__restrict__ gpos, float4 *__restrict__ gvel,
                                                             uint32_t *__restrict__ active, uint32_t *__restrict__ prow,
                                                             double *__restrict__ phi, double *__restrict__ energy,
                                                             double *__restrict__ runs) {
    if (info->status) return;
    const uint32_t lane = threadIdx.x;
    uint32_t r, s, a0, a1;
    if (!item_chunk(row_start, info->rows, kListChunk, blockIdx.x, &r, &s, &a0, &a1)) return;
    const uint32_t *idx = info->passes[1] & 1 ? i1p : i0p;
    const uint32_t start = row_start[r];
    for (uint32_t a = a0; a < a1; a += kWave) {  // (kListChunk is a multiple of 64: a - start too)
        double t[kMomTerms] = {0.0, 0.0, 0.0, 0.0};
        const uint32_t p = a + lane;
        if (p < a1) {
            const uint32_t body = idx[p];
            const float4 q = posm[body], v = vel[body];
            gpos[p] = q;
            gvel[p] = make_float4(v.x, v.y, v.z, q.w);  // the mass stays here when the member leaves
            active[p] = 1u;
            prow[p] = r;
            phi[p] = energy[p] = __builtin_nan("");
            const double m = q.w;
            t[0] = m;
            t[1] = m * (double)v.x;
            t[2] = m * (double)v.y;
            t[3] = m * (double)v.z;
        }
        for (uint32_t f = 0; f < kMomTerms; ++f) t[f] = wave_sum(t[f]);
        if (lane < kMomTerms) {
            double mine = t[0];
            for (uint32_t f = 1; f < kMomTerms; ++f) mine = lane == f ? t[f] : mine;
            runs[(run_slot(start, r) + (a - start) / kWave) * kMomTerms + lane] = mine;
        }
    }
}

// ---- update: the verdict of round t (t = 0: before the first) ------------------------------------------
__global__ __launch_bounds__(kThreads) void bound_update_kernel(const FofInfo *__restrict__ info,
                                                                BoundInfo *__restrict__ bi,
                                                                const uint32_t *__restrict__ row_start,
                                                                const nb_fof_group *__restrict__ fof_rows,
                                                                const double *__restrict__ runs,
                                                                BoundRow *__restrict__ rs,
                                                                nb_bound_group *__restrict__ rows, uint32_t t,
                                                                uint32_t max_iter, uint32_t min_bound,
                                                                uint32_t max_group) {
    if (info->status) return;
    const size_t r = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= info->rows) return;
    const uint32_t start = row_start[r], count = row_start[r + 1] - start;
    BoundRow st;
    if (t == 0) {
        st = BoundRow{};
        st.active = count;
        nb_bound_group o{};
        o.label = fof_rows[r].label;
        o.count = fof_rows[r].count;
        o.most_bound = NB_FOF_NONE;
        o.phi_min = o.kinetic0 = o.potential0 = __builtin_nan("");
        rows[r] = o;
        if (max_group != 0 && count > max_group) st.status = NB_BOUND_SKIPPED;
    } else {
        st = rs[r];
        if (st.status) return;
        st.iterations = t;
        for (int a = 0; a < 3; ++a) st.v_last[a] = st.v[a];
        const uint32_t removed = st.removed;
        st.removed = 0;
        if (removed == 0) {
            st.status = NB_BOUND_CONVERGED;
        } else {
            st.active -= removed;
            if (st.active < min_bound) st.status = NB_BOUND_DISSOLVED;
            else if (t == max_iter) st.status = NB_BOUND_UNCONVERGED;
        }
    }
    if (!st.status) {  // M and P of the members that stay: the runs in order
        const double *p = runs + run_slot(start, (uint32_t)r) * kMomTerms;
        double sum[kMomTerms] = {0.0, 0.0, 0.0, 0.0};
        for (uint32_t q = 0; q < (count + kWave - 1) / kWave; ++q)
            for (uint32_t f = 0; f < kMomTerms; ++f) sum[f] += p[(size_t)q * kMomTerms + f];
        if (!(sum[0] > 0.0)) {
            st.status = NB_BOUND_DISSOLVED;
        } else {
            st.mass = sum[0];
            for (int a = 0; a < 3; ++a) st.v[a] = sum[1 + a] / sum[0];
        }
    }
    if (st.status) {
        atomicAdd(&bi->finished, 1u);
        atomicAdd(&bi->pairs, (unsigned long long)st.iterations * count * (unsigned long long)(count - 1));
    }
    rs[r] = st;
}

// ---- pairs ---------------------------------------------------------------------------------------------
// one i member against the T staged j positions: binary32 runs of 64 terms, each folded into the binary64 row
template <uint32_t T, bool kDiag, bool kMaskMassless>
__device__ __forceinline__ double tile_row(const float4 *tile, float4 pi, uint32_t tid, const PsiConst &c, double row) {
    for (uint32_t k0 = 0; k0 < T; k0 += kWave) {
        float run = 0.f;
#pragma unroll 8
        for (uint32_t k = k0; k < k0 + kWave; ++k) {
            const float4 q = tile[k];
            const float dx = q.x - pi.x, dy = q.y - pi.y, dz = q.z - pi.z;
            const float r2 = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
            float term = q.w * psi_f32(r2, c);
            if (kMaskMassless && q.w == 0.f) term = 0.f;
            if (kDiag && k == tid) term = 0.f;  // excluded by index
            run += term;
        }
        row += (double)run;
    }
    return row;
}

// The table of the tiles of kBlock members of the rows of MORE than kBlock members, by position and not by row, so
// that its size does not grow with the rows there can be: work item 2 w + kind belongs to the window of positions
// [kBlock w, kBlock w + kBlock).  A tile start of such a row lies in exactly one window, and a window holds at
// most two of them: the start of the one long row that can begin in it (kind 0: the last row that begins there --
// after a long row's start the next row begins beyond the window), and one later tile of the one long row that
// began before it (kind 1: the row that holds the window's first position; its first tile start at or after it).
// False for an item without a tile.
__device__ inline bool long_row_tile(const uint32_t *__restrict__ start, uint32_t count, uint32_t g, uint32_t *l_out,
                                     uint32_t *a0, uint32_t *a1) {
    if (count == 0) return false;
    const unsigned long long w0 = (unsigned long long)(g >> 1) * kBlock, total = start[count];
    if (w0 >= total) return false;
    const bool first = (g & 1u) == 0;
    // the last row that begins at or before x: the window's last position (kind 0) or its first (kind 1)
    const unsigned long long x = first ? std::min<unsigned long long>(w0 + kBlock, total) - 1 : w0;
    uint32_t lo = 0, hi = count;  // start[0] = 0 <= x
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (start[mid] <= x) lo = mid;
        else hi = mid;
    }
    const uint32_t s = start[lo], end = start[lo + 1];
    if (end - s <= kBlock) return false;  // not a long row
    unsigned long long t = s;
    if (first) {
        if (s < w0) return false;  // no row begins in this window
    } else {
        if (s >= w0) return false;  // (it begins here: kind 0 has it)
        t = s + (w0 - s + kBlock - 1) / kBlock * kBlock;  // in [w0, w0 + kBlock)
        if (t >= end) return false;
    }
    *l_out = lo;
    *a0 = (uint32_t)t;
    *a1 = (uint32_t)std::min<unsigned long long>(end, t + kBlock);
    return true;
}

// Block (x, y): i-tile item0 + x against segments [y spi, (y + 1) spi) of its row, spi = max(1, chunk_len / segment
// length).  The i-tiles come from the table over the rows' lists cut into tiles of T (item_chunk), or, kLongRows
// (T = kBlock), from the table of the long rows' tiles by position.  Rows outside (lo_count, hi_count] belong to the
// other tile size.  part[q * plane + p]: the partial of position p over segment q.
// kMaskMassless (e = 0 only): a massless or removed j at distance 0 would give 0 * inf; such terms are 0.
template <uint32_t T, bool kMaskMassless, bool kLongRows>
__global__ __launch_bounds__(T) void bound_pairs_kernel(const FofInfo *__restrict__ info,
                                                        const BoundInfo *__restrict__ bi,
                                                        const uint32_t *__restrict__ row_start,
                                                        const BoundRow *__restrict__ rs,
                                                        const float4 *__restrict__ gpos, uint32_t item0,
                                                        uint32_t lo_count, uint32_t hi_count, uint32_t chunk_len,
                                                        PsiConst c, double *__restrict__ part, size_t plane) {
    static_assert(!kLongRows || T == kBlock, "the table by position is the 256-thread tiles'");
    if (all_done(info, bi)) return;
    uint32_t r, s, a0, a1;
    if (kLongRows ? !long_row_tile(row_start, info->rows, item0 + blockIdx.x, &r, &a0, &a1)
                  : !item_chunk(row_start, info->rows, T, item0 + blockIdx.x, &r, &s, &a0, &a1))
        return;
    if (rs[r].status) return;
    const uint32_t start = row_start[r], count = row_start[r + 1] - start;
    if (count <= lo_count || count > hi_count) return;
    const uint32_t seg_len = bound_seg_len(count), segs = bound_segs(count);
    const uint32_t spi = chunk_len > seg_len ? chunk_len / seg_len : 1u;
    const unsigned long long q_first = (unsigned long long)blockIdx.y * spi;
    if (q_first >= segs) return;  // (everything so far is uniform over the block)
    const uint32_t q0 = (uint32_t)q_first, q1 = q_first + spi < segs ? (uint32_t)(q_first + spi) : segs;
    __shared__ float4 tile[T];
    const uint32_t tid = threadIdx.x, i = a0 + tid, end = start + count;
    float4 pi = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < a1) pi = gpos[i];
    for (uint32_t q = q0; q < q1; ++q) {
        const uint32_t j0 = start + q * seg_len, j1 = end - j0 < seg_len ? end : j0 + seg_len;  // (j0 < end <= n)
        double row = 0.0;
        for (uint32_t jt = j0; jt < j1; jt += T) {  // (the tiles of i and of j both count from the row's start)
            const uint32_t j = jt + tid;
            float4 pj = make_float4(0.f, 0.f, 0.f, 0.f);  // an absent j: massless at the origin
            if (j < j1) pj = gpos[j];
            __syncthreads();  // the previous tile has been read
            tile[tid] = pj;
            __syncthreads();
            row = jt == a0 ? tile_row<T, true, kMaskMassless>(tile, pi, tid, c, row)
                           : tile_row<T, false, kMaskMassless>(tile, pi, tid, c, row);
        }
        if (i < a1) part[(size_t)q * plane + i] = row;
    }
}

// ---- decide ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void bound_decide_kernel(const FofInfo *__restrict__ info,
                                                             const BoundInfo *__restrict__ bi,
                                                             const uint32_t *__restrict__ row_start,
                                                             BoundRow *__restrict__ rs, float4 *__restrict__ gpos,
                                                             const float4 *__restrict__ gvel,
                                                             uint32_t *__restrict__ active,
                                                             const double *__restrict__ part, size_t plane,
                                                             double coupling, double *__restrict__ phi,
                                                             double *__restrict__ energy, double *__restrict__ runs) {
#pragma clang fp contract(off)
    if (all_done(info, bi)) return;
    const uint32_t lane = threadIdx.x;
    uint32_t r, s, a0, a1;
    if (!item_chunk(row_start, info->rows, kListChunk, blockIdx.x, &r, &s, &a0, &a1)) return;
    if (rs[r].status) return;
    const uint32_t start = row_start[r], segs = bound_segs(row_start[r + 1] - start);
    const double vx = rs[r].v[0], vy = rs[r].v[1], vz = rs[r].v[2];
    for (uint32_t a = a0; a < a1; a += kWave) {
        double t[kMomTerms] = {0.0, 0.0, 0.0, 0.0};
        const uint32_t p = a + lane;
        bool leaves = false;
        if (p < a1 && active[p]) {
            double sum = part[p];
            for (uint32_t q = 1; q < segs; ++q) sum += part[(size_t)q * plane + p];
            const double ph = -(coupling * sum);
            const float4 v = gvel[p];
            const double ux = (double)v.x - vx, uy = (double)v.y - vy, uz = (double)v.z - vz;
            const double k = 0.5 * ((ux * ux + uy * uy) + uz * uz);
            const double e = k + ph;
            phi[p] = ph;
            energy[p] = e;
            leaves = e > 0.0;
            if (leaves) {
                active[p] = 0u;
                gpos[p].w = 0.f;
            } else {
                const double m = v.w;
                t[0] = m;
                t[1] = m * (double)v.x;
                t[2] = m * (double)v.y;
                t[3] = m * (double)v.z;
            }
        }
        for (uint32_t f = 0; f < kMomTerms; ++f) t[f] = wave_sum(t[f]);
        if (lane < kMomTerms) {
            double mine = t[0];
            for (uint32_t f = 1; f < kMomTerms; ++f) mine = lane == f ? t[f] : mine;
            runs[(run_slot(start, r) + (a - start) / kWave) * kMomTerms + lane] = mine;
        }
        const uint32_t gone = (uint32_t)__popcll(__ballot(leaves));
        if (lane == 0 && gone) atomicAdd(&rs[r].removed, gone);
    }
}

// ---- sums --------------------------------------------------------------------------------------------
// kFirst: over L with round 1's values, for the rows whose round 1 ran; else over B of the rows that have one
template <bool kFirst>
__global__ __launch_bounds__(kWave) void bound_sums_kernel(const FofInfo *__restrict__ info,
                                                           const uint32_t *__restrict__ row_start,
                                                           const BoundRow *__restrict__ rs,
                                                           const float4 *__restrict__ gpos,
                                                           const float4 *__restrict__ gvel,
                                                           const uint32_t *__restrict__ active,
                                                           const double *__restrict__ phi, double *__restrict__ sruns,
                                                           double *__restrict__ run_phi, uint32_t *__restrict__ run_p) {
#pragma clang fp contract(off)
    if (info->status) return;
    const uint32_t lane = threadIdx.x;
    uint32_t r, s, a0, a1;
    if (!item_chunk(row_start, info->rows, kListChunk, blockIdx.x, &r, &s, &a0, &a1)) return;
    if (kFirst ? rs[r].iterations != 1 : !(rs[r].status & kLive)) return;
    const uint32_t start = row_start[r];
    const double vx = rs[r].v_last[0], vy = rs[r].v_last[1], vz = rs[r].v_last[2];
    for (uint32_t a = a0; a < a1; a += kWave) {
        double t[kSumTerms];
        for (uint32_t f = 0; f < kSumTerms; ++f) t[f] = 0.0;
        double best = INFINITY;
        uint32_t best_p = NB_FOF_NONE;
        const uint32_t p = a + lane;
        if (p < a1 && (kFirst || active[p])) {
            const float4 q = gpos[p], v = gvel[p];
            const double m = v.w, x = q.x, y = q.y, z = q.z, wx = v.x, wy = v.y, wz = v.z;
            const double ux = wx - vx, uy = wy - vy, uz = wz - vz;
            const double k = 0.5 * ((ux * ux + uy * uy) + uz * uz);
            const double ph = phi[p];
            t[0] = m;
            t[1] = m * x;
            t[2] = m * y;
            t[3] = m * z;
            t[4] = m * wx;
            t[5] = m * wy;
            t[6] = m * wz;
            t[7] = m * ((x * x + y * y) + z * z);
            t[8] = m * k;
            t[9] = m * ph;
            best = ph;
            best_p = p;
        }
        for (uint32_t f = 0; f < kSumTerms; ++f) t[f] = wave_sum(t[f]);
        for (int o = 32; o > 0; o >>= 1) {  // the smallest phi, and the smallest position that has it
            const double other = __shfl_xor(best, o);
            const uint32_t other_p = __shfl_xor(best_p, o);
            if (other < best || (other == best && other_p < best_p)) {
                best = other;
                best_p = other_p;
            }
        }
        const size_t slot = run_slot(start, r) + (a - start) / kWave;
        if (lane < kSumTerms) {
            double mine = t[0];
            for (uint32_t f = 1; f < kSumTerms; ++f) mine = lane == f ? t[f] : mine;
            sruns[slot * kSumTerms + lane] = mine;
        }
        if (lane == 0) {
            run_phi[slot] = best;
            run_p[slot] = best_p;
        }
    }
}

// one thread per row adds the row's runs in order
template <bool kFirst>
__global__ __launch_bounds__(kThreads) void bound_combine_kernel(const FofInfo *__restrict__ info,
                                                                 const uint32_t *__restrict__ i0p,
                                                                 const uint32_t *__restrict__ i1p,
                                                                 const uint32_t *__restrict__ row_start,
                                                                 const BoundRow *__restrict__ rs,
                                                                 const double *__restrict__ sruns,
                                                                 const double *__restrict__ run_phi,
                                                                 const uint32_t *__restrict__ run_p,
                                                                 nb_bound_group *__restrict__ rows) {
    if (info->status) return;
    const size_t r = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= info->rows) return;
    const BoundRow st = rs[r];
    nb_bound_group &o = rows[r];
    if (!kFirst) {
        o.iterations = st.iterations;
        o.status = st.status;
    }
    if (kFirst ? st.iterations != 1 : !(st.status & kLive)) return;
    const uint32_t start = row_start[r], count = row_start[r + 1] - start, nruns = (count + kWave - 1) / kWave;
    const size_t slot0 = run_slot(start, (uint32_t)r);
    double sum[kSumTerms];
    for (uint32_t f = 0; f < kSumTerms; ++f) sum[f] = 0.0;
    for (uint32_t q = 0; q < nruns; ++q)
        for (uint32_t f = kFirst ? 8 : 0; f < kSumTerms; ++f) sum[f] += sruns[(slot0 + q) * kSumTerms + f];
    if (kFirst) {
        o.kinetic0 = sum[8];
        o.potential0 = 0.5 * sum[9];
        return;
    }
    double best = INFINITY;
    uint32_t best_p = NB_FOF_NONE;
    for (uint32_t q = 0; q < nruns; ++q)  // (positions ascend with the runs: < keeps the smallest)
        if (run_phi[slot0 + q] < best) {
            best = run_phi[slot0 + q];
            best_p = run_p[slot0 + q];
        }
    o.bound_count = st.active;
    o.mass = sum[0];
    for (int a = 0; a < 3; ++a) {
        o.mx[a] = sum[1 + a];
        o.mv[a] = sum[4 + a];
    }
    o.mr2 = sum[7];
    o.kinetic = sum[8];
    o.potential = 0.5 * sum[9];
    if (best_p != NB_FOF_NONE) {
        const uint32_t *idx = info->passes[1] & 1 ? i1p : i0p;
        o.phi_min = best;
        o.most_bound = idx[best_p];
    }
}

// ---- scatter: row order back to body order -----------------------------------------------------------
__global__ __launch_bounds__(kThreads) void bound_fill_kernel(uint32_t n, uint32_t *__restrict__ bound_of,
                                                              double *__restrict__ energy) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    bound_of[i] = NB_FOF_NONE;
    energy[i] = __builtin_nan("");
}

__global__ __launch_bounds__(kThreads) void bound_scatter_kernel(const FofInfo *__restrict__ info,
                                                                 const uint32_t *__restrict__ i0p,
                                                                 const uint32_t *__restrict__ i1p,
                                                                 const uint32_t *__restrict__ row_start,
                                                                 const BoundRow *__restrict__ rs,
                                                                 const uint32_t *__restrict__ prow,
                                                                 const uint32_t *__restrict__ active,
                                                                 const double *__restrict__ energy_p,
                                                                 uint32_t *__restrict__ bound_of,
                                                                 double *__restrict__ energy) {
    if (info->status || info->rows == 0) return;
    const size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= row_start[info->rows]) return;
    const uint32_t *idx = info->passes[1] & 1 ? i1p : i0p;
    const uint32_t body = idx[p], r = prow[p];
    energy[body] = energy_p[p];
    bound_of[body] = active[p] && (rs[r].status & kLive) ? r : NB_FOF_NONE;
}

}  // namespace

struct BoundWork : Workspace {  // (all grow to the largest call so far)
    DeviceBuf<float4> gpos, gvel;           // [n]: x y z m (0 once removed) and vx vy vz m, in row order
    DeviceBuf<uint32_t> active, prow;       // [n]: in row order
    DeviceBuf<double> phi, energy_p;        // [n]: in row order
    DeviceBuf<double> part;                 // [segments][n]
    DeviceBuf<double> runs, sruns, run_phi; // [run slots][kMomTerms], [run slots][kSumTerms], [run slots]
    DeviceBuf<uint32_t> run_p;              // [run slots]
    DeviceBuf<BoundRow> rs;                 // [rows possible]
    DeviceBuf<nb_bound_group> rows;         // [rows possible]
    DeviceBuf<uint32_t> bound_of;           // [n]: in body order
    DeviceBuf<double> energy;               // [n]: in body order
    DeviceBuf<BoundInfo> info;              // [1]
    PinnedBuf<uint32_t> h_group_of, h_bound_of;  // staged, so that a refused call leaves the outputs alone
    PinnedBuf<double> h_energy;
    PinnedBuf<nb_bound_group> h_rows;
    PinnedBuf<BoundInfo> h_info;            // [1]
};

namespace {

template <class B>
int bound_reserve(B &b, size_t count) {
    if (b.reserve(std::max<size_t>(1, count)) == hipSuccess) return NB_OK;
    (void)hipGetLastError();
    set_error("bound: cannot allocate the workspace (%zu elements)", count);
    return NB_ERR_ALLOC;
}

template <uint32_t T, bool kLongRows>
int launch_pairs(SimBase &sim, const FofWork &fw, const BoundWork &w, uint32_t items, uint32_t lo_count,
                 uint32_t hi_count, uint32_t largest, const PsiConst &c) {
    // An item meets at most T * largest terms: a launch takes as many items as the budget holds.  The tiles of the
    // table by position that begin in W windows are disjoint and lie within 256 W + 255 positions: two items a window.
    const uint64_t fit = std::max<uint64_t>(1, kPairsPerLaunch / ((uint64_t)T * largest));
    const uint32_t per_launch = (uint32_t)std::min<uint64_t>(items, kLongRows ? 2 * std::max<uint64_t>(1, fit - 1) : fit);
    const uint32_t ys = std::min(kSegs, (largest + kSegMin - 1) / kSegMin);  // the most segments a row can have
    for (uint32_t item0 = 0; item0 < items; item0 += per_launch) {
        const dim3 grid(std::min(per_launch, items - item0), ys);
        if (sim.params.e == 0.f)
            hipLaunchKernelGGL((bound_pairs_kernel<T, true, kLongRows>), grid, dim3(T), 0, sim.stream, fw.info, w.info,
                               fw.row_start, w.rs, w.gpos, item0, lo_count, hi_count, (uint32_t)sim.bound_chunk_len, c,
                               w.part, (size_t)sim.n);
        else
            hipLaunchKernelGGL((bound_pairs_kernel<T, false, kLongRows>), grid, dim3(T), 0, sim.stream, fw.info, w.info,
                               fw.row_start, w.rs, w.gpos, item0, lo_count, hi_count, (uint32_t)sim.bound_chunk_len, c,
                               w.part, (size_t)sim.n);
        NB_HIP_TRY(hipGetLastError());
    }
    return NB_OK;
}

}  // namespace

int sim_bound(SimBase &sim, const nb_bound_params &params, uint32_t *group_of, uint32_t *bound_of, double *energy,
              nb_bound_group *groups, size_t group_capacity, nb_bound_stats *stats) {
    if (int rc = analysis_begin(sim, "bound")) return rc;
    if (!group_of && !bound_of && !energy && !groups && !stats) {  // nothing to measure
        NB_HIP_TRY(hipStreamSynchronize(sim.stream));
        return sim.diag_status();
    }
    const uint32_t n = sim.n;
    nb_fof_params fp{};
    fp.link = params.link;
    fp.min_members = params.min_members;
    const uint32_t rows_cap = fof_rows_cap(n, group_capacity, params.min_members);
    FofWork *fof = nullptr;
    if (int rc = fof_work(sim, &fof)) return rc;
    BoundWork *work = nullptr;
    if (int rc = workspace(sim, kWorkBound, &work, [](BoundWork &f) {
            if (int rc = bound_reserve(f.info, 1)) return rc;
            return bound_reserve(f.h_info, 1);
        }))
        return rc;
    FofWork &fw = *fof;
    BoundWork &w = *work;
    FofInfo &res = *static_cast<FofInfo *>(fw.h_info);
    BoundInfo &bres = *static_cast<BoundInfo *>(w.h_info);
    std::memset(&res, 0, sizeof res);
    std::memset(&bres, 0, sizeof bres);

    if (n > 0) {
        // the largest row that is analysed, and the most runs the rows' lists can have
        const uint32_t largest = params.max_group ? std::min(n, params.max_group) : n;
        const size_t run_slots = (size_t)n / kWave + rows_cap + 1;
        const uint32_t list_items = n / kListChunk + rows_cap + 1;
        const uint32_t planes = std::min(kSegs, (largest + kSegMin - 1) / kSegMin);
        if (group_of)
            if (int rc = bound_reserve(w.h_group_of, n)) return rc;
        if (rows_cap > 0) {
            if (int rc = bound_reserve(w.gpos, n)) return rc;
            if (int rc = bound_reserve(w.gvel, n)) return rc;
            if (int rc = bound_reserve(w.active, n)) return rc;
            if (int rc = bound_reserve(w.prow, n)) return rc;
            if (int rc = bound_reserve(w.phi, n)) return rc;
            if (int rc = bound_reserve(w.energy_p, n)) return rc;
            if (int rc = bound_reserve(w.part, (size_t)planes * n)) return rc;
            if (int rc = bound_reserve(w.runs, run_slots * kMomTerms)) return rc;
            if (int rc = bound_reserve(w.sruns, run_slots * kSumTerms)) return rc;
            if (int rc = bound_reserve(w.run_phi, run_slots)) return rc;
            if (int rc = bound_reserve(w.run_p, run_slots)) return rc;
            if (int rc = bound_reserve(w.rs, rows_cap)) return rc;
            if (int rc = bound_reserve(w.rows, rows_cap)) return rc;
            if (int rc = bound_reserve(w.h_rows, rows_cap)) return rc;
            if (bound_of) {
                if (int rc = bound_reserve(w.bound_of, n)) return rc;
                if (int rc = bound_reserve(w.h_bound_of, n)) return rc;
            }
            if (energy) {
                if (int rc = bound_reserve(w.energy, n)) return rc;
                if (int rc = bound_reserve(w.h_energy, n)) return rc;
            }
        }
        if (int rc = fof_enqueue(sim, fw, fp, rows_cap, group_of != nullptr, false)) return rc;
        NB_HIP_TRY(hipMemcpyAsync(fw.h_info, fw.info, sizeof(FofInfo), hipMemcpyDeviceToHost, sim.stream));
        if (group_of)
            NB_HIP_TRY(hipMemcpyAsync(w.h_group_of, fw.group_of, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, sim.stream));
        if (rows_cap > 0) {
            const float4 *posm = nullptr, *vel = nullptr;
            sim.diag_state(&posm, &vel);
            const FofInfo *info = fw.info;
            const uint32_t *i0 = fw.sort.idx[0], *i1 = fw.sort.idx[1];
            const uint32_t row_blocks = (rows_cap + kThreads - 1) / kThreads, blocks = (n + kThreads - 1) / kThreads;
            const double coupling = (double)sim.params.g * (double)sim.params.dt;
            const PsiConst c = psi_const(sim.params.e);
            const uint32_t tile = (uint32_t)sim.bound_tile;
            NB_HIP_TRY(hipMemsetAsync(w.info, 0, sizeof(BoundInfo), sim.stream));
            hipLaunchKernelGGL(bound_gather_kernel, dim3(list_items), dim3(kWave), 0, sim.stream, info, posm, vel, i0, i1,
                               fw.row_start, w.gpos, w.gvel, w.active, w.prow, w.phi, w.energy_p, w.runs);
            NB_HIP_TRY(hipGetLastError());
            for (uint32_t t = 0; t <= params.max_iter; ++t) {
                if (t > 0) {
                    // wave tiles for the rows of (0, small], block tiles for those of (small, largest]
                    const uint32_t small = tile == 0 ? std::min(kSmallRow, largest) : tile == kWave ? largest : 0u;
                    if (small > 0)
                        if (int rc = launch_pairs<kWave, false>(sim, fw, w, n / kWave + rows_cap + 1, 0u, small, small, c))
                            return rc;
                    if (small < largest) {
                        // block tiles for all rows ("bound_tile" 256): the table over the rows' lists; for the
                        // rows above kSmallRow = kBlock members alone: the table by position, two items a window
                        if (int rc = small == kBlock
                                         ? launch_pairs<kThreads, true>(sim, fw, w, 2 * (n / kThreads + 1), small, largest,
                                                                        largest, c)
                                         : launch_pairs<kThreads, false>(sim, fw, w, n / kThreads + rows_cap + 1, small,
                                                                         largest, largest, c))
                            return rc;
                    }
                    hipLaunchKernelGGL(bound_decide_kernel, dim3(list_items), dim3(kWave), 0, sim.stream, info, w.info,
                                       fw.row_start, w.rs, w.gpos, w.gvel, w.active, w.part, (size_t)n, coupling, w.phi,
                                       w.energy_p, w.runs);
                    NB_HIP_TRY(hipGetLastError());
                }
                hipLaunchKernelGGL(bound_update_kernel, dim3(row_blocks), dim3(kThreads), 0, sim.stream, info, w.info,
                                   fw.row_start, fw.rows, w.runs, w.rs, w.rows, t, params.max_iter, params.min_bound,
                                   params.max_group);
                NB_HIP_TRY(hipGetLastError());
                if (t == 1) {  // kinetic0 and potential0, while round 1's values stand
                    hipLaunchKernelGGL(bound_sums_kernel<true>, dim3(list_items), dim3(kWave), 0, sim.stream, info,
                                       fw.row_start, w.rs, w.gpos, w.gvel, w.active, w.phi, w.sruns, w.run_phi, w.run_p);
                    NB_HIP_TRY(hipGetLastError());
                    hipLaunchKernelGGL(bound_combine_kernel<true>, dim3(row_blocks), dim3(kThreads), 0, sim.stream, info,
                                       i0, i1, fw.row_start, w.rs, w.sruns, w.run_phi, w.run_p, w.rows);
                    NB_HIP_TRY(hipGetLastError());
                }
            }
            hipLaunchKernelGGL(bound_sums_kernel<false>, dim3(list_items), dim3(kWave), 0, sim.stream, info, fw.row_start,
                               w.rs, w.gpos, w.gvel, w.active, w.phi, w.sruns, w.run_phi, w.run_p);
            NB_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(bound_combine_kernel<false>, dim3(row_blocks), dim3(kThreads), 0, sim.stream, info, i0, i1,
                               fw.row_start, w.rs, w.sruns, w.run_phi, w.run_p, w.rows);
            NB_HIP_TRY(hipGetLastError());
            if (bound_of || energy) {
                // (a buffer that is not asked for is not written: the other one's stands in for it)
                uint32_t *d_bound = bound_of ? (uint32_t *)w.bound_of : nullptr;
                double *d_energy = energy ? (double *)w.energy : nullptr;
                if (!d_bound) {
                    if (int rc = bound_reserve(w.bound_of, n)) return rc;
                    d_bound = w.bound_of;
                }
                if (!d_energy) {
                    if (int rc = bound_reserve(w.energy, n)) return rc;
                    d_energy = w.energy;
                }
                hipLaunchKernelGGL(bound_fill_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, n, d_bound, d_energy);
                NB_HIP_TRY(hipGetLastError());
                hipLaunchKernelGGL(bound_scatter_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, info, i0, i1,
                                   fw.row_start, w.rs, w.prow, w.active, w.energy_p, d_bound, d_energy);
                NB_HIP_TRY(hipGetLastError());
                if (bound_of)
                    NB_HIP_TRY(hipMemcpyAsync(w.h_bound_of, d_bound, sizeof(uint32_t) * n, hipMemcpyDeviceToHost,
                                              sim.stream));
                if (energy)
                    NB_HIP_TRY(hipMemcpyAsync(w.h_energy, d_energy, sizeof(double) * n, hipMemcpyDeviceToHost,
                                              sim.stream));
            }
            NB_HIP_TRY(hipMemcpyAsync(w.h_rows, w.rows, sizeof(nb_bound_group) * rows_cap, hipMemcpyDeviceToHost,
                                      sim.stream));
            NB_HIP_TRY(hipMemcpyAsync(w.h_info, w.info, sizeof(BoundInfo), hipMemcpyDeviceToHost, sim.stream));
        }
    }
    NB_HIP_TRY(hipStreamSynchronize(sim.stream));
    if (int rc = sim.diag_status()) return rc;
    if (res.status) return fof_refused(fp);
    const nb_bound_group *h_rows = w.h_rows;
    if (n > 0) {
        if (group_of) std::memcpy(group_of, w.h_group_of, sizeof(uint32_t) * n);
        if (rows_cap > 0) {
            if (bound_of) std::memcpy(bound_of, w.h_bound_of, sizeof(uint32_t) * n);
            if (energy) std::memcpy(energy, w.h_energy, sizeof(double) * n);
            if (groups && res.rows > 0) std::memcpy(groups, h_rows, sizeof(nb_bound_group) * res.rows);
        } else {  // no row is analysed
            if (bound_of) std::fill(bound_of, bound_of + n, NB_FOF_NONE);
            if (energy) std::fill(energy, energy + n, std::nan(""));
        }
    }
    if (stats) {
        nb_bound_stats o{};
        o.step_num = sim.step_num;
        o.n = n;
        o.nonfinite = n - res.n_ok;
        o.components = res.components;
        o.groups = res.groups;
        o.grouped_bodies = res.grouped_bodies;
        o.largest_count = (uint32_t)(res.largest >> 32);
        o.largest_label = ~(uint32_t)res.largest;
        for (uint32_t r = 0; r < res.rows; ++r) {
            const nb_bound_group &g = h_rows[r];
            if (g.bound_count > 0) {
                ++o.bound_groups;
                o.bound_bodies += g.bound_count;
            }
            o.dissolved += g.status == NB_BOUND_DISSOLVED;
            o.unconverged += g.status == NB_BOUND_UNCONVERGED;
            o.skipped += g.status == NB_BOUND_SKIPPED;
            o.rounds_max = std::max(o.rounds_max, g.iterations);
        }
        o.pairs = bres.pairs;
        *stats = o;
    }
    return NB_OK;
}

}  // namespace nb
