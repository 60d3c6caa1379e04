// nb_hop.hip -- nb_sim_hop: the density-peak groups of a simulator's current state, the boundaries between them
// (include/nbody.h "Density-peak groups"; no reference counterpart).
//
// Every inside body hops to the densest of itself and its first k_hop neighbours; the hops end at peaks, a
// body's label is its peak.  "Denser" is a strict total order (the density, then the smaller index), so next[],
// the labels, the catalogue and the boundary table are unique given the state, whatever order the threads ran in.
//   density -- knn_enqueue (nb_knn.hpp) with k = k_density: nb_sim_knn's own kernels, so the same bits.  It leaves
//              the sorted keys, the sorted positions and the plan, which the next search reads;
//   hop     -- the search of nb_knn.hpp again with k = max(k_hop, k_merge), one wave per inside body.  Its
//              epilogue: lanes < k_hop load the density of their neighbour, a wave butterfly in the "denser" order
//              over them and the body itself picks next[body]; lanes < k_merge store their neighbour into the
//              [n][k_merge] table.  A body that is not inside keeps next = NB_HOP_NONE and an empty table row;
//   chains  -- next resolved to peaks in place: every body walks to the body that points at itself and stores
//              it.  A stored value is always a body further along the same chain, so a walk that reads it ends
//              at the same peak: any interleaving reaches the same fixed point;
//   rows    -- fof_catalogue_enqueue (nb_fof.hpp): labels, sizes, rows, group_of and the nine sums exactly as
//              nb_sim_fof forms them; then the rows' peak densities;
//   bounds  -- one slot per (body, neighbour) of the table: the key (a << B | b, B = the bits of n) of a taken
//              pair, or the key past all of them, and the pair's value; the stable sort of nb_analysis_sort.hpp;
//              heads of equal keys scanned into table rows; count by integer atomic add, maximum by integer
//              atomic maximum of the order-preserving encoding of the value, decoded at the end.
// No float atomics anywhere.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "nb_analysis.hpp"
#include "nb_analysis_sort.hpp"
#include "nb_common.hpp"
#include "nb_fof.hpp"
#include "nb_knn.hpp"
#include "nb_sim.hpp"

namespace nb {

namespace {

constexpr uint32_t kThreads = kBlock;

// The integer results of a call, on the device.  Written by integer atomics or single threads.
struct HopInfo {
    unsigned long long outside, boundary_pairs;
    uint32_t boundaries;   // label pairs: the scan's total
    uint32_t reserved;
};

__device__ inline double unordered64_dev(unsigned long long e) {
    const unsigned long long u = (e >> 63) ? (e & ~(1ull << 63)) : ~e;
    return __longlong_as_double((long long)u);
}

// rho': the ordering key of a density
__device__ inline double rho_key(double density) { return density != density ? -(double)INFINITY : density; }

// is (ra, a) denser than (rb, b)?
__device__ inline bool denser(double ra, uint32_t a, double rb, uint32_t b) { return ra > rb || (ra == rb && a < b); }

// ---- hop ------------------------------------------------------------------------------------------
// One wave per sorted position, as knn_search_kernel.  k = max(k_hop, k_merge); k_all = max(k_density, k).
__global__ __launch_bounds__(kThreads) void hop_search_kernel(const KnnInfo *__restrict__ info,
                                                              const unsigned long long *__restrict__ keys,
                                                              const uint32_t *__restrict__ sidx,
                                                              const float4 *__restrict__ spos,
                                                              const double *__restrict__ density, uint32_t k_all,
                                                              uint32_t k, uint32_t k_hop, uint32_t k_merge,
                                                              double density_min, uint32_t span,
                                                              uint32_t *__restrict__ next, uint32_t *__restrict__ nbr,
                                                              HopInfo *__restrict__ hinfo) {
#pragma clang fp contract(off)
    const uint32_t c = info->n_ok;
    if (c <= k_all) return;  // short: the presets stand
    const size_t pl = (size_t)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
    if (pl >= c) return;  // (uniform over the wave)
    const uint32_t p = (uint32_t)pl, lane = threadIdx.x % kWave;
    const uint32_t body = sidx[p];
    const double rho = rho_key(density[body]);
    if (!(rho >= density_min)) {  // outside (uniform over the wave)
        if (lane == 0) atomicAdd(&hinfo->outside, 1ull);
        return;
    }
    Query q;
    knn_search(q, info, keys, sidx, spos, c, p, k, span);

    // lane l < k holds the (l + 1)-th body of the order
    double best_rho = rho;
    uint32_t best = body;
    if (lane < k_hop) {
        best_rho = rho_key(density[q.lj]);
        best = q.lj;
    }
    for (int o = 32; o > 0; o >>= 1) {  // a strict total order: every lane ends with the one densest candidate
        const double orho = __shfl_xor(best_rho, o);
        const uint32_t other = __shfl_xor(best, o);
        if (denser(orho, other, best_rho, best)) {
            best_rho = orho;
            best = other;
        }
    }
    if (denser(rho, body, best_rho, best)) best = body;  // (k_hop == 64: no lane held the body itself)
    if (lane < k_merge) nbr[(size_t)body * k_merge + lane] = q.lj;
    if (lane == 0) next[body] = best;
}

// ---- chains ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void hop_chain_kernel(uint32_t *next, uint32_t n) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    uint32_t x = __atomic_load_n(next + i, __ATOMIC_RELAXED);
    if (x == NB_HOP_NONE) return;
    for (;;) {  // every hop goes to a strictly denser body: the walk ends
        const uint32_t p = __atomic_load_n(next + x, __ATOMIC_RELAXED);
        if (p == x) break;
        x = p;
    }
    __atomic_store_n(next + i, x, __ATOMIC_RELAXED);
}

// peak[r] = density[label of row r]
__global__ __launch_bounds__(kThreads) void hop_peak_kernel(const FofInfo *__restrict__ finfo,
                                                            const nb_fof_group *__restrict__ rows,
                                                            const double *__restrict__ density,
                                                            double *__restrict__ peak) {
    const size_t r = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= finfo->rows) return;
    peak[r] = density[rows[r].label];
}

// ---- boundaries -----------------------------------------------------------------------------------
// slot s = (body i, neighbour l): the key of the pair when it is taken, else key_none; its value
__global__ __launch_bounds__(kThreads) void hop_emit_kernel(const uint32_t *__restrict__ labels,
                                                            const uint32_t *__restrict__ nbr,
                                                            const double *__restrict__ density, uint32_t slots,
                                                            uint32_t k_merge, uint32_t bits,
                                                            unsigned long long key_none,
                                                            unsigned long long *__restrict__ keys,
                                                            double *__restrict__ val, HopInfo *__restrict__ hinfo) {
#pragma clang fp contract(off)
    const size_t s = (size_t)blockIdx.x * kThreads + threadIdx.x;
    bool taken = false;
    if (s < slots) {
        const uint32_t i = (uint32_t)(s / k_merge), j = nbr[s];
        unsigned long long key = key_none;
        double v = 0.0;
        if (j != NB_HOP_NONE) {  // (i is inside: only then was its row of the table written)
            const uint32_t li = labels[i], lj = labels[j];
            if (lj != NB_HOP_NONE && li != lj) {
                taken = true;
                key = ((unsigned long long)std::min(li, lj) << bits) | std::max(li, lj);
                v = 0.5 * (rho_key(density[i]) + rho_key(density[j]));
            }
        }
        keys[s] = key;
        val[s] = v;
    }
    const unsigned long long m = __ballot(taken);
    if (m && threadIdx.x % kWave == 0) atomicAdd(&hinfo->boundary_pairs, (unsigned long long)__popcll(m));
}

// flags[p] = 1 where a label pair starts in the sorted keys
__global__ __launch_bounds__(kThreads) void hop_heads_kernel(const unsigned long long *__restrict__ keys,
                                                             uint32_t slots, unsigned long long key_none,
                                                             uint32_t *__restrict__ flags) {
    const size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= slots) return;
    const unsigned long long key = keys[p];
    flags[p] = key != key_none && (p == 0 || keys[p - 1] != key);
}

// flags scanned in place (inclusive inside a block of kScanThreads); block_tot[b] = the flags of block b
__global__ __launch_bounds__(kScanThreads) void hop_scan_local_kernel(uint32_t *__restrict__ flags, uint32_t slots,
                                                                      uint32_t *__restrict__ block_tot) {
    __shared__ uint32_t lds[2 * kScanThreads];
    const uint32_t tid = threadIdx.x;
    const size_t i = (size_t)blockIdx.x * kScanThreads + tid;
    uint32_t *a = lds, *b = lds + kScanThreads;
    a[tid] = i < slots ? flags[i] : 0u;
    __syncthreads();
    for (uint32_t o = 1; o < kScanThreads; o <<= 1) {
        b[tid] = tid >= o ? a[tid] + a[tid - o] : a[tid];
        __syncthreads();
        uint32_t *t = a;
        a = b;
        b = t;
    }
    if (i < slots) flags[i] = a[tid];
    if (tid == kScanThreads - 1) block_tot[blockIdx.x] = a[tid];
}

__global__ __launch_bounds__(kScanThreads) void hop_scan_blocks_kernel(uint32_t *__restrict__ block_tot,
                                                                       uint32_t blocks, HopInfo *__restrict__ hinfo) {
    __shared__ uint32_t lds[2 * kScanThreads];
    const uint32_t t = block_scan_runs(block_tot, blocks, lds);
    if (threadIdx.x == 0) hinfo->boundaries = t;
}

// sorted position p of a taken pair into its table row (rows below `capacity` only): the head writes the labels,
// every pair counts and offers its value
__global__ __launch_bounds__(kThreads) void hop_reduce_kernel(const unsigned long long *__restrict__ keys,
                                                              const uint32_t *__restrict__ idx,
                                                              const double *__restrict__ val,
                                                              const uint32_t *__restrict__ incl,
                                                              const uint32_t *__restrict__ block_tot, uint32_t slots,
                                                              uint32_t bits, unsigned long long key_none,
                                                              uint32_t capacity, nb_hop_boundary *__restrict__ table) {
    const size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= slots) return;
    const unsigned long long key = keys[p];
    if (key == key_none) return;
    const uint32_t row = incl[p] + block_tot[p / kScanThreads] - 1;
    if (row >= capacity) return;
    if (p == 0 || keys[p - 1] != key) {
        table[row].a = (uint32_t)(key >> bits);
        table[row].b = (uint32_t)(key & ((1ull << bits) - 1ull));
    }
    atomicAdd(&table[row].pairs, 1u);
    atomicMax(reinterpret_cast<unsigned long long *>(&table[row].density), ordered64(val[idx[p]]));
}

// the maxima decoded in place
__global__ __launch_bounds__(kThreads) void hop_decode_kernel(const HopInfo *__restrict__ hinfo, uint32_t capacity,
                                                              nb_hop_boundary *__restrict__ table) {
    const size_t r = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= std::min(hinfo->boundaries, capacity)) return;
    unsigned long long *e = reinterpret_cast<unsigned long long *>(&table[r].density);
    const double v = unordered64_dev(*e);
    table[r].density = v;
}

uint32_t bits_of(unsigned long long x) {
    uint32_t b = 0;
    while (x) {
        ++b;
        x >>= 1;
    }
    return b;
}

}  // namespace

static_assert(sizeof(nb_hop_boundary) == 24 && offsetof(nb_hop_boundary, density) == 16, "four words and a double");

struct HopWork : Workspace {  // (all grow to the largest call so far)
    DeviceBuf<uint32_t> next;               // [n]: the hop, then the peak
    DeviceBuf<uint32_t> nbr;                // [n][k_merge]: the first k_merge neighbours of an inside body
    SortBufs<unsigned long long> sort;      // [n k_merge]: the pairs' keys
    DeviceBuf<double> val;                  // [n k_merge]: the pairs' values, by slot
    DeviceBuf<uint32_t> flags, block_tot;   // [n k_merge], [scan blocks]: the heads and their scan
    DeviceBuf<nb_hop_boundary> table;       // [boundary rows possible]
    DeviceBuf<double> peak;                 // [catalogue rows possible]
    PinnedBuf<uint32_t> h_labels, h_group_of;  // staged, so that a failed call leaves the outputs alone
    PinnedBuf<double> h_density, h_peak;
    PinnedBuf<nb_fof_group> h_rows;
    PinnedBuf<nb_hop_boundary> h_table;
    DeviceBuf<HopInfo> info;                // [1]
    PinnedBuf<HopInfo> h_info;              // [1]
    PinnedBuf<FofInfo> h_finfo;             // [1]
    PinnedBuf<KnnInfo> h_kinfo;             // [1]
};

namespace {

template <class B>
int hop_reserve(B &b, size_t count) {
    if (b.reserve(std::max<size_t>(1, count)) == hipSuccess) return NB_OK;
    (void)hipGetLastError();
    set_error("hop: cannot allocate the workspace (%zu elements)", count);
    return NB_ERR_ALLOC;
}

}  // namespace

int sim_hop(SimBase &sim, const nb_hop_params &params, uint32_t *labels, uint32_t *group_of, double *density,
            nb_fof_group *groups, double *peak_density, size_t group_capacity, nb_hop_boundary *boundaries,
            size_t boundary_capacity, nb_hop_stats *stats) {
    if (int rc = analysis_begin(sim, "hop")) return rc;
    if (!groups && !peak_density) group_capacity = 0;
    if (!boundaries) boundary_capacity = 0;
    if (!labels && !group_of && !density && !groups && !peak_density && !boundaries && !stats) {  // nothing to measure
        NB_HIP_TRY(hipStreamSynchronize(sim.stream));
        return sim.diag_status();
    }
    const uint32_t n = sim.n, k_merge = params.k_merge, k = std::max(params.k_hop, k_merge);
    const uint32_t k_all = std::max(params.k_density, k);
    const unsigned long long slots64 = (unsigned long long)n * k_merge;
    if (slots64 > 0x7fffffffull) {
        set_error("hop: %u bodies of %u boundary neighbours are more than one call takes", n, k_merge);
        return NB_ERR_UNSUPPORTED;
    }
    const uint32_t slots = (uint32_t)slots64;
    const uint32_t rows_cap = fof_rows_cap(n, group_capacity, params.min_members);
    // a label pair needs at least one slot
    const uint32_t table_cap = (uint32_t)std::min<unsigned long long>(boundary_capacity, slots64);
    KnnWork *kwork = nullptr;
    FofWork *fwork = nullptr;
    HopWork *work = nullptr;
    if (int rc = knn_work(sim, &kwork)) return rc;
    if (int rc = fof_work(sim, &fwork)) return rc;
    if (int rc = workspace(sim, kWorkHop, &work, [](HopWork &f) {
            if (f.info.reserve(1) != hipSuccess || f.h_info.reserve(1) != hipSuccess ||
                f.h_finfo.reserve(1) != hipSuccess || f.h_kinfo.reserve(1) != hipSuccess) {
                (void)hipGetLastError();
                set_error("hop: cannot allocate the result workspace");
                return NB_ERR_ALLOC;
            }
            return NB_OK;
        }))
        return rc;
    KnnWork &kw = *kwork;
    FofWork &fw = *fwork;
    HopWork &w = *work;
    HopInfo &res = *static_cast<HopInfo *>(w.h_info);
    FofInfo &fres = *static_cast<FofInfo *>(w.h_finfo);
    KnnInfo &kres = *static_cast<KnnInfo *>(w.h_kinfo);
    std::memset(&res, 0, sizeof res);
    std::memset(&fres, 0, sizeof fres);  // (largest = 0: count 0, label NB_HOP_NONE)
    std::memset(&kres, 0, sizeof kres);

    if (n > 0) {
        const uint32_t blocks = (n + kThreads - 1) / kThreads, slot_blocks = (slots + kThreads - 1) / kThreads;
        const uint32_t scan_blocks = (slots + kScanThreads - 1) / kScanThreads;
        const SortShape shape = sort_shape(slots);
        const uint32_t bits = std::max(1u, bits_of(n - 1));   // labels are below n
        const unsigned long long key_none = 1ull << (2 * bits);  // past every pair's key (bits <= 31)
        const uint32_t passes = (2 * bits + 1 + 7) / 8;
        const uint32_t per_block = (uint32_t)sim.knn_block_queries, span = (uint32_t)sim.knn_span_cells;
        if (int rc = hop_reserve(w.next, n)) return rc;
        if (int rc = hop_reserve(w.nbr, slots)) return rc;
        if (int rc = w.sort.reserve(slots, shape, [](auto &b, size_t count) { return hop_reserve(b, count); })) return rc;
        if (int rc = hop_reserve(w.val, slots)) return rc;
        if (int rc = hop_reserve(w.flags, slots)) return rc;
        if (int rc = hop_reserve(w.block_tot, scan_blocks)) return rc;
        if (int rc = hop_reserve(w.table, table_cap)) return rc;
        if (int rc = hop_reserve(w.peak, rows_cap)) return rc;
        if (int rc = fof_catalogue_reserve(fw, n, rows_cap)) return rc;
        if (labels)
            if (int rc = hop_reserve(w.h_labels, n)) return rc;
        if (group_of)
            if (int rc = hop_reserve(w.h_group_of, n)) return rc;
        if (density)
            if (int rc = hop_reserve(w.h_density, n)) return rc;
        if (rows_cap > 0) {
            if (int rc = hop_reserve(w.h_rows, rows_cap)) return rc;
            if (int rc = hop_reserve(w.h_peak, rows_cap)) return rc;
        }
        if (table_cap > 0)
            if (int rc = hop_reserve(w.h_table, table_cap)) return rc;

        // density: nb_sim_knn's own kernels
        if (int rc = knn_enqueue(sim, kw, params.k_density)) return rc;
        // hop
        HopInfo *info = w.info;
        const unsigned long long *keys = kw.sort.keys[0];
        const uint32_t *sidx = kw.sort.idx[0];
        NB_HIP_TRY(hipMemsetAsync(info, 0, sizeof(HopInfo), sim.stream));
        NB_HIP_TRY(hipMemsetAsync(w.next, 0xff, sizeof(uint32_t) * n, sim.stream));     // NB_HOP_NONE
        NB_HIP_TRY(hipMemsetAsync(w.nbr, 0xff, sizeof(uint32_t) * slots, sim.stream));  // NB_HOP_NONE
        hipLaunchKernelGGL(hop_search_kernel, dim3((n + per_block - 1) / per_block), dim3(per_block * kWave), 0,
                           sim.stream, kw.info, keys, sidx, kw.spos, kw.density, k_all, k, params.k_hop, k_merge,
                           params.density_min, span, w.next, w.nbr, info);
        NB_HIP_TRY(hipGetLastError());
        // chains
        hipLaunchKernelGGL(hop_chain_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, w.next, n);
        NB_HIP_TRY(hipGetLastError());
        // rows: the group finders' shared catalogue, from a plan that refuses nothing
        NB_HIP_TRY(hipMemsetAsync(fw.info, 0, sizeof(FofInfo), sim.stream));
        if (int rc = fof_catalogue_enqueue(sim, fw, w.next, params.min_members, rows_cap, group_of != nullptr, true))
            return rc;
        if (rows_cap > 0) {
            hipLaunchKernelGGL(hop_peak_kernel, dim3((rows_cap + kThreads - 1) / kThreads), dim3(kThreads), 0,
                               sim.stream, fw.info, fw.rows, kw.density, w.peak);
            NB_HIP_TRY(hipGetLastError());
        }
        // boundaries
        hipLaunchKernelGGL(hop_emit_kernel, dim3(slot_blocks), dim3(kThreads), 0, sim.stream, w.next, w.nbr,
                           kw.density, slots, k_merge, bits, key_none, w.sort.keys[0], w.val, info);
        NB_HIP_TRY(hipGetLastError());
        if (int rc = enqueue_sort(sim.stream, w.sort, slots, shape, passes, 0, nullptr)) return rc;
        const unsigned long long *skeys = w.sort.keys[passes & 1];
        const uint32_t *sslot = w.sort.idx[passes & 1];
        hipLaunchKernelGGL(hop_heads_kernel, dim3(slot_blocks), dim3(kThreads), 0, sim.stream, skeys, slots, key_none,
                           w.flags);
        NB_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(hop_scan_local_kernel, dim3(scan_blocks), dim3(kScanThreads), 0, sim.stream, w.flags, slots,
                           w.block_tot);
        NB_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(hop_scan_blocks_kernel, dim3(1), dim3(kScanThreads), 0, sim.stream, w.block_tot, scan_blocks,
                           info);
        NB_HIP_TRY(hipGetLastError());
        if (table_cap > 0) {
            NB_HIP_TRY(hipMemsetAsync(w.table, 0, sizeof(nb_hop_boundary) * table_cap, sim.stream));
            hipLaunchKernelGGL(hop_reduce_kernel, dim3(slot_blocks), dim3(kThreads), 0, sim.stream, skeys, sslot, w.val,
                               w.flags, w.block_tot, slots, bits, key_none, table_cap, w.table);
            NB_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(hop_decode_kernel, dim3((table_cap + kThreads - 1) / kThreads), dim3(kThreads), 0,
                               sim.stream, info, table_cap, w.table);
            NB_HIP_TRY(hipGetLastError());
        }
        NB_HIP_TRY(hipMemcpyAsync(w.h_info, info, sizeof(HopInfo), hipMemcpyDeviceToHost, sim.stream));
        NB_HIP_TRY(hipMemcpyAsync(w.h_finfo, fw.info, sizeof(FofInfo), hipMemcpyDeviceToHost, sim.stream));
        NB_HIP_TRY(hipMemcpyAsync(w.h_kinfo, kw.info, sizeof(KnnInfo), hipMemcpyDeviceToHost, sim.stream));
        if (labels)
            NB_HIP_TRY(hipMemcpyAsync(w.h_labels, fw.labels, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, sim.stream));
        if (group_of)
            NB_HIP_TRY(hipMemcpyAsync(w.h_group_of, fw.group_of, sizeof(uint32_t) * n, hipMemcpyDeviceToHost,
                                      sim.stream));
        if (density)
            NB_HIP_TRY(hipMemcpyAsync(w.h_density, kw.density, sizeof(double) * n, hipMemcpyDeviceToHost, sim.stream));
        if (rows_cap > 0) {
            NB_HIP_TRY(hipMemcpyAsync(w.h_rows, fw.rows, sizeof(nb_fof_group) * rows_cap, hipMemcpyDeviceToHost,
                                      sim.stream));
            NB_HIP_TRY(hipMemcpyAsync(w.h_peak, w.peak, sizeof(double) * rows_cap, hipMemcpyDeviceToHost, sim.stream));
        }
        if (table_cap > 0)
            NB_HIP_TRY(hipMemcpyAsync(w.h_table, w.table, sizeof(nb_hop_boundary) * table_cap, hipMemcpyDeviceToHost,
                                      sim.stream));
    }
    NB_HIP_TRY(hipStreamSynchronize(sim.stream));
    if (int rc = sim.diag_status()) return rc;
    if (n > 0) {
        if (labels) std::memcpy(labels, w.h_labels, sizeof(uint32_t) * n);
        if (group_of) std::memcpy(group_of, w.h_group_of, sizeof(uint32_t) * n);
        if (density) std::memcpy(density, w.h_density, sizeof(double) * n);
        if (groups && fres.rows > 0) std::memcpy(groups, w.h_rows, sizeof(nb_fof_group) * fres.rows);
        if (peak_density && fres.rows > 0) std::memcpy(peak_density, w.h_peak, sizeof(double) * fres.rows);
        const size_t brows = std::min<size_t>(res.boundaries, table_cap);
        if (brows > 0) std::memcpy(boundaries, w.h_table, sizeof(nb_hop_boundary) * brows);
    }
    if (stats) {
        nb_hop_stats o{};
        o.step_num = sim.step_num;
        o.n = n;
        o.nonfinite = n - kres.n_ok;
        o.counted = kres.n_ok;
        o.outside = res.outside;
        o.short_of_k = kres.n_ok <= k_all ? kres.n_ok : 0;
        o.peaks = fres.components;
        o.groups = fres.groups;
        o.grouped_bodies = fres.grouped_bodies;
        o.boundaries = res.boundaries;
        o.boundary_pairs = res.boundary_pairs;
        o.largest_count = (uint32_t)(fres.largest >> 32);
        o.largest_label = ~(uint32_t)fres.largest;
        *stats = o;
    }
    return NB_OK;
}

}  // namespace nb
