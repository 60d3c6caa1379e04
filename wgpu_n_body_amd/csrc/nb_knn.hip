// nb_knn.hip -- nb_sim_knn: the k-th neighbour, the mass inside it and the density it gives, per body of a
// simulator's current state, and the density-weighted sums (include/nbody.h "k-nearest-neighbour density",
// DESIGN.md 6i; no reference counterpart).
//
// For a counted body i the other counted bodies are ordered by (d2(i, j), j); the k-th of them fixes r2, kth,
// mass_in and density.  The order is total (j is unique), so everything per body is unique given the state,
// whatever order the threads ran in.
//   bounds  -- the per-axis minimum and maximum of the counted bodies (body_ok) and their number c over the float4
//              SoA state (SimBase::diag_state), by the bounds pass of nb_analysis_sort.hpp; the one block that
//              finishes them makes the plan on the device: lo, hi and the side h = (largest extent) 2^-21 of
//              the finest cells.  Every later kernel reads the plan;
//   key     -- a body's cell on an axis is the q with e(q) <= x < e(q + 1), e(q) = lo + q h: found by a
//              division and then corrected by comparing x with the edges themselves, so that membership is a
//              comparison and not an arithmetic identity.  The key is the 63-bit Morton code of (qx, qy, qz),
//              or 2^63 for a body that does not count;
//   sort    -- the stable sort of nb_analysis_sort.hpp on (key, body index), all eight passes.  A cell of any
//              octree level is then a contiguous run of positions, its bodies of equal key in body order;
//   gather  -- positions and masses in sorted order; every body's outputs preset to those of a body that is
//              not counted, or of a state short of k;
//   search  -- one wave per counted body, "knn_block_queries" waves a block.  The k best (d2, j) sit one per
//              lane, ascending; a candidate that beats the k-th is inserted by a ballot and a shift.
//              (1) seed: the positions p - k .. p + k, at least k bodies, so the k-th is finite from here on;
//              (2) the body's own finest cell from its start, 64 positions a time: its bodies come in index
//                  order, so once the k-th is (0, j) with j no larger than the last index seen, nothing can
//                  beat it and the search is over (the k-zeros stop).  Coincident bodies share a cell;
//              (3) the range of finest cells per axis outside which the rule's own arithmetic on the gap to a
//                  cell edge already exceeds the k-th d2; the octree level at which that range is at most
//                  "knn_span_cells" cells an axis; each of those cells, one per lane: a lower bound of d2 from
//                  its edges, and, when the bound does not exceed the k-th d2, its run by two binary searches
//                  on key prefixes.  The runs are visited in ascending order of bound until the smallest
//                  exceeds the k-th d2 strictly; positions seen in (1) and (2) are skipped.
//              mass_in is then added over lanes 0 .. k - 2 in order, the density formed as written, and lane
//              0 stores the four results at the body's own index;
//   sums    -- over body order: the eight products of density, block_row slabs, sum_over_blocks<16>; the peak
//              by an integer maximum of the order-preserving encoding of the density, its index by an integer
//              minimum over the bodies that hold it.
// No float atomics anywhere.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "nb_analysis.hpp"
#include "nb_analysis_sort.hpp"
#include "nb_common.hpp"
#include "nb_knn.hpp"
#include "nb_sim.hpp"

namespace nb {

namespace {

constexpr uint32_t kThreads = kBlock;
constexpr uint32_t kPasses = kKnnPasses;
constexpr uint32_t kAxisMax = kKnnAxisMax;
constexpr unsigned long long kKeyNone = 1ull << 63;        // past every Morton code
constexpr uint32_t kSumFields = kKnnSumFields, kSumLive = 9;  // the eight sums and the degenerate bodies
constexpr uint32_t kFinishGroups = 16;                     // G of sum_over_blocks

// (the plan and the reduced results of a call, KnnInfo, and ordered64: nb_knn.hpp)
__host__ inline double unordered64(unsigned long long e) {
    const unsigned long long u = (e >> 63) ? (e & ~(1ull << 63)) : ~e;
    double f;
    std::memcpy(&f, &u, sizeof f);
    return f;
}

// One block: the bounds into the plan.
__global__ __launch_bounds__(kThreads) void knn_plan_kernel(const double *__restrict__ slabs, uint32_t blocks,
                                                            KnnInfo *__restrict__ info) {
    double lo[3], hi[3];
    KnnInfo o{};
    if (!bounds_finish(slabs, blocks, lo, hi, &o.n_ok)) return;
    o.peak_index = NB_KNN_NONE;
    if (o.n_ok > 0) {
        double extent = 0.0;
        for (int a = 0; a < 3; ++a) {
            o.lo[a] = lo[a];
            o.hi[a] = hi[a];
            extent = fmax(extent, o.hi[a] - o.lo[a]);  // finite: a difference of binary32 values
        }
        o.h = extent * 0x1p-21;  // exact; 0 only for a state at one point
    }
    *info = o;
}

// ---- key ------------------------------------------------------------------------------------------
// (edge, clamp_cell and the Morton code: nb_knn.hpp)

// The finest cell of x: the q in 0 .. kAxisMax with edge(q) <= x, and x < edge(q + 1) unless q is the last.
// The division proposes, the comparisons decide; lo <= x = edge(0) side always holds.  The proposal is off by
// a cell at the most (h is at least 2^8 units in the last place of any coordinate involved), so the loops are
// short; they end in any case, q moving one way inside 0 .. kAxisMax.
__device__ inline uint32_t cell_of(float xf, double lo, double h) {
    if (!(h > 0.0)) return 0u;
    const double x = xf;
    uint32_t q = clamp_cell(floor((x - lo) / h));
    while (q > 0 && x < edge(lo, h, q)) --q;
    while (q < kAxisMax && x >= edge(lo, h, q + 1)) ++q;
    return q;
}

__global__ __launch_bounds__(kThreads) void knn_key_kernel(const float4 *__restrict__ posm,
                                                           const float4 *__restrict__ vel, uint32_t n,
                                                           const KnnInfo *__restrict__ info,
                                                           unsigned long long *__restrict__ keys) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float4 p = posm[i];
    unsigned long long key = kKeyNone;
    if (body_ok(p, vel[i])) {
        const double h = info->h;
        key = morton(cell_of(p.x, info->lo[0], h), cell_of(p.y, info->lo[1], h), cell_of(p.z, info->lo[2], h));
    }
    keys[i] = key;
}

// ---- gather ---------------------------------------------------------------------------------------
// spos[p] = the body at sorted position p; body i's outputs preset: not counted, or (counted) short of k --
// the search overwrites the latter when there are more than k counted bodies
__global__ __launch_bounds__(kThreads) void knn_gather_kernel(const float4 *__restrict__ posm,
                                                              const float4 *__restrict__ vel, uint32_t n,
                                                              const KnnInfo *__restrict__ info,
                                                              const uint32_t *__restrict__ sidx,
                                                              float4 *__restrict__ spos, double *__restrict__ r2,
                                                              uint32_t *__restrict__ kth, double *__restrict__ mass_in,
                                                              double *__restrict__ density) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    if (i < info->n_ok) spos[i] = posm[sidx[i]];
    r2[i] = body_ok(posm[i], vel[i]) ? (double)INFINITY : (double)NAN;
    kth[i] = NB_KNN_NONE;
    mass_in[i] = 0.0;
    density[i] = 0.0;
}

// ---- search ---------------------------------------------------------------------------------------
// (the rule, the query and the search itself: nb_knn.hpp)
__global__ __launch_bounds__(kThreads) void knn_search_kernel(const KnnInfo *__restrict__ info,
                                                              const unsigned long long *__restrict__ keys,
                                                              const uint32_t *__restrict__ sidx,
                                                              const float4 *__restrict__ spos,
                                                              const float4 *__restrict__ posm, uint32_t k,
                                                              uint32_t span, double *__restrict__ r2,
                                                              uint32_t *__restrict__ kth, double *__restrict__ mass_in,
                                                              double *__restrict__ density) {
#pragma clang fp contract(off)
    const uint32_t c = info->n_ok;
    if (c <= k) return;  // short of k: the presets stand
    const size_t pl = (size_t)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
    if (pl >= c) return;  // (uniform over the wave)
    const uint32_t p = (uint32_t)pl;
    Query q;
    knn_search(q, info, keys, sidx, spos, c, p, k, span);

    // lane l < k holds the (l + 1)-th body of the order
    double mass, rho;
    knn_mass_density(q, posm, k, &mass, &rho);
    if (q.lane == 0) {
        const uint32_t body = sidx[p];
        r2[body] = q.kd;
        kth[body] = q.kj;
        mass_in[body] = mass;
        density[body] = rho;
    }
}

// ---- sums -----------------------------------------------------------------------------------------
// does body i enter the sums and the peak?  (*rho: its density; *degenerate: counted, r2 == 0)
__device__ inline bool summed(const KnnInfo *__restrict__ info, uint32_t k, float4 p, float4 v, double r2,
                              bool *degenerate) {
    *degenerate = false;
    if (info->n_ok <= k || !body_ok(p, v)) return false;
    *degenerate = r2 == 0.0;
    return r2 != 0.0 && isfinite(r2);
}

__global__ __launch_bounds__(kThreads) void knn_sum_kernel(const float4 *__restrict__ posm,
                                                           const float4 *__restrict__ vel, uint32_t n, uint32_t k,
                                                           KnnInfo *__restrict__ info, const double *__restrict__ r2,
                                                           const double *__restrict__ density,
                                                           double *__restrict__ slabs) {
#pragma clang fp contract(off)
    __shared__ double part[kThreads / kWave][kSumFields];
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    double t[kSumLive];
    for (uint32_t f = 0; f < kSumLive; ++f) t[f] = 0.0;
    unsigned long long peak = 0ull;
    if (i < n) {
        const float4 p = posm[i], v = vel[i];
        bool degenerate;
        if (summed(info, k, p, v, r2[i], &degenerate)) {
            const double rho = density[i];
            t[0] = rho;
            t[1] = rho * (double)p.x;
            t[2] = rho * (double)p.y;
            t[3] = rho * (double)p.z;
            t[4] = rho * (double)v.x;
            t[5] = rho * (double)v.y;
            t[6] = rho * (double)v.z;
            t[7] = rho * rho;
            if (isfinite(rho)) peak = ordered64(rho);
        }
        t[8] = degenerate ? 1.0 : 0.0;
    }
    block_row<kSumFields, kSumLive>(t, part, slabs + (size_t)blockIdx.x * kSumFields);
    for (int o = 32; o > 0; o >>= 1) peak = std::max(peak, (unsigned long long)__shfl_xor(peak, o));
    if (threadIdx.x % kWave == 0 && peak) atomicMax(&info->peak_key, peak);
}

__global__ __launch_bounds__(kThreads) void knn_finish_kernel(const double *__restrict__ slabs, uint32_t blocks,
                                                              KnnInfo *__restrict__ info) {
    constexpr uint32_t kPer = kThreads / kFinishGroups;
    static_assert(kPer == kSumFields, "one column per field");
    __shared__ double pp[kFinishGroups][kPer];
    const uint32_t tid = threadIdx.x;
    const double r = sum_over_blocks<kFinishGroups>(slabs, blocks, kSumFields, tid % kPer, pp);
    if (tid < kPer) info->sums[tid] = r;
}

// the smallest index that holds the peak
__global__ __launch_bounds__(kThreads) void knn_peak_kernel(const float4 *__restrict__ posm,
                                                            const float4 *__restrict__ vel, uint32_t n, uint32_t k,
                                                            KnnInfo *__restrict__ info, const double *__restrict__ r2,
                                                            const double *__restrict__ density) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const unsigned long long peak = info->peak_key;
    bool degenerate;
    if (!peak || !summed(info, k, posm[i], vel[i], r2[i], &degenerate)) return;
    const double rho = density[i];
    if (isfinite(rho) && ordered64(rho) == peak) atomicMin(&info->peak_index, (uint32_t)i);
}

}  // namespace


namespace {

template <class B>
int knn_reserve(B &b, size_t count) {
    if (b.reserve(std::max<size_t>(1, count)) == hipSuccess) return NB_OK;
    (void)hipGetLastError();
    set_error("knn: cannot allocate the workspace (%zu elements)", count);
    return NB_ERR_ALLOC;
}

}  // namespace

int knn_work(SimBase &sim, KnnWork **out) {
    return workspace(sim, kWorkKnn, out, [](KnnWork &f) {
        if (f.info.reserve(1) != hipSuccess || f.h_info.reserve(1) != hipSuccess) {
            (void)hipGetLastError();
            set_error("knn: cannot allocate the result workspace");
            return NB_ERR_ALLOC;
        }
        return NB_OK;
    });
}

int knn_enqueue_sorted(SimBase &sim, KnnWork &w) {
    const uint32_t n = sim.n;
    if (n > 0x7fffffffu) {
        set_error("knn: %u bodies are more than one call takes", n);
        return NB_ERR_UNSUPPORTED;
    }
    const uint32_t blocks = (n + kThreads - 1) / kThreads;
    const SortShape shape = sort_shape(n);
    if (int rc = w.sort.reserve(n, shape, [](auto &b, size_t count) { return knn_reserve(b, count); })) return rc;
    if (int rc = knn_reserve(w.slabs, (size_t)std::max(kBoundFields, kSumFields) * blocks)) return rc;
    if (int rc = knn_reserve(w.spos, n)) return rc;
    if (int rc = knn_reserve(w.r2, n)) return rc;
    if (int rc = knn_reserve(w.mass_in, n)) return rc;
    if (int rc = knn_reserve(w.density, n)) return rc;
    if (int rc = knn_reserve(w.kth, n)) return rc;

    const float4 *posm = nullptr, *vel = nullptr;
    sim.diag_state(&posm, &vel);
    KnnInfo *info = w.info;
    hipLaunchKernelGGL(bounds_kernel<>, dim3(blocks), dim3(kThreads), 0, sim.stream, posm, vel, n, w.slabs);
    NB_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(knn_plan_kernel, dim3(1), dim3(kThreads), 0, sim.stream, w.slabs, blocks, info);
    NB_HIP_TRY(hipGetLastError());
    static_assert(kPasses % 2 == 0, "the sort starts from side 0 and its result is read from there");
    unsigned long long *keys = w.sort.keys[0];
    const uint32_t *sidx = w.sort.idx[0];
    hipLaunchKernelGGL(knn_key_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, posm, vel, n, info, keys);
    NB_HIP_TRY(hipGetLastError());
    if (int rc = enqueue_sort(sim.stream, w.sort, n, shape, kPasses, 0, nullptr)) return rc;
    hipLaunchKernelGGL(knn_gather_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, posm, vel, n, info, sidx,
                       w.spos, w.r2, w.kth, w.mass_in, w.density);
    NB_HIP_TRY(hipGetLastError());
    return NB_OK;
}

int knn_enqueue(SimBase &sim, KnnWork &w, uint32_t k) {
    if (int rc = knn_enqueue_sorted(sim, w)) return rc;
    const uint32_t n = sim.n;
    const uint32_t per_block = (uint32_t)sim.knn_block_queries, span = (uint32_t)sim.knn_span_cells;
    const float4 *posm = nullptr, *vel = nullptr;
    sim.diag_state(&posm, &vel);
    const KnnInfo *info = w.info;
    const unsigned long long *keys = w.sort.keys[0];
    const uint32_t *sidx = w.sort.idx[0];
    // one wave per sorted position; those past the counted bodies, and all of them in a state short of k,
    // return at once: no host round trip decides the launch
    hipLaunchKernelGGL(knn_search_kernel, dim3((n + per_block - 1) / per_block), dim3(per_block * kWave), 0,
                       sim.stream, info, keys, sidx, w.spos, posm, k, span, w.r2, w.kth, w.mass_in, w.density);
    NB_HIP_TRY(hipGetLastError());
    return NB_OK;
}

int sim_knn(SimBase &sim, const nb_knn_params &params, double *r2, uint32_t *kth, double *mass_in, double *density,
            nb_knn_stats *stats) {
    if (int rc = analysis_begin(sim, "knn")) return rc;
    if (!r2 && !kth && !mass_in && !density && !stats) {  // nothing to measure
        NB_HIP_TRY(hipStreamSynchronize(sim.stream));
        return sim.diag_status();
    }
    const uint32_t n = sim.n, k = params.k;
    if (n > 0x7fffffffu) {
        set_error("knn: %u bodies are more than one call takes", n);
        return NB_ERR_UNSUPPORTED;
    }
    KnnWork *work = nullptr;
    if (int rc = knn_work(sim, &work)) return rc;
    KnnWork &w = *work;
    KnnInfo &res = *static_cast<KnnInfo *>(w.h_info);
    std::memset(&res, 0, sizeof res);
    res.peak_index = NB_KNN_NONE;

    if (n > 0) {
        const uint32_t blocks = (n + kThreads - 1) / kThreads;
        if (r2)
            if (int rc = knn_reserve(w.h_r2, n)) return rc;
        if (kth)
            if (int rc = knn_reserve(w.h_kth, n)) return rc;
        if (mass_in)
            if (int rc = knn_reserve(w.h_mass_in, n)) return rc;
        if (density)
            if (int rc = knn_reserve(w.h_density, n)) return rc;
        if (int rc = knn_enqueue(sim, w, k)) return rc;

        const float4 *posm = nullptr, *vel = nullptr;
        sim.diag_state(&posm, &vel);
        KnnInfo *info = w.info;
        hipLaunchKernelGGL(knn_sum_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, posm, vel, n, k, info, w.r2,
                           w.density, w.slabs);
        NB_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(knn_finish_kernel, dim3(1), dim3(kThreads), 0, sim.stream, w.slabs, blocks, info);
        NB_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(knn_peak_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, posm, vel, n, k, info, w.r2,
                           w.density);
        NB_HIP_TRY(hipGetLastError());
        NB_HIP_TRY(hipMemcpyAsync(w.h_info, info, sizeof(KnnInfo), hipMemcpyDeviceToHost, sim.stream));
        if (r2) NB_HIP_TRY(hipMemcpyAsync(w.h_r2, w.r2, sizeof(double) * n, hipMemcpyDeviceToHost, sim.stream));
        if (kth) NB_HIP_TRY(hipMemcpyAsync(w.h_kth, w.kth, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, sim.stream));
        if (mass_in)
            NB_HIP_TRY(hipMemcpyAsync(w.h_mass_in, w.mass_in, sizeof(double) * n, hipMemcpyDeviceToHost, sim.stream));
        if (density)
            NB_HIP_TRY(hipMemcpyAsync(w.h_density, w.density, sizeof(double) * n, hipMemcpyDeviceToHost, sim.stream));
    }
    NB_HIP_TRY(hipStreamSynchronize(sim.stream));
    if (int rc = sim.diag_status()) return rc;
    if (n > 0) {
        if (r2) std::memcpy(r2, w.h_r2, sizeof(double) * n);
        if (kth) std::memcpy(kth, w.h_kth, sizeof(uint32_t) * n);
        if (mass_in) std::memcpy(mass_in, w.h_mass_in, sizeof(double) * n);
        if (density) std::memcpy(density, w.h_density, sizeof(double) * n);
    }
    if (stats) {
        nb_knn_stats o{};
        o.step_num = sim.step_num;
        o.n = n;
        o.nonfinite = n - res.n_ok;
        o.counted = res.n_ok;
        o.degenerate = (uint64_t)res.sums[8];
        o.short_of_k = res.n_ok <= k ? res.n_ok : 0;
        o.sum_rho = res.sums[0];
        for (int a = 0; a < 3; ++a) {
            o.sum_rho_x[a] = res.sums[1 + a];
            o.sum_rho_v[a] = res.sums[4 + a];
        }
        o.sum_rho2 = res.sums[7];
        o.peak_index = res.peak_index;
        o.peak_density = res.peak_key ? unordered64(res.peak_key) : 0.0;
        *stats = o;
    }
    return NB_OK;
}

}  // namespace nb
