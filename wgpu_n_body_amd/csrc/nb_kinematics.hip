// nb_kinematics.hip -- nb_local_kinematics_sim: the mass and velocity moments of every body's k nearest
// neighbours relative to the body, and the sums its least-squares velocity gradient is solved from
// (include/nbody.h "Local kinematics"; no reference counterpart).
//
// The neighbour list is nb_sim_knn's order, found by nb_sim_knn's search (nb_knn.hpp), one search per body:
//   plan, key, sort, gather -- knn_enqueue_sorted: nb_sim_knn's own kernels, which also preset its four arrays;
//   preset  -- every sum of a body that is not counted NaN, of a counted body 0 (what stands when c <= k);
//   search  -- one wave per counted body, "knn_block_queries" waves a block.  After knn_search lane l < k holds the
//              (l + 1)-th body of the order: mass_in and the density by knn_mass_density, as nb_sim_knn forms
//              them; then the lane gathers its neighbour's position and velocity from the state and forms the 10
//              or 25 terms of the rule, each product rounded once.  The terms go through LDS, [l][field] in a
//              slab of the wave's own, and lane f adds field f over l = 0 .. k - 1 from its start value: the
//              order of the rule, k dependent additions once instead of k per field (DESIGN.md 6s has the
//              measurement against the __shfl loop, kept under NB_KIN_SHFL_SUMS).  Lane f stores sum f.
// No float atomics: the degenerate bodies are counted by an integer atomic.
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
constexpr uint32_t kMoments = NB_KIN_MOMENTS, kGrads = NB_KIN_GRADS;

struct KinInfo {
    unsigned long long degenerate;  // counted bodies with r2 == 0
};

struct KinWork : Workspace {  // (all grow to the largest call so far)
    DeviceBuf<double> moments, grads;    // [n][10], [n][15]
    PinnedBuf<double> h_moments, h_grads;  // staged, so that a failed call leaves the outputs alone
    DeviceBuf<KinInfo> info;             // [1]
    PinnedBuf<KinInfo> h_info;           // [1]
};

template <class B>
int kin_reserve(B &b, size_t count) {
    if (b.reserve(std::max<size_t>(1, count)) == hipSuccess) return NB_OK;
    (void)hipGetLastError();
    set_error("local_kinematics: cannot allocate the workspace (%zu elements)", count);
    return NB_ERR_ALLOC;
}

// every sum of body i: NaN when it is not counted, else 0 -- the search overwrites the latter when there are more
// than k counted bodies
__global__ __launch_bounds__(kThreads) void kin_preset_kernel(const float4 *__restrict__ posm,
                                                              const float4 *__restrict__ vel, uint32_t n,
                                                              double *__restrict__ moments,
                                                              double *__restrict__ grads, KinInfo *__restrict__ kinfo) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i == 0) kinfo->degenerate = 0ull;
    if (i >= n) return;
    const double v = body_ok(posm[i], vel[i]) ? 0.0 : (double)NAN;
    if (moments)
        for (uint32_t f = 0; f < kMoments; ++f) moments[i * kMoments + f] = v;
    if (grads)
        for (uint32_t f = 0; f < kGrads; ++f) grads[i * kGrads + f] = v;
}

// kFields: 0 (the search and nb_sim_knn's four values alone), 10 (the moments) or 25 (with the gradient sums).
// Dynamic LDS: (blockDim.x / 64) slabs of k (kFields | 1) doubles -- the odd row length keeps the lanes' rows on
// different banks.
template <uint32_t kFields>
__global__ __launch_bounds__(kThreads) void kin_search_kernel(
    const KnnInfo *__restrict__ info, const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ sidx,
    const float4 *__restrict__ spos, const float4 *__restrict__ posm, const float4 *__restrict__ vel, uint32_t k,
    uint32_t span, uint32_t self, double *__restrict__ r2, uint32_t *__restrict__ kth, double *__restrict__ mass_in,
    double *__restrict__ density, double *__restrict__ moments, double *__restrict__ grads,
    KinInfo *__restrict__ kinfo) {
#pragma clang fp contract(off)
    extern __shared__ double kin_lds[];
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
    const uint32_t body = sidx[p];
    if (q.lane == 0) {
        r2[body] = q.kd;
        kth[body] = q.kj;
        mass_in[body] = mass;
        density[body] = rho;
        if (q.kd == 0.0) atomicAdd(&kinfo->degenerate, 1ull);
    }
    if constexpr (kFields > 0) {
        double t[kFields];
        for (uint32_t f = 0; f < kFields; ++f) t[f] = 0.0;
        if (q.lane < k) {  // (c > k: the list is full, q.lj is a body)
            const float4 pj = posm[q.lj], vj = vel[q.lj], vi = vel[body];
            const double m = (double)pj.w;
            const double du[3] = {(double)vj.x - (double)vi.x, (double)vj.y - (double)vi.y,
                                  (double)vj.z - (double)vi.z};
            const double mu[3] = {m * du[0], m * du[1], m * du[2]};
            t[0] = m;
            t[1] = mu[0];
            t[2] = mu[1];
            t[3] = mu[2];
            t[4] = mu[0] * du[0];
            t[5] = mu[0] * du[1];
            t[6] = mu[0] * du[2];
            t[7] = mu[1] * du[1];
            t[8] = mu[1] * du[2];
            t[9] = mu[2] * du[2];
            if constexpr (kFields > kMoments) {
                const double dx[3] = {(double)pj.x - (double)q.p.x, (double)pj.y - (double)q.p.y,
                                      (double)pj.z - (double)q.p.z};
                const double md[3] = {m * dx[0], m * dx[1], m * dx[2]};
                t[10] = md[0] * dx[0];
                t[11] = md[0] * dx[1];
                t[12] = md[0] * dx[2];
                t[13] = md[1] * dx[1];
                t[14] = md[1] * dx[2];
                t[15] = md[2] * dx[2];
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < 3; ++b) t[16 + 3 * a + b] = mu[a] * dx[b];
            }
        }
        const double start = q.lane == 0 && self ? (double)q.p.w : 0.0;  // S0 with NB_KIN_SELF; every other sum: 0
        double s = start;
#ifdef NB_KIN_SHFL_SUMS
        // the dropped variant: every field by k dependent broadcasts on all lanes
        for (uint32_t f = 0; f < kFields; ++f) {
            double a = f == 0 && self ? (double)q.p.w : 0.0;
            for (uint32_t l = 0; l < k; ++l) a += __shfl(t[f], (int)l);
            if (q.lane == f) s = a;
        }
#else
        constexpr uint32_t kRow = kFields | 1u;
        double *slab = kin_lds + (size_t)(threadIdx.x / kWave) * k * kRow;
        if (q.lane < k)
            for (uint32_t f = 0; f < kFields; ++f) slab[q.lane * kRow + f] = t[f];
        // the slab is the wave's own: a wave-level fence orders its writes before its reads
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (q.lane < kFields)
            for (uint32_t l = 0; l < k; ++l) s += slab[l * kRow + q.lane];
#endif
        if (q.lane < kMoments) {
            if (moments) moments[(size_t)body * kMoments + q.lane] = s;
        } else if (q.lane < kFields) {
            grads[(size_t)body * kGrads + (q.lane - kMoments)] = s;
        }
    }
}

}  // namespace

int sim_local_kinematics(SimBase &sim, const nb_kin_params &params, double *moments, double *grads, double *r2,
                         uint32_t *kth, double *mass_in, double *density, nb_kin_stats *stats) {
    if (int rc = analysis_begin(sim, "local_kinematics")) return rc;
    if (!moments && !grads && !r2 && !kth && !mass_in && !density && !stats) {  // nothing to measure
        NB_HIP_TRY(hipStreamSynchronize(sim.stream));
        return sim.diag_status();
    }
    const uint32_t n = sim.n, k = params.k;
    if (n > 0x7fffffffu) {
        set_error("local_kinematics: %u bodies are more than one call takes", n);
        return NB_ERR_UNSUPPORTED;
    }
    KnnWork *kwork = nullptr;
    if (int rc = knn_work(sim, &kwork)) return rc;
    KnnWork &w = *kwork;
    KinWork *work = nullptr;
    if (int rc = workspace(sim, kWorkKin, &work, [](KinWork &f) {
            if (f.info.reserve(1) != hipSuccess || f.h_info.reserve(1) != hipSuccess) {
                (void)hipGetLastError();
                set_error("local_kinematics: cannot allocate the result workspace");
                return (int)NB_ERR_ALLOC;
            }
            return (int)NB_OK;
        }))
        return rc;
    KinWork &kw = *work;
    KnnInfo &res = *static_cast<KnnInfo *>(w.h_info);
    KinInfo &kres = *static_cast<KinInfo *>(kw.h_info);
    std::memset(&res, 0, sizeof res);
    std::memset(&kres, 0, sizeof kres);

    if (n > 0) {
        const uint32_t blocks = (n + kThreads - 1) / kThreads;
        const size_t nm = (size_t)n * kMoments, ng = (size_t)n * kGrads;
        if (moments) {
            if (int rc = kin_reserve(kw.moments, nm)) return rc;
            if (int rc = kin_reserve(kw.h_moments, nm)) return rc;
        }
        if (grads) {
            if (int rc = kin_reserve(kw.grads, ng)) return rc;
            if (int rc = kin_reserve(kw.h_grads, ng)) return rc;
        }
        if (r2)
            if (int rc = kin_reserve(w.h_r2, n)) return rc;
        if (kth)
            if (int rc = kin_reserve(w.h_kth, n)) return rc;
        if (mass_in)
            if (int rc = kin_reserve(w.h_mass_in, n)) return rc;
        if (density)
            if (int rc = kin_reserve(w.h_density, n)) return rc;
        if (int rc = knn_enqueue_sorted(sim, w)) return rc;

        const float4 *posm = nullptr, *vel = nullptr;
        sim.diag_state(&posm, &vel);
        double *d_moments = moments ? (double *)kw.moments : nullptr, *d_grads = grads ? (double *)kw.grads : nullptr;
        hipLaunchKernelGGL(kin_preset_kernel, dim3(blocks), dim3(kThreads), 0, sim.stream, posm, vel, n, d_moments,
                           d_grads, (KinInfo *)kw.info);
        NB_HIP_TRY(hipGetLastError());
        // one wave per sorted position, as nb_sim_knn's search
        const uint32_t per_block = (uint32_t)sim.knn_block_queries, span = (uint32_t)sim.knn_span_cells;
        const uint32_t fields = grads ? kMoments + kGrads : moments ? kMoments : 0u;
        size_t lds = (size_t)per_block * k * (fields | 1u) * sizeof(double);  // at most 4 64 25 8 = 51,200 bytes
#ifdef NB_KIN_SHFL_SUMS
        lds = 0;
#endif
        const dim3 grid((n + per_block - 1) / per_block), block(per_block * kWave);
        const uint32_t self = params.flags & NB_KIN_SELF;
        auto launch = [&](auto kernel, size_t bytes) {
            hipLaunchKernelGGL(kernel, grid, block, bytes, sim.stream, (const KnnInfo *)w.info,
                               (const unsigned long long *)w.sort.keys[0], (const uint32_t *)w.sort.idx[0],
                               (const float4 *)w.spos, posm, vel, k, span, self, (double *)w.r2, (uint32_t *)w.kth,
                               (double *)w.mass_in, (double *)w.density, d_moments, d_grads, (KinInfo *)kw.info);
        };
        if (fields == 0) launch(kin_search_kernel<0>, 0);
        else if (fields == kMoments) launch(kin_search_kernel<kMoments>, lds);
        else launch(kin_search_kernel<kMoments + kGrads>, lds);
        NB_HIP_TRY(hipGetLastError());

        NB_HIP_TRY(hipMemcpyAsync(w.h_info, w.info, sizeof(KnnInfo), hipMemcpyDeviceToHost, sim.stream));
        NB_HIP_TRY(hipMemcpyAsync(kw.h_info, kw.info, sizeof(KinInfo), hipMemcpyDeviceToHost, sim.stream));
        if (moments)
            NB_HIP_TRY(hipMemcpyAsync(kw.h_moments, kw.moments, sizeof(double) * nm, hipMemcpyDeviceToHost, sim.stream));
        if (grads)
            NB_HIP_TRY(hipMemcpyAsync(kw.h_grads, kw.grads, sizeof(double) * ng, hipMemcpyDeviceToHost, sim.stream));
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
        if (moments) std::memcpy(moments, kw.h_moments, sizeof(double) * n * kMoments);
        if (grads) std::memcpy(grads, kw.h_grads, sizeof(double) * n * kGrads);
        if (r2) std::memcpy(r2, w.h_r2, sizeof(double) * n);
        if (kth) std::memcpy(kth, w.h_kth, sizeof(uint32_t) * n);
        if (mass_in) std::memcpy(mass_in, w.h_mass_in, sizeof(double) * n);
        if (density) std::memcpy(density, w.h_density, sizeof(double) * n);
    }
    if (stats) {
        nb_kin_stats o{};
        o.step_num = sim.step_num;
        o.n = n;
        o.nonfinite = n - res.n_ok;
        o.counted = res.n_ok;
        o.degenerate = res.n_ok > k ? kres.degenerate : 0;
        o.short_of_k = res.n_ok <= k ? res.n_ok : 0;
        o.k = k;
        o.flags = params.flags;
        *stats = o;
    }
    return NB_OK;
}

}  // namespace nb
