// nb_diag.hip -- nb_sim_diagnostics: conserved-quantity monitor of a simulator's current state
// (include/nbody.h "Diagnostics"; no reference counterpart).
//
// Two passes over the float4 SoA state the simulator hands out (SimBase::diag_state), then one
// fixed-order finish:
//   moments  -- one streaming pass over posm and vel (32 B per body): each body's terms in fp64,
//               reduced per wave and per block (block_row, nb_analysis.hpp) into one 16-double slab per block;
//   pairs    -- W = sum_{i<j} m_i m_j psi(r_ij) over the upper triangle of 256 x 256 tiles: a block
//               owns one i-tile and a chunk of j-tiles at or right of the diagonal, stages every
//               j-tile through LDS, evaluates psi in fp32, folds each row's fp32 run of 64 pairs into
//               fp64, and writes one double per block.  The i-tiles go in row bands, one launch per
//               band, each bounded in pairs so that no launch runs for long on a shared GPU;
//   finish   -- one block sums the slabs in a fixed order (the moments by sum_over_blocks in 16 groups)
//               and writes 16 doubles, copied once into pinned host memory ahead of the one synchronisation.
// No float atomics: the grid shapes depend on n alone, so the result is bitwise reproducible.
#include <cmath>
#include <cstring>

#include "nb_analysis.hpp"
#include "nb_common.hpp"
#include "nb_psi.hpp"
#include "nb_sim.hpp"

namespace nb {

namespace {

constexpr uint32_t kDiagThreads = kBlock;  // both passes: 4 waves per block
constexpr uint32_t kMomMaxBlocks = 1024; // moments grid cap (grid-stride beyond)
constexpr uint32_t kMomFields = 16;      // per-block slab: see MomField
constexpr uint32_t kPairTile = 256;      // bodies per i-tile and per j-tile
constexpr uint32_t kPairRun = 64;        // pairs summed in fp32 before folding into fp64
constexpr uint32_t kPairChunks = 128;    // at most this many j-chunks per i-tile (slab count <= 128 T)
// pairs per launch of the pair pass.  Measured at 2^20 bodies: 1.3-1.9e12 pairs/s in
// the long rows, ~2.4x slower per pair in the short rows at the end of the triangle; 2^35 pairs keeps
// every launch near or under ~45 ms.  A 4 M-body potential is ~230 launches.
constexpr uint64_t kPairsPerLaunch = 1ull << 35;

enum MomField { kM = kDiagResMass, kMX = kDiagResMX, kMV = kDiagResMV, kL = 7, kK = 10, kVmax = 11, kBad = kDiagResBad, kW = 13 };

constexpr uint32_t kMomMax = 1u << kVmax;  // the one field reduced by fmax

// ---- moments: one slab of kMomFields doubles per block -------------------------------------
__global__ __launch_bounds__(kDiagThreads) void diag_moments_kernel(const float4 *__restrict__ posm,
                                                                    const float4 *__restrict__ vel, uint32_t n,
                                                                    double *__restrict__ slabs) {
    double acc[kBad + 1];
    for (int k = 0; k <= kBad; ++k) acc[k] = 0.0;
    for (uint32_t i = blockIdx.x * kDiagThreads + threadIdx.x; i < n; i += gridDim.x * kDiagThreads) {
        const float4 p = posm[i], v = vel[i];
        if (!body_ok(p, v)) {
            acc[kBad] += 1.0;
            continue;
        }
        const double m = p.w, x = p.x, y = p.y, z = p.z, vx = v.x, vy = v.y, vz = v.z;
        acc[kM] += m;
        acc[kMX + 0] += m * x;
        acc[kMX + 1] += m * y;
        acc[kMX + 2] += m * z;
        acc[kMV + 0] += m * vx;
        acc[kMV + 1] += m * vy;
        acc[kMV + 2] += m * vz;
        acc[kL + 0] += m * (y * vz - z * vy);
        acc[kL + 1] += m * (z * vx - x * vz);
        acc[kL + 2] += m * (x * vy - y * vx);
        const double v2 = vx * vx + vy * vy + vz * vz;
        acc[kK] += 0.5 * m * v2;
        acc[kVmax] = fmax(acc[kVmax], sqrt(v2));
    }
    __shared__ double part[kDiagThreads / kWave][kMomFields];
    block_row<kMomFields, kBad + 1, kMomMax>(acc, part, slabs + (size_t)blockIdx.x * kMomFields);
}

// one i body against the 256 staged j bodies: fp32 runs of kPairRun pairs, folded into fp64
template <bool kDiag, bool kMaskMassless>
__device__ inline double tile_row(const float4 *tile, float4 pi, uint32_t tid, const PsiConst &c) {
    double row = 0.0;
    for (uint32_t k0 = 0; k0 < kPairTile; k0 += kPairRun) {
        float run = 0.f;
#pragma unroll 8
        for (uint32_t k = k0; k < k0 + kPairRun; ++k) {
            const float4 q = tile[k];
            const float dx = q.x - pi.x, dy = q.y - pi.y, dz = q.z - pi.z;
            const float r2 = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
            float term = q.w * psi_f32(r2, c);
            if (kMaskMassless && q.w == 0.f) term = 0.f;
            if (kDiag && k <= tid) term = 0.f;
            run += term;
        }
        row += (double)run;
    }
    return row;
}

// ---- pairs: block (c, y) = i-tile t0 + y against j-tiles [max(t, c cj), min(T, (c + 1) cj)) ----
// One double per block at slabs[(t0 + y) * gridDim.x + c]; blocks left of the diagonal write 0.
// kMaskMassless (e = 0 only): a massless j at distance 0 would give 0 * inf; skip such terms.
template <bool kMaskMassless>
__global__ __launch_bounds__(kDiagThreads) void diag_pairs_kernel(const float4 *__restrict__ posm,
                                                                  const float4 *__restrict__ vel, uint32_t n,
                                                                  uint32_t n_tiles, uint32_t t0, uint32_t cj,
                                                                  PsiConst c, double *__restrict__ slabs) {
    const uint32_t t = t0 + blockIdx.y;
    const uint32_t j_begin = max(t, blockIdx.x * cj), j_end = min(n_tiles, (blockIdx.x + 1) * cj);
    double *out = slabs + (size_t)t * gridDim.x + blockIdx.x;
    if (j_begin >= j_end) {  // uniform across the block
        if (threadIdx.x == 0) *out = 0.0;
        return;
    }
    __shared__ float4 tile[kPairTile];
    __shared__ double part[kDiagThreads / kWave];
    const uint32_t tid = threadIdx.x, i = t * kPairTile + tid;
    float4 pi = make_float4(0.f, 0.f, 0.f, 0.f);
    bool ok_i = false;
    if (i < n) {
        pi = posm[i];
        ok_i = body_ok(pi, vel[i]);
    }
    double row = 0.0;
    for (uint32_t jt = j_begin; jt < j_end; ++jt) {
        const uint32_t j = jt * kPairTile + tid;
        float4 pj = make_float4(0.f, 0.f, 0.f, 0.f);  // absent or non-finite: massless at the origin
        if (j < n) {
            const float4 q = posm[j];
            if (body_ok(q, vel[j])) pj = q;
        }
        __syncthreads();  // the previous tile has been read
        tile[tid] = pj;
        __syncthreads();
        // only j > i inside the diagonal tile
        row += jt == t ? tile_row<true, kMaskMassless>(tile, pi, tid, c) : tile_row<false, kMaskMassless>(tile, pi, tid, c);
    }
    // a massless row is 0 (not 0 * inf); an excluded row adds nothing
    double w = ok_i && pi.w != 0.f ? (double)pi.w * row : 0.0;
    w = wave_sum(w);
    if (tid % kWave == 0) part[tid / kWave] = w;
    __syncthreads();
    if (tid == 0) {
        double s = part[0];
        for (uint32_t k = 1; k < kDiagThreads / kWave; ++k) s += part[k];
        *out = s;
    }
}

// ---- finish: fixed-order sums of every slab -> res[kMomFields] ------------------------------
// the moments by sum_over_blocks in 16 groups.  The pair slabs: thread k sums k, k + 256, ...; then 256
// partials in order.
__global__ __launch_bounds__(kDiagThreads) void diag_finish_kernel(const double *__restrict__ mom, uint32_t mom_blocks,
                                                                   const double *__restrict__ pairs,
                                                                   uint32_t pair_slabs, double *__restrict__ res) {
    constexpr uint32_t kGroups = kDiagThreads / kMomFields;
    __shared__ double mp[kGroups][kMomFields];
    __shared__ double pp[kDiagThreads];
    const uint32_t tid = threadIdx.x;
    double w = 0.0;
    for (uint32_t k = tid; k < pair_slabs; k += kDiagThreads) w += pairs[k];
    pp[tid] = w;
    const double m = sum_over_blocks<kGroups, kMomMax>(mom, mom_blocks, kMomFields, tid % kMomFields, mp);
    if (tid < kMomFields) {
        if (tid != kW) res[tid] = m;
    } else if (tid == kDiagThreads - 1) {
        double r = 0.0;
        for (uint32_t k = 0; k < kDiagThreads; ++k) r += pp[k];
        res[kW] = r;
    }
}

}  // namespace

struct DiagWork : Workspace {
    DeviceBuf<double> mom;    // [kMomMaxBlocks][kMomFields]
    DeviceBuf<double> pairs;  // the pair slabs of the largest call so far
    DeviceBuf<double> res;    // [kMomFields]
    PinnedBuf<double> h_res;  // as res
};

// the workspace of the moments pass, allocated by the first call that needs it
static int diag_work(SimBase &sim, DiagWork **w) {
    return workspace(sim, kWorkDiag, w, [](DiagWork &f) {
        NB_HIP_TRY(f.mom.reserve(kMomMaxBlocks * kMomFields));
        NB_HIP_TRY(f.res.reserve(kMomFields));
        NB_HIP_TRY(f.h_res.reserve(kMomFields));
        return NB_OK;
    });
}

static int launch_moments(SimBase &sim, DiagWork &w, uint32_t *mom_blocks) {
    const float4 *posm = nullptr, *vel = nullptr;
    sim.diag_state(&posm, &vel);
    *mom_blocks = std::min(kMomMaxBlocks, (sim.n + 4 * kDiagThreads - 1) / (4 * kDiagThreads));
    hipLaunchKernelGGL(diag_moments_kernel, dim3(*mom_blocks), dim3(kDiagThreads), 0, sim.stream, posm, vel, sim.n,
                       w.mom);
    NB_HIP_TRY(hipGetLastError());
    return NB_OK;
}

int diag_enqueue_moments(SimBase &sim, const double **res_dev) {
    DiagWork *w = nullptr;
    if (int rc = diag_work(sim, &w)) return rc;
    uint32_t mom_blocks = 0;
    if (int rc = launch_moments(sim, *w, &mom_blocks)) return rc;
    hipLaunchKernelGGL(diag_finish_kernel, dim3(1), dim3(kDiagThreads), 0, sim.stream, w->mom, mom_blocks,
                       w->pairs, 0u, w->res);
    NB_HIP_TRY(hipGetLastError());
    *res_dev = w->res;
    return NB_OK;
}

int sim_diagnostics(SimBase &sim, uint32_t flags, nb_diagnostics *out) {
    const bool potential = (flags & NB_DIAG_POTENTIAL) != 0;
    if (int rc = refuse_sharded(sim, "diagnostics")) return rc;
    const float e = sim.params.e;
    if (potential && !(e >= 0.f)) {
        set_error("diagnostics: the pair potential needs e >= 0 (e = %g)", (double)e);
        return NB_ERR_INVALID;
    }
    if (int rc = sim.bind_device()) return rc;
    DiagWork *work = nullptr;
    if (int rc = diag_work(sim, &work)) return rc;
    DiagWork &w = *work;
    const uint32_t n = sim.n;
    const float4 *posm = nullptr, *vel = nullptr;
    sim.diag_state(&posm, &vel);

    const uint32_t n_tiles = (n + kPairTile - 1) / kPairTile;
    const uint32_t cj = std::max(1u, (n_tiles + kPairChunks - 1) / kPairChunks);  // j-tiles per block
    const uint32_t chunks = (n_tiles + cj - 1) / cj;
    const size_t pair_slabs = potential ? (size_t)n_tiles * chunks : 0;
    NB_HIP_TRY(w.pairs.reserve(pair_slabs));

    double r[kMomFields] = {};
    if (n > 0) {
        uint32_t mom_blocks = 0;
        if (int rc = launch_moments(sim, w, &mom_blocks)) return rc;
        if (potential) {
            const PsiConst c = psi_const(e);
            // row bands: i-tile t meets (n_tiles - t) j-tiles; a band ends before it exceeds the budget
            const uint64_t tile_pairs = (uint64_t)kPairTile * kPairTile;
            for (uint32_t t0 = 0; t0 < n_tiles;) {
                uint32_t t1 = t0;
                uint64_t pairs = 0;
                do {
                    pairs += (uint64_t)(n_tiles - t1) * tile_pairs;
                    ++t1;
                } while (t1 < n_tiles && pairs + (uint64_t)(n_tiles - t1) * tile_pairs <= kPairsPerLaunch);
                const dim3 grid(chunks, t1 - t0);
                if (e == 0.f)
                    hipLaunchKernelGGL(diag_pairs_kernel<true>, grid, dim3(kDiagThreads), 0, sim.stream, posm, vel, n,
                                       n_tiles, t0, cj, c, w.pairs);
                else
                    hipLaunchKernelGGL(diag_pairs_kernel<false>, grid, dim3(kDiagThreads), 0, sim.stream, posm, vel,
                                       n, n_tiles, t0, cj, c, w.pairs);
                NB_HIP_TRY(hipGetLastError());
                t0 = t1;
            }
        }
        hipLaunchKernelGGL(diag_finish_kernel, dim3(1), dim3(kDiagThreads), 0, sim.stream, w.mom, mom_blocks,
                           w.pairs, (uint32_t)pair_slabs, w.res);
        NB_HIP_TRY(hipGetLastError());
        NB_HIP_TRY(hipMemcpyAsync(w.h_res, w.res, sizeof(double) * kMomFields, hipMemcpyDeviceToHost, sim.stream));
        NB_HIP_TRY(hipStreamSynchronize(sim.stream));
        std::memcpy(r, w.h_res, sizeof r);
    } else {
        NB_HIP_TRY(hipStreamSynchronize(sim.stream));
    }
    if (int rc = sim.diag_status()) return rc;

    nb_diagnostics d{};
    d.step_num = sim.step_num;
    d.n = n;
    d.nonfinite = (uint64_t)r[kBad];
    d.mass = r[kM];
    for (int k = 0; k < 3; ++k) {
        d.com[k] = r[kMX + k] / r[kM];
        d.momentum[k] = r[kMV + k];
        d.angular_momentum[k] = r[kL + k];
    }
    d.kinetic = r[kK];
    d.max_speed = r[kVmax];
    d.flags = NB_DIAG_MOMENTS | (potential ? NB_DIAG_POTENTIAL : 0u);
    if (potential) {
        d.pair_sum = r[kW];
        d.potential = -(double)sim.params.g * (double)sim.params.dt * d.pair_sum;
        d.total = d.kinetic + d.potential;
    } else {
        d.pair_sum = d.potential = d.total = std::nan("");
    }
    *out = d;
    return NB_OK;
}

}  // namespace nb
