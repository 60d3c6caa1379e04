// nb_phase.hip -- nb_phase_map_sim: the bodies of a simulator's current state binned on any two per-body
// quantities, a third summed per cell (include/nbody.h "Phase maps"; no reference counterpart).
//
//   classify  -- one thread per body over the float4 SoA state (SimBase::diag_state): fp64, no contraction.
//                Evaluates the two quantities (and, with NB_PHASE_WEIGHT, the third, only to tell whether it
//                is finite), finds the cell by a binary search in the caller's edges -- comparisons alone
//                decide -- and writes one key per body, (tile << 6) | cell in the tile, or the key of the tile
//                past the last for a body that is outside, undefined or non-finite.  The global sums (class
//                counts, masses) go through per-block slabs (block_row) and a fixed-order finish.  The edges
//                are read where the caller's upload left them, through the caches (staging them in LDS per
//                block was measured and dropped);
//   group, lists, sum, finish -- nb_tiles.hpp, the code nb_map.hip runs: the stable sort on (key, body index),
//                the tiles' lists cut into segments of at most "phase_segment_len" bodies, one block per
//                segment summing the terms below in list order, the segments in segment order.
// Without NB_PHASE_WEIGHT only the mass is formed, staged and summed.  With NB_PHASE_CENTER_COM the moments
// pass of nb_diag.hip runs first on the same stream: no host round trip.  No float atomics: the result is
// bitwise reproducible.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "nb_analysis.hpp"
#include "nb_analysis_sort.hpp"
#include "nb_common.hpp"
#include "nb_sim.hpp"
#include "nb_tiles.hpp"

namespace nb {

namespace {

constexpr uint32_t kGlobalFields = kTileGlobalFields;  // see GlobalField
constexpr uint32_t kWeightFields = 3;                  // planes with NB_PHASE_WEIGHT: mu, mu q, (mu q) q

enum GlobalField { kGBinned = 0, kGOutside, kGBad, kGBinnedMass, kGOutsideMass, kGMass, kGUndefined, kGLive };

struct PhaseConst {
    double c[3], vc[3], n[3], e1[3], e2[3];
    const double *xe, *ye;  // [w + 1], [h + 1] on the device
    const double *values;   // [n] on the device, or null
    uint32_t w, h, tiles_x, tiles;
    uint32_t center_com, qx, qy, qw, weight;
};

// Quantity `id` of the body with d = x - c, u = v - v_c, mass mu and index i, by the rule of include/nbody.h
__device__ inline double quantity(uint32_t id, const PhaseConst &k, const double (&d)[3], const double (&u)[3],
                                  double mu, size_t i) {
#pragma clang fp contract(off)
    const double dx = d[0], dy = d[1], dz = d[2], ux = u[0], uy = u[1], uz = u[2];
    auto along = [](double x, double y, double z, const double (&e)[3]) { return (x * e[0] + y * e[1]) + z * e[2]; };
    switch (id) {
        case NB_PHASE_Q_A: return along(dx, dy, dz, k.e1);
        case NB_PHASE_Q_B: return along(dx, dy, dz, k.e2);
        case NB_PHASE_Q_H: return along(dx, dy, dz, k.n);
        case NB_PHASE_Q_UA: return along(ux, uy, uz, k.e1);
        case NB_PHASE_Q_UB: return along(ux, uy, uz, k.e2);
        case NB_PHASE_Q_W: return along(ux, uy, uz, k.n);
        case NB_PHASE_Q_R_CYL:
        case NB_PHASE_Q_U_R_CYL:
        case NB_PHASE_Q_U_PHI:
        case NB_PHASE_Q_J_Z: {
            const double a = along(dx, dy, dz, k.e1), b = along(dx, dy, dz, k.e2);
            if (id == NB_PHASE_Q_R_CYL) return sqrt(a * a + b * b);
            const double ua = along(ux, uy, uz, k.e1), ub = along(ux, uy, uz, k.e2);
            if (id == NB_PHASE_Q_J_Z) return a * ub - b * ua;
            const double R = sqrt(a * a + b * b);
            return id == NB_PHASE_Q_U_R_CYL ? (a * ua + b * ub) / R : (a * ub - b * ua) / R;
        }
        case NB_PHASE_Q_R: return sqrt((dx * dx + dy * dy) + dz * dz);
        case NB_PHASE_Q_U_R:
        case NB_PHASE_Q_U_T: {
            const double r = sqrt((dx * dx + dy * dy) + dz * dz);
            const double ur = ((dx * ux + dy * uy) + dz * uz) / r;
            if (id == NB_PHASE_Q_U_R) return ur;
            double t = ((ux * ux + uy * uy) + uz * uz) - ur * ur;
            if (t < 0.0) t = 0.0;
            return sqrt(t);
        }
        case NB_PHASE_Q_SPEED: return sqrt((ux * ux + uy * uy) + uz * uz);
        case NB_PHASE_Q_J: {
            const double jx = dy * uz - dz * uy, jy = dz * ux - dx * uz, jz = dx * uy - dy * ux;
            return sqrt((jx * jx + jy * jy) + jz * jz);
        }
        case NB_PHASE_Q_E_KIN: return 0.5 * ((ux * ux + uy * uy) + uz * uz);
        case NB_PHASE_Q_MASS: return mu;
        default: return k.values[i];  // NB_PHASE_Q_VALUE (the ids were checked on the host)
    }
}

// The cell of x among `cells` cells with edges e[0 .. cells]: the i with e[i] <= x < e[i + 1], false when there
// is none.  The search keeps e[lo] <= x < e[hi]: every step is one comparison against an edge.
__device__ inline bool cell_of(const double *e, uint32_t cells, double x, uint32_t *out) {
    if (!(x >= e[0] && x < e[cells])) return false;
    uint32_t lo = 0, hi = cells;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (x >= e[mid]) lo = mid;
        else hi = mid;
    }
    *out = lo;
    return true;
}

__device__ inline void frame_of(float4 p, float4 v, const double (&c)[3], const double (&vc)[3], double (&d)[3],
                                double (&u)[3]) {
#pragma clang fp contract(off)
    d[0] = (double)p.x - c[0];
    d[1] = (double)p.y - c[1];
    d[2] = (double)p.z - c[2];
    u[0] = (double)v.x - vc[0];
    u[1] = (double)v.y - vc[1];
    u[2] = (double)v.z - vc[2];
}

// The terms of a body (the Terms of nb_tiles.hpp): F = 1 the mass, F = 3 mu, mu q, (mu q) q
template <uint32_t kFields>
struct PhaseTerms {
    static constexpr uint32_t F = kFields;
    static constexpr bool kVelocity = kFields > 1;
    const PhaseConst &k;
    double c[3], vc[3];
    __device__ PhaseTerms(const PhaseConst &k_in, const double *__restrict__ used) : k(k_in) {
        for (int a = 0; a < 3; ++a) {
            c[a] = used[a];
            vc[a] = used[3 + a];
        }
    }
    __device__ void operator()(uint32_t body, float4 p, float4 v, double (&t)[F]) const {
#pragma clang fp contract(off)
        const double mu = p.w;
        t[0] = mu;
        if constexpr (F > 1) {
            double d[3], u[3];
            frame_of(p, v, c, vc, d, u);
            const double q = quantity(k.qw, k, d, u, mu, body);
            t[1] = mu * q;
            t[2] = (mu * q) * q;
        }
    }
};

// ---- classify: keys[i] for every body, one slab of kGlobalFields doubles per block -----------------
// mom: the finished moments of nb_diag.hip (NB_PHASE_CENTER_COM) or null.  Block 0 also writes the centre
// and velocity it used to used[0..6) (centre_used).
__global__ __launch_bounds__(kBlock) void phase_classify_kernel(const float4 *__restrict__ posm,
                                                                const float4 *__restrict__ vel, uint32_t n,
                                                                PhaseConst k, const double *__restrict__ mom,
                                                                uint32_t *__restrict__ keys,
                                                                double *__restrict__ slabs, double *__restrict__ used) {
    __shared__ double part[kBlock / kWave][kGlobalFields];
    const uint32_t tid = threadIdx.x;
    const double *__restrict__ xe = k.xe, *__restrict__ ye = k.ye;
    double c[3], vc[3];
    centre_used(k.c, k.vc, k.center_com, mom, used, c, vc);
    double glob[kGLive];
    for (uint32_t f = 0; f < kGLive; ++f) glob[f] = 0.0;
    const size_t i = (size_t)blockIdx.x * kBlock + tid;
    if (i < n) {
        const float4 p = posm[i], v = vel[i];
        uint32_t key = k.tiles << kCellBits;  // the tile past the last: not binned
        if (!body_ok(p, v)) {
            glob[kGBad] = 1.0;
        } else {
            const double mu = p.w;
            glob[kGMass] = mu;
            double d[3], u[3];
            frame_of(p, v, c, vc, d, u);
            const double x = quantity(k.qx, k, d, u, mu, i), y = quantity(k.qy, k, d, u, mu, i);
            bool defined = isfinite(x) && isfinite(y);
            if (defined && k.weight) defined = isfinite(quantity(k.qw, k, d, u, mu, i));
            uint32_t ci = 0, cj = 0;
            if (defined && cell_of(xe, k.w, x, &ci) && cell_of(ye, k.h, y, &cj)) {
                const uint32_t tile = (cj / kTile) * k.tiles_x + ci / kTile;
                key = (tile << kCellBits) | ((cj % kTile) * kTile + ci % kTile);
                glob[kGBinned] = 1.0;
                glob[kGBinnedMass] = mu;
            } else {
                glob[kGOutside] = 1.0;
                glob[kGOutsideMass] = mu;
                if (!defined) glob[kGUndefined] = 1.0;
            }
        }
        keys[i] = key;
    }
    block_row<kGlobalFields, kGLive>(glob, part, slabs + (size_t)blockIdx.x * kGlobalFields);
}

}  // namespace

struct PhaseWork : Workspace, TileWork {
    DeviceBuf<double> edges;    // [w + 1 + h + 1]: x_edges, then y_edges
    PinnedBuf<double> h_edges;  // as edges
    DeviceBuf<double> values;   // [n]
    PinnedBuf<double> h_values;
};

int sim_phase_map(SimBase &sim, const nb_phase_params &params, const PhasePlan &plan, uint32_t *counts, double *planes,
                  nb_phase_stats *stats) {
    if (int rc = analysis_begin(sim, "phase_map")) return rc;
    if (!counts && !planes && !stats) {  // nothing to measure
        NB_HIP_TRY(hipStreamSynchronize(sim.stream));
        return sim.diag_status();
    }
    PhaseWork *work = nullptr;
    if (int rc = workspace(sim, kWorkPhase, &work, [](PhaseWork &f) { return tiles_init(f, "phase_map"); })) return rc;
    PhaseWork &w = *work;
    const uint32_t n = sim.n, width = params.width, height = params.height;
    const bool com = (params.flags & NB_PHASE_CENTER_COM) != 0, weight = (params.flags & NB_PHASE_WEIGHT) != 0;

    PhaseConst k{};
    for (int a = 0; a < 3; ++a) {
        k.c[a] = com ? 0.0 : params.center[a];
        k.vc[a] = com ? 0.0 : params.velocity[a];
        k.n[a] = plan.n[a];
        k.e1[a] = plan.e1[a];
        k.e2[a] = plan.e2[a];
    }
    k.w = width;
    k.h = height;
    k.tiles_x = (width + kTile - 1) / kTile;
    k.tiles = k.tiles_x * ((height + kTile - 1) / kTile);
    k.center_com = com;
    k.qx = params.x;
    k.qy = params.y;
    k.qw = params.q;
    k.weight = weight;

    if (n > 0) {  // the caller's arrays, staged through pinned memory and uploaded ahead of the kernels
        const size_t ne = (size_t)width + height + 2;
        if (int rc = tiles_reserve("phase_map", w.edges, ne)) return rc;
        if (int rc = tiles_reserve("phase_map", w.h_edges, ne)) return rc;
        std::memcpy(w.h_edges, params.x_edges, sizeof(double) * (width + 1));
        std::memcpy(w.h_edges + width + 1, params.y_edges, sizeof(double) * (height + 1));
        NB_HIP_TRY(hipMemcpyAsync(w.edges, w.h_edges, sizeof(double) * ne, hipMemcpyHostToDevice, sim.stream));
        k.xe = w.edges;
        k.ye = w.edges + width + 1;
        if (plan.uses_values) {
            if (int rc = tiles_reserve("phase_map", w.values, n)) return rc;
            if (int rc = tiles_reserve("phase_map", w.h_values, n)) return rc;
            std::memcpy(w.h_values, params.values, sizeof(double) * n);
            NB_HIP_TRY(hipMemcpyAsync(w.values, w.h_values, sizeof(double) * n, hipMemcpyHostToDevice, sim.stream));
            k.values = w.values;
        }
    }
    auto classify_launch = [&](uint32_t class_blocks, const float4 *posm, const float4 *vel, uint32_t *keys,
                               double *slabs, double *used) -> int {
        const double *mom = nullptr;
        if (com)
            if (int rc = diag_enqueue_moments(sim, &mom)) return rc;
        hipLaunchKernelGGL(phase_classify_kernel, dim3(class_blocks), dim3(kBlock), 0, sim.stream, posm, vel, n, k, mom,
                           keys, slabs, used);
        NB_HIP_TRY(hipGetLastError());
        return NB_OK;
    };
    if (int rc = tiles_pass<PhaseTerms<1>, PhaseTerms<kWeightFields>>(sim, w, "phase_map", k,
                                                                     (uint32_t)sim.phase_segment_len, weight, com,
                                                                     classify_launch, counts, planes))
        return rc;
    if (int rc = sim.diag_status()) return rc;

    if (stats) {
        const double *used = w.h_res, *g = w.h_res + kTileUsed;
        nb_phase_stats o{};
        o.step_num = sim.step_num;
        o.n = n;
        o.nonfinite = (uint64_t)g[kGBad];
        o.binned_count = (uint64_t)g[kGBinned];
        o.outside_count = (uint64_t)g[kGOutside];
        o.undefined_count = (uint64_t)g[kGUndefined];
        o.binned_mass = g[kGBinnedMass];
        o.outside_mass = g[kGOutsideMass];
        o.mass = g[kGMass];
        for (int a = 0; a < 3; ++a) {
            o.center[a] = used[a];
            o.velocity[a] = used[3 + a];
            o.n_hat[a] = plan.n[a];
            o.e1[a] = plan.e1[a];
            o.e2[a] = plan.e2[a];
        }
        o.width = width;
        o.height = height;
        o.flags = params.flags;
        o.max_count = (uint32_t)w.h_res[kTileResMax];
        o.x = params.x;
        o.y = params.y;
        o.q = params.q;
        *stats = o;
    }
    return NB_OK;
}

}  // namespace nb
