// nb_map.hip -- nb_sim_map: per-cell mass and velocity moments of a simulator's current state on a 2-D
// grid (include/nbody.h "Projected maps"; no reference counterpart).
//
// A map has up to 2^22 cells, so the per-block slab of nb_radial.hip (256 bins) does not carry over.
// The bodies are grouped by 8 x 8-cell tile instead, stably, and every tile's list is summed in LDS:
//   classify  -- one thread per body over the float4 SoA state (SimBase::diag_state): fp64, no
//                contraction, the cell by comparisons against the edges lo + i * size.  Writes one key per
//                body, (tile << 6) | cell in the tile, or the key of the tile past the last for a body
//                that is outside or non-finite.  The global sums (class counts, masses) go through
//                per-block slabs (block_row, nb_analysis.hpp) and a fixed-order finish;
//   group, lists, sum, finish -- nb_tiles.hpp, shared with nb_phase.hip: the stable sort on (key, body index),
//                the tiles' lists cut into segments of at most "map_segment_len" bodies, one block per segment
//                summing the terms below in list order, the segments of a longer list in segment order, then
//                the maximum count and the global sums in a fixed order.
// Without NB_MAP_VELOCITY only the mass is formed, staged and summed.  With NB_MAP_CENTER_COM the moments
// pass of nb_diag.hip runs first on the same stream and the threads divide its sums into the centre
// themselves: no host round trip.
// No float atomics; the grids and the cuts depend on n, the grid, the segment length and the lists'
// lengths alone: the result is bitwise reproducible.
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

constexpr uint32_t kThreads = kBlock;
constexpr uint32_t kGlobalFields = kTileGlobalFields;  // see GlobalField
constexpr uint32_t kMaxFields = 6;                     // planes with NB_MAP_VELOCITY

enum GlobalField { kGBinned = 0, kGOutside, kGBad, kGBinnedMass, kGOutsideMass, kGMass, kGLive };

struct MapConst {
    double c[3], vc[3], n[3], e1[3], e2[3];
    double xlo, xhi, ylo, yhi, dlo, dhi, dx, dy;
    uint32_t w, h, tiles_x, tiles;
    uint32_t center_com;
};

// The cell of coordinate a among `cells` cells of size d from lo, hi the last edge: the i with
// edge(i) <= a < edge(i + 1), edge(i) = lo + i * d below `cells` and hi at it.  lo <= a < hi is known.
// A division guesses, the comparisons decide.
__device__ inline uint32_t cell_of(double a, double lo, double d, uint32_t cells) {
#pragma clang fp contract(off)
    const double g = (a - lo) / d;
    uint32_t i = g >= (double)(cells - 1) ? cells - 1 : (uint32_t)g;  // (g >= 0)
    while (i > 0 && a < lo + (double)i * d) --i;
    while (i + 1 < cells && a >= lo + (double)(i + 1) * d) ++i;
    return i;
}

// One body by the rule of include/nbody.h: true when it is binned, then *key = (tile << 6) | cell in tile
__device__ inline bool classify(float4 p, const MapConst &k, const double (&c)[3], uint32_t *key) {
#pragma clang fp contract(off)
    const double dx = (double)p.x - c[0], dy = (double)p.y - c[1], dz = (double)p.z - c[2];
    const double a = (dx * k.e1[0] + dy * k.e1[1]) + dz * k.e1[2];
    const double b = (dx * k.e2[0] + dy * k.e2[1]) + dz * k.e2[2];
    const double h = (dx * k.n[0] + dy * k.n[1]) + dz * k.n[2];
    if (!(a >= k.xlo && a < k.xhi && b >= k.ylo && b < k.yhi && h >= k.dlo && h < k.dhi)) return false;
    const uint32_t i = cell_of(a, k.xlo, k.dx, k.w), j = cell_of(b, k.ylo, k.dy, k.h);
    const uint32_t tile = (j / kTile) * k.tiles_x + i / kTile;
    *key = (tile << kCellBits) | ((j % kTile) * kTile + i % kTile);
    return true;
}

// The terms of a body (the Terms of nb_tiles.hpp): F = 1 the mass, F = 6 mass, m ua, m ub, m w, (m w) w, m |u|^2
template <uint32_t kFields>
struct MapTerms {
    static constexpr uint32_t F = kFields;
    static constexpr bool kVelocity = kFields > 1;
    const MapConst &k;
    double vc[3];
    __device__ MapTerms(const MapConst &k_in, const double *__restrict__ used) : k(k_in) {
        for (int a = 0; a < 3; ++a) vc[a] = used[3 + a];
    }
    __device__ void operator()(uint32_t, float4 p, float4 v, double (&t)[F]) const {
#pragma clang fp contract(off)
        const double m = p.w;
        t[0] = m;
        if constexpr (F > 1) {
            const double ux = (double)v.x - vc[0], uy = (double)v.y - vc[1], uz = (double)v.z - vc[2];
            const double ua = (ux * k.e1[0] + uy * k.e1[1]) + uz * k.e1[2];
            const double ub = (ux * k.e2[0] + uy * k.e2[1]) + uz * k.e2[2];
            const double w = (ux * k.n[0] + uy * k.n[1]) + uz * k.n[2];
            t[1] = m * ua;
            t[2] = m * ub;
            t[3] = m * w;
            t[4] = (m * w) * w;
            t[5] = m * ((ux * ux + uy * uy) + uz * uz);
        }
    }
};

// ---- classify: keys[i] for every body, one slab of kGlobalFields doubles per block -----------------
// mom: the finished moments of nb_diag.hip (NB_MAP_CENTER_COM) or null.  Block 0 also writes the centre
// and velocity it used to used[0..6) (centre_used).
__global__ __launch_bounds__(kThreads) void map_classify_kernel(const float4 *__restrict__ posm,
                                                                const float4 *__restrict__ vel, uint32_t n,
                                                                MapConst k, const double *__restrict__ mom,
                                                                uint32_t *__restrict__ keys,
                                                                double *__restrict__ slabs, double *__restrict__ used) {
    __shared__ double part[kThreads / kWave][kGlobalFields];
    const uint32_t tid = threadIdx.x;
    double c[3], vc[3];
    centre_used(k.c, k.vc, k.center_com, mom, used, c, vc);
    double glob[kGLive];
    for (uint32_t f = 0; f < kGLive; ++f) glob[f] = 0.0;
    const size_t i = (size_t)blockIdx.x * kThreads + tid;
    if (i < n) {
        const float4 p = posm[i], v = vel[i];
        uint32_t key = k.tiles << kCellBits;  // the tile past the last: not binned
        if (!body_ok(p, v)) {
            glob[kGBad] = 1.0;
        } else {
            const double m = p.w;
            glob[kGMass] = m;
            if (classify(p, k, c, &key)) {
                glob[kGBinned] = 1.0;
                glob[kGBinnedMass] = m;
            } else {
                glob[kGOutside] = 1.0;
                glob[kGOutsideMass] = m;
            }
        }
        keys[i] = key;
    }
    block_row<kGlobalFields, kGLive>(glob, part, slabs + (size_t)blockIdx.x * kGlobalFields);
}

}  // namespace

struct MapWork : Workspace, TileWork {};

int sim_map(SimBase &sim, const nb_map_params &params, const MapPlan &plan, uint32_t *counts, double *planes,
            nb_map_stats *stats) {
    if (int rc = analysis_begin(sim, "map")) return rc;
    if (!counts && !planes && !stats) {  // nothing to measure
        NB_HIP_TRY(hipStreamSynchronize(sim.stream));
        return sim.diag_status();
    }
    MapWork *work = nullptr;
    if (int rc = workspace(sim, kWorkMap, &work, [](MapWork &f) { return tiles_init(f, "map"); })) return rc;
    MapWork &w = *work;
    const uint32_t n = sim.n, width = params.width, height = params.height;
    const bool com = (params.flags & NB_MAP_CENTER_COM) != 0, velocity = (params.flags & NB_MAP_VELOCITY) != 0;

    MapConst k{};
    for (int a = 0; a < 3; ++a) {
        k.c[a] = com ? 0.0 : params.center[a];
        k.vc[a] = com ? 0.0 : params.velocity[a];
        k.n[a] = plan.n[a];
        k.e1[a] = plan.e1[a];
        k.e2[a] = plan.e2[a];
    }
    k.xlo = params.x_range[0];
    k.xhi = params.x_range[1];
    k.ylo = params.y_range[0];
    k.yhi = params.y_range[1];
    k.dlo = params.depth_range[0];
    k.dhi = params.depth_range[1];
    k.dx = plan.dx;
    k.dy = plan.dy;
    k.w = width;
    k.h = height;
    k.tiles_x = (width + kTile - 1) / kTile;
    k.tiles = k.tiles_x * ((height + kTile - 1) / kTile);
    k.center_com = com;

    auto classify_launch = [&](uint32_t class_blocks, const float4 *posm, const float4 *vel, uint32_t *keys,
                               double *slabs, double *used) -> int {
        const double *mom = nullptr;
        if (com)
            if (int rc = diag_enqueue_moments(sim, &mom)) return rc;
        hipLaunchKernelGGL(map_classify_kernel, dim3(class_blocks), dim3(kThreads), 0, sim.stream, posm, vel, n, k, mom,
                           keys, slabs, used);
        NB_HIP_TRY(hipGetLastError());
        return NB_OK;
    };
    if (int rc = tiles_pass<MapTerms<1>, MapTerms<kMaxFields>>(sim, w, "map", k, (uint32_t)sim.map_segment_len, velocity,
                                                              com, classify_launch, counts, planes))
        return rc;
    if (int rc = sim.diag_status()) return rc;

    if (stats) {
        const double *used = w.h_res, *g = w.h_res + kTileUsed;
        nb_map_stats o{};
        o.step_num = sim.step_num;
        o.n = n;
        o.nonfinite = (uint64_t)g[kGBad];
        o.binned_count = (uint64_t)g[kGBinned];
        o.outside_count = (uint64_t)g[kGOutside];
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
        *stats = o;
    }
    return NB_OK;
}

}  // namespace nb
