// nb_probe.hpp -- what the probes of a simulator's current state at arbitrary points share (nb_field.hip: the
// acceleration and the potential; nb_tidal.hip: the tidal tensor; nb_stability.hip: the
// acceleration and the tensor in one pass): M points against
// the N bodies of the float4 SoA state the simulator hands out (SimBase::diag_state), summed pair by pair.
//   pairs   -- probe_kernel: a block of 256 threads owns a tile of 64 IB points, IB per lane in VGPRs, the same
//              points in each of its four waves.  blockIdx.y cuts the bodies into chunks of 256-body tiles; the
//              block stages each tile through LDS (double-buffered, one barrier per tile) with the diagnostics'
//              predicate applied on load -- an absent or non-finite body is massless at the origin -- and wave w
//              reads back bodies [64 w, 64 w + 64) of the tile as wave-uniform broadcasts: one fp32 run of 64
//              pairs per point and sum, by the unit's Rule, folded into the wave's fp64 sums.  At the end the four
//              waves' sums meet in LDS in wave order and the block writes its sums and a coincident count per
//              point into slab[chunk][field][point of the band];
//   host    -- run: the plan, the workspace, and the sequence of a call.  The point tiles go in bands, one pair
//              launch per band, each bounded in pairs so that no launch runs for long on a shared GPU; after each
//              band the unit's finish kernel adds the chunks in order and writes the samples, which are copied
//              once into pinned host memory ahead of the one synchronisation.
// A unit supplies the Rule (the per-pair arithmetic and its sums), the finish kernel and the points per lane.
// What is here only adds in fp64, counts, and forms the one explicit fma of at_origin: there is nothing to
// contract, so it is the same arithmetic in nb_tidal.hip, built with -ffp-contract=off, and in nb_field.hip,
// built without.  The pair arithmetic stays in its unit, whose contraction setting is part of its specification.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>

#include "nb_analysis.hpp"
#include "nb_common.hpp"
#include "nb_sim.hpp"

namespace nb {
namespace probe {

constexpr uint32_t kThreads = 256;      // 4 waves per block
constexpr uint32_t kWaves = kThreads / kWave;
constexpr uint32_t kTile = 256;         // bodies per staged tile: one run of kRun per wave
constexpr uint32_t kRun = kTile / kWaves;  // pairs summed in fp32 before folding into fp64 (R = 64)
constexpr uint32_t kBlocks = 1024;      // with few point tiles, chunks enough for this many blocks (4 per CU)
// pairs per launch by default, and what the chunking is always sized for: the budget the diagnostics' pair pass
// was measured for (nb_diag.hip), the default of "field_launch_pairs_log2"
constexpr uint64_t kPairsPerLaunch = 1ull << 35;
static_assert(kRun == 64, "the stated error bounds are for runs of 64");

// ---- pairs: block (x, y) = point tile tile0 + x against body tiles [y cj, min(n_tiles, (y + 1) cj)) ----
// Point k of lane l of the tile is tile * 64 IB + 64 k + l.  The slab holds one band of Rule::kSums + 1 fields, the
// coincident count last: slab[(y * fields + f) * stride + (point - tile0 * 64 IB)]; of the sums only those with
// Rule::writes(f) are written.  A Rule has
//   kSums, Const                                             -- the fp64 sums per point; what the arithmetic needs
//   static constexpr bool writes(int f)                      -- whether sum f is this instantiation's to write
//   run_pairs<IB>(run, px, py, pz, c, sum, cnt)              -- one tile of bodies for one wave: bodies [0, kRun)
//                                                               of `run` against the lane's IB points
template <class Rule, int IB>
__global__ __launch_bounds__(kThreads) void probe_kernel(const float4 *__restrict__ posm,
                                                         const float4 *__restrict__ vel, uint32_t n,
                                                         uint32_t n_tiles, uint32_t cj,
                                                         const float4 *__restrict__ pts, uint32_t m, uint32_t stride,
                                                         uint32_t tile0, typename Rule::Const c,
                                                         double *__restrict__ slab) {
    constexpr int kSums = Rule::kSums;
    constexpr uint32_t kSlabFields = kSums + 1;
    __shared__ float4 tile[2][kTile];
    __shared__ double red[IB][kSlabFields][kWave];
    const uint32_t tid = threadIdx.x, lane = tid % kWave;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    const uint32_t p0 = (tile0 + blockIdx.x) * (kWave * IB) + lane;
    const uint32_t j_begin = blockIdx.y * cj, j_end = min(n_tiles, j_begin + cj);  // (never empty: see the plan)

    float px[IB], py[IB], pz[IB];
    bool at_origin[IB];  // the point coincides with the bodies masked to the origin
    uint32_t cnt[IB];
    double sum[IB][kSums];
#pragma unroll
    for (int k = 0; k < IB; ++k) {
        const uint32_t p = p0 + kWave * k;
        const float4 pt = p < m ? pts[p] : make_float4(0.f, 0.f, 0.f, 0.f);
        px[k] = pt.x;
        py[k] = pt.y;
        pz[k] = pt.z;
        at_origin[k] = __builtin_fmaf(pt.z, pt.z, __builtin_fmaf(pt.y, pt.y, pt.x * pt.x)) == 0.f;
        cnt[k] = 0;
        for (int f = 0; f < kSums; ++f) sum[k][f] = 0.0;
    }

    // a tile's body for this thread: absent or non-finite -> massless at the origin
    auto load = [&](uint32_t jt, bool *masked) {
        const uint32_t j = jt * kTile + tid;
        float4 pj = make_float4(0.f, 0.f, 0.f, 0.f);
        *masked = true;
        if (j < n) {
            const float4 q = posm[j];
            if (body_ok(q, vel[j])) {
                pj = q;
                *masked = false;
            }
        }
        return pj;
    };
    // The stand-ins of masked bodies are coincident with a point at the origin: the barrier that publishes a
    // tile also counts its masked bodies, and such a point has the count of all the block's tiles subtracted.
    bool masked = false;
    uint32_t n_masked = 0, buf = 0;
    tile[0][tid] = load(j_begin, &masked);
    for (uint32_t jt = j_begin; jt < j_end; ++jt) {
        n_masked += __syncthreads_count(masked);  // tile[buf] is whole; tile[buf ^ 1] has been read
        float4 next = make_float4(0.f, 0.f, 0.f, 0.f);
        if (jt + 1 < j_end) next = load(jt + 1, &masked);  // in flight while this tile is summed
        Rule::template run_pairs<IB>(&tile[buf][wave * kRun], px, py, pz, c, sum, cnt);
        buf ^= 1;
        if (jt + 1 < j_end) tile[buf][tid] = next;
    }

    // the four waves' sums in wave order; wave 0 writes the slab
    for (uint32_t w = 1; w < kWaves; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int k = 0; k < IB; ++k) {
                for (int f = 0; f < kSums; ++f) red[k][f][lane] = sum[k][f];
                red[k][kSums][lane] = (double)cnt[k];
            }
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int k = 0; k < IB; ++k) {
                for (int f = 0; f < kSums; ++f) sum[k][f] += red[k][f][lane];
                cnt[k] += (uint32_t)red[k][kSums][lane];
            }
        }
    }
    if (wave == 0) {
        double *out = slab + (size_t)blockIdx.y * kSlabFields * stride;
        const uint32_t q0 = blockIdx.x * (kWave * IB) + lane;  // the point's place in the band
#pragma unroll
        for (int k = 0; k < IB; ++k) {
            const uint32_t p = p0 + kWave * k;
            if (p >= m) continue;
            const uint32_t q = q0 + kWave * k;
            for (int f = 0; f < kSums; ++f)
                if (Rule::writes(f)) out[(size_t)f * stride + q] = sum[k][f];
            out[(size_t)kSums * stride + q] = (double)(cnt[k] - (at_origin[k] ? n_masked : 0u));
        }
    }
}

// ---- host ----
template <class Sample>
struct Work : Workspace {  // (all but the last grow to the largest call so far)
    DeviceBuf<float4> pts;    // [padded points]
    PinnedBuf<float4> h_pts;  // as pts
    DeviceBuf<Sample> out;    // [padded points]
    PinnedBuf<Sample> h_out;  // as out
    DeviceBuf<double> slab;   // [chunks][slab fields][points of one band]
    PinnedBuf<double> h_bad;  // [1] the diagnostics' non-finite count
};

// What the two launches of a band are made from: the call's plan and buffers, and the band's point tiles
// [tile0, tile0 + tiles) = points [p0, p1)
template <class Sample>
struct Band {
    hipStream_t stream;
    const float4 *posm, *vel;  // the state (n > 0)
    uint32_t n, n_tiles, cj, chunks;
    const float4 *pts;
    uint32_t m, stride;
    double *slab;
    Sample *out;
    uint32_t tile0, tiles, p0, p1;
};

template <class Rule, int IB, class Sample>
void launch_pairs(const Band<Sample> &b, const typename Rule::Const &c) {
    hipLaunchKernelGGL((probe_kernel<Rule, IB>), dim3(b.tiles, b.chunks), dim3(kThreads), 0, b.stream, b.posm, b.vel,
                       b.n, b.n_tiles, b.cj, b.pts, b.m, b.stride, b.tile0, c, b.slab);
}
template <class Sample>
dim3 finish_grid(const Band<Sample> &b) {  // one thread per point of the band
    return dim3((b.p1 - b.p0 + kThreads - 1) / kThreads);
}

// The plan of m points, ib per lane, against n bodies: a function of (m, n, ib) alone but for the band, which
// "field_launch_pairs_log2" (pairs_log2) sizes.  The chunking is sized for a band of the default budget whatever the
// key says, so the key only partitions the points and cannot change a sum.
struct Plan {
    uint32_t tile_pts, p_tiles, m_pad;  // points per tile, point tiles, points padded to whole tiles
    uint32_t n_tiles, cj, chunks;       // body tiles, body tiles per chunk, chunks (0, 0 with no pairs)
    uint32_t band, stride;              // point tiles per launch, points of a band: the slab holds one band
};
inline Plan plan(uint32_t m, uint32_t n, int ib, int pairs_log2) {
    Plan p{};
    p.tile_pts = kWave * ib;
    p.p_tiles = (m + p.tile_pts - 1) / p.tile_pts;
    p.m_pad = p.p_tiles * p.tile_pts;
    p.n_tiles = (n + kTile - 1) / kTile;
    p.band = p.p_tiles;
    if (m > 0 && n > 0) {
        const uint64_t tile_pairs = (uint64_t)p.tile_pts * n;
        const uint32_t wide = (uint32_t)std::min<uint64_t>(p.p_tiles, std::max<uint64_t>(1, kPairsPerLaunch / tile_pairs));
        const uint32_t want = std::min(p.n_tiles, std::max(1u, (kBlocks + wide - 1) / wide));
        p.cj = (p.n_tiles + want - 1) / want;        // body tiles per chunk
        p.chunks = (p.n_tiles + p.cj - 1) / p.cj;    // every chunk holds at least one tile
        // bands of point tiles: a tile meets tile_pts * n pairs; at least one tile per launch
        p.band = (uint32_t)std::min<uint64_t>(p.p_tiles, std::max<uint64_t>(1, (1ull << pairs_log2) / tile_pairs));
    }
    p.stride = p.band * p.tile_pts;
    return p;
}

// A call: m points, ib per lane, into out[m] and *stats (stats->flags = flags), with the workspace of `slot` and
// a slab of slab_fields fields.  pairs(band) launches the unit's probe_kernel instantiation for a band -- only
// with n > 0 -- and finish(band) its finish kernel.
// The plan is plan()'s.
template <class Sample, class Pairs, class Finish>
int run(SimBase &sim, WorkSlot slot, const float *points, size_t m, int ib, uint32_t slab_fields, uint32_t flags,
        Sample *out, nb_field_stats *stats, Pairs pairs, Finish finish) {
    Work<Sample> *work = nullptr;
    if (int rc = workspace(sim, slot, &work, [](Work<Sample> &f) {
            NB_HIP_TRY(f.h_bad.reserve(1));
            return NB_OK;
        }))
        return rc;
    Work<Sample> &w = *work;
    const uint32_t n = sim.n, mm = (uint32_t)m;

    const Plan pl = plan(mm, n, ib, sim.field_pairs_log2);
    const uint32_t tile_pts = pl.tile_pts, p_tiles = pl.p_tiles, m_pad = pl.m_pad, n_tiles = pl.n_tiles;
    const uint32_t cj = pl.cj, chunks = pl.chunks, band = pl.band, stride = pl.stride;

    NB_HIP_TRY(w.pts.reserve(m_pad));
    NB_HIP_TRY(w.out.reserve(m_pad));
    NB_HIP_TRY(w.h_pts.reserve(m_pad));
    NB_HIP_TRY(w.h_out.reserve(m_pad));
    NB_HIP_TRY(w.slab.reserve((size_t)chunks * slab_fields * stride));

    uint64_t bad_points = 0;
    uint32_t launches = 0;
    *w.h_bad = 0.0;
    if (mm > 0) {
        for (uint32_t i = 0; i < mm; ++i) {
            const float x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
            w.h_pts[i] = make_float4(x, y, z, 0.f);
            bad_points += !(std::isfinite(x) && std::isfinite(y) && std::isfinite(z));
        }
        // from here the pinned points are being read: an error drains the stream before it returns
        const int rc = [&]() -> int {
            NB_HIP_TRY(hipMemcpyAsync(w.pts, w.h_pts, sizeof(float4) * mm, hipMemcpyHostToDevice, sim.stream));
            Band<Sample> b{sim.stream, nullptr, nullptr, n, n_tiles, cj, chunks, w.pts, mm, stride, w.slab, w.out, 0, 0, 0, 0};
            if (n > 0) {
                sim.diag_state(&b.posm, &b.vel);
                const double *mom = nullptr;  // the bodies nb_sim_diagnostics counts as non-finite
                if (int rc = diag_enqueue_moments(sim, &mom)) return rc;
                NB_HIP_TRY(hipMemcpyAsync(w.h_bad, mom + kDiagResBad, sizeof(double), hipMemcpyDeviceToHost, sim.stream));
            }
            for (b.tile0 = 0; b.tile0 < p_tiles; b.tile0 += band) {
                b.tiles = std::min(band, p_tiles - b.tile0);
                b.p0 = b.tile0 * tile_pts;
                b.p1 = std::min(mm, (b.tile0 + b.tiles) * tile_pts);
                if (n > 0) {
                    pairs(b);
                    NB_HIP_TRY(hipGetLastError());
                    ++launches;
                }
                finish(b);
                NB_HIP_TRY(hipGetLastError());
            }
            NB_HIP_TRY(hipMemcpyAsync(w.h_out, w.out, sizeof(Sample) * mm, hipMemcpyDeviceToHost, sim.stream));
            return NB_OK;
        }();
        if (rc != NB_OK) {
            (void)hipStreamSynchronize(sim.stream);
            return rc;
        }
    }
    NB_HIP_TRY(hipStreamSynchronize(sim.stream));
    if (int rc = sim.diag_status()) return rc;
    if (mm > 0) std::memcpy(out, w.h_out, sizeof(Sample) * mm);

    if (stats) {
        nb_field_stats s{};  // (nb_tidal_stats is the same struct)
        s.step_num = sim.step_num;
        s.n = n;
        s.nonfinite = (uint64_t)*w.h_bad;
        s.points = m;
        s.nonfinite_points = bad_points;
        s.flags = flags;
        s.launches = launches;
        *stats = s;
    }
    return NB_OK;
}

}  // namespace probe
}  // namespace nb
