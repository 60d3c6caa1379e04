// nb_tidal.hip -- nb_tidal_sim: the exact tidal tensor T_ab = d a_a / d x_b of a simulator's current state at
// arbitrary points (include/nbody.h "Tidal tensor probes"; no reference counterpart).
//
// The gradient of the field nb_field.hip sums, summed pair by pair as the field is.  For a point p and body j,
// d = x_j - p:
//   w = m_j / (r^4 + e r)    (the field's own pair weight)      c = (4 r^3 + e) / (r^2 (r^3 + e))
//   S_ab = sum_j w c d_a d_b (xx, yy, zz, xy, xz, yz)           W = sum_j w
//   T_ab = g (S_ab - delta_ab W)
// M points against the N bodies of the float4 SoA state the simulator hands out (SimBase::diag_state), tiled as
// nb_field.hip tiles them (its staging loop is repeated here on purpose: DESIGN.md 6r):
//   tidal   -- a block of 256 threads owns a tile of 64 IB points, IB per lane in VGPRs, the same points in
//              each of its four waves.  blockIdx.y cuts the bodies into chunks of 256-body tiles; the block
//              stages each tile through LDS (double-buffered, one barrier per tile) with the diagnostics'
//              predicate applied on load -- an absent or non-finite body is massless at the origin -- and
//              wave w reads back bodies [64 w, 64 w + 64) of the tile as wave-uniform broadcasts: one fp32
//              run of 64 pairs per point and sum, folded into the wave's seven fp64 sums.  At the end the four
//              waves' sums meet in LDS in wave order and the block writes seven doubles and a coincident count
//              per point into slab[chunk][field][point of the band].  The point tiles go in bands, one launch
//              per band, bounded in pairs by the field's "field_launch_pairs_log2";
//   finish  -- after each band, one thread per point adds the chunks in order, subtracts W from the diagonal
//              sums once, in fp64, scales by g and writes the nb_tidal_sample; the samples are copied once
//              into pinned host memory ahead of the one synchronisation.
// The non-finite count is the diagnostics' own (diag_enqueue_moments on the same stream).
// No float atomics; the grid and the chunking depend on (M, N) alone and every lane runs the same operations in
// the same order, so the result is bitwise reproducible and does not depend on where in the array a point
// stands.  The unit is built without FMA contraction: the pair arithmetic below is the arithmetic that runs,
// and the bound of include/nbody.h counts its roundings.
#include <cmath>
#include <cstring>

#include "nb_analysis.hpp"
#include "nb_common.hpp"
#include "nb_psi.hpp"
#include "nb_sim.hpp"

namespace nb {

namespace {

constexpr uint32_t kThreads = 256;      // 4 waves per block
constexpr uint32_t kWaves = kThreads / kWave;
constexpr uint32_t kTile = 256;         // bodies per staged tile: one run of kRun per wave
constexpr uint32_t kRun = kTile / kWaves;  // pairs summed in fp32 before folding into fp64 (R = 64)
constexpr uint32_t kBlocks = 1024;      // with few point tiles, chunks enough for this many blocks (4 per CU)
// pairs per launch the chunking is sized for: the default of "field_launch_pairs_log2" (nb_field.hip)
constexpr uint64_t kPairsPerLaunch = 1ull << 35;
constexpr int kSums = 7;                // S_xx, S_yy, S_zz, S_xy, S_xz, S_yz, W
constexpr uint32_t kSlabFields = kSums + 1;  // ... and the coincident count
static_assert(kRun == 64, "the stated error bound is for runs of 64");

// One tile of bodies for one wave: bodies [0, kRun) of `run` against the lane's IB points.  The per-pair form the
// bound's K = 33 is derived for: one sqrt, two rcp.
template <int IB>
__device__ __forceinline__ void run_pairs(const float4 *run, const float (&px)[IB], const float (&py)[IB],
                                          const float (&pz)[IB], float e, double (&sum)[IB][kSums],
                                          uint32_t (&cnt)[IB]) {
    float s[IB][kSums];
#pragma unroll
    for (int k = 0; k < IB; ++k)
        for (int f = 0; f < kSums; ++f) s[k][f] = 0.f;
#pragma unroll 2
    for (uint32_t j = 0; j < kRun; ++j) {
        const float4 q = run[j];  // wave-uniform address: LDS broadcast
#pragma unroll
        for (int k = 0; k < IB; ++k) {
            const float dx = q.x - px[k], dy = q.y - py[k], dz = q.z - pz[k];
            const float r2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
            const bool coincident = r2 == 0.f;  // adds nothing (not m / 0)
            cnt[k] += coincident ? 1u : 0u;
            const float r = __builtin_amdgcn_sqrtf(r2);       // v_sqrt_f32
            const float den = __builtin_fmaf(e, r, r2 * r2);  // r^4 + e r
            float w = __builtin_amdgcn_rcpf(den) * q.w;       // v_rcp_f32: the field's pair weight
            const float r3 = r2 * r;
            const float num = __builtin_fmaf(4.f, r3, e);     // 4 r^3 + e
            const float c = num * __builtin_amdgcn_rcpf(r2 * (r3 + e));
            w = coincident ? 0.f : w;
            // a body so far that r^3 is not an fp32 number (r > 6.9e12) adds 0 to S, not inf * 0: its w is 0 already
            const float wc = (coincident || !(r3 < INFINITY)) ? 0.f : w * c;
            const float tx = wc * dx, ty = wc * dy, tz = wc * dz;
            s[k][0] = __builtin_fmaf(tx, dx, s[k][0]);
            s[k][1] = __builtin_fmaf(ty, dy, s[k][1]);
            s[k][2] = __builtin_fmaf(tz, dz, s[k][2]);
            s[k][3] = __builtin_fmaf(tx, dy, s[k][3]);
            s[k][4] = __builtin_fmaf(tx, dz, s[k][4]);
            s[k][5] = __builtin_fmaf(ty, dz, s[k][5]);
            s[k][6] += w;
        }
    }
#pragma unroll
    for (int k = 0; k < IB; ++k)
        for (int f = 0; f < kSums; ++f) sum[k][f] += (double)s[k][f];
}

// ---- tidal: block (x, y) = point tile tile0 + x against body tiles [y cj, min(n_tiles, (y + 1) cj)) ----
// Point k of lane l of the tile is tile * 64 IB + 64 k + l.  The slab holds one band:
// slab[(y * kSlabFields + f) * stride + (point - tile0 * 64 IB)].
template <int IB>
__global__ __launch_bounds__(kThreads) void tidal_kernel(const float4 *__restrict__ posm,
                                                         const float4 *__restrict__ vel, uint32_t n,
                                                         uint32_t n_tiles, uint32_t cj,
                                                         const float4 *__restrict__ pts, uint32_t m, uint32_t stride,
                                                         uint32_t tile0, float e, double *__restrict__ slab) {
    __shared__ float4 tile[2][kTile];
    __shared__ double red[IB][kSlabFields][kWave];
    const uint32_t tid = threadIdx.x, lane = tid % kWave;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    const uint32_t p0 = (tile0 + blockIdx.x) * (kWave * IB) + lane;
    const uint32_t j_begin = blockIdx.y * cj, j_end = min(n_tiles, j_begin + cj);  // (never empty: see plan)

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
    bool masked = false;
    uint32_t n_masked = 0, buf = 0;
    tile[0][tid] = load(j_begin, &masked);
    for (uint32_t jt = j_begin; jt < j_end; ++jt) {
        n_masked += __syncthreads_count(masked);  // tile[buf] is whole; tile[buf ^ 1] has been read
        float4 next = make_float4(0.f, 0.f, 0.f, 0.f);
        if (jt + 1 < j_end) next = load(jt + 1, &masked);  // in flight while this tile is summed
        run_pairs<IB>(&tile[buf][wave * kRun], px, py, pz, e, sum, cnt);
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
            for (int f = 0; f < kSums; ++f) out[(size_t)f * stride + q] = sum[k][f];
            out[(size_t)kSums * stride + q] = (double)(cnt[k] - (at_origin[k] ? n_masked : 0u));
        }
    }
}

// ---- finish: the chunks of every point of a band [p0, p1) in order; the diagonal's S_aa - W once, in fp64; scaled
// by g once -> nb_tidal_sample ----
__global__ __launch_bounds__(kThreads) void tidal_finish_kernel(const double *__restrict__ slab, uint32_t chunks,
                                                                const float4 *__restrict__ pts, uint32_t p0,
                                                                uint32_t p1, uint32_t stride, double g,
                                                                nb_tidal_sample *__restrict__ out) {
    const uint32_t q = blockIdx.x * kThreads + threadIdx.x, p = p0 + q;
    if (p >= p1) return;
    const float4 pt = pts[p];
    const bool ok = isfinite(pt.x) && isfinite(pt.y) && isfinite(pt.z);
    double s[kSlabFields] = {};
    for (uint32_t c = 0; c < chunks; ++c) {
        const double *in = slab + (size_t)c * kSlabFields * stride + q;
        for (uint32_t f = 0; f < kSlabFields; ++f) s[f] += in[(size_t)f * stride];
    }
    nb_tidal_sample r{};
    for (int f = 0; f < 6; ++f) r.tensor[f] = ok ? g * (f < 3 ? s[f] - s[6] : s[f]) : (double)NAN;
    r.coincident = ok ? (uint32_t)s[kSums] : 0u;
    out[p] = r;
}

// the instantiations points_per_lane() can ask for
void launch_tidal(int ib, dim3 grid, hipStream_t stream, const float4 *posm, const float4 *vel, uint32_t n,
                  uint32_t n_tiles, uint32_t cj, const float4 *pts, uint32_t m, uint32_t stride, uint32_t tile0,
                  float e, double *slab) {
#define NB_TIDAL_LAUNCH(IB)                                                                                       \
    hipLaunchKernelGGL((tidal_kernel<IB>), grid, dim3(kThreads), 0, stream, posm, vel, n, n_tiles, cj, pts, m, stride, \
                       tile0, e, slab)
    if (ib == 1)
        NB_TIDAL_LAUNCH(1);
    else if (ib == 2)
        NB_TIDAL_LAUNCH(2);
    else
        NB_TIDAL_LAUNCH(4);
#undef NB_TIDAL_LAUNCH
}

}  // namespace

struct TidalWork : Workspace {  // (all but the last grow to the largest call so far)
    DeviceBuf<float4> pts;             // [padded points]
    PinnedBuf<float4> h_pts;           // as pts
    DeviceBuf<nb_tidal_sample> out;    // [padded points]
    PinnedBuf<nb_tidal_sample> h_out;  // as out
    DeviceBuf<double> slab;            // [chunks][kSlabFields][points of one band]
    PinnedBuf<double> h_bad;           // [1] the diagnostics' non-finite count
};

// Points per lane: a function of m alone.  The thresholds are those nb_field.hip measured for the acceleration
// alone (whole tiles of 256 points from 256 on, the narrowest tile that holds a handful); they have not been
// measured again for this kernel.
static int points_per_lane(size_t m) { return m >= 4 * kWave ? 4 : m > kWave ? 2 : 1; }

int sim_tidal(SimBase &sim, const float *points, size_t m, nb_tidal_sample *out, nb_tidal_stats *stats) {
    if (int rc = refuse_sharded(sim, "tidal")) return rc;
    if (int rc = sim.bind_device()) return rc;
    TidalWork *work = nullptr;
    if (int rc = workspace(sim, kWorkTidal, &work, [](TidalWork &f) {
            NB_HIP_TRY(f.h_bad.reserve(1));
            return NB_OK;
        }))
        return rc;
    TidalWork &w = *work;
    const uint32_t n = sim.n, mm = (uint32_t)m;

    // the plan: a function of (m, n) alone
    const int ib = points_per_lane(m);
    const uint32_t tile_pts = kWave * ib;
    const uint32_t p_tiles = (mm + tile_pts - 1) / tile_pts, m_pad = p_tiles * tile_pts;
    const uint32_t n_tiles = (n + kTile - 1) / kTile;
    uint32_t cj = 0, chunks = 0;
    if (mm > 0 && n > 0) {
        // (sized for a band of the default budget, whatever "field_launch_pairs_log2" says: the key must
        // not change a sum)
        const uint64_t tile_pairs = (uint64_t)tile_pts * n;
        const uint32_t wide = (uint32_t)std::min<uint64_t>(p_tiles, std::max<uint64_t>(1, kPairsPerLaunch / tile_pairs));
        const uint32_t want = std::min(n_tiles, std::max(1u, (kBlocks + wide - 1) / wide));
        cj = (n_tiles + want - 1) / want;        // body tiles per chunk
        chunks = (n_tiles + cj - 1) / cj;        // every chunk holds at least one tile
    }

    NB_HIP_TRY(w.pts.reserve(m_pad));
    NB_HIP_TRY(w.out.reserve(m_pad));
    NB_HIP_TRY(w.h_pts.reserve(m_pad));
    NB_HIP_TRY(w.h_out.reserve(m_pad));
    // bands of point tiles: a tile meets tile_pts * n pairs; at least one tile per launch.  The slab holds one band.
    uint32_t band = p_tiles;
    if (mm > 0 && n > 0)
        band = (uint32_t)std::min<uint64_t>(p_tiles, std::max<uint64_t>(1, (1ull << sim.field_pairs_log2) / ((uint64_t)tile_pts * n)));
    const uint32_t stride = band * tile_pts;
    NB_HIP_TRY(w.slab.reserve((size_t)chunks * kSlabFields * stride));

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
            const float4 *posm = nullptr, *vel = nullptr;
            if (n > 0) {
                sim.diag_state(&posm, &vel);
                const double *mom = nullptr;  // the bodies nb_sim_diagnostics counts as non-finite
                if (int rc = diag_enqueue_moments(sim, &mom)) return rc;
                NB_HIP_TRY(hipMemcpyAsync(w.h_bad, mom + kDiagResBad, sizeof(double), hipMemcpyDeviceToHost, sim.stream));
            }
            for (uint32_t t0 = 0; t0 < p_tiles; t0 += band) {
                const uint32_t tiles = std::min(band, p_tiles - t0);
                const uint32_t p0 = t0 * tile_pts, p1 = std::min(mm, (t0 + tiles) * tile_pts);
                if (n > 0) {
                    launch_tidal(ib, dim3(tiles, chunks), sim.stream, posm, vel, n, n_tiles, cj, w.pts, mm, stride, t0,
                                 sim.params.e, w.slab);
                    NB_HIP_TRY(hipGetLastError());
                    ++launches;
                }
                hipLaunchKernelGGL(tidal_finish_kernel, dim3((p1 - p0 + kThreads - 1) / kThreads), dim3(kThreads), 0,
                                   sim.stream, w.slab, chunks, w.pts, p0, p1, stride, (double)sim.params.g, w.out);
                NB_HIP_TRY(hipGetLastError());
            }
            NB_HIP_TRY(hipMemcpyAsync(w.h_out, w.out, sizeof(nb_tidal_sample) * mm, hipMemcpyDeviceToHost, sim.stream));
            return NB_OK;
        }();
        if (rc != NB_OK) {
            (void)hipStreamSynchronize(sim.stream);
            return rc;
        }
    }
    NB_HIP_TRY(hipStreamSynchronize(sim.stream));
    if (int rc = sim.diag_status()) return rc;
    if (mm > 0) std::memcpy(out, w.h_out, sizeof(nb_tidal_sample) * mm);

    if (stats) {
        nb_tidal_stats s{};
        s.step_num = sim.step_num;
        s.n = n;
        s.nonfinite = (uint64_t)*w.h_bad;
        s.points = m;
        s.nonfinite_points = bad_points;
        s.flags = 0;
        s.launches = launches;
        *stats = s;
    }
    return NB_OK;
}

}  // namespace nb
