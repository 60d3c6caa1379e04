// nb_tidal.hip -- nb_tidal_sim: the exact tidal tensor T_ab = d a_a / d x_b of a simulator's current state at
// arbitrary points (include/nbody.h "Tidal tensor probes"; no reference counterpart).
//
// The gradient of the field nb_field.hip sums, summed pair by pair as the field is.  For a point p and body j,
// d = x_j - p:
//   w = m_j / (r^4 + e r)    (the field's own pair weight)      c = (4 r^3 + e) / (r^2 (r^3 + e))
//   S_ab = sum_j w c d_a d_b (xx, yy, zz, xy, xz, yz)           W = sum_j w
//   T_ab = g (S_ab - delta_ab W)
// M points against the N bodies of the float4 SoA state the simulator hands out, tiled, staged, summed and
// sequenced as nb_field.hip's are, by the same code (nb_probe.hpp); here are the rule and what follows from it:
//   tidal   -- probe_kernel<TidalRule, IB>: seven fp32 run accumulators and seven fp64 sums per point, all written,
//              and the coincident count.  The bands are bounded in pairs by the field's "field_launch_pairs_log2";
//   finish  -- after each band, one thread per point adds the chunks in order, subtracts W from the diagonal
//              sums once, in fp64, scales by g and writes the nb_tidal_sample.
// The non-finite count is the diagnostics' own (diag_enqueue_moments on the same stream).
// No float atomics; the grid and the chunking depend on (M, N) alone and every lane runs the same operations in
// the same order, so the result is bitwise reproducible and does not depend on where in the array a point
// stands.  The unit is built without FMA contraction: the pair arithmetic below is the arithmetic that runs,
// and the bound of include/nbody.h counts its roundings.
#include "nb_probe.hpp"

namespace nb {

using namespace probe;

namespace {

struct TidalRule {
    static constexpr int kSums = 7;  // S_xx, S_yy, S_zz, S_xy, S_xz, S_yz, W
    using Const = float;             // e
    static constexpr bool writes(int) { return true; }

    // One tile of bodies for one wave: bodies [0, kRun) of `run` against the lane's IB points.  The per-pair form
    // the bound's K = 33 is derived for: one sqrt, two rcp.
    template <int IB>
    static __device__ __forceinline__ void run_pairs(const float4 *run, const float (&px)[IB], const float (&py)[IB],
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
};

constexpr int kSums = TidalRule::kSums;
constexpr uint32_t kSlabFields = kSums + 1;  // ... and the coincident count

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
void launch_tidal(int ib, const Band<nb_tidal_sample> &b, float e) {
    if (ib == 1)
        launch_pairs<TidalRule, 1>(b, e);
    else if (ib == 2)
        launch_pairs<TidalRule, 2>(b, e);
    else
        launch_pairs<TidalRule, 4>(b, e);
}

}  // namespace

// Points per lane: a function of m alone.  The thresholds are those nb_field.hip measured for the acceleration
// alone (whole tiles of 256 points from 256 on, the narrowest tile that holds a handful); they have not been
// measured again for this kernel.
static int points_per_lane(size_t m) { return m >= 4 * kWave ? 4 : m > kWave ? 2 : 1; }

int sim_tidal(SimBase &sim, const float *points, size_t m, nb_tidal_sample *out, nb_tidal_stats *stats) {
    if (int rc = analysis_begin(sim, "tidal")) return rc;
    const int ib = points_per_lane(m);
    const float e = sim.params.e;
    const double g = (double)sim.params.g;
    return run(
        sim, kWorkTidal, points, m, ib, kSlabFields, 0, out, stats,
        [&](const Band<nb_tidal_sample> &b) { launch_tidal(ib, b, e); },
        [&](const Band<nb_tidal_sample> &b) {
            hipLaunchKernelGGL(tidal_finish_kernel, finish_grid(b), dim3(kThreads), 0, b.stream, b.slab, b.chunks, b.pts,
                               b.p0, b.p1, b.stride, g, b.out);
        });
}

}  // namespace nb
