// nb_field.hip -- nb_sim_field: the exact acceleration and potential of a simulator's current state at
// arbitrary points (include/nbody.h "Field probes"; no reference counterpart).
//
// M points against the N bodies of the float4 SoA state the simulator hands out, tiled, staged, summed and
// sequenced by nb_probe.hpp; here are the rule and what follows from it:
//   field   -- probe_kernel<FieldRule<MODE>, IB>, MODE the requested fields: per pair the arithmetic of the step
//              (nb_naive.hip's pair()) and, for the potential, m psi(r); four fp64 sums per point -- ax, ay, az
//              and the psi sum -- of which an instantiation writes those of its MODE, and the coincident count;
//   finish  -- after each band, one thread per point adds the chunks in order, scales by g and writes the
//              nb_field_sample.
// The non-finite count is the diagnostics' own (diag_enqueue_moments on the same stream).
// No float atomics; the grid and the chunking depend on (M, N, flags) alone and every lane runs the same
// operations in the same order, so the result is bitwise reproducible and does not depend on where in
// the array a point stands.
#include "nb_probe.hpp"
#include "nb_psi.hpp"

namespace nb {

using namespace probe;

namespace {

enum : int { kAcc = NB_FIELD_ACCEL, kPot = NB_FIELD_POTENTIAL };

template <int MODE>
struct FieldRule {
    static constexpr int kSums = 4;  // ax, ay, az, psi sum
    using Const = PsiConst;
    static constexpr bool writes(int f) { return MODE & (f < 3 ? kAcc : kPot); }

    // One tile of bodies for one wave: bodies [0, kRun) of `run` against the lane's IB points.
    template <int IB>
    static __device__ __forceinline__ void run_pairs(const float4 *run, const float (&px)[IB], const float (&py)[IB],
                                                     const float (&pz)[IB], const PsiConst &c, double (&sum)[IB][4],
                                                     uint32_t (&cnt)[IB]) {
        const float e = c.e;
        float ax[IB], ay[IB], az[IB], ph[IB];
#pragma unroll
        for (int k = 0; k < IB; ++k) ax[k] = ay[k] = az[k] = ph[k] = 0.f;
#pragma unroll 4
        for (uint32_t j = 0; j < kRun; ++j) {
            const float4 q = run[j];  // wave-uniform address: LDS broadcast
#pragma unroll
            for (int k = 0; k < IB; ++k) {
                const float dx = q.x - px[k], dy = q.y - py[k], dz = q.z - pz[k];
                const float r2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
                const bool coincident = r2 == 0.f;  // adds nothing (not m / 0 or m psi(0))
                cnt[k] += coincident ? 1u : 0u;
                if (MODE & kAcc) {  // the pair arithmetic of nb_naive.hip's pair()
                    const float r = __builtin_amdgcn_sqrtf(r2);       // v_sqrt_f32
                    const float den = __builtin_fmaf(e, r, r2 * r2);  // r^4 + e r
                    float w = __builtin_amdgcn_rcpf(den) * q.w;       // v_rcp_f32
                    w = coincident ? 0.f : w;
                    ax[k] = __builtin_fmaf(w, dx, ax[k]);
                    ay[k] = __builtin_fmaf(w, dy, ay[k]);
                    az[k] = __builtin_fmaf(w, dz, az[k]);
                }
                if (MODE & kPot) {
                    const float t = q.w * psi_f32(r2, c);
                    ph[k] += coincident ? 0.f : t;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < IB; ++k) {
            if (MODE & kAcc) {
                sum[k][0] += (double)ax[k];
                sum[k][1] += (double)ay[k];
                sum[k][2] += (double)az[k];
            }
            if (MODE & kPot) sum[k][3] += (double)ph[k];
        }
    }
};

constexpr uint32_t kSlabFields = FieldRule<kAcc>::kSums + 1;  // ... and the coincident count

// ---- finish: the chunks of every point of a band [p0, p1) in order, scaled by g once -> nb_field_sample ----
__global__ __launch_bounds__(kThreads) void field_finish_kernel(const double *__restrict__ slab, uint32_t chunks,
                                                                const float4 *__restrict__ pts, uint32_t p0,
                                                                uint32_t p1, uint32_t stride, uint32_t flags, double g,
                                                                nb_field_sample *__restrict__ out) {
    const uint32_t q = blockIdx.x * kThreads + threadIdx.x, p = p0 + q;
    if (p >= p1) return;
    const float4 pt = pts[p];
    const bool ok = isfinite(pt.x) && isfinite(pt.y) && isfinite(pt.z);
    double s[kSlabFields] = {};
    for (uint32_t c = 0; c < chunks; ++c) {
        const double *in = slab + (size_t)c * kSlabFields * stride + q;
        if (flags & NB_FIELD_ACCEL)
            for (int f = 0; f < 3; ++f) s[f] += in[(size_t)f * stride];
        if (flags & NB_FIELD_POTENTIAL) s[3] += in[(size_t)3 * stride];
        s[4] += in[(size_t)4 * stride];
    }
    nb_field_sample r{};
    const bool acc = ok && (flags & NB_FIELD_ACCEL), pot = ok && (flags & NB_FIELD_POTENTIAL);
    for (int f = 0; f < 3; ++f) r.acc[f] = acc ? g * s[f] : (double)NAN;
    r.potential = pot ? -(g * s[3]) : (double)NAN;
    r.coincident = ok ? (uint32_t)s[4] : 0u;
    out[p] = r;
}

// the instantiations points_per_lane() can ask for
void launch_field(uint32_t flags, int ib, const Band<nb_field_sample> &b, const PsiConst &c) {
    if (flags == NB_FIELD_POTENTIAL)
        launch_pairs<FieldRule<kPot>, 2>(b, c);
    else if (flags != NB_FIELD_ACCEL)
        launch_pairs<FieldRule<kAcc | kPot>, 2>(b, c);
    else if (ib == 1)
        launch_pairs<FieldRule<kAcc>, 1>(b, c);
    else if (ib == 2)
        launch_pairs<FieldRule<kAcc>, 2>(b, c);
    else
        launch_pairs<FieldRule<kAcc>, 4>(b, c);
}

}  // namespace

// Points per lane, by measurement: a function of m and the flags alone.  The acceleration
// alone runs fastest with whole tiles of 256 points, four per lane, and with a handful of points on the
// narrowest tile that holds them; with the potential, two per lane are fastest at every m (psi's registers).
static int points_per_lane(size_t m, uint32_t flags) {
    if (flags & NB_FIELD_POTENTIAL) return 2;
    return m >= 4 * kWave ? 4 : m > kWave ? 2 : 1;
}

int sim_field(SimBase &sim, const float *points, size_t m, uint32_t flags, nb_field_sample *out,
              nb_field_stats *stats) {
    if (int rc = refuse_sharded(sim, "field")) return rc;
    const float e = sim.params.e;
    if ((flags & NB_FIELD_POTENTIAL) && !(e >= 0.f)) {
        set_error("field: the potential needs e >= 0 (e = %g)", (double)e);
        return NB_ERR_INVALID;
    }
    if (int rc = sim.bind_device()) return rc;
    const int ib = points_per_lane(m, flags);
    const PsiConst c = sim.n > 0 ? psi_const(e) : PsiConst{};
    const double g = (double)sim.params.g;
    return run(
        sim, kWorkField, points, m, ib, kSlabFields, flags, out, stats,
        [&](const Band<nb_field_sample> &b) { launch_field(flags, ib, b, c); },
        [&](const Band<nb_field_sample> &b) {
            hipLaunchKernelGGL(field_finish_kernel, finish_grid(b), dim3(kThreads), 0, b.stream, b.slab, b.chunks, b.pts,
                               b.p0, b.p1, b.stride, flags, g, b.out);
        });
}

}  // namespace nb
