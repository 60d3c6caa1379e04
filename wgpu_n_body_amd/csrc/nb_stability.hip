// nb_stability.hip -- nb_orbit_stability_sim: deviation vectors carried along the orbits of nb_orbits_sim by the
// tangent map of its step, renormalised by exact powers of two (include/nbody.h "Orbit stability"; no
// reference counterpart).
//
// The sequence is nb_orbits_sim's (orbits_run of nb_field.hip, with this unit as its rider: nb_orbit.hpp); here are
//   pairs   -- probe_kernel<StabilityRule, IB>: the acceleration's three sums and the tidal tensor's seven in one pass
//              over the bodies.  Per pair the lines of nb_field.hip's FieldRule<kAcc> and of nb_tidal.hip's TidalRule,
//              which share dx, r^2, r, den and w; ten fp32 run accumulators and ten fp64 sums per point.  The points
//              per lane and the plan are theirs, so each sum is bit for bit what nb_sim_field and nb_tidal_sim sum
//              at the same m points;
//   step    -- orbit_step of nb_orbit.hpp -- the lines that move x and v, stated once -- with the deviations riding
//              in it: one thread per tracer finishes the tensor as tidal_finish_kernel does and moves its D vectors.
// The unit is built without FMA contraction.  The acceleration's lines are explicit fmas and lone multiplies, so they
// are the arithmetic nb_field.hip runs; the tensor's are nb_tidal.hip's, built without contraction as well.
#include "nb_orbit.hpp"

namespace nb {

using namespace probe;
using namespace orbit;

namespace {

struct StabilityRule {
    static constexpr int kSums = 10;  // ax, ay, az; S_xx, S_yy, S_zz, S_xy, S_xz, S_yz, W
    using Const = float;              // e
    static constexpr bool writes(int) { return true; }

    // One tile of bodies for one wave: bodies [0, kRun) of `run` against the lane's IB points.
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
                // what the two rules share
                const float dx = q.x - px[k], dy = q.y - py[k], dz = q.z - pz[k];
                const float r2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
                const bool coincident = r2 == 0.f;  // adds nothing (not m / 0)
                cnt[k] += coincident ? 1u : 0u;
                const float r = __builtin_amdgcn_sqrtf(r2);       // v_sqrt_f32
                const float den = __builtin_fmaf(e, r, r2 * r2);  // r^4 + e r
                float w = __builtin_amdgcn_rcpf(den) * q.w;       // v_rcp_f32: the pair weight
                // the tensor's factor (nb_tidal.hip)
                const float r3 = r2 * r;
                const float num = __builtin_fmaf(4.f, r3, e);     // 4 r^3 + e
                const float c = num * __builtin_amdgcn_rcpf(r2 * (r3 + e));
                w = coincident ? 0.f : w;
                // the acceleration (nb_field.hip)
                s[k][0] = __builtin_fmaf(w, dx, s[k][0]);
                s[k][1] = __builtin_fmaf(w, dy, s[k][1]);
                s[k][2] = __builtin_fmaf(w, dz, s[k][2]);
                // the tensor: a body so far that r^3 is not an fp32 number adds 0 to S, not inf * 0
                const float wc = (coincident || !(r3 < INFINITY)) ? 0.f : w * c;
                const float tx = wc * dx, ty = wc * dy, tz = wc * dz;
                s[k][3] = __builtin_fmaf(tx, dx, s[k][3]);
                s[k][4] = __builtin_fmaf(ty, dy, s[k][4]);
                s[k][5] = __builtin_fmaf(tz, dz, s[k][5]);
                s[k][6] = __builtin_fmaf(tx, dy, s[k][6]);
                s[k][7] = __builtin_fmaf(tx, dz, s[k][7]);
                s[k][8] = __builtin_fmaf(ty, dz, s[k][8]);
                s[k][9] += w;
            }
        }
#pragma unroll
        for (int k = 0; k < IB; ++k)
            for (int f = 0; f < kSums; ++f) sum[k][f] += (double)s[k][f];
    }
};

constexpr int kAccSums = 3, kTensorSums = 7;  // of the rule's ten, in this order
constexpr uint32_t kStabilityFields = StabilityRule::kSums + 1;  // ... and the coincident count

// ---- the deviations as orbit_step's ride: state k of the D vectors of tracer p ----
struct StabilityRide {
    static constexpr uint32_t kSlabFields = kStabilityFields, kCount = StabilityRule::kSums;
    uint32_t D, renorm_log2;
    uint64_t step;             // step0 + k
    nb_orbit_deviation *cur;   // [m][D] the vectors between the launches (dv: dv_0, then the half-kicked one)
    nb_orbit_growth *growth;   // [m][D]
    nb_orbit_deviation *rec;   // [m][D] the record's row, or null

    __device__ __forceinline__ void state(uint32_t p, const double *in, uint32_t chunks, uint32_t stride, bool ok,
                                          const double (&)[3], const double (&)[3], const OrbitStep &st,
                                          const OrbitFrame &f) const {
#pragma clang fp contract(off)
        // T_snap: the chunks in order, S_aa - W once in fp64 and the scaling by g as tidal_finish_kernel has them,
        // then accel_scale
        double s[kTensorSums] = {};
        for (uint32_t c = 0; c < chunks; ++c) {
            const double *row = in + (size_t)c * kSlabFields * stride;
            for (int k = 0; k < kTensorSums; ++k) s[k] += row[(size_t)(kAccSums + k) * stride];
        }
        double T[6];  // xx, yy, zz, xy, xz, yz
        for (int k = 0; k < 6; ++k) T[k] = st.scale * (ok ? st.g * (k < 3 ? s[k] - s[6] : s[k]) : (double)NAN);

        for (uint32_t d = 0; d < D; ++d) {
            const size_t at = (size_t)p * D + d;
            nb_orbit_deviation dv = cur[at];
            nb_orbit_growth gr;
            if (st.first) {
                gr.peak_log2 = INT64_MIN;
                gr.peak_step = NB_ORBIT_NO_STEP;
                gr.renorms = gr.reserved = 0;
            } else {
                gr = growth[at];
            }
            // kappa = h turn_back(T_snap turn(dx)): turn is orbit_point's without the centre and the rounding
            double q[3] = {dv.d[0], dv.d[1], dv.d[2]};
            if (st.rotating) {
                const double a = (q[0] * f.e1[0] + q[1] * f.e1[1]) + q[2] * f.e1[2];
                const double b = (q[0] * f.e2[0] + q[1] * f.e2[1]) + q[2] * f.e2[2];
                const double l = (q[0] * f.n[0] + q[1] * f.n[1]) + q[2] * f.n[2];
                const double ar = a * st.ck + b * st.sk, br = b * st.ck - a * st.sk;
                for (int i = 0; i < 3; ++i) q[i] = (ar * f.e1[i] + br * f.e2[i]) + l * f.n[i];
            }
            const double t[3] = {(T[0] * q[0] + T[3] * q[1]) + T[4] * q[2], (T[3] * q[0] + T[1] * q[1]) + T[5] * q[2],
                                 (T[4] * q[0] + T[5] * q[1]) + T[2] * q[2]};
            double a[3] = {t[0], t[1], t[2]};
            if (st.rotating) orbit_turn_back(t, f, st.ck, st.sk, a);
            double kick[3];
            for (int i = 0; i < 3; ++i) {
                kick[i] = a[i] * st.h;
                if (!st.first) dv.d[3 + i] = dv.d[3 + i] + kick[i];
            }
            // mu, its exponent, the peak, and the renormalisation -- of the six components and of kappa, which the
            // next half-kick adds: scaling the vector alone would leave a run that is not the unscaled run x 2^log2
            double mu = 0.0;
            bool finite = true;
            for (int i = 0; i < 6; ++i) {
                const double c = fabs(dv.d[i]);
                finite = finite && isfinite(c);
                mu = c > mu ? c : mu;
            }
            if (finite && mu > 0.0) {
                int ex;
                (void)frexp(mu, &ex);
                const int E = ex - 1;
                const int64_t peak = dv.log2 + E;
                if (peak > gr.peak_log2) {
                    gr.peak_log2 = peak;
                    gr.peak_step = step;
                }
                if (!st.first && (uint32_t)(E < 0 ? -E : E) >= renorm_log2) {
                    for (int i = 0; i < 6; ++i) dv.d[i] = ldexp(dv.d[i], -E);
                    for (int i = 0; i < 3; ++i) kick[i] = ldexp(kick[i], -E);
                    dv.log2 += E;
                    ++gr.renorms;
                }
            }
            if (rec) rec[at] = dv;
            growth[at] = gr;
            if (st.last) continue;
            for (int i = 0; i < 3; ++i) {
                dv.d[3 + i] = dv.d[3 + i] + kick[i];
                dv.d[i] = dv.d[i] + dv.d[3 + i] * st.dt;
            }
            cur[at] = dv;
        }
    }
};

// before evaluation 0: the orbit's stage; the vectors of a tracer that starts non-finite are NaN throughout
__global__ __launch_bounds__(kThreads) void stability_stage_kernel(uint32_t m, OrbitFrame f, uint32_t rotating,
                                                                   double c, double s, double *__restrict__ xs,
                                                                   double *__restrict__ vs,
                                                                   uint32_t *__restrict__ coinc,
                                                                   float4 *__restrict__ pts, uint32_t D,
                                                                   nb_orbit_deviation *__restrict__ cur) {
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= m) return;
    if (orbit_stage(p, f, rotating, c, s, xs, vs, coinc, pts)) return;
    for (uint32_t d = 0; d < D; ++d)
        for (int i = 0; i < 6; ++i) cur[(size_t)p * D + d].d[i] = (double)NAN;
}

__global__ __launch_bounds__(kThreads) void stability_step_kernel(
    const double *__restrict__ slab, uint32_t chunks, uint32_t stride, uint32_t p0, uint32_t p1, OrbitStep st,
    OrbitFrame f, double *__restrict__ xs, double *__restrict__ vs, uint32_t *__restrict__ coinc,
    float4 *__restrict__ pts, nb_orbit_sample *__restrict__ rec, StabilityRide ride) {
    orbit_step(slab, chunks, stride, p0, p1, st, f, xs, vs, coinc, pts, rec, ride);
}

struct StabilityWork : Workspace {  // (all grow to the largest call so far)
    DeviceBuf<nb_orbit_deviation> cur;    // [m][D]
    DeviceBuf<nb_orbit_deviation> recs;   // [records][m][D]
    DeviceBuf<nb_orbit_growth> growth;    // [m][D]
    PinnedBuf<nb_orbit_deviation> h_cur;  // as cur: the caller's vectors
    PinnedBuf<nb_orbit_deviation> h_recs;
    PinnedBuf<nb_orbit_growth> h_growth;
};

// this unit in the sequence of nb_orbits_sim
struct StabilityRider final : OrbitRider {
    const nb_orbit_stability_params &params;
    const nb_orbit_deviation *dev0;
    nb_orbit_deviation *devs;
    nb_orbit_growth *growth;
    float e;
    StabilityWork *w = nullptr;
    size_t vectors = 0, samples = 0;  // m D, records m D

    StabilityRider(const nb_orbit_stability_params &p, const nb_orbit_deviation *d0, nb_orbit_deviation *d,
                   nb_orbit_growth *g, float e_)
        : params(p), dev0(d0), devs(d), growth(g), e(e_) {
        name = "orbit_stability";
        slab_fields = kStabilityFields;
    }
    int reserve(SimBase &sim, uint32_t m, uint32_t records) override {
        if (int rc = workspace(sim, kWorkStability, &w, [](StabilityWork &) { return NB_OK; })) return rc;
        vectors = (size_t)m * params.deviations;
        samples = vectors * records;
        NB_HIP_TRY(w->cur.reserve(vectors));
        NB_HIP_TRY(w->recs.reserve(samples));
        NB_HIP_TRY(w->growth.reserve(vectors));
        NB_HIP_TRY(w->h_cur.reserve(vectors));
        NB_HIP_TRY(w->h_recs.reserve(samples));
        NB_HIP_TRY(w->h_growth.reserve(vectors));
        return NB_OK;
    }
    int upload(hipStream_t stream) override {
        std::memcpy(w->h_cur, dev0, sizeof(nb_orbit_deviation) * vectors);
        NB_HIP_TRY(hipMemcpyAsync(w->cur, w->h_cur, sizeof(nb_orbit_deviation) * vectors, hipMemcpyHostToDevice,
                                  stream));
        return NB_OK;
    }
    void stage(hipStream_t stream, uint32_t m, const OrbitFrame &f, const OrbitStep &st,
               const OrbitDevice &d) override {
        hipLaunchKernelGGL(stability_stage_kernel, dim3((m + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, m,
                           f, st.rotating, st.cn, st.sn, d.x, d.v, d.coinc, d.pts, params.deviations,
                           (nb_orbit_deviation *)w->cur);
    }
    // the instantiations the shared points per lane can ask for
    void pairs(int ib, const OrbitBand &b) override {
        if (ib == 1)
            launch_pairs<StabilityRule, 1>(b, e);
        else if (ib == 2)
            launch_pairs<StabilityRule, 2>(b, e);
        else
            launch_pairs<StabilityRule, 4>(b, e);
    }
    void step(const OrbitBand &b, const OrbitStep &st, const OrbitFrame &f, const OrbitDevice &d,
              nb_orbit_sample *rec, uint32_t record, uint64_t step) override {
        StabilityRide ride{};
        ride.D = params.deviations;
        ride.renorm_log2 = params.renorm_log2;
        ride.step = step;
        ride.cur = w->cur;
        ride.growth = w->growth;
        ride.rec = rec ? (nb_orbit_deviation *)w->recs + (size_t)record * vectors : nullptr;
        hipLaunchKernelGGL(stability_step_kernel, finish_grid(b), dim3(kThreads), 0, b.stream, (const double *)b.slab,
                           b.chunks, b.stride, b.p0, b.p1, st, f, d.x, d.v, d.coinc, d.pts, rec, ride);
    }
    int download(hipStream_t stream) override {
        NB_HIP_TRY(hipMemcpyAsync(w->h_recs, w->recs, sizeof(nb_orbit_deviation) * samples, hipMemcpyDeviceToHost,
                                  stream));
        NB_HIP_TRY(hipMemcpyAsync(w->h_growth, w->growth, sizeof(nb_orbit_growth) * vectors, hipMemcpyDeviceToHost,
                                  stream));
        return NB_OK;
    }
    void deliver() override {
        std::memcpy(devs, w->h_recs, sizeof(nb_orbit_deviation) * samples);
        if (growth) std::memcpy(growth, w->h_growth, sizeof(nb_orbit_growth) * vectors);
    }
};

}  // namespace

int sim_orbit_stability(SimBase &sim, const nb_orbit_params &P, const nb_orbit_stability_params &sp,
                        const OrbitPlan &frame, const double *pos, const double *vel, size_t m,
                        const nb_orbit_deviation *dev0, nb_orbit_sample *tracks, uint32_t *coincident,
                        nb_orbit_deviation *devs, nb_orbit_growth *growth, nb_orbit_stability_stats *stats) {
    StabilityRider rider(sp, dev0, devs, growth, sim.params.e);
    nb_orbit_stats os{};
    if (int rc = sim_orbits_with(sim, P, frame, pos, vel, m, tracks, coincident, &os, rider)) return rc;
    if (stats) {
        nb_orbit_stability_stats s{};
        s.orbit = os;
        s.deviations = sp.deviations;
        s.renorm_log2 = sp.renorm_log2;
        if (m > 0 && rider.w)
            for (size_t i = 0; i < rider.vectors; ++i) s.renorms += rider.w->h_growth[i].renorms;
        *stats = s;
    }
    return NB_OK;
}

}  // namespace nb
