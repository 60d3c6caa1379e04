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
//   orbits  -- nb_orbits_sim (include/nbody.h "Orbits"): tracers kept on the device and moved through
//              the frozen field by the same pair launches; per step and band one more kernel, one thread per
//              tracer, is the finish above and everything else of the step.  Its lines are compiled without
//              contraction (the pragma); the pair kernels are the instantiations field() launches.
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

// ---- orbits: what a step does besides the pairs, one thread per tracer of a band --------------------------------
struct OrbitFrame {
    double e1[3], e2[3], n[3], c[3];
};
struct OrbitStep {
    double g, scale, h, dt, omega;
    double ck, sk;         // the phase of this evaluation: turns the acceleration back
    double cn, sn;         // the phase of the next one: turns the next point
    uint32_t field_flags;  // F_k
    uint32_t rotating, energy, first, last;
};

// q = c + R(-theta) (x - c) in the frame, rounded once to fp32: the point of an evaluation
__device__ __forceinline__ float4 orbit_point(const double (&x)[3], const OrbitFrame &f, bool rotating, double c,
                                               double s) {
#pragma clang fp contract(off)
    double q[3] = {x[0], x[1], x[2]};
    if (rotating) {
        const double dx = x[0] - f.c[0], dy = x[1] - f.c[1], dz = x[2] - f.c[2];
        const double a = (dx * f.e1[0] + dy * f.e1[1]) + dz * f.e1[2];
        const double b = (dx * f.e2[0] + dy * f.e2[1]) + dz * f.e2[2];
        const double l = (dx * f.n[0] + dy * f.n[1]) + dz * f.n[2];
        const double ar = a * c + b * s, br = b * c - a * s;
        for (int i = 0; i < 3; ++i) q[i] = f.c[i] + ((ar * f.e1[i] + br * f.e2[i]) + l * f.n[i]);
    }
    return make_float4((float)q[0], (float)q[1], (float)q[2], 0.f);
}

// before evaluation 0: a tracer that starts non-finite is NaN throughout; the first point
__global__ __launch_bounds__(kThreads) void orbit_stage_kernel(uint32_t m, OrbitFrame f, uint32_t rotating, double c,
                                                               double s, double *__restrict__ xs,
                                                               double *__restrict__ vs, uint32_t *__restrict__ coinc,
                                                               float4 *__restrict__ pts) {
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= m) return;
    double x[3], v[3];
    bool ok = true;
    for (int i = 0; i < 3; ++i) {
        x[i] = xs[3 * (size_t)p + i];
        v[i] = vs[3 * (size_t)p + i];
        ok = ok && isfinite(x[i]) && isfinite(v[i]);
    }
    if (!ok)
        for (int i = 0; i < 3; ++i) xs[3 * (size_t)p + i] = vs[3 * (size_t)p + i] = x[i] = (double)NAN;
    coinc[p] = 0;
    pts[p] = orbit_point(x, f, rotating, c, s);
}

// after the pairs of evaluation k for the band [p0, p1): the chunks in order and the scaling by g as
// field_finish_kernel has them, then accel_scale, the turn back, the second half-kick, the record if one is due
// (rec = the record's row, or null), the first half-kick and the drift of the next step, and the next point.
// vs holds v_0 on entry to evaluation 0 and w afterwards.
__global__ __launch_bounds__(kThreads) void orbit_step_kernel(const double *__restrict__ slab, uint32_t chunks,
                                                              uint32_t stride, uint32_t p0, uint32_t p1, OrbitStep st,
                                                              OrbitFrame f, double *__restrict__ xs,
                                                              double *__restrict__ vs, uint32_t *__restrict__ coinc,
                                                              float4 *__restrict__ pts,
                                                              nb_orbit_sample *__restrict__ rec) {
#pragma clang fp contract(off)
    const uint32_t q = blockIdx.x * kThreads + threadIdx.x, p = p0 + q;
    if (p >= p1) return;
    const float4 pt = pts[p];
    const bool ok = isfinite(pt.x) && isfinite(pt.y) && isfinite(pt.z);
    const uint32_t flags = st.field_flags;
    double s[kSlabFields] = {};
    for (uint32_t c = 0; c < chunks; ++c) {
        const double *in = slab + (size_t)c * kSlabFields * stride + q;
        for (int k = 0; k < 3; ++k) s[k] += in[(size_t)k * stride];
        if (flags & NB_FIELD_POTENTIAL) s[3] += in[(size_t)3 * stride];
        s[4] += in[(size_t)4 * stride];
    }
    const bool pot = ok && (flags & NB_FIELD_POTENTIAL);
    double as[3];  // A_snap
    for (int k = 0; k < 3; ++k) as[k] = st.scale * (ok ? st.g * s[k] : (double)NAN);
    const double phi = st.scale * (pot ? -(st.g * s[3]) : (double)NAN);
    coinc[p] += ok ? (uint32_t)s[4] : 0u;

    double a[3] = {as[0], as[1], as[2]};
    if (st.rotating) {
        const double u = (as[0] * f.e1[0] + as[1] * f.e1[1]) + as[2] * f.e1[2];
        const double v = (as[0] * f.e2[0] + as[1] * f.e2[1]) + as[2] * f.e2[2];
        const double t = (as[0] * f.n[0] + as[1] * f.n[1]) + as[2] * f.n[2];
        const double ur = u * st.ck - v * st.sk, vr = v * st.ck + u * st.sk;
        for (int i = 0; i < 3; ++i) a[i] = (ur * f.e1[i] + vr * f.e2[i]) + t * f.n[i];
    }

    double x[3], v[3], kick[3];
    for (int i = 0; i < 3; ++i) {
        x[i] = xs[3 * (size_t)p + i];
        v[i] = vs[3 * (size_t)p + i];
        kick[i] = a[i] * st.h;
        if (!st.first) v[i] = v[i] + kick[i];  // v_k = w + A_k h
    }
    if (rec) {
        nb_orbit_sample r;
        for (int i = 0; i < 3; ++i) {
            r.pos[i] = x[i];
            r.vel[i] = v[i];
        }
        r.potential = r.energy = (double)NAN;
        if (st.energy) {
            double e = 0.5 * ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + phi;
            if (st.rotating) {
                const double dx = x[0] - f.c[0], dy = x[1] - f.c[1], dz = x[2] - f.c[2];
                const double l = (f.n[0] * (dy * v[2] - dz * v[1]) + f.n[1] * (dz * v[0] - dx * v[2])) +
                                 f.n[2] * (dx * v[1] - dy * v[0]);
                e = e - st.omega * l;
            }
            r.potential = phi;
            r.energy = e;
        }
        rec[p] = r;
    }
    if (st.last) return;
    for (int i = 0; i < 3; ++i) {
        v[i] = v[i] + kick[i];      // w = v_k + A_k h
        x[i] = x[i] + v[i] * st.dt;  // x_{k+1} = x_k + w dt
        xs[3 * (size_t)p + i] = x[i];
        vs[3 * (size_t)p + i] = v[i];
    }
    pts[p] = orbit_point(x, f, st.rotating, st.cn, st.sn);
}

struct OrbitWork : Workspace {  // (all but the last grow to the largest call so far)
    DeviceBuf<double> x, v;             // [3 m] the state between the launches (v: v_0, then w)
    DeviceBuf<uint32_t> coinc;          // [m]
    DeviceBuf<float4> pts;              // [m] the staged points
    DeviceBuf<double> slab;             // [chunks][slab fields][points of one band]
    DeviceBuf<nb_orbit_sample> tracks;  // [records][m]
    PinnedBuf<double> h_in;             // [6 m] pos, then vel
    PinnedBuf<nb_orbit_sample> h_tracks;
    PinnedBuf<uint32_t> h_coinc;
    PinnedBuf<double> h_bad;  // [1] the diagnostics' non-finite count
};

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

int sim_orbits(SimBase &sim, const nb_orbit_params &P, const OrbitPlan &frame, const double *pos, const double *vel,
               size_t m, nb_orbit_sample *tracks, uint32_t *coincident, nb_orbit_stats *stats) {
    if (int rc = refuse_sharded(sim, "orbits")) return rc;
    const uint32_t n = sim.n, mm = (uint32_t)m, steps = P.steps, records = frame.records;
    const bool energy = P.flags & NB_ORBIT_ENERGY, rotating = P.omega != 0.0;
    // the plans of the two kinds of evaluation: field()'s own for m points and the flags of each
    const uint32_t flags_a = NB_FIELD_ACCEL, flags_e = NB_FIELD_ACCEL | NB_FIELD_POTENTIAL;
    const int ib_a = points_per_lane(m, flags_a), ib_e = points_per_lane(m, flags_e);
    const Plan plan_a = plan(mm, n, ib_a, sim.field_pairs_log2), plan_e = plan(mm, n, ib_e, sim.field_pairs_log2);
    const uint64_t m_pad = energy ? std::max(plan_a.m_pad, plan_e.m_pad) : plan_a.m_pad;
    // m_pad <= 2^20 + 255, n < 2^32, steps + 1 <= 2^20 + 1: the product may pass 2^64, so it is formed in fp64
    if (m_pad && n && (double)m_pad * (double)n * (double)(steps + 1ull) > std::ldexp(1.0, NB_ORBIT_MAX_PAIRS_LOG2)) {
        set_error("orbits: %llu padded tracers x %u bodies x %u evaluations are more than 2^%d pairs: split the call "
                  "(step0 continues a run exactly)", (unsigned long long)m_pad, n, steps + 1, NB_ORBIT_MAX_PAIRS_LOG2);
        return NB_ERR_UNSUPPORTED;
    }
    if (int rc = sim.bind_device()) return rc;

    OrbitWork *work = nullptr;
    if (int rc = workspace(sim, kWorkOrbits, &work, [](OrbitWork &f) {
            NB_HIP_TRY(f.h_bad.reserve(1));
            return NB_OK;
        }))
        return rc;
    OrbitWork &w = *work;
    const size_t samples = (size_t)records * mm;
    NB_HIP_TRY(w.x.reserve(3 * (size_t)mm));
    NB_HIP_TRY(w.v.reserve(3 * (size_t)mm));
    NB_HIP_TRY(w.coinc.reserve(mm));
    NB_HIP_TRY(w.pts.reserve(mm));
    NB_HIP_TRY(w.tracks.reserve(samples));
    NB_HIP_TRY(w.h_in.reserve(6 * (size_t)mm));
    NB_HIP_TRY(w.h_tracks.reserve(samples));
    NB_HIP_TRY(w.h_coinc.reserve(mm));
    const size_t slab_a = (size_t)plan_a.chunks * kSlabFields * plan_a.stride;
    const size_t slab_e = (size_t)plan_e.chunks * kSlabFields * plan_e.stride;
    NB_HIP_TRY(w.slab.reserve(energy ? std::max(slab_a, slab_e) : slab_a));

    OrbitFrame f{};
    for (int a = 0; a < 3; ++a) {
        f.e1[a] = frame.e1[a];
        f.e2[a] = frame.e2[a];
        f.n[a] = frame.n[a];
        f.c[a] = P.center[a];
    }
    const PsiConst c = n > 0 ? psi_const(sim.params.e) : PsiConst{};
    OrbitStep st{};
    st.g = (double)sim.params.g;
    st.scale = P.accel_scale;
    st.h = P.dt / 2;
    st.dt = P.dt;
    st.omega = P.omega;
    st.rotating = rotating;
    st.energy = energy;

    uint64_t bad_tracers = 0;
    uint32_t launches = 0;
    *w.h_bad = 0.0;
    if (mm > 0) {
        for (uint32_t i = 0; i < mm; ++i) {
            bool ok = true;
            for (int a = 0; a < 3; ++a) {
                const double x = pos[3 * (size_t)i + a], v = vel[3 * (size_t)i + a];
                w.h_in[3 * (size_t)i + a] = x;
                w.h_in[3 * ((size_t)mm + i) + a] = v;
                ok = ok && std::isfinite(x) && std::isfinite(v);
            }
            bad_tracers += !ok;
        }
        // from here the pinned state is being read: an error drains the stream before it returns
        const int rc = [&]() -> int {
            const size_t bytes = sizeof(double) * 3 * mm;
            NB_HIP_TRY(hipMemcpyAsync(w.x, w.h_in, bytes, hipMemcpyHostToDevice, sim.stream));
            NB_HIP_TRY(hipMemcpyAsync(w.v, w.h_in + 3 * (size_t)mm, bytes, hipMemcpyHostToDevice, sim.stream));
            Band<nb_field_sample> b{};
            b.stream = sim.stream;
            b.n = n;
            b.pts = w.pts;
            b.m = mm;
            b.slab = w.slab;
            if (n > 0) {
                sim.diag_state(&b.posm, &b.vel);
                const double *mom = nullptr;  // the bodies nb_sim_diagnostics counts as non-finite, once
                if (int rc = diag_enqueue_moments(sim, &mom)) return rc;
                NB_HIP_TRY(hipMemcpyAsync(w.h_bad, mom + kDiagResBad, sizeof(double), hipMemcpyDeviceToHost, sim.stream));
            }
            if (int rc = orbit_phase(P.omega, P.dt, P.step0, &st.cn, &st.sn)) return rc;
            hipLaunchKernelGGL(orbit_stage_kernel, dim3((mm + kThreads - 1) / kThreads), dim3(kThreads), 0, sim.stream,
                               mm, f, st.rotating, st.cn, st.sn, (double *)w.x, (double *)w.v, (uint32_t *)w.coinc,
                               (float4 *)w.pts);
            NB_HIP_TRY(hipGetLastError());
            uint32_t r = 0;
            for (uint32_t k = 0; k <= steps; ++k) {
                const bool due = k % P.every == 0 || k == steps;
                const bool both = energy && due;
                const Plan &pl = both ? plan_e : plan_a;
                const int ib = both ? ib_e : ib_a;
                st.field_flags = both ? flags_e : flags_a;
                st.first = k == 0;
                st.last = k == steps;
                st.ck = st.cn;
                st.sk = st.sn;
                if (!st.last)
                    if (int rc = orbit_phase(P.omega, P.dt, P.step0 + k + 1, &st.cn, &st.sn)) return rc;
                nb_orbit_sample *rec = due ? (nb_orbit_sample *)w.tracks + (size_t)r++ * mm : nullptr;
                b.n_tiles = pl.n_tiles;
                b.cj = pl.cj;
                b.chunks = pl.chunks;
                b.stride = pl.stride;
                for (b.tile0 = 0; b.tile0 < pl.p_tiles; b.tile0 += pl.band) {
                    b.tiles = std::min(pl.band, pl.p_tiles - b.tile0);
                    b.p0 = b.tile0 * pl.tile_pts;
                    b.p1 = std::min(mm, (b.tile0 + b.tiles) * pl.tile_pts);
                    if (n > 0) {
                        launch_field(st.field_flags, ib, b, c);
                        NB_HIP_TRY(hipGetLastError());
                        ++launches;
                    }
                    hipLaunchKernelGGL(orbit_step_kernel, finish_grid(b), dim3(kThreads), 0, sim.stream,
                                       (const double *)w.slab, b.chunks, b.stride, b.p0, b.p1, st, f, (double *)w.x,
                                       (double *)w.v, (uint32_t *)w.coinc, (float4 *)w.pts, rec);
                    NB_HIP_TRY(hipGetLastError());
                }
            }
            NB_HIP_TRY(hipMemcpyAsync(w.h_tracks, w.tracks, sizeof(nb_orbit_sample) * samples, hipMemcpyDeviceToHost,
                                      sim.stream));
            NB_HIP_TRY(hipMemcpyAsync(w.h_coinc, w.coinc, sizeof(uint32_t) * mm, hipMemcpyDeviceToHost, sim.stream));
            return NB_OK;
        }();
        if (rc != NB_OK) {
            (void)hipStreamSynchronize(sim.stream);
            return rc;
        }
    }
    NB_HIP_TRY(hipStreamSynchronize(sim.stream));
    if (int rc = sim.diag_status()) return rc;
    if (mm > 0) {
        std::memcpy(tracks, w.h_tracks, sizeof(nb_orbit_sample) * samples);
        if (coincident) std::memcpy(coincident, w.h_coinc, sizeof(uint32_t) * mm);
    }
    if (stats) {
        nb_orbit_stats s{};
        s.step_num = sim.step_num;
        s.n = n;
        s.nonfinite = (uint64_t)*w.h_bad;
        s.tracers = m;
        s.nonfinite_tracers = bad_tracers;
        s.records = records;
        s.pair_launches = launches;
        s.flags = P.flags;
        *stats = s;
    }
    return NB_OK;
}

}  // namespace nb
