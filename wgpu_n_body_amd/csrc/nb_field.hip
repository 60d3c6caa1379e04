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
//   sections -- nb_orbit_sections_sim (include/nbody.h "Orbit sections"): the same sequence with the
//              step kernel's sibling, which also compares every state with the tracer's previous one, stores the
//              plane crossings and keeps the tracer's summary.  No launch is added.
//   The step's own lines are nb_orbit.hpp's, shared with nb_stability.hip, which joins the sequence below as a rider.
// The non-finite count is the diagnostics' own (diag_enqueue_moments on the same stream).
// No float atomics; the grid and the chunking depend on (M, N, flags) alone and every lane runs the same
// operations in the same order, so the result is bitwise reproducible and does not depend on where in
// the array a point stands.
#include "nb_orbit.hpp"
#include "nb_probe.hpp"
#include "nb_psi.hpp"

namespace nb {

using namespace probe;
using namespace orbit;

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
static_assert(kSlabFields == NoRide::kSlabFields && NoRide::kCount == FieldRule<kAcc>::kSums,
              "orbit_step reads the slab this unit's pair kernels write");

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

// ---- orbits: what a step does besides the pairs, one thread per tracer of a band: orbit_step of nb_orbit.hpp ----
__global__ __launch_bounds__(kThreads) void orbit_stage_kernel(uint32_t m, OrbitFrame f, uint32_t rotating, double c,
                                                               double s, double *__restrict__ xs,
                                                               double *__restrict__ vs, uint32_t *__restrict__ coinc,
                                                               float4 *__restrict__ pts) {
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= m) return;
    orbit_stage(p, f, rotating, c, s, xs, vs, coinc, pts);
}

// ---- orbit sections (include/nbody.h "Orbit sections"): what the step kernel does with state k
// besides the step.  One thread per tracer, so a tracer's list needs no atomics and is in time order; every row is
// indexed by the tracer, never by its place in a band.
enum : int { kPrevXi = 0, kPrevEta = 3, kPrevS = 6, kPrevD = 7, kPrevA = 8, kPrevB = 9, kPrevFields = 10 };
struct OrbitSection {
    double normal[3], offset;
    int32_t direction;
    uint32_t max_crossings, m;
    uint64_t step;               // step0 + k of this state; the bracket that ends here began at step - 1
    double *prev;                // [kPrevFields][m] the previous state's xi, eta, s, D, a, b
    nb_orbit_crossing *cross;    // [m][max_crossings], zeroed before the first launch
    uint32_t *counts;            // [m]
    nb_orbit_summary *summary;   // [m]
};

__device__ __forceinline__ bool sign_up(double y0, double y1) { return y0 < 0.0 && y1 >= 0.0; }
__device__ __forceinline__ bool sign_down(double y0, double y1) { return y0 >= 0.0 && y1 < 0.0; }

__device__ __forceinline__ void orbit_section(uint32_t p, const double (&x)[3], const double (&v)[3],
                                              const OrbitStep &st, const OrbitFrame &f, const OrbitSection &sc) {
#pragma clang fp contract(off)
    const double dx = x[0] - f.c[0], dy = x[1] - f.c[1], dz = x[2] - f.c[2];
    const double a = (dx * f.e1[0] + dy * f.e1[1]) + dz * f.e1[2];
    const double b = (dx * f.e2[0] + dy * f.e2[1]) + dz * f.e2[2];
    const double l = (dx * f.n[0] + dy * f.n[1]) + dz * f.n[2];
    const double ar = a * st.ck + b * st.sk, br = b * st.ck - a * st.sk;
    const double u = (v[0] * f.e1[0] + v[1] * f.e1[1]) + v[2] * f.e1[2];
    const double w = (v[0] * f.e2[0] + v[1] * f.e2[1]) + v[2] * f.e2[2];
    const double t = (v[0] * f.n[0] + v[1] * f.n[1]) + v[2] * f.n[2];
    const double ur = u * st.ck + w * st.sk, wr = w * st.ck - u * st.sk;
    const double xi[3] = {ar, br, l};
    double eta[3] = {ur, wr, t};
    if (st.rotating) {
        eta[0] = ur + st.omega * br;
        eta[1] = wr - st.omega * ar;
    }
    const double s = ((sc.normal[0] * ar + sc.normal[1] * br) + sc.normal[2] * l) - sc.offset;
    const double D = (dx * v[0] + dy * v[1]) + dz * v[2];
    const double L = (f.n[0] * (dy * v[2] - dz * v[1]) + f.n[1] * (dz * v[0] - dx * v[2])) +
                     f.n[2] * (dx * v[1] - dy * v[0]);
    const double R2 = ar * ar + br * br, r2 = R2 + l * l, h = fabs(l);

    nb_orbit_summary sm;
    uint32_t count = 0;
    if (st.first) {
        sm = nb_orbit_summary{};
        sm.r2_min = sm.R2_min = sm.lz_min = (double)INFINITY;
        sm.r2_max = sm.R2_max = sm.lz_max = sm.h_max = -(double)INFINITY;
        sm.first_peri = sm.last_peri = NB_ORBIT_NO_STEP;
    } else {
        sm = sc.summary[p];
        count = sc.counts[p];
    }
    if (r2 < sm.r2_min) sm.r2_min = r2;
    if (r2 > sm.r2_max) sm.r2_max = r2;
    if (R2 < sm.R2_min) sm.R2_min = R2;
    if (R2 > sm.R2_max) sm.R2_max = R2;
    if (h > sm.h_max) sm.h_max = h;
    if (L < sm.lz_min) sm.lz_min = L;
    if (L > sm.lz_max) sm.lz_max = L;

    double *prev = sc.prev + p;
    const size_t m = sc.m;
    if (!st.first) {
        double pxi[3], peta[3];
        for (int i = 0; i < 3; ++i) {
            pxi[i] = prev[(kPrevXi + i) * m];
            peta[i] = prev[(kPrevEta + i) * m];
        }
        const double ps = prev[kPrevS * m], pD = prev[kPrevD * m], pa = prev[kPrevA * m], pb = prev[kPrevB * m];
        const bool up = sign_up(ps, s), down = sign_down(ps, s);
        if ((up && sc.direction >= 0) || (down && sc.direction <= 0)) {
            if (count < sc.max_crossings) {
                const double fr = ps / (ps - s);
                nb_orbit_crossing c;
                for (int i = 0; i < 3; ++i) {
                    c.xi[i] = pxi[i] + fr * (xi[i] - pxi[i]);
                    c.eta[i] = peta[i] + fr * (eta[i] - peta[i]);
                }
                c.time = (double)(sc.step - 1) * st.dt + fr * st.dt;
                c.step = sc.step - 1;
                sc.cross[(size_t)p * sc.max_crossings + count] = c;
            }
            ++count;
        }
        if (sign_up(pD, D)) {
            ++sm.pericentres;
            if (sm.first_peri == NB_ORBIT_NO_STEP) sm.first_peri = sc.step;
            sm.last_peri = sc.step;
        }
        if (sign_down(pD, D)) ++sm.apocentres;
        if (sign_up(pxi[2], l)) ++sm.plane_ups;
        // windings: a sign change of the second coordinate on the positive side of the first
        const bool bu = sign_up(pxi[1], br), bd = sign_down(pxi[1], br);
        if (bu || bd) {
            const double fb = pxi[1] / (pxi[1] - br);
            if (pxi[0] + fb * (ar - pxi[0]) > 0.0) sm.winding_pattern += bu ? 1 : -1;
        }
        const bool iu = sign_up(pb, b), id = sign_down(pb, b);
        if (iu || id) {
            const double fb = pb / (pb - b);
            if (pa + fb * (a - pa) > 0.0) sm.winding_inertial += iu ? 1 : -1;
        }
    }
    sc.summary[p] = sm;
    sc.counts[p] = count;
    if (st.last) return;
    for (int i = 0; i < 3; ++i) {
        prev[(kPrevXi + i) * m] = xi[i];
        prev[(kPrevEta + i) * m] = eta[i];
    }
    prev[kPrevS * m] = s;
    prev[kPrevD * m] = D;
    prev[kPrevA * m] = a;
    prev[kPrevB * m] = b;
}

// the section as orbit_step's ride
struct SectionRide {
    static constexpr uint32_t kSlabFields = NoRide::kSlabFields, kCount = NoRide::kCount;
    OrbitSection sc;
    __device__ __forceinline__ void state(uint32_t p, const double *, uint32_t, uint32_t, bool, const double (&x)[3],
                                          const double (&v)[3], const OrbitStep &st, const OrbitFrame &f) const {
        orbit_section(p, x, v, st, f, sc);
    }
};

__global__ __launch_bounds__(kThreads) void orbit_step_kernel(const double *__restrict__ slab, uint32_t chunks,
                                                              uint32_t stride, uint32_t p0, uint32_t p1, OrbitStep st,
                                                              OrbitFrame f, double *__restrict__ xs,
                                                              double *__restrict__ vs, uint32_t *__restrict__ coinc,
                                                              float4 *__restrict__ pts,
                                                              nb_orbit_sample *__restrict__ rec) {
    orbit_step(slab, chunks, stride, p0, p1, st, f, xs, vs, coinc, pts, rec, NoRide{});
}

// the same step with the section riding in it (include/nbody.h "Orbit sections")
__global__ __launch_bounds__(kThreads) void orbit_section_step_kernel(
    const double *__restrict__ slab, uint32_t chunks, uint32_t stride, uint32_t p0, uint32_t p1, OrbitStep st,
    OrbitFrame f, double *__restrict__ xs, double *__restrict__ vs, uint32_t *__restrict__ coinc,
    float4 *__restrict__ pts, nb_orbit_sample *__restrict__ rec, OrbitSection sec) {
    orbit_step(slab, chunks, stride, p0, p1, st, f, xs, vs, coinc, pts, rec, SectionRide{sec});
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
    // orbit sections: the previous state's row, the lists, their lengths and the summaries, by tracer
    DeviceBuf<double> prev;              // [kPrevFields][m]
    DeviceBuf<nb_orbit_crossing> cross;  // [m][max_crossings]
    DeviceBuf<uint32_t> counts;          // [m]
    DeviceBuf<nb_orbit_summary> summary;  // [m]
    PinnedBuf<nb_orbit_crossing> h_cross;
    PinnedBuf<uint32_t> h_counts;
    PinnedBuf<nb_orbit_summary> h_summary;
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

// what an nb_orbit_sections_sim call adds to the arguments of nb_orbits_sim
struct SectionCall {
    const nb_orbit_section_params &params;
    nb_orbit_crossing *crossings;
    uint32_t *counts;
    nb_orbit_summary *summaries;
    nb_orbit_section_stats *stats;
};

// nb_orbits_sim, and with `section` nb_orbit_sections_sim: the same sequence, the step kernel's sibling in the place
// of the step kernel, a memset up front and three copies at the end; with `rider` (nb_orbit.hpp) another unit's
// slab, pair kernel and step kernel in the same places
static int orbits_run(SimBase &sim, const nb_orbit_params &P, const OrbitPlan &frame, const double *pos,
                      const double *vel, size_t m, nb_orbit_sample *tracks, uint32_t *coincident,
                      nb_orbit_stats *stats, const SectionCall *section, OrbitRider *rider = nullptr) {
    if (int rc = refuse_sharded(sim, rider ? rider->name : section ? "orbit_sections" : "orbits")) return rc;
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
    const uint32_t fields = rider ? rider->slab_fields : kSlabFields;
    const size_t slab_a = (size_t)plan_a.chunks * fields * plan_a.stride;
    const size_t slab_e = (size_t)plan_e.chunks * kSlabFields * plan_e.stride;
    NB_HIP_TRY(w.slab.reserve(energy ? std::max(slab_a, slab_e) : slab_a));
    if (rider)
        if (int rc = rider->reserve(sim, mm, records)) return rc;
    const OrbitDevice dev{w.x, w.v, w.coinc, w.pts};
    OrbitSection sc{};
    const size_t slots = section ? (size_t)mm * section->params.max_crossings : 0;
    if (section) {
        NB_HIP_TRY(w.prev.reserve((size_t)kPrevFields * mm));
        NB_HIP_TRY(w.cross.reserve(slots));
        NB_HIP_TRY(w.counts.reserve(mm));
        NB_HIP_TRY(w.summary.reserve(mm));
        NB_HIP_TRY(w.h_cross.reserve(slots));
        NB_HIP_TRY(w.h_counts.reserve(mm));
        NB_HIP_TRY(w.h_summary.reserve(mm));
        for (int a = 0; a < 3; ++a) sc.normal[a] = section->params.normal[a];
        sc.offset = section->params.offset;
        sc.direction = section->params.direction;
        sc.max_crossings = section->params.max_crossings;
        sc.m = mm;
        sc.prev = w.prev;
        sc.cross = w.cross;
        sc.counts = w.counts;
        sc.summary = w.summary;
    }

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
            if (slots)
                NB_HIP_TRY(hipMemsetAsync((nb_orbit_crossing *)w.cross, 0, sizeof(nb_orbit_crossing) * slots, sim.stream));
            if (int rc = orbit_phase(P.omega, P.dt, P.step0, &st.cn, &st.sn)) return rc;
            if (rider) {
                if (int rc = rider->upload(sim.stream)) return rc;
                rider->stage(sim.stream, mm, f, st, dev);
            } else {
                hipLaunchKernelGGL(orbit_stage_kernel, dim3((mm + kThreads - 1) / kThreads), dim3(kThreads), 0,
                                   sim.stream, mm, f, st.rotating, st.cn, st.sn, dev.x, dev.v, dev.coinc, dev.pts);
            }
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
                sc.step = P.step0 + k;
                b.n_tiles = pl.n_tiles;
                b.cj = pl.cj;
                b.chunks = pl.chunks;
                b.stride = pl.stride;
                for (b.tile0 = 0; b.tile0 < pl.p_tiles; b.tile0 += pl.band) {
                    b.tiles = std::min(pl.band, pl.p_tiles - b.tile0);
                    b.p0 = b.tile0 * pl.tile_pts;
                    b.p1 = std::min(mm, (b.tile0 + b.tiles) * pl.tile_pts);
                    if (n > 0) {
                        if (rider)
                            rider->pairs(ib, b);
                        else
                            launch_field(st.field_flags, ib, b, c);
                        NB_HIP_TRY(hipGetLastError());
                        ++launches;
                    }
                    if (rider)
                        rider->step(b, st, f, dev, rec, r - 1, sc.step);
                    else if (section)
                        hipLaunchKernelGGL(orbit_section_step_kernel, finish_grid(b), dim3(kThreads), 0, sim.stream,
                                           (const double *)w.slab, b.chunks, b.stride, b.p0, b.p1, st, f,
                                           (double *)w.x, (double *)w.v, (uint32_t *)w.coinc, (float4 *)w.pts, rec,
                                           sc);
                    else
                        hipLaunchKernelGGL(orbit_step_kernel, finish_grid(b), dim3(kThreads), 0, sim.stream,
                                           (const double *)w.slab, b.chunks, b.stride, b.p0, b.p1, st, f,
                                           (double *)w.x, (double *)w.v, (uint32_t *)w.coinc, (float4 *)w.pts, rec);
                    NB_HIP_TRY(hipGetLastError());
                }
            }
            NB_HIP_TRY(hipMemcpyAsync(w.h_tracks, w.tracks, sizeof(nb_orbit_sample) * samples, hipMemcpyDeviceToHost,
                                      sim.stream));
            NB_HIP_TRY(hipMemcpyAsync(w.h_coinc, w.coinc, sizeof(uint32_t) * mm, hipMemcpyDeviceToHost, sim.stream));
            if (rider)
                if (int rc = rider->download(sim.stream)) return rc;
            if (section) {
                if (slots)
                    NB_HIP_TRY(hipMemcpyAsync(w.h_cross, w.cross, sizeof(nb_orbit_crossing) * slots,
                                              hipMemcpyDeviceToHost, sim.stream));
                NB_HIP_TRY(hipMemcpyAsync(w.h_counts, w.counts, sizeof(uint32_t) * mm, hipMemcpyDeviceToHost,
                                          sim.stream));
                NB_HIP_TRY(hipMemcpyAsync(w.h_summary, w.summary, sizeof(nb_orbit_summary) * mm,
                                          hipMemcpyDeviceToHost, sim.stream));
            }
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
    if (rider && mm > 0) rider->deliver();
    if (section) {
        nb_orbit_section_stats ss{};
        const uint32_t cap = section->params.max_crossings;
        for (uint32_t i = 0; i < mm; ++i) {
            const uint32_t c = w.h_counts[i];
            ss.crossings += c;
            ss.stored += std::min(c, cap);
            ss.overflowed += c > cap;
        }
        if (mm > 0) {
            if (slots) std::memcpy(section->crossings, w.h_cross, sizeof(nb_orbit_crossing) * slots);
            if (section->counts) std::memcpy(section->counts, w.h_counts, sizeof(uint32_t) * mm);
            if (section->summaries) std::memcpy(section->summaries, w.h_summary, sizeof(nb_orbit_summary) * mm);
        }
        if (section->stats) *section->stats = ss;
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

int sim_orbits(SimBase &sim, const nb_orbit_params &P, const OrbitPlan &frame, const double *pos, const double *vel,
               size_t m, nb_orbit_sample *tracks, uint32_t *coincident, nb_orbit_stats *stats) {
    return orbits_run(sim, P, frame, pos, vel, m, tracks, coincident, stats, nullptr);
}

int sim_orbits_with(SimBase &sim, const nb_orbit_params &P, const OrbitPlan &frame, const double *pos,
                    const double *vel, size_t m, nb_orbit_sample *tracks, uint32_t *coincident, nb_orbit_stats *stats,
                    OrbitRider &rider) {
    return orbits_run(sim, P, frame, pos, vel, m, tracks, coincident, stats, nullptr, &rider);
}

int sim_orbit_sections(SimBase &sim, const nb_orbit_params &P, const nb_orbit_section_params &sec,
                       const OrbitPlan &frame, const double *pos, const double *vel, size_t m, nb_orbit_sample *tracks,
                       uint32_t *coincident, nb_orbit_crossing *crossings, uint32_t *counts,
                       nb_orbit_summary *summaries, nb_orbit_section_stats *stats) {
    const SectionCall call{sec, crossings, counts, summaries, stats};
    return orbits_run(sim, P, frame, pos, vel, m, tracks, coincident, stats ? &stats->orbit : nullptr, &call);
}

}  // namespace nb
