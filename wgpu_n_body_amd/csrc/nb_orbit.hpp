// nb_orbit.hpp -- the step of a tracer through the frozen field (include/nbody.h "Orbits"), stated once
// for the units whose kernels run it: nb_field.hip (nb_orbits_sim, nb_orbit_sections_sim) and nb_stability.hip
// (nb_orbit_stability_sim).  Here are the frame, the constants of an evaluation, the point of an evaluation, the
// stage kernel, and orbit_step: the lines that finish the field's sums and move x and v, with a Ride -- what else
// the unit's step kernel does with state k -- handed the state before the next step begins.
// Every line that rounds is compiled without contraction (the pragmas), whatever the unit's own setting is.
#pragma once

#include "nb_probe.hpp"

namespace nb {
namespace orbit {

using probe::kThreads;

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

// the lines that turn a sampled vector back by +theta_k: the acceleration's, and a deviation's kick
__device__ __forceinline__ void orbit_turn_back(const double (&as)[3], const OrbitFrame &f, double c, double s,
                                                double (&a)[3]) {
#pragma clang fp contract(off)
    const double u = (as[0] * f.e1[0] + as[1] * f.e1[1]) + as[2] * f.e1[2];
    const double v = (as[0] * f.e2[0] + as[1] * f.e2[1]) + as[2] * f.e2[2];
    const double t = (as[0] * f.n[0] + as[1] * f.n[1]) + as[2] * f.n[2];
    const double ur = u * c - v * s, vr = v * c + u * s;
    for (int i = 0; i < 3; ++i) a[i] = (ur * f.e1[i] + vr * f.e2[i]) + t * f.n[i];
}

// before evaluation 0: a tracer that starts non-finite is NaN throughout; the first point
__device__ __forceinline__ bool orbit_stage(uint32_t p, const OrbitFrame &f, uint32_t rotating, double c, double s,
                                            double *__restrict__ xs, double *__restrict__ vs,
                                            uint32_t *__restrict__ coinc, float4 *__restrict__ pts) {
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
    return ok;
}

// A Ride has
//   kSlabFields, kCount                 -- the fields of the unit's slab and which of them is the coincident count;
//                                          fields 0..2 are the acceleration's sums and, with the potential among
//                                          the evaluation's flags, field 3 is the psi sum
//   state(p, in, chunks, stride, ok, x, v, st, f)
//                                       -- state k of tracer p, after the record and before the next step:
//                                          `in` is the tracer's place in chunk 0 of the slab, ok whether its point
//                                          was finite
// and NoRide is the step alone.
struct NoRide {
    static constexpr uint32_t kSlabFields = 5, kCount = 4;
    __device__ __forceinline__ void state(uint32_t, const double *, uint32_t, uint32_t, bool, const double (&)[3],
                                          const double (&)[3], const OrbitStep &, const OrbitFrame &) const {}
};

// after the pairs of evaluation k for the band [p0, p1): the chunks in order and the scaling by g as
// field_finish_kernel has them, then accel_scale, the turn back, the second half-kick, the record if one is due
// (rec = the record's row, or null), the ride, the first half-kick and the drift of the next step, and the next
// point.  vs holds v_0 on entry to evaluation 0 and w afterwards.
template <class Ride>
__device__ __forceinline__ void orbit_step(const double *__restrict__ slab, uint32_t chunks, uint32_t stride,
                                           uint32_t p0, uint32_t p1, const OrbitStep &st, const OrbitFrame &f,
                                           double *__restrict__ xs, double *__restrict__ vs,
                                           uint32_t *__restrict__ coinc, float4 *__restrict__ pts,
                                           nb_orbit_sample *__restrict__ rec, const Ride &ride) {
#pragma clang fp contract(off)
    constexpr uint32_t kSlabFields = Ride::kSlabFields, kCount = Ride::kCount;
    const uint32_t q = blockIdx.x * kThreads + threadIdx.x, p = p0 + q;
    if (p >= p1) return;
    const float4 pt = pts[p];
    const bool ok = isfinite(pt.x) && isfinite(pt.y) && isfinite(pt.z);
    const uint32_t flags = st.field_flags;
    double s[5] = {};
    for (uint32_t c = 0; c < chunks; ++c) {
        const double *in = slab + (size_t)c * kSlabFields * stride + q;
        for (int k = 0; k < 3; ++k) s[k] += in[(size_t)k * stride];
        if (flags & NB_FIELD_POTENTIAL) s[3] += in[(size_t)3 * stride];
        s[4] += in[(size_t)kCount * stride];
    }
    const bool pot = ok && (flags & NB_FIELD_POTENTIAL);
    double as[3];  // A_snap
    for (int k = 0; k < 3; ++k) as[k] = st.scale * (ok ? st.g * s[k] : (double)NAN);
    const double phi = st.scale * (pot ? -(st.g * s[3]) : (double)NAN);
    coinc[p] += ok ? (uint32_t)s[4] : 0u;

    double a[3] = {as[0], as[1], as[2]};
    if (st.rotating) orbit_turn_back(as, f, st.ck, st.sk, a);

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
    ride.state(p, slab + q, chunks, stride, ok, x, v, st, f);
    if (st.last) return;
    for (int i = 0; i < 3; ++i) {
        v[i] = v[i] + kick[i];      // w = v_k + A_k h
        x[i] = x[i] + v[i] * st.dt;  // x_{k+1} = x_k + w dt
        xs[3 * (size_t)p + i] = x[i];
        vs[3 * (size_t)p + i] = v[i];
    }
    pts[p] = orbit_point(x, f, st.rotating, st.cn, st.sn);
}

// ---- host: what a unit outside nb_field.hip puts into the sequence of nb_orbits_sim (orbits_run) ----
// The sequence -- the refusals, the plan, the state's upload, the stage, per evaluation and band one pair launch
// and one step launch, the copies ahead of the one synchronisation -- stays stated once, in nb_field.hip; a rider
// supplies its own slab layout, pair kernel and step kernel, and what it keeps on the device besides x and v.
// Its calls run in the order they are listed; every launch and copy goes to `stream`.
using OrbitBand = probe::Band<nb_field_sample>;
struct OrbitDevice {  // the sequence's own buffers, as the step kernel takes them
    double *x, *v;
    uint32_t *coinc;
    float4 *pts;
};
struct OrbitRider {
    const char *name;      // of the pass, for a refusal
    uint32_t slab_fields;  // of its pair kernel's slab
    virtual ~OrbitRider() = default;
    virtual int reserve(SimBase &sim, uint32_t m, uint32_t records) = 0;
    virtual int upload(hipStream_t stream) = 0;  // before the stage
    virtual void stage(hipStream_t stream, uint32_t m, const OrbitFrame &f, const OrbitStep &st,
                       const OrbitDevice &d) = 0;
    virtual void pairs(int ib, const OrbitBand &b) = 0;
    // evaluation k = step - step0 of the band; rec and record: the row of the tracks and its number, or null and
    // unspecified when state k is not recorded
    virtual void step(const OrbitBand &b, const OrbitStep &st, const OrbitFrame &f, const OrbitDevice &d,
                      nb_orbit_sample *rec, uint32_t record, uint64_t step) = 0;
    virtual int download(hipStream_t stream) = 0;  // ahead of the synchronisation
    virtual void deliver() = 0;                    // after it: pinned memory to the caller's
};

}  // namespace orbit

// nb_field.hip: nb_orbits_sim's sequence with a rider (a call with NB_ORBIT_ENERGY is the caller's to refuse)
int sim_orbits_with(SimBase &sim, const nb_orbit_params &params, const OrbitPlan &plan, const double *pos,
                    const double *vel, size_t m, nb_orbit_sample *tracks, uint32_t *coincident, nb_orbit_stats *stats,
                    orbit::OrbitRider &rider);

}  // namespace nb
