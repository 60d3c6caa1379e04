// simulator.hpp -- header-only C++17 host mirror of the reference's simulation API, over the
// C ABI of include/nbody.h.  The reference is a Rust crate and this image has no Rust
// toolchain, so the host side a Rust user would see is written here in C++ with the same
// names, argument meaning and error behaviour:
//
//   sims::SimParams / AddParams / Particle   (src/sims/mod.rs:9-23,51-71)  -> nbody::SimParams ...
//   trait sims::Simulator                    (src/sims/mod.rs:73-90)       -> nbody::Simulator
//   sims::NaiveSim, sims::TreeSim            (src/sims/mod.rs:4-5)         -> nbody::NaiveSim, TreeSim
//   runners::OfflineHeadless<T>              (src/runners/offline_headless.rs) -> nbody::OfflineHeadless<T>
//   inits::{uniform,disc,spherical}_init     (src/inits.rs)                -> nbody::inits::*
//
// Constructors return anyhow::Result in the reference; here they throw nbody::Error
// (status code + nb_last_error() text).  step() panics on failure in the reference
// (src/sims/tree.rs:278-280); here it throws.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <functional>
#include <limits>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "nbody.h"

namespace nbody {

using Particle = nb_particle;    // 40 B
using SimParams = nb_sim_params;  // 16 B
using Octant = nb_octant;        // 52 B
using Diagnostics = nb_diagnostics;  // conserved-quantity monitor (no reference counterpart)
using RadialParams = nb_radial_params;    // bins, flags, centre, axis and edges of a radial profile
using RadialBin = nb_radial_bin;          // 88 B
using FieldSample = nb_field_sample;      // 40 B: acceleration, potential and coincident count at a point
using FieldRing = nb_field_ring;          // a ring's means: a_R, a_n, potential, v_c
using TidalSample = nb_tidal_sample;      // 56 B: the tidal tensor (xx, yy, zz, xy, xz, yz) and coincident count at a point
using OrbitSample = nb_orbit_sample;      // 64 B: position, velocity, potential and energy of a tracer at a recorded state
using TidalRing = nb_tidal_ring;          // a ring's means of the tensor, and omega2, kappa2, nu2
using MapParams = nb_map_params;          // grid, window, line of sight and centre of a projected map
using MapStats = nb_map_stats;
using PhaseParams = nb_phase_params;      // quantities, flags, centre and axis of a phase map (the edges are set by the call)
using PhaseStats = nb_phase_stats;
using FofGroup = nb_fof_group;            // 80 B: label, count and the nine sums of a catalogued group
using FofStats = nb_fof_stats;
using BoundGroup = nb_bound_group;        // 128 B: a catalogued group's bound set
using BoundStats = nb_bound_stats;
using ShapeGroup = nb_shape_group;        // 360 B: a row's sums, eigenvalues, axes and axis ratios
using ShapeStats = nb_shape_stats;
using RadiiGroup = nb_radii_group;        // 264 B: a row's mass radii, extent and peak of M / r
using RadiiStats = nb_radii_stats;
using HopBoundary = nb_hop_boundary;      // 24 B: two labels, their body pairs and the largest pair density
using HopStats = nb_hop_stats;
using MstStats = nb_mst_stats;            // the counts, the rounds and the plan of nb_mst_sim
using KnnStats = nb_knn_stats;            // the counts, the density-weighted sums and the peak of nb_sim_knn
using KinStats = nb_kin_stats;            // the counts of nb_local_kinematics_sim
using KinDerived = nb_kin_derived;        // 256 B: a body's local mean velocity, dispersion, Q and velocity gradient
using HaloHead = nb_halo_head;            // 64 B: what lies inside edges[0], the centre and velocity used, flags
using HaloStats = nb_halo_stats;
using SmoothParams = nb_smooth_params;    // a map's parameters and the bounds of the smoothing lengths
using SmoothStats = nb_smooth_stats;
using Camera = nb_camera;               // `Camera`, runners/online_renderer.rs:12-20
using RenderParams = nb_render_params;  // size, view-projection matrix and constants of the draw pass
using RenderStats = nb_render_stats;

inline SimParams default_sim_params() {  // SimParams::default(), sims/mod.rs:62-71
    return SimParams{NB_DEFAULT_PARTICLE_NUM, NB_DEFAULT_G, NB_DEFAULT_E, NB_DEFAULT_DT};
}

struct AddParams {  // enum AddParams, sims/mod.rs:18-23
    nb_add_params c{NB_NAIVE_SIM_PARAMS, 0.0f};
    static AddParams NaiveSimParams() { return AddParams{}; }
    static AddParams TreeSimParams(float theta) {
        AddParams a;
        a.c = nb_add_params{NB_TREE_SIM_PARAMS, theta};
        return a;
    }
};

class Error : public std::runtime_error {
   public:
    Error(int code, const std::string &what) : std::runtime_error(what), code_(code) {}
    int code() const { return code_; }

   private:
    int code_;
};

inline void check(int rc) {
    if (rc != NB_OK) throw Error(rc, std::string("nbody_hip: ") + nb_last_error());
}

inline Camera default_camera(uint32_t width, uint32_t height) {  // online_renderer.rs:231-239
    Camera c{};
    check(nb_camera_default(&c, width, height));
    return c;
}
inline RenderParams default_render_params(uint32_t width, uint32_t height) {
    RenderParams p{};
    check(nb_render_params_default(&p, width, height));
    return p;
}
inline RenderParams render_params(const Camera &cam, uint32_t width, uint32_t height) {
    RenderParams p = default_render_params(width, height);
    check(nb_camera_view_proj(&cam, p.view_proj));  // Camera::build_view_projection_matrix
    return p;
}

// nbins + 1 radii from rmin to rmax, constant ratio (log) or constant step
inline std::vector<double> radial_edges(double rmin, double rmax, uint32_t nbins, bool log = true) {
    std::vector<double> e((size_t)nbins + 1);
    check((log ? nb_radial_edges_log : nb_radial_edges_linear)(rmin, rmax, nbins, e.data()));
    return e;
}

// A radial profile (no reference counterpart): the header, the bins and the edges they lie between
struct RadialProfile {
    nb_radial_profile profile{};
    std::vector<RadialBin> bins;
    std::vector<double> edges;
    // radii enclosing the given fractions of profile.mass (binned: limited by the bins' resolution)
    std::vector<double> lagrangian(const std::vector<double> &fractions) const {
        std::vector<double> r(fractions.size());
        check(nb_radial_lagrangian(&profile, bins.data(), edges.data(), fractions.data(), (uint32_t)fractions.size(),
                                   r.data()));
        return r;
    }
};

namespace detail {
template <class H>
RadialProfile radial_profile(int (*call)(H *, const nb_radial_params *, nb_radial_profile *, nb_radial_bin *), H *h,
                             const std::vector<double> &edges, RadialParams p) {
    RadialProfile r;
    r.edges = edges;
    r.bins.resize(edges.size() > 1 ? edges.size() - 1 : 1);
    p.nbins = edges.empty() ? 0u : (uint32_t)(edges.size() - 1);
    p.edges = r.edges.data();
    check(call(h, &p, &r.profile, r.bins.data()));
    return r;
}
}  // namespace detail

// The azimuthal Fourier sums of a disc per annulus (nb_disc_modes_sim; no reference counterpart): the header, the
// bins, modes[nbins][mmax + 1][6] in the order NB_MODES_C .. NB_MODES_ZS, and the edges they lie between
using ModesParams = nb_modes_params;      // 96 B
using ModesBin = nb_modes_bin;            // 24 B: count, sum mu R, sum mu h^2
using ModesDerived = nb_modes_derived;    // 40 B: amplitude, phase, pattern speed, bending amplitude and phase
struct BarStrength {
    double a2;    // the largest A_2 / A_0 over the bins with mass (NaN: none)
    int bin;      // the bin it occurs in (-1: none)
};
struct DiscModes {
    nb_modes_head head{};
    std::vector<ModesBin> bins;
    std::vector<double> modes;
    std::vector<double> edges;
    double dt = 0.0;  // the simulator's time step (pattern_speed_between)
    double field(size_t bin, uint32_t m, uint32_t f) const { return modes[(bin * (head.mmax + 1) + m) * NB_MODES_FIELDS + f]; }
    // mode m (1 <= m <= mmax) of every bin: nb_disc_modes_derive
    std::vector<ModesDerived> derived(uint32_t m) const {
        std::vector<ModesDerived> d(bins.size());
        check(nb_disc_modes_derive(modes.data(), head.nbins, head.mmax, m, d.data()));
        return d;
    }
    BarStrength bar_strength() const {
        const std::vector<ModesDerived> d = derived(2);
        BarStrength b{std::nan(""), -1};
        for (size_t k = 0; k < d.size(); ++k)
            if (std::isfinite(d[k].amplitude) && field(k, 0, NB_MODES_C) != 0.0 && (b.bin < 0 || d[k].amplitude > b.a2))
                b = BarStrength{d[k].amplitude, (int)k};
        return b;
    }
    // 2 hypot(ZC_1, ZS_1) / sum mu R: the tilt of the annulus' plane
    double warp_tilt(size_t bin) const {
        return 2.0 * std::hypot(field(bin, 1, NB_MODES_ZC), field(bin, 1, NB_MODES_ZS)) / bins[bin].m_r;
    }
    // sqrt(sum mu h^2 / C_0 - (ZC_0 / C_0)^2): the rms height about the mean height
    double thickness(size_t bin) const {
        const double c0 = field(bin, 0, NB_MODES_C), mean = field(bin, 0, NB_MODES_ZC) / c0;
        return std::sqrt(std::max(bins[bin].m_h2 / c0 - mean * mean, 0.0));
    }
    // the six sums of mode m over all bins, the bins added in order
    std::array<double, 6> total(uint32_t m) const {
        std::array<double, 6> t{};
        for (size_t k = 0; k < bins.size(); ++k)
            for (uint32_t f = 0; f < NB_MODES_FIELDS; ++f) t[f] = t[f] + field(k, m, f);
        return t;
    }
    // the pattern speed of mode m per bin from two measurements: the phase difference wrapped into (-pi/m, pi/m]
    // over `time` (<= 0: the steps between the two times dt)
    std::vector<double> pattern_speed_between(const DiscModes &other, uint32_t m, double time = 0.0) const {
        const std::vector<ModesDerived> a = derived(m), b = other.derived(m);
        if (!(time > 0.0)) time = ((double)other.head.step_num - (double)head.step_num) * dt;
        const double period = 2.0 * 3.14159265358979323846 / (double)m;
        std::vector<double> w(a.size());
        for (size_t k = 0; k < a.size(); ++k) {
            const double x = b[k].phase - a[k].phase;
            w[k] = (x - period * std::ceil(x / period - 0.5)) / time;
        }
        return w;
    }
};

namespace detail {
// p: mmax, flags (NB_MODES_CENTER_COM), centre, velocity and axis (nbins and edges are set here)
template <class H>
DiscModes disc_modes(int (*call)(H *, const nb_modes_params *, nb_modes_head *, nb_modes_bin *, double *), H *h,
                     double dt, const std::vector<double> &edges, ModesParams p) {
    DiscModes r;
    r.edges = edges;
    r.dt = dt;
    r.bins.resize(edges.size() > 1 ? edges.size() - 1 : 1);
    r.modes.resize(r.bins.size() * (std::min<size_t>(p.mmax, NB_MODES_MAX_M) + 1) * NB_MODES_FIELDS);
    p.nbins = edges.empty() ? 0u : (uint32_t)(edges.size() - 1);
    p.edges = r.edges.data();
    check(call(h, &p, &r.head, r.bins.data(), r.modes.data()));
    return r;
}
}  // namespace detail

// The spherical-harmonic sums per radial shell (nb_shell_modes_sim; no reference counterpart): the header, the bins,
// coef[nbins][(lmax + 1)^2 (1 + rates)] (sum i of (l, m): l^2, l^2 + 2m - 1 for C, l^2 + 2m for S; the rates in a
// second block) and the edges they lie between
using ShellParams = nb_shell_params;    // 96 B
using ShellBin = nb_shell_bin;          // 24 B: count, sum mu r, sum mu u_r
using ShellDerived = nb_shell_derived;  // 232 B: power and relative power per l, the l = 1 vector, the l = 2 axes
struct ShellModes {
    nb_shell_head head{};
    std::vector<ShellBin> bins;
    std::vector<double> coef;
    std::vector<double> edges;
    double dt = 0.0;  // the simulator's time step (phase_between)
    bool rates() const { return (head.flags & NB_SHELL_RATES) != 0; }
    size_t terms() const { return (size_t)(head.lmax + 1) * (head.lmax + 1); }
    static size_t index(uint32_t l, uint32_t m, bool sine = false) { return (size_t)l * l + (m ? 2 * m - (sine ? 0 : 1) : 0); }
    // sum (l, m) of a bin: the cosine sum, or with sine the sine sum (m >= 1)
    double coefficient(size_t bin, uint32_t l, uint32_t m, bool sine = false) const {
        return coef[bin * terms() * (rates() ? 2 : 1) + index(l, m, sine)];
    }
    // ... and its time derivative (needs NB_SHELL_RATES)
    double rate(size_t bin, uint32_t l, uint32_t m, bool sine = false) const {
        return coef[bin * terms() * 2 + terms() + index(l, m, sine)];
    }
    // nb_shell_modes_derive: one record per bin; norm, phase and speed are null or resized to nbins (lmax + 1)^2
    std::vector<ShellDerived> derived(std::vector<double> *norm = nullptr, std::vector<double> *phase = nullptr,
                                      std::vector<double> *speed = nullptr) const {
        std::vector<ShellDerived> d(bins.size());
        for (std::vector<double> *v : {norm, phase, speed})
            if (v) v->assign(bins.size() * terms(), 0.0);
        check(nb_shell_modes_derive(&head, coef.data(), d.data(), norm ? norm->data() : nullptr,
                                    phase ? phase->data() : nullptr, speed ? speed->data() : nullptr));
        return d;
    }
    // sum_m a_lm^2 / (2l + 1) per bin, and sqrt(power_l / power_0)
    std::vector<double> power(uint32_t l) const { return per_l(l, false); }
    std::vector<double> relative(uint32_t l) const { return per_l(l, true); }
    // the l = 1 vector per bin, in the state's coordinates
    std::vector<std::array<double, 3>> dipole() const {
        const std::vector<ShellDerived> d = derived();
        std::vector<std::array<double, 3>> out(d.size());
        for (size_t k = 0; k < d.size(); ++k) std::copy(d[k].dipole, d[k].dipole + 3, out[k].begin());
        return out;
    }
    // the l = 2 tensor's eigenvalues, descending, and unit vectors (axes[3 j + i]: component i of vector j) per bin
    std::pair<std::vector<std::array<double, 3>>, std::vector<std::array<double, 9>>> quadrupole_axes() const {
        const std::vector<ShellDerived> d = derived();
        std::vector<std::array<double, 3>> values(d.size());
        std::vector<std::array<double, 9>> axes(d.size());
        for (size_t k = 0; k < d.size(); ++k) {
            std::copy(d[k].quad_values, d[k].quad_values + 3, values[k].begin());
            std::copy(d[k].quad_axes, d[k].quad_axes + 9, axes[k].begin());
        }
        return {values, axes};
    }
    // atan2(S, C) / m of component (l, m) per bin
    std::vector<double> phase(uint32_t l, uint32_t m) const { return column(l, m, 1); }
    // (C DS - S DC) / (m (C^2 + S^2)) per bin: the rate at which component (l, m) turns about the axis
    std::vector<double> pattern_speed(uint32_t l, uint32_t m) const { return column(l, m, 2); }
    // the phase difference of component (l, m) per bin between two measurements, wrapped into (-pi/m, pi/m]
    std::vector<double> phase_between(const ShellModes &other, uint32_t l, uint32_t m) const {
        const std::vector<double> a = phase(l, m), b = other.phase(l, m);
        const double period = 2.0 * 3.14159265358979323846 / (double)m;
        std::vector<double> w(a.size());
        for (size_t k = 0; k < a.size(); ++k) {
            const double x = b[k] - a[k];
            w[k] = x - period * std::ceil(x / period - 0.5);
        }
        return w;
    }

   private:
    std::vector<double> per_l(uint32_t l, bool relative_to_l0) const {
        if (l > head.lmax) throw std::invalid_argument("ShellModes: needs l <= lmax");
        const std::vector<ShellDerived> d = derived();
        std::vector<double> out(d.size());
        for (size_t k = 0; k < d.size(); ++k) out[k] = relative_to_l0 ? d[k].relative[l] : d[k].power[l];
        return out;
    }
    std::vector<double> column(uint32_t l, uint32_t m, int which) const {
        if (m < 1 || m > l || l > head.lmax) throw std::invalid_argument("ShellModes: needs 1 <= m <= l <= lmax");
        std::vector<double> all, out(bins.size());
        derived(nullptr, which == 1 ? &all : nullptr, which == 2 ? &all : nullptr);
        for (size_t k = 0; k < out.size(); ++k) out[k] = all[k * terms() + index(l, m)];
        return out;
    }
};

namespace detail {
// p: lmax, flags (NB_SHELL_CENTER_COM, NB_SHELL_RATES), centre, velocity and axis (nbins and edges are set here)
template <class H>
ShellModes shell_modes(int (*call)(H *, const nb_shell_params *, nb_shell_head *, nb_shell_bin *, double *), H *h,
                       double dt, const std::vector<double> &edges, ShellParams p) {
    ShellModes r;
    r.edges = edges;
    r.dt = dt;
    r.bins.resize(edges.size() > 1 ? edges.size() - 1 : 1);
    const size_t lm = std::min<size_t>(p.lmax, NB_SHELL_MAX_L) + 1;
    r.coef.resize(r.bins.size() * lm * lm * 2);  // (the call refuses what it does not take)
    p.nbins = edges.empty() ? 0u : (uint32_t)(edges.size() - 1);
    p.edges = r.edges.data();
    check(call(h, &p, &r.head, r.bins.data(), r.coef.data()));
    r.coef.resize(r.bins.size() * r.terms() * (r.rates() ? 2 : 1));
    return r;
}
}  // namespace detail

// The field at a set of points (no reference counterpart): the samples and what the call measured
struct Field {
    std::vector<FieldSample> samples;
    nb_field_stats stats{};
};

// k * n_phi points (3 floats each, ring-major) on the rings of the given radii about `axis` through `center`
inline std::vector<float> field_rings(const std::vector<double> &radii, const std::array<double, 3> &axis,
                                      const std::array<double, 3> &center, uint32_t n_phi) {
    std::vector<float> pts(3 * radii.size() * (size_t)n_phi);
    check(nb_field_rings(center.data(), axis.data(), radii.data(), (uint32_t)radii.size(), n_phi, pts.data()));
    return pts;
}

// A rotation curve from the force: per ring the means of nb_field_ring_means, and the samples behind them
struct RingMeans {
    std::vector<double> radii;
    std::vector<FieldRing> rings;
    Field field;
};

namespace detail {
template <class H>
Field field(int (*call)(H *, const float *, size_t, uint32_t, nb_field_sample *, nb_field_stats *), H *h,
            const std::vector<float> &points, uint32_t flags) {
    Field f;
    f.samples.resize(points.size() / 3);
    check(call(h, points.data(), points.size() / 3, flags, f.samples.data(), &f.stats));
    return f;
}
template <class H>
RingMeans circular_velocity(int (*call)(H *, const float *, size_t, uint32_t, nb_field_sample *, nb_field_stats *),
                            H *h, const std::vector<double> &radii, const std::array<double, 3> &axis,
                            const std::array<double, 3> &center, uint32_t n_phi, bool potential) {
    RingMeans r;
    r.radii = radii;
    const std::vector<float> pts = field_rings(radii, axis, center, n_phi);
    r.field = field(call, h, pts, NB_FIELD_ACCEL | (potential ? NB_FIELD_POTENTIAL : 0u));
    r.rings.resize(radii.size());
    check(nb_field_ring_means(center.data(), axis.data(), radii.data(), (uint32_t)radii.size(), n_phi, pts.data(),
                              r.field.samples.data(), r.rings.data()));
    return r;
}
}  // namespace detail

// The tidal tensor at a set of points (no reference counterpart): the samples and what the call measured
struct TidalField {
    std::vector<TidalSample> samples;
    nb_tidal_stats stats{};
    // the eigenvalues of sample i, descending, and their unit vectors (nb_shape_eigen)
    void eigen(size_t i, double lambda[3], double axes[9]) const {
        const double *s = samples[i].tensor;
        const double t[6] = {s[0], s[3], s[4], s[1], s[5], s[2]};  // nb_shape_eigen's order: xx, xy, xz, yy, yz, zz
        check(nb_shape_eigen(t, lambda, axes));
    }
    // the count of negative eigenvalues, 0 to 3: the cosmic-web class of the point (-1 where the tensor is not finite)
    int compressive_axes(size_t i) const {
        for (double v : samples[i].tensor)
            if (!std::isfinite(v)) return -1;
        double lambda[3], axes[9];
        eigen(i, lambda, axes);
        return (lambda[0] < 0.0) + (lambda[1] < 0.0) + (lambda[2] < 0.0);
    }
};

// A disc's frequencies from the force and its gradient: per ring the means of nb_tidal_ring_means, the field's ring
// means behind omega2 and v_c, and the tidal samples behind the rest
struct DiscFrequencies {
    std::vector<double> radii;
    std::vector<TidalRing> rings;
    RingMeans means;
    TidalField tidal;
    static double root(double x) { return x >= 0.0 ? std::sqrt(x) : std::nan(""); }  // NaN where the square is negative
    double omega(size_t i) const { return root(rings[i].omega2); }
    double kappa(size_t i) const { return root(rings[i].kappa2); }
    double nu(size_t i) const { return root(rings[i].nu2); }
};

namespace detail {
template <class H>
TidalField tidal_tensor(int (*call)(H *, const float *, size_t, nb_tidal_sample *, nb_tidal_stats *), H *h,
                        const std::vector<float> &points) {
    TidalField f;
    f.samples.resize(points.size() / 3);
    check(call(h, points.data(), points.size() / 3, f.samples.data(), &f.stats));
    return f;
}
template <class H>
DiscFrequencies disc_frequencies(int (*field_call)(H *, const float *, size_t, uint32_t, nb_field_sample *,
                                                   nb_field_stats *),
                                 int (*tidal_call)(H *, const float *, size_t, nb_tidal_sample *, nb_tidal_stats *),
                                 H *h, const std::vector<double> &radii, const std::array<double, 3> &axis,
                                 const std::array<double, 3> &center, uint32_t n_phi) {
    DiscFrequencies r;
    r.radii = radii;
    r.means = circular_velocity(field_call, h, radii, axis, center, n_phi, false);
    const std::vector<float> pts = field_rings(radii, axis, center, n_phi);
    r.tidal = tidal_tensor(tidal_call, h, pts);
    r.rings.resize(radii.size());
    check(nb_tidal_ring_means(center.data(), axis.data(), radii.data(), (uint32_t)radii.size(), n_phi, pts.data(),
                              r.tidal.samples.data(), r.means.rings.data(), r.rings.data()));
    return r;
}
}  // namespace detail

// Test particles in the frozen field of the current state (no reference counterpart): records * tracers samples,
// record-major, the coincident count per tracer, and what the call measured
struct Orbits {
    uint32_t records = 0;
    size_t tracers = 0;
    std::vector<OrbitSample> tracks;
    std::vector<uint32_t> coincident;
    nb_orbit_stats stats{};
    nb_orbit_params params{};
    const OrbitSample &at(uint32_t record, size_t tracer) const { return tracks[(size_t)record * tracers + tracer]; }
    // the step number of a record: step0 + k
    uint64_t step(uint32_t record) const {
        const uint64_t k = std::min<uint64_t>((uint64_t)record * params.every, params.steps);
        return params.step0 + k;
    }
};

// dt, steps and the rest of an orbits() call; accel_scale 1 is field()'s own coupling
inline nb_orbit_params orbit_params(double dt, uint32_t steps, uint32_t every = 1, bool energy = false,
                                    double omega = 0.0, const std::array<double, 3> &axis = {0.0, 1.0, 0.0},
                                    const std::array<double, 3> &center = {0.0, 0.0, 0.0}, double accel_scale = 1.0,
                                    uint64_t step0 = 0) {
    nb_orbit_params p{};
    p.dt = dt;
    p.step0 = step0;
    p.steps = steps;
    p.every = every;
    p.flags = energy ? NB_ORBIT_ENERGY : 0u;
    p.accel_scale = accel_scale;
    p.omega = omega;
    for (int a = 0; a < 3; ++a) {
        p.axis[a] = axis[(size_t)a];
        p.center[a] = center[(size_t)a];
    }
    return p;
}

namespace detail {
template <class H>
Orbits orbits(int (*call)(H *, const nb_orbit_params *, const double *, const double *, size_t, nb_orbit_sample *,
                          uint32_t *, nb_orbit_stats *),
              H *h, const nb_orbit_params &p, const std::vector<double> &pos, const std::vector<double> &vel) {
    if (pos.size() != vel.size() || pos.size() % 3) throw Error(NB_ERR_INVALID, "orbits: pos and vel are 3 doubles per tracer");
    Orbits o;
    o.params = p;
    o.tracers = pos.size() / 3;
    o.records = nb_orbit_records(p.steps, p.every);
    // (the call refuses what it does not take, before it writes)
    const bool big = o.tracers > NB_ORBIT_MAX_TRACERS || (uint64_t)o.records * o.tracers > NB_ORBIT_MAX_SAMPLES;
    o.tracks.resize(big ? 0 : (size_t)o.records * o.tracers);
    o.coincident.resize(o.tracers);
    check(call(h, &p, pos.data(), vel.data(), o.tracers, o.tracks.data(), o.coincident.data(), &o.stats));
    return o;
}
}  // namespace detail

// The surface of section and the summaries of an orbits() call (include/nbody.h "Orbit sections"): max_crossings
// slots per tracer, tracer-major, of which min(counts, max_crossings) are written, and one summary per tracer
struct OrbitSections {
    Orbits orbits;
    uint32_t max_crossings = 0;
    std::vector<nb_orbit_crossing> crossings;
    std::vector<uint32_t> counts;
    std::vector<nb_orbit_summary> summaries;
    nb_orbit_section_stats stats{};
    nb_orbit_section_params section{};
    uint32_t stored(size_t tracer) const { return std::min(counts[tracer], max_crossings); }
    const nb_orbit_crossing &at(size_t tracer, uint32_t j) const { return crossings[tracer * max_crossings + j]; }
};

// the plane normal . xi = offset of the pattern frame, the crossings kept (+1 up, -1 down, 0 both) and the room
inline nb_orbit_section_params orbit_section_params(const std::array<double, 3> &normal = {0.0, 1.0, 0.0},
                                                    double offset = 0.0, int32_t direction = 1,
                                                    uint32_t max_crossings = 256) {
    nb_orbit_section_params s{};
    for (int a = 0; a < 3; ++a) s.normal[a] = normal[(size_t)a];
    s.offset = offset;
    s.direction = direction;
    s.max_crossings = max_crossings;
    return s;
}

namespace detail {
template <class H>
OrbitSections orbit_sections(int (*call)(H *, const nb_orbit_params *, const nb_orbit_section_params *, const double *,
                                         const double *, size_t, nb_orbit_sample *, uint32_t *, nb_orbit_crossing *,
                                         uint32_t *, nb_orbit_summary *, nb_orbit_section_stats *),
                             H *h, const nb_orbit_params &p, const nb_orbit_section_params &sec,
                             const std::vector<double> &pos, const std::vector<double> &vel) {
    if (pos.size() != vel.size() || pos.size() % 3)
        throw Error(NB_ERR_INVALID, "orbit_sections: pos and vel are 3 doubles per tracer");
    OrbitSections o;
    o.section = sec;
    o.max_crossings = sec.max_crossings;
    Orbits &t = o.orbits;
    t.params = p;
    t.tracers = pos.size() / 3;
    t.records = nb_orbit_records(p.steps, p.every);
    // (the call refuses what it does not take, before it writes)
    const bool big = t.tracers > NB_ORBIT_MAX_TRACERS || (uint64_t)t.records * t.tracers > NB_ORBIT_MAX_SAMPLES ||
                     (uint64_t)t.tracers * sec.max_crossings > NB_ORBIT_SECTION_MAX_CROSSINGS;
    t.tracks.resize(big ? 0 : (size_t)t.records * t.tracers);
    t.coincident.resize(t.tracers);
    o.crossings.resize(big ? 0 : t.tracers * sec.max_crossings);
    o.counts.resize(t.tracers);
    o.summaries.resize(t.tracers);
    check(call(h, &p, &sec, pos.data(), vel.data(), t.tracers, t.tracks.data(), t.coincident.data(),
               o.crossings.empty() ? nullptr : o.crossings.data(), o.counts.data(), o.summaries.data(), &o.stats));
    t.stats = o.stats.orbit;
    return o;
}
}  // namespace detail

// The deviation vectors of an orbits() call (include/nbody.h "Orbit stability"): records * tracers * deviations
// vectors, record-major and vector-minor, each d * 2^log2; the growth per tracer and vector; and derive(), what
// nb_orbit_stability_derive reads from them
struct OrbitStability {
    Orbits orbits;
    uint32_t deviations = 0;
    std::vector<nb_orbit_deviation> dev0;  // [tracers][deviations] what the call began with
    std::vector<nb_orbit_deviation> devs;  // [records][tracers][deviations]
    std::vector<nb_orbit_growth> growth;   // [tracers][deviations]
    nb_orbit_stability_stats stats{};
    const nb_orbit_deviation &at(uint32_t record, size_t tracer, uint32_t j) const {
        return devs[((size_t)record * orbits.tracers + tracer) * deviations + j];
    }
    struct Derived {
        std::vector<double> log_growth, lyapunov;  // [records][tracers][deviations]
        std::vector<double> sali, gali2;           // [records][tracers]
    };
    Derived derive() const {
        Derived d;
        const size_t rows = (size_t)orbits.records * orbits.tracers;
        d.log_growth.resize(rows * deviations);
        d.lyapunov.resize(rows * deviations);
        d.sali.resize(rows);
        d.gali2.resize(rows);
        check(nb_orbit_stability_derive(orbits.params.dt, orbits.params.steps, orbits.params.every, orbits.tracers,
                                        deviations, dev0.data(), devs.data(), d.log_growth.data(), d.lyapunov.data(),
                                        d.sali.data(), d.gali2.data()));
        return d;
    }
};

namespace detail {
template <class H>
OrbitStability orbit_stability(int (*call)(H *, const nb_orbit_params *, const nb_orbit_stability_params *,
                                           const double *, const double *, size_t, const nb_orbit_deviation *,
                                           nb_orbit_sample *, uint32_t *, nb_orbit_deviation *, nb_orbit_growth *,
                                           nb_orbit_stability_stats *),
                               H *h, const nb_orbit_params &p, const std::vector<double> &pos,
                               const std::vector<double> &vel, const std::vector<nb_orbit_deviation> &dev0,
                               uint32_t renorm_log2) {
    if (pos.size() != vel.size() || pos.size() % 3)
        throw Error(NB_ERR_INVALID, "orbit_stability: pos and vel are 3 doubles per tracer");
    OrbitStability o;
    Orbits &t = o.orbits;
    t.params = p;
    t.tracers = pos.size() / 3;
    t.records = nb_orbit_records(p.steps, p.every);
    if (t.tracers == 0 || dev0.size() % t.tracers)
        throw Error(NB_ERR_INVALID, "orbit_stability: dev0 holds the same number of vectors for every tracer");
    o.deviations = (uint32_t)(dev0.size() / t.tracers);
    o.dev0 = dev0;
    nb_orbit_stability_params sp{};
    sp.deviations = o.deviations;
    sp.renorm_log2 = renorm_log2;
    // (the call refuses what it does not take, before it writes)
    const bool big = t.tracers > NB_ORBIT_MAX_TRACERS ||
                     (uint64_t)t.records * t.tracers * std::max(o.deviations, 1u) > NB_ORBIT_MAX_SAMPLES;
    t.tracks.resize(big ? 0 : (size_t)t.records * t.tracers);
    t.coincident.resize(t.tracers);
    o.devs.resize(big ? 0 : (size_t)t.records * dev0.size());
    o.growth.resize(dev0.size());
    check(call(h, &p, &sp, pos.data(), vel.data(), t.tracers, dev0.data(), t.tracks.data(), t.coincident.data(),
               o.devs.data(), o.growth.data(), &o.stats));
    t.stats = o.stats.orbit;
    return o;
}
}  // namespace detail

// A projected map (no reference counterpart): width * height counts, row 0 the smallest b, the planes
// (1, or 6 with NB_MAP_VELOCITY: mass, m_ua, m_ub, m_w, m_w2, m_u2) plane-major, and what the call measured
struct ProjectedMap {
    uint32_t width = 0, height = 0, nplanes = 0;
    std::vector<uint32_t> counts;
    std::vector<double> planes;
    MapStats stats{};
    const double *plane(uint32_t k) const { return planes.data() + (size_t)k * width * height; }
};

// The parameters of a map of the window [x0, x1) x [y0, y1) about the centre of mass, seen along `axis`,
// with the velocity planes and no depth cut
inline MapParams map_params(uint32_t width, uint32_t height, double x0, double x1, double y0, double y1,
                            const std::array<double, 3> &axis = {0.0, 1.0, 0.0}) {
    MapParams p{};
    p.width = width;
    p.height = height;
    p.flags = NB_MAP_CENTER_COM | NB_MAP_VELOCITY;
    for (int k = 0; k < 3; ++k) p.axis[k] = axis[(size_t)k];
    p.x_range[0] = x0;
    p.x_range[1] = x1;
    p.y_range[0] = y0;
    p.y_range[1] = y1;
    p.depth_range[0] = -HUGE_VAL;
    p.depth_range[1] = HUGE_VAL;
    return p;
}

namespace detail {
template <class H>
ProjectedMap projected_map(int (*call)(H *, const nb_map_params *, uint32_t *, double *, nb_map_stats *), H *h,
                           const MapParams &p) {
    ProjectedMap m;
    const bool ok = p.width >= 1 && p.width <= NB_MAP_MAX_SIDE && p.height >= 1 && p.height <= NB_MAP_MAX_SIDE &&
                    (uint64_t)p.width * p.height <= NB_MAP_MAX_CELLS;  // (the call refuses the sizes itself)
    m.width = ok ? p.width : 1;
    m.height = ok ? p.height : 1;
    m.nplanes = (p.flags & NB_MAP_VELOCITY) ? 6 : 1;
    m.counts.resize((size_t)m.width * m.height);
    m.planes.resize((size_t)m.nplanes * m.width * m.height);
    check(call(h, &p, m.counts.data(), m.planes.data(), &m.stats));
    return m;
}
}  // namespace detail

// A phase map (no reference counterpart): the bodies binned on two per-body quantities, x along the columns and y
// along the rows, width * height counts, the planes (1, or 3 with NB_PHASE_WEIGHT: mass, m_q, m_q2) plane-major,
// the edges they lie between and what the call measured
struct PhaseMap {
    uint32_t width = 0, height = 0, nplanes = 0;
    std::vector<uint32_t> counts;
    std::vector<double> planes;
    std::vector<double> x_edges, y_edges;
    PhaseStats stats{};
    const double *plane(uint32_t k) const { return planes.data() + (size_t)k * width * height; }
};

// the id of the per-body quantity called `name` (nb_phase_quantity)
inline uint32_t phase_quantity(const std::string &name) {
    uint32_t id = 0;
    check(nb_phase_quantity(name.c_str(), &id));
    return id;
}

// the cells + 1 edges of one side: nb_map_edges, or (log) a constant ratio from lo > 0 -- nb_radial_edges_log up to
// its NB_RADIAL_MAX_BINS bins, the same expression lo (hi / lo)^(k / cells) beyond
inline std::vector<double> phase_edges(double lo, double hi, uint32_t cells, bool log = false) {
    std::vector<double> e((size_t)cells + 1);
    if (!log) {
        check(nb_map_edges(lo, hi, cells, e.data()));
    } else if (cells <= NB_RADIAL_MAX_BINS) {
        check(nb_radial_edges_log(lo, hi, cells, e.data()));
    } else {
        if (!(lo > 0.0 && hi > lo && std::isfinite(hi))) throw std::invalid_argument("log edges need finite 0 < lo < hi");
        for (uint32_t k = 0; k <= cells; ++k) e[k] = lo * std::pow(hi / lo, (double)k / (double)cells);
        e[0] = lo;
        e[cells] = hi;
    }
    return e;
}

// The parameters of a phase map of x against y about the centre of mass in the frame of `axis`; weight: the name of
// the quantity to sum, or empty
inline PhaseParams phase_params(const std::string &x, const std::string &y, const std::string &weight = "",
                                const std::array<double, 3> &axis = {0.0, 1.0, 0.0}) {
    PhaseParams p{};
    p.x = phase_quantity(x);
    p.y = phase_quantity(y);
    p.q = weight.empty() ? (uint32_t)NB_PHASE_Q_MASS : phase_quantity(weight);
    p.flags = NB_PHASE_CENTER_COM | (weight.empty() ? 0u : NB_PHASE_WEIGHT);
    for (int k = 0; k < 3; ++k) p.axis[k] = axis[(size_t)k];
    p.step_num = NB_PHASE_ANY_STEP;
    return p;
}

namespace detail {
template <class H>
PhaseMap phase_map(int (*call)(H *, const nb_phase_params *, uint32_t *, double *, nb_phase_stats *), H *h,
                   PhaseParams p, const std::vector<double> &x_edges, const std::vector<double> &y_edges) {
    PhaseMap m;
    m.x_edges = x_edges;
    m.y_edges = y_edges;
    p.width = x_edges.empty() ? 0 : (uint32_t)(x_edges.size() - 1);
    p.height = y_edges.empty() ? 0 : (uint32_t)(y_edges.size() - 1);
    p.x_edges = m.x_edges.data();
    p.y_edges = m.y_edges.data();
    const bool ok = p.width >= 1 && p.width <= NB_MAP_MAX_SIDE && p.height >= 1 && p.height <= NB_MAP_MAX_SIDE &&
                    (uint64_t)p.width * p.height <= NB_MAP_MAX_CELLS;  // (the call refuses the sizes itself)
    m.width = ok ? p.width : 1;
    m.height = ok ? p.height : 1;
    m.nplanes = (p.flags & NB_PHASE_WEIGHT) ? 3 : 1;
    m.counts.resize((size_t)m.width * m.height);
    m.planes.resize((size_t)m.nplanes * m.width * m.height);
    check(call(h, &p, m.counts.data(), m.planes.data(), &m.stats));
    return m;
}
}  // namespace detail

// The friends-of-friends groups of a state (no reference counterpart): per body the label (the smallest body
// index of its group) and the catalogue row (NB_FOF_NONE: none), the catalogue in ascending label order
struct FofGroups {
    std::vector<uint32_t> labels, group_of;
    std::vector<FofGroup> groups;
    FofStats stats{};
    // the rows by count, descending, ties by label
    std::vector<uint32_t> by_size() const {
        std::vector<uint32_t> o(groups.size());
        for (size_t i = 0; i < o.size(); ++i) o[i] = (uint32_t)i;
        std::sort(o.begin(), o.end(), [this](uint32_t a, uint32_t b) {
            return groups[a].count != groups[b].count ? groups[a].count > groups[b].count : groups[a].label < groups[b].label;
        });
        return o;
    }
};

namespace detail {
template <class H>
FofGroups fof_groups(int (*call)(H *, const nb_fof_params *, uint32_t *, uint32_t *, nb_fof_group *, size_t,
                                 nb_fof_stats *),
                     H *h, size_t n, double link, uint32_t min_members, bool labels) {
    FofGroups g;
    nb_fof_params p{};
    p.link = link;
    p.min_members = min_members;
    const size_t cap = min_members ? n / min_members : 0;  // the most there can be (the call refuses 0 itself)
    if (labels) g.labels.resize(n);
    g.group_of.resize(n);
    g.groups.resize(cap);
    check(call(h, &p, labels ? g.labels.data() : nullptr, g.group_of.data(), g.groups.data(), cap, &g.stats));
    g.groups.resize((size_t)g.stats.groups);
    return g;
}
}  // namespace detail

// The phase-space groups of a state (nb_fof6_sim; no reference counterpart): friends-of-friends in position and
// velocity, with FofGroups' fields.  Every group lies inside one group of fof_groups(link).
struct PhaseSpaceGroups : FofGroups {
    double link = 0.0, vlink = 0.0;
    // per row the catalogue row of `parent` -- fof_groups(link) of the same step -- that holds it, or NB_FOF_NONE
    std::vector<uint32_t> parent_rows(const FofGroups &parent) const {
        if (parent.stats.step_num != stats.step_num)
            throw Error(NB_ERR_INVALID, "parent_rows: the parent was made at another step");
        std::vector<uint32_t> o(groups.size());
        for (size_t r = 0; r < o.size(); ++r) o[r] = parent.group_of[groups[r].label];
        return o;
    }
};

namespace detail {
template <class H>
PhaseSpaceGroups phase_space_groups(int (*call)(H *, const nb_fof6_params *, uint32_t *, uint32_t *, nb_fof_group *,
                                                size_t, nb_fof_stats *),
                                    H *h, size_t n, double link, double vlink, uint32_t min_members, bool labels) {
    PhaseSpaceGroups g;
    g.link = link;
    g.vlink = vlink;
    nb_fof6_params p{};
    p.link = link;
    p.vlink = vlink;
    p.min_members = min_members;
    const size_t cap = min_members ? n / min_members : 0;  // the most there can be (the call refuses 0 itself)
    if (labels) g.labels.resize(n);
    g.group_of.resize(n);
    g.groups.resize(cap);
    check(call(h, &p, labels ? g.labels.data() : nullptr, g.group_of.data(), g.groups.data(), cap, &g.stats));
    g.groups.resize((size_t)g.stats.groups);
    return g;
}
}  // namespace detail

// The bound groups of a state (nb_sim_bound; no reference counterpart): per body the catalogue row of its
// friends-of-friends group, the row whose bound set it belongs to (NB_FOF_NONE: none) and its energy in the last
// round it was active in; the catalogue in ascending label order.  bound_of and energy are empty when not asked for
struct BoundGroups {
    std::vector<uint32_t> group_of, bound_of;
    std::vector<double> energy;
    std::vector<BoundGroup> groups;
    BoundStats stats{};
    // the rows by bound mass, descending, ties by label
    std::vector<uint32_t> by_bound_mass() const {
        std::vector<uint32_t> o(groups.size());
        for (size_t i = 0; i < o.size(); ++i) o[i] = (uint32_t)i;
        std::sort(o.begin(), o.end(), [this](uint32_t a, uint32_t b) {
            return groups[a].mass != groups[b].mass ? groups[a].mass > groups[b].mass : groups[a].label < groups[b].label;
        });
        return o;
    }
};

namespace detail {
template <class H>
BoundGroups bound_groups(int (*call)(H *, const nb_bound_params *, uint32_t *, uint32_t *, double *, nb_bound_group *,
                                     size_t, nb_bound_stats *),
                         H *h, size_t n, double link, uint32_t min_members, uint32_t min_bound, uint32_t max_iter,
                         uint32_t max_group, bool per_body) {
    BoundGroups g;
    nb_bound_params p{};
    p.link = link;
    p.min_members = min_members;
    p.min_bound = min_bound;
    p.max_iter = max_iter;
    p.max_group = max_group;
    const size_t cap = min_members ? n / min_members : 0;  // the most there can be (the call refuses 0 itself)
    g.group_of.resize(n);
    if (per_body) {
        g.bound_of.resize(n);
        g.energy.resize(n);
    }
    g.groups.resize(cap);
    check(call(h, &p, g.group_of.data(), per_body ? g.bound_of.data() : nullptr, per_body ? g.energy.data() : nullptr,
               g.groups.data(), cap, &g.stats));
    g.groups.resize((size_t)g.stats.groups);
    return g;
}
}  // namespace detail

// The shapes of the rows of an assignment of bodies to rows (nb_sim_group_shapes; no reference counterpart): one
// row per row of the assignment; selected_of is empty when not asked for
struct ShapeOptions {
    bool reduced = false;       // weight the tensor by 1 / rho^2 (needs finite radii)
    uint32_t max_iter = 32, min_members = 10;
    double tol = 1e-3;
    bool per_body = false;      // selected_of
    uint64_t step_num = NB_SHAPE_ANY_STEP;  // the step the assignment was made at, or no check
};
struct GroupShapes {
    std::vector<ShapeGroup> rows;
    std::vector<uint32_t> selected_of;
    ShapeStats stats{};
    // (1 - q^2) / (1 - s^2) of row r: 0 oblate, 1 prolate
    double triaxiality(size_t r) const { return (1.0 - rows[r].q * rows[r].q) / (1.0 - rows[r].s * rows[r].s); }
    double j_norm(size_t r) const {
        const double *j = rows[r].j;
        return std::sqrt(j[0] * j[0] + j[1] * j[1] + j[2] * j[2]);
    }
};

namespace detail {
// centers, velocities: empty (the members' own, formed on the device) or three per row; radius: empty (+inf) or one per row
template <class H>
GroupShapes group_shapes(int (*call)(H *, const nb_shape_params *, const uint32_t *, size_t, const double *, const double *,
                                     const double *, nb_shape_group *, uint32_t *, nb_shape_stats *),
                         H *h, size_t n, const std::vector<uint32_t> &group_of, size_t m, const ShapeOptions &o,
                         const std::vector<double> &centers, const std::vector<double> &velocities,
                         const std::vector<double> &radius) {
    if (group_of.size() != n) throw std::invalid_argument("group_shapes: one group_of value per body");
    if ((!centers.empty() && centers.size() != 3 * m) || (!velocities.empty() && velocities.size() != 3 * m) ||
        (!radius.empty() && radius.size() != m))
        throw std::invalid_argument("group_shapes: centers, velocities and radius are per row, or empty");
    GroupShapes g;
    nb_shape_params p{};
    p.flags = o.reduced ? NB_SHAPE_REDUCED : 0u;
    p.min_members = o.min_members;
    p.max_iter = o.max_iter;
    p.tol = o.tol;
    p.step_num = o.step_num;
    g.rows.resize(m);
    if (o.per_body) g.selected_of.resize(n);
    check(call(h, &p, group_of.data(), m, centers.empty() ? nullptr : centers.data(),
               velocities.empty() ? nullptr : velocities.data(), radius.empty() ? nullptr : radius.data(), g.rows.data(),
               o.per_body ? g.selected_of.data() : nullptr, &g.stats));
    return g;
}
// ... of a friends-of-friends catalogue about its centres of mass and mean velocities, out to k_rms times every
// group's rms radius (k_rms <= 0: no cut)
template <class H, class Call>
GroupShapes fof_shapes(Call call, H *h, size_t n, const FofGroups &f, double k_rms, ShapeOptions o) {
    const size_t m = f.groups.size();
    std::vector<double> c(3 * m), v(3 * m), radius;
    if (k_rms > 0.0) radius.resize(m);
    for (size_t r = 0; r < m; ++r) {
        const FofGroup &g = f.groups[r];
        double c2 = 0.0;
        for (int a = 0; a < 3; ++a) {
            c[3 * r + a] = g.mx[a] / g.mass;
            v[3 * r + a] = g.mv[a] / g.mass;
            c2 += c[3 * r + a] * c[3 * r + a];
        }
        if (k_rms > 0.0) radius[r] = k_rms * std::sqrt(std::max(g.mr2 / g.mass - c2, 0.0));
    }
    o.step_num = f.stats.step_num;
    return group_shapes(call, h, n, f.group_of, m, o, c, v, radius);
}
}  // namespace detail

// The exact mass radii of the rows of an assignment of bodies to rows (nb_group_radii_sim; no reference counterpart):
// one row per row of the assignment; rank_of and enclosed_of are empty when not asked for
struct RadiiOptions {
    std::vector<double> fractions{0.1, 0.5, 0.9};  // 1 to 16 ascending values in (0, 1]
    uint32_t vmax_skip = 10;                       // the innermost ranks left out of the peak of M / r
    bool per_body = false;                         // rank_of, enclosed_of
    uint64_t step_num = NB_RADII_ANY_STEP;         // the step the assignment was made at, or no check
};
struct GroupRadii {
    std::vector<RadiiGroup> rows;
    std::vector<uint32_t> catalogue_rows;  // the catalogue row of every row (group_radii leaves out the rows without
                                           // a finite centre; radii_of, lagrangian_radii: 0 .. m - 1)
    std::vector<double> fractions;
    std::vector<uint32_t> rank_of;
    std::vector<double> enclosed_of;
    RadiiStats stats{};
    double radius(size_t r, size_t f) const { return rows[r].radius[f]; }
    double vmax(size_t r, double G) const { return std::sqrt(G * rows[r].vc2_max); }
};

namespace detail {
// centers: empty (the members' own centre of mass, formed on the device) or three per row
template <class H>
GroupRadii group_radii(int (*call)(H *, const nb_radii_params *, const uint32_t *, size_t, const double *,
                                   nb_radii_group *, uint32_t *, double *, nb_radii_stats *),
                       H *h, size_t n, const std::vector<uint32_t> &group_of, size_t m, const RadiiOptions &o,
                       const std::vector<double> &centers) {
    if (group_of.size() != n) throw std::invalid_argument("group_radii: one group_of value per body");
    if (!centers.empty() && centers.size() != 3 * m)
        throw std::invalid_argument("group_radii: centers are per row, or empty");
    GroupRadii g;
    nb_radii_params p{};
    p.nf = (uint32_t)o.fractions.size();  // (the call refuses a number it does not take)
    for (size_t f = 0; f < o.fractions.size() && f < NB_RADII_MAX_FRACTIONS; ++f) p.fractions[f] = o.fractions[f];
    p.vmax_skip = o.vmax_skip;
    p.step_num = o.step_num;
    g.fractions = o.fractions;
    g.rows.resize(m);
    if (o.per_body) {
        g.rank_of.resize(n);
        g.enclosed_of.resize(n);
    }
    check(call(h, &p, group_of.data(), m, centers.empty() ? nullptr : centers.data(), g.rows.data(),
               o.per_body ? g.rank_of.data() : nullptr, o.per_body ? g.enclosed_of.data() : nullptr, &g.stats));
    g.catalogue_rows.resize(m);
    for (size_t r = 0; r < m; ++r) g.catalogue_rows[r] = (uint32_t)r;
    return g;
}
// ... of a friends-of-friends catalogue about its centres of mass.  As the Python group_radii: a catalogue row without
// a finite centre (no mass) is left out, the others are renumbered in order and named by catalogue_rows
template <class H, class Call>
GroupRadii fof_radii(Call call, H *h, size_t n, const FofGroups &f, RadiiOptions o) {
    const size_t total = f.groups.size();
    std::vector<double> c;
    std::vector<uint32_t> kept, renumber(total, NB_FOF_NONE);
    for (size_t r = 0; r < total; ++r) {
        const FofGroup &g = f.groups[r];
        const double x[3] = {g.mx[0] / g.mass, g.mx[1] / g.mass, g.mx[2] / g.mass};
        if (!std::isfinite(x[0]) || !std::isfinite(x[1]) || !std::isfinite(x[2])) continue;
        renumber[r] = (uint32_t)kept.size();
        kept.push_back((uint32_t)r);
        c.insert(c.end(), x, x + 3);
    }
    std::vector<uint32_t> mapped(f.group_of.size());
    for (size_t i = 0; i < mapped.size(); ++i)
        mapped[i] = f.group_of[i] < total ? renumber[f.group_of[i]] : NB_FOF_NONE;
    o.step_num = f.stats.step_num;
    GroupRadii g = group_radii(call, h, n, mapped, kept.size(), o, c);
    g.catalogue_rows = kept;
    return g;
}
}  // namespace detail

// The density-peak groups of a state (nb_sim_hop; no reference counterpart): per body the label (the body at its
// density peak) and the catalogue row (NB_HOP_NONE: none), the catalogue in ascending label order with one peak
// density per row, and the boundaries between labels in ascending (a, b).  A vector that was not asked for is empty
struct HopParams {
    uint32_t k_density = 64, k_hop = 16, k_merge = 4, min_members = 1;
    double density_min = -std::numeric_limits<double>::infinity();
};
struct HopGroups {
    std::vector<uint32_t> labels, group_of;
    std::vector<double> density;
    std::vector<FofGroup> groups;
    std::vector<double> peak_density;
    std::vector<HopBoundary> boundaries;
    HopStats stats{};
    // the rows by count, descending, ties by label
    std::vector<uint32_t> by_size() const {
        std::vector<uint32_t> o(groups.size());
        for (size_t i = 0; i < o.size(); ++i) o[i] = (uint32_t)i;
        std::sort(o.begin(), o.end(), [this](uint32_t a, uint32_t b) {
            return groups[a].count != groups[b].count ? groups[a].count > groups[b].count : groups[a].label < groups[b].label;
        });
        return o;
    }
    // nb_hop_regroup: the merged catalogue, labels and group_of mapped through the merge, no boundaries
    HopGroups regroup(double saddle, double peak) const {
        HopGroups m;
        nb_hop_regroup_params rp{};
        rp.saddle = saddle;
        rp.peak = peak;
        std::vector<uint32_t> merged(groups.size());
        m.groups.resize(groups.size());
        m.peak_density.resize(groups.size());
        size_t count = 0;
        check(nb_hop_regroup(groups.data(), peak_density.data(), groups.size(), boundaries.data(), boundaries.size(), &rp,
                             merged.data(), m.groups.data(), m.peak_density.data(), groups.size(), &count));
        m.groups.resize(count);
        m.peak_density.resize(count);
        m.density = density;
        m.stats = stats;
        m.stats.groups = count;
        m.stats.grouped_bodies = m.stats.boundaries = m.stats.boundary_pairs = 0;
        m.stats.largest_count = 0;
        m.stats.largest_label = NB_HOP_NONE;
        for (const FofGroup &g : m.groups) {
            m.stats.grouped_bodies += g.count;
            if (g.count > m.stats.largest_count) {
                m.stats.largest_count = g.count;
                m.stats.largest_label = g.label;
            }
        }
        m.group_of.assign(group_of.size(), NB_HOP_NONE);
        if (!labels.empty()) m.labels.assign(labels.size(), NB_HOP_NONE);
        for (size_t i = 0; i < group_of.size(); ++i) {
            if (group_of[i] == NB_HOP_NONE || merged[group_of[i]] == NB_HOP_NONE) continue;
            const uint32_t label = merged[group_of[i]];
            const auto at = std::lower_bound(m.groups.begin(), m.groups.end(), label,
                                             [](const FofGroup &g, uint32_t l) { return g.label < l; });
            m.group_of[i] = (uint32_t)(at - m.groups.begin());
            if (!labels.empty()) m.labels[i] = label;
        }
        return m;
    }
};

namespace detail {
template <class H>
HopGroups hop_groups(int (*call)(H *, const nb_hop_params *, uint32_t *, uint32_t *, double *, nb_fof_group *, double *,
                                 size_t, nb_hop_boundary *, size_t, nb_hop_stats *),
                     H *h, size_t n, const HopParams &hp, bool labels, bool density, bool boundaries) {
    HopGroups g;
    nb_hop_params p{};
    p.k_density = hp.k_density;
    p.k_hop = hp.k_hop;
    p.k_merge = hp.k_merge;
    p.min_members = hp.min_members;
    p.density_min = hp.density_min;
    if (labels) g.labels.resize(n);
    g.group_of.resize(n);
    if (density) g.density.resize(n);
    size_t cap = n / 4 + 1, bcap = boundaries ? 4 * cap : 0;
    for (int attempt = 0; attempt < 2; ++attempt) {  // once more with the sizes the stats report, if they are larger
        g.groups.assign(cap, FofGroup{});
        g.peak_density.assign(cap, 0.0);
        g.boundaries.assign(bcap, HopBoundary{});
        check(call(h, &p, labels ? g.labels.data() : nullptr, g.group_of.data(), density ? g.density.data() : nullptr,
                   g.groups.data(), g.peak_density.data(), cap, boundaries ? g.boundaries.data() : nullptr, bcap,
                   &g.stats));
        if (g.stats.groups <= cap && (!boundaries || g.stats.boundaries <= bcap)) break;
        cap = std::max<size_t>(cap, (size_t)g.stats.groups);
        if (boundaries) bcap = std::max<size_t>(bcap, (size_t)g.stats.boundaries);
    }
    g.groups.resize((size_t)g.stats.groups);
    g.peak_density.resize((size_t)g.stats.groups);
    g.boundaries.resize(boundaries ? (size_t)g.stats.boundaries : 0);
    return g;
}
}  // namespace detail

// The k-th nearest neighbour of every body of a state, the mass inside it and the density from them (no
// reference counterpart); a vector that was not asked for is empty
struct KnnDensity {
    uint32_t k = 0;
    std::vector<double> r2, mass_in, density;
    std::vector<uint32_t> kth;  // NB_KNN_NONE: none
    KnnStats stats{};
    // the density centre sum rho x / sum rho and its velocity (NaN when sum rho is 0)
    std::array<double, 3> center() const { return per_rho(stats.sum_rho_x); }
    std::array<double, 3> center_velocity() const { return per_rho(stats.sum_rho_v); }

   private:
    std::array<double, 3> per_rho(const double (&s)[3]) const {
        const double nan = std::numeric_limits<double>::quiet_NaN(), w = stats.sum_rho;
        if (w == 0.0) return {nan, nan, nan};
        return {s[0] / w, s[1] / w, s[2] / w};
    }
};

namespace detail {
template <class H>
KnnDensity knn_density(int (*call)(H *, const nb_knn_params *, double *, uint32_t *, double *, double *, nb_knn_stats *),
                       H *h, size_t n, uint32_t k, bool density, bool neighbours) {
    KnnDensity d;
    nb_knn_params p{};
    p.k = d.k = k;
    if (neighbours) {
        d.r2.resize(n);
        d.kth.resize(n);
    }
    if (density) {
        d.mass_in.resize(n);
        d.density.resize(n);
    }
    check(call(h, &p, neighbours ? d.r2.data() : nullptr, neighbours ? d.kth.data() : nullptr,
               density ? d.mass_in.data() : nullptr, density ? d.density.data() : nullptr, &d.stats));
    return d;
}
}  // namespace detail

// nb_mst_sim's tree (no reference counterpart): the Euclidean minimum spanning tree of the counted bodies in
// ascending (d2, lo, hi); degree is empty when not asked for
struct SpanningTree {
    std::vector<uint32_t> edge_lo, edge_hi;
    std::vector<double> d2;
    std::vector<uint32_t> degree;  // NB_MST_NONE: a body that is not counted
    MstStats stats{};

    size_t counted() const { return (size_t)(stats.n - stats.nonfinite); }
    std::vector<double> length() const {
        std::vector<double> l(d2.size());
        for (size_t e = 0; e < d2.size(); ++e) l[e] = std::sqrt(d2[e]);
        return l;
    }
    double total_length() const {
        double t = 0.0;
        for (double d : d2) t += std::sqrt(d);
        return t;
    }
    // the length of the last edge (0 for a tree without edges)
    double longest() const { return d2.empty() ? 0.0 : std::sqrt(d2.back()); }
    // per body the smallest index of its component under the edges with d2 <= link^2 (nb_mst_cut): the labels of
    // fof_groups(link, 1) of the same state
    std::vector<uint32_t> cut(double link) const {
        std::vector<uint32_t> labels((size_t)stats.n);
        check(nb_mst_cut((size_t)stats.n, d2.size(), edge_lo.data(), edge_hi.data(), d2.data(),
                         degree.empty() ? nullptr : degree.data(), link, labels.data(), nullptr));
        return labels;
    }
    // the dendrogram (nb_mst_linkage): per edge the two components it joins, smallest indices and sizes
    struct Linkage {
        std::vector<uint32_t> label_a, label_b, count_a, count_b;
    };
    Linkage linkage() const {
        const size_t m = d2.size();
        Linkage l{std::vector<uint32_t>(m), std::vector<uint32_t>(m), std::vector<uint32_t>(m),
                  std::vector<uint32_t>(m)};
        check(nb_mst_linkage((size_t)stats.n, m, edge_lo.data(), edge_hi.data(), l.label_a.data(), l.label_b.data(),
                             l.count_a.data(), l.count_b.data()));
        return l;
    }
    // the percolation curve: per link the components of at least min_members bodies, from one pass over the linkage
    std::vector<uint64_t> group_counts(const std::vector<double> &links, uint32_t min_members = 1) const {
        const Linkage l = linkage();
        const size_t m = d2.size();
        std::vector<int64_t> after(m + 1);
        after[0] = min_members <= 1 ? (int64_t)counted() : 0;
        for (size_t e = 0; e < m; ++e) {
            const uint64_t a = l.count_a[e], b = l.count_b[e];
            after[e + 1] = after[e] + (a + b >= min_members) - (a >= min_members) - (b >= min_members);
        }
        std::vector<uint64_t> out;
        for (double link : links) {
            const double b2 = link * link;
            out.push_back((uint64_t)after[(size_t)(std::upper_bound(d2.begin(), d2.end(), b2) - d2.begin())]);
        }
        return out;
    }
};

namespace detail {
template <class H>
SpanningTree spanning_tree(int (*call)(H *, const nb_mst_params *, uint32_t *, uint32_t *, double *, uint32_t *,
                                       nb_mst_stats *),
                           H *h, size_t n, bool degree) {
    SpanningTree t;
    nb_mst_params p{};
    const size_t room = n ? n - 1 : 0;
    t.edge_lo.resize(room);
    t.edge_hi.resize(room);
    t.d2.resize(room);
    if (degree) t.degree.resize(n);
    check(call(h, &p, t.edge_lo.data(), t.edge_hi.data(), t.d2.data(), degree ? t.degree.data() : nullptr, &t.stats));
    t.edge_lo.resize((size_t)t.stats.edges);
    t.edge_hi.resize((size_t)t.stats.edges);
    t.d2.resize((size_t)t.stats.edges);
    return t;
}
}  // namespace detail

// nb_local_kinematics_sim's per-body sums over the k nearest neighbours (no reference counterpart) and the rows
// nb_local_kinematics_derive makes of them: moments 10 and grads 15 doubles per body, grads and kth empty when not
// asked for; derived[i].mean_velocity is NaN until derive() is given the state's velocities
struct LocalKinematics {
    uint32_t k = 0;
    std::vector<double> moments, grads, r2, mass_in, density;
    std::vector<uint32_t> kth;
    std::vector<KinDerived> derived;
    KinStats stats{};
    // nb_local_kinematics_derive again, with the velocities (3 floats per body) of the state the sums were made from
    void derive(const std::vector<float> *velocities = nullptr) {
        derived.resize(r2.size());
        check(nb_local_kinematics_derive(moments.data(), grads.empty() ? nullptr : grads.data(), r2.data(),
                                         density.data(), velocities ? velocities->data() : nullptr, r2.size(),
                                         derived.data()));
    }
};

namespace detail {
template <class H>
LocalKinematics local_kinematics(int (*call)(H *, const nb_kin_params *, double *, double *, double *, uint32_t *,
                                             double *, double *, nb_kin_stats *),
                                 H *h, size_t n, uint32_t k, bool gradient, bool include_self, bool neighbours) {
    LocalKinematics d;
    nb_kin_params p{};
    p.k = d.k = k;
    p.flags = include_self ? NB_KIN_SELF : 0u;
    d.moments.resize(n * NB_KIN_MOMENTS);
    if (gradient) d.grads.resize(n * NB_KIN_GRADS);
    d.r2.resize(n);
    d.mass_in.resize(n);
    d.density.resize(n);
    if (neighbours) d.kth.resize(n);
    check(call(h, &p, d.moments.data(), gradient ? d.grads.data() : nullptr, d.r2.data(),
               neighbours ? d.kth.data() : nullptr, d.mass_in.data(), d.density.data(), &d.stats));
    d.derive();
    return d;
}
}  // namespace detail

// The spherical radial profiles of a state about many centres (nb_sim_halo_profiles; no reference counterpart):
// heads[c] and bins[c * nbins + k] for centre c and bin k, the edges shared by all centres
struct HaloProfiles {
    std::vector<double> edges;  // nbins + 1
    std::vector<HaloHead> heads;
    std::vector<RadialBin> bins;
    HaloStats stats{};
    uint32_t nbins() const { return (uint32_t)edges.size() - 1; }
    size_t centers() const { return heads.size(); }
    const RadialBin *row(size_t c) const { return bins.data() + c * nbins(); }
    // nb_halo_enclosed: the mass inside every edge
    std::vector<double> enclosed(size_t c) const {
        std::vector<double> out(edges.size());
        check(nb_halo_enclosed(&heads[c], row(c), nbins(), out.data()));
        return out;
    }
    // nb_halo_overdensity: {r, mass} where the mean enclosed density first falls through rho (NaN: nowhere)
    std::array<double, 2> overdensity(size_t c, double rho) const {
        std::array<double, 2> o{};
        check(nb_halo_overdensity(&heads[c], row(c), edges.data(), nbins(), rho, &o[0], &o[1]));
        return o;
    }
};

namespace detail {
template <class H>
HaloProfiles halo_profiles(int (*call)(H *, const nb_halo_params *, nb_halo_head *, nb_radial_bin *, nb_halo_stats *),
                           H *h, const std::vector<double> &edges, const std::vector<double> *centers,
                           const std::vector<uint32_t> *bodies, const std::vector<double> &velocities) {
    HaloProfiles o;
    o.edges = edges;
    nb_halo_params p{};
    p.nbins = edges.empty() ? 0u : (uint32_t)(edges.size() - 1);
    p.edges = edges.data();
    p.m = centers ? centers->size() / 3 : bodies->size();
    if (centers) p.centers = centers->data();
    if (bodies) p.bodies = bodies->data();
    if (!velocities.empty()) {
        if (velocities.size() != 3 * p.m) throw Error(NB_ERR_INVALID, "halo_profiles: one velocity per centre");
        p.velocities = velocities.data();
    }
    o.heads.resize(p.m);
    o.bins.resize(p.m * p.nbins);
    check(call(h, &p, o.heads.data(), o.bins.data(), &o.stats));
    return o;
}
}  // namespace detail

// A smoothed map (no reference counterpart): width * height counts (the bodies that reach a pixel), row 0 the
// smallest b, the planes (1, or 6 with NB_SMOOTH_VELOCITY: wm, wm_ua, wm_ub, wm_w, wm_w2, wm_u2; plane 0 is the
// surface density) plane-major, the smoothing lengths that were passed and what the call measured
struct SmoothedMap {
    uint32_t width = 0, height = 0, nplanes = 0;
    std::vector<uint32_t> counts;
    std::vector<double> planes;
    std::vector<double> smoothing;
    SmoothStats stats{};
    const double *plane(uint32_t k) const { return planes.data() + (size_t)k * width * height; }
};

// The parameters of a smoothed map of the window [x0, x1) x [y0, y1) about the centre of mass, seen along
// `axis`, with the velocity planes, no depth cut, and the smoothing lengths held between 2 and 64 times the
// larger side of a pixel
inline SmoothParams smooth_params(uint32_t width, uint32_t height, double x0, double x1, double y0, double y1,
                                  const std::array<double, 3> &axis = {0.0, 1.0, 0.0}) {
    SmoothParams p{};
    p.width = width;
    p.height = height;
    p.flags = NB_SMOOTH_CENTER_COM | NB_SMOOTH_VELOCITY;
    for (int k = 0; k < 3; ++k) p.axis[k] = axis[(size_t)k];
    p.x_range[0] = x0;
    p.x_range[1] = x1;
    p.y_range[0] = y0;
    p.y_range[1] = y1;
    p.depth_range[0] = -HUGE_VAL;
    p.depth_range[1] = HUGE_VAL;
    const double pixel = std::max(width ? std::fabs(x1 - x0) / width : 0.0, height ? std::fabs(y1 - y0) / height : 0.0);
    p.s_min = 2.0 * pixel;
    p.s_max = 64.0 * pixel;
    return p;
}

namespace detail {
template <class H>
SmoothedMap smoothed_map(int (*call)(H *, const nb_smooth_params *, const double *, uint32_t *, double *,
                                     nb_smooth_stats *),
                         H *h, size_t n, const SmoothParams &p, std::vector<double> s) {
    if (s.size() != n) throw Error(NB_ERR_INVALID, "nbody_hip: smoothed_map: one smoothing length per body");
    SmoothedMap m;
    const bool ok = p.width >= 1 && p.width <= NB_MAP_MAX_SIDE && p.height >= 1 && p.height <= NB_MAP_MAX_SIDE &&
                    (uint64_t)p.width * p.height <= NB_MAP_MAX_CELLS;  // (the call refuses the sizes itself)
    m.width = ok ? p.width : 1;
    m.height = ok ? p.height : 1;
    m.nplanes = (p.flags & NB_SMOOTH_VELOCITY) ? 6 : 1;
    m.counts.resize((size_t)m.width * m.height);
    m.planes.resize((size_t)m.nplanes * m.width * m.height);
    m.smoothing = std::move(s);
    check(call(h, &p, m.smoothing.empty() ? nullptr : m.smoothing.data(), m.counts.data(), m.planes.data(), &m.stats));
    return m;
}
// scale times the distance to the k-th neighbour of every body: the lengths of a smoothed map, composed on the host
inline std::vector<double> knn_lengths(const KnnDensity &d, double scale) {
    std::vector<double> s(d.r2.size());
    for (size_t i = 0; i < s.size(); ++i) s[i] = scale * std::sqrt(d.r2[i]);
    return s;
}
}  // namespace detail

// A frame drawn off screen: width * height RGBA8 pixels, rows top to bottom, and its statistics
struct Frame {
    uint32_t width = 0, height = 0;
    std::vector<uint8_t> rgba;
    std::vector<uint32_t> counts;  // filled on request
    RenderStats stats{};
};

// init_fn: fn(&SimParams) -> Vec<Particle>, sims/mod.rs:79
using InitFn = std::function<std::vector<Particle>(const SimParams &)>;

namespace inits {  // src/inits.rs, seeded
inline InitFn seeded(void (*fn)(const nb_sim_params *, nb_particle *, void *), uint64_t seed) {
    return [fn, seed](const SimParams &p) {
        std::vector<Particle> out(p.particle_num);
        uint64_t s = seed;
        fn(&p, out.data(), &s);
        return out;
    };
}
inline InitFn uniform_init(uint64_t seed = 0) { return seeded(nb_init_uniform, seed); }
inline InitFn disc_init(uint64_t seed = 0) { return seeded(nb_init_disc, seed); }
inline InitFn spherical_init(uint64_t seed = 0) { return seeded(nb_init_spherical, seed); }
}  // namespace inits

namespace detail {
struct InitThunk {
    const InitFn *fn;
    std::string error;
    static void call(const nb_sim_params *p, nb_particle *out, void *user) {
        auto *self = static_cast<InitThunk *>(user);
        try {  // never unwind through the C ABI
            std::vector<Particle> v = (*self->fn)(*p);
            if (v.size() != p->particle_num) {
                self->error = "init_fn returned the wrong number of particles";
                return;
            }
            for (size_t i = 0; i < v.size(); ++i) out[i] = v[i];
        } catch (const std::exception &e) {
            self->error = e.what();
        } catch (...) {
            self->error = "init_fn threw";
        }
    }
};

// the entry points of the analysis passes per handle type: nb_sim_X, and nb_runner_X -- the same pass on the
// runner's simulator, refused by a several-GPU runner
template <class H>
struct PassAbi;
template <>
struct PassAbi<nb_sim> {
    static constexpr auto sim_params = nb_sim_sim_params;
    static constexpr auto diagnostics = nb_sim_diagnostics;
    static constexpr auto radial_profile = nb_sim_radial_profile;
    static constexpr auto field = nb_sim_field;
    static constexpr auto map = nb_sim_map;
    static constexpr auto fof = nb_sim_fof;
    static constexpr auto bound = nb_sim_bound;
    static constexpr auto knn = nb_sim_knn;
    static constexpr auto mst = nb_mst_sim;
    static constexpr auto hop = nb_sim_hop;
    static constexpr auto halo_profiles = nb_sim_halo_profiles;
    static constexpr auto group_shapes = nb_sim_group_shapes;
    static constexpr auto group_radii = nb_group_radii_sim;
    static constexpr auto disc_modes = nb_disc_modes_sim;
    static constexpr auto shell_modes = nb_shell_modes_sim;
    static constexpr auto phase_map = nb_phase_map_sim;
    static constexpr auto tidal = nb_tidal_sim;
    static constexpr auto orbits = nb_orbits_sim;
    static constexpr auto orbit_sections = nb_orbit_sections_sim;
    static constexpr auto orbit_stability = nb_orbit_stability_sim;
    static constexpr auto local_kinematics = nb_local_kinematics_sim;
    static constexpr auto fof6 = nb_fof6_sim;
    static constexpr auto smooth_map = nb_sim_smooth_map;
    static constexpr auto render = nb_sim_render;
};
template <>
struct PassAbi<nb_runner> {
    static constexpr auto sim_params = nb_runner_sim_params;
    static constexpr auto diagnostics = nb_runner_diagnostics;
    static constexpr auto radial_profile = nb_runner_radial_profile;
    static constexpr auto field = nb_runner_field;
    static constexpr auto map = nb_runner_map;
    static constexpr auto fof = nb_runner_fof;
    static constexpr auto bound = nb_runner_bound;
    static constexpr auto knn = nb_runner_knn;
    static constexpr auto mst = nb_mst_runner;
    static constexpr auto hop = nb_runner_hop;
    static constexpr auto halo_profiles = nb_runner_halo_profiles;
    static constexpr auto group_shapes = nb_runner_group_shapes;
    static constexpr auto group_radii = nb_group_radii_runner;
    static constexpr auto disc_modes = nb_disc_modes_runner;
    static constexpr auto shell_modes = nb_shell_modes_runner;
    static constexpr auto phase_map = nb_phase_map_runner;
    static constexpr auto tidal = nb_tidal_runner;
    static constexpr auto orbits = nb_orbits_runner;
    static constexpr auto orbit_sections = nb_orbit_sections_runner;
    static constexpr auto orbit_stability = nb_orbit_stability_runner;
    static constexpr auto local_kinematics = nb_local_kinematics_runner;
    static constexpr auto fof6 = nb_fof6_runner;
    static constexpr auto smooth_map = nb_runner_smooth_map;
    static constexpr auto render = nb_runner_render;
};
}  // namespace detail

// The analysis passes of the current state (no reference counterpart), once for Simulator and OfflineHeadless<T>;
// on a runner each is the pass of the runner's simulator, for one device only
template <class H>
class Passes {
    using Abi = detail::PassAbi<H>;

   public:
    // energy, momentum, angular momentum of the current state; potential: the O(N^2) pair potential too
    Diagnostics diagnostics(bool potential = false) {
        Diagnostics d{};
        check(Abi::diagnostics(h_, NB_DIAG_MOMENTS | (potential ? NB_DIAG_POTENTIAL : 0u), &d));
        return d;
    }
    // per-shell mass and velocity moments of the current state between `edges`; p: flags
    // (NB_RADIAL_CYLINDRICAL, NB_RADIAL_CENTER_COM), centre, velocity and axis (nbins and edges are set here)
    RadialProfile radial_profile(const std::vector<double> &edges, const RadialParams &p = RadialParams{0, NB_RADIAL_CENTER_COM}) {
        return detail::radial_profile(Abi::radial_profile, h_, edges, p);
    }
    // the azimuthal Fourier sums per annulus between `edges` about p.axis; p: mmax, flags (NB_MODES_CENTER_COM),
    // centre, velocity and axis (nbins and edges are set here)
    DiscModes disc_modes(const std::vector<double> &edges, const ModesParams &p) {
        SimParams sp{};
        check(Abi::sim_params(h_, &sp));
        return detail::disc_modes(Abi::disc_modes, h_, (double)sp.dt, edges, p);
    }
    // the spherical-harmonic sums per radial shell between `edges`, the polar axis p.axis; p: lmax, flags
    // (NB_SHELL_CENTER_COM, NB_SHELL_RATES), centre, velocity and axis (nbins and edges are set here)
    ShellModes shell_modes(const std::vector<double> &edges, const ShellParams &p) {
        SimParams sp{};
        check(Abi::sim_params(h_, &sp));
        return detail::shell_modes(Abi::shell_modes, h_, (double)sp.dt, edges, p);
    }
    // the exact acceleration and potential of the current state at points (3 floats each); flags: NB_FIELD_*
    ProjectedMap projected_map(const MapParams &p) { return detail::projected_map(Abi::map, h_, p); }
    // the bodies of the current state binned on p.x and p.y between the edges, p.q summed with NB_PHASE_WEIGHT;
    // p: phase_params(); p.values (the quantity "value") must hold one double per body of read_particles() now
    PhaseMap phase_map(const PhaseParams &p, const std::vector<double> &x_edges, const std::vector<double> &y_edges) {
        return detail::phase_map(Abi::phase_map, h_, p, x_edges, y_edges);
    }
    // the friends-of-friends groups of the current state: bodies within `link` are friends
    FofGroups fof_groups(double link, uint32_t min_members = 20, bool labels = true) {
        return detail::fof_groups(Abi::fof, h_, n_bodies(), link, min_members, labels);
    }
    PhaseSpaceGroups phase_space_groups(double link, double vlink, uint32_t min_members = 20, bool labels = true) {
        return detail::phase_space_groups(Abi::fof6, h_, n_bodies(), link, vlink, min_members, labels);
    }
    // those groups unbound: min_bound 0 stands for min_members, max_group 0 for no limit
    BoundGroups bound_groups(double link, uint32_t min_members = 20, uint32_t min_bound = 0, uint32_t max_iter = 32,
                             uint32_t max_group = 262144, bool per_body = true) {
        return detail::bound_groups(Abi::bound, h_, n_bodies(), link, min_members,
                                    min_bound ? min_bound : min_members, max_iter, max_group, per_body);
    }
    // the shapes of the rows of an assignment: group_of of read_particles() now, NB_FOF_NONE or a row < m
    GroupShapes group_shapes(const std::vector<uint32_t> &group_of, size_t m, const ShapeOptions &o = ShapeOptions{},
                             const std::vector<double> &centers = {}, const std::vector<double> &velocities = {},
                             const std::vector<double> &radius = {}) {
        return detail::group_shapes(Abi::group_shapes, h_, n_bodies(), group_of, m, o, centers,
                                    velocities, radius);
    }
    GroupShapes group_shapes(const FofGroups &f, double k_rms = 0.0, const ShapeOptions &o = ShapeOptions{}) {
        return detail::fof_shapes(Abi::group_shapes, h_, n_bodies(), f, k_rms, o);
    }
    // the exact mass radii, the extent and the peak of M / r of the rows of an assignment
    GroupRadii radii_of(const std::vector<uint32_t> &group_of, size_t m, const RadiiOptions &o = RadiiOptions{},
                        const std::vector<double> &centers = {}) {
        return detail::group_radii(Abi::group_radii, h_, n_bodies(), group_of, m, o, centers);
    }
    GroupRadii group_radii(const FofGroups &f, const RadiiOptions &o = RadiiOptions{}) {
        return detail::fof_radii(Abi::group_radii, h_, n_bodies(), f, o);
    }
    // ... of the whole state as one row: center empty (its own centre of mass, formed on the device) or x y z.  The
    // Python method's center="density" is this with knn_density(6, true, false).center() as the point
    GroupRadii lagrangian_radii(const RadiiOptions &o = RadiiOptions{{0.01, 0.05, 0.1, 0.25, 0.5, 0.75, 0.9}},
                                const std::vector<double> &center = {}) {
        return detail::group_radii(Abi::group_radii, h_, n_bodies(), std::vector<uint32_t>(n_bodies(), 0u), 1, o,
                                   center);
    }
    // the k-th neighbour, the mass inside it and the density at every body; center() is the density centre
    HopGroups hop_groups(const HopParams &p = HopParams{}, bool labels = true, bool density = false,
                         bool boundaries = true) {
        return detail::hop_groups(Abi::hop, h_, n_bodies(), p, labels, density, boundaries);
    }
    KnnDensity knn_density(uint32_t k = 6, bool density = true, bool neighbours = true) {
        return detail::knn_density(Abi::knn, h_, n_bodies(), k, density, neighbours);
    }
    // the minimum spanning tree of the current state: cut(link) is fof_groups(link, 1)'s labels for every link
    SpanningTree spanning_tree(bool degree = true) { return detail::spanning_tree(Abi::mst, h_, n_bodies(), degree); }
    // how the k nearest neighbours of every body move: the moments, with gradient the velocity-gradient sums, and
    // the derived rows (sigma, rho / sigma^3, divergence, vorticity, shear)
    LocalKinematics local_kinematics(uint32_t k = 32, bool gradient = false, bool include_self = true,
                                     bool neighbours = false) {
        return detail::local_kinematics(Abi::local_kinematics, h_, n_bodies(), k, gradient, include_self, neighbours);
    }
    // the profiles about points (centers: x y z per centre) or about bodies; velocities: empty, or three per centre
    HaloProfiles halo_profiles(const std::vector<double> &edges, const std::vector<double> &centers,
                               const std::vector<double> &velocities = {}) {
        return detail::halo_profiles(Abi::halo_profiles, h_, edges, &centers, nullptr, velocities);
    }
    HaloProfiles halo_profiles_of_bodies(const std::vector<double> &edges, const std::vector<uint32_t> &bodies,
                                         const std::vector<double> &velocities = {}) {
        return detail::halo_profiles(Abi::halo_profiles, h_, edges, nullptr, &bodies, velocities);
    }
    // the smoothed map of the current state: s[i] the smoothing length of body i in the order of read_particles() now
    SmoothedMap smoothed_map(const SmoothParams &p, std::vector<double> s) {
        return detail::smoothed_map(Abi::smooth_map, h_, n_bodies(), p, std::move(s));
    }
    // ... with scale times the distance to the k-th neighbour (knn_density(k) on the same state)
    SmoothedMap smoothed_map_knn(const SmoothParams &p, uint32_t k = 32, double scale = 1.0) {
        return smoothed_map(p, detail::knn_lengths(knn_density(k, false, true), scale));
    }
    Field field(const std::vector<float> &points, uint32_t flags = NB_FIELD_ACCEL | NB_FIELD_POTENTIAL) {
        return detail::field(Abi::field, h_, points, flags);
    }
    // the rotation curve from the force on n_phi points of each ring: v_c = sqrt(max(0, -R a_R))
    RingMeans circular_velocity(const std::vector<double> &radii, const std::array<double, 3> &axis = {0.0, 1.0, 0.0},
                                const std::array<double, 3> &center = {0.0, 0.0, 0.0}, uint32_t n_phi = 16,
                                bool potential = false) {
        return detail::circular_velocity(Abi::field, h_, radii, axis, center, n_phi, potential);
    }
    // the exact tidal tensor T_ab = d acc_a / d x_b of the current state at the points
    TidalField tidal_tensor(const std::vector<float> &points) { return detail::tidal_tensor(Abi::tidal, h_, points); }
    // Omega, kappa and nu of a disc on n_phi points of each ring: the force and its gradient on the same rings
    DiscFrequencies disc_frequencies(const std::vector<double> &radii,
                                     const std::array<double, 3> &axis = {0.0, 1.0, 0.0},
                                     const std::array<double, 3> &center = {0.0, 0.0, 0.0}, uint32_t n_phi = 16) {
        return detail::disc_frequencies(Abi::field, Abi::tidal, h_, radii, axis, center, n_phi);
    }
    // test particles from pos, vel (3 doubles per tracer) through the frozen field of the current state, the
    // pattern turning at p.omega (orbit_params)
    Orbits orbits(const nb_orbit_params &p, const std::vector<double> &pos, const std::vector<double> &vel) {
        return detail::orbits(Abi::orbits, h_, p, pos, vel);
    }
    // ... one tracer per radius from the first point of its ring, with speed times the circular velocity along the
    // direction of rotation there (p.axis and p.center are the rings')
    Orbits circular_orbits(const nb_orbit_params &p, const std::vector<double> &radii, uint32_t n_phi = 16,
                           double speed = 1.0) {
        std::vector<double> pos, vel;
        circular_launch(p, radii, n_phi, speed, pos, vel);
        return orbits(p, pos, vel);
    }
    // orbits() whose step kernel also takes the crossings of the plane `sec` of the pattern frame and a summary per
    // tracer (orbit_section_params); no launch is added
    OrbitSections orbit_sections(const nb_orbit_params &p, const nb_orbit_section_params &sec,
                                 const std::vector<double> &pos, const std::vector<double> &vel) {
        return detail::orbit_sections(Abi::orbit_sections, h_, p, sec, pos, vel);
    }
    // ... launched as circular_orbits() launches
    OrbitSections circular_orbit_sections(const nb_orbit_params &p, const nb_orbit_section_params &sec,
                                          const std::vector<double> &radii, uint32_t n_phi = 16, double speed = 1.0) {
        std::vector<double> pos, vel;
        circular_launch(p, radii, n_phi, speed, pos, vel);
        return orbit_sections(p, sec, pos, vel);
    }
    // orbits() that also carries dev0's vectors ([tracers][D], D the same for every tracer) along every orbit by the
    // tangent map of its step, renormalised by powers of two beyond 2^+-renorm_log2; p without NB_ORBIT_ENERGY
    OrbitStability orbit_stability(const nb_orbit_params &p, const std::vector<double> &pos,
                                   const std::vector<double> &vel, const std::vector<nb_orbit_deviation> &dev0,
                                   uint32_t renorm_log2 = 32) {
        return detail::orbit_stability(Abi::orbit_stability, h_, p, pos, vel, dev0, renorm_log2);
    }
    // the tracers of circular_orbits()
    void circular_launch(const nb_orbit_params &p, const std::vector<double> &radii, uint32_t n_phi, double speed,
                         std::vector<double> &pos, std::vector<double> &vel) {
        const std::array<double, 3> axis{p.axis[0], p.axis[1], p.axis[2]}, center{p.center[0], p.center[1], p.center[2]};
        const RingMeans cv = circular_velocity(radii, axis, center, n_phi);
        const std::vector<float> pts = field_rings(radii, axis, center, n_phi);
        double n[3], e1[3], e2[3];
        check(nb_map_frame(axis.data(), n, e1, e2));
        pos.assign(3 * radii.size(), 0.0);
        vel.assign(3 * radii.size(), 0.0);
        for (size_t i = 0; i < radii.size(); ++i)
            for (size_t a = 0; a < 3; ++a) {
                pos[3 * i + a] = (double)pts[3 * (i * n_phi) + a];
                vel[3 * i + a] = (speed * cv.rings[i].v_c) * e2[a];
            }
    }
    // the current state drawn on the device (OnlineRenderer::render, online_renderer.rs:331-367)
    Frame render(const RenderParams &p, bool counts = false) {
        Frame f;
        f.width = p.width;
        f.height = p.height;
        f.rgba.resize((size_t)p.width * p.height * 4);
        if (counts) f.counts.resize((size_t)p.width * p.height);
        check(Abi::render(h_, &p, f.rgba.data(), counts ? f.counts.data() : nullptr, &f.stats));
        return f;
    }

   protected:
    Passes() = default;
    ~Passes() = default;
    size_t n_bodies() const {
        SimParams p{};
        check(Abi::sim_params(h_, &p));
        return p.particle_num;
    }
    H *h_ = nullptr;
};

// trait Simulator, sims/mod.rs:73-90
class Simulator : public Passes<nb_sim> {
   public:
    Simulator(const Simulator &) = delete;
    Simulator &operator=(const Simulator &) = delete;
    Simulator(Simulator &&o) noexcept : owned_(o.owned_) {
        h_ = o.h_;
        o.h_ = nullptr;
    }
    virtual ~Simulator() {
        if (h_ && owned_) nb_sim_destroy(h_);
    }

    void encode() { check(nb_sim_encode(h_)); }    // Simulator::encode + queue.submit
    void cleanup() { check(nb_sim_cleanup(h_)); }  // Simulator::cleanup
    void wait() { check(nb_sim_wait(h_)); }        // device.poll(Maintain::Wait)
    SimParams sim_params() const {                 // Simulator::sim_params
        SimParams p{};
        check(nb_sim_sim_params(h_, &p));
        return p;
    }
    // Simulator::dest_particle_slice -- the POST-step state, copied to the host
    std::vector<Particle> dest_particle_slice() {
        std::vector<Particle> out(sim_params().particle_num);
        check(nb_sim_read_particles(h_, out.data(), out.size()));
        return out;
    }
    void write_particles(const std::vector<Particle> &p) {
        check(nb_sim_write_particles(h_, p.data(), p.size()));
    }
    uint64_t step_num() const {
        uint64_t v = 0;
        check(nb_sim_step_num(h_, &v));
        return v;
    }
    nb_sim *handle() { return h_; }

   protected:
    Simulator(nb_sim *h, bool owned) : owned_(owned) { h_ = h; }
    static nb_sim *create(const SimParams &sp, nb_add_params ap, const InitFn &init,
                          const nb_placement *pl) {
        detail::InitThunk thunk{&init, {}};
        nb_sim *h = nullptr;
        int rc = nb_sim_create(&h, &sp, &ap, pl, &detail::InitThunk::call, &thunk);
        if (!thunk.error.empty()) {
            if (rc == NB_OK) nb_sim_destroy(h);
            throw Error(NB_ERR_INVALID, thunk.error);
        }
        check(rc);
        return h;
    }
    bool owned_;
    template <class T>
    friend class OfflineHeadless;
};

class NaiveSim : public Simulator {  // sims/naive.rs
   public:
    static constexpr int kKind = NB_NAIVE_SIM_PARAMS;
    NaiveSim(const SimParams &sp, const AddParams &, const InitFn &init,
             const nb_placement *pl = nullptr)
        : Simulator(create(sp, nb_add_params{NB_NAIVE_SIM_PARAMS, 0.f}, init, pl), true) {}
    NaiveSim(nb_sim *borrowed) : Simulator(borrowed, false) {}
};

class TreeSim : public Simulator {  // sims/tree.rs
   public:
    static constexpr int kKind = NB_TREE_SIM_PARAMS;
    // any other AddParams falls back to theta 0.75 as TreeSim::new does (tree.rs:42-51)
    TreeSim(const SimParams &sp, const AddParams &ap, const InitFn &init,
            const nb_placement *pl = nullptr)
        : Simulator(create(sp,
                           nb_add_params{NB_TREE_SIM_PARAMS,
                                         ap.c.kind == NB_TREE_SIM_PARAMS ? ap.c.theta : 0.f},
                           init, pl),
                    true) {}
    TreeSim(nb_sim *borrowed) : Simulator(borrowed, false) {}
    std::pair<std::vector<Octant>, float> read_tree() {
        std::vector<Octant> t((size_t)4 * sim_params().particle_num + 8);
        size_t n = 0;
        float rw = 0.f;
        check(nb_sim_read_tree(h_, t.data(), t.size(), &n, &rw));
        t.resize(n);
        return {std::move(t), rw};
    }
};

// OfflineHeadless<T: Simulator>, runners/offline_headless.rs:4-45
template <class T>
class OfflineHeadless : public Passes<nb_runner> {
   public:
    OfflineHeadless(const SimParams &sp, const AddParams &ap, const InitFn &init, int device_id = -1) {
        detail::InitThunk thunk{&init, {}};
        nb_add_params c = ap.c;
        if (c.kind != T::kKind) c = nb_add_params{T::kKind, 0.f};
        int rc = nb_runner_create(&h_, &sp, &c, &detail::InitThunk::call, &thunk, device_id);
        if (!thunk.error.empty()) {
            if (rc == NB_OK) nb_runner_destroy(h_);
            throw Error(NB_ERR_INVALID, thunk.error);
        }
        check(rc);
    }
    // several GPUs of this process (nb_runner_create_multi): rank r owns a contiguous
    // body range on device_ids[r]
    // let_migrate_every >= 0 (TreeSim): Morton domains + LET exchange (nb_runner_create_multi_let)
    OfflineHeadless(const SimParams &sp, const AddParams &ap, const InitFn &init, const std::vector<int> &device_ids,
                    int let_migrate_every = -1) {
        detail::InitThunk thunk{&init, {}};
        nb_add_params c = ap.c;
        if (c.kind != T::kKind) c = nb_add_params{T::kKind, 0.f};
        int rc = let_migrate_every >= 0
                     ? nb_runner_create_multi_let(&h_, &sp, &c, &detail::InitThunk::call, &thunk, device_ids.data(),
                                                  (int)device_ids.size(), let_migrate_every)
                     : nb_runner_create_multi(&h_, &sp, &c, &detail::InitThunk::call, &thunk, device_ids.data(),
                                              (int)device_ids.size());
        if (!thunk.error.empty()) {
            if (rc == NB_OK) nb_runner_destroy(h_);
            throw Error(NB_ERR_INVALID, thunk.error);
        }
        check(rc);
    }
    OfflineHeadless(const OfflineHeadless &) = delete;
    ~OfflineHeadless() {
        if (h_) nb_runner_destroy(h_);
    }
    void step() { check(nb_runner_step(h_)); }  // encode -> submit -> cleanup -> poll(Wait)
    void step_n(int n) { check(nb_runner_step_n(h_, n)); }
    T sim() { return T(nb_runner_sim(h_)); }  // borrowed view of the runner's simulator (one device)
    uint64_t step_num() const {
        uint64_t v = 0;
        check(nb_runner_step_num(h_, &v));
        return v;
    }
    std::vector<Particle> read_particles() {
        SimParams p{};
        check(nb_runner_sim_params(h_, &p));
        std::vector<Particle> out(p.particle_num);
        check(nb_runner_read_particles(h_, out.data(), out.size()));
        return out;
    }

};

}  // namespace nbody
