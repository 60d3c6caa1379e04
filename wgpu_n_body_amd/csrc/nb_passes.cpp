// nb_passes.cpp -- everything an analysis pass does without a device: the refusal rules of every pass (the
// *_check_params and *_check_args that run before the simulator is looked at, and the two checks that read the
// simulator's parameters), the frames, edges and grids the passes and the host-only entry points share, and the
// bodies of the host-only entry points of include/nbody.h.  No HIP call is made here; the functions are declared
// in nb_sim.hpp next to the sim_X they guard.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "nb_common.hpp"
#include "nb_sim.hpp"

namespace nb {

// The frame nb_field_rings and the maps share (include/nbody.h): n the unit axis, e1 the coordinate axis
// of the smallest |n_k| made orthogonal to n, e2 = n x e1.
bool axis_frame(const double axis[3], double n[3], double e1[3], double e2[3]) {
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(axis[a])) return false;
    // (an axis whose length over- or underflows has no finite unit vector either)
    const double len = std::sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
    if (!(len > 0.0) || !std::isfinite(len)) return false;
    for (int a = 0; a < 3; ++a) n[a] = axis[a] / len;
    int s = 0;  // the coordinate axis of the smallest |n_k|, the lowest index on ties
    for (int a = 1; a < 3; ++a)
        if (std::fabs(n[a]) < std::fabs(n[s])) s = a;
    double el = 0.0;
    for (int a = 0; a < 3; ++a) {
        e1[a] = (a == s ? 1.0 : 0.0) - n[s] * n[a];
        el += e1[a] * e1[a];
    }
    el = std::sqrt(el);  // >= sqrt(2/3): |n_s| <= 1/sqrt(3)
    for (int a = 0; a < 3; ++a) e1[a] /= el;
    e2[0] = n[1] * e1[2] - n[2] * e1[1];
    e2[1] = n[2] * e1[0] - n[0] * e1[2];
    e2[2] = n[0] * e1[1] - n[1] * e1[0];
    return true;
}

// nb_sim_radial_profile: everything that can be refused without a device
int radial_check_params(const nb_radial_params *p, const nb_radial_profile *out, const nb_radial_bin *bins) {
    if (!p || !out || !bins || !p->edges) {
        set_error("radial_profile: null %s", !p ? "params" : !out ? "out" : !bins ? "bins" : "edges");
        return NB_ERR_INVALID;
    }
    if (p->nbins < 1 || p->nbins > NB_RADIAL_MAX_BINS) {
        set_error("radial_profile: nbins must be 1..%u (got %u)", NB_RADIAL_MAX_BINS, p->nbins);
        return NB_ERR_INVALID;
    }
    if (p->flags & ~(NB_RADIAL_CYLINDRICAL | NB_RADIAL_CENTER_COM)) {
        set_error("radial_profile: unknown flag bits 0x%x", p->flags & ~(NB_RADIAL_CYLINDRICAL | NB_RADIAL_CENTER_COM));
        return NB_ERR_INVALID;
    }
    for (uint32_t k = 0; k <= p->nbins; ++k) {
        const double e = p->edges[k];
        if (!std::isfinite(e) || e < 0.0 || (k > 0 && !(e > p->edges[k - 1]))) {
            set_error("radial_profile: edges must be finite, >= 0 and strictly ascending (edges[%u] = %g)", k, e);
            return NB_ERR_INVALID;
        }
    }
    if (!(p->flags & NB_RADIAL_CENTER_COM))
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(p->center[k]) || !std::isfinite(p->velocity[k])) {
                set_error("radial_profile: center and velocity must be finite");
                return NB_ERR_INVALID;
            }
    const double *a = p->axis;
    if (!std::isfinite(a[0]) || !std::isfinite(a[1]) || !std::isfinite(a[2])) {
        set_error("radial_profile: axis must be finite");
        return NB_ERR_INVALID;
    }
    if (p->flags & NB_RADIAL_CYLINDRICAL) {
        // (an axis whose length over- or underflows has no finite unit vector either)
        const double len = std::sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
        if (!(len > 0.0) || !std::isfinite(len)) {
            set_error("radial_profile: a cylindrical profile needs a non-zero axis");
            return NB_ERR_INVALID;
        }
    }
    return NB_OK;
}

int radial_edges(const char *what, bool log, double rmin, double rmax, uint32_t nbins, double *edges) {
    if (!edges) {
        set_error("%s: edges is null", what);
        return NB_ERR_INVALID;
    }
    if (nbins < 1 || nbins > NB_RADIAL_MAX_BINS) {
        set_error("%s: nbins must be 1..%u (got %u)", what, NB_RADIAL_MAX_BINS, nbins);
        return NB_ERR_INVALID;
    }
    if (!std::isfinite(rmin) || !std::isfinite(rmax) || !(rmax > rmin) || !(log ? rmin > 0.0 : rmin >= 0.0)) {
        set_error("%s: needs finite %s rmin < rmax (got %g, %g)", what, log ? "0 <" : "0 <=", rmin, rmax);
        return NB_ERR_INVALID;
    }
    double prev = rmin;
    for (uint32_t k = 1; k < nbins; ++k) {  // checked before anything is written
        const double t = (double)k / (double)nbins;
        const double e = log ? rmin * std::pow(rmax / rmin, t) : rmin + (rmax - rmin) * t;
        if (!(e > prev) || !(e < rmax)) {
            set_error("%s: %u bins between %g and %g are not strictly ascending in fp64", what, nbins, rmin, rmax);
            return NB_ERR_INVALID;
        }
        prev = e;
    }
    edges[0] = rmin;
    for (uint32_t k = 1; k < nbins; ++k) {
        const double t = (double)k / (double)nbins;
        edges[k] = log ? rmin * std::pow(rmax / rmin, t) : rmin + (rmax - rmin) * t;
    }
    edges[nbins] = rmax;
    return NB_OK;
}

// nb_sim_field / nb_tidal_sim: what can be refused about the points of a probe without a device
static int probe_check_args(const char *name, const float *points, size_t m, const void *out) {
    if (m > 0 && (!points || !out)) {
        set_error("%s: null %s", name, !points ? "points" : "out");
        return NB_ERR_INVALID;
    }
    if (m > NB_FIELD_MAX_POINTS) {
        set_error("%s: at most %u points (got %zu)", name, NB_FIELD_MAX_POINTS, m);
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

int field_check_args(const float *points, size_t m, uint32_t flags, const nb_field_sample *out) {
    if (int rc = probe_check_args("field", points, m, out)) return rc;
    if (!flags || (flags & ~(NB_FIELD_ACCEL | NB_FIELD_POTENTIAL))) {
        set_error("field: flags must be NB_FIELD_ACCEL, NB_FIELD_POTENTIAL or both (got 0x%x)", flags);
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

int tidal_check_args(const float *points, size_t m, const nb_tidal_sample *out) {
    return probe_check_args("tidal", points, m, out);
}

// nb_orbits_sim: the recorded states, the phase of a state, and everything that can be refused without a device
// (the softening is the simulator's: orbits_check_e)
uint32_t orbit_records(uint32_t steps, uint32_t every) {
    if (every == 0) return 0;
    return steps / every + 1u + (steps % every ? 1u : 0u);
}

int orbit_phase(double omega, double dt, uint64_t k, double *c, double *s) {
    if (!c || !s) {
        set_error("orbit_phase: null %s", !c ? "c" : "s");
        return NB_ERR_INVALID;
    }
    if (!std::isfinite(omega) || !std::isfinite(dt)) {
        set_error("orbit_phase: omega and dt must be finite (got %g, %g)", omega, dt);
        return NB_ERR_INVALID;
    }
    if (omega == 0.0) {
        *c = 1.0;
        *s = 0.0;
        return NB_OK;
    }
    const double t = (double)k * dt, theta = omega * t;
    *c = std::cos(theta);
    *s = std::sin(theta);
    return NB_OK;
}

int orbits_check_args(const nb_orbit_params *p, const double *pos, const double *vel, size_t m,
                      const nb_orbit_sample *tracks, OrbitPlan *plan) {
    if (!p) {
        set_error("orbits: null params");
        return NB_ERR_INVALID;
    }
    if (m > 0 && (!pos || !vel || !tracks)) {
        set_error("orbits: null %s", !pos ? "pos" : !vel ? "vel" : "tracks");
        return NB_ERR_INVALID;
    }
    if (p->steps < 1 || p->steps > NB_ORBIT_MAX_STEPS) {
        set_error("orbits: steps must be 1..%u (got %u)", NB_ORBIT_MAX_STEPS, p->steps);
        return NB_ERR_INVALID;
    }
    if (p->every < 1) {
        set_error("orbits: every must be at least 1");
        return NB_ERR_INVALID;
    }
    if ((p->flags & ~NB_ORBIT_ENERGY) || p->reserved) {
        set_error("orbits: unknown flag bits 0x%x or reserved %u != 0", p->flags & ~NB_ORBIT_ENERGY, p->reserved);
        return NB_ERR_INVALID;
    }
    if (m > NB_ORBIT_MAX_TRACERS) {
        set_error("orbits: at most %u tracers (got %zu)", NB_ORBIT_MAX_TRACERS, m);
        return NB_ERR_INVALID;
    }
    plan->records = orbit_records(p->steps, p->every);
    if ((uint64_t)plan->records * m > NB_ORBIT_MAX_SAMPLES) {
        set_error("orbits: %u records of %zu tracers are more than %u samples", plan->records, m, NB_ORBIT_MAX_SAMPLES);
        return NB_ERR_INVALID;
    }
    if (!std::isfinite(p->dt) || p->dt == 0.0) {
        set_error("orbits: dt must be finite and not zero (got %g)", p->dt);
        return NB_ERR_INVALID;
    }
    if (!std::isfinite(p->accel_scale)) {
        set_error("orbits: accel_scale must be finite (got %g)", p->accel_scale);
        return NB_ERR_INVALID;
    }
    if (!std::isfinite(p->omega)) {
        set_error("orbits: omega must be finite (got %g)", p->omega);
        return NB_ERR_INVALID;
    }
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(p->center[a])) {
            set_error("orbits: center must be finite");
            return NB_ERR_INVALID;
        }
    for (int a = 0; a < 3; ++a) plan->n[a] = plan->e1[a] = plan->e2[a] = 0.0;
    if (p->omega != 0.0 && !axis_frame(p->axis, plan->n, plan->e1, plan->e2)) {
        set_error("orbits: a pattern speed needs a non-zero finite axis");
        return NB_ERR_INVALID;
    }
    return NB_OK;
}
int orbits_check_e(const SimBase &s, const nb_orbit_params *p) {
    if ((p->flags & NB_ORBIT_ENERGY) && !(s.params.e >= 0.f)) {
        set_error("orbits: the potential needs e >= 0 (e = %g)", (double)s.params.e);
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// nb_orbit_sections_sim: nb_orbits_sim's refusals, then the section's; the frame is formed for omega == 0 too
int orbit_sections_check_args(const nb_orbit_params *p, const nb_orbit_section_params *sec, const double *pos,
                              const double *vel, size_t m, const nb_orbit_sample *tracks,
                              const nb_orbit_crossing *crossings, OrbitPlan *plan) {
    if (int rc = orbits_check_args(p, pos, vel, m, tracks, plan)) return rc;
    if (!sec) {
        set_error("orbit_sections: null section params");
        return NB_ERR_INVALID;
    }
    bool finite = true, zero = true;
    for (int a = 0; a < 3; ++a) {
        finite = finite && std::isfinite(sec->normal[a]);
        zero = zero && sec->normal[a] == 0.0;
    }
    if (!finite || zero) {
        set_error("orbit_sections: normal must be finite and not all zero");
        return NB_ERR_INVALID;
    }
    if (!std::isfinite(sec->offset)) {
        set_error("orbit_sections: offset must be finite (got %g)", sec->offset);
        return NB_ERR_INVALID;
    }
    if (sec->direction < -1 || sec->direction > 1) {
        set_error("orbit_sections: direction must be -1, 0 or 1 (got %d)", (int)sec->direction);
        return NB_ERR_INVALID;
    }
    if (sec->flags || sec->reserved) {
        set_error("orbit_sections: unknown flag bits 0x%x or reserved %u != 0", sec->flags, sec->reserved);
        return NB_ERR_INVALID;
    }
    if ((uint64_t)m * sec->max_crossings > NB_ORBIT_SECTION_MAX_CROSSINGS) {
        set_error("orbit_sections: %zu tracers of %u crossings are more than %u records", m, sec->max_crossings,
                  NB_ORBIT_SECTION_MAX_CROSSINGS);
        return NB_ERR_INVALID;
    }
    if (m > 0 && sec->max_crossings > 0 && !crossings) {
        set_error("orbit_sections: null crossings with max_crossings = %u", sec->max_crossings);
        return NB_ERR_INVALID;
    }
    if (!axis_frame(p->axis, plan->n, plan->e1, plan->e2)) {
        set_error("orbit_sections: the section's frame needs a non-zero finite axis");
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

int orbit_summary_merge(const nb_orbit_summary *a, const nb_orbit_summary *b, nb_orbit_summary *out) {
    if (!a || !b || !out) {
        set_error("orbit_summary_merge: null %s", !a ? "a" : !b ? "b" : "out");
        return NB_ERR_INVALID;
    }
    nb_orbit_summary r{};
    r.r2_min = std::fmin(a->r2_min, b->r2_min);
    r.r2_max = std::fmax(a->r2_max, b->r2_max);
    r.R2_min = std::fmin(a->R2_min, b->R2_min);
    r.R2_max = std::fmax(a->R2_max, b->R2_max);
    r.h_max = std::fmax(a->h_max, b->h_max);
    r.lz_min = std::fmin(a->lz_min, b->lz_min);
    r.lz_max = std::fmax(a->lz_max, b->lz_max);
    r.first_peri = a->first_peri != NB_ORBIT_NO_STEP ? a->first_peri : b->first_peri;
    r.last_peri = b->last_peri != NB_ORBIT_NO_STEP ? b->last_peri : a->last_peri;
    r.pericentres = a->pericentres + b->pericentres;
    r.apocentres = a->apocentres + b->apocentres;
    r.plane_ups = a->plane_ups + b->plane_ups;
    r.winding_pattern = a->winding_pattern + b->winding_pattern;
    r.winding_inertial = a->winding_inertial + b->winding_inertial;
    *out = r;
    return NB_OK;
}

// nb_orbit_stability_sim: nb_orbits_sim's refusals, then its own
int orbit_stability_check_args(const nb_orbit_params *p, const nb_orbit_stability_params *sp, const double *pos,
                               const double *vel, size_t m, const nb_orbit_deviation *dev0,
                               const nb_orbit_sample *tracks, const nb_orbit_deviation *devs, OrbitPlan *plan) {
    if (int rc = orbits_check_args(p, pos, vel, m, tracks, plan)) return rc;
    if (p->flags & NB_ORBIT_ENERGY) {
        set_error("orbit_stability: NB_ORBIT_ENERGY is not taken (the tracks are nb_orbits_sim's, which gives it)");
        return NB_ERR_INVALID;
    }
    if (!sp) {
        set_error("orbit_stability: null stability params");
        return NB_ERR_INVALID;
    }
    if (sp->deviations < 1 || sp->deviations > NB_ORBIT_MAX_DEVIATIONS) {
        set_error("orbit_stability: deviations must be 1..%u (got %u)", NB_ORBIT_MAX_DEVIATIONS, sp->deviations);
        return NB_ERR_INVALID;
    }
    if (sp->renorm_log2 < 1 || sp->renorm_log2 > NB_ORBIT_MAX_RENORM_LOG2) {
        set_error("orbit_stability: renorm_log2 must be 1..%u (got %u)", NB_ORBIT_MAX_RENORM_LOG2, sp->renorm_log2);
        return NB_ERR_INVALID;
    }
    if (sp->reserved) {
        set_error("orbit_stability: reserved %u != 0", sp->reserved);
        return NB_ERR_INVALID;
    }
    if (m > 0 && (!dev0 || !devs)) {
        set_error("orbit_stability: null %s", !dev0 ? "dev0" : "devs");
        return NB_ERR_INVALID;
    }
    if ((uint64_t)plan->records * m * sp->deviations > NB_ORBIT_MAX_SAMPLES) {
        set_error("orbit_stability: %u records of %zu tracers with %u vectors are more than %u samples", plan->records,
                  m, sp->deviations, NB_ORBIT_MAX_SAMPLES);
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// nb_orbit_stability_derive: the norm of a vector as 2^E sqrt(sum (d_i 2^-E)^2), its ln, and the unit vector
static bool deviation_unit(const nb_orbit_deviation &v, double *ln_norm, double u[6]) {
    double mu = 0.0;
    for (int i = 0; i < 6; ++i) {
        if (!std::isfinite(v.d[i])) return false;
        mu = std::fmax(mu, std::fabs(v.d[i]));
    }
    if (mu == 0.0) return false;
    int ex = 0;
    (void)std::frexp(mu, &ex);
    double s[6], sum = 0.0;
    for (int i = 0; i < 6; ++i) {
        s[i] = std::ldexp(v.d[i], -ex);
        sum += s[i] * s[i];
    }
    const double norm = std::sqrt(sum);
    for (int i = 0; i < 6; ++i) u[i] = s[i] / norm;
    *ln_norm = (double)ex * M_LN2 + std::log(norm);
    return true;
}

int orbit_stability_derive(double dt, uint32_t steps, uint32_t every, size_t m, uint32_t D,
                           const nb_orbit_deviation *dev0, const nb_orbit_deviation *devs, double *log_growth,
                           double *lyapunov, double *sali, double *gali2) {
    if (m > 0 && (!dev0 || !devs)) {
        set_error("orbit_stability_derive: null %s", !dev0 ? "dev0" : "devs");
        return NB_ERR_INVALID;
    }
    if (D < 1 || D > NB_ORBIT_MAX_DEVIATIONS || steps < 1 || every < 1 || !std::isfinite(dt) || dt == 0.0) {
        set_error("orbit_stability_derive: deviations must be 1..%u, steps and every at least 1, dt finite and not "
                  "zero (got %u, %u, %u, %g)", NB_ORBIT_MAX_DEVIATIONS, D, steps, every, dt);
        return NB_ERR_INVALID;
    }
    size_t r = 0;
    for (uint32_t k = 0; k <= steps; ++k) {
        if (k % every != 0 && k != steps) continue;
        for (size_t i = 0; i < m; ++i) {
            double u[2][6] = {};
            bool have[2] = {false, false};
            for (uint32_t j = 0; j < D; ++j) {
                const size_t at = (r * m + i) * D + j;
                const nb_orbit_deviation &v = devs[at], &v0 = dev0[i * D + j];
                double ln = 0.0, ln0 = 0.0, uj[6], u0[6];
                const bool ok = deviation_unit(v, &ln, uj), ok0 = deviation_unit(v0, &ln0, u0);
                const double lg = ok && ok0 ? (double)(v.log2 - v0.log2) * M_LN2 + ln - ln0 : (double)NAN;
                if (log_growth) log_growth[at] = lg;
                if (lyapunov) lyapunov[at] = k > 0 ? lg / ((double)k * dt) : (double)NAN;
                if (j < 2) {
                    have[j] = ok;
                    for (int a = 0; a < 6; ++a) u[j][a] = uj[a];
                }
            }
            double sa = NAN, ga = NAN;
            if (D >= 2 && have[0] && have[1]) {
                double plus = 0.0, minus = 0.0, wedge = 0.0;
                for (int a = 0; a < 6; ++a) {
                    const double p = u[0][a] + u[1][a], q = u[0][a] - u[1][a];
                    plus += p * p;
                    minus += q * q;
                    for (int b = a + 1; b < 6; ++b) {
                        const double c = u[0][a] * u[1][b] - u[0][b] * u[1][a];
                        wedge += c * c;
                    }
                }
                sa = std::sqrt(std::fmin(plus, minus));
                ga = std::sqrt(wedge);
            }
            if (sali) sali[r * m + i] = sa;
            if (gali2) gali2[r * m + i] = ga;
        }
        ++r;
    }
    return NB_OK;
}

// nb_field_rings / nb_field_ring_means / nb_tidal_ring_means: the unit axis n and the ring basis e1, e2 = n x e1
static int ring_basis(const char *what, const double *center, const double *axis, const double *radii, uint32_t k,
                      uint32_t n_phi, double n[3], double e1[3], double e2[3]) {
    if (!center || !axis || (k && !radii)) {
        set_error("%s: null %s", what, !center ? "center" : !axis ? "axis" : "radii");
        return NB_ERR_INVALID;
    }
    if (n_phi == 0) {
        set_error("%s: n_phi must be at least 1", what);
        return NB_ERR_INVALID;
    }
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(center[a]) || !std::isfinite(axis[a])) {
            set_error("%s: center and axis must be finite", what);
            return NB_ERR_INVALID;
        }
    double fn[3], f1[3], f2[3];  // (nothing is written on a refusal)
    if (!axis_frame(axis, fn, f1, f2)) {
        set_error("%s: needs a non-zero axis", what);
        return NB_ERR_INVALID;
    }
    for (uint32_t i = 0; i < k; ++i)
        if (!std::isfinite(radii[i]) || radii[i] < 0.0) {
            set_error("%s: radii must be finite and >= 0 (radii[%u] = %g)", what, i, radii[i]);
            return NB_ERR_INVALID;
        }
    for (int a = 0; a < 3; ++a) {
        n[a] = fn[a];
        e1[a] = f1[a];
        e2[a] = f2[a];
    }
    return NB_OK;
}

// nb_sim_fof: everything that can be refused without a device
int fof_check_params(const nb_fof_params *p) {
    if (!p) {
        set_error("fof: null params");
        return NB_ERR_INVALID;
    }
    if (!std::isfinite(p->link) || !(p->link > 0.0)) {
        set_error("fof: link must be finite and > 0 (got %g)", p->link);
        return NB_ERR_INVALID;
    }
    const double b2 = p->link * p->link;  // what the rule compares with
    if (!(b2 > 0.0) || !std::isfinite(b2)) {
        set_error("fof: link %g squared is not a positive finite double", p->link);
        return NB_ERR_INVALID;
    }
    if (p->min_members < 1) {
        set_error("fof: min_members must be at least 1");
        return NB_ERR_INVALID;
    }
    if (p->flags || p->reserved) {
        set_error("fof: unknown flag bits 0x%x or reserved %llu != 0", p->flags, (unsigned long long)p->reserved);
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// nb_fof6_sim: everything that can be refused without a device
int fof6_check_params(const nb_fof6_params *p) {
    if (!p) {
        set_error("fof6: null params");
        return NB_ERR_INVALID;
    }
    if (!std::isfinite(p->link) || !(p->link > 0.0) || !std::isfinite(p->vlink) || !(p->vlink > 0.0)) {
        set_error("fof6: link and vlink must be finite and > 0 (got %g, %g)", p->link, p->vlink);
        return NB_ERR_INVALID;
    }
    const double b2 = p->link * p->link, v2 = p->vlink * p->vlink, rhs = b2 * v2;  // what the rule compares with
    if (!(b2 > 0.0) || !std::isfinite(b2) || !(v2 > 0.0) || !std::isfinite(v2) || !(rhs > 0.0) || !std::isfinite(rhs)) {
        set_error("fof6: link %g squared, vlink %g squared or their product is not a positive finite double", p->link,
                  p->vlink);
        return NB_ERR_INVALID;
    }
    if (p->min_members < 1) {
        set_error("fof6: min_members must be at least 1");
        return NB_ERR_INVALID;
    }
    if (p->flags || p->reserved) {
        set_error("fof6: unknown flag bits 0x%x or reserved %llu != 0", p->flags, (unsigned long long)p->reserved);
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// nb_sim_bound: everything that can be refused without a device (the softening is the simulator's: bound_check_e)
int bound_check_params(const nb_bound_params *p) {
    if (!p) {
        set_error("bound: null params");
        return NB_ERR_INVALID;
    }
    nb_fof_params fp{};
    fp.link = p->link;
    fp.min_members = p->min_members;
    if (int rc = fof_check_params(&fp)) return rc;
    if (p->max_iter < 1 || p->max_iter > NB_BOUND_MAX_ITER) {
        set_error("bound: max_iter must be 1..%u (got %u)", NB_BOUND_MAX_ITER, p->max_iter);
        return NB_ERR_INVALID;
    }
    if (p->min_bound < 1) {
        set_error("bound: min_bound must be at least 1");
        return NB_ERR_INVALID;
    }
    if (p->flags || p->reserved32 || p->reserved) {
        set_error("bound: unknown flag bits 0x%x or a reserved field != 0", p->flags);
        return NB_ERR_INVALID;
    }
    return NB_OK;
}
int bound_check_e(const SimBase &s) {
    if (!(s.params.e >= 0.f)) {
        set_error("bound: the pair potential needs e >= 0 (e = %g)", (double)s.params.e);
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// nb_sim_group_shapes: everything that can be refused without a device -- the parameters alone, then (a handle in
// hand) what needs the simulator's n and step number
int shape_check_params(const nb_shape_params *p) {
    if (!p) {
        set_error("group_shapes: null params");
        return NB_ERR_INVALID;
    }
    if ((p->flags & ~NB_SHAPE_REDUCED) || p->reserved32 || p->reserved) {
        set_error("group_shapes: unknown flag bits 0x%x or a reserved field != 0", p->flags);
        return NB_ERR_INVALID;
    }
    if (p->min_members < 1) {
        set_error("group_shapes: min_members must be at least 1");
        return NB_ERR_INVALID;
    }
    if (p->max_iter < 1 || p->max_iter > NB_SHAPE_MAX_ITER) {
        set_error("group_shapes: max_iter must be 1..%u (got %u)", NB_SHAPE_MAX_ITER, p->max_iter);
        return NB_ERR_INVALID;
    }
    if (!std::isfinite(p->tol) || !(p->tol > 0.0)) {
        set_error("group_shapes: tol must be finite and > 0 (got %g)", p->tol);
        return NB_ERR_INVALID;
    }
    return NB_OK;
}
int shape_check_args(const SimBase &s, const nb_shape_params *p, const uint32_t *group_of, size_t m,
                     const double *centers, const double *velocities, const double *radius) {
    if (s.n > 0 && !group_of) {
        set_error("group_shapes: null group_of");
        return NB_ERR_INVALID;
    }
    if (m > std::max<size_t>(s.n, 1)) {
        set_error("group_shapes: %zu rows are more than %u bodies can fill", m, s.n);
        return NB_ERR_INVALID;
    }
    for (size_t k = 0; k < 3 * m; ++k)
        if ((centers && !std::isfinite(centers[k])) || (velocities && !std::isfinite(velocities[k]))) {
            set_error("group_shapes: the centre or the velocity of row %zu is not finite", k / 3);
            return NB_ERR_INVALID;
        }
    const bool reduced = (p->flags & NB_SHAPE_REDUCED) != 0;
    if (reduced && !radius && m > 0) {
        set_error("group_shapes: NB_SHAPE_REDUCED needs a finite radius for every row (radius is null)");
        return NB_ERR_INVALID;
    }
    for (size_t r = 0; radius && r < m; ++r) {
        if (!(radius[r] > 0.0)) {  // (a NaN too)
            set_error("group_shapes: radius[%zu] = %g is neither finite and > 0 nor +inf", r, radius[r]);
            return NB_ERR_INVALID;
        }
        if (reduced && std::isinf(radius[r])) {
            set_error("group_shapes: NB_SHAPE_REDUCED needs a finite radius (radius[%zu] is +inf)", r);
            return NB_ERR_INVALID;
        }
    }
    if (p->step_num != NB_SHAPE_ANY_STEP && p->step_num != s.step_num) {
        set_error("group_shapes: the assignment was made at step %llu, the simulator is at step %llu",
                  (unsigned long long)p->step_num, (unsigned long long)s.step_num);
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// nb_group_radii_sim: everything that can be refused without a device, split as nb_sim_group_shapes' checks are
int radii_check_params(const nb_radii_params *p) {
    if (!p) {
        set_error("group_radii: null params");
        return NB_ERR_INVALID;
    }
    if (p->reserved) {
        set_error("group_radii: a reserved field != 0");
        return NB_ERR_INVALID;
    }
    if (p->nf < 1 || p->nf > NB_RADII_MAX_FRACTIONS) {
        set_error("group_radii: nf must be 1..%u (got %u)", NB_RADII_MAX_FRACTIONS, p->nf);
        return NB_ERR_INVALID;
    }
    for (uint32_t f = 0; f < p->nf; ++f) {
        const double x = p->fractions[f];
        if (!std::isfinite(x) || !(x > 0.0) || !(x <= 1.0)) {
            set_error("group_radii: fractions[%u] = %g is not finite and in (0, 1]", f, x);
            return NB_ERR_INVALID;
        }
        if (f > 0 && !(x > p->fractions[f - 1])) {
            set_error("group_radii: fractions[%u] = %g is not above fractions[%u] = %g (strictly ascending)", f, x,
                      f - 1, p->fractions[f - 1]);
            return NB_ERR_INVALID;
        }
    }
    return NB_OK;
}
int radii_check_args(const SimBase &s, const nb_radii_params *p, const uint32_t *group_of, size_t m,
                     const double *centers) {
    if (s.n > 0 && !group_of) {
        set_error("group_radii: null group_of");
        return NB_ERR_INVALID;
    }
    if (m > std::max<size_t>(s.n, 1)) {
        set_error("group_radii: %zu rows are more than %u bodies can fill", m, s.n);
        return NB_ERR_INVALID;
    }
    for (size_t k = 0; centers && k < 3 * m; ++k)
        if (!std::isfinite(centers[k])) {
            set_error("group_radii: the centre of row %zu is not finite", k / 3);
            return NB_ERR_INVALID;
        }
    if (p->step_num != NB_RADII_ANY_STEP && p->step_num != s.step_num) {
        set_error("group_radii: the assignment was made at step %llu, the simulator is at step %llu",
                  (unsigned long long)p->step_num, (unsigned long long)s.step_num);
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// nb_disc_modes_sim: everything that can be refused without a device; the edges exactly as radial_check_params'
int modes_check_params(const nb_modes_params *p, const nb_modes_head *out, const nb_modes_bin *bins,
                       const double *modes) {
    if (!p || !out || !bins || !modes || !p->edges) {
        set_error("disc_modes: null %s", !p ? "params" : !out ? "out" : !bins ? "bins" : !modes ? "modes" : "edges");
        return NB_ERR_INVALID;
    }
    if (p->nbins < 1 || p->nbins > NB_MODES_MAX_BINS) {
        set_error("disc_modes: nbins must be 1..%u (got %u)", NB_MODES_MAX_BINS, p->nbins);
        return NB_ERR_INVALID;
    }
    if (p->mmax > NB_MODES_MAX_M) {
        set_error("disc_modes: mmax must be 0..%u (got %u)", NB_MODES_MAX_M, p->mmax);
        return NB_ERR_INVALID;
    }
    if (p->flags & ~NB_MODES_CENTER_COM) {
        set_error("disc_modes: unknown flag bits 0x%x", p->flags & ~NB_MODES_CENTER_COM);
        return NB_ERR_INVALID;
    }
    if (p->reserved) {
        set_error("disc_modes: a reserved field != 0");
        return NB_ERR_INVALID;
    }
    for (uint32_t k = 0; k <= p->nbins; ++k) {
        const double e = p->edges[k];
        if (!std::isfinite(e) || e < 0.0 || (k > 0 && !(e > p->edges[k - 1]))) {
            set_error("disc_modes: edges must be finite, >= 0 and strictly ascending (edges[%u] = %g)", k, e);
            return NB_ERR_INVALID;
        }
    }
    if (!(p->flags & NB_MODES_CENTER_COM))
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(p->center[k]) || !std::isfinite(p->velocity[k])) {
                set_error("disc_modes: center and velocity must be finite");
                return NB_ERR_INVALID;
            }
    double n[3], e1[3], e2[3];
    if (!axis_frame(p->axis, n, e1, e2)) {
        set_error("disc_modes: needs a non-zero finite axis");
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// nb_disc_modes_derive
int modes_derive(const double *modes, uint32_t nbins, uint32_t mmax, uint32_t m, nb_modes_derived *out) {
#pragma clang fp contract(off)
    if (!modes || !out) {
        set_error("disc_modes_derive: null %s", !modes ? "modes" : "out");
        return NB_ERR_INVALID;
    }
    if (nbins < 1 || nbins > NB_MODES_MAX_BINS || mmax > NB_MODES_MAX_M || m < 1 || m > mmax) {
        set_error("disc_modes_derive: needs nbins in 1..%u, mmax in 0..%u and 1 <= m <= mmax (got %u, %u, %u)",
                  NB_MODES_MAX_BINS, NB_MODES_MAX_M, nbins, mmax, m);
        return NB_ERR_INVALID;
    }
    const double nan = std::nan("");
    for (uint32_t k = 0; k < nbins; ++k) {
        const double *f0 = modes + (size_t)k * (mmax + 1) * NB_MODES_FIELDS, *f = f0 + (size_t)m * NB_MODES_FIELDS;
        const double c0 = f0[NB_MODES_C], c = f[NB_MODES_C], s = f[NB_MODES_S];
        const double zc = f[NB_MODES_ZC], zs = f[NB_MODES_ZS];
        nb_modes_derived d{nan, nan, nan, nan, nan};
        if (c0 != 0.0 && c0 == c0) {  // (a NaN C_0: NaN throughout, as without mass)
            const double p2 = c * c + s * s, z2 = zc * zc + zs * zs;
            d.amplitude = std::hypot(c, s) / c0;
            d.bend_amplitude = std::hypot(zc, zs) / c0;
            if (p2 != 0.0) {
                d.phase = std::atan2(s, c) / (double)m;
                d.pattern_speed = (c * f[NB_MODES_DC] + s * f[NB_MODES_DS]) / p2;
            }
            if (z2 != 0.0) d.bend_phase = std::atan2(zs, zc) / (double)m;
        }
        out[k] = d;
    }
    return NB_OK;
}

// nb_shell_modes_sim: everything that can be refused without a device, as modes_check_params
int shell_check_params(const nb_shell_params *p, const nb_shell_head *out, const nb_shell_bin *bins,
                       const double *coef) {
    if (!p || !out || !bins || !coef || !p->edges) {
        set_error("shell_modes: null %s", !p ? "params" : !out ? "out" : !bins ? "bins" : !coef ? "coef" : "edges");
        return NB_ERR_INVALID;
    }
    if (p->nbins < 1 || p->nbins > NB_SHELL_MAX_BINS) {
        set_error("shell_modes: nbins must be 1..%u (got %u)", NB_SHELL_MAX_BINS, p->nbins);
        return NB_ERR_INVALID;
    }
    if (p->flags & ~(NB_SHELL_CENTER_COM | NB_SHELL_RATES)) {
        set_error("shell_modes: unknown flag bits 0x%x", p->flags & ~(NB_SHELL_CENTER_COM | NB_SHELL_RATES));
        return NB_ERR_INVALID;
    }
    const uint32_t lcap = (p->flags & NB_SHELL_RATES) ? NB_SHELL_MAX_L_RATES : NB_SHELL_MAX_L;
    if (p->lmax > lcap) {
        set_error("shell_modes: lmax must be 0..%u%s (got %u)", lcap,
                  (p->flags & NB_SHELL_RATES) ? " with NB_SHELL_RATES" : "", p->lmax);
        return NB_ERR_INVALID;
    }
    if (p->reserved) {
        set_error("shell_modes: a reserved field != 0");
        return NB_ERR_INVALID;
    }
    for (uint32_t k = 0; k <= p->nbins; ++k) {
        const double e = p->edges[k];
        if (!std::isfinite(e) || e < 0.0 || (k > 0 && !(e > p->edges[k - 1]))) {
            set_error("shell_modes: edges must be finite, >= 0 and strictly ascending (edges[%u] = %g)", k, e);
            return NB_ERR_INVALID;
        }
    }
    if (!(p->flags & NB_SHELL_CENTER_COM))
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(p->center[k]) || !std::isfinite(p->velocity[k])) {
                set_error("shell_modes: center and velocity must be finite");
                return NB_ERR_INVALID;
            }
    double n[3], e1[3], e2[3];
    if (!axis_frame(p->axis, n, e1, e2)) {
        set_error("shell_modes: needs a non-zero finite axis");
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// nb_shell_modes_derive
int shell_derive(const nb_shell_head *head, const double *coef, nb_shell_derived *out, double *norm, double *phase,
                 double *speed) {
#pragma clang fp contract(off)
    if (!head || !coef || !out) {
        set_error("shell_modes_derive: null %s", !head ? "head" : !coef ? "coef" : "out");
        return NB_ERR_INVALID;
    }
    const uint32_t nbins = head->nbins, lmax = head->lmax;
    const bool rates = (head->flags & NB_SHELL_RATES) != 0;
    if (nbins < 1 || nbins > NB_SHELL_MAX_BINS || lmax > (rates ? NB_SHELL_MAX_L_RATES : NB_SHELL_MAX_L) ||
        (head->flags & ~(NB_SHELL_CENTER_COM | NB_SHELL_RATES))) {
        set_error("shell_modes_derive: needs nbins in 1..%u, lmax in 0..%u (0..%u with rates) and known flags "
                  "(got %u, %u, 0x%x)",
                  NB_SHELL_MAX_BINS, NB_SHELL_MAX_L, NB_SHELL_MAX_L_RATES, nbins, lmax, head->flags);
        return NB_ERR_INVALID;
    }
    constexpr uint32_t kMaxK = (NB_SHELL_MAX_L + 1) * (NB_SHELL_MAX_L + 1);
    const uint32_t nk = (lmax + 1) * (lmax + 1), stride = nk * (rates ? 2u : 1u);
    const double nan = std::nan("");
    double fact[2 * NB_SHELL_MAX_L + 1], nlm[kMaxK];
    fact[0] = 1.0;
    for (uint32_t j = 1; j <= 2 * NB_SHELL_MAX_L; ++j) fact[j] = fact[j - 1] * (double)j;  // (exact)
    for (uint32_t l = 0; l <= lmax; ++l) {
        const double f = (double)(2 * l + 1) / NB_SHELL_FOUR_PI;
        nlm[l * l] = std::sqrt(f);
        for (uint32_t m = 1; m <= l; ++m)
            nlm[l * l + 2 * m - 1] = nlm[l * l + 2 * m] = std::sqrt((2.0 * f) * (fact[l - m] / fact[l + m]));
    }
    const double *fn = head->axis, *f1 = head->e1, *f2 = head->e2;
    for (uint32_t k = 0; k < nbins; ++k) {
        const double *c = coef + (size_t)k * stride;
        double a[kMaxK];
        for (uint32_t i = 0; i < nk; ++i) {
            a[i] = nlm[i] * c[i];
            if (norm) norm[(size_t)k * nk + i] = a[i];
            if (phase) phase[(size_t)k * nk + i] = nan;
            if (speed) speed[(size_t)k * nk + i] = nan;
        }
        nb_shell_derived d;
        for (uint32_t l = 0; l <= NB_SHELL_MAX_L; ++l) d.power[l] = d.relative[l] = nan;
        for (int j = 0; j < 3; ++j) d.dipole[j] = d.quad_values[j] = nan;
        for (int j = 0; j < 9; ++j) d.quad_axes[j] = nan;
        for (uint32_t l = 0; l <= lmax; ++l) {
            double sum = a[l * l] * a[l * l];
            for (uint32_t i = l * l + 1; i < (l + 1) * (l + 1); ++i) sum = sum + a[i] * a[i];
            d.power[l] = sum / (double)(2 * l + 1);
        }
        if (d.power[0] != 0.0 && d.power[0] == d.power[0])
            for (uint32_t l = 0; l <= lmax; ++l) d.relative[l] = std::sqrt(d.power[l] / d.power[0]);
        for (uint32_t l = 1; l <= lmax; ++l)
            for (uint32_t m = 1; m <= l; ++m) {
                const uint32_t i = l * l + 2 * m - 1;
                const double cc = c[i], ss = c[i + 1], p2 = cc * cc + ss * ss;
                if (p2 == 0.0 || p2 != p2) continue;
                if (phase) phase[(size_t)k * nk + i] = std::atan2(ss, cc) / (double)m;
                if (speed && rates)
                    speed[(size_t)k * nk + i] = (cc * c[nk + i + 1] - ss * c[nk + i]) / ((double)m * p2);
            }
        if (lmax >= 1)
            for (int j = 0; j < 3; ++j) d.dipole[j] = (a[2] * f1[j] + a[3] * f2[j]) + a[1] * fn[j];
        if (lmax >= 2) {
            const double q0 = nlm[4] * a[4], q1c = nlm[5] * a[5], q1s = nlm[6] * a[6], q2c = nlm[7] * a[7],
                         q2s = nlm[8] * a[8];
            double t[3][3], w[3][3], m6[6];
            t[0][0] = (-0.5 * q0) + 3.0 * q2c;
            t[1][1] = (-0.5 * q0) - 3.0 * q2c;
            t[2][2] = q0;
            t[0][1] = t[1][0] = 3.0 * q2s;
            t[0][2] = t[2][0] = 1.5 * q1c;
            t[1][2] = t[2][1] = 1.5 * q1s;
            for (int i = 0; i < 3; ++i)
                for (int b = 0; b < 3; ++b) w[i][b] = (f1[i] * t[0][b] + f2[i] * t[1][b]) + fn[i] * t[2][b];
            int e = 0;
            for (int i = 0; i < 3; ++i)
                for (int j = i; j < 3; ++j) m6[e++] = (w[i][0] * f1[j] + w[i][1] * f2[j]) + w[i][2] * fn[j];
            shape_eigen_host(m6, d.quad_values, d.quad_axes);  // (xx, xy, xz, yy, yz, zz)
        }
        out[k] = d;
    }
    return NB_OK;
}

// nb_sim_knn: everything that can be refused without a device
int knn_check_params(const nb_knn_params *p) {
    if (!p) {
        set_error("knn: null params");
        return NB_ERR_INVALID;
    }
    if (p->k < 1 || p->k > NB_KNN_MAX_K) {
        set_error("knn: k must be 1..%u (got %u)", NB_KNN_MAX_K, p->k);
        return NB_ERR_INVALID;
    }
    if (p->flags || p->reserved) {
        set_error("knn: unknown flag bits 0x%x or reserved %llu != 0", p->flags, (unsigned long long)p->reserved);
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// nb_local_kinematics_sim: everything that can be refused without a device
int kin_check_params(const nb_kin_params *p) {
    if (!p) {
        set_error("local_kinematics: null params");
        return NB_ERR_INVALID;
    }
    if (p->k < 1 || p->k > NB_KNN_MAX_K) {
        set_error("local_kinematics: k must be 1..%u (got %u)", NB_KNN_MAX_K, p->k);
        return NB_ERR_INVALID;
    }
    if ((p->flags & ~NB_KIN_SELF) || p->reserved) {
        set_error("local_kinematics: unknown flag bits 0x%x or reserved %llu != 0", p->flags & ~NB_KIN_SELF,
                  (unsigned long long)p->reserved);
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// nb_local_kinematics_derive
int kin_derive(const double *moments, const double *grads, const double *r2, const double *density,
               const float *velocities, size_t n, nb_kin_derived *out) {
#pragma clang fp contract(off)
    if (n > 0 && (!moments || !r2 || !out)) {
        set_error("local_kinematics_derive: null %s", !moments ? "moments" : !r2 ? "r2" : "out");
        return NB_ERR_INVALID;
    }
    const double nan = std::nan("");
    for (size_t i = 0; i < n; ++i) {
        const double *s = moments + i * NB_KIN_MOMENTS;
        nb_kin_derived d{};
        const auto fill = [nan](double *a, int count) {
            for (int q = 0; q < count; ++q) a[q] = nan;
        };
        d.mass = s[0];
        fill(d.relative_velocity, 3);
        fill(d.mean_velocity, 3);
        fill(d.dispersion, 6);
        d.sigma2 = d.sigma = d.phase_space_density = nan;
        fill(d.gradient, 9);
        d.det = d.divergence = d.shear = nan;
        fill(d.vorticity, 3);
        d.status = std::isnan(r2[i]) ? NB_KIN_NOT_COUNTED : std::isinf(r2[i]) ? NB_KIN_SHORT
                   : r2[i] == 0.0    ? NB_KIN_DEGENERATE
                                     : 0u;
        if (!(d.status & (NB_KIN_NOT_COUNTED | NB_KIN_SHORT))) {
            double u[3];
            for (int a = 0; a < 3; ++a) {
                u[a] = s[1 + a] / s[0];
                d.relative_velocity[a] = u[a];
                if (velocities) d.mean_velocity[a] = (double)velocities[3 * i + a] + u[a];
            }
            static const int ia[6] = {0, 0, 0, 1, 1, 2}, ib[6] = {0, 1, 2, 1, 2, 2};
            for (int q = 0; q < 6; ++q) d.dispersion[q] = s[4 + q] / s[0] - u[ia[q]] * u[ib[q]];
            d.sigma2 = ((d.dispersion[0] + d.dispersion[3]) + d.dispersion[5]) / 3.0;
            d.sigma = d.sigma2 < 0.0 ? 0.0 : std::sqrt(d.sigma2);
            if (density) d.phase_space_density = density[i] / (d.sigma2 * d.sigma);
            if (grads) {
                const double *g = grads + i * NB_KIN_GRADS, *c = g + 6;
                const double xx = g[0], xy = g[1], xz = g[2], yy = g[3], yz = g[4], zz = g[5];
                double adj[3][3];
                adj[0][0] = yy * zz - yz * yz;
                adj[0][1] = adj[1][0] = xz * yz - xy * zz;
                adj[0][2] = adj[2][0] = xy * yz - xz * yy;
                adj[1][1] = xx * zz - xz * xz;
                adj[1][2] = adj[2][1] = xy * xz - xx * yz;
                adj[2][2] = xx * yy - xy * xy;
                const double det = (xx * adj[0][0] + xy * adj[0][1]) + xz * adj[0][2];
                d.det = det;
                if (!(det > 0x1p-30 * ((xx * yy) * zz))) {
                    d.status |= NB_KIN_SINGULAR;
                } else {
                    double *G = d.gradient;
                    for (int a = 0; a < 3; ++a)
                        for (int b = 0; b < 3; ++b)
                            G[3 * a + b] =
                                ((c[3 * a] * adj[0][b] + c[3 * a + 1] * adj[1][b]) + c[3 * a + 2] * adj[2][b]) / det;
                    d.divergence = (G[0] + G[4]) + G[8];
                    d.vorticity[0] = G[7] - G[5];
                    d.vorticity[1] = G[2] - G[6];
                    d.vorticity[2] = G[3] - G[1];
                    const double t = d.divergence / 3.0;
                    const double sxx = G[0] - t, syy = G[4] - t, szz = G[8] - t;
                    const double sxy = (G[1] + G[3]) / 2.0, sxz = (G[2] + G[6]) / 2.0, syz = (G[5] + G[7]) / 2.0;
                    d.shear = std::sqrt(((sxx * sxx + syy * syy) + szz * szz) +
                                        2.0 * ((sxy * sxy + sxz * sxz) + syz * syz));
                }
            }
        }
        out[i] = d;
    }
    return NB_OK;
}

// nb_sim_hop: everything that can be refused without a device
int hop_check_params(const nb_hop_params *p) {
    if (!p) {
        set_error("hop: null params");
        return NB_ERR_INVALID;
    }
    if (p->k_density < 2 || p->k_density > NB_KNN_MAX_K) {
        set_error("hop: k_density must be 2..%u (got %u)", NB_KNN_MAX_K, p->k_density);
        return NB_ERR_INVALID;
    }
    if (p->k_hop < 1 || p->k_hop > NB_KNN_MAX_K || p->k_merge < 1 || p->k_merge > NB_KNN_MAX_K) {
        set_error("hop: k_hop and k_merge must be 1..%u (got %u, %u)", NB_KNN_MAX_K, p->k_hop, p->k_merge);
        return NB_ERR_INVALID;
    }
    if (p->min_members < 1) {
        set_error("hop: min_members must be at least 1");
        return NB_ERR_INVALID;
    }
    if (std::isnan(p->density_min)) {
        set_error("hop: density_min must not be NaN (-inf: no cut)");
        return NB_ERR_INVALID;
    }
    if (p->flags || p->reserved32 || p->reserved) {
        set_error("hop: unknown flag bits 0x%x or a reserved field != 0", p->flags);
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// nb_hop_regroup behind the ABI boundary (include/nbody.h: the rule, step by step)
// the ordering key of a density, and the "denser" order of include/nbody.h
static double hop_rho_key(double d) { return std::isnan(d) ? -INFINITY : d; }
static bool hop_denser(double ra, uint32_t a, double rb, uint32_t b) { return ra > rb || (ra == rb && a < b); }

int hop_regroup(const nb_fof_group *rows, const double *peak_density, size_t m, const nb_hop_boundary *bnd,
                size_t b, const nb_hop_regroup_params *params, uint32_t *merged_of_row, nb_fof_group *out_rows,
                double *out_peak, size_t out_capacity, size_t *out_count) {
    {
        if (!params || !out_count || (m && (!rows || !peak_density)) || (b && !bnd)) {
            set_error("hop_regroup: null argument");
            return NB_ERR_INVALID;
        }
        if (std::isnan(params->saddle) || std::isnan(params->peak) || params->saddle > params->peak) {
            set_error("hop_regroup: saddle and peak must not be NaN, with saddle <= peak (got %g, %g)", params->saddle,
                      params->peak);
            return NB_ERR_INVALID;
        }
        if (params->flags || params->reserved) {
            set_error("hop_regroup: unknown flag bits 0x%x or reserved != 0", params->flags);
            return NB_ERR_INVALID;
        }
        for (size_t r = 1; r < m; ++r)
            if (!(rows[r - 1].label < rows[r].label)) {
                set_error("hop_regroup: rows must be in strictly ascending label order (row %zu)", r);
                return NB_ERR_INVALID;
            }
        for (size_t e = 0; e < b; ++e) {
            const bool ordered = e == 0 || bnd[e - 1].a < bnd[e].a || (bnd[e - 1].a == bnd[e].a && bnd[e - 1].b < bnd[e].b);
            if (!ordered || !(bnd[e].a < bnd[e].b)) {
                set_error("hop_regroup: boundaries must be in strictly ascending (a, b) with a < b (boundary %zu)", e);
                return NB_ERR_INVALID;
            }
        }
        // the row of a label: a binary search in the ascending labels
        auto row_of = [&](uint32_t label) -> size_t {
            size_t lo = 0, hi = m;
            while (lo < hi) {
                const size_t mid = lo + (hi - lo) / 2;
                if (rows[mid].label < label) lo = mid + 1;
                else hi = mid;
            }
            return lo < m && rows[lo].label == label ? lo : m;
        };
        struct Edge {
            double density;
            size_t ra, rb, at;
        };
        std::vector<Edge> edges;
        for (size_t e = 0; e < b; ++e) {
            const size_t ra = row_of(bnd[e].a), rb = row_of(bnd[e].b);
            if (ra < m && rb < m) edges.push_back({bnd[e].density, ra, rb, e});
        }
        // descending density (a NaN as -inf, like a peak's), ties in ascending (a, b) -- the table's own order
        std::stable_sort(edges.begin(), edges.end(), [](const Edge &x, const Edge &y) {
            return hop_rho_key(x.density) > hop_rho_key(y.density);
        });
        std::vector<size_t> parent(m);
        std::vector<char> viable(m);  // of a root: its set's
        for (size_t r = 0; r < m; ++r) {
            parent[r] = r;
            viable[r] = hop_rho_key(peak_density[r]) >= params->peak;
        }
        auto find = [&](size_t x) {
            while (parent[x] != x) {
                parent[x] = parent[parent[x]];
                x = parent[x];
            }
            return x;
        };
        for (const Edge &e : edges) {
            const size_t x = find(e.ra), y = find(e.rb);
            if (x == y) continue;
            if (viable[x] && viable[y] && e.density < params->saddle) continue;
            parent[y] = x;
            viable[x] = viable[x] || viable[y];
        }
        // the representative of every set: its densest peak
        std::vector<size_t> rep(m);
        for (size_t r = 0; r < m; ++r) rep[r] = m;
        for (size_t r = 0; r < m; ++r) {
            const size_t x = find(r);
            if (rep[x] == m || hop_denser(hop_rho_key(peak_density[r]), rows[r].label, hop_rho_key(peak_density[rep[x]]),
                                          rows[rep[x]].label))
                rep[x] = r;
        }
        // the viable sets in ascending representative label: a set is listed at its representative's row
        std::vector<size_t> out_of(m, m);
        size_t count = 0;
        for (size_t r = 0; r < m; ++r) {
            const size_t x = find(r);
            if (viable[x] && rep[x] == r) out_of[r] = count++;
        }
        for (size_t r = 0; r < m; ++r) {
            const size_t x = find(r);
            if (merged_of_row) merged_of_row[r] = viable[x] ? rows[rep[x]].label : NB_HOP_NONE;
            if (!viable[x] || out_of[rep[x]] >= out_capacity) continue;
            const size_t o = out_of[rep[x]];
            if (out_peak && rep[x] == r) out_peak[o] = peak_density[r];
        }
        if (out_rows) {
            const size_t listed = std::min(count, out_capacity);
            for (size_t o = 0; o < listed; ++o) out_rows[o] = nb_fof_group{};
            for (size_t r = 0; r < m; ++r) {  // the member rows in ascending row order
                const size_t x = find(r);
                if (!viable[x] || out_of[rep[x]] >= out_capacity) continue;
                nb_fof_group &g = out_rows[out_of[rep[x]]];
                g.label = rows[rep[x]].label;
                g.count += rows[r].count;
                g.mass += rows[r].mass;
                for (int a = 0; a < 3; ++a) {
                    g.mx[a] += rows[r].mx[a];
                    g.mv[a] += rows[r].mv[a];
                }
                g.mr2 += rows[r].mr2;
                g.mv2 += rows[r].mv2;
            }
        }
        *out_count = count;
        return NB_OK;
    }
}

// nb_sim_halo_profiles: everything that can be refused without a device (a body index needs n: sim_halo_profiles)
int halo_check_params(const nb_halo_params *p) {
    if (!p || !p->edges) {
        set_error("halo_profiles: null %s", !p ? "params" : "edges");
        return NB_ERR_INVALID;
    }
    if (p->nbins < 1 || p->nbins > NB_HALO_MAX_BINS) {
        set_error("halo_profiles: nbins must be 1..%u (got %u)", NB_HALO_MAX_BINS, p->nbins);
        return NB_ERR_INVALID;
    }
    if (p->flags) {
        set_error("halo_profiles: unknown flag bits 0x%x", p->flags);
        return NB_ERR_INVALID;
    }
    if (p->m > NB_HALO_MAX_CENTERS || p->m * p->nbins > NB_HALO_MAX_ROWS) {
        set_error("halo_profiles: %llu centres of %u bins are more than one call takes (%u centres, %u rows)",
                  (unsigned long long)p->m, p->nbins, NB_HALO_MAX_CENTERS, NB_HALO_MAX_ROWS);
        return NB_ERR_INVALID;
    }
    for (uint32_t k = 0; k <= p->nbins; ++k) {
        const double e = p->edges[k];
        if (!std::isfinite(e) || e < 0.0 || (k > 0 && !(e > p->edges[k - 1]))) {
            set_error("halo_profiles: edges must be finite, >= 0 and strictly ascending (edges[%u] = %g)", k, e);
            return NB_ERR_INVALID;
        }
    }
    if (p->m == 0) return NB_OK;
    if (!p->centers == !p->bodies) {
        set_error("halo_profiles: exactly one of centers and bodies must be given (%s)",
                  p->centers ? "got both" : "got neither");
        return NB_ERR_INVALID;
    }
    for (uint64_t j = 0; j < 3 * p->m; ++j)
        if ((p->centers && !std::isfinite(p->centers[j])) || (p->velocities && !std::isfinite(p->velocities[j]))) {
            set_error("halo_profiles: centre %llu has a non-finite %s", (unsigned long long)(j / 3),
                      p->centers && !std::isfinite(p->centers[j]) ? "position" : "velocity");
            return NB_ERR_INVALID;
        }
    return NB_OK;
}

// nb_map_edges / nb_sim_map: the cell size of `cells` cells in [lo, hi), refused unless the edges
// lo + i * size (i < cells), hi come out strictly ascending
static int map_cell_size(const char *what, double lo, double hi, uint32_t cells, double *size) {
    if (cells < 1 || cells > NB_MAP_MAX_SIDE) {
        set_error("%s: a side must be 1..%u cells (got %u)", what, NB_MAP_MAX_SIDE, cells);
        return NB_ERR_INVALID;
    }
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(hi > lo)) {
        set_error("%s: a window needs finite lo < hi (got %g, %g)", what, lo, hi);
        return NB_ERR_INVALID;
    }
    const double d = (hi - lo) / (double)cells;
    double prev = lo;
    for (uint32_t i = 1; i <= cells; ++i) {
        const double e = i < cells ? lo + (double)i * d : hi;
        if (!(e > prev) || !std::isfinite(e)) {
            set_error("%s: %u cells between %g and %g are not strictly ascending in fp64", what, cells, lo, hi);
            return NB_ERR_INVALID;
        }
        prev = e;
    }
    *size = d;
    return NB_OK;
}

// nb_sim_map: everything that can be refused without a device; the frame and the cell sizes on the way
int map_check_params(const nb_map_params *p, MapPlan *plan) {
    if (!p) {
        set_error("map: null params");
        return NB_ERR_INVALID;
    }
    if (p->width < 1 || p->width > NB_MAP_MAX_SIDE || p->height < 1 || p->height > NB_MAP_MAX_SIDE) {
        set_error("map: a side must be 1..%u cells (got %u x %u)", NB_MAP_MAX_SIDE, p->width, p->height);
        return NB_ERR_INVALID;
    }
    if ((uint64_t)p->width * p->height > NB_MAP_MAX_CELLS) {
        set_error("map: at most %u cells (got %u x %u)", NB_MAP_MAX_CELLS, p->width, p->height);
        return NB_ERR_INVALID;
    }
    if ((p->flags & ~(NB_MAP_CENTER_COM | NB_MAP_VELOCITY)) || p->reserved) {
        set_error("map: unknown flag bits 0x%x or reserved %u != 0", p->flags & ~(NB_MAP_CENTER_COM | NB_MAP_VELOCITY),
                  p->reserved);
        return NB_ERR_INVALID;
    }
    if (!axis_frame(p->axis, plan->n, plan->e1, plan->e2)) {
        set_error("map: needs a non-zero finite axis");
        return NB_ERR_INVALID;
    }
    if (!(p->flags & NB_MAP_CENTER_COM))
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(p->center[k]) || !std::isfinite(p->velocity[k])) {
                set_error("map: center and velocity must be finite");
                return NB_ERR_INVALID;
            }
    if (int rc = map_cell_size("map: x_range", p->x_range[0], p->x_range[1], p->width, &plan->dx)) return rc;
    if (int rc = map_cell_size("map: y_range", p->y_range[0], p->y_range[1], p->height, &plan->dy)) return rc;
    // (either bound may be infinite; a NaN fails the comparison)
    if (!(p->depth_range[1] > p->depth_range[0])) {
        set_error("map: depth_range needs lo < hi without NaN (got %g, %g)", p->depth_range[0], p->depth_range[1]);
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// nb_phase_quantity / nb_phase_quantity_name: the names of NB_PHASE_Q_*, in the enum's order
static const char *const kPhaseNames[NB_PHASE_Q_COUNT] = {"a",   "b",     "h",   "R",     "r",   "ua", "ub",    "w",    "u_R",
                                                          "u_phi", "u_r", "u_t", "speed", "j_z", "j",  "e_kin", "mass", "value"};

int phase_quantity(const char *name, uint32_t *id) {
    if (!name || !id) {
        set_error("phase_quantity: null argument");
        return NB_ERR_INVALID;
    }
    for (uint32_t q = 0; q < NB_PHASE_Q_COUNT; ++q)
        if (std::string(name) == kPhaseNames[q]) {
            *id = q;
            return NB_OK;
        }
    set_error("phase_quantity: no quantity is called '%s'", name);
    return NB_ERR_INVALID;
}

const char *phase_quantity_name(uint32_t id) { return id < NB_PHASE_Q_COUNT ? kPhaseNames[id] : nullptr; }

// nb_phase_map_sim: the edges of one side, strictly ascending, the interior ones finite; the first may be -inf
// and the last +inf
static int phase_check_edges(const char *what, const double *e, uint32_t cells) {
    for (uint32_t i = 0; i <= cells; ++i) {
        const bool outer_ok = (i == 0 && e[i] == -INFINITY) || (i == cells && e[i] == INFINITY);
        if (!(std::isfinite(e[i]) || outer_ok) || (i > 0 && !(e[i] > e[i - 1]))) {
            set_error("phase_map: %s must be strictly ascending with finite interior edges (%s[%u] = %g)", what, what, i,
                      e[i]);
            return NB_ERR_INVALID;
        }
    }
    return NB_OK;
}

// nb_phase_map_sim: everything that can be refused without a device; the frame on the way
int phase_check_params(const nb_phase_params *p, PhasePlan *plan) {
    if (!p || !p->x_edges || !p->y_edges) {
        set_error("phase_map: null %s", !p ? "params" : !p->x_edges ? "x_edges" : "y_edges");
        return NB_ERR_INVALID;
    }
    if (p->width < 1 || p->width > NB_MAP_MAX_SIDE || p->height < 1 || p->height > NB_MAP_MAX_SIDE) {
        set_error("phase_map: a side must be 1..%u cells (got %u x %u)", NB_MAP_MAX_SIDE, p->width, p->height);
        return NB_ERR_INVALID;
    }
    if ((uint64_t)p->width * p->height > NB_MAP_MAX_CELLS) {
        set_error("phase_map: at most %u cells (got %u x %u)", NB_MAP_MAX_CELLS, p->width, p->height);
        return NB_ERR_INVALID;
    }
    if ((p->flags & ~(NB_PHASE_CENTER_COM | NB_PHASE_WEIGHT)) || p->reserved || p->reserved2) {
        set_error("phase_map: unknown flag bits 0x%x or a reserved field != 0",
                  p->flags & ~(NB_PHASE_CENTER_COM | NB_PHASE_WEIGHT));
        return NB_ERR_INVALID;
    }
    if (p->x >= NB_PHASE_Q_COUNT || p->y >= NB_PHASE_Q_COUNT || p->q >= NB_PHASE_Q_COUNT) {
        set_error("phase_map: unknown quantity id (x %u, y %u, q %u; ids end at %u)", p->x, p->y, p->q,
                  NB_PHASE_Q_COUNT - 1);
        return NB_ERR_INVALID;
    }
    if (!axis_frame(p->axis, plan->n, plan->e1, plan->e2)) {
        set_error("phase_map: needs a non-zero finite axis");
        return NB_ERR_INVALID;
    }
    if (!(p->flags & NB_PHASE_CENTER_COM))
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(p->center[k]) || !std::isfinite(p->velocity[k])) {
                set_error("phase_map: center and velocity must be finite");
                return NB_ERR_INVALID;
            }
    if (int rc = phase_check_edges("x_edges", p->x_edges, p->width)) return rc;
    if (int rc = phase_check_edges("y_edges", p->y_edges, p->height)) return rc;
    plan->uses_values = p->x == NB_PHASE_Q_VALUE || p->y == NB_PHASE_Q_VALUE ||
                        ((p->flags & NB_PHASE_WEIGHT) && p->q == NB_PHASE_Q_VALUE);
    if (plan->uses_values && !p->values) {
        set_error("phase_map: the quantity `value` needs params->values");
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// ... and what needs the simulator's step number: `values` is in the order of the bodies now
int phase_check_args(const SimBase &s, const nb_phase_params *p, const PhasePlan &plan) {
    if (plan.uses_values && p->step_num != NB_PHASE_ANY_STEP && p->step_num != s.step_num) {
        set_error("phase_map: the values were made at step %llu, the simulator is at step %llu",
                  (unsigned long long)p->step_num, (unsigned long long)s.step_num);
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// nb_smooth_centres / nb_sim_smooth_map: the `cells` pixel centres of a window, from the edges of nb_map_edges
static void smooth_centres(double lo, double hi, uint32_t cells, double size, double *out) {
    double prev = lo;  // xe[i]
    for (uint32_t i = 0; i < cells; ++i) {
        const double next = i + 1 < cells ? lo + (double)(i + 1) * size : hi;
        out[i] = 0.5 * (prev + next);
        prev = next;
    }
}

// nb_sim_smooth_map: everything that can be refused without a device, in the words of the pass; the frame, the
// pixel sizes and the pixel centres on the way.  The fields the two share are checked by map_check_params.
int smooth_check_params(const nb_smooth_params *p, SmoothPlan *plan) {
    if (!p) {
        set_error("smooth_map: null params");
        return NB_ERR_INVALID;
    }
    if ((p->flags & ~(NB_SMOOTH_CENTER_COM | NB_SMOOTH_VELOCITY)) || p->reserved) {
        set_error("smooth_map: unknown flag bits 0x%x or reserved %u != 0",
                  p->flags & ~(NB_SMOOTH_CENTER_COM | NB_SMOOTH_VELOCITY), p->reserved);
        return NB_ERR_INVALID;
    }
    if (!std::isfinite(p->s_min) || !std::isfinite(p->s_max) || !(p->s_min > 0.0) || !(p->s_max >= p->s_min)) {
        set_error("smooth_map: needs finite 0 < s_min <= s_max (got %g, %g)", p->s_min, p->s_max);
        return NB_ERR_INVALID;
    }
    static_assert(NB_SMOOTH_CENTER_COM == NB_MAP_CENTER_COM && NB_SMOOTH_VELOCITY == NB_MAP_VELOCITY, "shared flag bits");
    nb_map_params m{};
    m.width = p->width;
    m.height = p->height;
    m.flags = p->flags;
    for (int k = 0; k < 3; ++k) {
        m.center[k] = p->center[k];
        m.velocity[k] = p->velocity[k];
        m.axis[k] = p->axis[k];
    }
    for (int k = 0; k < 2; ++k) {
        m.x_range[k] = p->x_range[k];
        m.y_range[k] = p->y_range[k];
        m.depth_range[k] = p->depth_range[k];
    }
    if (int rc = map_check_params(&m, &plan->frame)) {
        const std::string why = nb_last_error();  // "map: ..."
        set_error("smooth_%s", why.c_str());
        return rc;
    }
    plan->xc.resize(p->width);
    plan->yc.resize(p->height);
    smooth_centres(p->x_range[0], p->x_range[1], p->width, plan->frame.dx, plan->xc.data());
    smooth_centres(p->y_range[0], p->y_range[1], p->height, plan->frame.dy, plan->yc.data());
    return NB_OK;
}

// ---- the host-only entry points of include/nbody.h behind the ABI boundary (nb_X is X here) ----
int radial_lagrangian(const nb_radial_profile *p, const nb_radial_bin *bins, const double *edges,
                      const double *fractions, uint32_t k, double *radii) {
    if (!p || !bins || !edges || (k && (!fractions || !radii))) {
        set_error("radial_lagrangian: null argument");
        return NB_ERR_INVALID;
    }
    if (p->nbins < 1 || p->nbins > NB_RADIAL_MAX_BINS) {
        set_error("radial_lagrangian: profile with %u bins", p->nbins);
        return NB_ERR_INVALID;
    }
    for (uint32_t i = 0; i < k; ++i) {
        const double f = fractions[i], target = f * p->mass;
        radii[i] = std::nan("");
        if (!(f > 0.0 && f < 1.0) || !(target >= p->inside_mass)) continue;  // ... or the crossing lies in `inside`
        double cum = p->inside_mass;
        for (uint32_t b = 0; b < p->nbins; ++b) {
            const double m = bins[b].mass, next = cum + m;
            if (target <= next) {  // linear in r inside the bin that crosses
                radii[i] = m > 0.0 ? edges[b] + (target - cum) / m * (edges[b + 1] - edges[b]) : edges[b];
                break;
            }
            cum = next;
        }
    }
    return NB_OK;
}

int field_rings(const double center[3], const double axis[3], const double *radii, uint32_t k, uint32_t n_phi,
                float *points) {
    double n[3], e1[3], e2[3];
    if (int rc = ring_basis("field_rings", center, axis, radii, k, n_phi, n, e1, e2)) return rc;
    if (k && !points) {
        set_error("field_rings: null points");
        return NB_ERR_INVALID;
    }
    const double two_pi = 6.283185307179586476925286766559;
    for (uint32_t i = 0; i < k; ++i)
        for (uint32_t q = 0; q < n_phi; ++q) {
            const double phi = two_pi * (double)q / (double)n_phi, c = std::cos(phi), s = std::sin(phi);
            float *p = points + 3 * ((size_t)i * n_phi + q);
            for (int a = 0; a < 3; ++a) p[a] = (float)(center[a] + radii[i] * (c * e1[a] + s * e2[a]));
        }
    return NB_OK;
}

int field_ring_means(const double center[3], const double axis[3], const double *radii, uint32_t k,
                     uint32_t n_phi, const float *points, const nb_field_sample *samples, nb_field_ring *out) {
    double n[3], e1[3], e2[3];
    if (int rc = ring_basis("field_ring_means", center, axis, radii, k, n_phi, n, e1, e2)) return rc;
    if (k && (!points || !samples || !out)) {
        set_error("field_ring_means: null %s", !points ? "points" : !samples ? "samples" : "out");
        return NB_ERR_INVALID;
    }
    for (uint32_t i = 0; i < k; ++i) {
        double a_r = 0.0, a_n = 0.0, pot = 0.0;
        for (uint32_t q = 0; q < n_phi; ++q) {
            const size_t j = (size_t)i * n_phi + q;
            const nb_field_sample &f = samples[j];
            double d[3], h = 0.0;  // the fp32 point actually used, from the centre; its height along n
            for (int a = 0; a < 3; ++a) {
                d[a] = (double)points[3 * j + a] - center[a];
                h += d[a] * n[a];
            }
            double len = 0.0, dot = 0.0;
            for (int a = 0; a < 3; ++a) {
                d[a] -= h * n[a];
                len += d[a] * d[a];
                dot += f.acc[a] * d[a];
            }
            len = std::sqrt(len);
            if (len > 0.0) a_r += dot / len;
            a_n += f.acc[0] * n[0] + f.acc[1] * n[1] + f.acc[2] * n[2];
            pot += f.potential;
        }
        nb_field_ring r{};
        r.a_R = a_r / (double)n_phi;
        r.a_n = a_n / (double)n_phi;
        r.potential = pot / (double)n_phi;
        r.v_c = std::sqrt(std::fmax(0.0, -radii[i] * r.a_R));
        out[i] = r;
    }
    return NB_OK;
}

int tidal_ring_means(const double center[3], const double axis[3], const double *radii, uint32_t k, uint32_t n_phi,
                     const float *points, const nb_tidal_sample *samples, const nb_field_ring *rings,
                     nb_tidal_ring *out) {
    double n[3], e1[3], e2[3];
    if (int rc = ring_basis("tidal_ring_means", center, axis, radii, k, n_phi, n, e1, e2)) return rc;
    if (k && (!points || !samples || !rings || !out)) {
        set_error("tidal_ring_means: null %s", !points ? "points" : !samples ? "samples" : !rings ? "rings" : "out");
        return NB_ERR_INVALID;
    }
    for (uint32_t i = 0; i < k; ++i) {
        double t_rr = 0.0, t_pp = 0.0, t_nn = 0.0, t_rn = 0.0;
        for (uint32_t q = 0; q < n_phi; ++q) {
            const size_t j = (size_t)i * n_phi + q;
            const double *s = samples[j].tensor;  // xx, yy, zz, xy, xz, yz
            const double t[3][3] = {{s[0], s[3], s[4]}, {s[3], s[1], s[5]}, {s[4], s[5], s[2]}};
            double d[3], h = 0.0;  // the fp32 point actually used, from the centre; its height along n
            for (int a = 0; a < 3; ++a) {
                d[a] = (double)points[3 * j + a] - center[a];
                h += d[a] * n[a];
            }
            double len = 0.0;
            for (int a = 0; a < 3; ++a) {
                d[a] -= h * n[a];
                len += d[a] * d[a];
            }
            len = std::sqrt(len);
            double tn[3];  // T n
            for (int a = 0; a < 3; ++a) tn[a] = t[a][0] * n[0] + t[a][1] * n[1] + t[a][2] * n[2];
            t_nn += n[0] * tn[0] + n[1] * tn[1] + n[2] * tn[2];
            if (!(len > 0.0)) continue;  // on the axis: no rhat
            double rh[3], ph[3], tr[3], tp[3];
            for (int a = 0; a < 3; ++a) rh[a] = d[a] / len;
            ph[0] = n[1] * rh[2] - n[2] * rh[1];  // phihat = n x rhat
            ph[1] = n[2] * rh[0] - n[0] * rh[2];
            ph[2] = n[0] * rh[1] - n[1] * rh[0];
            for (int a = 0; a < 3; ++a) {
                tr[a] = t[a][0] * rh[0] + t[a][1] * rh[1] + t[a][2] * rh[2];
                tp[a] = t[a][0] * ph[0] + t[a][1] * ph[1] + t[a][2] * ph[2];
            }
            t_rr += rh[0] * tr[0] + rh[1] * tr[1] + rh[2] * tr[2];
            t_pp += ph[0] * tp[0] + ph[1] * tp[1] + ph[2] * tp[2];
            t_rn += rh[0] * tn[0] + rh[1] * tn[1] + rh[2] * tn[2];
        }
        nb_tidal_ring r{};
        r.t_RR = t_rr / (double)n_phi;
        r.t_pp = t_pp / (double)n_phi;
        r.t_nn = t_nn / (double)n_phi;
        r.t_Rn = t_rn / (double)n_phi;
        r.omega2 = radii[i] > 0.0 ? -rings[i].a_R / radii[i] : std::nan("");
        r.kappa2 = -r.t_RR + 3.0 * r.omega2;
        r.nu2 = -r.t_nn;
        out[i] = r;
    }
    return NB_OK;
}

int halo_enclosed(const nb_halo_head *head, const nb_radial_bin *bins, uint32_t nbins, double *out) {
    if (!head || !bins || !out) {
        set_error("halo_enclosed: null argument");
        return NB_ERR_INVALID;
    }
    if (nbins < 1 || nbins > NB_HALO_MAX_BINS) {
        set_error("halo_enclosed: nbins must be 1..%u (got %u)", NB_HALO_MAX_BINS, nbins);
        return NB_ERR_INVALID;
    }
    out[0] = head->inside_mass;
    for (uint32_t k = 0; k < nbins; ++k) out[k + 1] = out[k] + bins[k].mass;
    return NB_OK;
}

int halo_overdensity(const nb_halo_head *head, const nb_radial_bin *bins, const double *edges, uint32_t nbins,
                     double rho, double *r, double *mass) {
    if (!edges || !r || !mass) {
        set_error("halo_overdensity: null argument");
        return NB_ERR_INVALID;
    }
    double enclosed[NB_HALO_MAX_BINS + 1];
    if (int rc = halo_enclosed(head, bins, nbins, enclosed)) return rc;
    if (!std::isfinite(rho) || !(rho > 0.0)) {
        set_error("halo_overdensity: rho must be finite and > 0 (got %g)", rho);
        return NB_ERR_INVALID;
    }
    *r = *mass = std::nan("");
    for (uint32_t k = 1; k <= nbins; ++k) {
        const double e0 = edges[k - 1], e1 = edges[k];
        if (!(e0 > 0.0)) continue;
        const double rho0 = enclosed[k - 1] / (NB_KNN_SPHERE * ((e0 * e0) * e0));
        const double rho1 = enclosed[k] / (NB_KNN_SPHERE * ((e1 * e1) * e1));
        if (rho0 >= rho && rho > rho1) {
            const double t = (std::log(rho0) - std::log(rho)) / (std::log(rho0) - std::log(rho1));
            const double x = std::exp(std::log(e0) + t * (std::log(e1) - std::log(e0)));
            *r = x;
            *mass = rho * NB_KNN_SPHERE * ((x * x) * x);
            break;
        }
    }
    return NB_OK;
}

int smooth_centres(double lo, double hi, uint32_t cells, double *out) {
    if (!out) {
        set_error("smooth_centres: out is null");
        return NB_ERR_INVALID;
    }
    double d = 0.0;
    if (int rc = map_cell_size("smooth_centres", lo, hi, cells, &d)) return rc;
    smooth_centres(lo, hi, cells, d, out);
    return NB_OK;
}

int map_frame(const double axis[3], double n_hat[3], double e1[3], double e2[3]) {
    if (!axis || !n_hat || !e1 || !e2) {
        set_error("map_frame: null argument");
        return NB_ERR_INVALID;
    }
    double n[3], f1[3], f2[3];
    if (!axis_frame(axis, n, f1, f2)) {
        set_error("map_frame: needs a non-zero finite axis");
        return NB_ERR_INVALID;
    }
    for (int a = 0; a < 3; ++a) {
        n_hat[a] = n[a];
        e1[a] = f1[a];
        e2[a] = f2[a];
    }
    return NB_OK;
}

int map_edges(double lo, double hi, uint32_t cells, double *edges) {
    if (!edges) {
        set_error("map_edges: edges is null");
        return NB_ERR_INVALID;
    }
    double d = 0.0;
    if (int rc = map_cell_size("map_edges", lo, hi, cells, &d)) return rc;
    for (uint32_t i = 0; i < cells; ++i) edges[i] = lo + (double)i * d;
    edges[cells] = hi;
    return NB_OK;
}

// nb_mst_sim: everything that can be refused without a device
int mst_check_params(const nb_mst_params *p) {
    if (!p) {
        set_error("mst: null params");
        return NB_ERR_INVALID;
    }
    if (p->flags || p->reserved32 || p->reserved) {
        set_error("mst: unknown flag bits 0x%x or a reserved field != 0", p->flags);
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

namespace {

// what nb_mst_cut and nb_mst_linkage refuse about an edge list
int mst_check_edges(const char *what, size_t n, size_t edges, const uint32_t *edge_lo, const uint32_t *edge_hi) {
    if (n > 0xffffffffull) {
        set_error("%s: %zu bodies are more than a 32-bit index names", what, n);
        return NB_ERR_INVALID;
    }
    if (edges >= std::max<size_t>(n, 1)) {
        set_error("%s: %zu edges are not a tree's on %zu bodies", what, edges, n);
        return NB_ERR_INVALID;
    }
    if (edges && (!edge_lo || !edge_hi)) {
        set_error("%s: null edge_lo or edge_hi for %zu edges", what, edges);
        return NB_ERR_INVALID;
    }
    for (size_t e = 0; e < edges; ++e)
        if (!(edge_lo[e] < edge_hi[e]) || edge_hi[e] >= n) {
            set_error("%s: edge %zu (%u, %u) is not lo < hi < n = %zu", what, e, edge_lo[e], edge_hi[e], n);
            return NB_ERR_INVALID;
        }
    return NB_OK;
}

// the forest of nb_fof.hpp on the host: the larger root under the smaller, so a root is its tree's smallest index
uint32_t mst_root(std::vector<uint32_t> &parent, uint32_t x) {
    while (parent[x] != x) {
        parent[x] = parent[parent[x]];
        x = parent[x];
    }
    return x;
}

}  // namespace

int mst_cut(size_t n, size_t edges, const uint32_t *edge_lo, const uint32_t *edge_hi, const double *d2,
            const uint32_t *degree, double link, uint32_t *labels, size_t *components) {
    if (int rc = mst_check_edges("mst_cut", n, edges, edge_lo, edge_hi)) return rc;
    if ((edges && !d2) || (n && !labels)) {
        set_error("mst_cut: null d2 or labels");
        return NB_ERR_INVALID;
    }
    if (!std::isfinite(link) || !(link > 0.0)) {
        set_error("mst_cut: link must be finite and > 0 (got %g)", link);
        return NB_ERR_INVALID;
    }
    const double b2 = link * link;  // what the rule compares with, formed once (nb_sim_fof)
    if (!(b2 > 0.0) || !std::isfinite(b2)) {
        set_error("mst_cut: link %g squared is not a positive finite double", link);
        return NB_ERR_INVALID;
    }
    std::vector<uint32_t> parent(n);
    for (size_t i = 0; i < n; ++i) parent[i] = (uint32_t)i;
    for (size_t e = 0; e < edges; ++e) {
        if (!(d2[e] <= b2)) continue;
        const uint32_t a = mst_root(parent, edge_lo[e]), b = mst_root(parent, edge_hi[e]);
        if (a != b) parent[std::max(a, b)] = std::min(a, b);
    }
    size_t count = 0;
    for (size_t i = 0; i < n; ++i) {
        if (degree && degree[i] == NB_MST_NONE) {
            labels[i] = NB_FOF_NONE;
            continue;
        }
        labels[i] = mst_root(parent, (uint32_t)i);
        count += labels[i] == i;
    }
    if (components) *components = count;
    return NB_OK;
}

int mst_linkage(size_t n, size_t edges, const uint32_t *edge_lo, const uint32_t *edge_hi, uint32_t *label_a,
                uint32_t *label_b, uint32_t *count_a, uint32_t *count_b) {
    if (int rc = mst_check_edges("mst_linkage", n, edges, edge_lo, edge_hi)) return rc;
    std::vector<uint32_t> parent(n), size(n, 1u);
    for (size_t i = 0; i < n; ++i) parent[i] = (uint32_t)i;
    for (size_t e = 0; e < edges; ++e)
        if (mst_root(parent, edge_lo[e]) == mst_root(parent, edge_hi[e])) {
            set_error("mst_linkage: edge %zu (%u, %u) closes a cycle", e, edge_lo[e], edge_hi[e]);
            return NB_ERR_INVALID;
        } else {
            const uint32_t ra = mst_root(parent, edge_lo[e]), rb = mst_root(parent, edge_hi[e]);
            parent[std::max(ra, rb)] = std::min(ra, rb);
        }
    // (checked before anything is written: the outputs are written only by a call that succeeds)
    for (size_t i = 0; i < n; ++i) parent[i] = (uint32_t)i;
    for (size_t e = 0; e < edges; ++e) {
        const uint32_t ra = mst_root(parent, edge_lo[e]), rb = mst_root(parent, edge_hi[e]);
        const uint32_t a = std::min(ra, rb), b = std::max(ra, rb);
        if (label_a) label_a[e] = a;
        if (label_b) label_b[e] = b;
        if (count_a) count_a[e] = size[a];
        if (count_b) count_b[e] = size[b];
        parent[b] = a;
        size[a] += size[b];
    }
    return NB_OK;
}

}  // namespace nb
