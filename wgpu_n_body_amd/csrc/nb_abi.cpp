// nb_abi.cpp -- the C ABI of include/nbody.h: the extern "C" surface over the simulator objects
// (nb_simbase.cpp, nb_tree.hip), the analysis passes stated once for both handle types, and the
// OfflineHeadless-shaped runner.  What a pass refuses without a device, and the host-only entry
// points' bodies, are in nb_passes.cpp.
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "nb_common.hpp"
#include "nb_group.hpp"
#include "nb_sim.hpp"

namespace nb {

static thread_local std::string g_last_error;

void set_error(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

static int make_sim(nb_sim **out, const nb_sim_params *sp, const nb_add_params *ap,
                    const nb_placement *pl, const nb_particle *particles, size_t count) {
    if (!out || !sp) {
        set_error("null argument");
        return NB_ERR_INVALID;
    }
    *out = nullptr;
    std::unique_ptr<SimBase> impl;
    if (int rc = make_sim_impl(impl, sp, ap, pl, particles, count)) return rc;
    nb_sim *s = new (std::nothrow) nb_sim();
    if (!s) {
        set_error("out of host memory");
        return NB_ERR_ALLOC;
    }
    s->impl = std::move(impl);
    *out = s;
    return NB_OK;
}

}  // namespace nb

// ==========================================================================================
// extern "C"
// ==========================================================================================
using namespace nb;

#define NB_GUARD(body)                                            \
    try {                                                         \
        body                                                      \
    } catch (const std::bad_alloc &) {                            \
        set_error("out of host memory");                          \
        return NB_ERR_ALLOC;                                      \
    } catch (...) {                                               \
        set_error("unexpected C++ exception at the ABI boundary"); \
        return NB_ERR_INVALID;                                    \
    }

// ---- runner: OfflineHeadless<T>, src/runners/offline_headless.rs ---------------------------
struct nb_runner {
    nb_sim *sim = nullptr;                  // one device
    std::unique_ptr<DeviceGroup> group;      // several devices of this process (nb_runner_create_multi)
    bool profiling = false;                  // nb_runner_set_profiling, one device: events around step_n
    float kernel_ms = 0.f;
};

static int check_runner(const nb_runner *runner) {  // a runner that owns a simulator or a group
    if (!runner || (!runner->sim && !runner->group)) {
        set_error("null runner");
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// ---- the analysis passes, once for both handle types ----------------------------------------
// The simulator object behind a handle.  A runner's is its own simulator's; the passes read the whole state of
// one simulator, so a several-GPU runner refuses `pass`.
static int sim_behind(nb_sim *sim, const char *, SimBase **out) {
    if (!sim || !sim->impl) {
        set_error("null simulator");
        return NB_ERR_INVALID;
    }
    *out = sim->impl.get();
    return NB_OK;
}
static int sim_behind(nb_runner *runner, const char *pass, SimBase **out) {
    if (int rc = check_runner(runner)) return rc;
    if (runner->group) {
        set_error("%s: not available on a several-GPU runner (nb_runner_create_multi*)", pass);
        return NB_ERR_UNSUPPORTED;
    }
    return sim_behind(runner->sim, pass, out);
}

// A pass is: the refusals that need no simulator, then on_sim -- the handle, for a runner the several-GPU
// refusal, and `call` (the checks that read the simulator, then sim_X) on the object behind it.
template <class H, class Call>
static int on_sim(H *handle, const char *pass, Call call) {
    SimBase *sim = nullptr;
    if (int rc = sim_behind(handle, pass, &sim)) return rc;
    NB_GUARD({ return call(*sim); })
}

template <class H>
static int pass_diagnostics(H *h, uint32_t flags, nb_diagnostics *out) {
    if (!out) {
        set_error("diagnostics: out is null");
        return NB_ERR_INVALID;
    }
    if (flags & ~(NB_DIAG_MOMENTS | NB_DIAG_POTENTIAL)) {
        set_error("diagnostics: unknown flag bits 0x%x", flags & ~(NB_DIAG_MOMENTS | NB_DIAG_POTENTIAL));
        return NB_ERR_INVALID;
    }
    return on_sim(h, "diagnostics", [&](SimBase &s) { return sim_diagnostics(s, flags, out); });
}

template <class H>
static int pass_radial_profile(H *h, const nb_radial_params *params, nb_radial_profile *out, nb_radial_bin *bins) {
    if (int rc = radial_check_params(params, out, bins)) return rc;
    return on_sim(h, "radial_profile", [&](SimBase &s) { return sim_radial_profile(s, *params, out, bins); });
}

template <class H>
static int pass_field(H *h, const float *points, size_t m, uint32_t flags, nb_field_sample *out,
                      nb_field_stats *stats) {
    if (int rc = field_check_args(points, m, flags, out)) return rc;
    return on_sim(h, "field", [&](SimBase &s) { return sim_field(s, points, m, flags, out, stats); });
}

template <class H>
static int pass_tidal(H *h, const float *points, size_t m, nb_tidal_sample *out, nb_tidal_stats *stats) {
    if (int rc = tidal_check_args(points, m, out)) return rc;
    return on_sim(h, "tidal", [&](SimBase &s) { return sim_tidal(s, points, m, out, stats); });
}

template <class H>
static int pass_orbits(H *h, const nb_orbit_params *params, const double *pos, const double *vel, size_t m,
                       nb_orbit_sample *tracks, uint32_t *coincident, nb_orbit_stats *stats) {
    OrbitPlan plan{};
    if (int rc = orbits_check_args(params, pos, vel, m, tracks, &plan)) return rc;
    return on_sim(h, "orbits", [&](SimBase &s) {
        if (int rc = orbits_check_e(s, params)) return rc;
        return sim_orbits(s, *params, plan, pos, vel, m, tracks, coincident, stats);
    });
}

template <class H>
static int pass_orbit_sections(H *h, const nb_orbit_params *params, const nb_orbit_section_params *section,
                               const double *pos, const double *vel, size_t m, nb_orbit_sample *tracks,
                               uint32_t *coincident, nb_orbit_crossing *crossings, uint32_t *counts,
                               nb_orbit_summary *summaries, nb_orbit_section_stats *stats) {
    OrbitPlan plan{};
    if (int rc = orbit_sections_check_args(params, section, pos, vel, m, tracks, crossings, &plan)) return rc;
    return on_sim(h, "orbit_sections", [&](SimBase &s) {
        if (int rc = orbits_check_e(s, params)) return rc;
        return sim_orbit_sections(s, *params, *section, plan, pos, vel, m, tracks, coincident, crossings, counts,
                                  summaries, stats);
    });
}

template <class H>
static int pass_orbit_stability(H *h, const nb_orbit_params *params, const nb_orbit_stability_params *stability,
                                const double *pos, const double *vel, size_t m, const nb_orbit_deviation *dev0,
                                nb_orbit_sample *tracks, uint32_t *coincident, nb_orbit_deviation *devs,
                                nb_orbit_growth *growth, nb_orbit_stability_stats *stats) {
    OrbitPlan plan{};
    if (int rc = orbit_stability_check_args(params, stability, pos, vel, m, dev0, tracks, devs, &plan)) return rc;
    return on_sim(h, "orbit_stability", [&](SimBase &s) {
        return sim_orbit_stability(s, *params, *stability, plan, pos, vel, m, dev0, tracks, coincident, devs, growth,
                                   stats);
    });
}

template <class H>
static int pass_map(H *h, const nb_map_params *params, uint32_t *counts, double *planes, nb_map_stats *stats) {
    MapPlan plan{};
    if (int rc = map_check_params(params, &plan)) return rc;
    return on_sim(h, "map", [&](SimBase &s) { return sim_map(s, *params, plan, counts, planes, stats); });
}

template <class H>
static int pass_fof(H *h, const nb_fof_params *params, uint32_t *labels, uint32_t *group_of, nb_fof_group *groups,
                    size_t group_capacity, nb_fof_stats *stats) {
    if (int rc = fof_check_params(params)) return rc;
    return on_sim(h, "fof", [&](SimBase &s) {
        return sim_fof(s, *params, labels, group_of, groups, group_capacity, stats);
    });
}

template <class H>
static int pass_fof6(H *h, const nb_fof6_params *params, uint32_t *labels, uint32_t *group_of, nb_fof_group *groups,
                     size_t group_capacity, nb_fof_stats *stats) {
    if (int rc = fof6_check_params(params)) return rc;
    return on_sim(h, "fof6", [&](SimBase &s) {
        return sim_fof6(s, *params, labels, group_of, groups, group_capacity, stats);
    });
}

template <class H>
static int pass_bound(H *h, const nb_bound_params *params, uint32_t *group_of, uint32_t *bound_of, double *energy,
                      nb_bound_group *groups, size_t group_capacity, nb_bound_stats *stats) {
    if (int rc = bound_check_params(params)) return rc;
    return on_sim(h, "bound", [&](SimBase &s) {
        if (int rc = bound_check_e(s)) return rc;
        return sim_bound(s, *params, group_of, bound_of, energy, groups, group_capacity, stats);
    });
}

template <class H>
static int pass_knn(H *h, const nb_knn_params *params, double *r2, uint32_t *kth, double *mass_in, double *density,
                    nb_knn_stats *stats) {
    if (int rc = knn_check_params(params)) return rc;
    return on_sim(h, "knn", [&](SimBase &s) { return sim_knn(s, *params, r2, kth, mass_in, density, stats); });
}

template <class H>
static int pass_mst(H *h, const nb_mst_params *params, uint32_t *edge_lo, uint32_t *edge_hi, double *d2,
                    uint32_t *degree, nb_mst_stats *stats) {
    if (int rc = mst_check_params(params)) return rc;
    return on_sim(h, "mst", [&](SimBase &s) { return sim_mst(s, *params, edge_lo, edge_hi, d2, degree, stats); });
}

template <class H>
static int pass_local_kinematics(H *h, const nb_kin_params *params, double *moments, double *grads, double *r2,
                                 uint32_t *kth, double *mass_in, double *density, nb_kin_stats *stats) {
    if (int rc = kin_check_params(params)) return rc;
    return on_sim(h, "local_kinematics", [&](SimBase &s) {
        return sim_local_kinematics(s, *params, moments, grads, r2, kth, mass_in, density, stats);
    });
}

template <class H>
static int pass_hop(H *h, const nb_hop_params *params, uint32_t *labels, uint32_t *group_of, double *density,
                    nb_fof_group *groups, double *peak_density, size_t group_capacity, nb_hop_boundary *boundaries,
                    size_t boundary_capacity, nb_hop_stats *stats) {
    if (int rc = hop_check_params(params)) return rc;
    return on_sim(h, "hop", [&](SimBase &s) {
        return sim_hop(s, *params, labels, group_of, density, groups, peak_density, group_capacity, boundaries,
                       boundary_capacity, stats);
    });
}

template <class H>
static int pass_halo_profiles(H *h, const nb_halo_params *params, nb_halo_head *heads, nb_radial_bin *bins,
                              nb_halo_stats *stats) {
    if (int rc = halo_check_params(params)) return rc;
    return on_sim(h, "halo_profiles", [&](SimBase &s) { return sim_halo_profiles(s, *params, heads, bins, stats); });
}

template <class H>
static int pass_group_shapes(H *h, const nb_shape_params *params, const uint32_t *group_of, size_t m,
                             const double *centers, const double *velocities, const double *radius,
                             nb_shape_group *rows_out, uint32_t *selected_of, nb_shape_stats *stats) {
    if (int rc = shape_check_params(params)) return rc;
    return on_sim(h, "group_shapes", [&](SimBase &s) {
        if (int rc = shape_check_args(s, params, group_of, m, centers, velocities, radius)) return rc;
        return sim_group_shapes(s, *params, group_of, m, centers, velocities, radius, rows_out, selected_of, stats);
    });
}

template <class H>
static int pass_group_radii(H *h, const nb_radii_params *params, const uint32_t *group_of, size_t m,
                            const double *centers, nb_radii_group *rows_out, uint32_t *rank_of, double *enclosed_of,
                            nb_radii_stats *stats) {
    if (int rc = radii_check_params(params)) return rc;
    return on_sim(h, "group_radii", [&](SimBase &s) {
        if (int rc = radii_check_args(s, params, group_of, m, centers)) return rc;
        return sim_group_radii(s, *params, group_of, m, centers, rows_out, rank_of, enclosed_of, stats);
    });
}

template <class H>
static int pass_disc_modes(H *h, const nb_modes_params *params, nb_modes_head *out, nb_modes_bin *bins,
                           double *modes) {
    if (int rc = modes_check_params(params, out, bins, modes)) return rc;
    return on_sim(h, "disc_modes", [&](SimBase &s) { return sim_disc_modes(s, *params, out, bins, modes); });
}

template <class H>
static int pass_shell_modes(H *h, const nb_shell_params *params, nb_shell_head *out, nb_shell_bin *bins,
                            double *coef) {
    if (int rc = shell_check_params(params, out, bins, coef)) return rc;
    return on_sim(h, "shell_modes", [&](SimBase &s) { return sim_shell_modes(s, *params, out, bins, coef); });
}

template <class H>
static int pass_phase_map(H *h, const nb_phase_params *params, uint32_t *counts, double *planes,
                          nb_phase_stats *stats) {
    PhasePlan plan{};
    if (int rc = phase_check_params(params, &plan)) return rc;
    return on_sim(h, "phase_map", [&](SimBase &s) {
        if (int rc = phase_check_args(s, params, plan)) return rc;
        return sim_phase_map(s, *params, plan, counts, planes, stats);
    });
}

template <class H>
static int pass_smooth_map(H *h, const nb_smooth_params *params, const double *s, uint32_t *counts, double *planes,
                           nb_smooth_stats *stats) {
    NB_GUARD({
        SmoothPlan plan{};
        if (int rc = smooth_check_params(params, &plan)) return rc;
        return on_sim(h, "smooth_map", [&](SimBase &sim) {
            if (!s && sim.n > 0) {
                set_error("smooth_map: null s for %u bodies", sim.n);
                return (int)NB_ERR_INVALID;
            }
            return sim_smooth_map(sim, *params, plan, s, counts, planes, stats);
        });
    })
}

template <class H>
static int pass_render(H *h, const nb_render_params *params, uint8_t *rgba, uint32_t *counts,
                       nb_render_stats *stats) {
    if (int rc = render_check_params(params)) return rc;
    return on_sim(h, "render", [&](SimBase &s) { return sim_render(s, *params, rgba, counts, stats); });
}

// ---- nb_sim_set_tuning: the keys of the analysis passes, whichever simulator holds the state ----
struct TuningKey {
    const char *key;
    int SimBase::*member;
    const char *allowed;  // the wording of the allowed values ...
    bool (*ok)(int);      // ... and the test for them
};
static bool multiple_in(int v, int step, int hi) { return v >= step && v <= hi && v % step == 0; }
static const TuningKey kTuningKeys[] = {
    {"field_launch_pairs_log2", &SimBase::field_pairs_log2, "16..40", [](int v) { return v >= 16 && v <= 40; }},
    {"map_segment_len", &SimBase::map_segment_len, "a multiple of 256 in 256..65536",
     [](int v) { return multiple_in(v, 256, 65536); }},
    {"phase_segment_len", &SimBase::phase_segment_len, "a multiple of 256 in 256..65536",
     [](int v) { return multiple_in(v, 256, 65536); }},
    {"smooth_segment_len", &SimBase::smooth_segment_len, "a multiple of 256 in 256..65536",
     [](int v) { return multiple_in(v, 256, 65536); }},
    {"fof_chunk_len", &SimBase::fof_chunk_len, "a multiple of 64 in 64..65536",
     [](int v) { return multiple_in(v, 64, 65536); }},
    {"fof_cell_boxes", &SimBase::fof_cell_boxes, "0 or 1", [](int v) { return v == 0 || v == 1; }},
    {"fof6_boxes", &SimBase::fof6_boxes, "0 or 1", [](int v) { return v == 0 || v == 1; }},
    {"bound_chunk_len", &SimBase::bound_chunk_len, "a multiple of 64 in 64..1048576",
     [](int v) { return multiple_in(v, 64, 1048576); }},
    {"shape_chunk_len", &SimBase::shape_chunk_len, "a multiple of 64 in 64..65536",
     [](int v) { return multiple_in(v, 64, 65536); }},
    {"bound_tile", &SimBase::bound_tile, "0, 64 or 256", [](int v) { return v == 0 || v == 64 || v == 256; }},
    {"knn_span_cells", &SimBase::knn_span_cells, "1..8", [](int v) { return v >= 1 && v <= 8; }},
    {"knn_block_queries", &SimBase::knn_block_queries, "1, 2 or 4", [](int v) { return v == 1 || v == 2 || v == 4; }},
    {"mst_span_cells", &SimBase::mst_span_cells, "1..8", [](int v) { return v >= 1 && v <= 8; }},
    {"mst_block_queries", &SimBase::mst_block_queries, "1, 2 or 4", [](int v) { return v == 1 || v == 2 || v == 4; }},
    {"mst_skip_runs", &SimBase::mst_skip_runs, "0 or 1", [](int v) { return v == 0 || v == 1; }},
    {"mst_shared_bound", &SimBase::mst_shared_bound, "0 or 1", [](int v) { return v == 0 || v == 1; }},
};

extern "C" {

const char *nb_last_error(void) { return g_last_error.c_str(); }
#ifndef NB_SOURCE_HASH
#define NB_SOURCE_HASH "unknown"
#endif
// "... src:<hash>": sha256 prefix of the sources this binary was built from (build.py), so that a
// stale library next to newer sources is detectable (tests/test_abi.py)
const char *nb_version(void) { return "nbody_hip 0.2.0 gfx950 src:" NB_SOURCE_HASH; }

int nb_device_count(void) {
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return 0;
    return c;
}

size_t nb_shard_bodies_per_rank(size_t particle_num, int world) { return shard_bodies_per_rank(particle_num, world); }
size_t nb_shard_padded_bodies(size_t particle_num, int world) { return shard_padded_bodies(particle_num, world); }

int nb_sim_create(nb_sim **out, const nb_sim_params *sim_params, const nb_add_params *add_params,
                  const nb_placement *placement, nb_init_fn init, void *user) {
    NB_GUARD({
        if (!sim_params || !init) {
            set_error("nb_sim_create: sim_params and init must be non-null");
            return NB_ERR_INVALID;
        }
        // init_fn(&sim_params) -> Vec<Particle>, naive.rs:97 / tree.rs:149
        std::vector<nb_particle> host(sim_params->particle_num);
        init(sim_params, host.data(), user);
        return make_sim(out, sim_params, add_params, placement, host.data(), host.size());
    })
}

int nb_sim_create_from_particles(nb_sim **out, const nb_sim_params *sim_params,
                                 const nb_add_params *add_params, const nb_placement *placement,
                                 const nb_particle *particles, size_t n) {
    NB_GUARD({
        if (!particles && n) {
            set_error("nb_sim_create_from_particles: particles is null");
            return NB_ERR_INVALID;
        }
        return make_sim(out, sim_params, add_params, placement, particles, n);
    })
}

#define NB_SIM_CALL(sim, expr)                \
    NB_GUARD({                                \
        if (!(sim) || !(sim)->impl) {         \
            set_error("null simulator");      \
            return NB_ERR_INVALID;            \
        }                                     \
        return (sim)->impl->expr;             \
    })

int nb_sim_encode(nb_sim *sim) { NB_SIM_CALL(sim, encode()) }
int nb_sim_encode_phase(nb_sim *sim, int phase) { NB_SIM_CALL(sim, encode_phase(phase)) }
int nb_sim_let_set_imports(nb_sim *sim, const uint32_t *counts, int world) {
    NB_SIM_CALL(sim, let_set_imports(counts, world))
}
int nb_sim_let_set_import_stride(nb_sim *sim, uint32_t stride) {
    NB_SIM_CALL(sim, let_set_import_stride(stride))
}
int nb_sim_let_set_owners(nb_sim *sim, const unsigned long long *splits, int world, float ref_bound,
                          uint32_t seg_cap) {
    NB_SIM_CALL(sim, let_set_owners(splits, world, ref_bound, seg_cap))
}
int nb_sim_let_set_arrivals(nb_sim *sim, uint32_t stay, const uint32_t *counts, int world) {
    NB_SIM_CALL(sim, let_set_arrivals(stay, counts, world))
}
int nb_sim_cleanup(nb_sim *sim) { NB_SIM_CALL(sim, cleanup()) }
int nb_sim_wait(nb_sim *sim) { NB_SIM_CALL(sim, wait()) }

int nb_sim_sim_params(const nb_sim *sim, nb_sim_params *out) {
    if (!sim || !sim->impl || !out) {
        set_error("null argument");
        return NB_ERR_INVALID;
    }
    *out = sim->impl->params;
    return NB_OK;
}

int nb_sim_read_particles(nb_sim *sim, nb_particle *dst, size_t n) {
    if (!dst && n) {
        set_error("read_particles: dst is null");
        return NB_ERR_INVALID;
    }
    NB_SIM_CALL(sim, read_particles(dst, n))
}

int nb_sim_write_particles(nb_sim *sim, const nb_particle *src, size_t n) {
    if (!src && n) {
        set_error("write_particles: src is null");
        return NB_ERR_INVALID;
    }
    NB_SIM_CALL(sim, write_particles(src, n))
}

int nb_sim_read_tree(nb_sim *sim, nb_octant *dst, size_t cap, size_t *n_nodes, float *root_width) {
    NB_SIM_CALL(sim, read_tree(dst, cap, n_nodes, root_width))
}

int nb_sim_exchange_region(nb_sim *sim, void **dev_ptr, size_t *offset_bytes, size_t *slice_bytes,
                           size_t *total_bytes) {
    NB_SIM_CALL(sim, exchange_region(0, dev_ptr, offset_bytes, slice_bytes, total_bytes))
}

int nb_sim_exchange_count(nb_sim *sim, int *count) {
    if (!sim || !sim->impl || !count) {
        set_error("null argument");
        return NB_ERR_INVALID;
    }
    *count = sim->impl->exchange_count();
    return NB_OK;
}

int nb_sim_exchange_region_i(nb_sim *sim, int index, void **dev_ptr, size_t *offset_bytes,
                             size_t *slice_bytes, size_t *total_bytes) {
    NB_SIM_CALL(sim, exchange_region(index, dev_ptr, offset_bytes, slice_bytes, total_bytes))
}

int nb_sim_step_num(const nb_sim *sim, uint64_t *out) {
    if (!sim || !sim->impl || !out) {
        set_error("null argument");
        return NB_ERR_INVALID;
    }
    *out = sim->impl->step_num;
    return NB_OK;
}

int nb_sim_encode_n_timed(nb_sim *sim, int n, float *ms_total, float *ms_kernel) {
    NB_SIM_CALL(sim, encode_n_timed(n, ms_total, ms_kernel))
}

int nb_sim_set_tuning(nb_sim *sim, const char *key, int value) {
    if (!key) {
        set_error("null key");
        return NB_ERR_INVALID;
    }
    if (!std::strcmp(key, "render_design"))  // the renderer's, whichever simulator holds the state
        return on_sim(sim, key, [&](SimBase &s) { return sim_render_set_design(s, value); });
    for (const TuningKey &t : kTuningKeys) {
        if (std::strcmp(key, t.key)) continue;
        if (!sim || !sim->impl) {
            set_error("null simulator");
            return NB_ERR_INVALID;
        }
        if (!t.ok(value)) {
            set_error("%s: %s, not %d", t.key, t.allowed, value);
            return NB_ERR_INVALID;
        }
        sim->impl.get()->*t.member = value;
        return NB_OK;
    }
    NB_SIM_CALL(sim, set_tuning(key, value))
}

int nb_sim_debug_buffer(nb_sim *sim, const char *name, void *dst, size_t cap, size_t *bytes) {
    if (!name) {
        set_error("null name");
        return NB_ERR_INVALID;
    }
    NB_SIM_CALL(sim, debug_buffer(name, dst, cap, bytes))
}

int nb_sim_diagnostics(nb_sim *sim, uint32_t flags, nb_diagnostics *out) { return pass_diagnostics(sim, flags, out); }
int nb_runner_diagnostics(nb_runner *runner, uint32_t flags, nb_diagnostics *out) {
    return pass_diagnostics(runner, flags, out);
}

int nb_sim_radial_profile(nb_sim *sim, const nb_radial_params *params, nb_radial_profile *out,
                          nb_radial_bin *bins) {
    return pass_radial_profile(sim, params, out, bins);
}
int nb_runner_radial_profile(nb_runner *runner, const nb_radial_params *params, nb_radial_profile *out,
                             nb_radial_bin *bins) {
    return pass_radial_profile(runner, params, out, bins);
}

int nb_radial_edges_log(double rmin, double rmax, uint32_t nbins, double *edges) {
    return radial_edges("radial_edges_log", true, rmin, rmax, nbins, edges);
}
int nb_radial_edges_linear(double rmin, double rmax, uint32_t nbins, double *edges) {
    return radial_edges("radial_edges_linear", false, rmin, rmax, nbins, edges);
}
int nb_radial_lagrangian(const nb_radial_profile *p, const nb_radial_bin *bins, const double *edges,
                         const double *fractions, uint32_t k, double *radii) {
    return radial_lagrangian(p, bins, edges, fractions, k, radii);
}

int nb_sim_field(nb_sim *sim, const float *points, size_t m, uint32_t flags, nb_field_sample *out,
                 nb_field_stats *stats) {
    return pass_field(sim, points, m, flags, out, stats);
}
int nb_runner_field(nb_runner *runner, const float *points, size_t m, uint32_t flags, nb_field_sample *out,
                    nb_field_stats *stats) {
    return pass_field(runner, points, m, flags, out, stats);
}
int nb_field_rings(const double center[3], const double axis[3], const double *radii, uint32_t k, uint32_t n_phi,
                   float *points) {
    return field_rings(center, axis, radii, k, n_phi, points);
}
int nb_field_ring_means(const double center[3], const double axis[3], const double *radii, uint32_t k,
                        uint32_t n_phi, const float *points, const nb_field_sample *samples, nb_field_ring *out) {
    return field_ring_means(center, axis, radii, k, n_phi, points, samples, out);
}

int nb_tidal_sim(nb_sim *sim, const float *points, size_t m, nb_tidal_sample *out, nb_tidal_stats *stats) {
    return pass_tidal(sim, points, m, out, stats);
}
int nb_tidal_runner(nb_runner *runner, const float *points, size_t m, nb_tidal_sample *out, nb_tidal_stats *stats) {
    return pass_tidal(runner, points, m, out, stats);
}
int nb_tidal_ring_means(const double center[3], const double axis[3], const double *radii, uint32_t k,
                        uint32_t n_phi, const float *points, const nb_tidal_sample *samples,
                        const nb_field_ring *rings, nb_tidal_ring *out) {
    return tidal_ring_means(center, axis, radii, k, n_phi, points, samples, rings, out);
}

int nb_orbits_sim(nb_sim *sim, const nb_orbit_params *params, const double *pos, const double *vel, size_t m,
                  nb_orbit_sample *tracks, uint32_t *coincident, nb_orbit_stats *stats) {
    return pass_orbits(sim, params, pos, vel, m, tracks, coincident, stats);
}
int nb_orbits_runner(nb_runner *runner, const nb_orbit_params *params, const double *pos, const double *vel,
                     size_t m, nb_orbit_sample *tracks, uint32_t *coincident, nb_orbit_stats *stats) {
    return pass_orbits(runner, params, pos, vel, m, tracks, coincident, stats);
}
int nb_orbit_sections_sim(nb_sim *sim, const nb_orbit_params *params, const nb_orbit_section_params *section,
                          const double *pos, const double *vel, size_t m, nb_orbit_sample *tracks,
                          uint32_t *coincident, nb_orbit_crossing *crossings, uint32_t *counts,
                          nb_orbit_summary *summaries, nb_orbit_section_stats *stats) {
    return pass_orbit_sections(sim, params, section, pos, vel, m, tracks, coincident, crossings, counts, summaries,
                               stats);
}
int nb_orbit_sections_runner(nb_runner *runner, const nb_orbit_params *params,
                             const nb_orbit_section_params *section, const double *pos, const double *vel, size_t m,
                             nb_orbit_sample *tracks, uint32_t *coincident, nb_orbit_crossing *crossings,
                             uint32_t *counts, nb_orbit_summary *summaries, nb_orbit_section_stats *stats) {
    return pass_orbit_sections(runner, params, section, pos, vel, m, tracks, coincident, crossings, counts, summaries,
                               stats);
}
int nb_orbit_stability_sim(nb_sim *sim, const nb_orbit_params *params, const nb_orbit_stability_params *stability,
                           const double *pos, const double *vel, size_t m, const nb_orbit_deviation *dev0,
                           nb_orbit_sample *tracks, uint32_t *coincident, nb_orbit_deviation *devs,
                           nb_orbit_growth *growth, nb_orbit_stability_stats *stats) {
    return pass_orbit_stability(sim, params, stability, pos, vel, m, dev0, tracks, coincident, devs, growth, stats);
}
int nb_orbit_stability_runner(nb_runner *runner, const nb_orbit_params *params,
                              const nb_orbit_stability_params *stability, const double *pos, const double *vel,
                              size_t m, const nb_orbit_deviation *dev0, nb_orbit_sample *tracks, uint32_t *coincident,
                              nb_orbit_deviation *devs, nb_orbit_growth *growth, nb_orbit_stability_stats *stats) {
    return pass_orbit_stability(runner, params, stability, pos, vel, m, dev0, tracks, coincident, devs, growth, stats);
}
int nb_orbit_stability_derive(double dt, uint32_t steps, uint32_t every, size_t m, uint32_t deviations,
                              const nb_orbit_deviation *dev0, const nb_orbit_deviation *devs, double *log_growth,
                              double *lyapunov, double *sali, double *gali2) {
    NB_GUARD({
        return orbit_stability_derive(dt, steps, every, m, deviations, dev0, devs, log_growth, lyapunov, sali, gali2);
    })
}
int nb_orbit_summary_merge(const nb_orbit_summary *a, const nb_orbit_summary *b, nb_orbit_summary *out) {
    return orbit_summary_merge(a, b, out);
}
uint32_t nb_orbit_records(uint32_t steps, uint32_t every) { return orbit_records(steps, every); }
int nb_orbit_phase(double omega, double dt, uint64_t k, double *c, double *s) {
    return orbit_phase(omega, dt, k, c, s);
}

int nb_sim_map(nb_sim *sim, const nb_map_params *params, uint32_t *counts, double *planes, nb_map_stats *stats) {
    return pass_map(sim, params, counts, planes, stats);
}
int nb_runner_map(nb_runner *runner, const nb_map_params *params, uint32_t *counts, double *planes,
                  nb_map_stats *stats) {
    return pass_map(runner, params, counts, planes, stats);
}
int nb_map_frame(const double axis[3], double n_hat[3], double e1[3], double e2[3]) {
    return map_frame(axis, n_hat, e1, e2);
}
int nb_map_edges(double lo, double hi, uint32_t cells, double *edges) { return map_edges(lo, hi, cells, edges); }

int nb_phase_map_sim(nb_sim *sim, const nb_phase_params *params, uint32_t *counts, double *planes,
                     nb_phase_stats *stats) {
    return pass_phase_map(sim, params, counts, planes, stats);
}
int nb_phase_map_runner(nb_runner *runner, const nb_phase_params *params, uint32_t *counts, double *planes,
                        nb_phase_stats *stats) {
    return pass_phase_map(runner, params, counts, planes, stats);
}
int nb_phase_quantity(const char *name, uint32_t *id) { return phase_quantity(name, id); }
const char *nb_phase_quantity_name(uint32_t id) { return phase_quantity_name(id); }

int nb_sim_fof(nb_sim *sim, const nb_fof_params *params, uint32_t *labels, uint32_t *group_of, nb_fof_group *groups,
               size_t group_capacity, nb_fof_stats *stats) {
    return pass_fof(sim, params, labels, group_of, groups, group_capacity, stats);
}
int nb_runner_fof(nb_runner *runner, const nb_fof_params *params, uint32_t *labels, uint32_t *group_of,
                  nb_fof_group *groups, size_t group_capacity, nb_fof_stats *stats) {
    return pass_fof(runner, params, labels, group_of, groups, group_capacity, stats);
}

int nb_sim_bound(nb_sim *sim, const nb_bound_params *params, uint32_t *group_of, uint32_t *bound_of, double *energy,
                 nb_bound_group *groups, size_t group_capacity, nb_bound_stats *stats) {
    return pass_bound(sim, params, group_of, bound_of, energy, groups, group_capacity, stats);
}
int nb_runner_bound(nb_runner *runner, const nb_bound_params *params, uint32_t *group_of, uint32_t *bound_of,
                    double *energy, nb_bound_group *groups, size_t group_capacity, nb_bound_stats *stats) {
    return pass_bound(runner, params, group_of, bound_of, energy, groups, group_capacity, stats);
}

int nb_sim_knn(nb_sim *sim, const nb_knn_params *params, double *r2, uint32_t *kth, double *mass_in, double *density,
               nb_knn_stats *stats) {
    return pass_knn(sim, params, r2, kth, mass_in, density, stats);
}
int nb_runner_knn(nb_runner *runner, const nb_knn_params *params, double *r2, uint32_t *kth, double *mass_in,
                  double *density, nb_knn_stats *stats) {
    return pass_knn(runner, params, r2, kth, mass_in, density, stats);
}

int nb_fof6_sim(nb_sim *sim, const nb_fof6_params *params, uint32_t *labels, uint32_t *group_of, nb_fof_group *groups,
                size_t group_capacity, nb_fof_stats *stats) {
    return pass_fof6(sim, params, labels, group_of, groups, group_capacity, stats);
}
int nb_fof6_runner(nb_runner *runner, const nb_fof6_params *params, uint32_t *labels, uint32_t *group_of,
                   nb_fof_group *groups, size_t group_capacity, nb_fof_stats *stats) {
    return pass_fof6(runner, params, labels, group_of, groups, group_capacity, stats);
}
int nb_local_kinematics_sim(nb_sim *sim, const nb_kin_params *params, double *moments, double *grads, double *r2,
                            uint32_t *kth, double *mass_in, double *density, nb_kin_stats *stats) {
    return pass_local_kinematics(sim, params, moments, grads, r2, kth, mass_in, density, stats);
}
int nb_local_kinematics_runner(nb_runner *runner, const nb_kin_params *params, double *moments, double *grads,
                               double *r2, uint32_t *kth, double *mass_in, double *density, nb_kin_stats *stats) {
    return pass_local_kinematics(runner, params, moments, grads, r2, kth, mass_in, density, stats);
}
int nb_local_kinematics_derive(const double *moments, const double *grads, const double *r2, const double *density,
                               const float *velocities, size_t n, nb_kin_derived *out) {
    NB_GUARD({ return kin_derive(moments, grads, r2, density, velocities, n, out); })
}

int nb_sim_hop(nb_sim *sim, const nb_hop_params *params, uint32_t *labels, uint32_t *group_of, double *density,
               nb_fof_group *groups, double *peak_density, size_t group_capacity, nb_hop_boundary *boundaries,
               size_t boundary_capacity, nb_hop_stats *stats) {
    return pass_hop(sim, params, labels, group_of, density, groups, peak_density, group_capacity, boundaries,
                    boundary_capacity, stats);
}
int nb_runner_hop(nb_runner *runner, const nb_hop_params *params, uint32_t *labels, uint32_t *group_of,
                  double *density, nb_fof_group *groups, double *peak_density, size_t group_capacity,
                  nb_hop_boundary *boundaries, size_t boundary_capacity, nb_hop_stats *stats) {
    return pass_hop(runner, params, labels, group_of, density, groups, peak_density, group_capacity, boundaries,
                    boundary_capacity, stats);
}
int nb_hop_regroup(const nb_fof_group *rows, const double *peak_density, size_t m, const nb_hop_boundary *bnd,
                   size_t b, const nb_hop_regroup_params *params, uint32_t *merged_of_row, nb_fof_group *out_rows,
                   double *out_peak, size_t out_capacity, size_t *out_count) {
    NB_GUARD({
        return hop_regroup(rows, peak_density, m, bnd, b, params, merged_of_row, out_rows, out_peak, out_capacity,
                           out_count);
    })
}

int nb_mst_sim(nb_sim *sim, const nb_mst_params *params, uint32_t *edge_lo, uint32_t *edge_hi, double *d2,
               uint32_t *degree, nb_mst_stats *stats) {
    return pass_mst(sim, params, edge_lo, edge_hi, d2, degree, stats);
}
int nb_mst_runner(nb_runner *runner, const nb_mst_params *params, uint32_t *edge_lo, uint32_t *edge_hi, double *d2,
                  uint32_t *degree, nb_mst_stats *stats) {
    return pass_mst(runner, params, edge_lo, edge_hi, d2, degree, stats);
}
int nb_mst_cut(size_t n, size_t edges, const uint32_t *edge_lo, const uint32_t *edge_hi, const double *d2,
               const uint32_t *degree, double link, uint32_t *labels, size_t *components) {
    NB_GUARD({ return mst_cut(n, edges, edge_lo, edge_hi, d2, degree, link, labels, components); })
}
int nb_mst_linkage(size_t n, size_t edges, const uint32_t *edge_lo, const uint32_t *edge_hi, uint32_t *label_a,
                   uint32_t *label_b, uint32_t *count_a, uint32_t *count_b) {
    NB_GUARD({ return mst_linkage(n, edges, edge_lo, edge_hi, label_a, label_b, count_a, count_b); })
}

int nb_sim_halo_profiles(nb_sim *sim, const nb_halo_params *params, nb_halo_head *heads, nb_radial_bin *bins,
                         nb_halo_stats *stats) {
    return pass_halo_profiles(sim, params, heads, bins, stats);
}
int nb_runner_halo_profiles(nb_runner *runner, const nb_halo_params *params, nb_halo_head *heads,
                            nb_radial_bin *bins, nb_halo_stats *stats) {
    return pass_halo_profiles(runner, params, heads, bins, stats);
}
int nb_halo_enclosed(const nb_halo_head *head, const nb_radial_bin *bins, uint32_t nbins, double *out) {
    return halo_enclosed(head, bins, nbins, out);
}
int nb_halo_overdensity(const nb_halo_head *head, const nb_radial_bin *bins, const double *edges, uint32_t nbins,
                        double rho, double *r, double *mass) {
    return halo_overdensity(head, bins, edges, nbins, rho, r, mass);
}

int nb_sim_group_shapes(nb_sim *sim, const nb_shape_params *params, const uint32_t *group_of, size_t m,
                        const double *centers, const double *velocities, const double *radius,
                        nb_shape_group *rows_out, uint32_t *selected_of, nb_shape_stats *stats) {
    return pass_group_shapes(sim, params, group_of, m, centers, velocities, radius, rows_out, selected_of, stats);
}
int nb_runner_group_shapes(nb_runner *runner, const nb_shape_params *params, const uint32_t *group_of, size_t m,
                           const double *centers, const double *velocities, const double *radius,
                           nb_shape_group *rows_out, uint32_t *selected_of, nb_shape_stats *stats) {
    return pass_group_shapes(runner, params, group_of, m, centers, velocities, radius, rows_out, selected_of, stats);
}
int nb_group_radii_sim(nb_sim *sim, const nb_radii_params *params, const uint32_t *group_of, size_t m,
                       const double *centers, nb_radii_group *rows_out, uint32_t *rank_of, double *enclosed_of,
                       nb_radii_stats *stats) {
    return pass_group_radii(sim, params, group_of, m, centers, rows_out, rank_of, enclosed_of, stats);
}
int nb_group_radii_runner(nb_runner *runner, const nb_radii_params *params, const uint32_t *group_of, size_t m,
                          const double *centers, nb_radii_group *rows_out, uint32_t *rank_of, double *enclosed_of,
                          nb_radii_stats *stats) {
    return pass_group_radii(runner, params, group_of, m, centers, rows_out, rank_of, enclosed_of, stats);
}
int nb_disc_modes_sim(nb_sim *sim, const nb_modes_params *params, nb_modes_head *out, nb_modes_bin *bins,
                      double *modes) {
    return pass_disc_modes(sim, params, out, bins, modes);
}
int nb_disc_modes_runner(nb_runner *runner, const nb_modes_params *params, nb_modes_head *out, nb_modes_bin *bins,
                         double *modes) {
    return pass_disc_modes(runner, params, out, bins, modes);
}
int nb_disc_modes_derive(const double *modes, uint32_t nbins, uint32_t mmax, uint32_t m, nb_modes_derived *out) {
    NB_GUARD({ return modes_derive(modes, nbins, mmax, m, out); })
}
int nb_shell_modes_sim(nb_sim *sim, const nb_shell_params *params, nb_shell_head *out, nb_shell_bin *bins,
                       double *coef) {
    return pass_shell_modes(sim, params, out, bins, coef);
}
int nb_shell_modes_runner(nb_runner *runner, const nb_shell_params *params, nb_shell_head *out, nb_shell_bin *bins,
                          double *coef) {
    return pass_shell_modes(runner, params, out, bins, coef);
}
int nb_shell_modes_derive(const nb_shell_head *head, const double *coef, nb_shell_derived *out, double *norm,
                          double *phase, double *speed) {
    NB_GUARD({ return shell_derive(head, coef, out, norm, phase, speed); })
}
int nb_shape_eigen(const double t[6], double lambda[3], double axes[9]) {
    if (!t || !lambda || !axes) {
        set_error("shape_eigen: null argument");
        return NB_ERR_INVALID;
    }
    shape_eigen_host(t, lambda, axes);
    return NB_OK;
}

int nb_sim_smooth_map(nb_sim *sim, const nb_smooth_params *params, const double *s, uint32_t *counts, double *planes,
                      nb_smooth_stats *stats) {
    return pass_smooth_map(sim, params, s, counts, planes, stats);
}
int nb_runner_smooth_map(nb_runner *runner, const nb_smooth_params *params, const double *s, uint32_t *counts,
                         double *planes, nb_smooth_stats *stats) {
    return pass_smooth_map(runner, params, s, counts, planes, stats);
}
int nb_smooth_centres(double lo, double hi, uint32_t cells, double *out) { return smooth_centres(lo, hi, cells, out); }

int nb_sim_render(nb_sim *sim, const nb_render_params *params, uint8_t *rgba, uint32_t *counts,
                  nb_render_stats *stats) {
    return pass_render(sim, params, rgba, counts, stats);
}
int nb_runner_render(nb_runner *runner, const nb_render_params *params, uint8_t *rgba, uint32_t *counts,
                     nb_render_stats *stats) {
    return pass_render(runner, params, rgba, counts, stats);
}

int nb_naive_variant_count(void) { return naive_variant_count(); }
const char *nb_naive_variant_name(int v) { return naive_variant_name(v); }

int nb_sim_destroy(nb_sim *sim) {
    if (!sim) return NB_OK;
    if (sim->impl) (void)sim->impl->wait();
    delete sim;
    return NB_OK;
}

// ---- runner: create, step and read (the analysis passes are above, next to the simulator's) ----
int nb_runner_create(nb_runner **out, const nb_sim_params *sim_params,
                     const nb_add_params *add_params, nb_init_fn init, void *user, int device_id) {
    NB_GUARD({
        if (!out) {
            set_error("null argument");
            return NB_ERR_INVALID;
        }
        *out = nullptr;
        nb_placement pl{};
        pl.device_id = device_id < 0 ? 0 : device_id;  // HighPerformance adapter, :23-30
        pl.rank = 0;
        pl.world = 1;
        nb_sim *sim = nullptr;
        if (int rc = nb_sim_create(&sim, sim_params, add_params, &pl, init, user)) return rc;
        nb_runner *r = new nb_runner();
        r->sim = sim;
        *out = r;
        return NB_OK;
    })
}

static int runner_create_group(nb_runner **out, const nb_sim_params *sim_params, const nb_add_params *add_params,
                               nb_init_fn init, void *user, const int *device_ids, int n_devices, int let_migrate_every);

int nb_runner_create_multi(nb_runner **out, const nb_sim_params *sim_params, const nb_add_params *add_params,
                           nb_init_fn init, void *user, const int *device_ids, int n_devices) {
    return runner_create_group(out, sim_params, add_params, init, user, device_ids, n_devices, -1);
}

int nb_runner_create_multi_let(nb_runner **out, const nb_sim_params *sim_params, const nb_add_params *add_params,
                               nb_init_fn init, void *user, const int *device_ids, int n_devices, int migrate_every) {
    if (!add_params || add_params->kind != NB_TREE_SIM_PARAMS || migrate_every < 0) {
        set_error("nb_runner_create_multi_let: TreeSimParams and migrate_every >= 0");
        return NB_ERR_INVALID;
    }
    return runner_create_group(out, sim_params, add_params, init, user, device_ids, n_devices, migrate_every);
}

static int runner_create_group(nb_runner **out, const nb_sim_params *sim_params, const nb_add_params *add_params,
                               nb_init_fn init, void *user, const int *device_ids, int n_devices, int let_migrate_every) {
    NB_GUARD({
        if (!out || !sim_params || !init || !device_ids || n_devices < 1) {
            set_error("nb_runner_create_multi: null argument or no device");
            return NB_ERR_INVALID;
        }
        *out = nullptr;
        if (n_devices == 1 && let_migrate_every < 0)
            return nb_runner_create(out, sim_params, add_params, init, user, device_ids[0]);
        const nb_add_params add = add_params_or_default(add_params);
        if (add.kind != NB_NAIVE_SIM_PARAMS && add.kind != NB_TREE_SIM_PARAMS) {
            set_error("unknown add_params.kind %d", add.kind);
            return NB_ERR_INVALID;
        }
        std::vector<nb_particle> host(sim_params->particle_num);
        init(sim_params, host.data(), user);  // init_fn(&sim_params) -> Vec<Particle>, once, on the host
        std::unique_ptr<DeviceGroup> g;
        if (int rc = DeviceGroup::create(g, *sim_params, add, host.data(), device_ids, n_devices, let_migrate_every))
            return rc;
        nb_runner *r = new nb_runner();
        r->group = std::move(g);
        *out = r;
        return NB_OK;
    })
}

// offline_headless.rs:38-44: encode -> submit -> cleanup -> poll(Wait)
int nb_runner_step(nb_runner *runner) {
    if (int rc = check_runner(runner)) return rc;
    if (runner->group) NB_GUARD({ return runner->group->step_n(1); })
    if (int rc = nb_sim_encode(runner->sim)) return rc;
    if (int rc = nb_sim_cleanup(runner->sim)) return rc;
    return nb_sim_wait(runner->sim);
}

int nb_runner_step_n(nb_runner *runner, int n) {
    if (int rc = check_runner(runner)) return rc;
    if (runner->group) NB_GUARD({ return runner->group->step_n(n); })
    hipEvent_t ev[2] = {nullptr, nullptr};
    const bool prof = runner->profiling && runner->sim->impl && runner->sim->impl->bind_device() == NB_OK &&
                      hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess;
    if (prof) (void)hipEventRecord(ev[0], runner->sim->impl->stream);
    int rc = NB_OK;
    for (int k = 0; k < n && rc == NB_OK; ++k) {
        rc = nb_sim_encode(runner->sim);
        if (rc == NB_OK) rc = nb_sim_cleanup(runner->sim);
    }
    if (prof) (void)hipEventRecord(ev[1], runner->sim->impl->stream);
    const int rw = nb_sim_wait(runner->sim);
    if (prof && hipEventElapsedTime(&runner->kernel_ms, ev[0], ev[1]) != hipSuccess) runner->kernel_ms = 0.f;
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    return rc != NB_OK ? rc : rw;
}

int nb_runner_set_profiling(nb_runner *runner, int on) {
    if (int rc = check_runner(runner)) return rc;
    runner->profiling = on != 0;
    if (runner->group) return runner->group->set_profiling(on != 0);
    return NB_OK;
}

int nb_runner_rank_times(nb_runner *runner, float *kernel_ms, float *wait_ms, int n) {
    if (check_runner(runner) || n < 1) {
        set_error("null runner");
        return NB_ERR_INVALID;
    }
    for (int r = 0; r < n; ++r) {
        if (kernel_ms) kernel_ms[r] = 0.f;
        if (wait_ms) wait_ms[r] = 0.f;
    }
    if (runner->group) return runner->group->rank_times(kernel_ms, wait_ms, n);
    if (kernel_ms) kernel_ms[0] = runner->kernel_ms;
    return NB_OK;
}

int nb_runner_read_particles(nb_runner *runner, nb_particle *dst, size_t n) {
    if (!runner) {
        set_error("null runner");
        return NB_ERR_INVALID;
    }
    if (runner->group) {
        if (!dst && n) {
            set_error("read_particles: dst is null");
            return NB_ERR_INVALID;
        }
        NB_GUARD({ return runner->group->read_particles(dst, n); })
    }
    return nb_sim_read_particles(runner->sim, dst, n);
}

int nb_runner_sim_params(const nb_runner *runner, nb_sim_params *out) {
    if (!runner || !out) {
        set_error("null runner");
        return NB_ERR_INVALID;
    }
    if (runner->group) {
        *out = runner->group->params();
        return NB_OK;
    }
    return nb_sim_sim_params(runner->sim, out);
}

int nb_runner_step_num(const nb_runner *runner, uint64_t *out) {
    if (!runner || !out) {
        set_error("null runner");
        return NB_ERR_INVALID;
    }
    if (runner->group) {
        *out = runner->group->step_num();
        return NB_OK;
    }
    return nb_sim_step_num(runner->sim, out);
}

nb_sim *nb_runner_sim(nb_runner *runner) { return runner ? runner->sim : nullptr; }

int nb_runner_destroy(nb_runner *runner) {
    if (!runner) return NB_OK;
    runner->group.reset();
    nb_sim_destroy(runner->sim);
    delete runner;
    return NB_OK;
}

}  // extern "C"
