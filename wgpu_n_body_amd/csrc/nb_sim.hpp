// nb_sim.hpp -- internal simulator classes behind the opaque nb_sim handle.
#pragma once

#include <memory>
#include <vector>

#include "nb_common.hpp"

namespace nb {

// The workspace of an analysis pass (nb_analysis.hpp): a struct of buffers that free themselves, made by the
// pass's first call and kept in the pass's slot of SimBase::work until the simulator goes.
struct Workspace {
    virtual ~Workspace() = default;
};
enum WorkSlot : int { kWorkDiag = 0, kWorkRender, kWorkRadial, kWorkField, kWorkMap, kWorkFof, kWorkKnn, kWorkSmooth,
                      kWorkBound, kWorkHalo, kWorkHop, kWorkShape, kWorkRadii, kWorkModes, kWorkShell, kWorkPhase, kWorkTidal,
                      kWorkKin, kWorkOrbits, kWorkFof6, kWorkStability, kWorkMst, kWorkSlots };

// The exchange regions of a TreeSim (the index of nb_sim_exchange_region_i), for both of its placements.
enum ExchangeRegion : int {
    // replicated tree (placement world > 1): the rank's slice of each state array
    kRegionPositions = 0,
    kRegionVelocities = 1,
    kRegionAccelerations = 2,
    kReplicatedRegions = 3,
    // LET (tree_let_world set): the protocol's four buffers ...
    kLetMeta = 0,            // bounds, one row of kLetMetaWords words per rank (all-gathered)
    kLetExportCounts = 1,    // one row of `world` counts per rank (all-gathered)
    kLetExportSegments = 2,  // segment q = the records for peer q, segment stride = slice_bytes
    kLetImportArea = 3,      // the peers' records, in rank order with this rank skipped
    kLetRegions = 4,
    // ... and the migration's three, after nb_sim_let_set_owners
    kLetMigrationCounts = 4,  // one row of `world` counts per rank (all-gathered), stayers at [rank]
    kLetLeavers = 5,          // segment q = the bodies whose new owner is q, segment stride = slice_bytes
    kLetArrivals = 6,         // the bodies that arrived, packed in rank order
    kLetRegionsWithMigration = 7,
};
// a migrated body in regions kLetLeavers / kLetArrivals: position + mass, velocity, acceleration
constexpr size_t kMigratedBodyBytes = 3 * sizeof(float4);

// What `trait Simulator` (src/sims/mod.rs:73-90) requires of an implementor, in HIP terms.
class SimBase {
   public:
    virtual ~SimBase();

    int setup_common(const nb_sim_params &p, const nb_add_params &ap, const nb_placement *pl);
    int bind_device() const;
    virtual int wait();  // device.poll(Wait); a TreeSim also reports its device status words

    virtual int init(const nb_particle *host, size_t count) = 0;          // Simulator::new
    virtual int encode() = 0;                                             // Simulator::encode
    virtual int encode_phase(int) {
        set_error("this simulator has no two-phase step");
        return NB_ERR_UNSUPPORTED;
    }
    virtual int cleanup() { return NB_OK; }                               // Simulator::cleanup
    virtual int read_particles(nb_particle *dst, size_t count) = 0;       // dest_particle_slice
    virtual int write_particles(const nb_particle *src, size_t count) = 0;
    virtual int encode_n_timed(int count, float *ms_total, float *ms_kernel) = 0;
    virtual int exchange_count() { return 0; }
    virtual int exchange_region(int, void **, size_t *, size_t *, size_t *) {
        set_error("this simulator has no exchange region");
        return NB_ERR_UNSUPPORTED;
    }
    // one-process runner: store this rank's slice of every exchange region into the same place of
    // every peer's arrays, in one launch on this simulator's stream (peer_bases[q * exchange_count()
    // + k] = base of region k on peer q)
    virtual int push_exchange(void *const *, int) {
        set_error("this simulator has no peer push");
        return NB_ERR_UNSUPPORTED;
    }
    // ... and one small region k (this rank's [off, off + len) of it) into the same place of every peer's
    // region k (peer_bases[q] = base of region k on peer q): the all-gathers of the LET protocol
    virtual int push_region(int, void *const *, int) {
        set_error("this simulator has no peer push");
        return NB_ERR_UNSUPPORTED;
    }
    // LET: the records exported for every peer q (region 2, segment q; as many as the export counted, read
    // on the device) into peer q's import area (import_bases[q] = base of region 3 on rank q; [me] unused),
    // at the segment the fixed-stride layout of nb_sim_let_set_import_stride(stride) gives this rank
    virtual int let_push_segments(void *const *, int, uint32_t) {
        set_error("let_push_segments: not a TreeSim");
        return NB_ERR_UNSUPPORTED;
    }
    virtual int let_set_imports(const uint32_t *, int) {
        set_error("let_set_imports: not a TreeSim");
        return NB_ERR_UNSUPPORTED;
    }
    virtual int let_set_import_stride(uint32_t) {
        set_error("let_set_import_stride: not a TreeSim");
        return NB_ERR_UNSUPPORTED;
    }
    virtual int let_set_owners(const unsigned long long *, int, float, uint32_t) {
        set_error("let_set_owners: not a TreeSim");
        return NB_ERR_UNSUPPORTED;
    }
    virtual int let_set_arrivals(uint32_t, const uint32_t *, int) {
        set_error("let_set_arrivals: not a TreeSim");
        return NB_ERR_UNSUPPORTED;
    }
    virtual int read_tree(nb_octant *, size_t, size_t *, float *) {
        set_error("read_tree: not a TreeSim");
        return NB_ERR_UNSUPPORTED;
    }
    virtual int debug_buffer(const char *name, void *, size_t, size_t *) {
        set_error("unknown debug buffer '%s'", name);
        return NB_ERR_INVALID;
    }
    virtual int set_tuning(const char *key, int) {
        set_error("unknown tuning key '%s'", key);
        return NB_ERR_INVALID;
    }
    // nb_sim_diagnostics: the buffers nb_sim_read_particles converts (x,y,z,m and vx,vy,vz,- per body,
    // bodies [0, n)), and the status of the steps that produced them, read after the stream has drained
    virtual void diag_state(const float4 **posm_out, const float4 **vel_out) const = 0;
    virtual int diag_status() { return NB_OK; }

    nb_sim_params params{};
    nb_add_params add{};
    nb_placement place{};
    hipStream_t stream = nullptr;
    bool own_stream = false;
    uint64_t step_num = 0;
    uint32_t n = 0, n_pad = 0, per_rank = 0, lo = 0, hi = 0;
    std::unique_ptr<Workspace> work[kWorkSlots];  // the analysis passes' workspaces (nb_analysis.hpp)
    int field_pairs_log2 = 35;  // "field_launch_pairs_log2": pairs per launch of nb_sim_field, 2^16 .. 2^40
    int map_segment_len = 4096;  // "map_segment_len": bodies of a tile summed by one block of nb_sim_map
    int phase_segment_len = 4096;  // "phase_segment_len": bodies of a tile summed by one block of nb_phase_map_sim
    int smooth_segment_len = 4096;  // "smooth_segment_len": entries of a tile summed by one block of nb_sim_smooth_map
    int fof_chunk_len = 1024;    // "fof_chunk_len": bodies of a cell or a catalogue row per work item of nb_sim_fof
    int fof_cell_boxes = 1;      // "fof_cell_boxes": per-cell bounding boxes decide neighbour cells where they can
    int fof6_boxes = 1;          // "fof6_boxes": per-cell position and velocity boxes decide cell pairs of nb_fof6_sim
    int bound_chunk_len = 1024;  // "bound_chunk_len": j positions of a group per work item of nb_sim_bound's pair pass
    int bound_tile = 0;          // "bound_tile": members per i-tile of that pass, 64 or 256; 0 chooses by the group's size
    int shape_chunk_len = 1024;  // "shape_chunk_len": positions of a row's list per work item of nb_sim_group_shapes
    int knn_span_cells = 3;      // "knn_span_cells": octree cells per axis the search of nb_sim_knn opens around a body
    int knn_block_queries = 4;   // "knn_block_queries": bodies (a wave each) per block of that search
    int mst_span_cells = 3;      // "mst_span_cells": octree cells per axis the search of nb_mst_sim starts from
    int mst_block_queries = 4;   // "mst_block_queries": bodies (a wave each) per block of that search
    int mst_skip_runs = 1;       // "mst_skip_runs": stretches of the body's own component are stepped over
    int mst_shared_bound = 1;    // "mst_shared_bound": a component's bodies share the smallest d2 found so far
};

// nb_diag.hip: nb_sim_diagnostics behind the handle
int sim_diagnostics(SimBase &sim, uint32_t flags, nb_diagnostics *out);
// the moments pass and its finish alone, enqueued on the simulator's stream (n > 0; the device is bound):
// *res_dev = the finished sums on the device, mass at [kDiagResMass], sum m x at [kDiagResMX + k], sum m v
// at [kDiagResMV + k] -- what sim_diagnostics divides into `com` and reports as `momentum`
// (and the count of non-finite bodies at [kDiagResBad])
constexpr int kDiagResMass = 0, kDiagResMX = 1, kDiagResMV = 4, kDiagResBad = 12;
int diag_enqueue_moments(SimBase &sim, const double **res_dev);

// Every pass below is stated as its refusal rules and the call behind the handle.  The rules that need no device
// live in nb_passes.cpp (the renderer's in nb_camera.cpp, next to the camera they share) and run before the
// simulator is looked at; sim_X takes arguments they have passed.

// nb_render.hip: nb_sim_render behind the handle and the "render_design" tuning key
int render_check_params(const nb_render_params *params);
int sim_render(SimBase &sim, const nb_render_params &params, uint8_t *rgba, uint32_t *counts, nb_render_stats *stats);
int sim_render_set_design(SimBase &sim, int design);

// nb_radial.hip: nb_sim_radial_profile behind the handle; radial_edges: nb_radial_edges_log / _linear behind the
// ABI boundary (`what` names the entry point in a refusal)
int radial_check_params(const nb_radial_params *p, const nb_radial_profile *out, const nb_radial_bin *bins);
int sim_radial_profile(SimBase &sim, const nb_radial_params &params, nb_radial_profile *out, nb_radial_bin *bins);
int radial_edges(const char *what, bool log, double rmin, double rmax, uint32_t nbins, double *edges);

// nb_field.hip: nb_sim_field behind the handle
int field_check_args(const float *points, size_t m, uint32_t flags, const nb_field_sample *out);
int sim_field(SimBase &sim, const float *points, size_t m, uint32_t flags, nb_field_sample *out, nb_field_stats *stats);

// nb_tidal.hip: nb_tidal_sim behind the handle
int tidal_check_args(const float *points, size_t m, const nb_tidal_sample *out);
int sim_tidal(SimBase &sim, const float *points, size_t m, nb_tidal_sample *out, nb_tidal_stats *stats);

// nb_field.hip: nb_orbits_sim behind the handle (the orbit unit shares the field's pair kernels); orbits_check_args
// also forms the frame; orbit_records / orbit_phase: nb_orbit_records / nb_orbit_phase behind the ABI boundary
struct OrbitPlan {
    double n[3], e1[3], e2[3];  // axis_frame of the caller's axis (omega != 0)
    uint32_t records;
};
int orbits_check_args(const nb_orbit_params *p, const double *pos, const double *vel, size_t m,
                      const nb_orbit_sample *tracks, OrbitPlan *plan);
int orbits_check_e(const SimBase &sim, const nb_orbit_params *p);
int sim_orbits(SimBase &sim, const nb_orbit_params &params, const OrbitPlan &plan, const double *pos, const double *vel,
               size_t m, nb_orbit_sample *tracks, uint32_t *coincident, nb_orbit_stats *stats);
uint32_t orbit_records(uint32_t steps, uint32_t every);
int orbit_phase(double omega, double dt, uint64_t k, double *c, double *s);
// ... nb_orbit_sections_sim (include/nbody.h "Orbit sections"): the same call whose step kernel also takes the
// crossings and the summaries; orbit_sections_check_args runs orbits_check_args and forms the frame for omega == 0 too
int orbit_sections_check_args(const nb_orbit_params *p, const nb_orbit_section_params *sec, const double *pos,
                              const double *vel, size_t m, const nb_orbit_sample *tracks,
                              const nb_orbit_crossing *crossings, OrbitPlan *plan);
int sim_orbit_sections(SimBase &sim, const nb_orbit_params &params, const nb_orbit_section_params &sec,
                       const OrbitPlan &plan, const double *pos, const double *vel, size_t m, nb_orbit_sample *tracks,
                       uint32_t *coincident, nb_orbit_crossing *crossings, uint32_t *counts,
                       nb_orbit_summary *summaries, nb_orbit_section_stats *stats);
int orbit_summary_merge(const nb_orbit_summary *a, const nb_orbit_summary *b, nb_orbit_summary *out);
// nb_stability.hip: nb_orbit_stability_sim behind the handle (include/nbody.h "Orbit stability"): the orbit's sequence
// with this unit's pair kernel and step kernel; orbit_stability_check_args runs orbits_check_args and then its own
// refusals; orbit_stability_derive: nb_orbit_stability_derive behind the ABI boundary
int orbit_stability_check_args(const nb_orbit_params *p, const nb_orbit_stability_params *sp, const double *pos,
                               const double *vel, size_t m, const nb_orbit_deviation *dev0,
                               const nb_orbit_sample *tracks, const nb_orbit_deviation *devs, OrbitPlan *plan);
int sim_orbit_stability(SimBase &sim, const nb_orbit_params &params, const nb_orbit_stability_params &sp,
                        const OrbitPlan &plan, const double *pos, const double *vel, size_t m,
                        const nb_orbit_deviation *dev0, nb_orbit_sample *tracks, uint32_t *coincident,
                        nb_orbit_deviation *devs, nb_orbit_growth *growth, nb_orbit_stability_stats *stats);
int orbit_stability_derive(double dt, uint32_t steps, uint32_t every, size_t m, uint32_t deviations,
                           const nb_orbit_deviation *dev0, const nb_orbit_deviation *devs, double *log_growth,
                           double *lyapunov, double *sali, double *gali2);

// nb_map.hip: nb_sim_map behind the handle; map_check_params also forms the frame and the cell sizes
struct MapPlan {
    double n[3], e1[3], e2[3];  // axis_frame of the caller's axis
    double dx, dy;              // (hi - lo) / W, (hi - lo) / H
};
int map_check_params(const nb_map_params *p, MapPlan *plan);
int sim_map(SimBase &sim, const nb_map_params &params, const MapPlan &plan, uint32_t *counts, double *planes,
            nb_map_stats *stats);
// nb_phase.hip: nb_phase_map_sim behind the handle; phase_check_params also forms the frame, phase_check_args is
// what needs the simulator's step number; phase_quantity / phase_quantity_name: the table of names behind
// nb_phase_quantity / nb_phase_quantity_name
struct PhasePlan {
    double n[3], e1[3], e2[3];  // axis_frame of the caller's axis
    bool uses_values;           // x, y or (NB_PHASE_WEIGHT) q is NB_PHASE_Q_VALUE
};
int phase_check_params(const nb_phase_params *p, PhasePlan *plan);
int phase_check_args(const SimBase &sim, const nb_phase_params *p, const PhasePlan &plan);
int sim_phase_map(SimBase &sim, const nb_phase_params &params, const PhasePlan &plan, uint32_t *counts, double *planes,
                  nb_phase_stats *stats);
int phase_quantity(const char *name, uint32_t *id);
const char *phase_quantity_name(uint32_t id);
// nb_fof.hip: nb_sim_fof behind the handle
int fof_check_params(const nb_fof_params *p);
int sim_fof(SimBase &sim, const nb_fof_params &params, uint32_t *labels, uint32_t *group_of, nb_fof_group *groups,
            size_t group_capacity, nb_fof_stats *stats);
// nb_fof6.hip: nb_fof6_sim behind the handle
int fof6_check_params(const nb_fof6_params *p);
int sim_fof6(SimBase &sim, const nb_fof6_params &params, uint32_t *labels, uint32_t *group_of, nb_fof_group *groups,
             size_t group_capacity, nb_fof_stats *stats);
// nb_halo.hip: nb_sim_halo_profiles behind the handle (the body indices need n: they are checked there)
int halo_check_params(const nb_halo_params *p);
int sim_halo_profiles(SimBase &sim, const nb_halo_params &params, nb_halo_head *heads, nb_radial_bin *bins,
                      nb_halo_stats *stats);

// nb_bound.hip: nb_sim_bound behind the handle; the softening is the simulator's (bound_check_e)
int bound_check_params(const nb_bound_params *p);
int bound_check_e(const SimBase &sim);
int sim_bound(SimBase &sim, const nb_bound_params &params, uint32_t *group_of, uint32_t *bound_of, double *energy,
              nb_bound_group *groups, size_t group_capacity, nb_bound_stats *stats);
// nb_shape.hip: nb_sim_group_shapes behind the handle -- the parameters alone, then what needs the simulator's n and
// step number (the values of group_of are checked on the device) -- and nb_shape_eigen's body, which lives in the
// unit built without contraction
int shape_check_params(const nb_shape_params *p);
int shape_check_args(const SimBase &sim, const nb_shape_params *p, const uint32_t *group_of, size_t m,
                     const double *centers, const double *velocities, const double *radius);
int sim_group_shapes(SimBase &sim, const nb_shape_params &params, const uint32_t *group_of, size_t m,
                     const double *centers, const double *velocities, const double *radius, nb_shape_group *rows,
                     uint32_t *selected_of, nb_shape_stats *stats);
void shape_eigen_host(const double t[6], double lambda[3], double axes[9]);
// nb_radii.hip: nb_group_radii_sim behind the handle, checked like nb_sim_group_shapes: the parameters alone, then
// what needs the simulator's n and step number (the values of group_of are checked on the device)
int radii_check_params(const nb_radii_params *p);
int radii_check_args(const SimBase &sim, const nb_radii_params *p, const uint32_t *group_of, size_t m,
                     const double *centers);
int sim_group_radii(SimBase &sim, const nb_radii_params &params, const uint32_t *group_of, size_t m,
                    const double *centers, nb_radii_group *rows, uint32_t *rank_of, double *enclosed_of,
                    nb_radii_stats *stats);
// nb_modes.hip: nb_disc_modes_sim behind the handle; modes_derive: nb_disc_modes_derive behind the ABI boundary
int modes_check_params(const nb_modes_params *p, const nb_modes_head *out, const nb_modes_bin *bins,
                       const double *modes);
int sim_disc_modes(SimBase &sim, const nb_modes_params &params, nb_modes_head *out, nb_modes_bin *bins, double *modes);
int modes_derive(const double *modes, uint32_t nbins, uint32_t mmax, uint32_t m, nb_modes_derived *out);
// nb_shell.hip: nb_shell_modes_sim behind the handle; shell_derive: nb_shell_modes_derive behind the ABI boundary
int shell_check_params(const nb_shell_params *p, const nb_shell_head *out, const nb_shell_bin *bins,
                       const double *coef);
int sim_shell_modes(SimBase &sim, const nb_shell_params &params, nb_shell_head *out, nb_shell_bin *bins, double *coef);
int shell_derive(const nb_shell_head *head, const double *coef, nb_shell_derived *out, double *norm, double *phase,
                 double *speed);
// nb_knn.hip: nb_sim_knn behind the handle
int knn_check_params(const nb_knn_params *p);
int sim_knn(SimBase &sim, const nb_knn_params &params, double *r2, uint32_t *kth, double *mass_in, double *density,
            nb_knn_stats *stats);
// nb_mst.hip: nb_mst_sim behind the handle; mst_cut / mst_linkage: nb_mst_cut / nb_mst_linkage behind the ABI boundary
int mst_check_params(const nb_mst_params *p);
int sim_mst(SimBase &sim, const nb_mst_params &params, uint32_t *edge_lo, uint32_t *edge_hi, double *d2,
            uint32_t *degree, nb_mst_stats *stats);
int mst_cut(size_t n, size_t edges, const uint32_t *edge_lo, const uint32_t *edge_hi, const double *d2,
            const uint32_t *degree, double link, uint32_t *labels, size_t *components);
int mst_linkage(size_t n, size_t edges, const uint32_t *edge_lo, const uint32_t *edge_hi, uint32_t *label_a,
                uint32_t *label_b, uint32_t *count_a, uint32_t *count_b);
// nb_kinematics.hip: nb_local_kinematics_sim behind the handle; kin_derive: nb_local_kinematics_derive behind the
// ABI boundary
int kin_check_params(const nb_kin_params *p);
int sim_local_kinematics(SimBase &sim, const nb_kin_params &params, double *moments, double *grads, double *r2,
                         uint32_t *kth, double *mass_in, double *density, nb_kin_stats *stats);
int kin_derive(const double *moments, const double *grads, const double *r2, const double *density,
               const float *velocities, size_t n, nb_kin_derived *out);
// nb_hop.hip: nb_sim_hop behind the handle
int hop_check_params(const nb_hop_params *p);
int sim_hop(SimBase &sim, const nb_hop_params &params, uint32_t *labels, uint32_t *group_of, double *density,
            nb_fof_group *groups, double *peak_density, size_t group_capacity, nb_hop_boundary *boundaries,
            size_t boundary_capacity, nb_hop_stats *stats);
// nb_smooth.hip: nb_sim_smooth_map behind the handle; smooth_check_params also forms the frame, the pixel sizes and
// the pixel centres
struct SmoothPlan {
    MapPlan frame;
    std::vector<double> xc, yc;  // nb_smooth_centres of the two windows
};
int smooth_check_params(const nb_smooth_params *p, SmoothPlan *plan);
int sim_smooth_map(SimBase &sim, const nb_smooth_params &params, const SmoothPlan &plan, const double *s,
                   uint32_t *counts, double *planes, nb_smooth_stats *stats);
// nb_passes.cpp: the unit axis n and the basis e1, e2 = n x e1 that nb_field_rings and the maps share (the
// rule of include/nbody.h); false for an axis without a finite, non-zero length
bool axis_frame(const double axis[3], double n[3], double e1[3], double e2[3]);
// nb_passes.cpp: the host-only entry points of include/nbody.h behind the ABI boundary (nb_X is X here)
int radial_lagrangian(const nb_radial_profile *p, const nb_radial_bin *bins, const double *edges,
                      const double *fractions, uint32_t k, double *radii);
int field_rings(const double center[3], const double axis[3], const double *radii, uint32_t k, uint32_t n_phi,
                float *points);
int field_ring_means(const double center[3], const double axis[3], const double *radii, uint32_t k, uint32_t n_phi,
                     const float *points, const nb_field_sample *samples, nb_field_ring *out);
int tidal_ring_means(const double center[3], const double axis[3], const double *radii, uint32_t k, uint32_t n_phi,
                     const float *points, const nb_tidal_sample *samples, const nb_field_ring *rings,
                     nb_tidal_ring *out);
int halo_enclosed(const nb_halo_head *head, const nb_radial_bin *bins, uint32_t nbins, double *out);
int halo_overdensity(const nb_halo_head *head, const nb_radial_bin *bins, const double *edges, uint32_t nbins,
                     double rho, double *r, double *mass);
int hop_regroup(const nb_fof_group *rows, const double *peak_density, size_t m, const nb_hop_boundary *bnd, size_t b,
                const nb_hop_regroup_params *params, uint32_t *merged_of_row, nb_fof_group *out_rows,
                double *out_peak, size_t out_capacity, size_t *out_count);
int map_frame(const double axis[3], double n_hat[3], double e1[3], double e2[3]);
int map_edges(double lo, double hi, uint32_t cells, double *edges);
int smooth_centres(double lo, double hi, uint32_t cells, double *out);

class NaiveSim final : public SimBase {
   public:
    ~NaiveSim() override;
    int init(const nb_particle *host, size_t count) override;
    int encode() override;
    int encode_phase(int phase) override;
    int read_particles(nb_particle *dst, size_t count) override;
    int write_particles(const nb_particle *src, size_t count) override;
    int encode_n_timed(int count, float *ms_total, float *ms_kernel) override;
    int exchange_count() override { return 1; }
    int exchange_region(int index, void **dev_ptr, size_t *off, size_t *len, size_t *total) override;
    int set_tuning(const char *key, int value) override;
    void diag_state(const float4 **posm_out, const float4 **vel_out) const override {
        *posm_out = posm[cur];
        *vel_out = vel;
    }
    // one-process multi-GPU (nb_group.cpp): this simulator's two position buffers, and the peers'
    void position_buffers(float4 *out[2]) const {
        out[0] = posm[0];
        out[1] = posm[1];
    }
    int set_peers(float4 *const *peer_buf0, float4 *const *peer_buf1, int count);

   private:
    PeerDst peers[2] = {};                 // peers[b]: the peers' buffers with ping-pong index b
    float4 *posm[2] = {nullptr, nullptr};  // ping-pong position/mass (naive.rs:99-132)
    bool own_posm = true;
    float4 *vel = nullptr, *acc = nullptr;  // this rank's bodies only
    nb_particle *d_aos = nullptr;           // AoS staging for the 40-byte boundary layout
    int cur = 0;                            // posm[cur] holds the current state
    int variant = -1, jsplit = 0;           // tuning overrides (<0 / 0 = automatic)
    int mass_runs = 1;                      // sum runs of equal masses unweighted (nb_naive.hip)
    float4 *partial = nullptr;              // j-split partial sums [slices][per_rank]
    uint32_t partial_slices = 0;
    int ensure_workspace();
    int launch(int phase);
    bool local_done = false;                // phase 0 of the NEXT step already enqueued
    std::vector<hipEvent_t> events;
};

// Implemented in nb_tree.hip; returns nullptr when the tree path is not built.
SimBase *make_tree_sim();

// nb_simbase.cpp: construct a simulator object (what nb_sim_create does behind the handle); add_params == NULL
// stands for the all-pairs simulator; the shard layout of nb_shard_bodies_per_rank / nb_shard_padded_bodies
nb_add_params add_params_or_default(const nb_add_params *ap);
size_t shard_bodies_per_rank(size_t particle_num, int world);
size_t shard_padded_bodies(size_t particle_num, int world);
int make_sim_impl(std::unique_ptr<SimBase> &out, const nb_sim_params *sp, const nb_add_params *ap,
                  const nb_placement *pl, const nb_particle *particles, size_t count);

}  // namespace nb

struct nb_sim {
    std::unique_ptr<nb::SimBase> impl;
};
