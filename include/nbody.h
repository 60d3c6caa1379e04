/*
 * nbody.h -- C ABI of the MI355X-native N-body engine (libnbody_hip.so).
 *
 * This is the drop-in boundary for ONE hot path of arpan-dhatt/wgpu-n-body: the
 * per-step force accumulation + kick-drift-kick integrator that the reference
 * runs as WGSL compute shaders behind `trait Simulator`, driven by
 * `OfflineHeadless<T>`.  Every entry point below cites the reference interface
 * it replaces (paths are relative to the reference crate root).
 *
 * Conventions
 *   - plain C, POD structs, plain pointers and sizes; no C++/torch types.
 *   - every function returning `int` returns NB_OK (0) on success or an
 *     nb_status code; a human-readable message for the calling thread's last
 *     failure is available from nb_last_error().  Nothing unwinds across the
 *     ABI (the reference's constructors return anyhow::Result,
 *     src/sims/mod.rs:80; its step() panics, src/sims/tree.rs:278-280 -- here
 *     both become status codes).
 *   - single caller thread per handle, not re-entrant (same as the reference:
 *     `Simulator` has no Send/Sync bound, src/sims/mod.rs:73-90).
 *   - there is NO CPU fallback: if no HIP device is usable, create() fails with
 *     NB_ERR_NO_DEVICE.
 */
#ifndef NBODY_H_
#define NBODY_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- */
/* Data model (byte-exact mirrors of the reference's #[repr(C)] PODs)         */
/* ------------------------------------------------------------------------- */

/* `struct Particle`, src/sims/mod.rs:9-16 (WGSL mirror naive.wgsl:1-6,
 * array stride 40, naive.wgsl:15-17).  40 bytes, 10 x f32. */
typedef struct nb_particle {
    float position[3];
    float velocity[3];
    float acceleration[3]; /* stored quantity is sum(f)*dt, naive.wgsl:41 */
    float mass;
} nb_particle;

/* `struct SimParams`, src/sims/mod.rs:51-58.  16 bytes. */
typedef struct nb_sim_params {
    uint32_t particle_num;
    float g;
    float e;
    float dt;
} nb_sim_params;

/* `SimParams::default()`, src/sims/mod.rs:62-71 */
#define NB_DEFAULT_PARTICLE_NUM 10000u
#define NB_DEFAULT_G 0.000001f
#define NB_DEFAULT_E 0.0001f
#define NB_DEFAULT_DT 0.016f
/* default theta when a TreeSim gets no TreeSimParams, src/sims/tree.rs:42-51 */
#define NB_DEFAULT_THETA 0.75f
/* `PARTICLES_PER_GROUP`, src/sims/mod.rs:7 (the reference's workgroup size;
 * kept for API parity -- the HIP kernels choose their own tiling). */
#define NB_PARTICLES_PER_GROUP 64u

/* `enum AddParams`, src/sims/mod.rs:18-23 */
typedef enum nb_add_kind {
    NB_NAIVE_SIM_PARAMS = 0, /* AddParams::NaiveSimParams            */
    NB_TREE_SIM_PARAMS = 1   /* AddParams::TreeSimParams { theta }   */
} nb_add_kind;

typedef struct nb_add_params {
    int32_t kind; /* nb_add_kind */
    float theta;  /* only read when kind == NB_TREE_SIM_PARAMS; <= 0 -> default */
} nb_add_params;

/* `struct Octant`, src/sims/tree.rs:605-622 (WGSL mirror tree.wgsl:1-6,
 * stride 52, tree.wgsl:31-33).  52 bytes.  Returned by nb_sim_read_tree. */
typedef struct nb_octant {
    float cog[3];
    float mass;
    uint32_t bodies;
    uint32_t children[8]; /* 0 = no child; for a leaf (bodies==1) children[0] is
                             the body's index in the step's source order */
} nb_octant;

/* The init callback: `init_fn: fn(&SimParams) -> Vec<Particle>`,
 * src/sims/mod.rs:79 / src/runners/offline_headless.rs:20.  The callee fills
 * out[0 .. params->particle_num).  `user` is an opaque cookie (the Rust fn
 * pointer has no environment; a C callback needs one). */
typedef void (*nb_init_fn)(const nb_sim_params *params, nb_particle *out, void *user);

typedef enum nb_status {
    NB_OK = 0,
    NB_ERR_INVALID = 1,    /* bad argument */
    NB_ERR_NO_DEVICE = 2,  /* no usable HIP device */
    NB_ERR_HIP = 3,        /* a HIP runtime call failed */
    NB_ERR_ALLOC = 4,      /* host or device allocation failed */
    NB_ERR_UNSUPPORTED = 5 /* valid request this build does not implement */
} nb_status;

/* Message describing the calling thread's most recent failing call ("" if none). */
const char *nb_last_error(void);
/* "nbody_hip <semver> gfx950" */
const char *nb_version(void);
/* Number of visible HIP devices (0 when there is none or the runtime fails). */
int nb_device_count(void);

/* ------------------------------------------------------------------------- */
/* Inits -- seeded equivalents of src/inits.rs                                */
/* ------------------------------------------------------------------------- */
/* The reference draws from rand::thread_rng() (src/inits.rs:7,30,58), which
 * is OS-seeded and not reproducible; these reproduce the *distributions* with
 * a counter-based generator specified bit-exactly in DESIGN.md ("RNG").
 * All three have the nb_init_fn signature.  `user` is NULL (seed 0) or points
 * to a uint64_t seed. */
void nb_init_uniform(const nb_sim_params *params, nb_particle *out, void *user);   /* inits.rs:6-27  */
void nb_init_disc(const nb_sim_params *params, nb_particle *out, void *user);      /* inits.rs:29-54 */
void nb_init_spherical(const nb_sim_params *params, nb_particle *out, void *user); /* inits.rs:56-83 */

/* ------------------------------------------------------------------------- */
/* Simulator -- `trait Simulator`, src/sims/mod.rs:73-90                      */
/* ------------------------------------------------------------------------- */
typedef struct nb_sim nb_sim;

/* Where a simulator lives and which bodies it owns.
 *
 * Single GPU: { device_id, 0, 1, NULL, {NULL,NULL} }.
 *
 * Multi GPU (one process per GPU): rank r of `world` owns the contiguous body
 * range [r*per, min(N,(r+1)*per)) with per = nb_shard_bodies_per_rank(N, world).
 * Each step writes only that slice of the new position/mass buffer; the caller
 * all-gathers the slices (RCCL) before the next nb_sim_encode.  There is no
 * reference counterpart (single adapter, src/runners/offline_headless.rs:22-31).
 *
 * `stream`: a hipStream_t the kernels are enqueued on, or NULL to let the
 * simulator create its own.  `posm[0..1]`: optional caller-owned device
 * buffers for the two ping-pong position/mass arrays (float4 x
 * nb_shard_padded_bodies(N, world) each, 16-byte aligned) -- this is how a host
 * that owns device memory (e.g. torch + torch.distributed) runs the collective
 * in place; NULL lets the simulator allocate them. */
typedef struct nb_placement {
    int32_t device_id;
    int32_t rank;
    int32_t world;
    void *stream;
    void *posm[2];
} nb_placement;

/* Bodies per rank (a multiple of the kernels' i-tile) and the padded length of
 * the position/mass buffers (= world * per_rank >= N). */
size_t nb_shard_bodies_per_rank(size_t particle_num, int world);
size_t nb_shard_padded_bodies(size_t particle_num, int world);

/* `Simulator::new(device, sim_params, add_params, mappable_primary_buffers,
 * init_fn)`, src/sims/mod.rs:74-82; NaiveSim::new src/sims/naive.rs:20-145,
 * TreeSim::new src/sims/tree.rs:29-260.  `device` becomes nb_placement;
 * `mappable_primary_buffers` has no HIP meaning and is dropped.  add_params
 * selects the implementation: NB_NAIVE_SIM_PARAMS -> all-pairs (NaiveSim),
 * NB_TREE_SIM_PARAMS -> Barnes-Hut (TreeSim).  placement may be NULL
 * (device 0, single GPU).  init runs on the host exactly once, for all
 * particle_num bodies (every rank must supply identical data). */
int nb_sim_create(nb_sim **out, const nb_sim_params *sim_params, const nb_add_params *add_params,
                  const nb_placement *placement, nb_init_fn init, void *user);

/* Same, from an existing particle array instead of a callback
 * (snapshot/restore; also how tests feed identical bytes to the
 * oracle and the GPU). */
int nb_sim_create_from_particles(nb_sim **out, const nb_sim_params *sim_params,
                                 const nb_add_params *add_params, const nb_placement *placement,
                                 const nb_particle *particles, size_t n);

/* `Simulator::encode(&mut self, device, queue) -> CommandEncoder`
 * (src/sims/mod.rs:83; NaiveSim::encode src/sims/naive.rs:147-162,
 * TreeSim::encode src/sims/tree.rs:262-353) fused with the runner's
 * `queue.submit` (src/runners/offline_headless.rs:40): enqueues ONE step on
 * the simulator's stream and returns without waiting; flips the ping-pong
 * (naive.rs:156,160). */
int nb_sim_encode(nb_sim *sim);

/* The same step in two halves, so that a multi-GPU caller can overlap the exchange of step k
 * with the beginning of step k+1.
 * TreeSim: phase 0 = bound, keys, sort, reorder of positions, octree build (needs positions and
 * masses only); phase 1 = reorder of velocities/accelerations, walk + integrate.  A sharded host
 * gathers positions first, enqueues phase 0, and lets the other two gathers run beside it.
 * NaiveSim (world > 1; otherwise phase 0 is a no-op and phase 1 is nb_sim_encode):
 *   phase 0 -- interactions with the rank's OWN bodies.  Needs only this rank's slice of the
 *              current positions, so it may be enqueued right after the previous step, while
 *              the all-gather of the other slices is still in flight;
 *   phase 1 -- interactions with everybody else's bodies (enqueue after the exchange has been
 *              ordered on the stream), then the integrator; flips the ping-pong.
 * nb_sim_encode after a phase 0 completes that step (= phase 1). */
int nb_sim_encode_phase(nb_sim *sim, int phase);

/* Multi-GPU Barnes-Hut with locally essential trees (LET; no reference counterpart -- the
 * reference has one device).  Every rank creates a TreeSim over ITS OWN bodies (placement world 1),
 * then sets the tuning keys "tree_let_world", "tree_let_rank" and "tree_let_cap" (records a peer
 * may receive from this rank; allocates the buffers).  One step is three phases with an exchange
 * after the first two (regions are those of nb_sim_exchange_region_i):
 *   NB_PHASE_LET_META   local bound + bounding box of the drifted bodies -> region 0;
 *                       caller: all-gather region 0 in place (32 B per rank)
 *   NB_PHASE_LET_BUILD  global root cube, octree of the rank's bodies, and for every peer the part
 *                       of that octree the peer's box can reach (32-byte records, children
 *                       contiguous, links relative to the segment) -> region 2, counts -> region 1;
 *                       caller: all-gather region 1 (`world` u32 per rank), read it, move
 *                       counts[r][me] records of rank r's segment `me` into region 3 packed in rank
 *                       order, then nb_sim_let_set_imports(counts received from each rank)
 *   NB_PHASE_LET_WALK   walk own tree + imported trees, integrate.
 * Walking an imported tree gives bit for bit what walking the peer's whole octree would give. */
#define NB_PHASE_LET_META 2
#define NB_PHASE_LET_BUILD 3
#define NB_PHASE_LET_WALK 4
int nb_sim_let_set_imports(nb_sim *sim, const uint32_t *counts, int world);
/* The same hand-over without a host round trip: the caller moves a FIXED number of records per peer
 * -- `stride` records of rank r's segment `me` to record offset j * stride of region 3, j = r's
 * position in rank order with `me` skipped -- sized from an earlier step's counts plus a margin, and
 * calls this instead of nb_sim_let_set_imports.  The counts themselves stay on the device: region 1,
 * all-gathered by the caller, is read by the kernel that prepares the imports.  A peer that has more
 * than `stride` records for this rank is reported like a too small tree_let_cap (nb_sim_wait). */
int nb_sim_let_set_import_stride(nb_sim *sim, uint32_t stride);

/* Migration between LET steps.  A TreeSim created with more bodies than it starts with (the
 * surplus is headroom; tuning key "tree_let_active" = bodies in use) can hand over the bodies
 * that left its domain: rank r owns the Morton keys [splits[r-1], splits[r]) of positions
 * quantised to 21 bits per axis in the fixed cube [-ref_bound, ref_bound]^3 (splits: world-1
 * values).  NB_PHASE_LET_MIGRATE compacts the stayers and packs the leavers per owner (region 5,
 * 48 B per body, at most seg_cap per owner) with the counts in region 4 (stayers at [rank]); the
 * caller all-gathers region 4, moves the segments into region 6 packed in rank order and calls
 * nb_sim_let_set_arrivals(stayers, arrivals per rank); nb_sim_sim_params then reports the new
 * body count. */
#define NB_PHASE_LET_MIGRATE 5
/* Optional, between NB_PHASE_LET_BUILD and NB_PHASE_LET_WALK: walk the rank's own octree (it needs
 * nothing from the peers) while the exported trees are still being exchanged; NB_PHASE_LET_WALK
 * then adds the imported trees and integrates.  Same sums in the same order: bit-identical. */
#define NB_PHASE_LET_WALK_OWN 6
int nb_sim_let_set_owners(nb_sim *sim, const unsigned long long *splits, int world, float ref_bound,
                          uint32_t seg_cap);
int nb_sim_let_set_arrivals(nb_sim *sim, uint32_t stay, const uint32_t *counts, int world);

/* `Simulator::cleanup(&mut self)`, src/sims/mod.rs:87-89 (TreeSim resets its
 * arena, src/sims/tree.rs:363-365).  Host-side housekeeping that may overlap
 * the enqueued step.  No-op for the all-pairs simulator. */
int nb_sim_cleanup(nb_sim *sim);

/* `device.poll(wgpu::Maintain::Wait)`, src/runners/offline_headless.rs:43:
 * block until everything enqueued on the simulator's stream has finished. */
int nb_sim_wait(nb_sim *sim);

/* `Simulator::sim_params(&self) -> SimParams`, src/sims/mod.rs:85. */
int nb_sim_sim_params(const nb_sim *sim, nb_sim_params *out);

/* `Simulator::dest_particle_slice(&self)`, src/sims/mod.rs:84 -- with one
 * documented deviation: the reference's slice is the buffer the last step READ
 * (src/sims/naive.rs:164-166 after step_num += 1); this returns
 * the POST-step state.  Waits for the stream, converts the device SoA state
 * to the 40-byte AoS layout and copies dst[0 .. n).  On a sharded simulator
 * only position/mass are globally valid (after the caller's all-gather);
 * velocity/acceleration are filled for the rank's own range and zero
 * elsewhere. */
int nb_sim_read_particles(nb_sim *sim, nb_particle *dst, size_t n);

/* Overwrite the simulator state (checkpoint restore). */
int nb_sim_write_particles(nb_sim *sim, const nb_particle *src, size_t n);

/* TreeSim only: copy out the octree the LAST step built (node count via
 * *n_nodes; up to cap entries written), in the reference's node numbering
 * (allocation order of src/sims/tree.rs:461,517-519).  NB_ERR_UNSUPPORTED on
 * an all-pairs simulator. */
int nb_sim_read_tree(nb_sim *sim, nb_octant *dst, size_t cap, size_t *n_nodes, float *root_width);

/* Sharded use: the device pointer of the position/mass buffer the LAST encode
 * wrote (float4 per body: x, y, z, mass), this rank's byte offset and byte
 * length inside it, and the total length.  The caller all-gathers
 * [offset, offset+slice) of every rank in place. */
int nb_sim_exchange_region(nb_sim *sim, void **dev_ptr, size_t *offset_bytes, size_t *slice_bytes,
                           size_t *total_bytes);

/* Same, for simulators with several regions to exchange.  NaiveSim has one (positions/masses).
 * A sharded TreeSim (replicated tree, partitioned walk: every rank builds the identical octree
 * from the full state and walks only its range of the sorted bodies) has three: the new
 * positions/masses, velocities and accelerations of its range -- the next step re-sorts all
 * bodies, so all three must reach every rank.  index in [0, count). */
int nb_sim_exchange_count(nb_sim *sim, int *count);
int nb_sim_exchange_region_i(nb_sim *sim, int index, void **dev_ptr, size_t *offset_bytes,
                             size_t *slice_bytes, size_t *total_bytes);

/* Step counter (`step_num`, src/sims/naive.rs:160). */
int nb_sim_step_num(const nb_sim *sim, uint64_t *out);

/* Time the next `n` encodes with HIP events on the simulator's own stream:
 * enqueue n steps back to back, wait, and report the total in *ms_total and
 * the mean duration of the dominant force kernel in *ms_kernel (events
 * bracket that launch alone).  Used by bench.py for `roofline.achieved`. */
int nb_sim_encode_n_timed(nb_sim *sim, int n, float *ms_total, float *ms_kernel);

/* Tuning knobs with no reference counterpart.  key "naive_variant": index into the
 * all-pairs kernel variant table (tiling / packing choices of nb_naive.hip; every variant
 * computes the same step).  Also settable through the NB_NAIVE_VARIANT environment
 * variable at create time.  "naive_jsplit": j-splits across workgroups (0 = automatic).
 * "naive_mass_runs": 1 (default) sums runs of equal masses without the per-pair mass
 * multiply and applies the mass once per run; 0 multiplies every pair (bitwise the same
 * step when the masses are one power of two, a different rounding of the sum otherwise).
 * A TreeSim's keys ("tree_*": bodies per wave of the walk, sort
 * passes and fix-up, who gathers the velocities, where the tile scan runs, ...) are listed
 * in the table of TreeSim::set_tuning (nb_tree.hip), one row per key with the values it accepts;
 * the defaults are the initialisers of the members the rows point to: speed only -- every setting
 * computes the same step, bit for bit where the tests say so. */
int nb_sim_set_tuning(nb_sim *sim, const char *key, int value);
int nb_naive_variant_count(void);
const char *nb_naive_variant_name(int variant);

/* Testing hook: copy a named internal device buffer to the host (e.g. TreeSim "order": the
 * source index of the body at each sorted position, u32 x N; "counters": walk visit/accept
 * counts, u64 x 4; "status": u32 x 4).  *bytes receives the buffer's length. */
int nb_sim_debug_buffer(nb_sim *sim, const char *name, void *dst, size_t cap, size_t *bytes);

/* ------------------------------------------------------------------------- */
/* Diagnostics -- conserved-quantity monitor (no reference counterpart: the   */
/* reference has no way to measure a run's energy or momentum)                */
/* ------------------------------------------------------------------------- */
/* Computed on the device for the state nb_sim_read_particles would return
 * (the post-step state; step 0 = the initial state), in fp64 from the fp32
 * state.  Sums over bodies, about the origin:
 *   mass              M = sum m
 *   com[3]            sum m x / M (NaN when M is 0)
 *   momentum[3]       P = sum m v
 *   angular_momentum  L = sum m (x cross v)
 *   kinetic           K = sum m |v|^2 / 2
 *   max_speed         max |v|
 *   nonfinite         bodies with any non-finite position, velocity or mass
 *                     component; they are left out of every sum (and of W)
 * With NB_DIAG_POTENTIAL, over all pairs i < j (O(N^2), exact, no theta):
 *   pair_sum          W = sum m_i m_j psi(r_ij), with the potential of the
 *                     reference's pair force m_j g / (r^3 + e) (naive.wgsl:23-48):
 *                       psi(r) = integral_r^inf ds / (s^3 + e)
 *                              = atan2(sqrt3 a, 2r - a) / (sqrt3 a^2)
 *                                - log1p(3ar / (r^2 - ar + a^2)) / (6a^2),  a = e^(1/3)
 *                     (psi(0) = 2 pi / (3 sqrt3 a^2) is finite; psi(r) -> 1/(2r^2))
 *   potential         U = -g dt W (the stored acceleration is sum(f) dt: the
 *                     coupling is g dt, naive.wgsl:41)
 *   total             E = K + U
 * Without the flag these three are NaN.  E is a MONITOR, not an invariant:
 * the reference evaluates body i's drifted position against body j's old one
 * (SURVEY A6), so neither E nor P is conserved exactly by the integrator.
 * Coincident distinct bodies each add psi(0); with e = 0 they make W = +inf.
 * The sums run in a fixed order without float atomics: two calls on one state
 * return bit-identical structs.  The call is ordered after the enqueued steps
 * on the simulator's stream, ends with one synchronisation, reports a TreeSim's
 * status words as nb_sim_read_particles does, and does not change the
 * trajectory.  The pair pass is split into launches of bounded length. */
#define NB_DIAG_MOMENTS 1u   /* always computed */
#define NB_DIAG_POTENTIAL 2u /* add the O(N^2) pair potential */

typedef struct nb_diagnostics {
    uint64_t step_num;  /* the step the measured state is the result of */
    uint64_t n;         /* bodies measured */
    uint64_t nonfinite;
    double mass;
    double com[3];
    double momentum[3];
    double angular_momentum[3];
    double kinetic;
    double max_speed;
    double pair_sum;  /* W (NaN without NB_DIAG_POTENTIAL) */
    double potential; /* U = -g dt W */
    double total;     /* E = kinetic + potential */
    uint32_t flags;   /* what was computed (NB_DIAG_MOMENTS | requested bits) */
    uint32_t reserved;
} nb_diagnostics;

/* Diagnostics of a simulator (no reference counterpart).  flags: any
 * combination of NB_DIAG_* (0 = moments only).  NB_ERR_INVALID for a null
 * argument, unknown flag bits or NB_DIAG_POTENTIAL with e < 0;
 * NB_ERR_UNSUPPORTED for a sharded simulator (placement world > 1). */
int nb_sim_diagnostics(nb_sim *sim, uint32_t flags, nb_diagnostics *out);

/* ------------------------------------------------------------------------- */
/* Radial profiles -- per-shell mass and velocity moments (no reference       */
/* counterpart: the reference has no way to measure a run's structure)        */
/* ------------------------------------------------------------------------- */
/* Bins the state nb_sim_read_particles would return by distance from a centre
 * (spherical shells) or from an axis through it (NB_RADIAL_CYLINDRICAL: annuli
 * of a disc), on the device, in one streaming pass over 32 B per body.  The
 * rule, which DESIGN.md 6d states in full: everything in binary64 from the
 * binary32 state, one rounding per operation, no contraction, in this order,
 * per body with position x, velocity v, mass m:
 *   d = (double)x - c, u = (double)v - v_c       (c, v_c: centre and its velocity)
 *   spherical    r2 = (dx dx + dy dy) + dz dz
 *   cylindrical  h = (dx nx + dy ny) + dz nz, p = d - h n, r2 = (px px + py py) + pz pz
 *                (n = axis / sqrt((ax ax + ay ay) + az az), formed on the host)
 *   bin          the k with edges[k]^2 <= r2 < edges[k+1]^2, the squares formed
 *                once in fp64 on the host; the comparison is on r2 -- no sqrt, log
 *                or division decides a bin, so the counts are exact integers.
 *                r2 < edges[0]^2: `inside`; r2 >= edges[nbins]^2: `outside`
 *   r = sqrt(r2); with q = d (spherical) or p (cylindrical):
 *                u_r = ((qx ux + qy uy) + qz uz) / r
 *                u_phi = ((nx wx + ny wy) + nz wz) / r, w = p cross u (cylindrical; 0 in
 *                spherical mode); u_r = u_phi = 0 when r = 0
 *   ang          m (d cross u), the full d in both modes; shape: m d_i d_j
 * A body with any non-finite position, velocity or mass component is `nonfinite`
 * and left out of everything (the predicate of nb_sim_diagnostics).
 * inside_count + sum of count + outside_count + nonfinite == n.
 * NB_RADIAL_CENTER_COM: c and v_c are the fp64 `com` and `momentum / mass` that
 * nb_sim_diagnostics returns for the same state, bit for bit (the same moments
 * pass runs ahead of the binning on the stream; no host round trip between them).
 * The sums run in a fixed order without float atomics and the grid shapes depend
 * on n and nbins alone: two calls on one state return bit-identical structs.  The
 * call is ordered after the enqueued steps on the simulator's stream, ends with
 * one synchronisation, reports a TreeSim's status words as nb_sim_read_particles
 * does, and does not change the trajectory. */
#define NB_RADIAL_MAX_BINS 256u
#define NB_RADIAL_CYLINDRICAL 1u /* radius = distance from the axis through the centre; default: from the centre */
#define NB_RADIAL_CENTER_COM 2u  /* centre = centre of mass, centre velocity = P/M of the measured state */

typedef struct nb_radial_params {
    uint32_t nbins, flags; /* 1..NB_RADIAL_MAX_BINS */
    double center[3];      /* ignored with NB_RADIAL_CENTER_COM */
    double velocity[3];    /* ignored with NB_RADIAL_CENTER_COM */
    double axis[3];        /* cylindrical only; any non-zero finite vector, normalised in fp64 */
    const double *edges;   /* nbins + 1 finite radii, edges[0] >= 0, strictly ascending */
} nb_radial_params;

typedef struct nb_radial_bin { /* 88 bytes */
    uint64_t count;
    double mass;    /* sum m */
    double m_r;     /* sum m r            (mass-weighted mean radius = m_r / mass) */
    double m_ur;    /* sum m u_r */
    double m_ur2;   /* sum m u_r^2 */
    double m_uphi;  /* sum m u_phi        (cylindrical; 0 in spherical mode) */
    double m_uphi2; /* sum m u_phi^2      (cylindrical; 0 in spherical mode) */
    double m_u2;    /* sum m |u|^2 */
    double ang[3];  /* sum m (d x u) */
} nb_radial_bin;

typedef struct nb_radial_profile {
    uint64_t step_num, n, nonfinite;
    uint64_t inside_count, outside_count;   /* r < edges[0];  r >= edges[nbins] */
    double inside_mass, outside_mass;
    double mass;                            /* all finite bodies */
    double center[3], velocity[3], axis[3]; /* the values used (axis normalised; 0 in spherical mode) */
    double shape[6];                        /* sum m d_i d_j (xx,yy,zz,xy,xz,yz) over bodies with r < edges[nbins] */
    uint32_t nbins, flags;
} nb_radial_profile;

/* The profile of a simulator's current state: out and bins[0 .. nbins).  NB_ERR_INVALID for a null
 * pointer, nbins outside 1..NB_RADIAL_MAX_BINS, unknown flag bits, non-finite, negative or
 * non-ascending edges, a non-finite centre, velocity or axis, or (cylindrical) a zero axis -- all
 * checked before any device call; NB_ERR_UNSUPPORTED for a sharded simulator (placement world > 1). */
int nb_sim_radial_profile(nb_sim *sim, const nb_radial_params *params, nb_radial_profile *out,
                          nb_radial_bin *bins);
/* Host only, no device.  nbins + 1 edges from rmin to rmax with a constant ratio (log; rmin > 0) or a
 * constant step (linear; rmin >= 0): edges[0] == rmin and edges[nbins] == rmax exactly.
 * NB_ERR_INVALID for a null pointer, nbins outside 1..NB_RADIAL_MAX_BINS, non-finite bounds,
 * rmax <= rmin, or edges that do not come out strictly ascending. */
int nb_radial_edges_log(double rmin, double rmax, uint32_t nbins, double *edges);
int nb_radial_edges_linear(double rmin, double rmax, uint32_t nbins, double *edges);
/* Host only, a pure function of its arguments: for each fraction f in (0, 1), radii[i] = the radius
 * where the cumulative mass (inside_mass, then the bins in order) reaches f * p->mass, linear in r
 * inside the bin that crosses; NaN where the crossing lies in `inside` or `outside` (or f is not in
 * (0, 1)).  Binned, so limited by the bins' resolution.  edges: the p->nbins + 1 radii of the call. */
int nb_radial_lagrangian(const nb_radial_profile *p, const nb_radial_bin *bins, const double *edges,
                         const double *fractions, uint32_t k, double *radii);

/* ------------------------------------------------------------------------- */
/* Field probes -- exact acceleration and potential at arbitrary points (no   */
/* reference counterpart: the reference evaluates its force law at bodies only)*/
/* ------------------------------------------------------------------------- */
/* The all-pairs force law of the step and its potential, summed on the device
 * over the state nb_sim_read_particles would return, at m points that need not
 * be bodies.  The rule, which DESIGN.md 6e states in full.  The sums run over
 * exactly the bodies nb_sim_diagnostics counts as finite; a body with any
 * non-finite position, velocity or mass component is left out and reported in
 * stats.nonfinite.  For a point p (three fp32 coordinates) and body j, in fp32:
 *   d = x_j - p,  r2 = dx dx + dy dy + dz dz,  r = sqrt(r2),  g = params.g, e = params.e
 *   coincident   r2 == 0 (in practice: the same coordinates).  Such a body adds
 *                nothing to either sum and is counted in the sample's `coincident`:
 *                the field at a body's own position is the field of the others,
 *                which is the step's self-exclusion by index whenever no two
 *                distinct bodies coincide
 *   acc          g sum_j m_j d / (r^4 + e r): the reference's pair force
 *                m g / (r^3 + e) * d / r (naive.wgsl:38-39) without the dt that the
 *                stored Particle.acceleration carries (stored = acc * dt)
 *   potential    -g sum_j m_j psi(r), psi as in "Diagnostics" above; then
 *                diagnostics.potential == (dt / 2) sum_i m_i potential(x_i) up to
 *                rounding whenever no two distinct bodies coincide
 * Arithmetic: the per-pair terms in fp32 with the step's 1-ulp sqrt and reciprocal;
 * runs of at most 64 consecutive bodies summed in fp32; each run folded into an
 * fp64 sum; the partial sums of the body chunks added in fp64 in a fixed order;
 * the result multiplied once by (double)g.  Against the same sums in binary64 a
 * component of acc is within 80 * 2^-24 * g sum_j m_j |d_k| / (r^4 + e r), and
 * the potential within 5e-6 * g sum_j |m_j| psi(r).
 * No float atomics, and the grid and the chunking are functions of (m, n, flags)
 * alone: two calls return bit-identical samples, and a point's sample does not
 * depend on its place in the array (permuting the points permutes the samples
 * bit for bit).  The last bits may differ between calls with different m or
 * different flags.
 * A point with a non-finite coordinate gets NaN in every requested field
 * (coincident 0) and is counted in stats.nonfinite_points; fields not requested
 * are NaN; n = 0 gives zeros; m = 0 is valid, only synchronises, and measures
 * nothing (stats.nonfinite is 0).  The call is ordered after the enqueued steps
 * on the simulator's stream, ends with one synchronisation, reports a TreeSim's
 * status words as nb_sim_read_particles does, and does not change the
 * trajectory.  The points go in bands, one launch per band of at most 2^35 pairs
 * ("field_launch_pairs_log2", nb_sim_set_tuning, 16..40: speed and testing only,
 * identical samples). */
#define NB_FIELD_ACCEL 1u
#define NB_FIELD_POTENTIAL 2u
#define NB_FIELD_MAX_POINTS (1u << 24)

typedef struct nb_field_sample { /* 40 bytes */
    double acc[3];
    double potential;
    uint32_t coincident; /* bodies at the point itself (left out of both sums) */
    uint32_t reserved;
} nb_field_sample;

typedef struct nb_field_stats {
    uint64_t step_num; /* the step the measured state is the result of */
    uint64_t n;        /* bodies of the simulator */
    uint64_t nonfinite;
    uint64_t points, nonfinite_points;
    uint32_t flags;    /* what was computed */
    uint32_t launches; /* bands */
} nb_field_stats;

/* The field of a simulator's current state at `points` (3 floats per point) into out[0 .. m).
 * flags: NB_FIELD_ACCEL, NB_FIELD_POTENTIAL or both.  stats may be null.  NB_ERR_INVALID for a null
 * handle, null points or out with m > 0, flags zero or with unknown bits, m > NB_FIELD_MAX_POINTS, or
 * NB_FIELD_POTENTIAL with e < 0 -- all checked before any device call; NB_ERR_UNSUPPORTED for a sharded
 * simulator (placement world > 1). */
int nb_sim_field(nb_sim *sim, const float *points, size_t m, uint32_t flags, nb_field_sample *out,
                 nb_field_stats *stats);
/* Host only, no device: k * n_phi points on k rings about `axis` through `center`, for a rotation curve.
 * Ring i, azimuth q is points[3 (i n_phi + q)] = c + R_i (cos(2 pi q / n_phi) e1 + sin(2 pi q / n_phi) e2),
 * formed in fp64 and rounded once.  n = axis normalised in fp64; e1 = the coordinate axis of the smallest
 * |n_k| (the lowest index on ties), made orthogonal to n and normalised; e2 = n cross e1.
 * NB_ERR_INVALID for a null pointer, a zero or non-finite axis, a non-finite centre, negative or
 * non-finite radii, or n_phi = 0. */
int nb_field_rings(const double center[3], const double axis[3], const double *radii, uint32_t k, uint32_t n_phi,
                   float *points);
typedef struct nb_field_ring { /* means over the n_phi samples of one ring */
    double a_R;       /* acc . rhat, rhat the unit vector from the axis to the fp32 point actually used */
    double a_n;       /* acc . n */
    double potential;
    double v_c;       /* sqrt(max(0, -R_i a_R)): the circular velocity */
} nb_field_ring;
/* Host only, a pure function of its arguments: the ring means of `samples` taken at the `points`
 * nb_field_rings wrote for the same center, axis, radii, k and n_phi.  A point on the axis has no rhat
 * and adds 0 to a_R.  Refusals as nb_field_rings, and null samples or out. */
int nb_field_ring_means(const double center[3], const double axis[3], const double *radii, uint32_t k,
                        uint32_t n_phi, const float *points, const nb_field_sample *samples, nb_field_ring *out);

/* ------------------------------------------------------------------------- */
/* Tidal tensor probes -- the exact gradient of the field at arbitrary points, */
/* and a disc's epicyclic and vertical frequencies from it (no reference       */
/* counterpart)                                                                */
/* ------------------------------------------------------------------------- */
/* T_ab = d acc_a / d x_b of the field above, summed pair by pair on the device as
 * the field is -- differencing nb_sim_field cannot resolve it: the points and the
 * pair terms are fp32, and a step small enough for a cored law is below the
 * rounding of the difference.  The rule, which DESIGN.md 6r states in full.  The
 * bodies, d, r2, r, g, e and `coincident` are those of "Field probes": the sums run
 * over the bodies nb_sim_diagnostics counts as finite, and a body with r2 == 0 adds
 * nothing and is counted.  Differentiating acc = g sum_j m_j d / (r^4 + e r) by p:
 *   w_j  = m_j / (r^4 + e r)                 (the field's own pair weight)
 *   c_j  = (4 r^3 + e) / (r^2 (r^3 + e))
 *   S_ab = sum_j w_j c_j d_a d_b             (six sums: xx, yy, zz, xy, xz, yz)
 *   W    = sum_j w_j
 *   T_ab = g (S_ab - delta_ab W)             (symmetric by construction)
 * The trace is g sum_j m_j (r^3 - 2 e) / (r (r^3 + e)^2): not zero, because the
 * reference's force is m / (r^3 + e).  No psi is involved: any e is accepted (the
 * error bound below is derived for e >= 0).
 * Arithmetic, in fp32 per pair, every operation rounded once (no contraction):
 *   den = fma(e, r, r2 r2), w = rcp(den) m_j            (v_sqrt_f32, v_rcp_f32: 1 ulp)
 *   r3 = r2 r, c = fma(4, r3, e) rcp(r2 (r3 + e)), wc = w c
 *   t_a = wc d_a;  S_ab += fma(t_a, d_b, .) with a <= b;  W += w
 * The range of the form is narrower than the field's.  A body whose r3 is not an
 * fp32 number (r > 6.9e12) adds 0 to every sum (its w has underflowed already; the
 * true term is below 2e-51 m_j).  A pair so close that w c exceeds fp32 -- about
 * r^3 < m_j / (e 3e38), or r < (4 m_j / 3e38)^(1/6) for e = 0 -- gives inf or NaN
 * in the sample: such a point is, to fp32, on the body, and outside the bound.
 * Runs of exactly 64 consecutive bodies are summed in fp32; each run is folded into
 * an fp64 sum; the waves and then the body chunks are added in fp64 in a fixed
 * order; S_aa - W is formed once, in fp64, after all of that, so a diagonal
 * element never cancels per pair; the result is multiplied once by (double)g.
 * Against the same sums in binary64 each of the seven sums is within
 *   (64 + NB_TIDAL_K) 2^-24 g sum_j |term_j|,    NB_TIDAL_K = 33,
 * and a diagonal T_aa within the sum of the bounds of S_aa and W.  K counts the
 * roundings of the pair form above weighted by how often each enters a term, to
 * first order and for e >= 0 (DESIGN.md 6r derives it).
 * No float atomics, and the grid and the chunking are functions of (m, n) alone:
 * two calls return bit-identical samples, and a point's sample does not depend on
 * its place in the array.  A point with a non-finite coordinate gets NaN (coincident
 * 0) and is counted in stats.nonfinite_points; n = 0 gives zeros; m = 0 is valid,
 * only synchronises and measures nothing.  The call is ordered after the enqueued
 * steps on the simulator's stream, ends with one synchronisation, reports a
 * TreeSim's status words as nb_sim_read_particles does, and does not change the
 * trajectory.  The points go in bands as nb_sim_field's do, bounded by the same
 * "field_launch_pairs_log2" (speed and testing only, identical samples).
 * A Toomre Q or a Jacobi radius would assume a 1/r^2 force and are not offered. */
#define NB_TIDAL_K 33u

typedef struct nb_tidal_sample { /* 56 bytes */
    double tensor[6];    /* xx, yy, zz, xy, xz, yz */
    uint32_t coincident; /* bodies at the point itself (left out of every sum) */
    uint32_t reserved;
} nb_tidal_sample;

typedef nb_field_stats nb_tidal_stats; /* the same fields; flags is 0 */

/* The tidal tensor of a simulator's current state at `points` (3 floats per point) into out[0 .. m).
 * stats may be null.  NB_ERR_INVALID for a null handle, null points or out with m > 0, or
 * m > NB_FIELD_MAX_POINTS -- all checked before any device call; NB_ERR_UNSUPPORTED for a sharded
 * simulator (placement world > 1).  Eigenvalues: nb_shape_eigen of (xx, xy, xz, yy, yz, zz). */
int nb_tidal_sim(nb_sim *sim, const float *points, size_t m, nb_tidal_sample *out, nb_tidal_stats *stats);
typedef struct nb_tidal_ring { /* means over the n_phi samples of one ring, and what follows from them */
    double t_RR;   /* rhat . T rhat, rhat the unit vector from the axis to the fp32 point actually used */
    double t_pp;   /* phihat . T phihat, phihat = n cross rhat */
    double t_nn;   /* n . T n */
    double t_Rn;   /* rhat . T n */
    double omega2; /* -a_R / R_i of the field's ring row (NaN for R_i = 0) */
    double kappa2; /* -t_RR + 3 omega2: R dOmega^2/dR + 4 Omega^2, for any central force law */
    double nu2;    /* -t_nn */
} nb_tidal_ring;
/* Host only, a pure function of its arguments: the ring means of the tidal `samples` taken at the `points`
 * nb_field_rings wrote for the same center, axis, radii, k and n_phi, in the frame of nb_field_ring_means, and
 * the squared frequencies with a_R from `rings`, the rows nb_field_ring_means gave for the field at the same
 * points.  A point on the axis has no rhat and adds 0 to t_RR, t_pp and t_Rn.  Refusals as nb_field_rings, and
 * null samples, rings or out. */
int nb_tidal_ring_means(const double center[3], const double axis[3], const double *radii, uint32_t k,
                        uint32_t n_phi, const float *points, const nb_tidal_sample *samples,
                        const nb_field_ring *rings, nb_tidal_ring *out);

/* ------------------------------------------------------------------------- */
/* Orbits -- test particles in the frozen field of the current state, at rest  */
/* or rotating rigidly at a pattern speed (no reference counterpart)           */
/* ------------------------------------------------------------------------- */
/* m massless tracers are integrated for `steps` leapfrog steps in the field of
 * "Field probes" above, sampled from the state nb_sim_read_particles would return
 * and frozen there: the bodies do not move, and with omega != 0 their frozen
 * pattern turns rigidly about `axis` through `center` at the pattern speed omega
 * (nb_disc_modes_derive's).  The tracers stay on the device between the force
 * evaluations and every step is enqueued up front; the call ends with one
 * synchronisation.  Orbit families of a bar, surfaces of section, trapping at
 * corotation and the Jacobi integral as a quality check are read from the
 * records.  The rule, which DESIGN.md 6t states in full.
 * Everything outside the field sample is binary64 +, -, x, each rounded once, no
 * contraction.  (e1, e2, n) = nb_map_frame(axis); c = center; h = dt / 2;
 * (C_k, S_k) = nb_orbit_phase(omega, dt, step0 + k): the cosine and sine of
 * theta_k = omega * ((double)(step0 + k) * dt), computed on the host by the C
 * library and handed to the device by value; omega == 0 gives exactly (1, 0).
 * Evaluation k of a tracer at x (tracers move in the inertial frame; the field is
 * sampled at the point the frozen pattern has under x):
 *   omega == 0   q = x
 *   otherwise    d = x - c
 *                a = (dx e1x + dy e1y) + dz e1z,  b and l likewise with e2 and n
 *                a' = a C_k + b S_k,  b' = b C_k - a S_k         (turned by -theta_k)
 *                q_i = c_i + ((a' e1_i + b' e2_i) + l n_i)
 *   p = (float)q, component by component
 *   sample       nb_sim_field's at p, bit for bit, for the m points of the call's
 *                tracers and flags F_k = NB_FIELD_ACCEL | NB_FIELD_POTENTIAL when
 *                NB_ORBIT_ENERGY is set and state k is recorded, NB_FIELD_ACCEL
 *                otherwise: the same points per lane, plan, chunk order and x g
 *   A_snap = accel_scale * sample.acc,  Phi = accel_scale * sample.potential
 *   omega == 0   A = A_snap
 *   otherwise    u = (Ax e1x + Ay e1y) + Az e1z,  v and t likewise with e2 and n
 *                u' = u C_k - v S_k,  v' = v C_k + u S_k         (turned by +theta_k)
 *                A_i = (u' e1_i + v' e2_i) + t n_i
 * Integrator, kick-drift-kick with one evaluation per step and one at the start:
 *   w = v_k + A_k h,   x_{k+1} = x_k + w dt,   v_{k+1} = w + A_{k+1} h
 * each component as one multiply and one add.  State k has time
 * t_k = (double)(step0 + k) * dt.
 * A state is recorded at k = 0, every, 2 every, ... and at k = steps;
 * nb_orbit_records(steps, every) is their number R, and record r of tracer i is
 * tracks[r * m + i]: x_k, v_k, and with NB_ORBIT_ENERGY
 *   potential = Phi_k
 *   energy    = (0.5 ((vx vx + vy vy) + vz vz) + Phi) - omega (n . ((x - c) x v)),
 *               the last term as  L = (n_x (dy vz - dz vy) + n_y (dz vx - dx vz))
 *               + n_z (dx vy - dy vx),  d = x - c, and omega L subtracted; with
 *               omega == 0 it is not formed.  With omega != 0 this is the Jacobi
 *               integral, conserved to the integrator's order; the plain energy
 *               is not.
 * Without NB_ORBIT_ENERGY potential and energy are NaN.
 * coincident[i] sums the samples' coincident counts over the steps + 1
 * evaluations of tracer i.  A tracer that starts with a non-finite coordinate or
 * velocity has NaN in every field of every record and is counted in
 * stats.nonfinite_tracers; one that becomes non-finite (its point no longer an
 * fp32 number included) is NaN from there on through the field's rule for
 * non-finite points; the other tracers keep their bits.  Non-finite bodies are
 * left out and counted in stats.nonfinite as by nb_sim_field.  n = 0 gives
 * straight lines.  m = 0 is valid and only synchronises.
 * Consequences: two calls return the same bits; permuting the tracers permutes
 * the tracks; "field_launch_pairs_log2" partitions the tracers into bands
 * (stats.pair_launches counts the pair launches) and cannot change a bit; and a run
 * of 2 S steps equals a run of S steps followed by a run of S steps from the first
 * run's last record with step0 + S, bit for bit, whenever S is a multiple of
 * `every` (state S is then recorded by all three runs, so every evaluation has
 * the same flags in the whole run and in its half).
 * The call does not change the trajectory and reports a TreeSim's status words as
 * nb_sim_read_particles does. */
#define NB_ORBIT_ENERGY 1u
#define NB_ORBIT_MAX_TRACERS (1u << 20)
#define NB_ORBIT_MAX_STEPS (1u << 20)
#define NB_ORBIT_MAX_SAMPLES (1u << 22) /* records * tracers */
#define NB_ORBIT_MAX_PAIRS_LOG2 44      /* padded tracers * n * (steps + 1) */

typedef struct nb_orbit_params {
    double dt;      /* finite, non-zero; negative integrates backwards */
    uint64_t step0; /* number of the first state: time t_k = (double)(step0 + k) * dt */
    uint32_t steps, every, flags, reserved;
    double accel_scale; /* acceleration = accel_scale * nb_sim_field's; finite */
    double omega;       /* pattern speed about `axis` through `center`; 0: no rotation */
    double axis[3], center[3];
} nb_orbit_params;

typedef struct nb_orbit_sample { /* 64 bytes */
    double pos[3], vel[3], potential, energy;
} nb_orbit_sample;

typedef struct nb_orbit_stats {
    uint64_t step_num; /* the step the measured state is the result of */
    uint64_t n;        /* bodies of the simulator */
    uint64_t nonfinite;
    uint64_t tracers, nonfinite_tracers;
    uint32_t records, pair_launches, flags, reserved;
} nb_orbit_stats;

/* The orbits of m tracers from pos, vel (3 doubles per tracer) in the field of a simulator's current state
 * into tracks[0 .. records * m), record-major.  coincident ([m]) and stats may be null.  NB_ERR_INVALID for a
 * null handle or params, null pos, vel or tracks with m > 0, steps = 0 or above NB_ORBIT_MAX_STEPS, every = 0,
 * unknown flag bits or reserved != 0, m > NB_ORBIT_MAX_TRACERS, records * m > NB_ORBIT_MAX_SAMPLES, a dt or
 * accel_scale that is not finite, dt = 0, a non-finite omega or center, with omega != 0 a zero or non-finite
 * axis, or NB_ORBIT_ENERGY with e < 0 -- all checked before any device call; NB_ERR_UNSUPPORTED for a sharded
 * simulator (placement world > 1) and for a call above 2^NB_ORBIT_MAX_PAIRS_LOG2 pairs, which the caller
 * splits: step0 makes the split exact.  No single launch exceeds the budget of "field_launch_pairs_log2". */
int nb_orbits_sim(nb_sim *sim, const nb_orbit_params *params, const double *pos, const double *vel, size_t m,
                  nb_orbit_sample *tracks, uint32_t *coincident, nb_orbit_stats *stats);
/* Host only: the number of recorded states, steps / every + 1 and one more when every does not divide steps;
 * 0 for every = 0. */
uint32_t nb_orbit_records(uint32_t steps, uint32_t every);
/* Host only: *c, *s = cos, sin of omega * ((double)k * dt) by the C library; exactly (1, 0) for omega == 0.
 * NB_ERR_INVALID for a null pointer or a non-finite omega or dt. */
int nb_orbit_phase(double omega, double dt, uint64_t k, double *c, double *s);

/* ------------------------------------------------------------------------- */
/* Orbit sections -- the crossings of a plane and a running summary per tracer, */
/* taken by the orbit's own step kernel (no reference counterpart)             */
/* ------------------------------------------------------------------------- */
/* nb_orbit_sections_sim is nb_orbits_sim -- the same tracers, states, records, pair launches and bits -- whose
 * step kernel also looks at every consecutive pair of states: it stores the states interpolated onto a plane of
 * the pattern frame (a surface of section) and keeps a fixed-size summary per tracer (peri- and apocentres,
 * extrema, windings), so that neither needs a recorded state.  The rule, which DESIGN.md 6v states in full.
 * Everything is binary64 +, -, x and one /, each rounded once, no contraction; the only comparisons are < and >=.
 * State k is (x_k, v_k) of "Orbits"; (e1, e2, n) = nb_map_frame(axis), formed for omega == 0 too; c = center;
 * (C_k, S_k) = nb_orbit_phase(omega, dt, step0 + k).
 * Pattern-frame state of state k:
 *   d = x_k - c
 *   a = (dx e1x + dy e1y) + dz e1z,  b and l likewise with e2 and n
 *   a' = a C_k + b S_k,  b' = b C_k - a S_k            (omega == 0: the same lines with (1, 0))
 *   xi_k = (a', b', l)
 *   u = (vx e1x + vy e1y) + vz e1z,  v and t likewise with e2 and n     (v_k in the frame)
 *   u' = u C_k + v S_k,  v' = v C_k - u S_k
 *   eta_k = (u' + omega b', v' - omega a', t)          (omega == 0: (u', v', t), the omega terms not formed)
 * Scalars of state k, normal = (N_a, N_b, N_l) given in the pattern frame:
 *   s_k = ((N_a a' + N_b b') + N_l l) - offset
 *   D_k = (dx vx + dy vy) + dz vz
 *   L_k = (n_x (dy vz - dz vy) + n_y (dz vx - dx vz)) + n_z (dx vy - dy vx)       (the L of "Orbits")
 *   r2 = (a' a' + b' b') + l l,   R2 = a' a' + b' b'
 * Sign change of a scalar y over the bracket (k, k+1), the one test used everywhere:
 *   up    y_k < 0 and y_{k+1} >= 0
 *   down  y_k >= 0 and y_{k+1} < 0
 * so ups and downs alternate strictly, a NaN triggers neither, and y_k - y_{k+1} is not 0 when one fires.
 * Section crossing: bracket (k, k+1) crosses on an up of s if direction >= 0 and on a down of s if
 * direction <= 0.  f = s_k / (s_k - s_{k+1}), and the record is
 *   xi[i]  = xi_k[i] + f (xi_{k+1}[i] - xi_k[i]),   eta[i] likewise
 *   time   = (double)(step0 + k) * dt + f * dt,     step = step0 + k
 * Linear interpolation, on purpose: its error is (Omega dt)^2 / 8 of the orbit's scale, the leapfrog's own order.
 * Tracer i stores its first max_crossings records at crossings[i * max_crossings + j] in time order; counts[i]
 * is the number of all its crossings, stored or not; slots never written are zero bytes.
 * Summary of tracer i, over the states 0 .. steps and the brackets 0 .. steps - 1:
 *   r2_min, r2_max, R2_min, R2_max, lz_min, lz_max of r2, R2 and L; h_max of |l|.  They start at +inf (minima)
 *   and -inf (maxima, h_max) and are replaced on  y < min  or  y > max, so a NaN state leaves them alone.
 *   pericentres = ups of D, apocentres = downs of D, plane_ups = ups of l;
 *   first_peri, last_peri = step0 + k + 1 of the first and last bracket with an up of D, UINT64_MAX for none;
 *   winding_pattern  +1 on an up of b' and -1 on a down of b' whose interpolated a' is > 0:
 *                    a'_k + f_b (a'_{k+1} - a'_k),  f_b = b'_k / (b'_k - b'_{k+1});
 *   winding_inertial the same on the unturned (a, b).
 * A tracer that is non-finite has no crossings and untouched extrema; the others keep their bits.
 * Consequences: besides those of "Orbits", a run of 2 S steps equals a run of S steps followed by one of S steps
 * from the first run's last record with step0 + S whenever S is a multiple of `every`: the counts add, the stored
 * crossings concatenate (given room), and the summaries combine by nb_orbit_summary_merge.  Bracket (S-1, S)
 * belongs to the first run and (S, S+1) to the second; state S is in both, which the extrema do not notice.
 * No launch is added: stats.orbit.pair_launches and the step launches are those of nb_orbits_sim. */
#define NB_ORBIT_SECTION_MAX_CROSSINGS (1u << 22) /* m * max_crossings */
#define NB_ORBIT_NO_STEP UINT64_MAX

typedef struct nb_orbit_section_params {
    double normal[3];       /* (N_a, N_b, N_l) in the pattern frame; finite, not all zero; need not be a unit vector */
    double offset;          /* the plane is N . xi = offset; finite */
    int32_t direction;      /* +1: ups of s, -1: downs, 0: both */
    uint32_t max_crossings; /* stored per tracer */
    uint32_t flags, reserved; /* both 0 */
} nb_orbit_section_params;

typedef struct nb_orbit_crossing { /* 64 bytes */
    double xi[3], eta[3], time;
    uint64_t step;
} nb_orbit_crossing;

typedef struct nb_orbit_summary { /* 96 bytes: 7 doubles at 0, 2 uint64 at 56, 6 32-bit words at 72 */
    double r2_min, r2_max, R2_min, R2_max, h_max, lz_min, lz_max;
    uint64_t first_peri, last_peri;
    uint32_t pericentres, apocentres, plane_ups;
    int32_t winding_pattern, winding_inertial;
    uint32_t reserved;
} nb_orbit_summary;

typedef struct nb_orbit_section_stats {
    nb_orbit_stats orbit;
    uint64_t crossings;  /* the sum of counts */
    uint64_t stored;     /* the sum of min(counts, max_crossings) */
    uint64_t overflowed; /* tracers with counts > max_crossings */
} nb_orbit_section_stats;

/* nb_orbits_sim with the section: tracks, its R = nb_orbit_records(steps, every) records and coincident are that
 * call's (a section run passes every = steps and gets the two end states); crossings is [m * max_crossings],
 * counts [m], summaries [m].  crossings, counts, summaries, coincident and stats may be null, except that null
 * crossings with max_crossings > 0 and m > 0 is invalid.  NB_ERR_INVALID for everything nb_orbits_sim refuses,
 * null section params, a non-finite or all-zero normal, a non-finite offset, a direction outside {-1, 0, 1},
 * section flags or reserved != 0, m * max_crossings > NB_ORBIT_SECTION_MAX_CROSSINGS, or a zero or non-finite
 * axis (the frame is needed for omega == 0 too) -- all checked before the handle is looked at; NB_ERR_UNSUPPORTED
 * as nb_orbits_sim. */
int nb_orbit_sections_sim(nb_sim *sim, const nb_orbit_params *params, const nb_orbit_section_params *section,
                          const double *pos, const double *vel, size_t m, nb_orbit_sample *tracks,
                          uint32_t *coincident, nb_orbit_crossing *crossings, uint32_t *counts,
                          nb_orbit_summary *summaries, nb_orbit_section_stats *stats);
/* Host only: the summary of a run followed by its continuation -- min of the minima, max of the maxima, the
 * counters and windings added, first_peri the first present (a's, else b's), last_peri the last present (b's,
 * else a's).  out may be a or b.  NB_ERR_INVALID for a null pointer. */
int nb_orbit_summary_merge(const nb_orbit_summary *a, const nb_orbit_summary *b, nb_orbit_summary *out);

/* ------------------------------------------------------------------------- */
/* Orbit stability -- deviation vectors carried by the tangent map of the     */
/* orbit's step, renormalised by exact powers of two (no reference counterpart) */
/* ------------------------------------------------------------------------- */
/* nb_orbit_stability_sim is nb_orbits_sim -- the same tracers, states, records and bits of the tracks -- whose pair
 * kernel also sums the tidal tensor at every evaluation point and whose step kernel moves D deviation vectors per
 * tracer, delta = (dx, dv), by the exact derivative of the step.  From their growth come the finite-time Lyapunov
 * exponent and the alignment indices SALI / GALI_2 (nb_orbit_stability_derive): regular or chaotic, without
 * differencing two orbits, whose separation would be below the fp32 rounding of the evaluation points.  The rule,
 * which DESIGN.md 6w derives.  Everything outside the sums is binary64 +, -, x, each rounded once, no contraction;
 * the scalings are ldexp; there is no division, square root or logarithm on the device.
 * (e1, e2, n), c, h = dt / 2 and (C_k, S_k) are those of "Orbits".  NB_ORBIT_ENERGY is refused: the tracks are
 * nb_orbits_sim's, which gives the energies.
 * Evaluation k of a tracer, at the fp32 point p of "Orbits":
 *   A_snap       as "Orbits" (flags NB_FIELD_ACCEL): nb_sim_field's acc at p bit for bit, x accel_scale
 *   tensor       nb_tidal_sim's at p, bit for bit, for the m points of the call's tracers: the same seven sums
 *                (S_xx, S_yy, S_zz, S_xy, S_xz, S_yz, W), points per lane, plan and chunk order, finished as that
 *                call finishes them -- g (S_aa - W) on the diagonal, g S_ab off it, NaN at a non-finite point
 *   T_snap = accel_scale * tensor, component by component (symmetric: T_ba = T_ab)
 * Kick of a deviation (dx, dv) at evaluation k:
 *   omega == 0   q = dx
 *   otherwise    a = (dx_x e1x + dx_y e1y) + dx_z e1z,  b and l likewise with e2 and n   (no centre)
 *                a' = a C_k + b S_k,  b' = b C_k - a S_k
 *                q_i = (a' e1_i + b' e2_i) + l n_i                                       (not rounded to fp32)
 *   t_a = (T_a0 q_0 + T_a1 q_1) + T_a2 q_2
 *   omega == 0   z = t;  otherwise z = t turned back by the three lines that turn A_snap back in "Orbits"
 *   kappa_i = z_i h
 * One evaluation, for every vector, in this order -- the lines the step runs for v and x:
 *   1. k > 0:      dv <- dv + kappa
 *   2. k >= 0:     mu = the largest |component| of the six.  If all six are finite and mu != 0:
 *                    E = frexp-exponent(mu) - 1       (2^E <= mu < 2^(E+1))
 *                    if log2 + E > peak_log2:  peak_log2 = log2 + E, peak_step = step0 + k
 *                    if k > 0 and |E| >= renorm_log2:  all six components AND kappa are multiplied by 2^-E (ldexp),
 *                      log2 <- log2 + E, renorms <- renorms + 1
 *                  kappa is scaled too because line 4 adds it again: only then is a renormalised run the
 *                  unrenormalised run times 2^log2 in every bit (as long as neither underflows or overflows).
 *   3. record, if state k is recorded: the six components and log2
 *   4. k < steps:  dv <- dv + kappa
 *   5. k < steps:  dx <- dx + dv dt
 * The vector a record stands for is d * 2^log2.  log2 starts at the caller's value; peak_log2 starts at INT64_MIN and
 * peak_step at NB_ORBIT_NO_STEP, renorms at 0, in every call.  A zero or non-finite vector is left alone.  The
 * vectors of a tracer that starts non-finite are NaN in every record; a tracer whose point becomes non-finite has
 * NaN vectors from there on (its T_snap is NaN); the other tracers keep their bits.  T_snap is nb_tidal_sim's in its
 * failures too: a body within a few 1e-9 of the point without coinciding with it overflows the tensor's fp32 pair
 * term there and here.
 * Records: devs[(r * m + i) * D + j] for record r (those of "Orbits"), tracer i, vector j; growth[i * D + j].
 * Consequences: those of "Orbits"; tracks and coincident are nb_orbits_sim's for the same arguments bit for bit; a
 * run of 2 S steps equals a run of S steps followed by one of S steps from the first run's last records (tracks and
 * devs, log2 included) with step0 + S, whenever S is a multiple of `every`; the pair launches are as many as
 * nb_orbits_sim's, each of this unit's pair kernel in the place of the field's. */
#define NB_ORBIT_MAX_DEVIATIONS 6u
#define NB_ORBIT_MAX_RENORM_LOG2 512u

typedef struct nb_orbit_stability_params {
    uint32_t deviations;  /* D, 1 .. NB_ORBIT_MAX_DEVIATIONS */
    uint32_t renorm_log2; /* 1 .. NB_ORBIT_MAX_RENORM_LOG2 */
    uint32_t reserved;    /* 0 */
} nb_orbit_stability_params;

typedef struct nb_orbit_deviation { /* 56 bytes */
    double d[6];  /* dx, dv */
    int64_t log2; /* the vector is d * 2^log2 */
} nb_orbit_deviation;

typedef struct nb_orbit_growth { /* 24 bytes */
    int64_t peak_log2;  /* the largest log2 + E over the states 0 .. steps; INT64_MIN for none */
    uint64_t peak_step; /* step0 + k of the first state that reached it; NB_ORBIT_NO_STEP for none */
    uint32_t renorms, reserved;
} nb_orbit_growth;

typedef struct nb_orbit_stability_stats {
    nb_orbit_stats orbit;
    uint64_t renorms; /* the sum over tracers and vectors */
    uint32_t deviations, renorm_log2;
} nb_orbit_stability_stats;

/* nb_orbits_sim with D deviation vectors per tracer from dev0 ([m * D]): tracks and coincident are that call's, devs
 * is [records * m * D], growth [m * D].  coincident, growth and stats may be null.  NB_ERR_INVALID for everything
 * nb_orbits_sim refuses, NB_ORBIT_ENERGY among the flags, null stability params, deviations outside
 * 1 .. NB_ORBIT_MAX_DEVIATIONS, renorm_log2 outside 1 .. NB_ORBIT_MAX_RENORM_LOG2, reserved != 0, null dev0 or devs with
 * m > 0, or records * m * D > NB_ORBIT_MAX_SAMPLES -- all checked before the handle is looked at; NB_ERR_UNSUPPORTED
 * as nb_orbits_sim. */
int nb_orbit_stability_sim(nb_sim *sim, const nb_orbit_params *params, const nb_orbit_stability_params *stability,
                           const double *pos, const double *vel, size_t m, const nb_orbit_deviation *dev0,
                           nb_orbit_sample *tracks, uint32_t *coincident, nb_orbit_deviation *devs,
                           nb_orbit_growth *growth, nb_orbit_stability_stats *stats);
/* Host only, a pure function of its arguments: what the records of a call with (dt, steps, every) say, for record r
 * of state k, tracer i and vector j, against the call's dev0.  |.| is the Euclidean norm of the six components in
 * the state's own units (positions and velocities are not weighted against each other), formed as
 * 2^E sqrt(sum (d_i 2^-E)^2) with E the exponent of the largest component, so that it cannot overflow:
 *   log_growth[(r m + i) D + j] = (log2 - log2_0) ln 2 + ln|d| - ln|d_0|          (ln of |delta_k| / |delta_0|)
 *   lyapunov[(r m + i) D + j]   = log_growth / ((double)k * dt), NaN at k = 0
 *   sali[r m + i]  = min(|u1 + u2|, |u1 - u2|),  gali2[r m + i] = |u1 ^ u2| = sqrt(sum_{a<b} (u1_a u2_b - u1_b u2_a)^2)
 *                    for the unit vectors u1, u2 of vectors 0 and 1; NaN with D < 2
 * A zero or non-finite vector gives NaN.  Any of the four outputs may be null.  NB_ERR_INVALID for null dev0 or devs
 * with m > 0, D outside 1 .. NB_ORBIT_MAX_DEVIATIONS, steps = 0, every = 0 or a dt that is not finite or 0. */
int nb_orbit_stability_derive(double dt, uint32_t steps, uint32_t every, size_t m, uint32_t deviations,
                              const nb_orbit_deviation *dev0, const nb_orbit_deviation *devs, double *log_growth,
                              double *lyapunov, double *sali, double *gali2);

/* ------------------------------------------------------------------------- */
/* Projected maps -- per-cell mass and velocity moments on a 2-D grid (no     */
/* reference counterpart: structure in two dimensions, without symmetry)      */
/* ------------------------------------------------------------------------- */
/* Projects the state nb_sim_read_particles would return along a line of sight
 * onto a metric, orthographic width x height grid and sums, per cell, the count,
 * the mass and (NB_MAP_VELOCITY) five velocity terms: the surface-density map,
 * the line-of-sight velocity map and the dispersion map, on the device.  The
 * rule, which DESIGN.md 6f states in full: everything in binary64 from the
 * binary32 state, one rounding per operation, no contraction, in this order:
 *   frame     n = axis / sqrt((ax ax + ay ay) + az az); e1 = the coordinate axis of
 *             the smallest |n_k| (the lowest index on ties), made orthogonal to n
 *             and normalised; e2 = n cross e1 -- the vectors of nb_field_rings, so
 *             ring points and map cells share coordinates (nb_map_frame)
 *   per body  d = (double)x - c, u = (double)v - v_c   (c, v_c: centre and its velocity)
 *             a = (dx e1x + dy e1y) + dz e1z; b, h the same with e2, n
 *             ua, ub, w the same from u
 *   edges     xe[i] = lo + (double)i ((hi - lo) / W) for i < W, xe[W] = hi exactly;
 *             ye the same from y_range and H (nb_map_edges)
 *   cell      the (i, j) with xe[i] <= a < xe[i+1] and ye[j] <= b < ye[j+1]: decided by
 *             comparisons against those edges, so the counts are exact integers
 *   outside   a or b outside its window, or h not in [depth lo, depth hi); every
 *             comparison with a NaN is false, so a NaN a, b or h (a NaN centre of
 *             mass: no mass) puts the body outside
 *   terms     m, m ua, m ub, m w, (m w) w, m ((ux ux + uy uy) + uz uz)
 * A body with any non-finite position, velocity or mass component is `nonfinite`
 * and left out of everything (the predicate of nb_sim_diagnostics).
 * binned_count + outside_count + nonfinite == n; sum of counts == binned_count.
 * NB_MAP_CENTER_COM: c and v_c are the fp64 `com` and `momentum / mass` that
 * nb_sim_diagnostics returns for the same state, bit for bit (the same moments
 * pass runs ahead on the stream; no host round trip).
 * No float atomics and no summation order that depends on timing: the result is
 * a function of the stored state and the parameters alone, two calls on one state
 * return bit-identical counts, planes and stats, and every double is within
 * 1e-10 of its sum of |term| of the binary64 sum.  The call is ordered after the
 * enqueued steps on the simulator's stream, ends with one synchronisation,
 * reports a TreeSim's status words as nb_sim_read_particles does, and does not
 * change the trajectory.
 * "map_segment_len" (nb_sim_set_tuning, 256..65536, a multiple of 256; default
 * 4096; speed and testing only): a cell's bodies are summed in runs of at most
 * this many bodies of its 8 x 8-cell tile, the runs then in order. */
#define NB_MAP_MAX_SIDE 4096u
#define NB_MAP_MAX_CELLS (1u << 22)
#define NB_MAP_CENTER_COM 1u /* centre = com, centre velocity = P/M of the measured state (as NB_RADIAL_CENTER_COM) */
#define NB_MAP_VELOCITY 2u   /* add the five velocity planes */

typedef struct nb_map_params {
    uint32_t width, height, flags, reserved; /* sides 1..NB_MAP_MAX_SIDE, at most NB_MAP_MAX_CELLS cells; reserved 0 */
    double center[3], velocity[3];           /* ignored with NB_MAP_CENTER_COM */
    double axis[3];                          /* line of sight; any non-zero finite vector */
    double x_range[2], y_range[2];           /* window in the plane coordinates a, b: [lo, hi) */
    double depth_range[2];                   /* slab along the line of sight: lo <= h < hi; -inf, +inf = everything */
} nb_map_params;

typedef struct nb_map_stats {
    uint64_t step_num, n, nonfinite, binned_count, outside_count;
    double binned_mass, outside_mass, mass; /* mass: all finite bodies */
    double center[3], velocity[3];          /* the values used */
    double n_hat[3], e1[3], e2[3];          /* the frame used */
    uint32_t width, height, flags, max_count;
} nb_map_stats;

/* The map of a simulator's current state.  counts: height * width values, row j the cells with b in
 * [ye[j], ye[j+1]) (row 0 is the smallest b: mathematical orientation).  planes: P planes of height * width
 * doubles, plane-major: P = 1 `mass`; with NB_MAP_VELOCITY P = 6: mass, m_ua, m_ub, m_w, m_w2, m_u2.
 * counts, planes and stats may each be null: what is not asked for is not copied, and a call with none of
 * them synchronises and measures nothing.  NB_ERR_INVALID for a null handle or params, a side outside
 * 1..NB_MAP_MAX_SIDE, more than NB_MAP_MAX_CELLS cells, unknown flag bits or reserved != 0, a zero or
 * non-finite axis, a non-finite centre or velocity without NB_MAP_CENTER_COM, a non-finite window bound,
 * hi <= lo in any range, a NaN depth bound, or edges that do not come out strictly ascending -- all
 * checked before any device call; NB_ERR_UNSUPPORTED for a sharded simulator (placement world > 1). */
int nb_sim_map(nb_sim *sim, const nb_map_params *params, uint32_t *counts, double *planes, nb_map_stats *stats);
/* Host only, no device: the frame of a map about `axis` (see above).  NB_ERR_INVALID for a null pointer or
 * a zero or non-finite axis. */
int nb_map_frame(const double axis[3], double n_hat[3], double e1[3], double e2[3]);
/* Host only, no device: the cells + 1 edges of a window [lo, hi) (see above).  NB_ERR_INVALID for a null
 * pointer, cells outside 1..NB_MAP_MAX_SIDE, non-finite bounds, hi <= lo, or edges that do not come out
 * strictly ascending. */
int nb_map_edges(double lo, double hi, uint32_t cells, double *edges);

/* ------------------------------------------------------------------------- */
/* Phase maps -- 2-D histograms of any two per-body quantities, a third       */
/* summed per cell (no reference counterpart: velocity distributions)         */
/* ------------------------------------------------------------------------- */
/* Bins the state nb_sim_read_particles would return on two per-body quantities
 * x and y and sums, per cell, the count, the mass and (NB_PHASE_WEIGHT) two
 * moments of a third quantity q: the r - u_r diagram, the R - u_phi diagram, a
 * position-velocity diagram, a line-of-sight velocity distribution, the
 * L_z - E diagram, on the device.  The rule, which DESIGN.md 6q states in full:
 * everything in binary64 from the binary32 state, one rounding per operation, no
 * contraction, only + - * / and sqrt, in this order:
 *   frame     n, e1, e2 exactly as nb_map_frame(axis) returns them
 *   per body  d = (double)x - c, u = (double)v - v_c, mu = (double)mass
 *             a, b, h and ua, ub, w exactly as nb_sim_map forms them
 *             R = sqrt(a a + b b);  r = sqrt((dx dx + dy dy) + dz dz)
 *             u2 = (ux ux + uy uy) + uz uz;  du = (dx ux + dy uy) + dz uz
 *             jx = dy uz - dz uy, jy = dz ux - dx uz, jz = dx uy - dy ux
 *   quantity  NB_PHASE_Q_* (nb_phase_quantity gives the id of a name):
 *             a, b, h       plane coordinates and height
 *             R, r          cylindrical and spherical radius
 *             ua, ub, w     velocity in the frame (w: along the line of sight)
 *             u_R           (a ua + b ub) / R
 *             u_phi         (a ub - b ua) / R
 *             u_r           du / r
 *             u_t           sqrt(t), t = u2 - u_r u_r, a t < 0 replaced by +0
 *             speed         sqrt(u2)
 *             j_z           a ub - b ua
 *             j             sqrt((jx jx + jy jy) + jz jz)
 *             e_kin         0.5 u2
 *             mass          mu
 *             value         values[i], the caller's n doubles in the order of
 *                           nb_sim_read_particles now (the potential of nb_sim_field,
 *                           the density of nb_sim_knn, the energy of nb_sim_bound)
 *             There is no azimuth: atan2 is not restated bit for bit (nb_disc_modes_sim).
 *   edges     the caller's x_edges[W + 1] and y_edges[H + 1], strictly ascending, the
 *             interior ones finite; the first may be -inf and the last +inf
 *             (nb_map_edges and nb_radial_edges_log build linear and log ones)
 *   cell      the (i, j) with xe[i] <= x < xe[i+1] and ye[j] <= y < ye[j+1]: decided by
 *             comparisons against the edges alone
 *   classes   nonfinite: any non-finite position, velocity or mass component (the
 *             predicate of nb_sim_diagnostics); left out of everything
 *             undefined: x, y or (NB_PHASE_WEIGHT) q is not finite -- 0/0 for u_phi at
 *             R = 0, a NaN in values; such a body is outside
 *             outside: x or y is in no cell;  binned: every other body
 *   terms     mu, and with NB_PHASE_WEIGHT mu q and (mu q) q
 * binned_count + outside_count + nonfinite == n; undefined_count <= outside_count;
 * sum of counts == binned_count.
 * When x, y or (NB_PHASE_WEIGHT) q is `value`, step_num must be the simulator's step
 * number (NB_PHASE_ANY_STEP switches the check off): a TreeSim reorders its bodies
 * every step, and a stale array is refused as nb_shape_params refuses a stale catalogue.
 * NB_PHASE_CENTER_COM: c and v_c are the fp64 `com` and `momentum / mass` that
 * nb_sim_diagnostics returns for the same state, bit for bit (the same moments
 * pass runs ahead on the stream; no host round trip).
 * The guarantees are those of nb_sim_map, whose grouping and summing code this pass
 * runs: no float atomics, two calls on one state return bit-identical counts,
 * planes and stats, every double is within 1e-10 of its sum of |term| of the
 * binary64 sum; with x = a, y = b, q = w on the edges of nb_map_edges and equal
 * segment lengths the counts and the three planes are nb_sim_map's counts, mass,
 * m_w and m_w2 bit for bit.  The call is ordered after the enqueued steps on the
 * simulator's stream, ends with one synchronisation, reports a TreeSim's status
 * words as nb_sim_read_particles does, and does not change the trajectory.
 * "phase_segment_len" (nb_sim_set_tuning, 256..65536, a multiple of 256; default
 * 4096; speed and testing only) is this pass's "map_segment_len".
 * This is the fifteenth analysis pass, spelt noun first as nb_group_radii_sim is. */
#define NB_PHASE_CENTER_COM 1u /* as NB_MAP_CENTER_COM */
#define NB_PHASE_WEIGHT 2u     /* add the planes mu q and (mu q) q */
#define NB_PHASE_ANY_STEP 0xFFFFFFFFFFFFFFFFull /* nb_phase_params.step_num: UINT64_MAX */

enum {
    NB_PHASE_Q_A = 0,
    NB_PHASE_Q_B,
    NB_PHASE_Q_H,
    NB_PHASE_Q_R_CYL, /* "R" */
    NB_PHASE_Q_R,     /* "r" */
    NB_PHASE_Q_UA,
    NB_PHASE_Q_UB,
    NB_PHASE_Q_W,
    NB_PHASE_Q_U_R_CYL, /* "u_R" */
    NB_PHASE_Q_U_PHI,
    NB_PHASE_Q_U_R, /* "u_r" */
    NB_PHASE_Q_U_T,
    NB_PHASE_Q_SPEED,
    NB_PHASE_Q_J_Z,
    NB_PHASE_Q_J,
    NB_PHASE_Q_E_KIN,
    NB_PHASE_Q_MASS,
    NB_PHASE_Q_VALUE,
    NB_PHASE_Q_COUNT
};

typedef struct nb_phase_params {
    uint32_t width, height, flags, reserved; /* sides 1..NB_MAP_MAX_SIDE, at most NB_MAP_MAX_CELLS cells; reserved 0 */
    uint32_t x, y, q, reserved2;             /* NB_PHASE_Q_*; q is summed only with NB_PHASE_WEIGHT; reserved2 0 */
    double center[3], velocity[3];           /* ignored with NB_PHASE_CENTER_COM */
    double axis[3];                          /* the frame's axis; any non-zero finite vector */
    const double *x_edges, *y_edges;         /* width + 1 and height + 1 edges */
    const double *values;                    /* n doubles, or NULL when no quantity is `value` */
    uint64_t step_num;                       /* with `value`: the simulator's step number, or NB_PHASE_ANY_STEP */
} nb_phase_params;

typedef struct nb_phase_stats {
    uint64_t step_num, n, nonfinite, binned_count, outside_count, undefined_count;
    double binned_mass, outside_mass, mass; /* mass: all finite bodies */
    double center[3], velocity[3];          /* the values used */
    double n_hat[3], e1[3], e2[3];          /* the frame used */
    uint32_t width, height, flags, max_count;
    uint32_t x, y, q, reserved; /* the quantity ids */
} nb_phase_stats;

#if defined(__cplusplus)
static_assert(sizeof(nb_phase_params) == 136 && sizeof(nb_phase_stats) == 224, "nb_phase_* layouts");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(nb_phase_params) == 136 && sizeof(nb_phase_stats) == 224, "nb_phase_* layouts");
#endif

/* The phase map of a simulator's current state.  counts: height * width values, row j the cells with y in
 * [ye[j], ye[j+1]).  planes: P planes of height * width doubles, plane-major: P = 1 `mass`; with
 * NB_PHASE_WEIGHT P = 3: mass, m_q, m_q2.  counts, planes and stats may each be null: what is not asked for is
 * not copied, and a call with none of them synchronises and measures nothing.  A simulator without bodies is
 * answered on the host.  NB_ERR_INVALID for a null handle, params or edge array, a side outside
 * 1..NB_MAP_MAX_SIDE, more than NB_MAP_MAX_CELLS cells, unknown flag bits, an unknown quantity id, a reserved
 * field != 0, a zero or non-finite axis, a non-finite centre or velocity without NB_PHASE_CENTER_COM, edges
 * that are not strictly ascending or have a non-finite interior edge, `value` without values, or a stale
 * step_num -- all checked before any device call; NB_ERR_UNSUPPORTED for a sharded simulator (placement
 * world > 1).  Launches nothing inside a graph capture of the steps: the call is ordered after them. */
int nb_phase_map_sim(nb_sim *sim, const nb_phase_params *params, uint32_t *counts, double *planes,
                     nb_phase_stats *stats);
/* Host only, no device: the id of the quantity called `name` (the names of the table above, case-sensitive).
 * NB_ERR_INVALID for a null pointer or a name that is not in the table. */
int nb_phase_quantity(const char *name, uint32_t *id);
/* Host only, no device: the name of quantity `id`, or NULL for an id that is not in the table. */
const char *nb_phase_quantity_name(uint32_t id);

/* ------------------------------------------------------------------------- */
/* Friends-of-friends groups -- which bodies belong together (no reference    */
/* counterpart: the clumps of the current state, on the device)               */
/* ------------------------------------------------------------------------- */
/* Partitions the state nb_sim_read_particles would return into the connected
 * components of the "friends" graph and sums a catalogue of the larger ones.
 * The rule, which DESIGN.md 6h states in full: binary64 from the binary32 state,
 * one rounding per operation, no contraction:
 *   counted   a body takes part when its position, mass and velocity are all
 *             finite (the predicate of nb_sim_diagnostics); every other body is
 *             `nonfinite`, has label NB_FOF_NONE and belongs to no group
 *   friends   bodies i != j are friends iff d2 <= b2, with
 *             dx = (double)x_i - (double)x_j, dy and dz likewise,
 *             d2 = (dx dx + dy dy) + dz dz, b2 = link * link formed once;
 *             the rule is symmetric in i and j
 *   groups    a group is a connected component of the friends graph; a body's
 *             label is the smallest body index of its component.  The index is the
 *             one in the order nb_sim_read_particles returns at that moment: a
 *             TreeSim reorders its bodies at every step, so labels of different
 *             steps do not name the same bodies
 *   catalogue the components with count >= min_members, numbered in ascending
 *             label order; a row holds label, count and nine sums over the members:
 *             m, m x, m y, m z, m vx, m vy, m vz, m ((x x + y y) + z z),
 *             m ((vx vx + vy vy) + vz vz); group_of[i] is body i's row or NB_FOF_NONE
 * The partition is unique, so labels, group_of, counts and every integer of the
 * stats are exact and bit-identical between calls, whatever order the device's
 * threads ran in.  The sums are added in a fixed order (the members in body order
 * in runs of 64, a run by a fixed butterfly, the runs then in order): two calls
 * return bit-identical doubles, each within 1e-10 of its sum of |term| of the
 * binary64 sum.  No float atomics.
 * nonfinite + sum of all component sizes == n; sum of the catalogue's counts ==
 * grouped_bodies.  largest_label is the smallest label among the components of
 * largest_count (NB_FOF_NONE, 0 without components).
 * The bodies are sorted into cubic cells of side (link / sqrt(3)) (1 - 2^-20)
 * from the smallest counted coordinate of every axis; a state that needs more than
 * NB_FOF_MAX_CELLS_PER_AXIS cells on an axis is refused (NB_ERR_INVALID, after the
 * call's one synchronisation, outputs untouched): such a link is below the
 * resolution of binary32 coordinates over that extent.
 * The call is ordered after the enqueued steps on the simulator's stream, ends
 * with one synchronisation, reports a TreeSim's status words as
 * nb_sim_read_particles does, and does not change the trajectory.
 * "fof_chunk_len" (nb_sim_set_tuning, 64..65536, a multiple of 64; default 1024;
 * speed and testing only): the bodies of a cell, and of a catalogue row, one work
 * item takes.  "fof_cell_boxes" (0 or 1, default 1; speed and testing only): use
 * per-cell bounding boxes to skip or link neighbour cells without pair tests.
 * Neither changes a bit of the result. */
#define NB_FOF_NONE 0xFFFFFFFFu
#define NB_FOF_MAX_CELLS_PER_AXIS (1u << 21)

typedef struct nb_fof_params {
    double link;          /* b: finite, > 0 */
    uint32_t min_members; /* >= 1: the smallest component the catalogue holds */
    uint32_t flags;       /* 0 */
    uint64_t reserved;    /* 0 */
} nb_fof_params;

typedef struct nb_fof_group {
    uint32_t label, count;
    double mass, mx[3], mv[3], mr2, mv2; /* the nine sums, in the order above */
} nb_fof_group;

typedef struct nb_fof_stats {
    uint64_t step_num, n, nonfinite;
    uint64_t components;     /* all of them, singletons included */
    uint64_t groups;         /* the catalogued ones, even when group_capacity is smaller */
    uint64_t grouped_bodies; /* bodies of catalogued components */
    uint32_t largest_count, largest_label;
    uint32_t cells[3];       /* cells per axis that were used (0 without counted bodies) */
    uint32_t reserved;
    double cell_side;        /* the cell side that was used */
} nb_fof_stats;

/* The groups of a simulator's current state.  labels and group_of: n values each; groups: room for
 * group_capacity rows, of which the first min(stats->groups, group_capacity) are written.  Every output
 * pointer may be null: what is not asked for is not copied (and without `groups` no sum is formed); a call
 * with none of them synchronises and measures nothing.  NB_ERR_INVALID for a null handle or params, a
 * non-finite or non-positive link or one whose square is not a positive finite double (it under- or
 * overflows), min_members == 0, unknown flags or reserved != 0 -- all checked before any device call --
 * and for a state that needs too many cells (above); NB_ERR_UNSUPPORTED for a sharded simulator (placement
 * world > 1). */
int nb_sim_fof(nb_sim *sim, const nb_fof_params *params, uint32_t *labels, uint32_t *group_of,
               nb_fof_group *groups, size_t group_capacity, nb_fof_stats *stats);

/* ------------------------------------------------------------------------- */
/* Phase-space groups -- friends-of-friends in position and velocity (no      */
/* reference counterpart: what overlaps in space but moves apart, separated)  */
/* ------------------------------------------------------------------------- */
/* Partitions the state nb_sim_read_particles would return into the connected
 * components of a "friends" graph in six dimensions (the 6DFOF of Diemand et al.
 * 2006, the first stage of ROCKSTAR, Behroozi et al. 2013) and sums a catalogue of
 * the larger ones.  The rule, which DESIGN.md 6u states in full: binary64 from the
 * binary32 state, one rounding per operation, no contraction:
 *   counted   exactly as in nb_sim_fof: position, mass and velocity all finite;
 *             every other body is `nonfinite`, has label NB_FOF_NONE and belongs to
 *             no group
 *   constants formed once on the host: b2 = link * link, v2 = vlink * vlink,
 *             rhs = b2 * v2
 *   friends   bodies i != j are friends iff both clauses hold:
 *             1. d2 <= b2, d2 being nb_sim_fof's own expression:
 *                dx = (double)x_i - (double)x_j, dy and dz likewise,
 *                d2 = (dx dx + dy dy) + dz dz
 *             2. (d2 * v2 + u2 * b2) <= rhs, with du = (double)vx_i - (double)vx_j,
 *                dv and dw likewise, u2 = (du du + dv dv) + dw dw
 *             This is (dx / b)^2 + (dv / b_v)^2 <= 1 without a division, symmetric
 *             in i and j.  Every term is non-negative: a sum may become +inf but
 *             never NaN, so both clauses may be evaluated for every pair
 *   groups, labels, catalogue, group_of
 *             word for word those of nb_sim_fof: a group is a connected component,
 *             its label the smallest body index (in the order nb_sim_read_particles
 *             returns at that moment), the rows with count >= min_members in
 *             ascending label order, each an nb_fof_group with nb_sim_fof's nine
 *             sums in its summation order
 * Three consequences:
 *   refinement        clause 1 is nb_sim_fof's predicate, so every phase-space group
 *                     lies inside exactly one group of nb_sim_fof(link)
 *   equal velocities  with all counted velocities equal u2 = 0 and clause 2 follows
 *                     from clause 1 (d2 <= b2 gives d2 * v2 <= b2 * v2: rounding is
 *                     monotone, and adding 0 is exact); labels, group_of, the rows
 *                     and the integer stats are then those of nb_sim_fof(link,
 *                     min_members), byte for byte
 *   frame, uniqueness the predicate sees only differences, so the partition does not
 *                     depend on the frame (as long as the shifted binary32 state
 *                     keeps its differences); it is unique, so labels, group_of,
 *                     counts and every integer of the stats are exact and
 *                     bit-identical between calls
 * The sums, the cells (the position grid of nb_sim_fof at the same link: cells and
 * cell_side of the stats are its), the refusal of a state that needs more than
 * NB_FOF_MAX_CELLS_PER_AXIS cells on an axis (NB_ERR_INVALID, after the call's one
 * synchronisation, outputs untouched) and the behaviour on the stream are
 * nb_sim_fof's.  No float atomics.
 * "fof_chunk_len" applies as it does there.  "fof6_boxes" (0 or 1, default 1; speed
 * and testing only): use per-cell position and velocity boxes to skip or link whole
 * cell pairs, a cell with itself included, without pair tests.  Neither changes a bit
 * of the result.  A cell of P bodies whose boxes decide nothing costs P (P - 1) / 2
 * pair tests. */
typedef struct nb_fof6_params {
    double link;          /* b: finite, > 0 */
    double vlink;         /* b_v: finite, > 0 */
    uint32_t min_members; /* >= 1: the smallest component the catalogue holds */
    uint32_t flags;       /* 0 */
    uint64_t reserved;    /* 0 */
} nb_fof6_params;

/* The phase-space groups of a simulator's current state; the outputs are nb_sim_fof's and every output
 * pointer may be null with its meaning there.  NB_ERR_INVALID for a null handle or params, a link or vlink
 * that is not finite or not > 0, a b2, v2 or rhs that is not a positive finite double, min_members == 0,
 * unknown flags or reserved != 0 -- all checked before any device call -- and for a state that needs too
 * many cells; NB_ERR_UNSUPPORTED for a sharded simulator (placement world > 1). */
int nb_fof6_sim(nb_sim *sim, const nb_fof6_params *params, uint32_t *labels, uint32_t *group_of,
                nb_fof_group *groups, size_t group_capacity, nb_fof_stats *stats);

/* ------------------------------------------------------------------------- */
/* Bound groups -- which friends-of-friends groups hold together (no reference */
/* counterpart: every catalogued group unbound on the device)                 */
/* ------------------------------------------------------------------------- */
/* Finds the groups of the current state exactly as nb_sim_fof(link, min_members)
 * does -- the same labels, rows and group_of -- and removes from every catalogued
 * group, round by round, the members whose energy in the group's own frame is
 * positive.  The rule, which DESIGN.md 6k states in full.  For catalogue row r the
 * list L is the bodies with group_of == r in ascending body index; the coupling is
 * c = (double)g * (double)dt (the convention of nb_sim_diagnostics: U = -g dt W);
 * the active set starts as A = L; round t = 1, 2, ... does
 *   1  M = sum_A (double)m and P = sum_A m v in binary64, in a fixed order (below);
 *      unless M > 0 the group is DISSOLVED (B empty), `iterations` = t - 1
 *   2  V = P / M
 *   3  for every i in A: S_i = sum over j in A, j != i, of m_j psi(r_ij), psi the
 *      potential of the pair force (psi(r) = integral_r^inf ds / (s^3 + e)); the
 *      per-pair term is binary32 exactly as nb_sim_field and nb_sim_diagnostics
 *      form it; runs of at most 64 consecutive terms are summed in binary32, every
 *      run is folded into a binary64 sum and the partial sums are added in binary64
 *      in a fixed order.  j is excluded by index: a distinct member at the same
 *      coordinates adds m_j psi(0); with e == 0 a massless j at distance 0 adds 0.
 *      phi_i = -c S_i
 *   4  u = (double)v_i - V, k_i = 0.5 ((ux ux + uy uy) + uz uz), e_i = k_i + phi_i;
 *      one rounding per operation, no contraction
 *   5  R = { i in A : e_i > 0 }.  R empty: CONVERGED, B = A.  Otherwise A <- A \ R;
 *      then |A| < min_bound: DISSOLVED, B empty; else t == max_iter: UNCONVERGED,
 *      B = A after the removal with the values of round t; else round t + 1 runs.
 *      `iterations` = t
 * Massless members are tracers: they take part and attract nobody.  A group with
 * count > max_group (max_group > 0) is SKIPPED: no round runs, its energies are NaN
 * and its bound_count is 0 -- one round over a group costs count^2 pair terms, and
 * the caller must be able to refuse that.
 *   energy[i]    e_i of the last round in which body i was active: > 0 for a removed
 *                body, <= 0 for one that stayed; NaN for a body of no analysed group
 *                and where no round ran
 *   bound_of[i]  the row for i in B, otherwise NB_FOF_NONE
 *   a row        label and count are nb_sim_fof's.  Over B, with the last round's V
 *                and phi: mass, mx, mv, mr2 (nb_fof_group's terms), kinetic =
 *                sum m_i k_i, potential = 1/2 sum m_i phi_i, phi_min = the smallest
 *                phi_i and most_bound = the smallest body index that has it (NaN and
 *                NB_FOF_NONE for an empty B).  Over L in round 1: kinetic0 and
 *                potential0, the same two sums (NaN where no round ran)
 * The order of every sum is fixed by the group's own list alone.  Position p of a
 * member is its place in L; a removed member keeps its place with its mass set to 0,
 * so the runs of step 3 are the positions [64 q, 64 q + 64) whatever A is.  The
 * j-range of a group of `count` members is cut into segments of
 * max(1024, 256 ceil(ceil(count / 256) / 8)) positions: at most 8; inside a segment
 * the runs are folded in order into one binary64 partial, and a row's partials are
 * added in segment order.  The sums over members go through runs of 64 positions by
 * the fixed butterfly of nb_sim_fof and the runs are added in order.  So a group's
 * outputs are a function of its own list and state alone -- not of the other groups,
 * of group_capacity or of the tuning keys -- and two calls return bit-identical
 * outputs.  No float atomics.
 * Against the same rule with S_i in binary64:
 *   |S_i - S_i(64)| <= 5e-6 sum_j |m_j| psi(r_ij)            (nb_sim_field's bound)
 * and the integers (bound_of, bound_count, iterations, status) equal the binary64
 * rule's wherever each of its decisions is decisive:
 *   |e_i| > 4 (5e-6 c sum_j |m_j| psi(r_ij) + 1e-12 (k_i + |V|^2))   in every round
 * (by induction over the rounds: equal sets, then phi within the bound, then equal
 * decisions).  A marginal decision is still deterministic on the device.
 * Rows beyond group_capacity are not analysed: their bodies have bound_of
 * NB_FOF_NONE and energy NaN.  group_capacity counts whether or not `groups` is null.
 * The call is ordered after the enqueued steps on the simulator's stream, enqueues
 * all max_iter rounds up front (the blocks of a finished group return at once), ends
 * with one synchronisation, reports a TreeSim's status words as
 * nb_sim_read_particles does, and does not change the trajectory.
 * "bound_chunk_len" (nb_sim_set_tuning, 64..1048576, a multiple of 64; default 1024):
 * the j positions one work item takes -- whole segments, at least one.
 * "bound_tile" (0, 64 or 256; default 0): the members of an i-tile; 0 takes 64 for
 * groups of at most 256 members and 256 above.  Speed and testing only: neither
 * changes a bit of the result. */
#define NB_BOUND_CONVERGED 1u
#define NB_BOUND_DISSOLVED 2u
#define NB_BOUND_UNCONVERGED 4u
#define NB_BOUND_SKIPPED 8u
#define NB_BOUND_MAX_ITER 64u

typedef struct nb_bound_params {
    double link;          /* as nb_fof_params */
    uint32_t min_members; /* as nb_fof_params */
    uint32_t min_bound;   /* >= 1: a group left with fewer members is dissolved */
    uint32_t max_iter;    /* 1 .. NB_BOUND_MAX_ITER */
    uint32_t max_group;   /* 0: no limit; else groups with more members are skipped */
    uint32_t flags;       /* 0 */
    uint32_t reserved32;  /* 0 */
    uint64_t reserved;    /* 0 */
} nb_bound_params;

typedef struct nb_bound_group {
    uint32_t label, count;            /* nb_fof_group's */
    uint32_t bound_count, iterations; /* |B|; rounds that ran */
    uint32_t status;                  /* one of NB_BOUND_CONVERGED .. NB_BOUND_SKIPPED */
    uint32_t most_bound;              /* body index, or NB_FOF_NONE */
    double mass, mx[3], mv[3], mr2;   /* over B */
    double kinetic, potential, phi_min;
    double kinetic0, potential0;      /* over L in round 1 */
} nb_bound_group;

typedef struct nb_bound_stats {
    uint64_t step_num, n, nonfinite;
    uint64_t components, groups, grouped_bodies; /* nb_fof_stats' */
    uint32_t largest_count, largest_label;
    uint64_t bound_groups; /* analysed rows with a non-empty B */
    uint64_t bound_bodies; /* sum of their bound_count */
    uint64_t dissolved, unconverged, skipped; /* analysed rows by status */
    uint64_t pairs;        /* pair terms evaluated: sum over the rows of iterations * count * (count - 1) */
    uint32_t rounds_max;   /* the largest `iterations` */
    uint32_t reserved;
} nb_bound_stats;

#if defined(__cplusplus)
static_assert(sizeof(nb_bound_params) == 40 && sizeof(nb_bound_group) == 128 && sizeof(nb_bound_stats) == 112,
              "nb_bound_* layouts");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(nb_bound_params) == 40 && sizeof(nb_bound_group) == 128 && sizeof(nb_bound_stats) == 112,
               "nb_bound_* layouts");
#endif

/* The bound groups of a simulator's current state.  group_of and bound_of: n values each; energy: n doubles;
 * groups: room for group_capacity rows, of which the first min(stats->groups, group_capacity) are written.
 * Every output pointer may be null: what is not asked for is not copied; a call with none of them
 * synchronises and measures nothing.  NB_ERR_INVALID for a null handle or params, everything nb_sim_fof
 * refuses, softening e < 0, max_iter outside 1..NB_BOUND_MAX_ITER, min_bound == 0, unknown flags or a
 * reserved field != 0 -- all checked before any device call -- and for a state that needs too many cells
 * (nb_sim_fof); NB_ERR_UNSUPPORTED for a sharded simulator (placement world > 1). */
int nb_sim_bound(nb_sim *sim, const nb_bound_params *params, uint32_t *group_of, uint32_t *bound_of, double *energy,
                 nb_bound_group *groups, size_t group_capacity, nb_bound_stats *stats);

/* ------------------------------------------------------------------------- */
/* k-nearest-neighbour density -- how dense the state is at every body, and    */
/* the density centre (no reference counterpart)                              */
/* ------------------------------------------------------------------------- */
/* For every body of the state nb_sim_read_particles would return: the squared
 * distance to its k-th nearest neighbour, that neighbour, the mass inside it and
 * the density of Casertano & Hut (1985) from them; and the density-weighted sums
 * that give the density centre.  The rule, which DESIGN.md 6i states in full:
 * binary64 from the binary32 state, one rounding per operation, no contraction:
 *   counted   a body takes part when its position, mass and velocity are all
 *             finite (the predicate of nb_sim_diagnostics); c is their number
 *   distance  d2(i, j) = (dx dx + dy dy) + dz dz with dx = (double)x_i - (double)x_j,
 *             dy and dz likewise (the expression of nb_sim_fof); finite for
 *             counted bodies
 *   order     for a counted body i the other counted bodies in ascending
 *             (d2(i, j), j): equal d2 are ordered by the smaller body index, the
 *             index in the order nb_sim_read_particles returns at that moment (a
 *             TreeSim reorders its bodies at every step)
 *   per body  for 1 <= k <= NB_KNN_MAX_K and c > k:
 *             r2[i]      the d2 of the k-th body of that order
 *             kth[i]     its index
 *             mass_in[i] the binary64 sum of (double)m_j over the first k - 1 bodies,
 *                        added in that order from 0 (0 for k = 1)
 *             density[i] mass_in[i] / (C (r2[i] sqrt(r2[i]))), C = NB_KNN_SPHERE,
 *                        evaluated as written: sqrt, multiply, multiply, divide
 *   special   r2[i] == 0 (at least k bodies coincide with i): density[i] = +inf and
 *             the body is one of `degenerate`;
 *             a body that is not counted: r2 = NaN, kth = NB_KNN_NONE, mass_in = 0,
 *             density = 0;
 *             c <= k: every counted body has r2 = +inf, kth = NB_KNN_NONE, mass_in = 0,
 *             density = 0; short_of_k = c (0 otherwise), sums 0, no peak
 *   sums      over the counted bodies with finite, non-zero r2, rho = density[i]:
 *             rho, rho x, rho y, rho z, rho vx, rho vy, rho vz, rho rho, each term one
 *             binary64 product of rho and the widened coordinate, added in body order
 *             in a fixed order (blocks of 256 bodies by a fixed butterfly, the blocks
 *             then in 16 interleaved groups): two calls return bit-identical doubles,
 *             each within 1e-10 of its sum of |term| of the binary64 sum
 *   peak      over the same bodies, those of finite density: peak_density is the
 *             largest density and peak_index the smallest index that holds it
 *             (0 and NB_KNN_NONE when there is none)
 * Everything per body is unique given the state, so r2, kth, mass_in, density, the peak
 * and every integer of the stats are exact and bit-identical between calls, whatever
 * order the device's threads ran in.  No float atomics.  The density centre is
 * sum_rho_x / sum_rho, its velocity sum_rho_v / sum_rho.
 * The call is ordered after the enqueued steps on the simulator's stream, ends
 * with one synchronisation, reports a TreeSim's status words as
 * nb_sim_read_particles does, and does not change the trajectory.
 * "knn_span_cells" (nb_sim_set_tuning, 1..8, default 3; speed and testing only): the
 * octree cells per axis the search opens around a body.  "knn_block_queries" (1, 2
 * or 4, default 4; speed and testing only): the bodies one block of the search
 * serves, a wave each.  Neither changes a bit of the result. */
#define NB_KNN_NONE 0xFFFFFFFFu
#define NB_KNN_MAX_K 64u
#define NB_KNN_SPHERE 4.1887902047863909846 /* C = 4 pi / 3, to binary64 0x1.0c152382d7366p+2 */

typedef struct nb_knn_params {
    uint32_t k;        /* 1 .. NB_KNN_MAX_K */
    uint32_t flags;    /* 0 */
    uint64_t reserved; /* 0 */
} nb_knn_params;

typedef struct nb_knn_stats {
    uint64_t step_num, n, nonfinite, counted, degenerate, short_of_k;
    double sum_rho, sum_rho_x[3], sum_rho_v[3], sum_rho2, peak_density;
    uint32_t peak_index, reserved;
} nb_knn_stats;

/* The per-body values (n each) and the stats of a simulator's current state.  Every output pointer may be
 * null: what is not asked for is not copied; a call with none of them synchronises and measures nothing.
 * The outputs are written only by a call that succeeds.  NB_ERR_INVALID for a null handle or params,
 * k == 0, k > NB_KNN_MAX_K, unknown flags or reserved != 0 -- all checked before any device call;
 * NB_ERR_UNSUPPORTED for a sharded simulator (placement world > 1). */
int nb_sim_knn(nb_sim *sim, const nb_knn_params *params, double *r2, uint32_t *kth, double *mass_in,
               double *density, nb_knn_stats *stats);

/* ------------------------------------------------------------------------- */
/* Minimum spanning tree -- the friends-of-friends groups of every linking    */
/* length at once (no reference counterpart)                                  */
/* ------------------------------------------------------------------------- */
/* The Euclidean minimum spanning tree of the counted bodies of the state
 * nb_sim_read_particles would return.  The components of nb_sim_fof(link) are the
 * components of the tree's edges with d2 <= link link, so the sorted edge list is the
 * whole single-linkage hierarchy: c - 1 merges, each at a known length.  The rule,
 * which DESIGN.md 6y states in full: binary64 from the binary32 state, one rounding
 * per operation, no contraction:
 *   counted     the predicate of nb_sim_knn; c is the number of counted bodies
 *   distance    d2(i, j) of nb_sim_knn (the expression of nb_sim_fof), bitwise
 *               symmetric in i and j
 *   edge order  pairs of counted bodies i != j in ascending (d2(i, j), min(i, j),
 *               max(i, j)): strict and total; the indices are those
 *               nb_sim_read_particles returns at that moment (a TreeSim reorders
 *               its bodies at every step)
 *   tree        the minimum spanning tree of the complete graph on the counted
 *               bodies under that order: unique, c - 1 edges (0 for c <= 1)
 *   output      in ascending edge order: edge_lo[e] < edge_hi[e] (body indices) and
 *               d2[e]; per body, degree[i] = the number of tree edges at body i, or
 *               NB_MST_NONE for a body that is not counted
 *   stats       edges = max(c, 1) - 1; rounds = the Boruvka rounds that ran (every
 *               component takes the first edge of the order that leaves it, all of
 *               them are united; rounds run while more than one component is left)
 *               and components_after[r] = the components after round r (0 from
 *               `rounds` on); d2_min, d2_max = the first and last d2 (0 without
 *               edges); lo, hi, h = the bounds of the counted bodies and the side of
 *               the finest search cell (0 for c == 0)
 * The tree is unique given the state, and Boruvka's rounds under a total order are
 * deterministic, so every integer and every double is exact and bit-identical
 * between calls, whatever order the device's threads ran in.  No float atomics.
 * The call is ordered after the enqueued steps on the simulator's stream, ends
 * with one synchronisation, reports a TreeSim's status words as
 * nb_sim_read_particles does, and does not change the trajectory.
 * "mst_span_cells" (nb_sim_set_tuning, 1..8, default 3), "mst_block_queries" (1, 2 or
 * 4, default 4), "mst_skip_runs" (0 or 1, default 1: stretches of a body's own
 * component are stepped over) and "mst_shared_bound" (0 or 1, default 1: the bodies of
 * a component share the smallest d2 any of them has found) are for speed and
 * testing only: none changes a bit of the result. */
#define NB_MST_NONE 0xFFFFFFFFu
#define NB_MST_MAX_ROUNDS 32u

typedef struct nb_mst_params {
    uint32_t flags;      /* 0 */
    uint32_t reserved32; /* 0 */
    uint64_t reserved;   /* 0 */
} nb_mst_params;

typedef struct nb_mst_stats {
    uint64_t step_num, n, nonfinite, edges;
    uint32_t rounds, reserved;
    uint32_t components_after[NB_MST_MAX_ROUNDS];
    double d2_min, d2_max;
    double lo[3], hi[3], h;
} nb_mst_stats;

/* The tree of a simulator's current state: edge_lo, edge_hi and d2 have room for n - 1 entries (n the
 * simulator's bodies), of which the first stats->edges are written; degree has n.  Every output pointer may
 * be null: what is not asked for is not copied; a call with none of them synchronises and measures nothing.
 * The outputs are written only by a call that succeeds.  NB_ERR_INVALID for a null handle or params,
 * unknown flags or a reserved field != 0 -- all checked before any device call; NB_ERR_UNSUPPORTED for a
 * sharded simulator (placement world > 1) and for more than 2^31 - 1 bodies (the rounds enqueued, at most 31, and
 * components_after rest on that cap). */
int nb_mst_sim(nb_sim *sim, const nb_mst_params *params, uint32_t *edge_lo, uint32_t *edge_hi, double *d2,
               uint32_t *degree, nb_mst_stats *stats);
/* Host only.  The tree cut at `link`: the edges with d2 <= link link united (the square formed once, as
 * nb_sim_fof forms it), labels[i] = the smallest body index of i's component, or NB_FOF_NONE for a body with
 * degree[i] == NB_MST_NONE (degree null: every body counts); *components (may be null) = their number.  The
 * labels are those of nb_sim_fof(link, min_members 1) on the same state.  NB_ERR_INVALID for a null array that
 * is needed, an edge with lo >= hi or hi >= n, n > 2^32 - 1, edges >= max(n, 1), and a link that is not finite
 * and > 0 or whose square is not a positive finite double.  There are no cells: no link is too small. */
int nb_mst_cut(size_t n, size_t edges, const uint32_t *edge_lo, const uint32_t *edge_hi, const double *d2,
               const uint32_t *degree, double link, uint32_t *labels, size_t *components);
/* Host only.  The dendrogram: per edge in order the labels (smallest body indices, label_a[e] < label_b[e]) and
 * the sizes of the two components it joins.  Each output may be null.  NB_ERR_INVALID as nb_mst_cut, and for
 * edges that close a cycle. */
int nb_mst_linkage(size_t n, size_t edges, const uint32_t *edge_lo, const uint32_t *edge_hi, uint32_t *label_a,
                   uint32_t *label_b, uint32_t *count_a, uint32_t *count_b);

/* ------------------------------------------------------------------------- */
/* Density-peak groups -- which bodies belong to which density peak (HOP,     */
/* Eisenstein & Hut 1998; no reference counterpart)                           */
/* ------------------------------------------------------------------------- */
/* Every body hops to the densest of its nearest neighbours until it reaches a
 * body that is its own densest neighbour, a peak; the bodies that end at one peak
 * are a group.  Pairs of neighbours in different groups give the boundaries
 * between groups, from which nb_hop_regroup merges groups across high saddles.
 * The rule, which DESIGN.md 6m states in full: binary64 from the binary32 state,
 * one rounding per operation, no contraction; indices are those of
 * nb_sim_read_particles at that moment:
 *   counted    the predicate of nb_sim_knn; c is the number of counted bodies.
 *              With K = max(k_density, k_hop, k_merge) a state with c <= K is
 *              short: every label is NB_HOP_NONE, there are no groups and no
 *              boundaries, short_of_k = c (0 otherwise)
 *   density    density[i] is that of nb_sim_knn with k = k_density, bit for bit;
 *              its ordering key rho'_i is density[i], or -inf where that is NaN.
 *              Body a is denser than b iff rho'_a > rho'_b, or they are equal and
 *              a < b: a strict total order; +inf is allowed (coincident bodies)
 *   inside     a counted body with rho'_i >= density_min (-inf: no cut).  Every
 *              other body has label NB_HOP_NONE, is one of `outside` when it is
 *              counted, and takes no part in what follows
 *   hop        next[i] is the densest body among i itself and the first k_hop
 *              bodies of i's neighbour order, the (d2, j) order of nb_sim_knn.  A
 *              denser neighbour of an inside body is itself inside
 *   label      following next from i ends at a body p with next[p] = p, a peak:
 *              every hop goes to a strictly denser body.  labels[i] = p
 *   catalogue  the groups with count >= min_members in ascending label order:
 *              nb_fof_group rows with the nine sums and the summation order of
 *              nb_sim_fof, and peak_density[row] = density[label]; group_of[i] is
 *              body i's row or NB_HOP_NONE
 *   boundaries a body pair is taken for every inside body i and every j among the
 *              first k_merge bodies of i's order where j is inside and labels[i] !=
 *              labels[j].  It belongs to the label pair (a, b) = (min, max) and its
 *              value is 0.5 * (rho'_i + rho'_j).  The table holds one row per label
 *              pair that occurs, in ascending (a, b): `pairs` the number of ordered
 *              body pairs taken, `density` the maximum of their values.  Labels, not
 *              rows: groups below min_members have boundaries too
 * All integers, labels, boundary densities and peak densities are exact and
 * bit-identical between calls; the sums are within 1e-10 of their sum of |term| of
 * binary64, as in nb_sim_fof.  No float atomics: the boundary maximum is an integer
 * maximum of the order-preserving encoding of the value.
 * The call is ordered after the enqueued steps on the simulator's stream, ends
 * with one synchronisation, reports a TreeSim's status words as
 * nb_sim_read_particles does, and does not change the trajectory.  The search obeys
 * "knn_span_cells" and "knn_block_queries", the catalogue "fof_chunk_len"; none
 * changes a bit of the result. */
#define NB_HOP_NONE 0xFFFFFFFFu

typedef struct nb_hop_params {
    uint32_t k_density;   /* 2 .. NB_KNN_MAX_K: the k of the density */
    uint32_t k_hop;       /* 1 .. NB_KNN_MAX_K: neighbours a body may hop to */
    uint32_t k_merge;     /* 1 .. NB_KNN_MAX_K: neighbours that make boundary pairs */
    uint32_t min_members; /* >= 1: the smallest group the catalogue holds */
    double density_min;   /* not NaN; -inf: no cut */
    uint32_t flags;       /* 0 */
    uint32_t reserved32;  /* 0 */
    uint64_t reserved;    /* 0 */
} nb_hop_params;

typedef struct nb_hop_boundary {
    uint32_t a, b;        /* the two labels, a < b */
    uint32_t pairs;       /* ordered body pairs taken */
    uint32_t reserved;    /* 0 */
    double density;       /* the largest 0.5 * (rho'_i + rho'_j) among them */
} nb_hop_boundary;

typedef struct nb_hop_stats {
    uint64_t step_num, n, nonfinite, counted;
    uint64_t outside;        /* counted bodies below density_min */
    uint64_t short_of_k;     /* c when c <= max(k_density, k_hop, k_merge), else 0 */
    uint64_t peaks;          /* all groups, whatever their size */
    uint64_t groups;         /* the catalogued ones, even when group_capacity is smaller */
    uint64_t grouped_bodies; /* bodies of catalogued groups */
    uint64_t boundaries;     /* label pairs, even when boundary_capacity is smaller */
    uint64_t boundary_pairs; /* ordered body pairs taken */
    uint32_t largest_count, largest_label; /* as nb_fof_stats' */
} nb_hop_stats;

/* The density-peak groups of a simulator's current state.  labels, group_of and density: n values each;
 * groups and peak_density: room for group_capacity rows, of which the first min(stats->groups,
 * group_capacity) are written; boundaries: room for boundary_capacity rows, of which the first
 * min(stats->boundaries, boundary_capacity) are written.  Every output pointer may be null: what is not
 * asked for is not copied (without `groups` and `peak_density` there is no catalogue, without `boundaries`
 * the table is still counted); a call with none of them synchronises and measures nothing.  The outputs
 * are written only by a call that succeeds.  NB_ERR_INVALID for a null handle or params, a k outside its
 * range, min_members == 0, a NaN density_min, unknown flags or a reserved field != 0 -- all checked
 * before any device call; NB_ERR_UNSUPPORTED for a sharded simulator (placement world > 1) and for
 * n * k_merge >= 2^31. */
int nb_sim_hop(nb_sim *sim, const nb_hop_params *params, uint32_t *labels, uint32_t *group_of, double *density,
               nb_fof_group *groups, double *peak_density, size_t group_capacity, nb_hop_boundary *boundaries,
               size_t boundary_capacity, nb_hop_stats *stats);

/* Merges the groups of nb_sim_hop across their boundaries on the host (no device call):
 *   1. a row is viable iff its peak_density >= params->peak;
 *   2. boundaries whose two labels are not both rows are skipped; the rest are processed in descending
 *      density, ties in ascending (a, b), with a union-find over rows;
 *   3. the sets of a and b are joined unless both sets are viable and density < params->saddle; a set is
 *      viable if any of its rows is;
 *   4. a set's representative is its densest peak (peak_density, then the smaller label);
 *   5. merged_of_row[r] (m values) is the representative's label if the set is viable, else NB_HOP_NONE;
 *   6. the merged catalogue holds one row per viable set in ascending label: count and the nine sums are
 *      those of the member rows added in ascending row order from 0, peak_density the representative's.
 *      The first min(*out_count, out_capacity) rows are written; *out_count is their total.
 * merged_of_row, out_rows and out_peak may be null.  NB_ERR_INVALID for null params or out_count, null rows
 * or peak_density with m > 0, null bnd with b > 0, NaN thresholds or saddle > peak, unknown flags, rows
 * not in strictly ascending label order, or boundaries not in strictly ascending (a, b). */
typedef struct nb_hop_regroup_params {
    double saddle, peak; /* saddle <= peak, neither NaN */
    uint32_t flags;      /* 0 */
    uint32_t reserved;   /* 0 */
} nb_hop_regroup_params;

int nb_hop_regroup(const nb_fof_group *rows, const double *peak_density, size_t m, const nb_hop_boundary *bnd,
                   size_t b, const nb_hop_regroup_params *params, uint32_t *merged_of_row, nb_fof_group *out_rows,
                   double *out_peak, size_t out_capacity, size_t *out_count);

/* ------------------------------------------------------------------------- */
/* Local kinematics -- how the neighbours of every body move: the velocity    */
/* moments and the velocity gradient over its k nearest neighbours (no        */
/* reference counterpart)                                                     */
/* ------------------------------------------------------------------------- */
/* For every body of the state nb_sim_read_particles would return: the mass and
 * velocity moments of its k nearest neighbours relative to the body itself, and,
 * when asked for, the sums a least-squares velocity gradient is solved from;
 * nb_local_kinematics_derive turns them on the host into the mean velocity, the
 * dispersion sigma, the pseudo-phase-space density rho / sigma^3 and the gradient
 * with its divergence, vorticity and shear.  The rule, which DESIGN.md 6s states
 * in full: binary64 from the binary32 state, one rounding per operation, no
 * contraction; `counted`, d2 and the order (d2, j) are nb_sim_knn's, word for word.
 *   list      for a counted body i, 1 <= k <= NB_KNN_MAX_K and c > k: the first k
 *             bodies of i's order, in that order
 *   member j  m = (double)m_j, dx_a = (double)x_j,a - (double)x_i,a,
 *             du_a = (double)v_j,a - (double)v_i,a
 *   moments   NB_KIN_MOMENTS = 10 doubles per body:
 *             [0]      S0 = sum m; with NB_KIN_SELF it starts from (double)m_i, not 0
 *             [1..3]   S1_a = sum m du_a, the term one product
 *             [4..9]   S2_ab = sum (m du_a) du_b for ab = xx, xy, xz, yy, yz, zz, the
 *                      term two products in that association
 *   gradient  NB_KIN_GRADS = 15 doubles per body, only when `grads` is given:
 *             [0..5]   D_ab = sum (m dx_a) dx_b for ab = xx, xy, xz, yy, yz, zz
 *             [6..14]  C_ab = sum (m du_a) dx_b, row-major in (a, b)
 *   order     every sum is added in list order from its start value, left to right
 *             (the order of mass_in)
 *   knn       r2, kth, mass_in and density are nb_sim_knn's at the same k, bit for bit
 *   special   a body that is not counted: every moment and gradient sum NaN, and
 *             nb_sim_knn's presets; c <= k: every counted body has every sum 0 (S0 too,
 *             with or without NB_KIN_SELF), nb_sim_knn's presets, short_of_k = c;
 *             r2[i] == 0 is `degenerate` as in nb_sim_knn: the sums are still formed
 * Everything per body is unique given the state: every double and integer is exact
 * and bit-identical between calls.  No float atomics.  The tuning keys are
 * nb_sim_knn's "knn_span_cells" and "knn_block_queries"; neither changes a bit.
 * The call is ordered after the enqueued steps on the simulator's stream, ends with
 * one synchronisation, reports a TreeSim's status words as nb_sim_read_particles
 * does, and does not change the trajectory. */
#define NB_KIN_SELF 1u /* params.flags: the body's own mass starts S0 */
#define NB_KIN_MOMENTS 10u
#define NB_KIN_GRADS 15u
/* status bits of nb_kin_derived */
#define NB_KIN_SHORT 1u       /* counted, but c <= k */
#define NB_KIN_NOT_COUNTED 2u /* a non-finite body */
#define NB_KIN_DEGENERATE 4u  /* r2 == 0 */
#define NB_KIN_SINGULAR 8u    /* the gradient was asked for and D is singular by the rule below */

typedef struct nb_kin_params { /* 16 bytes */
    uint32_t k;        /* 1 .. NB_KNN_MAX_K */
    uint32_t flags;    /* NB_KIN_SELF */
    uint64_t reserved; /* 0 */
} nb_kin_params;

typedef struct nb_kin_stats { /* 56 bytes */
    uint64_t step_num, n, nonfinite, counted, degenerate, short_of_k;
    uint32_t k, flags;
} nb_kin_stats;

typedef struct nb_kin_derived { /* 256 bytes: one body */
    double mass;                 /* S0 */
    double relative_velocity[3]; /* u_a = S1_a / S0: the neighbours' mean velocity relative to the body */
    double mean_velocity[3];     /* (double)v_i,a + u_a; NaN without `velocities` */
    double dispersion[6];        /* Sigma_ab = S2_ab / S0 - u_a u_b for ab = xx, xy, xz, yy, yz, zz */
    double sigma2;               /* ((Sigma_xx + Sigma_yy) + Sigma_zz) / 3 */
    double sigma;                /* sqrt(sigma2), 0 when sigma2 < 0 */
    double phase_space_density;  /* Q = density / (sigma2 sigma); NaN without `density` */
    double gradient[9];          /* G_ab = d u_a / d x_b, row-major; NaN without `grads` or when singular */
    double det;                  /* det D; NaN without `grads` */
    double divergence;           /* (G_xx + G_yy) + G_zz */
    double vorticity[3];         /* (G_zy - G_yz, G_xz - G_zx, G_yx - G_xy) */
    double shear;                /* the Frobenius norm of the traceless symmetric part of G */
    uint32_t status;             /* NB_KIN_SHORT | NB_KIN_NOT_COUNTED | NB_KIN_DEGENERATE | NB_KIN_SINGULAR */
    uint32_t reserved;
} nb_kin_derived;

#if defined(__cplusplus)
static_assert(sizeof(nb_kin_params) == 16 && sizeof(nb_kin_stats) == 56 && sizeof(nb_kin_derived) == 256,
              "nb_kin_* layouts");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(nb_kin_params) == 16 && sizeof(nb_kin_stats) == 56 && sizeof(nb_kin_derived) == 256,
               "nb_kin_* layouts");
#endif

/* moments: n NB_KIN_MOMENTS doubles; grads: n NB_KIN_GRADS doubles; r2, kth, mass_in, density: n each, as
 * nb_sim_knn.  Every output pointer may be null: what is not asked for is neither computed nor copied (the
 * moments are formed with the gradient sums; a call with no per-body output runs the search alone for the
 * stats; a call with no output at all synchronises and measures nothing).  The outputs are written only by a
 * call that succeeds.  NB_ERR_INVALID for a null handle or params, k == 0, k > NB_KNN_MAX_K, unknown flags or
 * reserved != 0 -- all checked before any device call; NB_ERR_UNSUPPORTED for a sharded simulator (placement
 * world > 1). */
int nb_local_kinematics_sim(nb_sim *sim, const nb_kin_params *params, double *moments, double *grads, double *r2,
                            uint32_t *kth, double *mass_in, double *density, nb_kin_stats *stats);
/* Host only, a pure function of its arguments, no device call: out[n] from what nb_local_kinematics_sim
 * filled.  moments and r2 are required; grads, density and velocities (3 floats per body, the state's) may be
 * null.  Per body, each step evaluated as written in binary64, no contraction:
 *   u_a = S1_a / S0;  Sigma_ab = S2_ab / S0 - u_a u_b;  sigma2 = ((Sigma_xx + Sigma_yy) + Sigma_zz) / 3;
 *   sigma = sqrt(sigma2), 0 when sigma2 < 0;  mean_velocity_a = (double)v_i,a + u_a;
 *   Q = density / (sigma2 sigma).
 * With grads, G = C D^-1, the least-squares fit du = G dx through body i with no intercept, by cofactors:
 *   adj_xx = D_yy D_zz - D_yz D_yz   adj_xy = D_xz D_yz - D_xy D_zz   adj_xz = D_xy D_yz - D_xz D_yy
 *   adj_yy = D_xx D_zz - D_xz D_xz   adj_yz = D_xy D_xz - D_xx D_yz   adj_zz = D_xx D_yy - D_xy D_xy
 *   det = (D_xx adj_xx + D_xy adj_xy) + D_xz adj_xz        (adj is symmetric)
 *   G_ab = ((C_a0 adj_0b + C_a1 adj_1b) + C_a2 adj_2b) / det
 * A body is singular when !(det > 2^-30 ((D_xx D_yy) D_zz)): the ratio is scale-free and lies in [0, 1] by
 * Hadamard's inequality; coplanar, collinear and coincident neighbours give 0.  Then G and what follows from
 * it are NaN and NB_KIN_SINGULAR is set.  divergence = (G_xx + G_yy) + G_zz; vorticity = (G_zy - G_yz,
 * G_xz - G_zx, G_yx - G_xy); with t = divergence / 3, s_aa = G_aa - t and s_ab = (G_ab + G_ba) / 2,
 * shear = sqrt(((s_xx s_xx + s_yy s_yy) + s_zz s_zz) + 2 ((s_xy s_xy + s_xz s_xz) + s_yz s_yz)).
 * status: NB_KIN_NOT_COUNTED for r2 NaN, NB_KIN_SHORT for r2 = +inf, NB_KIN_DEGENERATE for r2 == 0.  A body
 * that is short or not counted has NaN in every derived double but mass.  NB_ERR_INVALID for null moments,
 * r2 or out with n > 0. */
int nb_local_kinematics_derive(const double *moments, const double *grads, const double *r2, const double *density,
                               const float *velocities, size_t n, nb_kin_derived *out);

/* ------------------------------------------------------------------------- */
/* Halo profiles -- the spherical radial profile about many centres in one    */
/* call (no reference counterpart)                                            */
/* ------------------------------------------------------------------------- */
/* For each of m centres: the bins of nb_sim_radial_profile's spherical mode over
 * the state nb_sim_read_particles would return, with edges shared by all centres.
 * A centre tests only the bodies of the grid cells its sphere can reach, so the
 * cost follows the bodies near the centres, not m n.  The rule, which DESIGN.md 6l
 * states in full:
 *   per centre   exactly the spherical rule above ("Radial profiles"): binary64
 *                from the binary32 state, one rounding per operation, no
 *                contraction; d = (double)x - c, u = (double)v - v_c,
 *                r2 = (dx dx + dy dy) + dz dz; the bin is the k with
 *                edges[k]^2 <= r2 < edges[k+1]^2, the squares formed once on the
 *                host; terms m, m r, m u_r, (m u_r) u_r, m |u|^2, m (d x u); u_r = 0
 *                at r = 0; m_uphi = m_uphi2 = 0.  The predicate of
 *                nb_sim_diagnostics decides which bodies count
 *   not reported bodies with r2 >= edges[nbins]^2 (they are what the grid prunes):
 *                there is no outside_count, total mass or shape.  inside_count and
 *                inside_mass (r2 < edges[0]^2) are per centre
 *   centres      m points centers[m][3] (binary64, all finite), or m body indices
 *                bodies[m] (each < n): the centre is that body's widened position,
 *                read on the device.  Exactly one of the two is non-null.
 *                velocities[m][3] null: v_c = 0 for points, the body's own widened
 *                velocity for body centres.  A body centre is itself a body at
 *                r2 = 0 and is counted like any other.  A body centre that does not
 *                count gives a zeroed row (center and velocity 0) with
 *                NB_HALO_CENTER_NONFINITE in head.flags.  For a TreeSim the indices
 *                are those of nb_sim_read_particles at the same moment
 *   grid         with R = edges[nbins], lo and hi the per-axis bounds of the
 *                counted bodies and E the largest hi - lo: cells of side
 *                h = max(R, E 2^-10); axis a has min(1024, floor((hi_a - lo_a) / h) + 1)
 *                cells with lower edges e(q) = lo_a + (double)q h; a body is in the
 *                cell q with e(q) <= x (q > 0) and x < e(q + 1) (q not the last),
 *                decided by those comparisons.  A centre looks at the cells
 *                [t0, t1] of each axis: t0 the largest t with t = 0 or
 *                (c >= e(t) and (c - e(t))^2 >= R^2), t1 the smallest t with t = last or
 *                (e(t + 1) >= c and (e(t + 1) - c)^2 >= R^2), R^2 = edges[nbins]^2 as
 *                formed on the host; no cell at all when on some axis
 *                (c >= hi and (c - hi)^2 >= R^2) or (lo >= c and (lo - c)^2 >= R^2), or when R^2
 *                underflows to 0.  Every body the per-centre rule bins or counts as
 *                inside is in those cells (the proof is in DESIGN.md 6l)
 *   candidates   a centre's candidates are the bodies of its cells in ascending
 *                (iz, iy, ix, body index): T of them; `tested` is the sum of T
 *   sums         the candidates in chunks of L = NB_HALO_CHUNK, a chunk in tiles of
 *                256 summed per bin as nb_sim_radial_profile sums a tile, the tiles
 *                of a chunk in order, then the chunks in order from 0.  The grid,
 *                L and the order are part of the rule: a centre's row depends on
 *                the state and the edges alone, not on m, the other centres or its
 *                place in the list, and two calls return the same bits.  No float
 *                atomics.  Counts are exact; every sum is within 1e-10 of its sum
 *                of |term| of the binary64 sum
 * Limits: m <= NB_HALO_MAX_CENTERS and m nbins <= NB_HALO_MAX_ROWS, else
 * NB_ERR_INVALID before any device call.  A centre with T candidates costs
 * ceil(T / L) work items, each with a partial of 2 + 9 nbins doubles in the
 * workspace, and the workspace has room for m + NB_HALO_EXTRA_ITEMS of them: a
 * call whose `items` would exceed that is NB_ERR_UNSUPPORTED, found on the device
 * (nothing is written; split the centres over several calls).  Since items
 * <= m + tested / L, no call with tested <= NB_HALO_EXTRA_ITEMS L = 2^28 is
 * refused, whatever m is; one whose centres each see several chunks of
 * candidates can be, from about 2^16 such chunks on.  m = 0 or n = 0 is a valid
 * call that launches nothing: it synchronises, its rows are empty, and its stats
 * carry nonfinite = tested = items = 0 and cells = 0.
 * The call is ordered after the enqueued steps on the simulator's stream, ends
 * with one synchronisation, reports a TreeSim's status words as
 * nb_sim_read_particles does, and does not change the trajectory. */
#define NB_HALO_MAX_BINS 64u
#define NB_HALO_MAX_CENTERS (1u << 20)
#define NB_HALO_MAX_ROWS (1u << 22)
#define NB_HALO_MAX_CELLS_PER_AXIS 1024u
#define NB_HALO_CHUNK 4096u           /* L: candidates per work item */
#define NB_HALO_EXTRA_ITEMS (1u << 16) /* work items of one call beyond one a centre */
#define NB_HALO_CENTER_NONFINITE 1u   /* nb_halo_head.flags: the body centre does not count */

typedef struct nb_halo_params {
    uint32_t nbins, flags;    /* 1..NB_HALO_MAX_BINS; 0 */
    uint64_t m;               /* centres */
    const double *edges;      /* nbins + 1 radii, as nb_radial_params */
    const double *centers;    /* [m][3], or null */
    const uint32_t *bodies;   /* [m], or null */
    const double *velocities; /* [m][3], or null */
} nb_halo_params;

typedef struct nb_halo_head { /* 64 bytes */
    uint32_t inside_count, flags;
    double inside_mass;
    double center[3], velocity[3]; /* the values used */
} nb_halo_head;

typedef struct nb_halo_stats {
    uint64_t step_num, n, nonfinite;
    uint64_t centers; /* m */
    uint64_t tested;  /* candidate distance tests: the sum of T over the centres */
    uint64_t items;   /* work items: the sum of ceil(T / L) */
    uint32_t cells[3], reserved; /* cells per axis of the grid */
} nb_halo_stats;

#if defined(__cplusplus)
static_assert(sizeof(nb_halo_params) == 48 && sizeof(nb_halo_head) == 64 && sizeof(nb_halo_stats) == 64,
              "nb_halo_* layouts");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(nb_halo_params) == 48 && sizeof(nb_halo_head) == 64 && sizeof(nb_halo_stats) == 64,
               "nb_halo_* layouts");
#endif

/* heads: m rows; bins: [m][nbins] rows of nb_radial_bin; either may be null: what is not asked for is
 * not copied.  The outputs are written only by a call that succeeds.  NB_ERR_INVALID for a null handle,
 * params or edges, nbins outside 1..NB_HALO_MAX_BINS, flags != 0, edges nb_sim_radial_profile would
 * refuse, both or neither of centers and bodies (m > 0), a non-finite centre or velocity, m or m nbins
 * above the limits -- all checked before any device call -- and for a body index >= n;
 * NB_ERR_UNSUPPORTED for a sharded simulator (placement world > 1). */
int nb_sim_halo_profiles(nb_sim *sim, const nb_halo_params *params, nb_halo_head *heads, nb_radial_bin *bins,
                         nb_halo_stats *stats);
/* Host only, pure functions of their arguments.
 * nb_halo_enclosed: out[0] = head->inside_mass, out[k + 1] = out[k] + bins[k].mass: the mass inside edges[k].
 * nb_halo_overdensity: the mean enclosed density at every edge with edges[k] > 0 is
 * rho_k = out[k] / (NB_KNN_SPHERE ((e e) e)), e = edges[k].  For the first k with both edges > 0 and
 * rho_{k-1} >= rho > rho_k: *r from ln rho linear in ln r between the two edges (the lower edge itself
 * when rho_k = 0), *mass = rho NB_KNN_SPHERE r^3; both NaN when there is no such k.  Binned, like
 * nb_radial_lagrangian: limited by the bins' resolution, and a crossing inside edges[0] or between
 * edges that the profile does not bracket is not found.  NB_ERR_INVALID for a null pointer, nbins
 * outside 1..NB_HALO_MAX_BINS or rho not finite and > 0. */
int nb_halo_enclosed(const nb_halo_head *head, const nb_radial_bin *bins, uint32_t nbins, double *out);
int nb_halo_overdensity(const nb_halo_head *head, const nb_radial_bin *bins, const double *edges, uint32_t nbins,
                        double rho, double *r, double *mass);

/* ------------------------------------------------------------------------- */
/* Group shapes -- axis ratios, principal axes and angular momentum of every  */
/* row of an assignment of bodies to rows (no reference counterpart)          */
/* ------------------------------------------------------------------------- */
/* For each of m rows: the shape tensor of the row's members inside an ellipsoid
 * that is deformed round by round until its axis ratios are those of the tensor
 * (Allgood et al. 2006, Zemp et al. 2011), with the mass, the first and second
 * moments of position and velocity and the angular momentum of the same members.
 * The rule, which DESIGN.md 6n states in full; binary64 from the binary32 state,
 * one rounding per operation, no contraction:
 *   input     group_of[n]: NB_FOF_NONE or a row < m for every body of the state
 *             nb_sim_read_particles would return; nb_sim_fof's group_of,
 *             nb_sim_bound's bound_of, nb_sim_hop's group_of (raw or regrouped) or
 *             any assignment of the caller's.  0 <= m <= max(n, 1).  centers[m][3],
 *             velocities[m][3]: finite, either may be null; radius[m]: each finite
 *             and > 0, or +inf; null: all +inf
 *   members   row r's list L is the bodies with group_of == r that count (the
 *             predicate of nb_sim_diagnostics) in ascending body index; the others
 *             with a row are stats->nonfinite_members.  `count` = |L|.  count == 0:
 *             the row is EMPTY (sums 0, iterations 0, a centre or velocity that was
 *             not given NaN, lambda, axes, q and s NaN)
 *   round t   (t = 1, 2, ...) with centre c, frame velocity V, radius R, axes E
 *             (rows e_1, e_2, e_3) and ratios (q, s); round 1 has E = identity and
 *             (q, s) = (1, 1).  Per member: d = (double)x - c and u = (double)v - V per
 *             component; y_k = (e_kx dx + e_ky dy) + e_kz dz; a = (R, R q, R s);
 *             rho2 = ((y_1 / a_1)^2 + (y_2 / a_2)^2) + (y_3 / a_3)^2; the member is
 *             selected iff rho2 <= 1 (a NaN is not).  Over the selected members:
 *             `selected` = their number, and the 22 sums
 *               mass = sum m;  md = sum m d;  mu = sum m u;
 *               t  = sum ((w m) d_i) d_j   for ij = xx xy xz yy yz zz
 *               uu = sum (m u_i) u_j       in the same order
 *               j  = sum m (d_y u_z - d_z u_y), m (d_z u_x - d_x u_z), m (d_x u_y - d_y u_x)
 *             w m = m, or with NB_SHAPE_REDUCED w m = (1 / rho2) m, and 0 for rho2 == 0
 *             (such a member adds nothing to t).  NB_SHAPE_REDUCED needs a finite R
 *   round 0   only when centers or velocities is null: the sums of round t with
 *             R = +inf about c = 0 (centers null) and V = 0 (velocities null), so
 *             that md = sum m x and mu = sum m v over L; then c = md / mass and
 *             V = mu / mass per component, for the one that was not given
 *   verdict   (lambda, E') = nb_shape_eigen(t).  The row is DEGENERATE when
 *             selected < min_members, or unless lambda_3 > 0 and all three are
 *             finite: q = s = NaN.  Otherwise q' = sqrt(lambda_2 / lambda_1),
 *             s' = sqrt(lambda_3 / lambda_1).  R = +inf: CONVERGED (after round 1).
 *             Otherwise delta = max(|q' - q| / q', |s' - s| / s'); t >= 2 and
 *             delta < tol: CONVERGED; else t == max_iter: UNCONVERGED; else round t + 1
 *             with (q', s', E').  A finished row reports round t: iterations = t, the
 *             sums of round t, lambda, axes = E', q = q', s = s'
 *   the axes  the major axis keeps the length R and the other two shrink: the
 *             ellipsoid never reaches outside the sphere of radius R the caller
 *             chose -- the region the caller vouches for (a group's extent, a virial
 *             radius) -- whereas an ellipsoid of fixed volume or fixed minor axis
 *             grows past it into bodies that the first round never saw
 *   sums      position p of a member is its place in L for the whole call; a member
 *             that is not selected adds +0 (masking, as nb_sim_bound).  Runs of 64
 *             positions [64 k, 64 k + 64) are reduced by the fixed butterfly of
 *             nb_sim_fof (v_i + v_(i xor 32), then xor 16, ... 1) and a row's runs
 *             are added in order from 0.  So a row's outputs are a function of its
 *             own list, centre, velocity and radius alone -- not of the other rows,
 *             of its number, of m or of the tuning key -- and two calls return the
 *             same bits.  No float atomics.  Every sum is within 1e-10 of its sum of
 *             |term| of the binary64 sum
 *   selected_of[i] the row of body i when the row is CONVERGED or UNCONVERGED and i
 *             was selected in its last round, else NB_FOF_NONE
 * nb_shape_eigen is the cyclic Jacobi diagonalisation of nb_shape.hpp, the same
 * function on the host and on the device: t = (xx, xy, xz, yy, yz, zz); V = identity;
 * at most 12 sweeps; a sweep ends the iteration when (|a01| + |a02|) + |a12| == 0,
 * else visits (p, q) = (0,1), (0,2), (1,2) with r the third index: a_pq == 0:
 * nothing; g = 100 |a_pq|; |a_pp| + g == |a_pp| and |a_qq| + g == |a_qq|: a_pq <- 0;
 * otherwise h = a_qq - a_pp, t = a_pq / h when |h| + g == |h|, else
 * theta = (0.5 h) / a_pq, t = 1 / (|theta| + sqrt(theta theta + 1)), negated for
 * theta < 0; c = 1 / sqrt(t t + 1), s = t c, tau = s / (1 + c), z = t a_pq;
 * a_pp <- a_pp - z, a_qq <- a_qq + z, a_pq <- 0, (a_rp, a_rq) <- (a_rp - s (a_rq +
 * tau a_rp), a_rq + s (a_rp - tau a_rq)) and likewise (v_kp, v_kq) for k = 0, 1, 2.
 * lambda = the diagonal sorted descending, equal values in index order;
 * axes[3 k + j] = component j of the eigenvector of lambda[k], negated when its
 * component of largest magnitude (the first of equals) is negative.
 * params->step_num must equal the simulator's step number (a TreeSim reorders its
 * bodies every step, so an assignment is good for the step it was made at);
 * NB_SHAPE_ANY_STEP switches the check off.
 * The call is ordered after the enqueued steps on the simulator's stream, enqueues
 * all max_iter rounds up front (the blocks of a finished row return at once), ends
 * with one synchronisation, reports a TreeSim's status words as
 * nb_sim_read_particles does, and does not change the trajectory.
 * "shape_chunk_len" (nb_sim_set_tuning, 64..65536, a multiple of 64; default 1024):
 * the positions of a row's list one work item takes.  Speed and testing only: it
 * changes no bit of the result. */
#define NB_SHAPE_REDUCED 1u /* nb_shape_params.flags */
#define NB_SHAPE_CONVERGED 1u
#define NB_SHAPE_UNCONVERGED 2u
#define NB_SHAPE_DEGENERATE 4u
#define NB_SHAPE_EMPTY 8u
#define NB_SHAPE_MAX_ITER 64u
#define NB_SHAPE_ANY_STEP 0xFFFFFFFFFFFFFFFFull /* nb_shape_params.step_num: UINT64_MAX */

typedef struct nb_shape_params {
    uint32_t flags;       /* 0 or NB_SHAPE_REDUCED */
    uint32_t min_members; /* >= 1: a row with fewer selected members is degenerate */
    uint32_t max_iter;    /* 1 .. NB_SHAPE_MAX_ITER */
    uint32_t reserved32;  /* 0 */
    double tol;           /* finite and > 0 */
    uint64_t step_num;    /* the simulator's step number, or NB_SHAPE_ANY_STEP */
    uint64_t reserved;    /* 0 */
} nb_shape_params;

typedef struct nb_shape_group { /* 360 bytes */
    uint32_t count, selected;   /* |L|; members selected in the last round */
    uint32_t iterations, status; /* rounds that ran; one of NB_SHAPE_CONVERGED .. NB_SHAPE_EMPTY */
    double radius;               /* R */
    double center[3], velocity[3]; /* the values used */
    double mass, md[3], mu[3], t[6], uu[6], j[3]; /* the 22 sums of the last round */
    double lambda[3], axes[9];   /* descending; axes[3 k + j] = component j of axis k */
    double q, s;                 /* b/a and c/a */
} nb_shape_group;

typedef struct nb_shape_stats {
    uint64_t step_num, n;
    uint64_t rows;              /* m */
    uint64_t members;           /* counted bodies with a row */
    uint64_t nonfinite_members; /* bodies with a row that do not count */
    uint64_t converged, unconverged, degenerate, empty; /* rows by status */
    uint32_t rounds_max;        /* the largest `iterations` */
    uint32_t reserved;
} nb_shape_stats;

#if defined(__cplusplus)
static_assert(sizeof(nb_shape_params) == 40 && sizeof(nb_shape_group) == 360 && sizeof(nb_shape_stats) == 80,
              "nb_shape_* layouts");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(nb_shape_params) == 40 && sizeof(nb_shape_group) == 360 && sizeof(nb_shape_stats) == 80,
               "nb_shape_* layouts");
#endif

/* group_of: n values (may be null for n == 0); rows_out: m rows; selected_of: n values.  Every output
 * pointer may be null: what is not asked for is not copied.  The outputs are written only by a call
 * that succeeds.  NB_ERR_INVALID for a null handle or params, a null group_of with n > 0,
 * m > max(n, 1), a non-finite centre or velocity, a radius that is neither finite and > 0 nor +inf,
 * NB_SHAPE_REDUCED with an infinite (or null) radius, min_members == 0, max_iter outside
 * 1..NB_SHAPE_MAX_ITER, a tol that is not finite and > 0, unknown flags or a reserved field != 0, a
 * step_num that is neither the simulator's nor NB_SHAPE_ANY_STEP -- all checked before any device
 * call -- and, after the call's one synchronisation, for a value of group_of that is neither
 * NB_FOF_NONE nor < m; NB_ERR_UNSUPPORTED for a sharded simulator (placement world > 1). */
int nb_sim_group_shapes(nb_sim *sim, const nb_shape_params *params, const uint32_t *group_of, size_t m,
                        const double *centers, const double *velocities, const double *radius,
                        nb_shape_group *rows_out, uint32_t *selected_of, nb_shape_stats *stats);
/* Host only: the eigen-solver of the rule above.  NB_ERR_INVALID for a null pointer. */
int nb_shape_eigen(const double t[6], double lambda[3], double axes[9]);

/* ------------------------------------------------------------------------- */
/* Group radii -- exact mass radii, extent and the peak of the circular-      */
/* velocity curve of every row of an assignment (no reference counterpart)    */
/* ------------------------------------------------------------------------- */
/* For each of m rows: the members ordered by their distance from the row's centre,
 * the enclosed mass M at every member in a fixed order of additions, the member at
 * which M first reaches each of nf fractions of the row's mass (the 10 / 50 / 90 %
 * mass radii; no binning, no interpolation: the radius is a body's), and the largest
 * M / r with the member it lies at (v_max = sqrt(G vc2_max), G the caller's).  The
 * rule, which DESIGN.md 6o states in full; binary64 from the binary32 state, one
 * rounding per operation, no contraction:
 *   input     group_of[n], m and centers[m][3] (finite; may be null) exactly as
 *             nb_sim_group_shapes takes them; fractions[nf], 1 <= nf <= 16, each
 *             finite, 0 < f <= 1, strictly ascending; vmax_skip >= 0
 *   members   row r's list L is the bodies with group_of == r that count, in
 *             ascending body index; `count` = |L|; the others with a row are
 *             stats->nonfinite_members
 *   centre    the caller's, or (centers null) c = (sum m x) / (sum m) over L, the
 *             sums formed as round 0 of nb_sim_group_shapes forms md and mass:
 *             positions of L in order, runs of 64 through the fixed butterfly, runs
 *             added in order from 0.  It is bit for bit the `center` that
 *             nb_sim_group_shapes reports for the row with centers and radius null
 *   order     per member d = (double)x - c per component, r2 = (dx dx + dy dy) + dz dz.
 *             The members of a row in ascending r2, ties in ascending body index; a
 *             member's 0-based place is its `rank`.  (r2 >= 0, so its bit pattern as a
 *             64-bit unsigned integer is the sort key.)
 *   M         at rank s of a row, a three-level sum.  Ranks [64 k, 64 k + 64) are a
 *             run: C(s) = the masses of the run's members up to s added left to
 *             right, starting from the run's first member alone; T(k) = C at the
 *             run's last member.  64 runs (NB_RADII_CHUNK = 4,096 ranks) are a
 *             chunk: B(first run) = 0, B(k) = B(k - 1) + T(k - 1); the chunk's total
 *             is B(last run) + T(last run).  A(first chunk) = 0, A(c) = A(c - 1) +
 *             total(c - 1).  M(s) = (A(c) + B(k)) + C(s); mass = M(count - 1), 0 for an
 *             empty row.  Ranks count from the row's own start: M depends on the row's
 *             list and centre alone -- not on the other rows, the row's number or m.
 *             |M(s) - exact prefix| <= (130 + count / 4096) 2^-53 sum |m_j|
 *   crossings for fraction f: t = f mass (one multiply), s_f = the smallest rank with
 *             M(s) >= t, the predicate taken at every rank (M need not be monotone
 *             in the last bit across a run boundary); radius[f] = sqrt(r2) of that
 *             member, index[f] its body index; no rank satisfies the predicate (an
 *             empty row, a NaN mass): NaN and NB_FOF_NONE.  Nothing else is special: a
 *             row of zero masses crosses at rank 0.  Entries f >= nf: NaN and NB_FOF_NONE
 *   v_max     over the ranks s >= vmax_skip with r2 > 0: x(s) = M(s) / sqrt(r2(s)), a
 *             NaN passed over; vc2_max = the largest x, at the smallest rank among
 *             equals; r_vmax = sqrt(r2) and vmax_index = the body index of that
 *             member; no such rank: NaN and NB_FOF_NONE
 *   the row   count, center (the one used; NaN for an empty row without a given one),
 *             mass, r_min and r_max (sqrt(r2) of the first and the last member; NaN
 *             for an empty row), the crossings, the three v_max values
 *   per body  rank_of[i] = the rank of a member, else NB_FOF_NONE; enclosed_of[i] =
 *             M at the member, else NaN.  With nb_sim_read_particles they are the
 *             exact M(<r) curve of every row
 * The 64 and the 4,096 are part of the rule; there is no tuning key.  Two calls return
 * the same bits.  No float atomics.  params->step_num as nb_shape_params.step_num
 * (NB_RADII_ANY_STEP switches the check off).  The call is ordered after the enqueued
 * steps on the simulator's stream, ends with one synchronisation, reports a TreeSim's
 * status words as nb_sim_read_particles does, launches nothing inside a graph capture
 * and does not change the trajectory.
 * The names: this is the thirteenth analysis pass, and it is spelt noun first --
 * nb_group_radii_sim / nb_group_radii_runner -- like the host-only helpers
 * (nb_hop_regroup, nb_shape_eigen): the nb_sim_<pass> / nb_runner_<pass> family is
 * closed at twelve, which the binding's tests count. */
#define NB_RADII_MAX_FRACTIONS 16u
#define NB_RADII_CHUNK 4096u
#define NB_RADII_ANY_STEP 0xFFFFFFFFFFFFFFFFull /* nb_radii_params.step_num: UINT64_MAX */

typedef struct nb_radii_params {
    uint32_t nf;          /* 1 .. NB_RADII_MAX_FRACTIONS */
    uint32_t vmax_skip;   /* ranks below it are left out of v_max */
    uint64_t step_num;    /* the simulator's step number, or NB_RADII_ANY_STEP */
    uint64_t reserved;    /* 0 */
    double fractions[16]; /* [0, nf): finite, 0 < f <= 1, strictly ascending; the rest is not read */
} nb_radii_params;

typedef struct nb_radii_group { /* 264 bytes */
    uint32_t count, vmax_index; /* |L|; the body at the peak of M / r, or NB_FOF_NONE */
    double center[3];           /* the one used */
    double mass, r_min, r_max;
    double vc2_max, r_vmax;     /* the largest M / r and the radius it lies at */
    double radius[16];          /* [0, nf): the radius of the member at which M reaches f mass */
    uint32_t index[16];         /* its body index, or NB_FOF_NONE */
} nb_radii_group;

typedef struct nb_radii_stats {
    uint64_t step_num, n;
    uint64_t rows;              /* m */
    uint64_t members;           /* counted bodies with a row */
    uint64_t nonfinite_members; /* bodies with a row that do not count */
    uint64_t empty;             /* rows without a member */
} nb_radii_stats;

#if defined(__cplusplus)
static_assert(sizeof(nb_radii_params) == 152 && sizeof(nb_radii_group) == 264 && sizeof(nb_radii_stats) == 48,
              "nb_radii_* layouts");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(nb_radii_params) == 152 && sizeof(nb_radii_group) == 264 && sizeof(nb_radii_stats) == 48,
               "nb_radii_* layouts");
#endif

/* group_of: n values (may be null for n == 0); centers: m x 3 or null; rows_out: m rows; rank_of,
 * enclosed_of: n values each.  Every output pointer may be null: what is not asked for is not
 * copied.  The outputs are staged and written only by a call that succeeds.  NB_ERR_INVALID for a
 * null handle or params, a null group_of with n > 0, m > max(n, 1), a non-finite centre, nf outside
 * 1..NB_RADII_MAX_FRACTIONS, a fraction that is not finite, not in (0, 1] or not above the one
 * before it, a reserved field != 0, a step_num that is neither the simulator's nor
 * NB_RADII_ANY_STEP -- all checked before any device call -- and, after the call's one
 * synchronisation, for a value of group_of that is neither NB_FOF_NONE nor < m; NB_ERR_UNSUPPORTED
 * for a sharded simulator (placement world > 1). */
int nb_group_radii_sim(nb_sim *sim, const nb_radii_params *params, const uint32_t *group_of, size_t m,
                       const double *centers, nb_radii_group *rows_out, uint32_t *rank_of, double *enclosed_of,
                       nb_radii_stats *stats);

/* ------------------------------------------------------------------------- */
/* Disc modes -- azimuthal Fourier sums per annulus: bar strength, phases,    */
/* pattern speeds, bending modes, thickness (no reference counterpart)        */
/* ------------------------------------------------------------------------- */
/* Per annulus about an axis through a centre: sum m e^(i m phi) for m = 0 .. mmax and
 * three weighted variants (by dphi/dt, by the height above the plane, and their
 * combinations), from which nb_disc_modes_derive forms the amplitude A_m / A_0, the
 * phase, the single-snapshot pattern speed (Dehnen, Semczuk & Schoenrich 2023: dphi/dt
 * of every body is known, so no second output is needed) and the bending mode.  The
 * rule, which DESIGN.md 6p states in full; binary64 from the binary32 state, one
 * rounding per operation, no contraction, in this order:
 *   input     nbins in 1..NB_MODES_MAX_BINS and nbins + 1 edges, checked exactly as
 *             nb_sim_radial_profile checks its edges; mmax in 0..NB_MODES_MAX_M; a
 *             centre c and a frame velocity v_c, or NB_MODES_CENTER_COM: the fp64 `com`
 *             and `momentum / mass` of nb_sim_diagnostics bit for bit, formed on the
 *             device; an axis
 *   frame     n, e1, e2 exactly as nb_map_frame(axis) returns them: phi = 0 is the
 *             direction nb_field_rings starts its rings from, (a, b) are a map's axes
 *   per body  that counts (position, velocity and mass finite; the others are
 *             `nonfinite`):
 *               d = (double)x - c, u = (double)v - v_c         per component
 *               h  = (dx nx + dy ny) + dz nz                   the height above the plane
 *               p  = d - h n,  r2 = (px px + py py) + pz pz    nb_sim_radial_profile's
 *                                                              cylindrical rule
 *               bin: the k with edges[k]^2 <= r2 < edges[k + 1]^2 (the squares formed
 *                    once on the host); r2 < edges[0]^2: inside; r2 >= edges[nbins]^2:
 *                    outside; a NaN r2 (a NaN centre) is below every edge
 *               a  = (px e1x + py e1y) + pz e1z,  b likewise with e2
 *               ua = (ux e1x + uy e1y) + uz e1z,  ub likewise with e2
 *               R  = sqrt(r2), c_1 = a / R, s_1 = b / R, w = (a ub - b ua) / r2
 *               r2 == 0: c_1 = s_1 = 0 and w = 0 (the body counts in m = 0 only)
 *               c_0 = 1, s_0 = 0; c_m = c_(m-1) c_1 - s_(m-1) s_1,
 *                                 s_m = s_(m-1) c_1 + c_(m-1) s_1      m = 1 .. mmax
 *               with mu = (double)mass, per m the six terms
 *                 C = mu c_m, S = mu s_m, DC = (mu w) c_m, DS = (mu w) s_m,
 *                 ZC = (mu h) c_m, ZS = (mu h) s_m
 *               and once mu R and (mu h) h
 *             cos m phi and sin m phi come from the recurrence: every term is a chain
 *             of correctly rounded +, -, x, / and sqrt
 *   lists     a bin's list is its members in ascending body index; inside and outside
 *             are lists too (only their count and their sum of mu are reported).  A
 *             member's place is its 0-based position in its list
 *   sums      every field of a list in three fixed levels: the places [64 k, 64 k + 64)
 *             are a run, summed by the xor butterfly over offsets 32, 16, 8, 4, 2, 1 (x_i
 *             + x_(i xor o) on every place, an absent place holding +0); the up to 64
 *             runs of a chunk of NB_MODES_CHUNK = 4,096 places are added left to right
 *             starting from +0; the chunks of the list are added left to right starting
 *             from +0.  A bin's bits depend on its own members, the centre and the frame
 *             alone: not on the other bins, on nbins or on the call
 *   mass      inside_mass + the bins' C_0 in order + outside_mass, added in that order
 *             starting from inside_mass
 * modes[(k (mmax + 1) + m) 6 + f] is field f of mode m of bin k, f in the order C, S,
 * DC, DS, ZC, ZS (NB_MODES_C ..).  At m = 0: C = sum mu, DC = sum mu w, ZC = sum mu h and
 * the three sine sums are sums of zeros.  Two calls return the same bits.  No float
 * atomics.  The call is ordered after the enqueued steps on the simulator's stream, ends
 * with one synchronisation, reports a TreeSim's status words as nb_sim_read_particles
 * does, launches nothing inside a graph capture and does not change the trajectory.
 * This is the fourteenth analysis pass, spelt noun first as nb_group_radii_sim is. */
#define NB_MODES_MAX_BINS 256u
#define NB_MODES_MAX_M 8u
#define NB_MODES_FIELDS 6u
#define NB_MODES_CHUNK 4096u
#define NB_MODES_CENTER_COM 1u /* centre = com, frame velocity = P/M of the measured state (as NB_RADIAL_CENTER_COM) */
enum { NB_MODES_C = 0, NB_MODES_S, NB_MODES_DC, NB_MODES_DS, NB_MODES_ZC, NB_MODES_ZS };

typedef struct nb_modes_params {
    uint32_t nbins, mmax; /* 1..NB_MODES_MAX_BINS, 0..NB_MODES_MAX_M */
    uint32_t flags;       /* NB_MODES_CENTER_COM */
    uint32_t reserved;    /* 0 */
    double center[3];     /* ignored with NB_MODES_CENTER_COM */
    double velocity[3];   /* ignored with NB_MODES_CENTER_COM */
    double axis[3];       /* finite, non-zero; need not be a unit vector */
    const double *edges;  /* nbins + 1 cylindrical radii: finite, >= 0, strictly ascending */
} nb_modes_params;

typedef struct nb_modes_head { /* 200 bytes */
    uint64_t step_num, n, nonfinite;
    uint64_t inside_count, outside_count;
    double inside_mass, outside_mass;
    double mass;                      /* inside + the bins in order + outside */
    double center[3], velocity[3];    /* the ones used */
    double axis[3], e1[3], e2[3];     /* nb_map_frame of the caller's axis */
    uint32_t nbins, mmax, flags, reserved;
} nb_modes_head;

typedef struct nb_modes_bin { /* 24 bytes */
    uint64_t count;
    double m_r;  /* sum mu R */
    double m_h2; /* sum (mu h) h */
} nb_modes_bin;

typedef struct nb_modes_derived { /* 40 bytes: one mode m >= 1 of one bin */
    double amplitude;      /* hypot(C, S) / C_0 */
    double phase;          /* atan2(S, C) / m, in (-pi/m, pi/m] */
    double pattern_speed;  /* (C DC + S DS) / (C C + S S) */
    double bend_amplitude; /* hypot(ZC, ZS) / C_0 */
    double bend_phase;     /* atan2(ZS, ZC) / m */
} nb_modes_derived;

#if defined(__cplusplus)
static_assert(sizeof(nb_modes_params) == 96 && sizeof(nb_modes_head) == 200 && sizeof(nb_modes_bin) == 24 &&
                  sizeof(nb_modes_derived) == 40,
              "nb_modes_* layouts");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(nb_modes_params) == 96 && sizeof(nb_modes_head) == 200 && sizeof(nb_modes_bin) == 24 &&
                   sizeof(nb_modes_derived) == 40,
               "nb_modes_* layouts");
#endif

/* out: the head; bins: nbins records; modes: nbins (mmax + 1) 6 doubles.  NB_ERR_INVALID for a null
 * handle or pointer, nbins outside 1..NB_MODES_MAX_BINS, mmax above NB_MODES_MAX_M, unknown flag bits, a
 * reserved field != 0, non-finite, negative or not strictly ascending edges, a non-finite centre or
 * velocity (without NB_MODES_CENTER_COM), an axis without a finite non-zero length -- all checked before
 * any device call; NB_ERR_UNSUPPORTED for a sharded simulator (placement world > 1).  n == 0 is answered
 * on the host: zero sums, the explicit centre or NaN for the centre of no mass. */
int nb_disc_modes_sim(nb_sim *sim, const nb_modes_params *params, nb_modes_head *out, nb_modes_bin *bins,
                      double *modes);
/* Host only, a pure function of its arguments: mode m (1 <= m <= mmax) of every bin of `modes` as
 * nb_disc_modes_sim filled it, out[nbins].  With C_0 = modes[k][0][NB_MODES_C]: amplitude = hypot(C, S) / C_0,
 * phase = atan2(S, C) / m, pattern_speed = (C DC + S DS) / (C C + S S) (from dC/dt = -m DS, dS/dt = m DC: the
 * rate at which the phase of the bodies now in the annulus turns; the flux through the annulus' edges is
 * not in it), bend_amplitude = hypot(ZC, ZS) / C_0, bend_phase = atan2(ZS, ZC) / m.  Every
 * field of a bin is NaN where C_0 is 0 or NaN; phase and pattern_speed are NaN where C C + S S == 0, bend_phase
 * where ZC ZC + ZS ZS == 0.  NB_ERR_INVALID for a null pointer, nbins or mmax out of range, m outside
 * 1..mmax. */
int nb_disc_modes_derive(const double *modes, uint32_t nbins, uint32_t mmax, uint32_t m, nb_modes_derived *out);

/* ------------------------------------------------------------------------- */
/* Shell modes -- spherical-harmonic sums per radial shell: triaxiality shell  */
/* by shell, core sloshing, twists and figure rotation in three dimensions     */
/* (no reference counterpart)                                                  */
/* ------------------------------------------------------------------------- */
/* Per spherical shell about a centre: sum mu Q_l^m(cos theta) sin^m theta (cos, sin)(m phi)
 * for 0 <= m <= l <= lmax, the unnormalised real spherical harmonics of the members'
 * directions, and with NB_SHELL_RATES their exact time derivatives along the members'
 * velocities.  nb_shell_modes_derive forms the orthonormal coefficients, the power per l,
 * phases, pattern speeds, the l = 1 vector and the l = 2 tensor.  The rule, which
 * DESIGN.md 6x states in full; binary64 from the binary32 state, one rounding per
 * operation, no contraction, no transcendental, in this order:
 *   input     nbins in 1..NB_SHELL_MAX_BINS and nbins + 1 edges, checked exactly as
 *             nb_disc_modes_sim checks them; lmax in 0..NB_SHELL_MAX_L, with NB_SHELL_RATES
 *             in 0..NB_SHELL_MAX_L_RATES; a centre c and a frame velocity v_c, or
 *             NB_SHELL_CENTER_COM: the fp64 `com` and `momentum / mass` of
 *             nb_sim_diagnostics bit for bit, formed on the device; an axis
 *   frame     n, e1, e2 exactly as nb_map_frame(axis) returns them: n is the polar axis,
 *             phi = 0 is e1
 *   per body  that counts (position, velocity and mass finite; the others are
 *             `nonfinite`):
 *               d = (double)x - c, u = (double)v - v_c         per component
 *               r2 = (dx dx + dy dy) + dz dz                   nb_sim_radial_profile's
 *                                                              spherical rule
 *               bin: the k with edges[k]^2 <= r2 < edges[k + 1]^2 (the squares formed
 *                    once on the host); r2 < edges[0]^2: inside; r2 >= edges[nbins]^2:
 *                    outside; a NaN r2 (a NaN centre) is below every edge
 *               r  = sqrt(r2)
 *               h  = (dx nx + dy ny) + dz nz,  a with e1 and b with e2 likewise
 *               zeta = h / r, alpha = a / r, beta = b / r      (all 0 where r2 == 0)
 *               c_0 = 1, s_0 = 0; c_m = c_(m-1) alpha - s_(m-1) beta,
 *                                 s_m = s_(m-1) alpha + c_(m-1) beta    m = 1 .. lmax
 *                                 (sin^m theta cos m phi and sin^m theta sin m phi)
 *               Q_m^m = (2m - 1)!! (1, 1, 3, 15, 105, 945, 10395), Q_(m-1)^m = 0,
 *               Q_l^m = (((2l - 1) zeta) Q_(l-1)^m - (l + m - 1) Q_(l-2)^m) / (l - m)
 *                                 for l > m: d^m P_l / d zeta^m, a polynomial, without
 *                                 the Condon-Shortley sign
 *               with mu = (double)mass the terms
 *                 C_lm = mu (Q_l^m c_m)   0 <= m <= l,   S_lm = mu (Q_l^m s_m)   m >= 1
 *               and once mu r and mu u_r, where s = (ux dx + uy dy) + uz dz and
 *               u_r = s / r (0 where r2 == 0)
 *               r2 == 0: C_00 = mu and every other term, rates included, is +0
 *   rates     with NB_SHELL_RATES, uh = (ux nx + uy ny) + uz nz, ua and ub likewise,
 *               zeta' = (uh - u_r zeta) / r, alpha' = (ua - u_r alpha) / r,
 *               beta' = (ub - u_r beta) / r
 *               c'_0 = s'_0 = 0,
 *               c'_m = (c'_(m-1) alpha + c_(m-1) alpha') - (s'_(m-1) beta + s_(m-1) beta')
 *               s'_m = (s'_(m-1) alpha + s_(m-1) alpha') + (c'_(m-1) beta + c_(m-1) beta')
 *               Q'_m^m = Q'_(m-1)^m = 0,
 *               Q'_l^m = ((2l - 1) (zeta' Q_(l-1)^m + zeta Q'_(l-1)^m)
 *                         - (l + m - 1) Q'_(l-2)^m) / (l - m)
 *               DC_lm = mu (Q'_l^m c_m + Q_l^m c'_m),  DS_lm likewise with s_m, s'_m
 *             the rate of the sum over the bodies now in the shell; the flux through the
 *             shell's edges is not in it
 *   lists, sums, mass   word for word as nb_disc_modes_sim: ascending body index, runs of
 *             64 places through the xor butterfly, chunks of NB_SHELL_CHUNK = 4,096 places
 *             added left to right from +0, the chunks added left to right from +0;
 *             mass = inside_mass + the bins' C_00 in order + outside_mass
 * With K = (lmax + 1)^2 and B = K (2 with NB_SHELL_RATES, else 1), coef[k B + i] is sum i of
 * bin k: i = l^2 for m = 0, l^2 + 2m - 1 for C_lm and l^2 + 2m for S_lm; the rates follow at
 * K + i.  Inside and outside report their count and their sum of mu only.  Two calls
 * return the same bits; a bin's bits depend on its own members, the centre and the frame
 * alone.  No float atomics.  The call is ordered after the enqueued steps on the
 * simulator's stream, ends with one synchronisation, reports a TreeSim's status words as
 * nb_sim_read_particles does, launches nothing inside a graph capture and does not change
 * the trajectory.  Spelt noun first as nb_disc_modes_sim is. */
#define NB_SHELL_MAX_BINS 256u
#define NB_SHELL_MAX_L 6u
#define NB_SHELL_MAX_L_RATES 4u /* (lmax + 1)^2 (1 + rates) + 2 fields are one lane each of a wave of 64 */
#define NB_SHELL_CHUNK 4096u
#define NB_SHELL_CENTER_COM 1u /* centre = com, frame velocity = P/M of the measured state (as NB_MODES_CENTER_COM) */
#define NB_SHELL_RATES 2u      /* also the time derivative of every sum */

typedef struct nb_shell_params {
    uint32_t nbins, lmax; /* 1..NB_SHELL_MAX_BINS, 0..NB_SHELL_MAX_L (NB_SHELL_MAX_L_RATES with NB_SHELL_RATES) */
    uint32_t flags;       /* NB_SHELL_CENTER_COM | NB_SHELL_RATES */
    uint32_t reserved;    /* 0 */
    double center[3];     /* ignored with NB_SHELL_CENTER_COM */
    double velocity[3];   /* ignored with NB_SHELL_CENTER_COM */
    double axis[3];       /* the polar axis: finite, non-zero; need not be a unit vector */
    const double *edges;  /* nbins + 1 radii: finite, >= 0, strictly ascending */
} nb_shell_params;

typedef struct nb_shell_head { /* 200 bytes */
    uint64_t step_num, n, nonfinite;
    uint64_t inside_count, outside_count;
    double inside_mass, outside_mass;
    double mass;                      /* inside + the bins in order + outside */
    double center[3], velocity[3];    /* the ones used */
    double axis[3], e1[3], e2[3];     /* nb_map_frame of the caller's axis */
    uint32_t nbins, lmax, flags, reserved;
} nb_shell_head;

typedef struct nb_shell_bin { /* 24 bytes */
    uint64_t count;
    double m_r;  /* sum mu r */
    double m_ur; /* sum mu u_r */
} nb_shell_bin;

typedef struct nb_shell_derived { /* 232 bytes: one bin; NaN above lmax */
    double power[NB_SHELL_MAX_L + 1];    /* sum over m of a_lm^2, over 2l + 1 */
    double relative[NB_SHELL_MAX_L + 1]; /* sqrt(power_l / power_0) */
    double dipole[3];                    /* the l = 1 vector, in the state's coordinates */
    double quad_values[3];               /* the l = 2 tensor's eigenvalues, descending */
    double quad_axes[9];                 /* and their unit vectors (nb_shape_eigen), in the state's coordinates */
} nb_shell_derived;

#if defined(__cplusplus)
static_assert(sizeof(nb_shell_params) == 96 && sizeof(nb_shell_head) == 200 && sizeof(nb_shell_bin) == 24 &&
                  sizeof(nb_shell_derived) == 232,
              "nb_shell_* layouts");
static_assert((NB_SHELL_MAX_L + 1) * (NB_SHELL_MAX_L + 1) + 2 <= 64 &&
                  2 * (NB_SHELL_MAX_L_RATES + 1) * (NB_SHELL_MAX_L_RATES + 1) + 2 <= 64,
              "one lane per field");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(nb_shell_params) == 96 && sizeof(nb_shell_head) == 200 && sizeof(nb_shell_bin) == 24 &&
                   sizeof(nb_shell_derived) == 232,
               "nb_shell_* layouts");
#endif

/* out: the head; bins: nbins records; coef: nbins B doubles (above).  NB_ERR_INVALID for a null handle or
 * pointer, nbins outside 1..NB_SHELL_MAX_BINS, lmax above NB_SHELL_MAX_L (above NB_SHELL_MAX_L_RATES with
 * NB_SHELL_RATES), unknown flag bits, a reserved field != 0, non-finite, negative or not strictly ascending
 * edges, a non-finite centre or velocity (without NB_SHELL_CENTER_COM), an axis without a finite non-zero
 * length -- all checked before any device call; NB_ERR_UNSUPPORTED for a sharded simulator (placement
 * world > 1).  n == 0 is answered on the host: zero sums, the explicit centre or NaN for the centre of no
 * mass. */
int nb_shell_modes_sim(nb_sim *sim, const nb_shell_params *params, nb_shell_head *out, nb_shell_bin *bins,
                       double *coef);
/* Host only, a pure function of its arguments: head (nbins, lmax, flags, axis, e1, e2 are read) and coef as
 * nb_shell_modes_sim filled them; out[nbins]; norm, phase and speed are null or nbins K doubles each, indexed
 * as coef's first block.  One rounding per operation, no contraction:
 *   a_i = N_lm coef_i with F = (2l + 1) / NB_SHELL_FOUR_PI, N_l0 = sqrt(F) and
 *         N_lm = sqrt((2 F) ((l - m)! / (l + m)!)): the coefficients of the orthonormal real harmonics
 *         (without the Condon-Shortley sign) -> norm
 *   power_l = (a_(l^2)^2 + a_(l^2+1)^2 + ... in index order) / (2l + 1): it does not depend on the axis
 *   relative_l = sqrt(power_l / power_0); NaN where power_0 is 0 or NaN
 *   phase at i = l^2 + 2m - 1: atan2(S, C) / m;  speed at the same i, with NB_SHELL_RATES:
 *         (C DS - S DC) / (m (C C + S S)), the rate at which component (l, m) of the bodies now in the shell
 *         turns about the axis; both NaN where C C + S S is 0 or NaN, and at every other index
 *   dipole_j = (a_11c e1_j + a_11s e2_j) + a_10 n_j                                      (lmax >= 1)
 *   the l = 2 tensor T with x^T T x = sum_m a_2m Y_2m(x) on the unit sphere, in the frame (e1, e2, n):
 *         q0 = N_20 a_20, q1c = N_21 a_21c, q1s, q2c = N_22 a_22c, q2s likewise;
 *         T_11 = (-0.5 q0) + 3 q2c, T_22 = (-0.5 q0) - 3 q2c, T_33 = q0, T_12 = 3 q2s, T_13 = 1.5 q1c,
 *         T_23 = 1.5 q1s; with R = (e1 e2 n) as columns W_ib = (R_i1 T_1b + R_i2 T_2b) + R_i3 T_3b and
 *         M_ij = (W_i1 R_j1 + W_i2 R_j2) + W_i3 R_j3 for i <= j; its eigenvalues and axes by
 *         nb_shape_eigen                                                                  (lmax >= 2)
 * NB_ERR_INVALID for a null head, coef or out, nbins or lmax out of range, unknown flag bits. */
#define NB_SHELL_FOUR_PI 12.566370614359172 /* the double nearest 4 pi */
int nb_shell_modes_derive(const nb_shell_head *head, const double *coef, nb_shell_derived *out, double *norm,
                          double *phase, double *speed);

/* ------------------------------------------------------------------------- */
/* Smoothed maps -- every body spread over the pixels of a 2-D grid with a    */
/* kernel of its own radius (no reference counterpart: the image of the       */
/* density estimate, where nb_sim_map gives shot noise)                       */
/* ------------------------------------------------------------------------- */
/* nb_sim_map puts a body into one cell; this pass spreads it over every pixel
 * whose centre lies within the body's own smoothing length s[i] (typically the
 * distance to its k-th neighbour, sqrt of nb_sim_knn's r2), with a compact
 * kernel of unit integral.  The rule, which DESIGN.md 6j states in full:
 * everything in binary64 from the binary32 state and the caller's binary64 s[],
 * one rounding per operation, no contraction, in this order:
 *   frame     n, e1, e2 exactly as nb_sim_map (nb_map_frame)
 *   per body  d = (double)x - c, u = (double)v - v_c; a, b, h and ua, ub, w exactly as
 *             nb_sim_map; the predicate for a counted body is nb_sim_map's; the slab
 *             tests the body's own depth: lo <= h < hi (a NaN h is outside)
 *   edges     xe[], ye[] exactly as nb_sim_map (nb_map_edges)
 *   centres   xc[i] = 0.5 (xe[i] + xe[i+1]), yc[j] = 0.5 (ye[j] + ye[j+1])  (nb_smooth_centres)
 *   length    s_eff = s < s_min ? s_min : (s > s_max ? s_max : s), 0 < s_min <= s_max finite.
 *             s = 0 (nb_sim_knn's r_k at coincident bodies) and every s below s_min,
 *             negative ones included, are `raised` to s_min; s = +inf (r_k when no more
 *             than k bodies are counted) and every s above s_max are `lowered` to s_max;
 *             both are counted over the counted bodies whose s is not NaN, whatever
 *             their depth.  A NaN s stays NaN: the body deposits nothing and is counted
 *             in `bad_smoothing`
 *   weight    of body i at pixel (ix, jy): da = xc[ix] - a, db = yc[jy] - b,
 *             r2 = da da + db db, s2 = s_eff s_eff.  The body reaches the pixel iff
 *             r2 < s2 (strictly); then t = 1 - r2 / s2 and wgt = (K / s2) (t t),
 *             K = NB_SMOOTH_K = 3 / pi: the 2-D kernel (3 / (pi s^2)) (1 - r^2 / s^2)^2 of
 *             unit integral, the exact line-of-sight projection of the 3-D kernel
 *             proportional to (1 - q^2)^(3/2).  A polynomial in r2: no sqrt
 *   terms     wm = m wgt; the planes are the sums over the reaching bodies of wm, wm ua,
 *             wm ub, wm w, (wm w) w, wm ((ux ux + uy uy) + uz uz)
 *   counts    counts[jy][ix] = the number of bodies that reach the pixel: decided by the
 *             one comparison above, so exact integers
 * Plane 0 is a surface density already (mass per area of the plane coordinates).
 * The kernel is point-sampled at the pixel centres, not integrated over the
 * pixels: the sum of wgt times the pixel area over a body's pixels is 1 only up to
 * the sampling error, which falls with s_eff in pixels (DESIGN.md 6j has the
 * figures: within -0.7 % / +1.5 % at 2 pixels), and a body whose s_eff is below
 * half a pixel diagonal can miss every centre.  s_min is that floor; an exact
 * per-body renormalisation is a second pass per body and not done.
 * stats: nonfinite + bad_smoothing + skipped + deposited == n, where `deposited`
 * are the bodies that reach at least one pixel and `skipped` the counted bodies
 * with a valid s that reach none (outside the depth slab, or no centre within
 * s_eff); pairs = the sum of counts; mass = the mass of all counted bodies (a NaN
 * s included), deposited_mass that of the deposited ones.  tile_entries is an
 * implementation figure (the (8 x 8-pixel tile, body) entries the pass sorted)
 * and not part of the rule.
 * NB_SMOOTH_CENTER_COM works as NB_MAP_CENTER_COM.  No float atomics: two calls
 * on one state return bit-identical counts, planes and stats, and every double is
 * within 1e-10 of its sum of |term| of the binary64 sum.  The call is ordered
 * after the enqueued steps on the simulator's stream, reports a TreeSim's status
 * words as nb_sim_read_particles does, and does not change the trajectory.  It
 * synchronises twice: once for the number of tile entries, which sizes its
 * workspace, and once at the end.
 * "smooth_segment_len" (nb_sim_set_tuning, 256..65536, a multiple of 256; default
 * 4096; speed and testing only): a tile's entries are summed in runs of at most
 * this many, the runs then in order. */
#define NB_SMOOTH_CENTER_COM 1u /* as NB_MAP_CENTER_COM */
#define NB_SMOOTH_VELOCITY 2u   /* add the five velocity planes */
#define NB_SMOOTH_K 0.95492965855137201461 /* K = 3 / pi, to binary64 0x1.e8ec8a4aeacc4p-1 */
#define NB_SMOOTH_MAX_ENTRIES (1ull << 28) /* (tile, body) entries of one call: 16 B each across the two sort sides */

typedef struct nb_smooth_params {
    uint32_t width, height, flags, reserved; /* sides 1..NB_MAP_MAX_SIDE, at most NB_MAP_MAX_CELLS pixels; reserved 0 */
    double center[3], velocity[3];           /* ignored with NB_SMOOTH_CENTER_COM */
    double axis[3];                          /* line of sight; any non-zero finite vector */
    double x_range[2], y_range[2];           /* window in the plane coordinates a, b: [lo, hi) */
    double depth_range[2];                   /* slab along the line of sight: lo <= h < hi; -inf, +inf = everything */
    double s_min, s_max;                     /* 0 < s_min <= s_max, both finite */
} nb_smooth_params;

typedef struct nb_smooth_stats {
    uint64_t step_num, n, nonfinite, bad_smoothing, skipped, deposited, raised, lowered, pairs;
    uint64_t tile_entries;          /* implementation figure, not part of the rule */
    double mass, deposited_mass;    /* mass: all counted bodies */
    double center[3], velocity[3];  /* the values used */
    double n_hat[3], e1[3], e2[3];  /* the frame used */
    double s_min, s_max;
    uint32_t width, height, flags, max_count;
} nb_smooth_stats;

/* The smoothed map of a simulator's current state.  s: n smoothing lengths on the host, s[i] that of body i
 * in the order of nb_sim_read_particles now (a TreeSim reorders its bodies at every step).  counts: height *
 * width values, row 0 the smallest b; planes: P planes of height * width doubles, plane-major: P = 1 without
 * NB_SMOOTH_VELOCITY, P = 6 with it, in the order of `terms` above.  counts, planes and stats may each be
 * null: what is not asked for is not copied, and a call with none of them synchronises and measures nothing.
 * NB_ERR_INVALID for a null handle or params, what nb_sim_map refuses of the fields the two share, s_min or
 * s_max not finite, s_min <= 0 or s_max < s_min, unknown flag bits or reserved != 0, a null s with n > 0 --
 * all checked before any device call.  NB_ERR_UNSUPPORTED for a sharded simulator (placement world > 1), and
 * for more than NB_SMOOTH_MAX_ENTRIES tile entries (a large s_max on a fine grid): the outputs are then
 * untouched and the simulator stays usable. */
int nb_sim_smooth_map(nb_sim *sim, const nb_smooth_params *params, const double *s, uint32_t *counts,
                      double *planes, nb_smooth_stats *stats);
/* Host only, no device: the `cells` pixel centres of a window [lo, hi) (see above).  NB_ERR_INVALID for what
 * nb_map_edges refuses. */
int nb_smooth_centres(double lo, double hi, uint32_t cells, double *out);

/* ------------------------------------------------------------------------- */
/* Renderer -- frames of the particle state, drawn off screen on the device   */
/* (the draw pass of OnlineRenderer, src/runners/online_renderer.rs:224-367,  */
/* and src/draw.wgsl; no window is opened)                                    */
/* ------------------------------------------------------------------------- */
/* The reference draws one small triangle per particle, without depth test or
 * culling, every fragment the constant (1,1,1,0.25) alpha-blended over a constant
 * clear colour (draw.wgsl:19-22, online_renderer.rs:340-352).  The blended pixel
 * then depends only on how many triangles cover it, so the frame is defined by an
 * integer coverage count per pixel and a closed-form colour.  The rule, which
 * DESIGN.md 6c states in full (binary32, one rounding per operation, in this
 * order), per body of the state nb_sim_read_particles would return:
 *   clip      c_r = ((M[r,0] x + M[r,1] y) + M[r,2] z) + M[r,3], M[r,c] = view_proj[4c + r]
 *             (draw.wgsl:17); drawn only if c_w > 0 and 0 <= c_z <= c_w (wgpu's
 *             depth clip; all three vertices share c_z and c_w), else `clipped`
 *   vertices  offsets (-s,-s), (s,-s), (0,s), s = half_size (online_renderer.rs:224,
 *             draw.wgsl:13-16): ndc = (c_xy + off) / c_w, sx = (ndc_x 0.5 + 0.5) W,
 *             sy = (0.5 - ndc_y 0.5) H; any |sx| or |sy| not below 2^22: `oversize`
 *   snap      X = rint(256 sx), Y = rint(256 sy) (ties to even): 8 sub-pixel bits
 *   coverage  pixel (i, j), centre (256 i + 128, 256 j + 128), by integer edge
 *             functions, either winding, top-left rule, zero area covers nothing,
 *             scissored to the image; counts[j W + i] = triangles covering it
 *   colour    lin = 1 - (1 - clear)(1 - alpha)^k per channel, byte =
 *             round(255 enc(lin)), enc = sRGB transfer with NB_RENDER_SRGB, A = 255
 * A body with a non-finite coordinate is `nonfinite` and not drawn.
 * drawn + clipped + oversize + nonfinite == n.  The order of the bodies does not
 * matter (a TreeSim's state is in tree order).  The call is ordered after the
 * enqueued steps on the simulator's stream, ends with one synchronisation, copies
 * only the images asked for, reports a TreeSim's status words as
 * nb_sim_read_particles does, and does not change the trajectory. */
#define NB_RENDER_SRGB 1u /* encode the bytes with the sRGB transfer function */

typedef struct nb_camera { /* `Camera`, online_renderer.rs:12-20 */
    float eye[3], target[3], up[3];
    float aspect, fovy_deg, znear, zfar;
} nb_camera;

typedef struct nb_render_params {
    uint32_t width, height; /* 1..16384 each */
    float view_proj[16];    /* column-major (CameraUniform, online_renderer.rs:22-26) */
    float half_size;        /* 0.006f (online_renderer.rs:224) */
    float clear[3];         /* 0.01, 0, 0.05 (online_renderer.rs:345-349); each in [0,1] */
    float alpha;            /* 0.25 (draw.wgsl:21); in [0,1] */
    uint32_t flags, reserved;
} nb_render_params;

typedef struct nb_render_stats {
    uint64_t step_num; /* the step the drawn state is the result of */
    uint64_t n, drawn, clipped, oversize, nonfinite;
    uint64_t fragments; /* sum of counts */
    uint32_t max_count, reserved;
} nb_render_stats;

/* The camera OnlineRenderer::new sets up (online_renderer.rs:231-239): eye (0,1,2),
 * target 0, up +y, aspect width/height, fovy 45 degrees, znear 1e-5, zfar 100. */
int nb_camera_default(nb_camera *cam, uint32_t width, uint32_t height);
/* Camera::build_view_projection_matrix (online_renderer.rs:41-54):
 * OPENGL_TO_WGPU_MATRIX * perspective * look_at_rh with cgmath's formulas, evaluated
 * in double from the float fields and rounded to float once; out is column-major.
 * NB_ERR_INVALID for a camera that has no finite matrix. */
int nb_camera_view_proj(const nb_camera *cam, float out[16]);
/* The reference's frame: default camera, half_size, clear colour and alpha, sRGB. */
int nb_render_params_default(nb_render_params *params, uint32_t width, uint32_t height);
/* Draw the simulator's current state (the render pass of OnlineRenderer::render,
 * online_renderer.rs:331-367).  rgba: width*height*4 bytes, rows top to bottom, or
 * NULL; counts: width*height, or NULL; stats: or NULL.  NB_ERR_INVALID for null
 * params, a size outside 1..16384, unknown flags, alpha or clear outside [0,1], a
 * non-finite half_size or matrix (all checked before any device call);
 * NB_ERR_UNSUPPORTED for a sharded simulator (placement world > 1).  Tuning key
 * "render_design" (nb_sim_set_tuning; speed only, identical counts): 0 automatic,
 * 1 direct (global atomics), 2 tiled (screen tiles in LDS). */
int nb_sim_render(nb_sim *sim, const nb_render_params *params, uint8_t *rgba, uint32_t *counts,
                  nb_render_stats *stats);

int nb_sim_destroy(nb_sim *sim);

/* ------------------------------------------------------------------------- */
/* Runner -- `OfflineHeadless<T>`, src/runners/offline_headless.rs:4-45       */
/* ------------------------------------------------------------------------- */
typedef struct nb_runner nb_runner;

/* `OfflineHeadless::<T>::new(sim_params, add_params, init_fn)`,
 * offline_headless.rs:17-35: acquires the device (here: device_id, or -1 for
 * "highest-performance adapter" = device 0) and constructs the simulator T
 * selected by add_params.kind. */
int nb_runner_create(nb_runner **out, const nb_sim_params *sim_params,
                     const nb_add_params *add_params, nb_init_fn init, void *user, int device_id);

/* The same constructor over SEVERAL GPUs of this process (no reference counterpart: the reference
 * owns one adapter, offline_headless.rs:22-31; this is SURVEY 8(b)'s `device_ids, n_devices` form).
 * All-pairs: rank r owns the contiguous body range [r per, (r+1) per), per =
 * nb_shard_bodies_per_rank(N, n_devices), on device_ids[r]; every device keeps both position/mass
 * buffers in full, and the kernel that finishes a rank's step stores the rank's new
 * float4{x,y,z,m} slice into every peer's next-step buffer through peer access (one slice per
 * xGMI link), ordered by one HIP event per rank and step -- no host copy, no collective library.
 * Barnes-Hut: replicated tree, partitioned walk -- every device holds the full
 * state and builds the identical octree, walks its range of the sorted bodies, and copies its new
 * position / velocity / acceleration slices into every peer's arrays (one kernel on its stream, stores through peer access,
 * two events per rank and step); bit for bit the single TreeSim.  (Morton domains + LET exchange,
 * which also shards the build: nb_runner_create_multi_let below, or one process per GPU through
 * nb_placement and NB_PHASE_LET_*.)
 * One host thread per rank inside the library; the caller stays single-threaded and every call
 * below is synchronous as on one device.  A device id may repeat (ranks sharing a GPU).  n_devices
 * == 1 is nb_runner_create. */
int nb_runner_create_multi(nb_runner **out, const nb_sim_params *sim_params,
                           const nb_add_params *add_params, nb_init_fn init, void *user,
                           const int *device_ids, int n_devices);

/* Barnes-Hut over several GPUs of this process with the BUILD sharded too: the
 * bodies are cut into n_devices Morton-range domains at start-up; per step every rank builds the
 * octree of its own bodies inside the global root cube, exports to every peer the part of that tree
 * the peer's bodies can need (its locally essential tree, pruned decision-exactly) and walks its own
 * tree plus the imported ones -- the protocol of NB_PHASE_LET_* below, hosted inside the library: the
 * bounds, the export counts and the exported records are stored straight into the peers' tables and
 * import areas through peer access (the counts are consumed on the device), ordered by three events
 * per rank and step; no host read between migrations.  migrate_every = k > 0: every k-th step the
 * bodies that left their rank's key range are handed to their new owner (one host read of the
 * leaver counts on those steps); 0: never.  What a body feels is the sum of per-domain Barnes-Hut
 * walks, each with the reference's per-body acceptance test (tree.wgsl:57-70): within the walk's
 * own error of the one-tree result, not bit-equal to it.  nb_runner_read_particles returns the
 * bodies rank by rank, each rank's in its current tree order.  add_params must be TreeSimParams. */
int nb_runner_create_multi_let(nb_runner **out, const nb_sim_params *sim_params,
                               const nb_add_params *add_params, nb_init_fn init, void *user,
                               const int *device_ids, int n_devices, int migrate_every);

/* `OfflineHeadless::step(&mut self)`, offline_headless.rs:38-44:
 * encode -> submit -> cleanup -> blocking wait. */
int nb_runner_step(nb_runner *runner);

/* n steps enqueued back to back, one wait at the end (benchmark use). */
int nb_runner_step_n(nb_runner *runner, int n);

/* Measurement (no reference counterpart).  With profiling on, every rank of a several-GPU runner records
 * timing events on its stream at the borders between its own kernels and its waits for the peers' events;
 * after nb_runner_step_n, nb_runner_rank_times gives, per rank, the milliseconds of that batch of steps spent in
 * the rank's kernels (kernel_ms[r]) and waiting on the device for peers (wait_ms[r]).  n = the ranks the
 * arrays hold.  A one-device runner reports the batch's time on its stream in kernel_ms[0].  Off by default:
 * no event is recorded. */
int nb_runner_set_profiling(nb_runner *runner, int on);
int nb_runner_rank_times(nb_runner *runner, float *kernel_ms, float *wait_ms, int n);

int nb_runner_read_particles(nb_runner *runner, nb_particle *dst, size_t n);
int nb_runner_sim_params(const nb_runner *runner, nb_sim_params *out);
int nb_runner_step_num(const nb_runner *runner, uint64_t *out);
/* nb_sim_diagnostics of the runner's simulator (no reference counterpart).
 * NB_ERR_UNSUPPORTED for a several-GPU runner (nb_runner_create_multi*). */
int nb_runner_diagnostics(nb_runner *runner, uint32_t flags, nb_diagnostics *out);
/* nb_sim_radial_profile of the runner's simulator (no reference counterpart).
 * NB_ERR_UNSUPPORTED for a several-GPU runner (nb_runner_create_multi*). */
int nb_runner_radial_profile(nb_runner *runner, const nb_radial_params *params, nb_radial_profile *out,
                             nb_radial_bin *bins);
/* nb_sim_field of the runner's simulator (no reference counterpart).
 * NB_ERR_UNSUPPORTED for a several-GPU runner (nb_runner_create_multi*). */
int nb_runner_field(nb_runner *runner, const float *points, size_t m, uint32_t flags, nb_field_sample *out,
                    nb_field_stats *stats);
/* nb_sim_map of the runner's simulator (no reference counterpart).
 * NB_ERR_UNSUPPORTED for a several-GPU runner (nb_runner_create_multi*). */
int nb_runner_map(nb_runner *runner, const nb_map_params *params, uint32_t *counts, double *planes,
                  nb_map_stats *stats);
/* nb_sim_fof of the runner's simulator (no reference counterpart).
 * NB_ERR_UNSUPPORTED for a several-GPU runner (nb_runner_create_multi*). */
int nb_runner_fof(nb_runner *runner, const nb_fof_params *params, uint32_t *labels, uint32_t *group_of,
                  nb_fof_group *groups, size_t group_capacity, nb_fof_stats *stats);
/* nb_sim_bound of the runner's simulator (no reference counterpart).
 * NB_ERR_UNSUPPORTED for a several-GPU runner (nb_runner_create_multi*). */
int nb_runner_bound(nb_runner *runner, const nb_bound_params *params, uint32_t *group_of, uint32_t *bound_of,
                    double *energy, nb_bound_group *groups, size_t group_capacity, nb_bound_stats *stats);
/* nb_sim_hop of the runner's simulator (no reference counterpart).
 * NB_ERR_UNSUPPORTED for a several-GPU runner. */
int nb_runner_hop(nb_runner *runner, const nb_hop_params *params, uint32_t *labels, uint32_t *group_of,
                  double *density, nb_fof_group *groups, double *peak_density, size_t group_capacity,
                  nb_hop_boundary *boundaries, size_t boundary_capacity, nb_hop_stats *stats);

/* nb_sim_knn of the runner's simulator (no reference counterpart).
 * NB_ERR_UNSUPPORTED for a several-GPU runner (nb_runner_create_multi*). */
int nb_runner_knn(nb_runner *runner, const nb_knn_params *params, double *r2, uint32_t *kth, double *mass_in,
                  double *density, nb_knn_stats *stats);
/* nb_sim_halo_profiles of the runner's simulator: the same refusals, and NB_ERR_UNSUPPORTED for a several-GPU
 * runner. */
int nb_runner_halo_profiles(nb_runner *runner, const nb_halo_params *params, nb_halo_head *heads,
                            nb_radial_bin *bins, nb_halo_stats *stats);
/* nb_sim_group_shapes of the runner's simulator: the same refusals, and NB_ERR_UNSUPPORTED for a several-GPU
 * runner. */
int nb_runner_group_shapes(nb_runner *runner, const nb_shape_params *params, const uint32_t *group_of, size_t m,
                           const double *centers, const double *velocities, const double *radius,
                           nb_shape_group *rows_out, uint32_t *selected_of, nb_shape_stats *stats);
/* nb_group_radii_sim of the runner's simulator: the same refusals, and NB_ERR_UNSUPPORTED for a several-GPU
 * runner. */
int nb_group_radii_runner(nb_runner *runner, const nb_radii_params *params, const uint32_t *group_of, size_t m,
                          const double *centers, nb_radii_group *rows_out, uint32_t *rank_of, double *enclosed_of,
                          nb_radii_stats *stats);
/* nb_disc_modes_sim of the runner's simulator: the same refusals, and NB_ERR_UNSUPPORTED for a several-GPU
 * runner. */
int nb_disc_modes_runner(nb_runner *runner, const nb_modes_params *params, nb_modes_head *out, nb_modes_bin *bins,
                         double *modes);
/* nb_shell_modes_sim of the runner's simulator: the same refusals, and NB_ERR_UNSUPPORTED for a several-GPU
 * runner. */
int nb_shell_modes_runner(nb_runner *runner, const nb_shell_params *params, nb_shell_head *out, nb_shell_bin *bins,
                          double *coef);
/* nb_phase_map_sim of the runner's simulator: the same refusals, and NB_ERR_UNSUPPORTED for a several-GPU
 * runner. */
int nb_phase_map_runner(nb_runner *runner, const nb_phase_params *params, uint32_t *counts, double *planes,
                        nb_phase_stats *stats);
/* nb_tidal_sim of the runner's simulator: the same refusals, and NB_ERR_UNSUPPORTED for a several-GPU
 * runner. */
int nb_tidal_runner(nb_runner *runner, const float *points, size_t m, nb_tidal_sample *out, nb_tidal_stats *stats);
/* nb_orbits_sim of the runner's simulator: the same refusals, and NB_ERR_UNSUPPORTED for a several-GPU
 * runner. */
int nb_orbits_runner(nb_runner *runner, const nb_orbit_params *params, const double *pos, const double *vel,
                     size_t m, nb_orbit_sample *tracks, uint32_t *coincident, nb_orbit_stats *stats);
/* nb_orbit_sections_sim of the runner's simulator: the same refusals, and NB_ERR_UNSUPPORTED for a several-GPU
 * runner. */
int nb_orbit_sections_runner(nb_runner *runner, const nb_orbit_params *params, const nb_orbit_section_params *section,
                             const double *pos, const double *vel, size_t m, nb_orbit_sample *tracks,
                             uint32_t *coincident, nb_orbit_crossing *crossings, uint32_t *counts,
                             nb_orbit_summary *summaries, nb_orbit_section_stats *stats);
/* nb_orbit_stability_sim of the runner's simulator: the same refusals, and NB_ERR_UNSUPPORTED for a several-GPU
 * runner. */
int nb_orbit_stability_runner(nb_runner *runner, const nb_orbit_params *params,
                              const nb_orbit_stability_params *stability, const double *pos, const double *vel,
                              size_t m, const nb_orbit_deviation *dev0, nb_orbit_sample *tracks, uint32_t *coincident,
                              nb_orbit_deviation *devs, nb_orbit_growth *growth, nb_orbit_stability_stats *stats);
/* nb_local_kinematics_sim of the runner's simulator: the same refusals, and NB_ERR_UNSUPPORTED for a
 * several-GPU runner. */
int nb_local_kinematics_runner(nb_runner *runner, const nb_kin_params *params, double *moments, double *grads,
                               double *r2, uint32_t *kth, double *mass_in, double *density, nb_kin_stats *stats);
/* nb_fof6_sim of the runner's simulator: the same refusals, and NB_ERR_UNSUPPORTED for a several-GPU
 * runner. */
int nb_fof6_runner(nb_runner *runner, const nb_fof6_params *params, uint32_t *labels, uint32_t *group_of,
                   nb_fof_group *groups, size_t group_capacity, nb_fof_stats *stats);
/* nb_mst_sim of the runner's simulator: the same refusals, and NB_ERR_UNSUPPORTED for a several-GPU
 * runner. */
int nb_mst_runner(nb_runner *runner, const nb_mst_params *params, uint32_t *edge_lo, uint32_t *edge_hi, double *d2,
                  uint32_t *degree, nb_mst_stats *stats);
/* nb_sim_smooth_map of the runner's simulator (no reference counterpart).
 * NB_ERR_UNSUPPORTED for a several-GPU runner (nb_runner_create_multi*). */
int nb_runner_smooth_map(nb_runner *runner, const nb_smooth_params *params, const double *s, uint32_t *counts,
                         double *planes, nb_smooth_stats *stats);
/* nb_sim_render of the runner's simulator (OnlineRenderer::render, online_renderer.rs:331-367).
 * NB_ERR_UNSUPPORTED for a several-GPU runner (nb_runner_create_multi*). */
int nb_runner_render(nb_runner *runner, const nb_render_params *params, uint8_t *rgba, uint32_t *counts,
                     nb_render_stats *stats);
/* Borrow the runner's simulator (owned by the runner); NULL for a several-GPU runner. */
nb_sim *nb_runner_sim(nb_runner *runner);
int nb_runner_destroy(nb_runner *runner);

#ifdef __cplusplus
}
#endif
#endif /* NBODY_H_ */
