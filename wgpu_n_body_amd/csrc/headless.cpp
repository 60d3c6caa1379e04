// headless.cpp -- C++ counterpart of the reference's src/bin/headless.rs:14-35 (and of the
// criterion groups in benches/benchmark.rs:12-49) over the drop-in API of simulator.hpp.
//
//   headless [--sim naive|tree] [--n N] [--steps S] [--theta T] [--init uniform|disc|spherical]
//            [--seed K] [--device D | --devices D0,D1,...] [--g G] [--dt DT] [--dump FILE]
//            [--e E] [--diag K [--diag-potential 1]] [--frames DIR [--frame-every K] [--frame-size WxH]]
//            [--radial K --radial-range RMIN,RMAX [--radial-bins B] [--radial-log 0|1] [--radial-axis X,Y,Z]
//             [--radial-center com|X,Y,Z]]
//            [--rotcurve K --rotcurve-range RMIN,RMAX [--rotcurve-bins B] [--rotcurve-phi Q]
//             [--rotcurve-axis X,Y,Z] [--rotcurve-center X,Y,Z]]
//            [--freq K --freq-range RMIN,RMAX [--freq-bins B] [--freq-phi Q] [--freq-axis X,Y,Z]
//             [--freq-center X,Y,Z]]
//            [--orbits DIR [--orbits-at K] --orbits-range RMIN,RMAX [--orbits-bins B] --orbits-dt DT --orbits-steps S
//             [--orbits-every E] [--orbits-omega W] [--orbits-speed F] [--orbits-axis X,Y,Z] [--orbits-center X,Y,Z]]
//            [--sections DIR [--sections-at K] --sections-range RMIN,RMAX [--sections-bins B] --sections-dt DT
//             --sections-steps S [--sections-omega W] [--sections-speed F] [--sections-axis X,Y,Z]
//             [--sections-center X,Y,Z] [--sections-normal A,B,L] [--sections-offset D] [--sections-direction -1|0|1]
//             [--sections-max K]]
//            [--stability DIR [--stability-at K] --stability-range RMIN,RMAX [--stability-bins B] --stability-dt DT
//             --stability-steps S [--stability-omega W] [--stability-speed F] [--stability-axis X,Y,Z]
//             [--stability-center X,Y,Z]]
//            [--maps DIR [--map-every K] --map-size WxH --map-extent X0,X1,Y0,Y1 [--map-axis X,Y,Z]
//             [--map-center com|X,Y,Z] [--map-depth LO,HI]]
//            [--smaps DIR [--smap-every K] --smap-size WxH --smap-extent X0,X1,Y0,Y1 [--smap-axis X,Y,Z]
//             [--smap-center com|X,Y,Z] [--smap-depth LO,HI] [--smap-k 32] [--smap-max PIXELS]]
//            [--fof K --fof-link B [--fof-min M] [--fof-top T]]
//            [--fof6 K --fof6-link B --fof6-vlink V [--fof6-min M] [--fof6-top T]]
//            [--bound K --bound-link B [--bound-min M] [--bound-iter I] [--bound-max-group G] [--bound-top T]]
//            [--shapes K --shapes-link B [--shapes-min M] [--shapes-radius KRMS] [--shapes-reduced 0|1]
//             [--shapes-iter I] [--shapes-top T]]
//            [--lagr K [--lagr-fractions F1,F2,...] [--lagr-center com|X,Y,Z]]
//            [--radii K --radii-link B [--radii-min M] [--radii-top T]]
//            [--phase DIR [--phase-every K] --phase-x NAME,LO,HI,CELLS[,log] --phase-y NAME,LO,HI,CELLS[,log]
//             [--phase-weight NAME] [--phase-axis X,Y,Z] [--phase-center com|X,Y,Z]]
//            [--modes K --modes-range RMIN,RMAX [--modes-bins B] [--modes-m M] [--modes-log 0|1]
//             [--modes-axis X,Y,Z] [--modes-center com|X,Y,Z]]
//            [--shells K --shells-range RMIN,RMAX [--shells-bins B] [--shells-l L] [--shells-log 0|1]
//             [--shells-rates 0|1] [--shells-axis X,Y,Z] [--shells-center com|X,Y,Z]]
//            [--knn K [--knn-k 6]]
//            [--mst K [--mst-links L1,L2,...] [--mst-min M] [--mst-dump DIR]]
//            [--kin K [--kin-k 32] [--kin-gradient 0|1]]
//            [--hop K [--hop-k 64,16,4] [--hop-min M] [--hop-density-min D] [--hop-saddle S --hop-peak P] [--hop-top T]]
//            [--halo K --halo-link B --halo-range RMIN,RMAX [--halo-bins 32] [--halo-min M] [--halo-top T]
//             [--halo-rho RHO]]
//
// --devices: the step sharded over several GPUs of this process (nb_runner_create_multi; both simulators);
// --let K (with --sim tree --devices): Morton domains + LET exchange, migration every K-th step (0: never);
// a device id may repeat.
//
// --diag K prints the diagnostics (nb_runner_diagnostics) of step 0 and of every K-th step, one line
// "Diagnostics: step S kinetic K potential U total E momentum px py pz angular_momentum lx ly lz"
// (%.9e; potential and total are nan unless --diag-potential 1 adds the O(N^2) pair potential).  The
// time they take is not part of any "Step Duration"; without --diag the output is unchanged.
//
// --radial K prints the radial profile (nb_runner_radial_profile) of step 0 and of every K-th step: B
// bins (--radial-bins, default 64) between RMIN and RMAX, logarithmic unless --radial-log 0, about the
// centre of mass unless --radial-center gives a point (at rest); --radial-axis bins by distance from
// that axis through the centre (a disc's annuli) instead of from the centre.  One header line
// "Radial: step S n N nonfinite B nbins NB flags F inside_count IC inside_mass IM outside_count OC
// outside_mass OM mass M center x y z velocity x y z axis x y z shape xx yy zz xy xz yz" and one line
// per bin "RadialBin: step S bin k lo E0 hi E1 count C mass M m_r . m_ur . m_ur2 . m_uphi . m_uphi2 .
// m_u2 . ang x y z" (the fields of nb_radial_profile and nb_radial_bin; every real %.17g).  The time they
// take is not part of any "Step Duration"; without --radial the output is unchanged.
//
// --rotcurve K prints the rotation curve from the force (nb_runner_field on rings, nb_field_ring_means)
// of step 0 and of every K-th step: B radii (--rotcurve-bins, default 32) linear from RMIN to RMAX, Q
// points per ring (--rotcurve-phi, default 16) about --rotcurve-axis (default 0,1,0) through
// --rotcurve-center (default 0,0,0).  One line per ring "rotcurve <step> <R> <a_R> <a_n> <v_c>" (%.9e).
// The time they take is not part of any "Step Duration"; without --rotcurve the output is unchanged.
// --freq K prints the disc's frequencies from the force and its gradient (nb_runner_field and nb_tidal_runner on
// the same rings, nb_field_ring_means, nb_tidal_ring_means) of step 0 and of every K-th step; --freq-range,
// --freq-bins, --freq-phi, --freq-axis and --freq-center as --rotcurve's.  One line per ring
// "freq <step> <R> <Omega> <kappa> <nu> <v_c>" (%.9e; nan where the square of a frequency is negative).
// --orbits DIR integrates test particles in the frozen field (nb_orbits_runner) of the state after step K
// (--orbits-at, default 0: the initial state): one tracer per ring of B radii (--orbits-bins, default 32) linear from
// RMIN to RMAX about --orbits-axis (default 0,1,0) through --orbits-center (default 0,0,0), started on the ring's first
// point with F (--orbits-speed, default 1) times the circular velocity of --rotcurve's construction, through S steps of
// DT, the pattern turning at W (--orbits-omega, default 0), a record every E steps (--orbits-every, default 1) with
// the potential and the Jacobi integral.  Written as DIR/orbits_<step, 6 digits>.npy: NumPy format 1.0, <f8, shape
// (R, B, 8) -- position, velocity, potential, energy -- and one line "orbits <step> <records> <tracers>
// <nonfinite_tracers> <pair_launches>".  The time it takes is not part of any "Step Duration".
// --sections DIR takes a surface of section (nb_orbit_sections_runner) of the state after step K (--sections-at,
// default 0), the tracers launched as --orbits launches them (--sections-range, -bins, -speed, -axis, -center, -dt,
// -steps, -omega): the crossings of the plane A a' + B b' + L l = D of the pattern frame (--sections-normal, default
// 0,1,0; --sections-offset, default 0) upwards, downwards or both (--sections-direction 1, -1 or 0, default 1), the
// first K of each tracer (--sections-max, default 256).  Written as DIR/sections_<step, 6 digits>.npy: <f8, shape
// (B, K, 8) -- xi, eta, time and the step as a double, zero where no crossing is stored -- and
// DIR/sections_<step>_counts.npy: <f8, shape (B,), all crossings of each tracer; and one line "sections <step>
// <tracers> <crossings> <stored> <overflowed> <pair_launches>".  The time it takes is not part of any "Step Duration".
// --stability DIR measures the stability (nb_orbit_stability_runner) of the orbits of the state after step K
// (--stability-at, default 0), the tracers launched as --orbits launches them (--stability-range, -bins, -speed, -axis,
// -center, -dt, -steps, -omega), each with two deviation vectors: the unit dx along its radius in the plane of its
// ring, and the unit dx along the axis.  Written as DIR/stability_<step, 6 digits>.npy: <f8, shape (B, 6) -- the
// finite-time Lyapunov exponents of the two vectors, SALI and GALI_2 at the last state, and the peak log2 of the first
// vector with the step it was reached at -- and one line "stability <step> <tracers> <renorms> <pair_launches>".
//
// --maps DIR writes the projected map (nb_runner_map) of step 0 and of every K-th step (--map-every,
// default 1) as DIR/map_<step, 6 digits>.npy: NumPy format 1.0, <f8, shape (7, H, W) -- the counts as
// doubles, then the planes mass, m_ua, m_ub, m_w, m_w2, m_u2 -- of the window [X0, X1) x [Y0, Y1) seen
// along --map-axis (default 0,1,0) about the centre of mass unless --map-center gives a point (at rest),
// row 0 the smallest b; --map-depth keeps LO <= h < HI along the line of sight.  One line per map
// "map <step> <binned> <outside> <nonfinite> <max_count>".  DIR must exist.  The time they take is not
// part of any "Step Duration"; without --maps the output is unchanged.
//
// --smaps DIR writes the smoothed map (nb_runner_knn, then nb_runner_smooth_map with the distance to the k-th
// neighbour, k = --smap-k, as every body's smoothing length) of step 0 and of every K-th step (--smap-every,
// default 1) as DIR/smap_<step, 6 digits>.npy: the layout of --maps, shape (7, H, W) -- the counts (the bodies
// that reach a pixel) as doubles, then the planes wm, wm_ua, wm_ub, wm_w, wm_w2, wm_u2; plane 1 is the surface
// density.  The lengths are held between 2 and --smap-max (default 64) times the larger side of a pixel; the
// window, axis, centre and depth options read as those of --maps.  One line per map "smap <step> <deposited>
// <skipped> <bad_smoothing> <nonfinite> <pairs> <max_count> <tile_entries>".  DIR must exist.  The time they
// take is not part of any "Step Duration"; without --smaps the output is unchanged.
//
// --fof K finds the friends-of-friends groups (nb_runner_fof) of step 0 and of every K-th step: bodies within
// --fof-link B of each other are friends, the catalogue holds the groups of at least M bodies (--fof-min,
// default 20).  One line "fof <step> <groups> <grouped_bodies> <largest_count>", then the T largest rows
// (--fof-top, default 0) as "fof_group <step> <row> <label> <count> <mass> <x> <y> <z>" (%.9e: the mass and the
// centre of mass).  The time they take is not part of any "Step Duration"; without --fof the output is
// unchanged.
//
// --bound K unbinds the friends-of-friends groups (nb_runner_bound) of step 0 and of every K-th step: the groups of
// --bound-link B and at least M bodies (--bound-min, default 20; also the fewest a bound set may keep), at most I
// rounds (--bound-iter, default 32), groups of more than G bodies skipped (--bound-max-group, default 262144; 0:
// none).  One line "bound <step> <groups> <bound_groups> <bound_bodies> <dissolved> <unconverged> <skipped>
// <rounds_max> <pairs>", then the T rows of the largest bound mass (--bound-top, default 0) as "bound_group <step>
// <row> <label> <count> <bound_count> <iterations> <status> <mass> <x> <y> <z> <kinetic> <potential>" (%.9e: the
// bound mass, its centre of mass and its energies).  The time they take is not part of any "Step Duration";
// without --bound the output is unchanged.
//
// --shapes K finds the friends-of-friends groups (as --fof, with --shapes-link and --shapes-min, default 20) of step 0
// and of every K-th step and measures the shape of all of them in one call (nb_runner_group_shapes) about their centres
// of mass in their own frames: inside KRMS times every group's rms radius (--shapes-radius; default 0: no cut, one
// round), the tensor weighted by 1 / rho^2 with --shapes-reduced 1, at most I rounds (--shapes-iter, default 32).  One
// line "shapes <step> <groups> <converged> <unconverged> <degenerate> <empty> <rounds_max>", then the T largest groups
// (--shapes-top, default 0) as "shape_group <step> <row> <count> <selected> <q> <s> <T> <|J|> <status>" (every real
// %.17g; T the triaxiality).  The time it takes is not part of any "Step Duration"; without --shapes the output is
// unchanged.
//
// --lagr K prints the exact Lagrangian radii (nb_group_radii_runner, the whole state as one row) of step 0 and of every
// K-th step: the radii of the bodies at which the enclosed mass reaches F1, F2, ... of the total (--lagr-fractions,
// default 0.01,0.05,0.1,0.25,0.5,0.75,0.9; 1 to 16 ascending values in (0, 1]) about the centre of mass, formed on the
// device, unless --lagr-center gives a point.  One line "lagr <step> <count> <mass> <x> <y> <z> <r_vmax> <vc2_max>",
// then one line per fraction "lagr_radius <step> <fraction> <radius> <body>" (every real %.17g).  The time it takes
// is not part of any "Step Duration"; without --lagr the output is unchanged.
//
// --radii K finds the friends-of-friends groups (as --fof, with --radii-link and --radii-min, default 20) of step 0 and
// of every K-th step and measures the 10 / 50 / 90 % mass radii and the peak of M / r of all of them in one call
// (nb_group_radii_runner) about their centres of mass.  One line "radii <step> <groups> <members> <empty>", then the T
// largest groups (--radii-top, default 0) as "radii_group <step> <row> <count> <mass> <r10> <r50> <r90> <r_vmax>
// <vc2_max>" (every real %.17g).  The time it takes is not part of any "Step Duration"; without --radii the output
// is unchanged.
//
// --phase DIR writes the phase map (nb_phase_map_runner) of step 0 and of every K-th step (--phase-every, default 1)
// as DIR/phase_<step, 6 digits>.npy: the layout of --maps, shape (1 + P, H, W) -- the counts as doubles, then the
// mass and, with --phase-weight NAME, the sums of mass times that quantity and its square.  --phase-x and --phase-y
// name the quantity of the columns and of the rows (include/nbody.h "Phase maps": a, b, h, R, r, ua, ub, w, u_R,
// u_phi, u_r, u_t, speed, j_z, j, e_kin, mass) with CELLS cells between LO and HI, of constant ratio with ",log",
// in the frame of --phase-axis (default 0,1,0) about the centre of mass unless --phase-center gives a point (at
// rest).  One line per map "phase <step> <binned> <outside> <undefined> <nonfinite> <max_count>".  DIR must exist.
// The time they take is not part of any "Step Duration"; without --phase the output is unchanged.
//
// --modes K measures the azimuthal Fourier sums (nb_disc_modes_runner) of step 0 and of every K-th step in B annuli
// (--modes-bins, default 32; --modes-log 1: of constant ratio) between RMIN and RMAX about --modes-axis (default
// 0,1,0) through the centre of mass, unless --modes-center gives a point, up to mode M (--modes-m, default 4, at
// least 2).  One line "modes <step> <A2> <radius> <phase> <pattern_speed> <tilt>" (every real %.17g): the largest
// A_2 / A_0 over the annuli with mass, that annulus' mass-weighted mean radius, the phase and the single-snapshot
// pattern speed of its m = 2 mode, and the largest warp tilt of any annulus (NaN where there is none).  The time it
// takes is not part of any "Step Duration"; without --modes the output is unchanged.
//
// --shells K measures the spherical-harmonic sums (nb_shell_modes_runner) of step 0 and of every K-th step in B shells
// (--shells-bins, default 32; --shells-log, default 1: of constant ratio) between RMIN and RMAX about the centre of
// mass, unless --shells-center gives a point, with the polar axis --shells-axis (default 0,1,0), up to degree L
// (--shells-l, default 4, at least 2); --shells-rates 1 (L at most 4) sums the time derivatives too.  One line
// "shells <step> <Q2> <radius> <phase> <pattern_speed> <D1>" (every real %.17g): the largest sqrt(power_2 / power_0)
// over the shells with mass, that shell's mass-weighted mean radius, the phase and (with rates, else NaN) the pattern
// speed of its (2, 2) component, and the largest sqrt(power_1 / power_0) of any shell (NaN where there is none).  The
// time it takes is not part of any "Step Duration"; without --shells the output is unchanged.
//
// --knn K finds the k-th nearest neighbour of every body (nb_runner_knn, k = --knn-k, default 6) of step 0 and of
// every K-th step and prints one line "knn <step> <counted> <degenerate> <x> <y> <z> <vx> <vy> <vz>
// <peak_density> <peak_index>" (every real %.17g): the density centre and its velocity, the largest density and
// the body that holds it.  The time it takes is not part of any "Step Duration"; without --knn the output is
// unchanged.
//
// --mst K finds the minimum spanning tree (nb_mst_runner) of step 0 and of every K-th step and prints one line
// "mst <step> <edges> <rounds> <total length> <longest edge> <groups at L1> <groups at L2> ..." (every real %.17g): the
// groups are the components of at least M bodies (--mst-min, default 1) the tree has at each link of --mst-links, what
// nb_runner_fof finds at that link.  --mst-dump DIR writes the tree as DIR/mst_<step>.npy: NumPy format 1.0, <f8, shape
// (edges, 3) -- lo, hi and d2 per edge, in ascending order.  The time it takes is not part of any "Step Duration";
// without --mst the output is unchanged.
//
// --kin K measures how the k nearest neighbours of every body move (nb_local_kinematics_runner, k = --kin-k, default
// 32; --kin-gradient 1 adds the velocity gradient) at step 0 and at every K-th step and prints one line "kin <step>
// <counted> <degenerate> <singular> <mean_sigma> <max_Q> <max_Q_index>" (every real %.17g): the bodies whose gradient
// is singular (0 without --kin-gradient), the mean of sigma weighted by the bodies' own masses over the bodies with a
// finite sigma, the largest finite Q = rho / sigma^3 and the first body that holds it (nan and 4294967295 when there
// is none), all formed on the host in body order.  The time it takes is not part of any "Step Duration"; without
// --kin the output is unchanged.
//
// --hop K finds the density-peak groups (nb_runner_hop; --hop-k DENS,HOP,MERGE, default 64,16,4; --hop-min M, default
// 1; --hop-density-min D, default none) of step 0 and of every K-th step.  One line "hop <step> <peaks> <groups>
// <grouped_bodies> <largest_count> <boundaries> <boundary_pairs>", then the T largest rows (--hop-top, default 0) as
// "hop_group <step> <row> <label> <count> <mass> <x> <y> <z> <peak_density>" (%.9e).  With --hop-saddle S --hop-peak P
// the groups are then merged (nb_hop_regroup): "hop_merged <step> <groups> <grouped_bodies> <largest_count>" and the T
// largest merged rows as "hop_merged_group ..." in the columns of hop_group.  The time they take is not part of any
// "Step Duration"; without --hop the output is unchanged.
// --halo K finds the friends-of-friends groups (as --fof, with --halo-link and --halo-min) of step 0 and of every
// K-th step and profiles all of them about their centres of mass in their own frames in one call
// (nb_runner_halo_profiles): --halo-bins log bins (default 32) from RMIN to RMAX.  One line "halo <step> <groups>
// <tested> <items>" (<groups>: those with a finite centre of mass, which are profiled), then the T largest groups (--halo-top, default 0) as "halo_group <step> <row> <label> <count>
// <R> <M> <r_peak> <peak>" (every real %.17g): R and M where the mean enclosed density falls through RHO
// (nb_halo_overdensity; nan without --halo-rho or without a crossing), and the largest M(< r) / r over the edges
// with the edge that holds it -- the square of the circular-velocity peak over G.  The time it takes is not part of
// any "Step Duration"; without --halo the output is unchanged.
//
// --frames DIR draws the state on the device (nb_runner_render: the reference's draw pass with its
// default camera, src/runners/online_renderer.rs:224-367) at step 0 and after every K-th step
// (--frame-every, default 1) and writes DIR/frame_<step, 6 digits>.ppm (binary P6, --frame-size,
// default 1280x720), with one line "Frame S: drawn D clipped C oversize O nonfinite B fragments F
// max_count M" each.  DIR must exist.  Frame time is not part of any "Step Duration"; without
// --frames the output is unchanged.  bin/visualize.rs's run: --sim tree --n 100000 --init disc
// --g 1e-5 --e 1e-4 --dt 0.0016 --theta 0.75 --frames DIR.
//
// --dump FILE writes the final state as a snapshot (the layout of
// wgpu_n_body_amd/snapshot.py: "NBSNAP01", u64 step, SimParams, Particle[n]).
//
// Defaults reproduce headless.rs: TreeSim, 4,000,000 bodies, theta 0.75, uniform_init,
// 10 steps, printing "Step Duration: {} us" per step.  (TreeSim needs the Barnes-Hut build;
// pass --sim naive --n 65536 for the all-pairs path.)
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "simulator.hpp"

static bool write_snapshot(const std::string &path, const nbody::SimParams &sp,
                           const std::vector<nbody::Particle> &parts, uint64_t step) {
    std::FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    bool ok = std::fwrite("NBSNAP01", 1, 8, f) == 8 && std::fwrite(&step, sizeof step, 1, f) == 1 &&
              std::fwrite(&sp, sizeof sp, 1, f) == 1 &&
              std::fwrite(parts.data(), sizeof(nbody::Particle), parts.size(), f) == parts.size();
    return std::fclose(f) == 0 && ok;
}

template <class Sim>
static void print_diag(nbody::OfflineHeadless<Sim> &runner, bool potential) {
    const nbody::Diagnostics d = runner.diagnostics(potential);
    std::printf("Diagnostics: step %llu kinetic %.9e potential %.9e total %.9e momentum %.9e %.9e %.9e "
                "angular_momentum %.9e %.9e %.9e\n",
                (unsigned long long)d.step_num, d.kinetic, d.potential, d.total, d.momentum[0], d.momentum[1],
                d.momentum[2], d.angular_momentum[0], d.angular_momentum[1], d.angular_momentum[2]);
}

struct RadialOptions {
    int every = 0;
    uint32_t bins = 64;
    bool log = true, have_range = false;
    double rmin = 0.0, rmax = 0.0;
    nbody::RadialParams params{0, NB_RADIAL_CENTER_COM};  // flags, centre, axis
};

template <class Sim>
static void print_radial(nbody::OfflineHeadless<Sim> &runner, const RadialOptions &ro) {
    const nbody::RadialProfile r = runner.radial_profile(nbody::radial_edges(ro.rmin, ro.rmax, ro.bins, ro.log), ro.params);
    const nb_radial_profile &p = r.profile;
    const unsigned long long step = p.step_num;
    std::printf("Radial: step %llu n %llu nonfinite %llu nbins %u flags %u inside_count %llu inside_mass %.17g "
                "outside_count %llu outside_mass %.17g mass %.17g center %.17g %.17g %.17g velocity %.17g %.17g %.17g "
                "axis %.17g %.17g %.17g shape %.17g %.17g %.17g %.17g %.17g %.17g\n",
                step, (unsigned long long)p.n, (unsigned long long)p.nonfinite, p.nbins, p.flags,
                (unsigned long long)p.inside_count, p.inside_mass, (unsigned long long)p.outside_count, p.outside_mass,
                p.mass, p.center[0], p.center[1], p.center[2], p.velocity[0], p.velocity[1], p.velocity[2], p.axis[0],
                p.axis[1], p.axis[2], p.shape[0], p.shape[1], p.shape[2], p.shape[3], p.shape[4], p.shape[5]);
    for (uint32_t k = 0; k < p.nbins; ++k) {
        const nbody::RadialBin &b = r.bins[k];
        std::printf("RadialBin: step %llu bin %u lo %.17g hi %.17g count %llu mass %.17g m_r %.17g m_ur %.17g m_ur2 %.17g "
                    "m_uphi %.17g m_uphi2 %.17g m_u2 %.17g ang %.17g %.17g %.17g\n",
                    step, k, r.edges[k], r.edges[k + 1], (unsigned long long)b.count, b.mass, b.m_r, b.m_ur, b.m_ur2,
                    b.m_uphi, b.m_uphi2, b.m_u2, b.ang[0], b.ang[1], b.ang[2]);
    }
}

struct RotcurveOptions {
    int every = 0;
    uint32_t bins = 32, phi = 16;
    bool have_range = false;
    double rmin = 0.0, rmax = 0.0;
    std::array<double, 3> axis{0.0, 1.0, 0.0}, center{0.0, 0.0, 0.0};
};

template <class Sim>
static void print_rotcurve(nbody::OfflineHeadless<Sim> &runner, const RotcurveOptions &ro) {
    std::vector<double> radii(ro.bins);
    for (uint32_t i = 0; i < ro.bins; ++i)
        radii[i] = ro.bins > 1 ? ro.rmin + (ro.rmax - ro.rmin) * (double)i / (double)(ro.bins - 1) : ro.rmin;
    const nbody::RingMeans r = runner.circular_velocity(radii, ro.axis, ro.center, ro.phi);
    for (uint32_t i = 0; i < ro.bins; ++i)
        std::printf("rotcurve %llu %.9e %.9e %.9e %.9e\n", (unsigned long long)r.field.stats.step_num, radii[i],
                    r.rings[i].a_R, r.rings[i].a_n, r.rings[i].v_c);
}

// --freq: the rings are --rotcurve's, so are the options
template <class Sim>
static void print_freq(nbody::OfflineHeadless<Sim> &runner, const RotcurveOptions &fo) {
    std::vector<double> radii(fo.bins);
    for (uint32_t i = 0; i < fo.bins; ++i)
        radii[i] = fo.bins > 1 ? fo.rmin + (fo.rmax - fo.rmin) * (double)i / (double)(fo.bins - 1) : fo.rmin;
    const nbody::DiscFrequencies f = runner.disc_frequencies(radii, fo.axis, fo.center, fo.phi);
    for (uint32_t i = 0; i < fo.bins; ++i)
        std::printf("freq %llu %.9e %.9e %.9e %.9e %.9e\n", (unsigned long long)f.tidal.stats.step_num, radii[i],
                    f.omega(i), f.kappa(i), f.nu(i), f.means.rings[i].v_c);
}

// DIR/<name>: NumPy format 1.0, <f8, shape (1 + planes, H, W): the counts as doubles, then the planes
static bool write_npy_planes(const std::string &path, uint32_t width, uint32_t height, const std::vector<uint32_t> &counts,
                             const std::vector<double> &planes) {
    std::FILE *out = std::fopen(path.c_str(), "wb");
    if (!out) {
        std::fprintf(stderr, "cannot write %s\n", path.c_str());
        return false;
    }
    // magic, version, a little-endian uint16 header length, the header padded with spaces to a multiple of 64
    // bytes in all and ended by a newline
    const size_t cells = (size_t)width * height;
    char dict[128];
    const int len = std::snprintf(dict, sizeof dict, "{'descr': '<f8', 'fortran_order': False, 'shape': (%zu, %u, %u), }",
                                  1 + planes.size() / cells, height, width);
    const size_t total = (10 + (size_t)len + 1 + 63) / 64 * 64, hlen = total - 10;
    std::string head("\x93NUMPY\x01\x00", 8);
    head += (char)(hlen & 0xff);
    head += (char)(hlen >> 8);
    head += dict;
    head.append(total - 1 - head.size(), ' ');
    head += '\n';
    std::vector<double> cnt(cells);
    for (size_t i = 0; i < cells; ++i) cnt[i] = (double)counts[i];
    bool ok = std::fwrite(head.data(), 1, head.size(), out) == head.size() &&
              std::fwrite(cnt.data(), sizeof(double), cells, out) == cells &&
              std::fwrite(planes.data(), sizeof(double), planes.size(), out) == planes.size();
    if (std::fclose(out) != 0 || !ok) {
        std::fprintf(stderr, "cannot write %s\n", path.c_str());
        return false;
    }
    return true;
}

struct OrbitsOptions {
    std::string dir;
    int at = 0;
    uint32_t bins = 32, steps = 0, every = 1;
    bool have_range = false;
    double rmin = 0.0, rmax = 0.0, dt = 0.0, omega = 0.0, speed = 1.0;
    std::array<double, 3> axis{0.0, 1.0, 0.0}, center{0.0, 0.0, 0.0};
};

template <class Sim>
static bool write_orbits(nbody::OfflineHeadless<Sim> &runner, const OrbitsOptions &oo) {
    std::vector<double> radii(oo.bins);
    for (uint32_t i = 0; i < oo.bins; ++i)
        radii[i] = oo.bins > 1 ? oo.rmin + (oo.rmax - oo.rmin) * (double)i / (double)(oo.bins - 1) : oo.rmin;
    const nb_orbit_params p = nbody::orbit_params(oo.dt, oo.steps, oo.every, true, oo.omega, oo.axis, oo.center);
    const nbody::Orbits o = runner.circular_orbits(p, radii, 16, oo.speed);
    char name[64];
    std::snprintf(name, sizeof name, "/orbits_%06llu.npy", (unsigned long long)o.stats.step_num);
    const std::string path = oo.dir + name;
    std::FILE *out = std::fopen(path.c_str(), "wb");
    if (!out) {
        std::fprintf(stderr, "cannot write %s\n", path.c_str());
        return false;
    }
    // the header of write_npy_planes; an nb_orbit_sample is eight doubles
    char dict[128];
    const int len = std::snprintf(dict, sizeof dict, "{'descr': '<f8', 'fortran_order': False, 'shape': (%u, %zu, 8), }",
                                  o.records, o.tracers);
    const size_t total = (10 + (size_t)len + 1 + 63) / 64 * 64, hlen = total - 10;
    std::string head("\x93NUMPY\x01\x00", 8);
    head += (char)(hlen & 0xff);
    head += (char)(hlen >> 8);
    head += dict;
    head.append(total - 1 - head.size(), ' ');
    head += '\n';
    static_assert(sizeof(nbody::OrbitSample) == 8 * sizeof(double), "a sample is eight doubles");
    const bool ok = std::fwrite(head.data(), 1, head.size(), out) == head.size() &&
                    std::fwrite(o.tracks.data(), sizeof(nbody::OrbitSample), o.tracks.size(), out) == o.tracks.size();
    if (std::fclose(out) != 0 || !ok) {
        std::fprintf(stderr, "cannot write %s\n", path.c_str());
        return false;
    }
    std::printf("orbits %llu %u %zu %llu %u\n", (unsigned long long)o.stats.step_num, o.records, o.tracers,
                (unsigned long long)o.stats.nonfinite_tracers, o.stats.pair_launches);
    return true;
}

struct SectionsOptions {
    OrbitsOptions launch;  // dir, at, the rings, dt, steps, omega, speed, axis, center
    std::array<double, 3> normal{0.0, 1.0, 0.0};
    double offset = 0.0;
    int direction = 1;
    uint32_t max_crossings = 256;
};

// NumPy format 1.0, <f8, C order: the header for `shape` (the text between the brackets)
static std::string npy_head_f8(const char *shape) {
    char dict[128];
    const int len = std::snprintf(dict, sizeof dict, "{'descr': '<f8', 'fortran_order': False, 'shape': (%s), }", shape);
    const size_t total = (10 + (size_t)len + 1 + 63) / 64 * 64, hlen = total - 10;
    std::string head("\x93NUMPY\x01\x00", 8);
    head += (char)(hlen & 0xff);
    head += (char)(hlen >> 8);
    head += dict;
    head.append(total - 1 - head.size(), ' ');
    head += '\n';
    return head;
}

static bool write_f8(const std::string &path, const char *shape, const std::vector<double> &data) {
    std::FILE *out = std::fopen(path.c_str(), "wb");
    const std::string head = npy_head_f8(shape);
    const bool ok = out && std::fwrite(head.data(), 1, head.size(), out) == head.size() &&
                    std::fwrite(data.data(), sizeof(double), data.size(), out) == data.size();
    if (!out || std::fclose(out) != 0 || !ok) {
        std::fprintf(stderr, "cannot write %s\n", path.c_str());
        return false;
    }
    return true;
}

template <class Sim>
static bool write_sections(nbody::OfflineHeadless<Sim> &runner, const SectionsOptions &so) {
    const OrbitsOptions &oo = so.launch;
    std::vector<double> radii(oo.bins);
    for (uint32_t i = 0; i < oo.bins; ++i)
        radii[i] = oo.bins > 1 ? oo.rmin + (oo.rmax - oo.rmin) * (double)i / (double)(oo.bins - 1) : oo.rmin;
    const nb_orbit_params p = nbody::orbit_params(oo.dt, oo.steps, oo.steps, false, oo.omega, oo.axis, oo.center);
    const nb_orbit_section_params sec = nbody::orbit_section_params(so.normal, so.offset, so.direction, so.max_crossings);
    const nbody::OrbitSections o = runner.circular_orbit_sections(p, sec, radii, 16, oo.speed);
    const size_t m = o.orbits.tracers, cap = o.max_crossings;
    std::vector<double> rows(m * cap * 8, 0.0), counts(m);
    for (size_t i = 0; i < m; ++i) {
        counts[i] = (double)o.counts[i];
        for (uint32_t j = 0; j < o.stored(i); ++j) {
            const nb_orbit_crossing &c = o.at(i, j);
            double *r = rows.data() + (i * cap + j) * 8;
            for (int a = 0; a < 3; ++a) {
                r[a] = c.xi[a];
                r[3 + a] = c.eta[a];
            }
            r[6] = c.time;
            r[7] = (double)c.step;
        }
    }
    char name[64], shape[64];
    const unsigned long long step = (unsigned long long)o.stats.orbit.step_num;
    std::snprintf(name, sizeof name, "/sections_%06llu.npy", step);
    std::snprintf(shape, sizeof shape, "%zu, %zu, 8", m, cap);
    if (!write_f8(so.launch.dir + name, shape, rows)) return false;
    std::snprintf(name, sizeof name, "/sections_%06llu_counts.npy", step);
    std::snprintf(shape, sizeof shape, "%zu,", m);
    if (!write_f8(so.launch.dir + name, shape, counts)) return false;
    std::printf("sections %llu %zu %llu %llu %llu %u\n", step, m, (unsigned long long)o.stats.crossings,
                (unsigned long long)o.stats.stored, (unsigned long long)o.stats.overflowed,
                o.stats.orbit.pair_launches);
    return true;
}

// --stability: --orbits' tracers with two deviation vectors each -- the unit dx along the tracer's radius in the
// plane of its ring, and the unit dx along the axis -- and what nb_orbit_stability_derive reads at the last state
template <class Sim>
static bool write_stability(nbody::OfflineHeadless<Sim> &runner, const OrbitsOptions &oo) {
    std::vector<double> radii(oo.bins);
    for (uint32_t i = 0; i < oo.bins; ++i)
        radii[i] = oo.bins > 1 ? oo.rmin + (oo.rmax - oo.rmin) * (double)i / (double)(oo.bins - 1) : oo.rmin;
    const nb_orbit_params p = nbody::orbit_params(oo.dt, oo.steps, oo.steps, false, oo.omega, oo.axis, oo.center);
    std::vector<double> pos, vel;
    runner.circular_launch(p, radii, 16, oo.speed, pos, vel);
    const size_t m = radii.size();
    double n[3], e1[3], e2[3];
    nbody::check(nb_map_frame(oo.axis.data(), n, e1, e2));
    std::vector<nb_orbit_deviation> dev0(2 * m);
    for (size_t i = 0; i < m; ++i) {
        double d[3], len2 = 0.0;
        const double *x = pos.data() + 3 * i;
        for (int a = 0; a < 3; ++a) d[a] = x[a] - oo.center[(size_t)a];
        const double l = (d[0] * n[0] + d[1] * n[1]) + d[2] * n[2];
        for (int a = 0; a < 3; ++a) {
            d[a] = d[a] - l * n[a];
            len2 += d[a] * d[a];
        }
        const double len = std::sqrt(len2);
        for (int a = 0; a < 3; ++a) {
            dev0[2 * i].d[a] = len > 0.0 ? d[a] / len : e1[a];
            dev0[2 * i + 1].d[a] = n[a];
        }
    }
    const nbody::OrbitStability o = runner.orbit_stability(p, pos, vel, dev0);
    const nbody::OrbitStability::Derived dv = o.derive();
    const uint32_t last = o.orbits.records - 1;
    std::vector<double> rows(m * 6);
    for (size_t i = 0; i < m; ++i) {
        double *r = rows.data() + 6 * i;
        r[0] = dv.lyapunov[((size_t)last * m + i) * 2];
        r[1] = dv.lyapunov[((size_t)last * m + i) * 2 + 1];
        r[2] = dv.sali[(size_t)last * m + i];
        r[3] = dv.gali2[(size_t)last * m + i];
        r[4] = (double)o.growth[2 * i].peak_log2;
        r[5] = (double)o.growth[2 * i].peak_step;
    }
    char name[64], shape[64];
    const unsigned long long step = (unsigned long long)o.stats.orbit.step_num;
    std::snprintf(name, sizeof name, "/stability_%06llu.npy", step);
    std::snprintf(shape, sizeof shape, "%zu, 6", m);
    if (!write_f8(oo.dir + name, shape, rows)) return false;
    std::printf("stability %llu %zu %llu %u\n", step, m, (unsigned long long)o.stats.renorms,
                o.stats.orbit.pair_launches);
    return true;
}

struct MapOptions {
    std::string dir;
    int every = 1;
    bool have_size = false, have_extent = false;
    nbody::MapParams params = nbody::map_params(0, 0, 0.0, 0.0, 0.0, 0.0);
};

template <class Sim>
static bool write_map(nbody::OfflineHeadless<Sim> &runner, const MapOptions &mo) {
    const nbody::ProjectedMap m = runner.projected_map(mo.params);
    char name[64];
    std::snprintf(name, sizeof name, "/map_%06llu.npy", (unsigned long long)m.stats.step_num);
    const std::string path = mo.dir + name;
    if (!write_npy_planes(path, m.width, m.height, m.counts, m.planes)) return false;
    std::printf("map %llu %llu %llu %llu %u\n", (unsigned long long)m.stats.step_num,
                (unsigned long long)m.stats.binned_count, (unsigned long long)m.stats.outside_count,
                (unsigned long long)m.stats.nonfinite, m.stats.max_count);
    return true;
}

struct PhaseSide {
    std::string name;
    double lo = 0.0, hi = 0.0;
    uint32_t cells = 0;
    bool log = false;
};

struct PhaseOptions {
    std::string dir, weight;
    int every = 1;
    PhaseSide x, y;
    std::array<double, 3> axis{0.0, 1.0, 0.0};
    std::vector<double> center;  // empty: the centre of mass
};

// NAME,LO,HI,CELLS[,log]
static bool parse_phase_side(const std::string &v, PhaseSide *side) {
    const size_t comma = v.find(',');
    if (comma == std::string::npos) return false;
    side->name = v.substr(0, comma);
    char tail[8] = "";
    const int got = std::sscanf(v.c_str() + comma + 1, "%lf,%lf,%u,%7s", &side->lo, &side->hi, &side->cells, tail);
    if (got < 3 || (got == 4 && std::string(tail) != "log")) return false;
    side->log = got == 4;
    return true;
}

template <class Sim>
static bool write_phase(nbody::OfflineHeadless<Sim> &runner, const PhaseOptions &po) {
    nbody::PhaseParams p = nbody::phase_params(po.x.name, po.y.name, po.weight, po.axis);
    if (!po.center.empty()) {
        p.flags &= ~NB_PHASE_CENTER_COM;
        for (int k = 0; k < 3; ++k) p.center[k] = po.center[(size_t)k];
    }
    const nbody::PhaseMap m = runner.phase_map(p, nbody::phase_edges(po.x.lo, po.x.hi, po.x.cells, po.x.log),
                                               nbody::phase_edges(po.y.lo, po.y.hi, po.y.cells, po.y.log));
    char name[64];
    std::snprintf(name, sizeof name, "/phase_%06llu.npy", (unsigned long long)m.stats.step_num);
    if (!write_npy_planes(po.dir + name, m.width, m.height, m.counts, m.planes)) return false;
    std::printf("phase %llu %llu %llu %llu %llu %u\n", (unsigned long long)m.stats.step_num,
                (unsigned long long)m.stats.binned_count, (unsigned long long)m.stats.outside_count,
                (unsigned long long)m.stats.undefined_count, (unsigned long long)m.stats.nonfinite, m.stats.max_count);
    return true;
}

struct SmapOptions {
    std::string dir;
    int every = 1;
    bool have_size = false, have_extent = false;
    uint32_t k = 32;
    double max_pixels = 64.0;
    nbody::SmoothParams params = nbody::smooth_params(0, 0, 0.0, 0.0, 0.0, 0.0);
};

template <class Sim>
static bool write_smap(nbody::OfflineHeadless<Sim> &runner, const SmapOptions &so) {
    const nbody::SmoothedMap m = runner.smoothed_map_knn(so.params, so.k);
    char name[64];
    std::snprintf(name, sizeof name, "/smap_%06llu.npy", (unsigned long long)m.stats.step_num);
    if (!write_npy_planes(so.dir + name, m.width, m.height, m.counts, m.planes)) return false;
    std::printf("smap %llu %llu %llu %llu %llu %llu %u %llu\n", (unsigned long long)m.stats.step_num,
                (unsigned long long)m.stats.deposited, (unsigned long long)m.stats.skipped,
                (unsigned long long)m.stats.bad_smoothing, (unsigned long long)m.stats.nonfinite,
                (unsigned long long)m.stats.pairs, m.stats.max_count, (unsigned long long)m.stats.tile_entries);
    return true;
}

struct FofOptions {
    int every = 0, top = 0;
    double link = 0.0;
    uint32_t min_members = 20;
};

template <class Sim>
static void print_fof(nbody::OfflineHeadless<Sim> &runner, const FofOptions &fo) {
    const nbody::FofGroups g = runner.fof_groups(fo.link, fo.min_members, false);
    const unsigned long long step = (unsigned long long)g.stats.step_num;
    std::printf("fof %llu %llu %llu %u\n", step, (unsigned long long)g.stats.groups,
                (unsigned long long)g.stats.grouped_bodies, g.stats.largest_count);
    const std::vector<uint32_t> order = g.by_size();
    for (size_t k = 0; k < order.size() && k < (size_t)fo.top; ++k) {
        const nbody::FofGroup &r = g.groups[order[k]];
        std::printf("fof_group %llu %u %u %u %.9e %.9e %.9e %.9e\n", step, order[k], r.label, r.count, r.mass,
                    r.mx[0] / r.mass, r.mx[1] / r.mass, r.mx[2] / r.mass);
    }
}

struct Fof6Options {
    int every = 0, top = 0;
    double link = 0.0, vlink = 0.0;
    uint32_t min_members = 20;
};

// --fof6 K: the phase-space groups (nb_fof6_runner) of step 0 and of every K-th step -- friends are within --fof6-link
// B in position and --fof6-vlink V in velocity, (dx / B)^2 + (dv / V)^2 <= 1 -- printed as --fof prints its groups,
// the lines starting "fof6" and "fof6_group"
template <class Sim>
static void print_fof6(nbody::OfflineHeadless<Sim> &runner, const Fof6Options &fo) {
    const nbody::PhaseSpaceGroups g = runner.phase_space_groups(fo.link, fo.vlink, fo.min_members, false);
    const unsigned long long step = (unsigned long long)g.stats.step_num;
    std::printf("fof6 %llu %llu %llu %u\n", step, (unsigned long long)g.stats.groups,
                (unsigned long long)g.stats.grouped_bodies, g.stats.largest_count);
    const std::vector<uint32_t> order = g.by_size();
    for (size_t k = 0; k < order.size() && k < (size_t)fo.top; ++k) {
        const nbody::FofGroup &r = g.groups[order[k]];
        std::printf("fof6_group %llu %u %u %u %.9e %.9e %.9e %.9e\n", step, order[k], r.label, r.count, r.mass,
                    r.mx[0] / r.mass, r.mx[1] / r.mass, r.mx[2] / r.mass);
    }
}

struct BoundOptions {
    int every = 0, top = 0;
    double link = 0.0;
    uint32_t min_members = 20, max_iter = 32, max_group = 262144;
};

template <class Sim>
static void print_bound(nbody::OfflineHeadless<Sim> &runner, const BoundOptions &bo) {
    const nbody::BoundGroups g = runner.bound_groups(bo.link, bo.min_members, 0, bo.max_iter, bo.max_group, false);
    const unsigned long long step = (unsigned long long)g.stats.step_num;
    std::printf("bound %llu %llu %llu %llu %llu %llu %llu %u %llu\n", step, (unsigned long long)g.stats.groups,
                (unsigned long long)g.stats.bound_groups, (unsigned long long)g.stats.bound_bodies,
                (unsigned long long)g.stats.dissolved, (unsigned long long)g.stats.unconverged,
                (unsigned long long)g.stats.skipped, g.stats.rounds_max, (unsigned long long)g.stats.pairs);
    const std::vector<uint32_t> order = g.by_bound_mass();
    for (size_t k = 0; k < order.size() && k < (size_t)bo.top; ++k) {
        const nbody::BoundGroup &r = g.groups[order[k]];
        std::printf("bound_group %llu %u %u %u %u %u %u %.9e %.9e %.9e %.9e %.9e %.9e\n", step, order[k], r.label,
                    r.count, r.bound_count, r.iterations, r.status, r.mass, r.mx[0] / r.mass, r.mx[1] / r.mass,
                    r.mx[2] / r.mass, r.kinetic, r.potential);
    }
}

struct ShapesOptions {
    int every = 0, top = 0;
    double link = 0.0, k_rms = 0.0;
    uint32_t min_members = 20, max_iter = 32;
    bool reduced = false;
};

template <class Sim>
static void print_shapes(nbody::OfflineHeadless<Sim> &runner, const ShapesOptions &so) {
    const nbody::FofGroups f = runner.fof_groups(so.link, so.min_members, false);
    nbody::ShapeOptions o;
    o.reduced = so.reduced;
    o.max_iter = so.max_iter;
    const nbody::GroupShapes g = runner.group_shapes(f, so.k_rms, o);
    const unsigned long long step = (unsigned long long)g.stats.step_num;
    std::printf("shapes %llu %llu %llu %llu %llu %llu %u\n", step, (unsigned long long)g.stats.rows,
                (unsigned long long)g.stats.converged, (unsigned long long)g.stats.unconverged,
                (unsigned long long)g.stats.degenerate, (unsigned long long)g.stats.empty, g.stats.rounds_max);
    const std::vector<uint32_t> order = f.by_size();
    for (size_t k = 0; k < order.size() && k < (size_t)so.top; ++k) {
        const nbody::ShapeGroup &r = g.rows[order[k]];
        std::printf("shape_group %llu %u %u %u %.17g %.17g %.17g %.17g %u\n", step, order[k], r.count, r.selected, r.q,
                    r.s, g.triaxiality(order[k]), g.j_norm(order[k]), r.status);
    }
}

struct LagrOptions {
    int every = 0;
    std::vector<double> fractions{0.01, 0.05, 0.1, 0.25, 0.5, 0.75, 0.9};
    std::vector<double> center;  // empty: the centre of mass
};

template <class Sim>
static void print_lagr(nbody::OfflineHeadless<Sim> &runner, const LagrOptions &lo) {
    nbody::RadiiOptions o;
    o.fractions = lo.fractions;
    const nbody::GroupRadii g = runner.lagrangian_radii(o, lo.center);
    const unsigned long long step = (unsigned long long)g.stats.step_num;
    const nbody::RadiiGroup &r = g.rows[0];
    std::printf("lagr %llu %u %.17g %.17g %.17g %.17g %.17g %.17g\n", step, r.count, r.mass, r.center[0], r.center[1],
                r.center[2], r.r_vmax, r.vc2_max);
    for (size_t f = 0; f < g.fractions.size(); ++f)
        std::printf("lagr_radius %llu %.17g %.17g %u\n", step, g.fractions[f], r.radius[f], r.index[f]);
}

struct RadiiCliOptions {
    int every = 0, top = 0;
    double link = 0.0;
    uint32_t min_members = 20;
};

template <class Sim>
static void print_radii(nbody::OfflineHeadless<Sim> &runner, const RadiiCliOptions &ro) {
    const nbody::FofGroups f = runner.fof_groups(ro.link, ro.min_members, false);
    const nbody::GroupRadii g = runner.group_radii(f);
    const unsigned long long step = (unsigned long long)g.stats.step_num;
    std::printf("radii %llu %llu %llu %llu\n", step, (unsigned long long)g.stats.rows,
                (unsigned long long)g.stats.members, (unsigned long long)g.stats.empty);
    std::vector<uint32_t> row_of(f.groups.size(), NB_FOF_NONE);  // a catalogue row without a finite centre has none
    for (size_t r = 0; r < g.catalogue_rows.size(); ++r) row_of[g.catalogue_rows[r]] = (uint32_t)r;
    const std::vector<uint32_t> order = f.by_size();
    for (size_t k = 0, shown = 0; k < order.size() && shown < (size_t)ro.top; ++k) {
        if (row_of[order[k]] == NB_FOF_NONE) continue;
        ++shown;
        const nbody::RadiiGroup &r = g.rows[row_of[order[k]]];
        std::printf("radii_group %llu %u %u %.17g %.17g %.17g %.17g %.17g %.17g\n", step, order[k], r.count, r.mass,
                    r.radius[0], r.radius[1], r.radius[2], r.r_vmax, r.vc2_max);
    }
}

struct ModesOptions {
    int every = 0;
    bool have_range = false, log = false;
    double rmin = 0.0, rmax = 0.0;
    uint32_t bins = 32, mmax = 4;
    double axis[3] = {0.0, 1.0, 0.0};
    std::vector<double> center;  // empty: the centre of mass
};

template <class Sim>
static void print_modes(nbody::OfflineHeadless<Sim> &runner, const ModesOptions &mo) {
    nbody::ModesParams p{};
    p.mmax = mo.mmax;
    p.flags = mo.center.empty() ? NB_MODES_CENTER_COM : 0u;
    for (int a = 0; a < 3; ++a) {
        p.axis[a] = mo.axis[a];
        p.center[a] = mo.center.empty() ? 0.0 : mo.center[a];
    }
    const nbody::DiscModes d = runner.disc_modes(nbody::radial_edges(mo.rmin, mo.rmax, mo.bins, mo.log), p);
    const nbody::BarStrength bar = d.bar_strength();
    const double nan = std::nan("");
    double radius = nan, phase = nan, omega = nan, tilt = nan;
    if (bar.bin >= 0) {
        const nbody::ModesDerived m2 = d.derived(2)[bar.bin];
        radius = d.bins[bar.bin].m_r / d.field(bar.bin, 0, NB_MODES_C);
        phase = m2.phase;
        omega = m2.pattern_speed;
    }
    for (size_t k = 0; k < d.bins.size(); ++k) {
        const double t = d.warp_tilt(k);
        if (std::isfinite(t) && !(t <= tilt)) tilt = t;
    }
    std::printf("modes %llu %.17g %.17g %.17g %.17g %.17g\n", (unsigned long long)d.head.step_num, bar.a2, radius,
                phase, omega, tilt);
}

struct ShellsOptions {
    int every = 0;
    bool have_range = false, log = true, rates = false;
    double rmin = 0.0, rmax = 0.0;
    uint32_t bins = 32, lmax = 4;
    double axis[3] = {0.0, 1.0, 0.0};
    std::vector<double> center;  // empty: the centre of mass
};

template <class Sim>
static void print_shells(nbody::OfflineHeadless<Sim> &runner, const ShellsOptions &so) {
    nbody::ShellParams p{};
    p.lmax = so.lmax;
    p.flags = (so.center.empty() ? NB_SHELL_CENTER_COM : 0u) | (so.rates ? NB_SHELL_RATES : 0u);
    for (int a = 0; a < 3; ++a) {
        p.axis[a] = so.axis[a];
        p.center[a] = so.center.empty() ? 0.0 : so.center[a];
    }
    const nbody::ShellModes d = runner.shell_modes(nbody::radial_edges(so.rmin, so.rmax, so.bins, so.log), p);
    const std::vector<double> rel1 = d.relative(1), rel2 = d.relative(2);
    const double nan = std::nan("");
    double q2 = nan, radius = nan, phase = nan, omega = nan, d1 = nan;
    int best = -1;
    for (size_t k = 0; k < rel2.size(); ++k) {
        if (std::isfinite(rel2[k]) && (best < 0 || rel2[k] > q2)) {
            q2 = rel2[k];
            best = (int)k;
        }
        if (std::isfinite(rel1[k]) && !(rel1[k] <= d1)) d1 = rel1[k];
    }
    if (best >= 0) {
        radius = d.bins[best].m_r / d.coefficient(best, 0, 0);
        phase = d.phase(2, 2)[best];
        if (d.rates()) omega = d.pattern_speed(2, 2)[best];
    }
    std::printf("shells %llu %.17g %.17g %.17g %.17g %.17g\n", (unsigned long long)d.head.step_num, q2, radius, phase,
                omega, d1);
}

struct KnnOptions {
    int every = 0;
    uint32_t k = 6;
};

template <class Sim>
static void print_knn(nbody::OfflineHeadless<Sim> &runner, const KnnOptions &ko) {
    const nbody::KnnDensity d = runner.knn_density(ko.k, false, false);
    const std::array<double, 3> c = d.center(), v = d.center_velocity();
    std::printf("knn %llu %llu %llu %.17g %.17g %.17g %.17g %.17g %.17g %.17g %u\n",
                (unsigned long long)d.stats.step_num, (unsigned long long)d.stats.counted,
                (unsigned long long)d.stats.degenerate, c[0], c[1], c[2], v[0], v[1], v[2], d.stats.peak_density,
                d.stats.peak_index);
}

struct MstOptions {
    int every = 0;
    std::vector<double> links;
    uint32_t min_members = 1;
    bool have_min = false;
    std::string dir;
};

template <class Sim>
static bool print_mst(nbody::OfflineHeadless<Sim> &runner, const MstOptions &mo) {
    const nbody::SpanningTree t = runner.spanning_tree(true);
    std::printf("mst %llu %llu %u %.17g %.17g", (unsigned long long)t.stats.step_num, (unsigned long long)t.stats.edges,
                t.stats.rounds, t.total_length(), t.longest());
    for (uint64_t c : t.group_counts(mo.links, mo.min_members)) std::printf(" %llu", (unsigned long long)c);
    std::printf("\n");
    if (mo.dir.empty()) return true;
    std::vector<double> rows(3 * t.d2.size());
    for (size_t e = 0; e < t.d2.size(); ++e) {
        rows[3 * e] = (double)t.edge_lo[e];
        rows[3 * e + 1] = (double)t.edge_hi[e];
        rows[3 * e + 2] = t.d2[e];
    }
    char name[64], shape[64];
    std::snprintf(name, sizeof name, "/mst_%llu.npy", (unsigned long long)t.stats.step_num);
    std::snprintf(shape, sizeof shape, "%zu, 3", t.d2.size());
    return write_f8(mo.dir + name, shape, rows);
}

struct KinOptions {
    int every = 0;
    uint32_t k = 32;
    bool gradient = false;
};

template <class Sim>
static void print_kin(nbody::OfflineHeadless<Sim> &runner, const KinOptions &ko) {
    const nbody::LocalKinematics d = runner.local_kinematics(ko.k, ko.gradient, true, false);
    const std::vector<nbody::Particle> parts = runner.read_particles();
    unsigned long long singular = 0;
    double ms = 0.0, m = 0.0, q_max = std::nan("");
    uint32_t q_at = 0xFFFFFFFFu;
    for (size_t i = 0; i < d.derived.size(); ++i) {
        const nbody::KinDerived &r = d.derived[i];
        if (r.status & NB_KIN_SINGULAR) ++singular;
        if (std::isfinite(r.sigma)) {
            ms += (double)parts[i].mass * r.sigma;
            m += (double)parts[i].mass;
        }
        if (std::isfinite(r.phase_space_density) && !(r.phase_space_density <= q_max)) {
            q_max = r.phase_space_density;
            q_at = (uint32_t)i;
        }
    }
    std::printf("kin %llu %llu %llu %llu %.17g %.17g %u\n", (unsigned long long)d.stats.step_num,
                (unsigned long long)d.stats.counted, (unsigned long long)d.stats.degenerate, singular, ms / m, q_max,
                q_at);
}

struct HopOptions {
    int every = 0, top = 0;
    nbody::HopParams params;
    bool regroup = false;
    double saddle = 0.0, peak = 0.0;
};

static void print_hop_rows(const char *tag, const nbody::HopGroups &g, int top) {
    const unsigned long long step = (unsigned long long)g.stats.step_num;
    const std::vector<uint32_t> order = g.by_size();
    for (size_t k = 0; k < order.size() && k < (size_t)top; ++k) {
        const nbody::FofGroup &r = g.groups[order[k]];
        std::printf("%s %llu %u %u %u %.9e %.9e %.9e %.9e %.9e\n", tag, step, order[k], r.label, r.count, r.mass,
                    r.mx[0] / r.mass, r.mx[1] / r.mass, r.mx[2] / r.mass, g.peak_density[order[k]]);
    }
}

template <class Sim>
static void print_hop(nbody::OfflineHeadless<Sim> &runner, const HopOptions &ho) {
    const nbody::HopGroups g = runner.hop_groups(ho.params, false, false, true);
    const unsigned long long step = (unsigned long long)g.stats.step_num;
    std::printf("hop %llu %llu %llu %llu %u %llu %llu\n", step, (unsigned long long)g.stats.peaks,
                (unsigned long long)g.stats.groups, (unsigned long long)g.stats.grouped_bodies, g.stats.largest_count,
                (unsigned long long)g.stats.boundaries, (unsigned long long)g.stats.boundary_pairs);
    print_hop_rows("hop_group", g, ho.top);
    if (!ho.regroup) return;
    const nbody::HopGroups m = g.regroup(ho.saddle, ho.peak);
    std::printf("hop_merged %llu %llu %llu %u\n", step, (unsigned long long)m.stats.groups,
                (unsigned long long)m.stats.grouped_bodies, m.stats.largest_count);
    print_hop_rows("hop_merged_group", m, ho.top);
}

struct HaloOptions {
    int every = 0, top = 0;
    double link = 0.0, rmin = 0.0, rmax = 0.0, rho = 0.0;
    uint32_t min_members = 20, bins = 32;
    bool have_range = false;
};

template <class Sim>
static void print_halo(nbody::OfflineHeadless<Sim> &runner, const HaloOptions &ho) {
    const nbody::FofGroups g = runner.fof_groups(ho.link, ho.min_members, false);
    // the rows with a finite centre of mass and velocity (a group of massless bodies has none), as
    // Simulator.group_profiles takes them; profile_of[row]: the row's profile, or -1
    std::vector<double> centers, velocities;
    std::vector<long> profile_of(g.groups.size(), -1);
    for (size_t i = 0; i < g.groups.size(); ++i) {
        const nbody::FofGroup &r = g.groups[i];
        double c[3], v[3];
        bool ok = true;
        for (int a = 0; a < 3; ++a) {
            c[a] = r.mx[a] / r.mass;
            v[a] = r.mv[a] / r.mass;
            ok = ok && std::isfinite(c[a]) && std::isfinite(v[a]);
        }
        if (!ok) continue;
        profile_of[i] = (long)(centers.size() / 3);
        centers.insert(centers.end(), c, c + 3);
        velocities.insert(velocities.end(), v, v + 3);
    }
    const nbody::HaloProfiles h =
        runner.halo_profiles(nbody::radial_edges(ho.rmin, ho.rmax, ho.bins, true), centers, velocities);
    const unsigned long long step = (unsigned long long)h.stats.step_num;
    std::printf("halo %llu %llu %llu %llu\n", step, (unsigned long long)h.stats.centers,
                (unsigned long long)h.stats.tested, (unsigned long long)h.stats.items);
    const std::vector<uint32_t> order = g.by_size();
    for (size_t k = 0; k < order.size() && k < (size_t)ho.top; ++k) {
        const uint32_t row = order[k];
        const double nan = std::nan("");
        if (profile_of[row] < 0) {
            std::printf("halo_group %llu %u %u %u nan nan nan nan\n", step, row, g.groups[row].label, g.groups[row].count);
            continue;
        }
        const size_t pr = (size_t)profile_of[row];
        const std::array<double, 2> od = ho.rho > 0.0 ? h.overdensity(pr, ho.rho) : std::array<double, 2>{nan, nan};
        const std::vector<double> enclosed = h.enclosed(pr);
        double peak = 0.0, r_peak = nan;
        for (size_t e = 0; e < enclosed.size(); ++e)
            if (h.edges[e] > 0.0 && enclosed[e] / h.edges[e] > peak) {
                peak = enclosed[e] / h.edges[e];
                r_peak = h.edges[e];
            }
        std::printf("halo_group %llu %u %u %u %.17g %.17g %.17g %.17g\n", step, row, g.groups[row].label,
                    g.groups[row].count, od[0], od[1], r_peak, peak);
    }
}

struct FrameOptions {
    std::string dir;
    int every = 1;
    uint32_t width = 1280, height = 720;
};

template <class Sim>
static bool write_frame(nbody::OfflineHeadless<Sim> &runner, const FrameOptions &fo) {
    const nbody::Frame f = runner.render(nbody::default_render_params(fo.width, fo.height));
    char name[64];
    std::snprintf(name, sizeof name, "/frame_%06llu.ppm", (unsigned long long)f.stats.step_num);
    const std::string path = fo.dir + name;
    std::FILE *out = std::fopen(path.c_str(), "wb");
    if (!out) {
        std::fprintf(stderr, "cannot write %s\n", path.c_str());
        return false;
    }
    std::vector<uint8_t> rgb((size_t)f.width * f.height * 3);
    for (size_t p = 0; p < (size_t)f.width * f.height; ++p)
        for (int c = 0; c < 3; ++c) rgb[3 * p + c] = f.rgba[4 * p + c];
    const bool ok = std::fprintf(out, "P6\n%u %u\n255\n", f.width, f.height) > 0 &&
                    std::fwrite(rgb.data(), 1, rgb.size(), out) == rgb.size();
    if (std::fclose(out) != 0 || !ok) {
        std::fprintf(stderr, "cannot write %s\n", path.c_str());
        return false;
    }
    std::printf("Frame %llu: drawn %llu clipped %llu oversize %llu nonfinite %llu fragments %llu max_count %u\n",
                (unsigned long long)f.stats.step_num, (unsigned long long)f.stats.drawn,
                (unsigned long long)f.stats.clipped, (unsigned long long)f.stats.oversize,
                (unsigned long long)f.stats.nonfinite, (unsigned long long)f.stats.fragments, f.stats.max_count);
    return true;
}

template <class Sim>
static int run(const nbody::SimParams &sp, const nbody::AddParams &ap, const nbody::InitFn &init,
               int steps, int device, const std::vector<int> &devices, const std::string &dump, int let,
               int diag, bool diag_potential, const FrameOptions &frames, const RadialOptions &radial,
               const RotcurveOptions &rotcurve, const MapOptions &maps, const SmapOptions &smaps, const FofOptions &fof,
               const KnnOptions &knn, const BoundOptions &bound, const HaloOptions &halo, const HopOptions &hop,
               const ShapesOptions &shapes, const LagrOptions &lagr, const RadiiCliOptions &radii,
               const ModesOptions &modes, const PhaseOptions &phase, const RotcurveOptions &freq,
               const KinOptions &kin, const OrbitsOptions &orbits, const Fof6Options &fof6,
               const SectionsOptions &sections, const OrbitsOptions &stability, const ShellsOptions &shells,
               const MstOptions &mst) {
    std::puts("Initializing Simulation");
    nbody::OfflineHeadless<Sim> runner = devices.empty() ? nbody::OfflineHeadless<Sim>(sp, ap, init, device)
                                                         : nbody::OfflineHeadless<Sim>(sp, ap, init, devices, let);
    std::puts("Running Simulation");
    if (diag > 0) print_diag(runner, diag_potential);
    if (radial.every > 0) print_radial(runner, radial);
    if (rotcurve.every > 0) print_rotcurve(runner, rotcurve);
    if (freq.every > 0) print_freq(runner, freq);
    if (!orbits.dir.empty() && orbits.at == 0 && !write_orbits(runner, orbits)) return 1;
    if (!sections.launch.dir.empty() && sections.launch.at == 0 && !write_sections(runner, sections)) return 1;
    if (!stability.dir.empty() && stability.at == 0 && !write_stability(runner, stability)) return 1;
    if (!maps.dir.empty() && !write_map(runner, maps)) return 1;
    if (!smaps.dir.empty() && !write_smap(runner, smaps)) return 1;
    if (fof.every > 0) print_fof(runner, fof);
    if (fof6.every > 0) print_fof6(runner, fof6);
    if (bound.every > 0) print_bound(runner, bound);
    if (knn.every > 0) print_knn(runner, knn);
    if (mst.every > 0 && !print_mst(runner, mst)) return 1;
    if (kin.every > 0) print_kin(runner, kin);
    if (hop.every > 0) print_hop(runner, hop);
    if (halo.every > 0) print_halo(runner, halo);
    if (shapes.every > 0) print_shapes(runner, shapes);
    if (lagr.every > 0) print_lagr(runner, lagr);
    if (radii.every > 0) print_radii(runner, radii);
    if (modes.every > 0) print_modes(runner, modes);
    if (shells.every > 0) print_shells(runner, shells);
    if (!phase.dir.empty() && !write_phase(runner, phase)) return 1;
    if (!frames.dir.empty() && !write_frame(runner, frames)) return 1;
    for (int i = 0; i < steps; ++i) {
        const auto t0 = std::chrono::steady_clock::now();
        runner.step();
        const auto us = std::chrono::duration_cast<std::chrono::microseconds>(
                            std::chrono::steady_clock::now() - t0).count();
        std::printf("Step Duration: %lld \xC2\xB5s\n", (long long)us);
        if (diag > 0 && (i + 1) % diag == 0) print_diag(runner, diag_potential);
        if (radial.every > 0 && (i + 1) % radial.every == 0) print_radial(runner, radial);
        if (rotcurve.every > 0 && (i + 1) % rotcurve.every == 0) print_rotcurve(runner, rotcurve);
        if (freq.every > 0 && (i + 1) % freq.every == 0) print_freq(runner, freq);
        if (!orbits.dir.empty() && i + 1 == orbits.at && !write_orbits(runner, orbits)) return 1;
        if (!sections.launch.dir.empty() && i + 1 == sections.launch.at && !write_sections(runner, sections)) return 1;
        if (!stability.dir.empty() && i + 1 == stability.at && !write_stability(runner, stability)) return 1;
        if (!maps.dir.empty() && (i + 1) % maps.every == 0 && !write_map(runner, maps)) return 1;
        if (!smaps.dir.empty() && (i + 1) % smaps.every == 0 && !write_smap(runner, smaps)) return 1;
        if (fof.every > 0 && (i + 1) % fof.every == 0) print_fof(runner, fof);
        if (fof6.every > 0 && (i + 1) % fof6.every == 0) print_fof6(runner, fof6);
        if (bound.every > 0 && (i + 1) % bound.every == 0) print_bound(runner, bound);
        if (knn.every > 0 && (i + 1) % knn.every == 0) print_knn(runner, knn);
        if (mst.every > 0 && (i + 1) % mst.every == 0 && !print_mst(runner, mst)) return 1;
        if (kin.every > 0 && (i + 1) % kin.every == 0) print_kin(runner, kin);
        if (hop.every > 0 && (i + 1) % hop.every == 0) print_hop(runner, hop);
        if (halo.every > 0 && (i + 1) % halo.every == 0) print_halo(runner, halo);
        if (shapes.every > 0 && (i + 1) % shapes.every == 0) print_shapes(runner, shapes);
        if (lagr.every > 0 && (i + 1) % lagr.every == 0) print_lagr(runner, lagr);
        if (radii.every > 0 && (i + 1) % radii.every == 0) print_radii(runner, radii);
        if (modes.every > 0 && (i + 1) % modes.every == 0) print_modes(runner, modes);
        if (shells.every > 0 && (i + 1) % shells.every == 0) print_shells(runner, shells);
        if (!phase.dir.empty() && (i + 1) % phase.every == 0 && !write_phase(runner, phase)) return 1;
        if (!frames.dir.empty() && (i + 1) % frames.every == 0 && !write_frame(runner, frames)) return 1;
    }
    std::puts("Finished Running");
    if (!dump.empty()) {
        const std::vector<nbody::Particle> parts = runner.read_particles();
        if (!write_snapshot(dump, sp, parts, runner.step_num())) {
            std::fprintf(stderr, "cannot write %s\n", dump.c_str());
            return 1;
        }
    }
    return 0;
}

int main(int argc, char **argv) {
    std::string sim = "tree", init = "uniform", dump;
    std::vector<int> devices;
    nbody::SimParams sp{4000000u, 0.000001f, 0.0001f, 0.016f};  // headless.rs:15-20
    float theta = 0.75f;
    int steps = 10, device = -1, let = -1, diag = 0;
    bool diag_potential = false;
    FrameOptions frames;
    RadialOptions radial;
    RotcurveOptions rotcurve, freq;
    MapOptions maps;
    SmapOptions smaps;
    FofOptions fof;
    KnnOptions knn;
    MstOptions mst;
    KinOptions kin;
    OrbitsOptions orbits;
    SectionsOptions sections;
    OrbitsOptions stability;
    Fof6Options fof6;
    BoundOptions bound;
    HaloOptions halo;
    HopOptions hop;
    ShapesOptions shapes;
    LagrOptions lagr;
    RadiiCliOptions radii;
    ModesOptions modes;
    ShellsOptions shells;
    PhaseOptions phase;
    bool hop_saddle = false, hop_peak = false;
    uint64_t seed = 0;
    for (int i = 1; i + 1 < argc; i += 2) {
        const std::string k = argv[i], v = argv[i + 1];
        if (k == "--sim") sim = v;
        else if (k == "--n") sp.particle_num = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--steps") steps = std::atoi(v.c_str());
        else if (k == "--theta") theta = (float)std::atof(v.c_str());
        else if (k == "--init") init = v;
        else if (k == "--seed") seed = std::strtoull(v.c_str(), nullptr, 10);
        else if (k == "--device") device = std::atoi(v.c_str());
        else if (k == "--g") sp.g = (float)std::atof(v.c_str());
        else if (k == "--e") sp.e = (float)std::atof(v.c_str());
        else if (k == "--dt") sp.dt = (float)std::atof(v.c_str());
        else if (k == "--dump") dump = v;
        else if (k == "--let") let = std::atoi(v.c_str());  // with --devices and --sim tree: LET scheme, migrate every k-th step
        else if (k == "--diag") diag = std::atoi(v.c_str());
        else if (k == "--diag-potential") diag_potential = std::atoi(v.c_str()) != 0;
        else if (k == "--radial") radial.every = std::atoi(v.c_str());
        else if (k == "--radial-bins") radial.bins = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--radial-log") radial.log = std::atoi(v.c_str()) != 0;
        else if (k == "--radial-range") {
            if (std::sscanf(v.c_str(), "%lf,%lf", &radial.rmin, &radial.rmax) != 2) {
                std::fprintf(stderr, "--radial-range takes RMIN,RMAX, not %s\n", v.c_str());
                return 2;
            }
            radial.have_range = true;
        }
        else if (k == "--radial-axis") {
            double *a = radial.params.axis;
            if (std::sscanf(v.c_str(), "%lf,%lf,%lf", &a[0], &a[1], &a[2]) != 3) {
                std::fprintf(stderr, "--radial-axis takes X,Y,Z, not %s\n", v.c_str());
                return 2;
            }
            radial.params.flags |= NB_RADIAL_CYLINDRICAL;
        }
        else if (k == "--radial-center") {
            double *c = radial.params.center;
            if (v == "com") radial.params.flags |= NB_RADIAL_CENTER_COM;
            else if (std::sscanf(v.c_str(), "%lf,%lf,%lf", &c[0], &c[1], &c[2]) == 3)
                radial.params.flags &= ~NB_RADIAL_CENTER_COM;
            else {
                std::fprintf(stderr, "--radial-center takes com or X,Y,Z, not %s\n", v.c_str());
                return 2;
            }
        }
        else if (k == "--rotcurve") rotcurve.every = std::atoi(v.c_str());
        else if (k == "--rotcurve-bins") rotcurve.bins = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--rotcurve-phi") rotcurve.phi = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--rotcurve-range") {
            if (std::sscanf(v.c_str(), "%lf,%lf", &rotcurve.rmin, &rotcurve.rmax) != 2) {
                std::fprintf(stderr, "--rotcurve-range takes RMIN,RMAX, not %s\n", v.c_str());
                return 2;
            }
            rotcurve.have_range = true;
        }
        else if (k == "--rotcurve-axis" || k == "--rotcurve-center") {
            double *a = k == "--rotcurve-axis" ? rotcurve.axis.data() : rotcurve.center.data();
            if (std::sscanf(v.c_str(), "%lf,%lf,%lf", &a[0], &a[1], &a[2]) != 3) {
                std::fprintf(stderr, "%s takes X,Y,Z, not %s\n", k.c_str(), v.c_str());
                return 2;
            }
        }
        else if (k == "--freq") freq.every = std::atoi(v.c_str());
        else if (k == "--freq-bins") freq.bins = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--freq-phi") freq.phi = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--freq-range") {
            if (std::sscanf(v.c_str(), "%lf,%lf", &freq.rmin, &freq.rmax) != 2) {
                std::fprintf(stderr, "--freq-range takes RMIN,RMAX, not %s\n", v.c_str());
                return 2;
            }
            freq.have_range = true;
        }
        else if (k == "--freq-axis" || k == "--freq-center") {
            double *a = k == "--freq-axis" ? freq.axis.data() : freq.center.data();
            if (std::sscanf(v.c_str(), "%lf,%lf,%lf", &a[0], &a[1], &a[2]) != 3) {
                std::fprintf(stderr, "%s takes X,Y,Z, not %s\n", k.c_str(), v.c_str());
                return 2;
            }
        }
        else if (k == "--maps") maps.dir = v;
        else if (k == "--map-every") maps.every = std::max(1, std::atoi(v.c_str()));
        else if (k == "--map-size") {
            if (std::sscanf(v.c_str(), "%ux%u", &maps.params.width, &maps.params.height) != 2) {
                std::fprintf(stderr, "--map-size takes WxH, not %s\n", v.c_str());
                return 2;
            }
            maps.have_size = true;
        }
        else if (k == "--map-extent") {
            nbody::MapParams &mp = maps.params;
            if (std::sscanf(v.c_str(), "%lf,%lf,%lf,%lf", &mp.x_range[0], &mp.x_range[1], &mp.y_range[0],
                            &mp.y_range[1]) != 4) {
                std::fprintf(stderr, "--map-extent takes X0,X1,Y0,Y1, not %s\n", v.c_str());
                return 2;
            }
            maps.have_extent = true;
        }
        else if (k == "--map-axis") {
            double *a = maps.params.axis;
            if (std::sscanf(v.c_str(), "%lf,%lf,%lf", &a[0], &a[1], &a[2]) != 3) {
                std::fprintf(stderr, "--map-axis takes X,Y,Z, not %s\n", v.c_str());
                return 2;
            }
        }
        else if (k == "--map-center") {
            double *c = maps.params.center;
            if (v == "com") maps.params.flags |= NB_MAP_CENTER_COM;
            else if (std::sscanf(v.c_str(), "%lf,%lf,%lf", &c[0], &c[1], &c[2]) == 3)
                maps.params.flags &= ~NB_MAP_CENTER_COM;
            else {
                std::fprintf(stderr, "--map-center takes com or X,Y,Z, not %s\n", v.c_str());
                return 2;
            }
        }
        else if (k == "--map-depth") {
            if (std::sscanf(v.c_str(), "%lf,%lf", &maps.params.depth_range[0], &maps.params.depth_range[1]) != 2) {
                std::fprintf(stderr, "--map-depth takes LO,HI, not %s\n", v.c_str());
                return 2;
            }
        }
        else if (k == "--frames") frames.dir = v;
        else if (k == "--frame-every") frames.every = std::max(1, std::atoi(v.c_str()));
        else if (k == "--frame-size") {
            unsigned w = 0, h = 0;
            if (std::sscanf(v.c_str(), "%ux%u", &w, &h) != 2) {
                std::fprintf(stderr, "--frame-size takes WxH, not %s\n", v.c_str());
                return 2;
            }
            frames.width = w;
            frames.height = h;
        }
        else if (k == "--fof") fof.every = std::atoi(v.c_str());
        else if (k == "--fof-link") fof.link = std::atof(v.c_str());
        else if (k == "--fof-min") fof.min_members = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--fof-top") fof.top = std::atoi(v.c_str());
        else if (k == "--fof6") fof6.every = std::atoi(v.c_str());
        else if (k == "--fof6-link") fof6.link = std::atof(v.c_str());
        else if (k == "--fof6-vlink") fof6.vlink = std::atof(v.c_str());
        else if (k == "--fof6-min") fof6.min_members = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--fof6-top") fof6.top = std::atoi(v.c_str());
        else if (k == "--bound") bound.every = std::atoi(v.c_str());
        else if (k == "--bound-link") bound.link = std::atof(v.c_str());
        else if (k == "--bound-min") bound.min_members = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--bound-iter") bound.max_iter = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--bound-max-group") bound.max_group = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--bound-top") bound.top = std::atoi(v.c_str());
        else if (k == "--shapes") shapes.every = std::atoi(v.c_str());
        else if (k == "--shapes-link") shapes.link = std::atof(v.c_str());
        else if (k == "--shapes-min") shapes.min_members = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--shapes-radius") shapes.k_rms = std::atof(v.c_str());
        else if (k == "--shapes-reduced") shapes.reduced = std::atoi(v.c_str()) != 0;
        else if (k == "--shapes-iter") shapes.max_iter = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--shapes-top") shapes.top = std::atoi(v.c_str());
        else if (k == "--lagr") lagr.every = std::atoi(v.c_str());
        else if (k == "--lagr-fractions") {
            lagr.fractions.clear();
            const char *s = v.c_str();
            char *end = nullptr;
            for (;;) {
                const double f = std::strtod(s, &end);
                if (end == s) break;
                lagr.fractions.push_back(f);
                if (*end != ',') break;
                s = end + 1;
            }
            if (end == s || *end != '\0') {
                std::fprintf(stderr, "--lagr-fractions takes F1,F2,..., not %s\n", v.c_str());
                return 2;
            }
        }
        else if (k == "--lagr-center") {
            lagr.center.assign(3, 0.0);
            if (v == "com") lagr.center.clear();
            else if (std::sscanf(v.c_str(), "%lf,%lf,%lf", &lagr.center[0], &lagr.center[1], &lagr.center[2]) != 3) {
                std::fprintf(stderr, "--lagr-center takes com or X,Y,Z, not %s\n", v.c_str());
                return 2;
            }
        }
        else if (k == "--radii") radii.every = std::atoi(v.c_str());
        else if (k == "--radii-link") radii.link = std::atof(v.c_str());
        else if (k == "--radii-min") radii.min_members = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--radii-top") radii.top = std::atoi(v.c_str());
        else if (k == "--phase") phase.dir = v;
        else if (k == "--phase-every") phase.every = std::max(1, std::atoi(v.c_str()));
        else if (k == "--phase-x" || k == "--phase-y") {
            if (!parse_phase_side(v, k == "--phase-x" ? &phase.x : &phase.y)) {
                std::fprintf(stderr, "%s takes NAME,LO,HI,CELLS[,log], not %s\n", k.c_str(), v.c_str());
                return 2;
            }
        }
        else if (k == "--phase-weight") phase.weight = v;
        else if (k == "--phase-axis") {
            if (std::sscanf(v.c_str(), "%lf,%lf,%lf", &phase.axis[0], &phase.axis[1], &phase.axis[2]) != 3) {
                std::fprintf(stderr, "--phase-axis takes X,Y,Z, not %s\n", v.c_str());
                return 2;
            }
        }
        else if (k == "--phase-center") {
            phase.center.assign(3, 0.0);
            if (v == "com") phase.center.clear();
            else if (std::sscanf(v.c_str(), "%lf,%lf,%lf", &phase.center[0], &phase.center[1], &phase.center[2]) != 3) {
                std::fprintf(stderr, "--phase-center takes com or X,Y,Z, not %s\n", v.c_str());
                return 2;
            }
        }
        else if (k == "--shells") shells.every = std::atoi(v.c_str());
        else if (k == "--shells-range") {
            if (std::sscanf(v.c_str(), "%lf,%lf", &shells.rmin, &shells.rmax) != 2) {
                std::fprintf(stderr, "--shells-range takes RMIN,RMAX, not %s\n", v.c_str());
                return 2;
            }
            shells.have_range = true;
        }
        else if (k == "--shells-bins") shells.bins = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--shells-l") shells.lmax = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--shells-log") shells.log = std::atoi(v.c_str()) != 0;
        else if (k == "--shells-rates") shells.rates = std::atoi(v.c_str()) != 0;
        else if (k == "--shells-axis") {
            if (std::sscanf(v.c_str(), "%lf,%lf,%lf", &shells.axis[0], &shells.axis[1], &shells.axis[2]) != 3) {
                std::fprintf(stderr, "--shells-axis takes X,Y,Z, not %s\n", v.c_str());
                return 2;
            }
        }
        else if (k == "--shells-center") {
            shells.center.assign(3, 0.0);
            if (v == "com") shells.center.clear();
            else if (std::sscanf(v.c_str(), "%lf,%lf,%lf", &shells.center[0], &shells.center[1], &shells.center[2]) != 3) {
                std::fprintf(stderr, "--shells-center takes com or X,Y,Z, not %s\n", v.c_str());
                return 2;
            }
        }
        else if (k == "--modes") modes.every = std::atoi(v.c_str());
        else if (k == "--modes-range") {
            if (std::sscanf(v.c_str(), "%lf,%lf", &modes.rmin, &modes.rmax) != 2) {
                std::fprintf(stderr, "--modes-range takes RMIN,RMAX, not %s\n", v.c_str());
                return 2;
            }
            modes.have_range = true;
        }
        else if (k == "--modes-bins") modes.bins = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--modes-m") modes.mmax = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--modes-log") modes.log = std::atoi(v.c_str()) != 0;
        else if (k == "--modes-axis") {
            if (std::sscanf(v.c_str(), "%lf,%lf,%lf", &modes.axis[0], &modes.axis[1], &modes.axis[2]) != 3) {
                std::fprintf(stderr, "--modes-axis takes X,Y,Z, not %s\n", v.c_str());
                return 2;
            }
        }
        else if (k == "--modes-center") {
            modes.center.assign(3, 0.0);
            if (v == "com") modes.center.clear();
            else if (std::sscanf(v.c_str(), "%lf,%lf,%lf", &modes.center[0], &modes.center[1], &modes.center[2]) != 3) {
                std::fprintf(stderr, "--modes-center takes com or X,Y,Z, not %s\n", v.c_str());
                return 2;
            }
        }
        else if (k == "--smaps") smaps.dir = v;
        else if (k == "--smap-every") smaps.every = std::max(1, std::atoi(v.c_str()));
        else if (k == "--smap-size") {
            if (std::sscanf(v.c_str(), "%ux%u", &smaps.params.width, &smaps.params.height) != 2) {
                std::fprintf(stderr, "--smap-size takes WxH, not %s\n", v.c_str());
                return 2;
            }
            smaps.have_size = true;
        }
        else if (k == "--smap-extent") {
            nbody::SmoothParams &mp = smaps.params;
            if (std::sscanf(v.c_str(), "%lf,%lf,%lf,%lf", &mp.x_range[0], &mp.x_range[1], &mp.y_range[0], &mp.y_range[1]) != 4) {
                std::fprintf(stderr, "--smap-extent takes X0,X1,Y0,Y1, not %s\n", v.c_str());
                return 2;
            }
            smaps.have_extent = true;
        }
        else if (k == "--smap-axis") {
            double *a = smaps.params.axis;
            if (std::sscanf(v.c_str(), "%lf,%lf,%lf", &a[0], &a[1], &a[2]) != 3) {
                std::fprintf(stderr, "--smap-axis takes X,Y,Z, not %s\n", v.c_str());
                return 2;
            }
        }
        else if (k == "--smap-center") {
            double *c = smaps.params.center;
            if (v == "com") smaps.params.flags |= NB_SMOOTH_CENTER_COM;
            else if (std::sscanf(v.c_str(), "%lf,%lf,%lf", &c[0], &c[1], &c[2]) == 3)
                smaps.params.flags &= ~NB_SMOOTH_CENTER_COM;
            else {
                std::fprintf(stderr, "--smap-center takes com or X,Y,Z, not %s\n", v.c_str());
                return 2;
            }
        }
        else if (k == "--smap-depth") {
            if (std::sscanf(v.c_str(), "%lf,%lf", &smaps.params.depth_range[0], &smaps.params.depth_range[1]) != 2) {
                std::fprintf(stderr, "--smap-depth takes LO,HI, not %s\n", v.c_str());
                return 2;
            }
        }
        else if (k == "--smap-k") smaps.k = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--smap-max") smaps.max_pixels = std::atof(v.c_str());
        else if (k == "--hop") hop.every = std::atoi(v.c_str());
        else if (k == "--hop-k") {
            unsigned a = 0, b = 0, c = 0;
            if (std::sscanf(v.c_str(), "%u,%u,%u", &a, &b, &c) != 3) {
                std::fprintf(stderr, "--hop-k needs DENS,HOP,MERGE\n");
                return 2;
            }
            hop.params.k_density = a;
            hop.params.k_hop = b;
            hop.params.k_merge = c;
        } else if (k == "--hop-min") hop.params.min_members = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--hop-density-min") hop.params.density_min = std::atof(v.c_str());
        else if (k == "--hop-saddle") {
            hop.saddle = std::atof(v.c_str());
            hop_saddle = true;
        } else if (k == "--hop-peak") {
            hop.peak = std::atof(v.c_str());
            hop_peak = true;
        } else if (k == "--hop-top") hop.top = std::atoi(v.c_str());
        else if (k == "--mst") mst.every = std::atoi(v.c_str());
        else if (k == "--mst-links") {
            for (const char *c = v.c_str(); *c;) {
                char *end = nullptr;
                const double link = std::strtod(c, &end);
                if (end == c || !(link > 0.0) || !std::isfinite(link) || !(link * link > 0.0) ||
                    !std::isfinite(link * link) || (*end && *end != ',') || (*end == ',' && !end[1])) {
                    std::fprintf(stderr, "--mst-links takes L1,L2,... (each finite and > 0), not %s\n", v.c_str());
                    return 2;
                }
                mst.links.push_back(link);
                c = *end ? end + 1 : end;
            }
        }
        else if (k == "--mst-min") {
            char *end = nullptr;
            const unsigned long mm = std::strtoul(v.c_str(), &end, 10);
            if (end == v.c_str() || *end || mm < 1 || mm > 0xfffffffful) {
                std::fprintf(stderr, "--mst-min takes a count of at least 1, not %s\n", v.c_str());
                return 2;
            }
            mst.min_members = (uint32_t)mm;
            mst.have_min = true;
        }
        else if (k == "--mst-dump") mst.dir = v;
        else if (k == "--knn") knn.every = std::atoi(v.c_str());
        else if (k == "--knn-k") knn.k = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--orbits") orbits.dir = v;
        else if (k == "--orbits-at") orbits.at = std::atoi(v.c_str());
        else if (k == "--orbits-bins") orbits.bins = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--orbits-steps") orbits.steps = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--orbits-every") orbits.every = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--orbits-dt") orbits.dt = std::atof(v.c_str());
        else if (k == "--orbits-omega") orbits.omega = std::atof(v.c_str());
        else if (k == "--orbits-speed") orbits.speed = std::atof(v.c_str());
        else if (k == "--orbits-range") {
            if (std::sscanf(v.c_str(), "%lf,%lf", &orbits.rmin, &orbits.rmax) != 2) {
                std::fprintf(stderr, "--orbits-range takes RMIN,RMAX, not %s\n", v.c_str());
                return 2;
            }
            orbits.have_range = true;
        }
        else if (k == "--orbits-axis" || k == "--orbits-center") {
            double *a = k == "--orbits-axis" ? orbits.axis.data() : orbits.center.data();
            if (std::sscanf(v.c_str(), "%lf,%lf,%lf", a, a + 1, a + 2) != 3) {
                std::fprintf(stderr, "%s takes X,Y,Z, not %s\n", k.c_str(), v.c_str());
                return 2;
            }
        }
        else if (k == "--sections") sections.launch.dir = v;
        else if (k == "--sections-at") sections.launch.at = std::atoi(v.c_str());
        else if (k == "--sections-bins") sections.launch.bins = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--sections-steps") sections.launch.steps = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--sections-dt") sections.launch.dt = std::atof(v.c_str());
        else if (k == "--sections-omega") sections.launch.omega = std::atof(v.c_str());
        else if (k == "--sections-speed") sections.launch.speed = std::atof(v.c_str());
        else if (k == "--sections-offset") sections.offset = std::atof(v.c_str());
        else if (k == "--sections-direction") sections.direction = std::atoi(v.c_str());
        else if (k == "--sections-max") sections.max_crossings = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--sections-range") {
            if (std::sscanf(v.c_str(), "%lf,%lf", &sections.launch.rmin, &sections.launch.rmax) != 2) {
                std::fprintf(stderr, "--sections-range takes RMIN,RMAX, not %s\n", v.c_str());
                return 2;
            }
            sections.launch.have_range = true;
        }
        else if (k == "--sections-axis" || k == "--sections-center" || k == "--sections-normal") {
            double *a = k == "--sections-axis"     ? sections.launch.axis.data()
                        : k == "--sections-center" ? sections.launch.center.data()
                                                   : sections.normal.data();
            if (std::sscanf(v.c_str(), "%lf,%lf,%lf", a, a + 1, a + 2) != 3) {
                std::fprintf(stderr, "%s takes three numbers X,Y,Z, not %s\n", k.c_str(), v.c_str());
                return 2;
            }
        }
        else if (k == "--stability") stability.dir = v;
        else if (k == "--stability-at") stability.at = std::atoi(v.c_str());
        else if (k == "--stability-bins") stability.bins = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--stability-steps") stability.steps = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--stability-dt") stability.dt = std::atof(v.c_str());
        else if (k == "--stability-omega") stability.omega = std::atof(v.c_str());
        else if (k == "--stability-speed") stability.speed = std::atof(v.c_str());
        else if (k == "--stability-range") {
            if (std::sscanf(v.c_str(), "%lf,%lf", &stability.rmin, &stability.rmax) != 2) {
                std::fprintf(stderr, "--stability-range takes RMIN,RMAX, not %s\n", v.c_str());
                return 2;
            }
            stability.have_range = true;
        }
        else if (k == "--stability-axis" || k == "--stability-center") {
            double *a = k == "--stability-axis" ? stability.axis.data() : stability.center.data();
            if (std::sscanf(v.c_str(), "%lf,%lf,%lf", a, a + 1, a + 2) != 3) {
                std::fprintf(stderr, "%s takes X,Y,Z, not %s\n", k.c_str(), v.c_str());
                return 2;
            }
        }
        else if (k == "--kin") kin.every = std::atoi(v.c_str());
        else if (k == "--kin-k") kin.k = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--kin-gradient") kin.gradient = std::atoi(v.c_str()) != 0;
        else if (k == "--halo") halo.every = std::atoi(v.c_str());
        else if (k == "--halo-link") halo.link = std::atof(v.c_str());
        else if (k == "--halo-range") {
            if (std::sscanf(v.c_str(), "%lf,%lf", &halo.rmin, &halo.rmax) != 2) {
                std::fprintf(stderr, "--halo-range takes RMIN,RMAX, not %s\n", v.c_str());
                return 2;
            }
            halo.have_range = true;
        }
        else if (k == "--halo-bins") halo.bins = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--halo-min") halo.min_members = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (k == "--halo-top") halo.top = std::atoi(v.c_str());
        else if (k == "--halo-rho") halo.rho = std::atof(v.c_str());
        else if (k == "--devices") {
            for (size_t a = 0; a <= v.size();) {
                const size_t b = std::min(v.find(',', a), v.size());
                devices.push_back(std::atoi(v.substr(a, b - a).c_str()));
                a = b + 1;
            }
        }
        else { std::fprintf(stderr, "unknown option %s\n", k.c_str()); return 2; }
    }
    if (radial.every > 0 && !radial.have_range) {
        std::fprintf(stderr, "--radial needs --radial-range RMIN,RMAX\n");
        return 2;
    }
    if (freq.every > 0 && !freq.have_range) {
        std::fprintf(stderr, "--freq needs --freq-range RMIN,RMAX\n");
        return 2;
    }
    if (!orbits.dir.empty() && (!orbits.have_range || orbits.steps == 0 || orbits.dt == 0.0 || orbits.at < 0)) {
        std::fprintf(stderr, "--orbits needs --orbits-range RMIN,RMAX, --orbits-dt DT and --orbits-steps S\n");
        return 2;
    }
    if (!sections.launch.dir.empty() && (!sections.launch.have_range || sections.launch.steps == 0 ||
                                         sections.launch.dt == 0.0 || sections.launch.at < 0)) {
        std::fprintf(stderr, "--sections needs --sections-range RMIN,RMAX, --sections-dt DT and --sections-steps S\n");
        return 2;
    }
    if (!stability.dir.empty() && (!stability.have_range || stability.steps == 0 || stability.dt == 0.0 ||
                                   stability.at < 0)) {
        std::fprintf(stderr, "--stability needs --stability-range RMIN,RMAX, --stability-dt DT and --stability-steps S\n");
        return 2;
    }
    if (rotcurve.every > 0 && !rotcurve.have_range) {
        std::fprintf(stderr, "--rotcurve needs --rotcurve-range RMIN,RMAX\n");
        return 2;
    }
    if (!maps.dir.empty() && !(maps.have_size && maps.have_extent)) {
        std::fprintf(stderr, "--maps needs --map-size WxH and --map-extent X0,X1,Y0,Y1\n");
        return 2;
    }
    if (!smaps.dir.empty()) {
        nbody::SmoothParams &mp = smaps.params;
        if (!(smaps.have_size && smaps.have_extent) || mp.width == 0 || mp.height == 0) {
            std::fprintf(stderr, "--smaps needs --smap-size WxH and --smap-extent X0,X1,Y0,Y1\n");
            return 2;
        }
        if (!(smaps.max_pixels >= 2.0)) {
            std::fprintf(stderr, "--smap-max takes at least 2 pixels, not %g\n", smaps.max_pixels);
            return 2;
        }
        // the floor of two pixels and the cap, in the larger side of a pixel (nbody::smooth_params)
        const double pixel = std::max(std::fabs(mp.x_range[1] - mp.x_range[0]) / mp.width,
                                      std::fabs(mp.y_range[1] - mp.y_range[0]) / mp.height);
        mp.s_min = 2.0 * pixel;
        mp.s_max = smaps.max_pixels * pixel;
    }
    if (hop_saddle != hop_peak) {
        std::fprintf(stderr, "--hop-saddle and --hop-peak go together\n");
        return 2;
    }
    hop.regroup = hop_saddle;
    if (fof6.every > 0 && (!(fof6.link > 0.0) || !(fof6.vlink > 0.0))) {
        std::fprintf(stderr, "--fof6 needs --fof6-link B > 0 and --fof6-vlink V > 0\n");
        return 2;
    }
    if (fof.every > 0 && !(fof.link > 0.0)) {
        std::fprintf(stderr, "--fof needs --fof-link B > 0\n");
        return 2;
    }
    if (bound.every > 0 && !(bound.link > 0.0)) {
        std::fprintf(stderr, "--bound needs --bound-link B > 0\n");
        return 2;
    }
    if (shapes.every > 0 && !(shapes.link > 0.0)) {
        std::fprintf(stderr, "--shapes needs --shapes-link B > 0\n");
        return 2;
    }
    if (shapes.every > 0 && shapes.reduced && !(shapes.k_rms > 0.0)) {
        std::fprintf(stderr, "--shapes-reduced 1 needs --shapes-radius KRMS > 0\n");
        return 2;
    }
    if (!phase.dir.empty() && (phase.x.cells == 0 || phase.y.cells == 0)) {
        std::fprintf(stderr, "--phase needs --phase-x and --phase-y NAME,LO,HI,CELLS[,log]\n");
        return 2;
    }
    if (modes.every > 0 && (!modes.have_range || modes.mmax < 2)) {
        std::fprintf(stderr, "--modes needs --modes-range RMIN,RMAX and --modes-m M >= 2\n");
        return 2;
    }
    if (mst.every <= 0 && (!mst.links.empty() || !mst.dir.empty() || mst.have_min)) {
        std::fprintf(stderr, "--mst-links, --mst-min and --mst-dump need --mst K\n");
        return 2;
    }
    if (shells.every > 0 && (!shells.have_range || shells.lmax < 2)) {
        std::fprintf(stderr, "--shells needs --shells-range RMIN,RMAX and --shells-l L >= 2\n");
        return 2;
    }
    if (radii.every > 0 && !(radii.link > 0.0)) {
        std::fprintf(stderr, "--radii needs --radii-link B > 0\n");
        return 2;
    }
    if (halo.every > 0 && (!(halo.link > 0.0) || !halo.have_range)) {
        std::fprintf(stderr, "--halo needs --halo-link B > 0 and --halo-range RMIN,RMAX\n");
        return 2;
    }
    const nbody::InitFn fn = init == "disc" ? nbody::inits::disc_init(seed)
                           : init == "spherical" ? nbody::inits::spherical_init(seed)
                                                 : nbody::inits::uniform_init(seed);
    try {
        if (sim == "naive")
            return run<nbody::NaiveSim>(sp, nbody::AddParams::NaiveSimParams(), fn, steps, device, devices, dump, -1, diag,
                                        diag_potential, frames, radial, rotcurve, maps, smaps, fof, knn, bound, halo, hop, shapes, lagr, radii, modes, phase, freq, kin, orbits, fof6, sections, stability, shells, mst);
        return run<nbody::TreeSim>(sp, nbody::AddParams::TreeSimParams(theta), fn, steps, device, devices, dump, let,
                                       diag, diag_potential, frames, radial, rotcurve, maps, smaps, fof, knn, bound, halo, hop, shapes, lagr, radii, modes, phase, freq, kin, orbits, fof6, sections, stability, shells, mst);
    } catch (const nbody::Error &e) {
        std::fprintf(stderr, "error %d: %s\n", e.code(), e.what());
        return 1;
    }
}
