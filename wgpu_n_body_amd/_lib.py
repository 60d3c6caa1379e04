"""ctypes declarations for libnbody_hip.so (include/nbody.h).  Fails loudly if the HIP
library is missing: there is no CPU fallback in the product."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
# NB_LIB: an alternative build of the same library (kernel tuning experiments); default in-tree
LIB_PATH = os.environ.get("NB_LIB") or os.path.join(_PKG, "libnbody_hip.so")

# `struct Particle`, src/sims/mod.rs:9-16 -- 40 bytes
PARTICLE_DTYPE = np.dtype(
    [("position", "<f4", (3,)), ("velocity", "<f4", (3,)), ("acceleration", "<f4", (3,)),
     ("mass", "<f4")]
)
assert PARTICLE_DTYPE.itemsize == 40
# `struct Octant`, src/sims/tree.rs:605-622 -- 52 bytes
OCTANT_DTYPE = np.dtype(
    [("cog", "<f4", (3,)), ("mass", "<f4"), ("bodies", "<u4"), ("children", "<u4", (8,))]
)
assert OCTANT_DTYPE.itemsize == 52


class nb_sim_params(C.Structure):
    _fields_ = [("particle_num", C.c_uint32), ("g", C.c_float), ("e", C.c_float),
                ("dt", C.c_float)]


class nb_add_params(C.Structure):
    _fields_ = [("kind", C.c_int32), ("theta", C.c_float)]


class nb_placement(C.Structure):
    _fields_ = [("device_id", C.c_int32), ("rank", C.c_int32), ("world", C.c_int32),
                ("stream", C.c_void_p), ("posm", C.c_void_p * 2)]


class nb_diagnostics(C.Structure):
    _fields_ = [("step_num", C.c_uint64), ("n", C.c_uint64), ("nonfinite", C.c_uint64),
                ("mass", C.c_double), ("com", C.c_double * 3), ("momentum", C.c_double * 3),
                ("angular_momentum", C.c_double * 3), ("kinetic", C.c_double), ("max_speed", C.c_double),
                ("pair_sum", C.c_double), ("potential", C.c_double), ("total", C.c_double),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class nb_camera(C.Structure):
    _fields_ = [("eye", C.c_float * 3), ("target", C.c_float * 3), ("up", C.c_float * 3),
                ("aspect", C.c_float), ("fovy_deg", C.c_float), ("znear", C.c_float), ("zfar", C.c_float)]


class nb_render_params(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("view_proj", C.c_float * 16),
                ("half_size", C.c_float), ("clear", C.c_float * 3), ("alpha", C.c_float),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class nb_render_stats(C.Structure):
    _fields_ = [("step_num", C.c_uint64), ("n", C.c_uint64), ("drawn", C.c_uint64), ("clipped", C.c_uint64),
                ("oversize", C.c_uint64), ("nonfinite", C.c_uint64), ("fragments", C.c_uint64),
                ("max_count", C.c_uint32), ("reserved", C.c_uint32)]


class nb_radial_params(C.Structure):
    _fields_ = [("nbins", C.c_uint32), ("flags", C.c_uint32), ("center", C.c_double * 3),
                ("velocity", C.c_double * 3), ("axis", C.c_double * 3), ("edges", C.POINTER(C.c_double))]


class nb_radial_bin(C.Structure):
    _fields_ = [("count", C.c_uint64), ("mass", C.c_double), ("m_r", C.c_double), ("m_ur", C.c_double),
                ("m_ur2", C.c_double), ("m_uphi", C.c_double), ("m_uphi2", C.c_double), ("m_u2", C.c_double),
                ("ang", C.c_double * 3)]


class nb_radial_profile(C.Structure):
    _fields_ = [("step_num", C.c_uint64), ("n", C.c_uint64), ("nonfinite", C.c_uint64),
                ("inside_count", C.c_uint64), ("outside_count", C.c_uint64),
                ("inside_mass", C.c_double), ("outside_mass", C.c_double), ("mass", C.c_double),
                ("center", C.c_double * 3), ("velocity", C.c_double * 3), ("axis", C.c_double * 3),
                ("shape", C.c_double * 6), ("nbins", C.c_uint32), ("flags", C.c_uint32)]


class nb_field_sample(C.Structure):
    _fields_ = [("acc", C.c_double * 3), ("potential", C.c_double), ("coincident", C.c_uint32),
                ("reserved", C.c_uint32)]


class nb_field_stats(C.Structure):
    _fields_ = [("step_num", C.c_uint64), ("n", C.c_uint64), ("nonfinite", C.c_uint64), ("points", C.c_uint64),
                ("nonfinite_points", C.c_uint64), ("flags", C.c_uint32), ("launches", C.c_uint32)]


class nb_field_ring(C.Structure):
    _fields_ = [("a_R", C.c_double), ("a_n", C.c_double), ("potential", C.c_double), ("v_c", C.c_double)]


class nb_tidal_sample(C.Structure):
    _fields_ = [("tensor", C.c_double * 6), ("coincident", C.c_uint32), ("reserved", C.c_uint32)]


nb_tidal_stats = nb_field_stats  # (the header's typedef)


class nb_tidal_ring(C.Structure):
    _fields_ = [("t_RR", C.c_double), ("t_pp", C.c_double), ("t_nn", C.c_double), ("t_Rn", C.c_double),
                ("omega2", C.c_double), ("kappa2", C.c_double), ("nu2", C.c_double)]


class nb_orbit_params(C.Structure):
    _fields_ = [("dt", C.c_double), ("step0", C.c_uint64), ("steps", C.c_uint32), ("every", C.c_uint32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32), ("accel_scale", C.c_double), ("omega", C.c_double),
                ("axis", C.c_double * 3), ("center", C.c_double * 3)]


class nb_orbit_sample(C.Structure):
    _fields_ = [("pos", C.c_double * 3), ("vel", C.c_double * 3), ("potential", C.c_double), ("energy", C.c_double)]


class nb_orbit_stats(C.Structure):
    _fields_ = [("step_num", C.c_uint64), ("n", C.c_uint64), ("nonfinite", C.c_uint64), ("tracers", C.c_uint64),
                ("nonfinite_tracers", C.c_uint64), ("records", C.c_uint32), ("pair_launches", C.c_uint32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class nb_orbit_section_params(C.Structure):
    _fields_ = [("normal", C.c_double * 3), ("offset", C.c_double), ("direction", C.c_int32),
                ("max_crossings", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class nb_orbit_crossing(C.Structure):
    _fields_ = [("xi", C.c_double * 3), ("eta", C.c_double * 3), ("time", C.c_double), ("step", C.c_uint64)]


class nb_orbit_summary(C.Structure):
    _fields_ = [("r2_min", C.c_double), ("r2_max", C.c_double), ("R2_min", C.c_double), ("R2_max", C.c_double),
                ("h_max", C.c_double), ("lz_min", C.c_double), ("lz_max", C.c_double),
                ("first_peri", C.c_uint64), ("last_peri", C.c_uint64),
                ("pericentres", C.c_uint32), ("apocentres", C.c_uint32), ("plane_ups", C.c_uint32),
                ("winding_pattern", C.c_int32), ("winding_inertial", C.c_int32), ("reserved", C.c_uint32)]


class nb_orbit_section_stats(C.Structure):
    _fields_ = [("orbit", nb_orbit_stats), ("crossings", C.c_uint64), ("stored", C.c_uint64),
                ("overflowed", C.c_uint64)]


class nb_orbit_stability_params(C.Structure):
    _fields_ = [("deviations", C.c_uint32), ("renorm_log2", C.c_uint32), ("reserved", C.c_uint32)]


class nb_orbit_deviation(C.Structure):
    _fields_ = [("d", C.c_double * 6), ("log2", C.c_int64)]


class nb_orbit_growth(C.Structure):
    _fields_ = [("peak_log2", C.c_int64), ("peak_step", C.c_uint64), ("renorms", C.c_uint32),
                ("reserved", C.c_uint32)]


class nb_orbit_stability_stats(C.Structure):
    _fields_ = [("orbit", nb_orbit_stats), ("renorms", C.c_uint64), ("deviations", C.c_uint32),
                ("renorm_log2", C.c_uint32)]


class nb_map_params(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("center", C.c_double * 3), ("velocity", C.c_double * 3), ("axis", C.c_double * 3),
                ("x_range", C.c_double * 2), ("y_range", C.c_double * 2), ("depth_range", C.c_double * 2)]


class nb_map_stats(C.Structure):
    _fields_ = [("step_num", C.c_uint64), ("n", C.c_uint64), ("nonfinite", C.c_uint64),
                ("binned_count", C.c_uint64), ("outside_count", C.c_uint64),
                ("binned_mass", C.c_double), ("outside_mass", C.c_double), ("mass", C.c_double),
                ("center", C.c_double * 3), ("velocity", C.c_double * 3),
                ("n_hat", C.c_double * 3), ("e1", C.c_double * 3), ("e2", C.c_double * 3),
                ("width", C.c_uint32), ("height", C.c_uint32), ("flags", C.c_uint32), ("max_count", C.c_uint32)]


class nb_phase_params(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("x", C.c_uint32), ("y", C.c_uint32), ("q", C.c_uint32), ("reserved2", C.c_uint32),
                ("center", C.c_double * 3), ("velocity", C.c_double * 3), ("axis", C.c_double * 3),
                ("x_edges", C.POINTER(C.c_double)), ("y_edges", C.POINTER(C.c_double)),
                ("values", C.POINTER(C.c_double)), ("step_num", C.c_uint64)]


class nb_phase_stats(C.Structure):
    _fields_ = [("step_num", C.c_uint64), ("n", C.c_uint64), ("nonfinite", C.c_uint64),
                ("binned_count", C.c_uint64), ("outside_count", C.c_uint64), ("undefined_count", C.c_uint64),
                ("binned_mass", C.c_double), ("outside_mass", C.c_double), ("mass", C.c_double),
                ("center", C.c_double * 3), ("velocity", C.c_double * 3),
                ("n_hat", C.c_double * 3), ("e1", C.c_double * 3), ("e2", C.c_double * 3),
                ("width", C.c_uint32), ("height", C.c_uint32), ("flags", C.c_uint32), ("max_count", C.c_uint32),
                ("x", C.c_uint32), ("y", C.c_uint32), ("q", C.c_uint32), ("reserved", C.c_uint32)]


class nb_fof_params(C.Structure):
    _fields_ = [("link", C.c_double), ("min_members", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint64)]


class nb_fof6_params(C.Structure):
    _fields_ = [("link", C.c_double), ("vlink", C.c_double), ("min_members", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint64)]


class nb_fof_group(C.Structure):
    _fields_ = [("label", C.c_uint32), ("count", C.c_uint32), ("mass", C.c_double), ("mx", C.c_double * 3),
                ("mv", C.c_double * 3), ("mr2", C.c_double), ("mv2", C.c_double)]


class nb_fof_stats(C.Structure):
    _fields_ = [("step_num", C.c_uint64), ("n", C.c_uint64), ("nonfinite", C.c_uint64),
                ("components", C.c_uint64), ("groups", C.c_uint64), ("grouped_bodies", C.c_uint64),
                ("largest_count", C.c_uint32), ("largest_label", C.c_uint32), ("cells", C.c_uint32 * 3),
                ("reserved", C.c_uint32), ("cell_side", C.c_double)]


class nb_bound_params(C.Structure):
    _fields_ = [("link", C.c_double), ("min_members", C.c_uint32), ("min_bound", C.c_uint32),
                ("max_iter", C.c_uint32), ("max_group", C.c_uint32), ("flags", C.c_uint32),
                ("reserved32", C.c_uint32), ("reserved", C.c_uint64)]


class nb_bound_group(C.Structure):
    _fields_ = [("label", C.c_uint32), ("count", C.c_uint32), ("bound_count", C.c_uint32),
                ("iterations", C.c_uint32), ("status", C.c_uint32), ("most_bound", C.c_uint32),
                ("mass", C.c_double), ("mx", C.c_double * 3), ("mv", C.c_double * 3), ("mr2", C.c_double),
                ("kinetic", C.c_double), ("potential", C.c_double), ("phi_min", C.c_double),
                ("kinetic0", C.c_double), ("potential0", C.c_double)]


class nb_bound_stats(C.Structure):
    _fields_ = [("step_num", C.c_uint64), ("n", C.c_uint64), ("nonfinite", C.c_uint64),
                ("components", C.c_uint64), ("groups", C.c_uint64), ("grouped_bodies", C.c_uint64),
                ("largest_count", C.c_uint32), ("largest_label", C.c_uint32),
                ("bound_groups", C.c_uint64), ("bound_bodies", C.c_uint64), ("dissolved", C.c_uint64),
                ("unconverged", C.c_uint64), ("skipped", C.c_uint64), ("pairs", C.c_uint64),
                ("rounds_max", C.c_uint32), ("reserved", C.c_uint32)]


class nb_knn_params(C.Structure):
    _fields_ = [("k", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint64)]


class nb_knn_stats(C.Structure):
    _fields_ = [("step_num", C.c_uint64), ("n", C.c_uint64), ("nonfinite", C.c_uint64), ("counted", C.c_uint64),
                ("degenerate", C.c_uint64), ("short_of_k", C.c_uint64),
                ("sum_rho", C.c_double), ("sum_rho_x", C.c_double * 3), ("sum_rho_v", C.c_double * 3),
                ("sum_rho2", C.c_double), ("peak_density", C.c_double),
                ("peak_index", C.c_uint32), ("reserved", C.c_uint32)]


class nb_mst_params(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("reserved32", C.c_uint32), ("reserved", C.c_uint64)]


class nb_mst_stats(C.Structure):
    _fields_ = [("step_num", C.c_uint64), ("n", C.c_uint64), ("nonfinite", C.c_uint64), ("edges", C.c_uint64),
                ("rounds", C.c_uint32), ("reserved", C.c_uint32), ("components_after", C.c_uint32 * 32),
                ("d2_min", C.c_double), ("d2_max", C.c_double), ("lo", C.c_double * 3), ("hi", C.c_double * 3),
                ("h", C.c_double)]


class nb_kin_params(C.Structure):
    _fields_ = [("k", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint64)]


class nb_kin_stats(C.Structure):
    _fields_ = [("step_num", C.c_uint64), ("n", C.c_uint64), ("nonfinite", C.c_uint64), ("counted", C.c_uint64),
                ("degenerate", C.c_uint64), ("short_of_k", C.c_uint64), ("k", C.c_uint32), ("flags", C.c_uint32)]


class nb_hop_params(C.Structure):
    _fields_ = [("k_density", C.c_uint32), ("k_hop", C.c_uint32), ("k_merge", C.c_uint32),
                ("min_members", C.c_uint32), ("density_min", C.c_double), ("flags", C.c_uint32),
                ("reserved32", C.c_uint32), ("reserved", C.c_uint64)]


class nb_hop_boundary(C.Structure):
    _fields_ = [("a", C.c_uint32), ("b", C.c_uint32), ("pairs", C.c_uint32), ("reserved", C.c_uint32),
                ("density", C.c_double)]


class nb_hop_stats(C.Structure):
    _fields_ = [("step_num", C.c_uint64), ("n", C.c_uint64), ("nonfinite", C.c_uint64), ("counted", C.c_uint64),
                ("outside", C.c_uint64), ("short_of_k", C.c_uint64), ("peaks", C.c_uint64), ("groups", C.c_uint64),
                ("grouped_bodies", C.c_uint64), ("boundaries", C.c_uint64), ("boundary_pairs", C.c_uint64),
                ("largest_count", C.c_uint32), ("largest_label", C.c_uint32)]


class nb_hop_regroup_params(C.Structure):
    _fields_ = [("saddle", C.c_double), ("peak", C.c_double), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class nb_halo_params(C.Structure):
    _fields_ = [("nbins", C.c_uint32), ("flags", C.c_uint32), ("m", C.c_uint64), ("edges", C.POINTER(C.c_double)),
                ("centers", C.POINTER(C.c_double)), ("bodies", C.POINTER(C.c_uint32)),
                ("velocities", C.POINTER(C.c_double))]


class nb_halo_head(C.Structure):
    _fields_ = [("inside_count", C.c_uint32), ("flags", C.c_uint32), ("inside_mass", C.c_double),
                ("center", C.c_double * 3), ("velocity", C.c_double * 3)]


class nb_halo_stats(C.Structure):
    _fields_ = [("step_num", C.c_uint64), ("n", C.c_uint64), ("nonfinite", C.c_uint64), ("centers", C.c_uint64),
                ("tested", C.c_uint64), ("items", C.c_uint64), ("cells", C.c_uint32 * 3), ("reserved", C.c_uint32)]


class nb_shape_params(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("min_members", C.c_uint32), ("max_iter", C.c_uint32),
                ("reserved32", C.c_uint32), ("tol", C.c_double), ("step_num", C.c_uint64), ("reserved", C.c_uint64)]


class nb_shape_group(C.Structure):
    _fields_ = [("count", C.c_uint32), ("selected", C.c_uint32), ("iterations", C.c_uint32), ("status", C.c_uint32),
                ("radius", C.c_double), ("center", C.c_double * 3), ("velocity", C.c_double * 3),
                ("mass", C.c_double), ("md", C.c_double * 3), ("mu", C.c_double * 3), ("t", C.c_double * 6),
                ("uu", C.c_double * 6), ("j", C.c_double * 3), ("lambda", C.c_double * 3), ("axes", C.c_double * 9),
                ("q", C.c_double), ("s", C.c_double)]


class nb_shape_stats(C.Structure):
    _fields_ = [("step_num", C.c_uint64), ("n", C.c_uint64), ("rows", C.c_uint64), ("members", C.c_uint64),
                ("nonfinite_members", C.c_uint64), ("converged", C.c_uint64), ("unconverged", C.c_uint64),
                ("degenerate", C.c_uint64), ("empty", C.c_uint64), ("rounds_max", C.c_uint32),
                ("reserved", C.c_uint32)]


class nb_radii_params(C.Structure):
    _fields_ = [("nf", C.c_uint32), ("vmax_skip", C.c_uint32), ("step_num", C.c_uint64), ("reserved", C.c_uint64),
                ("fractions", C.c_double * 16)]


class nb_radii_group(C.Structure):
    _fields_ = [("count", C.c_uint32), ("vmax_index", C.c_uint32), ("center", C.c_double * 3), ("mass", C.c_double),
                ("r_min", C.c_double), ("r_max", C.c_double), ("vc2_max", C.c_double), ("r_vmax", C.c_double),
                ("radius", C.c_double * 16), ("index", C.c_uint32 * 16)]


class nb_radii_stats(C.Structure):
    _fields_ = [("step_num", C.c_uint64), ("n", C.c_uint64), ("rows", C.c_uint64), ("members", C.c_uint64),
                ("nonfinite_members", C.c_uint64), ("empty", C.c_uint64)]


class nb_modes_params(C.Structure):
    _fields_ = [("nbins", C.c_uint32), ("mmax", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("center", C.c_double * 3), ("velocity", C.c_double * 3), ("axis", C.c_double * 3),
                ("edges", C.POINTER(C.c_double))]


class nb_modes_head(C.Structure):
    _fields_ = [("step_num", C.c_uint64), ("n", C.c_uint64), ("nonfinite", C.c_uint64),
                ("inside_count", C.c_uint64), ("outside_count", C.c_uint64), ("inside_mass", C.c_double),
                ("outside_mass", C.c_double), ("mass", C.c_double), ("center", C.c_double * 3),
                ("velocity", C.c_double * 3), ("axis", C.c_double * 3), ("e1", C.c_double * 3),
                ("e2", C.c_double * 3), ("nbins", C.c_uint32), ("mmax", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


class nb_shell_params(C.Structure):
    _fields_ = [("nbins", C.c_uint32), ("lmax", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("center", C.c_double * 3), ("velocity", C.c_double * 3), ("axis", C.c_double * 3),
                ("edges", C.POINTER(C.c_double))]


class nb_shell_head(C.Structure):
    _fields_ = [("step_num", C.c_uint64), ("n", C.c_uint64), ("nonfinite", C.c_uint64),
                ("inside_count", C.c_uint64), ("outside_count", C.c_uint64), ("inside_mass", C.c_double),
                ("outside_mass", C.c_double), ("mass", C.c_double), ("center", C.c_double * 3),
                ("velocity", C.c_double * 3), ("axis", C.c_double * 3), ("e1", C.c_double * 3),
                ("e2", C.c_double * 3), ("nbins", C.c_uint32), ("lmax", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


class nb_smooth_params(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("center", C.c_double * 3), ("velocity", C.c_double * 3), ("axis", C.c_double * 3),
                ("x_range", C.c_double * 2), ("y_range", C.c_double * 2), ("depth_range", C.c_double * 2),
                ("s_min", C.c_double), ("s_max", C.c_double)]


class nb_smooth_stats(C.Structure):
    _fields_ = [("step_num", C.c_uint64), ("n", C.c_uint64), ("nonfinite", C.c_uint64),
                ("bad_smoothing", C.c_uint64), ("skipped", C.c_uint64), ("deposited", C.c_uint64),
                ("raised", C.c_uint64), ("lowered", C.c_uint64), ("pairs", C.c_uint64), ("tile_entries", C.c_uint64),
                ("mass", C.c_double), ("deposited_mass", C.c_double),
                ("center", C.c_double * 3), ("velocity", C.c_double * 3),
                ("n_hat", C.c_double * 3), ("e1", C.c_double * 3), ("e2", C.c_double * 3),
                ("s_min", C.c_double), ("s_max", C.c_double),
                ("width", C.c_uint32), ("height", C.c_uint32), ("flags", C.c_uint32), ("max_count", C.c_uint32)]


# nb_fof_group[] as a numpy record array
FOF_GROUP_DTYPE = np.dtype([("label", "<u4"), ("count", "<u4"), ("mass", "<f8"), ("mx", "<f8", (3,)),
                            ("mv", "<f8", (3,)), ("mr2", "<f8"), ("mv2", "<f8")])

# nb_hop_boundary[] as a numpy record array
HOP_BOUNDARY_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("pairs", "<u4"), ("reserved", "<u4"), ("density", "<f8")])

# nb_bound_group[] as a numpy record array
BOUND_GROUP_DTYPE = np.dtype([("label", "<u4"), ("count", "<u4"), ("bound_count", "<u4"), ("iterations", "<u4"),
                              ("status", "<u4"), ("most_bound", "<u4"), ("mass", "<f8"), ("mx", "<f8", (3,)),
                              ("mv", "<f8", (3,)), ("mr2", "<f8"), ("kinetic", "<f8"), ("potential", "<f8"),
                              ("phi_min", "<f8"), ("kinetic0", "<f8"), ("potential0", "<f8")])

# nb_field_sample[] and nb_field_ring[] as numpy record arrays
FIELD_SAMPLE_DTYPE = np.dtype([("acc", "<f8", (3,)), ("potential", "<f8"), ("coincident", "<u4"), ("reserved", "<u4")])
FIELD_RING_DTYPE = np.dtype([("a_R", "<f8"), ("a_n", "<f8"), ("potential", "<f8"), ("v_c", "<f8")])

# nb_tidal_sample[] and nb_tidal_ring[] as numpy record arrays
TIDAL_SAMPLE_DTYPE = np.dtype([("tensor", "<f8", (6,)), ("coincident", "<u4"), ("reserved", "<u4")])
TIDAL_RING_DTYPE = np.dtype([("t_RR", "<f8"), ("t_pp", "<f8"), ("t_nn", "<f8"), ("t_Rn", "<f8"), ("omega2", "<f8"),
                             ("kappa2", "<f8"), ("nu2", "<f8")])

# nb_orbit_sample[] as a numpy record array
ORBIT_SAMPLE_DTYPE = np.dtype([("pos", "<f8", (3,)), ("vel", "<f8", (3,)), ("potential", "<f8"), ("energy", "<f8")])

# nb_orbit_crossing[] and nb_orbit_summary[] as numpy record arrays
ORBIT_CROSSING_DTYPE = np.dtype([("xi", "<f8", (3,)), ("eta", "<f8", (3,)), ("time", "<f8"), ("step", "<u8")])
ORBIT_SUMMARY_DTYPE = np.dtype([("r2_min", "<f8"), ("r2_max", "<f8"), ("R2_min", "<f8"), ("R2_max", "<f8"),
                                ("h_max", "<f8"), ("lz_min", "<f8"), ("lz_max", "<f8"), ("first_peri", "<u8"),
                                ("last_peri", "<u8"), ("pericentres", "<u4"), ("apocentres", "<u4"),
                                ("plane_ups", "<u4"), ("winding_pattern", "<i4"), ("winding_inertial", "<i4"),
                                ("reserved", "<u4")])

# nb_orbit_deviation[] and nb_orbit_growth[] as numpy record arrays
ORBIT_DEVIATION_DTYPE = np.dtype([("d", "<f8", (6,)), ("log2", "<i8")])
ORBIT_GROWTH_DTYPE = np.dtype([("peak_log2", "<i8"), ("peak_step", "<u8"), ("renorms", "<u4"), ("reserved", "<u4")])

# nb_halo_head[] as a numpy record array
HALO_HEAD_DTYPE = np.dtype([("inside_count", "<u4"), ("flags", "<u4"), ("inside_mass", "<f8"),
                            ("center", "<f8", (3,)), ("velocity", "<f8", (3,))])

# nb_shape_group[] as a numpy record array
SHAPE_GROUP_DTYPE = np.dtype([("count", "<u4"), ("selected", "<u4"), ("iterations", "<u4"), ("status", "<u4"),
                              ("radius", "<f8"), ("center", "<f8", (3,)), ("velocity", "<f8", (3,)), ("mass", "<f8"),
                              ("md", "<f8", (3,)), ("mu", "<f8", (3,)), ("t", "<f8", (6,)), ("uu", "<f8", (6,)),
                              ("j", "<f8", (3,)), ("lambda", "<f8", (3,)), ("axes", "<f8", (9,)), ("q", "<f8"),
                              ("s", "<f8")])

# nb_radii_group[] as a numpy record array
RADII_GROUP_DTYPE = np.dtype([("count", "<u4"), ("vmax_index", "<u4"), ("center", "<f8", (3,)), ("mass", "<f8"),
                              ("r_min", "<f8"), ("r_max", "<f8"), ("vc2_max", "<f8"), ("r_vmax", "<f8"),
                              ("radius", "<f8", (16,)), ("index", "<u4", (16,))])

# nb_modes_bin[] and nb_modes_derived[] as numpy record arrays
MODES_BIN_DTYPE = np.dtype([("count", "<u8"), ("m_r", "<f8"), ("m_h2", "<f8")])
MODES_DERIVED_DTYPE = np.dtype([("amplitude", "<f8"), ("phase", "<f8"), ("pattern_speed", "<f8"),
                                ("bend_amplitude", "<f8"), ("bend_phase", "<f8")])

# nb_shell_bin[] and nb_shell_derived[] as numpy record arrays
SHELL_BIN_DTYPE = np.dtype([("count", "<u8"), ("m_r", "<f8"), ("m_ur", "<f8")])
SHELL_DERIVED_DTYPE = np.dtype([("power", "<f8", (7,)), ("relative", "<f8", (7,)), ("dipole", "<f8", (3,)),
                                ("quad_values", "<f8", (3,)), ("quad_axes", "<f8", (3, 3))])

# nb_kin_derived[] as a numpy record array
KIN_DERIVED_DTYPE = np.dtype([("mass", "<f8"), ("relative_velocity", "<f8", (3,)), ("mean_velocity", "<f8", (3,)),
                              ("dispersion", "<f8", (6,)), ("sigma2", "<f8"), ("sigma", "<f8"),
                              ("phase_space_density", "<f8"), ("gradient", "<f8", (9,)), ("det", "<f8"),
                              ("divergence", "<f8"), ("vorticity", "<f8", (3,)), ("shear", "<f8"),
                              ("status", "<u4"), ("reserved", "<u4")])

# nb_radial_bin[] as a numpy record array
RADIAL_BIN_DTYPE = np.dtype([("count", "<u8"), ("mass", "<f8"), ("m_r", "<f8"), ("m_ur", "<f8"), ("m_ur2", "<f8"),
                             ("m_uphi", "<f8"), ("m_uphi2", "<f8"), ("m_u2", "<f8"), ("ang", "<f8", (3,))])

assert C.sizeof(nb_sim_params) == 16 and C.sizeof(nb_add_params) == 8
assert C.sizeof(nb_diagnostics) == 152
assert C.sizeof(nb_radial_bin) == 88 == RADIAL_BIN_DTYPE.itemsize
assert C.sizeof(nb_radial_params) == 88 and C.sizeof(nb_radial_profile) == 192
assert C.sizeof(nb_field_sample) == 40 == FIELD_SAMPLE_DTYPE.itemsize and C.sizeof(nb_field_stats) == 48
assert C.sizeof(nb_field_ring) == 32 == FIELD_RING_DTYPE.itemsize
assert C.sizeof(nb_tidal_sample) == 56 == TIDAL_SAMPLE_DTYPE.itemsize
assert C.sizeof(nb_tidal_ring) == 56 == TIDAL_RING_DTYPE.itemsize
assert C.sizeof(nb_orbit_params) == 96 and C.sizeof(nb_orbit_stats) == 56
assert C.sizeof(nb_orbit_sample) == 64 == ORBIT_SAMPLE_DTYPE.itemsize
assert C.sizeof(nb_orbit_section_params) == 48 and C.sizeof(nb_orbit_section_stats) == 80
assert C.sizeof(nb_orbit_crossing) == 64 == ORBIT_CROSSING_DTYPE.itemsize
assert C.sizeof(nb_orbit_summary) == 96 == ORBIT_SUMMARY_DTYPE.itemsize
assert C.sizeof(nb_orbit_stability_params) == 12 and C.sizeof(nb_orbit_stability_stats) == 72
assert C.sizeof(nb_orbit_deviation) == 56 == ORBIT_DEVIATION_DTYPE.itemsize
assert C.sizeof(nb_orbit_growth) == 24 == ORBIT_GROWTH_DTYPE.itemsize
assert C.sizeof(nb_map_params) == 136 and C.sizeof(nb_map_stats) == 200
assert C.sizeof(nb_phase_params) == 136 and C.sizeof(nb_phase_stats) == 224
assert C.sizeof(nb_fof_params) == 24 and C.sizeof(nb_fof_stats) == 80
assert C.sizeof(nb_fof_group) == 80 == FOF_GROUP_DTYPE.itemsize and C.sizeof(nb_fof6_params) == 32
assert C.sizeof(nb_bound_params) == 40 and C.sizeof(nb_bound_stats) == 112
assert C.sizeof(nb_bound_group) == 128 == BOUND_GROUP_DTYPE.itemsize
assert C.sizeof(nb_knn_params) == 16 and C.sizeof(nb_knn_stats) == 128
assert C.sizeof(nb_mst_params) == 16 and C.sizeof(nb_mst_stats) == 240
assert C.sizeof(nb_kin_params) == 16 and C.sizeof(nb_kin_stats) == 56 and KIN_DERIVED_DTYPE.itemsize == 256
assert C.sizeof(nb_hop_params) == 40 and C.sizeof(nb_hop_stats) == 96 and C.sizeof(nb_hop_regroup_params) == 24
assert C.sizeof(nb_hop_boundary) == 24 == HOP_BOUNDARY_DTYPE.itemsize
assert C.sizeof(nb_halo_params) == 48 and C.sizeof(nb_halo_stats) == 64
assert C.sizeof(nb_halo_head) == 64 == HALO_HEAD_DTYPE.itemsize
assert C.sizeof(nb_shape_params) == 40 and C.sizeof(nb_shape_stats) == 80
assert C.sizeof(nb_shape_group) == 360 == SHAPE_GROUP_DTYPE.itemsize
assert C.sizeof(nb_radii_params) == 152 and C.sizeof(nb_radii_stats) == 48
assert C.sizeof(nb_radii_group) == 264 == RADII_GROUP_DTYPE.itemsize
assert C.sizeof(nb_modes_params) == 96 and C.sizeof(nb_modes_head) == 200
assert MODES_BIN_DTYPE.itemsize == 24 and MODES_DERIVED_DTYPE.itemsize == 40
assert C.sizeof(nb_shell_params) == 96 and C.sizeof(nb_shell_head) == 200
assert SHELL_BIN_DTYPE.itemsize == 24 and SHELL_DERIVED_DTYPE.itemsize == 232
assert C.sizeof(nb_smooth_params) == 152 and C.sizeof(nb_smooth_stats) == 248
assert C.sizeof(nb_camera) == 52 and C.sizeof(nb_render_params) == 100 and C.sizeof(nb_render_stats) == 64

NB_INIT_FN = C.CFUNCTYPE(None, C.POINTER(nb_sim_params), C.c_void_p, C.c_void_p)

NB_OK, NB_ERR_INVALID, NB_ERR_NO_DEVICE, NB_ERR_HIP, NB_ERR_ALLOC, NB_ERR_UNSUPPORTED = range(6)
NB_NAIVE_SIM_PARAMS, NB_TREE_SIM_PARAMS = 0, 1
NB_DIAG_MOMENTS, NB_DIAG_POTENTIAL = 1, 2
NB_RENDER_SRGB = 1
NB_RADIAL_MAX_BINS = 256
NB_RADIAL_CYLINDRICAL, NB_RADIAL_CENTER_COM = 1, 2
NB_FIELD_ACCEL, NB_FIELD_POTENTIAL = 1, 2
NB_FIELD_MAX_POINTS = 1 << 24
NB_TIDAL_K = 33
NB_ORBIT_ENERGY = 1
NB_ORBIT_SECTION_MAX_CROSSINGS, NB_ORBIT_NO_STEP = 1 << 22, (1 << 64) - 1
NB_ORBIT_MAX_TRACERS, NB_ORBIT_MAX_STEPS, NB_ORBIT_MAX_SAMPLES, NB_ORBIT_MAX_PAIRS_LOG2 = 1 << 20, 1 << 20, 1 << 22, 44
NB_ORBIT_MAX_DEVIATIONS, NB_ORBIT_MAX_RENORM_LOG2 = 6, 512
NB_MAP_MAX_SIDE, NB_MAP_MAX_CELLS = 4096, 1 << 22
NB_MAP_CENTER_COM, NB_MAP_VELOCITY = 1, 2
NB_PHASE_CENTER_COM, NB_PHASE_WEIGHT, NB_PHASE_ANY_STEP = 1, 2, 0xFFFFFFFFFFFFFFFF
NB_PHASE_Q_COUNT, NB_PHASE_Q_MASS, NB_PHASE_Q_VALUE = 18, 16, 17
NB_FOF_NONE, NB_FOF_MAX_CELLS_PER_AXIS = 0xFFFFFFFF, 1 << 21
NB_BOUND_CONVERGED, NB_BOUND_DISSOLVED, NB_BOUND_UNCONVERGED, NB_BOUND_SKIPPED = 1, 2, 4, 8
NB_BOUND_MAX_ITER = 64
NB_KNN_NONE, NB_KNN_MAX_K = 0xFFFFFFFF, 64
NB_MST_NONE, NB_MST_MAX_ROUNDS = 0xFFFFFFFF, 32
NB_KIN_SELF, NB_KIN_MOMENTS, NB_KIN_GRADS = 1, 10, 15
NB_KIN_SHORT, NB_KIN_NOT_COUNTED, NB_KIN_DEGENERATE, NB_KIN_SINGULAR = 1, 2, 4, 8
NB_HOP_NONE = 0xFFFFFFFF
NB_HALO_MAX_BINS, NB_HALO_MAX_CENTERS, NB_HALO_MAX_ROWS = 64, 1 << 20, 1 << 22
NB_HALO_MAX_CELLS_PER_AXIS, NB_HALO_CHUNK, NB_HALO_EXTRA_ITEMS = 1024, 4096, 1 << 16
NB_HALO_CENTER_NONFINITE = 1
NB_SHAPE_REDUCED = 1
NB_SHAPE_CONVERGED, NB_SHAPE_UNCONVERGED, NB_SHAPE_DEGENERATE, NB_SHAPE_EMPTY = 1, 2, 4, 8
NB_SHAPE_MAX_ITER, NB_SHAPE_ANY_STEP = 64, 0xFFFFFFFFFFFFFFFF
NB_RADII_MAX_FRACTIONS, NB_RADII_CHUNK, NB_RADII_ANY_STEP = 16, 4096, 0xFFFFFFFFFFFFFFFF
NB_MODES_MAX_BINS, NB_MODES_MAX_M, NB_MODES_FIELDS, NB_MODES_CHUNK, NB_MODES_CENTER_COM = 256, 8, 6, 4096, 1
NB_SHELL_MAX_BINS, NB_SHELL_MAX_L, NB_SHELL_MAX_L_RATES, NB_SHELL_CHUNK = 256, 6, 4, 4096
NB_SHELL_CENTER_COM, NB_SHELL_RATES = 1, 2
NB_SHELL_FOUR_PI = float("12.566370614359172")  # the header's literal
NB_SMOOTH_CENTER_COM, NB_SMOOTH_VELOCITY = 1, 2
NB_SMOOTH_K = float("0.95492965855137201461")  # K = 3 / pi, the header's literal
NB_SMOOTH_MAX_ENTRIES = 1 << 28
NB_KNN_SPHERE = float("4.1887902047863909846")  # C = 4 pi / 3, the header's literal

# every symbol include/nbody.h declares (tests check the library exports all of them)
ABI_SYMBOLS = [
    "nb_last_error", "nb_version", "nb_device_count",
    "nb_init_uniform", "nb_init_disc", "nb_init_spherical",
    "nb_shard_bodies_per_rank", "nb_shard_padded_bodies",
    "nb_sim_create", "nb_sim_create_from_particles", "nb_sim_encode", "nb_sim_encode_phase",
    "nb_sim_let_set_imports", "nb_sim_let_set_import_stride", "nb_sim_let_set_owners", "nb_sim_let_set_arrivals", "nb_sim_cleanup",
    "nb_sim_wait", "nb_sim_sim_params", "nb_sim_read_particles", "nb_sim_write_particles",
    "nb_sim_read_tree", "nb_sim_exchange_region", "nb_sim_exchange_count",
    "nb_sim_exchange_region_i", "nb_sim_step_num", "nb_sim_encode_n_timed",
    "nb_sim_set_tuning", "nb_sim_debug_buffer", "nb_sim_diagnostics",
    "nb_sim_radial_profile", "nb_radial_edges_log", "nb_radial_edges_linear", "nb_radial_lagrangian",
    "nb_sim_field", "nb_field_rings", "nb_field_ring_means", "nb_runner_field",
    "nb_tidal_sim", "nb_tidal_runner", "nb_tidal_ring_means",
    "nb_orbits_sim", "nb_orbits_runner", "nb_orbit_records", "nb_orbit_phase",
    "nb_orbit_sections_sim", "nb_orbit_sections_runner", "nb_orbit_summary_merge",
    "nb_orbit_stability_sim", "nb_orbit_stability_runner", "nb_orbit_stability_derive",
    "nb_sim_map", "nb_runner_map", "nb_map_frame", "nb_map_edges",
    "nb_phase_map_sim", "nb_phase_map_runner", "nb_phase_quantity", "nb_phase_quantity_name",
    "nb_sim_fof", "nb_runner_fof",
    "nb_fof6_sim", "nb_fof6_runner",
    "nb_sim_bound", "nb_runner_bound",
    "nb_sim_knn", "nb_runner_knn",
    "nb_local_kinematics_sim", "nb_local_kinematics_runner", "nb_local_kinematics_derive",
    "nb_mst_sim", "nb_mst_runner", "nb_mst_cut", "nb_mst_linkage",
    "nb_sim_hop", "nb_runner_hop", "nb_hop_regroup",
    "nb_sim_halo_profiles", "nb_runner_halo_profiles", "nb_halo_enclosed", "nb_halo_overdensity",
    "nb_sim_group_shapes", "nb_runner_group_shapes", "nb_shape_eigen",
    "nb_group_radii_sim", "nb_group_radii_runner",
    "nb_disc_modes_sim", "nb_disc_modes_runner", "nb_disc_modes_derive",
    "nb_shell_modes_sim", "nb_shell_modes_runner", "nb_shell_modes_derive",
    "nb_sim_smooth_map", "nb_runner_smooth_map", "nb_smooth_centres",
    "nb_camera_default", "nb_camera_view_proj", "nb_render_params_default", "nb_sim_render", "nb_naive_variant_count", "nb_naive_variant_name", "nb_sim_destroy",
    "nb_runner_create", "nb_runner_create_multi", "nb_runner_create_multi_let", "nb_runner_step_num", "nb_runner_step", "nb_runner_step_n", "nb_runner_read_particles",
    "nb_runner_set_profiling", "nb_runner_rank_times",
    "nb_runner_sim_params", "nb_runner_diagnostics", "nb_runner_radial_profile", "nb_runner_render", "nb_runner_sim", "nb_runner_destroy",
]


class NBodyError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"nbody_hip error {code}: {message}")
        self.code = code


_lib = None


def lib() -> C.CDLL:
    """Load libnbody_hip.so.  Raises (no fallback) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m wgpu_n_body_amd.build` "
            "(or __graft_entry__.build()); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp, sz, u64 = C.c_void_p, C.c_size_t, C.c_uint64
    P = C.POINTER
    L.nb_last_error.restype = C.c_char_p
    L.nb_version.restype = C.c_char_p
    L.nb_device_count.restype = C.c_int
    for name in ("nb_init_uniform", "nb_init_disc", "nb_init_spherical"):
        f = getattr(L, name)
        f.argtypes = [P(nb_sim_params), vp, vp]
        f.restype = None
    L.nb_shard_bodies_per_rank.argtypes = [sz, C.c_int]
    L.nb_shard_bodies_per_rank.restype = sz
    L.nb_shard_padded_bodies.argtypes = [sz, C.c_int]
    L.nb_shard_padded_bodies.restype = sz
    L.nb_sim_create.argtypes = [P(vp), P(nb_sim_params), P(nb_add_params), P(nb_placement), vp, vp]
    L.nb_sim_create_from_particles.argtypes = [P(vp), P(nb_sim_params), P(nb_add_params),
                                               P(nb_placement), vp, sz]
    for name in ("nb_sim_encode", "nb_sim_cleanup", "nb_sim_wait", "nb_sim_destroy"):
        getattr(L, name).argtypes = [vp]
    L.nb_sim_encode_phase.argtypes = [vp, C.c_int]
    L.nb_sim_let_set_imports.argtypes = [vp, P(C.c_uint32), C.c_int]
    L.nb_sim_let_set_import_stride.argtypes = [vp, C.c_uint32]
    L.nb_sim_let_set_owners.argtypes = [vp, P(C.c_ulonglong), C.c_int, C.c_float, C.c_uint32]
    L.nb_sim_let_set_arrivals.argtypes = [vp, C.c_uint32, P(C.c_uint32), C.c_int]
    L.nb_sim_sim_params.argtypes = [vp, P(nb_sim_params)]
    L.nb_sim_read_particles.argtypes = [vp, vp, sz]
    L.nb_sim_write_particles.argtypes = [vp, vp, sz]
    L.nb_sim_read_tree.argtypes = [vp, vp, sz, P(sz), P(C.c_float)]
    L.nb_sim_exchange_region.argtypes = [vp, P(vp), P(sz), P(sz), P(sz)]
    L.nb_sim_exchange_count.argtypes = [vp, P(C.c_int)]
    L.nb_sim_exchange_region_i.argtypes = [vp, C.c_int, P(vp), P(sz), P(sz), P(sz)]
    L.nb_sim_step_num.argtypes = [vp, P(u64)]
    L.nb_sim_encode_n_timed.argtypes = [vp, C.c_int, P(C.c_float), P(C.c_float)]
    L.nb_sim_set_tuning.argtypes = [vp, C.c_char_p, C.c_int]
    L.nb_sim_debug_buffer.argtypes = [vp, C.c_char_p, vp, sz, P(sz)]
    # the analysis passes: the arguments after the handle, the same for nb_sim_X and nb_runner_X
    passes = {
        "diagnostics": [C.c_uint32, P(nb_diagnostics)],
        "radial_profile": [P(nb_radial_params), P(nb_radial_profile), vp],
        "field": [vp, sz, C.c_uint32, vp, P(nb_field_stats)],
        "map": [P(nb_map_params), vp, vp, P(nb_map_stats)],
        "fof": [P(nb_fof_params), vp, vp, vp, sz, P(nb_fof_stats)],
        "bound": [P(nb_bound_params), vp, vp, vp, vp, sz, P(nb_bound_stats)],
        "knn": [P(nb_knn_params), vp, vp, vp, vp, P(nb_knn_stats)],
        "hop": [P(nb_hop_params), vp, vp, vp, vp, vp, sz, vp, sz, P(nb_hop_stats)],
        "halo_profiles": [P(nb_halo_params), vp, vp, P(nb_halo_stats)],
        "group_shapes": [P(nb_shape_params), vp, sz, vp, vp, vp, vp, vp, P(nb_shape_stats)],
        "smooth_map": [P(nb_smooth_params), vp, vp, vp, P(nb_smooth_stats)],
        "render": [P(nb_render_params), vp, vp, P(nb_render_stats)],
    }
    for name, args in passes.items():
        for prefix in ("nb_sim_", "nb_runner_"):
            getattr(L, prefix + name).argtypes = [vp] + args
    # the thirteenth pass is spelt noun first (include/nbody.h "Group radii"): one list for its two symbols too
    group_radii = [vp, P(nb_radii_params), vp, sz, vp, vp, vp, vp, P(nb_radii_stats)]
    for suffix in ("sim", "runner"):
        getattr(L, "nb_group_radii_" + suffix).argtypes = group_radii
    # ... and the fourteenth (include/nbody.h "Disc modes")
    disc_modes = [vp, P(nb_modes_params), P(nb_modes_head), vp, vp]
    for suffix in ("sim", "runner"):
        getattr(L, "nb_disc_modes_" + suffix).argtypes = disc_modes
    # ... and the shells' harmonics (include/nbody.h "Shell modes")
    shell_modes = [vp, P(nb_shell_params), P(nb_shell_head), vp, vp]
    for suffix in ("sim", "runner"):
        getattr(L, "nb_shell_modes_" + suffix).argtypes = shell_modes
    L.nb_shell_modes_derive.argtypes = [P(nb_shell_head), vp, vp, vp, vp, vp]
    # ... and the fifteenth (include/nbody.h "Phase maps")
    phase_map = [vp, P(nb_phase_params), vp, vp, P(nb_phase_stats)]
    for suffix in ("sim", "runner"):
        getattr(L, "nb_phase_map_" + suffix).argtypes = phase_map
    # ... and the sixteenth (include/nbody.h "Tidal tensor probes")
    tidal = [vp, vp, sz, vp, P(nb_tidal_stats)]
    for suffix in ("sim", "runner"):
        getattr(L, "nb_tidal_" + suffix).argtypes = tidal
    # ... and the seventeenth (include/nbody.h "Local kinematics")
    local_kinematics = [vp, P(nb_kin_params), vp, vp, vp, vp, vp, vp, P(nb_kin_stats)]
    for suffix in ("sim", "runner"):
        getattr(L, "nb_local_kinematics_" + suffix).argtypes = local_kinematics
    L.nb_local_kinematics_derive.argtypes = [vp, vp, vp, vp, vp, sz, vp]
    # ... and the eighteenth (include/nbody.h "Orbits")
    orbits = [vp, P(nb_orbit_params), vp, vp, sz, vp, vp, P(nb_orbit_stats)]
    for suffix in ("sim", "runner"):
        getattr(L, "nb_orbits_" + suffix).argtypes = orbits
    # ... and the nineteenth (include/nbody.h "Phase-space groups")
    fof6 = [vp, P(nb_fof6_params), vp, vp, vp, sz, P(nb_fof_stats)]
    for suffix in ("sim", "runner"):
        getattr(L, "nb_fof6_" + suffix).argtypes = fof6
    # ... and the orbits' sections (include/nbody.h "Orbit sections")
    orbit_sections = [vp, P(nb_orbit_params), P(nb_orbit_section_params), vp, vp, sz, vp, vp, vp, vp, vp,
                      P(nb_orbit_section_stats)]
    for suffix in ("sim", "runner"):
        getattr(L, "nb_orbit_sections_" + suffix).argtypes = orbit_sections
    L.nb_orbit_summary_merge.argtypes = [vp, vp, vp]
    # ... and their stability (include/nbody.h "Orbit stability")
    orbit_stability = [vp, P(nb_orbit_params), P(nb_orbit_stability_params), vp, vp, sz, vp, vp, vp, vp, vp,
                       P(nb_orbit_stability_stats)]
    for suffix in ("sim", "runner"):
        getattr(L, "nb_orbit_stability_" + suffix).argtypes = orbit_stability
    L.nb_orbit_stability_derive.argtypes = [C.c_double, C.c_uint32, C.c_uint32, sz, C.c_uint32, vp, vp, vp, vp, vp, vp]
    # ... and the spanning tree (include/nbody.h "Minimum spanning tree")
    mst = [vp, P(nb_mst_params), vp, vp, vp, vp, P(nb_mst_stats)]
    for suffix in ("sim", "runner"):
        getattr(L, "nb_mst_" + suffix).argtypes = mst
    L.nb_mst_cut.argtypes = [sz, sz, vp, vp, vp, vp, C.c_double, vp, P(sz)]
    L.nb_mst_linkage.argtypes = [sz, sz, vp, vp, vp, vp, vp, vp]
    L.nb_orbit_records.argtypes = [C.c_uint32, C.c_uint32]
    L.nb_orbit_records.restype = C.c_uint32
    L.nb_orbit_phase.argtypes = [C.c_double, C.c_double, u64, P(C.c_double), P(C.c_double)]
    L.nb_phase_quantity.argtypes = [C.c_char_p, P(C.c_uint32)]
    L.nb_phase_quantity_name.argtypes = [C.c_uint32]
    L.nb_phase_quantity_name.restype = C.c_char_p
    L.nb_disc_modes_derive.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp]
    for name in ("nb_radial_edges_log", "nb_radial_edges_linear"):
        getattr(L, name).argtypes = [C.c_double, C.c_double, C.c_uint32, P(C.c_double)]
    L.nb_radial_lagrangian.argtypes = [P(nb_radial_profile), vp, P(C.c_double), P(C.c_double), C.c_uint32,
                                       P(C.c_double)]
    L.nb_field_rings.argtypes = [P(C.c_double), P(C.c_double), P(C.c_double), C.c_uint32, C.c_uint32, vp]
    L.nb_field_ring_means.argtypes = [P(C.c_double), P(C.c_double), P(C.c_double), C.c_uint32, C.c_uint32, vp, vp,
                                      vp]
    L.nb_tidal_ring_means.argtypes = [P(C.c_double), P(C.c_double), P(C.c_double), C.c_uint32, C.c_uint32, vp, vp,
                                      vp, vp]
    L.nb_hop_regroup.argtypes = [vp, vp, sz, vp, sz, P(nb_hop_regroup_params), vp, vp, vp, sz, P(sz)]
    L.nb_shape_eigen.argtypes = [P(C.c_double), P(C.c_double), P(C.c_double)]
    L.nb_halo_enclosed.argtypes = [vp, vp, C.c_uint32, P(C.c_double)]
    L.nb_halo_overdensity.argtypes = [vp, vp, P(C.c_double), C.c_uint32, C.c_double, P(C.c_double), P(C.c_double)]
    L.nb_smooth_centres.argtypes = [C.c_double, C.c_double, C.c_uint32, P(C.c_double)]
    L.nb_map_frame.argtypes = [P(C.c_double), P(C.c_double), P(C.c_double), P(C.c_double)]
    L.nb_map_edges.argtypes = [C.c_double, C.c_double, C.c_uint32, P(C.c_double)]
    L.nb_camera_default.argtypes = [P(nb_camera), C.c_uint32, C.c_uint32]
    L.nb_camera_view_proj.argtypes = [P(nb_camera), P(C.c_float)]
    L.nb_render_params_default.argtypes = [P(nb_render_params), C.c_uint32, C.c_uint32]
    L.nb_naive_variant_count.restype = C.c_int
    L.nb_naive_variant_name.argtypes = [C.c_int]
    L.nb_naive_variant_name.restype = C.c_char_p
    L.nb_runner_create.argtypes = [P(vp), P(nb_sim_params), P(nb_add_params), vp, vp, C.c_int]
    L.nb_runner_create_multi.argtypes = [P(vp), P(nb_sim_params), P(nb_add_params), vp, vp, P(C.c_int), C.c_int]
    L.nb_runner_create_multi_let.argtypes = [P(vp), P(nb_sim_params), P(nb_add_params), vp, vp, P(C.c_int), C.c_int,
                                             C.c_int]
    L.nb_runner_step_num.argtypes = [vp, P(u64)]
    L.nb_runner_step.argtypes = [vp]
    L.nb_runner_step_n.argtypes = [vp, C.c_int]
    L.nb_runner_read_particles.argtypes = [vp, vp, sz]
    L.nb_runner_set_profiling.argtypes = [vp, C.c_int]
    L.nb_runner_rank_times.argtypes = [vp, P(C.c_float), P(C.c_float), C.c_int]
    L.nb_runner_sim_params.argtypes = [vp, P(nb_sim_params)]
    L.nb_runner_sim.argtypes = [vp]
    L.nb_runner_sim.restype = vp
    L.nb_runner_destroy.argtypes = [vp]
    _lib = L
    return L


def check(rc: int) -> None:
    if rc != NB_OK:
        raise NBodyError(rc, lib().nb_last_error().decode(errors="replace"))
