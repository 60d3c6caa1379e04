"""wgpu_n_body_amd -- MI355X-native drop-in for the simulation hot path of
arpan-dhatt/wgpu-n-body (its `sims` + `runners::OfflineHeadless` + `inits` API).

Python host-side mirror of the reference's interface for this path, over the C ABI of
include/nbody.h (libnbody_hip.so: hand-written HIP kernels for gfx950).  Names follow
the reference crate:

    reference (Rust)                               here
    ---------------------------------------------  -----------------------------------
    sims::SimParams            (sims/mod.rs:51-71)  SimParams
    sims::AddParams            (sims/mod.rs:18-23)  AddParams.NaiveSimParams / .TreeSimParams
    sims::Particle             (sims/mod.rs:9-16)   PARTICLE_DTYPE (numpy, 40 B)
    trait sims::Simulator      (sims/mod.rs:73-90)  Simulator (new/encode/dest_particle_slice/
                                                    sim_params/cleanup)
    sims::NaiveSim, TreeSim    (sims/mod.rs:4-5)    NaiveSim, TreeSim
    runners::OfflineHeadless   (offline_headless.rs) OfflineHeadless
    inits::{uniform,disc,spherical}_init (inits.rs) inits.uniform_init / disc_init / spherical_init

There is no CPU fallback: importing works without a GPU (so the ABI can be checked), but
constructing a simulator raises NBodyError(NB_ERR_NO_DEVICE) when no HIP device exists.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools
import math
from dataclasses import dataclass
from typing import Callable, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import (NB_NAIVE_SIM_PARAMS, NB_TREE_SIM_PARAMS, OCTANT_DTYPE, PARTICLE_DTYPE,
                   NBodyError, check)

__all__ = ["SimParams", "AddParams", "Placement", "Simulator", "NaiveSim", "TreeSim",
           "OfflineHeadless", "inits", "PARTICLE_DTYPE", "OCTANT_DTYPE", "NBodyError",
           "PARTICLES_PER_GROUP", "device_count", "version", "shard_bodies_per_rank",
           "shard_padded_bodies", "naive_variants", "Diagnostics", "RadialProfile", "radial_edges",
           "Field", "RingMeans", "field_rings", "TidalField", "DiscFrequencies", "Orbits", "OrbitStats", "OrbitSections", "OrbitSectionStats", "OrbitStability", "OrbitStabilityStats", "ProjectedMap", "map_frame", "map_edges",
           "PhaseMap", "PhaseStats", "phase_quantity", "phase_quantities", "phase_edges",
           "FofGroups", "FofStats", "FOF_NONE", "PhaseSpaceGroups",
           "BoundGroups", "BoundStats", "BOUND_CONVERGED", "BOUND_DISSOLVED", "BOUND_UNCONVERGED", "BOUND_SKIPPED",
           "KnnDensity", "KnnStats", "KNN_NONE",
           "SpanningTree", "MstStats", "MST_NONE",
           "LocalKinematics", "KinStats", "kinematics_derive", "KIN_SHORT", "KIN_NOT_COUNTED", "KIN_DEGENERATE",
           "KIN_SINGULAR",
           "HopGroups", "HopStats", "HOP_NONE",
           "HaloProfiles", "HaloStats", "HALO_CENTER_NONFINITE",
           "GroupRadii", "RadiiStats",
           "DiscModes", "MODES_FIELDS", "ShellModes", "shell_index",
           "SmoothedMap", "SmoothStats", "smooth_centres", "SMOOTH_K", "SMOOTH_PLANES",
           "Camera", "RenderParams", "RenderStats", "Frame", "write_ppm"]

PARTICLES_PER_GROUP = 64  # sims/mod.rs:7


@dataclass(frozen=True)
class SimParams:
    """`struct SimParams` with `Default` (sims/mod.rs:51-71)."""
    particle_num: int = 10000
    g: float = 0.000001
    e: float = 0.0001
    dt: float = 0.016

    def to_c(self) -> _lib.nb_sim_params:
        return _lib.nb_sim_params(int(self.particle_num), float(self.g), float(self.e),
                                  float(self.dt))


@dataclass(frozen=True)
class AddParams:
    """`enum AddParams` (sims/mod.rs:18-23)."""
    kind: int = NB_NAIVE_SIM_PARAMS
    theta: float = 0.0

    @staticmethod
    def NaiveSimParams() -> "AddParams":
        return AddParams(NB_NAIVE_SIM_PARAMS, 0.0)

    @staticmethod
    def TreeSimParams(theta: float) -> "AddParams":
        return AddParams(NB_TREE_SIM_PARAMS, float(theta))

    def to_c(self) -> _lib.nb_add_params:
        return _lib.nb_add_params(int(self.kind), float(self.theta))


@dataclass(frozen=True)
class Placement:
    """Device + body shard of a simulator (nb_placement; no reference counterpart -- the
    reference is single-adapter, offline_headless.rs:22-31)."""
    device_id: int = 0
    rank: int = 0
    world: int = 1
    stream: int = 0                      # hipStream_t as an integer, 0 = own stream
    posm: Sequence[int] = (0, 0)         # optional caller-owned ping-pong buffers

    def to_c(self) -> _lib.nb_placement:
        p = _lib.nb_placement()
        p.device_id, p.rank, p.world = int(self.device_id), int(self.rank), int(self.world)
        p.stream = C.c_void_p(int(self.stream) or None)
        p.posm[0] = C.c_void_p(int(self.posm[0]) or None)
        p.posm[1] = C.c_void_p(int(self.posm[1]) or None)
        return p


InitFn = Callable[[SimParams], np.ndarray]


@dataclass(frozen=True)
class Diagnostics:
    """nb_diagnostics (include/nbody.h "Diagnostics"; no reference counterpart): conserved-quantity
    monitor of the state read_particles would return, computed on the device in fp64.  Vectors are
    float64 arrays of 3.  pair_sum W = sum_{i<j} m_i m_j psi(r_ij), potential U = -g dt W and
    total E = kinetic + U are NaN unless the potential was requested.  E is a monitor, not an
    invariant of the integrator."""
    step_num: int
    n: int
    nonfinite: int
    mass: float
    com: np.ndarray
    momentum: np.ndarray
    angular_momentum: np.ndarray
    kinetic: float
    max_speed: float
    pair_sum: float
    potential: float
    total: float
    flags: int

    @staticmethod
    def _from_c(d: "_lib.nb_diagnostics") -> "Diagnostics":
        vec = lambda a: np.array(list(a), dtype=np.float64)  # noqa: E731
        return Diagnostics(int(d.step_num), int(d.n), int(d.nonfinite), float(d.mass), vec(d.com),
                           vec(d.momentum), vec(d.angular_momentum), float(d.kinetic), float(d.max_speed),
                           float(d.pair_sum), float(d.potential), float(d.total), int(d.flags))


def _diag_flags(potential: bool) -> int:
    return _lib.NB_DIAG_MOMENTS | (_lib.NB_DIAG_POTENTIAL if potential else 0)


def radial_edges(rmin: float, rmax: float, nbins: int = 64, log: bool = True) -> np.ndarray:
    """nb_radial_edges_log / nb_radial_edges_linear: nbins + 1 radii from rmin to rmax (both exact) with
    a constant ratio (log, rmin > 0) or a constant step."""
    out = np.empty(int(nbins) + 1 if 1 <= int(nbins) <= _lib.NB_RADIAL_MAX_BINS else 1, dtype=np.float64)
    fn = _lib.lib().nb_radial_edges_log if log else _lib.lib().nb_radial_edges_linear
    check(fn(float(rmin), float(rmax), int(nbins), out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


@dataclass(frozen=True)
class RadialProfile:
    """nb_radial_profile + nb_radial_bin[nbins] (include/nbody.h "Radial profiles"; no reference
    counterpart): the state read_particles would return, binned on the device by distance from a centre
    (or, cylindrical, from an axis through it).  Per-bin fields are float64 arrays of nbins (count:
    uint64, ang: (nbins, 3)); `mass` is the mass of all finite bodies, `bin_mass` the per-bin sums.
    inside_* / outside_* hold what fell below edges[0] / at or beyond edges[-1]."""
    step_num: int
    n: int
    nonfinite: int
    inside_count: int
    outside_count: int
    inside_mass: float
    outside_mass: float
    mass: float
    center: np.ndarray
    velocity: np.ndarray
    axis: np.ndarray
    shape: np.ndarray      # sum m d_i d_j: xx, yy, zz, xy, xz, yz over the bodies inside edges[-1]
    flags: int
    edges: np.ndarray      # nbins + 1
    count: np.ndarray
    bin_mass: np.ndarray   # sum m
    m_r: np.ndarray        # sum m r
    m_ur: np.ndarray       # sum m u_r
    m_ur2: np.ndarray      # sum m u_r^2
    m_uphi: np.ndarray     # sum m u_phi (cylindrical)
    m_uphi2: np.ndarray    # sum m u_phi^2 (cylindrical)
    m_u2: np.ndarray       # sum m |u|^2
    ang: np.ndarray        # sum m (d x u)

    @staticmethod
    def _from_c(p: "_lib.nb_radial_profile", bins: np.ndarray, edges: np.ndarray) -> "RadialProfile":
        vec = lambda a: np.array(list(a), dtype=np.float64)  # noqa: E731
        return RadialProfile(int(p.step_num), int(p.n), int(p.nonfinite), int(p.inside_count), int(p.outside_count),
                             float(p.inside_mass), float(p.outside_mass), float(p.mass), vec(p.center),
                             vec(p.velocity), vec(p.axis), vec(p.shape), int(p.flags), edges.copy(),
                             bins["count"].copy(), bins["mass"].copy(), bins["m_r"].copy(), bins["m_ur"].copy(),
                             bins["m_ur2"].copy(), bins["m_uphi"].copy(), bins["m_uphi2"].copy(),
                             bins["m_u2"].copy(), bins["ang"].copy())

    @property
    def nbins(self) -> int:
        return self.edges.shape[0] - 1

    @property
    def cylindrical(self) -> bool:
        return bool(self.flags & _lib.NB_RADIAL_CYLINDRICAL)

    @property
    def density(self) -> np.ndarray:
        """bin_mass over the shell's volume 4 pi (b^3 - a^3) / 3, or (cylindrical) the annulus' area
        pi (b^2 - a^2): a surface density."""
        a, b = self.edges[:-1], self.edges[1:]
        size = np.pi * (b * b - a * a) if self.cylindrical else 4.0 * np.pi / 3.0 * (b ** 3 - a ** 3)
        return self.bin_mass / size

    @property
    def sigma_r(self) -> np.ndarray:
        """Mass-weighted radial velocity dispersion per bin (NaN in a bin without mass)."""
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = self.m_ur / self.bin_mass
            return np.sqrt(np.maximum(self.m_ur2 / self.bin_mass - mean * mean, 0.0))

    @property
    def mean_uphi(self) -> np.ndarray:
        """Mass-weighted mean tangential velocity per bin: a disc's rotation curve (cylindrical)."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.m_uphi / self.bin_mass

    @property
    def cumulative_mass(self) -> np.ndarray:
        """Mass within edges[k + 1]: inside_mass plus the bins up to and including k."""
        return self.inside_mass + np.cumsum(self.bin_mass)

    def lagrangian(self, fractions) -> np.ndarray:
        """nb_radial_lagrangian: the radii enclosing the given fractions of `mass`, linear inside the bin
        that crosses (so limited by the bins' resolution); NaN where the crossing is not in a bin."""
        f = np.ascontiguousarray(np.atleast_1d(fractions), dtype=np.float64)
        p = _lib.nb_radial_profile()
        p.mass, p.inside_mass, p.outside_mass, p.nbins = self.mass, self.inside_mass, self.outside_mass, self.nbins
        bins = np.zeros(self.nbins, dtype=_lib.RADIAL_BIN_DTYPE)
        bins["mass"] = self.bin_mass
        edges = np.ascontiguousarray(self.edges, dtype=np.float64)
        out = np.empty(f.shape[0], dtype=np.float64)
        dp = C.POINTER(C.c_double)
        check(_lib.lib().nb_radial_lagrangian(C.byref(p), bins.ctypes.data, edges.ctypes.data_as(dp),
                                              f.ctypes.data_as(dp), f.shape[0], out.ctypes.data_as(dp)))
        return out


def _radial_profile(call, handle, edges, nbins, rmin, rmax, log, cylindrical, axis, center, velocity):
    if edges is None:
        if rmin is None or rmax is None:
            raise ValueError("radial_profile needs edges, or rmin and rmax")
        edges = radial_edges(rmin, rmax, nbins, log)
    edges = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
    p = _lib.nb_radial_params()
    p.nbins = max(edges.shape[0] - 1, 0)
    p.flags = _lib.NB_RADIAL_CYLINDRICAL if cylindrical else 0
    if isinstance(center, str):
        if center != "com":
            raise ValueError('center is "com" or three coordinates')
        p.flags |= _lib.NB_RADIAL_CENTER_COM
    else:
        for k in range(3):
            p.center[k], p.velocity[k] = float(center[k]), float(velocity[k])
    for k in range(3):
        p.axis[k] = float(axis[k])
    p.edges = edges.ctypes.data_as(C.POINTER(C.c_double))
    out = _lib.nb_radial_profile()
    bins = np.zeros(max(int(p.nbins), 1), dtype=_lib.RADIAL_BIN_DTYPE)
    check(call(handle, C.byref(p), C.byref(out), bins.ctypes.data))
    return RadialProfile._from_c(out, bins, edges)


MODES_FIELDS = ("C", "S", "DC", "DS", "ZC", "ZS")


def _wrap_phase(x, m):
    """x wrapped into (-pi/m, pi/m]."""
    period = 2.0 * np.pi / m
    return x - period * np.ceil(x / period - 0.5)


@dataclass(frozen=True)
class DiscModes:
    """nb_modes_head + nb_modes_bin[nbins] + modes[nbins][mmax + 1][6] (include/nbody.h "Disc modes"; no reference
    counterpart): per annulus of the state read_particles would return, about `axis` through `center`, the sums
    over the members of mu e^(i m phi) (C, S), of the same weighted by dphi/dt (DC, DS) and by the height above the
    plane (ZC, ZS), summed on the device in a fixed order.  phi = 0 is along e1 (map_frame(axis)).  modes:
    (nbins, mmax + 1, 6) float64 in the order MODES_FIELDS; count: uint64; m_r: sum mu R; m_h2: sum mu h^2."""
    step_num: int
    n: int
    nonfinite: int
    inside_count: int
    outside_count: int
    inside_mass: float
    outside_mass: float
    mass: float
    center: np.ndarray
    velocity: np.ndarray
    axis: np.ndarray
    e1: np.ndarray
    e2: np.ndarray
    flags: int
    mmax: int
    dt: float              # the simulator's time step (pattern_speed_between)
    edges: np.ndarray      # nbins + 1
    count: np.ndarray
    m_r: np.ndarray
    m_h2: np.ndarray
    modes: np.ndarray

    @property
    def nbins(self) -> int:
        return self.edges.shape[0] - 1

    @property
    def bin_mass(self) -> np.ndarray:
        """C_0: the mass of every annulus."""
        return self.modes[:, 0, 0]

    def derived(self, m: int) -> np.ndarray:
        """nb_disc_modes_derive: _lib.MODES_DERIVED_DTYPE records of mode m (1 <= m <= mmax), one per bin."""
        out = np.zeros(self.nbins, dtype=_lib.MODES_DERIVED_DTYPE)
        modes = np.ascontiguousarray(self.modes, dtype=np.float64)
        check(_lib.lib().nb_disc_modes_derive(modes.ctypes.data, self.nbins, self.mmax, int(m), out.ctypes.data))
        return out

    def amplitude(self, m: int) -> np.ndarray:
        """A_m / A_0 = hypot(C_m, S_m) / C_0 per bin (NaN in a bin without mass)."""
        return self.derived(m)["amplitude"]

    def phase(self, m: int) -> np.ndarray:
        """atan2(S_m, C_m) / m per bin, in (-pi/m, pi/m]: the azimuth of the mode's maximum from e1."""
        return self.derived(m)["phase"]

    def pattern_speed(self, m: int) -> np.ndarray:
        """The single-snapshot pattern speed (C DC + S DS) / (C^2 + S^2) per bin: the rate at which the phase of the
        bodies now in the annulus turns (the flux through the annulus' edges is not in it)."""
        return self.derived(m)["pattern_speed"]

    def bending(self, m: int):
        """(amplitude, phase) of the bending mode m: hypot(ZC_m, ZS_m) / C_0 and atan2(ZS_m, ZC_m) / m per bin."""
        d = self.derived(m)
        return d["bend_amplitude"], d["bend_phase"]

    def bar_strength(self):
        """(A_2, bin): the largest A_2 / A_0 over the bins with mass and the bin it occurs in ((nan, -1): none)."""
        a = self.amplitude(2)
        ok = np.isfinite(a) & (self.bin_mass != 0.0)
        if not ok.any():
            return float("nan"), -1
        k = int(np.argmax(np.where(ok, a, -np.inf)))
        return float(a[k]), k

    def warp_tilt(self) -> np.ndarray:
        """2 hypot(ZC_1, ZS_1) / sum mu R per bin: the tilt (rise over run) of the annulus' plane."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return 2.0 * np.hypot(self.modes[:, 1, 4], self.modes[:, 1, 5]) / self.m_r

    def thickness(self) -> np.ndarray:
        """sqrt(sum mu h^2 / C_0 - (ZC_0 / C_0)^2) per bin: the rms height about the mean height."""
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = self.modes[:, 0, 4] / self.bin_mass
            return np.sqrt(np.maximum(self.m_h2 / self.bin_mass - mean * mean, 0.0))

    def total(self, m: int) -> np.ndarray:
        """The six sums of mode m over all bins, the bins added in order."""
        out = np.zeros(6)
        for k in range(self.nbins):
            out = out + self.modes[k, m]
        return out

    def pattern_speed_between(self, other: "DiscModes", m: int, time=None) -> np.ndarray:
        """The pattern speed of mode m from two measurements: (other.phase(m) - self.phase(m)) wrapped into
        (-pi/m, pi/m], over `time` (default: the steps between the two times dt)."""
        if time is None:
            time = (other.step_num - self.step_num) * self.dt
        return _wrap_phase(other.phase(m) - self.phase(m), int(m)) / time


def _disc_modes(call, handle, dt, edges, nbins, rmin, rmax, log, mmax, axis, center, velocity) -> DiscModes:
    if edges is None:
        if rmin is None or rmax is None:
            raise ValueError("disc_modes needs edges, or rmin and rmax")
        edges = radial_edges(rmin, rmax, nbins, log)
    edges = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
    if not 0 <= int(mmax) <= 0xFFFFFFFF:
        raise ValueError(f"disc_modes: mmax = {mmax} is not a 32-bit count")
    p = _lib.nb_modes_params()
    p.nbins, p.mmax, p.flags, p.reserved = max(edges.shape[0] - 1, 0), int(mmax), 0, 0
    if isinstance(center, str):
        if center != "com":
            raise ValueError('center is "com", "density" or three coordinates')
        if velocity is not None:
            raise ValueError('center="com" brings its own velocity')
        p.flags |= _lib.NB_MODES_CENTER_COM
    else:
        velocity = (0.0, 0.0, 0.0) if velocity is None else velocity
        for k in range(3):
            p.center[k], p.velocity[k] = float(center[k]), float(velocity[k])
    for k in range(3):
        p.axis[k] = float(axis[k])
    p.edges = edges.ctypes.data_as(C.POINTER(C.c_double))
    out = _lib.nb_modes_head()
    nb_, mm = max(int(p.nbins), 1), min(int(p.mmax), _lib.NB_MODES_MAX_M)  # (the call refuses what it does not take)
    bins = np.zeros(nb_, dtype=_lib.MODES_BIN_DTYPE)
    modes = np.zeros((nb_, mm + 1, _lib.NB_MODES_FIELDS), dtype=np.float64)
    check(call(handle, C.byref(p), C.byref(out), bins.ctypes.data, modes.ctypes.data))
    vec = lambda a: np.array(list(a), dtype=np.float64)  # noqa: E731
    return DiscModes(int(out.step_num), int(out.n), int(out.nonfinite), int(out.inside_count),
                     int(out.outside_count), float(out.inside_mass), float(out.outside_mass), float(out.mass),
                     vec(out.center), vec(out.velocity), vec(out.axis), vec(out.e1), vec(out.e2), int(out.flags),
                     int(out.mmax), float(dt), edges.copy(), bins["count"].copy(), bins["m_r"].copy(),
                     bins["m_h2"].copy(), modes)


def shell_index(l: int, m: int, sine: bool = False) -> int:
    """The place of sum (l, m) in a shell's block of (lmax + 1)^2: l^2 for m = 0, l^2 + 2m - 1 for the cosine sum and
    l^2 + 2m for the sine sum."""
    l, m = int(l), int(m)
    if not 0 <= m <= l or (sine and m == 0):
        raise ValueError(f"shell_index: needs 0 <= m <= l, and m >= 1 for a sine sum (got l = {l}, m = {m})")
    return l * l + (2 * m - (0 if sine else 1) if m else 0)


@dataclass(frozen=True)
class ShellModes:
    """nb_shell_head + nb_shell_bin[nbins] + coef[nbins][(lmax + 1)^2 (1 + rates)] (include/nbody.h "Shell modes"; no
    reference counterpart): per spherical shell of the state read_particles would return, about `center`, the sums
    over the members of mu Q_l^m(cos theta) sin^m theta (cos, sin)(m phi), the unnormalised real spherical harmonics
    with `axis` as the polar axis and phi = 0 along e1 (map_frame(axis)), summed on the device in a fixed order.
    coef: (nbins, (lmax + 1)^2) float64 indexed by shell_index(); rate: their time derivatives for the bodies now in
    the shell, or None; count: uint64; m_r: sum mu r; m_ur: sum mu u_r."""
    step_num: int
    n: int
    nonfinite: int
    inside_count: int
    outside_count: int
    inside_mass: float
    outside_mass: float
    mass: float
    center: np.ndarray
    velocity: np.ndarray
    axis: np.ndarray
    e1: np.ndarray
    e2: np.ndarray
    flags: int
    lmax: int
    dt: float              # the simulator's time step
    edges: np.ndarray      # nbins + 1
    count: np.ndarray
    m_r: np.ndarray
    m_ur: np.ndarray
    coef: np.ndarray
    rate: Optional[np.ndarray]

    @property
    def nbins(self) -> int:
        return self.edges.shape[0] - 1

    @property
    def bin_mass(self) -> np.ndarray:
        """C_00: the mass of every shell."""
        return self.coef[:, 0]

    def coefficient(self, l: int, m: int, sine: bool = False) -> np.ndarray:
        """Sum (l, m) per bin: the cosine sum, or with sine=True the sine sum."""
        self._check_lm(l, m, 0)
        return self.coef[:, shell_index(l, m, sine)]

    def _check_lm(self, l, m, mmin):
        if not (mmin <= int(m) <= int(l) <= self.lmax):
            raise ValueError(f"ShellModes: needs {mmin} <= m <= l <= lmax = {self.lmax} (got l = {l}, m = {m})")

    def _derive(self, norm=False, phase=False, speed=False):
        """nb_shell_modes_derive: (_lib.SHELL_DERIVED_DTYPE records per bin, norm, phase, speed), the arrays asked for
        (nbins, (lmax + 1)^2), the others None."""
        head = _lib.nb_shell_head()
        head.nbins, head.lmax, head.flags = self.nbins, self.lmax, self.flags
        for k in range(3):
            head.axis[k], head.e1[k], head.e2[k] = float(self.axis[k]), float(self.e1[k]), float(self.e2[k])
        nk = (self.lmax + 1) ** 2
        both = self.coef if self.rate is None else np.concatenate([self.coef, self.rate], axis=1)
        both = np.ascontiguousarray(both, dtype=np.float64)
        out = np.zeros(self.nbins, dtype=_lib.SHELL_DERIVED_DTYPE)
        arrays = [np.zeros((self.nbins, nk)) if want else None for want in (norm, phase, speed)]
        check(_lib.lib().nb_shell_modes_derive(C.byref(head), both.ctypes.data, out.ctypes.data,
                                               *[None if a is None else a.ctypes.data for a in arrays]))
        return (out, *arrays)

    def normalised(self) -> np.ndarray:
        """The coefficients of the orthonormal real harmonics, N_lm times the sums: (nbins, (lmax + 1)^2)."""
        return self._derive(norm=True)[1]

    def power(self) -> np.ndarray:
        """sum_m a_lm^2 / (2l + 1) per bin and l, (nbins, lmax + 1): it does not depend on the axis."""
        return self._derive()[0]["power"][:, :self.lmax + 1]

    def relative(self, l: int) -> np.ndarray:
        """sqrt(power_l / power_0) per bin (NaN in a bin without mass)."""
        self._check_lm(l, 0, 0)
        return self._derive()[0]["relative"][:, int(l)]

    def dipole(self) -> np.ndarray:
        """The l = 1 vector a_11c e1 + a_11s e2 + a_10 n per bin, (nbins, 3) in the state's coordinates: the direction
        in which the shell's mass is displaced (NaN for lmax = 0)."""
        return self._derive()[0]["dipole"]

    def quadrupole_axes(self):
        """(values, axes): the eigenvalues (nbins, 3), descending, and unit eigenvectors (nbins, 3, 3; axes[k, j] is
        vector j) of the traceless tensor of the l = 2 coefficients, in the state's coordinates (nb_shape_eigen).
        NaN for lmax < 2."""
        d = self._derive()[0]
        return d["quad_values"], d["quad_axes"]

    def phase(self, l: int, m: int) -> np.ndarray:
        """atan2(S_lm, C_lm) / m per bin, in (-pi/m, pi/m]: the azimuth about the axis of component (l, m)."""
        self._check_lm(l, m, 1)
        return self._derive(phase=True)[2][:, shell_index(l, m)]

    def pattern_speed(self, l: int, m: int) -> np.ndarray:
        """(C DS - S DC) / (m (C^2 + S^2)) per bin: the rate at which component (l, m) of the bodies now in the shell
        turns about the axis (the flux through the shell's edges is not in it).  Needs rates=True."""
        self._check_lm(l, m, 1)
        if self.rate is None:
            raise ValueError("ShellModes.pattern_speed needs shell_modes(rates=True)")
        return self._derive(speed=True)[3][:, shell_index(l, m)]

    def phase_between(self, other: "ShellModes", l: int, m: int) -> np.ndarray:
        """(other.phase(l, m) - self.phase(l, m)) wrapped into (-pi/m, pi/m] per bin: over the time between the two
        measurements it is the pattern speed of component (l, m), flux through the edges included."""
        return _wrap_phase(other.phase(l, m) - self.phase(l, m), int(m))


def _shell_modes(call, handle, dt, edges, nbins, rmin, rmax, log, lmax, rates, axis, center, velocity) -> ShellModes:
    if edges is None:
        if rmin is None or rmax is None:
            raise ValueError("shell_modes needs edges, or rmin and rmax")
        edges = radial_edges(rmin, rmax, nbins, log)
    edges = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
    if not 0 <= int(lmax) <= 0xFFFFFFFF:
        raise ValueError(f"shell_modes: lmax = {lmax} is not a 32-bit count")
    p = _lib.nb_shell_params()
    p.nbins, p.lmax, p.reserved = max(edges.shape[0] - 1, 0), int(lmax), 0
    p.flags = _lib.NB_SHELL_RATES if rates else 0
    if isinstance(center, str):
        if center != "com":
            raise ValueError('center is "com", "density" or three coordinates')
        if velocity is not None:
            raise ValueError('center="com" brings its own velocity')
        p.flags |= _lib.NB_SHELL_CENTER_COM
    else:
        velocity = (0.0, 0.0, 0.0) if velocity is None else velocity
        for k in range(3):
            p.center[k], p.velocity[k] = float(center[k]), float(velocity[k])
    for k in range(3):
        p.axis[k] = float(axis[k])
    p.edges = edges.ctypes.data_as(C.POINTER(C.c_double))
    out = _lib.nb_shell_head()
    nb_, nk = max(int(p.nbins), 1), (min(int(p.lmax), _lib.NB_SHELL_MAX_L) + 1) ** 2  # (the call refuses the rest)
    bins = np.zeros(nb_, dtype=_lib.SHELL_BIN_DTYPE)
    coef = np.zeros((nb_, nk * (2 if rates else 1)), dtype=np.float64)
    check(call(handle, C.byref(p), C.byref(out), bins.ctypes.data, coef.ctypes.data))
    vec = lambda a: np.array(list(a), dtype=np.float64)  # noqa: E731
    return ShellModes(int(out.step_num), int(out.n), int(out.nonfinite), int(out.inside_count),
                      int(out.outside_count), float(out.inside_mass), float(out.outside_mass), float(out.mass),
                      vec(out.center), vec(out.velocity), vec(out.axis), vec(out.e1), vec(out.e2), int(out.flags),
                      int(out.lmax), float(dt), edges.copy(), bins["count"].copy(), bins["m_r"].copy(),
                      bins["m_ur"].copy(), coef[:, :nk].copy(), coef[:, nk:].copy() if rates else None)


@dataclass(frozen=True)
class Field:
    """nb_field_sample[M] + nb_field_stats (include/nbody.h "Field probes"; no reference counterpart): the
    exact all-pairs acceleration (without the dt the stored Particle.acceleration carries) and potential
    of the state read_particles would return, at M points.  A field that was not requested is NaN."""
    acc: np.ndarray          # (M, 3) float64
    potential: np.ndarray    # (M,) float64
    coincident: np.ndarray   # (M,) uint32: bodies at the point itself, left out of both sums
    step_num: int
    n: int
    nonfinite: int           # bodies left out, as diagnostics() counts them
    points: int
    nonfinite_points: int
    flags: int
    launches: int


@dataclass(frozen=True)
class RingMeans:
    """nb_field_ring[k]: per ring the means over its azimuths of the radial and axial acceleration and the
    potential, and the circular velocity sqrt(max(0, -R a_R))."""
    radii: np.ndarray
    a_R: np.ndarray
    a_n: np.ndarray
    potential: np.ndarray
    v_c: np.ndarray
    field: Field             # the samples behind the means, ring-major


def _vec3(v):
    return (C.c_double * 3)(*(float(x) for x in v))


def field_rings(radii, *, axis=(0.0, 1.0, 0.0), center=(0.0, 0.0, 0.0), n_phi: int = 16) -> np.ndarray:
    """nb_field_rings: (len(radii) * n_phi, 3) float32 points, n_phi evenly spaced on each ring of radius
    radii[i] about `axis` through `center`, ring-major."""
    r = np.ascontiguousarray(np.atleast_1d(radii), dtype=np.float64)
    out = np.empty((r.shape[0] * max(int(n_phi), 0), 3), dtype=np.float32)
    check(_lib.lib().nb_field_rings(_vec3(center), _vec3(axis), r.ctypes.data_as(C.POINTER(C.c_double)), r.shape[0],
                                    int(n_phi), out.ctypes.data))
    return out


def _field(call, handle, points, accel, potential) -> Field:
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    flags = (_lib.NB_FIELD_ACCEL if accel else 0) | (_lib.NB_FIELD_POTENTIAL if potential else 0)
    out = np.zeros(pts.shape[0], dtype=_lib.FIELD_SAMPLE_DTYPE)
    st = _lib.nb_field_stats()
    check(call(handle, pts.ctypes.data, pts.shape[0], flags, out.ctypes.data, C.byref(st)))
    return Field(out["acc"].copy(), out["potential"].copy(), out["coincident"].copy(), int(st.step_num), int(st.n),
                 int(st.nonfinite), int(st.points), int(st.nonfinite_points), int(st.flags), int(st.launches))


def _circular_velocity(call, handle, radii, axis, center, n_phi, potential) -> RingMeans:
    r = np.ascontiguousarray(np.atleast_1d(radii), dtype=np.float64)
    pts = field_rings(r, axis=axis, center=center, n_phi=n_phi)
    f = _field(call, handle, pts, True, potential)
    samples = np.zeros(pts.shape[0], dtype=_lib.FIELD_SAMPLE_DTYPE)
    samples["acc"], samples["potential"] = f.acc, f.potential
    out = np.zeros(r.shape[0], dtype=_lib.FIELD_RING_DTYPE)
    check(_lib.lib().nb_field_ring_means(_vec3(center), _vec3(axis), r.ctypes.data_as(C.POINTER(C.c_double)),
                                         r.shape[0], int(n_phi), pts.ctypes.data, samples.ctypes.data,
                                         out.ctypes.data))
    return RingMeans(r, out["a_R"].copy(), out["a_n"].copy(), out["potential"].copy(), out["v_c"].copy(), f)


@dataclass(frozen=True)
class TidalField:
    """nb_tidal_sample[M] + nb_tidal_stats (include/nbody.h "Tidal tensor probes"; no reference counterpart): the
    exact tidal tensor T_ab = d acc_a / d x_b of the state read_particles would return, at M points."""
    tensor: np.ndarray       # (M, 3, 3) float64, symmetric
    coincident: np.ndarray   # (M,) uint32: bodies at the point itself, left out of every sum
    step_num: int
    n: int
    nonfinite: int           # bodies left out, as diagnostics() counts them
    points: int
    nonfinite_points: int
    launches: int

    @property
    def trace(self) -> np.ndarray:
        """(M,): the divergence of the acceleration, T_xx + T_yy + T_zz."""
        return self.tensor[:, 0, 0] + self.tensor[:, 1, 1] + self.tensor[:, 2, 2]

    @functools.cached_property
    def _eigen_cache(self):
        """(eigenvalues, eigenvectors), computed once per object: one nb_shape_eigen call per finite sample."""
        lam = np.full((self.tensor.shape[0], 3), np.nan)
        axes = np.full((self.tensor.shape[0], 3, 3), np.nan)
        eig, DP = _lib.lib().nb_shape_eigen, C.POINTER(C.c_double)
        t6, l3, a9 = (C.c_double * 6)(), (C.c_double * 3)(), (C.c_double * 9)()
        for i, t in enumerate(self.tensor):
            if not np.isfinite(t).all():
                continue
            t6[:] = [t[0, 0], t[0, 1], t[0, 2], t[1, 1], t[1, 2], t[2, 2]]  # nb_shape_eigen's order
            check(eig(C.cast(t6, DP), C.cast(l3, DP), C.cast(a9, DP)))
            lam[i], axes[i] = list(l3), np.array(list(a9)).reshape(3, 3)
        return lam, axes

    def eigenvalues(self) -> np.ndarray:
        """(M, 3), descending (nb_shape_eigen); NaN for a point without a finite tensor.  Positive stretches,
        negative compresses."""
        return self._eigen_cache[0].copy()

    def eigenvectors(self) -> np.ndarray:
        """(M, 3, 3): row k of sample i is the unit eigenvector of eigenvalues()[i, k], with nb_shape_eigen's sign."""
        return self._eigen_cache[1].copy()

    def compressive_axes(self) -> np.ndarray:
        """(M,) int: the count of negative eigenvalues, 0 to 3 -- the cosmic-web class of the point (-1 where the
        tensor is not finite)."""
        lam = self.eigenvalues()
        return np.where(np.isnan(lam).any(axis=1), -1, (lam < 0).sum(axis=1))


@dataclass(frozen=True)
class DiscFrequencies:
    """Per ring of field_rings(): the angular, epicyclic and vertical frequencies of a disc from the force and its
    gradient (nb_field_ring_means, nb_tidal_ring_means).  omega2 = -a_R / R, kappa2 = -T_RR + 3 omega2 (= R dOmega^2/dR
    + 4 Omega^2, for any central force law), nu2 = -T_nn; omega, kappa and nu are their roots, NaN where the square
    is negative."""
    radii: np.ndarray
    omega2: np.ndarray
    kappa2: np.ndarray
    nu2: np.ndarray
    v_c: np.ndarray
    t_RR: np.ndarray
    t_pp: np.ndarray
    t_nn: np.ndarray
    t_Rn: np.ndarray
    rings: "RingMeans"       # the field's ring means behind omega2 and v_c
    tidal: TidalField        # the tidal samples behind the rest, ring-major

    @staticmethod
    def _root(x):
        with np.errstate(invalid="ignore"):
            return np.where(x >= 0, np.sqrt(np.where(x >= 0, x, 0.0)), np.nan)

    @property
    def omega(self) -> np.ndarray:
        return self._root(self.omega2)

    @property
    def kappa(self) -> np.ndarray:
        return self._root(self.kappa2)

    @property
    def nu(self) -> np.ndarray:
        return self._root(self.nu2)

    def _crossings(self, f, level):
        d = f - level
        out = []
        for i in range(len(d)):
            if d[i] == 0.0:  # on a ring
                out.append(self.radii[i])
            elif i + 1 < len(d) and d[i] * d[i + 1] < 0.0:  # (False with a NaN on either side)
                out.append(self.radii[i] + d[i] / (d[i] - d[i + 1]) * (self.radii[i + 1] - self.radii[i]))
        return np.array(out, dtype=np.float64)

    def resonances(self, pattern_speed: float, m: int = 2) -> dict:
        """The radii where a pattern of speed `pattern_speed` (DiscModes.pattern_speed) and m arms resonates with
        the disc: "corotation" (Omega = Omega_p), "inner_lindblad" (Omega - kappa / m = Omega_p) and
        "outer_lindblad" (Omega + kappa / m = Omega_p), each an array (empty where the curve never crosses).
        Found by linear interpolation between the neighbouring rings where the sign of the difference changes: as
        fine as the rings, no finer.  Rings where a frequency is NaN are not crossed."""
        om, ka = self.omega, self.kappa
        return {"corotation": self._crossings(om, pattern_speed),
                "inner_lindblad": self._crossings(om - ka / m, pattern_speed),
                "outer_lindblad": self._crossings(om + ka / m, pattern_speed)}


def _tidal_tensor(call, handle, points) -> TidalField:
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    out = np.zeros(pts.shape[0], dtype=_lib.TIDAL_SAMPLE_DTYPE)
    st = _lib.nb_tidal_stats()
    check(call(handle, pts.ctypes.data, pts.shape[0], out.ctypes.data, C.byref(st)))
    t = out["tensor"]
    tensor = t[:, [0, 3, 4, 3, 1, 5, 4, 5, 2]].reshape(-1, 3, 3)  # xx, yy, zz, xy, xz, yz -> symmetric rows
    return TidalField(tensor, out["coincident"].copy(), int(st.step_num), int(st.n), int(st.nonfinite),
                      int(st.points), int(st.nonfinite_points), int(st.launches))


def _disc_frequencies(field_call, tidal_call, handle, radii, axis, center, n_phi) -> DiscFrequencies:
    cv = _circular_velocity(field_call, handle, radii, axis, center, n_phi, False)
    r = cv.radii
    pts = field_rings(r, axis=axis, center=center, n_phi=n_phi)
    t = _tidal_tensor(tidal_call, handle, pts)
    samples = np.zeros(pts.shape[0], dtype=_lib.TIDAL_SAMPLE_DTYPE)
    samples["tensor"] = t.tensor.reshape(-1, 9)[:, [0, 4, 8, 1, 2, 5]]
    rings = np.zeros(r.shape[0], dtype=_lib.FIELD_RING_DTYPE)
    rings["a_R"], rings["a_n"], rings["potential"], rings["v_c"] = cv.a_R, cv.a_n, cv.potential, cv.v_c
    out = np.zeros(r.shape[0], dtype=_lib.TIDAL_RING_DTYPE)
    check(_lib.lib().nb_tidal_ring_means(_vec3(center), _vec3(axis), r.ctypes.data_as(C.POINTER(C.c_double)),
                                         r.shape[0], int(n_phi), pts.ctypes.data, samples.ctypes.data,
                                         rings.ctypes.data, out.ctypes.data))
    return DiscFrequencies(r, out["omega2"].copy(), out["kappa2"].copy(), out["nu2"].copy(), cv.v_c,
                           out["t_RR"].copy(), out["t_pp"].copy(), out["t_nn"].copy(), out["t_Rn"].copy(), cv, t)


@dataclass(frozen=True)
class OrbitStats:
    """nb_orbit_stats: what an orbits() call measured."""
    step_num: int
    n: int
    nonfinite: int           # bodies left out, as diagnostics() counts them
    tracers: int
    nonfinite_tracers: int   # tracers that started non-finite: NaN in every record
    records: int
    pair_launches: int       # pair launches in all: evaluations x bands
    flags: int


@dataclass(frozen=True)
class Orbits:
    """nb_orbit_sample[R][M] + nb_orbit_stats (include/nbody.h "Orbits"; no reference counterpart): M test particles
    integrated through the frozen field of the state read_particles would return, the pattern at rest (omega = 0) or
    turning rigidly about `axis` through `center`.  Positions and velocities are inertial; with energy=True `energy`
    is the Jacobi integral (the plain energy for omega = 0), otherwise it and `potential` are NaN."""
    pos: np.ndarray          # (R, M, 3) float64
    vel: np.ndarray          # (R, M, 3) float64
    potential: np.ndarray    # (R, M) float64
    energy: np.ndarray       # (R, M) float64
    step: np.ndarray         # (R,) uint64: step0 + k of every record
    time: np.ndarray         # (R,) float64: (double)(step0 + k) * dt
    coincident: np.ndarray   # (M,) uint32: bodies at a tracer's point, summed over its evaluations
    stats: OrbitStats
    dt: float
    omega: float
    axis: np.ndarray
    center: np.ndarray

    def in_pattern_frame(self) -> np.ndarray:
        """(R, M, 3): the positions in the frame that turns with the pattern -- each record turned back by its
        theta_k about `axis` through `center`, with the phases of nb_orbit_phase the device used."""
        if self.omega == 0.0:
            return self.pos.copy()
        n, e1, e2 = map_frame(self.axis)
        out = np.empty_like(self.pos)
        c, s_ = C.c_double(), C.c_double()
        for r, k in enumerate(self.step):
            check(_lib.lib().nb_orbit_phase(self.omega, self.dt, int(k), C.byref(c), C.byref(s_)))
            d = self.pos[r] - self.center
            a, b, l = d @ e1, d @ e2, d @ n
            ar, br = a * c.value + b * s_.value, b * c.value - a * s_.value
            out[r] = self.center + (ar[:, None] * e1 + br[:, None] * e2) + l[:, None] * n
        return out

    def energy_range(self) -> np.ndarray:
        """(M,): max - min of `energy` over the records, per tracer (NaN without energy=True)."""
        return self.energy.max(axis=0) - self.energy.min(axis=0)

    def final(self):
        """(pos, vel, step): the last record and its step number -- what a continuing call takes as pos, vel and
        step0.  The continuation is exact when this call's `steps` is a multiple of its `every`."""
        return self.pos[-1].copy(), self.vel[-1].copy(), int(self.step[-1])


def _orbits(call, handle, pos, vel, dt, steps, every, energy, omega, axis, center, accel_scale, step0) -> Orbits:
    x = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
    v = np.ascontiguousarray(vel, dtype=np.float64).reshape(-1, 3)
    if x.shape != v.shape:
        raise ValueError(f"orbits: pos {x.shape} and vel {v.shape} differ")
    for name, val in (("steps", steps), ("every", every)):
        if not 0 <= int(val) <= 0xFFFFFFFF:
            raise ValueError(f"orbits: {name} = {val} is not a 32-bit count")
    p = _lib.nb_orbit_params()
    p.dt, p.step0, p.steps, p.every = float(dt), int(step0), int(steps), int(every)
    p.flags, p.reserved = (_lib.NB_ORBIT_ENERGY if energy else 0), 0
    p.accel_scale, p.omega = float(accel_scale), float(omega)
    for k in range(3):
        p.axis[k], p.center[k] = float(axis[k]), float(center[k])
    m = x.shape[0]
    records = int(_lib.lib().nb_orbit_records(p.steps, p.every))
    # (the call refuses what it does not take, before it writes)
    big = m > _lib.NB_ORBIT_MAX_TRACERS or records * m > _lib.NB_ORBIT_MAX_SAMPLES
    tracks = np.zeros((0 if big else records, m), dtype=_lib.ORBIT_SAMPLE_DTYPE)
    coincident = np.zeros(m, dtype=np.uint32)
    st = _lib.nb_orbit_stats()
    check(call(handle, C.byref(p), x.ctypes.data, v.ctypes.data, m, tracks.ctypes.data, coincident.ctypes.data,
               C.byref(st)))
    ks = np.array([k for k in range(p.steps + 1) if k % p.every == 0 or k == p.steps], dtype=np.uint64)
    step = ks + np.uint64(p.step0)
    stats = OrbitStats(int(st.step_num), int(st.n), int(st.nonfinite), int(st.tracers), int(st.nonfinite_tracers),
                       int(st.records), int(st.pair_launches), int(st.flags))
    return Orbits(tracks["pos"].copy(), tracks["vel"].copy(), tracks["potential"].copy(), tracks["energy"].copy(),
                  step, step.astype(np.float64) * p.dt, coincident, stats, float(p.dt), float(p.omega),
                  np.array(list(p.axis)), np.array(list(p.center)))


@dataclass(frozen=True)
class OrbitSectionStats:
    """nb_orbit_section_stats: what an orbit_sections() call measured."""
    orbit: OrbitStats
    crossings: int    # all crossings of all tracers
    stored: int       # those that found room
    overflowed: int   # tracers with more crossings than max_crossings


_SUMMARY_FIELDS = ("r2_min", "r2_max", "R2_min", "R2_max", "h_max", "lz_min", "lz_max", "first_peri", "last_peri",
                   "pericentres", "apocentres", "plane_ups", "winding_pattern", "winding_inertial")


@dataclass(frozen=True)
class OrbitSections:
    """nb_orbit_crossing[M][K] + nb_orbit_summary[M] (include/nbody.h "Orbit sections"; no reference counterpart):
    the states of M tracers interpolated onto a plane of the pattern frame -- a surface of section -- and a running
    summary per tracer, both taken inside the orbit's step kernel.  xi = (a', b', l) is the position and eta the
    velocity the turning pattern sees, in the frame of map_frame(axis) about `center`."""
    orbits: Orbits           # the recorded states of the same call
    count: np.ndarray        # (M,) uint32: all crossings of a tracer
    stored: np.ndarray       # (M,) uint32: min(count, K)
    xi: np.ndarray           # (M, K, 3) float64
    eta: np.ndarray          # (M, K, 3) float64
    time: np.ndarray         # (M, K) float64
    step: np.ndarray         # (M, K) uint64: the step the bracket began at
    valid: np.ndarray        # (M, K) bool: slot j < stored
    summary: np.ndarray      # (M,) ORBIT_SUMMARY_DTYPE
    stats: OrbitSectionStats

    def __getattr__(self, name):
        if name in _SUMMARY_FIELDS and "summary" in self.__dict__:
            return self.summary[name]
        raise AttributeError(name)

    @property
    def r_min(self) -> np.ndarray:
        return np.sqrt(self.summary["r2_min"])

    @property
    def r_max(self) -> np.ndarray:
        return np.sqrt(self.summary["r2_max"])

    def points(self, coord: int = 0, vel: int = 0):
        """(xi[coord], eta[vel]) of every stored crossing, flattened: the two arrays of a scatter plot."""
        return self.xi[..., coord][self.valid], self.eta[..., vel][self.valid]

    def radial_period(self) -> np.ndarray:
        """(M,): (last_peri - first_peri) dt / (pericentres - 1); NaN below two pericentres."""
        n = self.summary["pericentres"].astype(np.int64)
        span = (self.summary["last_peri"].astype(np.float64) - self.summary["first_peri"].astype(np.float64))
        with np.errstate(all="ignore"):
            return np.where(n >= 2, span * self.orbits.dt / np.maximum(n - 1, 1), np.nan)

    def frequency_ratio(self) -> np.ndarray:
        """(M,): winding_pattern / pericentres -- turns about the pattern's axis per radial oscillation (NaN
        without a pericentre)."""
        n = self.summary["pericentres"].astype(np.float64)
        with np.errstate(all="ignore"):
            return np.where(n > 0, self.summary["winding_pattern"] / np.where(n > 0, n, 1.0), np.nan)

    def merge(self, other: "OrbitSections") -> "OrbitSections":
        """This run followed by `other`, its continuation from orbits.final(): the counts added, the stored
        crossings concatenated, the summaries combined by nb_orbit_summary_merge.  `.orbits` is the continuation's."""
        m = self.count.shape[0]
        if other.count.shape[0] != m:
            raise ValueError("merge: the two runs have different tracers")
        summary = np.zeros(m, dtype=_lib.ORBIT_SUMMARY_DTYPE)
        a, b = np.ascontiguousarray(self.summary), np.ascontiguousarray(other.summary)
        size = _lib.ORBIT_SUMMARY_DTYPE.itemsize
        for i in range(m):
            check(_lib.lib().nb_orbit_summary_merge(a.ctypes.data + i * size, b.ctypes.data + i * size,
                                                    summary.ctypes.data + i * size))
        k = self.xi.shape[1] + other.xi.shape[1]
        rec = np.zeros((m, k), dtype=_lib.ORBIT_CROSSING_DTYPE)
        stored = np.zeros(m, dtype=np.uint32)
        for i in range(m):
            rows = np.concatenate([self._records()[i, :self.stored[i]], other._records()[i, :other.stored[i]]])
            rec[i, :rows.shape[0]] = rows
            stored[i] = rows.shape[0]
        count = self.count + other.count
        valid = np.arange(k)[None, :] < stored[:, None]
        stats = OrbitSectionStats(other.stats.orbit, int(count.sum()), int(stored.sum()), int((count > stored).sum()))
        return OrbitSections(other.orbits, count, stored, rec["xi"].copy(), rec["eta"].copy(), rec["time"].copy(),
                             rec["step"].copy(), valid, summary, stats)

    def _records(self) -> np.ndarray:
        rec = np.zeros(self.time.shape, dtype=_lib.ORBIT_CROSSING_DTYPE)
        rec["xi"], rec["eta"], rec["time"], rec["step"] = self.xi, self.eta, self.time, self.step
        return rec


def _orbit_sections(call, handle, pos, vel, dt, steps, normal, offset, direction, max_crossings, every, energy, omega,
                    axis, center, accel_scale, step0) -> OrbitSections:
    x = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
    v = np.ascontiguousarray(vel, dtype=np.float64).reshape(-1, 3)
    if x.shape != v.shape:
        raise ValueError(f"orbit_sections: pos {x.shape} and vel {v.shape} differ")
    every = steps if every is None else every
    for name, val in (("steps", steps), ("every", every), ("max_crossings", max_crossings)):
        if not 0 <= int(val) <= 0xFFFFFFFF:
            raise ValueError(f"orbit_sections: {name} = {val} is not a 32-bit count")
    if not -0x80000000 <= int(direction) <= 0x7FFFFFFF:
        raise ValueError(f"orbit_sections: direction = {direction}")
    p = _lib.nb_orbit_params()
    p.dt, p.step0, p.steps, p.every = float(dt), int(step0), int(steps), int(every)
    p.flags, p.reserved = (_lib.NB_ORBIT_ENERGY if energy else 0), 0
    p.accel_scale, p.omega = float(accel_scale), float(omega)
    s = _lib.nb_orbit_section_params()
    for k in range(3):
        p.axis[k], p.center[k], s.normal[k] = float(axis[k]), float(center[k]), float(normal[k])
    s.offset, s.direction, s.max_crossings = float(offset), int(direction), int(max_crossings)
    m, cap = x.shape[0], int(max_crossings)
    records = int(_lib.lib().nb_orbit_records(p.steps, p.every))
    # (the call refuses what it does not take, before it writes)
    big = (m > _lib.NB_ORBIT_MAX_TRACERS or records * m > _lib.NB_ORBIT_MAX_SAMPLES
           or m * cap > _lib.NB_ORBIT_SECTION_MAX_CROSSINGS)
    tracks = np.zeros((0 if big else records, m), dtype=_lib.ORBIT_SAMPLE_DTYPE)
    rec = np.zeros((m, 0 if big else cap), dtype=_lib.ORBIT_CROSSING_DTYPE)
    coincident = np.zeros(m, dtype=np.uint32)
    count = np.zeros(m, dtype=np.uint32)
    summary = np.zeros(m, dtype=_lib.ORBIT_SUMMARY_DTYPE)
    st = _lib.nb_orbit_section_stats()
    check(call(handle, C.byref(p), C.byref(s), x.ctypes.data, v.ctypes.data, m, tracks.ctypes.data,
               coincident.ctypes.data, rec.ctypes.data if rec.size else None, count.ctypes.data, summary.ctypes.data,
               C.byref(st)))
    ks = np.array([k for k in range(p.steps + 1) if k % p.every == 0 or k == p.steps], dtype=np.uint64)
    step = ks + np.uint64(p.step0)
    so = st.orbit
    ostats = OrbitStats(int(so.step_num), int(so.n), int(so.nonfinite), int(so.tracers), int(so.nonfinite_tracers),
                        int(so.records), int(so.pair_launches), int(so.flags))
    orbits = Orbits(tracks["pos"].copy(), tracks["vel"].copy(), tracks["potential"].copy(), tracks["energy"].copy(),
                    step, step.astype(np.float64) * p.dt, coincident, ostats, float(p.dt), float(p.omega),
                    np.array(list(p.axis)), np.array(list(p.center)))
    stored = np.minimum(count, np.uint32(cap)).astype(np.uint32)
    valid = np.arange(cap)[None, :] < stored[:, None]
    return OrbitSections(orbits, count, stored, rec["xi"].copy(), rec["eta"].copy(), rec["time"].copy(),
                         rec["step"].copy(), valid, summary,
                         OrbitSectionStats(ostats, int(st.crossings), int(st.stored), int(st.overflowed)))


@dataclass(frozen=True)
class OrbitStabilityStats:
    """nb_orbit_stability_stats: what an orbit_stability() call measured."""
    orbit: OrbitStats
    renorms: int        # renormalisations of all vectors of all tracers
    deviations: int     # D
    renorm_log2: int


@dataclass(frozen=True)
class OrbitStability:
    """nb_orbit_deviation[R][M][D] + nb_orbit_growth[M][D] (include/nbody.h "Orbit stability"; no reference
    counterpart): D deviation vectors per tracer carried along the orbits by the tangent map of the step.  The vector
    of record r is dev[r] * 2^log2[r], dev = (dx, dv).  Norms are Euclidean over the six components in the state's
    own units."""
    orbits: Orbits           # the recorded states of the same call: orbits()'s, bit for bit
    dev: np.ndarray          # (R, M, D, 6) float64
    log2: np.ndarray         # (R, M, D) int64
    growth: np.ndarray       # (M, D) ORBIT_GROWTH_DTYPE: peak_log2, peak_step, renorms
    dev0: np.ndarray         # (M, D, 6) float64: the vectors the call began with ...
    log2_0: np.ndarray       # (M, D) int64: ... and their exponents
    steps: int
    every: int
    stats: OrbitStabilityStats

    def _derive(self):
        r, m, d = self.log2.shape
        dev0 = np.zeros((m, d), dtype=_lib.ORBIT_DEVIATION_DTYPE)
        dev0["d"], dev0["log2"] = self.dev0, self.log2_0
        devs = np.zeros((r, m, d), dtype=_lib.ORBIT_DEVIATION_DTYPE)
        devs["d"], devs["log2"] = self.dev, self.log2
        lg, ly = np.empty((r, m, d)), np.empty((r, m, d))
        sa, ga = np.empty((r, m)), np.empty((r, m))
        check(_lib.lib().nb_orbit_stability_derive(self.orbits.dt, self.steps, self.every, m, d, dev0.ctypes.data,
                                                   devs.ctypes.data, lg.ctypes.data, ly.ctypes.data, sa.ctypes.data,
                                                   ga.ctypes.data))
        return lg, ly, sa, ga

    def log_growth(self) -> np.ndarray:
        """(R, M, D): ln(|delta_k| / |delta_0|) of every record (nb_orbit_stability_derive)."""
        return self._derive()[0]

    def lyapunov_curve(self) -> np.ndarray:
        """(R, M, D): the finite-time exponent log_growth / (k dt) of every record; NaN at k = 0."""
        return self._derive()[1]

    def lyapunov(self) -> np.ndarray:
        """(M, D): the exponent at the last record."""
        return self._derive()[1][-1]

    def sali(self) -> np.ndarray:
        """(R, M): min(|u1 + u2|, |u1 - u2|) of the unit vectors of vectors 0 and 1; NaN with D < 2."""
        return self._derive()[2]

    def gali2(self) -> np.ndarray:
        """(R, M): |u1 ^ u2| of the same two."""
        return self._derive()[3]

    def chaotic(self, sali_below: float = 1e-8) -> np.ndarray:
        """(M,) bool: the last record's SALI is below `sali_below` (a NaN is not)."""
        with np.errstate(invalid="ignore"):
            return self.sali()[-1] < float(sali_below)

    def final(self):
        """(pos, vel, dev, log2, step): the last record -- what a continuing call takes as pos, vel, deviations,
        log2_0 and step0.  The continuation is exact when this call's `steps` is a multiple of its `every`."""
        pos, vel, step = self.orbits.final()
        return pos, vel, self.dev[-1].copy(), self.log2[-1].copy(), step


def _default_deviations(count: int) -> np.ndarray:
    """(count, 6): orthonormal vectors from numpy.random.default_rng(0) (QR of a 6 x 6 normal matrix)."""
    q, _ = np.linalg.qr(np.random.default_rng(0).standard_normal((6, 6)))
    return np.ascontiguousarray(q.T[:count])


def _orbit_stability(call, handle, pos, vel, dt, steps, deviations, renorm_log2, every, log2_0, omega, axis, center,
                     accel_scale, step0) -> OrbitStability:
    x = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
    v = np.ascontiguousarray(vel, dtype=np.float64).reshape(-1, 3)
    if x.shape != v.shape:
        raise ValueError(f"orbit_stability: pos {x.shape} and vel {v.shape} differ")
    m = x.shape[0]
    every = steps if every is None else every
    if np.ndim(deviations) == 0:
        d = int(deviations)
        if not 0 <= d <= 0xFFFFFFFF:
            raise ValueError(f"orbit_stability: deviations = {deviations} is not a 32-bit count")
        vec = np.broadcast_to(_default_deviations(min(d, 6)), (m, min(d, 6), 6))
    else:
        vec = np.asarray(deviations, dtype=np.float64)
        if vec.ndim != 3 or vec.shape[0] != m or vec.shape[2] != 6:
            raise ValueError(f"orbit_stability: deviations {vec.shape} are not ({m}, D, 6)")
        d = vec.shape[1]
    for name, val in (("steps", steps), ("every", every), ("renorm_log2", renorm_log2)):
        if not 0 <= int(val) <= 0xFFFFFFFF:
            raise ValueError(f"orbit_stability: {name} = {val} is not a 32-bit count")
    p = _lib.nb_orbit_params()
    p.dt, p.step0, p.steps, p.every = float(dt), int(step0), int(steps), int(every)
    p.flags, p.reserved = 0, 0
    p.accel_scale, p.omega = float(accel_scale), float(omega)
    for k in range(3):
        p.axis[k], p.center[k] = float(axis[k]), float(center[k])
    sp = _lib.nb_orbit_stability_params(d, int(renorm_log2), 0)
    rows = vec.shape[1]  # (d itself when the call takes it)
    dev0 = np.zeros((m, rows), dtype=_lib.ORBIT_DEVIATION_DTYPE)
    dev0["d"] = vec
    dev0["log2"] = 0 if log2_0 is None else np.broadcast_to(np.asarray(log2_0, dtype=np.int64), (m, rows))
    records = int(_lib.lib().nb_orbit_records(p.steps, p.every))
    # (the call refuses what it does not take, before it reads or writes)
    big = (m > _lib.NB_ORBIT_MAX_TRACERS or rows != d or records * m * max(d, 1) > _lib.NB_ORBIT_MAX_SAMPLES)
    tracks = np.zeros((0 if big else records, m), dtype=_lib.ORBIT_SAMPLE_DTYPE)
    devs = np.zeros((0 if big else records, m, rows), dtype=_lib.ORBIT_DEVIATION_DTYPE)
    growth = np.zeros((m, rows), dtype=_lib.ORBIT_GROWTH_DTYPE)
    coincident = np.zeros(m, dtype=np.uint32)
    st = _lib.nb_orbit_stability_stats()
    check(call(handle, C.byref(p), C.byref(sp), x.ctypes.data, v.ctypes.data, m, dev0.ctypes.data, tracks.ctypes.data,
               coincident.ctypes.data, devs.ctypes.data, growth.ctypes.data, C.byref(st)))
    ks = np.array([k for k in range(p.steps + 1) if k % p.every == 0 or k == p.steps], dtype=np.uint64)
    step = ks + np.uint64(p.step0)
    so = st.orbit
    ostats = OrbitStats(int(so.step_num), int(so.n), int(so.nonfinite), int(so.tracers), int(so.nonfinite_tracers),
                        int(so.records), int(so.pair_launches), int(so.flags))
    orbits = Orbits(tracks["pos"].copy(), tracks["vel"].copy(), tracks["potential"].copy(), tracks["energy"].copy(),
                    step, step.astype(np.float64) * p.dt, coincident, ostats, float(p.dt), float(p.omega),
                    np.array(list(p.axis)), np.array(list(p.center)))
    return OrbitStability(orbits, devs["d"].copy(), devs["log2"].copy(), growth, dev0["d"].copy(), dev0["log2"].copy(),
                          int(p.steps), int(p.every),
                          OrbitStabilityStats(ostats, int(st.renorms), int(st.deviations), int(st.renorm_log2)))


def map_frame(axis):
    """nb_map_frame: (n_hat, e1, e2) of a map about `axis`, float64 arrays of 3.  n_hat is the axis normalised,
    e1 the coordinate axis of the smallest |n_k| made orthogonal to it, e2 = n_hat x e1: the vectors
    field_rings() lays its points with."""
    out = [(C.c_double * 3)() for _ in range(3)]
    check(_lib.lib().nb_map_frame(_vec3(axis), *out))
    return tuple(np.array(list(v), dtype=np.float64) for v in out)


def map_edges(lo: float, hi: float, cells: int) -> np.ndarray:
    """nb_map_edges: the cells + 1 edges of a map's window, lo + i (hi - lo) / cells with edges[cells] = hi."""
    out = np.empty(int(cells) + 1 if 1 <= int(cells) <= _lib.NB_MAP_MAX_SIDE else 1, dtype=np.float64)
    check(_lib.lib().nb_map_edges(float(lo), float(hi), int(cells), out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


MAP_PLANES = ("mass", "m_ua", "m_ub", "m_w", "m_w2", "m_u2")


@dataclass(frozen=True)
class ProjectedMap:
    """nb_sim_map's counts, planes and nb_map_stats (include/nbody.h "Projected maps"; no reference
    counterpart): the state read_particles would return, projected along n_hat onto the plane coordinates
    a (along e1, columns) and b (along e2, rows; row 0 is the smallest b) and summed per cell on the
    device.  counts: (H, W) uint32; the planes (H, W) float64, the five velocity planes None unless
    velocities were asked for.  w is the velocity along the line of sight, ua and ub in the plane."""
    counts: np.ndarray
    mass: np.ndarray
    m_ua: Optional[np.ndarray]   # sum m ua
    m_ub: Optional[np.ndarray]   # sum m ub
    m_w: Optional[np.ndarray]    # sum m w
    m_w2: Optional[np.ndarray]   # sum m w^2
    m_u2: Optional[np.ndarray]   # sum m |u|^2
    x_edges: np.ndarray          # W + 1
    y_edges: np.ndarray          # H + 1
    step_num: int
    n: int
    nonfinite: int
    binned_count: int
    outside_count: int
    binned_mass: float
    outside_mass: float
    total_mass: float            # nb_map_stats.mass: all finite bodies
    center: np.ndarray
    velocity: np.ndarray
    n_hat: np.ndarray
    e1: np.ndarray
    e2: np.ndarray
    flags: int
    max_count: int

    def _per_mass(self, plane):
        if plane is None:
            raise ValueError("this map was taken without velocities")
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.mass != 0.0, plane / self.mass, np.nan)

    @property
    def surface_density(self) -> np.ndarray:
        """mass over the cell's area (NaN in a cell without mass)."""
        area = np.outer(np.diff(self.y_edges), np.diff(self.x_edges))
        return np.where(self.mass != 0.0, self.mass / area, np.nan)

    @property
    def mean_w(self) -> np.ndarray:
        """Mass-weighted mean line-of-sight velocity per cell (NaN in a cell without mass)."""
        return self._per_mass(self.m_w)

    @property
    def mean_ua(self) -> np.ndarray:
        return self._per_mass(self.m_ua)

    @property
    def mean_ub(self) -> np.ndarray:
        return self._per_mass(self.m_ub)

    @property
    def sigma_w(self) -> np.ndarray:
        """Mass-weighted line-of-sight velocity dispersion per cell: sqrt(max(0, m_w2 / mass - mean_w^2))."""
        mean = self.mean_w
        return np.sqrt(np.maximum(self._per_mass(self.m_w2) - mean * mean, 0.0))


def _projected_map(call, handle, width, height, extent, axis, center, velocity, depth, velocities) -> ProjectedMap:
    p = _lib.nb_map_params()
    p.width, p.height = int(width), int(height)
    p.flags = _lib.NB_MAP_VELOCITY if velocities else 0
    if isinstance(center, str):
        if center != "com":
            raise ValueError('center is "com" or three coordinates')
        if velocity is not None:
            raise ValueError('center="com" brings its own velocity')
        p.flags |= _lib.NB_MAP_CENTER_COM
    else:
        velocity = (0.0, 0.0, 0.0) if velocity is None else velocity
        for k in range(3):
            p.center[k], p.velocity[k] = float(center[k]), float(velocity[k])
    x0, x1, y0, y1 = (float(v) for v in extent)
    p.x_range[0], p.x_range[1], p.y_range[0], p.y_range[1] = x0, x1, y0, y1
    p.depth_range[0], p.depth_range[1] = (-np.inf, np.inf) if depth is None else (float(depth[0]), float(depth[1]))
    for k in range(3):
        p.axis[k] = float(axis[k])
    ok = 1 <= p.width <= _lib.NB_MAP_MAX_SIDE and 1 <= p.height <= _lib.NB_MAP_MAX_SIDE and \
        p.width * p.height <= _lib.NB_MAP_MAX_CELLS
    h, w = (p.height, p.width) if ok else (1, 1)  # (the call refuses the sizes itself)
    nplanes = len(MAP_PLANES) if velocities else 1
    counts = np.empty((h, w), dtype=np.uint32)
    planes = np.empty((nplanes, h, w), dtype=np.float64)
    st = _lib.nb_map_stats()
    check(call(handle, C.byref(p), counts.ctypes.data, planes.ctypes.data, C.byref(st)))
    vec = lambda a: np.array(list(a), dtype=np.float64)  # noqa: E731
    rest = [planes[k] for k in range(1, nplanes)] if velocities else [None] * 5
    return ProjectedMap(counts, planes[0], *rest, map_edges(x0, x1, w), map_edges(y0, y1, h), int(st.step_num),
                        int(st.n), int(st.nonfinite), int(st.binned_count), int(st.outside_count),
                        float(st.binned_mass), float(st.outside_mass), float(st.mass), vec(st.center),
                        vec(st.velocity), vec(st.n_hat), vec(st.e1), vec(st.e2), int(st.flags), int(st.max_count))


def phase_quantity(name: str) -> int:
    """nb_phase_quantity: the id (NB_PHASE_Q_*) of the per-body quantity called `name`."""
    out = C.c_uint32()
    check(_lib.lib().nb_phase_quantity(str(name).encode(), C.byref(out)))
    return int(out.value)


def phase_quantities() -> tuple:
    """The names of the per-body quantities a phase map bins and sums, in the order of their ids
    (nb_phase_quantity_name)."""
    L = _lib.lib()
    return tuple(L.nb_phase_quantity_name(q).decode() for q in range(_lib.NB_PHASE_Q_COUNT))


def phase_edges(lo: float, hi: float, cells: int, log: bool = False) -> np.ndarray:
    """The cells + 1 edges of one side of a phase map: map_edges() (linear), or edges with a constant ratio from
    lo > 0 (radial_edges() up to its 256 bins, the same expression lo (hi / lo)^(k / cells) beyond)."""
    if not log:
        return map_edges(lo, hi, cells)
    if int(cells) <= _lib.NB_RADIAL_MAX_BINS:
        return radial_edges(lo, hi, cells, log=True)
    lo, hi, cells = float(lo), float(hi), int(cells)
    if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 < lo < hi):
        raise ValueError("log edges need finite 0 < lo < hi")
    out = lo * np.power(hi / lo, np.arange(cells + 1, dtype=np.float64) / cells)
    out[0], out[cells] = lo, hi
    return out


@dataclass(frozen=True)
class PhaseStats:
    """nb_phase_stats.  undefined_count: the bodies whose x, y or weight is not finite (they are among the
    outside_count); binned_count + outside_count + nonfinite == n."""
    step_num: int
    n: int
    nonfinite: int
    binned_count: int
    outside_count: int
    undefined_count: int
    binned_mass: float
    outside_mass: float
    total_mass: float            # nb_phase_stats.mass: all finite bodies
    center: np.ndarray
    velocity: np.ndarray
    n_hat: np.ndarray
    e1: np.ndarray
    e2: np.ndarray
    flags: int
    max_count: int
    x: str                       # the names of the three quantities; weight None without one
    y: str
    weight: Optional[str]


@dataclass(frozen=True)
class PhaseMap:
    """nb_phase_map_sim's counts, planes and nb_phase_stats (include/nbody.h "Phase maps"; no reference
    counterpart): the bodies of the state read_particles would return, binned on two per-body quantities --
    x along the columns, y along the rows, row 0 the smallest y -- and summed per cell on the device.
    counts: (H, W) uint32; mass (H, W) float64; m_q and m_q2, the sums of mass times the weight quantity and its
    square, None unless a weight was asked for."""
    counts: np.ndarray
    mass: np.ndarray
    m_q: Optional[np.ndarray]
    m_q2: Optional[np.ndarray]
    x_edges: np.ndarray          # W + 1
    y_edges: np.ndarray          # H + 1
    stats: PhaseStats

    def _per_mass(self, plane):
        if plane is None:
            raise ValueError("this phase map was taken without a weight")
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.mass != 0.0, plane / self.mass, np.nan)

    @property
    def mean_q(self) -> np.ndarray:
        """Mass-weighted mean of the weight quantity per cell (NaN in a cell without mass)."""
        return self._per_mass(self.m_q)

    @property
    def sigma_q(self) -> np.ndarray:
        """Mass-weighted dispersion of the weight quantity per cell: sqrt(max(0, m_q2 / mass - mean_q^2))."""
        mean = self.mean_q
        return np.sqrt(np.maximum(self._per_mass(self.m_q2) - mean * mean, 0.0))

    @property
    def density(self) -> np.ndarray:
        """mass per unit of x times y (NaN in a cell without mass; a cell with an infinite edge has density 0)."""
        area = np.outer(np.diff(self.y_edges), np.diff(self.x_edges))
        return np.where(self.mass != 0.0, self.mass / area, np.nan)

    def marginal_x(self) -> np.ndarray:
        """The mass per column: the distribution of x over the binned bodies."""
        return self.mass.sum(axis=0)

    def marginal_y(self) -> np.ndarray:
        """The mass per row: the distribution of y over the binned bodies."""
        return self.mass.sum(axis=1)


def _phase_side(what, edges, rng, cells, log):
    if edges is not None:
        if rng is not None:
            raise ValueError(f"give {what}_edges or {what}_range, not both")
        return np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
    if rng is None:
        raise ValueError(f"a phase map needs {what}_edges or {what}_range")
    return phase_edges(rng[0], rng[1], cells, log)


def _phase_map(call, handle, n, step_now, x, y, x_edges, y_edges, weight, values, axis, center, velocity,
               check_step) -> PhaseMap:
    p = _lib.nb_phase_params()
    names = (str(x), str(y), None if weight is None else str(weight))
    p.x, p.y = phase_quantity(names[0]), phase_quantity(names[1])
    p.q = _lib.NB_PHASE_Q_MASS if weight is None else phase_quantity(names[2])
    p.flags = 0 if weight is None else _lib.NB_PHASE_WEIGHT
    if isinstance(center, str):
        if center != "com":
            raise ValueError('center is "com", "density" or three coordinates')
        if velocity is not None:
            raise ValueError('center="com" brings its own velocity')
        p.flags |= _lib.NB_PHASE_CENTER_COM
    else:
        velocity = (0.0, 0.0, 0.0) if velocity is None else velocity
        for k in range(3):
            p.center[k], p.velocity[k] = float(center[k]), float(velocity[k])
    for k in range(3):
        p.axis[k] = float(axis[k])
    if len(x_edges) < 2 or len(y_edges) < 2:
        raise ValueError("a side of a phase map needs at least two edges")
    p.width, p.height = len(x_edges) - 1, len(y_edges) - 1
    dp = C.POINTER(C.c_double)
    p.x_edges, p.y_edges = x_edges.ctypes.data_as(dp), y_edges.ctypes.data_as(dp)
    if values is not None:
        values = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        if values.shape[0] != n:
            raise ValueError(f"values needs one entry per body ({n}), not {values.shape[0]}")
        p.values = values.ctypes.data_as(dp)
    # values in hand were read off the state as it is now unless the caller says otherwise (check_step: a step number)
    p.step_num = _lib.NB_PHASE_ANY_STEP if check_step is False else step_now if check_step is True else int(check_step)
    ok = 1 <= p.width <= _lib.NB_MAP_MAX_SIDE and 1 <= p.height <= _lib.NB_MAP_MAX_SIDE and \
        p.width * p.height <= _lib.NB_MAP_MAX_CELLS
    h, w = (p.height, p.width) if ok else (1, 1)  # (the call refuses the sizes itself)
    nplanes = 1 if weight is None else 3
    counts = np.empty((h, w), dtype=np.uint32)
    planes = np.empty((nplanes, h, w), dtype=np.float64)
    st = _lib.nb_phase_stats()
    check(call(handle, C.byref(p), counts.ctypes.data, planes.ctypes.data, C.byref(st)))
    vec = lambda a: np.array(list(a), dtype=np.float64)  # noqa: E731
    stats = PhaseStats(int(st.step_num), int(st.n), int(st.nonfinite), int(st.binned_count), int(st.outside_count),
                       int(st.undefined_count), float(st.binned_mass), float(st.outside_mass), float(st.mass),
                       vec(st.center), vec(st.velocity), vec(st.n_hat), vec(st.e1), vec(st.e2), int(st.flags),
                       int(st.max_count), *names)
    rest = [planes[1], planes[2]] if weight is not None else [None, None]
    return PhaseMap(counts, planes[0], *rest, x_edges, y_edges, stats)


FOF_NONE = _lib.NB_FOF_NONE


@dataclass(frozen=True)
class FofStats:
    """nb_fof_stats (include/nbody.h "Friends-of-friends groups")."""
    step_num: int
    n: int
    nonfinite: int
    components: int       # all of them, singletons included
    groups: int           # the catalogued ones
    grouped_bodies: int
    largest_count: int
    largest_label: int
    cells: tuple          # cells per axis that were used
    cell_side: float


@dataclass(frozen=True)
class FofGroups:
    """nb_sim_fof's partition and catalogue (include/nbody.h "Friends-of-friends groups"; no reference
    counterpart): bodies closer than `link` are friends, a group is a connected component of the friends
    graph of the state read_particles would return, its label the smallest body index in it.  labels and
    group_of: (n,) uint32, FOF_NONE for a non-finite body / a body of no catalogued group (labels None when
    not asked for).  rows: the catalogue, _lib.FOF_GROUP_DTYPE records in ascending label order -- the
    components with at least min_members bodies."""
    labels: Optional[np.ndarray]
    group_of: np.ndarray
    rows: np.ndarray
    link: float
    min_members: int
    stats: FofStats

    def _per_mass(self, a):
        with np.errstate(invalid="ignore", divide="ignore"):
            return a / (self.mass if a.ndim == 1 else self.mass[:, None])

    @property
    def label(self) -> np.ndarray:
        return self.rows["label"]

    @property
    def count(self) -> np.ndarray:
        return self.rows["count"]

    @property
    def mass(self) -> np.ndarray:
        return self.rows["mass"]

    @property
    def com(self) -> np.ndarray:
        """(groups, 3): sum m x / sum m."""
        return self._per_mass(self.rows["mx"])

    @property
    def velocity(self) -> np.ndarray:
        """(groups, 3): sum m v / sum m."""
        return self._per_mass(self.rows["mv"])

    @property
    def rms_radius(self) -> np.ndarray:
        """Mass-weighted rms distance of the members from com: sqrt(max(0, sum m |x|^2 / mass - |com|^2))."""
        c = self.com
        return np.sqrt(np.maximum(self._per_mass(self.rows["mr2"]) - (c * c).sum(axis=1), 0.0))

    @property
    def sigma(self) -> np.ndarray:
        """Mass-weighted 3-D velocity dispersion about the group's velocity."""
        v = self.velocity
        return np.sqrt(np.maximum(self._per_mass(self.rows["mv2"]) - (v * v).sum(axis=1), 0.0))

    def by_size(self) -> np.ndarray:
        """The rows' numbers by count, descending, ties by label (ascending)."""
        return np.lexsort((self.rows["label"], -self.rows["count"].astype(np.int64)))


def _fof_groups(call, handle, n, link, min_members, labels) -> FofGroups:
    p = _lib.nb_fof_params()
    p.link, p.flags, p.reserved = float(link), 0, 0
    mm = int(min_members)
    p.min_members = mm if 0 <= mm <= 0xFFFFFFFF else 0  # (the call refuses 0 itself)
    cap = n // mm if mm >= 1 else 0  # the most there can be
    lab = np.empty(n, dtype=np.uint32) if labels else None
    gof = np.empty(n, dtype=np.uint32)
    rows = np.zeros(cap, dtype=_lib.FOF_GROUP_DTYPE)
    st = _lib.nb_fof_stats()
    check(call(handle, C.byref(p), lab.ctypes.data if labels else None, gof.ctypes.data, rows.ctypes.data, cap,
               C.byref(st)))
    stats = FofStats(int(st.step_num), int(st.n), int(st.nonfinite), int(st.components), int(st.groups),
                     int(st.grouped_bodies), int(st.largest_count), int(st.largest_label),
                     tuple(int(c) for c in st.cells), float(st.cell_side))
    return FofGroups(lab, gof, rows[:stats.groups], float(link), mm, stats)


@dataclass(frozen=True)
class PhaseSpaceGroups(FofGroups):
    """nb_fof6_sim's partition and catalogue (include/nbody.h "Phase-space groups"; no reference counterpart):
    bodies are friends when (dx / link)^2 + (dv / vlink)^2 <= 1 and dx <= link, a group is a connected component.
    The fields and properties are FofGroups'; every group lies inside one group of fof_groups(link)."""
    vlink: float = float("nan")

    def parent_rows(self, parent: FofGroups) -> np.ndarray:
        """Per row, the catalogue row of `parent` -- a fof_groups(link) of the same step -- that holds it, or FOF_NONE
        when that group is not in the parent's catalogue: the parent's group_of at the row's label."""
        if parent.stats.step_num != self.stats.step_num:
            raise ValueError(f"parent_rows: the parent was made at step {parent.stats.step_num}, these groups at "
                             f"step {self.stats.step_num}")
        if parent.link != self.link:
            raise ValueError(f"parent_rows: the parent's link {parent.link} is not these groups' {self.link}")
        return parent.group_of[self.rows["label"].astype(np.int64)]


def _phase_space_groups(call, handle, n, link, vlink, min_members, labels) -> PhaseSpaceGroups:
    p = _lib.nb_fof6_params()
    p.link, p.vlink, p.flags, p.reserved = float(link), float(vlink), 0, 0
    mm = int(min_members)
    p.min_members = mm if 0 <= mm <= 0xFFFFFFFF else 0  # (the call refuses 0 itself)
    cap = n // mm if mm >= 1 else 0  # the most there can be
    lab = np.empty(n, dtype=np.uint32) if labels else None
    gof = np.empty(n, dtype=np.uint32)
    rows = np.zeros(cap, dtype=_lib.FOF_GROUP_DTYPE)
    st = _lib.nb_fof_stats()
    check(call(handle, C.byref(p), lab.ctypes.data if labels else None, gof.ctypes.data, rows.ctypes.data, cap,
               C.byref(st)))
    stats = FofStats(int(st.step_num), int(st.n), int(st.nonfinite), int(st.components), int(st.groups),
                     int(st.grouped_bodies), int(st.largest_count), int(st.largest_label),
                     tuple(int(c) for c in st.cells), float(st.cell_side))
    return PhaseSpaceGroups(lab, gof, rows[:stats.groups], float(link), mm, stats, float(vlink))


HOP_NONE = _lib.NB_HOP_NONE


@dataclass(frozen=True)
class HopStats:
    """nb_hop_stats (include/nbody.h "Density-peak groups")."""
    step_num: int
    n: int
    nonfinite: int
    counted: int
    outside: int          # counted bodies below density_min
    short_of_k: int
    peaks: int            # all groups, whatever their size
    groups: int           # the catalogued ones
    grouped_bodies: int
    boundaries: int       # label pairs
    boundary_pairs: int   # ordered body pairs taken
    largest_count: int
    largest_label: int


@dataclass(frozen=True)
class HopGroups:
    """nb_sim_hop's partition, catalogue and boundary table (include/nbody.h "Density-peak groups"; no
    reference counterpart): every body hops to the densest of its k_hop nearest neighbours until it reaches a
    density peak, whose body index is the group's label.  labels and group_of: (n,) uint32, HOP_NONE for a body
    of no group / of no catalogued group (labels None when not asked for); density: (n,) float64, knn_density's
    at k_density, or None.  rows: FofGroups' catalogue records in ascending label order, peak_density one per
    row.  boundaries: _lib.HOP_BOUNDARY_DTYPE records in ascending (a, b), one per pair of labels with
    neighbouring bodies -- `pairs` body pairs, `density` the largest mean density of a pair -- or None.
    regroup(saddle, peak) merges the groups across boundaries denser than `saddle` and drops the sets with no
    peak of at least `peak`."""
    labels: Optional[np.ndarray]
    group_of: np.ndarray
    density: Optional[np.ndarray]
    rows: np.ndarray
    peak_density: np.ndarray
    boundaries: Optional[np.ndarray]
    k: tuple              # (k_density, k_hop, k_merge)
    min_members: int
    density_min: float
    stats: HopStats

    _per_mass = FofGroups._per_mass
    label = FofGroups.label
    count = FofGroups.count
    mass = FofGroups.mass
    com = FofGroups.com
    velocity = FofGroups.velocity
    rms_radius = FofGroups.rms_radius
    sigma = FofGroups.sigma
    by_size = FofGroups.by_size

    def regroup(self, saddle: float, peak: float) -> "HopGroups":
        """nb_hop_regroup on this catalogue and boundary table: a HopGroups of the merged rows, labels and
        group_of mapped through the merge (HOP_NONE for a body of a set that is not viable), no boundaries."""
        if self.boundaries is None:
            raise ValueError("regroup: this HopGroups was made with boundaries=False")
        m = len(self.rows)
        rows = np.ascontiguousarray(self.rows)
        pk = np.ascontiguousarray(self.peak_density, dtype=np.float64)
        bnd = np.ascontiguousarray(self.boundaries)
        rp = _lib.nb_hop_regroup_params()
        rp.saddle, rp.peak, rp.flags, rp.reserved = float(saddle), float(peak), 0, 0
        merged = np.empty(m, dtype=np.uint32)
        out_rows = np.zeros(m, dtype=_lib.FOF_GROUP_DTYPE)
        out_peak = np.zeros(m, dtype=np.float64)
        cnt = C.c_size_t(0)
        check(_lib.lib().nb_hop_regroup(rows.ctypes.data, pk.ctypes.data, m, bnd.ctypes.data, len(bnd), C.byref(rp),
                                        merged.ctypes.data, out_rows.ctypes.data, out_peak.ctypes.data, m,
                                        C.byref(cnt)))
        out_rows, out_peak = out_rows[:cnt.value], out_peak[:cnt.value]
        # body -> raw row -> merged label -> merged row
        raw = self.group_of
        has = raw != HOP_NONE
        lab = np.full(raw.shape, HOP_NONE, dtype=np.uint32)
        lab[has] = merged[raw[has]]
        gof = np.full(raw.shape, HOP_NONE, dtype=np.uint32)
        ok = lab != HOP_NONE
        gof[ok] = np.searchsorted(out_rows["label"], lab[ok]).astype(np.uint32)
        big = int(np.lexsort((out_rows["label"], -out_rows["count"].astype(np.int64)))[0]) if len(out_rows) else -1
        stats = dataclasses.replace(
            self.stats, groups=len(out_rows), grouped_bodies=int(out_rows["count"].sum(dtype=np.uint64)),
            boundaries=0, boundary_pairs=0, largest_count=int(out_rows["count"][big]) if big >= 0 else 0,
            largest_label=int(out_rows["label"][big]) if big >= 0 else HOP_NONE)
        return HopGroups(lab if self.labels is not None else None, gof, self.density, out_rows, out_peak, None,
                         self.k, self.min_members, self.density_min, stats)


def _hop_groups(call, handle, n, k_density, k_hop, k_merge, min_members, density_min, labels, density,
                boundaries) -> HopGroups:
    p = _lib.nb_hop_params()
    u32 = lambda v: int(v) if 0 <= int(v) <= 0xFFFFFFFF else 0  # (the call refuses 0 itself)
    p.k_density, p.k_hop, p.k_merge, p.min_members = u32(k_density), u32(k_hop), u32(k_merge), u32(min_members)
    p.density_min = -np.inf if density_min is None else float(density_min)
    p.flags, p.reserved32, p.reserved = 0, 0, 0
    lab = np.empty(n, dtype=np.uint32) if labels else None
    gof = np.empty(n, dtype=np.uint32)
    den = np.empty(n, dtype=np.float64) if density else None
    st = _lib.nb_hop_stats()
    cap = n // 4 + 1
    bcap = 4 * cap if boundaries else 0
    for attempt in range(2):
        rows = np.zeros(cap, dtype=_lib.FOF_GROUP_DTYPE)
        peak = np.zeros(cap, dtype=np.float64)
        bnd = np.zeros(bcap, dtype=_lib.HOP_BOUNDARY_DTYPE) if boundaries else None
        check(call(handle, C.byref(p), lab.ctypes.data if labels else None, gof.ctypes.data,
                   den.ctypes.data if density else None, rows.ctypes.data, peak.ctypes.data, cap,
                   bnd.ctypes.data if boundaries else None, bcap, C.byref(st)))
        if int(st.groups) <= cap and (not boundaries or int(st.boundaries) <= bcap):
            break
        cap = max(cap, int(st.groups))  # once more, with the sizes the stats report
        bcap = max(bcap, int(st.boundaries)) if boundaries else 0
    stats = HopStats(int(st.step_num), int(st.n), int(st.nonfinite), int(st.counted), int(st.outside),
                     int(st.short_of_k), int(st.peaks), int(st.groups), int(st.grouped_bodies), int(st.boundaries),
                     int(st.boundary_pairs), int(st.largest_count), int(st.largest_label))
    return HopGroups(lab, gof, den, rows[:stats.groups], peak[:stats.groups],
                     bnd[:stats.boundaries] if boundaries else None, (int(k_density), int(k_hop), int(k_merge)),
                     int(min_members), float(p.density_min), stats)


BOUND_CONVERGED, BOUND_DISSOLVED = _lib.NB_BOUND_CONVERGED, _lib.NB_BOUND_DISSOLVED
BOUND_UNCONVERGED, BOUND_SKIPPED = _lib.NB_BOUND_UNCONVERGED, _lib.NB_BOUND_SKIPPED


@dataclass(frozen=True)
class BoundStats:
    """nb_bound_stats (include/nbody.h "Bound groups")."""
    step_num: int
    n: int
    nonfinite: int
    components: int
    groups: int
    grouped_bodies: int
    largest_count: int
    largest_label: int
    bound_groups: int     # analysed rows with a non-empty bound set
    bound_bodies: int
    dissolved: int
    unconverged: int
    skipped: int
    pairs: int            # pair terms evaluated
    rounds_max: int


@dataclass(frozen=True)
class BoundGroups:
    """nb_sim_bound's catalogue (include/nbody.h "Bound groups"; no reference counterpart): the
    friends-of-friends groups of the state read_particles would return, each unbound round by round in its own
    frame.  group_of: (n,) uint32, as FofGroups.  bound_of: (n,) uint32, the row for a body of the row's bound
    set, FOF_NONE otherwise; energy: (n,) float64, a body's energy in the last round it was active in, NaN for
    a body of no analysed group (both None when not asked for).  rows: _lib.BOUND_GROUP_DTYPE records in
    ascending label order; the sums are over the bound set."""
    group_of: np.ndarray
    bound_of: Optional[np.ndarray]
    energy: Optional[np.ndarray]
    rows: np.ndarray
    link: float
    min_members: int
    min_bound: int
    max_iter: int
    max_group: int
    stats: BoundStats

    def _per_mass(self, a):
        with np.errstate(invalid="ignore", divide="ignore"):
            return a / (self.mass if a.ndim == 1 else self.mass[:, None])

    @property
    def label(self) -> np.ndarray:
        return self.rows["label"]

    @property
    def count(self) -> np.ndarray:
        return self.rows["count"]

    @property
    def bound_count(self) -> np.ndarray:
        return self.rows["bound_count"]

    @property
    def status(self) -> np.ndarray:
        return self.rows["status"]

    @property
    def mass(self) -> np.ndarray:
        return self.rows["mass"]

    @property
    def com(self) -> np.ndarray:
        """(groups, 3): sum m x / sum m over the bound set (NaN for an empty one)."""
        return self._per_mass(self.rows["mx"])

    @property
    def velocity(self) -> np.ndarray:
        """(groups, 3): sum m v / sum m over the bound set."""
        return self._per_mass(self.rows["mv"])

    @property
    def bound_fraction(self) -> np.ndarray:
        """bound_count / count."""
        return self.rows["bound_count"] / self.rows["count"]

    @property
    def virial_ratio(self) -> np.ndarray:
        """2 K / |U| of the whole friends-of-friends group in round 1 (kinetic0, potential0): 1 in virial
        equilibrium, above 2 unbound as a whole; NaN where no round ran."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return 2.0 * self.rows["kinetic0"] / np.abs(self.rows["potential0"])

    def by_bound_mass(self) -> np.ndarray:
        """The rows' numbers by bound mass, descending, ties by label (ascending)."""
        return np.lexsort((self.rows["label"], -self.rows["mass"]))


def _bound_groups(call, handle, n, link, min_members, min_bound, max_iter, max_group, per_body) -> BoundGroups:
    p = _lib.nb_bound_params()
    mm = int(min_members)
    mb = mm if min_bound is None else int(min_bound)
    for name, v in (("min_members", mm), ("min_bound", mb), ("max_iter", max_iter), ("max_group", max_group)):
        if not 0 <= int(v) <= 0xFFFFFFFF:  # (the call itself refuses the zeros that mean nothing)
            raise ValueError(f"bound_groups: {name} = {v} is not a 32-bit count")
    p.link, p.flags, p.reserved32, p.reserved = float(link), 0, 0, 0
    p.min_members, p.min_bound, p.max_iter, p.max_group = mm, mb, int(max_iter), int(max_group)
    cap = n // mm if mm >= 1 else 0  # the most there can be
    gof = np.empty(n, dtype=np.uint32)
    bof = np.empty(n, dtype=np.uint32) if per_body else None
    en = np.empty(n, dtype=np.float64) if per_body else None
    rows = np.zeros(cap, dtype=_lib.BOUND_GROUP_DTYPE)
    st = _lib.nb_bound_stats()
    check(call(handle, C.byref(p), gof.ctypes.data, bof.ctypes.data if per_body else None,
               en.ctypes.data if per_body else None, rows.ctypes.data, cap, C.byref(st)))
    stats = BoundStats(int(st.step_num), int(st.n), int(st.nonfinite), int(st.components), int(st.groups),
                       int(st.grouped_bodies), int(st.largest_count), int(st.largest_label), int(st.bound_groups),
                       int(st.bound_bodies), int(st.dissolved), int(st.unconverged), int(st.skipped), int(st.pairs),
                       int(st.rounds_max))
    return BoundGroups(gof, bof, en, rows[:stats.groups], float(link), mm, mb, int(max_iter), int(max_group), stats)


KNN_NONE = _lib.NB_KNN_NONE


@dataclass(frozen=True)
class KnnStats:
    """nb_knn_stats (include/nbody.h "k-nearest-neighbour density")."""
    step_num: int
    n: int
    nonfinite: int
    counted: int
    degenerate: int       # counted bodies with at least k others at their own position: density +inf
    short_of_k: int       # the counted bodies when there are no more than k of them, else 0
    sum_rho: float
    sum_rho_x: np.ndarray
    sum_rho_v: np.ndarray
    sum_rho2: float
    peak_density: float
    peak_index: int


@dataclass(frozen=True)
class KnnDensity:
    """nb_sim_knn's per-body values and sums (include/nbody.h "k-nearest-neighbour density"; no reference
    counterpart).  For body i of the state read_particles would return: r2[i] the squared distance to its
    k-th nearest counted neighbour (ties by the smaller index), kth[i] that neighbour (KNN_NONE: none),
    mass_in[i] the mass of the k - 1 nearer ones, density[i] = mass_in / (4 pi / 3 r_k^3) (Casertano & Hut
    1985).  An array that was not asked for is None."""
    k: int
    r2: Optional[np.ndarray]
    kth: Optional[np.ndarray]
    mass_in: Optional[np.ndarray]
    density: Optional[np.ndarray]
    stats: KnnStats

    @property
    def r_k(self) -> Optional[np.ndarray]:
        """sqrt(r2): the distance to the k-th neighbour."""
        return None if self.r2 is None else np.sqrt(self.r2)

    def _per_rho(self, a) -> np.ndarray:
        s = self.stats.sum_rho
        return a / s if s != 0.0 else np.full(3, np.nan)

    @property
    def center(self) -> np.ndarray:
        """The density centre sum rho x / sum rho (NaN when sum rho is 0)."""
        return self._per_rho(self.stats.sum_rho_x)

    @property
    def center_velocity(self) -> np.ndarray:
        """sum rho v / sum rho (NaN when sum rho is 0)."""
        return self._per_rho(self.stats.sum_rho_v)

    @property
    def peak_index(self) -> int:
        return self.stats.peak_index

    @property
    def peak_density(self) -> float:
        return self.stats.peak_density


def _knn_stats(st) -> KnnStats:
    return KnnStats(int(st.step_num), int(st.n), int(st.nonfinite), int(st.counted), int(st.degenerate),
                    int(st.short_of_k), float(st.sum_rho), np.array(st.sum_rho_x[:], dtype=np.float64),
                    np.array(st.sum_rho_v[:], dtype=np.float64), float(st.sum_rho2), float(st.peak_density),
                    int(st.peak_index))


def _knn_density(call, handle, n, k, density, neighbours) -> KnnDensity:
    p = _lib.nb_knn_params()
    kk = int(k)
    p.k, p.flags, p.reserved = (kk if 0 <= kk <= 0xFFFFFFFF else 0), 0, 0  # (the call refuses 0 itself)
    r2 = np.empty(n, dtype=np.float64) if neighbours else None
    kth = np.empty(n, dtype=np.uint32) if neighbours else None
    mass_in = np.empty(n, dtype=np.float64) if density else None
    rho = np.empty(n, dtype=np.float64) if density else None
    ptr = lambda a: None if a is None else a.ctypes.data
    st = _lib.nb_knn_stats()
    check(call(handle, C.byref(p), ptr(r2), ptr(kth), ptr(mass_in), ptr(rho), C.byref(st)))
    return KnnDensity(kk, r2, kth, mass_in, rho, _knn_stats(st))


MST_NONE = _lib.NB_MST_NONE


@dataclass(frozen=True)
class MstStats:
    """nb_mst_stats (include/nbody.h "Minimum spanning tree")."""
    step_num: int
    n: int
    nonfinite: int
    edges: int
    rounds: int                   # the Boruvka rounds that ran
    components_after: np.ndarray  # (32,) uint32: the components after each round, 0 from `rounds` on
    d2_min: float
    d2_max: float
    lo: np.ndarray                # the bounds of the counted bodies and the side of the finest search cell
    hi: np.ndarray
    h: float


@dataclass(frozen=True)
class SpanningTree:
    """nb_mst_sim's tree (include/nbody.h "Minimum spanning tree"; no reference counterpart): the Euclidean minimum
    spanning tree of the counted bodies under the order (d2, lo, hi).  edges: (m, 2) uint32, lo < hi, the body
    indices of read_particles() at that moment; d2: (m,) float64, ascending; degree: (n,) uint32, MST_NONE for a body
    that is not counted, or None when not asked for.  The components of fof_groups(link, min_members=1) are those
    of the edges with d2 <= link^2: cut(link) returns them, for every link, without another pass over the bodies."""
    edges: np.ndarray
    d2: np.ndarray
    degree: Optional[np.ndarray]
    stats: MstStats

    @property
    def length(self) -> np.ndarray:
        """sqrt(d2): the edges' lengths, ascending."""
        return np.sqrt(self.d2)

    @property
    def total_length(self) -> float:
        """The lengths added in edge order from 0 (what the C++ mirror and `headless --mst` print)."""
        return float(np.cumsum(self.length)[-1]) if len(self.d2) else 0.0

    @property
    def counted(self) -> int:
        return self.stats.n - self.stats.nonfinite

    def longest(self):
        """(lo, hi, length) of the last edge, the one whose removal splits the state at the largest scale; None
        for a tree without edges."""
        if len(self.d2) == 0:
            return None
        return int(self.edges[-1, 0]), int(self.edges[-1, 1]), float(math.sqrt(self.d2[-1]))

    def _columns(self):
        return np.ascontiguousarray(self.edges[:, 0]), np.ascontiguousarray(self.edges[:, 1])

    def cut(self, link: float) -> np.ndarray:
        """(n,) uint32: per body the smallest index of its component under the edges with d2 <= link^2
        (nb_mst_cut), FOF_NONE for a body that is not counted: fof_groups(link, min_members=1).labels of the same
        state, and an assignment shapes_of / radii_of (with m = n rows: a label is a body index) and
        phase_map(values=...) accept.  A tree taken with degree=False of a state with bodies that are not counted
        cannot tell them apart and raises, as to_scipy does."""
        if self.degree is None and self.stats.nonfinite:
            raise ValueError("cut: a state with bodies that are not counted needs degree=True")
        n, m = self.stats.n, len(self.d2)
        lo, hi = self._columns()
        labels = np.empty(n, dtype=np.uint32)
        deg = None if self.degree is None else self.degree.ctypes.data
        check(_lib.lib().nb_mst_cut(n, m, lo.ctypes.data, hi.ctypes.data, self.d2.ctypes.data, deg, float(link),
                                    labels.ctypes.data, None))
        return labels

    def linkage(self):
        """The dendrogram (nb_mst_linkage): per edge in order label_a < label_b, the smallest indices of the two
        components it joins, and count_a, count_b, their sizes; four (m,) uint32 arrays."""
        n, m = self.stats.n, len(self.d2)
        lo, hi = self._columns()
        out = [np.empty(m, dtype=np.uint32) for _ in range(4)]
        check(_lib.lib().nb_mst_linkage(n, m, lo.ctypes.data, hi.ctypes.data, *[a.ctypes.data for a in out]))
        return tuple(out)

    def group_counts(self, links, min_members: int = 1) -> np.ndarray:
        """The percolation curve: per link the number of components of at least min_members bodies, from one pass
        over the linkage: a merge changes the number by [a + b >= M] - [a >= M] - [b >= M]."""
        mm = int(min_members)
        if mm < 1:
            raise ValueError("group_counts: min_members must be at least 1")
        links = np.atleast_1d(np.asarray(links, dtype=np.float64))
        if not np.all(np.isfinite(links) & (links > 0.0)):
            raise ValueError("group_counts: every link must be finite and > 0")
        _, _, ca, cb = self.linkage()
        ca, cb = ca.astype(np.int64), cb.astype(np.int64)
        delta = (ca + cb >= mm).astype(np.int64) - (ca >= mm) - (cb >= mm)
        after = np.concatenate(([self.counted if mm == 1 else 0], delta)).cumsum()
        return after[np.searchsorted(self.d2, links * links, side="right")]

    def to_scipy(self) -> np.ndarray:
        """The (m, 4) linkage matrix of scipy.cluster.hierarchy: per merge the two cluster ids (the smaller first), the
        distance sqrt(d2) and the new cluster's size; observation k is the k-th counted body, merge e makes cluster
        c + e."""
        la, lb, ca, cb = self.linkage()
        c, m = self.counted, len(self.d2)
        if self.degree is None:
            if self.stats.nonfinite:
                raise ValueError("to_scipy: a state with bodies that are not counted needs degree=True")
            obs = np.arange(self.stats.n, dtype=np.int64)
        else:
            obs = np.cumsum(self.degree != MST_NONE) - 1
        cid = {}
        z = np.empty((m, 4), dtype=np.float64)
        dist = self.length
        for e in range(m):
            a, b = int(la[e]), int(lb[e])
            x, y = cid.get(a, int(obs[a])), cid.get(b, int(obs[b]))
            z[e] = (min(x, y), max(x, y), dist[e], int(ca[e]) + int(cb[e]))
            cid[a] = c + e
        return z

    def largest_gap(self):
        """(ratio, link): the largest ratio length[e + 1] / length[e] over the edges of positive length, and
        length[e], the link just below the gap -- cut(link) unites everything shorter.  (nan, nan) with fewer than two
        such edges."""
        ln = self.length
        ln = ln[ln > 0.0]
        if len(ln) < 2:
            return float("nan"), float("nan")
        r = ln[1:] / ln[:-1]
        e = int(np.argmax(r))
        return float(r[e]), float(ln[e])


def _spanning_tree(call, handle, n, degree) -> SpanningTree:
    p = _lib.nb_mst_params()
    room = max(n - 1, 0)
    lo = np.empty(room, dtype=np.uint32)
    hi = np.empty(room, dtype=np.uint32)
    d2 = np.empty(room, dtype=np.float64)
    deg = np.empty(n, dtype=np.uint32) if degree else None
    st = _lib.nb_mst_stats()
    check(call(handle, C.byref(p), lo.ctypes.data, hi.ctypes.data, d2.ctypes.data,
               deg.ctypes.data if degree else None, C.byref(st)))
    m = int(st.edges)
    stats = MstStats(int(st.step_num), int(st.n), int(st.nonfinite), m, int(st.rounds),
                     np.array(st.components_after[:], dtype=np.uint32), float(st.d2_min), float(st.d2_max),
                     np.array(st.lo[:], dtype=np.float64), np.array(st.hi[:], dtype=np.float64), float(st.h))
    return SpanningTree(np.stack((lo[:m], hi[:m]), axis=1), d2[:m].copy(), deg, stats)


KIN_SHORT, KIN_NOT_COUNTED = _lib.NB_KIN_SHORT, _lib.NB_KIN_NOT_COUNTED
KIN_DEGENERATE, KIN_SINGULAR = _lib.NB_KIN_DEGENERATE, _lib.NB_KIN_SINGULAR


@dataclass(frozen=True)
class KinStats:
    """nb_kin_stats (include/nbody.h "Local kinematics")."""
    step_num: int
    n: int
    nonfinite: int
    counted: int
    degenerate: int   # counted bodies with at least k others at their own position
    short_of_k: int   # the counted bodies when there are no more than k of them, else 0
    k: int
    flags: int


def _sym33(six: np.ndarray) -> np.ndarray:
    """(n, 6) xx, xy, xz, yy, yz, zz -> (n, 3, 3)."""
    return six[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


@dataclass(frozen=True)
class LocalKinematics:
    """nb_local_kinematics_sim's per-body sums over the k nearest neighbours and what nb_local_kinematics_derive
    makes of them (include/nbody.h "Local kinematics"; no reference counterpart).  moments (n, 10): S0, S1[3],
    S2[6]; grads (n, 15) with gradient=True: D[6], C[9]; r2, mass_in, density as knn_density(k) returns them; kth
    with neighbours=True; derived: _lib.KIN_DERIVED_DTYPE records, one per body, which the properties read.  A body
    that is short of k or not counted has NaN in every derived value (status says which)."""
    k: int
    moments: np.ndarray
    grads: Optional[np.ndarray]
    r2: np.ndarray
    kth: Optional[np.ndarray]
    mass_in: np.ndarray
    density: np.ndarray
    derived: np.ndarray
    stats: KinStats

    @property
    def r_k(self) -> np.ndarray:
        """sqrt(r2): the distance to the k-th neighbour."""
        return np.sqrt(self.r2)

    @property
    def mass(self) -> np.ndarray:
        """S0: the mass of the neighbours (and, with include_self, of the body)."""
        return self.derived["mass"]

    @property
    def mean_velocity(self) -> np.ndarray:
        """(n, 3): the bulk velocity at the body, its own velocity plus relative_velocity."""
        return self.derived["mean_velocity"]

    @property
    def relative_velocity(self) -> np.ndarray:
        """(n, 3): the neighbours' mass-weighted mean velocity relative to the body, S1 / S0."""
        return self.derived["relative_velocity"]

    @property
    def dispersion_tensor(self) -> np.ndarray:
        """(n, 3, 3): S2 / S0 - u u."""
        return _sym33(self.derived["dispersion"])

    @property
    def sigma(self) -> np.ndarray:
        """The one-dimensional velocity dispersion sqrt(trace / 3)."""
        return self.derived["sigma"]

    @property
    def phase_space_density(self) -> np.ndarray:
        """Q = density / sigma^3."""
        return self.derived["phase_space_density"]

    @property
    def status(self) -> np.ndarray:
        """KIN_SHORT | KIN_NOT_COUNTED | KIN_DEGENERATE | KIN_SINGULAR per body."""
        return self.derived["status"]

    def _needs_gradient(self):
        if self.grads is None:
            raise ValueError("local_kinematics(gradient=True) makes the velocity gradient")

    @property
    def velocity_gradient(self) -> np.ndarray:
        """(n, 3, 3): G[a, b] = d u_a / d x_b by least squares over the neighbours; NaN where KIN_SINGULAR."""
        self._needs_gradient()
        return self.derived["gradient"].reshape(-1, 3, 3)

    @property
    def divergence(self) -> np.ndarray:
        self._needs_gradient()
        return self.derived["divergence"]

    @property
    def vorticity(self) -> np.ndarray:
        self._needs_gradient()
        return self.derived["vorticity"]

    @property
    def shear(self) -> np.ndarray:
        self._needs_gradient()
        return self.derived["shear"]


def kinematics_derive(moments, grads, r2, density, velocities) -> np.ndarray:
    """nb_local_kinematics_derive: _lib.KIN_DERIVED_DTYPE records from the raw sums (host only).  grads, density and
    velocities ((n, 3) float32) may be None."""
    moments = np.ascontiguousarray(moments, dtype=np.float64).reshape(-1, _lib.NB_KIN_MOMENTS)
    n = moments.shape[0]

    def arr(a, dtype, width):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dtype)
        if a.size != n * width:
            raise ValueError(f"expected {n} x {width} values, got {a.size}")
        return a

    grads, r2 = arr(grads, np.float64, _lib.NB_KIN_GRADS), arr(r2, np.float64, 1)
    density, velocities = arr(density, np.float64, 1), arr(velocities, np.float32, 3)
    out = np.zeros(n, dtype=_lib.KIN_DERIVED_DTYPE)
    ptr = lambda a: None if a is None else a.ctypes.data
    check(_lib.lib().nb_local_kinematics_derive(moments.ctypes.data, ptr(grads), ptr(r2), ptr(density),
                                                ptr(velocities), n, out.ctypes.data))
    return out


def _local_kinematics(call, owner, n, k, gradient, include_self, neighbours) -> LocalKinematics:
    p = _lib.nb_kin_params()
    kk = int(k)
    p.k, p.reserved = (kk if 0 <= kk <= 0xFFFFFFFF else 0), 0  # (the call refuses 0 itself)
    p.flags = _lib.NB_KIN_SELF if include_self else 0
    moments = np.empty((n, _lib.NB_KIN_MOMENTS), dtype=np.float64)
    grads = np.empty((n, _lib.NB_KIN_GRADS), dtype=np.float64) if gradient else None
    r2, mass_in, rho = (np.empty(n, dtype=np.float64) for _ in range(3))
    kth = np.empty(n, dtype=np.uint32) if neighbours else None
    ptr = lambda a: None if a is None else a.ctypes.data
    st = _lib.nb_kin_stats()
    check(call(owner._h, C.byref(p), moments.ctypes.data, ptr(grads), r2.ctypes.data, ptr(kth), mass_in.ctypes.data,
               rho.ctypes.data, C.byref(st)))
    vel = np.ascontiguousarray(owner.read_particles()["velocity"], dtype=np.float32)
    derived = kinematics_derive(moments, grads, r2, rho, vel)
    stats = KinStats(int(st.step_num), int(st.n), int(st.nonfinite), int(st.counted), int(st.degenerate),
                     int(st.short_of_k), int(st.k), int(st.flags))
    return LocalKinematics(kk, moments, grads, r2, kth, mass_in, rho, derived, stats)


HALO_CENTER_NONFINITE = _lib.NB_HALO_CENTER_NONFINITE


@dataclass(frozen=True)
class HaloStats:
    """nb_halo_stats (include/nbody.h "Halo profiles")."""
    step_num: int
    n: int
    nonfinite: int
    centers: int
    tested: int           # candidate distance tests: what the grid did not prune
    items: int            # work items of NB_HALO_CHUNK candidates
    cells: tuple          # cells per axis of the grid


@dataclass(frozen=True)
class HaloProfiles:
    """nb_sim_halo_profiles' rows (include/nbody.h "Halo profiles"; no reference counterpart): the spherical
    profile of RadialProfile about m centres at once, with shared edges.  Per-bin fields are (m, nbins) arrays
    (count: uint64, ang: (m, nbins, 3)); inside_count, inside_mass, center, velocity and flags are per centre.
    Bodies at or beyond edges[-1] are not reported."""
    edges: np.ndarray      # nbins + 1
    count: np.ndarray
    mass: np.ndarray       # sum m
    m_r: np.ndarray        # sum m r
    m_ur: np.ndarray       # sum m u_r
    m_ur2: np.ndarray      # sum m u_r^2
    m_u2: np.ndarray       # sum m |u|^2
    ang: np.ndarray        # sum m (d x u)
    inside_count: np.ndarray
    inside_mass: np.ndarray
    center: np.ndarray     # (m, 3): the centres used
    velocity: np.ndarray   # (m, 3)
    flags: np.ndarray      # HALO_CENTER_NONFINITE: a body centre that does not count (its row is zero)
    stats: HaloStats

    @property
    def nbins(self) -> int:
        return self.edges.shape[0] - 1

    @property
    def enclosed_mass(self) -> np.ndarray:
        """(m, nbins + 1): the mass inside edges[k] (nb_halo_enclosed: inside_mass, then the bins in order)."""
        return np.cumsum(np.concatenate([self.inside_mass[:, None], self.mass], axis=1), axis=1)

    @property
    def density(self) -> np.ndarray:
        """mass over the shell's volume 4 pi (b^3 - a^3) / 3."""
        a, b = self.edges[:-1], self.edges[1:]
        return self.mass / (_lib.NB_KNN_SPHERE * (b ** 3 - a ** 3))

    @property
    def mean_ur(self) -> np.ndarray:
        """Mass-weighted mean radial velocity per bin (NaN in a bin without mass)."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.m_ur / self.mass

    @property
    def sigma_r(self) -> np.ndarray:
        """Mass-weighted radial velocity dispersion per bin (NaN in a bin without mass)."""
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = self.m_ur / self.mass
            return np.sqrt(np.maximum(self.m_ur2 / self.mass - mean * mean, 0.0))

    def vcirc(self, G: float) -> np.ndarray:
        """(m, nbins + 1): sqrt(G M(<r) / r) at every edge (NaN at an edge of radius 0)."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.sqrt(float(G) * self.enclosed_mass / np.where(self.edges > 0.0, self.edges, np.nan))

    def overdensity(self, rho: float):
        """nb_halo_overdensity per centre: (r, mass), each (m,), where the mean enclosed density first falls
        through rho, interpolated between two edges (binned: limited by the bins' resolution); NaN where the
        profile has no such crossing."""
        m, nbins = self.mass.shape
        edges = np.ascontiguousarray(self.edges, dtype=np.float64)
        head = np.zeros(1, dtype=_lib.HALO_HEAD_DTYPE)
        bins = np.zeros(nbins, dtype=_lib.RADIAL_BIN_DTYPE)
        r, mass = np.empty(m, dtype=np.float64), np.empty(m, dtype=np.float64)
        a, b = C.c_double(), C.c_double()
        for j in range(m):
            head["inside_mass"][0] = self.inside_mass[j]
            bins["mass"] = self.mass[j]
            check(_lib.lib().nb_halo_overdensity(head.ctypes.data, bins.ctypes.data,
                                                 edges.ctypes.data_as(C.POINTER(C.c_double)), nbins, float(rho),
                                                 C.byref(a), C.byref(b)))
            r[j], mass[j] = a.value, b.value
        return r, mass


def _halo_profiles(call, handle, centers, bodies, velocities, edges, nbins, rmin, rmax, log) -> HaloProfiles:
    if edges is None:
        if rmin is None or rmax is None:
            raise ValueError("halo_profiles needs edges, or rmin and rmax")
        if not 1 <= int(nbins) <= _lib.NB_HALO_MAX_BINS:
            raise ValueError(f"halo_profiles: nbins must be 1..{_lib.NB_HALO_MAX_BINS}")
        edges = radial_edges(rmin, rmax, nbins, log)
    edges = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
    dp = C.POINTER(C.c_double)
    p = _lib.nb_halo_params()
    p.nbins, p.flags = max(edges.shape[0] - 1, 0), 0
    p.edges = edges.ctypes.data_as(dp)
    m = 0
    if centers is not None:
        centers = np.ascontiguousarray(centers, dtype=np.float64).reshape(-1, 3)
        m = centers.shape[0]
        p.centers = centers.ctypes.data_as(dp)
    if bodies is not None:
        bodies = np.ascontiguousarray(bodies).reshape(-1)
        if bodies.size and (bodies.min() < 0 or bodies.max() > 0xFFFFFFFF):
            raise ValueError("halo_profiles: bodies are 32-bit body indices")
        bodies = bodies.astype(np.uint32)
        if centers is None:
            m = bodies.shape[0]
        p.bodies = bodies.ctypes.data_as(C.POINTER(C.c_uint32))
    if velocities is not None:
        velocities = np.ascontiguousarray(velocities, dtype=np.float64).reshape(-1, 3)
        if velocities.shape[0] != m:
            raise ValueError("halo_profiles: one velocity per centre")
        p.velocities = velocities.ctypes.data_as(dp)
    if centers is not None and bodies is not None and bodies.shape[0] != m:
        raise ValueError("halo_profiles: centers and bodies differ in length (and only one may be given)")
    p.m = m
    nb = int(p.nbins)
    heads = np.zeros(m, dtype=_lib.HALO_HEAD_DTYPE)
    bins = np.zeros((m, max(nb, 1)), dtype=_lib.RADIAL_BIN_DTYPE)
    st = _lib.nb_halo_stats()
    check(call(handle, C.byref(p), heads.ctypes.data, bins.ctypes.data, C.byref(st)))
    stats = HaloStats(int(st.step_num), int(st.n), int(st.nonfinite), int(st.centers), int(st.tested), int(st.items),
                      tuple(int(c) for c in st.cells))
    return HaloProfiles(edges.copy(), bins["count"].copy(), bins["mass"].copy(), bins["m_r"].copy(),
                        bins["m_ur"].copy(), bins["m_ur2"].copy(), bins["m_u2"].copy(), bins["ang"].copy(),
                        heads["inside_count"].copy(), heads["inside_mass"].copy(), heads["center"].copy(),
                        heads["velocity"].copy(), heads["flags"].copy(), stats)


def _group_profiles(halo_profiles, groups, center, kw):
    """rows, HaloProfiles: the profiles about the usable rows of a FofGroups / BoundGroups / HopGroups catalogue."""
    if center == "com":
        with np.errstate(invalid="ignore", divide="ignore"):
            c, v = groups.com, groups.velocity
        rows = np.nonzero(np.isfinite(c).all(axis=1) & np.isfinite(v).all(axis=1))[0]
        return rows, halo_profiles(c[rows], velocities=v[rows], **kw)
    if center == "most_bound":
        if "most_bound" not in (groups.rows.dtype.names or ()):
            raise ValueError('group_profiles: center="most_bound" needs a BoundGroups')
        mb = groups.rows["most_bound"]
        rows = np.nonzero(mb != _lib.NB_FOF_NONE)[0]
        return rows, halo_profiles(bodies=mb[rows], **kw)
    if center == "peak":
        if not isinstance(groups, HopGroups):
            raise ValueError('group_profiles: center="peak" needs a HopGroups')
        rows = np.arange(len(groups.rows))
        return rows, halo_profiles(bodies=groups.rows["label"], **kw)
    raise ValueError('group_profiles: center is "com", "most_bound" or "peak"')


SHAPE_CONVERGED, SHAPE_UNCONVERGED = _lib.NB_SHAPE_CONVERGED, _lib.NB_SHAPE_UNCONVERGED
SHAPE_DEGENERATE, SHAPE_EMPTY = _lib.NB_SHAPE_DEGENERATE, _lib.NB_SHAPE_EMPTY


@dataclass(frozen=True)
class ShapeStats:
    """nb_shape_stats (include/nbody.h "Group shapes")."""
    step_num: int
    n: int
    rows: int
    members: int            # counted bodies with a row
    nonfinite_members: int
    converged: int
    unconverged: int
    degenerate: int
    empty: int
    rounds_max: int


@dataclass(frozen=True)
class GroupShapes:
    """nb_sim_group_shapes' rows (include/nbody.h "Group shapes"; no reference counterpart): for every row of an
    assignment of bodies to rows the shape tensor of the members inside an ellipsoid deformed until its axis ratios
    are the tensor's, with the mass, the velocity moments and the angular momentum of the same members.  rows:
    _lib.SHAPE_GROUP_DTYPE records; catalogue_rows: the rows of the catalogue they belong to (group_shapes leaves
    out the rows without a finite centre; shapes_of: 0 .. m - 1); selected_of: (n,) uint32, the row (of `rows`) of a
    body selected in the last round of a row with a shape, FOF_NONE otherwise, or None when not asked for."""
    rows: np.ndarray
    catalogue_rows: np.ndarray
    selected_of: Optional[np.ndarray]
    reduced: bool
    max_iter: int
    tol: float
    min_members: int
    stats: ShapeStats

    @property
    def status(self) -> np.ndarray:
        return self.rows["status"]

    @property
    def b_over_a(self) -> np.ndarray:
        """q = sqrt(lambda_2 / lambda_1); NaN for a row without a shape."""
        return self.rows["q"]

    @property
    def c_over_a(self) -> np.ndarray:
        """s = sqrt(lambda_3 / lambda_1)."""
        return self.rows["s"]

    @property
    def triaxiality(self) -> np.ndarray:
        """(1 - q^2) / (1 - s^2): 0 oblate, 1 prolate; NaN for a sphere."""
        q, s = self.rows["q"], self.rows["s"]
        with np.errstate(invalid="ignore", divide="ignore"):
            return (1.0 - q * q) / (1.0 - s * s)

    @property
    def major_axis(self) -> np.ndarray:
        """(rows, 3): the unit eigenvector of the largest eigenvalue."""
        return self.rows["axes"][:, 0:3]

    @property
    def minor_axis(self) -> np.ndarray:
        return self.rows["axes"][:, 6:9]

    @property
    def angular_momentum(self) -> np.ndarray:
        """(rows, 3): J = sum m (d x u) of the selected members about the centre, in the frame of `velocity`."""
        return self.rows["j"]

    @property
    def spin_axis(self) -> np.ndarray:
        """(rows, 3): J / |J|; NaN for J = 0."""
        j = self.rows["j"]
        with np.errstate(invalid="ignore", divide="ignore"):
            return j / np.sqrt((j * j).sum(axis=1))[:, None]

    @property
    def misalignment(self) -> np.ndarray:
        """The angle between J and the minor axis, 0 .. pi/2 (an axis has no sign)."""
        with np.errstate(invalid="ignore"):
            return np.arccos(np.minimum(np.abs((self.spin_axis * self.minor_axis).sum(axis=1)), 1.0))

    @property
    def sigma_tensor(self) -> np.ndarray:
        """(rows, 3, 3): the mass-weighted velocity dispersion tensor of the selected members about their mean."""
        r = self.rows
        with np.errstate(invalid="ignore", divide="ignore"):
            uu = r["uu"] / r["mass"][:, None]
            mean = r["mu"] / r["mass"][:, None]
        out = np.empty((len(r), 3, 3))
        for k, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            out[:, i, j] = out[:, j, i] = uu[:, k] - mean[:, i] * mean[:, j]
        return out

    def spin_bullock(self, G: float) -> np.ndarray:
        """|J| / (sqrt(2) M R sqrt(G M / R)) (Bullock et al. 2001) of the selected members, for a finite R."""
        r = self.rows
        j = np.sqrt((r["j"] * r["j"]).sum(axis=1))
        with np.errstate(invalid="ignore", divide="ignore"):
            lam = j / (math.sqrt(2.0) * r["mass"] * r["radius"] * np.sqrt(G * r["mass"] / r["radius"]))
        return np.where(np.isfinite(r["radius"]), lam, np.nan)


def _shape_radius(radius, m, rms):
    """None, or the (m,) radii of a call: a number for all rows, one per row, or ("rms", k) for k rms[r]."""
    if radius is None:
        return None
    if isinstance(radius, tuple) and len(radius) == 2 and radius[0] == "rms":
        if rms is None:
            raise ValueError('group_shapes: radius=("rms", k) needs a catalogue with an rms radius')
        return np.ascontiguousarray(float(radius[1]) * np.asarray(rms, dtype=np.float64))
    r = np.asarray(radius, dtype=np.float64)
    if r.ndim == 0:
        return np.full(m, float(r))
    if r.shape != (m,):
        raise ValueError(f"group_shapes: {m} rows need {m} radii, or one for all")
    return np.ascontiguousarray(r)


def _group_shapes(call, handle, n, group_of, m, centers, velocities, radius, reduced, max_iter, tol, min_members,
                  per_body, step_num, catalogue_rows) -> GroupShapes:
    for name, v in (("min_members", min_members), ("max_iter", max_iter), ("m", m)):
        if not 0 <= int(v) <= 0xFFFFFFFF:  # (the call itself refuses the zeros that mean nothing)
            raise ValueError(f"group_shapes: {name} = {v} is not a 32-bit count")
    m = int(m)
    gof = np.ascontiguousarray(group_of, dtype=np.uint32).reshape(-1)
    if gof.shape[0] != n:
        raise ValueError(f"group_shapes: group_of has {gof.shape[0]} values for {n} bodies")
    p = _lib.nb_shape_params()
    p.flags, p.reserved32, p.reserved = (_lib.NB_SHAPE_REDUCED if reduced else 0), 0, 0
    p.min_members, p.max_iter, p.tol = int(min_members), int(max_iter), float(tol)
    p.step_num = _lib.NB_SHAPE_ANY_STEP if step_num is None else int(step_num)

    def vec(a, width, what):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1, width) if width > 1 else _shape_radius(a, m, None)
        if a.shape[0] != m:
            raise ValueError(f"group_shapes: {m} rows need {m} {what}")
        return a
    centers, velocities, radius = vec(centers, 3, "centers"), vec(velocities, 3, "velocities"), vec(radius, 1, "radii")
    rows = np.zeros(m, dtype=_lib.SHAPE_GROUP_DTYPE)
    sel = np.empty(n, dtype=np.uint32) if per_body else None
    st = _lib.nb_shape_stats()
    ptr = lambda a: a.ctypes.data if a is not None else None
    check(call(handle, C.byref(p), ptr(gof), m, ptr(centers), ptr(velocities), ptr(radius), rows.ctypes.data, ptr(sel),
               C.byref(st)))
    stats = ShapeStats(int(st.step_num), int(st.n), int(st.rows), int(st.members), int(st.nonfinite_members),
                       int(st.converged), int(st.unconverged), int(st.degenerate), int(st.empty), int(st.rounds_max))
    return GroupShapes(rows, np.asarray(catalogue_rows), sel, bool(reduced), int(max_iter), float(tol),
                       int(min_members), stats)


def _catalogue_rms(groups):
    """The catalogue's mass-weighted rms radius about com (FofGroups.rms_radius), for every kind of catalogue."""
    with np.errstate(invalid="ignore", divide="ignore"):
        c = groups.com
        return np.sqrt(np.maximum(groups._per_mass(groups.rows["mr2"]) - (c * c).sum(axis=1), 0.0))


def _catalogue_assignment(what, read_particles, groups, members, center):
    """(mapped, rows, c, v) of a catalogue for `what` (group_shapes, group_radii): the catalogue rows with a finite
    centre (as _group_profiles resolves them), their centres and velocities, and the assignment renumbered to them."""
    if members == "group":
        assign = groups.group_of
    elif members == "bound":
        assign = getattr(groups, "bound_of", None)
        if assign is None:
            raise ValueError(f'{what}: members="bound" needs a BoundGroups made with per_body=True')
    else:
        raise ValueError(f'{what}: members is "group" or "bound"')
    total = len(groups.rows)
    if center == "com":
        with np.errstate(invalid="ignore", divide="ignore"):
            c, v = groups.com, groups.velocity
        rows = np.nonzero(np.isfinite(c).all(axis=1) & np.isfinite(v).all(axis=1))[0]
        c, v = c[rows], v[rows]
    elif center in ("most_bound", "peak"):
        if center == "most_bound":
            if "most_bound" not in (groups.rows.dtype.names or ()):
                raise ValueError(f'{what}: center="most_bound" needs a BoundGroups')
            body = groups.rows["most_bound"]
            rows = np.nonzero(body != _lib.NB_FOF_NONE)[0]
        else:
            if not isinstance(groups, HopGroups):
                raise ValueError(f'{what}: center="peak" needs a HopGroups')
            body = groups.rows["label"]
            rows = np.arange(total)
        parts = read_particles()  # the body's widened position and velocity, as a body centre of halo_profiles
        at = body[rows].astype(np.int64)
        c = parts["position"][at].astype(np.float64)
        v = parts["velocity"][at].astype(np.float64)
        ok = np.isfinite(c).all(axis=1) & np.isfinite(v).all(axis=1)
        rows, c, v = rows[ok], c[ok], v[ok]
    else:
        raise ValueError(f'{what}: center is "com", "most_bound" or "peak"')
    # the usable rows renumbered 0 .. len(rows) - 1; a body of another row has no row
    renumber = np.full(total + 1, _lib.NB_FOF_NONE, dtype=np.uint32)
    renumber[rows] = np.arange(len(rows), dtype=np.uint32)
    assign = np.asarray(assign, dtype=np.uint32)
    mapped = renumber[np.minimum(assign, total)]  # (FOF_NONE -> the spare entry)
    return mapped, rows, c, v


def _shapes_of_groups(shapes_of, read_particles, groups, members, center, radius, check_step, kw) -> GroupShapes:
    """group_shapes: the assignment, the centres (as _group_profiles resolves them) and the radii from a catalogue."""
    mapped, rows, c, v = _catalogue_assignment("group_shapes", read_particles, groups, members, center)
    rad = _shape_radius(radius, len(groups.rows), _catalogue_rms(groups) if isinstance(radius, tuple) else None)
    step = groups.stats.step_num if check_step else None
    return shapes_of(mapped, len(rows), centers=c, velocities=v, radius=None if rad is None else rad[rows],
                     step_num=step, catalogue_rows=rows, **kw)


@dataclass(frozen=True)
class RadiiStats:
    """nb_radii_stats (include/nbody.h "Group radii")."""
    step_num: int
    n: int
    rows: int
    members: int            # counted bodies with a row
    nonfinite_members: int
    empty: int


@dataclass(frozen=True)
class GroupRadii:
    """nb_group_radii_sim's rows (include/nbody.h "Group radii"; no reference counterpart): for every row of an
    assignment of bodies to rows the members ordered by distance from the row's centre, the enclosed mass in a fixed
    order, the member at which it reaches each fraction of the row's mass and the peak of M / r.  rows:
    _lib.RADII_GROUP_DTYPE records; catalogue_rows: the rows of the catalogue they belong to (group_radii leaves out
    the rows without a finite centre; radii_of: 0 .. m - 1); fractions: as asked for; rank_of (n,) uint32 and
    enclosed_of (n,) float64: a member's place in its row's order (FOF_NONE for a body of no row) and M there (NaN),
    or None when not asked for."""
    rows: np.ndarray
    catalogue_rows: np.ndarray
    fractions: tuple
    vmax_skip: int
    rank_of: Optional[np.ndarray]
    enclosed_of: Optional[np.ndarray]
    stats: RadiiStats

    @property
    def radius(self) -> np.ndarray:
        """(rows, nf): the distance of the member at which the enclosed mass reaches fractions[f] of the row's."""
        return self.rows["radius"][:, :len(self.fractions)]

    @property
    def index(self) -> np.ndarray:
        """(rows, nf): that member's body index, FOF_NONE where there is none."""
        return self.rows["index"][:, :len(self.fractions)]

    @property
    def half_mass_radius(self) -> np.ndarray:
        """(rows,): the column of fraction 0.5; a ValueError when 0.5 was not asked for."""
        if 0.5 not in self.fractions:
            raise ValueError("half_mass_radius: 0.5 is not among the fractions of this call")
        return self.radius[:, self.fractions.index(0.5)]

    @property
    def r_vmax(self) -> np.ndarray:
        """(rows,): the radius at which M / r peaks; NaN where no member qualifies."""
        return self.rows["r_vmax"]

    def vmax(self, G: float) -> np.ndarray:
        """(rows,): sqrt(G max(M / r)), the peak of the circular-velocity curve."""
        with np.errstate(invalid="ignore"):
            return np.sqrt(float(G) * self.rows["vc2_max"])


def _group_radii(call, handle, n, group_of, m, fractions, centers, vmax_skip, per_body, step_num,
                 catalogue_rows) -> GroupRadii:
    for name, v in (("vmax_skip", vmax_skip), ("m", m)):
        if not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError(f"group_radii: {name} = {v} is not a 32-bit count")
    m = int(m)
    fractions = tuple(float(f) for f in np.asarray(fractions, dtype=np.float64).reshape(-1))
    gof = np.ascontiguousarray(group_of, dtype=np.uint32).reshape(-1)
    if gof.shape[0] != n:
        raise ValueError(f"group_radii: group_of has {gof.shape[0]} values for {n} bodies")
    p = _lib.nb_radii_params()
    p.nf, p.vmax_skip, p.reserved = len(fractions), int(vmax_skip), 0  # (the call refuses an nf it does not take)
    for k, f in enumerate(fractions[:_lib.NB_RADII_MAX_FRACTIONS]):
        p.fractions[k] = f
    p.step_num = _lib.NB_RADII_ANY_STEP if step_num is None else int(step_num)
    if centers is not None:
        centers = np.ascontiguousarray(centers, dtype=np.float64).reshape(-1, 3)
        if centers.shape[0] != m:
            raise ValueError(f"group_radii: {m} rows need {m} centers")
    rows = np.zeros(m, dtype=_lib.RADII_GROUP_DTYPE)
    rank = np.empty(n, dtype=np.uint32) if per_body else None
    enc = np.empty(n, dtype=np.float64) if per_body else None
    st = _lib.nb_radii_stats()
    ptr = lambda a: a.ctypes.data if a is not None else None
    check(call(handle, C.byref(p), ptr(gof), m, ptr(centers), rows.ctypes.data, ptr(rank), ptr(enc), C.byref(st)))
    stats = RadiiStats(int(st.step_num), int(st.n), int(st.rows), int(st.members), int(st.nonfinite_members),
                       int(st.empty))
    return GroupRadii(rows, np.asarray(catalogue_rows), fractions, int(vmax_skip), rank, enc, stats)


SMOOTH_K = _lib.NB_SMOOTH_K
SMOOTH_PLANES = ("wm", "wm_ua", "wm_ub", "wm_w", "wm_w2", "wm_u2")


def smooth_centres(lo: float, hi: float, cells: int) -> np.ndarray:
    """nb_smooth_centres: the pixel centres of a smoothed map's window, the means of successive map_edges."""
    out = np.empty(int(cells) if 1 <= int(cells) <= _lib.NB_MAP_MAX_SIDE else 1, dtype=np.float64)
    check(_lib.lib().nb_smooth_centres(float(lo), float(hi), int(cells), out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


@dataclass(frozen=True)
class SmoothStats:
    """nb_smooth_stats (include/nbody.h "Smoothed maps").  nonfinite + bad_smoothing + skipped + deposited == n."""
    step_num: int
    n: int
    nonfinite: int
    bad_smoothing: int    # counted bodies whose smoothing length is NaN
    skipped: int          # outside the depth slab, or no pixel centre within the smoothing length
    deposited: int
    raised: int           # smoothing lengths below s_min
    lowered: int          # ... above s_max
    pairs: int            # the sum of counts
    tile_entries: int     # implementation figure: the (tile, body) entries sorted
    mass: float           # all counted bodies
    deposited_mass: float
    center: np.ndarray
    velocity: np.ndarray
    n_hat: np.ndarray
    e1: np.ndarray
    e2: np.ndarray
    s_min: float
    s_max: float
    flags: int
    max_count: int


@dataclass(frozen=True)
class SmoothedMap:
    """nb_sim_smooth_map's counts, planes and stats (include/nbody.h "Smoothed maps"; no reference counterpart):
    every body of the state read_particles would return spread over the pixels whose centre lies within its
    smoothing length, with the kernel (3 / (pi s^2)) (1 - r^2 / s^2)^2.  counts: (H, W) uint32, the bodies that
    reach a pixel.  planes: (P, H, W) float64, P = 1 or 6 in the order of SMOOTH_PLANES; plane 0 is the surface
    density itself.  w is the velocity along the line of sight."""
    counts: np.ndarray
    planes: np.ndarray
    x_centres: np.ndarray
    y_centres: np.ndarray
    smoothing: np.ndarray  # the n lengths passed to the call (before s_min and s_max)
    stats: SmoothStats

    def _plane(self, k):
        if self.planes.shape[0] <= k:
            raise ValueError("this map was taken without velocities")
        return self.planes[k]

    def _per_mass(self, k):
        wm = self.planes[0]
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(wm != 0.0, self._plane(k) / wm, np.nan)

    @property
    def surface_density(self) -> np.ndarray:
        """Plane 0: mass per area of the plane coordinates (0 where no body reaches)."""
        return self.planes[0]

    @property
    def mean_w(self) -> np.ndarray:
        """Kernel- and mass-weighted mean line-of-sight velocity per pixel (NaN where plane 0 is 0)."""
        return self._per_mass(3)

    @property
    def sigma_w(self) -> np.ndarray:
        """The line-of-sight velocity dispersion per pixel: sqrt(max(0, wm_w2 / wm - mean_w^2))."""
        mean = self.mean_w
        return np.sqrt(np.maximum(self._per_mass(4) - mean * mean, 0.0))


def _smoothed_map(call, handle, n, s, width, height, extent, axis, center, velocity, depth, velocities, s_min,
                  s_max) -> SmoothedMap:
    p = _lib.nb_smooth_params()
    p.width, p.height = int(width), int(height)
    p.flags = _lib.NB_SMOOTH_VELOCITY if velocities else 0
    if isinstance(center, str):
        if center != "com":
            raise ValueError('center is "com" or three coordinates')
        if velocity is not None:
            raise ValueError('center="com" brings its own velocity')
        p.flags |= _lib.NB_SMOOTH_CENTER_COM
    else:
        velocity = (0.0, 0.0, 0.0) if velocity is None else velocity
        for k in range(3):
            p.center[k], p.velocity[k] = float(center[k]), float(velocity[k])
    x0, x1, y0, y1 = (float(v) for v in extent)
    p.x_range[0], p.x_range[1], p.y_range[0], p.y_range[1] = x0, x1, y0, y1
    p.depth_range[0], p.depth_range[1] = (-np.inf, np.inf) if depth is None else (float(depth[0]), float(depth[1]))
    for k in range(3):
        p.axis[k] = float(axis[k])
    ok = 1 <= p.width <= _lib.NB_MAP_MAX_SIDE and 1 <= p.height <= _lib.NB_MAP_MAX_SIDE and \
        p.width * p.height <= _lib.NB_MAP_MAX_CELLS
    h, w = (p.height, p.width) if ok else (1, 1)  # (the call refuses the sizes itself)
    pixel = max(abs(x1 - x0) / w, abs(y1 - y0) / h)
    p.s_min = 2.0 * pixel if s_min is None else float(s_min)
    p.s_max = 64.0 * pixel if s_max is None else float(s_max)
    s = np.ascontiguousarray(np.broadcast_to(np.asarray(s, dtype=np.float64), (n,)))
    nplanes = len(SMOOTH_PLANES) if velocities else 1
    counts = np.empty((h, w), dtype=np.uint32)
    planes = np.empty((nplanes, h, w), dtype=np.float64)
    st = _lib.nb_smooth_stats()
    check(call(handle, C.byref(p), s.ctypes.data, counts.ctypes.data, planes.ctypes.data, C.byref(st)))
    vec = lambda a: np.array(list(a), dtype=np.float64)  # noqa: E731
    stats = SmoothStats(int(st.step_num), int(st.n), int(st.nonfinite), int(st.bad_smoothing), int(st.skipped),
                        int(st.deposited), int(st.raised), int(st.lowered), int(st.pairs), int(st.tile_entries),
                        float(st.mass), float(st.deposited_mass), vec(st.center), vec(st.velocity), vec(st.n_hat),
                        vec(st.e1), vec(st.e2), float(st.s_min), float(st.s_max), int(st.flags), int(st.max_count))
    return SmoothedMap(counts, planes, smooth_centres(x0, x1, w), smooth_centres(y0, y1, h), s, stats)


def _smoothing_lengths(owner, smoothing, k, scale):
    """The n smoothing lengths of smoothed_map(): "knn" composes knn_density on the host, as center="density"
    does for the maps."""
    if isinstance(smoothing, str):
        if smoothing != "knn":
            raise ValueError('smoothing is "knn", an array of n or a scalar')
        return float(scale) * owner.knn_density(k, density=False).r_k
    return smoothing


@dataclass(frozen=True)
class Camera:
    """nb_camera (`Camera`, online_renderer.rs:12-20)."""
    eye: Sequence[float] = (0.0, 1.0, 2.0)
    target: Sequence[float] = (0.0, 0.0, 0.0)
    up: Sequence[float] = (0.0, 1.0, 0.0)
    aspect: float = 1.0
    fovy_deg: float = 45.0
    znear: float = 0.00001
    zfar: float = 100.0

    @staticmethod
    def default(width: int, height: int) -> "Camera":
        """nb_camera_default: the camera OnlineRenderer::new sets up (online_renderer.rs:231-239)."""
        c = _lib.nb_camera()
        check(_lib.lib().nb_camera_default(C.byref(c), int(width), int(height)))
        return Camera(tuple(c.eye), tuple(c.target), tuple(c.up), float(c.aspect), float(c.fovy_deg),
                      float(c.znear), float(c.zfar))

    def to_c(self) -> "_lib.nb_camera":
        c = _lib.nb_camera()
        for k in range(3):
            c.eye[k], c.target[k], c.up[k] = float(self.eye[k]), float(self.target[k]), float(self.up[k])
        c.aspect, c.fovy_deg, c.znear, c.zfar = self.aspect, self.fovy_deg, self.znear, self.zfar
        return c

    def view_proj(self) -> np.ndarray:
        """nb_camera_view_proj: the 16 floats of OPENGL_TO_WGPU_MATRIX * perspective * look_at_rh,
        column-major (online_renderer.rs:41-54)."""
        out = (C.c_float * 16)()
        c = self.to_c()
        check(_lib.lib().nb_camera_view_proj(C.byref(c), out))
        return np.array(list(out), dtype=np.float32)


@dataclass(frozen=True)
class RenderParams:
    """nb_render_params: the frame's size, the column-major view-projection matrix and the constants of
    the reference's draw pass (online_renderer.rs:224, 345-349; draw.wgsl:21)."""
    width: int
    height: int
    view_proj: Sequence[float]
    half_size: float = 0.006
    clear: Sequence[float] = (0.01, 0.0, 0.05)
    alpha: float = 0.25
    srgb: bool = True

    @staticmethod
    def default(width: int, height: int) -> "RenderParams":
        """nb_render_params_default: the reference's frame at this size."""
        p = _lib.nb_render_params()
        check(_lib.lib().nb_render_params_default(C.byref(p), int(width), int(height)))
        return RenderParams(int(p.width), int(p.height), np.array(list(p.view_proj), dtype=np.float32),
                            float(p.half_size), tuple(p.clear), float(p.alpha), bool(p.flags & _lib.NB_RENDER_SRGB))

    def to_c(self) -> "_lib.nb_render_params":
        p = _lib.nb_render_params()
        p.width, p.height = int(self.width), int(self.height)
        vp = np.asarray(self.view_proj, dtype=np.float32).reshape(-1)
        if vp.size != 16:
            raise ValueError("view_proj must hold 16 floats (column-major)")
        for k in range(16):
            p.view_proj[k] = float(vp[k])
        p.half_size, p.alpha = float(self.half_size), float(self.alpha)
        for k in range(3):
            p.clear[k] = float(self.clear[k])
        p.flags = _lib.NB_RENDER_SRGB if self.srgb else 0
        return p


@dataclass(frozen=True)
class RenderStats:
    """nb_render_stats: drawn + clipped + oversize + nonfinite == n; fragments = sum of the counts."""
    step_num: int
    n: int
    drawn: int
    clipped: int
    oversize: int
    nonfinite: int
    fragments: int
    max_count: int

    @staticmethod
    def _from_c(s: "_lib.nb_render_stats") -> "RenderStats":
        return RenderStats(int(s.step_num), int(s.n), int(s.drawn), int(s.clipped), int(s.oversize),
                           int(s.nonfinite), int(s.fragments), int(s.max_count))


class Frame(np.ndarray):
    """What render() returns: the (H, W, 4) uint8 RGBA image, rows top to bottom, with the frame's
    RenderStats as .stats."""
    stats: Optional[RenderStats] = None

    def __array_finalize__(self, obj):
        self.stats = getattr(obj, "stats", None)


def _render_params(width, height, camera, view_proj, params) -> RenderParams:
    if camera is not None and view_proj is not None:
        raise ValueError("give a camera or a view_proj matrix, not both")
    if view_proj is None:
        view_proj = (camera if camera is not None else Camera.default(width, height)).view_proj()
    return RenderParams(int(width), int(height), view_proj, **params)


def _render(call, handle, rp: RenderParams, want_counts: bool):
    p = rp.to_c()
    rgba = np.empty((rp.height, rp.width, 4), dtype=np.uint8)
    counts = np.empty((rp.height, rp.width), dtype=np.uint32) if want_counts else None
    st = _lib.nb_render_stats()
    check(call(handle, C.byref(p), rgba.ctypes.data, counts.ctypes.data if want_counts else None, C.byref(st)))
    frame = rgba.view(Frame)
    frame.stats = RenderStats._from_c(st)
    return (frame, counts) if want_counts else frame


def write_ppm(path, rgba) -> None:
    """Write an (H, W, 3 or 4) uint8 image as a binary P6 file (the alpha channel is dropped)."""
    a = np.asarray(rgba)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4):
        raise ValueError("write_ppm takes an (H, W, 3 or 4) uint8 array")
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (a.shape[1], a.shape[0]))
        f.write(np.ascontiguousarray(a[:, :, :3]).tobytes())


def version() -> str:
    return _lib.lib().nb_version().decode()


def device_count() -> int:
    return int(_lib.lib().nb_device_count())


def shard_bodies_per_rank(particle_num: int, world: int) -> int:
    return int(_lib.lib().nb_shard_bodies_per_rank(particle_num, world))


def shard_padded_bodies(particle_num: int, world: int) -> int:
    return int(_lib.lib().nb_shard_padded_bodies(particle_num, world))


def naive_variants() -> list:
    L = _lib.lib()
    return [L.nb_naive_variant_name(i).decode() for i in range(L.nb_naive_variant_count())]


def as_particles(a) -> np.ndarray:
    """View/convert an (n,10) float32 array or a structured array as PARTICLE_DTYPE[n]."""
    a = np.asarray(a)
    if a.dtype == PARTICLE_DTYPE:
        return np.ascontiguousarray(a)
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 10:
        raise ValueError("particles must be PARTICLE_DTYPE[n] or float32[n,10]")
    return a.view(PARTICLE_DTYPE).reshape(-1)


def as_floats(p: np.ndarray) -> np.ndarray:
    """PARTICLE_DTYPE[n] -> float32[n,10] view (px py pz vx vy vz ax ay az mass)."""
    return np.ascontiguousarray(p).view(np.float32).reshape(-1, 10)


class _Inits:
    """`mod inits` (src/inits.rs): seeded equivalents of the three distributions.  Each
    function has the reference's shape `fn(&SimParams) -> Vec<Particle>`; the seed (the
    reference uses the unseedable thread_rng) is an optional keyword."""

    @staticmethod
    def _run(name: str, sim_params: SimParams, seed: int) -> np.ndarray:
        out = np.zeros(sim_params.particle_num, dtype=PARTICLE_DTYPE)
        cp = sim_params.to_c()
        s = C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)
        getattr(_lib.lib(), name)(C.byref(cp), out.ctypes.data, C.cast(C.byref(s), C.c_void_p))
        return out

    def uniform_init(self, sim_params: SimParams, seed: int = 0) -> np.ndarray:
        return self._run("nb_init_uniform", sim_params, seed)        # inits.rs:6-27

    def disc_init(self, sim_params: SimParams, seed: int = 0) -> np.ndarray:
        return self._run("nb_init_disc", sim_params, seed)           # inits.rs:29-54

    def spherical_init(self, sim_params: SimParams, seed: int = 0) -> np.ndarray:
        return self._run("nb_init_spherical", sim_params, seed)      # inits.rs:56-83


inits = _Inits()


def _init_trampoline(init_fn: InitFn, sim_params: SimParams):
    """Wrap a Python `init_fn(sim_params) -> particles` as an nb_init_fn C callback."""
    err = []

    def trampoline(_params_ptr, out_ptr, _user):
        try:
            arr = as_particles(init_fn(sim_params))
            if arr.shape[0] != sim_params.particle_num:
                raise ValueError(f"init_fn returned {arr.shape[0]} particles, expected "
                                 f"{sim_params.particle_num}")
            C.memmove(out_ptr, arr.ctypes.data, arr.nbytes)
        except BaseException as ex:  # never unwind through C
            err.append(ex)

    return _lib.NB_INIT_FN(trampoline), err


class _Passes:
    """The analysis passes of the current state, once for Simulator (nb_sim_*) and OfflineHeadless (nb_runner_*: the
    same pass on the runner's simulator).  The two differ in the ABI prefix and in read_particles()."""

    _ABI: str

    def _pass(self, name: str):
        return getattr(_lib.lib(), self._ABI + name)

    def diagnostics(self, potential: bool = False) -> Diagnostics:
        """Energy, momentum and angular momentum of the current state (nb_sim_diagnostics); with
        potential=True also the exact O(N^2) pair potential.  A several-GPU runner refuses."""
        d = _lib.nb_diagnostics()
        check(self._pass("diagnostics")(self._h, _diag_flags(potential), C.byref(d)))
        return Diagnostics._from_c(d)

    def radial_profile(self, edges=None, *, nbins: int = 64, rmin=None, rmax=None, log: bool = True,
                       cylindrical: bool = False, axis=(0.0, 1.0, 0.0), center="com",
                       velocity=(0.0, 0.0, 0.0)) -> RadialProfile:
        """Per-shell mass and velocity moments of the current state (nb_sim_radial_profile).  edges: the
        nbins + 1 radii, or rmin, rmax, nbins and log for radial_edges().  cylindrical: bin by distance
        from `axis` through the centre (a disc's annuli) instead of from the centre.  center: "com" (the
        centre of mass and its velocity P/M, as diagnostics() returns them) or three coordinates, then
        with `velocity` as the centre's velocity; "density": the density centre and its velocity of
        knn_density(6), passed on as explicit values.  A several-GPU runner refuses."""
        if isinstance(center, str) and center == "density":
            d = self.knn_density(6, neighbours=False)
            center, velocity = d.center, d.center_velocity
        return _radial_profile(self._pass("radial_profile"), self._h, edges, nbins, rmin, rmax, log,
                               cylindrical, axis, center, velocity)

    def disc_modes(self, edges=None, *, nbins: int = 32, rmin=None, rmax=None, log: bool = False, mmax: int = 4,
                   axis=(0.0, 1.0, 0.0), center="com", velocity=None) -> DiscModes:
        """The azimuthal Fourier sums of the current state per annulus about `axis` (nb_disc_modes_sim): bar strength,
        phases, pattern speeds, bending modes and thickness are methods of the DiscModes it returns.  edges: the
        nbins + 1 cylindrical radii, or rmin, rmax, nbins and log for radial_edges().  mmax: the highest mode, 0 to 8.
        center: "com" (the centre of mass and its velocity P/M, as diagnostics() returns them), three coordinates,
        then with `velocity` as the frame's velocity (default: at rest), or "density": the density centre and its
        velocity of knn_density(6), passed on as explicit values.  A several-GPU runner refuses."""
        if isinstance(center, str) and center == "density":
            if velocity is not None:
                raise ValueError('center="density" brings its own velocity')
            d = self.knn_density(6, neighbours=False)
            center, velocity = d.center, d.center_velocity
        suffix = "sim" if self._ABI == "nb_sim_" else "runner"  # (the noun-first names of include/nbody.h)
        return _disc_modes(getattr(_lib.lib(), "nb_disc_modes_" + suffix), self._h, self.sim_params().dt, edges,
                           nbins, rmin, rmax, log, mmax, axis, center, velocity)

    def shell_modes(self, edges=None, *, nbins: int = 32, rmin=None, rmax=None, log: bool = True, lmax: int = 4,
                    rates: bool = False, axis=(0.0, 1.0, 0.0), center="com", velocity=None) -> ShellModes:
        """The spherical-harmonic sums of the current state per radial shell (nb_shell_modes_sim): the power per
        degree l, the l = 1 vector, the l = 2 axes, phases and pattern speeds are methods of the ShellModes it
        returns.  edges: the nbins + 1 radii, or rmin, rmax, nbins and log for radial_edges().  lmax: the highest
        degree, 0 to 6, with rates=True (the time derivative of every sum too) 0 to 4.  axis: the polar axis.
        center: "com" (the centre of mass and its velocity P/M, as diagnostics() returns them), three coordinates,
        then with `velocity` as the frame's velocity (default: at rest), or "density": the density centre and its
        velocity of knn_density(6), passed on as explicit values.  A several-GPU runner refuses."""
        if isinstance(center, str) and center == "density":
            if velocity is not None:
                raise ValueError('center="density" brings its own velocity')
            d = self.knn_density(6, neighbours=False)
            center, velocity = d.center, d.center_velocity
        suffix = "sim" if self._ABI == "nb_sim_" else "runner"  # (the noun-first names of include/nbody.h)
        return _shell_modes(getattr(_lib.lib(), "nb_shell_modes_" + suffix), self._h, self.sim_params().dt, edges,
                            nbins, rmin, rmax, log, lmax, rates, axis, center, velocity)

    def field(self, points, *, accel: bool = True, potential: bool = True) -> Field:
        """The exact acceleration and potential of the current state at `points` ((M, 3), float32), summed
        over all bodies on the device (nb_sim_field).  A body at a point itself adds nothing and is counted
        in `.coincident`, so the field at a body's position is the field of the others.
        A several-GPU runner refuses."""
        return _field(self._pass("field"), self._h, points, accel, potential)

    def circular_velocity(self, radii, *, axis=(0.0, 1.0, 0.0), center=(0.0, 0.0, 0.0), n_phi: int = 16,
                          potential: bool = False) -> RingMeans:
        """The rotation curve from the force: field() on n_phi points of each ring of field_rings(), then
        the ring means (nb_field_ring_means): v_c = sqrt(max(0, -R a_R)).  A several-GPU runner refuses."""
        return _circular_velocity(self._pass("field"), self._h, radii, axis, center, n_phi, potential)

    def tidal_tensor(self, points) -> TidalField:
        """The exact tidal tensor T_ab = d acc_a / d x_b of the current state at `points` ((M, 3), float32), summed
        pair by pair over all bodies on the device (nb_tidal_sim): whether a clump is stretched or compressed by the
        rest of the system (eigenvalues(), compressive_axes()).  A body at a point itself adds nothing and is counted
        in `.coincident`.  A several-GPU runner refuses."""
        suffix = "sim" if self._ABI == "nb_sim_" else "runner"  # (the noun-first names of include/nbody.h)
        return _tidal_tensor(getattr(_lib.lib(), "nb_tidal_" + suffix), self._h, points)

    def disc_frequencies(self, radii, *, axis=(0.0, 1.0, 0.0), center=(0.0, 0.0, 0.0),
                         n_phi: int = 16) -> DiscFrequencies:
        """Omega(R), the epicyclic frequency kappa(R) and the vertical frequency nu(R) of a disc about `axis` through
        `center`: field() and tidal_tensor() on n_phi points of each ring of field_rings(), then the ring means
        (nb_field_ring_means, nb_tidal_ring_means).  DiscFrequencies.resonances() sets them against a pattern speed
        of disc_modes().  A several-GPU runner refuses."""
        suffix = "sim" if self._ABI == "nb_sim_" else "runner"  # (the noun-first names of include/nbody.h)
        return _disc_frequencies(self._pass("field"), getattr(_lib.lib(), "nb_tidal_" + suffix), self._h, radii, axis,
                                 center, n_phi)

    def _accel_scale(self, coupling) -> float:
        if isinstance(coupling, str):
            if coupling == "field":
                return 1.0
            if coupling == "step":
                return float(self.sim_params().dt)
            raise ValueError('coupling is "field", "step" or a number')
        return float(coupling)

    def orbits(self, pos, vel, *, dt: float, steps: int, every: int = 1, energy: bool = False, omega: float = 0.0,
               axis=(0.0, 1.0, 0.0), center=(0.0, 0.0, 0.0), coupling="field", step0: int = 0) -> Orbits:
        """Test particles from `pos`, `vel` ((M, 3), float64) through `steps` leapfrog steps of `dt` in the frozen
        field of the current state (nb_orbits_sim): the tracers stay on the device and every step is enqueued up
        front.  omega: the pattern speed (DiscModes.pattern_speed) at which the frozen bodies turn rigidly about `axis`
        through `center`; 0 holds them at rest.  A state is recorded every `every` steps and at the end;
        energy=True also records the potential and the Jacobi integral.  coupling sets the acceleration's scale:
        "field" is field()'s own (the convention of circular_velocity() and disc_frequencies()), "step" multiplies it
        by the simulator's dt, the g dt with which its own bodies move (the diagnostics' coupling); a number is used
        as given.  step0 numbers the first state, so that Orbits.final() continues a run exactly.  A several-GPU
        runner refuses."""
        suffix = "sim" if self._ABI == "nb_sim_" else "runner"  # (the noun-first names of include/nbody.h)
        return _orbits(getattr(_lib.lib(), "nb_orbits_" + suffix), self._h, pos, vel, dt, steps, every, energy, omega,
                       axis, center, self._accel_scale(coupling), step0)

    def circular_orbits(self, radii, *, dt: float, steps: int, axis=(0.0, 1.0, 0.0), center=(0.0, 0.0, 0.0),
                        n_phi: int = 16, speed: float = 1.0, **kw) -> Orbits:
        """orbits() of one tracer per radius, started at the first point of its field_rings() ring with `speed` times
        the circular velocity of circular_velocity() (field()'s coupling) along the direction of rotation there:
        speed = 1 is the circular orbit of the azimuthally averaged force.  The other arguments are orbits()'s."""
        r = np.ascontiguousarray(np.atleast_1d(radii), dtype=np.float64)
        cv = self.circular_velocity(r, axis=axis, center=center, n_phi=n_phi)
        pts = field_rings(r, axis=axis, center=center, n_phi=n_phi)
        _, _, e2 = map_frame(axis)
        pos = pts[:: max(int(n_phi), 1)].astype(np.float64)
        vel = (float(speed) * cv.v_c)[:, None] * e2[None, :]
        return self.orbits(pos, vel, dt=dt, steps=steps, axis=axis, center=center, **kw)

    def orbit_sections(self, pos, vel, *, dt: float, steps: int, normal=(0.0, 1.0, 0.0), offset: float = 0.0,
                       direction: int = 1, max_crossings: int = 256, every=None, energy: bool = False,
                       omega: float = 0.0, axis=(0.0, 1.0, 0.0), center=(0.0, 0.0, 0.0), coupling="field",
                       step0: int = 0) -> OrbitSections:
        """orbits() whose step kernel also takes a surface of section and a summary per tracer
        (nb_orbit_sections_sim): every crossing of the plane normal . xi = offset of the pattern frame -- xi = (a', b',
        l) in map_frame(axis) about `center`, turned with the pattern -- interpolated linearly between the two states
        around it, the first `max_crossings` per tracer stored; and peri- and apocentres, extrema of r, R, |l| and L_z
        and the windings about the axis, counted over every step.  direction: +1 keeps the crossings towards positive
        normal . xi, -1 the others, 0 both.  every=None records the two end states only; the other arguments are
        orbits()'s, and no launch is added to that call's.  A several-GPU runner refuses."""
        suffix = "sim" if self._ABI == "nb_sim_" else "runner"  # (the noun-first names of include/nbody.h)
        return _orbit_sections(getattr(_lib.lib(), "nb_orbit_sections_" + suffix), self._h, pos, vel, dt, steps,
                               normal, offset, direction, max_crossings, every, energy, omega, axis, center,
                               self._accel_scale(coupling), step0)

    def orbit_stability(self, pos, vel, *, dt: float, steps: int, deviations=2, renorm_log2: int = 32, every=None,
                        log2_0=None, omega: float = 0.0, axis=(0.0, 1.0, 0.0), center=(0.0, 0.0, 0.0),
                        coupling="field", step0: int = 0) -> OrbitStability:
        """orbits() that also carries deviation vectors along every orbit by the tangent map of its step
        (nb_orbit_stability_sim): one pair kernel sums the acceleration and the tidal tensor at each evaluation point,
        and the step kernel moves the vectors, renormalising each by an exact power of two whenever its largest
        component leaves [2^-renorm_log2, 2^renorm_log2).  deviations: a count D (1..6) of orthonormal vectors from
        numpy.random.default_rng(0), the same for every tracer, or an (M, D, 6) array of (dx, dv); log2_0: their
        starting exponents (default 0).  every=None records the two end states only.  OrbitStability gives the
        finite-time Lyapunov exponents, SALI and GALI_2; `.orbits` is orbits()'s result for the same arguments, bit for
        bit; final() continues a run exactly.  The other arguments are orbits()'s; the energy is not taken.  A
        several-GPU runner refuses."""
        suffix = "sim" if self._ABI == "nb_sim_" else "runner"  # (the noun-first names of include/nbody.h)
        return _orbit_stability(getattr(_lib.lib(), "nb_orbit_stability_" + suffix), self._h, pos, vel, dt, steps,
                                deviations, renorm_log2, every, log2_0, omega, axis, center,
                                self._accel_scale(coupling), step0)

    def jacobi_launch(self, energy: float, a, *, omega: float, axis=(0.0, 1.0, 0.0), center=(0.0, 0.0, 0.0),
                      coupling="field"):
        """(pos, vel), inertial, of tracers that all have the Jacobi integral `energy`: on the pattern's a' axis at
        a' = `a` (an array), b' = l = 0, moving along b' alone in the pattern frame with
        b'' = sqrt(2 (E_J - Phi_eff)), Phi_eff = Phi - omega^2 a'^2 / 2, Phi the potential of field() at the point an
        orbits() call samples at state 0 of step0 = 0 (where the two frames coincide).  Where Phi_eff > E_J the
        position is forbidden and both rows are NaN.  Every curve of one orbit_sections() plot then shares E_J."""
        a = np.ascontiguousarray(np.atleast_1d(a), dtype=np.float64)
        n, e1, e2 = map_frame(axis)
        c = np.asarray(center, dtype=np.float64)
        omega, scale = float(omega), self._accel_scale(coupling)
        pos = c + a[:, None] * e1
        q = pos
        if omega != 0.0:  # the point of evaluation 0, line by line
            d = pos - c
            da, db, dl = ((d[:, 0] * f[0] + d[:, 1] * f[1]) + d[:, 2] * f[2] for f in (e1, e2, n))
            ar, br = da * 1.0 + db * 0.0, db * 1.0 - da * 0.0
            q = c + ((ar[:, None] * e1 + br[:, None] * e2) + dl[:, None] * n)
        with np.errstate(all="ignore"):
            phi = scale * self.field(q.astype(np.float32), accel=False, potential=True).potential
            phi_eff = phi - 0.5 * (omega * omega) * (a * a)
            speed = np.sqrt(2.0 * (float(energy) - phi_eff))
        vel = (speed + omega * a)[:, None] * e2
        bad = ~np.isfinite(speed)
        pos[bad], vel[bad] = np.nan, np.nan
        return pos, vel

    def projected_map(self, width: int, height: int, *, extent, axis=(0.0, 1.0, 0.0), center="com", velocity=None,
                      depth=None, velocities: bool = True) -> ProjectedMap:
        """Per-cell count, mass and velocity moments of the current state on a width x height grid seen
        along `axis` (nb_sim_map).  extent: (x0, x1, y0, y1), the window [x0, x1) x [y0, y1) in the plane
        coordinates of map_frame(axis) about the centre.  center: "com" (the centre of mass and its
        velocity P/M, as diagnostics() returns them) or three coordinates, then with `velocity` (default:
        at rest); "density": the density centre and its velocity of knn_density(6), passed on as explicit
        values.  depth: (lo, hi) keeps the bodies with lo <= h < hi along the line of sight.
        velocities=False returns the counts and the mass alone.  A several-GPU runner refuses."""
        if isinstance(center, str) and center == "density":
            if velocity is not None:
                raise ValueError('center="density" brings its own velocity')
            d = self.knn_density(6, neighbours=False)
            center, velocity = d.center, d.center_velocity
        return _projected_map(self._pass("map"), self._h, width, height, extent, axis, center, velocity, depth,
                              velocities)

    def phase_map(self, x: str, y: str, *, x_edges=None, y_edges=None, x_range=None, y_range=None, bins=(128, 128),
                  log=(False, False), weight: Optional[str] = None, values=None, axis=(0.0, 1.0, 0.0), center="com",
                  velocity=None, check_step=True) -> PhaseMap:
        """The 2-D histogram of the current state on two per-body quantities (nb_phase_map_sim): x and y are names
        of phase_quantities() -- "a", "b", "h", "R", "r", "ua", "ub", "w", "u_R", "u_phi", "u_r", "u_t", "speed",
        "j_z", "j", "e_kin", "mass", "value" -- in the frame of map_frame(axis) about the centre.  Per side either
        the edges (strictly ascending; the first may be -inf, the last +inf) or a range (lo, hi) with bins[side]
        cells, log[side] for a constant ratio (phase_edges()).  weight: a third quantity whose mass-weighted mean
        and dispersion per cell the PhaseMap gives.  values: one float64 per body of read_particles() now, the
        quantity "value" (a potential from field(), a density from knn_density(), an energy from bound_groups()).
        center: "com" (the centre of mass and its velocity P/M, as diagnostics() returns them), three coordinates,
        then with `velocity` (default: at rest), or "density": the density centre and its velocity of
        knn_density(6), passed on as explicit values.  check_step: True takes `values` as made from the state as it
        is now; a step number names the step they were made at, to have stale ones refused (a TreeSim reorders its
        bodies every step); False: not checked.  A several-GPU runner refuses."""
        if isinstance(center, str) and center == "density":
            if velocity is not None:
                raise ValueError('center="density" brings its own velocity')
            d = self.knn_density(6, neighbours=False)
            center, velocity = d.center, d.center_velocity
        xe = _phase_side("x", x_edges, x_range, bins[0], log[0])
        ye = _phase_side("y", y_edges, y_range, bins[1], log[1])
        suffix = "sim" if self._ABI == "nb_sim_" else "runner"  # (the noun-first names of include/nbody.h)
        return _phase_map(getattr(_lib.lib(), "nb_phase_map_" + suffix), self._h,
                          int(self.sim_params().particle_num), int(self.step_num()), x, y, xe, ye, weight, values, axis,
                          center, velocity, check_step)

    def distribution(self, x: str, edges, **kw) -> PhaseMap:
        """The 1-D distribution of quantity x over `edges`: a phase map of height 1 with y = "mass" on the edges
        (-inf, +inf); the other arguments are phase_map's.  counts[0], mass[0] and marginal_x() are the histogram."""
        return self.phase_map(x, "mass", x_edges=edges, y_edges=(-np.inf, np.inf), **kw)

    def fof_groups(self, link: float, *, min_members: int = 20, labels: bool = True) -> FofGroups:
        """The friends-of-friends groups of the current state (nb_sim_fof): bodies within `link` of each
        other are friends, a group is a connected component; the catalogue holds the groups of at least
        min_members bodies.  The body indices are those of read_particles() now: a TreeSim reorders its
        bodies at every step.  labels=False leaves the per-body labels on the device.  A several-GPU runner refuses."""
        return _fof_groups(self._pass("fof"), self._h, int(self.sim_params().particle_num), link, min_members,
                           labels)

    def spanning_tree(self, *, degree: bool = True) -> SpanningTree:
        """The Euclidean minimum spanning tree of the current state (nb_mst_sim): its edges in ascending order are the
        single-linkage hierarchy, so .cut(link) gives fof_groups(link, min_members=1)'s labels for every link at
        once, .group_counts(links) the percolation curve and .linkage() the dendrogram.  The body indices are those
        of read_particles() now.  A several-GPU runner refuses."""
        suffix = "sim" if self._ABI == "nb_sim_" else "runner"  # (the noun-first names of include/nbody.h)
        return _spanning_tree(getattr(_lib.lib(), "nb_mst_" + suffix), self._h,
                              int(self.sim_params().particle_num), degree)

    def phase_space_groups(self, link: float, vlink: float, *, min_members: int = 20,
                           labels: bool = True) -> PhaseSpaceGroups:
        """The phase-space groups of the current state (nb_fof6_sim): friends-of-friends in position and velocity.
        Bodies within `link` of each other with (dx / link)^2 + (dv / vlink)^2 <= 1 are friends, a group is a
        connected component; the catalogue holds the groups of at least min_members bodies.  Two streams that cross,
        or a cold clump inside a hot halo, are one group to fof_groups(link) and separate ones here.  The body indices
        are those of read_particles() now.  labels=False leaves the per-body labels on the device.
        A several-GPU runner refuses."""
        suffix = "sim" if self._ABI == "nb_sim_" else "runner"  # (the noun-first names of include/nbody.h)
        return _phase_space_groups(getattr(_lib.lib(), "nb_fof6_" + suffix), self._h,
                                   int(self.sim_params().particle_num), link, vlink, min_members, labels)

    def bound_groups(self, link: float, *, min_members: int = 20, min_bound: Optional[int] = None,
                     max_iter: int = 32, max_group: int = 262144, per_body: bool = True) -> BoundGroups:
        """The friends-of-friends groups of the current state (as fof_groups(link, min_members=...)), each
        unbound on the device (nb_sim_bound): round by round the members with positive energy in the group's
        own frame leave, until nobody does, fewer than min_bound (default min_members) are left, or max_iter
        rounds have run.  A group of more than max_group members (0: no limit) is skipped: a round costs
        count^2 pair terms.  per_body=False leaves bound_of and energy on the device.  A several-GPU runner refuses."""
        return _bound_groups(self._pass("bound"), self._h, int(self.sim_params().particle_num), link,
                             min_members, min_bound, max_iter, max_group, per_body)

    def hop_groups(self, *, k_density: int = 64, k_hop: int = 16, k_merge: int = 4, min_members: int = 1,
                   density_min=None, labels: bool = True, density: bool = False, boundaries: bool = True) -> HopGroups:
        """The density-peak groups of the current state (nb_sim_hop): knn_density(k_density) orders the bodies,
        every body hops to the densest of its k_hop nearest neighbours until it reaches a peak, and pairs
        among the k_merge nearest neighbours that end at different peaks give the boundaries .regroup() merges
        across.  density_min leaves bodies below it out.  The body indices are those of read_particles() now: a
        TreeSim reorders its bodies at every step.  labels=False and density=False leave the per-body arrays
        on the device, boundaries=False the boundary table.  A several-GPU runner refuses."""
        return _hop_groups(self._pass("hop"), self._h, int(self.sim_params().particle_num), k_density, k_hop,
                           k_merge, min_members, density_min, labels, density, boundaries)

    def knn_density(self, k: int = 6, *, density: bool = True, neighbours: bool = True) -> KnnDensity:
        """The k-th nearest neighbour of every body of the current state, the mass inside it and the density
        from them (nb_sim_knn), with the density-weighted sums: .center is the density centre of Casertano &
        Hut (1985).  The body indices are those of read_particles() now: a TreeSim reorders its bodies at
        every step.  density=False leaves mass_in and density on the device, neighbours=False r2 and kth.
        A several-GPU runner refuses."""
        return _knn_density(self._pass("knn"), self._h, int(self.sim_params().particle_num), k, density,
                            neighbours)

    def local_kinematics(self, k: int = 32, *, gradient: bool = False, include_self: bool = True,
                         neighbours: bool = False) -> LocalKinematics:
        """How the k nearest neighbours of every body of the current state move (nb_local_kinematics_sim, then
        nb_local_kinematics_derive on the host): the local mean velocity, the dispersion tensor and sigma, the
        pseudo-phase-space density rho / sigma^3 with knn_density(k)'s rho, and with gradient=True the least-squares
        velocity gradient with its divergence, vorticity and shear.  include_self: the body's own mass starts the
        mass sum.  neighbours=True also returns kth.  The body indices are those of read_particles() now: a TreeSim
        reorders its bodies at every step.  A several-GPU runner refuses."""
        suffix = "sim" if self._ABI == "nb_sim_" else "runner"  # (the noun-first names of include/nbody.h)
        return _local_kinematics(getattr(_lib.lib(), "nb_local_kinematics_" + suffix), self,
                                 int(self.sim_params().particle_num), k, gradient, include_self, neighbours)

    def halo_profiles(self, centers=None, *, bodies=None, velocities=None, edges=None, nbins: int = 32, rmin=None,
                      rmax=None, log: bool = True) -> HaloProfiles:
        """The spherical radial profile of the current state about many centres at once (nb_sim_halo_profiles):
        centers (m, 3) points, or bodies (m,) body indices whose positions (and, without velocities, velocities)
        are the centres; edges shared by all centres, or rmin, rmax, nbins and log for radial_edges().  A centre
        tests only the bodies of the grid cells its sphere of radius edges[-1] reaches.  The body indices are
        those of read_particles() now: a TreeSim reorders its bodies at every step.  A several-GPU runner refuses."""
        return _halo_profiles(self._pass("halo_profiles"), self._h, centers, bodies, velocities, edges, nbins,
                              rmin, rmax, log)

    def group_profiles(self, groups, *, center: str = "com", **kw):
        """(rows, HaloProfiles): halo_profiles about the groups of a FofGroups or BoundGroups of the same
        state -- center="com": their centres of mass and mean velocities, the rows where those are finite;
        "most_bound": a BoundGroups' most bound bodies, the rows that have one; "peak": a HopGroups' labels, the
        bodies at the density peaks.  rows: the catalogue rows
        the profiles belong to, in order.  kw: edges / nbins / rmin / rmax / log of halo_profiles.
        A several-GPU runner refuses."""
        return _group_profiles(self.halo_profiles, groups, center, kw)

    def shapes_of(self, group_of, m: int, *, centers=None, velocities=None, radius=None, reduced: bool = False,
                  max_iter: int = 32, tol: float = 1e-3, min_members: int = 10, per_body: bool = False,
                  step_num=None, catalogue_rows=None) -> GroupShapes:
        """The shapes of the m rows of a raw assignment (nb_sim_group_shapes): group_of (n,) uint32, FOF_NONE or a
        row < m for every body of read_particles() now.  centers, velocities: (m, 3) or None for the members' own
        centre of mass and mean velocity, formed on the device; radius: None (no cut: one round), a number or (m,);
        reduced: weight the tensor by 1 / rho^2 (needs a radius).  step_num: the step the assignment was made at, to
        have a stale one refused (a TreeSim reorders its bodies every step); None: not checked.
        A several-GPU runner refuses."""
        rows = np.arange(int(m)) if catalogue_rows is None else catalogue_rows
        return _group_shapes(self._pass("group_shapes"), self._h, int(self.sim_params().particle_num), group_of, m,
                             centers, velocities, radius, reduced, max_iter, tol, min_members, per_body, step_num, rows)

    def group_shapes(self, groups, *, members: str = "group", center: str = "com", radius=None, reduced: bool = False,
                     max_iter: int = 32, tol: float = 1e-3, min_members: int = 10, per_body: bool = False,
                     check_step: bool = True) -> GroupShapes:
        """The shapes of the groups of a FofGroups, BoundGroups or HopGroups (raw or regrouped) of the same state:
        axis ratios, principal axes, angular momentum and velocity moments of every group inside an ellipsoid
        deformed to its own shape.  members: "group" (group_of) or "bound" (a BoundGroups' bound_of); center: as
        group_profiles -- "com", "most_bound" or "peak" -- and the rows without a finite centre are left out
        (GroupShapes.catalogue_rows names the ones that stay).  radius: None, a number, one per catalogue row, or
        ("rms", k) for k times the catalogue's rms radius.  check_step: refuse a catalogue made at another step.
        A several-GPU runner refuses."""
        kw = dict(reduced=reduced, max_iter=max_iter, tol=tol, min_members=min_members, per_body=per_body)
        return _shapes_of_groups(self.shapes_of, self.read_particles, groups, members, center, radius, check_step,
                                 kw)

    def radii_of(self, group_of, m: int, *, fractions=(0.1, 0.5, 0.9), centers=None, vmax_skip: int = 10,
                 per_body: bool = False, step_num=None, catalogue_rows=None) -> GroupRadii:
        """The exact mass radii of the m rows of a raw assignment (nb_group_radii_sim): group_of (n,) uint32, FOF_NONE
        or a row < m for every body of read_particles() now.  fractions: 1 to 16 ascending values in (0, 1]; centers:
        (m, 3) or None for the members' own centre of mass, formed on the device (group_shapes' bits); vmax_skip: the
        innermost ranks left out of the peak of M / r; per_body: also every member's rank and enclosed mass.
        step_num: the step the assignment was made at, to have a stale one refused; None: not checked.
        A several-GPU runner refuses."""
        rows = np.arange(int(m)) if catalogue_rows is None else catalogue_rows
        suffix = "sim" if self._ABI == "nb_sim_" else "runner"  # (the noun-first names of include/nbody.h)
        return _group_radii(getattr(_lib.lib(), "nb_group_radii_" + suffix), self._h,
                            int(self.sim_params().particle_num), group_of, m, fractions, centers, vmax_skip, per_body,
                            step_num, rows)

    def group_radii(self, groups, *, members: str = "group", center: str = "com", fractions=(0.1, 0.5, 0.9),
                    vmax_skip: int = 10, per_body: bool = False, check_step: bool = True) -> GroupRadii:
        """The exact mass radii, the half-mass radius and v_max of the groups of a FofGroups, BoundGroups or HopGroups
        (raw or regrouped) of the same state.  members and center: as group_shapes resolves them -- "group" or
        "bound"; "com", "most_bound" or "peak" -- and the rows without a finite centre are left out
        (GroupRadii.catalogue_rows names the ones that stay).  check_step: refuse a catalogue made at another step.
        A several-GPU runner refuses."""
        mapped, rows, c, _ = _catalogue_assignment("group_radii", self.read_particles, groups, members, center)
        return self.radii_of(mapped, len(rows), fractions=fractions, centers=c, vmax_skip=vmax_skip,
                             per_body=per_body, step_num=groups.stats.step_num if check_step else None,
                             catalogue_rows=rows)

    def lagrangian_radii(self, fractions=(0.01, 0.05, 0.1, 0.25, 0.5, 0.75, 0.9), *, center="com",
                         vmax_skip: int = 10, per_body: bool = False) -> GroupRadii:
        """The exact Lagrangian radii of the whole state, taken as one row (nb_group_radii_sim): .radius[0] are the
        radii of the bodies at which the enclosed mass reaches each fraction.  center: "com" (the row's own centre of
        mass, formed on the device), "density" (knn_density(6)'s density centre) or three coordinates.
        A several-GPU runner refuses."""
        n = int(self.sim_params().particle_num)
        if isinstance(center, str):
            if center == "com":
                c = None
            elif center == "density":
                c = np.asarray(self.knn_density(6, neighbours=False).center, dtype=np.float64).reshape(1, 3)
            else:
                raise ValueError('lagrangian_radii: center is "com", "density" or three coordinates')
        else:
            c = np.asarray(center, dtype=np.float64).reshape(1, 3)
        return self.radii_of(np.zeros(n, dtype=np.uint32), 1, fractions=fractions, centers=c, vmax_skip=vmax_skip,
                             per_body=per_body)

    def smoothed_map(self, width: int, height: int, *, extent, axis=(0.0, 1.0, 0.0), center="com", velocity=None,
                     depth=None, velocities: bool = True, smoothing="knn", k: int = 32, scale: float = 1.0,
                     s_min=None, s_max=None) -> SmoothedMap:
        """The smoothed image of the current state on a width x height grid seen along `axis`
        (nb_sim_smooth_map): every body spread over the pixels whose centre lies within its smoothing length.
        extent, axis, center, velocity, depth, velocities: as projected_map (center="density" is not offered).
        smoothing: "knn" (scale times the distance to the k-th neighbour, from knn_density(k) on the same
        state), an array of n lengths in the order of read_particles() now, or one length for all.  s_min,
        s_max: the lengths are raised and lowered to these; default 2 and 64 times the larger side of a pixel.
        A several-GPU runner refuses."""
        n = int(self.sim_params().particle_num)
        s = _smoothing_lengths(self, smoothing, k, scale)
        return _smoothed_map(self._pass("smooth_map"), self._h, n, s, width, height, extent, axis, center,
                             velocity, depth, velocities, s_min, s_max)

    def render(self, width: int, height: int, camera: Optional[Camera] = None, view_proj=None,
               counts: bool = False, **params):
        """The current state drawn on the device (nb_sim_render; OnlineRenderer::render,
        online_renderer.rs:331-367): a Frame, the (H, W, 4) uint8 image with .stats; with counts=True
        (frame, counts), counts the (H, W) uint32 coverage image.  camera: a Camera (default: the
        reference's); view_proj: 16 floats, column-major, instead; params: half_size, clear, alpha,
        srgb of RenderParams.  A several-GPU runner refuses."""
        return _render(self._pass("render"), self._h, _render_params(width, height, camera, view_proj, params),
                       counts)


class Simulator(_Passes):
    """`trait Simulator` (sims/mod.rs:73-90) over an nb_sim handle."""

    KIND = NB_NAIVE_SIM_PARAMS
    _ABI = "nb_sim_"

    def __init__(self, handle: int, borrowed: bool = False):
        self._h = C.c_void_p(handle)
        self._borrowed = borrowed  # owned by an nb_runner

    # -- Simulator::new(device, sim_params, add_params, mappable_primary_buffers, init_fn) --
    @classmethod
    def new(cls, sim_params: SimParams, add_params: Optional[AddParams], init_fn: InitFn,
            placement: Optional[Placement] = None) -> "Simulator":
        L = _lib.lib()
        if add_params is None:
            add_params = AddParams(cls.KIND, 0.0)
        if add_params.kind != cls.KIND and cls is not Simulator:
            # the reference's TreeSim::new accepts any AddParams and falls back to theta
            # 0.75 with a warning (tree.rs:42-51); mirror that
            add_params = AddParams(cls.KIND, 0.0)
        sp, ap = sim_params.to_c(), add_params.to_c()
        pl = (placement or Placement()).to_c()
        cb, err = _init_trampoline(init_fn, sim_params)
        h = C.c_void_p()
        rc = L.nb_sim_create(C.byref(h), C.byref(sp), C.byref(ap), C.byref(pl),
                             C.cast(cb, C.c_void_p), None)
        if err:
            if rc == 0:
                L.nb_sim_destroy(h)
            raise err[0]
        check(rc)
        return cls(h.value)

    @classmethod
    def from_particles(cls, sim_params: SimParams, add_params: Optional[AddParams], particles,
                       placement: Optional[Placement] = None) -> "Simulator":
        L = _lib.lib()
        if add_params is None:
            add_params = AddParams(cls.KIND, 0.0)
        arr = as_particles(particles)
        sp, ap = sim_params.to_c(), add_params.to_c()
        pl = (placement or Placement()).to_c()
        h = C.c_void_p()
        check(L.nb_sim_create_from_particles(C.byref(h), C.byref(sp), C.byref(ap), C.byref(pl),
                                             arr.ctypes.data, arr.shape[0]))
        return cls(h.value)

    # -- Simulator::encode (+ queue.submit): enqueue one step, do not wait --
    def encode(self) -> None:
        check(_lib.lib().nb_sim_encode(self._h))

    def encode_phase(self, phase: int) -> None:
        """Half a step (nb_sim_encode_phase): 0 = own bodies' tiles, 1 = the rest + integrate."""
        check(_lib.lib().nb_sim_encode_phase(self._h, int(phase)))

    def let_set_imports(self, counts) -> None:
        """LET protocol (nb_sim_let_set_imports): records received from every rank this step."""
        arr = (C.c_uint32 * len(counts))(*[int(c) for c in counts])
        check(_lib.lib().nb_sim_let_set_imports(self._h, arr, len(counts)))

    def let_set_import_stride(self, stride: int) -> None:
        """LET protocol without a host round trip (nb_sim_let_set_import_stride): this step's imports
        are fixed-stride segments, their counts are read on the device."""
        check(_lib.lib().nb_sim_let_set_import_stride(self._h, int(stride)))

    def let_set_owners(self, splits, ref_bound: float, seg_cap: int) -> None:
        """LET migration (nb_sim_let_set_owners): rank r owns reference keys [splits[r-1], splits[r])."""
        world = len(splits) + 1
        arr = (C.c_ulonglong * max(1, len(splits)))(*[int(x) for x in splits])
        check(_lib.lib().nb_sim_let_set_owners(self._h, arr, world, float(ref_bound), int(seg_cap)))

    def let_set_arrivals(self, stay: int, counts) -> None:
        """LET migration (nb_sim_let_set_arrivals): bodies kept, bodies received from every rank."""
        arr = (C.c_uint32 * len(counts))(*[int(c) for c in counts])
        check(_lib.lib().nb_sim_let_set_arrivals(self._h, int(stay), arr, len(counts)))

    # -- Simulator::cleanup --
    def cleanup(self) -> None:
        check(_lib.lib().nb_sim_cleanup(self._h))

    # -- device.poll(Maintain::Wait) --
    def wait(self) -> None:
        check(_lib.lib().nb_sim_wait(self._h))

    # -- Simulator::sim_params --
    def sim_params(self) -> SimParams:
        sp = _lib.nb_sim_params()
        check(_lib.lib().nb_sim_sim_params(self._h, C.byref(sp)))
        return SimParams(sp.particle_num, sp.g, sp.e, sp.dt)

    # -- Simulator::dest_particle_slice: here the POST-step state, copied to the host --
    def dest_particle_slice(self) -> np.ndarray:
        n = self.sim_params().particle_num
        out = np.zeros(n, dtype=PARTICLE_DTYPE)
        check(_lib.lib().nb_sim_read_particles(self._h, out.ctypes.data, n))
        return out

    read_particles = dest_particle_slice

    def write_particles(self, particles) -> None:
        arr = as_particles(particles)
        check(_lib.lib().nb_sim_write_particles(self._h, arr.ctypes.data, arr.shape[0]))

    def step_num(self) -> int:
        v = C.c_uint64()
        check(_lib.lib().nb_sim_step_num(self._h, C.byref(v)))
        return int(v.value)

    def encode_n_timed(self, n: int):
        """n steps back to back -> (ms_total, ms_mean_force_kernel), HIP-event timed."""
        a, b = C.c_float(), C.c_float()
        check(_lib.lib().nb_sim_encode_n_timed(self._h, n, C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)

    def exchange_region(self, index: int = 0):
        """(device_ptr, offset_bytes, slice_bytes, total_bytes) of exchange region `index`."""
        p, o, s, t = C.c_void_p(), C.c_size_t(), C.c_size_t(), C.c_size_t()
        check(_lib.lib().nb_sim_exchange_region_i(self._h, int(index), C.byref(p), C.byref(o),
                                                  C.byref(s), C.byref(t)))
        return int(p.value or 0), int(o.value), int(s.value), int(t.value)

    def exchange_count(self) -> int:
        c = C.c_int()
        check(_lib.lib().nb_sim_exchange_count(self._h, C.byref(c)))
        return int(c.value)

    def set_tuning(self, key: str, value: int) -> None:
        check(_lib.lib().nb_sim_set_tuning(self._h, key.encode(), int(value)))

    def debug_buffer(self, name: str, dtype) -> np.ndarray:
        """Testing hook (nb_sim_debug_buffer): a named internal device buffer as a numpy array."""
        nbytes = C.c_size_t()
        check(_lib.lib().nb_sim_debug_buffer(self._h, name.encode(), None, 0, C.byref(nbytes)))
        out = np.zeros(nbytes.value // np.dtype(dtype).itemsize, dtype=dtype)
        check(_lib.lib().nb_sim_debug_buffer(self._h, name.encode(), out.ctypes.data, out.nbytes,
                                             C.byref(nbytes)))
        return out

    def read_tree(self):
        """TreeSim: (octants[n_nodes], root_width) of the tree the last step built."""
        n = self.sim_params().particle_num
        cap = max(4 * n, 8)
        buf = np.zeros(cap, dtype=OCTANT_DTYPE)
        nn, rw = C.c_size_t(), C.c_float()
        check(_lib.lib().nb_sim_read_tree(self._h, buf.ctypes.data, cap, C.byref(nn), C.byref(rw)))
        return buf[: nn.value].copy(), float(rw.value)

    def tree_node_count(self) -> int:
        """TreeSim: number of octants of the tree the last step built (no copy of the tree)."""
        nn, rw = C.c_size_t(), C.c_float()
        check(_lib.lib().nb_sim_read_tree(self._h, None, 0, C.byref(nn), C.byref(rw)))
        return int(nn.value)

    def destroy(self) -> None:
        if self._h and not self._borrowed:
            _lib.lib().nb_sim_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class NaiveSim(Simulator):
    """`NaiveSim` (sims/naive.rs): all-pairs O(N^2)."""
    KIND = NB_NAIVE_SIM_PARAMS


class TreeSim(Simulator):
    """`TreeSim` (sims/tree.rs): Barnes-Hut octree."""
    KIND = NB_TREE_SIM_PARAMS


class OfflineHeadless(_Passes):
    """`OfflineHeadless<T: Simulator>` (runners/offline_headless.rs:4-45) over nb_runner.

    OfflineHeadless(NaiveSim, sim_params, add_params, init_fn) ~
    OfflineHeadless::<NaiveSim>::new(sim_params, add_params, init_fn)."""

    _ABI = "nb_runner_"

    def __init__(self, sim_type, sim_params: SimParams, add_params: Optional[AddParams],
                 init_fn: InitFn, device_id: int = -1, device_ids: Optional[Sequence[int]] = None,
                 let_migrate_every: Optional[int] = None):
        """device_ids: several GPUs of this process (nb_runner_create_multi; all-pairs: body ranges +
        peer stores, TreeSim: replicated tree + partitioned walk): rank r owns a contiguous body
        range on device_ids[r]; a device id may repeat.  let_migrate_every (TreeSim, with device_ids):
        Morton domains + LET exchange instead (nb_runner_create_multi_let)."""
        L = _lib.lib()
        if add_params is None or add_params.kind != sim_type.KIND:
            add_params = AddParams(sim_type.KIND, 0.0)
        sp, ap = sim_params.to_c(), add_params.to_c()
        cb, err = _init_trampoline(init_fn, sim_params)
        h = C.c_void_p()
        if device_ids is not None:
            ids = (C.c_int * len(device_ids))(*[int(d) for d in device_ids])
            if let_migrate_every is not None:
                rc = L.nb_runner_create_multi_let(C.byref(h), C.byref(sp), C.byref(ap), C.cast(cb, C.c_void_p), None,
                                                  ids, len(device_ids), int(let_migrate_every))
            else:
                rc = L.nb_runner_create_multi(C.byref(h), C.byref(sp), C.byref(ap), C.cast(cb, C.c_void_p), None,
                                              ids, len(device_ids))
        else:
            rc = L.nb_runner_create(C.byref(h), C.byref(sp), C.byref(ap), C.cast(cb, C.c_void_p), None,
                                    int(device_id))
        if err:
            if rc == 0:
                L.nb_runner_destroy(h)
            raise err[0]
        check(rc)
        self._h = h
        sim_h = L.nb_runner_sim(h)                 # NULL for a several-GPU runner
        self.sim = sim_type(sim_h, borrowed=True) if sim_h else None

    @classmethod
    def new(cls, sim_type, sim_params, add_params, init_fn, device_id: int = -1, device_ids=None,
            let_migrate_every=None):
        return cls(sim_type, sim_params, add_params, init_fn, device_id, device_ids, let_migrate_every)

    def step_num(self) -> int:
        v = C.c_uint64()
        check(_lib.lib().nb_runner_step_num(self._h, C.byref(v)))
        return int(v.value)

    def step(self) -> None:
        """offline_headless.rs:38-44: encode -> submit -> cleanup -> poll(Wait)."""
        check(_lib.lib().nb_runner_step(self._h))

    def step_n(self, n: int) -> None:
        check(_lib.lib().nb_runner_step_n(self._h, int(n)))

    def set_profiling(self, on: bool = True) -> None:
        """Measurement: timing events around every rank's kernels and its waits for the peers."""
        check(_lib.lib().nb_runner_set_profiling(self._h, 1 if on else 0))

    def rank_times(self, world: int):
        """(kernel_ms[world], wait_ms[world]) of the last step_n() with profiling on."""
        k, w = (C.c_float * world)(), (C.c_float * world)()
        check(_lib.lib().nb_runner_rank_times(self._h, k, w, world))
        return [float(x) for x in k], [float(x) for x in w]

    def read_particles(self) -> np.ndarray:
        n = self.sim_params().particle_num
        out = np.zeros(n, dtype=PARTICLE_DTYPE)
        check(_lib.lib().nb_runner_read_particles(self._h, out.ctypes.data, n))
        return out

    def sim_params(self) -> SimParams:
        sp = _lib.nb_sim_params()
        check(_lib.lib().nb_runner_sim_params(self._h, C.byref(sp)))
        return SimParams(sp.particle_num, sp.g, sp.e, sp.dt)

    def destroy(self) -> None:
        if self._h:
            if self.sim is not None:
                self.sim._h = C.c_void_p()
            _lib.lib().nb_runner_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass
