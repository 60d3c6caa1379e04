"""Radial profiles at the C-ABI boundary, without a device: the entry points are exported, the Python
mirrors have the C layout, bad arguments are refused before any device is touched, the host-only helpers
(edges, Lagrangian radii) give what can be worked out by hand, and the tests' own restatement of the
binning rule (tests/radial_ref.py) reproduces closed forms."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import radial_ref as R
from tests.helpers import ROOT

NAMES = ("nb_sim_radial_profile", "nb_runner_radial_profile", "nb_radial_edges_log", "nb_radial_edges_linear",
         "nb_radial_lagrangian")

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "nbody.h"
#define F(T, x) printf(#T "." #x " %zu %zu\n", offsetof(T, x), sizeof(((T *)0)->x));
#define S(T) printf(#T " %zu %zu\n", sizeof(T), _Alignof(T));
int main(void) {
    S(nb_radial_params) F(nb_radial_params, nbins) F(nb_radial_params, flags) F(nb_radial_params, center)
    F(nb_radial_params, velocity) F(nb_radial_params, axis) F(nb_radial_params, edges)
    S(nb_radial_bin) F(nb_radial_bin, count) F(nb_radial_bin, mass) F(nb_radial_bin, m_r) F(nb_radial_bin, m_ur)
    F(nb_radial_bin, m_ur2) F(nb_radial_bin, m_uphi) F(nb_radial_bin, m_uphi2) F(nb_radial_bin, m_u2)
    F(nb_radial_bin, ang)
    S(nb_radial_profile) F(nb_radial_profile, step_num) F(nb_radial_profile, n) F(nb_radial_profile, nonfinite)
    F(nb_radial_profile, inside_count) F(nb_radial_profile, outside_count) F(nb_radial_profile, inside_mass)
    F(nb_radial_profile, outside_mass) F(nb_radial_profile, mass) F(nb_radial_profile, center)
    F(nb_radial_profile, velocity) F(nb_radial_profile, axis) F(nb_radial_profile, shape)
    F(nb_radial_profile, nbins) F(nb_radial_profile, flags)
    printf("NB_RADIAL_MAX_BINS %u 0\n", NB_RADIAL_MAX_BINS);
    printf("NB_RADIAL_CYLINDRICAL %u 0\n", NB_RADIAL_CYLINDRICAL);
    printf("NB_RADIAL_CENTER_COM %u 0\n", NB_RADIAL_CENTER_COM);
    return 0;
}
"""


def test_radial_entry_points_are_exported(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.ABI_SYMBOLS, name
    for name in ("RadialProfile", "radial_edges"):
        assert name in nb.__all__ and hasattr(nb, name)
    assert hasattr(nb.Simulator, "radial_profile") and hasattr(nb.OfflineHeadless, "radial_profile")
    for prop in ("density", "sigma_r", "mean_uphi", "cumulative_mass", "lagrangian"):
        assert hasattr(nb.RadialProfile, prop)


def test_python_mirrors_match_the_c_layout(nb, tmp_path):
    from wgpu_n_body_amd import _lib
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    cc = os.environ.get("CC", "gcc")
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    rows = [ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True,
                                                check=True).stdout.splitlines()]
    info = {r[0]: (int(r[1]), int(r[2])) for r in rows}
    for S, size in ((_lib.nb_radial_params, 88), (_lib.nb_radial_bin, 88), (_lib.nb_radial_profile, 192)):
        name = S.__name__
        assert info[name] == (C.sizeof(S), C.alignment(S)) and C.sizeof(S) == size, name
        for f, _ in S._fields_:
            assert info[f"{name}.{f}"] == (getattr(S, f).offset, getattr(S, f).size), (name, f)
        assert len(S._fields_) == sum(1 for k in info if k.startswith(name + "."))
    # the numpy record of a bin is the same 88 bytes
    dt = _lib.RADIAL_BIN_DTYPE
    assert dt.itemsize == 88
    for f, _ in _lib.nb_radial_bin._fields_:
        assert dt.fields[f][1] == getattr(_lib.nb_radial_bin, f).offset, f
    assert info["NB_RADIAL_MAX_BINS"][0] == _lib.NB_RADIAL_MAX_BINS == 256
    assert info["NB_RADIAL_CYLINDRICAL"][0] == _lib.NB_RADIAL_CYLINDRICAL
    assert info["NB_RADIAL_CENTER_COM"][0] == _lib.NB_RADIAL_CENTER_COM


def _params(_lib, nbins=4, flags=0, edges=None):
    p = _lib.nb_radial_params()
    p.nbins, p.flags = nbins, flags
    e = np.array(edges if edges is not None else np.linspace(0.0, 1.0, nbins + 1), dtype=np.float64)
    p.edges = e.ctypes.data_as(C.POINTER(C.c_double))
    p.axis[1] = 1.0
    return p, e  # (e keeps the edges alive)


def test_bad_arguments_are_invalid_without_a_device(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    INV = _lib.NB_ERR_INVALID
    CYL, COM = _lib.NB_RADIAL_CYLINDRICAL, _lib.NB_RADIAL_CENTER_COM
    out = _lib.nb_radial_profile()
    bins = (_lib.nb_radial_bin * 256)()
    nan, inf = float("nan"), float("inf")
    for call in (L.nb_sim_radial_profile, L.nb_runner_radial_profile):
        def bad(p, word, o=C.byref(out), b=bins):
            assert call(None, p, o, b) == INV, word
            assert word in L.nb_last_error(), (word, L.nb_last_error())

        p, keep = _params(_lib)
        bad(None, b"params")
        bad(C.byref(p), b"out", o=None)
        bad(C.byref(p), b"bins", b=None)
        p.edges = C.POINTER(C.c_double)()
        bad(C.byref(p), b"edges")
        for nbins in (0, 257, 1 << 31):
            p, keep = _params(_lib, edges=np.linspace(0.0, 1.0, 258))
            p.nbins = nbins
            bad(C.byref(p), b"nbins")
        for flags in (4, 0x80000000, 7):
            p, keep = _params(_lib, flags=flags)
            bad(C.byref(p), b"flag")
        for edges in ([0.0, 1.0, nan, 3.0, 4.0], [0.0, 1.0, 2.0, 3.0, inf], [0.0, 1.0, 2.0, 2.0, 3.0],
                      [0.0, 2.0, 1.0, 3.0, 4.0], [-1.0, 0.0, 1.0, 2.0, 3.0], [-0.5, -0.25, 1.0, 2.0, 3.0],
                      [4.0, 3.0, 2.0, 1.0, 0.0], [nan, 1.0, 2.0, 3.0, 4.0]):
            p, keep = _params(_lib, edges=edges)
            bad(C.byref(p), b"edges")
        for field, k, value in (("center", 0, nan), ("center", 2, inf), ("velocity", 1, -inf), ("velocity", 0, nan)):
            p, keep = _params(_lib)
            getattr(p, field)[k] = value
            bad(C.byref(p), b"center and velocity")
        for flags in (0, CYL, COM, CYL | COM):
            for value in (nan, inf):
                p, keep = _params(_lib, flags=flags)
                p.axis[2] = value
                bad(C.byref(p), b"axis")
        for flags in (CYL, CYL | COM):
            p, keep = _params(_lib, flags=flags)
            p.axis[1] = 0.0
            bad(C.byref(p), b"axis")
        # good parameters, no simulator: every variant gets past the argument checks
        for flags in (0, CYL, COM, CYL | COM):
            p, keep = _params(_lib, flags=flags)
            bad(C.byref(p), b"null")
        # what the flags say is ignored is not looked at
        p, keep = _params(_lib, flags=COM)
        p.center[0], p.velocity[1] = nan, inf
        bad(C.byref(p), b"null")
        p, keep = _params(_lib, flags=0)
        p.axis[1] = 0.0  # a zero axis is fine in spherical mode
        bad(C.byref(p), b"null")
    assert bytes(out) == bytes(C.sizeof(out)) and bytes(bins) == bytes(C.sizeof(bins))  # nothing was written


@pytest.mark.parametrize("nbins", [1, 2, 7, 64, 256])
def test_edge_helpers(nb, nbins):
    for rmin, rmax in ((0.01, 10.0), (1e-3, 3.7), (0.5, 0.75)):
        e = nb.radial_edges(rmin, rmax, nbins, log=True)
        assert e.shape == (nbins + 1,) and e[0] == rmin and e[-1] == rmax
        assert np.all(np.diff(e) > 0)
        ratio = e[1:] / e[:-1]
        assert np.all(np.abs(ratio / (rmax / rmin) ** (1.0 / nbins) - 1.0) <= 1e-12)
    for rmin, rmax in ((0.0, 1.0), (0.25, 10.0), (1.0, 1.0 + 1e-6)):
        e = nb.radial_edges(rmin, rmax, nbins, log=False)
        assert e.shape == (nbins + 1,) and e[0] == rmin and e[-1] == rmax
        assert np.all(np.diff(e) > 0)
        step = (rmax - rmin) / nbins
        assert np.all(np.abs(np.diff(e) - step) <= 1e-12 * rmax)


def test_edge_helpers_refuse_bad_arguments(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    INV = _lib.NB_ERR_INVALID
    buf = (C.c_double * 300)()
    nan, inf = float("nan"), float("inf")
    for fn in (L.nb_radial_edges_log, L.nb_radial_edges_linear):
        assert fn(0.1, 1.0, 4, None) == INV
        for nbins in (0, 257):
            assert fn(0.1, 1.0, nbins, buf) == INV and b"nbins" in L.nb_last_error()
        for rmin, rmax in ((1.0, 1.0), (2.0, 1.0), (nan, 1.0), (0.1, nan), (0.1, inf), (-1.0, 1.0)):
            assert fn(rmin, rmax, 4, buf) == INV, (rmin, rmax)
        # 256 bins do not fit between two neighbouring doubles
        assert fn(1.0, float(np.nextafter(1.0, 2.0)), 256, buf) == INV and b"ascending" in L.nb_last_error()
    assert L.nb_radial_edges_log(0.0, 1.0, 4, buf) == INV  # no ratio from 0 ...
    assert L.nb_radial_edges_linear(0.0, 1.0, 4, buf) == 0  # ... but a step
    assert list(buf[:5]) == [0.0, 0.25, 0.5, 0.75, 1.0] and buf[5] == 0.0
    with pytest.raises(nb.NBodyError):
        nb.radial_edges(1.0, 0.5, 8)
    with pytest.raises(nb.NBodyError):
        nb.radial_edges(0.1, 1.0, 1000)


def _hand_profile(nb, edges, bin_mass, inside_mass=0.0, outside_mass=0.0):
    """A RadialProfile made by hand: only what nb_radial_lagrangian reads is meaningful."""
    nbins = len(bin_mass)
    z, z3 = np.zeros(nbins), np.zeros(3)
    mass = inside_mass + float(np.sum(bin_mass)) + outside_mass
    return nb.RadialProfile(0, 0, 0, 0, 0, inside_mass, outside_mass, mass, z3, z3, z3, np.zeros(6), 0,
                            np.array(edges, dtype=np.float64), np.zeros(nbins, np.uint64),
                            np.array(bin_mass, dtype=np.float64), z, z, z, z, z, z, np.zeros((nbins, 3)))


def test_lagrangian_radii_on_hand_made_profiles(nb):
    # two equal bins: half the mass lies inside the shared edge
    p = _hand_profile(nb, [1.0, 2.0, 4.0], [3.0, 3.0])
    assert p.lagrangian([0.5])[0] == 2.0
    assert p.lagrangian(0.5)[0] == 2.0  # a scalar is one fraction
    # linear inside the bin that crosses: a quarter of the mass is half of bin 0, 0.75 half of bin 1
    assert np.array_equal(p.lagrangian([0.25, 0.75]), [1.5, 3.0])
    # a crossing exactly on an interior edge, four bins of masses 1, 2, 1, 4: f = 3/8 ends bin 1
    q = _hand_profile(nb, [0.0, 1.0, 2.0, 3.0, 5.0], [1.0, 2.0, 1.0, 4.0])
    assert np.array_equal(q.lagrangian([0.125, 0.375, 0.5, 0.75]), [1.0, 2.0, 3.0, 4.0])
    assert np.array_equal(q.cumulative_mass, [1.0, 3.0, 4.0, 8.0])
    # mass below edges[0] and beyond edges[-1]: 2 inside, 4 binned, 2 outside
    w = _hand_profile(nb, [1.0, 2.0, 3.0], [2.0, 2.0], inside_mass=2.0, outside_mass=2.0)
    r = w.lagrangian([0.125, 0.25, 0.375, 0.5, 0.75, 0.875, 0.99])
    assert np.isnan(r[0])                      # crosses in `inside`
    assert np.array_equal(r[1:5], [1.0, 1.5, 2.0, 3.0])  # 0.25: exactly all of `inside`, at edges[0]
    assert np.isnan(r[5]) and np.isnan(r[6])   # crosses in `outside`
    # fractions outside (0, 1) have no radius; an empty bin is skipped
    assert np.all(np.isnan(p.lagrangian([0.0, 1.0, -0.5, 1.5, float("nan")])))
    g = _hand_profile(nb, [0.0, 1.0, 2.0, 3.0], [1.0, 0.0, 1.0])
    assert np.array_equal(g.lagrangian([0.25, 0.75]), [0.5, 2.5])
    # the restatement agrees
    for prof in (p, q, w, g):
        f = np.linspace(0.01, 0.99, 23)
        a, b = prof.lagrangian(f), R.lagrangian64(prof.edges, prof.bin_mass, prof.inside_mass, prof.mass, f)
        assert np.allclose(a, b, rtol=1e-15, atol=0, equal_nan=True)
    # pure function of its arguments, null pointers refused
    from wgpu_n_body_amd import _lib
    assert _lib.lib().nb_radial_lagrangian(None, None, None, None, 0, None) == _lib.NB_ERR_INVALID


def test_derived_quantities(nb):
    p = _hand_profile(nb, [0.0, 1.0, 2.0], [2.0, 14.0])
    assert np.allclose(p.density, [2.0 / (4 * np.pi / 3), 14.0 / (4 * np.pi / 3 * 7)], rtol=1e-15)
    c = nb.RadialProfile(**{**p.__dict__, "flags": 1})
    assert c.cylindrical and not p.cylindrical and p.nbins == 2
    assert np.allclose(c.density, [2.0 / np.pi, 14.0 / (3 * np.pi)], rtol=1e-15)
    # sigma_r^2 = <u_r^2> - <u_r>^2; mean_uphi = m_uphi / mass; an empty bin has neither
    d = nb.RadialProfile(**{**p.__dict__, "bin_mass": np.array([2.0, 0.0]), "m_ur": np.array([2.0, 0.0]),
                            "m_ur2": np.array([10.0, 0.0]), "m_uphi": np.array([3.0, 0.0])})
    assert d.sigma_r[0] == 2.0 and np.isnan(d.sigma_r[1])
    assert d.mean_uphi[0] == 1.5 and np.isnan(d.mean_uphi[1])


# ---------------------------------------------------------------------------------------------
# the restatement against closed forms
# ---------------------------------------------------------------------------------------------
def _bodies(x, v, m):
    s = np.zeros((len(x), 10), np.float32)
    s[:, 0:3], s[:, 3:6], s[:, 9] = x, v, m
    return s


def _sphere_points(rng, n):
    p = rng.normal(size=(n, 3))
    return p / np.linalg.norm(p, axis=1)[:, None]


def test_restatement_bodies_on_known_shells():
    rng = np.random.default_rng(1)
    radii = np.array([0.5, 1.5, 1.5, 2.5, 2.5, 2.5, 7.0, 0.05])  # the last two: outside, inside
    x = _sphere_points(rng, 8) * radii[:, None]
    s = _bodies(x, rng.normal(size=(8, 3)), np.arange(1, 9))
    edges = [0.1, 1.0, 2.0, 3.0]
    ref = R.profile64(s, edges)
    assert list(ref["count"]) == [1, 2, 3]
    assert (ref["inside_count"], ref["outside_count"], ref["nonfinite"]) == (1, 1, 0)
    assert np.array_equal(ref["mass"], [1.0, 5.0, 15.0])
    assert (ref["inside_mass"], ref["outside_mass"], ref["total_mass"]) == (8.0, 7.0, 36.0)
    assert np.allclose(ref["m_r"] / ref["mass"], [0.5, 1.5, 2.5], rtol=1e-6)  # (float32 positions)
    # about another centre the same shells are found again
    c = np.array([0.25, -1.0, 3.0])
    ref2 = R.profile64(_bodies(x + c, s[:, 3:6], s[:, 9]), edges, center=c)
    assert np.array_equal(ref2["count"], ref["count"]) and ref2["inside_count"] == 1 and ref2["outside_count"] == 1
    # a non-finite body is counted and left out
    s[2, 4] = np.inf
    ref3 = R.profile64(s, edges)
    assert ref3["nonfinite"] == 1 and list(ref3["count"]) == [1, 1, 3] and ref3["mass"][1] == 2.0
    assert ref3["inside_count"] + ref3["count"].sum() + ref3["outside_count"] + ref3["nonfinite"] == 8
    # edges are inclusive below and exclusive above; r = 0 is in bin 0 when edges[0] == 0, with u_r = 0
    t = _bodies([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 3]], [[1, 1, 1]] * 4, [1, 1, 1, 1])
    ref4 = R.profile64(t, [0.0, 1.0, 2.0, 3.0])
    assert list(ref4["count"]) == [1, 1, 1] and ref4["outside_count"] == 1 and ref4["inside_count"] == 0
    assert ref4["m_ur"][0] == 0.0 and ref4["m_u2"][0] == 3.0 and ref4["m_ur"][1] == 1.0


@pytest.mark.parametrize("axis", [(0.0, 1.0, 0.0), (1.0, 2.0, 3.0)])
def test_restatement_rigidly_rotating_ring(axis):
    """Bodies on a ring of radius R about `axis`, at heights along it, in rigid rotation Omega about it:
    u = Omega n x d, so u_phi = Omega R, u_r = 0 and the angular momentum of the ring (heights
    symmetric about the centre) is parallel to the axis."""
    nh = R.unit_axis(axis)
    e1 = np.cross(nh, [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(nh, e1)
    n, ring, omega = 64, 1.75, 0.3
    phi = 2 * np.pi * np.arange(n) / n
    height = np.where(np.arange(n) % 2 == 0, 0.5, -0.5)[:, None] * nh
    rho = ring * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2)
    d = np.concatenate([rho + height, -rho + height])  # mirrored through the axis: L across the axis cancels
    c, vc = np.array([0.5, -0.25, 2.0]), np.array([0.01, 0.02, -0.03])
    s = _bodies(d + c, omega * np.cross(nh, d) + vc, np.full(2 * n, 0.5))
    ref = R.profile64(s, [1.0, 1.5, 2.0, 2.5], center=c, velocity=vc, axis=axis)
    assert list(ref["count"]) == [0, 2 * n, 0] and ref["inside_count"] == ref["outside_count"] == 0
    mass = ref["mass"][1]
    assert mass == n
    assert abs(ref["m_r"][1] / mass - ring) < 1e-6
    assert abs(ref["m_uphi"][1] / mass - omega * ring) < 1e-6
    assert abs(ref["m_uphi2"][1] / mass - (omega * ring) ** 2) < 1e-6
    assert abs(ref["m_ur"][1]) / mass < 1e-6 and ref["m_ur2"][1] / mass < 1e-12
    ang = ref["ang"][1]
    assert np.linalg.norm(np.cross(ang, nh)) < 1e-5 * np.linalg.norm(ang)
    assert abs(ang @ nh - mass * omega * ring ** 2) < 1e-5 * mass
    # in spherical bins about the same centre the radius is sqrt(R^2 + h^2) and u_phi is not defined
    sph = R.profile64(s, [1.0, 1.5, 2.0, 2.5], center=c, velocity=vc)
    assert list(sph["count"]) == [0, 2 * n, 0] and np.all(sph["m_uphi"] == 0) and np.all(sph["m_uphi2"] == 0)
    assert abs(sph["m_r"][1] / mass - np.hypot(ring, 0.5)) < 1e-6


@pytest.mark.parametrize("axis", [None, (0.0, 1.0, 0.0), (1.0, 2.0, 3.0)])
def test_restatement_pure_radial_expansion(axis):
    """u = H d: in spherical bins u_r = H r and nothing else; in cylindrical bins u_r = H r with r the
    distance from the axis (u along the axis does not count), u_phi = 0, and no angular momentum."""
    rng = np.random.default_rng(3)
    n, hubble = 500, 0.7
    d = rng.uniform(-1.0, 1.0, size=(n, 3)).astype(np.float32).astype(np.float64)
    m = rng.uniform(0.5, 1.5, size=n)
    s = _bodies(d, hubble * d, m)
    edges = np.linspace(0.0, 2.0, 9)
    ref = R.profile64(s, edges, axis=axis)
    assert ref["inside_count"] == 0 and ref["outside_count"] == 0 and ref["count"].sum() == n
    full = ref["count"] > 0
    assert np.allclose(ref["m_ur"][full], hubble * ref["m_r"][full], rtol=1e-6)
    assert np.all(np.abs(ref["m_uphi"]) <= 1e-6 * ref["mass"]) and np.all(np.abs(ref["ang"]) <= 1e-6 * ref["mass"][:, None])
    x = s[:, 0:3].astype(np.float64)
    mm = s[:, 9].astype(np.float64)
    assert np.allclose(ref["shape"], [(mm * x[:, a] * x[:, b]).sum() for a, b in
                                      ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))], rtol=1e-12)
    assert abs(ref["mass"].sum() - mm.sum()) <= 1e-12 * mm.sum() and abs(ref["total_mass"] - mm.sum()) <= 1e-12 * mm.sum()
