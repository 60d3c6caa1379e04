"""nb_sim_halo_profiles without a device: the numpy restatement of its rule (tests/halo_ref.py) against integer
arithmetic on dyadic coordinates and against the radial restatement, the grid of the rule shown to lose no body,
the host helpers nb_halo_enclosed and nb_halo_overdensity against their restatements, the struct layouts and the
refusals that need no device.  `-m "not gpu"`."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import halo_ref as H
from tests import radial_ref
from tests.helpers import ROOT


def _state(x, v=None, m=None):
    x = np.asarray(x, dtype=np.float32).reshape(-1, 3)
    s = np.zeros((x.shape[0], 10), np.float32)
    s[:, 0:3] = x
    s[:, 3:6] = 0.0 if v is None else v
    s[:, 9] = 1.0 if m is None else m
    return s


def test_layouts_and_constants(nb):
    from wgpu_n_body_amd import _lib
    assert C.sizeof(_lib.nb_halo_params) == 48
    assert C.sizeof(_lib.nb_halo_head) == 64 == _lib.HALO_HEAD_DTYPE.itemsize
    assert C.sizeof(_lib.nb_halo_stats) == 64
    assert _lib.nb_halo_head.center.offset == 16 and _lib.nb_halo_head.velocity.offset == 40
    assert _lib.HALO_HEAD_DTYPE.fields["center"][1] == 16 and _lib.HALO_HEAD_DTYPE.fields["velocity"][1] == 40
    header = open(os.path.join(ROOT, "include", "nbody.h")).read()

    def const(name):
        text = re.search(r"#define %s (\S+( << \d+\))?)" % name, header).group(1)
        return eval(text.replace("u", ""))

    for name, want in (("NB_HALO_MAX_BINS", H.MAX_BINS), ("NB_HALO_MAX_CENTERS", H.MAX_CENTERS),
                       ("NB_HALO_MAX_ROWS", H.MAX_ROWS), ("NB_HALO_MAX_CELLS_PER_AXIS", H.MAX_CELLS),
                       ("NB_HALO_CHUNK", H.CHUNK), ("NB_HALO_EXTRA_ITEMS", H.EXTRA_ITEMS),
                       ("NB_HALO_CENTER_NONFINITE", H.CENTER_NONFINITE)):
        assert const(name) == want == getattr(_lib, name), name
    assert H.SPHERE == _lib.NB_KNN_SPHERE
    for sym in ("nb_sim_halo_profiles", "nb_runner_halo_profiles", "nb_halo_enclosed", "nb_halo_overdensity"):
        assert sym in _lib.ABI_SYMBOLS and hasattr(_lib.lib(), sym)


def test_dyadic_edges_are_inclusive_below_exclusive_above():
    """Coordinates, centres and edges in units of 1/8: every r^2 is an exact integer of 1/64, so integers say which
    bin a body is in -- among them bodies exactly on an edge (3-4-5 and 6-8-10 triangles, axis points)."""
    rng = np.random.default_rng(5)
    pts = rng.integers(-24, 25, size=(600, 3))
    on_edge = np.array([[3, 4, 0], [0, -3, 4], [5, 0, 0], [6, 8, 0], [0, 0, 10], [-10, 0, 0], [0, 0, 0], [1, 0, 0],
                        [0, 15, 0], [9, 12, 0], [0, 0, 2], [0, 2, 0]])
    centres = np.array([[0, 0, 0], [8, -8, 16], [1, 2, 3]])
    edges_i = np.array([2, 5, 10, 15])
    for ci in centres:
        p = np.concatenate([pts, on_edge + ci])
        ref = H.halo_ref(_state(p / 8.0), edges_i / 8.0, centers=[ci / 8.0])
        r2 = ((p - ci) ** 2).sum(1)
        want = [int(((r2 >= a * a) & (r2 < b * b)).sum()) for a, b in zip(edges_i[:-1], edges_i[1:])]
        assert ref["count"][0].tolist() == want
        assert ref["inside_count"][0] == int((r2 < 4).sum())
        # the bodies on an edge are in the bin above it, those on the last edge in none
        assert int((r2 == 25).sum()) >= 3 and int((r2 == 225).sum()) >= 2
        assert ref["mass"][0].tolist() == [float(w) for w in want]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_agrees_with_the_radial_restatement(seed):
    rng = np.random.default_rng(seed)
    s = np.zeros((300, 10), np.float32)
    s[:, 0:6] = rng.normal(size=(300, 6))
    s[:, 9] = rng.uniform(0.5, 2.0, 300)
    s[7, 2] = np.nan
    edges = np.array([0.25, 0.5, 0.9, 1.4, 2.0])
    c, vc = rng.normal(size=(3, 3)) * 0.3, rng.normal(size=(3, 3)) * 0.1
    ref = H.halo_ref(s, edges, centers=c, velocities=vc)
    for j in range(3):
        one = radial_ref.profile64(s, edges, center=c[j], velocity=vc[j])
        assert np.array_equal(ref["count"][j], one["count"]) and ref["inside_count"][j] == one["inside_count"]
        for name in H.SUMS:
            assert np.array_equal(ref[name][j], one[name]), name
    assert ref["nonfinite"] == 1


@pytest.mark.parametrize("seed", range(6))
def test_the_grid_loses_no_body(seed):
    """The restated grid against brute force: every body with r2 < R^2 lies in the cells its centre looks at, for
    centres inside, on the faces of and outside the bounding box, and R from far below the cell limit to above the
    box.  So T >= the bodies inside the sphere, with the bodies of the range counted one by one."""
    rng = np.random.default_rng(100 + seed)
    n = 2000
    x = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    x[:50] = x[50:100]  # coincident bodies
    s = _state(x)
    R = [1e-4, 0.03, 0.11, 0.5, 1.0, 5.0][seed]
    edges = np.array([0.0, R / 2, R])
    lo, hi = x.min(0).astype(np.float64), x.max(0).astype(np.float64)
    c = np.concatenate([rng.uniform(-1.2, 1.2, (40, 3)), x[:20].astype(np.float64), [lo, hi, (lo + hi) / 2],
                        [[lo[0], 0, 0], [hi[0] + R, 0, 0], [hi[0] + R * (1 - 1e-16), 0, 0], [lo[0] - R, hi[1], lo[2]]]])
    g = H.grid64(s, edges)
    assert g["h"] >= R and max(g["cells"]) <= H.MAX_CELLS
    q = H.cells64(g, x.astype(np.float64))
    T = H.candidates64(s, edges, c)
    for j, cj in enumerate(c):
        d = x.astype(np.float64) - cj
        r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        inside = r2 < g["r2max"]
        rng_ = [H.axis_range64(g, a, cj[a]) for a in range(3)]
        if any(r is None for r in rng_):
            assert not inside.any()
            continue
        sel = np.ones(n, bool)
        for a in range(3):
            sel &= (q[:, a] >= rng_[a][0]) & (q[:, a] <= rng_[a][1])
            assert rng_[a][1] - rng_[a][0] <= 4
        assert not (inside & ~sel).any()
        assert T[j] == sel.sum() >= inside.sum()


def _c_helpers(inside_mass, bin_mass, edges, rho):
    from wgpu_n_body_amd import _lib
    nbins = len(bin_mass)
    head = np.zeros(1, _lib.HALO_HEAD_DTYPE)
    head["inside_mass"] = inside_mass
    bins = np.zeros(nbins, _lib.RADIAL_BIN_DTYPE)
    bins["mass"] = bin_mass
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    enc = np.empty(nbins + 1)
    dp = C.POINTER(C.c_double)
    assert _lib.lib().nb_halo_enclosed(head.ctypes.data, bins.ctypes.data, nbins, enc.ctypes.data_as(dp)) == 0
    r, m = C.c_double(), C.c_double()
    assert _lib.lib().nb_halo_overdensity(head.ctypes.data, bins.ctypes.data, edges.ctypes.data_as(dp), nbins,
                                          float(rho), C.byref(r), C.byref(m)) == 0
    return enc, r.value, m.value


def _close(a, b):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-12 * abs(b)


def test_helpers_against_their_restatements(nb):
    rng = np.random.default_rng(3)
    for trial in range(20):
        nbins = int(rng.integers(1, 65))
        edges = np.cumsum(rng.uniform(0.05, 0.3, nbins + 1)) - (0.05 if trial % 4 == 0 else 0.0)
        if trial % 5 == 0:
            edges[0] = 0.0
        bin_mass, inside = rng.uniform(0.0, 2.0, nbins), float(rng.uniform(0.0, 1.0))
        M = H.enclosed64(inside, bin_mass)
        mean = M[1:] / (H.SPHERE * ((edges[1:] * edges[1:]) * edges[1:]))  # as the helper forms it
        for rho in (mean.min() * 0.5, mean.max() * 2.0, np.median(mean), mean[nbins // 2] * 1.0001):
            enc, r, m = _c_helpers(inside, bin_mass, edges, rho)
            assert np.all(np.abs(enc - M) <= 1e-12 * np.abs(M))
            wr, wm = H.overdensity64(inside, bin_mass, edges, rho)
            assert _close(r, wr) and _close(m, wm), (trial, rho, r, wr)
            if not np.isnan(r):
                assert edges[0] <= r <= edges[-1] and _close(m, rho * H.SPHERE * r ** 3)


def test_overdensity_without_a_crossing_is_nan(nb):
    edges = np.array([0.1, 0.2, 0.4, 0.8])
    mass = np.array([1.0, 1.0, 1.0])
    mean = H.enclosed64(0.5, mass) / (H.SPHERE * edges ** 3)
    for rho in (mean.max() * 1.01, mean.min() * 0.99):  # denser than the innermost edge; still denser at the last
        _, r, m = _c_helpers(0.5, mass, edges, rho)
        assert np.isnan(r) and np.isnan(m)
        assert np.isnan(H.overdensity64(0.5, mass, edges, rho)[0])
    _, r, m = _c_helpers(0.0, np.zeros(3), edges, 1.0)  # an empty profile
    assert np.isnan(r) and np.isnan(m)


def test_overdensity_takes_the_first_of_two_crossings(nb):
    """A shell of mass far out lifts the mean density back above rho: it falls through rho between edges 1 and 2
    and again between edges 4 and 5."""
    edges = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6])
    mass = np.array([0.0, 0.0, 0.0, 12.0, 0.0])
    M = H.enclosed64(1.0, mass)
    mean = M / (H.SPHERE * edges ** 3)
    rho = 0.5 * (mean[1] + mean[2])
    assert mean[1] >= rho > mean[2] and mean[4] >= rho > mean[5]
    _, r, m = _c_helpers(1.0, mass, edges, rho)
    wr, wm = H.overdensity64(1.0, mass, edges, rho)
    assert edges[1] <= r < edges[2] and _close(r, wr) and _close(m, wm)
    # with no mass between them the enclosed mass is flat: r is where rho C r^3 = M exactly
    assert abs(r - (1.0 / (rho * H.SPHERE)) ** (1.0 / 3.0)) <= 1e-12 * r


def _refused(nb, why, sim=None, **kw):
    from wgpu_n_body_amd import _lib
    dp = C.POINTER(C.c_double)
    keep = []

    def arr(a, dtype=np.float64):
        a = np.ascontiguousarray(a, dtype=dtype)
        keep.append(a)
        return a

    p = _lib.nb_halo_params()
    edges = arr(kw.get("edges", [0.1, 0.2, 0.3]))
    p.nbins = kw.get("nbins", edges.shape[0] - 1)
    p.flags = kw.get("flags", 0)
    p.edges = edges.ctypes.data_as(dp) if kw.get("edges", 1) is not None else None
    if kw.get("centers") is not None:
        p.centers = arr(kw["centers"]).ctypes.data_as(dp)
    if kw.get("bodies") is not None:
        p.bodies = arr(kw["bodies"], np.uint32).ctypes.data_as(C.POINTER(C.c_uint32))
    if kw.get("velocities") is not None:
        p.velocities = arr(kw["velocities"]).ctypes.data_as(dp)
    p.m = kw.get("m", 1)
    st = _lib.nb_halo_stats()
    rc = _lib.lib().nb_sim_halo_profiles(sim, C.byref(p) if not kw.get("null_params") else None, None, None,
                                         C.byref(st))
    assert rc == _lib.NB_ERR_INVALID
    assert why in _lib.lib().nb_last_error().decode(), _lib.lib().nb_last_error()


def test_refusals_that_need_no_device(nb):
    """Every argument check comes before the handle is looked at: the message names the argument, not the null
    simulator."""
    one = [[0.0, 0.0, 0.0]]
    _refused(nb, "null params", null_params=True)
    _refused(nb, "nbins must be", centers=one, nbins=0)
    _refused(nb, "nbins must be", centers=one, edges=np.linspace(0.1, 1.0, 66), nbins=65)
    _refused(nb, "unknown flag", centers=one, flags=1)
    _refused(nb, "strictly ascending", centers=one, edges=[0.1, 0.1, 0.3])
    _refused(nb, "strictly ascending", centers=one, edges=[-0.1, 0.1, 0.3])
    _refused(nb, "strictly ascending", centers=one, edges=[0.1, np.nan, 0.3])
    _refused(nb, "strictly ascending", centers=one, edges=[0.1, 0.2, np.inf])
    _refused(nb, "got neither")
    _refused(nb, "got both", centers=one, bodies=[0])
    _refused(nb, "non-finite position", centers=[[0.0, np.nan, 0.0]])
    _refused(nb, "non-finite position", centers=[[0.0, 0.0, 0.0], [np.inf, 0.0, 0.0]], m=2)
    _refused(nb, "non-finite velocity", centers=one, velocities=[[0.0, 0.0, np.nan]])
    _refused(nb, "more than one call takes", m=H.MAX_CENTERS + 1, edges=[0.1, 0.2], nbins=1)
    _refused(nb, "more than one call takes", m=H.MAX_ROWS // 64 + 1, edges=np.linspace(0.1, 1.0, 65), nbins=64)
    _refused(nb, "null simulator", centers=one)  # valid arguments: only now the handle
    _refused(nb, "null simulator", m=0)          # no centres: neither array is needed


def test_helper_refusals(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    head, bins = np.zeros(1, _lib.HALO_HEAD_DTYPE), np.zeros(2, _lib.RADIAL_BIN_DTYPE)
    edges, out = np.array([0.1, 0.2, 0.3]), np.empty(3)
    dp = C.POINTER(C.c_double)
    r, m = C.c_double(), C.c_double()
    assert L.nb_halo_enclosed(None, bins.ctypes.data, 2, out.ctypes.data_as(dp)) == _lib.NB_ERR_INVALID
    assert L.nb_halo_enclosed(head.ctypes.data, bins.ctypes.data, 0, out.ctypes.data_as(dp)) == _lib.NB_ERR_INVALID
    assert L.nb_halo_enclosed(head.ctypes.data, bins.ctypes.data, 65, out.ctypes.data_as(dp)) == _lib.NB_ERR_INVALID
    for rho in (0.0, -1.0, np.nan, np.inf):
        assert L.nb_halo_overdensity(head.ctypes.data, bins.ctypes.data, edges.ctypes.data_as(dp), 2, rho,
                                     C.byref(r), C.byref(m)) == _lib.NB_ERR_INVALID
    assert L.nb_halo_overdensity(head.ctypes.data, bins.ctypes.data, None, 2, 1.0, C.byref(r),
                                 C.byref(m)) == _lib.NB_ERR_INVALID
