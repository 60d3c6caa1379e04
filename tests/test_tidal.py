"""Tidal tensor probes without a device: the fp64 restatement (tests/tidal_ref.py) against central differences of
the field's restatement, its trace identity and one-body answers; that the stated bound tells each of five wrong
rules from the right one on the very point sets the device test uses; nb_tidal_ring_means against numpy; the entry
points, the layouts and the refusals that need no simulator."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import field_ref as F
from tests import tidal_ref as T
from tests.helpers import E, G, ROOT

NAMES = ("nb_tidal_sim", "nb_tidal_runner", "nb_tidal_ring_means")

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "nbody.h"
#define F(T, x) printf(#T "." #x " %zu %zu\n", offsetof(T, x), sizeof(((T *)0)->x));
#define S(T) printf(#T " %zu %zu\n", sizeof(T), _Alignof(T));
int main(void) {
    S(nb_tidal_sample) F(nb_tidal_sample, tensor) F(nb_tidal_sample, coincident) F(nb_tidal_sample, reserved)
    S(nb_tidal_stats) S(nb_field_stats)
    S(nb_tidal_ring) F(nb_tidal_ring, t_RR) F(nb_tidal_ring, t_pp) F(nb_tidal_ring, t_nn) F(nb_tidal_ring, t_Rn)
    F(nb_tidal_ring, omega2) F(nb_tidal_ring, kappa2) F(nb_tidal_ring, nu2)
    printf("NB_TIDAL_K %u 0\n", NB_TIDAL_K);
    return 0;
}
"""

DP = C.POINTER(C.c_double)


def _v3(v):
    return (C.c_double * 3)(*v)


# ---- the restatement ---------------------------------------------------------------------------
def _fd_case(regime, seed):
    """300 bodies and 24 points whose coordinates are multiples of 2^-8 in (-1, 1), so that p +- h is an fp32
    number for h = 2^-19 (field64 takes fp32 points).  regime "far": every body at least 0.15 from every point
    (r^3 >= 34 e); "near": each point also has a body 0.3 to 0.9 e^(1/3) away."""
    rng = np.random.default_rng(seed)
    pts = (rng.integers(-200, 201, size=(24, 3)) / 256.0).astype(np.float32)
    s = np.zeros((300, 10), np.float32)
    x = rng.uniform(-1.0, 1.0, size=(4000, 3))
    far = np.sqrt(((x[:, None, :] - pts[None, :, :].astype(np.float64)) ** 2).sum(2)).min(1) >= 0.15
    s[:, 0:3] = x[far][:300]
    s[:, 9] = rng.uniform(0.5, 2.0, size=300)
    if regime == "near":
        u = rng.normal(size=(24, 3))
        u *= (rng.uniform(0.3, 0.9, size=24) * E ** (1.0 / 3.0) / np.sqrt((u * u).sum(1)))[:, None]
        s[:24, 0:3] = pts + u
    return s, pts


@pytest.mark.parametrize("e", [E, 0.0])
@pytest.mark.parametrize("regime", ["far", "near"])
def test_restatement_against_central_differences(regime, e):
    """T_ab = d acc_a / d x_b: central differences of field64's acceleration with h = 2^-19.  Truncation is
    (10 / 3) (h / r)^2 of the term of a body at distance r under a 1 / r^3 law -- 6e-8 at the nearest body of the
    near regime, 0.3 e^(1/3) = 0.014 away -- and the rounding of the difference 1e-16 / h = 5e-11 of |acc| over
    |T|, which is of the size of the distances: below 1e-6 together."""
    s, pts = _fd_case(regime, seed=3)
    ref = T.tidal64(s, pts, G, e)
    d = np.sqrt(((s[None, :, 0:3].astype(np.float64) - pts[:, None, :]) ** 2).sum(2)).min(1)
    assert np.all(d >= 0.15) if regime == "far" else np.all(d <= 0.9 * E ** (1.0 / 3.0) * 1.001)
    h = 2.0 ** -19
    fd = np.zeros((24, 3, 3))
    for b in range(3):
        step = np.zeros(3, np.float32)
        step[b] = h
        hi, lo = pts + step, pts - step
        assert np.array_equal(hi.astype(np.float64), pts.astype(np.float64) + step)  # exact in fp32
        assert np.array_equal(lo.astype(np.float64), pts.astype(np.float64) - step)
        fd[:, :, b] = (F.field64(s, hi, G, e, potential=False)["acc"]
                       - F.field64(s, lo, G, e, potential=False)["acc"]) / (2.0 * h)
    scale = np.abs(ref["tensor"]).max(axis=(1, 2))[:, None, None]
    rel = (np.abs(fd - ref["tensor"]) / scale).max()
    print("central differences: worst relative difference", rel)
    assert rel <= 1e-6
    assert np.array_equal(ref["tensor"], ref["tensor"].transpose(0, 2, 1))  # symmetric by construction


@pytest.mark.parametrize("e", [E, 0.0, 0.02])
def test_trace_identity(e):
    """tr T = g sum m (r^3 - 2 e) / (r (r^3 + e)^2): not zero, and negative inside a core."""
    s, pts = _fd_case("near", seed=4)
    ref = T.tidal64(s, pts, G, e)
    tr = ref["tensor6"][:, :3].sum(1)
    tol = 1e-13 * (ref["scales"][:, :3].sum(1) + 3 * ref["scales"][:, 6])
    assert np.all(np.abs(tr - ref["trace_direct"]) <= tol)
    assert np.all(ref["trace_direct"] != 0)
    # one body: inside r^3 < 2 e the trace is negative (compressive), outside positive
    one = np.zeros((1, 10), np.float32)
    one[0, 9] = 1.0
    r = np.float64(e) ** (1.0 / 3.0) if e else 0.5
    t = T.tidal64(one, [[0.5 * r, 0, 0], [2.0 * r, 0, 0]], G, e)["tensor6"][:, :3].sum(1)
    assert (t[0] < 0 and t[1] > 0) if e else np.all(t > 0)


def _ring_case(L, _lib, e, axis, center, radii, n_phi, mass):
    """One body at the centre: the ring points, the reference field and tensor there, and both ring means."""
    r = np.ascontiguousarray(radii, dtype=np.float64)
    s = np.zeros((1, 10), np.float32)
    s[0, 0:3], s[0, 9] = center, mass
    pts = np.zeros((r.shape[0] * n_phi, 3), np.float32)
    assert L.nb_field_rings(_v3(center), _v3(axis), r.ctypes.data_as(DP), r.shape[0], n_phi, pts.ctypes.data) == 0
    f = F.field64(s, pts, G, e, potential=False)
    fs = np.zeros(pts.shape[0], _lib.FIELD_SAMPLE_DTYPE)
    fs["acc"] = f["acc"]
    rings = np.zeros(r.shape[0], _lib.FIELD_RING_DTYPE)
    assert L.nb_field_ring_means(_v3(center), _v3(axis), r.ctypes.data_as(DP), r.shape[0], n_phi, pts.ctypes.data,
                                 fs.ctypes.data, rings.ctypes.data) == 0
    ts = np.zeros(pts.shape[0], _lib.TIDAL_SAMPLE_DTYPE)
    ts["tensor"] = T.tidal64(s, pts, G, e)["tensor6"]
    out = np.zeros(r.shape[0], _lib.TIDAL_RING_DTYPE)
    assert L.nb_tidal_ring_means(_v3(center), _v3(axis), r.ctypes.data_as(DP), r.shape[0], n_phi, pts.ctypes.data,
                                 ts.ctypes.data, rings.ctypes.data, out.ctypes.data) == 0
    return pts, ts, rings, out


@pytest.mark.parametrize("axis", [(0.0, 1.0, 0.0), (1.0, 2.0, 3.0)])
@pytest.mark.parametrize("e", [E, 0.0, 0.05])
def test_one_body_known_answers(nb, e, axis):
    """One body of mass M at the centre: Omega^2 = nu^2 = g M / (R (R^3 + e)), kappa^2 = 3 e g M / (R (R^3 + e)^2),
    which is 0 for e = 0 (a 1 / r^3 force is marginally stable).  The points are fp32: an ulp of R moves R^-4 by
    four, and kappa^2 is the difference of two terms of the size of 4 Omega^2."""
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    M, radii = 150000.0, np.linspace(0.125, 2.0, 16)
    _, _, rings, out = _ring_case(L, _lib, e, axis, (0.25, -0.5, 0.125), radii, 8, M)
    g, e64 = np.float64(np.float32(G)), np.float64(np.float32(e))
    om2 = g * M / (radii * (radii ** 3 + e64))
    ka2 = 3.0 * e64 * g * M / (radii * (radii ** 3 + e64) ** 2)
    tol = 32 * 2.0 ** -24
    assert np.all(np.abs(out["omega2"] - om2) <= tol * om2) and np.all(np.abs(out["nu2"] - om2) <= tol * om2)
    assert np.all(np.abs(out["kappa2"] - ka2) <= tol * 4 * om2)
    assert np.all(np.abs(out["t_pp"] + om2) <= tol * om2)       # T_phiphi = a_R / R for any central force
    assert np.all(np.abs(out["t_Rn"]) <= tol * om2)
    assert np.array_equal(out["omega2"], -rings["a_R"] / radii)
    assert np.array_equal(out["kappa2"], -out["t_RR"] + 3.0 * out["omega2"]) and np.array_equal(out["nu2"], -out["t_nn"])
    if e == 0.0:
        assert np.all(np.abs(out["kappa2"]) <= tol * 4 * om2)
    else:
        assert np.all(out["kappa2"] > 0)


# ---- the bound has power -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def shape_refs():
    """The right rule on every point set of the device test, once."""
    cases = [T.shape_case(i, E) for i in range(len(T.SHAPES))]
    return [(s, p, T.tidal64(s, p, G, E)) for s, p, _ in cases]


@pytest.mark.parametrize("mutation", T.MUTATIONS)
def test_a_wrong_rule_exceeds_the_bound(nb, shape_refs, mutation):
    """4 r^3 -> 3 r^3, e dropped from the numerator of c, the delta_ab W term dropped, xz and yz swapped, the sign
    of xy flipped: each is further from the right rule than the bound allows the device to be, in at least one
    component, on each of the very point sets tests/test_tidal_gpu.py uses -- so no such kernel passes there.  (The second
    needs the points within e^(1/3) of a body.)"""
    worst = 0.0
    for (m, n), (s, p, ref) in zip(T.SHAPES, shape_refs):
        wrong = T.tidal64(s, p, G, E, mutation=mutation)["tensor6"]
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.abs(wrong - ref["tensor6"]) / ref["bound6"]
        ratio = np.nanmax(np.where(ref["bound6"] > 0, ratio, 0.0), initial=0.0)
        print(f"{mutation}: M {m} N {n}: worst difference / bound {ratio:.1f}")
        worst = max(worst, ratio)
        assert n == 0 or ratio > 2.0, (m, n, ratio)  # (twice: the device's own error may take one bound of it)
    assert worst > 2.0, worst


def test_the_point_sets_reach_inside_the_core(shape_refs):
    for (m, n), (s, p, ref) in zip(T.SHAPES, shape_refs):
        if n == 0 or m < 4:
            continue
        d = np.sqrt(((s[None, :, 0:3].astype(np.float64) - p[:, None, :]) ** 2).sum(2))
        d[d == 0] = np.inf
        assert (d.min(1) < E ** (1.0 / 3.0)).sum() >= (m - (m + 1) // 2 + 1) // 2, (m, n)
        assert np.all(ref["coincident"][: (m + 1) // 2] >= 1)


# ---- nb_tidal_ring_means -----------------------------------------------------------------------
def test_ring_means_against_numpy(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(11)
    center, axis = np.array([0.5, 0.25, -1.0]), (1.0, 2.0, 3.0)
    radii = np.array([0.0, 0.5, 1.0, 3.0])  # ring 0 sits on the axis
    n_phi = 6
    pts = nb.field_rings(radii, axis=axis, center=center, n_phi=n_phi)
    ts = np.zeros(pts.shape[0], _lib.TIDAL_SAMPLE_DTYPE)
    ts["tensor"] = rng.normal(size=(pts.shape[0], 6))
    rings = np.zeros(4, _lib.FIELD_RING_DTYPE)
    rings["a_R"] = [-0.0, -2.0, -3.0, 0.5]
    out = np.zeros(4, _lib.TIDAL_RING_DTYPE)
    args = [_v3(center), _v3(axis), radii.ctypes.data_as(DP), 4, n_phi, pts.ctypes.data, ts.ctypes.data,
            rings.ctypes.data, out.ctypes.data]
    assert L.nb_tidal_ring_means(*args) == 0
    n, _, _ = nb.map_frame(axis)
    t = ts["tensor"][:, [0, 3, 4, 3, 1, 5, 4, 5, 2]].reshape(-1, 3, 3)
    d = pts.astype(np.float64) - center
    rho = d - (d @ n)[:, None] * n
    R = np.sqrt((rho * rho).sum(1))
    on_axis = R == 0
    assert on_axis[:n_phi].all() and not on_axis[n_phi:].any()
    rhat = np.where(on_axis[:, None], 0.0, rho / np.where(on_axis, 1.0, R)[:, None])
    phat = np.cross(n, rhat)
    ein = lambda a, b: np.einsum("ia,iab,ib->i", a, t, b).reshape(4, n_phi).mean(1)  # noqa: E731
    nn = np.tile(n, (pts.shape[0], 1))
    assert np.allclose(out["t_RR"], ein(rhat, rhat), rtol=1e-13, atol=1e-15)
    assert np.allclose(out["t_pp"], ein(phat, phat), rtol=1e-13, atol=1e-15)
    assert np.allclose(out["t_nn"], ein(nn, nn), rtol=1e-13, atol=1e-15)
    assert np.allclose(out["t_Rn"], ein(rhat, nn), rtol=1e-13, atol=1e-15)
    assert out["t_RR"][0] == 0 and out["t_pp"][0] == 0 and out["t_Rn"][0] == 0 and out["t_nn"][0] != 0
    assert np.isnan(out["omega2"][0]) and np.isnan(out["kappa2"][0])
    assert np.array_equal(out["omega2"][1:], -rings["a_R"][1:] / radii[1:]) and out["omega2"][3] < 0
    assert np.array_equal(out["kappa2"][1:], -out["t_RR"][1:] + 3.0 * out["omega2"][1:])
    assert np.array_equal(out["nu2"], -out["t_nn"])
    # refusals: as nb_field_rings, and null samples, rings or out
    INV = _lib.NB_ERR_INVALID
    for k, v in ((0, None), (1, None), (2, None), (5, None), (6, None), (7, None), (8, None), (4, 0),
                 (1, _v3((0, 0, 0))), (0, _v3((float("nan"), 0, 0)))):
        bad = list(args)
        bad[k] = v
        before = out.copy()
        assert L.nb_tidal_ring_means(*bad) == INV and L.nb_last_error(), k
        assert before.tobytes() == out.tobytes()


def test_disc_frequency_roots_and_resonances(nb):
    """The Python object's arithmetic, without a device: roots are NaN where the square is negative, and the
    resonances are the linear crossings between rings."""
    r = np.array([1.0, 2.0, 3.0, 4.0])
    om2, ka2 = np.array([16.0, 4.0, 1.0, -1.0]), np.array([16.0, 4.0, -1.0, 1.0])
    z = np.zeros(4)
    d = nb.DiscFrequencies(r, om2, ka2, om2, z, z, z, z, z, None, None)
    assert np.array_equal(d.omega[:3], [4.0, 2.0, 1.0]) and np.isnan(d.omega[3]) and np.isnan(d.kappa[2])
    res = d.resonances(3.0, m=2)
    assert np.array_equal(res["corotation"], [1.5])               # Omega: 4 -> 2 between R = 1 and 2
    assert np.array_equal(res["inner_lindblad"], [])              # Omega - kappa / 2: 2, 1, nan, nan
    assert np.allclose(res["outer_lindblad"], [1.0 + 3.0 / 3.0])  # Omega + kappa / 2: 6, 3: the crossing is R = 2
    assert np.array_equal(d.resonances(2.0, m=2)["corotation"], [2.0])


# ---- the C surface -----------------------------------------------------------------------------
def test_tidal_entry_points_are_exported(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.ABI_SYMBOLS, name
    for name in ("TidalField", "DiscFrequencies"):
        assert name in nb.__all__ and hasattr(nb, name)
    # one method, shared by the two owners of a state
    for cls in (nb.Simulator, nb.OfflineHeadless):
        assert cls.tidal_tensor is nb._Passes.tidal_tensor and cls.disc_frequencies is nb._Passes.disc_frequencies
    assert list(L.nb_tidal_sim.argtypes) == list(L.nb_tidal_runner.argtypes)
    # the C++ mirror names the same pass for both handle types, and the same two methods
    hpp = open(os.path.join(ROOT, "wgpu_n_body_amd", "csrc", "simulator.hpp")).read()
    assert "static constexpr auto tidal = nb_tidal_sim;" in hpp and "static constexpr auto tidal = nb_tidal_runner;" in hpp
    assert "TidalField tidal_tensor(" in hpp and "DiscFrequencies disc_frequencies(" in hpp


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
    assert info["nb_tidal_sample"][0] == 56 and info["nb_tidal_stats"] == info["nb_field_stats"]
    assert _lib.nb_tidal_stats is _lib.nb_field_stats
    for S, dt, size in ((_lib.nb_tidal_sample, _lib.TIDAL_SAMPLE_DTYPE, 56), (_lib.nb_tidal_ring, _lib.TIDAL_RING_DTYPE, 56)):
        name = S.__name__
        assert info[name] == (C.sizeof(S), C.alignment(S)) and C.sizeof(S) == size == dt.itemsize, name
        for f, _ in S._fields_:
            assert info[f"{name}.{f}"] == (getattr(S, f).offset, getattr(S, f).size), (name, f)
            assert dt.fields[f][1] == getattr(S, f).offset, f
        assert len(S._fields_) == sum(1 for k in info if k.startswith(name + "."))
    assert info["NB_TIDAL_K"][0] == _lib.NB_TIDAL_K == T.K


def test_bad_arguments_are_invalid_without_a_device(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    INV = _lib.NB_ERR_INVALID
    pts = np.zeros((4, 3), np.float32)
    out = np.zeros(4, _lib.TIDAL_SAMPLE_DTYPE)
    st = _lib.nb_tidal_stats()
    for call, who in ((L.nb_tidal_sim, b"simulator"), (L.nb_tidal_runner, b"runner")):
        def bad(word, p=pts.ctypes.data, m=4, o=out.ctypes.data):
            assert call(None, p, m, o, C.byref(st)) == INV, word
            assert word in L.nb_last_error(), (word, L.nb_last_error())

        bad(b"null " + who)                      # a null handle, everything else in order
        bad(b"points", p=None)
        bad(b"out", o=None)
        bad(b"at most", m=_lib.NB_FIELD_MAX_POINTS + 1)
        # m = 0 needs neither array: only the handle is then at fault; stats may be null
        assert call(None, None, 0, None, None) == INV and b"null " + who in L.nb_last_error()
