"""Orbit stability without a device: the entry points and layouts, the refusals that need no simulator,
nb_orbit_stability_derive against numpy, and the rule's restatement (tests/stability_ref.py) in binary64: the deviation
is the derivative of the orbit (a centred difference of two runs), the tangent map keeps the symplectic form and two
wrong rules do not, the renormalisation and the continuation are exact, no bodies give straight lines, and about one
body the vertical deviation of a circular orbit follows the leapfrog's own closed form."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import orbit_ref as R
from tests import stability_ref as S
from tests.helpers import ROOT

NAMES = ("nb_orbit_stability_sim", "nb_orbit_stability_runner", "nb_orbit_stability_derive")
G, E = R.CASE_G, R.CASE_E
AXIS = (0.0, 0.0, 1.0)

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "nbody.h"
#define F(T, x) printf(#T "." #x " %zu %zu\n", offsetof(T, x), sizeof(((T *)0)->x));
#define S(T) printf(#T " %zu %zu\n", sizeof(T), _Alignof(T));
int main(void) {
    S(nb_orbit_stability_params) F(nb_orbit_stability_params, deviations) F(nb_orbit_stability_params, renorm_log2)
    F(nb_orbit_stability_params, reserved)
    S(nb_orbit_deviation) F(nb_orbit_deviation, d) F(nb_orbit_deviation, log2)
    S(nb_orbit_growth) F(nb_orbit_growth, peak_log2) F(nb_orbit_growth, peak_step) F(nb_orbit_growth, renorms)
    F(nb_orbit_growth, reserved)
    S(nb_orbit_stability_stats) F(nb_orbit_stability_stats, orbit) F(nb_orbit_stability_stats, renorms)
    F(nb_orbit_stability_stats, deviations) F(nb_orbit_stability_stats, renorm_log2)
    printf("NB_ORBIT_MAX_DEVIATIONS %u 0\n", NB_ORBIT_MAX_DEVIATIONS);
    printf("NB_ORBIT_MAX_RENORM_LOG2 %u 0\n", NB_ORBIT_MAX_RENORM_LOG2);
    return 0;
}
"""


def _tracers(m=6, seed=3):
    """Tracers on mildly eccentric, slightly inclined orbits between r = 1.2 and 2.5: clear of the two bodies at
    (+-0.5, 0, 0)."""
    rng = np.random.default_rng(seed)
    ang, rad = rng.uniform(0, 2 * np.pi, m), rng.uniform(1.2, 2.5, m)
    pos = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-0.2, 0.2, m)], axis=1)
    vc = 1 / np.sqrt(rad)
    vel = np.stack([-np.sin(ang) * vc, np.cos(ang) * vc, rng.uniform(-0.1, 0.1, m)], axis=1)
    return pos, vel * rng.uniform(0.8, 1.1, (m, 1))


def _vectors(m, d=2):
    q, _ = np.linalg.qr(np.random.default_rng(0).standard_normal((6, 6)))
    return np.broadcast_to(q.T[:d], (m, d, 6)).copy()


# ---- the C surface -----------------------------------------------------------------------------
def test_entry_points_are_exported(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.ABI_SYMBOLS, name
    for name in ("OrbitStability", "OrbitStabilityStats"):
        assert name in nb.__all__ and hasattr(nb, name)
    assert nb.Simulator.orbit_stability is nb.OfflineHeadless.orbit_stability is nb._Passes.orbit_stability
    a, b = L.nb_orbit_stability_sim.argtypes, L.nb_orbit_stability_runner.argtypes
    assert a is not None and list(a) == list(b) and len(a) == 12
    hpp = open(os.path.join(ROOT, "wgpu_n_body_amd", "csrc", "simulator.hpp")).read()
    assert "static constexpr auto orbit_stability = nb_orbit_stability_sim;" in hpp
    assert "static constexpr auto orbit_stability = nb_orbit_stability_runner;" in hpp
    assert "OrbitStability orbit_stability(" in hpp
    assert np.array_equal(nb._default_deviations(2), _vectors(1)[0])


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
    for T, size in ((_lib.nb_orbit_stability_params, 12), (_lib.nb_orbit_deviation, 56), (_lib.nb_orbit_growth, 24),
                    (_lib.nb_orbit_stability_stats, 72)):
        name = T.__name__
        assert info[name] == (C.sizeof(T), C.alignment(T)) and C.sizeof(T) == size, name
        for f, _ in T._fields_:
            assert info[f"{name}.{f}"] == (getattr(T, f).offset, getattr(T, f).size), (name, f)
        assert len(T._fields_) == sum(1 for k in info if k.startswith(name + "."))
    for dt, T in ((_lib.ORBIT_DEVIATION_DTYPE, _lib.nb_orbit_deviation), (_lib.ORBIT_GROWTH_DTYPE, _lib.nb_orbit_growth)):
        assert dt.itemsize == C.sizeof(T)
        assert all(dt.fields[f][1] == getattr(T, f).offset for f in dt.names) and len(dt.names) == len(T._fields_)
    assert info["NB_ORBIT_MAX_DEVIATIONS"][0] == _lib.NB_ORBIT_MAX_DEVIATIONS == 6
    assert info["NB_ORBIT_MAX_RENORM_LOG2"][0] == _lib.NB_ORBIT_MAX_RENORM_LOG2 == 512


# ---- the refusals ------------------------------------------------------------------------------
def _params(_lib, **kw):
    p = _lib.nb_orbit_params()
    p.dt, p.step0, p.steps, p.every, p.flags, p.reserved = 0.02, 0, 5, 5, 0, 0
    p.accel_scale, p.omega = 1.0, 0.0
    p.axis[:], p.center[:] = (0.0, 1.0, 0.0), (0.0, 0.0, 0.0)
    s = _lib.nb_orbit_stability_params(2, 32, 0)
    for k, v in kw.items():
        if k in ("axis", "center"):
            getattr(p, k)[:] = v
        elif k.startswith("s_"):
            setattr(s, k[2:], v)
        else:
            setattr(p, k, v)
    return p, s


def test_bad_arguments_are_invalid_without_a_device(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    INV = _lib.NB_ERR_INVALID
    nan, inf = float("nan"), float("inf")
    pos, vel = np.zeros((4, 3)), np.zeros((4, 3))
    dev0 = np.zeros((4, 6), _lib.ORBIT_DEVIATION_DTYPE)
    tracks = np.zeros((2, 4), _lib.ORBIT_SAMPLE_DTYPE)
    devs = np.zeros((2, 4, 6), _lib.ORBIT_DEVIATION_DTYPE)
    growth = np.zeros((4, 6), _lib.ORBIT_GROWTH_DTYPE)
    co = np.zeros(4, np.uint32)
    st = _lib.nb_orbit_stability_stats()
    for call, who in ((L.nb_orbit_stability_sim, b"simulator"), (L.nb_orbit_stability_runner, b"runner")):
        def bad(word, params="ok", stability="ok", x=pos.ctypes.data, v=vel.ctypes.data, m=4, d0=dev0.ctypes.data,
                t=tracks.ctypes.data, dv=devs.ctypes.data, **kw):
            p, s = _params(_lib, **kw)
            before = tracks.tobytes() + devs.tobytes() + growth.tobytes()
            rc = call(None, None if params is None else C.byref(p), None if stability is None else C.byref(s), x, v,
                      m, d0, t, co.ctypes.data, dv, growth.ctypes.data, C.byref(st))
            assert rc == INV, (word, kw)
            assert word in L.nb_last_error(), (word, L.nb_last_error())
            assert tracks.tobytes() + devs.tobytes() + growth.tobytes() == before

        bad(b"null " + who)                       # a null handle, everything else in order
        # what nb_orbits_sim refuses
        bad(b"params", params=None)
        bad(b"pos", x=None)
        bad(b"vel", v=None)
        bad(b"tracks", t=None)
        bad(b"steps", steps=0)
        bad(b"every", every=0)
        bad(b"flag", flags=2)
        bad(b"reserved", reserved=1)
        bad(b"tracers", m=_lib.NB_ORBIT_MAX_TRACERS + 1)
        for v in (nan, inf, 0.0):
            bad(b"dt", dt=v)
        bad(b"omega", omega=nan)
        bad(b"axis", omega=0.7, axis=(0.0, 0.0, 0.0))
        # its own: the energy flag, the params, D, renorm_log2, reserved, the vectors, the samples
        bad(b"NB_ORBIT_ENERGY", flags=_lib.NB_ORBIT_ENERGY)
        bad(b"stability params", stability=None)
        for d in (0, 7, 1 << 31):
            bad(b"deviations", s_deviations=d)
        for r in (0, 513, 1 << 31):
            bad(b"renorm_log2", s_renorm_log2=r)
        bad(b"reserved", s_reserved=1)
        bad(b"dev0", d0=None)
        bad(b"devs", dv=None)
        bad(b"samples", m=1 << 19, steps=8, every=2, s_deviations=2)   # 5 records x 2^19 x 2 > 2^22
        # in order, so that only the handle is at fault: every D and the ends of renorm_log2, the optional outputs
        # null, m = 0 without arrays, records * m * D = 2^22 exactly
        for d in range(1, 7):
            bad(b"null " + who, s_deviations=d)
        for r in (1, 512):
            bad(b"null " + who, s_renorm_log2=r)
        bad(b"null " + who, m=1 << 19, steps=8, every=8, s_deviations=4)
        p, s = _params(_lib)
        assert call(None, C.byref(p), C.byref(s), pos.ctypes.data, vel.ctypes.data, 4, dev0.ctypes.data,
                    tracks.ctypes.data, None, devs.ctypes.data, None, None) == INV and b"null " + who in L.nb_last_error()
        assert call(None, C.byref(p), C.byref(s), None, None, 0, None, None, None, None, None, None) == INV \
            and b"null " + who in L.nb_last_error()


# ---- nb_orbit_stability_derive -----------------------------------------------------------------
def test_derive_against_numpy(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(11)
    m, D, steps, every, dt = 5, 3, 7, 3, 0.25   # records at 0, 3, 6, 7
    ks = R.records(steps, every)
    dev0 = np.zeros((m, D), _lib.ORBIT_DEVIATION_DTYPE)
    devs = np.zeros((len(ks), m, D), _lib.ORBIT_DEVIATION_DTYPE)
    dev0["d"], dev0["log2"] = rng.normal(size=(m, D, 6)), rng.integers(-50, 50, (m, D))
    devs["d"] = rng.normal(size=(len(ks), m, D, 6)) * np.exp2(rng.integers(-300, 300, (len(ks), m, D, 1)))
    devs["log2"] = rng.integers(-5000, 5000, (len(ks), m, D))
    devs["d"][1, 2, 1] = 0.0          # a zero vector
    devs["d"][2, 3, 0, 4] = np.nan    # a non-finite one
    devs["d"][3, 0] *= 2.0 ** 700     # squares that overflow unscaled
    devs["d"][3, 1, 1] = -devs["d"][3, 1, 0] * 4.0 + 1e-9 * np.abs(devs["d"][3, 1, 0]).max() * rng.normal(size=6)  # nearly aligned, opposite
    out = [np.full((len(ks), m, D), 7.0), np.full((len(ks), m, D), 7.0), np.full((len(ks), m), 7.0),
           np.full((len(ks), m), 7.0)]
    assert L.nb_orbit_stability_derive(dt, steps, every, m, D, dev0.ctypes.data, devs.ctypes.data,
                                       *(o.ctypes.data for o in out)) == 0
    with np.errstate(all="ignore"):
        ref = S.derive({"dev": devs["d"], "log2": devs["log2"]}, dev0["d"], dev0["log2"], dt, ks)
    for got, want, name in zip(out, ref, ("log_growth", "lyapunov", "sali", "gali2")):
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        ok = ~np.isnan(want)
        # sums of six (fifteen) products, a square root, a logarithm: a few roundings of the result's own size, and
        # for the two indices of nearly aligned vectors of the unit vectors' components
        tol = 64 * 2.0 ** -53 * (np.abs(want[ok]) + 1.0)
        assert np.all(np.abs(got[ok] - want[ok]) <= tol), (name, np.abs(got[ok] - want[ok]).max())
    assert np.isnan(out[0][1, 2, 1]) and np.isnan(out[0][2, 3, 0]) and np.isnan(out[2][2, 3]) and np.isnan(out[3][2, 3])
    assert np.isnan(out[1][0]).all() and np.isfinite(out[1][3, 0]).all()
    assert out[2][3, 1] < 1e-8 and out[3][3, 1] < 1e-8                      # the aligned pair
    # the optional outputs, D = 1, and the refusals
    assert L.nb_orbit_stability_derive(dt, steps, every, m, D, dev0.ctypes.data, devs.ctypes.data, None, None, None,
                                       None) == 0
    one = np.ascontiguousarray(devs[:, :, :1])
    sali = np.zeros((len(ks), m))
    assert L.nb_orbit_stability_derive(dt, steps, every, m, 1, np.ascontiguousarray(dev0[:, :1]).ctypes.data,
                                       one.ctypes.data, None, None, sali.ctypes.data, None) == 0
    assert np.isnan(sali).all()
    INV = _lib.NB_ERR_INVALID
    for args in ((dt, steps, every, m, 0), (dt, steps, every, m, 7), (dt, 0, every, m, D), (dt, steps, 0, m, D),
                 (0.0, steps, every, m, D), (float("nan"), steps, every, m, D)):
        assert L.nb_orbit_stability_derive(*args, dev0.ctypes.data, devs.ctypes.data, None, None, None, None) == INV
    assert L.nb_orbit_stability_derive(dt, steps, every, m, D, None, devs.ctypes.data, None, None, None, None) == INV
    assert L.nb_orbit_stability_derive(dt, steps, every, 0, D, None, None, None, None, None, None) == 0


# ---- the restatement: the deviation is the derivative of the orbit ------------------------------
# the worst relative error measured below, over six tracers, two vectors, omega 0 and 0.35, eps = 1e-7: 1.3e-8
# (truncation eps^2 of the centred difference and rounding 2^-53 / eps of the orbits, both ~1e-8 to 1e-9); times 10
FD_TOL = 1.3e-7


@pytest.mark.parametrize("omega", [0.0, 0.35])
def test_the_deviation_is_the_centred_difference_of_two_orbits(omega):
    """An exact binary64 field at points that are not rounded to fp32: the field whose tangent map two neighbouring
    orbits can measure."""
    pos, vel = _tracers()
    dev0 = _vectors(pos.shape[0])
    sample, tensor = S.exact64(R.binary_state(), G, E)
    kw = dict(dt=0.01, steps=100, omega=omega, axis=AXIS, renorm_log2=None, round_points=False)
    o = S.stability(sample, tensor, pos, vel, dev0, **kw)
    eps, worst = 1e-7, 0.0
    for j in range(2):
        a, b = (S.stability(sample, tensor, pos + s * eps * dev0[:, j, :3], vel + s * eps * dev0[:, j, 3:], dev0, **kw)
                for s in (1.0, -1.0))
        fd = np.concatenate([a["pos"][-1] - b["pos"][-1], a["vel"][-1] - b["vel"][-1]], axis=1) / (2 * eps)
        d = o["dev"][-1, :, j]
        worst = max(worst, (np.linalg.norm(fd - d, axis=1) / np.linalg.norm(d, axis=1)).max())
    print("centred difference: worst relative error", worst)
    assert worst <= FD_TOL
    assert np.abs(o["dev"][-1] - dev0).max() > 0.1  # (the vectors have moved)


# ---- the symplectic form -----------------------------------------------------------------------
@pytest.mark.parametrize("omega", [0.0, 0.35])
def test_the_tangent_map_keeps_the_symplectic_form_and_wrong_rules_do_not(omega):
    """|omega_k - omega_0| <= C K 2^-53 max_k(|d1| |d2|) with C = 1 over K = 200 steps of dt = 0.02.  Measured: the
    rule C <= 0.03; without the turn of dx in the rotating frame C >= 1e11 (the rule itself at omega = 0); with an
    antisymmetric T_xy C >= 1e11."""
    pos, vel = _tracers()
    dev0 = _vectors(pos.shape[0])
    sample, tensor = S.model64(R.binary_state(), G, E)
    kw = dict(dt=0.02, steps=200, every=1, omega=omega, axis=AXIS, renorm_log2=None)
    C_ = {mut: S.symplectic_C(S.vectors(S.stability(sample, tensor, pos, vel, dev0, mutation=mut, **kw)), 200)
          for mut in (None, "no_turn", "antisymmetric_xy")}
    print("symplectic C:", {k: (v.min(), v.max()) for k, v in C_.items()})
    assert C_[None].max() <= 0.1           # (the inputs the device is asked C <= 1 on stay below 0.1 here)
    assert C_[None].max() <= 1.0
    assert C_["antisymmetric_xy"].min() > 1.0
    if omega != 0.0:
        assert C_["no_turn"].min() > 1.0
    else:
        assert np.array_equal(C_["no_turn"], C_[None])


# ---- the renormalisation and the continuation --------------------------------------------------
@pytest.mark.parametrize("omega", [0.0, 0.35])
def test_renormalisation_and_continuation_are_exact(omega):
    pos, vel = _tracers()
    m = pos.shape[0]
    dev0 = _vectors(m, 3)
    dev0[:, 1] *= 2.0 ** 40
    dev0[:, 2] *= 2.0 ** -40
    sample, tensor = S.model64(R.binary_state(), G, E)
    kw = dict(dt=0.05, every=4, omega=omega, axis=AXIS, center=(0.05, 0.0, 0.0))
    plain = S.stability(sample, tensor, pos, vel, dev0, steps=40, renorm_log2=None, **kw)
    re = S.stability(sample, tensor, pos, vel, dev0, steps=40, renorm_log2=8, **kw)
    assert np.all(plain["log2"] == 0) and np.all(plain["renorms"] == 0)
    assert np.all(re["renorms"][:, 1:] >= 1) and np.all(re["log2"][-1, :, 1] >= 33) and np.all(re["log2"][-1, :, 2] <= -33)
    assert np.array_equal(S.vectors(re), plain["dev"])                  # x 2^log2, in every bit
    assert np.all(np.abs(re["dev"][1:]).max(axis=-1) < 2.0 ** 8) and np.all(np.abs(re["dev"][1:]).max(axis=-1) >= 2.0 ** -8)
    assert np.array_equal(re["peak_log2"], plain["peak_log2"]) and np.array_equal(re["peak_step"], plain["peak_step"])
    assert np.array_equal(re["pos"], plain["pos"]) and np.array_equal(re["vel"], plain["vel"])
    # the mistake the header warns of: kappa left unscaled
    wrong = S.stability(sample, tensor, pos, vel, dev0, steps=40, renorm_log2=8, mutation="kappa_unscaled", **kw)
    assert not np.array_equal(S.vectors(wrong), plain["dev"])
    # every step renormalises with renorm_log2 = 1 whenever E != 0, and the run is still the same
    often = S.stability(sample, tensor, pos, vel, dev0, steps=40, renorm_log2=1, **kw)
    assert np.array_equal(S.vectors(often), plain["dev"]) and often["renorms"].sum() > re["renorms"].sum()
    # a run of 40 = 24 + 16 steps through the last record
    first = S.stability(sample, tensor, pos, vel, dev0, steps=24, renorm_log2=8, step0=7, **kw)
    rest = S.stability(sample, tensor, first["pos"][-1], first["vel"][-1], first["dev"][-1], steps=16, renorm_log2=8,
                       step0=7 + 24, log2_0=first["log2"][-1], **kw)
    whole = S.stability(sample, tensor, pos, vel, dev0, steps=40, renorm_log2=8, step0=7, **kw)
    for name in ("pos", "vel", "dev", "log2"):
        assert np.array_equal(np.concatenate([first[name], rest[name][1:]]), whole[name]), name
    assert np.array_equal(np.maximum(first["peak_log2"], rest["peak_log2"]), whole["peak_log2"])
    assert np.array_equal(first["renorms"] + rest["renorms"], whole["renorms"])


# ---- no bodies ---------------------------------------------------------------------------------
def test_no_bodies_give_straight_lines():
    pos, vel = _tracers()
    m = pos.shape[0]
    dev0 = _vectors(m)

    def sample(p, potential):
        return np.zeros((m, 3)), np.full(m, np.nan), np.zeros(m, np.int64)

    def tensor(p):
        return np.zeros((m, 6))
    o = S.stability(sample, tensor, pos, vel, dev0, dt=0.03, steps=50, every=1, omega=0.35, axis=AXIS)
    dx = dev0[:, :, :3].copy()
    for k in range(51):
        assert np.array_equal(o["dev"][k, :, :, :3], dx) and np.array_equal(o["dev"][k, :, :, 3:], dev0[:, :, 3:])
        dx = dx + dev0[:, :, 3:] * np.float64(0.03)
    assert np.all(o["log2"] == 0) and np.all(o["renorms"] == 0)


# ---- one body ----------------------------------------------------------------------------------
# the worst |dz_k - cos(k theta)| of the binary64 model over 200 steps of dt = 0.1 (1.4 periods), measured below:
# 2.2e-12 (the orbit is the leapfrog's own circle only to the roundings of its steps, 7.6e-13 in r, and cos(k theta)
# collects k roundings of theta); times 10
CIRCLE_TOL = 2.2e-11


def test_the_vertical_deviation_of_a_circular_orbit_follows_the_leapfrogs_closed_form():
    """One body of mass M at the origin, the tracer on the leapfrog's own circle of radius R -- positions R (cos k
    theta, sin k theta, 0) with 2 - 2 cos theta = (Omega dt)^2, Omega^2 = g M / (R (R^3 + e)), which the kick-drift-kick
    step keeps when |v_0| = R sin(theta) / dt.  There T_nn = -Omega^2, so delta = (n, 0) stays along n and follows
    cos(k theta): the leapfrog of a harmonic oscillator of frequency Omega from rest."""
    state = np.zeros((1, 10), np.float32)
    state[0, 9] = 1e6
    g, e = np.float64(np.float32(G)), np.float64(np.float32(E))
    Rad, dt, steps = 1.5, 0.1, 200
    w2 = g * 1e6 / (Rad * (Rad ** 3 + e))
    theta = np.arccos(1.0 - w2 * dt * dt / 2)
    pos = np.array([[Rad, 0.0, 0.0]])
    vel = np.array([[0.0, Rad * np.sin(theta) / dt, 0.0]])
    dev0 = np.zeros((1, 1, 6))
    dev0[0, 0, 2] = 1.0
    sample, tensor = S.exact64(state, G, E)
    o = S.stability(sample, tensor, pos, vel, dev0, dt=dt, steps=steps, every=1, renorm_log2=None, round_points=False)
    k = np.arange(steps + 1)
    drift = np.abs(np.linalg.norm(o["pos"][:, 0], axis=1) - Rad).max()
    print("circular orbit: worst |r_k - R|", drift)
    assert drift < 7.6e-12                 # the circle (measured 7.6e-13, the roundings of 200 steps; times 10)
    assert np.all(o["dev"][:, 0, 0, [0, 1, 3, 4]] == 0.0)                           # along n throughout
    worst = np.abs(o["dev"][:, 0, 0, 2] - np.cos(k * theta)).max()
    print("circular orbit: worst |dz_k - cos(k theta)|", worst, "over", k[-1] * theta / (2 * np.pi), "periods")
    assert worst <= CIRCLE_TOL
    assert o["dev"][:, 0, 0, 2].min() < -0.9                                        # (more than half a period)
