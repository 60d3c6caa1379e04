"""Orbit sections without a device: the entry points and layouts, the refusals that need no simulator,
nb_orbit_summary_merge against numpy, and the physics of the rule's restatement (tests/section_ref.py) in binary64
around one body: a circular orbit crosses b' = 0 once per turn of the pattern frame at the period the leapfrog has,
the interpolated crossing is second order in dt, an eccentric orbit alternates peri- and apocentres and winds once
per turn, a retrograde one winds backwards, and the three directions partition the same crossings."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import map_ref
from tests import orbit_ref as R
from tests import section_ref as S
from tests.helpers import ROOT

NAMES = ("nb_orbit_sections_sim", "nb_orbit_sections_runner", "nb_orbit_summary_merge")

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "nbody.h"
#define F(T, x) printf(#T "." #x " %zu %zu\n", offsetof(T, x), sizeof(((T *)0)->x));
#define S(T) printf(#T " %zu %zu\n", sizeof(T), _Alignof(T));
int main(void) {
    S(nb_orbit_section_params) F(nb_orbit_section_params, normal) F(nb_orbit_section_params, offset)
    F(nb_orbit_section_params, direction) F(nb_orbit_section_params, max_crossings)
    F(nb_orbit_section_params, flags) F(nb_orbit_section_params, reserved)
    S(nb_orbit_crossing) F(nb_orbit_crossing, xi) F(nb_orbit_crossing, eta) F(nb_orbit_crossing, time)
    F(nb_orbit_crossing, step)
    S(nb_orbit_summary) F(nb_orbit_summary, r2_min) F(nb_orbit_summary, r2_max) F(nb_orbit_summary, R2_min)
    F(nb_orbit_summary, R2_max) F(nb_orbit_summary, h_max) F(nb_orbit_summary, lz_min) F(nb_orbit_summary, lz_max)
    F(nb_orbit_summary, first_peri) F(nb_orbit_summary, last_peri) F(nb_orbit_summary, pericentres)
    F(nb_orbit_summary, apocentres) F(nb_orbit_summary, plane_ups) F(nb_orbit_summary, winding_pattern)
    F(nb_orbit_summary, winding_inertial) F(nb_orbit_summary, reserved)
    S(nb_orbit_section_stats) F(nb_orbit_section_stats, orbit) F(nb_orbit_section_stats, crossings)
    F(nb_orbit_section_stats, stored) F(nb_orbit_section_stats, overflowed)
    printf("NB_ORBIT_SECTION_MAX_CROSSINGS %u 0\n", NB_ORBIT_SECTION_MAX_CROSSINGS);
    printf("NB_ORBIT_NO_STEP %llu 0\n", (unsigned long long)NB_ORBIT_NO_STEP);
    return 0;
}
"""


# ---- the C surface -----------------------------------------------------------------------------
def test_entry_points_are_exported(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.ABI_SYMBOLS, name
    for name in ("OrbitSections", "OrbitSectionStats"):
        assert name in nb.__all__ and hasattr(nb, name)
    assert nb.Simulator.orbit_sections is nb.OfflineHeadless.orbit_sections is nb._Passes.orbit_sections
    assert nb.Simulator.jacobi_launch is nb.OfflineHeadless.jacobi_launch is nb._Passes.jacobi_launch
    a, b = L.nb_orbit_sections_sim.argtypes, L.nb_orbit_sections_runner.argtypes
    assert a is not None and list(a) == list(b) and len(a) == 12
    hpp = open(os.path.join(ROOT, "wgpu_n_body_amd", "csrc", "simulator.hpp")).read()
    assert "static constexpr auto orbit_sections = nb_orbit_sections_sim;" in hpp
    assert "static constexpr auto orbit_sections = nb_orbit_sections_runner;" in hpp
    assert "OrbitSections orbit_sections(" in hpp


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
    for T, size in ((_lib.nb_orbit_section_params, 48), (_lib.nb_orbit_crossing, 64), (_lib.nb_orbit_summary, 96),
                    (_lib.nb_orbit_section_stats, 80)):
        name = T.__name__
        assert info[name] == (C.sizeof(T), C.alignment(T)) and C.sizeof(T) == size, name
        for f, _ in T._fields_:
            assert info[f"{name}.{f}"] == (getattr(T, f).offset, getattr(T, f).size), (name, f)
        assert len(T._fields_) == sum(1 for k in info if k.startswith(name + "."))
    for dt, T, ref in ((_lib.ORBIT_CROSSING_DTYPE, _lib.nb_orbit_crossing, S.CROSSING),
                       (_lib.ORBIT_SUMMARY_DTYPE, _lib.nb_orbit_summary, S.SUMMARY)):
        assert dt.itemsize == C.sizeof(T) and dt == ref
        assert all(dt.fields[f][1] == getattr(T, f).offset for f in dt.names) and len(dt.names) == len(T._fields_)
    assert info["NB_ORBIT_SECTION_MAX_CROSSINGS"][0] == _lib.NB_ORBIT_SECTION_MAX_CROSSINGS == 1 << 22
    assert info["NB_ORBIT_NO_STEP"][0] == _lib.NB_ORBIT_NO_STEP == int(S.NO_STEP)


# ---- the refusals ------------------------------------------------------------------------------
def _params(_lib, **kw):
    p = _lib.nb_orbit_params()
    p.dt, p.step0, p.steps, p.every, p.flags, p.reserved = 0.02, 0, 5, 5, 0, 0
    p.accel_scale, p.omega = 1.0, 0.0
    p.axis[:], p.center[:] = (0.0, 1.0, 0.0), (0.0, 0.0, 0.0)
    s = _lib.nb_orbit_section_params()
    s.normal[:] = (0.0, 1.0, 0.0)
    s.offset, s.direction, s.max_crossings, s.flags, s.reserved = 0.0, 1, 4, 0, 0
    for k, v in kw.items():
        if k in ("axis", "center"):
            getattr(p, k)[:] = v
        elif k == "normal":
            s.normal[:] = v
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
    tracks = np.zeros((2, 4), _lib.ORBIT_SAMPLE_DTYPE)
    cross = np.zeros((4, 4), _lib.ORBIT_CROSSING_DTYPE)
    co, counts = np.zeros(4, np.uint32), np.zeros(4, np.uint32)
    sm = np.zeros(4, _lib.ORBIT_SUMMARY_DTYPE)
    st = _lib.nb_orbit_section_stats()
    for call, who in ((L.nb_orbit_sections_sim, b"simulator"), (L.nb_orbit_sections_runner, b"runner")):
        def bad(word, params="ok", section="ok", x=pos.ctypes.data, v=vel.ctypes.data, m=4, t=tracks.ctypes.data,
                cr=cross.ctypes.data, **kw):
            p, s = _params(_lib, **kw)
            before = tracks.tobytes() + cross.tobytes() + counts.tobytes() + sm.tobytes()
            rc = call(None, None if params is None else C.byref(p), None if section is None else C.byref(s), x, v,
                      m, t, co.ctypes.data, cr, counts.ctypes.data, sm.ctypes.data, C.byref(st))
            assert rc == INV, (word, kw)
            assert word in L.nb_last_error(), (word, L.nb_last_error())
            assert tracks.tobytes() + cross.tobytes() + counts.tobytes() + sm.tobytes() == before

        bad(b"null " + who)                       # a null handle, everything else in order
        # everything nb_orbits_sim refuses
        bad(b"params", params=None)
        bad(b"pos", x=None)
        bad(b"vel", v=None)
        bad(b"tracks", t=None)
        bad(b"steps", steps=0)
        bad(b"steps", steps=_lib.NB_ORBIT_MAX_STEPS + 1)
        bad(b"every", every=0)
        bad(b"flag", flags=2)
        bad(b"reserved", reserved=1)
        bad(b"tracers", m=_lib.NB_ORBIT_MAX_TRACERS + 1, s_max_crossings=0)
        bad(b"samples", m=1 << 20, steps=8, every=1, s_max_crossings=0)
        for v in (nan, inf, 0.0):
            bad(b"dt", dt=v)
        for v in (nan, inf):
            bad(b"accel_scale", accel_scale=v)
            bad(b"omega", omega=v)
            bad(b"center", center=(0.0, v, 0.0))
            bad(b"axis", omega=0.7, axis=(0.0, v, 0.0))
        bad(b"axis", omega=0.7, axis=(0.0, 0.0, 0.0))
        # the section's own
        bad(b"section", section=None)
        for v in (nan, inf, -inf):
            bad(b"normal", normal=(0.0, v, 1.0))
            bad(b"offset", s_offset=v)
        bad(b"normal", normal=(0.0, -0.0, 0.0))
        for v in (-2, 2, 7, -(1 << 31)):
            bad(b"direction", s_direction=v)
        bad(b"flag", s_flags=1)
        bad(b"reserved", s_reserved=1)
        bad(b"crossings", m=4, s_max_crossings=(1 << 20) + 1)       # 4 x (2^20 + 1) > 2^22
        bad(b"crossings", m=1 << 20, steps=5, every=5, s_max_crossings=5)
        bad(b"null crossings", cr=None)
        # the frame is needed without a pattern speed too
        bad(b"axis", omega=0.0, axis=(0.0, 0.0, 0.0))
        bad(b"axis", omega=0.0, axis=(nan, 0.0, 0.0))
        # in order, so that only the handle is at fault: null crossings with max_crossings = 0, the other outputs
        # null, m = 0 without arrays, every direction, m * max_crossings = 2^22 exactly
        p, s = _params(_lib, s_max_crossings=0)
        assert call(None, C.byref(p), C.byref(s), pos.ctypes.data, vel.ctypes.data, 4, tracks.ctypes.data, None, None,
                    None, None, None) == INV and b"null " + who in L.nb_last_error()
        p, s = _params(_lib)
        assert call(None, C.byref(p), C.byref(s), None, None, 0, None, None, None, None, None, None) == INV \
            and b"null " + who in L.nb_last_error()
        for d in (-1, 0, 1):
            bad(b"null " + who, s_direction=d)
        bad(b"null " + who, m=4, s_max_crossings=1 << 20)


# ---- nb_orbit_summary_merge --------------------------------------------------------------------
def _summary(**kw):
    a = np.zeros(1, S.SUMMARY)
    a["r2_min"], a["R2_min"], a["lz_min"] = np.inf, np.inf, np.inf
    a["r2_max"], a["R2_max"], a["lz_max"], a["h_max"] = -np.inf, -np.inf, -np.inf, -np.inf
    a["first_peri"] = a["last_peri"] = S.NO_STEP
    for k, v in kw.items():
        a[k] = v
    return a


def test_summary_merge_against_numpy(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    none = _summary()
    one = _summary(r2_min=1.0, r2_max=4.0, R2_min=0.5, R2_max=3.0, h_max=0.25, lz_min=-1.0, lz_max=2.0, first_peri=7,
                   last_peri=31, pericentres=3, apocentres=2, plane_ups=5, winding_pattern=-2, winding_inertial=4)
    two = _summary(r2_min=2.0, r2_max=9.0, R2_min=0.25, R2_max=2.0, h_max=0.5, lz_min=-3.0, lz_max=1.0, first_peri=40,
                   last_peri=40, pericentres=1, apocentres=1, plane_ups=0, winding_pattern=3, winding_inertial=-1)
    peri_less = _summary(r2_min=0.1, r2_max=0.2, R2_min=0.1, R2_max=0.2, h_max=0.0, lz_min=0.0, lz_max=0.0,
                         apocentres=1, winding_pattern=(1 << 31) - 5)
    cases = [(none, none), (one, none), (none, one), (one, two), (two, one), (one, peri_less), (peri_less, two),
             (peri_less, peri_less), (one, one)]
    for a, b in cases:
        out = np.zeros(1, S.SUMMARY)
        out["reserved"] = 77
        assert L.nb_orbit_summary_merge(a.ctypes.data, b.ctypes.data, out.ctypes.data) == 0
        want = S.merge(a, b)
        assert out.tobytes() == want.tobytes(), (a, b, out, want)
    got = np.zeros(1, S.SUMMARY)
    L.nb_orbit_summary_merge(one.ctypes.data, two.ctypes.data, got.ctypes.data)
    assert (got["first_peri"][0], got["last_peri"][0], got["pericentres"][0]) == (7, 40, 4)
    L.nb_orbit_summary_merge(peri_less.ctypes.data, two.ctypes.data, got.ctypes.data)
    assert (got["first_peri"][0], got["last_peri"][0]) == (40, 40)
    L.nb_orbit_summary_merge(one.ctypes.data, peri_less.ctypes.data, got.ctypes.data)
    assert (got["first_peri"][0], got["last_peri"][0]) == (7, 31)
    L.nb_orbit_summary_merge(none.ctypes.data, none.ctypes.data, got.ctypes.data)
    assert got["first_peri"][0] == got["last_peri"][0] == S.NO_STEP and got["r2_min"][0] == np.inf
    # in place
    acc = one.copy()
    assert L.nb_orbit_summary_merge(acc.ctypes.data, two.ctypes.data, acc.ctypes.data) == 0
    assert acc.tobytes() == S.merge(one, two).tobytes()
    INV = _lib.NB_ERR_INVALID
    assert L.nb_orbit_summary_merge(None, two.ctypes.data, acc.ctypes.data) == INV
    assert L.nb_orbit_summary_merge(one.ctypes.data, None, acc.ctypes.data) == INV
    assert L.nb_orbit_summary_merge(one.ctypes.data, two.ctypes.data, None) == INV


# ---- the restatement's physics: one body, g M = 1 ----------------------------------------------------------
# The law is g M / (r^3 + e).  Without the softening it is 1 / r^3, whose circular orbits are neutral (kappa^2 =
# (3 + d ln F / d ln r) Omega^2 = 0): every integrator's error then grows along the orbit and no bound orbit has a
# peri- and an apocentre.  With e = 1 and R = 0.5, d ln F / d ln r = -3 r^3 / (r^3 + e) = -1/3 and kappa^2 =
# 8/3 Omega^2: the circular orbit is stable and its neighbours are rosettes.
G_, E_, M_ = 1e-6, 1.0, 1e6
AXIS = (0.0, 0.0, 1.0)
FRAME = map_ref.frame(AXIS)  # (n, e1, e2)
RADIUS = 0.5
OMEGA_C = float(np.sqrt(G_ * M_ / (RADIUS * (RADIUS ** 3 + E_))))  # v^2 / r = g M / (r^3 + e)


def _one_body():
    s = np.zeros((1, 10), np.float32)
    s[0, 9] = M_
    return s


def _run(x0, v0, **kw):
    kw.setdefault("axis", AXIS)
    return S.sections(R.all_pairs64(_one_body(), G_, E_), [x0], [v0], **kw)


def _circular(sign=1.0):
    n, e1, e2 = FRAME
    return RADIUS * e1, sign * OMEGA_C * RADIUS * e2


@pytest.mark.parametrize("omega", [0.0, 0.3, -0.5, 1.7])
def test_a_circular_orbit_crosses_once_per_turn_of_the_pattern_frame(omega):
    """Successive up-crossings of b' = 0 are 2 pi / |Omega - omega| apart within (Omega dt)^2 relative: the
    leapfrog's frequency error for a harmonic oscillator is (Omega dt)^2 / 24, and the bound is 24 times that to cover
    the law's nonlinearity and the interpolation."""
    dt = 0.05
    x0, v0 = _circular()
    period = 2 * np.pi / abs(OMEGA_C - omega)
    turns = 4
    steps = int(np.ceil((turns + 0.25) * period / dt))
    o = _run(x0, v0, dt=dt, steps=steps, omega=omega, normal=(0.0, 1.0, 0.0), direction=1, max_crossings=16)
    k = int(o["counts"][0])
    # the tracer starts on b' = 0 itself (s_0 >= 0: no crossing there); (turns + 1/4) periods hold `turns` ups,
    # after 1, 2, ... periods when it moves forwards in the frame and after 1/2, 3/2, ... when it moves backwards
    assert k == turns, (k, omega)
    t = o["crossings"]["time"][0, :k]
    gaps = np.diff(t)
    bound = (OMEGA_C * dt) ** 2
    print("omega", omega, "gaps / period - 1", gaps / period - 1, "bound", bound)
    assert np.all(np.abs(gaps / period - 1) <= bound)
    step = o["crossings"]["step"][0, :k]
    assert np.all(step * dt <= t) and np.all(t < (step + 1) * dt)
    xi = o["crossings"]["xi"][0, :k]
    assert np.all(np.abs(xi[:, 1]) <= 1e-15) and np.all(xi[:, 2] == 0)  # on the plane, to rounding
    assert np.all(xi[:, 0] * np.sign(OMEGA_C - omega) > 0.9 * RADIUS)
    # (the pattern sees the tracer pass at (Omega - omega) R)
    assert np.allclose(o["crossings"]["eta"][0, :k, 1], (OMEGA_C - omega) * xi[:, 0], rtol=0.0, atol=2 * bound)
    sm = o["summaries"][0]
    assert sm["winding_inertial"] == int((turns + 0.25) * period * OMEGA_C / (2 * np.pi))
    # (backwards, b' = 0 >= 0 at state 0 is left downwards at once: the start counts as a passage)
    assert sm["winding_pattern"] == (turns if omega < OMEGA_C else -(turns + 1))
    assert sm["plane_ups"] == 0 and sm["h_max"] == 0


def test_the_interpolated_crossing_is_second_order():
    """a' - R of the first return has two parts, both of second order: the chord between two states of a circle lies
    inside it by R (Omega dt)^2 f (1 - f) / 2 at the fraction f, and the leapfrog's own orbit is an epicycle of
    amplitude ~ (Omega dt)^2 about the circle, read at the same time whatever dt.  dt = T / (k + 1/3) puts the return
    at f = 1/3, and half of it at f = 2/3: the same f (1 - f), so the sum falls by four; the test allows 3 to 5."""
    x0, v0 = _circular()
    period = 2 * np.pi / OMEGA_C
    errs = []
    for halvings in (0, 1):
        dt = period / (100 + 1.0 / 3.0) / 2 ** halvings
        o = _run(x0, v0, dt=dt, steps=int(1.2 * period / dt), max_crossings=2)
        assert o["counts"][0] == 1
        c = o["crossings"][0, 0]
        f = (c["time"] - c["step"] * dt) / dt
        errs.append(c["xi"][0] - RADIUS)
        print("dt", dt, "f", f, "a' - R", errs[-1], "chord", -RADIUS * (OMEGA_C * dt) ** 2 * f * (1 - f) / 2)
        assert abs(f - (1 + halvings) / 3.0) < 0.05
    assert errs[1] != 0 and 3.0 <= errs[0] / errs[1] <= 5.0


def _eccentric(sign=1.0, tilt=0.1):
    n, e1, e2 = FRAME
    return RADIUS * e1, sign * 0.8 * OMEGA_C * RADIUS * e2 + tilt * n  # at its apocentre, slightly inclined


@pytest.mark.parametrize("omega", [0.0, 0.3])
def test_an_eccentric_orbit_alternates_and_winds_once_per_turn(omega):
    dt, steps = 0.02, 1500
    x0, v0 = _eccentric()
    states = []
    o = _run(x0, v0, dt=dt, steps=steps, omega=omega, max_crossings=64, states=states)
    sm = o["summaries"][0]
    D = np.array([st[2]["D"][0] for st in states])
    # the sign changes of D alternate (the test's own reading of the states, not the restatement's counters)
    sign = D >= 0
    flips = np.nonzero(sign[1:] != sign[:-1])[0]
    kinds = sign[flips + 1]  # True: an up, a pericentre
    assert len(flips) >= 4 and np.all(kinds[1:] != kinds[:-1])
    assert sm["pericentres"] == int(kinds.sum()) and sm["apocentres"] == int((~kinds).sum())
    assert abs(int(sm["pericentres"]) - int(sm["apocentres"])) <= 1
    assert sm["first_peri"] == flips[kinds][0] + 1 and sm["last_peri"] == flips[kinds][-1] + 1
    # windings: the unwrapped angle in the inertial and in the pattern frame
    for key, a, b in (("winding_inertial", [st[2]["a"][0] for st in states], [st[2]["b"][0] for st in states]),
                      ("winding_pattern", [st[2]["xi"][0, 0] for st in states], [st[2]["xi"][0, 1] for st in states])):
        phi = np.unwrap(np.arctan2(b, a))
        assert phi[-1] > 4 * np.pi and sm[key] == int(np.floor(phi[-1] / (2 * np.pi))), key
    # extrema
    xi = np.array([st[2]["xi"][0] for st in states])
    r2 = (xi ** 2).sum(1)
    assert np.all(sm["r2_min"] <= r2 * (1 + 4e-16)) and np.all(r2 * (1 - 4e-16) <= sm["r2_max"])
    assert sm["r2_max"] == pytest.approx(RADIUS ** 2, rel=1e-3)  # (it starts at its apocentre)
    assert 0 < sm["r2_min"] < 0.75 * RADIUS ** 2 and sm["R2_min"] <= sm["r2_min"] and sm["R2_max"] <= sm["r2_max"]
    assert sm["h_max"] == np.abs(xi[:, 2]).max() > 0 and sm["plane_ups"] >= 2
    L = np.array([st[2]["L"][0] for st in states])
    assert sm["lz_min"] == L.min() and sm["lz_max"] == L.max() and L.min() > 0
    # a central force, but sampled at the fp32 point: a torque of at most |a| r 2^-24 <= 6e-8 over t = 30
    assert np.ptp(L) <= 1e-5
    # the derived figures a caller reads: the radial period between the first and the last pericentre
    assert sm["pericentres"] >= 2
    t_r = (int(sm["last_peri"]) - int(sm["first_peri"])) * dt / (int(sm["pericentres"]) - 1)
    assert 0.5 * 2 * np.pi / OMEGA_C < t_r < 2 * np.pi / OMEGA_C


def test_a_retrograde_tracer_winds_backwards():
    x0, v0 = _eccentric(sign=-1.0)
    for omega in (0.0, 0.3):
        o = _run(x0, v0, dt=0.02, steps=1500, omega=omega, direction=0, max_crossings=64)
        sm = o["summaries"][0]
        assert sm["winding_inertial"] <= -2 and sm["winding_pattern"] <= sm["winding_inertial"]
        assert sm["lz_max"] < 0 and sm["pericentres"] >= 2


def test_the_three_directions_partition_the_crossings():
    x0, v0 = _eccentric()
    kw = dict(dt=0.02, steps=1500, omega=0.3, normal=(0.6, 0.8, 0.5), offset=0.05, max_crossings=64)
    both, ups, downs = (_run(x0, v0, direction=d, **kw) for d in (0, 1, -1))
    nb_, nu, nd = (int(o["counts"][0]) for o in (both, ups, downs))
    assert nu >= 3 and nd >= 3 and nb_ == nu + nd and abs(nu - nd) <= 1
    merged = np.concatenate([ups["crossings"][0, :nu], downs["crossings"][0, :nd]])
    merged = merged[np.argsort(merged["time"], kind="stable")]
    assert merged.tobytes() == both["crossings"][0, :nb_].tobytes()
    assert np.all(np.diff(both["crossings"]["time"][0, :nb_]) > 0)
    assert not both["crossings"][0, nb_:].tobytes().strip(b"\0")  # unwritten slots are zero bytes
    for o in (ups, downs):  # the summaries do not depend on the section
        assert o["summaries"].tobytes() == both["summaries"].tobytes()
    # every stored crossing lies on the plane, and eta points through it the way its direction says
    normal = np.array(kw["normal"])
    for o, n_, sgn in ((ups, nu, 1), (downs, nd, -1)):
        c = o["crossings"][0, :n_]
        assert np.all(np.abs(c["xi"] @ normal - kw["offset"]) <= 1e-14)
        assert np.all(sgn * (c["eta"] @ normal) > 0)
    # a list shorter than the crossings keeps the first ones, in order, and counts them all
    short = _run(x0, v0, direction=0, **{**kw, "max_crossings": 3})
    assert short["counts"][0] == nb_ and short["crossings"][0].tobytes() == both["crossings"][0, :3].tobytes()
