"""Orbits without a device: nb_orbit_records and nb_orbit_phase, the refusals that need no simulator, the entry
points and the layouts, and that the restatement of the rule (tests/orbit_ref.py) in binary64 is a second-order
leapfrog that conserves the Jacobi integral of a rotating pattern and not the plain energy."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import orbit_ref as R
from tests.helpers import ROOT

NAMES = ("nb_orbits_sim", "nb_orbits_runner", "nb_orbit_records", "nb_orbit_phase")

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "nbody.h"
#define F(T, x) printf(#T "." #x " %zu %zu\n", offsetof(T, x), sizeof(((T *)0)->x));
#define S(T) printf(#T " %zu %zu\n", sizeof(T), _Alignof(T));
int main(void) {
    S(nb_orbit_params) F(nb_orbit_params, dt) F(nb_orbit_params, step0) F(nb_orbit_params, steps)
    F(nb_orbit_params, every) F(nb_orbit_params, flags) F(nb_orbit_params, reserved) F(nb_orbit_params, accel_scale)
    F(nb_orbit_params, omega) F(nb_orbit_params, axis) F(nb_orbit_params, center)
    S(nb_orbit_sample) F(nb_orbit_sample, pos) F(nb_orbit_sample, vel) F(nb_orbit_sample, potential)
    F(nb_orbit_sample, energy)
    S(nb_orbit_stats) F(nb_orbit_stats, step_num) F(nb_orbit_stats, n) F(nb_orbit_stats, nonfinite)
    F(nb_orbit_stats, tracers) F(nb_orbit_stats, nonfinite_tracers) F(nb_orbit_stats, records)
    F(nb_orbit_stats, pair_launches) F(nb_orbit_stats, flags) F(nb_orbit_stats, reserved)
    printf("NB_ORBIT_ENERGY %u 0\n", NB_ORBIT_ENERGY);
    printf("NB_ORBIT_MAX_TRACERS %u 0\n", NB_ORBIT_MAX_TRACERS);
    printf("NB_ORBIT_MAX_STEPS %u 0\n", NB_ORBIT_MAX_STEPS);
    printf("NB_ORBIT_MAX_SAMPLES %u 0\n", NB_ORBIT_MAX_SAMPLES);
    printf("NB_ORBIT_MAX_PAIRS_LOG2 %u 0\n", NB_ORBIT_MAX_PAIRS_LOG2);
    return 0;
}
"""


# ---- the host-only entry points ----------------------------------------------------------------
@pytest.mark.parametrize("steps,every,want", [(1, 1, 2), (5, 2, 4), (6, 3, 3), (6, 2, 4), (1, 7, 2), (7, 7, 2),
                                              (8, 7, 3), (100, 1, 101), (1 << 20, 1 << 20, 2), (1 << 20, 3, 349527),
                                              (0xFFFFFFFF, 0xFFFFFFFF, 2), (5, 0, 0)])
def test_orbit_records(nb, steps, every, want):
    from wgpu_n_body_amd import _lib
    assert _lib.lib().nb_orbit_records(steps, every) == want
    if every and steps <= 1 << 20:
        assert len(R.records(steps, every)) == want


def test_orbit_phase(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    c, s = C.c_double(), C.c_double()
    rng = np.random.default_rng(1)
    ks = [0, 1, 2, 3, 1000, (1 << 20) + 5, (1 << 40) - 1, 1 << 40] + [int(k) for k in rng.integers(0, 1 << 40, 40)]
    for omega, dt in ((0.7, 0.02), (-0.31, 0.016), (2.5, -0.001), (1e-3, 1e-4)):
        for k in ks:
            assert L.nb_orbit_phase(omega, dt, k, C.byref(c), C.byref(s)) == 0
            theta = np.float64(omega) * (np.float64(k) * np.float64(dt))
            assert abs(c.value - np.cos(theta)) <= 2.0 ** -52 and abs(s.value - np.sin(theta)) <= 2.0 ** -52, (omega, k)
    for k in ks:  # no rotation: exactly (1, 0), whatever the time
        assert L.nb_orbit_phase(0.0, 0.02, k, C.byref(c), C.byref(s)) == 0 and (c.value, s.value) == (1.0, 0.0)
        assert L.nb_orbit_phase(-0.0, 0.02, k, C.byref(c), C.byref(s)) == 0 and (c.value, s.value) == (1.0, 0.0)
    INV = _lib.NB_ERR_INVALID
    assert L.nb_orbit_phase(0.7, 0.02, 1, None, C.byref(s)) == INV and L.nb_orbit_phase(0.7, 0.02, 1, C.byref(c), None) == INV
    assert L.nb_orbit_phase(float("nan"), 0.02, 1, C.byref(c), C.byref(s)) == INV
    assert L.nb_orbit_phase(0.7, float("inf"), 1, C.byref(c), C.byref(s)) == INV


# ---- the refusals ------------------------------------------------------------------------------
def _params(_lib, **kw):
    p = _lib.nb_orbit_params()
    p.dt, p.step0, p.steps, p.every, p.flags, p.reserved = 0.02, 0, 5, 2, 0, 0
    p.accel_scale, p.omega = 1.0, 0.0
    p.axis[:], p.center[:] = (0.0, 1.0, 0.0), (0.0, 0.0, 0.0)
    for k, v in kw.items():
        if k in ("axis", "center"):
            getattr(p, k)[:] = v
        else:
            setattr(p, k, v)
    return p


def test_bad_arguments_are_invalid_without_a_device(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    INV = _lib.NB_ERR_INVALID
    nan, inf = float("nan"), float("inf")
    pos, vel = np.zeros((4, 3)), np.zeros((4, 3))
    tracks = np.zeros((4, 4), _lib.ORBIT_SAMPLE_DTYPE)
    co = np.zeros(4, np.uint32)
    st = _lib.nb_orbit_stats()
    for call, who in ((L.nb_orbits_sim, b"simulator"), (L.nb_orbits_runner, b"runner")):
        def bad(word, params="ok", x=pos.ctypes.data, v=vel.ctypes.data, m=4, t=tracks.ctypes.data, **kw):
            p = _params(_lib, **kw)
            before = tracks.tobytes()
            rc = call(None, None if params is None else C.byref(p), x, v, m, t, co.ctypes.data, C.byref(st))
            assert rc == INV, (word, kw)
            assert word in L.nb_last_error(), (word, L.nb_last_error())
            assert tracks.tobytes() == before

        bad(b"null " + who)                       # a null handle, everything else in order
        bad(b"params", params=None)
        bad(b"pos", x=None)
        bad(b"vel", v=None)
        bad(b"tracks", t=None)
        bad(b"steps", steps=0)
        bad(b"steps", steps=_lib.NB_ORBIT_MAX_STEPS + 1)
        bad(b"every", every=0)
        bad(b"flag", flags=2)
        bad(b"flag", flags=0x80000001)
        bad(b"reserved", reserved=1)
        bad(b"tracers", m=_lib.NB_ORBIT_MAX_TRACERS + 1)
        bad(b"samples", m=1 << 20, steps=8, every=1)          # 9 records x 2^20 tracers
        bad(b"samples", steps=1 << 20, every=1)               # 2^20 + 1 records x 4 tracers
        for v in (nan, inf, -inf, 0.0, -0.0):
            bad(b"dt", dt=v)
        for v in (nan, inf):
            bad(b"accel_scale", accel_scale=v)
            bad(b"omega", omega=v)
            bad(b"center", center=(0.0, v, 0.0))
            bad(b"axis", omega=0.7, axis=(0.0, v, 0.0))
        bad(b"axis", omega=0.7, axis=(0.0, 0.0, 0.0))
        # without a pattern speed the axis is not looked at: only the handle is then at fault
        bad(b"null " + who, omega=0.0, axis=(0.0, 0.0, 0.0))
        bad(b"null " + who, omega=0.0, axis=(nan, 0.0, 0.0))
        # m = 0 needs no array; coincident and stats may be null
        p = _params(_lib)
        assert call(None, C.byref(p), None, None, 0, None, None, None) == INV and b"null " + who in L.nb_last_error()


# ---- the C surface -----------------------------------------------------------------------------
def test_orbit_entry_points_are_exported(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.ABI_SYMBOLS, name
    for name in ("Orbits", "OrbitStats"):
        assert name in nb.__all__ and hasattr(nb, name)
    # one method, shared by the two owners of a state
    assert nb.Simulator.orbits is nb.OfflineHeadless.orbits is nb._Passes.orbits
    assert nb.Simulator.circular_orbits is nb.OfflineHeadless.circular_orbits is nb._Passes.circular_orbits
    assert L.nb_orbits_sim.argtypes is not None and list(L.nb_orbits_sim.argtypes) == list(L.nb_orbits_runner.argtypes)
    # the C++ mirror names the same pass for both handle types, and the same method
    hpp = open(os.path.join(ROOT, "wgpu_n_body_amd", "csrc", "simulator.hpp")).read()
    assert "static constexpr auto orbits = nb_orbits_sim;" in hpp
    assert "static constexpr auto orbits = nb_orbits_runner;" in hpp
    assert "Orbits orbits(" in hpp


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
    for S, size in ((_lib.nb_orbit_params, 96), (_lib.nb_orbit_sample, 64), (_lib.nb_orbit_stats, 56)):
        name = S.__name__
        assert info[name] == (C.sizeof(S), C.alignment(S)) and C.sizeof(S) == size, name
        for f, _ in S._fields_:
            assert info[f"{name}.{f}"] == (getattr(S, f).offset, getattr(S, f).size), (name, f)
        assert len(S._fields_) == sum(1 for k in info if k.startswith(name + "."))
    dt = _lib.ORBIT_SAMPLE_DTYPE
    assert dt.itemsize == 64 and all(dt.fields[f][1] == getattr(_lib.nb_orbit_sample, f).offset for f in dt.names)
    for name in ("NB_ORBIT_ENERGY", "NB_ORBIT_MAX_TRACERS", "NB_ORBIT_MAX_STEPS", "NB_ORBIT_MAX_SAMPLES",
                 "NB_ORBIT_MAX_PAIRS_LOG2"):
        assert info[name][0] == getattr(_lib, name), name


# ---- the restatement ---------------------------------------------------------------------------
def restated_ranges(omega, dt, t_end=2.0):
    """(range of the recorded energy, range of 0.5 v^2 + Phi) of the case, every state recorded."""
    steps = int(round(t_end / dt))
    o = R.orbits(R.all_pairs64(R.binary_state(), R.CASE_G, R.CASE_E), [R.CASE_X0], [R.CASE_V0], dt=dt, steps=steps,
                 energy=True, omega=omega, axis=(0.0, 0.0, 1.0))
    v = o["vel"][:, 0]
    plain = 0.5 * (v * v).sum(1) + o["potential"][:, 0]
    return np.ptp(o["energy"][:, 0]), np.ptp(plain)


def test_the_restatement_is_a_second_order_leapfrog():
    """Halving dt quarters the error of the conserved quantity: the Jacobi integral with a pattern speed (its range
    is 2.19e-5 at dt = 0.02 and 5.49e-6 at dt = 0.01), the energy without (2.0e-6 and 5.0e-7).  With the pattern
    turning the plain energy is not conserved at all: its range, 0.122, does not care about dt."""
    j2, p2 = restated_ranges(0.7, 0.02)
    j1, p1 = restated_ranges(0.7, 0.01)
    print("jacobi range", j2, j1, j2 / j1, "plain energy range", p2, p1)
    assert 3.5 <= j2 / j1 <= 4.5
    # (the quoted figures to a few per cent: they depend on which states are looked at, the ratio does not)
    assert abs(j2 - 2.19e-5) <= 0.05 * 2.19e-5 and abs(j1 - 5.49e-6) <= 0.05 * 5.49e-6
    assert abs(p2 - 0.122) <= 0.05 * 0.122 and abs(p1 - 0.122) <= 0.05 * 0.122
    e2, q2 = restated_ranges(0.0, 0.02)
    e1, q1 = restated_ranges(0.0, 0.01)
    print("energy range", e2, e1, e2 / e1)
    assert 3.5 <= e2 / e1 <= 4.5
    assert abs(e2 - 2.0e-6) <= 0.05 * 2.0e-6 and abs(e1 - 5.0e-7) <= 0.05 * 5.0e-7
    assert e2 == q2 and e1 == q1  # (without a pattern speed the recorded energy is the plain one)


def test_the_restatement_turns_with_the_pattern():
    """A tracer at rest in the turning frame of a field-free pattern: no force, so a straight line in the inertial
    frame, whatever omega; and the point the field is sampled at is x turned back by theta."""
    none = lambda p, pot: (np.zeros((len(p), 3)), np.zeros(len(p)), np.zeros(len(p), np.int64))  # noqa: E731
    o = R.orbits(none, [[1.0, 2.0, 3.0]], [[0.5, -0.25, 0.125]], dt=0.5, steps=4, omega=0.7, axis=(1.0, 2.0, 3.0))
    for r, k in enumerate(range(5)):
        x = np.array([1.0, 2.0, 3.0])
        for _ in range(k):
            x = x + np.array([0.5, -0.25, 0.125]) * 0.5
        assert np.array_equal(o["pos"][r, 0], x)
    frame = (np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]))
    c, s = R.phase_numpy(0.7, 0.5, 3)
    q = R.point(np.array([[1.0, 0.0, 0.25]]), frame, np.zeros(3), 0.7, c, s)
    assert np.allclose(q[0], [np.cos(1.05), -np.sin(1.05), 0.25], rtol=0, atol=1e-15)
    back = R.turn_back(q, frame, 0.7, c, s)
    assert np.allclose(back[0], [1.0, 0.0, 0.25], rtol=0, atol=1e-15)
