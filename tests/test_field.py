"""Field probes at the C-ABI boundary, without a device: the entry points are exported, the Python mirrors
have the C layout, bad arguments are refused before any device is touched, and the host-only helpers
(rings, ring means) give what can be worked out by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import ROOT

NAMES = ("nb_sim_field", "nb_runner_field", "nb_field_rings", "nb_field_ring_means")

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "nbody.h"
#define F(T, x) printf(#T "." #x " %zu %zu\n", offsetof(T, x), sizeof(((T *)0)->x));
#define S(T) printf(#T " %zu %zu\n", sizeof(T), _Alignof(T));
int main(void) {
    S(nb_field_sample) F(nb_field_sample, acc) F(nb_field_sample, potential) F(nb_field_sample, coincident)
    F(nb_field_sample, reserved)
    S(nb_field_stats) F(nb_field_stats, step_num) F(nb_field_stats, n) F(nb_field_stats, nonfinite)
    F(nb_field_stats, points) F(nb_field_stats, nonfinite_points) F(nb_field_stats, flags) F(nb_field_stats, launches)
    S(nb_field_ring) F(nb_field_ring, a_R) F(nb_field_ring, a_n) F(nb_field_ring, potential) F(nb_field_ring, v_c)
    printf("NB_FIELD_ACCEL %u 0\n", NB_FIELD_ACCEL);
    printf("NB_FIELD_POTENTIAL %u 0\n", NB_FIELD_POTENTIAL);
    printf("NB_FIELD_MAX_POINTS %u 0\n", NB_FIELD_MAX_POINTS);
    return 0;
}
"""

DP = C.POINTER(C.c_double)


def _v3(v):
    return (C.c_double * 3)(*v)


def test_field_entry_points_are_exported(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.ABI_SYMBOLS, name
    for name in ("Field", "RingMeans", "field_rings"):
        assert name in nb.__all__ and hasattr(nb, name)
    for cls in (nb.Simulator, nb.OfflineHeadless):
        assert hasattr(cls, "field") and hasattr(cls, "circular_velocity")


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
    assert info["nb_field_sample"][0] == 40
    for S, size in ((_lib.nb_field_sample, 40), (_lib.nb_field_stats, 48), (_lib.nb_field_ring, 32)):
        name = S.__name__
        assert info[name] == (C.sizeof(S), C.alignment(S)) and C.sizeof(S) == size, name
        for f, _ in S._fields_:
            assert info[f"{name}.{f}"] == (getattr(S, f).offset, getattr(S, f).size), (name, f)
        assert len(S._fields_) == sum(1 for k in info if k.startswith(name + "."))
    for S, dt in ((_lib.nb_field_sample, _lib.FIELD_SAMPLE_DTYPE), (_lib.nb_field_ring, _lib.FIELD_RING_DTYPE)):
        assert dt.itemsize == C.sizeof(S)
        for f, _ in S._fields_:
            assert dt.fields[f][1] == getattr(S, f).offset, f
    assert info["NB_FIELD_ACCEL"][0] == _lib.NB_FIELD_ACCEL == 1
    assert info["NB_FIELD_POTENTIAL"][0] == _lib.NB_FIELD_POTENTIAL == 2
    assert info["NB_FIELD_MAX_POINTS"][0] == _lib.NB_FIELD_MAX_POINTS == 1 << 24


def test_bad_arguments_are_invalid_without_a_device(nb):
    """Every refusal that does not need a simulator's parameters (potential with e < 0 is refused the same
    way, ahead of any device call, but needs a simulator: tests/test_field_gpu.py)."""
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    INV = _lib.NB_ERR_INVALID
    pts = np.zeros((4, 3), np.float32)
    out = np.zeros(4, _lib.FIELD_SAMPLE_DTYPE)
    st = _lib.nb_field_stats()
    BOTH = _lib.NB_FIELD_ACCEL | _lib.NB_FIELD_POTENTIAL
    for call, who in ((L.nb_sim_field, b"simulator"), (L.nb_runner_field, b"runner")):
        def bad(word, p=pts.ctypes.data, m=4, flags=BOTH, o=out.ctypes.data):
            assert call(None, p, m, flags, o, C.byref(st)) == INV, word
            assert word in L.nb_last_error(), (word, L.nb_last_error())

        bad(b"null " + who)                      # a null handle, everything else in order
        bad(b"points", p=None)
        bad(b"out", o=None)
        bad(b"flags", flags=0)
        bad(b"flags", flags=4)
        bad(b"flags", flags=BOTH | 8)
        bad(b"at most", m=(1 << 24) + 1)
        # m = 0 needs neither array: only the handle is then at fault; stats may be null
        assert call(None, None, 0, BOTH, None, None) == INV and b"null " + who in L.nb_last_error()


def _rings(L, center, axis, radii, n_phi):
    r = np.ascontiguousarray(radii, dtype=np.float64)
    pts = np.full((r.shape[0] * n_phi, 3), 7.0, np.float32)
    rc = L.nb_field_rings(_v3(center), _v3(axis), r.ctypes.data_as(DP), r.shape[0], n_phi, pts.ctypes.data)
    return rc, pts


def _basis(axis):
    """The rule of include/nbody.h, restated: n, e1 from the coordinate axis of the smallest |n_k|, e2 = n x e1."""
    n = np.asarray(axis, np.float64)
    n = n / np.sqrt((n * n).sum())
    s = int(np.argmin(np.abs(n)))  # (argmin returns the lowest index on ties)
    e1 = np.eye(3)[s] - n[s] * n
    e1 /= np.sqrt((e1 * e1).sum())
    return n, e1, np.cross(n, e1)


@pytest.mark.parametrize("axis", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, -3, 0), (1.0, 2.0, 3.0), (-2.0, 0.5, 0.5)])
def test_rings_lie_where_the_rule_puts_them(nb, axis):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    center = np.array([0.25, -1.5, 3.0])
    radii = np.array([0.0, 0.125, 1.0, 2.5, 40.0])
    n_phi = 12
    rc, pts = _rings(L, center, axis, radii, n_phi)
    assert rc == 0
    n, e1, e2 = _basis(axis)
    # the basis rule, for the axes along x, y, z by hand: e1 is the next coordinate axis that is not the axis
    by_hand = {(1, 0, 0): (0, 1, 0), (0, 1, 0): (1, 0, 0), (0, 0, 1): (1, 0, 0), (0, -3, 0): (1, 0, 0)}
    if tuple(axis) in by_hand:
        assert np.array_equal(e1, by_hand[tuple(axis)])
    assert abs(e1 @ n) < 1e-15 and abs(e2 @ n) < 1e-15 and abs(e1 @ e2) < 1e-15
    d = pts.astype(np.float64).reshape(len(radii), n_phi, 3) - center
    ulp = np.spacing(np.float32(np.abs(center).max() + radii))[:, None].astype(np.float64)  # one fp32 ulp of |c| + R
    # the axis is orthogonal to every point - centre, and the radii hold, to one fp32 ulp of |c| + R (each
    # coordinate is off by at most half of one: sqrt(3) / 2 of an ulp in any direction)
    assert np.all(np.abs(d @ n) <= ulp)
    assert np.all(np.abs(np.sqrt((d * d).sum(2)) - radii[:, None]) <= ulp)
    # evenly spaced azimuths, starting on e1 and turning towards e2
    phi = np.arctan2(d @ e2, d @ e1)
    want = 2.0 * np.pi * np.arange(n_phi) / n_phi
    for i in range(1, len(radii)):
        err = np.angle(np.exp(1j * (phi[i] - want)))
        assert np.all(np.abs(err) <= 2.0 * ulp[i] / radii[i]), (i, err)
    # formed in fp64 and rounded once: the restatement gives the same floats
    c, s = np.cos(want), np.sin(want)
    ref = center + radii[:, None, None] * (c[None, :, None] * e1 + s[None, :, None] * e2)
    assert np.array_equal(pts.reshape(ref.shape), ref.astype(np.float32))
    assert np.array_equal(pts[:n_phi], np.tile(center.astype(np.float32), (n_phi, 1)))  # radius 0: the centre


def test_rings_and_ring_means_refusals(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    INV = _lib.NB_ERR_INVALID
    nan, inf = float("nan"), float("inf")
    good = dict(center=(0, 0, 0), axis=(0, 1, 0), radii=[1.0, 2.0], n_phi=4)
    assert _rings(L, **good)[0] == 0
    for change in (dict(axis=(0, 0, 0)), dict(axis=(0, nan, 1)), dict(axis=(inf, 0, 0)), dict(axis=(1e-200, 0, 0)),
                   dict(center=(0, nan, 0)), dict(center=(inf, 0, 0)), dict(radii=[1.0, -1e-9]), dict(radii=[nan]),
                   dict(radii=[inf, 1.0]), dict(n_phi=0)):
        rc, pts = _rings(L, **{**good, **change})
        assert rc == INV and L.nb_last_error(), change
        assert np.all(pts == 7.0), change  # nothing written
    r = np.array([1.0, 2.0])
    pts = np.zeros((8, 3), np.float32)
    sam = np.zeros(8, _lib.FIELD_SAMPLE_DTYPE)
    out = np.zeros(2, _lib.FIELD_RING_DTYPE)
    args = lambda **kw: [kw.get("c", _v3((0, 0, 0))), kw.get("a", _v3((0, 1, 0))), kw.get("r", r.ctypes.data_as(DP)), 2,  # noqa: E731
                         kw.get("q", 4), kw.get("p", pts.ctypes.data), kw.get("s", sam.ctypes.data),
                         kw.get("o", out.ctypes.data)]
    assert L.nb_field_ring_means(*args()) == 0
    for kw in (dict(c=None), dict(a=None), dict(r=None), dict(p=None), dict(s=None), dict(o=None), dict(q=0),
               dict(a=_v3((0, 0, 0))), dict(c=_v3((nan, 0, 0)))):
        assert L.nb_field_ring_means(*args(**kw)) == INV, kw
    assert L.nb_field_rings(_v3((0, 0, 0)), _v3((0, 1, 0)), r.ctypes.data_as(DP), 2, 4, None) == INV


def _means(L, _lib, center, axis, radii, n_phi, pts, acc, pot):
    r = np.ascontiguousarray(radii, dtype=np.float64)
    sam = np.zeros(pts.shape[0], _lib.FIELD_SAMPLE_DTYPE)
    sam["acc"], sam["potential"] = acc, pot
    out = np.zeros(r.shape[0], _lib.FIELD_RING_DTYPE)
    assert L.nb_field_ring_means(_v3(center), _v3(axis), r.ctypes.data_as(DP), r.shape[0], n_phi, pts.ctypes.data,
                                 sam.ctypes.data, out.ctypes.data) == 0
    return out


@pytest.mark.parametrize("axis", [(0, 1, 0), (1.0, 2.0, 3.0)])
def test_ring_means_of_hand_made_fields(nb, axis):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    center = np.array([0.5, 0.25, -1.0])
    radii = np.array([0.5, 1.0, 3.0])
    n_phi = 8
    rc, pts = _rings(L, center, axis, radii, n_phi)
    assert rc == 0
    n, _, _ = _basis(axis)
    d = pts.astype(np.float64) - center
    rho = d - (d @ n)[:, None] * n
    R = np.sqrt((rho * rho).sum(1))
    rhat = rho / R[:, None]
    # a pure radial field -k / R^2 towards the axis, from the points actually used; potential -k / R
    k = 3.0
    m = _means(L, _lib, center, axis, radii, n_phi, pts, (-k / R ** 2)[:, None] * rhat, -k / R)
    a_R = (-k / R ** 2).reshape(3, n_phi).mean(1)
    assert np.allclose(m["a_R"], a_R, rtol=1e-14, atol=0)
    assert np.allclose(m["a_R"], -k / radii ** 2, rtol=1e-6)            # the nominal radii to fp32 rounding
    assert np.all(np.abs(m["a_n"]) <= 1e-15 * k / radii ** 2)
    assert np.allclose(m["potential"], (-k / R).reshape(3, n_phi).mean(1), rtol=1e-15, atol=0)
    assert np.array_equal(m["v_c"], np.sqrt(np.maximum(0.0, -radii * m["a_R"])))
    assert np.allclose(m["v_c"], np.sqrt(k / radii), rtol=1e-6)         # v_c^2 = k / R
    # an outward field has no circular orbit
    m = _means(L, _lib, center, axis, radii, n_phi, pts, (k / R ** 2)[:, None] * rhat, 0 * R)
    assert np.all(m["a_R"] > 0) and np.all(m["v_c"] == 0)
    # a uniform field along n gives a_n only
    m = _means(L, _lib, center, axis, radii, n_phi, pts, np.tile(2.5 * n, (len(R), 1)), np.full(len(R), -1.0))
    assert np.allclose(m["a_n"], 2.5, rtol=1e-15) and np.all(np.abs(m["a_R"]) <= 1e-15)
    assert np.all(m["v_c"] <= 1e-7) and np.all(m["potential"] == -1.0)
    # the Python wrapper returns the same points
    assert np.array_equal(nb.field_rings(radii, axis=axis, center=center, n_phi=n_phi), pts)
