"""Projected maps at the C-ABI boundary, without a device: the entry points are exported, the Python mirrors
have the C layout, bad arguments are refused before any device is touched, the host-only helpers (frame,
edges) give what can be worked out by hand, and the numpy restatement (tests/map_ref.py) equals a plain
Python double loop."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from tests import map_ref as M
from tests.helpers import ROOT

NAMES = ("nb_sim_map", "nb_runner_map", "nb_map_frame", "nb_map_edges")

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "nbody.h"
#define F(T, x) printf(#T "." #x " %zu %zu\n", offsetof(T, x), sizeof(((T *)0)->x));
#define S(T) printf(#T " %zu %zu\n", sizeof(T), _Alignof(T));
int main(void) {
    S(nb_map_params) F(nb_map_params, width) F(nb_map_params, height) F(nb_map_params, flags)
    F(nb_map_params, reserved) F(nb_map_params, center) F(nb_map_params, velocity) F(nb_map_params, axis)
    F(nb_map_params, x_range) F(nb_map_params, y_range) F(nb_map_params, depth_range)
    S(nb_map_stats) F(nb_map_stats, step_num) F(nb_map_stats, n) F(nb_map_stats, nonfinite)
    F(nb_map_stats, binned_count) F(nb_map_stats, outside_count) F(nb_map_stats, binned_mass)
    F(nb_map_stats, outside_mass) F(nb_map_stats, mass) F(nb_map_stats, center) F(nb_map_stats, velocity)
    F(nb_map_stats, n_hat) F(nb_map_stats, e1) F(nb_map_stats, e2) F(nb_map_stats, width) F(nb_map_stats, height)
    F(nb_map_stats, flags) F(nb_map_stats, max_count)
    printf("NB_MAP_MAX_SIDE %u 0\n", NB_MAP_MAX_SIDE);
    printf("NB_MAP_MAX_CELLS %u 0\n", NB_MAP_MAX_CELLS);
    printf("NB_MAP_CENTER_COM %u 0\n", NB_MAP_CENTER_COM);
    printf("NB_MAP_VELOCITY %u 0\n", NB_MAP_VELOCITY);
    return 0;
}
"""

DP = C.POINTER(C.c_double)


def _v3(v):
    return (C.c_double * 3)(*v)


def test_map_entry_points_are_exported(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.ABI_SYMBOLS, name
    for name in ("ProjectedMap", "map_frame", "map_edges"):
        assert name in nb.__all__ and hasattr(nb, name)
    for cls in (nb.Simulator, nb.OfflineHeadless):
        assert hasattr(cls, "projected_map")


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
    for S, size in ((_lib.nb_map_params, 136), (_lib.nb_map_stats, 200)):
        name = S.__name__
        assert info[name] == (C.sizeof(S), C.alignment(S)) and C.sizeof(S) == size, name
        for f, _ in S._fields_:
            assert info[f"{name}.{f}"] == (getattr(S, f).offset, getattr(S, f).size), (name, f)
        assert len(S._fields_) == sum(1 for k in info if k.startswith(name + "."))
    assert info["NB_MAP_MAX_SIDE"][0] == _lib.NB_MAP_MAX_SIDE == 4096
    assert info["NB_MAP_MAX_CELLS"][0] == _lib.NB_MAP_MAX_CELLS == 1 << 22
    assert info["NB_MAP_CENTER_COM"][0] == _lib.NB_MAP_CENTER_COM == 1
    assert info["NB_MAP_VELOCITY"][0] == _lib.NB_MAP_VELOCITY == 2


def good_params(_lib, **change):
    p = _lib.nb_map_params()
    p.width, p.height, p.flags, p.reserved = 16, 8, _lib.NB_MAP_VELOCITY, 0
    vals = dict(center=(0, 0, 0), velocity=(0, 0, 0), axis=(0, 1, 0), x_range=(-1, 1), y_range=(-2, 2),
                depth_range=(-math.inf, math.inf))
    for k, v in change.items():
        if k in vals:
            vals[k] = v
        else:
            setattr(p, k, v)
    for k, v in vals.items():
        for i, x in enumerate(v):
            getattr(p, k)[i] = x
    return p


def test_bad_arguments_are_invalid_without_a_device(nb):
    """Every refusal that needs no simulator: the parameters are checked before the handle is looked at, so a
    null handle with good parameters is the one refusal that names the handle."""
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    INV = _lib.NB_ERR_INVALID
    nan, inf = math.nan, math.inf
    counts = np.full(16 * 8, 7, np.uint32)
    planes = np.full(6 * 16 * 8, 7.0)
    st = _lib.nb_map_stats()
    for call, who in ((L.nb_sim_map, b"simulator"), (L.nb_runner_map, b"runner")):
        def bad(word, p):
            assert call(None, C.byref(p) if p is not None else None, counts.ctypes.data, planes.ctypes.data,
                        C.byref(st)) == INV, word
            assert word in L.nb_last_error(), (word, L.nb_last_error())

        bad(b"null " + who, good_params(_lib))
        bad(b"null " + who, good_params(_lib, depth_range=(-1.0, inf)))
        bad(b"params", None)
        for w, h in ((0, 8), (8, 0), (4097, 1), (1, 4097)):
            bad(b"side", good_params(_lib, width=w, height=h))
        bad(b"cells", good_params(_lib, width=4096, height=2048))
        bad(b"flag", good_params(_lib, flags=4))
        bad(b"flag", good_params(_lib, flags=3 | 8))
        bad(b"reserved", good_params(_lib, reserved=1))
        for axis in ((0, 0, 0), (nan, 1, 0), (0, inf, 0), (1e-200, 0, 0), (1e200, 1e200, 0)):
            bad(b"axis", good_params(_lib, axis=axis))
        bad(b"center", good_params(_lib, center=(0, nan, 0)))
        bad(b"center", good_params(_lib, velocity=(inf, 0, 0)))
        for rng in ((nan, 1), (0, inf), (-inf, 0), (1, 1), (2, 1)):
            bad(b"x_range", good_params(_lib, x_range=rng))
            bad(b"y_range", good_params(_lib, y_range=rng))
        bad(b"ascending", good_params(_lib, x_range=(1.0, 1.0 + 4e-16)))  # 16 cells in two ulps
        for rng in ((nan, 1), (0, nan), (1, 1), (2, 1), (inf, inf)):
            bad(b"depth", good_params(_lib, depth_range=rng))
        # a non-finite centre is no fault with NB_MAP_CENTER_COM: only the handle is then
        bad(b"null " + who, good_params(_lib, flags=_lib.NB_MAP_CENTER_COM, center=(nan, nan, nan)))
        # counts, planes and stats may each be null
        assert call(None, C.byref(good_params(_lib)), None, None, None) == INV and b"null " + who in L.nb_last_error()
    assert np.all(counts == 7) and np.all(planes == 7.0)  # nothing written


def _frame(L, axis):
    out = [(C.c_double * 3)() for _ in range(3)]
    rc = L.nb_map_frame(_v3(axis), *out)
    return rc, [np.array(list(v)) for v in out]


@pytest.mark.parametrize("axis", [(1.0, 2.0, 3.0), (-2.0, 0.5, 0.5), (0.3, -0.3, 0.1), (0, 1, 0), (0, 0, 1), (5, 0, 0)])
def test_frame_is_orthonormal_and_the_rings_frame(nb, axis):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    rc, (n, e1, e2) = _frame(L, axis)
    assert rc == 0
    for a, b, want in ((n, n, 1), (e1, e1, 1), (e2, e2, 1), (n, e1, 0), (n, e2, 0), (e1, e2, 0)):
        assert abs(a @ b - want) <= 1e-15, (a, b)
    assert np.allclose(np.cross(e1, e2), n, rtol=0, atol=1e-15)  # right-handed: e1 x e2 = n
    # the restatement and the Python wrapper give the same bits
    for got, ref, py in zip((n, e1, e2), M.frame(axis), nb.map_frame(axis)):
        assert got.tobytes() == ref.tobytes() == py.tobytes()
    # ... and nb_field_rings lays its points in this frame: q = 0 at c + R e1, q = n_phi / 4 at c + R e2
    c, R = np.array([0.25, -1.5, 3.0]), 2.5
    r = np.array([R])
    pts = np.zeros((8, 3), np.float32)
    assert L.nb_field_rings(_v3(c), _v3(axis), r.ctypes.data_as(DP), 1, 8, pts.ctypes.data) == 0
    assert np.array_equal(pts[0], (c + R * (1.0 * e1 + 0.0 * e2)).astype(np.float32))
    cq, sq = math.cos(2.0 * math.pi * 2 / 8), math.sin(2.0 * math.pi * 2 / 8)
    assert np.array_equal(pts[2], (c + R * (cq * e1 + sq * e2)).astype(np.float32))
    assert np.allclose(pts[2], c + R * e2, rtol=0, atol=1e-6)


def test_frames_worked_out_by_hand(nb):
    # the default line of sight y: e1 = x, e2 = y cross x = -z; face-on to disc_init's disc (z): e1 = x, e2 = y
    for axis, want in (((0, 1, 0), ((0, 1, 0), (1, 0, 0), (0, 0, -1))), ((0, 0, 1), ((0, 0, 1), (1, 0, 0), (0, 1, 0))),
                       ((0, -3, 0), ((0, -1, 0), (1, 0, 0), (0, 0, 1))), ((2, 0, 0), ((1, 0, 0), (0, 1, 0), (0, 0, 1)))):
        got = nb.map_frame(axis)
        for g, w in zip(got, want):
            assert np.array_equal(g, np.array(w, dtype=np.float64)), (axis, got)
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    for axis in ((0, 0, 0), (math.nan, 0, 1), (math.inf, 0, 0), (1e-200, 0, 0)):
        rc, out = _frame(L, axis)
        assert rc == _lib.NB_ERR_INVALID and all(np.all(v == 0) for v in out), axis
    assert L.nb_map_frame(None, None, None, None) == _lib.NB_ERR_INVALID


def test_edges(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    for lo, hi, cells in ((-1.0, 1.0, 7), (0.1, 0.7, 3), (-3.3, 12.9, 4096), (1e-9, 2e-9, 100), (-5.0, -4.0, 1)):
        e = nb.map_edges(lo, hi, cells)
        assert e.shape == (cells + 1,) and e[0] == lo and e[cells] == hi and np.all(np.diff(e) > 0)
        assert e.tobytes() == M.edges(lo, hi, cells).tobytes()
        d = (hi - lo) / cells
        assert all(e[i] == lo + i * d for i in range(cells))
    # dyadic: integer arithmetic
    assert np.array_equal(nb.map_edges(-2.0, 2.0, 256) * 64.0, np.arange(-128, 129))
    assert np.array_equal(nb.map_edges(0.0, 1.0, 1024) * 1024.0, np.arange(1025))
    assert np.array_equal(nb.map_edges(0.25, 0.75, 8) * 16.0, np.arange(4, 13))
    # refusals: a range too narrow to give ascending edges, bad bounds, bad cell numbers, a null pointer
    buf = np.full(8, 7.0)
    for lo, hi, cells in ((1.0, 1.0 + 4e-16, 4), (1.0, 1.0, 2), (2.0, 1.0, 2), (math.nan, 1.0, 2), (0.0, math.inf, 2),
                          (0.0, 1.0, 0), (0.0, 1.0, 4097)):
        assert L.nb_map_edges(lo, hi, cells, buf.ctypes.data_as(DP)) == _lib.NB_ERR_INVALID, (lo, hi, cells)
        assert np.all(buf == 7.0)
    assert L.nb_map_edges(0.0, 1.0, 2, None) == _lib.NB_ERR_INVALID
    with pytest.raises(nb.NBodyError):
        nb.map_edges(1.0, 1.0 + 4e-16, 4)


def _loop_map(state, width, height, extent, axis, center, velocity, depth):
    """The rule in a plain Python double loop over bodies and cells, Python floats (binary64) throughout."""
    n_hat, e1, e2 = ([float(x) for x in v] for v in M.frame(axis))
    xe = [float(x) for x in M.edges(extent[0], extent[1], width)]
    ye = [float(x) for x in M.edges(extent[2], extent[3], height)]
    counts = [[0] * width for _ in range(height)]
    planes = {k: [[0.0] * width for _ in range(height)] for k in M.PLANES}
    tally = dict(nonfinite=0, binned_count=0, outside_count=0, binned_mass=0.0, outside_mass=0.0, total_mass=0.0)
    dot = lambda p, q: (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]  # noqa: E731
    for row in state:
        vals = [float(x) for x in row]
        x, v, m = vals[0:3], vals[3:6], vals[9]
        if not all(math.isfinite(t) for t in x + v + [m]):
            tally["nonfinite"] += 1
            continue
        tally["total_mass"] += m
        d = [x[k] - center[k] for k in range(3)]
        u = [v[k] - velocity[k] for k in range(3)]
        a, b, h = dot(d, e1), dot(d, e2), dot(d, n_hat)
        cell = None
        if depth[0] <= h < depth[1]:
            for j in range(height):
                for i in range(width):
                    if xe[i] <= a < xe[i + 1] and ye[j] <= b < ye[j + 1]:
                        cell = (j, i)
        if cell is None:
            tally["outside_count"] += 1
            tally["outside_mass"] += m
            continue
        tally["binned_count"] += 1
        tally["binned_mass"] += m
        j, i = cell
        counts[j][i] += 1
        ua, ub, w = dot(u, e1), dot(u, e2), dot(u, n_hat)
        for name, t in zip(M.PLANES, (m, m * ua, m * ub, m * w, (m * w) * w, m * dot(u, u))):
            planes[name][j][i] += t
    return counts, planes, tally


@pytest.mark.parametrize("axis,depth", [((0, 1, 0), (-math.inf, math.inf)), ((1.0, 2.0, 3.0), (-0.4, 0.3))])
def test_restatement_against_a_plain_loop(axis, depth):
    rng = np.random.default_rng(12)
    state = np.zeros((50, 10), np.float32)
    state[:, 0:3] = rng.uniform(-1.0, 1.0, (50, 3))
    state[:, 3:6] = rng.normal(0.0, 0.3, (50, 3))
    state[:, 9] = rng.uniform(0.5, 2.0, 50)
    state[7, 1], state[19, 5], state[33, 9] = np.nan, np.inf, -np.inf
    state[3, 0:3] = (0.5, 0.0, 0.0)  # on edges when seen along y about (0.1, -0.2, 0.05) ... or not: no case excused
    extent, center, velocity = (-0.75, 0.5, -0.5, 0.75), (0.1, -0.2, 0.05), (0.01, 0.02, -0.03)
    W, H = 5, 3
    ref = M.map64(state, W, H, extent, axis=axis, center=center, velocity=velocity, depth=depth)
    counts, planes, tally = _loop_map(state, W, H, extent, axis, center, velocity, depth)
    assert ref["n"] == 50 and ref["nonfinite"] == tally["nonfinite"] == 3
    assert (ref["binned_count"], ref["outside_count"]) == (tally["binned_count"], tally["outside_count"])
    assert 0 < ref["binned_count"] < 47 and ref["binned_count"] + ref["outside_count"] + 3 == 50
    assert np.array_equal(ref["counts"], np.array(counts, dtype=np.uint32)) and ref["max_count"] == max(map(max, counts))
    for name in ("binned_mass", "outside_mass", "total_mass"):
        assert abs(ref[name] - tally[name]) <= 1e-14 * ref["scale"][name], name
    for name in M.PLANES:
        assert np.all(np.abs(ref[name] - np.array(planes[name])) <= 1e-14 * ref["scale"][name]), name
