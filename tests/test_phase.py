"""Phase maps at the C-ABI boundary, without a device: the entry points are exported, the Python mirrors have the
C layout, the table of quantity names round-trips, bad arguments are refused before any device is touched, and the
numpy restatement (tests/phase_ref.py) gives what can be worked out by hand."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from tests import phase_ref as P
from tests.helpers import ROOT

NAMES = ("nb_phase_map_sim", "nb_phase_map_runner", "nb_phase_quantity", "nb_phase_quantity_name")

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "nbody.h"
#define F(T, x) printf(#T "." #x " %zu %zu\n", offsetof(T, x), sizeof(((T *)0)->x));
#define S(T) printf(#T " %zu %zu\n", sizeof(T), _Alignof(T));
int main(void) {
    S(nb_phase_params) F(nb_phase_params, width) F(nb_phase_params, height) F(nb_phase_params, flags)
    F(nb_phase_params, reserved) F(nb_phase_params, x) F(nb_phase_params, y) F(nb_phase_params, q)
    F(nb_phase_params, reserved2) F(nb_phase_params, center) F(nb_phase_params, velocity) F(nb_phase_params, axis)
    F(nb_phase_params, x_edges) F(nb_phase_params, y_edges) F(nb_phase_params, values) F(nb_phase_params, step_num)
    S(nb_phase_stats) F(nb_phase_stats, step_num) F(nb_phase_stats, n) F(nb_phase_stats, nonfinite)
    F(nb_phase_stats, binned_count) F(nb_phase_stats, outside_count) F(nb_phase_stats, undefined_count)
    F(nb_phase_stats, binned_mass) F(nb_phase_stats, outside_mass) F(nb_phase_stats, mass)
    F(nb_phase_stats, center) F(nb_phase_stats, velocity) F(nb_phase_stats, n_hat) F(nb_phase_stats, e1)
    F(nb_phase_stats, e2) F(nb_phase_stats, width) F(nb_phase_stats, height) F(nb_phase_stats, flags)
    F(nb_phase_stats, max_count) F(nb_phase_stats, x) F(nb_phase_stats, y) F(nb_phase_stats, q)
    F(nb_phase_stats, reserved)
    printf("NB_PHASE_CENTER_COM %u 0\n", NB_PHASE_CENTER_COM);
    printf("NB_PHASE_WEIGHT %u 0\n", NB_PHASE_WEIGHT);
    printf("NB_PHASE_Q_COUNT %u 0\n", (unsigned)NB_PHASE_Q_COUNT);
    printf("NB_PHASE_Q_MASS %u 0\n", (unsigned)NB_PHASE_Q_MASS);
    printf("NB_PHASE_Q_VALUE %u 0\n", (unsigned)NB_PHASE_Q_VALUE);
    printf("NB_PHASE_ANY_STEP %d 0\n", NB_PHASE_ANY_STEP == 0xFFFFFFFFFFFFFFFFull);
    return 0;
}
"""

DP = C.POINTER(C.c_double)


@pytest.fixture(autouse=True)
def _the_restatement_names_the_librarys_quantities(nb):
    """The hand cases below speak of the restatement's quantities: they are the library's, name for name."""
    assert nb.phase_quantities() == P.QUANTITIES


def test_phase_entry_points_are_exported(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.ABI_SYMBOLS, name
    for name in ("PhaseMap", "PhaseStats", "phase_quantity", "phase_quantities", "phase_edges"):
        assert name in nb.__all__ and hasattr(nb, name)
    # one method, shared by the two owners of a state
    for cls in (nb.Simulator, nb.OfflineHeadless):
        assert cls.phase_map is nb._Passes.phase_map and cls.distribution is nb._Passes.distribution


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
    for S, size in ((_lib.nb_phase_params, 136), (_lib.nb_phase_stats, 224)):
        name = S.__name__
        assert info[name] == (C.sizeof(S), C.alignment(S)) and C.sizeof(S) == size, name
        for f, _ in S._fields_:
            assert info[f"{name}.{f}"] == (getattr(S, f).offset, getattr(S, f).size), (name, f)
        assert len(S._fields_) == sum(1 for k in info if k.startswith(name + "."))
    assert info["NB_PHASE_CENTER_COM"][0] == _lib.NB_PHASE_CENTER_COM == 1
    assert info["NB_PHASE_WEIGHT"][0] == _lib.NB_PHASE_WEIGHT == 2
    assert info["NB_PHASE_Q_COUNT"][0] == _lib.NB_PHASE_Q_COUNT == 18
    assert info["NB_PHASE_Q_MASS"][0] == _lib.NB_PHASE_Q_MASS and info["NB_PHASE_Q_VALUE"][0] == _lib.NB_PHASE_Q_VALUE
    assert info["NB_PHASE_ANY_STEP"][0] == 1 and _lib.NB_PHASE_ANY_STEP == 2 ** 64 - 1


def test_the_name_table_round_trips(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    names = nb.phase_quantities()
    assert names == P.QUANTITIES and len(set(names)) == 18
    for q, name in enumerate(names):
        assert nb.phase_quantity(name) == q and L.nb_phase_quantity_name(q) == name.encode()
    assert nb.phase_quantity("mass") == _lib.NB_PHASE_Q_MASS and nb.phase_quantity("value") == _lib.NB_PHASE_Q_VALUE
    assert nb.phase_quantity("R") != nb.phase_quantity("r") and nb.phase_quantity("u_R") != nb.phase_quantity("u_r")
    assert L.nb_phase_quantity_name(18) is None and L.nb_phase_quantity_name(0xFFFFFFFF) is None
    out = C.c_uint32(77)
    for name in (b"phi", b"", b"A", b"u_Phi", b"value "):
        assert L.nb_phase_quantity(name, C.byref(out)) == _lib.NB_ERR_INVALID and out.value == 77, name
    assert L.nb_phase_quantity(None, C.byref(out)) == _lib.NB_ERR_INVALID
    assert L.nb_phase_quantity(b"a", None) == _lib.NB_ERR_INVALID
    with pytest.raises(nb.NBodyError):
        nb.phase_quantity("azimuth")


def good_params(_lib, xe=None, ye=None, values=None, **change):
    p = _lib.nb_phase_params()
    xe = np.linspace(-1.0, 1.0, 17) if xe is None else np.asarray(xe, dtype=np.float64)
    ye = np.linspace(-2.0, 2.0, 9) if ye is None else np.asarray(ye, dtype=np.float64)
    p.width, p.height, p.flags = len(xe) - 1, len(ye) - 1, _lib.NB_PHASE_WEIGHT
    p.x, p.y, p.q = 0, 7, 12
    p.x_edges, p.y_edges = xe.ctypes.data_as(DP), ye.ctypes.data_as(DP)
    p._keep = (xe, ye, values)
    if values is not None:
        p.values = values.ctypes.data_as(DP)
    p.step_num = _lib.NB_PHASE_ANY_STEP
    vals = dict(center=(0, 0, 0), velocity=(0, 0, 0), axis=(0, 1, 0))
    for k, v in change.items():
        if k in vals:
            vals[k] = v
        elif k in ("x_edges", "y_edges", "values"):
            setattr(p, k, DP())  # a null pointer
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
    counts = np.full(4096, 7, np.uint32)
    planes = np.full(3 * 4096, 7.0)
    st = _lib.nb_phase_stats()
    V = _lib.NB_PHASE_Q_VALUE
    for call, who in ((L.nb_phase_map_sim, b"simulator"), (L.nb_phase_map_runner, b"runner")):
        def bad(word, p):
            assert call(None, C.byref(p) if p is not None else None, counts.ctypes.data, planes.ctypes.data,
                        C.byref(st)) == INV, word
            assert word in L.nb_last_error(), (word, L.nb_last_error())

        bad(b"null " + who, good_params(_lib))
        bad(b"null " + who, good_params(_lib, xe=[-inf, 0.0, 1.0, inf], ye=[-inf, inf]))
        bad(b"null " + who, good_params(_lib, flags=_lib.NB_PHASE_CENTER_COM, center=(nan, 0, 0)))
        bad(b"null " + who, good_params(_lib, flags=0, q=V))  # q is not summed: it needs no array
        bad(b"null " + who, good_params(_lib, x=V, values=np.zeros(4)))
        bad(b"params", None)
        bad(b"x_edges", good_params(_lib, x_edges=None))
        bad(b"y_edges", good_params(_lib, y_edges=None))
        bad(b"side", good_params(_lib, xe=[0.0]))  # no cell
        bad(b"side", good_params(_lib, xe=np.arange(4098.0)))
        bad(b"side", good_params(_lib, ye=np.arange(4098.0)))
        bad(b"cells", good_params(_lib, xe=np.arange(4097.0), ye=np.arange(2049.0)))
        bad(b"flag", good_params(_lib, flags=4))
        bad(b"flag", good_params(_lib, flags=3 | 8))
        bad(b"reserved", good_params(_lib, reserved=1))
        bad(b"reserved", good_params(_lib, reserved2=1))
        for which in ("x", "y", "q"):
            bad(b"quantity", good_params(_lib, **{which: 18}))
            bad(b"quantity", good_params(_lib, **{which: 0xFFFFFFFF}))
        bad(b"quantity", good_params(_lib, flags=0, q=18))
        for axis in ((0, 0, 0), (nan, 1, 0), (0, inf, 0), (1e-200, 0, 0), (1e200, 1e200, 0)):
            bad(b"axis", good_params(_lib, axis=axis))
        bad(b"center", good_params(_lib, center=(0, nan, 0)))
        bad(b"center", good_params(_lib, velocity=(inf, 0, 0)))
        for e in ([0.0, 0.0, 1.0], [0.0, 2.0, 1.0], [1.0, 0.0], [0.0, nan, 1.0], [nan, 0.0, 1.0], [0.0, 1.0, nan],
                  [0.0, inf, inf], [-inf, -inf, 0.0], [0.0, inf, 2.0], [inf, 0.0], [0.0, -inf], [0.0, 1.0, -inf],
                  [-inf, 0.0, -inf], [inf, inf]):
            bad(b"x_edges", good_params(_lib, xe=e))
            bad(b"y_edges", good_params(_lib, ye=e))
        for which in ("x", "y", "q"):
            bad(b"values", good_params(_lib, **{which: V}))
    assert np.all(counts == 7) and np.all(planes == 7.0) and st.n == 0


def _state(rows):
    """float32[n, 10] from (position, velocity, mass) rows."""
    s = np.zeros((len(rows), 10), np.float32)
    for k, (x, v, m) in enumerate(rows):
        s[k, 0:3], s[k, 3:6], s[k, 9] = x, v, m
    return s


def _q(state, **kw):
    return P.quantities(state[:, 0:3].astype(np.float64), state[:, 3:6].astype(np.float64),
                        state[:, 9].astype(np.float64), **kw)


def test_a_circular_and_a_radial_orbit():
    # the frame about z: e1 = x, e2 = y.  A body at (3, 4, 2) moving along the tangent (-4, 3, 0) / 5 * 2.5:
    # a circular orbit about the axis, whatever its height
    s = _state([((3.0, 4.0, 2.0), (-2.0, 1.5, 0.0), 1.0),
                ((3.0, 4.0, 0.0), (1.5, 2.0, 0.0), 2.0),      # a radial orbit in the plane: u = 0.5 d
                ((0.0, 3.0, 4.0), (0.0, -0.75, -1.0), 1.0)])  # a radial orbit towards the centre: u = -0.25 d
    q = _q(s, axis=(0.0, 0.0, 1.0))
    assert q["a"][0] == 3.0 and q["b"][0] == 4.0 and q["h"][0] == 2.0 and q["R"][0] == 5.0
    assert q["u_R"][0] == 0.0 and q["u_phi"][0] == 2.5 == q["speed"][0]
    assert q["j_z"][0] == 12.5 and q["w"][0] == 0.0 and q["e_kin"][0] == 3.125
    assert q["u_t"][1] == 0.0 and q["u_r"][1] == 2.5 == q["u_R"][1] and q["u_phi"][1] == 0.0 and q["j"][1] == 0.0
    assert q["u_t"][2] == 0.0 and q["u_r"][2] == -1.25 and q["r"][2] == 5.0 and q["j"][2] == 0.0
    assert np.array_equal(q["mass"], [1.0, 2.0, 1.0])
    # a circular orbit has u_t == speed and u_r == 0
    assert q["u_r"][0] == 0.0 and q["u_t"][0] == 2.5
    # about a moving centre: the same body seen from (1, 1, 1) at velocity (-2, 1.5, 0) is at rest
    q = _q(s[:1], axis=(0.0, 0.0, 1.0), center=(1.0, 1.0, 1.0), velocity=(-2.0, 1.5, 0.0))
    assert q["a"][0] == 2.0 and q["b"][0] == 3.0 and q["h"][0] == 1.0 and q["speed"][0] == 0.0 and q["j"][0] == 0.0


def test_a_body_at_the_centre_is_undefined_for_the_angles_and_binned_for_the_rest():
    s = _state([((0.0, 0.0, 0.0), (1.0, 2.0, 2.0), 1.0),    # at the centre
                ((0.0, 0.0, 0.5), (1.0, 0.0, 0.0), 1.0),    # on the axis z: R = 0, r > 0
                ((0.25, 0.0, 0.0), (0.0, 1.0, 0.0), 4.0)])
    q = _q(s, axis=(0.0, 0.0, 1.0))
    assert np.isnan(q["u_phi"][0]) and np.isnan(q["u_R"][0]) and np.isnan(q["u_r"][0]) and np.isnan(q["u_t"][0])
    assert q["a"][0] == 0.0 and q["R"][0] == 0.0 and q["r"][0] == 0.0 and q["speed"][0] == 3.0 and q["j"][0] == 0.0
    assert np.isnan(q["u_phi"][1]) and q["u_r"][1] == 0.0 and q["u_t"][1] == 1.0
    e, full = np.array([-1.0, 0.0, 1.0]), np.array([-math.inf, math.inf])
    for x in ("u_phi", "u_r"):
        ref = P.phase64(s, x, "mass", e * 8.0, full, axis=(0.0, 0.0, 1.0))
        want = 1 if x == "u_r" else 2
        assert (ref["undefined_count"], ref["outside_count"], ref["binned_count"]) == (want, want, 3 - want), x
    ref = P.phase64(s, "a", "mass", e, full, axis=(0.0, 0.0, 1.0))
    assert (ref["undefined_count"], ref["outside_count"], ref["binned_count"]) == (0, 0, 3)
    assert np.array_equal(ref["counts"], [[0, 3]]) and ref["mass"][0, 1] == 6.0
    # a weight that is undefined puts the body outside; a NaN among the values does the same
    ref = P.phase64(s, "a", "mass", e, full, weight="u_phi", axis=(0.0, 0.0, 1.0))
    assert (ref["undefined_count"], ref["outside_count"], ref["binned_count"]) == (2, 2, 1)
    assert ref["m_q"][0, 1] == 4.0 and ref["m_q2"][0, 1] == 4.0 and ref["outside_mass"] == 2.0
    ref = P.phase64(s, "value", "mass", e, full, values=[0.5, math.nan, 7.0], axis=(0.0, 0.0, 1.0))
    assert (ref["undefined_count"], ref["outside_count"], ref["binned_count"]) == (1, 2, 1)
    assert ref["binned_count"] + ref["outside_count"] + ref["nonfinite"] == ref["n"]


def test_edges_are_lower_inclusive_and_upper_exclusive():
    e = np.array([-1.0, -0.5, 0.0, 0.25, 2.0])
    x = np.array([-1.0, -0.5, -0.0, 0.0, 0.25, 2.0, np.nextafter(2.0, 0.0), np.nextafter(-1.0, -2.0), math.nan,
                  math.inf, -math.inf, np.nextafter(0.25, 0.0)])
    assert np.array_equal(P.cell_of(e, x), [0, 1, 2, 2, 3, -1, 3, -1, -1, -1, -1, 2])
    # infinite outer edges take every finite value, and no infinite one: such a value is undefined
    e = np.array([-math.inf, 0.0, math.inf])
    assert np.array_equal(P.cell_of(e, x), [0, 0, 1, 1, 1, 1, 1, 0, -1, -1, 0, 1])
    s = _state([((v, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0) for v in (-3e38, -1.0, 0.0, 5.0, 3e38)])
    ref = P.phase64(s, "a", "b", e, [-math.inf, math.inf])
    assert np.array_equal(ref["counts"], [[2, 3]]) and ref["outside_count"] == 0
    # the largest binary32 speeds leave every quantity and term finite in binary64
    s = _state([((1.0, 0.0, 0.0), (3e38, 3e38, 3e38), 1.0), ((1.0, 0.0, 0.0), (1.0, 0.0, 0.0), 1.0)])
    ref = P.phase64(s, "a", "b", e, [-math.inf, math.inf], weight="e_kin")
    assert ref["binned_count"] == 2 and np.isfinite(ref["m_q2"]).all()


def test_phase_edges(nb):
    assert nb.phase_edges(-1.0, 1.0, 7).tobytes() == nb.map_edges(-1.0, 1.0, 7).tobytes()
    assert nb.phase_edges(0.01, 10.0, 64, log=True).tobytes() == nb.radial_edges(0.01, 10.0, 64, log=True).tobytes()
    e = nb.phase_edges(0.01, 10.0, 1024, log=True)
    assert e.shape == (1025,) and e[0] == 0.01 and e[-1] == 10.0 and np.all(np.diff(e) > 0)
    with pytest.raises(ValueError):
        nb.phase_edges(0.0, 1.0, 1024, log=True)
