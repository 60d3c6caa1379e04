"""The group shapes without a device: nb_shape_eigen (csrc/nb_shape.hpp, through the C ABI) against the numpy
restatement of the same Jacobi (tests/shape_ref.py), bit for bit, and against numpy.linalg.eigh; the rule's hand
cases on the restatement; that every status occurs in the named cases and that no case the GPU tests use has a
marginal decision; the layouts and the refusals that need no device."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import shape_ref as S
from tests.helpers import ROOT

DP = C.POINTER(C.c_double)


def _eigen(L, t):
    t = np.ascontiguousarray(t, np.float64)
    lam, axes = np.zeros(3), np.zeros(9)
    assert L.nb_shape_eigen(t.ctypes.data_as(DP), lam.ctypes.data_as(DP), axes.ctypes.data_as(DP)) == 0
    return lam, axes


def _pack(T):
    return np.array([T[0, 0], T[0, 1], T[0, 2], T[1, 1], T[1, 2], T[2, 2]])


def test_eigen_solver_is_the_restatement_and_reproduces_eigh(nb):
    """Bit for bit the restatement's Jacobi; on 1,000 random symmetric positive matrices over twelve decades the
    eigenvalues of numpy.linalg.eigh within 1e-13 lambda_1, |E^T Lambda E - T| <= 1e-13 lambda_1 (axes are the rows
    of E), E orthonormal to 1e-14."""
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(2024)
    for i in range(1000):
        a = rng.normal(size=(3, 3))
        T = (a @ a.T) * 10.0 ** rng.uniform(-6, 6)
        if i % 10 == 0:  # nearly degenerate pairs too
            T = T + np.eye(3) * np.trace(T) * 1e3
        T = (T + T.T) / 2
        lam, axes = _eigen(L, _pack(T))
        want_lam, want_axes = S.jacobi(_pack(T))
        assert lam.tobytes() == want_lam.tobytes() and axes.tobytes() == want_axes.tobytes(), i
        E = axes.reshape(3, 3)
        assert lam[0] >= lam[1] >= lam[2] > 0
        assert np.abs(np.linalg.eigvalsh(T)[::-1] - lam).max() <= 1e-13 * lam[0]
        assert np.abs(E.T @ np.diag(lam) @ E - T).max() <= 1e-13 * lam[0]
        assert np.abs(E @ E.T - np.eye(3)).max() <= 1e-14
        for k in range(3):  # the sign: the component of largest magnitude is positive
            assert E[k, np.argmax(np.abs(E[k]))] > 0


def test_eigen_solver_edge_cases(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    lam, axes = _eigen(L, [3.0, 0, 0, 3.0, 0, 5.0])  # diagonal with a tie: by value, then by index
    assert lam.tolist() == [5.0, 3.0, 3.0] and axes.tolist() == [0, 0, 1, 1, 0, 0, 0, 1, 0]
    lam, axes = _eigen(L, np.zeros(6))
    assert lam.tolist() == [0.0, 0.0, 0.0] and axes.tolist() == np.eye(3).ravel().tolist()
    lam, axes = _eigen(L, [math.nan, 0, 0, 1.0, 0, 2.0])  # a NaN compares false: it keeps its place, the rest sort
    assert math.isnan(lam[0]) and lam[1:].tolist() == [2.0, 1.0]
    t = np.zeros(6)
    lam, axes = np.zeros(3), np.zeros(9)
    assert L.nb_shape_eigen(None, lam.ctypes.data_as(DP), axes.ctypes.data_as(DP)) == _lib.NB_ERR_INVALID
    assert L.nb_shape_eigen(t.ctypes.data_as(DP), None, axes.ctypes.data_as(DP)) == _lib.NB_ERR_INVALID
    assert L.nb_shape_eigen(t.ctypes.data_as(DP), lam.ctypes.data_as(DP), None) == _lib.NB_ERR_INVALID


def test_six_masses_on_the_axes():
    state, gof, m, kw = S.case("six")
    row = S.shape_ref(state, gof, m, **kw)["rows"][0]
    assert row["status"] == S.CONVERGED and row["iterations"] == 1 and row["selected"] == 6
    assert row["q"] == 1.25 / 2.0 and row["s"] == 0.5 / 2.0
    assert np.abs(row["axes"] - np.eye(3).ravel()).max() <= 1e-15
    assert row["lambda"].tolist() == [8.0, 3.125, 0.5]


def test_a_rotated_copy_has_the_same_ratios_and_the_rotated_axes():
    """The rotated coordinates are rounded to binary32 (2^-24 relative), which moves the tensor by a few 2^-24 of
    lambda_1 and the axes by that over the relative eigenvalue gap (>= 0.3 here): 1e-6 holds both."""
    state, gof, m, kw = S.case("six")
    rot = S.rotation(np.random.default_rng(5))
    turned = state.copy()
    turned[:, 0:3] = state[:, 0:3].astype(np.float64) @ rot.T
    row = S.shape_ref(turned, gof, m, **kw)["rows"][0]
    assert abs(row["q"] - 0.625) <= 1e-6 and abs(row["s"] - 0.25) <= 1e-6
    E = row["axes"].reshape(3, 3)
    for k in range(3):  # axis k is the image of the unit vector k, up to the sign convention
        assert abs(abs(E[k] @ rot[:, k]) - 1.0) <= 1e-6
        assert E[k, np.argmax(np.abs(E[k]))] > 0


def test_rigid_rotation_has_j_equal_to_inertia_times_omega():
    """Coordinates in eighths and omega in quarters: v = omega x x is exact in binary32, so J = (tr T) omega - T omega
    up to the rounding of the sums, 1e-13 of their sum of |term|."""
    rng = np.random.default_rng(6)
    n = 200
    omega = np.array([0.5, 0.25, 1.0])
    state = np.zeros((n, 10), np.float32)
    state[:, 0:3] = rng.integers(-16, 17, (n, 3)) / 8.0
    state[:, 3:6] = np.cross(omega, state[:, 0:3].astype(np.float64))
    state[:, 9] = rng.integers(1, 9, n) / 4.0
    ref = S.shape_ref(state, np.zeros(n, np.uint32), 1, centers=np.zeros((1, 3)), velocities=np.zeros((1, 3)))
    row = ref["rows"][0]
    t = row["t"]
    T = np.array([[t[0], t[1], t[2]], [t[1], t[3], t[4]], [t[2], t[4], t[5]]])
    want = np.trace(T) * omega - T @ omega
    assert row["status"] == S.CONVERGED and row["selected"] == n
    assert np.abs(row["j"] - want).max() <= 1e-13 * ref["scale"][0][19:22].max()


def test_four_coplanar_bodies_are_degenerate():
    state, gof, m, kw = S.case("coplanar")
    row = S.shape_ref(state, gof, m, **kw)["rows"][0]
    assert row["status"] == S.DEGENERATE and row["selected"] == 4 and row["lambda"][2] == 0.0
    assert math.isnan(row["q"]) and math.isnan(row["s"])


def test_every_status_occurs_in_the_named_cases():
    seen = set()
    for name in S.GPU_CASES:
        seen |= set(S.reference(name)["rows"]["status"].tolist())
    assert seen == {S.CONVERGED, S.UNCONVERGED, S.DEGENERATE, S.EMPTY}
    mixed = S.reference("mixed")["rows"]
    assert mixed["status"].tolist() == [S.CONVERGED, S.CONVERGED, S.CONVERGED, S.DEGENERATE, S.CONVERGED, S.EMPTY,
                                        S.UNCONVERGED]
    assert mixed["iterations"][0] == 2 and mixed["iterations"][2] >= 10 and mixed["iterations"][4] == 1
    assert np.isinf(mixed["radius"][4])


@pytest.mark.parametrize("name", S.GPU_CASES)
def test_no_case_of_the_gpu_tests_has_a_marginal_decision(name):
    assert not S.reference(name)["marginal"].any()


def test_the_reference_masks_and_orders_as_the_rule_says():
    """A member that is not selected adds +0 at its own position: dropping it from the list instead moves the later
    members to other runs and changes the bits of a sum, which is what masking is there to avoid."""
    rng = np.random.default_rng(9)
    terms = rng.normal(size=(200, 2))
    keep = np.ones(200, bool)
    keep[3] = False
    masked = S.run_sums(np.where(keep[:, None], terms, 0.0))
    assert masked.tobytes() != S.run_sums(terms[keep]).tobytes()
    assert np.allclose(masked, terms[keep].sum(axis=0), rtol=0, atol=1e-12)


def test_layouts(nb):
    from wgpu_n_body_amd import _lib
    p, g, st = _lib.nb_shape_params, _lib.nb_shape_group, _lib.nb_shape_stats
    assert C.sizeof(p) == 40 and C.sizeof(g) == 360 and C.sizeof(st) == 80
    assert [getattr(p, f).offset for f in ("flags", "min_members", "max_iter", "reserved32", "tol", "step_num",
                                           "reserved")] == [0, 4, 8, 12, 16, 24, 32]
    names = ("count", "selected", "iterations", "status", "radius", "center", "velocity", "mass", "md", "mu", "t", "uu",
             "j", "lambda", "axes", "q", "s")
    assert tuple(n for n, _ in g._fields_) == names == _lib.SHAPE_GROUP_DTYPE.names
    assert [getattr(g, k).offset for k in names] == [_lib.SHAPE_GROUP_DTYPE.fields[k][1] for k in names] == \
        [0, 4, 8, 12, 16, 24, 48, 72, 80, 104, 128, 176, 224, 248, 272, 344, 352]
    assert _lib.SHAPE_GROUP_DTYPE == S.ROW_DTYPE
    assert [getattr(st, f).offset for f in ("step_num", "n", "rows", "members", "nonfinite_members", "converged",
                                            "unconverged", "degenerate", "empty", "rounds_max", "reserved")] == \
        [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 76]
    assert (nb.SHAPE_CONVERGED, nb.SHAPE_UNCONVERGED, nb.SHAPE_DEGENERATE, nb.SHAPE_EMPTY) == \
        (S.CONVERGED, S.UNCONVERGED, S.DEGENERATE, S.EMPTY)
    hdr = open(os.path.join(ROOT, "include", "nbody.h")).read()
    for word, value in (("CONVERGED", 1), ("UNCONVERGED", 2), ("DEGENERATE", 4), ("EMPTY", 8), ("MAX_ITER", 64)):
        assert f"#define NB_SHAPE_{word} {value}u" in hdr
    assert "sizeof(nb_shape_params) == 40 && sizeof(nb_shape_group) == 360 && sizeof(nb_shape_stats) == 80" in hdr
    for sym in ("nb_sim_group_shapes", "nb_runner_group_shapes", "nb_shape_eigen"):
        assert sym in _lib.ABI_SYMBOLS and hasattr(_lib.lib(), sym)


def good_params(_lib, **kw):
    p = _lib.nb_shape_params()
    p.flags, p.min_members, p.max_iter, p.tol, p.step_num = 0, 10, 32, 1e-3, 0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_bad_parameters_are_invalid_without_a_device(nb):
    """The parameters are checked before the handle is looked at: a null handle with good parameters is the one
    refusal that names the handle.  The outputs stay as they were."""
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    gof = np.zeros(8, np.uint32)
    rows = np.zeros(2, _lib.SHAPE_GROUP_DTYPE)
    sel = np.full(8, 7, np.uint32)
    st = _lib.nb_shape_stats()
    for call, who in ((L.nb_sim_group_shapes, b"simulator"), (L.nb_runner_group_shapes, b"runner")):
        def bad(word, p):
            assert call(None, C.byref(p) if p is not None else None, gof.ctypes.data, 1, None, None, None,
                        rows.ctypes.data, sel.ctypes.data, C.byref(st)) == _lib.NB_ERR_INVALID, word
            assert word in L.nb_last_error(), (word, L.nb_last_error())
        bad(b"null params", None)
        bad(b"min_members", good_params(_lib, min_members=0))
        for it in (0, 65, 1 << 31):
            bad(b"max_iter", good_params(_lib, max_iter=it))
        for tol in (0.0, -1e-3, math.nan, math.inf):
            bad(b"tol", good_params(_lib, tol=tol))
        bad(b"flag", good_params(_lib, flags=2))
        bad(b"reserved", good_params(_lib, reserved32=1))
        bad(b"reserved", good_params(_lib, reserved=1 << 40))
        bad(b"null " + who, good_params(_lib))
        bad(b"null " + who, good_params(_lib, flags=_lib.NB_SHAPE_REDUCED, max_iter=64, min_members=1))
    assert np.all(sel == 7) and not rows.tobytes().strip(b"\0") and bytes(st) == bytes(_lib.nb_shape_stats())


def test_the_wrapper_resolves_the_radius_without_a_device(nb):
    rms = np.array([0.5, 2.0, 1.0])
    assert nb._shape_radius(None, 3, rms) is None
    assert nb._shape_radius(1.5, 3, rms).tolist() == [1.5, 1.5, 1.5]
    assert nb._shape_radius([1.0, 2.0, np.inf], 3, rms).tolist() == [1.0, 2.0, np.inf]
    assert nb._shape_radius(("rms", 2.0), 3, rms).tolist() == [1.0, 4.0, 2.0]
    with pytest.raises(ValueError):
        nb._shape_radius([1.0, 2.0], 3, rms)
    with pytest.raises(ValueError):
        nb._shape_radius(("rms", 2.0), 3, None)
