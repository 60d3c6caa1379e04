"""nb_sim_knn's rule restated twice (tests/knn_ref.py): the vectorised and the per-body restatement agree with ==
on random states, the lattice (where the index rule decides), coincident bodies, k = 1, 2, 6, 64, c = k and
c = k + 1, and non-finite bodies; what the library refuses without a device; the Python result class."""
import ctypes as C

import numpy as np
import pytest

from tests import knn_ref as K


def _same(a: K.KnnRef, b: K.KnnRef):
    assert np.array_equal(a.r2, b.r2, equal_nan=True) and np.array_equal(a.kth, b.kth)
    assert np.array_equal(a.mass_in, b.mass_in) and np.array_equal(a.density, b.density)
    for f in ("n", "nonfinite", "counted", "degenerate", "short_of_k", "peak_density", "peak_index"):
        assert getattr(a, f) == getattr(b, f), f
    assert np.array_equal(a.sums, b.sums) and np.array_equal(a.sums_abs, b.sums_abs)


@pytest.mark.parametrize("k", [1, 2, 6, 64])
def test_restatements_agree_on_random_states(k):
    rng = np.random.default_rng(k)
    for n in (k, k + 1, k + 2, 130):  # c = k (short), c = k + 1, ...
        s = K.state_of(rng.normal(size=(n, 3)), k)
        a, b = K.knn_vectorised(*K.split(s), k), K.knn_loop(*K.split(s), k)
        _same(a, b)
        assert a.short_of_k == (n if n <= k else 0) and a.counted == n
        if n > k:
            assert np.all(a.kth != K.NONE) and np.all(a.kth != np.arange(n)) and a.peak_index != K.NONE
        else:
            assert np.all(np.isinf(a.r2)) and np.all(a.kth == K.NONE) and not a.sums.any() and a.peak_index == K.NONE


CASES = K.synthetic_cases(small=True)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c[0] for c in CASES])
def test_restatements_agree_on_synthetic_cases(idx):
    name, state, ks, _ = CASES[idx]
    for k in ks:
        a = K.knn_vectorised(*K.split(state), k)
        _same(a, K.knn_loop(*K.split(state), k))
        if name == "lattice8" and k == 6:  # an inner body's six nearest are its face neighbours: all tied at d2 = 1
            inner = 1 * 64 + 1 * 8 + 1
            assert a.r2[inner] == 1.0 and a.kth[inner] == inner + 64  # the largest index of the six
            m = state[:, 9].astype(np.float64)
            want = 0.0
            for j in (inner - 64, inner - 8, inner - 1, inner + 1, inner + 8):
                want += m[j]
            assert a.mass_in[inner] == want
        if name == "three_points":
            assert a.degenerate == (200 if k <= 39 else 160 if k <= 59 else 100)
            assert np.all(np.isinf(a.density[a.r2 == 0.0]))
        if name == "one_point":
            assert a.degenerate == 70 and not a.sums.any() and a.peak_index == K.NONE


def test_restatements_agree_with_nonfinite_bodies():
    rng = np.random.default_rng(11)
    s = K.inject_nonfinite(K.state_of(rng.normal(size=(90, 3)), 2), 25, 3)
    ok = K.counted_mask(*K.split(s))
    assert 60 <= ok.sum() < 90
    for k in (1, 6, 64, int(ok.sum()), int(ok.sum()) - 1):
        a = K.knn_vectorised(*K.split(s), k)
        _same(a, K.knn_loop(*K.split(s), k))
        assert np.all(np.isnan(a.r2[~ok])) and np.all(a.kth[~ok] == K.NONE) and not a.density[~ok].any()
        assert a.nonfinite == 90 - ok.sum() and np.all(ok[a.kth[a.kth != K.NONE]])


def test_the_sphere_constant():
    import math
    assert K.SPHERE.hex() == "0x1.0c152382d7366p+2" and abs(K.SPHERE - 4.0 * math.pi / 3.0) < 1e-15


def test_refusals_without_a_device(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    assert _lib.NB_KNN_SPHERE == K.SPHERE and nb.KNN_NONE == K.NONE == _lib.NB_KNN_NONE and _lib.NB_KNN_MAX_K == K.MAX_K
    fake = C.c_void_p(1)  # never dereferenced: the parameters are checked first

    def call(fn, handle, **kw):
        p = _lib.nb_knn_params()
        p.k = 6
        for key, v in kw.items():
            setattr(p, key, v)
        r2 = np.full(4, 7.0)
        rc = fn(handle, C.byref(p), r2.ctypes.data, None, None, None, None)
        assert np.all(r2 == 7.0)
        return rc

    for fn in (L.nb_sim_knn, L.nb_runner_knn):
        for bad in ({"k": 0}, {"k": 65}, {"k": 0xFFFFFFFF}, {"flags": 1}, {"reserved": 1}):
            assert call(fn, fake, **bad) == _lib.NB_ERR_INVALID and L.nb_last_error()
        assert fn(fake, None, None, None, None, None, None) == _lib.NB_ERR_INVALID and b"null params" in L.nb_last_error()
        assert call(fn, None) == _lib.NB_ERR_INVALID


def test_result_class(nb):
    z3 = np.zeros(3)
    st = nb.KnnStats(3, 4, 0, 4, 4, 0, 0.0, z3, z3, 0.0, 0.0, nb.KNN_NONE)
    d = nb.KnnDensity(6, np.array([0.0, 4.0, np.inf, np.nan]), None, None, None, st)
    assert np.all(np.isnan(d.center)) and np.all(np.isnan(d.center_velocity)) and d.kth is None
    assert np.array_equal(d.r_k, [0.0, 2.0, np.inf, np.nan], equal_nan=True) and d.peak_index == nb.KNN_NONE
    st = nb.KnnStats(3, 4, 0, 4, 0, 0, 2.0, np.array([1.0, -2.0, 4.0]), np.array([0.0, 6.0, 1.0]), 5.0, 1.5, 2)
    d = nb.KnnDensity(6, None, None, None, None, st)
    assert np.array_equal(d.center, [0.5, -1.0, 2.0]) and np.array_equal(d.center_velocity, [0.0, 3.0, 0.5])
    assert d.r_k is None and (d.peak_index, d.peak_density) == (2, 1.5)
