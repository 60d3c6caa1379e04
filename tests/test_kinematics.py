"""nb_local_kinematics_sim's rule restated twice (tests/kinematics_ref.py): the vectorised and the per-body
restatement agree with == over knn_ref's small synthetic cases; the struct sizes; what the library refuses without a
device; nb_local_kinematics_derive against numpy -- bit for bit but for the gradient, which is held to
c kappa(D) 2^-53 ||G|| of numpy.linalg.solve; the singular rule; and the two states with a known answer, on the
restatement alone."""
import ctypes as C

import numpy as np
import pytest

from tests import kinematics_ref as R
from tests import knn_ref as K

CASES = K.synthetic_cases(small=True)


def _same(a: R.KinRef, b: R.KinRef):
    for f in ("moments", "grads", "s0_self", "s0_noself"):
        assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), f
    assert (a.counted, a.degenerate, a.short_of_k) == (b.counted, b.degenerate, b.short_of_k)
    assert np.array_equal(a.knn.r2, b.knn.r2, equal_nan=True) and np.array_equal(a.knn.kth, b.knn.kth)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c[0] for c in CASES])
def test_restatements_agree_on_synthetic_cases(idx):
    name, state, ks, _ = CASES[idx]
    for j, k in enumerate(ks):
        include_self = j % 2 == 0
        a = R.kin_vectorised(*K.split(state), k, include_self)
        _same(a, R.kin_loop(*K.split(state), k, include_self))
        assert np.array_equal(a.moments[:, 0], a.s0_self if include_self else a.s0_noself)
        if name == "lattice8" and k == 6:  # an inner body: its six face neighbours, D = 2 m on the diagonal
            inner = 1 * 64 + 1 * 8 + 1
            m = state[:, 9].astype(np.float64)
            order = (inner - 64, inner - 8, inner - 1, inner + 1, inner + 8, inner + 64)  # d2 = 1 each: by index
            want = m[inner]
            for j2 in order:
                want += m[j2]
            assert a.s0_self[inner] == want
            assert a.grads[inner, 0] == m[inner - 64] + m[inner + 64] and not a.grads[inner, [1, 2, 4]].any()
        if name == "one_point":
            assert a.degenerate == 70 and not a.grads[:, 0:6].any()


def test_restatements_agree_short_of_k_and_with_nonfinite_bodies():
    rng = np.random.default_rng(11)
    s = K.inject_nonfinite(K.state_of(rng.normal(size=(90, 3)), 2), 25, 3)
    ok = K.counted_mask(*K.split(s))
    c = int(ok.sum())
    for k in (1, 6, 64, c, c - 1):
        a = R.kin_vectorised(*K.split(s), k)
        _same(a, R.kin_loop(*K.split(s), k))
        assert np.all(np.isnan(a.moments[~ok])) and np.all(np.isnan(a.grads[~ok]))
        if c <= k:
            assert not a.moments[ok].any() and not a.grads[ok].any() and a.short_of_k == c
        else:
            assert np.all(a.moments[ok, 0] > 0.0) and a.short_of_k == 0


def test_struct_sizes_and_constants(nb):
    from wgpu_n_body_amd import _lib
    assert C.sizeof(_lib.nb_kin_params) == 16 and C.sizeof(_lib.nb_kin_stats) == 56
    assert _lib.KIN_DERIVED_DTYPE.itemsize == 256
    assert (_lib.NB_KIN_MOMENTS, _lib.NB_KIN_GRADS, _lib.NB_KIN_SELF) == (R.MOMENTS, R.GRADS, 1)
    assert (nb.KIN_SHORT, nb.KIN_NOT_COUNTED, nb.KIN_DEGENERATE, nb.KIN_SINGULAR) == (R.SHORT, R.NOT_COUNTED,
                                                                                     R.DEGENERATE, R.SINGULAR)


def test_refusals_without_a_device(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    fake = C.c_void_p(1)  # never dereferenced: the parameters are checked first

    def call(fn, handle, **kw):
        p = _lib.nb_kin_params()
        p.k = 6
        for key, v in kw.items():
            setattr(p, key, v)
        mom = np.full(40, 7.0)
        rc = fn(handle, C.byref(p), mom.ctypes.data, None, None, None, None, None, None)
        assert np.all(mom == 7.0)
        return rc

    for fn in (L.nb_local_kinematics_sim, L.nb_local_kinematics_runner):
        for bad in ({"k": 0}, {"k": 65}, {"k": 0xFFFFFFFF}, {"flags": 2}, {"flags": 3}, {"reserved": 1}):
            assert call(fn, fake, **bad) == _lib.NB_ERR_INVALID and L.nb_last_error()
        assert fn(fake, None, None, None, None, None, None, None, None) == _lib.NB_ERR_INVALID
        assert b"null params" in L.nb_last_error()
        assert call(fn, None) == _lib.NB_ERR_INVALID
    out = np.zeros(2, _lib.KIN_DERIVED_DTYPE)
    ok = np.zeros(20)
    derive = L.nb_local_kinematics_derive
    assert derive(None, None, ok.ctypes.data, None, None, 2, out.ctypes.data) == _lib.NB_ERR_INVALID
    assert derive(ok.ctypes.data, None, None, None, None, 2, out.ctypes.data) == _lib.NB_ERR_INVALID
    assert derive(ok.ctypes.data, None, ok.ctypes.data, None, None, 2, None) == _lib.NB_ERR_INVALID
    assert derive(None, None, None, None, None, 0, None) == 0


def _derive_states():
    """(state, k): round and flattened neighbourhoods, few and many neighbours."""
    out = []
    for seed, (n, k, squash) in enumerate([(300, 6, 1.0), (300, 32, 1.0), (300, 6, 1e-3), (300, 32, 1e-4),
                                           (300, 12, 1e-2), (400, 64, 1.0)]):
        rng = np.random.default_rng(seed)
        out.append((K.state_of(rng.normal(size=(n, 3)) * [1.0, 1.0, squash], seed), k))
    s = K.inject_nonfinite(K.state_of(np.random.default_rng(9).normal(size=(90, 3)), 9), 20, 4)
    out.append((s, 6))
    out.append((s, 80))  # short of k
    return out


def test_derive_against_numpy(nb):
    """Everything but the gradient equals the restatement bit for bit (the gradient too: one formula, two
    languages); the gradient against numpy.linalg.solve within c kappa(D) 2^-53 ||G||.  c = 2.6 is the largest
    ratio over these matrices (kappa up to 5e8; the largest ratio is on the round k = 64 set, whose kappa stays below
    13, where a few roundings of nine entries are all there is); the bound has four times that."""
    worst = 0.0
    for state, k in _derive_states():
        a = R.kin_loop(*K.split(state), k) if k == 80 else R.kin_vectorised(*K.split(state), k)
        vel = state[:, 3:6]
        want = R.derive_ref(a.moments, a.grads, a.knn.r2, a.knn.density, vel)
        got = nb.kinematics_derive(a.moments, a.grads, a.knn.r2, a.knn.density, vel)
        for f, w in want.items():
            assert np.array_equal(np.asarray(got[f]).reshape(w.shape), w, equal_nan=True), f
        bare = nb.kinematics_derive(a.moments, None, a.knn.r2, None, None)
        assert np.array_equal(bare["sigma"], got["sigma"], equal_nan=True)
        assert np.all(np.isnan(bare["gradient"])) and np.all(np.isnan(bare["phase_space_density"]))
        assert np.all(np.isnan(bare["mean_velocity"])) and not np.any(bare["status"] & R.SINGULAR)
        live = (want["status"] & (R.SINGULAR | R.SHORT | R.NOT_COUNTED)) == 0
        if live.any():
            G, bound, kappa = R.solve_bound(a.grads[live], R.SOLVE_C)
            err = np.linalg.norm(want["gradient"][live] - G, axis=1)
            worst = max(worst, float((err / bound).max()) * R.SOLVE_C)
            assert np.all(err <= bound), (k, float((err / bound).max()))
    print("derive: the largest measured c", worst)


def _rows(pts, k_mass=1.0):
    """moments and grads of one body at the origin at rest with the neighbours `pts` (u = x: G is the identity
    wherever it exists), r2 > 0."""
    pts = np.asarray(pts, np.float64)
    mom, gr = np.zeros((1, 10)), np.zeros((1, 15))
    for x in pts:
        mom[0, 0] += k_mass
        mom[0, 1:4] += k_mass * x
        for f, (a, b) in enumerate(R.PAIRS):
            mom[0, 4 + f] += (k_mass * x[a]) * x[b]
            gr[0, f] += (k_mass * x[a]) * x[b]
        for a in range(3):
            for b in range(3):
                gr[0, 6 + 3 * a + b] += (k_mass * x[a]) * x[b]
    return mom, gr


def test_the_singular_rule(nb):
    lattice = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    coplanar = [(1, 2, 1), (-3, 1, -3), (2, -1, 2), (5, 0, 5), (-1, -4, -1), (0, 7, 0)]  # the plane x = z
    collinear = [(1, 2, 3), (2, 4, 6), (-3, -6, -9), (0.5, 1, 1.5), (4, 8, 12), (-1, -2, -3)]
    coincident = [(0, 0, 0)] * 6
    for pts, singular, r2 in ((lattice, False, 1.0), (coplanar, True, 6.0), (collinear, True, 14.0),
                              (coincident, True, 0.0)):
        mom, gr = _rows(pts)
        d = nb.kinematics_derive(mom, gr, [r2], [1.0], None)
        assert bool(d["status"][0] & R.SINGULAR) == singular, pts
        assert bool(d["status"][0] & R.DEGENERATE) == (r2 == 0.0)
        if singular:
            assert np.all(np.isnan(d["gradient"])) and np.isnan(d["divergence"][0]) and np.isnan(d["shear"][0])
            assert d["det"][0] == 0.0  # exactly: the inputs are small integers
        else:
            assert np.array_equal(d["gradient"][0], np.eye(3).ravel()) and d["divergence"][0] == 3.0
            assert not d["vorticity"][0].any() and d["shear"][0] == 0.0 and d["det"][0] == 8.0
    # the ratio det / (D_xx D_yy D_zz) against 2^-30, the ratio in exact rational arithmetic: the plane x = z with
    # two bodies lifted off it by t (the ratio falls as t^2); an axis-aligned thin slab has ratio 1 and is kept
    from fractions import Fraction
    seen = set()
    for e in (10, 13, 14, 15, 16, 17, 20):
        t = 2.0 ** -e
        near = [(1, 2, 1 + t), (-3, 1, -3 - t)] + coplanar[2:]
        mom, gr = _rows(near)
        d = nb.kinematics_derive(mom, gr, [1.0], None, None)
        D = [[sum(Fraction(p[a]) * Fraction(p[b]) for p in near) for b in range(3)] for a in range(3)]
        det = (D[0][0] * (D[1][1] * D[2][2] - D[1][2] * D[2][1]) - D[0][1] * (D[1][0] * D[2][2] - D[1][2] * D[2][0])
               + D[0][2] * (D[1][0] * D[2][1] - D[1][1] * D[2][0]))
        ratio = det / (D[0][0] * D[1][1] * D[2][2])
        assert 0 <= ratio <= 1 and abs(float(ratio) / 2.0 ** -30 - 1.0) > 0.01  # (not a borderline case)
        singular = not ratio > Fraction(1, 2 ** 30)
        seen.add(singular)
        assert bool(d["status"][0] & R.SINGULAR) == singular, (e, float(ratio))
    assert seen == {True, False}
    mom, gr = _rows([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 2.0 ** -20), (0, 0, -2.0 ** -20)])
    assert nb.kinematics_derive(mom, gr, [1.0], None, None)["status"][0] == 0


def test_exact_linear_flow_on_the_restatement(nb):
    state, A = R.linear_flow_state()
    a = R.kin_vectorised(*K.split(state), 32)
    d = nb.kinematics_derive(a.moments, a.grads, a.knn.r2, a.knn.density, state[:, 3:6])
    R.check_linear_flow(a.moments, a.grads, A, d)


def test_a_cold_clump_on_the_restatement(nb):
    state, clump = R.clump_state()
    a = R.kin_vectorised(*K.split(state), 32)
    d = nb.kinematics_derive(a.moments, None, a.knn.r2, a.knn.density, state[:, 3:6])
    R.check_clump(d["sigma"], d["phase_space_density"], a.knn.density, clump)


def test_result_class(nb):
    from wgpu_n_body_amd import _lib
    d = np.zeros(2, _lib.KIN_DERIVED_DTYPE)
    d["dispersion"][1] = [1, 2, 3, 4, 5, 6]
    st = nb.KinStats(3, 2, 0, 2, 0, 0, 6, 1)
    r = nb.LocalKinematics(6, np.zeros((2, 10)), None, np.array([4.0, np.inf]), None, np.zeros(2), np.zeros(2), d, st)
    assert np.array_equal(r.r_k, [2.0, np.inf]) and r.sigma.shape == (2,) and r.mean_velocity.shape == (2, 3)
    assert np.array_equal(r.dispersion_tensor[1], [[1, 2, 3], [2, 4, 5], [3, 5, 6]])
    with pytest.raises(ValueError):
        r.divergence
    r = nb.LocalKinematics(6, np.zeros((2, 10)), np.zeros((2, 15)), np.zeros(2), None, np.zeros(2), np.zeros(2), d, st)
    assert r.velocity_gradient.shape == (2, 3, 3) and r.vorticity.shape == (2, 3) and r.shear.shape == (2,)
