"""Disc modes without a GPU (include/nbody.h "Disc modes"): the numpy restatement of the rule
(tests/modes_ref.py) held to what the rule is for -- the recurrence against an 80-bit evaluation, exact dyadic cases,
a ring with a known mode, pattern speed and tilt, the three-level sums against math.fsum -- and the host side of the
library: nb_disc_modes_derive, the Python methods, the refusals that need no device."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import modes_ref as M

U = 2.0 ** -53


def as_disc_modes(nb, ref, edges, mmax, step_num=0, dt=0.016):
    """The restatement's result as the DiscModes a call returns (center, velocity: not part of the restatement)."""
    z = np.zeros(3)
    return nb.DiscModes(step_num, ref["n"], ref["nonfinite"], ref["inside_count"], ref["outside_count"],
                        float(ref["inside_mass"]), float(ref["outside_mass"]), float(ref["mass"]), z, z, ref["axis"],
                        ref["e1"], ref["e2"], 0, mmax, dt, np.asarray(edges, dtype=np.float64), ref["count"],
                        ref["m_r"], ref["m_h2"], ref["modes"])


# ---- the recurrence ------------------------------------------------------------------------------------------------
def test_recurrence_stays_within_4m_ulp_of_an_80_bit_evaluation():
    """c_m, s_m of the rule against cos / sin (m atan2(b, a)) in the platform's long double, over 1.2 10^6
    binary32-valued (a, b) with |b / a| spread over six decades either way.  Measured: 2.28 m 2^-53 at worst
    (17.8 2^-53 at m = 8)."""
    assert np.finfo(np.longdouble).nmant >= 63, "needs an 80-bit long double"
    rng = np.random.default_rng(20261020)
    k = 1_200_000
    a = (rng.uniform(0.5, 2.0, k) * rng.choice([-1.0, 1.0], k)).astype(np.float32)
    ratio = 10.0 ** rng.uniform(-6.0, 6.0, k)
    b = (a * ratio * rng.choice([-1.0, 1.0], k)).astype(np.float32)
    a, b = a.astype(np.float64), b.astype(np.float64)
    r2 = a * a + b * b
    big_r = np.sqrt(r2)
    rec = M.recurrence(a / big_r, b / big_r, M.MAX_M)
    phi = np.arctan2(b.astype(np.longdouble), a.astype(np.longdouble))
    worst = 0.0
    for m in range(1, M.MAX_M + 1):
        ec = np.abs(rec[m][0].astype(np.longdouble) - np.cos(m * phi)).max()
        es = np.abs(rec[m][1].astype(np.longdouble) - np.sin(m * phi)).max()
        err = float(max(ec, es)) / U
        print(f"m = {m}: worst |error| = {err:.2f} 2^-53 = {err / m:.2f} m 2^-53")
        worst = max(worst, err / m)
        assert err <= 4.0 * m, (m, err)
    print(f"worst over m: {worst:.2f} m 2^-53")


# ---- exact cases -----------------------------------------------------------------------------------------------------
def on_axes(radii, masses, speeds, heights):
    """One body per (radius, quarter turn q): at phi = q pi / 2 in the frame of axis (0, 1, 0) -- e1 = +x, e2 = -z --
    with mass masses[j][q], angular speed speeds[j][q] (velocity w R along the direction of growing phi) and
    height heights[j][q]."""
    e1, e2, n = np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, -1.0]), np.array([0.0, 1.0, 0.0])
    x, v, mass = [], [], []
    for j, r in enumerate(radii):
        for q in range(4):
            rad = (e1, e2, -e1, -e2)[q]
            tan = (e2, -e1, -e2, e1)[q]
            x.append(r * rad + heights[j][q] * n)
            v.append(speeds[j][q] * r * tan)
            mass.append(masses[j][q])
    return M.make_parts(np.array(x), np.array(v), np.array(mass))


def test_bodies_on_the_axes_give_exact_sums():
    radii = [1.0, 2.0, 4.0]
    masses = [[1.0, 0.5, 0.25, 2.0], [3.0, 1.5, 0.75, 0.125], [1.0, 1.0, 1.0, 1.0]]
    speeds = [[0.5, -0.25, 2.0, 1.0], [1.0, 1.0, -3.0, 0.5], [0.75, 0.75, 0.75, 0.75]]
    heights = [[0.5, 0.0, -0.25, 1.0], [0.0, 0.125, 0.0, -2.0], [0.25, 0.25, 0.25, 0.25]]
    parts = on_axes(radii, masses, speeds, heights)
    assert M.frame((0.0, 1.0, 0.0))[1].tolist() == [1.0, 0.0, 0.0] and M.frame((0.0, 1.0, 0.0))[2].tolist() == [0.0, 0.0, -1.0]
    edges = [1.0, 2.0, 4.0, 8.0]  # lower edge inclusive: the body at R = edges[k] is in bin k
    ref = M.modes_ref(parts, edges, 8, (0.0, 1.0, 0.0), (0.0, 0.0, 0.0))
    assert ref["count"].tolist() == [4, 4, 4] and ref["inside_count"] == 0 and ref["outside_count"] == 0
    cos4 = lambda m, q: (1, 0, -1, 0)[(m * q) % 4]  # noqa: E731   cos (m q pi / 2)
    sin4 = lambda m, q: (0, 1, 0, -1)[(m * q) % 4]  # noqa: E731
    for j in range(3):
        for m in range(9):
            want = [0.0] * 6
            for q in range(4):
                mu, w, h = masses[j][q], speeds[j][q], heights[j][q]
                for f, t in enumerate((mu * cos4(m, q), mu * sin4(m, q), mu * w * cos4(m, q), mu * w * sin4(m, q),
                                       mu * h * cos4(m, q), mu * h * sin4(m, q))):
                    want[f] += t
            assert ref["modes"][j, m].tolist() == want, (j, m)
        assert ref["m_r"][j] == sum(masses[j]) * radii[j]
        assert ref["m_h2"][j] == sum(mu * h * h for mu, h in zip(masses[j], heights[j]))
    # four equal bodies: C_4 = C_8 = sum mu, and nothing at m = 1, 2, 3
    assert ref["modes"][2, 4, 0] == 4.0 == ref["modes"][2, 8, 0] == ref["modes"][2, 0, 0]
    for m in (1, 2, 3, 5, 6, 7):
        assert ref["modes"][2, m].tolist() == [0.0] * 6
    assert ref["mass"] == sum(sum(r) for r in masses)


def test_edges_are_lower_inclusive_and_upper_exclusive():
    """Bodies at integer radii against integer edges: the bin by integer arithmetic."""
    radii = np.arange(0, 12)
    x = np.zeros((12, 3))
    x[:, 0] = radii
    parts = M.make_parts(x, np.zeros((12, 3)), np.ones(12))
    edges = [2.0, 3.0, 5.0, 9.0]
    ref = M.modes_ref(parts, edges, 0, (0.0, 1.0, 0.0), (0.0, 0.0, 0.0))
    want = [sum(1 for r in radii if lo <= r < hi) for lo, hi in zip((2, 3, 5), (3, 5, 9))]
    assert ref["count"].tolist() == want == [1, 2, 4]
    assert ref["inside_count"] == 2 and ref["outside_count"] == 3 and ref["mass"] == 12.0
    # a body at the centre counts in m = 0 alone
    ref = M.modes_ref(parts[:1], [0.0, 1.0], 3, (0.0, 1.0, 0.0), (0.0, 0.0, 0.0))
    assert ref["modes"][0, 0].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert not ref["modes"][0, 1:].any() and ref["count"].tolist() == [1]


def test_nonfinite_bodies_do_not_count_and_massless_ones_do():
    parts = on_axes([1.0], [[1.0, 0.0, 1.0, 0.0]], [[1.0] * 4], [[0.0] * 4])
    bad = parts.copy()
    bad["position"][0, 1] = np.nan
    bad["velocity"][1, 0] = np.inf
    bad["mass"][2] = np.nan
    ref = M.modes_ref(np.concatenate([parts, bad[:3]]), [0.5, 2.0], 2, (0.0, 1.0, 0.0), (0.0, 0.0, 0.0))
    assert ref["nonfinite"] == 3 and ref["count"].tolist() == [4]
    assert ref["modes"][0, 2].tolist()[:2] == [2.0, 0.0] and ref["mass"] == 2.0


# ---- a ring ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [(0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.3, -0.5, 0.8)])
def test_a_ring_gives_its_mode_phase_and_pattern_speed(nb, axis):
    """Tolerance 1e-6: binary32's 6e-8 relative rounding of the inputs with a margin."""
    eps, phi0, omega0 = 0.25, 0.3, 1.7
    parts = M.ring(360, 1.0, eps, phi0, omega0, axis)
    edges = [0.5, 1.5]
    d = as_disc_modes(nb, M.modes_ref(parts, edges, 4, axis, (0.0, 0.0, 0.0)), edges, 4)
    a2, phase, omega = d.amplitude(2)[0], d.phase(2)[0], d.pattern_speed(2)[0]
    print(f"A2 - eps/2 = {a2 - eps / 2:.2e}, phase - phi0 = {phase - phi0:.2e}, Omega - Omega0 = {omega - omega0:.2e}, "
          f"A1 = {d.amplitude(1)[0]:.2e}, A3 = {d.amplitude(3)[0]:.2e}")
    assert abs(a2 - eps / 2) < 1e-6 and abs(phase - phi0) < 1e-6 and abs(omega - omega0) < 1e-6
    assert d.amplitude(1)[0] < 1e-6 and d.amplitude(3)[0] < 1e-6
    assert d.bar_strength() == (a2, 0)
    assert abs(d.thickness()[0]) < 1e-6 and d.warp_tilt()[0] < 1e-6


@pytest.mark.parametrize("axis", [(0.0, 1.0, 0.0), (0.3, -0.5, 0.8)])
def test_a_tilted_ring_gives_its_tilt_and_its_line_of_nodes(nb, axis):
    """h = R (alpha cos phi + beta sin phi) on equal masses: warp_tilt = hypot(alpha, beta), the highest point at
    atan2(beta, alpha), the line of nodes a quarter turn from it."""
    alpha, beta = 0.03, -0.04
    parts = M.ring(360, 1.0, 0.0, 0.0, 1.7, axis, alpha, beta)
    edges = [0.5, 1.5]
    d = as_disc_modes(nb, M.modes_ref(parts, edges, 2, axis, (0.0, 0.0, 0.0)), edges, 2)
    amp, phase = d.bending(1)
    print(f"tilt - hypot = {d.warp_tilt()[0] - math.hypot(alpha, beta):.2e}, "
          f"phase - atan2 = {phase[0] - math.atan2(beta, alpha):.2e}")
    assert abs(d.warp_tilt()[0] - math.hypot(alpha, beta)) < 1e-6
    assert abs(phase[0] - math.atan2(beta, alpha)) < 1e-6
    assert abs(2.0 * amp[0] - math.hypot(alpha, beta)) < 1e-6  # (R = 1)
    assert abs(d.thickness()[0] - math.hypot(alpha, beta) / math.sqrt(2.0)) < 1e-6


# ---- the sums against a brute force ----------------------------------------------------------------------------------
def float_state(seed, n=12000):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, (n, 3)) * [1.0, 0.1, 1.0]
    v = rng.normal(0.0, 1.0, (n, 3))
    mass = 10.0 ** rng.uniform(-3.0, 3.0, n)
    return M.make_parts(x, v, mass)


@pytest.mark.parametrize("seed", [1, 2])
def test_sums_stay_within_1e10_of_fsum(seed):
    """Every sum of the restatement against math.fsum of its terms: 1e-10 sum |term|, the halo pass's constant."""
    parts = float_state(seed)
    edges = [0.0, 0.2, 3.0, 4.0]  # the middle bin holds more than two chunks
    ref = M.modes_ref(parts, edges, 8, (0.1, 1.0, -0.2), (0.01, 0.02, -0.01), (0.1, 0.0, 0.0))
    assert ref["count"][1] > 2 * M.CHUNK
    worst = 0.0
    for k in range(3):
        terms = ref["terms"][ref["key"] == k + 1]
        for f in range(terms.shape[1]):
            exact, scale = math.fsum(terms[:, f]), math.fsum(np.abs(terms[:, f]))
            got = (ref["modes"][k].reshape(-1)[f] if f < 54 else (ref["m_r"][k], ref["m_h2"][k])[f - 54])
            assert abs(got - exact) <= 1e-10 * scale, (k, f, got, exact, scale)
            worst = max(worst, abs(got - exact) / scale if scale else 0.0)
    print(f"worst |sum - fsum| / sum |term| = {worst:.2e}")
    assert ref["inside_count"] + ref["outside_count"] + int(ref["count"].sum()) == len(parts)


def test_a_bins_bits_depend_on_its_members_alone():
    parts = float_state(3, 6000)
    args = ((0.0, 1.0, 0.0), (0.0, 0.0, 0.0))
    a = M.modes_ref(parts, [0.5, 1.0, 2.0], 4, *args)
    b = M.modes_ref(parts, [0.1, 0.2, 0.5, 1.0, 5.0], 4, *args)
    assert a["modes"][0].tobytes() == b["modes"][2].tobytes() and a["count"][0] == b["count"][2]
    assert (a["m_r"][0], a["m_h2"][0]) == (b["m_r"][2], b["m_h2"][2])


# ---- through the library, without a device ---------------------------------------------------------------------------
def test_frame_is_map_frame(nb):
    for axis in ((0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.3, -0.5, 0.8), (1.0, 1.0, 1.0), (-2.0, 0.1, 0.1)):
        for mine, theirs in zip(M.frame(axis), nb.map_frame(axis)):
            assert mine.tobytes() == theirs.tobytes(), axis


def test_struct_sizes_and_symbols(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    assert C.sizeof(_lib.nb_modes_params) == 96 and C.sizeof(_lib.nb_modes_head) == 200
    assert _lib.MODES_BIN_DTYPE.itemsize == 24 and _lib.MODES_DERIVED_DTYPE.itemsize == 40
    assert (_lib.NB_MODES_MAX_BINS, _lib.NB_MODES_MAX_M, _lib.NB_MODES_FIELDS, _lib.NB_MODES_CHUNK) == \
        (M.MAX_BINS, M.MAX_M, M.FIELDS, M.CHUNK)
    for name in ("nb_disc_modes_sim", "nb_disc_modes_runner", "nb_disc_modes_derive"):
        assert name in _lib.ABI_SYMBOLS and hasattr(L, name)
    a, b = L.nb_disc_modes_sim.argtypes, L.nb_disc_modes_runner.argtypes
    assert a is not None and a is b  # one list for the two
    assert nb.MODES_FIELDS == ("C", "S", "DC", "DS", "ZC", "ZS")


def test_the_method_is_shared(nb):
    assert nb.Simulator.disc_modes is nb.OfflineHeadless.disc_modes


def test_derive_equals_the_numpy_formulas(nb):
    rng = np.random.default_rng(5)
    modes = rng.normal(0.0, 1.0, (7, 5, 6))
    modes[:, 0, 0] = np.abs(modes[:, 0, 0]) + 1.0
    modes[1, 0, 0] = 0.0                 # no mass: NaN throughout
    modes[2, 2, 0:2] = 0.0               # no mode 2: phase and pattern speed NaN, amplitude 0
    modes[3, 2, 4:6] = 0.0               # no bending mode 2: its phase NaN
    modes[4, 0, 0] = np.nan
    ref = dict(n=0, nonfinite=0, inside_count=0, outside_count=0, inside_mass=0.0, outside_mass=0.0, mass=0.0,
               axis=np.zeros(3), e1=np.zeros(3), e2=np.zeros(3), count=np.zeros(7, np.uint64), m_r=np.ones(7),
               m_h2=np.ones(7), modes=modes)
    d = as_disc_modes(nb, ref, np.arange(8.0), 4)
    for m in (1, 2, 3, 4):
        want = M.derive(modes, m)
        got = d.derived(m)
        for name, w in zip(("amplitude", "phase", "pattern_speed", "bend_amplitude", "bend_phase"), want):
            # the pattern speed is +, x and / alone: to the bit; hypot and atan2 are the C library's against Python's:
            # a few units in the last place, the NaNs in the same places
            assert np.array_equal(np.isnan(got[name]), np.isnan(w)), (m, name)
            if name == "pattern_speed":
                assert np.array_equal(got[name], w, equal_nan=True), (m, name, got[name], w)
            else:
                assert np.allclose(got[name], w, rtol=1e-15, atol=0.0, equal_nan=True), (m, name, got[name], w)
        assert np.all(np.abs(got["phase"][np.isfinite(got["phase"])]) <= math.pi / m)
    got = d.derived(2)
    assert all(np.isnan(got[name][1]) and np.isnan(got[name][4]) for name in got.dtype.names)
    assert got["amplitude"][2] == 0.0 and np.isnan(got["phase"][2]) and np.isnan(got["pattern_speed"][2])
    assert np.isnan(got["bend_phase"][3]) and np.isfinite(got["phase"][3])
    assert np.array_equal(d.total(2), sum((modes[k, 2] for k in range(1, 7)), modes[0, 2] + np.zeros(6)), equal_nan=True)
    with pytest.raises(nb.NBodyError):
        d.derived(0)
    with pytest.raises(nb.NBodyError):
        d.derived(5)


@pytest.mark.parametrize("m", [1, 2, 3, 4])
@pytest.mark.parametrize("turn", [0.1, -0.2, 2.0, -2.9])
def test_pattern_speed_between_recovers_a_rotation(nb, m, turn):
    """Two restated rings whose mode m is `turn` apart: the phase difference wrapped into (-pi/m, pi/m], over the
    time between them."""
    edges, axis = [0.5, 1.5], (0.0, 1.0, 0.0)
    phi0 = 0.2
    first = as_disc_modes(nb, M.modes_ref(M.ring(360, 1.0, 0.25, phi0, 0.0, axis, m=m), edges, 4, axis, (0, 0, 0)),
                          edges, 4, step_num=10, dt=0.5)
    second = as_disc_modes(nb, M.modes_ref(M.ring(360, 1.0, 0.25, phi0 + turn, 0.0, axis, m=m), edges, 4, axis,
                                           (0, 0, 0)), edges, 4, step_num=14, dt=0.5)
    period = 2.0 * math.pi / m
    wrapped = turn - period * math.ceil(turn / period - 0.5)
    assert -period / 2 < wrapped <= period / 2
    assert abs(first.pattern_speed_between(second, m, time=1.0)[0] - wrapped) < 1e-6
    assert abs(first.pattern_speed_between(second, m)[0] - wrapped / 2.0) < 1e-6  # 4 steps of 0.5


def test_argument_refusals_need_no_device(nb):
    """What is refused before any device call is refused before the handle is looked at: the same messages with no
    simulator at all."""
    from wgpu_n_body_amd import _lib
    L = _lib.lib()

    def call(fn, edges=(0.5, 1.0, 2.0), mmax=4, flags=0, reserved=0, axis=(0.0, 1.0, 0.0), center=(0.0, 0.0, 0.0),
             velocity=(0.0, 0.0, 0.0), nbins=None, params=True, out=True, bins=True, modes=True, null_edges=False):
        e = np.asarray(edges, dtype=np.float64)
        p = _lib.nb_modes_params()
        p.nbins, p.mmax, p.flags, p.reserved = (len(e) - 1 if nbins is None else nbins), mmax, flags, reserved
        for k in range(3):
            p.axis[k], p.center[k], p.velocity[k] = axis[k], center[k], velocity[k]
        p.edges = None if null_edges else e.ctypes.data_as(C.POINTER(C.c_double))
        head = _lib.nb_modes_head()
        b = np.full(8 * 24, 7, np.uint8)
        md = np.full(64, 7.0)
        rc = fn(None, C.byref(p) if params else None, C.byref(head) if out else None, b.ctypes.data if bins else None,
                md.ctypes.data if modes else None)
        assert np.all(b == 7) and np.all(md == 7.0)
        return rc, L.nb_last_error()

    nan, inf = float("nan"), float("inf")
    for fn in (L.nb_disc_modes_sim, L.nb_disc_modes_runner):
        for word, kw in ((b"null params", dict(params=False)), (b"null out", dict(out=False)),
                         (b"null bins", dict(bins=False)), (b"null modes", dict(modes=False)),
                         (b"null edges", dict(null_edges=True)), (b"nbins must be 1..256", dict(nbins=0)),
                         (b"nbins must be 1..256", dict(nbins=257)), (b"mmax must be 0..8", dict(mmax=9)),
                         (b"unknown flag bits", dict(flags=2)), (b"reserved", dict(reserved=1)),
                         (b"edges[1]", dict(edges=(0.5, 0.5, 2.0))), (b"edges[2]", dict(edges=(0.5, 1.0, 0.9))),
                         (b"edges[0]", dict(edges=(-0.5, 1.0))), (b"edges[1]", dict(edges=(0.5, nan))),
                         (b"edges[1]", dict(edges=(0.5, inf))), (b"center and velocity", dict(center=(0.0, nan, 0.0))),
                         (b"center and velocity", dict(velocity=(inf, 0.0, 0.0))),
                         (b"non-zero finite axis", dict(axis=(0.0, 0.0, 0.0))),
                         (b"non-zero finite axis", dict(axis=(0.0, nan, 0.0))),
                         (b"non-zero finite axis", dict(axis=(1e200, 1e200, 0.0)))):
            rc, msg = call(fn, **kw)
            assert rc == _lib.NB_ERR_INVALID and word in msg, (word, rc, msg)
        for kw in (dict(), dict(flags=1, center=(nan, nan, nan)), dict(mmax=0), dict(mmax=8)):
            rc, msg = call(fn, **kw)  # good arguments: the handle is what is missing
            assert rc == _lib.NB_ERR_INVALID and (b"null simulator" in msg or b"null runner" in msg), (kw, msg)
    out = np.zeros(2, _lib.MODES_DERIVED_DTYPE)
    md = np.zeros((2, 3, 6))
    assert L.nb_disc_modes_derive(None, 2, 2, 1, out.ctypes.data) == _lib.NB_ERR_INVALID
    assert L.nb_disc_modes_derive(md.ctypes.data, 2, 2, 1, None) == _lib.NB_ERR_INVALID
    assert L.nb_disc_modes_derive(md.ctypes.data, 0, 2, 1, out.ctypes.data) == _lib.NB_ERR_INVALID
    assert L.nb_disc_modes_derive(md.ctypes.data, 2, 9, 1, out.ctypes.data) == _lib.NB_ERR_INVALID
    assert L.nb_disc_modes_derive(md.ctypes.data, 2, 2, 3, out.ctypes.data) == _lib.NB_ERR_INVALID
    assert L.nb_disc_modes_derive(md.ctypes.data, 2, 2, 2, out.ctypes.data) == _lib.NB_OK
