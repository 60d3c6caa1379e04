"""Shell modes without a GPU (include/nbody.h "Shell modes"): the numpy restatement of the rule
(tests/shell_ref.py) held to what the rule is for -- the recurrences against an 80-bit evaluation, exact dyadic cases
on the axes, rotation invariance of the power, the rates against central differences, rigid rotation and pure
expansion, the three-level sums against math.fsum -- and the host side of the library: nb_shell_modes_derive, the
Python result class, the refusals that need no device."""
import ctypes as C
import functools
import math
from fractions import Fraction

import numpy as np
import pytest
from numpy.polynomial.legendre import Legendre

from tests import shell_ref as S

U = 2.0 ** -53
LM = [(l, m) for l in range(S.MAX_L + 1) for m in range(l + 1)]


def q_at_one(l, m):
    """Q_l^m(1) = (l + m)! / (2^m m! (l - m)!): the largest |d^m P_l / d zeta^m| on [-1, 1], the unit of a term."""
    return math.factorial(l + m) / (2 ** m * math.factorial(m) * math.factorial(l - m))


# The worst error of every term Q_l^m (c_m, s_m) in units of 2^-53 Q_l^m(1), measured by
# test_recurrences_stay_within_twice_the_measured_error_of_an_80_bit_evaluation (seed 20261021, 1.2 10^6 directions),
# and the bound held: twice the measured worst, rounded up to an integer.  The m = 0 column is the largest because
# dP_l / d zeta reaches l (l + 1) / 2 at the poles: the 1.5 2^-53 relative rounding of zeta = h / r itself moves P_6 by
# up to 31 units there, whatever evaluates the polynomial afterwards.
MEASURED = {(0, 0): 0.0, (1, 0): 1.91, (1, 1): 2.09, (2, 0): 6.75, (2, 1): 2.44, (2, 2): 4.99, (3, 0): 14.41,
            (3, 1): 3.26, (3, 2): 2.66, (3, 3): 6.89, (4, 0): 22.79, (4, 1): 3.84, (4, 2): 2.38, (4, 3): 2.93,
            (4, 4): 9.26, (5, 0): 32.91, (5, 1): 4.86, (5, 2): 2.16, (5, 3): 2.10, (5, 4): 2.98, (5, 5): 11.10,
            (6, 0): 45.39, (6, 1): 5.36, (6, 2): 2.09, (6, 3): 1.44, (6, 4): 1.70, (6, 5): 3.19, (6, 6): 13.46}
BOUND = {lm: math.ceil(2.0 * w) for lm, w in MEASURED.items()}


def as_shell_modes(nb, ref, edges, step_num=0, dt=0.016):
    """The restatement's result as the ShellModes a call returns (center, velocity: not part of the restatement)."""
    z = np.zeros(3)
    flags = 0 if ref["rate"] is None else 2
    return nb.ShellModes(step_num, ref["n"], ref["nonfinite"], ref["inside_count"], ref["outside_count"],
                         float(ref["inside_mass"]), float(ref["outside_mass"]), float(ref["mass"]), z, z, ref["axis"],
                         ref["e1"], ref["e2"], flags, ref["lmax"], dt, np.asarray(edges, dtype=np.float64),
                         ref["count"], ref["m_r"], ref["m_ur"], ref["coef"], ref["rate"])


# ---- the recurrences -------------------------------------------------------------------------------------------------
def directions(seed, k):
    """k binary32-valued vectors: three quarters isotropic, an eighth within 10^-9 .. 10^-6 of a pole, an eighth
    within 10^-9 .. 10^-6 of the equator; lengths 2^-3 .. 2^3."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(k, 3))
    q = k // 8
    eps, turn = 10.0 ** rng.uniform(-9.0, -6.0, q), rng.uniform(0.0, 2.0 * np.pi, q)
    d[:q, 0], d[:q, 1], d[:q, 2] = eps * np.cos(turn), eps * np.sin(turn), rng.choice([-1.0, 1.0], q)
    eps = 10.0 ** rng.uniform(-9.0, -6.0, q) * rng.choice([-1.0, 1.0], q)
    d[q:2 * q, 2] = eps * np.hypot(d[q:2 * q, 0], d[q:2 * q, 1])
    d *= (2.0 ** rng.integers(-3, 4, k))[:, None]
    return d.astype(np.float32)


def test_recurrences_stay_within_twice_the_measured_error_of_an_80_bit_evaluation():
    """Q_l^m c_m and Q_l^m s_m of the rule -- zeta, alpha, beta as the rule divides them, polar axis z -- against
    Legendre.basis(l).deriv(m) evaluated in the platform's long double times sin^m theta (cos, sin)(m atan2(y, x)),
    over 1.2 10^6 binary32-valued vectors, a quarter of them within 10^-6 of the poles or of the equator.  In units
    of 2^-53 Q_l^m(1) the measured worst is 45.39 (l = 6, m = 0; seeds 1 and 2: 47.92 and 43.32); per term it is
    MEASURED above, and twice that, rounded up, is asserted.  The margin covers other seeds, not other code."""
    assert np.finfo(np.longdouble).nmant >= 63, "needs an 80-bit long double"
    d = directions(20261021, 1_200_000).astype(np.float64)
    r = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    val, _ = S.harmonics(d[:, 2] / r, d[:, 0] / r, d[:, 1] / r, S.MAX_L)
    ld = np.longdouble
    x, y, z = (d[:, j].astype(ld) for j in range(3))
    rho2 = x * x + y * y
    big = np.sqrt(rho2 + z * z)
    zeta, sin_theta, phi = z / big, np.sqrt(rho2) / big, np.arctan2(y, x)
    assert (np.abs(zeta) > 1.0 - 1e-12).sum() > 1000 and (np.abs(zeta) < 1e-6).sum() > 1000
    failed = []
    for l, m in LM:
        q = Legendre.basis(l).deriv(m)(zeta)
        assert q.dtype == ld
        base = q * sin_theta ** m
        err = np.abs(val[S.index(l, m)].astype(ld) - base * np.cos(m * phi)).max()
        if m:
            err = max(err, np.abs(val[S.index(l, m, True)].astype(ld) - base * np.sin(m * phi)).max())
        units = float(err) / (U * q_at_one(l, m))
        print(f"(l, m) = ({l}, {m}): worst |error| = {units:.2f} 2^-53 Q(1), bound {BOUND[l, m]}")
        if units > BOUND[l, m]:
            failed.append((l, m, units))
    assert not failed, failed


def test_q_is_the_legendre_derivative_and_its_diagonal_is_the_double_factorial():
    zeta = np.linspace(-1.0, 1.0, 41)
    one, zero = np.ones_like(zeta), np.zeros_like(zeta)
    val, _ = S.harmonics(zeta, one, zero, S.MAX_L)  # alpha = 1, beta = 0: c_m = 1, s_m = 0
    for l, m in LM:
        want = Legendre.basis(l).deriv(m)(zeta)
        assert np.abs(val[S.index(l, m)] - want).max() <= 64 * U * q_at_one(l, m), (l, m)
        if m:
            assert not val[S.index(l, m, True)].any()
    for m, dfact in enumerate((1.0, 1.0, 3.0, 15.0, 105.0, 945.0, 10395.0)):
        assert val[S.index(m, m)].tolist() == [dfact] * len(zeta)
        assert val[S.index(m, m), -1] == q_at_one(m, m)


# ---- exact cases -----------------------------------------------------------------------------------------------------
def q_at_zero(l, m):
    """d^m P_l / d zeta^m at 0: 0 for odd l - m, else (-1)^((l - m) / 2) (l + m - 1)!! / (l - m)!!."""
    if (l - m) % 2:
        return Fraction(0)
    dfact = lambda k: functools.reduce(lambda a, b: a * b, range(k, 0, -2), 1)  # noqa: E731
    return Fraction((-1) ** ((l - m) // 2) * dfact(l + m - 1), dfact(l - m))


def on_axis_values(which, lmax):
    """The (lmax + 1)^2 values Q_l^m (c_m, s_m) of a body on +e1, -e1, +e2, -e2, +n, -n (which = 0 .. 5), exactly."""
    out = [Fraction(0)] * (lmax + 1) ** 2
    for l in range(lmax + 1):
        for m in range(l + 1):
            if which >= 4:    # zeta = +-1, alpha = beta = 0: m = 0 alone, P_l(+-1) = (+-1)^l
                c, s, q = (1 if m == 0 else 0), 0, Fraction(1 if which == 4 else (-1) ** l)
            else:             # zeta = 0, (alpha, beta) = (+-1, 0) or (0, +-1): c_m + i s_m = (alpha + i beta)^m
                turn = (0, 2, 1, 3)[which]  # quarter turns of phi
                c, s = (1, 0, -1, 0)[(m * turn) % 4], (0, 1, 0, -1)[(m * turn) % 4]
                q = q_at_zero(l, m)
            out[S.index(l, m)] = q * c
            if m:
                out[S.index(l, m, True)] = q * s
    return out


AXIS_Y = (0.0, 1.0, 0.0)  # e1 = +x, e2 = -z, n = +y
SIX = [np.array(v) for v in ((1.0, 0, 0), (-1.0, 0, 0), (0, 0, -1.0), (0, 0, 1.0), (0, 1.0, 0), (0, -1.0, 0))]


def test_bodies_on_the_axes_give_exact_sums():
    """One body on each of +-e1, +-e2, +-n per shell, at power-of-two radii and masses: every value is a dyadic
    rational that the recurrences reach without a rounding, so every sum equals the closed form."""
    n, e1, e2 = S.frame(AXIS_Y)
    assert e1.tolist() == [1.0, 0.0, 0.0] and e2.tolist() == [0.0, 0.0, -1.0] and n.tolist() == [0.0, 1.0, 0.0]
    radii = [0.5, 1.0, 4.0]
    masses = [[1.0, 0.5, 0.25, 2.0, 4.0, 0.125], [1.0] * 6, [2.0, 2.0, 0.5, 0.5, 8.0, 1.0]]
    x = np.array([r * SIX[w] for r in radii for w in range(6)])
    parts = S.make_parts(x, 0.5 * x, np.array(masses).reshape(-1))
    edges = [0.5, 1.0, 4.0, 8.0]  # lower edge inclusive
    ref = S.shell_ref(parts, edges, S.MAX_L, AXIS_Y, (0.0, 0.0, 0.0))
    assert ref["count"].tolist() == [6, 6, 6] and ref["inside_count"] == 0 == ref["outside_count"]
    for j in range(3):
        want = [sum(Fraction(masses[j][w]) * on_axis_values(w, S.MAX_L)[i] for w in range(6)) for i in range(49)]
        assert [Fraction(float(v)) for v in ref["coef"][j]] == want, j
        assert ref["m_r"][j] == sum(masses[j]) * radii[j]
        assert ref["m_ur"][j] == 0.5 * sum(masses[j]) * radii[j]
    # six equal bodies on the axes: an octahedron has no l = 1, 2, 3, 5 and a definite l = 4: C_40 = 2 + 4 (3 / 8)
    assert not ref["coef"][1, 1:16].any() and not ref["coef"][1, 25:36].any()
    assert ref["coef"][1, S.index(4, 0)] == 3.5 and ref["coef"][1, S.index(4, 4)] == 4 * 105.0
    assert ref["mass"] == sum(sum(r) for r in masses)


@pytest.mark.parametrize("which", range(6))
def test_one_body_on_an_axis_has_a_flat_spectrum(nb, which):
    """A point on the sphere: sum_m Y_lm^2 = (2l + 1) / 4 pi for every l (the addition theorem), so power_l = 1 / 4 pi
    and relative_l = 1 whatever the axis -- which holds N_lm of nb_shell_modes_derive to its closed form.  The sums
    are exact, so only N_lm (two roundings and a square root each), the squares and 2l additions round: 16 2^-53."""
    parts = S.make_parts([2.0 * SIX[which]], [[0.0, 0.0, 0.0]], [4.0])
    ref = S.shell_ref(parts, [1.0, 4.0], S.MAX_L, AXIS_Y, (0.0, 0.0, 0.0))
    d = as_shell_modes(nb, ref, [1.0, 4.0])
    power, a = d.power()[0], d.normalised()[0]
    assert np.abs(power * (4.0 * math.pi) / 16.0 - 1.0).max() <= 16 * U, power
    assert np.abs(np.array([d.relative(l)[0] for l in range(S.MAX_L + 1)]) - 1.0).max() <= 16 * U
    values = on_axis_values(which, S.MAX_L)
    for l, m in LM:
        n_lm = math.sqrt((1 if m == 0 else 2) * (2 * l + 1) / (4.0 * math.pi)
                         * math.factorial(l - m) / math.factorial(l + m))
        assert abs(a[S.index(l, m)] - 4.0 * n_lm * float(values[S.index(l, m)])) <= 8 * U * 4.0 * n_lm * q_at_one(l, m)
    want = 4.0 * math.sqrt(3.0 / (4.0 * math.pi)) * SIX[which]  # the l = 1 vector points at the body
    assert np.abs(d.dipole()[0] - want).max() <= 8 * U * np.abs(want).max()
    lam, axes = d.quadrupole_axes()  # mu (5 / 4 pi) (3 x x^T - 1) / 2: eigenvalues (1, -1/2, -1/2) mu 5 / 4 pi, major axis x
    scale = 4.0 * 5.0 / (4.0 * math.pi)
    assert np.abs(lam[0] / scale - [1.0, -0.5, -0.5]).max() <= 32 * U
    assert np.abs(np.abs(axes[0, 0]) - np.abs(SIX[which])).max() <= 32 * U


def test_edges_are_lower_inclusive_and_the_centre_counts_in_l0_alone():
    radii = np.arange(0, 12)
    x = np.zeros((12, 3))
    x[:, 2] = radii
    parts = S.make_parts(x, np.ones((12, 3)), np.ones(12))
    ref = S.shell_ref(parts, [2.0, 3.0, 5.0, 9.0], 0, AXIS_Y, (0.0, 0.0, 0.0))
    assert ref["count"].tolist() == [1, 2, 4] and ref["inside_count"] == 2 and ref["outside_count"] == 3
    assert ref["mass"] == 12.0
    ref = S.shell_ref(parts[:1], [0.0, 1.0], 4, AXIS_Y, (0.0, 0.0, 0.0), rates=True)
    assert ref["coef"][0].tolist() == [1.0] + [0.0] * 24 and ref["rate"][0].tolist() == [0.0] * 25
    assert not np.signbit(ref["coef"][0]).any() and not np.signbit(ref["rate"][0]).any()
    assert ref["m_r"][0] == 0.0 and ref["m_ur"][0] == 0.0 and ref["count"].tolist() == [1]


def test_nonfinite_bodies_do_not_count_and_massless_ones_do():
    x = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [1.0, 1.0, 0]])
    parts = S.make_parts(x, np.zeros((4, 3)), [1.0, 0.0, 1.0, 0.0])
    bad = parts.copy()
    bad["position"][0, 1] = np.nan
    bad["velocity"][1, 0] = np.inf
    bad["mass"][2] = np.nan
    ref = S.shell_ref(np.concatenate([parts, bad[:3]]), [0.5, 2.0], 2, AXIS_Y, (0.0, 0.0, 0.0))
    assert ref["nonfinite"] == 3 and ref["count"].tolist() == [4] and ref["mass"] == 2.0


# ---- rotation invariance ---------------------------------------------------------------------------------------------
def rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def term_tolerance(l, m, extra):
    """The error of one body's term (l, m) per unit mass: (BOUND + extra) 2^-53 Q_l^m(1)."""
    return (BOUND[l, m] + extra) * U * q_at_one(l, m)


def test_power_does_not_change_under_a_rotation_of_the_bodies(nb):
    """power_l of a triaxial Gaussian cloud of 4,000 bodies before and after a random rotation, the rotated positions
    formed in long double and rounded once to binary64 (binary32 would move every direction by 6 10^-8).  With exact
    arithmetic |a_l| would not change.  A computed a_lm is off by at most N_lm sum mu (BOUND + 2l + 70) 2^-53
    Q_l^m(1): BOUND the measured term bound, 2l the rounding of the rotated position (a direction moves by at most
    sqrt(3) 2^-53 and a spherical polynomial of degree l, |term| <= Q(1), has a gradient of at most l Q(1)), 70 the 6
    + 63 additions of the run and chunk levels (one chunk).  Then |power - power'| <= (|a| + |a'|) (|delta| +
    |delta'|) / (2l + 1)."""
    rng = np.random.default_rng(7)
    n_bodies = 4000
    x = rng.normal(size=(n_bodies, 3)) * [1.0, 0.7, 0.4]
    mass = rng.uniform(0.5, 1.5, n_bodies)
    rot = rotation(rng)
    xr = (x.astype(np.longdouble) @ rot.T.astype(np.longdouble)).astype(np.float64)
    n, e1, e2 = S.frame((0.3, -0.5, 0.8))
    zero = np.zeros(3)
    nlm = S.norms(S.MAX_L)

    def measure(pos):
        _, terms = S.body_terms(pos, np.zeros_like(pos), mass, zero, zero, n, e1, e2, S.MAX_L, False)
        coef = S.level_sums(terms)[None, :49]
        return S.derive(coef, None, S.MAX_L, n, e1, e2)

    a, b = measure(x), measure(xr)
    assert a["relative"][0, 2] > 0.05  # (the cloud is triaxial: there is something to preserve)
    worst = 0.0
    for l in range(S.MAX_L + 1):
        idx = range(l * l, (l + 1) ** 2)
        delta = math.sqrt(sum((nlm[S.index(l, m)] * mass.sum() * term_tolerance(l, m, 2 * l + 70)) ** 2
                              * (1 if m == 0 else 2) for m in range(l + 1)))
        na, nb_ = (math.sqrt(sum(r["norm"][0, i] ** 2 for i in idx)) for r in (a, b))
        tol = (na + nb_) * 2.0 * delta / (2 * l + 1)
        diff = abs(a["power"][0, l] - b["power"][0, l])
        print(f"l = {l}: power {a['power'][0, l]:.6e}, |difference| {diff:.2e}, tolerance {tol:.2e}")
        assert diff <= tol, (l, diff, tol)
        worst = max(worst, diff / tol)
    print(f"worst |difference| / tolerance = {worst:.3f}")
    # and the l = 2 axes turn with the bodies
    assert np.abs(np.abs(a["quad_axes"][0] @ rot.T) - np.abs(b["quad_axes"][0])).max() < 1e-9
    assert np.abs(a["quad_values"][0] - b["quad_values"][0]).max() < 1e-9 * np.abs(a["quad_values"][0]).max()


def test_the_quadrupole_axes_are_the_inertia_tensors():
    """Of one thin shell: the l = 2 tensor is (5 / 4 pi) sum mu (3 x x^T - 1) / 2 over unit vectors, so its axes are
    those of sum mu x x^T, major first."""
    rng = np.random.default_rng(11)
    x = rng.normal(size=(3000, 3)) * [0.4, 1.0, 0.7]
    x /= np.linalg.norm(x, axis=1)[:, None]
    parts = S.make_parts(x, np.zeros_like(x), np.ones(len(x)))
    ref = S.shell_ref(parts, [0.5, 2.0], 2, (0.2, 0.9, -0.4), (0.0, 0.0, 0.0))
    d = S.derive(ref["coef"], None, 2, ref["axis"], ref["e1"], ref["e2"])
    xs = parts["position"].astype(np.float64)
    xs /= np.linalg.norm(xs, axis=1)[:, None]
    tensor = (5.0 / (4.0 * math.pi)) * (1.5 * xs.T @ xs - 0.5 * len(xs) * np.eye(3))
    lam, vec = np.linalg.eigh(tensor)
    assert np.abs(d["quad_values"][0] - lam[::-1]).max() < 1e-9 * np.abs(lam).max()
    assert np.abs(np.abs(d["quad_axes"][0]) - np.abs(vec[:, ::-1].T)).max() < 1e-9
    assert abs(d["quad_values"][0].sum()) < 1e-9 * np.abs(lam).max()  # traceless


# ---- the rates -------------------------------------------------------------------------------------------------------
def shell_cloud(seed, n_bodies, rmin=0.5, rmax=2.0):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n_bodies, 3)) * [1.0, 0.7, 0.4]
    x *= (rng.uniform(rmin, rmax, n_bodies) / np.linalg.norm(x, axis=1))[:, None]
    return rng, x.astype(np.float32).astype(np.float64)


def test_rates_equal_central_differences():
    """The rates of 500 bodies (0.5 <= r <= 2, |u| <= 1, masses 0.5 .. 1.5) against (f(x + h u) - f(x - h u)) / 2h of
    the restatement's own values on binary64 positions, h = 10^-4, lmax = 4.  Tolerance per (l, m), times sum mu:
      truncation  h^2 / 6 max |f'''| with |f'''| <= 5 l^3 w^3 Q(1), w = max |u| / min r = 2 the largest angular rate:
                  along a straight line the angle has |theta'| <= w, |theta''| <= 0.65 w^2, |theta'''| <= 2 w^3, a
                  spherical polynomial of degree l has |d^k f / d theta^k| <= l^k Q(1), and l^3 + 1.95 l^2 + 2 l <=
                  5 l^3;
      rounding    2 (BOUND + 2l) 2^-53 Q(1) / 2h for the two values (2l: the rounding of x +- h u) and the same
                  again, without h, for the rate itself."""
    rng, x = shell_cloud(3, 500)
    u = rng.normal(size=x.shape)
    u /= np.maximum(np.linalg.norm(u, axis=1), 1.0)[:, None]
    u = u.astype(np.float32).astype(np.float64)
    mass = rng.uniform(0.5, 1.5, len(x)).astype(np.float32).astype(np.float64)
    n, e1, e2 = S.frame((0.3, -0.5, 0.8))
    zero, lmax, h, w = np.zeros(3), S.MAX_L_RATES, 1e-4, 2.0
    nk = (lmax + 1) ** 2

    def per_body(pos, rates):
        return S.body_terms(pos, u, mass, zero, zero, n, e1, e2, lmax, rates)[1]

    rate = per_body(x, True)[:, nk:2 * nk]
    fd = (per_body(x + h * u, False)[:, :nk] - per_body(x - h * u, False)[:, :nk]) / (2.0 * h)
    worst = 0.0
    for l in range(lmax + 1):
        for m in range(l + 1):
            q1 = q_at_one(l, m)
            tol = (h * h / 6.0 * 5.0 * l ** 3 * w ** 3 * q1 + 2.0 * term_tolerance(l, m, 2 * l) / (2.0 * h)
                   + term_tolerance(l, m, 2 * l) * w * l)
            for i in [S.index(l, m)] + ([S.index(l, m, True)] if m else []):
                err = (np.abs(rate[:, i] - fd[:, i]) / mass).max()
                assert err <= tol, (l, m, err, tol)
                worst = max(worst, err / tol) if tol else worst
    print(f"worst |rate - difference| / tolerance = {worst:.3f}")
    assert not rate[:, 0].any()  # l = 0 does not change


def test_rigid_rotation_gives_its_pattern_speed_and_keeps_the_power(nb):
    """u = Omega n x d: every component (l, m >= 1) turns at Omega and no power_l changes.  Tolerance 10^-6 relative:
    binary32's 6 10^-8 rounding of the velocities with a margin, as the disc tests take it."""
    omega, axis = 0.37, (0.3, -0.5, 0.8)
    _, x = shell_cloud(5, 3000)
    n, e1, e2 = S.frame(axis)
    parts = S.make_parts(x, omega * np.cross(n, x), np.ones(len(x)))
    edges = [0.5, 1.0, 2.5]
    d = as_shell_modes(nb, S.shell_ref(parts, edges, 4, axis, (0.0, 0.0, 0.0), rates=True), edges)
    for l in range(1, 5):
        for m in range(1, l + 1):
            got = d.pattern_speed(l, m)
            assert np.abs(got - omega).max() < 1e-6 * omega, (l, m, got)
    nlm = np.array(S.norms(4))
    a, adot = d.normalised(), nlm * d.rate
    for l in range(5):
        sl = slice(l * l, (l + 1) ** 2)
        power_rate = 2.0 * (a[:, sl] * adot[:, sl]).sum(axis=1) / (2 * l + 1)
        scale = 2.0 * l * omega * (a[:, sl] ** 2).sum(axis=1) / (2 * l + 1)  # what |a| |da/dt| could be
        assert np.all(np.abs(power_rate) <= 1e-6 * scale + 1e-300), (l, power_rate, scale)
    zonal = d.rate[:, [S.index(l, 0) for l in range(5)]]  # m = 0 does not turn: |dQ_l^0 / d zeta| <= 10, |zeta'| ~ 0
    assert np.abs(zonal).max() < 1e-6 * 10.0 * omega * len(x)


def test_pure_expansion_gives_zero_rates():
    """u = d / 2, exact in binary32: no direction changes.  uh = h / 2 exactly and u_r zeta = (r2 / r) (h / r) / 2 is
    within 3 roundings of it, so each of zeta', alpha', beta' is at most 4 2^-53 / 2 and a term of degree l (gradient
    at most l Q(1) per unit of direction, three components) moves by at most 3 l 2 2^-53 Q(1) mu per unit time;
    m_ur is sum mu r / 2 to the same roundings."""
    _, x = shell_cloud(9, 2000)
    parts = S.make_parts(x, 0.5 * x, np.ones(len(x)))
    ref = S.shell_ref(parts, [0.5, 1.0, 2.5], 4, (0.3, -0.5, 0.8), (0.0, 0.0, 0.0), rates=True)
    counts = ref["count"].astype(np.float64)
    for l in range(5):
        for m in range(l + 1):
            tol = 6.0 * l * U * q_at_one(l, m) * counts
            for i in [S.index(l, m)] + ([S.index(l, m, True)] if m else []):
                assert np.all(np.abs(ref["rate"][:, i]) <= tol), (l, m, ref["rate"][:, i], tol)
    assert np.allclose(ref["m_ur"], 0.5 * ref["m_r"], rtol=1e-14, atol=0.0)


# ---- the sums against a brute force ----------------------------------------------------------------------------------
def float_state(seed, n=12000):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, (n, 3)) * [1.0, 0.6, 0.8]
    v = rng.normal(0.0, 1.0, (n, 3))
    mass = 10.0 ** rng.uniform(-3.0, 3.0, n)
    return S.make_parts(x, v, mass)


@pytest.mark.parametrize("lmax,rates", [(6, False), (4, True)])
def test_sums_stay_within_1e10_of_fsum(lmax, rates):
    """Every sum of the restatement against math.fsum of its terms: 1e-10 sum |term|, the disc modes' own bound for
    the three levels."""
    parts = float_state(1)
    edges = [0.0, 0.4, 3.0, 4.0]  # the middle bin holds more than two chunks
    ref = S.shell_ref(parts, edges, lmax, (0.1, 1.0, -0.2), (0.01, 0.02, -0.01), (0.1, 0.0, 0.0), rates=rates)
    assert ref["count"][1] > 2 * S.CHUNK
    nk = (lmax + 1) ** 2
    worst = 0.0
    for k in range(3):
        terms = ref["terms"][ref["key"] == k + 1]
        got = np.concatenate([ref["coef"][k], ref["rate"][k] if rates else [], [ref["m_r"][k], ref["m_ur"][k]]])
        assert terms.shape[1] == len(got) == nk * (2 if rates else 1) + 2
        for f in range(terms.shape[1]):
            exact, scale = math.fsum(terms[:, f]), math.fsum(np.abs(terms[:, f]))
            assert abs(got[f] - exact) <= 1e-10 * scale, (k, f, got[f], exact, scale)
            worst = max(worst, abs(got[f] - exact) / scale if scale else 0.0)
    print(f"worst |sum - fsum| / sum |term| = {worst:.2e}")
    assert ref["inside_count"] + ref["outside_count"] + int(ref["count"].sum()) == len(parts)


def test_a_bins_bits_depend_on_its_members_alone():
    parts = float_state(3, 6000)
    args = ((0.0, 1.0, 0.0), (0.0, 0.0, 0.0))
    a = S.shell_ref(parts, [0.5, 1.0, 2.0], 4, *args)
    b = S.shell_ref(parts, [0.1, 0.2, 0.5, 1.0, 5.0], 4, *args)
    assert a["coef"][0].tobytes() == b["coef"][2].tobytes() and a["count"][0] == b["count"][2]
    assert (a["m_r"][0], a["m_ur"][0]) == (b["m_r"][2], b["m_ur"][2])
    c = S.shell_ref(parts, [0.5, 1.0, 2.0], 2, *args)  # a lower lmax is a prefix
    assert c["coef"][0].tobytes() == a["coef"][0, :9].tobytes()


# ---- through the library, without a device ---------------------------------------------------------------------------
def test_frame_is_map_frame(nb):
    for axis in ((0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.3, -0.5, 0.8), (1.0, 1.0, 1.0)):
        for mine, theirs in zip(S.frame(axis), nb.map_frame(axis)):
            assert mine.tobytes() == theirs.tobytes(), axis


def test_struct_sizes_and_symbols(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    assert C.sizeof(_lib.nb_shell_params) == 96 and C.sizeof(_lib.nb_shell_head) == 200
    assert _lib.SHELL_BIN_DTYPE.itemsize == 24 and _lib.SHELL_DERIVED_DTYPE.itemsize == 232
    assert (_lib.NB_SHELL_MAX_BINS, _lib.NB_SHELL_MAX_L, _lib.NB_SHELL_MAX_L_RATES, _lib.NB_SHELL_CHUNK) == \
        (S.MAX_BINS, S.MAX_L, S.MAX_L_RATES, S.CHUNK) == (256, 6, 4, 4096)
    assert (_lib.NB_SHELL_CENTER_COM, _lib.NB_SHELL_RATES) == (1, 2) and _lib.NB_SHELL_CENTER_COM == _lib.NB_MODES_CENTER_COM
    assert _lib.NB_SHELL_FOUR_PI == S.FOUR_PI == 4.0 * math.pi
    assert (S.MAX_L + 1) ** 2 + 2 <= 64 and 2 * (S.MAX_L_RATES + 1) ** 2 + 2 <= 64 < 2 * (S.MAX_L_RATES + 2) ** 2 + 2
    for name in ("nb_shell_modes_sim", "nb_shell_modes_runner", "nb_shell_modes_derive"):
        assert name in _lib.ABI_SYMBOLS and hasattr(L, name)
    a, b = L.nb_shell_modes_sim.argtypes, L.nb_shell_modes_runner.argtypes
    assert a is not None and a is b  # one list for the two
    assert S.PARTICLE_DTYPE == _lib.PARTICLE_DTYPE
    assert [nb.shell_index(l, m) for l, m in LM] == [S.index(l, m) for l, m in LM]
    assert nb.shell_index(3, 2, sine=True) == S.index(3, 2, True) == 13
    with pytest.raises(ValueError):
        nb.shell_index(2, 3)
    with pytest.raises(ValueError):
        nb.shell_index(2, 0, sine=True)


def test_the_method_is_shared(nb):
    assert nb.Simulator.shell_modes is nb.OfflineHeadless.shell_modes


@pytest.mark.parametrize("lmax,rates", [(0, False), (1, True), (2, False), (4, True), (6, False)])
def test_derive_equals_the_restatement(nb, lmax, rates):
    """Everything but the phase is +, x, / and sqrt alone, the eigen-solver included: to the bit.  atan2 is the C
    library's against Python's: a few units in the last place, the NaNs in the same places."""
    rng = np.random.default_rng(5 + lmax)
    nk = (lmax + 1) ** 2
    coef = rng.normal(0.0, 1.0, (7, nk))
    rate = rng.normal(0.0, 1.0, (7, nk)) if rates else None
    coef[:, 0] = np.abs(coef[:, 0]) + 1.0
    coef[1, 0] = 0.0                      # no mass: relative NaN
    coef[4, 0] = np.nan
    if lmax >= 2:
        coef[2, S.index(2, 2):S.index(2, 2) + 2] = 0.0  # no (2, 2): its phase and speed NaN
    n, e1, e2 = S.frame((0.3, -0.5, 0.8))
    ref = dict(n=0, nonfinite=0, inside_count=0, outside_count=0, inside_mass=0.0, outside_mass=0.0, mass=0.0,
               axis=n, e1=e1, e2=e2, count=np.zeros(7, np.uint64), m_r=np.ones(7), m_ur=np.ones(7), coef=coef,
               rate=rate, lmax=lmax)
    d = as_shell_modes(nb, ref, np.arange(8.0))
    want = S.derive(coef, rate, lmax, n, e1, e2)
    rec, norm, phase, speed = d._derive(norm=True, phase=True, speed=True)
    assert norm.tobytes() == want["norm"].tobytes()
    for name in ("power", "relative", "dipole", "quad_values", "quad_axes"):
        assert np.array_equal(rec[name], want[name], equal_nan=True), (name, rec[name], want[name])
    assert np.array_equal(speed, want["speed"], equal_nan=True)
    assert np.array_equal(np.isnan(phase), np.isnan(want["phase"]))
    assert np.allclose(phase, want["phase"], rtol=1e-15, atol=0.0, equal_nan=True)
    assert np.isnan(rec["relative"][1]).all() and np.isnan(rec["relative"][4]).all()
    assert np.isnan(rec["power"][:, lmax + 1:]).all() and np.isfinite(rec["power"][0, :lmax + 1]).all()
    assert np.array_equal(d.power(), want["power"][:, :lmax + 1], equal_nan=True)
    assert np.isnan(rec["dipole"]).all() == (lmax < 1) and np.isnan(rec["quad_values"][0]).all() == (lmax < 2)
    assert np.isnan(speed).all() if not rates else True
    for l in range(1, lmax + 1):
        for m in range(1, l + 1):
            got = d.phase(l, m)
            assert np.array_equal(got, phase[:, S.index(l, m)], equal_nan=True)
            assert np.all(np.abs(got[np.isfinite(got)]) <= math.pi / m)
            assert np.array_equal(d.coefficient(l, m, sine=True), coef[:, S.index(l, m, True)], equal_nan=True)
            if rates:
                assert np.array_equal(d.pattern_speed(l, m), speed[:, S.index(l, m)], equal_nan=True)
            else:
                with pytest.raises(ValueError):
                    d.pattern_speed(l, m)
    if lmax >= 2:
        assert np.isnan(phase[2, S.index(2, 2)]) and np.isfinite(phase[3, S.index(2, 2)])
    with pytest.raises(ValueError):
        d.phase(lmax + 1, 1)
    with pytest.raises(ValueError):
        d.relative(lmax + 1)


@pytest.mark.parametrize("l,m", [(1, 1), (2, 2), (3, 1), (4, 4)])
@pytest.mark.parametrize("turn", [0.1, -0.2, 2.0, -2.9])
def test_phase_between_recovers_a_rotation(nb, l, m, turn):
    """Two restated clouds, the second turned by `turn` about the polar axis: the phase difference wrapped into
    (-pi/m, pi/m]."""
    axis = (0.0, 1.0, 0.0)
    _, x = shell_cloud(13, 2000)
    n, e1, e2 = S.frame(axis)
    a, b, h = x @ e1, x @ e2, x @ n
    xt = ((a * math.cos(turn) - b * math.sin(turn))[:, None] * e1 + (a * math.sin(turn) + b * math.cos(turn))[:, None] * e2
          + h[:, None] * n)
    edges = [0.5, 2.5]
    first, second = (as_shell_modes(nb, S.shell_ref(S.make_parts(p, np.zeros_like(p), np.ones(len(p))), edges, 4, axis,
                                                    (0.0, 0.0, 0.0)), edges) for p in (x, xt))
    period = 2.0 * math.pi / m
    wrapped = turn - period * math.ceil(turn / period - 0.5)
    assert abs(first.phase_between(second, l, m)[0] - wrapped) < 1e-5  # (binary32 positions, a noisy cloud)


def test_argument_refusals_need_no_device(nb):
    """What is refused before any device call is refused before the handle is looked at: the same messages with no
    simulator at all."""
    from wgpu_n_body_amd import _lib
    L = _lib.lib()

    def call(fn, edges=(0.5, 1.0, 2.0), lmax=4, flags=0, reserved=0, axis=(0.0, 1.0, 0.0), center=(0.0, 0.0, 0.0),
             velocity=(0.0, 0.0, 0.0), nbins=None, params=True, out=True, bins=True, coef=True, null_edges=False):
        e = np.asarray(edges, dtype=np.float64)
        p = _lib.nb_shell_params()
        p.nbins, p.lmax, p.flags, p.reserved = (len(e) - 1 if nbins is None else nbins), lmax, flags, reserved
        for k in range(3):
            p.axis[k], p.center[k], p.velocity[k] = axis[k], center[k], velocity[k]
        p.edges = None if null_edges else e.ctypes.data_as(C.POINTER(C.c_double))
        head = _lib.nb_shell_head()
        b = np.full(8 * 24, 7, np.uint8)
        cf = np.full(128, 7.0)
        rc = fn(None, C.byref(p) if params else None, C.byref(head) if out else None, b.ctypes.data if bins else None,
                cf.ctypes.data if coef else None)
        assert np.all(b == 7) and np.all(cf == 7.0)
        return rc, L.nb_last_error()

    nan, inf = float("nan"), float("inf")
    for fn in (L.nb_shell_modes_sim, L.nb_shell_modes_runner):
        for word, kw in ((b"null params", dict(params=False)), (b"null out", dict(out=False)),
                         (b"null bins", dict(bins=False)), (b"null coef", dict(coef=False)),
                         (b"null edges", dict(null_edges=True)), (b"nbins must be 1..256", dict(nbins=0)),
                         (b"nbins must be 1..256", dict(nbins=257)), (b"lmax must be 0..6", dict(lmax=7)),
                         (b"lmax must be 0..4 with NB_SHELL_RATES", dict(lmax=5, flags=2)),
                         (b"lmax must be 0..4 with NB_SHELL_RATES", dict(lmax=6, flags=3)),
                         (b"unknown flag bits", dict(flags=4)), (b"unknown flag bits", dict(flags=8 | 1)),
                         (b"reserved", dict(reserved=1)),
                         (b"edges[1]", dict(edges=(0.5, 0.5, 2.0))), (b"edges[2]", dict(edges=(0.5, 1.0, 0.9))),
                         (b"edges[0]", dict(edges=(-0.5, 1.0))), (b"edges[1]", dict(edges=(0.5, nan))),
                         (b"edges[1]", dict(edges=(0.5, inf))), (b"center and velocity", dict(center=(0.0, nan, 0.0))),
                         (b"center and velocity", dict(velocity=(inf, 0.0, 0.0))),
                         (b"center and velocity", dict(flags=2, velocity=(inf, 0.0, 0.0))),
                         (b"non-zero finite axis", dict(axis=(0.0, 0.0, 0.0))),
                         (b"non-zero finite axis", dict(axis=(0.0, nan, 0.0))),
                         (b"non-zero finite axis", dict(axis=(1e200, 1e200, 0.0)))):
            rc, msg = call(fn, **kw)
            assert rc == _lib.NB_ERR_INVALID and word in msg, (word, rc, msg)
        for kw in (dict(), dict(flags=1, center=(nan, nan, nan)), dict(lmax=0), dict(lmax=6), dict(lmax=4, flags=2),
                   dict(lmax=4, flags=3, velocity=(nan, 0.0, 0.0))):
            rc, msg = call(fn, **kw)  # good arguments: the handle is what is missing
            assert rc == _lib.NB_ERR_INVALID and (b"null simulator" in msg or b"null runner" in msg), (kw, msg)
    head = _lib.nb_shell_head()
    head.nbins, head.lmax, head.flags = 2, 2, 0
    head.axis[1] = head.e1[0] = 1.0
    head.e2[2] = -1.0
    out = np.zeros(2, _lib.SHELL_DERIVED_DTYPE)
    cf = np.ones((2, 9))
    derive = L.nb_shell_modes_derive
    assert derive(None, cf.ctypes.data, out.ctypes.data, None, None, None) == _lib.NB_ERR_INVALID
    assert derive(C.byref(head), None, out.ctypes.data, None, None, None) == _lib.NB_ERR_INVALID
    assert derive(C.byref(head), cf.ctypes.data, None, None, None, None) == _lib.NB_ERR_INVALID
    assert derive(C.byref(head), cf.ctypes.data, out.ctypes.data, None, None, None) == _lib.NB_OK
    for field, value in (("nbins", 0), ("nbins", 257), ("lmax", 7), ("flags", 4)):
        bad = _lib.nb_shell_head.from_buffer_copy(head)
        setattr(bad, field, value)
        assert derive(C.byref(bad), cf.ctypes.data, out.ctypes.data, None, None, None) == _lib.NB_ERR_INVALID, field
    bad = _lib.nb_shell_head.from_buffer_copy(head)
    bad.lmax, bad.flags = 5, 2
    assert derive(C.byref(bad), cf.ctypes.data, out.ctypes.data, None, None, None) == _lib.NB_ERR_INVALID
