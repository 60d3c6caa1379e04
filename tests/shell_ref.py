"""The rule of nb_shell_modes_sim (include/nbody.h "Shell modes") restated in numpy, operation by
operation: binary64 from the binary32 state, one rounding per operation, no contraction, no transcendental.

  frame     n, e1, e2 of nb_map_frame(axis): n the polar axis, phi = 0 along e1
  per body  d = x - c, u = v - v_c; r2 = (dx dx + dy dy) + dz dz; the bin k has edges[k]^2 <= r2 < edges[k + 1]^2
            (below edges[0]^2, and a NaN r2: inside; at or above edges[nbins]^2: outside); r = sqrt(r2);
            h = (dx nx + dy ny) + dz nz, a with e1, b with e2; zeta = h / r, alpha = a / r, beta = b / r;
            c_0 = 1, s_0 = 0, c_m = c_(m-1) alpha - s_(m-1) beta, s_m = s_(m-1) alpha + c_(m-1) beta;
            Q_m^m = (2m - 1)!!, Q_(m-1)^m = 0, Q_l^m = (((2l - 1) zeta) Q_(l-1)^m - (l + m - 1) Q_(l-2)^m) / (l - m);
            C_lm = mu (Q_l^m c_m), S_lm = mu (Q_l^m s_m); once mu r and mu u_r with s = (ux dx + uy dy) + uz dz,
            u_r = s / r; r2 == 0: C_00 = mu, every other term +0
  rates     uh, ua, ub as h, a, b from u; zeta' = (uh - u_r zeta) / r, alpha', beta' likewise;
            c'_m = (c'_(m-1) alpha + c_(m-1) alpha') - (s'_(m-1) beta + s_(m-1) beta'),
            s'_m = (s'_(m-1) alpha + s_(m-1) alpha') + (c'_(m-1) beta + c_(m-1) beta');
            Q'_l^m = ((2l - 1) (zeta' Q_(l-1)^m + zeta Q'_(l-1)^m) - (l + m - 1) Q'_(l-2)^m) / (l - m);
            DC_lm = mu (Q'_l^m c_m + Q_l^m c'_m), DS_lm likewise
  lists     inside, every bin and outside hold their members in ascending body index
  sums      runs of 64 places through the halving butterfly (absent places +0), the runs of a chunk of 4,096 places
            added left to right from +0, the chunks added left to right from +0
  mass      inside + the bins in order + outside
shell_ref() returns a dict with the fields of nb_shell_head, `count`, `m_r`, `m_ur`, `coef` (nbins, (lmax + 1)^2),
`rate` (the same shape, or None), plus `scale`: the sum of |term| behind every entry of coef.  Nothing here comes from
the library; the eigen-solver of derive() is tests/shape_ref.py's restatement of nb_shape_eigen."""
import math

import numpy as np

from tests.shape_ref import jacobi

RUN, CHUNK = 64, 4096
MAX_L, MAX_L_RATES, MAX_BINS = 6, 4, 256
FOUR_PI = float("12.566370614359172")  # the header's literal
PARTICLE_DTYPE = np.dtype([("position", "<f4", (3,)), ("velocity", "<f4", (3,)), ("acceleration", "<f4", (3,)),
                           ("mass", "<f4")])


def index(l, m, sine=False):
    return l * l + ((2 * m - (0 if sine else 1)) if m else 0)


def frame(axis):
    """nb_map_frame: n the unit axis, e1 the coordinate axis of the smallest |n_k| (the lowest index on ties) made
    orthogonal to n, e2 = n x e1."""
    a = [float(x) for x in axis]
    length = math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
    n = [x / length for x in a]
    s = 0
    for k in (1, 2):
        if abs(n[k]) < abs(n[s]):
            s = k
    e1 = [(1.0 if k == s else 0.0) - n[s] * n[k] for k in range(3)]
    el = 0.0
    for k in range(3):
        el += e1[k] * e1[k]
    el = math.sqrt(el)
    e1 = [x / el for x in e1]
    e2 = [n[1] * e1[2] - n[2] * e1[1], n[2] * e1[0] - n[0] * e1[2], n[0] * e1[1] - n[1] * e1[0]]
    return np.array(n), np.array(e1), np.array(e2)


def body_ok(parts):
    return (np.isfinite(parts["position"]).all(axis=1) & np.isfinite(parts["velocity"]).all(axis=1)
            & np.isfinite(parts["mass"]))


def harmonics(zeta, alpha, beta, lmax, dots=None):
    """The recurrences on arrays: ((lmax + 1)^2, k) values Q_l^m c_m and Q_l^m s_m in the order of index(); with
    dots = (zeta', alpha', beta') also their time derivatives (else None)."""
    k = len(zeta)
    nk = (lmax + 1) ** 2
    val = np.zeros((nk, k))
    der = np.zeros((nk, k)) if dots is not None else None
    if dots is not None:
        zeta_d, alpha_d, beta_d = dots
    with np.errstate(all="ignore"):
        cm, sm = np.ones(k), np.zeros(k)
        cd, sd = np.zeros(k), np.zeros(k)
        qmm = 1.0
        for m in range(lmax + 1):
            if m > 1:
                qmm = qmm * float(2 * m - 1)
            q1, q2 = np.zeros(k), np.zeros(k)
            qd1, qd2 = np.zeros(k), np.zeros(k)
            for l in range(m, lmax + 1):
                if l == m:
                    q, qd = np.full(k, qmm), np.zeros(k)
                else:
                    f1, f2, den = float(2 * l - 1), float(l + m - 1), float(l - m)
                    q = ((f1 * zeta) * q1 - f2 * q2) / den
                    if dots is not None:
                        qd = (f1 * (zeta_d * q1 + zeta * qd1) - f2 * qd2) / den
                i = index(l, m)
                val[i] = q * cm
                if m:
                    val[i + 1] = q * sm
                if dots is not None:
                    der[i] = qd * cm + q * cd
                    if m:
                        der[i + 1] = qd * sm + q * sd
                q2, q1 = q1, q
                qd2, qd1 = qd1, qd
            cn, sn = cm * alpha - sm * beta, sm * alpha + cm * beta
            if dots is not None:
                cdn = (cd * alpha + cm * alpha_d) - (sd * beta + sm * beta_d)
                sdn = (sd * alpha + sm * alpha_d) + (cd * beta + cm * beta_d)
                cd, sd = cdn, sdn
            cm, sm = cn, sn
    return val, der


def dot3(p, e):
    return (p[:, 0] * e[0] + p[:, 1] * e[1]) + p[:, 2] * e[2]


def body_terms(x, v, mass, c, vc, n, e1, e2, lmax, rates):
    """x, v (k, 3) and mass (k,) binary32 -> r2 (k,), terms (k, F), F = (lmax + 1)^2 (1 + rates) + 2: the sums,
    their rates, then mu r and mu u_r."""
    nk = (lmax + 1) ** 2
    nf = nk * (2 if rates else 1) + 2
    if len(mass) == 0:
        return np.zeros(0), np.zeros((0, nf))
    with np.errstate(all="ignore"):
        d = x.astype(np.float64) - c
        u = v.astype(np.float64) - vc
        mu = mass.astype(np.float64)
        r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        r = np.sqrt(r2)
        centre = r2 == 0.0
        zeta = np.where(centre, 0.0, dot3(d, n) / r)
        alpha = np.where(centre, 0.0, dot3(d, e1) / r)
        beta = np.where(centre, 0.0, dot3(d, e2) / r)
        ur = np.where(centre, 0.0, ((u[:, 0] * d[:, 0] + u[:, 1] * d[:, 1]) + u[:, 2] * d[:, 2]) / r)
        dots = None
        if rates:
            dots = tuple(np.where(centre, 0.0, (dot3(u, e) - ur * w) / r)
                         for e, w in ((n, zeta), (e1, alpha), (e2, beta)))
        val, der = harmonics(zeta, alpha, beta, lmax, dots)
        terms = np.zeros((len(mu), nf))
        terms[:, :nk] = (mu * val).T
        terms[centre, 1:nk] = 0.0
        if rates:
            terms[:, nk:2 * nk] = (mu * der).T
            terms[centre, nk:2 * nk] = 0.0
        terms[:, nf - 2] = mu * r
        terms[:, nf - 1] = mu * ur
    return r2, terms


def level_sums(terms):
    """(count, F) terms in list order -> (F,): the three fixed levels."""
    count, f = terms.shape
    total = np.zeros(f)
    with np.errstate(all="ignore"):
        for c0 in range(0, count, CHUNK):
            part = terms[c0:c0 + CHUNK]
            nruns = (len(part) + RUN - 1) // RUN
            x = np.zeros((nruns * RUN, f))
            x[:len(part)] = part
            x = x.reshape(nruns, RUN, f)
            for o in (32, 16, 8, 4, 2, 1):
                x = x[:, :o] + x[:, o:2 * o]
            chunk = np.zeros(f)
            for k in range(nruns):
                chunk = chunk + x[k, 0]
            total = total + chunk
    return total


def keys_of(r2, edges):
    """0 inside, k + 1 for bin k, nbins + 1 outside: the number of squared edges at or below r2 (a NaN: none)."""
    e2 = np.asarray(edges, dtype=np.float64) * np.asarray(edges, dtype=np.float64)
    key = np.searchsorted(e2, r2, side="right")
    return np.where(np.isnan(r2), 0, key)


def shell_ref(parts, edges, lmax, axis, center, velocity=(0.0, 0.0, 0.0), rates=False):
    edges = np.asarray(edges, dtype=np.float64)
    nbins = len(edges) - 1
    n, e1, e2 = frame(axis)
    c, vc = np.asarray(center, dtype=np.float64), np.asarray(velocity, dtype=np.float64)
    ok = body_ok(parts)
    idx = np.nonzero(ok)[0]
    r2, terms = body_terms(parts["position"][idx], parts["velocity"][idx], parts["mass"][idx], c, vc, n, e1, e2, lmax,
                           rates)
    key = keys_of(r2, edges)
    nk = (lmax + 1) ** 2
    nf = terms.shape[1]
    sums = [level_sums(terms[key == k]) for k in range(nbins + 2)]       # boolean masks keep the body order
    scale = [level_sums(np.abs(terms[key == k + 1])) for k in range(nbins)]
    count = np.array([(key == k + 1).sum() for k in range(nbins)], dtype=np.uint64)
    mass = sums[0][0]
    for k in range(nbins):
        mass = mass + sums[k + 1][0]
    mass = mass + sums[nbins + 1][0]
    return {
        "n": len(parts), "nonfinite": int(len(parts) - len(idx)),
        "inside_count": int((key == 0).sum()), "outside_count": int((key == nbins + 1).sum()),
        "inside_mass": sums[0][0], "outside_mass": sums[nbins + 1][0], "mass": mass,
        "axis": n, "e1": e1, "e2": e2, "count": count, "lmax": lmax,
        "m_r": np.array([sums[k + 1][nf - 2] for k in range(nbins)]),
        "m_ur": np.array([sums[k + 1][nf - 1] for k in range(nbins)]),
        "coef": np.array([sums[k + 1][:nk] for k in range(nbins)]).reshape(nbins, nk),
        "rate": np.array([sums[k + 1][nk:2 * nk] for k in range(nbins)]).reshape(nbins, nk) if rates else None,
        "scale": np.array([scale[k][:nf - 2] for k in range(nbins)]).reshape(nbins, nf - 2),
        "key": key, "index": idx, "terms": terms,
    }


def norms(lmax):
    """N_lm in the order of index(): sqrt(F) for m = 0 and sqrt((2 F) ((l - m)! / (l + m)!)) with
    F = (2l + 1) / FOUR_PI."""
    out = [0.0] * (lmax + 1) ** 2
    for l in range(lmax + 1):
        f = float(2 * l + 1) / FOUR_PI
        out[l * l] = math.sqrt(f)
        for m in range(1, l + 1):
            out[index(l, m)] = out[index(l, m, True)] = math.sqrt(
                (2.0 * f) * (float(math.factorial(l - m)) / float(math.factorial(l + m))))
    return out


def derive(coef, rate, lmax, n, e1, e2):
    """nb_shell_modes_derive restated on Python floats (math.atan2 is the C library's): a dict of norm, phase, speed
    (nbins, (lmax + 1)^2), power, relative (nbins, 7), dipole (nbins, 3), quad_values (nbins, 3), quad_axes
    (nbins, 3, 3); NaN as the header says."""
    coef = np.asarray(coef, dtype=np.float64)
    nbins, nk = coef.shape
    nlm = norms(lmax)
    nan = float("nan")
    out = {"norm": np.zeros((nbins, nk)), "phase": np.full((nbins, nk), nan), "speed": np.full((nbins, nk), nan),
           "power": np.full((nbins, 7), nan), "relative": np.full((nbins, 7), nan), "dipole": np.full((nbins, 3), nan),
           "quad_values": np.full((nbins, 3), nan), "quad_axes": np.full((nbins, 3, 3), nan)}
    f1, f2, fn = ([float(x) for x in v] for v in (e1, e2, n))
    for k in range(nbins):
        c = [float(x) for x in coef[k]]
        a = [nlm[i] * c[i] for i in range(nk)]
        out["norm"][k] = a
        for l in range(lmax + 1):
            total = a[l * l] * a[l * l]
            for i in range(l * l + 1, (l + 1) ** 2):
                total = total + a[i] * a[i]
            out["power"][k, l] = total / float(2 * l + 1)
        p0 = out["power"][k, 0]
        if p0 != 0.0 and p0 == p0:
            for l in range(lmax + 1):
                q = float(out["power"][k, l]) / float(p0)
                out["relative"][k, l] = np.sqrt(np.float64(q))
        for l in range(1, lmax + 1):
            for m in range(1, l + 1):
                i = index(l, m)
                cc, ss = c[i], c[i + 1]
                p2 = cc * cc + ss * ss
                if p2 == 0.0 or p2 != p2:
                    continue
                out["phase"][k, i] = math.atan2(ss, cc) / float(m)
                if rate is not None:
                    dc, ds = float(rate[k, i]), float(rate[k, i + 1])
                    den = float(m) * p2
                    num = cc * ds - ss * dc
                    with np.errstate(all="ignore"):
                        out["speed"][k, i] = np.float64(num) / np.float64(den)
        if lmax >= 1:
            out["dipole"][k] = [(a[2] * f1[j] + a[3] * f2[j]) + a[1] * fn[j] for j in range(3)]
        if lmax >= 2:
            q0, q1c, q1s, q2c, q2s = (nlm[i] * a[i] for i in range(4, 9))
            t = [[(-0.5 * q0) + 3.0 * q2c, 3.0 * q2s, 1.5 * q1c],
                 [3.0 * q2s, (-0.5 * q0) - 3.0 * q2c, 1.5 * q1s],
                 [1.5 * q1c, 1.5 * q1s, q0]]
            w = [[(f1[i] * t[0][b] + f2[i] * t[1][b]) + fn[i] * t[2][b] for b in range(3)] for i in range(3)]
            m6 = [(w[i][0] * f1[j] + w[i][1] * f2[j]) + w[i][2] * fn[j] for i in range(3) for j in range(i, 3)]
            lam, axes = jacobi(m6)
            out["quad_values"][k] = lam
            out["quad_axes"][k] = axes.reshape(3, 3)
    return out


def make_parts(x, v, mass):
    """A read_particles-shaped record array from positions, velocities and masses (rounded to binary32)."""
    parts = np.zeros(len(mass), dtype=PARTICLE_DTYPE)
    parts["position"] = np.asarray(x, dtype=np.float32)
    parts["velocity"] = np.asarray(v, dtype=np.float32)
    parts["mass"] = np.asarray(mass, dtype=np.float32)
    return parts
