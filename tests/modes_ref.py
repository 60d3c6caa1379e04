"""The rule of nb_disc_modes_sim (include/nbody.h "Disc modes") restated in numpy, operation by
operation: binary64 from the binary32 state, one rounding per operation, no contraction.

  frame     n, e1, e2 of nb_map_frame(axis)
  per body  d = x - c, u = v - v_c; h = (dx nx + dy ny) + dz nz; p = d - h n; r2 = (px px + py py) + pz pz;
            the bin k has edges[k]^2 <= r2 < edges[k + 1]^2 (below edges[0]^2, and a NaN r2: inside; at or above
            edges[nbins]^2: outside); a = (px e1x + py e1y) + pz e1z, b with e2, ua and ub likewise from u;
            R = sqrt(r2), c_1 = a / R, s_1 = b / R, w = (a ub - b ua) / r2, all three 0 where r2 == 0;
            c_0 = 1, s_0 = 0, c_m = c_(m-1) c_1 - s_(m-1) s_1, s_m = s_(m-1) c_1 + c_(m-1) s_1;
            per m: C = mu c_m, S = mu s_m, DC = (mu w) c_m, DS = (mu w) s_m, ZC = (mu h) c_m, ZS = (mu h) s_m;
            once: mu R and (mu h) h
  lists     inside, every bin and outside hold their members in ascending body index
  sums      runs of 64 places through the halving butterfly (absent places +0), the runs of a chunk of 4,096 places
            added left to right from +0, the chunks added left to right from +0
  mass      inside + the bins in order + outside
modes_ref() returns a dict with the fields of nb_modes_head, `count`, `m_r`, `m_h2` and `modes` (nbins, mmax + 1, 6),
plus `scale`: the sum of |term| behind every entry of `modes` (for the brute-force comparison)."""
import math

import numpy as np

FIELDS = 6
RUN, CHUNK = 64, 4096
MAX_M, MAX_BINS = 8, 256


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


def recurrence(c1, s1, mmax):
    """[(c_m, s_m) for m = 0 .. mmax]"""
    cm, sm = np.ones_like(c1), np.zeros_like(c1)
    out = []
    for _ in range(mmax + 1):
        out.append((cm, sm))
        cm, sm = cm * c1 - sm * s1, sm * c1 + cm * s1
    return out


def body_terms(x, v, mass, c, vc, n, e1, e2, mmax):
    """x, v (k, 3) and mass (k,) binary32 -> r2 (k,), terms (k, 6 (mmax + 1) + 2): the modes, then mu R and
    (mu h) h."""
    with np.errstate(all="ignore"):
        d = x.astype(np.float64) - c
        u = v.astype(np.float64) - vc
        mu = mass.astype(np.float64)
        h = (d[:, 0] * n[0] + d[:, 1] * n[1]) + d[:, 2] * n[2]
        p = [d[:, k] - h * n[k] for k in range(3)]
        r2 = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]
        a = (p[0] * e1[0] + p[1] * e1[1]) + p[2] * e1[2]
        b = (p[0] * e2[0] + p[1] * e2[1]) + p[2] * e2[2]
        ua = (u[:, 0] * e1[0] + u[:, 1] * e1[1]) + u[:, 2] * e1[2]
        ub = (u[:, 0] * e2[0] + u[:, 1] * e2[1]) + u[:, 2] * e2[2]
        big_r = np.sqrt(r2)
        zero = r2 == 0.0
        c1 = np.where(zero, 0.0, a / big_r)
        s1 = np.where(zero, 0.0, b / big_r)
        w = np.where(zero, 0.0, (a * ub - b * ua) / r2)
        muw, muh = mu * w, mu * h
        cols = []
        for cm, sm in recurrence(c1, s1, mmax):
            cols += [mu * cm, mu * sm, muw * cm, muw * sm, muh * cm, muh * sm]
        cols += [mu * big_r, muh * h]
    return r2, np.stack(cols, axis=1) if len(r2) else np.zeros((0, FIELDS * (mmax + 1) + 2))


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


def modes_ref(parts, edges, mmax, axis, center, velocity=(0.0, 0.0, 0.0)):
    edges = np.asarray(edges, dtype=np.float64)
    nbins = len(edges) - 1
    n, e1, e2 = frame(axis)
    c, vc = np.asarray(center, dtype=np.float64), np.asarray(velocity, dtype=np.float64)
    ok = body_ok(parts)
    idx = np.nonzero(ok)[0]
    r2, terms = body_terms(parts["position"][idx], parts["velocity"][idx], parts["mass"][idx], c, vc, n, e1, e2, mmax)
    key = keys_of(r2, edges)
    nf = FIELDS * (mmax + 1)
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
        "axis": n, "e1": e1, "e2": e2, "count": count,
        "m_r": np.array([sums[k + 1][nf] for k in range(nbins)]),
        "m_h2": np.array([sums[k + 1][nf + 1] for k in range(nbins)]),
        "modes": np.array([sums[k + 1][:nf] for k in range(nbins)]).reshape(nbins, mmax + 1, FIELDS),
        "scale": np.array([scale[k][:nf] for k in range(nbins)]).reshape(nbins, mmax + 1, FIELDS),
        "key": key, "index": idx, "terms": terms,
    }


def derive(modes, m):
    """nb_disc_modes_derive restated on Python floats (math.hypot and math.atan2 are the C library's): amplitude,
    phase, pattern_speed, bend_amplitude, bend_phase per bin."""
    modes = np.asarray(modes, dtype=np.float64)
    out = np.full((5, len(modes)), np.nan)
    for k in range(len(modes)):
        c0 = float(modes[k, 0, 0])
        c, s, dc, ds, zc, zs = (float(modes[k, m, f]) for f in range(FIELDS))
        if c0 == 0.0 or c0 != c0:
            continue
        p2, z2 = c * c + s * s, zc * zc + zs * zs
        out[0, k] = math.hypot(c, s) / c0
        out[3, k] = math.hypot(zc, zs) / c0
        if p2 != 0.0:
            out[1, k] = math.atan2(s, c) / float(m)
            out[2, k] = (c * dc + s * ds) / p2
        if z2 != 0.0:
            out[4, k] = math.atan2(zs, zc) / float(m)
    return tuple(out)


def make_parts(x, v, mass):
    """A read_particles-shaped record array from positions, velocities and masses (rounded to binary32)."""
    from wgpu_n_body_amd import PARTICLE_DTYPE
    parts = np.zeros(len(mass), dtype=PARTICLE_DTYPE)
    parts["position"] = np.asarray(x, dtype=np.float32)
    parts["velocity"] = np.asarray(v, dtype=np.float32)
    parts["mass"] = np.asarray(mass, dtype=np.float32)
    return parts


def ring(n_bodies=360, radius=1.0, eps=0.25, phi0=0.3, omega0=1.7, axis=(0.0, 1.0, 0.0), alpha=0.0, beta=0.0, m=2):
    """n_bodies at phi_k = 2 pi k / n on one radius of the plane of `axis`, masses 1 + eps cos m (phi_k - phi0),
    velocities omega0 n x d, lifted to h = R (alpha cos phi + beta sin phi); everything rounded to binary32."""
    n, e1, e2 = frame(axis)
    phi = 2.0 * np.pi * np.arange(n_bodies) / n_bodies
    h = radius * (alpha * np.cos(phi) + beta * np.sin(phi))
    d = radius * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2) + h[:, None] * n
    v = omega0 * np.cross(n, d)
    return make_parts(d, v, 1.0 + eps * np.cos(m * (phi - phi0)))
