"""The rule of nb_sim_group_shapes (include/nbody.h "Group shapes") restated in numpy, operation by
operation: binary64 from the binary32 state, one rounding per operation, the members of a row in ascending body
index, runs of 64 positions through the butterfly and the runs added in order, and the same cyclic Jacobi as
csrc/nb_shape.hpp.  shape_ref() returns the rows, the per-body selected_of, the stats, `marginal` -- whether any
decision of a row was too close to call for a comparison of integers (|rho2 - 1| < 1e-9 for a member, |delta / tol - 1|
< 1e-6, or lambda_3 / lambda_1 < 1e-12 where the eigenvalues decide) -- and `scale`, the sum of |term| of every sum."""
import functools
import math

import numpy as np

NONE = 0xFFFFFFFF
CONVERGED, UNCONVERGED, DEGENERATE, EMPTY = 1, 2, 4, 8
SWEEPS = 12
FIELDS = 23  # the count and the 22 sums
ROW_DTYPE = np.dtype([("count", "<u4"), ("selected", "<u4"), ("iterations", "<u4"), ("status", "<u4"),
                      ("radius", "<f8"), ("center", "<f8", (3,)), ("velocity", "<f8", (3,)), ("mass", "<f8"),
                      ("md", "<f8", (3,)), ("mu", "<f8", (3,)), ("t", "<f8", (6,)), ("uu", "<f8", (6,)),
                      ("j", "<f8", (3,)), ("lambda", "<f8", (3,)), ("axes", "<f8", (9,)), ("q", "<f8"), ("s", "<f8")])
SUMS = (("mass", 1), ("md", 3), ("mu", 3), ("t", 6), ("uu", 6), ("j", 3))
MARGIN_RHO, MARGIN_DELTA, MARGIN_LAMBDA = 1e-9, 1e-6, 1e-12


def jacobi(t):
    """nb_shape_eigen on Python floats (IEEE binary64, one rounding per operation): (lambda[3], axes[9])."""
    t = [float(x) for x in t]
    a = [[t[0], t[1], t[2]], [t[1], t[3], t[4]], [t[2], t[4], t[5]]]
    v = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(SWEEPS):
        off = (abs(a[0][1]) + abs(a[0][2])) + abs(a[1][2])
        if off == 0.0:
            break
        for p, q in ((0, 1), (0, 2), (1, 2)):
            r = 3 - p - q
            apq = a[p][q]
            if apq == 0.0:
                continue
            g = 100.0 * abs(apq)
            if abs(a[p][p]) + g == abs(a[p][p]) and abs(a[q][q]) + g == abs(a[q][q]):
                a[p][q] = a[q][p] = 0.0
                continue
            h = a[q][q] - a[p][p]
            if abs(h) + g == abs(h):
                tn = apq / h
            else:
                theta = (0.5 * h) / apq
                tn = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
                if theta < 0.0:
                    tn = -tn
            c = 1.0 / math.sqrt(tn * tn + 1.0)
            s = tn * c
            tau = s / (1.0 + c)
            z = tn * apq
            a[p][p] = a[p][p] - z
            a[q][q] = a[q][q] + z
            a[p][q] = a[q][p] = 0.0
            arp, arq = a[r][p], a[r][q]
            a[r][p] = a[p][r] = arp - s * (arq + tau * arp)
            a[r][q] = a[q][r] = arq + s * (arp - tau * arq)
            for k in range(3):
                vp, vq = v[k][p], v[k][q]
                v[k][p] = vp - s * (vq + tau * vp)
                v[k][q] = vq + s * (vp - tau * vq)
    order = [0, 1, 2]
    for i in (1, 2):
        j = i
        while j > 0 and a[order[j]][order[j]] > a[order[j - 1]][order[j - 1]]:
            order[j], order[j - 1] = order[j - 1], order[j]
            j -= 1
    lam, axes = [], []
    for col in order:
        lam.append(a[col][col])
        big = 0
        for j in (1, 2):
            if abs(v[j][col]) > abs(v[big][col]):
                big = j
        flip = v[big][col] < 0.0
        axes += [-v[j][col] if flip else v[j][col] for j in range(3)]
    return np.array(lam), np.array(axes)


def body_ok(state):
    return np.isfinite(state[:, 0:6]).all(axis=1) & np.isfinite(state[:, 9])


def run_sums(terms):
    """(count, F) terms in list order -> (F,): runs of 64 through the butterfly, the runs added in order from 0."""
    count, f = terms.shape
    nruns = (count + 63) // 64
    x = np.zeros((nruns * 64, f))
    x[:count] = terms
    x = x.reshape(nruns, 64, f)
    for o in (32, 16, 8, 4, 2, 1):
        x = x[:, :o] + x[:, o:2 * o]
    total = np.zeros(f)
    for k in range(nruns):
        total = total + x[k, 0]
    return total


def _round(x, v, m, c, vc, radius, q, s, e, reduced):
    """One round over a row's list: the 23 sums, the selection, rho2 and the sum of |term|."""
    with np.errstate(all="ignore"):
        d = x - c
        u = v - vc
        y = [(e[3 * k] * d[:, 0] + e[3 * k + 1] * d[:, 1]) + e[3 * k + 2] * d[:, 2] for k in range(3)]
        ax = (radius, radius * q, radius * s)
        z = [y[k] / ax[k] for k in range(3)]
        rho2 = (z[0] * z[0] + z[1] * z[1]) + z[2] * z[2]
        sel = rho2 <= 1.0
        wm = m
        if reduced:
            wm = np.where(rho2 == 0.0, 0.0, (1.0 / rho2) * m)
        md = m[:, None] * d
        mu = m[:, None] * u
        wd = wm[:, None] * d
        pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
        cols = [np.ones(len(m)), m, md[:, 0], md[:, 1], md[:, 2], mu[:, 0], mu[:, 1], mu[:, 2]]
        cols += [wd[:, i] * d[:, j] for i, j in pairs]
        cols += [mu[:, i] * u[:, j] for i, j in pairs]
        cols += [m * (d[:, 1] * u[:, 2] - d[:, 2] * u[:, 1]), m * (d[:, 2] * u[:, 0] - d[:, 0] * u[:, 2]),
                 m * (d[:, 0] * u[:, 1] - d[:, 1] * u[:, 0])]
        terms = np.where(sel[:, None], np.stack(cols, axis=1), 0.0)
    return run_sums(terms), sel, rho2, np.abs(terms[:, 1:]).sum(axis=0)


def round0(state, group_of, m):
    """The centre and the frame velocity round 0 forms for every row, and what an error of them is measured in:
    (c, V, c_scale, v_scale), each (m, 3); scale = sum |m x| / M."""
    ok = body_ok(state)
    x, v, mass = (state[:, 0:3].astype(np.float64), state[:, 3:6].astype(np.float64), state[:, 9].astype(np.float64))
    out = [np.full((m, 3), np.nan) for _ in range(4)]
    ident = np.eye(3).ravel()
    for r in range(m):
        idx = np.flatnonzero((group_of == r) & ok)
        if len(idx) == 0:
            continue
        sums, _, _, scale = _round(x[idx], v[idx], mass[idx], np.zeros(3), np.zeros(3), np.inf, 1.0, 1.0, ident, False)
        with np.errstate(all="ignore"):
            out[0][r], out[1][r] = sums[2:5] / sums[1], sums[5:8] / sums[1]
            out[2][r], out[3][r] = scale[1:4] / sums[1], scale[4:7] / sums[1]
    return tuple(out)


def shape_ref(state, group_of, m, centers=None, velocities=None, radius=None, reduced=False, max_iter=32, tol=1e-3,
              min_members=10):
    state = np.asarray(state, np.float32)
    group_of = np.asarray(group_of, np.uint32)
    n = len(state)
    assert np.all((group_of == NONE) | (group_of < m))
    ok = body_ok(state)
    x, v, mass = (state[:, 0:3].astype(np.float64), state[:, 3:6].astype(np.float64), state[:, 9].astype(np.float64))
    rows = np.zeros(m, ROW_DTYPE)
    selected_of = np.full(n, NONE, np.uint32)
    marginal = np.zeros(m, bool)
    scale = np.zeros((m, FIELDS - 1))
    rounds = [[] for _ in range(m)]  # (q, s) after every round
    c0 = v0 = None
    if centers is None or velocities is None:
        c0, v0, _, _ = round0(state, group_of, m)
    centers = c0 if centers is None else np.asarray(centers, np.float64).reshape(m, 3)
    velocities = v0 if velocities is None else np.asarray(velocities, np.float64).reshape(m, 3)
    radius = np.full(m, np.inf) if radius is None else np.asarray(radius, np.float64).reshape(m)
    for r in range(m):
        idx = np.flatnonzero((group_of == r) & ok)
        o = rows[r]
        o["count"], o["radius"], o["center"], o["velocity"] = len(idx), radius[r], centers[r], velocities[r]
        o["lambda"], o["axes"], o["q"], o["s"] = np.nan, np.nan, np.nan, np.nan
        if len(idx) == 0:
            o["status"] = EMPTY
            continue
        q, s, e = 1.0, 1.0, np.eye(3).ravel()
        for t in range(1, max_iter + 1):
            sums, sel, rho2, sc = _round(x[idx], v[idx], mass[idx], centers[r], velocities[r], radius[r], q, s, e,
                                         reduced)
            marginal[r] |= bool(np.any(np.abs(rho2 - 1.0) < MARGIN_RHO))
            lam, axes = jacobi(sums[8:14])
            by_count = int(sums[0]) < min_members
            shaped = (not by_count) and lam[2] > 0.0 and bool(np.isfinite(lam).all())
            if not by_count:
                with np.errstate(all="ignore"):
                    marginal[r] |= bool(lam[2] / lam[0] < MARGIN_LAMBDA)
            status, q1, s1 = 0, np.nan, np.nan
            if not shaped:
                status = DEGENERATE
            else:
                q1, s1 = math.sqrt(lam[1] / lam[0]), math.sqrt(lam[2] / lam[0])
                if radius[r] == np.inf:
                    status = CONVERGED
                else:
                    delta = max(abs(q1 - q) / q1, abs(s1 - s) / s1)
                    if t >= 2:
                        marginal[r] |= abs(delta / tol - 1.0) < MARGIN_DELTA
                    if t >= 2 and delta < tol:
                        status = CONVERGED
                    elif t == max_iter:
                        status = UNCONVERGED
            rounds[r].append((q1, s1))
            if status:
                o["selected"], o["iterations"], o["status"] = int(sums[0]), t, status
                at = 1
                for name, k in SUMS:
                    o[name] = sums[at:at + k] if k > 1 else sums[at]
                    at += k
                o["lambda"], o["axes"], o["q"], o["s"] = lam, axes, q1, s1
                scale[r] = sc
                if status in (CONVERGED, UNCONVERGED):
                    selected_of[idx[sel]] = r
                break
            q, s, e = q1, s1, axes
    has = group_of != NONE
    stats = dict(n=n, rows=m, members=int((has & ok).sum()), nonfinite_members=int((has & ~ok).sum()),
                 converged=int((rows["status"] == CONVERGED).sum()), unconverged=int((rows["status"] == UNCONVERGED).sum()),
                 degenerate=int((rows["status"] == DEGENERATE).sum()), empty=int((rows["status"] == EMPTY).sum()),
                 rounds_max=int(rows["iterations"].max()) if m else 0)
    return dict(rows=rows, selected_of=selected_of, stats=stats, marginal=marginal, scale=scale, rounds=rounds)


# ---- the states ---------------------------------------------------------------------------------------
def rotation(rng):
    """A proper rotation, uniformly drawn."""
    a, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(a) < 0:
        a[:, 0] = -a[:, 0]
    return a


def cloud(rng, n, axes=(1.0, 0.7, 0.4), kind="gauss", rot=None, centre=(0.0, 0.0, 0.0), omega=(0.0, 0.0, 0.3),
          sigma_v=0.05, bulk=(0.0, 0.0, 0.0), equal_mass=False):
    """float32[n, 10]: a triaxial Gaussian (sigma = axes) or a uniform ellipsoid (semi-axes = axes), rotated by
    `rot`, moved to `centre`, rotating rigidly with `omega` plus isotropic noise, masses U[0.5, 2]."""
    if kind == "gauss":
        p = rng.normal(size=(n, 3))
    else:
        p = rng.normal(size=(n, 3))
        p *= (rng.uniform(0.0, 1.0, n) ** (1.0 / 3.0) / np.linalg.norm(p, axis=1))[:, None]
    p = p * np.asarray(axes)
    if rot is not None:
        p = p @ rot.T
    s = np.zeros((n, 10), np.float32)
    s[:, 0:3] = p + np.asarray(centre)
    s[:, 3:6] = np.cross(np.asarray(omega), p) + rng.normal(0.0, sigma_v, (n, 3)) + np.asarray(bulk)
    s[:, 9] = 1.0 if equal_mass else rng.uniform(0.5, 2.0, n)
    return s


def assemble(rng, parts, shuffle=True, extra_rows=0, loose=0):
    """(state, group_of, m): part k is row k; `loose` bodies of no row; the body indices shuffled."""
    state = np.concatenate(list(parts) + [cloud(rng, loose, centre=(50.0, 0.0, 0.0))])
    gof = np.concatenate([np.full(len(p), k, np.uint32) for k, p in enumerate(parts)] + [np.full(loose, NONE, np.uint32)])
    if shuffle:
        perm = rng.permutation(len(state))
        state, gof = state[perm], gof[perm]
    return np.ascontiguousarray(state), gof, len(parts) + extra_rows


SIZES = (1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1025)


@functools.lru_cache(maxsize=None)
def case(name):
    """(state, group_of, m, kw): kw are shape_ref's keywords."""
    if name == "six":  # six equal masses on the axes at +-a, +-b, +-c
        a, b, c = 2.0, 1.25, 0.5
        s = np.zeros((6, 10), np.float32)
        s[:, 0:3] = [[a, 0, 0], [-a, 0, 0], [0, b, 0], [0, -b, 0], [0, 0, c], [0, 0, -c]]
        s[:, 9] = 1.0
        return s, np.zeros(6, np.uint32), 1, dict(centers=np.zeros((1, 3)), velocities=np.zeros((1, 3)), min_members=1)
    if name == "coplanar":  # four bodies in the plane z = 0.5 about a centre in it: lambda_3 = 0 exactly
        s = np.zeros((4, 10), np.float32)
        s[:, 0:3] = [[1, 0, 0.5], [-1, 0.25, 0.5], [0, 2, 0.5], [0.5, -2, 0.5]]
        s[:, 9] = 1.0
        return s, np.zeros(4, np.uint32), 1, dict(centers=[[0.0, 0.0, 0.5]], velocities=np.zeros((1, 3)), min_members=1)
    if name == "sizes":  # every run border in one call, R = +inf, device centres; the rows below 5 degenerate by count
        rng = np.random.default_rng(101)
        parts = [cloud(rng, k, rot=rotation(rng), centre=rng.uniform(-5, 5, 3)) for k in SIZES]
        return (*assemble(rng, parts), dict(min_members=5))
    if name == "big":  # one row of 5,000 over many chunks of 64, a finite radius
        rng = np.random.default_rng(111)
        parts = [cloud(rng, 5000, rot=rotation(rng), centre=(0.3, -0.2, 0.1))]
        return (*assemble(rng, parts, loose=37), dict(radius=[2.0]))
    if name in ("mixed", "mixed_reduced"):
        # 0: all inside a wide radius, converged after 2 rounds; 1: a Gaussian cut at R = 2 sigma: 8 rounds (12 reduced);
        # 2: a uniform ellipsoid cut at its own major axis: 20 rounds (30 reduced); 3: too few members: degenerate;
        # 4: R = +inf (reduced: R = 3); 5: no member: empty; 6: a flat cloud that keeps shrinking: 21 rounds, so
        # unconverged at the plain case's max_iter of 20 (27 reduced)
        rng = np.random.default_rng(121)
        parts = [cloud(rng, 300, rot=rotation(rng), centre=(4.0, 0.0, 0.0)),
                 cloud(rng, 2000, axes=(1.0, 0.6, 0.35), rot=rotation(rng), centre=(0.0, 6.0, 0.0)),
                 cloud(rng, 2000, axes=(1.0, 0.7, 0.4), kind="uniform", rot=rotation(rng), centre=(0.0, 0.0, -7.0)),
                 cloud(rng, 5, centre=(-8.0, 0.0, 0.0)),
                 cloud(rng, 700, axes=(1.0, 0.9, 0.8), rot=rotation(rng), centre=(9.0, 9.0, 0.0)),
                 cloud(rng, 0),
                 cloud(rng, 300, axes=(1.0, 0.5, 0.3), rot=rotation(rng), centre=(-3.0, -3.0, 3.0))]
        radius = [100.0, 2.0, 1.0, 1.0, np.inf, 1.0, 1.0]
        kw = dict(radius=radius, max_iter=20)
        if name == "mixed_reduced":
            radius[4] = 3.0
            kw = dict(radius=radius, reduced=True)
        return (*assemble(rng, parts, loose=64), kw)
    if name == "members":  # non-finite members, tracers, a body exactly at the centre, reduced
        rng = np.random.default_rng(131)
        a = cloud(rng, 400, rot=rotation(rng))
        a[rng.choice(400, 50, replace=False), 9] = 0.0  # tracers
        a[7, 0:3] = (0.25, -0.5, 0.125)                 # at the explicit centre: rho2 = 0
        b = cloud(rng, 200, centre=(6.0, 0.0, 0.0))
        b[3, 0], b[4, 4], b[5, 9] = np.nan, np.inf, np.nan
        state, gof, m = assemble(rng, [a, b])
        return state, gof, m, dict(centers=[[0.25, -0.5, 0.125], [6.0, 0.0, 0.0]], velocities=np.zeros((2, 3)),
                                   radius=[1.5, 1.5], reduced=True)
    raise KeyError(name)


# the cases whose integers the GPU tests hold the device to: tests/test_shape.py checks that none has a marginal decision
GPU_CASES = ("sizes", "big", "mixed", "mixed_reduced", "members")


@functools.lru_cache(maxsize=None)
def reference(name):
    state, gof, m, kw = case(name)
    return shape_ref(state, gof, m, **kw)
