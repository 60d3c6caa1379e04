"""The unbinding rule of include/nbody.h ("Bound groups") restated in numpy binary64, and the states
the tests run it on.  psi comes from tests/diag_ref.psi64, the groups from tests/fof_ref.  bound_ref returns
everything nb_sim_bound returns and, per group, how many of the rule's decisions were marginal -- within four
times the device's stated error of zero -- and the worst margin; only a case without a marginal decision pins
the device's integers.

The states are float32[n, 10] (px py pz vx vy vz ax ay az mass), as everywhere in tests/."""
import functools

import numpy as np

from tests import fof_ref
from tests.diag_ref import psi64

NONE = 0xFFFFFFFF
CONVERGED, DISSOLVED, UNCONVERGED, SKIPPED = 1, 2, 4, 8
S_BOUND = 5e-6       # |S_i - S_i(64)| <= S_BOUND * sum_j |m_j| psi(r_ij)   (include/nbody.h)
ROUNDING = 1e-12     # ... and the binary64 rounding of k_i, V and the sums, times k_i + |V|^2
ROW_DTYPE = np.dtype([("label", "<u4"), ("count", "<u4"), ("bound_count", "<u4"), ("iterations", "<u4"),
                      ("status", "<u4"), ("most_bound", "<u4"), ("mass", "<f8"), ("mx", "<f8", (3,)),
                      ("mv", "<f8", (3,)), ("mr2", "<f8"), ("kinetic", "<f8"), ("potential", "<f8"),
                      ("phi_min", "<f8"), ("kinetic0", "<f8"), ("potential0", "<f8")])


def coupling(g, dt):
    return np.float64(np.float32(g)) * np.float64(np.float32(dt))


def _pair_sums(x, m, act, e, psi_cache):
    """S_i = sum_{j active, j != i} m_j psi(r_ij) and the same with |m_j|, for every i (float64[count])."""
    n = len(m)
    w = np.where(act, m, 0.0)
    s, sabs = np.zeros(n), np.zeros(n)
    rows = max(1, (1 << 22) // max(n, 1))
    for i0 in range(0, n, rows):
        i1 = min(n, i0 + rows)
        key = (i0, i1)
        if key not in psi_cache:
            d = x[None, :, :] - x[i0:i1, None, :]
            r = np.sqrt((d * d).sum(axis=2))
            p = psi64(r.ravel(), e).reshape(r.shape)
            p[np.arange(i0, i1) - i0, np.arange(i0, i1)] = 0.0  # excluded by index
            if n <= 2048:
                psi_cache[key] = p
        else:
            p = psi_cache[key]
        with np.errstate(invalid="ignore"):
            t = w[None, :] * p
        t = np.where(w[None, :] == 0.0, 0.0, t)  # a massless or removed j adds 0, also at distance 0 with e = 0
        s[i0:i1] = t.sum(axis=1)
        sabs[i0:i1] = np.abs(t).sum(axis=1)
    return s, sabs


def unbind(x, v, m, c, e, min_bound, max_iter):
    """One group (float64 arrays in list order).  dict: active (bool, the bound set), energy, phi, tol (the
    device's stated error of energy), iterations, status, v_last, kinetic0, potential0, marginal, margin."""
    n = len(m)
    act = np.ones(n, bool)
    energy, phi, tol = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    out = dict(iterations=0, status=0, v_last=np.zeros(3), kinetic0=np.nan, potential0=np.nan, marginal=0,
               margin=np.inf)
    cache = {}
    t = 0
    while True:
        t += 1
        big_m = m[act].sum()
        if not big_m > 0:
            out["status"] = DISSOLVED
            act[:] = False
            break
        big_v = (m[act, None] * v[act]).sum(axis=0) / big_m
        s, sabs = _pair_sums(x, m, act, e, cache)
        ph = -(c * s)
        u = v - big_v
        k = 0.5 * ((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])
        en = k + ph
        err = S_BOUND * c * sabs + ROUNDING * (k + (big_v * big_v).sum())
        energy[act], phi[act], tol[act] = en[act], ph[act], err[act]
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.abs(en[act]) / (4.0 * err[act])
        # a member at rest in the group's frame with nobody to attract it (a group of one body at rest) has
        # e = 0 + -0 with no rounding anywhere: exact on every implementation of the rule, so decisive
        ratio[(err[act] == 0.0) & (en[act] == 0.0)] = np.inf
        out["marginal"] += int((~(ratio > 1.0)).sum())
        out["margin"] = min(out["margin"], float(np.min(np.where(np.isnan(ratio), 0.0, ratio))))
        out["iterations"], out["v_last"] = t, big_v
        if t == 1:
            out["kinetic0"], out["potential0"] = (m * k).sum(), 0.5 * (m * ph).sum()
        leave = act & (en > 0)
        if not leave.any():
            out["status"] = CONVERGED
            break
        act &= ~leave
        if act.sum() < min_bound:
            out["status"] = DISSOLVED
            act[:] = False
            break
        if t == max_iter:
            out["status"] = UNCONVERGED
            break
    out.update(active=act, energy=energy, phi=phi, tol=tol)
    return out


def bound_ref(state, g, e, dt, link, min_members=20, min_bound=None, max_iter=32, max_group=262144, capacity=None):
    """Everything nb_sim_bound returns, as a dict: group_of, bound_of, energy, energy_tol, phi (per body), rows
    (ROW_DTYPE), scale (the sums of |term| of mass, mx, mv, mr2, kinetic, potential per row), the stats by name,
    and marginal / margin per row."""
    state = np.asarray(state, np.float32)
    n = state.shape[0]
    min_bound = min_members if min_bound is None else min_bound
    f = fof_ref.fof_grid(state, link, min_members) if n else fof_ref.catalogue(state, np.zeros(0, np.uint32), link, 1)
    groups = f["groups"]
    rows_n = groups if capacity is None else min(groups, capacity)
    c, e64 = coupling(g, dt), np.float64(np.float32(e))
    s64 = state.astype(np.float64)
    bound_of = np.full(n, NONE, np.uint32)
    energy, energy_tol, phi = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    rows = np.zeros(rows_n, ROW_DTYPE)
    scale = np.zeros((rows_n, 10))
    marginal, margin = np.zeros(rows_n, np.int64), np.full(rows_n, np.inf)
    pairs = 0
    for r in range(rows_n):
        members = np.flatnonzero(f["group_of"] == r)  # ascending body index
        row = rows[r]
        row["label"], row["count"] = f["rows_label"][r], f["rows_count"][r]
        row["most_bound"] = NONE
        row["phi_min"] = row["kinetic0"] = row["potential0"] = np.nan
        if max_group and len(members) > max_group:
            row["status"] = SKIPPED
            continue
        x, v, m = s64[members, 0:3], s64[members, 3:6], s64[members, 9]
        u = unbind(x, v, m, c, e64, min_bound, max_iter)
        row["iterations"], row["status"] = u["iterations"], u["status"]
        row["kinetic0"], row["potential0"] = u["kinetic0"], u["potential0"]
        energy[members], energy_tol[members], phi[members] = u["energy"], u["tol"], u["phi"]
        marginal[r], margin[r] = u["marginal"], u["margin"]
        pairs += u["iterations"] * len(members) * (len(members) - 1)
        b = u["active"]
        if u["status"] in (CONVERGED, UNCONVERGED) and b.any():
            bound_of[members[b]] = r
            mb, xb, vb, pb = m[b], x[b], v[b], u["phi"][b]
            w = vb - u["v_last"]
            kb = 0.5 * ((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
            terms = np.concatenate([mb[:, None], mb[:, None] * xb, mb[:, None] * vb,
                                    (mb * ((xb[:, 0] * xb[:, 0] + xb[:, 1] * xb[:, 1]) + xb[:, 2] * xb[:, 2]))[:, None],
                                    (mb * kb)[:, None], (0.5 * mb * pb)[:, None]], axis=1)
            tot = terms.sum(axis=0)
            scale[r] = np.abs(terms).sum(axis=0)
            row["bound_count"] = int(b.sum())
            row["mass"], row["mx"], row["mv"], row["mr2"] = tot[0], tot[1:4], tot[4:7], tot[7]
            row["kinetic"], row["potential"] = tot[8], tot[9]
            row["phi_min"] = pb.min()
            row["most_bound"] = members[b][np.flatnonzero(pb == pb.min())[0]]
    live = rows["bound_count"] > 0
    return dict(n=n, nonfinite=f["nonfinite"], components=f["components"], groups=groups,
                grouped_bodies=f["grouped_bodies"], largest_count=f["largest_count"], largest_label=f["largest_label"],
                labels=f["labels"], group_of=f["group_of"], bound_of=bound_of, energy=energy, energy_tol=energy_tol,
                phi=phi, rows=rows, scale=scale, marginal=marginal, margin=margin,
                bound_groups=int(live.sum()), bound_bodies=int(rows["bound_count"].sum()),
                dissolved=int((rows["status"] == DISSOLVED).sum()), unconverged=int((rows["status"] == UNCONVERGED).sum()),
                skipped=int((rows["status"] == SKIPPED).sum()),
                rounds_max=int(rows["iterations"].max()) if rows_n else 0, pairs=int(pairs))


# ---- the states ---------------------------------------------------------------------------------------
G, DT, E = 6.25e-5, 0.016, 1e-4  # c = g dt = 1e-6 (as binary32 rounds them)


def _ball(rng, n, radius, centre):
    d = rng.normal(size=(n, 3))
    d *= (radius * rng.uniform(0.0, 1.0, n) ** (1.0 / 3.0) / np.linalg.norm(d, axis=1))[:, None]
    return d + np.asarray(centre)


def clump(rng, n, radius, centre, heat, e=E, bulk=(0.0, 0.0, 0.0), m_lo=0.5):
    """float32[n, 10]: a ball of n bodies, masses U[m_lo, 2], velocities N(0, sigma) about `bulk` with
    sigma = heat * sqrt(median(c S_i)): heat 0.6 sheds a sixth of a large ball and settles, 1.0 boils it away."""
    s = np.zeros((n, 10), np.float32)
    s[:, 0:3] = _ball(rng, n, radius, centre)
    s[:, 9] = rng.uniform(m_lo, 2.0, n)
    if n > 1:
        x, m = s[:, 0:3].astype(np.float64), s[:, 9].astype(np.float64)
        some = np.arange(min(n, 256))  # (the median over the first 256 members: the ball is the same everywhere)
        d = x[None, :, :] - x[some, None, :]
        psi = psi64(np.sqrt((d * d).sum(axis=2)).ravel(), np.float64(np.float32(e))).reshape(len(some), n)
        psi[some, some] = 0.0
        sigma = heat * np.sqrt(np.median(coupling(G, DT) * (m[None, :] * psi).sum(axis=1)))
    else:
        sigma = 0.0
    s[:, 3:6] = rng.normal(0.0, 1.0, (n, 3)) * sigma + np.asarray(bulk)
    return s


def _grid_centres(count, spacing):
    side = int(np.ceil(count ** (1.0 / 3.0)))
    k = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)[:count]
    return (k - (side - 1) / 2.0) * spacing


SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1025)


@functools.lru_cache(maxsize=None)
def case(name):
    """(state, params): params are bound_ref's keywords (g, e, dt, link, ...)."""
    p = dict(g=G, e=E, dt=DT)
    if name == "two_at_rest":
        s = np.zeros((2, 10), np.float32)
        s[1, 0] = 0.1
        s[:, 9] = 1.0
        return s, dict(p, link=0.2, min_members=2, min_bound=2)
    if name == "two_fast":  # a relative speed far above sqrt(2 c m psi(r)) sqrt(2): both leave
        s = np.zeros((2, 10), np.float32)
        s[1, 0] = 0.1
        s[:, 9] = 1.0
        s[0, 3], s[1, 3] = -1.0, 1.0
        return s, dict(p, link=0.2, min_members=2, min_bound=1)
    if name == "interloper":  # a cold clump and one fast body passing through it
        rng = np.random.default_rng(11)
        s = clump(rng, 100, 0.05, (0.0, 0.0, 0.0), 0.2)
        fast = np.zeros((1, 10), np.float32)
        fast[0, 0:3], fast[0, 3], fast[0, 9] = (0.01, 0.0, 0.0), 1.0, 1.0
        return np.concatenate([s[:50], fast, s[50:]]), dict(p, link=0.2, min_members=20)
    if name == "sizes":  # every tile border: one ball per size, far more than link apart, all members friends
        rng = np.random.default_rng(21)
        link = 0.2
        parts = [clump(rng, k, link / 4, c, heat)
                 for k, c, heat in zip(SIZES, _grid_centres(len(SIZES), 10 * link), (0, 0.3, 0.6, 0.6, 0.6, 0.6, 1.0, 0.6, 0.6))]
        return np.concatenate(parts), dict(p, link=link, min_members=1, min_bound=1)
    if name in ("fates", "fates_two_rounds"):  # 300 clumps of 20-70 bodies and one of 5,000, the indices shuffled
        rng = np.random.default_rng(31)
        link = 0.02
        centres = _grid_centres(301, 10 * link)
        sizes = rng.integers(20, 71, 300)
        heats = (0.3, 0.6, 0.8, 1.2)
        parts = [clump(rng, int(k), link / 4, centres[i], heats[i % 4], bulk=rng.normal(0, 0.05, 3))
                 for i, k in enumerate(sizes)]
        parts.append(clump(rng, 5000, link / 4, centres[300], 0.6))
        s = np.concatenate(parts)
        return s[rng.permutation(len(s))], dict(p, link=link, min_members=20, min_bound=10, max_group=4000,
                                                max_iter=2 if name == "fates_two_rounds" else 32)
    if name == "members":  # non-finite bodies, massless and coincident members, bodies of no group
        rng = np.random.default_rng(41)
        link = 0.1
        a = clump(rng, 300, link / 4, (0.0, 0.0, 0.0), 0.6)
        b = clump(rng, 120, link / 4, (2.0, 0.0, 0.0), 0.5)
        a[rng.choice(300, 40, replace=False), 9] = 0.0      # tracers
        a[200:210, 0:3] = a[100:110, 0:3]                   # ten pairs at the same coordinates
        b[60:64, 0:3] = b[0, 0:3]                           # five at one point
        bad = clump(rng, 6, link / 4, (0.0, 0.0, 0.0), 0.0)
        bad[0, 0], bad[1, 4], bad[2, 9] = np.nan, np.inf, np.nan
        bad[3:, 0:3] = rng.uniform(5.0, 9.0, (3, 3))        # far singletons: of no group
        s = np.concatenate([a, bad, b])
        return s[rng.permutation(len(s))], dict(p, link=link, min_members=5, min_bound=3)
    if name == "e0":  # no softening, no coincidences
        rng = np.random.default_rng(51)
        s = np.concatenate([clump(rng, 300, 0.05, (0.0, 0.0, 0.0), 0.6, e=0.0),
                            clump(rng, 70, 0.05, (3.0, 0.0, 0.0), 0.9, e=0.0)])
        s[5, 9] = 0.0
        return s[rng.permutation(len(s))], dict(p, e=0.0, link=0.2, min_members=20, min_bound=5)
    if name == "cascade":  # the hot ball: sheds a sixth in round 1 and settles in 7-11 rounds
        rng = np.random.default_rng(61)
        return clump(rng, 1500, 0.2, (0.1, -0.2, 0.3), 0.6), dict(p, link=0.4, min_members=20)
    if name == "ball4096":  # one group equal to the whole state
        rng = np.random.default_rng(71)
        return clump(rng, 4096, 0.2, (0.0, 0.0, 0.0), 0.5), dict(p, link=0.4, min_members=20)
    raise KeyError(name)


# the cases whose integers the GPU tests hold the device to: tests/test_bound.py checks that none has a marginal decision
GPU_CASES = ("two_at_rest", "two_fast", "interloper", "sizes", "fates", "fates_two_rounds", "members", "e0", "cascade")


@functools.lru_cache(maxsize=None)
def reference(name, capacity=None):
    state, params = case(name)
    return bound_ref(state, capacity=capacity, **params)
