"""The halo-profile rule of include/nbody.h ("Halo profiles"), restated in numpy from the header
text.  The sums come from brute force: every counted body against every centre, no cells -- so a body the
device's grid dropped shows as a count that differs.  The grid is restated separately (grid64, cells64,
axis_range64, candidates64), only to predict the integers of nb_halo_stats.  binary64 from the binary32 state,
one rounding per operation (numpy never contracts).  Used by tests/test_halo.py and tests/test_halo_gpu.py."""
import numpy as np

MAX_BINS, MAX_CENTERS, MAX_ROWS = 64, 1 << 20, 1 << 22
MAX_CELLS, CHUNK, EXTRA_ITEMS = 1024, 4096, 1 << 16
SPHERE = float("4.1887902047863909846")  # NB_KNN_SPHERE
CENTER_NONFINITE = 1
SUMS = ("mass", "m_r", "m_ur", "m_ur2", "m_u2", "ang")


def split(state):
    """x, v, m in binary64 and the mask of the bodies that count."""
    state = np.asarray(state, dtype=np.float32).reshape(-1, 10)
    x, v, m = state[:, 0:3].astype(np.float64), state[:, 3:6].astype(np.float64), state[:, 9].astype(np.float64)
    return x, v, m, np.isfinite(x).all(1) & np.isfinite(v).all(1) & np.isfinite(m)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


# ---- the grid: only what nb_halo_stats reports depends on it ------------------------------------------------
def grid64(state, edges):
    x, _, _, ok = split(state)
    edges = np.asarray(edges, dtype=np.float64)
    g = dict(n_ok=int(ok.sum()), r2max=edges[-1] * edges[-1], h=edges[-1], cells=(1, 1, 1),
             lo=np.zeros(3), hi=np.zeros(3))
    if g["n_ok"]:
        lo, hi = x[ok].min(0), x[ok].max(0)
        h = max(edges[-1], (hi - lo).max() * 2.0 ** -10)
        cells = tuple(int(min(MAX_CELLS, np.floor((hi[a] - lo[a]) / h) + 1.0)) for a in range(3))
        g.update(lo=lo, hi=hi, h=h, cells=cells)
    return g


def lower_edges(g, a):
    """e(q) = lo + (double)q h for q = 0 .. cells - 1 of axis a."""
    return g["lo"][a] + np.arange(g["cells"][a], dtype=np.float64) * g["h"]


def cells64(g, x):
    """(n, 3): per axis the largest q with e(q) <= x (0 when there is none)."""
    return np.stack([np.maximum(np.searchsorted(lower_edges(g, a), x[:, a], side="right") - 1, 0)
                     for a in range(3)], axis=1)


def axis_range64(g, a, c):
    """(t0, t1), the cells of axis a a centre at coordinate c looks at, or None."""
    lo, hi, r2max = g["lo"][a], g["hi"][a], g["r2max"]
    with np.errstate(over="ignore", invalid="ignore"):
        if (c >= hi and (c - hi) * (c - hi) >= r2max) or (lo >= c and (lo - c) * (lo - c) >= r2max):
            return None
        e = lower_edges(g, a)
        last = e.shape[0] - 1
        below = (c >= e) & ((c - e) * (c - e) >= r2max)
        below[0] = True
        up = np.append(e[1:], np.inf)
        above = (up >= c) & ((up - c) * (up - c) >= r2max)
        above[last] = True
    t0, t1 = int(np.flatnonzero(below).max()), int(np.flatnonzero(above).min())
    return (t0, t1) if t0 <= t1 else None


def candidates64(state, edges, centers):
    """T per centre: the counted bodies of the cells the centre looks at."""
    x, _, _, ok = split(state)
    g = grid64(state, edges)
    centers = np.asarray(centers, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(centers.shape[0], dtype=np.int64)
    if not g["n_ok"] or not g["r2max"] > 0.0:
        return out
    q = cells64(g, x[ok])
    for j, c in enumerate(centers):
        if not np.isfinite(c).all():
            continue
        rng = [axis_range64(g, a, c[a]) for a in range(3)]
        if any(r is None for r in rng):
            continue
        sel = np.ones(q.shape[0], dtype=bool)
        for a in range(3):
            sel &= (q[:, a] >= rng[a][0]) & (q[:, a] <= rng[a][1])
        out[j] = sel.sum()
    return out


# ---- the rule ---------------------------------------------------------------------------------------------
def halo_ref(state, edges, centers=None, bodies=None, velocities=None):
    """Returns a dict: count (m, nbins) and the SUMS as (m, nbins[, 3]) arrays, inside_count, inside_mass, center,
    velocity, flags per centre, the integers of nb_halo_stats, and under "scale" the sum of |term| of every sum."""
    x, v, m, ok = split(state)
    n = x.shape[0]
    edges = np.asarray(edges, dtype=np.float64)
    nbins = edges.shape[0] - 1
    e2 = edges * edges
    if centers is not None:
        c = np.asarray(centers, dtype=np.float64).reshape(-1, 3)
        vc = np.zeros_like(c) if velocities is None else np.asarray(velocities, dtype=np.float64).reshape(-1, 3)
        flags = np.zeros(c.shape[0], dtype=np.uint32)
    else:
        bodies = np.asarray(bodies, dtype=np.int64).reshape(-1)
        c = x[bodies]
        vc = v[bodies] if velocities is None else np.asarray(velocities, dtype=np.float64).reshape(-1, 3).copy()
        flags = np.where(ok[bodies], 0, CENTER_NONFINITE).astype(np.uint32)
        c = np.where(flags[:, None] != 0, 0.0, c)
        vc = np.where(flags[:, None] != 0, 0.0, vc)
    mc = c.shape[0]
    xs, vs, ms = x[ok], v[ok], m[ok]
    out = dict(count=np.zeros((mc, nbins), np.uint64), inside_count=np.zeros(mc, np.uint32),
               inside_mass=np.zeros(mc), center=c, velocity=vc, flags=flags)
    scale = dict(inside_mass=np.zeros(mc))
    for name in SUMS:
        shape = (mc, nbins, 3) if name == "ang" else (mc, nbins)
        out[name], scale[name] = np.zeros(shape), np.zeros(shape)
    for j in range(mc):
        if flags[j] or not xs.shape[0]:
            continue
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            d, u = xs - c[j], vs - vc[j]
            r2 = _dot(d, d)
            cnt = np.searchsorted(e2, r2, side="right")  # edges at or below r2
            inside = cnt == 0
            binned = (cnt >= 1) & (cnt <= nbins)
            if not binned.any() and not inside.any():
                continue
            d, u, r2, mm, k = d[binned], u[binned], r2[binned], ms[binned], cnt[binned] - 1
            r = np.sqrt(r2)
            zero = r2 == 0.0
            ur = np.where(zero, 0.0, _dot(d, u) / np.where(zero, 1.0, r))
            terms = {"mass": mm, "m_r": mm * r, "m_ur": mm * ur, "m_ur2": (mm * ur) * ur, "m_u2": mm * _dot(u, u),
                     "ang": mm[:, None] * _cross(d, u)}
        out["count"][j] = np.bincount(k, minlength=nbins)
        out["inside_count"][j] = inside.sum()
        out["inside_mass"][j] = ms[inside].sum()
        scale["inside_mass"][j] = np.abs(ms[inside]).sum()
        for name in SUMS:
            t = terms[name]
            if t.ndim == 2:
                for a in range(3):
                    out[name][j, :, a] = np.bincount(k, weights=t[:, a], minlength=nbins)
                    scale[name][j, :, a] = np.bincount(k, weights=np.abs(t[:, a]), minlength=nbins)
            else:
                out[name][j] = np.bincount(k, weights=t, minlength=nbins)
                scale[name][j] = np.bincount(k, weights=np.abs(t), minlength=nbins)
    launched = n > 0 and mc > 0
    if launched:
        T = candidates64(state, edges, np.where(flags[:, None] != 0, np.nan, c))
        g = grid64(state, edges)
        out.update(nonfinite=int(n - ok.sum()), tested=int(T.sum()), items=int(((T + CHUNK - 1) // CHUNK).sum()),
                   cells=g["cells"], candidates=T)
    else:
        out.update(nonfinite=0, tested=0, items=0, cells=(0, 0, 0), candidates=np.zeros(mc, np.int64))
    out.update(n=n, centers=mc, scale=scale)
    return out


# ---- the host helpers -------------------------------------------------------------------------------------
def enclosed64(inside_mass, bin_mass):
    out = [float(inside_mass)]
    for mb in bin_mass:
        out.append(out[-1] + float(mb))
    return np.array(out)


def overdensity64(inside_mass, bin_mass, edges, rho):
    """(r, mass): the first pair of edges > 0 whose mean enclosed densities bracket rho, ln rho linear in ln r."""
    M = enclosed64(inside_mass, bin_mass)
    edges = np.asarray(edges, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(1, edges.shape[0]):
            if not edges[k - 1] > 0.0:
                continue
            e0, e1 = edges[k - 1], edges[k]
            r0, r1 = M[k - 1] / (SPHERE * ((e0 * e0) * e0)), M[k] / (SPHERE * ((e1 * e1) * e1))
            if r0 >= rho > r1:
                t = (np.log(r0) - np.log(rho)) / (np.log(r0) - np.log(r1))
                r = np.exp(np.log(edges[k - 1]) + t * (np.log(edges[k]) - np.log(edges[k - 1])))
                return r, rho * SPHERE * ((r * r) * r)
    return np.nan, np.nan
