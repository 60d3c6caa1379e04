"""Two independent numpy restatements of nb_sim_knn's rule (include/nbody.h "k-nearest-neighbour density",
DESIGN.md 6i): binary64 from the binary32 state, one rounding per operation.

knn_vectorised  -- the d2 matrix of the queried bodies against all counted ones, np.lexsort on (index, d2) per
                   row, the masses of the first k - 1 added column by column;
knn_loop        -- a plain loop per body that inserts (d2, j) into a sorted list and adds mass_in one by one.

Both return a KnnRef.  knn_vectorised takes `queries` (body indices) to evaluate a sample against all bodies,
which is exact for the sampled bodies; the sums of a KnnRef are formed only when every body was queried."""
from __future__ import annotations

import bisect
import math
from dataclasses import dataclass, field

import numpy as np

NONE = 0xFFFFFFFF
MAX_K = 64
SPHERE = float("4.1887902047863909846")  # the header's literal of 4 pi / 3
TOL = 1e-10  # a sum against its sum of |term|


@dataclass
class KnnRef:
    k: int
    r2: np.ndarray
    kth: np.ndarray
    mass_in: np.ndarray
    density: np.ndarray
    n: int
    nonfinite: int
    counted: int
    degenerate: int = 0
    short_of_k: int = 0
    sums: np.ndarray = field(default_factory=lambda: np.zeros(8))      # rho, rho x[3], rho v[3], rho rho
    sums_abs: np.ndarray = field(default_factory=lambda: np.zeros(8))  # the sums of |term|
    peak_density: float = 0.0
    peak_index: int = NONE


def counted_mask(pos, mass, vel) -> np.ndarray:
    return np.isfinite(pos).all(axis=1) & np.isfinite(mass) & np.isfinite(vel).all(axis=1)


def density_of(mass_in: float, r2: float) -> float:
    """mass_in / (C (r2 sqrt(r2))) as written; +inf for r2 == 0."""
    if r2 == 0.0:
        return math.inf
    den = SPHERE * (r2 * math.sqrt(r2))
    if den == 0.0:
        return math.copysign(math.inf, mass_in) if mass_in != 0.0 else math.nan
    return mass_in / den


def finish(ref: KnnRef, pos, vel, ok, whole: bool) -> KnnRef:
    """degenerate, the eight sums with their sums of |term| (math.fsum: the binary64 sum) and the peak."""
    if ref.counted <= ref.k or not whole:
        return ref
    ref.degenerate = int(np.count_nonzero(ok & (ref.r2 == 0.0)))
    sel = np.nonzero(ok & (ref.r2 != 0.0) & np.isfinite(ref.r2))[0]
    rho = ref.density[sel]
    x, v = pos[sel].astype(np.float64), vel[sel].astype(np.float64)
    terms = [rho, rho * x[:, 0], rho * x[:, 1], rho * x[:, 2], rho * v[:, 0], rho * v[:, 1], rho * v[:, 2], rho * rho]
    ref.sums = np.array([math.fsum(t) for t in terms])
    ref.sums_abs = np.array([math.fsum(np.abs(t)) for t in terms])
    fin = np.isfinite(rho)
    if fin.any():
        ref.peak_density = float(rho[fin].max()) + 0.0
        ref.peak_index = int(sel[fin][rho[fin] == ref.peak_density].min())
    return ref


def _empty(n, k, ok) -> KnnRef:
    c = int(ok.sum())
    ref = KnnRef(k, np.full(n, np.nan), np.full(n, NONE, dtype=np.uint32), np.zeros(n), np.zeros(n), n, n - c, c)
    if c <= k:
        ref.r2[ok] = np.inf
        ref.short_of_k = c
    return ref


def knn_vectorised(pos, mass, vel, k: int, queries=None, rows: int = 256) -> KnnRef:
    pos, mass, vel = np.asarray(pos, np.float32), np.asarray(mass, np.float32), np.asarray(vel, np.float32)
    n = pos.shape[0]
    ok = counted_mask(pos, mass, vel)
    ref = _empty(n, k, ok)
    if ref.counted <= k:
        return ref
    idx = np.nonzero(ok)[0]
    place = np.full(n, -1, dtype=np.int64)
    place[idx] = np.arange(idx.size)
    x = pos[idx].astype(np.float64)
    m = mass[idx].astype(np.float64)
    whole = queries is None
    qs = idx if whole else np.array([q for q in np.asarray(queries, dtype=np.int64) if ok[q]], dtype=np.int64)
    for lo in range(0, qs.size, rows):
        q = qs[lo:lo + rows]
        xq = x[place[q]]
        dx, dy, dz = (xq[:, None, a] - x[None, :, a] for a in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        d2[np.arange(q.size), place[q]] = np.inf  # the body itself is not in its order (the others are finite)
        # the first k of the order (d2, index): only the bodies at or inside a row's k-th smallest d2 can be among
        # them, so those alone are sorted (ascending position is ascending index)
        kd = np.partition(d2, k - 1, axis=-1)[:, k - 1]
        order = np.empty((q.size, k), dtype=np.int64)
        for t, row in enumerate(d2):
            cand = np.nonzero(row <= kd[t])[0]
            order[t] = cand[np.lexsort((cand, row[cand]))[:k]]
        r = np.arange(q.size)
        ref.r2[q] = d2[r, order[:, k - 1]]
        ref.kth[q] = idx[order[:, k - 1]]
        acc = np.zeros(q.size)
        for t in range(k - 1):
            acc = acc + m[order[:, t]]
        ref.mass_in[q] = acc
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            r2 = ref.r2[q]
            ref.density[q] = np.where(r2 == 0.0, np.inf, acc / (SPHERE * (r2 * np.sqrt(r2))))
    return finish(ref, pos, vel, ok, whole)


def knn_loop(pos, mass, vel, k: int) -> KnnRef:
    pos, mass, vel = np.asarray(pos, np.float32), np.asarray(mass, np.float32), np.asarray(vel, np.float32)
    n = pos.shape[0]
    ok = counted_mask(pos, mass, vel)
    ref = _empty(n, k, ok)
    if ref.counted <= k:
        return ref
    bodies = [int(i) for i in np.nonzero(ok)[0]]
    xs = [[float(pos[i, a]) for a in range(3)] for i in range(n)]
    ms = [float(mass[i]) for i in range(n)]
    for i in bodies:
        best = []  # ascending (d2, j), at most k of them
        xi = xs[i]
        for j in bodies:
            if j == i:
                continue
            dx, dy, dz = xi[0] - xs[j][0], xi[1] - xs[j][1], xi[2] - xs[j][2]
            e = ((dx * dx + dy * dy) + dz * dz, j)
            if len(best) < k or e < best[-1]:
                bisect.insort(best, e)
                del best[k:]
        total = 0.0
        for _, j in best[:k - 1]:
            total += ms[j]
        ref.r2[i], ref.kth[i], ref.mass_in[i] = best[k - 1][0], best[k - 1][1], total
        ref.density[i] = density_of(total, best[k - 1][0])
    return finish(ref, pos, vel, ok, True)


def tie_free(ref: KnnRef, pos, mass, vel) -> bool:
    """No counted body has two others at its k-th distance: a permutation of the bodies permutes r2, mass_in
    and density and maps kth.  (Checked through the (k + 1)-th neighbour: r2 of k + 1 differs from r2 of k, and
    so on down to 1.)"""
    prev = None
    for kk in range(1, ref.k + 2):
        if ref.counted <= kk:
            break
        r = knn_vectorised(pos, mass, vel, kk).r2
        if prev is not None and np.any(r[np.isfinite(r)] == prev[np.isfinite(r)]):
            return False
        prev = r
    return True


# ---- the states the tests use ---------------------------------------------------------------------------
def state_of(pos, seed=0) -> np.ndarray:
    """float32[n, 10] with the given positions, seeded velocities and unequal masses."""
    rng = np.random.default_rng(seed)
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    n = len(pos)
    s = np.zeros((n, 10), np.float32)
    s[:, 0:3] = pos
    s[:, 3:6] = rng.normal(0.0, 0.1, (n, 3))
    s[:, 9] = rng.uniform(0.5, 2.0, n)
    return s


def split(state):
    """pos, mass, vel of a float32[n, 10] state."""
    return state[:, 0:3], state[:, 9], state[:, 3:6]


def ball(rng, n, radius, centre=(0.0, 0.0, 0.0)):
    v = rng.normal(size=(n, 3))
    v *= (radius * rng.uniform(0.0, 1.0, n) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]
    return v + np.asarray(centre)


def lattice(side):
    g = np.arange(side, dtype=np.float64)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def border_points(rng):
    """Bodies on the borders of the cells of every octree level of the unit cube (the extent is exactly 1, from
    the corners (0, 0, 0) and (1, 1, 1): a border of level L is a multiple of 2^-L), one binary32 step to either
    side of them, and a few elsewhere."""
    pts = [(0.0, 0.0, 0.0), (1.0, 1.0, 1.0)]
    for level in range(1, 22):
        w = 2.0 ** -level
        for _ in range(6):
            a = rng.integers(0, 2 ** level + 1, 3) * w
            pts.append(tuple(a))
            b = np.float32(a)
            pts.append(tuple(np.nextafter(b, np.float32(2.0))))
            pts.append(tuple(np.nextafter(b, np.float32(-1.0))))
            pts.append((a[0], float(rng.uniform()), a[2]))
    pts = np.clip(np.array(pts, dtype=np.float32), 0.0, 1.0)
    return np.concatenate([pts, rng.uniform(0.0, 1.0, (100, 3)).astype(np.float32)])


def inject_nonfinite(state, count, seed):
    rng = np.random.default_rng(seed)
    n = state.shape[0]
    rows, cols = rng.choice(n, count, replace=False), rng.choice([0, 1, 2, 3, 4, 5, 9], count)
    state[rows, cols] = rng.choice([np.nan, np.inf, -np.inf], count)
    return state


def synthetic_cases(small: bool):
    """(name, state, ks, steppable): steppable says whether an octree can step the state (it refuses bodies
    closer than its finest cell).  small: sizes for the per-body loop restatement."""
    rng = np.random.default_rng(4321)
    out = []
    side = (8,) if small else (8, 16)
    for s in side:
        out.append((f"lattice{s}", state_of(lattice(s), 1), (1, 2, 6, 64) if s == 8 else (6, 32), True))
        out.append((f"lattice{s}_far", state_of(1.0e6 + lattice(s) * 2.0 ** -10, 2), (6, 32), False))
    pts = np.array([(0.1, 0.2, 0.3), (0.1, 0.2, 0.3 + 2.0 ** -20), (-0.4, 0.0, 0.9)])
    three = pts[np.repeat([0, 1, 2], (100, 60, 40))][rng.permutation(200)]
    out.append(("three_points", state_of(three, 3), (6, 32, 64), False))  # multiplicities 100, 60, 40
    m = 150 if small else 700
    line = np.zeros((m, 3))
    line[:, 1] = rng.uniform(-1.0, 1.0, m)
    out.append(("line", state_of(line + (0.5, 0.0, -2.0), 4), (6, 32), False))
    plane = rng.uniform(-1.0, 1.0, (m, 3))
    plane[:, 0] = 0.25
    out.append(("plane", state_of(plane, 5), (6, 32), False))
    m = 200 if small else 2000
    far = np.concatenate([ball(rng, m, 1.0e-3), [(1.0e30, 0.0, 0.0)]])
    out.append(("ball_and_outlier", state_of(far[rng.permutation(m + 1)], 6), (6, 32), False))
    m = 150 if small else 1000
    blobs = np.concatenate([ball(rng, m, 0.01, (0.0, 0.0, 0.0)), ball(rng, m, 0.01, (100.0, 3.0, -7.0))])
    out.append(("two_blobs", state_of(blobs[rng.permutation(2 * m)], 7), (6, 32), True))
    out.append(("cell_borders", state_of(border_points(rng), 8)[:300 if small else None], (1, 6, 32), False))
    one = np.tile([(3.0, -1.0, 2.0)], (70, 1))
    out.append(("one_point", state_of(one, 9), (6, 64), False))
    return out
