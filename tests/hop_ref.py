"""The density-peak rule of include/nbody.h ("Density-peak groups") restated in numpy binary64,
O(n^2), on the distance expression of tests/knn_ref.py:

  hop_vectorised -- the neighbour order from the d2 matrix (np.lexsort on (index, d2) per row), the hop by an
                    argmax over a lexsort key, the chains by repeated jumping, the boundaries by np.unique;
  hop_loop       -- plain Python per body: a sorted list of (d2, j), the hop by comparing tuples, the chains by
                    walking; labels only (what the two restatements are compared on);
  regroup        -- nb_hop_regroup in plain Python.

All take the float32[n, 10] state (px py pz vx vy vz ax ay az mass)."""
from __future__ import annotations

import math

import numpy as np

from . import fof_ref, knn_ref

NONE = 0xFFFFFFFF


def _split(state):
    state = np.asarray(state, np.float32)
    return state[:, 0:3], state[:, 9], state[:, 3:6]


def neighbour_order(pos, ok, k: int, rows: int = 256) -> np.ndarray:
    """order[i, t]: the (t + 1)-th body of counted body i's (d2, j) order, t < k (NONE for other bodies); needs
    more than k counted bodies."""
    n = pos.shape[0]
    idx = np.nonzero(ok)[0]
    x = pos[idx].astype(np.float64)
    order = np.full((n, k), NONE, dtype=np.int64)
    for lo in range(0, idx.size, rows):
        q = np.arange(lo, min(idx.size, lo + rows))
        xq = x[q]
        dx, dy, dz = (xq[:, None, a] - x[None, :, a] for a in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        d2[np.arange(q.size), q] = np.inf  # the body itself is not in its order
        kd = np.partition(d2, k - 1, axis=-1)[:, k - 1]
        for t, row in enumerate(d2):
            cand = np.nonzero(row <= kd[t])[0]
            order[idx[q[t]]] = idx[cand[np.lexsort((cand, row[cand]))[:k]]]
    return order


def rho_key(density):
    return np.where(np.isnan(density), -np.inf, density)


def hop_vectorised(state, k_density: int, k_hop: int, k_merge: int, min_members: int = 1,
                   density_min: float = -math.inf) -> dict:
    state = np.asarray(state, np.float32)
    pos, mass, vel = _split(state)
    n = pos.shape[0]
    ok = knn_ref.counted_mask(pos, mass, vel)
    c = int(ok.sum())
    k_all = max(k_density, k_hop, k_merge)
    density = knn_ref.knn_vectorised(pos, mass, vel, k_density).density
    labels = np.full(n, NONE, dtype=np.uint32)
    out = dict(n=n, nonfinite=n - c, counted=c, density=density, short_of_k=c if c <= k_all else 0, outside=0)
    bnd = np.zeros(0, dtype=[("a", "<u4"), ("b", "<u4"), ("pairs", "<u4"), ("density", "<f8")])
    pairs_total = 0
    if c > k_all:
        rho = rho_key(density)
        inside = ok & (rho >= density_min)
        out["outside"] = int((ok & ~inside).sum())
        order = neighbour_order(pos, ok, max(k_hop, k_merge))
        ins = np.nonzero(inside)[0]
        # the hop: the densest among the body and its first k_hop neighbours
        cand = np.concatenate([ins[:, None], order[ins, :k_hop]], axis=1)
        nxt = np.arange(n, dtype=np.int64)
        for t, i in enumerate(ins):
            cc = cand[t]
            nxt[i] = cc[np.lexsort((cc, -rho[cc]))[0]]  # descending rho', then ascending index
        assert inside[nxt[ins]].all()  # a denser neighbour of an inside body is inside
        while True:
            jump = nxt[nxt]
            if np.array_equal(jump, nxt):
                break
            nxt = jump
        labels[ins] = nxt[ins]
        # the boundaries
        if ins.size:
            i = np.repeat(ins, k_merge)
            j = order[ins, :k_merge].reshape(-1)
            keep = inside[j]
            i, j = i[keep], j[keep]
            keep = labels[i] != labels[j]
            i, j = i[keep], j[keep]
            pairs_total = int(i.size)
            if i.size:
                a = np.minimum(labels[i], labels[j]).astype(np.uint64)
                b = np.maximum(labels[i], labels[j]).astype(np.uint64)
                with np.errstate(invalid="ignore"):
                    v = 0.5 * (rho[i] + rho[j])
                key = (a << np.uint64(32)) | b
                uk, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
                mx = np.full(uk.size, -np.inf)
                np.maximum.at(mx, inv, v)
                bnd = np.zeros(uk.size, dtype=bnd.dtype)
                bnd["a"], bnd["b"] = (uk >> np.uint64(32)).astype(np.uint32), (uk & np.uint64(NONE)).astype(np.uint32)
                bnd["pairs"], bnd["density"] = cnt, mx + 0.0  # (a zero maximum is +0)
    cat = fof_ref.catalogue(state, labels, 0.0, min_members)
    out.update(labels=labels, group_of=cat["group_of"], peaks=cat["components"], groups=cat["groups"],
               grouped_bodies=cat["grouped_bodies"], largest_count=cat["largest_count"],
               largest_label=cat["largest_label"], rows_label=cat["rows_label"], rows_count=cat["rows_count"],
               sums=cat["sums"], scale=cat["scale"], peak_density=density[cat["rows_label"]],
               boundaries=bnd, boundary_pairs=pairs_total)
    return out


def hop_loop(state, k_density: int, k_hop: int, k_merge: int, density_min: float = -math.inf) -> np.ndarray:
    """The labels alone, body by body."""
    state = np.asarray(state, np.float32)
    pos, mass, vel = _split(state)
    n = pos.shape[0]
    ok = knn_ref.counted_mask(pos, mass, vel)
    labels = [NONE] * n
    bodies = [int(i) for i in np.nonzero(ok)[0]]
    if len(bodies) <= max(k_density, k_hop, k_merge):
        return np.array(labels, dtype=np.uint32)
    dens = knn_ref.knn_loop(pos, mass, vel, k_density).density
    rho = [(-math.inf if math.isnan(d) else float(d)) for d in dens]
    xs = [[float(pos[i, a]) for a in range(3)] for i in range(n)]
    nxt = {}
    for i in bodies:
        if not rho[i] >= density_min:
            continue
        near = []
        for j in bodies:
            if j != i:
                dx, dy, dz = xs[i][0] - xs[j][0], xs[i][1] - xs[j][1], xs[i][2] - xs[j][2]
                near.append(((dx * dx + dy * dy) + dz * dz, j))
        near.sort()
        best = i
        for _, j in near[:k_hop]:
            if rho[j] > rho[best] or (rho[j] == rho[best] and j < best):
                best = j
        nxt[i] = best
    for i in nxt:
        p = i
        while nxt[p] != p:
            p = nxt[p]
        labels[i] = p
    return np.array(labels, dtype=np.uint32)


def regroup(rows_label, rows_count, sums, peak_density, boundaries, saddle: float, peak: float):
    """nb_hop_regroup: (merged_of_row, out_label, out_count, out_sums, out_peak).  boundaries: records or tuples
    (a, b, ..., density) in ascending (a, b), the density last."""
    m = len(rows_label)
    row_of = {int(lab): r for r, lab in enumerate(rows_label)}
    key = [(-math.inf if math.isnan(float(p)) else float(p)) for p in peak_density]
    viable = [key[r] >= peak for r in range(m)]
    parent = list(range(m))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    edges = [(float(e[-1]), int(e[0]), int(e[1])) for e in boundaries if int(e[0]) in row_of and int(e[1]) in row_of]
    edges.sort(key=lambda e: (math.inf if math.isnan(e[0]) else -e[0], e[1], e[2]))  # (a NaN as -inf, like a peak's)
    for d, a, b in edges:
        x, y = find(row_of[a]), find(row_of[b])
        if x == y:
            continue
        if viable[x] and viable[y] and d < saddle:
            continue
        parent[y] = x
        viable[x] = viable[x] or viable[y]
    sets = {}
    for r in range(m):
        sets.setdefault(find(r), []).append(r)
    merged = np.full(m, NONE, dtype=np.uint32)
    out = []
    for root, members in sets.items():
        if not viable[root]:
            continue
        rep = min(members, key=lambda r: (-key[r], int(rows_label[r])))
        merged[members] = rows_label[rep]
        total = np.zeros(9)
        for r in members:  # ascending row order
            total = total + np.asarray(sums[r], dtype=np.float64)
        out.append((int(rows_label[rep]), int(sum(int(rows_count[r]) for r in members)), total,
                    float(peak_density[rep])))
    out.sort(key=lambda o: o[0])
    return (merged, np.array([o[0] for o in out], dtype=np.uint32), np.array([o[1] for o in out], dtype=np.uint32),
            np.array([o[2] for o in out]).reshape(len(out), 9), np.array([o[3] for o in out]))


# ---- the states the tests use ---------------------------------------------------------------------------
def two_clumps(seed: int = 1, per: int = 2048, sigma: float = 0.3, apart: float = 2.0, bridge: int = 0):
    """Two Gaussian clumps of `per` bodies each, their centres `apart` on x; `bridge` bodies of each clump are
    moved onto the line between the centres (a thin bridge: friends-of-friends joins the clumps along it)."""
    rng = np.random.default_rng(seed)
    a = rng.normal(0.0, sigma, (per, 3)) + (-apart / 2, 0.0, 0.0)
    b = rng.normal(0.0, sigma, (per, 3)) + (apart / 2, 0.0, 0.0)
    if bridge:
        t = (np.arange(2 * bridge) + 0.5) / (2 * bridge)
        line = np.zeros((2 * bridge, 3))
        line[:, 0] = (t - 0.5) * apart
        a[:bridge], b[:bridge] = line[:bridge], line[bridge:]
    return knn_ref.state_of(np.concatenate([a, b]), seed)
