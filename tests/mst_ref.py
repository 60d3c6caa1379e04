"""Numpy restatements of nb_mst_sim's rule (include/nbody.h "Minimum spanning tree"): binary64 from the
binary32 state, one rounding per operation, pairs ordered by (d2, min index, max index).

prim            -- vectorised, O(n^2) time and O(n) memory: every body outside the tree keeps its first edge of the
                   order into the tree;
kruskal         -- every pair, np.lexsort((hi, lo, d2)), a union-find;
boruvka         -- literal: every round each component takes the first edge of the order that leaves it; records
                   `rounds` and `components_after`;
boruvka_on_tree -- the same rounds on a tree's own edges: a component's first leaving edge is always a tree edge
                   (the cut property), so the rounds are those of the complete graph (checked against boruvka);
cut, linkage    -- nb_mst_cut and nb_mst_linkage restated.

All return or take an MstRef."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from tests import knn_ref as K
from tests.helpers import make_state

NONE = 0xFFFFFFFF
MAX_ROUNDS = 32


@dataclass
class MstRef:
    n: int
    nonfinite: int
    lo: np.ndarray       # (m,) uint32, ascending edge order
    hi: np.ndarray
    d2: np.ndarray       # (m,) float64
    degree: np.ndarray   # (n,) uint32, NONE for a body that is not counted
    rounds: int = 0
    components_after: np.ndarray = field(default_factory=lambda: np.zeros(MAX_ROUNDS, np.uint32))
    plan_lo: np.ndarray = field(default_factory=lambda: np.zeros(3))
    plan_hi: np.ndarray = field(default_factory=lambda: np.zeros(3))
    h: float = 0.0

    @property
    def edges(self) -> int:
        return len(self.d2)

    @property
    def d2_min(self) -> float:
        return float(self.d2[0]) if len(self.d2) else 0.0

    @property
    def d2_max(self) -> float:
        return float(self.d2[-1]) if len(self.d2) else 0.0


def _split(state):
    state = np.asarray(state, np.float32)
    pos, mass, vel = K.split(state)
    return pos, K.counted_mask(pos, mass, vel)


def d2_rows(x, rows, cols=slice(None)):
    """d2 of the rule between x[rows] and x[cols], x binary64."""
    dx, dy, dz = (x[rows, None, a] - x[None, cols, a] for a in range(3))
    return (dx * dx + dy * dy) + dz * dz


def _finish(state, pairs) -> MstRef:
    """An MstRef from (d2, lo, hi) triples in any order: sorted, the degrees counted, the plan restated."""
    pos, ok = _split(state)
    n = len(pos)
    pairs = sorted(pairs)
    d2 = np.array([p[0] for p in pairs], np.float64)
    lo = np.array([p[1] for p in pairs], np.uint32)
    hi = np.array([p[2] for p in pairs], np.uint32)
    degree = np.where(ok, 0, NONE).astype(np.uint32)
    np.add.at(degree, lo, 1)
    np.add.at(degree, hi, 1)
    ref = MstRef(n, int(n - ok.sum()), lo, hi, d2, degree)
    if ok.any():
        x = pos[ok].astype(np.float64)
        ref.plan_lo, ref.plan_hi = x.min(axis=0), x.max(axis=0)
        ref.h = float((ref.plan_hi - ref.plan_lo).max() * 2.0 ** -21)
    return ref


def prim(state) -> MstRef:
    pos, ok = _split(state)
    idx = np.flatnonzero(ok)
    c = idx.size
    pairs = []
    if c > 1:
        x = pos[idx].astype(np.float64)
        inside = np.zeros(c, bool)
        inside[0] = True
        best_d = d2_rows(x, [0])[0]
        best_u = np.zeros(c, np.int64)  # (positions among the counted bodies: ascending position = ascending index)
        me = np.arange(c)
        for _ in range(c - 1):
            out = np.flatnonzero(~inside)
            d = best_d[out]
            t = out[d == d.min()]
            a, b = np.minimum(t, best_u[t]), np.maximum(t, best_u[t])
            w = t[np.lexsort((b, a))[0]]
            u = best_u[w]
            pairs.append((float(best_d[w]), int(idx[min(u, w)]), int(idx[max(u, w)])))
            inside[w] = True
            d = d2_rows(x, [w])[0]
            lo_new, hi_new = np.minimum(me, w), np.maximum(me, w)
            lo_old, hi_old = np.minimum(me, best_u), np.maximum(me, best_u)
            better = (d < best_d) | ((d == best_d) & ((lo_new < lo_old) | ((lo_new == lo_old) & (hi_new < hi_old))))
            better &= ~inside
            best_d[better] = d[better]
            best_u[better] = w
    return _finish(state, pairs)


def all_pairs(state):
    """(d2, lo, hi) of every pair of counted bodies, as three arrays (lo < hi, body indices)."""
    pos, ok = _split(state)
    idx = np.flatnonzero(ok)
    x = pos[idx].astype(np.float64)
    a, b = np.triu_indices(idx.size, 1)
    dx, dy, dz = (x[a, k] - x[b, k] for k in range(3))
    return (dx * dx + dy * dy) + dz * dz, idx[a], idx[b]


class _Forest:
    def __init__(self, n):
        self.parent = list(range(n))

    def root(self, x):
        p = self.parent
        while p[x] != x:
            p[x] = p[p[x]]
            x = p[x]
        return x

    def unite(self, a, b):
        a, b = self.root(a), self.root(b)
        if a == b:
            return False
        self.parent[max(a, b)] = min(a, b)
        return True


def kruskal(state, order=None) -> MstRef:
    """order: the sort of the pairs, by default the rule's lexsort((hi, lo, d2)) (a mutation passes another)."""
    d2, lo, hi = all_pairs(state)
    order = np.lexsort((hi, lo, d2)) if order is None else order(d2, lo, hi)
    f = _Forest(len(np.asarray(state)))
    pairs = []
    for e in order:
        if f.unite(int(lo[e]), int(hi[e])):
            pairs.append((float(d2[e]), int(lo[e]), int(hi[e])))
    return _finish(state, pairs)


def _rounds(ref: MstRef, state, choose) -> MstRef:
    """Boruvka's rounds: choose(labels) -> {component label: (d2, lo, hi)}, the first edge that leaves each."""
    _, ok = _split(state)
    f = _Forest(ref.n)
    comps = int(ok.sum())
    pairs = set()
    after = np.zeros(MAX_ROUNDS, np.uint32)
    rounds = 0
    while comps > 1:
        labels = np.array([f.root(i) for i in range(ref.n)])
        for e in choose(labels).values():
            pairs.add(e)
            f.unite(e[1], e[2])
        comps = len({f.root(i) for i in np.flatnonzero(ok)})
        after[rounds] = comps
        rounds += 1
    out = _finish(state, pairs)
    out.rounds, out.components_after = rounds, after
    return out


def boruvka(state) -> MstRef:
    pos, ok = _split(state)
    idx = np.flatnonzero(ok)
    x = pos[idx].astype(np.float64)

    def choose(labels):
        lab = labels[idx]
        best = {}
        for s in range(0, idx.size, 256):
            rows = np.arange(s, min(idx.size, s + 256))
            d = d2_rows(x, rows)
            d[lab[rows, None] == lab[None, :]] = np.inf
            for t, r in enumerate(rows):
                row = d[t]
                j = int(np.flatnonzero(row == row.min())[0])  # ascending position = ascending index
                i, j = int(idx[r]), int(idx[j])
                e = (float(row.min()), min(i, j), max(i, j))
                if lab[r] not in best or e < best[lab[r]]:
                    best[lab[r]] = e
        return best

    return _rounds(MstRef(len(pos), 0, None, None, None, None), state, choose)


def boruvka_on_tree(tree: MstRef, state) -> MstRef:
    edges = list(zip(tree.d2.tolist(), tree.lo.tolist(), tree.hi.tolist()))

    def choose(labels):
        best = {}
        for e in edges:  # ascending: the first edge seen that leaves a component is its choice
            a, b = labels[e[1]], labels[e[2]]
            if a != b:
                best.setdefault(a, e)
                best.setdefault(b, e)
        return best

    return _rounds(tree, state, choose)


def reference(state) -> MstRef:
    """prim's tree with the rounds of boruvka_on_tree: what a device call is compared with."""
    return boruvka_on_tree(prim(state), state)


def cut(ref: MstRef, link: float):
    """labels (n,) uint32 and the number of components: the edges with d2 <= link * link united."""
    b2 = float(link) * float(link)
    f = _Forest(ref.n)
    for d, a, b in zip(ref.d2, ref.lo, ref.hi):
        if d <= b2:
            f.unite(int(a), int(b))
    labels = np.array([NONE if ref.degree[i] == NONE else f.root(i) for i in range(ref.n)], np.uint32)
    return labels, int(np.count_nonzero(labels == np.arange(ref.n)))


def linkage(ref: MstRef):
    f = _Forest(ref.n)
    size = [1] * ref.n
    out = np.zeros((4, ref.edges), np.uint32)
    for e, (a, b) in enumerate(zip(ref.lo, ref.hi)):
        ra, rb = f.root(int(a)), f.root(int(b))
        a, b = min(ra, rb), max(ra, rb)
        out[:, e] = (a, b, size[a], size[b])
        f.unite(a, b)
        size[a] += size[b]
    return tuple(out)


def tie_free(state) -> bool:
    """No two pairs of counted bodies share a d2: the tree does not depend on the indices."""
    d2 = all_pairs(state)[0]
    return np.unique(d2).size == d2.size


def boruvka_cells(pos, cell: float, strict: bool) -> set:
    """Boruvka with a cell-pruned search on a grid of side `cell`, every body counted: a body looks at the cells in
    ascending order of their lower bound B of d2 -- among equal bounds the cell of the larger index first, the order
    least kind to a wrong rule -- and skips a cell when B > best (strict, the rule of DESIGN.md 6y) or when
    B >= best (the mutation).  Returns the set of (d2, lo, hi)."""
    x = np.asarray(pos, np.float32).astype(np.float64)
    n = len(x)
    cells = {}
    for i in range(n):
        cells.setdefault(tuple(np.floor(x[i] / cell).astype(int)), []).append(i)
    f = _Forest(n)
    pairs = set()
    while len({f.root(i) for i in range(n)}) > 1:
        labels = [f.root(i) for i in range(n)]
        best = {}
        for i in range(n):
            todo = []
            for cc, members in cells.items():
                lo_edge, hi_edge = np.array(cc) * cell, (np.array(cc) + 1) * cell
                g = np.maximum(0.0, np.maximum(lo_edge - x[i], x[i] - hi_edge))
                todo.append((float((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]), -min(members), members))
            mine = None
            for bound, _, members in sorted(todo):
                if mine is not None and (bound > mine[0] if strict else bound >= mine[0]):
                    continue
                for j in members:
                    if labels[j] == labels[i]:
                        continue
                    d = x[i] - x[j]
                    e = (float((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]), j)
                    if mine is None or e < mine:
                        mine = e
            e = (mine[0], min(i, mine[1]), max(i, mine[1]))
            if labels[i] not in best or e < best[labels[i]]:
                best[labels[i]] = e
        for e in best.values():
            pairs.add(e)
            f.unite(e[1], e[2])
    return pairs


# ---- the states the tests use ---------------------------------------------------------------------------
def piles(rng, points: int, each: int, seed=0):
    """`points` places with `each` coincident bodies, shuffled."""
    p = rng.uniform(-1.0, 1.0, (points, 3)).astype(np.float32)
    return K.state_of(p[np.repeat(np.arange(points), each)][rng.permutation(points * each)], seed)


def two_blobs(rng, each: int, radius=1.0e-3, apart=10.0, seed=0):
    b = np.concatenate([K.ball(rng, each, radius), K.ball(rng, each, radius, (apart, 0.3 * apart, -0.1 * apart))])
    return K.state_of(b[rng.permutation(2 * each)], seed)


def crowd_and_outlier(rng, crowd: int, seed=0):
    """`crowd` bodies within 2^-20 of the extent, and one outlier that sets it."""
    b = np.concatenate([1.0 + K.ball(rng, crowd, 2.0 ** -21), [(1.0 + 1.0, 1.0, 1.0)]])
    return K.state_of(b[rng.permutation(crowd + 1)], seed)


def small_cases():
    """(name, state): small enough for kruskal's all pairs and the literal boruvka."""
    rng = np.random.default_rng(977)
    out = [(f"n{n}", K.state_of(K.ball(rng, n, 1.0), n)) for n in (0, 1, 2, 3, 64, 65)]
    out.append(("ball96", K.state_of(K.ball(rng, 96, 1.0), 11)))
    out.append(("lattice4", K.state_of(K.lattice(4), 12)))
    out.append(("lattice8", K.state_of(K.lattice(8), 13)))
    out.append(("piles6x12", piles(rng, 6, 12, 14)))
    out.append(("two_blobs", two_blobs(rng, 100, seed=15)))
    out.append(("crowd_and_outlier", crowd_and_outlier(rng, 255, 16)))
    out.append(("cell_borders", K.state_of(K.border_points(rng), 17)[:300]))
    out.append(("nonfinite", K.inject_nonfinite(K.state_of(K.ball(rng, 200, 1.0), 18), 12, 19)))
    out.append(("none_counted", K.state_of(np.full((9, 3), np.nan), 20)))
    return out


def gpu_cases():
    """(name, state, steppable): the states of tests/test_mst_gpu.py; steppable as in tests/knn_ref.py."""
    rng = np.random.default_rng(1979)
    out = [(f"n{n}", K.state_of(K.ball(rng, n, 1.0), n), n > 0) for n in (0, 1, 2, 3, 64, 65)]
    for init in ("uniform", "disc", "spherical"):
        out.append((init, make_state(init, 4096, seed=7), True))
    out.append(("lattice8", K.state_of(K.lattice(8), 13), True))
    out.append(("piles16x64", piles(rng, 16, 64, 14), False))
    out.append(("two_blobs", two_blobs(rng, 2048, seed=15), False))
    out.append(("crowd_and_outlier", crowd_and_outlier(rng, 4095, 16), False))
    out.append(("cell_borders", K.state_of(K.border_points(rng), 17), False))
    out.append(("sample16385", K.state_of(K.ball(rng, 16385, 1.0), 21), True))
    out.append(("nonfinite_disc", K.inject_nonfinite(make_state("disc", 4096, seed=5).copy(), 40, 3), False))
    out.append(("nonfinite_ball", K.inject_nonfinite(K.state_of(K.ball(rng, 1000, 1.0), 22), 25, 4), False))
    return out
