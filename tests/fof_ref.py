"""The friends-of-friends rule of include/nbody.h ("Friends-of-friends groups") restated in numpy
binary64, twice and independently of each other and of the library's cells:

  fof_brute -- every pair by the rule and a plain union-find; O(n^2), for small n;
  fof_grid  -- candidate pairs from cubic cells of side 1.0001 link about the origin (27 neighbours, every
               candidate decided by the same rule), components by repeated minimum-label relaxation.

Both take the float32[n, 10] state (px py pz vx vy vz ax ay az mass) and return the same dictionary.
"""
import numpy as np

NONE = 0xFFFFFFFF
SUMS = ("mass", "mx", "my", "mz", "mvx", "mvy", "mvz", "mr2", "mv2")


def body_ok(state):
    return np.isfinite(state[:, [0, 1, 2, 3, 4, 5, 9]]).all(axis=1)


def friends(pi, pj, link):
    """The rule on float32 positions pi, pj (..., 3): d2 <= b2 in binary64, one rounding per operation."""
    d = pi.astype(np.float64) - pj.astype(np.float64)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    b2 = np.float64(link) * np.float64(link)
    return (dx * dx + dy * dy) + dz * dz <= b2


def _labels_brute(pos, ok, link):
    n = pos.shape[0]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    idx = np.flatnonzero(ok)
    for a, i in enumerate(idx):
        js = idx[a + 1:][friends(pos[i][None, :], pos[idx[a + 1:]], link)]
        ri = find(int(i))
        for j in js:
            rj = find(int(j))
            if rj != ri:
                lo, hi = min(ri, rj), max(ri, rj)
                parent[hi] = lo
                ri = lo
    labels = np.full(n, NONE, np.uint32)
    for i in idx:
        labels[i] = find(int(i))
    return labels


def _pairs_grid(pos, ok, link):
    """Every friends pair (i, j), i < j, as two index arrays."""
    idx = np.flatnonzero(ok)
    if idx.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    p = pos[idx].astype(np.float64)
    # cells a little larger than link: friends then differ by at most one cell per axis whatever the division rounds to
    cell = np.floor(p / (1.0001 * np.float64(link))).astype(np.int64)
    cell -= cell.min(axis=0)
    dims = cell.max(axis=0) + 3  # room for the +-1 neighbours
    key = ((cell[:, 2] + 1) * dims[1] + (cell[:, 1] + 1)) * dims[0] + (cell[:, 0] + 1)
    order = np.argsort(key, kind="stable")
    skey = key[order]
    out_i, out_j = [], []
    for oz in (-1, 0, 1):
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                want = skey + (oz * dims[1] + oy) * dims[0] + ox
                lo, hi = np.searchsorted(skey, want, "left"), np.searchsorted(skey, want, "right")
                cnt = hi - lo
                total = int(cnt.sum())
                if total == 0:
                    continue
                step = 1 << 22  # candidate pairs at a time
                ends = np.cumsum(cnt)
                a0 = 0
                while a0 < skey.size:
                    a1 = int(np.searchsorted(ends, (ends[a0 - 1] if a0 else 0) + step, "right"))
                    a1 = max(a1, a0 + 1)
                    c = cnt[a0:a1]
                    if c.sum():
                        src = np.repeat(np.arange(a0, a1), c)
                        first = np.repeat(lo[a0:a1] - (np.cumsum(c) - c), c)
                        dst = np.arange(src.size) + first
                        gi, gj = idx[order[src]], idx[order[dst]]
                        keep = gi < gj
                        gi, gj = gi[keep], gj[keep]
                        keep = friends(pos[gi], pos[gj], link)
                        out_i.append(gi[keep])
                        out_j.append(gj[keep])
                    a0 = a1
    if not out_i:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(out_i).astype(np.int64), np.concatenate(out_j).astype(np.int64)


def _labels_grid(pos, ok, link):
    n = pos.shape[0]
    i, j = _pairs_grid(pos, ok, link)
    lab = np.arange(n, dtype=np.int64)
    while True:  # hook to the smaller label across every edge, then jump: ends when no edge joins two labels
        new = lab.copy()
        np.minimum.at(new, i, lab[j])
        np.minimum.at(new, j, lab[i])
        # a body whose label fell pulls its old label's body down with it
        np.minimum.at(new, lab, new)
        while True:
            jump = new[new]
            if np.array_equal(jump, new):
                break
            new = jump
        if np.array_equal(new, lab):
            break
        lab = new
    out = lab.astype(np.uint32)
    out[~ok] = NONE
    return out


def catalogue(state, labels, link, min_members):
    """Everything nb_sim_fof returns, from the labels."""
    n = state.shape[0]
    ok = labels != NONE
    roots, counts = np.unique(labels[ok], return_counts=True)  # ascending labels
    listed = counts >= min_members
    rows_label, rows_count = roots[listed], counts[listed]
    row_of_root = np.full(n, NONE, np.uint32)
    row_of_root[rows_label] = np.arange(rows_label.size, dtype=np.uint32)
    group_of = np.full(n, NONE, np.uint32)
    group_of[ok] = row_of_root[labels[ok]]
    s = state.astype(np.float64)
    x, v, m = s[:, 0:3], s[:, 3:6], s[:, 9]
    with np.errstate(invalid="ignore", over="ignore"):  # (non-finite bodies are members of nothing)
        terms = np.stack([m, m * x[:, 0], m * x[:, 1], m * x[:, 2], m * v[:, 0], m * v[:, 1], m * v[:, 2],
                          m * ((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]),
                          m * ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])], axis=1)
    g = rows_label.size
    sums, scale = np.zeros((g, 9)), np.zeros((g, 9))
    member = group_of != NONE
    if g:
        np.add.at(sums, group_of[member], terms[member])
        np.add.at(scale, group_of[member], np.abs(terms[member]))
    big = int(counts.max()) if counts.size else 0
    return dict(n=n, nonfinite=int(n - ok.sum()), labels=labels, group_of=group_of, components=int(roots.size),
                groups=int(g), grouped_bodies=int(rows_count.sum()), largest_count=big,
                largest_label=int(roots[counts == big].min()) if counts.size else NONE,
                rows_label=rows_label.astype(np.uint32), rows_count=rows_count.astype(np.uint32), sums=sums,
                scale=scale)


def fof_brute(state, link, min_members=1):
    ok = body_ok(state)
    return catalogue(state, _labels_brute(state[:, 0:3], ok, link), link, min_members)


def fof_grid(state, link, min_members=1):
    ok = body_ok(state)
    return catalogue(state, _labels_grid(state[:, 0:3], ok, link), link, min_members)


def cell_side(link):
    """The library's cell side (nb_fof_stats.cell_side): (link / sqrt(3)) (1 - 2^-20)."""
    return (np.float64(link) / np.sqrt(np.float64(3.0))) * (np.float64(1.0) - np.float64(2.0) ** -20)


def _state(pos, seed=0):
    """float32[n, 10] with the given positions, seeded velocities and unequal masses."""
    rng = np.random.default_rng(seed)
    n = len(pos)
    s = np.zeros((n, 10), np.float32)
    s[:, 0:3] = np.asarray(pos, np.float32).reshape(n, 3)
    s[:, 3:6] = rng.normal(0.0, 0.1, (n, 3))
    s[:, 9] = rng.uniform(0.5, 2.0, n)
    return s


def _ball(rng, n, radius, centre):
    v = rng.normal(size=(n, 3))
    v *= (radius * rng.uniform(0.0, 1.0, n) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]
    return v + np.asarray(centre)


def synthetic_cases(small):
    """(name, state, link, expected number of components or None).  small: every case at n <= 2048, for the
    brute-force restatement; otherwise at the sizes the device is tested at."""
    rng = np.random.default_rng(1234)
    out = []
    b = 0.25
    out.append(("edge_inside", _state([(0.5, 0.0, 0.0), (0.75, 0.0, 0.0)]), b, 1))
    out.append(("edge_outside", _state([(0.5, 0.0, 0.0), (np.nextafter(np.float32(0.75), np.float32(1.0)), 0.0, 0.0)]),
                b, 2))
    out.append(("edge_diagonal", _state([(-0.5, -0.25, 0.125), (-0.5 + 0.0625, -0.25 - 0.125, 0.125 + 0.125)]),
                0.1875, 1))  # (1, 2, 2) / 16: length 3 / 16 exactly
    b = 2.0 ** -6
    n = 2048 if small else 4096
    chain = np.zeros((n, 3))
    chain[:, 0] = np.arange(n) * b - 7.0
    out.append(("chain", _state(chain[rng.permutation(n)], 1), b, 1))
    side = 12 if small else 16
    k = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    out.append(("lattice", _state(k * (b * (1.0 + 2.0 ** -10)) - 0.07, 2), b, side ** 3))
    co = np.concatenate([np.tile([[0.3, -0.2, 0.1]], (1000, 1)), rng.uniform(-1.0, 1.0, (200, 3))])
    out.append(("coincident", _state(co[rng.permutation(len(co))], 3), 0.01, None))
    b, m = 0.05, (1000 if small else 3000)
    balls = np.concatenate([_ball(rng, m, b / 4, (0.1, 0.2, -0.3)), _ball(rng, m, b / 4, (0.1 + 1.6 * b, 0.2, -0.3))])
    out.append(("two_balls", _state(balls[rng.permutation(2 * m)], 4), b, 2))
    b = 1e-3
    clump = rng.uniform(-0.01, 0.01, (2000, 3)) + np.array([1000.0, -1000.0, 1000.0])
    out.append(("far_clump", _state(clump, 5), b, None))
    # bodies on the cells' borders: the first body is the grid's origin, the others sit at multiples of the
    # cell side from it, as float32 rounds them and one ulp to either side
    b = 0.01
    h = cell_side(b)
    origin = np.array([-0.37, -1.25, -2.0], np.float32)
    steps = rng.integers(0, 40, (600, 3))
    at = (origin.astype(np.float64) + steps * h).astype(np.float32)
    nudge = rng.integers(-1, 2, (600, 3))
    at = np.where(nudge < 0, np.nextafter(at, np.float32(-np.inf)), np.where(nudge > 0, np.nextafter(at, np.float32(np.inf)), at))
    at = np.maximum(at, origin)
    out.append(("cell_borders", _state(np.concatenate([origin[None, :], at]), 6), b, None))
    return out


def partition(labels):
    """The partition as a set of frozensets of body indices (bodies of no group left out)."""
    out = {}
    for i, lab in enumerate(labels):
        if lab != NONE:
            out.setdefault(int(lab), []).append(i)
    return {frozenset(v) for v in out.values()}
