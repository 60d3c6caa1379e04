"""The phase-space friends rule of include/nbody.h ("Phase-space groups") restated in numpy binary64,
twice and independently of each other and of the library's cells:

  fof6_brute -- every pair by the rule and a plain union-find; O(n^2), for small n;
  fof6_grid  -- candidate pairs from cubic position cells of side 1.0001 link about the origin (27 neighbours, every
                candidate decided by the same rule), components by repeated minimum-label relaxation.

Both take the float32[n, 10] state (px py pz vx vy vz ax ay az mass) and return the dictionary of tests/fof_ref.py,
whose catalogue code (and whose synthetic states, given velocities here) they reuse.
"""
import numpy as np

from tests import fof_ref as F

NONE = F.NONE


def friends6(pi, vi, pj, vj, link, vlink):
    """The rule on float32 positions and velocities (..., 3): both clauses in binary64, one rounding per operation."""
    b2 = np.float64(link) * np.float64(link)
    v2 = np.float64(vlink) * np.float64(vlink)
    rhs = b2 * v2
    d = pi.astype(np.float64) - pj.astype(np.float64)
    u = vi.astype(np.float64) - vj.astype(np.float64)
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    u2 = (u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2]
    with np.errstate(over="ignore"):
        return (d2 <= b2) & ((d2 * v2 + u2 * b2) <= rhs)


def _labels_brute(pos, vel, ok, link, vlink):
    n = pos.shape[0]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    idx = np.flatnonzero(ok)
    for a, i in enumerate(idx):
        rest = idx[a + 1:]
        for j in rest[friends6(pos[i][None, :], vel[i][None, :], pos[rest], vel[rest], link, vlink)]:
            ri, rj = find(int(i)), find(int(j))
            if ri != rj:
                parent[max(ri, rj)] = min(ri, rj)
    labels = np.full(n, NONE, np.uint32)
    for i in idx:
        labels[i] = find(int(i))
    return labels


def _pairs_grid(pos, vel, ok, link, vlink):
    """Every friends pair (i, j), i < j, as two index arrays: the candidates by sorted cell codes, offset by offset."""
    idx = np.flatnonzero(ok)
    empty = np.zeros(0, np.int64)
    if idx.size == 0:
        return empty, empty
    cell = np.floor(pos[idx].astype(np.float64) / (1.0001 * np.float64(link))).astype(np.int64)
    cell -= cell.min(axis=0) - 1
    dims = cell.max(axis=0) + 2
    code = (cell[:, 2] * dims[1] + cell[:, 1]) * dims[0] + cell[:, 0]
    order = np.argsort(code, kind="stable")
    scode = code[order]
    out_i, out_j = [empty], [empty]
    for off in np.ndindex(3, 3, 3):
        oz, oy, ox = (o - 1 for o in off)
        want = scode + (oz * dims[1] + oy) * dims[0] + ox
        lo, hi = np.searchsorted(scode, want, "left"), np.searchsorted(scode, want, "right")
        cnt = hi - lo
        ends = np.cumsum(cnt)
        a0 = 0
        while a0 < len(scode):  # the bodies a0 .. a1 - 1 against their neighbour cells, about 2^22 candidates at a time
            a1 = max(a0 + 1, int(np.searchsorted(ends, ends[a0] - cnt[a0] + (1 << 22), "right")))
            c = cnt[a0:a1]
            src = np.repeat(np.arange(a0, a1), c)
            dst = np.arange(src.size) - np.repeat(np.cumsum(c) - c, c) + np.repeat(lo[a0:a1], c)
            gi, gj = idx[order[src]], idx[order[dst]]
            keep = gi < gj
            gi, gj = gi[keep], gj[keep]
            keep = friends6(pos[gi], vel[gi], pos[gj], vel[gj], link, vlink)
            out_i.append(gi[keep])
            out_j.append(gj[keep])
            a0 = a1
    return np.concatenate(out_i).astype(np.int64), np.concatenate(out_j).astype(np.int64)


def _labels_grid(pos, vel, ok, link, vlink):
    n = pos.shape[0]
    i, j = _pairs_grid(pos, vel, ok, link, vlink)
    lab = np.arange(n, dtype=np.int64)
    while True:  # every body takes the smallest label across its edges, labels then follow their own label down
        new = lab.copy()
        np.minimum.at(new, i, lab[j])
        np.minimum.at(new, j, lab[i])
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


def labels_grid(state, link, vlink):
    """fof6_grid's labels alone: F.catalogue(state, labels, link, min_members) makes the rest for any min_members."""
    return _labels_grid(state[:, 0:3], state[:, 3:6], F.body_ok(state), link, vlink)


def fof6_brute(state, link, vlink, min_members=1):
    ok = F.body_ok(state)
    return F.catalogue(state, _labels_brute(state[:, 0:3], state[:, 3:6], ok, link, vlink), link, min_members)


def fof6_grid(state, link, vlink, min_members=1):
    ok = F.body_ok(state)
    return F.catalogue(state, _labels_grid(state[:, 0:3], state[:, 3:6], ok, link, vlink), link, min_members)


def refines(fine_labels, coarse_labels):
    """Every group of fine_labels lies inside exactly one group of coarse_labels, and both leave out the same bodies."""
    if not np.array_equal(fine_labels == NONE, coarse_labels == NONE):
        return False
    ok = fine_labels != NONE
    pairs = np.unique(np.stack([fine_labels[ok], coarse_labels[ok]], axis=1), axis=0)
    return len(pairs) == len(np.unique(fine_labels[ok]))


# ---- states ------------------------------------------------------------------------------------------------

def state_of(pos, vel, seed=0):
    """float32[n, 10] with the given positions and velocities and seeded unequal masses."""
    s = F._state(pos, seed)
    s[:, 3:6] = np.asarray(vel, np.float32).reshape(len(s), 3)
    return s


def crossing_streams(m=200, spacing=0.01, jitter=0.01, seed=11):
    """Two lines of m bodies at `spacing`, along x and along y, crossing at a shared point (the origin, which body
    m // 2 of either line sits on), with velocities (1, 0, 0) and (0, 1, 0) plus `jitter`."""
    rng = np.random.default_rng(seed)
    t = (np.arange(m) - m // 2) * spacing
    pos = np.zeros((2 * m, 3))
    pos[:m, 0], pos[m:, 1] = t, t
    vel = rng.uniform(-jitter, jitter, (2 * m, 3))
    vel[:m, 0] += 1.0
    vel[m:, 1] += 1.0
    return state_of(pos, vel, seed)


def one_cell(n, layout, seed=21):
    """n bodies inside one position cell of link 1 (a cube of side 0.25 about (3, -2, 5)) at vlink 1:
      cold   -- velocities within 0.01 of each other: all friends;
      parity -- two velocity clumps 10 apart, by body parity: two groups, interleaved in every wave;
      last   -- velocities 10 apart in a line (nobody is anybody's friend), but the last body within 0.25 of body
                n // 3: one pair, found in the last lane of the last chunk."""
    rng = np.random.default_rng(seed + n)
    pos = rng.uniform(-0.125, 0.125, (n, 3)) + np.array([3.0, -2.0, 5.0])
    vel = rng.uniform(-0.005, 0.005, (n, 3))
    if layout == "parity":
        vel[1::2, 1] += 10.0
    elif layout == "last":
        vel = np.zeros((n, 3))
        vel[:, 2] = 10.0 * np.arange(n)
        vel[n - 1] = vel[n // 3] + np.array([0.25, 0.0, 0.0])
    elif layout != "cold":
        raise ValueError(layout)
    return state_of(pos, vel, seed)


def partial_joins(seed=31):
    """Link 1, vlink 1.  Cell A (100 bodies near the origin) and cell B (100 bodies 0.7 further along x -- another
    cell, within the link).  B's bodies move at (0, 0, 0) -- component B0, its even bodies -- or (0, 50, 0) -- B1, the
    odd ones.  A's bodies move at 100 + 10 k along z, friends of nobody, except body 37 of A, which moves with B0, and
    body 81, which moves with B1: {A37} + B0 and {A81} + B1 are groups, the other 98 of A singletons."""
    rng = np.random.default_rng(seed)
    pa = rng.uniform(0.0, 0.05, (100, 3))
    pb = rng.uniform(0.0, 0.05, (100, 3)) + np.array([0.7, 0.0, 0.0])
    va = np.zeros((100, 3))
    va[:, 2] = 100.0 + 10.0 * np.arange(100)
    vb = np.zeros((100, 3))
    vb[1::2, 1] = 50.0
    va[37] = (0.0, 0.0, 0.0)
    va[81] = (0.0, 50.0, 0.0)
    return state_of(np.concatenate([pa, pb]), np.concatenate([va, vb]), seed)


def gaussian_clumps(n, seed=41, sigma_x=0.05, sigma_v=0.05):
    """n bodies in three overlapping Gaussian clumps with different mean velocities, shuffled."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 3, n)
    centre = np.array([(0.0, 0.0, 0.0), (0.04, 0.0, 0.0), (0.0, 0.05, 0.02)])[k]
    drift = np.array([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, -1.0, 0.5)])[k]
    return state_of(centre + rng.normal(0.0, sigma_x, (n, 3)), drift + rng.normal(0.0, sigma_v, (n, 3)), seed)


def with_velocities(state, seed, scale):
    """`state` with seeded velocity clumps: the bodies move with one of four drifts `scale` apart, plus a tenth of it."""
    rng = np.random.default_rng(seed)
    s = state.copy()
    drift = scale * np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)], np.float64)[rng.integers(0, 4, len(s))]
    s[:, 3:6] = (drift + rng.normal(0.0, 0.1 * scale, (len(s), 3))).astype(np.float32)
    return s


def synthetic_cases(small):
    """(name, state, link, vlink): fof_ref's synthetic states under four velocity drifts, and this rule's own states."""
    out = []
    for k, (name, state, link, _) in enumerate(F.synthetic_cases(small)):
        out.append((name, with_velocities(state, 100 + k, 1.0), link, 0.5))
    out.append(("crossing_streams", crossing_streams(), 0.015, 0.5))
    for n in (63, 65, 130):
        for layout in ("cold", "parity", "last"):
            out.append((f"one_cell_{layout}_{n}", one_cell(n, layout), 1.0, 1.0))
    out.append(("partial_joins", partial_joins(), 1.0, 1.0))
    out.append(("gaussian_clumps", gaussian_clumps(1500 if small else 4096), 0.02, 0.1))
    return out
