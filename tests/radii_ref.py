"""The rule of nb_group_radii_sim (include/nbody.h "Group radii") restated in numpy, operation by
operation: binary64 from the binary32 state, one rounding per operation; a row's members in ascending body index,
ordered by (r2, body index) with `lexsort`; the enclosed mass as three levels of `reshape` and `cumsum` (runs of 64,
chunks of 64 runs, the chunks of a row); the crossings as the first rank at which the predicate holds, taken over
every rank; the largest M / r with ties to the smaller rank.  The centre of a row without a given one is round 0 of
nb_sim_group_shapes (tests/shape_ref.py's run_sums: runs of 64 through the butterfly, added in order from 0).

radii_ref() returns the rows, rank_of, enclosed_of and the stats.  `tie`, `one_cumsum` and `skip` exist for the
mutation check of tests/test_radii.py alone: each switches one clause of the rule off."""
import numpy as np

NONE = 0xFFFFFFFF
RUN, CHUNK, MAX_F = 64, 4096, 16
ROW_DTYPE = np.dtype([("count", "<u4"), ("vmax_index", "<u4"), ("center", "<f8", (3,)), ("mass", "<f8"),
                      ("r_min", "<f8"), ("r_max", "<f8"), ("vc2_max", "<f8"), ("r_vmax", "<f8"),
                      ("radius", "<f8", (MAX_F,)), ("index", "<u4", (MAX_F,))])
# |M(s) - the exact prefix sum| <= bound_units(count) * 2^-53 * sum |m_j| (DESIGN.md 6o "The bound")
EPS = 2.0 ** -53


def bound_units(count):
    return 130.0 + count / CHUNK


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


def com(x, mass):
    """Round 0 of nb_sim_group_shapes over a row's list: c = (sum m x) / (sum m)."""
    sums = run_sums(np.concatenate([mass[:, None], mass[:, None] * (x - 0.0)], axis=1))
    with np.errstate(all="ignore"):
        return sums[1:4] / sums[0]


def enclosed(mass, one_cumsum=False):
    """M(s) of the masses in rank order: (A(c) + B(k)) + C(s)."""
    count = len(mass)
    if count == 0 or one_cumsum:
        return np.cumsum(mass)
    nchunks = (count + CHUNK - 1) // CHUNK
    x = np.zeros(nchunks * CHUNK)
    x[:count] = mass
    c = np.cumsum(x.reshape(nchunks, RUN, RUN), axis=2)          # C: left to right inside a run
    last = np.minimum(count - (np.arange(nchunks * RUN) * RUN), RUN).reshape(nchunks, RUN) - 1  # a run's last member
    t = np.take_along_axis(c, np.maximum(last, 0)[:, :, None], axis=2)[:, :, 0]
    t = np.where(last >= 0, t, 0.0)                               # T: C at the run's last member (+0: no run)
    b = np.cumsum(np.concatenate([np.zeros((nchunks, 1)), t[:, :-1]], axis=1), axis=1)  # B(k) = B(k-1) + T(k-1) from 0
    runs_in = np.minimum((count - np.arange(nchunks) * CHUNK + RUN - 1) // RUN, RUN) - 1  # a chunk's last run
    ar = np.arange(nchunks)
    total = b[ar, runs_in] + t[ar, runs_in]                       # B(last run) + T(last run)
    a = np.cumsum(np.concatenate([[0.0], total[:-1]]))            # A(c) = A(c-1) + total(c-1) from 0
    m_of = (a[:, None, None] + b[:, :, None]) + c
    return m_of.reshape(-1)[:count]


def radii_ref(state, group_of, m, fractions=(0.1, 0.5, 0.9), centers=None, vmax_skip=10, tie=True, one_cumsum=False,
              skip=True):
    state = np.asarray(state, np.float32).reshape(-1, 10)
    n = state.shape[0]
    group_of = np.asarray(group_of, np.uint32).reshape(-1)
    fractions = np.asarray(fractions, np.float64)
    nf = len(fractions)
    ok = body_ok(state)
    x, mass = state[:, 0:3].astype(np.float64), state[:, 9].astype(np.float64)
    rows = np.zeros(m, ROW_DTYPE)
    rank_of = np.full(n, NONE, np.uint32)
    enclosed_of = np.full(n, np.nan)
    has_row = group_of != NONE
    stats = dict(n=n, rows=m, members=int((has_row & ok).sum()) if m else 0,
                 nonfinite_members=int((has_row & ~ok).sum()), empty=0)
    for r in range(m):
        o = rows[r]
        idx = np.flatnonzero((group_of == r) & ok)  # ascending body index
        count = len(idx)
        o["count"] = count
        for f in ("r_min", "r_max", "vc2_max", "r_vmax"):
            o[f] = np.nan
        o["radius"][:] = np.nan
        o["index"][:] = NONE
        o["vmax_index"] = NONE
        if centers is not None:
            c = np.asarray(centers, np.float64).reshape(-1, 3)[r]
        elif count:
            c = com(x[idx], mass[idx])
        else:
            c = np.full(3, np.nan)
        o["center"] = c
        if count == 0:
            stats["empty"] += 1
            continue
        with np.errstate(all="ignore"):
            d = x[idx] - c
            r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            order = np.lexsort((idx, r2)) if tie else np.lexsort((-idx.astype(np.int64), r2))
            body, r2s, ms = idx[order], r2[order], mass[idx][order]
            big_m = enclosed(ms, one_cumsum)
            rank_of[body] = np.arange(count, dtype=np.uint32)
            enclosed_of[body] = big_m
            total = big_m[-1]
            o["mass"] = total
            o["r_min"], o["r_max"] = np.sqrt(r2s[0]), np.sqrt(r2s[-1])
            for k in range(nf):
                hit = np.flatnonzero(big_m >= fractions[k] * total)  # the predicate at every rank, the smallest
                if len(hit):
                    o["radius"][k] = np.sqrt(r2s[hit[0]])
                    o["index"][k] = body[hit[0]]
            ranks = np.arange(count)
            xs = big_m / np.sqrt(r2s)
            cand = (r2s > 0.0) & ~np.isnan(xs)
            if skip:
                cand &= ranks >= vmax_skip
            if cand.any():
                best = np.flatnonzero(cand & (xs == xs[cand].max()))[0]  # the smallest rank among equals
                o["vc2_max"], o["r_vmax"], o["vmax_index"] = xs[best], np.sqrt(r2s[best]), body[best]
    return dict(rows=rows, rank_of=rank_of, enclosed_of=enclosed_of, stats=stats)


# ---- states -------------------------------------------------------------------------------------------------------
def cloud(rng, n, centre=(0.0, 0.0, 0.0), scale=1.0, equal_mass=False):
    """float32[n, 10]: an isotropic Gaussian about `centre`, masses U[0.5, 2] (or all 1)."""
    s = np.zeros((n, 10), np.float32)
    s[:, 0:3] = rng.normal(0.0, scale, (n, 3)) + np.asarray(centre)
    s[:, 3:6] = rng.normal(0.0, 0.05, (n, 3))
    s[:, 9] = 1.0 if equal_mass else rng.uniform(0.5, 2.0, n)
    return s


def dyadic(rng, n, centre=(0.0, 0.0, 0.0)):
    """float32[n, 10] whose sums are all exact: coordinates multiples of 1/8 in [-4, 4], masses multiples of 2^-10 in
    (0, 2] -- many exact ties in r2."""
    s = np.zeros((n, 10), np.float32)
    s[:, 0:3] = rng.integers(-32, 33, (n, 3)) / 8.0 + np.asarray(centre)
    s[:, 9] = rng.integers(1, 2049, n) / 1024.0
    return s


def assemble(rng, parts, loose=0, shuffle=True, extra_rows=0):
    """(state, group_of, m): part k is row k, then `extra_rows` empty rows; `loose` bodies of no row; shuffled."""
    state = np.concatenate(list(parts) + [cloud(rng, loose, centre=(50.0, 0.0, 0.0))])
    gof = np.concatenate([np.full(len(p), k, np.uint32) for k, p in enumerate(parts)] + [np.full(loose, NONE, np.uint32)])
    if shuffle:
        perm = rng.permutation(len(state))
        state, gof = state[perm], gof[perm]
    return np.ascontiguousarray(state), np.ascontiguousarray(gof), len(parts) + extra_rows
