"""A plain numpy, binary64 reference for the pair sums of the all-pairs step (test infrastructure only, like
tree_ref.py and field_ref.py): every body's stored acceleration as the sum of its pair terms, the sum of |term| per
component that a rounding bound is relative to, and the probe-mass states with which a test can tell that every
pair was counted exactly once.

Used by tests/test_naive_ref.py (this reference against the oracles, and the probe design's power, on the CPU) and
tests/test_naive_pairs_gpu.py (nb_naive.hip against this reference).

The bound.  Against the binary64 sum of the same terms, from the same binary32 positions, a component k of body i
may be off by at most

    bound = (chain + 16) x 2^-24 x sum_j |term_jk|

`chain` units (of 2^-24 = half an fp32 ulp, relative) for a sequential fp32 sum with `chain` inexact additions, and
16 for everything that happens to one term, counted to first order in the worst case: d_k = x_j - x_i' (1); r^2 from
three rounded differences, a product and two fma (3.5); v_sqrt_f32, a 1-ulp instruction (r: 3.75); r^2 r^2 and the
fma with e r (r^4 + e r: 9); v_rcp_f32, the other 1-ulp instruction (11); times m_j (12), or, inside a run of equal
masses, the one multiply of the sum by the run's mass; times d_k (13, the fma's own rounding belongs to the chain);
g dt rounded and multiplied in once per body (15).  The kernel's longest chain for a dense state is

    chain = 64 ceil(n_tiles / W) + W + 32

the 64-body tiles one of the W waves of a workgroup sums one after the other, the W - 1 additions of the cross-wave
reduction, and at most 32 partial sums of a j-split or two-phase step (pick_jsplit gives every wave at least one
tile, so a launch has at most n_tiles / W <= 11 slices at the 6,000 bodies tested and a two-phase step twice
that).  Any split only shortens a wave's run, so the figure holds for every launch shape.  In a probe state only P
bodies have mass; every other term is an exact 0 and adding 0 is exact, so chain = P.  The literal-fp32 oracle adds
j = 0 .. n-1 in order: chain = n.  Nothing here is fitted to what the GPU returns.

The probes.  With all masses 0 but P <= 8 probes (distinct masses in [0.5, 2), none a power of two) body i's sum
holds exactly the terms of the probes.  A (body, probe) pair is STRONG when in some component its term is at least
4 x the body's bound: a launch that drops that pair, or counts it twice, then misses the bound by a factor of 3 or
more whatever its rounding does.  Bodies with a pair that is not strong are left out of that argument; the seeds
are chosen so that they are at most 1 % of any probe state (a condition on the inputs).

What the old norm let through (CPU, one step, the fp32 oracle against binary64): the share of bodies whose smallest
pair term is below the existing tolerance 2e-5 max|acc| -- a dropped pair there is invisible to
max|err| / max|acc| <= 2e-5 -- and the literal-fp32 oracle's standing against `bound(., n)`.  tests/test_naive_ref.py
prints both with `-s`:

    state            bodies with a term     typical term        oracle fp32, fraction of bound(., n)
                     < 2e-5 max|acc|        / max|acc|          worst body     median body
    uniform-2          0.0 %                1.9e+00             0.227          0.220
    uniform-3          0.0 %                1.3e+00             0.139          0.088
    uniform-65         0.0 %                8.5e-03             0.059          0.025
    uniform-257       87.9 %                7.2e-04             0.054          0.010
    uniform-1337      99.3 %                5.7e-04             0.036          0.003
    spherical-3000    99.9 %                5.8e-04             0.014          0.002
    disc-3000        100.0 %                1.1e-06             0.112          0.008

Probe states (the ones the GPU tests use, every probe set of each): bodies left out 0.39 % in the worst set of
uniform-257 (one body, its weakest pair at 3.6 bounds) and none anywhere else; the weakest pair of the other
states is 10 .. 48 bounds.

Measured on an MI355X (a record, not a tolerance): the worst component of any body as a fraction of its bound, over
every launch shape of tests/test_naive_pairs_gpu.py -- all variants give the same figure to two digits.

    probes, bound(., P):   uniform-257 0.448   uniform-1025 0.296   uniform-2113 0.282   uniform-4099 0.321
                           uniform-300 0.395   uniform-700 0.295    uniform-3000 0.315   (placed ranks and runner alike)
    dense, bound(., chain): uniform-2 0.035    uniform-3 0.032      uniform-63 0.042     uniform-65 0.040
                           uniform-257 0.045 (second step 0.053)    uniform-1337 0.044   uniform-4099 0.030
                           spherical-3000 0.030 (0.023)             disc-3000 0.128      dense-core 0.016
                           wide-7.5 0.081     small-0.01 0.018      log-mass 0.062 (0.038)   tracers 0.044
                           uniform-1337 with e = 0: 0.055, with e = 1e-2: 0.030
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from tests import tree_ref
from tests.helpers import DT, E, G, make_state

EPS32 = 2.0 ** -24
PER_TERM = 16.0            # units of 2^-24 for one term's own roundings (see above)
STRONG = 4.0               # a probe's term counts when it is at least this many bounds, in some component
MAX_LEFT_OUT = 0.01        # share of a probe state's bodies that may have a pair that is not strong
J_TILE = 64                # kJTile of nb_common.hpp
PAD_TO = 256               # kPadTo: a rank's share of the bodies is a multiple of it
MAX_PARTIALS = 32


# ---- the sums -----------------------------------------------------------------------------------------------------

def _rows(out, sl, who, xi, xj, mj, cols, g, e, dt):
    with np.errstate(all="ignore"):    # (coincident distinct bodies are NaN, as in the reference)
        d = xj[None, :, :] - xi[:, None, :]
        r = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        own = cols[None, :] == who[:, None]
        r[own] = 1.0
        s = (mj[None, :] * g) / ((r * r) * r + e)
        t = (s[..., None] * (d / r[..., None])) * dt
        t[own] = 0.0
        out["acc"][sl] = t.sum(axis=1)
        out["sum_abs"][sl] = np.abs(t).sum(axis=1)
        norm = np.sqrt((t * t).sum(axis=2))
        norm[own] = np.inf
        out["min_term"][sl] = norm.min(axis=1) if norm.shape[1] else np.inf


def terms64(src, x_new, g, e, dt, cols=None, rows=None, chunk=None, x64=False):
    """The pair sums of one step in binary64.  src: the float32[n, 10] SOURCE state (old positions, masses);
    x_new: the bodies' new positions, float32[n, 3] -- the literal-fp32 oracle's, which the GPU reproduces bit for
    bit, so that the comparison measures the force and not the rounding of x' amplified by |x| / |d|; g, e, dt are
    widened from their fp32 values as oracle.naive_step_f64 does.  cols: the j summed over (default: all);
    rows: the i summed for (default: all).  (x64=True takes binary64 positions instead: only for holding this
    function against naive_step_f64, whose drift is binary64.)
    Returns dict(acc[rows, 3] -- sum over j in cols, j != i of m_j g / (r^3 + e) (d / r) dt, d = x_j - x_new_i --,
    sum_abs[rows, 3] -- the same sum of |term_k| --, min_term[rows] -- the smallest Euclidean |term| over cols, inf
    where there is none)."""
    src = np.asarray(src)
    x_new = np.asarray(x_new)
    if not x64:
        assert src.dtype == np.float32 and x_new.dtype == np.float32, "binary32 state and positions"
    n = len(src)
    cols = np.arange(n) if cols is None else np.asarray(cols, dtype=np.int64).reshape(-1)
    rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64).reshape(-1)
    g, e, dt = (float(np.float32(v)) for v in (g, e, dt))
    xj, mj = src[cols, 0:3].astype(np.float64), src[cols, 9].astype(np.float64)
    xi = x_new[rows].astype(np.float64)
    out = {"acc": np.zeros((len(rows), 3)), "sum_abs": np.zeros((len(rows), 3)), "min_term": np.full(len(rows), np.inf)}
    chunk = chunk or max(1, (1 << 19) // max(len(cols), 1))
    # (row blocks are independent and numpy releases the lock: a few threads keep the 6,000-body case short)
    with ThreadPoolExecutor(max_workers=8) as pool:
        list(pool.map(lambda i0: _rows(out, slice(i0, i0 + chunk), rows[i0:i0 + chunk], xi[i0:i0 + chunk], xj, mj,
                                       cols, g, e, dt), range(0, len(rows), chunk)))
    return out


def bound(sum_abs_k, chain):
    """(chain + 16) x 2^-24 x sum |term_k|: see the module docstring."""
    return (chain + PER_TERM) * EPS32 * np.asarray(sum_abs_k, dtype=np.float64)


def waves_of(variant_name):
    """W of a kernel variant, from its name (nb.naive_variants(): ib4_w16_kLds_pktrue_u4)."""
    for w in (8, 16):
        if f"_w{w}_" in variant_name:
            return w
    raise ValueError(f"no _w8_ / _w16_ in {variant_name!r}")


def chain_dense(n, waves):
    n_tiles = (n + J_TILE - 1) // J_TILE
    return J_TILE * ((n_tiles + waves - 1) // waves) + waves + MAX_PARTIALS


def fraction(got_acc, ref, chain):
    """|got - ref| / bound per body and component; 0 where both are 0, inf where only the bound is."""
    err = np.abs(np.asarray(got_acc, dtype=np.float64) - ref["acc"])
    b = bound(ref["sum_abs"], chain)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(b > 0.0, err / b, np.where(err == 0.0, 0.0, np.inf))


def within(got_acc, ref, chain):
    """THE criterion, per body: every component within its bound (a NaN is outside)."""
    return (fraction(got_acc, ref, chain) <= 1.0).all(axis=1)


def kick32(v, a, dt):
    """kick() of nb_naive.hip / naive.wgsl:63,66 in numpy float32: one rounding per operation."""
    return tree_ref.kick32(v, a, dt)


def rank_range(n, rank, world):
    """[lo, hi) of a rank: nb_shard_bodies_per_rank restated (shares are padded to PAD_TO bodies)."""
    per = -(-max(-(-n // world), 1) // PAD_TO) * PAD_TO
    return min(n, rank * per), min(n, (rank + 1) * per)


# ---- dense states ---------------------------------------------------------------------------------------------------

# name -> (kind, n, seed, g, e, dt); the tree_ref cases are taken by name from tree_ref.CASES
DENSE = {
    "uniform-2": ("uniform", 2, 52, G, E, DT), "uniform-3": ("uniform", 3, 53, G, E, DT),
    "uniform-63": ("uniform", 63, 54, G, E, DT), "uniform-65": ("uniform", 65, 55, G, E, DT),
    "uniform-257": ("uniform", 257, 56, G, E, DT), "uniform-1337": ("uniform", 1337, 57, G, E, DT),
    "uniform-4099": ("uniform", 4099, 58, G, E, DT),
    "spherical-3000": ("spherical", 3000, 59, G, E, DT),
    "disc-3000": ("disc", 3000, 60, 0.00001, E, 0.0016),
    "uniform-1337-e0": ("uniform", 1337, 61, G, 0.0, DT),
    "uniform-1337-e1e-2": ("uniform", 1337, 62, G, 0.01, DT),
}
TREE_CASES = ("dense-core", "wide-7.5", "small-0.01", "log-mass", "tracers")
DENSE_IDS = list(DENSE)[:9] + list(TREE_CASES) + list(DENSE)[9:]
CPU_IDS = ["uniform-2", "uniform-3", "uniform-65", "uniform-257", "uniform-1337", "spherical-3000", "disc-3000"]
TWO_STEPS = ("uniform-257", "spherical-3000", "log-mass")


def dense_state(name):
    """(float32[n, 10] source state, g, e, dt) of a dense case."""
    if name in TREE_CASES:
        case = tree_ref.CASES[tree_ref.CASE_IDS.index(name)]
        return tree_ref.case_state(case), case[5], E, case[6]
    kind, n, seed, g, e, dt = DENSE[name]
    return make_state(kind, n, seed, g), g, e, dt


# ---- probe states ---------------------------------------------------------------------------------------------------

PROBE_MASSES = np.array([0.53, 0.71, 0.89, 1.07, 1.31, 1.49, 1.73, 1.93], dtype=np.float32)

# name -> (n, seed, worlds): the base is make_state("uniform", n, seed) with a seeded non-zero a_old, so that the
# first kick has something to carry; worlds: the rank counts whose borders are probed as well
PROBE_STATES = {
    "uniform-257": (257, 71, ()), "uniform-1025": (1025, 72, ()), "uniform-2113": (2113, 73, ()),
    "uniform-4099": (4099, 74, ()),
    "uniform-300": (300, 75, (3,)),       # of 3 ranks the last owns no body, the middle one a ragged 44
    "uniform-700": (700, 76, (2, 3)),     # of 3: 256-body ranks and a tail of 188
    "uniform-3000": (3000, 77, (2, 3)),   # of 3, with 8 waves: a phase's own window (16 tiles) is itself split
}
SINGLE_IDS = [k for k, v in PROBE_STATES.items() if not v[2]]
PLACED_IDS = [k for k, v in PROBE_STATES.items() if v[2]]


def probe_base(name):
    n, seed, _world = PROBE_STATES[name]
    s = make_state("uniform", n, seed)
    rng = np.random.default_rng(seed)
    s[:, 6:9] = rng.normal(0.0, 1e-3, size=(n, 3)).astype(np.float32)
    return s


def probe_sets(name):
    """[(label, columns)]: the structural columns -- where an index mask, a tile number or a window can be off by
    one -- in sets of at most 8, and one seeded random set."""
    n, seed, worlds = PROBE_STATES[name]
    n_tiles = (n + J_TILE - 1) // J_TILE

    def keep(c):
        out = []
        for v in c:
            if 0 <= v < n and v not in out:
                out.append(int(v))
        return np.array(out[:8], dtype=np.int64)

    sets = [
        # the first tile's borders; first and last body of a 128- and a 256-wide i-tile
        ("head", keep([0, 63, 64, 65, 127, 128, 255, 256])),
        # the last real slot of the ragged tail tile, its first body, n - 64, n - 65, and the i-tile borders before it
        ("tail", keep([n - 1, n - 64, n - 65, J_TILE * (n_tiles - 1), J_TILE * (n_tiles - 1) - 1,
                       128 * ((n - 1) // 128), 256 * ((n - 1) // 256), 256 * ((n - 1) // 256) - 1])),
        # the first body of a wave's first tile (wave s of a launch starts at tile s): its run breaks at once
        ("wave-first", keep([J_TILE * s for s in (1, 7, 8, 9, 15, 16, 17, 31, 32, 33)])),
    ]
    for world in worlds:
        for r in range(world):
            lo, hi = rank_range(n, r, world)
            if hi > lo:    # the last body before and the first after lo and hi; the rank's own first i-tile
                sets.append((f"rank{r}of{world}",
                             keep([lo - 1, lo, lo + 63, lo + 64, lo + 127, lo + 128, hi - 1, hi])))
    rng = np.random.default_rng(1000 + seed)
    sets.append(("random", np.sort(rng.choice(n, size=8, replace=False)).astype(np.int64)))
    return sets


def probe_state(base, cols, shift=0):
    """`base` with every mass 0 but those of `cols`, which take the probe masses (rotated by `shift`)."""
    s = base.copy()
    s[:, 9] = 0.0
    s[cols, 9] = np.roll(PROBE_MASSES, shift)[:len(cols)]
    return s


def probe_terms(src, x_new, g, e, dt, cols, rows=None):
    """(ref, per_probe): terms64 over the probe columns, and each probe's own term, float64[P, rows, 3]."""
    ref = terms64(src, x_new, g, e, dt, cols=cols, rows=rows)
    each = np.stack([terms64(src, x_new, g, e, dt, cols=[c], rows=rows)["acc"] for c in cols])
    return ref, each


def strong_pairs(ref, each, cols, rows=None):
    """bool[rows, P]: the (body, probe) pairs whose term is at least STRONG bounds in some component.  A probe's
    pair with itself does not exist and counts as strong."""
    b = bound(ref["sum_abs"], len(cols))
    n_rows = each.shape[1]
    rows = np.arange(n_rows) if rows is None else np.asarray(rows)
    ok = (np.abs(each) >= STRONG * b[None, :, :]).any(axis=2).T
    ok |= rows[:, None] == np.asarray(cols)[None, :]
    return ok
