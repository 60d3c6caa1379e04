"""fp64 host restatement of the tidal tensor probes' rule (include/nbody.h "Tidal tensor probes"):
the gradient of the all-pairs acceleration of a state at arbitrary points, the coincident counts, and the sums of
|term| the derived error bound is relative to; the point sets the device tests use; and the wrong rules the bound
must be able to tell from the right one.  It lives with the tests on purpose: the package has no CPU path for it."""
import numpy as np

from tests.diag_ref import body_mask
from tests.helpers import make_state

RUN = 64                                   # R: pairs summed in fp32 before the fold into fp64
K = 33                                     # NB_TIDAL_K: the roundings of the pair form, weighted
BOUND = (RUN + K) * 2.0 ** -24             # per sum, of g sum |term|
SUMS = ("xx", "yy", "zz", "xy", "xz", "yz", "w")
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))   # the order of nb_tidal_sample.tensor

# the wrong rules of tests/test_tidal.py's mutation test
MUTATIONS = ("3r3", "no_e", "no_w", "swap_xz_yz", "flip_xy")


def tidal64(state, points, g, e, mutation=None, rows=None):
    """dict: tensor6 (M, 6) in the order xx, yy, zz, xy, xz, yz, tensor (M, 3, 3), sums (M, 7) = g S_ab and g W,
    scales (M, 7) = g sum |term| per sum, bound6 (M, 6) = the bound of each tensor component (a diagonal gets the
    bounds of S_aa and W), trace_direct (M,) = g sum m (r^3 - 2 e) / (r (r^3 + e)^2), coincident (M,), nonfinite.
    g and e are taken as the fp32 values the simulator holds; d = x_j - p from the fp32 coordinates (exact in
    fp64); a body with d == 0 is coincident and adds nothing.  mutation: one of MUTATIONS, a wrong rule."""
    s = np.asarray(state, dtype=np.float32)
    ok = body_mask(s)
    x, m = s[ok, 0:3].astype(np.float64), s[ok, 9].astype(np.float64)
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    g, e = np.float64(np.float32(g)), np.float64(np.float32(e))
    M, n = p.shape[0], x.shape[0]
    sums, scales = np.zeros((M, 7)), np.zeros((M, 7))
    coincident, trace = np.zeros(M, np.int64), np.zeros(M)
    rows = rows or max(1, (1 << 21) // max(n, 1))
    for i0 in range(0, M, rows):
        sl = slice(i0, i0 + rows)
        with np.errstate(all="ignore"):  # (a non-finite point is NaN throughout; said so below)
            d = [x[None, :, k] - p[sl, None, k] for k in range(3)]
            r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
            co = r2 == 0.0
            r2[co] = 1.0
            r = np.sqrt(r2)
            r3 = r2 * r
            w = m[None, :] / (r2 * r2 + e * r)
            c = ((3.0 if mutation == "3r3" else 4.0) * r3 + (0.0 if mutation == "no_e" else e)) / (r2 * (r3 + e))
            w[co] = 0.0
            coincident[sl] = co.sum(axis=1)
            for f, (a, b) in enumerate(PAIRS):
                t = w * c * d[a] * d[b]
                sums[sl, f], scales[sl, f] = g * t.sum(axis=1), g * np.abs(t).sum(axis=1)
            sums[sl, 6], scales[sl, 6] = g * w.sum(axis=1), g * np.abs(w).sum(axis=1)
            t = m[None, :] * (r3 - 2.0 * e) / (r * (r3 + e) ** 2)
            t[co] = 0.0
            trace[sl] = g * t.sum(axis=1)
    t6 = sums[:, :6].copy()
    if mutation != "no_w":
        t6[:, :3] -= sums[:, 6:7]
    if mutation == "swap_xz_yz":
        t6[:, [4, 5]] = t6[:, [5, 4]]
    if mutation == "flip_xy":
        t6[:, 3] = -t6[:, 3]
    bound6 = BOUND * scales[:, :6]
    bound6[:, :3] += BOUND * scales[:, 6:7]
    bad = ~np.isfinite(p).all(axis=1)
    for a in (t6, sums, scales, bound6, trace):
        a[bad] = np.nan
    coincident[bad] = 0
    return {"tensor6": t6, "tensor": t6[:, [0, 3, 4, 3, 1, 5, 4, 5, 2]].reshape(-1, 3, 3), "sums": sums,
            "scales": scales, "bound6": bound6, "trace_direct": trace, "coincident": coincident,
            "nonfinite": int((~ok).sum()), "nonfinite_points": int(bad.sum())}


def points(state, m, seed, e):
    """Half of the points on bodies (the first half, rounded up), as tests/test_field_gpu.py's; of the other half
    every second one within e^(1/3) of a body -- there the e of the numerator of c matters -- and the rest random
    in the bodies' box.  (points, on): `on` leads."""
    rng = np.random.default_rng(seed)
    pts = np.empty((m, 3), np.float32)
    n = state.shape[0]
    if n == 0:
        pts[:] = rng.uniform(-1.0, 1.0, size=(m, 3)).astype(np.float32)
        return pts, 0
    on = (m + 1) // 2
    pts[:on] = state[rng.integers(0, n, size=on), 0:3]
    lo, hi = state[:, 0:3].min(0) - 0.1, state[:, 0:3].max(0) + 0.1
    pts[on:] = rng.uniform(lo, hi, size=(m - on, 3)).astype(np.float32)
    near = np.arange(on, m, 2)
    u = rng.normal(size=(near.size, 3))
    u *= (rng.uniform(0.1, 0.9, size=near.size) * np.float64(e) ** (1.0 / 3.0) / np.sqrt((u * u).sum(1)))[:, None]
    pts[near] = (state[rng.integers(0, n, size=near.size), 0:3].astype(np.float64) + u).astype(np.float32)
    return pts, on


def plan(m, n, ib=None):
    """(ib, cj, chunks) of a call with m points on n bodies: the plan of csrc/nb_probe.hpp restated -- points per
    lane (nb_tidal.hip's, unless the caller gives nb_field.hip's), 256-body tiles per chunk (the iterations of a
    block's double-buffered loop), chunks (blockIdx.y)."""
    if ib is None:
        ib = 4 if m >= 256 else 2 if m > 64 else 1
    tile_pts = 64 * ib
    p_tiles, n_tiles = -(-m // tile_pts), -(-n // 256)
    if m == 0 or n == 0:
        return ib, 0, 0
    wide = min(p_tiles, max(1, (1 << 35) // (tile_pts * n)))
    want = min(n_tiles, max(1, -(-1024 // wide)))
    cj = -(-n_tiles // want)
    return ib, cj, -(-n_tiles // cj)


# (M, N) of the device tests -- every points-per-lane instantiation with a ragged last tile, a ragged last body tile,
# one and 17 chunks.  Every one of them has one tile per chunk (the bodies are cut into up to 1,024 chunks before a
# chunk gets a second tile): the double-buffered loop runs more than once only in DEEP below
SHAPES = [(1, 4099), (63, 255), (64, 256), (65, 257), (255, 1), (256, 2), (257, 0), (600, 1000), (600, 4099)]
assert {m for m, _ in SHAPES} == {1, 63, 64, 65, 255, 256, 257, 600}
assert {n for _, n in SHAPES} == {0, 1, 2, 255, 256, 257, 1000, 4099}
assert all(plan(m, n)[1] <= 1 for m, n in SHAPES)
INITS = ["uniform", "disc", "spherical"]
# (M, N) -> (ib, cj, chunks): two, three and four tiles per chunk, at each points-per-lane instantiation; the last tile
# of each N is ragged but for 2^20
DEEP = {(5, 300_000): (1, 2, 586), (5, 600_000): (1, 3, 782), (5, 1 << 20): (1, 4, 1024), (65, 300_000): (2, 2, 586),
        (257, 140_000): (4, 2, 274)}
assert all(plan(m, n) == v for (m, n), v in DEEP.items())


def shape_case(idx, e):
    """(state, points, on) of SHAPES[idx]: the initial state the device test makes its simulators from."""
    m, n = SHAPES[idx]
    state = make_state(INITS[idx % 3], n, seed=60 + idx) if n else np.zeros((0, 10), np.float32)
    pts, on = points(state, m, seed=idx, e=e)
    return state, pts, on
