"""nb_sim_halo_profiles on the device (csrc/nb_halo.hip) against the numpy restatement of its rule
(tests/halo_ref.py, brute force over all bodies, no cells) and against nb_sim_radial_profile about the same centre:
every count, inside_count and integer of the stats equal, every sum within 1e-10 of its sum of |term| of the
binary64 sum (2e-10 between the two device passes).  The smallest shapes that can go wrong, the work-item border,
the bodies a wrong prune would lose, the invariants of the sum order, the refusals, that a call does not perturb the
trajectory; the wrapper, group_profiles, the runner, the C++ mirror and the CLI.  `-m gpu`."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from tests import halo_ref as H
from tests.helpers import ROOT, make_state

pytestmark = pytest.mark.gpu

TOL = 1e-10
FILL = 0xA5
STATS = ("n", "nonfinite", "centers", "tested", "items")
L = H.CHUNK


def _sim(nb, kind, state, theta=0.75):
    sp = nb.SimParams(particle_num=state.shape[0])
    if kind == "naive":
        return nb.NaiveSim.from_particles(sp, None, state)
    return nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(theta), state)


def _state_of(nb, sim):
    return nb.as_floats(sim.read_particles()).copy()


def _prepared(nb, kind, state):
    """A simulator and the state its passes see: a TreeSim after one step (its bodies reordered)."""
    sim = _sim(nb, kind, state)
    if kind == "tree":
        sim.encode()
        state = _state_of(nb, sim)
    return sim, state


def _state(x, v=None, m=None):
    x = np.asarray(x, dtype=np.float32).reshape(-1, 3)
    s = np.zeros((x.shape[0], 10), np.float32)
    s[:, 0:3] = x
    s[:, 3:6] = 0.0 if v is None else v
    s[:, 9] = 1.0 if m is None else m
    return s


def _raw(sim, edges, centers=None, bodies=None, velocities=None, m=None, want=(True, True), call=None, handle=None,
         nbins=None):
    """The C call with every buffer pre-filled and one row more than it may write."""
    from wgpu_n_body_amd import _lib
    dp = C.POINTER(C.c_double)
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    p = _lib.nb_halo_params()
    p.nbins = edges.shape[0] - 1 if nbins is None else nbins
    p.edges = edges.ctypes.data_as(dp)
    keep = [edges]
    if centers is not None:
        keep.append(np.ascontiguousarray(centers, dtype=np.float64).reshape(-1, 3))
        p.centers = keep[-1].ctypes.data_as(dp)
        count = keep[-1].shape[0]
    if bodies is not None:
        keep.append(np.ascontiguousarray(bodies, dtype=np.uint32))
        p.bodies = keep[-1].ctypes.data_as(C.POINTER(C.c_uint32))
        count = keep[-1].shape[0]
    if velocities is not None:
        keep.append(np.ascontiguousarray(velocities, dtype=np.float64).reshape(-1, 3))
        p.velocities = keep[-1].ctypes.data_as(dp)
    if centers is None and bodies is None:
        count = 0
    p.m = count if m is None else m
    # (a count without arrays is a refusal under test: a few rows to show that nothing is written)
    rows, nb_ = int(p.m) if m is None else int(min(p.m, 1 << 12)), max(int(p.nbins), 1)
    heads = np.frombuffer(bytes([FILL]) * (64 * (rows + 1)), dtype=_lib.HALO_HEAD_DTYPE).copy()
    bins = np.frombuffer(bytes([FILL]) * (88 * (rows + 1) * nb_), dtype=_lib.RADIAL_BIN_DTYPE).copy()
    st = _lib.nb_halo_stats()
    rc = (call or _lib.lib().nb_sim_halo_profiles)(handle or sim._h, C.byref(p), heads.ctypes.data if want[0] else None,
                                                   bins.ctypes.data if want[1] else None, C.byref(st))
    return SimpleNamespace(rc=rc, heads=heads[:rows], bins=bins[:rows * nb_].reshape(rows, nb_), st=st,
                           tail=heads[rows:].tobytes() + bins[rows * nb_:].tobytes(),
                           all=heads.tobytes() + bins.tobytes(), bytes=heads.tobytes() + bins.tobytes() + bytes(st))


def _halo(sim, edges, **kw):
    from wgpu_n_body_amd import _lib
    g = _raw(sim, edges, **kw)
    assert g.rc == 0, _lib.lib().nb_last_error()
    assert set(g.tail) == {FILL}  # nothing beyond m rows
    return g


def _check(g, ref, rows=None, stats=True):
    """Every integer equal, every sum within TOL of its sum of |term|; rows: the reference's rows the call was
    given (default: all).  Returns the worst error in units of the bound."""
    sel = np.arange(ref["centers"]) if rows is None else np.asarray(rows)
    if stats:
        for k in STATS:
            assert getattr(g.st, k) == ref[k], (k, getattr(g.st, k), ref[k])
        assert tuple(g.st.cells) == tuple(ref["cells"])
    assert np.array_equal(g.bins["count"], ref["count"][sel]), np.argwhere(g.bins["count"] != ref["count"][sel])[:8]
    assert np.array_equal(g.heads["inside_count"], ref["inside_count"][sel])
    assert np.array_equal(g.heads["flags"], ref["flags"][sel])
    assert np.array_equal(g.heads["center"], ref["center"][sel])
    assert np.array_equal(g.heads["velocity"], ref["velocity"][sel])
    assert not g.bins["m_uphi"].any() and not g.bins["m_uphi2"].any()
    worst = 0.0
    for name in H.SUMS + ("inside_mass",):
        got = g.heads[name] if name == "inside_mass" else g.bins[name]
        d, s = np.abs(got - ref[name][sel]), ref["scale"][name][sel]
        assert np.all(d <= TOL * s), (name, float((d / (s + 1e-300)).max()))
        assert not got[s == 0].any(), name  # a sum without terms is 0, not merely small
        worst = max(worst, float((d[s > 0] / s[s > 0]).max()) if (s > 0).any() else 0.0)
    return worst / TOL


def _check_radial(sim, g, edges, rows, ref, ref_rows=None):
    """nb_sim_radial_profile about the same explicit centre, velocity and edges: counts and inside_count equal, the
    sums within 2e-10 of their sum of |term| (the reference's) of each other."""
    for j in rows:
        k = j if ref_rows is None else ref_rows[j]
        h = g.heads[j]
        r = sim.radial_profile(edges, center=h["center"], velocity=h["velocity"])
        b = g.bins[j]
        assert np.array_equal(b["count"], r.count) and h["inside_count"] == r.inside_count
        assert abs(h["inside_mass"] - r.inside_mass) <= 2 * TOL * ref["scale"]["inside_mass"][k]
        assert np.array_equal(r.center, h["center"]) and np.array_equal(r.velocity, h["velocity"])
        for name, other in (("mass", r.bin_mass), ("m_r", r.m_r), ("m_ur", r.m_ur), ("m_ur2", r.m_ur2),
                            ("m_u2", r.m_u2), ("ang", r.ang)):
            assert np.all(np.abs(b[name] - other) <= 2 * TOL * ref["scale"][name][k]), name


EDGES = np.array([0.02, 0.05, 0.11, 0.2, 0.33])


# ---- the smallest states ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["naive", "tree"])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_tiny_states(gpu, kind, n):
    nb = gpu
    base = make_state("spherical", 8, seed=1)[:n]
    base[:, 0:3] *= 0.1 / max(np.abs(base[:, 0:3]).max(), 1e-30)
    sim, state = _prepared(nb, kind, base)
    x = state[:, 0:3].astype(np.float64)
    for edges in (EDGES, np.array([0.0, 0.05, 0.4])):
        for c in (x[0], x[0] + [0.03, 0.0, 0.0], [5.0, 5.0, 5.0]):
            g = _halo(sim, edges, centers=[c], velocities=[[0.01, 0.0, -0.02]])
            _check(g, H.halo_ref(state, edges, centers=[c], velocities=[[0.01, 0.0, -0.02]]))
        g = _halo(sim, edges, bodies=[n - 1])  # r = 0, u = 0: u_r = 0 and the body is counted
        ref = H.halo_ref(state, edges, bodies=[n - 1])
        _check(g, ref)
        assert g.heads["inside_count"][0] + g.bins["count"][0].sum() >= 1
        if edges[0] == 0.0 and n == 1:
            assert g.bins["count"][0, 0] == 1 and g.bins["m_ur"][0, 0] == 0.0 and g.bins["m_r"][0, 0] == 0.0
    sim.destroy()


@pytest.fixture(scope="module")
def sized():
    """Per n: the state, 1,025 centres (bodies' neighbourhoods, random points, outside points) and the reference
    over all of them, computed once: a centre's row does not depend on m."""
    cache = {}

    def get(n):
        if n not in cache:
            state = make_state("spherical", n, seed=n)
            state[:, 0:3] *= 0.5 / np.abs(state[:, 0:3]).max()
            rng = np.random.default_rng(n)
            x = state[:, 0:3].astype(np.float64)
            c = np.concatenate([x[rng.integers(0, n, 600)] + rng.normal(scale=0.02, size=(600, 3)),
                                rng.uniform(-0.6, 0.6, (400, 3)), rng.uniform(-3, 3, (25, 3))])
            vc = rng.normal(scale=0.05, size=(1025, 3))
            cache[n] = (state, c, vc, H.halo_ref(state, EDGES, centers=c, velocities=vc))
        return cache[n]

    return get


@pytest.mark.parametrize("n", [255, 256, 257, 4097])
def test_sizes(gpu, sized, n):
    nb = gpu
    state, c, vc, ref = sized(n)
    sim = _sim(nb, "naive", state)
    worst = 0.0
    for m in (1, 2, 255, 257, 1025):
        g = _halo(sim, EDGES, centers=c[:m], velocities=vc[:m])
        worst = max(worst, _check(g, ref, rows=np.arange(m), stats=False))
        T = ref["candidates"][:m]
        assert (g.st.n, g.st.centers, g.st.nonfinite) == (n, m, 0) and tuple(g.st.cells) == tuple(ref["cells"])
        assert g.st.tested == int(T.sum()) and g.st.items == int(((T + L - 1) // L).sum())
    _check_radial(sim, g, EDGES, [0, 3, 599, 700, 1024], ref)
    print(f"n={n}: worst error {worst:.3g} of the bound")
    sim.destroy()


def test_tree_after_a_step(gpu):
    nb = gpu
    sim, state = _prepared(nb, "tree", make_state("disc", 4097, seed=3))
    x = state[:, 0:3].astype(np.float64)
    edges = np.array([0.0, 0.01, 0.03, 0.08])
    bodies = np.arange(0, 4097, 64)
    g = _halo(sim, edges, bodies=bodies)
    ref = H.halo_ref(state, edges, bodies=bodies)
    _check(g, ref)
    # the body form is the point form at the body's widened position and velocity, bit for bit
    p = _halo(sim, edges, centers=x[bodies], velocities=state[bodies, 3:6].astype(np.float64))
    assert p.all == g.all and bytes(p.st) == bytes(g.st)
    _check_radial(sim, g, edges, [0, 17, 64], ref)
    sim.destroy()


# ---- the work-item border -----------------------------------------------------------------------------------
@pytest.mark.parametrize("total", [L - 1, L, L + 1, 2 * L + 1])
def test_candidate_totals_at_the_chunk_border(gpu, total):
    """A lattice of spacing 1/32 in one grid cell (R exceeds its extent): T = n for a centre inside, and the counts
    follow from integers."""
    nb = gpu
    i = np.arange(total)
    p = np.stack([i % 16, (i // 16) % 16, i // 256], axis=1)
    state = _state(p / 32.0, v=np.stack([p[:, 1], -p[:, 0], p[:, 2]], axis=1) / 64.0, m=1.0 + (i % 3))
    sim = _sim(nb, "naive", state)
    edges_i = np.array([1, 4, 9, 40])
    ci = np.array([[8, 8, 2], [0, 0, 0], [15, 3, 9]])
    g = _halo(sim, edges_i / 32.0, centers=ci / 32.0)
    ref = H.halo_ref(state, edges_i / 32.0, centers=ci / 32.0)
    _check(g, ref)
    assert tuple(g.st.cells) == (1, 1, 1) and g.st.tested == 3 * total and g.st.items == 3 * ((total + L - 1) // L)
    for j in range(3):
        r2 = ((p - ci[j]) ** 2).sum(1)
        assert g.bins["count"][j].tolist() == [int(((r2 >= a * a) & (r2 < b * b)).sum())
                                               for a, b in zip(edges_i[:-1], edges_i[1:])]
        assert g.heads["inside_count"][j] == int((r2 < 1).sum())
    assert g.bins["count"][0].sum() + g.heads["inside_count"][0] == total  # the sphere holds every body
    _check_radial(sim, g, edges_i / 32.0, [0, 2], ref)
    sim.destroy()


# ---- what a wrong prune loses ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["face", "edge", "corner"])
def test_bodies_at_exactly_R_across_a_cell_border(gpu, case):
    """Cells of side h = R with lo = 0: a body on the lattice point 3h (cell 3) or one binary32 step below it (cell
    2), a centre in the neighbouring cell across a face, an edge or a corner at exactly R (dyadic offsets: r2 = R^2
    without rounding; out) and one binary64 step nearer (in) or further (out)."""
    nb = gpu
    R, d = {"face": (1.0, [1.0, 0.0, 0.0]), "edge": (0.625, [0.375, 0.5, 0.0]),
            "corner": (0.75, [0.25, 0.5, 0.5])}[case]
    d = np.array(d)
    rng = np.random.default_rng(8)
    B = np.full(3, 3 * R, dtype=np.float32)
    Bl = np.where(d > 0, np.nextafter(B, np.float32(0)), B).astype(np.float32)
    filler = rng.uniform(0, 8 * R, (500, 3)).astype(np.float32)
    x = np.concatenate([[B], [Bl], [[0, 0, 0]], [np.full(3, 8 * R)], filler]).astype(np.float32)
    state = _state(x, v=rng.normal(size=(x.shape[0], 3)))
    edges = np.array([R / 4, R / 2, R])
    centres = []
    for body, sign in ((B.astype(np.float64), -1.0), (Bl.astype(np.float64), +1.0)):
        c0 = body + sign * d  # exact: dyadic
        a = int(np.argmax(d > 0))
        near, far = c0.copy(), c0.copy()
        near[a] = np.nextafter(c0[a], body[a])
        far[a] = np.nextafter(c0[a], c0[a] + sign)
        centres += [c0, near, far]
    centres = np.array(centres)
    ref = H.halo_ref(state, edges, centers=centres)
    g0 = H.grid64(state, edges)
    assert g0["h"] == R and g0["lo"].tolist() == [0, 0, 0] and g0["cells"] == (9, 9, 9)
    q = H.cells64(g0, x[:2].astype(np.float64))
    assert q[0].tolist() == [3, 3, 3] and q[1].tolist() == [2 if di > 0 else 3 for di in d]
    # the reference itself: the body is out at exactly R and one step further, in one step nearer
    tot = ref["count"].sum(1) + ref["inside_count"]
    assert tot[1] == tot[0] + 1 and tot[2] <= tot[0] and tot[4] == tot[3] + 1 and tot[5] <= tot[3]
    sim = _sim(nb, "naive", state)
    g = _halo(sim, edges, centers=centres)
    _check(g, ref)
    _check_radial(sim, g, edges, range(6), ref)
    sim.destroy()


def test_centres_on_borders_outside_and_around(gpu):
    nb = gpu
    rng = np.random.default_rng(12)
    x = rng.uniform(-1, 1, (3000, 3)).astype(np.float32)
    state = _state(x, v=rng.normal(size=(3000, 3)), m=rng.uniform(0.5, 2, 3000))
    R = 0.25
    edges = np.array([0.0, 0.05, 0.1, R])
    g0 = H.grid64(state, edges)
    lo, hi, h = g0["lo"], g0["hi"], g0["h"]
    on_borders = [lo + h * np.array(k) for k in ([1, 1, 1], [2, 0, 3], [0, 0, 0], [3, 3.5, 1])]
    c = np.array(on_borders + [lo, hi, [lo[0], hi[1], 0.0],
                               [hi[0] + 2 * R, 0, 0], [0, lo[1] - R, 0], [0, 0, hi[2] + R],       # wholly outside
                               [hi[0] + R / 2, 0, 0], [lo[0] - R / 2, lo[1] - R / 2, 0],          # half inside
                               [hi[0] + R * (1 - 2.0 ** -50), 0.3, 0.3], [1e30, 0, 0], [0, -1e300, 0]])
    ref = H.halo_ref(state, edges, centers=c)
    sim = _sim(nb, "naive", state)
    g = _halo(sim, edges, centers=c)
    _check(g, ref)
    for j in (7, 8, 9, 13, 14):
        assert ref["candidates"][j] == 0 and not g.bins["count"][j].any() and g.heads["inside_count"][j] == 0
    assert g.bins["count"][10].sum() > 0 and g.bins["count"][11].sum() > 0
    _check_radial(sim, g, edges, [0, 2, 4, 5, 10], ref)
    # a sphere that holds every body: one cell, every body a candidate of every centre
    big = np.array([0.5, 1.0, 2.0, 4.0])
    g = _halo(sim, big, centers=[[0, 0, 0], [0.5, 0.5, 0.5]])
    ref = H.halo_ref(state, big, centers=[[0, 0, 0], [0.5, 0.5, 0.5]])
    _check(g, ref)
    assert tuple(g.st.cells) == (1, 1, 1) and g.st.tested == 6000
    assert g.bins["count"][0].sum() + g.heads["inside_count"][0] == 3000
    sim.destroy()


def test_degenerate_geometries(gpu):
    nb = gpu
    # all bodies at one point: zero extents, one cell
    state = _state(np.tile(np.float32([0.3, -0.2, 0.1]), (300, 1)), v=np.random.default_rng(1).normal(size=(300, 3)))
    sim = _sim(nb, "naive", state)
    for edges in (np.array([0.0, 0.1, 0.2]), np.array([0.05, 0.1, 0.2])):
        c = [state[0, 0:3].astype(np.float64), [0.3, -0.2, 0.25], [0.3, -0.2, 0.31]]
        g = _halo(sim, edges, centers=c)
        _check(g, H.halo_ref(state, edges, centers=c))
        assert tuple(g.st.cells) == (1, 1, 1)
        gb = _halo(sim, edges, bodies=[299, 0])
        _check(gb, H.halo_ref(state, edges, bodies=[299, 0]))
        assert gb.heads["inside_count"][0] + gb.bins["count"][0, 0] == 300 and gb.bins["m_ur"][0, 0] == 0.0
    sim.destroy()
    # one outlier 2^20 times further out than the rest
    rng = np.random.default_rng(2)
    x = rng.uniform(-1, 1, (1000, 3)).astype(np.float32)
    x[500] = [2.0 ** 20, 0, 0]
    state = _state(x)
    sim = _sim(nb, "naive", state)
    edges = np.array([0.0, 0.1, 0.3])
    c = np.concatenate([x[:5].astype(np.float64), [x[500].astype(np.float64)], [[2.0 ** 20 - 0.2, 0, 0]]])
    g = _halo(sim, edges, centers=c)
    ref = H.halo_ref(state, edges, centers=c)
    _check(g, ref)
    assert g.st.cells[0] == 1024 and g.bins["count"][5, 0] == 1 and g.bins["count"][6].tolist() == [0, 1]
    sim.destroy()


def test_nonfinite_bodies_and_empty_calls(gpu):
    nb = gpu
    from wgpu_n_body_amd import _lib
    state = make_state("spherical", 600, seed=5)
    state[:, 0:3] *= 0.5 / np.abs(state[:, 0:3]).max()
    state[3, 0], state[77, 4], state[300, 9], state[599, 2] = np.nan, np.inf, np.nan, -np.inf
    sim = _sim(nb, "naive", state)
    bodies = [0, 3, 77, 5, 300, 599, 598]
    g = _halo(sim, EDGES, bodies=bodies)
    ref = H.halo_ref(state, EDGES, bodies=bodies)
    _check(g, ref)
    assert g.st.nonfinite == 4 and g.heads["flags"].tolist() == [0, 1, 1, 0, 1, 1, 0]
    for j in (1, 2, 4, 5):  # a zeroed row
        assert g.heads[j].tobytes() == np.array([(0, 1, 0.0, [0] * 3, [0] * 3)], _lib.HALO_HEAD_DTYPE).tobytes()
        assert set(g.bins[j].tobytes()) == {0}
    g = _halo(sim, EDGES, bodies=bodies, velocities=np.ones((7, 3)))
    _check(g, H.halo_ref(state, EDGES, bodies=bodies, velocities=np.ones((7, 3))))
    x = state[:, 0:3].astype(np.float64)
    g = _halo(sim, EDGES, centers=x[[0, 5, 10]])
    _check(g, H.halo_ref(state, EDGES, centers=x[[0, 5, 10]]))
    # no body counts at all
    bad = state[:40].copy()
    bad[:, 1] = np.nan
    sim2 = _sim(nb, "naive", bad)
    g = _halo(sim2, EDGES, centers=[[0, 0, 0]])
    _check(g, H.halo_ref(bad, EDGES, centers=[[0, 0, 0]]))
    assert (g.st.nonfinite, g.st.tested, tuple(g.st.cells)) == (40, 0, (1, 1, 1))
    g = _halo(sim2, EDGES, bodies=[7])
    assert g.heads["flags"][0] == 1
    sim2.destroy()
    # m = 0: nothing is written, the stats say so
    g = _halo(sim, EDGES, m=0)
    assert (g.st.n, g.st.centers, g.st.tested, g.st.items, tuple(g.st.cells)) == (600, 0, 0, 0, (0, 0, 0))
    g = _halo(sim, EDGES, centers=np.zeros((0, 3)))
    assert g.st.centers == 0
    sim.destroy()
    # n = 0
    sim0 = _sim(nb, "naive", state[:0])
    c, vc = [[0.1, 0.2, 0.3], [1, 2, 3]], [[0, 0, 1], [0, 0, 0]]
    g = _halo(sim0, EDGES, centers=c, velocities=vc)
    _check(g, H.halo_ref(state[:0], EDGES, centers=c, velocities=vc))
    assert set(g.bins.tobytes()) == {0}
    assert _raw(sim0, EDGES, bodies=[0]).rc == _lib.NB_ERR_INVALID
    assert _halo(sim0, EDGES, m=0).st.n == 0
    sim0.destroy()


# ---- invariants ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_bits_do_not_depend_on_the_call(gpu, kind):
    """Two calls, a subset, a permutation, a duplicated centre and another nbins between: the same bits per centre."""
    nb = gpu
    sim, state = _prepared(nb, kind, make_state("disc", 4097, seed=2))
    rng = np.random.default_rng(3)
    x = state[:, 0:3].astype(np.float64)
    c = x[rng.integers(0, 4097, 300)] + rng.normal(scale=0.01, size=(300, 3))
    vc = rng.normal(scale=0.1, size=(300, 3))
    edges = np.array([0.0, 0.02, 0.05, 0.1, 0.3])
    a = _halo(sim, edges, centers=c, velocities=vc)
    assert a.bins["count"].sum() > 2000
    b = _halo(sim, edges, centers=c, velocities=vc)
    assert a.bytes == b.bytes
    _halo(sim, edges[:3], centers=c[:7])
    perm = rng.permutation(300)
    p = _halo(sim, edges, centers=c[perm], velocities=vc[perm])
    assert p.heads.tobytes() == a.heads[perm].tobytes() and p.bins.tobytes() == a.bins[perm].tobytes()
    assert p.st.tested == a.st.tested and p.st.items == a.st.items
    sub = np.array([5, 5, 299, 0, 5, 17])
    s = _halo(sim, edges, centers=c[sub], velocities=vc[sub])
    assert s.heads.tobytes() == a.heads[sub].tobytes() and s.bins.tobytes() == a.bins[sub].tobytes()
    one = _halo(sim, edges, centers=c[123:124], velocities=vc[123:124])
    assert one.bins.tobytes() == a.bins[123:124].tobytes()
    sim.destroy()


def _other_passes(sim):
    sim.knn_density(6)
    sim.fof_groups(0.02, min_members=2)
    sim.radial_profile(rmin=1e-3, rmax=10.0, nbins=16)


def test_first_use_order_against_other_passes(gpu):
    """The result does not depend on which pass made its workspace (and used the shared sort) first."""
    nb = gpu
    state = make_state("spherical", 3000, seed=4)
    c = state[::100, 0:3].astype(np.float64)
    edges = np.array([0.01, 0.1, 0.5])
    sim = _sim(nb, "naive", state)
    first = _halo(sim, edges, centers=c)
    _other_passes(sim)
    again = _halo(sim, edges, centers=c)
    sim.destroy()
    sim = _sim(nb, "naive", state)
    _other_passes(sim)
    late = _halo(sim, edges, centers=c)
    sim.destroy()
    assert first.bytes == again.bytes == late.bytes


def test_null_outputs_and_refusals(gpu):
    nb = gpu
    from wgpu_n_body_amd import _lib
    Lb = _lib.lib()
    state = make_state("spherical", 2000, seed=3)
    sim = _sim(nb, "naive", state)
    c = state[:9, 0:3].astype(np.float64)
    full = _halo(sim, EDGES, centers=c)
    for want in ((False, False), (True, False), (False, True)):
        g = _halo(sim, EDGES, centers=c, want=want)
        assert bytes(g.st) == bytes(full.st)
        assert g.heads.tobytes() == (full.heads.tobytes() if want[0] else bytes([FILL]) * (64 * 9))
        assert g.bins.tobytes() == (full.bins.tobytes() if want[1] else bytes([FILL]) * (88 * 9 * 4))

    def refused(code=_lib.NB_ERR_INVALID, **kw):
        g = _raw(sim, kw.pop("edges", EDGES), **kw)
        assert g.rc == code and Lb.nb_last_error()
        assert set(g.all) == {FILL} and bytes(g.st) == bytes(_lib.nb_halo_stats())  # a refused call writes nothing

    refused(edges=[0.1, 0.1, 0.2], centers=c)
    refused(edges=[0.1, np.nan], centers=c)
    refused(edges=[-0.1, 0.2], centers=c)
    refused(edges=np.linspace(0.1, 1, 66), centers=c)
    refused(centers=c, nbins=0)
    refused(m=3)                                         # neither
    refused(centers=c, bodies=np.arange(9))              # both
    refused(centers=[[0, 0, np.inf]])
    refused(centers=c, velocities=np.full((9, 3), np.nan))
    refused(bodies=[0, 2000])                            # an index that is no body
    refused(bodies=[0xFFFFFFFF])
    refused(edges=[0.1, 0.2], m=H.MAX_CENTERS + 1)       # the limits: before any pointer is read
    refused(edges=np.linspace(0.1, 1, 65), m=H.MAX_ROWS // 64 + 1)
    with pytest.raises(nb.NBodyError) as ex:
        sim.halo_profiles(c, edges=[0.2, 0.1])
    assert ex.value.code == _lib.NB_ERR_INVALID
    assert _halo(sim, EDGES, centers=c).bytes == full.bytes  # the simulator stays usable
    sim.destroy()
    # a sharded simulator (rank 0 of 2)
    s = make_state("uniform", 64, seed=1)
    sharded = nb.NaiveSim.from_particles(nb.SimParams(particle_num=64), None, s, placement=nb.Placement(world=2))
    g = _raw(sharded, EDGES, centers=c)
    assert g.rc == _lib.NB_ERR_UNSUPPORTED and b"sharded" in Lb.nb_last_error() and set(g.all) == {FILL}
    sharded.destroy()
    # a several-GPU runner, both ranks on device 0
    r = nb.OfflineHeadless(nb.NaiveSim, nb.SimParams(particle_num=512), None,
                           lambda sp: nb.inits.uniform_init(sp, seed=1), device_ids=[0, 0])
    with pytest.raises(nb.NBodyError) as ex:
        r.halo_profiles(c, edges=EDGES)
    assert ex.value.code == _lib.NB_ERR_UNSUPPORTED
    r.destroy()


@pytest.mark.parametrize("case", ["naive", "tree"])
def test_does_not_perturb_the_trajectory(gpu, case):
    nb = gpu
    n, steps = 4096, 8
    state = make_state("uniform", n, seed=9)
    finals = []
    for with_halo in (False, True):
        sim = _sim(nb, case, state)
        for j in range(steps):
            sim.encode()
            if with_halo:
                h = sim.halo_profiles(bodies=np.arange(0, n, 97 + j), rmin=0.01, rmax=0.2, nbins=4 + j)
                assert h.stats.step_num == j + 1 and h.stats.nonfinite == 0 and h.count.sum() > 0
        finals.append(nb.as_floats(sim.read_particles()).copy())
        sim.destroy()
    assert np.array_equal(finals[0].view(np.uint32), finals[1].view(np.uint32))


# ---- pruning ---------------------------------------------------------------------------------------------------
def _clumps(n_clumps, per, seed, spread=0.01, box=1.0):
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-box, box, (n_clumps, 3))
    x = (centres[:, None, :] + rng.normal(scale=spread, size=(n_clumps, per, 3))).reshape(-1, 3)
    v = rng.normal(scale=0.05, size=x.shape)
    return _state(x, v=v, m=rng.uniform(0.5, 1.5, x.shape[0])), centres


def test_pruning_works(gpu):
    nb = gpu
    state, centres = _clumps(64, 64, seed=7)
    sim = _sim(nb, "naive", state)
    edges = np.array([0.0, 0.005, 0.01, 0.02, 0.04])
    a, b = _halo(sim, edges, centers=centres), _halo(sim, edges, centers=centres)
    _check(a, H.halo_ref(state, edges, centers=centres))
    assert a.st.tested == b.st.tested and a.bytes == b.bytes
    assert a.st.tested < 4096 * 64 // 4, a.st.tested
    assert np.all(a.bins["count"].sum(1) + a.heads["inside_count"] >= 60)  # each centre sees its clump
    sim.destroy()


# ---- the work-item limit -----------------------------------------------------------------------------------------
def test_more_centres_than_extra_items(gpu):
    """One work item a centre always fits: 2^18 + 1 body centres over 256 bodies (more centres than
    NB_HALO_EXTRA_ITEMS, few candidates each) is an ordinary call, and each row is the bits of its body's row in a call
    with 256 centres."""
    nb = gpu
    rng = np.random.default_rng(21)
    state = _state(rng.uniform(-1, 1, (256, 3)), v=rng.normal(size=(256, 3)), m=rng.uniform(0.5, 2, 256))
    sim = _sim(nb, "naive", state)
    edges = np.array([0.0, 0.3])
    m = (1 << 18) + 1
    assert m > H.EXTRA_ITEMS
    few = _halo(sim, edges, bodies=np.arange(256))
    ref = H.halo_ref(state, edges, bodies=np.arange(256))
    _check(few, ref)
    which = np.arange(m) % 256
    g = _halo(sim, edges, bodies=which)
    assert g.heads.tobytes() == few.heads[which].tobytes() and g.bins.tobytes() == few.bins[which].tobytes()
    T = ref["candidates"][which]
    assert (g.st.centers, g.st.tested, g.st.items) == (m, int(T.sum()), m) and T.min() >= 1
    sim.destroy()


def test_too_many_work_items_are_refused(gpu):
    """32,768 bodies in one cell are 8 work items a centre: 10,000 centres need 80,000, more than 10,000 +
    NB_HALO_EXTRA_ITEMS.  The refusal is found on the device: nothing is written, and the simulator stays usable --
    9,000 centres fit."""
    nb = gpu
    from wgpu_n_body_amd import _lib
    rng = np.random.default_rng(22)
    n = 8 * L
    state = _state(rng.uniform(-1, 1, (n, 3)), v=rng.normal(size=(n, 3)))
    sim = _sim(nb, "naive", state)
    edges = np.array([0.5, 4.0])
    c = rng.uniform(-1, 1, (10000, 3))
    assert 8 * 10000 > 10000 + H.EXTRA_ITEMS >= 8 * 9000 - 9000
    g = _raw(sim, edges, centers=c)
    assert g.rc == _lib.NB_ERR_UNSUPPORTED and b"80000 work items" in _lib.lib().nb_last_error()
    assert set(g.all) == {FILL} and bytes(g.st) == bytes(_lib.nb_halo_stats())
    g = _raw(sim, edges, centers=c, want=(False, False))
    assert g.rc == _lib.NB_ERR_UNSUPPORTED and bytes(g.st) == bytes(_lib.nb_halo_stats())
    ok = _halo(sim, edges, centers=c[:9000])
    assert (ok.st.tested, ok.st.items, tuple(ok.st.cells)) == (9000 * n, 9000 * 8, (1, 1, 1))
    rows = [0, 4500, 8999]
    three = _halo(sim, edges, centers=c[rows])
    _check(three, H.halo_ref(state, edges, centers=c[rows]))
    assert ok.heads[rows].tobytes() == three.heads.tobytes() and ok.bins[rows].tobytes() == three.bins.tobytes()
    assert np.all(ok.bins["count"][:, 0] + ok.heads["inside_count"] == n)
    sim.destroy()


# ---- the mirrors -----------------------------------------------------------------------------------------------
def test_python_wrapper_and_group_profiles(gpu):
    nb = gpu
    state, centres = _clumps(24, 200, seed=11, spread=0.01)
    sim = _sim(nb, "naive", state)
    edges = nb.radial_edges(0.002, 0.05, 12)
    h = sim.halo_profiles(centres, edges=edges)
    g = _halo(sim, edges, centers=centres)
    assert h.nbins == 12 and np.array_equal(h.count, g.bins["count"]) and np.array_equal(h.mass, g.bins["mass"])
    assert np.array_equal(h.ang, g.bins["ang"]) and np.array_equal(h.inside_mass, g.heads["inside_mass"])
    assert np.array_equal(h.center, centres) and not h.velocity.any() and not h.flags.any()
    assert (h.stats.tested, h.stats.items, h.stats.cells) == (g.st.tested, g.st.items, tuple(g.st.cells))
    enc = h.enclosed_mass
    for j in (0, 23):
        assert np.allclose(enc[j], H.enclosed64(h.inside_mass[j], h.mass[j]), rtol=1e-14, atol=0)
    assert np.allclose(h.density * H.SPHERE * (edges[1:] ** 3 - edges[:-1] ** 3), h.mass, rtol=1e-13)
    assert np.allclose(h.vcirc(2.0) ** 2 * edges, 2.0 * enc, rtol=1e-13)
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(h.mean_ur, h.m_ur / h.mass, equal_nan=True)
        assert np.all((h.sigma_r >= 0) | np.isnan(h.sigma_r))
    rho = 0.5 * enc[:, -1].max() / (H.SPHERE * edges[-1] ** 3) * 8
    r, mass = h.overdensity(rho)
    for j in range(24):
        wr, wm = H.overdensity64(h.inside_mass[j], h.mass[j], edges, rho)
        assert (np.isnan(r[j]) and np.isnan(wr)) or (abs(r[j] - wr) <= 1e-12 * wr and abs(mass[j] - wm) <= 1e-12 * wm)
    assert np.isfinite(r).any()
    same = sim.halo_profiles(centres, rmin=0.002, rmax=0.05, nbins=12)
    assert np.array_equal(same.edges, edges) and np.array_equal(same.mass, h.mass)
    with pytest.raises(ValueError):
        sim.halo_profiles(centres)
    # the groups of the same state, about their centres of mass and about their most bound bodies
    fof = sim.fof_groups(0.01, min_members=50)
    rows, hp = sim.group_profiles(fof, edges=edges)
    assert len(rows) == fof.stats.groups >= 20 and np.array_equal(hp.center, fof.com[rows])
    assert np.array_equal(hp.velocity, fof.velocity[rows])
    ref = H.halo_ref(state, edges, centers=fof.com[rows], velocities=fof.velocity[rows])
    assert np.array_equal(hp.count, ref["count"]) and np.all(np.abs(hp.mass - ref["mass"]) <= TOL * ref["scale"]["mass"])
    with pytest.raises(ValueError):
        sim.group_profiles(fof, center="most_bound", edges=edges)
    sim.destroy()
    # a catalogue of bound groups (the clumps of tests/bound_ref.py, some of which dissolve)
    from tests import bound_ref as B
    state, bp = B.case("fates")
    sim = nb.NaiveSim.from_particles(nb.SimParams(particle_num=state.shape[0], g=bp["g"], e=bp["e"], dt=bp["dt"]),
                                     None, state)
    bg = sim.bound_groups(bp["link"], min_members=bp["min_members"], min_bound=bp["min_bound"],
                          max_group=bp["max_group"])
    edges = nb.radial_edges(0.0005, 0.02, 8)
    rows, hb = sim.group_profiles(bg, center="most_bound", edges=edges)
    assert np.array_equal(rows, np.flatnonzero(bg.rows["most_bound"] != nb.FOF_NONE))
    assert 1 <= len(rows) < bg.stats.groups  # some rows have no bound set
    mb = bg.rows["most_bound"][rows]
    assert np.array_equal(hb.center, state[mb, 0:3].astype(np.float64))
    assert np.array_equal(hb.velocity, state[mb, 3:6].astype(np.float64))
    assert np.array_equal(hb.count, H.halo_ref(state, edges, bodies=mb)["count"])
    rows, hc = sim.group_profiles(bg, edges=edges)
    assert np.array_equal(rows, np.flatnonzero(bg.rows["mass"] > 0)) and np.array_equal(hc.center, bg.com[rows])
    sim.destroy()


def test_runner_and_cli(gpu):
    """nb_runner_halo_profiles equals nb_sim_halo_profiles on nb_runner_sim, and headless --halo (the C++ mirror over
    nb_runner_fof and nb_runner_halo_profiles) prints what the Python runner and the helpers return."""
    nb = gpu
    from wgpu_n_body_amd import _lib
    cli = os.path.join(ROOT, "wgpu_n_body_amd", "headless")
    rho = 2000.0
    base = [cli, "--sim", "tree", "--n", "4096", "--init", "disc", "--steps", "2"]
    p = subprocess.run(base + ["--halo", "2", "--halo-link", "0.02", "--halo-range", "0.01,1.0", "--halo-bins", "16",
                               "--halo-min", "8", "--halo-top", "3", "--halo-rho", str(rho)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    heads = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("halo ")]
    lines = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("halo_group ")]
    assert len(heads) == 2 and [int(h[1]) for h in heads] == [0, 2]
    assert len([ln for ln in p.stdout.splitlines() if ln.startswith("Step Duration: ")]) == 2

    runner = nb.OfflineHeadless(nb.TreeSim, nb.SimParams(particle_num=4096), nb.AddParams.TreeSimParams(0.75),
                                lambda sp: nb.inits.disc_init(sp, seed=0))
    edges = nb.radial_edges(0.01, 1.0, 16)
    fof = runner.fof_groups(0.02, min_members=8)  # the same seeded init, no step yet: the lines of step 0
    rows, hp = runner.group_profiles(fof, edges=edges)
    assert len(rows) == fof.stats.groups >= 1 and int(heads[0][2]) == fof.stats.groups
    assert (int(heads[0][3]), int(heads[0][4])) == (hp.stats.tested, hp.stats.items)
    r, mass = hp.overdensity(rho)
    enc = hp.enclosed_mass
    top = [ln for ln in lines if int(ln[1]) == 0]
    assert len(top) == min(3, fof.stats.groups)
    for ln, row in zip(top, fof.by_size()):
        assert [int(ln[2]), int(ln[3]), int(ln[4])] == [row, fof.label[row], fof.count[row]]
        got = np.array([float(v) for v in ln[5:9]])
        peak = enc[row] / edges
        want = np.array([r[row], mass[row], edges[np.argmax(peak)], peak.max()])
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.all(np.abs(got[ok] - want[ok]) <= 1e-12 * np.abs(want[ok]))  # (%.17g round-trips)
    runner.step()
    c = nb.as_floats(runner.read_particles())[::500, 0:3].astype(np.float64)
    via_runner = _raw(None, edges, centers=c, call=_lib.lib().nb_runner_halo_profiles, handle=runner._h)
    via_sim = _raw(runner.sim, edges, centers=c)
    state = _state_of(nb, runner.sim)
    runner.destroy()
    assert via_runner.rc == via_sim.rc == 0 and via_runner.bytes == via_sim.bytes
    _check(via_sim, H.halo_ref(state, edges, centers=c))
