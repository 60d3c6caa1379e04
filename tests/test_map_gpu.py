"""nb_sim_map on the device (csrc/nb_map.hip) against the numpy restatement of its rule (tests/map_ref.py) on
the read-back state: every count equal, every sum to 1e-10 of its sum of |term|; bodies exactly on cell
edges; concentrated and sparse states; cross-checks against the diagnostics and the radial profile; bitwise
reproducibility; that a call does not perturb the trajectory; the refusals; the runner, the C++ mirror and
the CLI.  `-m gpu`."""
import ctypes as C
import itertools
import math
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from tests import map_ref as M
from tests.helpers import ROOT, make_state

pytestmark = pytest.mark.gpu

TOL = 1e-10  # of the sum of |term|: TOL of tests/test_radial_gpu.py, what the diagnostics' moments are held to
SENTINEL = -12345.5
INF = math.inf


def _sim(nb, kind, state, theta=0.75):
    sp = nb.SimParams(particle_num=state.shape[0])
    if kind == "naive":
        return nb.NaiveSim.from_particles(sp, None, state)
    return nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(theta), state)


def _params(width, height, extent, axis=(0.0, 1.0, 0.0), center="com", velocity=(0.0, 0.0, 0.0), depth=(-INF, INF),
            velocities=True):
    from wgpu_n_body_amd import _lib
    p = _lib.nb_map_params()
    p.width, p.height = width, height
    p.flags = (_lib.NB_MAP_VELOCITY if velocities else 0) | (_lib.NB_MAP_CENTER_COM if isinstance(center, str) else 0)
    for k in range(3):
        p.axis[k] = axis[k]
        if not isinstance(center, str):
            p.center[k], p.velocity[k] = center[k], velocity[k]
    p.x_range[0], p.x_range[1], p.y_range[0], p.y_range[1] = extent
    p.depth_range[0], p.depth_range[1] = depth
    return p


def _raw(sim, p, call=None, handle=None):
    """The C call with every buffer pre-filled: six planes are offered whatever the flags ask for."""
    from wgpu_n_body_amd import _lib
    cells = p.width * p.height
    counts = np.full(cells, 0xDEADBEEF, np.uint32)
    planes = np.full(6 * cells, SENTINEL)
    st = _lib.nb_map_stats()
    rc = (call or _lib.lib().nb_sim_map)(handle or sim._h, C.byref(p), counts.ctypes.data, planes.ctypes.data, C.byref(st))
    return rc, counts.reshape(p.height, p.width), planes.reshape(6, p.height, p.width), st


def _map(sim, *args, **kw):
    from wgpu_n_body_amd import _lib
    p = _params(*args, **kw)
    rc, counts, planes, st = _raw(sim, p)
    assert rc == 0, _lib.lib().nb_last_error()
    vec = lambda a: np.array(list(a))  # noqa: E731
    return SimpleNamespace(counts=counts, planes=planes, st=st, nplanes=6 if p.flags & _lib.NB_MAP_VELOCITY else 1,
                           center=vec(st.center), velocity=vec(st.velocity), flags=p.flags,
                           bytes=counts.tobytes() + planes.tobytes() + bytes(st))


def _check(m, ref, tol=TOL):
    """Every integer equal, every sum within tol of the restatement's sum of |term|; the identities; planes that
    were not asked for untouched; the frame bit-equal to the restatement's."""
    st, sc = m.st, ref["scale"]
    H, W = ref["counts"].shape
    assert (st.n, st.nonfinite, st.binned_count, st.outside_count) == \
        (ref["n"], ref["nonfinite"], ref["binned_count"], ref["outside_count"])
    assert (st.width, st.height, st.flags, st.max_count) == (W, H, m.flags, ref["max_count"])
    assert np.array_equal(m.counts, ref["counts"]), np.argwhere(m.counts != ref["counts"])[:8]
    assert st.binned_count + st.outside_count + st.nonfinite == st.n and int(m.counts.sum(dtype=np.uint64)) == st.binned_count
    for got, name in ((st.binned_mass, "binned_mass"), (st.outside_mass, "outside_mass"), (st.mass, "total_mass")):
        assert abs(got - ref[name]) <= tol * sc[name], (name, got, ref[name])
    worst = 0.0
    for k, name in enumerate(M.PLANES[:m.nplanes]):
        err = np.abs(m.planes[k] - ref[name])
        assert np.all(err <= tol * sc[name] + 1e-300), (name, float(err.max()))
        worst = max(worst, float((err / (sc[name] + 1e-300)).max()))
        assert np.all(m.planes[k][ref["counts"] == 0] == 0.0), name  # no body: exactly zero
    assert np.all(m.planes[m.nplanes:] == SENTINEL)
    for got, name in ((st.n_hat, "n_hat"), (st.e1, "e1"), (st.e2, "e2")):
        assert np.array(list(got)).tobytes() == ref[name].tobytes(), name
    return worst


GRIDS = [(1, 1), (1, 7), (7, 1), (16, 16), (17, 33), (100, 60), (256, 256)]
AXES = [(0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 2.0, 3.0)]
# the cross product of every axis of the issue, thinned to 60 cases that keep every value of every axis
_ALL = list(itertools.product(["naive", "tree"], ["uniform", "disc", "spherical"], [1, 2, 63, 65, 257, 1000, 4097],
                              range(len(GRIDS)), range(len(AXES)), ["explicit", "com"], [True, False], ["all", "slab"]))
CASES = [_ALL[(i * 3977 + 13) % len(_ALL)] for i in range(60)]
assert len(set(CASES)) == 60 and [len({c[a] for c in CASES}) for a in range(8)] == [2, 3, 7, 7, 3, 2, 2, 2]


def _case_id(c):
    return "-".join(["%dx%d" % GRIDS[v] if a == 3 else "ax%d" % v if a == 4 else "vel%d" % v if a == 6 else str(v)
                     for a, v in enumerate(c)])


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[_case_id(c) for c in CASES])
def test_parity_with_the_restatement(gpu, idx):
    nb = gpu
    kind, init, n, grid, ax, centre, velocities, slab = CASES[idx]
    (W, H), axis = GRIDS[grid], AXES[ax]
    sim = _sim(nb, kind, make_state(init, n, seed=idx + 31))
    if kind == "tree":  # the state is then in tree order
        for _ in range(3):
            sim.encode()
    # windows that leave bodies outside (every init reaches beyond 0.5), one of them off-centre
    extent = (-0.5, 0.5, -0.5, 0.5) if idx % 2 == 0 else (-0.3, 0.45, -0.6, 0.2)
    depth = (-INF, INF) if slab == "all" else (-0.25, 0.3)
    if centre == "com":
        m = _map(sim, W, H, extent, axis, "com", depth=depth, velocities=velocities)
        d = sim.diagnostics()
        assert m.center.tobytes() == d.com.tobytes()
        assert m.velocity.tobytes() == (d.momentum / d.mass).tobytes()
        c, vc = m.center, m.velocity
    else:
        c, vc = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)) if idx % 4 < 2 else ((0.05, -0.02, 0.01), (1e-3, -2e-3, 5e-4))
        m = _map(sim, W, H, extent, axis, c, vc, depth=depth, velocities=velocities)
        assert np.array_equal(m.center, c) and np.array_equal(m.velocity, vc)
    state = nb.as_floats(sim.read_particles())
    sim.destroy()
    assert m.st.step_num == (3 if kind == "tree" else 0)
    ref = M.map64(state, W, H, extent, axis=axis, center=c, velocity=vc, depth=depth)
    worst = _check(m, ref)
    print(f"binned {m.st.binned_count} outside {m.st.outside_count} worst error / bound {worst / TOL:.3g}")
    if n >= 1000:
        assert 0 < m.st.binned_count and 0 < m.st.outside_count  # the window does cut


def _dyadic_state(n):
    """Coordinates k / 64: the named ones first, the rest seeded.  Seen along z, a = x and b = y."""
    rng = np.random.default_rng(8)
    q = rng.integers(-96, 97, size=(n, 3))
    q[0] = (-64, 0, 5)      # on the window's lower x bound: cell 0
    q[1] = (64, 0, 5)       # on its upper x bound: outside
    q[2] = (8, -32, 0)      # on an interior x edge: the cell above; on the lower y bound: row 0
    q[3] = (0, 32, 0)       # on the upper y bound: outside
    q[4] = (63, 31, 9)      # the last cell
    q[5] = (-8, 8, 0)       # interior edges both ways
    q[6] = (7, 7, -64)      # inside the cell below those edges
    q[7] = (-65, 0, 0)      # just outside
    s = np.zeros((n, 10), np.float32)
    s[:, 0:3] = q / 64.0
    s[:, 3:6] = rng.integers(-64, 65, size=(n, 3)) / 64.0
    s[:, 9] = rng.integers(1, 9, size=n)
    return q, s


@pytest.mark.parametrize("kind", ["naive", "tree"])
@pytest.mark.parametrize("n", [256, 257])
def test_bodies_exactly_on_cell_edges(gpu, kind, n):
    """Coordinates, windows and cell sizes are dyadic, so every edge is exact and the expected cells follow from
    integer arithmetic alone: lower edge inclusive, upper exclusive, the window's upper bound outside."""
    nb = gpu
    q, s = _dyadic_state(n)
    W, H = 16, 8                            # x in [-1, 1): cells of 8 / 64; y in [-1/2, 1/2): cells of 8 / 64
    extent = (-1.0, 1.0, -0.5, 0.5)
    inside = (q[:, 0] >= -64) & (q[:, 0] < 64) & (q[:, 1] >= -32) & (q[:, 1] < 32)
    i, j = (q[:, 0] + 64) // 8, (q[:, 1] + 32) // 8
    by_hand = [(0, 4, True), (16, 4, False), (9, 0, True), (8, 8, False), (15, 7, True), (7, 5, True), (8, 4, True)]
    assert [(int(i[k]), int(j[k]), bool(inside[k])) for k in range(7)] == by_hand and not inside[7]
    want = np.zeros((H, W), np.int64)
    np.add.at(want, (j[inside], i[inside]), 1)
    mass = np.zeros((H, W))
    np.add.at(mass, (j[inside], i[inside]), s[inside, 9].astype(np.float64))
    sim = _sim(nb, kind, s)
    m = _map(sim, W, H, extent, (0.0, 0.0, 1.0), (0.0, 0.0, 0.0))
    sim.destroy()
    assert np.array_equal(m.counts, want) and m.st.outside_count == int((~inside).sum()) and m.st.nonfinite == 0
    assert np.array_equal(m.planes[0], mass)  # small integers: exact in any order
    _check(m, M.map64(s, W, H, extent, axis=(0.0, 0.0, 1.0)))


def _concentrated(n, mode, seed):
    """Seen along z in the window [-1, 1)^2 at 256 x 256 (cells of 1 / 128, tiles of 1 / 16): `cell` puts every
    body in cell (37, 150), `tile` in tile (3, 5) but spread over its cells, `half` half of them there."""
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 10), np.float32)
    s[:, 0:3] = rng.uniform(-0.99, 0.99, (n, 3))
    s[:, 3:6] = rng.normal(0.0, 0.5, (n, 3))
    s[:, 9] = rng.uniform(0.5, 2.0, n)
    if mode == "cell":
        s[:, 0] = -1.0 + (37 + rng.uniform(0.05, 0.95, n)) / 128.0
        s[:, 1] = -1.0 + (150 + rng.uniform(0.05, 0.95, n)) / 128.0
    else:
        k = n if mode == "tile" else n // 2
        who = rng.permutation(n)[:k]
        s[who, 0] = -1.0 + (3 * 8 + rng.uniform(0.01, 7.99, k)) / 128.0
        s[who, 1] = -1.0 + (5 * 8 + rng.uniform(0.01, 7.99, k)) / 128.0
    return s


@pytest.mark.parametrize("mode,n,segment", [("cell", 65536, 0), ("tile", 65536, 0), ("half", 262144, 0),
                                            ("half", 262144, 32768)])
def test_concentrated_states(gpu, mode, n, segment):
    """Every body in one cell, in one tile, or half of 262,144 in one tile: that tile's list is cut into 32
    segments of the default 4,096 bodies (or, with "map_segment_len" 32768, into 4 or 5), each summed by its
    own block and the partials added in order.  Correct to the same tolerance, and bit-reproducible."""
    nb = gpu
    s = _concentrated(n, mode, seed=3)
    sim = _sim(nb, "naive", s)
    if segment:
        sim.set_tuning("map_segment_len", segment)
    extent, axis = (-1.0, 1.0, -1.0, 1.0), (0.0, 0.0, 1.0)
    a = _map(sim, 256, 256, extent, axis, (0.0, 0.0, 0.0))
    b = _map(sim, 256, 256, extent, axis, (0.0, 0.0, 0.0))
    sim.destroy()
    ref = M.map64(s, 256, 256, extent, axis=axis)
    worst = _check(a, ref)
    print(f"worst error / bound {worst / TOL:.3g}")
    assert a.bytes == b.bytes
    tile = a.counts[40:48, 24:32]
    if mode == "cell":
        assert a.counts[150, 37] == n == a.st.max_count
    elif mode == "tile":
        assert int(tile.sum()) == n and np.all(tile > 0)
    else:
        assert int(tile.sum()) >= n // 2 > 2 * (segment or 4096)


@pytest.mark.parametrize("n", [262145, 524289])
def test_sort_chunks_beyond_the_other_suites(gpu, n):
    """The shared sort (csrc/nb_analysis_sort.hpp) where no other test takes it: 262,145 bodies are 1,025 chunks of
    256, the last of one body, and the first size at which a thread of the scan owns two chunks; 524,289 are 1,639
    chunks of 320.  Uniform bodies, 256 x 256 cells (two passes), velocities on, a window that cuts."""
    nb = gpu
    state = make_state("uniform", n, seed=13)
    sim = _sim(nb, "naive", state)
    extent, axis = (-0.5, 0.5, -0.5, 0.5), (0.0, 0.0, 1.0)
    m = _map(sim, 256, 256, extent, axis, (0.0, 0.0, 0.0))
    sim.destroy()
    worst = _check(m, M.map64(state, 256, 256, extent, axis=axis))
    print(f"binned {m.st.binned_count} outside {m.st.outside_count} worst error / bound {worst / TOL:.3g}")
    assert 0 < m.st.binned_count and 0 < m.st.outside_count


def test_segment_length_key_is_checked(gpu):
    nb = gpu
    sim = _sim(nb, "naive", make_state("uniform", 64, seed=1))
    for bad in (0, 255, 300, 131072, -256):
        with pytest.raises(nb.NBodyError):
            sim.set_tuning("map_segment_len", bad)
    sim.set_tuning("map_segment_len", 256)
    sim.destroy()


def test_sparse_maximum_then_a_smaller_call(gpu):
    """1,000 bodies in 2048 x 2048: exactly the reached cells are non-zero.  Then 17 x 33 on the same simulator:
    the workspace is reused and no stale cell remains."""
    nb = gpu
    state = make_state("uniform", 1000, seed=17)
    sim = _sim(nb, "naive", state)
    extent = (-0.5, 0.5, -0.5, 0.5)
    big = sim.projected_map(2048, 2048, extent=extent, axis=(1.0, 2.0, 3.0), center=(0.0, 0.0, 0.0), velocities=False)
    ref = M.map64(state, 2048, 2048, extent, axis=(1.0, 2.0, 3.0))
    assert np.array_equal(big.counts, ref["counts"]) and big.binned_count == ref["binned_count"] > 100
    assert np.array_equal(big.mass != 0.0, ref["counts"] > 0) and np.count_nonzero(big.mass) <= 1000
    assert np.all(np.abs(big.mass - ref["mass"]) <= TOL * ref["scale"]["mass"])
    assert big.m_w is None and big.max_count == ref["max_count"]
    assert np.isnan(big.surface_density[ref["counts"] == 0]).all()
    m = _map(sim, 17, 33, extent, (1.0, 2.0, 3.0), (0.0, 0.0, 0.0))
    sim.destroy()
    _check(m, M.map64(state, 17, 33, extent, axis=(1.0, 2.0, 3.0)))


@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_cross_checks_against_the_diagnostics(gpu, kind):
    nb = gpu
    n = 3000
    sim = _sim(nb, kind, make_state("disc", n, seed=21))
    sim.encode()
    d = sim.diagnostics()
    # a window that cuts: the mass plane and what fell outside make up the diagnostics' mass
    cut = sim.projected_map(40, 24, extent=(-0.4, 0.5, -0.3, 0.3), axis=(0.0, 0.0, 1.0))
    assert cut.outside_count > 0 and abs(cut.mass.sum() + cut.outside_mass - d.mass) <= 1e-10 * d.mass
    assert cut.total_mass == d.mass or abs(cut.total_mass - d.mass) <= 1e-10 * d.mass
    # at rest about the origin with everything in the window: half of sum m |u|^2 is the kinetic energy (the sum
    # of |term| of a sum of non-negative terms is the sum itself)
    full = sim.projected_map(33, 17, extent=(-50.0, 50.0, -50.0, 50.0), axis=(1.0, 2.0, 3.0), center=(0.0, 0.0, 0.0))
    sim.destroy()
    assert full.outside_count == 0 and full.binned_count == n
    assert abs(full.m_u2.sum() / 2.0 - d.kinetic) <= TOL * d.kinetic
    # derived quantities: NaN exactly where there is no mass, and a dispersion that is real
    empty = full.mass == 0.0
    assert empty.any() and not empty.all()
    for q in (full.surface_density, full.mean_w, full.mean_ua, full.mean_ub, full.sigma_w):
        assert np.array_equal(np.isnan(q), empty)
    assert np.all(full.sigma_w[~empty] >= 0.0)
    area = (100.0 / 33) * (100.0 / 17)
    assert np.allclose(full.surface_density[~empty], full.mass[~empty] / area, rtol=1e-12)


@pytest.mark.parametrize("axis", [(0.0, 0.0, 1.0), (1.0, 2.0, 3.0)])
def test_counts_against_the_cylindrical_profile(gpu, axis):
    """A map about n with the window centred on the point, and the cylindrical profile about the same axis: the
    cells wholly inside radius R hold no more bodies than the profile has inside R, those that touch it no fewer.
    (The two form the radius differently, so cells within 1e-9 R of the circle count as touching.)"""
    nb = gpu
    n, R, half, side = 4097, 0.4, 0.5, 50
    sim = _sim(nb, "tree", make_state("spherical", n, seed=12))
    sim.encode()
    c = (0.02, -0.01, 0.03)
    pm = sim.projected_map(side, side, extent=(-half, half, -half, half), axis=axis, center=c, velocities=False)
    prof = sim.radial_profile([0.0, R], cylindrical=True, axis=axis, center=c)
    sim.destroy()
    within = int(prof.count[0])
    e = pm.x_edges
    lo, hi = np.minimum(np.abs(e[:-1]), np.abs(e[1:])), np.maximum(np.abs(e[:-1]), np.abs(e[1:]))
    lo[(e[:-1] < 0) & (e[1:] > 0)] = 0.0
    far = np.sqrt(hi[None, :] ** 2 + hi[:, None] ** 2)    # the farthest and the nearest point of every cell
    near = np.sqrt(lo[None, :] ** 2 + lo[:, None] ** 2)
    inner, touching = far <= R * (1 - 1e-9), near < R * (1 + 1e-9)
    assert 0 < int(pm.counts[inner].sum()) <= within <= int(pm.counts[touching].sum()) < n


def test_two_sims_same_state(gpu):
    nb = gpu
    state = make_state("spherical", 5000, seed=5)
    a, b = _sim(nb, "naive", state), _sim(nb, "tree", state)
    args = (100, 60, (-0.5, 0.4, -0.3, 0.6), (1.0, 2.0, 3.0), "com")
    ma, mb = _map(a, *args), _map(b, *args)
    a.destroy()
    b.destroy()
    ref = M.map64(state, *args[:4], center=ma.center, velocity=ma.velocity)
    _check(ma, ref)
    _check(mb, M.map64(state, *args[:4], center=mb.center, velocity=mb.velocity))
    assert np.array_equal(ma.counts, mb.counts)
    for k, name in enumerate(M.PLANES):
        assert np.all(np.abs(ma.planes[k] - mb.planes[k]) <= 2 * TOL * ref["scale"][name] + 1e-300), name


@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_bitwise_reproducible(gpu, kind):
    nb = gpu
    sim = _sim(nb, kind, make_state("disc", 4097, seed=2))
    sim.encode()
    args = (100, 60, (-0.5, 0.5, -0.4, 0.4), (0.0, 0.0, 1.0), "com")
    m1, m2 = _map(sim, *args), _map(sim, *args)
    sim.diagnostics(potential=True)  # shares the moments' workspace
    _map(sim, 16, 16, (-1.0, 1.0, -1.0, 1.0), (0.0, 1.0, 0.0), (0.0, 0.0, 0.0), velocities=False)  # another shape between
    m3 = _map(sim, *args)
    sim.destroy()
    assert m1.st.n == 4097 and m1.st.binned_count > 0
    assert m1.bytes == m2.bytes == m3.bytes


@pytest.mark.parametrize("case", ["naive", "tree", "tree_graph", "tree_gather"])
def test_does_not_perturb_the_trajectory(gpu, case):
    nb = gpu
    n, steps = (1 << 20, 3) if case == "tree_gather" else (4096, 10)
    state = make_state("uniform", n, seed=9)
    finals = []
    for with_map in (False, True):
        sim = _sim(nb, "naive" if case == "naive" else "tree", state)
        if case == "tree_graph":
            sim.set_tuning("tree_use_graph", 1)
        for k in range(steps):
            sim.encode()
            if with_map:
                pm = sim.projected_map(64, 48, extent=(-0.8, 0.8, -0.6, 0.6), axis=(1.0, 2.0, 3.0),
                                       center="com" if k % 3 else (0, 0, 0), velocities=k % 2 == 1)
                assert pm.step_num == k + 1 and pm.binned_count + pm.outside_count == n
        finals.append(nb.as_floats(sim.read_particles()).copy())
        sim.destroy()
    assert np.array_equal(finals[0].view(np.uint32), finals[1].view(np.uint32))


@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_nonfinite_bodies_are_counted_and_left_out(gpu, kind):
    nb = gpu
    n = 1000
    extent, axis = (-0.5, 0.5, -0.5, 0.5), (1.0, 2.0, 3.0)
    for col in (1, 4, 9):  # a position, a velocity, the mass
        for bad in (np.nan, np.inf, -np.inf):
            state = make_state("uniform", n, seed=4)
            state[137, col] = bad
            sim = _sim(nb, kind, state)
            m = _map(sim, 17, 33, extent, axis, (0.0, 0.0, 0.0))
            sim.destroy()
            assert m.st.nonfinite == 1 and np.isfinite(m.st.mass) and np.isfinite(m.planes).all()
            _check(m, M.map64(state, 17, 33, extent, axis=axis))
            # ... which is the map of the state without that body
            rest = M.map64(np.delete(state, 137, axis=0), 17, 33, extent, axis=axis)
            assert np.array_equal(m.counts, rest["counts"])


def test_null_outputs(gpu):
    """counts, planes and stats may each be null; a call with none of them measures nothing."""
    nb = gpu
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    sim = _sim(nb, "naive", make_state("uniform", 1000, seed=3))
    p = _params(17, 33, (-0.5, 0.5, -0.5, 0.5), (0.0, 0.0, 1.0), "com")
    rc, counts, planes, st = _raw(sim, p)
    assert rc == 0
    assert L.nb_sim_map(sim._h, C.byref(p), None, None, None) == 0
    only = np.zeros_like(counts)
    assert L.nb_sim_map(sim._h, C.byref(p), only.ctypes.data, None, None) == 0 and np.array_equal(only, counts)
    pl = np.zeros_like(planes)
    assert L.nb_sim_map(sim._h, C.byref(p), None, pl.ctypes.data, None) == 0 and pl.tobytes() == planes.tobytes()
    st2 = _lib.nb_map_stats()
    assert L.nb_sim_map(sim._h, C.byref(p), None, None, C.byref(st2)) == 0 and bytes(st2) == bytes(st)
    sim.destroy()


def test_refusals(gpu):
    nb = gpu
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    s = make_state("uniform", 64, seed=1)
    good = lambda **kw: _params(16, 8, (-1.0, 1.0, -1.0, 1.0), **kw)  # noqa: E731
    sim = _sim(nb, "naive", s)
    for p in (_params(0, 8, (-1.0, 1.0, -1.0, 1.0)), _params(16, 8, (1.0, -1.0, -1.0, 1.0)), good(axis=(0.0, 0.0, 0.0)),
              good(depth=(1.0, 1.0)), good(center=(math.nan, 0.0, 0.0))):
        rc, counts, planes, _ = _raw(sim, p)
        assert rc == _lib.NB_ERR_INVALID and L.nb_last_error()
        assert np.all(counts == 0xDEADBEEF) and np.all(planes == SENTINEL)  # nothing written
    p = good()
    p.flags, p.reserved = 4, 0
    assert _raw(sim, p)[0] == _lib.NB_ERR_INVALID
    p = good()
    p.reserved = 9
    assert _raw(sim, p)[0] == _lib.NB_ERR_INVALID
    rc, _, _, st = _raw(sim, good())
    assert rc == 0 and st.n == 64
    with pytest.raises(nb.NBodyError):
        sim.projected_map(4097, 1, extent=(-1, 1, -1, 1))
    with pytest.raises(ValueError):
        sim.projected_map(8, 8, extent=(-1, 1, -1, 1), center="com", velocity=(0, 0, 0))
    sim.destroy()
    # a sharded simulator (rank 0 of 2)
    sharded = nb.NaiveSim.from_particles(nb.SimParams(particle_num=64), None, s, placement=nb.Placement(world=2))
    rc, _, _, _ = _raw(sharded, good())
    assert rc == _lib.NB_ERR_UNSUPPORTED and b"sharded" in L.nb_last_error()
    sharded.destroy()
    # a several-GPU runner, both ranks on device 0
    r = nb.OfflineHeadless(nb.NaiveSim, nb.SimParams(particle_num=512), None,
                           lambda p: nb.inits.uniform_init(p, seed=1), device_ids=[0, 0])
    with pytest.raises(nb.NBodyError) as ex:
        r.projected_map(16, 8, extent=(-1, 1, -1, 1))
    assert ex.value.code == _lib.NB_ERR_UNSUPPORTED
    r.destroy()


def test_runner_and_cli(gpu, tmp_path):
    """nb_runner_map equals nb_sim_map on nb_runner_sim, and headless --maps (the C++ mirror over nb_runner_map)
    writes what the Python runner returns."""
    nb = gpu
    from wgpu_n_body_amd import _lib
    cli = os.path.join(ROOT, "wgpu_n_body_amd", "headless")
    base = [cli, "--sim", "tree", "--n", "4096", "--init", "disc", "--steps", "4"]
    out = tmp_path / "maps"
    out.mkdir()
    p = subprocess.run(base + ["--maps", str(out), "--map-every", "2", "--map-size", "64x48", "--map-extent", "-1,1,-1,1",
                               "--map-axis", "0,0,1"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    plain = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "map" not in plain.stdout
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("map ")]
    assert sorted(os.listdir(out)) == ["map_000000.npy", "map_000002.npy", "map_000004.npy"] and len(lines) == 3
    # the other output lines are those of a run without --maps (the durations apart)
    blank = lambda text: [re.sub(r"\d+", "#", ln) for ln in text.splitlines() if not ln.startswith("map ")]  # noqa: E731
    assert blank(p.stdout) == blank(plain.stdout)
    assert len([ln for ln in p.stdout.splitlines() if ln.startswith("Step Duration: ")]) == 4

    runner = nb.OfflineHeadless(nb.TreeSim, nb.SimParams(particle_num=4096), nb.AddParams.TreeSimParams(0.75),
                                lambda sp: nb.inits.disc_init(sp, seed=0))
    kw = dict(extent=(-1.0, 1.0, -1.0, 1.0), axis=(0.0, 0.0, 1.0))
    ours = [runner.projected_map(64, 48, **kw)]
    for k in range(4):
        runner.step()
        if (k + 1) % 2 == 0:
            ours.append(runner.projected_map(64, 48, **kw))
    # nb_runner_map against nb_sim_map on the runner's simulator, byte for byte
    pr = _params(64, 48, kw["extent"], kw["axis"], "com")
    via_runner = _raw(None, pr, call=_lib.lib().nb_runner_map, handle=runner._h)
    via_sim = _raw(runner.sim, pr)
    runner.destroy()
    assert via_runner[0] == via_sim[0] == 0
    assert all(a.tobytes() == b.tobytes() for a, b in zip(via_runner[1:3], via_sim[1:3]))
    assert bytes(via_runner[3]) == bytes(via_sim[3]) and np.array_equal(via_sim[1], ours[-1].counts)

    for j, (ln, o) in enumerate(zip(lines, ours)):
        a = np.load(out / ("map_%06d.npy" % (2 * j)))
        assert a.shape == (7, 48, 64) and a.dtype == np.dtype("<f8") and o.step_num == 2 * j
        assert [int(x) for x in ln.split()[1:]] == [o.step_num, int(a[0].sum()), o.n - int(a[0].sum()) - o.nonfinite,
                                                    o.nonfinite, int(a[0].max())]
        if j == 0:  # the same seeded init, no step yet: the file is the Python call, bit for bit
            assert (o.binned_count, o.outside_count, o.max_count) == (int(a[0].sum()), o.n - o.binned_count, int(a[0].max()))
            assert np.array_equal(a[0], o.counts.astype(np.float64))
            for k, name in enumerate(M.PLANES):
                assert a[1 + k].tobytes() == getattr(o, name).tobytes(), name
        else:       # (the trajectory of two runs of the tree is not specified bit for bit)
            assert abs(int(a[0].sum()) - o.binned_count) <= 4096
    assert ours[0].binned_count > 2000
