"""nb_phase_map_sim on the device (csrc/nb_phase.hip) against the numpy restatement of its rule (tests/phase_ref.py)
on the read-back state: every count and class count equal, every sum to 1e-10 of its sum of |term|; bodies exactly
on edges; the grids at which the grouping changes path; concentrated, outside and undefined states; bit-equality
with nb_sim_map where the two overlap; the caller's values; bitwise reproducibility; that a call does not perturb
the trajectory; null outputs, the runner, the C++ mirror and the CLI.  `-m gpu`."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import phase_ref as P
from tests.helpers import ROOT, make_state

pytestmark = pytest.mark.gpu

TOL = 1e-10  # of the sum of |term|: the bound include/nbody.h states for the map and for this pass
INF = math.inf
SIZES = [1, 63, 64, 65, 257, 1000, 4097]
Q = P.QUANTITIES


def _sim(nb, kind, state, steps=2):
    sp = nb.SimParams(particle_num=state.shape[0])
    if kind == "naive":
        return nb.NaiveSim.from_particles(sp, None, state)
    sim = nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(0.75), state)
    for _ in range(steps):  # the state is then in tree order
        sim.encode()
    return sim


def _blob(pm):
    s = pm.stats
    ints = (s.step_num, s.n, s.nonfinite, s.binned_count, s.outside_count, s.undefined_count, s.flags, s.max_count)
    reals = np.array([s.binned_mass, s.outside_mass, s.total_mass])
    planes = b"".join(p.tobytes() for p in (pm.mass, pm.m_q, pm.m_q2) if p is not None)
    return pm.counts.tobytes() + planes + repr(ints).encode() + reals.tobytes() + s.center.tobytes() + \
        s.velocity.tobytes() + s.n_hat.tobytes() + s.e1.tobytes() + s.e2.tobytes()


def _check(pm, ref, tol=TOL):
    """Every integer equal, every sum within tol of the restatement's sum of |term|; the identities; the frame
    bit-equal to the restatement's."""
    st, sc = pm.stats, ref["scale"]
    got = (st.n, st.nonfinite, st.binned_count, st.outside_count, st.undefined_count, st.max_count)
    want = (ref["n"], ref["nonfinite"], ref["binned_count"], ref["outside_count"], ref["undefined_count"],
            ref["max_count"])
    print("classes (n, nonfinite, binned, outside, undefined, max_count):", got, "restatement:", want)
    assert got == want
    assert np.array_equal(pm.counts, ref["counts"]), np.argwhere(pm.counts != ref["counts"])[:8]
    assert st.binned_count + st.outside_count + st.nonfinite == st.n and st.undefined_count <= st.outside_count
    assert int(pm.counts.sum(dtype=np.uint64)) == st.binned_count
    for val, name in ((st.binned_mass, "binned_mass"), (st.outside_mass, "outside_mass"), (st.total_mass, "total_mass")):
        assert abs(val - ref[name]) <= tol * sc[name], (name, val, ref[name])
    worst = 0.0
    for plane, name in ((pm.mass, "mass"), (pm.m_q, "m_q"), (pm.m_q2, "m_q2")):
        if plane is None:
            assert name not in ref
            continue
        err = np.abs(plane - ref[name])
        worst = max(worst, float((err / (sc[name] + 1e-300)).max()))
        assert np.all(err <= tol * sc[name] + 1e-300), (name, float(err.max()))
        assert np.all(plane[ref["counts"] == 0] == 0.0), name  # no body: exactly zero
    for val, name in ((st.n_hat, "n_hat"), (st.e1, "e1"), (st.e2, "e2")):
        assert val.tobytes() == ref[name].tobytes(), name
    print(f"worst error / bound {worst / tol:.3g}")
    return worst


def _values(state):
    """A caller's per-body array: any float64 function of the read-back state."""
    s = state.astype(np.float64)
    return 2.0 * s[:, 0] - s[:, 4] + 0.25 * s[:, 9]


def _range(v):
    """A window that cuts: the 5th to the 95th percentile of the finite values (one value: a window about it)."""
    v = v[np.isfinite(v)]
    if v.size == 0:
        return -1.0, 1.0
    lo, hi = (float(x) for x in np.quantile(v, [0.05, 0.95]))
    return (lo, hi) if hi > lo else (lo - 1.0, lo + 1.0)


GRIDS = [(16, 16), (17, 33), (5, 3), (100, 60)]
AXES = [(0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 2.0, 3.0)]


@pytest.mark.parametrize("k", range(len(Q)), ids=list(Q))
def test_parity_with_the_restatement(gpu, k):
    """Quantity k as x, as y and as the weight, one call each, paired with two others; n, simulator, init, grid,
    axis and centre go round with k.  The windows come from the restatement's own values, so they cut."""
    nb = gpu
    n, kind = SIZES[k % len(SIZES)], ("naive", "tree")[k % 2]
    init, axis = ("uniform", "disc", "spherical")[k % 3], AXES[k % 3]
    (W, H) = GRIDS[k % len(GRIDS)]
    sim = _sim(nb, kind, make_state(init, n, seed=k + 41))
    state = nb.as_floats(sim.read_particles()).copy()
    values = _values(state)
    if (k // 2) % 2:
        d = sim.diagnostics()
        center, c, vc = "com", d.com, d.momentum / d.mass
    else:
        center, c, vc = (0.05, -0.02, 0.01), (0.05, -0.02, 0.01), (1e-3, -2e-3, 5e-4)
    qs = P.quantities(state[:, 0:3].astype(np.float64), state[:, 3:6].astype(np.float64),
                      state[:, 9].astype(np.float64), axis, c, vc, values)
    others = (Q[(k + 5) % len(Q)], Q[(k + 11) % len(Q)])
    for x, y, weight in ((Q[k], others[0], others[1]), (others[0], Q[k], None), (others[1], others[0], Q[k])):
        xe, ye = nb.phase_edges(*_range(qs[x]), W), nb.phase_edges(*_range(qs[y]), H)
        if k % 4 == 3:  # infinite outer edges: nothing defined is outside along x
            xe = np.concatenate(([-INF], xe[1:-1], [INF]))
        kw = dict(velocity=vc) if center != "com" else {}
        pm = sim.phase_map(x, y, x_edges=xe, y_edges=ye, weight=weight, values=values, axis=axis, center=center, **kw)
        assert pm.stats.center.tobytes() == np.asarray(c, dtype=np.float64).tobytes()
        assert pm.stats.velocity.tobytes() == np.asarray(vc, dtype=np.float64).tobytes()
        assert (pm.stats.x, pm.stats.y, pm.stats.weight) == (x, y, weight)
        assert pm.stats.step_num == (2 if kind == "tree" else 0)
        ref = P.phase64(state, x, y, xe, ye, weight=weight, values=values, axis=axis, center=c, velocity=vc)
        _check(pm, ref)
        if n >= 1000:
            assert 0 < pm.stats.binned_count and (k % 4 == 3 or 0 < pm.stats.outside_count)
    sim.destroy()


def _on_edges(edges32):
    """Bodies of mass 1..: at (e, 0, 0), (0, e, 0) and (0, 0, e) for every edge e, and one binary32 step below."""
    below = np.nextafter(edges32, np.float32(-INF), dtype=np.float32)
    vals = np.concatenate([edges32, below])
    rows = []
    for axis in range(3):
        p = np.zeros((len(vals), 3), np.float32)
        p[:, axis] = vals
        rows.append(p)
    s = np.zeros((3 * len(vals), 10), np.float32)
    s[:, 0:3] = np.concatenate(rows)
    s[:, 3:6] = 0.5
    s[:, 9] = 1.0 + np.arange(len(s)) % 7
    return s


@pytest.mark.parametrize("kind", ["naive", "tree"])
@pytest.mark.parametrize("spacing", ["linear", "log"])
@pytest.mark.parametrize("outer", ["finite", "infinite"])
def test_bodies_exactly_on_edges(gpu, kind, spacing, outer):
    """The frame about z (a = x, b = y), centre 0, binary32 coordinates equal to edge values: a = e exactly, and
    r = sqrt(e e) = e exactly (the square of a binary32 value is exact in binary64).  The expected cells follow from
    the indices alone: a body on edge i is in cell i, one binary32 step below in cell i - 1, on the last edge outside."""
    nb = gpu
    W = 16
    e = nb.phase_edges(0.125, 1.0, W) if spacing == "linear" else nb.phase_edges(0.01, 1.0, W, log=True)
    e32 = e.astype(np.float32)
    xe = e32.astype(np.float64)  # the edges are binary32 values
    assert np.all(np.diff(xe) > 0)
    if outer == "infinite":
        xe[0], xe[-1] = -INF, INF
    s = _on_edges(e32)
    sim = _sim(nb, kind, s, steps=0)  # (a step would move the bodies off the edges)
    state = nb.as_floats(sim.read_particles()).copy()
    full = np.array([-INF, INF])

    def by_hand(lines, at_zero):
        """`lines` lines of bodies on and just below every edge, `at_zero` bodies whose value is 0, below edge 0."""
        want, outside = np.zeros(W, np.int64), 0
        cells = [i for i in range(W + 1)] + [i - 1 for i in range(W + 1)]  # on edge i; one step below it
        for cell, times in [(c, lines) for c in cells] + [(-1, at_zero)]:
            if outer == "infinite":  # the first cell reaches down to -inf, the last up to +inf
                cell = min(max(cell, 0), W - 1)
            if 0 <= cell < W:
                want[cell] += times
            else:
                outside += times
        return want, outside

    per_line = 2 * (W + 1)
    for x, (want, outside) in (("a", by_hand(1, 2 * per_line)), ("r", by_hand(3, 0))):
        pm = sim.phase_map(x, "mass", x_edges=xe, y_edges=full, axis=(0.0, 0.0, 1.0), center=(0.0, 0.0, 0.0))
        assert np.array_equal(pm.counts[0], want), (x, pm.counts[0], want)
        assert pm.stats.outside_count == outside and pm.stats.undefined_count == 0
        assert int(want.sum()) + outside == 3 * per_line and (outside == 0) == (outer == "infinite")
        _check(pm, P.phase64(state, x, "mass", xe, full, axis=(0.0, 0.0, 1.0)))
    sim.destroy()


@pytest.mark.parametrize("W,H", [(1, 1), (8, 8), (9, 7), (1, 4096), (4096, 1), (200, 200)])
def test_grids(gpu, W, H):
    """One tile, whole tiles, partial tiles, one row and one column of tiles, and 625 tiles (two sort passes)."""
    nb = gpu
    state = make_state("spherical", 1000, seed=7)
    sim = _sim(nb, "naive", state)
    q = P.quantities(state[:, 0:3].astype(np.float64), state[:, 3:6].astype(np.float64), state[:, 9].astype(np.float64))
    xe, ye = nb.phase_edges(0.02, 0.6, W, log=W <= 256), nb.phase_edges(*_range(q["u_r"]), H)
    pm = sim.phase_map("r", "u_r", x_edges=xe, y_edges=ye, weight="u_t", center=(0.0, 0.0, 0.0))
    sim.destroy()
    _check(pm, P.phase64(state, "r", "u_r", xe, ye, weight="u_t"))
    assert pm.stats.binned_count > 0 and pm.counts.shape == (H, W)


def test_the_largest_grid(gpu):
    """2048 x 2048: 65,536 tiles, three sort passes, exactly NB_MAP_MAX_CELLS.  Counts only."""
    nb = gpu
    state = make_state("uniform", 4097, seed=8)
    sim = _sim(nb, "naive", state)
    xe, ye = nb.phase_edges(-0.5, 0.5, 2048), nb.phase_edges(-0.5, 0.5, 2048)
    pm = sim.phase_map("a", "b", x_edges=xe, y_edges=ye, axis=(0.0, 0.0, 1.0), center=(0.0, 0.0, 0.0))
    # the key's range: the key of a body that is not binned is 65,536 << 6, past every cell's; all of them outside
    far = sim.phase_map("a", "b", x_edges=xe + 100.0, y_edges=ye, axis=(0.0, 0.0, 1.0), center=(0.0, 0.0, 0.0))
    sim.destroy()
    ref = P.phase64(state, "a", "b", xe, ye, axis=(0.0, 0.0, 1.0))
    assert np.array_equal(pm.counts, ref["counts"]) and pm.stats.binned_count == ref["binned_count"] > 1000
    assert (pm.stats.outside_count, pm.stats.max_count) == (ref["outside_count"], ref["max_count"])
    assert not far.counts.any() and not far.mass.any() and far.stats.outside_count == 4097 and far.stats.max_count == 0


def test_concentrated_outside_and_undefined(gpu):
    nb = gpu
    n = 1000
    state = make_state("uniform", n, seed=9)
    sim = _sim(nb, "naive", state)
    sim.set_tuning("phase_segment_len", 256)  # 1,000 bodies of one tile: four segments, the combine path
    wide = np.array([-50.0, 50.0])
    xe = np.array([-100.0, -50.0, 50.0, 100.0])
    one = sim.phase_map("a", "b", x_edges=xe, y_edges=wide, weight="speed", center=(0.0, 0.0, 0.0))
    _check(one, P.phase64(state, "a", "b", xe, wide, weight="speed"))
    assert one.counts[0, 1] == n == one.stats.max_count and one.stats.outside_count == 0
    out = sim.phase_map("a", "b", x_edges=xe + 500.0, y_edges=wide, weight="speed", center=(0.0, 0.0, 0.0))
    _check(out, P.phase64(state, "a", "b", xe + 500.0, wide, weight="speed"))
    assert (out.stats.outside_count, out.stats.undefined_count, out.stats.binned_count) == (n, 0, 0)
    assert out.stats.outside_mass == one.stats.binned_mass or abs(out.stats.outside_mass - one.stats.binned_mass) <= \
        TOL * one.stats.binned_mass
    und = sim.phase_map("value", "b", x_edges=xe, y_edges=wide, values=np.full(n, np.nan), center=(0.0, 0.0, 0.0))
    _check(und, P.phase64(state, "value", "b", xe, wide, values=np.full(n, np.nan)))
    assert (und.stats.outside_count, und.stats.undefined_count, und.stats.binned_count) == (n, n, 0)
    assert not und.counts.any() and not und.mass.any()
    for bad in (0, 255, 300, 131072, -256):
        with pytest.raises(nb.NBodyError):
            sim.set_tuning("phase_segment_len", bad)
    sim.destroy()


@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_nonfinite_bodies_are_left_out_and_massless_bodies_binned(gpu, kind):
    nb = gpu
    n = 257
    xe, ye = nb.phase_edges(0.0, 0.8, 9), nb.phase_edges(-0.001, 0.001, 7)
    xe[-1], ye[0], ye[-1] = INF, -INF, INF  # every body that counts is binned, the massless one too
    for col, bad in ((1, np.nan), (4, np.inf), (9, -np.inf)):  # a position, a velocity, the mass
        state = make_state("uniform", n, seed=4)
        state[100, col] = bad
        state[7, 9] = 0.0
        sim = _sim(nb, kind, state, steps=0)
        back = nb.as_floats(sim.read_particles()).copy()
        pm = sim.phase_map("R", "w", x_edges=xe, y_edges=ye, weight="j_z", center=(0.0, 0.0, 0.0))
        sim.destroy()
        assert pm.stats.nonfinite == 1 and np.isfinite(pm.mass).all() and np.isfinite(pm.m_q2).all()
        _check(pm, P.phase64(back, "R", "w", xe, ye, weight="j_z"))
        # the massless body is counted where it lies: without it the counts drop by one
        rest = P.phase64(np.delete(back, np.flatnonzero(back[:, 9] == 0.0), axis=0), "R", "w", xe, ye, weight="j_z")
        assert int(pm.counts.sum()) - int(rest["counts"].sum()) == 1


@pytest.mark.parametrize("kind", ["naive", "tree"])
@pytest.mark.parametrize("segment", [256, 4096])
def test_agrees_with_the_projected_map_bit_for_bit(gpu, kind, segment):
    """x = a, y = b, weight = w on the edges of nb_map_edges is the projected map: the same cells by the same
    comparisons, the same terms, and -- what this test is for -- the same grouping and summing code, so counts, mass,
    m_w and m_w2 are the same bits at the same segment length."""
    nb = gpu
    state = make_state("disc", 4097, seed=6)
    sim = _sim(nb, kind, state, steps=3)
    sim.set_tuning("map_segment_len", segment)
    sim.set_tuning("phase_segment_len", segment)
    for (W, H), extent, axis, center in (((9, 7), (-0.3, 0.45, -0.6, 0.2), (0.0, 0.0, 1.0), "com"),
                                         ((100, 60), (-0.5, 0.5, -0.5, 0.5), (1.0, 2.0, 3.0), (0.05, -0.02, 0.01))):
        vel = None if center == "com" else (1e-3, -2e-3, 5e-4)
        m = sim.projected_map(W, H, extent=extent, axis=axis, center=center, velocity=vel, velocities=True)
        pm = sim.phase_map("a", "b", x_edges=nb.map_edges(extent[0], extent[1], W),
                           y_edges=nb.map_edges(extent[2], extent[3], H), weight="w", axis=axis, center=center,
                           velocity=vel)
        assert m.binned_count > 1000
        if segment == 256 and W == 9:  # two tiles: one of them holds several segments, so the combine path ran
            assert m.binned_count > 2 * 2 * 256
        assert pm.counts.tobytes() == m.counts.tobytes()
        assert pm.mass.tobytes() == m.mass.tobytes()
        assert pm.m_q.tobytes() == m.m_w.tobytes()
        assert pm.m_q2.tobytes() == m.m_w2.tobytes()
        s = pm.stats
        assert (s.binned_count, s.outside_count, s.nonfinite, s.max_count) == \
            (m.binned_count, m.outside_count, m.nonfinite, m.max_count)
        assert (s.binned_mass, s.outside_mass, s.total_mass) == (m.binned_mass, m.outside_mass, m.total_mass)
        assert s.center.tobytes() == m.center.tobytes() and s.velocity.tobytes() == m.velocity.tobytes()
    sim.destroy()


@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_the_com_centre_is_the_diagnostics(gpu, kind):
    nb = gpu
    sim = _sim(nb, kind, make_state("spherical", 1000, seed=3))
    pm = sim.phase_map("r", "u_r", x_range=(0.01, 1.0), y_range=(-0.5, 0.5), bins=(16, 8), log=(True, False))
    d = sim.diagnostics()
    sim.destroy()
    assert pm.stats.center.tobytes() == d.com.tobytes()
    assert pm.stats.velocity.tobytes() == (d.momentum / d.mass).tobytes()
    assert pm.stats.flags & 1 and pm.stats.total_mass == d.mass


def test_values(gpu):
    """An array made in numpy from read_particles() is binned like the built-in quantity it restates; stale values
    are refused; a NaN entry is undefined."""
    nb = gpu
    from wgpu_n_body_amd import _lib
    n = 1000
    sim = _sim(nb, "tree", make_state("spherical", n, seed=5))
    state = nb.as_floats(sim.read_particles()).copy()
    c = (0.01, 0.02, -0.01)
    q = P.quantities(state[:, 0:3].astype(np.float64), state[:, 3:6].astype(np.float64),
                     state[:, 9].astype(np.float64), center=c)
    kw = dict(x_range=(0.01, 1.0), y_range=(-0.3, 0.3), bins=(24, 16), log=(True, False), center=c)
    made_at = sim.step_num()
    builtin = sim.phase_map("r", "ua", weight="e_kin", **kw)
    as_x = sim.phase_map("value", "ua", weight="e_kin", values=q["r"], **kw)
    as_w = sim.phase_map("r", "ua", weight="value", values=q["e_kin"], check_step=made_at, **kw)
    assert builtin.stats.binned_count > 500
    for got in (as_x, as_w):
        assert got.counts.tobytes() == builtin.counts.tobytes() and got.mass.tobytes() == builtin.mass.tobytes()
        assert got.m_q.tobytes() == builtin.m_q.tobytes() and got.m_q2.tobytes() == builtin.m_q2.tobytes()
    holes = q["r"].copy()
    holes[::10] = np.nan
    und = sim.phase_map("value", "ua", values=holes, **kw)
    assert und.stats.undefined_count == 100 and und.stats.binned_count < builtin.stats.binned_count
    _check(und, P.phase64(state, "value", "ua", und.x_edges, und.y_edges, values=holes, center=c))
    with pytest.raises(ValueError):
        sim.phase_map("value", "ua", values=holes[:-1], **kw)
    with pytest.raises(nb.NBodyError):
        sim.phase_map("value", "ua", **kw)  # no array
    sim.encode()  # the tree reorders: the array is stale
    with pytest.raises(nb.NBodyError) as ex:
        sim.phase_map("value", "ua", values=q["r"], check_step=made_at, **kw)
    assert ex.value.code == _lib.NB_ERR_INVALID and "step" in str(ex.value)
    with pytest.raises(nb.NBodyError):
        sim.phase_map("r", "ua", weight="value", values=q["r"], check_step=made_at, **kw)
    sim.phase_map("r", "ua", weight="e_kin", check_step=made_at, **kw)  # no quantity is `value`: nothing to be stale
    sim.phase_map("value", "ua", values=q["r"], check_step=False, **kw)
    sim.destroy()


@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_bitwise_reproducible(gpu, kind):
    nb = gpu
    state = make_state("disc", 4097, seed=2)
    big = dict(x_range=(0.0, 0.6), y_range=(-0.1, 0.1), bins=(100, 60), weight="u_R", axis=(0.0, 0.0, 1.0))
    small = dict(x_range=(-0.5, 0.5), y_range=(-0.5, 0.5), bins=(5, 3), center=(0.0, 0.0, 0.0))
    calls = {
        "phase": lambda s: _blob(s.phase_map("R", "u_phi", **big)),
        "small": lambda s: _blob(s.phase_map("a", "h", **small)),
        "map": lambda s: s.projected_map(17, 33, extent=(-1.0, 1.0, -1.0, 1.0)).mass.tobytes(),
    }
    seen = {}
    for order in (["phase", "small", "map"], ["map", "small", "phase"], ["small", "map", "phase"]):
        sim = _sim(nb, kind, state)
        for name in order + order[::-1]:  # every first-use order; a smaller call after a larger one and back
            got = calls[name](sim)
            assert seen.setdefault(name, got) == got, f"{name} differs (first use order {order})"
        sim.destroy()
    # the smaller call is right, whatever ran before it
    sim = _sim(nb, kind, state)
    back = nb.as_floats(sim.read_particles()).copy()
    sim.phase_map("R", "u_phi", **big)
    got = sim.phase_map("a", "h", **small)
    sim.destroy()
    assert _blob(got) == seen["small"]
    _check(got, P.phase64(back, "a", "h", nb.phase_edges(-0.5, 0.5, 5), nb.phase_edges(-0.5, 0.5, 3)))


@pytest.mark.parametrize("case", ["naive", "tree", "tree_graph"])
def test_does_not_perturb_the_trajectory(gpu, case):
    nb = gpu
    n, steps = 4096, 6
    state = make_state("uniform", n, seed=9)
    finals = []
    for with_map in (False, True):
        sim = _sim(nb, "naive" if case == "naive" else "tree", state, steps=0)
        if case == "tree_graph":
            sim.set_tuning("tree_use_graph", 1)
        for k in range(steps):
            sim.encode()
            if with_map:
                pm = sim.phase_map("r", "u_r", x_range=(0.01, 1.0), y_range=(-0.002, 0.002), bins=(64, 48),
                                   log=(True, False), weight="u_t" if k % 2 else None,
                                   center="com" if k % 3 else (0, 0, 0))
                assert pm.stats.step_num == k + 1 and pm.stats.binned_count + pm.stats.outside_count == n
        finals.append(nb.as_floats(sim.read_particles()).copy())
        sim.destroy()
    assert np.array_equal(finals[0].view(np.uint32), finals[1].view(np.uint32))


def _params(nb, x, y, xe, ye, weight=None, axis=(0.0, 1.0, 0.0)):
    from wgpu_n_body_amd import _lib
    p = _lib.nb_phase_params()
    p.width, p.height = len(xe) - 1, len(ye) - 1
    p.flags = _lib.NB_PHASE_CENTER_COM | (_lib.NB_PHASE_WEIGHT if weight else 0)
    p.x, p.y, p.q = nb.phase_quantity(x), nb.phase_quantity(y), nb.phase_quantity(weight or "mass")
    DP = C.POINTER(C.c_double)
    p.x_edges, p.y_edges = xe.ctypes.data_as(DP), ye.ctypes.data_as(DP)
    p.step_num = _lib.NB_PHASE_ANY_STEP
    for k in range(3):
        p.axis[k] = axis[k]
    return p


def _raw(call, handle, p):
    from wgpu_n_body_amd import _lib
    cells = p.width * p.height
    counts = np.full(cells, 0xDEADBEEF, np.uint32)
    planes = np.full(3 * cells, -12345.5)
    st = _lib.nb_phase_stats()
    rc = call(handle, C.byref(p), counts.ctypes.data, planes.ctypes.data, C.byref(st))
    return rc, counts, planes, st


def test_null_outputs_no_bodies_and_refusals(gpu):
    """counts, planes and stats may each be null; a call with none of them measures nothing; planes that were not
    asked for stay untouched; no bodies are answered on the host; a shard and a several-GPU runner are refused."""
    nb = gpu
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    state = make_state("uniform", 1000, seed=3)
    sim = _sim(nb, "naive", state)
    xe, ye = nb.phase_edges(-0.5, 0.5, 17), nb.phase_edges(0.0, 0.0015, 33)
    p = _params(nb, "a", "speed", xe, ye, weight="w")
    rc, counts, planes, st = _raw(L.nb_phase_map_sim, sim._h, p)
    assert rc == 0 and st.binned_count > 0 and (st.x, st.y, st.q) == (0, 12, 7)
    assert L.nb_phase_map_sim(sim._h, C.byref(p), None, None, None) == 0
    only = np.zeros_like(counts)
    assert L.nb_phase_map_sim(sim._h, C.byref(p), only.ctypes.data, None, None) == 0 and np.array_equal(only, counts)
    pl = np.zeros_like(planes)
    assert L.nb_phase_map_sim(sim._h, C.byref(p), None, pl.ctypes.data, None) == 0 and pl.tobytes() == planes.tobytes()
    st2 = _lib.nb_phase_stats()
    assert L.nb_phase_map_sim(sim._h, C.byref(p), None, None, C.byref(st2)) == 0 and bytes(st2) == bytes(st)
    p1 = _params(nb, "a", "speed", xe, ye)
    rc, counts1, planes1, _ = _raw(L.nb_phase_map_sim, sim._h, p1)
    cells = 17 * 33
    assert rc == 0 and np.array_equal(counts1, counts) and planes1[:cells].tobytes() == planes[:cells].tobytes()
    assert np.all(planes1[cells:] == -12345.5)
    p.flags |= 8
    rc, c2, pl2, _ = _raw(L.nb_phase_map_sim, sim._h, p)
    assert rc == _lib.NB_ERR_INVALID and np.all(c2 == 0xDEADBEEF) and np.all(pl2 == -12345.5)
    sim.destroy()
    for kind in ("naive", "tree"):
        empty = _sim(nb, kind, np.zeros((0, 10), np.float32), steps=0)
        pm = empty.phase_map("a", "speed", x_edges=xe, y_edges=ye, weight="w", center=(0.5, 0.25, 0.0),
                             velocity=(1.0, 2.0, 3.0))
        assert np.array_equal(pm.stats.center, (0.5, 0.25, 0.0)) and np.array_equal(pm.stats.velocity, (1.0, 2.0, 3.0))
        assert not pm.counts.any() and not pm.mass.any() and not pm.m_q.any() and not pm.m_q2.any()
        s = pm.stats
        assert (s.n, s.nonfinite, s.binned_count, s.outside_count, s.undefined_count, s.max_count) == (0,) * 6
        assert np.isnan(empty.phase_map("a", "speed", x_edges=xe, y_edges=ye).stats.center).all()
        empty.destroy()
    sharded = nb.NaiveSim.from_particles(nb.SimParams(particle_num=64), None, state[:64], placement=nb.Placement(world=2))
    p = _params(nb, "a", "speed", xe, ye)
    assert _raw(L.nb_phase_map_sim, sharded._h, p)[0] == _lib.NB_ERR_UNSUPPORTED and b"sharded" in L.nb_last_error()
    sharded.destroy()
    r = nb.OfflineHeadless(nb.NaiveSim, nb.SimParams(particle_num=512), None,
                           lambda sp: nb.inits.uniform_init(sp, seed=1), device_ids=[0, 0])
    with pytest.raises(nb.NBodyError) as ex:
        r.phase_map("a", "speed", x_edges=xe, y_edges=ye)
    assert ex.value.code == _lib.NB_ERR_UNSUPPORTED
    r.destroy()


def test_distribution_and_derived_quantities(gpu):
    nb = gpu
    state = make_state("spherical", 1000, seed=11)
    sim = _sim(nb, "naive", state)
    e = nb.phase_edges(0.0, 0.9, 32)
    d = sim.distribution("r", e, center=(0.0, 0.0, 0.0))
    pm = sim.phase_map("r", "ua", x_range=(0.01, 1.0), y_range=(-0.3, 0.3), bins=(16, 8), log=(True, False),
                       weight="ub", center=(0.0, 0.0, 0.0))
    sim.destroy()
    ref = P.phase64(state, "r", "mass", e, [-INF, INF])
    assert d.counts.shape == (1, 32) and np.array_equal(d.counts[0], ref["counts"][0])
    assert 0 < d.stats.outside_count == ref["outside_count"] and d.stats.binned_count > 500
    assert np.array_equal(d.marginal_x(), d.mass[0]) and d.marginal_y().shape == (1,)
    empty = pm.mass == 0.0
    assert empty.any() and not empty.all()
    for got in (pm.mean_q, pm.sigma_q, pm.density):
        assert np.array_equal(np.isnan(got), empty)
    assert np.all(pm.sigma_q[~empty] >= 0.0)
    area = np.outer(np.diff(pm.y_edges), np.diff(pm.x_edges))
    assert np.allclose(pm.density[~empty], (pm.mass / area)[~empty], rtol=1e-12)
    assert abs(pm.marginal_x().sum() - pm.stats.binned_mass) <= TOL * pm.stats.binned_mass
    with pytest.raises(ValueError):
        d.mean_q


def test_runner_mirror_and_cli(gpu, tmp_path):
    """nb_phase_map_runner equals nb_phase_map_sim on nb_runner_sim, and headless --phase (the C++ mirror over
    nb_phase_map_runner) writes what the Python runner returns."""
    nb = gpu
    from wgpu_n_body_amd import _lib
    cli = os.path.join(ROOT, "wgpu_n_body_amd", "headless")
    base = [cli, "--sim", "tree", "--n", "4096", "--init", "disc", "--steps", "4"]
    out = tmp_path / "phase"
    out.mkdir()
    p = subprocess.run(base + ["--phase", str(out), "--phase-every", "2", "--phase-x", "R,0.01,1,64,log", "--phase-y",
                               "u_phi,-0.15,0.15,48", "--phase-weight", "w", "--phase-axis", "0,0,1"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    plain = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "phase" not in plain.stdout
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("phase ")]
    assert sorted(os.listdir(out)) == ["phase_000000.npy", "phase_000002.npy", "phase_000004.npy"] and len(lines) == 3
    blank = lambda text: [re.sub(r"\d+", "#", ln) for ln in text.splitlines() if not ln.startswith("phase ")]  # noqa: E731
    assert blank(p.stdout) == blank(plain.stdout)
    bad = subprocess.run(base + ["--phase", str(out), "--phase-x", "R,0.01,1,64,lin", "--phase-y", "w,-1,1,8"],
                         capture_output=True, text=True, timeout=300)
    assert bad.returncode == 2 and "--phase-x" in bad.stderr

    runner = nb.OfflineHeadless(nb.TreeSim, nb.SimParams(particle_num=4096), nb.AddParams.TreeSimParams(0.75),
                                lambda sp: nb.inits.disc_init(sp, seed=0))
    kw = dict(x_range=(0.01, 1.0), y_range=(-0.15, 0.15), bins=(64, 48), log=(True, False), weight="w",
              axis=(0.0, 0.0, 1.0))
    ours = [runner.phase_map("R", "u_phi", **kw)]
    for k in range(4):
        runner.step()
        if (k + 1) % 2 == 0:
            ours.append(runner.phase_map("R", "u_phi", **kw))
    pr = _params(nb, "R", "u_phi", ours[0].x_edges, ours[0].y_edges, weight="w", axis=(0.0, 0.0, 1.0))
    via_runner = _raw(_lib.lib().nb_phase_map_runner, runner._h, pr)
    via_sim = _raw(_lib.lib().nb_phase_map_sim, runner.sim._h, pr)
    runner.destroy()
    assert via_runner[0] == via_sim[0] == 0
    assert all(a.tobytes() == b.tobytes() for a, b in zip(via_runner[1:3], via_sim[1:3]))
    assert bytes(via_runner[3]) == bytes(via_sim[3]) and np.array_equal(via_sim[1].reshape(48, 64), ours[-1].counts)

    for j, (ln, o) in enumerate(zip(lines, ours)):
        a = np.load(out / ("phase_%06d.npy" % (2 * j)))
        s = o.stats
        assert a.shape == (4, 48, 64) and a.dtype == np.dtype("<f8") and s.step_num == 2 * j
        words = [int(x) for x in ln.split()[1:]]
        assert words[0] == s.step_num and words[1] == int(a[0].sum()) and words[1] + words[2] + words[4] == s.n
        assert words[5] == int(a[0].max())
        if j == 0:  # the same seeded init, no step yet: the file is the Python call, bit for bit
            assert words == [0, s.binned_count, s.outside_count, s.undefined_count, s.nonfinite, s.max_count]
            assert np.array_equal(a[0], o.counts.astype(np.float64))
            for k, plane in enumerate((o.mass, o.m_q, o.m_q2)):
                assert a[1 + k].tobytes() == plane.tobytes(), k
        else:       # (the trajectory of two runs of the tree is not specified bit for bit)
            assert abs(int(a[0].sum()) - s.binned_count) <= 4096
    assert ours[0].stats.binned_count > 2000
