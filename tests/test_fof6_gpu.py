"""nb_fof6_sim on the device (csrc/nb_fof6.hip) against the numpy restatements of its rule (tests/fof6_ref.py) on the
read-back state: labels, group_of, counts and every integer of the stats equal, every sum to 1e-10 of its sum of
|term|.  Tiny and degenerate states; the edge of the rule; partitions a position-only finder gets differently; one
cell at wave and chunk borders in three layouts; neighbour cells with partial joins; random states; equal velocities
against nb_sim_fof byte for byte; refinement; a velocity offset; reproducibility; the tuning keys; permutations; the
capacity; cell borders, far states and a multi-pass sort; the refusals; that a call does not perturb the trajectory;
the runner, the C++ mirror and the CLI; the passes that take the catalogue.  `-m gpu`."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from tests import fof6_ref as F6
from tests import fof_ref as F
from tests.helpers import ROOT, make_state

pytestmark = pytest.mark.gpu

TOL = 1e-10  # of the sum of |term|: TOL of tests/test_fof_gpu.py, the same summation code
FILL = 0xDEADBEEF


def _sim(nb, kind, state, theta=0.75):
    sp = nb.SimParams(particle_num=state.shape[0])
    if kind == "naive":
        return nb.NaiveSim.from_particles(sp, None, state)
    return nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(theta), state)


def _raw(sim, link, vlink, min_members=1, capacity=None, call=None, handle=None, n=None):
    """The C call with every buffer pre-filled; vlink None: nb_sim_fof."""
    from wgpu_n_body_amd import _lib
    n = int(sim.sim_params().particle_num) if n is None else n
    if vlink is None:
        p = _lib.nb_fof_params()
        call = call or _lib.lib().nb_sim_fof
    else:
        p = _lib.nb_fof6_params()
        p.vlink = vlink
        call = call or _lib.lib().nb_fof6_sim
    p.link, p.min_members = link, min_members
    cap = n // min_members if capacity is None else capacity
    labels, group_of = np.full(n, FILL, np.uint32), np.full(n, FILL, np.uint32)
    rows = np.zeros(cap + 1, _lib.FOF_GROUP_DTYPE)
    rows["label"] = FILL
    st = _lib.nb_fof_stats()
    rc = call(handle or sim._h, C.byref(p), labels.ctypes.data, group_of.ctypes.data, rows.ctypes.data, cap,
              C.byref(st))
    return SimpleNamespace(rc=rc, labels=labels, group_of=group_of, rows=rows, st=st, cap=cap,
                           bytes=labels.tobytes() + group_of.tobytes() + rows.tobytes() + bytes(st))


def _fof6(sim, link, vlink, min_members=1, **kw):
    from wgpu_n_body_amd import _lib
    g = _raw(sim, link, vlink, min_members, **kw)
    assert g.rc == 0, _lib.lib().nb_last_error()
    return g


def _check(g, ref, tol=TOL):
    """Every integer equal, every sum within tol of the restatement's sum of |term|; the identities; rows beyond the
    catalogue untouched."""
    st = g.st
    for k in ("n", "nonfinite", "components", "groups", "grouped_bodies", "largest_count", "largest_label"):
        assert getattr(st, k) == ref[k], (k, getattr(st, k), ref[k])
    assert np.array_equal(g.labels, ref["labels"]), np.flatnonzero(g.labels != ref["labels"])[:8]
    assert np.array_equal(g.group_of, ref["group_of"]), np.flatnonzero(g.group_of != ref["group_of"])[:8]
    k = min(ref["groups"], g.cap)
    rows = g.rows[:k]
    assert np.array_equal(rows["label"], ref["rows_label"][:k]) and np.array_equal(rows["count"], ref["rows_count"][:k])
    assert np.all(g.rows["label"][k:] == FILL) and not g.rows["mass"][k:].any()
    got = np.concatenate([rows["mass"][:, None], rows["mx"], rows["mv"], rows["mr2"][:, None], rows["mv2"][:, None]],
                         axis=1)
    err = np.abs(got - ref["sums"][:k])
    assert np.all(err <= tol * ref["scale"][:k] + 1e-300), float((err / (ref["scale"][:k] + 1e-300)).max())
    sizes = np.unique(g.labels[g.labels != F.NONE], return_counts=True)[1]
    assert st.nonfinite + int(sizes.sum()) == st.n and st.components == sizes.size
    if g.cap >= ref["groups"]:
        assert int(rows["count"].sum()) == st.grouped_bodies


def _state_of(nb, sim):
    return nb.as_floats(sim.read_particles()).copy()


def _prepared(nb, kind, state, step=True):
    """The simulator and the state it holds: a TreeSim after one step, in tree order."""
    sim = _sim(nb, kind, state)
    if kind == "tree" and step:
        sim.encode()
    return sim, _state_of(nb, sim)


# ---- tiny and degenerate states ------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 2])
@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_tiny_states(gpu, kind, n):
    nb = gpu
    state = F6.state_of(np.array([(0.1, 0.2, 0.3), (0.15, 0.2, 0.3)])[:n], np.array([(0.0, 0, 0), (0.3, 0, 0)])[:n])
    sim = _sim(nb, kind, state)
    for link, vlink, comps in ((0.1, 1.0, min(n, 1)), (0.1, 0.2, n), (0.01, 1.0, n)):
        for mm in (1, 2):
            g = _fof6(sim, link, vlink, mm)
            _check(g, F6.fof6_brute(state, link, vlink, mm))
            assert g.st.components == comps
    if n == 0:
        assert (g.st.largest_count, g.st.largest_label, tuple(g.st.cells)) == (0, F.NONE, (0, 0, 0))
    sim.destroy()


def test_no_body_counts(gpu):
    """n > 0 and every body non-finite -- a third each in position, velocity and mass: no cell, no component."""
    nb = gpu
    state = F._state(np.full((300, 3), np.nan))
    state[::3, 0], state[1::3, 4], state[2::3, 9] = 0.5, np.inf, -np.inf
    sim = _sim(nb, "naive", state)
    g = _fof6(sim, 0.1, 0.1)
    _check(g, F6.fof6_brute(state, 0.1, 0.1))
    assert (g.st.nonfinite, g.st.components, g.st.groups, g.st.largest_label) == (300, 0, 0, F.NONE)
    assert np.all(g.labels == F.NONE) and np.all(g.group_of == F.NONE) and tuple(g.st.cells) == (0, 0, 0)
    sim.destroy()


def test_a_third_of_the_bodies_non_finite(gpu):
    nb = gpu
    state = F6.gaussian_clumps(1500)
    state[0::9, 1], state[1::9, 4], state[2::9, 9] = np.nan, np.inf, -np.inf
    sim = _sim(nb, "naive", state)
    state = _state_of(nb, sim)
    for mm in (1, 5):
        g = _fof6(sim, 0.02, 0.1, mm)
        _check(g, F6.fof6_brute(state, 0.02, 0.1, mm))
    assert g.st.nonfinite == 501 and g.st.groups >= 3
    sim.destroy()


def test_the_rule_at_its_edge(gpu):
    """link = vlink = 1: dx = (0.5, 0.5, 0.5), dv = (0.5, 0, 0) is exactly 1, friends; the next float32 up in one
    component of dv (clause 2 fails) or of dx is not; dx = (1, 0, 0), dv = 0 is the edge of clause 1, the next float32
    up fails clause 1 -- and clause 2 with it; dx = (0.75, 0.75, 0.75), dv = 0 fails clause 1 at d2 = 1.6875."""
    nb = gpu
    up = np.nextafter(np.float32(0.5), np.float32(1.0))
    for dx, dv, friends in (((0.5, 0.5, 0.5), (0.5, 0, 0), True), ((0.5, up, 0.5), (0.5, 0, 0), False),
                            ((0.5, 0.5, 0.5), (up, 0, 0), False), ((0.5, 0.5, 0.5), (0, 0, -up), False),
                            ((1, 0, 0), (0, 0, 0), True),
                            ((np.nextafter(np.float32(1.0), np.float32(2.0)), 0, 0), (0, 0, 0), False),
                            ((0.75, 0.75, 0.75), (0, 0, 0), False)):
        state = F6.state_of([(0, 0, 0), dx], [(0, 0, 0), dv])  # (from 0: every difference is the number itself)
        sim = _sim(nb, "naive", state)
        for boxes in (1, 0):
            sim.set_tuning("fof6_boxes", boxes)
            g = _fof6(sim, 1.0, 1.0)
            _check(g, F6.fof6_brute(state, 1.0, 1.0))
            assert g.st.components == (1 if friends else 2), (dx, dv, boxes)
        sim.destroy()


# ---- partitions a position-only finder gets differently --------------------------------------------------------

def test_coincident_positions(gpu):
    """600 bodies at one point: two velocity clumps give two groups; a velocity chain whose links are within vlink and
    whose ends are far apart gives one."""
    nb = gpu
    rng = np.random.default_rng(5)
    pos = np.tile([[0.3, -0.2, 0.1]], (600, 1))
    vel = rng.uniform(-0.01, 0.01, (600, 3))
    vel[rng.permutation(600)[:250], 2] += 3.0
    chain = np.zeros((600, 3))
    chain[:, 0] = rng.permutation(600) * 0.09
    for v, comps in ((vel, 2), (chain, 1)):
        state = F6.state_of(pos, v)
        sim = _sim(nb, "naive", state)
        g = _fof6(sim, 0.01, 0.1)
        _check(g, F6.fof6_brute(state, 0.01, 0.1))
        assert g.st.components == comps and _fof6(sim, 0.01, None).st.components == 1
        sim.destroy()


@pytest.fixture(scope="module")
def streams():
    return F6.crossing_streams()


def test_crossing_streams(gpu, streams):
    nb = gpu
    sim = _sim(nb, "naive", streams)
    g = _fof6(sim, 0.015, 0.5, 2)
    _check(g, F6.fof6_brute(streams, 0.015, 0.5, 2))
    assert g.st.groups == 2 and g.rows["count"][:2].tolist() == [200, 200]
    assert sim.fof_groups(0.015, min_members=2).stats.groups == 1
    sim.destroy()


# ---- shapes where the pair loop can go wrong -------------------------------------------------------------------

@pytest.mark.parametrize("chunk", [64, 1024])
@pytest.mark.parametrize("layout", ["cold", "parity", "last"])
@pytest.mark.parametrize("n", [63, 64, 65, 130, 1025])
def test_one_cell_at_wave_and_chunk_borders(gpu, n, layout, chunk):
    nb = gpu
    state = F6.one_cell(n, layout)
    sim = _sim(nb, "naive", state)
    sim.set_tuning("fof_chunk_len", chunk)
    ref = F6.fof6_brute(state, 1.0, 1.0, 2)
    for boxes in (1, 0):
        sim.set_tuning("fof6_boxes", boxes)
        g = _fof6(sim, 1.0, 1.0, 2)
        _check(g, ref)
        assert tuple(g.st.cells) == (1, 1, 1)
    want = {"cold": (1, 1), "parity": (2, 2), "last": (n - 1, 1)}[layout]
    assert (g.st.components, g.st.groups) == want
    if layout == "last":
        assert g.labels[n - 1] == n // 3 and g.rows["count"][0] == 2
    sim.destroy()


@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_neighbour_cells_with_partial_joins(gpu, kind):
    """One body of cell A -- not its first -- has friends in cell B, and another body of A has friends in a different
    component of B; the other 98 bodies of A are friends of nobody."""
    nb = gpu
    sim = _sim(nb, kind, F6.partial_joins())
    state = _state_of(nb, sim)
    ref = F6.fof6_brute(state, 1.0, 1.0, 2)
    for chunk, boxes in ((1024, 1), (64, 1), (64, 0)):
        sim.set_tuning("fof_chunk_len", chunk)
        sim.set_tuning("fof6_boxes", boxes)
        g = _fof6(sim, 1.0, 1.0, 2)
        _check(g, ref)
        assert tuple(g.st.cells)[0] == 2 and g.st.components == 100 and g.rows["count"][:2].tolist() == [51, 51]
    if kind == "naive":  # (the order the state was given in)
        assert g.rows["label"][:2].tolist() == [37, 81]
    sim.destroy()


CASES = F6.synthetic_cases(small=False)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c[0] for c in CASES])
def test_synthetic_cases(gpu, idx):
    """fof_ref's states -- chains, lattices, coincident bodies, bodies on cell borders and far from the origin -- under
    four velocity drifts, and this rule's own."""
    nb = gpu
    name, state, link, vlink = CASES[idx]
    sim = _sim(nb, "naive", state)
    if state.shape[0] <= 512:
        labels = F6.fof6_brute(state, link, vlink)["labels"]
    else:
        labels = F6.labels_grid(state, link, vlink)
    for mm in (1, 20):
        g = _fof6(sim, link, vlink, mm)
        _check(g, F.catalogue(state, labels, link, mm))
    assert g.st.cell_side == F.cell_side(link)
    sim.destroy()


# ---- larger random states --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def clumps():
    state = F6.gaussian_clumps(4096)
    return state, F6.fof6_brute(state, 0.02, 0.1, 5)


@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_gaussian_clumps_against_brute_force(gpu, clumps, kind):
    nb = gpu
    state0, ref = clumps
    sim, state = _prepared(nb, kind, state0)
    if kind == "tree":
        ref = F6.fof6_brute(state, 0.02, 0.1, 5)
    g = _fof6(sim, 0.02, 0.1, 5)
    _check(g, ref)
    assert g.st.groups >= 3 and g.st.largest_count > 300
    sim.destroy()


def _median_neighbour_distance(pos):
    p = pos.astype(np.float64)
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d2, np.inf)
    return float(np.sqrt(np.median(d2.min(axis=1))))


def test_hundred_thousand_against_the_grid(gpu):
    nb = gpu
    n = 100000
    state = F6.with_velocities(make_state("spherical", n, seed=3), 7, 0.3)
    sim = _sim(nb, "naive", state)
    state = _state_of(nb, sim)
    # twice the median distance to the nearest neighbour, scaled from a sample of 2,048 bodies: thousands of groups
    link, vlink = 2.0 * _median_neighbour_distance(state[:2048, 0:3]) * (2048 / n) ** (1.0 / 3.0), 0.15
    g = _fof6(sim, link, vlink, 5)
    _check(g, F6.fof6_grid(state, link, vlink, 5))
    assert g.st.groups > 10
    sim.destroy()


def test_multi_pass_sort(gpu):
    """65,536 bodies over a grid of more than 2^16 cells: three sort passes, several blocks of every scan."""
    nb = gpu
    state = F6.with_velocities(make_state("uniform", 65536, seed=5), 8, 1.0)
    sim = _sim(nb, "naive", state)
    ext = state[:, 0:3].max(axis=0) - state[:, 0:3].min(axis=0)
    link = 0.7 * float((ext.prod() / 65536) ** (1.0 / 3.0))
    g = _fof6(sim, link, 0.5, 2)
    assert int(g.st.cells[0]) * int(g.st.cells[1]) * int(g.st.cells[2]) > 1 << 16
    _check(g, F6.fof6_grid(state, link, 0.5, 2))
    assert 100 < g.st.groups and g.st.components < 65536
    sim.destroy()


# ---- cross-checks ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_equal_velocities_give_the_bytes_of_fof(gpu, kind):
    nb = gpu
    state = make_state("spherical", 8192, seed=7)
    state[:, 3:6] = np.float32([0.25, -1.5, 3.0])
    state[::50, 9] = np.nan  # (and the bodies that do not count are the same)
    sim = _sim(nb, kind, state)
    for link, vlink, mm in ((0.02, 1.0, 2), (0.05, 1e-30, 20)):
        assert _fof6(sim, link, vlink, mm).bytes == _fof6(sim, link, None, mm).bytes
    sim.destroy()


def test_refinement_and_velocity_offset(gpu):
    """Every phase-space group lies inside one nb_sim_fof group; adding (8, -16, 4) to velocities that are multiples
    of 2^-10 below 4 keeps every velocity exact, and the partition."""
    nb = gpu
    state = F6.with_velocities(make_state("disc", 8192, seed=2), 9, 1.0)
    state[:, 3:6] = np.clip(np.round(state[:, 3:6] * 1024.0) / 1024.0, -3.0, 3.0)
    sim = _sim(nb, "naive", state)
    link, vlink = 0.02, 0.4
    g, f = _fof6(sim, link, vlink, 2), _fof6(sim, link, None, 2)
    sim.destroy()
    assert F6.refines(g.labels, f.labels) and g.st.components > f.st.components and g.st.groups > 3
    moved = state.copy()
    moved[:, 3:6] += np.float32([8.0, -16.0, 4.0])
    assert np.array_equal((moved[:, 3:6] - np.float32([8.0, -16.0, 4.0])), state[:, 3:6])
    sim = _sim(nb, "naive", moved)
    m = _fof6(sim, link, vlink, 2)
    sim.destroy()
    assert np.array_equal(m.labels, g.labels) and np.array_equal(m.group_of, g.group_of)
    assert np.array_equal(m.rows["count"], g.rows["count"])


@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_bitwise_reproducible(gpu, kind):
    nb = gpu
    sim, state = _prepared(nb, kind, F6.with_velocities(make_state("disc", 4097, seed=2), 3, 0.5))
    g1, g2 = _fof6(sim, 0.02, 0.3, 3), _fof6(sim, 0.02, 0.3, 3)
    _fof6(sim, 0.05, 1.0, 1)  # another shape between
    _fof6(sim, 0.02, None, 3)  # ... and the pass that shares the workspace
    g3 = _fof6(sim, 0.02, 0.3, 3)
    sim.destroy()
    assert g1.st.groups > 0 and g1.bytes == g2.bytes == g3.bytes


def test_tuning_keys_do_not_change_a_bit(gpu):
    """One cell of 3,000 bodies in two velocity clumps beside scattered ones."""
    nb = gpu
    rng = np.random.default_rng(8)
    pos = np.concatenate([rng.uniform(0.0, 1e-4, (3000, 3)) + 0.25, F._ball(rng, 3000, 0.2, (0.25, 0.25, 0.25))])
    vel = rng.normal(0.0, 0.02, (6000, 3))
    vel[:1500, 0] += 2.0
    perm = rng.permutation(6000)
    state = F6.state_of(pos[perm], vel[perm], 9)
    sim = _sim(nb, "naive", state)
    link, vlink = 0.01, 0.2
    base = _fof6(sim, link, vlink, 2)
    _check(base, F6.fof6_grid(state, link, vlink, 2))
    assert base.st.largest_count >= 1500
    for key, value in (("fof_chunk_len", 64), ("fof6_boxes", 0), ("fof_chunk_len", 65536), ("fof6_boxes", 1),
                       ("fof_chunk_len", 1024)):
        sim.set_tuning(key, value)
        assert _fof6(sim, link, vlink, 2).bytes == base.bytes, (key, value)
    with pytest.raises(nb.NBodyError):
        sim.set_tuning("fof6_boxes", 2)
    sim.destroy()


def test_a_permutation_permutes_the_partition(gpu):
    nb = gpu
    state = F6.gaussian_clumps(4096, seed=6)
    perm = np.random.default_rng(4).permutation(4096)
    parts = []
    for s, back in ((state, np.arange(4096)), (state[perm], perm)):
        sim = _sim(nb, "naive", s)
        g = _fof6(sim, 0.02, 0.1)
        sim.destroy()
        parts.append({frozenset(int(back[i]) for i in grp) for grp in F.partition(g.labels)})
    assert parts[0] == parts[1] and 1 < len(parts[0]) < 4096


def test_capacity_smaller_than_the_catalogue(gpu, clumps):
    nb = gpu
    state, _ = clumps
    sim = _sim(nb, "naive", state)
    full = _fof6(sim, 0.02, 0.1, 2)
    ref = F6.fof6_grid(state, 0.02, 0.1, 2)
    assert full.st.groups > 8
    for cap in (0, 1, 7):
        g = _fof6(sim, 0.02, 0.1, 2, capacity=cap)
        _check(g, ref)
        assert g.st.groups == full.st.groups and bytes(g.st) == bytes(full.st)
        assert g.rows[:cap].tobytes() == full.rows[:cap].tobytes()
    sim.destroy()


def test_null_outputs(gpu, clumps):
    nb = gpu
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    state, _ = clumps
    n = len(state)
    sim = _sim(nb, "naive", state)
    full = _fof6(sim, 0.02, 0.1, 2)
    p = _lib.nb_fof6_params()
    p.link, p.vlink, p.min_members = 0.02, 0.1, 2
    assert L.nb_fof6_sim(sim._h, C.byref(p), None, None, None, 0, None) == 0
    st = _lib.nb_fof_stats()
    assert L.nb_fof6_sim(sim._h, C.byref(p), None, None, None, 0, C.byref(st)) == 0 and bytes(st) == bytes(full.st)
    lab = np.zeros(n, np.uint32)
    assert L.nb_fof6_sim(sim._h, C.byref(p), lab.ctypes.data, None, None, 0, None) == 0
    assert np.array_equal(lab, full.labels)
    rows = np.zeros(n // 2, _lib.FOF_GROUP_DTYPE)
    assert L.nb_fof6_sim(sim._h, C.byref(p), None, None, rows.ctypes.data, n // 2, None) == 0
    assert rows[:full.st.groups].tobytes() == full.rows[:full.st.groups].tobytes()
    sim.destroy()


# ---- refusals, the trajectory, the other layers ----------------------------------------------------------------

def test_refusals(gpu):
    nb = gpu
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    s = make_state("uniform", 64, seed=1)
    sim = _sim(nb, "naive", s)
    for link, vlink, mm in ((0.0, 1.0, 1), (0.1, float("nan"), 1), (0.1, 0.0, 1), (0.1, 1.0, 0)):
        g = _raw(sim, link, vlink, mm, capacity=8)
        assert g.rc == _lib.NB_ERR_INVALID and L.nb_last_error()
        assert np.all(g.labels == FILL) and np.all(g.group_of == FILL) and np.all(g.rows["label"] == FILL)
    sim.destroy()
    # one far body pushes an axis past 2^21 cells: refused after the synchronisation, nothing written
    far = s.copy()
    far[17, 0] = 3.0e4
    sim = _sim(nb, "naive", far)
    g = _raw(sim, 0.01, 1.0)
    assert g.rc == _lib.NB_ERR_INVALID and b"cells" in L.nb_last_error() and b"fof6" in L.nb_last_error()
    assert np.all(g.labels == FILL) and np.all(g.group_of == FILL) and np.all(g.rows["label"] == FILL)
    assert bytes(g.st) == bytes(_lib.nb_fof_stats())
    ok = _fof6(sim, 0.1, 1.0)  # the simulator stays usable, and a link the grid can carry goes through
    _check(ok, F6.fof6_brute(far, 0.1, 1.0))
    with pytest.raises(nb.NBodyError) as ex:
        sim.phase_space_groups(0.01, 1.0)
    assert ex.value.code == _lib.NB_ERR_INVALID
    sim.destroy()
    # a sharded simulator (rank 0 of 2)
    sharded = nb.NaiveSim.from_particles(nb.SimParams(particle_num=64), None, s, placement=nb.Placement(world=2))
    g = _raw(sharded, 0.1, 1.0, n=64)
    assert g.rc == _lib.NB_ERR_UNSUPPORTED and b"sharded" in L.nb_last_error()
    sharded.destroy()
    # a several-GPU runner, both ranks on device 0
    r = nb.OfflineHeadless(nb.NaiveSim, nb.SimParams(particle_num=512), None,
                           lambda p: nb.inits.uniform_init(p, seed=1), device_ids=[0, 0])
    with pytest.raises(nb.NBodyError) as ex:
        r.phase_space_groups(0.1, 1.0)
    assert ex.value.code == _lib.NB_ERR_UNSUPPORTED
    r.destroy()


@pytest.mark.parametrize("case", ["naive", "tree", "tree_graph"])
def test_does_not_perturb_the_trajectory(gpu, case):
    nb = gpu
    n, steps = 4096, 10
    state = make_state("uniform", n, seed=9)
    finals = []
    for with_groups in (False, True):
        sim = _sim(nb, "naive" if case == "naive" else "tree", state)
        if case == "tree_graph":
            sim.set_tuning("tree_use_graph", 1)
        for k in range(steps):
            sim.encode()
            if with_groups:
                g = sim.phase_space_groups(0.03 if k % 2 else 0.06, 5.0, min_members=2, labels=k % 3 == 0)
                assert g.stats.step_num == k + 1 and g.stats.n == n and g.stats.groups > 0
        finals.append(nb.as_floats(sim.read_particles()).copy())
        sim.destroy()
    assert np.array_equal(finals[0].view(np.uint32), finals[1].view(np.uint32))


def test_python_wrapper_and_parent_rows(gpu, streams):
    nb = gpu
    sim = _sim(nb, "naive", streams)
    g = sim.phase_space_groups(0.015, 0.5, min_members=2)
    raw = _fof6(sim, 0.015, 0.5, 2)
    assert isinstance(g, nb.PhaseSpaceGroups) and (g.link, g.vlink, g.min_members) == (0.015, 0.5, 2)
    assert np.array_equal(g.labels, raw.labels) and np.array_equal(g.group_of, raw.group_of)
    assert g.rows.tobytes() == raw.rows[:2].tobytes() and g.count.tolist() == [200, 200]
    assert np.allclose(g.velocity, [(1, 0, 0), (0, 1, 0)], atol=0.01) and np.all(g.sigma < 0.02)
    assert sim.phase_space_groups(0.015, 0.5, labels=False).labels is None
    assert sim.phase_space_groups(0.015, 0.5).min_members == 20
    parent = sim.fof_groups(0.015, min_members=2)
    assert g.parent_rows(parent).tolist() == [0, 0]
    assert g.parent_rows(sim.fof_groups(0.015, min_members=401)).tolist() == [F.NONE, F.NONE]
    with pytest.raises(ValueError):
        g.parent_rows(sim.fof_groups(0.02, min_members=2))
    sim.encode()
    with pytest.raises(ValueError):
        g.parent_rows(sim.fof_groups(0.015, min_members=2))
    sim.destroy()


def test_the_passes_that_take_a_catalogue(gpu, clumps):
    nb = gpu
    state, _ = clumps
    sim = _sim(nb, "naive", state)
    g = sim.phase_space_groups(0.02, 0.1, min_members=50)
    m = len(g.rows)
    assert m >= 3 and np.isfinite(g.com).all()
    a, b = sim.group_shapes(g), sim.shapes_of(g.group_of, m, centers=g.com, velocities=g.velocity)
    assert a.rows.tobytes() == b.rows.tobytes() and np.array_equal(a.catalogue_rows, np.arange(m))
    a, b = sim.group_radii(g), sim.radii_of(g.group_of, m, centers=g.com)
    assert a.rows.tobytes() == b.rows.tobytes()
    rows, a = sim.group_profiles(g, rmin=1e-3, rmax=0.2, nbins=8)
    b = sim.halo_profiles(g.com, velocities=g.velocity, rmin=1e-3, rmax=0.2, nbins=8)
    assert np.array_equal(rows, np.arange(m))
    for f in ("count", "mass", "m_r", "m_ur", "m_ur2", "m_u2", "ang", "inside_mass"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    sim.destroy()


def test_runner_and_cli(gpu):
    """nb_fof6_runner equals nb_fof6_sim on nb_runner_sim, and headless --fof6 (the C++ mirror over nb_fof6_runner)
    prints what the Python runner returns."""
    nb = gpu
    from wgpu_n_body_amd import _lib
    cli = os.path.join(ROOT, "wgpu_n_body_amd", "headless")
    base = [cli, "--sim", "tree", "--n", "4096", "--init", "disc", "--steps", "2"]
    link, vlink = 0.02, 0.5
    p = subprocess.run(base + ["--fof6", "2", "--fof6-link", repr(link), "--fof6-vlink", repr(vlink), "--fof6-min", "5",
                               "--fof6-top", "3"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    plain = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "fof6" not in plain.stdout
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("fof6 ")]
    tops = [ln for ln in p.stdout.splitlines() if ln.startswith("fof6_group ")]
    assert len(lines) == 2
    blank = lambda text: [re.sub(r"\d+", "#", ln) for ln in text.splitlines() if not ln.startswith("fof6")]  # noqa: E731
    assert blank(p.stdout) == blank(plain.stdout)
    bad = subprocess.run(base + ["--fof6", "2", "--fof6-link", repr(link)], capture_output=True, text=True, timeout=300)
    assert bad.returncode == 2 and "--fof6-vlink" in bad.stderr

    runner = nb.OfflineHeadless(nb.TreeSim, nb.SimParams(particle_num=4096), nb.AddParams.TreeSimParams(0.75),
                                lambda sp: nb.inits.disc_init(sp, seed=0))
    o = runner.phase_space_groups(link, vlink, min_members=5)
    runner.step()
    via_runner = _raw(None, link, vlink, 5, call=_lib.lib().nb_fof6_runner, handle=runner._h, n=4096)
    via_sim = _raw(runner.sim, link, vlink, 5)
    state = _state_of(nb, runner.sim)
    runner.destroy()
    assert via_runner.rc == via_sim.rc == 0 and via_runner.bytes == via_sim.bytes
    _check(via_sim, F6.fof6_grid(state, link, vlink, 5))

    # the same seeded init, no step yet: the line is the Python call
    assert [int(x) for x in lines[0].split()[1:]] == [0, o.stats.groups, o.stats.grouped_bodies, o.stats.largest_count]
    assert o.stats.groups >= 3 and int(lines[1].split()[1]) == 2
    for ln, r in zip([ln.split() for ln in tops[:3]], o.by_size()[:3]):
        assert [int(x) for x in ln[1:5]] == [0, int(r), int(o.label[r]), int(o.count[r])]
        assert float(ln[5]) == pytest.approx(o.mass[r], rel=1e-5)
