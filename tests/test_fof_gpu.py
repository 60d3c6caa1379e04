"""nb_sim_fof on the device (csrc/nb_fof.hip) against the numpy restatements of its rule (tests/fof_ref.py) on
the read-back state: labels, group_of, counts and every integer of the stats equal, every sum to 1e-10 of its sum
of |term|; the edge of the rule, chains, lattices, coincident bodies, dense neighbours that are not friends, bodies
on cell borders and far from the origin; the inits with non-finite bodies; a multi-pass sort; the tuning keys;
bitwise reproducibility; permutations; the capacity; the refusals; that a call does not perturb the trajectory; the
diagnostics; the runner, the C++ mirror and the CLI.  `-m gpu`."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from tests import fof_ref as F
from tests.helpers import ROOT, make_state

pytestmark = pytest.mark.gpu

TOL = 1e-10  # of the sum of |term|: TOL of tests/test_map_gpu.py
FILL = 0xDEADBEEF


def _sim(nb, kind, state, theta=0.75):
    sp = nb.SimParams(particle_num=state.shape[0])
    if kind == "naive":
        return nb.NaiveSim.from_particles(sp, None, state)
    return nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(theta), state)


def _raw(sim, link, min_members=1, capacity=None, call=None, handle=None, n=None):
    """The C call with every buffer pre-filled."""
    from wgpu_n_body_amd import _lib
    n = int(sim.sim_params().particle_num) if n is None else n
    p = _lib.nb_fof_params()
    p.link, p.min_members = link, min_members
    cap = n // min_members if capacity is None else capacity
    labels, group_of = np.full(n, FILL, np.uint32), np.full(n, FILL, np.uint32)
    rows = np.zeros(cap + 1, _lib.FOF_GROUP_DTYPE)
    rows["label"] = FILL
    st = _lib.nb_fof_stats()
    rc = (call or _lib.lib().nb_sim_fof)(handle or sim._h, C.byref(p), labels.ctypes.data, group_of.ctypes.data,
                                         rows.ctypes.data, cap, C.byref(st))
    return SimpleNamespace(rc=rc, labels=labels, group_of=group_of, rows=rows, st=st, cap=cap,
                           bytes=labels.tobytes() + group_of.tobytes() + rows.tobytes() + bytes(st))


def _fof(sim, link, min_members=1, **kw):
    from wgpu_n_body_amd import _lib
    g = _raw(sim, link, min_members, **kw)
    assert g.rc == 0, _lib.lib().nb_last_error()
    return g


def _check(g, ref, tol=TOL):
    """Every integer equal, every sum within tol of the restatement's sum of |term|; the identities; rows beyond
    the catalogue untouched."""
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
    return float((err / (ref["scale"][:k] + 1e-300)).max()) if k else 0.0


def _state_of(nb, sim):
    return nb.as_floats(sim.read_particles()).copy()


def _prepared(nb, kind, state, step=True):
    """The simulator and the state it holds: a TreeSim after one step, in tree order."""
    sim = _sim(nb, kind, state)
    if kind == "tree" and step:
        sim.encode()
    return sim, _state_of(nb, sim)


@pytest.mark.parametrize("n", [0, 1, 2])
@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_tiny_states(gpu, kind, n):
    nb = gpu
    state = F._state(np.array([(0.1, 0.2, 0.3), (0.15, 0.2, 0.3)])[:n])
    sim = _sim(nb, kind, state)
    for link, comps in ((0.1, min(n, 1)), (0.01, n)):
        for mm in (1, 2):
            g = _fof(sim, link, mm)
            _check(g, F.fof_brute(state, link, mm))
            assert g.st.components == comps
    if n == 0:
        assert (g.st.largest_count, g.st.largest_label, tuple(g.st.cells)) == (0, F.NONE, (0, 0, 0))
    sim.destroy()


def test_no_body_counts(gpu):
    """n > 0 and every body non-finite: no cell, no component, every label NB_FOF_NONE."""
    nb, kind = gpu, "naive"
    state = F._state(np.full((300, 3), np.nan))
    state[::3, 0], state[1::3, 4], state[2::3, 9] = 0.5, np.inf, -np.inf  # (a third each: position, velocity, mass)
    sim = _sim(nb, kind, state)
    g = _fof(sim, 0.1, 1)
    _check(g, F.fof_brute(state, 0.1, 1))
    assert (g.st.nonfinite, g.st.components, g.st.groups, g.st.largest_label) == (300, 0, 0, F.NONE)
    assert np.all(g.labels == F.NONE) and np.all(g.group_of == F.NONE) and tuple(g.st.cells) == (0, 0, 0)
    sim.destroy()


CASES = F.synthetic_cases(small=False)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c[0] for c in CASES])
@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_synthetic_cases(gpu, kind, idx):
    nb = gpu
    name, state0, link, components = CASES[idx]
    # (an octree refuses to step bodies closer than root_width / 2^21: those states are grouped as they were given)
    stepped = kind == "tree" and name not in ("coincident", "far_clump", "cell_borders")
    sim, state = _prepared(nb, kind, state0, step=stepped)
    restate = F.fof_brute if state.shape[0] <= 16 else F.fof_grid
    worst = 0.0
    for mm in (1, 2, 20):
        g = _fof(sim, link, mm)
        worst = max(worst, _check(g, restate(state, link, mm)))
    if not stepped and components is not None:  # (a step moves the bodies off the construction)
        assert g.st.components == components
    h = F.cell_side(link)
    assert g.st.cell_side == h and g.st.step_num == (1 if stepped else 0)
    ok = F.body_ok(state)
    ext = state[ok, 0:3].astype(np.float64).max(axis=0) - state[ok, 0:3].astype(np.float64).min(axis=0)
    assert tuple(g.st.cells) == tuple(int(c) for c in np.floor(ext / h) + 1)
    print(f"{name}: components {g.st.components} largest {g.st.largest_count} worst error / bound {worst / TOL:.3g}")
    sim.destroy()


def _median_neighbour_distance(pos):
    p = pos.astype(np.float64)
    best = np.empty(len(p))
    for a in range(0, len(p), 1024):
        d2 = ((p[a:a + 1024, None, :] - p[None, :, :]) ** 2).sum(axis=2)
        d2[np.arange(len(d2)), np.arange(a, a + len(d2))] = np.inf
        best[a:a + 1024] = d2.min(axis=1)
    return float(np.sqrt(np.median(best)))


@pytest.mark.parametrize("bad", [False, True], ids=["finite", "nonfinite"])
@pytest.mark.parametrize("init", ["spherical", "disc"])
@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_project_inits(gpu, kind, init, bad):
    nb = gpu
    state0 = make_state(init, 8192, seed=7)
    if bad and kind == "tree":  # (a tree is not stepped over non-finite bodies: they go in after the step)
        sim, state = _prepared(nb, kind, state0)
        sim.destroy()
        state0 = state
    if bad:
        rng = np.random.default_rng(3)
        rows, cols = rng.choice(8192, 40, replace=False), rng.choice([0, 1, 2, 3, 4, 5, 9], 40)
        state0[rows, cols] = rng.choice([np.nan, np.inf, -np.inf], 40)
        sim = _sim(nb, kind, state0)
        state = _state_of(nb, sim)
    else:
        sim, state = _prepared(nb, kind, state0)
    ok = F.body_ok(state)
    link = _median_neighbour_distance(state[ok, 0:3])
    for mm in (20, 1, 2):
        g = _fof(sim, link, mm)
        _check(g, F.fof_grid(state, link, mm))
    assert g.st.nonfinite == (40 if bad else 0) and np.all(g.labels[~ok] == F.NONE) and np.all(g.group_of[~ok] == F.NONE)
    assert 1 <= g.st.groups < g.st.components < 8192 and g.st.largest_count > 2  # (of min_members = 2)
    # with min_members = 1 the catalogue's sums are the diagnostics' mass and mass * com
    g1 = _fof(sim, link, 1)
    d = sim.diagnostics()
    m = state[ok].astype(np.float64)
    assert abs(g1.rows["mass"].sum() - d.mass) <= TOL * np.abs(m[:, 9]).sum()
    for a in range(3):
        assert abs(g1.rows["mx"][:, a].sum() - d.mass * d.com[a]) <= TOL * np.abs(m[:, 9] * m[:, a]).sum()
    sim.destroy()


def test_multi_pass_sort(gpu):
    """65,536 bodies over a grid of more than 2^16 cells: three sort passes, several blocks of every scan."""
    nb = gpu
    state = make_state("uniform", 65536, seed=5)
    sim = _sim(nb, "naive", state)
    ext = state[:, 0:3].max(axis=0) - state[:, 0:3].min(axis=0)
    link = 0.7 * float((ext.prod() / 65536) ** (1.0 / 3.0))
    g = _fof(sim, link, 2)
    assert int(g.st.cells[0]) * int(g.st.cells[1]) * int(g.st.cells[2]) > 1 << 16
    _check(g, F.fof_grid(state, link, 2))
    assert 100 < g.st.groups and g.st.components < 65536
    sim.destroy()


def test_sort_chunks_beyond_the_other_suites(gpu):
    """524,289 bodies, uniform in a cube, over 200^3 cells: 1,639 sort chunks of 320 bodies, the last of one body,
    so a thread of the shared sort's scan (csrc/nb_analysis_sort.hpp) owns two chunks; three of the eight enqueued
    passes run, the rest are gated off by the plan."""
    nb = gpu
    n = 524289
    state = make_state("uniform", n, seed=5)
    sim = _sim(nb, "naive", state)
    ext = state[:, 0:3].max(axis=0) - state[:, 0:3].min(axis=0)
    link = 0.7 * float((ext.prod() / n) ** (1.0 / 3.0))
    g = _fof(sim, link, 2)
    sim.destroy()
    assert 1 << 16 < int(g.st.cells[0]) * int(g.st.cells[1]) * int(g.st.cells[2]) < 1 << 24  # three passes
    _check(g, F.fof_grid(state, link, 2))
    assert 100 < g.st.groups and g.st.components < n


def test_tuning_keys_do_not_change_a_bit(gpu):
    """One cell of 5,000 bodies beside scattered ones: the shortest chunks, and no boxes, give the default's bytes."""
    nb = gpu
    rng = np.random.default_rng(8)
    pos = np.concatenate([rng.uniform(0.0, 1e-4, (5000, 3)) + 0.25, F._ball(rng, 3000, 0.2, (0.25, 0.25, 0.25))])
    state = F._state(pos[rng.permutation(8000)], 9)
    sim = _sim(nb, "naive", state)
    link = 0.01
    base = _fof(sim, link, 2)
    _check(base, F.fof_grid(state, link, 2))
    assert base.st.largest_count >= 5000
    for key, value in (("fof_chunk_len", 64), ("fof_cell_boxes", 0), ("fof_chunk_len", 65536)):
        sim.set_tuning(key, value)
        assert _fof(sim, link, 2).bytes == base.bytes, (key, value)
    for key, value in (("fof_chunk_len", 0), ("fof_chunk_len", 100), ("fof_chunk_len", 1 << 17), ("fof_cell_boxes", 2)):
        with pytest.raises(nb.NBodyError):
            sim.set_tuning(key, value)
    sim.destroy()


@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_bitwise_reproducible(gpu, kind):
    nb = gpu
    sim, state = _prepared(nb, kind, make_state("disc", 4097, seed=2))
    link = 0.01
    g1, g2 = _fof(sim, link, 3), _fof(sim, link, 3)
    sim.diagnostics()
    _fof(sim, 0.05, 1)  # another shape between
    g3 = _fof(sim, link, 3)
    sim.destroy()
    assert g1.st.groups > 0 and g1.bytes == g2.bytes == g3.bytes


def test_a_permutation_permutes_the_partition(gpu):
    nb = gpu
    state = make_state("spherical", 4096, seed=6)
    perm = np.random.default_rng(4).permutation(4096)
    link = 0.02
    parts = []
    for s, back in ((state, np.arange(4096)), (state[perm], perm)):
        sim = _sim(nb, "naive", s)
        g = _fof(sim, link, 1)
        sim.destroy()
        parts.append({frozenset(int(back[i]) for i in grp) for grp in F.partition(g.labels)})
    assert parts[0] == parts[1] and 1 < len(parts[0]) < 4096


def test_capacity_smaller_than_the_catalogue(gpu):
    nb = gpu
    state = make_state("spherical", 4096, seed=6)
    sim = _sim(nb, "naive", state)
    link = 0.02
    full = _fof(sim, link, 2)
    ref = F.fof_grid(state, link, 2)
    assert full.st.groups > 8
    for cap in (0, 1, 7):
        g = _fof(sim, link, 2, capacity=cap)
        _check(g, ref)
        assert g.st.groups == full.st.groups and bytes(g.st) == bytes(full.st)
        assert g.rows[:cap].tobytes() == full.rows[:cap].tobytes()
    sim.destroy()


def test_null_outputs(gpu):
    nb = gpu
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    state = make_state("spherical", 2000, seed=3)
    sim = _sim(nb, "naive", state)
    full = _fof(sim, 0.03, 2)
    p = _lib.nb_fof_params()
    p.link, p.min_members = 0.03, 2
    assert L.nb_sim_fof(sim._h, C.byref(p), None, None, None, 0, None) == 0
    st = _lib.nb_fof_stats()
    assert L.nb_sim_fof(sim._h, C.byref(p), None, None, None, 0, C.byref(st)) == 0 and bytes(st) == bytes(full.st)
    lab = np.zeros(2000, np.uint32)
    assert L.nb_sim_fof(sim._h, C.byref(p), lab.ctypes.data, None, None, 0, None) == 0
    assert np.array_equal(lab, full.labels)
    gof = np.zeros(2000, np.uint32)
    assert L.nb_sim_fof(sim._h, C.byref(p), None, gof.ctypes.data, None, 0, None) == 0
    assert np.array_equal(gof, full.group_of)
    rows = np.zeros(1000, _lib.FOF_GROUP_DTYPE)
    assert L.nb_sim_fof(sim._h, C.byref(p), None, None, rows.ctypes.data, 1000, None) == 0
    assert rows[:full.st.groups].tobytes() == full.rows[:full.st.groups].tobytes()
    sim.destroy()


def test_refusals(gpu):
    nb = gpu
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    s = make_state("uniform", 64, seed=1)
    sim = _sim(nb, "naive", s)
    for link, mm in ((0.0, 1), (float("nan"), 1), (0.1, 0)):
        g = _raw(sim, link, mm, capacity=8)
        assert g.rc == _lib.NB_ERR_INVALID and L.nb_last_error()
        assert np.all(g.labels == FILL) and np.all(g.group_of == FILL) and np.all(g.rows["label"] == FILL)
    sim.destroy()
    # one far body pushes an axis past 2^21 cells: refused after the synchronisation, nothing written
    far = s.copy()
    far[17, 0] = 3.0e4
    sim = _sim(nb, "naive", far)
    g = _raw(sim, 0.01, 1)
    assert g.rc == _lib.NB_ERR_INVALID and b"cells" in L.nb_last_error()
    assert np.all(g.labels == FILL) and np.all(g.group_of == FILL) and np.all(g.rows["label"] == FILL)
    assert bytes(g.st) == bytes(_lib.nb_fof_stats())
    ok = _fof(sim, 0.1, 1)  # the simulator stays usable, and a link the grid can carry goes through
    _check(ok, F.fof_brute(far, 0.1, 1))
    fresh = _sim(nb, "naive", far)  # ... with the bytes of a simulator that never refused: the refusal left nothing
    assert _fof(fresh, 0.1, 1).bytes == ok.bytes
    fresh.destroy()
    with pytest.raises(nb.NBodyError) as ex:
        sim.fof_groups(0.01)
    assert ex.value.code == _lib.NB_ERR_INVALID
    sim.destroy()
    # a sharded simulator (rank 0 of 2)
    sharded = nb.NaiveSim.from_particles(nb.SimParams(particle_num=64), None, s, placement=nb.Placement(world=2))
    g = _raw(sharded, 0.1, 1, n=64)
    assert g.rc == _lib.NB_ERR_UNSUPPORTED and b"sharded" in L.nb_last_error()
    sharded.destroy()
    # a several-GPU runner, both ranks on device 0
    r = nb.OfflineHeadless(nb.NaiveSim, nb.SimParams(particle_num=512), None,
                           lambda p: nb.inits.uniform_init(p, seed=1), device_ids=[0, 0])
    with pytest.raises(nb.NBodyError) as ex:
        r.fof_groups(0.1)
    assert ex.value.code == _lib.NB_ERR_UNSUPPORTED
    r.destroy()


@pytest.mark.parametrize("case", ["naive", "tree", "tree_graph"])
def test_does_not_perturb_the_trajectory(gpu, case):
    nb = gpu
    n, steps = 4096, 10
    state = make_state("uniform", n, seed=9)
    finals = []
    for with_fof in (False, True):
        sim = _sim(nb, "naive" if case == "naive" else "tree", state)
        if case == "tree_graph":
            sim.set_tuning("tree_use_graph", 1)
        for k in range(steps):
            sim.encode()
            if with_fof:
                fg = sim.fof_groups(0.03 if k % 2 else 0.06, min_members=2, labels=k % 3 == 0)
                assert fg.stats.step_num == k + 1 and fg.stats.n == n and fg.stats.groups > 0
        finals.append(nb.as_floats(sim.read_particles()).copy())
        sim.destroy()
    assert np.array_equal(finals[0].view(np.uint32), finals[1].view(np.uint32))


def test_python_wrapper(gpu):
    nb = gpu
    state = make_state("disc", 4096, seed=0)
    sim = _sim(nb, "naive", state)
    link = 0.02
    default = sim.fof_groups(link)
    assert default.min_members == 20 and default.stats.groups == F.fof_grid(state, link, 20)["groups"]
    fg = sim.fof_groups(link, min_members=5)
    g = _fof(sim, link, 5)
    ref = F.fof_grid(state, link, 5)
    assert fg.stats.groups == ref["groups"] >= 3 and fg.rows.shape == (ref["groups"],)
    assert np.array_equal(fg.labels, g.labels) and np.array_equal(fg.group_of, g.group_of)
    assert fg.rows.tobytes() == g.rows[:ref["groups"]].tobytes()
    assert np.array_equal(fg.count, ref["rows_count"]) and np.array_equal(fg.label, ref["rows_label"])
    order = fg.by_size()
    assert sorted(order) == list(range(ref["groups"]))
    assert all((fg.count[a], -int(fg.label[a])) >= (fg.count[b], -int(fg.label[b])) for a, b in zip(order, order[1:]))
    assert fg.count[order[0]] == fg.stats.largest_count and fg.label[order[0]] == fg.stats.largest_label
    s = state.astype(np.float64)
    for r in order[:3]:
        mem = fg.group_of == r
        m = s[mem, 9]
        com = (m[:, None] * s[mem, 0:3]).sum(axis=0) / m.sum()
        vel = (m[:, None] * s[mem, 3:6]).sum(axis=0) / m.sum()
        assert np.allclose(fg.com[r], com, rtol=0, atol=1e-9) and np.allclose(fg.velocity[r], vel, rtol=0, atol=1e-9)
        rms = np.sqrt((m * ((s[mem, 0:3] - com) ** 2).sum(axis=1)).sum() / m.sum())
        sig = np.sqrt((m * ((s[mem, 3:6] - vel) ** 2).sum(axis=1)).sum() / m.sum())
        assert abs(fg.rms_radius[r] - rms) <= 1e-6 * max(rms, 1e-3) and abs(fg.sigma[r] - sig) <= 1e-6 * max(sig, 1e-3)
    assert sim.fof_groups(link, labels=False).labels is None
    sim.destroy()


def test_runner_and_cli(gpu):
    """nb_runner_fof equals nb_sim_fof on nb_runner_sim, and headless --fof (the C++ mirror over nb_runner_fof)
    prints what the Python runner returns."""
    nb = gpu
    from wgpu_n_body_amd import _lib
    cli = os.path.join(ROOT, "wgpu_n_body_amd", "headless")
    base = [cli, "--sim", "tree", "--n", "4096", "--init", "disc", "--steps", "4"]
    link = 0.02
    p = subprocess.run(base + ["--fof", "2", "--fof-link", repr(link), "--fof-min", "5", "--fof-top", "3"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    plain = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "fof" not in plain.stdout
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("fof ")]
    tops = [ln for ln in p.stdout.splitlines() if ln.startswith("fof_group ")]
    assert len(lines) == 3
    blank = lambda text: [re.sub(r"\d+", "#", ln) for ln in text.splitlines() if not ln.startswith("fof")]  # noqa: E731
    assert blank(p.stdout) == blank(plain.stdout)
    assert len([ln for ln in p.stdout.splitlines() if ln.startswith("Step Duration: ")]) == 4

    runner = nb.OfflineHeadless(nb.TreeSim, nb.SimParams(particle_num=4096), nb.AddParams.TreeSimParams(0.75),
                                lambda sp: nb.inits.disc_init(sp, seed=0))
    ours = [runner.fof_groups(link, min_members=5)]
    for k in range(4):
        runner.step()
        if (k + 1) % 2 == 0:
            ours.append(runner.fof_groups(link, min_members=5))
    via_runner = _raw(None, link, 5, call=_lib.lib().nb_runner_fof, handle=runner._h, n=4096)
    via_sim = _raw(runner.sim, link, 5)
    state = _state_of(nb, runner.sim)
    runner.destroy()
    assert via_runner.rc == via_sim.rc == 0 and via_runner.bytes == via_sim.bytes
    _check(via_sim, F.fof_grid(state, link, 5))
    assert np.array_equal(via_sim.labels, ours[-1].labels)

    o = ours[0]  # the same seeded init, no step yet: the line is the Python call
    assert [int(x) for x in lines[0].split()[1:]] == [0, o.stats.groups, o.stats.grouped_bodies, o.stats.largest_count]
    assert o.stats.groups >= 3
    first = [ln.split() for ln in tops[:3]]
    for ln, r in zip(first, o.by_size()[:3]):
        assert [int(x) for x in ln[1:5]] == [0, int(r), int(o.label[r]), int(o.count[r])]
        assert float(ln[5]) == pytest.approx(o.mass[r], rel=1e-5)
    for j, ln in enumerate(lines):  # (the trajectory of two runs of the tree is not specified bit for bit)
        assert int(ln.split()[1]) == 2 * j == ours[j].stats.step_num
