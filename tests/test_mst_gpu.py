"""nb_mst_sim on the device (csrc/nb_mst.hip) against the numpy restatements of its rule (tests/mst_ref.py) on the
read-back state: every edge, d2, degree and stat equal, `rounds` and `components_after` included; two calls the same
bytes; every combination of the tuning keys' extreme values the same bytes; cut(link) against nb_sim_fof of the same
simulator at the same step, byte for byte; the null outputs and refusals; that a call does not perturb the
trajectory; the runner, the C++ mirror and the CLI.  Nothing here has a tolerance.  `-m gpu`."""
import ctypes as C
import itertools
import math
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from tests import knn_ref as K
from tests import mst_ref as M
from tests.helpers import ROOT, make_state

pytestmark = pytest.mark.gpu

FILL = 0xDEADBEEF
CASES = M.gpu_cases()
IDS = [c[0] for c in CASES]
REFS = {}


def _reference(state):
    """The restatement of a state, made once and left unchanged."""
    key = state.tobytes()
    if key not in REFS:
        REFS[key] = M.reference(state)
    return REFS[key]


def _sim(nb, kind, state, theta=0.75):
    sp = nb.SimParams(particle_num=state.shape[0])
    if kind == "naive":
        return nb.NaiveSim.from_particles(sp, None, state)
    return nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(theta), state)


def _state_of(nb, sim):
    return nb.as_floats(sim.read_particles()).copy()


def _prepared(nb, kind, state, step=True):
    """The simulator and the state it holds: a TreeSim after one step, in tree order."""
    sim = _sim(nb, "naive" if kind == "naive" else "tree", state)
    if kind == "tree_graph":
        sim.set_tuning("tree_use_graph", 1)
    if kind != "naive" and step and state.shape[0] > 0:
        sim.encode()
    return sim, _state_of(nb, sim)


def _raw(sim, call=None, handle=None, n=None, flags=0):
    """The C call with every buffer pre-filled."""
    from wgpu_n_body_amd import _lib
    n = int(sim.sim_params().particle_num) if n is None else n
    p = _lib.nb_mst_params()
    p.flags = flags
    lo, hi, deg = (np.full(n + 1, FILL, np.uint32) for _ in range(3))
    d2 = np.full(n + 1, -7.0)
    st = _lib.nb_mst_stats()
    rc = (call or _lib.lib().nb_mst_sim)(handle or sim._h, C.byref(p), lo.ctypes.data, hi.ctypes.data, d2.ctypes.data,
                                         deg.ctypes.data, C.byref(st))
    m = int(st.edges)
    return SimpleNamespace(rc=rc, n=n, m=m, lo=lo[:m], hi=hi[:m], d2=d2[:m], degree=deg[:n], st=st,
                           rest=(lo[m:], hi[m:], d2[m:], deg[n:]),
                           bytes=lo.tobytes() + hi.tobytes() + d2.tobytes() + deg.tobytes() + bytes(st))


def _rest_untouched(g):
    return np.all(g.rest[0] == FILL) and np.all(g.rest[1] == FILL) and np.all(g.rest[2] == -7.0) and np.all(
        g.rest[3] == FILL)


def _mst(sim, **kw):
    from wgpu_n_body_amd import _lib
    g = _raw(sim, **kw)
    assert g.rc == 0, _lib.lib().nb_last_error()
    assert _rest_untouched(g)  # the first `edges` entries and n degrees, no more
    return g


def _check(g, ref):
    """Every integer and the bytes of every double equal."""
    st = g.st
    assert (st.n, st.nonfinite, st.edges) == (ref.n, ref.nonfinite, ref.edges)
    assert st.edges == max(st.n - st.nonfinite, 1) - 1
    print("rounds", st.rounds, "components_after", list(st.components_after[:st.rounds]), "reference", ref.rounds,
          ref.components_after[:ref.rounds].tolist())
    assert np.array_equal(g.lo, ref.lo), np.flatnonzero(g.lo != ref.lo)[:8]
    assert np.array_equal(g.hi, ref.hi), np.flatnonzero(g.hi != ref.hi)[:8]
    assert g.d2.tobytes() == ref.d2.tobytes()
    assert np.array_equal(g.degree, ref.degree)
    assert st.rounds == ref.rounds and list(st.components_after) == ref.components_after.tolist()
    for a, b in ((st.d2_min, ref.d2_min), (st.d2_max, ref.d2_max), (st.h, ref.h)):
        assert np.float64(a).tobytes() == np.float64(b).tobytes(), (a, b)
    assert np.array(st.lo[:]).tobytes() == ref.plan_lo.tobytes() and np.array(st.hi[:]).tobytes() == ref.plan_hi.tobytes()
    assert st.reserved == 0


def _kinds(name):
    return ("naive",) if name == "sample16385" else ("naive", "tree")


@pytest.mark.parametrize("name,kind", [(n, k) for n in IDS for k in _kinds(n)])
def test_cases(gpu, name, kind):
    """The tree, the degrees and every stat against the restatement; two calls the same bytes."""
    nb = gpu
    _, state0, steppable = CASES[IDS.index(name)]
    sim, state = _prepared(nb, kind, state0, step=steppable)
    g = _mst(sim)
    again = _mst(sim)
    sim.destroy()
    _check(g, _reference(state))
    assert g.bytes == again.bytes
    if name == "piles16x64":
        assert np.count_nonzero(g.d2 == 0.0) == 16 * 63 and g.st.components_after[0] == 16
    if name == "sample16385":
        assert g.st.rounds >= 6


@pytest.mark.parametrize("name", IDS)
def test_tuning_keys_do_not_change_a_bit(gpu, name):
    """Every combination of the four keys' extreme values."""
    nb = gpu
    _, state0, _ = CASES[IDS.index(name)]
    sim, state = _prepared(nb, "naive", state0)
    want = _mst(sim)
    _check(want, _reference(state))  # (the restatement test_cases made of the same state)
    for span, per, skip, shared in itertools.product((1, 8), (1, 4), (0, 1), (0, 1)):
        for key, value in (("mst_span_cells", span), ("mst_block_queries", per), ("mst_skip_runs", skip),
                           ("mst_shared_bound", shared)):
            sim.set_tuning(key, value)
        assert _mst(sim).bytes == want.bytes, (span, per, skip, shared)
    for key, value in (("mst_span_cells", 0), ("mst_span_cells", 9), ("mst_block_queries", 3), ("mst_skip_runs", 2),
                       ("mst_shared_bound", -1)):
        with pytest.raises(nb.NBodyError):
            sim.set_tuning(key, value)
    sim.destroy()


def _fof_links(tree, state):
    """Five links: lengths of the tree's own edges, one of them rounded down and one up, none so small that
    nb_sim_fof's grid refuses it."""
    ok = K.counted_mask(*K.split(state))
    x = state[ok, 0:3].astype(np.float64)
    floor = float((x.max(axis=0) - x.min(axis=0)).max()) * 2.0 ** -19 if ok.any() else 0.0
    ln = np.unique(tree.length[tree.length > floor])
    if ln.size == 0:
        return [max(floor, 1e-3) * s for s in (1.0, 1.5, 2.0, 3.0, 5.0)]
    q = [float(ln[int(f * (ln.size - 1))]) for f in (0.0, 0.25, 0.5, 0.75, 1.0)]
    return [q[0], float(np.nextafter(q[1], 0.0)), q[2], float(np.nextafter(q[3], math.inf)), q[4]]


@pytest.mark.parametrize("kind", ["naive", "tree", "tree_graph"])
@pytest.mark.parametrize("name", IDS)
def test_cut_is_fof_of_the_same_simulator(gpu, name, kind):
    """cut(link) equals fof_groups(link, min_members=1).labels of the same simulator at the same step, byte for
    byte; group_counts is the catalogue's size."""
    nb = gpu
    _, state0, steppable = CASES[IDS.index(name)]
    sim, state = _prepared(nb, kind, state0, step=steppable)
    tree = sim.spanning_tree()
    for link in _fof_links(tree, state):
        f = sim.fof_groups(link, min_members=1)
        assert f.stats.step_num == tree.stats.step_num
        got = tree.cut(link)
        assert got.tobytes() == f.labels.tobytes(), (name, kind, link)
        assert tree.group_counts([link])[0] == f.stats.groups
        assert tree.group_counts([link], 5)[0] == np.count_nonzero(f.rows["count"] >= 5)
    sim.destroy()


@pytest.mark.parametrize("case", ["naive", "tree", "tree_graph"])
def test_does_not_perturb_the_trajectory(gpu, case):
    nb = gpu
    n, steps = 4096, 8
    state = make_state("uniform", n, seed=9)
    finals = []
    for with_mst in (False, True):
        sim = _sim(nb, "naive" if case == "naive" else "tree", state)
        if case == "tree_graph":
            sim.set_tuning("tree_use_graph", 1)
        for j in range(steps):
            sim.encode()
            if with_mst:
                t = sim.spanning_tree(degree=j % 2 == 0)
                assert t.stats.step_num == j + 1 and t.stats.edges == n - 1 and (t.degree is None) == (j % 2 == 1)
        finals.append(nb.as_floats(sim.read_particles()).copy())
        sim.destroy()
    assert np.array_equal(finals[0].view(np.uint32), finals[1].view(np.uint32))


def test_null_outputs_and_refusals(gpu):
    nb = gpu
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    n = 2000
    sim = _sim(nb, "naive", make_state("spherical", n, seed=3))
    full = _mst(sim)
    p = _lib.nb_mst_params()
    assert L.nb_mst_sim(sim._h, C.byref(p), None, None, None, None, None) == 0
    st = _lib.nb_mst_stats()
    assert L.nb_mst_sim(sim._h, C.byref(p), None, None, None, None, C.byref(st)) == 0 and bytes(st) == bytes(full.st)
    for which in range(4):
        bufs = [np.full(n + 1, FILL, np.uint32), np.full(n + 1, FILL, np.uint32), np.full(n + 1, -7.0),
                np.full(n + 1, FILL, np.uint32)]
        args = [b.ctypes.data if j == which else None for j, b in enumerate(bufs)]
        assert L.nb_mst_sim(sim._h, C.byref(p), *args, None) == 0
        want = (full.lo, full.hi, full.d2, full.degree)[which]
        assert np.array_equal(bufs[which][:len(want)], want) and np.all(bufs[which][len(want):] == (-7.0, FILL)[which != 2])
    for field in ("flags", "reserved32", "reserved"):  # refused calls write nothing
        q = _lib.nb_mst_params()
        setattr(q, field, 2)
        lo = np.full(n, FILL, np.uint32)
        st = _lib.nb_mst_stats()
        assert L.nb_mst_sim(sim._h, C.byref(q), lo.ctypes.data, None, None, None, C.byref(st)) == _lib.NB_ERR_INVALID
        assert np.all(lo == FILL) and bytes(st) == bytes(_lib.nb_mst_stats())
    assert _mst(sim).bytes == full.bytes  # the simulator stays usable
    t = sim.spanning_tree()
    assert np.array_equal(t.edges, np.stack((full.lo, full.hi), axis=1)) and t.d2.tobytes() == full.d2.tobytes()
    assert np.array_equal(t.degree, full.degree) and t.stats.rounds == full.st.rounds
    assert t.total_length == float(np.cumsum(np.sqrt(full.d2))[-1]) and t.longest()[:2] == (full.lo[-1], full.hi[-1])
    assert sim.spanning_tree(degree=False).degree is None
    sim.destroy()
    # a sharded simulator (rank 0 of 2)
    s = make_state("uniform", 64, seed=1)
    sharded = nb.NaiveSim.from_particles(nb.SimParams(particle_num=64), None, s, placement=nb.Placement(world=2))
    g = _raw(sharded, n=64)
    assert g.rc == _lib.NB_ERR_UNSUPPORTED and b"sharded" in L.nb_last_error()
    assert g.m == 0 and _rest_untouched(g) and bytes(g.st) == bytes(_lib.nb_mst_stats())
    sharded.destroy()
    # a several-GPU runner, both ranks on device 0
    r = nb.OfflineHeadless(nb.NaiveSim, nb.SimParams(particle_num=512), None,
                           lambda sp: nb.inits.uniform_init(sp, seed=1), device_ids=[0, 0])
    with pytest.raises(nb.NBodyError) as ex:
        r.spanning_tree()
    assert ex.value.code == _lib.NB_ERR_UNSUPPORTED
    r.destroy()


def test_the_tree_feeds_the_group_passes(gpu):
    """cut(link) is an assignment shapes_of / radii_of (with as many rows as bodies: a label is a body index) and
    phase_map(values=...) accept."""
    nb = gpu
    n = 2048
    sim = _sim(nb, "naive", make_state("spherical", n, seed=2))
    tree = sim.spanning_tree()
    ratio, link = tree.largest_gap()
    assert ratio > 1.0 and link > 0.0
    link = float(np.median(tree.length))
    labels = tree.cut(link)
    assert labels.tobytes() == sim.fof_groups(link, min_members=1).labels.tobytes()
    sizes = np.bincount(labels, minlength=n)
    big = int(np.argmax(sizes))
    assert sizes[big] >= 10
    step = tree.stats.step_num
    assert sim.shapes_of(labels, n, step_num=step).rows["count"][big] == sizes[big]
    assert sim.radii_of(labels, n, step_num=step).rows["count"][big] == sizes[big]
    pm = sim.phase_map("value", "r", x_edges=[-np.inf, big - 0.5, big + 0.5, np.inf], y_edges=[-np.inf, np.inf],
                       values=labels.astype(np.float64))
    assert pm.counts.shape == (1, 3) and pm.counts[0, 1] == sizes[big] and pm.counts.sum() == n
    with pytest.raises(ValueError):  # without the degrees cut cannot tell which bodies are not counted
        bad = K.inject_nonfinite(make_state("uniform", 256, seed=3).copy(), 5, 1)
        other = _sim(nb, "naive", bad)
        try:
            other.spanning_tree(degree=False).cut(1.0)
        finally:
            other.destroy()
    sim.destroy()


def test_runner_and_cli(gpu, tmp_path):
    """nb_mst_runner equals nb_mst_sim on nb_runner_sim, and headless --mst (the C++ mirror over nb_mst_runner) prints
    and dumps what the Python runner returns."""
    nb = gpu
    from wgpu_n_body_amd import _lib
    cli = os.path.join(ROOT, "wgpu_n_body_amd", "headless")
    base = [cli, "--sim", "tree", "--n", "4096", "--init", "disc", "--steps", "4"]
    p = subprocess.run(base + ["--mst", "2", "--mst-links", "0.01,0.05", "--mst-min", "3", "--mst-dump", str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("mst ")]
    assert len(lines) == 3 and all(len(ln) == 8 for ln in lines)
    assert len([ln for ln in p.stdout.splitlines() if ln.startswith("Step Duration: ")]) == 4

    runner = nb.OfflineHeadless(nb.TreeSim, nb.SimParams(particle_num=4096), nb.AddParams.TreeSimParams(0.75),
                                lambda sp: nb.inits.disc_init(sp, seed=0))
    o = runner.spanning_tree()  # the same seeded init, no step yet: the line is the Python call
    for _ in range(2):
        runner.step()
    via_runner = _raw(None, call=_lib.lib().nb_mst_runner, handle=runner._h, n=4096)
    via_sim = _raw(runner.sim)
    state = _state_of(nb, runner.sim)
    runner.destroy()
    assert via_runner.rc == via_sim.rc == 0 and via_runner.bytes == via_sim.bytes
    _check(via_sim, _reference(state))

    ln = lines[0]  # mst step edges rounds total longest count(link 1) count(link 2)
    assert [int(x) for x in ln[1:4]] == [0, o.stats.edges, o.stats.rounds]
    assert float(ln[4]) == o.total_length and float(ln[5]) == o.longest()[2]  # (%.17g round-trips)
    assert [int(x) for x in ln[6:8]] == o.group_counts([0.01, 0.05], 3).tolist()
    for j, ln in enumerate(lines):  # (the trajectory of two runs of the tree is not specified bit for bit)
        assert int(ln[1]) == 2 * j and int(ln[2]) == 4095
    dump = np.load(os.path.join(tmp_path, "mst_0.npy"))
    assert dump.dtype == np.float64 and dump.shape == (4095, 3)
    assert np.array_equal(dump[:, 0:2], o.edges.astype(np.float64)) and dump[:, 2].tobytes() == o.d2.tobytes()
    for bad in (["--mst-links", "0.01"], ["--mst-min", "2"], ["--mst", "2", "--mst-links", "0,1"],
                ["--mst", "2", "--mst-links", "0.01,"], ["--mst", "2", "--mst-min", "0"],
                ["--mst", "2", "--mst-min", "abc"]):
        q = subprocess.run(base + bad, capture_output=True, text=True, timeout=300)
        assert q.returncode != 0, bad
