"""The multi-domain Barnes-Hut step (locally essential trees) against binary64, on a real MI355X -- `-m gpu`.

tests/test_let_gpu.py pins the LET path against itself bit for bit (pruning, fixed stride, one-launch export, own tree
first, native runner) and against all-pairs statistically.  Here ONE step of every rank is held per node and per body
to tests/let_ref.py -- tree_ref.walk64 of every rank's tree for every rank's bodies, added in binary64 -- whose own
standing tests/test_let_ref.py establishes on the CPU.  For every case of let_ref.CASES, on every rank:
  1. status words clear; every body comes back exactly once;
  2. read_tree's root_width is the same float on all ranks: 2 x max(1, max |coord| over ALL bodies);
  3. topology: where every rank spans the global cube, bodies / children / body order are the oracle's tree of that
     rank's bodies alone, bit for bit; elsewhere (wide-7.5) tree_shape's invariants, each body in one leaf;
  4. moments: tree_ref.check_moments per node; leaves bit-exact; a massless cell has mass 0 and a NaN cog;
  5. forces: let_walk64 over the trees read back; an unflagged body within K_LET units of 2^-24 x sum |term| (derived in
     let_ref.py on the CPU, not from the GPU's output), a flagged one within rel < 5e-2;
  6. visits and accepts summed over the ranks equal let_walk64's where no body is flagged (else within max(2, 1e-5 x));
  7. v' == kick(kick(v, a_old, dt), a'_gpu, dt), mass and position bit for bit; everything finite.
Bodies are identified by each rank's `order` buffer (three cases edit the masses, so tags are not available); check 7
confirms the identification bit for bit through the drifted positions.

Default variant, worst / median unflagged body in units of K_LET = 96 (MI355X):
    uniform-3x4         1.69 / 1.15      uniform-65x8        2.49 / 0.73
    uniform-4099x2      2.16 / 0.38      uniform-4099x3      2.59 / 0.39
    uniform-4099x8      2.93 / 0.39      sphericalx4         2.30 / 0.40
    discx3              6.37 / 1.28      dense-corex4        4.22 / 0.63
    wide-7.5x3          4.58 / 0.46      small-0.01x2        2.21 / 0.64
    log-massx4          5.28 / 0.53      tracersx3           3.14 / 0.50
    massless-pocketx4   2.74 / 0.45      after a migration   2.63 / 0.42
(the other walk shapes: up to 8.25 units on uniform-4099x3 and 19.03 on discx3, one body per lane; all counts exact)
"""
import functools

import numpy as np
import pytest

from tests import let_ref as L
from tests import tree_ref as T
from tests.helpers import E, bits
from tests.test_let_gpu import LetGroup, moving
from tests.test_tree_gpu import WALK_SHAPES, rel_err

pytestmark = pytest.mark.gpu


def read_ranks(nb, grp, srcs, before=None):
    """Per rank of a LetGroup after a step: dict(src -- the rank's source rows --, dst, order, tree, root_width,
    counters (visits, accepts; less `before`), status)."""
    out = []
    for r, sim in enumerate(grp.sims):
        sim.wait()
        dst = nb.as_floats(sim.dest_particle_slice()).copy()
        tree, rw = sim.read_tree()
        c = sim.debug_buffer("counters", np.uint64)
        c0 = before[r] if before is not None else (0, 0)
        out.append(dict(src=srcs[r], dst=dst, tree=tree, root_width=np.float32(rw),
                        order=sim.debug_buffer("order", np.uint32).astype(np.int64),
                        counters=(int(c[0]) - c0[0], int(c[1]) - c0[1]),
                        status=sim.debug_buffer("status", np.uint32)))
    return out


def run_case(nb, name, tuning=None, **group_kw):
    """One LET step of a case from its source state -> (per-rank results, the group's export counts)."""
    case = L.CASES[L.CASE_IDS.index(name)]
    _name, _kind, n, _seed, theta, g, dt = L.base_case(case)
    s = T.case_state(L.base_case(case))
    sp = nb.SimParams(particle_num=n, g=g, e=E, dt=dt)
    grp = LetGroup(nb, sp, nb.as_particles(s), case[2], theta, **group_kw)
    for sim in grp.sims:
        sim.set_tuning("tree_count_visits", 1)
        for key, value in (tuning or {}).items():
            sim.set_tuning(key, value)
    grp.step()
    runs = read_ranks(nb, grp, [s[idx] for idx in L.domains(s, case[2])])
    counts = grp.counts
    grp.destroy()
    return runs, counts


def spans_global_cube(run, rw):
    return np.float32(2.0) * max(np.float32(1.0), np.abs(run["src"][:, 0:3]).max()) == rw


def check_build(O, runs, params):
    """Checks 1 to 4 on every rank; returns the global root width."""
    theta, g, dt = params
    everybody = np.concatenate([run["src"] for run in runs])
    rw = L.global_root_width(everybody)
    for r, run in enumerate(runs):
        src, tree, n = run["src"], run["tree"], len(run["src"])
        # 1. status, and the rank's bodies once each
        assert not run["status"].any(), (r, run["status"])
        assert len(run["dst"]) == n and np.array_equal(np.sort(run["order"]), np.arange(n)), r
        # 2. the global root
        assert run["root_width"] == rw, (r, run["root_width"], rw)
        if n == 0:
            assert len(tree) == 0
            continue
        # 3. topology
        parent, depth, leaf = T.tree_shape(tree)
        named = tree["children"][leaf, 0].astype(np.int64)
        assert np.array_equal(np.sort(named), np.arange(n)), r
        assert tree["bodies"][0] == n
        if spans_global_cube(run, rw):     # the oracle's cube of this rank's bodies alone is the global one
            want = O.tree_step_f32(src, g, E, dt, theta, flags=O.INTENDED)
            assert np.float32(want["root_width"]) == rw and len(tree) == len(want["tree"]), r
            assert np.array_equal(tree["bodies"], want["tree"]["bodies"]), r
            assert np.array_equal(tree["children"], want["tree"]["children"]), r
            assert np.array_equal(run["order"], want["order"]), r
        else:
            assert np.array_equal(run["order"], O.tree_dfs_order(tree, n)), r
            assert np.array_equal(T.sum_up(tree, np.ones(n), (parent, depth, leaf))[~leaf], tree["bodies"][~leaf]), r
        # 4. moments; leaves bit for bit
        assert np.array_equal(bits(tree["cog"][leaf]), bits(src[named, 0:3])), r
        assert np.array_equal(bits(tree["mass"][leaf]), bits(src[named, 9])), r
        T.check_moments(tree, src)
    return rw


def check_forces(label, runs, params, w=None, rows=None):
    """Checks 5 to 7; returns let_walk64 (computed from the runs' trees unless given).  rows: other post-step rows to
    hold against the runs' trees and orders (the native runner's)."""
    theta, g, dt = params
    got = rows if rows is not None else [run["dst"] for run in runs]
    if w is None:
        ranks = [dict(x_new=run["dst"][:, 0:3], order=run["order"]) for run in runs]
        # (a rank without bodies reports the initial root_width, 2.0: never above the global one)
        w = L.let_walk64([run["tree"] for run in runs], max(run["root_width"] for run in runs), ranks, theta, g, E, dt)
    units, flagged, rel = [], [], []
    for r, run in enumerate(runs):
        src = run["src"][run["order"]]          # the source rows in sorted order
        d = got[r]
        assert np.isfinite(d).all() and np.isfinite(w[r]["acc"]).all(), (label, r)
        units.append(T.force_units(d[:, 6:9], w[r]))
        flagged.append(w[r]["flagged"])
        rel.append(rel_err(d[:, 6:9], w[r]["acc"]))
        # 7. velocity from the GPU's own new acceleration, mass, position: bit for bit
        v_new = T.kick32(T.kick32(src[:, 3:6], src[:, 6:9], dt), d[:, 6:9], dt)
        assert np.array_equal(bits(d[:, 3:6]), bits(v_new)), (label, r)
        assert np.array_equal(bits(d[:, 9]), bits(src[:, 9])), (label, r)
        assert np.array_equal(bits(d[:, 0:3]), bits(L.drift32(src, dt))), (label, r)
    units, flagged, rel = np.concatenate(units), np.concatenate(flagged), np.concatenate(rel)
    visits, accepts = sum(run["counters"][0] for run in runs), sum(run["counters"][1] for run in runs)
    want_visits, want_accepts = L.totals(w)
    worst = float(units[~flagged].max()) if (~flagged).any() else 0.0
    print(f"{label}: worst body {worst:.2f} units of K_LET = {L.K_LET}, median {np.median(units):.2f}; "
          f"{int(flagged.sum())} flagged (worst rel {rel[flagged].max() if flagged.any() else 0.0:.1e}); "
          f"visits {visits} / {want_visits}, accepts {accepts} / {want_accepts}")
    # 5. forces
    assert worst <= L.K_LET, (label, int(np.argmax(np.where(flagged, 0.0, units))), worst)
    assert (rel[flagged] < 5e-2).all(), (label, rel[flagged].max())
    # 6. counters
    if rows is None:
        if not flagged.any():
            assert (visits, accepts) == (want_visits, want_accepts), label
        else:
            assert abs(visits - want_visits) <= max(2, 1e-5 * want_visits), label
            assert abs(accepts - want_accepts) <= max(2, 1e-5 * want_accepts), label
    return w


def case_params(name):
    _name, _kind, _n, _seed, theta, g, dt = L.base_case(L.CASES[L.CASE_IDS.index(name)])
    return theta, g, dt


@functools.lru_cache(maxsize=None)
def default_run(nb, name):
    """(runs, export counts, let_walk64) of a case's default step, checked; computed once, shared by the variants."""
    from oracle import oracle as O
    O.build()
    runs, counts = run_case(nb, name)
    params = case_params(name)
    rw = check_build(O, runs, params)
    assert all(spans_global_cube(run, rw) for run in runs if len(run["src"])) == (name in L.UNIT_CUBE)
    w = check_forces(name, runs, params)
    return runs, counts, w


def same_bytes(runs, first):
    return all(a["dst"].tobytes() == b["dst"].tobytes() and a["tree"].tobytes() == b["tree"].tobytes()
               and np.array_equal(a["order"], b["order"]) for a, b in zip(runs, first))


@pytest.mark.parametrize("name", L.CASE_IDS)
def test_every_rank_against_binary64(gpu, name):
    runs, _counts, w = default_run(gpu, name)
    world = len(runs)
    sizes = [len(run["src"]) for run in runs]
    if name == "uniform-3x4":
        assert 0 in sizes and 1 in sizes
    if name == "wide-7.5x3":       # a rank whose own cube would have been smaller than the global one
        assert min(np.abs(run["src"][:, 0:3]).max() for run in runs) * np.float32(2.0) < runs[0]["root_width"]
    if name == "massless-pocketx4":
        cells = [int(((run["tree"]["mass"] == 0.0) & (run["tree"]["bodies"] > 1)).sum()) for run in runs]
        assert sum(cells) >= 1 and world > 1, cells
    if L.CASES[L.CASE_IDS.index(name)][1] in T.MASSLESS:      # the massless bodies are accelerated like any other
        for run, ref in zip(runs, w):
            massless = run["src"][run["order"], 9] == 0.0
            assert (np.linalg.norm(ref["acc"][massless], axis=1) > 0.0).all()
            assert (np.linalg.norm(run["dst"][massless, 6:9], axis=1) > 0.0).all()


@pytest.mark.parametrize("name", ["uniform-4099x3", "dense-corex4", "massless-pocketx4"])
def test_export_and_hand_over_variants_give_the_default_runs_bytes(gpu, name):
    """Whole trees instead of LETs, the level-by-level export, the own tree walked first, and fixed-stride imports:
    the bodies, trees and orders of the default step, byte for byte -- and so its standing against let_walk64."""
    first, counts, _w = default_run(gpu, name)
    need = int(counts.max())
    for variant in (dict(prune=False), dict(export_mode=0), dict(own_first=True),
                    dict(fixed_stride=need + need // 4 + 64)):
        runs, _c = run_case(gpu, name, **variant)
        assert not any(run["status"].any() for run in runs), variant
        assert same_bytes(runs, first), variant
        # the counting rule: pruned, whole-tree and two-phase walks visit and accept the same
        assert [run["counters"] for run in runs] == [run["counters"] for run in first], variant


@pytest.mark.parametrize("name", ["uniform-4099x3", "discx3"])
def test_every_walk_shape_against_binary64(gpu, name):
    """The summation order changes with the walk's shape: checks 5 to 7 again for each, on the same trees."""
    first, _counts, w = default_run(gpu, name)
    for shape in WALK_SHAPES:
        runs, _c = run_case(gpu, name, tuning=shape)
        assert not any(run["status"].any() for run in runs), shape
        assert all(a["tree"].tobytes() == b["tree"].tobytes() and np.array_equal(a["order"], b["order"])
                   and a["root_width"] == b["root_width"] for a, b in zip(runs, first)), shape
        check_forces(f"{name} {shape}", runs, case_params(name), w=w)


def test_the_step_after_a_migration(gpu, oracle):
    """a_old is non-zero, arrivals sit behind the residents, and the bound words come from a previous walk."""
    nb = gpu
    n, world, theta = 3000, 4, 0.5
    sp, p = moving(nb, n, 31, 1.5)
    grp = LetGroup(nb, sp, p, world, theta)
    for sim in grp.sims:
        sim.set_tuning("tree_count_visits", 1)
    grp.step()
    counts = grp.migrate()
    assert counts.sum() == n and (counts.sum() - np.trace(counts)) > 0          # some bodies did change owner
    srcs, before = [], []
    for r, sim in enumerate(grp.sims):
        sim.wait()
        srcs.append(nb.as_floats(sim.dest_particle_slice()).copy())
        assert len(srcs[r]) == counts[:, r].sum()                               # the active count: stayers + arrivals
        c = sim.debug_buffer("counters", np.uint64)
        before.append((int(c[0]), int(c[1])))
    everybody = np.concatenate(srcs)
    assert np.array_equal(np.sort(everybody[:, 9]), np.sort(nb.as_floats(p)[:, 9]))   # nobody lost (tagged masses)
    assert np.abs(everybody[:, 6:9]).max() > 0.0
    grp.step()
    runs = read_ranks(nb, grp, srcs, before)
    grp.destroy()
    params = (theta, sp.g, sp.dt)
    check_build(oracle, runs, params)
    check_forces("after a migration", runs, params)


def test_the_native_runner_against_binary64(gpu):
    """nb_runner_create_multi_let, 3 ranks on one device, one step: the LetGroup run's bytes, and checks 5 and 7
    directly against let_walk64 of the trees that run read back."""
    nb = gpu
    name = "uniform-4099x3"
    runs, _counts, w = default_run(nb, name)
    case = L.CASES[L.CASE_IDS.index(name)]
    _name, _kind, n, _seed, theta, g, dt = L.base_case(case)
    p = nb.as_particles(T.case_state(L.base_case(case)))
    native = nb.OfflineHeadless(nb.TreeSim, nb.SimParams(particle_num=n, g=g, e=E, dt=dt),
                                nb.AddParams.TreeSimParams(theta), lambda _p: p, device_ids=[0] * case[2],
                                let_migrate_every=0)
    native.step()
    got = nb.as_floats(native.read_particles()).copy()
    native.destroy()
    assert got.tobytes() == np.concatenate([run["dst"] for run in runs]).tobytes()
    cuts = np.cumsum([0] + [len(run["dst"]) for run in runs])
    check_forces("native runner", runs, (theta, g, dt), w=w, rows=[got[cuts[r]:cuts[r + 1]] for r in range(len(runs))])
