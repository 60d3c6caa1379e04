"""nb_sim_bound on the device (csrc/nb_bound.hip) against the numpy restatement of its rule (tests/bound_ref.py):
the partition, the rows' integers, bound_of and the stats equal -- tests/test_bound.py shows that no case used here
has a marginal decision -- every energy within the stated bound of the reference's, every sum within 1e-10 of its
sum of |term| (the moment terms) or 2e-6 (kinetic, potential).  Tiny states, every tile border, different fates in
one call, the other kinds of member, one group equal to the whole state against the diagnostics, bitwise
reproducibility over calls and tuning keys, independence of the other groups, permutations, the capacity, null
outputs, the refusals, that a call does not perturb the trajectory; the wrapper, the runner, the C++ mirror and the
CLI.  `-m gpu`."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from tests import bound_ref as B
from tests.helpers import ROOT, make_state

pytestmark = pytest.mark.gpu

TOL_MOMENT = 1e-10  # of the sum of |term|: the bound of nb_sim_fof's sums
TOL_ENERGY = 2e-6   # kinetic and potential, of the sum of |term|
FILL = 0xDEADBEEF
FILL_E = -12345.0


def _sim(nb, kind, state, params, theta=0.75):
    sp = nb.SimParams(particle_num=state.shape[0], g=params["g"], e=params["e"], dt=params["dt"])
    if kind == "naive":
        return nb.NaiveSim.from_particles(sp, None, state)
    return nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(theta), state)


def _params(_lib, link, min_members=20, min_bound=None, max_iter=32, max_group=262144, **_):
    p = _lib.nb_bound_params()
    p.link, p.min_members, p.max_iter, p.max_group = link, min_members, max_iter, max_group
    p.min_bound = min_members if min_bound is None else min_bound
    return p


def _raw(sim, params, capacity=None, call=None, handle=None, n=None):
    """The C call with every buffer pre-filled."""
    from wgpu_n_body_amd import _lib
    n = int(sim.sim_params().particle_num) if n is None else n
    p = _params(_lib, **params)
    cap = n // max(p.min_members, 1) if capacity is None else capacity
    group_of, bound_of = np.full(n, FILL, np.uint32), np.full(n, FILL, np.uint32)
    energy = np.full(n, FILL_E)
    rows = np.zeros(cap + 1, _lib.BOUND_GROUP_DTYPE)
    rows["label"] = FILL
    st = _lib.nb_bound_stats()
    rc = (call or _lib.lib().nb_sim_bound)(handle or sim._h, C.byref(p), group_of.ctypes.data, bound_of.ctypes.data,
                                           energy.ctypes.data, rows.ctypes.data, cap, C.byref(st))
    return SimpleNamespace(rc=rc, group_of=group_of, bound_of=bound_of, energy=energy, rows=rows, st=st, cap=cap,
                           bytes=group_of.tobytes() + bound_of.tobytes() + energy.tobytes() + rows.tobytes() + bytes(st))


def _bound(sim, params, **kw):
    from wgpu_n_body_amd import _lib
    g = _raw(sim, params, **kw)
    assert g.rc == 0, _lib.lib().nb_last_error()
    return g


STATS = ("n", "nonfinite", "components", "groups", "grouped_bodies", "largest_count", "largest_label", "bound_groups",
         "bound_bodies", "dissolved", "unconverged", "skipped", "rounds_max", "pairs")


def _check(g, ref, stats=True):
    """Every integer equal, every energy within the stated bound, every sum within its tolerance; rows beyond the
    catalogue untouched.  Returns the worst energy error in units of the bound."""
    if stats:
        for k in STATS:
            assert getattr(g.st, k) == ref[k], (k, getattr(g.st, k), ref[k])
    assert np.array_equal(g.group_of, ref["group_of"])
    k = len(ref["rows"])
    assert k == min(ref["groups"], g.cap)
    rows, want = g.rows[:k], ref["rows"]
    for f in ("label", "count", "bound_count", "iterations", "status"):
        assert np.array_equal(rows[f], want[f]), (f, np.flatnonzero(rows[f] != want[f])[:8])
    assert np.all(g.rows["label"][k:] == FILL) and not g.rows["mass"][k:].any()
    assert np.array_equal(g.bound_of, ref["bound_of"]), np.flatnonzero(g.bound_of != ref["bound_of"])[:8]
    # energies: NaN exactly where the reference has none, else within the bound
    assert np.array_equal(np.isnan(g.energy), np.isnan(ref["energy"]))
    has = ~np.isnan(ref["energy"])
    err = np.abs(g.energy[has] - ref["energy"][has])
    both_inf = np.isinf(ref["energy"][has]) & (g.energy[has] == ref["energy"][has])
    err[both_inf] = 0.0
    assert np.all(err <= ref["energy_tol"][has]), float(np.max(err - ref["energy_tol"][has]))
    assert np.array_equal(g.energy[has] > 0, ref["energy"][has] > 0)
    # sums over the bound set
    got = np.concatenate([rows["mass"][:, None], rows["mx"], rows["mv"], rows["mr2"][:, None], rows["kinetic"][:, None],
                          rows["potential"][:, None]], axis=1)
    exp = np.concatenate([want["mass"][:, None], want["mx"], want["mv"], want["mr2"][:, None], want["kinetic"][:, None],
                          want["potential"][:, None]], axis=1)
    tol = np.array([TOL_MOMENT] * 8 + [TOL_ENERGY] * 2)
    d = np.abs(got - exp)
    assert np.all(d <= tol * ref["scale"] + 1e-300), float((d / (tol * ref["scale"] + 1e-300)).max())
    for f in ("kinetic0", "potential0"):
        assert np.array_equal(np.isnan(rows[f]), np.isnan(want[f]))
        ran = ~np.isnan(want[f])
        assert np.all(np.abs(rows[f][ran] - want[f][ran]) <= TOL_ENERGY * np.abs(want[f][ran])), f
    # the potential minimum: the body the device names has, in the reference, a potential within the bound of the
    # smallest (two members closer than the bound are both right), and phi_min is that body's potential
    live = want["bound_count"] > 0
    assert np.all(rows["most_bound"][~live] == B.NONE) and np.all(np.isnan(rows["phi_min"][~live]))
    mb = rows["most_bound"][live]
    assert np.array_equal(g.bound_of[mb], np.flatnonzero(live))
    slack = ref["energy_tol"][mb]
    assert np.all(ref["phi"][mb] - want["phi_min"][live] <= 2 * slack)
    assert np.all(np.abs(rows["phi_min"][live] - ref["phi"][mb]) <= slack)
    sized = ref["energy_tol"][has] > 0  # (a body at rest alone in its group has error 0 of bound 0)
    return float(np.max(err[sized] / ref["energy_tol"][has][sized])) if sized.any() else 0.0


@pytest.mark.parametrize("n", [0, 1, 2])
@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_tiny_states(gpu, kind, n):
    nb = gpu
    state, params = B.case("two_at_rest")
    state = state[:n]
    sim = _sim(nb, kind, state, params)
    for link in (0.2, 0.01):
        for mm in (1, 2):
            p = dict(params, link=link, min_members=mm, min_bound=1)
            g = _bound(sim, p)
            ref = B.bound_ref(state, **p)
            assert int(ref["marginal"].sum()) == 0
            _check(g, ref)
    if n == 0:
        assert (g.st.groups, g.st.pairs, g.st.largest_label) == (0, 0, B.NONE)
    sim.destroy()


@pytest.mark.parametrize("tile", [0, 64, 256])
def test_every_tile_border(gpu, tile):
    """Groups of 1, 2, 63, 64, 65, 255, 256, 257 and 1,025 members in one call, by every tile size."""
    nb = gpu
    state, params = B.case("sizes")
    sim = _sim(nb, "naive", state, params)
    sim.set_tuning("bound_tile", tile)
    g = _bound(sim, params)
    ref = B.reference("sizes")
    assert tuple(ref["rows"]["count"]) == B.SIZES
    worst = _check(g, ref)
    print(f"sizes, tile {tile}: worst energy error {worst:.3f} of the bound")
    sim.destroy()


@pytest.mark.parametrize("name", ["fates", "fates_two_rounds"])
def test_different_fates_in_one_call(gpu, name):
    """300 clumps of 20-70 bodies and one of 5,000, shuffled: converged, dissolved, (two rounds) unconverged and
    (max_group 4,000) skipped rows side by side, the segments one work item each."""
    nb = gpu
    state, params = B.case(name)
    assert params["max_group"] == 4000
    sim = _sim(nb, "naive", state, params)
    sim.set_tuning("bound_chunk_len", 64)
    g = _bound(sim, params)
    ref = B.reference(name)
    worst = _check(g, ref)
    seen = set(int(s) for s in g.rows["status"][:ref["groups"]])
    assert seen == ({B.CONVERGED, B.DISSOLVED, B.SKIPPED} | ({B.UNCONVERGED} if name == "fates_two_rounds" else set()))
    print(f"{name}: worst energy error {worst:.3f} of the bound")
    sim.destroy()


@pytest.mark.parametrize("kind,name", [("naive", "two_at_rest"), ("naive", "two_fast"), ("naive", "interloper"),
                                       ("naive", "members"), ("tree", "members"), ("naive", "e0"), ("tree", "e0"),
                                       ("naive", "cascade")])
def test_against_the_reference(gpu, kind, name):
    nb = gpu
    state, params = B.case(name)
    sim = _sim(nb, kind, state, params)
    g = _bound(sim, params)
    worst = _check(g, B.reference(name))
    print(f"{name} on {kind}: worst energy error {worst:.3f} of the bound")
    sim.destroy()


def test_one_group_equal_to_the_whole_state(gpu):
    """potential0 of the one group is the diagnostics' pair potential: both are held to 2e-6 of binary64."""
    nb = gpu
    state, params = B.case("ball4096")
    sim = _sim(nb, "naive", state, params)
    bg = sim.bound_groups(params["link"], min_members=20)
    d = sim.diagnostics(potential=True)
    assert bg.stats.groups == 1 and bg.count[0] == 4096 and bg.rows["iterations"][0] >= 1
    u0 = bg.rows["potential0"][0]
    print(f"potential0 {u0!r} diagnostics {d.potential!r} relative {abs(u0 - d.potential) / abs(d.potential):.2e}")
    assert abs(u0 - d.potential) <= 4e-6 * abs(d.potential)
    # the kinetic energy about the group's velocity: the diagnostics' less that of the centre of mass
    v = np.array(d.momentum) / d.mass
    k0 = d.kinetic - 0.5 * d.mass * float(v @ v)
    assert abs(bg.rows["kinetic0"][0] - k0) <= 1e-9 * d.kinetic
    sim.destroy()


def test_two_calls_and_every_tuning_are_bit_identical(gpu):
    nb = gpu
    for name, extra in (("sizes", {}), ("fates", {"max_group": 0})):
        state, params = B.case(name)
        params = dict(params, **extra)
        sim = _sim(nb, "naive", state, params)
        first = _bound(sim, params)
        assert _bound(sim, params).bytes == first.bytes
        for chunk, tile in ((64, 0), (2048, 0), (4096, 256), (1048576, 0), (1024, 64), (1024, 256), (64, 64)):
            sim.set_tuning("bound_chunk_len", chunk)
            sim.set_tuning("bound_tile", tile)
            assert _bound(sim, params).bytes == first.bytes, (name, chunk, tile)
        fresh = _sim(nb, "naive", state, params)
        assert _bound(fresh, params).bytes == first.bytes
        fresh.destroy()
        sim.destroy()
    from wgpu_n_body_amd import _lib
    sim = _sim(nb, "naive", state, params)
    for key, bad in (("bound_chunk_len", 0), ("bound_chunk_len", 100), ("bound_chunk_len", 1 << 21), ("bound_tile", 128)):
        with pytest.raises(nb.NBodyError) as ex:
            sim.set_tuning(key, bad)
        assert ex.value.code == _lib.NB_ERR_INVALID
    sim.destroy()


def test_a_group_does_not_depend_on_the_others(gpu):
    """Every other group's bodies scattered to distant singletons, at the same indices: the group's row and its
    members' energies do not change by a bit -- nor with a capacity that leaves the later rows out."""
    nb = gpu
    state, params = B.case("fates")
    ref = B.reference("fates")
    rows = ref["rows"]
    pick = [int(r) for r in np.flatnonzero((rows["status"] == B.CONVERGED) & (rows["iterations"] >= 3))[:2]]
    pick.append(int(np.flatnonzero(rows["status"] == B.DISSOLVED)[0]))
    sim = _sim(nb, "naive", state, params)
    full = _bound(sim, params)
    sim.destroy()
    for r in pick:
        mem = ref["group_of"] == r
        alone = state.copy()
        others = np.flatnonzero(~mem)
        alone[others, 0:3] = np.stack([50.0 + 0.5 * np.arange(len(others)), np.zeros(len(others)), np.zeros(len(others))],
                                      axis=1)
        sim = _sim(nb, "naive", alone, params)
        g = _bound(sim, params)
        sim.destroy()
        assert g.st.groups == 1 and g.rows["label"][0] == rows["label"][r]
        assert g.rows[:1].tobytes() == full.rows[r:r + 1].tobytes()
        assert g.energy[mem].tobytes() == full.energy[mem].tobytes()
        assert np.array_equal(g.bound_of[mem] == 0, full.bound_of[mem] == r)
        assert np.all(np.isnan(g.energy[~mem])) and np.all(g.bound_of[~mem] == B.NONE)
    sim = _sim(nb, "naive", state, params)
    cap = pick[0] + 1
    part = _bound(sim, params, capacity=cap)
    sim.destroy()
    assert part.rows[:cap].tobytes() == full.rows[:cap].tobytes()
    inside = ref["group_of"] < cap
    assert part.energy[inside].tobytes() == full.energy[inside].tobytes()


def test_a_permutation_permutes_the_bound_sets(gpu):
    nb = gpu
    state, params = B.case("sizes")
    ref = B.reference("sizes")
    perm = np.random.default_rng(4).permutation(len(state))
    sets, energies = [], []
    for s, back in ((state, np.arange(len(state))), (state[perm], perm)):
        sim = _sim(nb, "naive", s, params)
        before = sim.fof_groups(params["link"], min_members=params["min_members"])
        g = _bound(sim, params)
        after = sim.fof_groups(params["link"], min_members=params["min_members"])
        sim.destroy()
        # nb_sim_fof returns what it returned before the call, and the call's group_of is its group_of
        assert before.labels.tobytes() == after.labels.tobytes() and before.rows.tobytes() == after.rows.tobytes()
        assert np.array_equal(g.group_of, before.group_of)
        by_row = {}
        for i in np.flatnonzero(g.bound_of != B.NONE):
            by_row.setdefault(int(g.bound_of[i]), []).append(int(back[i]))
        sets.append({frozenset(v) for v in by_row.values()})
        e = np.empty(len(state))
        e[back] = g.energy
        energies.append(e)
    assert sets[0] == sets[1] and len(sets[0]) == ref["bound_groups"]
    assert np.all(np.abs(energies[0] - energies[1]) <= 2 * ref["energy_tol"])


def test_capacity_smaller_than_the_catalogue(gpu):
    nb = gpu
    state, params = B.case("sizes")
    sim = _sim(nb, "naive", state, params)
    full = _bound(sim, params)
    for cap in (0, 1, 3, 8):
        g = _bound(sim, params, capacity=cap)
        _check(g, B.reference("sizes", capacity=cap))
        assert g.st.groups == 9 and g.rows[:cap].tobytes() == full.rows[:cap].tobytes()
    sim.destroy()


def test_null_outputs(gpu):
    nb = gpu
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    state, params = B.case("members")
    n = len(state)
    sim = _sim(nb, "naive", state, params)
    full = _bound(sim, params)
    p = _params(_lib, **params)
    cap = full.cap
    assert L.nb_sim_bound(sim._h, C.byref(p), None, None, None, None, cap, None) == 0
    for mask in range(1, 32):
        gof = np.full(n, FILL, np.uint32) if mask & 1 else None
        bof = np.full(n, FILL, np.uint32) if mask & 2 else None
        en = np.full(n, FILL_E) if mask & 4 else None
        rows = np.zeros(cap + 1, _lib.BOUND_GROUP_DTYPE) if mask & 8 else None
        st = _lib.nb_bound_stats() if mask & 16 else None
        ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
        assert L.nb_sim_bound(sim._h, C.byref(p), ptr(gof), ptr(bof), ptr(en), ptr(rows), cap,
                              C.byref(st) if st is not None else None) == 0, mask
        assert gof is None or np.array_equal(gof, full.group_of)
        assert bof is None or np.array_equal(bof, full.bound_of)
        assert en is None or en.tobytes() == full.energy.tobytes()
        assert rows is None or (rows[:2].tobytes() == full.rows[:2].tobytes() and not rows[2:].tobytes().strip(b"\0"))
        assert st is None or bytes(st) == bytes(full.st)
    sim.destroy()


def test_refusals(gpu):
    nb = gpu
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    state, params = B.case("interloper")

    def untouched(g):
        return np.all(g.group_of == FILL) and np.all(g.bound_of == FILL) and np.all(g.energy == FILL_E) and \
            np.all(g.rows["label"] == FILL) and bytes(g.st) == bytes(_lib.nb_bound_stats())

    sim = _sim(nb, "naive", state, params)
    for bad in (dict(link=0.0), dict(min_members=0), dict(min_bound=0), dict(max_iter=0), dict(max_iter=65)):
        g = _raw(sim, dict(params, **bad), capacity=8)
        assert g.rc == _lib.NB_ERR_INVALID and L.nb_last_error() and untouched(g)
    sim.destroy()
    # a negative softening has no potential
    sim = _sim(nb, "naive", state, dict(params, e=-1e-4))
    g = _raw(sim, params)
    assert g.rc == _lib.NB_ERR_INVALID and b"e >= 0" in L.nb_last_error() and untouched(g)
    sim.destroy()
    # one far body pushes an axis past 2^21 cells: refused after the synchronisation, nothing written
    far = state.copy()
    far[17, 0] = 3.0e4
    sim = _sim(nb, "naive", far, params)
    g = _raw(sim, dict(params, link=0.01))
    assert g.rc == _lib.NB_ERR_INVALID and b"cells" in L.nb_last_error() and untouched(g)
    ok = _bound(sim, params)  # the simulator stays usable
    fresh = _sim(nb, "naive", far, params)
    assert _bound(fresh, params).bytes == ok.bytes
    fresh.destroy()
    with pytest.raises(nb.NBodyError) as ex:
        sim.bound_groups(0.01)
    assert ex.value.code == _lib.NB_ERR_INVALID
    sim.destroy()
    # a sharded simulator (rank 0 of 2)
    s64 = make_state("uniform", 64, seed=1)
    sharded = nb.NaiveSim.from_particles(nb.SimParams(particle_num=64), None, s64, placement=nb.Placement(world=2))
    g = _raw(sharded, params, n=64)
    assert g.rc == _lib.NB_ERR_UNSUPPORTED and b"sharded" in L.nb_last_error() and untouched(g)
    sharded.destroy()
    # a several-GPU runner, both ranks on device 0
    r = nb.OfflineHeadless(nb.NaiveSim, nb.SimParams(particle_num=512), None,
                           lambda p: nb.inits.uniform_init(p, seed=1), device_ids=[0, 0])
    with pytest.raises(nb.NBodyError) as ex:
        r.bound_groups(0.1)
    assert ex.value.code == _lib.NB_ERR_UNSUPPORTED
    r.destroy()


@pytest.mark.parametrize("case", ["naive", "tree", "tree_graph"])
def test_does_not_perturb_the_trajectory(gpu, case):
    nb = gpu
    n, steps = 4096, 10
    state = make_state("uniform", n, seed=9)
    finals = []
    for with_bound in (False, True):
        sp = nb.SimParams(particle_num=n)
        sim = nb.NaiveSim.from_particles(sp, None, state) if case == "naive" else \
            nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(0.75), state)
        if case == "tree_graph":
            sim.set_tuning("tree_use_graph", 1)
        for k in range(steps):
            sim.encode()
            if with_bound:
                bg = sim.bound_groups(0.03 if k % 2 else 0.06, min_members=2, max_iter=4, per_body=k % 3 == 0)
                assert bg.stats.step_num == k + 1 and bg.stats.n == n and bg.stats.groups > 0
        finals.append(nb.as_floats(sim.read_particles()).copy())
        sim.destroy()
    assert np.array_equal(finals[0].view(np.uint32), finals[1].view(np.uint32))


def test_python_wrapper(gpu):
    nb = gpu
    state, params = B.case("fates")
    ref = B.reference("fates")
    sim = _sim(nb, "naive", state, params)
    bg = sim.bound_groups(params["link"], min_members=20, min_bound=10, max_group=4000)
    g = _bound(sim, params)
    assert bg.rows.tobytes() == g.rows[:ref["groups"]].tobytes() and bg.rows.shape == (ref["groups"],)
    assert np.array_equal(bg.group_of, g.group_of) and np.array_equal(bg.bound_of, g.bound_of)
    assert bg.energy.tobytes() == g.energy.tobytes()
    assert (bg.min_members, bg.min_bound, bg.max_iter, bg.max_group) == (20, 10, 32, 4000)
    for k in STATS:
        assert getattr(bg.stats, k) == ref[k], k
    assert sim.bound_groups(params["link"]).min_bound == 20  # min_bound defaults to min_members
    live = np.flatnonzero(bg.bound_count > 0)
    s = state.astype(np.float64)
    for r in live[:3]:
        mem = bg.bound_of == r
        m = s[mem, 9]
        assert np.allclose(bg.com[r], (m[:, None] * s[mem, 0:3]).sum(axis=0) / m.sum(), rtol=0, atol=1e-9)
        assert np.allclose(bg.velocity[r], (m[:, None] * s[mem, 3:6]).sum(axis=0) / m.sum(), rtol=0, atol=1e-9)
    assert np.array_equal(bg.bound_fraction, bg.bound_count / bg.count)
    ran = bg.rows["iterations"] > 0
    assert np.allclose(bg.virial_ratio[ran], 2 * bg.rows["kinetic0"][ran] / -bg.rows["potential0"][ran])
    assert np.all(np.isnan(bg.virial_ratio[~ran])) and (~ran).sum() == 1
    order = bg.by_bound_mass()
    assert sorted(order) == list(range(ref["groups"]))
    assert all((bg.mass[a], -int(bg.label[a])) >= (bg.mass[b], -int(bg.label[b])) for a, b in zip(order, order[1:]))
    quiet = sim.bound_groups(params["link"], min_members=20, min_bound=10, max_group=4000, per_body=False)
    assert quiet.bound_of is None and quiet.energy is None and quiet.rows.tobytes() == bg.rows.tobytes()
    sim.destroy()


def test_runner_and_cli(gpu):
    """nb_runner_bound equals nb_sim_bound on nb_runner_sim, and headless --bound (the C++ mirror over
    nb_runner_bound) prints what the Python runner returns."""
    nb = gpu
    from wgpu_n_body_amd import _lib
    cli = os.path.join(ROOT, "wgpu_n_body_amd", "headless")
    base = [cli, "--sim", "naive", "--n", "4096", "--init", "disc", "--steps", "2"]
    link = 0.02
    p = subprocess.run(base + ["--bound", "2", "--bound-link", repr(link), "--bound-min", "5", "--bound-iter", "8",
                               "--bound-top", "3"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    plain = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "bound" not in plain.stdout
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("bound ")]
    tops = [ln for ln in p.stdout.splitlines() if ln.startswith("bound_group ")]
    assert len(lines) == 2

    runner = nb.OfflineHeadless(nb.NaiveSim, nb.SimParams(particle_num=4096), None,
                                lambda sp: nb.inits.disc_init(sp, seed=0))
    params = dict(link=link, min_members=5, min_bound=5, max_iter=8)
    ours = [runner.bound_groups(link, min_members=5, max_iter=8)]
    runner.step()
    runner.step()
    ours.append(runner.bound_groups(link, min_members=5, max_iter=8))
    via_runner = _raw(None, params, call=_lib.lib().nb_runner_bound, handle=runner._h, n=4096)
    via_sim = _raw(runner.sim, params)
    runner.destroy()
    assert via_runner.rc == via_sim.rc == 0 and via_runner.bytes == via_sim.bytes
    assert via_sim.rows[:ours[1].stats.groups].tobytes() == ours[1].rows.tobytes()
    # the runner's path against the reference, on states tests/test_bound.py shows to be decisive
    for name in ("members", "cascade"):
        state, cp = B.case(name)
        held = nb.OfflineHeadless(nb.NaiveSim, nb.SimParams(particle_num=len(state), g=cp["g"], e=cp["e"], dt=cp["dt"]),
                                  None, lambda sp, s=state: nb.as_particles(s))
        g = _raw(None, cp, call=_lib.lib().nb_runner_bound, handle=held._h, n=len(state))
        bg = held.bound_groups(cp["link"], min_members=cp["min_members"], min_bound=cp.get("min_bound"))
        held.destroy()
        assert g.rc == 0, _lib.lib().nb_last_error()
        _check(g, B.reference(name))
        assert bg.rows.tobytes() == g.rows[:bg.stats.groups].tobytes() and bg.energy.tobytes() == g.energy.tobytes()
    o = ours[0]  # the same seeded init, no step yet: the line is the Python call
    st = o.stats
    assert [int(x) for x in lines[0].split()[1:]] == [0, st.groups, st.bound_groups, st.bound_bodies, st.dissolved,
                                                      st.unconverged, st.skipped, st.rounds_max, st.pairs]
    assert int(lines[1].split()[1]) == 2 == ours[1].stats.step_num
    assert o.stats.groups >= 3
    for ln, r in zip([t.split() for t in tops[:3]], o.by_bound_mass()[:3]):
        assert [int(x) for x in ln[1:8]] == [0, int(r), int(o.label[r]), int(o.count[r]), int(o.bound_count[r]),
                                             int(o.rows["iterations"][r]), int(o.status[r])]
        assert float(ln[8]) == pytest.approx(o.mass[r], rel=1e-8)
        assert float(ln[12]) == pytest.approx(o.rows["kinetic"][r], rel=1e-8, abs=1e-300)
        assert float(ln[13]) == pytest.approx(o.rows["potential"][r], rel=1e-8, abs=1e-300)
