"""nb_group_radii_sim on the device (csrc/nb_radii.hip) against the numpy restatement of its rule
(tests/radii_ref.py): everything equal to the last bit -- the order, the enclosed mass at every member, the
crossings, the peak of M / r, the centres formed on the device.  Rows across every run and chunk border at unaligned
starts, empty rows, bodies of no row, non-finite members, duplicate positions, members at the centre; a row's bits
independent of the other rows, of its number and of the call; the centre of nb_sim_group_shapes; the whole state as one
row against the binned radii; each kind of catalogue; the refusals, null outputs, the trajectory; the runner, the
C++ mirror and the CLI.  `-m gpu`."""
import ctypes as C
import functools
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from tests import radii_ref as R
from tests.helpers import ROOT

pytestmark = pytest.mark.gpu

FILL = 0xDEADBEEF
G, E, DT = 1e-6, 1e-4, 0.016
SIZES = (1, 2, 63, 64, 65, 4095, 4096, 4097, 8193, 20011)
FLOATS = ("center", "mass", "r_min", "r_max", "vc2_max", "r_vmax", "radius")
INTS = ("count", "vmax_index", "index")
STATS = ("n", "rows", "members", "nonfinite_members", "empty")


def _sim(nb, kind, state, theta=0.75, **kw):
    sp = nb.SimParams(particle_num=state.shape[0], g=G, e=E, dt=DT)
    if kind == "naive":
        return nb.NaiveSim.from_particles(sp, None, state, **kw)
    return nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(theta), state, **kw)


def _raw(sim, gof, m, fractions=(0.1, 0.5, 0.9), centers=None, vmax_skip=10, step_num=None, call=None, handle=None,
         n=None, outputs=("rows", "rank", "enc", "st"), reserved=0):
    """The C call with every buffer pre-filled."""
    from wgpu_n_body_amd import _lib
    n = int(sim.sim_params().particle_num) if n is None else n
    p = _lib.nb_radii_params()
    p.nf, p.vmax_skip, p.reserved = len(fractions), vmax_skip, reserved
    for k, f in enumerate(list(fractions)[:16]):
        p.fractions[k] = f
    p.step_num = _lib.NB_RADII_ANY_STEP if step_num is None else step_num
    centers = None if centers is None else np.ascontiguousarray(np.asarray(centers, np.float64).reshape(-1, 3))
    gof = None if gof is None else np.ascontiguousarray(gof, np.uint32)
    rows = np.zeros(m + 1, _lib.RADII_GROUP_DTYPE)
    rows["count"] = FILL
    rank = np.full(n + 1, FILL, np.uint32)
    enc = np.full(n + 1, -7.0)
    st = _lib.nb_radii_stats()
    st.empty = 77
    ptr = lambda a: a.ctypes.data if a is not None else None
    rc = (call or _lib.lib().nb_group_radii_sim)(
        handle or sim._h, C.byref(p), ptr(gof), m, ptr(centers), rows.ctypes.data if "rows" in outputs else None,
        rank.ctypes.data if "rank" in outputs else None, enc.ctypes.data if "enc" in outputs else None,
        C.byref(st) if "st" in outputs else None)
    return SimpleNamespace(rc=rc, rows=rows, rank=rank, enc=enc, st=st, m=m, n=n,
                           bytes=rows.tobytes() + rank.tobytes() + enc.tobytes() + bytes(st))


def _radii(sim, gof, m, **kw):
    from wgpu_n_body_amd import _lib
    g = _raw(sim, gof, m, **kw)
    assert g.rc == 0, _lib.lib().nb_last_error()
    assert g.rows["count"][m] == FILL and g.rank[g.n] == FILL and g.enc[g.n] == -7.0  # nothing past the end
    return g


def _untouched(g):
    return np.all(g.rows["count"] == FILL) and np.all(g.rank == FILL) and np.all(g.enc == -7.0) and g.st.empty == 77


def _check(g, ref):
    """Every value equal: integers with ==, doubles bit for bit (NaN where the reference has NaN)."""
    for k in STATS:
        assert getattr(g.st, k) == ref["stats"][k], (k, getattr(g.st, k), ref["stats"][k])
    rows, want = g.rows[:g.m], ref["rows"]
    for f in INTS:
        assert np.array_equal(rows[f], want[f]), (f, np.flatnonzero((rows[f] != want[f]).reshape(g.m, -1).any(axis=1))[:8])
    for f in FLOATS:
        bad = ~((rows[f] == want[f]) | (np.isnan(rows[f]) & np.isnan(want[f])))
        assert not bad.any(), (f, np.flatnonzero(bad.reshape(g.m, -1).any(axis=1))[:8])
    assert np.array_equal(g.rank[:g.n], ref["rank_of"]), np.flatnonzero(g.rank[:g.n] != ref["rank_of"])[:8]
    assert np.array_equal(g.enc[:g.n], ref["enclosed_of"], equal_nan=True)


@functools.lru_cache(maxsize=None)
def _borders():
    """(plain, state, gof, m, centers): rows of SIZES members at unaligned starts, two empty rows, 300 bodies of no
    row: 40,987 bodies; rows 0..4 have equal masses.  `state` is `plain` with duplicate positions in row 7, five
    members of row 6 at what the explicit centres give it, and seven members of three rows not finite -- what an
    all-pairs simulator takes and an octree cannot (it refuses bodies that share a position)."""
    rng = np.random.default_rng(20261)
    parts = [R.cloud(rng, k, centre=(3.0 * i, -2.0 * (i % 3), 0.5 * i), scale=0.2 + 0.1 * i, equal_mass=i < 5)
             for i, k in enumerate(SIZES)]
    plain, gof, m = R.assemble(rng, parts, loose=300, extra_rows=2)
    centers = np.array([[3.0 * i, -2.0 * (i % 3), 0.5 * i] for i in range(m)], np.float64)
    state = plain.copy()
    of = lambda row: np.flatnonzero(gof == row)
    state[of(7)[100:140], 0:3] = state[of(7)[200:240], 0:3]  # duplicate positions, unequal masses
    state[of(7)[300:310], 0:3] = state[of(7)[300], 0:3]
    state[of(6)[0:5], 0:3] = centers[6].astype(np.float32)   # at the explicit centre of row 6
    for row, field, value in ((9, 0, np.nan), (9, 9, np.inf), (8, 4, np.nan), (5, 2, -np.inf), (9, 1, np.nan),
                              (8, 9, np.nan), (5, 0, np.inf)):
        state[of(row)[3 + field], field] = value
    for a in (plain, state, gof, centers):
        a.setflags(write=False)
    return plain, state, gof, m, centers


@pytest.mark.parametrize("n", [0, 1, 2])
def test_tiny_states(gpu, n):
    rng = np.random.default_rng(3)
    state = R.cloud(rng, 2)[:n]
    sim = _sim(gpu, "naive", state)
    none = np.full(n, R.NONE, np.uint32)
    for gof, m in ((none, 0), (none, 1), (np.zeros(n, np.uint32), 1), (np.arange(n, dtype=np.uint32), max(n, 1))):
        for kw in (dict(vmax_skip=0), dict(centers=np.zeros((m, 3)))):
            g = _radii(sim, gof if n else None, m, **kw)
            _check(g, R.radii_ref(state, gof, m, **kw))


@pytest.mark.parametrize("given", [True, False])
@pytest.mark.parametrize("vmax_skip", [0, 10, 100000])
def test_every_border_on_the_all_pairs_simulator(gpu, vmax_skip, given):
    """Every run and chunk border, empty rows, bodies of no row, non-finite members, duplicates and members at the
    centre, about explicit centres and about the ones formed on the device."""
    _, state, gof, m, centers = _borders()
    sim = _sim(gpu, "naive", state)
    kw = dict(vmax_skip=vmax_skip, centers=centers if given else None, fractions=(0.01, 0.1, 0.25, 0.5, 0.9, 1.0))
    g = _radii(sim, gof, m, **kw)
    ref = R.radii_ref(state, gof, m, **kw)
    assert sorted(ref["rows"]["count"].tolist()) == sorted([0, 0, 1, 2, 63, 64, 65, 4093, 4096, 4097, 8191, 20008])
    assert ref["stats"]["nonfinite_members"] == 7 and ref["stats"]["empty"] == 2
    if given:  # five members at the centre: r2 = 0, passed over by v_max
        assert ref["rows"]["r_min"][6] == 0.0
        if vmax_skip == 0:
            assert ref["rank_of"][ref["rows"]["vmax_index"][6]] >= 5
    if vmax_skip == 100000:
        assert np.all(ref["rows"]["vmax_index"] == R.NONE)
    else:
        assert np.all(ref["rows"]["vmax_index"][ref["rows"]["count"] > vmax_skip + 5] != R.NONE)
    _check(g, ref)


def test_after_a_step_of_the_tree_simulator(gpu):
    """The bodies reordered by a Barnes-Hut step: the assignment is to the order read back now.  (The state without
    the duplicates and the non-finite bodies, which an octree does not take; a member at the centre stays.)"""
    state, _, gof, m, centers = _borders()
    sim = _sim(gpu, "tree", state)
    sim.encode()
    now = gpu.as_floats(sim.dest_particle_slice()).copy()
    assert not np.array_equal(now[:, 9], state[:, 9])  # reordered
    centers = centers.copy()
    centers[6] = now[np.flatnonzero(gof == 6)[5], 0:3].astype(np.float64)  # a member: r2 = 0
    for kw in (dict(centers=centers, step_num=1), dict(fractions=(0.5,), vmax_skip=0)):
        g = _radii(sim, gof, m, **kw)
        kw.pop("step_num", None)
        _check(g, R.radii_ref(now, gof, m, **kw))


def test_a_rows_bits_are_its_own(gpu):
    """Row 8 (8,193 members) when the other rows change, when it is renumbered, and between two calls."""
    state, _, gof, m, centers = _borders()
    sim = _sim(gpu, "naive", state)
    first = _radii(sim, gof, m)
    assert _radii(sim, gof, m).bytes == first.bytes
    mine = gof == 8
    for other, row, rows in ((np.where(mine, 0, R.NONE), 0, 1),                      # alone, renumbered to 0
                             (np.where(mine, 3, np.where(gof == 9, 0, R.NONE)), 3, 5),  # behind another big row
                             (np.where(mine, 8, np.where(gof < 4, 9, gof)), 8, m)):   # the small rows merged
        g = _radii(sim, other.astype(np.uint32), rows)
        assert g.rows[row:row + 1].tobytes() == first.rows[8:9].tobytes()
        assert np.array_equal(g.rank[:g.n][mine], first.rank[:g.n][mine])
        assert g.enc[:g.n][mine].tobytes() == first.enc[:g.n][mine].tobytes()


def test_null_centres_are_group_shapes_centres(gpu):
    state, _, gof, m, _ = _borders()
    sim = _sim(gpu, "naive", state)
    shapes = sim.shapes_of(gof, m)
    radii = sim.radii_of(gof, m)
    has = shapes.rows["count"] > 0
    assert has.sum() == m - 2 and np.array_equal(radii.rows["count"], shapes.rows["count"])
    assert radii.rows["center"][has].tobytes() == shapes.rows["center"][has].tobytes()
    assert np.isnan(radii.rows["center"][~has]).all() and np.isnan(shapes.rows["center"][~has]).all()


def test_the_whole_state_as_one_row(gpu):
    """lagrangian_radii on 70,000 bodies: each exact radius lies in the bin where the binned estimate puts it."""
    rng = np.random.default_rng(11)
    state = R.cloud(rng, 70000, centre=(0.3, -0.2, 0.1))
    sim = _sim(gpu, "naive", state)
    fractions = (0.01, 0.05, 0.1, 0.25, 0.5, 0.75, 0.9)
    centre = (0.3, -0.2, 0.1)
    got = sim.lagrangian_radii(fractions, center=centre)
    assert got.rows["count"][0] == 70000 and got.radius.shape == (1, 7) and np.all(np.diff(got.radius[0]) > 0)
    prof = sim.radial_profile(rmin=1e-3, rmax=20.0, nbins=64, center=centre)
    binned = prof.lagrangian(fractions)
    k = np.searchsorted(prof.edges, binned, side="right") - 1
    assert np.all((prof.edges[k] <= got.radius[0]) & (got.radius[0] <= prof.edges[k + 1])), (got.radius[0], binned)
    assert got.half_mass_radius[0] == got.radius[0, 4]
    ref = R.radii_ref(state, np.zeros(70000, np.uint32), 1, fractions=fractions, centers=[centre])
    assert got.rows.tobytes() == ref["rows"].tobytes()
    own = sim.lagrangian_radii(fractions, per_body=True)  # about its own centre of mass, formed on the device
    ref = R.radii_ref(state, np.zeros(70000, np.uint32), 1, fractions=fractions)
    assert own.rows.tobytes() == ref["rows"].tobytes() and np.array_equal(own.rank_of, ref["rank_of"])
    assert np.array_equal(own.enclosed_of, ref["enclosed_of"])
    dens = sim.lagrangian_radii((0.5,), center="density")
    assert np.array_equal(dens.rows["center"][0], sim.knn_density(6, neighbours=False).center)
    assert np.isfinite(dens.vmax(G)[0]) and dens.r_vmax[0] > 0


def _two_clumps():
    rng = np.random.default_rng(77)
    parts = [R.cloud(rng, 900, centre=(0, 0, 0), scale=0.05), R.cloud(rng, 500, centre=(3, 0, 0), scale=0.05),
             R.cloud(rng, 200, centre=(1.5, 1.5, 1.5), scale=4.0)]
    for p in parts:
        p[:, 3:6] *= 0.01
    state = np.concatenate(parts)
    return np.ascontiguousarray(state[rng.permutation(len(state))])


def test_each_kind_of_catalogue(gpu):
    nb = gpu
    state = _two_clumps()
    sim = _sim(nb, "tree", state)
    sim.encode()
    now = nb.as_floats(sim.dest_particle_slice()).copy()
    fof = sim.fof_groups(0.05, min_members=20)
    assert len(fof.rows) == 2
    got = sim.group_radii(fof, per_body=True)
    ref = R.radii_ref(now, fof.group_of, 2, centers=fof.com)
    assert got.rows.tobytes() == ref["rows"].tobytes() and np.array_equal(got.rank_of, ref["rank_of"])
    assert got.stats.step_num == 1 and np.array_equal(got.catalogue_rows, [0, 1])
    assert got.stats.members == int((fof.group_of != R.NONE).sum())
    assert np.all(got.half_mass_radius < 0.2) and np.all(np.isfinite(got.vmax(G)))

    bound = sim.bound_groups(0.05, min_members=20)
    got = sim.group_radii(bound, members="bound", center="most_bound", fractions=(0.5,), vmax_skip=3)
    rows = got.catalogue_rows
    assert np.array_equal(rows, np.flatnonzero(bound.rows["most_bound"] != R.NONE)) and len(rows) >= 1
    renumber = np.full(len(bound.rows) + 1, R.NONE, np.uint32)
    renumber[rows] = np.arange(len(rows))
    at = bound.rows["most_bound"][rows]
    ref = R.radii_ref(now, renumber[np.minimum(bound.bound_of, len(bound.rows))], len(rows), fractions=(0.5,),
                      centers=now[at, 0:3].astype(np.float64), vmax_skip=3)
    assert got.rows.tobytes() == ref["rows"].tobytes() and got.rank_of is None
    assert np.all(got.rows["r_min"] == 0.0)  # the most bound body is a member

    hop = sim.hop_groups(k_density=32, k_hop=16, k_merge=4, min_members=20)
    assert len(hop.rows) >= 2
    got = sim.group_radii(hop, center="peak")
    ref = R.radii_ref(now, hop.group_of, len(hop.rows), centers=now[hop.rows["label"], 0:3].astype(np.float64))
    assert got.rows.tobytes() == ref["rows"].tobytes()

    sim.encode()
    with pytest.raises(nb.NBodyError):
        sim.group_radii(fof)  # a catalogue of the step before
    assert len(sim.group_radii(fof, check_step=False).rows) == 2


def test_refusals(gpu):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(5)
    state, gof, m = R.assemble(rng, [R.cloud(rng, 300), R.cloud(rng, 200, centre=(2, 0, 0))], loose=20)
    sim = _sim(gpu, "tree", state)

    def refused(word, code=_lib.NB_ERR_INVALID, **over):
        args = dict(over)
        g = _raw(sim, args.pop("gof", gof), args.pop("m", m), **args)
        assert g.rc == code, (word, g.rc)
        assert word in L.nb_last_error(), (word, L.nb_last_error())
        assert _untouched(g)

    bad = gof.copy()
    bad[11] = m
    bad[40] = 0xFFFFFFFE
    refused(b"group_of[11]", gof=bad)  # after the call's synchronisation: the outputs are untouched
    refused(b"null group_of", gof=None)
    refused(b"rows", m=len(state) + 1)
    refused(b"nf", fractions=())
    refused(b"nf", fractions=tuple(np.linspace(0.01, 0.99, 17)))
    for f in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        refused(b"fractions[1]", fractions=(0.001, f))
    refused(b"ascending", fractions=(0.5, 0.5))
    refused(b"ascending", fractions=(0.5, 0.25))
    refused(b"reserved", reserved=1)
    c = np.zeros((m, 3))
    c[1, 2] = np.nan
    refused(b"row 1", centers=c)
    assert _raw(sim, gof, m, step_num=0).rc == 0
    sim.encode()
    refused(b"step", step_num=0)
    assert _raw(sim, gof, m, step_num=1).rc == 0  # the simulator is still usable
    sp = gpu.SimParams(particle_num=len(state), g=G, e=E, dt=DT)
    shard = gpu.NaiveSim.from_particles(sp, None, state, placement=gpu.Placement(world=2))
    n_shard = int(shard.sim_params().particle_num)
    g = _raw(shard, np.full(n_shard, R.NONE, np.uint32), 1, n=n_shard)
    assert g.rc == _lib.NB_ERR_UNSUPPORTED and b"sharded" in L.nb_last_error() and _untouched(g)


def test_null_outputs(gpu):
    """Every output pointer null in turn: the others are what the full call returns."""
    rng = np.random.default_rng(6)
    state, gof, m = R.assemble(rng, [R.cloud(rng, 5000), R.cloud(rng, 70, centre=(2, 0, 0))], loose=20, extra_rows=1)
    sim = _sim(gpu, "naive", state)
    full = _radii(sim, gof, m)
    for outputs in (("rank", "enc", "st"), ("rows", "enc", "st"), ("rows", "rank", "st"), ("rows", "rank", "enc"),
                    ("rows",), ("st",), ()):
        g = _radii(sim, gof, m, outputs=outputs)
        assert g.rows.tobytes() == full.rows.tobytes() if "rows" in outputs else np.all(g.rows["count"] == FILL)
        assert np.array_equal(g.rank, full.rank) if "rank" in outputs else np.all(g.rank == FILL)
        assert g.enc.tobytes() == full.enc.tobytes() if "enc" in outputs else np.all(g.enc == -7.0)
        assert bytes(g.st) == bytes(full.st) if "st" in outputs else g.st.empty == 77


@pytest.mark.parametrize("kind", ["naive", "tree", "tree_graph"])
def test_a_call_does_not_perturb_the_trajectory(gpu, kind):
    rng = np.random.default_rng(7)
    state, gof, m = R.assemble(rng, [R.cloud(rng, 5000), R.cloud(rng, 700, centre=(2, 0, 0))], loose=20)
    a, b = _sim(gpu, kind[:5].rstrip("_"), state), _sim(gpu, kind[:5].rstrip("_"), state)
    if kind == "tree_graph":
        a.set_tuning("tree_use_graph", 1)
        b.set_tuning("tree_use_graph", 1)
    _radii(a, gof, m)
    for _ in range(3):
        a.encode()
        b.encode()
    _radii(a, gof, m, centers=np.zeros((m, 3)))
    a.encode()
    b.encode()
    assert a.dest_particle_slice().tobytes() == b.dest_particle_slice().tobytes()


def test_runner_cpp_mirror_and_cli(gpu):
    """nb_group_radii_runner equals nb_group_radii_sim on nb_runner_sim, and headless --lagr / --radii (the C++ mirror)
    print what the Python runner returns."""
    nb = gpu
    from wgpu_n_body_amd import _lib
    sp = nb.SimParams(particle_num=4096, g=1e-4, e=E, dt=DT)
    runner = nb.OfflineHeadless.new(nb.TreeSim, sp, nb.AddParams.TreeSimParams(0.75), nb.inits.disc_init)
    held = nb.Simulator(_lib.lib().nb_runner_sim(runner._h), borrowed=True)
    link = 0.02
    fof = runner.fof_groups(link, min_members=20)
    assert len(fof.rows) >= 2
    via_runner = runner.group_radii(fof)
    via_sim = held.group_radii(fof)
    assert via_runner.rows.tobytes() == via_sim.rows.tobytes()
    raw = _raw(None, fof.group_of, len(fof.rows), centers=fof.com, step_num=0,
               call=_lib.lib().nb_group_radii_runner, handle=runner._h, n=4096)
    assert raw.rc == 0 and raw.rows[:len(fof.rows)].tobytes() == via_runner.rows.tobytes()
    fractions = (0.1, 0.5, 0.75)
    whole = runner.lagrangian_radii(fractions)
    about = runner.lagrangian_radii(fractions, center=(0.5, 0.0, -0.25))

    exe = os.path.join(ROOT, "wgpu_n_body_amd", "headless")
    base = [exe, "--sim", "tree", "--n", "4096", "--init", "disc", "--g", "1e-4", "--steps", "0"]
    for extra, want in (([], whole), (["--lagr-center", "0.5,0.0,-0.25"], about)):
        out = subprocess.run(base + ["--lagr", "1", "--lagr-fractions", "0.1,0.5,0.75"] + extra, capture_output=True,
                             text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        lines = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("lagr")]
        row = want.rows[0]
        assert lines[0][:3] == ["lagr", "0", str(row["count"])]
        got = np.array([float(x) for x in lines[0][3:]])
        assert np.array_equal(got, np.concatenate([[row["mass"]], row["center"], [row["r_vmax"], row["vc2_max"]]]))
        assert len(lines) == 4
        for k, ln in enumerate(lines[1:]):
            assert ln[:2] == ["lagr_radius", "0"] and ln[4] == str(row["index"][k])
            assert float(ln[2]) == fractions[k] and float(ln[3]) == row["radius"][k]  # %.17g round-trips

    out = subprocess.run(base + ["--radii", "1", "--radii-link", str(link), "--radii-min", "20", "--radii-top", "3"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("radii")]
    st = via_runner.stats
    assert lines[0] == ["radii", "0", str(st.rows), str(st.members), str(st.empty)]
    order = fof.by_size()[:3]
    assert len(lines) == 1 + len(order)
    for ln, r in zip(lines[1:], order):
        row = via_runner.rows[r]
        assert ln[:4] == ["radii_group", "0", str(r), str(row["count"])]
        got = np.array([float(x) for x in ln[4:]])
        want = np.concatenate([[row["mass"]], row["radius"][:3], [row["r_vmax"], row["vc2_max"]]])
        assert np.array_equal(got, want, equal_nan=True), (got, want)
