"""nb_sim_hop on the device (csrc/nb_hop.hip) against the numpy restatement of its rule (tests/hop_ref.py) on the
read-back state: labels, group_of, the catalogue's labels and counts, the boundary table with its densities, the
peak densities and every integer of the stats equal, every sum to 1e-10 of its sum of |term|; the density equal
to nb_sim_knn's bit for bit.  `-m gpu`."""
import ctypes as C
import math
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from tests import fof_ref
from tests import hop_ref as H
from tests import knn_ref as K
from tests.helpers import ROOT, make_state

pytestmark = pytest.mark.gpu

TOL = 1e-10  # of the sum of |term|: TOL of tests/test_fof_gpu.py
FILL = 0xDEADBEEF
KS = [(2, 1, 1), (6, 6, 6), (32, 16, 4), (64, 64, 64), (8, 64, 2)]


def _sim(nb, kind, state, theta=0.75):
    sp = nb.SimParams(particle_num=state.shape[0])
    if kind == "naive":
        return nb.NaiveSim.from_particles(sp, None, state)
    return nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(theta), state)


def _state_of(nb, sim):
    return nb.as_floats(sim.read_particles()).copy()


def _prepared(nb, kind, state, step=True):
    """The simulator and the state it holds: a TreeSim after one step, in tree order."""
    sim = _sim(nb, kind, state)
    if kind == "tree" and step and state.shape[0] > 0:
        sim.encode()
    return sim, _state_of(nb, sim)


def _raw(sim, ks, min_members=1, density_min=-math.inf, cap=None, bcap=None, call=None, handle=None, n=None, flags=0,
         want=("labels", "group_of", "density", "groups", "peak", "boundaries", "stats")):
    """The C call with every buffer pre-filled."""
    from wgpu_n_body_amd import _lib
    n = int(sim.sim_params().particle_num) if n is None else n
    cap = n + 1 if cap is None else cap
    bcap = 64 * n + 1 if bcap is None else bcap
    p = _lib.nb_hop_params()
    p.k_density, p.k_hop, p.k_merge = ks
    p.min_members, p.density_min, p.flags = min_members, density_min, flags
    labels, gof = np.full(n + 1, FILL, np.uint32), np.full(n + 1, FILL, np.uint32)
    density, peak = np.full(n + 1, -7.0), np.full(cap + 1, -7.0)
    rows = np.zeros(cap + 1, dtype=_lib.FOF_GROUP_DTYPE)
    rows["label"] = FILL
    bnd = np.zeros(bcap + 1, dtype=_lib.HOP_BOUNDARY_DTYPE)
    bnd["a"] = FILL
    st = _lib.nb_hop_stats()
    ptr = lambda name, a: a.ctypes.data if name in want else None
    rc = (call or _lib.lib().nb_sim_hop)(handle or sim._h, C.byref(p), ptr("labels", labels), ptr("group_of", gof),
                                         ptr("density", density), ptr("groups", rows), ptr("peak", peak), cap,
                                         ptr("boundaries", bnd), bcap, C.byref(st) if "stats" in want else None)
    return SimpleNamespace(rc=rc, n=n, cap=cap, bcap=bcap, labels=labels, group_of=gof, density=density, rows=rows,
                           peak=peak, bnd=bnd, st=st,
                           bytes=b"".join(a.tobytes() for a in (labels, gof, density, rows, peak, bnd)) + bytes(st))


def _hop(sim, ks, **kw):
    from wgpu_n_body_amd import _lib
    g = _raw(sim, ks, **kw)
    assert g.rc == 0, _lib.lib().nb_last_error()
    n = g.n
    assert g.labels[n] == FILL and g.group_of[n] == FILL and g.density[n] == -7.0  # n values each, no more
    return g


def _untouched(g):
    return (np.all(g.labels == FILL) and np.all(g.group_of == FILL) and np.all(g.density == -7.0)
            and np.all(g.rows["label"] == FILL) and np.all(g.peak == -7.0) and np.all(g.bnd["a"] == FILL))


def _sums_of(rows):
    return np.column_stack([rows["mass"], rows["mx"], rows["mv"], rows["mr2"], rows["mv2"]]).reshape(len(rows), 9)


def _check(g, ref, tol=TOL):
    """Every integer, label, boundary and peak density equal; every sum within tol of its sum of |term|."""
    st, n = g.st, g.n
    for f in ("n", "nonfinite", "counted", "outside", "short_of_k", "peaks", "groups", "grouped_bodies",
              "boundary_pairs", "largest_count", "largest_label"):
        assert getattr(st, f) == ref[f], (f, getattr(st, f), ref[f])
    assert st.boundaries == len(ref["boundaries"])
    assert np.array_equal(g.labels[:n], ref["labels"]), np.flatnonzero(g.labels[:n] != ref["labels"])[:8]
    assert np.array_equal(g.group_of[:n], ref["group_of"])
    assert np.array_equal(g.density[:n], ref["density"], equal_nan=True)
    rows = min(ref["groups"], g.cap)
    assert np.array_equal(g.rows["label"][:rows], ref["rows_label"][:rows])
    assert np.array_equal(g.rows["count"][:rows], ref["rows_count"][:rows])
    assert np.array_equal(g.peak[:rows], ref["peak_density"][:rows], equal_nan=True)
    assert np.all(g.rows["label"][rows:] == FILL) and np.all(g.peak[rows:] == -7.0)  # no row past the total
    err = np.abs(_sums_of(g.rows[:rows]) - ref["sums"][:rows])
    if rows:
        print("sums: error / (TOL * sum of |term|) =", (err / (tol * ref["scale"][:rows] + 1e-300)).max())
    assert np.all(err <= tol * ref["scale"][:rows])
    b = min(len(ref["boundaries"]), g.bcap)
    for f in ("a", "b", "pairs"):
        assert np.array_equal(g.bnd[f][:b], ref["boundaries"][f][:b]), f
    assert np.array_equal(g.bnd["density"][:b], ref["boundaries"]["density"][:b], equal_nan=True)
    assert not g.bnd["reserved"][:b].any() and np.all(g.bnd["a"][b:] == FILL)
    assert st.nonfinite + st.counted == st.n


def _ref(state, ks, **kw):
    return H.hop_vectorised(state, *ks, **kw)


@pytest.mark.parametrize("n", [0, 1, 2, 7, 63, 64, 65, 66, 1000])
@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_sizes(gpu, kind, n):
    """Every parameter triple against every n: the short states (c <= max k) among them."""
    nb = gpu
    state0 = K.state_of(K.ball(np.random.default_rng(n), n, 1.0), n)
    sim, state = _prepared(nb, kind, state0)
    for ks in KS:
        g = _hop(sim, ks)
        _check(g, _ref(state, ks))
        assert g.st.short_of_k == (n if n <= max(ks) else 0)
        if n <= max(ks):
            assert np.all(g.labels[:n] == H.NONE) and g.st.groups == 0 and g.st.boundaries == 0 and g.st.peaks == 0
        else:
            assert np.all(g.labels[:n] != H.NONE) and g.st.peaks >= 1
    sim.destroy()


@pytest.mark.parametrize("init", ["uniform", "disc", "spherical"])
@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_project_inits(gpu, kind, init):
    nb = gpu
    sim, state = _prepared(nb, kind, make_state(init, 4096, seed=7))
    for ks in ((32, 16, 4), (6, 6, 6)):
        g = _hop(sim, ks)
        _check(g, _ref(state, ks))
        assert g.st.peaks > 1 and g.st.boundaries > 0
    sim.destroy()


def test_lattice_where_the_index_decides(gpu):
    """Equal distances everywhere (the neighbour order) and, with equal masses, equal densities (the hop)."""
    nb = gpu
    for masses in ("unequal", "equal"):
        state = K.state_of(K.lattice(9), 1)
        if masses == "equal":
            state[:, 9] = 1.0
        sim = _sim(nb, "naive", state)
        for ks in ((6, 6, 6), (32, 16, 4), (2, 1, 1)):
            _check(_hop(sim, ks), _ref(state, ks))
        sim.destroy()


def test_coincident_zero_and_negative_masses(gpu):
    """More than k_density + 1 coincident bodies (+inf densities, ordered by the index alone); zero and negative
    masses (zero and negative densities; finite binary32 masses cannot make a NaN density, whose -inf key the
    restatements and nb_hop_regroup cover on the host)."""
    nb = gpu
    rng = np.random.default_rng(3)
    pts = np.concatenate([np.tile([(0.3, -0.2, 0.1)], (40, 1)), np.tile([(-0.5, 0.5, 0.0)], (9, 1)),
                          rng.normal(0.0, 0.5, (700, 3))])
    state = K.state_of(pts[rng.permutation(len(pts))], 3)
    state[rng.choice(len(pts), 60, replace=False), 9] = 0.0
    state[rng.choice(len(pts), 60, replace=False), 9] = -1.0
    sim = _sim(nb, "naive", state)
    for ks in ((6, 6, 6), (32, 16, 4), (8, 64, 2)):
        g = _hop(sim, ks)
        ref = _ref(state, ks)
        _check(g, ref)
        if ks[0] <= 32:
            assert np.isinf(ref["density"]).sum() >= 40
    sim.destroy()
    # masses of +1 and -1: many densities of exactly +0 and -0, which are equal in the order
    state = K.state_of(rng.normal(0.0, 0.5, (300, 3)), 4)
    state[:, 9] = np.where(np.arange(300) % 2 == 0, 1.0, -1.0)
    sim = _sim(nb, "naive", state)
    ref = _ref(state, (6, 6, 6))
    _check(_hop(sim, (6, 6, 6)), ref)
    assert (ref["density"] < 0).any() and (ref["density"] > 0).any()
    sim.destroy()


@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_nonfinite_bodies(gpu, kind):
    nb = gpu
    sim, state0 = _prepared(nb, kind, make_state("spherical", 4096, seed=5))
    sim.destroy()
    state0 = K.inject_nonfinite(state0, 40, 3)
    sim = _sim(nb, kind, state0)
    state = _state_of(nb, sim)
    ok = K.counted_mask(*K.split(state))
    g = _hop(sim, (32, 16, 4))
    _check(g, _ref(state, (32, 16, 4)))
    assert g.st.nonfinite == 40 and np.all(g.labels[:4096][~ok] == H.NONE) and np.all(g.labels[:4096][ok] != H.NONE)
    sim.destroy()


def test_density_min_and_min_members(gpu):
    nb = gpu
    state = make_state("disc", 3001, seed=2)
    sim = _sim(nb, "naive", state)
    ks = (32, 16, 4)
    full = _ref(state, ks)
    cut = float(np.quantile(full["density"], 0.4))
    g = _hop(sim, ks, density_min=cut)
    ref = _ref(state, ks, density_min=cut)
    _check(g, ref)
    assert 1000 < g.st.outside < 1400 and np.all((g.labels[:3001] == H.NONE) == (full["density"] < cut))
    # a cut at a density that occurs: the body at the cut is inside
    assert g.labels[int(np.argmin(np.where(full["density"] >= cut, full["density"], np.inf)))] != H.NONE
    g = _hop(sim, ks, density_min=math.inf)  # cuts everything (no coincident bodies here)
    _check(g, _ref(state, ks, density_min=math.inf))
    assert g.st.outside == 3001 and g.st.peaks == 0 and g.st.boundaries == 0 and np.all(g.labels[:3001] == H.NONE)
    for mm in (2, 50, 4000):
        g = _hop(sim, ks, min_members=mm)
        ref = _ref(state, ks, min_members=mm)
        _check(g, ref)
        assert g.st.peaks == full["peaks"] and g.st.boundaries == len(full["boundaries"])  # labels, not rows
        assert g.st.groups == int((full["rows_count"] >= mm).sum())
    sim.destroy()


def test_capacities_and_null_outputs(gpu):
    nb = gpu
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    n, ks = 2000, (32, 16, 4)
    state = make_state("spherical", n, seed=3)
    sim = _sim(nb, "naive", state)
    ref = _ref(state, ks)
    full = _hop(sim, ks)
    _check(full, ref)
    assert ref["groups"] > 3 and len(ref["boundaries"]) > 3
    for cap, bcap in ((0, 0), (1, 2), (3, 1), (ref["groups"], len(ref["boundaries"]))):
        g = _hop(sim, ks, cap=cap, bcap=bcap)
        _check(g, ref)  # the first min(total, capacity) rows; the stats report the totals
        assert bytes(g.st) == bytes(full.st)
    # every subset of one output
    for name in ("labels", "group_of", "density", "groups", "peak", "boundaries", "stats"):
        g = _hop(sim, ks, want=(name,))
        for other, a, b in (("labels", g.labels, full.labels), ("group_of", g.group_of, full.group_of),
                            ("density", g.density, full.density), ("groups", g.rows, full.rows),
                            ("peak", g.peak, full.peak), ("boundaries", g.bnd, full.bnd)):
            if other == name:
                assert a.tobytes() == b.tobytes(), name
            elif a.dtype.names:
                assert np.all(a[a.dtype.names[0]] == FILL), (name, other)
            else:
                assert np.all(a == (FILL if a.dtype == np.uint32 else -7.0)), (name, other)
        if name == "stats":
            assert bytes(g.st) == bytes(full.st)
    p = _lib.nb_hop_params()
    p.k_density, p.k_hop, p.k_merge, p.min_members, p.density_min = 32, 16, 4, 1, -math.inf
    assert L.nb_sim_hop(sim._h, C.byref(p), None, None, None, None, None, 0, None, 0, None) == 0
    # refused calls write nothing
    for bad in (dict(ks=(1, 16, 4)), dict(ks=(32, 0, 4)), dict(ks=(32, 16, 65)), dict(min_members=0),
                dict(density_min=math.nan), dict(flags=2)):
        kw = dict(ks=ks)
        kw.update(bad)
        g = _raw(sim, **kw)
        assert g.rc == _lib.NB_ERR_INVALID and L.nb_last_error() and _untouched(g)
        assert bytes(g.st) == bytes(_lib.nb_hop_stats())
    with pytest.raises(nb.NBodyError) as ex:
        sim.hop_groups(k_density=1)
    assert ex.value.code == _lib.NB_ERR_INVALID
    assert _hop(sim, ks).bytes == full.bytes  # the simulator stays usable
    sim.destroy()
    # a sharded simulator (rank 0 of 2)
    s = make_state("uniform", 64, seed=1)
    sharded = nb.NaiveSim.from_particles(nb.SimParams(particle_num=64), None, s, placement=nb.Placement(world=2))
    g = _raw(sharded, (6, 6, 6), n=64)
    assert g.rc == _lib.NB_ERR_UNSUPPORTED and b"sharded" in L.nb_last_error() and _untouched(g)
    sharded.destroy()
    # a several-GPU runner, both ranks on device 0
    r = nb.OfflineHeadless(nb.NaiveSim, nb.SimParams(particle_num=512), None,
                           lambda sp: nb.inits.uniform_init(sp, seed=1), device_ids=[0, 0])
    with pytest.raises(nb.NBodyError) as ex:
        r.hop_groups()
    assert ex.value.code == _lib.NB_ERR_UNSUPPORTED
    r.destroy()


@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_bitwise_reproducible_and_tuning_keys(gpu, kind):
    nb = gpu
    sim, state = _prepared(nb, kind, make_state("disc", 4097, seed=2))
    ks = (32, 16, 4)
    base = _hop(sim, ks)
    _hop(sim, (6, 6, 6))  # other parameters between
    sim.fof_groups(0.02, min_members=2)  # the catalogue's workspace is shared with it
    sim.knn_density(6)  # and the search's with this
    assert _hop(sim, ks).bytes == base.bytes
    for span in (1, 2, 5, 8):
        sim.set_tuning("knn_span_cells", span)
        assert _hop(sim, ks).bytes == base.bytes, span
    sim.set_tuning("knn_span_cells", 3)
    for per in (1, 2):
        sim.set_tuning("knn_block_queries", per)
        assert _hop(sim, ks).bytes == base.bytes, per
    sim.set_tuning("knn_block_queries", 4)
    for length in (64, 256, 65536):
        sim.set_tuning("fof_chunk_len", length)
        assert _hop(sim, ks).bytes == base.bytes, length
    sim.destroy()


def test_density_is_knn_density(gpu):
    nb = gpu
    sim = _sim(nb, "naive", make_state("spherical", 4096, seed=1))
    for kd in (2, 6, 32, 64):
        g = _hop(sim, (kd, 16, 4), want=("density",))
        d = sim.knn_density(kd, neighbours=False)
        assert g.density[:4096].tobytes() == d.density.tobytes()
    sim.destroy()


def test_a_permutation_permutes_the_partition(gpu):
    nb = gpu
    n, ks = 1500, (6, 6, 6)
    state = K.state_of(np.random.default_rng(6).normal(size=(n, 3)), 6)
    # no ties in the distances up to the 7-th neighbour, and no two equal densities: the index decides nothing
    assert K.tie_free(K.knn_vectorised(*K.split(state), 6), *K.split(state))
    assert len(np.unique(K.knn_vectorised(*K.split(state), 6).density)) == n
    perm = np.random.default_rng(4).permutation(n)  # body i of the permuted state is body perm[i]
    res = []
    for s in (state, state[perm]):
        sim = _sim(nb, "naive", s)
        res.append(_hop(sim, ks))
        sim.destroy()
    a, b = res
    assert np.array_equal(perm[b.labels[:n]], a.labels[:n][perm])  # the same peaks, renumbered
    assert fof_ref.partition(a.labels[:n]) == {frozenset(int(perm[i]) for i in s) for s in fof_ref.partition(b.labels[:n])}
    assert (a.st.peaks, a.st.boundaries, a.st.boundary_pairs) == (b.st.peaks, b.st.boundaries, b.st.boundary_pairs)
    assert sorted(a.bnd["density"][:a.st.boundaries]) == sorted(b.bnd["density"][:b.st.boundaries])


@pytest.mark.parametrize("case", ["naive", "tree"])
def test_does_not_perturb_the_trajectory(gpu, case):
    nb = gpu
    n, steps = 4096, 6
    state = make_state("uniform", n, seed=9)
    finals = []
    for with_hop in (False, True):
        sim = _sim(nb, case, state)
        for j in range(steps):
            sim.encode()
            if with_hop:
                g = sim.hop_groups(k_density=32 if j % 2 else 8, labels=j % 3 != 0, boundaries=j % 3 != 1)
                assert g.stats.step_num == j + 1 and g.stats.counted == n and g.stats.peaks > 0
        finals.append(nb.as_floats(sim.read_particles()).copy())
        sim.destroy()
    assert np.array_equal(finals[0].view(np.uint32), finals[1].view(np.uint32))


def test_python_wrapper_regroup_and_profiles(gpu):
    nb = gpu
    state = make_state("disc", 4096, seed=0)
    sim = _sim(nb, "naive", state)
    ks = (32, 16, 4)
    g = _hop(sim, ks)
    h = sim.hop_groups(k_density=32, density=True)
    G, B = g.st.groups, g.st.boundaries
    assert h.k == ks and np.array_equal(h.labels, g.labels[:4096]) and np.array_equal(h.group_of, g.group_of[:4096])
    assert h.density.tobytes() == g.density[:4096].tobytes() and h.rows.tobytes() == g.rows[:G].tobytes()
    assert h.peak_density.tobytes() == g.peak[:G].tobytes() and h.boundaries.tobytes() == g.bnd[:B].tobytes()
    assert (h.stats.groups, h.stats.boundaries, h.stats.peaks) == (G, B, g.st.peaks)
    part = sim.hop_groups(k_density=32, labels=False, boundaries=False)
    assert part.labels is None and part.density is None and part.boundaries is None and part.rows.tobytes() == h.rows.tobytes()
    # the wrapper repeats the call once when its first sizes were too small: (2, 1, 1) makes more than n / 4 groups
    many = sim.hop_groups(k_density=2, k_hop=1, k_merge=1)
    ref = _ref(state, (2, 1, 1))
    assert ref["groups"] > 4096 // 4 + 1 and len(many.rows) == ref["groups"] == many.stats.groups
    assert np.array_equal(many.label, ref["rows_label"]) and len(many.boundaries) == len(ref["boundaries"])
    # regroup: the library's against the restatement's, through the wrapper
    med = float(np.median(h.density))
    m = h.regroup(2.5 * med, 3.0 * med)
    want = H.regroup(h.rows["label"], h.rows["count"], _sums_of(h.rows), h.peak_density, [tuple(e) for e in h.boundaries],
                     2.5 * med, 3.0 * med)
    assert np.array_equal(m.label, want[1]) and np.array_equal(m.count, want[2]) and np.array_equal(_sums_of(m.rows), want[3])
    raw = h.group_of != H.NONE
    assert np.array_equal(m.labels[raw], want[0][h.group_of[raw]]) and np.all(m.labels[~raw] == H.NONE)
    assert np.array_equal(np.bincount(m.group_of[m.group_of != H.NONE], minlength=len(m.rows)), m.count)
    # group_profiles(center="peak") is halo_profiles about the labels
    kw = dict(rmin=1e-3, rmax=1.0, nbins=12)
    rows, a = sim.group_profiles(h, center="peak", **kw)
    b = sim.halo_profiles(bodies=h.label, **kw)
    assert np.array_equal(rows, np.arange(G))
    for f in a.__dataclass_fields__:
        x, y = getattr(a, f), getattr(b, f)
        if isinstance(x, np.ndarray):
            assert x.tobytes() == y.tobytes(), f
    with pytest.raises(ValueError):
        sim.group_profiles(sim.fof_groups(0.05), center="peak", **kw)
    sim.destroy()


def test_two_clumps_and_a_bridge(gpu):
    """What the feature exists for.  Two Gaussian clumps of 2048 bodies (sigma 0.3, centres 2.0 apart), 32 bodies of
    each moved onto the line between the centres: friends-of-friends at a link that catches the clumps (0.2)
    follows the line and returns one group; the density-peak groups regrouped at saddle / peak of 2.5 / 3 times the
    median density are two, one per clump.  From a CPU run of the restatement (seed 1): 28 raw groups, merged
    groups of 2050 and 2046 bodies."""
    nb = gpu
    state = H.two_clumps(1, bridge=32)
    sim = _sim(nb, "naive", state)
    ks = (32, 16, 4)
    ref = _ref(state, ks)
    _check(_hop(sim, ks), ref)
    fof = sim.fof_groups(0.2, min_members=20)
    assert len(fof.rows) == 1 and fof.count[0] > 4000
    h = sim.hop_groups(k_density=32, k_hop=16, k_merge=4, density=True)
    med = float(np.median(h.density))
    m = h.regroup(2.5 * med, 3.0 * med)
    want = H.regroup(ref["rows_label"], ref["rows_count"], ref["sums"], ref["peak_density"], ref["boundaries"],
                     2.5 * med, 3.0 * med)
    sim.destroy()
    assert len(want[1]) == 2 and len(h.rows) == ref["groups"] > 2
    assert np.array_equal(m.label, want[1]) and np.array_equal(m.count, want[2]) and m.count.sum() == 4096
    assert np.array_equal(m.peak_density, want[4])
    left = state[:, 0] < 0.0  # the clump of a body, but for a few in the middle
    side = m.labels == m.label[0]
    assert min((side == left).mean(), (side != left).mean()) < 0.01


def test_runner(gpu):
    """nb_runner_hop equals nb_sim_hop on nb_runner_sim."""
    nb = gpu
    from wgpu_n_body_amd import _lib
    runner = nb.OfflineHeadless(nb.TreeSim, nb.SimParams(particle_num=4096), nb.AddParams.TreeSimParams(0.75),
                                lambda sp: nb.inits.disc_init(sp, seed=0))
    for _ in range(2):
        runner.step()
    ks = (32, 16, 4)
    via_runner = _raw(None, ks, call=_lib.lib().nb_runner_hop, handle=runner._h, n=4096)
    via_sim = _raw(runner.sim, ks)
    o = runner.hop_groups(k_density=32)
    state = _state_of(nb, runner.sim)
    runner.destroy()
    assert via_runner.rc == via_sim.rc == 0 and via_runner.bytes == via_sim.bytes
    _check(via_sim, _ref(state, ks))
    assert np.array_equal(o.labels, via_sim.labels[:4096]) and o.stats.step_num == 2


def test_cli_and_cpp_mirror(gpu):
    """headless --hop (the C++ mirror over nb_runner_hop and nb_hop_regroup) prints what the Python runner returns."""
    nb = gpu
    runner = nb.OfflineHeadless(nb.TreeSim, nb.SimParams(particle_num=4096), nb.AddParams.TreeSimParams(0.75),
                                lambda sp: nb.inits.disc_init(sp, seed=0))
    o = runner.hop_groups(k_density=32, k_hop=16, k_merge=4, min_members=3, density=True)  # the seeded init, no step yet
    runner.destroy()
    med = float(np.median(o.density))
    saddle, peak = 2.5 * med, 3.0 * med
    m = o.regroup(saddle, peak)
    cli = os.path.join(ROOT, "wgpu_n_body_amd", "headless")
    cmd = [cli, "--sim", "tree", "--n", "4096", "--init", "disc", "--steps", "2", "--hop", "2", "--hop-k", "32,16,4",
           "--hop-min", "3", "--hop-top", "3", "--hop-saddle", repr(saddle), "--hop-peak", repr(peak)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    out = [ln.split() for ln in p.stdout.splitlines()]
    hop = [ln for ln in out if ln and ln[0] == "hop"]
    merged = [ln for ln in out if ln and ln[0] == "hop_merged"]
    assert len(hop) == len(merged) == 2 and [int(ln[1]) for ln in hop] == [0, 2]
    assert len([ln for ln in p.stdout.splitlines() if ln.startswith("Step Duration: ")]) == 2
    st = o.stats
    assert [int(x) for x in hop[0][1:]] == [0, st.peaks, st.groups, st.grouped_bodies, st.largest_count, st.boundaries,
                                            st.boundary_pairs]
    assert [int(x) for x in merged[0][1:]] == [0, m.stats.groups, m.stats.grouped_bodies, m.stats.largest_count]
    for tag, g in (("hop_group", o), ("hop_merged_group", m)):
        lines = [ln for ln in out if ln and ln[0] == tag and ln[1] == "0"]
        order = g.by_size()[:3]
        assert len(lines) == len(order) > 0
        for ln, r in zip(lines, order):
            assert [int(x) for x in ln[2:5]] == [r, g.label[r], g.count[r]]
            want = [g.mass[r], *g.com[r], g.peak_density[r]]
            assert ln[5:] == ["%.9e" % x for x in want]
    # the pairs of options that go together
    p = subprocess.run(cmd[:-2], capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "go together" in p.stderr
