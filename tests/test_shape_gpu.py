"""nb_sim_group_shapes on the device (csrc/nb_shape.hip) against the numpy restatement of its rule
(tests/shape_ref.py): the integers (count, selected, iterations, status, selected_of, the stats) equal --
tests/test_shape.py shows that no case used here has a marginal decision -- every sum within 1e-10 of its sum of
|term|, lambda, q and s within 1e-9 relative, the axes within 1e-9 where the eigenvalues are apart.  Tiny states,
every run, chunk and table border, different fates in one call, the other kinds of member, device-formed centres,
bitwise independence of the other rows, of the rows' order, of the chunk length and of the call, the refusals, null
outputs, that a call perturbs neither the trajectory nor the passes that follow; the wrappers, the runner, the C++
mirror and the CLI.  `-m gpu`."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from tests import shape_ref as S
from tests.helpers import ROOT

pytestmark = pytest.mark.gpu

TOL_SUM = 1e-10     # of the sum of |term|
TOL_EIGEN = 1e-9    # lambda, q, s relative; 1 - |e . e_ref|
GAP = 1e-3          # axes are compared where the eigenvalues are further apart than this, in lambda_1
FILL = 0xDEADBEEF
G, E, DT = 1e-6, 1e-4, 0.016
INTS = ("count", "selected", "iterations", "status")
STATS = ("n", "rows", "members", "nonfinite_members", "converged", "unconverged", "degenerate", "empty", "rounds_max")
SUM_FIELDS = ("mass", "md", "mu", "t", "uu", "j")


def _sim(nb, kind, state, theta=0.75):
    sp = nb.SimParams(particle_num=state.shape[0], g=G, e=E, dt=DT)
    if kind == "naive":
        return nb.NaiveSim.from_particles(sp, None, state)
    return nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(theta), state)


def _raw(sim, gof, m, centers=None, velocities=None, radius=None, reduced=False, max_iter=32, tol=1e-3, min_members=10,
         step_num=None, call=None, handle=None, n=None, outputs=("rows", "sel", "st")):
    """The C call with every buffer pre-filled."""
    from wgpu_n_body_amd import _lib
    n = int(sim.sim_params().particle_num) if n is None else n
    p = _lib.nb_shape_params()
    p.flags = _lib.NB_SHAPE_REDUCED if reduced else 0
    p.min_members, p.max_iter, p.tol = min_members, max_iter, tol
    p.step_num = _lib.NB_SHAPE_ANY_STEP if step_num is None else step_num
    arr = lambda a, w: None if a is None else np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1, w))
    centers, velocities, radius = arr(centers, 3), arr(velocities, 3), arr(radius, 1)
    gof = None if gof is None else np.ascontiguousarray(gof, np.uint32)
    rows = np.zeros(m + 1, _lib.SHAPE_GROUP_DTYPE)
    rows["count"] = FILL
    sel = np.full(n + 1, FILL, np.uint32)
    st = _lib.nb_shape_stats()
    st.reserved = 77
    ptr = lambda a: a.ctypes.data if a is not None else None
    rc = (call or _lib.lib().nb_sim_group_shapes)(
        handle or sim._h, C.byref(p), ptr(gof), m, ptr(centers), ptr(velocities), ptr(radius),
        rows.ctypes.data if "rows" in outputs else None, sel.ctypes.data if "sel" in outputs else None,
        C.byref(st) if "st" in outputs else None)
    return SimpleNamespace(rc=rc, rows=rows, sel=sel, st=st, m=m, n=n,
                           bytes=rows.tobytes() + sel.tobytes() + bytes(st))


def _shapes(sim, gof, m, **kw):
    from wgpu_n_body_amd import _lib
    g = _raw(sim, gof, m, **kw)
    assert g.rc == 0, _lib.lib().nb_last_error()
    assert g.rows["count"][m] == FILL and g.sel[g.n] == FILL  # nothing past the end
    return g


def _flat(rows):
    return np.concatenate([rows[f].reshape(len(rows), int(np.prod(rows[f].shape[1:]))) for f in SUM_FIELDS], axis=1)


def _check(g, ref, worst=None):
    """Every integer equal, every sum within its tolerance, the eigen-system within its own."""
    for k in STATS:
        assert getattr(g.st, k) == ref["stats"][k], (k, getattr(g.st, k), ref["stats"][k])
    rows, want = g.rows[:g.m], ref["rows"]
    for f in INTS:
        assert np.array_equal(rows[f], want[f]), (f, rows[f], want[f])
    assert np.array_equal(g.sel[:g.n], ref["selected_of"]), np.flatnonzero(g.sel[:g.n] != ref["selected_of"])[:8]
    if g.m == 0:
        return {}
    for f in ("radius", "center", "velocity"):
        assert np.array_equal(rows[f], want[f], equal_nan=True), f
    d = np.abs(_flat(rows) - _flat(want))
    bound = TOL_SUM * ref["scale"]
    assert np.all(d <= bound + 1e-300), float((d / (bound + 1e-300)).max())
    ratios = dict(sums=float((d / (bound / TOL_SUM + 1e-300)).max()), eigen=0.0, axes=0.0)
    for f in ("lambda", "axes", "q", "s"):
        assert np.array_equal(np.isnan(rows[f]), np.isnan(want[f])), f
    for r in range(g.m):
        lam, wlam = rows["lambda"][r], want["lambda"][r]
        if np.isnan(wlam).any():
            continue
        assert np.all(np.abs(lam - wlam) <= TOL_EIGEN * np.abs(wlam[0])), (r, lam, wlam)
        ratios["eigen"] = max(ratios["eigen"], float(np.abs(lam - wlam).max() / max(abs(wlam[0]), 1e-300)))
        if want["status"][r] in (S.CONVERGED, S.UNCONVERGED):
            for f in ("q", "s"):
                err = abs(rows[f][r] - want[f][r]) / want[f][r]
                assert err <= TOL_EIGEN, (r, f)
                ratios["eigen"] = max(ratios["eigen"], float(err))
            e, we = rows["axes"][r].reshape(3, 3), want["axes"][r].reshape(3, 3)
            gaps = (wlam[0] - wlam[1], min(wlam[0] - wlam[1], wlam[1] - wlam[2]), wlam[1] - wlam[2])
            for k in range(3):
                if gaps[k] > GAP * wlam[0]:
                    miss = 1.0 - abs(e[k] @ we[k])
                    assert miss <= TOL_EIGEN, (r, k, miss)
                    ratios["axes"] = max(ratios["axes"], float(miss))
    if worst is not None:
        for k, v in ratios.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("worst ratios:", ratios)
    return ratios


def _ref_with_device_centres(g, state, gof, m, kw):
    """The reference about the centres and velocities the device used (the test of the centres holds them to the
    reference's own): explicit ones are the same values, device-formed ones are what round 0 gave."""
    kw = dict(kw)
    kw["centers"], kw["velocities"] = g.rows["center"][:m].copy(), g.rows["velocity"][:m].copy()
    return S.shape_ref(state, gof, m, **kw)


def _run_case(nb, name, kind="naive", chunk=None):
    state, gof, m, kw = S.case(name)
    sim = _sim(nb, kind, state)
    if chunk:
        sim.set_tuning("shape_chunk_len", chunk)
    g = _shapes(sim, gof, m, **kw)
    ref = _ref_with_device_centres(g, state, gof, m, kw)
    assert not ref["marginal"].any()
    return sim, g, ref


@pytest.mark.parametrize("n", [0, 1, 2])
@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_tiny_states(gpu, kind, n):
    rng = np.random.default_rng(3)
    state = S.cloud(rng, 2)[:n]
    sim = _sim(gpu, kind, state)
    none = np.full(n, S.NONE, np.uint32)
    for gof, m in ((none, 0), (none, 1), (np.zeros(n, np.uint32), 1), (np.arange(n, dtype=np.uint32), max(n, 1))):
        for kw in (dict(min_members=1), dict(min_members=1, centers=np.zeros((m, 3)), velocities=np.zeros((m, 3)),
                                            radius=np.full(m, 2.0), reduced=True)):
            g = _shapes(sim, gof if n else None, m, **kw)
            _check(g, S.shape_ref(state, gof, m, **kw))
            if m and np.all(gof == S.NONE):
                assert g.rows["status"][0] == S.EMPTY and g.st.empty == m and g.st.members == 0


def test_every_run_border_in_one_call(gpu):
    """Rows of 1, 2, 3, 4, 63, 64, 65, 255, 256, 257 and 1,025 members, R = +inf, centres formed on the device."""
    _, g, ref = _run_case(gpu, "sizes")
    assert sorted(g.rows["count"][:g.m].tolist()) == sorted(S.SIZES)
    _check(g, ref)


def test_one_row_over_many_chunks(gpu):
    """5,000 members with "shape_chunk_len" 64: 79 work items of one run each, the last one partial."""
    _, g, ref = _run_case(gpu, "big", chunk=64)
    assert g.rows["count"][0] == 5000 and g.rows["iterations"][0] >= 2
    _check(g, ref)


@pytest.mark.parametrize("kind", ["naive", "tree"])
@pytest.mark.parametrize("name", ["mixed", "mixed_reduced"])
def test_against_the_reference(gpu, kind, name):
    """Converged after 2 rounds and after 20, unconverged, degenerate, empty and R = +inf in one call."""
    _, g, ref = _run_case(gpu, name, kind)
    if name == "mixed":
        assert g.rows["status"][:g.m].tolist() == [1, 1, 1, 4, 1, 8, 2] and g.rows["iterations"][2] >= 10
    _check(g, ref)


def test_other_members(gpu):
    """Non-finite members are counted apart, tracers take part in the count and add nothing, a body at the centre
    adds nothing to the reduced tensor."""
    state, gof, m, kw = S.case("members")
    _, g, ref = _run_case(gpu, "members")
    assert g.st.nonfinite_members == 3 and g.st.members == 597
    assert np.all(g.sel[:g.n][~S.body_ok(state)] == S.NONE)
    assert np.all(np.isfinite(_flat(g.rows[:m])))
    _check(g, ref)


@pytest.mark.parametrize("name", ["sizes", "mixed"])
def test_device_centres(gpu, name):
    """Round 0's centre and velocity are the reference's within 1e-10 of sum |m x| / M; a call with them as explicit
    centres returns the same bits, and so does one that gives only one of the two."""
    state, gof, m, kw = S.case(name)
    sim = _sim(gpu, "naive", state)
    g = _shapes(sim, gof, m, **kw)
    c, v, c_scale, v_scale = S.round0(state, gof, m)
    has = ~np.isnan(c[:, 0])
    assert np.array_equal(np.isnan(g.rows["center"][:m, 0]), ~has)
    assert np.all(np.abs(g.rows["center"][:m][has] - c[has]) <= 1e-10 * c_scale[has])
    assert np.all(np.abs(g.rows["velocity"][:m][has] - v[has]) <= 1e-10 * v_scale[has] + 1e-300)
    cc = np.where(has[:, None], g.rows["center"][:m], 0.0)
    vv = np.where(has[:, None], g.rows["velocity"][:m], 0.0)
    for kw2 in (dict(centers=cc, velocities=vv), dict(centers=cc), dict(velocities=vv)):
        again = _shapes(sim, gof, m, **dict(kw, **kw2))
        a, b = again.rows[:m][has], g.rows[:m][has]
        assert a.tobytes() == b.tobytes()
        assert np.array_equal(again.sel, g.sel)


@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_rows_are_independent_bit_for_bit(gpu, kind):
    """A row's bits do not depend on the call, the chunk length, the row's number or the other rows."""
    state, gof, m, kw = S.case("mixed_reduced")
    sim = _sim(gpu, kind, state)
    if kind == "tree":  # a stepped TreeSim has reordered its bodies: the assignment follows them by position
        sim.encode()
        now = gpu.as_floats(sim.dest_particle_slice())[:, 0:3].astype(np.float64)
        centres = np.array([(4, 0, 0), (0, 6, 0), (0, 0, -7), (-8, 0, 0), (9, 9, 0), (-3, -3, 3), (50, 0, 0)], float)
        row_at = np.array([0, 1, 2, 3, 4, 6, S.NONE], np.uint32)  # (the clouds of the case, and the loose bodies)
        gof = row_at[np.argmin(((now[:, None, :] - centres[None]) ** 2).sum(axis=2), axis=1)]
        kw = dict(kw, step_num=1)
    first = _shapes(sim, gof, m, **kw)
    assert first.st.converged + first.st.unconverged >= 4
    assert _shapes(sim, gof, m, **kw).bytes == first.bytes
    for chunk in (64, 1024, 65536):
        sim.set_tuning("shape_chunk_len", chunk)
        assert _shapes(sim, gof, m, **kw).bytes == first.bytes, chunk
    sim.set_tuning("shape_chunk_len", 1024)
    # the rows permuted
    perm = np.random.default_rng(8).permutation(m)  # new row k is old row perm[k]
    inverse = np.argsort(perm).astype(np.uint32)
    gof2 = np.where(gof == S.NONE, S.NONE, inverse[np.minimum(gof, m - 1)]).astype(np.uint32)
    kw2 = dict(kw, radius=np.asarray(kw["radius"])[perm])
    moved = _shapes(sim, gof2, m, **kw2)
    assert moved.rows[:m].tobytes() == first.rows[:m][perm].tobytes()
    sel = np.where(first.sel[:-1] == S.NONE, S.NONE, inverse[np.minimum(first.sel[:-1], m - 1)])
    assert np.array_equal(moved.sel[:-1], sel)
    # every other row replaced: row 1 alone, as row 0 of one row, the other bodies in no row
    alone = np.where(gof == 1, 0, S.NONE).astype(np.uint32)
    one = _shapes(sim, alone, 1, **dict(kw, radius=[np.asarray(kw["radius"])[1]]))
    assert one.rows[:1].tobytes() == first.rows[1:2].tobytes()
    # ... and with the others regrouped into different rows
    other = np.where(gof == 1, 1, np.where(gof == S.NONE, 0, 2)).astype(np.uint32)
    three = _shapes(sim, other, 3, **dict(kw, radius=[5.0, np.asarray(kw["radius"])[1], 7.0]))
    assert three.rows[1:2].tobytes() == first.rows[1:2].tobytes()


def test_refusals(gpu):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    state, gof, m, kw = S.case("mixed")
    sim = _sim(gpu, "tree", state)

    def refused(word, code=_lib.NB_ERR_INVALID, **over):
        args = dict(kw, **over)
        g = _raw(sim, args.pop("gof", gof), args.pop("m", m), **args)
        assert g.rc == code, (word, g.rc)
        assert word in L.nb_last_error(), (word, L.nb_last_error())
        assert np.all(g.rows["count"] == FILL) and np.all(g.sel == FILL) and g.st.reserved == 77  # untouched

    bad = gof.copy()
    bad[11] = m
    bad[40] = 0xFFFFFFFE
    refused(b"group_of[11]", gof=bad)
    refused(b"null group_of", gof=None)
    refused(b"rows", m=len(state) + 1, radius=None)
    refused(b"REDUCED", reduced=True)  # R = +inf in row 4
    refused(b"REDUCED", reduced=True, radius=None)
    refused(b"max_iter", max_iter=0)
    refused(b"max_iter", max_iter=65)
    for tol in (0.0, -1.0, float("nan"), float("inf")):
        refused(b"tol", tol=tol)
    refused(b"min_members", min_members=0)
    for r in (0.0, -1.0, float("nan")):
        refused(b"radius[2]", radius=[1.0, 1.0, r, 1.0, 1.0, 1.0, 1.0])
    c = np.zeros((m, 3))
    c[3, 1] = np.inf
    refused(b"row 3", centers=c)
    refused(b"row 3", velocities=c)
    assert _raw(sim, gof, m, step_num=0, **kw).rc == 0
    sim.encode()
    refused(b"step", step_num=0)
    assert _raw(sim, np.full(len(state), S.NONE, np.uint32), m, step_num=1, **kw).rc == 0
    # the simulator is still usable, and a sharded one is refused as such
    assert _raw(sim, np.full(len(state), S.NONE, np.uint32), m, **kw).rc == 0
    sp = gpu.SimParams(particle_num=len(state), g=G, e=E, dt=DT)
    shard = gpu.NaiveSim.from_particles(sp, None, state, placement=gpu.Placement(world=2))
    n_shard = int(shard.sim_params().particle_num)
    g = _raw(shard, np.full(n_shard, S.NONE, np.uint32), 1, n=n_shard)
    assert g.rc == _lib.NB_ERR_UNSUPPORTED and b"sharded" in L.nb_last_error()
    assert np.all(g.rows["count"] == FILL) and np.all(g.sel == FILL)


def test_null_outputs(gpu):
    """Every output pointer null in turn: the others are what the full call returns."""
    state, gof, m, kw = S.case("mixed")
    sim = _sim(gpu, "naive", state)
    full = _shapes(sim, gof, m, **kw)
    for outputs in (("sel", "st"), ("rows", "st"), ("rows", "sel"), ("st",), ()):
        g = _shapes(sim, gof, m, outputs=outputs, **kw)
        if "rows" in outputs:
            assert g.rows.tobytes() == full.rows.tobytes()
        else:
            assert np.all(g.rows["count"] == FILL)
        assert np.array_equal(g.sel, full.sel) if "sel" in outputs else np.all(g.sel == FILL)
        assert bytes(g.st)[:72] == bytes(full.st)[:72] if "st" in outputs else g.st.reserved == 77


@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_a_call_does_not_perturb_the_trajectory(gpu, kind):
    state, gof, m, kw = S.case("mixed")
    a, b = _sim(gpu, kind, state), _sim(gpu, kind, state)
    _shapes(a, gof, m, **kw)
    for _ in range(3):
        a.encode()
        b.encode()
    _shapes(a, np.full(len(state), S.NONE, np.uint32), m, **kw)
    assert a.dest_particle_slice().tobytes() == b.dest_particle_slice().tobytes()


@pytest.mark.parametrize("shapes_first", [True, False])
def test_a_call_does_not_disturb_the_group_finders(gpu, shapes_first):
    """nb_sim_fof and nb_sim_bound return the same bits before and after a shapes call, whichever pass makes its
    workspace first."""
    state, gof, m, kw = S.case("mixed")
    plain = _sim(gpu, "naive", state)
    want_fof = plain.fof_groups(0.3, min_members=20)
    want_bound = plain.bound_groups(0.3, min_members=20, max_iter=4)
    sim = _sim(gpu, "naive", state)
    if not shapes_first:
        sim.fof_groups(0.3, min_members=20)
        sim.bound_groups(0.3, min_members=20, max_iter=4)
    first = _shapes(sim, gof, m, **kw)
    fof = sim.fof_groups(0.3, min_members=20)
    bound = sim.bound_groups(0.3, min_members=20, max_iter=4)
    assert fof.rows.tobytes() == want_fof.rows.tobytes() and np.array_equal(fof.group_of, want_fof.group_of)
    assert bound.rows.tobytes() == want_bound.rows.tobytes() and np.array_equal(bound.bound_of, want_bound.bound_of)
    assert _shapes(sim, gof, m, **kw).bytes == first.bytes


def _clumps():
    """Five triaxial clumps and a thin background, the indices shuffled: what the group finders are given."""
    rng = np.random.default_rng(77)
    parts = [S.cloud(rng, k, axes=(0.1, 0.06, 0.04), rot=S.rotation(rng), centre=c, sigma_v=0.002, omega=(0, 0, 0.05))
             for k, c in zip((900, 500, 300, 200, 120), ((0, 0, 0), (3, 0, 0), (0, 3, 0), (0, 0, 3), (3, 3, 3)))]
    back = S.cloud(rng, 200, axes=(4.0, 4.0, 4.0), kind="uniform", centre=(1.5, 1.5, 1.5))
    state = np.concatenate(parts + [back])
    return np.ascontiguousarray(state[rng.permutation(len(state))])


def test_wrappers_equal_the_raw_call(gpu):
    """group_shapes over a FofGroups, a BoundGroups' bound sets and a regrouped HopGroups about its peaks; shapes_of;
    the runner."""
    nb = gpu
    state = _clumps()
    sim = _sim(nb, "tree", state)
    sim.encode()
    n = len(state)
    fof = sim.fof_groups(0.05, min_members=20)
    assert len(fof.rows) == 5
    got = sim.group_shapes(fof, radius=("rms", 2.0), per_body=True)
    raw = _shapes(sim, fof.group_of, 5, centers=fof.com, velocities=fof.velocity, radius=2.0 * fof.rms_radius,
                  step_num=1)
    assert got.rows.tobytes() == raw.rows[:5].tobytes() and np.array_equal(got.selected_of, raw.sel[:n])
    assert got.stats.converged == 5 and got.stats.step_num == 1 and np.array_equal(got.catalogue_rows, np.arange(5))
    assert np.all(got.b_over_a < 0.9) and np.all(got.c_over_a < got.b_over_a) and np.all(got.triaxiality > 0)
    assert np.allclose(np.linalg.norm(got.major_axis, axis=1), 1.0) and got.sigma_tensor.shape == (5, 3, 3)
    assert np.all(got.misalignment >= 0) and np.all(np.isfinite(got.spin_bullock(G)))
    assert np.allclose(np.linalg.norm(got.spin_axis, axis=1), 1.0)

    bound = sim.bound_groups(0.05, min_members=20)
    got = sim.group_shapes(bound, members="bound", radius=0.3, reduced=True)
    rows = got.catalogue_rows
    assert len(rows) >= 1
    renumber = np.full(len(bound.rows) + 1, S.NONE, np.uint32)
    renumber[rows] = np.arange(len(rows))
    assign = renumber[np.minimum(bound.bound_of, len(bound.rows))]
    raw = _shapes(sim, assign, len(rows), centers=bound.com[rows], velocities=bound.velocity[rows],
                  radius=np.full(len(rows), 0.3), reduced=True, step_num=1)
    assert got.rows.tobytes() == raw.rows[:len(rows)].tobytes() and got.selected_of is None

    got = sim.group_shapes(bound, members="bound", center="most_bound", radius=0.3)
    rows = got.catalogue_rows
    assert np.array_equal(rows, np.flatnonzero(bound.rows["most_bound"] != S.NONE)) and len(rows) >= 1
    renumber[:] = S.NONE
    renumber[rows] = np.arange(len(rows))
    parts = sim.dest_particle_slice()
    at = bound.rows["most_bound"][rows]
    raw = _shapes(sim, renumber[np.minimum(bound.bound_of, len(bound.rows))], len(rows),
                  centers=parts["position"][at].astype(np.float64), velocities=parts["velocity"][at].astype(np.float64),
                  radius=np.full(len(rows), 0.3), step_num=1)
    assert got.rows.tobytes() == raw.rows[:len(rows)].tobytes()

    hop = sim.hop_groups(k_density=32, k_hop=16, k_merge=4, min_members=20, density=True)
    merged = hop.regroup(saddle=float(np.median(hop.density)) * 2.0, peak=float(np.median(hop.density)) * 4.0)
    assert len(merged.rows) >= 1
    got = sim.group_shapes(merged, center="peak", radius=0.25)
    parts = sim.dest_particle_slice()
    peaks = merged.rows["label"]
    raw = _shapes(sim, merged.group_of, len(peaks), centers=parts["position"][peaks].astype(np.float64),
                  velocities=parts["velocity"][peaks].astype(np.float64), radius=np.full(len(peaks), 0.25), step_num=1)
    assert got.rows.tobytes() == raw.rows[:len(peaks)].tobytes()

    got = sim.shapes_of(fof.group_of, 5, radius=0.2, step_num=1)
    raw = _shapes(sim, fof.group_of, 5, radius=np.full(5, 0.2), step_num=1)
    assert got.rows.tobytes() == raw.rows[:5].tobytes()
    with pytest.raises(nb.NBodyError):
        sim.encode()
        sim.group_shapes(fof)  # a catalogue of the step before
    assert len(sim.group_shapes(fof, check_step=False).rows) == 5


def test_runner_cpp_mirror_and_cli(gpu):
    """nb_runner_group_shapes equals nb_sim_group_shapes on nb_runner_sim, and headless --shapes (the C++ mirror over
    nb_runner_fof and nb_runner_group_shapes) prints what the Python runner returns."""
    nb = gpu
    from wgpu_n_body_amd import _lib
    sp = nb.SimParams(particle_num=4096, g=1e-4, e=E, dt=DT)
    runner = nb.OfflineHeadless.new(nb.TreeSim, sp, nb.AddParams.TreeSimParams(0.75), nb.inits.disc_init)
    held = nb.Simulator(_lib.lib().nb_runner_sim(runner._h), borrowed=True)
    link, k_rms = 0.02, 1.5
    fof = runner.fof_groups(link, min_members=20)
    assert len(fof.rows) >= 2
    via_runner = runner.group_shapes(fof, radius=("rms", k_rms))
    via_sim = held.group_shapes(fof, radius=("rms", k_rms))
    assert via_runner.rows.tobytes() == via_sim.rows.tobytes()
    raw = _raw(None, fof.group_of, len(fof.rows), centers=fof.com, velocities=fof.velocity,
               radius=k_rms * fof.rms_radius, min_members=10, step_num=0,
               call=_lib.lib().nb_runner_group_shapes, handle=runner._h, n=4096)
    assert raw.rc == 0 and raw.rows[:len(fof.rows)].tobytes() == via_runner.rows.tobytes()

    exe = os.path.join(ROOT, "wgpu_n_body_amd", "headless")
    out = subprocess.run([exe, "--sim", "tree", "--n", "4096", "--init", "disc", "--g", "1e-4", "--steps", "0",
                          "--shapes", "1", "--shapes-link", str(link), "--shapes-min", "20", "--shapes-radius",
                          str(k_rms), "--shapes-top", "3"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("shape")]
    st = via_runner.stats
    assert lines[0] == ["shapes", "0", str(st.rows), str(st.converged), str(st.unconverged), str(st.degenerate),
                        str(st.empty), str(st.rounds_max)]
    order = fof.by_size()[:3]
    assert len(lines) == 1 + len(order)
    j = via_runner.angular_momentum
    jn = np.sqrt(j[:, 0] * j[:, 0] + j[:, 1] * j[:, 1] + j[:, 2] * j[:, 2])  # (the order of GroupShapes::j_norm)
    for ln, r in zip(lines[1:], order):
        row = via_runner.rows[r]
        assert ln[:5] == ["shape_group", "0", str(r), str(row["count"]), str(row["selected"])]
        got = np.array([float(x) for x in ln[5:9]])
        want = np.array([row["q"], row["s"], via_runner.triaxiality[r], jn[r]])
        assert np.array_equal(got, want, equal_nan=True), (got, want)  # %.17g round-trips
        assert ln[9] == str(row["status"])
