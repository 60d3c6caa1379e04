"""nb_orbit_sections_sim on the device (the orbit unit of csrc/nb_field.hip): every double and integer of the
tracks, crossings, counts and summaries against a host replay of the rule (tests/section_ref.py) whose accelerations
are the same simulator's field(); the tracks against orbits(); determinism, permutation and bands; the exact
continuation; non-finite tracers, no bodies, no room; jacobi_launch; the runner, the refusals that need a simulator,
the status words, the untouched trajectory and the CLI.  `-m gpu`."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import orbit_ref as R
from tests import section_ref as S
from tests.helpers import ROOT, make_state

pytestmark = pytest.mark.gpu

STEPS = 48
AXIS = (1.0, 2.0, 3.0)
CENTER = (0.1, -0.2, 0.05)
NORMAL = (0.6, 0.8, 0.3)  # no axis of the frame, and no unit vector
OFFSET = 0.05
SUMMARY_FIELDS = S.SUMMARY.names


def _sim(nb, kind, state, theta=0.75, **params):
    sp = nb.SimParams(particle_num=state.shape[0], **params)
    if kind == "naive":
        return nb.NaiveSim.from_particles(sp, None, state)
    return nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(theta), state)


def _state(n, seed):
    if n == 1:
        s = np.zeros((1, 10), np.float32)
        s[0, 0:3], s[0, 9] = (0.25, -0.5, 0.125), 3e5
        return s
    return make_state("disc" if seed % 2 else "uniform", n, seed=seed)


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def _tracers(state, m, seed):
    """m tracers in the bodies' box with velocities of the size of the box per unit time; the first on a body.  From
    m = 4 on, three are laid on the frame's axis, where the turning of the pattern does not move them:
      1  at rest, far out on the axis and far from the plane: no crossing;
      2  far below the plane, moving up along the axis so fast that the bodies hardly deflect it (N . eta = 6, against
         the |omega| |xi| of the little it is pushed off the axis): one up-crossing, at t = 2.4;
      3  far above the plane, moving down likewise: one down-crossing."""
    rng = np.random.default_rng(seed)
    lo, hi = state[:, 0:3].min(0) - 0.5, state[:, 0:3].max(0) + 0.5
    pos = rng.uniform(lo, hi, size=(m, 3))
    vel = rng.normal(size=(m, 3)) * 0.5
    pos[0] = state[rng.integers(0, state.shape[0]), 0:3]
    if m >= 4:
        n, c = _unit(AXIS), np.asarray(CENTER)
        pos[1], vel[1] = c + 50.0 * n, 0.0
        pos[2], vel[2] = c - 48.0 * n, 20.0 * n
        pos[3], vel[3] = c + 48.0 * n, -20.0 * n
    return pos, vel


def _lib_phase(omega, dt, k):
    from wgpu_n_body_amd import _lib
    c, s = C.c_double(), C.c_double()
    assert _lib.lib().nb_orbit_phase(omega, dt, k, C.byref(c), C.byref(s)) == 0
    return c.value, s.value


def _same(a, b):
    """Bit for bit where finite, NaN where NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb_ = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb_) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb_])


def _same_summary(a, b):
    return all(_same(a[f], b[f]) if a[f].dtype.kind == "f" else np.array_equal(a[f], b[f]) for f in SUMMARY_FIELDS)


def _same_sections(a, b, tracks=True):
    """Two OrbitSections, every bit."""
    ok = (np.array_equal(a.count, b.count) and np.array_equal(a.stored, b.stored) and _same(a.xi, b.xi)
          and _same(a.eta, b.eta) and _same(a.time, b.time) and np.array_equal(a.step, b.step)
          and _same_summary(a.summary, b.summary))
    if tracks:
        ok = ok and _same_tracks(a.orbits, b.orbits)
    return ok


def _same_tracks(a, b):
    return (_same(a.pos, b.pos) and _same(a.vel, b.vel) and _same(a.potential, b.potential)
            and _same(a.energy, b.energy) and np.array_equal(a.coincident, b.coincident))


def _replay(nb, sim, pos, vel, **kw):
    """The rule on the host around the simulator's own field(): phases from nb_orbit_phase, frame from
    nb_map_frame."""
    coupling = kw.pop("coupling", "field")
    scale = {"field": 1.0, "step": float(sim.sim_params().dt)}[coupling]
    return S.sections(R.device_field(sim), pos, vel, accel_scale=scale, phase=_lib_phase, frame=nb.map_frame(kw["axis"]),
                      **kw)


def _assert_is_replay(o, ref, what):
    for name in ("pos", "vel", "potential", "energy"):
        assert _same(getattr(o.orbits, name), ref[name]), (name, what)
    assert np.array_equal(o.orbits.coincident, ref["coincident"]), what
    assert np.array_equal(o.orbits.step, ref["step"]), what
    assert np.array_equal(o.count, ref["counts"]), (what, o.count, ref["counts"])
    cr = ref["crossings"]
    for name in ("xi", "eta", "time"):
        assert _same(getattr(o, name), cr[name]), (name, what)
    assert np.array_equal(o.step, cr["step"]), what
    for f in SUMMARY_FIELDS:
        a, b = o.summary[f], ref["summaries"][f]
        assert _same(a, b) if a.dtype.kind == "f" else np.array_equal(a, b), (f, what, a, b)


# ---- 1. replay, bit for bit --------------------------------------------------------------------
CASES = [("naive", n, m) for n in (1, 257, 4099) for m in (1, 65, 257)] + [("tree", 257, 65), ("tree", 4099, 257)]
# omega dt steps = 19.2 = 3.06 turns: every finite tracer off the axis crosses about three times each way by the
# frame's turning alone.  "step" multiplies the acceleration by dt = 0.016: longer steps, so that the tracers still turn
OPTIONS = [dict(omega=0.0, energy=False, coupling="field", dt=0.1), dict(omega=4.0, energy=True, coupling="field", dt=0.1),
           dict(omega=0.8, energy=False, coupling="step", dt=0.5), dict(omega=0.0, energy=True, coupling="step", dt=0.5)]


def _case(nb, idx):
    kind, n, m = CASES[idx]
    sim = _sim(nb, kind, _state(n, seed=20 + idx))
    if kind == "tree":
        for _ in range(3):  # the state read_particles returns, in the tree's order
            sim.encode()
    state = nb.as_floats(sim.read_particles())
    pos, vel = _tracers(state, m, seed=idx)
    return sim, pos, vel


def _case_kw(idx, j):
    opt = dict(OPTIONS[(idx + 2 * j + (idx // 4)) % 4])  # (j = 0, 1: one of the two turns)
    return dict(steps=STEPS, every=(48, 5)[j], max_crossings=2, normal=NORMAL, offset=OFFSET,
                direction=(idx + j) % 3 - 1, axis=AXIS, center=CENTER, **opt)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[f"{k}-n{n}-m{m}" for k, n, m in CASES])
def test_replay_bit_for_bit(gpu, idx):
    nb = gpu
    kind, n, m = CASES[idx]
    sim, pos, vel = _case(nb, idx)
    for j in range(2):
        kw = _case_kw(idx, j)
        o = sim.orbit_sections(pos, vel, **kw)
        ref = _replay(nb, sim, pos, vel, **kw)
        records = 2 if j == 0 else 11
        assert o.orbits.pos.shape == (records, m, 3) and o.xi.shape == (m, 2, 3) and o.time.shape == (m, 2)
        _assert_is_replay(o, ref, kw)
        # the lists: the first min(count, 2) slots written in time order, the others zero bytes
        assert np.array_equal(o.stored, np.minimum(o.count, 2)) and np.array_equal(o.valid, np.arange(2)[None, :] < o.stored[:, None])
        assert np.all(o.xi[~o.valid] == 0) and np.all(o.eta[~o.valid] == 0) and np.all(o.time[~o.valid] == 0)
        assert np.all(o.step[~o.valid] == 0)
        both = o.stored == 2
        assert np.all(o.time[both, 0] * np.sign(kw["dt"]) < o.time[both, 1] * np.sign(kw["dt"]))
        assert np.all(np.abs(np.einsum("mkc,c->mk", o.xi, NORMAL) - OFFSET)[o.valid] <= 1e-12 * (1 + np.abs(o.xi).max()))
        st = o.stats
        assert (st.crossings, st.stored, st.overflowed) == (int(o.count.sum()), int(o.stored.sum()), int((o.count > 2).sum()))
        so = st.orbit
        assert (so.step_num, so.n, so.nonfinite, so.tracers, so.nonfinite_tracers) == (3 * (kind == "tree"), n, 0, m, 0)
        assert (so.records, so.pair_launches, so.flags) == (records, STEPS + 1, int(kw["energy"]))
        assert np.isfinite(o.orbits.pos).all() and np.isfinite(o.summary["r2_max"]).all()
        if m >= 65 and kw["omega"] != 0.0:
            # on the replay, not on the device: the three kinds of list are all there
            cnt = ref["counts"]
            assert cnt[1] == 0 and np.any((cnt >= 1) & (cnt <= 2)) and np.any(cnt > 2), np.bincount(cnt)
            assert 1 <= cnt[2] + cnt[3] <= 2
    sim.destroy()


# ---- 2. the tracks are orbits()'s --------------------------------------------------------------
@pytest.mark.parametrize("idx", [4, 8, 10])
def test_tracks_are_those_of_orbits(gpu, idx):
    nb = gpu
    sim, pos, vel = _case(nb, idx)
    for j in range(2):
        kw = _case_kw(idx, j)
        o = sim.orbit_sections(pos, vel, **kw)
        plain = sim.orbits(pos, vel, **{k: v for k, v in kw.items()
                                        if k not in ("max_crossings", "normal", "offset", "direction")})
        assert _same_tracks(o.orbits, plain) and np.array_equal(o.orbits.step, plain.step)
        assert o.stats.orbit == plain.stats and plain.stats.pair_launches == STEPS + 1
    sim.destroy()


# ---- 3. determinism and places -----------------------------------------------------------------
@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_determinism_permutation_and_bands(gpu, kind):
    nb = gpu
    n, m = 4099, 257
    state = _state(n, seed=41)
    sim = _sim(nb, kind, state)
    pos, vel = _tracers(state, m, seed=6)
    for energy in (False, True):
        kw = dict(dt=0.1, steps=STEPS, every=5, omega=4.0, axis=AXIS, center=CENTER, energy=energy, normal=NORMAL,
                  offset=OFFSET, direction=0, max_crossings=2)
        a = sim.orbit_sections(pos, vel, **kw)
        assert _same_sections(a, sim.orbit_sections(pos, vel, **kw))
        perm = np.random.default_rng(7).permutation(m)
        p = sim.orbit_sections(pos[perm], vel[perm], **kw)
        assert np.array_equal(p.count, a.count[perm]) and _same(p.xi, a.xi[perm]) and _same(p.eta, a.eta[perm])
        assert _same(p.time, a.time[perm]) and np.array_equal(p.step, a.step[perm])
        assert _same_summary(p.summary, a.summary[perm]) and _same(p.orbits.pos, a.orbits.pos[:, perm])
        # bands: 2^16 pairs are less than one tile of tracers against 4099 bodies, so every tile is a launch and
        # a tracer's place in its band is not its number
        sim.set_tuning("field_launch_pairs_log2", 16)
        b = sim.orbit_sections(pos, vel, **kw)
        sim.set_tuning("field_launch_pairs_log2", 35)
        assert _same_sections(a, b)
        assert a.stats.orbit.pair_launches == STEPS + 1
        assert b.stats.orbit.pair_launches > 2 * a.stats.orbit.pair_launches - 1
        assert a.count.max() > 2 and a.count.min() == 0
    sim.destroy()


# ---- 4. continuation ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,every", [(257, 65, 8), (4099, 257, 24)])
def test_continuation_is_exact(gpu, n, m, every):
    nb = gpu
    half = 24
    state = _state(n, seed=51)
    sim = _sim(nb, "naive", state)
    pos, vel = _tracers(state, m, seed=8)
    kw = dict(dt=0.1, every=every, omega=4.0, axis=AXIS, center=CENTER, energy=True, normal=NORMAL, offset=OFFSET,
              direction=0, max_crossings=16)
    whole = sim.orbit_sections(pos, vel, steps=2 * half, step0=11, **kw)
    first = sim.orbit_sections(pos, vel, steps=half, step0=11, **kw)
    x, v, step = first.orbits.final()
    assert step == 11 + half
    second = sim.orbit_sections(x, v, steps=half, step0=step, **kw)
    sim.destroy()
    r = half // every
    for name in ("pos", "vel", "potential", "energy"):
        w = getattr(whole.orbits, name)
        assert _same(w[:r + 1], getattr(first.orbits, name)) and _same(w[r:], getattr(second.orbits, name)), name
    assert whole.count.max() <= 16 and whole.count.max() >= 6  # (room for all)
    assert np.array_equal(whole.count, first.count + second.count)
    both = first.merge(second)
    # (the merged lists have the room of both: 32 slots, of which the whole run's 16 hold everything)
    assert both.xi.shape == (m, 32, 3) and not both.valid[:, 16:].any() and np.all(both.time[:, 16:] == 0)
    assert np.array_equal(both.count, whole.count) and np.array_equal(both.stored, whole.stored)
    assert _same(both.xi[:, :16], whole.xi) and _same(both.eta[:, :16], whole.eta)
    assert _same(both.time[:, :16], whole.time) and np.array_equal(both.step[:, :16], whole.step)
    assert np.array_equal(both.valid[:, :16], whole.valid) and _same_summary(both.summary, whole.summary)
    assert both.stats.crossings == whole.stats.crossings and both.stats.overflowed == 0
    # ... and the summaries are nb_orbit_summary_merge's, as numpy has it
    assert _same_summary(whole.summary, S.merge(first.summary, second.summary))
    assert np.any(first.summary["pericentres"] + first.summary["apocentres"] > 0)
    # every bracket belongs to one half
    assert np.all(first.step[first.valid] < 11 + half) and np.all(second.step[second.valid] >= 11 + half)


# ---- 5. edge cases -----------------------------------------------------------------------------
def test_nonfinite_tracers(gpu):
    nb = gpu
    n, m = 4099, 257
    state = _state(n, seed=41)
    sim = _sim(nb, "naive", state)
    pos, vel = _tracers(state, m, seed=6)
    kw = dict(dt=0.1, steps=STEPS, omega=4.0, axis=AXIS, center=CENTER, normal=NORMAL, offset=OFFSET, direction=0,
              max_crossings=4)
    a = sim.orbit_sections(pos, vel, **kw)
    # a tracer that starts non-finite, and one thrown out of fp32's range at the first step (x_1 = 1e40: finite in
    # binary64, no fp32 number, so v_1 is NaN and x_2 too)
    dirty_p, dirty_v = pos.copy(), vel.copy()
    dirty_p[100, 1] = np.nan
    dirty_v[7] = (1e41, 0.0, 0.0)
    d = sim.orbit_sections(dirty_p, dirty_v, **kw)
    ref = _replay(nb, sim, dirty_p, dirty_v, **kw)
    sim.destroy()
    _assert_is_replay(d, ref, "non-finite")
    assert d.stats.orbit.nonfinite_tracers == 1
    # started non-finite: nothing, and the extrema as they were initialised
    s = d.summary[100]
    assert d.count[100] == 0 and not d.valid[100].any()
    assert s["r2_min"] == s["R2_min"] == s["lz_min"] == np.inf
    assert s["r2_max"] == s["R2_max"] == s["lz_max"] == s["h_max"] == -np.inf
    assert s["first_peri"] == s["last_peri"] == S.NO_STEP
    assert (s["pericentres"], s["apocentres"], s["plane_ups"], s["winding_pattern"], s["winding_inertial"]) == (0,) * 5
    # became non-finite: states 0 and 1 have finite positions, so r2's extrema are theirs; the velocity is NaN from
    # state 1 on, so L_z has state 0 alone; no crossing after bracket (0, 1)
    s = d.summary[7]
    assert np.isfinite(s["r2_min"]) and s["r2_max"] > 1e79 and s["lz_min"] == s["lz_max"]
    assert d.count[7] <= 1 and np.all(d.step[7][d.valid[7]] == 0)
    assert s["pericentres"] + s["apocentres"] <= 1
    # the neighbours keep their bits
    ok = (np.arange(m) != 100) & (np.arange(m) != 7)
    assert np.array_equal(d.count[ok], a.count[ok]) and _same(d.xi[ok], a.xi[ok]) and _same(d.eta[ok], a.eta[ok])
    assert _same(d.time[ok], a.time[ok]) and _same_summary(d.summary[ok], a.summary[ok])


@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_no_bodies_gives_straight_lines_that_cross_once(gpu, kind):
    """x_k = x_0 + k (v dt) to rounding, so s is linear in time and the linear interpolation is exact: the crossing
    is at t = -s(0) / (N . v'), where ' is the frame."""
    nb = gpu
    sim = _sim(nb, kind, np.zeros((0, 10), np.float32))
    rng = np.random.default_rng(9)
    m, dt = 65, 0.3
    pos, vel = rng.normal(size=(m, 3)), rng.normal(size=(m, 3))
    n, e1, e2 = nb.map_frame(AXIS)
    frame = np.stack([e1, e2, n])  # rows: a, b, l
    s0 = (pos - np.asarray(CENTER)) @ frame.T @ np.asarray(NORMAL) - OFFSET
    rate = vel @ frame.T @ np.asarray(NORMAL)
    t_star = -s0 / rate
    o = sim.orbit_sections(pos, vel, dt=dt, steps=STEPS, axis=AXIS, center=CENTER, normal=NORMAL, offset=OFFSET,
                           direction=0, max_crossings=3)
    inside = (t_star > 0.01) & (t_star < STEPS * dt - 0.01)
    outside = (t_star < -0.01) | (t_star > STEPS * dt + 0.01)
    assert inside.sum() >= 10 and outside.sum() >= 10
    assert np.all(o.count[inside] == 1) and np.all(o.count[outside] == 0)
    assert np.allclose(o.time[inside, 0], t_star[inside], rtol=0, atol=1e-12)
    assert np.array_equal(o.step[inside, 0], np.floor(o.time[inside, 0] / dt).astype(np.uint64))
    x_star = pos + vel * t_star[:, None]
    assert np.allclose(o.xi[inside, 0], ((x_star - np.asarray(CENTER)) @ frame.T)[inside], rtol=0, atol=1e-12)
    assert np.allclose(o.eta[inside, 0], (vel @ frame.T)[inside], rtol=0, atol=1e-13)
    assert (o.stats.orbit.n, o.stats.orbit.pair_launches, o.stats.crossings) == (0, 0, int(o.count.sum()))
    # one direction keeps the crossings that go its way
    up = sim.orbit_sections(pos, vel, dt=dt, steps=STEPS, axis=AXIS, center=CENTER, normal=NORMAL, offset=OFFSET,
                            direction=1, max_crossings=3)
    assert np.array_equal(up.count[inside], (rate[inside] > 0).astype(np.uint32))
    # m = 0 is valid
    e = sim.orbit_sections(np.zeros((0, 3)), np.zeros((0, 3)), dt=dt, steps=2)
    assert e.xi.shape == (0, 256, 3) and e.count.shape == (0,) and e.stats.crossings == 0
    sim.destroy()


def test_no_room_gives_counts_and_summaries_alone(gpu):
    nb = gpu
    from wgpu_n_body_amd import _lib
    state = _state(257, seed=23)
    sim = _sim(nb, "naive", state)
    pos, vel = _tracers(state, 65, seed=3)
    kw = dict(dt=0.1, steps=STEPS, omega=4.0, axis=AXIS, center=CENTER, normal=NORMAL, offset=OFFSET, direction=0)
    full = sim.orbit_sections(pos, vel, max_crossings=16, **kw)
    none = sim.orbit_sections(pos, vel, max_crossings=0, **kw)  # (null crossings)
    assert none.xi.shape == (65, 0, 3) and np.array_equal(none.count, full.count)
    assert _same_summary(none.summary, full.summary) and _same_tracks(none.orbits, full.orbits)
    assert (none.stats.crossings, none.stats.stored, none.stats.overflowed) == (
        full.stats.crossings, 0, int((full.count > 0).sum()))
    # ... and every output but the tracks may be null
    p, s = _lib.nb_orbit_params(), _lib.nb_orbit_section_params()
    p.dt, p.steps, p.every, p.accel_scale, p.omega = 0.1, STEPS, STEPS, 1.0, 4.0
    p.axis[:], p.center[:], s.normal[:] = AXIS, CENTER, NORMAL
    s.offset, s.direction, s.max_crossings = OFFSET, 0, 0
    x, v = np.ascontiguousarray(pos), np.ascontiguousarray(vel)
    tracks = np.zeros((2, 65), _lib.ORBIT_SAMPLE_DTYPE)
    assert _lib.lib().nb_orbit_sections_sim(sim._h, C.byref(p), C.byref(s), x.ctypes.data, v.ctypes.data, 65,
                                            tracks.ctypes.data, None, None, None, None, None) == 0
    assert _same(tracks["pos"], full.orbits.pos)
    sim.destroy()


# ---- 6. the launch helper ----------------------------------------------------------------------
def test_jacobi_launch_shares_the_jacobi_integral(gpu):
    """The k = 0 energy record of tracers from jacobi_launch is E_J within eight roundings of the three terms it is
    made of: 8 2^-53 (eta^2 / 2 + |Phi| + |omega L|)."""
    nb = gpu
    state = R.binary_state()
    sim = _sim(nb, "naive", state)
    omega, axis, e_j = 0.7, (0.0, 0.0, 1.0), -0.9
    a = np.linspace(0.2, 2.5, 65)
    pos, vel = sim.jacobi_launch(e_j, a, omega=omega, axis=axis)
    ok = np.isfinite(pos).all(1)
    assert ok.sum() >= 10 and (~ok).sum() >= 10 and np.array_equal(ok, np.isfinite(vel).all(1))
    o = sim.orbit_sections(pos, vel, dt=0.02, steps=8, energy=True, omega=omega, axis=axis)
    phi = o.orbits.potential[0]
    v0 = o.orbits.vel[0]
    L = (pos[:, 0] * v0[:, 1] - pos[:, 1] * v0[:, 0])
    eta = v0[:, 1] - omega * a  # (the velocity the pattern sees: along b' alone)
    bound = 8 * 2.0 ** -53 * (0.5 * eta * eta + np.abs(phi) + np.abs(omega * L))
    err = np.abs(o.orbits.energy[0] - e_j)
    print("jacobi_launch: worst error / bound", (err[ok] / bound[ok]).max())
    assert np.all(err[ok] <= bound[ok])
    assert np.isnan(o.orbits.energy[0][~ok]).all() and o.stats.orbit.nonfinite_tracers == int((~ok).sum())
    # forbidden: where Phi_eff > E_J
    f = sim.field(pos[ok].astype(np.float32), accel=False, potential=True).potential
    assert np.all(f - 0.5 * omega ** 2 * a[ok] ** 2 <= e_j)
    g = sim.field(np.stack([a[~ok], 0 * a[~ok], 0 * a[~ok]], 1).astype(np.float32), accel=False, potential=True).potential
    assert np.all(g - 0.5 * omega ** 2 * a[~ok] ** 2 > e_j)
    # they start on the a' axis, moving along b' alone in the pattern frame
    assert np.all(pos[ok, 1:] == 0) and np.all(vel[ok][:, [0, 2]] == 0)
    sim.destroy()


# ---- 7. the runner, the refusals that need a simulator, status words, the trajectory --------------------------
def test_refusals_and_the_runner(gpu):
    nb = gpu
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    s = make_state("uniform", 64, seed=1)
    pos, vel = _tracers(s, 8, seed=1)
    sharded = nb.NaiveSim.from_particles(nb.SimParams(particle_num=64), None, s, placement=nb.Placement(world=2))
    with pytest.raises(nb.NBodyError) as ex:
        sharded.orbit_sections(pos, vel, dt=0.1, steps=2)
    assert ex.value.code == _lib.NB_ERR_UNSUPPORTED and b"sharded" in L.nb_last_error()
    sharded.destroy()
    r = nb.OfflineHeadless(nb.NaiveSim, nb.SimParams(particle_num=512), None,
                           lambda p: nb.inits.uniform_init(p, seed=1), device_ids=[0, 0])
    with pytest.raises(nb.NBodyError) as ex:
        r.orbit_sections(pos, vel, dt=0.1, steps=2)
    assert ex.value.code == _lib.NB_ERR_UNSUPPORTED
    r.destroy()
    sim = _sim(nb, "naive", s, e=-1e-4)
    with pytest.raises(nb.NBodyError) as ex:
        sim.orbit_sections(pos, vel, dt=0.1, steps=2, energy=True)
    assert ex.value.code == _lib.NB_ERR_INVALID and "e >= 0" in str(ex.value)
    with pytest.raises(nb.NBodyError) as ex:
        sim.orbit_sections(pos, vel, dt=0.1, steps=2, direction=2)
    assert ex.value.code == _lib.NB_ERR_INVALID and "direction" in str(ex.value)
    sim.destroy()
    big = _sim(nb, "naive", make_state("uniform", 1 << 18, seed=2))
    with pytest.raises(nb.NBodyError) as ex:  # 256 padded tracers x 2^18 bodies x (2^20 + 1) evaluations
        big.orbit_sections(np.zeros((200, 3)), np.zeros((200, 3)), dt=0.1, steps=1 << 20)
    assert ex.value.code == _lib.NB_ERR_UNSUPPORTED and "split" in str(ex.value)
    big.destroy()
    # nb_orbit_sections_runner is nb_orbit_sections_sim of the runner's simulator
    r = nb.OfflineHeadless(nb.TreeSim, nb.SimParams(particle_num=2048), nb.AddParams.TreeSimParams(0.75),
                           lambda p: nb.inits.disc_init(p, seed=2))
    r.step()
    state = nb.as_floats(r.read_particles())
    pos, vel = _tracers(state, 100, seed=13)
    kw = dict(dt=0.5, steps=STEPS, every=5, omega=0.8, energy=True, coupling="step", normal=NORMAL, offset=OFFSET,
              direction=0, max_crossings=4, axis=AXIS, center=CENTER)
    a, b = r.orbit_sections(pos, vel, **kw), r.sim.orbit_sections(pos, vel, **kw)
    r.destroy()
    assert _same_sections(a, b) and a.stats == b.stats and a.stats.orbit.step_num == 1 and a.stats.crossings > 0


def test_a_tree_steps_status_words_surface(gpu):
    nb = gpu
    n = 2048
    s = make_state("uniform", n, 78)
    s[100:112, 0:3] = s[100, 0:3] + (np.arange(12, dtype=np.float32)[:, None] * np.float32(1e-9))
    sim = _sim(nb, "tree", s, theta=0.5)
    sim.encode()
    with pytest.raises(nb.NBodyError) as ei:
        sim.orbit_sections(s[:4, 0:3], np.zeros((4, 3)), dt=0.1, steps=2)
    assert "Morton key" in str(ei.value)
    sim.destroy()


@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_does_not_perturb_the_trajectory(gpu, kind):
    nb = gpu
    state = make_state("uniform", 4096, seed=9)
    pos, vel = _tracers(state, 300, seed=12)
    finals = []
    for with_sections in (False, True):
        sim = _sim(nb, kind, state)
        for k in range(3):
            sim.encode()
            if with_sections:
                o = sim.orbit_sections(pos, vel, dt=0.1, steps=3, energy=k != 1, omega=4.0 * (k != 2), max_crossings=2)
                assert o.stats.orbit.step_num == k + 1
        finals.append(nb.as_floats(sim.read_particles()).copy())
        sim.destroy()
    assert np.array_equal(finals[0].view(np.uint32), finals[1].view(np.uint32))


# ---- 8. the CLI --------------------------------------------------------------------------------
def test_cli_sections(gpu, tmp_path):
    """headless --sections (the C++ mirror's circular_orbit_sections over nb_orbit_sections_runner) writes what the
    Python runner's orbit_sections returns from the tracers of circular_orbits, bit for bit."""
    nb = gpu
    cli = os.path.join(ROOT, "wgpu_n_body_amd", "headless")
    p = subprocess.run([cli, "--sim", "tree", "--n", "2048", "--init", "disc", "--steps", "3", "--sections", str(tmp_path),
                        "--sections-at", "2", "--sections-range", "0.2,1.2", "--sections-bins", "6", "--sections-dt",
                        "0.05", "--sections-steps", "200", "--sections-omega", "0.9", "--sections-speed", "0.9",
                        "--sections-axis", "0,0,1", "--sections-normal", "0.2,1,0", "--sections-offset", "0.01",
                        "--sections-direction", "0", "--sections-max", "5"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("sections ")]
    assert len(lines) == 1 and lines[0][1:3] == ["2", "6"], p.stdout
    assert len([ln for ln in p.stdout.splitlines() if ln.startswith("Step Duration: ")]) == 3
    got = np.load(tmp_path / "sections_000002.npy")
    counts = np.load(tmp_path / "sections_000002_counts.npy")
    assert got.shape == (6, 5, 8) and got.dtype == np.float64 and counts.shape == (6,)
    runner = nb.OfflineHeadless(nb.TreeSim, nb.SimParams(particle_num=2048), nb.AddParams.TreeSimParams(0.75),
                                lambda sp: nb.inits.disc_init(sp, seed=0))
    runner.step()
    runner.step()
    radii = np.array([0.2 + (1.2 - 0.2) * i / 5 for i in range(6)])
    axis = (0.0, 0.0, 1.0)
    cv = runner.circular_velocity(radii, axis=axis)
    pts = nb.field_rings(radii, axis=axis, center=(0, 0, 0), n_phi=16)
    pos = pts[::16].astype(np.float64)
    vel = (0.9 * cv.v_c)[:, None] * nb.map_frame(axis)[2][None, :]
    o = runner.orbit_sections(pos, vel, dt=0.05, steps=200, omega=0.9, axis=axis, normal=(0.2, 1.0, 0.0), offset=0.01,
                              direction=0, max_crossings=5)
    runner.destroy()
    ours = np.concatenate([o.xi, o.eta, o.time[:, :, None], o.step.astype(np.float64)[:, :, None]], axis=2)
    assert _same(got, ours) and np.array_equal(counts, o.count.astype(np.float64))
    assert o.count.sum() > 0 and lines[0][3:6] == [str(o.stats.crossings), str(o.stats.stored), str(o.stats.overflowed)]
    p = subprocess.run([cli, "--sim", "naive", "--n", "256", "--steps", "2"], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and "sections" not in p.stdout
