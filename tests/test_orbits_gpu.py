"""nb_orbits_sim on the device (the orbit unit of csrc/nb_field.hip): every double of every record against a host
replay of the rule (tests/orbit_ref.py) whose accelerations are the same simulator's field(); the first step against
binary64 within the field's derived bound; determinism, permutation, bands and non-finite tracers and bodies; the
exact continuation; hand cases; the Jacobi integral against the restatement's; that a call does not perturb the
trajectory; the runner, the refusals that need a simulator and the CLI.  `-m gpu`."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import field_ref as F
from tests import orbit_ref as R
from tests.helpers import E, G, ROOT, make_state

pytestmark = pytest.mark.gpu

STEPS, EVERY, DT_ = 5, 2, 0.02  # records at 0, 2, 4, 5
AXIS = (1.0, 2.0, 3.0)


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


def _tracers(state, m, seed):
    """m tracers in the bodies' box with velocities of the size of the box per unit time; the first on a body."""
    rng = np.random.default_rng(seed)
    lo, hi = state[:, 0:3].min(0) - 0.5, state[:, 0:3].max(0) + 0.5
    pos = rng.uniform(lo, hi, size=(m, 3))
    vel = rng.normal(size=(m, 3)) * 0.5
    pos[0] = state[rng.integers(0, state.shape[0]), 0:3]
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


def _same_orbits(a, b):
    return (_same(a.pos, b.pos) and _same(a.vel, b.vel) and _same(a.potential, b.potential)
            and _same(a.energy, b.energy) and np.array_equal(a.coincident, b.coincident))


def _replay(nb, sim, pos, vel, **kw):
    """The rule on the host around the simulator's own field(): phases from nb_orbit_phase, frame from
    nb_map_frame."""
    coupling = kw.pop("coupling", "field")
    scale = {"field": 1.0, "step": float(sim.sim_params().dt)}[coupling]
    omega = kw.get("omega", 0.0)
    frame = nb.map_frame(kw["axis"]) if omega != 0.0 else None
    return R.orbits(R.device_field(sim), pos, vel, accel_scale=scale, phase=_lib_phase, frame=frame, **kw)


# ---- 1. replay, bit for bit --------------------------------------------------------------------
# every M against every N on the all-pairs simulator, the options turning over; three of them on the tree
CASES = [("naive", n, m) for n in (1, 257, 4099) for m in (1, 65, 257)] + [("tree", 257, 65), ("tree", 4099, 257),
                                                                           ("tree", 4099, 1)]
OPTIONS = [dict(omega=0.0, energy=False, coupling="field"), dict(omega=0.7, energy=True, coupling="field"),
           dict(omega=0.7, energy=False, coupling="step"), dict(omega=0.0, energy=True, coupling="step")]


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[f"{k}-n{n}-m{m}" for k, n, m in CASES])
def test_replay_bit_for_bit(gpu, idx):
    nb = gpu
    kind, n, m = CASES[idx]
    sim = _sim(nb, kind, _state(n, seed=20 + idx))
    if kind == "tree":
        for _ in range(3):  # the state read_particles returns, in the tree's order
            sim.encode()
    state = nb.as_floats(sim.read_particles())
    pos, vel = _tracers(state, m, seed=idx)
    for j in range(2):
        opt = dict(OPTIONS[(idx + 2 * j + (idx // 4)) % 4])
        # "step" multiplies the acceleration by dt = 0.016: longer steps, so that the tracers still turn
        dt = DT_ if opt["coupling"] == "field" else 2.5
        kw = dict(dt=dt, steps=STEPS, every=EVERY, axis=AXIS, center=(0.1, -0.2, 0.05), **opt)
        o = sim.orbits(pos, vel, **kw)
        ref = _replay(nb, sim, pos, vel, **kw)
        assert o.pos.shape == (4, m, 3) and list(o.step) == [0, 2, 4, 5] and np.array_equal(o.time, o.step * dt)
        for name in ("pos", "vel", "potential", "energy"):
            assert _same(getattr(o, name), ref[name]), (name, opt)
        assert np.array_equal(o.coincident, ref["coincident"])
        assert o.coincident[0] >= 1 or opt["omega"] != 0.0  # (on a body at k = 0, unless the frame's lines round it off)
        assert np.isfinite(o.pos).all() and np.isfinite(o.vel).all()
        assert np.isfinite(o.energy).all() if opt["energy"] else np.isnan(o.energy).all() and np.isnan(o.potential).all()
        st = o.stats
        assert (st.step_num, st.n, st.nonfinite, st.tracers, st.nonfinite_tracers) == (3 * (kind == "tree"), n, 0, m, 0)
        assert (st.records, st.pair_launches, st.flags) == (4, STEPS + 1, int(opt["energy"]))
        assert np.any(o.vel[-1] != vel, axis=1).all()  # (under a force)
    sim.destroy()


# ---- 2. the first step against binary64 --------------------------------------------------------
@pytest.mark.parametrize("n,m", [(257, 65), (4099, 257)])
def test_first_step_against_binary64(gpu, n, m):
    """x_1 = x_0 + (v_0 + A_0 h) dt: the field's derived bound, (64 + 16) 2^-24 g sum m |d_k| / (r^4 + e r), carried
    through the two lines that use A_0, and eight roundings of binary64 for the lines themselves."""
    nb = gpu
    state = _state(n, seed=31)
    sim = _sim(nb, "naive", state)
    pos, vel = _tracers(state, m, seed=5)
    pos = pos.astype(np.float32).astype(np.float64)  # (points that are fp32 numbers: the bound is the field's)
    dt = 0.05
    o = sim.orbits(pos, vel, dt=dt, steps=1)
    sim.destroy()
    ref = F.field64(state, pos.astype(np.float32), G, E, potential=False)
    h = dt / 2
    x1 = pos + (vel + ref["acc"] * h) * dt
    bound = abs(h * dt) * F.ACC_BOUND * ref["acc_scale"] \
        + 8 * 2.0 ** -53 * (np.abs(pos) + np.abs(vel * dt) + np.abs(ref["acc"] * h * dt))
    err = np.abs(o.pos[1] - x1)
    print("first step: worst error / bound", (err / bound).max(), "force part of the bound",
          (abs(h * dt) * F.ACC_BOUND * ref["acc_scale"] / bound).min())
    assert np.all(err <= bound)
    assert np.array_equal(o.pos[0], pos) and np.array_equal(o.vel[0], vel)
    print("first step: the kick's part of the step over the bound", (np.abs(ref["acc"] * h * dt) / bound).max())


# ---- 3. determinism and places -----------------------------------------------------------------
@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_determinism_permutation_bands_and_nonfinite(gpu, kind):
    nb = gpu
    n, m = 4099, 257
    state = _state(n, seed=41)
    state[1234, 4] = np.nan  # a NaN body: left out and counted
    sim = _sim(nb, kind, state)
    pos, vel = _tracers(state[np.isfinite(state).all(1)], m, seed=6)
    for energy in (False, True):
        kw = dict(dt=DT_, steps=STEPS, every=EVERY, omega=0.7, axis=AXIS, energy=energy)
        a = sim.orbits(pos, vel, **kw)
        again = sim.orbits(pos, vel, **kw)
        assert _same_orbits(a, again)
        perm = np.random.default_rng(7).permutation(m)
        p = sim.orbits(pos[perm], vel[perm], **kw)
        assert _same(p.pos, a.pos[:, perm]) and _same(p.vel, a.vel[:, perm]) and _same(p.energy, a.energy[:, perm])
        assert _same(p.potential, a.potential[:, perm]) and np.array_equal(p.coincident, a.coincident[perm])
        # bands: 2^16 pairs are less than one tile of tracers against 4099 bodies, so every tile is a launch
        sim.set_tuning("field_launch_pairs_log2", 16)
        b = sim.orbits(pos, vel, **kw)
        sim.set_tuning("field_launch_pairs_log2", 35)
        assert _same_orbits(a, b)
        assert a.stats.pair_launches == STEPS + 1 and b.stats.pair_launches > 2 * a.stats.pair_launches - 1
        assert a.stats.nonfinite == b.stats.nonfinite == 1 and a.stats.nonfinite_tracers == 0
        # a NaN tracer: NaN rows, its neighbours bit for bit
        dirty_p, dirty_v = pos.copy(), vel.copy()
        dirty_p[100, 1] = np.nan
        d = sim.orbits(dirty_p, dirty_v, **kw)
        ok = np.arange(m) != 100
        assert d.stats.nonfinite_tracers == 1 and d.coincident[100] == 0
        assert np.isnan(d.pos[:, 100]).all() and np.isnan(d.vel[:, 100]).all()
        assert np.isnan(d.potential[:, 100]).all() and np.isnan(d.energy[:, 100]).all()
        assert _same(d.pos[:, ok], a.pos[:, ok]) and _same(d.vel[:, ok], a.vel[:, ok])
        assert _same(d.energy[:, ok], a.energy[:, ok]) and np.array_equal(d.coincident[ok], a.coincident[ok])
    # the NaN body is left out: the replay through field(), which leaves it out, is the same
    ref = _replay(nb, sim, pos, vel, dt=DT_, steps=STEPS, every=EVERY, omega=0.7, axis=AXIS, energy=True)
    assert _same(a.pos, ref["pos"]) and _same(a.energy, ref["energy"])
    # a tracer thrown out of fp32's range becomes NaN from there on, and only it
    far_v = vel.copy()
    far_v[7] = (1e41, 0.0, 0.0)  # x_1 = 2e39, not an fp32 number
    f = sim.orbits(pos, far_v, **kw)
    assert np.isfinite(f.pos[0, 7]).all() and np.isnan(f.vel[1:, 7]).all() and f.stats.nonfinite_tracers == 0
    ok = np.arange(m) != 7
    assert _same(f.pos[:, ok], a.pos[:, ok])
    sim.destroy()


# ---- 4. continuation ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(257, 65), (4099, 257)])
def test_continuation_is_exact(gpu, n, m):
    nb = gpu
    state = _state(n, seed=51)
    sim = _sim(nb, "naive", state)
    pos, vel = _tracers(state, m, seed=8)
    kw = dict(dt=DT_, every=3, omega=0.7, axis=AXIS, center=(0.1, 0.0, -0.1), energy=True)
    whole = sim.orbits(pos, vel, steps=6, step0=11, **kw)
    first = sim.orbits(pos, vel, steps=3, step0=11, **kw)
    x, v, step = first.final()
    assert step == 14
    second = sim.orbits(x, v, steps=3, step0=step, **kw)
    other = sim.orbits(x, v, steps=3, step0=0, **kw)
    sim.destroy()
    assert list(whole.step) == [11, 14, 17] and list(first.step) == [11, 14] and list(second.step) == [14, 17]
    for name in ("pos", "vel", "potential", "energy"):
        w = getattr(whole, name)
        assert _same(w[:2], getattr(first, name)) and _same(w[1:], getattr(second, name)), name
    # state 14 is evaluated by both halves, and by the whole run once
    assert np.all(first.coincident + second.coincident >= whole.coincident)
    # the phase matters: the same second half numbered from 0 is another orbit
    assert not _same(other.pos, second.pos)


# ---- 5. hand cases -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_no_bodies_gives_straight_lines(gpu, kind):
    nb = gpu
    sim = _sim(nb, kind, np.zeros((0, 10), np.float32))
    rng = np.random.default_rng(9)
    pos, vel = rng.normal(size=(65, 3)), rng.normal(size=(65, 3))
    for omega in (0.0, 0.7):
        o = sim.orbits(pos, vel, dt=0.3, steps=STEPS, every=EVERY, omega=omega, axis=AXIS, energy=True)
        x, rows = pos.copy(), {}
        for k in range(STEPS + 1):
            rows[k] = x
            w = vel + 0.0 * (0.3 / 2)
            x = x + w * 0.3
        for r, k in enumerate((0, 2, 4, 5)):
            assert _same(o.pos[r], rows[k]) and _same(o.vel[r], vel), (omega, k)
        assert np.all(o.potential == 0) and np.all(o.coincident == 0)
        assert (o.stats.n, o.stats.pair_launches, o.stats.records) == (0, 0, 4)
    # m = 0 is valid
    o = sim.orbits(np.zeros((0, 3)), np.zeros((0, 3)), dt=0.3, steps=2)
    assert o.pos.shape == (3, 0, 3) and o.stats.tracers == 0
    sim.destroy()


def test_a_tracer_at_rest_on_the_only_body_stays(gpu):
    nb = gpu
    state = _state(1, seed=0)
    sim = _sim(nb, "naive", state)
    x0 = state[0, 0:3].astype(np.float64)[None, :]
    o = sim.orbits(x0, np.zeros((1, 3)), dt=0.1, steps=STEPS, every=EVERY, energy=True)
    sim.destroy()
    assert np.array_equal(o.pos, np.broadcast_to(x0, (4, 1, 3))) and np.all(o.vel == 0)
    assert o.coincident[0] == STEPS + 1 and np.all(o.potential == 0) and np.all(o.energy == 0)


# ---- 6. the Jacobi integral --------------------------------------------------------------------
@pytest.mark.parametrize("omega", [0.7, 0.0])
def test_jacobi_integral_is_conserved_to_the_integrators_order(gpu, omega):
    """The case of tests/test_orbits.py on the device, 100 steps of 0.02: the recorded energy -- the Jacobi integral
    with the pattern turning -- stays within twice the range the binary64 restatement has in the same run plus
    twice the field's potential bound, 5e-6 g sum m psi; the plain energy of a turning pattern does not."""
    nb = gpu
    state = R.binary_state()
    sim = _sim(nb, "naive", state)
    kw = dict(dt=0.02, steps=100, energy=True, omega=omega, axis=(0.0, 0.0, 1.0))
    o = sim.orbits([R.CASE_X0], [R.CASE_V0], **kw)
    sim.destroy()
    ref = R.orbits(R.all_pairs64(state, R.CASE_G, R.CASE_E), [R.CASE_X0], [R.CASE_V0], **kw)
    pot_scale = max(F.field64(state, ref["pos"][:, 0].astype(np.float32), R.CASE_G, R.CASE_E)["pot_scale"].max(),
                    F.field64(state, o.pos[:, 0].astype(np.float32), R.CASE_G, R.CASE_E)["pot_scale"].max())
    ref_range = np.ptp(ref["energy"][:, 0])
    got = o.energy_range()[0]
    v = o.vel[:, 0]
    plain = np.ptp(0.5 * (v * v).sum(1) + o.potential[:, 0])
    print("omega", omega, "energy range: device", got, "restatement", ref_range, "potential bound",
          F.POT_BOUND * pot_scale, "plain energy range", plain)
    assert got == np.ptp(o.energy[:, 0]) and ref_range > 0
    assert got <= 2 * ref_range + 2 * F.POT_BOUND * pot_scale
    if omega:
        assert plain >= 0.05
        # in the frame of the pattern the tracer starts where it starts, and the frame has turned by the end
        assert _same(o.in_pattern_frame()[0], o.pos[0]) and not np.allclose(o.in_pattern_frame()[-1], o.pos[-1])
    else:
        assert np.ptp(0.5 * (v * v).sum(1) + o.potential[:, 0]) <= 2 * ref_range + 2 * F.POT_BOUND * pot_scale
        assert _same(o.in_pattern_frame(), o.pos)
    # the trajectory itself: a force off by 80 2^-24 = 4.8e-6 of |a| < 1 for t = 2 displaces by 0.5 4.8e-6 t^2 = 1e-5
    # along an orbit that is not chaotic; ten times that
    assert np.abs(o.pos - ref["pos"]).max() <= 1e-4


# ---- 7. does not perturb the trajectory --------------------------------------------------------
@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_does_not_perturb_the_trajectory(gpu, kind):
    nb = gpu
    state = make_state("uniform", 4096, seed=9)
    pos, vel = _tracers(state, 300, seed=12)
    finals = []
    for with_orbits in (False, True):
        sim = _sim(nb, kind, state)
        for k in range(3):
            sim.encode()
            if with_orbits:
                o = sim.orbits(pos, vel, dt=DT_, steps=3, energy=k != 1, omega=0.7 * (k != 2))
                assert o.stats.step_num == k + 1
        finals.append(nb.as_floats(sim.read_particles()).copy())
        sim.destroy()
    assert np.array_equal(finals[0].view(np.uint32), finals[1].view(np.uint32))


def test_a_tree_steps_status_words_surface(gpu):
    """Twelve bodies on one Morton key: the step completes in bounds and raises a status word, which orbits()
    reports after its synchronisation as read_particles does."""
    nb = gpu
    n = 2048
    s = make_state("uniform", n, 78)
    s[100:112, 0:3] = s[100, 0:3] + (np.arange(12, dtype=np.float32)[:, None] * np.float32(1e-9))
    sim = _sim(nb, "tree", s, theta=0.5)
    sim.encode()
    with pytest.raises(nb.NBodyError) as ei:
        sim.orbits(s[:4, 0:3], np.zeros((4, 3)), dt=DT_, steps=2)
    assert "Morton key" in str(ei.value)
    sim.destroy()


# ---- 8. the runner, the refusals that need a simulator, the CLI ----------------------------------
def test_refusals_and_the_runner(gpu):
    nb = gpu
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    s = make_state("uniform", 64, seed=1)
    pos, vel = _tracers(s, 8, seed=1)
    # a sharded simulator (rank 0 of 2)
    sharded = nb.NaiveSim.from_particles(nb.SimParams(particle_num=64), None, s, placement=nb.Placement(world=2))
    with pytest.raises(nb.NBodyError) as ex:
        sharded.orbits(pos, vel, dt=DT_, steps=2)
    assert ex.value.code == _lib.NB_ERR_UNSUPPORTED and b"sharded" in L.nb_last_error()
    sharded.destroy()
    # a several-GPU runner, both ranks on device 0
    r = nb.OfflineHeadless(nb.NaiveSim, nb.SimParams(particle_num=512), None,
                           lambda p: nb.inits.uniform_init(p, seed=1), device_ids=[0, 0])
    with pytest.raises(nb.NBodyError) as ex:
        r.orbits(pos, vel, dt=DT_, steps=2)
    assert ex.value.code == _lib.NB_ERR_UNSUPPORTED
    r.destroy()
    # the potential with e < 0, and a call above 2^44 pairs
    sim = _sim(nb, "naive", s, e=-1e-4)
    with pytest.raises(nb.NBodyError) as ex:
        sim.orbits(pos, vel, dt=DT_, steps=2, energy=True)
    assert ex.value.code == _lib.NB_ERR_INVALID and "e >= 0" in str(ex.value)
    assert np.isfinite(sim.orbits(pos[1:], vel[1:], dt=DT_, steps=2).pos).all()
    with pytest.raises(ValueError):
        sim.orbits(pos, vel, dt=DT_, steps=2, coupling="both")
    sim.destroy()
    big = _sim(nb, "naive", make_state("uniform", 1 << 18, seed=2))
    with pytest.raises(nb.NBodyError) as ex:  # 256 padded tracers x 2^18 bodies x (2^20 + 1) evaluations
        big.orbits(np.zeros((200, 3)), np.zeros((200, 3)), dt=DT_, steps=1 << 20, every=1 << 20)
    assert ex.value.code == _lib.NB_ERR_UNSUPPORTED and "split" in str(ex.value)
    big.destroy()
    # nb_orbits_runner is nb_orbits_sim of the runner's simulator
    r = nb.OfflineHeadless(nb.TreeSim, nb.SimParams(particle_num=2048), nb.AddParams.TreeSimParams(0.75),
                           lambda p: nb.inits.disc_init(p, seed=2))
    r.step()
    state = nb.as_floats(r.read_particles())
    pos, vel = _tracers(state, 100, seed=13)
    kw = dict(dt=DT_, steps=STEPS, every=EVERY, omega=0.7, energy=True, coupling="step")
    a, b = r.orbits(pos, vel, **kw), r.sim.orbits(pos, vel, **kw)
    r.destroy()
    assert _same_orbits(a, b) and a.stats == b.stats and a.stats.step_num == 1


def test_cli_orbits(gpu, tmp_path):
    """headless --orbits (the C++ mirror's circular_orbits over nb_orbits_runner) writes the array the Python
    runner's circular_orbits returns, bit for bit."""
    nb = gpu
    cli = os.path.join(ROOT, "wgpu_n_body_amd", "headless")
    p = subprocess.run([cli, "--sim", "tree", "--n", "2048", "--init", "disc", "--steps", "3", "--orbits", str(tmp_path),
                        "--orbits-at", "2", "--orbits-range", "0.2,1.2", "--orbits-bins", "6", "--orbits-dt", "0.05",
                        "--orbits-steps", "7", "--orbits-every", "3", "--orbits-omega", "0.4", "--orbits-speed", "0.9",
                        "--orbits-axis", "0,0,1"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("orbits ")]
    assert len(lines) == 1 and lines[0][1:4] == ["2", "4", "6"], p.stdout
    assert len([ln for ln in p.stdout.splitlines() if ln.startswith("Step Duration: ")]) == 3
    got = np.load(tmp_path / "orbits_000002.npy")
    assert got.shape == (4, 6, 8) and got.dtype == np.float64
    runner = nb.OfflineHeadless(nb.TreeSim, nb.SimParams(particle_num=2048), nb.AddParams.TreeSimParams(0.75),
                                lambda sp: nb.inits.disc_init(sp, seed=0))
    runner.step()
    runner.step()
    radii = [0.2 + (1.2 - 0.2) * i / 5 for i in range(6)]
    o = runner.circular_orbits(radii, dt=0.05, steps=7, every=3, omega=0.4, speed=0.9, axis=(0, 0, 1), energy=True)
    runner.destroy()
    ours = np.concatenate([o.pos, o.vel, o.potential[:, :, None], o.energy[:, :, None]], axis=2)
    assert _same(got, ours)
    assert np.isfinite(ours).all() and list(o.step) == [0, 3, 6, 7]
    # without --orbits the output has no such line
    p = subprocess.run([cli, "--sim", "naive", "--n", "256", "--steps", "2"], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and "orbits" not in p.stdout
