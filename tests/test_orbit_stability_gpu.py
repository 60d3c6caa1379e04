"""nb_orbit_stability_sim on the device (csrc/nb_stability.hip): every double and exponent of every record against a
host replay of the rule (tests/stability_ref.py) around the same simulator's field() and tidal_tensor(); the tracks
against orbits(); the first step against binary64 within the tidal tensor's derived bound; the symplectic form over 200
steps; determinism, permutation, bands and non-finite tracers; the exact continuation; no bodies; that a call does not
perturb the trajectory; the runner, the refusals that need a simulator and the CLI.  `-m gpu`."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import stability_ref as S
from tests import tidal_ref as T
from tests.helpers import E, G, ROOT, make_state
from tests.test_orbits_gpu import AXIS, CASES, _lib_phase, _same, _same_orbits, _sim, _state, _tracers

pytestmark = pytest.mark.gpu

STEPS, EVERY, DT_ = 5, 2, 0.02  # records at 0, 2, 4, 5


def _vectors(m, d, seed):
    """d vectors per tracer, every tracer its own; the second scaled by 2^40 and the third by 2^-40."""
    v = np.random.default_rng(seed).normal(size=(m, d, 6))
    if d > 1:
        v[:, 1] *= 2.0 ** 40
    if d > 2:
        v[:, 2] *= 2.0 ** -40
    return v


def _replay(nb, sim, pos, vel, dev0, **kw):
    """The rule on the host around the simulator's own field() and tidal_tensor(): phases from nb_orbit_phase, frame
    from nb_map_frame."""
    coupling = kw.pop("coupling", "field")
    scale = {"field": 1.0, "step": float(sim.sim_params().dt)}[coupling]
    omega = kw.get("omega", 0.0)
    frame = nb.map_frame(kw["axis"]) if omega != 0.0 else None
    sample, tensor = S.device(sim)
    return S.stability(sample, tensor, pos, vel, dev0, accel_scale=scale, phase=_lib_phase, frame=frame, **kw)


def _same_stability(a, b):
    return (_same_orbits(a.orbits, b.orbits) and _same(a.dev, b.dev) and np.array_equal(a.log2, b.log2)
            and a.growth.tobytes() == b.growth.tobytes())


def _check_against(o, ref):
    assert _same(o.dev, ref["dev"]) and np.array_equal(o.log2, ref["log2"])
    assert np.array_equal(o.growth["peak_log2"], ref["peak_log2"])
    assert np.array_equal(o.growth["peak_step"], ref["peak_step"])
    assert np.array_equal(o.growth["renorms"], ref["renorms"])
    assert _same(o.orbits.pos, ref["pos"]) and _same(o.orbits.vel, ref["vel"])
    assert np.array_equal(o.orbits.coincident, ref["coincident"])


# ---- 1. replay, bit for bit; 2. the tracks are orbits()'s ----------------------------------------
# the shapes of tests/test_orbits_gpu.py: m crosses both points-per-lane thresholds, n one tile and several chunks
OPTIONS = [dict(omega=0.0, coupling="field"), dict(omega=0.7, coupling="field"), dict(omega=0.7, coupling="step"),
           dict(omega=0.0, coupling="step")]


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
        D = (1, 3)[(idx + j) % 2]
        dev0 = _vectors(m, D, seed=100 + idx)
        # "step" multiplies the field by dt = 0.016: longer steps, so that the tracers still turn
        dt = DT_ if opt["coupling"] == "field" else 2.5
        kw = dict(dt=dt, steps=STEPS, every=EVERY, axis=AXIS, center=(0.1, -0.2, 0.05), **opt)
        o = sim.orbit_stability(pos, vel, deviations=dev0, renorm_log2=1, **kw)
        ref = _replay(nb, sim, pos, vel, dev0, renorm_log2=1, **kw)
        assert o.dev.shape == (4, m, D, 6) and o.log2.shape == (4, m, D) and o.growth.shape == (m, D)
        assert list(o.orbits.step) == [0, 2, 4, 5]
        _check_against(o, ref)
        # (tracer 0 starts on a body: where the frame's lines round its point a few 1e-9 off the body, the tensor's
        # fp32 pair term overflows as tidal_tensor()'s does, and the replay has the same NaN)
        assert np.isfinite(o.dev[:, 1:]).all()
        # renorm_log2 = 1: every state after the first is left with its largest component in [1, 2)
        mu = np.abs(o.dev[1:, 1:]).max(axis=-1)
        assert np.all(mu >= 1.0) and np.all(mu < 2.0) and np.all(o.growth["renorms"] <= STEPS)
        if D == 3:
            # (2^80 apart at the start; a tide moves the three exponents together)
            assert np.all(o.log2[1:, 1:, 1] - o.log2[1:, 1:, 2] >= 60) and np.all(o.log2[1:, 1:, 1] > o.log2[1:, 1:, 0])
        assert np.any(S.vectors({"dev": o.dev, "log2": o.log2})[-1, 1:, :, 3:] != dev0[1:, :, 3:], axis=-1).all()  # (a tide)
        assert _same_orbits(o.orbits, sim.orbits(pos, vel, **kw))
        st = o.stats
        assert (st.deviations, st.renorm_log2, st.renorms) == (D, 1, int(o.growth["renorms"].sum()))
        assert (st.orbit.records, st.orbit.pair_launches, st.orbit.flags, st.orbit.tracers) == (4, STEPS + 1, 0, m)
    sim.destroy()


# ---- 3. the first step against binary64 --------------------------------------------------------
@pytest.mark.parametrize("n,m", [(257, 65), (4099, 257)])
def test_first_step_against_binary64(gpu, n, m):
    """dv_1 - dv_0 = kappa_0 + kappa_1 = h T(p_0) dx_0 + h T(p_1) dx_1 against the binary64 tensor at the same two
    fp32 points: each component within h sum_b bound6_ab |dx_b| (tests/tidal_ref.py's BOUND: (64 + 33) 2^-24 of g sum
    |term| per sum, a diagonal component the bounds of S_aa and W) summed over the two evaluations, plus sixteen
    roundings of binary64 for the products, the sums and the two additions."""
    nb = gpu
    state = _state(n, seed=31)
    sim = _sim(nb, "naive", state)
    pos, vel = _tracers(state, m, seed=5)
    pos = pos.astype(np.float32).astype(np.float64)
    dev0 = np.random.default_rng(6).normal(size=(m, 2, 6))
    dt = 0.05
    o = sim.orbit_stability(pos, vel, deviations=dev0, dt=dt, steps=1, renorm_log2=512)
    sim.destroy()
    assert np.all(o.log2 == 0) and _same(o.dev[0], dev0)
    h = dt / 2
    idx = np.array([[0, 3, 4], [3, 1, 5], [4, 5, 2]])
    want, bound = np.zeros((m, 2, 3)), np.zeros((m, 2, 3))
    for r in (0, 1):
        t = T.tidal64(state, o.orbits.pos[r].astype(np.float32), G, E)
        t6, b6 = t["tensor6"][:, idx], t["bound6"][:, idx]             # (m, 3, 3)
        dx = o.dev[r, :, :, 0:3]                                        # (m, 2, 3)
        terms = np.abs(t6[:, None] * dx[:, :, None, :]).sum(-1)
        want += h * (t6[:, None] * dx[:, :, None, :]).sum(-1)
        bound += h * (b6[:, None] * np.abs(dx[:, :, None, :])).sum(-1) + 16 * 2.0 ** -53 * h * terms
    bound += 16 * 2.0 ** -53 * (np.abs(o.dev[0, :, :, 3:]) + np.abs(o.dev[1, :, :, 3:]))
    err = np.abs((o.dev[1, :, :, 3:] - o.dev[0, :, :, 3:]) - want)
    print("first step: worst error / bound", (err / bound).max())
    assert np.all(err <= bound)
    assert np.abs(want).min() > 0


# ---- 4. the symplectic form on the device ------------------------------------------------------
def test_symplectic_form_over_200_steps(gpu):
    """|omega_k - omega_0| <= C K 2^-53 max_k(|d1| |d2|) with C = 1 at every state of 200 steps, n = 257, m = 65, for
    every tracer, on inputs for which the binary64 model of the same run stays below 0.1 (it measures 0.03)."""
    nb = gpu
    n, m, K = 257, 65, 200
    state = _state(n, seed=61)
    sim = _sim(nb, "naive", state)
    pos, vel = _tracers(state, m, seed=14)
    pos[0] += 0.05  # (not on a body)
    dev0 = np.broadcast_to(nb._default_deviations(2), (m, 2, 6)).copy()
    for omega in (0.0, 0.35):
        kw = dict(dt=0.02, steps=K, every=1, omega=omega, axis=AXIS, center=(0.1, 0.0, -0.1))
        o = sim.orbit_stability(pos, vel, deviations=dev0, **kw)
        sample, tensor = S.model64(state, G, E)
        ref = S.stability(sample, tensor, pos, vel, dev0, **kw)
        C_ref = S.symplectic_C(S.vectors(ref), K)
        C_dev = S.symplectic_C(S.vectors({"dev": o.dev, "log2": o.log2}), K)
        print("omega", omega, "symplectic C: reference max", C_ref.max(), "device max", C_dev.max())
        assert C_ref.max() <= 0.1
        assert np.all(C_dev <= 1.0)
    sim.destroy()


# ---- 5. determinism and places -----------------------------------------------------------------
@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_determinism_permutation_bands_and_nonfinite(gpu, kind):
    nb = gpu
    n, m, D = 4099, 257, 2
    state = _state(n, seed=41)
    state[1234, 4] = np.nan  # a NaN body: left out and counted
    sim = _sim(nb, kind, state)
    pos, vel = _tracers(state[np.isfinite(state).all(1)], m, seed=6)
    dev0 = _vectors(m, D, seed=7)
    kw = dict(dt=DT_, steps=STEPS, every=EVERY, omega=0.7, axis=AXIS, renorm_log2=4)
    a = sim.orbit_stability(pos, vel, deviations=dev0, **kw)
    assert _same_stability(a, sim.orbit_stability(pos, vel, deviations=dev0, **kw))
    perm = np.random.default_rng(7).permutation(m)
    p = sim.orbit_stability(pos[perm], vel[perm], deviations=dev0[perm], **kw)
    assert _same(p.dev, a.dev[:, perm]) and np.array_equal(p.log2, a.log2[:, perm])
    assert p.growth.tobytes() == np.ascontiguousarray(a.growth[perm]).tobytes() and _same(p.orbits.pos, a.orbits.pos[:, perm])
    # bands: 2^16 pairs are less than one tile of tracers against 4099 bodies, so every tile is a launch
    sim.set_tuning("field_launch_pairs_log2", 16)
    b = sim.orbit_stability(pos, vel, deviations=dev0, **kw)
    sim.set_tuning("field_launch_pairs_log2", 35)
    assert _same_stability(a, b)
    assert a.stats.orbit.pair_launches == STEPS + 1 and b.stats.orbit.pair_launches > 2 * a.stats.orbit.pair_launches - 1
    assert a.stats.orbit.nonfinite == b.stats.orbit.nonfinite == 1 and a.stats.orbit.nonfinite_tracers == 0
    # a NaN tracer: NaN vectors, its neighbours bit for bit
    dirty = pos.copy()
    dirty[100, 1] = np.nan
    d = sim.orbit_stability(dirty, vel, deviations=dev0, **kw)
    ok = np.arange(m) != 100
    assert d.stats.orbit.nonfinite_tracers == 1 and np.isnan(d.dev[:, 100]).all() and np.all(d.log2[:, 100] == 0)
    assert np.all(d.growth["renorms"][100] == 0) and np.all(d.growth["peak_step"][100] == np.uint64(2 ** 64 - 1))
    assert _same(d.dev[:, ok], a.dev[:, ok]) and np.array_equal(d.log2[:, ok], a.log2[:, ok])
    assert d.growth[ok].tobytes() == a.growth[ok].tobytes()
    # a tracer thrown out of fp32's range: its vectors are NaN from there on, and only its
    far_v = vel.copy()
    far_v[7] = (1e41, 0.0, 0.0)  # x_1 = 2e39, not an fp32 number
    f = sim.orbit_stability(pos, far_v, deviations=dev0, **kw)
    assert np.isfinite(f.dev[0, 7]).all() and np.isnan(f.dev[1:, 7, :, 3:]).all()
    ok = np.arange(m) != 7
    assert _same(f.dev[:, ok], a.dev[:, ok])
    # the NaN body is left out: the replay through field() and tidal_tensor(), which leave it out, is the same
    _check_against(a, _replay(nb, sim, pos, vel, dev0, **kw))
    sim.destroy()


# ---- 6. continuation ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(257, 65), (4099, 257)])
def test_continuation_is_exact(gpu, n, m):
    nb = gpu
    state = _state(n, seed=51)
    sim = _sim(nb, "naive", state)
    pos, vel = _tracers(state, m, seed=8)
    dev0 = _vectors(m, 3, seed=9)
    kw = dict(dt=DT_, every=3, omega=0.7, axis=AXIS, center=(0.1, 0.0, -0.1), renorm_log2=2)
    whole = sim.orbit_stability(pos, vel, deviations=dev0, steps=6, step0=11, **kw)
    first = sim.orbit_stability(pos, vel, deviations=dev0, steps=3, step0=11, **kw)
    x, v, dev, log2, step = first.final()
    assert step == 14
    second = sim.orbit_stability(x, v, deviations=dev, log2_0=log2, steps=3, step0=step, **kw)
    sim.destroy()
    assert _same(whole.dev[:2], first.dev) and _same(whole.dev[1:], second.dev)
    assert np.array_equal(whole.log2[:2], first.log2) and np.array_equal(whole.log2[1:], second.log2)
    assert _same(whole.orbits.pos[1:], second.orbits.pos) and _same(whole.orbits.vel[1:], second.orbits.vel)
    assert np.array_equal(np.maximum(first.growth["peak_log2"], second.growth["peak_log2"]), whole.growth["peak_log2"])
    assert np.array_equal(first.growth["renorms"] + second.growth["renorms"], whole.growth["renorms"])
    assert np.any(whole.log2[-1] != 0)
    # the growth since the whole run's start, from the continuation's records and the first run's vectors
    lg = whole.log_growth()[-1]
    assert np.allclose(second.log_growth()[-1] + first.log_growth()[-1], lg, rtol=0, atol=1e-12 * (1 + np.abs(lg).max()))


# ---- 7. no bodies ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_no_bodies_gives_straight_lines(gpu, kind):
    nb = gpu
    sim = _sim(nb, kind, np.zeros((0, 10), np.float32))
    rng = np.random.default_rng(9)
    pos, vel, dev0 = rng.normal(size=(65, 3)), rng.normal(size=(65, 3)), rng.normal(size=(65, 2, 6))
    for omega in (0.0, 0.7):
        o = sim.orbit_stability(pos, vel, deviations=dev0, dt=0.3, steps=STEPS, every=EVERY, omega=omega, axis=AXIS)
        dx, rows = dev0[:, :, :3].copy(), {}
        for k in range(STEPS + 1):
            rows[k] = dx
            dx = dx + (dev0[:, :, 3:] + 0.0) * 0.3
        for r, k in enumerate((0, 2, 4, 5)):
            assert _same(o.dev[r, :, :, :3], rows[k]) and _same(o.dev[r, :, :, 3:], dev0[:, :, 3:]), (omega, k)
        assert np.all(o.log2 == 0) and np.all(o.growth["renorms"] == 0)
        assert (o.stats.orbit.n, o.stats.orbit.pair_launches, o.stats.orbit.records) == (0, 0, 4)
        assert _same_orbits(o.orbits, sim.orbits(pos, vel, dt=0.3, steps=STEPS, every=EVERY, omega=omega, axis=AXIS))
    o = sim.orbit_stability(np.zeros((0, 3)), np.zeros((0, 3)), dt=0.3, steps=2, every=1)  # m = 0 is valid
    assert o.dev.shape == (3, 0, 2, 6) and o.stats.orbit.tracers == 0
    sim.destroy()


# ---- 8. does not perturb the trajectory --------------------------------------------------------
@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_does_not_perturb_the_trajectory(gpu, kind):
    nb = gpu
    state = make_state("uniform", 4096, seed=9)
    pos, vel = _tracers(state, 300, seed=12)
    finals = []
    for with_pass in (False, True):
        sim = _sim(nb, kind, state)
        for k in range(3):
            sim.encode()
            if with_pass:
                o = sim.orbit_stability(pos, vel, dt=DT_, steps=3, deviations=1 + k, omega=0.7 * (k != 2))
                assert o.stats.orbit.step_num == k + 1 and sim.step_num() == k + 1
        finals.append(nb.as_floats(sim.read_particles()).copy())
        sim.destroy()
    assert np.array_equal(finals[0].view(np.uint32), finals[1].view(np.uint32))


# ---- 9. the runner, the refusals that need a simulator, the CLI ----------------------------------
def test_refusals_and_the_runner(gpu):
    nb = gpu
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    s = make_state("uniform", 64, seed=1)
    pos, vel = _tracers(s, 8, seed=1)
    sharded = nb.NaiveSim.from_particles(nb.SimParams(particle_num=64), None, s, placement=nb.Placement(world=2))
    with pytest.raises(nb.NBodyError) as ex:
        sharded.orbit_stability(pos, vel, dt=DT_, steps=2)
    assert ex.value.code == _lib.NB_ERR_UNSUPPORTED and b"sharded" in L.nb_last_error()
    sharded.destroy()
    r = nb.OfflineHeadless(nb.NaiveSim, nb.SimParams(particle_num=512), None,
                           lambda p: nb.inits.uniform_init(p, seed=1), device_ids=[0, 0])
    with pytest.raises(nb.NBodyError) as ex:
        r.orbit_stability(pos, vel, dt=DT_, steps=2)
    assert ex.value.code == _lib.NB_ERR_UNSUPPORTED
    r.destroy()
    sim = _sim(nb, "naive", s)
    for d in (0, 7):
        with pytest.raises(nb.NBodyError) as ex:
            sim.orbit_stability(pos, vel, dt=DT_, steps=2, deviations=d)
        assert ex.value.code == _lib.NB_ERR_INVALID and "deviations" in str(ex.value)
    with pytest.raises(nb.NBodyError) as ex:
        sim.orbit_stability(pos, vel, dt=DT_, steps=2, deviations=np.zeros((8, 7, 6)))
    assert ex.value.code == _lib.NB_ERR_INVALID
    with pytest.raises(ValueError):
        sim.orbit_stability(pos, vel, dt=DT_, steps=2, deviations=np.zeros((7, 2, 6)))
    # the energy flag, which the Python call never sets: through the C entry point, on a live simulator
    p = _lib.nb_orbit_params()
    p.dt, p.steps, p.every, p.flags, p.accel_scale = DT_, 2, 2, _lib.NB_ORBIT_ENERGY, 1.0
    p.axis[:] = (0.0, 1.0, 0.0)
    sp = _lib.nb_orbit_stability_params(1, 32, 0)
    dev0 = np.zeros((8, 1), _lib.ORBIT_DEVIATION_DTYPE)
    tracks, devs = np.zeros((2, 8), _lib.ORBIT_SAMPLE_DTYPE), np.zeros((2, 8, 1), _lib.ORBIT_DEVIATION_DTYPE)
    assert L.nb_orbit_stability_sim(sim._h, C.byref(p), C.byref(sp), pos.ctypes.data, vel.ctypes.data, 8,
                                    dev0.ctypes.data, tracks.ctypes.data, None, devs.ctypes.data, None,
                                    None) == _lib.NB_ERR_INVALID and b"NB_ORBIT_ENERGY" in L.nb_last_error()
    # a softening below zero is no obstacle without the potential
    sim.destroy()
    big = _sim(nb, "naive", make_state("uniform", 1 << 18, seed=2))
    with pytest.raises(nb.NBodyError) as ex:  # 256 padded tracers x 2^18 bodies x (2^20 + 1) evaluations
        big.orbit_stability(np.zeros((200, 3)), np.zeros((200, 3)), dt=DT_, steps=1 << 20)
    assert ex.value.code == _lib.NB_ERR_UNSUPPORTED and "split" in str(ex.value)
    big.destroy()
    # nb_orbit_stability_runner is nb_orbit_stability_sim of the runner's simulator
    r = nb.OfflineHeadless(nb.TreeSim, nb.SimParams(particle_num=2048), nb.AddParams.TreeSimParams(0.75),
                           lambda p: nb.inits.disc_init(p, seed=2))
    r.step()
    state = nb.as_floats(r.read_particles())
    pos, vel = _tracers(state, 100, seed=13)
    kw = dict(dt=DT_, steps=STEPS, every=EVERY, omega=0.7, coupling="step", deviations=3)
    a, b = r.orbit_stability(pos, vel, **kw), r.sim.orbit_stability(pos, vel, **kw)
    r.destroy()
    assert _same_stability(a, b) and a.stats == b.stats and a.stats.orbit.step_num == 1
    assert a.lyapunov().shape == (100, 3) and a.sali().shape == (4, 100) and a.chaotic().shape == (100,)
    assert np.all(a.sali()[0] > 1.0) and np.allclose(a.gali2()[0], 1.0)  # (orthonormal at the start)


def test_cli_stability(gpu, tmp_path):
    """headless --stability (the C++ mirror's orbit_stability over nb_orbit_stability_runner, and its derive()) writes
    what the Python runner computes for the same tracers and vectors, bit for bit."""
    nb = gpu
    cli = os.path.join(ROOT, "wgpu_n_body_amd", "headless")
    p = subprocess.run([cli, "--sim", "tree", "--n", "2048", "--init", "disc", "--steps", "3", "--stability",
                        str(tmp_path), "--stability-at", "2", "--stability-range", "0.2,1.2", "--stability-bins", "6",
                        "--stability-dt", "0.05", "--stability-steps", "40", "--stability-omega", "0.4",
                        "--stability-speed", "0.9", "--stability-axis", "0,0,1"], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("stability ")]
    assert len(lines) == 1 and lines[0][1:3] == ["2", "6"] and lines[0][4] == "41", p.stdout
    got = np.load(tmp_path / "stability_000002.npy")
    assert got.shape == (6, 6) and got.dtype == np.float64
    runner = nb.OfflineHeadless(nb.TreeSim, nb.SimParams(particle_num=2048), nb.AddParams.TreeSimParams(0.75),
                                lambda sp: nb.inits.disc_init(sp, seed=0))
    runner.step()
    runner.step()
    radii = [0.2 + (1.2 - 0.2) * i / 5 for i in range(6)]
    launch = runner.circular_orbits(radii, dt=0.05, steps=1, omega=0.4, speed=0.9, axis=(0, 0, 1))
    pos, vel = launch.pos[0], launch.vel[0]
    n, e1, e2 = nb.map_frame((0, 0, 1))
    d = pos - 0.0
    l = (d[:, 0] * n[0] + d[:, 1] * n[1]) + d[:, 2] * n[2]
    d = d - l[:, None] * n
    d = d / np.sqrt((d * d).sum(1))[:, None]
    dev0 = np.zeros((6, 2, 6))
    dev0[:, 0, :3], dev0[:, 1, :3] = d, n
    o = runner.orbit_stability(pos, vel, deviations=dev0, dt=0.05, steps=40, omega=0.4, axis=(0, 0, 1))
    runner.destroy()
    ours = np.stack([o.lyapunov()[:, 0], o.lyapunov()[:, 1], o.sali()[-1], o.gali2()[-1],
                     o.growth["peak_log2"][:, 0].astype(np.float64), o.growth["peak_step"][:, 0].astype(np.float64)],
                    axis=1)
    assert _same(got, ours)
    assert np.isfinite(ours).all() and int(lines[0][3]) == o.stats.renorms
    p = subprocess.run([cli, "--sim", "naive", "--n", "256", "--steps", "2"], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and "stability" not in p.stdout
