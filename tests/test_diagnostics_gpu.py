"""nb_sim_diagnostics on the device (csrc/nb_diag.hip): every field against fp64 host sums of the
read-back state (tests/diag_ref.py), on both simulators, at sizes that cut the 256-body tiles
anywhere; a closed-form two-body case; bitwise reproducibility; that a call does not perturb the
trajectory; the physics (energy tracking an fp64 all-pairs run); the refusals; the CLI.  `-m gpu`."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.diag_ref import energy64, moments64, pair_sum64, psi64
from tests.helpers import DT, E, G, ROOT, make_state

pytestmark = pytest.mark.gpu

E64 = np.float64(np.float32(E))  # the softening the device sees


def _sim(nb, kind, state, sp, theta=0.75):
    if kind == "naive":
        return nb.NaiveSim.from_particles(sp, None, state)
    return nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(theta), state)


def _raw(sim, flags):
    from wgpu_n_body_amd import _lib
    d = _lib.nb_diagnostics()
    rc = _lib.lib().nb_sim_diagnostics(sim._h, flags, C.byref(d))
    return rc, d


def _check_moments(d, state, tol=1e-10):
    ref = moments64(state)
    sc = ref["scale"]
    assert d.n == state.shape[0] and d.nonfinite == ref["nonfinite"]
    assert abs(d.mass - ref["mass"]) <= tol * sc["mass"]
    assert np.all(np.abs(d.com * d.mass - ref["mx"]) <= tol * sc["mx"] + 1e-300)
    for k in ("momentum", "angular_momentum"):
        assert np.all(np.abs(getattr(d, k) - ref[k]) <= tol * sc[k] + 1e-300), (k, getattr(d, k), ref[k])
    assert abs(d.kinetic - ref["kinetic"]) <= tol * sc["kinetic"]
    assert abs(d.max_speed - ref["max_speed"]) <= 1e-12 * ref["max_speed"]


def test_two_body_known_answer(gpu):
    nb = gpu
    sp = nb.SimParams(particle_num=2)
    s = np.zeros((2, 10), np.float32)
    s[0, 0:3], s[0, 3:6], s[0, 9] = (0.25, 0.0, 0.0), (0.0, 0.5, 0.0), 2.0
    s[1, 0:3], s[1, 3:6], s[1, 9] = (-0.25, 0.0, 0.0), (0.0, -0.25, 0.125), 3.0
    for kind in ("naive", "tree"):
        sim = _sim(nb, kind, s, sp)
        d = sim.diagnostics(potential=True)
        sim.destroy()
        x = s[:, 0:3].astype(np.float64)
        v = s[:, 3:6].astype(np.float64)
        m = s[:, 9].astype(np.float64)
        assert d.step_num == 0 and d.n == 2 and d.nonfinite == 0
        assert d.flags == 3
        assert d.mass == 5.0
        close = lambda a, b: np.allclose(a, b, rtol=1e-12, atol=1e-15)  # noqa: E731
        assert close(d.com, (m[:, None] * x).sum(0) / 5.0) and close(d.com, [-0.05, 0, 0])
        assert close(d.momentum, [0.0, 0.25, 0.375])
        assert close(d.angular_momentum, (m[:, None] * np.cross(x, v)).sum(0))
        assert close(d.kinetic, 0.5 * 2 * 0.25 + 0.5 * 3 * (0.0625 + 0.015625))
        assert close(d.max_speed, 0.5)
        w = 6.0 * psi64(np.array([0.5]), E64)[0]
        assert abs(d.pair_sum / w - 1) < 2e-6, (d.pair_sum, w)
        u = -np.float64(np.float32(G)) * np.float64(np.float32(DT)) * d.pair_sum
        assert d.potential == u and d.total == d.kinetic + u
    # without the flag: NaN
    sim = _sim(nb, "naive", s, sp)
    d = sim.diagnostics()
    sim.destroy()
    assert d.flags == 1 and np.isnan(d.pair_sum) and np.isnan(d.potential) and np.isnan(d.total)


@pytest.mark.parametrize("kind", ["naive", "tree"])
@pytest.mark.parametrize("init", ["uniform", "disc", "spherical"])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 65, 1000, 4097, 8192])
def test_against_host_fp64(gpu, kind, init, n):
    nb = gpu
    sp = nb.SimParams(particle_num=n)
    state = make_state(init, n, seed=n + 7)
    sim = _sim(nb, kind, state, sp)
    for steps in (0, 3):
        if steps:
            for _ in range(steps):
                sim.encode()
        d = sim.diagnostics(potential=True)
        got = nb.as_floats(sim.read_particles())
        assert d.step_num == steps
        _check_moments(d, got)
        w = pair_sum64(got, E64)
        assert abs(d.pair_sum - w) <= 2e-6 * abs(w), (steps, d.pair_sum, w)
        if n == 1:
            assert d.pair_sum == 0.0
    sim.destroy()


def test_large_tree_in_the_gather_range(gpu):
    """2^20 bodies: from 524,288 the walk gathers and the state changes buffer set every step -- the
    diagnostics must read the buffer read_particles converts, not a stale one."""
    nb = gpu
    n = 1 << 20
    sp = nb.SimParams(particle_num=n)
    state = make_state("uniform", n, seed=11)
    sim = _sim(nb, "tree", state, sp)
    for steps in (1, 2):
        sim.encode()
        d = sim.diagnostics()
        got = nb.as_floats(sim.read_particles())
        assert d.step_num == steps
        _check_moments(d, got)
        # a stale buffer would hold the previous state: its kinetic energy differs
    sim.destroy()


def test_two_sims_same_state(gpu):
    nb = gpu
    n = 5000
    sp = nb.SimParams(particle_num=n)
    state = make_state("spherical", n, seed=5)
    a = _sim(nb, "naive", state, sp)
    b = _sim(nb, "tree", state, sp)
    da, db = a.diagnostics(potential=True), b.diagnostics(potential=True)
    a.destroy()
    b.destroy()
    assert abs(da.pair_sum - db.pair_sum) <= 2e-6 * abs(da.pair_sum)
    assert abs(da.kinetic - db.kinetic) <= 1e-12 * abs(da.kinetic)


@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_bitwise_reproducible(gpu, kind):
    nb = gpu
    n = 4097
    sp = nb.SimParams(particle_num=n)
    sim = _sim(nb, kind, make_state("disc", n, seed=2), sp)
    sim.encode()
    rc1, d1 = _raw(sim, 3)
    rc2, d2 = _raw(sim, 3)
    rc3, d3 = _raw(sim, 1)
    sim.destroy()
    assert rc1 == rc2 == rc3 == 0
    assert bytes(d1) == bytes(d2)
    # the moments do not depend on whether the potential was asked for
    for f in ("mass", "kinetic", "max_speed", "nonfinite"):
        assert getattr(d1, f) == getattr(d3, f)
    assert list(d1.momentum) == list(d3.momentum) and list(d1.angular_momentum) == list(d3.angular_momentum)


@pytest.mark.parametrize("case", ["naive", "tree", "tree_graph", "tree_gather"])
def test_does_not_perturb_the_trajectory(gpu, case):
    nb = gpu
    n = 600_000 if case == "tree_gather" else 4096
    sp = nb.SimParams(particle_num=n)
    state = make_state("uniform", n, seed=9)
    finals = []
    for with_diag in (False, True):
        sim = _sim(nb, "naive" if case == "naive" else "tree", state, sp)
        if case == "tree_graph":
            sim.set_tuning("tree_use_graph", 1)
        for _ in range(10):
            sim.encode()
            if with_diag:
                d = sim.diagnostics(potential=True)
                assert np.isfinite(d.total)
        finals.append(nb.as_floats(sim.read_particles()).copy())
        sim.destroy()
    assert np.array_equal(finals[0].view(np.uint32), finals[1].view(np.uint32))


@pytest.mark.parametrize("case", ["disc_tree", "uniform_naive"])
def test_energy_tracks_an_fp64_run(gpu, oracle, case):
    """E from the device diagnostics against E computed on the host (fp64 psi) from the fp64 all-pairs
    oracle's states (oracle.naive_step_f64), 50 steps.

    Bound, measured on the CPU first (seed 3, |E_a - E_b| / (K + |U|), both energies from the host fp64
    sums, every step 0..50): the oracle's fp32 Barnes-Hut run (tree_step_f32, theta 0.75) against the
    fp64 all-pairs run, 2,048-body disc, g = 1e-5, dt = 0.0016 (visualize.rs): 2.2e-7 worst; the
    oracle's fp32 all-pairs run, 4,096-body uniform, default params: 3.8e-9 worst.  Over those 50 steps
    E itself moves by 1.0e-4 (disc) and 4e-7 (uniform) of K + |U|.  The device adds the pair sum's own
    error (W to 2e-6, tested above), so the bound is 2e-6 + 4 x the measured trajectory difference."""
    nb = gpu
    if case == "disc_tree":
        n, g, dt, kind, init, measured = 2048, 1e-5, 0.0016, "tree", "disc", 2.2e-7
    else:
        n, g, dt, kind, init, measured = 4096, G, DT, "naive", "uniform", 3.8e-9
    bound = 2e-6 + 4 * measured
    sp = nb.SimParams(particle_num=n, g=g, e=E, dt=dt)
    fn = {"disc": nb.inits.disc_init, "uniform": nb.inits.uniform_init}[init]
    state = nb.as_floats(fn(sp, seed=3)).copy()
    sim = _sim(nb, kind, state, sp, theta=0.75)
    ref = state.astype(np.float64)
    worst = 0.0
    for k in range(51):
        if k:
            sim.encode()
            ref = oracle.naive_step_f64(ref, g, E, dt)
        if k % 10 == 0 or k == 25:
            d = sim.diagnostics(potential=True)
            kk, uu, ee = energy64(ref.astype(np.float32), g, E, dt)
            worst = max(worst, abs(d.total - ee) / (kk + abs(uu)))
    sim.destroy()
    assert worst < bound, (worst, bound)


def test_nonfinite_body_is_counted_and_left_out(gpu):
    nb = gpu
    n = 1000
    sp = nb.SimParams(particle_num=n)
    state = make_state("uniform", n, seed=4)
    state[137, 4] = np.nan
    sim = _sim(nb, "naive", state, sp)
    d = sim.diagnostics(potential=True)
    sim.destroy()
    assert d.nonfinite == 1
    assert all(np.isfinite(x) for x in (d.mass, d.kinetic, d.max_speed, d.pair_sum, d.total))
    assert np.isfinite(d.momentum).all() and np.isfinite(d.angular_momentum).all()
    _check_moments(d, state)
    w = pair_sum64(state, E64)
    assert abs(d.pair_sum - w) <= 2e-6 * abs(w)


def test_zero_softening_and_coincident_bodies(gpu):
    nb = gpu
    s = np.zeros((3, 10), np.float32)
    s[:, 9] = 1.0
    s[2, 0] = 1.0  # bodies 0 and 1 coincide
    d = _sim(nb, "naive", s, nb.SimParams(particle_num=3, e=0.0)).diagnostics(potential=True)
    assert d.pair_sum == np.inf
    d = _sim(nb, "naive", s, nb.SimParams(particle_num=3)).diagnostics(potential=True)
    a2 = np.cbrt(E64) ** 2
    w = 2 * np.pi / (3 * np.sqrt(3) * a2) + 2 * psi64(np.array([1.0]), E64)[0]
    assert abs(d.pair_sum / w - 1) < 2e-6


def test_refusals(gpu):
    nb = gpu
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    s = make_state("uniform", 64, seed=1)
    sim = _sim(nb, "naive", s, nb.SimParams(particle_num=64, e=-1e-4))
    rc, _ = _raw(sim, 3)
    assert rc == _lib.NB_ERR_INVALID
    rc, _ = _raw(sim, 1)  # the moments need no e >= 0
    assert rc == 0
    rc, _ = _raw(sim, 4)
    assert rc == _lib.NB_ERR_INVALID
    sim.destroy()
    # a sharded simulator (rank 0 of 2)
    sharded = nb.NaiveSim.from_particles(nb.SimParams(particle_num=64), None, s, placement=nb.Placement(world=2))
    rc, _ = _raw(sharded, 1)
    assert rc == _lib.NB_ERR_UNSUPPORTED and b"sharded" in L.nb_last_error()
    sharded.destroy()
    # a several-GPU runner, both ranks on device 0
    r = nb.OfflineHeadless(nb.NaiveSim, nb.SimParams(particle_num=512), None,
                           lambda p: nb.inits.uniform_init(p, seed=1), device_ids=[0, 0])
    with pytest.raises(nb.NBodyError) as ex:
        r.diagnostics()
    assert ex.value.code == _lib.NB_ERR_UNSUPPORTED
    r.destroy()


def test_runner_diagnostics_and_cli(gpu, tmp_path):
    nb = gpu
    cli = os.path.join(ROOT, "wgpu_n_body_amd", "headless")
    p = subprocess.run([cli, "--sim", "naive", "--n", "1024", "--steps", "4", "--diag", "2", "--diag-potential", "1"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("Diagnostics: ")]
    assert len(lines) == 3
    assert len([ln for ln in p.stdout.splitlines() if ln.startswith("Step Duration: ")]) == 4
    num = r"(\S+)"
    pat = re.compile(r"Diagnostics: step (\d+) kinetic {0} potential {0} total {0} momentum {0} {0} {0} "
                     r"angular_momentum {0} {0} {0}$".format(num))
    runner = nb.OfflineHeadless(nb.NaiveSim, nb.SimParams(particle_num=1024), None,
                                lambda sp: nb.inits.uniform_init(sp, seed=0))
    ours = [runner.diagnostics(potential=True)]
    for k in range(4):
        runner.step()
        if (k + 1) % 2 == 0:
            ours.append(runner.diagnostics(potential=True))
    runner.destroy()
    for ln, d in zip(lines, ours):
        m = pat.match(ln)
        assert m, ln
        vals = [float(x) for x in m.groups()[1:]]
        assert int(m.group(1)) == d.step_num
        want = [d.kinetic, d.potential, d.total, *d.momentum, *d.angular_momentum]
        for a, b in zip(vals, want):
            assert abs(a - b) <= 1e-9 * abs(b) + 1e-300, (ln, want)
    # without --diag the output has no such line
    p = subprocess.run([cli, "--sim", "naive", "--n", "256", "--steps", "2"], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and "Diagnostics" not in p.stdout
