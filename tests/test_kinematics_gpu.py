"""nb_local_kinematics_sim on the device (csrc/nb_kinematics.hip) against the numpy restatements of its rule
(tests/kinematics_ref.py) on the read-back state: every per-body double and integer equal, no tolerance on the
device's sums; states short of k, lattices, coincident bodies, zero extents, an outlier, cell borders, non-finite
bodies; a large case against a sample; equality with nb_sim_knn; the tuning keys; reproducibility; permutations; null
outputs and refusals; the trajectory; the runner, the CLI and the Python mirror; an exact linear flow; a cold clump
in a hot sphere.  `-m gpu`."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from tests import kinematics_ref as R
from tests import knn_ref as K
from tests.helpers import ROOT, make_state

pytestmark = pytest.mark.gpu

FILL = 0xDEADBEEF


def _sim(nb, kind, state, theta=0.75):
    sp = nb.SimParams(particle_num=state.shape[0])
    if kind == "naive":
        return nb.NaiveSim.from_particles(sp, None, state)
    return nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(theta), state)


def _raw(sim, k, grad=True, include_self=True, call=None, handle=None, n=None, flags=None, reserved=0):
    """The C call with every buffer pre-filled."""
    from wgpu_n_body_amd import _lib
    n = int(sim.sim_params().particle_num) if n is None else n
    p = _lib.nb_kin_params()
    p.k, p.reserved = k, reserved
    p.flags = (_lib.NB_KIN_SELF if include_self else 0) if flags is None else flags
    mom, gr = np.full(10 * n + 1, -7.0), np.full(15 * n + 1, -7.0)
    r2, mass_in, density = np.full(n + 1, -7.0), np.full(n + 1, -7.0), np.full(n + 1, -7.0)
    kth = np.full(n + 1, FILL, np.uint32)
    st = _lib.nb_kin_stats()
    rc = (call or _lib.lib().nb_local_kinematics_sim)(
        handle or sim._h, C.byref(p), mom.ctypes.data, gr.ctypes.data if grad else None, r2.ctypes.data,
        kth.ctypes.data, mass_in.ctypes.data, density.ctypes.data, C.byref(st))
    bufs = (mom, gr, r2, kth, mass_in, density)
    return SimpleNamespace(rc=rc, n=n, moments=mom[:10 * n].reshape(n, 10), grads=gr[:15 * n].reshape(n, 15), r2=r2[:n],
                           kth=kth[:n], mass_in=mass_in[:n], density=density[:n], st=st, grad=grad,
                           tail=(mom[-1], gr[-1], r2[n], kth[n], mass_in[n], density[n]),
                           untouched=all(np.all(b == (FILL if b is kth else -7.0)) for b in bufs),
                           bytes=b"".join(b.tobytes() for b in bufs) + bytes(st))


def _kin(sim, k, **kw):
    from wgpu_n_body_amd import _lib
    g = _raw(sim, k, **kw)
    assert g.rc == 0, _lib.lib().nb_last_error()
    assert g.tail == (-7.0, -7.0, -7.0, FILL, -7.0, -7.0)  # n rows each, no more
    if not g.grad:
        assert np.all(g.grads == -7.0)
    return g


def _knn_raw(sim, k):
    from wgpu_n_body_amd import _lib
    n = int(sim.sim_params().particle_num)
    p = _lib.nb_knn_params()
    p.k = k
    r2, mass_in, density, kth = np.full(n, -7.0), np.full(n, -7.0), np.full(n, -7.0), np.full(n, FILL, np.uint32)
    assert _lib.lib().nb_sim_knn(sim._h, C.byref(p), r2.ctypes.data, kth.ctypes.data, mass_in.ctypes.data,
                                 density.ctypes.data, None) == 0
    return r2.tobytes() + kth.tobytes() + mass_in.tobytes() + density.tobytes()


def _same(a, b, what, sel):
    assert np.array_equal(a[sel], b[sel], equal_nan=True), (what, np.argwhere(~((a[sel] == b[sel]) | (a[sel] != a[sel])))[:6])


def _check(g, ref, include_self=True, sel=slice(None), stats=True):
    """Every per-body double and integer equal."""
    want = ref.moments.copy()
    want[:, 0] = ref.s0_self if include_self else ref.s0_noself
    _same(g.moments, want, "moments", sel)
    if g.grad:
        _same(g.grads, ref.grads, "grads", sel)
    _same(g.r2, ref.knn.r2, "r2", sel)
    _same(g.kth, ref.knn.kth, "kth", sel)
    _same(g.mass_in, ref.knn.mass_in, "mass_in", sel)
    _same(g.density, ref.knn.density, "density", sel)
    if stats:
        st = g.st
        got = (st.n, st.nonfinite, st.counted, st.degenerate, st.short_of_k, st.k)
        assert got == (ref.knn.n, ref.knn.nonfinite, ref.counted, ref.degenerate, ref.short_of_k, ref.k), got


def _state_of(nb, sim):
    return nb.as_floats(sim.read_particles()).copy()


def _prepared(nb, kind, state, step=True):
    """The simulator and the state it holds: a TreeSim after one step, in tree order."""
    sim = _sim(nb, kind, state)
    if kind == "tree" and step and state.shape[0] > 0:
        sim.encode()
    return sim, _state_of(nb, sim)


def _all_ways(sim, state, k):
    """With and without the gradient sums, with and without self, against one restatement."""
    ref = R.kin_vectorised(*K.split(state), k)
    for grad in (True, False):
        for include_self in (True, False):
            _check(_kin(sim, k, grad=grad, include_self=include_self), ref, include_self)
    return ref


@pytest.mark.parametrize("n", [0, 1, 2, 7, 63, 64, 65, 66, 1000])
@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_sizes(gpu, kind, n):
    """Every k against every n: c <= k, c = k + 1, and the 65-entry list (k = 64 with self)."""
    nb = gpu
    state0 = K.state_of(K.ball(np.random.default_rng(n), n, 1.0), n)
    sim, state = _prepared(nb, kind, state0)
    for k in (1, 2, 6, 32, 64):
        ref = _all_ways(sim, state, k)
        g = _kin(sim, k)
        assert g.st.short_of_k == (n if n <= k else 0)
        if 0 < n <= k:
            assert not g.moments.any() and not g.grads.any() and np.all(np.isinf(g.r2)) and np.all(g.kth == K.NONE)
        if n > k:
            assert np.all(ref.moments[:, 0] > 0.0)
            assert g.r2.tobytes() + g.kth.tobytes() + g.mass_in.tobytes() + g.density.tobytes() == _knn_raw(sim, k)
    sim.destroy()


CASES = K.synthetic_cases(small=False)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c[0] for c in CASES])
@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_synthetic_cases(gpu, kind, idx):
    nb = gpu
    name, state0, ks, steppable = CASES[idx]
    sim, state = _prepared(nb, kind, state0, step=steppable)
    for k in ks:
        ref = _all_ways(sim, state, k)
        if name == "one_point":  # every neighbour at the body itself: the sums are formed, every dx is 0
            assert ref.degenerate == 70 and not ref.grads[:, 0:6].any() and ref.moments[:, 4].any()
    sim.destroy()


@pytest.mark.parametrize("init", ["disc", "spherical"])
@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_nonfinite_bodies(gpu, kind, init):
    """NaN / inf positions, masses and velocities (a tree is not stepped over them: they go in after the step)."""
    nb = gpu
    sim, state0 = _prepared(nb, kind, make_state(init, 4096, seed=5))
    sim.destroy()
    state0 = K.inject_nonfinite(state0, 40, 3)
    sim = _sim(nb, kind, state0)
    state = _state_of(nb, sim)
    ok = K.counted_mask(*K.split(state))
    for k in (6, 32):
        _all_ways(sim, state, k)
        g = _kin(sim, k)
        assert g.st.nonfinite == 40 and np.all(np.isnan(g.moments[~ok])) and np.all(np.isnan(g.grads[~ok]))
        assert np.all(np.isfinite(g.moments[ok])) and np.all(np.isfinite(g.grads[ok]))
    sim.destroy()


def test_no_body_counts(gpu):
    nb = gpu
    state = K.state_of(np.full((300, 3), np.nan))
    sim = _sim(nb, "naive", state)
    g = _kin(sim, 6)
    _check(g, R.kin_vectorised(*K.split(state), 6))
    assert (g.st.counted, g.st.nonfinite, g.st.short_of_k) == (0, 300, 0) and np.all(np.isnan(g.moments))
    sim.destroy()


@pytest.mark.parametrize("kind,k", [("naive", 32), ("tree", 6)])
def test_large_case_against_a_sample(gpu, kind, k):
    """70,001 bodies: hundreds of blocks of every kernel.  The vectorised restatement for 512 seeded bodies against
    all bodies."""
    nb = gpu
    n = 70001
    sim, state = _prepared(nb, kind, make_state("spherical", n, seed=11))
    g = _kin(sim, k)
    knn_bytes = _knn_raw(sim, k)
    sim.destroy()
    sample = np.sort(np.random.default_rng(k).choice(n, 512, replace=False))
    ref = R.kin_vectorised(*K.split(state), k, queries=sample, rows=48)
    _check(g, ref, sel=sample, stats=False)
    assert (g.st.n, g.st.counted, g.st.nonfinite, g.st.short_of_k) == (n, n, 0, 0)
    assert g.st.degenerate == np.count_nonzero(g.r2 == 0.0)
    assert g.r2.tobytes() + g.kth.tobytes() + g.mass_in.tobytes() + g.density.tobytes() == knn_bytes
    assert np.all(np.isfinite(g.moments)) and np.all(np.isfinite(g.grads)) and np.all(g.moments[:, 0] > 0.0)


def test_tuning_keys_do_not_change_a_bit(gpu):
    """A crowded cell beside scattered bodies: every span and every cut of the work gives the default's bytes."""
    nb = gpu
    rng = np.random.default_rng(8)
    pos = np.concatenate([rng.uniform(0.0, 1e-6, (1500, 3)) + 0.25, K.ball(rng, 2500, 0.2, (0.25, 0.25, 0.25)),
                          [(40.0, 0.0, 0.0)]])
    state = K.state_of(pos[rng.permutation(4001)], 9)
    sim = _sim(nb, "naive", state)
    for k in (6, 64):
        base = _kin(sim, k)
        _check(base, R.kin_vectorised(*K.split(state), k))
        for span in range(1, 9):
            sim.set_tuning("knn_span_cells", span)
            assert _kin(sim, k).bytes == base.bytes, span
        sim.set_tuning("knn_span_cells", 3)
        for per in (1, 2, 4):
            sim.set_tuning("knn_block_queries", per)
            assert _kin(sim, k).bytes == base.bytes, per
            assert _kin(sim, k, grad=False).moments.tobytes() == base.moments.tobytes(), per
    sim.destroy()


@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_bitwise_reproducible(gpu, kind):
    nb = gpu
    sim, state = _prepared(nb, kind, make_state("disc", 4097, seed=2))
    g1, g2 = _kin(sim, 32), _kin(sim, 32)
    _kin(sim, 6, grad=False)  # another k and another kernel between
    nb_knn = _knn_raw(sim, 32)
    g3 = _kin(sim, 32)
    sim.destroy()
    assert g1.bytes == g2.bytes == g3.bytes
    assert g1.r2.tobytes() + g1.kth.tobytes() + g1.mass_in.tobytes() + g1.density.tobytes() == nb_knn


def _other_passes(sim):
    sim.diagnostics()
    sim.knn_density(6)
    sim.hop_groups(k_density=16, k_hop=8, k_merge=4)
    sim.fof_groups(0.02, min_members=2)


def test_workspaces_of_other_passes(gpu):
    """The result does not depend on which pass made its workspace first (nb_sim_knn's is shared)."""
    nb = gpu
    state = make_state("spherical", 3000, seed=4)
    sim = _sim(nb, "naive", state)
    first = _kin(sim, 6)
    _other_passes(sim)
    again = _kin(sim, 6)
    sim.destroy()
    sim = _sim(nb, "naive", state)
    _other_passes(sim)
    late = _kin(sim, 6)
    sim.destroy()
    assert first.bytes == again.bytes == late.bytes


def test_a_permutation_permutes_the_result(gpu):
    nb = gpu
    n, k = 1500, 6
    state = K.state_of(np.random.default_rng(6).normal(size=(n, 3)), 6)
    assert K.tie_free(K.knn_vectorised(*K.split(state), k), *K.split(state))
    perm = np.random.default_rng(4).permutation(n)  # body i of the permuted state is body perm[i]
    res = []
    for s in (state, state[perm]):
        sim = _sim(nb, "naive", s)
        res.append(_kin(sim, k))
        sim.destroy()
    a, b = res
    assert np.array_equal(b.moments, a.moments[perm]) and np.array_equal(b.grads, a.grads[perm])
    assert np.array_equal(b.r2, a.r2[perm]) and np.array_equal(perm[b.kth], a.kth[perm])


def test_null_outputs_and_refusals(gpu):
    nb = gpu
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    n = 2000
    state = make_state("spherical", n, seed=3)
    sim = _sim(nb, "naive", state)
    full = _kin(sim, 6)
    p = _lib.nb_kin_params()
    p.k, p.flags = 6, _lib.NB_KIN_SELF
    call = L.nb_local_kinematics_sim
    assert call(sim._h, C.byref(p), None, None, None, None, None, None, None) == 0
    st = _lib.nb_kin_stats()
    assert call(sim._h, C.byref(p), None, None, None, None, None, None, C.byref(st)) == 0
    assert bytes(st) == bytes(full.st)
    wants = (full.moments, full.grads, full.r2, full.kth, full.mass_in, full.density)
    for which in range(6):
        bufs = [np.full(10 * n + 1, -7.0), np.full(15 * n + 1, -7.0), np.full(n + 1, -7.0),
                np.full(n + 1, FILL, np.uint32), np.full(n + 1, -7.0), np.full(n + 1, -7.0)]
        args = [b.ctypes.data if j == which else None for j, b in enumerate(bufs)]
        assert call(sim._h, C.byref(p), *args, None) == 0
        assert np.array_equal(bufs[which][:-1], wants[which].ravel()) and bufs[which][-1] in (-7.0, FILL), which
    # refused calls write nothing
    for k, flags, reserved in ((0, 1, 0), (65, 1, 0), (6, 2, 0), (6, 1, 1)):
        g = _raw(sim, k, flags=flags, reserved=reserved)
        assert g.rc == _lib.NB_ERR_INVALID and L.nb_last_error() and g.untouched
        assert bytes(g.st) == bytes(_lib.nb_kin_stats())
    with pytest.raises(nb.NBodyError) as ex:
        sim.local_kinematics(0)
    assert ex.value.code == _lib.NB_ERR_INVALID
    assert _kin(sim, 6).bytes == full.bytes  # the simulator stays usable
    sim.destroy()
    # a sharded simulator (rank 0 of 2)
    s = make_state("uniform", 64, seed=1)
    sharded = nb.NaiveSim.from_particles(nb.SimParams(particle_num=64), None, s, placement=nb.Placement(world=2))
    g = _raw(sharded, 6, n=64)
    assert g.rc == _lib.NB_ERR_UNSUPPORTED and b"sharded" in L.nb_last_error() and g.untouched
    sharded.destroy()
    # a several-GPU runner, both ranks on device 0
    r = nb.OfflineHeadless(nb.NaiveSim, nb.SimParams(particle_num=512), None,
                           lambda sp: nb.inits.uniform_init(sp, seed=1), device_ids=[0, 0])
    with pytest.raises(nb.NBodyError) as ex:
        r.local_kinematics(6)
    assert ex.value.code == _lib.NB_ERR_UNSUPPORTED
    r.destroy()


@pytest.mark.parametrize("case", ["naive", "tree", "tree_graph"])
def test_does_not_perturb_the_trajectory(gpu, case):
    nb = gpu
    n, steps = 4096, 10
    state = make_state("uniform", n, seed=9)
    finals = []
    for with_pass in (False, True):
        sim = _sim(nb, "naive" if case == "naive" else "tree", state)
        if case == "tree_graph":
            sim.set_tuning("tree_use_graph", 1)
        for j in range(steps):
            sim.encode()
            if with_pass:
                d = sim.local_kinematics(6 if j % 2 else 32, gradient=j % 3 != 0)
                assert d.stats.step_num == j + 1 and d.stats.counted == n
        finals.append(nb.as_floats(sim.read_particles()).copy())
        sim.destroy()
    assert np.array_equal(finals[0].view(np.uint32), finals[1].view(np.uint32))


def test_python_wrapper(gpu):
    """The Python mirror end to end: the raw call's arrays, and nb_local_kinematics_derive's rows as the numpy
    restatement of the derive rule makes them."""
    nb = gpu
    state = make_state("disc", 4096, seed=0)
    sim = _sim(nb, "naive", state)
    d = sim.local_kinematics(gradient=True, neighbours=True)
    g = _kin(sim, 32)
    assert d.k == 32 and np.array_equal(d.moments, g.moments) and np.array_equal(d.grads, g.grads)
    assert np.array_equal(d.r2, g.r2) and np.array_equal(d.kth, g.kth) and np.array_equal(d.density, g.density)
    assert np.array_equal(d.r_k, np.sqrt(g.r2)) and d.stats.counted == 4096 and d.stats.k == 32
    want = R.derive_ref(g.moments, g.grads, g.r2, g.density, state[:, 3:6])
    for name, got in (("mass", d.mass), ("mean_velocity", d.mean_velocity), ("relative_velocity", d.relative_velocity),
                      ("sigma", d.sigma), ("phase_space_density", d.phase_space_density), ("status", d.status),
                      ("gradient", d.velocity_gradient.reshape(-1, 9)), ("divergence", d.divergence),
                      ("vorticity", d.vorticity), ("shear", d.shear)):
        assert np.array_equal(got, want[name], equal_nan=True), name
    assert np.array_equal(d.dispersion_tensor[:, 1, 2], want["dispersion"][:, 4])
    assert np.array_equal(d.dispersion_tensor[:, 2, 1], want["dispersion"][:, 4])
    flat = (d.status & nb.KIN_SINGULAR) != 0  # (a disc is thin: some neighbourhoods lie in its plane)
    assert np.all(d.sigma > 0.0) and np.all(d.status[~flat] == 0) and np.count_nonzero(~flat) > 0
    assert np.all(np.isfinite(d.shear[~flat])) and np.all(np.isnan(d.shear[flat]))
    part = sim.local_kinematics(6, include_self=False)
    assert part.grads is None and part.kth is None and part.stats.flags == 0
    assert np.array_equal(part.moments, _kin(sim, 6, grad=False, include_self=False).moments)
    with pytest.raises(ValueError):
        part.velocity_gradient
    sim.destroy()


def _cli_line(nb, d, state):
    """What headless --kin prints, from the Python mirror's arrays in body order."""
    ms = m = 0.0
    q_max, q_at = float("nan"), 0xFFFFFFFF
    for i in range(len(d.sigma)):
        if np.isfinite(d.sigma[i]):
            ms += float(state[i, 9]) * float(d.sigma[i])
            m += float(state[i, 9])
        q = float(d.phase_space_density[i])
        if np.isfinite(q) and not q <= q_max:
            q_max, q_at = q, i
    return [d.stats.step_num, d.stats.counted, d.stats.degenerate, int(np.count_nonzero(d.status & nb.KIN_SINGULAR))], \
        [ms / m, q_max], q_at


def test_runner_and_cli(gpu):
    """nb_local_kinematics_runner equals nb_local_kinematics_sim on nb_runner_sim, and headless --kin (the C++ mirror
    over the runner's call) prints what the Python runner returns."""
    nb = gpu
    from wgpu_n_body_amd import _lib
    cli = os.path.join(ROOT, "wgpu_n_body_amd", "headless")
    base = [cli, "--sim", "tree", "--n", "4096", "--init", "disc", "--steps", "4"]
    p = subprocess.run(base + ["--kin", "2", "--kin-k", "8", "--kin-gradient", "1"], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("kin ")]
    assert len(lines) == 3 and all(len(ln) == 8 for ln in lines)
    assert len([ln for ln in p.stdout.splitlines() if ln.startswith("Step Duration: ")]) == 4

    runner = nb.OfflineHeadless(nb.TreeSim, nb.SimParams(particle_num=4096), nb.AddParams.TreeSimParams(0.75),
                                lambda sp: nb.inits.disc_init(sp, seed=0))
    o = runner.local_kinematics(8, gradient=True)  # the same seeded init, no step yet: the line is the Python call
    state0 = _state_of(nb, runner)
    for _ in range(2):
        runner.step()
    via_runner = _raw(None, 8, call=_lib.lib().nb_local_kinematics_runner, handle=runner._h, n=4096)
    via_sim = _raw(runner.sim, 8)
    state = _state_of(nb, runner.sim)
    runner.destroy()
    assert via_runner.rc == via_sim.rc == 0 and via_runner.bytes == via_sim.bytes
    _check(via_sim, R.kin_vectorised(*K.split(state), 8))

    ints, reals, q_at = _cli_line(nb, o, state0)
    ln = lines[0]
    assert [int(x) for x in ln[1:5]] == ints and int(ln[7]) == q_at
    assert [float(x) for x in ln[5:7]] == reals  # (%.17g round-trips)
    for j, ln in enumerate(lines):  # (the trajectory of two runs of the tree is not specified bit for bit)
        assert int(ln[1]) == 2 * j and int(ln[2]) == 4096


def test_exact_linear_flow(gpu):
    nb = gpu
    state, A = R.linear_flow_state()
    sim = _sim(nb, "naive", state)
    g = _kin(sim, 32)
    d = sim.local_kinematics(32, gradient=True)
    sim.destroy()
    _check(g, R.kin_vectorised(*K.split(state), 32))
    R.check_linear_flow(g.moments, g.grads, A, d.derived)


def test_a_cold_clump_stands_out_in_phase_space(gpu):
    """What the feature exists for: the clump is no denser than its surroundings -- the two median densities are
    within a factor of 3 -- but its median sigma is below a tenth of the background's and its median Q more than
    100 times above it."""
    nb = gpu
    state, clump = R.clump_state()
    sim = _sim(nb, "naive", state)
    d = sim.local_kinematics(32)
    sim.destroy()
    R.check_clump(d.sigma, d.phase_space_density, d.density, clump)
