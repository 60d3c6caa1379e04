"""nb_sim_knn on the device (csrc/nb_knn.hip) against the numpy restatements of its rule (tests/knn_ref.py) on the
read-back state: r2, kth, mass_in, density, the peak and every integer of the stats equal, every sum to 1e-10 of
its sum of |term|; states short of k, lattices (where the index decides), coincident bodies, zero extents, an
outlier, bodies on cell borders, the inits with non-finite bodies; a large case against a sample; the tuning keys;
bitwise reproducibility; permutations; the null outputs and refusals; that a call does not perturb the
trajectory; the runner, the C++ mirror and the CLI; center="density".  `-m gpu`."""
import ctypes as C
import math
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from tests import knn_ref as K
from tests.helpers import ROOT, make_state

pytestmark = pytest.mark.gpu

TOL = K.TOL  # of the sum of |term|: TOL of tests/test_map_gpu.py and tests/test_fof_gpu.py
FILL = 0xDEADBEEF


def _sim(nb, kind, state, theta=0.75):
    sp = nb.SimParams(particle_num=state.shape[0])
    if kind == "naive":
        return nb.NaiveSim.from_particles(sp, None, state)
    return nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(theta), state)


def _raw(sim, k, call=None, handle=None, n=None, flags=0):
    """The C call with every buffer pre-filled."""
    from wgpu_n_body_amd import _lib
    n = int(sim.sim_params().particle_num) if n is None else n
    p = _lib.nb_knn_params()
    p.k, p.flags = k, flags
    r2, mass_in, density = np.full(n + 1, -7.0), np.full(n + 1, -7.0), np.full(n + 1, -7.0)
    kth = np.full(n + 1, FILL, np.uint32)
    st = _lib.nb_knn_stats()
    rc = (call or _lib.lib().nb_sim_knn)(handle or sim._h, C.byref(p), r2.ctypes.data, kth.ctypes.data,
                                         mass_in.ctypes.data, density.ctypes.data, C.byref(st))
    return SimpleNamespace(rc=rc, n=n, r2=r2[:n], kth=kth[:n], mass_in=mass_in[:n], density=density[:n], st=st,
                           tail=(r2[n], kth[n], mass_in[n], density[n]),
                           bytes=r2.tobytes() + kth.tobytes() + mass_in.tobytes() + density.tobytes() + bytes(st))


def _knn(sim, k, **kw):
    from wgpu_n_body_amd import _lib
    g = _raw(sim, k, **kw)
    assert g.rc == 0, _lib.lib().nb_last_error()
    assert g.tail == (-7.0, FILL, -7.0, -7.0)  # n values each, no more
    return g


def _untouched(g):
    return (np.all(g.r2 == -7.0) and np.all(g.kth == FILL) and np.all(g.mass_in == -7.0) and np.all(g.density == -7.0)
            and g.tail == (-7.0, FILL, -7.0, -7.0))


def _check_bodies(g, ref, sel=slice(None)):
    assert np.array_equal(g.r2[sel], ref.r2[sel], equal_nan=True), np.flatnonzero(~(g.r2[sel] == ref.r2[sel]))[:8]
    assert np.array_equal(g.kth[sel], ref.kth[sel]), np.flatnonzero(g.kth[sel] != ref.kth[sel])[:8]
    assert np.array_equal(g.mass_in[sel], ref.mass_in[sel]), np.flatnonzero(g.mass_in[sel] != ref.mass_in[sel])[:8]
    assert np.array_equal(g.density[sel], ref.density[sel]), np.flatnonzero(g.density[sel] != ref.density[sel])[:8]


def _sums_of(st):
    return np.array([st.sum_rho, *st.sum_rho_x, *st.sum_rho_v, st.sum_rho2])


def _check(g, ref, tol=TOL):
    """Every per-body value and integer equal, the peak equal, every sum within tol of its sum of |term|."""
    st = g.st
    for f in ("n", "nonfinite", "counted", "degenerate", "short_of_k", "peak_index", "peak_density"):
        assert getattr(st, f) == getattr(ref, f), (f, getattr(st, f), getattr(ref, f))
    _check_bodies(g, ref)
    err = np.abs(_sums_of(st) - ref.sums)
    print("sums: error / (TOL * sum of |term|) =", (err / (tol * ref.sums_abs + 1e-300)).max())
    assert np.all(err <= tol * ref.sums_abs), (err, ref.sums_abs)
    assert st.nonfinite + st.counted == st.n


def _state_of(nb, sim):
    return nb.as_floats(sim.read_particles()).copy()


def _prepared(nb, kind, state, step=True):
    """The simulator and the state it holds: a TreeSim after one step, in tree order."""
    sim = _sim(nb, kind, state)
    if kind == "tree" and step and state.shape[0] > 0:
        sim.encode()
    return sim, _state_of(nb, sim)


@pytest.mark.parametrize("n", [0, 1, 2, 7, 63, 64, 65, 66, 1000])
@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_sizes(gpu, kind, n):
    """Every k against every n: the states short of k (c <= k) among them."""
    nb = gpu
    state0 = K.state_of(K.ball(np.random.default_rng(n), n, 1.0), n)
    sim, state = _prepared(nb, kind, state0)
    for k in (1, 6, 32, 64):
        g = _knn(sim, k)
        ref = K.knn_vectorised(*K.split(state), k)
        _check(g, ref)
        assert g.st.short_of_k == (n if n <= k else 0)
        if 0 < n <= k:
            assert np.all(np.isinf(g.r2)) and np.all(g.kth == K.NONE) and g.st.peak_index == K.NONE
    sim.destroy()


@pytest.mark.parametrize("init", ["uniform", "disc", "spherical"])
@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_project_inits(gpu, kind, init):
    nb = gpu
    sim, state = _prepared(nb, kind, make_state(init, 4096, seed=7))
    for k in (6, 32):
        _check(_knn(sim, k), K.knn_vectorised(*K.split(state), k))
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
        g = _knn(sim, k)
        _check(g, K.knn_vectorised(*K.split(state), k))
        assert g.st.nonfinite == 40 and np.all(np.isnan(g.r2[~ok])) and np.all(g.kth[~ok] == K.NONE)
        assert not g.mass_in[~ok].any() and not g.density[~ok].any() and np.all(ok[g.kth[ok]])
    sim.destroy()


def test_no_body_counts(gpu):
    nb = gpu
    state = K.state_of(np.full((300, 3), np.nan))
    sim = _sim(nb, "naive", state)
    g = _knn(sim, 6)
    _check(g, K.knn_vectorised(*K.split(state), 6))
    assert (g.st.counted, g.st.nonfinite, g.st.short_of_k, g.st.peak_index) == (0, 300, 0, K.NONE)
    assert np.all(np.isnan(g.r2)) and not _sums_of(g.st).any()
    sim.destroy()


CASES = K.synthetic_cases(small=False)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c[0] for c in CASES])
@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_synthetic_cases(gpu, kind, idx):
    nb = gpu
    name, state0, ks, steppable = CASES[idx]
    sim, state = _prepared(nb, kind, state0, step=steppable)
    for k in ks:
        g = _knn(sim, k)
        _check(g, K.knn_vectorised(*K.split(state), k))
        print(f"{name} k {k}: degenerate {g.st.degenerate} peak {g.st.peak_density:.6g} at {g.st.peak_index}")
    if name == "three_points":
        assert g.st.degenerate == 100 and k == 64  # (k above the multiplicities 60 and 40)
    sim.destroy()


@pytest.mark.parametrize("kind,k", [("naive", 6), ("naive", 32), ("tree", 32)])
def test_large_case_against_a_sample(gpu, kind, k):
    """70,001 bodies: chunks of more than one wave-load per sort block, hundreds of blocks of every kernel.  The
    restatement for 512 seeded bodies, the 32 of smallest and of largest device r2 and the peak's, each against
    all bodies; the sums in full from the device's own density by a binary64 host sum."""
    nb = gpu
    n = 70001
    sim, state = _prepared(nb, kind, make_state("spherical", n, seed=11))
    g = _knn(sim, k)
    sim.destroy()
    order = np.argsort(g.r2, kind="stable")
    sample = np.unique(np.concatenate([np.random.default_rng(k).choice(n, 512, replace=False), order[:32], order[-32:],
                                       [g.st.peak_index]]))
    assert 512 <= sample.size <= 577 and g.st.peak_index in sample
    ref = K.knn_vectorised(*K.split(state), k, queries=sample, rows=48)
    _check_bodies(g, ref, sample)
    assert (g.st.n, g.st.counted, g.st.nonfinite, g.st.short_of_k) == (n, n, 0, 0)
    assert g.st.degenerate == np.count_nonzero(g.r2 == 0.0)
    full = K.KnnRef(k, g.r2, g.kth, g.mass_in, g.density, n, 0, n)
    K.finish(full, state[:, 0:3], state[:, 3:6], np.ones(n, bool), True)
    err = np.abs(_sums_of(g.st) - full.sums)
    assert np.all(err <= TOL * full.sums_abs), (err, full.sums_abs)
    assert (g.st.peak_density, g.st.peak_index) == (full.peak_density, full.peak_index)
    assert np.all(g.kth < n) and np.all(g.kth != np.arange(n)) and np.all(np.isfinite(g.density[g.r2 > 0]))


def test_sort_chunks_beyond_the_other_suites(gpu):
    """524,289 bodies, k = 6: 1,639 sort chunks of 320 bodies, the last of one body, so a thread of the shared sort's
    scan (csrc/nb_analysis_sort.hpp) owns two chunks, in all eight passes.  As the large case above: the restatement
    for 128 seeded bodies, the 32 of smallest and of largest device r2 and the peak's, each against all bodies; the
    sums in full from the device's own density by a binary64 host sum."""
    nb = gpu
    n, k = 524289, 6
    sim, state = _prepared(nb, "naive", make_state("spherical", n, seed=11))
    g = _knn(sim, k)
    sim.destroy()
    order = np.argsort(g.r2, kind="stable")
    sample = np.unique(np.concatenate([np.random.default_rng(k).choice(n, 128, replace=False), order[:32], order[-32:],
                                       [g.st.peak_index]]))
    assert 128 <= sample.size <= 193 and g.st.peak_index in sample
    ref = K.knn_vectorised(*K.split(state), k, queries=sample, rows=48)
    _check_bodies(g, ref, sample)
    assert (g.st.n, g.st.counted, g.st.nonfinite, g.st.short_of_k) == (n, n, 0, 0)
    assert g.st.degenerate == np.count_nonzero(g.r2 == 0.0)
    full = K.KnnRef(k, g.r2, g.kth, g.mass_in, g.density, n, 0, n)
    K.finish(full, state[:, 0:3], state[:, 3:6], np.ones(n, bool), True)
    err = np.abs(_sums_of(g.st) - full.sums)
    assert np.all(err <= TOL * full.sums_abs), (err, full.sums_abs)
    assert (g.st.peak_density, g.st.peak_index) == (full.peak_density, full.peak_index)
    assert np.all(g.kth < n) and np.all(g.kth != np.arange(n)) and np.all(np.isfinite(g.density[g.r2 > 0]))


def test_tuning_keys_do_not_change_a_bit(gpu):
    """A crowded cell beside scattered bodies: every span and every cut of the work gives the default's bytes."""
    nb = gpu
    rng = np.random.default_rng(8)
    pos = np.concatenate([rng.uniform(0.0, 1e-6, (1500, 3)) + 0.25, K.ball(rng, 2500, 0.2, (0.25, 0.25, 0.25)),
                          [(40.0, 0.0, 0.0)]])
    state = K.state_of(pos[rng.permutation(4001)], 9)
    sim = _sim(nb, "naive", state)
    for k in (6, 32):
        base = _knn(sim, k)
        _check(base, K.knn_vectorised(*K.split(state), k))
        for span in range(1, 9):
            sim.set_tuning("knn_span_cells", span)
            assert _knn(sim, k).bytes == base.bytes, span
        sim.set_tuning("knn_span_cells", 3)
        for per in (1, 2, 4):
            sim.set_tuning("knn_block_queries", per)
            assert _knn(sim, k).bytes == base.bytes, per
    for key, value in (("knn_span_cells", 0), ("knn_span_cells", 9), ("knn_block_queries", 3), ("knn_block_queries", 8)):
        with pytest.raises(nb.NBodyError):
            sim.set_tuning(key, value)
    sim.destroy()


@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_bitwise_reproducible(gpu, kind):
    nb = gpu
    sim, state = _prepared(nb, kind, make_state("disc", 4097, seed=2))
    g1, g2 = _knn(sim, 6), _knn(sim, 6)
    _knn(sim, 32)  # another k between
    g3 = _knn(sim, 6)
    sim.destroy()
    assert g1.st.peak_index != K.NONE and g1.bytes == g2.bytes == g3.bytes


def _other_passes(sim):
    sim.diagnostics()
    sim.radial_profile(rmin=1e-3, rmax=10.0, nbins=16)
    sim.projected_map(32, 32, extent=(-1.0, 1.0, -1.0, 1.0))
    sim.fof_groups(0.02, min_members=2)
    sim.field(np.zeros((4, 3), np.float32))


def test_workspaces_of_other_passes(gpu):
    """The result does not depend on which pass made its workspace first."""
    nb = gpu
    state = make_state("spherical", 3000, seed=4)
    sim = _sim(nb, "naive", state)
    first = _knn(sim, 6)
    _other_passes(sim)
    again = _knn(sim, 6)
    sim.destroy()
    sim = _sim(nb, "naive", state)
    _other_passes(sim)
    late = _knn(sim, 6)
    sim.destroy()
    assert first.bytes == again.bytes == late.bytes


def test_a_permutation_permutes_the_result(gpu):
    nb = gpu
    n, k = 1500, 6
    state = K.state_of(np.random.default_rng(6).normal(size=(n, 3)), 6)
    ref = K.knn_vectorised(*K.split(state), k)
    assert K.tie_free(ref, *K.split(state))  # otherwise the index would decide, and a permutation change the answer
    perm = np.random.default_rng(4).permutation(n)  # body i of the permuted state is body perm[i]
    res = []
    for s in (state, state[perm]):
        sim = _sim(nb, "naive", s)
        res.append(_knn(sim, k))
        sim.destroy()
    a, b = res
    assert np.array_equal(b.r2, a.r2[perm]) and np.array_equal(b.mass_in, a.mass_in[perm])
    assert np.array_equal(b.density, a.density[perm]) and np.array_equal(perm[b.kth], a.kth[perm])
    assert perm[b.st.peak_index] == a.st.peak_index and b.st.peak_density == a.st.peak_density


def test_null_outputs_and_refusals(gpu):
    nb = gpu
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    state = make_state("spherical", 2000, seed=3)
    sim = _sim(nb, "naive", state)
    full = _knn(sim, 6)
    p = _lib.nb_knn_params()
    p.k = 6
    assert L.nb_sim_knn(sim._h, C.byref(p), None, None, None, None, None) == 0
    st = _lib.nb_knn_stats()
    assert L.nb_sim_knn(sim._h, C.byref(p), None, None, None, None, C.byref(st)) == 0 and bytes(st) == bytes(full.st)
    for which in range(4):
        bufs = [np.full(2001, -7.0), np.full(2001, FILL, np.uint32), np.full(2001, -7.0), np.full(2001, -7.0)]
        args = [b.ctypes.data if j == which else None for j, b in enumerate(bufs)]
        assert L.nb_sim_knn(sim._h, C.byref(p), *args, None) == 0
        want = (full.r2, full.kth, full.mass_in, full.density)[which]
        assert np.array_equal(bufs[which][:2000], want) and bufs[which][2000] in (-7.0, FILL)
    # refused calls write nothing
    for k, flags in ((0, 0), (65, 0), (6, 2)):
        g = _raw(sim, k, flags=flags)
        assert g.rc == _lib.NB_ERR_INVALID and L.nb_last_error() and _untouched(g)
        assert bytes(g.st) == bytes(_lib.nb_knn_stats())
    with pytest.raises(nb.NBodyError) as ex:
        sim.knn_density(0)
    assert ex.value.code == _lib.NB_ERR_INVALID
    assert _knn(sim, 6).bytes == full.bytes  # the simulator stays usable
    sim.destroy()
    # a sharded simulator (rank 0 of 2)
    s = make_state("uniform", 64, seed=1)
    sharded = nb.NaiveSim.from_particles(nb.SimParams(particle_num=64), None, s, placement=nb.Placement(world=2))
    g = _raw(sharded, 6, n=64)
    assert g.rc == _lib.NB_ERR_UNSUPPORTED and b"sharded" in L.nb_last_error() and _untouched(g)
    sharded.destroy()
    # a several-GPU runner, both ranks on device 0
    r = nb.OfflineHeadless(nb.NaiveSim, nb.SimParams(particle_num=512), None,
                           lambda sp: nb.inits.uniform_init(sp, seed=1), device_ids=[0, 0])
    with pytest.raises(nb.NBodyError) as ex:
        r.knn_density(6)
    assert ex.value.code == _lib.NB_ERR_UNSUPPORTED
    r.destroy()


@pytest.mark.parametrize("case", ["naive", "tree", "tree_graph"])
def test_does_not_perturb_the_trajectory(gpu, case):
    nb = gpu
    n, steps = 4096, 10
    state = make_state("uniform", n, seed=9)
    finals = []
    for with_knn in (False, True):
        sim = _sim(nb, "naive" if case == "naive" else "tree", state)
        if case == "tree_graph":
            sim.set_tuning("tree_use_graph", 1)
        for j in range(steps):
            sim.encode()
            if with_knn:
                d = sim.knn_density(6 if j % 2 else 32, density=j % 3 != 0, neighbours=j % 3 != 1)
                assert d.stats.step_num == j + 1 and d.stats.counted == n and d.stats.peak_index != K.NONE
        finals.append(nb.as_floats(sim.read_particles()).copy())
        sim.destroy()
    assert np.array_equal(finals[0].view(np.uint32), finals[1].view(np.uint32))


def test_python_wrapper_and_diagnostics(gpu):
    nb = gpu
    state = make_state("disc", 4096, seed=0)
    sim = _sim(nb, "naive", state)
    before = sim.diagnostics()
    d = sim.knn_density()
    after = sim.diagnostics()
    for f in before.__dataclass_fields__:  # the diagnostics are unchanged by a call
        assert np.array_equal(np.asarray(getattr(before, f)), np.asarray(getattr(after, f)), equal_nan=True), f
    g = _knn(sim, 6)
    assert d.k == 6 and np.array_equal(d.r2, g.r2) and np.array_equal(d.kth, g.kth)
    assert np.array_equal(d.mass_in, g.mass_in) and np.array_equal(d.density, g.density)
    assert np.array_equal(d.r_k, np.sqrt(g.r2)) and (d.peak_index, d.peak_density) == (g.st.peak_index, g.st.peak_density)
    assert np.array_equal(d.center, np.array(g.st.sum_rho_x[:]) / g.st.sum_rho)
    assert np.array_equal(d.center_velocity, np.array(g.st.sum_rho_v[:]) / g.st.sum_rho)
    assert d.density[d.peak_index] == d.peak_density == d.density[np.isfinite(d.density)].max()
    part = sim.knn_density(32, neighbours=False)
    assert part.r2 is None and part.kth is None and part.r_k is None and part.density is not None
    part = sim.knn_density(32, density=False)
    assert part.density is None and part.mass_in is None and np.array_equal(part.r2, _knn(sim, 32).r2)
    sim.destroy()


def test_runner_and_cli(gpu):
    """nb_runner_knn equals nb_sim_knn on nb_runner_sim, and headless --knn (the C++ mirror over nb_runner_knn)
    prints what the Python runner returns."""
    nb = gpu
    from wgpu_n_body_amd import _lib
    cli = os.path.join(ROOT, "wgpu_n_body_amd", "headless")
    base = [cli, "--sim", "tree", "--n", "4096", "--init", "disc", "--steps", "4"]
    p = subprocess.run(base + ["--knn", "2", "--knn-k", "8"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("knn ")]
    assert len(lines) == 3 and all(len(ln) == 12 for ln in lines)
    assert len([ln for ln in p.stdout.splitlines() if ln.startswith("Step Duration: ")]) == 4

    runner = nb.OfflineHeadless(nb.TreeSim, nb.SimParams(particle_num=4096), nb.AddParams.TreeSimParams(0.75),
                                lambda sp: nb.inits.disc_init(sp, seed=0))
    o = runner.knn_density(8)  # the same seeded init, no step yet: the line is the Python call
    for _ in range(2):
        runner.step()
    via_runner = _raw(None, 8, call=_lib.lib().nb_runner_knn, handle=runner._h, n=4096)
    via_sim = _raw(runner.sim, 8)
    state = _state_of(nb, runner.sim)
    runner.destroy()
    assert via_runner.rc == via_sim.rc == 0 and via_runner.bytes == via_sim.bytes
    _check(via_sim, K.knn_vectorised(*K.split(state), 8))

    ln = lines[0]
    assert [int(x) for x in ln[1:4]] == [0, o.stats.counted, o.stats.degenerate] and int(ln[11]) == o.peak_index
    got = np.array([float(x) for x in ln[4:11]])
    assert np.array_equal(got, np.concatenate([o.center, o.center_velocity, [o.peak_density]]))  # (%.17g round-trips)
    for j, ln in enumerate(lines):  # (the trajectory of two runs of the tree is not specified bit for bit)
        assert int(ln[1]) == 2 * j and int(ln[2]) == 4096


def _same_result(a, b):
    for f in a.__dataclass_fields__:
        x, y = getattr(a, f), getattr(b, f)
        if isinstance(x, np.ndarray):
            assert x.tobytes() == y.tobytes(), f
        elif isinstance(x, float):
            assert x == y or (math.isnan(x) and math.isnan(y)), f
        else:
            assert x == y, f


def test_center_density_is_the_explicit_call(gpu):
    nb = gpu
    sim = _sim(nb, "naive", make_state("spherical", 4096, seed=1))
    d = sim.knn_density(6, neighbours=False)
    kw = dict(rmin=1e-3, rmax=10.0, nbins=24)
    a = sim.radial_profile(center="density", **kw)
    b = sim.radial_profile(center=d.center, velocity=d.center_velocity, **kw)
    _same_result(a, b)
    assert np.array_equal(a.center, d.center)
    kw = dict(extent=(-0.5, 0.5, -0.5, 0.5), axis=(0.0, 0.0, 1.0))
    a = sim.projected_map(48, 40, center="density", **kw)
    b = sim.projected_map(48, 40, center=d.center, velocity=d.center_velocity, **kw)
    _same_result(a, b)
    with pytest.raises(ValueError):
        sim.projected_map(8, 8, center="density", velocity=(0.0, 0.0, 0.0), extent=(-1, 1, -1, 1))
    with pytest.raises(ValueError):
        sim.radial_profile(center="densest", rmin=1e-3, rmax=1.0)
    sim.destroy()


def test_center_density_on_a_runner_is_its_simulators(gpu):
    """radial_profile and projected_map are one method for Simulator and OfflineHeadless: center="density" on a
    one-device runner returns what the runner's simulator returns, field for field and bit for bit."""
    nb = gpu
    runner = nb.OfflineHeadless(nb.TreeSim, nb.SimParams(particle_num=2048), nb.AddParams.TreeSimParams(0.75),
                                lambda sp: nb.inits.spherical_init(sp, seed=1), device_id=0)
    for _ in range(2):
        runner.step()
    kw = dict(rmin=1e-3, rmax=10.0, nbins=24)
    _same_result(runner.radial_profile(center="density", **kw), runner.sim.radial_profile(center="density", **kw))
    kw = dict(extent=(-0.5, 0.5, -0.5, 0.5), axis=(0.0, 0.0, 1.0))
    a = runner.projected_map(48, 40, center="density", **kw)
    _same_result(a, runner.sim.projected_map(48, 40, center="density", **kw))
    d = runner.knn_density(6, neighbours=False)
    assert np.array_equal(a.center, d.center)
    with pytest.raises(ValueError):
        runner.projected_map(8, 8, center="density", velocity=(0.0, 0.0, 0.0), extent=(-1, 1, -1, 1))
    runner.destroy()


def test_the_density_centre_ignores_escapers(gpu):
    """What the feature exists for.  A 4,096-body `spherical` state, then the same with 40 bodies moved 57 length
    units out: the density centre of the disturbed state stays within 0.25 r_core of the undisturbed one, where
    r_core is the median r_k (k = 6) of the 410 densest bodies of the undisturbed state; the centre of mass does
    not stay within r_core.  From a CPU run of the restatement (tests/knn_ref.py, seeds 1, 2, 3): r_core = 0.087,
    the density centre moves by 0.044-0.063 r_core (the 40 bodies' own share of the sum), the centre of mass by
    6.0-6.4 r_core: the factor 0.25 leaves four times the largest of them."""
    nb = gpu
    state = make_state("spherical", 4096, seed=1)
    moved = state.copy()
    rows = np.random.default_rng(5).choice(4096, 40, replace=False)
    moved[rows, 0:3] += np.float32(50.0) * np.array([1.0, 0.5, -0.25], np.float32)
    res = []
    for s in (state, moved):
        sim = _sim(nb, "naive", s)
        res.append((sim.knn_density(6), sim.diagnostics()))
        sim.destroy()
    (d0, _), (d1, diag1) = res
    r_core = float(np.median(d0.r_k[np.argsort(-d0.density)[:410]]))
    shift = float(np.linalg.norm(d1.center - d0.center))
    com_shift = float(np.linalg.norm(np.asarray(diag1.com) - d0.center))
    print(f"r_core {r_core:.4g} density centre moved {shift / r_core:.3g} r_core, centre of mass {com_shift / r_core:.3g}")
    assert shift <= 0.25 * r_core
    assert com_shift > r_core
