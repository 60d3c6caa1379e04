"""nb_sim_radial_profile on the device (csrc/nb_radial.hip) against the numpy restatement of its rule
(tests/radial_ref.py) on the read-back state: every count equal, every sum to 1e-10 of its sum of
|term|; edges hit exactly; the identities; bitwise reproducibility; that a call does not perturb the
trajectory; the refusals; the runner, the C++ mirror and the CLI.  `-m gpu`."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import radial_ref as R
from tests.helpers import ROOT, make_state

pytestmark = pytest.mark.gpu

TOL = 1e-10  # of the sum of |term|: what the diagnostics' moments are held to
TILTED = (1.0, 2.0, 3.0)
AXES = {"sph": None, "cyl_y": (0.0, 1.0, 0.0), "cyl_tilt": TILTED}


def _sim(nb, kind, state, theta=0.75):
    sp = nb.SimParams(particle_num=state.shape[0])
    if kind == "naive":
        return nb.NaiveSim.from_particles(sp, None, state)
    return nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(theta), state)


def _profile(sim, edges, axis, center, velocity=(0.0, 0.0, 0.0)):
    return sim.radial_profile(edges, cylindrical=axis is not None, axis=axis or (0.0, 1.0, 0.0), center=center,
                              velocity=velocity)


def _raw(sim, edges, flags=0, axis=(0.0, 1.0, 0.0), center=(0.0, 0.0, 0.0)):
    from wgpu_n_body_amd import _lib
    e = np.ascontiguousarray(edges, dtype=np.float64)
    p = _lib.nb_radial_params()
    p.nbins, p.flags = e.shape[0] - 1, flags
    for k in range(3):
        p.axis[k], p.center[k] = axis[k], center[k]
    p.edges = e.ctypes.data_as(C.POINTER(C.c_double))
    out = _lib.nb_radial_profile()
    bins = (_lib.nb_radial_bin * (e.shape[0] - 1))()
    rc = _lib.lib().nb_sim_radial_profile(sim._h, C.byref(p), C.byref(out), bins)
    return rc, out, bins


def _check(p, ref, tol=TOL):
    """Every integer equal, every sum within tol of the restatement's sum of |term|; the identities."""
    sc = ref["scale"]
    assert (p.n, p.nonfinite, p.nbins) == (ref["n"], ref["nonfinite"], ref["nbins"])
    assert (p.inside_count, p.outside_count) == (ref["inside_count"], ref["outside_count"])
    assert np.array_equal(p.count, ref["count"]), (p.count, ref["count"])
    assert p.inside_count + int(p.count.sum()) + p.outside_count + p.nonfinite == p.n
    assert abs(p.inside_mass - ref["inside_mass"]) <= tol * sc["inside_mass"]
    assert abs(p.outside_mass - ref["outside_mass"]) <= tol * sc["outside_mass"]
    assert abs(p.mass - ref["total_mass"]) <= tol * sc["total_mass"]
    assert np.all(np.abs(p.shape - ref["shape"]) <= tol * sc["shape"] + 1e-300), (p.shape, ref["shape"])
    for name in R.BIN_SUMS:
        got = p.bin_mass if name == "mass" else getattr(p, name)
        assert np.all(np.abs(got - ref[name]) <= tol * sc[name] + 1e-300), (name, got, ref[name])
    assert abs(p.inside_mass + p.bin_mass.sum() + p.outside_mass - p.mass) <= 1e-12 * abs(p.mass)
    assert np.array_equal(p.axis, ref["axis"])
    if not p.cylindrical:
        assert np.all(p.m_uphi == 0) and np.all(p.m_uphi2 == 0)


# the cross product of every axis of the issue, thinned to 60 cases that keep every value of every axis
_ALL = list(itertools.product(["naive", "tree"], ["uniform", "disc", "spherical"], [1, 2, 63, 65, 257, 1000, 4097],
                              [1, 7, 64, 256], ["sph", "cyl_y", "cyl_tilt"], ["explicit", "com"]))
CASES = [_ALL[(i * 17 + 5) % len(_ALL)] for i in range(60)]
assert len(set(CASES)) == 60 and [len({c[a] for c in CASES}) for a in range(6)] == [2, 3, 7, 4, 3, 2]


@pytest.mark.parametrize("idx", range(len(CASES)), ids=["-".join(str(v) for v in c) for c in CASES])
def test_parity_with_the_restatement(gpu, idx):
    nb = gpu
    kind, init, n, nbins, mode, centre = CASES[idx]
    sim = _sim(nb, kind, make_state(init, n, seed=idx + 11))
    if kind == "tree":  # the state is then in tree order
        for _ in range(3):
            sim.encode()
    # log bins that leave bodies inside and outside, or linear bins from 0 (r = 0 is then in bin 0)
    edges = nb.radial_edges(0.05, 1.2, nbins, log=True) if idx % 2 == 0 else nb.radial_edges(0.0, 1.0, nbins, log=False)
    if centre == "com":
        p = _profile(sim, edges, AXES[mode], "com")
        d = sim.diagnostics()
        assert p.center.tobytes() == d.com.tobytes()
        assert p.velocity.tobytes() == (d.momentum / d.mass).tobytes()
        c, vc = p.center, p.velocity
    else:
        c, vc = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)) if idx % 4 < 2 else ((0.05, -0.02, 0.01), (1e-3, -2e-3, 5e-4))
        p = _profile(sim, edges, AXES[mode], c, vc)
        assert np.array_equal(p.center, c) and np.array_equal(p.velocity, vc)
    state = nb.as_floats(sim.read_particles())
    sim.destroy()
    assert p.step_num == (3 if kind == "tree" else 0) and np.array_equal(p.edges, edges)
    _check(p, R.profile64(state, edges, center=c, velocity=vc, axis=AXES[mode]))


def _dyadic_bodies():
    """64 bodies with coordinates k / 1024: the named ones first, the rest seeded."""
    rng = np.random.default_rng(8)
    q = rng.integers(-1536, 1537, size=(64, 3))
    q[0] = (0, 0, 0)            # r = 0
    q[1] = (256, 0, 0)          # r = 1/4
    q[2] = (0, 0, -512)         # r = 1/2
    q[3] = (384, 0, 512)        # r = 5/8 (3-4-5)
    q[4] = (0, 1024, 0)         # r = 1 (on the y axis: cylindrical radius 0)
    q[5] = (-768, 0, 1024)      # r = 5/4
    q[6] = (0, 0, 2048)         # r = 2
    q[7] = (1024, 777, 0)       # cylindrical radius 1 about y
    s = np.zeros((64, 10), np.float32)
    s[:, 0:3] = q / 1024.0
    s[:, 3:6] = rng.integers(-64, 65, size=(64, 3)) / 64.0
    s[:, 9] = rng.integers(1, 9, size=64)
    return q, s


@pytest.mark.parametrize("kind", ["naive", "tree"])
@pytest.mark.parametrize("cyl", [False, True])
@pytest.mark.parametrize("first", [0, 256])
def test_bodies_exactly_on_edges(gpu, kind, cyl, first):
    """Coordinates and edges are dyadic, so r^2 and the squared edges are exact and the expected bins follow
    from integer arithmetic alone: lower edge inclusive, upper exclusive."""
    nb = gpu
    q, s = _dyadic_bodies()
    e_int = np.array([first, 512, 1024, 1280, 2048])        # edges * 1024: 0 or 1/4, then 1/2, 1, 5/4, 2
    edges = e_int / 1024.0
    axis = (0.0, 1.0, 0.0) if cyl else None
    r2 = (q[:, 0] ** 2 + q[:, 2] ** 2) if cyl else (q ** 2).sum(1)
    want = np.searchsorted(e_int ** 2, r2, side="right")    # in integers: 0 inside, k + 1 bin k, 5 outside
    # by hand: r = 0 is in bin 0 only when edges[0] == 0; a body on edges[0] is in bin 0, one on an interior edge
    # in the bin above it, one on edges[nbins] outside
    at_zero = 1 if first == 0 else 0
    by_hand = [at_zero, 1, 2, 2, at_zero, 4, 5, 3] if cyl else [at_zero, 1, 2, 2, 3, 4, 5, 4]
    assert list(want[:8]) == by_hand
    sim = _sim(nb, kind, s)
    p = _profile(sim, edges, axis, (0.0, 0.0, 0.0))
    sim.destroy()
    assert p.inside_count == int((want == 0).sum()) and p.outside_count == int((want == 5).sum())
    assert np.array_equal(p.count, np.bincount(want, minlength=6)[1:5])
    _check(p, R.profile64(s, edges, axis=axis))
    if first == 0:
        # the bodies at r = 0 add their mass to bin 0 and nothing radial or tangential: the bin's other
        # bodies alone give its velocity sums
        zero = np.flatnonzero(r2 == 0)
        others = np.flatnonzero((want == 1) & (r2 != 0))
        assert len(zero) == (2 if cyl else 1) and p.count[0] == len(zero) + len(others)
        ref = R.profile64(s[others], edges, axis=axis)
        for name in ("m_r", "m_ur", "m_ur2", "m_uphi", "m_uphi2"):
            assert abs(getattr(p, name)[0] - ref[name][0]) <= TOL * ref["scale"][name][0] + 1e-300, name
        assert p.bin_mass[0] == ref["mass"][0] + s[zero, 9].astype(np.float64).sum()  # (small integers)


@pytest.mark.parametrize("kind", ["naive", "tree"])
@pytest.mark.parametrize("mode", ["sph", "cyl_tilt"])
def test_all_bodies_in_range_angular_momentum(gpu, kind, mode):
    """`ang` is only binned, so its total is checked where every body is in a bin: against the restatement,
    and -- about the origin at rest -- against the diagnostics' angular momentum."""
    nb = gpu
    n = 3000
    sim = _sim(nb, kind, make_state("disc", n, seed=21))
    sim.encode()
    edges = nb.radial_edges(0.0, 8.0, 32, log=False)
    p = _profile(sim, edges, AXES[mode], (0.0, 0.0, 0.0))
    d = sim.diagnostics()
    state = nb.as_floats(sim.read_particles())
    sim.destroy()
    ref = R.profile64(state, edges, axis=AXES[mode])
    assert p.inside_count == 0 and p.outside_count == 0 and int(p.count.sum()) == n
    _check(p, ref)
    scale = ref["scale"]["ang"].sum(0)
    assert np.all(np.abs(p.ang.sum(0) - ref["ang"].sum(0)) <= TOL * scale)
    assert np.all(np.abs(p.ang.sum(0) - d.angular_momentum) <= TOL * scale)
    assert abs(p.mass - d.mass) <= 1e-12 * d.mass and abs(p.m_u2.sum() - 2.0 * d.kinetic) <= TOL * 2.0 * d.kinetic
    # derived quantities hold together
    assert abs(p.cumulative_mass[-1] - p.mass) <= 1e-12 * p.mass
    half = p.lagrangian([0.5])[0]
    k = int(np.searchsorted(p.cumulative_mass, 0.5 * p.mass))
    assert edges[k] <= half <= edges[k + 1]


def test_two_sims_same_state(gpu):
    nb = gpu
    n = 5000
    state = make_state("spherical", n, seed=5)
    edges = nb.radial_edges(0.05, 1.2, 48)
    a, b = _sim(nb, "naive", state), _sim(nb, "tree", state)
    pa, pb = _profile(a, edges, TILTED, "com"), _profile(b, edges, TILTED, "com")
    a.destroy()
    b.destroy()
    ref = R.profile64(state, edges, center=pa.center, velocity=pa.velocity, axis=TILTED)
    assert np.array_equal(pa.count, pb.count) and (pa.inside_count, pa.outside_count) == (pb.inside_count, pb.outside_count)
    _check(pa, ref)
    _check(pb, R.profile64(state, edges, center=pb.center, velocity=pb.velocity, axis=TILTED))
    for name in R.BIN_SUMS:
        x, y = (pa.bin_mass, pb.bin_mass) if name == "mass" else (getattr(pa, name), getattr(pb, name))
        assert np.all(np.abs(x - y) <= 2 * TOL * ref["scale"][name] + 1e-300), name


@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_bitwise_reproducible(gpu, kind):
    nb = gpu
    from wgpu_n_body_amd import _lib
    n = 4097
    sim = _sim(nb, kind, make_state("disc", n, seed=2))
    sim.encode()
    edges = nb.radial_edges(0.02, 1.5, 64)
    flags = _lib.NB_RADIAL_CYLINDRICAL | _lib.NB_RADIAL_CENTER_COM
    rc1, o1, b1 = _raw(sim, edges, flags, axis=(0.0, 0.0, 1.0))
    rc2, o2, b2 = _raw(sim, edges, flags, axis=(0.0, 0.0, 1.0))
    sim.diagnostics(potential=True)  # shares the moments' workspace
    rc3, o3, b3 = _raw(sim, edges, flags, axis=(0.0, 0.0, 1.0))
    sim.destroy()
    assert rc1 == rc2 == rc3 == 0 and o1.n == n and o1.nbins == 64
    assert bytes(o1) == bytes(o2) == bytes(o3) and bytes(b1) == bytes(b2) == bytes(b3)


@pytest.mark.parametrize("case", ["naive", "tree", "tree_graph", "tree_gather"])
def test_does_not_perturb_the_trajectory(gpu, case):
    nb = gpu
    n, steps = (1 << 20, 3) if case == "tree_gather" else (4096, 10)
    state = make_state("uniform", n, seed=9)
    edges = nb.radial_edges(0.05, 1.5, 64)
    finals = []
    for with_profile in (False, True):
        sim = _sim(nb, "naive" if case == "naive" else "tree", state)
        if case == "tree_graph":
            sim.set_tuning("tree_use_graph", 1)
        for k in range(steps):
            sim.encode()
            if with_profile:
                p = sim.radial_profile(edges, cylindrical=k % 2 == 1, axis=TILTED, center="com" if k % 3 else (0, 0, 0))
                assert p.step_num == k + 1 and p.inside_count + int(p.count.sum()) + p.outside_count == n
        finals.append(nb.as_floats(sim.read_particles()).copy())
        sim.destroy()
    assert np.array_equal(finals[0].view(np.uint32), finals[1].view(np.uint32))


def test_large_tree_in_the_gather_range(gpu):
    """2^20 bodies: from 524,288 the walk gathers and the state changes buffer set every step -- the profile
    must read the buffer read_particles converts, not a stale one.  Also the largest grid of the suite."""
    nb = gpu
    n = 1 << 20
    sim = _sim(nb, "tree", make_state("uniform", n, seed=11))
    edges = nb.radial_edges(0.0, 1.7, 128, log=False)
    for steps in (1, 2):
        sim.encode()
        p = _profile(sim, edges, None, (0.0, 0.0, 0.0))
        assert p.step_num == steps
        _check(p, R.profile64(nb.as_floats(sim.read_particles()), edges))
    sim.destroy()


@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_nonfinite_body_is_counted_and_left_out(gpu, kind):
    nb = gpu
    n = 1000
    state = make_state("uniform", n, seed=4)
    state[137, 4] = np.nan
    state[500, 0] = np.inf
    state[901, 9] = -np.inf
    sim = _sim(nb, kind, state)
    edges = nb.radial_edges(0.3, 1.4, 7)
    for axis in (None, TILTED):
        p = _profile(sim, edges, axis, (0.0, 0.0, 0.0))
        assert p.nonfinite == 3 and np.isfinite(p.mass) and np.isfinite(p.shape).all()
        for name in R.BIN_SUMS:
            assert np.isfinite(p.bin_mass if name == "mass" else getattr(p, name)).all(), name
        _check(p, R.profile64(state, edges, axis=axis))
    sim.destroy()


@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_every_body_in_one_bin(gpu, kind):
    """nbins = 1 with all 4,097 bodies in the bin: every thread of a tile then holds a body of the one bin."""
    nb = gpu
    n = 4097
    state = make_state("spherical", n, seed=6)
    sim = _sim(nb, kind, state)
    for axis in (None, (0.0, 1.0, 0.0)):
        p = _profile(sim, [0.0, 10.0], axis, (0.0, 0.0, 0.0))
        assert p.count[0] == n and p.inside_count == 0 and p.outside_count == 0
        _check(p, R.profile64(state, [0.0, 10.0], axis=axis))
    # ... and all of them in the last of 256 bins, or beyond it
    edges = np.concatenate([np.linspace(0.0, 1e-3, 256), [10.0]])
    p = _profile(sim, edges, None, (0.0, 0.0, 0.0))
    assert p.count[255] == n
    _check(p, R.profile64(state, edges))
    p = _profile(sim, edges[:-1], None, (0.0, 0.0, 0.0))
    assert p.outside_count == n and p.count.sum() == 0
    _check(p, R.profile64(state, edges[:-1]))
    sim.destroy()


def test_refusals(gpu):
    nb = gpu
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    s = make_state("uniform", 64, seed=1)
    edges = [0.0, 1.0, 2.0]
    sim = _sim(nb, "naive", s)
    rc, _, _ = _raw(sim, edges, flags=4)
    assert rc == _lib.NB_ERR_INVALID
    rc, _, _ = _raw(sim, [0.0, 2.0, 1.0])
    assert rc == _lib.NB_ERR_INVALID
    rc, out, _ = _raw(sim, edges)
    assert rc == 0 and out.n == 64
    sim.destroy()
    # a sharded simulator (rank 0 of 2)
    sharded = nb.NaiveSim.from_particles(nb.SimParams(particle_num=64), None, s, placement=nb.Placement(world=2))
    rc, _, _ = _raw(sharded, edges)
    assert rc == _lib.NB_ERR_UNSUPPORTED and b"sharded" in L.nb_last_error()
    sharded.destroy()
    # a several-GPU runner, both ranks on device 0
    r = nb.OfflineHeadless(nb.NaiveSim, nb.SimParams(particle_num=512), None,
                           lambda p: nb.inits.uniform_init(p, seed=1), device_ids=[0, 0])
    with pytest.raises(nb.NBodyError) as ex:
        r.radial_profile(edges)
    assert ex.value.code == _lib.NB_ERR_UNSUPPORTED
    r.destroy()


def test_runner_and_cli(gpu):
    """headless --radial (the C++ mirror over nb_runner_radial_profile) prints what the Python runner returns."""
    nb = gpu
    cli = os.path.join(ROOT, "wgpu_n_body_amd", "headless")
    p = subprocess.run([cli, "--sim", "tree", "--n", "2048", "--init", "disc", "--steps", "20", "--radial", "10",
                        "--radial-bins", "16", "--radial-range", "0.05,1.25", "--radial-axis", "0,0,1"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    heads = [ln for ln in p.stdout.splitlines() if ln.startswith("Radial: ")]
    rows = [ln for ln in p.stdout.splitlines() if ln.startswith("RadialBin: ")]
    assert len(heads) == 3 and len(rows) == 3 * 16
    assert len([ln for ln in p.stdout.splitlines() if ln.startswith("Step Duration: ")]) == 20
    num = r"(\S+)"
    head = re.compile(r"Radial: step (\d+) n (\d+) nonfinite (\d+) nbins (\d+) flags (\d+) inside_count (\d+) "
                      r"inside_mass {0} outside_count (\d+) outside_mass {0} mass {0} center {0} {0} {0} "
                      r"velocity {0} {0} {0} axis {0} {0} {0} shape {0} {0} {0} {0} {0} {0}$".format(num))
    row = re.compile(r"RadialBin: step (\d+) bin (\d+) lo {0} hi {0} count (\d+) mass {0} m_r {0} m_ur {0} m_ur2 {0} "
                     r"m_uphi {0} m_uphi2 {0} m_u2 {0} ang {0} {0} {0}$".format(num))
    runner = nb.OfflineHeadless(nb.TreeSim, nb.SimParams(particle_num=2048), nb.AddParams.TreeSimParams(0.75),
                                lambda sp: nb.inits.disc_init(sp, seed=0))
    kw = dict(nbins=16, rmin=0.05, rmax=1.25, cylindrical=True, axis=(0.0, 0.0, 1.0))
    ours = [runner.radial_profile(**kw)]
    for k in range(20):
        runner.step()
        if (k + 1) % 10 == 0:
            ours.append(runner.radial_profile(**kw))
    sim_view = runner.sim.radial_profile(**kw)  # the runner's simulator gives the same
    runner.destroy()
    assert sim_view.count.tobytes() == ours[-1].count.tobytes() and sim_view.m_uphi.tobytes() == ours[-1].m_uphi.tobytes()

    def close(got, want):
        for a, b in zip(got, want):
            assert abs(float(a) - b) <= 1e-9 * abs(b) + 1e-300, (got, want)

    for j, (ln, o) in enumerate(zip(heads, ours)):
        m = head.match(ln)
        assert m, ln
        g = m.groups()
        assert [int(g[0]), int(g[1]), int(g[2]), int(g[3]), int(g[4]), int(g[5]), int(g[7])] == \
            [o.step_num, o.n, o.nonfinite, 16, 3, o.inside_count, o.outside_count]
        assert o.step_num == 10 * j
        close([g[6], g[8], g[9]], [o.inside_mass, o.outside_mass, o.mass])
        close(g[10:25], [*o.center, *o.velocity, *o.axis, *o.shape])
        for k in range(16):
            m = row.match(rows[16 * j + k])
            assert m, rows[16 * j + k]
            g = m.groups()
            assert [int(g[0]), int(g[1]), int(g[4])] == [o.step_num, k, int(o.count[k])]
            close(g[2:4], o.edges[k:k + 2])
            close(g[5:], [o.bin_mass[k], o.m_r[k], o.m_ur[k], o.m_ur2[k], o.m_uphi[k], o.m_uphi2[k], o.m_u2[k],
                          *o.ang[k]])
    # the disc rotates: a rotation curve of one sign, and the central mass lies below edges[0]
    last = ours[-1]
    full = last.count > 0
    assert full.sum() >= 8 and last.inside_mass >= 150000.0
    assert np.all(last.mean_uphi[full] < 0) or np.all(last.mean_uphi[full] > 0)
    # without --radial the output has no such line
    p = subprocess.run([cli, "--sim", "naive", "--n", "256", "--steps", "2"], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and "Radial" not in p.stdout
