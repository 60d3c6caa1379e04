"""nb_disc_modes_sim on the device (csrc/nb_modes.hip) against the numpy restatement of its rule (tests/modes_ref.py)
on read_particles() of the same moment: every integer and every double equal.  Lists across every run and chunk
border, nbins 1 to 256, mmax 0 and 8, empty bins, everything in one bin, inside or outside, bodies at the centre,
non-finite and massless bodies, a tilted axis, the centre of mass against an explicit centre, the three inits; a
bin's bits independent of the other bins and of the call; the trajectory; the counts of the cylindrical radial
profile; the runner, the C++ mirror behind the CLI, and the refusals.  `-m gpu`."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import modes_ref as M
from tests.helpers import ROOT

pytestmark = pytest.mark.gpu

G, E, DT = 1e-6, 1e-4, 0.016
TILTED = (0.3, -0.5, 0.8)
CENTRE = (0.25, -0.5, 0.125)      # binary32 values: a body can sit exactly on it
VELOCITY = (0.01, -0.02, 0.005)


def _sim(nb, kind, parts, theta=0.75, **kw):
    sp = nb.SimParams(particle_num=len(parts), g=G, e=E, dt=DT)
    if kind == "naive":
        return nb.NaiveSim.from_particles(sp, None, parts, **kw)
    return nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(theta), parts, **kw)


def _check(d, ref):
    """Every value equal: integers with ==, doubles with == (NaN where the restatement has NaN)."""
    for k in ("n", "nonfinite", "inside_count", "outside_count"):
        assert getattr(d, k) == ref[k], (k, getattr(d, k), ref[k])
    assert np.array_equal(d.count, ref["count"]), (d.count, ref["count"])
    for k in ("inside_mass", "outside_mass", "mass"):
        assert np.array_equal(getattr(d, k), ref[k], equal_nan=True), (k, getattr(d, k), ref[k])
    for k in ("axis", "e1", "e2", "m_r", "m_h2"):
        assert np.array_equal(getattr(d, k), ref[k], equal_nan=True), (k, getattr(d, k), ref[k])
    bad = ~((d.modes == ref["modes"]) | (np.isnan(d.modes) & np.isnan(ref["modes"])))
    assert not bad.any(), (np.argwhere(bad)[:8], d.modes[bad][:8], ref["modes"][bad][:8])


def _against_ref(sim, edges, mmax, axis, center, velocity=None):
    d = sim.disc_modes(edges, mmax=mmax, axis=axis, center=center, velocity=velocity)
    ref = M.modes_ref(sim.read_particles(), edges, mmax, axis, d.center, d.velocity)
    _check(d, ref)
    return d, ref


def annuli(seed, lengths, edges, axis, centre, inside=0, outside=0, at_centre=0, massless=0):
    """Bodies placed into the annuli of `edges` about `axis` through `centre`, lengths[k] of them in bin k, `inside`
    below edges[0] and `outside` beyond edges[-1], in a random body order; then `at_centre` bodies exactly on the
    centre, and `massless` of all of them given mass 0."""
    rng = np.random.default_rng(seed)
    n, e1, e2 = M.frame(axis)
    lo = np.concatenate([np.repeat(edges[:-1], lengths), np.full(inside, 0.05 * edges[0]),
                         np.full(outside, 1.05 * edges[-1])])
    hi = np.concatenate([np.repeat(edges[1:], lengths), np.full(inside, 0.9 * edges[0]), np.full(outside, 3.0 * edges[-1])])
    k = len(lo)
    radius = lo + (hi - lo) * rng.uniform(0.02, 0.98, k)
    phi = rng.uniform(0.0, 2.0 * np.pi, k)
    h = rng.normal(0.0, 0.05, k)
    x = radius[:, None] * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2) + h[:, None] * n + np.asarray(centre)
    v = rng.normal(0.0, 0.3, (k, 3)) + 0.8 * np.cross(n, x - np.asarray(centre))
    mass = 10.0 ** rng.uniform(-3.0, 1.0, k)
    order = rng.permutation(k)
    parts = M.make_parts(x[order], v[order], mass[order])
    extra = M.make_parts(np.tile(np.asarray(centre), (at_centre, 1)), rng.normal(0.0, 0.3, (at_centre, 3)),
                         np.ones(at_centre))
    parts = np.concatenate([parts, extra])
    pick = rng.permutation(len(parts))
    parts["mass"][pick[:massless]] = 0.0
    return parts


@functools.lru_cache(maxsize=None)
def _borders(which):
    """Two states of under 20,000 bodies whose bins have the lengths of the run and chunk borders (checked by the
    tests through the restatement's counts)."""
    if which == "a":
        lengths, axis, centre = (1, 63, 64, 65, 4095, 0, 8193), TILTED, CENTRE
    else:
        lengths, axis, centre = (4096, 0, 4097, 2, 129), (0.0, 1.0, 0.0), (0.0, 0.0, 0.0)
    edges = 0.5 + 0.25 * np.arange(len(lengths) + 1)
    parts = annuli(11 if which == "a" else 12, lengths, edges, axis, centre, inside=70, outside=130, at_centre=3,
                   massless=40)
    parts.setflags(write=False)
    edges.setflags(write=False)
    return parts, edges, lengths, axis, centre


def _spoil(parts, seed, massless, bad):
    """A copy with `massless` bodies given mass 0 and `bad` bodies a non-finite position, velocity or mass."""
    rng = np.random.default_rng(seed)
    parts = parts.copy()
    pick = rng.permutation(len(parts))[:massless + bad]
    parts["mass"][pick[:massless]] = 0.0
    for j, i in enumerate(pick[massless:]):
        if j % 3 == 2:
            parts["mass"][i] = np.inf
        else:
            parts[("position", "velocity")[j % 3]][i, j % 3] = (np.nan, -np.inf)[j % 2]
    return parts


@pytest.mark.parametrize("which,mmax,com", [("a", 8, False), ("a", 0, True), ("b", 8, True), ("b", 3, False)])
def test_every_border(gpu, which, mmax, com):
    parts, edges, lengths, axis, centre = _borders(which)
    sim = _sim(gpu, "naive", parts)
    if com:
        d, ref = _against_ref(sim, edges, mmax, axis, "com")
    else:
        d, ref = _against_ref(sim, edges, mmax, axis, centre, VELOCITY)
        assert tuple(d.count) == lengths  # the explicit centre is the one the state was built about
        assert d.inside_count == 70 + 3 and d.outside_count == 130 and d.nonfinite == 0
        assert d.velocity.tolist() == list(VELOCITY) and d.center.tolist() == list(centre)
    assert d.modes.shape == (len(lengths), mmax + 1, 6) and d.step_num == 0


def test_nonfinite_and_massless_bodies(gpu):
    parts, edges, lengths, axis, centre = _borders("a")
    spoiled = _spoil(parts, 5, massless=200, bad=31)
    sim = _sim(gpu, "naive", spoiled)
    d, ref = _against_ref(sim, edges, 8, axis, centre, VELOCITY)
    assert d.nonfinite == 31 and int(d.count.sum()) + d.inside_count + d.outside_count == len(parts) - 31
    d, ref = _against_ref(sim, edges, 2, axis, "com")
    assert d.nonfinite == 31


def test_bodies_at_the_centre_count_in_mode_0_alone(gpu):
    parts = annuli(8, (40, 70), np.array([0.0, 1.0, 2.0]), TILTED, CENTRE, at_centre=5)
    sim = _sim(gpu, "naive", parts)
    d, ref = _against_ref(sim, [0.0, 1.0, 2.0], 8, TILTED, CENTRE)
    assert d.count.tolist() == [45, 70] and d.inside_count == 0
    alone = _sim(gpu, "naive", parts[-5:])
    d, ref = _against_ref(alone, [0.0, 1.0], 8, TILTED, CENTRE)
    assert d.count.tolist() == [5] and d.modes[0, 0, 0] == 5.0 and not d.modes[0, 1:, :2].any()
    assert d.modes[0, 0, 2] == 0.0  # w = 0 at the centre


@functools.lru_cache(maxsize=None)
def _disc():
    rng = np.random.default_rng(21)
    n = 6000
    radius = rng.exponential(0.6, n) + 0.01
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    x = np.stack([radius * np.cos(phi), rng.normal(0.0, 0.03, n), radius * np.sin(phi)], axis=1)
    v = np.stack([-np.sin(phi), rng.normal(0.0, 0.05, n), np.cos(phi)], axis=1) * 0.7
    parts = M.make_parts(x, v, 10.0 ** rng.uniform(-2.0, 0.0, n))
    parts.setflags(write=False)
    return parts


@pytest.mark.parametrize("nbins,log", [(1, False), (2, False), (64, True), (256, False), (256, True)])
def test_nbins(gpu, nbins, log):
    sim = _sim(gpu, "naive", _disc())
    edges = gpu.radial_edges(0.02 if log else 0.0, 6.0, nbins, log)
    d, ref = _against_ref(sim, edges, 4, (0.0, 1.0, 0.0), "com")
    if nbins == 256:
        assert (d.count == 0).any() and (d.count > 0).any()  # empty bins among full ones
        assert not d.modes[d.count == 0].any()


@pytest.mark.parametrize("edges,where", [((0.0, 100.0), "bin"), ((50.0, 60.0, 70.0), "inside"),
                                         ((1e-6, 2e-6, 3e-6), "outside")])
def test_every_body_in_one_list(gpu, edges, where):
    parts = _disc()
    sim = _sim(gpu, "naive", parts)
    d, ref = _against_ref(sim, edges, 8, TILTED, (0.0, 0.0, 0.0))
    got = {"bin": int(d.count[0]), "inside": d.inside_count, "outside": d.outside_count}[where]
    assert got == len(parts)


def test_the_centre_of_mass_is_the_diagnostics(gpu):
    sim = _sim(gpu, "naive", _disc())
    edges = np.linspace(0.0, 3.0, 13)
    d = sim.disc_modes(edges, mmax=4, center="com")
    diag = sim.diagnostics()
    assert d.center.tobytes() == np.asarray(diag.com, dtype=np.float64).tobytes()
    assert d.velocity.tobytes() == (np.asarray(diag.momentum, dtype=np.float64) / diag.mass).tobytes()
    explicit = sim.disc_modes(edges, mmax=4, center=d.center, velocity=d.velocity)
    assert explicit.modes.tobytes() == d.modes.tobytes() and np.array_equal(explicit.count, d.count)
    assert (explicit.m_r.tobytes(), explicit.m_h2.tobytes(), explicit.mass) == (d.m_r.tobytes(), d.m_h2.tobytes(), d.mass)
    assert d.flags == 1 and explicit.flags == 0


@pytest.mark.parametrize("init", ["uniform_init", "disc_init", "spherical_init"])
def test_the_three_inits(gpu, init):
    sp = gpu.SimParams(particle_num=4096, g=G, e=E, dt=DT)
    sim = gpu.NaiveSim.new(sp, None, getattr(gpu.inits, init))
    d, ref = _against_ref(sim, gpu.radial_edges(0.05, 2.0, 16, True), 4, (0.0, 1.0, 0.0), "com")
    assert int(d.count.sum()) > 0


def test_a_bins_bits_are_its_own(gpu):
    """The same bin with the edges changed elsewhere, with nbins changed, and with bodies added outside it at higher
    indices: the same 6 (mmax + 1) + 2 doubles."""
    parts, edges, lengths, axis, centre = _borders("a")
    sim = _sim(gpu, "naive", parts)
    base = sim.disc_modes(edges, mmax=8, axis=axis, center=centre, velocity=VELOCITY)
    k = 6  # the bin of 8,193 members: more than two chunks
    lo, hi = edges[k], edges[k + 1]

    def same(d, j):
        assert d.count[j] == base.count[k]
        assert d.modes[j].tobytes() == base.modes[k].tobytes()
        assert (d.m_r[j], d.m_h2[j]) == (base.m_r[k], base.m_h2[k])

    same(sim.disc_modes([lo, hi], mmax=8, axis=axis, center=centre, velocity=VELOCITY), 0)
    same(sim.disc_modes([0.1, 0.9, 1.3, lo, hi, 5.0], mmax=8, axis=axis, center=centre, velocity=VELOCITY), 3)
    other = np.concatenate([np.linspace(0.0, lo, 200), [hi]])
    same(sim.disc_modes(other, mmax=8, axis=axis, center=centre, velocity=VELOCITY), 199)
    more = annuli(13, (300, 0, 0, 0, 500, 0, 0), edges, axis, centre, inside=100, outside=200)
    bigger = _sim(gpu, "naive", np.concatenate([parts, more]))
    same(bigger.disc_modes(edges, mmax=8, axis=axis, center=centre, velocity=VELOCITY), k)
    # fewer modes are the first of more
    fewer = sim.disc_modes(edges, mmax=3, axis=axis, center=centre, velocity=VELOCITY)
    assert fewer.modes.tobytes() == base.modes[:, :4].tobytes()


def test_two_calls_return_the_same_bits(gpu):
    parts, edges, lengths, axis, centre = _borders("b")
    sim = _sim(gpu, "naive", parts)
    a = sim.disc_modes(edges, mmax=8, axis=axis, center="com")
    sim.disc_modes(np.linspace(0.0, 4.0, 100), mmax=2, axis=TILTED, center=centre)  # (another shape in between)
    b = sim.disc_modes(edges, mmax=8, axis=axis, center="com")
    for k in ("modes", "m_r", "m_h2", "count", "center", "velocity"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
    assert (a.mass, a.inside_mass, a.outside_mass) == (b.mass, b.inside_mass, b.outside_mass)


def _clean(seed, n):
    rng = np.random.default_rng(seed)
    radius = rng.uniform(0.1, 2.0, n)
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    x = np.stack([radius * np.cos(phi), rng.normal(0.0, 0.05, n), radius * np.sin(phi)], axis=1)
    v = np.stack([-np.sin(phi), np.zeros(n), np.cos(phi)], axis=1) * 0.02
    return M.make_parts(x, v, rng.uniform(0.5, 1.5, n))


@pytest.mark.parametrize("kind", ["naive", "tree", "tree_graph"])
def test_a_call_does_not_perturb_the_trajectory(gpu, kind):
    parts = _clean(31, 5000)
    edges = np.linspace(0.0, 2.5, 11)
    a, b = _sim(gpu, kind[:5].rstrip("_"), parts), _sim(gpu, kind[:5].rstrip("_"), parts)
    if kind == "tree_graph":
        a.set_tuning("tree_use_graph", 1)
        b.set_tuning("tree_use_graph", 1)
    a.disc_modes(edges, mmax=4)
    for _ in range(3):
        a.encode()
        b.encode()
    d = a.disc_modes(edges, mmax=8, axis=TILTED, center=(0.0, 0.0, 0.0))
    assert d.step_num == 3
    a.encode()
    b.encode()
    assert a.dest_particle_slice().tobytes() == b.dest_particle_slice().tobytes()


@pytest.mark.parametrize("graph", [0, 1])
def test_after_steps_of_the_tree_simulator(gpu, graph):
    """A TreeSim reorders its bodies at every step: the lists are those of its own read_particles()."""
    sim = _sim(gpu, "tree", _clean(32, 9000))
    sim.set_tuning("tree_use_graph", graph)
    for _ in range(3):
        sim.encode()
    d, ref = _against_ref(sim, np.linspace(0.0, 2.5, 7), 8, (0.0, 1.0, 0.0), "com")
    assert d.step_num == 3 and d.count.max() > 1024


def test_counts_are_the_cylindrical_radial_profiles(gpu):
    parts, edges, lengths, axis, centre = _borders("a")
    sim = _sim(gpu, "naive", _spoil(parts, 6, massless=10, bad=9))
    for modes_kw, radial_kw in ((dict(center=centre, velocity=VELOCITY), dict(center=centre, velocity=VELOCITY)),
                                (dict(center="com"), dict(center="com"))):
        d = sim.disc_modes(edges, mmax=1, axis=axis, **modes_kw)
        r = sim.radial_profile(edges, cylindrical=True, axis=axis, **radial_kw)
        assert np.array_equal(d.count, r.count)
        assert (d.inside_count, d.outside_count, d.nonfinite) == (r.inside_count, r.outside_count, r.nonfinite)
        assert d.center.tobytes() == r.center.tobytes() and d.axis.tobytes() == r.axis.tobytes()
        assert d.velocity.tobytes() == r.velocity.tobytes()


def _raw(nb, call, handle, edges=(0.5, 1.0, 2.0), mmax=4, flags=0, nbins=None, axis=(0.0, 1.0, 0.0)):
    from wgpu_n_body_amd import _lib
    e = np.asarray(edges, dtype=np.float64)
    p = _lib.nb_modes_params()
    p.nbins, p.mmax, p.flags = (len(e) - 1 if nbins is None else nbins), mmax, flags
    for k in range(3):
        p.axis[k] = axis[k]
    p.edges = e.ctypes.data_as(C.POINTER(C.c_double))
    head = _lib.nb_modes_head()
    head.n = 77
    bins = np.full(300 * 24, 7, np.uint8)
    modes = np.full(300 * 9 * 6, -7.0)
    rc = call(handle, C.byref(p), C.byref(head), bins.ctypes.data, modes.ctypes.data)
    untouched = head.n == 77 and np.all(bins == 7) and np.all(modes == -7.0)
    return rc, untouched, head, modes


def test_refusals_and_an_empty_state(gpu):
    nb = gpu
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    sim = _sim(nb, "naive", _clean(33, 300))
    for word, kw in ((b"nbins", dict(nbins=0)), (b"nbins", dict(nbins=257)), (b"mmax", dict(mmax=9)),
                     (b"flag", dict(flags=6)), (b"edges[2]", dict(edges=(0.5, 1.0, 1.0))),
                     (b"axis", dict(axis=(0.0, 0.0, 0.0)))):
        rc, untouched, _, _ = _raw(nb, L.nb_disc_modes_sim, sim._h, **kw)
        assert rc == _lib.NB_ERR_INVALID and word in L.nb_last_error() and untouched, word
    rc, untouched, head, modes = _raw(nb, L.nb_disc_modes_sim, sim._h)
    assert rc == 0 and head.n == 300 and not untouched and np.all(modes[2 * 5 * 6:] == -7.0)  # nothing past the end
    shard = nb.NaiveSim.from_particles(nb.SimParams(particle_num=300), None, _clean(33, 300),
                                       placement=nb.Placement(world=2))
    rc, untouched, _, _ = _raw(nb, L.nb_disc_modes_sim, shard._h)
    assert rc == _lib.NB_ERR_UNSUPPORTED and b"sharded" in L.nb_last_error() and untouched
    multi = nb.OfflineHeadless(nb.NaiveSim, nb.SimParams(particle_num=512), None,
                               lambda p: nb.inits.uniform_init(p, seed=1), device_ids=[0, 0])
    rc, untouched, _, _ = _raw(nb, L.nb_disc_modes_runner, multi._h)
    assert rc == _lib.NB_ERR_UNSUPPORTED and b"several-GPU" in L.nb_last_error() and untouched
    with pytest.raises(nb.NBodyError) as ex:
        multi.disc_modes([0.5, 1.0])
    assert ex.value.code == _lib.NB_ERR_UNSUPPORTED
    multi.destroy()
    empty = _sim(nb, "naive", _clean(33, 300)[:0])
    d = empty.disc_modes([0.5, 1.0, 2.0], mmax=2, center=(1.0, 2.0, 3.0), velocity=(0.5, 0.0, 0.0))
    assert d.n == 0 and not d.modes.any() and not d.count.any() and d.mass == 0.0
    assert d.center.tolist() == [1.0, 2.0, 3.0] and d.velocity.tolist() == [0.5, 0.0, 0.0]
    assert np.isnan(empty.disc_modes([0.5, 1.0]).center).all()  # the centre of no mass
    assert np.isnan(d.amplitude(2)).all()


def test_runner_cpp_mirror_and_cli(gpu):
    """The ring with a known mode through nb_disc_modes_runner, the runner against its simulator, and headless
    --modes (the C++ mirror) printing what the Python runner returns for the same seeded disc."""
    nb = gpu
    from wgpu_n_body_amd import _lib
    eps, phi0, omega0 = 0.25, 0.3, 1.7
    ring = M.ring(360, 1.0, eps, phi0, omega0, TILTED)
    sp = nb.SimParams(particle_num=360, g=G, e=E, dt=DT)
    runner = nb.OfflineHeadless.new(nb.NaiveSim, sp, None, lambda _p: ring)
    d = runner.disc_modes([0.5, 1.5], mmax=4, axis=TILTED, center=(0.0, 0.0, 0.0))
    _check(d, M.modes_ref(runner.read_particles(), [0.5, 1.5], 4, TILTED, (0.0, 0.0, 0.0)))
    assert abs(d.amplitude(2)[0] - eps / 2) < 1e-6 and abs(d.phase(2)[0] - phi0) < 1e-6
    assert abs(d.pattern_speed(2)[0] - omega0) < 1e-6
    assert d.amplitude(1)[0] < 1e-6 and d.amplitude(3)[0] < 1e-6
    held = nb.Simulator(_lib.lib().nb_runner_sim(runner._h), borrowed=True)
    via_sim = held.disc_modes([0.5, 1.5], mmax=4, axis=TILTED, center=(0.0, 0.0, 0.0))
    assert via_sim.modes.tobytes() == d.modes.tobytes()

    sp = nb.SimParams(particle_num=4096, g=1e-4, e=E, dt=DT)
    disc = nb.OfflineHeadless.new(nb.TreeSim, sp, nb.AddParams.TreeSimParams(0.75), nb.inits.disc_init)
    exe = os.path.join(ROOT, "wgpu_n_body_amd", "headless")
    base = [exe, "--sim", "tree", "--n", "4096", "--init", "disc", "--g", "1e-4", "--steps", "2", "--modes", "2",
            "--modes-range", "0.05,1.5", "--modes-bins", "12", "--modes-m", "3"]
    for extra, kw in (([], dict(center="com")),
                      (["--modes-axis", "0.3,-0.5,0.8", "--modes-center", "0.01,0,-0.02", "--modes-log", "1"],
                       dict(axis=TILTED, center=(0.01, 0.0, -0.02), log=True))):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        lines = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("modes ")]
        assert [ln[1] for ln in lines] == ["0", "2"]
        want = disc.disc_modes(nbins=12, rmin=0.05, rmax=1.5, mmax=3, **kw)
        a2, k = want.bar_strength()
        got = np.array([float(x) for x in lines[0][2:]])
        tilt = want.warp_tilt()
        expect = [a2, want.m_r[k] / want.bin_mass[k], want.phase(2)[k], want.pattern_speed(2)[k],
                  np.max(tilt[np.isfinite(tilt)])]
        assert np.array_equal(got[:4], np.array(expect[:4])), (got, expect)  # %.17g round-trips
        assert abs(got[4] - expect[4]) <= 1e-15 * expect[4]  # (hypot: the C library's against numpy's)
    bad = subprocess.run(base[:-6] + ["--modes", "1"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--modes-range" in bad.stderr
