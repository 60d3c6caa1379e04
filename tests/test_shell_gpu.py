"""nb_shell_modes_sim on the device (csrc/nb_shell.hip) against the numpy restatement of its rule (tests/shell_ref.py)
on read_particles() of the same moment: every integer and every double equal.  Lists across every run and chunk
border at lmax 0, 4 with rates and 6, nbins 1 and 256, everything in one bin, inside or outside, bodies on the centre
and on the polar axis, non-finite and massless bodies, a tilted axis, the centre of mass against an explicit centre,
both simulators after steps, the three inits; a bin's bits independent of the other bins and of the call; the
trajectory; the counts of the spherical radial profile; a planar state against disc_modes; the runner, the C++ mirror
behind the CLI, and the refusals.  `-m gpu`."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import shell_ref as S
from tests.helpers import ROOT

pytestmark = pytest.mark.gpu

G, E, DT = 1e-6, 1e-4, 0.016
TILTED = (0.3, -0.5, 0.8)
AXIS_Y = (0.0, 1.0, 0.0)
CENTRE = (0.25, -0.5, 0.125)      # binary32 values: a body can sit exactly on it
VELOCITY = (0.01, -0.02, 0.005)


def _sim(nb, kind, parts, theta=0.75, **kw):
    sp = nb.SimParams(particle_num=len(parts), g=G, e=E, dt=DT)
    if kind == "naive":
        return nb.NaiveSim.from_particles(sp, None, parts, **kw)
    return nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(theta), parts, **kw)


def _same(got, want):
    return (got == want) | (np.isnan(got) & np.isnan(want))


def _check(d, ref):
    """Every value equal: integers with ==, doubles with == (NaN where the restatement has NaN)."""
    for k in ("n", "nonfinite", "inside_count", "outside_count"):
        assert getattr(d, k) == ref[k], (k, getattr(d, k), ref[k])
    assert np.array_equal(d.count, ref["count"]), (d.count, ref["count"])
    for k in ("inside_mass", "outside_mass", "mass"):
        assert np.array_equal(getattr(d, k), ref[k], equal_nan=True), (k, getattr(d, k), ref[k])
    for k in ("axis", "e1", "e2", "m_r", "m_ur"):
        assert np.array_equal(getattr(d, k), ref[k], equal_nan=True), (k, getattr(d, k), ref[k])
    bad = ~_same(d.coef, ref["coef"])
    assert not bad.any(), (np.argwhere(bad)[:8], d.coef[bad][:8], ref["coef"][bad][:8])
    assert (d.rate is None) == (ref["rate"] is None)
    if d.rate is not None:
        bad = ~_same(d.rate, ref["rate"])
        assert not bad.any(), (np.argwhere(bad)[:8], d.rate[bad][:8], ref["rate"][bad][:8])


def _against_ref(sim, edges, lmax, axis, center, velocity=None, rates=False):
    d = sim.shell_modes(edges, lmax=lmax, rates=rates, axis=axis, center=center, velocity=velocity)
    ref = S.shell_ref(sim.read_particles(), edges, lmax, axis, d.center, d.velocity, rates=rates)
    _check(d, ref)
    assert d.lmax == lmax and d.coef.shape == (len(edges) - 1, (lmax + 1) ** 2)
    return d, ref


def shells(seed, lengths, edges, centre, inside=0, outside=0, at_centre=0, on_axis=0, massless=0):
    """Bodies placed into the shells of `edges` about `centre`, lengths[k] of them in bin k, `inside` below edges[0]
    and `outside` beyond edges[-1], in a triaxial distribution of directions and a random body order; then
    `at_centre` bodies exactly on the centre and `on_axis` bodies exactly on the line through it along y, and
    `massless` of all of them given mass 0."""
    rng = np.random.default_rng(seed)
    edges = np.asarray(edges, dtype=np.float64)
    lo = np.concatenate([np.repeat(edges[:-1], lengths), np.full(inside, 0.05 * edges[0]),
                         np.full(outside, 1.05 * edges[-1])])
    hi = np.concatenate([np.repeat(edges[1:], lengths), np.full(inside, 0.9 * edges[0]), np.full(outside, 3.0 * edges[-1])])
    k = len(lo)
    radius = lo + (hi - lo) * rng.uniform(0.02, 0.98, k)
    direction = rng.normal(size=(k, 3)) * [1.0, 0.6, 0.8]
    direction /= np.linalg.norm(direction, axis=1)[:, None]
    x = radius[:, None] * direction + np.asarray(centre)
    v = rng.normal(0.0, 0.3, (k, 3)) + 0.8 * np.cross(TILTED, x - np.asarray(centre))
    mass = 10.0 ** rng.uniform(-3.0, 1.0, k)
    order = rng.permutation(k)
    parts = S.make_parts(x[order], v[order], mass[order])
    extra = S.make_parts(np.tile(np.asarray(centre), (at_centre, 1)), rng.normal(0.0, 0.3, (at_centre, 3)),
                         np.ones(at_centre))
    height = rng.uniform(edges[0], edges[-1], on_axis) * rng.choice([-1.0, 1.0], on_axis)
    polar = S.make_parts(np.asarray(centre) + height[:, None] * np.array([0.0, 1.0, 0.0]),
                         rng.normal(0.0, 0.3, (on_axis, 3)), np.full(on_axis, 0.5))
    parts = np.concatenate([parts, extra, polar])
    pick = rng.permutation(len(parts))
    parts["mass"][pick[:massless]] = 0.0
    return parts


@functools.lru_cache(maxsize=None)
def _borders(which):
    """Two states of under 20,000 bodies whose bins have the lengths of the run and chunk borders (checked by the
    tests against the explicit centre)."""
    if which == "a":
        lengths, axis, centre = (1, 63, 64, 65, 4095, 0, 8193), TILTED, CENTRE
    else:
        lengths, axis, centre = (4096, 0, 4097, 2, 129), AXIS_Y, (0.0, 0.0, 0.0)
    edges = 0.5 + 0.25 * np.arange(len(lengths) + 1)
    parts = shells(11 if which == "a" else 12, lengths, edges, centre, inside=70, outside=130, at_centre=3,
                   massless=40)
    assert len(parts) < 20000
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


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("lmax,rates,com", [(0, False, True), (4, True, False), (6, False, False), (0, True, False),
                                            (4, True, True)])
def test_every_border(gpu, which, lmax, rates, com):
    """Lists of 1, 63, 64, 65, 4095, 0 and 8193 members (a) and of 4096, 0, 4097, 2 and 129 (b)."""
    parts, edges, lengths, axis, centre = _borders(which)
    sim = _sim(gpu, "naive", parts)
    if com:
        d, ref = _against_ref(sim, edges, lmax, axis, "com", rates=rates)
    else:
        d, ref = _against_ref(sim, edges, lmax, axis, centre, VELOCITY, rates=rates)
        assert tuple(d.count) == lengths  # the explicit centre is the one the state was built about
        assert d.inside_count == 70 + 3 and d.outside_count == 130 and d.nonfinite == 0
        assert d.velocity.tolist() == list(VELOCITY) and d.center.tolist() == list(centre)
    assert d.step_num == 0 and d.flags == (1 if com else 0) | (2 if rates else 0)
    assert np.array_equal(d.bin_mass, ref["coef"][:, 0])


def test_nonfinite_and_massless_bodies(gpu):
    parts, edges, lengths, axis, centre = _borders("a")
    spoiled = _spoil(parts, 5, massless=200, bad=31)
    sim = _sim(gpu, "naive", spoiled)
    d, ref = _against_ref(sim, edges, 6, axis, centre, VELOCITY)
    assert d.nonfinite == 31 and int(d.count.sum()) + d.inside_count + d.outside_count == len(parts) - 31
    d, ref = _against_ref(sim, edges, 2, axis, "com", rates=True)
    assert d.nonfinite == 31


def test_bodies_on_the_centre_count_in_l0_alone(gpu):
    parts = shells(8, (40, 70), [0.0, 1.0, 2.0], CENTRE, at_centre=5)
    sim = _sim(gpu, "naive", parts)
    d, ref = _against_ref(sim, [0.0, 1.0, 2.0], 4, TILTED, CENTRE, VELOCITY, rates=True)
    assert d.count.tolist() == [45, 70] and d.inside_count == 0
    alone = _sim(gpu, "naive", parts[-5:])
    for lmax, rates in ((6, False), (4, True)):
        d, ref = _against_ref(alone, [0.0, 1.0], lmax, TILTED, CENTRE, VELOCITY, rates=rates)
        assert d.count.tolist() == [5] and d.coef[0, 0] == 5.0 and not d.coef[0, 1:].any()
        assert not np.signbit(d.coef).any() and d.m_r[0] == 0.0 and d.m_ur[0] == 0.0
        assert d.rate is None or (not d.rate.any() and not np.signbit(d.rate).any())


def test_bodies_on_the_polar_axis(gpu):
    """alpha = beta = 0 exactly: every m >= 1 term is a zero and zeta = +-1, where dP_l / d zeta is largest."""
    parts = shells(9, (30, 50), [0.25, 1.0, 2.0], CENTRE, on_axis=90)
    sim = _sim(gpu, "naive", parts)
    for lmax, rates in ((6, False), (4, True)):
        d, ref = _against_ref(sim, [0.25, 1.0, 2.0], lmax, AXIS_Y, CENTRE, VELOCITY, rates=rates)
        assert int(d.count.sum()) == 170
    alone = _sim(gpu, "naive", parts[-90:])
    d, ref = _against_ref(alone, [0.25, 1.0, 2.0], 6, AXIS_Y, CENTRE)
    for l in range(7):
        for m in range(1, l + 1):
            assert not d.coefficient(l, m).any() and not d.coefficient(l, m, sine=True).any()
    assert np.array_equal(d.coefficient(2, 0), d.bin_mass) and np.array_equal(d.coefficient(6, 0), d.bin_mass)


@functools.lru_cache(maxsize=None)
def _halo():
    rng = np.random.default_rng(21)
    n = 6000
    radius = rng.exponential(0.6, n) + 0.01
    direction = rng.normal(size=(n, 3)) * [1.0, 0.5, 0.75]
    direction /= np.linalg.norm(direction, axis=1)[:, None]
    x = radius[:, None] * direction
    v = rng.normal(0.0, 0.3, (n, 3)) + 0.5 * np.cross(TILTED, x)
    parts = S.make_parts(x, v, 10.0 ** rng.uniform(-2.0, 0.0, n))
    parts.setflags(write=False)
    return parts


@pytest.mark.parametrize("nbins,log", [(1, False), (2, False), (64, True), (256, False), (256, True)])
def test_nbins(gpu, nbins, log):
    sim = _sim(gpu, "naive", _halo())
    edges = gpu.radial_edges(0.02 if log else 0.0, 6.0, nbins, log)
    d, ref = _against_ref(sim, edges, 4, AXIS_Y, "com", rates=True)
    if nbins == 256:
        assert (d.count == 0).any() and (d.count > 0).any()  # empty bins among full ones
        assert not d.coef[d.count == 0].any() and not d.rate[d.count == 0].any()


@pytest.mark.parametrize("edges,where", [((0.0, 100.0), "bin"), ((50.0, 60.0, 70.0), "inside"),
                                         ((1e-6, 2e-6, 3e-6), "outside")])
def test_every_body_in_one_list(gpu, edges, where):
    parts = _halo()
    sim = _sim(gpu, "naive", parts)
    d, ref = _against_ref(sim, edges, 6, TILTED, (0.0, 0.0, 0.0))
    got = {"bin": int(d.count[0]), "inside": d.inside_count, "outside": d.outside_count}[where]
    assert got == len(parts)
    if where != "bin":
        assert not d.coef.any()


def test_the_centre_of_mass_is_the_diagnostics(gpu):
    sim = _sim(gpu, "naive", _halo())
    edges = np.linspace(0.0, 3.0, 13)
    d = sim.shell_modes(edges, lmax=4, rates=True, center="com")
    diag = sim.diagnostics()
    assert d.center.tobytes() == np.asarray(diag.com, dtype=np.float64).tobytes()
    assert d.velocity.tobytes() == (np.asarray(diag.momentum, dtype=np.float64) / diag.mass).tobytes()
    explicit = sim.shell_modes(edges, lmax=4, rates=True, center=d.center, velocity=d.velocity)
    for k in ("coef", "rate", "count", "m_r", "m_ur"):
        assert getattr(explicit, k).tobytes() == getattr(d, k).tobytes(), k
    assert explicit.mass == d.mass and d.flags == 3 and explicit.flags == 2
    dens = sim.shell_modes(edges, lmax=2, center="density")
    want = sim.knn_density(6, neighbours=False)
    assert dens.center.tobytes() == np.asarray(want.center, dtype=np.float64).tobytes() and dens.flags == 0


@pytest.mark.parametrize("init", ["uniform_init", "disc_init", "spherical_init"])
def test_the_three_inits(gpu, init):
    sp = gpu.SimParams(particle_num=4096, g=G, e=E, dt=DT)
    sim = gpu.NaiveSim.new(sp, None, getattr(gpu.inits, init))
    d, ref = _against_ref(sim, gpu.radial_edges(0.05, 2.0, 16, True), 4, AXIS_Y, "com", rates=True)
    assert int(d.count.sum()) > 0


def test_a_bins_bits_are_its_own(gpu):
    """The same bin with the edges changed elsewhere, with nbins changed, with bodies added outside it at higher
    indices, with fewer degrees and without the rates: the same doubles."""
    parts, edges, lengths, axis, centre = _borders("a")
    sim = _sim(gpu, "naive", parts)
    kw = dict(lmax=4, rates=True, axis=axis, center=centre, velocity=VELOCITY)
    base = sim.shell_modes(edges, **kw)
    k = 6  # the bin of 8,193 members: more than two chunks
    lo, hi = edges[k], edges[k + 1]

    def same(d, j):
        assert d.count[j] == base.count[k]
        assert d.coef[j].tobytes() == base.coef[k].tobytes() and d.rate[j].tobytes() == base.rate[k].tobytes()
        assert (d.m_r[j], d.m_ur[j]) == (base.m_r[k], base.m_ur[k])

    same(sim.shell_modes([lo, hi], **kw), 0)
    same(sim.shell_modes([0.1, 0.4, 0.6, lo, hi, 5.0], **kw), 3)
    other = np.concatenate([np.linspace(0.0, lo, 200), [hi]])
    same(sim.shell_modes(other, **kw), 199)
    more = shells(13, (300, 0, 0, 0, 500, 0, 0), edges, centre, inside=100, outside=200)
    bigger = _sim(gpu, "naive", np.concatenate([parts, more]))
    same(bigger.shell_modes(edges, **kw), k)
    # fewer degrees are the first of more, and the sums do not depend on the rates being asked for
    fewer = sim.shell_modes(edges, **dict(kw, lmax=2))
    assert fewer.coef.tobytes() == base.coef[:, :9].tobytes() and fewer.rate.tobytes() == base.rate[:, :9].tobytes()
    plain = sim.shell_modes(edges, **dict(kw, lmax=6, rates=False))
    assert plain.coef[:, :25].tobytes() == base.coef.tobytes() and plain.rate is None


def test_two_calls_return_the_same_bits(gpu):
    parts, edges, lengths, axis, centre = _borders("b")
    sim = _sim(gpu, "naive", parts)
    a = sim.shell_modes(edges, lmax=4, rates=True, axis=axis, center="com")
    sim.shell_modes(np.linspace(0.0, 4.0, 100), lmax=6, axis=TILTED, center=centre)  # (another shape in between)
    b = sim.shell_modes(edges, lmax=4, rates=True, axis=axis, center="com")
    for k in ("coef", "rate", "m_r", "m_ur", "count", "center", "velocity"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
    assert (a.mass, a.inside_mass, a.outside_mass) == (b.mass, b.inside_mass, b.outside_mass)


def _clean(seed, n):
    rng = np.random.default_rng(seed)
    radius = rng.uniform(0.1, 2.0, n)
    direction = rng.normal(size=(n, 3)) * [1.0, 0.6, 0.8]
    direction /= np.linalg.norm(direction, axis=1)[:, None]
    x = radius[:, None] * direction
    v = 0.02 * np.cross(AXIS_Y, x)
    return S.make_parts(x, v, rng.uniform(0.5, 1.5, n))


@pytest.mark.parametrize("kind", ["naive", "tree", "tree_graph"])
def test_a_call_does_not_perturb_the_trajectory(gpu, kind):
    parts = _clean(31, 5000)
    edges = np.linspace(0.0, 2.5, 11)
    a, b = _sim(gpu, kind[:5].rstrip("_"), parts), _sim(gpu, kind[:5].rstrip("_"), parts)
    if kind == "tree_graph":
        a.set_tuning("tree_use_graph", 1)
        b.set_tuning("tree_use_graph", 1)
    a.shell_modes(edges, lmax=4)
    for _ in range(3):
        a.encode()
        b.encode()
    d = a.shell_modes(edges, lmax=4, rates=True, axis=TILTED, center=(0.0, 0.0, 0.0))
    assert d.step_num == 3
    a.encode()
    b.encode()
    assert a.dest_particle_slice().tobytes() == b.dest_particle_slice().tobytes()


@pytest.mark.parametrize("kind,graph", [("naive", 0), ("tree", 0), ("tree", 1)])
def test_after_steps_of_both_simulators(gpu, kind, graph):
    """A TreeSim reorders its bodies at every step: the lists are those of its own read_particles()."""
    sim = _sim(gpu, kind, _clean(32, 9000))
    if kind == "tree":
        sim.set_tuning("tree_use_graph", graph)
    for _ in range(3):
        sim.encode()
    d, ref = _against_ref(sim, np.linspace(0.0, 2.5, 7), 4, AXIS_Y, "com", rates=True)
    assert d.step_num == 3 and d.count.max() > 1024
    _against_ref(sim, np.linspace(0.0, 2.5, 7), 6, TILTED, "com")


def test_counts_are_the_spherical_radial_profiles(gpu):
    parts, edges, lengths, axis, centre = _borders("a")
    sim = _sim(gpu, "naive", _spoil(parts, 6, massless=10, bad=9))
    for kw in (dict(center=centre, velocity=VELOCITY), dict(center="com")):
        d = sim.shell_modes(edges, lmax=1, axis=axis, **kw)
        r = sim.radial_profile(edges, **kw)
        assert np.array_equal(d.count, r.count)
        assert (d.inside_count, d.outside_count, d.nonfinite) == (r.inside_count, r.outside_count, r.nonfinite)
        assert d.center.tobytes() == r.center.tobytes() and d.velocity.tobytes() == r.velocity.tobytes()


def test_a_planar_state_gives_the_disc_modes_first_mode(gpu):
    """Every body in the plane y = 0 through the centre, axis (0, 1, 0): h = 0, the spherical and the cylindrical
    radius are one number, and C_11, S_11 are disc_modes' C and S of m = 1 bit for bit; C_00 is its C_0."""
    rng = np.random.default_rng(41)
    n = 9000
    radius, phi = rng.uniform(0.05, 2.0, n), rng.uniform(0.0, 2.0 * np.pi, n)
    x = np.stack([radius * np.cos(phi) + 0.25, np.zeros(n), radius * np.sin(phi) + 0.125], axis=1)
    parts = S.make_parts(x, rng.normal(0.0, 0.3, (n, 3)), 10.0 ** rng.uniform(-2.0, 0.0, n))
    sim = _sim(gpu, "naive", parts)
    edges = np.linspace(0.0, 2.0, 9)
    kw = dict(axis=AXIS_Y, center=(0.25, 0.0, 0.125), velocity=VELOCITY)
    d = sim.shell_modes(edges, lmax=2, **kw)
    m = sim.disc_modes(edges, mmax=1, **kw)
    assert np.array_equal(d.count, m.count) and d.count.max() > 1024
    assert d.coefficient(1, 1).tobytes() == m.modes[:, 1, 0].tobytes()
    assert d.coefficient(1, 1, sine=True).tobytes() == m.modes[:, 1, 1].tobytes()
    assert d.coefficient(0, 0).tobytes() == m.modes[:, 0, 0].tobytes() and d.m_r.tobytes() == m.m_r.tobytes()
    assert d.mass == m.mass and not d.coefficient(1, 0).any()


def _raw(nb, call, handle, edges=(0.5, 1.0, 2.0), lmax=4, flags=0, nbins=None, axis=(0.0, 1.0, 0.0)):
    from wgpu_n_body_amd import _lib
    e = np.asarray(edges, dtype=np.float64)
    p = _lib.nb_shell_params()
    p.nbins, p.lmax, p.flags = (len(e) - 1 if nbins is None else nbins), lmax, flags
    for k in range(3):
        p.axis[k] = axis[k]
    p.edges = e.ctypes.data_as(C.POINTER(C.c_double))
    head = _lib.nb_shell_head()
    head.n = 77
    bins = np.full(300 * 24, 7, np.uint8)
    coef = np.full(300 * 50, -7.0)
    rc = call(handle, C.byref(p), C.byref(head), bins.ctypes.data, coef.ctypes.data)
    untouched = head.n == 77 and np.all(bins == 7) and np.all(coef == -7.0)
    return rc, untouched, head, coef


def test_refusals_and_an_empty_state(gpu):
    nb = gpu
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    sim = _sim(nb, "naive", _clean(33, 300))
    for word, kw in ((b"nbins", dict(nbins=0)), (b"nbins", dict(nbins=257)), (b"lmax", dict(lmax=7)),
                     (b"lmax", dict(lmax=5, flags=2)), (b"flag", dict(flags=12)),
                     (b"edges[2]", dict(edges=(0.5, 1.0, 1.0))), (b"axis", dict(axis=(0.0, 0.0, 0.0)))):
        rc, untouched, _, _ = _raw(nb, L.nb_shell_modes_sim, sim._h, **kw)
        assert rc == _lib.NB_ERR_INVALID and word in L.nb_last_error() and untouched, word
    rc, untouched, head, coef = _raw(nb, L.nb_shell_modes_sim, sim._h)
    assert rc == 0 and head.n == 300 and not untouched and np.all(coef[2 * 25:] == -7.0)  # nothing past the end
    rc, untouched, head, coef = _raw(nb, L.nb_shell_modes_sim, sim._h, flags=2)
    assert rc == 0 and np.all(coef[:2 * 50] != -7.0) and np.all(coef[2 * 50:] == -7.0)
    shard = nb.NaiveSim.from_particles(nb.SimParams(particle_num=300), None, _clean(33, 300),
                                       placement=nb.Placement(world=2))
    rc, untouched, _, _ = _raw(nb, L.nb_shell_modes_sim, shard._h)
    assert rc == _lib.NB_ERR_UNSUPPORTED and b"sharded" in L.nb_last_error() and untouched
    multi = nb.OfflineHeadless(nb.NaiveSim, nb.SimParams(particle_num=512), None,
                               lambda p: nb.inits.uniform_init(p, seed=1), device_ids=[0, 0])
    rc, untouched, _, _ = _raw(nb, L.nb_shell_modes_runner, multi._h)
    assert rc == _lib.NB_ERR_UNSUPPORTED and b"several-GPU" in L.nb_last_error() and untouched
    with pytest.raises(nb.NBodyError) as ex:
        multi.shell_modes([0.5, 1.0])
    assert ex.value.code == _lib.NB_ERR_UNSUPPORTED
    multi.destroy()
    with pytest.raises(nb.NBodyError) as ex:
        sim.shell_modes([0.5, 1.0], lmax=5, rates=True)
    assert ex.value.code == _lib.NB_ERR_INVALID
    empty = _sim(nb, "naive", _clean(33, 300)[:0])
    d = empty.shell_modes([0.5, 1.0, 2.0], lmax=2, rates=True, center=(1.0, 2.0, 3.0), velocity=(0.5, 0.0, 0.0))
    assert d.n == 0 and not d.coef.any() and not d.rate.any() and not d.count.any() and d.mass == 0.0
    assert d.center.tolist() == [1.0, 2.0, 3.0] and d.velocity.tolist() == [0.5, 0.0, 0.0]
    assert np.isnan(empty.shell_modes([0.5, 1.0]).center).all()  # the centre of no mass
    assert np.isnan(d.relative(2)).all() and np.isnan(d.phase(2, 2)).all()


def _cli_expect(want):
    """What headless --shells prints after the step number, from a ShellModes."""
    rel2, rel1 = want.relative(2), want.relative(1)
    nan = float("nan")
    if not np.isfinite(rel2).any():
        return [nan, nan, nan, nan, np.max(rel1[np.isfinite(rel1)]) if np.isfinite(rel1).any() else nan]
    k = int(np.argmax(np.where(np.isfinite(rel2), rel2, -np.inf)))
    speed = want.pattern_speed(2, 2)[k] if want.rate is not None else nan
    return [rel2[k], want.m_r[k] / want.bin_mass[k], want.phase(2, 2)[k], speed, np.max(rel1[np.isfinite(rel1)])]


def test_runner_cpp_mirror_and_cli(gpu):
    """A cloud in rigid rotation through nb_shell_modes_runner, the runner against its simulator, and headless
    --shells (the C++ mirror) printing what the Python runner returns for the same seeded sphere."""
    nb = gpu
    from wgpu_n_body_amd import _lib
    omega = 0.37
    rng = np.random.default_rng(51)
    x = rng.normal(size=(3000, 3)) * [1.0, 0.7, 0.4]
    n, e1, e2 = S.frame(TILTED)
    cloud = S.make_parts(x, omega * np.cross(n, x), np.ones(len(x)))
    sp = nb.SimParams(particle_num=len(cloud), g=G, e=E, dt=DT)
    runner = nb.OfflineHeadless.new(nb.NaiveSim, sp, None, lambda _p: cloud)
    edges = [0.25, 1.0, 3.0]
    d = runner.shell_modes(edges, lmax=4, rates=True, axis=TILTED, center=(0.0, 0.0, 0.0))
    _check(d, S.shell_ref(runner.read_particles(), edges, 4, TILTED, (0.0, 0.0, 0.0), rates=True))
    assert np.abs(d.pattern_speed(2, 2) - omega).max() < 1e-6 and np.abs(d.pattern_speed(2, 1) - omega).max() < 1e-6
    assert d.relative(2).min() > 0.05  # the cloud is triaxial
    held = nb.Simulator(_lib.lib().nb_runner_sim(runner._h), borrowed=True)
    via_sim = held.shell_modes(edges, lmax=4, rates=True, axis=TILTED, center=(0.0, 0.0, 0.0))
    assert via_sim.coef.tobytes() == d.coef.tobytes() and via_sim.rate.tobytes() == d.rate.tobytes()

    sp = nb.SimParams(particle_num=4096, g=1e-4, e=E, dt=DT)
    sphere = nb.OfflineHeadless.new(nb.TreeSim, sp, nb.AddParams.TreeSimParams(0.75), nb.inits.spherical_init)
    exe = os.path.join(ROOT, "wgpu_n_body_amd", "headless")
    base = [exe, "--sim", "tree", "--n", "4096", "--init", "spherical", "--g", "1e-4", "--steps", "2", "--shells", "2",
            "--shells-range", "0.05,1.5", "--shells-bins", "12", "--shells-l", "3"]
    for extra, kw in (([], dict(center="com")),
                      (["--shells-axis", "0.3,-0.5,0.8", "--shells-center", "0.01,0,-0.02", "--shells-log", "0",
                        "--shells-rates", "1"], dict(axis=TILTED, center=(0.01, 0.0, -0.02), log=False, rates=True))):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        lines = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("shells ")]
        assert [ln[1] for ln in lines] == ["0", "2"]
        want = sphere.shell_modes(nbins=12, rmin=0.05, rmax=1.5, lmax=3, **kw)
        got = np.array([float(x) for x in lines[0][2:]])
        expect = np.array(_cli_expect(want))
        assert np.isfinite(expect[:3]).all() and np.isfinite(expect[3]) == ("rates" in kw)
        assert np.array_equal(got, expect, equal_nan=True), (got, expect)  # %.17g round-trips
    bad = subprocess.run(base[:-6] + ["--shells", "1"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--shells-range" in bad.stderr
