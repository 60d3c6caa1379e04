"""nb_sim_field on the device (csrc/nb_field.hip) against the fp64 restatement of its rule
(tests/field_ref.py) on the read-back state: every component within the derived bounds of include/nbody.h
"Field probes" -- (64 + 16) 2^-24 of g sum m |d_k| / (r^4 + e r) per acceleration component, 5e-6 of
g sum |m| psi(r) for the potential -- every coincident count equal; known answers; chunks and bands;
bitwise reproducibility and permutation; the ties to the step and to the diagnostics; non-finite bodies and
points; that a call does not perturb the trajectory; the refusals; the runner and the CLI.  `-m gpu`."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import field_ref as F
from tests import tidal_ref as T
from tests.diag_ref import psi64
from tests.helpers import DT, E, G, ROOT, bits, make_state

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _sim(nb, kind, state, theta=0.75, **params):
    sp = nb.SimParams(particle_num=state.shape[0], **params)
    if kind == "naive":
        return nb.NaiveSim.from_particles(sp, None, state)
    return nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(theta), state)


def _points(state, m, seed):
    """Half of the points on bodies (the first half, rounded up), half random off-body in the bodies' box."""
    rng = np.random.default_rng(seed)
    on = (m + 1) // 2
    pts = np.empty((m, 3), np.float32)
    pts[:on] = state[rng.integers(0, state.shape[0], size=on), 0:3]
    lo, hi = state[:, 0:3].min(0) - 0.1, state[:, 0:3].max(0) + 0.1
    pts[on:] = rng.uniform(lo, hi, size=(m - on, 3)).astype(np.float32)
    return pts, on


def _check(f, ref, accel=True, potential=True):
    """Within the derived bounds; a field that was not requested is NaN."""
    assert np.array_equal(f.coincident, ref["coincident"]), (f.coincident, ref["coincident"])
    if accel:
        err, lim = np.abs(f.acc - ref["acc"]), F.ACC_BOUND * ref["acc_scale"]
        print("acc: worst error / bound", np.nanmax(np.where(lim > 0, err / np.where(lim > 0, lim, 1), 0), initial=0))
        assert np.all((err <= lim) | np.isnan(ref["acc"])), (err / U, ref["acc_scale"])
        assert np.array_equal(np.isnan(f.acc), np.isnan(ref["acc"]))
    else:
        assert np.isnan(f.acc).all()
    if potential:
        err, lim = np.abs(f.potential - ref["potential"]), F.POT_BOUND * ref["pot_scale"]
        print("potential: worst error / bound", np.nanmax(np.where(lim > 0, err / np.where(lim > 0, lim, 1), 0), initial=0))
        assert np.all((err <= lim) | np.isnan(ref["potential"])), (err, ref["pot_scale"])
        assert np.array_equal(np.isnan(f.potential), np.isnan(ref["potential"]))
    else:
        assert np.isnan(f.potential).all()


# ---- known answers ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_one_body_on_a_ring(gpu, kind):
    nb = gpu
    m, R = 3.0, 0.75
    s = np.zeros((1, 10), np.float32)
    s[0, 0:3], s[0, 9] = (0.25, -0.5, 0.125), m
    sim = _sim(nb, kind, s)
    ring = nb.field_rings([R], axis=(1.0, 2.0, 3.0), center=s[0, 0:3], n_phi=16)
    pts = np.concatenate([ring, s[:, 0:3]])
    f = sim.field(pts)
    sim.destroy()
    g, e = np.float64(np.float32(G)), np.float64(np.float32(E))
    d = s[0, 0:3].astype(np.float64) - ring.astype(np.float64)   # towards the body: acc = -g m R / (R^4 + e R) rhat
    r = np.sqrt((d * d).sum(1))
    acc = g * m * d / (r ** 4 + e * r)[:, None]
    assert np.all(np.abs(f.acc[:16] - acc) <= F.ACC_BOUND * np.abs(acc))
    assert np.all(np.abs(f.potential[:16] + g * m * psi64(r, e)) <= F.POT_BOUND * g * m * psi64(r, e))
    # ... and of the nominal radius, to the rounding of the points (one fp32 ulp of |c| + R moves a^-3 by 3 of them)
    a0 = g * m * R / (R ** 4 + e * R)
    assert np.all(np.abs(np.sqrt((f.acc[:16] ** 2).sum(1)) - a0) <= (F.ACC_BOUND + 8 * U) * a0)
    assert np.all(f.coincident[:16] == 0)
    # a point on the body: zeros, coincident 1
    assert np.all(f.acc[16] == 0) and f.potential[16] == 0 and f.coincident[16] == 1
    assert (f.n, f.nonfinite, f.nonfinite_points, f.step_num) == (1, 0, 0, 0)


def test_midpoint_of_two_equal_bodies(gpu):
    """The two terms cancel: the result is within the bound of 0 -- the bound is relative to the sum of |term|."""
    nb = gpu
    s = np.zeros((2, 10), np.float32)
    s[0, 0:3], s[1, 0:3] = (0.5, 0.25, -0.125), (-0.25, 0.75, 0.375)
    s[:, 9] = 2.0
    mid = ((s[0, 0:3] + s[1, 0:3]) / 2)[None, :]  # exact: dyadic coordinates
    sim = _sim(nb, "naive", s)
    f = sim.field(mid)
    sim.destroy()
    ref = F.field64(s, mid, G, E)
    assert np.all(ref["acc"] == 0) and np.all(ref["acc_scale"] > 0)
    _check(f, ref)


# ---- against fp64 ------------------------------------------------------------------------------
# pairs that cover every N and every M of the issue (M = 1 and M = 1000 at N = 4097: test_chunks_and_bands)
SHAPES = [(1, 2), (2, 1000), (63, 255), (64, 256), (65, 257), (255, 1), (256, 257), (257, 256), (1000, 1000),
          (4097, 255), (4097, 2)]
assert {n for n, _ in SHAPES} == {1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097}
assert {m for _, m in SHAPES} == {1, 2, 255, 256, 257, 1000}
INITS = ["uniform", "disc", "spherical"]


@pytest.mark.parametrize("steps", [0, 3])
@pytest.mark.parametrize("kind", ["naive", "tree"])
@pytest.mark.parametrize("idx", range(len(SHAPES)), ids=[f"n{n}-m{m}" for n, m in SHAPES])
def test_parity_with_the_restatement(gpu, idx, kind, steps):
    nb = gpu
    n, m = SHAPES[idx]
    init = INITS[(idx + steps + (kind == "tree")) % 3]
    sim = _sim(nb, kind, make_state(init, n, seed=40 + idx))
    for _ in range(steps):
        sim.encode()
    state = nb.as_floats(sim.read_particles())
    pts, on = _points(state, m, seed=idx)
    both = sim.field(pts)
    acc = sim.field(pts, potential=False)
    pot = sim.field(pts, accel=False)
    sim.destroy()
    ref = F.field64(state, pts, G, E)
    _check(both, ref)
    assert np.all(both.coincident[:on] >= 1)
    assert (both.step_num, both.n, both.nonfinite, both.nonfinite_points) == (steps, n, 0, 0)
    assert (both.flags, acc.flags, pot.flags) == (3, 1, 2) and both.launches == acc.launches == pot.launches == 1
    assert both.points == acc.points == pot.points == m
    # each flag alone: the other field NaN, the requested one within the bound of the restatement and of the
    # both-flags result
    _check(acc, ref, potential=False)
    _check(pot, ref, accel=False)
    assert np.all(np.abs(acc.acc - both.acc) <= F.ACC_BOUND * ref["acc_scale"])
    assert np.all(np.abs(pot.potential - both.potential) <= F.POT_BOUND * ref["pot_scale"])


# ---- chunks and bands --------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_chunks_and_bands(gpu, kind):
    nb = gpu
    n = 4097
    sim = _sim(nb, kind, make_state("disc", n, seed=3))
    sim.encode()
    state = nb.as_floats(sim.read_particles())
    # one point against 17 body tiles: as many chunks
    one, _ = _points(state, 1, seed=1)
    _check(sim.field(one), F.field64(state, one, G, E))
    # 1000 points in bands of at most 2^16 pairs (one tile of points each): the sums do not change.  With both
    # fields (tiles of 128 points) and with the acceleration alone (tiles of 256)
    pts, _ = _points(state, 1000, seed=2)
    ref = F.field64(state, pts, G, E)
    perm = np.random.default_rng(5).permutation(1000)
    for kw, tiles in ((dict(), 8), (dict(potential=False), 4)):
        a = sim.field(pts, **kw)
        again = sim.field(pts, **kw)
        sim.set_tuning("field_launch_pairs_log2", 16)
        b = sim.field(pts, **kw)
        sim.set_tuning("field_launch_pairs_log2", 35)
        c = sim.field(pts, **kw)
        _check(a, ref, potential=not kw)
        assert a.launches == c.launches == 1 and b.launches == tiles >= 4 and a.points == b.points == 1000
        for x in (again, b, c):  # two calls, and any budget: bit-identical
            assert x.acc.tobytes() == a.acc.tobytes() and x.potential.tobytes() == a.potential.tobytes()
            assert np.array_equal(x.coincident, a.coincident)
        # permuted points give permuted results bit for bit
        p = sim.field(pts[perm], **kw)
        assert p.acc.tobytes() == a.acc[perm].tobytes() and p.potential.tobytes() == a.potential[perm].tobytes()
        assert np.array_equal(p.coincident, a.coincident[perm])
    for bad in (15, 41):
        with pytest.raises(nb.NBodyError):
            sim.set_tuning("field_launch_pairs_log2", bad)
    sim.destroy()


@pytest.mark.parametrize("m,n", [(5, 300_000), (257, 140_000)])
def test_several_tiles_per_chunk(gpu, m, n):
    """The double-buffered loop of a block runs once per tile of its chunk, and a chunk gets a second tile only from
    about 87,000 bodies on: the counterpart of tests/test_tidal_gpu.py's case for the field's instantiations of the
    same loop (csrc/nb_probe.hpp), with the acceleration alone, the potential alone and both.  The flags change the
    points per lane and not the tiles per chunk, two here (asserted from the restated plan).  The prefetch, the
    other buffer and the masked-body count carried from tile to tile: non-finite bodies and bodies at the origin in
    the first, second and last tile of a chunk, and a point at the origin."""
    nb = gpu
    acc_ib = 4 if m >= 256 else 2 if m > 64 else 1     # points_per_lane of csrc/nb_field.hip; 2 with the potential
    assert acc_ib != 2                                 # (so the flags do change the points per lane)
    (_, cj, chunks), (_, cj2, chunks2) = T.plan(m, n, acc_ib), T.plan(m, n, 2)
    assert cj == cj2 == 2 and chunks == chunks2 and (acc_ib, cj, chunks) == T.DEEP[(m, n)]
    state = make_state("uniform", n, seed=70 + cj)
    first, second, last = 256 * cj * 3, 256 * (cj * 3 + 1), 256 * (cj * 4 + cj - 1)  # tiles of chunks 3 and 4
    state[first + 7, 0:3] = 0.0
    state[second + 9, 0:3] = 0.0
    state[first + 100, 4] = np.nan
    state[second + 3, 0] = np.inf
    state[second + 200, 9] = np.nan
    state[last + 255, 2] = np.nan
    state[n - 1, 5] = -np.inf            # (the call's last tile too)
    sim = _sim(nb, "naive", state)
    pts, _ = _points(state[np.isfinite(state).all(1)], m, seed=n % 97)
    pts[0] = 0.0                         # on two bodies and on every masked body's stand-in
    ref = F.field64(state, pts, G, E)
    assert ref["nonfinite"] == 5
    for kw in (dict(potential=False), dict(accel=False), dict()):
        f = sim.field(pts, **kw)
        assert f.nonfinite == 5 and f.coincident[0] == 2 and f.launches == 1, kw
        _check(f, ref, accel=kw.get("accel", True), potential=kw.get("potential", True))
    sim.destroy()


# ---- ties to what exists -----------------------------------------------------------------------
def test_the_step_stores_the_field_times_dt(gpu):
    """(a) From rest with no stored acceleration one all-pairs step leaves the positions where they are and
    stores g dt sum m d / (r^4 + e r), summed in fp32 in some order: within (N + 100) 2^-24 g dt sum |term| of
    field(x).acc dt (N units cover any fp32 summation order; 80 are this rule's own)."""
    nb = gpu
    n = 1000
    s = make_state("uniform", n, seed=12)
    s[:, 3:9] = 0
    sim = _sim(nb, "naive", s)
    sim.encode()
    after = nb.as_floats(sim.read_particles())
    assert np.array_equal(bits(after[:, 0:3]), bits(s[:, 0:3]))
    f = sim.field(s[:, 0:3], potential=False)
    sim.destroy()
    assert np.all(f.coincident == 1) and f.step_num == 1
    dt = np.float64(np.float32(DT))
    ref = F.field64(s, s[:, 0:3], G, E, potential=False)
    err = np.abs(after[:, 6:9].astype(np.float64) - f.acc * dt)
    print("step tie: worst error in units of 2^-24 dt scale", (err / (U * dt * ref["acc_scale"])).max())
    assert np.all(err <= (n + 100) * U * dt * ref["acc_scale"])


@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_the_potentials_sum_to_the_diagnostics(gpu, kind):
    """(b) (dt / 2) sum m_i phi(x_i) is the diagnostics' potential: relative 1e-5, this rule's 5e-6 for phi and
    the same for W, which the diagnostics sum by the same fp32 runs (all masses positive: sum |term| = |sum|)."""
    nb = gpu
    sim = _sim(nb, kind, make_state("spherical", 1000, seed=13))
    sim.encode()
    state = nb.as_floats(sim.read_particles())
    f = sim.field(state[:, 0:3], accel=False)
    d = sim.diagnostics(potential=True)
    sim.destroy()
    assert np.all(f.coincident == 1)
    u = 0.5 * np.float64(np.float32(DT)) * (state[:, 9].astype(np.float64) * f.potential).sum()
    print("potential tie: relative difference", abs(u - d.potential) / abs(d.potential))
    assert abs(u - d.potential) <= 1e-5 * abs(d.potential)


def test_two_sims_same_state(gpu):
    """(c) A TreeSim after a step holds its bodies in tree order; a NaiveSim made from that state shuffled holds
    the same bodies in another order, so the two sum the same terms in different runs: within twice the bound."""
    nb = gpu
    b = _sim(nb, "tree", make_state("disc", 4097, seed=14))
    b.encode()
    state = nb.as_floats(b.read_particles())
    shuffled = state[np.random.default_rng(15).permutation(4097)]
    a = _sim(nb, "naive", shuffled)
    pts, _ = _points(state, 257, seed=3)
    fa, fb = a.field(pts), b.field(pts)
    a.destroy()
    b.destroy()
    ref = F.field64(state, pts, G, E)
    _check(fa, ref)
    _check(fb, ref)
    assert fa.acc.tobytes() != fb.acc.tobytes()  # (another order of summation indeed)
    assert np.all(np.abs(fa.acc - fb.acc) <= 2 * F.ACC_BOUND * ref["acc_scale"])
    assert np.all(np.abs(fa.potential - fb.potential) <= 2 * F.POT_BOUND * ref["pot_scale"])
    assert np.array_equal(fa.coincident, fb.coincident)


# ---- non-finite handling -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_nonfinite_bodies_are_left_out(gpu, kind):
    nb = gpu
    n = 1000  # (not a multiple of the tile: the last tile has absent bodies too)
    state = make_state("uniform", n, seed=4)
    state[7, 0:3] = 0.0                      # a body at the origin, where masked bodies are staged
    state[137, 4] = np.nan
    state[500, 0] = np.inf
    state[901, 9] = -np.inf
    state[902, 2] = np.nan
    sim = _sim(nb, kind, state)
    pts, _ = _points(state[np.isfinite(state).all(1)], 255, seed=6)
    pts[0] = 0.0                             # on body 7 and on every masked body's stand-in
    pts[1] = state[138, 0:3]
    f = sim.field(pts)
    d = sim.diagnostics()
    sim.destroy()
    ref = F.field64(state, pts, G, E)
    assert f.nonfinite == d.nonfinite == ref["nonfinite"] == 4
    assert f.coincident[0] == 1 and np.isfinite(f.acc).all() and np.isfinite(f.potential).all()
    _check(f, ref)


def test_nonfinite_point(gpu):
    nb = gpu
    state = make_state("disc", 1000, seed=5)
    sim = _sim(nb, "naive", state)
    pts, _ = _points(state, 257, seed=7)
    clean = sim.field(pts)
    dirty = pts.copy()
    dirty[3, 1], dirty[100, 0], dirty[256, 2] = np.nan, np.inf, -np.inf
    f = sim.field(dirty)
    only_acc = sim.field(dirty, potential=False)
    sim.destroy()
    bad = np.zeros(257, bool)
    bad[[3, 100, 256]] = True
    assert f.nonfinite_points == 3 and clean.nonfinite_points == 0 and f.nonfinite == 0
    assert np.isnan(f.acc[bad]).all() and np.isnan(f.potential[bad]).all() and np.all(f.coincident[bad] == 0)
    assert np.isnan(only_acc.acc[bad]).all() and np.isnan(only_acc.potential).all()
    # the neighbours are unaffected, bit for bit
    assert f.acc[~bad].tobytes() == clean.acc[~bad].tobytes()
    assert f.potential[~bad].tobytes() == clean.potential[~bad].tobytes()
    assert np.array_equal(f.coincident[~bad], clean.coincident[~bad])
    _check(f, F.field64(state, dirty, G, E))


# ---- other properties --------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_masses_over_six_decades_and_massless_bodies(gpu, kind):
    nb = gpu
    n = 1000
    state = make_state("spherical", n, seed=8)
    rng = np.random.default_rng(9)
    state[:, 9] = (10.0 ** rng.uniform(-3, 3, size=n)).astype(np.float32)
    state[::7, 9] = 0.0
    sim = _sim(nb, kind, state)
    pts, _ = _points(state, 256, seed=10)
    pts[0] = state[7, 0:3]  # on a massless body: coincident all the same
    f = sim.field(pts)
    sim.destroy()
    assert f.coincident[0] == 1
    _check(f, F.field64(state, pts, G, E))


def test_no_softening_and_no_bodies(gpu):
    nb = gpu
    from wgpu_n_body_amd import _lib
    state = make_state("uniform", 257, seed=15)
    sim = _sim(nb, "naive", state, e=0.0)
    pts, on = _points(state, 256, seed=11)
    f = sim.field(pts)
    sim.destroy()
    assert np.isfinite(f.acc).all() and np.isfinite(f.potential).all()   # off-body, and on-body with self left out
    _check(f, F.field64(state, pts, G, 0.0))
    # potential with e < 0 is refused; the acceleration is the step's law for any e
    sim = _sim(nb, "naive", state, e=-1e-4)
    with pytest.raises(nb.NBodyError) as ex:
        sim.field(pts)
    assert ex.value.code == _lib.NB_ERR_INVALID and "e >= 0" in str(ex.value)
    with pytest.raises(nb.NBodyError):
        sim.field(pts, accel=False)
    assert np.isfinite(sim.field(pts[on:], potential=False).acc).all()
    sim.destroy()
    # N = 0 gives zeros; M = 0 is valid
    for kind in ("naive", "tree"):
        sim = _sim(nb, kind, np.zeros((0, 10), np.float32))
        f = sim.field(pts[:5])
        assert np.all(f.acc == 0) and np.all(f.potential == 0) and np.all(f.coincident == 0) and f.n == 0
        assert f.launches == 0
        sim.destroy()
    sim = _sim(nb, "tree", state)
    sim.encode()
    f = sim.field(np.zeros((0, 3), np.float32))
    assert f.acc.shape == (0, 3) and f.potential.shape == (0,) and (f.step_num, f.n, f.launches) == (1, 257, 0)
    sim.destroy()


@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_does_not_perturb_the_trajectory(gpu, kind):
    nb = gpu
    state = make_state("uniform", 4096, seed=9)
    pts, _ = _points(state, 300, seed=12)
    finals = []
    for with_field in (False, True):
        sim = _sim(nb, kind, state)
        for k in range(3):
            sim.encode()
            if with_field:
                f = sim.field(pts, accel=k != 1, potential=k != 2)
                assert f.step_num == k + 1
        finals.append(nb.as_floats(sim.read_particles()).copy())
        sim.destroy()
    assert np.array_equal(finals[0].view(np.uint32), finals[1].view(np.uint32))


def test_refusals_and_the_runner(gpu):
    nb = gpu
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    s = make_state("uniform", 64, seed=1)
    pts = s[:8, 0:3].copy()
    # a sharded simulator (rank 0 of 2)
    sharded = nb.NaiveSim.from_particles(nb.SimParams(particle_num=64), None, s, placement=nb.Placement(world=2))
    with pytest.raises(nb.NBodyError) as ex:
        sharded.field(pts)
    assert ex.value.code == _lib.NB_ERR_UNSUPPORTED and b"sharded" in L.nb_last_error()
    sharded.destroy()
    # a several-GPU runner, both ranks on device 0
    r = nb.OfflineHeadless(nb.NaiveSim, nb.SimParams(particle_num=512), None,
                           lambda p: nb.inits.uniform_init(p, seed=1), device_ids=[0, 0])
    with pytest.raises(nb.NBodyError) as ex:
        r.field(pts)
    assert ex.value.code == _lib.NB_ERR_UNSUPPORTED
    r.destroy()
    # nb_runner_field is nb_sim_field of the runner's simulator
    r = nb.OfflineHeadless(nb.TreeSim, nb.SimParams(particle_num=2048), nb.AddParams.TreeSimParams(0.75),
                           lambda p: nb.inits.disc_init(p, seed=2))
    r.step()
    state = nb.as_floats(r.read_particles())
    pts, _ = _points(state, 100, seed=13)
    a, b = r.field(pts), r.sim.field(pts)
    r.destroy()
    assert a.acc.tobytes() == b.acc.tobytes() and a.potential.tobytes() == b.potential.tobytes()
    assert np.array_equal(a.coincident, b.coincident) and a.step_num == b.step_num == 1
    _check(a, F.field64(state, pts, G, E))


def test_a_tree_steps_status_words_surface(gpu):
    """Twelve bodies on one Morton key: the step completes in bounds and raises a status word, which field()
    reports after its synchronisation as read_particles does."""
    nb = gpu
    n = 2048
    s = make_state("uniform", n, 78)
    s[100:112, 0:3] = s[100, 0:3] + (np.arange(12, dtype=np.float32)[:, None] * np.float32(1e-9))
    sim = _sim(nb, "tree", s, theta=0.5)
    sim.encode()
    with pytest.raises(nb.NBodyError) as ei:
        sim.field(s[:4, 0:3])
    assert "Morton key" in str(ei.value)
    with pytest.raises(nb.NBodyError):
        sim.read_particles()
    sim.destroy()


# ---- the rotation curve ------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [(0.0, 1.0, 0.0), (1.0, 2.0, 3.0)])
def test_circular_velocity_of_one_central_mass(gpu, axis):
    nb = gpu
    m = 150000.0
    s = np.zeros((1, 10), np.float32)
    s[0, 9] = m
    sim = _sim(nb, "naive", s)
    radii = np.linspace(0.125, 2.0, 16)
    cv = sim.circular_velocity(radii, axis=axis, n_phi=8, potential=True)
    sim.destroy()
    g, e = np.float64(np.float32(G)), np.float64(np.float32(E))
    a = g * m * radii / (radii ** 4 + e * radii)
    # one body: every component is within the bound of itself, so the vector is within the bound of its length;
    # and the fp32 rounding of the points: an ulp of R moves a ~ R^-3 by three
    tol = F.ACC_BOUND + 8 * U
    assert np.all(np.abs(cv.a_R + a) <= tol * a) and np.all(np.abs(cv.a_n) <= tol * a)
    assert np.all(np.abs(cv.v_c - np.sqrt(radii * a)) <= tol * np.sqrt(radii * a))  # (half of it, in fact)
    psi = psi64(radii, e)
    assert np.all(np.abs(cv.potential + g * m * psi) <= (F.POT_BOUND + 8 * U) * g * m * psi)
    assert np.array_equal(cv.radii, radii) and cv.field.acc.shape == (128, 3)


def test_cli_rotcurve(gpu):
    """headless --rotcurve (the C++ mirror over nb_runner_field and nb_field_ring_means) prints what the Python
    runner returns, to the printed digits."""
    nb = gpu
    cli = os.path.join(ROOT, "wgpu_n_body_amd", "headless")
    p = subprocess.run([cli, "--sim", "tree", "--n", "2048", "--init", "disc", "--steps", "4", "--rotcurve", "2",
                        "--rotcurve-range", "0.1,1.2", "--rotcurve-bins", "8", "--rotcurve-phi", "12",
                        "--rotcurve-axis", "0,0,1"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    rows = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("rotcurve ")]
    assert len(rows) == 3 * 8 and all(len(r) == 6 for r in rows)
    assert len([ln for ln in p.stdout.splitlines() if ln.startswith("Step Duration: ")]) == 4
    runner = nb.OfflineHeadless(nb.TreeSim, nb.SimParams(particle_num=2048), nb.AddParams.TreeSimParams(0.75),
                                lambda sp: nb.inits.disc_init(sp, seed=0))
    radii = [0.1 + (1.2 - 0.1) * i / 7 for i in range(8)]
    ours = [runner.circular_velocity(radii, axis=(0, 0, 1), n_phi=12)]
    for k in range(4):
        runner.step()
        if (k + 1) % 2 == 0:
            ours.append(runner.circular_velocity(radii, axis=(0, 0, 1), n_phi=12))
    runner.destroy()
    num = re.compile(r"^-?\d\.\d{9}e[+-]\d\d$")
    for j, cv in enumerate(ours):
        for i in range(8):
            row = rows[8 * j + i]
            assert int(row[1]) == cv.field.step_num == 2 * j and all(num.match(x) for x in row[2:]), row
            assert row[2:] == ["%.9e" % v for v in (radii[i], cv.a_R[i], cv.a_n[i], cv.v_c[i])], (row, i, j)
    # the disc's central mass binds it: an inward pull and a rotation curve at every radius
    assert np.all(ours[-1].a_R < 0) and np.all(ours[-1].v_c > 0)
    # without --rotcurve the output has no such line
    p = subprocess.run([cli, "--sim", "naive", "--n", "256", "--steps", "2"], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and "rotcurve" not in p.stdout


def test_large_tree_in_the_gather_range(gpu):
    """2^20 bodies: from 524,288 the walk gathers and the state changes buffer set every step -- the field must
    read the buffer read_particles converts, not a stale one.  64 points against fp64 numpy after two steps."""
    nb = gpu
    n = 1 << 20
    sim = _sim(nb, "tree", make_state("uniform", n, seed=11))
    sim.encode()
    sim.encode()
    state = nb.as_floats(sim.read_particles())
    pts, on = _points(state, 64, seed=14)
    f = sim.field(pts)
    sim.destroy()
    assert (f.step_num, f.n, f.nonfinite) == (2, n, 0) and np.all(f.coincident[:on] == 1)
    _check(f, F.field64(state, pts, G, E))
