"""nb_tidal_sim on the device (csrc/nb_tidal.hip) against the fp64 restatement of its rule (tests/tidal_ref.py):
every component within the derived bound of include/nbody.h "Tidal tensor probes" -- (64 + 33) 2^-24 of g sum |term|
per sum, a diagonal element the bounds of S_aa and W -- every coincident count equal; known answers; bitwise
reproducibility, permutation and bands; non-finite bodies and points; that a call does not perturb the trajectory;
the disc's frequencies; the refusals; the runner and the CLI.  `-m gpu`."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import field_ref as F
from tests import tidal_ref as T
from tests.helpers import E, G, ROOT, make_state

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
WORST = [0.0]  # the worst error / bound any check of this module has seen (printed by each)


def _sim(nb, kind, state, theta=0.75, **params):
    sp = nb.SimParams(particle_num=state.shape[0], **params)
    if kind == "naive":
        return nb.NaiveSim.from_particles(sp, None, state)
    return nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(theta), state)


def _check(t, ref):
    """Every component within its bound of the restatement, the tensor symmetric, every coincident count equal."""
    assert np.array_equal(t.coincident, ref["coincident"]), (t.coincident, ref["coincident"])
    got = t.tensor.reshape(-1, 9)[:, [0, 4, 8, 1, 2, 5]]
    assert np.array_equal(t.tensor, t.tensor.transpose(0, 2, 1), equal_nan=True)
    err, lim = np.abs(got - ref["tensor6"]), ref["bound6"]
    worst = np.nanmax(np.where(lim > 0, err / np.where(lim > 0, lim, 1), 0), initial=0)
    WORST[0] = max(WORST[0], worst)
    print("tidal: worst error / bound", worst, "of the module so far", WORST[0])
    assert np.all((err <= lim) | np.isnan(ref["tensor6"])), (err / U, ref["scales"])
    assert np.array_equal(np.isnan(got), np.isnan(ref["tensor6"]))
    assert np.array_equal(t.trace, t.tensor[:, 0, 0] + t.tensor[:, 1, 1] + t.tensor[:, 2, 2], equal_nan=True)


@functools.lru_cache(maxsize=None)
def _case(idx):
    """(state, points, on, reference) of T.SHAPES[idx], computed once for both simulators."""
    state, pts, on = T.shape_case(idx, E)
    return state, pts, on, T.tidal64(state, pts, G, E)


# ---- against fp64 ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["naive", "tree"])
@pytest.mark.parametrize("idx", range(len(T.SHAPES)), ids=[f"m{m}-n{n}" for m, n in T.SHAPES])
def test_parity_with_the_restatement(gpu, idx, kind):
    nb = gpu
    m, n = T.SHAPES[idx]
    state, pts, on, ref = _case(idx)
    sim = _sim(nb, kind, state)
    t = sim.tidal_tensor(pts)
    again = sim.tidal_tensor(pts)
    sim.destroy()
    _check(t, ref)
    assert np.all(t.coincident[:on] >= 1)
    assert (t.step_num, t.n, t.nonfinite, t.nonfinite_points, t.points) == (0, n, 0, 0, m)
    assert t.launches == (1 if n else 0)
    if n == 0:
        assert np.all(t.tensor == 0) and np.all(t.coincident == 0)
    # two calls: the same bits
    assert again.tensor.tobytes() == t.tensor.tobytes() and np.array_equal(again.coincident, t.coincident)


@pytest.mark.parametrize("m,n", list(T.DEEP), ids=[f"m{m}-n{n}-cj{v[1]}" for (m, n), v in T.DEEP.items()])
def test_several_tiles_per_chunk(gpu, m, n):
    """The double-buffered loop of a block runs once per tile of its chunk, and a chunk gets a second tile only from
    about 87,000 bodies on (T.plan restates the plan; T.DEEP asserts two, three and four tiles per chunk for these
    shapes).  The prefetch, the other buffer and the masked-body count carried from tile to tile: non-finite bodies
    and bodies at the origin in the first, second and last tile of a chunk, and a point at the origin."""
    nb = gpu
    ib, cj, chunks = T.plan(m, n)
    assert cj >= 2 and (ib, cj, chunks) == T.DEEP[(m, n)]
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
    pts, _ = T.points(state[np.isfinite(state).all(1)], m, seed=n % 97, e=E)
    pts[0] = 0.0                         # on two bodies and on every masked body's stand-in
    t = sim.tidal_tensor(pts)
    sim.destroy()
    ref = T.tidal64(state, pts, G, E)
    assert t.nonfinite == ref["nonfinite"] == 5 and t.coincident[0] == 2 and t.launches == 1
    _check(t, ref)


def test_after_steps_a_tree_measures_the_state_it_returns(gpu):
    nb = gpu
    sim = _sim(nb, "tree", make_state("disc", 4099, seed=3))
    for _ in range(3):
        sim.encode()
    state = nb.as_floats(sim.read_particles())
    pts, on = T.points(state, 257, seed=21, e=E)
    t = sim.tidal_tensor(pts)
    empty = sim.tidal_tensor(np.zeros((0, 3), np.float32))
    sim.destroy()
    _check(t, T.tidal64(state, pts, G, E))
    assert t.step_num == 3 and np.all(t.coincident[:on] >= 1)
    # M = 0 only synchronises
    assert empty.tensor.shape == (0, 3, 3) and (empty.step_num, empty.n, empty.launches, empty.points) == (3, 4099, 0, 0)


# ---- known answers -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["naive", "tree"])
@pytest.mark.parametrize("e", [E, 0.0])
def test_one_body_on_a_ring(gpu, kind, e):
    """One body of mass M, a ring of radius R about it.  In closed form from the rule: T rhat = g w (c R^2 - 1) rhat
    and T t = -g w t for t orthogonal to rhat, w = M / (R^4 + e R): stretched along rhat, compressed across."""
    nb = gpu
    M, R = 3.0, 0.75
    s = np.zeros((1, 10), np.float32)
    s[0, 0:3], s[0, 9] = (0.25, -0.5, 0.125), M
    sim = _sim(nb, kind, s, e=e)
    ring = nb.field_rings([R], axis=(1.0, 2.0, 3.0), center=s[0, 0:3], n_phi=16)
    pts = np.concatenate([ring, s[:, 0:3]])
    t = sim.tidal_tensor(pts)
    sim.destroy()
    _check(t, T.tidal64(s, pts, G, e))
    g, e64 = np.float64(np.float32(G)), np.float64(np.float32(e))
    d = s[0, 0:3].astype(np.float64) - ring.astype(np.float64)
    r = np.sqrt((d * d).sum(1))
    w = M / (r ** 4 + e64 * r)
    c = (4 * r ** 3 + e64) / (r ** 2 * (r ** 3 + e64))
    rhat = d / r[:, None]
    want = g * w[:, None, None] * ((c * r * r)[:, None, None] * rhat[:, :, None] * rhat[:, None, :] - np.eye(3))
    # one body: every sum is within the bound of itself; |d_a d_b| <= r^2
    lim = T.BOUND * g * w * (c * r * r + 1)
    assert np.all(np.abs(t.tensor[:16] - want) <= lim[:, None, None])
    # the eigenvalues: one along rhat, g w (c r^2 - 1) > 0 (stretched), and two equal ones -g w (compressed)
    lam, vec = t.eigenvalues(), t.eigenvectors()
    assert np.all(np.abs(lam[:16, 0] - g * w * (c * r * r - 1)) <= 3 * lim) and np.all(np.abs(lam[:16, 1:] + (g * w)[:, None]) <= 3 * lim[:, None])
    assert np.all(np.abs(np.abs((vec[:16, 0] * rhat).sum(1)) - 1) <= 1e-5)
    assert np.array_equal(t.compressive_axes()[:16], np.full(16, 2))
    # a point on the body: zeros, coincident 1
    assert np.all(t.tensor[16] == 0) and t.coincident[16] == 1 and np.all(t.coincident[:16] == 0)
    assert (t.n, t.nonfinite, t.nonfinite_points, t.step_num) == (1, 0, 0, 0)


def test_two_equal_bodies(gpu):
    """At the midpoint of two equal bodies the accelerations cancel, the tensor does not: d -> -d leaves d_a d_b as
    it is, so each sum is twice one body's.  What cancels in the tensor is a mirror pair: bodies at p + (a, b, c)
    and p + (a, -b, c) give xy and yz terms of opposite sign, which must lie within the bound of 0 -- the bound is
    relative to the sum of |term|."""
    nb = gpu
    s = np.zeros((2, 10), np.float32)
    s[0, 0:3], s[1, 0:3] = (0.5, 0.25, -0.125), (-0.25, 0.75, 0.375)
    s[:, 9] = 2.0
    mid = ((s[0, 0:3] + s[1, 0:3]) / 2)[None, :]  # exact: dyadic coordinates
    mirror = np.array([[0.5 - 0.375, 0.5, -0.125 + 0.25]], np.float32)  # p = x_0 - (a, b, c), (a, b, c) = (.375, -.25, -.25)
    s2 = s.copy()
    s2[1, 0:3] = (0.5, 0.75, -0.125)  # = p + (a, -b, c)
    for state, p in ((s, mid), (s2, mirror)):
        sim = _sim(nb, "naive", state)
        t = sim.tidal_tensor(p)
        f = sim.field(p, potential=False)
        sim.destroy()
        ref = T.tidal64(state, p, G, E)
        _check(t, ref)
        if p is mid:
            assert np.all(f.acc == 0) or np.all(np.abs(f.acc) <= F.ACC_BOUND * F.field64(state, p, G, E)["acc_scale"])
            one = T.tidal64(state[:1], p, G, E)
            assert np.allclose(ref["sums"], 2 * one["sums"], rtol=1e-14, atol=0)
        else:
            assert ref["tensor6"][0, 3] == 0 and ref["tensor6"][0, 5] == 0 and ref["scales"][0, 3] > 0
            assert abs(t.tensor[0, 0, 1]) <= ref["bound6"][0, 3] and abs(t.tensor[0, 1, 2]) <= ref["bound6"][0, 5]
            assert abs(t.tensor[0, 0, 2]) > 1000 * ref["bound6"][0, 4]  # (xz does not cancel)


# ---- reproducibility ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_bands_permutations_and_places(gpu, kind):
    nb = gpu
    idx = T.SHAPES.index((600, 1000))
    state, pts, _, ref = _case(idx)
    sim = _sim(nb, kind, state)
    a = sim.tidal_tensor(pts)
    sim.set_tuning("field_launch_pairs_log2", 16)   # tiles of 256 points, 256,000 pairs each: three bands
    b = sim.tidal_tensor(pts)
    sim.set_tuning("field_launch_pairs_log2", 35)
    c = sim.tidal_tensor(pts)
    assert (a.launches, b.launches, c.launches) == (1, 3, 1)
    for x in (b, c):
        assert x.tensor.tobytes() == a.tensor.tobytes() and np.array_equal(x.coincident, a.coincident)
    # permuted points give permuted samples bit for bit
    perm = np.random.default_rng(5).permutation(600)
    p = sim.tidal_tensor(pts[perm])
    assert p.tensor.tobytes() == a.tensor[perm].tobytes() and np.array_equal(p.coincident, a.coincident[perm])
    # a point's sample does not depend on its place in a 600-point call, nor on the other points of it
    other, _ = T.points(state, 600, seed=99, e=E)
    for src, place in ((7, 0), (450, 255), (451, 256), (599, 3), (0, 599)):
        q = other.copy()
        q[place] = pts[src]
        x = sim.tidal_tensor(q)
        assert x.tensor[place].tobytes() == a.tensor[src].tobytes() and x.coincident[place] == a.coincident[src]
    sim.destroy()
    _check(a, ref)


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
    pts, _ = T.points(state[np.isfinite(state).all(1)], 255, seed=6, e=E)
    pts[0] = 0.0                             # on body 7 and on every masked body's stand-in
    pts[1] = state[138, 0:3]
    t = sim.tidal_tensor(pts)
    d = sim.diagnostics()
    sim.destroy()
    ref = T.tidal64(state, pts, G, E)
    assert t.nonfinite == d.nonfinite == ref["nonfinite"] == 4
    assert t.coincident[0] == 1 and np.isfinite(t.tensor).all()
    _check(t, ref)


def test_nonfinite_point(gpu):
    nb = gpu
    state = make_state("disc", 1000, seed=5)
    sim = _sim(nb, "naive", state)
    pts, _ = T.points(state, 257, seed=7, e=E)
    clean = sim.tidal_tensor(pts)
    dirty = pts.copy()
    dirty[3, 1], dirty[100, 0], dirty[256, 2] = np.nan, np.inf, -np.inf
    t = sim.tidal_tensor(dirty)
    sim.destroy()
    bad = np.zeros(257, bool)
    bad[[3, 100, 256]] = True
    assert t.nonfinite_points == 3 and clean.nonfinite_points == 0 and t.nonfinite == 0
    assert np.isnan(t.tensor[bad]).all() and np.all(t.coincident[bad] == 0)
    assert np.isnan(t.eigenvalues()[bad]).all() and np.all(t.compressive_axes()[bad] == -1)
    # the neighbours are unaffected, bit for bit
    assert t.tensor[~bad].tobytes() == clean.tensor[~bad].tobytes()
    assert np.array_equal(t.coincident[~bad], clean.coincident[~bad])
    _check(t, T.tidal64(state, dirty, G, E))


# ---- state -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["naive", "tree"])
def test_does_not_perturb_the_trajectory(gpu, kind):
    nb = gpu
    state = make_state("uniform", 4096, seed=9)
    pts, _ = T.points(state, 300, seed=12, e=E)
    finals = []
    for with_call in (False, True):
        sim = _sim(nb, kind, state)
        for k in range(3):
            sim.encode()
            if with_call:
                assert sim.tidal_tensor(pts).step_num == k + 1
        finals.append(nb.as_floats(sim.read_particles()).copy())
        sim.destroy()
    assert np.array_equal(finals[0].view(np.uint32), finals[1].view(np.uint32))


def test_a_tree_steps_status_words_surface(gpu):
    """Twelve bodies on one Morton key: the step completes in bounds and raises a status word, which
    tidal_tensor() reports after its synchronisation as field() and read_particles do."""
    nb = gpu
    n = 2048
    s = make_state("uniform", n, 78)
    s[100:112, 0:3] = s[100, 0:3] + (np.arange(12, dtype=np.float32)[:, None] * np.float32(1e-9))
    sim = _sim(nb, "tree", s, theta=0.5)
    sim.encode()
    with pytest.raises(nb.NBodyError) as ei:
        sim.tidal_tensor(s[:4, 0:3])
    assert "Morton key" in str(ei.value)
    sim.destroy()


# ---- the disc's frequencies --------------------------------------------------------------------
@pytest.mark.parametrize("axis", [(0.0, 1.0, 0.0), (1.0, 2.0, 3.0)])
def test_frequencies_of_one_central_mass(gpu, axis):
    nb = gpu
    M = 150000.0
    s = np.zeros((1, 10), np.float32)
    s[0, 9] = M
    radii = np.linspace(0.125, 2.0, 16)
    g = np.float64(np.float32(G))
    for e in (E, 0.0):
        sim = _sim(nb, "naive", s, e=e)
        d = sim.disc_frequencies(radii, axis=axis, n_phi=8)
        sim.destroy()
        e64 = np.float64(np.float32(e))
        om2 = g * M / (radii * (radii ** 3 + e64))
        ka2 = 3.0 * e64 * g * M / (radii * (radii ** 3 + e64) ** 2)
        # one body: every sum is within the bound of itself, and any projection u . T v of the tensor within the bound
        # of sum |u_a v_b| scale_ab <= g w (c R^2 + 1) <= 5 Omega^2 (c R^2 <= 4, g w = Omega^2); and the fp32 rounding
        # of the points: an ulp of R moves R^-4 by four, of a tensor of at most 3 Omega^2
        lim_t = (T.BOUND * 5 + 8 * U * 3) * om2
        lim_a = (F.ACC_BOUND + 8 * U) * om2
        lim_k = lim_t + 3 * lim_a
        assert np.all(np.abs(d.omega2 - om2) <= lim_a)
        assert np.all(np.abs(d.nu2 - om2) <= lim_t) and np.all(np.abs(d.t_pp + om2) <= lim_t)
        assert np.all(np.abs(d.kappa2 - ka2) <= lim_k) and np.all(np.abs(d.t_Rn) <= lim_t)
        assert np.array_equal(d.omega, np.sqrt(d.omega2)) and np.array_equal(d.nu, np.sqrt(d.nu2))
        assert np.array_equal(d.v_c, d.rings.v_c) and np.array_equal(d.radii, radii)
        assert d.tidal.tensor.shape == (128, 3, 3)
        if e:
            sure = ka2 > 2 * lim_k  # (at R = 2, kappa^2 = 4e-5 Omega^2 is below what fp32 pair terms resolve)
            assert sure.sum() >= 8 and np.all(d.kappa[sure] > 0)
            # Omega - kappa / 2 rises outwards here, Omega falls: a pattern between the two has both resonances
            res = d.resonances(float(np.sqrt(om2[8])), m=2)
            assert len(res["corotation"]) == 1 and abs(res["corotation"][0] - radii[8]) <= radii[1] - radii[0]


def test_frequencies_of_a_disc_and_the_runner(gpu):
    """A disc_init disc of 4,096 bodies: finite Omega and kappa at every ring, and kappa <= 2 Omega up to the
    bounds of the sums behind them -- kappa^2 - 4 Omega^2 = R dOmega^2/dR, and Omega falls outwards.  The runner's
    entry point is the simulator's.
    The softening is e = 0.05 here.  Under the 1 / r^3 law the central mass alone has kappa^2 / Omega^2 =
    3 e / (R^3 + e), which at the default e = 1e-4 is 0.0024 at R = 0.5 -- marginally stable -- so there the sign of
    kappa^2 is decided by the 4,095 unit masses (2.7 % of the mass, a smooth kappa^2 / Omega^2 of about 0.03 R) and
    by their graininess (one body 0.05 away adds 3e5 g to T_RR beside kappa^2 = 3e4 g), and kappa is not defined at
    every ring: the binary64 restatement has kappa^2 < 0 at 4 of these 12 rings.  With e = 0.05 the central mass
    gives 0.08 (R = 1.2) to 2.9 (R = 0.1) Omega^2, a body adds at most 1.25 e^(-4/3) g = 68 g, and kappa is finite
    and below 2 Omega."""
    nb = gpu
    e = 0.05
    r = nb.OfflineHeadless(nb.TreeSim, nb.SimParams(particle_num=4096, e=e), nb.AddParams.TreeSimParams(0.75),
                           lambda p: nb.inits.disc_init(p, seed=2))
    r.step()
    state = nb.as_floats(r.read_particles())
    radii = np.linspace(0.1, 1.2, 12)
    axis = (0.0, 0.0, 1.0)
    a, b = r.disc_frequencies(radii, axis=axis, n_phi=12), r.sim.disc_frequencies(radii, axis=axis, n_phi=12)
    pts = nb.field_rings(radii, axis=axis, n_phi=12)
    ta, tb = r.tidal_tensor(pts), r.sim.tidal_tensor(pts)
    r.destroy()
    for k in ("omega2", "kappa2", "nu2", "t_RR", "t_pp", "t_nn", "t_Rn", "v_c"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
    assert ta.tensor.tobytes() == tb.tensor.tobytes() == a.tidal.tensor.tobytes() and ta.step_num == tb.step_num == 1
    ref = T.tidal64(state, pts, G, e)
    _check(ta, ref)
    assert np.isfinite(a.omega).all() and np.isfinite(a.kappa).all() and np.all(a.omega > 0) and np.all(a.kappa > 0)
    # |rhat_a rhat_b| <= 1: the bound of T_RR is at most the sum of the nine components', the mean over a ring no more
    # than the worst of it; Omega^2 = -a_R / R carries the field's bound
    t_bound = (ref["bound6"][:, :3].sum(1) + 2 * ref["bound6"][:, 3:].sum(1)).reshape(12, 12).max(1)
    a_bound = (F.ACC_BOUND * F.field64(state, pts, G, e, potential=False)["acc_scale"].sum(1)).reshape(12, 12).max(1)
    slack = t_bound + 3 * a_bound / radii
    print("kappa^2 / (4 Omega^2):", a.kappa2 / (4 * a.omega2))
    print("slack / Omega^2:", slack / a.omega2)
    assert np.all(a.kappa2 <= 4 * a.omega2 + slack)


def test_cli_freq(gpu):
    """headless --freq (the C++ mirror over nb_runner_field, nb_tidal_runner and the two ring means) prints what the
    Python runner returns, to the printed digits."""
    nb = gpu
    cli = os.path.join(ROOT, "wgpu_n_body_amd", "headless")
    p = subprocess.run([cli, "--sim", "tree", "--n", "2048", "--init", "disc", "--steps", "2", "--freq", "2",
                        "--freq-range", "0.1,1.2", "--freq-bins", "8", "--freq-phi", "12", "--freq-axis", "0,0,1"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    rows = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("freq ")]
    assert len(rows) == 2 * 8 and all(len(r) == 7 for r in rows)
    assert len([ln for ln in p.stdout.splitlines() if ln.startswith("Step Duration: ")]) == 2
    runner = nb.OfflineHeadless(nb.TreeSim, nb.SimParams(particle_num=2048), nb.AddParams.TreeSimParams(0.75),
                                lambda sp: nb.inits.disc_init(sp, seed=0))
    radii = [0.1 + (1.2 - 0.1) * i / 7 for i in range(8)]
    ours = [runner.disc_frequencies(radii, axis=(0, 0, 1), n_phi=12)]
    runner.step()
    runner.step()
    ours.append(runner.disc_frequencies(radii, axis=(0, 0, 1), n_phi=12))
    runner.destroy()
    num = re.compile(r"^(-?\d\.\d{9}e[+-]\d\d|nan)$")
    for j, d in enumerate(ours):
        for i in range(8):
            row = rows[8 * j + i]
            assert int(row[1]) == d.tidal.step_num == 2 * j and all(num.match(x) for x in row[2:]), row
            assert row[2:] == ["%.9e" % v for v in (radii[i], d.omega[i], d.kappa[i], d.nu[i], d.v_c[i])], (row, i, j)
    assert np.all(ours[-1].omega > 0)
    # without --freq the output has no such line; without a range it is refused
    p = subprocess.run([cli, "--sim", "naive", "--n", "256", "--steps", "1"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "freq" not in p.stdout
    p = subprocess.run([cli, "--sim", "naive", "--n", "256", "--steps", "1", "--freq", "1"], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 2 and "--freq-range" in p.stderr


# ---- refusals ----------------------------------------------------------------------------------
def test_refusals(gpu):
    nb = gpu
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    s = make_state("uniform", 64, seed=1)
    pts = s[:8, 0:3].copy()
    # a sharded simulator (rank 0 of 2)
    sharded = nb.NaiveSim.from_particles(nb.SimParams(particle_num=64), None, s, placement=nb.Placement(world=2))
    for call in (lambda: sharded.tidal_tensor(pts), lambda: sharded.disc_frequencies([0.5])):
        with pytest.raises(nb.NBodyError) as ex:
            call()
        assert ex.value.code == _lib.NB_ERR_UNSUPPORTED and b"sharded" in L.nb_last_error()
    sharded.destroy()
    # a several-GPU runner, both ranks on device 0
    r = nb.OfflineHeadless(nb.NaiveSim, nb.SimParams(particle_num=512), None,
                           lambda p: nb.inits.uniform_init(p, seed=1), device_ids=[0, 0])
    for call in (lambda: r.tidal_tensor(pts), lambda: r.disc_frequencies([0.5])):
        with pytest.raises(nb.NBodyError) as ex:
            call()
        assert ex.value.code == _lib.NB_ERR_UNSUPPORTED
    r.destroy()
    # a live handle does not excuse the arguments
    sim = _sim(nb, "naive", s)
    st = _lib.nb_tidal_stats()
    out = np.zeros(8, _lib.TIDAL_SAMPLE_DTYPE)
    assert L.nb_tidal_sim(sim._h, None, 8, out.ctypes.data, C.byref(st)) == _lib.NB_ERR_INVALID
    assert L.nb_tidal_sim(sim._h, pts.ctypes.data, (1 << 24) + 1, out.ctypes.data, None) == _lib.NB_ERR_INVALID
    assert L.nb_tidal_sim(sim._h, pts.ctypes.data, 8, out.ctypes.data, None) == _lib.NB_OK  # stats may be null
    sim.destroy()
