"""Runs of equal masses in the all-pairs kernel (nb_naive.hip), on a real MI355X -- `-m gpu`.

With the tuning key `naive_mass_runs` = 1 (the default) a wave sums d / (r^4 + e r) without the
per-pair mass multiply for as long as the j tiles it reads hold one mass, and multiplies its sums by
that mass once.  `naive_mass_runs` = 0 multiplies every pair, which is the arithmetic the kernel
had before, and serves here as the reference inside the same build.

What must hold:
  * masses that are all the same power of two: multiplying by it commutes with every rounding of
    the sum, so both modes give the same bits, for every kernel variant and every tail shape;
  * any other equal mass: only the rounding of the sum changes -- the oracle tolerances of
    tests/test_naive_gpu.py apply unchanged, and the result is deterministic;
  * a run that breaks (one odd body anywhere, or two halves of different mass): every wave that
    meets the break goes on with the weighted body -- oracle tolerances, in both modes.
Every case runs 2 steps.
"""
import numpy as np
import pytest

from tests.helpers import DT, E, G, bits, make_state
from tests.test_naive_gpu import (check_against_oracles, run_gpu,
                                  test_sharded_ranks_reproduce_the_single_simulator as sharded_ranks_case)

pytestmark = pytest.mark.gpu

STEPS = 2


def mode(nb, mass_runs):
    """A stand-in for nb.NaiveSim that run_gpu() accepts as `cls`: the simulator with the key set."""
    class Sim:
        @staticmethod
        def from_particles(sp, add, state):
            sim = nb.NaiveSim.from_particles(sp, add, state)
            sim.set_tuning("naive_mass_runs", mass_runs)
            return sim
    return Sim


def state_with_masses(n, seed, masses):
    s = make_state("uniform", n, seed)
    s[:, 9] = masses
    return s


def oracles(oracle, s, g=G, dt=DT):
    return oracle.naive_run_f32(s, g, E, dt, STEPS), oracle.naive_run_f64(s, g, E, dt, STEPS)


@pytest.mark.parametrize("mass", [1.0, 0.5, 4.0])
def test_power_of_two_masses_give_the_same_bits_in_every_variant(gpu, mass):
    s = state_with_masses(1337, 11, mass)
    for v, name in enumerate(gpu.naive_variants()):
        on = run_gpu(gpu, s, STEPS, variant=v, cls=mode(gpu, 1))
        off = run_gpu(gpu, s, STEPS, variant=v, cls=mode(gpu, 0))
        assert np.isfinite(on).all() and np.abs(on[:, 6:9]).max() > 0
        assert np.array_equal(bits(on), bits(off)), name


@pytest.mark.parametrize("n", [1337, 5000])
def test_equal_mass_that_is_no_power_of_two(gpu, oracle, n):
    s = state_with_masses(n, 12, 1.3)
    ref32, ref64 = oracles(oracle, s)
    out = run_gpu(gpu, s, STEPS, cls=mode(gpu, 1))
    check_against_oracles(out, ref32, ref64, STEPS)
    again = run_gpu(gpu, s, STEPS, cls=mode(gpu, 1))
    assert np.array_equal(bits(out), bits(again))


def _both_modes_against_oracles(gpu, oracle, s, **kw):
    ref32, ref64 = oracles(oracle, s)
    for m in (1, 0):
        out = run_gpu(gpu, s, STEPS, cls=mode(gpu, m), **kw)
        try:
            check_against_oracles(out, ref32, ref64, STEPS)
        except AssertionError as ex:
            raise AssertionError(f"naive_mass_runs={m}: {ex}") from ex


@pytest.mark.parametrize("k", [0, 63, 64, 2500, 4999])
def test_one_odd_body_breaks_the_run(gpu, oracle, k):
    """79 j tiles over the 16 waves of the default variant: about 5 tiles per wave, and the wave that owns
    tile k // 64 leaves its run there (at its first tile for k < 64)."""
    m = np.ones(5000, np.float32)
    m[k] = 7.5
    _both_modes_against_oracles(gpu, oracle, state_with_masses(5000, 13, m), jsplit=1)


def test_two_halves_of_different_mass_break_every_waves_run(gpu, oracle):
    m = np.where(np.arange(5000) < 3072, 1.0, 3.0).astype(np.float32)   # tile 48 on is the heavier half
    _both_modes_against_oracles(gpu, oracle, state_with_masses(5000, 14, m), jsplit=1)


def test_disc_init_heavy_body_zero(gpu, oracle):
    g, dt = 0.00001, 0.0016
    s = make_state("disc", 1024, 15, g)
    assert s[0, 9] != s[1, 9] and (s[1:, 9] == s[1, 9]).all()
    ref32, ref64 = oracles(oracle, s, g, dt)
    check_against_oracles(run_gpu(gpu, s, STEPS, g=g, dt=dt, cls=mode(gpu, 1)), ref32, ref64, STEPS)


@pytest.mark.parametrize("n", [64, 65, 256, 257, 4096, 4097])
def test_ragged_and_aligned_tails(gpu, n):
    """n % 64 == 0: the last tile has no padding and runs the unmasked body; otherwise the masked one."""
    s = state_with_masses(n, 16, 2.0)
    on = run_gpu(gpu, s, STEPS, cls=mode(gpu, 1))
    off = run_gpu(gpu, s, STEPS, cls=mode(gpu, 0))
    assert np.isfinite(on).all() and np.abs(on[:, 6:9]).max() > 0
    assert np.array_equal(bits(on), bits(off))


@pytest.mark.parametrize("n,variant,jsplit", [(4096, 3, 4), (5000, 1, 3)])
def test_j_split_partial_sums_are_weighted(gpu, oracle, n, variant, jsplit):
    s = state_with_masses(n, 17, 1.3)
    ref32, ref64 = oracles(oracle, s)
    out = run_gpu(gpu, s, STEPS, variant=variant, jsplit=jsplit, cls=mode(gpu, 1))
    check_against_oracles(out, ref32, ref64, STEPS)


def test_sharded_ranks_of_unit_masses_reproduce_the_single_simulator(gpu):
    """Body-range sharding (a rank's i range starts mid-tile, its j tiles are everybody's): bitwise the
    single simulator's step.  The construction's uniform_init has every mass 1."""
    init = gpu.inits.uniform_init(gpu.SimParams(particle_num=1000), seed=9)
    assert (gpu.as_floats(init)[:, 9] == 1.0).all()
    sharded_ranks_case(gpu, 1000, 2, 1)


def test_all_masses_zero(gpu, oracle):
    s = state_with_masses(300, 18, 0.0)
    ref32, _ = oracles(oracle, s)
    out = run_gpu(gpu, s, STEPS, cls=mode(gpu, 1))
    assert (out[:, 6:9] == 0.0).all()
    assert np.array_equal(bits(out[:, 0:3]), bits(ref32[:, 0:3]))   # pure drift: exact in fp32


def test_coincident_bodies_are_nan_in_the_same_places(gpu):
    c = np.zeros((3, 10), np.float32)
    c[2, 0] = 1.0
    c[:, 9] = 1.0
    on = run_gpu(gpu, c, STEPS, cls=mode(gpu, 1))
    off = run_gpu(gpu, c, STEPS, cls=mode(gpu, 0))
    assert np.isnan(on[0, 6:9]).any() and np.isnan(on[1, 6:9]).any()
    assert np.array_equal(np.isnan(on), np.isnan(off))


def test_the_key_takes_0_or_1_only(gpu):
    sim = gpu.NaiveSim.from_particles(gpu.SimParams(particle_num=2), None, np.zeros((2, 10), np.float32))
    with pytest.raises(gpu.NBodyError):
        sim.set_tuning("naive_mass_runs", 2)
    sim.set_tuning("naive_mass_runs", 0)
    sim.set_tuning("naive_mass_runs", 1)
    sim.destroy()
