"""The all-pairs step (nb_naive.hip) held per body and per pair, on a real MI355X through the C ABI -- `-m gpu`.

tests/test_naive_gpu.py judges the stored acceleration by max|err| / max|acc| <= 2e-5; from a few hundred bodies up
one dropped, doubled or wrongly masked pair stays below that for nearly every body (tests/naive_ref.py has the
table).  Here every body and component is held to the derived bound of tests/naive_ref.py against the binary64 sum
of the same terms:

  (a) probe masses: all masses 0 but P <= 8 probes, so that every row holds exactly P terms under bound(., P) and a
      missing or doubled (body, probe) pair misses the bound by a factor of 3 or more -- over every shipped variant,
      forced and automatic j-splits, mass runs on and off, placed ranks in both step forms, and the one-process
      runner on one device;
  (b) dense states: every body's force under bound(., chain) with the kernel's longest summation chain;
  (c) masses that are all 2.0: mass runs on == off bit for bit over the launch shapes of (a).

Each check of a step has five parts: x' bit-identical to the literal-fp32 oracle; every component of the
acceleration within its bound; v' == kick(kick(v, a_old), a'_gpu) bit for bit, from the GPU's own a'; the mass
carried bit for bit; everything finite.  Each case prints its worst body as a fraction of the bound (`-s`).
"""
import functools

import numpy as np
import pytest

from tests import naive_ref as R
from tests.helpers import DT, E, G, bits

pytestmark = pytest.mark.gpu

N_VARIANTS = 5                       # nb.naive_variants(): a variant added to the table joins the matrix here
JSPLITS = (1, 2, 3, 8, 0)            # naive_jsplit; 0 = the planner's own choice
FORMS = ("encode", "phases")


@functools.lru_cache(maxsize=None)
def oracle_lib():
    from oracle import oracle as O
    O.build()
    return O


@functools.lru_cache(maxsize=None)
def probe_base(name):
    """(base state, x' of the fp32 oracle): a body's new position depends on its own x, v, a only, not on a mass."""
    base = R.probe_base(name)
    return base, oracle_lib().naive_step_f32(base, G, E, DT)[:, 0:3].copy()


@functools.lru_cache(maxsize=None)
def probe_case(name, si):
    """(label, columns, state, terms64 over the probes for all rows), computed once and shared; never modified."""
    base, x_new = probe_base(name)
    label, cols = R.probe_sets(name)[si]
    s = R.probe_state(base, cols, si)
    return label, cols, s, R.terms64(s, x_new, G, E, DT, cols=cols)


def test_the_matrix_covers_every_variant(gpu):
    assert len(gpu.naive_variants()) == N_VARIANTS
    assert {R.waves_of(v) for v in gpu.naive_variants()} == {8, 16}


# ---- one step and its five checks -------------------------------------------------------------------------------

def step(nb, sim, form):
    if form == "encode":
        sim.encode()
    else:
        sim.encode_phase(0)
        sim.encode_phase(1)
    sim.cleanup()
    sim.wait()
    return nb.as_floats(sim.dest_particle_slice()).copy()


def check_step(got, src, x_new, ref, chain, dt, lo=0, hi=None, rows_of_ref=None):
    """The five checks for the bodies [lo, hi) a simulator owns; `ref` has one row per body of [lo, hi) when
    rows_of_ref is None, else rows_of_ref selects them.  Returns the worst fraction of the bound."""
    n = len(src)
    hi = n if hi is None else hi
    own = slice(lo, hi)
    assert got.shape == src.shape and np.isfinite(got).all()
    assert np.array_equal(bits(got[own, 0:3]), bits(x_new[own])), "x' differs from the literal-fp32 oracle"
    assert np.array_equal(bits(got[:, 9]), bits(src[:, 9])), "mass not carried"
    if rows_of_ref is not None:
        ref = {k: v[rows_of_ref] for k, v in ref.items()}
    frac = R.fraction(got[own, 6:9], ref, chain)
    ok = R.within(got[own, 6:9], ref, chain)
    worst = float(frac.max()) if frac.size else 0.0
    assert ok.all(), (f"{int((~ok).sum())} bodies outside the bound, worst {worst:.3g} bounds; first "
                      f"{(lo + np.nonzero(~ok)[0][:8]).tolist()}")
    v_half = R.kick32(src[own, 3:6], src[own, 6:9], dt)
    assert np.array_equal(bits(got[own, 3:6]), bits(R.kick32(v_half, got[own, 6:9], dt))), "v' is not kick(kick(v, a), a')"
    # a placed simulator: the other ranks' bodies keep their positions and have no v, a here
    rest = np.r_[0:lo, hi:n]
    assert not got[rest, 3:9].any() and np.array_equal(bits(got[rest, 0:3]), bits(src[rest, 0:3]))
    return worst


def sims_of(nb, name, variant, placed):
    """[(label, simulator, lo, hi)]: the single simulator, or one per rank of every world of a placed state."""
    state, worlds = probe_base(name)[0], R.PROBE_STATES[name][2]
    n = len(state)
    sp = nb.SimParams(particle_num=n, g=G, e=E, dt=DT)
    out = []
    if not placed:
        out.append(("single", nb.NaiveSim.from_particles(sp, None, state), 0, n))
    else:
        for world in worlds:
            for r in range(world):
                lo, hi = R.rank_range(n, r, world)
                out.append((f"rank {r} of {world}", nb.NaiveSim.from_particles(sp, None, state, nb.Placement(0, r, world)),
                            lo, hi))
    for _label, sim, _lo, _hi in out:
        sim.set_tuning("naive_variant", variant)
    return out


def launch_shapes(sims, placed):
    """(label, sim, lo, hi, form) for every j-split: the simulator is retuned in place."""
    for label, sim, lo, hi in sims:
        for form in (FORMS if placed else FORMS[:1]):
            for js in JSPLITS:
                sim.set_tuning("naive_jsplit", js)
                yield f"{label} {form} jsplit {js}", sim, lo, hi, form


# ---- (a) probe masses ---------------------------------------------------------------------------------------------

def probe_matrix(nb, name, variant, placed):
    sims = sims_of(nb, name, variant, placed)
    x_new = probe_base(name)[1]
    worst, runs = 0.0, 0
    for where, sim, lo, hi, form in launch_shapes(sims, placed):
        for mr in (1, 0):
            sim.set_tuning("naive_mass_runs", mr)
            for si in range(len(R.probe_sets(name))):
                label, cols, s, ref = probe_case(name, si)
                sim.write_particles(s)
                got = step(nb, sim, form)
                try:
                    worst = max(worst, check_step(got, s, x_new, ref, len(cols), DT, lo, hi, slice(lo, hi)))
                except AssertionError as ex:
                    raise AssertionError(f"{name} variant {variant} {where} mass_runs {mr} probes '{label}' "
                                         f"{cols.tolist()}: {ex}") from ex
                runs += 1
    for _l, sim, _lo, _hi in sims:
        sim.destroy()
    print(f"\n    probes {name:13s} variant {variant} {'placed' if placed else 'single'}: {runs} steps, "
          f"worst body {worst:.3f} of bound(P)")


@pytest.mark.parametrize("variant", range(N_VARIANTS))
@pytest.mark.parametrize("name", R.SINGLE_IDS)
def test_probe_masses_single_simulator(gpu, name, variant):
    """257: one i-tile and a tail; 1025: j-split 2 with 8 waves; 2113: 33 tiles + 1 body, j-split 2 with 16 waves;
    4099: j-split up to 4 with 16 waves, up to 8 with 8."""
    probe_matrix(gpu, name, variant, placed=False)


@pytest.mark.parametrize("variant", range(N_VARIANTS))
@pytest.mark.parametrize("name", R.PLACED_IDS)
def test_probe_masses_placed_ranks_in_both_step_forms(gpu, name, variant):
    """Every rank of every world of the state: first, middle, ragged last, and (uniform-300) one without bodies;
    encode() and encode_phase(0), encode_phase(1) -- the windows {lo_tile, local} and {0, rest, skip lo_tile, local}."""
    probe_matrix(gpu, name, variant, placed=True)


@pytest.mark.parametrize("variant", range(N_VARIANTS))
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["uniform-700", "uniform-3000"])
def test_probe_masses_one_process_runner(gpu, monkeypatch, name, world, variant):
    """OfflineHeadless over `world` ranks on device 0: two-phase steps, new slices stored to the peers.  The ranks
    read their variant and j-split from the environment at creation; no key reaches their mass-run switch, so
    this path runs with the default (on) only.  That the environment reached them shows in the bits: every rank's
    bodies equal those of a placed simulator tuned to the same variant and j-split, stepped in two phases."""
    nb = gpu
    base, x_new = probe_base(name)
    n = len(base)
    sp = nb.SimParams(particle_num=n)
    placed = [nb.NaiveSim.from_particles(sp, None, base, nb.Placement(0, r, world)) for r in range(world)]
    for sim in placed:
        sim.set_tuning("naive_variant", variant)
    monkeypatch.setenv("NB_NAIVE_VARIANT", str(variant))
    worst, runs = 0.0, 0
    for js in JSPLITS:
        monkeypatch.setenv("NB_NAIVE_JSPLIT", str(js))
        for sim in placed:
            sim.set_tuning("naive_jsplit", js)
        for si in range(len(R.probe_sets(name))):
            label, cols, s, ref = probe_case(name, si)
            runner = nb.OfflineHeadless(nb.NaiveSim, sp, None, lambda _p: s, device_ids=[0] * world)
            runner.step()
            got = nb.as_floats(runner.read_particles()).copy()
            assert runner.step_num() == 1
            runner.destroy()
            try:
                worst = max(worst, check_step(got, s, x_new, ref, len(cols), DT))
                for r, sim in enumerate(placed):
                    lo, hi = R.rank_range(n, r, world)
                    sim.write_particles(s)
                    assert np.array_equal(bits(step(nb, sim, "phases")[lo:hi]), bits(got[lo:hi])), f"rank {r} differs"
            except AssertionError as ex:
                raise AssertionError(f"{name} runner world {world} variant {variant} jsplit {js} probes '{label}' "
                                     f"{cols.tolist()}: {ex}") from ex
            runs += 1
    for sim in placed:
        sim.destroy()
    print(f"\n    probes {name:13s} variant {variant} runner x{world}: {runs} steps, worst body {worst:.3f} of bound(P)")


# ---- (c) mass runs on == off --------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", range(N_VARIANTS))
@pytest.mark.parametrize("name", R.SINGLE_IDS + R.PLACED_IDS)
def test_mass_runs_on_equals_off_for_masses_of_two(gpu, name, variant):
    """Multiplying by 2 commutes with every rounding: with every mass 2.0 the unweighted sum times the run's mass
    is, bit for bit, the weighted sum -- in every launch shape of (a) but the runner's, whose ranks have no switch."""
    nb = gpu
    placed = name in R.PLACED_IDS
    s = probe_base(name)[0].copy()
    s[:, 9] = 2.0
    sims = sims_of(nb, name, variant, placed)
    runs = 0
    for where, sim, lo, hi, form in launch_shapes(sims, placed):
        out = []
        for mr in (1, 0):
            sim.set_tuning("naive_mass_runs", mr)
            sim.write_particles(s)
            out.append(step(nb, sim, form))
        assert np.isfinite(out[0]).all() and (hi == lo or np.abs(out[0][lo:hi, 6:9]).max() > 0)
        assert np.array_equal(bits(out[0]), bits(out[1])), f"{name} variant {variant} {where}"
        runs += 1
    for _l, sim, _lo, _hi in sims:
        sim.destroy()
    assert runs == len(sims) * len(JSPLITS) * (2 if placed else 1)


# ---- (b) dense states ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", R.DENSE_IDS)
def test_dense_states_every_body_within_the_bound(gpu, oracle, name):
    """Every variant, j-splits {1, 4, auto}; the middle rank of three in both step forms where it owns a body.
    Three of the states take a second step on three of the paths, so that a non-zero a_old reaches the first kick:
    its reference takes the GPU's own state after step 1 as the source."""
    nb = gpu
    s, g, e, dt = R.dense_state(name)
    n = len(s)
    x_new = oracle.naive_step_f32(s, g, e, dt)[:, 0:3].copy()
    ref = R.terms64(s, x_new, g, e, dt)
    variants = nb.naive_variants()
    mid = R.rank_range(n, 1, 3)
    second = {(len(variants) - 1, "single", "encode", 0), (0, "single", "encode", 4),
              (len(variants) - 1, "placed", "phases", 0)} if name in R.TWO_STEPS else set()
    worst, worst2, runs = 0.0, 0.0, 0
    sp = nb.SimParams(particle_num=n, g=g, e=e, dt=dt)
    for v, vname in enumerate(variants):
        chain = R.chain_dense(n, R.waves_of(vname))
        paths = [("single", None, 0, n, "encode")]
        if mid[1] > mid[0]:
            paths += [("placed", nb.Placement(0, 1, 3), mid[0], mid[1], form) for form in FORMS]
        for kind, place, lo, hi, form in paths:
            sim = nb.NaiveSim.from_particles(sp, None, s, place)
            sim.set_tuning("naive_variant", v)
            for js in (1, 4, 0):
                sim.set_tuning("naive_jsplit", js)
                where = f"{name} {vname} {kind} {form} jsplit {js}"
                sim.write_particles(s)
                got = step(nb, sim, form)
                try:
                    worst = max(worst, check_step(got, s, x_new, ref, chain, dt, lo, hi, slice(lo, hi)))
                    if (v, kind, form, js) in second:
                        x2 = oracle.naive_step_f32(got, g, e, dt, lo, hi)[:, 0:3]
                        ref2 = R.terms64(got, x2, g, e, dt, rows=np.arange(lo, hi))
                        assert np.abs(got[lo:hi, 6:9]).max() > 0
                        got2 = step(nb, sim, form)
                        worst2 = max(worst2, check_step(got2, got, x2, ref2, chain, dt, lo, hi))
                except AssertionError as ex:
                    raise AssertionError(f"{where}: {ex}") from ex
                runs += 1
            sim.destroy()
    print(f"\n    dense {name:18s} n={n:5d}: {runs} launch shapes, worst body {worst:.3f} of the bound"
          + (f"; second step {worst2:.3f}" if second else ""))
