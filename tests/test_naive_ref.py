"""tests/naive_ref.py against the CPU oracles, on the states the GPU tests use -- `-m "not gpu"`.

What this pins is the REFERENCE and the INPUTS: that terms64 is the sum oracle.naive_step_f64 computes, that the
literal-fp32 oracle (a sequential sum of n terms) sits within bound(., n) of it per component, that in every probe
state nearly every (body, probe) pair is strong enough for a dropped or doubled pair to break the bound, and that
the criterion the GPU tests apply really fails every such body.
"""
import functools

import numpy as np
import pytest

from tests import naive_ref as R

OLD_TOL = 2e-5      # tests/test_naive_gpu.py's ACC_TOL, of max |acc|


@functools.lru_cache(maxsize=None)
def dense(name):
    """(state, g, e, dt, fp32 oracle step, terms64 from its positions), computed once and shared; never modified."""
    from oracle import oracle as O
    O.build()
    s, g, e, dt = R.dense_state(name)
    ref32 = O.naive_step_f32(s, g, e, dt)
    return s, g, e, dt, ref32, R.terms64(s, ref32[:, 0:3], g, e, dt)


@functools.lru_cache(maxsize=None)
def probe(name):
    """(base state, the fp32 oracle's new positions) of a probe state.  x' depends on a body's own x, v, a only."""
    from oracle import oracle as O
    O.build()
    base = R.probe_base(name)
    return base, O.naive_step_f32(base, R.G, R.E, R.DT)[:, 0:3]


@pytest.mark.parametrize("name", R.CPU_IDS)
def test_terms64_is_the_binary64_oracles_sum(nb, oracle, name):
    s, g, e, dt, _ref32, _t = dense(name)
    ref64 = oracle.naive_step_f64(s.astype(np.float64), g, e, dt)
    t = R.terms64(s.astype(np.float64), ref64[:, 0:3], g, e, dt, x64=True)
    scale = np.abs(ref64[:, 6:9]).max()
    assert np.isfinite(t["acc"]).all() and scale > 0.0
    assert np.abs(t["acc"] - ref64[:, 6:9]).max() <= 1e-12 * scale
    assert (t["sum_abs"] >= np.abs(t["acc"])).all()
    # columns and rows select: a subset of the columns plus the rest is the whole, on a subset of the rows
    n = len(s)
    rows = np.arange(0, n, 3)
    a = R.terms64(s, dense(name)[4][:, 0:3], g, e, dt, cols=np.arange(0, n, 2), rows=rows)
    b = R.terms64(s, dense(name)[4][:, 0:3], g, e, dt, cols=np.arange(1, n, 2), rows=rows)
    whole = dense(name)[5]
    assert np.abs(a["acc"] + b["acc"] - whole["acc"][rows]).max() <= 1e-12 * scale
    assert np.array_equal(np.minimum(a["min_term"], b["min_term"]), whole["min_term"][rows])


def test_the_fp32_oracle_is_within_the_bound_and_the_old_norm_is_blind(nb, oracle):
    """Per component, chain = n (the oracle adds j in order).  Printed with `-s`: the table of naive_ref.py."""
    lines = []
    for name in R.CPU_IDS:
        s, _g, _e, _dt, ref32, t = dense(name)
        n = len(s)
        frac = R.fraction(ref32[:, 6:9], t, n)
        assert np.isfinite(ref32).all() and R.within(ref32[:, 6:9], t, n).all(), (name, frac.max())
        assert np.array_equal(ref32[:, 9], s[:, 9])
        body = frac.max(axis=1)
        blind = (t["min_term"] < OLD_TOL * np.abs(t["acc"]).max()).mean()
        typical = np.median(t["sum_abs"].sum(axis=1) / max(n - 1, 1)) / np.abs(t["acc"]).max()
        lines.append(f"    {name:16s} {100.0 * blind:5.1f} %   typical term / max|acc| {typical:8.1e}   "
                     f"oracle fp32: worst {body.max():.3f}, median {np.median(body):.3f} of bound(n)")
        if n >= 1337:    # why the per-pair tests exist: nearly every body has a pair the max norm cannot see
            assert blind > 0.99, (name, blind)
    print("\n" + "\n".join(lines))


@pytest.mark.parametrize("name", list(R.PROBE_STATES))
def test_probe_states_have_the_power_and_the_criterion_bites(nb, oracle, name):
    """A condition on the inputs (the seeds are chosen so that it holds): per probe set at most 1 % of the bodies
    have a (body, probe) pair that is not strong.  Then the mutation check, with the GPU test's own criterion
    (naive_ref.within): the sum with one probe column dropped, and with one doubled, rounded to fp32 as a kernel
    would store it, fails for every body that is counted; the unmutated sum passes for all."""
    base, x_new = probe(name)
    n = len(base)
    worst_share, weakest = 0.0, np.inf
    for si, (label, cols) in enumerate(R.probe_sets(name)):
        masses = R.probe_state(base, cols, si)[cols, 9]
        assert len(cols) <= 8 and len(set(cols.tolist())) == len(cols)
        assert len(set(masses.tolist())) == len(cols) and ((masses >= 0.5) & (masses < 2.0)).all()
        assert (np.frexp(masses)[0] != 0.5).all(), "no probe mass is a power of two"
        s = R.probe_state(base, cols, si)
        ref, each = R.probe_terms(s, x_new, R.G, R.E, R.DT, cols)
        assert np.abs(each.sum(axis=0) - ref["acc"]).max() <= 1e-12 * np.abs(ref["acc"]).max()
        strong = R.strong_pairs(ref, each, cols)
        counted = strong.all(axis=1)
        share = 1.0 - counted.mean()
        worst_share = max(worst_share, share)
        b = R.bound(ref["sum_abs"], len(cols))
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(b[None] > 0, np.abs(each) / b[None], 0.0).max(axis=2).T    # [rows, P]
        ratio[np.arange(n)[:, None] == cols[None, :]] = np.inf
        weakest = min(weakest, float(ratio.min()))
        assert share <= R.MAX_LEFT_OUT, (name, label, share)
        exact = ref["acc"].astype(np.float32)
        assert R.within(exact, ref, len(cols)).all()
        for p in range(len(cols)):
            hit = counted & (np.arange(n) != cols[p])     # (a probe has no pair with itself to lose)
            for sign in (-1.0, +1.0):                     # dropped, doubled
                mutated = (ref["acc"] + sign * each[p]).astype(np.float32)
                ok = R.within(mutated, ref, len(cols))
                assert not ok[hit].any(), (name, label, int(cols[p]), sign, np.nonzero(ok & hit)[0][:5])
    print(f"\n    {name:14s} bodies left out, worst set {100.0 * worst_share:5.2f} %; weakest pair {weakest:9.1f} bounds")


def test_chain_and_rank_range_restate_the_product(nb):
    assert R.chain_dense(4099, 16) == 64 * 5 + 16 + 32 and R.chain_dense(4099, 8) == 64 * 9 + 8 + 32
    assert R.chain_dense(2, 8) == 64 + 8 + 32
    assert [R.waves_of(v) for v in nb.naive_variants()] == [8, 8, 16, 16, 16]
    for n, world in [(300, 3), (700, 3), (3000, 3), (3000, 2), (2, 3), (4099, 1)]:
        per = nb.shard_bodies_per_rank(n, world)
        for r in range(world):
            assert R.rank_range(n, r, world) == (min(n, r * per), min(n, (r + 1) * per))
    # the placed probe states have what the GPU matrix claims: a first, a middle, a ragged last and an empty rank
    assert R.rank_range(300, 2, 3) == (300, 300) and R.rank_range(300, 1, 3) == (256, 300)
    assert [R.rank_range(700, r, 3) for r in range(3)] == [(0, 256), (256, 512), (512, 700)]
    assert [R.rank_range(3000, r, 3) for r in range(3)] == [(0, 1024), (1024, 2048), (2048, 3000)]
    assert R.rank_range(3000, 1, 2) == (1536, 3000) and R.rank_range(700, 1, 2) == (512, 700)
