"""tests/tree_ref.py against the CPU oracle, on the case list the GPU tests use -- `-m "not gpu"`.

What this pins is the REFERENCE: that moments64 books every body into the right nodes, that walk64 visits and
accepts exactly what the oracle's per-thread walk does, that the oracle's own fp32 forces sit within K_REF units of
2^-24 x sum |term| of it (K_REF is what the GPU's bound K = 4 K_REF is derived from), and that the inputs keep the
share of bodies with an acceptance test on the edge of theta small enough for the exact checks to mean something.
"""
import functools

import numpy as np
import pytest

from tests import tree_ref as R
from tests.helpers import E


@functools.lru_cache(maxsize=None)
def reference(name):
    """(state, oracle step, walk64 of the oracle's tree) of a case, computed once and shared; never modified."""
    from oracle import oracle as O
    O.build()
    case = R.CASES[R.CASE_IDS.index(name)]
    _name, _kind, _n, _seed, theta, g, dt = case
    s = R.case_state(case)
    ref = O.tree_step_f32(s, g, E, dt, theta, flags=O.INTENDED)
    w = R.walk64(ref["tree"], ref["root_width"], ref["order"], ref["dst"][:, 0:3], theta, g, E, dt)
    return s, ref, w


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_moments64_books_the_oracles_tree(nb, name):
    """Against the oracle's own sequential fp32 sums, to the bound those deserve: b terms added one by one carry up
    to b roundings (plus the products' and the division's), relative to the sum of |term| of the cell."""
    s, ref, _w = reference(name)
    tree = ref["tree"]
    mom = R.moments64(tree, s)
    assert abs(mom["mass"][0] - s[:, 9].astype(np.float64).sum()) <= 1e-12 * mom["mass"][0]
    assert (mom["depth"][1:] == mom["depth"][mom["parent"][1:]] + 1).all()
    assert mom["leaf"].sum() == len(s) and np.array_equal(np.sort(tree["children"][mom["leaf"], 0]), np.arange(len(s)))
    x, m = s[:, 0:3].astype(np.float64), s[:, 9].astype(np.float64)
    abs_mx = R.sum_up(tree, np.abs(m[:, None] * x))
    b = tree["bodies"].astype(np.float64)
    internal = ~mom["leaf"]
    empty = internal & (mom["mass"] == 0.0)
    assert (tree["mass"][empty] == 0.0).all() and np.isnan(tree["cog"][empty]).all()
    if name == "massless-pocket":
        assert empty.sum() >= 3
    full = internal & ~empty
    assert (np.abs(tree["mass"] - mom["mass"])[full] <= (b * R.EPS32 * mom["mass"])[full]).all()
    want = mom["mom"][full] / mom["mass"][full, None]
    tol = ((2.0 * b + 4.0) * R.EPS32)[full, None] * abs_mx[full] / mom["mass"][full, None]
    assert (np.abs(tree["cog"][full] - want) <= tol).all()


def test_walk64_counts_and_forces_against_the_oracle(nb):
    """Visits and accepts equal the oracle's in every case; outside the flagged bodies the oracle's fp32 force is
    within K_REF units; the flagged share is at most 1 % per case and at least half the cases of 1,000 bodies or more
    have no flagged body at all (a condition on the inputs: a seed that breaks it is changed, not the cap)."""
    rows, big, clean = [], 0, 0
    for case in R.CASES:
        name, _kind, n, _seed, theta, g, dt = case
        s, ref, w = reference(name)
        assert (w["visits"], w["accepts"]) == (ref["stats"]["visits"], ref["stats"]["accepted"]), name
        units = R.force_units(ref["dst"][:, 6:9], w)
        share = w["flagged"].mean()
        worst = float(units[~w["flagged"]].max()) if (~w["flagged"]).any() else 0.0
        rows.append((name, n, share, worst))
        assert np.isfinite(ref["dst"]).all() and np.isfinite(w["acc"]).all(), name
        assert worst <= R.K_REF, (name, worst)
        assert share <= 0.01, (name, share)
        if n >= 1000:
            big += 1
            clean += int(not w["flagged"].any())
        # the massless bodies are accelerated like any other: their own mass does not enter
        if name in R.MASSLESS:
            massless = ref["dst"][:, 9] == 0.0
            assert massless.sum() >= R.POCKET_BODIES
            assert (np.linalg.norm(w["acc"][massless], axis=1) > 0.0).all()
    for name, n, share, worst in rows:     # (shown with `-s`: the table in tree_ref.py's docstring)
        print(f"    {name:16s} n={n:5d}  flagged {100.0 * share:6.3f} %  worst oracle body {worst:5.2f} units")
    print(f"    K_REF {R.K_REF} (max measured {max(r[3] for r in rows):.2f}), K {R.K}")
    assert 2 * clean >= big, (clean, big)
    assert max(r[3] for r in rows) > R.K_REF / 2.0     # K_REF is the measured maximum, rounded up -- not a loose guess


def test_walk64_of_a_subset_and_small_chunks_are_the_same_walk(nb):
    """`bodies` and `chunk` only slice the work: same rows, bit for bit."""
    name = "uniform-257"
    case = R.CASES[R.CASE_IDS.index(name)]
    _s, ref, w = reference(name)
    theta, g, dt = case[4], case[5], case[6]
    pick = np.array([0, 3, 100, 256])
    sub = R.walk64(ref["tree"], ref["root_width"], ref["order"], ref["dst"][:, 0:3], theta, g, E, dt, bodies=pick, chunk=3)
    assert np.array_equal(sub["acc"], w["acc"][pick]) and np.array_equal(sub["sum_abs"], w["sum_abs"][pick])
    assert np.array_equal(sub["flagged"], w["flagged"][pick])


def test_walk64_sees_a_dropped_cell(nb):
    """The size of the defect the bound K is meant to catch: one accepted cell dropped -- even a far one, two levels
    below the root -- moves a body by far more than K units."""
    name = "uniform-4099"
    case = R.CASES[R.CASE_IDS.index(name)]
    _s, ref, w = reference(name)
    theta, g, dt = case[4], case[5], case[6]
    tree = ref["tree"].copy()
    # the cells of depth 2 that body 0 accepts as a whole: drop each in turn and walk again for that body
    one = R.walk64(tree, ref["root_width"], ref["order"], ref["dst"][:, 0:3], theta, g, E, dt, bodies=[0])
    depth1 = np.nonzero(R.tree_shape(tree)[1] == 2)[0]
    moved = 0
    for node in depth1:
        t2 = tree.copy()
        t2["mass"][node] = 0.0
        two = R.walk64(t2, ref["root_width"], ref["order"], ref["dst"][:, 0:3], theta, g, E, dt, bodies=[0])
        if not np.array_equal(two["acc"], one["acc"]):       # body 0 accepts this cell as a whole
            moved += 1
            assert R.force_units(two["acc"], one)[0] > 10.0 * R.K
    assert moved > 0
