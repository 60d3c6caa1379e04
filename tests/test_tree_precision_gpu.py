"""The floating-point half of the Barnes-Hut step against binary64, on a real MI355X -- `-m gpu`.

tests/test_tree_gpu.py pins the integer work bit for bit and the forces statistically.  Here every internal node's
moments and every body's force, velocity, mass and position of ONE step are held to what their number formats allow,
per node and per body, against tests/tree_ref.py (whose own standing against the oracle tests/test_tree_ref.py
establishes on the CPU), in every walk shape:
  1. moments: each internal node of read_tree within moment_tolerance of moments64 -- one rounding to float plus the
     cancellation of a binary64 prefix difference; a massless cell has mass 0 and a NaN cog; leaves bit-exact;
  2. forces: each body whose acceptance tests all stay clear of theta (not "flagged") within K x 2^-24 x sum |term| of
     walk64 of the tree read back from the GPU (K = 4 K_REF, derived in tree_ref.py, not from the GPU's output); a
     flagged body within check_step's cap on the worst body;
  3. counters: visits and accepts equal walk64's where the case has no flagged body;
  4. v' == kick(kick(v, a_old, dt), a'_gpu, dt) bit for bit from the GPU's own new acceleration; mass carried bit
     for bit; positions the oracle's bit for bit;
  5. everything finite -- in the massless cases too, where whole cells have no centre of gravity.
"""
import functools

import numpy as np
import pytest

from tests import tree_ref as R
from tests.helpers import E, bits
from tests.test_tree_gpu import WALK_SHAPES, rel_err, run_tree

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(case, state, oracle step) -- computed once per case, shared by the tests, never modified."""
    from oracle import oracle as O
    O.build()
    case = R.CASES[R.CASE_IDS.index(name)]
    _name, _kind, _n, _seed, theta, g, dt = case
    s = R.case_state(case)
    s.setflags(write=False)
    return case, s, O.tree_step_f32(s, g, E, dt, theta, flags=O.INTENDED)


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_node_moments_against_binary64(gpu, name):
    case, s, ref = case_inputs(name)
    _name, _kind, n, _seed, theta, g, dt = case
    r = run_tree(gpu, s, theta, 1, g, E, dt)
    assert not r["status"].any()
    tree, want = r["tree"], ref["tree"]
    assert r["root_width"] == np.float32(ref["root_width"]) and len(tree) == len(want)
    assert np.array_equal(r["order"], ref["order"])
    assert np.array_equal(tree["bodies"], want["bodies"]) and np.array_equal(tree["children"], want["children"])
    leaves = want["bodies"] == 1
    leaves[0] = False
    assert np.array_equal(bits(tree["cog"][leaves]), bits(want["cog"][leaves]))
    assert np.array_equal(bits(tree["mass"][leaves]), bits(want["mass"][leaves]))
    worst_m, worst_c = R.check_moments(tree, s)
    print(f"{name}: worst internal node at {worst_m:.3f} (mass) and {worst_c:.3f} (cog) of its tolerance")
    if name == "massless-pocket":
        assert ((tree["mass"] == 0.0) & ~leaves).sum() >= 3          # whole internal cells of mass 0


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_forces_counters_and_integrator_in_every_walk_shape(gpu, name):
    case, s, ref = case_inputs(name)
    _name, _kind, n, _seed, theta, g, dt = case
    src = s[ref["order"]]                  # the source rows in sorted order
    w = first = None
    for shape in WALK_SHAPES:
        r = run_tree(gpu, s, theta, 1, g, E, dt, tuning=shape)
        got = r["dst"]
        assert not r["status"].any(), shape
        if first is None:
            first = r
            assert np.array_equal(r["order"], ref["order"])
            w = R.walk64(r["tree"], r["root_width"], r["order"], got[:, 0:3], theta, g, E, dt)
            assert np.isfinite(w["acc"]).all()
            if name in R.MASSLESS:         # the massless bodies are accelerated like any other
                assert (np.linalg.norm(w["acc"][src[:, 9] == 0.0], axis=1) > 0.0).all()
        else:
            assert r["tree"].tobytes() == first["tree"].tobytes() and r["root_width"] == first["root_width"], shape
        flagged = w["flagged"]
        units = R.force_units(got[:, 6:9], w)
        rel = rel_err(got[:, 6:9], w["acc"])
        print(f"{name} {shape}: worst body {units[~flagged].max() if (~flagged).any() else 0.0:.2f} units of K = {R.K}, "
              f"median {np.median(units):.2f}; {int(flagged.sum())} flagged (worst rel {rel[flagged].max() if flagged.any() else 0.0:.1e}); "
              f"visits {int(r['counters'][0])} / {w['visits']}, accepts {int(r['counters'][1])} / {w['accepts']}")
        # 5. finite
        assert np.isfinite(got).all(), (shape, int((~np.isfinite(got).all(1)).sum()))
        # 2. forces
        assert (units[~flagged] <= R.K).all(), (shape, int(np.argmax(np.where(flagged, 0.0, units))), float(units[~flagged].max()))
        assert (rel[flagged] < 5e-2).all(), (shape, rel[flagged].max())
        # 3. counters
        visits, accepts = int(r["counters"][0]), int(r["counters"][1])
        if not flagged.any():
            assert (visits, accepts) == (w["visits"], w["accepts"]), shape
        else:
            assert abs(visits - w["visits"]) <= max(2, 1e-5 * w["visits"]), shape
            assert abs(accepts - w["accepts"]) <= max(2, 1e-5 * w["accepts"]), shape
        # 4. velocity from the GPU's own new acceleration, mass, position: bit for bit
        v_new = R.kick32(R.kick32(src[:, 3:6], src[:, 6:9], dt), got[:, 6:9], dt)
        assert np.array_equal(bits(got[:, 3:6]), bits(v_new)), shape
        assert np.array_equal(bits(got[:, 9]), bits(src[:, 9])), shape
        assert np.array_equal(bits(got[:, 0:3]), bits(ref["dst"][:, 0:3])), shape
