"""The numpy restatement of the unbinding rule (tests/bound_ref.py; include/nbody.h "Bound groups") against cases
worked by hand, the condition that lets tests/test_bound_gpu.py demand equal integers -- no case it uses has a
marginal decision -- the ctypes layouts, and the refusals that need no device.  No GPU."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import bound_ref as B
from tests.diag_ref import psi64
from tests.helpers import ROOT


def test_two_bodies_at_rest_are_bound():
    r = B.reference("two_at_rest")
    row = r["rows"][0]
    assert (row["count"], row["bound_count"], row["iterations"], row["status"]) == (2, 2, 1, B.CONVERGED)
    c = B.coupling(B.G, B.DT)
    phi = -c * 1.0 * psi64(np.array([np.float64(np.float32(0.1))]), np.float64(np.float32(B.E)))[0]
    assert np.allclose(r["energy"], phi, rtol=1e-14) and phi < 0
    assert np.array_equal(r["bound_of"], [0, 0]) and row["most_bound"] == 0
    assert row["kinetic"] == 0.0 and math.isclose(row["potential"], phi, rel_tol=1e-14)  # 1/2 (phi + phi)
    assert math.isclose(row["potential0"], row["potential"], rel_tol=1e-15) and row["kinetic0"] == 0.0
    assert r["pairs"] == 2 and r["bound_groups"] == 1 and r["bound_bodies"] == 2


def test_two_fast_bodies_dissolve():
    s, p = B.case("two_fast")
    c = B.coupling(B.G, B.DT)
    escape = math.sqrt(2.0 * c * 2.0 * psi64(np.array([0.1]), B.E)[0])  # of the relative orbit: sqrt(2 c (m1 + m2) psi)
    assert abs(s[1, 3] - s[0, 3]) > 10 * escape
    r = B.reference("two_fast")
    row = r["rows"][0]
    assert (row["bound_count"], row["iterations"], row["status"]) == (0, 1, B.DISSOLVED)
    assert np.all(r["energy"] > 0) and np.all(r["bound_of"] == B.NONE) and row["most_bound"] == B.NONE
    assert row["mass"] == 0.0 and math.isnan(row["phi_min"]) and row["kinetic0"] > -row["potential0"] > 0
    assert r["dissolved"] == 1 and r["bound_groups"] == 0


def test_an_interloper_leaves_in_round_one():
    s, p = B.case("interloper")
    r = B.reference("interloper")
    row = r["rows"][0]
    assert (row["count"], row["bound_count"], row["iterations"], row["status"]) == (101, 100, 2, B.CONVERGED)
    assert r["bound_of"][50] == B.NONE and r["energy"][50] > 0 and np.all(np.delete(r["bound_of"], 50) == 0)
    assert np.all(np.delete(r["energy"], 50) < 0)
    # the energies are those of round 2: about the clump's own velocity, without the interloper's pull
    rest = np.delete(s, 50, axis=0)
    alone = B.bound_ref(rest, **p)
    assert alone["rows"][0]["iterations"] == 1
    assert np.allclose(np.delete(r["energy"], 50), alone["energy"], rtol=1e-12, atol=0)
    assert math.isclose(row["potential"], alone["rows"][0]["potential"], rel_tol=1e-12)


@pytest.mark.parametrize("name", B.GPU_CASES)
def test_no_case_of_the_gpu_tests_has_a_marginal_decision(name):
    """The condition that lets tests/test_bound_gpu.py demand the reference's integers."""
    r = B.reference(name)
    assert int(r["marginal"].sum()) == 0, (name, np.flatnonzero(r["marginal"]), r["margin"].min())
    assert r["margin"].min() > 1.0


def test_the_cascade_takes_at_least_three_rounds():
    r = B.reference("cascade")
    row = r["rows"][0]
    assert row["status"] == B.CONVERGED and row["iterations"] >= 3 and 0 < row["bound_count"] < row["count"] == 1500
    assert r["pairs"] == int(row["iterations"]) * 1500 * 1499


def test_every_status_word_occurs():
    seen = set()
    for name in ("fates", "fates_two_rounds", "sizes"):
        seen |= set(int(x) for x in B.reference(name)["rows"]["status"])
    assert seen == {B.CONVERGED, B.DISSOLVED, B.UNCONVERGED, B.SKIPPED}
    two = B.reference("fates_two_rounds")
    assert two["unconverged"] > 0 and two["rounds_max"] == 2 and two["skipped"] == 1
    full = B.reference("fates")
    assert full["dissolved"] > 0 and full["unconverged"] == 0 and full["bound_groups"] > 0 and full["skipped"] == 1
    big = full["rows"][full["rows"]["count"] == 5000][0]
    assert big["status"] == B.SKIPPED and big["iterations"] == 0 and big["bound_count"] == 0
    assert np.all(np.isnan(full["energy"][full["group_of"] == np.flatnonzero(full["rows"]["count"] == 5000)[0]]))


def test_the_other_members():
    """Non-finite bodies and bodies of no group have no energy; tracers take part and attract nobody."""
    s, p = B.case("members")
    r = B.reference("members")
    assert r["nonfinite"] == 3 and r["groups"] == 2 and int((r["group_of"] == B.NONE).sum()) == 6
    assert np.all(np.isnan(r["energy"][r["group_of"] == B.NONE])) and np.all(np.isfinite(r["energy"][r["group_of"] != B.NONE]))
    massless = (s[:, 9] == 0) & (r["group_of"] != B.NONE)
    assert massless.sum() == 40
    drop = np.flatnonzero(~massless)
    without = B.bound_ref(s[drop], **p)  # the massive members alone: the same energies
    assert np.allclose(without["energy"], r["energy"][drop], rtol=1e-12, atol=0, equal_nan=True)


def test_capacity_leaves_the_later_rows_alone():
    full, part = B.reference("sizes"), B.reference("sizes", capacity=3)
    assert part["groups"] == 9 and len(part["rows"]) == 3 and part["rows"].tobytes() == full["rows"][:3].tobytes()
    later = part["group_of"] >= 3
    assert np.all(part["bound_of"][later] == B.NONE) and np.all(np.isnan(part["energy"][later]))
    assert np.array_equal(part["bound_of"][~later], full["bound_of"][~later])


def test_layouts(nb):
    from wgpu_n_body_amd import _lib
    p, g, st = _lib.nb_bound_params, _lib.nb_bound_group, _lib.nb_bound_stats
    assert C.sizeof(p) == 40 and C.sizeof(g) == 128 and C.sizeof(st) == 112
    assert [getattr(p, f).offset for f in ("link", "min_members", "min_bound", "max_iter", "max_group", "flags",
                                           "reserved32", "reserved")] == [0, 8, 12, 16, 20, 24, 28, 32]
    assert [getattr(g, f).offset for f in ("label", "count", "bound_count", "iterations", "status", "most_bound", "mass",
                                           "mx", "mv", "mr2", "kinetic", "potential", "phi_min", "kinetic0",
                                           "potential0")] == [0, 4, 8, 12, 16, 20, 24, 32, 56, 80, 88, 96, 104, 112, 120]
    assert [_lib.BOUND_GROUP_DTYPE.fields[k][1] for k in _lib.BOUND_GROUP_DTYPE.names] == \
        [getattr(g, k).offset for k in _lib.BOUND_GROUP_DTYPE.names]
    assert _lib.BOUND_GROUP_DTYPE == B.ROW_DTYPE
    assert [getattr(st, f).offset for f in ("step_num", "grouped_bodies", "largest_count", "largest_label", "bound_groups",
                                            "pairs", "rounds_max")] == [0, 40, 48, 52, 56, 96, 104]
    assert (nb.BOUND_CONVERGED, nb.BOUND_DISSOLVED, nb.BOUND_UNCONVERGED, nb.BOUND_SKIPPED) == \
        (B.CONVERGED, B.DISSOLVED, B.UNCONVERGED, B.SKIPPED)
    hdr = open(os.path.join(ROOT, "include", "nbody.h")).read()
    for word, value in (("CONVERGED", 1), ("DISSOLVED", 2), ("UNCONVERGED", 4), ("SKIPPED", 8), ("MAX_ITER", 64)):
        assert f"#define NB_BOUND_{word} {value}u" in hdr


def test_the_wrapper_refuses_counts_that_do_not_fit(nb):
    """An out-of-range count is an error, not 0: for max_group, 0 would lift the limit."""
    for bad in (dict(max_group=-1), dict(max_group=1 << 32), dict(max_iter=-3), dict(min_members=1 << 40),
                dict(min_bound=-1)):
        kw = dict(min_members=20, min_bound=None, max_iter=32, max_group=262144)
        kw.update(bad)
        with pytest.raises(ValueError):  # (before the library is called: no handle is needed)
            nb._bound_groups(None, None, 64, 0.1, kw["min_members"], kw["min_bound"], kw["max_iter"], kw["max_group"], True)


def good_params(_lib, **kw):
    p = _lib.nb_bound_params()
    p.link, p.min_members, p.min_bound, p.max_iter, p.max_group = 0.1, 20, 20, 32, 262144
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_bad_arguments_are_invalid_without_a_device(nb):
    """The parameters are checked before the handle is looked at: a null handle with good parameters is the one
    refusal that names the handle."""
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    group_of, bound_of = np.full(8, 7, np.uint32), np.full(8, 7, np.uint32)
    energy = np.full(8, 7.0)
    rows = np.zeros(4, _lib.BOUND_GROUP_DTYPE)
    st = _lib.nb_bound_stats()
    for call, who in ((L.nb_sim_bound, b"simulator"), (L.nb_runner_bound, b"runner")):
        def bad(word, p):
            assert call(None, C.byref(p) if p is not None else None, group_of.ctypes.data, bound_of.ctypes.data,
                        energy.ctypes.data, rows.ctypes.data, 4, C.byref(st)) == _lib.NB_ERR_INVALID, word
            assert word in L.nb_last_error(), (word, L.nb_last_error())
        bad(b"null params", None)
        for link in (0.0, -1.0, math.nan, math.inf, 1e-200, 1e200):
            bad(b"link", good_params(_lib, link=link))
        bad(b"min_members", good_params(_lib, min_members=0))
        bad(b"min_bound", good_params(_lib, min_bound=0))
        for it in (0, 65, 1 << 31):
            bad(b"max_iter", good_params(_lib, max_iter=it))
        bad(b"flag", good_params(_lib, flags=1))
        bad(b"reserved", good_params(_lib, reserved32=1))
        bad(b"reserved", good_params(_lib, reserved=1 << 40))
        bad(b"null " + who, good_params(_lib))
        bad(b"null " + who, good_params(_lib, max_iter=64, max_group=0, min_bound=1))
    assert np.all(group_of == 7) and np.all(bound_of == 7) and np.all(energy == 7.0) and not rows.tobytes().strip(b"\0")
    assert bytes(st) == bytes(_lib.nb_bound_stats())
