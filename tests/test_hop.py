"""nb_hop_regroup against the plain-Python regroup of tests/hop_ref.py on random group graphs (ties in the
boundary densities, non-viable chains, everything non-viable, no rows, no boundaries) and its refusals; what
nb_sim_hop refuses without a device; the Python result class; the two restatements of the hop agreeing with ==."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import hop_ref as H
from tests import knn_ref as K


def _graph(rng, m, b, levels=None, nan_peaks=False):
    """m rows of random labels, counts, sums and peak densities; b boundaries among random label pairs, some of
    whose labels are no row's.  levels: draw the densities from that many values, so that many tie."""
    from wgpu_n_body_amd import _lib
    labels = np.sort(rng.choice(4 * m + 8, m, replace=False)).astype(np.uint32)
    rows = np.zeros(m, dtype=_lib.FOF_GROUP_DTYPE)
    rows["label"], rows["count"] = labels, rng.integers(1, 500, m)
    for f in ("mass", "mr2", "mv2"):
        rows[f] = rng.uniform(0.5, 2.0, m)
    rows["mx"], rows["mv"] = rng.normal(size=(m, 3)), rng.normal(size=(m, 3))
    draw = (lambda k: rng.uniform(0.0, 10.0, k)) if levels is None else (lambda k: rng.integers(0, levels, k) * 1.25)
    peak = draw(m)
    if nan_peaks and m:
        peak[rng.integers(0, m, max(1, m // 5))] = np.nan
    pool = np.unique(np.concatenate([labels, rng.choice(4 * m + 8, 3, replace=False).astype(np.uint32)]))
    pairs = set()
    for _ in range(4 * b):
        a, c = rng.choice(pool, 2, replace=False)
        pairs.add((int(min(a, c)), int(max(a, c))))
        if len(pairs) >= b:
            break
    pairs = sorted(pairs)
    bnd = np.zeros(len(pairs), dtype=_lib.HOP_BOUNDARY_DTYPE)
    if pairs:
        bnd["a"], bnd["b"] = np.array(pairs, dtype=np.uint32).T
    bnd["pairs"], bnd["density"] = rng.integers(1, 9, len(pairs)), draw(len(pairs))
    return rows, peak, bnd


def _call(rows, peak, bnd, saddle, peak_thr, cap=None, flags=0, reserved=0, params=True, count=True):
    from wgpu_n_body_amd import _lib
    m = len(rows)
    cap = m if cap is None else cap
    rp = _lib.nb_hop_regroup_params()
    rp.saddle, rp.peak, rp.flags, rp.reserved = saddle, peak_thr, flags, reserved
    merged = np.full(m + 1, 0xDEADBEEF, np.uint32)
    out_rows = np.zeros(cap + 1, dtype=_lib.FOF_GROUP_DTYPE)
    out_rows["label"] = 0xDEADBEEF
    out_peak = np.full(cap + 1, -7.0)
    cnt = C.c_size_t(12345)
    rc = _lib.lib().nb_hop_regroup(rows.ctypes.data if m else None, peak.ctypes.data if m else None, m,
                                   bnd.ctypes.data if len(bnd) else None, len(bnd), C.byref(rp) if params else None,
                                   merged.ctypes.data, out_rows.ctypes.data, out_peak.ctypes.data, cap,
                                   C.byref(cnt) if count else None)
    return rc, merged, out_rows, out_peak, cnt.value


def _sums_of(rows):
    return np.column_stack([rows["mass"], rows["mx"], rows["mv"], rows["mr2"], rows["mv2"]]).reshape(len(rows), 9)


def _check(rows, peak, bnd, saddle, peak_thr):
    m = len(rows)
    rc, merged, out_rows, out_peak, cnt = _call(rows, peak, bnd, saddle, peak_thr)
    assert rc == 0
    want = H.regroup(rows["label"], rows["count"], _sums_of(rows), peak, [tuple(e) for e in bnd], saddle, peak_thr)
    assert cnt == len(want[1])
    assert np.array_equal(merged[:m], want[0]) and merged[m] == 0xDEADBEEF
    assert np.array_equal(out_rows["label"][:cnt], want[1]) and np.array_equal(out_rows["count"][:cnt], want[2])
    assert np.array_equal(_sums_of(out_rows[:cnt]), want[3])  # the same additions in the same order
    assert np.array_equal(out_peak[:cnt], want[4], equal_nan=True)
    assert out_rows["label"][cnt] == 0xDEADBEEF and np.all(out_peak[cnt:] == -7.0)
    return want


@pytest.mark.parametrize("seed", range(8))
def test_regroup_random_graphs(nb, seed):
    rng = np.random.default_rng(seed)
    for m, b in ((1, 0), (2, 1), (7, 10), (40, 90), (200, 500)):
        rows, peak, bnd = _graph(rng, m, b, nan_peaks=seed % 2 == 1)
        for saddle, thr in ((2.0, 5.0), (5.0, 5.0), (-math.inf, -math.inf), (0.0, math.inf), (9.0, 9.5)):
            _check(rows, peak, bnd, saddle, thr)


@pytest.mark.parametrize("seed", range(4))
def test_regroup_ties_in_boundary_density(nb, seed):
    """Densities from three values: the processing order among equal ones is ascending (a, b), and it matters."""
    rng = np.random.default_rng(100 + seed)
    for m, b in ((6, 12), (30, 120)):
        rows, peak, bnd = _graph(rng, m, b, levels=3)
        for saddle, thr in ((1.25, 1.25), (2.5, 2.5), (1.25, 2.5)):
            _check(rows, peak, bnd, saddle, thr)


def test_regroup_chains_and_empties(nb):
    from wgpu_n_body_amd import _lib
    rows = np.zeros(5, dtype=_lib.FOF_GROUP_DTYPE)
    rows["label"], rows["count"], rows["mass"] = [3, 10, 11, 40, 90], [5, 6, 7, 8, 9], [1.0, 2.0, 4.0, 8.0, 16.0]
    peak = np.array([9.0, 1.0, 1.5, 1.2, 8.0])
    bnd = np.zeros(4, dtype=_lib.HOP_BOUNDARY_DTYPE)
    bnd["a"], bnd["b"], bnd["density"] = [3, 10, 11, 40], [10, 11, 40, 90], [0.9, 0.8, 0.7, 0.6]
    # a chain of three non-viable groups between two viable ones: 10, 11 and 40 end up with the peak at 3, whose
    # boundary is processed first; the last boundary then lies between two viable sets, below the saddle
    want = _check(rows, peak, bnd, 2.0, 5.0)
    assert list(want[0]) == [3, 3, 3, 3, 90] and list(want[2]) == [26, 9]
    # ... above the saddle: one group, represented by the denser peak
    want = _check(rows, peak, bnd, 0.5, 5.0)
    assert list(want[0]) == [3] * 5 and list(want[2]) == [35] and want[4][0] == 9.0
    # everything non-viable: no rows, every merged_of_row NONE
    want = _check(rows, peak, bnd, 2.0, 100.0)
    assert np.all(want[0] == H.NONE) and len(want[1]) == 0
    # no boundaries: the viable rows, unchanged
    want = _check(rows, peak, bnd[:0], 2.0, 5.0)
    assert list(want[1]) == [3, 90] and list(want[0]) == [3, H.NONE, H.NONE, H.NONE, 90]
    # no rows (boundaries between labels that are no rows are skipped)
    want = _check(rows[:0], peak[:0], bnd, 2.0, 5.0)
    assert len(want[1]) == 0
    _check(rows[:0], peak[:0], bnd[:0], 2.0, 5.0)
    # a capacity below the total: the first rows, the total reported
    rc, merged, out_rows, out_peak, cnt = _call(rows, peak, bnd, 2.0, 5.0, cap=1)
    assert rc == 0 and cnt == 2 and out_rows["label"][0] == 3 and out_rows["count"][0] == 26
    assert out_rows["label"][1] == 0xDEADBEEF and out_peak[1] == -7.0 and list(merged[:5]) == [3, 3, 3, 3, 90]


def test_regroup_refusals(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(5)
    rows, peak, bnd = _graph(rng, 6, 8)

    def refused(*a, **kw):
        rc, merged, out_rows, out_peak, cnt = _call(*a, **kw)
        assert np.all(merged == 0xDEADBEEF) and np.all(out_peak == -7.0) and np.all(out_rows["label"] == 0xDEADBEEF)
        assert cnt == 12345
        return rc == _lib.NB_ERR_INVALID and bool(L.nb_last_error())

    assert _call(rows, peak, bnd, 1.0, 2.0)[0] == 0
    assert refused(rows, peak, bnd, math.nan, 2.0) and refused(rows, peak, bnd, 1.0, math.nan)
    assert refused(rows, peak, bnd, 3.0, 2.0)  # saddle > peak
    assert refused(rows, peak, bnd, 1.0, 2.0, flags=1) and refused(rows, peak, bnd, 1.0, 2.0, reserved=1)
    assert refused(rows, peak, bnd, 1.0, 2.0, params=False) and refused(rows, peak, bnd, 1.0, 2.0, count=False)
    swapped = rows.copy()
    swapped[[1, 2]] = swapped[[2, 1]]
    assert refused(swapped, peak, bnd, 1.0, 2.0)
    same = rows.copy()
    same["label"][3] = same["label"][2]
    assert refused(same, peak, bnd, 1.0, 2.0)
    bad = bnd.copy()
    bad[[0, 1]] = bad[[1, 0]]
    assert refused(rows, peak, bad, 1.0, 2.0)
    bad = bnd.copy()
    bad["a"][2], bad["b"][2] = bad["b"][2], bad["a"][2]  # a > b
    assert refused(rows, peak, bad, 1.0, 2.0)
    rp = _lib.nb_hop_regroup_params()
    rp.saddle, rp.peak = 1.0, 2.0
    cnt = C.c_size_t(0)
    assert L.nb_hop_regroup(None, None, 3, None, 0, C.byref(rp), None, None, None, 0, C.byref(cnt)) == _lib.NB_ERR_INVALID
    assert L.nb_hop_regroup(rows.ctypes.data, peak.ctypes.data, 6, None, 2, C.byref(rp), None, None, None, 0,
                            C.byref(cnt)) == _lib.NB_ERR_INVALID
    # null outputs are allowed
    assert L.nb_hop_regroup(rows.ctypes.data, peak.ctypes.data, 6, bnd.ctypes.data, len(bnd), C.byref(rp), None, None,
                            None, 0, C.byref(cnt)) == 0


def test_refusals_without_a_device(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    assert nb.HOP_NONE == H.NONE == _lib.NB_HOP_NONE
    fake = C.c_void_p(1)  # never dereferenced: the parameters are checked first

    def call(fn, handle, **kw):
        p = _lib.nb_hop_params()
        p.k_density, p.k_hop, p.k_merge, p.min_members, p.density_min = 32, 16, 4, 1, -math.inf
        for key, v in kw.items():
            setattr(p, key, v)
        lab = np.full(4, 7, np.uint32)
        rc = fn(handle, C.byref(p), lab.ctypes.data, None, None, None, None, 0, None, 0, None)
        assert np.all(lab == 7)
        return rc

    for fn in (L.nb_sim_hop, L.nb_runner_hop):
        for bad in ({"k_density": 1}, {"k_density": 0}, {"k_density": 65}, {"k_hop": 0}, {"k_hop": 65}, {"k_merge": 0},
                    {"k_merge": 65}, {"k_merge": 0xFFFFFFFF}, {"min_members": 0}, {"density_min": math.nan},
                    {"flags": 1}, {"reserved32": 1}, {"reserved": 1}):
            assert call(fn, fake, **bad) == _lib.NB_ERR_INVALID and L.nb_last_error(), bad
        assert fn(fake, None, None, None, None, None, None, 0, None, 0, None) == _lib.NB_ERR_INVALID
        assert b"null params" in L.nb_last_error()
        assert call(fn, None) == _lib.NB_ERR_INVALID
        assert call(fn, None, density_min=math.inf) == _lib.NB_ERR_INVALID  # (valid parameters: the null handle)


def test_result_class(nb):
    from wgpu_n_body_amd import _lib
    rows = np.zeros(3, dtype=_lib.FOF_GROUP_DTYPE)
    rows["label"], rows["count"], rows["mass"] = [0, 4, 5], [3, 2, 1], [2.0, 4.0, 0.0]
    rows["mx"][:, 0], rows["mv"][:, 1], rows["mr2"], rows["mv2"] = [2.0, 4.0, 0.0], [4.0, 2.0, 0.0], [4.0, 8.0, 0.0], 16.0
    bnd = np.zeros(2, dtype=_lib.HOP_BOUNDARY_DTYPE)
    bnd["a"], bnd["b"], bnd["pairs"], bnd["density"] = [0, 4], [4, 5], [3, 1], [2.0, 0.25]
    labels = np.array([0, 0, 0, H.NONE, 4, 5, 4], np.uint32)
    gof = np.array([0, 0, 0, H.NONE, 1, 2, 1], np.uint32)
    st = nb.HopStats(7, 7, 1, 6, 0, 0, 3, 3, 6, 2, 4, 3, 0)
    g = nb.HopGroups(labels, gof, None, rows, np.array([5.0, 3.0, 0.5]), bnd, (32, 16, 4), 1, -math.inf, st)
    assert np.array_equal(g.label, [0, 4, 5]) and np.array_equal(g.count, [3, 2, 1]) and np.array_equal(g.mass, [2.0, 4.0, 0.0])
    assert np.array_equal(g.com[:2], [[1.0, 0.0, 0.0], [1.0, 0.0, 0.0]]) and np.all(np.isnan(g.com[2]))
    assert np.array_equal(g.velocity[:2], [[0.0, 2.0, 0.0], [0.0, 0.5, 0.0]])
    assert np.array_equal(g.rms_radius[:2], [1.0, 1.0]) and np.array_equal(g.sigma[:2], [2.0, math.sqrt(3.75)])
    assert list(g.by_size()) == [0, 1, 2]
    # the saddle between 0 and 4 (2.0) is above 1.0: they merge; 5 (peak 0.5) is not viable and joins them through
    # its boundary with 4
    m = g.regroup(1.0, 2.5)
    assert np.array_equal(m.label, [0]) and np.array_equal(m.count, [6]) and np.array_equal(m.peak_density, [5.0])
    assert np.array_equal(m.labels, [0, 0, 0, H.NONE, 0, 0, 0]) and np.array_equal(m.group_of, [0, 0, 0, H.NONE, 0, 0, 0])
    assert m.boundaries is None and (m.stats.groups, m.stats.grouped_bodies, m.stats.boundaries) == (1, 6, 0)
    assert (m.stats.largest_count, m.stats.largest_label) == (6, 0) and m.mass[0] == 6.0
    # a saddle above every boundary: 0 and 4 stay apart, 5 goes to the set its densest boundary leads to
    m = g.regroup(2.5, 2.5)
    assert np.array_equal(m.label, [0, 4]) and np.array_equal(m.count, [3, 3])
    assert np.array_equal(m.labels, [0, 0, 0, H.NONE, 4, 4, 4]) and np.array_equal(m.group_of, [0, 0, 0, H.NONE, 1, 1, 1])
    # nothing viable
    m = g.regroup(2.5, 50.0)
    assert len(m.rows) == 0 and np.all(m.labels == H.NONE) and np.all(m.group_of == H.NONE)
    assert (m.stats.largest_count, m.stats.largest_label) == (0, H.NONE)
    with pytest.raises(ValueError):
        m.regroup(1.0, 2.0)  # no boundaries
    with pytest.raises(nb.NBodyError):
        g.regroup(3.0, 2.0)


CASES = [("ball", K.state_of(K.ball(np.random.default_rng(1), 150, 1.0), 1)),
         ("lattice", K.state_of(K.lattice(5), 2)),
         ("coincident", K.state_of(np.concatenate([np.tile([(0.3, -0.2, 0.1)], (12, 1)),
                                                   np.random.default_rng(3).normal(size=(100, 3))]), 3)),
         ("two_clumps", H.two_clumps(4, per=80, bridge=6)),
         ("nonfinite", K.inject_nonfinite(K.state_of(np.random.default_rng(5).normal(size=(120, 3)), 5), 20, 6))]


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c[0] for c in CASES])
def test_restatements_agree(idx):
    name, state = CASES[idx]
    if name == "coincident":
        state[5, 9] = 0.0
        state[20:24, 9] = -1.0  # zero and negative masses
    for ks in ((2, 1, 1), (6, 6, 6), (8, 64, 2), (32, 16, 4)):
        a = H.hop_vectorised(state, *ks)
        assert np.array_equal(a["labels"], H.hop_loop(state, *ks)), ks
        inside = a["labels"] != H.NONE
        assert np.all(a["labels"][a["labels"][inside]] == a["labels"][inside])  # a peak is its own label
        assert a["counted"] + a["nonfinite"] == a["n"] and a["peaks"] >= (1 if inside.any() else 0)
        assert a["boundary_pairs"] == int(a["boundaries"]["pairs"].sum())
        if name == "coincident" and ks[0] <= 6:
            assert np.isinf(a["density"]).sum() >= 12
    cut = float(np.median(H.hop_vectorised(state, 6, 6, 6)["density"]))
    a = H.hop_vectorised(state, 6, 6, 6, density_min=cut)
    assert np.array_equal(a["labels"], H.hop_loop(state, 6, 6, 6, density_min=cut)) and a["outside"] > 0
    assert np.all(H.hop_vectorised(state, 6, 6, 6, density_min=math.inf)["labels"][~np.isinf(a["density"])] == H.NONE)


def test_short_states_of_the_restatement():
    s = K.state_of(np.random.default_rng(9).normal(size=(17, 3)), 9)
    for ks in ((16, 17, 2), (17, 2, 2), (2, 2, 17)):
        a = H.hop_vectorised(s, *ks)
        assert a["short_of_k"] == 17 and np.all(a["labels"] == H.NONE) and a["groups"] == 0 and len(a["boundaries"]) == 0
    a = H.hop_vectorised(s, 16, 16, 16)
    assert a["short_of_k"] == 0 and np.all(a["labels"] != H.NONE)


def test_the_physical_case_of_the_restatement():
    """Two clumps and a thin bridge: one friends-of-friends group, two regrouped density-peak groups."""
    from tests import fof_ref
    s = H.two_clumps(1, bridge=32)
    assert fof_ref.fof_grid(s, 0.2, 20)["groups"] == 1
    r = H.hop_vectorised(s, 32, 16, 4)
    med = float(np.median(r["density"]))
    out = H.regroup(r["rows_label"], r["rows_count"], r["sums"], r["peak_density"], r["boundaries"], 2.5 * med, 3 * med)
    assert r["groups"] > 2 and len(out[1]) == 2 and out[2].sum() == 4096 and abs(int(out[2][0]) - 2048) < 16
