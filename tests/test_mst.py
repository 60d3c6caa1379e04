"""The restatements of the spanning tree's rule (tests/mst_ref.py) against each other, against scipy and against the
friends-of-friends restatement (tests/fof_ref.py); nb_mst_cut and nb_mst_linkage through the library; the host side of
SpanningTree; every refusal that needs no device; and mutations that show the cases have power.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import fof_ref as F
from tests import knn_ref as K
from tests import mst_ref as M

CASES = M.small_cases()
IDS = [c[0] for c in CASES]
REFS = {}


def _ref(idx):
    """prim's tree with its rounds, made once per case and left unchanged."""
    if idx not in REFS:
        REFS[idx] = M.reference(CASES[idx][1])
    return REFS[idx]


def _same_tree(a, b):
    return (np.array_equal(a.lo, b.lo) and np.array_equal(a.hi, b.hi) and a.d2.tobytes() == b.d2.tobytes()
            and np.array_equal(a.degree, b.degree))


def _links(ref):
    """Below the shortest edge, between edges, exactly at an edge's sqrt(d2) rounded both ways, above the longest."""
    d = np.unique(ref.d2[ref.d2 > 0.0])
    if d.size == 0:
        return [0.5, 2.0]
    out = [0.5 * math.sqrt(d[0]), 2.0 * math.sqrt(d[-1])]
    for q in (d[0], d[d.size // 2], d[-1]):
        r = math.sqrt(q)
        out += [float(np.nextafter(r, 0.0)), r, float(np.nextafter(r, math.inf))]
    if d.size > 1:
        out.append(0.5 * (math.sqrt(d[d.size // 2 - 1]) + math.sqrt(d[d.size // 2])))
    return [x for x in out if x > 0.0 and x * x > 0.0]


def _tree_of(nb, ref, stats_n=None):
    """A SpanningTree around a restatement's arrays: the host side of the class without a device."""
    st = nb.MstStats(0, ref.n, ref.nonfinite, ref.edges, ref.rounds, ref.components_after, ref.d2_min, ref.d2_max,
                     ref.plan_lo, ref.plan_hi, ref.h)
    return nb.SpanningTree(np.stack((ref.lo, ref.hi), axis=1).astype(np.uint32), ref.d2.copy(), ref.degree.copy(), st)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_restatements_agree(idx):
    name, state = CASES[idx]
    ref = _ref(idx)
    ok = F.body_ok(state)
    c = int(ok.sum())
    assert ref.edges == max(c, 1) - 1 and ref.nonfinite == len(state) - c
    assert _same_tree(ref, M.kruskal(state))
    b = M.boruvka(state)
    assert _same_tree(ref, b)
    assert (ref.rounds, ref.components_after.tolist()) == (b.rounds, b.components_after.tolist())
    assert np.all(ref.lo < ref.hi) and np.all(np.diff(ref.d2) >= 0)
    key = list(zip(ref.d2.tolist(), ref.lo.tolist(), ref.hi.tolist()))
    assert key == sorted(key) and len(set(key)) == len(key)
    assert ref.degree[ok].sum() == 2 * ref.edges and np.all(ref.degree[~ok] == M.NONE)
    before = c
    for r in range(ref.rounds):  # a round at least halves the components
        assert ref.components_after[r] <= before // 2
        before = int(ref.components_after[r])
    assert before == min(c, 1) and not ref.components_after[ref.rounds:].any()
    assert ref.rounds <= max(1, math.ceil(math.log2(max(len(state), 2))))


def test_piles_are_one_round_of_zero_edges():
    """P bodies at one point are P - 1 edges of d2 = 0 to the smallest index among them, found in the first round."""
    idx = IDS.index("piles6x12")
    ref, state = _ref(idx), CASES[idx][1]
    zero = ref.d2 == 0.0
    assert zero.sum() == 6 * 11 and ref.components_after[0] == 6
    for a, b in zip(ref.lo[zero], ref.hi[zero]):
        same = np.flatnonzero((state[:, 0:3] == state[b, 0:3]).all(axis=1))
        assert a == same.min()


@pytest.mark.parametrize("name", ["ball96", "n64", "n65", "two_blobs"])
def test_tie_free_cases_against_scipy(nb, name):
    from scipy.cluster.hierarchy import linkage
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import minimum_spanning_tree
    idx = IDS.index(name)
    state, ref = CASES[idx][1], _ref(idx)
    assert M.tie_free(state)
    pos64 = state[:, 0:3].astype(np.float64)
    dense = M.d2_rows(pos64, np.arange(len(pos64)))
    # (the dense matrix handed over in CSR form, every pair stored: scipy's own conversion of a dense graph takes
    # entries below 1e-8 for missing edges, and the d2 inside a blob of radius 1e-3 are smaller than that)
    t = minimum_spanning_tree(csr_matrix(dense)).tocoo()
    assert math.fsum(t.data) == math.fsum(ref.d2)
    assert sorted(zip(np.minimum(t.row, t.col), np.maximum(t.row, t.col))) == sorted(zip(ref.lo, ref.hi))
    z = _tree_of(nb, ref).to_scipy()
    want = linkage(pos64, "single")
    assert np.array_equal(z[:, [0, 1, 3]], want[:, [0, 1, 3]])
    # scipy forms its distances from its own sum of squares; sqrt(d2) is within two units in the last place of it
    assert np.array_equal(z[:, 2], np.sqrt(ref.d2)) and np.allclose(z[:, 2], want[:, 2], rtol=4e-16, atol=0.0)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_cut_is_friends_of_friends(nb, idx):
    """cut(link), restated and through the library, equals the brute-force friends-of-friends labels."""
    name, state = CASES[idx]
    ref = _ref(idx)
    tree = _tree_of(nb, ref)
    for link in _links(ref):
        want = F.fof_brute(state, link)["labels"]
        got, comps = M.cut(ref, link)
        assert np.array_equal(got, want), (name, link)
        lib = tree.cut(link)
        assert lib.dtype == np.uint32 and np.array_equal(lib, want), (name, link)
        assert comps == len(set(want[want != M.NONE].tolist()))
        sizes = np.bincount(want[want != M.NONE], minlength=1)
        for mm in (1, 2, 5):
            assert tree.group_counts([link], mm)[0] == np.count_nonzero(sizes >= mm), (name, link, mm)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_linkage_through_the_library(nb, idx):
    ref = _ref(idx)
    tree = _tree_of(nb, ref)
    want = M.linkage(ref)
    got = tree.linkage()
    for g, w in zip(got, want):
        assert g.dtype == np.uint32 and np.array_equal(g, w)
    la, lb, ca, cb = got
    assert np.all(la < lb)
    if ref.edges:
        assert int(ca[-1]) + int(cb[-1]) == ref.n - ref.nonfinite
        assert tree.longest() == (int(ref.lo[-1]), int(ref.hi[-1]), math.sqrt(ref.d2[-1]))
        assert tree.total_length == float(np.cumsum(np.sqrt(ref.d2))[-1])
    else:
        assert tree.longest() is None and tree.total_length == 0.0


def test_largest_gap(nb):
    idx = IDS.index("two_blobs")
    tree = _tree_of(nb, _ref(idx))
    ratio, link = tree.largest_gap()
    ln = tree.length
    assert link == ln[-2] and ratio == ln[-1] / ln[-2] and ratio > 100.0  # the bridge between the blobs
    assert tree.group_counts([link], 2)[0] == 2 and len(set(tree.cut(link).tolist())) == 2
    assert np.isnan(_tree_of(nb, _ref(IDS.index("n2"))).largest_gap()).all()


def test_cut_without_degree_and_null_outputs(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    idx = IDS.index("nonfinite")
    ref = _ref(idx)
    labels = np.empty(ref.n, np.uint32)
    comps = C.c_size_t(77)
    link = 2.0 * math.sqrt(ref.d2_max)
    assert L.nb_mst_cut(ref.n, ref.edges, ref.lo.ctypes.data, ref.hi.ctypes.data, ref.d2.ctypes.data, None, link,
                        labels.ctypes.data, C.byref(comps)) == 0
    bad = ref.degree == M.NONE  # without degree every body counts: the uncounted are components of their own
    assert comps.value == 1 + bad.sum() and np.array_equal(labels[bad], np.flatnonzero(bad))
    assert L.nb_mst_linkage(ref.n, ref.edges, ref.lo.ctypes.data, ref.hi.ctypes.data, None, None, None, None) == 0
    assert L.nb_mst_cut(0, 0, None, None, None, None, 1.0, None, None) == 0
    assert L.nb_mst_linkage(0, 0, None, None, None, None, None, None) == 0


def test_refusals_without_a_device(nb):
    from wgpu_n_body_amd import _lib
    L = _lib.lib()
    lo, hi = np.array([0, 1], np.uint32), np.array([1, 2], np.uint32)
    d2 = np.array([1.0, 4.0])
    labels = np.full(4, 0xDEADBEEF, np.uint32)

    def cut(n=4, m=2, a=lo, b=hi, d=d2, link=1.5, out=labels):
        ptr = lambda x: None if x is None else x.ctypes.data
        return L.nb_mst_cut(n, m, ptr(a), ptr(b), ptr(d), None, link, ptr(out), None)

    assert cut() == 0 and labels.tolist() == [0, 0, 2, 3]
    labels[:] = 0xDEADBEEF
    for link in (0.0, -1.0, math.nan, math.inf, 1e-170, 1e160):  # the refusals of nb_sim_fof's link
        assert cut(link=link) == _lib.NB_ERR_INVALID, link
    assert cut(link=1e-9) == 0  # (no cells: a link nb_sim_fof may refuse for its grid)
    labels[:] = 0xDEADBEEF
    for kw in (dict(a=None), dict(b=None), dict(d=None), dict(out=None), dict(m=4), dict(n=2), dict(n=2 ** 32),
               dict(a=np.array([1, 1], np.uint32)), dict(a=np.array([2, 1], np.uint32)),
               dict(b=np.array([1, 4], np.uint32))):
        assert cut(**kw) == _lib.NB_ERR_INVALID, kw
        assert b"mst_cut" in L.nb_last_error()
    assert np.all(labels == 0xDEADBEEF)  # a refused call writes nothing

    out = [np.full(3, 0xDEADBEEF, np.uint32) for _ in range(4)]
    cyc_lo, cyc_hi = np.array([0, 1, 0], np.uint32), np.array([1, 2, 2], np.uint32)
    args = [o.ctypes.data for o in out]
    assert L.nb_mst_linkage(4, 3, cyc_lo.ctypes.data, cyc_hi.ctypes.data, *args) == _lib.NB_ERR_INVALID
    assert b"cycle" in L.nb_last_error() and all(np.all(o == 0xDEADBEEF) for o in out)
    assert L.nb_mst_linkage(4, 3, None, cyc_hi.ctypes.data, *args) == _lib.NB_ERR_INVALID
    assert L.nb_mst_linkage(3, 3, cyc_lo.ctypes.data, cyc_hi.ctypes.data, *args) == _lib.NB_ERR_INVALID

    # nb_mst_sim / nb_mst_runner: params are checked before the handle is looked at, the handle before any device call
    st = _lib.nb_mst_stats()
    for call in (L.nb_mst_sim, L.nb_mst_runner):
        assert call(None, None, None, None, None, None, C.byref(st)) == _lib.NB_ERR_INVALID
        assert b"null params" in L.nb_last_error()
        for field in ("flags", "reserved32", "reserved"):
            p = _lib.nb_mst_params()
            setattr(p, field, 1)
            assert call(None, C.byref(p), None, None, None, None, C.byref(st)) == _lib.NB_ERR_INVALID
            assert b"mst:" in L.nb_last_error()
        p = _lib.nb_mst_params()
        assert call(None, C.byref(p), None, None, None, None, C.byref(st)) == _lib.NB_ERR_INVALID
        assert b"null" in L.nb_last_error()
    assert C.sizeof(_lib.nb_mst_stats) == 240 and _lib.NB_MST_NONE == M.NONE == nb.MST_NONE == nb.FOF_NONE

    tree = _tree_of(nb, _ref(IDS.index("ball96")))
    with pytest.raises(ValueError):
        tree.group_counts([1.0], 0)
    with pytest.raises(ValueError):
        tree.group_counts([0.0])
    with pytest.raises(nb.NBodyError):
        tree.cut(-1.0)


def test_mutation_the_index_decides_on_a_lattice():
    """A restatement that ignores the index tie-break differs from the rule where every nearest distance ties."""
    idx = IDS.index("lattice4")
    state, ref = CASES[idx][1], _ref(idx)
    wrong = M.kruskal(state, order=lambda d2, lo, hi: np.lexsort((-hi.astype(np.int64), -lo.astype(np.int64), d2)))
    assert wrong.edges == ref.edges and wrong.d2.tobytes() == ref.d2.tobytes()  # a minimum spanning tree all the same
    assert not _same_tree(ref, wrong)
    ball = IDS.index("ball96")  # ... and where nothing ties the order of the indices is immaterial
    assert _same_tree(_ref(ball), M.kruskal(CASES[ball][1], order=lambda d2, lo, hi: np.argsort(d2, kind="stable")))


def test_mutation_pruning_on_an_equal_bound_loses_an_edge():
    """Four bodies on a unit square whose sides are cell borders, so that a neighbour cell's bound equals the d2 of the
    body in it.  The rule keeps (0, 1), (0, 3), (1, 2).  Body 3 sees body 2 first and, pruning on B >= best, never
    opens the cell of body 0; body 2 likewise never opens body 1's: the edge (1, 2) is lost for (2, 3)."""
    pos = np.array([(1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 0)], np.float32)
    ref = M.kruskal(K.state_of(pos))
    rule = {(float(d), int(a), int(b)) for d, a, b in zip(ref.d2, ref.lo, ref.hi)}
    assert rule == {(1.0, 0, 1), (1.0, 0, 3), (1.0, 1, 2)}
    assert M.boruvka_cells(pos, 1.0, strict=True) == rule
    lost = M.boruvka_cells(pos, 1.0, strict=False)
    assert (1.0, 1, 2) not in lost and (1.0, 2, 3) in lost
