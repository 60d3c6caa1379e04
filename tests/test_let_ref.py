"""tests/let_ref.py against the CPU oracle and against all-pairs, on the case list the GPU tests use -- `-m "not gpu"`.

What this pins is the REFERENCE of the multi-domain step: that let_walk64 with one rank is walk64, that with theta -> 0
it is the all-pairs sum (no remote body skipped, no lone-body rank dropped), that its counts are the oracle's per-pair
walks added up, that the oracle's own fp32 forces sit within K_LET_REF units of it (what K_LET derives from), that the
inputs keep the flagged share small, and that the bound bites: three mutations of the reference each move a body by
more than K_LET units.

The oracle walks a tree for the rows it is given and skips the leaf whose children[0] equals order[row] (order=None:
the row's own number) -- so order=None would make a FOREIGN walker skip the remote body that happens to carry its
number.  oracle_pair therefore passes an order of 0xffffffff for foreign walkers (no leaf names that), appends one
unused row (the oracle walks nothing where it is given fewer than two rows) and, for a tree of ONE body, marks the
root as the internal cell the product makes of it (bodies = 2 in a copy: the oracle takes any octant of one body for
a leaf, the root of a lone body included, which tree_ref.tree_shape and the kernels do not).
"""
import functools

import numpy as np
import pytest

from tests import let_ref as L
from tests import tree_ref as T
from tests.helpers import E


@functools.lru_cache(maxsize=None)
def reference(name):
    """dict(state, dom, root_width, trees, ranks, src (sorted source rows per rank), w (let_walk64)) of a case,
    computed once and shared; never modified.  Unit-cube cases: the trees are the oracle's of each rank's bodies alone
    (both bounds are 1.0, so its root is the global root); wide-7.5: let_ref.tree_in_cube."""
    from oracle import oracle as O
    O.build()
    case = L.CASES[L.CASE_IDS.index(name)]
    _name, _kind, _n, _seed, theta, g, dt = L.base_case(case)
    s = T.case_state(L.base_case(case))
    dom = L.domains(s, case[2])
    rw = L.global_root_width(s)
    trees, ranks, srcs = [], [], []
    for idx in dom:
        src = s[idx]
        if len(src) == 0:
            trees.append(None)
            ranks.append(dict(x_new=np.zeros((0, 3), dtype=np.float32), order=np.zeros(0, dtype=np.int64)))
            srcs.append(src)
            continue
        if name in L.UNIT_CUBE:
            ref = O.tree_step_f32(src, g, E, dt, theta, flags=O.INTENDED)
            assert np.float32(ref["root_width"]) == rw
            tree, order = ref["tree"], ref["order"]
        else:
            tree = L.tree_in_cube(src, rw)
            order = O.tree_dfs_order(tree, len(src))
        trees.append(tree)
        srcs.append(src[order])
        ranks.append(dict(x_new=L.drift32(src[order], dt), order=order.astype(np.int64)))
    w = L.let_walk64(trees, rw, ranks, theta, g, E, dt)
    return dict(state=s, dom=dom, root_width=rw, trees=trees, ranks=ranks, src=srcs, w=w, params=(theta, g, dt))


def oracle_pair(O, ref, me, r, theta=None):
    """The oracle's fp32 walk of tree r for rank me's bodies -> (acc float32[n_me, 3], stats); see the module docstring."""
    th, g, dt = ref["params"]
    rows, n = ref["src"][me], len(ref["src"][me])
    rows = np.concatenate([rows, rows[-1:]])
    order = np.full(n + 1, 0xFFFFFFFF, dtype=np.uint32)
    if r == me:
        order[:n] = ref["ranks"][me]["order"]
    tree = ref["trees"][r]
    if tree["bodies"][0] == 1:
        tree = tree.copy()
        tree["bodies"][0] = 2
    out, stats = O.tree_walk_indices(rows, tree, ref["root_width"], g, E, dt, th if theta is None else theta,
                                     np.arange(n), order=order)
    return out[:, 6:9], stats


@pytest.mark.parametrize("base", ["uniform-2", "uniform-65", "uniform-4099", "disc", "massless-pocket"])
def test_one_rank_is_walk64_of_the_single_tree(nb, oracle, base):
    case = T.CASES[T.CASE_IDS.index(base)]
    _name, _kind, _n, _seed, theta, g, dt = case
    s = T.case_state(case)
    dom = L.domains(s, 1)
    assert len(dom) == 1 and np.array_equal(np.sort(dom[0]), np.arange(len(s)))
    src = s[dom[0]]
    ref = oracle.tree_step_f32(src, g, E, dt, theta, flags=oracle.INTENDED)
    one = T.walk64(ref["tree"], ref["root_width"], ref["order"], ref["dst"][:, 0:3], theta, g, E, dt)
    assert np.array_equal(L.drift32(src[ref["order"]], dt), ref["dst"][:, 0:3])
    let, = L.let_walk64([ref["tree"]], ref["root_width"], [dict(x_new=ref["dst"][:, 0:3], order=ref["order"])],
                        theta, g, E, dt)
    for key in ("acc", "sum_abs", "flagged"):
        assert np.array_equal(let[key], one[key]), key
    assert (let["visits"], let["accepts"]) == (one["visits"], one["accepts"])


@pytest.mark.parametrize("name", ["uniform-4099x3", "uniform-3x4"])
def test_theta_to_zero_is_the_all_pairs_sum(nb, name):
    """No internal cell is accepted at theta = 1e-4, so every body must feel every other body, of every rank, once: a
    remote body skipped for carrying the walker's number, or a rank of one body dropped, shows here."""
    ref = reference(name)
    _theta, g, dt = ref["params"]
    w = L.let_walk64(ref["trees"], ref["root_width"], ref["ranks"], 1e-4, g, E, dt)
    gg, ee, dd = (float(np.float32(v)) for v in (g, E, dt))
    x_src = np.concatenate(ref["src"])[:, 0:3].astype(np.float64)
    m_src = np.concatenate(ref["src"])[:, 9].astype(np.float64)
    x_new = np.concatenate([rk["x_new"] for rk in ref["ranks"]]).astype(np.float64)
    n = len(x_src)
    assert n == len(ref["state"])
    want, want_abs = np.zeros((n, 3)), np.zeros(n)
    for lo in range(0, n, 512):                               # (rows and columns are in the same order: rank by rank)
        rows = np.arange(lo, min(lo + 512, n))
        d = x_src[None, :, :] - x_new[rows, None, :]
        r = np.sqrt((d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2])
        t = (m_src[None, :] * gg / (r * r * r + ee))[:, :, None] * (d / r[:, :, None]) * dd
        t[rows - lo, rows] = 0.0
        want[rows], want_abs[rows] = t.sum(1), np.sqrt((t * t).sum(2)).sum(1)
    got, got_abs = np.concatenate([x["acc"] for x in w]), np.concatenate([x["sum_abs"] for x in w])
    assert np.isfinite(want).all() and (want_abs > 0.0).all()
    assert (np.linalg.norm(got - want, axis=1) <= 1e-12 * np.linalg.norm(want, axis=1)).all()
    assert (np.abs(got_abs - want_abs) <= 1e-12 * want_abs).all()
    assert L.totals(w)[1] == n * (n - 1)                      # one accept per ordered pair of bodies


@pytest.mark.parametrize("name", L.UNIT_CUBE)
def test_counts_are_the_oracles_walks_added_up(nb, oracle, name):
    """... per ordered pair of ranks that both hold bodies; and for the own tree the oracle's step itself."""
    ref = reference(name)
    theta, g, dt = ref["params"]
    world = len(ref["trees"])
    for me in range(world):
        if not len(ref["src"][me]):
            assert (ref["w"][me]["visits"], ref["w"][me]["accepts"]) == (0, 0)
            continue
        visits = accepts = 0
        for r in range(world):
            if ref["trees"][r] is None:
                continue
            _acc, st = oracle_pair(oracle, ref, me, r)
            visits += st["visits"]
            accepts += st["accepted"]
        assert (ref["w"][me]["visits"], ref["w"][me]["accepts"]) == (visits, accepts), (name, me)
        if len(ref["src"][me]) >= 2:       # oracle_pair of the own tree is the oracle's step of the rank alone
            own = oracle.tree_step_f32(ref["state"][ref["dom"][me]], g, E, dt, theta, flags=oracle.INTENDED)
            acc, st = oracle_pair(oracle, ref, me, me)
            assert np.array_equal(acc, own["dst"][:, 6:9])
            assert (st["visits"], st["accepted"]) == (own["stats"]["visits"], own["stats"]["accepted"])
    # tree_in_cube, which stands in for the oracle's build where a rank does not span the global cube, is that build
    for r in range(world):
        if ref["trees"][r] is not None:
            mine = L.tree_in_cube(ref["state"][ref["dom"][r]], ref["root_width"])
            assert np.array_equal(mine["bodies"], ref["trees"][r]["bodies"])
            assert np.array_equal(mine["children"], ref["trees"][r]["children"])
            T.check_moments(mine, ref["state"][ref["dom"][r]])


def test_the_inputs_exercise_what_they_are_there_for(nb):
    # ranks of 0 and 1 bodies
    sizes = [len(i) for i in reference("uniform-3x4")["dom"]]
    assert 0 in sizes and 1 in sizes, sizes
    assert min(len(i) for i in reference("uniform-65x8")["dom"]) < 16
    # wide-7.5: a rank whose own cube would be smaller than the global one, and trees that are well-formed
    ref = reference("wide-7.5x3")
    own = [np.abs(ref["state"][i][:, 0:3]).max() for i in ref["dom"]]
    assert ref["root_width"] == np.float32(2.0) * max(own) and min(own) < max(own) and max(own) > 7.0
    for r, tree in enumerate(ref["trees"]):
        _parent, _depth, leaf = T.tree_shape(tree)
        assert np.array_equal(np.sort(tree["children"][leaf, 0]), np.arange(len(ref["dom"][r])))
        T.check_moments(tree, ref["state"][ref["dom"][r]])
    # massless-pocket: a whole internal cell of mass 0 in some rank's tree, reached by the bodies of ANOTHER rank --
    # cutting its children off changes what they visit
    ref = reference("massless-pocketx4")
    theta, g, dt = ref["params"]
    reached = 0
    for r, tree in enumerate(ref["trees"]):
        leaf = T.tree_shape(tree)[2]
        empty = np.nonzero(~leaf & (tree["mass"] == 0.0))[0]
        assert np.isnan(tree["cog"][empty]).all()
        if not len(empty):
            continue
        cut = tree.copy()
        cut["children"][empty] = 0
        for me in range(len(ref["trees"])):
            if me != r:
                a = L.walk_pair(me, r, tree, ref["root_width"], ref["ranks"][me], theta, g, E, dt, T.FLAG_DELTA)
                b = L.walk_pair(me, r, cut, ref["root_width"], ref["ranks"][me], theta, g, E, dt, T.FLAG_DELTA)
                reached += int(a["visits"] != b["visits"])
    assert reached > 0
    # tracers: massless bodies in every rank; disc: the heavy centre inside one rank
    ref = reference("tracersx3")
    assert all((ref["state"][i][:, 9] == 0.0).any() for i in ref["dom"])
    ref = reference("discx3")
    assert sum(int((ref["state"][i][:, 9] > 1e4).any()) for i in ref["dom"]) == 1
    # dense-core: the clump is split between ranks
    ref = reference("dense-corex4")
    in_clump = [int((np.abs(ref["state"][i][:, 0:3] - np.float32(0.3)).max(1) < 3e-3).sum()) for i in ref["dom"]]
    assert sum(1 for k in in_clump if k > 100) >= 2, in_clump


def test_oracle_forces_flagged_share_and_the_bound(nb, oracle):
    """The oracle's fp32 force of a body: its fp32 walks of every rank's tree, added in fp32, own tree first and then
    the others in rank order (the order of the product's roots).  Outside the flagged bodies within K_LET_REF units
    of let_walk64; at most 1 % flagged per case, none in at least half the cases of 1,000 bodies or more."""
    rows, big, clean = [], 0, 0
    for case in L.CASES:
        name, _base, world = case
        ref = reference(name)
        n = len(ref["state"])
        units, flagged = [], []
        for me in range(world):
            if not len(ref["src"][me]):
                continue
            acc = np.zeros((len(ref["src"][me]), 3), dtype=np.float32)
            for r in [me] + [q for q in range(world) if q != me]:
                if ref["trees"][r] is not None:
                    acc = acc + oracle_pair(oracle, ref, me, r)[0]
            assert np.isfinite(acc).all() and np.isfinite(ref["w"][me]["acc"]).all(), name
            units.append(T.force_units(acc, ref["w"][me]))
            flagged.append(ref["w"][me]["flagged"])
            if case[1] in T.MASSLESS:      # the massless bodies are accelerated like any other
                massless = ref["src"][me][:, 9] == 0.0
                assert (np.linalg.norm(ref["w"][me]["acc"][massless], axis=1) > 0.0).all()
        units, flagged = np.concatenate(units), np.concatenate(flagged)
        assert len(units) == n
        worst = float(units[~flagged].max()) if (~flagged).any() else 0.0
        rows.append((name, n, world, flagged.mean(), worst))
        assert worst <= L.K_LET_REF, (name, worst)
        assert flagged.mean() <= 0.01, (name, flagged.mean())
        if n >= 1000:
            big += 1
            clean += int(not flagged.any())
    for name, n, world, share, worst in rows:    # (shown with `-s`: the table in let_ref.py's docstring)
        print(f"    {name:18s} {n:5d}  {world:5d}  {100.0 * share:5.3f} %  {worst:6.2f}")
    print(f"    K_LET_REF {L.K_LET_REF} (max measured {max(r[4] for r in rows):.2f}), K_LET {L.K_LET}")
    assert 2 * clean >= big, (clean, big)
    assert max(r[4] for r in rows) > L.K_LET_REF / 2.0     # the measured maximum rounded up, not a loose guess
    assert L.K_LET == max(T.K, 4.0 * L.K_LET_REF)


def _moves(ref, mutated):
    """The most any unflagged body of rank 0 (the mutations touch only what rank 0 walks) moves, in units, between
    let_walk64 and a mutated let_walk64."""
    theta, g, dt = ref["params"]
    nobody = dict(x_new=np.zeros((0, 3), dtype=np.float32), order=np.zeros(0, dtype=np.int64))
    only0 = [ref["ranks"][0]] + [nobody] * (len(ref["ranks"]) - 1)
    w2 = L.let_walk64(ref["trees"], ref["root_width"], only0, theta, g, E, dt, pair=mutated)[0]
    ok = ~ref["w"][0]["flagged"]
    return float(T.force_units(w2["acc"], ref["w"][0])[ok].max())


@pytest.mark.parametrize("name,q", [("uniform-4099x3", 1), ("dense-corex4", 3), ("uniform-65x8", 1)])
def test_a_mutated_reference_fails_the_bound(nb, name, q):
    """The size of the defects K_LET is meant to catch (as test_walk64_sees_a_dropped_cell): one rank's tree not
    walked, one remote cell walked with twice its size, the own-leaf skip applied to a remote tree -- each moves some
    unflagged body by more than K_LET units.  The mutations touch what rank 0 walks of rank q (dense-core: ranks 1 and 2
    lie inside the clump, and the upper cells of their trees are a chain of cells with one child, which give the same
    term opened or accepted)."""
    ref = reference(name)
    world = len(ref["trees"])
    empty = dict(acc=0.0, sum_abs=0.0, flagged=False, visits=0, accepts=0)

    def dropped(me, r, *args):             # rank q's tree never reaches rank 0
        return empty if (me, r) == (0, q) else L.walk_pair(me, r, *args)

    def skipping(me, r, tree, root_width, walker, theta, g, e, dt, delta):   # a remote leaf taken for the walker's own
        return T.walk64(tree, root_width, walker["order"], walker["x_new"], theta, g, e, dt, delta,
                        foreign=(r != me and (me, r) != (0, q)), lone=True)

    assert _moves(ref, dropped) > L.K_LET
    assert _moves(ref, skipping) > L.K_LET
    # a cell two to four levels below rank q's root that some body of rank 0 accepts with size / r in [theta / 2, theta):
    # at twice its size it is opened instead
    tree = ref["trees"][q]
    depth = T.tree_shape(tree)[1]
    most = 0.0
    for node in np.nonzero((depth >= 2) & (depth <= 4) & (tree["bodies"] > 1))[0][:40]:
        scale = np.ones(len(tree))
        scale[node] = 2.0

        def doubled(me, r, tree, root_width, walker, theta, g, e, dt, delta, scale=scale):
            return T.walk64(tree, root_width, walker["order"], walker["x_new"], theta, g, e, dt, delta,
                            foreign=(r != me), lone=True, size_scale=scale if (me, r) == (0, q) else None)

        most = max(most, _moves(ref, doubled))     # (0 where no body of rank 0 accepts that cell in that range)
        if most > L.K_LET:
            break
    assert most > L.K_LET or name == "uniform-65x8"      # (8 bodies a rank: no cell that deep holds two of them)
    assert world > 1
