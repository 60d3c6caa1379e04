"""A plain numpy, binary64 reference for the floating-point half of the Barnes-Hut step (test infrastructure only,
like diag_ref.py and radial_ref.py): the node moments of a given octree, a level-synchronous walk of it for all
bodies at once, and the tolerance a binary64 prefix difference rounded once to binary32 deserves.  The integer half
(tree, numbering, body order) is pinned bit for bit against the oracle elsewhere; nothing here rebuilds a tree.

Used by tests/test_tree_ref.py (this reference against the oracle, on the CPU), tests/test_tree_precision_gpu.py
(the kernels against this reference), tools/tree_fuzz.py and tests/let_ref.py (the multi-domain step: walk64 per pair
of ranks).

Measured on the CPU over CASES (tests/test_tree_ref.py prints the table with `-s`): the oracle's fp32 walk -- ~6
correctly rounded operations per term, a sequential sum -- against walk64 of the same tree, in units of
2^-24 x sum |term| per body, bodies flagged at delta = FLAG_DELTA aside; and the share of flagged bodies.

    case               n  flagged  worst body      case               n  flagged  worst body
    uniform-1          1  0         0.00           dense-core      6000  0        23.02
    uniform-2          2  0         2.77           wide-7.5        3000  0.067 %  16.27
    uniform-3          3  0         1.68           small-0.01      3000  0        12.42
    uniform-63        63  0         3.85           log-mass        3000  0        11.56
    uniform-65        65  0         4.17           tracers         2000  0.050 %   9.84
    uniform-257      257  0         6.41           massless-pocket 2000  0         8.30
    uniform-4099    4099  0         7.76
    spherical       3000  0.067 %  13.31
    disc            3000  0        12.26

(Medians are 1 .. 4.5 units.  In every case walk64's visit and accept counts equal the oracle's.)
K_REF is the maximum of the last column, rounded up; K = 4 K_REF is the bound for the GPU: its kernels use the
1-ulp v_rcp_f32 / v_sqrt_f32 and fused multiply-adds, two ulps per term more than the oracle's operations, and add
the terms in a different, partly pairwise order.  Neither figure is tuned on what the GPU gives.
"""
import numpy as np

from tests.helpers import DT, E, G, make_state

FLAG_DELTA = 4.0 * 2.0 ** -23     # an acceptance test this close to theta (relative) may go either way in fp32
K_REF = 24.0                      # worst oracle body over CASES: 23.02 units (dense-core)
K = 4.0 * K_REF                   # the GPU's bound, in units of 2^-24 x sum |term|
EPS32, EPS64 = 2.0 ** -24, 2.0 ** -52

# (name, kind, n, seed, theta, g, dt): the states are the product's host-side inits plus the edits of case_state.
# The seeds are chosen so that no case has more than 1 % of its bodies flagged and at least half of those of 1,000
# bodies or more have none -- a condition on the inputs, not on the code under test.
CASES = [
    ("uniform-1", "uniform", 1, 11, 0.5, G, DT), ("uniform-2", "uniform", 2, 12, 0.5, G, DT),
    ("uniform-3", "uniform", 3, 13, 0.5, G, DT), ("uniform-63", "uniform", 63, 14, 0.5, G, DT),
    ("uniform-65", "uniform", 65, 15, 0.5, G, DT), ("uniform-257", "uniform", 257, 16, 0.5, G, DT),
    # ragged for every group size (4, 8, 16), for 8 .. 64 bodies per wave and for the 256-thread workgroup
    ("uniform-4099", "uniform", 4099, 17, 0.5, G, DT),
    ("spherical", "spherical", 3000, 18, 0.3, G, DT),
    ("disc", "disc", 3000, 19, 0.75, 0.00001, 0.0016),
    ("dense-core", "uniform", 6000, 30, 0.5, G, DT),
    ("wide-7.5", "uniform", 3000, 21, 0.5, G, DT), ("small-0.01", "uniform", 3000, 22, 0.5, G, DT),
    ("log-mass", "uniform", 3000, 23, 0.5, G, DT),
    ("tracers", "uniform", 2000, 24, 0.5, G, DT),
    ("massless-pocket", "uniform", 2000, 25, 0.5, G, DT),
]
CASE_IDS = [c[0] for c in CASES]
MASSLESS = ("tracers", "massless-pocket")
POCKET_AT, POCKET_BODIES = (0.3, -0.2, 0.1), 40


def case_state(case):
    """float32[n, 10] source state of a case."""
    name, kind, n, seed, _theta, g, _dt = case
    s = make_state(kind, n, seed, g)
    rng = np.random.default_rng(seed)
    if name == "dense-core":      # the input of test_deep_clustered_tree_against_oracle (core 0.9, spread 3e-4), cut to 6,000
        k = int(0.9 * n)
        s[:k, 0:3] = (np.float32(0.3) + rng.normal(0.0, 3e-4, size=(k, 3))).astype(np.float32)
        s[:, 3:6] *= np.float32(0.01)
    elif name == "wide-7.5":
        s[:, 0:3] *= np.float32(7.5)
    elif name == "small-0.01":
        s[:, 0:3] *= np.float32(0.01)
    elif name == "log-mass":      # six decades: the range the binary64 prefix differences are good for
        s[:, 9] = (10.0 ** rng.uniform(-3.0, 3.0, size=n)).astype(np.float32)
    elif name == "tracers":
        s[1::2, 9] = 0.0
    elif name == "massless-pocket":   # whole internal cells of mass 0
        d2 = ((s[:, 0:3].astype(np.float64) - np.asarray(POCKET_AT)) ** 2).sum(1)
        s[np.argsort(d2, kind="stable")[:POCKET_BODIES], 9] = 0.0
    return s


# ---- moments ----------------------------------------------------------------------------------------------------

def tree_shape(tree):
    """parent, depth and leaf mask of every node.  A leaf has one body and is not the root (a lone body's root is
    an internal octant with one child); children carry larger ids than their parent."""
    n_nodes = len(tree)
    leaf = tree["bodies"] == 1
    leaf[0] = False
    ch = tree["children"].astype(np.int64)
    ch[leaf] = 0                    # (a leaf's children[0] names its body, not a node)
    parent = np.full(n_nodes, -1, dtype=np.int64)
    rows, cols = np.nonzero(ch)
    parent[ch[rows, cols]] = rows
    assert (parent[1:] >= 0).all() and (parent[1:] < np.arange(1, n_nodes)).all()
    depth = np.zeros(n_nodes, dtype=np.int64)
    todo = np.arange(1, n_nodes)    # (a parent's id is smaller: level by level from the root)
    known = np.zeros(n_nodes, dtype=bool)
    known[0] = True
    while len(todo):
        ready = known[parent[todo]]
        depth[todo[ready]] = depth[parent[todo[ready]]] + 1
        known[todo[ready]] = True
        todo = todo[~ready]
    return parent, depth, leaf


def sum_up(tree, leaf_values, shape=None):
    """Per node, the binary64 sum of `leaf_values[body]` (float64[n] or [n, k]) over the node's bodies: a leaf takes
    the value of body children[0], an internal node the sum of its children, added bottom-up level by level."""
    parent, depth, leaf = shape if shape is not None else tree_shape(tree)
    vals = np.asarray(leaf_values, dtype=np.float64)
    out = np.zeros((len(tree),) + vals.shape[1:], dtype=np.float64)
    out[leaf] = vals[tree["children"][leaf, 0]]
    for d in range(int(depth.max()) if len(depth) else 0, 0, -1):
        ids = np.nonzero(depth == d)[0]
        np.add.at(out, parent[ids], out[ids])
    return out


def moments64(tree, src):
    """tree: OCTANT_DTYPE array (read_tree's or the oracle's); src: the float32[n, 10] SOURCE state (leaves name
    their body by source index).  Returns dict(mass[n_nodes], mom[n_nodes, 3] -- the first moments sum m x --
    parent, depth, leaf)."""
    src = np.asarray(src, dtype=np.float32)
    shape = tree_shape(tree)
    x, m = src[:, 0:3].astype(np.float64), src[:, 9].astype(np.float64)
    both = sum_up(tree, np.concatenate([m[:, None] * x, m[:, None]], axis=1), shape)
    return dict(mass=both[:, 3], mom=both[:, 0:3], parent=shape[0], depth=shape[1], leaf=shape[2])


def moment_tolerance(mom, src):
    """(tol_mass[n_nodes], tol_cog[n_nodes, 3]) for a cell's mass and centre of gravity taken as differences of
    binary64 prefix sums over ALL bodies and rounded once to binary32 (nb_tree_cells.hpp 6a):
        2^-24 |v|                                    the one rounding to float, plus
        4 x 2^-52 x sum over all bodies of |m|       (mass), or of |m x_c| / m_cell  (cog, component c)
    the cancellation of the prefix difference -- the prefixes are as large as the whole problem's sums, whatever
    the cell holds.  Cells of mass 0 get a tolerance of 0 for the mass (a difference of equal prefixes)."""
    src = np.asarray(src, dtype=np.float32)
    x, m = src[:, 0:3].astype(np.float64), src[:, 9].astype(np.float64)
    all_m, all_mx = np.abs(m).sum(), np.abs(m[:, None] * x).sum(0)
    mass = mom["mass"]
    with np.errstate(invalid="ignore", divide="ignore"):
        cog = mom["mom"] / mass[:, None]
        tol_cog = EPS32 * np.abs(cog) + 4.0 * EPS64 * all_mx[None, :] / mass[:, None]
    tol_mass = EPS32 * np.abs(mass) + np.where(mass > 0.0, 4.0 * EPS64 * all_m, 0.0)
    return tol_mass, tol_cog


def check_moments(tree, src):
    """Every internal node of `tree` against moments64, per node and component; returns the worst ratio
    error / tolerance (mass, cog) for the record.  A massless cell: mass 0 and a NaN cog, as the reference has."""
    mom = moments64(tree, src)
    tol_m, tol_c = moment_tolerance(mom, src)
    internal = ~mom["leaf"]
    got_m, got_c = tree["mass"].astype(np.float64), tree["cog"].astype(np.float64)
    empty = internal & (mom["mass"] == 0.0)
    assert (got_m[empty] == 0.0).all() and np.isnan(got_c[empty]).all(), "a massless cell: mass 0, cog NaN"
    full = internal & ~empty
    with np.errstate(invalid="ignore", divide="ignore"):
        want_c = mom["mom"] / mom["mass"][:, None]
    err_m = np.abs(got_m - mom["mass"])[full]
    err_c = np.abs(got_c - want_c)[full]
    assert np.isfinite(err_m).all() and np.isfinite(err_c).all()
    worst_m = float((err_m / tol_m[full]).max()) if full.any() else 0.0
    worst_c = float((err_c / tol_c[full]).max()) if full.any() else 0.0
    bad = np.nonzero(err_m > tol_m[full])[0]
    assert not len(bad), ("mass", np.nonzero(full)[0][bad][:5], worst_m)
    bad = np.nonzero((err_c > tol_c[full]).any(1))[0]
    assert not len(bad), ("cog", np.nonzero(full)[0][bad][:5], worst_c)
    return worst_m, worst_c


# ---- walk -------------------------------------------------------------------------------------------------------

def walk64(tree, root_width, order, x_new, theta, g, e, dt, delta=FLAG_DELTA, bodies=None, chunk=2048,
           foreign=False, lone=False, size_scale=None):
    """The walk of tree.wgsl:41-90 (intended semantics: oracle flags = INTENDED) for all bodies at once, in
    binary64 from the binary32 cog and mass of the tree it is given; g, e, dt, theta widened from their fp32 values.
    x_new: the bodies' drifted positions in SORTED order (float32[n, 3]); order[k]: source index of sorted body k;
    bodies: the sorted positions to walk for (default: all).
    For the multi-domain step (tests/let_ref.py) -- the defaults are the single tree's walk:
      foreign: the walkers are not the tree's bodies (another rank's tree): no leaf is anybody's own, whatever
               children[0] it carries -- an index into ANOTHER set of bodies;
      lone:    walk also where there are fewer than two walkers (the shortcut below is the single tree's);
      size_scale[node]: factor on a cell's size in its acceptance test (tests of the tests: a mutated walk).
    Returns dict(acc[k, 3], sum_abs[k] -- the sum of the terms' Euclidean norms --, flagged[k] -- some internal cell
    had |size / r - theta| <= delta theta --, visits, accepts), rows in the order of `bodies`."""
    theta, g, e, dt = (float(np.float32(v)) for v in (theta, g, e, dt))
    n = len(x_new) if foreign else len(order)
    sel = np.arange(n) if bodies is None else np.asarray(bodies, dtype=np.int64)
    cog = tree["cog"].astype(np.float64)
    mass = tree["mass"].astype(np.float64)
    children = tree["children"].astype(np.int64)
    leaf = tree["bodies"] == 1
    leaf[0] = False
    self_src = np.where(leaf, children[:, 0], -1)
    x_all = np.asarray(x_new, dtype=np.float32).astype(np.float64)
    order = np.full(n, -2, dtype=np.int64) if foreign else np.asarray(order, dtype=np.int64)
    scale = None if size_scale is None else np.asarray(size_scale, dtype=np.float64)
    acc = np.zeros((len(sel), 3))
    sum_abs = np.zeros(len(sel))
    flagged = np.zeros(len(sel), dtype=bool)
    visits = accepts = 0
    # (a lone body feels nothing and nothing is walked for it: the oracle and the product alike -- the reference's
    # tree of one body is ill-formed)
    for c0 in range(0, len(sel) if n >= 2 or lone else 0, chunk):
        who = sel[c0:c0 + chunk]
        k = len(who)
        x, me = x_all[who], order[who]
        body = np.arange(k)                       # the frontier: (body, node, size) rows
        node = np.zeros(k, dtype=np.int64)
        size = np.full(k, float(np.float32(root_width)))
        a, sa, fl = np.zeros((k, 3)), np.zeros(k), np.zeros(k, dtype=bool)
        while len(body):
            visits += len(body)
            other = self_src[node] != me[body]    # a body's own leaf: visited, neither taken nor opened
            body, node, size = body[other], node[other], size[other]
            d = cog[node] - x[body]
            with np.errstate(invalid="ignore", divide="ignore"):
                r = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
                ratio = (size if scale is None else size * scale[node]) / r
                is_leaf = leaf[node]
                take = is_leaf | (ratio < theta)  # a comparison with NaN is false: the cell is opened
                close = ~is_leaf & (np.abs(ratio - theta) <= delta * theta)
                t = (mass[node] * g / (r * r * r + e))[:, None] * (d / r[:, None]) * dt
            fl[np.unique(body[close])] = True
            tb, tt = body[take], t[take]
            for comp in range(3):
                a[:, comp] += np.bincount(tb, weights=tt[:, comp], minlength=k)
            sa += np.bincount(tb, weights=np.sqrt((tt * tt).sum(1)), minlength=k)
            accepts += int(take.sum())
            body, node, size = body[~take], node[~take], size[~take]
            ch = children[node]
            has = ch != 0
            cnt = has.sum(1)
            body, size, node = np.repeat(body, cnt), np.repeat(size / 2.0, cnt), ch[has]
        acc[c0:c0 + k], sum_abs[c0:c0 + k], flagged[c0:c0 + k] = a, sa, fl
    return dict(acc=acc, sum_abs=sum_abs, flagged=flagged, visits=visits, accepts=accepts)


def force_units(got_acc, ref):
    """|got - walk64| per body in units of 2^-24 x sum |term| (0 where a body has no term at all)."""
    err = np.linalg.norm(np.asarray(got_acc, dtype=np.float64) - ref["acc"], axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(ref["sum_abs"] > 0.0, err / (EPS32 * ref["sum_abs"]), np.where(err == 0.0, 0.0, np.inf))


def kick32(v, a, dt):
    """kick() of nb_tree_wave.hpp / tree.wgsl:105,108 in numpy float32: one rounding per operation."""
    v, a = np.asarray(v, dtype=np.float32), np.asarray(a, dtype=np.float32)
    return v + (a * np.float32(dt)) / np.float32(2.0)
