"""A binary64 reference of ONE multi-domain Barnes-Hut step with locally essential trees (test infrastructure only, in
the style of tree_ref.py, whose moments, walk and units it uses as they are).

The method, from the header of csrc/nb_tree_let.hpp: every rank builds the octree of ITS bodies inside the GLOBAL root
cube; a body feels the sum over all ranks of a walk of that rank's tree; pruning an export never changes a decision.
That is tree_ref.walk64 applied `world` times per rank, the results added in binary64: let_walk64.  The domain cut is
host code tested elsewhere and enters as an input (domains), as the tree enters tree_ref.

Counting rule (walk_kernel / walk_cells_kernel count one visit per (body, record) a body's mask reaches and one accept
per term added; let_export_kernel / let_export_level_kernel): for every ordered pair (me, r) of ranks that BOTH hold
bodies, every body of `me` walks tree r from its root, and the counts are walk64's --
  * r != me: no leaf is the walker's own (imported records carry self_pos = ~0).  A pruned cell arrives as a terminal
    record: one visit, one accept -- what a body walking that rank's whole tree does with it, since every point of
    the walker's bounding box accepts it.  So pruned, whole-tree (tree_let_prune 0) and reference counts are equal;
  * r == me: walk64 with the own-leaf skip, a rank of ONE body included: the LET walk always starts at the own root
    (let_walk / let_walk_own push root 0 whenever the rank has a body; only the single-tree step takes own_root()'s
    "a lone body walks nothing"), so that body visits its root, opens it (it sits at the root's centre of gravity)
    and visits its own leaf: 2 visits, 0 accepts, no force;
  * a rank without bodies is nobody's root (let_set_imports / let_rebase_fixed_kernel skip segments of 0 records, and
    the exporters send an empty peer nothing) and walks nothing itself;
  * NB_PHASE_LET_WALK_OWN only splits the same walks over two launches; the counters add up to the same numbers.

Measured on the CPU over CASES (tests/test_let_ref.py prints the table with `-s`): per rank the oracle's fp32 walk of
every rank's tree, the per-tree results added in fp32 own tree first, against let_walk64 of the same trees, in units of
2^-24 x sum |term| per body, flagged bodies (delta = tree_ref.FLAG_DELTA) aside; and the share of flagged bodies.

    case                  n  world  flagged  worst body
    uniform-3x4            3      4  0          1.68
    uniform-65x8          65      8  0          4.06
    uniform-4099x2      4099      2  0          8.16
    uniform-4099x3      4099      3  0          7.21
    uniform-4099x8      4099      8  0          5.43
    sphericalx4         3000      4  0.067 %    9.93
    discx3              3000      3  0          8.11
    dense-corex4        6000      4  0.067 %    6.65
    wide-7.5x3          3000      3  0.067 %   10.71
    small-0.01x2        3000      2  0          9.34
    log-massx4          3000      4  0          9.81
    tracersx3           2000      3  0          7.62
    massless-pocketx4   2000      4  0          6.02

(In every unit-cube case let_walk64's visit and accept counts equal the oracle's per-pair walks added up.  The states and
seeds are tree_ref's; they meet its conditions here too: no case above 1 % flagged, 8 of the 11 cases of 1,000 bodies or
more with none.  The figures are lower than tree_ref's for the single tree because a body's sum is split into `world`
shorter fp32 sums.  The trees are the oracle's of each rank's bodies alone, whose cube is the global one in every case
but wide-7.5; there they are tree_in_cube's.)

K_LET_REF = 11 is the maximum of the last column, rounded up; K_LET = max(tree_ref.K, 4 K_LET_REF) = 96 is the bound for
the GPU, by tree_ref.py's argument (1-ulp rcp / sqrt and fused multiply-adds, a different and partly pairwise order of
the terms).  Neither figure is tuned on what the GPU gives.
"""
import numpy as np

from tests import tree_ref as T
from tests.tree_ref import FLAG_DELTA

K_LET_REF = 11.0                            # worst oracle body over CASES: 10.71 units (wide-7.5x3)
K_LET = max(T.K, 4.0 * K_LET_REF)           # the GPU's bound, in units of 2^-24 x sum |term|

# (name, base case of tree_ref.CASES, world): the smallest shapes at which each mechanism of the LET path is exercised
CASES = [
    ("uniform-3x4", "uniform-3", 4), ("uniform-65x8", "uniform-65", 8),     # ranks of 0 and 1 bodies; more ranks than waves
    ("uniform-4099x2", "uniform-4099", 2), ("uniform-4099x3", "uniform-4099", 3), ("uniform-4099x8", "uniform-4099", 8),
    ("sphericalx4", "spherical", 4),        # theta 0.3: deep exports, little is pruned
    ("discx3", "disc", 3),                  # thin Morton domains that interleave; the 150000-mass centre in one rank
    ("dense-corex4", "dense-core", 4),      # the cuts run through the clump: deep cells split between ranks
    ("wide-7.5x3", "wide-7.5", 3),          # a rank whose own max |coord| is below the global one
    ("small-0.01x2", "small-0.01", 2), ("log-massx4", "log-mass", 4), ("tracersx3", "tracers", 3),
    ("massless-pocketx4", "massless-pocket", 4),   # massless cells (NaN cog) through the export's box test
]
CASE_IDS = [c[0] for c in CASES]
UNIT_CUBE = [c[0] for c in CASES if c[1] != "wide-7.5"]


def base_case(case):
    return T.CASES[T.CASE_IDS.index(case[1])]


def domains(state, world, with_owners=False):
    """Rank -> source indices, as wgpu_n_body_amd.sharded.morton_domains cuts them (with_owners: also splits, ref_bound)."""
    from wgpu_n_body_amd.sharded import morton_domains
    order, cuts, splits, ref_bound = morton_domains(np.ascontiguousarray(state, dtype=np.float32), world, with_owners=True)
    dom = [np.asarray(order[cuts[r]:cuts[r + 1]], dtype=np.int64) for r in range(world)]
    return (dom, splits, ref_bound) if with_owners else dom


def drift32(src, dt):
    """The walk's evaluation points, float32[n, 3]: kick + drift with one rounding per operation."""
    src = np.asarray(src, dtype=np.float32)
    return src[:, 0:3] + T.kick32(src[:, 3:6], src[:, 6:9], dt) * np.float32(dt)


def global_root_width(state):
    """2 x max(1, max |coord| over ALL bodies), in float32 like the meta words."""
    return np.float32(2.0) * max(np.float32(1.0), np.abs(np.asarray(state, dtype=np.float32)[:, 0:3]).max())


def tree_in_cube(src, root_width, max_depth=64):
    """The breadth-first octree of `src` (float32[n, 10], n >= 1) in the cube of width `root_width` about the origin --
    the oracle's nbo_tree_build (tree.rs:458-546: octant bit c set where x_c > centre_c, children numbered in queue
    order, a cell of one body a leaf naming it in children[0]) with the cube GIVEN instead of taken from the bodies,
    which the oracle cannot do.  bodies and children are the oracle's bit for bit where the cubes agree
    (tests/test_let_ref.py); mass and cog of the internal cells are binary64 sums rounded once.  For the case whose
    ranks do not span the global cube, on the CPU."""
    from oracle.oracle import OCTANT_DTYPE
    src = np.asarray(src, dtype=np.float32)
    n = len(src)
    x, m = src[:, 0:3], src[:, 9].astype(np.float64)
    mx = m[:, None] * x.astype(np.float64)
    nodes = [np.zeros(1, dtype=OCTANT_DTYPE)]
    n_nodes = 1
    # the level's open cells, in queue order: node id, centre, and their bodies grouped by cell in index order
    cell_node, cell_centre = np.zeros(1, dtype=np.int64), np.zeros((1, 3), dtype=np.float32)
    body, body_cell = np.arange(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    width = np.float32(root_width)
    for _depth in range(max_depth + 1):
        if not len(cell_node):
            break
        c = cell_centre[body_cell]
        octant = ((x[body, 0] > c[:, 0]).astype(np.int64) | ((x[body, 1] > c[:, 1]).astype(np.int64) << 1)
                  | ((x[body, 2] > c[:, 2]).astype(np.int64) << 2))
        key = body_cell * 8 + octant
        cnt = np.bincount(key, minlength=8 * len(cell_node))
        used = np.nonzero(cnt)[0]                        # the children, in allocation order
        child_id = np.zeros(len(cnt), dtype=np.int64)
        child_id[used] = n_nodes + np.arange(len(used))
        # this level's cells
        cells = np.concatenate(nodes)
        m_cell = np.bincount(body_cell, weights=m[body], minlength=len(cell_node))
        with np.errstate(invalid="ignore", divide="ignore"):
            for comp in range(3):
                cells["cog"][cell_node, comp] = np.bincount(body_cell, weights=mx[body, comp], minlength=len(cell_node)) / m_cell
        cells["mass"][cell_node] = m_cell
        cells["bodies"][cell_node] = np.bincount(body_cell, minlength=len(cell_node))
        cells["children"][cell_node] = child_id.reshape(-1, 8)
        # the children: leaves now, cells of two or more bodies at the next level
        new = np.zeros(len(used), dtype=OCTANT_DTYPE)
        order = np.argsort(key, kind="stable")
        body, key = body[order], key[order]
        single = cnt[key] == 1
        at = child_id[key[single]] - n_nodes
        new["cog"][at], new["mass"][at], new["bodies"][at] = x[body[single]], src[body[single], 9], 1
        new["children"][at, 0] = body[single]
        nodes = [cells, new]
        n_nodes += len(used)
        opened = used[cnt[used] > 1]
        quarter = width / np.float32(4.0)
        sign = np.stack([(opened & 1), (opened >> 1) & 1, (opened >> 2) & 1], axis=1).astype(np.float32) * np.float32(2.0) - np.float32(1.0)
        cell_centre = cell_centre[opened // 8] + sign * quarter
        cell_node = child_id[opened]
        renumber = np.full(len(cnt), -1, dtype=np.int64)
        renumber[opened] = np.arange(len(opened))
        body, body_cell = body[~single], renumber[key[~single]]
        width = width / np.float32(2.0)
    else:
        raise RuntimeError("tree_in_cube: deeper than max_depth (coincident bodies)")
    return np.concatenate(nodes)


def walk_pair(me, r, tree, root_width, walker, theta, g, e, dt, delta):
    """Rank `me`'s bodies walking rank r's tree."""
    return T.walk64(tree, root_width, walker["order"], walker["x_new"], theta, g, e, dt, delta,
                    foreign=(r != me), lone=True)


def let_walk64(trees, root_width, ranks, theta, g, e, dt, delta=FLAG_DELTA, pair=walk_pair):
    """trees[r]: OCTANT_DTYPE tree of rank r in the global cube (None or empty: the rank holds no body);
    ranks[me]: dict(x_new = rank me's drifted positions in ITS sorted order, float32[n_me, 3]; order[k] = index of
    sorted body k among the rank's own bodies -- what the leaves of trees[me] name).
    Returns one dict(acc, sum_abs, flagged, visits, accepts) per rank -- tree_ref.walk64's, added over the trees in
    binary64; rows in the rank's sorted order.  `pair` is replaced only by the tests that mutate the reference."""
    out = []
    for me, walker in enumerate(ranks):
        n = len(walker["x_new"])
        tot = dict(acc=np.zeros((n, 3)), sum_abs=np.zeros(n), flagged=np.zeros(n, dtype=bool), visits=0, accepts=0)
        for r, tree in enumerate(trees):
            if n == 0 or tree is None or len(tree) == 0:
                continue
            w = pair(me, r, tree, root_width, walker, theta, g, e, dt, delta)
            tot["acc"] += w["acc"]
            tot["sum_abs"] += w["sum_abs"]
            tot["flagged"] |= w["flagged"]
            tot["visits"] += w["visits"]
            tot["accepts"] += w["accepts"]
        out.append(tot)
    return out


def totals(per_rank):
    return sum(w["visits"] for w in per_rank), sum(w["accepts"] for w in per_rank)
