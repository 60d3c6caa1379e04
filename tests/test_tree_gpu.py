"""Barnes-Hut parity on a real MI355X, through the C ABI -- `-m gpu`.

Hot path under test: nb_sim_encode on a TreeSim (nb_tree.hip + nb_tree_*.hpp): bound, Morton keys, radix sort,
reorder, octree build, mass/cog, tree walk + integrator -- the device replacement for
TreeSim::encode (src/sims/tree.rs:262-353) + build_tree/sort_particles (tree.rs:417-602) +
shaders/tree.wgsl:41-111.

What must hold, against the CPU oracle (oracle/nbody_oracle_tree.c, flags = INTENDED):
  * integer/index work BIT-EXACT: node count, every node's `bodies` and `children[8]` (the
    reference's BFS allocation numbering), the DFS body order, root_width;
  * float fields of the tree within fp32 summation tolerance (the reference sums a cell's
    bodies sequentially, the GPU sums children hierarchically): mass rel 2e-5, cog abs 2e-5;
  * positions after ONE step bit-identical to the oracle (literal integrator lines);
  * accelerations: the per-lane walk visits the same nodes in the same order as the
    reference's per-thread walk, so errors are at fp32 rounding level (median < 1e-5) -- except
    where an acceptance test size/dist < theta sits within an ulp of theta and flips ("MAC
    flip"), which changes one body's force by at most the Barnes-Hut approximation error:
    99 % of bodies within 1e-4 relative, all within 5e-2;
  * walk statistics (nodes visited / accepted) within 1e-5 of the oracle's counts.
"""
import glob
import os

import numpy as np
import pytest

from tests.helpers import DT, E, G, GOLDEN, bits, make_state

pytestmark = pytest.mark.gpu


def run_tree(nb, state, theta, steps=1, g=G, e=E, dt=DT, count=True, tuning=None):
    sp = nb.SimParams(particle_num=len(state), g=g, e=e, dt=dt)
    sim = nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(theta), state)
    for key, value in (tuning or {}).items():
        sim.set_tuning(key, value)
    if count:
        sim.set_tuning("tree_count_visits", 1)
    for _ in range(steps):
        sim.encode()
        sim.cleanup()
    sim.wait()
    out = nb.as_floats(sim.dest_particle_slice()).copy()
    tree, rw = sim.read_tree()
    res = dict(dst=out, tree=tree, root_width=rw, order=sim.debug_buffer("order", np.uint32),
               counters=sim.debug_buffer("counters", np.uint64),
               status=sim.debug_buffer("status", np.uint32))
    sim.destroy()
    return res


def rel_err(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.linalg.norm(a - b, axis=1) / np.maximum(np.linalg.norm(b, axis=1), 1e-300)


def check_tree(got_tree, got_rw, got_order, ref_tree, ref_rw, ref_order, extent=1.0):
    """extent: max |coordinate| where it exceeds 1 (the cog tolerance is fp32 rounding of the coordinates)."""
    assert got_rw == np.float32(ref_rw)
    assert len(got_tree) == len(ref_tree)
    assert np.array_equal(got_order, ref_order)                        # DFS / Morton order
    assert np.array_equal(got_tree["bodies"], ref_tree["bodies"])      # bit-exact
    assert np.array_equal(got_tree["children"], ref_tree["children"])  # bit-exact, BFS numbering
    mscale = ref_tree["mass"].max()
    assert np.abs(got_tree["mass"] - ref_tree["mass"]).max() <= 2e-5 * mscale
    assert np.abs(got_tree["cog"] - ref_tree["cog"]).max() <= 2e-5 * max(1.0, extent)
    leaves = ref_tree["bodies"] == 1
    leaves[0] = False    # (a lone body's root is an internal octant: its cog is m x / m, rounded where the sums are)
    assert np.array_equal(bits(got_tree["cog"][leaves]), bits(ref_tree["cog"][leaves]))
    assert np.array_equal(bits(got_tree["mass"][leaves]), bits(ref_tree["mass"][leaves]))


def check_step(got, ref_dst, one_step=True):
    assert np.isfinite(got).all()
    if one_step:
        assert np.array_equal(bits(got[:, 0:3]), bits(ref_dst[:, 0:3]))
    assert np.array_equal(got[:, 9], ref_dst[:, 9])
    r = rel_err(got[:, 6:9], ref_dst[:, 6:9])
    assert np.median(r) < 1e-5, np.median(r)
    assert np.percentile(r, 99) < 1e-4, np.percentile(r, 99)
    assert r.max() < 5e-2, r.max()


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "tree_*.npz"))))
def test_golden_fixtures(gpu, path):
    z = np.load(path)
    g, e, dt, theta = (float(x) for x in z["params"])
    r = run_tree(gpu, z["init"], theta, 1, g, e, dt)
    assert not r["status"].any()
    check_tree(r["tree"], r["root_width"], r["order"], z["tree"], z["root_width"], z["order"])
    check_step(r["dst"], z["dst_intended"])
    visits, accepted = (int(x) for x in z["stats_intended"][:2])
    assert abs(int(r["counters"][0]) - visits) <= max(2, 1e-5 * visits)
    assert abs(int(r["counters"][1]) - accepted) <= max(2, 1e-5 * accepted)
    # the literal (defective) tree.wgsl walk is NOT what the GPU implements (in the disc
    # fixture the 150000-mass centre dominates every force, so the defects barely show)
    lit = rel_err(r["dst"][:, 6:9], z["dst_literal"][:, 6:9])
    if "disc" not in os.path.basename(path):
        assert np.median(lit) > 0.1
    # 4 chained steps (each step re-sorts the bodies, as the reference does)
    r4 = run_tree(gpu, z["init"], theta, 4, g, e, dt)
    ref4 = z["dst_intended_step4"]
    assert np.abs(r4["dst"][:, 0:3] - ref4[:, 0:3]).max() < 1e-6
    r = rel_err(r4["dst"][:, 6:9], ref4[:, 6:9])
    assert np.median(r) < 1e-4 and np.percentile(r, 99) < 5e-2


@pytest.mark.parametrize("kind,n,theta,g,dt", [
    ("uniform", 1, 0.5, G, DT), ("uniform", 2, 0.5, G, DT), ("uniform", 3, 0.5, G, DT), ("uniform", 63, 0.75, G, DT),
    ("uniform", 65, 0.5, G, DT), ("spherical", 257, 0.3, G, DT), ("uniform", 4096, 0.5, G, DT),
    ("spherical", 5000, 0.75, G, DT), ("disc", 3000, 0.75, 0.00001, 0.0016),
    ("uniform", 20000, 1.0, G, DT)])
def test_tree_and_step_against_oracle(gpu, oracle, kind, n, theta, g, dt):
    s = make_state(kind, n, 500 + n, g)
    ref = oracle.tree_step_f32(s, g, E, dt, theta, flags=oracle.INTENDED)
    r = run_tree(gpu, s, theta, 1, g, E, dt)
    assert not r["status"].any()
    check_tree(r["tree"], r["root_width"], r["order"], ref["tree"], ref["root_width"], ref["order"])
    check_step(r["dst"], ref["dst"])
    assert abs(int(r["counters"][0]) - ref["stats"]["visits"]) <= max(2, 1e-5 * ref["stats"]["visits"])


# every shape of the walk: cells across the lanes with 4 / 8 / 16 bodies per wave (mode 1, the
# default is 8), and bodies across the lanes with 8 ... 64 bodies per wave (mode 0)
WALK_SHAPES = [{"tree_walk_mode": 1, "tree_walk_group": 4}, {"tree_walk_mode": 1, "tree_walk_group": 8},
               {"tree_walk_mode": 1, "tree_walk_group": 16},
               # two-word stack entries (what problems whose cell ids need more than 24 bits take)
               {"tree_walk_mode": 1, "tree_walk_group": 8, "tree_walk_packed": 0},
               {"tree_walk_mode": 1, "tree_walk_group": 4, "tree_walk_packed": 0},
               {"tree_walk_mode": 0, "tree_walk_bpw": 8}, {"tree_walk_mode": 0, "tree_walk_bpw": 16},
               {"tree_walk_mode": 0, "tree_walk_bpw": 32}, {"tree_walk_mode": 0, "tree_walk_bpw": 64}]


@pytest.mark.parametrize("kind,n,theta,g,dt", [("uniform", 4096, 0.5, G, DT), ("spherical", 5003, 0.75, G, DT),
                                               ("disc", 3000, 0.75, 0.00001, 0.0016), ("uniform", 67, 0.5, G, DT)])
def test_every_walk_shape_against_oracle(gpu, oracle, kind, n, theta, g, dt):
    """All lanes, masks and group sizes of both walk kernels against the oracle: forces within the
    fp32 tolerances of check_step, visit / accept counts equal to the oracle's per-thread walk,
    and the integer work (tree, order, positions) bit-identical across the shapes."""
    s = make_state(kind, n, 900 + n, g)
    ref = oracle.tree_step_f32(s, g, E, dt, theta, flags=oracle.INTENDED)
    first, by_shape = None, []
    for shape in WALK_SHAPES:
        r = run_tree(gpu, s, theta, 1, g, E, dt, tuning=shape)
        by_shape.append(r["dst"])
        assert not r["status"].any(), shape
        check_step(r["dst"], ref["dst"])
        assert abs(int(r["counters"][0]) - ref["stats"]["visits"]) <= max(2, 1e-5 * ref["stats"]["visits"]), shape
        assert abs(int(r["counters"][1]) - ref["stats"]["accepted"]) <= max(2, 1e-5 * ref["stats"]["accepted"]), shape
        if first is None:
            first = r
        else:
            assert np.array_equal(r["order"], first["order"])
            assert np.array_equal(bits(r["dst"][:, 0:3]), bits(first["dst"][:, 0:3]))
            # the shapes add the same terms in different orders: fp32 rounding apart
            scale = np.abs(first["dst"][:, 6:9]).max()
            assert np.abs(r["dst"][:, 6:9] - first["dst"][:, 6:9]).max() <= 3e-6 * scale, shape
    # (one-word and two-word stack entries are the same traversal with stacks of different depth -- 1,024 and 896
    # entries: a batch is narrowed when the stack is nearly full, so the two add the same terms in different orders
    # where a walk fills its stack; everything else of the step is bit for bit the same, checked above)


@pytest.mark.parametrize("core,spread", [(0.5, 2e-3), (0.9, 3e-4)])
def test_deep_clustered_tree_against_oracle(gpu, oracle, core, spread):
    """A dense core inside a sparse halo: a tree 14+ levels deep whose frontier is far wider than
    on uniform data (the reference's fixed 64-entry stack overflows on this kind of input, SURVEY
    A14 D3).  Exercises the walk's stack discipline -- batch width limited by the free space, down
    to single-cell depth-first batches -- and the build on long common key prefixes."""
    nb = gpu
    n = 24000
    rng = np.random.default_rng(7)
    s = make_state("uniform", n, 321)
    k = int(core * n)
    s[:k, 0:3] = (np.float32(0.3) + rng.normal(0.0, spread, size=(k, 3))).astype(np.float32)
    s[:, 3:6] *= np.float32(0.01)
    ref = oracle.tree_step_f32(s, G, E, DT, 0.5, flags=oracle.INTENDED)
    depth_proxy = ref["stats"]["high_water"]
    assert depth_proxy > 40                       # far beyond the uniform case (~22 at this size)
    for shape in ({"tree_walk_mode": 1, "tree_walk_group": 8}, {"tree_walk_mode": 1, "tree_walk_group": 16},
                  {"tree_walk_mode": 0}):
        r = run_tree(gpu, s, 0.5, 1, tuning=shape)
        assert not r["status"].any(), shape
        check_tree(r["tree"], r["root_width"], r["order"], ref["tree"], ref["root_width"], ref["order"])
        assert np.isfinite(r["dst"]).all()
        assert np.array_equal(bits(r["dst"][:, 0:3]), bits(ref["dst"][:, 0:3]))
        # (inside the core a body's force is a sum of large, nearly cancelling neighbour terms: the
        # order of summation shows at a few 1e-5 -- in the oracle's sequential fp32 sum as well)
        err = rel_err(r["dst"][:, 6:9], ref["dst"][:, 6:9])
        assert np.median(err) < 2e-4 and np.percentile(err, 99) < 5e-3 and err.max() < 5e-2, (shape, np.median(err))
        assert abs(int(r["counters"][0]) - ref["stats"]["visits"]) <= max(2, 1e-5 * ref["stats"]["visits"]), shape
        assert abs(int(r["counters"][1]) - ref["stats"]["accepted"]) <= max(2, 1e-5 * ref["stats"]["accepted"]), shape


def test_bodies_outside_the_unit_cube_scale_the_root(gpu, oracle):
    s = make_state("uniform", 2000, 61)
    s[:, 0:3] *= 7.5          # bound = max |coord| > 1 -> root_width = 2 * bound (tree.rs:446-451)
    ref = oracle.tree_step_f32(s, G, E, DT, 0.5)
    r = run_tree(gpu, s, 0.5)
    assert r["root_width"] == np.float32(ref["root_width"]) and r["root_width"] > 14
    check_tree(r["tree"], r["root_width"], r["order"], ref["tree"], ref["root_width"], ref["order"])
    check_step(r["dst"], ref["dst"])


def test_theta_to_zero_degenerates_to_all_pairs(gpu, oracle):
    """With theta -> 0 every cell is opened and every leaf is a body: the result must equal
    the all-pairs step (same integrator, summation order differs)."""
    s = make_state("uniform", 1500, 62)
    r = run_tree(gpu, s, 1e-6)
    ap = oracle.naive_step_f32(s, G, E, DT)[r["order"]]
    assert np.array_equal(bits(r["dst"][:, 0:3]), bits(ap[:, 0:3]))
    scale = np.abs(ap[:, 6:9]).max()
    assert np.abs(r["dst"][:, 6:9] - ap[:, 6:9]).max() / scale < 2e-5
    n = 1500
    assert int(r["counters"][1]) == n * (n - 1)          # every other body accepted exactly once


def test_default_theta_and_runner(gpu, oracle):
    """TreeSim::new with no TreeSimParams falls back to theta 0.75 (tree.rs:42-51)."""
    nb = gpu
    sp = nb.SimParams(particle_num=1000)
    init = nb.inits.uniform_init(sp, seed=63)
    runner = nb.OfflineHeadless(nb.TreeSim, sp, nb.AddParams.NaiveSimParams(),
                                lambda p: nb.inits.uniform_init(p, seed=63))
    runner.step()
    got = nb.as_floats(runner.read_particles())
    ref = oracle.tree_step_f32(nb.as_floats(init), sp.g, sp.e, sp.dt, 0.75)
    check_step(got, ref["dst"])
    tree, rw = runner.sim.read_tree()
    assert len(tree) == len(ref["tree"])
    runner.destroy()


def test_tree_sim_is_deterministic_and_restorable(gpu):
    nb = gpu
    s = make_state("spherical", 3000, 64)
    a = run_tree(nb, s, 0.5, 3)["dst"]
    b = run_tree(nb, s, 0.5, 3)["dst"]
    assert np.array_equal(bits(a), bits(b))


def test_accuracy_against_all_pairs_at_16k(gpu):
    """End-to-end physics check on the GPU alone: Barnes-Hut vs the all-pairs simulator."""
    nb = gpu
    n = 16384
    s = make_state("uniform", n, 65)
    r = run_tree(nb, s, 0.5)
    sp = nb.SimParams(particle_num=n)
    sim = nb.NaiveSim.from_particles(sp, None, s)
    sim.encode()
    ap = nb.as_floats(sim.dest_particle_slice())[r["order"]]
    sim.destroy()
    err = rel_err(r["dst"][:, 6:9], ap[:, 6:9])
    assert np.median(err) < 0.03 and np.percentile(err, 95) < 0.10
    assert np.array_equal(bits(r["dst"][:, 0:3]), bits(ap[:, 0:3]))


# ---- BASELINE.json configs[2] size: 1,048,576 bodies, theta 0.5 -------------------------------

def test_full_size_tree_invariants_and_sampled_walk(gpu, oracle):
    nb = gpu
    n = 1 << 20
    s = make_state("uniform", n, 3)
    r = run_tree(nb, s, 0.5)
    assert not r["status"].any()
    tree, order = r["tree"], r["order"]
    # the DFS order is a permutation; leaves are in bijection with bodies
    assert np.array_equal(np.sort(order), np.arange(n, dtype=np.uint32))
    leaves = tree["bodies"] == 1
    assert leaves.sum() == n
    assert np.array_equal(np.sort(tree["children"][leaves, 0]), np.arange(n, dtype=np.uint32))
    assert not tree["children"][leaves, 1:].any()
    assert tree["bodies"][0] == n
    # every internal node: bodies = sum over children, children ids contiguous and increasing
    internal = np.nonzero(~leaves)[0]
    ch = tree["children"][internal]
    cb = np.where(ch > 0, tree["bodies"][ch], 0)
    assert np.array_equal(cb.sum(1), tree["bodies"][internal])
    first = np.where(ch > 0, ch, np.iinfo(np.uint32).max).min(1)
    cnt = (ch > 0).sum(1)
    last = ch.max(1)
    assert np.array_equal(last - first + 1, cnt) and (first > internal).all()
    # mass conservation at the root; node count ~1.5 N
    assert tree["mass"][0] == pytest.approx(float(n), rel=1e-5)
    assert 1.3 * n < len(tree) < 1.7 * n
    # the oracle builds the same tree (serial BFS, a few seconds) and walks a window of bodies
    ref_tree, ref_rw = oracle.tree_build(s)
    assert len(ref_tree) == len(tree) and r["root_width"] == np.float32(ref_rw)
    assert np.array_equal(ref_tree["bodies"], tree["bodies"])
    assert np.array_equal(ref_tree["children"], tree["children"])
    assert np.array_equal(oracle.tree_dfs_order(ref_tree, n), order)
    # ... and the FORCES at this size (depth >= 10, ~1,000 cells per body, the XCD remap, full
    # stacks): the oracle's per-thread walk (tree.wgsl:41-90, intended semantics) over windows of
    # the sorted bodies at the start, in the middle and at the end, against the bit-identical tree
    sorted_src = s[order]
    for start in (0, n // 2 - 128, n - 256):
        sel = np.arange(start, start + 256)
        want, stats = oracle.tree_walk_window(sorted_src, ref_tree, ref_rw, G, E, DT, 0.5, start, start + 256, order)
        got = r["dst"][sel]
        assert np.array_equal(bits(got[:, 0:3]), bits(want[:, 0:3]))
        err = rel_err(got[:, 6:9], want[:, 6:9])
        assert np.median(err) < 1e-5 and np.percentile(err, 99) < 1e-4 and err.max() < 5e-2, (start, err.max())
    # visit / accept totals of the whole problem against the oracle's walk of a 1/64 sample,
    # scaled (the walk statistics are homogeneous on uniform data): within 2 %
    sample = np.arange(0, n, 64)
    _w, st = oracle.tree_walk_indices(sorted_src, ref_tree, ref_rw, G, E, DT, 0.5, sample, order)
    assert abs(int(r["counters"][0]) / n - st["visits"] / len(sample)) < 0.02 * st["visits"] / len(sample)
    assert abs(int(r["counters"][1]) / n - st["accepted"] / len(sample)) < 0.02 * st["accepted"] / len(sample)


@pytest.mark.parametrize("n,world,mode", [(5000, 2, "tree"), (3000, 3, "tree-overlap"),
                                          (6000, 2, "tree-overlap")])
def test_sharded_tree_sim_ranks_on_one_gpu(gpu, tmp_path, n, world, mode):
    """Multi-GPU Barnes-Hut, step 1 of SURVEY 8(e): replicated tree, partitioned walk, three
    in-place all-gathers (ShardedTreeSim).  `world` processes share this one GPU with gloo
    standing in for RCCL; every rank must end with the single simulator's state, bit for bit."""
    import socket
    import subprocess
    import sys
    from tests.helpers import ROOT
    nb = gpu
    steps = 3
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    from tests.helpers import run_workers
    run_workers([[sys.executable, os.path.join(ROOT, "tests", "_gpu_shard_worker.py"), str(tmp_path), str(n),
                  str(steps), mode]] * world, port, tmp_path)
    sp = nb.SimParams(particle_num=n)
    single = nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(0.5),
                                       nb.inits.uniform_init(sp, seed=77))
    for _ in range(steps):
        single.encode()
    want = nb.as_floats(single.dest_particle_slice())
    single.destroy()
    for rank in range(world):
        z = np.load(os.path.join(tmp_path, f"gpu_rank{rank}.npz"))
        assert np.array_equal(bits(z["state"]), bits(want)), rank


def test_many_fresh_tree_sims_are_consistent(gpu):
    """Regression guard against order/initialisation dependence in the ~40-kernel build: many
    simulators of varying size in one process (allocator reuse, stale device memory); with unit
    masses every cell's mass must equal its body count exactly, and a repeat must be bit-equal."""
    nb = gpu
    rng = np.random.default_rng(5)
    keep = []
    for it in range(14):
        n = int(rng.integers(1500, 70000))
        sp = nb.SimParams(particle_num=n)
        init = nb.inits.uniform_init(sp, seed=900 + it)
        outs = []
        for rep in range(2):
            sim = nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(0.5), init)
            if rep == 1:
                sim.set_tuning("tree_use_graph", 1)     # the hipGraph replay must equal eager launches
            sim.encode()
            sim.encode()
            sim.wait()
            tree, _ = sim.read_tree()
            outs.append(sim.dest_particle_slice().copy())
            assert not sim.debug_buffer("status", np.uint32).any()
            assert np.array_equal(tree["mass"], tree["bodies"].astype(np.float32)), (it, rep, n)
            if rep == 0 and it % 3 == 0:
                keep.append(sim)
            else:
                sim.destroy()
            if len(keep) > 2:
                keep.pop(0).destroy()
        assert np.array_equal(outs[0], outs[1]), (it, n)
    for s in keep:
        s.destroy()


def test_graph_captured_after_an_eager_step_survives_a_new_state(gpu):
    """A hipGraph captured after an eager step takes the root cube from the slots the previous walk
    filled and holds no bound_kernel.  nb_sim_write_particles (snapshot resume, re-init) must drop it:
    replayed on a state 7.5x as wide it would key every body in the old cube.  Against a fresh
    simulator on the same state, bit for bit."""
    nb = gpu
    n = 20000
    sp = nb.SimParams(particle_num=n)
    first = nb.inits.uniform_init(sp, seed=41)
    wide = nb.as_floats(nb.inits.uniform_init(sp, seed=42)).copy()
    wide[:, 0:3] *= np.float32(7.5)
    sim = nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(0.5), first)
    sim.encode(); sim.wait()                       # eager: the walk leaves the next root cube
    sim.set_tuning("tree_use_graph", 1)
    sim.encode(); sim.wait()                       # captured without bound_kernel
    sim.write_particles(wide)
    sim.encode(); sim.encode(); sim.wait()
    got = sim.dest_particle_slice().copy()
    _, rw = sim.read_tree()
    assert not sim.debug_buffer("status", np.uint32).any()
    sim.destroy()
    ref = nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(0.5), wide)
    ref.encode(); ref.encode(); ref.wait()
    want = ref.dest_particle_slice().copy()
    _, rw_ref = ref.read_tree()
    ref.destroy()
    assert rw == rw_ref and rw > 7.0
    assert np.array_equal(got, want)


def test_clustered_input_cannot_overflow_the_build(gpu):
    """Pairs of nearly coincident bodies open ~20 single-child cells each: far more internal
    cells than the reference's 4N-node capacity (tree.rs:188-190, where the reference panics).
    The build must stay in bounds and report it -- from nb_sim_wait already (a caller that only
    steps and never reads back must see it too), not fault."""
    nb = gpu
    n = 4096
    s = make_state("uniform", n, 77)
    s[1::2, 0:3] = s[0::2, 0:3] + np.float32(3e-7)       # every body gets a twin 3e-7 away
    sp = nb.SimParams(particle_num=n)
    sim = nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(0.5), s)
    sim.encode()
    with pytest.raises(nb.NBodyError) as ei:
        sim.wait()
    assert "nodes" in str(ei.value) or "Morton key" in str(ei.value)
    status = sim.debug_buffer("status", np.uint32)
    assert status.any()
    with pytest.raises(nb.NBodyError):
        sim.read_tree()
    sim.destroy()


def test_more_than_eight_bodies_on_one_key_are_reported(gpu):
    """Twelve bodies inside one cell of the finest level (closer than root_width / 2^21): the
    reference's build_tree recurses on them until its node buffer overflows (tree.rs:473-544);
    here the step completes in bounds and every entry point that waits reports it -- the runner's
    step, the timing loop and the read-back alike -- instead of silently dropping sources."""
    nb = gpu
    n = 2048
    s = make_state("uniform", n, 78)
    s[100:112, 0:3] = s[100, 0:3] + (np.arange(12, dtype=np.float32)[:, None] * np.float32(1e-9))
    sp = nb.SimParams(particle_num=n)
    runner = nb.OfflineHeadless(nb.TreeSim, sp, nb.AddParams.TreeSimParams(0.5), lambda p: s)
    with pytest.raises(nb.NBodyError) as ei:
        runner.step()
    assert "Morton key" in str(ei.value)
    with pytest.raises(nb.NBodyError):
        runner.sim.encode_n_timed(2)
    with pytest.raises(nb.NBodyError):
        runner.read_particles()
    runner.destroy()


def test_tree_step_in_two_phases(gpu):
    """nb_sim_encode_phase on a TreeSim: phase 0 (sort + build, positions only) then phase 1
    (walk) is the same step as encode(), bit for bit; a second phase 0 in a row is an error."""
    nb = gpu
    s = make_state("uniform", 4000, 71)
    sp = nb.SimParams(particle_num=4000)
    a = nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(0.5), s)
    b = nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(0.5), s)
    for _ in range(3):
        a.encode()
        b.encode_phase(0)
        b.encode_phase(1)
    assert b.step_num() == 3
    assert np.array_equal(a.dest_particle_slice(), b.dest_particle_slice())
    b.encode_phase(0)
    with pytest.raises(nb.NBodyError):
        b.encode_phase(0)
    b.encode()                       # completes the step whose first half is pending
    a.encode()
    assert np.array_equal(a.dest_particle_slice(), b.dest_particle_slice())
    a.destroy()
    b.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("n,init", [(20000, "uniform"), (20000, "disc"), (100000, "uniform"), (100000, "disc"),
                                    (600000, "uniform"), (600000, "disc")])
def test_high_digit_sort_with_fix_up_gives_the_stable_key_order(gpu, n, init):
    """Above 12,288 bodies the radix sort covers only the high key bits (3 passes of 8 bits at 20,000
    and 100,000 bodies, 4 at 600,000 -- 3 of 9 bits with `tree_sort_wide` 1) and fixes the runs
    that tie there up afterwards; `tree_sort_mode` 0 runs seven 9-bit passes over the whole key instead.  Both must give the same stable
    order by key (which the oracle pins at <= 20,000 bodies above and at 2^20 / 4 M / 8 M bodies in
    test_full_size_gpu.py): body order, tree and new state bit for bit the same, after 2 steps (the
    second sorts a state that is already in sorted order; the disc has thousands of runs)."""
    nb = gpu
    sp = nb.SimParams(particle_num=n)
    state = nb.as_floats(getattr(nb.inits, init + "_init")(sp, seed=n % 97))
    a = run_tree(nb, state, 0.75, steps=2, count=False)
    b = run_tree(nb, state, 0.75, steps=2, count=False, tuning={"tree_sort_mode": 0})
    c = run_tree(nb, state, 0.75, steps=2, count=False, tuning={"tree_sort_wide": 1})   # 9-bit digits where they save a pass
    assert not a["status"].any() and not b["status"].any() and not c["status"].any()
    assert np.array_equal(a["order"], c["order"]) and np.array_equal(bits(a["dst"]), bits(c["dst"]))
    assert np.array_equal(a["order"], b["order"])
    assert np.array_equal(np.sort(a["order"]), np.arange(n, dtype=np.uint32))
    assert a["tree"].tobytes() == b["tree"].tobytes() and a["root_width"] == b["root_width"]
    assert np.array_equal(bits(a["dst"]), bits(b["dst"]))


@pytest.mark.gpu
@pytest.mark.parametrize("n,init", [(1, "uniform"), (255, "uniform"), (256, "disc"), (3000, "spherical"),
                                    (12288, "uniform"), (13000, "disc"), (16127, "uniform"), (16128, "uniform"),
                                    (40000, "disc"), (65279, "uniform")])
def test_tile_scan_inside_cells_c_gives_the_launched_scan_bits(gpu, n, init):
    """Up to 64 tiles of 256 bodies (16,127 bodies + the closing prefix) cells_c_kernel sums the tile table
    itself instead of reading cells_scan_kernel's scan (one dependent launch fewer); `tree_cell_scan_inline` 0
    launches the scan at every size, 2 uses the in-kernel form up to the 256 tiles it can do.  Node ids, slots
    and the binary64 moment prefixes must come out the same: order, tree and state bit for bit, over 3 steps
    (both sort paths: counted up to 12,288 bodies, radix + fix-up above)."""
    nb = gpu
    sp = nb.SimParams(particle_num=n)
    state = nb.as_floats(getattr(nb.inits, init + "_init")(sp, seed=7 + n % 89))
    runs = [run_tree(nb, state, 0.75, steps=3, count=False, tuning={"tree_cell_scan_inline": v}) for v in (0, 1, 2)]
    a = runs[0]
    assert not a["status"].any()
    for b in runs[1:]:
        assert not b["status"].any()
        assert np.array_equal(a["order"], b["order"])
        assert a["tree"].tobytes() == b["tree"].tobytes() and a["root_width"] == b["root_width"]
        assert np.array_equal(bits(a["dst"]), bits(b["dst"]))


@pytest.mark.parametrize("n,scale", [(4096, 1.0), (50000, 1.0), (3000, 4.0), (3000, 0.3), (20000, 0.5)])
def test_closed_form_keys_equal_the_descent(gpu, oracle, n, scale):
    """In a cube whose width is a power of two (every state inside the unit cube: bound 1.0) morton_kernel takes a
    body's key from ceil(x / h) instead of the 21-level descent of decide_octant / shift_node_center
    (tree.rs:549-562); `tree_key_descent` 1 forces the descent.  Bodies ON cell boundaries of every level (strict >
    sends them to the lower cell), on the cube's faces, at denormal distances from a boundary and at +-0 are the
    cases that could tell the two apart: same order, same tree, same state bit for bit -- and the tree is the
    oracle's."""
    nb = gpu
    rng = np.random.default_rng(n)
    s = make_state("uniform", n, 77 + n)
    half = 1.0 if scale <= 1.0 else scale          # max |coord| -> bound (never below 1.0)
    s[:, 0:3] *= np.float32(scale)
    k = n // 4                                      # a quarter of the bodies onto cell boundaries of random levels
    lev = rng.integers(1, 22, size=(k, 3))
    cells = rng.integers(0, 2 ** 21, size=(k, 3)) >> (21 - lev)
    edge = (cells.astype(np.float64) * (2.0 * half) / (2.0 ** lev) - half).astype(np.float32)
    s[:k, 0:3] = edge
    tiny = np.float32(1e-42)
    s[k:k + 64, 0] = np.nextafter(s[:64, 0], np.float32(np.inf))     # just above a boundary
    s[k + 64:k + 128, 1] = np.nextafter(s[:64, 1], np.float32(-np.inf))
    s[k + 128, 0:3] = (half, half, half)
    s[k + 129, 0:3] = (-half, -half, -half)
    s[k + 130, 0:3] = (0.0, -0.0, tiny)
    s[k + 131, 0:3] = (-tiny, tiny, 0.0)
    s[:, 0:3] = np.clip(s[:, 0:3], np.float32(-half), np.float32(half))   # (a step beyond a face would widen the cube)
    # no two bodies in one finest cell (the octree could not separate them): later duplicates are drawn again
    h = 2.0 * half / 2.0 ** 21
    for _ in range(20):
        cell = np.clip(np.ceil((s[:, 0:3].astype(np.float64) + half) / h) - 1, 0, 2 ** 21 - 1).astype(np.int64)
        code = (cell[:, 0] << 42) | (cell[:, 1] << 21) | cell[:, 2]
        _, first = np.unique(code, return_index=True)
        dup = np.setdiff1d(np.arange(n), first)
        if not len(dup):
            break
        s[dup, 0:3] = rng.uniform(-half, half, size=(len(dup), 3)).astype(np.float32) * np.float32(0.999)
    a = run_tree(nb, s, 0.75, steps=2, count=False)
    b = run_tree(nb, s, 0.75, steps=2, count=False, tuning={"tree_key_descent": 1})
    assert not a["status"].any() and not b["status"].any()
    assert np.array_equal(a["order"], b["order"])
    assert a["tree"].tobytes() == b["tree"].tobytes() and a["root_width"] == b["root_width"]
    assert np.array_equal(bits(a["dst"]), bits(b["dst"]))
    ref = oracle.tree_step_f32(s, G, E, DT, 0.75, flags=oracle.INTENDED)
    one = run_tree(nb, s, 0.75, steps=1)
    check_tree(one["tree"], one["root_width"], one["order"], ref["tree"], ref["root_width"], ref["order"],
               extent=float(np.abs(s[:, 0:3]).max()))


@pytest.mark.parametrize("n,init,steps", [(1, "uniform", 3), (7, "uniform", 2), (1000, "spherical", 5), (20000, "disc", 4),
                                          (300000, "uniform", 3)])
def test_walk_that_gathers_velocities_gives_the_sorted_copys_bits(gpu, n, init, steps):
    """From 524,288 bodies the walk fetches a body's velocity and acceleration through the order itself instead of
    having cells_c_kernel sort them first, writes the new position over the sorted old one and the state lands in the
    other buffer set (`cur` flips every step); `tree_walk_gathers` 0 / 2 force either form at any size.  Same values,
    same operations: state, order and the tree read back after the last step (its leaves from the walk records:
    the sorted source positions are gone by then) bit for bit, after an odd and an even number of steps, and
    through write_particles / a phase-split step in between."""
    nb = gpu
    sp = nb.SimParams(particle_num=n)
    state = nb.as_floats(getattr(nb.inits, init + "_init")(sp, seed=5 + n % 83))
    g, dt = (1e-5, 0.0016) if init == "disc" else (G, DT)
    for k in (steps, steps + 1):
        a = run_tree(nb, state, 0.75, steps=k, g=g, dt=dt, count=False, tuning={"tree_walk_gathers": 0})
        b = run_tree(nb, state, 0.75, steps=k, g=g, dt=dt, count=False, tuning={"tree_walk_gathers": 2})
        assert not a["status"].any() and not b["status"].any()
        assert np.array_equal(a["order"], b["order"])
        assert np.array_equal(bits(a["dst"]), bits(b["dst"]))
        assert a["tree"].tobytes() == b["tree"].tobytes() and a["root_width"] == b["root_width"]
    # mixed: whole steps (gathering), a step in two phases (never gathers), a new state, more whole steps
    sp2 = nb.SimParams(particle_num=n, g=g, dt=dt)
    sims = []
    for mode in (0, 2):
        sim = nb.TreeSim.from_particles(sp2, nb.AddParams.TreeSimParams(0.75), state)
        sim.set_tuning("tree_walk_gathers", mode)
        sim.encode(); sim.encode()
        sim.encode_phase(0); sim.encode_phase(1)
        sim.encode()
        mid = nb.as_floats(sim.dest_particle_slice()).copy()
        sim.write_particles(nb.as_particles(state))
        sim.encode(); sim.encode(); sim.encode()
        sim.wait()
        sims.append((mid, nb.as_floats(sim.dest_particle_slice()).copy()))
        sim.destroy()
    assert np.array_equal(bits(sims[0][0]), bits(sims[1][0]))
    assert np.array_equal(bits(sims[0][1]), bits(sims[1][1]))


def test_random_cases_against_oracle(gpu, oracle):
    """tools/tree_fuzz.py, 80 cases of a fixed seed: size (1 .. 30,000), distribution, theta (0.3 .. 1.3), scale of
    the cube (0.01 .. 300), walk shape, sort path and tile-scan form drawn at random; tree and order bit-exact,
    positions bit-exact, accelerations and visit counts within the tolerances stated in the tool."""
    from tools.tree_fuzz import fuzz
    lines = []
    cases, fails, _ = fuzz(budget=120.0, seed=2026, max_cases=80, log=lambda *a: lines.append(" ".join(str(x) for x in a)))
    assert cases >= 40, cases
    assert fails == 0, "\n".join(lines)


def test_visualize_workload_at_its_own_size_against_oracle(gpu, oracle):
    """the workload of src/bin/visualize.rs:26-38 at its own size -- 100,000 bodies of
    `disc_init` (a 150,000-mass body at the origin, mass contrast 1.5e5 : 1, a thin and deep tree),
    g = 1e-5, dt = 0.0016, theta = 0.75 -- against the oracle's restatement of the reference's builder and
    per-thread walk: tree, numbering and body order bit for bit, every body's new position bit for bit,
    forces to the tolerances of check_step (on all bodies and, separately, on the windows where the disc
    is hardest: around the central mass, mid-disc, at the rim), visit / accept totals.  Recorded, not
    required: the deepest the reference's 64-entry stack (tree.wgsl:44-45) would have gone on this input."""
    n, g, dt, theta = 100000, 0.00001, 0.0016, 0.75
    s = make_state("disc", n, 26, g)
    ref = oracle.tree_step_f32(s, g, E, dt, theta, flags=oracle.INTENDED)
    r = run_tree(gpu, s, theta, 1, g, E, dt)
    assert not r["status"].any()
    check_tree(r["tree"], r["root_width"], r["order"], ref["tree"], ref["root_width"], ref["order"])
    check_step(r["dst"], ref["dst"])
    pos0 = int(np.nonzero(ref["order"] == 0)[0][0])                       # the central mass, in sorted order
    rim = int(np.hypot(ref["sorted_src"][:, 0], ref["sorted_src"][:, 1]).argmax())
    for centre in (pos0, n // 2, rim):
        lo = min(max(centre - 128, 0), n - 256)
        check_step(r["dst"][lo:lo + 256], ref["dst"][lo:lo + 256])
    assert abs(int(r["counters"][0]) - ref["stats"]["visits"]) <= max(2, 1e-5 * ref["stats"]["visits"])
    assert abs(int(r["counters"][1]) - ref["stats"]["accepted"]) <= max(2, 1e-5 * ref["stats"]["accepted"])
    # the reference's fixed stack: 36 of its 64 entries on this input (seed 26) -- it does not overflow here
    assert ref["stats"]["overflowed"] == 0 and ref["stats"]["high_water"] <= 64, ref["stats"]
    print(f"disc 100,000: {len(ref['tree'])} nodes, oracle stack high water {ref['stats']['high_water']} of 64, "
          f"{ref['stats']['visits'] / n:.0f} visits per body")


def test_visualize_workload_over_fifty_steps(gpu, oracle):
    """... and over time.  (a) 100,000 bodies, 50 steps: finite, no status word raised (node capacity, key
    collisions, stack guard).  (b) A 4,096-body disc with the same parameters, 50 Barnes-Hut steps
    against 50 binary64 all-pairs steps of the oracle (naive.wgsl's force law): the
    disc is not in equilibrium (its kinetic energy grows 14 % over the 50 steps), so what is compared is
    the energy reached (to 1e-4; measured 5.7e-6) and the angular momentum kept (to 1e-5; measured 9e-8)."""
    nb = gpu
    g, dt, theta = 0.00001, 0.0016, 0.75
    big = run_tree(nb, make_state("disc", 100000, 26, g), theta, 50, g, E, dt, count=False)
    assert np.isfinite(big["dst"]).all() and not big["status"].any()
    s = make_state("disc", 4096, 27, g)
    got = run_tree(nb, s, theta, 50, g, E, dt, count=False)
    assert np.isfinite(got["dst"]).all() and not got["status"].any()
    ref = oracle.naive_run_f64(s, g, E, dt, 50)
    f8 = lambda a: a.astype(np.float64)
    ke = lambda a: (0.5 * f8(a[:, 9]) * (f8(a[:, 3:6]) ** 2).sum(1)).sum()
    lz = lambda a: (f8(a[:, 9]) * (f8(a[:, 0]) * f8(a[:, 4]) - f8(a[:, 1]) * f8(a[:, 3]))).sum()
    d_ke = abs(ke(got["dst"]) - ke(ref)) / ke(ref)
    d_lz = abs(lz(got["dst"]) - lz(ref)) / abs(lz(ref))
    print(f"disc 4,096 x 50 steps: kinetic energy {ke(s):.4f} -> {ke(got['dst']):.4f} (all-pairs fp64 {ke(ref):.4f}, "
          f"rel diff {d_ke:.2e}); L_z rel diff {d_lz:.2e}")
    assert d_ke < 1e-4 and d_lz < 1e-5, (d_ke, d_lz)


@pytest.mark.gpu
def test_dense_core_does_not_stall_the_sort(gpu):
    """The normal late state of a gravitational run: a dense core plus a few far escapers that set the root
    cube.  The core then fills a handful of the cells the high-digit passes can tell apart, the fix-up
    meets runs of 10^4 .. 10^6 bodies that tie there, and ranking such a run by counting (L^2 compares
    in one workgroup) would take seconds to minutes.  Runs longer than 1,024 are radix-sorted by the
    workgroup instead, and the statistics the fix-up leaves make the next builds sort more high digits
    (TreeSim::adapt_sort).  Must hold: the same order / tree / state as the 8-pass full sort, bit for
    bit, on every step; a first step in well under a second; later steps at the usual speed."""
    import time
    nb = gpu
    n = 1 << 20
    rng = np.random.default_rng(2025)    # (a seed without two bodies in one 2^-21 cell)
    state = np.zeros((n, 10), dtype=np.float32)
    core = int(0.9 * n)
    state[:core, 0:3] = rng.uniform(-0.006, 0.006, size=(core, 3)).astype(np.float32) + np.float32(0.3)
    state[core:, 0:3] = rng.uniform(-1.0, 1.0, size=(n - core, 3)).astype(np.float32)
    state[:, 9] = 1.0
    state = state[rng.permutation(n)]
    sp = nb.SimParams(particle_num=n, g=1e-9)          # (weak coupling: the core must not collapse within the test)
    sims = {}
    for mode in (1, 0):
        sim = nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(0.75), state)
        sim.set_tuning("tree_sort_mode", mode)
        sims[mode] = sim
    times = []
    for step in range(5):
        outs = {}
        for mode, sim in sims.items():
            t0 = time.perf_counter()
            sim.encode()
            sim.wait()
            if mode == 1:
                times.append(time.perf_counter() - t0)
            outs[mode] = (sim.debug_buffer("order", np.uint32).copy(), sim.dest_particle_slice().copy())
        assert np.array_equal(outs[0][0], outs[1][0]), step
        assert np.array_equal(outs[0][1], outs[1][1]), step
    assert not sims[1].debug_buffer("status", np.uint32).any()
    for sim in sims.values():
        sim.destroy()
    assert times[0] < 0.5, times        # the step that meets the long runs unprepared
    assert max(times[2:]) < 0.02, times  # once the passes cover them: a few ms (the walk of a dense core)


@pytest.mark.gpu
def test_single_body_and_empty_tree_sims(gpu, oracle):
    """One body: pure kick-drift-kick with its old acceleration (no force: the only leaf is its own),
    bit for bit the oracle -- velocity, acceleration and mass included.  No body: steps and reads
    back nothing (the reference would build a root octant of 0 bodies and dispatch no workgroup)."""
    nb = gpu
    s = np.array([[0.1, 0.2, 0.3, 1.0, -2.0, 0.5, 0.25, 0.5, -0.75, 3.0]], np.float32)
    ref = oracle.tree_step_f32(s, G, E, DT, 0.5)
    r = run_tree(nb, s, 0.5, 1)
    assert not r["status"].any()
    assert np.array_equal(bits(r["dst"]), bits(ref["dst"]))
    sp = nb.SimParams(particle_num=0)
    sim = nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(0.5), np.zeros((0, 10), np.float32))
    for _ in range(2):
        sim.encode()
        sim.cleanup()
    sim.wait()
    assert nb.as_floats(sim.dest_particle_slice()).shape == (0, 10)
    sim.destroy()
