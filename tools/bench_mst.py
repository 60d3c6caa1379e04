"""Minimum-spanning-tree benchmark (nb_mst_sim, csrc/nb_mst.hip).  Per case: the kernels alone -- HIP events on the
simulator's stream around a call that asks for the stats only -- and the median wall time of whole calls (host clock:
launches, the copies of the edges and degrees, the synchronisation); the rounds and the kernel time per round; beside
it, in the same run on the same state, nb_sim_knn(k = 6) and nb_sim_fof at 0.2 mean inter-body spacings (stats-only
calls by HIP events).  --prunings times the kernels with "mst_skip_runs" and "mst_shared_bound" each off for the cases
named.  --baseline adds what the call replaces on the spread rows: read_particles, then scipy's minimum spanning tree
of a candidate graph that is exact -- every pair within r of each other (cKDTree.query_pairs), r the longest edge of
the device's tree: that graph is connected (checked), so it holds every edge of the tree of the complete graph, whose
longest edge is the smallest r at which the graph connects; every candidate's d2 is formed by the rule of
include/nbody.h.  A row whose candidate graph would not fit (--max-pairs), or of more than --baseline-max-n bodies,
has no baseline.  A call that takes longer than --budget-s / 15 is repeated less often than --reps; the row says how
often.  The cases of DESIGN.md 6y: the
100,000-body disc, 2^20 bodies spherical, 4,000,000 uniform, and three concentrated states of 2^20 bodies: two blobs of
1e-3 a hundred apart, 1,024 points of 1,024 coincident bodies, and every body but one within 2^-20 of the extent.
Prints one JSON line per case, a table and a summary line.  Secondary to bench.py."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wgpu_n_body_amd as nb  # noqa: E402
from wgpu_n_body_amd import _lib  # noqa: E402

# name, init, n, concentration
CASES = [
    ("disc 100k", "disc", 100_000, None),
    ("sphere 2^20", "spherical", 1 << 20, None),
    ("uniform 4M", "uniform", 4_000_000, None),
    ("2^20 two blobs", "uniform", 1 << 20, "blobs"),
    ("2^20 at 1024 points", "uniform", 1 << 20, "points"),
    ("2^20 and an outlier", "uniform", 1 << 20, "outlier"),
]

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, nargs="*", default=list(range(len(CASES))), help="indices into the case list")
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--budget-s", type=float, default=20.0, help="seconds of timed mst calls per case and setting")
ap.add_argument("--prunings", type=int, nargs="*", default=[1, 4], help="cases timed with each pruning off")
ap.add_argument("--baseline", type=int, default=0, help="timed read_particles + scipy runs per spread case (0: none)")
ap.add_argument("--baseline-max-n", type=int, default=1 << 20, help="the largest state a baseline is made for")
ap.add_argument("--max-pairs", type=float, default=1.5e8, help="candidate pairs a baseline may hold")
ap.add_argument("--table", default="", help="also write the table to this file")
args = ap.parse_args()

if nb.device_count() < 1:
    sys.exit("bench_mst needs a HIP device (no CPU fallback)")


def make(init, n, conc, stream):
    sp = nb.SimParams(particle_num=n)
    state = nb.as_floats({"uniform": nb.inits.uniform_init, "disc": nb.inits.disc_init,
                          "spherical": nb.inits.spherical_init}[init](sp, seed=1)).copy()
    rng = np.random.default_rng(2)
    if conc == "blobs":  # two balls of radius 1e-3, 100 apart
        v = rng.normal(size=(n, 3))
        v *= (1e-3 * rng.uniform(0.0, 1.0, n) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]
        v[n // 2:, 0] += 100.0
        state[:, 0:3] = v
    elif conc == "points":  # 1,024 places, 1,024 bodies each
        places = rng.uniform(-1.0, 1.0, (1024, 3)).astype(np.float32)
        state[:, 0:3] = places[rng.permutation(n) % 1024]
    elif conc == "outlier":  # all within 2^-20 of the extent, which one body sets
        state[:, 0:3] = rng.uniform(0.0, 2.0 ** -20, (n, 3))
        state[0, 0:3] = (1.0, 0.0, 0.0)
    # the fof link: 0.2 spacings of the volume that holds the middle 80 % of the bodies on every axis
    lo, hi = np.percentile(state[:, 0:3], [10, 90], axis=0)
    inside = np.all((state[:, 0:3] >= lo) & (state[:, 0:3] <= hi), axis=1).sum()
    link = 0.2 * float((np.prod(np.maximum(hi - lo, 1e-6)) / max(inside, 1)) ** (1.0 / 3.0))
    return nb.NaiveSim.from_particles(sp, None, state, placement=nb.Placement(stream=stream.cuda_stream)), link


def timed(stream, call, reps, warmup, budget):
    """Median and minimum ms of call() by HIP events; fewer repetitions when one takes long."""
    ts = []
    for r in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        if r >= warmup:
            ts.append(e0.elapsed_time(e1))
            if sum(ts) > budget * 1e3:
                break
    return float(np.median(ts)), float(np.min(ts)), len(ts)


def host_tree(state, r):
    """read_particles' state -> (lo, hi, d2) of scipy's tree of every pair within r, or None when not connected."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components, minimum_spanning_tree
    from scipy.spatial import cKDTree
    pos = state[:, 0:3]
    tree = cKDTree(pos.astype(np.float64))
    if tree.count_neighbors(tree, r * (1.0 + 1e-9)) / 2 > args.max_pairs:
        return "too many pairs"
    pairs = tree.query_pairs(r * (1.0 + 1e-9), output_type="ndarray")
    d = pos[pairs[:, 0]].astype(np.float64) - pos[pairs[:, 1]].astype(np.float64)
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    n = len(pos)
    # (scipy takes a stored 0 for a missing edge: coincident bodies would need a shift; the spread states have none)
    g = coo_matrix((d2, (pairs[:, 0], pairs[:, 1])), shape=(n, n)).tocsr()
    if connected_components(g, directed=False)[0] != 1:
        return "not connected"
    t = minimum_spanning_tree(g).tocoo()
    a, b = np.minimum(t.row, t.col), np.maximum(t.row, t.col)
    o = np.lexsort((b, a, t.data))
    return a[o].astype(np.uint32), b[o].astype(np.uint32), t.data[o]


rows = []
stream = torch.cuda.Stream()
L = _lib.lib()
for ci in args.cases:
    name, init, n, conc = CASES[ci]
    sim, link = make(init, n, conc, stream)
    p, st = _lib.nb_mst_params(), _lib.nb_mst_stats()
    stats_only = lambda: _lib.check(L.nb_mst_sim(sim._h, C.byref(p), None, None, None, None, C.byref(st)))
    row = {"case": name, "n": n}
    settings = [("", 1, 1)] + ([("_no_skip", 0, 1), ("_no_shared", 1, 0)] if ci in args.prunings else [])
    for tag, skip, shared in settings:
        sim.set_tuning("mst_skip_runs", skip)
        sim.set_tuning("mst_shared_bound", shared)
        med, low, reps = timed(stream, stats_only, args.reps, args.warmup, args.budget_s)
        row.update({"kernels%s_median_ms" % tag: med, "kernels%s_min_ms" % tag: low, "kernels%s_reps" % tag: reps})
    sim.set_tuning("mst_skip_runs", 1)
    sim.set_tuning("mst_shared_bound", 1)
    tw = []
    for r in range(args.warmup + row["kernels_reps"]):
        t0 = time.perf_counter()
        tree = sim.spanning_tree()
        t1 = time.perf_counter()
        if r >= args.warmup:
            tw.append((t1 - t0) * 1e3)
    row.update({"call_median_ms": float(np.median(tw)), "call_min_ms": float(np.min(tw)), "edges": tree.stats.edges,
                "rounds": tree.stats.rounds, "components_after": tree.stats.components_after[:tree.stats.rounds].tolist(),
                "ms_per_round": row["kernels_median_ms"] / max(tree.stats.rounds, 1),
                "total_length": tree.total_length, "longest": tree.longest()[2] if tree.longest() else 0.0})
    kp, ks = _lib.nb_knn_params(), _lib.nb_knn_stats()
    kp.k = 6
    row["knn6_median_ms"], _, row["knn6_reps"] = timed(
        stream, lambda: _lib.check(L.nb_sim_knn(sim._h, C.byref(kp), None, None, None, None, C.byref(ks))), args.reps,
        args.warmup, args.budget_s)
    fp, fs = _lib.nb_fof_params(), _lib.nb_fof_stats()
    fp.link, fp.min_members = link, 1
    row["fof_link"] = link
    try:
        row["fof_median_ms"], _, _ = timed(
            stream, lambda: _lib.check(L.nb_sim_fof(sim._h, C.byref(fp), None, None, None, 0, C.byref(fs))), args.reps,
            args.warmup, args.budget_s)
        row["fof_components"] = int(fs.components)
        row["cut_components"] = int(tree.group_counts([link])[0])
    except nb.NBodyError as e:  # (a link that needs too many cells)
        row["fof_refused"] = str(e)[:80]
    if args.baseline > 0 and conc is None and n <= args.baseline_max_n:
        tb, got = [], None
        for _ in range(args.baseline):
            t0 = time.perf_counter()
            got = host_tree(nb.as_floats(sim.read_particles()), tree.longest()[2])
            tb.append((time.perf_counter() - t0) * 1e3)
            if isinstance(got, str):
                break
        if isinstance(got, str):
            row["baseline"] = got
        else:
            row["baseline_median_ms"] = float(np.median(tb))
            row["baseline"] = "cKDTree + csgraph"
            row["edges_equal"] = bool(np.array_equal(got[0], tree.edges[:, 0]) and np.array_equal(got[1], tree.edges[:, 1])
                                      and got[2].tobytes() == tree.d2.tobytes())
    sim.destroy()
    rows.append(row)
    print(json.dumps(row), flush=True)

lines = ["# tools/bench_mst.py: nb_mst_sim on a NaiveSim, ms per call, median of up to %d (kernels: HIP events around a "
         "stats-only call; call: host clock around the whole call with edges, d2 and degrees; reps: the timed calls, "
         "fewer where they exceed %g s together)" % (args.reps, args.budget_s),
         "# " + nb.version(),
         "# knn6, fof: stats-only nb_sim_knn(k = 6) and nb_sim_fof(0.2 spacings, min_members 1) on the same state in the "
         "same run, HIP events; no skip / no shared: the kernels with \"mst_skip_runs\" / \"mst_shared_bound\" off",
         "# baseline: read_particles + cKDTree.query_pairs(longest edge) + scipy's minimum_spanning_tree, ms; equal: its "
         "edges and d2 against the device's",
         "%-20s %8s %6s %10s %10s %5s %10s %10s %10s %10s %10s %10s %12s %6s" % (
             "case", "n", "rounds", "kernels", "per round", "reps", "call", "knn6", "fof", "no skip", "no shared",
             "baseline", "by", "equal")]
for r in rows:
    f = lambda k: "%.3f" % r[k] if k in r else "-"
    lines.append("%-20s %8d %6d %10s %10s %5d %10s %10s %10s %10s %10s %10s %12s %6s" % (
        r["case"], r["n"], r["rounds"], f("kernels_median_ms"), f("ms_per_round"), r["kernels_reps"],
        f("call_median_ms"), f("knn6_median_ms"), f("fof_median_ms"), f("kernels_no_skip_median_ms"),
        f("kernels_no_shared_median_ms"), f("baseline_median_ms"), r.get("baseline", "-"),
        {True: "yes", False: "NO"}.get(r.get("edges_equal"), "-")))
print("\n".join(lines))
if args.table:
    with open(args.table, "w") as f:
        f.write("\n".join(lines) + "\n")
print(json.dumps({"bench": "spanning_tree", "rows": len(rows), "device": nb.version()}))
