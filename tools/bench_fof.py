"""Friends-of-friends benchmark (nb_sim_fof, csrc/nb_fof.hip).  Per case: the kernels alone -- HIP events on the
simulator's stream around a call that asks for the stats only -- with the cells' bounding boxes on and off
("fof_cell_boxes"), and the median wall time of whole calls (host clock: launches, the copies of labels, group_of and
the catalogue, the synchronisation).  --baseline adds what the call replaces, read_particles plus a CPU neighbour
search (scipy.spatial.cKDTree and scipy.sparse.csgraph where scipy is installed, else the grid restatement of
tests/fof_ref.py), every candidate pair decided by the rule of include/nbody.h, and compares its labels with the
device's.  The cases of DESIGN.md 6h: the 100,000-body disc, 2^20 bodies spherical and 4,000,000 uniform, each at a
link of 0.2 mean inter-body spacings, and three concentrated states of 2^20 bodies: every body in one cell, two dense
blobs in neighbouring cells that are not friends, and a uniform state at ten times that link (one giant component).
The first two of those have no pair list a CPU could hold: their groups are checked against the construction (one
component, two components) instead.  Prints one JSON line per case, a table and a summary line.  Secondary to
bench.py."""
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

# name, init, n, link in mean inter-body spacings (None: set by the concentration), concentration
CASES = [
    ("disc 100k", "disc", 100_000, 0.2, None),
    ("sphere 2^20", "spherical", 1 << 20, 0.2, None),
    ("uniform 4M", "uniform", 4_000_000, 0.2, None),
    ("2^20 one cell", "uniform", 1 << 20, None, "cell"),
    ("2^20 two blobs", "uniform", 1 << 20, None, "blobs"),
    ("2^20 giant", "uniform", 1 << 20, 2.0, None),
]

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, nargs="*", default=list(range(len(CASES))), help="indices into the case list")
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--no-boxes-reps", type=int, default=3, help="timed stats-only calls without the cells' boxes")
ap.add_argument("--min-members", type=int, default=20)
ap.add_argument("--baseline", type=int, default=0, help="timed read_particles + CPU runs per case (0: none)")
ap.add_argument("--table", default="", help="also write the table to this file")
args = ap.parse_args()

if nb.device_count() < 1:
    sys.exit("bench_fof needs a HIP device (no CPU fallback)")


def make(init, n, spacings, conc, stream):
    sp = nb.SimParams(particle_num=n)
    state = nb.as_floats({"uniform": nb.inits.uniform_init, "disc": nb.inits.disc_init,
                          "spherical": nb.inits.spherical_init}[init](sp, seed=1)).copy()
    rng = np.random.default_rng(2)
    expect = None
    if conc == "cell":  # every body within link / 4 of one point
        link, expect = 0.01, 1
        state[:, 0:3] = 0.3 + rng.uniform(0.0, link / 4, (n, 3))
    elif conc == "blobs":  # two cubes of side link / 4, 1.5 link apart
        link, expect = 0.01, 2
        state[:, 0:3] = 0.3 + rng.uniform(0.0, link / 4, (n, 3))
        state[n // 2:, 0] += 1.5 * link
    else:  # spacing: of the volume that holds the middle 80 % of the bodies on every axis
        lo, hi = np.percentile(state[:, 0:3], [10, 90], axis=0)
        inside = np.all((state[:, 0:3] >= lo) & (state[:, 0:3] <= hi), axis=1).sum()
        link = spacings * float((np.prod(np.maximum(hi - lo, 1e-6)) / max(inside, 1)) ** (1.0 / 3.0))
    return nb.NaiveSim.from_particles(sp, None, state, placement=nb.Placement(stream=stream.cuda_stream)), link, expect


def cpu_labels(state, link):
    """What the call replaces: a neighbour search on the host, the rule on every candidate, connected components."""
    from tests import fof_ref
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        from scipy.spatial import cKDTree
    except ImportError:
        return fof_ref.fof_grid(state, link)["labels"], "grid"
    ok = fof_ref.body_ok(state)
    idx = np.flatnonzero(ok)
    pos = state[idx, 0:3]
    pairs = cKDTree(pos.astype(np.float64)).query_pairs(link * (1.0 + 1e-9), output_type="ndarray")
    keep = fof_ref.friends(pos[pairs[:, 0]], pos[pairs[:, 1]], link)
    i, j = pairs[keep, 0], pairs[keep, 1]
    m = idx.size
    _, comp = connected_components(coo_matrix((np.ones(i.size, np.int8), (i, j)), shape=(m, m)), directed=False)
    first = np.full(comp.max() + 1 if m else 0, m, np.int64)
    np.minimum.at(first, comp, np.arange(m))
    labels = np.full(state.shape[0], fof_ref.NONE, np.uint32)
    labels[idx] = idx[first[comp]]
    return labels, "cKDTree"


rows = []
stream = torch.cuda.Stream()
for ci in args.cases:
    name, init, n, spacings, conc = CASES[ci]
    sim, link, expect = make(init, n, spacings, conc, stream)
    p = _lib.nb_fof_params()
    p.link, p.min_members = link, args.min_members
    st = _lib.nb_fof_stats()
    tk = {0: [], 1: []}
    tw = []
    for r in range(args.warmup + args.reps):
        for boxes in (0, 1):
            if boxes == 0 and r >= args.warmup + args.no_boxes_reps:  # (up to 2^38 pair tests a call on the two blobs)
                continue
            sim.set_tuning("fof_cell_boxes", boxes)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            _lib.check(_lib.lib().nb_sim_fof(sim._h, C.byref(p), None, None, None, 0, C.byref(st)))
            e1.record(stream)
            e1.synchronize()
            if r >= args.warmup:
                tk[boxes].append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        fg = sim.fof_groups(link, min_members=args.min_members)
        t1 = time.perf_counter()
        if r >= args.warmup:
            tw.append((t1 - t0) * 1e3)
    tw = np.array(tw)
    s = fg.stats
    row = {"case": name, "n": n, "link": link, "min_members": args.min_members, "reps": args.reps,
           "kernels_median_ms": float(np.median(tk[1])), "kernels_min_ms": float(np.min(tk[1])),
           "kernels_no_boxes_median_ms": float(np.median(tk[0])), "call_median_ms": float(np.median(tw)),
           "call_min_ms": float(tw.min()), "call_max_ms": float(tw.max()), "cells": list(s.cells),
           "components": s.components, "groups": s.groups, "grouped_bodies": s.grouped_bodies,
           "largest_count": s.largest_count}
    if expect is not None:
        row["groups_equal"] = bool(s.components == expect and s.nonfinite == 0 and
                                   np.unique(fg.labels).size == expect)
        row["baseline"] = "construction"
    elif args.baseline > 0:
        tb = []
        for _ in range(args.baseline):
            t0 = time.perf_counter()
            labels, how = cpu_labels(nb.as_floats(sim.read_particles()), link)
            tb.append((time.perf_counter() - t0) * 1e3)
        row["baseline_median_ms"] = float(np.median(tb))
        row["baseline"] = how
        row["groups_equal"] = bool(np.array_equal(labels, fg.labels))
    sim.destroy()
    rows.append(row)
    print(json.dumps(row), flush=True)

lines = ["# tools/bench_fof.py: nb_sim_fof on a NaiveSim, ms per call, median of %d (kernels: HIP events around a "
         "stats-only call, with and without the cells' boxes; call: host clock around the whole call with labels, "
         "group_of and the catalogue at min_members %d)" % (args.reps, args.min_members),
         "# " + nb.version(),
         "# baseline: read_particles + the CPU neighbour search and components, ms; equal: its labels against the "
         "device's (construction: the state has a known partition and no pair list a CPU could hold, so those rows have no "
         "baseline time); no boxes: median of %d" % args.no_boxes_reps,
         "%-15s %9s %10s %9s %9s %9s %9s %9s %9s %9s %10s %12s %6s" % (
             "case", "n", "link", "kernels", "kern min", "no boxes", "call", "call min", "groups", "largest",
             "baseline", "by", "equal")]
for r in rows:
    lines.append("%-15s %9d %10.3e %9.4f %9.4f %9.4f %9.4f %9.4f %9d %9d %10s %12s %6s" % (
        r["case"], r["n"], r["link"], r["kernels_median_ms"], r["kernels_min_ms"], r["kernels_no_boxes_median_ms"],
        r["call_median_ms"], r["call_min_ms"], r["groups"], r["largest_count"],
        "%.1f" % r["baseline_median_ms"] if "baseline_median_ms" in r else "-", r.get("baseline", "-"),
        {True: "yes", False: "NO"}.get(r.get("groups_equal"), "-")))
print("\n".join(lines))
if args.table:
    with open(args.table, "w") as f:
        f.write("\n".join(lines) + "\n")
print(json.dumps({"bench": "fof_groups", "rows": len(rows), "device": nb.version()}))
