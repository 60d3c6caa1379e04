"""Phase-space groups benchmark (nb_fof6_sim, csrc/nb_fof6.hip) beside nb_sim_fof at the same state and link.  Per case
and pass: the kernels alone -- HIP events on the simulator's stream around a call that asks for the stats only -- and
the median wall time of whole calls (host clock: launches, the copies of labels, group_of and the catalogue, the
synchronisation); for nb_fof6_sim also the kernels without the cells' boxes ("fof6_boxes" 0) where that is not a run
of P^2 unions.  The cases of DESIGN.md 6u: the 100,000-body disc, 2^20 bodies spherical and 4,000,000 uniform, each at
a link of 0.2 mean inter-body spacings and a vlink of 0.2 of the state's own 3-D velocity dispersion; 2^20 bodies in one
cell, cold (all friends) and hot (nobody is anybody's friend in velocity: P (P - 1) / 2 pair tests); and two
interpenetrating uniform blobs of 2^19 bodies whose velocities are disjoint.  Prints one JSON line per case, a table
and a summary line.  Secondary to bench.py."""
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

# name, init, n, link in mean inter-body spacings (None: set by the construction), construction
CASES = [
    ("disc 100k", "disc", 100_000, 0.2, None),
    ("sphere 2^20", "spherical", 1 << 20, 0.2, None),
    ("uniform 4M", "uniform", 4_000_000, 0.2, None),
    ("2^20 cell cold", "uniform", 1 << 20, None, "cold"),
    ("2^20 cell hot", "uniform", 1 << 20, None, "hot"),
    ("2x2^19 blobs", "uniform", 1 << 20, 0.5, "blobs"),
]

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, nargs="*", default=list(range(len(CASES))), help="indices into the case list")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--hot-reps", type=int, default=2, help="timed calls of the hot cell (seconds each), after one warm-up")
ap.add_argument("--no-boxes-reps", type=int, default=3, help="timed stats-only calls without the cells' boxes")
ap.add_argument("--min-members", type=int, default=20)
ap.add_argument("--table", default="", help="also write the table to this file")
args = ap.parse_args()

if nb.device_count() < 1:
    sys.exit("bench_fof6 needs a HIP device (no CPU fallback)")


def spacing(pos):
    """Of the volume that holds the middle 80 % of the bodies on every axis (tools/bench_fof.py's)."""
    lo, hi = np.percentile(pos, [10, 90], axis=0)
    inside = np.all((pos >= lo) & (pos <= hi), axis=1).sum()
    return float((np.prod(np.maximum(hi - lo, 1e-6)) / max(inside, 1)) ** (1.0 / 3.0))


def make(init, n, spacings, how, stream):
    sp = nb.SimParams(particle_num=n)
    state = nb.as_floats({"uniform": nb.inits.uniform_init, "disc": nb.inits.disc_init,
                          "spherical": nb.inits.spherical_init}[init](sp, seed=1)).copy()
    rng = np.random.default_rng(2)
    expect = None
    if how in ("cold", "hot"):  # every body within link / 4 of one point
        link, vlink = 0.01, 1.0
        state[:, 0:3] = 0.3 + rng.uniform(0.0, link / 4, (n, 3))
        if how == "cold":  # ... and within vlink / 100 in velocity: one component
            state[:, 3:6], expect = rng.uniform(0.0, vlink / 100, (n, 3)), 1
        else:  # ... and 8 vlink from the next body in velocity (exact in binary32): n components
            state[:, 3:6], expect = 0.0, n
            state[:, 4] = 8.0 * vlink * rng.permutation(n)
    elif how == "blobs":  # the same cube twice, the second half 10 apart in velocity from the first, both cold
        link, vlink = spacings * spacing(state[:, 0:3]), 0.1
        state[:, 3:6] = rng.normal(0.0, 0.01, (n, 3))
        state[n // 2:, 3] += 10.0
    else:
        v = state[:, 3:6].astype(np.float64)
        link, vlink = spacings * spacing(state[:, 0:3]), 0.2 * float(np.sqrt(((v - v.mean(axis=0)) ** 2).sum(axis=1).mean()))
    return (nb.NaiveSim.from_particles(sp, None, state, placement=nb.Placement(stream=stream.cuda_stream)), link, vlink,
            expect)


def kernels_ms(stream, call, handle, p, st):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    _lib.check(call(handle, C.byref(p), None, None, None, 0, C.byref(st)))
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


rows = []
stream = torch.cuda.Stream()
L = _lib.lib()
for ci in args.cases:
    name, init, n, spacings, how = CASES[ci]
    sim, link, vlink, expect = make(init, n, spacings, how, stream)
    p3, p6 = _lib.nb_fof_params(), _lib.nb_fof6_params()
    p3.link, p3.min_members = link, args.min_members
    p6.link, p6.vlink, p6.min_members = link, vlink, args.min_members
    st = _lib.nb_fof_stats()
    warmup, reps = (1, args.hot_reps) if how == "hot" else (args.warmup, args.reps)
    t = {"fof": [], "fof6": [], "fof6_no_boxes": [], "fof_call": [], "fof6_call": []}
    for r in range(warmup + reps):
        timed = r >= warmup
        a = kernels_ms(stream, L.nb_sim_fof, sim._h, p3, st)
        b = kernels_ms(stream, L.nb_fof6_sim, sim._h, p6, st)
        t0 = time.perf_counter()
        f3 = sim.fof_groups(link, min_members=args.min_members)
        t1 = time.perf_counter()
        f6 = sim.phase_space_groups(link, vlink, min_members=args.min_members)
        t2 = time.perf_counter()
        if timed:
            t["fof"].append(a)
            t["fof6"].append(b)
            t["fof_call"].append((t1 - t0) * 1e3)
            t["fof6_call"].append((t2 - t1) * 1e3)
        if how not in ("cold", "hot") and warmup <= r < warmup + args.no_boxes_reps:
            sim.set_tuning("fof6_boxes", 0)
            t["fof6_no_boxes"].append(kernels_ms(stream, L.nb_fof6_sim, sim._h, p6, st))
            sim.set_tuning("fof6_boxes", 1)
    med = {k: float(np.median(v)) if v else None for k, v in t.items()}
    s3, s6 = f3.stats, f6.stats
    row = {"case": name, "n": n, "link": link, "vlink": vlink, "min_members": args.min_members, "reps": reps,
           "fof_kernels_ms": med["fof"], "fof6_kernels_ms": med["fof6"], "fof6_kernels_min_ms": float(np.min(t["fof6"])),
           "fof6_no_boxes_ms": med["fof6_no_boxes"], "fof_call_ms": med["fof_call"], "fof6_call_ms": med["fof6_call"],
           "kernels_ratio": med["fof6"] / med["fof"], "call_ratio": med["fof6_call"] / med["fof_call"],
           "cells": list(s6.cells), "fof_components": s3.components, "components": s6.components, "groups": s6.groups,
           "largest_count": s6.largest_count}
    # every phase-space group inside one friends-of-friends group; the constructed states' known partitions
    ok = f6.labels != nb.FOF_NONE
    pairs = np.unique(np.stack([f6.labels[ok], f3.labels[ok]], axis=1), axis=0)
    row["refines"] = bool(len(pairs) == s6.components and np.array_equal(ok, f3.labels != nb.FOF_NONE))
    if expect is not None:
        row["as_constructed"] = bool(s6.components == expect and s3.components == 1)
    sim.destroy()
    rows.append(row)
    print(json.dumps(row), flush=True)

lines = ["# tools/bench_fof6.py: nb_fof6_sim beside nb_sim_fof on the same NaiveSim and link, ms per call, median of %d "
         "(%d for the hot cell) (kernels: HIP events around a stats-only call; no boxes: \"fof6_boxes\" 0, median of %d; "
         "call: host clock around the whole call with labels, group_of and the catalogue at min_members %d)"
         % (args.reps, args.hot_reps, args.no_boxes_reps, args.min_members),
         "# " + nb.version(),
         "# ratio: nb_fof6_sim / nb_sim_fof; refines: every phase-space group lies inside one friends-of-friends group; "
         "built: the constructed partition was found (cold: one component, hot: n components)",
         "%-15s %8s %10s %10s %9s %9s %9s %7s %9s %9s %7s %9s %9s %7s %5s" % (
             "case", "n", "link", "vlink", "fof kern", "fof6 kern", "no boxes", "ratio", "fof call", "fof6 call",
             "ratio", "groups", "largest", "refines", "built")]
yn = {True: "yes", False: "NO", None: "-"}
for r in rows:
    lines.append("%-15s %8d %10.3e %10.3e %9.3f %9.3f %9s %7.2f %9.3f %9.3f %7.2f %9d %9d %7s %5s" % (
        r["case"], r["n"], r["link"], r["vlink"], r["fof_kernels_ms"], r["fof6_kernels_ms"],
        "-" if r["fof6_no_boxes_ms"] is None else "%.3f" % r["fof6_no_boxes_ms"], r["kernels_ratio"], r["fof_call_ms"],
        r["fof6_call_ms"], r["call_ratio"], r["groups"], r["largest_count"], yn[r["refines"]],
        yn[r.get("as_constructed")]))
print("\n".join(lines))
if args.table:
    with open(args.table, "w") as f:
        f.write("\n".join(lines) + "\n")
print(json.dumps({"bench": "phase_space_groups", "rows": len(rows), "device": nb.version()}))
