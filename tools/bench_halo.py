"""Halo-profiles benchmark (nb_sim_halo_profiles, csrc/nb_halo.hip).  Per state: HIP events on the simulator's
stream around calls that ask for the stats only (kernels: everything but the copy of the rows), the median wall time
of whole calls with every output (host clock), and the two ways to the same rows without the pass, in the same
process:
  loop  -- nb_sim_radial_profile once per centre with the same explicit centre, velocity and edges (the only way
           the rows could be had without this pass), through the C ABI with its buffers made once, like the halo
           call; the median over a sample of the centres after warm-up calls, scaled to all of them;
  tree  -- read_particles, scipy's cKDTree over the bodies, query_ball_point per centre and the rule in numpy on
           what it returns (the build is counted once, the queries over the same sample and scaled).
The counts of both must equal the device's for every sampled centre, else the run fails.  ps/test is the kernels'
time over stats.tested.  The last state's spheres hold every body: its ns/body is the kernels' time over m n, beside
nb_sim_radial_profile's per body on the same state.
Prints one JSON line per state, a table and a summary line.  Secondary to bench.py."""
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

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, nargs="*", default=[0, 1, 2, 3])
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--sample", type=int, default=64, help="centres the baselines are timed on")
ap.add_argument("--nbins", type=int, default=32)
ap.add_argument("--label", default="", help="a word for the table's rows (another build, by NB_LIB)")
ap.add_argument("--no-baselines", action="store_true")
ap.add_argument("--table", default="", help="also write the table to this file")
args = ap.parse_args()

if nb.device_count() < 1:
    sys.exit("bench_halo needs a HIP device (no CPU fallback)")
try:
    from scipy.spatial import cKDTree
except ImportError:
    cKDTree = None

stream = torch.cuda.Stream()
L = _lib.lib()


def clumps():
    """bench_bound.py's 4,096 balls of 256 bodies and radius 0.2, four apart; the centres: the centres of mass of
    the friends-of-friends groups; R = three ball radii."""
    rng = np.random.default_rng(3)
    groups, members, link = 4096, 256, 0.4
    n = groups * members
    side = int(np.ceil(groups ** (1.0 / 3.0)))
    k = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)[:groups]
    d = rng.normal(size=(n, 3))
    d *= ((link / 2) * rng.uniform(0.0, 1.0, n) ** (1.0 / 3.0) / np.linalg.norm(d, axis=1))[:, None]
    state = np.zeros((n, 10), np.float32)
    state[:, 0:3] = d + np.repeat((k - (side - 1) / 2.0) * (10 * link), members, axis=0)
    state[:, 3:6] = rng.normal(0.0, 1e-3, (n, 3))
    state[:, 9] = rng.uniform(0.5, 2.0, n)
    sim = nb.NaiveSim.from_particles(nb.SimParams(particle_num=n), None, state,
                                     placement=nb.Placement(stream=stream.cuda_stream))
    fof = sim.fof_groups(link, min_members=20, labels=False)
    return sim, fof.com, fof.velocity, 0.006, 0.6


def from_init(kind, n, m, rmin, rmax_of):
    sp = nb.SimParams(particle_num=n)
    state = nb.as_floats({"disc": nb.inits.disc_init, "spherical": nb.inits.spherical_init,
                          "uniform": nb.inits.uniform_init}[kind](sp, seed=0)).copy()
    sim = nb.NaiveSim.from_particles(sp, None, state, placement=nb.Placement(stream=stream.cuda_stream))
    x = state[:, 0:3].astype(np.float64)
    pick = np.arange(m) * (n // m)
    rmax = rmax_of(x)
    return sim, x[pick], state[pick, 3:6].astype(np.float64), rmin * rmax, rmax


CASES = [
    ("clumps 4096x256", clumps),
    ("disc 100k", lambda: from_init("disc", 100000, 256, 0.01, lambda x: 0.05 * np.ptp(x, axis=0).max())),
    ("uniform 4M", lambda: from_init("uniform", 4000000, 32768, 0.05,
                                     lambda x: (100.0 / 4e6 * np.prod(np.ptp(x, axis=0)) / 4.18879) ** (1 / 3))),
    ("spherical 2^20 all", lambda: from_init("spherical", 1 << 20, 64, 1e-3, lambda x: 4.0 * np.abs(x).max())),
]


def events(fn, reps, warmup):
    out = []
    for r in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        if r >= warmup:
            out.append(e0.elapsed_time(e1))
    return float(np.median(out))


rows = []
for ci in args.cases:
    name, make = CASES[ci]
    sim, c, vc, rmin, rmax = make()
    n, m = int(sim.sim_params().particle_num), c.shape[0]
    edges = nb.radial_edges(rmin, rmax, args.nbins)
    c, vc = np.ascontiguousarray(c), np.ascontiguousarray(vc)
    dp = C.POINTER(C.c_double)
    p = _lib.nb_halo_params()
    p.nbins, p.m, p.edges = args.nbins, m, edges.ctypes.data_as(dp)
    p.centers, p.velocities = c.ctypes.data_as(dp), vc.ctypes.data_as(dp)
    heads, bins = np.zeros(m, _lib.HALO_HEAD_DTYPE), np.zeros((m, args.nbins), _lib.RADIAL_BIN_DTYPE)
    st = _lib.nb_halo_stats()
    print("# %s: n %d, m %d, timing %d + %d calls a figure" % (name, n, m, args.warmup, args.reps), file=sys.stderr,
          flush=True)
    t_kernels = events(lambda: _lib.check(L.nb_sim_halo_profiles(sim._h, C.byref(p), None, None, C.byref(st))),
                       args.reps, args.warmup)
    tw = []
    for r in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        _lib.check(L.nb_sim_halo_profiles(sim._h, C.byref(p), heads.ctypes.data, bins.ctypes.data, C.byref(st)))
        if r >= args.warmup:
            tw.append((time.perf_counter() - t0) * 1e3)
    row = {"state": name, "label": args.label, "n": n, "m": m, "nbins": args.nbins, "rmax": rmax, "reps": args.reps,
           "kernels_ms": t_kernels, "call_median_ms": float(np.median(tw)), "call_min_ms": float(np.min(tw)),
           "tested": int(st.tested), "items": int(st.items), "cells": list(st.cells),
           "inside_edges": int(bins["count"].sum() + heads["inside_count"].sum()),
           "ps_per_test": t_kernels * 1e9 / max(int(st.tested), 1), "pruned_to": int(st.tested) / (float(n) * m),
           "ns_per_body_centre": t_kernels * 1e6 / (float(n) * m)}
    if not args.no_baselines:
        sample = np.unique(np.linspace(0, m - 1, min(m, args.sample)).astype(np.int64))
        # the loop through the C ABI with buffers made once, as the halo call is timed; warm-up calls first
        rp, ro = _lib.nb_radial_params(), _lib.nb_radial_profile()
        rp.nbins, rp.flags, rp.edges = args.nbins, 0, edges.ctypes.data_as(dp)
        rbins = np.zeros(args.nbins, _lib.RADIAL_BIN_DTYPE)

        def radial(j):
            for a in range(3):
                rp.center[a], rp.velocity[a] = c[j, a], vc[j, a]
            _lib.check(L.nb_sim_radial_profile(sim._h, C.byref(rp), C.byref(ro), rbins.ctypes.data))

        for j in sample[:args.warmup]:
            radial(j)
        tl = []
        for j in sample:
            t0 = time.perf_counter()
            radial(j)
            tl.append((time.perf_counter() - t0) * 1e3)
            if not (np.array_equal(rbins["count"], bins["count"][j]) and ro.inside_count == heads["inside_count"][j]):
                sys.exit("%s: nb_sim_radial_profile counts differently about centre %d" % (name, j))
        # the device side of one such call (its two kernels and two small copies), by HIP events
        t_radial_dev = events(lambda: radial(sample[0]), args.reps, args.warmup)
        row.update(sample=len(sample), loop_call_ms=float(np.median(tl)), loop_ms=float(np.median(tl)) * m,
                   loop_ratio=float(np.median(tl)) * m / row["call_median_ms"],
                   radial_ns_per_body=float(np.median(tl)) * 1e6 / n, radial_device_ms=t_radial_dev,
                   radial_device_ns_per_body=t_radial_dev * 1e6 / n)
        if cKDTree is not None:
            t0 = time.perf_counter()
            x = nb.as_floats(sim.read_particles())[:, 0:3].astype(np.float64)
            t_read = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            tree = cKDTree(x)
            t_build = (time.perf_counter() - t0) * 1e3
            e2 = edges * edges
            t0 = time.perf_counter()
            for j in sample:
                near = np.asarray(tree.query_ball_point(c[j], rmax * (1 + 1e-9)), dtype=np.int64)
                d = x[near] - c[j]
                cnt = np.searchsorted(e2, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], side="right")
                got = np.bincount(cnt, minlength=args.nbins + 2)
                if not (np.array_equal(got[1:args.nbins + 1], bins["count"][j]) and got[0] == heads["inside_count"][j]):
                    sys.exit("%s: the k-d tree counts differently about centre %d" % (name, j))
            t_query = (time.perf_counter() - t0) * 1e3 / len(sample) * m
            row.update(tree_read_ms=t_read, tree_build_ms=t_build, tree_query_ms=t_query,
                       tree_ms=t_read + t_build + t_query,
                       tree_ratio=(t_read + t_build + t_query) / row["call_median_ms"])
    sim.destroy()
    rows.append(row)
    print(json.dumps(row), flush=True)

lines = ["# tools/bench_halo.py: nb_sim_halo_profiles on a NaiveSim, %d log bins, ms, median of the reps (kernels: HIP "
         "events around a stats-only call; call: host clock, every output)" % args.nbins,
         "# " + nb.version(),
         "# tested: candidate distance tests (stats.tested), of m n without the grid; ps/test: kernels over tested; "
         "loop: nb_sim_radial_profile per centre, the median of `of` centres times m; tree: read_particles + cKDTree "
         "build + query_ball_point and numpy per centre, the queries scaled from the same centres; x: over the call",
         "%-20s %-8s %8s %6s %9s %9s %10s %8s %8s %7s %10s %8s %10s %8s %4s %10s" % (
             "state", "build", "n", "m", "kernels", "call", "tested", "of m n", "ps/test", "items", "loop", "x", "tree",
             "x", "of", "ns/body")]
for r in rows:
    lines.append("%-20s %-8s %8d %6d %9.3f %9.3f %10.3e %8.2e %8.1f %7d %10s %8s %10s %8s %4s %10.4f" % (
        r["state"], r["label"] or "-", r["n"], r["m"], r["kernels_ms"], r["call_median_ms"], r["tested"], r["pruned_to"],
        r["ps_per_test"], r["items"], "%.1f" % r["loop_ms"] if "loop_ms" in r else "-",
        "%.1f" % r["loop_ratio"] if "loop_ratio" in r else "-", "%.1f" % r["tree_ms"] if "tree_ms" in r else "-",
        "%.1f" % r["tree_ratio"] if "tree_ratio" in r else "-", r.get("sample", "-"), r["ns_per_body_centre"]))
    if "radial_ns_per_body" in r and r["pruned_to"] > 0.99:
        lines.append("#   %s: every body a candidate of every centre: %.4f ns per body and centre; one nb_sim_radial_profile "
                     "call %.4f ns per body by the host clock, %.4f by HIP events around it (%.4f ms: radial_bins_kernel, "
                     "the finish and two small copies)" % (r["state"], r["ns_per_body_centre"], r["radial_ns_per_body"],
                                                          r["radial_device_ns_per_body"], r["radial_device_ms"]))
print("\n".join(lines))
if args.table:
    with open(args.table, "a") as f:
        f.write("\n".join(lines) + "\n")
print(json.dumps({"bench": "halo_profiles", "rows": len(rows), "device": nb.version()}))
