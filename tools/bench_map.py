"""Projected-map benchmark (nb_sim_map, csrc/nb_map.hip).  Per case and simulator: the median wall time of
whole calls (host clock: launches, the copy of W * H * (4 + 8 P) bytes into pageable memory, the
synchronisation) on an idle simulator stream, and beside it the kernels alone -- HIP events on the
simulator's stream around a call that asks for the stats only, so that nothing but 136 bytes is copied.
Large grids are dominated by the copy; the two columns say which is which.  The cases of DESIGN.md 6f: the
100,000-body disc face-on at 512 x 512 with and without velocities, 2^20 bodies at 1024 x 1024, 4,000,000
bodies at 1920 x 1080, and 2^20 bodies with every body in one cell and in one tile of 1024 x 1024;
--baseline adds what the call replaces, read_particles plus numpy (np.add.at per plane), and compares its
counts with the device's.  Prints one JSON line per case, a table and a summary line.  Secondary to
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

Z = (0.0, 0.0, 1.0)
SQUARE = (-1.0, 1.0, -1.0, 1.0)
# name, init, n, (W, H), extent, axis, velocities, concentration (None, "cell" or "tile")
CASES = [
    ("disc 100k vel", "disc", 100_000, (512, 512), SQUARE, Z, True, None),
    ("disc 100k mass", "disc", 100_000, (512, 512), SQUARE, Z, False, None),
    ("sphere 2^20", "spherical", 1 << 20, (1024, 1024), SQUARE, Z, True, None),
    ("uniform 4M", "uniform", 4_000_000, (1920, 1080), (-1.0, 1.0, -0.5625, 0.5625), Z, True, None),
    ("2^20 one cell", "spherical", 1 << 20, (1024, 1024), SQUARE, Z, True, "cell"),
    ("2^20 one tile", "spherical", 1 << 20, (1024, 1024), SQUARE, Z, True, "tile"),
]

ap = argparse.ArgumentParser()
ap.add_argument("--sims", nargs="*", default=["naive", "tree"])
ap.add_argument("--cases", type=int, nargs="*", default=list(range(len(CASES))), help="indices into the case list")
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--baseline", type=int, default=0, help="timed read_particles + numpy runs per case (0: none)")
ap.add_argument("--table", default="", help="also write the table to this file")
args = ap.parse_args()

if nb.device_count() < 1:
    sys.exit("bench_map needs a HIP device (no CPU fallback)")


def make(kind, init, n, grid, conc, stream):
    sp = nb.SimParams(particle_num=n)
    state = nb.as_floats({"uniform": nb.inits.uniform_init, "disc": nb.inits.disc_init,
                          "spherical": nb.inits.spherical_init}[init](sp, seed=1)).copy()
    if conc:  # cell (300, 700) of the square window, or the tile that holds it
        rng = np.random.default_rng(2)
        (w, h), span = grid, 1.0 if conc == "cell" else 8.0
        i0, j0 = (300, 700) if conc == "cell" else (296, 696)
        state[:, 0] = -1.0 + 2.0 * (i0 + rng.uniform(0.01, span - 0.01, n)) / w
        state[:, 1] = -1.0 + 2.0 * (j0 + rng.uniform(0.01, span - 0.01, n)) / h
    pl = nb.Placement(stream=stream.cuda_stream)
    if kind == "naive":
        return nb.NaiveSim.from_particles(sp, None, state, placement=pl)
    sim = nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(0.75), state, placement=pl)
    sim.encode()  # tree order (and, past 524,288 bodies, the other buffer set)
    sim.wait()
    return sim


def numpy_map(state, grid, extent, axis, velocities, c, vc):
    """What the call replaces: the rule of include/nbody.h on the host, one np.add.at per plane."""
    from tests import map_ref
    (w, h) = grid
    x, v, m = state[:, 0:3].astype(np.float64), state[:, 3:6].astype(np.float64), state[:, 9].astype(np.float64)
    n_hat, e1, e2 = map_ref.frame(axis)
    xe, ye = map_ref.edges(extent[0], extent[1], w), map_ref.edges(extent[2], extent[3], h)
    dot = lambda p, q: (p[:, 0] * q[0] + p[:, 1] * q[1]) + p[:, 2] * q[2]  # noqa: E731  (the rule's order)
    d, u = x - c, v - vc
    a, b = dot(d, e1), dot(d, e2)
    inside = (a >= xe[0]) & (a < xe[w]) & (b >= ye[0]) & (b < ye[h])
    i, j = np.searchsorted(xe, a[inside], side="right") - 1, np.searchsorted(ye, b[inside], side="right") - 1
    counts = np.zeros((h, w), np.uint32)
    np.add.at(counts, (j, i), 1)
    terms = [m]
    if velocities:
        ua, ub, los = dot(u, e1), dot(u, e2), dot(u, n_hat)
        terms += [m * ua, m * ub, m * los, m * los * los, m * (u * u).sum(1)]
    planes = np.zeros((len(terms), h, w))
    for k, t in enumerate(terms):
        np.add.at(planes[k], (j, i), t[inside])
    return counts, planes


rows = []
stream = torch.cuda.Stream()
for ci in args.cases:
    name, init, n, grid, extent, axis, velocities, conc = CASES[ci]
    for kind in args.sims:
        sim = make(kind, init, n, grid, conc, stream)
        centre = (0.0, 0.0, 0.0) if conc else "com"  # (the concentrated states' cell is placed about the origin)
        call = lambda: sim.projected_map(grid[0], grid[1], extent=extent, axis=axis, center=centre,  # noqa: E731
                                         velocities=velocities)
        p = _lib.nb_map_params()
        p.width, p.height = grid
        p.flags = (0 if conc else _lib.NB_MAP_CENTER_COM) | (_lib.NB_MAP_VELOCITY if velocities else 0)
        for k in range(3):
            p.axis[k] = axis[k]
        p.x_range[0], p.x_range[1], p.y_range[0], p.y_range[1] = extent
        p.depth_range[0], p.depth_range[1] = -np.inf, np.inf
        st = _lib.nb_map_stats()
        tw, tk = [], []
        for r in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            pm = call()
            t1 = time.perf_counter()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            _lib.check(_lib.lib().nb_sim_map(sim._h, C.byref(p), None, None, C.byref(st)))
            e1.record(stream)
            e1.synchronize()
            if r >= args.warmup:
                tw.append((t1 - t0) * 1e3)
                tk.append(e0.elapsed_time(e1))
        tw, tk = np.array(tw), np.array(tk)
        planes = 6 if velocities else 1
        row = {"case": name, "sim": kind, "n": n, "width": grid[0], "height": grid[1], "planes": planes,
               "reps": args.reps, "call_median_ms": float(np.median(tw)), "call_min_ms": float(tw.min()),
               "call_max_ms": float(tw.max()), "kernels_median_ms": float(np.median(tk)),
               "kernels_min_ms": float(tk.min()), "copied_bytes": grid[0] * grid[1] * (4 + 8 * planes),
               "binned": pm.binned_count, "max_count": pm.max_count}
        if args.baseline > 0:
            tb = []
            for _ in range(args.baseline):
                t0 = time.perf_counter()
                counts, _ = numpy_map(nb.as_floats(sim.read_particles()), grid, extent, axis, velocities, pm.center,
                                      pm.velocity)  # (the centre of mass the device used)
                tb.append((time.perf_counter() - t0) * 1e3)
            row["baseline_median_ms"] = float(np.median(tb))
            row["baseline_counts_equal"] = bool(np.array_equal(counts, pm.counts))
        sim.destroy()
        rows.append(row)
        print(json.dumps(row), flush=True)

lines = ["# tools/bench_map.py: nb_sim_map, ms per call, median of %d (call: host clock around the whole call with "
         "its copy; kernels: HIP events around a stats-only call)" % args.reps,
         "# " + nb.version(),
         "# copied: MB the whole call returns; largest: bodies in the fullest cell; baseline: read_particles + numpy "
         "(np.add.at), ms; equal: its counts against the device's",
         "%-16s %-6s %9s %10s %2s %9s %9s %9s %9s %8s %9s %10s %6s" % (
             "case", "sim", "n", "grid", "P", "call", "call min", "kernels", "kern min", "copied", "largest",
             "baseline", "equal")]
for r in rows:
    lines.append("%-16s %-6s %9d %10s %2d %9.4f %9.4f %9.4f %9.4f %8.1f %9d %10s %6s" % (
        r["case"], r["sim"], r["n"], "%dx%d" % (r["width"], r["height"]), r["planes"], r["call_median_ms"],
        r["call_min_ms"], r["kernels_median_ms"], r["kernels_min_ms"], r["copied_bytes"] / 1e6, r["max_count"],
        "%.1f" % r["baseline_median_ms"] if "baseline_median_ms" in r else "-",
        {True: "yes", False: "NO"}.get(r.get("baseline_counts_equal"), "-")))
print("\n".join(lines))
if args.table:
    with open(args.table, "w") as f:
        f.write("\n".join(lines) + "\n")
print(json.dumps({"bench": "projected_map", "rows": len(rows), "device": nb.version()}))
