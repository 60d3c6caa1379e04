"""Phase-map benchmark (nb_phase_map_sim, csrc/nb_phase.hip).  Per case and simulator: the median wall time of whole
calls (host clock: the upload of the edges, launches, the copy of W * H * (4 + 8 P) bytes into pageable memory, the
synchronisation) on an idle simulator stream, and beside it the kernels alone -- HIP events on the simulator's stream
around a call that asks for the stats only.  Beside every row two comparisons on the same state and grid in the same
process: projected_map(velocities=True), call and kernels, and what the call replaces, read_particles plus
numpy.histogram2d (one per plane).  The cases of DESIGN.md 6q: the 100,000-body disc as R - u_phi at 512 x 512,
2^20 spherical bodies as r - u_r with log r at 1024 x 1024, 4,000,000 uniform bodies as a - b weighted by w at
1920 x 1080 (the map's own planes, so that row against the map is the cost of searching arbitrary edges), and 2^20
bodies in one cell.
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

Z = (0.0, 0.0, 1.0)
SQUARE = (-1.0, 1.0, -1.0, 1.0)
# name, init, n, x (name, lo, hi, cells, log), y, weight, axis, the map's extent, every body in one cell
CASES = [
    ("disc 100k R-u_phi", "disc", 100_000, ("R", 0.0, 1.0, 512, False), ("u_phi", -0.15, 0.15, 512, False), "w", Z,
     SQUARE, False),
    ("sphere 2^20 r-u_r", "spherical", 1 << 20, ("r", 0.01, 1.0, 1024, True), ("u_r", -0.5, 0.5, 1024, False), "u_t",
     Z, SQUARE, False),
    ("uniform 4M a-b-w", "uniform", 4_000_000, ("a", -1.0, 1.0, 1920, False), ("b", -0.5625, 0.5625, 1080, False),
     "w", Z, (-1.0, 1.0, -0.5625, 0.5625), False),
    ("2^20 one cell", "spherical", 1 << 20, ("a", -1.0, 1.0, 1024, False), ("b", -1.0, 1.0, 1024, False), "w", Z,
     SQUARE, True),
]

ap = argparse.ArgumentParser()
ap.add_argument("--sims", nargs="*", default=["naive", "tree"])
ap.add_argument("--cases", type=int, nargs="*", default=list(range(len(CASES))), help="indices into the case list")
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--baseline", type=int, default=0, help="timed read_particles + numpy runs per case (0: none)")
ap.add_argument("--table", default="", help="also write the table to this file")
args = ap.parse_args()

if nb.device_count() < 1:
    sys.exit("bench_phase needs a HIP device (no CPU fallback)")


def make(kind, init, n, one_cell, stream):
    sp = nb.SimParams(particle_num=n)
    state = nb.as_floats({"uniform": nb.inits.uniform_init, "disc": nb.inits.disc_init,
                          "spherical": nb.inits.spherical_init}[init](sp, seed=1)).copy()
    if one_cell:  # cell (300, 700) of the square window at 1024 x 1024, as tools/bench_map.py's
        rng = np.random.default_rng(2)
        state[:, 0] = -1.0 + 2.0 * (300 + rng.uniform(0.01, 0.99, n)) / 1024
        state[:, 1] = -1.0 + 2.0 * (700 + rng.uniform(0.01, 0.99, n)) / 1024
    pl = nb.Placement(stream=stream.cuda_stream)
    if kind == "naive":
        return nb.NaiveSim.from_particles(sp, None, state, placement=pl)
    sim = nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(0.75), state, placement=pl)
    sim.encode()  # tree order (and, past 524,288 bodies, the other buffer set)
    sim.wait()
    return sim


def numpy_phase(state, x, y, weight, xe, ye, axis, c, vc):
    """What the call replaces: the quantities on the host, one numpy.histogram2d per plane."""
    from tests import phase_ref
    q = phase_ref.quantities(state[:, 0:3].astype(np.float64), state[:, 3:6].astype(np.float64),
                             state[:, 9].astype(np.float64), axis, c, vc)
    ok = np.isfinite(q[x]) & np.isfinite(q[y]) & np.isfinite(q[weight])
    qx, qy, m, w = q[x][ok], q[y][ok], q["mass"][ok], q[weight][ok]
    counts = np.histogram2d(qy, qx, bins=(ye, xe))[0]
    planes = [np.histogram2d(qy, qx, bins=(ye, xe), weights=t)[0] for t in (m, m * w, m * w * w)]
    return counts, planes


def timed(stream, whole, kernels):
    tw, tk = [], []
    for r in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        out = whole()
        t1 = time.perf_counter()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        kernels()
        e1.record(stream)
        e1.synchronize()
        if r >= args.warmup:
            tw.append((t1 - t0) * 1e3)
            tk.append(e0.elapsed_time(e1))
    return out, float(np.median(tw)), float(np.median(tk)), float(np.min(tk))


rows = []
stream = torch.cuda.Stream()
DP = C.POINTER(C.c_double)
for ci in args.cases:
    name, init, n, xs, ys, weight, axis, extent, one_cell = CASES[ci]
    for kind in args.sims:
        sim = make(kind, init, n, one_cell, stream)
        centre = (0.0, 0.0, 0.0) if one_cell else "com"
        xe, ye = nb.phase_edges(*xs[1:]), nb.phase_edges(*ys[1:])
        W, H = xs[3], ys[3]
        p = _lib.nb_phase_params()
        p.width, p.height = W, H
        p.flags = _lib.NB_PHASE_WEIGHT | (0 if one_cell else _lib.NB_PHASE_CENTER_COM)
        p.x, p.y, p.q = nb.phase_quantity(xs[0]), nb.phase_quantity(ys[0]), nb.phase_quantity(weight)
        p.x_edges, p.y_edges = xe.ctypes.data_as(DP), ye.ctypes.data_as(DP)
        p.step_num = _lib.NB_PHASE_ANY_STEP
        mp = _lib.nb_map_params()
        mp.width, mp.height = W, H
        mp.flags = _lib.NB_MAP_VELOCITY | (0 if one_cell else _lib.NB_MAP_CENTER_COM)
        for k in range(3):
            p.axis[k] = mp.axis[k] = axis[k]
        mp.x_range[0], mp.x_range[1], mp.y_range[0], mp.y_range[1] = extent
        mp.depth_range[0], mp.depth_range[1] = -np.inf, np.inf
        st, mst = _lib.nb_phase_stats(), _lib.nb_map_stats()
        L = _lib.lib()
        pm, call_ms, kern_ms, kern_min = timed(
            stream, lambda: sim.phase_map(xs[0], ys[0], x_edges=xe, y_edges=ye, weight=weight, axis=axis, center=centre),
            lambda: _lib.check(L.nb_phase_map_sim(sim._h, C.byref(p), None, None, C.byref(st))))
        row = {"case": name, "sim": kind, "n": n, "width": W, "height": H, "x": xs[0], "y": ys[0], "weight": weight,
               "reps": args.reps, "call_median_ms": call_ms, "kernels_median_ms": kern_ms, "kernels_min_ms": kern_min,
               "copied_bytes": W * H * (4 + 8 * 3), "binned": pm.stats.binned_count,
               "undefined": pm.stats.undefined_count, "max_count": pm.stats.max_count}
        _, row["map_call_median_ms"], row["map_kernels_median_ms"], _ = timed(
            stream, lambda: sim.projected_map(W, H, extent=extent, axis=axis, center=centre, velocities=True),
            lambda: _lib.check(L.nb_sim_map(sim._h, C.byref(mp), None, None, C.byref(mst))))
        row["call_over_map"] = row["call_median_ms"] / row["map_call_median_ms"]
        row["kernels_over_map"] = row["kernels_median_ms"] / row["map_kernels_median_ms"]
        if args.baseline > 0:
            tb = []
            for _ in range(args.baseline):
                t0 = time.perf_counter()
                counts, _ = numpy_phase(nb.as_floats(sim.read_particles()), xs[0], ys[0], weight, xe, ye, axis,
                                        pm.stats.center, pm.stats.velocity)
                tb.append((time.perf_counter() - t0) * 1e3)
            row["baseline_median_ms"] = float(np.median(tb))
            # (histogram2d closes the last bin on the right: a body exactly on the last edge may differ)
            row["baseline_counts_differ"] = int(np.abs(counts - pm.counts).sum())
        sim.destroy()
        rows.append(row)
        print(json.dumps(row), flush=True)

lines = ["# tools/bench_phase.py: nb_phase_map_sim with a weight (3 planes), ms per call, median of %d (call: host "
         "clock around the whole call with its copy; kernels: HIP events around a stats-only call)" % args.reps,
         "# " + nb.version(),
         "# map: projected_map(velocities=True), 6 planes, same state and "
         "grid; /map: phase over map; baseline: read_particles + numpy.histogram2d, ms",
         "%-18s %-6s %9s %10s %9s %9s %9s %9s %9s %7s %7s %10s" % (
             "case", "sim", "n", "grid", "call", "kernels", "kern min", "map call", "map kern", "call/map",
             "kern/map", "baseline")]
for r in rows:
    lines.append("%-18s %-6s %9d %10s %9.4f %9.4f %9.4f %9.4f %9.4f %7.3f %7.3f %10s" % (
        r["case"], r["sim"], r["n"], "%dx%d" % (r["width"], r["height"]), r["call_median_ms"], r["kernels_median_ms"],
        r["kernels_min_ms"], r["map_call_median_ms"], r["map_kernels_median_ms"], r["call_over_map"], r["kernels_over_map"],
        "%.1f" % r["baseline_median_ms"] if "baseline_median_ms" in r else "-"))
print("\n".join(lines))
if args.table:
    with open(args.table, "w") as f:
        f.write("\n".join(lines) + "\n")
print(json.dumps({"bench": "phase_map", "rows": len(rows), "device": nb.version()}))
