"""Smoothed-map benchmark (nb_sim_smooth_map, csrc/nb_smooth.hip).  Per case: the smoothing lengths come from one
knn_density(k) call on the same state, timed on its own (the knn column: it is a separate call and not part of the
others); then the median wall time of whole smoothed-map calls with those lengths (host clock: the upload of s, the
launches, the read of the entry count, the copy of W * H * (4 + 8 P) bytes into pageable memory) and beside it the
kernels alone -- HIP events on the simulator's stream around a call that asks for the stats only.  Beside each, the
same two figures of nb_sim_map on the same state and grid.  The cases of DESIGN.md 6j: the 100,000-body disc at 512 x
512, 2^20 bodies at 1024 x 1024, 4,000,000 bodies at 1920 x 1080, each at k = 32 with the default floor (2 pixels)
and cap (64 pixels); 2^20 bodies with every body in one tile; and the 2^20-body case with the cap at 8, 64 and 256
pixels, the number of tile entries beside each.  --baseline adds what the call replaces, read_particles plus the numpy
restatement (tests/smooth_ref.py, the per-body loop), on the first --baseline-bodies bodies (the loop takes minutes at
2^20; the column says how many it ran and the time is for those alone), and compares its counts with the device's
where it ran them all.  Prints one JSON line per case, a table and a summary line.  Secondary to bench.py."""
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
WIDE = (-1.0, 1.0, -0.5625, 0.5625)
# name, init, n, (W, H), extent, cap in pixels, every body in one tile
CASES = [
    ("disc 100k", "disc", 100_000, (512, 512), SQUARE, 64, False),
    ("sphere 2^20", "spherical", 1 << 20, (1024, 1024), SQUARE, 64, False),
    ("uniform 4M", "uniform", 4_000_000, (1920, 1080), WIDE, 64, False),
    ("2^20 one tile", "spherical", 1 << 20, (1024, 1024), SQUARE, 64, True),
    ("2^20 cap 8", "spherical", 1 << 20, (1024, 1024), SQUARE, 8, False),
    ("2^20 cap 256", "spherical", 1 << 20, (1024, 1024), SQUARE, 256, False),
]

ap = argparse.ArgumentParser()
ap.add_argument("--sims", nargs="*", default=["naive"])
ap.add_argument("--cases", type=int, nargs="*", default=list(range(len(CASES))), help="indices into the case list")
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--k", type=int, default=32)
ap.add_argument("--baseline", type=int, default=0, help="timed read_particles + numpy runs per case (0: none)")
ap.add_argument("--baseline-bodies", type=int, default=100_000, help="bodies the numpy loop runs (the first ones)")
ap.add_argument("--table", default="", help="also write the table to this file")
args = ap.parse_args()

if nb.device_count() < 1:
    sys.exit("bench_smooth needs a HIP device (no CPU fallback)")


def make(kind, init, n, grid, one_tile, stream):
    sp = nb.SimParams(particle_num=n)
    state = nb.as_floats({"uniform": nb.inits.uniform_init, "disc": nb.inits.disc_init,
                          "spherical": nb.inits.spherical_init}[init](sp, seed=1)).copy()
    if one_tile:  # the tile of pixels [296, 304) x [696, 704) of the square window
        rng = np.random.default_rng(2)
        w, h = grid
        state[:, 0] = -1.0 + 2.0 * (296 + rng.uniform(0.01, 7.99, n)) / w
        state[:, 1] = -1.0 + 2.0 * (696 + rng.uniform(0.01, 7.99, n)) / h
    pl = nb.Placement(stream=stream.cuda_stream)
    if kind == "naive":
        return nb.NaiveSim.from_particles(sp, None, state, placement=pl)
    sim = nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(0.75), state, placement=pl)
    sim.encode()
    sim.wait()
    return sim


def timed(stream, whole, kernels, reps, warmup):
    tw, tk = [], []
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        out = whole()
        t1 = time.perf_counter()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        kernels()
        e1.record(stream)
        e1.synchronize()
        if r >= warmup:
            tw.append((t1 - t0) * 1e3)
            tk.append(e0.elapsed_time(e1))
    return out, float(np.median(tw)), float(np.min(tw)), float(np.median(tk)), float(np.min(tk))


rows = []
stream = torch.cuda.Stream()
for ci in args.cases:
    name, init, n, grid, extent, cap, one_tile = CASES[ci]
    for kind in args.sims:
        sim = make(kind, init, n, grid, one_tile, stream)
        w, h = grid
        pixel = max((extent[1] - extent[0]) / w, (extent[3] - extent[2]) / h)
        kw = dict(extent=extent, axis=Z, center=(0.0, 0.0, 0.0))
        tknn = []
        for r in range(3):
            t0 = time.perf_counter()
            s = sim.knn_density(args.k, density=False).r_k
            tknn.append((time.perf_counter() - t0) * 1e3)
        sp = _lib.nb_smooth_params()
        sp.width, sp.height, sp.flags = w, h, _lib.NB_SMOOTH_VELOCITY
        mp = _lib.nb_map_params()
        mp.width, mp.height, mp.flags = w, h, _lib.NB_MAP_VELOCITY
        for p in (sp, mp):
            for k in range(3):
                p.axis[k] = Z[k]
            p.x_range[0], p.x_range[1], p.y_range[0], p.y_range[1] = extent
            p.depth_range[0], p.depth_range[1] = -np.inf, np.inf
        sp.s_min, sp.s_max = 2.0 * pixel, cap * pixel
        sst, mst = _lib.nb_smooth_stats(), _lib.nb_map_stats()
        L = _lib.lib()
        if L.nb_sim_smooth_map(sim._h, C.byref(sp), s.ctypes.data, None, None, C.byref(sst)) != 0:
            row = {"case": name, "sim": kind, "n": n, "width": w, "height": h, "k": args.k, "cap_pixels": cap,
                   "knn_ms": float(np.median(tknn)), "refused": L.nb_last_error().decode()}
            sim.destroy()
            rows.append(row)
            print(json.dumps(row), flush=True)
            continue
        sm, call, call_min, kern, kern_min = timed(
            stream, lambda: sim.smoothed_map(w, h, smoothing=s, s_max=cap * pixel, **kw),
            lambda: _lib.check(L.nb_sim_smooth_map(sim._h, C.byref(sp), s.ctypes.data, None, None, C.byref(sst))),
            args.reps, args.warmup)
        pm, mcall, _, mkern, _ = timed(
            stream, lambda: sim.projected_map(w, h, **kw),
            lambda: _lib.check(L.nb_sim_map(sim._h, C.byref(mp), None, None, C.byref(mst))), args.reps, args.warmup)
        st = sm.stats
        row = {"case": name, "sim": kind, "n": n, "width": w, "height": h, "k": args.k, "cap_pixels": cap,
               "reps": args.reps, "knn_ms": float(np.median(tknn)), "call_median_ms": call, "call_min_ms": call_min,
               "kernels_median_ms": kern, "kernels_min_ms": kern_min, "map_call_median_ms": mcall,
               "map_kernels_median_ms": mkern, "tile_entries": st.tile_entries, "pairs": st.pairs,
               "deposited": st.deposited, "raised": st.raised, "lowered": st.lowered, "max_count": st.max_count}
        if args.baseline > 0:
            from tests import smooth_ref
            m = min(n, args.baseline_bodies)
            tb = []
            for _ in range(args.baseline):
                t0 = time.perf_counter()
                state = nb.as_floats(sim.read_particles())
                ref = smooth_ref.smooth64(state[:m], s[:m], w, h, extent, s_min=2.0 * pixel, s_max=cap * pixel, axis=Z)
                tb.append((time.perf_counter() - t0) * 1e3)
            row["baseline_bodies"] = m
            row["baseline_median_ms"] = float(np.median(tb))
            if m == n:
                row["baseline_counts_equal"] = bool(np.array_equal(ref["counts"], sm.counts))
        sim.destroy()
        rows.append(row)
        print(json.dumps(row), flush=True)

lines = ["# tools/bench_smooth.py: nb_sim_smooth_map with s = r_k of knn_density(k = %d), six planes, ms per call, median "
         "of %d (call: host clock around the whole call with its copies; kernels: HIP events around a stats-only call)"
         % (args.k, args.reps),
         "# " + nb.version(),
         "# knn: the separate knn_density call that made s (not in the other columns); map: nb_sim_map on the same state "
         "and grid; cap: s_max in pixels (s_min: 2); entries: tile_entries; baseline: read_particles + the numpy "
         "restatement's loop over the first `of` bodies, ms; equal: its counts against the device's (all bodies only)",
         "%-14s %-6s %8s %10s %4s %8s %9s %9s %9s %9s %9s %10s %12s %8s %9s %7s %6s" % (
             "case", "sim", "n", "grid", "cap", "knn", "call", "call min", "kernels", "map call", "map kern",
             "entries", "pairs", "largest", "baseline", "of", "equal")]
for r in rows:
    if "refused" in r:
        lines.append("%-14s %-6s %8d %10s %4d %8.2f refused: %s" % (
            r["case"], r["sim"], r["n"], "%dx%d" % (r["width"], r["height"]), r["cap_pixels"], r["knn_ms"], r["refused"]))
        continue
    lines.append("%-14s %-6s %8d %10s %4d %8.2f %9.3f %9.3f %9.3f %9.3f %9.3f %10d %12d %8d %9s %7s %6s" % (
        r["case"], r["sim"], r["n"], "%dx%d" % (r["width"], r["height"]), r["cap_pixels"], r["knn_ms"],
        r["call_median_ms"], r["call_min_ms"], r["kernels_median_ms"], r["map_call_median_ms"],
        r["map_kernels_median_ms"], r["tile_entries"], r["pairs"], r["max_count"],
        "%.0f" % r["baseline_median_ms"] if "baseline_median_ms" in r else "-",
        r.get("baseline_bodies", "-"), {True: "yes", False: "NO"}.get(r.get("baseline_counts_equal"), "-")))
print("\n".join(lines))
if args.table:
    with open(args.table, "w") as f:
        f.write("\n".join(lines) + "\n")
print(json.dumps({"bench": "smoothed_map", "rows": len(rows), "device": nb.version()}))
