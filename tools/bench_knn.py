"""k-nearest-neighbour density benchmark (nb_sim_knn, csrc/nb_knn.hip).  Per case and k: the kernels alone -- HIP
events on the simulator's stream around a call that asks for the stats only -- and the wall time of whole calls
(host clock: launches, the copies of r2, kth, mass_in and density, the synchronisation), each as minimum and median
over --reps calls after --warmup.  --baseline adds what the call replaces, read_particles plus
scipy.spatial.cKDTree.query(k + 1) on the host, and checks that its distances agree with sqrt(r2) to binary32
resolution (they are not the rule's, so they are not compared with ==).  The cases of DESIGN.md 6i: the
100,000-body disc, 2^20 bodies spherical and 4,000,000 uniform, and three concentrated states of 2^20 bodies: all
within 2^-20 of the extent that one far outlier sets, two tight blobs far apart, and 1,024 distinct points of 1,024
coincident bodies each.  Prints one JSON line per row, a table and a summary line.  Secondary to bench.py."""
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

# name, init, n, concentration, baseline possible
CASES = [
    ("disc 100k", "disc", 100_000, None, True),
    ("sphere 2^20", "spherical", 1 << 20, None, True),
    ("uniform 4M", "uniform", 4_000_000, None, True),
    ("2^20 + outlier", "uniform", 1 << 20, "outlier", True),
    ("2^20 two blobs", "uniform", 1 << 20, "blobs", True),
    ("2^20 at 1024 pts", "uniform", 1 << 20, "points", False),
]

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, nargs="*", default=list(range(len(CASES))), help="indices into the case list")
ap.add_argument("--ks", type=int, nargs="*", default=[6, 32])
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--baseline", type=int, default=0, help="timed read_particles + cKDTree runs per row (0: none)")
ap.add_argument("--span", type=int, default=0, help='"knn_span_cells" (0: the default)')
ap.add_argument("--block-queries", type=int, default=0, help='"knn_block_queries" (0: the default)')
ap.add_argument("--table", default="", help="also write the table to this file")
args = ap.parse_args()

if nb.device_count() < 1:
    sys.exit("bench_knn needs a HIP device (no CPU fallback)")


def make(init, n, conc, stream):
    sp = nb.SimParams(particle_num=n)
    state = nb.as_floats({"uniform": nb.inits.uniform_init, "disc": nb.inits.disc_init,
                          "spherical": nb.inits.spherical_init}[init](sp, seed=1)).copy()
    rng = np.random.default_rng(2)
    if conc == "outlier":  # a cube of side 1 and one body 2^20 sides away: the cube is within 2^-20 of the extent
        state[:, 0:3] = rng.uniform(0.0, 1.0, (n, 3))
        state[0, 0:3] = (float(1 << 20), 0.0, 0.0)
    elif conc == "blobs":  # two cubes of side 1e-3, 100 apart
        state[:, 0:3] = rng.uniform(0.0, 1e-3, (n, 3))
        state[n // 2:, 0] += 100.0
    elif conc == "points":  # 1,024 points, every one 1,024 times
        pts = rng.uniform(-1.0, 1.0, (1024, 3)).astype(np.float32)
        state[:, 0:3] = pts[rng.permutation(n) % 1024]
    return nb.NaiveSim.from_particles(sp, None, state, placement=nb.Placement(stream=stream.cuda_stream))


def cpu_distances(state, k):
    """What the call replaces: the k-th neighbour distance from a k-d tree on the host."""
    from scipy.spatial import cKDTree
    pos = state[:, 0:3].astype(np.float64)
    d, _ = cKDTree(pos).query(pos, k + 1)
    return d[:, k]


try:
    import scipy.spatial  # noqa: F401
    have_scipy = True
except ImportError:
    have_scipy = False

rows = []
stream = torch.cuda.Stream()
for ci in args.cases:
    name, init, n, conc, can_base = CASES[ci]
    sim = make(init, n, conc, stream)
    if args.span:
        sim.set_tuning("knn_span_cells", args.span)
    if args.block_queries:
        sim.set_tuning("knn_block_queries", args.block_queries)
    for k in args.ks:
        p = _lib.nb_knn_params()
        p.k = k
        st = _lib.nb_knn_stats()
        tk, tw = [], []
        for r in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            _lib.check(_lib.lib().nb_sim_knn(sim._h, C.byref(p), None, None, None, None, C.byref(st)))
            e1.record(stream)
            e1.synchronize()
            t0 = time.perf_counter()
            d = sim.knn_density(k)
            t1 = time.perf_counter()
            if r >= args.warmup:
                tk.append(e0.elapsed_time(e1))
                tw.append((t1 - t0) * 1e3)
        tk, tw = np.array(tk), np.array(tw)
        s = d.stats
        row = {"case": name, "n": n, "k": k, "reps": args.reps, "kernels_min_ms": float(tk.min()),
               "kernels_median_ms": float(np.median(tk)), "call_min_ms": float(tw.min()),
               "call_median_ms": float(np.median(tw)), "counted": s.counted, "degenerate": s.degenerate,
               "peak_index": s.peak_index}
        if args.baseline > 0 and can_base and have_scipy:
            tb = []
            for _ in range(args.baseline):
                t0 = time.perf_counter()
                dist = cpu_distances(nb.as_floats(sim.read_particles()), k)
                tb.append((time.perf_counter() - t0) * 1e3)
            row["baseline_min_ms"], row["baseline_median_ms"] = float(np.min(tb)), float(np.median(tb))
            # the tree's distance is sqrt of a sum of squared binary64 differences in another order: it agrees
            # with sqrt(r2) to a few units of binary64, far inside binary32 resolution (2^-23 relative)
            rk = d.r_k
            row["distances_agree"] = bool(np.all(np.abs(dist - rk) <= 2.0 ** -23 * rk))
        rows.append(row)
        print(json.dumps(row), flush=True)
    sim.destroy()

lines = ["# tools/bench_knn.py: nb_sim_knn on a NaiveSim, ms per call, minimum and median of %d after %d warm-up calls "
         "(kernels: HIP events around a stats-only call; call: host clock around the whole call with r2, kth, mass_in "
         "and density)" % (args.reps, args.warmup),
         "# " + nb.version(),
         "# baseline: read_particles + scipy.spatial.cKDTree.query(k + 1), ms, median of %d; agree: its distances "
         "against sqrt(r2) to binary32 resolution" % args.baseline,
         "%-17s %9s %3s %9s %9s %9s %9s %10s %10s %6s" % (
             "case", "n", "k", "kern min", "kern med", "call min", "call med", "degenerate", "baseline", "agree")]
for r in rows:
    lines.append("%-17s %9d %3d %9.4f %9.4f %9.4f %9.4f %10d %10s %6s" % (
        r["case"], r["n"], r["k"], r["kernels_min_ms"], r["kernels_median_ms"], r["call_min_ms"], r["call_median_ms"],
        r["degenerate"], "%.1f" % r["baseline_median_ms"] if "baseline_median_ms" in r else "-",
        {True: "yes", False: "NO"}.get(r.get("distances_agree"), "-")))
print("\n".join(lines))
if args.table:
    with open(args.table, "w") as f:
        f.write("\n".join(lines) + "\n")
print(json.dumps({"bench": "knn_density", "rows": len(rows), "device": nb.version()}))
