"""Radial-profile benchmark (nb_sim_radial_profile, csrc/nb_radial.hip): wall time per call, host clock
around the whole call (launches, the two small copies, the synchronisation), on an idle simulator
stream, with a moments-only diagnostics() call timed beside it in the same process.  The cases of
DESIGN.md 6d: the 100,000-body disc in annuli, 2^20 bodies in 64 and 256 shells, 4,000,000 bodies in 128,
the two degenerate inputs (one bin holding every body; the disc -- most of its mass in one body at the
centre -- in spherical shells), each on both simulators; --baseline adds what the call replaces,
read_particles plus the numpy restatement of the rule (tests/radial_ref.py).  Prints one JSON line per
case, a table and a summary line.  Secondary to bench.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wgpu_n_body_amd as nb  # noqa: E402

# name, init, n, nbins, (rmin, rmax, log), axis (None: spherical), centre
CASES = [
    ("disc 100k annuli", "disc", 100_000, 64, (0.02, 1.2, True), (0.0, 0.0, 1.0), "com"),
    ("sphere 2^20 b64", "spherical", 1 << 20, 64, (0.02, 1.2, True), None, "com"),
    ("sphere 2^20 b256", "spherical", 1 << 20, 256, (0.02, 1.2, True), None, "com"),
    ("uniform 4M b128", "uniform", 4_000_000, 128, (0.05, 1.8, True), None, "com"),
    ("one bin 2^20", "spherical", 1 << 20, 1, (0.0, 10.0, False), None, (0.0, 0.0, 0.0)),
    ("disc 2^20 shells", "disc", 1 << 20, 64, (0.02, 1.2, True), None, "com"),
]

ap = argparse.ArgumentParser()
ap.add_argument("--sims", nargs="*", default=["naive", "tree"])
ap.add_argument("--cases", type=int, nargs="*", default=list(range(len(CASES))), help="indices into the case list")
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--baseline", type=int, default=0, help="timed read_particles + numpy runs per case (0: none)")
ap.add_argument("--table", default="", help="also write the table to this file")
args = ap.parse_args()

if nb.device_count() < 1:
    sys.exit("bench_radial needs a HIP device (no CPU fallback)")


def make(kind, init, n):
    sp = nb.SimParams(particle_num=n)
    state = {"uniform": nb.inits.uniform_init, "disc": nb.inits.disc_init,
             "spherical": nb.inits.spherical_init}[init](sp, seed=1)
    if kind == "naive":
        return nb.NaiveSim.from_particles(sp, None, state)
    sim = nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(0.75), state)
    sim.encode()  # tree order (and, past 524,288 bodies, the other buffer set)
    sim.wait()
    return sim


def time_calls(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return np.array(ts) * 1e3, out


rows = []
for ci in args.cases:
    name, init, n, nbins, (rmin, rmax, log), axis, centre = CASES[ci]
    edges = nb.radial_edges(rmin, rmax, nbins, log)
    for kind in args.sims:
        sim = make(kind, init, n)
        call = lambda: sim.radial_profile(edges, cylindrical=axis is not None, axis=axis or (0.0, 1.0, 0.0),  # noqa: E731
                                          center=centre)
        # the two calls alternate, so that both see the same machine
        tp, tm = [], []
        for _ in range(args.warmup):
            call()
            sim.diagnostics()
        for _ in range(args.reps):
            a, p = time_calls(call, 1, 0)
            b, _ = time_calls(sim.diagnostics, 1, 0)
            tp.append(a[0])
            tm.append(b[0])
        tp, tm = np.array(tp), np.array(tm)
        row = {"case": name, "sim": kind, "n": n, "nbins": nbins, "cylindrical": axis is not None,
               "center": "com" if centre == "com" else "explicit", "reps": args.reps,
               "median_ms": float(np.median(tp)), "min_ms": float(tp.min()), "max_ms": float(tp.max()),
               "moments_median_ms": float(np.median(tm)), "ratio": float(np.median(tp) / np.median(tm)),
               "bytes_read": 32 * n, "largest_bin": int(p.count.max()), "binned": int(p.count.sum())}
        if args.baseline > 0:
            from tests import radial_ref  # the rule in numpy

            def host():
                s = nb.as_floats(sim.read_particles())
                d = sim.diagnostics() if centre == "com" else None
                c = d.com if d else centre
                vc = d.momentum / d.mass if d else (0.0, 0.0, 0.0)
                return radial_ref.profile64(s, edges, center=c, velocity=vc, axis=axis)

            tb, ref = time_calls(host, args.baseline, 1)
            row["baseline_median_ms"] = float(np.median(tb))
            row["baseline_counts_equal"] = bool(np.array_equal(ref["count"], p.count))
        sim.destroy()
        rows.append(row)
        print(json.dumps(row), flush=True)

lines = ["# tools/bench_radial.py: nb_sim_radial_profile, wall ms per call (host clock, %d calls alternating with a "
         "moments-only diagnostics())" % args.reps,
         "# " + nb.version(),
         "# ratio: profile / moments; largest: bodies in the fullest bin; baseline: read_particles + numpy, ms",
         "%-18s %-6s %9s %5s %4s %4s %9s %9s %9s %9s %6s %9s %10s" % (
             "case", "sim", "n", "bins", "cyl", "ctr", "median", "min", "max", "moments", "ratio", "largest", "baseline")]
for r in rows:
    lines.append("%-18s %-6s %9d %5d %4s %4s %9.4f %9.4f %9.4f %9.4f %6.2f %9d %10s" % (
        r["case"], r["sim"], r["n"], r["nbins"], "yes" if r["cylindrical"] else "no", r["center"][:3],
        r["median_ms"], r["min_ms"], r["max_ms"], r["moments_median_ms"], r["ratio"], r["largest_bin"],
        "%.1f" % r["baseline_median_ms"] if "baseline_median_ms" in r else "-"))
print("\n".join(lines))
if args.table:
    with open(args.table, "w") as f:
        f.write("\n".join(lines) + "\n")
print(json.dumps({"bench": "radial_profile", "rows": len(rows), "device": nb.version()}))
