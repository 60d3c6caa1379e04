"""Disc-modes benchmark (nb_disc_modes_sim, csrc/nb_modes.hip): wall time per call, host clock around the whole call
(launches, the small copies, the synchronisation), on an idle simulator stream, median of --reps calls, at mmax = 2,
4 and 8.  Beside each row, in the same process: the cylindrical nb_sim_radial_profile call on the same state, edges,
centre and axis, and (--baseline) what the call replaces, read_particles plus the numpy restatement of the rule
(tests/modes_ref.py), with the two results compared bit for bit.  The cases of DESIGN.md 6p: the 100,000-body disc in
64 annuli about z, 2^20 and 4,000,000 bodies in 64 bins, 2^20 bodies all in one bin.  --trace-only makes a few calls
of the chosen cases and nothing else, for a rocprofv3 --kernel-trace --stats run of its own.  Prints one JSON line per
row, a table and a summary line.  Secondary to bench.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wgpu_n_body_amd as nb  # noqa: E402

# name, init, n, nbins, (rmin, rmax, log), axis
CASES = [
    ("disc 100k annuli", "disc", 100_000, 64, (0.0, 1.2, False), (0.0, 0.0, 1.0)),
    ("sphere 2^20 b64", "spherical", 1 << 20, 64, (0.0, 1.2, False), (0.0, 1.0, 0.0)),
    ("uniform 4M b64", "uniform", 4_000_000, 64, (0.0, 1.8, False), (0.0, 1.0, 0.0)),
    ("one bin 2^20", "spherical", 1 << 20, 1, (0.0, 100.0, False), (0.0, 1.0, 0.0)),
]

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, nargs="*", default=list(range(len(CASES))), help="indices into the case list")
ap.add_argument("--mmax", type=int, nargs="*", default=[2, 4, 8])
ap.add_argument("--reps", type=int, default=40)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--baseline", type=int, default=0, help="timed read_particles + numpy runs per case at the first "
                                                          "mmax (0: none)")
ap.add_argument("--trace-only", action="store_true", help="three calls per row and nothing else (for rocprofv3)")
ap.add_argument("--table", default="", help="also write the table to this file")
args = ap.parse_args()

if nb.device_count() < 1:
    sys.exit("bench_modes needs a HIP device (no CPU fallback)")


def make(init, n):
    sp = nb.SimParams(particle_num=n)
    state = {"uniform": nb.inits.uniform_init, "disc": nb.inits.disc_init,
             "spherical": nb.inits.spherical_init}[init](sp, seed=1)
    return nb.NaiveSim.from_particles(sp, None, state)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


rows = []
for ci in args.cases:
    name, init, n, nbins, (rmin, rmax, log), axis = CASES[ci]
    edges = nb.radial_edges(rmin, rmax, nbins, log)
    sim = make(init, n)
    radial = lambda: sim.radial_profile(edges, cylindrical=True, axis=axis, center="com")  # noqa: E731
    for mi, mmax in enumerate(args.mmax):
        call = lambda: sim.disc_modes(edges, mmax=mmax, axis=axis, center="com")  # noqa: E731
        if args.trace_only:
            for _ in range(3):
                call()
            continue
        for _ in range(args.warmup):
            call()
            radial()
        tm, tr = [], []
        for _ in range(args.reps):  # the two calls alternate, so that both see the same machine
            a, d = timed(call)
            b, r = timed(radial)
            tm.append(a)
            tr.append(b)
        tm, tr = np.array(tm), np.array(tr)
        row = {"case": name, "n": n, "nbins": nbins, "mmax": mmax, "reps": args.reps,
               "median_ms": float(np.median(tm)), "min_ms": float(tm.min()), "max_ms": float(tm.max()),
               "radial_median_ms": float(np.median(tr)), "ratio": float(np.median(tm) / np.median(tr)),
               "largest_bin": int(d.count.max()), "binned": int(d.count.sum()),
               "counts_equal_radial": bool(np.array_equal(d.count, r.count)),
               "a2_max": d.bar_strength()[0] if mmax >= 2 else None}
        if args.baseline > 0 and mi == 0:
            from tests import modes_ref  # the rule in numpy

            def host():
                parts = sim.read_particles()
                diag = sim.diagnostics()
                return modes_ref.modes_ref(parts, edges, mmax, axis, diag.com, diag.momentum / diag.mass)

            tb = []
            for _ in range(args.baseline):
                t, ref = timed(host)
                tb.append(t)
            row["baseline_median_ms"] = float(np.median(tb))
            row["baseline_bits_equal"] = bool(ref["modes"].tobytes() == d.modes.tobytes()
                                              and np.array_equal(ref["count"], d.count))
        rows.append(row)
        print(json.dumps(row), flush=True)
    sim.destroy()

if not args.trace_only:
    lines = ["# tools/bench_modes.py: nb_disc_modes_sim on a NaiveSim, centre of mass, wall ms per whole call (host "
             "clock, median of %d calls alternating with the cylindrical nb_sim_radial_profile call on the same state "
             "and edges)" % args.reps,
             "# " + nb.version(),
             "# ratio: modes / radial; largest: bodies in the fullest bin; baseline: read_particles + numpy "
             "(tests/modes_ref.py), ms, and whether its modes equal the device's bit for bit",
             "%-18s %9s %5s %5s %9s %9s %9s %9s %6s %9s %10s %5s" % (
                 "case", "n", "bins", "mmax", "median", "min", "max", "radial", "ratio", "largest", "baseline", "bits")]
    for r in rows:
        lines.append("%-18s %9d %5d %5d %9.4f %9.4f %9.4f %9.4f %6.2f %9d %10s %5s" % (
            r["case"], r["n"], r["nbins"], r["mmax"], r["median_ms"], r["min_ms"], r["max_ms"], r["radial_median_ms"],
            r["ratio"], r["largest_bin"],
            "%.1f" % r["baseline_median_ms"] if "baseline_median_ms" in r else "-",
            ("yes" if r["baseline_bits_equal"] else "NO") if "baseline_bits_equal" in r else "-"))
    print("\n".join(lines))
    if args.table:
        with open(args.table, "w") as f:
            f.write("\n".join(lines) + "\n")
print(json.dumps({"bench": "disc_modes", "rows": len(rows), "device": nb.version()}))
