"""Shell-modes benchmark (nb_shell_modes_sim, csrc/nb_shell.hip): wall time per call, host clock around the whole call
(launches, the small copies, the synchronisation), on an idle simulator stream, median of --reps calls, at lmax = 2, 4,
4 with rates and 6.  Beside each row, in the same process and alternating with it: disc_modes(mmax=4) and the
spherical nb_sim_radial_profile call on the same state, edges, centre and axis, and (--baseline) what the call
replaces, read_particles plus the numpy restatement of the rule (tests/shell_ref.py), with the two results compared
bit for bit.  The cases of DESIGN.md 6x: the 100,000-body disc, 2^20 and 4,000,000 bodies in 64 shells, 2^20 bodies
all in one shell.  --trace-only makes three calls per row and nothing else, for a rocprofv3 --kernel-trace run of its
own; --summarize DIR turns that run's kernel trace into the per-kernel table.  Prints one JSON line per row, a table
and a summary line.  Secondary to bench.py."""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name, init, n, nbins, (rmin, rmax, log), axis
CASES = [
    ("disc 100k shells", "disc", 100_000, 64, (0.0, 1.2, False), (0.0, 0.0, 1.0)),
    ("sphere 2^20 b64", "spherical", 1 << 20, 64, (0.0, 1.2, False), (0.0, 1.0, 0.0)),
    ("uniform 4M b64", "uniform", 4_000_000, 64, (0.0, 1.8, False), (0.0, 1.0, 0.0)),
    ("one bin 2^20", "spherical", 1 << 20, 1, (0.0, 100.0, False), (0.0, 1.0, 0.0)),
]
CONFIGS = {"2": (2, False), "4": (4, False), "4r": (4, True), "6": (6, False)}  # lmax, rates

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, nargs="*", default=list(range(len(CASES))), help="indices into the case list")
ap.add_argument("--configs", nargs="*", default=list(CONFIGS), choices=list(CONFIGS), help="lmax, r: with rates")
ap.add_argument("--reps", type=int, default=40)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--baseline", type=int, default=0, help="timed read_particles + numpy runs per case at the first "
                                                          "configuration (0: none)")
ap.add_argument("--trace-only", action="store_true", help="three calls per row and nothing else (for rocprofv3)")
ap.add_argument("--summarize", default="", help="the output directory of a rocprofv3 --kernel-trace run of "
                                                "--trace-only: print the per-kernel table and nothing else")
ap.add_argument("--table", default="", help="also write the table to this file")
args = ap.parse_args()

KERNELS = (("moments", ("diag_moments_kernel", "diag_finish_kernel")), ("classifier", ("shell_key_kernel",)),
           ("sort", ("sort_",)), ("row starts", ("assign_rows_kernel",)), ("gather", ("assign_gather_kernel",)),
           ("sums", ("shell_sum_kernel",)), ("rows", ("shell_rows_kernel",)))


def summarize(root):
    """The kernel trace of a --trace-only run: a call ends with its shell_rows_kernel, and the third call of every
    row is reported, microseconds by kernel."""
    path = glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)[0]
    with open(path) as f:
        trace = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    calls, cur = [], {}
    for r in trace:
        name = r["Kernel_Name"]
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        label = next((lab for lab, words in KERNELS if any(w in name for w in words)), "other")
        cur[label] = cur.get(label, 0.0) + us
        if "shell_rows_kernel" in name:
            calls.append(cur)
            cur = {}
    rows = [(CASES[ci][0], cfg) for ci in args.cases for cfg in args.configs]
    assert len(calls) == 3 * len(rows), (len(calls), len(rows))
    labels = [lab for lab, _ in KERNELS]
    lines = ["# kernel time of one call by kernel, microseconds (one rocprofv3 --kernel-trace run of its own: "
             "tools/bench_shell.py --trace-only, the third call of each row); sort: the passes of nb_analysis_sort.hpp",
             "%-18s %5s " % ("case", "lmax") + " ".join("%10s" % lab for lab in labels) + " %10s" % "total"]
    for k, (name, cfg) in enumerate(rows):
        c = calls[3 * k + 2]
        lines.append("%-18s %5s " % (name, cfg) + " ".join("%10.1f" % c.get(lab, 0.0) for lab in labels)
                     + " %10.1f" % sum(c.get(lab, 0.0) for lab in labels))
    print("\n".join(lines))


if args.summarize:
    summarize(args.summarize)
    sys.exit(0)

import wgpu_n_body_amd as nb  # noqa: E402

if nb.device_count() < 1:
    sys.exit("bench_shell needs a HIP device (no CPU fallback)")


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
    radial = lambda: sim.radial_profile(edges, axis=axis, center="com")  # noqa: E731
    disc = lambda: sim.disc_modes(edges, mmax=4, axis=axis, center="com")  # noqa: E731
    for ki, cfg in enumerate(args.configs):
        lmax, rates = CONFIGS[cfg]
        call = lambda: sim.shell_modes(edges, lmax=lmax, rates=rates, axis=axis, center="com")  # noqa: E731
        if args.trace_only:
            for _ in range(3):
                call()
            continue
        for _ in range(args.warmup):
            call()
            disc()
            radial()
        ts, tm, tr = [], [], []
        for _ in range(args.reps):  # the three calls alternate, so that all see the same machine
            a, d = timed(call)
            b, m = timed(disc)
            c, r = timed(radial)
            ts.append(a)
            tm.append(b)
            tr.append(c)
        ts, tm, tr = np.array(ts), np.array(tm), np.array(tr)
        rel2 = d.relative(2) if lmax >= 2 else np.array([np.nan])
        row = {"case": name, "n": n, "nbins": nbins, "lmax": cfg, "reps": args.reps,
               "median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "max_ms": float(ts.max()),
               "disc_median_ms": float(np.median(tm)), "radial_median_ms": float(np.median(tr)),
               "ratio_disc": float(np.median(ts) / np.median(tm)), "ratio_radial": float(np.median(ts) / np.median(tr)),
               "largest_bin": int(d.count.max()), "binned": int(d.count.sum()),
               "counts_equal_radial": bool(np.array_equal(d.count, r.count)),
               "relative2_max": float(np.nanmax(rel2)) if np.isfinite(rel2).any() else None}
        if args.baseline > 0 and ki == 0:
            from tests import shell_ref  # the rule in numpy

            def host():
                parts = sim.read_particles()
                diag = sim.diagnostics()
                return shell_ref.shell_ref(parts, edges, lmax, axis, diag.com, diag.momentum / diag.mass, rates=rates)

            tb = []
            for _ in range(args.baseline):
                t, ref = timed(host)
                tb.append(t)
            row["baseline_median_ms"] = float(np.median(tb))
            row["baseline_bits_equal"] = bool(ref["coef"].tobytes() == d.coef.tobytes()
                                              and np.array_equal(ref["count"], d.count))
        rows.append(row)
        print(json.dumps(row), flush=True)
    sim.destroy()

if not args.trace_only:
    lines = ["# tools/bench_shell.py: nb_shell_modes_sim on a NaiveSim, centre of mass, wall ms per whole call (host "
             "clock, median of %d calls alternating with disc_modes(mmax=4) and the spherical nb_sim_radial_profile "
             "call on the same state and edges)" % args.reps,
             "# " + nb.version(),
             "# lmax: 4r is lmax 4 with NB_SHELL_RATES; /disc, /radial: shell / disc_modes, shell / radial_profile; "
             "largest: bodies in the fullest bin; baseline: read_particles + numpy (tests/shell_ref.py), ms, and "
             "whether its sums equal the device's bit for bit",
             "%-18s %9s %5s %5s %9s %9s %9s %9s %9s %6s %7s %9s %10s %5s" % (
                 "case", "n", "bins", "lmax", "median", "min", "max", "disc", "radial", "/disc", "/radial", "largest",
                 "baseline", "bits")]
    for r in rows:
        lines.append("%-18s %9d %5d %5s %9.4f %9.4f %9.4f %9.4f %9.4f %6.2f %7.2f %9d %10s %5s" % (
            r["case"], r["n"], r["nbins"], r["lmax"], r["median_ms"], r["min_ms"], r["max_ms"], r["disc_median_ms"],
            r["radial_median_ms"], r["ratio_disc"], r["ratio_radial"], r["largest_bin"],
            "%.1f" % r["baseline_median_ms"] if "baseline_median_ms" in r else "-",
            ("yes" if r["baseline_bits_equal"] else "NO") if "baseline_bits_equal" in r else "-"))
    spread = {r["lmax"]: r["median_ms"] for r in rows if r["case"] == "sphere 2^20 b64"}
    one = {r["lmax"]: r["median_ms"] for r in rows if r["case"] == "one bin 2^20"}
    for cfg in one:
        if cfg in spread:
            lines.append("# one bin / spread at 2^20 bodies, lmax %s: %.2f" % (cfg, one[cfg] / spread[cfg]))
    print("\n".join(lines))
    if args.table:
        with open(args.table, "w") as f:
            f.write("\n".join(lines) + "\n")
print(json.dumps({"bench": "shell_modes", "rows": len(rows), "device": nb.version()}))
