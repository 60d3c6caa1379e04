"""Local-kinematics benchmark (nb_local_kinematics_sim, csrc/nb_kinematics.hip) on a NaiveSim, on the first three
states of tools/bench_knn.py: the 100,000-body disc, 2^20 bodies spherical, 4,000,000 uniform; k = 6 and 32; the
moments alone and with the gradient sums.  The comparison is nb_sim_knn at the same k on the same state in the same
run: the search is the same code, the epilogue adds k gathers of 32 bytes and 10 or 25 ordered sums per body.
Per state and k, the median of --reps after --warmup: the whole calls on the host clock -- nb_sim_knn with its four
arrays, the pass with the moments, r2, mass_in and density, and the same with the gradient sums (the copies to the
host are part of a call: 28, 104 and 224 bytes a body).
  --trace-only     per state and k three calls each of nb_sim_knn (stats only), the moments and the gradient sums
                   and nothing else: the program to run under a kernel trace, a run of its own per state;
  --summarize DIR  reads the kernel traces under DIR (csv, one row per launch; a directory per state): the search
                   kernels' time per launch -- knn_search_kernel, kin_search_kernel<10> and <25> -- and their ratios.
Prints one JSON line per row, a table and a summary line.  Secondary to bench.py."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [("disc 100k", "disc", 100_000), ("sphere 2^20", "spherical", 1 << 20), ("uniform 4M", "uniform", 4_000_000)]
TRACE_CALLS = 3

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, nargs="*", default=list(range(len(CASES))), help="indices into the state list")
ap.add_argument("--ks", type=int, nargs="*", default=[6, 32])
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--trace-only", action="store_true")
ap.add_argument("--summarize", default="", help="directory with the kernel trace csv files of --trace-only runs")
ap.add_argument("--table", default="", help="also write (default) or append (--summarize) the table to this file")
args = ap.parse_args()


def summarize(root):
    lines = ["# tools/bench_kinematics.py --summarize: the search kernels, ms per launch, mean of %d launches (rocprofv3 "
             "--kernel-trace, a run of its own per state; per k: nb_sim_knn's kernel, then the pass with 10 and with "
             "25 sums; x: against nb_sim_knn's)" % TRACE_CALLS,
             "%-14s %3s %10s %10s %6s %10s %6s" % ("state", "k", "knn", "moments", "x", "+gradient", "x")]
    newest = {}
    for path in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        state = os.path.relpath(path, root).split(os.sep)[0]
        if state not in newest or os.path.getmtime(path) > os.path.getmtime(newest[state]):
            newest[state] = path
    for state in sorted(newest):
        with open(newest[state], newline="") as f:
            rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
        seq = [("knn" if "knn_search_kernel" in r["Kernel_Name"] else
                "mom" if "kin_search_kernel<10" in r["Kernel_Name"] else "grad",
                (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
               for r in rows if "knn_search_kernel" in r["Kernel_Name"] or "kin_search_kernel" in r["Kernel_Name"]]
        per_k = 3 * TRACE_CALLS
        for j, k in enumerate(args.ks):  # the order --trace-only launches them in
            part = seq[j * per_k:(j + 1) * per_k]
            if len(part) < per_k or [p[0] for p in part] != ["knn"] * TRACE_CALLS + ["mom"] * TRACE_CALLS + ["grad"] * TRACE_CALLS:
                lines.append("%-14s %3d (the trace does not hold the launches of --trace-only --ks %s)" % (state, k, args.ks))
                continue
            t = [float(np.mean([p[1] for p in part[i * TRACE_CALLS:(i + 1) * TRACE_CALLS]])) for i in range(3)]
            lines.append("%-14s %3d %10.3f %10.3f %6.2f %10.3f %6.2f" % (state, k, t[0], t[1], t[1] / t[0], t[2],
                                                                        t[2] / t[0]))
    print("\n".join(lines))
    if args.table:
        with open(args.table, "a") as f:
            f.write("\n".join(lines) + "\n")


if args.summarize:
    summarize(args.summarize)
    sys.exit(0)

import torch  # noqa: E402

import wgpu_n_body_amd as nb  # noqa: E402
from wgpu_n_body_amd import _lib  # noqa: E402

if nb.device_count() < 1:
    sys.exit("bench_kinematics needs a HIP device (no CPU fallback)")
stream = torch.cuda.Stream()
L = _lib.lib()


def wall(fn):
    out = []
    for r in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        fn()
        if r >= args.warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


rows = []
for ci in args.cases:
    name, init, n = CASES[ci]
    sp = nb.SimParams(particle_num=n)
    state = nb.as_floats({"uniform": nb.inits.uniform_init, "disc": nb.inits.disc_init,
                          "spherical": nb.inits.spherical_init}[init](sp, seed=1)).copy()
    sim = nb.NaiveSim.from_particles(sp, None, state, placement=nb.Placement(stream=stream.cuda_stream))
    mom, gr = np.empty((n, 10)), np.empty((n, 15))
    r2, mass_in, rho, kth = np.empty(n), np.empty(n), np.empty(n), np.empty(n, np.uint32)
    for k in args.ks:
        kp, ks = _lib.nb_knn_params(), _lib.nb_knn_stats()
        kp.k = k
        p, st = _lib.nb_kin_params(), _lib.nb_kin_stats()
        p.k, p.flags = k, _lib.NB_KIN_SELF

        def knn(outputs=True):
            a = (r2.ctypes.data, kth.ctypes.data, mass_in.ctypes.data, rho.ctypes.data) if outputs else (None,) * 4
            _lib.check(L.nb_sim_knn(sim._h, C.byref(kp), *a, C.byref(ks)))

        def kin(grads):
            _lib.check(L.nb_local_kinematics_sim(sim._h, C.byref(p), mom.ctypes.data, gr.ctypes.data if grads else None,
                                                 r2.ctypes.data, None, mass_in.ctypes.data, rho.ctypes.data,
                                                 C.byref(st)))

        if args.trace_only:
            for fn in (lambda: knn(False), lambda: kin(False), lambda: kin(True)):
                for _ in range(TRACE_CALLS):
                    fn()
            continue
        row = {"case": name, "n": n, "k": k, "reps": args.reps, "knn_call_ms": wall(knn),
               "moments_call_ms": wall(lambda: kin(False)), "gradient_call_ms": wall(lambda: kin(True)),
               "counted": int(st.counted), "degenerate": int(st.degenerate)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    sim.destroy()

if args.trace_only:
    sys.exit(0)
lines = ["# tools/bench_kinematics.py: whole calls on a NaiveSim, ms, median of %d after %d warm-up calls (host clock: "
         "launches, the copies to the host, the synchronisation; knn: r2, kth, mass_in, density; moments: the 10 sums, "
         "r2, mass_in, density; +gradient: the 15 sums too)" % (args.reps, args.warmup),
         "# " + nb.version(),
         "%-14s %9s %3s %10s %10s %6s %10s %6s" % ("state", "n", "k", "knn", "moments", "x", "+gradient", "x")]
for r in rows:
    lines.append("%-14s %9d %3d %10.3f %10.3f %6.2f %10.3f %6.2f" % (
        r["case"], r["n"], r["k"], r["knn_call_ms"], r["moments_call_ms"], r["moments_call_ms"] / r["knn_call_ms"],
        r["gradient_call_ms"], r["gradient_call_ms"] / r["knn_call_ms"]))
print("\n".join(lines))
if args.table:
    with open(args.table, "w") as f:
        f.write("\n".join(lines) + "\n")
print(json.dumps({"bench": "local_kinematics", "rows": len(rows), "device": nb.version()}))
