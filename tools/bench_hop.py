"""Density-peak group benchmark (nb_sim_hop, csrc/nb_hop.hip).  Three modes:

  (default)        per case: the kernels of a call -- HIP events on the simulator's stream around a call that asks for
                   the stats only -- and the wall time of whole calls (host clock around Simulator.hop_groups: launches,
                   the copies of labels, group_of, the catalogue and the boundary table, the synchronisation), each as
                   minimum and median over --reps calls after --warmup; in the same run the kernels of nb_sim_knn at
                   k = k_density and at k = max(k_hop, k_merge), the same way.  --baseline adds what the call replaces:
                   read_particles, scipy.spatial.cKDTree and numpy for the same labels, and reports the share of them
                   that equal the call's (the k-d tree's order and sums are not the rule's);
  --trace-only     a few whole calls per case and nothing else: the program to run under a kernel trace;
  --summarize DIR  reads the kernel trace(s) under DIR (csv, one row per launch) and splits the time of a call by
                   phase: a call's launches come in a fixed order, so the phase of a launch follows from the kernels
                   that open each phase, although the sort kernels of the three phases share their names.

The cases of DESIGN.md 6m: the 100,000-body disc, 2^20 bodies spherical (clumped) and 4,000,000 uniform.  Prints one
JSON line per row and a table.  Secondary to bench.py."""
import argparse
import csv
import glob
import json
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [
    ("disc 100k", "disc", 100_000),
    ("sphere 2^20", "spherical", 1 << 20),
    ("uniform 4M", "uniform", 4_000_000),
]

# the kernel that opens each phase of a call, in the order of a call (csrc/nb_hop.hip)
PHASES = [("density", "bounds_kernel"), ("hop search", "hop_search_kernel"), ("chains", "hop_chain_kernel"),
          ("catalogue", "fof_label_kernel"), ("boundaries", "hop_emit_kernel")]

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, nargs="*", default=list(range(len(CASES))), help="indices into the case list")
ap.add_argument("--k", type=int, nargs=3, default=[64, 16, 4], metavar=("DENS", "HOP", "MERGE"))
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--baseline", type=int, default=0, help="timed read_particles + cKDTree + numpy runs per case (0: none)")
ap.add_argument("--trace-only", action="store_true")
ap.add_argument("--summarize", default="", help="directory with the kernel trace csv files of --trace-only runs")
ap.add_argument("--table", default="", help="also write (default) or append (--summarize) the table to this file")
args = ap.parse_args()


def summarize(root):
    """Per trace file: the launches in start order, cut into calls at every `density` opener, the first --warmup calls
    dropped; per phase and per kernel the mean time per call."""
    lines = ["# tools/bench_hop.py --summarize: kernel time of one whole nb_sim_hop call (every output) by phase, ms, mean "
             "over the traced calls after %d warm-up calls (rocprofv3 --kernel-trace, a run of its own per case)" % args.warmup]
    for path in sorted(glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)):
        with open(path, newline="") as f:
            rows = list(csv.DictReader(f))
        if not rows:
            continue
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        calls, phase = [], None
        for r in rows:
            name = r["Kernel_Name"]
            for ph, opener in PHASES:
                if opener in name:
                    if ph == "density":
                        calls.append({})
                    phase = ph
            if phase is None or not calls:
                continue
            found = re.search(r"(\w+_kernel)", name)
            short = found.group(1) if found else name[:28]
            ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
            calls[-1].setdefault(phase, {}).setdefault(short, [0, 0.0])
            calls[-1][phase][short][0] += 1
            calls[-1][phase][short][1] += ms
        calls = [c for c in calls[args.warmup:] if "boundaries" in c]  # (whole nb_sim_hop calls only)
        if not calls:
            continue
        lines.append("## %s: %d calls" % (os.path.relpath(path, root).split(os.sep)[0], len(calls)))
        total = {ph: np.mean([sum(v[1] for v in c.get(ph, {}).values()) for c in calls]) for ph, _ in PHASES}
        for ph, _ in PHASES:
            lines.append("%-11s %9.4f" % (ph, total[ph]))
            kernels = {}
            for c in calls:
                for k, (cnt, ms) in c.get(ph, {}).items():
                    kernels.setdefault(k, [0, 0.0])
                    kernels[k][0] += cnt
                    kernels[k][1] += ms
            for k, (cnt, ms) in sorted(kernels.items(), key=lambda kv: -kv[1][1]):
                lines.append("    %-28s %5.1f launches %9.4f" % (k, cnt / len(calls), ms / len(calls)))
        rest = total["chains"] + total["catalogue"] + total["boundaries"]
        search = total["density"] + total["hop search"]
        lines.append("chains + catalogue + boundaries %.4f against the two searches %.4f: %s" % (
            rest, search, "below" if rest < search else "ABOVE"))
    print("\n".join(lines))
    if args.table:
        with open(args.table, "a") as f:
            f.write("\n".join(lines) + "\n")


if args.summarize:
    summarize(args.summarize)
    sys.exit(0)

import ctypes as C  # noqa: E402

import torch  # noqa: E402

import wgpu_n_body_amd as nb  # noqa: E402
from wgpu_n_body_amd import _lib  # noqa: E402

if nb.device_count() < 1:
    sys.exit("bench_hop needs a HIP device (no CPU fallback)")

KD, KH, KM = args.k


def make(init, n, stream):
    sp = nb.SimParams(particle_num=n)
    state = nb.as_floats({"uniform": nb.inits.uniform_init, "disc": nb.inits.disc_init,
                          "spherical": nb.inits.spherical_init}[init](sp, seed=1)).copy()
    return nb.NaiveSim.from_particles(sp, None, state, placement=nb.Placement(stream=stream.cuda_stream))


def cpu_labels(state):
    """What the call replaces: the labels from a k-d tree and numpy on the host (the density as nb_sim_knn words it)."""
    from scipy.spatial import cKDTree
    pos = state[:, 0:3].astype(np.float64)
    mass = state[:, 9].astype(np.float64)
    k = max(KD, KH)
    d, j = cKDTree(pos).query(pos, k + 1, workers=16)
    r2 = d[:, KD] ** 2
    acc = np.zeros(len(pos))
    for t in range(1, KD):
        acc = acc + mass[j[:, t]]
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = np.where(r2 == 0.0, np.inf, acc / (_lib.NB_KNN_SPHERE * (r2 * np.sqrt(r2))))
    cand = j[:, :KH + 1]  # the body itself first
    order = np.lexsort((cand, -rho[cand]), axis=1)[:, 0]
    nxt = cand[np.arange(len(pos)), order]
    while True:
        jump = nxt[nxt]
        if np.array_equal(jump, nxt):
            return nxt.astype(np.uint32)
        nxt = jump


def events_ms(stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


rows = []
stream = torch.cuda.Stream()
for ci in args.cases:
    name, init, n = CASES[ci]
    sim = make(init, n, stream)
    hp = _lib.nb_hop_params()
    hp.k_density, hp.k_hop, hp.k_merge, hp.min_members, hp.density_min = KD, KH, KM, 1, -np.inf
    hst = _lib.nb_hop_stats()
    kst = _lib.nb_knn_stats()

    def hop_stats():
        _lib.check(_lib.lib().nb_sim_hop(sim._h, C.byref(hp), None, None, None, None, None, 0, None, 0, C.byref(hst)))

    def knn_stats(k):
        kp = _lib.nb_knn_params()
        kp.k = k
        _lib.check(_lib.lib().nb_sim_knn(sim._h, C.byref(kp), None, None, None, None, C.byref(kst)))

    if args.trace_only:
        for r in range(args.warmup + args.reps):  # whole calls: the catalogue's sums and the boundary table with them
            sim.hop_groups(k_density=KD, k_hop=KH, k_merge=KM)
        sim.destroy()
        continue
    th, tw, t1, t2 = [], [], [], []
    for r in range(args.warmup + args.reps):
        a = events_ms(stream, hop_stats)
        b = events_ms(stream, lambda: knn_stats(KD))
        c = events_ms(stream, lambda: knn_stats(max(KH, KM)))
        t0 = time.perf_counter()
        g = sim.hop_groups(k_density=KD, k_hop=KH, k_merge=KM)
        w = (time.perf_counter() - t0) * 1e3
        if r >= args.warmup:
            th.append(a)
            t1.append(b)
            t2.append(c)
            tw.append(w)
    th, tw, t1, t2 = (np.array(t) for t in (th, tw, t1, t2))
    s = g.stats
    row = {"case": name, "n": n, "k": [KD, KH, KM], "reps": args.reps, "kernels_min_ms": float(th.min()),
           "kernels_median_ms": float(np.median(th)), "call_min_ms": float(tw.min()),
           "call_median_ms": float(np.median(tw)), "knn_density_median_ms": float(np.median(t1)),
           "knn_hop_median_ms": float(np.median(t2)), "peaks": s.peaks, "boundaries": s.boundaries,
           "boundary_pairs": s.boundary_pairs, "largest_count": s.largest_count}
    if args.baseline > 0:
        tb = []
        for _ in range(args.baseline):
            t0 = time.perf_counter()
            lab = cpu_labels(nb.as_floats(sim.read_particles()))
            tb.append((time.perf_counter() - t0) * 1e3)
        row["baseline_min_ms"], row["baseline_median_ms"] = float(np.min(tb)), float(np.median(tb))
        # the tree's neighbour order and density are not the rule's (another summation order, no index rule for ties),
        # so a few bodies may hop elsewhere: the share of equal labels is reported, not asserted
        row["labels_equal_share"] = float((lab == g.labels).mean())
    rows.append(row)
    print(json.dumps(row), flush=True)
    sim.destroy()

if args.trace_only:
    sys.exit(0)

lines = ["# tools/bench_hop.py: nb_sim_hop(k_density %d, k_hop %d, k_merge %d) on a NaiveSim, ms per call, minimum and "
         "median of %d after %d warm-up calls (kernels: HIP events around a stats-only call; call: host clock around "
         "Simulator.hop_groups with labels, group_of, catalogue and boundaries)" % (KD, KH, KM, args.reps, args.warmup),
         "# " + nb.version(),
         "# knn: the kernels of nb_sim_knn (stats only) at k = k_density and at k = max(k_hop, k_merge), median, in the "
         "same run; baseline: read_particles + scipy.spatial.cKDTree + numpy for the labels, ms, median of %d; equal: "
         "the share of its labels equal to the call's" % args.baseline,
         "%-12s %8s %9s %9s %9s %9s %8s %8s %7s %9s %9s %7s" % (
             "case", "n", "kern min", "kern med", "call min", "call med", "knn dens", "knn hop", "peaks", "boundary",
             "baseline", "equal")]
for r in rows:
    lines.append("%-12s %8d %9.4f %9.4f %9.4f %9.4f %8.4f %8.4f %7d %9d %9s %7s" % (
        r["case"], r["n"], r["kernels_min_ms"], r["kernels_median_ms"], r["call_min_ms"], r["call_median_ms"],
        r["knn_density_median_ms"], r["knn_hop_median_ms"], r["peaks"], r["boundaries"],
        "%.1f" % r["baseline_median_ms"] if "baseline_median_ms" in r else "-",
        "%.4f" % r["labels_equal_share"] if "labels_equal_share" in r else "-"))
print("\n".join(lines))
if args.table:
    with open(args.table, "w") as f:
        f.write("\n".join(lines) + "\n")
print(json.dumps({"bench": "hop_groups", "rows": len(rows), "device": nb.version()}))
