"""Group-radii benchmark (nb_group_radii_sim, csrc/nb_radii.hip) on a NaiveSim.  Per state the median of --reps:
the kernels (HIP events on the simulator's stream around a call that asks for the stats only: the upload of
group_of, the front end, both sorts and the new kernels), the whole call with the rows and with the per-body outputs
too (host clock), and what the call replaces, measured in the same run: read_particles, then numpy -- the centres
of mass by bincount, one lexsort on (group, r2), one cumsum with the groups' offsets taken off, the crossings by
searchsorted per group.
  --trace-only     three stats-only calls per state and nothing else: the program to run under a kernel trace;
  --summarize DIR  reads the kernel trace(s) under DIR (csv, one row per launch; a directory per state): the share
                   of the kernel time that is the shared radix sort (sort_*), the front end (assign_*) and the new
                   kernels (radii_*).
Prints one JSON line per state, a table and a summary line.  Secondary to bench.py."""
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

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, nargs="*", default=None, help="indices into the state list")
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--baseline-reps", type=int, default=3)
ap.add_argument("--trace-only", action="store_true")
ap.add_argument("--summarize", default="", help="directory with the kernel trace csv files of --trace-only runs")
ap.add_argument("--table", default="", help="also write (default) or append (--summarize) the table to this file")
args = ap.parse_args()

FRACTIONS = (0.1, 0.5, 0.9)


def summarize(root):
    lines = ["# tools/bench_radii.py --summarize: kernel time of the traced calls by family, ms per call and share "
             "(rocprofv3 --kernel-trace, a run of its own per state, three calls each)"]
    newest = {}  # a directory per state; the newest trace of each, should an earlier run have left one
    for path in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        state = os.path.relpath(path, root).split(os.sep)[0]
        if state not in newest or os.path.getmtime(path) > os.path.getmtime(newest[state]):
            newest[state] = path
    for path in (newest[k] for k in sorted(newest)):
        with open(path, newline="") as f:
            rows = list(csv.DictReader(f))
        ms = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
        fam = {"sort": 0.0, "assign": 0.0, "radii": 0.0}
        calls = 0
        for r in rows:
            name = r["Kernel_Name"]
            calls += "radii_rows_kernel" in name
            for k in fam:
                if k + "_" in name:
                    fam[k] += ms(r)
                    break
        total = sum(fam.values())
        if not calls or total <= 0.0:
            continue
        rest = fam["assign"] + fam["radii"]
        lines.append("%-18s sort %8.3f (%4.1f%%)   front end %7.3f   new kernels %7.3f   outside the sort %8.3f: %s the sort"
                     % (os.path.relpath(path, root).split(os.sep)[0], fam["sort"] / calls, 100 * fam["sort"] / total,
                        fam["assign"] / calls, fam["radii"] / calls, rest / calls,
                        "less than" if rest < fam["sort"] else "MORE THAN"))
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
    sys.exit("bench_radii needs a HIP device (no CPU fallback)")
stream = torch.cuda.Stream()
L = _lib.lib()


def balls(groups, members):
    """bench_shapes.py's state: `groups` balls of `members` bodies and radius 0.2, four apart; row g = ball g."""
    rng = np.random.default_rng(3)
    n, link = groups * members, 0.4
    side = int(np.ceil(groups ** (1.0 / 3.0)))
    k = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)[:groups]
    d = rng.normal(size=(n, 3))
    d *= ((link / 2) * rng.uniform(0.0, 1.0, n) ** (1.0 / 3.0) / np.linalg.norm(d, axis=1))[:, None]
    state = np.zeros((n, 10), np.float32)
    state[:, 0:3] = d * np.array([1.0, 0.7, 0.45]) + np.repeat((k - (side - 1) / 2.0) * (10 * link), members, axis=0)
    state[:, 3:6] = rng.normal(0.0, 1e-3, (n, 3))
    state[:, 9] = rng.uniform(0.5, 2.0, n)
    return state, np.repeat(np.arange(groups, dtype=np.uint32), members), groups


def one_row(n):
    """A Plummer-like cloud of n bodies, the whole state one row."""
    rng = np.random.default_rng(5)
    state = np.zeros((n, 10), np.float32)
    d = rng.normal(size=(n, 3))
    r = 1.0 / np.sqrt(rng.uniform(1e-4, 1.0, n) ** (-2.0 / 3.0) - 1.0 + 1e-12)
    state[:, 0:3] = d * (r / np.linalg.norm(d, axis=1))[:, None]
    state[:, 9] = rng.uniform(0.5, 2.0, n)
    return state, np.zeros(n, np.uint32), 1


CASES = [
    ("1 x 65536", lambda: balls(1, 65536)),
    ("4096 x 256", lambda: balls(4096, 256)),
    ("32768 x 32", lambda: balls(32768, 32)),
    ("2^20 one row", lambda: one_row(1 << 20)),
    ("4000000 one row", lambda: one_row(4000000)),
]


def numpy_radii(state, gof, m):
    """The alternative on the host: centres of mass, the (group, r2) order, the enclosed mass, the crossings, v_max."""
    g = gof.astype(np.int64)
    x, w = state[:, 0:3].astype(np.float64), state[:, 9].astype(np.float64)
    mass = np.bincount(g, w, m)
    c = np.stack([np.bincount(g, w * x[:, a], m) for a in range(3)], axis=1) / mass[:, None]
    d = x - c[g]
    r2 = (d * d).sum(axis=1)
    order = np.lexsort((r2, g))
    gs, ws, rs = g[order], w[order], np.sqrt(r2[order])
    start = np.searchsorted(gs, np.arange(m + 1))
    cum = np.cumsum(ws)
    before = np.concatenate([[0.0], cum])[start[:-1]]
    enclosed = cum - before[gs]
    radius = np.empty((m, len(FRACTIONS)))
    for r in range(m):  # argsort + cumsum per group: the crossings of a group's own curve
        curve = enclosed[start[r]:start[r + 1]]
        at = np.minimum(np.searchsorted(curve, np.asarray(FRACTIONS) * curve[-1]), len(curve) - 1)
        radius[r] = rs[start[r] + at]
    with np.errstate(divide="ignore", invalid="ignore"):
        vc2 = np.where(rs > 0, enclosed / rs, 0.0)
    rank = np.arange(len(gs)) - start[gs]
    vmax = np.maximum.reduceat(np.where(rank >= 10, vc2, 0.0), start[:-1])
    return radius, vmax


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


def wall(fn, reps, warmup):
    out = []
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        if r >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


rows = []
for ci in (args.cases if args.cases is not None else range(len(CASES))):
    name, make = CASES[ci]
    state, gof, m = make()
    n = len(state)
    sim = nb.NaiveSim.from_particles(nb.SimParams(particle_num=n), None, state,
                                     placement=nb.Placement(stream=stream.cuda_stream))
    gof = np.ascontiguousarray(gof, np.uint32)
    st = _lib.nb_radii_stats()
    out_rows = np.zeros(m, _lib.RADII_GROUP_DTYPE)
    rank, enc = np.empty(n, np.uint32), np.empty(n, np.float64)
    p = _lib.nb_radii_params()
    p.nf, p.vmax_skip, p.step_num = len(FRACTIONS), 10, _lib.NB_RADII_ANY_STEP
    for k, f in enumerate(FRACTIONS):
        p.fractions[k] = f

    def call(want_rows=False, per_body=False):
        _lib.check(L.nb_group_radii_sim(sim._h, C.byref(p), gof.ctypes.data, m, None,
                                        out_rows.ctypes.data if want_rows else None,
                                        rank.ctypes.data if per_body else None, enc.ctypes.data if per_body else None,
                                        C.byref(st)))

    if args.trace_only:
        for _ in range(3):
            call()
        sim.destroy()
        continue
    print("# %s: %d rows, timing %d + %d calls a figure" % (name, m, args.warmup, args.reps), file=sys.stderr, flush=True)
    row = {"case": name, "n": n, "rows": m, "reps": args.reps,
           "kernels_ms": events(call, args.reps, args.warmup),
           "call_ms": wall(lambda: call(True), args.reps, args.warmup),
           "call_per_body_ms": wall(lambda: call(True, True), args.reps, args.warmup),
           "members": int(st.members)}
    if args.baseline_reps > 0:
        t_read, t_np = [], []
        for _ in range(args.baseline_reps):
            t0 = time.perf_counter()
            host = nb.as_floats(sim.read_particles())
            t1 = time.perf_counter()
            radius, vmax = numpy_radii(host, gof, m)
            t_np.append((time.perf_counter() - t1) * 1e3)
            t_read.append((t1 - t0) * 1e3)
        dev = out_rows["radius"][:, :len(FRACTIONS)]
        row.update(read_ms=float(np.median(t_read)), numpy_ms=float(np.median(t_np)),
                   baseline_ms=float(np.median(t_read)) + float(np.median(t_np)),
                   radius_rel_diff=float(np.nanmax(np.abs(radius - dev) / dev)))
        row["speedup"] = row["baseline_ms"] / row["call_ms"]
    sim.destroy()
    rows.append(row)
    print(json.dumps(row), flush=True)

if args.trace_only:
    sys.exit(0)
lines = ["# tools/bench_radii.py: nb_group_radii_sim on a NaiveSim, ms, median of %d (kernels: HIP events around a "
         "stats-only call, the upload of group_of included; call: host clock, with the rows; +body: with rank_of and "
         "enclosed_of too; centres formed on the device, fractions 0.1 0.5 0.9, vmax_skip 10)" % args.reps,
         "# " + nb.version(),
         "# baseline, median of %d in the same run: read = read_particles; numpy = centres of mass, lexsort on (group, "
         "r2), cumsum, crossings per group; x = (read + numpy) / call; diff = the largest relative difference of its "
         "radii from the call's" % args.baseline_reps,
         "%-16s %8s %6s %9s %9s %9s %9s %9s %7s %8s" % ("state", "n", "rows", "kernels", "call", "+body", "read", "numpy",
                                                        "x", "diff")]
for r in rows:
    lines.append("%-16s %8d %6d %9.3f %9.3f %9.3f %9s %9s %7s %8s" % (
        r["case"], r["n"], r["rows"], r["kernels_ms"], r["call_ms"], r["call_per_body_ms"],
        "%.3f" % r["read_ms"] if "read_ms" in r else "-", "%.3f" % r["numpy_ms"] if "numpy_ms" in r else "-",
        "%.1f" % r["speedup"] if "speedup" in r else "-",
        "%.1e" % r["radius_rel_diff"] if "radius_rel_diff" in r else "-"))
print("\n".join(lines))
if args.table:
    with open(args.table, "w") as f:
        f.write("\n".join(lines) + "\n")
print(json.dumps({"bench": "group_radii", "rows": len(rows), "device": nb.version()}))
