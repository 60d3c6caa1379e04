"""Group-shapes benchmark (nb_sim_group_shapes, csrc/nb_shape.hip) on a NaiveSim.  Per case, HIP events on the
simulator's stream around calls that ask for the stats only: the whole call (the front end and all rounds), and the
cost of one round -- the call with max_iter 2 less the call with max_iter 1, which is one launch of the
select-and-sum kernel over every row plus one update.  Then the median wall time of whole calls with the rows (host
clock), the launches of a call (a restatement in Python of the plan in sim_group_shapes, not a count the library
reports), the rounds taken, and what the call replaces: read_particles plus the numpy rule of tests/shape_ref.py per
group, timed over a sample of the groups and scaled to all of them.  The radius of a row is --k-rms times the rms
radius of its members, the centres are the members' own (round 0).
  --trace-only     a few calls of nb_sim_fof (with the catalogue's sums) and of nb_sim_group_shapes (max_iter 2) per
                   case and nothing else: the program to run under a kernel trace;
  --summarize DIR  reads the kernel trace(s) under DIR (csv, one row per launch): the mean time of a launch of the
                   select-and-sum kernel of round 1 and 2 beside the catalogue-sum kernel of nb_sim_fof
                   (fof_sum_kernel: nine sums through the same run slots) on the same state.
Prints one JSON line per case, a table and a summary line.  Secondary to bench.py."""
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
ap.add_argument("--cases", type=int, nargs="*", default=None, help="indices into the case list")
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--max-iter", type=int, default=32)
ap.add_argument("--k-rms", type=float, default=1.5)
ap.add_argument("--chunk-len", type=int, default=1024)
ap.add_argument("--baseline-groups", type=int, default=64, help="groups the numpy baseline takes (0: none)")
ap.add_argument("--trace-only", action="store_true")
ap.add_argument("--summarize", default="", help="directory with the kernel trace csv files of --trace-only runs")
ap.add_argument("--table", default="", help="also write (default) or append (--summarize) the table to this file")
args = ap.parse_args()

HBM_PEAK = 8.0e12    # bytes / s, MI355X
MEMBER_BYTES = 32    # a round reads a member's position + mass and velocity: two float4


def summarize(root):
    lines = ["# tools/bench_shapes.py --summarize: mean ms per launch (rocprofv3 --kernel-trace, a run of its own per "
             "case): the select-and-sum kernel of rounds 1 and 2 (the launches in which every row is live) beside "
             "nb_sim_fof's catalogue-sum kernel on the same state"]
    for path in sorted(glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)):
        with open(path, newline="") as f:
            rows = list(csv.DictReader(f))
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        ms = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
        fof = [ms(r) for r in rows if "fof_sum_kernel" in r["Kernel_Name"]]
        # a shapes call: init, then per round sum and update; round 0 first (the centres are the members' own)
        calls, cur = [], None
        for r in rows:
            name = r["Kernel_Name"]
            if "shape_init_kernel" in name:
                cur = []
                calls.append(cur)
            elif "shape_sum_kernel" in name and cur is not None:
                cur.append(ms(r))
        live = [t for c in calls[1:] for t in c[1:3]]  # (the first call warms up; c[0] is round 0)
        zero = [c[0] for c in calls[1:] if c]
        if not fof or not live:
            continue
        a, b = float(np.mean(live)), float(np.mean(fof[1:] or fof))
        lines.append("%-28s shape_sum %9.4f (round 0: %9.4f)   fof_sum %9.4f   ratio %5.2f (%s 3)" % (
            os.path.relpath(path, root).split(os.sep)[0], a, float(np.mean(zero)), b, a / b, "within" if a <= 3 * b else "ABOVE"))
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
    sys.exit("bench_shapes needs a HIP device (no CPU fallback)")
stream = torch.cuda.Stream()
L = _lib.lib()
NONE = _lib.NB_FOF_NONE


def balls(groups, members):
    """bench_bound.py's state: `groups` balls of `members` bodies and radius 0.2, four apart; row g = ball g."""
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
    sim = nb.NaiveSim.from_particles(nb.SimParams(particle_num=n), None, state,
                                     placement=nb.Placement(stream=stream.cuda_stream))
    return sim, np.repeat(np.arange(groups, dtype=np.uint32), members), groups, link


def clumps():
    """bench_halo.py's clumped state (the same 4,096 balls), the rows from the friends-of-friends catalogue."""
    sim, _, _, link = balls(4096, 256)
    fof = sim.fof_groups(link, min_members=20, labels=False)
    return sim, fof.group_of, len(fof.rows), link


def disc():
    """The 100,000-body disc, its friends-of-friends groups at half a mean spacing (bench_fof.py's spacing)."""
    sp = nb.SimParams(particle_num=100000)
    state = nb.as_floats(nb.inits.disc_init(sp, seed=1)).copy()
    lo, hi = np.percentile(state[:, 0:3], [10, 90], axis=0)
    inside = np.all((state[:, 0:3] >= lo) & (state[:, 0:3] <= hi), axis=1).sum()
    link = 0.5 * float((np.prod(np.maximum(hi - lo, 1e-6)) / max(inside, 1)) ** (1.0 / 3.0))
    sim = nb.NaiveSim.from_particles(sp, None, state, placement=nb.Placement(stream=stream.cuda_stream))
    fof = sim.fof_groups(link, min_members=20, labels=False)
    return sim, fof.group_of, len(fof.rows), link


CASES = [
    ("1 x 65536", lambda: balls(1, 65536)),
    ("4096 x 256", lambda: balls(4096, 256)),
    ("32768 x 32", lambda: balls(32768, 32)),
    ("clumps 2^20 fof", clumps),
    ("disc 100k fof", disc),
]


def rms_radius(state, gof, m):
    """k_rms times the mass-weighted rms distance of every row's members from their centre of mass."""
    has = gof != NONE
    g = gof[has].astype(np.int64)
    x, w = state[has, 0:3].astype(np.float64), state[has, 9].astype(np.float64)
    mass = np.bincount(g, w, m)
    c = np.stack([np.bincount(g, w * x[:, a], m) for a in range(3)], axis=1) / mass[:, None]
    r2 = np.bincount(g, w * ((x - c[g]) ** 2).sum(axis=1), m) / mass
    return args.k_rms * np.sqrt(r2)


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


def launches(m, max_iter):
    """The kernel launches of a stats-only call with device centres: the plan of sim_group_shapes restated."""
    passes = 1
    while passes < 4 and (m >> (8 * passes)):
        passes += 1
    return 1 + 3 * passes + 2 + 1 + 2 * (max_iter + 1)


rows = []
for ci in (args.cases if args.cases is not None else range(len(CASES))):
    name, make = CASES[ci]
    sim, gof, m, link = make()
    sim.set_tuning("shape_chunk_len", args.chunk_len)
    n = int(sim.sim_params().particle_num)
    gof = np.ascontiguousarray(gof, np.uint32)
    state = nb.as_floats(sim.read_particles())
    radius = np.ascontiguousarray(rms_radius(state, gof, m))
    st = _lib.nb_shape_stats()
    out_rows = np.zeros(m, _lib.SHAPE_GROUP_DTYPE)

    def call(max_iter, want_rows=False):
        p = _lib.nb_shape_params()
        p.flags, p.min_members, p.max_iter, p.tol, p.step_num = 0, 10, max_iter, 1e-3, _lib.NB_SHAPE_ANY_STEP
        _lib.check(L.nb_sim_group_shapes(sim._h, C.byref(p), gof.ctypes.data, m, None, None, radius.ctypes.data,
                                         out_rows.ctypes.data if want_rows else None, None, C.byref(st)))

    if args.trace_only:
        for _ in range(3):
            sim.fof_groups(link, min_members=20, labels=False)
            call(2)
        sim.destroy()
        continue
    print("# %s: %d rows, timing %d + %d calls a figure" % (name, m, args.warmup, args.reps), file=sys.stderr, flush=True)
    t_all = events(lambda: call(args.max_iter), args.reps, args.warmup)
    full = {k: int(getattr(st, k)) for k in ("members", "converged", "unconverged", "degenerate", "empty", "rounds_max")}
    t_1 = events(lambda: call(1), args.reps, args.warmup)
    t_2 = events(lambda: call(2), args.reps, args.warmup)
    clean = int(st.rounds_max) == 2 and int(st.degenerate) == 0  # every row ran its second round
    tw = []
    for r in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        call(args.max_iter, True)
        if r >= args.warmup:
            tw.append((time.perf_counter() - t0) * 1e3)
    round_ms = t_2 - t_1
    row = {"case": name, "n": n, "rows": m, "reps": args.reps, "k_rms": args.k_rms, "kernels_all_rounds_ms": t_all,
           "max_iter_1_ms": t_1, "max_iter_2_ms": t_2, "round_ms": round_ms, "round_is_clean": clean,
           "call_median_ms": float(np.median(tw)), "call_min_ms": float(np.min(tw)),
           "launches": launches(m, args.max_iter), "mean_rounds": float(out_rows["iterations"].mean()) if m else 0.0,
           "ns_per_member_round": round_ms * 1e6 / max(full["members"], 1),
           "round_bytes_per_s": MEMBER_BYTES * full["members"] / (round_ms * 1e-3),
           **full}
    row["hbm_share"] = row["round_bytes_per_s"] / HBM_PEAK
    if args.baseline_groups > 0 and m > 0:
        from tests import shape_ref
        t0 = time.perf_counter()
        state = nb.as_floats(sim.read_particles())
        t_read = (time.perf_counter() - t0) * 1e3
        take = np.unique(np.linspace(0, m - 1, min(m, args.baseline_groups)).astype(np.int64))
        t0 = time.perf_counter()
        same = True
        for r in take:  # the loop a user writes: one group at a time
            mem = np.flatnonzero(gof == r)
            ref = shape_ref.shape_ref(state[mem], np.zeros(len(mem), np.uint32), 1, radius=[radius[r]],
                                      max_iter=args.max_iter)
            same &= ref["rows"]["iterations"][0] == out_rows["iterations"][r] and \
                ref["rows"]["selected"][0] == out_rows["selected"][r]
        t_base = (time.perf_counter() - t0) * 1e3
        row.update(read_ms=t_read, baseline_groups=len(take), baseline_sample_ms=t_base,
                   baseline_all_ms=t_read + t_base * m / len(take), baseline_integers_equal=bool(same))
        row["speedup"] = row["baseline_all_ms"] / row["call_median_ms"]
    sim.destroy()
    rows.append(row)
    print(json.dumps(row), flush=True)

if args.trace_only:
    sys.exit(0)
lines = ["# tools/bench_shapes.py: nb_sim_group_shapes on a NaiveSim, ms, median of the reps (kernels: HIP events around a "
         "stats-only call, front end included; round: max_iter 2 less max_iter 1; call: host clock, with the rows; "
         "radius %g rms, max_iter %d, shape_chunk_len %d)" % (args.k_rms, args.max_iter, args.chunk_len),
         "# " + nb.version(),
         "# ns/mem: the round per member; HBM: 32 bytes a member and round against %.1f TB/s; baseline: read_particles, then "
         "the numpy rule on `of` groups one at a time, scaled to all rows; x: baseline / call" % (HBM_PEAK * 1e-12),
         "%-16s %8s %6s %9s %9s %9s %7s %7s %6s %6s %6s %5s %5s %11s %5s %9s" % (
             "case", "n", "rows", "kernels", "round", "call", "ns/mem", "HBM", "launch", "rounds", "mean", "unc", "deg",
             "baseline", "of", "x")]
for r in rows:
    lines.append("%-16s %8d %6d %9.3f %9.4f %9.3f %7.3f %6.2f%% %6d %6d %6.1f %5d %5d %11s %5s %9s" % (
        r["case"], r["n"], r["rows"], r["kernels_all_rounds_ms"], r["round_ms"], r["call_median_ms"],
        r["ns_per_member_round"], 100 * r["hbm_share"], r["launches"], r["rounds_max"], r["mean_rounds"], r["unconverged"],
        r["degenerate"], "%.1f" % r["baseline_all_ms"] if "baseline_all_ms" in r else "-", r.get("baseline_groups", "-"),
        "%.0f" % r["speedup"] if "speedup" in r else "-"))
print("\n".join(lines))
if args.table:
    with open(args.table, "w") as f:
        f.write("\n".join(lines) + "\n")
print(json.dumps({"bench": "group_shapes", "rows": len(rows), "device": nb.version()}))
