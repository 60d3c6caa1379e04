"""Tidal-tensor benchmark (nb_tidal_sim, csrc/nb_tidal.hip): wall time per call, host clock around the whole call
(the upload of the points, the moments pass, the launches, the copy of the samples, the synchronisation), on an idle
simulator stream; the median of repeated calls after warm-up.  The cases of DESIGN.md 6r: 64, 4,096 and 65,536
points against the 100,000-body disc, 2^20 bodies and 4,000,000 bodies (a NaiveSim holds the state: both
simulators hand the kernel the same arrays).  The yardstick is nb_sim_field with the acceleration alone on the same
state and the same points in the same run, the two calls alternating, the field's first in every round: the table
gives both and their ratio.  Kernel time is taken by
difference: the call minus the same call on a one-body simulator, which pays for everything but the pairs.  With
--baseline, what a call replaces at 64 points: read_particles plus the numpy restatement of the rule
(tests/tidal_ref.py).  No pass/fail threshold.  Prints one JSON line per case and a table.  Secondary to bench.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wgpu_n_body_amd as nb  # noqa: E402

STATES = [("disc 100k", "disc", 100_000), ("sphere 2^20", "spherical", 1 << 20), ("uniform 4M", "uniform", 4_000_000)]
POINTS = [64, 4096, 65536]

ap = argparse.ArgumentParser()
ap.add_argument("--states", type=int, nargs="*", default=list(range(len(STATES))), help="indices into the state list")
ap.add_argument("--points", type=int, nargs="*", default=POINTS)
ap.add_argument("--reps", type=int, default=30, help="timed calls per case (fewer where a call is long)")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--seconds", type=float, default=1.5, help="cap on the timed calls of one case")
ap.add_argument("--baseline", type=int, default=0, help="timed read_particles + numpy runs at 64 points (0: none)")
ap.add_argument("--table", default="", help="also write the table to this file")
args = ap.parse_args()

if nb.device_count() < 1:
    sys.exit("bench_tidal needs a HIP device (no CPU fallback)")

INITS = {"uniform": nb.inits.uniform_init, "disc": nb.inits.disc_init, "spherical": nb.inits.spherical_init}


def make(init, n):
    sp = nb.SimParams(particle_num=n)
    state = nb.as_floats(INITS[init](sp, seed=1))
    return nb.NaiveSim.from_particles(sp, None, state), state


def probe_points(state, m):
    """Half on bodies, half off-body in the bodies' box, as tools/bench_field.py takes them."""
    rng = np.random.default_rng(m)
    pts = np.empty((m, 3), np.float32)
    pts[:m // 2] = state[rng.integers(0, state.shape[0], size=m // 2), 0:3]
    lo, hi = state[:, 0:3].min(0), state[:, 0:3].max(0)
    pts[m // 2:] = rng.uniform(lo, hi, size=(m - m // 2, 3)).astype(np.float32)
    return pts


def time_calls(fn, reps, warmup, seconds=None):
    for _ in range(warmup):
        fn()
    ts, out = [], None
    while len(ts) < reps and (seconds is None or len(ts) < 3 or sum(ts) < seconds):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return np.array(ts) * 1e3, out


def time_pair(fa, fb, reps, warmup, seconds):
    """The two calls alternating, fb first in every round, so that neither always follows the other's caches."""
    for _ in range(warmup):
        fb()
        fa()
    ta, tb, out = [], [], None
    while len(ta) < reps and (len(ta) < 3 or sum(ta) + sum(tb) < 2 * seconds):
        t0 = time.perf_counter()
        fb()
        t1 = time.perf_counter()
        out = fa()
        t2 = time.perf_counter()
        tb.append(t1 - t0)
        ta.append(t2 - t1)
    return np.array(ta) * 1e3, np.array(tb) * 1e3, out


one, _ = make("uniform", 1)  # the calls' fixed costs: everything but the pairs
rows = []
for si in args.states:
    name, init, n = STATES[si]
    sim, state = make(init, n)
    for m in args.points:
        pts = probe_points(state, m)
        tt, tf, t = time_pair(lambda: sim.tidal_tensor(pts), lambda: sim.field(pts, potential=False), args.reps,
                              args.warmup, args.seconds)
        t0, f0, _ = time_pair(lambda: one.tidal_tensor(pts), lambda: one.field(pts, potential=False), args.reps,
                              args.warmup, args.seconds)
        mt, mf = float(np.median(tt)), float(np.median(tf))
        kt, kf = mt - float(np.median(t0)), mf - float(np.median(f0))
        row = {"state": name, "n": n, "m": m, "calls": len(tt), "launches": t.launches, "tidal_ms": mt,
               "tidal_min_ms": float(tt.min()), "tidal_max_ms": float(tt.max()), "field_acc_ms": mf,
               "call_ratio": mt / mf, "tidal_kernel_ms": kt, "field_kernel_ms": kf,
               "kernel_ratio": kt / kf if kf > 0 else float("nan"), "gpairs_per_s": float(m * n / mt / 1e6)}
        if args.baseline > 0 and m == 64:
            from tests import tidal_ref  # the rule in numpy

            tb, ref = time_calls(lambda: tidal_ref.tidal64(nb.as_floats(sim.read_particles()), pts, sim.sim_params().g,
                                                           sim.sim_params().e), args.baseline, 0)
            got = t.tensor.reshape(-1, 9)[:, [0, 4, 8, 1, 2, 5]]
            row["baseline_median_ms"] = float(np.median(tb))
            row["baseline_within_bounds"] = bool(np.all(np.abs(got - ref["tensor6"]) <= ref["bound6"]))
        rows.append(row)
        print(json.dumps(row), flush=True)
    sim.destroy()
one.destroy()

lines = ["# tools/bench_tidal.py: nb_tidal_sim beside nb_sim_field (acceleration alone), same state, same points, same "
         "run; wall ms per call",
         "# (host clock, median of up to %d calls after %d warm-up calls)" % (args.reps, args.warmup),
         "# " + nb.version(),
         "# kernel: the call minus the same call on a one-body simulator; ratio: tidal / field; Gpair/s: m * n / tidal",
         "# baseline: read_particles + numpy (tests/tidal_ref.py), ms, at 64 points; ok: the call's samples within the bound of it",
         "%-12s %9s %7s %5s %8s %10s %10s %7s %10s %10s %7s %9s %10s" % (
             "state", "n", "m", "calls", "launches", "tidal", "field", "ratio", "tidal-k", "field-k", "ratio", "Gpair/s",
             "baseline")]
for r in rows:
    lines.append("%-12s %9d %7d %5d %8d %10.4f %10.4f %7.2f %10.4f %10.4f %7.2f %9.1f %10s" % (
        r["state"], r["n"], r["m"], r["calls"], r["launches"], r["tidal_ms"], r["field_acc_ms"], r["call_ratio"],
        r["tidal_kernel_ms"], r["field_kernel_ms"], r["kernel_ratio"], r["gpairs_per_s"],
        "%.1f %s" % (r["baseline_median_ms"], "ok" if r["baseline_within_bounds"] else "OUT OF BOUNDS")
        if "baseline_median_ms" in r else "-"))
print("\n".join(lines))
if args.table:
    with open(args.table, "w") as f:
        f.write("\n".join(lines) + "\n")
print(json.dumps({"bench": "tidal", "rows": len(rows), "device": nb.version()}))
