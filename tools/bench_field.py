"""Field-probe benchmark (nb_sim_field, csrc/nb_field.hip): wall time per call, host clock around the whole
call (the upload of the points, the launches, the copy of the samples, the synchronisation), on an idle
simulator stream; the median of repeated calls after warm-up.  The cases of DESIGN.md 6e: 64, 4,096 and
65,536 points against the 100,000-body disc, 2^20 bodies and 4,000,000 bodies, each for the acceleration
alone and for both fields (a NaiveSim holds the state: both simulators hand the kernel the same arrays).
Three yardsticks from the same run: 65,536 points on 65,536 bodies beside one all-pairs step of the same
bodies (the same pair count; the step is timed by device events over 20 steps back to back, the call by the
host clock), the both-fields pair rate beside the diagnostics' pair pass, and -- with --baseline -- what a
call replaces at 64 points, read_particles plus the numpy restatement of the rule
(tests/field_ref.py).  Prints one JSON line per case, a table and a summary line.  Secondary to bench.py."""
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
YARD_N = 65536

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
    sys.exit("bench_field needs a HIP device (no CPU fallback)")

INITS = {"uniform": nb.inits.uniform_init, "disc": nb.inits.disc_init, "spherical": nb.inits.spherical_init}


def make(init, n):
    sp = nb.SimParams(particle_num=n)
    state = nb.as_floats(INITS[init](sp, seed=1))
    return nb.NaiveSim.from_particles(sp, None, state), state


def probe_points(state, m):
    """Half on bodies, half off-body in the bodies' box, as the tests take them."""
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


rows = []
for si in args.states:
    name, init, n = STATES[si]
    sim, state = make(init, n)
    for m in args.points:
        pts = probe_points(state, m)
        for flags, potential in (("acc", False), ("both", True)):
            t, f = time_calls(lambda: sim.field(pts, potential=potential), args.reps, args.warmup, args.seconds)
            row = {"state": name, "n": n, "m": m, "fields": flags, "calls": len(t), "launches": f.launches,
                   "median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()),
                   "gpairs_per_s": float(m * n / np.median(t) / 1e6)}
            if args.baseline > 0 and m == 64 and potential:
                from tests import field_ref  # the rule in numpy

                tb, ref = time_calls(lambda: field_ref.field64(nb.as_floats(sim.read_particles()), pts, sim.sim_params().g,
                                                               sim.sim_params().e), args.baseline, 0)
                row["baseline_median_ms"] = float(np.median(tb))
                row["baseline_within_bounds"] = bool(
                    np.all(np.abs(f.acc - ref["acc"]) <= field_ref.ACC_BOUND * ref["acc_scale"])
                    and np.all(np.abs(f.potential - ref["potential"]) <= field_ref.POT_BOUND * ref["pot_scale"]))
            rows.append(row)
            print(json.dumps(row), flush=True)
    sim.destroy()

# the yardsticks: the same pair count as one all-pairs step, and the diagnostics' pair pass
sim, state = make("uniform", YARD_N)
pts = state[:, 0:3].copy()
ta, _ = time_calls(lambda: sim.field(pts, potential=False), args.reps, args.warmup)
tb, _ = time_calls(lambda: sim.field(pts), args.reps, args.warmup)
tm, _ = time_calls(lambda: sim.diagnostics(), args.reps, args.warmup)
tp, _ = time_calls(lambda: sim.diagnostics(potential=True), args.reps, args.warmup)
sim.encode_n_timed(5)
step_ms = float(np.median([sim.encode_n_timed(20)[0] / 20 for _ in range(5)]))
sim.destroy()
pair_pass_ms = float(np.median(tp) - np.median(tm))
yard = {"n": YARD_N, "m": YARD_N, "field_acc_ms": float(np.median(ta)), "field_both_ms": float(np.median(tb)),
        "step_ms": step_ms, "acc_over_step": float(np.median(ta) / step_ms),
        "field_both_gpairs_per_s": float(YARD_N * YARD_N / np.median(tb) / 1e6),
        "diag_pair_pass_ms": pair_pass_ms,
        "diag_gpairs_per_s": float(YARD_N * (YARD_N - 1) / 2 / pair_pass_ms / 1e6)}
yard["both_rate_over_diag_rate"] = yard["field_both_gpairs_per_s"] / yard["diag_gpairs_per_s"]
print(json.dumps(yard), flush=True)

lines = ["# tools/bench_field.py: nb_sim_field, wall ms per call (host clock, median of up to %d calls after %d warm-up "
         "calls)" % (args.reps, args.warmup),
         "# " + nb.version(),
         "# Gpair/s: m * n / median; baseline: read_particles + numpy (tests/field_ref.py), ms, at 64 points",
         "%-12s %9s %7s %5s %5s %8s %10s %10s %10s %9s %10s" % (
             "state", "n", "m", "field", "calls", "launches", "median", "min", "max", "Gpair/s", "baseline")]
for r in rows:
    lines.append("%-12s %9d %7d %5s %5d %8d %10.4f %10.4f %10.4f %9.1f %10s" % (
        r["state"], r["n"], r["m"], r["fields"], r["calls"], r["launches"], r["median_ms"], r["min_ms"], r["max_ms"],
        r["gpairs_per_s"], "%.1f" % r["baseline_median_ms"] if "baseline_median_ms" in r else "-"))
lines += ["# yardsticks, %d points on %d bodies (uniform), same run:" % (YARD_N, YARD_N),
          "#   acceleration only %.4f ms (host clock, whole call); one all-pairs step %.4f ms (device events over 20 "
          "steps, encode_n_timed); ratio %.2f" % (
              yard["field_acc_ms"], yard["step_ms"], yard["acc_over_step"]),
          "#   both fields %.4f ms = %.1f Gpair/s; the diagnostics' pair pass %.4f ms = %.1f Gpair/s; rate ratio %.2f" % (
              yard["field_both_ms"], yard["field_both_gpairs_per_s"], yard["diag_pair_pass_ms"],
              yard["diag_gpairs_per_s"], yard["both_rate_over_diag_rate"])]
print("\n".join(lines))
if args.table:
    with open(args.table, "w") as f:
        f.write("\n".join(lines) + "\n")
print(json.dumps({"bench": "field", "rows": len(rows), "device": nb.version()}))
