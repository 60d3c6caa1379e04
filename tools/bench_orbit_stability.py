"""Orbit-stability benchmark (nb_orbit_stability_sim, csrc/nb_stability.hip) on the cases of DESIGN.md 6t: 64 tracers
x 1,000 steps on the 100,000-body disc, 4,096 x 100 on 2^20 bodies, 65,536 x 10 on 4,000,000 bodies.  Two comparisons,
each A/B in alternation within one process, wall time on the host clock around calls that end in a synchronisation;
per call kind the median and the spread (max - min) / median of the repeats:
  whole    the whole orbit_stability() call against the whole orbits() call with the same arguments (every = steps);
  pairs    what the fused pair kernel replaces: one field(accel) call plus one tidal_tensor() call at the tracers'
           m starting points (each one pair launch, its finish, two copies and a synchronisation) against the whole
           orbit_stability() call divided by its steps + 1 evaluations (each the fused pair launch and the step launch).
--kernels runs only a few calls of each kind and prints nothing else: the work of a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/bench_orbit_stability.py --kernels), whose probe_kernel<...> rows
are the pair kernels' own times.
No pass/fail threshold.  Prints one JSON line per case and a table.  Secondary to bench.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wgpu_n_body_amd as nb  # noqa: E402

CASES = [("disc 100k", "disc", 100_000, 64, 1000), ("sphere 2^20", "spherical", 1 << 20, 4096, 100),
         ("uniform 4M", "uniform", 4_000_000, 65536, 10)]

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, nargs="*", default=list(range(len(CASES))), help="indices into the case list")
ap.add_argument("--reps", type=int, default=9, help="timed calls of each kind per case (fewer where a call is long)")
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--seconds", type=float, default=6.0, help="cap on the timed calls of one comparison")
ap.add_argument("--dt", type=float, default=0.01)
ap.add_argument("--omega", type=float, default=0.5)
ap.add_argument("--deviations", type=int, default=2)
ap.add_argument("--kernels", action="store_true", help="a few calls of each kind, for a kernel trace")
ap.add_argument("--table", default="", help="also write the table to this file")
args = ap.parse_args()

if nb.device_count() < 1:
    sys.exit("bench_orbit_stability needs a HIP device (no CPU fallback)")

INITS = {"uniform": nb.inits.uniform_init, "disc": nb.inits.disc_init, "spherical": nb.inits.spherical_init}


def make(init, n):
    sp = nb.SimParams(particle_num=n)
    state = nb.as_floats(INITS[init](sp, seed=1))
    return nb.NaiveSim.from_particles(sp, None, state), state


def tracers(state, m):
    rng = np.random.default_rng(m)
    lo, hi = state[:, 0:3].min(0), state[:, 0:3].max(0)
    return rng.uniform(lo, hi, size=(m, 3)), rng.normal(size=(m, 3)) * 0.1


def interleaved(fa, fb, reps, warmup, seconds):
    """ms of fa and fb, called in turn, so that a drift of the machine meets both alike."""
    for _ in range(warmup):
        fa()
        fb()
    ta, tb, oa, ob = [], [], None, None
    while len(ta) < reps and (len(ta) < 3 or sum(ta) + sum(tb) < seconds):
        t0 = time.perf_counter()
        oa = fa()
        t1 = time.perf_counter()
        ob = fb()
        t2 = time.perf_counter()
        ta.append(t1 - t0)
        tb.append(t2 - t1)
    return np.array(ta) * 1e3, np.array(tb) * 1e3, oa, ob


def spread(t):
    return float((t.max() - t.min()) / np.median(t))


rows = []
for ci in args.cases:
    name, init, n, m, steps = CASES[ci]
    sim, state = make(init, n)
    pos, vel = tracers(state, m)
    pts = pos.astype(np.float32)
    kw = dict(dt=args.dt, steps=steps, every=steps, omega=args.omega)

    def separate():
        return sim.field(pts, accel=True, potential=False), sim.tidal_tensor(pts)

    if args.kernels:
        for _ in range(3):
            separate()
        sim.orbit_stability(pos, vel, deviations=args.deviations, **dict(kw, steps=min(steps, 10), every=min(steps, 10)))
        sim.orbits(pos, vel, **dict(kw, steps=min(steps, 10), every=min(steps, 10)))
        sim.destroy()
        continue
    ts, to, s, o = interleaved(lambda: sim.orbit_stability(pos, vel, deviations=args.deviations, **kw),
                               lambda: sim.orbits(pos, vel, **kw), args.reps, args.warmup, args.seconds)
    tf, tp, _, _ = interleaved(lambda: sim.orbit_stability(pos, vel, deviations=args.deviations, **kw), separate,
                               args.reps, args.warmup, args.seconds)
    same = bool(np.array_equal(s.orbits.pos, o.pos) and np.array_equal(s.orbits.vel, o.vel))
    evals = steps + 1
    row = {"state": name, "n": n, "m": m, "steps": steps, "deviations": args.deviations, "calls": len(ts),
           "pair_launches": s.stats.orbit.pair_launches, "orbits_pair_launches": o.stats.pair_launches,
           "stability_ms": float(np.median(ts)), "stability_spread": spread(ts), "orbits_ms": float(np.median(to)),
           "orbits_spread": spread(to), "whole_ratio": float(np.median(ts) / np.median(to)),
           "fused_eval_ms": float(np.median(tf) / evals), "separate_ms": float(np.median(tp)),
           "separate_spread": spread(tp), "pairs_ratio": float(np.median(tf) / evals / np.median(tp)),
           "tracks_same_bits": same, "renorms": s.stats.renorms}
    rows.append(row)
    print(json.dumps(row), flush=True)
    sim.destroy()

if args.kernels:
    sys.exit(0)

lines = ["# tools/bench_orbit_stability.py: wall ms per call (host clock, interleaved; median of up to %d calls of each after" % args.reps,
         "# %d warm-up); spread: (max - min) / median of the repeats; %d deviation vectors per tracer" % (
             args.warmup, args.deviations),
         "# " + nb.version(),
         "# whole: orbit_stability() / orbits(), every = steps; launches: pair launches, the same for both;",
         "# fused/eval: orbit_stability() / (steps + 1); separate: one field(accel) call + one tidal_tensor() call at the m",
         "# starting points; pairs: fused/eval over separate; same: the two calls' tracks agree bit for bit",
         "%-12s %9s %7s %6s %5s %8s %11s %7s %11s %7s %7s %11s %11s %7s %7s %5s" % (
             "state", "n", "m", "steps", "calls", "launches", "stability", "spread", "orbits", "spread", "whole",
             "fused/eval", "separate", "spread", "pairs", "same")]
for r in rows:
    lines.append("%-12s %9d %7d %6d %5d %8d %11.3f %7.3f %11.3f %7.3f %7.3f %11.4f %11.4f %7.3f %7.3f %5s" % (
        r["state"], r["n"], r["m"], r["steps"], r["calls"], r["pair_launches"], r["stability_ms"],
        r["stability_spread"], r["orbits_ms"], r["orbits_spread"], r["whole_ratio"], r["fused_eval_ms"],
        r["separate_ms"], r["separate_spread"], r["pairs_ratio"], "yes" if r["tracks_same_bits"] else "NO"))
print("\n".join(lines))
if args.table:
    with open(args.table, "w") as f:
        f.write("\n".join(lines) + "\n")
print(json.dumps({"bench": "orbit_stability", "rows": len(rows), "device": nb.version()}))
