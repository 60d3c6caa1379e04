"""Orbit benchmark (nb_orbits_sim, the orbit unit of csrc/nb_field.hip): wall time of a whole call, host clock around
it (the upload of the tracers, the moments pass, every launch of every step, the copy of the tracks, the one
synchronisation), on an idle simulator stream; the median of repeated calls after warm-up.  The cases of DESIGN.md
6t: 64 tracers x 1,000 steps on the 100,000-body disc, 4,096 x 100 on 2^20 bodies, 65,536 x 10 on 4,000,000 bodies (a
NaiveSim holds the state: both simulators hand the kernel the same arrays).  Beside each, in the same run:
  loop     -- what the package offered before: steps + 1 field(accel) calls from a Python loop around the numpy
              integrator of the same rule (tests/orbit_ref.py), every step an upload, a synchronisation and a download;
  field-k  -- the pair kernel's time in a plain field() call at the same (M, N), taken by difference (the call minus
              the same call on a one-body simulator, which pays for everything but the pairs), times steps + 1;
  orbit-k  -- the same difference for the orbits call: its pair launches and nothing else.  The kernel is the same
              instantiation, so the two are expected to agree.
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
ap.add_argument("--reps", type=int, default=10, help="timed calls per case (fewer where a call is long)")
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--seconds", type=float, default=3.0, help="cap on the timed calls of one case")
ap.add_argument("--loop", type=int, default=1, help="timed runs of the Python loop per case (0: none)")
ap.add_argument("--dt", type=float, default=0.01)
ap.add_argument("--omega", type=float, default=0.5)
ap.add_argument("--table", default="", help="also write the table to this file")
args = ap.parse_args()

if nb.device_count() < 1:
    sys.exit("bench_orbits needs a HIP device (no CPU fallback)")

INITS = {"uniform": nb.inits.uniform_init, "disc": nb.inits.disc_init, "spherical": nb.inits.spherical_init}


def make(init, n):
    sp = nb.SimParams(particle_num=n)
    state = nb.as_floats(INITS[init](sp, seed=1))
    return nb.NaiveSim.from_particles(sp, None, state), state


def tracers(state, m):
    rng = np.random.default_rng(m)
    lo, hi = state[:, 0:3].min(0), state[:, 0:3].max(0)
    return rng.uniform(lo, hi, size=(m, 3)), rng.normal(size=(m, 3)) * 0.1


def lib_phase(omega, dt, k):
    import ctypes as C

    from wgpu_n_body_amd import _lib
    c, s = C.c_double(), C.c_double()
    nb.check(_lib.lib().nb_orbit_phase(omega, dt, k, C.byref(c), C.byref(s)))
    return c.value, s.value


def time_calls(fn, reps, warmup, seconds=None):
    for _ in range(warmup):
        fn()
    ts, out = [], None
    while len(ts) < reps and (seconds is None or len(ts) < 3 or sum(ts) < seconds):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return np.array(ts) * 1e3, out


one, _ = make("uniform", 1)  # the calls' fixed costs: everything but the pairs
rows = []
for ci in args.cases:
    name, init, n, m, steps = CASES[ci]
    sim, state = make(init, n)
    pos, vel = tracers(state, m)
    kw = dict(dt=args.dt, steps=steps, every=max(1, steps // 10), omega=args.omega)
    to, o = time_calls(lambda: sim.orbits(pos, vel, **kw), args.reps, args.warmup, args.seconds)
    to1, _ = time_calls(lambda: one.orbits(pos, vel, **kw), args.reps, args.warmup, args.seconds)
    pts = pos.astype(np.float32)
    tf, _ = time_calls(lambda: sim.field(pts, potential=False), 30, 3, 1.5)
    tf1, _ = time_calls(lambda: one.field(pts, potential=False), 30, 3, 1.5)
    mo, mf = float(np.median(to)), float(np.median(tf))
    ko, kf = mo - float(np.median(to1)), (mf - float(np.median(tf1))) * (steps + 1)
    row = {"state": name, "n": n, "m": m, "steps": steps, "calls": len(to), "pair_launches": o.stats.pair_launches,
           "orbits_ms": mo, "orbits_min_ms": float(to.min()), "orbits_max_ms": float(to.max()),
           "orbits_kernel_ms": ko, "field_call_ms": mf, "field_kernel_ms": kf,
           "kernel_ratio": ko / kf if kf > 0 else float("nan"),
           "gpairs_per_s": float(m * n * (steps + 1) / mo / 1e6)}
    if args.loop > 0:
        from tests import orbit_ref  # the rule in numpy around field()

        tl, ref = time_calls(lambda: orbit_ref.orbits(orbit_ref.device_field(sim), pos, vel, phase=lib_phase,
                                                       frame=nb.map_frame((0, 1, 0)), **kw), args.loop, 0)
        row["loop_ms"] = float(np.median(tl))
        row["loop_same_bits"] = bool(np.array_equal(ref["pos"], o.pos) and np.array_equal(ref["vel"], o.vel))
    rows.append(row)
    print(json.dumps(row), flush=True)
    sim.destroy()
one.destroy()

lines = ["# tools/bench_orbits.py: nb_orbits_sim, wall ms per call (host clock, median of up to %d calls after %d "
         "warm-up)" % (args.reps, args.warmup),
         "# " + nb.version(),
         "# orbit-k / field-k: the call minus the same call on a one-body simulator; field-k is one field(accel) call's,",
         "# times steps + 1; ratio: orbit-k / field-k; Gpair/s: m * n * (steps + 1) / orbits",
         "# loop: steps + 1 field(accel) calls from Python around the numpy integrator (tests/orbit_ref.py), ms; same: its",
         "# positions and velocities are the call's, bit for bit",
         "%-12s %9s %7s %6s %5s %8s %11s %11s %11s %7s %9s %12s" % (
             "state", "n", "m", "steps", "calls", "launches", "orbits", "orbit-k", "field-k", "ratio", "Gpair/s", "loop")]
for r in rows:
    lines.append("%-12s %9d %7d %6d %5d %8d %11.3f %11.3f %11.3f %7.2f %9.1f %12s" % (
        r["state"], r["n"], r["m"], r["steps"], r["calls"], r["pair_launches"], r["orbits_ms"], r["orbits_kernel_ms"],
        r["field_kernel_ms"], r["kernel_ratio"], r["gpairs_per_s"],
        "%.1f %s" % (r["loop_ms"], "same" if r["loop_same_bits"] else "DIFFERENT") if "loop_ms" in r else "-"))
print("\n".join(lines))
if args.table:
    with open(args.table, "w") as f:
        f.write("\n".join(lines) + "\n")
print(json.dumps({"bench": "orbits", "rows": len(rows), "device": nb.version()}))
