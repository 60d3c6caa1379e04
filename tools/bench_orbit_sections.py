"""Orbit-section benchmark (nb_orbit_sections_sim, the orbit unit of csrc/nb_field.hip): the whole orbit_sections()
call against the whole orbits() call with the same arguments, both with every = steps, in one session and interleaved
call by call, on the cases of DESIGN.md 6t: 64 tracers x 1,000 steps on the 100,000-body disc, 4,096 x 100 on 2^20
bodies, 65,536 x 10 on 4,000,000 bodies.  Wall time on the host clock around the call; per call kind the median and
the spread (max - min) / median of the repeats.  The section adds no launch and no pair, so the ratio of the medians
is expected inside orbits()'s own spread where the pairs fill the device.
Beside them what the package offered for a section before: orbits(every=1) for 64 tracers at the largest step count
the 2^22 samples allow (65,535), and numpy's interpolation of the plane crossings from the tracks.
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
ap.add_argument("--seconds", type=float, default=6.0, help="cap on the timed calls of one case, both kinds together")
ap.add_argument("--dt", type=float, default=0.01)
ap.add_argument("--omega", type=float, default=0.5)
ap.add_argument("--max-crossings", type=int, default=64)
ap.add_argument("--parent", type=int, default=1, help="1: also time orbits(every=1) + numpy for 64 tracers x 65,535 steps")
ap.add_argument("--parent-steps", type=int, default=65535)
ap.add_argument("--table", default="", help="also write the table to this file")
args = ap.parse_args()

if nb.device_count() < 1:
    sys.exit("bench_orbit_sections needs a HIP device (no CPU fallback)")

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


def numpy_section(o, normal, offset):
    """The up-crossings of normal . xi = offset from the tracks of orbits(every=1): linear interpolation, as the
    device's rule has it (the pattern-frame positions alone; the velocities would double the work)."""
    xi = o.in_pattern_frame() - o.center
    n, e1, e2 = nb.map_frame(o.axis)
    s = (xi @ e1) * normal[0] + (xi @ e2) * normal[1] + (xi @ n) * normal[2] - offset
    up = (s[:-1] < 0) & (s[1:] >= 0)
    k, i = np.nonzero(up)
    f = s[k, i] / (s[k, i] - s[k + 1, i])
    return xi[k, i] + f[:, None] * (xi[k + 1, i] - xi[k, i]), (o.step[k] + f) * o.dt, i


rows = []
for ci in args.cases:
    name, init, n, m, steps = CASES[ci]
    sim, state = make(init, n)
    pos, vel = tracers(state, m)
    kw = dict(dt=args.dt, steps=steps, every=steps, omega=args.omega)
    ts, to, s, o = interleaved(lambda: sim.orbit_sections(pos, vel, max_crossings=args.max_crossings, **kw),
                               lambda: sim.orbits(pos, vel, **kw), args.reps, args.warmup, args.seconds)
    same = bool(np.array_equal(s.orbits.pos, o.pos) and np.array_equal(s.orbits.vel, o.vel))
    row = {"state": name, "n": n, "m": m, "steps": steps, "calls": len(ts),
           "pair_launches": s.stats.orbit.pair_launches, "orbits_pair_launches": o.stats.pair_launches,
           "sections_ms": float(np.median(ts)), "sections_spread": spread(ts), "orbits_ms": float(np.median(to)),
           "orbits_spread": spread(to), "ratio": float(np.median(ts) / np.median(to)), "tracks_same_bits": same,
           "crossings": s.stats.crossings, "stored": s.stats.stored}
    rows.append(row)
    print(json.dumps(row), flush=True)
    if ci == 0 and args.parent:
        m0, steps0 = 64, args.parent_steps
        p0, v0 = pos[:m0], vel[:m0]
        kw0 = dict(dt=args.dt, omega=args.omega)
        t0 = time.perf_counter()
        tr = sim.orbits(p0, v0, steps=steps0, every=1, **kw0)
        t1 = time.perf_counter()
        pts, tt, who = numpy_section(tr, (0.0, 1.0, 0.0), 0.0)
        t2 = time.perf_counter()
        sec = sim.orbit_sections(p0, v0, steps=steps0, max_crossings=4096, **kw0)
        t3 = time.perf_counter()
        parent = {"parent": "orbits(every=1) + numpy", "n": n, "m": m0, "steps": steps0, "orbits_every1_ms": (t1 - t0) * 1e3,
                  "numpy_ms": (t2 - t1) * 1e3, "track_bytes": int(tr.pos.nbytes * 8 // 3),
                  "orbit_sections_ms": (t3 - t2) * 1e3, "crossings_numpy": int(len(tt)),
                  "crossings_device": int(sec.stats.crossings)}
        rows.append(parent)
        print(json.dumps(parent), flush=True)
    sim.destroy()

lines = ["# tools/bench_orbit_sections.py: orbit_sections() against orbits(), every = steps, wall ms per call (host clock,",
         "# interleaved; median of up to %d calls of each after %d warm-up); spread: (max - min) / median of the repeats" % (
             args.reps, args.warmup),
         "# " + nb.version(),
         "# ratio: sections / orbits; launches: pair launches, the same for both; same: the two calls' tracks agree bit for bit",
         "%-12s %9s %7s %6s %5s %8s %11s %7s %11s %7s %7s %9s %5s" % (
             "state", "n", "m", "steps", "calls", "launches", "sections", "spread", "orbits", "spread", "ratio",
             "crossings", "same")]
for r in rows:
    if "parent" in r:
        lines.append("# before: orbits(every=1) for %d tracers x %d steps on the same state %.1f ms (%.0f MB of tracks) + numpy "
                     "interpolation %.1f ms, %d crossings; orbit_sections() of the same run %.1f ms, %d crossings" % (
                         r["m"], r["steps"], r["orbits_every1_ms"], r["track_bytes"] / 1e6, r["numpy_ms"],
                         r["crossings_numpy"], r["orbit_sections_ms"], r["crossings_device"]))
        continue
    lines.append("%-12s %9d %7d %6d %5d %8d %11.3f %7.3f %11.3f %7.3f %7.3f %9d %5s" % (
        r["state"], r["n"], r["m"], r["steps"], r["calls"], r["pair_launches"], r["sections_ms"], r["sections_spread"],
        r["orbits_ms"], r["orbits_spread"], r["ratio"], r["crossings"], "yes" if r["tracks_same_bits"] else "NO"))
print("\n".join(lines))
if args.table:
    with open(args.table, "w") as f:
        f.write("\n".join(lines) + "\n")
print(json.dumps({"bench": "orbit_sections", "rows": len(rows), "device": nb.version()}))
