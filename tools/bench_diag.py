"""Diagnostics benchmark (nb_sim_diagnostics, csrc/nb_diag.hip): wall time per call, host clock around
the whole call (launches, the one small copy, the synchronisation), on an idle simulator stream.
Moments at --moments-n bodies, the pair potential at each of --potential-n, on both simulators.
Prints one JSON line per case and a summary line.  Secondary to bench.py; used for DESIGN.md."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wgpu_n_body_amd as nb  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--moments-n", type=int, default=1 << 20)
ap.add_argument("--potential-n", type=int, nargs="*", default=[65536, 1 << 20])
ap.add_argument("--sims", nargs="*", default=["naive", "tree"])
ap.add_argument("--reps", type=int, default=20, help="timed calls (moments); potential: max(2, reps // 10)")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--init", default="uniform")
args = ap.parse_args()

if nb.device_count() < 1:
    sys.exit("bench_diag needs a HIP device (no CPU fallback)")


def make(kind, n):
    sp = nb.SimParams(particle_num=n)
    state = {"uniform": nb.inits.uniform_init, "disc": nb.inits.disc_init,
             "spherical": nb.inits.spherical_init}[args.init](sp, seed=1)
    if kind == "naive":
        return nb.NaiveSim.from_particles(sp, None, state)
    return nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(0.75), state)


def time_calls(sim, potential, reps, warmup):
    for _ in range(warmup):
        sim.diagnostics(potential)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        d = sim.diagnostics(potential)
        ts.append(time.perf_counter() - t0)
    return np.array(ts), d


rows = []
for kind in args.sims:
    cases = [(args.moments_n, False)] + [(n, True) for n in args.potential_n]
    for n, potential in cases:
        sim = make(kind, n)
        sim.encode()  # a stepped state (a TreeSim past 524,288 bodies has changed buffer set)
        sim.wait()
        reps = args.reps if not potential else max(2, args.reps // 10)
        warm = args.warmup if not potential else 1
        ts, d = time_calls(sim, potential, reps, warm)
        sim.destroy()
        pairs = n * (n - 1) // 2 if potential else 0
        row = {"sim": kind, "n": n, "what": "potential" if potential else "moments", "reps": reps,
               "median_ms": float(np.median(ts) * 1e3), "min_ms": float(ts.min() * 1e3),
               "max_ms": float(ts.max() * 1e3)}
        if potential:
            row["pairs_per_s"] = pairs / float(np.median(ts))
            row["pair_sum"] = d.pair_sum
        else:
            row["bytes_read"] = 32 * n
        rows.append(row)
        print(json.dumps(row), flush=True)
print(json.dumps({"bench": "diagnostics", "rows": len(rows), "device": nb.version()}))
