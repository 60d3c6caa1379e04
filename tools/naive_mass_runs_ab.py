"""A/B inside one build: the all-pairs step with `naive_mass_runs` 0 (every pair multiplied by m_j)
against 1 (runs of equal masses summed unweighted), same process, same device, alternating.

    python tools/naive_mass_runs_ab.py [--bodies 65536] [--steps 200] [--warmup 120] [--rounds 5]

Two simulators over the same uniform_init state (every mass 1); after the warm-up each round times
`--steps` back-to-back steps of either (nb_sim_encode_n_timed: wall of the batch and the mean
HIP-event duration of the force kernel).  Prints every round, the medians and their ratio, and
checks that both end in the same bits (unit masses: the two modes are the same arithmetic)."""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wgpu_n_body_amd as nb  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--bodies", type=int, default=65536)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=120)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--variant", type=int, default=None)
args = ap.parse_args()

n = args.bodies
sp = nb.SimParams(particle_num=n)
init = nb.inits.uniform_init(sp, seed=2)
sims = {}
for mode in (0, 1):
    sims[mode] = nb.NaiveSim.from_particles(sp, None, init)
    sims[mode].set_tuning("naive_mass_runs", mode)
    if args.variant is not None:
        sims[mode].set_tuning("naive_variant", args.variant)
print(f"{nb.version()}  n={n} steps={args.steps} warmup={args.warmup} rounds={args.rounds}")
for mode in (0, 1):
    for _ in range(args.warmup):
        sims[mode].encode()
    sims[mode].wait()
rate = {0: [], 1: []}
kern = {0: [], 1: []}
for r in range(args.rounds):
    for mode in (0, 1):
        ms_total, ms_kernel = sims[mode].encode_n_timed(args.steps)
        rate[mode].append(n * (n - 1) * args.steps / (ms_total * 1e-3))
        kern[mode].append(ms_kernel)
        print(f"round {r} naive_mass_runs={mode}: {ms_total / args.steps:.4f} ms/step, kernel {ms_kernel:.4f} ms, "
              f"{rate[mode][-1] / 1e12:.4f}e12 pairs/s", flush=True)
med = {m: statistics.median(rate[m]) for m in (0, 1)}
for m in (0, 1):
    print(f"naive_mass_runs={m}: median {med[m] / 1e12:.4f}e12 pairs/s, spread (max - min) "
          f"{(max(rate[m]) - min(rate[m])) / 1e12:.4f}e12, median kernel {statistics.median(kern[m]):.4f} ms")
print(f"ratio of the medians, 1 over 0: {med[1] / med[0]:.4f}")
out = [nb.as_floats(sims[m].dest_particle_slice()).copy() for m in (0, 1)]
same = np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))
print(f"states after {args.warmup + args.rounds * args.steps} steps bitwise equal: {same}")
for m in (0, 1):
    sims[m].destroy()
sys.exit(0 if same else 1)
