"""Bound-groups benchmark (nb_sim_bound, csrc/nb_bound.hip).  Per case, HIP events on the simulator's stream around
calls that ask for the stats only: the whole call (all rounds), and the cost of one round -- the call with max_iter 2
less the call with max_iter 1, on states whose groups all need a second round, so the difference is one pass of the
pair kernel over every group plus the decision and the update, O(n) beside it.  The pair rate is the groups' count^2
over that time.  On the same state in the same run the diagnostics' pair pass is timed the same way (the call with
the potential less the call without; n (n - 1) / 2 terms): the ratio of the two rates is the condition DESIGN.md 6k
states for the one-group row.  Then the median wall time of whole calls with every output (host clock), and
what the call replaces: read_particles plus the numpy restatement of tests/bound_ref.py on one group (at most
--baseline-members of it), stated per group.  The launches of a stats-only call after the group finder's are a
restatement in Python of the plan in sim_bound (csrc/nb_bound.hip), not a count the library reports.
Prints one JSON line per case, a table and a summary line.  Secondary to bench.py."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wgpu_n_body_amd as nb  # noqa: E402
from wgpu_n_body_amd import _lib  # noqa: E402

G, DT, E = 6.25e-5, 0.016, 1e-4  # c = g dt = 1e-6
HEAT = 0.6                       # velocity dispersion in sqrt(median c S): sheds a sixth in round 1, settles in ~8

# name, groups, members each
CASES = [
    ("1 x 65536", 1, 65536),
    ("16 x 65536", 16, 65536),
    ("4096 x 256", 4096, 256),
    ("32768 x 32", 32768, 32),
]

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, nargs="*", default=list(range(len(CASES))), help="indices into the case list")
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--min-members", type=int, default=20)
ap.add_argument("--max-iter", type=int, default=32)
ap.add_argument("--baseline-members", type=int, default=2048, help="members of one group the numpy baseline takes (0: none)")
ap.add_argument("--tile", type=int, default=0)
ap.add_argument("--chunk-len", type=int, default=1024)
ap.add_argument("--table", default="", help="also write the table to this file")
args = ap.parse_args()

if nb.device_count() < 1:
    sys.exit("bench_bound needs a HIP device (no CPU fallback)")


def make(groups, members, stream):
    """`groups` balls of `members` bodies and radius 0.2 = link / 2 (the hot ball of tests/bound_ref.py: all members
    friends), ten links apart: every ball one group."""
    rng = np.random.default_rng(3)
    n = groups * members
    link = 0.4
    side = int(np.ceil(groups ** (1.0 / 3.0)))
    k = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)[:groups]
    centres = (k - (side - 1) / 2.0) * (10 * link)
    d = rng.normal(size=(n, 3))
    d *= ((link / 2) * rng.uniform(0.0, 1.0, n) ** (1.0 / 3.0) / np.linalg.norm(d, axis=1))[:, None]
    state = np.zeros((n, 10), np.float32)
    state[:, 0:3] = d + np.repeat(centres, members, axis=0)
    state[:, 9] = rng.uniform(0.5, 2.0, n)
    # sigma from the first ball: S_i of 64 of its members over at most 8,192 of the others, scaled to all
    from tests.diag_ref import psi64
    x, m = state[:members, 0:3].astype(np.float64), state[:members, 9].astype(np.float64)
    js = np.arange(members) if members <= 8192 else rng.choice(members, 8192, replace=False)
    some = np.arange(min(members, 64))
    dd = x[None, js, :] - x[some, None, :]
    psi = psi64(np.sqrt((dd * dd).sum(axis=2)).ravel(), np.float64(np.float32(E))).reshape(len(some), len(js))
    psi[dd.any(axis=2) == 0] = 0.0
    s_med = np.median((m[None, js] * psi).sum(axis=1)) * members / len(js)
    sigma = HEAT * np.sqrt(np.float64(np.float32(G)) * np.float64(np.float32(DT)) * s_med)
    state[:, 3:6] = rng.normal(0.0, sigma, (n, 3))
    sp = nb.SimParams(particle_num=n, g=G, e=E, dt=DT)
    return nb.NaiveSim.from_particles(sp, None, state, placement=nb.Placement(stream=stream.cuda_stream)), link


def launches(n, rows_cap, max_iter, max_group, tile):
    """The kernel launches of one stats-only call after the group finder's: the plan of sim_bound
    (csrc/nb_bound.hip) restated -- the gather, an update per round and one before, the pair launches and the decision
    of every round, and the two pairs of sums; (all launches in a call, per round)."""
    largest = min(n, max_group) if max_group else n
    small = min(256, largest) if tile == 0 else largest if tile == 64 else 0

    def pair_launches(t, top, by_position=False):
        fit = max(1, (1 << 35) // (t * top))
        items = 2 * (n // t + 1) if by_position else n // t + rows_cap + 1
        per = min(items, 2 * max(1, fit - 1) if by_position else fit)
        return -(-items // per)
    per_round = (pair_launches(64, small) if small > 0 else 0) + \
        (pair_launches(256, largest, small == 256) if small < largest else 0)
    return 1 + (max_iter + 1) + max_iter * (per_round + 1) + 2 + 2, per_round


def events(stream, fn, reps, warmup):
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


rows = []
stream = torch.cuda.Stream()
L = _lib.lib()
for ci in args.cases:
    name, groups, members = CASES[ci]
    reps, warmup = args.reps, args.warmup
    n = groups * members
    sim, link = make(groups, members, stream)
    sim.set_tuning("bound_tile", args.tile)
    sim.set_tuning("bound_chunk_len", args.chunk_len)
    max_group = 262144
    cap = n // args.min_members
    st = _lib.nb_bound_stats()

    def call(max_iter):
        p = _lib.nb_bound_params()
        p.link, p.min_members, p.min_bound, p.max_iter, p.max_group = link, args.min_members, args.min_members, max_iter, max_group
        _lib.check(L.nb_sim_bound(sim._h, C.byref(p), None, None, None, None, cap, C.byref(st)))

    print("# %s: state made, timing %d + %d calls a figure" % (name, warmup, reps), file=sys.stderr, flush=True)
    t_all = events(stream, lambda: call(args.max_iter), reps, warmup)
    full = {k: int(getattr(st, k)) for k in ("groups", "bound_groups", "bound_bodies", "dissolved", "unconverged",
                                              "skipped", "rounds_max", "pairs")}
    t_1 = events(stream, lambda: call(1), reps, warmup)
    t_2 = events(stream, lambda: call(2), reps, warmup)
    two_rounds = int(st.rounds_max) == 2 and int(st.unconverged) == groups  # every group ran its second round
    d = _lib.nb_diagnostics()
    t_d0 = events(stream, lambda: _lib.check(L.nb_sim_diagnostics(sim._h, _lib.NB_DIAG_MOMENTS, C.byref(d))), reps, warmup)
    diag_reps = reps if n <= 65536 else min(reps, 3)  # (5.5e11 terms a call at 2^20)
    t_d1 = events(stream, lambda: _lib.check(L.nb_sim_diagnostics(
        sim._h, _lib.NB_DIAG_MOMENTS | _lib.NB_DIAG_POTENTIAL, C.byref(d))), diag_reps, min(warmup, 1))
    tw = []
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        bg = sim.bound_groups(link, min_members=args.min_members, max_iter=args.max_iter, max_group=max_group)
        if r >= warmup:
            tw.append((time.perf_counter() - t0) * 1e3)
    round_ms = t_2 - t_1
    terms = groups * members * members
    total_launches, per_round = launches(n, cap, args.max_iter, max_group, args.tile)
    row = {"case": name, "n": n, "groups": groups, "members": members, "link": link, "reps": reps,
           "kernels_all_rounds_ms": t_all, "max_iter_1_ms": t_1, "max_iter_2_ms": t_2, "round_ms": round_ms,
           "round_is_clean": two_rounds, "pair_terms_per_round": terms, "pair_rate": terms / (round_ms * 1e-3),
           "diag_pairs_ms": t_d1 - t_d0, "diag_rate": n * (n - 1) / 2 / ((t_d1 - t_d0) * 1e-3),
           "call_median_ms": float(np.median(tw)), "call_min_ms": float(np.min(tw)), "launches": total_launches,
           "pair_launches_per_round": per_round, "ns_per_body_round": round_ms * 1e6 / n, **full}
    row["rate_ratio"] = row["pair_rate"] / row["diag_rate"]
    if args.baseline_members > 0:
        from tests import bound_ref
        t0 = time.perf_counter()
        state = nb.as_floats(sim.read_particles())
        t_read = (time.perf_counter() - t0) * 1e3
        take = min(members, args.baseline_members)
        mem = np.flatnonzero(bg.group_of == 0)[:take]
        s64 = state[mem].astype(np.float64)
        t0 = time.perf_counter()
        u = bound_ref.unbind(s64[:, 0:3], s64[:, 3:6], s64[:, 9], bound_ref.coupling(G, DT), np.float64(np.float32(E)),
                             args.min_members, args.max_iter)
        row.update(read_ms=t_read, baseline_members=take, baseline_group_ms=(time.perf_counter() - t0) * 1e3,
                   baseline_rounds=int(u["iterations"]))
    sim.destroy()
    rows.append(row)
    print(json.dumps(row), flush=True)

lines = ["# tools/bench_bound.py: nb_sim_bound on a NaiveSim, ms, median of the reps (kernels: HIP events around a "
         "stats-only call, group finder included; round: max_iter 2 less max_iter 1; call: host clock, every output; "
         "min_members %d, max_iter %d, bound_tile %d, bound_chunk_len %d)" % (args.min_members, args.max_iter, args.tile,
                                                                              args.chunk_len),
         "# " + nb.version(),
         "# rate: pair terms of a round (groups x members^2) per second; diag: the diagnostics' pair pass on the same state "
         "in the same run (n (n - 1) / 2 terms); ratio: rate / diag.  baseline: read_particles, then the numpy rule on the "
         "first `of` members of one group, ms per group",
         "%-17s %8s %4s %9s %9s %9s %10s %10s %6s %9s %7s %6s %10s %7s %8s %9s %6s %6s" % (
             "case", "n", "reps", "kernels", "round", "call", "rate", "diag", "ratio", "ns/body", "launch", "/round",
             "pairs", "rounds", "bound", "baseline", "of", "read")]
for r in rows:
    lines.append("%-17s %8d %4d %9.3f %9.4f %9.3f %10.3e %10.3e %6.2f %9.3f %7d %6d %10.3e %7d %8d %9s %6s %6s" % (
        r["case"], r["n"], r["reps"], r["kernels_all_rounds_ms"], r["round_ms"], r["call_median_ms"], r["pair_rate"],
        r["diag_rate"], r["rate_ratio"], r["ns_per_body_round"], r["launches"], r["pair_launches_per_round"],
        r["pairs"], r["rounds_max"], r["bound_bodies"],
        "%.1f" % r["baseline_group_ms"] if "baseline_group_ms" in r else "-", r.get("baseline_members", "-"),
        "%.1f" % r["read_ms"] if "read_ms" in r else "-"))
print("\n".join(lines))
if args.table:
    with open(args.table, "w") as f:
        f.write("\n".join(lines) + "\n")
print(json.dumps({"bench": "bound_groups", "rows": len(rows), "device": nb.version()}))
