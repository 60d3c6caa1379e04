"""Renderer benchmark (nb_sim_render, csrc/nb_render.hip): milliseconds per frame of each kernel design
("render_design" 1 direct, 2 tiled) at the reference's two workloads, beside the step time of the same
simulator in the same process and the memory-traffic floor.

  A  bin/visualize.rs: TreeSim, 100,000-body disc, g 1e-5, dt 0.0016, theta 0.75; 1280 x 720 after 100 steps
  B  bin/headless.rs:  TreeSim, 4,000,000 uniform bodies, theta 0.75; 1920 x 1080 after 10 steps -- in tree
     (Morton) order as the TreeSim holds it, and the same bodies shuffled in a NaiveSim's buffer (an init-ordered
     buffer is in random spatial order)

  S  sweep: uniform and disc clouds of 25,000 .. 1,600,000 bodies in init order (NaiveSim) and in tree order
     (TreeSim after one step), at both sizes: where the designs cross

Frame time: HIP events on the simulator's stream around one render call that copies no image (kernels +
the 64-byte result copy), the designs alternating, `--reps` calls each after `--warmup`; median, min, max.
"copy": the extra host time of a call that also copies the RGBA image into pageable host memory.
Floor: (16 N + 4 W H [count write] + 4 W H [count read] + 4 W H [RGBA write]) bytes at the measured HBM copy
rate.  Prints one JSON line per case and the table; --out writes the table to a file.
Secondary to bench.py; used for DESIGN.md 6c."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # first: libnbody_hip.so then binds to the HIP runtime torch already loaded (the stream, the events)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wgpu_n_body_amd as nb  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--configs", nargs="*", default=["A", "B", "S"], help="A, B, and S: the sweep over body counts")
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--n-a", type=int, default=100000)
ap.add_argument("--n-b", type=int, default=4000000)
ap.add_argument("--out", default=None)
ap.add_argument("--frame", default=None, help="write configuration A's frame to this .ppm")
args = ap.parse_args()

if nb.device_count() < 1:
    sys.exit("bench_render needs a HIP device (no CPU fallback)")

HBM_BPS = 6.29e12  # measured float4 copy rate of the MI355X (8.0e12 is the specification)
DESIGNS = {1: "direct", 2: "tiled"}
stream = torch.cuda.Stream(0)
place = nb.Placement(0, 0, 1, stream.cuda_stream)


def frame_times(sim, width, height):
    """{design: ms array}, device time of calls that copy no image; the designs alternate."""
    from wgpu_n_body_amd import _lib
    p = nb.RenderParams.default(width, height).to_c()
    st = _lib.nb_render_stats()
    L = _lib.lib()
    out = {d: [] for d in DESIGNS}
    for rep in range(args.warmup + args.reps):
        for d in DESIGNS:
            sim.set_tuning("render_design", d)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            nb.check(L.nb_sim_render(sim._h, p, None, None, st))
            e1.record(stream)
            e1.synchronize()
            if rep >= args.warmup:
                out[d].append(e0.elapsed_time(e1))
    return {d: np.array(v) for d, v in out.items()}, st


def copy_time(sim, width, height, design):
    """Median extra host time (ms) of a call that also returns the RGBA image."""
    from wgpu_n_body_amd import _lib
    sim.set_tuning("render_design", design)
    p = nb.RenderParams.default(width, height).to_c()
    img = np.empty((height, width, 4), np.uint8)
    L = _lib.lib()
    with_img, without = [], []
    for rep in range(args.warmup + 10):
        for dst, acc in ((img.ctypes.data, with_img), (None, without)):
            t0 = time.perf_counter()
            nb.check(L.nb_sim_render(sim._h, p, dst, None, None))
            if rep >= args.warmup:
                acc.append(time.perf_counter() - t0)
    return (np.median(with_img) - np.median(without)) * 1e3


rows, lines = [], []


def case(name, sim, order, width, height, step_ms, copies=True):
    n = sim.sim_params().particle_num
    times, st = frame_times(sim, width, height)
    floor_ms = (16 * n + 12 * width * height) / HBM_BPS * 1e3
    for d, label in DESIGNS.items():
        t = times[d]
        row = {"config": name, "order": order, "n": n, "size": f"{width}x{height}", "design": label,
               "median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()), "reps": int(t.size),
               "copy_rgba_ms": float(copy_time(sim, width, height, d)) if copies else float("nan"), "step_ms": step_ms,
               "frame_over_step": float(np.median(t)) / step_ms if step_ms else None, "floor_ms": floor_ms,
               "fragments": int(st.fragments), "max_count": int(st.max_count), "drawn": int(st.drawn)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        ratio = f"{row['frame_over_step']:.3f}" if step_ms else "-"
        step = f"{step_ms:.3f}" if step_ms else "-"
        lines.append(f"{name:2s} {order:9s} {n:>8d} {row['size']:>9s} {label:7s} {row['median_ms']:9.4f} {row['min_ms']:9.4f} "
                     f"{row['max_ms']:9.4f} {row['copy_rgba_ms']:9.3f} {step:>9s} {ratio:>10s} {floor_ms:9.4f} "
                     f"{row['fragments']:>10d} {row['max_count']:>6d}")


def stepped(sp, theta, init, steps):
    sim = nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(theta), init, placement=place)
    for _ in range(steps):
        sim.encode()
    sim.wait()
    total, _ = sim.encode_n_timed(10)   # ten more steps, back to back, HIP events
    return sim, total / 10.0


if "A" in args.configs:
    sp = nb.SimParams(particle_num=args.n_a, g=1e-5, e=1e-4, dt=0.0016)          # bin/visualize.rs:26-31
    sim, step_ms = stepped(sp, 0.75, nb.inits.disc_init(sp, seed=1), 90)          # 100 steps in all
    case("A", sim, "tree", 1280, 720, step_ms)
    if args.frame:
        sim.set_tuning("render_design", 0)
        nb.write_ppm(args.frame, sim.render(1280, 720))
    sim.destroy()
if "B" in args.configs:
    sp = nb.SimParams(particle_num=args.n_b)                                     # bin/headless.rs:15-20 (the defaults)
    sim, step_ms = stepped(sp, 0.75, nb.inits.uniform_init(sp, seed=1), 0)        # 10 steps in all
    case("B", sim, "tree", 1920, 1080, step_ms)
    state = sim.read_particles()
    sim.destroy()
    state = state[np.random.default_rng(1).permutation(state.shape[0])]
    naive = nb.NaiveSim.from_particles(sp, None, state, placement=place)          # holds the buffer; never stepped
    case("B", naive, "shuffled", 1920, 1080, None)
    naive.destroy()

if "S" in args.configs:
    for init in ("uniform", "disc"):
        for n in (25000, 50000, 100000, 200000, 400000, 800000, 1600000):
            sp = nb.SimParams(particle_num=n)
            state = getattr(nb.inits, init + "_init")(sp, seed=1)
            for order in ("init", "tree"):
                if order == "init":
                    sim = nb.NaiveSim.from_particles(sp, None, state, placement=place)
                else:
                    sim = nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(0.75), state, placement=place)
                    sim.encode()
                    sim.wait()
                for width, height in ((1280, 720), (1920, 1080)):
                    case("S" + init[0], sim, order, width, height, None, copies=False)
                sim.destroy()

head = (f"# tools/bench_render.py: nb_sim_render, ms per frame (HIP events; no image copied), {args.reps} calls per design, "
        f"designs alternating\n# {nb.version()}\n# copy: extra host ms when the RGBA image is returned; step: ms per step of "
        f"the same TreeSim (10 back to back);\n# floor: (16 N + 12 W H) B at {HBM_BPS / 1e12:.2f} TB/s; cf Su / Sd: sweep, uniform / disc\n"
        f"{'cf':2s} {'order':9s} {'n':>8s} {'size':>9s} {'design':7s} {'median':>9s} {'min':>9s} {'max':>9s} {'copy':>9s} "
        f"{'step':>9s} {'frame/step':>10s} {'floor':>9s} {'fragments':>10s} {'maxcnt':>6s}")
table = head + "\n" + "\n".join(lines) + "\n"
print(table)
if args.out:
    with open(args.out, "w") as f:
        f.write(table)
print(json.dumps({"bench": "render", "rows": len(rows), "device": nb.version()}))
