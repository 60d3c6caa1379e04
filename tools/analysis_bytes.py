"""Every output byte of the three key-sorting analysis passes (nb_sim_map, nb_sim_fof, nb_sim_knn) over a fixed list
of states, one sha256 per row: run it once per library (NB_LIB names the library; each run its own process) and
compare the two listings with diff -- a refactor of csrc/nb_map.hip, nb_fof.hip, nb_knn.hip or
nb_analysis_sort.hpp must leave them identical.  The passes are called through the raw C entry points with every
buffer pre-filled, as the suites' _raw do, so bytes a call should not have written count too.  The states: the three
inits at 4,097 / 70,001 / 524,289 bodies on a NaiveSim and on a TreeSim after one step (the `state` rows hash what
the passes saw, so a trajectory that differs is told apart from a pass that does); the concentrated states of
tools/bench_map.py, bench_fof.py and bench_knn.py at 2^18 bodies; a state with non-finite bodies; a refused fof
link.  usage: NB_LIB=path/to/libnbody_hip.so python tools/analysis_bytes.py > listing.txt"""
import ctypes as C
import hashlib
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wgpu_n_body_amd as nb  # noqa: E402
from wgpu_n_body_amd import _lib  # noqa: E402

INITS = {"uniform": nb.inits.uniform_init, "disc": nb.inits.disc_init, "spherical": nb.inits.spherical_init}
FILL, SENTINEL = 0xDEADBEEF, -12345.5
rows = 0


def emit(name, what, rc, *bufs):
    global rows
    rows += 1
    h = hashlib.sha256()
    for b in bufs:
        h.update(b.tobytes() if isinstance(b, np.ndarray) else bytes(b))
    print(f"{name:34s} {what:5s} rc={rc:<3d} {h.hexdigest()}", flush=True)


def init_state(init, n):
    return nb.as_floats(INITS[init](nb.SimParams(particle_num=n), seed=1)).copy()


def spacing_link(state, spacings=0.2):
    """tools/bench_fof.py's: in mean spacings of the volume that holds the middle 80 % of the bodies on every axis"""
    pos = state[np.isfinite(state).all(axis=1), 0:3]
    lo, hi = np.percentile(pos, [10, 90], axis=0)
    inside = np.all((pos >= lo) & (pos <= hi), axis=1).sum()
    return spacings * float((np.prod(np.maximum(hi - lo, 1e-6)) / max(inside, 1)) ** (1.0 / 3.0))


def run(name, state, kind="naive", link=None, grid=(100, 60), extent=(-0.5, 0.5, -0.4, 0.4), axis=(1.0, 2.0, 3.0)):
    n = state.shape[0]
    sp = nb.SimParams(particle_num=n)
    if kind == "tree":
        sim = nb.TreeSim.from_particles(sp, nb.AddParams.TreeSimParams(0.75), state)
        sim.encode()
        state = nb.as_floats(sim.read_particles()).copy()
    else:
        sim = nb.NaiveSim.from_particles(sp, None, state)
    emit(name, "state", 0, state)
    L = _lib.lib()
    # map: the centre of mass, velocities on, six planes offered
    p = _lib.nb_map_params()
    p.width, p.height = grid
    p.flags = _lib.NB_MAP_VELOCITY | _lib.NB_MAP_CENTER_COM
    for a in range(3):
        p.axis[a] = axis[a]
    p.x_range[0], p.x_range[1], p.y_range[0], p.y_range[1] = extent
    p.depth_range[0], p.depth_range[1] = -math.inf, math.inf
    cells, st = grid[0] * grid[1], _lib.nb_map_stats()
    counts, planes = np.full(cells, FILL, np.uint32), np.full(6 * cells, SENTINEL)
    rc = L.nb_sim_map(sim._h, C.byref(p), counts.ctypes.data, planes.ctypes.data, C.byref(st))
    emit(name, "map", rc, counts, planes, st)
    # fof: min_members 2, room for every possible row
    q = _lib.nb_fof_params()
    q.link, q.min_members = (spacing_link(state) if link is None else link), 2
    labels, group_of = np.full(n, FILL, np.uint32), np.full(n, FILL, np.uint32)
    cat = np.zeros(n // 2 + 1, _lib.FOF_GROUP_DTYPE)
    cat["label"] = FILL
    fs = _lib.nb_fof_stats()
    rc = L.nb_sim_fof(sim._h, C.byref(q), labels.ctypes.data, group_of.ctypes.data, cat.ctypes.data, n // 2,
                      C.byref(fs))
    emit(name, "fof", rc, labels, group_of, cat, fs)
    # knn: k = 6
    k = _lib.nb_knn_params()
    k.k = 6
    r2, mass_in, density = np.full(n + 1, -7.0), np.full(n + 1, -7.0), np.full(n + 1, -7.0)
    kth, ks = np.full(n + 1, FILL, np.uint32), _lib.nb_knn_stats()
    rc = L.nb_sim_knn(sim._h, C.byref(k), r2.ctypes.data, kth.ctypes.data, mass_in.ctypes.data, density.ctypes.data,
                      C.byref(ks))
    emit(name, "knn", rc, r2, kth, mass_in, density, ks)
    sim.destroy()


if nb.device_count() < 1:
    sys.exit("analysis_bytes needs a HIP device (no CPU fallback)")
print("# " + nb.version())
for n in (4097, 70001, 524289):
    for init in INITS:
        for kind in ("naive", "tree"):
            run(f"{init} {n} {kind}", init_state(init, n), kind)

N, SQUARE, Z = 1 << 18, (-1.0, 1.0, -1.0, 1.0), (0.0, 0.0, 1.0)
rng = np.random.default_rng(2)
for conc, span, (i0, j0) in (("cell", 1.0, (300, 700)), ("tile", 8.0, (296, 696))):  # tools/bench_map.py
    s = init_state("spherical", N)
    s[:, 0] = -1.0 + 2.0 * (i0 + rng.uniform(0.01, span - 0.01, N)) / 1024
    s[:, 1] = -1.0 + 2.0 * (j0 + rng.uniform(0.01, span - 0.01, N)) / 1024
    run(f"map one {conc} 2^18", s, grid=(1024, 1024), extent=SQUARE, axis=Z)
s = init_state("uniform", N)                                                          # tools/bench_fof.py
s[:, 0:3] = 0.3 + rng.uniform(0.0, 0.01 / 4, (N, 3))
run("fof one cell 2^18", s, link=0.01)
s[N // 2:, 0] += 1.5 * 0.01
run("fof two blobs 2^18", s, link=0.01)
run("fof giant 2^18", init_state("uniform", N), link=spacing_link(init_state("uniform", N), 2.0))
s = init_state("uniform", N)                                                          # tools/bench_knn.py
s[:, 0:3] = rng.uniform(0.0, 1.0, (N, 3))
s[0, 0:3] = (float(1 << 20), 0.0, 0.0)
run("knn outlier 2^18", s)
s[:, 0:3] = rng.uniform(0.0, 1e-3, (N, 3))
s[N // 2:, 0] += 100.0
run("knn two blobs 2^18", s)
s[:, 0:3] = rng.uniform(-1.0, 1.0, (1024, 3)).astype(np.float32)[rng.permutation(N) % 1024]
run("knn 1024 points 2^18", s)

s = init_state("disc", 70001)                                                         # non-finite bodies
who, cols = rng.choice(70001, 40, replace=False), rng.choice([0, 1, 2, 3, 4, 5, 9], 40)
s[who, cols] = rng.choice([np.nan, np.inf, -np.inf], 40)
run("disc 70001 nonfinite", s)
s = init_state("uniform", 4097)                                                       # a refused fof link
s[17, 0] = 3.0e4
run("uniform 4097 far body", s, link=0.01)
print(f"# {rows} rows")
