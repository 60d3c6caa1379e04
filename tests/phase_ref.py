"""The phase-map rule of include/nbody.h ("Phase maps"), restated in numpy from the header text:
binary64 from the binary32 state, one rounding per operation (numpy never contracts), only + - * / and sqrt, the
cell decided by comparisons against the caller's edges, the sums by math.fsum (the binary64 sum, rounded once).
Used by tests/test_phase.py (hand cases) and tests/test_phase_gpu.py (parity with the device)."""
import math

import numpy as np

from tests.map_ref import frame

QUANTITIES = ("a", "b", "h", "R", "r", "ua", "ub", "w", "u_R", "u_phi", "u_r", "u_t", "speed", "j_z", "j", "e_kin",
              "mass", "value")
PLANES = ("mass", "m_q", "m_q2")


def _dot(a, b):
    return (a[:, 0] * b[0] + a[:, 1] * b[1]) + a[:, 2] * b[2]


def quantities(x, v, m, axis=(0.0, 1.0, 0.0), center=(0.0, 0.0, 0.0), velocity=(0.0, 0.0, 0.0), values=None):
    """Every quantity of the table for the bodies x, v (float64[n, 3], converted from binary32) and m: a dict of
    float64[n].  "value" is there when values is given."""
    c, vc = np.asarray(center, dtype=np.float64), np.asarray(velocity, dtype=np.float64)
    nh, e1, e2 = frame(axis)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = x - c
        u = v - vc
        a, b, h = _dot(d, e1), _dot(d, e2), _dot(d, nh)
        ua, ub, w = _dot(u, e1), _dot(u, e2), _dot(u, nh)
        R = np.sqrt(a * a + b * b)
        r = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        u2 = (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]
        du = (d[:, 0] * u[:, 0] + d[:, 1] * u[:, 1]) + d[:, 2] * u[:, 2]
        jx = d[:, 1] * u[:, 2] - d[:, 2] * u[:, 1]
        jy = d[:, 2] * u[:, 0] - d[:, 0] * u[:, 2]
        jz = d[:, 0] * u[:, 1] - d[:, 1] * u[:, 0]
        u_r = du / r
        t = u2 - u_r * u_r
        t = np.where(t < 0.0, 0.0, t)  # (a NaN stays a NaN)
        out = {"a": a, "b": b, "h": h, "R": R, "r": r, "ua": ua, "ub": ub, "w": w,
               "u_R": (a * ua + b * ub) / R, "u_phi": (a * ub - b * ua) / R, "u_r": u_r, "u_t": np.sqrt(t),
               "speed": np.sqrt(u2), "j_z": a * ub - b * ua, "j": np.sqrt((jx * jx + jy * jy) + jz * jz),
               "e_kin": 0.5 * u2, "mass": m.copy()}
    if values is not None:
        out["value"] = np.asarray(values, dtype=np.float64)
    return out


def cell_of(edges, x):
    """The i with edges[i] <= x < edges[i + 1] per element, -1 where there is none (a NaN is in none)."""
    e = np.asarray(edges, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        inside = (x >= e[0]) & (x < e[-1])
    i = np.searchsorted(e, np.where(inside, x, e[0]), side="right") - 1
    return np.where(inside, i, -1)


def phase64(state, x, y, x_edges, y_edges, weight=None, values=None, axis=(0.0, 1.0, 0.0), center=(0.0, 0.0, 0.0),
            velocity=(0.0, 0.0, 0.0)):
    """state: float32[n, 10] (px py pz vx vy vz ax ay az mass).  Returns a dict: the integers and sums of
    nb_phase_stats (`total_mass` is its `mass`), `counts` (H, W) and the PLANES (H, W), and under "scale" the sum of
    |term| of every sum (what a tolerance is relative to)."""
    state = np.asarray(state, dtype=np.float32)
    n = state.shape[0]
    pos, vel, m = (state[:, 0:3].astype(np.float64), state[:, 3:6].astype(np.float64), state[:, 9].astype(np.float64))
    ok = np.isfinite(pos).all(1) & np.isfinite(vel).all(1) & np.isfinite(m)
    vals = None if values is None else np.asarray(values, dtype=np.float64)[ok]
    pos, vel, m = pos[ok], vel[ok], m[ok]
    q = quantities(pos, vel, m, axis, center, velocity, vals)
    xe, ye = np.asarray(x_edges, dtype=np.float64), np.asarray(y_edges, dtype=np.float64)
    W, H = len(xe) - 1, len(ye) - 1
    qx, qy = q[x], q[y]
    defined = np.isfinite(qx) & np.isfinite(qy)
    if weight is not None:
        defined &= np.isfinite(q[weight])
    i, j = cell_of(xe, qx), cell_of(ye, qy)
    binned = defined & (i >= 0) & (j >= 0)
    cell = (j * W + i)[binned]
    with np.errstate(invalid="ignore", over="ignore"):
        terms = {"mass": m}
        if weight is not None:
            terms["m_q"] = m * q[weight]
            terms["m_q2"] = (m * q[weight]) * q[weight]

    def per_cell(t):
        lists = {}
        for c, v in zip(cell.tolist(), t[binned].tolist()):
            lists.setdefault(c, []).append(v)
        grid = np.zeros(W * H)
        for c, l in lists.items():
            grid[c] = math.fsum(l)
        return grid.reshape(H, W)

    fs = lambda a: math.fsum(a.tolist())  # noqa: E731
    nh, e1, e2 = frame(axis)
    out = dict(n=n, nonfinite=int(n - ok.sum()), binned_count=int(binned.sum()), outside_count=int((~binned).sum()),
               undefined_count=int((~defined).sum()), binned_mass=fs(m[binned]), outside_mass=fs(m[~binned]),
               total_mass=fs(m), n_hat=nh, e1=e1, e2=e2,
               counts=np.bincount(cell, minlength=W * H).reshape(H, W).astype(np.uint32))
    scale = dict(binned_mass=fs(np.abs(m[binned])), outside_mass=fs(np.abs(m[~binned])), total_mass=fs(np.abs(m)))
    for name, t in terms.items():
        out[name] = per_cell(t)
        scale[name] = per_cell(np.abs(t))
    out["max_count"] = int(out["counts"].max())
    out["scale"] = scale
    return out
