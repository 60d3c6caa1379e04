"""The projected-map rule of include/nbody.h ("Projected maps"), restated in numpy from the
header text: binary64 from the binary32 state, one rounding per operation (numpy never contracts), the
cell decided by comparisons against the edges.  Used by tests/test_map.py (a plain double loop) and
tests/test_map_gpu.py (parity with the device)."""
import numpy as np

PLANES = ("mass", "m_ua", "m_ub", "m_w", "m_w2", "m_u2")


def frame(axis):
    """n_hat, e1, e2: the axis normalised; the coordinate axis of the smallest |n_k| (the lowest index on
    ties) made orthogonal to it and normalised; their cross product."""
    a = np.asarray(axis, dtype=np.float64)
    n = a / np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    s = int(np.argmin(np.abs(n)))  # (argmin returns the lowest index on ties)
    e1 = np.array([(1.0 if k == s else 0.0) - n[s] * n[k] for k in range(3)])
    e1 = e1 / np.sqrt((e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2])
    e2 = np.array([n[1] * e1[2] - n[2] * e1[1], n[2] * e1[0] - n[0] * e1[2], n[0] * e1[1] - n[1] * e1[0]])
    return n, e1, e2


def edges(lo, hi, cells):
    """lo + i ((hi - lo) / cells) for i < cells, then hi exactly."""
    lo, hi = np.float64(lo), np.float64(hi)
    d = (hi - lo) / np.float64(cells)
    e = lo + np.arange(cells + 1, dtype=np.float64) * d
    e[cells] = hi
    return e


def _dot(a, b):
    return (a[:, 0] * b[0] + a[:, 1] * b[1]) + a[:, 2] * b[2]


def map64(state, width, height, extent, axis=(0.0, 1.0, 0.0), center=(0.0, 0.0, 0.0), velocity=(0.0, 0.0, 0.0),
          depth=(-np.inf, np.inf)):
    """state: float32[n, 10] (px py pz vx vy vz ax ay az mass).  extent: (x0, x1, y0, y1).  Returns a dict:
    the integers and sums of nb_map_stats (`total_mass` is its `mass`), `counts` (H, W) and the six PLANES
    (H, W), and under "scale" the sum of |term| of every sum (what a tolerance is relative to)."""
    state = np.asarray(state, dtype=np.float32)
    n = state.shape[0]
    x, v, m = (state[:, 0:3].astype(np.float64), state[:, 3:6].astype(np.float64), state[:, 9].astype(np.float64))
    ok = np.isfinite(x).all(1) & np.isfinite(v).all(1) & np.isfinite(m)
    x, v, m = x[ok], v[ok], m[ok]
    c, vc = np.asarray(center, dtype=np.float64), np.asarray(velocity, dtype=np.float64)
    nh, e1, e2 = frame(axis)
    xe, ye = edges(extent[0], extent[1], width), edges(extent[2], extent[3], height)
    with np.errstate(invalid="ignore"):
        d = x - c
        u = v - vc
        a, b, h = _dot(d, e1), _dot(d, e2), _dot(d, nh)
        ua, ub, w = _dot(u, e1), _dot(u, e2), _dot(u, nh)
        inside = (a >= xe[0]) & (a < xe[width]) & (b >= ye[0]) & (b < ye[height]) & (h >= depth[0]) & (h < depth[1])
        terms = {"mass": m, "m_ua": m * ua, "m_ub": m * ub, "m_w": m * w, "m_w2": (m * w) * w,
                 "m_u2": m * ((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])}
    i = np.searchsorted(xe, a[inside], side="right") - 1  # xe[i] <= a < xe[i + 1]
    j = np.searchsorted(ye, b[inside], side="right") - 1
    cell = j * width + i
    cells = width * height

    def per_cell(t):
        return np.bincount(cell, weights=t[inside], minlength=cells).reshape(height, width)

    out = dict(n=n, nonfinite=int(n - ok.sum()), binned_count=int(inside.sum()), outside_count=int((~inside).sum()),
               binned_mass=m[inside].sum(), outside_mass=m[~inside].sum(), total_mass=m.sum(),
               n_hat=nh, e1=e1, e2=e2, x_edges=xe, y_edges=ye,
               counts=np.bincount(cell, minlength=cells).reshape(height, width).astype(np.uint32))
    scale = dict(binned_mass=np.abs(m[inside]).sum(), outside_mass=np.abs(m[~inside]).sum(),
                 total_mass=np.abs(m).sum())
    for name in PLANES:
        out[name] = per_cell(terms[name])
        scale[name] = per_cell(np.abs(terms[name]))
    out["max_count"] = int(out["counts"].max())
    out["scale"] = scale
    return out
