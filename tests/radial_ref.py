"""The radial-profile rule of include/nbody.h ("Radial profiles"), restated in numpy from
the header text: binary64 from the binary32 state, one rounding per operation (numpy never contracts),
the bin decided on r^2 against the squared edges.  Used by tests/test_radial.py (closed forms) and
tests/test_radial_gpu.py (parity with the device)."""
import numpy as np

BIN_SUMS = ("mass", "m_r", "m_ur", "m_ur2", "m_uphi", "m_uphi2", "m_u2", "ang")


def unit_axis(axis):
    a = np.asarray(axis, dtype=np.float64)
    return a / np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])


def _dot(a, b):
    return (a[:, 0] * b[0] + a[:, 1] * b[1]) + a[:, 2] * b[2] if np.ndim(b) == 1 else \
        (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def profile64(state, edges, center=(0.0, 0.0, 0.0), velocity=(0.0, 0.0, 0.0), axis=None):
    """state: float32[n, 10] (px py pz vx vy vz ax ay az mass).  axis: None (spherical) or three numbers
    (cylindrical).  Returns a dict: the header's integers and sums (`total_mass` is the header's
    `mass`), per-bin arrays `count` and the BIN_SUMS, and under "scale" the sum of |term| of every sum
    (what a tolerance is relative to)."""
    state = np.asarray(state, dtype=np.float32)
    edges = np.asarray(edges, dtype=np.float64)
    nbins = edges.shape[0] - 1
    n = state.shape[0]
    x, v, m = (state[:, 0:3].astype(np.float64), state[:, 3:6].astype(np.float64), state[:, 9].astype(np.float64))
    ok = np.isfinite(x).all(1) & np.isfinite(v).all(1) & np.isfinite(m)
    x, v, m = x[ok], v[ok], m[ok]
    c, vc = np.asarray(center, dtype=np.float64), np.asarray(velocity, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = x - c
        u = v - vc
        if axis is None:
            nh = np.zeros(3)
            q = d
        else:
            nh = unit_axis(axis)
            h = _dot(d, nh)
            q = d - h[:, None] * nh
        r2 = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
        e2 = edges * edges
        cnt = np.searchsorted(e2, r2, side="right")  # edges at or below r2
        cnt[np.isnan(r2)] = 0
        r = np.sqrt(r2)
        zero = r2 == 0.0
        rs = np.where(zero, 1.0, r)
        ur = np.where(zero, 0.0, _dot(q, u) / rs)
        uphi = np.zeros_like(ur) if axis is None else np.where(zero, 0.0, _dot(_cross(q, u), nh) / rs)
        terms = {"mass": m, "m_r": m * r, "m_ur": m * ur, "m_ur2": (m * ur) * ur, "m_uphi": m * uphi,
                 "m_uphi2": (m * uphi) * uphi, "m_u2": m * _dot(u, u), "ang": m[:, None] * _cross(d, u)}
        sh = np.stack([(m * d[:, 0]) * d[:, 0], (m * d[:, 1]) * d[:, 1], (m * d[:, 2]) * d[:, 2],
                       (m * d[:, 0]) * d[:, 1], (m * d[:, 0]) * d[:, 2], (m * d[:, 1]) * d[:, 2]], axis=1)
    inside, outside = cnt == 0, cnt == nbins + 1
    binned = ~inside & ~outside
    k = cnt[binned] - 1

    def per_bin(t):
        t = t[binned]
        if t.ndim == 2:
            return np.stack([np.bincount(k, weights=t[:, a], minlength=nbins) for a in range(t.shape[1])], axis=1)
        return np.bincount(k, weights=t, minlength=nbins)

    out = dict(n=n, nonfinite=int(n - ok.sum()), nbins=nbins, inside_count=int(inside.sum()),
               outside_count=int(outside.sum()), inside_mass=m[inside].sum(), outside_mass=m[outside].sum(),
               total_mass=m.sum(), shape=sh[~outside].sum(0), axis=nh,
               count=np.bincount(k, minlength=nbins).astype(np.uint64))
    scale = dict(inside_mass=np.abs(m[inside]).sum(), outside_mass=np.abs(m[outside]).sum(),
                 total_mass=np.abs(m).sum(), shape=np.abs(sh[~outside]).sum(0))
    for name in BIN_SUMS:
        out[name] = per_bin(terms[name])
        scale[name] = per_bin(np.abs(terms[name]))
    out["scale"] = scale
    return out


def lagrangian64(edges, bin_mass, inside_mass, mass, fractions):
    """nb_radial_lagrangian restated: linear in r inside the bin where the cumulative mass crosses."""
    out = []
    for f in fractions:
        target, cum, r = f * mass, inside_mass, np.nan
        if 0.0 < f < 1.0 and target >= cum:
            for b, mb in enumerate(bin_mass):
                if target <= cum + mb:
                    r = edges[b] + (target - cum) / mb * (edges[b + 1] - edges[b]) if mb > 0 else edges[b]
                    break
                cum = cum + mb
        out.append(r)
    return np.array(out)
