"""fp64 host references for the diagnostics tests (include/nbody.h "Diagnostics"): the potential
psi of the reference's pair force m_j g / (r^3 + e), the pair sum W and the body moments.  They
live with the tests on purpose: the package has no CPU path for them."""
import numpy as np


def psi64(r, e):
    """psi(r) = integral_r^inf ds / (s^3 + e) in fp64: the closed form where r^3 < 8e, the series
    1/(2r^2) sum_k (-x)^k 2/(3k+2), x = e/r^3 <= 1/8, elsewhere (the closed form cancels there)."""
    r = np.asarray(r, dtype=np.float64)
    out = np.empty_like(r)
    far = r ** 3 >= 8.0 * e
    if e > 0:
        a = np.cbrt(e)
        rn = r[~far]
        out[~far] = (np.arctan2(np.sqrt(3.0) * a, 2.0 * rn - a) / (np.sqrt(3.0) * a * a)
                     - np.log1p(3.0 * a * rn / (rn * rn - a * rn + a * a)) / (6.0 * a * a))
    rf = r[far]
    with np.errstate(divide="ignore", invalid="ignore"):
        x = e / rf ** 3 if e > 0 else np.zeros_like(rf)
        s = np.zeros_like(rf)
        for k in range(24)[::-1]:  # x <= 1/8: 24 terms are far below fp64 rounding
            s = s * (-x) + 2.0 / (3 * k + 2)
        out[far] = s / (2.0 * rf * rf)
    return out


def body_mask(state):
    """Bodies with finite position, velocity and mass (the others are left out of every sum)."""
    s = np.asarray(state, dtype=np.float32)
    return np.isfinite(s[:, [0, 1, 2, 3, 4, 5, 9]]).all(axis=1)


def pair_sum64(state, e, rows=512):
    """W = sum_{i<j} m_i m_j psi(r_ij), fp64, with r from the fp32 positions."""
    s = np.asarray(state, dtype=np.float32)[body_mask(state)]
    x, m = s[:, 0:3].astype(np.float64), s[:, 9].astype(np.float64)
    n, w = len(m), 0.0
    for i0 in range(0, n, rows):
        i1 = min(n, i0 + rows)
        d = x[None, i0 + 1:, :] - x[i0:i1, None, :]  # j from i0 + 1: the triangle below is masked
        r = np.sqrt((d * d).sum(axis=2))
        p = psi64(r.ravel(), e).reshape(r.shape)
        jj = np.arange(i0 + 1, n)[None, :]
        ii = np.arange(i0, i1)[:, None]
        p = np.where(jj > ii, p, 0.0)
        w += float((m[i0:i1, None] * (m[None, i0 + 1:] * p)).sum())
    return w


def moments64(state):
    """dict of the fp64 moments, and of the sums of |term| per field (the tolerance scale)."""
    s = np.asarray(state, dtype=np.float32)
    ok = body_mask(s)
    t = s[ok].astype(np.float64)
    x, v, m = t[:, 0:3], t[:, 3:6], t[:, 9]
    mx, mv, lx = m[:, None] * x, m[:, None] * v, m[:, None] * np.cross(x, v)
    k = 0.5 * m * (v * v).sum(axis=1)
    speed = np.sqrt((v * v).sum(axis=1))
    return {
        "nonfinite": int((~ok).sum()), "mass": m.sum(), "mx": mx.sum(axis=0), "momentum": mv.sum(axis=0),
        "angular_momentum": lx.sum(axis=0), "kinetic": k.sum(), "max_speed": speed.max() if len(speed) else 0.0,
        "scale": {"mass": np.abs(m).sum(), "mx": np.abs(mx).sum(axis=0), "momentum": np.abs(mv).sum(axis=0),
                  "angular_momentum": np.abs(lx).sum(axis=0), "kinetic": np.abs(k).sum()},
    }


def energy64(state, g, e, dt):
    """(K, U, E) on the host: U = -g dt W."""
    k = moments64(state)["kinetic"]
    u = -np.float64(np.float32(g)) * np.float64(np.float32(dt)) * pair_sum64(state, np.float64(np.float32(e)))
    return k, u, k + u
