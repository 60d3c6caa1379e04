"""The orbit-stability rule of include/nbody.h ("Orbit stability"), restated in numpy from the header
text around two callbacks: the field sample and the tensor sample at the points of an evaluation.  With the binary64
all-pairs model (field_ref.field64 + tidal_ref.tidal64, or exact64 below at unrounded points) it is the model; with
the device's own field() and tidal_tensor() it is a replay whose every bit the device must reproduce.  numpy never
contracts, and frexp / ldexp restate the renormalisation exactly.  The tracers' own lines are tests/orbit_ref.py's."""
import numpy as np

from tests import map_ref
from tests import orbit_ref as R
from tests import tidal_ref as T

MUTATIONS = ("no_turn", "antisymmetric_xy", "kappa_unscaled")
NO_STEP = np.uint64(2 ** 64 - 1)
INT64_MIN = np.iinfo(np.int64).min


def turn(dx, frame, omega, c, s):
    """q of a deviation: orbit_ref.point's lines without the centre (and never rounded to fp32)."""
    if omega == 0.0:
        return dx.copy()
    n, e1, e2 = frame
    a, b, l = R._dot(dx, e1), R._dot(dx, e2), R._dot(dx, n)
    ar, br = a * c + b * s, b * c - a * s
    return (ar[:, None] * e1 + br[:, None] * e2) + l[:, None] * n


def apply_tensor(t6, q):
    """t_a = (T_a0 q_0 + T_a1 q_1) + T_a2 q_2 with T from (xx, yy, zz, xy, xz, yz)."""
    xx, yy, zz, xy, xz, yz = (t6[:, k] for k in range(6))
    return np.stack([(xx * q[:, 0] + xy * q[:, 1]) + xz * q[:, 2],
                     (xy * q[:, 0] + yy * q[:, 1]) + yz * q[:, 2],
                     (xz * q[:, 0] + yz * q[:, 1]) + zz * q[:, 2]], axis=1)


def stability(sample, tensor, pos, vel, dev0, *, dt, steps, every=None, renorm_log2=32, log2_0=None, omega=0.0,
              axis=(0.0, 1.0, 0.0), center=(0.0, 0.0, 0.0), accel_scale=1.0, step0=0, phase=R.phase_numpy, frame=None,
              round_points=True, mutation=None):
    """dict: pos, vel (R, M, 3); dev (R, M, D, 6), log2 (R, M, D); peak_log2, peak_step, renorms (M, D); coincident
    (M,), step (R,).  sample(points, False) -> (acc, potential, coincident) as orbit_ref's; tensor(points) -> (M, 6)
    in the order xx, yy, zz, xy, xz, yz, NaN at a non-finite point.  renorm_log2=None never renormalises.
    round_points=False hands the callbacks the binary64 points (the model of the finite-difference test).
    mutation: one of MUTATIONS, a wrong rule."""
    x = np.array(pos, dtype=np.float64).reshape(-1, 3)
    v = np.array(vel, dtype=np.float64).reshape(-1, 3)
    m = x.shape[0]
    dev = np.array(dev0, dtype=np.float64).reshape(m, -1, 6)
    D = dev.shape[1]
    log2 = np.zeros((m, D), np.int64) if log2_0 is None else np.array(np.broadcast_to(log2_0, (m, D)), dtype=np.int64)
    bad = ~(np.isfinite(x).all(1) & np.isfinite(v).all(1))
    x[bad], v[bad], dev[bad] = np.nan, np.nan, np.nan
    center = np.asarray(center, dtype=np.float64)
    frame = frame if frame is not None else (map_ref.frame(axis) if omega != 0.0 else None)
    dt, scale, omega = np.float64(dt), np.float64(accel_scale), float(omega)
    h = dt / 2
    every = steps if every is None else every
    due = R.records(steps, every)
    out = {"pos": np.empty((len(due), m, 3)), "vel": np.empty((len(due), m, 3)),
           "dev": np.empty((len(due), m, D, 6)), "log2": np.empty((len(due), m, D), np.int64),
           "peak_log2": np.full((m, D), INT64_MIN, np.int64), "peak_step": np.full((m, D), NO_STEP, np.uint64),
           "renorms": np.zeros((m, D), np.uint32), "coincident": np.zeros(m, np.int64),
           "step": np.array(due, dtype=np.uint64) + np.uint64(step0)}
    with np.errstate(all="ignore"):
        for k in range(steps + 1):
            c, s = phase(omega, float(dt), step0 + k)
            q = R.point(x, frame, center, omega, c, s)
            p = q.astype(np.float32) if round_points else q
            acc, _, co = sample(p, False)
            out["coincident"] += co
            t6 = scale * np.asarray(tensor(p), dtype=np.float64)
            kick = R.turn_back(scale * acc, frame, omega, c, s) * h
            if k > 0:
                v = v + kick
            for j in range(D):
                dx, dv = dev[:, j, 0:3], dev[:, j, 3:6]
                qd = dx.copy() if mutation == "no_turn" else turn(dx, frame, omega, c, s)
                t = apply_tensor(t6, qd)
                if mutation == "antisymmetric_xy":  # T_yx = -T_xy: the second row's first term with the other sign
                    t[:, 1] = (-t6[:, 3] * qd[:, 0] + t6[:, 1] * qd[:, 1]) + t6[:, 5] * qd[:, 2]
                kappa = R.turn_back(t, frame, omega, c, s) * h
                if k > 0:
                    dv = dv + kappa
                six = np.concatenate([dx, dv], axis=1)
                mu = np.abs(six).max(axis=1)
                live = np.isfinite(six).all(axis=1) & (mu != 0.0)
                E = np.where(live, np.frexp(np.where(live, mu, 1.0))[1].astype(np.int64) - 1, 0)
                peak = log2[:, j] + E
                up = live & (peak > out["peak_log2"][:, j])
                out["peak_log2"][up, j], out["peak_step"][up, j] = peak[up], np.uint64(step0 + k)
                if k > 0 and renorm_log2 is not None:
                    re = live & (np.abs(E) >= renorm_log2)
                    shift = np.where(re, -E, 0).astype(np.int32)
                    six = np.ldexp(six, shift[:, None])
                    if mutation != "kappa_unscaled":
                        kappa = np.ldexp(kappa, shift[:, None])
                    log2[:, j] += np.where(re, E, 0)
                    out["renorms"][:, j] += re.astype(np.uint32)
                dx, dv = six[:, 0:3], six[:, 3:6]
                if k in due:
                    r = due.index(k)
                    out["dev"][r, :, j, 0:3], out["dev"][r, :, j, 3:6], out["log2"][r, :, j] = dx, dv, log2[:, j]
                if k < steps:
                    dv = dv + kappa
                    dx = dx + dv * dt
                dev[:, j, 0:3], dev[:, j, 3:6] = dx, dv
            if k in due:
                r = due.index(k)
                out["pos"][r], out["vel"][r] = x, v
            if k < steps:
                v = v + kick
                x = x + v * dt
    return out


def vectors(out):
    """(R, M, D, 6): the vectors the records stand for, dev * 2^log2 (exact while it neither under- nor overflows)."""
    return np.ldexp(out["dev"], out["log2"][..., None].astype(np.int32))


def symplectic_form(d1, d2):
    """omega(d1, d2) = dx1 . dv2 - dx2 . dv1 over the last axis."""
    return (d1[..., 0:3] * d2[..., 3:6]).sum(-1) - (d2[..., 0:3] * d1[..., 3:6]).sum(-1)


def symplectic_C(vec, K):
    """(M,): max_k |omega_k - omega_0| / (K 2^-53 max_k(|d1| |d2|)) of vectors 0 and 1 of vec (R, M, D, 6)."""
    d1, d2 = vec[:, :, 0], vec[:, :, 1]
    w = symplectic_form(d1, d2)
    scale = (np.linalg.norm(d1, axis=-1) * np.linalg.norm(d2, axis=-1)).max(axis=0)
    return np.abs(w - w[0]).max(axis=0) / (K * 2.0 ** -53 * scale)


def model64(state, g, e):
    """(sample, tensor): the binary64 all-pairs model at fp32 points (tests/field_ref.py, tests/tidal_ref.py)."""
    def tensor(points):
        return T.tidal64(state, points, g, e)["tensor6"]
    return R.all_pairs64(state, g, e), tensor


def exact64(state, g, e):
    """(sample, tensor): the same field and its exact gradient in binary64 at binary64 points -- the field whose
    tangent map a centred difference of two orbits measures."""
    s = np.asarray(state, dtype=np.float64)
    xb, mb = s[:, 0:3], s[:, 9]
    g, e = np.float64(np.float32(g)), np.float64(np.float32(e))

    def parts(points):
        p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
        d = xb[None, :, :] - p[:, None, :]
        r2 = (d * d).sum(-1)
        r = np.sqrt(r2)
        w = mb[None, :] / (r2 * r2 + e * r)
        return d, r2, r, w

    def sample(points, potential):
        d, _, _, w = parts(points)
        acc = g * (w[:, :, None] * d).sum(axis=1)
        return acc, np.full(acc.shape[0], np.nan), np.zeros(acc.shape[0], np.int64)

    def tensor(points):
        d, r2, r, w = parts(points)
        r3 = r2 * r
        wc = w * (4.0 * r3 + e) / (r2 * (r3 + e))
        t6 = np.stack([(wc * d[..., a] * d[..., b]).sum(axis=1) for a, b in T.PAIRS], axis=1)
        t6[:, :3] -= w.sum(axis=1)[:, None]
        return g * t6
    return sample, tensor


def device(sim):
    """(sample, tensor): the device's own field() and tidal_tensor(): the replay the device must match bit for bit."""
    def tensor(points):
        return sim.tidal_tensor(points).tensor.reshape(-1, 9)[:, [0, 4, 8, 1, 2, 5]]
    return R.device_field(sim), tensor


def derive(out, dev0, log2_0, dt, ks):
    """The formulas of nb_orbit_stability_derive in numpy: log_growth, lyapunov (R, M, D), sali, gali2 (R, M)."""
    def unit(d):
        ex = np.frexp(np.abs(d).max(axis=-1))[1]
        s = np.ldexp(d, -ex[..., None])
        norm = np.sqrt((s * s).sum(-1))
        norm[~np.isfinite(d).all(-1) | (np.abs(d).max(axis=-1) == 0.0)] = np.nan  # a zero or non-finite vector
        return s / norm[..., None], ex * np.log(2.0) + np.log(norm)
    u, ln = unit(out["dev"])
    _, ln0 = unit(np.asarray(dev0, dtype=np.float64))
    lg = (out["log2"] - np.asarray(log2_0)[None]) * np.log(2.0) + ln - ln0[None]
    ks = np.asarray(ks, dtype=np.float64)
    with np.errstate(all="ignore"):
        ly = np.where(ks[:, None, None] > 0, lg / (ks[:, None, None] * dt), np.nan)
    if u.shape[2] < 2:
        nan = np.full(u.shape[:2], np.nan)
        return lg, ly, nan, nan.copy()
    u1, u2 = u[:, :, 0], u[:, :, 1]
    sali = np.minimum(np.linalg.norm(u1 + u2, axis=-1), np.linalg.norm(u1 - u2, axis=-1))
    wedge = u1[..., :, None] * u2[..., None, :] - u1[..., None, :] * u2[..., :, None]
    gali2 = np.sqrt((np.triu(wedge, 1) ** 2).sum((-1, -2)))
    return lg, ly, sali, gali2
