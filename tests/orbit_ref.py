"""The orbit rule of include/nbody.h ("Orbits"), restated in numpy from the header text: binary64
+, -, x with one rounding per operation (numpy never contracts) around a field sample that a callback supplies.  The
callback is what decides what the restatement is: with all_pairs64 (tests/field_ref.py in binary64) it is the model
the device is measured against; with the device's own field() it is a replay whose every bit the device must
reproduce.  It lives with the tests on purpose: the package has no CPU path for it."""
import numpy as np

from tests import field_ref as F
from tests import map_ref


def records(steps, every):
    """The recorded k: 0, every, 2 every, ... and steps."""
    return [k for k in range(steps + 1) if k % every == 0 or k == steps]


def phase_numpy(omega, dt, k):
    """cos, sin of omega * ((double)k * dt); exactly (1, 0) for omega == 0."""
    if omega == 0.0:
        return 1.0, 0.0
    theta = np.float64(omega) * (np.float64(k) * np.float64(dt))
    return float(np.cos(theta)), float(np.sin(theta))


def _dot(a, b):
    return (a[:, 0] * b[0] + a[:, 1] * b[1]) + a[:, 2] * b[2]


def point(x, frame, center, omega, c, s):
    """q of an evaluation (binary64) -- x itself, or x turned by -theta about the axis through the centre."""
    if omega == 0.0:
        return x.copy()
    n, e1, e2 = frame
    d = x - center
    a, b, l = _dot(d, e1), _dot(d, e2), _dot(d, n)
    ar, br = a * c + b * s, b * c - a * s
    return center + ((ar[:, None] * e1 + br[:, None] * e2) + l[:, None] * n)


def turn_back(a_snap, frame, omega, c, s):
    if omega == 0.0:
        return a_snap.copy()
    n, e1, e2 = frame
    u, v, t = _dot(a_snap, e1), _dot(a_snap, e2), _dot(a_snap, n)
    ur, vr = u * c - v * s, v * c + u * s
    return (ur[:, None] * e1 + vr[:, None] * e2) + t[:, None] * n


def energy_of(x, v, phi, frame, center, omega):
    e = 0.5 * ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]) + phi
    if omega != 0.0:
        n = frame[0]
        d = x - center
        l = (n[0] * (d[:, 1] * v[:, 2] - d[:, 2] * v[:, 1]) + n[1] * (d[:, 2] * v[:, 0] - d[:, 0] * v[:, 2])) \
            + n[2] * (d[:, 0] * v[:, 1] - d[:, 1] * v[:, 0])
        e = e - omega * l
    return e


def orbits(sample, pos, vel, *, dt, steps, every=1, energy=False, omega=0.0, axis=(0.0, 1.0, 0.0),
           center=(0.0, 0.0, 0.0), accel_scale=1.0, step0=0, phase=phase_numpy, frame=None):
    """dict: pos, vel (R, M, 3), potential, energy (R, M), coincident (M,), step (R,).
    sample(points float32 (M, 3), potential: bool) -> (acc (M, 3), potential (M,), coincident (M,)): the field at
    the points, NaN at a non-finite one as field() has it."""
    x = np.array(pos, dtype=np.float64).reshape(-1, 3)
    v = np.array(vel, dtype=np.float64).reshape(-1, 3)
    m = x.shape[0]
    bad = ~(np.isfinite(x).all(1) & np.isfinite(v).all(1))
    x[bad], v[bad] = np.nan, np.nan
    center = np.asarray(center, dtype=np.float64)
    frame = frame if frame is not None else (map_ref.frame(axis) if omega != 0.0 else None)
    dt, scale, omega = np.float64(dt), np.float64(accel_scale), float(omega)
    h = dt / 2
    due = records(steps, every)
    out = {"pos": np.empty((len(due), m, 3)), "vel": np.empty((len(due), m, 3)),
           "potential": np.full((len(due), m), np.nan), "energy": np.full((len(due), m), np.nan),
           "coincident": np.zeros(m, np.int64), "step": np.array(due, dtype=np.uint64) + np.uint64(step0),
           "nonfinite_tracers": int(bad.sum())}
    w = None
    with np.errstate(all="ignore"):
        for k in range(steps + 1):
            c, s = phase(omega, float(dt), step0 + k)
            both = energy and k in due
            p = point(x, frame, center, omega, c, s).astype(np.float32)
            acc, pot, co = sample(p, both)
            out["coincident"] += co
            a = turn_back(scale * acc, frame, omega, c, s)
            phi = scale * pot if both else np.full(m, np.nan)
            kick = a * h
            if k > 0:
                v = w + kick
            if k in due:
                r = due.index(k)
                out["pos"][r], out["vel"][r] = x, v
                if energy:
                    out["potential"][r] = phi
                    out["energy"][r] = energy_of(x, v, phi, frame, center, omega)
            if k < steps:
                w = v + kick
                x = x + w * dt
    return out


def all_pairs64(state, g, e):
    """The binary64 all-pairs field of tests/field_ref.py as a sample callback (the potential always computed)."""
    def sample(points, potential):
        f = F.field64(state, points, g, e, potential=True)
        return f["acc"], f["potential"], f["coincident"]
    return sample


def device_field(sim):
    """The device's own field() as a sample callback: the replay the device must match bit for bit."""
    def sample(points, potential):
        f = sim.field(points, accel=True, potential=potential)
        return f.acc, f.potential, f.coincident.astype(np.int64)
    return sample


# The case the device and the restatement are both measured on: g = 1e-6, e = 1e-4 (the defaults), two bodies of mass
# 5e5 at (+-0.5, 0, 0) -- a bar-like pair of G M = 1 in all -- about the z axis through the origin, and a tracer on a
# mildly eccentric, slightly inclined orbit outside them.
CASE_G, CASE_E = 1e-6, 1e-4
CASE_X0, CASE_V0 = (1.5, 0.0, 0.1), (0.05, 1.1 / 1.5, 0.0)


def binary_state():
    s = np.zeros((2, 10), np.float32)
    s[0, 0], s[1, 0] = 0.5, -0.5
    s[:, 9] = 5e5
    return s
