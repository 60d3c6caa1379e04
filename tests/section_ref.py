"""The section rule of include/nbody.h ("Orbit sections"), restated in numpy from the header text
around the orbit rule of tests/orbit_ref.py: binary64 +, -, x and one /, one rounding each, the comparisons < and >=
alone.  It has its own loop, because with energy=True the flags of an evaluation depend on `every` and the flags
choose the plan; the sample callback is orbit_ref's (all_pairs64 for the model, device_field for the replay)."""
import numpy as np

from tests import map_ref
from tests import orbit_ref as R

NO_STEP = np.uint64(0xFFFFFFFFFFFFFFFF)
CROSSING = np.dtype([("xi", "<f8", (3,)), ("eta", "<f8", (3,)), ("time", "<f8"), ("step", "<u8")])
SUMMARY = np.dtype([("r2_min", "<f8"), ("r2_max", "<f8"), ("R2_min", "<f8"), ("R2_max", "<f8"), ("h_max", "<f8"),
                    ("lz_min", "<f8"), ("lz_max", "<f8"), ("first_peri", "<u8"), ("last_peri", "<u8"),
                    ("pericentres", "<u4"), ("apocentres", "<u4"), ("plane_ups", "<u4"), ("winding_pattern", "<i4"),
                    ("winding_inertial", "<i4"), ("reserved", "<u4")])


def _dot(a, b):
    return (a[:, 0] * b[0] + a[:, 1] * b[1]) + a[:, 2] * b[2]


def up(y0, y1):
    return (y0 < 0.0) & (y1 >= 0.0)


def down(y0, y1):
    return (y0 >= 0.0) & (y1 < 0.0)


def frame_state(x, v, frame, center, omega, c, s, normal, offset):
    """xi, eta, s, D, L, a, b of a state."""
    n, e1, e2 = frame
    d = x - center
    a, b, l = _dot(d, e1), _dot(d, e2), _dot(d, n)
    ar, br = a * c + b * s, b * c - a * s
    u, w, t = _dot(v, e1), _dot(v, e2), _dot(v, n)
    ur, wr = u * c + w * s, w * c - u * s
    if omega != 0.0:
        eta = np.stack([ur + omega * br, wr - omega * ar, t], axis=1)
    else:
        eta = np.stack([ur, wr, t], axis=1)
    xi = np.stack([ar, br, l], axis=1)
    sv = ((normal[0] * ar + normal[1] * br) + normal[2] * l) - offset
    D = (d[:, 0] * v[:, 0] + d[:, 1] * v[:, 1]) + d[:, 2] * v[:, 2]
    L = (n[0] * (d[:, 1] * v[:, 2] - d[:, 2] * v[:, 1]) + n[1] * (d[:, 2] * v[:, 0] - d[:, 0] * v[:, 2])) \
        + n[2] * (d[:, 0] * v[:, 1] - d[:, 1] * v[:, 0])
    return dict(xi=xi, eta=eta, s=sv, D=D, L=L, a=a, b=b)


def sections(sample, pos, vel, *, dt, steps, normal=(0.0, 1.0, 0.0), offset=0.0, direction=1, max_crossings=256,
             every=None, energy=False, omega=0.0, axis=(0.0, 1.0, 0.0), center=(0.0, 0.0, 0.0), accel_scale=1.0,
             step0=0, phase=R.phase_numpy, frame=None, states=None):
    """dict: the keys of orbit_ref.orbits, and crossings (M, K) CROSSING, counts (M,), summaries (M,) SUMMARY.
    states: a list that receives (x, v, frame_state) of every state, for tests of the rule itself."""
    every = steps if every is None else every
    x = np.array(pos, dtype=np.float64).reshape(-1, 3)
    v = np.array(vel, dtype=np.float64).reshape(-1, 3)
    m = x.shape[0]
    bad = ~(np.isfinite(x).all(1) & np.isfinite(v).all(1))
    x[bad], v[bad] = np.nan, np.nan
    center = np.asarray(center, dtype=np.float64)
    frame = frame if frame is not None else map_ref.frame(axis)  # (for omega == 0 too)
    normal = np.asarray(normal, dtype=np.float64)
    dt, scale, omega, offset = np.float64(dt), np.float64(accel_scale), float(omega), np.float64(offset)
    h = dt / 2
    due = R.records(steps, every)
    out = {"pos": np.empty((len(due), m, 3)), "vel": np.empty((len(due), m, 3)),
           "potential": np.full((len(due), m), np.nan), "energy": np.full((len(due), m), np.nan),
           "coincident": np.zeros(m, np.int64), "step": np.array(due, dtype=np.uint64) + np.uint64(step0),
           "nonfinite_tracers": int(bad.sum())}
    cross = np.zeros((m, max_crossings), dtype=CROSSING)
    counts = np.zeros(m, dtype=np.uint32)
    sm = np.zeros(m, dtype=SUMMARY)
    for name in ("r2_min", "R2_min", "lz_min"):
        sm[name] = np.inf
    for name in ("r2_max", "R2_max", "lz_max", "h_max"):
        sm[name] = -np.inf
    sm["first_peri"] = sm["last_peri"] = NO_STEP
    w = prev = None
    ofr = frame if omega != 0.0 else None
    with np.errstate(all="ignore"):
        for k in range(steps + 1):
            c, s = phase(omega, float(dt), step0 + k)
            both = energy and k in due
            p = R.point(x, ofr, center, omega, c, s).astype(np.float32)
            acc, pot, co = sample(p, both)
            out["coincident"] += co
            a = R.turn_back(scale * acc, ofr, omega, c, s)
            phi = scale * pot if both else np.full(m, np.nan)
            kick = a * h
            if k > 0:
                v = w + kick
            if k in due:
                r = due.index(k)
                out["pos"][r], out["vel"][r] = x, v
                if energy:
                    out["potential"][r] = phi
                    out["energy"][r] = R.energy_of(x, v, phi, ofr, center, omega)
            # ---- the section: state k, and bracket (k - 1, k)
            cur = frame_state(x, v, frame, center, omega, c, s, normal, offset)
            if states is not None:
                states.append((x.copy(), v.copy(), cur))
            xi = cur["xi"]
            R2 = xi[:, 0] * xi[:, 0] + xi[:, 1] * xi[:, 1]
            r2 = R2 + xi[:, 2] * xi[:, 2]
            for name, y in (("r2", r2), ("R2", R2), ("lz", cur["L"])):
                lo, hi = sm[name + "_min"], sm[name + "_max"]
                sm[name + "_min"] = np.where(y < lo, y, lo)
                sm[name + "_max"] = np.where(y > hi, y, hi)
            hh = np.abs(xi[:, 2])
            sm["h_max"] = np.where(hh > sm["h_max"], hh, sm["h_max"])
            if prev is not None:
                u_, d_ = up(prev["s"], cur["s"]), down(prev["s"], cur["s"])
                fire = (u_ & (direction >= 0)) | (d_ & (direction <= 0))
                f = prev["s"] / (prev["s"] - cur["s"])
                cxi = prev["xi"] + f[:, None] * (xi - prev["xi"])
                ceta = prev["eta"] + f[:, None] * (cur["eta"] - prev["eta"])
                t = np.float64(step0 + k - 1) * dt + f * dt
                for i in np.nonzero(fire)[0]:
                    if counts[i] < max_crossings:
                        cross[i, counts[i]] = (cxi[i], ceta[i], t[i], step0 + k - 1)
                    counts[i] += 1
                peri = up(prev["D"], cur["D"])
                sm["pericentres"] += peri
                here = np.uint64(step0 + k)
                sm["first_peri"] = np.where(peri & (sm["first_peri"] == NO_STEP), here, sm["first_peri"])
                sm["last_peri"] = np.where(peri, here, sm["last_peri"])
                sm["apocentres"] += down(prev["D"], cur["D"])
                sm["plane_ups"] += up(prev["xi"][:, 2], xi[:, 2])
                for key, pa, pb, ca, cb in (("winding_pattern", prev["xi"][:, 0], prev["xi"][:, 1], xi[:, 0], xi[:, 1]),
                                            ("winding_inertial", prev["a"], prev["b"], cur["a"], cur["b"])):
                    bu, bd = up(pb, cb), down(pb, cb)
                    fb = pb / (pb - cb)
                    right = pa + fb * (ca - pa) > 0.0
                    sm[key] += (bu & right).astype(np.int32) - (bd & right).astype(np.int32)
            prev = cur
            if k < steps:
                w = v + kick
                x = x + w * dt
    out.update(crossings=cross, counts=counts, summaries=sm)
    return out


def merge(a, b):
    """nb_orbit_summary_merge on SUMMARY arrays."""
    r = np.zeros(a.shape, dtype=SUMMARY)
    for name in ("r2_min", "R2_min", "lz_min"):
        r[name] = np.minimum(a[name], b[name])
    for name in ("r2_max", "R2_max", "lz_max", "h_max"):
        r[name] = np.maximum(a[name], b[name])
    for name in ("pericentres", "apocentres", "plane_ups", "winding_pattern", "winding_inertial"):
        r[name] = a[name] + b[name]
    r["first_peri"] = np.where(a["first_peri"] != NO_STEP, a["first_peri"], b["first_peri"])
    r["last_peri"] = np.where(b["last_peri"] != NO_STEP, b["last_peri"], a["last_peri"])
    return r
