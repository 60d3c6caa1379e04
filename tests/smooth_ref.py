"""The smoothed-map rule of include/nbody.h ("Smoothed maps"), restated in numpy from the header
text, twice: smooth64 walks the bodies one by one over the pixels near each (a pruned window, one pixel wider
than a search of the centres says; the rule's comparison decides), smooth64_dense forms every (body, pixel) pair
of the grid at once, in chunks of bodies, with no pruning at all.  binary64 from the binary32 state and the
binary64 s, one rounding per operation (numpy never contracts).  The frame and the edges are the map's
(tests/map_ref.py).  Used by tests/test_smooth.py (the two against each other) and tests/test_smooth_gpu.py
(parity with the device)."""
import numpy as np

from tests import map_ref as M

PLANES = ("wm", "wm_ua", "wm_ub", "wm_w", "wm_w2", "wm_u2")
K = float.fromhex("0x1.e8ec8a4aeacc4p-1")  # 3 / pi
MAX_ENTRIES = 1 << 28


def centres(lo, hi, cells):
    """0.5 (xe[i] + xe[i + 1]) of the map's edges."""
    e = M.edges(lo, hi, cells)
    return 0.5 * (e[:-1] + e[1:])


def _bodies(state, s, extent, width, height, axis, center, velocity, depth, s_min, s_max):
    """Everything the rule forms of a body before a pixel is looked at, for all n bodies (NaN-safe)."""
    state = np.asarray(state, dtype=np.float32)
    s = np.broadcast_to(np.asarray(s, dtype=np.float64), (state.shape[0],))
    x, v, m = (state[:, 0:3].astype(np.float64), state[:, 3:6].astype(np.float64), state[:, 9].astype(np.float64))
    ok = np.isfinite(x).all(1) & np.isfinite(v).all(1) & np.isfinite(m)
    nan_s = np.isnan(s)
    c, vc = np.asarray(center, dtype=np.float64), np.asarray(velocity, dtype=np.float64)
    nh, e1, e2 = M.frame(axis)
    with np.errstate(invalid="ignore", over="ignore"):
        d, u = x - c, v - vc
        a, b, h = M._dot(d, e1), M._dot(d, e2), M._dot(d, nh)
        ua, ub, w = M._dot(u, e1), M._dot(u, e2), M._dot(u, nh)
        u2 = (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]
        s_eff = np.where(s < s_min, s_min, np.where(s > s_max, s_max, s))  # (a NaN stays)
        in_slab = (h >= depth[0]) & (h < depth[1])
    valid = ok & ~nan_s
    return dict(n=state.shape[0], ok=ok, valid=valid, candidate=valid & in_slab, a=a, b=b, ua=ua, ub=ub, w=w, u2=u2,
                m=m, s_eff=s_eff, raised=valid & (s < s_min), lowered=valid & (s > s_max),
                bad_smoothing=ok & nan_s, n_hat=nh, e1=e1, e2=e2,
                xc=centres(extent[0], extent[1], width), yc=centres(extent[2], extent[3], height))


def _terms(q, i, da, db):
    """reach and the six terms of body i at the pixels (db[:, None], da[None, :])."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        r2 = (da * da)[None, :] + (db * db)[:, None]
        s2 = q["s_eff"][i] * q["s_eff"][i]
        reach = r2 < s2
        t = 1.0 - r2 / s2
        wgt = (K / s2) * (t * t)
        wm = q["m"][i] * wgt
        w = q["w"][i]
        terms = np.stack([wm, wm * q["ua"][i], wm * q["ub"][i], wm * w, (wm * w) * w, wm * q["u2"][i]])
    return reach, np.where(reach[None], terms, 0.0)


def _finish(q, counts, planes, scale, deposited, keep):
    valid, m = q["valid"], q["m"]
    out = dict(n=q["n"], nonfinite=int((~q["ok"]).sum()), bad_smoothing=int(q["bad_smoothing"].sum()),
               deposited=int(deposited.sum()), skipped=int((valid & ~deposited).sum()), raised=int(q["raised"].sum()),
               lowered=int(q["lowered"].sum()), pairs=int(counts.sum(dtype=np.uint64)), max_count=int(counts.max()),
               mass=m[q["ok"]].sum(), deposited_mass=m[deposited].sum(), mass_scale=np.abs(m[q["ok"]]).sum(),
               deposited_body=deposited, counts=counts.astype(np.uint32), planes=planes, scale=scale,
               n_hat=q["n_hat"], e1=q["e1"], e2=q["e2"], xc=q["xc"], yc=q["yc"])
    if keep is not None:
        out["reach"], out["terms"] = keep
    return out


def smooth64(state, s, width, height, extent, *, s_min, s_max, axis=(0.0, 1.0, 0.0), center=(0.0, 0.0, 0.0),
             velocity=(0.0, 0.0, 0.0), depth=(-np.inf, np.inf), keep=False):
    """state: float32[n, 10] (px py pz vx vy vz ax ay az mass); s: n lengths (or one); extent (x0, x1, y0, y1).
    Returns a dict: the integers and masses of nb_smooth_stats, `counts` (H, W), `planes` (6, H, W) and under
    `scale` the sum of |term| of every plane value (what a tolerance is relative to).  keep=True adds `reach`
    (n, H, W) and `terms` (n, 6, H, W), the single terms (small cases only)."""
    q = _bodies(state, s, extent, width, height, axis, center, velocity, depth, s_min, s_max)
    xc, yc = q["xc"], q["yc"]
    counts = np.zeros((height, width), np.int64)
    planes, scale = np.zeros((6, height, width)), np.zeros((6, height, width))
    deposited = np.zeros(q["n"], bool)
    kept = (np.zeros((q["n"], height, width), bool), np.zeros((q["n"], 6, height, width))) if keep else None
    for i in np.nonzero(q["candidate"])[0]:
        a, b, se = q["a"][i], q["b"][i], q["s_eff"][i]
        i0, i1 = max(int(np.searchsorted(xc, a - se)) - 1, 0), min(int(np.searchsorted(xc, a + se, "right")) + 1, width)
        j0, j1 = max(int(np.searchsorted(yc, b - se)) - 1, 0), min(int(np.searchsorted(yc, b + se, "right")) + 1, height)
        if i0 >= i1 or j0 >= j1:
            continue
        reach, terms = _terms(q, i, xc[i0:i1] - a, yc[j0:j1] - b)
        if not reach.any():
            continue
        deposited[i] = True
        counts[j0:j1, i0:i1] += reach
        planes[:, j0:j1, i0:i1] += terms
        scale[:, j0:j1, i0:i1] += np.abs(terms)
        if keep:
            kept[0][i, j0:j1, i0:i1] = reach
            kept[1][i, :, j0:j1, i0:i1] = terms
    return _finish(q, counts, planes, scale, deposited, kept)


def smooth64_dense(state, s, width, height, extent, *, s_min, s_max, axis=(0.0, 1.0, 0.0), center=(0.0, 0.0, 0.0),
                   velocity=(0.0, 0.0, 0.0), depth=(-np.inf, np.inf), keep=False, chunk=64):
    """The same results from every (body, pixel) pair of the grid, a chunk of bodies at a time."""
    q = _bodies(state, s, extent, width, height, axis, center, velocity, depth, s_min, s_max)
    n, xc, yc = q["n"], q["xc"], q["yc"]
    counts = np.zeros((height, width), np.int64)
    planes, scale = np.zeros((6, height, width)), np.zeros((6, height, width))
    deposited = np.zeros(n, bool)
    kept = (np.zeros((n, height, width), bool), np.zeros((n, 6, height, width))) if keep else None
    col = lambda v: v[:, None, None]  # noqa: E731
    for lo in range(0, n, chunk):
        sl = slice(lo, min(n, lo + chunk))
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            da, db = xc[None, None, :] - col(q["a"][sl]), yc[None, :, None] - col(q["b"][sl])
            r2 = da * da + db * db
            s2 = col(q["s_eff"][sl] * q["s_eff"][sl])
            reach = (r2 < s2) & col(q["candidate"][sl])
            t = 1.0 - r2 / s2
            wm = col(q["m"][sl]) * ((K / s2) * (t * t))
            w = col(q["w"][sl])
            terms = np.stack([wm, wm * col(q["ua"][sl]), wm * col(q["ub"][sl]), wm * w, (wm * w) * w,
                              wm * col(q["u2"][sl])], axis=1)
        terms = np.where(reach[:, None], terms, 0.0)
        deposited[sl] = reach.any(axis=(1, 2))
        counts += reach.sum(axis=0)
        for i in range(terms.shape[0]):  # in body order, as the loop version adds
            planes += terms[i]
            scale += np.abs(terms[i])
        if keep:
            kept[0][sl], kept[1][sl] = reach, terms
    return _finish(q, counts, planes, scale, deposited, kept)


def sampled_integral(s_pixels, offsets):
    """The sum of wgt times the pixel area over the unit pixels of a large grid, for a body at each of `offsets`
    (k, 2), in pixels from a pixel's lower corner: 1 were the kernel integrated, not point-sampled."""
    half = int(np.ceil(s_pixels)) + 2
    side = 2 * half
    offsets = np.asarray(offsets, dtype=np.float64)
    state = np.zeros((len(offsets), 10), np.float32)
    state[:, 9] = 1.0
    out = np.empty(len(offsets))
    for i, (ox, oy) in enumerate(offsets):  # the offset goes into the centre: the state stays binary32-exact
        r = smooth64(state[i:i + 1], float(s_pixels), side, side, (-half, half, -half, half), s_min=1e-6, s_max=1e6,
                     axis=(0.0, 0.0, 1.0), center=(-ox, -oy, 0.0))
        out[i] = r["planes"][0].sum()  # (unit mass, unit pixels)
    return out
