"""fp64 host restatement of the field probes' rule (include/nbody.h "Field probes"): the
all-pairs acceleration and potential of a state at arbitrary points, the coincident counts, and the sums
of |term| the derived error bounds are relative to.  It lives with the tests on purpose: the package has
no CPU path for it."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from tests.diag_ref import body_mask, psi64

RUN = 64                                   # R: pairs summed in fp32 before the fold into fp64
ACC_BOUND = (RUN + 16) * 2.0 ** -24        # per component, of g sum m |d_k| / (r^4 + e r)
POT_BOUND = 5e-6                           # of g sum |m| psi(r)


def _rows64(out, sl, x, m, p, g, e, potential):
    with np.errstate(all="ignore"):  # (a non-finite point is NaN throughout; field64 says so afterwards)
        d = [x[None, :, k] - p[:, None, k] for k in range(3)]
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        co = r2 == 0.0
        r2[co] = 1.0
        r = np.sqrt(r2)
        w = m[None, :] / (r2 * r2 + e * r)
        w[co] = 0.0
        out["coincident"][sl] = co.sum(axis=1)
        for k in range(3):
            t = w * d[k]
            out["acc"][sl, k] = g * t.sum(axis=1)
            out["acc_scale"][sl, k] = g * np.abs(t).sum(axis=1)
        if potential:
            t = m[None, :] * psi64(r.ravel(), e).reshape(r.shape)
            t[co] = 0.0
            out["potential"][sl] = -g * t.sum(axis=1)
            out["pot_scale"][sl] = g * np.abs(t).sum(axis=1)


def field64(state, points, g, e, potential=True, rows=None):
    """dict: acc (M, 3), potential (M,), coincident (M,), nonfinite, and the scales acc_scale (M, 3) and
    pot_scale (M,).  g and e are taken as the fp32 values the simulator holds; d = x_j - p from the fp32
    coordinates (exact in fp64); a body with d == 0 is coincident and adds nothing."""
    s = np.asarray(state, dtype=np.float32)
    ok = body_mask(s)
    x, m = s[ok, 0:3].astype(np.float64), s[ok, 9].astype(np.float64)
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    g, e = np.float64(np.float32(g)), np.float64(np.float32(e))
    M, n = p.shape[0], x.shape[0]
    out = {"acc": np.zeros((M, 3)), "potential": np.zeros(M), "coincident": np.zeros(M, np.int64),
           "acc_scale": np.zeros((M, 3)), "pot_scale": np.zeros(M), "nonfinite": int((~ok).sum())}
    rows = rows or max(1, (1 << 22) // max(n, 1))
    # (row blocks are independent and numpy releases the lock: a few threads keep the 2^20-body case short)
    with ThreadPoolExecutor(max_workers=8) as pool:
        list(pool.map(lambda i0: _rows64(out, slice(i0, i0 + rows), x, m, p[i0:i0 + rows], g, e, potential),
                      range(0, M, rows)))
    bad = ~np.isfinite(p).all(axis=1)
    for k in ("acc", "potential", "acc_scale", "pot_scale"):
        out[k][bad] = np.nan
    out["coincident"][bad] = 0
    out["nonfinite_points"] = int(bad.sum())
    return out
