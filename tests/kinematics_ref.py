"""Two independent numpy restatements of nb_local_kinematics_sim's rule (include/nbody.h "Local kinematics",
DESIGN.md 6s), on the neighbour order of tests/knn_ref.py: binary64 from the binary32 state, one rounding per
operation, every sum added in list order from its start value.

kin_vectorised -- the d2 matrix of the queried bodies against all counted ones, np.lexsort on (index, d2) per row as
                  knn_ref.knn_vectorised, then the terms of the t-th neighbour of every queried body added column
                  by column, t = 0 .. k - 1;
kin_loop       -- a plain loop per body over Python floats, the list by insertion as knn_ref.knn_loop.

Both return a KinRef; its .knn is knn_ref's own result at the same k.  derive_ref restates
nb_local_kinematics_derive step by step on whole arrays."""
from __future__ import annotations

import bisect
from dataclasses import dataclass

import numpy as np

from tests import knn_ref as K

MOMENTS, GRADS = 10, 15
SHORT, NOT_COUNTED, DEGENERATE, SINGULAR = 1, 2, 4, 8
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # xx, xy, xz, yy, yz, zz


@dataclass
class KinRef:
    k: int
    moments: np.ndarray  # (n, 10), S0 as include_self says
    grads: np.ndarray    # (n, 15)
    s0_self: np.ndarray    # (n,): S0 started from the body's own mass ...
    s0_noself: np.ndarray  # ... and from 0
    knn: K.KnnRef
    counted: int
    degenerate: int
    short_of_k: int


def _start(pos, mass, vel, k):
    pos, mass, vel = np.asarray(pos, np.float32), np.asarray(mass, np.float32), np.asarray(vel, np.float32)
    ok = K.counted_mask(pos, mass, vel)
    n = pos.shape[0]
    mom, gr = np.full((n, MOMENTS), np.nan), np.full((n, GRADS), np.nan)
    mom[ok], gr[ok] = 0.0, 0.0
    return pos, mass, vel, ok, mom, gr


def _finish(k, mom, gr, s0, knn, ok, include_self):
    c = int(ok.sum())
    deg = int(np.count_nonzero(ok & (knn.r2 == 0.0))) if c > k else 0
    if s0 is None:  # short of k: every sum 0
        s0 = np.stack([mom[:, 0], mom[:, 0]])
    mom[:, 0] = s0[0] if include_self else s0[1]
    return KinRef(k, mom, gr, s0[0], s0[1], knn, c, deg, c if c <= k else 0)


def kin_vectorised(pos, mass, vel, k: int, include_self: bool = True, queries=None, rows: int = 256) -> KinRef:
    pos, mass, vel, ok, mom, gr = _start(pos, mass, vel, k)
    knn = K.knn_vectorised(pos, mass, vel, k, queries=queries, rows=rows)
    if int(ok.sum()) <= k:
        return _finish(k, mom, gr, None, knn, ok, include_self)
    s0 = np.stack([mom[:, 0], mom[:, 0]])
    idx = np.nonzero(ok)[0]
    place = np.full(pos.shape[0], -1, dtype=np.int64)
    place[idx] = np.arange(idx.size)
    x, v, m = pos[idx].astype(np.float64), vel[idx].astype(np.float64), mass[idx].astype(np.float64)
    qs = idx if queries is None else np.array([q for q in np.asarray(queries, dtype=np.int64) if ok[q]], dtype=np.int64)
    if queries is not None:  # bodies that were not asked for are not stated
        rest = np.setdiff1d(idx, qs)
        mom[rest], gr[rest], s0[:, rest] = np.nan, np.nan, np.nan
    for lo in range(0, qs.size, rows):
        q = qs[lo:lo + rows]
        pq = place[q]
        dxm, dym, dzm = (x[pq][:, None, a] - x[None, :, a] for a in range(3))
        d2 = (dxm * dxm + dym * dym) + dzm * dzm
        d2[np.arange(q.size), pq] = np.inf
        kd = np.partition(d2, k - 1, axis=-1)[:, k - 1]
        order = np.empty((q.size, k), dtype=np.int64)
        for t, row in enumerate(d2):
            cand = np.nonzero(row <= kd[t])[0]
            order[t] = cand[np.lexsort((cand, row[cand]))[:k]]
        a_m = np.zeros((q.size, MOMENTS))
        a_g = np.zeros((q.size, GRADS))
        a_self = m[pq].copy()
        for t in range(k):
            j = order[:, t]
            mj = m[j]
            du = v[j] - v[pq]
            dx = x[j] - x[pq]
            mu = mj[:, None] * du
            md = mj[:, None] * dx
            a_m[:, 0] = a_m[:, 0] + mj
            a_self = a_self + mj
            a_m[:, 1:4] = a_m[:, 1:4] + mu
            for f, (a, b) in enumerate(PAIRS):
                a_m[:, 4 + f] = a_m[:, 4 + f] + mu[:, a] * du[:, b]
                a_g[:, f] = a_g[:, f] + md[:, a] * dx[:, b]
            for a in range(3):
                for b in range(3):
                    a_g[:, 6 + 3 * a + b] = a_g[:, 6 + 3 * a + b] + mu[:, a] * dx[:, b]
        mom[q], gr[q] = a_m, a_g
        s0[0, q], s0[1, q] = a_self, a_m[:, 0]
    return _finish(k, mom, gr, s0, knn, ok, include_self)


def kin_loop(pos, mass, vel, k: int, include_self: bool = True) -> KinRef:
    pos, mass, vel, ok, mom, gr = _start(pos, mass, vel, k)
    knn = K.knn_loop(pos, mass, vel, k)
    if int(ok.sum()) <= k:
        return _finish(k, mom, gr, None, knn, ok, include_self)
    s0 = np.stack([mom[:, 0], mom[:, 0]])
    n = pos.shape[0]
    bodies = [int(i) for i in np.nonzero(ok)[0]]
    xs = [[float(pos[i, a]) for a in range(3)] for i in range(n)]
    vs = [[float(vel[i, a]) for a in range(3)] for i in range(n)]
    ms = [float(mass[i]) for i in range(n)]
    for i in bodies:
        best = []
        xi, vi = xs[i], vs[i]
        for j in bodies:
            if j == i:
                continue
            dx, dy, dz = xi[0] - xs[j][0], xi[1] - xs[j][1], xi[2] - xs[j][2]
            e = ((dx * dx + dy * dy) + dz * dz, j)
            if len(best) < k or e < best[-1]:
                bisect.insort(best, e)
                del best[k:]
        s = [0.0] * MOMENTS
        g = [0.0] * GRADS
        with_self = ms[i]
        for _, j in best:
            mj = ms[j]
            du = [vs[j][a] - vi[a] for a in range(3)]
            dx = [xs[j][a] - xi[a] for a in range(3)]
            s[0] += mj
            with_self += mj
            for a in range(3):
                s[1 + a] += mj * du[a]
            for f, (a, b) in enumerate(PAIRS):
                s[4 + f] += (mj * du[a]) * du[b]
                g[f] += (mj * dx[a]) * dx[b]
            for a in range(3):
                for b in range(3):
                    g[6 + 3 * a + b] += (mj * du[a]) * dx[b]
        mom[i], gr[i] = s, g
        s0[0, i], s0[1, i] = with_self, s[0]
    return _finish(k, mom, gr, s0, knn, ok, include_self)


def derive_ref(moments, grads, r2, density, vel):
    """nb_local_kinematics_derive on whole arrays, each step as the header writes it; a dict of arrays."""
    s = np.asarray(moments, np.float64)
    n = s.shape[0]
    r2 = np.asarray(r2, np.float64)
    status = np.where(np.isnan(r2), NOT_COUNTED, np.where(np.isinf(r2), SHORT, np.where(r2 == 0.0, DEGENERATE, 0)))
    status = status.astype(np.uint32)
    live = (status & (NOT_COUNTED | SHORT)) == 0
    out = {}
    with np.errstate(all="ignore"):
        u = s[:, 1:4] / s[:, 0:1]
        disp = np.stack([s[:, 4 + f] / s[:, 0] - u[:, a] * u[:, b] for f, (a, b) in enumerate(PAIRS)], axis=1)
        sigma2 = ((disp[:, 0] + disp[:, 3]) + disp[:, 5]) / 3.0
        sigma = np.where(sigma2 < 0.0, 0.0, np.sqrt(np.where(sigma2 < 0.0, 0.0, sigma2)))
        out["mass"] = s[:, 0].copy()
        out["relative_velocity"] = u
        out["mean_velocity"] = (np.asarray(vel, np.float32).astype(np.float64) + u if vel is not None
                                else np.full((n, 3), np.nan))
        out["dispersion"], out["sigma2"], out["sigma"] = disp, sigma2, sigma
        out["phase_space_density"] = (np.asarray(density, np.float64) / (sigma2 * sigma) if density is not None
                                      else np.full(n, np.nan))
        grad = np.full((n, 9), np.nan)
        det = np.full(n, np.nan)
        if grads is not None:
            g = np.asarray(grads, np.float64)
            xx, xy, xz, yy, yz, zz = (g[:, f] for f in range(6))
            c = g[:, 6:15].reshape(n, 3, 3)
            adj = np.empty((n, 3, 3))
            adj[:, 0, 0] = yy * zz - yz * yz
            adj[:, 0, 1] = adj[:, 1, 0] = xz * yz - xy * zz
            adj[:, 0, 2] = adj[:, 2, 0] = xy * yz - xz * yy
            adj[:, 1, 1] = xx * zz - xz * xz
            adj[:, 1, 2] = adj[:, 2, 1] = xy * xz - xx * yz
            adj[:, 2, 2] = xx * yy - xy * xy
            det = (xx * adj[:, 0, 0] + xy * adj[:, 0, 1]) + xz * adj[:, 0, 2]
            singular = live & ~(det > 2.0 ** -30 * ((xx * yy) * zz))
            status = status | np.where(singular, SINGULAR, 0).astype(np.uint32)
            for a in range(3):
                for b in range(3):
                    grad[:, 3 * a + b] = ((c[:, a, 0] * adj[:, 0, b] + c[:, a, 1] * adj[:, 1, b])
                                          + c[:, a, 2] * adj[:, 2, b]) / det
            grad[singular] = np.nan
        G = grad
        div = (G[:, 0] + G[:, 4]) + G[:, 8]
        t = div / 3.0
        sxx, syy, szz = G[:, 0] - t, G[:, 4] - t, G[:, 8] - t
        sxy, sxz, syz = (G[:, 1] + G[:, 3]) / 2.0, (G[:, 2] + G[:, 6]) / 2.0, (G[:, 5] + G[:, 7]) / 2.0
        out["gradient"], out["det"], out["divergence"] = G, det, div
        out["vorticity"] = np.stack([G[:, 7] - G[:, 5], G[:, 2] - G[:, 6], G[:, 3] - G[:, 1]], axis=1)
        out["shear"] = np.sqrt(((sxx * sxx + syy * syy) + szz * szz) + 2.0 * ((sxy * sxy + sxz * sxz) + syz * syz))
    for name, a in out.items():
        if name != "mass":
            a[~live] = np.nan
    out["status"] = status
    return out


def solve_bound(grads, c_const):
    """Per body: the reference gradient of numpy.linalg.solve (G D = C, D symmetric) and the bound
    c kappa(D) 2^-53 ||G|| on its distance to the cofactor solution."""
    g = np.asarray(grads, np.float64)
    n = g.shape[0]
    D = np.empty((n, 3, 3))
    for f, (a, b) in enumerate(PAIRS):
        D[:, a, b] = D[:, b, a] = g[:, f]
    Cm = g[:, 6:15].reshape(n, 3, 3)
    G = np.linalg.solve(D, np.swapaxes(Cm, 1, 2))  # D G^T = C^T
    G = np.swapaxes(G, 1, 2)
    kappa = np.linalg.cond(D)
    norm = np.linalg.norm(G.reshape(n, 9), axis=1)
    return G.reshape(n, 9), c_const * kappa * 2.0 ** -53 * norm, kappa


# ---- the two states with a known answer (tests/test_kinematics.py checks them on the restatement, without a
# device; tests/test_kinematics_gpu.py on the device) ---------------------------------------------------------
SOLVE_C = 4 * 2.6  # the cofactor solve against numpy.linalg.solve, measured 2.6, four times that


def linear_flow_state():
    """4,096 positions on a 2^-12 lattice in the unit cube, masses from {0.5, 1, 2}, v = A x + v0 with A's entries
    multiples of 1/4 in [-2, 2]: every term and every sum of the rule is exact in binary64."""
    rng = np.random.default_rng(12)
    pos = rng.integers(0, 4096, (4096, 3)) / 4096.0
    A = rng.integers(-8, 9, (3, 3)) / 4.0
    v0 = np.array([0.25, -1.5, 3.0])
    s = np.zeros((4096, 10), np.float32)
    s[:, 0:3] = pos
    s[:, 3:6] = pos @ A.T + v0
    s[:, 9] = rng.choice([0.5, 1.0, 2.0], 4096)
    assert np.array_equal(s[:, 3:6].astype(np.float64), pos @ A.T + v0)  # binary32 holds them
    return s, A


def check_linear_flow(moments, grads, A, derived):
    """C = A D and S2 = A C^T exactly (so Sigma differs from the spread A (D / S0 - xbar xbar^T) A^T by the derive
    step's own roundings alone); G equals A within the derive bound wherever the status is not singular, which is
    all but fewer than 1 % of the bodies; divergence and vorticity follow."""
    n = moments.shape[0]
    D, S2 = np.empty((n, 3, 3)), np.empty((n, 3, 3))
    for f, (a, b) in enumerate(PAIRS):
        D[:, a, b] = D[:, b, a] = grads[:, f]
        S2[:, a, b] = S2[:, b, a] = moments[:, 4 + f]
    Cm = grads[:, 6:15].reshape(n, 3, 3)
    assert np.array_equal(Cm, np.einsum("ab,nbc->nac", A, D))
    assert np.array_equal(S2, np.einsum("ab,ncb->nac", A, Cm))
    live = (derived["status"] & SINGULAR) == 0
    assert np.count_nonzero(~live) < 0.01 * n, np.count_nonzero(~live)
    G = derived["gradient"][live].reshape(-1, 3, 3)
    _, bound, _ = solve_bound(grads[live], SOLVE_C)
    err = np.linalg.norm((G - A).reshape(-1, 9), axis=1)
    print("linear flow: worst error / bound", (err / bound).max(), "singular", np.count_nonzero(~live))
    assert np.all(err <= bound)
    tol = 3.0 * bound  # a sum or difference of at most three entries of G
    assert np.all(np.abs(derived["divergence"][live] - np.trace(A)) <= tol)
    w = np.array([A[2, 1] - A[1, 2], A[0, 2] - A[2, 0], A[1, 0] - A[0, 1]])
    assert np.all(np.abs(derived["vorticity"][live] - w) <= tol[:, None])


def clump_state():
    """The hot `spherical` sphere of 4,096 bodies (unit radius, every speed 0.4: 0.231 per axis), 256 of which are
    made a compact cold clump beside it: a ball of radius (256 / 4096)^(1/3) about (1.6, 0, 0), which gives it the
    sphere's own density, at rest, with a dispersion of 1/100 of the sphere's per axis.  Returns the state and the
    clump's bodies.  On the restatement at k = 32 (tests/test_kinematics.py): median sigma 0.0022 in the clump against
    0.040 in the sphere (its velocity field is coherent, so its local sigma is below its global one), median Q 1.1e11
    against 2.3e7, median density 1,231 against 1,619."""
    from tests.helpers import make_state
    state = make_state("spherical", 4096, seed=3)
    rng = np.random.default_rng(3)
    clump = np.sort(rng.choice(4096, 256, replace=False))
    sigma = float(state[:, 3:6].astype(np.float64).std())
    state[clump, 0:3] = K.ball(rng, 256, (256.0 / 4096.0) ** (1.0 / 3.0), (1.6, 0.0, 0.0))
    state[clump, 3:6] = rng.normal(0.0, sigma / 100.0, (256, 3))
    return state, clump


def check_clump(sigma, q, density, clump):
    """The clump is no denser than the sphere -- the two median densities are within a factor of 3 -- but its median
    sigma is below a tenth of the sphere's and its median Q more than 100 times above it."""
    back = np.setdiff1d(np.arange(sigma.size), clump)
    s_c, s_b = np.median(sigma[clump]), np.median(sigma[back])
    q_c, q_b = np.median(q[clump]), np.median(q[back])
    r_c, r_b = np.median(density[clump]), np.median(density[back])
    print(f"sigma {s_c:.4g} / {s_b:.4g}  Q {q_c:.4g} / {q_b:.4g}  density {r_c:.4g} / {r_b:.4g}")
    assert s_c < 0.1 * s_b and q_c > 100.0 * q_b and 1.0 / 3.0 < r_c / r_b < 3.0
