// nb_shape.hpp -- the eigen-solver of the group shapes (include/nbody.h "Group shapes"): one cyclic
// Jacobi diagonalisation of a symmetric 3 x 3 matrix, the same function on the host (nb_shape_eigen) and on the device
// (the update kernel of nb_shape.hip).  Only +, -, *, /, sqrt, fabs and comparisons: built without contraction
// (nb_shape.hip is, and the function forbids it itself) the host, the device and the restatement of
// tests/shape_ref.py return the same bits.
#pragma once

#include <cmath>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

namespace nb {

constexpr int kShapeSweeps = 12;  // at most this many sweeps over (0,1), (0,2), (1,2); 4 to 6 are taken

// t = (xx, xy, xz, yy, yz, zz).  lambda[0] >= lambda[1] >= lambda[2]; axes[3 k + j] = component j of the unit
// eigenvector of lambda[k], its component of largest magnitude (the first of equals) positive.
//   a sweep     stops the iteration when (|a01| + |a02|) + |a12| == 0 (a NaN never stops it: kShapeSweeps run);
//               else visits (p, q) = (0,1), (0,2), (1,2), r the third index
//   a visit     a_pq == 0: nothing.  g = 100 |a_pq|; |a_pp| + g == |a_pp| and |a_qq| + g == |a_qq|: a_pq <- 0,
//               nothing else.  Otherwise h = a_qq - a_pp; t = a_pq / h when |h| + g == |h|, else
//               theta = (0.5 h) / a_pq, t = 1 / (|theta| + sqrt(theta theta + 1)), negated for theta < 0;
//               c = 1 / sqrt(t t + 1), s = t c, tau = s / (1 + c), z = t a_pq;
//               a_pp <- a_pp - z, a_qq <- a_qq + z, a_pq <- 0;
//               (a_rp, a_rq) <- (a_rp - s (a_rq + tau a_rp), a_rq + s (a_rp - tau a_rq)) from the old pair, and
//               the same for (v_kp, v_kq) of every row k of V, which starts as the identity
//   afterwards  the diagonal is the eigenvalues, the columns of V the eigenvectors: sorted by value descending,
//               equal values (and NaN, which compares false) keeping their index order
__host__ __device__ inline void shape_eigen(const double t[6], double lambda[3], double axes[9]) {
#pragma clang fp contract(off)
    double a[3][3] = {{t[0], t[1], t[2]}, {t[1], t[3], t[4]}, {t[2], t[4], t[5]}};
    double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < kShapeSweeps; ++sweep) {
        const double off = (fabs(a[0][1]) + fabs(a[0][2])) + fabs(a[1][2]);
        if (off == 0.0) break;
#pragma unroll
        for (int pair = 0; pair < 3; ++pair) {  // (unrolled: p, q and r are constants, the matrices stay in registers)
            const int p = pair == 2 ? 1 : 0, q = pair == 0 ? 1 : 2, r = 3 - p - q;
            const double apq = a[p][q];
            if (apq == 0.0) continue;
            const double g = 100.0 * fabs(apq);
            if (fabs(a[p][p]) + g == fabs(a[p][p]) && fabs(a[q][q]) + g == fabs(a[q][q])) {
                a[p][q] = a[q][p] = 0.0;
                continue;
            }
            const double h = a[q][q] - a[p][p];
            double tn;
            if (fabs(h) + g == fabs(h)) {
                tn = apq / h;
            } else {
                const double theta = (0.5 * h) / apq;
                tn = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                if (theta < 0.0) tn = -tn;
            }
            const double c = 1.0 / sqrt(tn * tn + 1.0), s = tn * c, tau = s / (1.0 + c), z = tn * apq;
            a[p][p] = a[p][p] - z;
            a[q][q] = a[q][q] + z;
            a[p][q] = a[q][p] = 0.0;
            const double arp = a[r][p], arq = a[r][q];
            a[r][p] = a[p][r] = arp - s * (arq + tau * arp);
            a[r][q] = a[q][r] = arq + s * (arp - tau * arq);
            for (int k = 0; k < 3; ++k) {
                const double vp = v[k][p], vq = v[k][q];
                v[k][p] = vp - s * (vq + tau * vp);
                v[k][q] = vq + s * (vp - tau * vq);
            }
        }
    }
    // a stable insertion sort of the three (value, column) pairs, descending, the columns moved with their values: every
    // index is a constant, so nothing is addressed through a register
    double d[3] = {a[0][0], a[1][1], a[2][2]};
    auto swap_columns = [&](int i, int j) {
        const double t0 = d[i];
        d[i] = d[j];
        d[j] = t0;
        for (int k = 0; k < 3; ++k) {
            const double t1 = v[k][i];
            v[k][i] = v[k][j];
            v[k][j] = t1;
        }
    };
    if (d[1] > d[0]) swap_columns(0, 1);
    if (d[2] > d[1]) {
        swap_columns(1, 2);
        if (d[1] > d[0]) swap_columns(0, 1);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lambda[k] = d[k];
        double big = v[0][k];  // the component of largest magnitude, the first of equals
        if (fabs(v[1][k]) > fabs(big)) big = v[1][k];
        if (fabs(v[2][k]) > fabs(big)) big = v[2][k];
        const bool flip = big < 0.0;
        for (int j = 0; j < 3; ++j) axes[3 * k + j] = flip ? -v[j][k] : v[j][k];
    }
}

}  // namespace nb
