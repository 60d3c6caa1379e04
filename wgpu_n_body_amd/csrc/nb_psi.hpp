// nb_psi.hpp -- what the pair passes over the float4 SoA state share (nb_diag.hip: the pair potential of
// the whole state; nb_field.hip: the field at arbitrary points): psi, the potential of the reference's
// force law, with the constants its fp32 form needs.  (The predicate that decides which bodies count is
// nb_analysis.hpp's.)
#pragma once

#include <cmath>

#include "nb_common.hpp"

namespace nb {

struct PsiConst {
    float e;      // softening
    float a;      // e^(1/3)
    float s3a;    // sqrt(3) a
    float inv1;   // 1 / (sqrt(3) a^2)
    float inv2;   // 1 / (6 a^2)
    float near2;  // 4 a^2: below, r^3 < 8e and the closed form is used; above, the series
};

// the constants of psi_f32 for softening e >= 0, formed in fp64 and rounded once
inline PsiConst psi_const(float e) {
    PsiConst c{};
    const double a = std::cbrt((double)e);
    c.e = e;
    c.a = (float)a;
    c.s3a = (float)(std::sqrt(3.0) * a);
    c.inv1 = a > 0 ? (float)(1.0 / (std::sqrt(3.0) * a * a)) : 0.f;
    c.inv2 = a > 0 ? (float)(1.0 / (6.0 * a * a)) : 0.f;
    c.near2 = (float)(4.0 * a * a);
    return c;
}

#ifdef __HIPCC__

// psi(r) = integral_r^inf ds / (s^3 + e), fp32, from r^2.  Far branch (r^3 >= 8e, x = e/r^3 <= 1/8):
// 1/(2r^2) sum_k (-x)^k 2/(3k+2), eight terms (truncation (1/8)^8 * 2/26 < 5e-9).  Near branch: the
// closed form, whose two terms cancel by at most ~2.5x there.  fp32 error against the fp64 psi, r
// on a dense grid from 0 to 100: < 9e-7 relative, mean 8e-8.
// e = 0: near2 = 0, the far branch alone; x = 0 * inf at r = 0 is NaN and fminf keeps 1/8, so psi(0)
// = +inf as the integral is.
__device__ inline float psi_f32(float r2, const PsiConst &c) {
    const float ir = __builtin_amdgcn_rsqf(r2);
    const float ir2 = ir * ir;
    const float x = fminf(c.e * ir2 * ir, 0.125f);
    float s = 2.f / 23.f;
    s = fmaf(s, -x, 2.f / 20.f);
    s = fmaf(s, -x, 2.f / 17.f);
    s = fmaf(s, -x, 2.f / 14.f);
    s = fmaf(s, -x, 2.f / 11.f);
    s = fmaf(s, -x, 2.f / 8.f);
    s = fmaf(s, -x, 2.f / 5.f);
    s = fmaf(s, -x, 1.f);
    float psi = 0.5f * ir2 * s;
    if (r2 < c.near2) {
        const float r = sqrtf(r2);
        const float t1 = atan2f(c.s3a, 2.f * r - c.a) * c.inv1;
        const float t2 = log1pf(3.f * c.a * r / (r2 - c.a * r + c.a * c.a)) * c.inv2;
        psi = t1 - t2;
    }
    return psi;
}

#endif  // __HIPCC__

}  // namespace nb
